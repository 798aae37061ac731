// lookahead_common.hpp -- what the one-step look-ahead kernels (sarl_value.hip, lstm_rl_value.hip) do around their
// networks, once: per (env, action) pair the robot after the candidate action (cadrl.py:104-129), the rotation into the
// 13 agent-centric features (cadrl.py:217-252), compute_reward (multi_human_rl.py:65-88) and
// value = reward + gamma^(dt * v_pref) * V (multi_human_rl.py:52).  float64 where the reference computes in Python
// floats, float32 where it has made a torch.Tensor; the operation order is the reference's and must stay the same in
// every kernel, which is why it is here.
//
// Form: free functions over small aggregates that are passed and returned BY VALUE.  One struct with member functions
// that lives across a kernel's pair loop stayed in scratch in the LSTM-RL kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "mfma_chain.hpp"
#include "fast_f32.hpp"

namespace mcn {

// kernel parameters every look-ahead shares (state: the buffers of mcn_env_state)
struct PairParams {
    const double *rpos, *rvel, *rgoal, *rrad, *rvpref, *rtheta;   // [E][2] / [E]
    const double *hpos, *hvel, *hrad;                             // [E*N][2] / [E*N]
    const int32_t *hcount;                                        // [E] or NULL: humans the policy sees
    // query_env = true (multi_human_rl.py:37-38): the humans' next states and the rewards come from the env's own
    // one-step look-ahead instead of constant-velocity propagation + compute_reward; all three NULL otherwise
    const double *next_hpos, *next_hvel;                          // [E*N][2]
    const double *reward_in;                                      // [E*A]
    const double *actions;                                        // [A][2]
    double *values;                                               // [E*A]
    long ngroups;                                                 // workgroup passes: ceil(16-pair tiles / waves per workgroup)
    int E, N, A, kinematics;
    double dt, gamma_pow;
};

inline PairParams pair_params(const mcn_env_state *st, const double *actions, int A, double dt, double gamma_pow,
                              int kinematics, double *values, const double *next_hpos, const double *next_hvel,
                              const double *reward_in, int E, int N, int waves_per_group)
{
    PairParams c;
    c.rpos = st->rpos; c.rvel = st->rvel; c.rgoal = st->rgoal; c.rrad = st->rrad; c.rvpref = st->rvpref; c.rtheta = st->rtheta;
    c.hpos = st->hpos; c.hvel = st->hvel; c.hrad = st->hrad; c.hcount = st->hcount;
    c.next_hpos = next_hpos; c.next_hvel = next_hvel; c.reward_in = reward_in;
    c.actions = actions; c.values = values;
    c.E = E; c.N = N; c.A = A; c.kinematics = kinematics; c.dt = dt; c.gamma_pow = gamma_pow;
    const long tiles = ((long)E * A + 15) / 16;
    c.ngroups = (tiles + waves_per_group - 1) / waves_per_group;
    return c;
}

__device__ __forceinline__ double norm2d(double x0, double x1) { return sqrt(fma(x1, x1, x0 * x0)); }

// pedestrians env e shows to the policy: hcount[e] clamped to 1 .. N, N without the table
__device__ __forceinline__ int humans_seen(const int32_t *hcount, long e, int N)
{
    int ne = N;
    if (hcount) { ne = hcount[e]; ne = ne < 1 ? 1 : (ne > N ? N : ne); }
    return ne;
}

// robot after the candidate action (cadrl.py:104-129), float64 like the reference
struct RobotNext { double px, py, vx, vy, th; };
__device__ __forceinline__ RobotNext robot_after(const PairParams &c, int e, int a, const double2 rp)
{
    const double2 ac = reinterpret_cast<const double2 *>(c.actions)[a];
    RobotNext r;
    if (c.kinematics == MCN_KIN_UNICYCLE) {
        r.th = c.rtheta[e] + ac.y;
        r.vx = ac.x * cos(r.th); r.vy = ac.x * sin(r.th);
        r.px = rp.x + r.vx * c.dt; r.py = rp.y + r.vy * c.dt;
    } else {
        r.th = c.rtheta ? c.rtheta[e] : 0.0;
        r.vx = ac.x; r.vy = ac.y;
        r.px = rp.x + ac.x * c.dt; r.py = rp.y + ac.y * c.dt;
    }
    return r;
}

// self part of the rotated state (cadrl.py:223-240), float32 like torch.Tensor(...): the six self features, and what
// the humans' features are rotated with
struct SelfFeatures {
    float px, py, cr, sr;                       // position; cos / sin of rot = atan2(goal - position)
    float dg, vpref, theta, rad, vx, vy;        // features 0 .. 5
};
__device__ __forceinline__ SelfFeatures self_features(const RobotNext r, const double2 rg, const double2 ra, int kinematics)
{
    SelfFeatures s;
    s.px = (float)r.px; s.py = (float)r.py;
    const float svx = (float)r.vx, svy = (float)r.vy;
    s.rad = (float)ra.x;
    const float sgx = (float)rg.x, sgy = (float)rg.y;
    s.vpref = (float)ra.y;
    const float gdx = sgx - s.px, gdy = sgy - s.py;
    s.dg = sqrtf(gdx * gdx + gdy * gdy);
    // cos/sin of rot = atan2(gdy, gdx) without the round trip through the angle
    s.cr = s.dg > 0.0f ? gdx / s.dg : 1.0f;
    s.sr = s.dg > 0.0f ? gdy / s.dg : 0.0f;
    s.theta = (kinematics == MCN_KIN_UNICYCLE) ? ((float)r.th - atan2f(gdy, gdx)) : 0.0f;
    s.vx = svx * s.cr + svy * s.sr;
    s.vy = svy * s.cr - svx * s.sr;
    return s;
}

// the 6 self features as an input tile packed "q first": feature j sits in register j/4 of lane group j%4 (two k-steps)
__device__ __forceinline__ f32x4 self_tile(const SelfFeatures s, int q)
{
    const float s0 = q == 0 ? s.dg : (q == 1 ? s.vpref : (q == 2 ? s.theta : s.rad));
    const float s1 = q == 0 ? s.vx : (q == 1 ? s.vy : 0.0f);
    return (f32x4){s0, s1, 0.0f, 0.0f};
}

// Human ha = e * N + i after propagation (constant velocity, or the env's look-ahead states): its 13 features as the B
// operand tile (register r of lane group q carries feature 4q + r), and whether any of them is not finite (SARL's
// `poisoned`; it folds away in the callers that drop it).  A human the policy sees (`seen`) also enters dmin, the
// reward's smallest distance to the robot (multi_human_rl.py:70) -- here, before the float32 part, and not at the
// caller's: taken after the call it cost the LSTM-RL and CADRL kernels two registers.
struct HumanTile { f32x4 x; bool nonfinite; };
__device__ __forceinline__ HumanTile human_tile(const PairParams &c, long ha, const RobotNext r, double rrad,
                                                const SelfFeatures s, int q, bool seen, double &dmin)
{
    const double2 hp = reinterpret_cast<const double2 *>(c.hpos)[ha];
    const double2 hv = reinterpret_cast<const double2 *>(c.hvel)[ha];
    const double hr = c.hrad[ha];
    double qx = hp.x + hv.x * c.dt, qy = hp.y + hv.y * c.dt;            // constant-velocity propagate
    double nhvx = hv.x, nhvy = hv.y;
    if (c.next_hpos) {                                                  // the env's look-ahead states instead
        const double2 np_ = reinterpret_cast<const double2 *>(c.next_hpos)[ha];
        const double2 nv_ = reinterpret_cast<const double2 *>(c.next_hvel)[ha];
        qx = np_.x; qy = np_.y; nhvx = nv_.x; nhvy = nv_.y;
    }
    const double d = norm2d(r.px - qx, r.py - qy) - rrad - hr;
    dmin = seen ? fmin(dmin, d) : dmin;
    const float hx = (float)qx, hy = (float)qy, hvx = (float)nhvx, hvy = (float)nhvy, hrad = (float)hr;
    const float ox = hx - s.px, oy = hy - s.py;
    float feat[16];
    feat[0] = s.dg; feat[1] = s.vpref; feat[2] = s.theta; feat[3] = s.rad; feat[4] = s.vx; feat[5] = s.vy;
    feat[6] = ox * s.cr + oy * s.sr;
    feat[7] = oy * s.cr - ox * s.sr;
    feat[8] = hvx * s.cr + hvy * s.sr;
    feat[9] = hvy * s.cr - hvx * s.sr;
    feat[10] = hrad;
    { const float ax_ = s.px - hx, ay_ = s.py - hy; feat[11] = sqrt_f32(ax_ * ax_ + ay_ * ay_); }   // == sqrtf (fast_f32.hpp)
    feat[12] = s.rad + hrad;
    feat[13] = feat[14] = feat[15] = 0.0f;
    HumanTile h;
    float z = 0.0f;                             // +-0 while every feature is finite, NaN otherwise (0 * inf, 0 * NaN)
#pragma unroll
    for (int k = 0; k < 13; ++k) z = z + feat[k] * 0.0f;
    h.nonfinite = z != z;
#pragma unroll
    for (int k = 0; k < 4; ++k) h.x[k] = q == 0 ? feat[k] : (q == 1 ? feat[4 + k] : (q == 2 ? feat[8 + k] : feat[12 + k]));
    return h;
}

// reward ladder of MultiHumanRL.compute_reward with its hard-coded constants; reward_in overrides it
__device__ __forceinline__ double pair_reward(const PairParams &c, const RobotNext r, const double2 rg, double rrad,
                                              double dmin, long pair)
{
    const bool reach = norm2d(r.px - rg.x, r.py - rg.y) < rrad;
    double reward;
    if (dmin < 0) reward = -0.25;
    else if (reach) reward = 1;
    else if (dmin < 0.2) reward = (dmin - 0.2) * 0.5 * c.dt;
    else reward = 0;
    if (c.reward_in) reward = c.reward_in[pair];
    return reward;
}

// value = reward + gamma^(dt * v_pref) * V   (multi_human_rl.py:52, Python float arithmetic)
__device__ __forceinline__ double pair_value(const PairParams &c, double reward, float V) { return reward + c.gamma_pow * (double)V; }

}  // namespace mcn
