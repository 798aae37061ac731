// env_common.hpp -- float64 helpers shared by the env-step kernels (reference operation order, no contraction).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"

namespace mcn {

// XCD-aware chunking: the index of the run of envs that workgroup blockIdx.x of a 1-D grid works on.  Workgroups are
// dealt round-robin over the 8 XCDs (b and b + 8 share one), each with a private L2, and a workgroup's envs cover only
// part of a cache line of the per-env arrays (3 envs x 16 B in the quad kernels at 5 humans; the u8 done / info and i32
// counters of the step kernel straddle neighbouring workgroups).  Giving every XCD one contiguous range of chunks keeps
// such a line inside ONE L2 instead of fetching it into, and writing it back partially from, two or three.  Bijective
// for any grid size.
__device__ __forceinline__ unsigned xcd_chunk()
{
    const unsigned nb = gridDim.x, xcd = blockIdx.x & 7u, idx = blockIdx.x >> 3;
    const unsigned qq = nb >> 3, rr = nb & 7u;            // the first rr XCDs hold qq + 1 chunks, the others qq
    return (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
}

__device__ __forceinline__ double norm2(double x0, double x1) { return sqrt(fma(x1, x1, x0 * x0)); }

// crowd_sim/envs/utils/utils.py:4-26 with (x3, y3) = (0, 0), the env's only call shape
__device__ __forceinline__ double p2s_origin(double x1, double y1, double x2, double y2)
{
    // Branch-free form with identical results: for a degenerate segment (px == py == 0) the reference returns
    // norm((0 - x1, 0 - y1)); with u forced to 0 the general formula gives norm((x1 + 0*0, y1 + 0*0)) -- the same
    // two squares under one fma and one sqrt.  Keeping one straight-line block lets the scheduler interleave this
    // long float64 dependency chain with the other independent ones around it.
    const double px = x2 - x1, py = y2 - y1;
    const bool degenerate = (px == 0) & (py == 0);
    double u = ((0.0 - x1) * px + (0.0 - y1) * py) / (px * px + py * py);
    u = degenerate ? 0.0 : u;
    if (u > 1) u = 1; else if (u < 0) u = 0;
    const double x = x1 + u * px, y = y1 + u * py;
    return norm2(x - 0.0, y - 0.0);
}

// One env's step record as two stores (16 + 8 bytes): assigning the struct member-wise makes the compiler emit
// separate byte / short / dword stores for done, info, padding and hh_count.
__device__ __forceinline__ void store_step_rec(mcn_step_rec *dst, double reward, double dmin, int done, int info, int hh)
{
    double *d = reinterpret_cast<double *>(dst);
    const unsigned long long tail = (unsigned long long)(unsigned)(done & 0xff) | ((unsigned long long)(unsigned)(info & 0xff) << 8) |
                                    ((unsigned long long)(unsigned)hh << 32);      // little-endian layout of mcn_step_rec
    reinterpret_cast<double2 *>(d)[0] = make_double2(reward, dmin);
    reinterpret_cast<unsigned long long *>(d)[2] = tail;
}

// Python's float % for a positive divisor: a negative remainder moves up by m, a zero one is +0.0 (copysign(0, m)),
// also when fmod returns -0.0 (a == -0.0 or a negative multiple of m)
__device__ __forceinline__ double pymod(double a, double m)
{
    double r = fmod(a, m);
    if (r < 0) r += m;
    return r == 0 ? 0.0 : r;
}

// ---- the step's tail, memory-resident form: env_step_body uses all four pieces, env_step_quad_kernel all but the
// accounting (written out there, for its SGPR spills).  env_pair_kernel keeps its own text throughout: ladder and pool
// restart written out, the accounting on the packed record, the robot stores as 16-byte pieces.
// The rollout kernels that keep the state in registers across steps (env_rollout_quad.hip, env_rollout_wg4.hip) hold
// their own text of the same contract: see the TWIN comments there.

// crowd_sim.py:379-403: timeout, collision, goal, discomfort, nothing -- in this order
__device__ __forceinline__ void reward_ladder(const mcn_env_cfg &c, double gtime, double dmin, bool reaching, double dt,
                                              double &rew, int &dn, int &inf)
{
    if (gtime >= c.time_limit - 1)      { rew = 0; dn = 1; inf = MCN_INFO_TIMEOUT; }
    else if (dmin < 0)                  { rew = c.collision_penalty; dn = 1; inf = MCN_INFO_COLLISION; }
    else if (reaching)                  { rew = c.success_reward; dn = 1; inf = MCN_INFO_REACHGOAL; }
    else if (dmin < c.discomfort_dist)  { rew = (dmin - c.discomfort_dist) * c.discomfort_penalty_factor * dt; dn = 0; inf = MCN_INFO_DANGER; }
    else                                { rew = 0; dn = 0; inf = MCN_INFO_NOTHING; }
}

// human a of a finished env starts again as human pa of the scenario pool (at rest where the pool holds no velocities)
__device__ __forceinline__ void restart_human_from_pool(const mcn_env_state &st, const mcn_rollout &ro, long a, long pa)
{
    reinterpret_cast<double2 *>(st.hpos)[a]  = reinterpret_cast<const double2 *>(ro.pool_hpos)[pa];
    reinterpret_cast<double2 *>(st.hgoal)[a] = reinterpret_cast<const double2 *>(ro.pool_hgoal)[pa];
    st.hrad[a] = ro.pool_hrad[pa];
    st.hvpref[a] = ro.pool_hvpref[pa];
    reinterpret_cast<double2 *>(st.hvel)[a]  = ro.pool_hvel
        ? reinterpret_cast<const double2 *>(ro.pool_hvel)[pa] : make_double2(0, 0);
    if (st.human_times) st.human_times[a] = 0;
}

// Explorer accounting of env e's step (explorer.py:88-99,124; include/mcn.h: mcn_rollout) on its record rs, loaded by
// the caller with next_case and the discount factor ep_disc of rs.ep_steps; ro.state is not NULL.  E: envs of the batch.
__device__ __forceinline__ void explorer_account(const mcn_env_cfg &c, const mcn_rollout &ro, mcn_roll_rec &rs, long e, int E,
                                                 int next_case, double ep_disc, double rew, double dmin, int dn, int inf,
                                                 double t_new, bool do_reset)
{
    if (inf == MCN_INFO_DANGER && (ro.danger_episodes <= 0 ||
        rs.fin_count < ro.danger_episodes - ((ro.danger_short_from > 0 && e >= ro.danger_short_from - 1) ? 1 : 0))) {
        rs.danger_count += 1; rs.danger_dist_sum += dmin;
    }
    const double ret = rs.ep_return + ep_disc * rew;
    if (dn) {
        const int k = rs.fin_count;
        // fin_slots == 1: keep the latest episode; otherwise keep the first fin_slots episodes
        const bool keep = (ro.fin_slots == 1) || (k < ro.fin_slots);
        const long rec = (long)(ro.fin_slots == 1 ? 0 : k) * E + e;
        if (keep && ro.fin_return) ro.fin_return[rec] = ret;
        if (keep && ro.fin_time)   ro.fin_time[rec] = (inf == MCN_INFO_TIMEOUT) ? c.time_limit : t_new;
        if (keep && ro.fin_info)   ro.fin_info[rec] = (uint8_t)inf;
        rs.fin_count = k + 1; rs.ep_return = 0; rs.ep_steps = 0;
        if (do_reset) {                          // both < pool_size (validated on the host): no division
            const int nc = next_case + ro.case_stride;
            rs.next_case = nc >= ro.pool_size ? nc - ro.pool_size : nc;
        }
    } else {
        rs.ep_return = ret; rs.ep_steps += 1;
    }
    ro.state[e] = rs;                            // one 32-byte store
}

// env e's robot and clock after the step: back at the start when the env restarts (restart_robot), else at the end
// pose of its action (store_robot).  Two functions and the branch at the caller: as one function that takes the
// condition, env_step_kernel<64, 7, 0, ORCA, 2> spills six more SGPRs and goes from 128 to 129 VGPRs
// (profiles/r19_env_refactor.txt).
__device__ __forceinline__ void restart_robot(const mcn_env_state &st, const mcn_rollout &ro, long e)
{
    reinterpret_cast<double2 *>(st.rpos)[e]  = make_double2(ro.robot_start[0], ro.robot_start[1]);
    reinterpret_cast<double2 *>(st.rgoal)[e] = make_double2(ro.robot_goal[0], ro.robot_goal[1]);
    reinterpret_cast<double2 *>(st.rvel)[e]  = make_double2(0, 0);
    if (st.rtheta) st.rtheta[e] = ro.robot_theta0;
    st.gtime[e] = 0;
}
__device__ __forceinline__ void store_robot(const mcn_env_cfg &c, const mcn_env_state &st, long e, double endx, double endy,
                                            double nrvx, double nrvy, double new_theta, double t_new)
{
    reinterpret_cast<double2 *>(st.rpos)[e] = make_double2(endx, endy);
    reinterpret_cast<double2 *>(st.rvel)[e] = make_double2(nrvx, nrvy);
    if (c.robot_kinematics == MCN_KIN_UNICYCLE) st.rtheta[e] = new_theta;
    st.gtime[e] = t_new;
}

}  // namespace mcn
