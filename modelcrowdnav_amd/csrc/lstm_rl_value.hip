// lstm_rl_value.hip -- LSTM-RL and CADRL 81-action one-step look-ahead, fused, for gfx950 (MI355X).
//
// Replaces, per environment and candidate action, the look-ahead loop of
//   LstmRL.predict   (crowd_nav/policy/lstm_rl.py:90-103 -> multi_human_rl.py:35-55): humans sorted by decreasing
//                    distance to the robot, ValueNetwork1.forward (lstm_rl.py:9-33: LSTM over the humans from
//                    h = c = 0, then mlp on [self features | h]);
//   CADRL.predict    (crowd_nav/policy/cadrl.py:131-178): the value network on every (robot, human) pair, the min
//                    over the humans (torch.min: NaN propagates);
// with propagate (cadrl.py:104-129), compute_reward (multi_human_rl.py:65-88) and the rotation into 13 features
// (cadrl.py:217-252) exactly as sarl_value.hip does them, value = reward + gamma^(dt*v_pref) * V in float64, then
// the strict-'>' argmax / epsilon-greedy kernel of sarl_value.hip.
//
// Layout as in sarl_value.hip: a pair (env, action) sits on the MFMA j index, one wavefront owns 16 pairs, features
// sit on i/k, every activation stays in registers and the layers chain with no LDS transposes (mfma_chain.hpp).
// Weights are mcn_pack_linear fragments.  The layer run once per human -- the LSTM gate layer, or CADRL's whole
// network -- is copied into LDS once per workgroup (80 / 136 KiB); LSTM-RL's tail (run once per pair) streams its
// fragments from L2.
//
// LSTM gate layer: gates = [W_ih | W_hh] [x ; h] + (b_ih + b_hh), 13 + 50 inputs (x tile, then 4 h tiles).  The packer's
// omap puts unit u of gate G (PyTorch order i, f, g, o) in output tile 4G + t, slot s, where (t, s) is the slot of unit
// u in h -- so the cell update is element-wise per register, and the new h is, as it stands, the next step's input.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "lookahead_common.hpp"
#include "launch.hpp"

namespace mcn {

namespace {

enum { kBodyLstm = 0, kBodyCadrl = 1 };
constexpr int kWaves = 8;                          // one 512-thread workgroup per CU (its LDS copy of the weights)
constexpr int kMaxBlocks = 256;                    // persistent grid: one workgroup per CU of an MI355X
// LDS float4s of the per-human layer: LSTM gates [16 tiles][5 k-tiles][64]; CADRL 13->150, 150->100, 100->100, 100->1
constexpr int kLdsGate = 16 * 5 * 64;
constexpr int kCadrlOff[5] = {0, 10 * 1 * 64, 10 * 64 + 7 * 10 * 64, 10 * 64 + 70 * 64 + 7 * 7 * 64,
                              10 * 64 + 70 * 64 + 49 * 64 + 1 * 7 * 64};

struct LookParams {
    const float4 *w[5], *b[5];     // LSTM: gate, mlp.0, mlp.2, mlp.4, mlp.6; CADRL: value_network.{0,2,4,6}
    PairParams c;
    int32_t *order;                // [E*N] or NULL (LSTM-RL)
};

// sgan_step.hip's forms (~2e-7 absolute error)
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }
__device__ __forceinline__ float tanh_f(float x)
{
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.88539008f * x)), 1.0f);
}

// Human order of LstmRL.predict (lstm_rl.py:99-103): sorted(humans, key=distance to the robot's CURRENT position,
// reverse=True).  Python's sort is stable, so for non-NaN distances (+inf included) equal distances keep their index
// order: selection of the first strict maximum among the humans not yet taken is the same permutation.  Only the
// env's first `ne` humans take part; the result is always a permutation of 0 .. ne-1.  Where CPython's order of NaN
// keys depends on its sort's internals, this path defines one: NaN distances come last, in index order -- init() holds
// them as -1, below every distance (a norm is >= 0 or +inf), so they never win a strict '>' against a real one.
template <int MAXN>
struct HumanOrder {
    double d[MAXN];
    uint32_t used;
    __device__ __forceinline__ void init(const double *hpos, long base, double rx, double ry, int ne)
    {
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            d[i] = 0.0;
            if (i < ne) {
                const double2 h = reinterpret_cast<const double2 *>(hpos)[base + i];
                const double di = norm2d(h.x - rx, h.y - ry);        // np.linalg.norm(human.position - self.position)
                d[i] = di == di ? di : -1.0;
            }
        }
        used = 0;
    }
    __device__ __forceinline__ int next(int ne)
    {
        int best = -1;
        double bd = 0.0;
#pragma unroll
        for (int i = 0; i < MAXN; ++i) {
            const bool open = i < ne && !((used >> i) & 1u);
            if (open && (best < 0 || d[i] > bd)) { best = i; bd = d[i]; }
        }
        best = best < 0 ? 0 : best;                        // (not reached: next() is called at most ne times)
        used |= 1u << best;
        return best;
    }
};

template <int BODY, int MAXN>
__global__ __launch_bounds__(kWaves * 64, 1) void lookahead_kernel(const LookParams p)
{
    constexpr int kLds = BODY == kBodyLstm ? kLdsGate : kCadrlOff[4];
    __shared__ float4 s_w[kLds];
    if constexpr (BODY == kBodyLstm) {
        for (int i = threadIdx.x; i < kLdsGate; i += kWaves * 64) s_w[i] = p.w[0][i];
    } else {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            for (int i = threadIdx.x; i < kCadrlOff[l + 1] - kCadrlOff[l]; i += kWaves * 64) s_w[kCadrlOff[l] + i] = p.w[l][i];
    }
    __syncthreads();

    const PairParams &pp = p.c;
    const long npairs = (long)pp.E * pp.A;
    const int N = pp.N;
    // no barrier below: a wavefront may leave as soon as its tiles are done
#pragma unroll 1
    for (long grp = blockIdx.x; grp < pp.ngroups; grp += gridDim.x) {
        // the thread id is made opaque once per pass (as in sarl_value.hip): the per-lane addresses of every weight
        // fragment would otherwise be hoisted out of the loop as loop invariants, live -- and spill -- across it
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, wave = tid >> 6;
        const int j = lane & 15, q = lane >> 4;
        const long pair0 = (grp * kWaves + wave) * 16;
        if (pair0 >= npairs) break;
        long pair = pair0 + j;
        const bool valid = pair < npairs;
        if (!valid) pair = npairs - 1;
        const int e = (int)(pair / pp.A), a = (int)(pair - (long)e * pp.A);
        const int ne = humans_seen(pp.hcount, e, N);
        const double2 rp = reinterpret_cast<const double2 *>(pp.rpos)[e];
        const double2 rg = reinterpret_cast<const double2 *>(pp.rgoal)[e];
        const double2 ra = make_double2(pp.rrad[e], pp.rvpref[e]);               // radius, v_pref
        const RobotNext rn = robot_after(pp, e, a, rp);
        const SelfFeatures sf = self_features(rn, rg, ra, pp.kinematics);
        double dmin = INFINITY;
        float V;
        if constexpr (BODY == kBodyLstm) {
            // ---- LSTM over the humans in sorted order (identity with the env's next states, multi_human_rl.py:37-38) ----
            HumanOrder<MAXN> ord;
            const bool sort = pp.next_hpos == nullptr;
            if (sort) ord.init(pp.hpos, (long)e * N, rp.x, rp.y, ne);
            f32x4 in[5];                               // [x | h0 h1 h2 h3]
            f32x4 c[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { in[1 + t] = (f32x4){0, 0, 0, 0}; c[t] = (f32x4){0, 0, 0, 0}; }
            for (int s = 0; s < N; ++s) {
                int lane_s = lane;                     // per step, likewise
                asm volatile("" : "+v"(lane_s));
                const bool seen = s < ne;
                const int hi = (seen && sort) ? ord.next(ne) : s;
                if (p.order && valid && q == 0 && a == 0) p.order[(long)e * N + s] = hi;
                in[0] = human_tile(pp, (long)e * N + hi, rn, ra.x, sf, q, seen, dmin).x;
                f32x4 hn[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x4 gi, gf, gg, go;
                    dense_tiles<5, kBiasFrag, 4, 1>(in, s_w, p.b[0], t, 4 + t, true, lane_s, gi, gf);
                    dense_tiles<5, kBiasFrag, 4, 1>(in, s_w, p.b[0], 8 + t, 12 + t, true, lane_s, gg, go);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float cn = sigmoid_f(gf[r]) * c[t][r] + sigmoid_f(gi[r]) * tanh_f(gg[r]);
                        const float h = sigmoid_f(go[r]) * tanh_f(cn);
                        c[t][r] = seen ? cn : c[t][r];
                        hn[t][r] = seen ? h : in[1 + t][r];
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) in[1 + t] = hn[t];
            }
            // ---- tail: mlp on [self(6) | h(50)] (lstm_rl.py:30-32) ----
            in[0] = self_tile(sf, q);
            f32x4 v1[10], v2[7], v3[7], vo[1];
            dense<5, 10, kReluKeepNan, kBiasFrag, 2, 1>(in, v1, p.w[1], p.b[1], lane);
            dense<10, 7, kReluKeepNan, kBiasFrag, 4, 2>(v1, v2, p.w[2], p.b[2], lane);
            dense<7, 7, kReluKeepNan, kBiasFrag, 4, 1>(v2, v3, p.w[3], p.b[3], lane);
            dense<7, 1, kLinear, kBiasFrag, 4, 1>(v3, vo, p.w[4], p.b[4], lane);
            V = vo[0][0];
        } else {
            // ---- CADRL: value network per (robot, human) pair, min over the humans (cadrl.py:162-165) ----
            V = INFINITY;
            for (int i = 0; i < N; ++i) {
                int lane_i = lane;
                asm volatile("" : "+v"(lane_i));
                const bool seen = i < ne;
                f32x4 x[1];
                x[0] = human_tile(pp, (long)e * N + i, rn, ra.x, sf, q, seen, dmin).x;
                f32x4 v1[10], v2[7], v3[7], vo[1];
                dense<1, 10, kReluKeepNan, kBiasFrag, 4, 4>(x, v1, s_w + kCadrlOff[0], p.b[0], lane_i);
                dense<10, 7, kReluKeepNan, kBiasFrag, 4, 2>(v1, v2, s_w + kCadrlOff[1], p.b[1], lane_i);
                dense<7, 7, kReluKeepNan, kBiasFrag, 4, 1>(v2, v3, s_w + kCadrlOff[2], p.b[2], lane_i);
                dense<7, 1, kLinear, kBiasFrag, 4, 1>(v3, vo, s_w + kCadrlOff[3], p.b[3], lane_i);
                const float v = vo[0][0];
                // torch.min: the first NaN wins and stays
                if (seen && (v < V || v != v) && V == V) V = v;
            }
        }
        const double reward = pair_reward(pp, rn, rg, ra.x, dmin, pair);
        if (valid && q == 0) pp.values[pair] = pair_value(pp, reward, V);
    }
}

// LstmRL's order on its own (the rows `transform` stores, lstm_rl.py:99-103 + multi_human_rl.py:60-61): one thread
// per env, the same HumanOrder as the look-ahead.  Slots >= hcount[e] keep their index.
template <int MAXN>
__global__ __launch_bounds__(64) void lstm_rl_order_kernel(const double *hpos, const double *rpos, const int32_t *hcount,
                                                          int32_t *order, int E, int N)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const int ne = humans_seen(hcount, e, N);
    const double2 rp = reinterpret_cast<const double2 *>(rpos)[e];
    HumanOrder<MAXN> ord;
    ord.init(hpos, (long)e * N, rp.x, rp.y, ne);
    for (int s = 0; s < N; ++s) order[(long)e * N + s] = s < ne ? ord.next(ne) : s;
}

template <int BODY>
void launch_body(const LookParams &p, int blocks, hipStream_t stream)
{
    // MAXN sizes the sort state: 1 where there is no sort (CADRL; the env's next states keep the env's order)
    if constexpr (BODY == kBodyCadrl) {
        hipLaunchKernelGGL((lookahead_kernel<BODY, 1>), dim3(blocks), dim3(kWaves * 64), 0, stream, p);
    } else if (p.c.next_hpos) {
        hipLaunchKernelGGL((lookahead_kernel<BODY, 1>), dim3(blocks), dim3(kWaves * 64), 0, stream, p);
    } else if (p.c.N <= 8) {
        hipLaunchKernelGGL((lookahead_kernel<BODY, 8>), dim3(blocks), dim3(kWaves * 64), 0, stream, p);
    } else if (p.c.N <= 16) {
        hipLaunchKernelGGL((lookahead_kernel<BODY, 16>), dim3(blocks), dim3(kWaves * 64), 0, stream, p);
    } else {
        hipLaunchKernelGGL((lookahead_kernel<BODY, 32>), dim3(blocks), dim3(kWaves * 64), 0, stream, p);
    }
}

int launch_lookahead(int body, const void *const *frags, int nlayers, const mcn_env_state *st, const double *actions,
                     int A, double dt, double gamma_pow, int kinematics, double *values, int32_t *best, double *best_val,
                     int32_t *order, const double *next_hpos, const double *next_hvel, const double *reward_in,
                     double *action_out, double epsilon, unsigned long long seed, int E, int N, hipStream_t stream)
{
    LookParams p;
    for (int l = 0; l < 5; ++l) {
        p.w[l] = l < nlayers ? reinterpret_cast<const float4 *>(frags[2 * l]) : nullptr;
        p.b[l] = l < nlayers ? reinterpret_cast<const float4 *>(frags[2 * l + 1]) : nullptr;
    }
    p.c = pair_params(st, actions, A, dt, gamma_pow, kinematics, values, next_hpos, next_hvel, reward_in, E, N, kWaves);
    p.order = order;
    const int blocks = (int)(p.c.ngroups < kMaxBlocks ? p.c.ngroups : kMaxBlocks);
    if (body == kBodyLstm) launch_body<kBodyLstm>(p, blocks, stream);
    else launch_body<kBodyCadrl>(p, blocks, stream);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    if (best) return launch_sarl_argmax(values, p.c.rpos, p.c.rgoal, p.c.rrad, E, A, best, best_val, actions, action_out,
                                        epsilon, seed, stream);
    return MCN_OK;
}

}  // namespace

int launch_lstm_rl(const mcn_lstm_rl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                   double gamma_pow, int kinematics, double *values, int32_t *best, double *best_val, int32_t *order,
                   const double *next_hpos, const double *next_hvel, const double *reward_in, double *action_out,
                   double epsilon, unsigned long long seed, int E, int N, hipStream_t stream)
{
    static_assert(sizeof(mcn_lstm_rl_net) == 10 * sizeof(void *), "mcn_lstm_rl_net: five (weights, bias) pairs");
    return launch_lookahead(kBodyLstm, reinterpret_cast<const void *const *>(net), 5, st, actions, A, dt, gamma_pow,
                            kinematics, values, best, best_val, order, next_hpos, next_hvel, reward_in, action_out,
                            epsilon, seed, E, N, stream);
}

int launch_cadrl(const mcn_cadrl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                 double gamma_pow, int kinematics, double *values, int32_t *best, double *best_val,
                 const double *next_hpos, const double *next_hvel, const double *reward_in, double *action_out,
                 double epsilon, unsigned long long seed, int E, int N, hipStream_t stream)
{
    static_assert(sizeof(mcn_cadrl_net) == 8 * sizeof(void *), "mcn_cadrl_net: four (weights, bias) pairs");
    return launch_lookahead(kBodyCadrl, reinterpret_cast<const void *const *>(net), 4, st, actions, A, dt, gamma_pow,
                            kinematics, values, best, best_val, nullptr, next_hpos, next_hvel, reward_in, action_out,
                            epsilon, seed, E, N, stream);
}

int launch_lstm_rl_order(const double *hpos, const double *rpos, const int32_t *hcount, int32_t *order, int E, int N,
                         hipStream_t stream)
{
    const dim3 grid((E + 63) / 64);
    if (N <= 8) hipLaunchKernelGGL(lstm_rl_order_kernel<8>, grid, dim3(64), 0, stream, hpos, rpos, hcount, order, E, N);
    else if (N <= 16) hipLaunchKernelGGL(lstm_rl_order_kernel<16>, grid, dim3(64), 0, stream, hpos, rpos, hcount, order, E, N);
    else hipLaunchKernelGGL(lstm_rl_order_kernel<32>, grid, dim3(64), 0, stream, hpos, rpos, hcount, order, E, N);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace mcn
