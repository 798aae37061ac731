// sarl_value.hip -- SARL 81-action one-step look-ahead, fused, for gfx950 (MI355X).
//
// Replaces, per environment and candidate action (crowd_nav/policy/multi_human_rl.py:35-52):
//   propagate (cadrl.py:104-129), compute_reward (multi_human_rl.py:65-88), the [N,14] -> [N,13]
//   agent-centric transform (cadrl.py:217-252), ValueNetwork.forward (sarl.py:28-65: mlp1, mlp2,
//   global-state attention, un-stabilised masked softmax, pooling, mlp3) and
//   value = reward + gamma^(dt*v_pref) * V, followed by the strict-'>' argmax (:53-55).
//
// Structure.  A "pair" is one (environment, action).  One wavefront owns 16 consecutive pairs and
// carries them through the whole network with every activation in registers:
//
//   v_mfma_f32_16x16x4_f32 computes D[i][j] += A[i][k] B[k][j] with lane l holding A[l&15][l>>4],
//   B[l>>4][l&15] and D[4(l>>4)+r][l&15] in accumulator register r.  We put the PAIR on j (the lane's
//   low 4 bits) and the FEATURE on i/k.  A layer's output tile (16 features x 16 pairs) is then
//   already, register by register, a valid B operand of the next layer: register r of lane l holds
//   feature 4(l>>4)+r of pair l&15, i.e. B[k=l>>4][j] of the k-step that sums features {r, 4+r, 8+r,
//   12+r}.  So layers chain with no LDS round trip, no transposes and no barriers; only the weights
//   move, as A operands, pre-permuted on the host into exactly that order (one coalesced 16-B load per
//   lane feeds four MFMAs).  The N humans of a pair are processed one after the other by the same
//   lanes, which makes the reductions over humans (global-state mean, softmax denominator, pooled
//   feature) plain per-lane register arithmetic.
//
//   pass 1, per human: features -> mlp1 (13->150->100); park mlp1's output in the wavefront's workspace slot,
//                      accumulate the mean.  The grid is PERSISTENT (at most kSarlMaxBlocks workgroups, two per CU,
//                      each walking over its share of the 16-pair tiles), so the workspace is indexed by resident
//                      wavefront, not by tile: 2 048 slots x N x 7 KiB = 72 MB at N = 5 (143 MB at N = 10) whatever
//                      the batch -- it lives in the 256 MB Infinity Cache between the two passes instead of making a
//                      round trip through HBM (0.74 / 1.49 GB per look-ahead when it was indexed by tile).
//   pass 2, per human: attention (200->100->100->1) with the global half folded into the accumulator
//                      init, exp, mlp2's first layer (100->100), acc += e * relu(.).
//   tail:              mlp2's second, linear layer (100->50) once on acc / sum(e); mlp3 (56->150->100->100->1),
//                      value, store.
//
// Arithmetic: float32 MFMA is an exact k-ordered fmaf chain (no TF32), so values match the
// reference's float32 network to summation-order noise (~1e-6); rewards are float64 in the
// reference's operation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/mcn.h"
#include "lookahead_common.hpp"
#include "launch.hpp"

namespace mcn {

// a layer's output tiles -> the next layer's input blocks, as one block after the layer
template <int NT, int NB>
__device__ __forceinline__ void split_after(const f32x4 (&t)[NT], X3 (&o)[NB])
{
    const f32x4 z = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < NB; ++m) o[m] = split8(t[2 * m], 2 * m + 1 < NT ? t[2 * m + 1] : z);
}

// tiles of 16 features
constexpr int T13 = 1, T150 = 10, T100 = 7, T50 = 4, T56 = 5 /* pooled 4 + self 1 */, T1 = 1;

struct SarlFrags {
    // weight fragments [NT][KT][64 lanes] float4 and bias fragments [NT][64] float4, see pack order in
    // modelcrowdnav_amd/policy/sarl.py (_pack_plan, pack_value_network)
    const float4 *w_m1a, *b_m1a;   // 13 -> 150
    const float4 *w_m1b, *b_m1b;   // 150 -> 100
    const float4 *w_m2a, *b_m2a;   // 100 -> 100
    const float4 *w_m2b, *b_m2b;   // 100 -> 50
    const float4 *w_ata, *b_ata;   // attention layer 0, local half (100 -> 100), bias = attention.0.bias
    const float4 *w_atg;           // attention layer 0, global half (100 -> 100), no bias
    const float4 *w_atb, *b_atb;   // 100 -> 100
    const float4 *w_atc, *b_atc;   // 100 -> 1
    const float4 *w_m3a, *b_m3a;   // 56 -> 150   (K tiles: pooled x4, self x1)
    const float4 *w_m3b, *b_m3b;   // 150 -> 100
    const float4 *w_m3c, *b_m3c;   // 100 -> 100
    const float4 *w_m3d, *b_m3d;   // 100 -> 1
};

// bf16x3 weight fragments (mcn_pack_x3 of the float32 fragments above; biases stay the float32 ones): NULL table = float32 MFMA
struct SarlX3 {
    const float4 *w_m1a, *w_m1b, *w_m2a, *w_m2b, *w_ata, *w_atg, *w_atb, *w_atc, *w_m3a, *w_m3b, *w_m3c, *w_m3d;
};
// 32-feature input blocks of the x3 layers
constexpr int B13 = 1, B150 = 5, B100 = 4, B56 = 3;
constexpr int kWsRowsF32 = T100, kWsRowsX3 = B100 * 3;      // 16-byte workspace rows per human and lane: float32 tiles / x3 pieces

struct SarlParams {
    SarlFrags f;
    SarlX3 x;
    PairParams c;                                         // ngroups: 4-tile groups (one per workgroup pass)
    float4 *workspace;                                    // [resident waves][N][12 rows][64] float4 (+ 7 rows unused)
    float *attention;                                     // [E*A*N] or NULL
    const float4 *om_init;                                // WITH_OM: [E*N][40], mlp1.0's accumulator start (sarl_om.hip)
};

// Diagnostic build only (tools/sarl_phases.py): shader cycles each resident wavefront spends in each phase of a tile,
// summed over the tiles it walks.  [wavefront][16]: see PHASES in the tool.
#ifdef MCN_DIAG
__device__ unsigned long long g_sarl_phase[2048 * 16];
#define SARL_T0() unsigned long long sp_t_ = __builtin_amdgcn_s_memtime()
#define SARL_PHASE(k_)                                                                                          \
    do {                                                                                                        \
        const unsigned long long n_ = __builtin_amdgcn_s_memtime();                                             \
        const int w_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);                                     \
        if ((threadIdx.x & 63) == 0 && w_ < 2048) g_sarl_phase[w_ * 16 + (k_)] += n_ - sp_t_;                   \
        sp_t_ = n_;                                                                                             \
    } while (0)
int read_sarl_phases(void *dst, size_t bytes, int reset)
{
    if (bytes > sizeof(g_sarl_phase)) bytes = sizeof(g_sarl_phase);
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_sarl_phase), bytes) != hipSuccess) return -1;
    if (reset) {
        void *p_ = nullptr;
        if (hipGetSymbolAddress(&p_, HIP_SYMBOL(g_sarl_phase)) != hipSuccess || hipMemset(p_, 0, sizeof(g_sarl_phase)) != hipSuccess) return -1;
    }
    return (int)(bytes / 8);
}
#else
#define SARL_T0()
#define SARL_PHASE(k_)
#endif

constexpr int kSarlWaves = kStageThreads / 64;     // 8 wavefronts share one LDS weight stage (2 per SIMD)

// The layers of a tile (and of the next tile) form ONE weight stream: each layer requests the first staged chunk of the
// layer that follows it (mfma_chain.hpp: dense_flow, dense_flow_x3).
// USE_X3 = false: float32 MFMA layers (v_mfma_f32_16x16x4_f32); USE_X3 = true: the same layers on the bf16 matrix pipe with every
// operand split into three bfloat16 pieces (mfma_chain.hpp: dense_flow_x3) -- float32-accurate, ~2.7 x fewer pipe cycles.
// WITH_OM (OM-SARL, sarl.py with_om = true: mlp1.0 is 61 -> 150 on [x13 | occupancy map 48]): the map's share of mlp1.0
// and the bias are the same for every action of an env and come precomputed per (env, human) in p.om_init, so mlp1.0
// stays the 13-wide layer and takes that row as its accumulator start, as attention.0 takes its global half.
template <bool USE_X3, bool WITH_OM>
__global__ __launch_bounds__(kSarlWaves * 64, kSarlWaves >= 8 ? 1 : 2) void sarl_value_kernel(const SarlParams p)
{
    __shared__ float4 s_stage[2 * (kStageFloat4 + kStageBias)];
    const PairParams &c = p.c;
    const long npairs = (long)c.E * c.A;
    const int N = c.N;
    // chunk 0 of every layer, as the layer before it requests it
#define SARL_FIRST(KT, KB, NT, INIT, name, bias)                                                              \
    (USE_X3 ? first_chunk_x3<KB, NT, INIT>(p.x.w_##name, bias) : first_chunk<KT, NT, INIT>(p.f.w_##name, bias))
    const NextChunk d_m1a = SARL_FIRST(T13, B13, T150, WITH_OM, m1a, WITH_OM ? nullptr : p.f.b_m1a), d_m1b = SARL_FIRST(T150, B150, T100, false, m1b, p.f.b_m1b);
    const NextChunk d_atg = SARL_FIRST(T100, B100, T100, false, atg, p.f.b_ata), d_ata = SARL_FIRST(T100, B100, T100, true, ata, nullptr);
    const NextChunk d_atb = SARL_FIRST(T100, B100, T100, false, atb, p.f.b_atb), d_atc = SARL_FIRST(T100, B100, T1, false, atc, p.f.b_atc);
    const NextChunk d_m2a = SARL_FIRST(T100, B100, T100, false, m2a, p.f.b_m2a), d_m2b = SARL_FIRST(T100, B100, T50, false, m2b, p.f.b_m2b);
    const NextChunk d_m3a = SARL_FIRST(T56, B56, T150, false, m3a, p.f.b_m3a), d_m3b = SARL_FIRST(T150, B150, T100, false, m3b, p.f.b_m3b);
    const NextChunk d_m3c = SARL_FIRST(T100, B100, T100, false, m3c, p.f.b_m3c), d_m3d = SARL_FIRST(T100, B100, T1, false, m3d, p.f.b_m3d);
#undef SARL_FIRST
    const NextChunk d_none = {nullptr, 0, nullptr, 0, 0};
    WeightFlow F{s_stage, (int)threadIdx.x, 0};
    if ((long)blockIdx.x < c.ngroups) flow_stage_first(F, d_m1a, 0);         // the very first layer of this workgroup
    __syncthreads();
    // every wavefront of the workgroup runs the same number of passes (the weight-staging barriers are collective)
#pragma unroll 1
  for (long grp = blockIdx.x; grp < c.ngroups; grp += gridDim.x) {
    // the thread id is made opaque once per pass: everything derived from it (the per-lane addresses of every weight
    // chunk of every layer) would otherwise be hoisted out of this loop and live -- and spill -- across it
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    // this wavefront's workspace slot: by resident wavefront (persistent grid), reused for every tile it walks over
    constexpr int WSR = USE_X3 ? kWsRowsX3 : kWsRowsF32;                   // 16-byte rows per human and lane
    // slot of this wavefront: N humans x WSR rows used, stride as sarl_workspace_float4s()
    float4 *const ws = p.workspace + ((long)blockIdx.x * kSarlWaves + wave) * ((long)N * kWsRowsX3 + T100) * 64;
    const long pair0 = (grp * kSarlWaves + wave) * 16;
    SARL_T0();
    // no early exit: every wavefront of the workgroup takes part in the weight staging barriers
    long pair = pair0 + j;
    const bool valid = pair < npairs;
    if (!valid) pair = npairs - 1;
    const int e = (int)(pair / c.A), a = (int)(pair - (long)e * c.A);
    // pedestrians this pair's env shows to the policy; the loops below stay N long for the whole workgroup (they
    // contain the weight-staging barriers) and absent slots are masked out of every reduction
    const int ne = humans_seen(c.hcount, e, N);
    const double2 rp = reinterpret_cast<const double2 *>(c.rpos)[e];
    const double2 rg = reinterpret_cast<const double2 *>(c.rgoal)[e];
    const double2 ra = make_double2(c.rrad[e], c.rvpref[e]);               // radius, v_pref
    const RobotNext rn = robot_after(c, e, a, rp);
    const SelfFeatures sf = self_features(rn, rg, ra, c.kinematics);

    // ---- pass 1: mlp1 per human, global-state sum, reward ----
    f32x4 gsum[T100];
#pragma unroll
    for (int t = 0; t < T100; ++t) gsum[t] = (f32x4){0, 0, 0, 0};
    double dmin = INFINITY;
    // NaN where the reference is NaN: its masked softmax makes NaN a specified result and torch.relu keeps NaN, while
    // the layers' ReLU here (relu_f32, an integer max: one vector instruction) turns a NaN with the sign bit set into 0
    // -- and both signs occur: hosts hand over either, the matrix pipe makes its own.  A ReLU that keeps NaN (compare +
    // select, one instruction more per activation) was measured in every layer: +0.7 % (4096 x 5) and +1.8 % (4096 x 10)
    // of the look-ahead, the latter outside the run-to-run spread.  So the layers keep the integer max and
    // this per-pair flag forces the stored value to NaN instead.  It is set by
    //   * a non-finite float32 feature of a present human (the robot's six are among every human's thirteen): in the
    //     reference it reaches every unit of mlp1, the mean and with it every score of the pair (NaN whatever the
    //     weights are; +-inf unless every weight it meets has one sign);
    //   * the normalised sum of the tail being NaN: 0 / 0 or inf / inf in the softmax.
    bool poisoned = false;
    SARL_PHASE(0);                      // tile set-up: robot state, self features
    for (int i = 0; i < N; ++i) {
        // per-pass opaque copy of the thread id, from the form in which every layer staged its own weights.  Nothing
        // reads it now (the flow layers derive their addresses in dma_lane), but the statement still orders the
        // schedule: without it the kernels come out different (202 instead of 204 VGPRs) -- a change to measure, not
        // one to make in passing
        int tid_i = tid;
        asm volatile("" : "+v"(tid_i));
        // mlp1.0's accumulator start of this human: ten 16-byte loads, by the LANE's env (a tile spans two envs whenever
        // A is not a multiple of 16); in registers for the length of that layer (fetched tile by tile inside the layer
        // the loads would queue on vmcnt behind the LDS-DMA weight stream: DESIGN 9)
        f32x4 omi[WITH_OM ? T150 : 1];
        if constexpr (WITH_OM) {
            const float4 *src = p.om_init + ((long)e * N + i) * (T150 * 4) + q;
#pragma unroll
            for (int n = 0; n < T150; ++n) { const float4 v = src[4 * n]; omi[n] = (f32x4){v.x, v.y, v.z, v.w}; }
        }
        const f32x4 *const m1a_init = WITH_OM ? omi : nullptr;
        const HumanTile ht = human_tile(c, (long)e * N + i, rn, ra.x, sf, q, i < ne, dmin);
        poisoned = poisoned || (i < ne && ht.nonfinite);
        f32x4 x[T13] = {ht.x};
        SARL_PHASE(1);                  // per human: state loads, float64 distance, rotated features
        f32x4 h1[T150];
        f32x4 h2[T100];
        const f32x4 zero4 = {0, 0, 0, 0};
        if constexpr (USE_X3) {
            const X3 xin[B13] = {split8(x[0], zero4)};
            X3 h1p[B150];
            dense_flow_x3<B13, T150, true, WITH_OM>(xin, m1a_init, h1, p.x.w_m1a, reinterpret_cast<const float4 *>(p.f.b_m1a), F, lane, d_m1b);
            split_after(h1, h1p);
            SARL_PHASE(2);              // mlp1.0
            X3 h2p[B100];
            auto add_to_mean = [&](int n, const f32x4 &v) { if (i < ne) gsum[n] += v; };       // global-state sum, tile by tile
            dense_flow_x3<B150, T100, true, false>(h1p, nullptr, h2, p.x.w_m1b, reinterpret_cast<const float4 *>(p.f.b_m1b),
                                                                F, lane, (i + 1 < N ? d_m1a : d_atg), add_to_mean);
            split_after(h2, h2p);
            SARL_PHASE(3);              // mlp1.2
            // the workspace keeps mlp1's output already split: pass 2 reads the pieces twice (attention.0, mlp2.0)
#pragma unroll
            for (int m = 0; m < B100; ++m) {
                ws[(i * WSR + 3 * m + 0) * 64 + lane] = __builtin_bit_cast(float4, h2p[m].hi);
                ws[(i * WSR + 3 * m + 1) * 64 + lane] = __builtin_bit_cast(float4, h2p[m].mid);
                ws[(i * WSR + 3 * m + 2) * 64 + lane] = __builtin_bit_cast(float4, h2p[m].lo);
            }
        } else {
        dense_flow<T13, T150, true, WITH_OM, 4, 4>(x, m1a_init, h1, p.f.w_m1a, p.f.b_m1a, F, lane, d_m1b);
        SARL_PHASE(2);                  // mlp1.0
        dense_flow<T150, T100, true, false, 2, 4>(h1, nullptr, h2, p.f.w_m1b, p.f.b_m1b, F, lane, (i + 1 < N ? d_m1a : d_atg));
        SARL_PHASE(3);                  // mlp1.2
#pragma unroll
        for (int t = 0; t < T100; ++t) {
            ws[(i * T100 + t) * 64 + lane] = make_float4(h2[t][0], h2[t][1], h2[t][2], h2[t][3]);
            if (i < ne) gsum[t] += h2[t];
        }
        }
        SARL_PHASE(4);                  // workspace store, global-state sum
    }
    const double reward = pair_reward(c, rn, rg, ra.x, dmin, pair);

    // global state = mean over humans (sarl.py:41); its contribution to attention layer 0 is the same for
    // every human of the pair, so it becomes the accumulator init of that layer
    // (one correctly rounded reciprocal + 28 multiplies instead of 28 IEEE divisions of ~11 instructions each: vector
    //  instructions are paid beside float32 MFMAs; the mean moves by <= 1 ulp, far inside the 1e-5 bar)
    const float inv_n = 1.0f / (float)ne;
#pragma unroll
    for (int t = 0; t < T100; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) gsum[t][r] = gsum[t][r] * inv_n;
    f32x4 gat[T100];
    const f32x4 zero4 = {0, 0, 0, 0};
    if constexpr (USE_X3) {
        X3 gp[B100];
#pragma unroll
        for (int m = 0; m < B100; ++m) gp[m] = split8(gsum[2 * m], 2 * m + 1 < T100 ? gsum[2 * m + 1] : zero4);
        dense_flow_x3<B100, T100, false, false>(gp, nullptr, gat, p.x.w_atg, reinterpret_cast<const float4 *>(p.f.b_ata), F, lane, d_m2a);
    } else {
    dense_flow<T100, T100, false, false, 1, 4>(gsum, nullptr, gat, p.f.w_atg, p.f.b_ata, F, lane, d_ata);
    }
    SARL_PHASE(5);                      // reward ladder, mean, global half of attention.0

    // ---- pass 2: attention score, mlp2, pooling ----
    // mlp2's last layer is linear (sarl.py:31, cadrl.py:11-19: no ReLU after the last Linear) and the attention
    // weights sum to one, so  sum_i w_i (W r_i + b) = W (sum_i w_i r_i) + b  with r_i = relu(mlp2.0(h_i)): the
    // weighted sum is taken over the 100-wide hidden activations and mlp2.2 runs ONCE per pair instead of once
    // per human (100 MFMAs per human fewer; same value to float32 summation-order noise, ~1e-7).
    f32x4 racc[T100];
#pragma unroll
    for (int t = 0; t < T100; ++t) racc[t] = (f32x4){0, 0, 0, 0};
    float denom = 0.0f;
    for (int i = 0; i < N; ++i) {
        int tid_i = tid;                // (as in pass 1)
        asm volatile("" : "+v"(tid_i));
        f32x4 h2[T100];
        f32x4 a1[T100];
        f32x4 a2[T100];
        f32x4 sc[T1];
        auto load_pieces = [&](X3 (&dst)[B100]) {          // mlp1's output of human i, as pass 1 split it
#pragma unroll
            for (int m = 0; m < B100; ++m) {
                dst[m].hi = __builtin_bit_cast(bf16x8, ws[(i * WSR + 3 * m + 0) * 64 + lane]);
                dst[m].mid = __builtin_bit_cast(bf16x8, ws[(i * WSR + 3 * m + 1) * 64 + lane]);
                dst[m].lo = __builtin_bit_cast(bf16x8, ws[(i * WSR + 3 * m + 2) * 64 + lane]);
            }
        };
        f32x4 m1[T100];
        if constexpr (USE_X3) {
            X3 hp[B100];
            load_pieces(hp);
            SARL_PHASE(6);              // workspace load
            // mlp2.0 of this human FIRST, while its mlp1 pieces are in registers for attention.0 anyway: its 28
            // output registers wait for the score instead of the 12 KiB of pieces being read a second time
            dense_flow_x3<B100, T100, true, false>(hp, nullptr, m1, p.x.w_m2a, reinterpret_cast<const float4 *>(p.f.b_m2a), F, lane, d_ata);
            X3 ap[B100], bp[B100];
            dense_flow_x3<B100, T100, true, true>(hp, gat, a1, p.x.w_ata, nullptr, F, lane, d_atb);
            split_after(a1, ap);
            SARL_PHASE(7);              // attention.0
            dense_flow_x3<B100, T100, true, false>(ap, nullptr, a2, p.x.w_atb, reinterpret_cast<const float4 *>(p.f.b_atb), F, lane, d_atc);
            split_after(a2, bp);
            SARL_PHASE(8);              // attention.2
            dense_flow_x3<B100, T1, false, false>(bp, nullptr, sc, p.x.w_atc, reinterpret_cast<const float4 *>(p.f.b_atc), F, lane,
                                                  (i + 1 < N ? d_m2a : d_m2b));
        } else {
#pragma unroll
        for (int t = 0; t < T100; ++t) {
            const float4 v = ws[(i * T100 + t) * 64 + lane];
            h2[t] = (f32x4){v.x, v.y, v.z, v.w};
        }
        SARL_PHASE(6);                  // workspace load
        dense_flow<T100, T100, true, true, 1, 4>(h2, gat, a1, p.f.w_ata, nullptr, F, lane, d_atb);
        SARL_PHASE(7);                  // attention.0
        dense_flow<T100, T100, true, false, 1, 4>(a1, nullptr, a2, p.f.w_atb, p.f.b_atb, F, lane, d_atc);
        SARL_PHASE(8);                  // attention.2
        dense_flow<T100, T1, false, false, 1, 4>(a2, nullptr, sc, p.f.w_atc, p.f.b_atc, F, lane, d_m2a);
        }
        SARL_PHASE(9);                  // attention.4
        // score of pair j sits in lane j (q = 0), register 0; broadcast to the pair's four lanes
        const float s = __shfl(sc[0][0], j);
        const float es = (s != 0.0f && i < ne) ? expf(s) : 0.0f;   // exp(s) * (s != 0), sarl.py:52; absent: 0
        if (p.attention && valid && q == 0) p.attention[pair * N + i] = es;   // normalised by the host view
        denom += es;
        SARL_PHASE(10);                 // exp, attention output
        if constexpr (!USE_X3)
            dense_flow<T100, T100, true, false, 1, 4>(h2, nullptr, m1, p.f.w_m2a, p.f.b_m2a, F, lane, (i + 1 < N ? d_ata : d_m2b));
        SARL_PHASE(11);                 // mlp2.0
#pragma unroll
        for (int t = 0; t < T100; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) racc[t][r] = i < ne ? __builtin_fmaf(es, m1[t][r], racc[t][r]) : racc[t][r];
        SARL_PHASE(12);                 // weighted accumulation
    }

    // ---- tail: mlp3 on [self(6), pooled(50)] ----
    f32x4 jin[T56];
    {
        // weights = exp(s) (s != 0) / sum (sarl.py:52-53): normalise the accumulated hidden activations, then mlp2.2.
        // One reciprocal and 28 multiplies, as for the mean -- but 1 / denom overflows below 2^-128 where the reference,
        // which divides, is finite (scores near -92: each exp ~1e-40), so a tiny sum is first scaled, with the
        // accumulators, by 2^64: exact, subnormals included (a branch no ordinary pair takes; no barrier inside).
        float dsum = denom;                     // (the attention output below divides by the sum itself)
        if (dsum < 0x1p-100f) {
            dsum *= 0x1p+64f;
#pragma unroll
            for (int t = 0; t < T100; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) racc[t][r] *= 0x1p+64f;
        }
        const float inv_d = 1.0f / dsum;
#pragma unroll
        for (int t = 0; t < T100; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) racc[t][r] = racc[t][r] * inv_d;
        // The softmax is the reference's, un-stabilised, and NaN where the reference's is: every present score exactly 0
        // or every exp underflowing is 0 / 0 (here 0 * inf), an exp that overflows is inf / inf (here inf * 0, or a NaN
        // accumulator).  Either makes EVERY accumulator of the pair NaN, so one is tested.
        poisoned = poisoned || racc[0][0] != racc[0][0];
        f32x4 pooled[T50];
        if constexpr (USE_X3) {
            X3 rp3[B100];
#pragma unroll
            for (int m = 0; m < B100; ++m) rp3[m] = split8(racc[2 * m], 2 * m + 1 < T100 ? racc[2 * m + 1] : zero4);
            dense_flow_x3<B100, T50, false, false>(rp3, nullptr, pooled, p.x.w_m2b, reinterpret_cast<const float4 *>(p.f.b_m2b), F, lane, d_m3a);
        } else {
        dense_flow<T100, T50, false, false, 1, 4>(racc, nullptr, pooled, p.f.w_m2b, p.f.b_m2b, F, lane, d_m3a);
        }
#pragma unroll
        for (int t = 0; t < T50; ++t) jin[t] = pooled[t];
    }
    jin[T50] = self_tile(sf, q);
    SARL_PHASE(13);                     // normalise, mlp2.2, self tile
    f32x4 v1[T150];
    f32x4 v2[T100];
    f32x4 v3[T100];
    f32x4 vo[T1];
    if constexpr (USE_X3) {
        X3 jp[B56];                     // input blocks: (pooled tiles 0, 1), (pooled tiles 2, 3), (self tile, -)
        jp[0] = split8(jin[0], jin[1]); jp[1] = split8(jin[2], jin[3]); jp[2] = split8(jin[4], zero4);
        X3 vp[B150];
        dense_flow_x3<B56, T150, true, false>(jp, nullptr, v1, p.x.w_m3a, reinterpret_cast<const float4 *>(p.f.b_m3a), F, lane, d_m3b);
        split_after(v1, vp);
        X3 wp[B100], xp[B100];
        dense_flow_x3<B150, T100, true, false>(vp, nullptr, v2, p.x.w_m3b, reinterpret_cast<const float4 *>(p.f.b_m3b), F, lane, d_m3c);
        split_after(v2, wp);
        dense_flow_x3<B100, T100, true, false>(wp, nullptr, v3, p.x.w_m3c, reinterpret_cast<const float4 *>(p.f.b_m3c), F, lane, d_m3d);
        split_after(v3, xp);
        dense_flow_x3<B100, T1, false, false>(xp, nullptr, vo, p.x.w_m3d, reinterpret_cast<const float4 *>(p.f.b_m3d), F, lane,
                                             (grp + gridDim.x < c.ngroups ? d_m1a : d_none));
    } else {
    dense_flow<T56, T150, true, false, 2, 1>(jin, nullptr, v1, p.f.w_m3a, p.f.b_m3a, F, lane, d_m3b);
    dense_flow<T150, T100, true, false, 2, 4>(v1, nullptr, v2, p.f.w_m3b, p.f.b_m3b, F, lane, d_m3c);
    dense_flow<T100, T100, true, false, 1, 4>(v2, nullptr, v3, p.f.w_m3c, p.f.b_m3c, F, lane, d_m3d);
    dense_flow<T100, T1, false, false, 1, 4>(v3, nullptr, vo, p.f.w_m3d, p.f.b_m3d, F, lane, (grp + gridDim.x < c.ngroups ? d_m1a : d_none));
    }
    if (valid && q == 0) {
        c.values[pair] = poisoned ? __builtin_nan("") : pair_value(c, reward, vo[0][0]);
    }
    if (p.attention && valid && q == 0) {
        // absent slots hold exactly 0 whatever the sum is; present ones are NaN where the reference's weights are
        for (int i = 0; i < ne; ++i) p.attention[pair * N + i] = poisoned ? __builtin_nanf("") : p.attention[pair * N + i] / denom;
    }
    SARL_PHASE(14);                     // mlp3, value store
  }
}

// Strict-'>' argmax over the A candidate values of each env (multi_human_rl.py:53-55: the first maximum
// wins), one wavefront per env.  Also reports reach_destination (policy.py:43-49), for which the reference
// returns the zero action without evaluating anything.
__global__ __launch_bounds__(64) void sarl_argmax_kernel(const double *__restrict__ values, const double *rpos,
                                                       const double *rgoal, const double *rrad, int E, int A,
                                                       int32_t *__restrict__ best, double *__restrict__ best_val,
                                                       const double *__restrict__ actions, double *__restrict__ action_out,
                                                       double epsilon, unsigned long long seed)
{
    const int e = blockIdx.x;
    const int lane = threadIdx.x;
    double bv = -INFINITY; int bi = -1;
    for (int k = lane; k < A; k += 64) {
        const double v = values[(long)e * A + k];
        if (v > bv) { bv = v; bi = k; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        const bool take = (oi >= 0) && (bi < 0 || ov > bv || (ov == bv && oi < bi));
        if (take) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        const double2 rp = reinterpret_cast<const double2 *>(rpos)[e];
        const double2 rg = reinterpret_cast<const double2 *>(rgoal)[e];
        // numpy norm((py - gy, px - gx)): dot = fma(x1, x1, x0 * x0) with x0 = py-gy, x1 = px-gx
        const bool reached = norm2d(rp.y - rg.y, rp.x - rg.x) < rrad[e];
        // epsilon-greedy (multi_human_rl.py:27-29, phase 'train'): with probability epsilon the env takes a uniformly
        // drawn table row instead (best = -2); a robot on its goal returns before the draw (:22-23).  Counter-based
        // stream: two 64-bit mixes of (seed, env) -- the caller passes a fresh seed per call.
        int choice = bi;
        bool explore = false;
        if (epsilon > 0.0 && !reached) {
            auto mix = [](unsigned long long z) {                      // splitmix64 finaliser
                z += 0x9E3779B97F4A7C15ull;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                return z ^ (z >> 31);
            };
            const unsigned long long r1 = mix(seed ^ mix((unsigned long long)e));
            const unsigned long long r2 = mix(r1);
            explore = (double)(r1 >> 11) * (1.0 / 9007199254740992.0) < epsilon;
            if (explore) choice = (int)(((r2 >> 32) * (unsigned long long)A) >> 32);
        }
        best[e] = reached ? -1 : (explore ? -2 : bi);
        best_val[e] = bv;
        if (action_out) {
            // what MultiHumanRL.predict returns: the table row of the best value, the zero action on the goal
            // (multi_human_rl.py:22-23) -- and also when every value is NaN (bi < 0: the host raises, as the reference)
            const bool zero = reached || choice < 0;
            const double2 act = reinterpret_cast<const double2 *>(actions)[zero ? 0 : choice];
            reinterpret_cast<double2 *>(action_out)[e] = zero ? make_double2(0.0, 0.0) : act;
        }
    }
}

// Persistent grid: two 4-wave workgroups per CU on the 256 CUs of an MI355X (fewer CUs: more passes, same result).
constexpr int kSarlMaxBlocks = (kSarlWaves >= 8 ? 1 : 2) * 256;

int launch_sarl(SarlParams &p, int32_t *best, double *best_val, double *action_out, double epsilon,
                unsigned long long seed, hipStream_t stream)
{
    const int blocks = (int)(p.c.ngroups < kSarlMaxBlocks ? p.c.ngroups : kSarlMaxBlocks);
    const dim3 grid(blocks), block(kSarlWaves * 64);
    if (p.om_init) {
        if (p.x.w_m1a) hipLaunchKernelGGL((sarl_value_kernel<true, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((sarl_value_kernel<false, true>), grid, block, 0, stream, p);
    } else {
        if (p.x.w_m1a) hipLaunchKernelGGL((sarl_value_kernel<true, false>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((sarl_value_kernel<false, false>), grid, block, 0, stream, p);
    }
    if (best) {
        hipLaunchKernelGGL(sarl_argmax_kernel, dim3(p.c.E), dim3(64), 0, stream, p.c.values, p.c.rpos, p.c.rgoal, p.c.rrad,
                           p.c.E, p.c.A, best, best_val, p.c.actions, action_out, epsilon, seed);
    }
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

int launch_sarl_argmax(const double *values, const double *rpos, const double *rgoal, const double *rrad, int E, int A,
                       int32_t *best, double *best_val, const double *actions, double *action_out, double epsilon,
                       unsigned long long seed, hipStream_t stream)
{
    hipLaunchKernelGGL(sarl_argmax_kernel, dim3(E), dim3(64), 0, stream, values, rpos, rgoal, rrad, E, A, best, best_val,
                       actions, action_out, epsilon, seed);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

int launch_sarl_c(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                  double gamma_pow, int kinematics, void *workspace, double *values, int32_t *best, double *best_val,
                  float *attention, const double *next_hpos, const double *next_hvel, const double *reward_in,
                  double *action_out, double epsilon, unsigned long long seed, int E, int N, const float *om_init,
                  hipStream_t stream)
{
    SarlParams p;
    const float4 *const *src = reinterpret_cast<const float4 *const *>(net);
    const float4 **dst = reinterpret_cast<const float4 **>(&p.f);
    static_assert(sizeof(SarlFrags) + sizeof(void *) == sizeof(mcn_sarl_net), "fragment tables must mirror the C struct");
    static_assert(sizeof(SarlX3) == sizeof(mcn_sarl_x3), "x3 fragment tables must mirror the C struct");
    for (size_t k = 0; k < sizeof(SarlFrags) / sizeof(float *); ++k) dst[k] = src[k];
    memset(&p.x, 0, sizeof(p.x));
    if (net->x3 && tuning_sarl_x3()) memcpy(&p.x, net->x3, sizeof(p.x));
    p.c = pair_params(st, actions, A, dt, gamma_pow, kinematics, values, next_hpos, next_hvel, reward_in, E, N, kSarlWaves);
    p.workspace = reinterpret_cast<float4 *>(workspace); p.attention = attention;
    p.om_init = reinterpret_cast<const float4 *>(om_init);
    return launch_sarl(p, best, best_val, action_out, epsilon, seed, stream);
}

long sarl_workspace_float4s(int E, int N, int A)
{
    const long waves = ((long)E * A + 15) / 16;
    long groups = (waves + kSarlWaves - 1) / kSarlWaves;
    if (groups > kSarlMaxBlocks) groups = kSarlMaxBlocks;          // one slot per RESIDENT wavefront
    // per wavefront: N humans x 12 rows (x3 layout) + 7 rows that no kernel uses any more (they held the parked global
    // half of attention.0): the size is public (mcn_sarl_workspace_bytes), shrinking it is a change of its own
    return groups * kSarlWaves * ((long)N * kWsRowsX3 + T100) * 64;
}

}  // namespace mcn
