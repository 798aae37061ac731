// sarl_om.hip -- OM-SARL's occupancy maps (crowd_nav/policy/multi_human_rl.py:109-163) and their share of mlp1.0, once per
// step, for gfx950 (MI355X).
//
// For every human i of an env: a 4 x 4 grid of cells centred on the human and turned so that +x is its velocity
// direction; per cell three channels -- 1 if any OTHER human of the env falls into it, and the mean of those humans'
// velocities in the turned frame.  The maps depend on the humans alone (in MultiHumanRL.predict they are built from the
// humans' next states of the first candidate action and reused for all of them, :46-49), so they are built here per
// (env, human) and not per (env, action, human) -- and so is everything mlp1.0 (61 -> 150) makes of them:
//
//   mlp1.0([x13 | om48]) = W[:, :13] x13 + (W[:, 13:] om48 + b)
//
// The bracket is this kernel's second output, `init`: the look-ahead (sarl_value.hip, WITH_OM) starts mlp1.0's
// accumulators from it instead of from the bias and runs the 13-wide layer it always ran.
//
// Arithmetic: float64 in the reference's (numpy's) operation sequence -- atan2 of the offset minus atan2 of the
// velocity, cos / sin of the difference times the distance -- and NOT the algebraically equal dot-product form:
// atan2(0.0, -0.0) is pi, so a still human whose stored vx is -0.0 is turned by pi in the reference.  A cell is decided
// by floor(): a coordinate within rounding noise of a cell edge may differ from numpy's libm (the tests keep 1e-9 away).
//
// Structure: one wavefront owns 16 consecutive (env, human) rows, row j on the lane's low four bits -- the layout of a
// 16 x 16 x 4 MFMA's B operand, so the finished map is, register by register, the input of the 48 -> 150 layer.
//   phase A  lane (j, q) tests the others k = q, q + 4, .. of row j: cell (or none) and turned velocity -> LDS
//   phase B  lane (j, q) owns map entries 16 t + 4 q + r (t < 3, r < 4): per entry the reference's sum(list) / len(list)
//            over the others IN INDEX ORDER, cast to float32
//   layer    dense<3, 10> on the fragments of W[:, 13:61] (mcn_pack_linear, natural input order) and mlp1.0's bias
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "lookahead_common.hpp"
#include "launch.hpp"

namespace mcn {

constexpr int kOmCells = 4, kOmChannels = 3;                        // [om] cell_num, om_channel_size of policy.config
constexpr int kOmWidth = kOmCells * kOmCells * kOmChannels;         // 48 inputs = three k-tiles
constexpr int kOmTiles = kOmWidth / 16, kOmOutTiles = 10;           // mlp1.0: 150 outputs in ten tiles
static_assert(kOmWidth % 16 == 0, "the map must fill whole input tiles");

struct OmParams {
    const double *hpos, *hvel;                // [E*N][2]
    const double *next_hpos, *next_hvel;      // [E*N][2] or both NULL
    const int32_t *hcount;                    // [E] or NULL
    const float4 *w, *b;                      // fragments [10][3][64] / [10][64], or both NULL: maps only
    float *om;                                // [E*N][48]
    float4 *init;                             // [E*N][40] (160 floats: tile n, slot 4q + r at 16 n + 4 q + r) or NULL
    double dt, cell_size;
    int E, N;
};

// position and velocity the map of a step is built from: the given next states, the current ones (dt = 0:
// MultiHumanRL.transform) or constant-velocity propagation (cadrl.py:104-129), as human_tile() in lookahead_common.hpp
struct OmHuman { double px, py, vx, vy; };
__device__ __forceinline__ OmHuman om_human(const OmParams &p, long ha)
{
    if (p.next_hpos) {
        const double2 np_ = reinterpret_cast<const double2 *>(p.next_hpos)[ha];
        const double2 nv_ = reinterpret_cast<const double2 *>(p.next_hvel)[ha];
        return {np_.x, np_.y, nv_.x, nv_.y};
    }
    const double2 hp = reinterpret_cast<const double2 *>(p.hpos)[ha];
    const double2 hv = reinterpret_cast<const double2 *>(p.hvel)[ha];
    if (p.dt == 0.0) return {hp.x, hp.y, hv.x, hv.y};
    return {hp.x + hv.x * p.dt, hp.y + hv.y * p.dt, hv.x, hv.y};
}

// floor(c / cell_size + cell_num / 2) as a cell index, -1 outside 0 .. 3; NaN and +-inf compare false and never reach
// the conversion (in numpy a NaN index is simply not in range(16))
__device__ __forceinline__ int om_index(double c, double cell_size)
{
    const double f = floor(c / cell_size + kOmCells / 2.0);
    return (f >= 0.0 && f < (double)kOmCells) ? (int)f : -1;
}

__global__ __launch_bounds__(64) void sarl_om_kernel(const OmParams p)
{
    __shared__ int s_cell[16][MCN_MAX_HUMANS];            // cell of other k in row j's grid, -1: none
    __shared__ double2 s_vel[16][MCN_MAX_HUMANS];         // its velocity in row j's frame
    const int lane = threadIdx.x, j = lane & 15, q = lane >> 4;
    const int N = p.N;
    const long rows = (long)p.E * N;
    long row = (long)blockIdx.x * 16 + j;
    const bool valid = row < rows;
    if (!valid) row = rows - 1;
    const long e = row / N;
    const int i = (int)(row - e * N);
    const int ne = humans_seen(p.hcount, e, N);
    const bool present = i < ne;                          // a human the policy does not see has no map (zeros)

    // ---- phase A ----
    const OmHuman me = om_human(p, row);
    const double thv = atan2(me.vy, me.vx);
    for (int k = q; k < N; k += 4) {
        int cell = -1;
        double2 v = make_double2(0.0, 0.0);
        if (present && k < ne && k != i) {
            const OmHuman o = om_human(p, e * N + k);
            const double dx = o.px - me.px, dy = o.py - me.py;
            const double rot = atan2(dy, dx) - thv;
            const double d = sqrt(dx * dx + dy * dy);
            const int ix = om_index(cos(rot) * d, p.cell_size), iy = om_index(sin(rot) * d, p.cell_size);
            if (ix >= 0 && iy >= 0) {
                cell = kOmCells * iy + ix;
                const double rv = atan2(o.vy, o.vx) - thv;
                const double speed = sqrt(o.vx * o.vx + o.vy * o.vy);
                v = make_double2(cos(rv) * speed, sin(rv) * speed);
            }
        }
        s_cell[j][k] = cell;
        s_vel[j][k] = v;
    }
    __syncthreads();

    // ---- phase B: entries 16 t + 4 q + r of row j; entry f is channel f % 3 of cell f / 3 ----
    double sum[kOmTiles][4];
    int cnt[kOmTiles][4];
#pragma unroll
    for (int t = 0; t < kOmTiles; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { sum[t][r] = 0.0; cnt[t][r] = 0; }
    for (int k = 0; k < N; ++k) {
        const int cell = s_cell[j][k];
        const double2 v = s_vel[j][k];
#pragma unroll
        for (int t = 0; t < kOmTiles; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 16 * t + 4 * q + r, ch = f % kOmChannels;
                if (cell == f / kOmChannels) {
                    sum[t][r] = sum[t][r] + (ch == 0 ? 1.0 : (ch == 1 ? v.x : v.y));
                    cnt[t][r] += 1;
                }
            }
    }
    f32x4 x[kOmTiles];
#pragma unroll
    for (int t = 0; t < kOmTiles; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[t][r] = cnt[t][r] ? (float)(sum[t][r] / (double)cnt[t][r]) : 0.0f;
        if (valid) reinterpret_cast<float4 *>(p.om + row * kOmWidth)[4 * t + q] = make_float4(x[t][0], x[t][1], x[t][2], x[t][3]);
    }

    // ---- the maps' share of mlp1.0, bias included ----
    if (!p.init) return;                                  // (uniform)
    f32x4 out[kOmOutTiles];
    dense<kOmTiles, kOmOutTiles, kLinear, kBiasFrag>(x, out, p.w, p.b, lane);
    if (valid) {
#pragma unroll
        for (int n = 0; n < kOmOutTiles; ++n)
            p.init[row * (kOmOutTiles * 4) + 4 * n + q] = make_float4(out[n][0], out[n][1], out[n][2], out[n][3]);
    }
}

int launch_sarl_om(const mcn_env_state *st, double dt, const double *next_hpos, const double *next_hvel,
                   double cell_size, const float *w_om, const float *b_om, float *om, float *init, int E, int N,
                   hipStream_t stream)
{
    OmParams p;
    p.hpos = st->hpos; p.hvel = st->hvel; p.next_hpos = next_hpos; p.next_hvel = next_hvel; p.hcount = st->hcount;
    p.w = reinterpret_cast<const float4 *>(w_om); p.b = reinterpret_cast<const float4 *>(b_om);
    p.om = om; p.init = reinterpret_cast<float4 *>(init);
    p.dt = dt; p.cell_size = cell_size; p.E = E; p.N = N;
    const long blocks = ((long)E * N + 15) / 16;
    hipLaunchKernelGGL(sarl_om_kernel, dim3((unsigned)blocks), dim3(64), 0, stream, p);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace mcn
