// orca_finish.hip -- CrowdSim.get_human_times (crowd_sim/envs/crowd_sim.py:219-258) for E envs in ONE launch.
//
// Once the robot has arrived the reference puts everybody -- the robot as agent 0, then the humans, each at its own
// radius and v_pref -- into one centralised rvo2 simulation and steps it until every human has reached its goal.  Here
// one lane is one agent, floor(64 / (N + 1)) envs share a wavefront (the lane-per-human layout of env_step.hip), the
// env's agent tile lives in LDS and the step loop runs inside the kernel: "is everybody there" is a ballot instead of
// a device round trip per simulated step.  The arithmetic and its order are the contract of mcn_orca_finish in
// include/mcn.h; float64 only for the preferred velocity, the clock and the arrival test.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "orca_device.hpp"
#include "launch.hpp"

namespace mcn {

// The other N agents of the lane's env, in agent-index order, from one buffer of the tile (the lane's own slot skipped).
struct TileCand {
    const float4 *pv; const float *rad;     // the wavefront's tile: (px, py, vx, vy) and radius per lane
    int base, k;                            // lane of agent 0 of my env, my agent index
    __device__ __forceinline__ void fetch(int c, float4 &o, float &r) const {
        const int j = base + c + (c >= k);
        o = pv[j]; r = rad[j];
    }
};

constexpr int kFinishBlock = 64;            // one wavefront per workgroup: envs never straddle wavefronts

struct FinishParams {
    mcn_env_state st;
    float *sim_vel; const uint8_t *select; int32_t *steps; float *traj;
    double time_step;
    float neighbor_dist, time_horizon;
    int max_neighbors, max_steps, E, N, nl_cap;
};

__global__ __launch_bounds__(kFinishBlock) void orca_finish_kernel(const FinishParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4 *sL  = reinterpret_cast<float4 *>(smem);                        // [nl_cap][64] half-planes
    float4 *sPV = sL + (size_t)p.nl_cap * kFinishBlock;                    // [2][64] agent tile, two buffers
    float  *sR  = reinterpret_cast<float *>(sPV + 2 * kFinishBlock);       // [64] radii (constant)

    const int lane = threadIdx.x;
    const int A = p.N + 1;                  // agents per env, <= 33
    const int G = kFinishBlock / A;         // envs per wavefront, >= 1
    const int g = lane / A;
    const int k = lane - g * A;             // 0 = robot, 1 .. N = humans
    const long e = (long)blockIdx.x * G + g;
    const bool in_grid = (g < G) && (e < p.E);
    const bool active = in_grid && (!p.select || p.select[e] != 0);
    const unsigned long long env_mask = ((1ull << A) - 1ull) << (g * A);     // my env's lanes (g * A <= 63, A <= 33)
    const long hi = active ? e * p.N + (k > 0 ? k - 1 : 0) : 0;       // my human's row (humans only)

    double2 p64 = make_double2(0, 0), goal = p64;
    double rad64 = 0, gtime = 0, ht = 1.0;
    float vmax = 0;
    float2 vel = make_float2(0, 0);
    if (active) {
        if (k == 0) {
            p64  = reinterpret_cast<const double2 *>(p.st.rpos)[e];
            goal = reinterpret_cast<const double2 *>(p.st.rgoal)[e];
            rad64 = p.st.rrad[e];
            vmax = (float)p.st.rvpref[e];
        } else {
            p64  = reinterpret_cast<const double2 *>(p.st.hpos)[hi];
            goal = reinterpret_cast<const double2 *>(p.st.hgoal)[hi];
            rad64 = p.st.hrad[hi];
            vmax = (float)p.st.hvpref[hi];
            ht = p.st.human_times[hi];
        }
        gtime = p.st.gtime[e];
        vel = reinterpret_cast<const float2 *>(p.sim_vel)[e * A + k];
    }
    float2 p32 = make_float2((float)p64.x, (float)p64.y);
    const float frad = (float)rad64;
    const float fdt = (float)p.time_step;
    sR[lane] = frad;

    const TileCand cand0{sPV, sR, lane - k, k};
    const LdsLines L{sL + lane, kFinishBlock};
    int taken = 0;
    for (int t = 0; t < p.max_steps; ++t) {
        // an env goes on while one of its humans has no arrival time; the wavefront while one of its envs goes on
        const unsigned long long pending = __ballot(active && ht == 0.0);
        if (pending == 0ull) break;
        const bool live = active && (pending & env_mask) != 0ull;
        // every lane publishes its own slot only, into the buffer last read two steps ago: the barrier of the step
        // in between is behind those reads, so one barrier per step is enough and everybody solves against the old state
        float4 *tile = sPV + (t & 1) * kFinishBlock;
        tile[lane] = make_float4(p32.x, p32.y, vel.x, vel.y);
        __syncthreads();
        if (live) {
            double ex = goal.x - p64.x, ey = goal.y - p64.y;
            const double n = sqrt(ex * ex + ey * ey);
            if (n > 1.0) { ex = ex / n; ey = ey / n; }
            TileCand cand = cand0;
            cand.pv = tile;
            float ox, oy;
            orca_solve(cand, p.N, p32.x, p32.y, vel.x, vel.y, frad, vmax, (float)ex, (float)ey,
                       p.neighbor_dist, p.max_neighbors, p.time_horizon, fdt, L, ox, oy);
            vel = make_float2(ox, oy);
            p32.x = p32.x + vel.x * fdt;
            p32.y = p32.y + vel.y * fdt;
            gtime += p.time_step;
            if (ht == 0.0) {
                const double dx = p64.x - goal.x, dy = p64.y - goal.y;
                if (sqrt(dx * dx + dy * dy) < rad64) ht = gtime;
            }
            p64 = make_double2((double)p32.x, (double)p32.y);
            if (p.traj) reinterpret_cast<float2 *>(p.traj)[((long)t * p.E + e) * A + k] = p32;
            ++taken;
        }
    }

    if (in_grid && k == 0) p.steps[e] = taken;
    if (taken > 0) {                                    // (implies active)
        reinterpret_cast<float2 *>(p.sim_vel)[e * A + k] = vel;
        if (k == 0) {
            reinterpret_cast<double2 *>(p.st.rpos)[e] = p64;
            p.st.gtime[e] = gtime;
        } else {
            reinterpret_cast<double2 *>(p.st.hpos)[hi] = p64;
            p.st.human_times[hi] = ht;
        }
    }
}

int launch_orca_finish(const mcn_env_state &st, float *sim_vel, const uint8_t *select, int max_steps, int32_t *steps,
                       float *traj, double time_step, float neighbor_dist, int max_neighbors, float time_horizon,
                       int E, int N, hipStream_t stream)
{
    FinishParams p;
    p.st = st; p.sim_vel = sim_vel; p.select = select; p.steps = steps; p.traj = traj;
    p.time_step = time_step; p.neighbor_dist = neighbor_dist; p.time_horizon = time_horizon;
    p.max_neighbors = max_neighbors; p.max_steps = max_steps; p.E = E; p.N = N;
    p.nl_cap = max_neighbors < N ? (max_neighbors > 0 ? max_neighbors : 1) : N;
    const int G = kFinishBlock / (N + 1);
    const int blocks = (E + G - 1) / G;
    const size_t sm = (size_t)kFinishBlock * (16u * p.nl_cap + 2u * 16u + 4u);
    hipLaunchKernelGGL(orca_finish_kernel, dim3(blocks), dim3(kFinishBlock), sm, stream, p);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace mcn
