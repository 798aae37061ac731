// social_force.hpp -- one human's social-force velocity (MCN_HUMANS_SOCIALFORCE, include/mcn.h).
//
// Circular form of Helbing, Farkas and Vicsek (2000), no body-contact or friction terms: relaxation towards the
// goal-directed desired velocity plus one exponential repulsion per other agent, integrated over one time step and
// clipped to the preferred speed.  All float64, one IEEE operation per line of the definition in this order (the build
// has contraction off), so that only exp may differ from a host evaluation:
//   e = goal - pos, clipped to length v_pref (the vector orca.py:113 hands to rvo2)
//   a = k (e - v) + sum_j A exp((r + r_j - dist_j) / B) (pos - pos_j) / dist_j       j in index order, the robot last
//   w = v + a dt, clipped to length v_pref
// The other humans come from the float64 LDS tiles the step kernel stages for its overlap count.
#pragma once
#include <hip/hip_runtime.h>

namespace mcn {

struct SocialForce { double strength, range, relaxation_rate; };      // A (m/s^2), B (m), k (1/s)

__device__ __forceinline__ void sf_repel(double &ax, double &ay, double px, double py, double r, double2 q, double rq,
                                         const SocialForce &f)
{
    const double dx = px - q.x, dy = py - q.y;
    const double dist = sqrt(dx * dx + dy * dy);
    if (dist > 0) {                                       // a coincident agent has no direction: contributes nothing
        const double m = f.strength * exp((r + rq - dist) / f.range);
        ax = ax + m * (dx / dist);
        ay = ay + m * (dy / dist);
    }
}

// sPosD / sRadD: the block's staged humans; gbase: tile index of human 0 of this env, h: my index, N: humans per env.
// with_robot: the humans see the robot (cfg.robot_visible); rob / rob_rad: its position and plain radius.
// NT > 0: N known at compile time, the loop over the others is unrolled (their independent sqrt / exp / division chains
// overlap; the sum keeps its order).
template <int NT>
__device__ __forceinline__ double2 social_force_velocity(double2 pos, double2 vel, double2 goal, double rad, double v_pref,
                                                         const double2 *sPosD, const double *sRadD, int gbase, int h, int N,
                                                         bool with_robot, double2 rob, double rob_rad,
                                                         const SocialForce &f, double dt)
{
    double ex = goal.x - pos.x, ey = goal.y - pos.y;
    const double d = sqrt(ex * ex + ey * ey);
    if (d > v_pref) { ex = ex / d * v_pref; ey = ey / d * v_pref; }
    double ax = f.relaxation_rate * (ex - vel.x), ay = f.relaxation_rate * (ey - vel.y);
    if constexpr (NT > 0) {
#pragma unroll
        for (int c = 0; c < NT - 1; ++c) {
            const int j = c + (c >= h);
            sf_repel(ax, ay, pos.x, pos.y, rad, sPosD[gbase + j], sRadD[gbase + j], f);
        }
    } else {
        for (int c = 0; c < N - 1; ++c) {
            const int j = c + (c >= h);                   // the others in index order, every lane busy in every round
            sf_repel(ax, ay, pos.x, pos.y, rad, sPosD[gbase + j], sRadD[gbase + j], f);
        }
    }
    if (with_robot) sf_repel(ax, ay, pos.x, pos.y, rad, rob, rob_rad, f);
    double wx = vel.x + ax * dt, wy = vel.y + ay * dt;
    const double n = sqrt(wx * wx + wy * wy);
    if (n > v_pref) { wx = wx / n * v_pref; wy = wy / n * v_pref; }
    return make_double2(wx, wy);
}

}  // namespace mcn
