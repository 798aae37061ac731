// env_step_params.hpp -- kernel argument block of env_step_kernel (passed by value).
#pragma once
#include <stdint.h>
#include "../../include/mcn.h"

namespace mcn {

// Limits that the kernels and the dispatch (env_dispatch.hpp) share; here because this header needs no HIP.
constexpr int kMaxLines = 10;          // ORCA line slots per agent (orca_device.hpp)
// longest discount table the dispatcher accepts for env_pair_kernel (longer ones stay on env_step_kernel)
constexpr int kPairDiscMax = 128;

struct StepParams {
    mcn_env_cfg cfg;
    mcn_env_state st;
    mcn_env_out out;
    mcn_rollout roll;
    const double *actions;
    const double *given_v;
    int E, N, G, update, has_roll;
    int nl_cap;   // LDS line slots per lane
    // The unused_* members held host-only dispatch inputs (quad_max_envs, force_generic, quad_split, step_block,
    // pair_stream) until the dispatch moved to env_dispatch.hpp.  No code reads or writes them; they stay as padding so
    // that sizeof and the offset of every member a kernel reads, and with them the kernels' argument loads, are unchanged.
    int unused_0, unused_1;
    int debug_noop;      // mcn_tuning.diag_noop, DIAGNOSTIC BUILD ONLY: kernels return at entry (launch-floor measurement)
    int unused_2, unused_3;
    int lp3_defer;       // 0 / 1 (StepPlan.lp3_defer): the compile-time-N ORCA kernels park their 3-D LPs in out.lp3_queue
    int unused_4;
    // MCN_HUMANS_SOCIALFORCE only (mcn_env_step_sf / mcn_env_rollout_sf / mcn_env_rollout_orca_sf): A (m/s^2), B (m),
    // k (1/s) of social_force.hpp
    double sf_strength, sf_range, sf_relaxation_rate;
};

// mcn_env_rollout_orca / mcn_env_rollout_orca_sf only (env_step.hip: env_step_loop_orca_kernel and its social-force
// twin): the robot's own ORCA parameters and the per-step trace arrays, each of which may be NULL.  A second kernel
// argument, so that StepParams stays what the other kernels take.
struct ClosedLoop {
    double safety_space;               // the robot policy's: a radius goes float32 as (radius + 0.01) + safety_space (orca.py:100,103)
    float neighbor_dist, time_horizon;
    int max_neighbors;
    double *tr_robot;                  // [T][E][5]
    double *tr_humans;                 // [T][E][N][4]
    double *tr_hrad;                   // [T][E][N]
    double *tr_action;                 // [T][E][2]
    mcn_step_rec *tr_rec;              // [T][E]
    double *tr_human_act;              // [T][E][N][2]
};

}  // namespace mcn
