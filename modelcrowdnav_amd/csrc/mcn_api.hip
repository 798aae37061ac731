// mcn_api.hip -- extern "C" entry points of libmcn_hip.so (see include/mcn.h).
// Argument validation happens here, on the host, before any kernel is launched: a kernel
// is never started on shapes its indexing does not assume.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <mutex>
#include "../../include/mcn.h"

#include "env_step_params.hpp"
#include "env_dispatch.hpp"
#include "launch.hpp"
#include "lp3_queue.hpp"

// Dispatch overrides (include/mcn.h: mcn_tuning).  The MCN_* environment variables are read ONCE, the first time a
// launch needs them, as the initial values; after that only mcn_set_tuning changes them.  No getenv on the launch path.
static mcn_tuning g_tuning;
static bool g_tuning_init = false;
static std::mutex g_tuning_mu;          // launches copy the settings under it: a concurrent mcn_set_tuning never tears them
static int env_or(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}
static mcn_tuning tuning_from_env()
{
    mcn_tuning t;
    memset(&t, 0, sizeof(t));
    t.force_generic = env_or("MCN_FORCE_GENERIC", 0);
    t.quad_max_envs = env_or("MCN_QUAD_MAX_ENVS", -1);
    t.quad_split = env_or("MCN_QUAD_SPLIT", -1);
    t.rollout_fused = env_or("MCN_ROLLOUT_FUSED", -1);
    t.rollout_split = env_or("MCN_ROLLOUT_SPLIT", -1);
    t.step_block = env_or("MCN_STEP_BLOCK", -1);
    t.pair_stream = env_or("MCN_PAIR_STREAM", -1);
    t.lp3_defer = env_or("MCN_LP3_DEFER", -1);
    t.sarl_x3 = env_or("MCN_SARL_X3", -1);
    return t;
}
static mcn_tuning tuning()
{
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    if (!g_tuning_init) { g_tuning = tuning_from_env(); g_tuning_init = true; }
    return g_tuning;
}

namespace mcn { bool tuning_sarl_x3() { return tuning().sarl_x3 != 0; } }

namespace mcn {

// A hyper-parameter that the C ABI carries as float32 (mcn_adam_step's lr, betas and eps; mcn_mlp_world_loss_grad's and
// mcn_dropout_mask's drop_p), as the float64 that was written.
// torch applies the hyper-parameters as the Python floats (float64) the user wrote -- 1e-3, 0.9, 0.999, 1e-8 -- and the C
// ABI carries them as float32, 5e-8 away.  That is enough to show: lr 0.001f in place of 0.001 moves every step by 5e-8 of
// itself, and on the recorded reference run (tests/golden/g20_trainer_sim.npz) that flipped one ReLU of one row at the
// sixth step, after which single weights were 2.6e-5 from the float64 replay instead of 8e-8.  So the float64 is
// recovered: the shortest decimal that rounds to the given float32, which is what was written for anything of up to 7
// digits.
double written_as(float x)
{
    char buf[40];
    for (int digits = 1; digits <= 8; ++digits) {
        snprintf(buf, sizeof buf, "%.*e", digits - 1, (double)x);
        if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
    }
    return (double)x;
}

}  // namespace mcn

// bf16 round-to-nearest-even of a float32 (NaN kept quiet), as the device's v_cvt_pk_bf16_f32
static uint16_t bf16_rne(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_to_f32(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

int64_t mcn_pack_x3_bytes(int32_t NT, int32_t KT)
{
    if (NT <= 0 || KT <= 0) return 0;
    return (int64_t)NT * ((KT + 1) / 2) * 3 * 64 * 8 * 2;
}

int mcn_pack_x3(const float *wfrag, int32_t NT, int32_t KT, void *x3_out)
{
    if (!wfrag || !x3_out || NT <= 0 || KT <= 0) return MCN_EINVAL;
    const int KB = (KT + 1) / 2;
    uint16_t *out = reinterpret_cast<uint16_t *>(x3_out);
    for (int n = 0; n < NT; ++n)
        for (int m = 0; m < KB; ++m)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 8; ++s) {
                    // k-slot 8 q + s of input block m = slot 4 q + (s & 3) of k-tile 2 m + (s >> 2)
                    const int t = 2 * m + (s >> 2);
                    const float w = t < KT ? wfrag[(((size_t)n * KT + t) * 64 + lane) * 4 + (s & 3)] : 0.0f;
                    const uint16_t hi = bf16_rne(w);
                    const float r1 = w - bf16_to_f32(hi);
                    const uint16_t mid = bf16_rne(r1);
                    const float r2 = r1 - bf16_to_f32(mid);
                    const size_t at = (((size_t)n * KB + m) * 3 * 64 + lane) * 8 + s;
                    out[at] = hi; out[at + 64 * 8] = mid; out[at + 2 * 64 * 8] = bf16_rne(r2);
                }
    return MCN_OK;
}

// mcn_last_dispatch(): the family of the plan the env entry points ran last (per host thread; env_dispatch.hpp: family_name)
static thread_local const char *g_last_dispatch = "";
const char *mcn_last_dispatch(void) { return g_last_dispatch; }
// mcn_last_rollout_form(): the form of mcn_env_rollout's last plan, -1 unless that was the fused quad rollout
static thread_local int32_t g_last_rollout_form = -1;
int32_t mcn_last_rollout_form(void) { return g_last_rollout_form; }

int32_t mcn_abi_version(void) { return MCN_ABI_VERSION; }
int64_t mcn_sizeof(int32_t which)
{
    switch (which) {
        case MCN_SIZEOF_ENV_CFG: return sizeof(mcn_env_cfg);
        case MCN_SIZEOF_ENV_STATE: return sizeof(mcn_env_state);
        case MCN_SIZEOF_ENV_OUT: return sizeof(mcn_env_out);
        case MCN_SIZEOF_ROLLOUT: return sizeof(mcn_rollout);
        case MCN_SIZEOF_TUNING: return sizeof(mcn_tuning);
        case MCN_SIZEOF_STEP_REC: return sizeof(mcn_step_rec);
        case MCN_SIZEOF_ROLL_REC: return sizeof(mcn_roll_rec);
        case MCN_SIZEOF_SARL_NET: return sizeof(mcn_sarl_net);
        case MCN_SIZEOF_SGAN_NET: return sizeof(mcn_sgan_net);
        case MCN_SIZEOF_SCENARIO_CFG: return sizeof(mcn_scenario_cfg);
        case MCN_SIZEOF_MLP_WORLD_NET: return sizeof(mcn_mlp_world_net);
        case MCN_SIZEOF_ATTN_WORLD_NET: return sizeof(mcn_attn_world_net);
        case MCN_SIZEOF_SARL_X3: return sizeof(mcn_sarl_x3);
        case MCN_SIZEOF_LSTM_RL_NET: return sizeof(mcn_lstm_rl_net);
        case MCN_SIZEOF_CADRL_NET: return sizeof(mcn_cadrl_net);
        default: return -1;
    }
}

// Validates one env-step problem and fills the kernel argument block; which kernel takes it is env_dispatch.hpp's to
// say.  Shared by mcn_env_step / mcn_env_rollout and their social-force twins: `social_force` says which family the
// caller is, and the cfg's policy must belong to it.  `tu`: the caller's snapshot of the tuning.
static int fill_step_params(mcn::StepParams &p, const mcn_tuning &tu, const mcn_env_cfg *cfg, const mcn_env_state *st,
                            const double *actions, const double *given_v, const mcn_env_out *out, const mcn_rollout *roll,
                            int32_t E, int32_t N, int32_t update, bool social_force = false, bool needs_actions = true)
{
    if (!cfg || !st || !out || (needs_actions && !actions)) return MCN_EINVAL;
    if (E <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (!st->hpos || !st->hvel || !st->hgoal || !st->hrad || !st->hvpref || !st->rpos || !st->rvel || !st->rgoal ||
        !st->rrad || !st->gtime) return MCN_EINVAL;
    if (cfg->robot_kinematics == MCN_KIN_UNICYCLE && !st->rtheta) return MCN_EINVAL;
    if (!out->rec) return MCN_EINVAL;
    if (!update && (!out->nobs_pos || !out->nobs_vel)) return MCN_EINVAL;
    if (cfg->human_policy == MCN_HUMANS_GIVEN && !given_v) return MCN_EINVAL;
    if (social_force) {
        if (cfg->human_policy != MCN_HUMANS_SOCIALFORCE) return MCN_EINVAL;
    } else if (cfg->human_policy < MCN_HUMANS_ORCA || cfg->human_policy > MCN_HUMANS_GIVEN) return MCN_EINVAL;
    if (cfg->orca_max_neighbors < 0 || cfg->orca_max_neighbors > MCN_MAX_LINES) return MCN_EINVAL;
    if (!(cfg->time_step > 0)) return MCN_EINVAL;
    if (roll) {
        if (roll->state && (!roll->disc_table || roll->disc_len <= 0 || roll->fin_slots < 1)) return MCN_EINVAL;
        if (roll->pool_hpos && !roll->state) return MCN_EINVAL;
        if (roll->pool_hpos && (!roll->pool_hgoal || !roll->pool_hrad || !roll->pool_hvpref || roll->pool_size <= 0)) return MCN_EINVAL;
        if (roll->pool_hpos && (roll->case_stride < 0 || roll->case_stride >= roll->pool_size)) return MCN_EINVAL;
    }
    memset(&p, 0, sizeof(p));
    p.cfg = *cfg; p.st = *st; p.out = *out;
    if (roll) { p.roll = *roll; p.has_roll = 1; }
    p.actions = actions; p.given_v = given_v;
    p.E = E; p.N = N; p.G = 64 / N; p.update = update ? 1 : 0;
    int ncand = N - 1 + (cfg->robot_visible ? 1 : 0);
    int nl = ncand < cfg->orca_max_neighbors ? ncand : cfg->orca_max_neighbors;
    if (cfg->human_policy != MCN_HUMANS_ORCA) nl = 0;
    p.nl_cap = nl;
#ifdef MCN_DIAG
    p.debug_noop = tu.diag_noop;
#endif
    return MCN_OK;
}

static int launched() { return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH; }

// T single steps as planned, step t on actions[t][E][2] (mcn_env_step: T = 1)
static int run_steps(mcn::StepParams &p, const mcn::StepPlan &plan, const double *actions, int32_t T, hipStream_t stream)
{
    g_last_dispatch = mcn::family_name(plan.family);
    p.lp3_defer = plan.lp3_defer ? 1 : 0;
    for (int32_t t = 0; t < T; ++t) {
        p.actions = actions + (size_t)t * p.E * 2;
        mcn::launch_env_step(p, plan, stream);
        const int rc = launched();
        if (rc != MCN_OK) return rc;
    }
    return MCN_OK;
}

static int run_rollout(mcn::StepParams &p, const mcn::RolloutPlan &plan, const double *actions, int32_t T, hipStream_t stream)
{
    switch (plan.family) {
        case mcn::kRolloutQuad: mcn::launch_env_rollout_quad(p, plan.form, T, stream); break;
        case mcn::kStepLoop:    mcn::launch_env_step_loop(p, T, stream); break;
        case mcn::kStepLoopSf:  mcn::launch_env_step_loop_sf(p, T, stream); break;
        default:                return run_steps(p, plan.step, actions, T, stream);
    }
    g_last_dispatch = mcn::family_name(plan.family);
    return launched();
}

// the model's parameters (include/mcn.h): A >= 0, B > 0, k >= 0, all finite
static bool sf_params_ok(double strength, double range, double relaxation_rate)
{
    return isfinite(strength) && isfinite(range) && isfinite(relaxation_rate) && strength >= 0 && range > 0 &&
           relaxation_rate >= 0;
}

// mcn_env_rollout_orca and its social-force twin: validation, argument blocks and the one launch.  `sf`: NULL for ORCA or
// linear humans, else {strength, range, relaxation_rate} (checked by the caller) for social-force ones.
static int closed_loop_rollout(const mcn_env_cfg *cfg, const double *sf, const mcn_env_state *st,
                               double robot_safety_space, float neighbor_dist, int32_t max_neighbors, float time_horizon,
                               int32_t T, const mcn_env_out *out, const mcn_rollout *roll, double *tr_robot,
                               double *tr_humans, double *tr_hrad, double *tr_action, mcn_step_rec *tr_rec,
                               double *tr_human_act, int32_t E, int32_t N, void *stream)
{
    if (!cfg || !st || !out || T < 1) return MCN_EINVAL;
    if (max_neighbors < 0 || max_neighbors > MCN_MAX_LINES) return MCN_EINVAL;
    if (!(time_horizon > 0) || !(cfg->time_step > 0) || !((float)cfg->time_step > 0)) return MCN_EINVAL;
    if (!isfinite(robot_safety_space)) return MCN_EINVAL;
    if (cfg->robot_kinematics != MCN_KIN_HOLONOMIC) return MCN_EINVAL;          // the ORCA robot is holonomic
    if (sf ? cfg->human_policy != MCN_HUMANS_SOCIALFORCE
           : cfg->human_policy != MCN_HUMANS_ORCA && cfg->human_policy != MCN_HUMANS_LINEAR) return MCN_EINVAL;
    if (!st->rvpref) return MCN_EINVAL;                                         // the robot's max speed
    mcn::StepParams p;
    const int rc = fill_step_params(p, tuning(), cfg, st, nullptr, nullptr, out, roll, E, N, 1, sf != nullptr, false);
    if (rc != MCN_OK) return rc;
    // line slots per lane: the larger of what a human's solve and the robot's solve (all N humans as candidates) can fill.
    // Social-force humans fill none: there the robot's 3-D LP keeps its projected lines (one fewer than its lines at most)
    // in rows behind its own
    const int rob_nl = max_neighbors < N ? max_neighbors : N;
    if (sf) p.nl_cap = rob_nl + (rob_nl > 0 ? rob_nl - 1 : 0);
    else if (rob_nl > p.nl_cap) p.nl_cap = rob_nl;
    mcn::ClosedLoop cl;
    memset(&cl, 0, sizeof(cl));
    cl.safety_space = robot_safety_space;       // added after the 0.01, in the reference's order (orca.py:100,103)
    cl.neighbor_dist = neighbor_dist; cl.time_horizon = time_horizon; cl.max_neighbors = max_neighbors;
    cl.tr_robot = tr_robot; cl.tr_humans = tr_humans; cl.tr_hrad = tr_hrad; cl.tr_action = tr_action;
    cl.tr_rec = tr_rec; cl.tr_human_act = tr_human_act;
    if (sf) {
        p.sf_strength = sf[0]; p.sf_range = sf[1]; p.sf_relaxation_rate = sf[2];
        g_last_dispatch = mcn::family_name(mcn::kStepLoopOrcaSf);
        mcn::launch_env_step_loop_orca_sf(p, cl, T, (hipStream_t)stream);
    } else {
        g_last_dispatch = mcn::family_name(mcn::kStepLoopOrca);
        mcn::launch_env_step_loop_orca(p, cl, T, (hipStream_t)stream);
    }
    return launched();
}

extern "C" {

#ifdef MCN_DIAG
const char *mcn_version(void) { return "modelcrowdnav_amd 0.4 (gfx950) DIAGNOSTIC BUILD (time stamps)"; }
#else
const char *mcn_version(void) { return "modelcrowdnav_amd 0.4 (gfx950)"; }
#endif

int mcn_set_tuning(const mcn_tuning *t)
{
    std::lock_guard<std::mutex> lock(g_tuning_mu);
    if (!t) { g_tuning = tuning_from_env(); g_tuning_init = true; return MCN_OK; }
    if (t->quad_split > 1 || t->rollout_fused > 1 || t->rollout_split > 2 || t->pair_stream > 3 || t->force_generic < 0 || t->force_generic > 1) return MCN_EINVAL;
    if (t->quad_max_envs < -1 || t->quad_split < -1 || t->rollout_fused < -1 || t->rollout_split < -1 || t->pair_stream < -1) return MCN_EINVAL;
    if (t->step_block != -1 && t->step_block != 64 && t->step_block != 256) return MCN_EINVAL;
    if (t->lp3_defer < -1 || t->lp3_defer > 1) return MCN_EINVAL;
    if (t->sarl_x3 < -1 || t->sarl_x3 > 1) return MCN_EINVAL;
#ifndef MCN_DIAG
    if (t->diag_noop) return MCN_EINVAL;          // kernels that do nothing exist in the diagnostic build only
#endif
    g_tuning = *t;
    g_tuning_init = true;
    return MCN_OK;
}

int mcn_get_tuning(mcn_tuning *t)
{
    if (!t) return MCN_EINVAL;
    *t = tuning();
    return MCN_OK;
}

int64_t mcn_env_lp3_queue_bytes(int32_t E, int32_t N)
{
    if (E <= 0 || N < 2 || N > 10) return 0;          // the compile-time-N ORCA kernels (env_step.hip)
    return mcn::lp3_queue_bytes(E, N, N < MCN_MAX_LINES ? N : MCN_MAX_LINES);
}

int mcn_env_step(const mcn_env_cfg *cfg, const mcn_env_state *st, const double *actions,
                 const double *given_v, const mcn_env_out *out, const mcn_rollout *roll,
                 int32_t E, int32_t N, int32_t update, void *stream)
{
    const mcn_tuning tu = tuning();
    mcn::StepParams p;
    const int rc = fill_step_params(p, tu, cfg, st, actions, given_v, out, roll, E, N, update);
    if (rc != MCN_OK) return rc;
    return run_steps(p, mcn::plan_env_step(p, tu), actions, 1, (hipStream_t)stream);
}

int mcn_env_rollout(const mcn_env_cfg *cfg, const mcn_env_state *st, const double *actions, int32_t T,
                    const mcn_env_out *out, const mcn_rollout *roll, int32_t E, int32_t N, void *stream)
{
    if (T <= 0) return MCN_EINVAL;
    const mcn_tuning tu = tuning();
    mcn::StepParams p;
    const int rc = fill_step_params(p, tu, cfg, st, actions, nullptr, out, roll, E, N, 1);
    if (rc != MCN_OK) return rc;
    const mcn::RolloutPlan plan = mcn::plan_env_rollout(p, T, tu);
    g_last_rollout_form = plan.form;
    return run_rollout(p, plan, actions, T, (hipStream_t)stream);
}

int mcn_env_rollout_orca(const mcn_env_cfg *cfg, const mcn_env_state *st, double robot_safety_space,
                         float neighbor_dist, int32_t max_neighbors, float time_horizon, int32_t T,
                         const mcn_env_out *out, const mcn_rollout *roll, double *tr_robot, double *tr_humans,
                         double *tr_hrad, double *tr_action, mcn_step_rec *tr_rec, double *tr_human_act,
                         int32_t E, int32_t N, void *stream)
{
    return closed_loop_rollout(cfg, nullptr, st, robot_safety_space, neighbor_dist, max_neighbors, time_horizon, T, out,
                               roll, tr_robot, tr_humans, tr_hrad, tr_action, tr_rec, tr_human_act, E, N, stream);
}

int mcn_env_rollout_orca_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                            const mcn_env_state *st, double robot_safety_space, float neighbor_dist,
                            int32_t max_neighbors, float time_horizon, int32_t T, const mcn_env_out *out,
                            const mcn_rollout *roll, double *tr_robot, double *tr_humans, double *tr_hrad,
                            double *tr_action, mcn_step_rec *tr_rec, double *tr_human_act, int32_t E, int32_t N,
                            void *stream)
{
    if (!sf_params_ok(strength, range, relaxation_rate)) return MCN_EINVAL;
    const double sf[3] = {strength, range, relaxation_rate};
    return closed_loop_rollout(cfg, sf, st, robot_safety_space, neighbor_dist, max_neighbors, time_horizon, T, out, roll,
                               tr_robot, tr_humans, tr_hrad, tr_action, tr_rec, tr_human_act, E, N, stream);
}

int mcn_env_step_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                    const mcn_env_state *st, const double *actions, const mcn_env_out *out,
                    const mcn_rollout *roll, int32_t E, int32_t N, int32_t update, void *stream)
{
    if (!sf_params_ok(strength, range, relaxation_rate)) return MCN_EINVAL;
    const mcn_tuning tu = tuning();
    mcn::StepParams p;
    const int rc = fill_step_params(p, tu, cfg, st, actions, nullptr, out, roll, E, N, update, true);
    if (rc != MCN_OK) return rc;
    p.sf_strength = strength; p.sf_range = range; p.sf_relaxation_rate = relaxation_rate;
    return run_steps(p, mcn::plan_env_step(p, tu), actions, 1, (hipStream_t)stream);
}

int mcn_env_rollout_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                       const mcn_env_state *st, const double *actions, int32_t T, const mcn_env_out *out,
                       const mcn_rollout *roll, int32_t E, int32_t N, void *stream)
{
    if (T <= 0 || !sf_params_ok(strength, range, relaxation_rate)) return MCN_EINVAL;
    const mcn_tuning tu = tuning();
    mcn::StepParams p;
    const int rc = fill_step_params(p, tu, cfg, st, actions, nullptr, out, roll, E, N, 1, true);
    if (rc != MCN_OK) return rc;
    p.sf_strength = strength; p.sf_range = range; p.sf_relaxation_rate = relaxation_rate;
    return run_rollout(p, mcn::plan_env_rollout(p, T, tu), actions, T, (hipStream_t)stream);
}

int mcn_scenario_pool(const mcn_scenario_cfg *cfg, uint64_t seed, int64_t first_case, int32_t P, int32_t N,
                      double *hpos, double *hgoal, double *hrad, double *hvpref, void *stream)
{
    if (!cfg || !hpos || !hgoal || !hrad || !hvpref) return MCN_EINVAL;
    if (P <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (cfg->rule != MCN_RULE_CIRCLE && cfg->rule != MCN_RULE_SQUARE) return MCN_EINVAL;
    if (!(cfg->circle_radius > 0) || !(cfg->square_width > 0) || !(cfg->human_radius > 0)) return MCN_EINVAL;
    return mcn::launch_scenario_pool(*cfg, seed, first_case, P, N, hpos, hgoal, hrad, hvpref, (hipStream_t)stream);
}

int mcn_orca_batch(const float *self, const float *others, const int32_t *n_other, float *out,
                   int32_t B, int32_t M, float neighbor_dist, int32_t max_neighbors,
                   float time_horizon, float time_step, void *stream)
{
    if (!self || !n_other || !out || B <= 0 || M < 0 || M > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (M > 0 && !others) return MCN_EINVAL;
    if (max_neighbors < 0 || max_neighbors > MCN_MAX_LINES) return MCN_EINVAL;
    if (!(time_horizon > 0) || !(time_step > 0)) return MCN_EINVAL;
    return mcn::launch_orca_batch(self, others, n_other, out, B, M, neighbor_dist, max_neighbors,
                                  time_horizon, time_step, (hipStream_t)stream);
}

int mcn_orca_finish(const mcn_env_state *st, float *sim_vel, const uint8_t *select, int32_t max_steps, int32_t *steps,
                    float *traj, double time_step, float neighbor_dist, int32_t max_neighbors, float time_horizon,
                    int32_t E, int32_t N, void *stream)
{
    if (!st || !sim_vel || !steps || max_steps < 1 || E <= 0 || N < 1 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (!st->hpos || !st->hgoal || !st->hrad || !st->hvpref || !st->rpos || !st->rgoal || !st->rrad || !st->rvpref ||
        !st->gtime || !st->human_times) return MCN_EINVAL;
    if (max_neighbors < 0 || max_neighbors > MCN_MAX_LINES) return MCN_EINVAL;
    if (!(time_horizon > 0) || !(time_step > 0) || !((float)time_step > 0)) return MCN_EINVAL;
    return mcn::launch_orca_finish(*st, sim_vel, select, max_steps, steps, traj, time_step, neighbor_dist, max_neighbors,
                                   time_horizon, E, N, (hipStream_t)stream);
}

int mcn_pack_linear(const float *weight, const float *bias, int32_t nout, int32_t kin,
                    const int32_t *kmap, int32_t KT, const int32_t *omap, int32_t NT,
                    float *wfrag_out, float *bfrag_out)
{
    if (!weight || !kmap || !wfrag_out || nout <= 0 || kin <= 0 || KT <= 0 || NT <= 0) return MCN_EINVAL;
    if (!omap && NT != (nout + 15) / 16) return MCN_EINVAL;
    auto orow = [&](int n, int slot) { return omap ? omap[n * 16 + slot] : 16 * n + slot; };
    for (int n = 0; n < NT; ++n)
        for (int slot = 0; slot < 16; ++slot)
            if (orow(n, slot) >= nout) { if (omap) return MCN_EINVAL; }
    for (int n = 0; n < NT; ++n)
        for (int t = 0; t < KT; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int row = orow(n, lane & 15);
                    const int col = kmap[t * 16 + 4 * (lane >> 4) + r];
                    float v = 0.0f;
                    if (row >= 0 && row < nout && col >= 0) {
                        if (col >= kin) return MCN_EINVAL;
                        v = weight[(size_t)row * kin + col];
                    }
                    wfrag_out[(((size_t)n * KT + t) * 64 + lane) * 4 + r] = v;
                }
    if (bfrag_out)
        for (int n = 0; n < NT; ++n)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int row = orow(n, 4 * (lane >> 4) + r);
                    bfrag_out[((size_t)n * 64 + lane) * 4 + r] = (bias && row >= 0 && row < nout) ? bias[row] : 0.0f;
                }
    return MCN_OK;
}

int64_t mcn_sarl_workspace_bytes(int32_t E, int32_t N, int32_t A)
{
    if (E <= 0 || N <= 0 || A <= 0) return 0;
    return (int64_t)mcn::sarl_workspace_float4s(E, N, A) * 16;
}

// What every look-ahead entry point checks alike (SARL, LSTM-RL, CADRL); each adds its own on top: which outputs may
// be NULL, whether `kinematics` is range-checked, how `rewards` pairs with the next states.
static bool lookahead_common_ok(const void *net, size_t net_bytes, const mcn_env_state *st, const double *actions,
                                int32_t A, double time_step, int32_t kinematics, const double *values,
                                const double *next_hpos, const double *next_hvel, double epsilon, int32_t E, int32_t N)
{
    if (!net || !st || !actions || !values) return false;
    if (!(epsilon >= 0.0 && epsilon <= 1.0)) return false;
    if (E <= 0 || N <= 0 || N > MCN_MAX_HUMANS || A <= 0) return false;
    if (!st->hpos || !st->hvel || !st->hrad || !st->rpos || !st->rgoal || !st->rrad || !st->rvpref) return false;
    if (kinematics == MCN_KIN_UNICYCLE && !st->rtheta) return false;
    if ((next_hpos == nullptr) != (next_hvel == nullptr)) return false;
    const float *const *fp = reinterpret_cast<const float *const *>(net);
    for (size_t k = 0; k < net_bytes / sizeof(float *); ++k)
        if (!fp[k]) return false;
    return time_step > 0;
}

static int sarl_lookahead_impl(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                               double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                               double *values, int32_t *best, double *best_val, float *attention,
                               const double *next_hpos, const double *next_hvel, const double *rewards,
                               double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N,
                               const float *om_init, void *stream)
{
    if (!lookahead_common_ok(net, sizeof(*net), st, actions, A, time_step, kinematics, values, next_hpos, next_hvel,
                             epsilon, E, N))
        return MCN_EINVAL;
    if (!workspace) return MCN_EINVAL;
    if (action_out && !best) return MCN_EINVAL;         // best may be NULL (values only) ...
    if (best && !best_val) return MCN_EINVAL;           // ... but not without best_val
    return mcn::launch_sarl_c(net, st, actions, A, time_step, gamma_pow, kinematics, workspace, values, best,
                              best_val, attention, next_hpos, next_hvel, rewards, action_out, epsilon,
                              (unsigned long long)seed, E, N, om_init, (hipStream_t)stream);
}

int mcn_sarl_lookahead(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                       double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                       double *values, int32_t *best, double *best_val, float *attention,
                       int32_t E, int32_t N, void *stream)
{
    return sarl_lookahead_impl(net, st, actions, A, time_step, gamma_pow, kinematics, workspace, values, best, best_val,
                               attention, nullptr, nullptr, nullptr, nullptr, 0.0, 0, E, N, nullptr, stream);
}

int mcn_sarl_lookahead_env(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                           double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                           double *values, int32_t *best, double *best_val, float *attention,
                           const double *next_hpos, const double *next_hvel, const double *rewards,
                           int32_t E, int32_t N, void *stream)
{
    if (!next_hpos || !next_hvel || !rewards) return MCN_EINVAL;
    return sarl_lookahead_impl(net, st, actions, A, time_step, gamma_pow, kinematics, workspace, values, best, best_val,
                               attention, next_hpos, next_hvel, rewards, nullptr, 0.0, 0, E, N, nullptr, stream);
}

int mcn_sarl_predict(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                     double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                     double *values, int32_t *best, double *best_val, float *attention,
                     const double *next_hpos, const double *next_hvel, const double *rewards,
                     double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream)
{
    if (!best || !action_out) return MCN_EINVAL;
    if ((next_hpos == nullptr) != (rewards == nullptr)) return MCN_EINVAL;
    return sarl_lookahead_impl(net, st, actions, A, time_step, gamma_pow, kinematics, workspace, values, best, best_val,
                               attention, next_hpos, next_hvel, rewards, action_out, epsilon, seed, E, N, nullptr, stream);
}

int mcn_sarl_om_prepare(const mcn_env_state *st, double time_step, const double *next_hpos, const double *next_hvel,
                        double cell_size, const float *w_om, const float *b_om, float *om, float *init,
                        int32_t E, int32_t N, void *stream)
{
    if (!st || !om) return MCN_EINVAL;
    if (E <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (!st->hpos || !st->hvel) return MCN_EINVAL;
    if ((next_hpos == nullptr) != (next_hvel == nullptr)) return MCN_EINVAL;
    if (!(time_step >= 0.0) || !(cell_size > 0.0)) return MCN_EINVAL;
    // the layer's operands and its output go together: all three, or none (maps only)
    if ((w_om == nullptr) != (init == nullptr) || (b_om == nullptr) != (init == nullptr)) return MCN_EINVAL;
    return mcn::launch_sarl_om(st, time_step, next_hpos, next_hvel, cell_size, w_om, b_om, om, init, E, N,
                               (hipStream_t)stream);
}

int mcn_sarl_predict_om(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                        double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                        double *values, int32_t *best, double *best_val, float *attention,
                        const double *next_hpos, const double *next_hvel, const double *rewards,
                        double *action_out, double epsilon, uint64_t seed, const float *om_init,
                        int32_t E, int32_t N, void *stream)
{
    if (!best || !action_out || !om_init) return MCN_EINVAL;
    if ((next_hpos == nullptr) != (rewards == nullptr)) return MCN_EINVAL;
    return sarl_lookahead_impl(net, st, actions, A, time_step, gamma_pow, kinematics, workspace, values, best, best_val,
                               attention, next_hpos, next_hvel, rewards, action_out, epsilon, seed, E, N, om_init, stream);
}

// validation of mcn_lstm_rl_predict / mcn_cadrl_predict: the common part, and every output required
static int lookahead_args_ok(const void *net, size_t net_bytes, const mcn_env_state *st, const double *actions, int32_t A,
                             double time_step, int32_t kinematics, const double *values, const int32_t *best,
                             const double *best_val, const double *next_hpos, const double *next_hvel,
                             const double *rewards, const double *action_out, double epsilon, int32_t E, int32_t N)
{
    if (!lookahead_common_ok(net, net_bytes, st, actions, A, time_step, kinematics, values, next_hpos, next_hvel, epsilon, E, N))
        return 0;
    if (!best || !best_val || !action_out) return 0;
    if (kinematics != MCN_KIN_HOLONOMIC && kinematics != MCN_KIN_UNICYCLE) return 0;
    return (next_hpos == nullptr) == (rewards == nullptr);
}

int mcn_lstm_rl_predict(const mcn_lstm_rl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                        double time_step, double gamma_pow, int32_t kinematics,
                        double *values, int32_t *best, double *best_val, int32_t *order,
                        const double *next_hpos, const double *next_hvel, const double *rewards,
                        double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream)
{
    if (!lookahead_args_ok(net, sizeof(*net), st, actions, A, time_step, kinematics, values, best, best_val, next_hpos,
                           next_hvel, rewards, action_out, epsilon, E, N))
        return MCN_EINVAL;
    return mcn::launch_lstm_rl(net, st, actions, A, time_step, gamma_pow, kinematics, values, best, best_val, order,
                               next_hpos, next_hvel, rewards, action_out, epsilon, (unsigned long long)seed, E, N,
                               (hipStream_t)stream);
}

int mcn_lstm_rl_order(const mcn_env_state *st, int32_t *order, int32_t E, int32_t N, void *stream)
{
    if (!st || !order || !st->hpos || !st->rpos || E <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    return mcn::launch_lstm_rl_order(st->hpos, st->rpos, st->hcount, order, E, N, (hipStream_t)stream);
}

int mcn_cadrl_predict(const mcn_cadrl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                      double time_step, double gamma_pow, int32_t kinematics,
                      double *values, int32_t *best, double *best_val,
                      const double *next_hpos, const double *next_hvel, const double *rewards,
                      double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream)
{
    if (!lookahead_args_ok(net, sizeof(*net), st, actions, A, time_step, kinematics, values, best, best_val, next_hpos,
                           next_hvel, rewards, action_out, epsilon, E, N))
        return MCN_EINVAL;
    return mcn::launch_cadrl(net, st, actions, A, time_step, gamma_pow, kinematics, values, best, best_val, next_hpos,
                             next_hvel, rewards, action_out, epsilon, (unsigned long long)seed, E, N, (hipStream_t)stream);
}

int64_t mcn_sarl_train_param_count(int32_t input_dim) { return (int64_t)mcn::sarl_train_param_count(input_dim); }

int64_t mcn_sarl_train_workspace_bytes(int32_t B, int32_t N, int32_t input_dim)
{
    if (B <= 0 || N <= 0 || N > MCN_MAX_HUMANS || mcn::sarl_train_param_count(input_dim) < 0) return 0;
    return (int64_t)mcn::sarl_train_workspace_floats(B, N, input_dim) * 4;
}

int mcn_sarl_loss_grad(const float *params, int32_t input_dim, const float *states, const float *values,
                       const int64_t *rows, int32_t B, int32_t N, void *workspace, float *grad, float *loss, void *stream)
{
    if (!params || !states || !values || !workspace || !grad || !loss) return MCN_EINVAL;
    if (B < 1 || N < 1 || N > MCN_MAX_HUMANS || (input_dim != 13 && input_dim != 61)) return MCN_EINVAL;
    return mcn::launch_sarl_loss_grad(params, input_dim, states, values, rows, B, N, workspace, grad, loss,
                                      (hipStream_t)stream);
}

int mcn_sgd_momentum_step(float *params, float *momentum_buf, const float *grad, int64_t count, float lr, float momentum,
                          void *stream)
{
    if (!params || !momentum_buf || !grad || count < 1 || !isfinite(lr) || !isfinite(momentum)) return MCN_EINVAL;
    return mcn::launch_sgd_momentum(params, momentum_buf, grad, count, lr, momentum, (hipStream_t)stream);
}

int64_t mcn_cadrl_train_param_count(void) { return (int64_t)mcn::cadrl_train_param_count(); }

int64_t mcn_cadrl_train_workspace_bytes(int32_t B)
{
    if (B <= 0) return 0;
    return (int64_t)mcn::cadrl_train_workspace_floats(B) * 4;
}

int mcn_cadrl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int32_t B,
                        void *workspace, float *grad, float *loss, void *stream)
{
    if (!params || !states || !values || !workspace || !grad || !loss || B < 1) return MCN_EINVAL;
    return mcn::launch_cadrl_loss_grad(params, states, values, rows, B, workspace, grad, loss, (hipStream_t)stream);
}

int64_t mcn_lstm_rl_train_param_count(void) { return (int64_t)mcn::lstm_rl_train_param_count(); }

int64_t mcn_lstm_rl_train_workspace_bytes(int32_t B, int32_t N)
{
    if (B <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return 0;
    return (int64_t)mcn::lstm_rl_train_workspace_floats(B, N) * 4;
}

int mcn_lstm_rl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int32_t B,
                          int32_t N, void *workspace, float *grad, float *loss, void *stream)
{
    if (!params || !states || !values || !workspace || !grad || !loss) return MCN_EINVAL;
    if (B < 1 || N < 1 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    return mcn::launch_lstm_rl_loss_grad(params, states, values, rows, B, N, workspace, grad, loss, (hipStream_t)stream);
}

int64_t mcn_attn_world_train_param_count(void) { return (int64_t)mcn::attn_world_train_param_count(); }

int64_t mcn_attn_world_train_workspace_bytes(int32_t B, int32_t N)
{
    if (B <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return 0;
    return (int64_t)mcn::attn_world_train_workspace_floats(B, N) * 4;
}

int mcn_attn_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int32_t B,
                             int32_t N, void *workspace, float *grad, float *loss, void *stream)
{
    if (!params || !cur || !nxt || !workspace || !loss) return MCN_EINVAL;
    if (B < 1 || N < 1 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    return mcn::launch_attn_world_loss_grad(params, cur, nxt, rows, B, N, workspace, grad, loss, (hipStream_t)stream);
}

int mcn_adam_step(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t count, float lr,
                  float beta1, float beta2, float eps, int32_t step, void *stream)
{
    if (!params || !exp_avg || !exp_avg_sq || !grad || count < 1 || step < 1) return MCN_EINVAL;
    if (!isfinite(lr) || !isfinite(eps) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return MCN_EINVAL;                              // (a NaN or infinite beta fails the range test)
    return mcn::launch_adam(params, exp_avg, exp_avg_sq, grad, count, lr, beta1, beta2, eps, step, (hipStream_t)stream);
}

int64_t mcn_mlp_world_train_param_count(int32_t N)
{
    if (N <= 0 || N > MCN_MAX_HUMANS) return 0;
    return (int64_t)mcn::mlp_world_train_param_count(N);
}

int64_t mcn_mlp_world_train_workspace_bytes(int32_t B, int32_t N)
{
    if (B <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return 0;
    return (int64_t)mcn::mlp_world_train_workspace_floats(B, N) * 4;
}

int mcn_mlp_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int32_t B,
                            int32_t N, float drop_p, uint64_t seed, uint64_t step, void *workspace, float *grad,
                            float *loss, void *stream)
{
    if (!params || !cur || !nxt || !workspace || !loss) return MCN_EINVAL;
    if (B < 1 || N < 1 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (!(drop_p >= 0.f && drop_p < 1.f)) return MCN_EINVAL;          // (a NaN or infinite drop_p fails the range test)
    return mcn::launch_mlp_world_loss_grad(params, cur, nxt, rows, B, N, drop_p, seed, step, workspace, grad, loss,
                                           (hipStream_t)stream);
}

int mcn_dropout_mask(uint64_t seed, uint64_t step, int32_t layer, int32_t B, int32_t width, float p, uint8_t *keep)
{
    if (!keep || B < 1 || width < 1 || width > 256 || layer < 0 || layer > 1 || !(p >= 0.f && p < 1.f)) return MCN_EINVAL;
    return mcn::dropout_mask_host(seed, step, layer, B, width, p, keep);
}

int mcn_mlp_world_step(const mcn_mlp_world_net *net, const double *hpos, const double *hvel, double *out_vel,
                       int32_t E, int32_t N, void *stream)
{
    if (!net || !hpos || !hvel || !out_vel || E <= 0 || N <= 0 || N > 10) return MCN_EINVAL;
    const float *const *fp = reinterpret_cast<const float *const *>(net);
    for (int k = 0; k < 8; ++k)
        if (!fp[k]) return MCN_EINVAL;
    return mcn::launch_mlp_world(net, hpos, hvel, out_vel, E, N, (hipStream_t)stream);
}

int64_t mcn_attn_world_workspace_bytes(int32_t E, int32_t N)
{
    if (E <= 0 || N <= 0) return 0;
    return (int64_t)mcn::attn_world_workspace_float4s(E, N) * 16;
}

int mcn_attn_world_step(const mcn_attn_world_net *net, const double *hpos, const double *hvel, const int32_t *hcount,
                        void *workspace, double *out_vel, int32_t E, int32_t N, void *stream)
{
    if (!net || !hpos || !hvel || !workspace || !out_vel || E <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    const float *const *fp = reinterpret_cast<const float *const *>(net);
    for (size_t k = 0; k < sizeof(mcn_attn_world_net) / sizeof(float *); ++k)
        if (!fp[k]) return MCN_EINVAL;
    return mcn::launch_attn_world(net, hpos, hvel, hcount, workspace, out_vel, E, N, (hipStream_t)stream);
}

int64_t mcn_sgan_workspace_bytes(int32_t E, int32_t N)
{
    if (E <= 0 || N <= 0) return 0;
    return (int64_t)E * N * (32 + 4 + 8) * 4;     // encoder state, last position / displacement, pooled features
}

int mcn_sgan_step(const mcn_sgan_net *net, double *hist, int32_t push_slot, int32_t oldest, const double *cur_pos,
                  const float *noise, const int32_t *hcount, void *workspace, double *out_vel, float *out_rel,
                  double time_step, int32_t E, int32_t N, void *stream)
{
    if (!net || !hist || !noise || !workspace || !out_vel) return MCN_EINVAL;
    if (E <= 0 || N <= 0 || N > MCN_MAX_HUMANS) return MCN_EINVAL;
    if (push_slot < 0 || push_slot > 7 || oldest < 0 || oldest > 7 || !(time_step > 0)) return MCN_EINVAL;
    const float *const *fp = reinterpret_cast<const float *const *>(net);
    for (int k = 0; k < 14; ++k) {
        const bool pool_only = (k >= 2 && k < 6);
        if (!fp[k] && !(pool_only && !net->pooling)) return MCN_EINVAL;
    }
    return mcn::launch_sgan(net, hist, push_slot, oldest, cur_pos, noise, hcount, workspace, out_vel, out_rel,
                            time_step, E, N, (hipStream_t)stream);
}

int mcn_sgan_predict(const mcn_sgan_net *net, const double *hist, int32_t oldest, const float *noise, int32_t K, int32_t T,
                     const int32_t *hcount, void *workspace, float *out_rel, double *out_pos, int32_t E, int32_t N,
                     void *stream)
{
    if (!net || !hist || !noise || !workspace || !out_rel) return MCN_EINVAL;
    if (K < 1 || K > 65535 || T < 1) return MCN_EINVAL;          // (K is a grid dimension)
    if (E <= 0 || N <= 0 || N > MCN_MAX_HUMANS || oldest < 0 || oldest > 7) return MCN_EINVAL;
    const float *const *fp = reinterpret_cast<const float *const *>(net);
    for (int k = 0; k < 14; ++k) {
        const bool pool_only = (k >= 2 && k < 6);
        if (!fp[k] && !(pool_only && !net->pooling)) return MCN_EINVAL;
    }
    return mcn::launch_sgan_predict(net, hist, oldest, noise, K, T, hcount, workspace, out_rel, out_pos, E, N,
                                    (hipStream_t)stream);
}

#ifdef MCN_DIAG
// diagnostic build only: [workgroup][4] = s_memtime, s_memrealtime before / after the SGAN pool kernel's unit loop
int mcn_debug_pool_clock(void *dst_host, int64_t bytes) { return mcn::read_pool_clock(dst_host, (size_t)bytes); }
// diagnostic build only: [resident wavefront][16] shader cycles per phase of sarl_value_kernel (tools/sarl_phases.py)
int mcn_debug_sarl_phases(void *dst_host, int64_t bytes, int32_t reset) { return mcn::read_sarl_phases(dst_host, (size_t)bytes, reset); }
// diagnostic build only: copies the rollout kernel's time stamps to host memory, returns the number of 8-byte words
int mcn_debug_stamps(void *dst_host, int64_t bytes) { return mcn::read_stamps(dst_host, (size_t)bytes, g_last_rollout_form); }
// per-wavefront counts of the data-dependent paths taken: [wave][4] = 3-D LP, restarts, overlap sqrt, goal sqrt
int mcn_debug_counts(void *dst_host, int64_t bytes, int reset) { return mcn::read_counts(dst_host, (size_t)bytes, reset, g_last_rollout_form); }
#endif

}  // extern "C"
