// launch.hpp -- the host functions one translation unit of libmcn_hip.so offers to another, each declared once.
// Included where a function is defined and where it is called.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/mcn.h"
#include "env_step_params.hpp"
#include "env_dispatch.hpp"

namespace mcn {

// mcn_api.hip
bool tuning_sarl_x3();              // mcn_tuning.sarl_x3 (-1 / 1: use the x3 fragments when given, 0: never)
double written_as(float x);         // a float32 hyper-parameter as the decimal that was written: 0.001f -> 0.001

// Env kernels.  mcn_api.hip plans (env_dispatch.hpp); each launcher gets its part of the plan, picks the instantiation,
// sizes the grid and launches.  None reports errors: the caller reads hipGetLastError() after each launch group.
// env_step.hip
void launch_env_step(const StepParams &p, const StepPlan &plan, hipStream_t stream);
void launch_env_step_loop(const StepParams &p, int T, hipStream_t stream);
void launch_env_step_loop_sf(const StepParams &p, int T, hipStream_t stream);
void launch_env_step_loop_orca(const StepParams &p, const ClosedLoop &cl, int T, hipStream_t stream);
void launch_env_step_loop_orca_sf(const StepParams &p, const ClosedLoop &cl, int T, hipStream_t stream);
// env_step_quad.hip, env_pair.hip
void launch_env_step_quad(const StepParams &p, bool split, hipStream_t stream);
void launch_env_pair(const StepParams &p, bool nontemporal, hipStream_t stream);
// env_rollout_quad.hip (forms 0 / 1, and the hand-over of form 2), env_rollout_wg4.hip (the four-wavefront form: 5 humans,
// invisible robot, one workgroup per 8 envs)
void launch_env_rollout_quad(const StepParams &p, int form, int T, hipStream_t stream);
void launch_env_rollout_wg4(const StepParams &p, int T, hipStream_t stream);

// scenario_gen.hip, orca_batch.hip, orca_finish.hip
int launch_scenario_pool(const mcn_scenario_cfg &c, uint64_t seed, int64_t first_case, int P, int N, double *hpos,
                         double *hgoal, double *hrad, double *hvpref, hipStream_t stream);
int launch_orca_batch(const float *self, const float *others, const int32_t *n_other, float *out,
                      int B, int M, float neighbor_dist, int max_neighbors, float time_horizon, float time_step,
                      hipStream_t stream);
int launch_orca_finish(const mcn_env_state &st, float *sim_vel, const uint8_t *select, int max_steps, int32_t *steps,
                       float *traj, double time_step, float neighbor_dist, int max_neighbors, float time_horizon,
                       int E, int N, hipStream_t stream);

// world_mlp.hip, world_attn.hip
int launch_mlp_world(const mcn_mlp_world_net *net, const double *hpos, const double *hvel, double *out_vel, int E, int N,
                     hipStream_t stream);
int launch_attn_world(const mcn_attn_world_net *net, const double *hpos, const double *hvel, const int32_t *hcount,
                      void *workspace, double *out_vel, int E, int N, hipStream_t stream);
long attn_world_workspace_float4s(int E, int N);

// sarl_value.hip, sarl_om.hip
long sarl_workspace_float4s(int E, int N, int A);
int launch_sarl_c(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                  double gamma_pow, int kinematics, void *workspace, double *values, int32_t *best, double *best_val,
                  float *attention, const double *next_hpos, const double *next_hvel, const double *reward_in,
                  double *action_out, double epsilon, unsigned long long seed, int E, int N, const float *om_init,
                  hipStream_t stream);
// the SARL look-ahead's argmax / epsilon-greedy kernel, for the other look-ahead kernels too (lstm_rl_value.hip)
int launch_sarl_argmax(const double *values, const double *rpos, const double *rgoal, const double *rrad, int E, int A,
                       int32_t *best, double *best_val, const double *actions, double *action_out, double epsilon,
                       unsigned long long seed, hipStream_t stream);
int launch_sarl_om(const mcn_env_state *st, double dt, const double *next_hpos, const double *next_hvel,
                   double cell_size, const float *w_om, const float *b_om, float *om, float *init, int E, int N,
                   hipStream_t stream);

// sarl_train.hip
long sarl_train_param_count(int input_dim);                          // -1 unless input_dim is 13 or 61
long sarl_train_workspace_floats(int B, int N, int input_dim);
int launch_sarl_loss_grad(const float *params, int input_dim, const float *states, const float *values,
                          const int64_t *rows, int B, int N, void *workspace, float *grad, float *loss,
                          hipStream_t stream);
int launch_sgd_momentum(float *params, float *momentum_buf, const float *grad, int64_t count, float lr, float momentum,
                        hipStream_t stream);

// world_train.hip
long attn_world_train_param_count();
long attn_world_train_workspace_floats(int B, int N);
int launch_attn_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int B,
                                int N, void *workspace, float *grad /* or NULL: the loss only */, float *loss,
                                hipStream_t stream);
int launch_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t count, float lr, float beta1,
                float beta2, float eps, int step, hipStream_t stream);

// world_mlp_train.hip (the masks: dropout_hash.hpp)
long mlp_world_train_param_count(int N);
long mlp_world_train_workspace_floats(int B, int N);
int launch_mlp_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int B, int N,
                               float drop_p, uint64_t seed, uint64_t step, void *workspace,
                               float *grad /* or NULL: the eval-mode loss only */, float *loss, hipStream_t stream);
int dropout_mask_host(uint64_t seed, uint64_t step, int layer, int B, int width, float p, uint8_t *keep);

// value_train.hip
long cadrl_train_param_count();
long cadrl_train_workspace_floats(int B);
int launch_cadrl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int B,
                           void *workspace, float *grad, float *loss, hipStream_t stream);
long lstm_rl_train_param_count();
long lstm_rl_train_workspace_floats(int B, int N);
int launch_lstm_rl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int B,
                             int N, void *workspace, float *grad, float *loss, hipStream_t stream);

// lstm_rl_value.hip
int launch_lstm_rl(const mcn_lstm_rl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                   double gamma_pow, int kinematics, double *values, int32_t *best, double *best_val, int32_t *order,
                   const double *next_hpos, const double *next_hvel, const double *reward_in, double *action_out,
                   double epsilon, unsigned long long seed, int E, int N, hipStream_t stream);
int launch_cadrl(const mcn_cadrl_net *net, const mcn_env_state *st, const double *actions, int A, double dt,
                 double gamma_pow, int kinematics, double *values, int32_t *best, double *best_val,
                 const double *next_hpos, const double *next_hvel, const double *reward_in, double *action_out,
                 double epsilon, unsigned long long seed, int E, int N, hipStream_t stream);
int launch_lstm_rl_order(const double *hpos, const double *rpos, const int32_t *hcount, int32_t *order, int E, int N,
                         hipStream_t stream);

// sgan_step.hip
int launch_sgan(const mcn_sgan_net *net, double *hist, int push_slot, int oldest, const double *cur_pos,
                const float *noise, const int32_t *hcount, void *workspace, double *out_vel, float *out_rel,
                double time_step, int E, int N, hipStream_t stream);
int launch_sgan_predict(const mcn_sgan_net *net, const double *hist, int oldest, const float *noise, int K, int T,
                        const int32_t *hcount, void *workspace, float *out_rel, double *out_pos, int E, int N,
                        hipStream_t stream);

#ifdef MCN_DIAG
// diagnostic build only
int read_pool_clock(void *dst, size_t bytes);                       // sgan_step.hip
int read_sarl_phases(void *dst, size_t bytes, int reset);           // sarl_value.hip
int read_stamps(void *dst, size_t bytes, int form);                 // env_rollout_quad.hip: those of the form that went out last
int read_counts(void *dst, size_t bytes, int reset, int form);
int read_stamps_wg4(void *dst, size_t bytes);                       // env_rollout_wg4.hip
int read_counts_wg4(void *dst, size_t bytes, int reset);
#endif

}  // namespace mcn
