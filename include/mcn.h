/*
 * mcn.h -- C ABI of libmcn_hip.so, the MI355X (gfx950) implementation of the
 * ModelCrowdNav data-parallel rollout hot path.
 *
 * The reference has no FFI of its own for this path: its boundary is three duck-typed
 * Python protocols (gym.Env, Policy, world-model callable) plus one native module, rvo2
 * (SURVEY.md section 8b).  Each entry point below names the reference interface it
 * replaces.  All pointers are DEVICE pointers into caller-owned HBM buffers unless
 * marked host; every call is stream-ordered on `stream` (a hipStream_t passed as
 * void*), performs no allocation and no synchronisation, and returns 0 on success or a
 * negative MCN_E* code.  No torch types appear in any signature.
 *
 * Buffer conventions (E environments, N humans, row-major, env-major):
 *   double2-packed arrays are [E*N][2] or [E][2] doubles, 16-byte aligned.
 *   hpos  (px,py)   hvel (vx,vy)   hgoal (gx,gy)                              [E*N][2]
 *   hrad, hvpref (radius, v_pref: separate so kernels that need only the radius stream only it)  [E*N]
 *   rpos  (px,py)   rvel (vx,vy)   rgoal (gx,gy)                              [E][2]
 *   rrad, rvpref                                                              [E]
 *   rtheta, gtime                                                             [E]
 * The observation the reference returns from step()/reset() -- a list of
 * ObservableState(px,py,vx,vy,radius), crowd_sim/envs/utils/state.py:27-43 -- is
 * (hpos, hvel, hrad) and is therefore never copied.
 */
#ifndef MCN_H_
#define MCN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCN_OK            0
#define MCN_EINVAL      (-1)   /* bad shape / null pointer / unsupported N */
#define MCN_ELAUNCH     (-2)   /* hipLaunchKernel reported an error        */

#define MCN_MAX_HUMANS   32    /* humans per environment (one wavefront holds >= 2 envs) */
#define MCN_MAX_LINES    10    /* ORCA maxNeighbors ceiling handled on device            */

/* info codes: crowd_sim/envs/utils/info.py:1-38 */
enum { MCN_INFO_NOTHING = 0, MCN_INFO_DANGER = 1, MCN_INFO_REACHGOAL = 2, MCN_INFO_COLLISION = 3, MCN_INFO_TIMEOUT = 4 };
/* how humans choose their velocity */
enum { MCN_HUMANS_ORCA = 0,     /* crowd_sim/envs/policy/orca.py:82-132            */
       MCN_HUMANS_LINEAR = 1,   /* crowd_sim/envs/policy/linear.py:15-22           */
       MCN_HUMANS_GIVEN = 2,    /* model_crowd_sim.py:347 step(new_v=...) / world model output */
       MCN_HUMANS_SOCIALFORCE = 3 };  /* social-force pedestrians: mcn_env_step_sf / mcn_env_rollout_sf only (they carry
                                       * the model's three parameters; mcn_env_step / mcn_env_rollout reject this value) */
enum { MCN_KIN_HOLONOMIC = 0, MCN_KIN_UNICYCLE = 1 };

/* Scalar configuration: env.config [env]/[reward] + orca.py:60-66 + robot flags.  The orca_* fields belong to
 * MCN_HUMANS_ORCA: with any other human_policy no kernel reads them (orca_max_neighbors is still range-checked), so
 * they may hold anything, NaN included, and change no output. */
typedef struct mcn_env_cfg {
    double time_step;                  /* env.config:3   */
    double time_limit;                 /* env.config:2   */
    double success_reward;             /* env.config:10  */
    double collision_penalty;          /* env.config:11  */
    double discomfort_dist;            /* env.config:12  */
    double discomfort_penalty_factor;  /* env.config:13  */
    double orca_safety_space;          /* orca.py:59     */
    float  orca_neighbor_dist;         /* orca.py:60     */
    float  orca_time_horizon;          /* orca.py:62     */
    int32_t orca_max_neighbors;        /* orca.py:61 (<= MCN_MAX_LINES) */
    int32_t robot_visible;             /* humans see the robot, crowd_sim.py:340 */
    int32_t human_policy;              /* MCN_HUMANS_*   */
    int32_t robot_kinematics;          /* MCN_KIN_*      */
    int32_t count_hh;                  /* crowd_sim.py:368-376 (CrowdSim yes, ModelCrowdSim no) */
    int32_t track_human_times;         /* crowd_sim.py:418-421 */
} mcn_env_cfg;

/* Device state of E environments (all device pointers, caller-owned). */
typedef struct mcn_env_state {
    double *hpos, *hvel, *hgoal;               /* [E*N][2] */
    double *hrad, *hvpref;                     /* [E*N]    */
    double *rpos, *rvel, *rgoal;               /* [E][2]   */
    double *rrad, *rvpref;                     /* [E]      */
    double *rtheta;                            /* [E]      */
    double *gtime;                             /* [E]  CrowdSim.global_time */
    double *human_times;                       /* [E*N] or NULL */
    const int32_t *hcount;                     /* [E] or NULL: pedestrians the ROBOT'S POLICY sees, 1 <= hcount[e] <= N.
                                                * mcn_sarl_lookahead ignores slots i >= hcount[e] (attention sum, mean,
                                                * distance test); the env kernels step all N slots regardless */
} mcn_env_state;

/* What one env reports per step, as ONE 24-byte record: the kernel issues one store per env instead of five
 * scattered 1..8-byte ones (at a million envs the narrow per-env streams, not the bytes, limit the kernel). */
/* Alignment: 8 bytes (24-byte stride); the first 16 bytes are written with one 16-byte store, which gfx950 global
 * memory accepts at 8-byte alignment. */
typedef struct mcn_step_rec {
    double  reward;
    double  dmin;         /* min boundary distance robot-human over the step */
    uint8_t done;
    uint8_t info;         /* MCN_INFO_* */
    uint16_t reserved;
    int32_t hh_count;     /* human-human overlaps (the reference only logs them) */
} mcn_step_rec;

/* Per-step outputs (device pointers). */
typedef struct mcn_env_out {
    mcn_step_rec *rec;    /* [E] */
    double  *human_act;   /* [E*N][2] velocity each human chose, or NULL */
    double  *nobs_pos;    /* [E*N][2] next observable positions  (update == 0 only) */
    double  *nobs_vel;    /* [E*N][2] next observable velocities (update == 0 only) */
    void    *lp3_queue;   /* optional: mcn_env_lp3_queue_bytes(E, N) bytes of device memory, zero-filled ONCE by the caller
                           * and then owned by the env (the kernels keep its header consistent), or NULL.  With a queue,
                           * large ORCA batches of <= 10 humans solve RVO2's rare linearProgram3 in a second, dense launch
                           * (one parked problem per lane) instead of inside the step kernel, where one or two lanes of a
                           * wavefront would run it while the others wait.  Same results bit for bit.  The queue holds
                           * half of the worst case (0.9-3.7 % of the humans use it in a circle crossing, in bursts):
                           * humans beyond that are solved inside the step kernel as without a queue. */
} mcn_env_out;

/* Bytes of mcn_env_out.lp3_queue for E envs of N humans (0 when N is outside the deferred path's range):
 * 65 KiB of counters + 256 sub-queues x max(64, worst case / 2) entries x (28 + 16 N) bytes -- 264 MB for 2^18 x 10. */
int64_t mcn_env_lp3_queue_bytes(int32_t E, int32_t N);

/*
 * Optional fused bookkeeping of Explorer.run_k_episodes (crowd_nav/utils/explorer.py:54-125)
 * and vector-env style auto-reset.  Any pointer may be NULL to disable that part.
 */
/* Rollout state of one env, ONE 32-byte record (one load + one store per step). */
typedef struct mcn_roll_rec {
    double  ep_return;         /* running discounted sum */
    int32_t ep_steps;          /* steps taken in the running episode */
    int32_t fin_count;         /* episodes finished so far */
    int32_t next_case;         /* pool index used at the next reset, in [0, pool_size); advanced by case_stride mod pool_size */
    int32_t danger_count;      /* steps whose info was Danger ("too close", explorer.py:88-90) */
    double  danger_dist_sum;   /* sum of their min_dist */
} mcn_roll_rec;

typedef struct mcn_rollout {
    /* discounted return: sum_t disc_table[t] * r_t, disc_table[t] = pow(gamma, t*dt*v_pref) (explorer.py:124), added up
     * step by step as ret + disc_table[t] * r_t (two roundings, no fused multiply-add).  Steps of an episode from index
     * disc_len on take the LAST entry, disc_table[disc_len - 1]: nothing is read past the table.  disc_len >= 1; the
     * streaming given-velocity kernel (env_pair.hip) takes tables of at most 128 entries, longer ones go to the
     * lane-per-human kernel (same results) */
    const double *disc_table;  int32_t disc_len;
    /* the "too close" statistics (danger_count / danger_dist_sum, explorer.py:88-90,138-141) only count steps of an env's
     * first `danger_episodes` episodes; <= 0 = every step, and danger_short_from is not looked at (see below).  The
     * distances are added in step order */
    int32_t danger_episodes;
    mcn_roll_rec *state;       /* [E], or NULL: no return accounting */
    /* records of finished episodes: with fin_slots == 1 slot 0 holds the latest episode of env e; with
     * fin_slots > 1 episode number k < fin_slots of env e lands in slot k and later ones are not recorded */
    double  *fin_return;       /* [fin_slots][E] */
    double  *fin_time;         /* [fin_slots][E] env.global_time after the last step (explorer.py:95,99); cfg->time_limit for
                                * an episode that ended in MCN_INFO_TIMEOUT (explorer.py:106) */
    uint8_t *fin_info;         /* [fin_slots][E] */
    int32_t  fin_slots;        /* >= 1 */
    /* k episodes over E envs leave the last round partial: when danger_short_from > 0, envs with index >=
     * danger_short_from - 1 count one episode fewer than danger_episodes (with danger_episodes = 1: none at all);
     * 0 = all envs count danger_episodes */
    int32_t  danger_short_from;
    /* auto-reset from a pool of host-generated scenarios (bit-exact CrowdSim.reset output) */
    const double *pool_hpos, *pool_hgoal;                /* [P*N][2] */
    const double *pool_hrad, *pool_hvpref;               /* [P*N]    */
    const double *pool_hvel;                             /* [P*N][2] or NULL (zeros) */
    int32_t pool_size;
    int32_t case_stride;       /* in [0, pool_size); pool resets need `state` (its next_case field) */
    double  robot_start[2], robot_goal[2], robot_theta0;  /* crowd_sim.py:284 */
} mcn_rollout;

/*
 * mcn_env_step -- one batched CrowdSim.step / ModelCrowdSim.step.
 * Replaces: crowd_sim/envs/crowd_sim.py:331-434 (step, update=True/False),
 *           crowd_sim/envs/crowd_sim.py:325-329 (onestep_lookahead),
 *           crowd_sim/envs/model_crowd_sim.py:347-441,
 *           and the per-human rvo2 round trip of crowd_sim/envs/policy/orca.py:82-132.
 * actions: [E][2] (vx,vy) holonomic or (v,r) unicycle.  given_v: [E*N][2] or NULL.
 * update != 0 advances state in place; update == 0 leaves state untouched and fills nobs_*.
 * roll may be NULL.
 */
int mcn_env_step(const mcn_env_cfg *cfg, const mcn_env_state *st, const double *actions,
                 const double *given_v, const mcn_env_out *out, const mcn_rollout *roll,
                 int32_t E, int32_t N, int32_t update, void *stream);

/*
 * mcn_env_rollout -- T consecutive mcn_env_step(update = 1) calls with the action sequence actions[T][E][2],
 * same results bit for bit.  Replaces the step loop of Explorer.run_k_episodes (crowd_nav/utils/explorer.py:69-99)
 * for robots whose actions do not depend on the observation (random / scripted sequences).  Where the batch is
 * small enough to be latency-bound the T steps run in ONE launch: with <= 4 ORCA neighbours per human the env state
 * stays in registers (env_rollout_quad.hip), with 6-10 ORCA humans the one-wavefront step kernel runs T times and the
 * state goes through L2 (env_step.hip: env_step_loop_kernel); otherwise this is T launches.  On return `st` is the state after step T,
 * `out->rec` / `out->human_act` are those of step T, `roll` has accounted for all T steps (episodes that end
 * inside the sequence are recorded and, with a pool, restarted in-kernel).  Humans: ORCA or linear (no given_v).
 */
int mcn_env_rollout(const mcn_env_cfg *cfg, const mcn_env_state *st, const double *actions, int32_t T,
                    const mcn_env_out *out, const mcn_rollout *roll, int32_t E, int32_t N, void *stream);

/*
 * mcn_env_rollout_orca -- T consecutive closed-loop steps with an ORCA-driven holonomic robot (the reference's
 * imitation-learning demonstrator, crowd_nav/train.py:150-160, and `test.py --policy orca`) in ONE launch
 * (env_step.hip: env_step_loop_orca_kernel), for any batch and any 1 <= N <= MCN_MAX_HUMANS.  Each step equals, bit for
 * bit, this per-step sequence:
 *   1  the robot's action, as mcn_orca_batch returns it for the robot as agent 0 with all N humans of its env as
 *      candidates in index order (hcount is not consulted); every operand float64 -> float32: position, velocity,
 *      radius float32((rrad + 0.01) + robot_safety_space), max speed float32(rvpref), preferred velocity
 *      float32(rgoal - rpos), the humans' positions, velocities and radii float32((hrad + 0.01) + robot_safety_space) --
 *      two float64 additions in the reference's order (crowd_sim/envs/policy/orca.py:100,103); with the given
 *      neighbor_dist / max_neighbors / time_horizon and float32(cfg->time_step); the float32 result widened to float64;
 *   2  mcn_env_step(cfg, st, that action, NULL, out, roll, E, N, update = 1).
 * The robot's parameters are its policy's own: they may differ from the humans' cfg->orca_* (imitation learning gives the
 * robot a safety space, the humans none).  Optional traces, plain device pointers, each of which may be NULL:
 *   tr_robot     [T][E][5]     robot px, py, vx, vy, theta BEFORE step t (theta 0 without st->rtheta)
 *   tr_humans    [T][E][N][4]  px, py, vx, vy before step t
 *   tr_hrad      [T][E][N]     radii before step t (a pool restart changes them)
 *   tr_action    [T][E][2]     the robot's action of step t
 *   tr_rec       [T][E]        that step's record
 *   tr_human_act [T][E][N][2]  the velocities the humans chose in step t
 * On return `st`, `out->rec`, `out->human_act` and `roll` are as after the T-th per-step call.  MCN_EINVAL before any
 * launch: NULL cfg / st / out, a missing state array (st->rvpref included), T < 1, N outside 1 .. MCN_MAX_HUMANS,
 * max_neighbors outside 0 .. MCN_MAX_LINES, time_horizon or time_step (also as float32) not positive, a robot_safety_space
 * that is not finite, cfg->robot_kinematics other than MCN_KIN_HOLONOMIC, cfg->human_policy other than MCN_HUMANS_ORCA /
 * MCN_HUMANS_LINEAR, and mcn_rollout's own rules (a `state` without a discount table, ...).
 */
int mcn_env_rollout_orca(const mcn_env_cfg *cfg, const mcn_env_state *st, double robot_safety_space,
                         float neighbor_dist, int32_t max_neighbors, float time_horizon, int32_t T,
                         const mcn_env_out *out, const mcn_rollout *roll, double *tr_robot, double *tr_humans,
                         double *tr_hrad, double *tr_action, mcn_step_rec *tr_rec, double *tr_human_act,
                         int32_t E, int32_t N, void *stream);

/*
 * mcn_env_step_sf / mcn_env_rollout_sf -- mcn_env_step / mcn_env_rollout for social-force pedestrians
 * (cfg->human_policy == MCN_HUMANS_SOCIALFORCE; the reference has no such model, it is defined here).  Circular form of
 * Helbing, Farkas and Vicsek (2000) without body-contact or friction terms.  Human i with position p, velocity v, goal g,
 * radius r, preferred speed s chooses, all in float64 and in this operation order (no fused multiply-add):
 *   1  e = g - p; d = sqrt(e.x*e.x + e.y*e.y); if d > s: e = (e.x / d * s, e.y / d * s)      (orca.py:113's vector)
 *   2  a = (k*(e.x - v.x), k*(e.y - v.y))
 *   3  for every other human j of the env in index order, then -- if cfg->robot_visible -- the robot (current position,
 *      plain radius): dx = p.x - q.x; dy = p.y - q.y; dist = sqrt(dx*dx + dy*dy); if dist > 0:
 *      m = A * exp((r + r_j - dist) / B); a.x = a.x + m * (dx / dist); a.y = a.y + m * (dy / dist)
 *      (a coincident agent contributes nothing; radii are the plain ones: no ORCA margin, no safety_space)
 *   4  w = (v.x + a.x*dt, v.y + a.y*dt); n = sqrt(w.x*w.x + w.y*w.y)
 *   5  if n > s: w = (w.x / n * s, w.y / n * s)
 * and w is the human's action; everything after it (swept test, overlap count, reward ladder, integration, look-ahead
 * observation, rollout accounting, pool restart) is mcn_env_step's.  strength = A (m/s^2, >= 0), range = B (m, > 0),
 * relaxation_rate = k (1/s, >= 0), all finite: anything else, or another cfg->human_policy, is MCN_EINVAL before any
 * launch.  No given_v.  `update`, out->human_act, out->nobs_*, roll: as mcn_env_step.  mcn_env_rollout_sf equals T
 * mcn_env_step_sf(update = 1) calls bit for bit; in a latency-bound batch it is one launch (env_step.hip:
 * env_step_loop_sf_kernel), otherwise T launches.  The cfg's orca_* fields are not read (orca_max_neighbors is still
 * range-checked).
 */
int mcn_env_step_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                    const mcn_env_state *st, const double *actions, const mcn_env_out *out,
                    const mcn_rollout *roll, int32_t E, int32_t N, int32_t update, void *stream);
int mcn_env_rollout_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                       const mcn_env_state *st, const double *actions, int32_t T, const mcn_env_out *out,
                       const mcn_rollout *roll, int32_t E, int32_t N, void *stream);

/*
 * mcn_env_rollout_orca_sf -- mcn_env_rollout_orca over social-force pedestrians (cfg->human_policy ==
 * MCN_HUMANS_SOCIALFORCE): T consecutive closed-loop steps with an ORCA-driven holonomic robot in ONE launch (env_step.hip:
 * env_step_loop_orca_sf_kernel), for any batch and any 1 <= N <= MCN_MAX_HUMANS.  Each step equals, bit for bit, this
 * per-step sequence:
 *   1  the robot's action exactly as in mcn_env_rollout_orca's step 1 (the robot's parameters are its policy's own);
 *   2  mcn_env_step_sf(cfg, strength, range, relaxation_rate, st, that action, out, roll, E, N, update = 1),
 *      cfg->robot_visible read at run time as that call reads it.
 * strength / range / relaxation_rate: as mcn_env_step_sf.  The traces, and `st`, `out->rec`, `out->human_act` and `roll`
 * on return: as mcn_env_rollout_orca.  MCN_EINVAL before any launch: everything mcn_env_rollout_orca refuses (NULL cfg /
 * st / out, a missing state array, st->rvpref included, T < 1, N outside 1 .. MCN_MAX_HUMANS, max_neighbors outside
 * 0 .. MCN_MAX_LINES, time_horizon or time_step not positive, a robot_safety_space that is not finite, a robot that is not
 * holonomic, mcn_rollout's own rules), everything mcn_env_step_sf refuses (strength or relaxation_rate negative or not
 * finite, range not finite or not > 0), and a cfg->human_policy other than MCN_HUMANS_SOCIALFORCE.
 */
int mcn_env_rollout_orca_sf(const mcn_env_cfg *cfg, double strength, double range, double relaxation_rate,
                            const mcn_env_state *st, double robot_safety_space, float neighbor_dist,
                            int32_t max_neighbors, float time_horizon, int32_t T, const mcn_env_out *out,
                            const mcn_rollout *roll, double *tr_robot, double *tr_humans, double *tr_hrad,
                            double *tr_action, mcn_step_rec *tr_rec, double *tr_human_act, int32_t E, int32_t N,
                            void *stream);

/* Scenario rules of CrowdSim.reset (crowd_sim.py:120-163). */
enum { MCN_RULE_CIRCLE = 0, MCN_RULE_SQUARE = 1 };

typedef struct mcn_scenario_cfg {
    double circle_radius, square_width;      /* env.config [sim] */
    double discomfort_dist;                  /* env.config [reward] */
    double human_radius, human_v_pref;       /* env.config [humans] (used when randomize_attributes == 0) */
    double robot_radius;
    double robot_start[2], robot_goal[2];    /* crowd_sim.py:284 */
    int32_t rule;                            /* MCN_RULE_* */
    int32_t randomize_attributes;            /* agent.py:39-45 */
} mcn_scenario_cfg;

/*
 * mcn_scenario_pool -- P crowd scenarios of N humans generated ON the device into the pool arrays that
 * mcn_rollout's in-kernel restart reads (pool_hpos / pool_hgoal [P*N][2], pool_hrad / pool_hvpref [P*N]).
 * Replaces, for rollouts that do not need bit-parity with the reference's random stream,
 * generate_random_human_position / generate_circle_crossing_human / generate_square_crossing_human
 * (crowd_sim/envs/crowd_sim.py:94-215): same placement rules and rejection tests, counter-based random numbers
 * keyed by (seed, first_case + i), so case i is the same whatever P or the partition.  The bit-exact generator
 * (numpy MT19937, host) stays in modelcrowdnav_amd/envs/scenarios.py.
 * Where the reference would draw for ever, this does not: every rejection loop (a circle crossing's start, a square
 * crossing's start and, independently, its goal) stops after 4096 tries and keeps the draw of try 4096; the stream
 * goes on from there, and later humans are tested against that draw like against any other.  A dense crowd can
 * therefore START with humans inside a comfort gap (radius_i + radius_j + discomfort_dist) of the robot or of an
 * earlier human, i.e. with a discomfort penalty or a collision at step 0: on the shipped circle (radius 4) about 1
 * case in 17 for 10 randomized humans, 1 in 8 for 20 humans of radius 0.3, every case for 20 randomized humans (rates:
 * DESIGN.md, "Device scenario generator").  The arrays do not say which cases those are;
 * VecCrowdSim.unplaced_cases (envs/crowd_sim.py) recomputes it from them.
 */
int mcn_scenario_pool(const mcn_scenario_cfg *cfg, uint64_t seed, int64_t first_case, int32_t P, int32_t N,
                      double *hpos, double *hgoal, double *hrad, double *hvpref, void *stream);

/*
 * mcn_orca_batch -- ORCA velocity for B independent agents, each with up to M candidate
 * neighbours (float32, RVO2 semantics).  Replaces the rvo2.PyRVOSimulator
 * addAgent / setAgent... / doStep / getAgentVelocity(0) sequence of orca.py:95-129 for arbitrary agents
 * (used for an ORCA-driven robot, test.py:52 --policy orca).
 * self:   [B][8] float  (px,py,vx,vy,radius,max_speed,pref_x,pref_y)
 * others: [B][M][5] float (px,py,vx,vy,radius); n_other: [B] int32 valid counts
 * out:    [B][2] float new velocity
 */
int mcn_orca_batch(const float *self, const float *others, const int32_t *n_other, float *out,
                   int32_t B, int32_t M, float neighbor_dist, int32_t max_neighbors,
                   float time_horizon, float time_step, void *stream);

/*
 * mcn_orca_finish -- CrowdSim.get_human_times (crowd_sim/envs/crowd_sim.py:219-258) for E envs in one launch: once
 * the robot has arrived, everybody goes into ONE centralised ORCA simulation per env (the reference's
 * rvo2.PyRVOSimulator(time_step, neighbor_dist, max_neighbors, time_horizon, ...)), agent 0 being the robot and agents
 * 1 .. N the humans, each at its own plain radius and v_pref, and the simulation runs until every human has reached its
 * goal.  The step loop and the "is everybody there" test run inside the kernel.
 *   st        reads hpos, hgoal, hrad, hvpref, rpos, rgoal, rrad, rvpref, gtime, human_times (none may be NULL); writes
 *             hpos, rpos, gtime, human_times.  hvel, rvel, rtheta and hcount are neither read nor written (the
 *             reference leaves the agents' velocity fields alone here).
 *   sim_vel   [E][N+1][2] float, in and out: the simulator's velocities.  The caller starts it from float32(rvel),
 *             float32(hvel) and hands it back unchanged to continue after a capped call.
 *   select    [E] bytes or NULL: envs with select[e] == 0 are not touched in any array (steps[e] = 0).
 *   max_steps >= 1: the most steps this call simulates per env; it bounds every loop of the kernel.
 *   steps     [E] int32 out: steps simulated by this call.
 *   traj      [max_steps][E][N+1][2] float or NULL: positions after each simulated step; rows at or beyond steps[e]
 *             keep what they held.
 *   1 <= N <= MCN_MAX_HUMANS (at most 32 candidate neighbours per agent), 0 <= max_neighbors <= MCN_MAX_LINES,
 *   time_step > 0, time_horizon > 0; anything else, or a NULL st / sim_vel / steps: MCN_EINVAL before any launch.
 * Per selected env, with p64 the agent's float64 position in st and p32 = float32(p64) at entry: while some
 * human_times[e][i] == 0 and fewer than max_steps steps have been taken, in this operation order and without fused
 * multiply-add:
 *   1  every agent: e = goal - p64 (float64); n = sqrt(e.x*e.x + e.y*e.y); if n > 1: e = (e.x / n, e.y / n);
 *      pref = float32(e)
 *   2  every agent: the ORCA solve of mcn_orca_batch with the other N agents as candidates in agent-index order, all
 *      agents' p32 and sim_vel from before this step, radius float32(radius), max speed float32(v_pref), pref,
 *      neighbor_dist, max_neighbors, time_horizon, float32(time_step)
 *   3  sim_vel = the new velocity; p32 = p32 + sim_vel * float32(time_step) (one float32 product, one float32 sum)
 *   4  gtime = gtime + time_step (float64)
 *   5  every human with human_times == 0: d = p64 - goal with the position from BEFORE this step's update;
 *      if sqrt(d.x*d.x + d.y*d.y) < radius (float64): human_times = gtime
 *   6  p64 = float64(p32); written back to st when the env stops
 * An env whose human_times are all non-zero at entry takes no step and nothing of it is written.  Two calls that
 * together take as many steps as one uncapped call leave the same bytes.
 */
int mcn_orca_finish(const mcn_env_state *st, float *sim_vel, const uint8_t *select, int32_t max_steps, int32_t *steps,
                    float *traj, double time_step, float neighbor_dist, int32_t max_neighbors, float time_horizon,
                    int32_t E, int32_t N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * SARL attention value network: 81-action one-step look-ahead (crowd_nav/policy/sarl.py:28-65,
 * multi_human_rl.py:11-63, cadrl.py:104-129,217-252).
 * ---------------------------------------------------------------------------------------------- */

/*
 * mcn_pack_linear -- HOST helper: permute one nn.Linear (weight [nout][kin] row-major, bias [nout])
 * into the MFMA operand order the network kernels stream (see mfma_chain.hpp; used for SARL and SGAN).  kmap[t*16 + s] is the column of
 * `weight` that input slot s of input tile t carries, or -1 for padding; KT input tiles.  omap[n*16 + s] is the
 * row of `weight` produced in output slot s of output tile n, or -1 (NULL = identity: row 16n + s); NT output
 * tiles.  Slot s = 4q + r lives in accumulator register r of lane group q, so a ragged last tile packed
 * "q first" (feature j at slot 4(j%4) + j/4) needs only ceil(w/4) k-steps in the layer that consumes it.
 * wfrag_out: [NT][KT][64][4] floats, bfrag_out: [NT][64][4] floats (may be NULL).
 */
int mcn_pack_linear(const float *weight, const float *bias, int32_t nout, int32_t kin,
                    const int32_t *kmap, int32_t KT, const int32_t *omap, int32_t NT,
                    float *wfrag_out, float *bfrag_out);

/*
 * mcn_pack_x3 -- HOST helper: regroup float32 weight fragments ([NT][KT][64][4] floats, mcn_pack_linear's wfrag_out)
 * for the bf16 matrix pipe: every weight as three bfloat16 pieces hi + mid + lo (round-to-nearest-even, exact to
 * 2^-24), per (output tile, 32-feature input block) three 16-byte rows per lane:
 * x3_out [NT][ceil(KT / 2)][3][64][8] bfloat16 (mcn_pack_x3_bytes bytes).  With these the look-ahead kernels run
 * v_mfma_f32_16x16x32_bf16 on six of the nine piece products instead of v_mfma_f32_16x16x4_f32: float32-accurate
 * (error against float64 as the float32 chain's), ~2.7 x fewer matrix-pipe cycles.
 */
int64_t mcn_pack_x3_bytes(int32_t NT, int32_t KT);
int mcn_pack_x3(const float *wfrag, int32_t NT, int32_t KT, void *x3_out);

/* Device pointers to the bf16x3 fragments of one ValueNetwork (biases stay the float32 fragments of mcn_sarl_net). */
typedef struct mcn_sarl_x3 {
    const void *w_m1a, *w_m1b, *w_m2a, *w_m2b, *w_ata, *w_atg, *w_atb, *w_atc, *w_m3a, *w_m3b, *w_m3c, *w_m3d;
} mcn_sarl_x3;

/* Device pointers to the packed fragments of one ValueNetwork (state_dict keys in comments). */
typedef struct mcn_sarl_net {
    const float *w_m1a, *b_m1a;   /* mlp1.0        13 -> 150 */
    const float *w_m1b, *b_m1b;   /* mlp1.2       150 -> 100 */
    const float *w_m2a, *b_m2a;   /* mlp2.0       100 -> 100 */
    const float *w_m2b, *b_m2b;   /* mlp2.2       100 -> 50  */
    const float *w_ata, *b_ata;   /* attention.0  columns   0..99  (per-human half) + bias */
    const float *w_atg;           /* attention.0  columns 100..199 (global-state half)     */
    const float *w_atb, *b_atb;   /* attention.2  100 -> 100 */
    const float *w_atc, *b_atc;   /* attention.4  100 -> 1   */
    const float *w_m3a, *b_m3a;   /* mlp3.0        56 -> 150 (input tiles: pooled x4, self x1) */
    const float *w_m3b, *b_m3b;   /* mlp3.2       150 -> 100 */
    const float *w_m3c, *b_m3c;   /* mlp3.4       100 -> 100 */
    const float *w_m3d, *b_m3d;   /* mlp3.6       100 -> 1   */
    const mcn_sarl_x3 *x3;        /* HOST pointer or NULL: when set, the layers run on the bf16 pipe from these fragments
                                   * (ABI 5; the float32 fragments above are still required: biases, and the fallback) */
} mcn_sarl_net;

/* Bytes of device workspace mcn_sarl_lookahead needs for (E, N, A): one slot per RESIDENT wavefront of the persistent
 * grid (at most 2 048), N x 12 KiB each (the bf16x3 path parks mlp1's output already split; the float32 path uses
 * 7 KiB of it) -- 123 MB at N = 5, whatever E. */
int64_t mcn_sarl_workspace_bytes(int32_t E, int32_t N, int32_t A);

/*
 * mcn_sarl_lookahead -- for every env and every candidate action: propagate, reward, rotate, value
 * network, value = reward + gamma_pow * V; then the first-max-wins argmax.
 * Replaces the `for action in self.action_space` loop of MultiHumanRL.predict (multi_human_rl.py:35-55).
 * actions: [A][2] device; values: [E][A] device out; best: [E] int32 out (-1 = robot already at its goal,
 * multi_human_rl.py:22; may be NULL); best_val: [E]; attention: [E][A][N] float out or NULL.
 * gamma_pow = pow(gamma, time_step * v_pref) computed by the caller (multi_human_rl.py:52).
 * Values are NaN where the reference's are (its masked softmax, exp(s) (s != 0) / sum, is not stabilised): for an env
 * with a NaN or infinite feature in a pedestrian it sees or in the robot, for an action row that holds one, where every
 * score of the env's pedestrians is exactly 0 or every exp(score) underflows (0 / 0) and where an exp(score)
 * overflows (inf / inf); `attention` is NaN there too, for the pedestrians the env sees, and exactly 0 for the slots
 * beyond hcount.  NaN values never win the argmax: an env whose values are all NaN reports best = -1, best_val = -inf.
 * Sums of exp(score) down to the smallest float32 subnormal give finite values, as the reference's division does.
 */
int mcn_sarl_lookahead(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                       double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                       double *values, int32_t *best, double *best_val, float *attention,
                       int32_t E, int32_t N, void *stream);

/*
 * mcn_sarl_lookahead_env -- the same look-ahead with `query_env = true` (multi_human_rl.py:37-38, cadrl.py:158-159):
 * the humans' next states and the per-action rewards are what the env's own one-step look-ahead returned
 * (CrowdSim.onestep_lookahead, crowd_sim.py:325-329) instead of constant-velocity propagation + compute_reward.
 * next_hpos / next_hvel: [E*N][2] -- out->nobs_pos / nobs_vel of one mcn_env_step(update = 0) (the humans' reaction
 * does not depend on the candidate action: they see the robot's current state, crowd_sim.py:336-342);
 * rewards: [E][A] -- reward of mcn_env_step for every (env, action).  Everything else as mcn_sarl_lookahead.
 */
int mcn_sarl_lookahead_env(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                           double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                           double *values, int32_t *best, double *best_val, float *attention,
                           const double *next_hpos, const double *next_hvel, const double *rewards,
                           int32_t E, int32_t N, void *stream);

/*
 * mcn_sarl_predict -- the look-ahead AND the action MultiHumanRL.predict returns (multi_human_rl.py:22-23,53-63), for
 * every env, with no host round trip: action_out[e] = actions[best[e]], or (0, 0) where best[e] == -1 (robot on its
 * goal) or every value is NaN (best[e] < 0 with best_val = -inf: "Value network is not well trained", the caller's
 * error).  next_hpos / next_hvel / rewards: all NULL (mcn_sarl_lookahead's propagate + compute_reward) or all set
 * (mcn_sarl_lookahead_env's `query_env` form).  action_out: [E][2] device out.  Everything else as above.
 * epsilon > 0 (phase 'train', multi_human_rl.py:27-29): each env not on its goal independently takes, with
 * probability epsilon, a uniformly drawn row of `actions` instead of the best one (best[e] = -2); the draws are a
 * counter-based function of (seed, env), so pass a fresh seed per call.  epsilon = 0: greedy, seed ignored.
 */
int mcn_sarl_predict(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                     double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                     double *values, int32_t *best, double *best_val, float *attention,
                     const double *next_hpos, const double *next_hvel, const double *rewards,
                     double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream);

/*
 * OM-SARL (`[sarl] with_om = true`): mlp1.0 is 61 -> 150 on [13 rotated features | 48 occupancy-map entries].
 *
 * mcn_sarl_om_prepare -- once per step, for the first hcount[e] humans of every env (hcount as in the look-ahead,
 * clamped to 1 .. N): MultiHumanRL.build_occupancy_maps (multi_human_rl.py:109-163) with cell_num = 4 and
 * om_channel_size = 3 -- a 4 x 4 grid of `cell_size` cells centred on the human, +x along its velocity; per cell
 * [occupied by another human of the env, mean vx, mean vy of those humans in the turned frame], entry 3 cell + channel,
 * cell = 4 iy + ix; float64 in the reference's operation sequence, stored as float32.  The humans' states are
 * next_hpos / next_hvel ([E*N][2], both or neither: the `query_env` form) when given, else hpos + time_step * hvel
 * with hvel (the look-ahead's constant-velocity propagation), or the current ones for time_step = 0 (what
 * MultiHumanRL.transform stores).  A human with a non-finite coordinate falls into no cell.  Rows the reference has
 * no answer for are ZERO maps: humans at index >= hcount[e] (which are in nobody's map either) and the single human
 * of an env with hcount[e] = 1 (or N = 1), where the reference's np.concatenate of an empty list raises.
 * om: [E][N][48] float32 device out.  w_om / b_om: device fragments of mlp1.0.weight[:, 13:61] (mcn_pack_linear with
 * three natural input tiles over columns 13 .. 60 and ten output tiles in mcn_sarl_net's ragged-tile order) and of
 * mlp1.0.bias; init: [E][N][160] float32 device out, W[:, 13:61] om + bias in that output-slot order -- what
 * mcn_sarl_predict_om starts mlp1.0's accumulators from.  w_om, b_om and init are given together or all NULL (maps only).
 */
int mcn_sarl_om_prepare(const mcn_env_state *st, double time_step, const double *next_hpos, const double *next_hvel,
                        double cell_size, const float *w_om, const float *b_om, float *om, float *init,
                        int32_t E, int32_t N, void *stream);

/*
 * mcn_sarl_predict_om -- mcn_sarl_predict for an OM-SARL network: net->w_m1a holds mlp1.0.weight[:, 0:13] as for SARL,
 * net->b_m1a is not read, and `om_init` ([E][N][160], mcn_sarl_om_prepare's `init` of the same step, same stream) is
 * where mlp1.0 starts from for all A actions of an env.  Same workspace, same MFMA work per (env, action) as SARL.
 */
int mcn_sarl_predict_om(const mcn_sarl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                        double time_step, double gamma_pow, int32_t kinematics, void *workspace,
                        double *values, int32_t *best, double *best_val, float *attention,
                        const double *next_hpos, const double *next_hvel, const double *rewards,
                        double *action_out, double epsilon, uint64_t seed, const float *om_init,
                        int32_t E, int32_t N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * LSTM-RL and CADRL value networks: the same 81-action one-step look-ahead (crowd_nav/policy/lstm_rl.py:9-33,90-103,
 * cadrl.py:21-29,131-178, multi_human_rl.py:11-63).  float32 MFMA layers only (no x3 fragments).
 * ---------------------------------------------------------------------------------------------- */

/* Device pointers to the packed fragments of one LSTM-RL ValueNetwork1 (with_interaction_module = false). */
typedef struct mcn_lstm_rl_net {
    const float *w_gate, *b_gate; /* lstm: [weight_ih_l0 | weight_hh_l0] (13 + 50) -> 200, bias_ih_l0 + bias_hh_l0;
                                   * input tiles x, h x4; output tile 4G + t slot s = unit u of gate G (i, f, g, o)
                                   * where (t, s) is the slot of unit u of h */
    const float *w_m0, *b_m0;     /* mlp.0  56 -> 150 (input tiles: self x1, h x4) */
    const float *w_m1, *b_m1;     /* mlp.2 150 -> 100 */
    const float *w_m2, *b_m2;     /* mlp.4 100 -> 100 */
    const float *w_m3, *b_m3;     /* mlp.6 100 -> 1   */
} mcn_lstm_rl_net;

/* Device pointers to the packed fragments of one CADRL ValueNetwork (state_dict value_network.{0,2,4,6}). */
typedef struct mcn_cadrl_net {
    const float *w_l0, *b_l0;     /* value_network.0  13 -> 150 */
    const float *w_l1, *b_l1;     /* value_network.2 150 -> 100 */
    const float *w_l2, *b_l2;     /* value_network.4 100 -> 100 */
    const float *w_l3, *b_l3;     /* value_network.6 100 -> 1   */
} mcn_cadrl_net;

/*
 * mcn_lstm_rl_predict -- mcn_sarl_predict for LstmRL (lstm_rl.py:90-103): per env the humans are taken in the order
 * LstmRL.predict sorts them, by decreasing float64 distance of their CURRENT position to the robot's current position
 * (np.linalg.norm, lstm_rl.py:99-101), equal distances in index order (sorted(reverse=True) is stable), NaN distances
 * last in index order, over the first hcount[e] humans only; the LSTM starts from h = c = 0 and humans at index >= hcount[e] do not touch it.  With
 * next_hpos / next_hvel / rewards set (`query_env`, multi_human_rl.py:37-38) the env's next states are taken in the
 * env's order, as the reference does.  order: [E][N] int32 device out or NULL: the human index at each LSTM step (slots
 * >= hcount[e] hold their own index).  No workspace.  Everything else as mcn_sarl_predict.
 */
int mcn_lstm_rl_predict(const mcn_lstm_rl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                        double time_step, double gamma_pow, int32_t kinematics,
                        double *values, int32_t *best, double *best_val, int32_t *order,
                        const double *next_hpos, const double *next_hvel, const double *rewards,
                        double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream);

/*
 * mcn_lstm_rl_order -- the human order of mcn_lstm_rl_predict (without query_env) on its own, for the rows
 * LstmRL.transform stores (multi_human_rl.py:60-61 on the sorted state).  Reads st->hpos, st->rpos and st->hcount
 * (may be NULL); order: [E][N] int32 device out.
 */
int mcn_lstm_rl_order(const mcn_env_state *st, int32_t *order, int32_t E, int32_t N, void *stream);

/*
 * mcn_cadrl_predict -- mcn_sarl_predict for CADRL (cadrl.py:131-178): the value network on every (robot, human) row,
 * V = min over the env's first hcount[e] humans (torch.min: one NaN makes V NaN), value = reward + gamma_pow * V.
 * No workspace.  Everything else as mcn_sarl_predict.
 */
int mcn_cadrl_predict(const mcn_cadrl_net *net, const mcn_env_state *st, const double *actions, int32_t A,
                      double time_step, double gamma_pow, int32_t kinematics,
                      double *values, int32_t *best, double *best_val,
                      const double *next_hpos, const double *next_hvel, const double *rewards,
                      double *action_out, double epsilon, uint64_t seed, int32_t E, int32_t N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * SARL value-network training step (crowd_nav/utils/trainer.py:64-82 on crowd_nav/policy/sarl.py:28-65).
 * ---------------------------------------------------------------------------------------------- */

/*
 * The network is the shipped SARL ValueNetwork with the global state on: input_dim 13 (SARL) or 61 (OM-SARL),
 * self_state_dim 6, mlp1 150-100, mlp2 100-50, attention 100-100-1, mlp3 150-100-100-1.  Parameters, gradient and
 * momentum are each ONE flat float32 device buffer in state_dict order -- mlp1.0.weight, mlp1.0.bias, mlp1.2.*, mlp2.0.*,
 * mlp2.2.*, attention.0.*, attention.2.*, attention.4.*, mlp3.0.*, mlp3.2.*, mlp3.4.*, mlp3.6.* -- every weight row-major
 * [out][in] as torch stores it: mcn_sarl_train_param_count floats, 96502 for input_dim 13 and 103702 for 61, -1 for any
 * other input_dim.
 */
int64_t mcn_sarl_train_param_count(int32_t input_dim);
int64_t mcn_sarl_train_workspace_bytes(int32_t B, int32_t N, int32_t input_dim);    /* 0 for arguments the step refuses */

/*
 * mcn_sarl_loss_grad -- loss = mean_b (V(states[rows[b]]) - values[rows[b]])^2 over a mini-batch of B states and its
 * gradient by every parameter, with the semantics of torch autograd on ValueNetwork.forward in float32: the softmax is
 * the un-stabilised exp(s) (s != 0) / sum with the mask a constant, ReLU passes gradient where its output is > 0, and
 * where torch gives NaN (a state whose scores are all exactly 0 is 0 / 0) so does this.
 * states: [rows of the memory][N][input_dim] float, values: [rows of the memory] float, both device.  rows: [B] int64
 * device, the memory row of each state of the batch, or NULL for rows 0 .. B-1.  The kernel TRUSTS the row indices:
 * the caller checks them against the number of rows the memory holds before it uploads them.
 * workspace: mcn_sarl_train_workspace_bytes(B, N, input_dim) device bytes, 8-byte aligned; grad: [param_count] float
 * device out; loss: [1] float device out.  Two launches on `stream` (per-workgroup partial gradients, then their sum in
 * workgroup order): no atomics, so the same inputs give the same bits.  The forward pass and the sums over the batch run
 * in float64, the backward pass in float32: loss and grad are within float32 rounding of float64 autograd's, and the
 * gradient of attention.4.bias, which the softmax makes 0, is returned as exactly 0 (or NaN).
 * MCN_EINVAL before any launch: a NULL params / states / values / workspace / grad / loss, B < 1, N outside
 * 1 .. MCN_MAX_HUMANS, an input_dim other than 13 / 61.
 */
int mcn_sarl_loss_grad(const float *params, int32_t input_dim, const float *states, const float *values,
                       const int64_t *rows, int32_t B, int32_t N, void *workspace, float *grad, float *loss, void *stream);

/*
 * mcn_sgd_momentum_step -- torch.optim.SGD(momentum) without dampening, weight decay or Nesterov over flat float32
 * device buffers of `count` elements: buf = momentum buf + grad, p = p - lr buf (the latter one fused multiply-add, as
 * torch's p.add_(buf, alpha=-lr)).  A zero buf makes it torch's first step.  One launch on `stream`.
 * MCN_EINVAL before any launch: a NULL pointer, count < 1, an lr or momentum that is not finite.
 */
int mcn_sgd_momentum_step(float *params, float *momentum_buf, const float *grad, int64_t count, float lr, float momentum,
                          void *stream);

/* ------------------------------------------------------------------------------------------------
 * CADRL and LSTM-RL value-network training steps (crowd_nav/utils/trainer.py:64-82 on crowd_nav/policy/cadrl.py:21-29 and
 * crowd_nav/policy/lstm_rl.py:9-33).  The update of both is mcn_sgd_momentum_step.
 * ---------------------------------------------------------------------------------------------- */

/*
 * The network is the shipped CADRL ValueNetwork: value_network 13-150-100-100-1 with ReLU between the layers.
 * Parameters, gradient and momentum are each ONE flat float32 device buffer in state_dict order -- value_network.0.weight,
 * value_network.0.bias, value_network.2.*, value_network.4.*, value_network.6.* -- every weight row-major [out][in] as
 * torch stores it: mcn_cadrl_train_param_count() = 27401 floats.
 */
int64_t mcn_cadrl_train_param_count(void);
int64_t mcn_cadrl_train_workspace_bytes(int32_t B);                                 /* 0 for arguments the step refuses */

/*
 * mcn_cadrl_loss_grad -- loss = mean_b (V(states[rows[b]]) - values[rows[b]])^2 over a mini-batch of B states and its
 * gradient by every parameter, with the semantics of torch autograd on ValueNetwork.forward in float32: ReLU passes
 * gradient where its output is > 0, and NaN goes where torch's goes.
 * states: [rows of the memory][13] float (one rotated joint row per state), values: [rows of the memory] float, both
 * device.  rows: [B] int64 device, the memory row of each state of the batch, or NULL for rows 0 .. B-1.  The kernel
 * TRUSTS the row indices: the caller checks them against the number of rows the memory holds before it uploads them.
 * workspace: mcn_cadrl_train_workspace_bytes(B) device bytes, 8-byte aligned; grad: [param_count] float device out;
 * loss: [1] float device out.  Two launches on `stream` (per-workgroup partial gradients of 8 states each, then their sum
 * in workgroup order): no atomics, so the same inputs give the same bits.  The forward pass and the sums over the batch
 * run in float64, the backward pass in float32: loss and grad are within float32 rounding of float64 autograd's; the loss
 * and the gradient of value_network.6.bias are float64 sums rounded once.
 * MCN_EINVAL before any launch: a NULL params / states / values / workspace / grad / loss, B < 1.
 */
int mcn_cadrl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int32_t B,
                        void *workspace, float *grad, float *loss, void *stream);

/*
 * The network is the shipped LSTM-RL ValueNetwork1: nn.LSTM(13, 50, batch_first) over the N rows of a state from zero
 * h0 / c0, then mlp 56-150-100-100-1 on [columns 0 .. 5 of the state's row 0 | h_N].  The flat float32 buffers are in
 * state_dict order, which puts the MLP FIRST: mlp.0.weight, mlp.0.bias, mlp.2.*, mlp.4.*, mlp.6.*, lstm.weight_ih_l0
 * [200][13], lstm.weight_hh_l0 [200][50], lstm.bias_ih_l0 [200], lstm.bias_hh_l0 [200]; the gate rows are torch's (i, f, g,
 * o: rows 0-49, 50-99, 100-149, 150-199).  mcn_lstm_rl_train_param_count() = 46851 floats.
 */
int64_t mcn_lstm_rl_train_param_count(void);
int64_t mcn_lstm_rl_train_workspace_bytes(int32_t B, int32_t N);                    /* 0 for arguments the step refuses */

/*
 * mcn_lstm_rl_loss_grad -- the same loss and its gradient for ValueNetwork1, with the semantics of torch autograd on its
 * forward in float32: gates_t = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh, c_t = f c_{t-1} + i g, h_t = o tanh(c_t);
 * sigmoid' = y (1 - y), tanh' = 1 - y^2, ReLU passes gradient where its output is > 0, NaN goes where torch's goes.
 * states: [rows of the memory][N][13] float, the rows of a state in the order the LSTM takes them (the memory holds them
 * sorted by LstmRL.transform_batch: nothing is sorted here); values, rows, workspace (mcn_lstm_rl_train_workspace_bytes(B,
 * N) bytes), grad, loss and the two launches as for mcn_cadrl_loss_grad, a workgroup taking 8 / N states for N <= 4 and one
 * state above; every activation of every step stays in LDS for all N <= MCN_MAX_HUMANS.  h and c are carried in float64
 * and the gates' sigmoid and tanh are evaluated in float64 (finite for any finite pre-activation); back through time runs
 * in float32.  lstm.bias_ih_l0 and lstm.bias_hh_l0 get the same bits; with N = 1 (h_0 = 0) lstm.weight_hh_l0 gets exactly
 * 0.
 * MCN_EINVAL before any launch: a NULL params / states / values / workspace / grad / loss, B < 1, N outside
 * 1 .. MCN_MAX_HUMANS.
 */
int mcn_lstm_rl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int32_t B,
                          int32_t N, void *workspace, float *grad, float *loss, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Social-GAN one-step world model (crowd_nav/policy/world_model.py:134-268, sgan/models.py:501-553).
 * ---------------------------------------------------------------------------------------------- */

/* Device pointers to packed fragments of one TrajectoryGenerator (shipped architecture: embedding 16,
 * encoder/decoder hidden 32, mlp 64, bottleneck 8, noise 8 'global', pool hidden 512, no batch norm).
 * The three spatial_embedding layers (Linear(2, 16), models.py:47,120,186) feed a Linear / LSTM input directly, so the
 * packer folds them into it (in float64, rounded once): a layer "W [emb | h] , b" arrives here as
 * "[W_emb W_se | W_h] , b + W_emb b_se" with 2 + 32 input columns.  Input tile 0 carries the displacement: x in slot
 * 0, y in slot 4 (both in MFMA k-step 0), tiles 1-2 the 32 hidden features. */
typedef struct mcn_sgan_net {
    const float *w_elstm, *b_elstm;   /* encoder: [weight_ih_l0 W_se | weight_hh_l0], bias_ih + bias_hh + weight_ih b_se */
    const float *w_p1, *b_p1;         /* pool_net.mlp_pre_pool.0 folded with pool_net.spatial_embedding (pooling only) */
    const float *w_p2, *b_p2;         /* pool_net.mlp_pre_pool.2                                         (pooling only) */
    const float *w_c1, *b_c1;         /* mlp_decoder_context.0 */
    const float *w_c2, *b_c2;         /* mlp_decoder_context.2 */
    const float *w_dlstm, *b_dlstm;   /* decoder: folded like the encoder's */
    const float *w_h2p, *b_h2p;       /* decoder.hidden2pos */
    int32_t pooling;                  /* 1: pooling_type == 'pool_net', 0: none */
} mcn_sgan_net;

int64_t mcn_sgan_workspace_bytes(int32_t E, int32_t N);

/*
 * mcn_sgan_step -- one SGANWorld.forward for E scenes of N pedestrians.
 * hist: [E][8][N][2] float64 ring of positions already rounded to 1e-4.  If cur_pos ([E*N][2]) is not NULL it
 * is rounded and written to ring slot `push_slot` first (the frame the reference appends to its cache file,
 * world_model.py:238-240).  `oldest` is the ring slot of the oldest of the 8 frames AFTER that push.
 * noise: [E][8] float (user_noise, sgan/models.py:475); out_vel: [E*N][2] float64 velocities
 * (world_model.py:266-268); out_rel: [E*N][2] float predicted displacement or NULL.
 * hcount: [E] or NULL -- pedestrians present in scene e (1 <= hcount[e] <= N): the pooling module looks only at
 * partners k < hcount[e] (a scene of hcount[e] pedestrians in the reference); outputs of slots >= hcount[e] are
 * meaningless.
 */
int mcn_sgan_step(const mcn_sgan_net *net, double *hist, int32_t push_slot, int32_t oldest, const double *cur_pos,
                  const float *noise, const int32_t *hcount, void *workspace, double *out_vel, float *out_rel,
                  double time_step, int32_t E, int32_t N, void *stream);

/*
 * mcn_sgan_predict -- TrajectoryGenerator.forward with decoder.seq_len = T (sgan/models.py:501-553, Decoder.forward
 * :127-164) for K user_noise vectors per scene (the K samples of generator_step's best_k / evaluate's num_samples),
 * from the ring as it stands: nothing is pushed, hist is only read.  `oldest`, `hcount` and `workspace`
 * (mcn_sgan_workspace_bytes(E, N)) as in mcn_sgan_step.  The encoder, the pooling module and mlp_decoder_context do not
 * depend on the noise or on the decoder step (pool_every_timestep = False), so they run once; the K T decoder cells
 * follow in one kernel, each step's displacement being the next step's input (:156-158).
 * noise: [K][E][8] float; out_rel: [K][T][E*N][2] float, pred_traj_fake_rel of sample k;
 * out_pos: [K][T][E*N][2] float64 or NULL: the last observed position (as float32, what the decoder holds) plus the
 * running float64 sum of those float32 displacements (relative_to_abs, sgan/utils.py:85-98, without float32 drift).
 * K < 1, K > 65535, T < 1 or a NULL net / hist / noise / workspace / out_rel: MCN_EINVAL, nothing is launched.
 * K = T = 1 gives out_rel of mcn_sgan_step(cur_pos = NULL) bit for bit.
 */
int mcn_sgan_predict(const mcn_sgan_net *net, const double *hist, int32_t oldest, const float *noise, int32_t K, int32_t T,
                     const int32_t *hcount, void *workspace, float *out_rel, double *out_pos, int32_t E, int32_t N,
                     void *stream);

/* ------------------------------------------------------------------------------------------------
 * MlpWorld one-step world model (crowd_nav/policy/world_model.py:22-42).
 * ---------------------------------------------------------------------------------------------- */

/* Device pointers to the four Linear layers of MlpWorld.mlp (state_dict keys mlp.0 / mlp.3 / mlp.6 / mlp.8), packed by
 * mcn_pack_linear: mlp.0 with KT = ceil(4N / 16) natural input tiles and 8 output tiles; mlp.3 8 -> 4 tiles; mlp.6
 * 4 -> 1 tile with its 12 outputs packed "q first" (omap: feature j at slot 4 (j % 4) + j / 4); mlp.8 with the matching
 * kmap, 1 input tile, ceil(2N / 16) natural output tiles. */
typedef struct mcn_mlp_world_net {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
} mcn_mlp_world_net;

/*
 * mcn_mlp_world_step -- MlpWorld.forward (eval mode: dropout is the identity) for E scenes of N <= 10 pedestrians:
 * input row = the scene's [px, py, vx, vy] x N as float32 (model_crowd_sim.py:401-405), output = the N predicted
 * velocities (tanh of mlp.8's output, world_model.py:33-35) as float64 [E*N][2] -- what ModelCrowdSim.step hands to
 * humans[i].step(ActionXY(new_v[i])) (model_crowd_sim.py:406-417), i.e. mcn_env_step's given_v.
 */
int mcn_mlp_world_step(const mcn_mlp_world_net *net, const double *hpos, const double *hvel, double *out_vel,
                       int32_t E, int32_t N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * AttentionWorld one-step world model (crowd_nav/policy/world_model.py:54-106).
 * ---------------------------------------------------------------------------------------------- */

/* Device pointers to the packed fragments of one AttentionWorld (state_dict keys in comments; ragged tiles packed
 * "q first" as for mcn_sarl_net).  The 4-wide pedestrian state [px, py, vx, vy] is one input tile with feature c in
 * slot 4 c (one MFMA k-step). */
typedef struct mcn_attn_world_net {
    const float *w_m1a, *b_m1a;   /* mlp1.0         4 -> 150 */
    const float *w_m1b, *b_m1b;   /* mlp1.2       150 -> 100 */
    const float *w_m2a, *b_m2a;   /* mlp2.0       100 -> 100 */
    const float *w_m2b, *b_m2b;   /* mlp2.2       100 -> 50  */
    const float *w_ata, *b_ata;   /* attention.0  columns   0..99  (per-pedestrian half) + bias */
    const float *w_atg;           /* attention.0  columns 100..199 (global-state half)          */
    const float *w_atb, *b_atb;   /* attention.2  100 -> 100 */
    const float *w_atc, *b_atc;   /* attention.4  100 -> 1   */
    const float *w_m3p, *b_m3p;   /* mlp3.0       columns 4..53 (pooled feature) + bias: 50 -> 150 */
    const float *w_m3s;           /* mlp3.0       columns 0..3  (the pedestrian's own state): 4 -> 150 */
    const float *w_m3b, *b_m3b;   /* mlp3.2       150 -> 100 */
    const float *w_m3c, *b_m3c;   /* mlp3.4       100 -> 100 */
    const float *w_m3d, *b_m3d;   /* mlp3.6       100 -> 2 (natural row order) */
} mcn_attn_world_net;

int64_t mcn_attn_world_workspace_bytes(int32_t E, int32_t N);

/*
 * mcn_attn_world_step -- AttentionWorld.forward for E scenes of N pedestrians: input = each pedestrian's
 * [px, py, vx, vy] as float32 (model_crowd_sim.py:401-405), output = its predicted velocity (mlp3's two outputs, no
 * output non-linearity, world_model.py:104-105) as float64 [E*N][2].  hcount ([E] int32 or NULL): scene e has only
 * its first hcount[e] pedestrians (the rest of the N slots is ignored and not written).  A scene whose present
 * pedestrians all score exactly 0 (the softmax exp(s) (s != 0) / sum is 0 / 0) gets NaN velocities, as the module does.
 */
int mcn_attn_world_step(const mcn_attn_world_net *net, const double *hpos, const double *hvel, const int32_t *hcount,
                        void *workspace, double *out_vel, int32_t E, int32_t N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * AttentionWorld training step (crowd_nav/utils/trainer_sim.py:48-110 on crowd_nav/policy/world_model.py:54-106).
 * ---------------------------------------------------------------------------------------------- */

/*
 * The network is the default AttentionWorld: input_dim 4, global state on, mlp1 150-100, mlp2 100-50, attention
 * 100-100-1, mlp3 (54 inputs: a pedestrian's own state and the scene's pooled feature) 150-100-100-2.  Parameters,
 * gradient and the two Adam moments are each ONE flat float32 device buffer in state_dict order -- mlp1.0.weight,
 * mlp1.0.bias, mlp1.2.*, mlp2.0.*, mlp2.2.*, attention.0.*, attention.2.*, attention.4.*, mlp3.0.*, mlp3.2.*, mlp3.4.*,
 * mlp3.6.* -- every weight row-major [out][in] as torch stores it: mcn_attn_world_train_param_count() = 94953 floats.
 */
int64_t mcn_attn_world_train_param_count(void);
int64_t mcn_attn_world_train_workspace_bytes(int32_t B, int32_t N);                 /* 0 for arguments the step refuses */

/*
 * mcn_attn_world_loss_grad -- loss = mean((model(cur[rows]) - nxt[rows])^2) over the B 2N outputs of a mini-batch of B
 * scenes of N pedestrians, and its gradient by every parameter, with the semantics of torch autograd on
 * AttentionWorld.forward: the softmax is the un-stabilised exp(s) (s != 0) / sum with the mask a constant, the global
 * state is the mean of mlp1's output over the scene, ReLU passes gradient where its output is > 0, and where torch gives
 * NaN (a scene whose scores are all exactly 0 is 0 / 0) so does this.
 * cur: [rows of the memory][4N] float, nxt: [rows of the memory][2N] float, both device.  rows: [B] int64 device, the
 * memory row of each scene of the batch, or NULL for rows 0 .. B-1.  The kernel TRUSTS the row indices: the caller checks
 * them against the number of rows the memory holds before it uploads them.
 * workspace: mcn_attn_world_train_workspace_bytes(B, N) device bytes, 8-byte aligned; grad: [param_count] float device
 * out, or NULL for the loss alone (the forward pass only; nothing but `loss` is written for the caller); loss: [1] float
 * device out, written by the second launch only.  Two launches on `stream` (per-workgroup loss and partial gradients,
 * then their sum in workgroup order): no atomics, so the same inputs give the same bits, and the loss has the same bits
 * with and without a gradient.  The forward pass and the sums over the batch run in float64, the backward pass in
 * float32: loss and grad are within float32 rounding of float64 autograd's, mlp3.6.bias comes from float64 sums, and the
 * gradient of attention.4.bias, which the softmax makes 0, is returned as exactly 0 (or NaN).  Up to 16 rows (scenes x
 * pedestrians) per workgroup every activation is in LDS; from N = 17 on the float64 buffers and mlp3's activations of a
 * scene are in the workspace.
 * MCN_EINVAL before any launch: a NULL params / cur / nxt / workspace / loss, B < 1, N outside 1 .. MCN_MAX_HUMANS.
 */
int mcn_attn_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int32_t B,
                             int32_t N, void *workspace, float *grad /* or NULL */, float *loss, void *stream);

/*
 * mcn_adam_step -- torch.optim.Adam without weight decay or amsgrad over flat float32 device buffers of `count`
 * elements, step number `step` >= 1: m = beta1 m + (1 - beta1) g, v = beta2 v + (1 - beta2) g^2,
 * p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps), each element in float64 and rounded once per
 * stored value.  Zero moments with step = 1 make it torch's first step; a gradient of exactly 0 with zero moments leaves
 * the parameter's bits.  One launch on `stream`.  torch applies lr, the betas and eps as the float64 values the user
 * wrote; each arrives here as float32 and is taken as the shortest decimal that rounds to it (0.001f means 0.001), so a
 * value of up to 7 significant digits is applied exactly as torch applies it.
 * MCN_EINVAL before any launch: a NULL pointer, count < 1, step < 1, an lr, eps or beta that is not finite, a beta
 * outside [0, 1).
 */
int mcn_adam_step(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t count, float lr, float beta1,
                  float beta2, float eps, int32_t step, void *stream);

/* ------------------------------------------------------------------------------------------------
 * MlpWorld training step (crowd_nav/utils/trainer_sim.py:48-110 on crowd_nav/policy/world_model.py:22-51).
 * ---------------------------------------------------------------------------------------------- */

/*
 * The dropout mask of the MlpWorld training step.  torch's Philox stream cannot be reproduced from outside torch, so the
 * step draws its masks from a stateless counter hash, the same code on the host and on the device
 * (csrc/dropout_hash.hpp).  All arithmetic is on uint64 and wraps:
 *
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 *   key  = mix(seed + 0x9E3779B97F4A7C15 * (2 * step + layer + 1))
 *   r    = mix(key  + 0x9E3779B97F4A7C15 * (256 * slot + unit + 1))
 *   keep = (r >> 40) < T,   T = llrint((1 - p) * 2^24)
 *
 * layer: 0 after mlp.1 (128 units), 1 after mlp.4 (64 units); slot: the scene's position in the mini-batch (not its
 * memory row); unit: the feature; step: the caller's count of training steps.  The mask is a function of these five
 * numbers and p alone: it does not depend on how scenes are dealt to workgroups.  A kept unit is multiplied by
 * 1 / (1 - p), a dropped one by 0 -- a multiplication in both passes, after the ReLU's own select, so NaN and Inf travel
 * as through nn.Dropout.  p arrives as float32 and is applied as the decimal that was written (0.1f means 0.1, as
 * mcn_adam_step takes its hyper-parameters): T is 8388608 for 0.5, 15099494 for 0.1f, 1677722 for 0.9f, 16777216 for 0
 * (every unit kept, multiplied by exactly 1).
 * r >> 40 for (seed, step, layer, slot, unit): (0,0,0,0,0) 10946269; (0,0,1,0,0) 4634430; (0,1,0,0,0) 15607633;
 * (1,0,0,0,0) 6177195; (12345,7,1,99,127) 13549691; (2^64-1, 2^40, 1, 3, 63) 822369.
 *
 * mcn_dropout_mask -- the mask of one layer of one step on the HOST (no GPU involved): keep[b * width + u] = 1 where unit
 * u of slot b is kept, else 0.  MCN_EINVAL: keep NULL, B < 1, width outside 1 .. 256, layer outside 0 .. 1, p not in [0, 1).
 */
int mcn_dropout_mask(uint64_t seed, uint64_t step, int32_t layer, int32_t B, int32_t width, float p,
                     uint8_t *keep /* host, [B][width] */);

/*
 * The network is MlpWorld(N): 4N -> 128 -> 64 -> 12 -> 2N, ReLU after the first three layers, dropout after the first two,
 * tanh on the output.  Parameters, gradient and the two Adam moments are each ONE flat float32 device buffer in
 * state_dict order -- mlp.0.weight, mlp.0.bias, mlp.3.*, mlp.6.*, mlp.8.* -- every weight row-major [out][in] as torch
 * stores it.
 */
int64_t mcn_mlp_world_train_param_count(int32_t N);            /* 538 N + 9164 (N = 5: 11854); 0 outside 1 .. MCN_MAX_HUMANS */
int64_t mcn_mlp_world_train_workspace_bytes(int32_t B, int32_t N);   /* 0 for arguments the step refuses */

/*
 * mcn_mlp_world_loss_grad -- loss = mean((model(cur[rows]) - nxt[rows])^2) over the B 2N outputs of a mini-batch of B
 * scenes of N pedestrians.  With grad it is the TRAIN-mode pass -- dropout with probability drop_p and the masks defined
 * above for (seed, step), slot b being scene b of the batch -- and grad receives the gradient by every parameter, with
 * the semantics of torch autograd (ReLU passes gradient where its output is > 0).  grad == NULL is the EVAL-mode forward
 * pass, which is what validation runs: no dropout, drop_p / seed / step are ignored (drop_p is still validated), and
 * nothing but `loss` is written for the caller.  With drop_p == 0 both modes give the same loss bits.
 * cur, nxt, rows, workspace (mcn_mlp_world_train_workspace_bytes(B, N) device bytes, 8-byte aligned), loss and the two
 * launches on `stream` are those of mcn_attn_world_loss_grad: the kernel TRUSTS the row indices, there are no atomics and
 * the same inputs give the same bits.  The forward pass, tanh, d loss / d z = d loss / d out (1 - out^2) and the sums over
 * the batch run in float64, the backward pass in float32; mlp.8.bias comes from float64 sums.  One workgroup takes 8
 * scenes, every activation in LDS.
 * MCN_EINVAL before any launch: a NULL params / cur / nxt / workspace / loss, B < 1, N outside 1 .. MCN_MAX_HUMANS,
 * drop_p outside [0, 1) or not finite.
 */
int mcn_mlp_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int32_t B, int32_t N,
                            float drop_p, uint64_t seed, uint64_t step, void *workspace,
                            float *grad /* or NULL */, float *loss, void *stream);

/*
 * Dispatch overrides (host, process-wide, not stream-ordered; for tests and tuning).  Every env-step arithmetic
 * exists in several kernel decompositions with bit-identical results; by default the entry points pick one from
 * the batch shape.  -1 = automatic.  The MCN_FORCE_GENERIC / MCN_QUAD_MAX_ENVS / MCN_QUAD_SPLIT /
 * MCN_ROLLOUT_FUSED / MCN_ROLLOUT_SPLIT / MCN_PAIR_STREAM / MCN_STEP_BLOCK / MCN_LP3_DEFER / MCN_SARL_X3 environment variables give the initial values and are read once, at
 * the first launch; no entry point calls getenv after that.
 */
typedef struct mcn_tuning {
    int32_t force_generic;   /* 1: run-time-N lane-per-human kernel even where a compile-time-N form exists */
    int32_t quad_max_envs;   /* mcn_env_step: lanes-per-neighbour ("quad") kernel up to this batch size (0 = never) */
    int32_t quad_split;      /* quad kernel: ORCA and float64 pairwise work on two cooperating wavefronts (0/1) */
    int32_t rollout_fused;   /* mcn_env_rollout: one T-step launch (1) or T single-step launches (0) */
    int32_t rollout_split;   /* fused rollout: 0 one wavefront per env group, 1 two cooperating ones, 2 workgroups of 8 envs on
                              * four wavefronts (5 humans, invisible robot; other shapes take form 1) */
    int32_t step_block;      /* lane-per-human step kernels: workgroup of 64 or 256 lanes (-1: 64 up to 4096 wavefronts, 256 above) */
    int32_t diag_noop;       /* DIAGNOSTIC build only (make stamp): env kernels return at entry; MCN_EINVAL otherwise */
    int32_t pair_stream;     /* given-velocity step: streaming kernel (env_pair.hip) 1 wherever it applies / 0 never;
                              * 2 / 3: wherever it applies, with non-temporal per-human streams forced on / off */
    int32_t lp3_defer;       /* lane-per-human ORCA kernels with mcn_env_out.lp3_queue set: park the 3-D LPs for a second,
                              * dense launch (1) or solve them in the step kernel (0); -1: defer from 8 ORCA neighbours and 16 384 wavefronts */
    int32_t sarl_x3;         /* SARL look-ahead with mcn_sarl_net.x3 set: bf16x3 layers (1 / -1) or the float32 MFMA layers (0).
                              * Input range of the bf16x3 layers: features and activations below 2^128 - 2^119 (3.3962e38)
                              * in size.  From there on a float32 rounds to an infinite first bfloat16 piece and has no
                              * three-piece split: what that variant returns for such an env is not specified, while the
                              * float32 MFMA layers, like the reference, carry every finite float32.  (+-inf and NaN
                              * features give NaN in both variants, as in the reference.) */
} mcn_tuning;

/* NULL restores the initial values.  Returns MCN_EINVAL for out-of-range fields.  The settings are one process-wide
 * struct; every launch takes a consistent snapshot of it under a lock, so mcn_set_tuning may be called while other
 * threads launch (they see the old or the new settings, never a mixture). */
int mcn_set_tuning(const mcn_tuning *t);
int mcn_get_tuning(mcn_tuning *t);

/* Library self-description (host). */
const char *mcn_version(void);

/*
 * ABI guard.  MCN_ABI_VERSION changes whenever a struct of this header changes size or layout or an entry point
 * changes its signature (0.3 grew mcn_tuning by lp3_defer and mcn_env_out by lp3_queue: ABI 4; 0.4 grew mcn_sarl_net by
 * x3: ABI 5; an entry point that is only ADDED, like mcn_sgan_predict or
 * mcn_env_step_sf, leaves it as it is).  A caller built against
 * another header must not pass structs to this library: compare mcn_abi_version() with the MCN_ABI_VERSION it was
 * compiled with, and (bindings without the header: ctypes, cgo) mcn_sizeof() with the size of its own struct mirrors.
 */
#define MCN_ABI_VERSION 5
int32_t mcn_abi_version(void);
enum { MCN_SIZEOF_ENV_CFG = 0, MCN_SIZEOF_ENV_STATE = 1, MCN_SIZEOF_ENV_OUT = 2, MCN_SIZEOF_ROLLOUT = 3,
       MCN_SIZEOF_TUNING = 4, MCN_SIZEOF_STEP_REC = 5, MCN_SIZEOF_ROLL_REC = 6, MCN_SIZEOF_SARL_NET = 7,
       MCN_SIZEOF_SGAN_NET = 8, MCN_SIZEOF_SCENARIO_CFG = 9, MCN_SIZEOF_MLP_WORLD_NET = 10, MCN_SIZEOF_ATTN_WORLD_NET = 11,
       MCN_SIZEOF_SARL_X3 = 12, MCN_SIZEOF_LSTM_RL_NET = 13, MCN_SIZEOF_CADRL_NET = 14 };
int64_t mcn_sizeof(int32_t which);                 /* sizeof the struct named by MCN_SIZEOF_*; -1 for an unknown id */

/*
 * Diagnostic: the kernel family ("env_step_quad_kernel", "env_rollout_quad_kernel", "env_step_loop_kernel",
 * "env_pair_kernel", "env_step_kernel", "env_step_loop_sf_kernel") that the calling thread's latest mcn_env_step /
 * mcn_env_rollout call (or social-force twin) dispatched to; "" before the first call.  bench.py attributes profiles to the kernel that really ran with it.
 */
const char *mcn_last_dispatch(void);

/*
 * Diagnostic: which form of the fused rollout kernel the calling thread's latest mcn_env_rollout call launched, noted
 * at the launch itself: 0 one wavefront per env group, 1 two cooperating wavefronts, 2 workgroups of 8 envs on four
 * wavefronts (env_rollout_wg4_kernel).  -1 when that call did not take the fused quad path, and before the first call.
 * mcn_tuning.rollout_split = 2 on a shape the four-wavefront form is not built for reports 1: what ran.
 */
int32_t mcn_last_rollout_form(void);

#ifdef __cplusplus
}
#endif
#endif /* MCN_H_ */
