// env_dispatch.hpp -- which env kernel runs for a problem: a pure function of (cfg, E, N, T, which optional buffers
// exist, tuning).  Plain inline host C++ over include/mcn.h and the argument block, so that a stand-alone program can
// include it with the host compiler (tests/env_dispatch_probe.cpp).  mcn_api.hip validates, takes one snapshot of the
// tuning, plans here and hands each launcher (launch.hpp) its part of the plan; the launchers only pick the
// instantiation, size the grid and launch.  Every measured threshold of the env kernels lives in this file.
#pragma once
#include <stdint.h>
#include "../../include/mcn.h"
#include "env_step_params.hpp"

namespace mcn {

// what mcn_last_dispatch() names (family_name)
enum KernelFamily {
    kStepQuad,          // env_step_quad.hip
    kStepPair,          // env_pair.hip
    kStepLane,          // env_step.hip: env_step_kernel, one lane per human
    kRolloutQuad,       // env_rollout_quad.hip / env_rollout_wg4.hip
    kStepLoop,          // env_step.hip: env_step_loop_kernel
    kStepLoopSf,        // env_step.hip: env_step_loop_sf_kernel
    kStepLoopOrca,      // env_step.hip: env_step_loop_orca_kernel (mcn_env_rollout_orca: its one path)
    kStepLoopOrcaSf,    // env_step.hip: env_step_loop_orca_sf_kernel (mcn_env_rollout_orca_sf: its one path)
};

inline const char *family_name(KernelFamily f)
{
    switch (f) {
        case kStepQuad:     return "env_step_quad_kernel";
        case kStepPair:     return "env_pair_kernel";
        case kStepLane:     return "env_step_kernel";
        case kRolloutQuad:  return "env_rollout_quad_kernel";
        case kStepLoop:     return "env_step_loop_kernel";
        case kStepLoopSf:   return "env_step_loop_sf_kernel";
        case kStepLoopOrca: return "env_step_loop_orca_kernel";
        case kStepLoopOrcaSf: return "env_step_loop_orca_sf_kernel";
    }
    return "";
}

// One mcn_env_step / mcn_env_step_sf launch.  Only the fields of the chosen family mean anything; the others are 0.
struct StepPlan {
    KernelFamily family;    // kStepQuad, kStepPair or kStepLane
    bool quad_split;        // kStepQuad: ORCA and pairwise work on two cooperating wavefronts
    int block;              // kStepLane: 64 / 256 lanes per workgroup
    bool static_n;          // kStepLane: compile-time-N body (else the run-time-N one)
    bool lp3_defer;         // kStepLane: park the 3-D LPs (lp3_queue.hpp) and finish them with env_lp3_kernel
    bool pair_nontemporal;  // kStepPair: non-temporal per-human streams
};

// One mcn_env_rollout / mcn_env_rollout_sf call: kRolloutQuad (with its form), kStepLoop or kStepLoopSf in one launch,
// or a single-step family, which means T launches of `step`.
struct RolloutPlan {
    KernelFamily family;
    int form;               // kRolloutQuad: 0 one wavefront per env group, 1 two, 2 four per 8 envs; -1 otherwise
    StepPlan step;          // the single steps, where they are used
};

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// candidate ORCA neighbours per human
inline int step_candidates(const StepParams &p) { return p.N - 1 + (p.cfg.robot_visible ? 1 : 0); }

// wavefronts of the lane-per-human kernels (G = 64 / N envs each)
inline long lane_wavefronts(const StepParams &p) { return ceil_div(p.E, 64 / p.N); }

// The quad layout (env_step_quad.hip, env_rollout_quad.hip): ORCA humans with at most 4 candidate neighbours each and
// no cut of the neighbour list.  Every such (N, visible) is built: N = 1..4 either way, N = 5 with an invisible robot.
inline bool quad_shape_applies(const StepParams &p)
{
    return p.cfg.human_policy == MCN_HUMANS_ORCA && p.cfg.orca_max_neighbors >= 4 && p.N >= 1 && step_candidates(p) <= 4;
}

// The streaming given-velocity kernel (env_pair.hip) handles: compile-time N in {5, 10}, holonomic robot, update = 1,
// no human-human count, no first-arrival bookkeeping, no human_act export, a discount table of at most kPairDiscMax
// entries; everything else stays on env_step_kernel.
inline bool pair_applies(const StepParams &p, const mcn_tuning &tu)
{
    if (p.cfg.human_policy != MCN_HUMANS_GIVEN || !p.update || p.cfg.count_hh || p.cfg.robot_kinematics != MCN_KIN_HOLONOMIC)
        return false;
    if ((p.cfg.track_human_times && p.st.human_times) || p.out.human_act) return false;
    if (p.has_roll && p.roll.state && p.roll.disc_len > kPairDiscMax) return false;
    if (tu.force_generic > 0) return false;
    return p.N == 5 || p.N == 10;
}

// Small batches run one wavefront per workgroup so that the grid covers as many CUs as possible (crowds of 9-10: the
// one-wavefront workgroups with the cooperative 3-D LP stay ahead longer -- 10 humans, 32 768 envs 63.6 vs 67.1 us,
// 65 536 envs 105 vs 110, 2^18 envs 391 vs 307; 7 humans cross at ~24 k envs).  mcn_tuning.step_block overrides.
inline bool one_wave_batch(const mcn_tuning &tu, long waves_total, int nc)
{
    return tu.step_block > 0 ? tu.step_block == 64 : waves_total <= (nc >= 8 ? 12288 : 4096);
}

// mcn_env_rollout for 6-10 ORCA humans (and 5 with a visible robot) in a latency-bound batch: one env_step_loop_kernel
// launch instead of T step launches.
inline bool step_loop_applies(const StepParams &p, const mcn_tuning &tu)
{
    // (5 humans + a visible robot = 5 neighbours: one more than the quad-parallel rollout kernel takes)
    const bool five_vis = p.N == 5 && p.cfg.robot_visible;
    if (p.cfg.human_policy != MCN_HUMANS_ORCA || tu.force_generic > 0 || !p.update || ((p.N < 6 || p.N > 10) && !five_vis)) return false;
    if (tu.lp3_defer > 0) return false;                                // forced deferral: two kernels per step
    const long waves_total = lane_wavefronts(p);
    if (!one_wave_batch(tu, waves_total, step_candidates(p))) return false;      // the single step's own rule
    // The looped kernel holds 234-282 VGPRs (one wavefront per SIMD) against the step kernel's 160 (three): it wins while
    // the batch leaves SIMDs idle anyway and loses once wavefronts queue up -- 10 humans: 4096 envs 28.9 -> 14.9 us per
    // step, 16 384 envs (2731 wavefronts) 43.0 -> 41.3, 32 768 envs (5462) 64.2 -> 80.7.
    return tu.step_block == 64 || waves_total <= 3072;
}

// mcn_env_rollout_sf in a latency-bound batch (the single step's own one-wavefront rule): one env_step_loop_sf_kernel
// launch instead of T step launches.
inline bool step_loop_sf_applies(const StepParams &p, const mcn_tuning &tu)
{
    if (p.cfg.human_policy != MCN_HUMANS_SOCIALFORCE || !p.update) return false;
    return one_wave_batch(tu, lane_wavefronts(p), step_candidates(p));
}

inline StepPlan plan_env_step(const StepParams &p, const mcn_tuning &tu)
{
    StepPlan s = {};
    const bool force_generic = tu.force_generic > 0;
    // Small batches are latency-bound: use the quad-parallel kernel (env_step_quad.hip) while its 4x wider
    // grid still fits the chip about twice over (measured cross-over on MI355X: ~2800 wavefronts, i.e.
    // E <= 8192 at 5 humans); above that the lane-per-human kernel wins on throughput.  Inside the quad
    // kernel, ORCA and the float64 pairwise work go to two cooperating wavefronts only while BOTH still get a
    // SIMD of their own (grid <= 512 workgroups).  mcn_set_tuning overrides (tests, tuning).
    const int envs_per_wave = 64 / (4 * p.N);
    const long quad_waves = envs_per_wave > 0 ? ceil_div(p.E, envs_per_wave) : (1L << 40);
    const int quad_max_envs = tu.quad_max_envs >= 0 ? tu.quad_max_envs : (quad_waves <= 2800 ? p.E : 0);
    // <= 4 ORCA neighbours per human: quad-parallel kernel (env_step_quad.hip); force_generic does not stop it
    if (quad_max_envs > 0 && p.E <= quad_max_envs && quad_shape_applies(p)) {
        s.family = kStepQuad;
        // two cooperating wavefronts per env group while the doubled grid still finds idle issue slots; re-measured in round 4
        // (5 humans, us per step without / with: 1024 envs 5.87 / 5.37, 2048 6.28 / 6.10, 4096 = 1366 wavefronts 7.20 / 6.95,
        //  5120 7.60 / 8.01, 6144 7.71 / 8.68): up to ~1400 wavefronts (round 3's rule stopped at 512)
        s.quad_split = tu.quad_split >= 0 ? tu.quad_split != 0 : quad_waves <= 1400;
        return s;
    }
    const long waves_total = lane_wavefronts(p);
    const int nc = step_candidates(p);
    // given velocities, large batch: the streaming form (env_pair.hip); mcn_tuning.pair_stream overrides
    if ((tu.pair_stream > 0 || (tu.pair_stream < 0 && waves_total > 4096)) && pair_applies(p, tu)) {
        s.family = kStepPair;
        // non-temporal per-human streams once one step's footprint (~(15 + 11 N) x 8 + 70 B per env) is well past the
        // 256 MB memory-side cache (measured cross-over, 5 humans: 2^18 envs = 165 MB 27.9 vs 32 us without / with,
        // 2^19 = 330 MB equal, 2^20 = 660 MB 126-142 vs 108-109); mcn_tuning.pair_stream 2 / 3 force it on / off
        const double footprint = (double)p.E * ((15 + 11 * p.N) * 8 + 70);
        s.pair_nontemporal = tu.pair_stream == 2 || (tu.pair_stream != 3 && footprint > 400e6);
        return s;
    }
    s.family = kStepLane;
    s.block = one_wave_batch(tu, waves_total, nc) ? 64 : 256;
    // register-resident ORCA specialisations for the crowd sizes the reference trains and tests on
    // (human_num 5 / 10 in the configs, 5,7,9 in test_mul_env.py:31-33, 1..5 in the 'mixed' rule); social force:
    // compile-time N for the reference's crowd sizes: the loop over the others is unrolled (4 - 9 % per launch)
    s.static_n = !force_generic && ((p.cfg.human_policy == MCN_HUMANS_ORCA && p.N >= 1 && p.N <= 10) ||
                                    (p.cfg.human_policy == MCN_HUMANS_SOCIALFORCE && (p.N == 5 || p.N == 10)));
    // The compile-time-N ORCA kernels can park their 3-D LPs when the caller gave them a queue.  Measured on MI355X
    // (round 3, circle crossing with pool restarts; step kernel alone / + the finish kernel vs solving in place):
    // 10 humans 2^18 envs 344 -> 249 + 40 us, 32 768 envs 65 -> 65, 4096 envs 27 -> 31; 7 humans 2^18 envs 110 -> 122;
    // 5 humans 2^20 envs 207 -> 205 + 20.  Only 0.9 / 1.8 / 3.7 % of the humans need the 3-D LP at 5 / 7 / 10 humans
    // and the in-place code already skips every block no lane of the wavefront needs, so deferral pays only for the
    // largest crowds in throughput-bound batches: automatic from 8 neighbours and 16 384 wavefronts.
    s.lp3_defer = p.out.lp3_queue && p.cfg.human_policy == MCN_HUMANS_ORCA && !force_generic && p.N >= 2 && p.N <= 10 &&
                  nc >= 1 && nc <= kMaxLines && (tu.lp3_defer > 0 || (tu.lp3_defer < 0 && nc >= 8 && waves_total >= 16384));
    return s;
}

inline RolloutPlan plan_env_rollout(const StepParams &p, int T, const mcn_tuning &tu)
{
    RolloutPlan r = {};
    r.form = -1;
    if (p.cfg.human_policy == MCN_HUMANS_SOCIALFORCE) {
        // latency-bound batch: the one-wavefront step kernel run T times inside one launch (env_step.hip:
        // env_step_loop_sf_kernel); rollout_fused = 0 keeps the T launches
        if (tu.rollout_fused != 0 && T > 1 && step_loop_sf_applies(p, tu)) { r.family = kStepLoopSf; return r; }
        r.step = plan_env_step(p, tu);
        r.family = r.step.family;
        return r;
    }
    // One launch with the env state held in registers for all T steps where the quad layout applies and beats T
    // launches of the throughput kernel: measured cross-over on MI355X at ~45 k envs of 5 humans (19.2 vs 18.6 us per
    // step at 49 152 envs, 13.9 vs 15.3 at 32 768), i.e. ~14 k env groups; below that the fused launch wins by up to
    // 2.7x.  Two cooperating wavefronts per env group while the doubled grid still finds idle issue slots (measured:
    // wins up to 1536 groups = 4608 envs, loses from 1707).  The four-wavefront form (rollout_split = 2: workgroups of 8
    // envs; built for 5 humans and an invisible robot) costs what its fullest CU holds and is taken only where it was
    // measured to win (profiles/r12_rollout_wg4.txt, T = 1000 and T = 20, us per step at T = 1000 against the better of
    // the other two forms):
    //   holonomic robot (95 VGPRs, up to 4 workgroups per CU resident: 1.86 / 2.32 / 2.78 us at 2 / 3 / 4 per CU):
    //     128 .. 512 workgroups (1024 envs 1.49 against 1.72, 4096 envs 1.86 against 2.10) and 768 .. 1024 (6144 / 8192
    //     envs: 2.32 / 2.78 against 3.29 / 3.33).  Not below: at 64 and 256 envs no form shares a CU and the two-wavefront
    //     form's shorter chain wins (1.43 against 1.47 / 1.51).  Not in between: at 4608 envs = 576 workgroups a quarter
    //     of the CUs hold three and it loses (2.30 against 2.13).
    //   unicycle robot (129 VGPRs: 3 wavefronts per SIMD, so the fourth workgroup of a CU waits; the other forms' 153 /
    //     168 VGPRs cost them more): 8 .. 1024 workgroups, every size measured from 64 envs (1.96 against 2.11) over
    //     4096 (2.32 against 3.37) and 4608 (3.06 against 3.39) to 8192 (4.18 against 5.45).
    // mcn_set_tuning (rollout_fused / rollout_split) overrides (tests, tuning).
    const int envs_per_wave = 64 / (4 * p.N) > 0 ? 64 / (4 * p.N) : 1;
    const long waves = ceil_div(p.E, envs_per_wave);
    const bool fused = tu.rollout_fused >= 0 ? tu.rollout_fused != 0 : waves <= 14000;
    if (fused && !(tu.force_generic > 0) && quad_shape_applies(p) && p.update) {
        const bool wg4_built = p.N == 5 && !p.cfg.robot_visible;      // env_rollout_wg4.hip
        const long wg4 = ceil_div(p.E, 8);
        const bool wg4_wins = wg4_built &&
                              (p.cfg.robot_kinematics == MCN_KIN_UNICYCLE ? wg4 >= 8 && wg4 <= 1024
                                                                         : (wg4 >= 128 && wg4 <= 512) || (wg4 >= 768 && wg4 <= 1024));
        const int split = tu.rollout_split >= 0 ? tu.rollout_split : wg4_wins ? 2 : (waves <= 1536 ? 1 : 0);
        r.family = kRolloutQuad;
        // a forced form 2 on a shape without the four-wavefront kernel keeps the two-wavefront form
        r.form = split == 2 && wg4_built ? 2 : (split ? 1 : 0);
        return r;
    }
    // 6-10 ORCA humans, latency-bound batch: the one-wavefront step kernel run T times inside one launch
    // (env_step.hip: env_step_loop_kernel); rollout_fused = 0 keeps the T launches
    if (tu.rollout_fused != 0 && T > 1 && step_loop_applies(p, tu)) { r.family = kStepLoop; return r; }
    r.step = plan_env_step(p, tu);
    r.family = r.step.family;
    return r;
}

}  // namespace mcn
