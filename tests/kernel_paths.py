"""The kernel paths the edge, ladder and accounting batteries run over: every decomposition of mcn_env_step, every path
of mcn_env_rollout, what each must reach, and the four-wavefront form's battery under rolled env orders.  Tests of the
oracle alone (no GPU) read the same tables."""
import functools

import numpy as np

from tests import edge_states as ES
from tests import helpers as H
from tests import ladder_states as LS
from tests.rollout_harness import assert_same_bytes, launch, need_gpu, snapshot
from tests.rollout_ref import sf_velocities      # tests/social_force_ref.py on an oracle state

STEP_KERNELS = ["auto", "lane-per-human", "lane-per-human-256", "deferred-lp3", "deferred-lp3-256", "run-time-N",
                "run-time-N-256", "quad", "quad-split"]
# what the quad kernels' inputs must reach (at most 4 neighbours and maxNeighbors >= 4: no cut of the neighbour list)
QUAD_EVENTS = ("disc_zero_lp2", "disc_zero_lp3", "dist_tie", "nonfinite_line", "nonfinite_line_in_lp3",
               "w_zero_collision", "parallel_lp1", "parallel_same_lp3", "parallel_opposite_lp3", "range_edge",
               "leg_det_zero", "pref_on_disc", "outside_fast_range")
STEP_EVENTS = ("swept_touch", "swept_point", "swept_u_zero", "swept_u_one", "dmin_tie", "danger_edge", "reach_edge",
               "reach_band", "collision_and_reach", "timeout_and_collision", "timeout_edge", "timeout_below",
               "hh_touch", "hh_band6", "hh_band3", "human_time_edge")
UNICYCLE_EVENTS = STEP_EVENTS + ("theta_zero_rem", "theta_neg_rem")


def select_step_kernel(kernel, tuning):
    """As tests/test_env_step_gpu.py::test_step_matches_oracle_bitexact pins each decomposition."""
    if kernel.startswith("lane-per-human"):
        tuning(quad_max_envs=0, lp3_defer=0)
    elif kernel.startswith("deferred-lp3"):
        tuning(quad_max_envs=0, lp3_defer=1)
    elif kernel.startswith("run-time-N"):
        tuning(quad_max_envs=0, force_generic=1)
    elif kernel.startswith("quad"):
        tuning(quad_max_envs=1 << 30, quad_split=1 if kernel == "quad-split" else 0)
    if kernel.endswith("-256"):
        tuning(step_block=256)


def edge_configs(Ns, quad, variants=ES.ORCA_VARIANTS):
    """(N, visible, variant) triples; the quad kernels take at most 4 candidate neighbours and 4 line slots."""
    for N in Ns:
        for visible in (False, True):
            if quad and N - 1 + visible > 4:
                continue
            for variant in variants:
                if quad and ES.orca_cfg(variant)["max_neighbors"] < 4:
                    continue
                yield N, visible, variant


def ladder_configs(Ns, quad):
    """(N, visible, dd, count_hh); the quad kernels take at most 4 candidate neighbours."""
    for N in Ns:
        for visible in (False, True):
            if quad and N - 1 + visible > 4:
                continue
            for dd in LS.DISCOMFORT:
                yield N, visible, dd, (N + visible) % 2 == 0 or dd == 0.25


ROLLOUT_PATHS = {
    # name: (human counts, quad layout, tuning)
    "quad-rollout": (range(1, 6), True, dict(rollout_fused=1, rollout_split=0)),
    "quad-rollout-split": (range(1, 6), True, dict(rollout_fused=1, rollout_split=1)),
    "step-loop": (range(6, 11), False, dict(rollout_fused=1, lp3_defer=0)),
    "lp3-defer": (range(2, 11), False, dict(rollout_fused=1, lp3_defer=1)),
    "unfused": (range(1, 11), False, dict(rollout_fused=0)),
    # the four-wavefront form (env_rollout_wg4.hip): built for 5 humans and an invisible robot only
    "quad-rollout-wg4": ((5,), True, dict(rollout_fused=1, rollout_split=2)),
}
WG4_SLOTS = 8                     # envs per workgroup of the four-wavefront form
WG4_STRADDLERS = (3, 6)           # quad q = 5 env + human: the envs in these slots have quads in two ORCA wavefronts
# the four-wavefront form double-buffers velocities by step parity, from 0 in every launch: an odd launch, a one-step
# launch and an even one
WG4_EDGE_CUTS = (0, 9, 10, 24)
_SLOT_MAJOR = ("roll_fin_return", "roll_fin_time", "roll_fin_info")      # [fin_slots, E]; everything else is [E, ...]


def forced_form(path):
    """The rollout form a quad path forces (mcn_tuning.rollout_split), None for the other paths."""
    Ns, quad, tu = ROLLOUT_PATHS[path]
    return tu["rollout_split"] if quad else None


def _roll_snapshot(snap, perm):
    return {k: np.take(v, perm, axis=1 if k in _SLOT_MAJOR else 0) for k, v in snap.items()}


def rolled_wg4_battery(build, take, st, acts, names, cuts, check_first, check_last, what, odd_roll=3):
    """The four-wavefront form on one batch under np.roll of the env order by 0 .. 7, so that every env meets every slot
    of an 8-env workgroup (each of the three ORCA wavefronts sees other envs, and the envs in slots 3 and 6 straddle
    two of them); the rare events sit at fixed offsets of their 16-env blocks and would otherwise only ever meet the
    same slots.  Actions and first_cases roll with the envs.

      every roll              a one-step launch; check_first(env, perm, rolled names, what) holds it to the oracle
      roll 0 and odd_roll     the whole sequence in the launches `cuts`, without and with a scenario pool: every byte of
                              the equally rolled result of single mcn_env_step calls (run once, unrolled), and without
                              a pool check_last(...) against the oracle

    build() gives a configured env, take(st, perm) the envs of an oracle state in another order."""
    torch = need_gpu()
    from modelcrowdnav_amd.envs import scenarios as S
    E, T = st.E, len(acts)
    assert cuts[0] == 0 and cuts[-1] == T
    cases = np.arange(E) % 16
    ident = np.arange(E)

    def start(perm, with_pool):
        env = build()
        H.upload(env, take(st, perm))
        if with_pool:
            pool = S.scenario_pool(env.spec(), "test", range(16), st.N, "circle_crossing")
            env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=cases[perm], fin_slots=2)
        return env, torch.from_numpy(np.ascontiguousarray(acts[:, perm])).to(env.device)

    singles = {}
    for with_pool in (False, True):
        env, a = start(ident, with_pool)
        for t in range(T):
            env.step(a[t])
        torch.cuda.synchronize()
        singles[with_pool] = snapshot(env)
    assert set(_SLOT_MAJOR) <= set(singles[True])
    seen = [set() for _ in range(E)]
    for r in range(WG4_SLOTS):
        perm = np.roll(ident, r)
        rolled = [names[i] for i in perm]
        for pos, i in enumerate(perm):
            seen[i].add(pos % WG4_SLOTS)
        env, a = start(perm, False)
        launch(env, a[:1], 2)
        torch.cuda.synchronize()
        check_first(env, perm, rolled, "%s roll %d first step" % (what, r))
        if r not in (0, odd_roll):
            continue
        for with_pool in (False, True):
            env, a = start(perm, with_pool)
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                launch(env, a[lo:hi], 2)
            torch.cuda.synchronize()
            assert_same_bytes(snapshot(env), _roll_snapshot(singles[with_pool], perm), (what, "roll", r, with_pool))
            if not with_pool:
                check_last(env, perm, rolled, "%s roll %d" % (what, r))
    # over the rolls every env but the last few (which wrap to the front) sat in every slot, and an env of every block
    # sat in the two straddling ones
    assert all(s == set(range(WG4_SLOTS)) for s in seen[:E - WG4_SLOTS + 1])
    for block in sorted(set(names)):
        slots = set().union(*(seen[i] for i in range(E) if names[i] == block))
        assert set(WG4_STRADDLERS) <= slots, (what, block, sorted(slots))


# ---------------------------------------------------------------------------------------------------------------------
# social-force humans (mcn_env_step_sf / mcn_env_rollout_sf)
SF_DEFAULT = (4.0, 0.2, 2.0)      # (strength A, range B, relaxation_rate k) as shipped
# A = 0: every m = 0 * exp(..) is exactly 0, so exp -- the only inexact operation -- is multiplied away and the
# restatement is bit-exact; k = 4 with dt = 0.25 gives a human at rest w = 0 + 4 * e * 0.25 = e exactly
SF_INERT = (0.0, 0.2, 4.0)
SF_COMPILED_NS = (5, 10)          # crowd sizes with compile-time-N step kernels besides the run-time-N ones
SF_GENERIC_NS = (1, 2, 3, 7, 13, 32)
SF_TOL = 8 * 2.0 ** -52           # of the restatement's magnitude M (tests/test_social_force_gpu.py, part 1)


def sf_step_forms(N):
    """(step_block, force_generic) of every env_step_kernel<.., MCN_HUMANS_SOCIALFORCE, ..> form that takes N humans."""
    return [(b, g) for g in ((0, 1) if N in SF_COMPILED_NS else (0,)) for b in (64, 256)]


@functools.lru_cache(maxsize=None)
def sf_ladder_reference(N, visible, dd, params):
    """The restatement's velocities on LS.ladder_batch(N, visible, dd), computed once per process; read-only."""
    st = LS.ladder_batch(N, visible, dd)[0]
    want, mag = sf_velocities(st, params, visible)
    want.setflags(write=False); mag.setflags(write=False)
    return want, mag


def sf_oracle_step(cfg, st, ax, ay, params, visible, update=True):
    """One host step of social-force humans: the restatement's velocities handed to the oracle's given-velocity step
    (cfg.human_policy must be HUMANS_GIVEN).  Returns (the oracle's outputs, the velocities, their magnitudes)."""
    from oracle import cport
    want, mag = sf_velocities(st, params, visible, cfg.time_step)
    return cport.env_step(cfg, st, ax, ay, update=update, given_v=want), want, mag
