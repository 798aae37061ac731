"""The lean take steps of the four-wavefront rollout form (env_rollout_wg4_kernel, rollout_split = 2; quad_common.hpp:
Path::lean_take, quad_take_plan.hpp: take_step_lean), bytes against single steps and against the oracle.

The form's 2-D LP decides each of its four compare-and-take steps from min(fail, code_i) beside the step's test; the
single-step kernel keeps the guarded steps, so a byte that differs between the two is a decision that differs.  What a
scene has to hold for that to show: solves that end at the clipped preferred velocity (no take), on the first line that
velocity violates (one take), somewhere else (several takes: a later step reads a running point an earlier one moved) and
in the 3-D LP (a violated line's 1-D LP is infeasible: the step that must stop every later take).  Each battery counts
the four on the host, from the oracle's states and its own half-planes (cport.orca_lines), BEFORE anything is launched,
and asserts at least one of each per robot kinematics.  The classification is for counting only: it uses float32 for the
tests as the solvers do and a float64 distance to decide whether a result lies on a line.

Batteries: a pool whose odd cases start packed (tests.rollout_harness.packed_pool) and the plain circle-crossing pool, both
robot kinematics, E in {1, 8, 9, 19} (one env, a full workgroup, one env behind a full workgroup, three behind two), up
to 40 steps, restarts from the pool inside the launch, and on a short sequence every cut into two launches and one-step
launches.  Full state, step record, Explorer record and finished-episode arrays after EVERY launch against single
mcn_env_step calls at that step; the final state also against the oracle stepping the same envs with the same restarts.
Every forced launch asserts mcn_last_rollout_form() == 2 (rollout_harness.launch).

The NaN, tie and zero half-planes of this form are the ORCA-edge and ladder batteries' (tests/test_rollout_wg4_gpu.py):
they run on this path unchanged and are not copied here."""
import functools

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests import lp2_gate_states as G
from tests.rollout_harness import every_cut, launches_against, oracle_rollout, packed_pool, random_actions, single_steps

N = 5
P, FIRST, STRIDE = 16, 7, 3
KINEMATICS = ["holonomic", "unicycle"]
CLASSES = ("no_take", "one_take", "several_takes", "lp3")
ON_LINE = 1e-5                   # float64 distance of a float32 result from a line it was projected on: ~1e-7


def _pool(kind, spec):
    from modelcrowdnav_amd.envs import scenarios as S
    if kind == "packed":
        return packed_pool(spec, P, N)
    return S.scenario_pool(spec, "test", range(P), N, "circle_crossing").copy()


def _actions(kinematics, T, E):
    """random robot actions; a holonomic robot goes up the middle, into the packed crowds and through the open ones, so
    that envs end inside the launch"""
    if kinematics == "holonomic":
        rng = np.random.RandomState(29)
        return np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
    return random_actions(kinematics, T, E, 29)


def count_classes(spec, cfg, pool, E, acts):
    """The oracle stepping E envs through acts with the in-kernel restarts (as rollout_harness.oracle_rollout, whose final
    state it must reproduce), classifying every human-step before it is taken.  Returns ({class: count}, restarts)."""
    from modelcrowdnav_amd.envs import scenarios as S
    ids = np.arange(E)
    st = cport.EnvState(E, N)

    def load(rows, cases):
        sc = pool[cases]
        st.hpx[rows], st.hpy[rows], st.hgx[rows], st.hgy[rows] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
        st.hvx[rows], st.hvy[rows] = sc[..., S.VX], sc[..., S.VY]
        st.hr[rows], st.hvpref[rows] = sc[..., S.RAD], sc[..., S.VPREF]
        st.human_times[rows] = 0
        rr = spec.robot_row()
        st.rpx[rows], st.rpy[rows], st.rgx[rows], st.rgy[rows] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
        st.rvx[rows], st.rvy[rows], st.rr[rows], st.gtime[rows] = 0.0, 0.0, rr[S.RAD], 0.0
        st.rtheta[rows] = rr[S.TH]                               # a unicycle robot starts, and restarts, at its start heading
    load(ids, ids % P)
    next_case = (ids + FIRST) % P
    counts, restarts = dict.fromkeys(CLASSES, 0), 0
    cport.lp3_entries(reset=True)
    for t in range(acts.shape[0]):
        before = [[(G.clipped_pref(cfg, st, e, i), G.human_lines(cfg, st, e, i)) for i in range(N)] for e in range(E)]
        ref = cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        for e in range(E):
            for i in range(N):
                v0, lines = before[e][i]
                got = ref["human_act"][e, i].astype(np.float32)
                if got.tobytes() == np.asarray(v0, np.float32).tobytes():
                    counts["no_take"] += 1
                    continue
                d = G.line_dets(lines, v0)
                first = np.nonzero(d > 0)[0]
                if len(first) == 0:
                    continue                                     # (moved without a violated line: not a class, not expected)
                ln = lines[first[0]].astype(np.float64)
                off = ln[2] * (ln[1] - float(got[1])) - ln[3] * (ln[0] - float(got[0]))
                counts["one_take" if abs(off) <= ON_LINE else "several_takes"] += 1
        d = np.nonzero(ref["done"])[0]
        if len(d):
            load(d, next_case[d])
            next_case[d] = (next_case[d] + STRIDE) % P
            restarts += len(d)
    counts["lp3"] = cport.lp3_entries()
    return counts, restarts, st


def _build(kind, kinematics, E):
    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        pool = _pool(kind, env.spec())
        ids = np.arange(E)
        env.load_scenarios(pool[ids % P])
        env.attach_rollout(gamma=0.9, pool=pool, case_stride=STRIDE, first_cases=(ids + FIRST) % P, fin_slots=2)
        return env
    return build


@functools.lru_cache(maxsize=None)
def _battery(kind, kinematics, E, T):
    """(actions, class counts, restarts, the oracle's final state), counted once per battery and before any launch"""
    probe = H.make_vec_env(E, N, kinematics=kinematics)
    spec, cfg = probe.spec(), H.oracle_cfg_for(probe)
    pool = _pool(kind, spec)
    acts = _actions(kinematics, T, E)
    counts, restarts, st = count_classes(spec, cfg, pool, E, acts)
    if kinematics == "holonomic":
        # (oracle_rollout carries no heading: a unicycle robot's replay is the one above alone)
        want, _, want_restarts, _, want_lp3 = oracle_rollout(spec, cfg, pool, np.arange(E), acts, FIRST, STRIDE)
        H.assert_state_equal(st, want, what="the counting replay against oracle_rollout")
        assert (restarts, counts["lp3"]) == (want_restarts.sum(), want_lp3)
    return acts, counts, restarts, st


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_every_class_of_take_sequence_occurs(kinematics):
    """The coverage the byte tests below rest on, per kinematics, over their batteries (host only): at least one
    human-step that takes nothing, one that takes one line, one that takes several and one 3-D LP entry; and envs that
    restart inside the launch."""
    total, restarts = dict.fromkeys(CLASSES, 0), 0
    for kind in ("packed", "plain"):
        for E in (1, 8, 9, 19):
            _, counts, r, _ = _battery(kind, kinematics, E, 40)
            print(kinematics, kind, "E=%d" % E, counts, "restarts", r)
            restarts += r
            for k in CLASSES:
                total[k] += counts[k]
    for k in CLASSES:
        assert total[k] >= 1, (kinematics, k, total)
    assert restarts >= 1, (kinematics, restarts)


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
@pytest.mark.parametrize("kind", ["packed", "plain"])
@pytest.mark.parametrize("E", [1, 8, 9, 19])
def test_lean_takes_leave_the_bytes_of_single_steps_and_the_oracle(E, kind, kinematics, tuning):
    """40 steps as one launch and as two (13 + 27): restarts fall inside both.  After every launch the bytes of the
    single-step run; after the last the oracle's state."""
    tuning(rollout_fused=1)
    T = 40
    acts, counts, restarts, want = _battery(kind, kinematics, E, T)
    assert counts["no_take"] >= 1                                # (the other classes: per kinematics, the test above)
    build = _build(kind, kinematics, E)
    env, snaps, _, done = single_steps(build, acts)
    assert done.sum() == restarts
    # a unicycle robot's pose goes through sin / cos, where the host's and the device's libraries differ in the last place:
    # against the oracle its envs compare in the humans (the robot is invisible to them), against single steps in everything
    fields = H.STATE_FIELDS if kinematics == "holonomic" else cport.EnvState.FIELDS_H + ("gtime", "human_times")
    H.assert_state_equal(H.download(env), want, fields, "single steps against the oracle, %s %s E=%d" % (kind, kinematics, E))
    for cuts in [(0, T), (0, 13, T)]:
        launches_against(build, acts, 2, cuts, snaps, "takes %s %s E=%d" % (kind, kinematics, E))


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_lean_takes_at_every_cut(kinematics, tuning):
    """9 envs on the packed pool, 8 steps: one launch, every cut into two, eight one-step launches.  The packed cases
    take lines and enter the 3-D LP from the first step on.  (In 8 steps only the holonomic robot, driven up the middle,
    ends an env; restarts under a unicycle robot are the 40-step batteries'.)"""
    tuning(rollout_fused=1)
    E, T = 9, 8
    acts, counts, _, _ = _battery("packed", kinematics, E, T)
    assert counts["one_take"] >= 1 and counts["several_takes"] >= 1 and counts["lp3"] >= 1, counts
    build = _build("packed", kinematics, E)
    _, snaps, _, _ = single_steps(build, acts)
    for cuts in every_cut(T):
        launches_against(build, acts, 2, cuts, snaps, "takes every cut %s" % kinematics)
