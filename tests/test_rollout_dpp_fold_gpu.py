"""The four-wavefront rollout form (env_rollout_wg4_kernel, rollout_split = 2) with its quad broadcasts folded into the
operations that read them (quad_common.hpp: Path::fold_rank, the rank's four v_sub_u32_dpp; Path::lean_lp3, the 3-D LP
candidate's three take steps in the lean form), bytes against single mcn_env_step calls and against the oracle.

The single-step kernel keeps the unfolded rank and the guarded steps, so a byte that differs between the two is a rank
or a decision that differs.  What a scene has to hold for that to show is counted on the host, from the oracle's states
and in float32 as the kernel forms its operands, BEFORE anything is launched; each class is asserted to occur:

  (a) rank: equal squared distances inside a quad (the tie rule q < k), two of them and all four;
  (b) rank: candidates out of orca_neighbor_dist (key = +inf, ties among themselves): one, several and all four of a quad;
      and a quad whose in-range count equals orca_max_neighbors (a battery with max_neighbors = 4).  A count ABOVE
      max_neighbors cannot reach this path: a quad has four candidates and the dispatcher routes orca_max_neighbors < 4 to
      the lane-per-human kernels (env_dispatch.hpp);
  (c) take steps: no take, one take, several takes, and 3-D LP entries with one round and with more than one;
  (d) the fast-range guards, per ORCA wavefront of a step (8 envs per workgroup, 3 + 3 + 2 per wavefront): a used lane
      outside the fast range in the clip only (|pref|^2 = 2^-110 > ms^2, as tests/test_oracle_edges.py's
      outside_fast_range), in the half-plane only (|w|^2 = 2^-120 on a colliding pair), in both, each beside ordinary
      quads; and a wavefront in which only an UNUSED lane is outside: the colliding pair again, in a battery whose
      orca_neighbor_dist (2^-4) is below the pair's distance.  (An out-of-range lane at the default neighbor_dist is ten
      units away, takes a leg or has |w| of the order of its speed, and stays inside the range.)
      A squared leg below 2^-102 on a used lane does not exist: the leg is read only where dist^2 > (r_a + r_b)^2, both
      float32 of magnitude >= 2^-12, and their difference is then at least one unit in the last place of the smaller.

The scenes of (a), (b) and (d) are written into the start state of chosen envs (dyadic coordinates: every squared distance
is exact); the other envs and every restart come from the packed pool (tests.rollout_harness.packed_pool), which supplies
(c).  E in {1, 8, 9, 19}, up to 40 steps, both robot kinematics, restarts inside the launch, every cut of a short
sequence.  Full state, step record, Explorer record and finished arrays after EVERY launch against single steps; the final
state against the oracle.  Every forced launch asserts mcn_last_rollout_form() == 2 (rollout_harness.launch).

What of this the change itself touches: (a) and (b) are the folded rank's inputs, the 3-D LP classes of (c) the lean steps of
lp3_candidate_quad.  The guard classes (d) run no code that the change adds (the merged guard of the step top was not
built): they are regression cover for the two separate guards on this path, beside ordinary quads.

The NaN, zero and tie half-planes of tests/edge_states.py run through this path in tests/test_rollout_wg4_gpu.py and are
not copied here."""
import functools

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests import lp1_spread_states as LS
from tests import lp2_gate_states as G
from tests.rollout_harness import every_cut, launches_against, packed_pool, random_actions, single_steps

N = 5
P, FIRST, STRIDE = 16, 7, 3
EW, EPW = 8, 3                   # envs per workgroup, envs per ORCA wavefront (env_rollout_wg4.hip: Wg4<5>)
KINEMATICS = ["holonomic", "unicycle"]
f32 = np.float32
FAST_LO = f32(2.0 ** -102)       # sqrt5's verified range starts here (fast_f32.hpp)
HR = 0.3
CLASSES = ("tie2", "tie4", "out1", "out_several", "out4", "at_max_neighbors", "no_take", "one_take", "several_takes",
           "lp3_one_round", "lp3_more_rounds", "guard_clip_only", "guard_halfplane_only", "guard_both", "guard_unused_only")


# ---------------------------------------------------------------------------------------------------------------------
# scenes: env e of the start state (oracle EnvState), five humans at rest unless a velocity is given
def _put(st, e, pos, goal=None, vel=None, vpref=None):
    pos = np.asarray(pos, np.float64)
    goal = -pos if goal is None else np.asarray(goal, np.float64)
    st.hpx[e], st.hpy[e], st.hgx[e], st.hgy[e] = pos[:, 0], pos[:, 1], goal[:, 0], goal[:, 1]
    vel = np.zeros((N, 2)) if vel is None else np.asarray(vel, np.float64)
    st.hvx[e], st.hvy[e] = vel[:, 0], vel[:, 1]
    st.hr[e] = HR
    st.hvpref[e] = 1.0 if vpref is None else np.asarray(vpref, np.float64)
    st.human_times[e] = 0


def _ties4(st, e):               # human 0 sees four candidates at 4.0; the others two at 8.0
    _put(st, e, [(0, 0), (2, 0), (0, 2), (-2, 0), (0, -2)], goal=[(3, 3), (-2, 0), (0, -2), (2, 0), (0, 2)])


def _out_one(st, e):             # the four near humans see one candidate beyond neighbor_dist, the far one four
    _put(st, e, [(0, 0), (1.5, 0), (0, 1.5), (-1.5, 0), (30, 0)], goal=[(1, 1), (-1.5, 0), (0, -1.5), (1.5, 0), (30, 4)])


def _out_several(st, e):         # the three near humans see two beyond, the far ones four
    _put(st, e, [(0, 0), (1.5, 0), (0, 1.5), (30, 0), (-30, 0)], goal=[(1, 1), (-1.5, 0), (0, -1.5), (30, 4), (-30, 4)])


def _w_tiny(st, e):
    # humans 0 and 1 overlap (0.125 apart, radii 0.31 each); v_0 - v_1 = rp / time_step + (0, 2^-60): w = (0, 2^-60)
    # on lane (0, 1) and (0, -2^-60) on lane (1, 0), |w|^2 = 2^-120, on the cut-off circle as every colliding pair
    _put(st, e, [(0, 0), (0.125, 0), (0, 3), (-3, 0), (0, -3)], goal=[(-4, 0), (4, 0), (0, -3), (3, 0), (0, 3)],
         vel=[(0.5, 2.0 ** -60), (0, 0), (0, 0), (0, 0), (0, 0)])


def _clip_tiny(st, e, who=2):
    # one human 2^-55 from its goal with preferred speed 2^-60: |pref|^2 = 2^-110 is clipped and below the fast range
    pos = [(2, 0), (0, 2), (0, 0), (-2, 2), (2, -2)]
    goal = [(-2, 0), (0, -2), (2.0 ** -55, 0), (2, -2), (-2, 2)]
    vpref = [1.0] * N
    vpref[who] = 2.0 ** -60
    _put(st, e, pos, goal=goal, vpref=vpref)


def _both(st, e):                # the overlapping pair of _w_tiny and, on human 2, the tiny clipped goal offset
    _put(st, e, [(3, 0), (3.125, 0), (0, 0), (-3, 0), (0, -3)], goal=[(-4, 0), (4, 0), (2.0 ** -55, 0), (3, 0), (0, 3)],
         vel=[(0.5, 2.0 ** -60), (0, 0), (0, 0), (0, 0), (0, 0)], vpref=[1, 1, 2.0 ** -60, 1, 1])


# wavefronts of a workgroup hold envs 0 - 2, 3 - 5, 6 - 7: the half-plane-only scene shares its wavefront with ties and a
# far candidate, the clip-only scene with far candidates and a pool case, `both` with a pool case; the next workgroups
# start with pool cases and, from env 16 on, the first wavefront's scenes again
SCENE_OF_ENV = {0: _ties4, 1: _out_one, 2: _w_tiny, 3: _out_several, 4: _clip_tiny, 6: _both, 16: _ties4, 17: _w_tiny}


# ---------------------------------------------------------------------------------------------------------------------
# host-side classes, float32 as quad_orca_core forms its operands
def _lane_flags(cfg, st, e, i):
    """human i of env e: (squared distances [4], in range [4], clip outside, per candidate: half-plane outside)"""
    with np.errstate(all="ignore"):
        others = [j for j in range(N) if j != i]
        px, py, vx, vy = f32(st.hpx[e, i]), f32(st.hpy[e, i]), f32(st.hvx[e, i]), f32(st.hvy[e, i])
        frad = f32(st.hr[e, i] + 0.01 + cfg.orca_safety_space)
        ms = f32(st.hvpref[e, i])
        prefx, prefy = f32(st.hgx[e, i] - st.hpx[e, i]), f32(st.hgy[e, i] - st.hpy[e, i])
        pp = prefx * prefx + prefy * prefy
        clip_out = bool(pp > ms * ms) and not bool(pp >= FAST_LO)
        rng2 = f32(cfg.orca_neighbor_dist) * f32(cfg.orca_neighbor_dist)
        d, inr, hp_out = [], [], []
        inv_th, inv_ts = f32(1) / f32(cfg.orca_time_horizon), f32(1) / f32(cfg.time_step)
        for j in others:
            rpx, rpy = f32(st.hpx[e, j]) - px, f32(st.hpy[e, j]) - py
            dd = rpx * rpx + rpy * rpy
            d.append(dd)
            inr.append(bool(dd < rng2))
            cr = frad + f32(st.hr[e, j] + 0.01 + cfg.orca_safety_space)
            cr_sq = cr * cr
            apart = bool(dd > cr_sq)
            inv = inv_th if apart else inv_ts
            rvx, rvy = vx - f32(st.hvx[e, j]), vy - f32(st.hvy[e, j])
            wx, wy = rvx - inv * rpx, rvy - inv * rpy
            wl_sq = wx * wx + wy * wy
            dp1 = wx * rpx + wy * rpy
            circle = (not apart) or (bool(dp1 < 0) and bool(dp1 * dp1 > cr_sq * wl_sq))
            leg_sq = dd - cr_sq
            ok = (bool(wl_sq >= FAST_LO) and bool(np.isfinite(wl_sq))) if circle else \
                (bool(leg_sq >= FAST_LO) and bool(np.isfinite(leg_sq)) and bool(dd < f32(2.0 ** 126)))
            hp_out.append(not ok)
    return np.array(d, f32), np.array(inr), clip_out, np.array(hp_out)


def _walk(lines, ms, prefx, prefy):
    """(takes of the 2-D LP, rounds of the 3-D LP) of one human over its sorted half-planes: RVO2's linearProgram2 / 3
    in float32 (tests.lp1_spread_states), counting"""
    with np.errstate(all="ignore"):
        L = [tuple(f32(v) for v in l) for l in lines]
        ms, prefx, prefy = f32(ms), f32(prefx), f32(prefy)
        if prefx * prefx + prefy * prefy > ms * ms:
            inv = f32(1) / np.sqrt(prefx * prefx + prefy * prefy)
            rx, ry = ms * (prefx * inv), ms * (prefy * inv)
        else:
            rx, ry = prefx, prefy
        takes, fail = 0, len(L)
        for i, (px, py, dx, dy) in enumerate(L):
            if dx * (py - ry) - dy * (px - rx) > 0:
                got, _ = LS.lp1(L, i, ms, prefx, prefy, False)
                if got is None:
                    fail = i
                    break
                takes += 1
                rx, ry = got
        rounds, dist = 0, f32(0)
        for i in range(fail, len(L)):
            px, py, dx, dy = L[i]
            if dx * (py - ry) - dy * (px - rx) > dist:
                rounds += 1
                rx, ry = LS.lp3(L[:i + 1], i, ms, rx, ry, set())   # one round: line i against the earlier ones
                dist = dx * (py - ry) - dy * (px - rx)
    return takes, rounds


def start_state(spec, pool, E):
    """env e from pool case e % P, the scenes written over their envs"""
    st = cport.EnvState(E, N)
    ids = np.arange(E)
    _load(st, spec, pool, ids, ids % P)
    for e, scene in SCENE_OF_ENV.items():
        if e < E:
            scene(st, e)
    return st


def _load(st, spec, pool, rows, cases):
    from modelcrowdnav_amd.envs import scenarios as S
    sc = pool[cases]
    st.hpx[rows], st.hpy[rows], st.hgx[rows], st.hgy[rows] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
    st.hvx[rows], st.hvy[rows] = sc[..., S.VX], sc[..., S.VY]
    st.hr[rows], st.hvpref[rows] = sc[..., S.RAD], sc[..., S.VPREF]
    st.human_times[rows] = 0
    rr = spec.robot_row()
    st.rpx[rows], st.rpy[rows], st.rgx[rows], st.rgy[rows] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
    st.rvx[rows], st.rvy[rows], st.rr[rows], st.gtime[rows] = 0.0, 0.0, rr[S.RAD], 0.0
    st.rtheta[rows] = rr[S.TH]


def count_classes(spec, cfg, pool, E, acts):
    """The oracle stepping E envs from start_state through acts with the in-kernel restarts, classifying every
    human-step and every ORCA wavefront of every step before the step is taken.  -> (counts, restarts, final state)"""
    st = start_state(spec, pool, E)
    ids = np.arange(E)
    next_case = (ids + FIRST) % P
    counts, restarts = dict.fromkeys(CLASSES, 0), 0
    for t in range(acts.shape[0]):
        waves = {}
        for e in range(E):
            wave = waves.setdefault((e // EW, (e % EW) // EPW), [False, False, False])   # used clip, used half-plane, unused
            for i in range(N):
                d, inr, clip_out, hp_out = _lane_flags(cfg, st, e, i)
                nin = int(inr.sum())
                eq = max(int((d[inr] == v).sum()) for v in d[inr]) if nin else 0
                counts["tie2"] += eq in (2, 3)
                counts["tie4"] += eq == 4
                counts["out1"] += nin == 3
                counts["out_several"] += nin in (1, 2)
                counts["out4"] += nin == 0
                counts["at_max_neighbors"] += nin == cfg.orca_max_neighbors
                wave[0] |= clip_out
                wave[1] |= bool((hp_out & inr).any())
                wave[2] |= bool((hp_out & ~inr).any())
                lines = G.human_lines(cfg, st, e, i)
                takes, rounds = _walk(lines, st.hvpref[e, i], f32(st.hgx[e, i] - st.hpx[e, i]),
                                      f32(st.hgy[e, i] - st.hpy[e, i]))
                if rounds:
                    counts["lp3_one_round" if rounds == 1 else "lp3_more_rounds"] += 1
                else:
                    counts[("no_take", "one_take", "several_takes")[min(takes, 2)]] += 1
        for clip, hp, unused in waves.values():
            counts["guard_clip_only"] += clip and not hp
            counts["guard_halfplane_only"] += hp and not clip
            counts["guard_both"] += clip and hp
            counts["guard_unused_only"] += unused and not clip and not hp
        ref = cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        done = np.nonzero(ref["done"])[0]
        if len(done):
            _load(st, spec, pool, done, next_case[done])
            next_case[done] = (next_case[done] + STRIDE) % P
            restarts += len(done)
    return counts, restarts, st


def _actions(kinematics, T, E):
    """a holonomic robot goes up the middle, into the crowds, so that envs end inside the launch"""
    if kinematics == "holonomic":
        rng = np.random.RandomState(31)
        return np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
    return random_actions(kinematics, T, E, 31)


DEFAULT = ("max_neighbors", 10)
AT_CUT = ("max_neighbors", 4)                                    # every quad with four candidates in range is at the cut
NEAR_SIGHTED = ("neighbor_dist", 2.0 ** -4)                      # nobody sees anybody: every lane unused


def _env(kinematics, E, variant):
    env = H.make_vec_env(E, N, kinematics=kinematics)
    setattr(env._orca, *variant)
    return env


def _build(kinematics, E, variant):
    def build():
        env = _env(kinematics, E, variant)
        spec = env.spec()
        pool = packed_pool(spec, P, N)
        ids = np.arange(E)
        env.load_scenarios(pool[ids % P])
        env.attach_rollout(gamma=0.9, pool=pool, case_stride=STRIDE, first_cases=(ids + FIRST) % P, fin_slots=2)
        H.upload(env, start_state(spec, pool, E))
        return env
    return build


@functools.lru_cache(maxsize=None)
def _battery(kinematics, E, T, variant=DEFAULT):
    """(actions, class counts, restarts, the oracle's final state), counted once per battery and before any launch"""
    probe = _env(kinematics, E, variant)
    spec, cfg = probe.spec(), H.oracle_cfg_for(probe)
    acts = _actions(kinematics, T, E)
    counts, restarts, st = count_classes(spec, cfg, packed_pool(spec, P, N), E, acts)
    return acts, counts, restarts, st


# what a battery of the default parameters holds by construction (SCENE_OF_ENV), asserted per battery in the byte test, so
# that no E / kinematics case compares bytes on a state that lacks them; the 3-D LP classes come from the packed pool
# and are asserted over the batteries of a kinematics (test_every_class_occurs)
HELD = {1: ("tie2", "tie4", "no_take", "one_take", "several_takes")}
HELD[8] = HELD[9] = HELD[19] = HELD[1] + ("out1", "out_several", "out4", "guard_clip_only", "guard_halfplane_only", "guard_both",
                                          "lp3_one_round", "lp3_more_rounds")


def _against_single_steps_and_oracle(kinematics, E, T, variant, cut_lists, what):
    acts, counts, restarts, want = _battery(kinematics, E, T, variant)
    if variant == DEFAULT:
        for k in HELD[E]:
            assert counts[k] >= 1, (what, k, counts)
    build = _build(kinematics, E, variant)
    env, snaps, _, done = single_steps(build, acts)
    assert done.sum() == restarts
    # a unicycle robot's pose goes through sin / cos, where the host's and the device's libraries differ in the last place:
    # against the oracle its envs compare in the humans (the robot is invisible to them), against single steps in everything
    fields = H.STATE_FIELDS if kinematics == "holonomic" else cport.EnvState.FIELDS_H + ("gtime", "human_times")
    H.assert_state_equal(H.download(env), want, fields, "single steps against the oracle, %s" % what)
    for cuts in cut_lists:
        launches_against(build, acts, 2, cuts, snaps, what)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_every_class_occurs(kinematics):
    """The coverage the byte tests below rest on, per kinematics, summed over their batteries (each battery's own share is
    asserted in the byte tests: HELD).  Counted on the host; marked gpu only because the env that supplies the scenario
    spec and the oracle's configuration needs a device to be made."""
    total, restarts = dict.fromkeys(CLASSES, 0), 0
    for E, T, variant in [(1, 40, DEFAULT), (8, 40, DEFAULT), (9, 40, DEFAULT), (19, 40, DEFAULT), (9, 8, AT_CUT),
                          (9, 8, NEAR_SIGHTED)]:
        _, counts, r, _ = _battery(kinematics, E, T, variant)
        print(kinematics, "E=%d T=%d" % (E, T), variant, counts, "restarts", r)
        restarts += r
        for k in CLASSES:
            if k != "at_max_neighbors" or variant == AT_CUT:
                total[k] += counts[k]
    for k in CLASSES:
        assert total[k] >= 1, (kinematics, k, total)
    assert restarts >= 1, (kinematics, restarts)


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
@pytest.mark.parametrize("E", [1, 8, 9, 19])
def test_folded_form_leaves_the_bytes_of_single_steps_and_the_oracle(E, kinematics, tuning):
    """40 steps as one launch and as two (13 + 27): restarts fall inside both."""
    tuning(rollout_fused=1)
    T = 40
    _against_single_steps_and_oracle(kinematics, E, T, DEFAULT, [(0, T), (0, 13, T)], "fold %s E=%d" % (kinematics, E))


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
@pytest.mark.parametrize("variant", [AT_CUT, NEAR_SIGHTED], ids=["max_neighbors_4", "neighbor_dist_2^-4"])
def test_folded_form_at_every_cut(variant, kinematics, tuning):
    """9 envs, 8 steps: one launch, every cut into two, eight one-step launches.  The scenes act from the first step on.
    With orca_max_neighbors = 4 every quad with four candidates in range is at the cut; with orca_neighbor_dist = 2^-4
    every key is +inf (the rank is the lane order), no line exists and the colliding pair's tiny |w| sits on unused lanes."""
    tuning(rollout_fused=1)
    E, T = 9, 8
    _, counts, _, _ = _battery(kinematics, E, T, variant)
    need = ("tie2", "tie4", "out1", "out_several", "out4", "at_max_neighbors", "guard_clip_only", "guard_halfplane_only",
            "guard_both", "one_take") if variant == AT_CUT else ("out4", "no_take", "guard_clip_only", "guard_unused_only")
    for k in need:
        assert counts[k] >= 1, (k, counts)
    _against_single_steps_and_oracle(kinematics, E, T, variant, every_cut(T), "fold every cut %s %s" % (variant[0], kinematics))
