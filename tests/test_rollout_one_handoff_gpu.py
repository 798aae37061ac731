"""The one-hand-off step of the four-wavefront rollout form (env_rollout_wg4_kernel, rollout_split = 2).

The ORCA wavefronts hold envs 3 w .. 3 w + 2 of their workgroup (wavefront 2: two envs), so a quad's candidates sit in
its own wavefront, and each quad carries a float64 copy of its human's position and goal, which it integrates itself
after the solve; the float64 wavefront integrates its own copy.  A normal step has one workgroup barrier; velocities and
restart flags cross it in buffers indexed by step parity.  On a restart step the float64 wavefront's restart lanes stage
the new human behind the hand-off, a second barrier follows and the ORCA quads re-read every operand, position and goal
only for the envs whose flag is set.  What can go wrong here and nowhere else:

  * the deal: env and human of a quad, the candidate's quad, the env's flag word and the staging slots at the edges of a
    wavefront (envs 2 | 3, 5 | 6), in wavefront 2's idle quads and in last workgroups of 1, 3 and 4 envs;
  * the parity of the two buffers and the barrier count: launches of 1, 2 and 3 steps, restarts on steps of both
    parities, on consecutive steps, on the first step and on the last step of a launch that another follows;
  * the ORCA copy across a restart: one env restarts while its seven neighbours keep their copy;
  * the two copies of a position drifting apart over many steps, 3-D LP rounds and overlaps included;
  * the bits of what goes through the candidate exchange: denormals, -0, NaN velocities, a NaN position;
  * a null pool pointer and a detached rollout record.

Every comparison is of BYTES: full state, step record, Explorer record and finished-episode arrays of the forced
four-wavefront form after EVERY launch against single mcn_env_step calls at that step, both robot kinematics.  Every
forced launch asserts mcn_last_rollout_form() == 2 (rollout_harness.launch).  Each test first shows, from the
single-step run or the oracle, that its inputs produce the situation it is about."""
import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests.rollout_harness import (every_cut, launches_against, oracle_rollout, packed_pool, pool_env, random_actions,
                                   single_steps)

N = 5
_P, _LIMIT = 8, 3               # pool cases; time_limit 3 s: an env whose clock reads 2 s at a step times out on it
NEVER = 100
KINEMATICS = ["holonomic", "unicycle"]


def _clock_pool(spec):
    """8 circle-crossing cases with randomised radii and v_pref; every case and human has a start velocity of its own,
    none of them a float32."""
    from modelcrowdnav_amd.envs import scenarios as S
    pool = S.scenario_pool(spec, "test", range(_P), N, "circle_crossing").copy()
    case, human = np.arange(_P)[:, None], np.arange(N)[None, :]
    pool[:, :, S.VX] = 0.1 + 0.01 * case + 0.001 * human
    pool[:, :, S.VY] = -0.3 + 0.02 * case - 0.003 * human
    return pool


def _clock_env(E, kinematics, first_done):
    """E envs on _clock_pool; the robot stands still far from everybody's path, so an env ends by its clock alone: env e
    at step first_done[e] (NEVER: not in these tests) and on the ninth step of every new episode.  Env e starts from
    case e % 8 and restarts from the next one.  Returns (env, pool)."""
    import torch
    env = H.make_vec_env(E, N, kinematics=kinematics, **{"env.time_limit": _LIMIT, "env.randomize_attributes": "true"})
    pool = _clock_pool(env.spec())
    ids = np.arange(E)
    env.load_scenarios(pool[ids % _P])
    far = torch.tensor([30.0, 30.0], dtype=torch.float64, device=env.device)
    env.rpos.copy_(far.expand(E, 2)); env.rgoal.copy_((far + 5.0).expand(E, 2))
    clock = 2.0 - 0.25 * np.asarray(first_done, dtype=np.float64)      # multiples of 1 / 4: exact
    env.gtime.copy_(torch.from_numpy(clock).to(env.device))
    env.attach_rollout(gamma=0.9, pool=pool, case_stride=1, first_cases=(ids + 1) % _P, fin_slots=3)
    return env, pool


def _expected_done(first, T):
    want = np.zeros((T, len(first)), bool)
    for e, s in enumerate(first):
        want[s::9, e] = True                                     # and on the ninth step of the new episode
    return want


def _check(build, acts, snaps, cut_list, what):
    for cuts in cut_list:
        launches_against(build, acts, 2, cuts, snaps, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. wavefront and workgroup edges of the deal
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
@pytest.mark.parametrize("E", [1, 2, 3, 4, 6, 7, 8, 9, 17, 19])
def test_deal_edges(E, kinematics, tuning):
    """7 steps.  The batch ends inside wavefront 0 (1 - 3 envs), inside wavefront 1 (4, 6), inside wavefront 2 with idle
    quads (7) and full (8), and in a last workgroup of 1 (9, 17) and 3 (19) envs behind full ones.  The last env of the
    batch restarts on step 2, the first on step 4 and, where they exist, the envs on either side of a wavefront edge
    (2 | 3 and 5 | 6 of the last workgroup) on steps 1, 3 and 5: a flag word, a staging slot or a candidate taken from
    the neighbouring env or wavefront changes bytes."""
    tuning(rollout_fused=1)
    T = 7
    first = [NEVER] * E
    base = (E - 1) // 8 * 8
    for env, step in ((base + 2, 1), (base + 3, 3), (base + 5, 5), (base + 6, 3), (0, 4), (E - 1, 2)):
        if env < E:
            first[env] = step
    build = lambda: _clock_env(E, kinematics, first)[0]
    acts = np.zeros((T, E, 2))
    _, snaps, _, done = single_steps(build, acts)
    assert (done == _expected_done(first, T)).all(), done.astype(int)
    assert done[2, E - 1] and done.any(1).sum() >= (2 if E > 1 else 1)
    _check(build, acts, snaps, [(0, T), (0, 3, T)], "deal %s E=%d" % (kinematics, E))


# ---------------------------------------------------------------------------------------------------------------------
# 2. step parity of the buffers, the barrier count
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_parity_and_barriers_every_cut(kinematics, tuning):
    """9 envs, 12 steps.  Workgroup 0 restarts on steps 0 and 1 (consecutive, both parities, the launch's first), is quiet
    on 2 - 4, restarts on 5, 7, 9, 10 and on the last step; workgroup 1 (env 8) on step 3 alone.  One launch, every
    two-launch cut and twelve one-step launches: every restart step is once the last of a launch that another follows
    and every step once the first.  Then launches of 1, 2 and 3 steps as sequences of their own."""
    tuning(rollout_fused=1)
    E, T = 9, 12
    first = [0, 1, 5, 5, 7, 11, NEVER, NEVER, 3]
    build = lambda: _clock_env(E, kinematics, first)[0]
    acts = np.zeros((T, E, 2))
    _, snaps, _, done = single_steps(build, acts)
    assert (done == _expected_done(first, T)).all(), done.astype(int)
    f = done[:, :8].any(1)
    assert list(np.nonzero(f)[0]) == [0, 1, 5, 7, 9, 10, 11], f
    assert {int(t) & 1 for t in np.nonzero(f)[0]} == {0, 1} and done[3, 8] and not f[3]
    _check(build, acts, snaps, every_cut(T), "parity %s" % kinematics)
    for short in (1, 2, 3):
        _check(build, acts[:short], snaps, every_cut(short), "parity T=%d %s" % (short, kinematics))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the ORCA copy across a restart
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_one_env_restarts_seven_keep_their_copy(kinematics, tuning):
    """8 envs, 8 steps; on steps 1 .. 6 exactly one env restarts, in turn env 0, 2, 3, 5, 6 and 7: first and last env of
    each ORCA wavefront.  The new case differs from the old in every human's position, goal, radius, v_pref and start
    velocity; the seven others pass the slow path and must keep position and goal of their own copy."""
    from modelcrowdnav_amd.envs import scenarios as S
    tuning(rollout_fused=1)
    E, T = 8, 8
    when = {0: 1, 2: 2, 3: 3, 5: 4, 6: 5, 7: 6}
    first = [when.get(e, NEVER) for e in range(E)]
    build = lambda: _clock_env(E, kinematics, first)[0]
    pool = _clock_env(E, kinematics, first)[1]
    for col in (S.PX, S.PY, S.GX, S.GY, S.RAD, S.VPREF, S.VX, S.VY):
        assert (pool != np.roll(pool, -1, 0))[:, :, col].all(), "consecutive cases share an attribute"
    vel = pool[:, :, [S.VX, S.VY]]
    assert (vel.astype(np.float32).astype(np.float64) != vel).all(), "a start velocity is a float32"
    acts = np.zeros((T, E, 2))
    _, snaps, start, done = single_steps(build, acts)
    assert (done == _expected_done(first, T)).all() and (done.sum(1) == [0, 1, 1, 1, 1, 1, 1, 0]).all(), done.astype(int)
    for e, s in when.items():
        for k in ("hpos", "hgoal", "hrad", "hvpref"):
            assert (snaps[s][k][e] != snaps[s - 1][k][e]).all(), "env %d restarts into the %s it had" % (e, k)
        assert (snaps[s]["hvel"][e] == vel[(e + 1) % _P]).all()
    _check(build, acts, snaps, [(0, T), (0, 2, T), (0, 4, 5, T)], "lone restart %s" % kinematics)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two copies of a position stay the same bits
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics,times", [("holonomic", False), ("unicycle", False), ("holonomic", True)])
def test_copies_agree_over_many_steps(kinematics, times, tuning):
    """9 envs, 40 random-action steps on a pool whose odd cases start packed: the ORCA quads integrate their copy 40
    times (fewer across restarts) while the float64 wavefront integrates the stored one; a difference in one bit shows in
    the next solve's operands.  From the oracle side: 3-D LP rounds, counted overlaps and restarts do occur."""
    tuning(rollout_fused=1)
    E, T, P = 9, 40, 16
    probe = H.make_vec_env(E, N, kinematics=kinematics)
    spec, cfg = probe.spec(), H.oracle_cfg_for(probe)
    pool = packed_pool(spec, P, N)
    acts = random_actions(kinematics, T, E, 29)
    if kinematics == "holonomic":
        # random, but up the middle: into the packed crowds (collisions) and through the open ones
        rng = np.random.RandomState(29)
        acts = np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
        _, _, restarts, overlaps, lp3 = oracle_rollout(spec, cfg, pool, np.arange(E), acts, 7, 3)
        assert lp3 > 0 and overlaps.sum() > 0 and restarts.sum() > 0, (lp3, overlaps, restarts)

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        env.track_human_times = times
        ids = np.arange(E)
        env.load_scenarios(pool[ids % P])
        env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % P, fin_slots=2)
        return env
    _, snaps, _, done = single_steps(build, acts)
    assert done.any() or kinematics != "holonomic"
    if times:
        assert (snaps[-1]["human_times"] != 0).any(), "no human arrives"
    else:
        assert (snaps[-1]["human_times"] == 0).all()
    _check(build, acts, snaps, [(0, T), (0, 13, T)], "copies %s times=%s" % (kinematics, times))


# ---------------------------------------------------------------------------------------------------------------------
# 5. values through the candidate exchange
_TINY = (1e-41, 1e-42, 1e-43, 1e-44, 1e-45, 1e-46, 1e-50)      # (float) of the last two is a zero


def _odd_values_state():
    """9 envs.  Human 0 sits (+d, -d) off its goal at the origin, d = 1e-41 .. 1e-50 (envs 0 - 6) and 1e-41 (envs 7, 8),
    so its velocity is (-d, +d) as float32: denormals, and -0 / +0 for the two smallest; humans 1 - 4 stand 4 m away (in
    range) and walk outwards.  Env 7: a NaN goal for human 2, whose velocity and then position are NaN.  Env 5: a NaN
    position of human 3 from the start.  No pool: nothing restarts."""
    E = 9
    st = cport.EnvState(E, N)
    out = np.array([(4.0, 0.0), (-4.0, 0.0), (0.0, 4.0), (0.0, -4.0)])
    for e in range(E):
        d = _TINY[e] if e < len(_TINY) else 1e-41
        st.hpx[e, 0], st.hpy[e, 0], st.hgx[e, 0], st.hgy[e, 0] = d, -d, 0.0, 0.0
        st.hpx[e, 1:], st.hpy[e, 1:] = out[:, 0], out[:, 1]
        st.hgx[e, 1:], st.hgy[e, 1:] = 2 * out[:, 0], 2 * out[:, 1]
    st.hvx[:] = 0; st.hvy[:] = 0
    st.hr[:] = 0.3; st.hvpref[:] = 1.0
    st.rpx[:], st.rpy[:], st.rgx[:], st.rgy[:] = 20.0, 20.0, 20.0, 25.0
    st.rvx[:] = 0; st.rvy[:] = 0; st.rr[:] = 0.3
    st.gtime[:] = 0
    st.hgx[7, 2] = np.nan
    st.hpx[5, 3] = np.nan
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
def test_odd_values_through_the_exchange(kinematics, tuning):
    """Denormal, -0 and NaN velocities and a NaN position through 6 steps: a quad's (px, py, rx, ry) reaches the quads
    whose candidate it is through a slot of the line table, and its own copy is integrated with the NaN.  Same bytes at
    every cut; the envs without a NaN hold none afterwards."""
    tuning(rollout_fused=1)
    st = _odd_values_state()
    E, T = st.E, 6

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        H.upload(env, st)
        env.attach_rollout(gamma=0.9, pool=None, fin_slots=2)
        return env
    acts = np.zeros((T, E, 2))
    _, snaps, _, done = single_steps(build, acts)
    assert not done.any()
    tiny = np.float32(2.0 ** -126)
    for t in range(1, T):
        w = snaps[t]["human_act"].astype(np.float32)
        assert ((np.abs(w) > 0) & (np.abs(w) < tiny)).any(), "no denormal velocity at step %d" % t
        assert ((w == 0) & np.signbit(w)).any(), "no -0 velocity at step %d" % t
        assert np.isnan(w[7]).any() and np.isnan(snaps[t]["hpos"][7, 2]).any(), "no NaN velocity at step %d" % t
        assert np.isnan(snaps[t]["hpos"][5, 3]).any(), "the NaN position is gone at step %d" % t
        clean = [e for e in range(E) if e not in (5, 7)]
        assert not np.isnan(snaps[t]["hpos"][clean]).any() and not np.isnan(snaps[t]["human_act"][clean]).any()
    _check(build, acts, snaps, every_cut(T), "odd values %s" % kinematics)


# ---------------------------------------------------------------------------------------------------------------------
# 6. no pool, no rollout record
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", KINEMATICS)
@pytest.mark.parametrize("attached", [True, False])
def test_no_pool_and_no_rollout_record(attached, kinematics, tuning):
    """9 envs, 12 random-action steps with a rollout record but no pool (envs that end stay ended: no flag is ever set,
    no pool pointer read), and with no rollout record at all."""
    tuning(rollout_fused=1)
    E, T = 9, 12

    def build():
        if attached:
            return pool_env(E, N, with_pool=False, kinematics=kinematics)
        env = H.make_vec_env(E, N, kinematics=kinematics)
        env.reset("test", test_cases=list(range(E)))
        return env
    acts = random_actions(kinematics, T, E, 31)
    _, snaps, _, _ = single_steps(build, acts)
    assert ("roll_state" in snaps[-1]) == attached
    _check(build, acts, snaps, [(0, T), (0, 1, 6, T)], "no pool attached=%s %s" % (attached, kinematics))
