"""GPU: mcn_orca_finish (orca_finish.hip) on the ORCA-edge batteries and on exact boundaries of its float64 half, every
byte against the host replay (tests/orca_finish_ref.replay on top of the C oracle's solver).

The inputs are tests/orca_finish_states.py: the dyadic edge batches of the other ORCA kernels converted to the all-ORCA
simulation, for N + 1 = 2 3 4 6 8 11 16 21 22 32 33 agents per env (wavefronts with and without idle lanes, two envs
and 20 idle lanes, idle lane 63 only, one env per wavefront) under four (max_neighbors, neighbor_dist, time_horizon,
time_step) settings, and one named case per env for the arrival test, the preferred velocity, odd human_times, the
clock, the select byte and the two radii.  tests/test_orca_finish_states_cpu.py shows that these inputs reach the
oracle's edge counters and every boundary event.  No tolerance anywhere: tests/helpers.py bit_mismatch (-0.0 against
+0.0 fails, NaN matches NaN), human_times and gtime of the boundary batch by their exact bytes.

What fails when the kernel's arithmetic is changed (each change made alone in a scratch build of orca_finish.hip, the
whole module run on the device; none of the changes touches an index, a bound or a loop condition):

  change in orca_finish.hip                                   fails (B = test_boundary_batch_matches_replay_bitwise)
  ---------------------------------------------------------   ------------------------------------------------------
  1 arrival `<` becomes `<=`                                  B, all four cases, in env arrival-touch; nothing else
  2 arrival tested on the position after the update           B in arrival-touch, arrival-before-move, f32-only; all 44
                                                              edge cases, rolled, capped; 7 tests of test_orca_finish_gpu
  3 p64 at entry taken as float64(p32)                        B, all four cases, in both arrival-f64-entry envs; of the
                                                              earlier tests only the g16 fixture states
  4 `ht == 0.0` becomes `!(ht > 0.0)` (ballot and test)       B, all four cases (times-odd); test_select_and_odd_times_
                                                              share_a_wavefront; nothing else
  5 p32 + vel * dt in float64, rounded once                   the 11 edge cases of config (3, 1.5, 2, 0.1), rolled[5-1],
                                                              capped, B at time_step 0.1; nothing at time_step 0.25
  6 gtime accumulated with (double)(float)time_step           the same tests as 5; nothing at time_step 0.25
  7 arrival against float64(float32(radius))                  B, all four cases, in arrival-below and radius-rounding;
                                                              test_select_and_odd_times_share_a_wavefront; nothing else
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import orca_finish_ref as R  # noqa: E402
from tests import orca_finish_states as S  # noqa: E402
from tests.orca_finish_harness import HELD, WRITTEN, Batch, assert_matches, tiled  # noqa: E402


def _where(names, envs):
    return sorted({names[int(e)] for e in envs})[:6]


def _matches(out, ref, names, what):
    """assert_matches, and on failure the block names of the first differing envs."""
    try:
        assert_matches(out, ref, what)
    except AssertionError as err:
        envs = set(np.nonzero(out["steps"] != ref["steps"])[0].tolist())
        for k in WRITTEN + ("sim_vel",):
            envs |= {int(i[0]) for i in H.bit_mismatch(out[k], ref[k])}
        for e, rows in enumerate(ref["traj"]):
            if len(H.bit_mismatch(out["traj"][:len(rows), e], rows)) or not np.all(out["traj"][len(rows):, e] == HELD):
                envs.add(e)
        first = sorted(envs)[:8]
        raise AssertionError("%s: %d envs differ, first %s in blocks %s (%s)" % (what, len(envs), first, _where(names, first), err))


def _take(st, vel, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in st.items()}, np.ascontiguousarray(vel[idx])


@pytest.mark.parametrize("config", range(len(S.CONFIGS)))
@pytest.mark.parametrize("N", S.HUMAN_COUNTS)
def test_edge_batches_match_replay_bitwise(N, config):
    """One launch of T_EDGE steps into a traj of T_EDGE + 2 rows: hpos, rpos, gtime, human_times, sim_vel, steps and
    traj, the rows nobody simulated still holding what they held."""
    st, vel, names = S.edge_batch(N, config)
    ref, counts, lp3 = S.edge_replay(N, config)
    b = Batch(st, vel, S.T_EDGE + 2)
    out = b.run(S.T_EDGE, **S.params(config))
    _matches(out, ref, names, "N %d config %s" % (N, S.CONFIGS[config]))
    b.untouched(out)


@pytest.mark.parametrize("N,config", [(5, 1), (7, 2)])
def test_edge_batches_under_rolled_env_order(N, config):
    """The env order rolled by 0 .. G - 1 (N = 5: ten envs and four idle lanes per wavefront; N = 7: eight envs, none
    idle): every block meets every env slot of the wavefront and the last, partial workgroup.  Envs are independent, so
    the result is the rolled replay."""
    st, vel, names = S.edge_batch(N, config)
    ref, _, _ = S.edge_replay(N, config)
    E, G = len(names), 64 // (N + 1)
    assert S.CONFIGS[config][0] < N and E % G != 0
    for r in range(G):
        idx = np.roll(np.arange(E), r)
        s, v = _take(st, vel, idx)
        b = Batch(s, v, S.T_EDGE + 2)
        out = b.run(S.T_EDGE, **S.params(config))
        _matches(out, tiled(ref, idx), [names[i] for i in idx], "N %d rolled by %d" % (N, r))
        b.untouched(out)


def test_capped_continuation_on_edge_batches():
    """max_neighbors 3 < N = 7, time_step 0.1: launches of 1, 2 and 3 steps leave the bytes of one launch of 6 and their
    traj pieces concatenate to its traj (the parity of the double-buffered tile restarts at 0 in every call)."""
    N, config = 7, 1
    assert S.CONFIGS[config] == (3, 1.5, 2.0, 0.1)
    st, vel, names = S.edge_batch(N, config)
    ref, _, _ = S.edge_replay(N, config)
    b = Batch(st, vel, S.T_EDGE)
    pieces = [[] for _ in names]
    for cap in (1, 2, 3):
        out = b.run(cap, **S.params(config))
        assert out["steps"].max() == cap
        for e in range(len(names)):
            pieces[e].append(out["traj"][:out["steps"][e], e])
            assert np.all(out["traj"][out["steps"][e]:, e] == HELD)
    out["steps"] = np.array([sum(len(p) for p in pieces[e]) for e in range(len(names))], np.int32)
    out["traj"] = np.full((S.T_EDGE,) + out["traj"].shape[1:], HELD, np.float32)
    for e in range(len(names)):
        got = np.concatenate(pieces[e])
        out["traj"][:len(got), e] = got
    _matches(out, ref, names, "1 + 2 + 3 steps")
    b.untouched(out)


@pytest.mark.parametrize("time_step", S.BOUNDARY_TIME_STEPS)
@pytest.mark.parametrize("N", S.BOUNDARY_COUNTS)
def test_boundary_batch_matches_replay_bitwise(N, time_step):
    """The named cases of boundary_batch for BOUNDARY_STEPS steps: every byte against the replay, then what the header
    says of each case directly (which step set which time, which odd human_times bytes survived)."""
    st, vel, names, select = S.boundary_batch(N)
    ref, _ = S.boundary_replay(N, time_step)
    b = Batch(st, vel, S.BOUNDARY_STEPS + 1)
    out = b.run(S.BOUNDARY_STEPS, select=select, time_step=time_step)
    _matches(out, ref, names, "boundary N %d" % N)
    for k in ("human_times", "gtime"):
        assert out[k].view(np.uint64).tolist() == ref[k].view(np.uint64).tolist(), k
    S.assert_boundary_cases(out, N, time_step, "kernel")
    b.untouched(out)


def test_select_and_odd_times_share_a_wavefront():
    """N = 5, ten envs per wavefront: unselected envs, envs whose human_times are all NaN / negative / infinite /
    subnormal (finished) and pending envs side by side, then a partial second wavefront.  The idle and the finished
    envs keep every byte, the pending ones are the replay's."""
    N = 5
    st, vel, names, select = S.boundary_batch(N)
    order = ["select-values/0", "times-odd/all-set-0", "select-values/1", "times-odd/all-set-1", "times-odd/one-zero-0",
             "select-values/0", "times-odd/all-set-3", "radius-rounding", "select-values/255", "times-odd/all-set-2",
             "times-odd/neg-zero-1", "select-values/0", "clock/2^53"]
    idx = [names.index(n) for n in order]
    ref, _ = S.boundary_replay(N, 0.25)
    s, v = _take(st, vel, idx)
    b = Batch(s, v, S.BOUNDARY_STEPS + 1)
    out = b.run(S.BOUNDARY_STEPS, select=select[idx])
    _matches(out, tiled(ref, idx), order, "mixed wavefront")
    for e, name in enumerate(order):
        if name == "select-values/0" or name.startswith("times-odd/all-set"):
            assert out["steps"][e] == 0
            for k in WRITTEN:
                assert out[k][e].tobytes() == s[k][e].tobytes(), (name, k)
            assert out["sim_vel"][e].tobytes() == v[e].tobytes() and np.all(out["traj"][:, e] == HELD), name
        else:
            assert out["steps"][e] > 0, name
    b.untouched(out)


def test_get_human_times_selects_by_the_strict_float64_test_and_starts_from_float32_velocities():
    """VecCrowdSim.get_human_times decides what the kernel is given: a robot at distance exactly rrad from its goal has
    not arrived (not selected by default, ValueError when selected), one whose radius is an ulp larger has; sim_vel
    starts from float32(rvel), float32(hvel).  The selected envs then are the replay's, bit for bit."""
    import torch
    E, N = 4, 2
    env = H.make_vec_env(E, N)
    env.reset("test", test_cases=[0, 1, 2, 3])
    up = lambda a: torch.tensor(a, dtype=torch.float64, device=env.device)
    env.rrad[:] = up([0.3125, 0.3125 + 2.0 ** -54, 0.3125, 0.3125])
    env.rpos[:] = env.rgoal + up([[0.1875, 0.25], [0.1875, 0.25], [0.0, 0.0], [3.0, 0.0]])
    env.rvel[:] = up([[0.1, 0.7], [0.1, 0.7], [-0.3, 0.2], [0.0, 0.0]])
    env.hvel[:] = up(np.random.RandomState(3).uniform(-0.5, 0.5, (E, N, 2)))
    d = (env.rpos - env.rgoal).cpu().numpy()
    assert np.sqrt(d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1]) == 0.3125
    given = []
    launch = env._orca_finish

    def spy(sim_vel, select, max_steps, steps, traj):
        given.append((sim_vel.cpu().numpy().copy(), select.cpu().numpy().copy()))
        return launch(sim_vel, select, max_steps, steps, traj)

    env._orca_finish = spy
    for bad in ([0], [0, 1], [3], torch.tensor([True, True, False, False])):
        with pytest.raises(ValueError):
            env.get_human_times(envs=bad, max_steps=4)
    assert not given
    st = {k: getattr(env, k).cpu().numpy().copy() for k in R.STATE_KEYS}
    want_vel = np.concatenate([env.rvel.cpu().numpy()[:, None], env.hvel.cpu().numpy()], 1).astype(np.float32)
    assert not np.array_equal(want_vel.astype(np.float64)[:, 0], env.rvel.cpu().numpy())
    times, steps = env.get_human_times(max_steps=4)
    assert len(given) == 1 and given[0][1].tolist() == [0, 1, 1, 0]
    assert given[0][0].dtype == np.float32 and given[0][0].tobytes() == want_vel.tobytes()
    ref = R.replay(st, want_vel, select=[0, 1, 1, 0], max_steps=4, time_step=env.time_step)
    assert steps.tolist() == ref["steps"].tolist() and steps.tolist()[0] == steps.tolist()[3] == 0 and steps.tolist()[1] > 0
    for k in WRITTEN:
        H.assert_bits_equal(getattr(env, k).cpu().numpy(), ref[k], "get_human_times " + k)
    assert times is env.human_times
