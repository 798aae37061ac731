"""GPU: mcn_scenario_pool (scenario_gen.hip) against its host replay (tests/scenario_gen_ref.py) on the shared table
of cases -- draw order, noise scale, every rejection test, the cap of the rejection loops, case ids beyond 2^32 and
below zero, the tail guard -- and the ids a device_scenarios rollout starts and restarts its episodes from.

Every table entry keeps each comparison of the replay at least 1e-9 from its gap (test_scenario_gen_cpu.py), so the
kernel, whose distances differ from the replay's by ~1e-15, has to take the same decisions: a mismatch is the kernel's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import scenario_gen_ref as R  # noqa: E402
from tests.rollout_harness import goal_seeking  # noqa: E402

# Largest error of double cos / sin of the device math library (OCML) in ulps: the library implements the OpenCL C
# math functions, whose specification (OpenCL C 3.0, 7.4 "Relative error as ULPs") allows double sin and cos 4 ulp.
COS_SIN_ULPS = 4
PAD = 64           # cases allocated beyond P, NaN-filled: the kernel must leave them alone


def circle_tolerance(circle_radius):
    """Device and replay each hold cos / sin within COS_SIN_ULPS ulps (of a value <= 1: 2^-52 at most) of the true
    one, so circle_radius * cos differs by at most 2 * COS_SIN_ULPS * 2^-52 * circle_radius; the product and the sum
    with the noise then round once each: 4x that in all."""
    return 4 * (2 * COS_SIN_ULPS * 2.0 ** -52 * circle_radius)


def _generate(c, seed, first_case, P, N):
    """mcn_scenario_pool called like VecCrowdSim.device_pool calls it, into arrays of P + PAD cases filled with NaN.
    Returns the four arrays whole, as numpy."""
    import torch
    from modelcrowdnav_amd import _hip
    sc = _hip.ScenarioCfg(c.circle_radius, c.square_width, c.discomfort_dist, c.human_radius, c.human_v_pref,
                          c.robot_radius, tuple(c.robot_start), tuple(c.robot_goal),
                          {R.CIRCLE: _hip.RULE_CIRCLE, R.SQUARE: _hip.RULE_SQUARE}[c.rule],
                          1 if c.randomize_attributes else 0)
    dev = torch.device("cuda", torch.cuda.current_device())
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
    out = [nan(P + PAD, N, 2), nan(P + PAD, N, 2), nan(P + PAD, N), nan(P + PAD, N)]
    rc = _hip.lib.mcn_scenario_pool(sc, seed & R.MASK, first_case, P, N, *[_hip.ptr(t) for t in out],
                                    _hip.stream_ptr(dev))
    _hip.check(rc, "mcn_scenario_pool")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _assert_matches(c, pos, goal, rad, vpref, want, what):
    """Device arrays of some cases against the replay's (same leading shape)."""
    assert np.array_equal(rad, want.rad), what
    assert np.array_equal(vpref, want.vpref), what
    if c.rule == R.SQUARE:                            # products and sums of draws: no transcendental, bit-equal
        assert np.array_equal(pos, want.pos), what
        assert np.array_equal(goal, want.goal), what
        return 0.0
    assert np.array_equal(goal, -pos), what
    diff = float(np.abs(pos - want.pos).max())
    assert diff <= circle_tolerance(c.circle_radius), (what, diff, circle_tolerance(c.circle_radius))
    return diff


@pytest.mark.parametrize("e", R.TABLE, ids=[e.name for e in R.TABLE])
def test_kernel_equals_replay(e):
    """hrad, hvpref bit-equal; a square crossing's hpos, hgoal bit-equal; a circle crossing's hgoal == -hpos exactly
    and its hpos within circle_tolerance (2.8e-14 on the shipped circle of radius 4, from the math library's
    documented 4 ulp for double cos / sin, not from what the kernel returns) of the replay.  In dense entries the
    humans inside a gap are exactly those the replay capped: the last draw is kept and the stream goes on.  The PAD
    cases beyond P still hold NaN, the cases below P none."""
    want = R.replay_entry(e)
    out = _generate(e.cfg, e.seed, e.first_case, e.P, e.N)
    for a in out:
        assert np.isnan(a[e.P:]).all() and not np.isnan(a[:e.P]).any()
    pos, goal, rad, vpref = (a[:e.P] for a in out)
    diff = _assert_matches(e.cfg, pos, goal, rad, vpref, want, e.name)
    print("%s: largest |hpos - replay| = %.3e (tolerance %.3e)" % (e.name, diff, circle_tolerance(e.cfg.circle_radius)))
    assert np.array_equal(R.unplaced(pos, goal, rad, e.cfg), want.capped)
    assert want.capped.any() == e.dense


@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("N", [1, 5, 32])
def test_nothing_is_written_beyond_P(P, N):
    """Below, at and across a wavefront, two workgroups and a tail: rows >= P keep their NaN, rows < P hold none."""
    for a in _generate(R.cfg(R.SQUARE, True), 7, 0, P, N):
        assert np.isnan(a[P:]).all() and a[P:].shape[0] == PAD
        assert not np.isnan(a[:P]).any()


@pytest.mark.parametrize("first_case", [100, -3, (1 << 32) - 68, 1 << 40])
def test_a_case_depends_on_its_id_only(first_case):
    """Rows [65, 130) of (first_case, P = 130) == (first_case + 65, P = 65) == 65 calls of P = 1, bit for bit, on
    all four outputs (ids across zero and across 2^32 included)."""
    c = R.cfg(R.CIRCLE, True)
    whole = [a[65:130] for a in _generate(c, 2 ** 64 - 1, first_case, 130, 5)]
    half = [a[:65] for a in _generate(c, 2 ** 64 - 1, first_case + 65, 65, 5)]
    singles = [_generate(c, 2 ** 64 - 1, first_case + 65 + i, 1, 5) for i in range(65)]
    for k in range(4):
        assert np.array_equal(whole[k], half[k])
        assert np.array_equal(whole[k], np.concatenate([s[k][:1] for s in singles]))
    assert len({whole[0][i].tobytes() for i in range(65)}) == 65                # and no two ids share a crowd


@pytest.mark.parametrize("name, over", [("circle-fixed-N5-P130", {}),
                                        ("circle-rand-N10-P3-dense", {"env.randomize_attributes": "true"}),
                                        ("square-width0.8-N3-P2-dense", {"sim.square_width": "0.8"})])
def test_unplaced_cases_are_the_replays_capped_cases(name, over):
    """VecCrowdSim.unplaced_cases on a device_pool() == the cases in which the replay capped a human."""
    e = next(x for x in R.TABLE if x.name == name)
    env = H.make_vec_env(1, e.N, **over)
    pool = env.device_pool(e.seed, e.first_case, e.P, e.N, e.cfg.rule)
    got = env.unplaced_cases(pool, e.cfg.rule)
    assert got.device == pool["hpos"].device and tuple(got.shape) == (e.P,)
    want = R.replay_entry(e).capped.any(axis=1)
    assert np.array_equal(got.cpu().numpy(), want) and want.any() == e.dense


@pytest.mark.parametrize("rounds", [1, 2])
@pytest.mark.parametrize("phase, counter", [("train", 37), ("val", 11)])
def test_rollout_plays_the_case_ids_of_its_phase(phase, counter, rounds):
    """run_k_episodes(device_scenarios=seed) over E = 8 envs: env e starts from case id offset(phase) + counter + e
    (train: case_capacity val + test = 2000, val: 0) and restarts from id + E when it has a second episode to play
    -- goals, radii and preferred speeds, which do not change during an episode, against the replay of those ids."""
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.rollout import VecExplorer
    E, N, seed = 8, 5, 2 ** 64 - 1
    env = H.make_vec_env(E, N, **{"env.randomize_attributes": "true"})
    env.track_human_times = False; env.export_human_actions = False
    env.case_counter[phase] = counter
    offset = {"train": env.case_capacity["val"] + env.case_capacity["test"], "val": 0}[phase]
    assert offset == {"train": 2000, "val": 0}[phase]
    n, rule = env._phase_rule(phase)
    assert n == N
    c = R.cfg(rule, True)
    snap = lambda: [t.cpu().numpy().copy() for t in (env.hgoal, env.hrad, env.hvpref)]
    first, bufs = [], []
    attach = env.attach_rollout

    def action_fn(env_, t):
        if t == 0:
            first.extend(snap())
        return goal_seeking(env_, t)

    env.attach_rollout = lambda *a, **kw: bufs.append(attach(*a, **kw)) or bufs[0]
    ex = VecExplorer(env, env.robot, gamma=0.9, policy=object())
    ex.run_k_episodes(rounds * E, phase, action_fn=action_fn, device_scenarios=seed)
    last = snap()
    assert env.case_counter[phase] == counter + rounds * E
    # every env finished `rounds` episodes and both finished-episode slots hold an outcome
    assert int(bufs[0]["fin_count"].min()) >= rounds and bufs[0]["fin_info"].shape[0] == 2
    if rounds == 2:
        assert (bufs[0]["fin_info"].cpu().numpy() >= _hip.INFO_REACHGOAL).all()
        assert (bufs[0]["fin_time"].cpu().numpy() > 0).all()
    assert len(ex.last_records["infos"]) == rounds * E
    plays = [R.replay(c, seed, offset + counter + r * E, E, N) for r in range(rounds)]
    tol = circle_tolerance(c.circle_radius) if rule == R.CIRCLE else 0.0

    def same(got, want, e):
        return (np.array_equal(got[1][e], want.rad[e]) and np.array_equal(got[2][e], want.vpref[e]) and
                float(np.abs(got[0][e] - want.goal[e]).max()) <= tol)

    for e in range(E):
        assert same(first, plays[0], e), (e, "first episode")
        assert any(same(last, w, e) for w in plays), (e, "restart")
    # the ids are distinct crowds: no env can pass with another env's case
    assert len({w.rad[e].tobytes() for w in plays for e in range(E)}) == rounds * E
