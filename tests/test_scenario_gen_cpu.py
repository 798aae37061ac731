"""CPU: the host replay of the device scenario generator (tests/scenario_gen_ref.py) is held to the published
splitmix64 vectors and, bit for bit, to the host generator of modelcrowdnav_amd/envs/scenarios.py (itself bit-exact
with the reference by tests/golden/g1_reset.npz) driven by the same stream; the table that the GPU test compares the
kernel on (scenario_gen_ref.TABLE) keeps every comparison at least 1e-9 away from its gap and reaches the cap of the
rejection loops in every dense shape."""
import numpy as np
import pytest

from modelcrowdnav_amd.envs import scenarios as S
from tests import scenario_gen_ref as R

_IDS = [e.name for e in R.TABLE]


def test_stream_is_splitmix64():
    """seed 0, case 0: the key is 0 and the raw outputs are splitmix64's published test vectors (state 0); a draw is
    the top 53 bits; the key of a negative or > 2^32 case id is that of its 64-bit two's complement."""
    assert R.case_key(0, 0) == 0
    s = R.Stream(R.case_key(0, 0))
    assert [s.raw() for _ in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    s = R.Stream(0)
    assert s.random() == (0xE220A8397B1DCDAF >> 11) * 2.0 ** -53 and s.ctr == 1
    assert R.case_key(0, 1) == 0xD1B54A32D192ED03
    assert R.case_key(0, -1) == (-0xD1B54A32D192ED03) % 2 ** 64 == R.case_key(0, 2 ** 64 - 1)
    assert R.case_key(7, 1 << 32) == 7 ^ ((0xD1B54A32D192ED03 << 32) % 2 ** 64) != R.case_key(7, 0)
    assert R.case_key(2 ** 64 - 1, 3) == R.case_key(0, 3) ^ (2 ** 64 - 1)


@pytest.mark.parametrize("N", [1, 5, 10])
@pytest.mark.parametrize("randomize", [False, True])
@pytest.mark.parametrize("rule", [R.CIRCLE, R.SQUARE])
def test_replay_equals_host_generator_on_the_same_stream(rule, randomize, N):
    """scenarios.generate has the reference's rules and no cap; on cases where the replay reaches no cap the two must
    agree on all six columns bit for bit and consume the same number of draws."""
    c = R.cfg(rule, randomize)
    seen = 0
    for seed, first in ((7, 100), (2 ** 64 - 1, -3), (0, 1 << 40)):
        for case_id in range(first, first + 12):
            got = R.replay_case(c, seed, case_id, N)
            if got.capped.any():                                  # (1 in 20 at N = 10 randomized; the host would loop on)
                continue
            want, draws = R.host_generate(c, seed, case_id, N)
            seen += 1
            assert got.draws == draws, (seed, case_id)
            assert np.array_equal(got.pos, want[:, [S.PX, S.PY]]), (seed, case_id)
            assert np.array_equal(got.goal, want[:, [S.GX, S.GY]]), (seed, case_id)
            assert np.array_equal(got.rad, want[:, S.RAD]) and np.array_equal(got.vpref, want[:, S.VPREF])
            assert not R.unplaced(got.pos, got.goal, got.rad, c).any()
    assert seen >= 30


@pytest.mark.parametrize("e", R.TABLE, ids=_IDS)
def test_table_entry_keeps_its_margin_and_its_cap_coverage(e):
    """No comparison of the replay sits within 1e-9 of its gap (five orders of magnitude above what the device's
    cos / sin / sqrt(fma) can move a distance by), so the kernel has to take the same decisions; dense entries reach
    the cap, the others do not; and the capped humans are exactly those that `unplaced` finds inside a gap."""
    b = R.replay_entry(e)
    assert b.margin >= 1e-9, b.margin
    assert b.pos.shape == (e.P, e.N, 2) and np.isfinite(b.pos).all() and np.isfinite(b.goal).all()
    assert np.array_equal(R.unplaced(b.pos, b.goal, b.rad, e.cfg), b.capped)
    if e.dense:
        assert b.capped.any() and b.max_tries == R.MAX_TRIES
    else:
        assert not b.capped.any() and b.max_tries < R.MAX_TRIES


def test_table_covers_the_shapes_and_ids():
    """The coverage the table is there for: N, P, both rules with fixed and randomized attributes, a robot off the
    axis, the seeds and first ids at which a key or counter mistake shows, one entry per dense shape."""
    assert {1, 5, 10, 32} <= {e.N for e in R.TABLE} and {1, 63, 64, 65, 130} <= {e.P for e in R.TABLE}
    assert {(e.cfg.rule, e.cfg.randomize_attributes) for e in R.TABLE} == {(r, a) for r in (R.CIRCLE, R.SQUARE)
                                                                          for a in (False, True)}
    assert {0, 7, 2 ** 64 - 1} <= {e.seed for e in R.TABLE}
    assert {0, 2 ** 32 - 2000 - 3, 2 ** 40, -3} <= {e.first_case for e in R.TABLE}
    assert any(e.first_case < 2 ** 32 <= e.first_case + e.P - 1 for e in R.TABLE)
    assert any(e.first_case < 0 <= e.first_case + e.P - 1 for e in R.TABLE)
    assert any(e.cfg.robot_goal != (0.0, e.cfg.circle_radius) for e in R.TABLE if e.cfg.rule == R.SQUARE)
    assert any(e.cfg.robot_start != (0.0, -e.cfg.circle_radius) for e in R.TABLE if e.cfg.rule == R.CIRCLE)
    dense = {(e.cfg.rule, e.cfg.randomize_attributes, e.N, e.cfg.circle_radius, e.cfg.square_width)
             for e in R.TABLE if e.dense}
    assert dense == {(R.CIRCLE, True, 10, 4.0, 10.0), (R.CIRCLE, False, 20, 4.0, 10.0), (R.CIRCLE, False, 32, 4.0, 10.0),
                     (R.CIRCLE, True, 32, 4.0, 10.0), (R.CIRCLE, False, 5, 0.5, 10.0), (R.SQUARE, False, 3, 4.0, 0.8)}


def test_cap_keeps_the_last_draw_and_the_stream_goes_on():
    """A capped circle-crossing human consumed exactly 3 * 4096 draws in its loop and holds the values of try 4096;
    the next human's draws follow on directly."""
    e = next(x for x in R.TABLE if x.name == "circle-radius0.5-N5-P2-dense")
    got = R.replay_case(e.cfg, e.seed, e.first_case, e.N)
    h = int(np.argmax(got.capped))                                # the first capped human: all before it were placed
    before = R.replay_case(e.cfg, e.seed, e.first_case, h)        # the same stream, stopped before human h
    assert not before.capped.any() and np.array_equal(before.pos, got.pos[:h])
    s = R.Stream(R.case_key(e.seed, e.first_case))
    s.ctr = before.draws + 3 * (R.MAX_TRIES - 1)
    angle = s.random() * np.pi * 2
    nx = (s.random() - 0.5) * e.cfg.human_v_pref
    ny = (s.random() - 0.5) * e.cfg.human_v_pref
    want = (e.cfg.circle_radius * np.cos(angle) + nx, e.cfg.circle_radius * np.sin(angle) + ny)
    assert tuple(got.pos[h]) == want and tuple(got.goal[h]) == (-want[0], -want[1])
    after = R.replay_case(e.cfg, e.seed, e.first_case, h + 1)
    assert after.draws == before.draws + 3 * R.MAX_TRIES and after.capped[h]


@pytest.mark.parametrize("name", ["circle-fixed-N5-P130", "circle-rand-N10-P3-dense", "square-width0.8-N3-P2-dense"])
def test_unplaced_cases_agrees_with_the_replay_on_host_tensors(name):
    """VecCrowdSim.unplaced_cases (torch, on whatever device the pool is on) has the definition of `unplaced`."""
    import torch
    from modelcrowdnav_amd.envs.crowd_sim import VecCrowdSim
    from tests import helpers as H
    e = next(x for x in R.TABLE if x.name == name)
    b = R.replay_entry(e)
    env = H.make_vec_env(1, e.N, cls=lambda E: VecCrowdSim(E, device="cpu"))
    pool = dict(hpos=torch.from_numpy(b.pos.copy()), hgoal=torch.from_numpy(b.goal.copy()),
                hrad=torch.from_numpy(b.rad.copy()))
    got = env.unplaced_cases(pool, e.cfg.rule)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), b.capped.any(axis=1))
    with pytest.raises(ValueError):
        env.unplaced_cases(pool, "mixed")
