"""No GPU: the comparing code of tests/lookahead_harness.py itself, on stand-in arrays -- what check_choice must reject
and what it must let pass -- and the helpers whose result can be written down: the env sample, the state rows against
the expressions they replace, the weight keys, the two tie constructions of tests/lookahead_states.py."""
import io

import numpy as np
import pytest

from tests import helpers as H
from tests import lookahead_harness as L
from tests import lookahead_states as LS

TABLE = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [-1.0, 0.5], [0.25, -0.75]])
REF = np.array([0.1, 0.7, 0.3, 0.5, -0.2])


def _rejects(*args, **kw):
    with pytest.raises(AssertionError):
        L.check_choice(*args, **kw)


def test_check_choice_passes_what_the_rule_allows():
    L.check_choice(REF.copy(), 1, TABLE[1], REF, TABLE, False)
    L.check_choice(REF + 0.9 * L.TOL, 1, TABLE[1], REF, TABLE, False)
    L.check_choice(REF.copy(), 1, TABLE[1], None, TABLE, False)                   # no reference: the device's own values
    L.check_choice(REF.copy(), -1, (0.0, 0.0), REF, TABLE, True)                  # on the goal
    L.check_choice(np.full(5, np.nan), -1, (0.0, 0.0), None, TABLE, False)        # no value wins
    L.check_choice(np.full(5, -np.inf), -1, (0.0, 0.0), None, TABLE, False)
    L.check_choice(np.array([np.nan, 0.2, np.nan, 0.2, 0.1]), 1, TABLE[1], None, TABLE, False)      # NaN never wins
    L.check_choice(np.array([0.4]), 0, TABLE[0], np.array([0.4]), TABLE[:1], False)                  # a one-row table


def test_check_choice_rejects_a_value_just_over_tol():
    off = REF.copy()
    off[3] += 1.01 * L.TOL
    _rejects(off, 1, TABLE[1], REF, TABLE, False)
    off[3] = REF[3] + 0.99 * L.TOL
    L.check_choice(off, 1, TABLE[1], REF, TABLE, False)
    _rejects(off, 1, TABLE[1], REF, TABLE, False, tol=0.5 * L.TOL)
    _rejects(off, -1, (0.0, 0.0), REF + 3 * L.TOL, TABLE, True)                   # the values bar holds on the goal too


def test_check_choice_wants_the_first_maximum_on_an_exact_tie():
    tie = np.array([0.1, 0.7, 0.3, 0.7, -0.2])
    L.check_choice(tie, 1, TABLE[1], None, TABLE, False)
    _rejects(tie, 3, TABLE[3], None, TABLE, False)
    _rejects(tie, 3, TABLE[3], tie, TABLE, False)


def test_check_choice_follows_the_reference_only_above_the_gap():
    ref = np.array([0.1, 0.7, 0.3, 0.7 - 1.5 * L.TOL, -0.2])                     # top-2 gap 1.5 TOL: below 2 TOL
    got = ref + np.array([0, -0.8, 0, 0.8, 0]) * L.TOL                            # the device orders the two the other way
    assert int(np.argmax(got)) == 3 and int(np.argmax(ref)) == 1
    L.check_choice(got, 3, TABLE[3], ref, TABLE, False)
    ref[3] = 0.7 - 2.5 * L.TOL                                                     # gap 2.5 TOL: the reference's choice
    got = ref.copy()
    L.check_choice(got, 1, TABLE[1], ref, TABLE, False)
    _rejects(got, 3, TABLE[3], ref, TABLE, False)
    # (with every value inside TOL a disagreement above the gap cannot be the first maximum of the device's own values;
    # the rule is stated on its own all the same: a looser value bar must not open it)
    got = ref + np.array([0, -1.5, 0, 1.5, 0]) * L.TOL
    assert int(np.argmax(got)) == 3
    _rejects(got, 3, TABLE[3], ref, TABLE, False, tol=1.2 * L.TOL)
    one = np.array([0.4])
    _rejects(one, -1, (0.0, 0.0), one, TABLE[:1], False)                          # one row: always the reference's


def test_check_choice_rejects_a_wrong_action_row():
    _rejects(REF.copy(), 1, TABLE[2], REF, TABLE, False)
    _rejects(REF.copy(), 1, (1.0, 1e-300), REF, TABLE, False)
    _rejects(REF.copy(), 1, (0.0, 0.0), None, TABLE, False)
    _rejects(np.full(5, np.nan), -1, TABLE[1], None, TABLE, False)                # no winner: the zero action


def test_check_choice_on_a_reached_env():
    _rejects(REF.copy(), 1, TABLE[1], REF, TABLE, True)
    _rejects(REF.copy(), 1, (0.0, 0.0), REF, TABLE, True)
    _rejects(REF.copy(), -1, TABLE[1], REF, TABLE, True)
    _rejects(REF.copy(), -2, (0.0, 0.0), None, TABLE, True)


def test_check_choice_rejects_nan_values_with_a_choice():
    nan = np.full(5, np.nan)
    for best in (0, 1, 4):
        _rejects(nan, best, TABLE[best], None, TABLE, False)
        _rejects(nan, best, TABLE[best], REF, TABLE, False)
    part = REF.copy()
    part[1] = np.nan
    _rejects(part, 1, TABLE[1], None, TABLE, False)                               # np.argmax would have said 1
    L.check_choice(part, 3, TABLE[3], None, TABLE, False)
    _rejects(part, 3, TABLE[3], REF, TABLE, False)                                # NaN against a finite reference


def test_sample_envs():
    for E, k, always in ((4096, 56, (1, 15, 16, 2047, 2048, 4094)), (37, 8, ()), (5, 8, (3,)), (1, 8, ()), (1333, 8, (1331, 1317))):
        got = L.sample_envs(np.random.RandomState(E), E, k, always)
        assert got == sorted(set(got)) and set(always) | {0, E - 1} <= set(got)
        assert all(0 <= e < E for e in got) and len(got) >= min(k, E)
        # the list the tests wrote out by hand, on the same stream
        rng = np.random.RandomState(E)
        assert got == sorted(set([0, E - 1] + list(always) + rng.choice(E, min(k, E), replace=False).tolist()))


def test_state_rows_equal_the_expressions_they_replace():
    rng = np.random.RandomState(3)
    E, N = 40, 6
    st = H.random_state(rng, E, N, randomize=True)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)                                   # a unicycle heading
    st.rtheta[0] = -0.0
    n_reached = 0
    for e in range(E):
        row = [st.rpx[e], st.rpy[e], st.rvx[e], st.rvy[e], st.rr[e], st.rgx[e], st.rgy[e], 1.0, st.rtheta[e]]
        H.assert_bits_equal(np.array(L.self_row(st, e)), np.array(row), "self_row")
        hum = np.stack([st.hpx[e], st.hpy[e], st.hvx[e], st.hvy[e], st.hr[e]], 1)
        assert L.humans(st, e).shape == (N, 5)
        H.assert_bits_equal(L.humans(st, e), hum, "humans")
        want = float(np.linalg.norm((st.rpy[e] - st.rgy[e], st.rpx[e] - st.rgx[e]))) < st.rr[e]
        assert L.reached(st, e) == want
        n_reached += int(want)
        js = L.joint_state(L.self_row(st, e), L.humans(st, e))
        assert (js.self_state.px, js.self_state.gy, js.self_state.theta) == (st.rpx[e], st.rgy[e], st.rtheta[e])
        assert [(h.px, h.py, h.vx, h.vy, h.radius) for h in js.human_states] == [tuple(r) for r in hum.tolist()]
    assert 0 < n_reached < E
    assert np.signbit(L.self_row(st, 0)[8])
    # exactly on the radius is outside (strict '<'): 3-4-5
    st.rpx[1], st.rpy[1], st.rgx[1], st.rgy[1], st.rr[1] = 3.0, 0.0, 0.0, 4.0, 5.0
    assert not L.reached(st, 1)
    st.rr[1] = np.nextafter(5.0, 6.0)
    assert L.reached(st, 1)


def test_weights_round_trips_a_key_with_dots():
    buf = io.BytesIO()
    a, b = np.arange(6, dtype=np.float32).reshape(2, 3), np.array([-0.0, 1.5], np.float32)
    np.savez(buf, **{"w1__mlp1__0__weight": a, "w1__attention__4__bias": b, "w10__mlp1__0__weight": a + 1, "pred1_self": b})
    buf.seek(0)
    w = L.weights(np.load(buf), "w1__")
    assert sorted(w) == ["attention.4.bias", "mlp1.0.weight"]
    H.assert_bits_equal(w["mlp1.0.weight"].numpy(), a, "weight")
    H.assert_bits_equal(w["attention.4.bias"].numpy(), b, "bias")


def _distances(st, e):
    """Exact where the tie constructions claim it: float64 offsets, numpy's 2-vector norm."""
    return [float(np.linalg.norm((st.hpx[e, i] - st.rpx[e], st.hpy[e, i] - st.rpy[e]))) for i in range(st.N)]


@pytest.mark.parametrize("N", [5, 10])
def test_both_tie_constructions_tie_exactly(N):
    E = 13
    quarter = LS.tie_state_quarter_grid(np.random.RandomState(N), E, N)
    eighth = LS.tie_state_eighth_grid(np.random.RandomState(N), E, N)
    plain = H.random_state(np.random.RandomState(N), E, N, randomize=True)
    assert not np.array_equal(quarter.hpx, eighth.hpx)                             # two different inputs, both kept
    for st in (quarter, eighth):
        for e in range(E):
            d = _distances(st, e)
            if e % 3:
                assert np.array_equal(st.hpx[e], plain.hpx[e]) and len(set(d)) == N
                continue
            assert d[0] == d[1] == d[2] > 0.0 and d[N - 1] == 0.0
            assert (st.hpx[e, 0], st.hpy[e, 0]) == (st.hpx[e, 2], st.hpy[e, 2])                   # a duplicate
            assert st.hpx[e, 0] - st.rpx[e] == -(st.hpx[e, 1] - st.rpx[e])                         # mirrored
    assert (quarter.rpx[::3] * 4 == np.round(quarter.rpx[::3] * 4)).all()
    assert np.array_equal(eighth.rpx, plain.rpx)
    for e in range(0, E, 3):
        if N > 5:
            d = _distances(eighth, e)
            assert d[N // 2] == d[0]                                               # (dy, dx) ties with (dx, -dy)
    uni = LS.tie_state_eighth_grid(np.random.RandomState(N), E, N, "unicycle")
    assert np.array_equal(uni.hpx, eighth.hpx) and uni.rtheta.any() and not eighth.rtheta.any()
