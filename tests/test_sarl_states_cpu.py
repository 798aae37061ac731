"""CPU self-tests of tests/sarl_states.py: the inputs of tests/test_sarl_edges_gpu.py hold what they claim, for every
row the GPU tests use."""
import numpy as np
import pytest
import torch

from modelcrowdnav_amd.policy.cadrl import build_action_space
from oracle import pyref
from tests import sarl_states as S

TABLE = build_action_space(1.0, "holonomic", 5, 16)[0]


def _sums(w, ref):
    """(float32 exp of every score, their per-row sums) as pyref.sarl_forward forms them."""
    s = S.scores(w, ref["feats"])
    e = torch.exp(s) * (s != 0).float()
    return e.numpy(), e.sum(1).numpy()


@pytest.mark.parametrize("shift", S.FINITE_SHIFTS)
def test_finite_shifts_are_finite_for_every_row(shift):
    w = S.shifted(S.g5_weights(), shift)
    for N in S.SOFTMAX_NS:
        st = S.softmax_batch(N)
        assert not S.reached(st).any()
        for e in range(st.E):
            ref = S.reference(w, st, e, TABLE, float64=True)
            assert np.isfinite(ref["V"]).all() and np.isfinite(ref["att"]).all()
            ex, total = _sums(w, ref)
            assert (ex > 0).all() and np.isfinite(total).all()
            assert np.abs(ref["V"] - ref["V64"]).max() < 1e-6          # the reference itself is well conditioned here
            if shift == -92.0:
                assert (total < S.TINY_SUM).all()        # 1 / sum overflows in float32, sum / sum does not
            if shift == -90.0:
                assert (total > S.TINY_SUM).all() and (total < 2.0 ** -126).all()       # subnormal, reciprocal finite
            if shift == 80.0:
                assert (total > 1e34).all()


@pytest.mark.parametrize("shift", S.NAN_SHIFTS)
def test_nan_shifts_are_nan_for_every_row(shift):
    w = S.shifted(S.g5_weights(), shift)
    for N in S.SOFTMAX_NAN_NS:
        st = S.softmax_batch(N)
        for e in range(st.E):
            ref = S.reference(w, st, e, TABLE)
            assert np.isnan(ref["V"]).all() and np.isnan(ref["att"]).all()
            ex, total = _sums(w, ref)
            assert np.isinf(ex).all() if shift > 0 else (ex == 0).all()


def test_zero_attention_scores_exactly_zero_and_zero_value_network_is_exactly_zero():
    w0 = S.g5_weights()
    for N in S.SOFTMAX_NAN_NS:
        st = S.softmax_batch(N)
        for e in range(st.E):
            ref = S.reference(S.zero_attention(w0), st, e, TABLE)
            assert (S.scores(S.zero_attention(w0), ref["feats"]).numpy() == 0).all()
            assert np.isnan(ref["V"]).all() and np.isnan(ref["att"]).all()
            z = S.reference(S.zero_value_network(w0), st, e, TABLE)
            assert (z["V"] == 0).all() and not np.signbit(z["V"]).any()
            np.testing.assert_allclose(z["att"], 1.0 / N, rtol=1e-6)
    every = {k: torch.zeros_like(v) for k, v in w0.items()}
    assert np.isnan(S.reference(every, st, 0, TABLE)["V"]).all()           # the all-zero network is 0 / 0


def test_mixed_network_scores_chosen_humans_exactly_zero():
    w = S.mixed_network(S.g5_weights())
    for N in (2, 5, 10):
        st = S.states(2, 8, N)
        st.hr[:] = S.mixed_radii(st.E, N)
        assert (st.hr[0] == 0.5).all() and (st.hr[1] == 0.25).all()
        for e in range(st.E):
            ref = S.reference(w, st, e, TABLE)
            s = S.scores(w, ref["feats"]).numpy()
            want = np.where(st.hr[e] == 0.25, 0.0, 1.0)
            assert np.array_equal(s, np.broadcast_to(want, s.shape))
            if e == 1:
                assert np.isnan(ref["V"]).all()
                continue
            assert np.isfinite(ref["V"]).all()
            assert (ref["att"][:, st.hr[e] == 0.25] == 0).all()
            np.testing.assert_allclose(ref["att"].sum(1), 1.0, rtol=1e-6)
            if e >= 2:
                assert (st.hr[e] == 0.25).any() and (st.hr[e] == 0.5).any()
        # pre-activations of the hand-set unit are far from 0: no rounding decides the class
        assert abs(0.25 - S.MIXED_RADIUS_EDGE) == abs(0.5 - S.MIXED_RADIUS_EDGE) == 0.125


@pytest.mark.parametrize("N", [5, 2])
def test_poison_batch_holds_every_value_in_every_place_and_the_reference_is_nan(N):
    clean, bad, names = S.poison_batch(N)
    assert not S.reached(clean).any()
    assert sorted(n for n in names if n) == sorted("%s:%s" % (p, v[0]) for p in S.POISON_PLACES for v in S.POISON_VALUES)
    for e, name in enumerate(names):
        fields = ("hpx", "hpy", "hvx", "hvy", "hr", "rpx", "rpy", "rgx", "rgy")
        diff = [f for f in fields if not np.array_equal(getattr(clean, f)[e], getattr(bad, f)[e], equal_nan=False)]
        if name is None:
            assert e % 2 == 0 and not diff
            # a clean env shares a 16-pair tile with each poisoned neighbour
            assert (81 * e) % 16 != 0 or (81 * (e + 1)) % 16 != 0
            continue
        place, vname = name.split(":")
        assert diff == [place]
        v = np.atleast_1d(getattr(bad, place)[e])
        v = v[~np.isfinite(v)]
        assert len(v) == 1 and np.isnan(v[0]) == vname.startswith("nan") and np.signbit(v[0]) == vname.endswith("-")
        assert (81 * e) % 16 != 0                # its first tile also holds pairs of the clean env before it
        ref = S.reference(S.g5_weights(), bad, e, TABLE)
        assert np.isnan(ref["values"]).all(), name
    t = S.poison_table(TABLE)
    ref = S.reference(S.g5_weights(), clean, 0, t)
    assert S.classes(ref["values"])[sorted(S.POISON_ROWS)].tolist() == [1, 1, 1, 1]
    assert (S.classes(ref["values"]) == 0).sum() == len(TABLE) - 4
    assert [np.signbit(t[r, r % 2]) for r in sorted(S.POISON_ROWS)] == [False, True, False, True]


def test_no_builder_puts_more_than_one_robot_in_eight_on_its_goal():
    for seed in range(15):
        for N in (1, 2, 3, 5, 6, 7, 10, 32):
            assert not S.reached(S.states(seed, 16, N)).any()
    st = S.states(14, 64, 5, on_goal=(0, 9, 31, 63))
    assert S.reached(st).nonzero()[0].tolist() == [0, 9, 31, 63]
    for kin in ("holonomic", "unicycle"):
        table = build_action_space(1.0, kin, 5, 16)[0]
        for N in (1, 5):
            st, kinds, act = S.feature_batch(N, table, kin)
            assert S.reached(st).sum() * 8 <= st.E
            assert set(kinds) >= {"on-goal", "human-on-next", "human-on-next-moving", "still-humans"}
            assert kin == "holonomic" or "heading-on-bearing" in kinds
            for e, kind in enumerate(kinds):
                if S.reached(st)[e]:
                    continue
                f = S.reference(S.g5_weights(), st, e, table, kin)["feats"][int(act[e])].numpy()
                if kind == "on-goal":
                    assert f[0, 0] == 0.0
                elif kind.startswith("human-on-next"):
                    assert (f[:, 11] == 0.0).any()
                elif kind == "still-humans":
                    assert (f[:, 8:10] == 0.0).all()
                elif kind == "heading-on-bearing":
                    assert f[0, 2] == 0.0


@pytest.mark.parametrize("A", S.ARGMAX_AS)
def test_argmax_rows_hold_their_ties_and_the_scan_picks_the_lowest_index(A):
    rows, names = S.argmax_rows(A)
    assert rows.shape == (len(names), A) and len(set(names)) == len(names)
    assert {"all-nan", "all-minus-inf", "subnormal-steps", "tie-ends", "random"} <= set(names)
    if A > 64:
        assert {"tie-stride-0", "tie-stride-last", "nan-before", "nan-after", "inf-tie"} <= set(names)
    if A >= 129:
        assert {"tie-neighbours-63", "tie-neighbours-127", "tie-stride-mid"} <= set(names)
    for v, name in zip(rows, names):
        idx, top = S.scan_argmax(v)
        if not (v > -np.inf).any():                   # all NaN, all -inf or a mixture of them: no value wins
            assert idx == -1 and top == -np.inf
            assert name in ("all-nan", "all-minus-inf", "nan-and-minus-inf") or A == 1
            continue
        assert idx >= 0
        finite_max = np.nanmax(v)
        assert top == finite_max and idx == int(np.flatnonzero(v == finite_max)[0])
        if A > 2 and (name.startswith("tie") or name == "inf-tie"):
            assert (v == finite_max).sum() >= 2, name
        if name.startswith("nan-b") or name == "nan-after":
            assert np.isnan(v).any() or A < 3
    sub = rows[names.index("subnormal-steps")]
    assert sub.max() <= 2 * S.SUB and (A < 8 or len(np.unique(sub)) == 3)


def test_reference_matches_pyref_sarl_predict():
    """sarl_states.reference is pyref.sarl_predict batched over the actions."""
    w = S.g5_weights()
    st = S.states(3, 3, 5)
    for e in range(st.E):
        row = [st.rpx[e], st.rpy[e], st.rvx[e], st.rvy[e], st.rr[e], st.rgx[e], st.rgy[e], 1.0, 0.0]
        hum = np.stack([st.hpx[e], st.hpy[e], st.hvx[e], st.hvy[e], st.hr[e]], 1)
        vals, idx = pyref.sarl_predict(w, row, hum, TABLE)
        ref = S.reference(w, st, e, TABLE)
        np.testing.assert_allclose(ref["values"], vals, rtol=0, atol=2e-7)
        assert S.scan_argmax(vals)[0] == idx
