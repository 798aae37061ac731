"""The batches of tests/lp2_gate_states.py have the properties they are made for, proved with the C oracle on the CPU:
every family is asserted non-empty (count > 0) for every shape, so that the GPU test (tests/test_lp2_gate_gpu.py)
cannot quietly cover less."""
import numpy as np
import pytest

from tests import helpers as H
from tests import lp2_gate_states as S

FREE, TAKE = S.FREE, S.TAKE


def _group_takes(tr, N):
    """[T, groups]: some human of the group (one ORCA wavefront) meets a violated line"""
    T, E, _ = tr["cls"].shape
    groups = S.group_of(E - 1, N) + 1
    out = np.zeros((T, groups), bool)
    for e in range(E):
        out[:, S.group_of(e, N)] |= tr["cls"][:, e].max(1) == TAKE
    return out


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
@pytest.mark.parametrize("family", S.FAMILIES)
def test_free_humans_get_the_clipped_preferred_velocity(family, shape):
    """The classification itself, from the oracle's own values: a human none of whose nl lines is violated by the clipped
    preferred velocity gets exactly that velocity; one with a violated line does not (it lies outside that half-plane)."""
    E, N, vis = shape
    tr = S.trace(family, E, N, vis)
    n_free = n_take = 0
    for t in range(S.T):
        act = tr["refs"][t]["human_act"]
        for e in range(E):
            for i in range(N):
                same = H.bits_equal(act[e, i], tr["pref"][t, e, i])
                if tr["cls"][t, e, i] == FREE:
                    assert same, (family, shape, t, e, i)
                    n_free += 1
                else:
                    assert not same, (family, shape, t, e, i)
                    n_take += 1
        assert not tr["refs"][t]["done"].any(), "no episode ends: the oracle does not restart envs"
    assert n_free + n_take == S.T * E * N and n_free + n_take > 0


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_all_free_with_transitions(shape):
    E, N, vis = shape
    tr = S.trace("all_free", E, N, vis)
    g = _group_takes(tr, N)
    free_steps = [t for t in range(S.T) if not g[t].any()]
    assert free_steps == [1, 2, 3, 4], g                  # the whole batch, 4 consecutive steps
    n = int((tr["cls"][1:5] == FREE).sum())
    assert n == 4 * E * N and n > 0
    assert g[0, 0] and g[5, 0], g                         # group 0: take -> skip and skip -> take inside the launch


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_one_quad_takes_and_its_mates_stay_free(shape):
    E, N, vis = shape
    tr = S.trace("one_quad", E, N, vis)
    takers = tr["cls"][0, 0] == TAKE
    assert takers.sum() > 0 and takers[0]
    assert (tr["cls"][:, 1:] == FREE).all()
    # a quad, not the whole env: somebody in env 0 is free at step 0 as well
    assert (tr["cls"][0, 0] == FREE).sum() > 0


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_boundary_exact_zero_and_both_neighbours(shape):
    E, N, vis = shape
    tr = S.trace("boundary", E, N, vis)
    exact = [e for e in range(E) if tr["on_line"][0, e, 0]]
    assert len(exact) > 0 and exact == list(range(0, E, 3)), exact
    for e in exact:                                       # on the line is not violated
        assert tr["cls"][0, e, 0] == FREE
    if E >= 3:
        above, below = list(range(1, E, 3)), list(range(2, E, 3))
        assert len(above) > 0 and len(below) > 0
        assert all(tr["cls"][0, e, 0] == TAKE and not tr["on_line"][0, e, 0] for e in above)
        assert all(tr["cls"][0, e, 0] == FREE and not tr["on_line"][0, e, 0] for e in below)
        # one ulp apart: the three preferred velocities are neighbours in float32
        px = tr["pref"][0, :3, 0, 0].astype(np.float32)
        assert np.nextafter(px[0], np.float32(np.inf)) == px[1] and np.nextafter(px[0], np.float32(-np.inf)) == px[2]


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_beyond_nl_only_a_left_out_line_is_violated(shape):
    E, N, vis = shape
    tr = S.trace("beyond_nl", E, N, vis)
    hidden = (tr["cls"][0] == FREE) & (tr["wide"][0] == TAKE)
    assert hidden[:, 0].all() and hidden.sum() > 0        # human 0 of every env, at step 0
    assert (tr["cls"][0] == FREE).all()
    if N >= 4 and E >= 2:                                 # both ways of being left out: range and max_neighbors
        cfg = S.oracle_cfg("beyond_nl", vis)
        st, _, _ = S.batch("beyond_nl", E, N, vis)
        n_in_range = [len(S.human_lines(cfg, st, e, 0, max_neighbors=10)) for e in range(E)]
        assert n_in_range[0] == 0 and n_in_range[1] == 3 and len(S.human_lines(cfg, st, 1, 0)) == 2


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_nonfinite_lines_in_a_free_group(shape):
    E, N, vis = shape
    tr = S.trace("nonfinite", E, N, vis)
    assert (tr["nonfinite"] > 0).all(), tr["nonfinite"]   # at every step
    assert (tr["cls"] == FREE).all()


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_ragged_env0_takes_every_step_the_rest_is_free(shape):
    E, N, vis = shape
    tr = S.trace("ragged", E, N, vis)
    assert (tr["cls"][:, 0].max(1) == TAKE).all() and (tr["cls"][:, 0] == TAKE).sum() > 0
    assert (tr["cls"][:, 1:] == FREE).all()


def test_ragged_shapes_have_a_partial_last_group():
    G = 64 // (4 * 5)
    assert [E for E, N, _ in S.SHAPES if N == 5 and E % G and E > G] == [4, 7]


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "E%d-N%d-vis%d" % s)
def test_packed_env_enters_the_3d_lp_its_mates_are_free(shape):
    E, N, vis = shape
    tr = S.trace("packed", E, N, vis)
    assert tr["lp3"][0, 0] > 0, tr["lp3"]
    assert (tr["lp3"][:, 1:] == 0).all()
    assert (tr["cls"][:, 1:] == FREE).all()
