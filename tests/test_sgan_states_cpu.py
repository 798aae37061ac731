"""CPU self-tests of tests/sgan_states.py (the inputs and restatements of tests/test_sgan_edges_gpu.py) and of the
float64 path of oracle/pyref.sgan_generator."""
import math

import numpy as np
import pytest
import torch

from tests import sgan_states as S


def test_round4_values_hold_every_edge():
    v = S.round4_values()
    prod = v * 1e4
    ties = np.isfinite(prod) & (prod - np.floor(prod) == 0.5)
    assert ties.sum() >= 40
    k = np.floor(prod[ties])
    assert (k % 2 == 0).any() and (k % 2 == 1).any() and (v[ties] < 0).any() and (v[ties] > 0).any()
    r = np.around(v, 4)
    assert np.array_equal(r.view(np.uint64), (np.rint(prod) / 1e4).view(np.uint64))     # numpy's own definition
    # half away from zero (C round) would disagree with round-half-even on the ties of even k
    away = np.array([math.copysign(math.floor(abs(x) + 0.5), x) for x in prod]) / 1e4
    assert (away.view(np.uint64) != r.view(np.uint64)).sum() >= 10
    minus_zero = (r == 0) & np.signbit(r)
    assert minus_zero.sum() >= 5 and ((v != 0) & minus_zero).sum() >= 4
    big = np.abs(v) >= 1e11
    assert big.sum() >= 6 and np.all(prod[big] == np.rint(prod[big])) and (v[big] < 0).any() and (v[big] > 0).any()
    assert (v < 0).sum() >= 40 and (v > 0).sum() >= 40


def test_ring_restatement_pushes_one_slot_and_reads_from_oldest():
    rng = np.random.RandomState(3)
    E, N = 3, 5
    hist = S.histories(rng, E, N)
    cur = rng.uniform(-5, 5, (E, N, 2))
    for push in range(8):
        after = S.ring_after(hist, push, cur)
        for s in range(8):
            want = np.around(cur, 4) if s == push else hist[:, s]
            assert np.array_equal(after[:, s], want)
        for oldest in range(8):
            win = S.window(after, oldest).reshape(8, E, N, 2)
            assert np.array_equal(win[(push - oldest) & 7], np.around(cur, 4))
            assert np.array_equal(win[0], after[:, oldest])
    assert np.array_equal(S.ring_after(hist, 2, None), hist)
    # VecSGANWorld's order: push over the oldest frame, which makes the pushed one the newest of the next window
    for push in range(8):
        assert ((push - ((push + 1) & 7)) & 7) == 7


def test_net_inputs_are_float32_differences_of_the_rounded_frames():
    rng = np.random.RandomState(4)
    win = S.window(S.histories(rng, 2, 3), 5)
    t32, r32 = S.net_inputs(win)
    assert t32.dtype == r32.dtype == torch.float32
    assert np.all(r32[0].numpy() == 0)
    assert np.array_equal(r32[1:].numpy(), (win[1:] - win[:-1]).astype(np.float32))


@pytest.mark.parametrize("tag", ["p", "np"])
def test_pyref_generator_follows_the_input_dtype(tag):
    """pyref.sgan_generator in float64 (float64 weights and inputs) stays float64 throughout and agrees with the float32
    path to float32 rounding; the float32 path is unchanged by the dtype plumbing."""
    from oracle import pyref
    rng = np.random.RandomState(5)
    E, N = 4, 6
    w = S.weights(tag)
    win = S.window(S.histories(rng, E, N), 0)
    noise = torch.from_numpy(rng.normal(0, 1, (E, 8)).astype(np.float32))
    p32, v32 = S.reference(w, win, N, noise, tag == "p")
    p64, _ = S.reference(w, win, N, noise, tag == "p", dtype=torch.float64)
    t32, r32 = S.net_inputs(win)
    raw = pyref.sgan_generator({k: v.double() for k, v in w.items()}, t32.double(), r32.double(), N, noise.double(),
                               tag == "p")
    assert raw.dtype == torch.float64 and p32.dtype == np.float32 and v32.dtype == np.float64
    assert 0 < np.abs(p32 - p64).max() < 5e-6
    assert np.abs(p64).max() > 0.05


def test_saturating_weights_saturate_and_grow_the_cell():
    rng = np.random.RandomState(6)
    win = S.window(S.histories(rng, 8, 10), 0)
    for tag in ("p", "np"):
        w = S.weights(tag)
        base, sat = S.encoder_cell_max(w, win), S.encoder_cell_max(S.saturating(w), win)
        assert np.all(np.diff(sat) > 0.5) and sat[-1] > 6.0 and sat[-1] > 1.5 * base[-1]      # |c| grows ~1 a step
        assert torch.equal(S.weights(tag)["encoder.encoder.weight_ih_l0"], w["encoder.encoder.weight_ih_l0"])
