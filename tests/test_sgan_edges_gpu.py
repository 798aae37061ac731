"""GPU: the Social-GAN step (sgan_step.hip through mcn_sgan_step) away from VecSGANWorld's shapes and at its edges.

  * N = 1 .. 32 with E x N mod 16 of many values, scenes at every lane offset of a 16-pedestrian tile, E x N < 16,
    and N = 32 with more pool-net work units than the persistent pool grid holds;
  * hcount: 0 and negative (clamped to 1), 1, N, N + 3 (clamped to N), NaN / +-inf histories beyond it, and at N = 32
    counts that end a scene in its first tile, its second, or on the boundary;
  * the ring: every (push_slot, oldest) pair, cur_pos = NULL, and np.around's rounding of the pushed frame on
    half-ties, -0.0 and large magnitudes -- all bit for bit against the numpy restatement of tests/sgan_states.py;
  * the network error against a float64 evaluation of the same inputs, with the shipped weights and with saturating
    LSTM gates.

Bar (as tests/test_sgan_gpu.py): 1e-5 on out_rel, 4e-5 on velocities (displacement / 0.25) against
oracle/pyref.sgan_generator in float32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import sgan_states as S  # noqa: E402

TOL, VTOL, TS = 1e-5, 4e-5, 0.25
TAGS = ("p", "np")
SHAPE_NS = (1, 2, 4, 5, 6, 10, 11, 15, 16, 17, 31, 32)


def _gen(tag, w=None):
    import torch
    from modelcrowdnav_amd.sgan.models import TrajectoryGenerator
    gen = TrajectoryGenerator(pooling_type="pool_net" if tag == "p" else None)
    S.load(gen, S.weights(tag) if w is None else w)
    return gen, torch.device("cuda", 0)


def _step(gen, hist, push, oldest, cur, noise, hcount=None):
    """mcn_sgan_step on copies of numpy arrays -> (hist after the call, velocities [E,N,2], out_rel [E,N,2])."""
    import torch
    from modelcrowdnav_amd.sgan.models import sgan_step
    dev = torch.device("cuda", 0)
    E, _, N, _ = hist.shape
    h = torch.from_numpy(np.ascontiguousarray(hist, np.float64)).to(dev)
    c = None if cur is None else torch.from_numpy(np.ascontiguousarray(cur, np.float64)).to(dev)
    z = torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(dev)
    hc = None if hcount is None else torch.from_numpy(np.ascontiguousarray(hcount, np.int32)).to(dev)
    vel, rel = sgan_step(gen, h, push, oldest, c, z, TS, want_rel=True, hcount=hc)
    torch.cuda.synchronize()
    return h.cpu().numpy(), vel.cpu().numpy(), rel.cpu().numpy().reshape(E, N, 2)


def _check_scenes(w, tag, hist_after, oldest, noise, vel, rel, scenes=None, counts=None, what=""):
    """Scenes (all, or the given ones) against pyref float32 on their first counts[e] pedestrians (all without
    counts)."""
    E, _, N, _ = hist_after.shape
    scenes = range(E) if scenes is None else scenes
    if counts is None:                                   # one batched reference call
        sel = np.asarray(list(scenes))
        win = S.window(hist_after[sel], oldest)
        pr, pv = S.reference(w, win, N, noise[sel], tag == "p")
        np.testing.assert_allclose(rel[sel].reshape(-1, 2), pr, rtol=0, atol=TOL, err_msg=what)
        np.testing.assert_allclose(vel[sel].reshape(-1, 2), pv, rtol=0, atol=VTOL, err_msg=what)
        return
    for e in scenes:
        n = int(min(max(counts[e], 1), N))
        win = S.window(hist_after[e:e + 1, :, :n], oldest)
        pr, pv = S.reference(w, win, n, noise[e:e + 1], tag == "p")
        np.testing.assert_allclose(rel[e, :n], pr, rtol=0, atol=TOL, err_msg="%s scene %d n %d" % (what, e, n))
        np.testing.assert_allclose(vel[e, :n], pv, rtol=0, atol=VTOL, err_msg="%s scene %d n %d" % (what, e, n))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N", SHAPE_NS)
def test_shapes_against_float32_reference(tag, N):
    """E = 1 (E x N < 16 for N < 16) and E = 19: for odd N the 19 scenes start at all 16 lane offsets of a tile, and
    E x N mod 16 is 3, 6, 12, 15, 2, 14, 1, 13, 0, 3, 13, 0 over SHAPE_NS.  Two calls in VecSGANWorld's ring order."""
    gen, _ = _gen(tag)
    w = S.weights(tag)
    for E in (1, 19):
        rng = np.random.RandomState(100 * N + E)
        hist = S.histories(rng, E, N)
        oldest = 0
        for call in range(2):
            push, nxt = oldest, (oldest + 1) & 7
            cur = S.next_positions(rng, hist, oldest)
            noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
            before = hist
            hist, vel, rel = _step(gen, before, push, nxt, cur, noise)
            H.assert_bits_equal(hist, S.ring_after(before, push, cur), what="ring E %d N %d" % (E, N))
            _check_scenes(w, tag, hist, nxt, noise, vel, rel, what="E %d N %d call %d" % (E, N, call))
            oldest = nxt


@pytest.mark.parametrize("tag", TAGS)
def test_more_pool_units_than_the_persistent_grid(tag):
    """N = 32, E = 2048: 4096 partner tiles x 7 units of five pedestrians (the last ragged), far more than the pool
    grid's workgroups x 16 wavefronts; a sample of scenes, the first and last ones included."""
    gen, _ = _gen(tag)
    w = S.weights(tag)
    E, N = 2048, 32
    rng = np.random.RandomState(7)
    hist = S.histories(rng, E, N)
    cur = S.next_positions(rng, hist, 3)
    noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
    hist_after, vel, rel = _step(gen, hist, 2, 3, cur, noise)
    assert np.isfinite(vel).all() and np.isfinite(rel).all()
    sample = np.concatenate([np.arange(4), rng.choice(np.arange(4, E - 4), 16, replace=False), np.arange(E - 4, E)])
    _check_scenes(w, tag, hist_after, 3, noise, vel, rel, scenes=sample, what="E 2048 N 32")


def _junk(hist, counts, kind, rng):
    out = hist.copy()
    for e, c in enumerate(counts):
        n = int(min(max(c, 1), hist.shape[2]))
        shape = out[e, :, n:].shape
        if kind == "finite":
            out[e, :, n:] = np.around(1000.0 + rng.uniform(0, 50, shape), 4)
        else:
            pick = rng.randint(0, 3, shape)
            out[e, :, n:] = np.where(pick == 0, np.nan, np.where(pick == 1, np.inf, -np.inf))
    return out


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N", [6, 17, 32])
def test_hcount_clamps_and_ignores_what_lies_beyond(tag, N):
    """hcount 0, -5 (both clamped to 1), 1, N, N + 3 (clamped to N) and values in between: the present pedestrians
    match the generator run on a scene of exactly that many; NaN / +-inf histories beyond hcount leave their outputs
    bit for bit as finite junk there does.  At N = 32 (two tiles per scene) counts end the scene in its first tile
    (10), on the boundary (16), just after it (17) and in its second tile (25)."""
    gen, _ = _gen(tag)
    w = S.weights(tag)
    E = 23
    rng = np.random.RandomState(N)
    counts = rng.randint(1, N + 1, E).astype(np.int32)
    counts[:5] = [0, -5, 1, N, N + 3]
    if N == 32:
        counts[5:9] = [10, 16, 17, 25]
    hist = S.histories(rng, E, N)
    cur = S.next_positions(rng, hist, 0)
    noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
    finite = _junk(hist, counts, "finite", rng)
    cur_f = cur.copy()
    for e, c in enumerate(counts):
        cur_f[e, max(c, 1):] = 2000.0
    ha, vel_a, rel_a = _step(gen, finite, 7, 0, cur_f, noise, hcount=counts)
    _check_scenes(w, tag, ha, 0, noise, vel_a, rel_a, counts=counts, what="N %d" % N)
    bad = _junk(hist, counts, "non-finite", rng)
    cur_b = cur.copy()
    for e, c in enumerate(counts):
        cur_b[e, max(c, 1):] = np.nan
    hb, vel_b, rel_b = _step(gen, bad, 7, 0, cur_b, noise, hcount=counts)
    for e, c in enumerate(counts):
        n = int(min(max(c, 1), N))
        H.assert_bits_equal(rel_b[e, :n], rel_a[e, :n], what="out_rel scene %d" % e)
        H.assert_bits_equal(vel_b[e, :n], vel_a[e, :n], what="velocity scene %d" % e)
        H.assert_bits_equal(hb[e, :, :n], ha[e, :, :n], what="ring scene %d" % e)


def test_every_ring_order_and_no_push():
    """All 64 (push_slot, oldest) pairs: the ring after the call is bit for bit the restatement (only push_slot
    changes, to np.around(cur_pos, 4)) and the outputs come from the window starting at `oldest`.  cur_pos = NULL
    leaves the ring untouched and reads the existing window."""
    gen, _ = _gen("p")
    w = S.weights("p")
    E, N = 3, 7
    rng = np.random.RandomState(11)
    hist = S.histories(rng, E, N)
    for push in range(8):
        for oldest in range(8):
            cur = S.next_positions(rng, hist, oldest)
            noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
            after, vel, rel = _step(gen, hist, push, oldest, cur, noise)
            H.assert_bits_equal(after, S.ring_after(hist, push, cur), what="ring %d %d" % (push, oldest))
            _check_scenes(w, "p", after, oldest, noise, vel, rel, what="push %d oldest %d" % (push, oldest))
    for oldest in (0, 5):
        noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
        after, vel, rel = _step(gen, hist, 3, oldest, None, noise)
        H.assert_bits_equal(after, hist, what="no push")
        _check_scenes(w, "p", after, oldest, noise, vel, rel, what="no push, oldest %d" % oldest)


def test_pushed_frame_rounds_like_numpy():
    """The pushed frame is np.around(cur_pos, 4) bit for bit on half-ties of x * 1e4 (round half to even), values that
    round to -0.0, magnitudes where x * 1e4 is an integer, both signs (tests/sgan_states.round4_values)."""
    gen, _ = _gen("p")
    vals = S.round4_values()
    N = 16
    E = (len(vals) // 2 + N - 1) // N
    cur = np.resize(vals, (E, N, 2))             # every value appears, some in x and some in y
    rng = np.random.RandomState(12)
    hist = S.histories(rng, E, N)
    for push, oldest in ((0, 1), (5, 5)):
        after, _, _ = _step(gen, hist, push, oldest, cur, np.zeros((E, 8), np.float32))
        H.assert_bits_equal(after, S.ring_after(hist, push, cur), what="round4 push %d" % push)
        assert np.array_equal(np.signbit(after[:, push]), np.signbit(np.around(cur, 4)))


@pytest.mark.parametrize("weights", ["shipped", "saturating"])
@pytest.mark.parametrize("tag", TAGS)
def test_network_error_against_float64(tag, weights, capsys):
    """|kernel - float64| <= 2 |torch float32 - float64| + 5e-7 on out_rel (the bar of the SARL / LSTM-RL float64
    tests), float64 = pyref.sgan_generator on the float32 positions / displacements the kernel sees.  'saturating'
    scales the encoder / decoder LSTM layers until their gates saturate and the encoder cell grows to |c| ~ 7."""
    import torch
    w = S.weights(tag)
    if weights == "saturating":
        w = S.saturating(w)
    gen, _ = _gen(tag, w)
    E, N = 37, 11
    rng = np.random.RandomState(13)
    hist = S.histories(rng, E, N)
    cur = S.next_positions(rng, hist, 6)
    noise = rng.normal(0, 1, (E, 8)).astype(np.float32)
    after, vel, rel = _step(gen, hist, 6, 7, cur, noise)
    win = S.window(after, 7)
    if weights == "saturating":
        assert S.encoder_cell_max(w, win)[-1] > 6.0
    p32, _ = S.reference(w, win, N, noise, tag == "p")
    p64, _ = S.reference(w, win, N, noise, tag == "p", dtype=torch.float64)
    k_err = float(np.abs(rel.reshape(-1, 2).astype(np.float64) - p64).max())
    t_err = float(np.abs(p32.astype(np.float64) - p64).max())
    with capsys.disabled():
        print("\n[sgan %s %s] kernel err %.3g  torch-f32 err %.3g  max|out_rel| %.3g" %
              (tag, weights, k_err, t_err, float(np.abs(p64).max())))
    assert k_err <= 2 * t_err + 5e-7, (k_err, t_err)
    assert float(np.abs(p64).max()) > 0.1
