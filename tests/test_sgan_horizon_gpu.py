"""GPU: full-horizon, K-sample Social-GAN prediction (sgan_predict_kernel through mcn_sgan_predict,
TrajectoryGenerator.forward / sample, VecSGANWorld.predict).

Bars: 1e-5 per displacement against the reference's recorded float32 outputs (tests/golden/g25_sgan_horizon.npz, the
project's bar for network outputs); EDGE_TOL against the float64 restatement tests/sgan_horizon_ref.py, which is twice
the kernel's worst per-step displacement error measured on the shapes of test_tile_and_lane_edges (8.4e-7 at T = 12,
K = 2: DESIGN 3.3); everything about the loop structure bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import sgan_horizon_ref as R  # noqa: E402
from tests import sgan_states as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
EDGE_TOL = 1.7e-6
TAGS = ("np", "p")
UNIFORM = (("S6_N5", 6, 5), ("S3_N10", 3, 10), ("S4_N1", 4, 1))


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "g25_sgan_horizon.npz"))


_GENS = {}


def _gen(tag):
    import torch
    from modelcrowdnav_amd.sgan.models import TrajectoryGenerator
    if tag not in _GENS:
        _GENS[tag] = S.load(TrajectoryGenerator(pooling_type="pool_net" if tag == "p" else None), S.weights(tag))
    return _GENS[tag], torch.device("cuda", 0)


def _predict(tag, hist, oldest, noise, T, hcount=None):
    """mcn_sgan_predict on copies of numpy arrays -> (hist after the call, rel [K,T,E,N,2] f32, pos [K,T,E,N,2] f64)."""
    import torch
    from modelcrowdnav_amd.sgan.models import sgan_predict
    gen, dev = _gen(tag)
    E, _, N, _ = hist.shape
    h = torch.from_numpy(np.ascontiguousarray(hist, np.float64)).to(dev)
    z = torch.from_numpy(np.ascontiguousarray(noise, np.float32)).to(dev)
    hc = None if hcount is None else torch.from_numpy(np.ascontiguousarray(hcount, np.int32)).to(dev)
    rel, pos = sgan_predict(gen, h, oldest, z, T, hcount=hc)
    torch.cuda.synchronize()
    shape = (noise.shape[0], T, E, N, 2)
    return h.cpu().numpy(), rel.cpu().numpy().reshape(shape), pos.cpu().numpy().reshape(shape)


def _sse(sizes):
    import torch
    ends = np.cumsum(sizes)
    return torch.tensor(np.stack([ends - np.asarray(sizes), ends], 1), dtype=torch.long)


@pytest.mark.parametrize("tag", TAGS)
def test_forward_and_sample_match_reference_fixture(fixture, tag):
    """forward with decoder.seq_len 8 and 12 (sample 0's noise as user_noise) and sample with K = 3, equal-size scenes
    and the ragged batch (in the caller's row order), every displacement of every step within 1e-5; out_pos of
    VecSGANWorld.predict within (t + 1) 1e-5 of last position + float64 running sum of the reference's displacements."""
    import torch
    from modelcrowdnav_amd.policy.world_model import VecSGANWorld
    gen, dev = _gen(tag)
    try:
        for case in [c[0] for c in UNIFORM] + ["ragged"]:
            key = "%s__%s__" % (tag, case)
            traj = torch.from_numpy(fixture[key + "obs_traj"]).to(dev)
            rel_in = torch.zeros_like(traj)
            rel_in[1:] = traj[1:] - traj[:-1]
            sse, noise = _sse(fixture[key + "sizes"]), torch.from_numpy(fixture[key + "noise"]).to(dev)
            for T in (8, 12):
                want = fixture[key + "T%d__pred_rel" % T]
                gen.decoder.seq_len = T
                got = gen(traj, rel_in, sse, user_noise=noise[0])
                assert tuple(got.shape) == (T, traj.shape[1], 2) and got.dtype == torch.float32
                np.testing.assert_allclose(got.cpu().numpy(), want[0], rtol=0, atol=TOL, err_msg="%s forward T %d" % (case, T))
                got = gen.sample(traj, sse, noise, T)
                assert tuple(got.shape) == (3, T, traj.shape[1], 2)
                np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=TOL, err_msg="%s sample T %d" % (case, T))
        for case, E, N in UNIFORM:
            key = "%s__%s__" % (tag, case)
            traj = fixture[key + "obs_traj"]
            world = VecSGANWorld(gen, E, N, dev)
            world.reset_history(torch.from_numpy(traj.reshape(8, E, N, 2).transpose(1, 0, 2, 3).astype(np.float64)))
            for T in (8, 12):
                want = fixture[key + "T%d__pred_rel" % T]
                rel, pos = world.predict(T, samples=3, noise=torch.from_numpy(fixture[key + "noise"]))
                assert tuple(rel.shape) == tuple(pos.shape) == (3, T, E, N, 2)
                assert rel.dtype == torch.float32 and pos.dtype == torch.float64
                np.testing.assert_allclose(rel.cpu().numpy().reshape(want.shape), want, rtol=0, atol=TOL)
                want_pos = R.positions(traj[-1].astype(np.float64), want)
                err = np.abs(pos.cpu().numpy().reshape(want.shape) - want_pos).max(axis=(0, 2, 3))
                assert (err <= (np.arange(T) + 1) * TOL).all(), err
    finally:
        gen.decoder.seq_len = 1


@pytest.mark.parametrize("tag", TAGS)
def test_one_sample_one_step_is_the_step_kernel_bit_for_bit(tag):
    """K = 1, T = 1: out_rel equals mcn_sgan_step(cur_pos = NULL, want_rel) on the same ring, for oldest 0 and 5."""
    import torch
    from modelcrowdnav_amd.sgan.models import sgan_step
    gen, dev = _gen(tag)
    E, N = 19, 7
    rng = np.random.RandomState(21)
    hist = S.histories(rng, E, N)
    for oldest in (0, 5):
        noise = rng.normal(0, 1, (1, E, 8)).astype(np.float32)
        _, rel, pos = _predict(tag, hist, oldest, noise, 1)
        _, step_rel = sgan_step(gen, torch.from_numpy(hist).to(dev), 0, oldest, None, torch.from_numpy(noise[0]).to(dev), 0.25,
                                want_rel=True)
        H.assert_bits_equal(rel.reshape(E * N, 2), step_rel.cpu().numpy(), what="oldest %d" % oldest)
        assert np.abs(rel).max() > 0.01


@pytest.mark.parametrize("tag", TAGS)
def test_loop_structure_is_deterministic(tag):
    """Steps 0 .. T' - 1 of a T-step call equal a T'-step call, sample k of a K = 3 call equals a K = 1 call with
    noise[k] (displacements and positions, bit for bit), and hist is unchanged after the call."""
    E, N = 9, 5
    rng = np.random.RandomState(22)
    hist = S.histories(rng, E, N)
    noise = rng.normal(0, 1, (3, E, 8)).astype(np.float32)
    runs = {}
    for T in (12, 8, 1):
        after, runs[T], pos = _predict(tag, hist, 3, noise, T)
        H.assert_bits_equal(after, hist, what="hist after T %d" % T)
        runs[T] = (runs[T], pos)
    for T, Tp in ((12, 8), (8, 1)):
        H.assert_bits_equal(runs[T][0][:, :Tp], runs[Tp][0], what="rel T %d / %d" % (T, Tp))
        H.assert_bits_equal(runs[T][1][:, :Tp], runs[Tp][1], what="pos T %d / %d" % (T, Tp))
    for k in range(3):
        _, rel, pos = _predict(tag, hist, 3, noise[k:k + 1], 12)
        H.assert_bits_equal(rel[0], runs[12][0][k], what="rel sample %d" % k)
        H.assert_bits_equal(pos[0], runs[12][1][k], what="pos sample %d" % k)
    assert np.abs(runs[12][0][0] - runs[12][0][1]).max() > 1e-3


def _edge_error(tag, hist, oldest, noise, T, rel, pos, what, counts=None, scenes=None):
    """Worst |kernel - float64 restatement| over the present pedestrians' displacements, printed then returned; out_pos
    is checked against the restatement's running sum with (t + 1) times the bound."""
    sel = np.arange(hist.shape[0]) if scenes is None else np.asarray(scenes)
    want = R.predict_ring(R.weights64(tag), hist[sel], oldest, noise[:, sel], T, tag == "p",
                          None if counts is None else np.asarray(counts)[sel])
    present = ~np.isnan(want)
    err = float(np.abs(rel[:, :, sel].astype(np.float64) - want)[present].max())
    print("[sgan predict %s %s] worst displacement error vs float64: %.3g" % (tag, what, err))
    last = S.window(hist[sel], oldest)[-1].astype(np.float32).astype(np.float64).reshape(len(sel), hist.shape[2], 2)
    want_pos = np.cumsum(want, axis=1) + last[None, None]
    perr = np.where(present, np.abs(pos[:, :, sel] - want_pos), 0.0).max(axis=(0, 2, 3, 4))
    assert (perr <= (np.arange(T) + 1) * EDGE_TOL).all(), (what, perr)
    return err


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("E,N", [(1, 1), (3, 5), (16, 1), (17, 1), (13, 10)])
def test_tile_and_lane_edges(tag, E, N):
    """E x N = 1, 15, 16, 17 and 130: a lone pedestrian, one short of a 16-pedestrian tile, exactly a tile, one over, and
    a last tile of 2 alone in the third workgroup.  T = 12, K = 2, against the float64 restatement."""
    rng = np.random.RandomState(1000 * E + N)
    hist = S.histories(rng, E, N)
    noise = rng.normal(0, 1, (2, E, 8)).astype(np.float32)
    _, rel, pos = _predict(tag, hist, 6, noise, 12)
    err = _edge_error(tag, hist, 6, noise, 12, rel, pos, "E %d N %d" % (E, N))
    assert err <= EDGE_TOL, err


@pytest.mark.parametrize("tag", TAGS)
def test_hcount_limits_the_scene(tag):
    """E = 40, N = 6, hcount[e] in 1 .. N: the present pedestrians equal the restatement run on a scene of hcount[e]
    pedestrians, and refilling the padded slots of hist with other finite values leaves their outputs bit-identical."""
    E, N, T = 40, 6, 12
    rng = np.random.RandomState(23)
    counts = rng.randint(1, N + 1, E).astype(np.int32)
    counts[:3] = [1, N, N - 1]
    hist = S.histories(rng, E, N)
    noise = rng.normal(0, 1, (2, E, 8)).astype(np.float32)
    fills = []
    for base in (1000.0, -37.0):
        h = hist.copy()
        for e, c in enumerate(counts):
            h[e, :, c:] = np.around(base + rng.uniform(0, 50, h[e, :, c:].shape), 4)
        fills.append(h)
    _, rel_a, pos_a = _predict(tag, fills[0], 2, noise, T, hcount=counts)
    err = _edge_error(tag, fills[0], 2, noise, T, rel_a, pos_a, "hcount", counts=counts)
    assert err <= EDGE_TOL, err
    _, rel_b, pos_b = _predict(tag, fills[1], 2, noise, T, hcount=counts)
    for e, c in enumerate(counts):
        H.assert_bits_equal(rel_b[:, :, e, :c], rel_a[:, :, e, :c], what="rel scene %d" % e)
        H.assert_bits_equal(pos_b[:, :, e, :c], pos_a[:, :, e, :c], what="pos scene %d" % e)


@pytest.mark.parametrize("E,N,K,T", [(17, 1, 2, 3), (3, 5, 3, 12)])
def test_outputs_stay_inside_their_buffers(E, N, K, T):
    """out_rel / out_pos sit between 4096 guard bytes holding a pattern: the guards are intact after the call and every
    element between them was written."""
    import torch
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.sgan.models import _workspace
    G = 4096
    gen, dev = _gen("p")
    net, _keep = gen.pack(dev)
    rng = np.random.RandomState(24)
    hist = torch.from_numpy(S.histories(rng, E, N)).to(dev)
    noise = torch.from_numpy(rng.normal(0, 1, (K, E, 8)).astype(np.float32)).to(dev)
    n = K * T * E * N * 2
    bufs = [torch.full((G + n * size + G,), 0xA5, dtype=torch.uint8, device=dev) for size in (4, 8)]
    rc = _hip.lib.mcn_sgan_predict(C.byref(net), _hip.ptr(hist), 1, _hip.ptr(noise), K, T, None,
                                   _hip.ptr(_workspace(E, N, dev)), C.c_void_p(bufs[0].data_ptr() + G),
                                   C.c_void_p(bufs[1].data_ptr() + G), E, N, _hip.stream_ptr(dev))
    assert rc == _hip.MCN_OK
    torch.cuda.synchronize()
    for b, dt in zip(bufs, (torch.float32, torch.float64)):
        host = b.cpu()
        assert bool((host[:G] == 0xA5).all()) and bool((host[-G:] == 0xA5).all())
        vals = host[G:-G].clone().view(dt)
        assert bool(torch.isfinite(vals).all()) and float(vals.abs().max()) < 100.0
        assert not bool((host[G:-G].view(-1, 4) == 0xA5).all(dim=1).any())                # no word still holds the pattern


def test_predict_does_not_disturb_stepping():
    """Two worlds from the same seed and history; one calls predict(8, samples=4, noise=given) between its steps: their
    __call__ outputs over 5 steps (noise drawn from the world's generator) are bit-identical."""
    import torch
    from modelcrowdnav_amd.policy.world_model import VecSGANWorld
    gen, dev = _gen("p")
    E, N = 11, 5
    rng = np.random.RandomState(25)
    hist = torch.from_numpy(S.histories(rng, E, N))
    given = torch.from_numpy(rng.normal(0, 1, (4, E, 8)).astype(np.float32))
    worlds = [VecSGANWorld(gen, E, N, dev, seed=3) for _ in range(2)]
    for w in worlds:
        w.reset_history(hist)
    pos = hist[:, -1].clone()
    for step in range(5):
        pos = pos + 0.05 + 0.01 * step
        a = worlds[0](pos.to(dev)).cpu().numpy().copy()
        rel, p = worlds[1].predict(8, samples=4, noise=given)
        assert tuple(rel.shape) == (4, 8, E, N, 2)
        b = worlds[1](pos.to(dev)).cpu().numpy().copy()
        H.assert_bits_equal(b, a, what="step %d" % step)
        assert worlds[0].oldest == worlds[1].oldest
        H.assert_bits_equal(worlds[1].hist.cpu().numpy(), worlds[0].hist.cpu().numpy(), what="ring %d" % step)
    assert np.abs(a).max() > 0.01


def test_benchmark_shape_on_sampled_scenes():
    """4096 x 10, pool-net weights, T = 8, K = 1: 64 sampled scenes (0 and E - 1 among them) against the restatement,
    every output finite."""
    E, N, T = 4096, 10, 8
    rng = np.random.RandomState(26)
    hist = S.histories(rng, E, N)
    noise = rng.normal(0, 1, (1, E, 8)).astype(np.float32)
    _, rel, pos = _predict("p", hist, 4, noise, T)
    assert np.isfinite(rel).all() and np.isfinite(pos).all()
    sample = np.concatenate([[0, E - 1], rng.choice(np.arange(1, E - 1), 62, replace=False)])
    err = _edge_error("p", hist, 4, noise, T, rel, pos, "4096 x 10", scenes=sample)
    assert err <= EDGE_TOL, err
