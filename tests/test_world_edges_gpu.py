"""GPU: the MlpWorld / AttentionWorld kernels (world_mlp.hip, world_attn.hip) away from the shipped shapes and at
their edges, against the torch module in float32 (1e-5) and against a float64 copy of the module on the same float32
inputs (|kernel - float64| <= 2 |torch float32 - float64| + 5e-7, the bar of the SARL / LSTM-RL float64 tests).

  * MlpWorld: N = 1, 2, 4, 9 (first and last N of the kernel's three instantiations), ragged E, saturated tanh;
  * AttentionWorld: N up to 32, ragged E, 4096 x 32 on sampled scenes, scores spanning tens;
  * hcount clamping, non-finite junk beyond hcount, output slots beyond hcount never written;
  * exactly-zero attention scores: such pedestrians drop out of the softmax, and a scene whose every score is 0 gives
    NaN as torch's 0 / 0 does."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _scene(rng, E, N, spread=4.0):
    """The attributes a world adapter reads from a VecModelCrowdSim."""
    import torch
    dev = torch.device("cuda", 0)
    pos = rng.uniform(-spread, spread, (E, N, 2))
    vel = rng.uniform(-1.2, 1.2, (E, N, 2))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    return SimpleNamespace(num_envs=E, _alloc_N=N, human_num=N, device=dev, hpos=t(pos), hvel=t(vel))


def _rows(env):
    import torch
    return torch.cat([env.hpos, env.hvel], 2).reshape(env.num_envs, -1).float()


def _torch(module, x):
    import torch
    with torch.no_grad():
        return module(x).view(x.shape[0], -1, 2).double()


def _errors(module, env, got):
    """(kernel error, torch float32 error) against the module in float64 on the float32 rows."""
    import torch
    x = _rows(env)
    y32 = _torch(module, x)
    y64 = _torch(copy.deepcopy(module).double(), x.double())
    return float((got - y64).abs().max()), float((y32 - y64).abs().max()), y64


def _mlp_world(N, weights, seed):
    import torch
    from modelcrowdnav_amd.policy.world_model import MlpWorld
    torch.manual_seed(seed)
    m = MlpWorld(N).cuda().eval()
    if weights == "saturating":             # pre-tanh outputs 20x larger: tanh saturates on a good part of them
        with torch.no_grad():
            m.mlp[8].weight.mul_(20.0)
            m.mlp[8].bias.mul_(20.0)
    return m


@pytest.mark.parametrize("weights", ["shipped", "saturating"])
@pytest.mark.parametrize("N", [1, 2, 4, 9])
def test_mlp_world_shapes_against_float32_and_float64(N, weights, capsys):
    """E = 1, 15, 63, 65 (one partial wavefront, one partial and one full workgroup, one scene beyond); the float64 bar
    holds for the largest errors over all four batches (a batch of one scene has as few as 2 outputs)."""
    from modelcrowdnav_amd.policy.world_model import VecMlpWorld
    k_err = t_err = 0.0
    saturated = []
    for E in (1, 15, 63, 65):
        m = _mlp_world(N, weights, 10 * N + E)
        env = _scene(np.random.RandomState(N * 100 + E), E, N)
        got = VecMlpWorld(m, env)(env.hpos).clone()
        want = _torch(m, _rows(env))
        assert got.shape == (E, N, 2)
        assert float((got - want).abs().max()) <= TOL, (E, N)
        k, t, y64 = _errors(m, env, got)
        k_err, t_err = max(k_err, k), max(t_err, t)
        saturated.append((y64.abs() > 0.999).double().flatten().cpu().numpy())
    with capsys.disabled():
        print("\n[mlp_world N %d %s] kernel err %.3g  torch-f32 err %.3g" % (N, weights, k_err, t_err))
    assert k_err <= 2 * t_err + 5e-7, (k_err, t_err)
    if weights == "saturating":
        assert np.concatenate(saturated).mean() > 0.1


def _attn_world(seed, weights="shipped", span=30.0, env=None):
    """AttentionWorld with the default initialisation; 'saturating' scales attention.4 so that the largest score of env
    has magnitude `span` (well below expf's overflow at 88)."""
    import torch
    from modelcrowdnav_amd.policy.world_model import AttentionWorld
    torch.manual_seed(seed)
    m = AttentionWorld().cuda().eval()
    if weights == "saturating":
        s = _scores(m, _rows(env))
        with torch.no_grad():
            k = span / float(s.abs().max())
            m.attention[4].weight.mul_(k)
            m.attention[4].bias.mul_(k)
    return m


def _scores(m, x):
    """The attention scores [B, N] of AttentionWorld.forward."""
    import torch
    with torch.no_grad():
        state = x.view(x.shape[0], -1, 4)
        B, N, _ = state.shape
        h = m.mlp1(state.reshape(B * N, -1))
        g = h.view(B, N, -1).mean(1, keepdim=True).expand(B, N, 100).reshape(B * N, -1)
        return m.attention(torch.cat([h, g], 1)).view(B, N)


def _rel_err(got, want):
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("weights", ["shipped", "saturating"])
@pytest.mark.parametrize("N", [2, 11, 15, 16, 17, 31, 32])
def test_attention_world_shapes_against_float32_and_float64(N, weights, capsys):
    """E = 1, 15, 17, 65: 16 scenes per wavefront, 4 wavefronts per workgroup; float64 bar over all four batches."""
    from modelcrowdnav_amd.policy.world_model import VecAttnWorld
    k_err = t_err = 0.0
    for E in (1, 15, 17, 65):
        env = _scene(np.random.RandomState(N * 100 + E), E, N)
        m = _attn_world(10 * N + E, weights, env=env)
        if weights == "saturating":
            s = _scores(m, _rows(env))
            assert 29.0 < float(s.abs().max()) < 31.0
        got = VecAttnWorld(m, env)(env.hpos).clone()
        want = _torch(m, _rows(env))
        assert _rel_err(got, want) <= TOL, (E, N)
        k, t, _ = _errors(m, env, got)
        k_err, t_err = max(k_err, k), max(t_err, t)
    with capsys.disabled():
        print("\n[attn_world N %d %s] kernel err %.3g  torch-f32 err %.3g" % (N, weights, k_err, t_err))
    assert k_err <= 2 * t_err + 5e-7, (k_err, t_err)


def test_attention_world_4096_x_32_on_sampled_scenes():
    import torch
    from modelcrowdnav_amd.policy.world_model import VecAttnWorld
    E, N = 4096, 32
    rng = np.random.RandomState(4)
    env = _scene(rng, E, N)
    m = _attn_world(4)
    got = VecAttnWorld(m, env)(env.hpos).clone()
    assert bool(torch.isfinite(got).all())
    sample = np.concatenate([np.arange(4), rng.choice(np.arange(4, E - 4), 24, replace=False), np.arange(E - 4, E)])
    idx = torch.from_numpy(sample).cuda()
    want = _torch(m, _rows(env)[idx])
    assert _rel_err(got[idx], want) <= TOL


def _junk_beyond(env, counts, kind, rng):
    """A copy of env whose slots beyond counts hold finite junk or NaN / +-inf."""
    import torch
    pos, vel = env.hpos.cpu().numpy().copy(), env.hvel.cpu().numpy().copy()
    N = pos.shape[1]
    for e, c in enumerate(counts):
        n = int(min(max(c, 1), N))
        for a in (pos, vel):
            shape = a[e, n:].shape
            if kind == "finite":
                a[e, n:] = 1000.0 + rng.uniform(0, 50, shape)
            else:
                pick = rng.randint(0, 3, shape)
                a[e, n:] = np.where(pick == 0, np.nan, np.where(pick == 1, np.inf, -np.inf))
    t = lambda a: torch.from_numpy(a).to(env.device)
    return SimpleNamespace(num_envs=env.num_envs, _alloc_N=N, human_num=N, device=env.device, hpos=t(pos), hvel=t(vel))


@pytest.mark.parametrize("N", [5, 17, 32])
def test_attention_world_hcount_clamps_masks_and_never_writes_beyond(N):
    """hcount 0 and -3 (clamped to 1), 1, N, N + 3 (clamped to N) and random counts: the present pedestrians match the
    module run on a scene of exactly that many, NaN / +-inf beyond hcount change none of their bits, and the output
    slots beyond hcount keep what the caller left there (mcn.h: ignored and not written)."""
    import torch
    from modelcrowdnav_amd.policy.world_model import VecAttnWorld
    E = 40
    rng = np.random.RandomState(N)
    base = _scene(rng, E, N)
    counts = rng.randint(1, N + 1, E).astype(np.int32)
    counts[:5] = [0, -3, 1, N, N + 3]
    hc = torch.from_numpy(counts).cuda()
    m = _attn_world(N)
    sentinel = -12345.25
    outs = []
    for kind in ("finite", "non-finite"):
        env = _junk_beyond(base, counts, kind, rng)
        fast = VecAttnWorld(m, env)
        fast(env.hpos)                                   # allocates out_vel
        fast.out_vel.fill_(sentinel)
        got = fast(env.hpos, hcount=hc).cpu().numpy().copy()
        outs.append(got)
        x = _rows(env)
        for e in range(E):
            n = int(min(max(counts[e], 1), N))
            assert np.all(got[e, n:] == sentinel), (kind, e, n)
            if kind == "finite":
                want = _torch(m, x[e:e + 1, :4 * n]).cpu().numpy()[0]
                assert np.abs(got[e, :n] - want).max() <= TOL * max(1.0, np.abs(want).max()), (e, n)
    for e in range(E):
        n = int(min(max(counts[e], 1), N))
        assert np.array_equal(outs[0][e, :n].view(np.uint64), outs[1][e, :n].view(np.uint64)), e


def _zero_score_world(seed, all_zero=False):
    """AttentionWorld whose score of pedestrian i is relu(px_i) * d with d != 0 and exactly +-0.0 for px_i <= 0:
    mlp1 / attention.0 carry relu(px) in feature 0, attention.2 reads only that feature (bias 0), attention.4 has
    bias 0.  all_zero: attention.2 is dead for everyone (weights and bias 0), so every score is 0."""
    import torch
    m = _attn_world(seed)
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for lin, col in ((m.mlp1[0], 0), (m.mlp1[2], 0), (m.attention[0], 0)):
            lin.weight[0].zero_()
            lin.weight[0, col] = 1.0
            lin.bias[0] = 0.0
        w2 = m.attention[2].weight
        w2.zero_()
        m.attention[2].bias.zero_()
        if not all_zero:
            w2[:, 0] = torch.from_numpy(np.abs(rng.normal(0, 0.3, 100)).astype(np.float32))
        w4 = m.attention[4].weight
        d = float((w4[0] * w2[:, 0]).sum())
        if not all_zero and abs(d) < 0.3:
            w4.mul_(0.3 / abs(d))
        m.attention[4].bias.zero_()
    return m


def test_exactly_zero_scores_drop_out_and_all_zero_gives_nan():
    """Scenes with some pedestrians at px <= 0 (score exactly 0: weight 0 in torch's exp(s) (s != 0) softmax), with all
    present pedestrians there (0 / 0: NaN everywhere in torch) and with none; then a weight set whose every score is
    0.  The kernel's outputs are NaN exactly where torch's are, and equal them elsewhere."""
    import torch
    from modelcrowdnav_amd.policy.world_model import VecAttnWorld
    E, N = 48, 6
    rng = np.random.RandomState(21)
    env = _scene(rng, E, N)
    pos = env.hpos.cpu().numpy()
    pos[:, :, 0] = np.abs(pos[:, :, 0]) + 0.25
    pos[0:16, ::2, 0] *= -1.0                            # some scores exactly 0
    pos[16:32, :, 0] = -pos[16:32, :, 0]                 # every score 0
    pos[32:36, :, 0] = 0.0                               # px exactly 0: score exactly 0
    env.hpos.copy_(torch.from_numpy(pos))
    m = _zero_score_world(5)
    s = _scores(m, _rows(env)).cpu().numpy()
    assert np.all((s == 0) == (pos[:, :, 0] <= 0)) and np.abs(s[s != 0]).min() > 0.05
    got = VecAttnWorld(m, env)(env.hpos).cpu().numpy()
    want = _torch(m, _rows(env)).cpu().numpy()
    nan_w = np.isnan(want)
    assert nan_w[16:36].all() and not nan_w[:16].any() and not nan_w[36:].any()
    assert np.array_equal(np.isnan(got), nan_w)
    ok = ~nan_w
    assert np.abs(got[ok] - want[ok]).max() <= TOL * max(1.0, np.abs(want[ok]).max())
    # with hcount, only the present pedestrians' scores count: scene 0 cut to its px <= 0 pedestrian 0 is all-zero
    counts = np.full(E, N, np.int32)
    counts[0], counts[1] = 1, 2                          # pedestrian 0 has px < 0, pedestrian 1 px > 0
    part = VecAttnWorld(m, env)(env.hpos, hcount=torch.from_numpy(counts).cuda()).cpu().numpy()
    assert np.isnan(part[0, :1]).all() and np.isfinite(part[1, :2]).all()
    m0 = _zero_score_world(6, all_zero=True)
    assert np.all(_scores(m0, _rows(env)).cpu().numpy() == 0)
    got0 = VecAttnWorld(m0, env)(env.hpos).cpu().numpy()
    assert np.isnan(_torch(m0, _rows(env)).cpu().numpy()).all()
    assert np.isnan(got0).all()
