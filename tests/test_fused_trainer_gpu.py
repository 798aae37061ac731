"""GPU: the fused SARL training step (csrc/sarl_train.hip through mcn_sarl_loss_grad / mcn_sgd_momentum_step and
Trainer(fused=True)) against the float64 yardstick of tests/trainer_ref.py.  Every bound is a multiple of what torch's
own float32 path (or the reference's recorded float32 Trainer) is away from that yardstick on the same inputs; nothing
is compared with an earlier output of the kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fused_train_harness as F  # noqa: E402
from tests import trainer_ref as R  # noqa: E402
from tests.fused_train_harness import MARGIN, SENTINEL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    import torch
    return torch.device("cuda", 0)


def kernel_loss_grad(model, states, values, rows, B):
    """mcn_sarl_loss_grad on device tensors (states [M,N,D], values [M,1], rows [B] int64 or None) with the float32
    weights of `model` -> (loss, flat gradient as numpy, loss bits).  The outputs start as a sentinel."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = _dev()
    N, D = int(states.shape[1]), int(states.shape[2])
    count = int(_hip.lib.mcn_sarl_train_param_count(D))
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dev, torch.float32).contiguous()
    assert params.numel() == count
    ws = torch.empty(int(_hip.lib.mcn_sarl_train_workspace_bytes(B, N, D)), dtype=torch.uint8, device=dev)
    grad = torch.full((count,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    rows_dev = None if rows is None else rows.to(dev, torch.long).contiguous()
    assert rows is None or (rows_dev.numel() == B and int(rows_dev.min()) >= 0 and int(rows_dev.max()) < states.shape[0])
    assert rows is not None or B <= states.shape[0]
    _hip.check(_hip.lib.mcn_sarl_loss_grad(_hip.ptr(params), D, _hip.ptr(states), _hip.ptr(values), _hip.ptr(rows_dev), B, N,
                                           _hip.ptr(ws), _hip.ptr(grad), _hip.ptr(loss), _hip.stream_ptr(dev)),
               "mcn_sarl_loss_grad")
    torch.cuda.synchronize()
    return float(loss.item()), grad.cpu().numpy(), loss.cpu().numpy().view(np.uint32)[0]


def _three_ways(model, states, values, rows, B):
    """(kernel, torch float32 on the GPU, float64 on the CPU), each (loss, flat gradient), on the same batch."""
    import copy
    import torch
    dev = _dev()
    pick = torch.arange(B) if rows is None else rows
    k_loss, k_grad, _ = kernel_loss_grad(model, states.to(dev), values.to(dev), rows, B)
    t_loss, t_grad = R.loss_and_grad(copy.deepcopy(model).to(dev), states[pick].to(dev), values[pick].to(dev))
    d_loss, d_grad = R.loss_and_grad64(model, states[pick], values[pick])
    return (k_loss, k_grad), (t_loss, t_grad), (d_loss, d_grad)


def _assert_parity(what, kernel, torch32, ref64, D):
    bad = F.parity(what, kernel, torch32, ref64, R.layout(D))
    assert not bad, "\n".join(bad)


SHAPES = [(1, 1), (1, 2), (1, 5), (3, 2), (5, 3), (3, 4), (7, 5), (100, 5), (33, 10), (2, 20), (2, 21), (2, 32)]


@pytest.mark.parametrize("input_dim", [13, 61])
@pytest.mark.parametrize("B,N", SHAPES)
def test_gradient_parity_with_float64(B, N, input_dim):
    """Loss and gradient of one mini-batch against float64 autograd, for two weight seeds, with the batch as rows
    0 .. B-1 (rows = NULL) and as a shuffled, non-contiguous index list into a memory of B + 9 rows.  Shapes: one state
    of one human, a group that is not full, several states per workgroup with a short last group (1 x 2, 3 x 2, 5 x 3,
    3 x 4: the grouping this kernel shares with the world model's), several workgroups with a short last one (7 x 5,
    100 x 5), one state per workgroup (33 x 10), both sides of the LDS / workspace threshold of the float64 row buffers
    (20 | 21) and the largest crowd (2 x 32).

    Bound: MARGIN = 4 times the error of torch's float32 autograd on the GPU on the same inputs, per parameter tensor
    and for the loss.

    Measured on an MI355X (table in DESIGN.md 3.6).  Worst parameter tensor among those that have a gradient: kernel
    2.4e-07 .. 6.4e-06, torch 6.2e-07 .. 3.2e-05 over the shapes; loss: kernel 1.7e-08 .. 5.5e-08, torch 3.4e-08 .. 1.5e-07,
    the kernel's never above torch's.  The bound holds in all 56 runs.  The three single numbers are what a float32
    forward pass misses it on (it is then a comparison of two roundings of equal size): the loss and mlp3.6.bias, which
    the kernel forms from a float64 forward pass, and attention.4.bias, which has no gradient (a common shift of the
    scores does not move the softmax: float64 gives 0 or 1e-19 of noise) and which the kernel returns as exactly 0."""
    import torch
    bad = []
    for seed in (0, 1):
        model = R.value_network(input_dim, seed)
        states, values = R.states_and_values(B + 9, N, input_dim, seed=100 + seed)
        shuffled = torch.randperm(B + 9, generator=torch.Generator().manual_seed(seed))[:B]
        for rows in (None, shuffled):
            what = "B %d N %d D %d seed %d rows %s" % (B, N, input_dim, seed, "NULL" if rows is None else "shuffled")
            bad += F.parity(what, *_three_ways(model, states, values, rows, B), R.layout(input_dim))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,N,input_dim", [(100, 5, 13), (33, 10, 61), (2, 32, 13)])
def test_two_calls_give_the_same_bits(B, N, input_dim):
    """No atomics, a fixed summation order: the same inputs give the same gradient and loss bits."""
    import torch
    model = R.value_network(input_dim, 0)
    states, values = R.states_and_values(B + 9, N, input_dim, seed=7)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(2))[:B]
    a = kernel_loss_grad(model, states.to(_dev()), values.to(_dev()), rows, B)
    b = kernel_loss_grad(model, states.to(_dev()), values.to(_dev()), rows, B)
    assert a[2] == b[2] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.isfinite(a[1]).all() and not (a[1] == SENTINEL).any()


@pytest.mark.parametrize("B,N", [(7, 5), (3, 2)])
def test_all_zero_scores_are_nan_where_torch_is(B, N):
    """attention.4 zeroed: every score is exactly 0, the masked softmax is 0 / 0.  Loss and gradient are NaN exactly
    where torch's float32 autograd has NaN; what is left (units behind a ReLU that is off in every row) is exactly 0."""
    import torch
    model = R.value_network(13, 0)
    with torch.no_grad():
        model.attention[4].weight.zero_()
        model.attention[4].bias.zero_()
    states, values = R.states_and_values(B, N, 13, seed=11)
    kernel, torch32, _ = _three_ways(model, states, values, None, B)
    assert np.isnan(kernel[0]) and np.isnan(torch32[0])
    assert np.isnan(torch32[1]).any()
    assert np.array_equal(np.isnan(kernel[1]), np.isnan(torch32[1]))
    keep = ~np.isnan(torch32[1])
    assert np.array_equal(kernel[1][keep], torch32[1][keep]) and not kernel[1][keep].any()


def test_dead_relu_layer_stops_the_gradient_exactly():
    """mlp1.2 with a large negative bias: its ReLU is off everywhere, so mlp1.2 and mlp1.0 below it get exactly 0, as
    from torch; the layers above keep the parity bound."""
    import torch
    B, N, D = 7, 5, 13
    model = R.value_network(D, 1)
    with torch.no_grad():
        model.mlp1[2].bias.fill_(-1e4)
    states, values = R.states_and_values(B, N, D, seed=12)
    kernel, torch32, ref64 = _three_ways(model, states, values, None, B)
    table, _ = R.layout(D)
    below = [(k, off, shp) for k, off, shp in table if k.startswith("mlp1.")]
    assert len(below) == 4
    for k, off, shp in below:
        n = int(np.prod(shp))
        assert not kernel[1][off:off + n].any() and not torch32[1][off:off + n].any() and not ref64[1][off:off + n].any(), k
    lo = below[-1][1] + int(np.prod(below[-1][2]))
    assert np.isfinite(kernel[1]).all() and np.abs(kernel[1][lo:]).max() > 0
    _assert_parity("dead mlp1.2", kernel, torch32, ref64, D)


def test_sgd_momentum_kernel_is_torchs_rule():
    """Five steps from a zero buffer against torch.optim.SGD(momentum=0.9) on a flat device tensor (a count that is no
    multiple of the workgroup, several workgroups).  The kernel forms buf = momentum buf + grad in two roundings, as
    torch's mul_ then add_, and p - lr buf as ONE fused multiply-add, as torch's add_(buf, alpha=-lr): so the bound
    is "1 ulp per element", the one for a kernel that uses an FMA.  The test prints how many elements differ at all
    (measured on an MI355X: none, in parameters and momentum, at every step)."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = _dev()
    count, lr, momentum = 96502 + 3, 0.01, 0.9
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(count, generator=g)
    grads = [torch.randn(count, generator=g) for _ in range(5)]
    want = p0.clone().to(dev).requires_grad_(True)
    opt = torch.optim.SGD([want], lr=lr, momentum=momentum)
    p, buf = p0.clone().to(dev), torch.zeros(count, device=dev)
    for s, gr in enumerate(grads):
        gd = gr.to(dev)
        want.grad = gd.clone()
        opt.step()
        _hip.check(_hip.lib.mcn_sgd_momentum_step(_hip.ptr(p), _hip.ptr(buf), _hip.ptr(gd), count, lr, momentum,
                                                  _hip.stream_ptr(dev)), "mcn_sgd_momentum_step")
        torch.cuda.synchronize()
        wp, wb = want.detach().cpu().numpy(), opt.state[want]["momentum_buffer"].cpu().numpy()
        up, ub = F.ulps(p.cpu().numpy(), wp), F.ulps(buf.cpu().numpy(), wb)
        print("step %d: params differ in %d of %d elements (max %.2f ulp), momentum in %d (max %.2f ulp)" %
              (s, int((up > 0).sum()), count, up.max(), int((ub > 0).sum()), ub.max()))
        assert up.max() <= 1.0 and ub.max() <= 1.0
    assert not torch.equal(p.cpu(), p0)


def _load_g10(mode, golden_dir, fused):
    import torch
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    from tests.test_training_cpu import _load_sd, _model
    g = np.load(os.path.join(golden_dir, "g10_trainer.npz"))
    model = _model(seed=3)
    _load_sd(model, g, "w0__")
    states, values = torch.from_numpy(g[mode + "_states"]), torch.from_numpy(g[mode + "_values"])
    mem = ReplayMemory(states.shape[0], device=_dev())
    mem.push_batch(states.to(_dev()), values.reshape(-1).to(_dev()))
    tr = Trainer(model.to(_dev()), mem, _dev(), 100, fused=fused)
    return g, model, states, values.reshape(-1, 1), tr


@pytest.mark.parametrize("mode", ["batch", "epoch"])
def test_fused_trainer_matches_reference_trainer(mode, golden_dir):
    """The scenario of tests/test_training_cpu.py::check_trainer_against_reference (g10_trainer.npz: the REFERENCE's own
    float32 Trainer; lr 0.01; `batch`: three optimize_batch(1) over a one-batch memory, `epoch`: two optimize_epoch(1)
    over a two-batch memory with the recorded permutations) with fused=True on the device.  Weights and losses are
    compared with the float64 replay of the same steps; the bound is MARGIN = 4 times the fixture's own distance from
    that replay, per parameter tensor (max |w - w64|) and over the returned losses (max |loss - loss64|)."""
    import torch
    g, model, states, values, tr = _load_g10(mode, golden_dir, fused=True)
    start = R.as64(model).float()
    tr.set_learning_rate(0.01)
    batches = []
    if mode == "batch":
        got = []
        for _ in range(3):
            got.append(tr.optimize_batch(1))
            batches += [b.clone() for b in tr.last_rows]
        assert all(sorted(b.tolist()) == list(range(100)) for b in batches)
    else:
        got = [tr.optimize_epoch(1, perms=g["epoch_perms"][i:i + 1]) for i in range(2)]
        for i in range(2):
            batches += [torch.from_numpy(g["epoch_perms"][i][lo:lo + 100].astype(np.int64)) for lo in (0, 100)]
        assert [b.tolist() for b in tr.last_rows] == [b.tolist() for b in batches[2:]]
    losses64, m64, _ = R.sgd64(start, states, values, batches, lr=0.01)
    if mode == "batch":
        want = losses64
    else:
        want = [(losses64[0] + losses64[1]) / 200, (losses64[2] + losses64[3]) / 200]
    fixture_loss = float(np.abs(np.asarray(g[mode + "_losses"], np.float64) - want).max())
    fused_loss = float(np.abs(np.asarray(got, np.float64) - want).max())
    print("mode %s: max |loss - loss64| fused %.3g, fixture %.3g" % (mode, fused_loss, fixture_loss))
    assert fused_loss <= MARGIN * fixture_loss
    sd64, worst = m64.state_dict(), 0.0
    for k, v in model.state_dict().items():
        w64 = sd64[k].numpy()
        d_fix = float(np.abs(g[mode + "_w1__" + k.replace(".", "__")].astype(np.float64) - w64).max())
        d_fused = float(np.abs(v.cpu().numpy().astype(np.float64) - w64).max())
        worst = max(worst, d_fused / d_fix if d_fix > 0 else 0.0)       # (attention.4.bias does not move at all)
        assert d_fused <= MARGIN * d_fix, (k, d_fused, d_fix)
    print("mode %s: worst max |w - w64| fused / fixture = %.3g" % (mode, worst))


def test_fused_and_torch_paths_train_on_the_same_batches(monkeypatch):
    """From the same weights and the same generator seed, optimize_batch(3) then optimize_epoch(1) (250 rows, batch 100:
    the epoch ends on a short batch) draw the same permutations on both paths -- captured at torch.randperm -- and the
    fused path's rows are their slices.  Weights: with d = max |w_torch - w64| per tensor against the float64 replay of
    those batches, the fused path may be MARGIN d from the replay (the bound of the tests above), so the two paths
    may differ by d + MARGIN d (triangle inequality)."""
    import copy
    import torch
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    dev = _dev()
    model0 = R.value_network(13, 2)
    states, values = R.states_and_values(250, 5, 13, seed=21)
    drawn = []
    real = torch.randperm

    def recording(n, *a, **kw):
        out = real(n, *a, **kw)
        drawn.append(out.clone())
        return out
    monkeypatch.setattr(torch, "randperm", recording)
    result = {}
    for fused in (False, True):
        del drawn[:]
        model = copy.deepcopy(model0).to(dev)
        mem = ReplayMemory(300, device=dev)
        mem.push_batch(states.to(dev), values.reshape(-1).to(dev))
        tr = Trainer(model, mem, dev, 100, fused=fused)
        tr._gen.manual_seed(77)
        tr.set_learning_rate(0.01)
        l1 = tr.optimize_batch(3)
        rows = [b.clone() for b in tr.last_rows] if fused else None
        l2 = tr.optimize_epoch(1)
        rows = rows + [b.clone() for b in tr.last_rows] if fused else None
        result[fused] = ([d.clone() for d in drawn], rows, [l1, l2], {k: v.cpu().numpy() for k, v in model.state_dict().items()})
    perms_t, _, losses_t, w_t = result[False]
    perms_f, rows_f, losses_f, w_f = result[True]
    assert len(perms_t) == len(perms_f) == 4 and all(torch.equal(a, b) for a, b in zip(perms_t, perms_f))
    batches = [p[:100] for p in perms_t[:3]] + [perms_t[3][lo:lo + 100] for lo in (0, 100, 200)]
    assert [b.numel() for b in batches] == [100] * 5 + [50]
    assert len(rows_f) == 6 and all(torch.equal(a, b) for a, b in zip(rows_f, batches))
    _, m64, _ = R.sgd64(model0, states, values, batches, lr=0.01)
    for k, w64 in m64.state_dict().items():
        d = float(np.abs(w_t[k].astype(np.float64) - w64.numpy()).max())
        gap = float(np.abs(w_t[k].astype(np.float64) - w_f[k].astype(np.float64)).max())
        assert gap <= (1 + MARGIN) * d, (k, gap, d)
    print("losses torch %r fused %r" % (losses_t, losses_f))


def test_fused_step_writes_back_and_reads_the_module():
    """After a fused optimize_batch the SARL look-ahead runs on the trained weights: predict_batch gives the bits of a
    fresh policy loaded with the trained state_dict (the packed weights were re-made: every parameter's version
    moved).  load_state_dict between two fused calls is honoured; set_learning_rate starts the momentum over: the first
    step after it is the plain gradient step p - lr g of the kernel's own gradient (momentum buffer == g bit for bit;
    p to 1 ulp: the check rounds a float64 product once more than the kernel's fused multiply-add)."""
    import torch
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    from tests import helpers as H
    from tests import lookahead_harness as L
    dev = _dev()
    rng = np.random.RandomState(17)
    E, N = 16, 5
    pol = L.policy("sarl", seed=21)
    env = H.make_vec_env(E, N)
    H.upload(env, H.random_state(rng, E, N))
    mem = ReplayMemory(64, device=dev)
    rows = pol.transform_batch(env)
    mem.push_batch(rows, torch.from_numpy(rng.uniform(-1, 1, E).astype(np.float32)).to(dev))
    w0 = {k: v.clone() for k, v in pol.model.state_dict().items()}
    _, _, v0 = pol.predict_batch(env, want_values=True)
    v0 = v0.cpu().numpy().copy()
    tr = Trainer(pol.model, mem, dev, batch_size=8, fused=True)
    tr._gen.manual_seed(1)
    tr.set_learning_rate(0.01)
    stamp0 = _hip.weights_stamp(list(pol.model.parameters()), dev)
    tr.optimize_batch(2)
    stamp1 = _hip.weights_stamp(list(pol.model.parameters()), dev)
    assert all(a[2] != b[2] for a, b in zip(stamp0[:-1], stamp1[:-1])), "a parameter's version counter did not move"
    w1 = {k: v.clone() for k, v in pol.model.state_dict().items()}
    # (attention.4.bias shifts every score alike, which the softmax does not see: its gradient is rounding noise)
    assert all(not torch.equal(w0[k], w1[k]) for k in w0 if k != "attention.4.bias")
    _, _, v1 = pol.predict_batch(env, want_values=True)
    v1 = v1.cpu().numpy().copy()
    fresh = L.policy("sarl", weights={k: v.cpu() for k, v in w1.items()})
    _, _, v2 = fresh.predict_batch(env, want_values=True)
    assert np.array_equal(v1, v2.cpu().numpy()) and not np.array_equal(v0, v1)

    # load_state_dict is honoured: back at w0 with the same draws and a fresh momentum, the same two steps give w1 again
    pol.model.load_state_dict(w0)
    tr._gen.manual_seed(1)
    tr.set_learning_rate(0.01)
    tr.optimize_batch(2)
    assert all(torch.equal(w1[k], v) for k, v in pol.model.state_dict().items())

    # set_learning_rate resets the momentum
    tr.set_learning_rate(0.02)
    before = torch.cat([p.detach().reshape(-1) for p in pol.model.parameters()]).cpu().numpy()
    import copy
    frozen = copy.deepcopy(pol.model)
    tr.optimize_batch(1)
    batch = tr.last_rows[0]
    _, grad, _ = kernel_loss_grad(frozen, mem._states, mem._values, batch, int(batch.numel()))
    assert np.array_equal(tr._fz["mom"].cpu().numpy().view(np.uint32), grad.view(np.uint32))
    after = torch.cat([p.detach().reshape(-1) for p in pol.model.parameters()]).cpu().numpy()
    want = (before.astype(np.float64) - np.float64(np.float32(0.02)) * grad.astype(np.float64)).astype(np.float32)
    assert F.ulps(after, want).max() <= 1.0 and not np.array_equal(after, before)


def test_fused_trainer_in_a_process_group_of_one(tmp_path):
    """Data parallel: with an initialised process group the flat gradient is the all-reduce bucket.  A fresh child
    process (tests/fused_dp_worker.py) trains once without a group and once, from the same weights and draws, inside a
    world-size-1 `nccl` (= RCCL) group: the same bits."""
    import torch
    port = 33700 + (os.getpid() % 1500)
    out = str(tmp_path / "fused_dp.pt")
    res = subprocess.run([sys.executable, "-m", "tests.fused_dp_worker", str(port), "nccl", out], cwd=ROOT,
                         env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    r = torch.load(out, weights_only=True)
    assert r["backend"] == "nccl" and r["world"] == 1 and r["bucket_is_grad"]
    assert r["losses_alone"] == r["losses_grouped"] and all(np.isfinite(r["losses_alone"]))
    for k, v in r["alone"].items():
        assert torch.equal(v, r["grouped"][k]), k
        assert k == "attention.4.bias" or not torch.equal(v, r["start"][k]), k     # (its gradient is rounding noise)
