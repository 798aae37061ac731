"""GPU: the fused training steps of the value networks -- SARL and OM-SARL (csrc/sarl_train.hip), LSTM-RL and CADRL
(csrc/value_train.hip) -- through mcn_<policy>_loss_grad / mcn_sgd_momentum_step and Trainer(fused=True), against the
float64 yardstick of tests/value_trainer_ref.py.  Every bound is a multiple of what torch's own float32 path (or the
reference's recorded float32 Trainer) is away from that yardstick on the same inputs; nothing is compared with an earlier
output of the kernel."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fused_train_harness as F  # noqa: E402
from tests import value_trainer_ref as R  # noqa: E402
from tests.fused_train_harness import MARGIN, SENTINEL  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SARL: one state of one human, a group that is not full, several states per workgroup with a short last group (1 x 2,
# 3 x 2, 5 x 3, 3 x 4: the grouping this kernel shares with the world model's), several workgroups with a short last one
# (7 x 5, 100 x 5), one state per workgroup (33 x 10), both sides of the LDS / workspace threshold of the float64 row
# buffers (20 | 21) and the largest crowd (2 x 32)
SARL_SHAPES = [(1, 1), (1, 2), (1, 5), (3, 2), (5, 3), (3, 4), (7, 5), (100, 5), (33, 10), (2, 20), (2, 21), (2, 32)]
# every crowd's activations fit LDS, so the LSTM-RL kernel has no LDS / workspace threshold; its paths are the grouping's:
# several states per workgroup with a short last group (N <= 4: 1 x 2, 3 x 2, 5 x 3, 3 x 4), one state per workgroup above
LSTM_SHAPES = [(1, 1), (1, 2), (3, 2), (5, 3), (3, 4), (7, 5), (100, 5), (33, 10), (2, 32)]
CADRL_SHAPES = [(B, 1) for B in (1, 3, R.CADRL_G, R.CADRL_G + 1, 100, 257)]
CASES = ([(p, B, N) for B, N in SARL_SHAPES for p in ("sarl", "sarl_om")] + [("lstm_rl", B, N) for B, N in LSTM_SHAPES] +
         [("cadrl", B, N) for B, N in CADRL_SHAPES])
HEAD = {"sarl": "mlp3", "lstm_rl": "mlp", "cadrl": "value_network"}     # the 150-100-100-1 MLP's state_dict prefix


def _dev():
    import torch
    return torch.device("cuda", 0)


def kernel_loss_grad(policy, model, states, values, rows, B):
    """mcn_<policy>_loss_grad on device tensors (states [M,N,D] or, for CADRL, [M,13]; values [M,1]; rows [B] int64 or
    None) with the float32 weights of `model` -> (loss, flat gradient as numpy, loss bits).  The outputs start as a
    sentinel."""
    import torch
    from modelcrowdnav_amd import _hip
    dev, lib = _dev(), _hip.lib
    D, count = R.INPUT_DIM[policy], R.COUNT[policy]
    name = "sarl" if policy == "sarl_om" else policy
    extra = (D,) if name == "sarl" else ()              # SARL's entry points take the input width
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dev, torch.float32).contiguous()
    assert params.numel() == count == int(getattr(lib, "mcn_%s_train_param_count" % name)(*extra))
    assert states.is_contiguous() and values.is_contiguous() and tuple(states.shape[-1:]) == (D,)
    grad = torch.full((count,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    rows_dev = None if rows is None else rows.to(dev, torch.long).contiguous()
    assert rows is None or (rows_dev.numel() == B and int(rows_dev.min()) >= 0 and int(rows_dev.max()) < states.shape[0])
    assert rows is not None or B <= states.shape[0]
    batch = (_hip.ptr(states), _hip.ptr(values), _hip.ptr(rows_dev), B)
    if policy == "cadrl":
        assert states.dim() == 2
        ws = torch.empty(int(lib.mcn_cadrl_train_workspace_bytes(B)), dtype=torch.uint8, device=dev)
        rc = lib.mcn_cadrl_loss_grad(_hip.ptr(params), *batch, _hip.ptr(ws), _hip.ptr(grad), _hip.ptr(loss), _hip.stream_ptr(dev))
    else:
        assert states.dim() == 3 and 1 <= states.shape[1] <= _hip.MAX_HUMANS
        N = int(states.shape[1])
        ws = torch.empty(int(getattr(lib, "mcn_%s_train_workspace_bytes" % name)(B, N, *extra)), dtype=torch.uint8, device=dev)
        rc = getattr(lib, "mcn_%s_loss_grad" % name)(_hip.ptr(params), *extra, *batch, N, _hip.ptr(ws), _hip.ptr(grad),
                                                     _hip.ptr(loss), _hip.stream_ptr(dev))
    assert ws.numel() > 0
    _hip.check(rc, "mcn_%s_loss_grad" % name)
    torch.cuda.synchronize()
    return float(loss.item()), grad.cpu().numpy(), loss.cpu().numpy().view(np.uint32)[0]


def _three_ways(policy, model, states, values, rows, B):
    """(kernel, torch float32 on the GPU, float64 on the CPU), each (loss, flat gradient), on the same batch."""
    import torch
    dev = _dev()
    pick = torch.arange(B) if rows is None else rows
    k_loss, k_grad, _ = kernel_loss_grad(policy, model, states.to(dev), values.to(dev), rows, B)
    t_loss, t_grad = R.loss_and_grad(copy.deepcopy(model).to(dev), states[pick].to(dev), values[pick].to(dev))
    d_loss, d_grad = R.loss_and_grad64(model, states[pick], values[pick])
    return (k_loss, k_grad), (t_loss, t_grad), (d_loss, d_grad)


def _slot(policy, name):
    off, n = F.slot(R.layout(policy), name)
    return slice(off, off + n)


def _same_lstm_biases(policy, grad):
    """The two LSTM biases are the same sum, formed twice in the same order: the same bits."""
    return policy != "lstm_rl" or np.array_equal(grad[_slot(policy, "lstm.bias_ih_l0")].view(np.uint32),
                                                 grad[_slot(policy, "lstm.bias_hh_l0")].view(np.uint32))


@pytest.mark.parametrize("policy,B,N", CASES)
def test_gradient_parity_with_float64(policy, B, N):
    """Loss and gradient of one mini-batch against float64 autograd, for two weight seeds, with the batch as rows
    0 .. B-1 (rows = NULL) and as a shuffled, non-contiguous index list into a memory of B + 9 rows.  The shapes of SARL
    (input_dim 13) and OM-SARL (61) and of LSTM-RL are explained at their lists above; LSTM-RL's one state of one step has
    h_0 = 0, so lstm.weight_hh_l0 gets exactly 0.  CADRL: one state, a short group, a full group (8), one more, several
    workgroups with a short last one.

    Bound (tests/value_trainer_ref.py: parity): per parameter tensor MARGIN = 4 times the error of torch's float32 autograd
    on the GPU on the same inputs; SARL's loss too; LSTM-RL's and CADRL's loss and one-element last bias within that, or
    within 1 float32 ulp of float64.

    Measured on an MI355X (tables in DESIGN.md 3.6 and 3.6b; the test prints both sides' figures per case).  SARL, worst
    parameter tensor among those that have a gradient: kernel 2.4e-07 .. 6.4e-06, torch 6.2e-07 .. 3.2e-05 over the shapes;
    loss: kernel 1.7e-08 .. 5.5e-08, torch 3.4e-08 .. 1.5e-07, the kernel's never above torch's.  The bound holds in all 56
    runs.  The three single numbers are what a float32 forward pass misses it on (it is then a comparison of two roundings
    of equal size): the loss and mlp3.6.bias, which the kernel forms from a float64 forward pass, and attention.4.bias,
    which has no gradient (a common shift of the scores does not move the softmax: float64 gives 0 or 1e-19 of noise) and
    which the kernel returns as exactly 0.  Worst parameter tensor of LSTM-RL: kernel 1.4e-07 .. 3.8e-07, torch 2.5e-07 ..
    7.6e-07; CADRL kernel 8.8e-08 .. 2.4e-07, torch 2.3e-07 .. 6.6e-07; loss: kernel 2.1e-10 .. 4.7e-08, torch 2.1e-10 ..
    1.5e-07.  The bound holds in all 60 runs; the kernel's worst tensor is above torch's in one of them (CADRL B = 9:
    2.43e-07 against 2.27e-07)."""
    import torch
    bad = []
    for seed in (0, 1):
        model = R.value_network(policy, seed)
        states, values = R.states_and_values(policy, B + 9, N, seed=100 + seed)
        shuffled = torch.randperm(B + 9, generator=torch.Generator().manual_seed(seed))[:B]
        for rows in (None, shuffled):
            what = "%s B %d N %d seed %d rows %s" % (policy, B, N, seed, "NULL" if rows is None else "shuffled")
            kernel, torch32, ref64 = _three_ways(policy, model, states, values, rows, B)
            bad += R.parity(what, policy, kernel, torch32, ref64)
            assert _same_lstm_biases(policy, kernel[1]), what
            if policy == "lstm_rl" and N == 1:
                whh = _slot(policy, "lstm.weight_hh_l0")
                assert not ref64[1][whh].any() and not kernel[1][whh].any(), what
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("policy,B,N", [("sarl", 100, 5), ("sarl_om", 33, 10), ("sarl", 2, 32), ("lstm_rl", 100, 5),
                                        ("lstm_rl", 33, 10), ("lstm_rl", 2, 32), ("cadrl", 100, 1), ("cadrl", 257, 1)])
def test_two_calls_give_the_same_bits(policy, B, N):
    """No atomics, a fixed summation order: the same inputs give the same gradient and loss bits; every element is
    written and finite; the two LSTM biases, which are the same sum, have the same bits."""
    import torch
    model = R.value_network(policy, 0)
    states, values = R.states_and_values(policy, B + 9, N, seed=7)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(2))[:B]
    a = kernel_loss_grad(policy, model, states.to(_dev()), values.to(_dev()), rows, B)
    b = kernel_loss_grad(policy, model, states.to(_dev()), values.to(_dev()), rows, B)
    assert a[2] == b[2] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.isfinite(a[1]).all() and np.isfinite(a[0]) and not (a[1] == SENTINEL).any() and a[0] != SENTINEL
    assert _same_lstm_biases(policy, a[1])
    if policy == "lstm_rl":
        assert a[1][_slot(policy, "lstm.bias_ih_l0")].any()


@pytest.mark.parametrize("B,N", [(7, 5), (3, 2)])
def test_all_zero_scores_are_nan_where_torch_is(B, N):
    """attention.4 zeroed: every score is exactly 0, the masked softmax is 0 / 0.  Loss and gradient are NaN exactly
    where torch's float32 autograd has NaN; what is left (units behind a ReLU that is off in every row) is exactly 0."""
    import torch
    model = R.value_network("sarl", 0)
    with torch.no_grad():
        model.attention[4].weight.zero_()
        model.attention[4].bias.zero_()
    states, values = R.states_and_values("sarl", B, N, seed=11)
    kernel, torch32, _ = _three_ways("sarl", model, states, values, None, B)
    assert np.isnan(kernel[0]) and np.isnan(torch32[0])
    assert np.isnan(torch32[1]).any()
    assert np.array_equal(np.isnan(kernel[1]), np.isnan(torch32[1]))
    keep = ~np.isnan(torch32[1])
    assert np.array_equal(kernel[1][keep], torch32[1][keep]) and not kernel[1][keep].any()


@pytest.mark.parametrize("policy", sorted(HEAD))
def test_dead_relu_layer_stops_the_gradient_exactly(policy):
    """A layer with a large negative bias -- SARL: mlp1.2; LSTM-RL and CADRL: the second layer of the MLP -- has its ReLU
    off everywhere, so that layer and everything below it (SARL: mlp1.0; the MLP's first layer and, for LSTM-RL, all four
    LSTM tensors) get exactly 0 from the kernel, torch float32 and float64 alike; the layers above keep the parity bound
    and the last ones of the MLP have a gradient."""
    import torch
    B, N = 7, 5
    model = R.value_network(policy, 1)
    head = HEAD[policy]
    dead, prefixes = ("mlp1", ("mlp1.",)) if policy == "sarl" else (head, (head + ".0.", head + ".2.", "lstm."))
    with torch.no_grad():
        getattr(model, dead)[2].bias.fill_(-1e4)
    states, values = R.states_and_values(policy, B, N, seed=12)
    kernel, torch32, ref64 = _three_ways(policy, model, states, values, None, B)
    below = [k for k, _, _ in R.layout(policy)[0] if k.startswith(prefixes)]
    assert len(below) == (8 if policy == "lstm_rl" else 4)
    for k in below:
        s = _slot(policy, k)
        assert not kernel[1][s].any() and not torch32[1][s].any() and not ref64[1][s].any(), k
    assert np.isfinite(kernel[1]).all()
    for k in (head + ".4.bias", head + ".6.weight", head + ".6.bias"):
        assert np.abs(kernel[1][_slot(policy, k)]).max() > 0, k
    bad = R.parity("dead %s.2" % dead, policy, kernel, torch32, ref64)
    assert not bad, "\n".join(bad)


def test_saturated_gates_stay_finite():
    """LSTM weights scaled by 1000: the gates' pre-activations reach +-1000 (asserted), where exp overflows in float32
    and in a careless float64 sigmoid gives inf / inf.  Loss and gradient are finite wherever torch's float32 autograd on
    the CPU is finite, and the loss keeps the parity bound against float64."""
    import torch
    B, N = 3, 3
    model = R.value_network("lstm_rl", 0)
    with torch.no_grad():
        for p in model.lstm.parameters():
            p.mul_(1000.0)
    states, values = R.states_and_values("lstm_rl", B, N, seed=5)
    with torch.no_grad():
        pre = states.reshape(-1, 13).double() @ model.lstm.weight_ih_l0.double().T
    assert float(pre.max()) > 1000 and float(pre.min()) < -1000
    k_loss, k_grad, _ = kernel_loss_grad("lstm_rl", model, states.to(_dev()), values.to(_dev()), None, B)
    c_loss, c_grad = R.loss_and_grad(model, states, values)                     # torch float32 on the CPU
    d_loss, _ = R.loss_and_grad64(model, states, values)
    print("saturated: loss kernel %.9g torch cpu %.9g float64 %.17g; finite elements kernel %d torch cpu %d of %d" %
          (k_loss, c_loss, d_loss, np.isfinite(k_grad).sum(), np.isfinite(c_grad).sum(), k_grad.size))
    assert np.isfinite(c_loss) and np.isfinite(k_loss)
    assert np.isfinite(k_grad[np.isfinite(c_grad)]).all() and np.isfinite(c_grad).any()
    assert abs(k_loss - d_loss) <= MARGIN * abs(c_loss - d_loss) or R.ulps(np.float32([k_loss]), np.float64([d_loss])).max() <= 1


def test_nan_goes_where_torchs_goes():
    """One NaN in column 7 of the second human row of one state: the loss is NaN and the gradient's NaN mask is that of
    torch's float32 autograd on the CPU (the composite LSTM formulas).  Whether torch on the GPU (MIOpen's LSTM) agrees is
    printed, not asserted."""
    B, N = 3, 3
    model = R.value_network("lstm_rl", 0)
    states, values = R.states_and_values("lstm_rl", B, N, seed=6)
    states[1, 1, 7] = float("nan")
    kernel, torch_gpu, _ = _three_ways("lstm_rl", model, states, values, None, B)
    c_loss, c_grad = R.loss_and_grad(model, states, values)
    print("NaN elements: kernel %d, torch cpu %d, torch gpu %d of %d; torch gpu mask == torch cpu mask: %s" %
          (np.isnan(kernel[1]).sum(), np.isnan(c_grad).sum(), np.isnan(torch_gpu[1]).sum(), c_grad.size,
           np.array_equal(np.isnan(torch_gpu[1]), np.isnan(c_grad))))
    assert np.isnan(kernel[0]) and np.isnan(c_loss) and np.isnan(c_grad).any()
    assert np.array_equal(np.isnan(kernel[1]), np.isnan(c_grad))
    assert not (kernel[1] == SENTINEL).any()


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


@pytest.mark.parametrize("run", ["batch", "epoch", "lstm_rl", "cadrl"])
def test_fused_trainer_matches_reference_trainer(run, golden_dir):
    """The recorded runs of the REFERENCE's own float32 Trainer on its own networks, lr 0.01, with fused=True on the
    device.  `batch` and `epoch`: SARL, the scenario of tests/test_training_cpu.py::check_trainer_against_reference
    (g10_trainer.npz; three optimize_batch(1) over a one-batch memory; two optimize_epoch(1) over a two-batch memory with
    the recorded permutations).  `lstm_rl` and `cadrl`: tests/golden/g26_value_trainers.npz, three optimize_batch(1) over
    a one-batch memory.  Weights and losses are compared with the float64 replay of the same steps; the bound is MARGIN =
    4 times the fixture's own distance from that replay, per parameter tensor (max |w - w64|) and over the returned losses
    (max |loss - loss64|)."""
    import torch
    if run in ("batch", "epoch"):
        g, model, states, values, tr = _load_g10(run, golden_dir, fused=True)
    else:
        from tests.test_fused_value_trainers_cpu import load_g26
        g, model, states, values, tr = load_g26(run, golden_dir, _dev(), fused=True)
    start = R.as64(model).float()
    tr.set_learning_rate(0.01)
    got, batches = [], []
    if run == "epoch":
        got = [tr.optimize_epoch(1, perms=g["epoch_perms"][i:i + 1]) for i in range(2)]
        for i in range(2):
            batches += [torch.from_numpy(g["epoch_perms"][i][lo:lo + 100].astype(np.int64)) for lo in (0, 100)]
        assert [b.tolist() for b in tr.last_rows] == [b.tolist() for b in batches[2:]]
    else:
        for _ in range(3):
            got.append(tr.optimize_batch(1))
            batches += [b.clone() for b in tr.last_rows]
        assert len(batches) == 3 and all(sorted(b.tolist()) == list(range(100)) for b in batches)
    want, m64, _ = R.sgd64(start, states, values, batches, lr=0.01)
    if run == "epoch":
        want = [(want[0] + want[1]) / 200, (want[2] + want[3]) / 200]
    fixture_loss = float(np.abs(np.asarray(g[run + "_losses"], np.float64) - want).max())
    fused_loss = float(np.abs(np.asarray(got, np.float64) - want).max())
    print("%s: max |loss - loss64| fused %.3g, fixture %.3g" % (run, fused_loss, fixture_loss))
    assert fused_loss <= MARGIN * fixture_loss
    sd64, worst = m64.state_dict(), 0.0
    for k, v in model.state_dict().items():
        w64 = sd64[k].numpy()
        d_fix = float(np.abs(g["%s_w1__%s" % (run, k.replace(".", "__"))].astype(np.float64) - w64).max())
        d_fused = float(np.abs(v.cpu().numpy().astype(np.float64) - w64).max())
        worst = max(worst, d_fused / d_fix if d_fix > 0 else 0.0)       # (SARL's attention.4.bias does not move at all)
        assert d_fused <= MARGIN * d_fix, (k, d_fused, d_fix)
    print("%s: worst max |w - w64| fused / fixture = %.3g" % (run, worst))


@pytest.mark.parametrize("policy", sorted(HEAD))
def test_fused_and_torch_paths_train_on_the_same_batches(policy, monkeypatch):
    """From the same weights and the same generator seed, optimize_batch(3) then optimize_epoch(1) (250 rows, batch 100:
    the epoch ends on a short batch; N = 5 for SARL and LSTM-RL) draw the same permutations on both paths -- captured at
    torch.randperm -- and the fused path's rows are their slices.  Weights: with d = max |w_torch - w64| per tensor against
    the float64 replay of those batches, the fused path may be MARGIN d from the replay (the bound of the tests above),
    so the two paths may differ by d + MARGIN d (triangle inequality)."""
    import torch
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    dev = _dev()
    model0 = R.value_network(policy, 2)
    states, values = R.states_and_values(policy, 250, 5, seed=21)
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
        print("%s %s: |torch - float64| %.3g, |torch - fused| %.3g" % (policy, k, d, gap))
        assert gap <= (1 + MARGIN) * d, (k, gap, d)
    print("losses torch %r fused %r" % (losses_t, losses_f))


@pytest.mark.parametrize("policy,N", [("sarl", 5), ("lstm_rl", 5), ("cadrl", 1)])
def test_fused_step_writes_back_and_reads_the_module(policy, N):
    """After a fused optimize_batch the look-ahead runs on the trained weights: predict_batch gives the bits of a fresh
    policy loaded with the trained state_dict (the packed weights were re-made: every parameter's version moved).
    load_state_dict between two fused calls is honoured; set_learning_rate starts the momentum over: the first step after
    it is the plain gradient step p - lr g of the kernel's own gradient (momentum buffer == g bit for bit; p to 1 ulp: the
    check rounds a float64 product once more than the kernel's fused multiply-add)."""
    import torch
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    from tests import helpers as H
    from tests import lookahead_harness as L
    dev = _dev()
    rng = np.random.RandomState(17)
    E = 16
    pol = L.policy(policy, seed=21)
    env = H.make_vec_env(E, N)
    H.upload(env, H.random_state(rng, E, N))
    mem = ReplayMemory(64, device=dev)
    mem.push_batch(pol.transform_batch(env), torch.from_numpy(rng.uniform(-1, 1, E).astype(np.float32)).to(dev))
    assert tuple(mem._states.shape[1:]) == ((13,) if policy == "cadrl" else (N, 13))
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
    # (SARL's attention.4.bias shifts every score alike, which the softmax does not see: its gradient is rounding noise)
    assert all(not torch.equal(w0[k], w1[k]) for k in w0 if k != "attention.4.bias")
    _, _, v1 = pol.predict_batch(env, want_values=True)
    v1 = v1.cpu().numpy().copy()
    fresh = L.policy(policy, weights={k: v.cpu() for k, v in w1.items()})
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
    frozen = copy.deepcopy(pol.model)
    tr.optimize_batch(1)
    batch = tr.last_rows[0]
    _, grad, _ = kernel_loss_grad(policy, frozen, mem._states, mem._values, batch, int(batch.numel()))
    assert np.array_equal(tr._fz["mom"].cpu().numpy().view(np.uint32), grad.view(np.uint32)) and grad.any()
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
