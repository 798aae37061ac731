"""GPU: the fused AttentionWorld training step (csrc/world_train.hip through mcn_attn_world_loss_grad / mcn_adam_step and
Trainer_Sim(fused=True)) against the float64 yardstick of tests/world_trainer_ref.py.  Every bound is a multiple of what
torch's own float32 path (or the reference's recorded float32 Trainer_Sim) is away from that yardstick on the same
inputs; nothing is compared with an earlier output of the kernel."""
import copy
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fused_train_harness as F  # noqa: E402
from tests import world_trainer_ref as R  # noqa: E402
from tests.fused_train_harness import MARGIN, SENTINEL  # noqa: E402


def _dev():
    import torch
    return torch.device("cuda", 0)


def kernel_loss_grad(model, cur, nxt, rows, B, want_grad=True):
    """mcn_attn_world_loss_grad on device tensors (cur [M,4N], nxt [M,2N], rows [B] int64 or None) with the float32
    weights of `model` -> (loss, flat gradient as numpy, loss bits).  The outputs start as a sentinel; without
    want_grad the gradient pointer is NULL and the sentinel buffer comes back as it was left."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = _dev()
    N = int(cur.shape[1]) // 4
    assert cur.shape[1] == 4 * N and nxt.shape[1] == 2 * N and cur.is_contiguous() and nxt.is_contiguous()
    count = int(_hip.lib.mcn_attn_world_train_param_count())
    params = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).to(dev, torch.float32).contiguous()
    assert params.numel() == count
    ws = torch.empty(int(_hip.lib.mcn_attn_world_train_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    grad = torch.full((count,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    rows_dev = None if rows is None else rows.to(dev, torch.long).contiguous()
    assert rows is None or (rows_dev.numel() == B and int(rows_dev.min()) >= 0 and int(rows_dev.max()) < cur.shape[0])
    assert rows is not None or B <= cur.shape[0]
    _hip.check(_hip.lib.mcn_attn_world_loss_grad(_hip.ptr(params), _hip.ptr(cur), _hip.ptr(nxt), _hip.ptr(rows_dev), B, N,
                                                 _hip.ptr(ws), _hip.ptr(grad) if want_grad else None, _hip.ptr(loss),
                                                 _hip.stream_ptr(dev)), "mcn_attn_world_loss_grad")
    torch.cuda.synchronize()
    return float(loss.item()), grad.cpu().numpy(), loss.cpu().numpy().view(np.uint32)[0]


def _three_ways(model, cur, nxt, rows, B):
    """(kernel, torch float32 on the GPU, float64 on the CPU), each (loss, flat gradient), on the same batch."""
    import torch
    dev = _dev()
    pick = torch.arange(B) if rows is None else rows
    k_loss, k_grad, _ = kernel_loss_grad(model, cur.to(dev), nxt.to(dev), rows, B)
    t_loss, t_grad = R.loss_and_grad(copy.deepcopy(model).to(dev), cur[pick].to(dev), nxt[pick].to(dev))
    d_loss, d_grad = R.loss_and_grad64(model, cur[pick], nxt[pick])
    return (k_loss, k_grad), (t_loss, t_grad), (d_loss, d_grad)


def _parity(what, kernel, torch32, ref64):
    return F.parity(what, kernel, torch32, ref64, R.layout())


def _slot(name):
    return F.slot(R.layout(), name)


# one scene of one pedestrian (weight 1: attention has no gradient); workgroups that are not full and a short last one
# (1 x 2, 3 x 2, 5 x 3, 3 x 4: several scenes per workgroup up to 4 pedestrians); the workload's shape (7 x 5, 100 x 5: one
# scene per workgroup from 5 on); 33 x 10; both sides of the LDS / workspace threshold (16 | 17); the largest crowd
SHAPES = [(1, 1), (1, 2), (3, 2), (5, 3), (3, 4), (7, 5), (100, 5), (33, 10), (2, 16), (2, 17), (2, 32)]


@pytest.mark.parametrize("B,N", SHAPES)
def test_gradient_parity_with_float64(B, N):
    """Loss and gradient of one mini-batch against float64 autograd, for two weight seeds, with the batch as rows
    0 .. B-1 (rows = NULL) and as a shuffled, non-contiguous index list into a memory of B + 9 rows.

    Bound: MARGIN = 4 times the error of torch's float32 autograd on the GPU on the same inputs, per parameter tensor
    and for the loss; the gradient of attention.4.bias exactly 0.  Measured figures: DESIGN.md 3.6a."""
    import torch
    bad = []
    off, _ = _slot("attention.4.bias")
    for seed in (0, 1):
        model = R.attention_world(seed)
        cur, nxt = R.pairs(B + 9, N, seed=100 + seed)
        shuffled = torch.randperm(B + 9, generator=torch.Generator().manual_seed(seed))[:B]
        for rows in (None, shuffled):
            what = "B %d N %d seed %d rows %s" % (B, N, seed, "NULL" if rows is None else "shuffled")
            kernel, torch32, ref64 = _three_ways(model, cur, nxt, rows, B)
            assert np.isfinite(kernel[1]).all() and not (kernel[1] == SENTINEL).any(), what
            bad += _parity(what, kernel, torch32, ref64)
            if kernel[1][off] != 0.0:
                bad.append("%s: attention.4.bias gradient %r, not exactly 0" % (what, kernel[1][off]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,N", [(7, 5), (3, 2), (2, 17)])
def test_forward_only_mode_gives_the_same_loss_and_writes_no_gradient(B, N):
    """grad == NULL: the loss has the bits of the call with a gradient, and the gradient buffer keeps its sentinel."""
    import torch
    model = R.attention_world(0)
    cur, nxt = R.pairs(B + 9, N, seed=5)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(3))[:B]
    for r in (None, rows):
        full = kernel_loss_grad(model, cur.to(_dev()), nxt.to(_dev()), r, B)
        only = kernel_loss_grad(model, cur.to(_dev()), nxt.to(_dev()), r, B, want_grad=False)
        assert full[2] == only[2] and np.isfinite(only[0]) and only[0] != SENTINEL
        assert (only[1] == SENTINEL).all() and not (full[1] == SENTINEL).any()


@pytest.mark.parametrize("B,N", [(100, 5), (33, 10), (2, 32)])
def test_two_calls_give_the_same_bits(B, N):
    """No atomics, a fixed summation order: the same inputs give the same gradient and loss bits."""
    import torch
    model = R.attention_world(0)
    cur, nxt = R.pairs(B + 9, N, seed=7)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(2))[:B]
    a = kernel_loss_grad(model, cur.to(_dev()), nxt.to(_dev()), rows, B)
    b = kernel_loss_grad(model, cur.to(_dev()), nxt.to(_dev()), rows, B)
    assert a[2] == b[2] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.isfinite(a[1]).all() and not (a[1] == SENTINEL).any()


@pytest.mark.parametrize("B,N", [(7, 5), (3, 2)])
def test_all_zero_scores_are_nan_where_torch_is(B, N):
    """attention.4 zeroed: every score is exactly 0, the masked softmax is 0 / 0.  Loss and gradient are NaN exactly
    where torch's float32 autograd has NaN; what is left (units behind a ReLU that is off in every row) is exactly 0."""
    import torch
    model = R.attention_world(0)
    with torch.no_grad():
        model.attention[4].weight.zero_()
        model.attention[4].bias.zero_()
    cur, nxt = R.pairs(B, N, seed=11)
    kernel, torch32, _ = _three_ways(model, cur, nxt, None, B)
    assert np.isnan(kernel[0]) and np.isnan(torch32[0])
    assert np.isnan(torch32[1]).any()
    assert np.array_equal(np.isnan(kernel[1]), np.isnan(torch32[1]))
    keep = ~np.isnan(torch32[1])
    assert np.array_equal(kernel[1][keep], torch32[1][keep]) and not kernel[1][keep].any()


def test_dead_relu_layer_stops_the_gradient_exactly():
    """mlp3.2 with a large negative bias: its ReLU is off in every row, so mlp3.2 itself and everything below it --
    mlp3.0, attention, mlp2, mlp1 -- get exactly 0, as from torch and from float64; mlp3.4.weight multiplies that zero
    output; mlp3.4.bias and mlp3.6 keep the parity bound."""
    import torch
    B, N = 7, 5
    model = R.attention_world(1)
    with torch.no_grad():
        model.mlp3[2].bias.fill_(-1e4)
    cur, nxt = R.pairs(B, N, seed=12)
    kernel, torch32, ref64 = _three_ways(model, cur, nxt, None, B)
    table, _ = R.layout()
    below = [(k, off, shp) for k, off, shp in table if not k.startswith(("mlp3.4", "mlp3.6"))]
    assert len(below) == 18 and below[-1][0] == "mlp3.2.bias"
    for k, off, shp in below:
        n = int(np.prod(shp))
        assert not torch32[1][off:off + n].any() and not ref64[1][off:off + n].any(), k
        assert not kernel[1][off:off + n].any(), k
    zero_t = torch32[1] == 0.0
    assert not kernel[1][zero_t].any()
    lo = _slot("mlp3.4.bias")[0]
    assert np.isfinite(kernel[1]).all() and np.abs(kernel[1][lo:]).max() > 0
    bad = _parity("dead mlp3.2", kernel, torch32, ref64)
    assert not bad, "\n".join(bad)


def test_adam_kernel_is_torchs_rule():
    """1, 2 and 10 steps of mcn_adam_step from zero moments on random parameters and gradients (a count that is no
    multiple of the workgroup, several workgroups, a block of exactly-zero gradients) against the float64 rule
    (world_trainer_ref.adam64).  Bound, in units of the parameter's float32 spacing: MARGIN times the error of
    torch.optim.Adam in float32 on the GPU on the same inputs, with a floor of one spacing; the zero-gradient block keeps
    its bits, with zero moments.  The hyper-parameters are torch's defaults as Python floats for all three: the entry
    point takes them as float32 and applies the float64 that was written (include/mcn.h)."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = _dev()
    count = 94953 + 3
    lr, beta1, beta2, eps = 1e-3, 0.9, 0.999, 1e-8
    zero = slice(1000, 1300)
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(count, generator=g) * 0.1
    p0 = p0 + 0.05 * torch.where(p0 < 0, -1.0, 1.0)     # |p| >= 0.05: ten steps of at most lr each do not reach 0
    grads = [torch.randn(count, generator=g) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g)) for _ in range(10)]
    for gr in grads:
        gr[zero] = 0.0
    want = p0.clone().to(dev).requires_grad_(True)
    opt = torch.optim.Adam([want], lr=lr, betas=(beta1, beta2), eps=eps)
    p, m, v = p0.clone().to(dev), torch.zeros(count, device=dev), torch.zeros(count, device=dev)
    p64, m64, v64 = p0.double(), torch.zeros(count, dtype=torch.float64), torch.zeros(count, dtype=torch.float64)
    for s, gr in enumerate(grads, start=1):
        gd = gr.to(dev)
        want.grad = gd.clone()
        opt.step()
        _hip.check(_hip.lib.mcn_adam_step(_hip.ptr(p), _hip.ptr(m), _hip.ptr(v), _hip.ptr(gd), count, lr, beta1, beta2,
                                          eps, s, _hip.stream_ptr(dev)), "mcn_adam_step")
        torch.cuda.synchronize()
        p64, m64, v64 = R.adam64(p64, m64, v64, gr.double(), s, lr, beta1, beta2, eps)
        if s in (1, 2, 10):
            uk, ut = F.ulps(p.cpu().numpy(), p64.numpy()), F.ulps(want.detach().cpu().numpy(), p64.numpy())
            print("step %d: max error in float32 spacings of the parameter: kernel %.3g, torch %.3g" % (s, uk.max(), ut.max()))
            assert uk.max() <= MARGIN * max(ut.max(), 1.0)
            assert torch.equal(p.cpu()[zero], p0[zero]) and not m.cpu()[zero].any() and not v.cpu()[zero].any()
            st = opt.state[want]
            for name, mine, ref, theirs in (("exp_avg", m, m64, st["exp_avg"]), ("exp_avg_sq", v, v64, st["exp_avg_sq"])):
                live = np.ones(count, bool)
                live[zero] = False
                uk = F.ulps(mine.cpu().numpy()[live], ref.numpy()[live])
                ut = F.ulps(theirs.cpu().numpy()[live], ref.numpy()[live])
                print("step %d: %s kernel %.3g, torch %.3g spacings" % (s, name, uk.max(), ut.max()))
                assert uk.max() <= MARGIN * max(ut.max(), 1.0), name
    assert not torch.equal(p.cpu(), p0)


def _g20(golden_dir, tag):
    import torch
    from modelcrowdnav_amd.policy.world_model import AttentionWorld
    g = np.load(os.path.join(golden_dir, "g20_trainer_sim.npz"))
    load = lambda pref: {k[len(pref):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pref)}
    model = AttentionWorld()
    model.load_state_dict(load("w0__"))
    nxt = g["next"] if tag == "short" else g["next_stop"]
    mem = [(torch.from_numpy(g["cur"][i]), torch.from_numpy(nxt[i])) for i in range(int(g[tag + "_rows"]))]
    return g, load, model, mem


def _within(what, got, fixture, replay):
    """|got - replay| <= MARGIN max(|fixture - replay|, one float32 spacing of the value): the kernel returns a float32."""
    d_got = float(np.abs(np.asarray(got, np.float64) - replay).max())
    d_fix = float(np.abs(np.asarray(fixture, np.float64) - replay).max())
    floor = float(np.spacing(np.float32(np.abs(replay).max())))
    print("%s: distance from the float64 replay: got %.3g, fixture / torch %.3g, float32 spacing %.3g" % (what, d_got, d_fix, floor))
    assert d_got <= MARGIN * max(d_fix, floor), (what, d_got, d_fix, floor)


@pytest.mark.parametrize("tag,calls", [("short", (5, 3)), ("stop", (50,))])
def test_fused_world_trainer_matches_reference_trainer(tag, calls, golden_dir, tmp_path):
    """The scenario of tests/test_training_cpu.py::test_world_model_trainer_matches_reference_trainer (g20_trainer_sim.npz:
    the REFERENCE's own float32 Trainer_Sim; the fixture's permutations, random.seed(2000), batch size 1000, lr 1e-3;
    `short` = 5 + 3 epochs, `stop` = early stopping) with fused=True on the device.  Early-stopping state and the number
    of best values equal the fixture's; each best validation loss, model.mse and (`short`) the trained function on the
    first 64 rows are within MARGIN times the larger of the fixture's own distance from the float64 replay of the run and one
    float32 spacing; single weights within lr x epochs of the fixture's (Adam turns a rounding-noise gradient into
    lr-sized steps, and the kernel's exact 0 on attention.4.bias leaves that weight where it was)."""
    import torch
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    dev, lr = _dev(), 1e-3
    g, load, model, mem = _g20(golden_dir, tag)
    perms = [(g["%s_call%d_train_perms" % (tag, c)], g["%s_call%d_val_perms" % (tag, c)]) for c in range(len(calls))]
    bests64, _, m64 = R.replay64(model, list(mem), calls, perms, 1000, lr, seed=2000)
    start = copy.deepcopy(model)
    tr = Trainer_Sim(model.to(dev), mem, dev, 1000, str(tmp_path / (tag + ".pt")), fused=True)
    tr.set_learning_rate(lr)
    random.seed(2000)
    bests = [tr.optimize_epoch(e, perms=perms[c]) for c, e in enumerate(calls)]
    assert len(bests) == len(g[tag + "_best"])
    assert tr.early_stopping.counter == int(g[tag + "_counter"])
    assert bool(tr.early_stopping.early_stop) == bool(g[tag + "_stopped"])
    for c in range(len(calls)):
        _within("%s call %d best" % (tag, c), [bests[c]], [g[tag + "_best"][c]], np.asarray([bests64[c]]))
    _within(tag + " model.mse", [model.mse], [float(g[tag + "_mse"])], np.asarray([bests64[-1]]))
    want = load(tag + "_w1__")
    if tag == "short":               # (the fixture keeps every tensor of `short`, and six of `stop`)
        # the trained function, each set of weights evaluated in float64
        x = torch.from_numpy(g["cur"][:64]).reshape(64, -1).double()
        fixture = copy.deepcopy(start)
        fixture.load_state_dict(want)
        with torch.no_grad():
            y64, y_fix, y_got = m64(x).numpy(), R.as64(fixture)(x).numpy(), R.as64(model)(x).numpy()
        _within(tag + " trained function", y_got, y_fix, y64)
    sd = model.state_dict()
    worst = max(float((sd[k].cpu() - v).abs().max()) for k, v in want.items())
    assert worst <= lr * sum(calls), (tag, worst)
    assert torch.equal(sd["attention.4.bias"].cpu(), start.state_dict()["attention.4.bias"])


def test_fused_and_torch_paths_train_on_the_same_batches(monkeypatch):
    """Without `perms`, from the same torch and Python seeds, a fused and a torch trainer split the memory alike (the
    stacked tensors _pairs() returns) and draw the same permutations -- captured at torch.randperm -- and the fused
    path's rows are those permutations.  130 rows, batch 16: 104 training rows end on a batch of 8, 26 validation rows
    on one of 10, which counts like a full one.  Best validation losses of the two calls: the fused path within MARGIN
    times the larger of the torch path's distance from the float64 replay of those batches and one float32 spacing."""
    import torch
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    dev, lr, N, calls = _dev(), 1e-3, 5, (3, 2)
    model0 = R.attention_world(2)
    cur, nxt = R.pairs(130, N, seed=21)
    memory = [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(130)]
    drawn, stacked = [], []
    real = torch.randperm

    def recording(n, *a, **kw):
        out = real(n, *a, **kw)
        drawn.append(out.clone().cpu())
        return out
    monkeypatch.setattr(torch, "randperm", recording)
    real_pairs = Trainer_Sim._pairs

    def pairs(self):
        out = real_pairs(self)
        stacked.append([t.clone().cpu() for part in out for t in part])
        return out
    monkeypatch.setattr(Trainer_Sim, "_pairs", pairs)
    result = {}
    for fused in (False, True):
        del drawn[:], stacked[:]
        model = copy.deepcopy(model0).to(dev)
        tr = Trainer_Sim(model, list(memory), dev, 16, fused=fused)
        tr.set_learning_rate(lr)
        torch.manual_seed(77)
        torch.cuda.manual_seed_all(77)
        random.seed(31)
        bests, used = [], []
        for e in calls:
            bests.append(tr.optimize_epoch(e))
            if fused:
                assert all(v is None for _, v in tr.last_rows)
                used += [p.cpu() for p, _ in tr.last_rows]
        result[fused] = (list(drawn), list(stacked), bests, used)
    perms_t, split_t, bests_t, _ = result[False]
    perms_f, split_f, bests_f, used_f = result[True]
    assert len(perms_t) == len(perms_f) == sum(calls) and all(torch.equal(a, b) for a, b in zip(perms_t, perms_f))
    assert all(p.numel() == 104 and sorted(p.tolist()) == list(range(104)) for p in perms_t)
    assert len(used_f) == sum(calls) and all(torch.equal(a, b) for a, b in zip(used_f, perms_t))
    assert len(split_t) == len(split_f) == 2 and [t.shape[0] for t in split_t[0]] == [104, 104, 26, 26]
    assert all(torch.equal(a, b) for s, t in zip(split_t, split_f) for a, b in zip(s, t))
    replay_perms, at = [], 0
    for e in calls:
        replay_perms.append(([p.numpy() for p in perms_t[at:at + e]], [np.arange(26)] * e))
        at += e
    bests64, _, _ = R.replay64(model0, list(memory), calls, replay_perms, 16, lr, seed=31)
    for c in range(len(calls)):
        _within("call %d best" % c, [bests_f[c]], [bests_t[c]], np.asarray([bests64[c]]))


def test_fused_world_trainer_writes_back_and_reads_the_module():
    """After a fused optimize_epoch the module holds the best weights (early stopping's copy), every parameter's version
    counter has moved, and a VecAttnWorld built on the module before training re-packs and reproduces the module's
    forward (the bar of tests/test_pipeline_gpu.py).  load_state_dict between two calls is honoured: back at the start
    with a fresh optimizer state the same epochs give the same weights again.  set_learning_rate resets the moments and
    the step count: the first step after it is Adam's first step on the kernel's own gradient."""
    import torch
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.envs import VecModelCrowdSim
    from modelcrowdnav_amd.policy.world_model import VecAttnWorld, VecTorchWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    from tests import helpers as H
    dev, N, E = _dev(), 5, 16
    model = R.attention_world(4).to(dev).eval()
    env = H.make_vec_env(E, N, cls=VecModelCrowdSim)
    H.upload(env, H.random_state(np.random.RandomState(3), E, N))
    fast, slow = VecAttnWorld(model, env), VecTorchWorld(model, env)
    v0 = fast(env.hpos).clone()
    cur, nxt = R.pairs(40, N, seed=8)
    memory = [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(40)]
    perms = (np.stack([np.random.RandomState(k).permutation(32) for k in range(2)]), np.stack([np.arange(8)] * 2))
    w0 = {k: v.clone() for k, v in model.state_dict().items()}
    tr = Trainer_Sim(model, list(memory), dev, 16, fused=True)
    tr.set_learning_rate(1e-2)
    stamp0 = _hip.weights_stamp(list(model.parameters()), dev)
    random.seed(5)
    tr.optimize_epoch(2, reset=True, perms=perms)
    stamp1 = _hip.weights_stamp(list(model.parameters()), dev)
    assert all(a[2] != b[2] for a, b in zip(stamp0[:-1], stamp1[:-1])), "a parameter's version counter did not move"
    w1 = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(v, tr.early_stopping.best_state[k]) for k, v in w1.items())
    assert all(not torch.equal(w0[k], w1[k]) for k in w0 if k != "attention.4.bias")
    assert tr._fz["step"] == 4 and abs(model.mse + tr.early_stopping.best_score) == 0
    v1, want1 = fast(env.hpos).clone(), slow(env.hpos)                   # no refresh()
    assert not torch.equal(v0, v1)
    assert float((v1 - want1).abs().max()) <= 1e-5 * max(1.0, float(want1.abs().max()))

    # load_state_dict is honoured: back at w0 with a fresh optimizer state, the same memory order and the same row orders
    model.load_state_dict(w0)
    tr.memory = list(memory)
    tr.set_learning_rate(1e-2)
    assert tr._fz["step"] == 0 and not tr._fz["m"].any() and not tr._fz["v"].any()
    random.seed(5)
    tr.optimize_epoch(2, reset=True, perms=perms)
    assert all(torch.equal(w1[k], v) for k, v in model.state_dict().items())

    # set_learning_rate resets the moments and the step count: one epoch of one batch is Adam's FIRST step
    tr.set_learning_rate(2e-3)
    frozen = copy.deepcopy(model)
    before = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().double()
    tr.batch_size = 64
    tr.memory = list(memory)
    random.seed(6)
    tr.optimize_epoch(1, reset=True, perms=(perms[0][:1], perms[1][:1]))
    assert tr._fz["step"] == 1
    (tx, ty), _ = Trainer_Sim._pairs(Trainer_Sim(frozen, _reseeded(memory, 6), dev, 64))
    _, grad, _ = kernel_loss_grad(frozen, tx, ty, torch.from_numpy(perms[0][0]), 32)
    g64 = torch.from_numpy(grad).double()
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    want, m64, v64 = R.adam64(before, torch.zeros_like(before), torch.zeros_like(before), g64, 1, lr, b1, b2, eps)
    assert np.array_equal(tr._fz["m"].cpu().numpy(), m64.float().numpy())
    after = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()
    assert F.ulps(after, want.numpy()).max() <= 1.0 and not np.array_equal(after, before.float().numpy())


def _reseeded(memory, seed):
    """A copy of the memory list with Python's generator seeded as for the trainer call it stands in for."""
    random.seed(seed)
    return list(memory)
