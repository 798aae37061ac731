"""GPU: the fused MlpWorld training step (csrc/world_mlp_train.hip through mcn_mlp_world_loss_grad / mcn_adam_step and
Trainer_Sim(fused=True)) against the float64 yardstick of tests/mlp_world_trainer_ref.py.  The dropout masks always come
from that file's numpy restatement of the definition, never from the kernel or the library.  Every bound is a multiple of
what torch's own float32 path (or the reference's recorded float32 Trainer_Sim) is away from the yardstick on the same
inputs and masks; nothing is compared with an earlier output of the kernel."""
import copy
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import fused_train_harness as F  # noqa: E402
from tests import mlp_world_trainer_ref as R  # noqa: E402
from tests.fused_train_harness import MARGIN, SENTINEL  # noqa: E402

G = R.GROUP


def _dev():
    import torch
    return torch.device("cuda", 0)


def kernel_loss_grad(model, cur, nxt, rows, B, p, seed=0, step=0, want_grad=True):
    """mcn_mlp_world_loss_grad on device tensors (cur [M,4N], nxt [M,2N], rows [B] int64 or None) with the float32
    weights of `model` -> (loss, flat gradient as numpy, loss bits).  The outputs start as a sentinel; without
    want_grad the gradient pointer is NULL and the sentinel buffer comes back as it was left."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = _dev()
    N = int(cur.shape[1]) // 4
    assert cur.shape[1] == 4 * N and nxt.shape[1] == 2 * N and cur.is_contiguous() and nxt.is_contiguous()
    count = int(_hip.lib.mcn_mlp_world_train_param_count(N))
    params = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).to(dev, torch.float32).contiguous()
    assert params.numel() == count == R.param_count(N)
    ws = torch.empty(int(_hip.lib.mcn_mlp_world_train_workspace_bytes(B, N)), dtype=torch.uint8, device=dev)
    grad = torch.full((count,), SENTINEL, dtype=torch.float32, device=dev)
    loss = torch.full((1,), SENTINEL, dtype=torch.float32, device=dev)
    rows_dev = None if rows is None else rows.to(dev, torch.long).contiguous()
    assert rows is None or (rows_dev.numel() == B and int(rows_dev.min()) >= 0 and int(rows_dev.max()) < cur.shape[0])
    assert rows is not None or B <= cur.shape[0]
    assert ws.numel() > 0
    _hip.check(_hip.lib.mcn_mlp_world_loss_grad(_hip.ptr(params), _hip.ptr(cur), _hip.ptr(nxt), _hip.ptr(rows_dev), B, N, p,
                                                seed, step, _hip.ptr(ws), _hip.ptr(grad) if want_grad else None,
                                                _hip.ptr(loss), _hip.stream_ptr(dev)), "mcn_mlp_world_loss_grad")
    torch.cuda.synchronize()
    return float(loss.item()), grad.cpu().numpy(), loss.cpu().numpy().view(np.uint32)[0]


def _three_ways(model, cur, nxt, rows, B, p, seed, step):
    """(kernel, torch float32 on the GPU, float64 on the CPU), each (loss, flat gradient), on the same batch with the
    definition's masks for (seed, step): slot b is scene b of the batch, whatever memory row it is."""
    import torch
    dev = _dev()
    pick = torch.arange(B) if rows is None else rows
    keep = R.masks(seed, step, B, p)
    kernel = kernel_loss_grad(model, cur.to(dev), nxt.to(dev), rows, B, p, seed, step)
    t32 = R.loss_and_grad_masked(copy.deepcopy(model).to(dev), cur[pick].to(dev), nxt[pick].to(dev), keep, p)
    r64 = R.loss_and_grad64_masked(model, cur[pick], nxt[pick], keep, p)
    return kernel[:2], t32, r64


# one scene; one short of a workgroup, a full one, one more, two and a short third; one pedestrian; the workload's batch
# (13 workgroups); 33 x 10; the largest crowd
SHAPES = [(1, 5), (G - 1, 5), (G, 5), (G + 1, 5), (2 * G + 3, 5), (7, 1), (100, 5), (33, 10), (2, 32)]


@pytest.mark.parametrize("B,N", SHAPES)
def test_gradient_parity_with_float64(B, N):
    """Loss and gradient of one mini-batch in train mode against float64 autograd with the same masks, for p = 0.5, 0.1
    and 0, two weight seeds, two (dropout seed, step) pairs, with the batch as rows 0 .. B-1 (rows = NULL) and as a
    shuffled, non-contiguous index list into a memory of B + 9 rows.

    Bound: MARGIN = 4 times the error of torch's float32 autograd on the GPU on the same inputs and masks, per
    parameter tensor and for the loss; no sentinel left.  Measured figures: DESIGN.md 3.6c."""
    import torch
    bad = []
    for wseed in (0, 1):
        cur, nxt = R.pairs(B + 9, N, seed=100 + wseed)
        shuffled = torch.randperm(B + 9, generator=torch.Generator().manual_seed(wseed))[:B]
        for p in (0.5, 0.1, 0.0):
            model = R.mlp_world(N, wseed, p)
            for seed, step in ((7, 0), (2 ** 63 + 5, 1234567)):
                for rows in (None, shuffled):
                    what = "B %d N %d p %g weights %d mask (%d, %d) rows %s" % (B, N, p, wseed, seed, step,
                                                                             "NULL" if rows is None else "shuffled")
                    kernel, torch32, ref64 = _three_ways(model, cur, nxt, rows, B, p, seed, step)
                    assert np.isfinite(kernel[1]).all() and not (kernel[1] == SENTINEL).any(), what
                    assert np.isfinite(kernel[0]) and kernel[0] != SENTINEL, what
                    bad += R.compare(what, kernel, torch32, ref64, N)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,N", [(2 * G + 3, 5), (33, 10)])
def test_masks_follow_step_and_seed_and_the_same_call_gives_the_same_bits(B, N):
    """Another step or another seed gives another gradient; the same arguments give the same gradient and loss bits
    twice (no atomics, a fixed summation order)."""
    import torch
    model = R.mlp_world(N, 0)
    cur, nxt = R.pairs(B + 9, N, seed=7)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(2))[:B]
    cur_d, nxt_d = cur.to(_dev()), nxt.to(_dev())
    a = kernel_loss_grad(model, cur_d, nxt_d, rows, B, 0.5, seed=3, step=10)
    b = kernel_loss_grad(model, cur_d, nxt_d, rows, B, 0.5, seed=3, step=10)
    assert a[2] == b[2] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.isfinite(a[1]).all() and not (a[1] == SENTINEL).any()
    for kw in (dict(seed=3, step=11), dict(seed=4, step=10)):
        c = kernel_loss_grad(model, cur_d, nxt_d, rows, B, 0.5, **kw)
        assert c[2] != a[2] and not np.array_equal(c[1], a[1]), kw
        off, n = F.slot(R.layout(N), "mlp.3.weight")
        assert (c[1][off:off + n] != a[1][off:off + n]).mean() > 0.25, kw


@pytest.mark.parametrize("B,N", [(7, 5), (G + 1, 5), (2, 32)])
def test_forward_only_mode_is_the_eval_pass_and_writes_no_gradient(B, N):
    """grad == NULL: the loss is the eval-mode forward's -- whatever drop_p, seed and step say -- within MARGIN times the
    error of torch's float32 eval forward on the GPU against the float64 one; with p = 0 it has the bits of the call with
    a gradient; the gradient buffer keeps its sentinel."""
    import torch
    dev = _dev()
    model = R.mlp_world(N, 0).eval()
    cur, nxt = R.pairs(B + 9, N, seed=5)
    rows = torch.randperm(B + 9, generator=torch.Generator().manual_seed(3))[:B]
    for r in (None, rows):
        pick = torch.arange(B) if r is None else r
        with torch.no_grad():
            want = float(torch.nn.functional.mse_loss(R.as64(model)(cur[pick].double()), nxt[pick].double()).item())
            t32 = float(torch.nn.functional.mse_loss(copy.deepcopy(model).to(dev)(cur[pick].to(dev)), nxt[pick].to(dev)).item())
        only = [kernel_loss_grad(model, cur.to(dev), nxt.to(dev), r, B, p, seed, step, want_grad=False)
                for p, seed, step in ((0.5, 1, 2), (0.0, 0, 0), (0.9, 99, 2 ** 40))]
        full0 = kernel_loss_grad(model, cur.to(dev), nxt.to(dev), r, B, 0.0, 5, 6)
        print("B %d N %d: eval loss err kernel %.3g torch %.3g (of %.3g)" % (B, N, abs(only[0][0] - want), abs(t32 - want), want))
        assert abs(only[0][0] - want) <= MARGIN * abs(t32 - want)
        assert only[0][2] == only[1][2] == only[2][2] == full0[2]
        assert all((o[1] == SENTINEL).all() for o in only) and not (full0[1] == SENTINEL).any()
        trained = kernel_loss_grad(model, cur.to(dev), nxt.to(dev), r, B, 0.5, 1, 2)
        assert trained[2] != only[0][2]                          # (the train-mode loss at p = 0.5 is another number)


def test_dead_relu_layer_stops_the_gradient_exactly():
    """mlp.3 with a large negative bias: its ReLU is off in every row, so mlp.3 itself and mlp.0 below it get exactly 0,
    as from torch and from float64; mlp.6.weight multiplies that zero output; mlp.6.bias and mlp.8 keep the parity
    bound."""
    import torch
    B, N, p = G + 3, 5, 0.5
    model = R.mlp_world(N, 1, p)
    with torch.no_grad():
        model.mlp[3].bias.fill_(-1e4)
    cur, nxt = R.pairs(B, N, seed=12)
    kernel, torch32, ref64 = _three_ways(model, cur, nxt, None, B, p, 7, 3)
    table, _ = R.layout(N)
    below = [(k, off, shp) for k, off, shp in table if k.startswith(("mlp.0", "mlp.3")) or k == "mlp.6.weight"]
    assert len(below) == 5
    for k, off, shp in below:
        n = int(np.prod(shp))
        assert not torch32[1][off:off + n].any() and not ref64[1][off:off + n].any(), k
        assert not kernel[1][off:off + n].any(), k
    lo = F.slot(R.layout(N), "mlp.6.bias")[0]
    assert np.isfinite(kernel[1]).all() and np.abs(kernel[1][lo:]).max() > 0
    bad = R.compare("dead mlp.3", kernel, torch32, ref64, N)
    assert not bad, "\n".join(bad)


def test_saturated_tanh_stays_finite():
    """mlp.8.bias = 30: every output is tanh(30) = 1 to float64, 1 - out^2 is 0 and so is every gradient; nothing
    overflows and the loss keeps its bound."""
    import torch
    B, N, p = G + 3, 5, 0.5
    model = R.mlp_world(N, 1, p)
    with torch.no_grad():
        model.mlp[8].bias.fill_(30.0)
    cur, nxt = R.pairs(B, N, seed=13)
    kernel, torch32, ref64 = _three_ways(model, cur, nxt, None, B, p, 7, 3)
    assert np.isfinite(kernel[0]) and np.isfinite(kernel[1]).all() and not (kernel[1] == SENTINEL).any()
    bad = R.compare("saturated tanh", kernel, torch32, ref64, N)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("column", [0, 13])
def test_nan_input_is_nan_where_torch_is(column):
    """One NaN in one scene's input at p = 0.5 (dropout is a product: a dropped NaN is NaN, as from nn.Dropout): loss
    and gradient are NaN exactly where torch's float32 autograd with the same masks has NaN, and what is left keeps the
    parity bound."""
    B, N, p = G + 3, 5, 0.5
    model = R.mlp_world(N, 0, p)
    cur, nxt = R.pairs(B, N, seed=11)
    cur[G + 1, column] = float("nan")
    kernel, torch32, ref64 = _three_ways(model, cur, nxt, None, B, p, 7, 3)
    assert np.isnan(kernel[0]) and np.isnan(torch32[0]) and np.isnan(ref64[0])
    assert np.isnan(torch32[1]).any() and not (kernel[1] == SENTINEL).any()
    assert np.array_equal(np.isnan(kernel[1]), np.isnan(torch32[1]))
    keep = ~np.isnan(torch32[1]) & ~np.isnan(ref64[1])
    if keep.any():
        ek, et = np.abs(kernel[1][keep] - ref64[1][keep]).max(), np.abs(torch32[1][keep] - ref64[1][keep]).max()
        assert ek <= MARGIN * et, (ek, et)


def _g27(golden_dir):
    import torch
    from modelcrowdnav_amd.policy.world_model import MlpWorld
    g = np.load(os.path.join(golden_dir, "g27_mlp_world_trainer.npz"))
    load = lambda pref: {k[len(pref):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pref)}
    model = MlpWorld(5, drop_rate=0.0)
    model.load_state_dict(load("w0__"))
    mem = [(torch.from_numpy(g["cur"][i]), torch.from_numpy(g["next"][i])) for i in range(int(g["short_rows"]))]
    return g, load, model, mem


def _within(what, got, other, replay):
    """|got - replay| <= MARGIN max(|other - replay|, one float32 spacing of the value): the kernel returns a float32."""
    d_got = float(np.abs(np.asarray(got, np.float64) - replay).max())
    d_other = float(np.abs(np.asarray(other, np.float64) - replay).max())
    floor = float(np.spacing(np.float32(np.abs(replay).max())))
    print("%s: distance from the float64 replay: got %.3g, fixture / float32 %.3g, float32 spacing %.3g" % (what, d_got, d_other, floor))
    assert d_got <= MARGIN * max(d_other, floor), (what, d_got, d_other, floor)


def test_fused_mlp_world_trainer_matches_reference_trainer(golden_dir, tmp_path):
    """g27_mlp_world_trainer.npz: the REFERENCE's own float32 Trainer_Sim on MlpWorld(5, drop_rate=0.0) (the fixture's
    permutations, random.seed(2000), batch size 1000, lr 1e-3, 5 + 3 epochs) with fused=True on the device.
    Early-stopping state and the number of best values equal the fixture's; each best validation loss, model.mse and the
    trained function on the first 64 rows are within MARGIN times the larger of the fixture's own distance from the
    float64 replay of the run and one float32 spacing."""
    import torch
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    dev, lr, calls = _dev(), 1e-3, (5, 3)
    g, load, model, mem = _g27(golden_dir)
    perms = [(g["short_call%d_train_perms" % c], g["short_call%d_val_perms" % c]) for c in range(len(calls))]
    bests64, _, m64 = R.replay(model, list(mem), calls, perms, 1000, lr, 0.0, 0, seed=2000)
    start = copy.deepcopy(model)
    tr = Trainer_Sim(model.to(dev), mem, dev, 1000, str(tmp_path / "short.pt"), fused=True)
    tr.set_learning_rate(lr)
    random.seed(2000)
    bests = [tr.optimize_epoch(e, perms=perms[c]) for c, e in enumerate(calls)]
    assert len(bests) == len(g["short_best"])
    assert tr.early_stopping.counter == int(g["short_counter"])
    assert bool(tr.early_stopping.early_stop) == bool(g["short_stopped"])
    for c in range(len(calls)):
        _within("call %d best" % c, [bests[c]], [g["short_best"][c]], np.asarray([bests64[c]]))
    _within("model.mse", [model.mse], [float(g["short_mse"])], np.asarray([bests64[-1]]))
    x = torch.from_numpy(g["cur"][:64]).reshape(64, -1).double()
    fixture = copy.deepcopy(start)
    fixture.load_state_dict(load("short_w1__"))
    with torch.no_grad():
        y64, y_fix, y_got = m64.eval()(x).numpy(), R.as64(fixture).eval()(x).numpy(), R.as64(model).eval()(x).numpy()
    _within("trained function", y_got, y_fix, y64)
    assert not any(torch.equal(v.cpu(), start.state_dict()[k]) for k, v in model.state_dict().items())


def test_fused_mlp_world_trainer_with_dropout_matches_the_float64_replay():
    """130 rows, batch 16 (104 training rows end on a batch of 8, 26 validation rows on one of 10), calls of 3 and 2
    epochs, p = 0.5, given permutations, dropout_seed = 7: against the float64 replay of the run with the definition's
    masks keyed by the trainer's count of training steps (0 .. 34, running on over epochs and calls).  Best validation
    losses, model.mse and the trained function: within MARGIN times the larger of the float32 replay's distance from the
    float64 one and one float32 spacing."""
    import torch
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    dev, lr, N, calls, p, B = _dev(), 1e-3, 5, (3, 2), 0.5, 16
    model0 = R.mlp_world(N, 2, p)
    cur, nxt = R.pairs(130, N, seed=21)
    memory = [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(130)]
    rs = np.random.RandomState(4)
    perms = [(np.stack([rs.permutation(104) for _ in range(e)]), np.stack([rs.permutation(26) for _ in range(e)])) for e in calls]
    bests64, every64, m64 = R.replay(model0, list(memory), calls, perms, B, lr, p, 7, seed=31)
    bests32, every32, m32 = R.replay(model0, list(memory), calls, perms, B, lr, p, 7, dtype=torch.float32, seed=31)
    model = copy.deepcopy(model0).to(dev)
    tr = Trainer_Sim(model, list(memory), dev, B, fused=True)
    tr.dropout_seed = 7
    tr.set_learning_rate(lr)
    random.seed(31)
    bests = [tr.optimize_epoch(e, perms=perms[c]) for c, e in enumerate(calls)]
    assert tr.mask_step == 7 * sum(calls) == tr._fz["step"] and tr.dropout_seed == 7
    assert not model.training
    for c in range(len(calls)):
        _within("call %d best" % c, [bests[c]], [bests32[c]], np.asarray([bests64[c]]))
    _within("model.mse", [model.mse], [bests32[-1]], np.asarray([bests64[-1]]))
    x = cur[:64].double()
    with torch.no_grad():
        y64, y32, y_got = m64.eval()(x).numpy(), R.as64(m32).eval()(x).numpy(), R.as64(model).eval()(x).numpy()
    _within("trained function", y_got, y32, y64)


def test_fused_mlp_world_trainer_writes_back_and_reads_the_module():
    """After a fused optimize_epoch the module holds the best weights (early stopping's copy), every parameter's version
    counter has moved, and a VecMlpWorld built on the module before training re-packs by itself and reproduces the
    module's eval forward.  load_state_dict between two calls is honoured and set_learning_rate starts Adam over while
    the masks' step counter goes on: the next step is Adam's FIRST step from the loaded weights on the gradient under
    the masks of step 4, not of step 0."""
    import torch
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.envs import VecModelCrowdSim
    from modelcrowdnav_amd.policy.world_model import VecMlpWorld, VecTorchWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    from tests import helpers as H
    dev, N, E, p = _dev(), 5, 16, 0.5
    model = R.mlp_world(N, 4, p).to(dev).eval()
    env = H.make_vec_env(E, N, cls=VecModelCrowdSim)
    H.upload(env, H.random_state(np.random.RandomState(3), E, N))
    fast, slow = VecMlpWorld(model, env), VecTorchWorld(model, env)
    v0 = fast(env.hpos).clone()
    cur, nxt = R.pairs(40, N, seed=8)
    memory = [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(40)]
    perms = (np.stack([np.random.RandomState(k).permutation(32) for k in range(2)]), np.stack([np.arange(8)] * 2))
    w0 = {k: v.clone() for k, v in model.state_dict().items()}
    tr = Trainer_Sim(model, list(memory), dev, 16, fused=True)
    tr.dropout_seed = 11
    tr.set_learning_rate(1e-2)
    stamp0 = _hip.weights_stamp(list(model.parameters()), dev)
    random.seed(5)
    tr.optimize_epoch(2, reset=True, perms=perms)
    stamp1 = _hip.weights_stamp(list(model.parameters()), dev)
    assert all(a[2] != b[2] for a, b in zip(stamp0[:-1], stamp1[:-1])), "a parameter's version counter did not move"
    w1 = {k: v.clone() for k, v in model.state_dict().items()}
    assert all(torch.equal(v, tr.early_stopping.best_state[k]) for k, v in w1.items())
    assert all(not torch.equal(w0[k], w1[k]) for k in w0)
    assert tr._fz["step"] == 4 == tr.mask_step and abs(model.mse + tr.early_stopping.best_score) == 0
    v1, want1 = fast(env.hpos).clone(), slow(env.hpos)                   # no refresh()
    assert not torch.equal(v0, v1)
    assert float((v1 - want1).abs().max()) <= 1e-5 * max(1.0, float(want1.abs().max()))

    # back at w0, a new optimizer: one epoch of one batch is Adam's first step, under the masks of step 4
    model.load_state_dict(w0)
    tr.set_learning_rate(2e-3)
    assert tr._fz["step"] == 0 and not tr._fz["m"].any() and not tr._fz["v"].any() and tr.mask_step == 4
    frozen = copy.deepcopy(model)
    before = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).cpu().double()
    tr.batch_size = 64
    tr.memory = list(memory)
    random.seed(6)
    tr.optimize_epoch(1, reset=True, perms=(perms[0][:1], perms[1][:1]))
    assert tr._fz["step"] == 1 and tr.mask_step == 5
    random.seed(6)
    (tx, ty), _ = Trainer_Sim._pairs(Trainer_Sim(frozen, list(memory), dev, 64))
    rows = torch.from_numpy(perms[0][0])
    loss, grad, _ = kernel_loss_grad(frozen, tx, ty, rows, 32, p, seed=11, step=4)
    _, grad_step0, _ = kernel_loss_grad(frozen, tx, ty, rows, 32, p, seed=11, step=0)
    lr, b1, b2, eps = 2e-3, 0.9, 0.999, 1e-8
    zeros = torch.zeros_like(before)
    want, m64, _ = R.adam64(before, zeros, zeros, torch.from_numpy(grad).double(), 1, lr, b1, b2, eps)
    _, m64_step0, _ = R.adam64(before, zeros, zeros, torch.from_numpy(grad_step0).double(), 1, lr, b1, b2, eps)
    got_m = tr._fz["m"].cpu().numpy()
    assert np.array_equal(got_m, m64.float().numpy()) and not np.array_equal(got_m, m64_step0.float().numpy())
    # the kernel's own gradient is the definition's: within the parity bound of the float64 one under the masks of step 4
    keep = R.masks(11, 4, 32, p)
    r64 = R.loss_and_grad64_masked(frozen, tx[rows.to(dev)].cpu(), ty[rows.to(dev)].cpu(), keep, p)
    t32 = R.loss_and_grad_masked(copy.deepcopy(frozen), tx[rows.to(dev)], ty[rows.to(dev)], keep, p)
    bad = R.compare("first step after set_learning_rate", (loss, grad), t32, r64, N)
    assert not bad, "\n".join(bad)
    after = torch.cat([q.detach().reshape(-1) for q in model.parameters()]).cpu().numpy()
    assert F.ulps(after, want.numpy()).max() <= 1.0 and not np.array_equal(after, before.float().numpy())
