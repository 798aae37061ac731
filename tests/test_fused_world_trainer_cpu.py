"""CPU: the host side of the fused AttentionWorld training step (csrc/world_train.hip; include/mcn.h:
mcn_attn_world_train_param_count, mcn_attn_world_train_workspace_bytes, mcn_attn_world_loss_grad, mcn_adam_step;
utils/trainer_sim.py: Trainer_Sim(fused=True)) -- the flat layout, the sizes, the argument validation (before any launch),
the refusals of the Python path, and that the default path is the one it was.  The kernels themselves are tested on the
device by tests/test_fused_world_trainer_gpu.py."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import world_trainer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcn_attn_world_train_param_count", "mcn_attn_world_train_workspace_bytes", "mcn_attn_world_loss_grad",
         "mcn_adam_step"]


def test_the_four_symbols_are_exported():
    from modelcrowdnav_amd import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in NAMES:
        assert n in _hip.EXPORTED and hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "mcn.h")).read()
    assert all(n + "(" in hdr for n in NAMES)


def test_param_count_and_flat_layout_are_the_modules():
    """94 953 floats in state_dict order: the library's count, the hand-written table of tests/world_trainer_ref.py, the
    module's own state_dict and the layout the trainer uses."""
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    model = R.attention_world(0)
    table, total = R.layout()
    assert _hip.lib.mcn_attn_world_train_param_count() == 94953 == total == sum(p.numel() for p in model.parameters())
    assert len(table) == 22 and table[0][0] == "mlp1.0.weight" and table[-1][0] == "mlp3.6.bias"
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, shp) for k, _, shp in table]
    assert [k for k, _ in model.named_parameters()] == [k for k, _, _ in table]
    tr = Trainer_Sim(model, [], torch.device("cpu"), 2)                   # not fused: only its layout is asked for
    assert tr._fused_layout() == (table, total)


def test_workspace_grows_with_the_batch_and_refuses_bad_shapes():
    from modelcrowdnav_amd import _hip
    ws = _hip.lib.mcn_attn_world_train_workspace_bytes
    for N in (1, 2, 3, 4, 5, 10, 16, 17, 32):
        sizes = [ws(B, N) for B in range(1, 130)]
        assert sizes[0] >= 4 * (94953 + 1) and sizes[0] % 8 == 0
        assert all(b >= a > 0 for a, b in zip(sizes[:-1], sizes[1:])), N
    # from 17 pedestrians on a scene's float64 buffers and mlp3 activations are in the workspace
    assert ws(1, 17) - ws(1, 16) > 17 * 8 * 400 and ws(1, 16) == ws(1, 5)
    assert ws(0, 5) == 0 and ws(-1, 5) == 0 and ws(4, 0) == 0 and ws(4, _hip.MAX_HUMANS + 1) == 0


_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = C.c_void_p(0x1000)                     # never dereferenced: validation fails first
inf, nan = float("inf"), float("nan")


def grad(params=fake, cur=fake, nxt=fake, rows=fake, B=4, N=5, ws=fake, g=fake, loss=fake):
    return lib.mcn_attn_world_loss_grad(params, cur, nxt, rows, B, N, ws, g, loss, None)


def adam(p=fake, m=fake, v=fake, g=fake, count=100, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
    return lib.mcn_adam_step(p, m, v, g, count, lr, beta1, beta2, eps, step, None)


# the acceptable calls get past validation and, with no device in sight, fail at the launch: each MCN_EINVAL below comes
# from the one argument that was changed (made only once the runtime itself confirms that it sees no device)
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert grad() == _hip.MCN_ELAUNCH
    assert grad(rows=None) == _hip.MCN_ELAUNCH, "rows = NULL means rows 0 .. B-1"
    assert grad(g=None) == _hip.MCN_ELAUNCH, "grad = NULL means the loss only"
    assert grad(N=_hip.MAX_HUMANS, B=1) == _hip.MCN_ELAUNCH and grad(N=1, B=1) == _hip.MCN_ELAUNCH
    assert adam() == _hip.MCN_ELAUNCH and adam(lr=0.0, beta1=0.0, beta2=0.0, eps=0.0, count=1, step=7) == _hip.MCN_ELAUNCH
    print("POSITIVE_CONTROL_OK")
bad_grad = {
    "params = NULL": dict(params=None), "cur = NULL": dict(cur=None), "nxt = NULL": dict(nxt=None),
    "workspace = NULL": dict(ws=None), "loss = NULL": dict(loss=None),
    "B = 0": dict(B=0), "B = -1": dict(B=-1), "N = 0": dict(N=0), "N = -3": dict(N=-3),
    "N = MCN_MAX_HUMANS + 1": dict(N=_hip.MAX_HUMANS + 1),
}
for what, kw in bad_grad.items():
    assert grad(**kw) == _hip.MCN_EINVAL, what
bad_adam = {
    "params = NULL": dict(p=None), "exp_avg = NULL": dict(m=None), "exp_avg_sq = NULL": dict(v=None),
    "grad = NULL": dict(g=None), "count = 0": dict(count=0), "count = -5": dict(count=-5),
    "step = 0": dict(step=0), "step = -1": dict(step=-1),
    "lr = inf": dict(lr=inf), "lr = -inf": dict(lr=-inf), "lr = nan": dict(lr=nan),
    "eps = inf": dict(eps=inf), "eps = nan": dict(eps=nan),
    "beta1 = inf": dict(beta1=inf), "beta1 = nan": dict(beta1=nan), "beta1 = 1": dict(beta1=1.0),
    "beta1 = -0.1": dict(beta1=-0.1), "beta1 = 1.5": dict(beta1=1.5),
    "beta2 = inf": dict(beta2=inf), "beta2 = nan": dict(beta2=nan), "beta2 = 1": dict(beta2=1.0),
    "beta2 = -0.1": dict(beta2=-0.1), "beta2 = 1.5": dict(beta2=1.5),
}
for what, kw in bad_adam.items():
    assert adam(**kw) == _hip.MCN_EINVAL, what
print("WORLD_TRAIN_VALIDATION_OK")
"""


def test_training_entry_points_validate_on_host():
    """Every MCN_EINVAL case of mcn_attn_world_loss_grad and mcn_adam_step.  The pointers are fakes, so a check that
    went missing would launch a kernel on them: the calls are made in a fresh child process that sees NO device, where
    such a launch fails with MCN_ELAUNCH instead of faulting a GPU that others share."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "WORLD_TRAIN_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def _memory(N=5, rows=10):
    cur, nxt = R.pairs(rows, N, seed=3)
    return [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(rows)]


def test_fused_world_trainer_refuses_what_it_is_not_built_for():
    from modelcrowdnav_amd.policy.world_model import AttentionWorld, MlpWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    cpu = torch.device("cpu")
    assert Trainer_Sim.fused_default is False
    with pytest.raises(ValueError, match="dropout"):
        Trainer_Sim(MlpWorld(5), _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="default AttentionWorld"):
        Trainer_Sim(AttentionWorld(with_global_state=False), _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="default AttentionWorld"):
        Trainer_Sim(AttentionWorld(input_dim=6), _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="default AttentionWorld"):
        Trainer_Sim(torch.nn.Linear(20, 10), _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="not float32"):
        Trainer_Sim(AttentionWorld().double(), _memory(), cpu, 4, fused=True)
    narrow = AttentionWorld()
    narrow.mlp2[2] = torch.nn.Linear(100, 40)
    with pytest.raises(ValueError, match=r"mlp2\.2\.weight"):
        Trainer_Sim(narrow, _memory(), cpu, 4, fused=True)
    # the default model, but no GPU to run on
    with pytest.raises(ValueError, match="not a GPU"):
        Trainer_Sim(AttentionWorld(), _memory(), cpu, 4, fused=True)
    # the class default is what fused=None reads
    Trainer_Sim.fused_default = True
    try:
        with pytest.raises(ValueError, match="dropout"):
            Trainer_Sim(MlpWorld(5), _memory(), cpu, 4)
        assert Trainer_Sim(MlpWorld(5), _memory(), cpu, 4, fused=False).fused is False
    finally:
        Trainer_Sim.fused_default = False


def test_default_world_trainer_is_the_torch_path(golden_dir, tmp_path):
    """The scenario of tests/test_training_cpu.py::test_world_model_trainer_matches_reference_trainer
    (g20_trainer_sim.npz, the reference's own Trainer_Sim) with fused=False passed explicitly, and again with no
    argument: the recorded best losses, model.mse and early-stopping state to that test's 2e-5, and the two trainers
    bit for bit alike, with no fused state made."""
    from modelcrowdnav_amd.policy.world_model import AttentionWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    g = np.load(os.path.join(golden_dir, "g20_trainer_sim.npz"))
    load = lambda pref: {k[len(pref):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pref)}
    for tag, calls in (("short", (5, 3)), ("stop", (50,))):
        out = []
        for kw in ({"fused": False}, {}):
            model = AttentionWorld()
            model.load_state_dict(load("w0__"))
            nxt = g["next"] if tag == "short" else g["next_stop"]
            mem = [(torch.from_numpy(g["cur"][i]), torch.from_numpy(nxt[i])) for i in range(int(g[tag + "_rows"]))]
            tr = Trainer_Sim(model, mem, torch.device("cpu"), 1000, str(tmp_path / (tag + ".pt")), **kw)
            assert tr.fused is False
            tr.set_learning_rate(1e-3)
            random.seed(2000)
            bests = [tr.optimize_epoch(e, perms=(g["%s_call%d_train_perms" % (tag, c)], g["%s_call%d_val_perms" % (tag, c)]))
                     for c, e in enumerate(calls)]
            assert tr._fz is None and tr.last_rows is None
            np.testing.assert_allclose(bests, g[tag + "_best"], rtol=2e-5, atol=0)
            assert abs(model.mse - float(g[tag + "_mse"])) <= 2e-5 * float(g[tag + "_mse"])
            assert tr.early_stopping.counter == int(g[tag + "_counter"])
            assert bool(tr.early_stopping.early_stop) == bool(g[tag + "_stopped"])
            out.append((bests, [p.detach().clone() for p in model.parameters()]))
        assert out[0][0] == out[1][0] and all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
