"""CPU: the host side of the fused MlpWorld training step (csrc/world_mlp_train.hip, csrc/dropout_hash.hpp; include/mcn.h:
mcn_dropout_mask, mcn_mlp_world_train_param_count, mcn_mlp_world_train_workspace_bytes, mcn_mlp_world_loss_grad;
utils/trainer_sim.py: Trainer_Sim(fused=True) on an MlpWorld) -- the mask's definition, the flat layout, the sizes, the
argument validation (before any launch), the refusals of the Python path, and that the default path is the one it was.
The kernel itself is tested on the device by tests/test_fused_mlp_world_trainer_gpu.py."""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mlp_world_trainer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcn_dropout_mask", "mcn_mlp_world_train_param_count", "mcn_mlp_world_train_workspace_bytes",
         "mcn_mlp_world_loss_grad"]
# (seed, step, layer, slot, unit) -> r >> 40, from plain Python integers (include/mcn.h)
VECTORS = [((0, 0, 0, 0, 0), 10946269), ((0, 0, 1, 0, 0), 4634430), ((0, 1, 0, 0, 0), 15607633), ((1, 0, 0, 0, 0), 6177195),
           ((12345, 7, 1, 99, 127), 13549691), ((2 ** 64 - 1, 2 ** 40, 1, 3, 63), 822369)]
THRESHOLDS = [(0.5, 8388608), (0.1, 15099494), (0.9, 1677722), (0.0, 16777216)]


def _lib_mask(seed, step, layer, B, width, p):
    from modelcrowdnav_amd import _hip
    keep = np.full((B, width), 7, np.uint8)
    rc = _hip.lib.mcn_dropout_mask(seed % 2 ** 64, step % 2 ** 64, layer, B, width, p, keep.ctypes.data)
    assert rc == _hip.MCN_OK
    return keep


def _python_bits(seed, step, layer, slot, unit):
    """The definition once more, on Python integers."""
    M = 2 ** 64 - 1

    def mix(z):
        z ^= z >> 30
        z = z * 0xBF58476D1CE4E5B9 & M
        z ^= z >> 27
        z = z * 0x94D049BB133111EB & M
        return z ^ (z >> 31)
    key = mix(seed + 0x9E3779B97F4A7C15 * (2 * step + layer + 1) & M)
    return mix(key + 0x9E3779B97F4A7C15 * (256 * slot + unit + 1) & M) >> 40


def test_the_four_symbols_are_exported():
    from modelcrowdnav_amd import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for n in NAMES:
        assert n in _hip.EXPORTED and hasattr(lib, n), n
    hdr = open(os.path.join(ROOT, "include", "mcn.h")).read()
    assert all(n + "(" in hdr for n in NAMES)


def test_param_count_and_flat_layout_are_the_modules():
    """538 N + 9164 floats in state_dict order: the library's count, the hand-written table of
    tests/mlp_world_trainer_ref.py, the module's own state_dict and the layout the trainer uses."""
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    count = _hip.lib.mcn_mlp_world_train_param_count
    for N in (1, 5, 10, 32):
        model = R.mlp_world(N, 0)
        table, total = R.layout(N)
        assert count(N) == 538 * N + 9164 == total == sum(p.numel() for p in model.parameters())
        assert len(table) == 8 and table[0][0] == "mlp.0.weight" and table[-1][0] == "mlp.8.bias"
        assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, shp) for k, _, shp in table]
        assert [k for k, _ in model.named_parameters()] == [k for k, _, _ in table]
        tr = Trainer_Sim(model, [], torch.device("cpu"), 2)               # not fused: only its layout is asked for
        assert tr._fused_layout() == (table, total)
    assert count(5) == 11854
    assert count(0) == 0 and count(-1) == 0 and count(_hip.MAX_HUMANS + 1) == 0 and _hip.MAX_HUMANS == 32


def test_workspace_grows_with_the_batch_and_refuses_bad_shapes():
    from modelcrowdnav_amd import _hip
    ws = _hip.lib.mcn_mlp_world_train_workspace_bytes
    for N in (1, 5, 10, 32):
        sizes = [ws(B, N) for B in range(1, 130)]
        assert sizes[0] >= 4 * R.param_count(N) + 8 * (1 + 2 * N) and all(s % 8 == 0 for s in sizes)
        assert all(b >= a > 0 for a, b in zip(sizes[:-1], sizes[1:])), N
        assert sizes[R.GROUP] > sizes[R.GROUP - 1] == sizes[0]             # one slice per workgroup of GROUP scenes
    assert ws(0, 5) == 0 and ws(-1, 5) == 0 and ws(4, 0) == 0 and ws(4, -2) == 0 and ws(4, _hip.MAX_HUMANS + 1) == 0
    assert ws(2 ** 31 - 1, 5) == 0                                         # more workgroups than the step launches


def test_the_definitions_test_vectors():
    """The six vectors and the thresholds of include/mcn.h: from Python integers, from the numpy restatement and from
    the library (a unit is kept exactly where its 24 bits are below T: probed with p = 0.5 on both sides of 2^23)."""
    for args, want in VECTORS:
        assert _python_bits(*args) == want, args
        seed, step, layer, slot, unit = args
        assert int(R.hash_bits(seed, step, layer, [slot], [unit])[0, 0]) == want, args
        got = _lib_mask(seed, step, layer, slot + 1, unit + 1, 0.5)
        assert got.shape == (slot + 1, unit + 1) and int(got[slot, unit]) == int(want < 8388608), args
    for p, want in THRESHOLDS:
        assert R.threshold(p) == want
    bits = "".join(str(int(b)) for b in _lib_mask(0, 1, 0, 1, 32, 0.5)[0])
    assert bits == "00011010100011011111101011010100"
    assert "".join(str(int(b)) for b in R.keep_mask(0, 1, 0, 1, 32, 0.5)[0]) == bits


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.9])
def test_library_mask_is_the_numpy_restatement_bit_for_bit(p):
    """mcn_dropout_mask against tests/mlp_world_trainer_ref.py: the neighbourhoods of the six test vectors (the
    vector's own slot and unit as the last ones of a [slot + 1, unit + 1] mask, the steps and seeds next to it, both
    layers) and the [100 x 128] and [7 x 64] masks of the two layers.  p reaches the library as float32 and the
    restatement as the decimal that was written."""
    for (seed, step, layer, slot, unit), _ in VECTORS:
        for ds, dt in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            s, t = (seed + ds) % 2 ** 64, (step + dt) % 2 ** 64
            for lay in (0, 1):
                B, W = slot + 2, min(unit + 2, 256)
                assert np.array_equal(_lib_mask(s, t, lay, B, W, p), R.keep_mask(s, t, lay, B, W, p)), (s, t, lay)
    for seed in (0, 1, 12345):
        for step in (0, 1, 19):
            for layer, (B, W) in enumerate(((100, 128), (7, 64))):
                got = _lib_mask(seed, step, layer, B, W, p)
                assert np.array_equal(got, R.keep_mask(seed, step, layer, B, W, p)), (seed, step, layer)
                assert set(np.unique(got)) <= {0, 1}
                if p == 0.0:
                    assert got.all()


def test_kept_share_and_independence_of_neighbouring_masks():
    """Seeds 0, 1 and 12345, steps 0 .. 19, both layers, [100 x 128] masks: the kept share is within 5 binomial standard
    deviations of 1 - p at p = 0.5, 0.1 and 0.9 -- for the library's masks and for the restated definition alike -- and
    masks of neighbouring steps, layers and seeds agree in half of their bits, within 5 standard deviations."""
    n = 100 * 128
    for p in (0.5, 0.1, 0.9):
        sd = (p * (1.0 - p) / n) ** 0.5
        for seed in (0, 1, 12345):
            for step in range(20):
                for layer in (0, 1):
                    for what, m in (("library", _lib_mask(seed, step, layer, 100, 128, p)),
                                    ("definition", R.keep_mask(seed, step, layer, 100, 128, p))):
                        share = float(m.mean())
                        assert abs(share - (1.0 - p)) <= 5.0 * sd, (what, p, seed, step, layer, share)
    sd = 0.5 / n ** 0.5
    for seed in (0, 1, 12345):
        for step in range(19):
            a = _lib_mask(seed, step, 0, 100, 128, 0.5)
            for what, b in (("next step", _lib_mask(seed, step + 1, 0, 100, 128, 0.5)),
                            ("other layer", _lib_mask(seed, step, 1, 100, 128, 0.5)),
                            ("next seed", _lib_mask(seed + 1, step, 0, 100, 128, 0.5))):
                agree = float((a == b).mean())
                assert abs(agree - 0.5) <= 5.0 * sd, (what, seed, step, agree)


def test_dropout_mask_validates_its_arguments():
    from modelcrowdnav_amd import _hip
    keep = np.zeros((4, 256), np.uint8)

    def call(seed=1, step=2, layer=0, B=4, width=256, p=0.5, out=keep.ctypes.data):
        return _hip.lib.mcn_dropout_mask(seed, step, layer, B, width, p, out)
    assert call() == _hip.MCN_OK and call(layer=1, width=1, B=1, p=0.0) == _hip.MCN_OK
    assert call(seed=2 ** 64 - 1, step=2 ** 64 - 1) == _hip.MCN_OK
    bad = {"keep = NULL": dict(out=None), "B = 0": dict(B=0), "B = -1": dict(B=-1), "width = 0": dict(width=0),
           "width = 257": dict(width=257), "width = -1": dict(width=-1), "layer = -1": dict(layer=-1),
           "layer = 2": dict(layer=2), "p = 1": dict(p=1.0), "p = -0.1": dict(p=-0.1), "p = 1.5": dict(p=1.5),
           "p = nan": dict(p=float("nan")), "p = inf": dict(p=float("inf"))}
    for what, kw in bad.items():
        assert call(**kw) == _hip.MCN_EINVAL, what


_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = C.c_void_p(0x1000)                     # never dereferenced: validation fails first
inf, nan = float("inf"), float("nan")


def grad(params=fake, cur=fake, nxt=fake, rows=fake, B=4, N=5, p=0.5, seed=1, step=2, ws=fake, g=fake, loss=fake):
    return lib.mcn_mlp_world_loss_grad(params, cur, nxt, rows, B, N, p, seed, step, ws, g, loss, None)


# the acceptable calls get past validation and, with no device in sight, fail at the launch: each MCN_EINVAL below comes
# from the one argument that was changed (made only once the runtime itself confirms that it sees no device)
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert grad() == _hip.MCN_ELAUNCH
    assert grad(rows=None) == _hip.MCN_ELAUNCH, "rows = NULL means rows 0 .. B-1"
    assert grad(g=None) == _hip.MCN_ELAUNCH, "grad = NULL means the eval-mode loss only"
    assert grad(N=_hip.MAX_HUMANS, B=1) == _hip.MCN_ELAUNCH and grad(N=1, B=1) == _hip.MCN_ELAUNCH
    assert grad(p=0.0) == _hip.MCN_ELAUNCH and grad(p=0.999, seed=2 ** 64 - 1, step=2 ** 64 - 1) == _hip.MCN_ELAUNCH
    print("POSITIVE_CONTROL_OK")
bad_grad = {
    "params = NULL": dict(params=None), "cur = NULL": dict(cur=None), "nxt = NULL": dict(nxt=None),
    "workspace = NULL": dict(ws=None), "loss = NULL": dict(loss=None),
    "B = 0": dict(B=0), "B = -1": dict(B=-1), "N = 0": dict(N=0), "N = -3": dict(N=-3),
    "N = MCN_MAX_HUMANS + 1": dict(N=_hip.MAX_HUMANS + 1),
    "drop_p = 1": dict(p=1.0), "drop_p = -0.1": dict(p=-0.1), "drop_p = 1.5": dict(p=1.5),
    "drop_p = nan": dict(p=nan), "drop_p = inf": dict(p=inf), "drop_p = -inf": dict(p=-inf),
    "drop_p = nan, forward only": dict(p=nan, g=None), "drop_p = 1, forward only": dict(p=1.0, g=None),
}
for what, kw in bad_grad.items():
    assert grad(**kw) == _hip.MCN_EINVAL, what
print("MLP_WORLD_TRAIN_VALIDATION_OK")
"""


def test_training_entry_point_validates_on_host():
    """Every MCN_EINVAL case of mcn_mlp_world_loss_grad.  The pointers are fakes, so a check that went missing would
    launch a kernel on them: the calls are made in a fresh child process that sees NO device, where such a launch fails
    with MCN_ELAUNCH instead of faulting a GPU that others share."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "MLP_WORLD_TRAIN_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def _memory(N=5, rows=10):
    cur, nxt = R.pairs(rows, N, seed=3)
    return [(cur[i].reshape(N, 4), nxt[i].reshape(N, 2)) for i in range(rows)]


def test_fused_mlp_world_trainer_refuses_what_it_is_not_built_for():
    """The refusals come in this order: the model (layers, dtype, count, dropout rates), then the device.  On the CPU
    device a model that passes the first reaches the second, whose text names the dropout masks."""
    from modelcrowdnav_amd.policy.world_model import MlpWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    cpu = torch.device("cpu")
    uneven = MlpWorld(5)
    uneven.mlp[5] = torch.nn.Dropout(0.25)
    with pytest.raises(ValueError, match="dropout rates"):
        Trainer_Sim(uneven, _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
        Trainer_Sim(MlpWorld(5, drop_rate=1.0), _memory(), cpu, 4, fused=True)
    narrow = MlpWorld(5)
    narrow.mlp[3] = torch.nn.Linear(128, 60)
    narrow.mlp[6] = torch.nn.Linear(60, 12)
    with pytest.raises(ValueError, match=r"mlp\.3\.weight"):
        Trainer_Sim(narrow, _memory(), cpu, 4, fused=True)
    odd_in = MlpWorld(5)
    odd_in.mlp[0] = torch.nn.Linear(18, 128)
    with pytest.raises(ValueError, match="not 4 N"):
        Trainer_Sim(odd_in, _memory(), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="not float32"):
        Trainer_Sim(MlpWorld(5).double(), _memory(), cpu, 4, fused=True)
    for p in (0.5, 0.0):
        with pytest.raises(ValueError, match="draws its dropout masks on the device; the trainer's device is cpu, not a GPU"):
            Trainer_Sim(MlpWorld(5, drop_rate=p), _memory(), cpu, 4, fused=True)


def test_pairs_of_another_crowd_size_are_refused(monkeypatch):
    """A model built for 5 pedestrians and a memory of 3: refused at the call, before anything is launched (the device
    check is stepped over here, since this test has no GPU; nothing after the refusal would run)."""
    from modelcrowdnav_amd.policy.world_model import MlpWorld
    from modelcrowdnav_amd.utils import trainer_sim
    real = trainer_sim._fused_step

    def check_model_only(self):
        self._step_hip, why = real(self)
        assert why is None
    monkeypatch.setattr(trainer_sim.Trainer_Sim, "_fused_check", check_model_only)
    tr = trainer_sim.Trainer_Sim(MlpWorld(5), _memory(N=3), torch.device("cpu"), 4, fused=True)
    tr.set_learning_rate(1e-3)
    with pytest.raises(ValueError, match="the pairs hold 3 pedestrians, the model is built for 5"):
        tr.optimize_epoch(1)
    assert tr._fz is None and tr.mask_step == 0


def test_default_mlp_world_trainer_is_the_torch_path(golden_dir, tmp_path):
    """The reference's own Trainer_Sim on MlpWorld(5, drop_rate=0.0) (g27_mlp_world_trainer.npz) with fused=False passed
    explicitly, and again with no argument: the recorded best losses, model.mse and early-stopping state to 2e-5, the
    two trainers bit for bit alike, and no fused state made."""
    from modelcrowdnav_amd.policy.world_model import MlpWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    g = np.load(os.path.join(golden_dir, "g27_mlp_world_trainer.npz"))
    load = lambda pref: {k[len(pref):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(pref)}
    out = []
    for kw in ({"fused": False}, {}):
        model = MlpWorld(5, drop_rate=0.0)
        model.load_state_dict(load("w0__"))
        mem = [(torch.from_numpy(g["cur"][i]), torch.from_numpy(g["next"][i])) for i in range(int(g["short_rows"]))]
        tr = Trainer_Sim(model, mem, torch.device("cpu"), 1000, str(tmp_path / "short.pt"), **kw)
        assert tr.fused is False
        tr.set_learning_rate(1e-3)
        random.seed(2000)
        bests = [tr.optimize_epoch(e, perms=(g["short_call%d_train_perms" % c], g["short_call%d_val_perms" % c]))
                 for c, e in enumerate((5, 3))]
        assert tr._fz is None and tr.last_rows is None and tr.mask_step == 0 and tr.dropout_seed is None
        np.testing.assert_allclose(bests, g["short_best"], rtol=2e-5, atol=0)
        assert abs(model.mse - float(g["short_mse"])) <= 2e-5 * float(g["short_mse"])
        assert tr.early_stopping.counter == int(g["short_counter"])
        assert bool(tr.early_stopping.early_stop) == bool(g["short_stopped"])
        want = load("short_w1__")
        assert all(float((v - want[k]).abs().max()) <= 2e-5 for k, v in model.state_dict().items())
        out.append((bests, [p.detach().clone() for p in model.parameters()]))
    assert out[0][0] == out[1][0] and all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))
