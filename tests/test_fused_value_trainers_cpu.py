"""CPU: the host side of the fused LSTM-RL and CADRL training steps (csrc/value_train.hip; include/mcn.h:
mcn_{cadrl,lstm_rl}_train_param_count, _train_workspace_bytes, _loss_grad; utils/trainer.py: Trainer(fused=True)) -- the
flat layouts, the sizes, the argument validation (before any launch), the choice of the step by the model's class and the
refusals of the Python path.  The kernels themselves are tested on the device by tests/test_fused_value_trainers_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import value_trainer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = ("lstm_rl", "cadrl")     # the networks of value_train.hip (SARL's host side: tests/test_fused_trainer_cpu.py)
NEW_SYMBOLS = ["mcn_cadrl_train_param_count", "mcn_cadrl_train_workspace_bytes", "mcn_cadrl_loss_grad",
               "mcn_lstm_rl_train_param_count", "mcn_lstm_rl_train_workspace_bytes", "mcn_lstm_rl_loss_grad"]


def _count(policy):
    from modelcrowdnav_amd import _hip
    return int(getattr(_hip.lib, "mcn_%s_train_param_count" % policy)())


def test_library_exports_the_six_symbols():
    from modelcrowdnav_amd import _hip
    import ctypes
    fresh = ctypes.CDLL(_hip.LIB_PATH)                  # a handle without the binding's attributes: dlsym decides
    for name in NEW_SYMBOLS:
        assert name in _hip.EXPORTED and getattr(fresh, name) is not None, name


def _configured(policy):
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.policy.policy_factory import policy_factory
    torch.manual_seed(0)
    p = policy_factory[policy]()
    p.configure(configs.policy_config())
    return p.model


@pytest.mark.parametrize("policy", POLICIES)
def test_param_count_and_flat_layout_are_state_dict_order(policy):
    """The library's count, the hand-written table, the layout the Trainer uses, the seeded module's and the configured
    policy's own state_dict all agree: for LSTM-RL that pins the MLP before the four LSTM tensors."""
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    model = R.value_network(policy, seed=0)
    table, total = R.layout(policy)
    assert total == R.COUNT[policy] == _count(policy) == sum(p.numel() for p in model.parameters())
    assert total == sum(p.numel() for p in _configured(policy).parameters())
    for m in (model, _configured(policy)):
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, shp) for k, _, shp in table]
        assert [k for k, _ in m.named_parameters()] == [k for k, _, _ in table]
    tr = Trainer(model, ReplayMemory(4), torch.device("cpu"), 2)          # not fused: only its layout is asked for
    assert tr._fused_layout() == (table, total)
    numel = {k: v.numel() for k, v in model.state_dict().items()}
    assert table[0][1] == 0 and all(b[1] == a[1] + numel[a[0]] for a, b in zip(table[:-1], table[1:]))
    assert table[-1][0] == ("lstm.bias_hh_l0" if policy == "lstm_rl" else R.LAST_BIAS[policy])


def test_workspace_grows_with_the_batch():
    from modelcrowdnav_amd import _hip
    lib = _hip.lib
    sizes = [lib.mcn_cadrl_train_workspace_bytes(B) for B in range(1, 300)]
    assert sizes[0] >= 4 * (R.COUNT["cadrl"] + 1)
    assert all(b >= a > 0 for a, b in zip(sizes[:-1], sizes[1:]))
    assert lib.mcn_cadrl_train_workspace_bytes(0) == 0 and lib.mcn_cadrl_train_workspace_bytes(-4) == 0
    for N in (1, 2, 3, 4, 5, 10, 32):
        sizes = [lib.mcn_lstm_rl_train_workspace_bytes(B, N) for B in range(1, 130)]
        assert sizes[0] >= 4 * (R.COUNT["lstm_rl"] + 1)
        assert all(b >= a > 0 for a, b in zip(sizes[:-1], sizes[1:])), N
    assert lib.mcn_lstm_rl_train_workspace_bytes(0, 5) == 0
    assert lib.mcn_lstm_rl_train_workspace_bytes(4, 0) == 0
    assert lib.mcn_lstm_rl_train_workspace_bytes(4, _hip.MAX_HUMANS + 1) == 0 and _hip.MAX_HUMANS == 32


_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = C.c_void_p(0x1000)                     # never dereferenced: validation fails first


def cadrl(params=fake, states=fake, values=fake, rows=fake, B=4, ws=fake, g=fake, loss=fake):
    return lib.mcn_cadrl_loss_grad(params, states, values, rows, B, ws, g, loss, None)


def lstm(params=fake, states=fake, values=fake, rows=fake, B=4, N=5, ws=fake, g=fake, loss=fake):
    return lib.mcn_lstm_rl_loss_grad(params, states, values, rows, B, N, ws, g, loss, None)


# the acceptable calls get past validation and, with no device in sight, fail at the launch: each MCN_EINVAL below comes
# from the one argument that was changed (made only once the runtime itself confirms that it sees no device)
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert cadrl() == _hip.MCN_ELAUNCH and cadrl(rows=None) == _hip.MCN_ELAUNCH, "rows = NULL means rows 0 .. B-1"
    assert lstm() == _hip.MCN_ELAUNCH and lstm(rows=None) == _hip.MCN_ELAUNCH
    assert lstm(N=1, B=1) == _hip.MCN_ELAUNCH and lstm(N=_hip.MAX_HUMANS) == _hip.MCN_ELAUNCH
    print("POSITIVE_CONTROL_OK")
null = {"params = NULL": dict(params=None), "states = NULL": dict(states=None), "values = NULL": dict(values=None),
        "workspace = NULL": dict(ws=None), "grad = NULL": dict(g=None), "loss = NULL": dict(loss=None),
        "B = 0": dict(B=0), "B = -1": dict(B=-1)}
for what, kw in null.items():
    assert cadrl(**kw) == _hip.MCN_EINVAL, "cadrl " + what
    assert lstm(**kw) == _hip.MCN_EINVAL, "lstm_rl " + what
for what, kw in {"N = 0": dict(N=0), "N = -3": dict(N=-3), "N = MCN_MAX_HUMANS + 1": dict(N=_hip.MAX_HUMANS + 1)}.items():
    assert lstm(**kw) == _hip.MCN_EINVAL, "lstm_rl " + what
print("VALUE_TRAIN_VALIDATION_OK")
"""


def test_training_entry_points_validate_on_host():
    """Every MCN_EINVAL case of mcn_cadrl_loss_grad and mcn_lstm_rl_loss_grad.  The pointers are fakes, so a check that
    went missing would launch a kernel on them: the calls are made in a fresh child process that sees NO device, where
    such a launch fails with MCN_ELAUNCH instead of faulting a GPU that others share."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "VALUE_TRAIN_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:],
                                                                               res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def _memory(policy, N=5, rows=8):
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    s, v = R.states_and_values(policy, rows, N, seed=3)
    mem = ReplayMemory(32)
    mem.push_batch(s, v)
    return mem


@pytest.mark.parametrize("policy", POLICIES)
def test_fused_trainer_takes_the_shipped_model_and_only_that(policy):
    from modelcrowdnav_amd.policy.cadrl import ValueNetwork
    from modelcrowdnav_amd.policy.lstm_rl import ValueNetwork1
    from modelcrowdnav_amd.utils import trainer as T
    cpu = torch.device("cpu")
    model = R.value_network(policy, seed=0)
    # the class picks the step; with the shipped model and a clean memory the only thing missing is a GPU
    step, why = T._fused_step(model)
    assert why is None and step.name == "mcn_%s_loss_grad" % policy
    assert step.state_shape == ((None, 13) if policy == "lstm_rl" else (13,))
    with pytest.raises(ValueError, match="not a GPU"):
        T.Trainer(model, _memory(policy), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="not a GPU"):
        T.Trainer(_configured(policy), _memory(policy), cpu, 4, fused=True)
    # non-shipped widths
    if policy == "lstm_rl":
        others = [ValueNetwork1(13, 6, [150, 90, 100, 1], 50), ValueNetwork1(13, 6, [150, 100, 100, 1], 40),
                  ValueNetwork1(14, 6, [150, 100, 100, 1], 50), ValueNetwork1(13, 5, [150, 100, 100, 1], 51)]
        text = "shipped LSTM-RL ValueNetwork1"
    else:
        others = [ValueNetwork(13, [150, 90, 100, 1]), ValueNetwork(14, [150, 100, 100, 1]), ValueNetwork(13, [150, 100, 1])]
        text = "shipped CADRL ValueNetwork"
    for other in others:
        with pytest.raises(ValueError, match=text):
            T.Trainer(other, _memory(policy), cpu, 4, fused=True)
    with pytest.raises(ValueError, match="its parameters are not float32"):
        T.Trainer(R.value_network(policy, 0).double(), _memory(policy), cpu, 4, fused=True)
    # a memory of another state shape: the other network's, and a row of another width; both shapes are named
    wrong = _memory("cadrl" if policy == "lstm_rl" else "lstm_rl")
    takes = r"\[N <= 32\]\[13\]" if policy == "lstm_rl" else r"the model takes \[13\]"
    with pytest.raises(ValueError, match=r"memory states are \((13,|5, 13)\), " + ".*" + takes):
        T.Trainer(model, wrong, cpu, 4, fused=True)
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    wide = ReplayMemory(8)
    wide.push_batch(torch.zeros((4, 5, 14) if policy == "lstm_rl" else (4, 14)), torch.zeros(4))
    with pytest.raises(ValueError, match="memory states are"):
        T.Trainer(model, wide, cpu, 4, fused=True)
    # _odd rows
    odd = _memory(policy)
    odd.push((torch.zeros(3, 13) if policy == "lstm_rl" else torch.zeros(2, 13), torch.zeros(1)))
    assert odd._odd
    with pytest.raises(ValueError, match="_odd"):
        T.Trainer(model, odd, cpu, 4, fused=True)


def test_unknown_class_names_all_three_networks():
    from modelcrowdnav_amd.utils.trainer import Trainer
    with pytest.raises(ValueError) as e:
        Trainer(torch.nn.Linear(13, 1), _memory("cadrl"), torch.device("cpu"), 4, fused=True)
    for text in ("shipped SARL value network", "LSTM-RL ValueNetwork1", "CADRL ValueNetwork", "sarl_train.hip",
                 "value_train.hip", "Linear"):
        assert text in str(e.value), text


@pytest.mark.parametrize("policy", POLICIES)
def test_unfused_trainer_is_unaffected(policy):
    """fused=False (and the default) takes the torch path whatever the memory holds, and leaves no fused state."""
    from modelcrowdnav_amd.utils.trainer import Trainer
    out = []
    for kw in ({}, {"fused": False}):
        model = R.value_network(policy, seed=4)
        tr = Trainer(model, _memory(policy), torch.device("cpu"), 4, **kw)
        assert tr.fused is False
        tr._gen.manual_seed(9)
        tr.set_learning_rate(0.01)
        losses = [tr.optimize_batch(2), tr.optimize_epoch(1)]
        assert tr._fz is None and tr.last_rows is None and np.isfinite(losses).all()
        out.append((losses, [p.detach().clone() for p in model.parameters()]))
    assert out[0][0] == out[1][0] and all(torch.equal(a, b) for a, b in zip(out[0][1], out[1][1]))


def load_g26(policy, golden_dir, device, fused):
    """The recorded run of tests/golden/g26_value_trainers.npz for `policy`: (fixture, model at w0, states, values
    [100, 1], Trainer over a one-batch memory on `device`)."""
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    g = np.load(os.path.join(golden_dir, "g26_value_trainers.npz"))
    model = R.value_network(policy, seed=3)
    assert list(g[policy + "_keys"]) == list(model.state_dict().keys()) == [k for k, _, _ in R.layout(policy)[0]]
    model.load_state_dict({k: torch.from_numpy(g["%s_w0__%s" % (policy, k.replace(".", "__"))].copy())
                           for k in model.state_dict()})
    states, values = torch.from_numpy(g[policy + "_states"]), torch.from_numpy(g[policy + "_values"])
    mem = ReplayMemory(100, device=device) if device.type != "cpu" else ReplayMemory(100)
    mem.push_batch(states.to(device), values.reshape(-1).to(device))
    return g, model, states, values.reshape(-1, 1), Trainer(model.to(device), mem, device, 100, fused=fused)


@pytest.mark.parametrize("policy", POLICIES)
def test_default_trainer_matches_reference_trainer(policy, golden_dir):
    """The default torch path against the REAL reference Trainer on the reference's own ValueNetwork1 / ValueNetwork
    (tests/golden_tools/gen_golden_value_trainers.py): same weights, same one-batch memory, lr 0.01, three
    optimize_batch(1).  Weights and losses to 1e-6, as tests/test_training_cpu.py holds the SARL run.  Loading the fixture
    also pins the state_dict order the flat buffers of value_train.hip rely on."""
    torch.set_num_threads(1)
    g, model, _, _, tr = load_g26(policy, golden_dir, torch.device("cpu"), fused=False)
    tr.set_learning_rate(0.01)
    losses = [tr.optimize_batch(1) for _ in range(3)]
    np.testing.assert_allclose(losses, g[policy + "_losses"], rtol=0, atol=1e-6)
    for k, v in model.state_dict().items():
        want = g["%s_w1__%s" % (policy, k.replace(".", "__"))]
        np.testing.assert_allclose(v.numpy(), want, rtol=0, atol=1e-6, err_msg=k)
        assert not np.array_equal(want, g["%s_w0__%s" % (policy, k.replace(".", "__"))]), k
