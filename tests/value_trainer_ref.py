"""Float64 yardstick of the value networks' training steps (csrc/sarl_train.hip, csrc/value_train.hip): the SAME modules
(policy/sarl.py: ValueNetwork with 13 inputs, or 61 for OM-SARL; policy/lstm_rl.py: ValueNetwork1; policy/cadrl.py:
ValueNetwork; shipped dimensions) in torch.float64 with torch autograd on the CPU, the flat layouts written out by hand,
seeded inputs, k SGD-momentum steps in float64 by torch's own rule, and the comparing function of the gradient tests.
Every tolerance of tests/test_fused_value_trainers_gpu.py is measured against this; nothing here touches a GPU or the HIP
library's kernels."""
import numpy as np
import torch

from tests import fused_train_harness as F
from tests.fused_train_harness import MARGIN, as64, loss_and_grad, loss_and_grad64, tensor_errors, ulps  # noqa: F401

POLICIES = ("sarl", "sarl_om", "lstm_rl", "cadrl")
INPUT_DIM = {"sarl": 13, "sarl_om": 61, "lstm_rl": 13, "cadrl": 13}
COUNT = {"sarl": 96502, "sarl_om": 103702, "lstm_rl": 46851, "cadrl": 27401}
LAST_BIAS = {"sarl": "mlp3.6.bias", "sarl_om": "mlp3.6.bias", "lstm_rl": "mlp.6.bias", "cadrl": "value_network.6.bias"}
CADRL_G = 8         # states per workgroup of cadrl_loss_grad_kernel (value_train.hip)
SARL_SHIPPED = dict(mlp1=[150, 100], mlp2=[100, 50], mlp3=[150, 100, 100, 1], attention=[100, 100, 1])


def value_network(policy, seed):
    """The shipped-dimension module of `policy` with torch's default initialisation under `seed`, float32 on the CPU."""
    torch.manual_seed(seed)
    if policy in ("sarl", "sarl_om"):
        from modelcrowdnav_amd.policy.sarl import ValueNetwork
        s = SARL_SHIPPED
        return ValueNetwork(INPUT_DIM[policy], 6, s["mlp1"], s["mlp2"], s["mlp3"], s["attention"], True, 1.0, 4)
    if policy == "lstm_rl":
        from modelcrowdnav_amd.policy.lstm_rl import ValueNetwork1
        return ValueNetwork1(13, 6, [150, 100, 100, 1], 50)
    from modelcrowdnav_amd.policy.cadrl import ValueNetwork
    return ValueNetwork(13, [150, 100, 100, 1])


def layout(policy):
    """[(state_dict key, offset, shape)] of the flat parameter / gradient / momentum buffers and their length, written
    out by hand: state_dict order (LSTM-RL: the MLP first, then the four LSTM tensors), each tensor row-major as torch
    stores it."""
    head = lambda prefix, fan_in: [(prefix + ".0", fan_in, 150), (prefix + ".2", 150, 100), (prefix + ".4", 100, 100),
                                   (prefix + ".6", 100, 1)]
    if policy in ("sarl", "sarl_om"):
        dims = [("mlp1.0", INPUT_DIM[policy], 150), ("mlp1.2", 150, 100), ("mlp2.0", 100, 100), ("mlp2.2", 100, 50),
                ("attention.0", 200, 100), ("attention.2", 100, 100), ("attention.4", 100, 1)] + head("mlp3", 56)
    else:
        dims = head("mlp", 56) if policy == "lstm_rl" else head("value_network", 13)
    table, off = [], 0
    for name, fan_in, fan_out in dims:
        table.append((name + ".weight", off, (fan_out, fan_in)))
        off += fan_in * fan_out
        table.append((name + ".bias", off, (fan_out,)))
        off += fan_out
    if policy == "lstm_rl":
        for name, shape in (("lstm.weight_ih_l0", (200, 13)), ("lstm.weight_hh_l0", (200, 50)), ("lstm.bias_ih_l0", (200,)),
                            ("lstm.bias_hh_l0", (200,))):
            table.append((name, off, shape))
            off += int(np.prod(shape))
    return table, off


def states_and_values(policy, rows, N, seed):
    """`rows` memory rows, float32: randn states -- [rows, N, input_dim] whose robot columns (the first six) are shared by
    the rows of a state, as in a rotated joint state, for SARL, OM-SARL and LSTM-RL; one row [rows, 13] for CADRL (N is
    ignored) -- and randn values [rows, 1]."""
    g = torch.Generator().manual_seed(seed)
    if policy == "cadrl":
        return torch.randn(rows, 13, generator=g), torch.randn(rows, 1, generator=g)
    s = torch.randn(rows, N, INPUT_DIM[policy], generator=g)
    s[:, :, :6] = s[:, :1, :6]
    return s, torch.randn(rows, 1, generator=g)


def sgd64(model, states, values, batches, lr, momentum=0.9, buf=None):
    """k = len(batches) SGD-momentum steps in float64 from the float32 `model`'s weights (buf = momentum buf + grad with
    the first buf = grad, p = p - lr buf): step s trains on the memory rows batches[s].  Returns (losses [k], trained
    float64 module, momentum buffers)."""
    m = as64(model)
    s64, v64 = states.detach().cpu().double(), values.detach().cpu().double().reshape(-1, 1)
    losses = []
    for rows in batches:
        rows = torch.as_tensor(np.asarray(rows), dtype=torch.long)
        for p in m.parameters():
            p.grad = None
        loss = torch.nn.functional.mse_loss(m(s64[rows]), v64[rows])
        loss.backward()
        losses.append(loss.item())
        with torch.no_grad():
            grads = [p.grad.clone() for p in m.parameters()]
            buf = grads if buf is None else [momentum * b + g for b, g in zip(buf, grads)]
            for p, b in zip(m.parameters(), buf):
                p.sub_(lr * b)
    return losses, m, buf


def parity(what, policy, kernel, torch32, ref64):
    """The metric, on three (loss, flat gradient) pairs.  A tensor of more than one element: max |g - g64| of the kernel
    may be MARGIN times torch's float32 figure for the same tensor (numerators of the same relative error; where the
    float64 gradient is exactly 0 and torch's too, the kernel's must be).  The loss and the one-element last bias: within
    that bound OR within 1 float32 ulp of the float64 value -- a single number from torch can be right by chance, and a
    kernel that forms these in float64 and rounds once is within half an ulp.  SARL and OM-SARL keep the bound they were
    measured under, which has no second clause (fused_train_harness.parity: MARGIN times torch's figure for every tensor
    and for the loss).  Prints both sides' figures; returns what misses the bound, as text."""
    lay = layout(policy)
    if policy in ("sarl", "sarl_om"):
        return F.parity(what, kernel, torch32, ref64, lay)
    ek, et = tensor_errors(kernel[1], ref64[1], lay), tensor_errors(torch32[1], ref64[1], lay)
    lk, lt = abs(kernel[0] - ref64[0]), abs(torch32[0] - ref64[0])
    rel = lambda e: max([num / den for num, den in e.values() if den > 0] or [0.0])
    print("%s: loss err kernel %.3g torch %.3g | worst grad err kernel %.3g torch %.3g" %
          (what, lk / abs(ref64[0]), lt / abs(ref64[0]), rel(ek), rel(et)))
    bad = []
    for name, off, shape in lay[0]:
        ok = ek[name][0] <= MARGIN * et[name][0]
        if not ok and int(np.prod(shape)) == 1:
            ok = ulps(kernel[1][off:off + 1], ref64[1][off:off + 1]).max() <= 1.0
        if not ok:
            bad.append("%s kernel %.3g > %g x torch %.3g (max |g64| %.3g)" % (name, ek[name][0], MARGIN, et[name][0], ek[name][1]))
    if not (lk <= MARGIN * lt or ulps(np.float32([kernel[0]]), np.float64([ref64[0]])).max() <= 1.0):
        bad.append("loss kernel %.3g > %g x torch %.3g and more than 1 ulp from float64" % (lk, MARGIN, lt))
    return ["%s: %s" % (what, b) for b in bad]
