"""What the tests of the fused training steps share (tests/test_fused_value_trainers_gpu.py with tests/value_trainer_ref.py,
tests/test_fused_world_trainer_gpu.py with tests/world_trainer_ref.py): the float64 yardstick of a loss and its gradient
-- the module itself in torch.float64 under torch autograd on the CPU -- and the comparing code, whose bound is a multiple
of what torch's own float32 path is away from that yardstick on the same inputs.  Nothing here touches a GPU or the HIP
library; a layout is the ([(state_dict key, offset, shape)], length) pair a ref module writes out by hand."""
import copy

import numpy as np
import torch

MARGIN = 4.0        # both float32 accumulations, differing in summation order only: workgroup partials against a GEMM
SENTINEL = 12345.0  # what the output buffers of a kernel call start as


def as64(model):
    m = copy.deepcopy(model).cpu().double()
    for p in m.parameters():
        p.grad = None
    return m


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors])


def loss_and_grad(model, inputs, targets):
    """torch autograd on `model` as it is (its dtype and device) with the MSE loss over all outputs: (loss as a Python
    float of the model's precision, flat gradient as a numpy array in state_dict order)."""
    for p in model.parameters():
        p.grad = None
    loss = torch.nn.functional.mse_loss(model(inputs), targets)
    loss.backward()
    return loss.detach().cpu().item(), flat([p.grad for p in model.parameters()])


def loss_and_grad64(model, inputs, targets):
    """The yardstick: loss and flat gradient of the float32 `model` on float32 inputs and targets, every operation in
    float64."""
    return loss_and_grad(as64(model), inputs.detach().cpu().double(), targets.detach().cpu().double())


def slot(layout, name):
    """(offset, length) of the tensor `name` in the flat buffers."""
    for k, off, shp in layout[0]:
        if k == name:
            return off, int(np.prod(shp))
    raise KeyError(name)


def tensor_errors(got_flat, want_flat, layout):
    """{state_dict key: (max |got - want|, max |want|)} over the tensors of the flat layout: numerator and denominator
    of the relative error max |got - want| / max |want|, kept apart because a tensor's float64 gradient can be exactly
    0 (one human: the softmax weight is 1 whatever the score, so attention gets no gradient), where the quotient is
    0 / 0 or x / 0.  Two errors against the same `want` compare by their numerators."""
    table, total = layout
    assert got_flat.shape == want_flat.shape == (total,)
    out = {}
    for name, off, shape in table:
        n = int(np.prod(shape))
        g, w = got_flat[off:off + n].astype(np.float64), want_flat[off:off + n].astype(np.float64)
        out[name] = (float(np.abs(g - w).max()), float(np.abs(w).max()))
    return out


def parity(what, kernel, torch32, ref64, layout):
    """The metric, on three (loss, flat gradient) pairs: per parameter tensor max |g - g64| / max |g64| and
    |loss - loss64| / |loss64|; the kernel's may be MARGIN times torch's float32 figure for the same inputs.  Both
    figures of a tensor share the denominator max |g64|, so the numerators are compared: the same inequality, and it
    still says something where the float64 gradient of a tensor is exactly 0 (attention with one human).  Returns what
    misses the bound, as text."""
    ek, et = tensor_errors(kernel[1], ref64[1], layout), tensor_errors(torch32[1], ref64[1], layout)
    lk, lt = abs(kernel[0] - ref64[0]) / abs(ref64[0]), abs(torch32[0] - ref64[0]) / abs(ref64[0])
    # printed: the worst tensor among those that HAVE a gradient (attention.4.bias has none: a common shift of the
    # scores does not move the softmax, its float64 "gradient" is 1e-19 of rounding noise; its absolute figures follow)
    rel = lambda e: max([num / den for num, den in e.values() if den > 1e-12])
    print("%s: loss err kernel %.3g torch %.3g | worst grad err kernel %.3g torch %.3g | attention.4.bias abs kernel %.3g "
          "torch %.3g float64 %.3g" % (what, lk, lt, rel(ek), rel(et), ek["attention.4.bias"][0], et["attention.4.bias"][0],
                                       ek["attention.4.bias"][1]))
    bad = ["%s kernel %.3g > %g x torch %.3g (max |g64| %.3g)" % (k, ek[k][0], MARGIN, et[k][0], ek[k][1])
           for k in ek if not ek[k][0] <= MARGIN * et[k][0]]
    if not lk <= MARGIN * lt:
        bad.append("loss kernel %.3g > %g x torch %.3g" % (lk, MARGIN, lt))
    return ["%s: %s" % (what, b) for b in bad]


def ulps(a, ref):
    """|a - ref| in units of the float32 spacing at ref, elementwise (ref float32, or float64 to be rounded to it)."""
    ref = np.asarray(ref)
    return np.abs(a.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
