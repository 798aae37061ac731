"""No GPU: the comparing code of tests/fused_train_harness.py itself, on hand-made arrays -- what tensor_errors returns,
what parity must report and what it must let pass, also for a tensor whose float64 gradient is exactly 0 -- and the
helpers whose result can be written down."""
import numpy as np
import pytest
import torch

from tests import fused_train_harness as F

# three tensors in a flat buffer of 9: a 2 x 3 weight, its bias, and the bias that has no gradient
LAYOUT = ([("mlp.weight", 0, (2, 3)), ("mlp.bias", 6, (2,)), ("attention.4.bias", 8, (1,))], 9)
G64 = np.array([1.0, -2.0, 0.5, 4.0, 0.25, -1.0, 0.5, -0.125, 0.0])


def _pair(loss, shift):
    """(loss, gradient): G64 with `shift` added, as the float64 arrays the helpers make of their inputs anyway."""
    return loss, G64 + np.asarray(shift, np.float64)


def test_tensor_errors_keeps_numerator_and_denominator_apart():
    shift = np.array([0.0, 0.25, 0.0, -0.5, 0.0, 0.0, 0.0, 0.125, 2.0 ** -20])
    e = F.tensor_errors(G64 + shift, G64, LAYOUT)
    assert e == {"mlp.weight": (0.5, 4.0), "mlp.bias": (0.125, 0.5), "attention.4.bias": (2.0 ** -20, 0.0)}
    assert F.tensor_errors(G64, G64, LAYOUT) == {"mlp.weight": (0.0, 4.0), "mlp.bias": (0.0, 0.5), "attention.4.bias": (0.0, 0.0)}
    f32 = F.tensor_errors((G64 + shift).astype(np.float32), G64, LAYOUT)          # float32 in, float64 arithmetic
    assert f32 == e
    with pytest.raises(AssertionError):
        F.tensor_errors(G64[:8], G64[:8], LAYOUT)                                  # not the layout's length
    with pytest.raises(AssertionError):
        F.tensor_errors(G64, G64[:8], LAYOUT)


def test_slot_finds_a_tensor_by_name():
    assert F.slot(LAYOUT, "mlp.weight") == (0, 6) and F.slot(LAYOUT, "mlp.bias") == (6, 2)
    assert F.slot(LAYOUT, "attention.4.bias") == (8, 1)
    with pytest.raises(KeyError):
        F.slot(LAYOUT, "mlp.2.bias")


def test_parity_passes_up_to_margin_times_torchs_error(capsys):
    ref = _pair(2.0, np.zeros(9))
    torch32 = _pair(2.0 + 2.0 ** -20, [2.0 ** -10] * 6 + [2.0 ** -12] * 2 + [2.0 ** -30])
    at_bound = _pair(2.0 - F.MARGIN * 2.0 ** -20, [-F.MARGIN * 2.0 ** -10] * 6 + [F.MARGIN * 2.0 ** -12] * 2 + [F.MARGIN * 2.0 ** -30])
    assert F.parity("at the bound", at_bound, torch32, ref, LAYOUT) == []
    assert F.parity("exact", ref, torch32, ref, LAYOUT) == []
    line = capsys.readouterr().out.splitlines()[0]
    # printed: the worst RELATIVE error among the tensors that have a gradient (mlp.bias: 4 x 2^-12 / 0.5), and the
    # absolute figures of attention.4.bias, whose float64 gradient is 0
    assert line.startswith("at the bound: loss err kernel %.3g torch %.3g | worst grad err kernel %.3g torch %.3g" %
                           (4 * 2.0 ** -21, 2.0 ** -21, 2.0 ** -9, 2.0 ** -11))
    assert line.endswith("attention.4.bias abs kernel %.3g torch %.3g float64 0" % (4 * 2.0 ** -30, 2.0 ** -30))


def test_parity_reports_each_tensor_and_the_loss_over_the_bound():
    ref = _pair(2.0, np.zeros(9))
    torch32 = _pair(2.0 + 2.0 ** -20, [2.0 ** -10] * 6 + [2.0 ** -12] * 2 + [2.0 ** -30])
    over = 1.01 * F.MARGIN
    bad = F.parity("w", _pair(2.0, [0, 0, over * 2.0 ** -10, 0, 0, 0, 0, 0, 0]), torch32, ref, LAYOUT)
    assert len(bad) == 1 and bad[0].startswith("w: mlp.weight kernel ") and "(max |g64| 4)" in bad[0]
    bad = F.parity("b", _pair(2.0, [0, 0, 0, 0, 0, 0, 0, -over * 2.0 ** -12, 0]), torch32, ref, LAYOUT)
    assert len(bad) == 1 and bad[0].startswith("b: mlp.bias kernel ")
    bad = F.parity("l", _pair(2.0 + over * 2.0 ** -20, np.zeros(9)), torch32, ref, LAYOUT)
    assert bad == ["l: loss kernel %.3g > %g x torch %.3g" % (over * 2.0 ** -21, F.MARGIN, 2.0 ** -21)]
    bad = F.parity("all", _pair(3.0, np.full(9, 1.0)), torch32, ref, LAYOUT)
    assert [b.split()[1] for b in bad] == ["mlp.weight", "mlp.bias", "attention.4.bias", "loss"]
    # NaN is over every bound, in a tensor and in the loss
    bad = F.parity("nan", _pair(np.nan, [0, np.nan, 0, 0, 0, 0, 0, 0, 0]), torch32, ref, LAYOUT)
    assert [b.split()[1] for b in bad] == ["mlp.weight", "loss"]


def test_parity_where_the_float64_gradient_is_exactly_zero():
    """The numerators are compared, so a tensor with max |g64| = 0 is still held to MARGIN times torch's ABSOLUTE error:
    an exact 0 passes whatever torch has, a kernel error passes only next to a torch error, and the printed worst
    relative error leaves the tensor out instead of dividing by 0."""
    ref = _pair(1.0, np.zeros(9))
    torch_exact = _pair(1.0 + 2.0 ** -22, [2.0 ** -12] * 8 + [0.0])
    torch_noise = _pair(1.0 + 2.0 ** -22, [2.0 ** -12] * 8 + [2.0 ** -30])
    assert F.parity("0 vs 0", ref, torch_exact, ref, LAYOUT) == []
    assert F.parity("0 vs noise", ref, torch_noise, ref, LAYOUT) == []
    noisy = _pair(1.0, [0] * 8 + [F.MARGIN * 2.0 ** -30])
    assert F.parity("noise vs noise", noisy, torch_noise, ref, LAYOUT) == []
    bad = F.parity("noise vs 0", noisy, torch_exact, ref, LAYOUT)
    assert len(bad) == 1 and bad[0].startswith("noise vs 0: attention.4.bias kernel ") and "(max |g64| 0)" in bad[0]
    bad = F.parity("more noise", _pair(1.0, [0] * 8 + [1.01 * F.MARGIN * 2.0 ** -30]), torch_noise, ref, LAYOUT)
    assert len(bad) == 1 and "attention.4.bias" in bad[0]


def test_ulps_counts_float32_spacings_of_the_reference():
    ref = np.array([1.0, 1.0, -2.0, 0.75, 1e-3], np.float32)
    got = ref.copy()
    got[1] = np.nextafter(np.float32(1.0), np.float32(2.0))
    got[2] = np.nextafter(np.nextafter(np.float32(-2.0), np.float32(-3.0)), np.float32(-3.0))
    got[3] = np.nextafter(np.float32(0.75), np.float32(0.0))
    assert F.ulps(got, ref).tolist() == [0.0, 1.0, 2.0, 1.0, 0.0]
    # a float64 reference is measured in the spacing of its float32 rounding
    ref64 = ref.astype(np.float64) + np.array([0.0, 2.0 ** -25, 0.0, 0.0, 0.0])
    assert F.ulps(ref, ref64).tolist() == [0.0, 0.25, 0.0, 0.0, 0.0]
    assert F.ulps(got, ref).dtype == np.float64 and F.SENTINEL == 12345.0 and F.MARGIN == 4.0


def test_yardstick_is_float64_autograd_of_the_same_module():
    """loss_and_grad64 on a small module against the gradient written out by hand; as64 copies (the module keeps its
    float32 weights and its .grad), flat follows the parameter order."""
    torch.manual_seed(0)
    model = torch.nn.Linear(3, 2)
    x, y = torch.randn(5, 3), torch.randn(5, 2)
    model.weight.grad = torch.ones_like(model.weight)
    loss, grad = F.loss_and_grad64(model, x, y)
    assert model.weight.dtype == torch.float32 and torch.equal(model.weight.grad, torch.ones_like(model.weight))
    w, b, x64, y64 = model.weight.detach().double(), model.bias.detach().double(), x.double(), y.double()
    d = x64 @ w.T + b - y64
    want = np.concatenate([(2.0 / d.numel() * d.T @ x64).numpy().reshape(-1), (2.0 / d.numel() * d.sum(0)).numpy()])
    assert grad.dtype == np.float64 and grad.shape == (8,)
    assert abs(loss - float((d * d).mean())) <= 1e-15 and np.abs(grad - want).max() <= 1e-15
    l32, g32 = F.loss_and_grad(model, x, y)                                        # the module as it is: float32
    assert g32.dtype == np.float32 and 0 < np.abs(g32 - want).max() < 1e-6 and abs(l32 - loss) < 1e-6
    assert np.array_equal(F.flat([model.weight, model.bias]), np.concatenate([w.float().numpy().reshape(-1), b.float().numpy()]))
    assert all(p.grad is None and p.dtype == torch.float64 for p in F.as64(model).parameters())
