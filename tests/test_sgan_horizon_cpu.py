"""CPU: the pieces around mcn_sgan_predict that need no GPU.

  * tests/sgan_horizon_ref.py (float64 numpy restatement of the generator for T decoder steps and K noise samples)
    against the reference's recorded outputs in tests/golden/g25_sgan_horizon.npz: at most 5e-6 per displacement (the
    reference's own float32 evaluation is at most 8.1e-7 from a float64 evaluation of its modules at T <= 12);
  * modelcrowdnav_amd/sgan/losses.py against the reference's displacement_error / final_displacement_error values;
  * the header, _hip.EXPORTED and the library agree on the new symbol, and every bad argument is rejected on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import sgan_horizon_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("S6_N5", "S3_N10", "S4_N1", "ragged")
TAGS = ("np", "p")
REF_TOL = 5e-6


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "g25_sgan_horizon.npz"))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag", TAGS)
def test_restatement_matches_reference_fixture(fixture, tag, case):
    key = "%s__%s__" % (tag, case)
    traj = fixture[key + "obs_traj"]
    assert traj.dtype == np.float32
    last, rel = R.inputs(traj.astype(np.float64))
    got = R.predict(R.weights64(tag), last, rel, fixture[key + "sizes"], fixture[key + "noise"], 12, tag == "p")
    for T in (8, 12):
        want = fixture[key + "T%d__pred_rel" % T]
        assert want.shape == (3, T, traj.shape[1], 2)
        err = float(np.abs(got[:, :T] - want).max())
        print("[%s %s T=%d] restatement - reference: %.3g" % (tag, case, T, err))
        assert err <= REF_TOL, err
        # relative_to_abs of the reference is a float32 cumsum: T additions of values below 1 near positions below 16
        np.testing.assert_allclose(R.positions(last, got[:, :T]), fixture[key + "T%d__pred_abs" % T], rtol=0,
                                   atol=T * (REF_TOL + 1e-6))
    assert float(np.abs(got).max()) > 0.1


def test_samples_and_steps_differ(fixture):
    """The fixture can tell samples and steps apart: the K futures of a scene differ, and so do its steps."""
    for tag in TAGS:
        pr = fixture["%s__S6_N5__T12__pred_rel" % tag]
        assert np.abs(pr[0] - pr[1]).max() > 1e-3 and np.abs(pr[1] - pr[2]).max() > 1e-3
        assert np.abs(pr[:, 0] - pr[:, 11]).max() > 1e-3


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag", TAGS)
def test_losses_match_reference_fixture(fixture, tag, case):
    from modelcrowdnav_amd.sgan.losses import displacement_error, final_displacement_error
    key = "%s__%s__" % (tag, case)
    mask = torch.from_numpy(fixture[key + "mask"])
    assert 0 < float(mask.sum()) < len(mask) or len(mask) < 6
    for T in (8, 12):
        gt = torch.from_numpy(fixture[key + "gt"][:T])
        pre = key + "T%d__" % T
        for k in range(3):
            pa = torch.from_numpy(fixture[pre + "pred_abs"][k])
            for mode in ("sum", "raw"):
                for sfx, cp in (("", None), ("_mask", mask)):
                    ade = displacement_error(pa, gt, cp, mode=mode)
                    fde = final_displacement_error(pa[-1], gt[-1], cp, mode=mode)
                    assert tuple(ade.shape) == (() if mode == "sum" else (pa.shape[1],))
                    np.testing.assert_allclose(ade.numpy(), fixture[pre + "ade_%s%s" % (mode, sfx)][k], rtol=1e-6, atol=0)
                    np.testing.assert_allclose(fde.numpy(), fixture[pre + "fde_%s%s" % (mode, sfx)][k], rtol=1e-6, atol=0)
    assert displacement_error(pa, gt).dtype == torch.float32                # defaults: no mask, mode 'sum'


def test_losses_are_aliased_for_drop_in_imports():
    from modelcrowdnav_amd import dropin
    table = next(v for v in vars(dropin).values() if isinstance(v, dict) and "sgan.models" in v)
    assert table["sgan.losses"] == "modelcrowdnav_amd.sgan.losses"


def test_header_binding_and_library_agree_on_the_symbol():
    from modelcrowdnav_amd import _hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcn.h")).read(), flags=re.S)
    decl = re.search(r"int\s+mcn_sgan_predict\s*\(([^)]*)\)", hdr)
    assert decl, "include/mcn.h does not declare mcn_sgan_predict"
    params = [p.strip() for p in decl.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["net", "hist", "oldest", "noise", "K", "T", "hcount", "workspace",
                                                           "out_rel", "out_pos", "E", "N", "stream"]
    assert "mcn_sgan_predict" in _hip.EXPORTED
    assert hasattr(C.CDLL(_hip.LIB_PATH), "mcn_sgan_predict")
    fn = _hip.lib.mcn_sgan_predict
    assert len(fn.argtypes) == len(params) and fn.restype is C.c_int
    for p, t in zip(params, fn.argtypes):
        assert (t is C.c_void_p) == ("*" in p), p
        assert (t is C.c_int32) == p.startswith("int32_t "), p
    assert _hip.lib.mcn_abi_version() == _hip.ABI_VERSION               # an added symbol does not move the ABI version


def test_bad_arguments_are_rejected_on_host():
    """Validation happens before any launch (the pointers are fakes that are never dereferenced)."""
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.sgan.models import _SganNet
    fake = 0x1000
    net = _SganNet(*([fake] * 14), 1)
    good = dict(net=C.byref(net), hist=fake, oldest=0, noise=fake, K=2, T=3, hcount=None, workspace=fake, out_rel=fake,
                out_pos=None, E=4, N=5, stream=None)
    bad = [dict(K=0), dict(K=-1), dict(K=65536), dict(T=0), dict(T=-3), dict(net=None), dict(hist=None), dict(noise=None),
           dict(workspace=None), dict(out_rel=None), dict(E=0), dict(N=0), dict(N=_hip.MAX_HUMANS + 1), dict(oldest=8),
           dict(oldest=-1)]
    for change in bad:
        args = dict(good, **change)
        assert _hip.lib.mcn_sgan_predict(*args.values()) == _hip.MCN_EINVAL, change
    for missing in ("w_elstm", "w_c1", "b_dlstm", "w_h2p", "w_p1"):       # a net without one of its layers
        broken = _SganNet(*([fake] * 14), 1)
        setattr(broken, missing, None)
        assert _hip.lib.mcn_sgan_predict(*dict(good, net=C.byref(broken)).values()) == _hip.MCN_EINVAL, missing
