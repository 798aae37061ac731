"""No GPU: the comparing code of tests/rollout_harness.py itself, on a stand-in env of small CPU tensors, and the helpers
whose result can be written down: the cut lists, the resource-table parser on the recorded tables, the oracle replay
with pool restarts on the inputs of tests/test_rollout_wg4_gpu.py."""
import os
import types

import numpy as np
import pytest

from oracle import cport
from tests import rollout_harness as RH


def _stand_in(with_roll=True):
    """SNAP_FIELDS as float64 tensors of different shapes and contents; rollout_buffers holds more than ROLL_FIELDS."""
    import torch
    env = types.SimpleNamespace(_roll=object() if with_roll else None)
    for i, k in enumerate(RH.SNAP_FIELDS):
        setattr(env, k, torch.arange(1, 3 + i, dtype=torch.float64) * (i + 1))
    env.rollout_buffers = dict(state=torch.arange(12, dtype=torch.float64).reshape(3, 4),
                               fin_return=torch.full((2, 3), 0.5, dtype=torch.float64),
                               fin_time=torch.full((2, 3), 7.25, dtype=torch.float64),
                               fin_info=torch.arange(6, dtype=torch.uint8).reshape(2, 3),
                               fin_count=torch.zeros(3, dtype=torch.int32), disc=torch.ones(5, dtype=torch.float64))
    return env


def test_snapshot_holds_the_fields_and_copies_them():
    env = _stand_in()
    snap = RH.snapshot(env)
    assert sorted(snap) == sorted(RH.SNAP_FIELDS + tuple("roll_" + k for k in RH.ROLL_FIELDS))
    assert sorted(RH.snapshot(_stand_in(with_roll=False))) == sorted(RH.SNAP_FIELDS)
    assert len(RH.SNAP_FIELDS) == 13 and RH.ROLL_FIELDS == ("state", "fin_return", "fin_time", "fin_info")
    before = {k: v.copy() for k, v in snap.items()}
    for k in RH.SNAP_FIELDS:
        getattr(env, k).add_(1.0)
    for v in env.rollout_buffers.values():
        v.add_(1)
    RH.assert_same_bytes(snap, before)
    with pytest.raises(AssertionError):
        RH.assert_same_bytes(RH.snapshot(env), before)


def _raises_naming(a, b, key):
    with pytest.raises(AssertionError) as err:
        RH.assert_same_bytes(a, b, "what")
    assert repr(key) in str(err.value) and "what" in str(err.value), str(err.value)


def test_one_byte_anywhere_is_seen():
    snap = RH.snapshot(_stand_in())
    RH.assert_same_bytes(snap, {k: v.copy() for k, v in snap.items()})
    for key in snap:
        other = {k: v.copy() for k, v in snap.items()}
        other[key].view(np.uint8).reshape(-1)[-1] ^= 1
        _raises_naming(snap, other, key)
        _raises_naming(other, snap, key)


def test_zero_signs_and_nan_payloads_are_bytes():
    snap = RH.snapshot(_stand_in())
    a, b = dict(snap, hvel=np.array([0.0, 1.0])), dict(snap, hvel=np.array([-0.0, 1.0]))
    assert np.array_equal(a["hvel"], b["hvel"])
    _raises_naming(a, b, "hvel")
    nan = np.array([0x7FF8000000000000, 0x7FF8000000000001], np.uint64).view(np.float64)
    assert np.isnan(nan).all()
    a, b = dict(snap, gtime=nan[:1].copy()), dict(snap, gtime=nan[1:].copy())
    RH.assert_same_bytes(a, dict(snap, gtime=nan[:1].copy()))
    _raises_naming(a, b, "gtime")


def test_missing_and_extra_keys_are_seen():
    snap = RH.snapshot(_stand_in())
    less = {k: v for k, v in snap.items() if k != "roll_fin_info"}
    for a, b in ((snap, less), (less, snap)):
        _raises_naming(a, b, "roll_fin_info")
    # what the unguarded copies compared when one env had no rollout attached
    _raises_naming(snap, RH.snapshot(_stand_in(with_roll=False)), "roll_state")


def test_every_cut():
    assert RH.every_cut(1) == [(0, 1)]
    assert RH.every_cut(2) == [(0, 2), (0, 1, 2)]
    assert RH.every_cut(3) == [(0, 3), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3)]
    cuts = RH.every_cut(8)
    assert cuts == [(0, 8)] + [(0, c, 8) for c in range(1, 8)] + [(0, 1, 2, 3, 4, 5, 6, 7, 8)]
    assert len(cuts) == 9 and all(c[0] == 0 and c[-1] == 8 and list(c) == sorted(set(c)) for c in cuts)


def test_parse_resources_on_the_recorded_tables():
    read = lambda name: open(os.path.join(RH.ROOT, "profiles", name)).read()
    txt = read("r17_kernel_resources.txt")
    rows = RH.parse_resources(txt[txt.index("# after, every kernel:"):])
    assert len(rows) > 150
    assert all(len(r) == 6 and all(type(v) is int for v in r) for r in rows.values())
    name = "void mcn::env_pair_kernel<5, true>(mcn::StepParams)"
    assert rows[name] == (66, 0, 96, 0, 6656, 0)                  # vgpr, agpr, sgpr, scratch, lds, vspill
    r13 = RH.parse_resources(read("r13_kernel_resources.txt"))
    quad = {k: v for k, v in r13.items() if k.startswith("void mcn::env_rollout_quad_kernel<")}
    assert len(quad) == 36
    assert quad["void mcn::env_rollout_quad_kernel<1, 0, true, true>(mcn::StepParams, int)"] == (133, 0, 106, 0, 768, 0)
    assert RH.parse_resources("no table here\n") == {}


def test_oracle_rollout_reaches_the_rare_paths_of_the_straddling_envs():
    """E = 9, P = 16, first restart from case (e + 7) % 16, stride 3, the robot walking up the middle into the packed
    pool: envs 3 and 6 each enter the 3-D LP, have a counted overlap and restart; an env replayed alone gives what it
    gives inside the batch."""
    from modelcrowdnav_amd.envs import scenarios as S
    E, T, P, N = 9, 60, 16, 5
    spec, cfg = S.ScenarioSpec(), cport.default_cfg(robot_visible=0)
    pool = RH.packed_pool(spec, P, N)
    plain = S.scenario_pool(spec, "test", range(P), N, "circle_crossing")
    assert np.array_equal(pool[0::2], plain[0::2]) and np.array_equal(pool[1::2, :, S.PX], plain[1::2, :, S.PX] * 0.12)
    rng = np.random.RandomState(11)
    acts = np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
    st, ref, restarts, overlaps, lp3 = RH.oracle_rollout(spec, cfg, pool, np.arange(E), acts, 7, 3)
    assert st.E == E and restarts.shape == overlaps.shape == (E,) and lp3 > 0
    for e in (3, 6):
        st1, ref1, r1, o1, lp3_1 = RH.oracle_rollout(spec, cfg, pool, [e], acts, 7, 3)
        assert lp3_1 > 0, "env %d never enters the 3-D LP" % e
        assert o1[0] > 0, "env %d has no counted overlap" % e
        assert r1[0] > 0, "env %d never restarts" % e
        assert (r1[0], o1[0]) == (restarts[e], overlaps[e])
        for k in ("hpx", "hpy", "hgx", "hr", "rpx", "rpy", "gtime"):
            assert np.array_equal(getattr(st1, k)[0], getattr(st, k)[e], equal_nan=True), (e, k)
        assert ref1["reward"][0] == ref["reward"][e]
