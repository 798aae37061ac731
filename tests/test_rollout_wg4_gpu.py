"""The four-wavefront form of the fused rollout launch (mcn_tuning.rollout_split = 2: workgroups of 8 envs, three ORCA
wavefronts for their 40 quads and one float64 wavefront with a lane per (env, human); built for 5 humans and an
invisible robot, both robot kinematics) against T mcn_env_step calls, against the C oracle's trajectory and against the
other two forms, bit for bit.  The forms share one mcn_last_dispatch family and give the same bytes, so every test that
forces the form also asserts mcn_last_rollout_form() == 2: the four-wavefront kernel is what was launched."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H

N = 5                                   # the only crowd size the form is instantiated for (robot invisible)
_FIELDS = ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal", "rtheta", "gtime", "human_times",
           "step_rec", "human_act")
_ROLL = ("state", "fin_return", "fin_time", "fin_info")


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _rollout_env(E, with_pool, kinematics="holonomic", fin_slots=2):
    from modelcrowdnav_amd.envs import scenarios as S
    env = H.make_vec_env(E, N, robot_visible=False, kinematics=kinematics)
    pool = S.scenario_pool(env.spec(), "test", range(64), N, "circle_crossing")
    ids = np.arange(E) % 64
    env.load_scenarios(pool[ids])
    env.attach_rollout(gamma=0.9, pool=pool if with_pool else None, case_stride=3, first_cases=(ids + 7) % 64,
                       fin_slots=fin_slots)
    return env


def _snapshot(env):
    c = lambda t: t.detach().cpu().numpy().copy()
    snap = {k: c(getattr(env, k)) for k in _FIELDS}
    snap.update({"roll_" + k: c(v) for k, v in env.rollout_buffers.items() if k in _ROLL})
    return snap


def _actions(kinematics, T, E, seed):
    rng = np.random.RandomState(seed)
    if kinematics == "unicycle":
        return np.stack([rng.uniform(0, 1, (T, E)), rng.uniform(-np.pi / 4, np.pi / 4, (T, E))], -1)
    sp, aa = rng.uniform(0, 1, (T, E)), rng.uniform(0, 2 * np.pi, (T, E))
    return np.stack([sp * np.cos(aa), sp * np.sin(aa)], -1)


_single_steps = {}


def _single_step_reference(E, with_pool, kinematics, T):
    """T mcn_env_step calls on the shared action sequence, computed once per configuration and left unchanged."""
    torch = _torch()
    key = (E, with_pool, kinematics)
    if key not in _single_steps:
        b = _rollout_env(E, with_pool, kinematics)
        acts_d = torch.from_numpy(_actions(kinematics, T, E, 5)).to(b.device)
        for t in range(T):
            b.step(acts_d[t])
        torch.cuda.synchronize()
        _single_steps[key] = _snapshot(b)
    return _single_steps[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("with_pool", [True, False])
@pytest.mark.parametrize("E", [1, 7, 8, 9, 1000])
def test_wg4_launch_equals_single_steps(E, with_pool, kinematics, tuning):
    """Less than one workgroup, exactly one, one plus a ragged tail, many ragged: every byte of state, step record,
    Explorer record and finished-episode records after launches of 30 + 1 + 79 steps equals 110 single steps; every
    env passes the time limit, so each finishes (and, with the pool, restarts) inside the sequence."""
    torch = _torch()
    from modelcrowdnav_amd import _hip
    T = 110
    ref = _single_step_reference(E, with_pool, kinematics, T)
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    a = _rollout_env(E, with_pool, kinematics)
    acts_d = torch.from_numpy(_actions(kinematics, T, E, 5)).to(a.device)
    a.rollout(acts_d[:30])
    assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == 2
    a.rollout(acts_d[30:31])                              # T = 1 on its own
    assert _hip.last_rollout_form() == 2
    a.rollout(acts_d[31:])
    assert _hip.last_rollout_form() == 2
    torch.cuda.synchronize()
    sa = _snapshot(a)
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), ref[k].view(np.uint8)), k
    assert int(a.rollout_buffers["fin_count"].min().item()) >= 1


@pytest.mark.gpu
def test_wg4_single_step_launch(tuning):
    """T = 1 from the start state: the seeded hand-off arrays are all the first step sees."""
    torch = _torch()
    from modelcrowdnav_amd import _hip
    E = 9
    acts_d = torch.from_numpy(_actions("holonomic", 1, E, 6))
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    a, b = _rollout_env(E, True), _rollout_env(E, True)
    a.rollout(acts_d.to(a.device))
    assert _hip.last_rollout_form() == 2
    b.step(acts_d[0].to(b.device))
    torch.cuda.synchronize()
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k


@pytest.mark.gpu
def test_rollout_split_forms_give_identical_bytes(tuning):
    """Each forced form is the one launched (mcn_last_rollout_form), and the three leave the same bytes."""
    torch = _torch()
    from modelcrowdnav_amd import _hip
    E, T = 100, 40
    acts = torch.from_numpy(_actions("holonomic", T, E, 7))
    tuning(rollout_fused=1)
    snaps = []
    for split in (0, 1, 2):
        tuning(rollout_split=split)
        env = _rollout_env(E, True)
        env.rollout(acts.to(env.device))
        assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == split
        torch.cuda.synchronize()
        snaps.append(_snapshot(env))
    for k in snaps[0]:
        assert np.array_equal(snaps[0][k].view(np.uint8), snaps[1][k].view(np.uint8)), k
        assert np.array_equal(snaps[0][k].view(np.uint8), snaps[2][k].view(np.uint8)), k


def test_rollout_split_range(tuning):
    """rollout_split takes -1 .. 2; 3 is refused with MCN_EINVAL (no GPU needed: the settings are host state)."""
    from modelcrowdnav_amd import _hip
    for v in (0, 1, 2, -1):
        tuning(rollout_split=v)
        assert _hip.get_tuning().rollout_split == v
    with pytest.raises(_hip.McnError, match="MCN_EINVAL"):
        _hip.set_tuning(rollout_split=3)
    assert _hip.get_tuning().rollout_split == -1


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics,E,form", [
    ("holonomic", 64, 1), ("holonomic", 1016, 1), ("holonomic", 1017, 2), ("holonomic", 4096, 2), ("holonomic", 4097, 1),
    ("holonomic", 4608, 1), ("holonomic", 6137, 2), ("holonomic", 8192, 2), ("holonomic", 8193, 0),
    ("unicycle", 56, 1), ("unicycle", 57, 2), ("unicycle", 4608, 2), ("unicycle", 8192, 2), ("unicycle", 8193, 0)])
def test_automatic_choice_follows_the_sweep(kinematics, E, form, tuning):
    """rollout_split = -1 takes the four-wavefront form where profiles/r12_rollout_wg4.txt measured it to win, and no
    further: a holonomic robot at 128 .. 512 and 768 .. 1024 workgroups of 8 envs, a unicycle robot at 8 .. 1024.  Every
    other size keeps the earlier choice (two wavefronts up to 1536 env groups of 3, one above)."""
    torch = _torch()
    from modelcrowdnav_amd import _hip
    tuning(rollout_fused=1)
    tuning(rollout_split=-1)
    env = _rollout_env(E, True, kinematics)
    env.rollout(torch.from_numpy(_actions(kinematics, 2, E, 8)).to(env.device))
    torch.cuda.synchronize()
    assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == form


def test_wg4_kernels_registers_and_scratch():
    """Both instantiations of env_rollout_wg4_kernel exist in the built library and run without scratch (read from the
    code objects), and each keeps the occupancy the dispatch rule of mcn_env_rollout was measured at.  VGPRs are
    allocated in granules of 8 out of 512 per SIMD.  Holonomic: up to four workgroups resident on a CU, four wavefronts
    on a SIMD, 128 VGPRs each.  Unicycle: measured with three wavefronts on a SIMD (129 VGPRs), which 168 still allow."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from modelcrowdnav_amd import _hip                     # the library is built and loads: so its objects must be there
    assert os.path.exists(_hip.LIB_PATH)
    assert os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"), "the ROCm tools that built the library are gone"
    assert os.path.exists(os.path.join(root, "modelcrowdnav_amd", "csrc", "env_rollout_quad.o")), \
        "libmcn_hip.so is there but the objects it was linked from are not: rebuild (make -C modelcrowdnav_amd/csrc)"
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "kernel_resources.py"), "env_rollout_wg4_kernel<"],
                         capture_output=True, text=True, check=True).stdout
    rows = dict((uni, (int(vgpr), int(scratch))) for uni, vgpr, scratch in
                re.findall(r"env_rollout_wg4_kernel<5, 0, (true|false)>.*vgpr\s+(\d+).*scratch\s+(\d+)", out))
    assert sorted(rows) == ["false", "true"], out
    assert rows["false"][0] <= 128 and rows["false"][1] == 0, out
    assert rows["true"][0] <= 168 and rows["true"][1] == 0, out


# ---------------------------------------------------------------------------------------------------------------------
# against the oracle: 9 envs, so envs 3 and 6 have their quads on two ORCA wavefronts (quads 15-19 and 30-34)
_E, _T, _P = 9, 60, 16
_PACK = 0.12            # odd pool cases start with the crowd pulled into the centre: overlapping discs


def _packed_pool(spec):
    from modelcrowdnav_amd.envs import scenarios as S
    pool = S.scenario_pool(spec, "test", range(_P), N, "circle_crossing").copy()
    pool[1::2, :, S.PX] *= _PACK
    pool[1::2, :, S.PY] *= _PACK
    return pool


def _oracle_actions():
    """The robot walks up the middle (into the packed crowds: collisions; through the open ones: the goal) with a
    little noise."""
    rng = np.random.RandomState(11)
    return np.stack([rng.uniform(-0.15, 0.15, (_T, _E)), rng.uniform(0.8, 1.0, (_T, _E))], -1)


def _oracle_replay(spec, cfg, pool, env_ids, acts):
    """The oracle stepping the given envs with the in-kernel restart replayed on the host (mcn.h mcn_rollout): start case
    e % P, next case (e + 7) % P, stride 3.  Returns the final state, the last step's outputs, restarts per env, counted
    overlaps per env and the number of 3-D LP entries."""
    from modelcrowdnav_amd.envs import scenarios as S
    env_ids = np.asarray(env_ids)
    n = len(env_ids)
    st = cport.EnvState(n, N)

    def load(rows, cases):
        sc = pool[cases]
        st.hpx[rows], st.hpy[rows], st.hgx[rows], st.hgy[rows] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
        st.hvx[rows], st.hvy[rows] = sc[..., S.VX], sc[..., S.VY]
        st.hr[rows], st.hvpref[rows] = sc[..., S.RAD], sc[..., S.VPREF]
        st.human_times[rows] = 0
        rr = spec.robot_row()
        st.rpx[rows], st.rpy[rows], st.rgx[rows], st.rgy[rows] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
        st.rvx[rows], st.rvy[rows], st.rr[rows], st.gtime[rows] = 0.0, 0.0, rr[S.RAD], 0.0
    load(np.arange(n), env_ids % _P)
    next_case = (env_ids + 7) % _P
    restarts, overlaps = np.zeros(n, int), np.zeros(n, int)
    cport.lp3_entries(reset=True)
    for t in range(acts.shape[0]):
        a = acts[t][env_ids]
        ref = cport.env_step(cfg, st, a[:, 0].copy(), a[:, 1].copy(), update=True)
        overlaps += ref["hh_count"]
        d = np.nonzero(ref["done"])[0]
        if len(d):
            load(d, next_case[d])
            next_case[d] = (next_case[d] + 3) % _P
            restarts[d] += 1
    return st, ref, restarts, overlaps, cport.lp3_entries()


def _assert_inputs_reach_the_rare_paths(spec, cfg, pool, acts):
    """From the oracle side, before any comparison: each env that straddles two ORCA wavefronts enters the 3-D LP, has a
    counted human-human overlap and restarts from the pool."""
    for e in (3, 6):
        _, _, restarts, overlaps, lp3 = _oracle_replay(spec, cfg, pool, [e], acts)
        assert lp3 > 0, "env %d never enters the 3-D LP" % e
        assert overlaps[0] > 0, "env %d has no counted overlap" % e
        assert restarts[0] > 0, "env %d never restarts" % e


@pytest.mark.gpu
def test_wg4_launch_matches_oracle_trajectory(tuning):
    """One 60-step launch of 9 envs against the C oracle with the pool restarts replayed on the host: final state, the
    last step's outputs and the number of finished episodes per env, bit for bit; the straddling envs 3 and 6 are shown
    (oracle side) to take the 3-D LP, to have counted overlaps and to restart."""
    torch = _torch()
    from modelcrowdnav_amd import _hip
    env = H.make_vec_env(_E, N)
    spec, cfg = env.spec(), H.oracle_cfg_for(env)
    pool, acts = _packed_pool(spec), _oracle_actions()
    _assert_inputs_reach_the_rare_paths(spec, cfg, pool, acts)
    ids = np.arange(_E)
    env.load_scenarios(pool[ids % _P])
    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % _P, fin_slots=2)
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    env.rollout(torch.from_numpy(acts).to(env.device))
    assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == 2
    torch.cuda.synchronize()
    st, ref, restarts, _, _ = _oracle_replay(spec, cfg, pool, ids, acts)
    H.assert_state_equal(H.download(env), st, what="after a %d-step launch" % _T)
    for k in ("reward", "done", "info", "dmin"):
        H.assert_bits_equal(getattr(env, k).cpu().numpy(), ref[k], k)
    assert np.array_equal(env.hh_count.cpu().numpy(), ref["hh_count"])
    H.assert_bits_equal(env.human_act.cpu().numpy(), ref["human_act"], "human_act")
    assert np.array_equal(env.rollout_buffers["fin_count"].cpu().numpy(), restarts)
