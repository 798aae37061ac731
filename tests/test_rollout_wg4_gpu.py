"""The four-wavefront form of the fused rollout launch (mcn_tuning.rollout_split = 2: workgroups of 8 envs, three ORCA
wavefronts for their 40 quads and one float64 wavefront with a lane per (env, human); built for 5 humans and an
invisible robot, both robot kinematics) against T mcn_env_step calls, against the C oracle's trajectory and against the
other two forms, bit for bit.  The forms share one mcn_last_dispatch family and give the same bytes, so every test that
forces the form also asserts mcn_last_rollout_form() == 2: the four-wavefront kernel is what was launched."""
import os
import shutil

import numpy as np
import pytest

from tests import helpers as H
from tests.rollout_harness import (assert_same_bytes, kernel_resources, launch, need_gpu, oracle_rollout, packed_pool,
                                   pool_env, random_actions, snapshot)

N = 5                                   # the only crowd size the form is instantiated for (robot invisible)

_single_steps = {}


def _single_step_reference(E, with_pool, kinematics, T):
    """T mcn_env_step calls on the shared action sequence, computed once per configuration and left unchanged."""
    torch = need_gpu()
    key = (E, with_pool, kinematics)
    if key not in _single_steps:
        b = pool_env(E, N, with_pool=with_pool, kinematics=kinematics)
        acts_d = torch.from_numpy(random_actions(kinematics, T, E, 5)).to(b.device)
        for t in range(T):
            b.step(acts_d[t])
        torch.cuda.synchronize()
        _single_steps[key] = snapshot(b)
    return _single_steps[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("with_pool", [True, False])
@pytest.mark.parametrize("E", [1, 7, 8, 9, 1000])
def test_wg4_launch_equals_single_steps(E, with_pool, kinematics, tuning):
    """Less than one workgroup, exactly one, one plus a ragged tail, many ragged: every byte of state, step record,
    Explorer record and finished-episode records after launches of 30 + 1 + 79 steps equals 110 single steps; every
    env passes the time limit, so each finishes (and, with the pool, restarts) inside the sequence."""
    torch = need_gpu()
    T = 110
    ref = _single_step_reference(E, with_pool, kinematics, T)
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    a = pool_env(E, N, with_pool=with_pool, kinematics=kinematics)
    acts_d = torch.from_numpy(random_actions(kinematics, T, E, 5)).to(a.device)
    launch(a, acts_d[:30], 2)
    launch(a, acts_d[30:31], 2)                           # T = 1 on its own
    launch(a, acts_d[31:], 2)
    torch.cuda.synchronize()
    assert_same_bytes(snapshot(a), ref)
    assert int(a.rollout_buffers["fin_count"].min().item()) >= 1


@pytest.mark.gpu
def test_wg4_single_step_launch(tuning):
    """T = 1 from the start state: the seeded hand-off arrays are all the first step sees."""
    torch = need_gpu()
    E = 9
    acts_d = torch.from_numpy(random_actions("holonomic", 1, E, 6))
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    a, b = pool_env(E, N), pool_env(E, N)
    launch(a, acts_d.to(a.device), 2)
    b.step(acts_d[0].to(b.device))
    torch.cuda.synchronize()
    assert_same_bytes(snapshot(a), snapshot(b))


@pytest.mark.gpu
def test_rollout_split_forms_give_identical_bytes(tuning):
    """Each forced form is the one launched (mcn_last_rollout_form), and the three leave the same bytes."""
    torch = need_gpu()
    E, T = 100, 40
    acts = torch.from_numpy(random_actions("holonomic", T, E, 7))
    tuning(rollout_fused=1)
    snaps = []
    for split in (0, 1, 2):
        tuning(rollout_split=split)
        env = pool_env(E, N)
        launch(env, acts.to(env.device), split)
        torch.cuda.synchronize()
        snaps.append(snapshot(env))
    assert_same_bytes(snaps[0], snaps[1], "forms 0 and 1")
    assert_same_bytes(snaps[0], snaps[2], "forms 0 and 2")


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
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    tuning(rollout_fused=1)
    tuning(rollout_split=-1)
    env = pool_env(E, N, kinematics=kinematics)
    env.rollout(torch.from_numpy(random_actions(kinematics, 2, E, 8)).to(env.device))
    torch.cuda.synchronize()
    assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == form


def test_wg4_kernels_registers_and_scratch():
    """Both instantiations of env_rollout_wg4_kernel exist in the built library and run without scratch (read from the
    code objects), and each keeps the occupancy the dispatch rule of mcn_env_rollout was measured at.  VGPRs are
    allocated in granules of 8 out of 512 per SIMD.  Holonomic: up to four workgroups resident on a CU, four wavefronts
    on a SIMD, 128 VGPRs each.  Unicycle: measured with three wavefronts on a SIMD (129 VGPRs), which 168 still allow."""
    assert os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"), "the ROCm tools that built the library are gone"
    out = kernel_resources("env_rollout_wg4_kernel<")
    rows = {uni: (r[0], r[3]) for uni in ("true", "false") for name, r in out.items()
            if "env_rollout_wg4_kernel<5, 0, %s>" % uni in name}
    assert sorted(rows) == ["false", "true"], out
    assert rows["false"][0] <= 128 and rows["false"][1] == 0, out
    assert rows["true"][0] <= 168 and rows["true"][1] == 0, out


# ---------------------------------------------------------------------------------------------------------------------
# against the oracle: 9 envs, so envs 3 and 6 have their quads on two ORCA wavefronts (quads 15-19 and 30-34)
_E, _T, _P = 9, 60, 16


def _oracle_actions():
    """The robot walks up the middle (into the packed crowds: collisions; through the open ones: the goal) with a
    little noise."""
    rng = np.random.RandomState(11)
    return np.stack([rng.uniform(-0.15, 0.15, (_T, _E)), rng.uniform(0.8, 1.0, (_T, _E))], -1)


def _assert_inputs_reach_the_rare_paths(spec, cfg, pool, acts):
    """From the oracle side, before any comparison: each env that straddles two ORCA wavefronts enters the 3-D LP, has a
    counted human-human overlap and restarts from the pool."""
    for e in (3, 6):
        _, _, restarts, overlaps, lp3 = oracle_rollout(spec, cfg, pool, [e], acts, 7, 3)
        assert lp3 > 0, "env %d never enters the 3-D LP" % e
        assert overlaps[0] > 0, "env %d has no counted overlap" % e
        assert restarts[0] > 0, "env %d never restarts" % e


@pytest.mark.gpu
def test_wg4_launch_matches_oracle_trajectory(tuning):
    """One 60-step launch of 9 envs against the C oracle with the pool restarts replayed on the host: final state, the
    last step's outputs and the number of finished episodes per env, bit for bit; the straddling envs 3 and 6 are shown
    (oracle side) to take the 3-D LP, to have counted overlaps and to restart."""
    torch = need_gpu()
    env = H.make_vec_env(_E, N)
    spec, cfg = env.spec(), H.oracle_cfg_for(env)
    pool, acts = packed_pool(spec, _P, N), _oracle_actions()
    _assert_inputs_reach_the_rare_paths(spec, cfg, pool, acts)
    ids = np.arange(_E)
    env.load_scenarios(pool[ids % _P])
    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % _P, fin_slots=2)
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    launch(env, torch.from_numpy(acts).to(env.device), 2)
    torch.cuda.synchronize()
    st, ref, restarts, _, _ = oracle_rollout(spec, cfg, pool, ids, acts, 7, 3)
    H.assert_state_equal(H.download(env), st, what="after a %d-step launch" % _T)
    for k in ("reward", "done", "info", "dmin"):
        H.assert_bits_equal(getattr(env, k).cpu().numpy(), ref[k], k)
    assert np.array_equal(env.hh_count.cpu().numpy(), ref["hh_count"])
    H.assert_bits_equal(env.human_act.cpu().numpy(), ref["human_act"], "human_act")
    assert np.array_equal(env.rollout_buffers["fin_count"].cpu().numpy(), restarts)
