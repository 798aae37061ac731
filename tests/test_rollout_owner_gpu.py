"""Who owns the humans in the four-wavefront rollout form (env_rollout_wg4_kernel, mcn_tuning.rollout_split = 2).

The float64 wavefront holds every human's float64 state (position, velocity, goal, radius, v_pref, human_times), one
human per lane, integrates or restarts it, and hands the ORCA wavefronts float32 operand packs through LDS; the ORCA
wavefronts hand back the new velocity.  What the other rollout tests cannot see, because every fixture of theirs has
radius 0.3 and v_pref 1.0 for everybody and the optional outputs switched on:

  * a candidate's radius or maximum speed read from the wrong human: per-human attributes;
  * the goal, radius and v_pref of a restarted case at the edges of a launch (the finishing step last, or first);
  * the benchmark's own variant: human_times allocated but not tracked, no human_act export.

Every launch that forces the form also asserts mcn_last_rollout_form() == 2.  The last test needs no GPU: the header
split that made this possible (quad_common.hpp: quad_orca_operands + quad_orca_core) left every other quad kernel its
registers."""
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests.rollout_harness import (ROOT, as_device_pool, assert_same_bytes, kernel_resources, launch_cuts, need_gpu,
                                   oracle_rollout, packed_pool, parse_resources, random_actions, snapshot)

N = 5


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-human attributes: 9 envs, so envs 3 and 6 have their quads on two ORCA wavefronts
_E, _T, _P = 9, 60, 16


def _attr_env():
    return H.make_vec_env(_E, N, **{"env.randomize_attributes": "true"})


def _attr_pool(spec):
    assert spec.randomize_attributes
    return packed_pool(spec, _P, N)


def _attr_actions():
    """The robot walks up the middle (into the packed crowds: collisions; through the open ones: the goal)."""
    rng = np.random.RandomState(11)
    return np.stack([rng.uniform(-0.15, 0.15, (_T, _E)), rng.uniform(0.8, 1.0, (_T, _E))], -1)


def _assert_run_is_discriminating(env, cfg, pool, acts):
    """From the oracle side, before any comparison: the five radii (and v_pref) of every case differ, some solve has a
    neighbour in range, some solve enters the 3-D LP and some env restarts from the pool -- the straddling envs 3 and 6
    among them.  The replay is oracle_rollout: start case e % P, next (e + 7) % P, stride 3."""
    from modelcrowdnav_amd.envs import scenarios as S
    spec = env.spec()
    for col in (S.RAD, S.VPREF):
        assert all(len(set(case[:, col])) == N for case in pool), "two humans of a case share an attribute"
    assert pool[:, :, S.RAD].min() >= 0.3 and pool[:, :, S.RAD].max() < 0.5
    # in range: float32 squared distance below neighbor_dist^2, as the solve tests it, already in the start state
    p32 = pool[np.arange(_E) % _P][:, :, [S.PX, S.PY]].astype(np.float32)
    d2 = ((p32[:, :, None] - p32[:, None, :]) ** 2).sum(-1)[:, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]]
    assert (d2 < np.float32(env._orca.neighbor_dist) ** 2).any(), "no neighbour in range"
    st, ref, restarts, _, lp3 = oracle_rollout(spec, cfg, pool, np.arange(_E), acts, 7, 3)
    assert lp3 > 0, "no solve enters the 3-D LP"
    assert restarts[3] > 0 and restarts[6] > 0, "the straddling envs never restart: %s" % restarts
    return st, ref, restarts


def _attr_run(pool, acts, how):
    torch = need_gpu()
    env = _attr_env()
    ids = np.arange(_E)
    env.load_scenarios(pool[ids % _P])
    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % _P, fin_slots=2)
    acts_d = torch.from_numpy(acts).to(env.device)
    if how == "steps":
        for t in range(_T):
            env.step(acts_d[t])
    else:
        launch_cuts(env, acts_d, how, (0, _T))
    torch.cuda.synchronize()
    return env, snapshot(env)


@pytest.mark.gpu
def test_per_human_attributes_three_ways(tuning):
    """Radii 0.3 - 0.5 and v_pref 0.5 - 1.5 drawn per human: one 60-step launch of the four-wavefront form, one of the
    two-wavefront form and 60 single steps leave the same bytes in every state array, step record, Explorer record and
    finished-episode slot -- and the oracle's state; with equal attributes an owner's radius in the place of a
    candidate's would change nothing."""
    tuning(rollout_fused=1)
    env = _attr_env()
    cfg = H.oracle_cfg_for(env)
    pool, acts = _attr_pool(env.spec()), _attr_actions()
    st, ref, restarts = _assert_run_is_discriminating(env, cfg, pool, acts)
    env4, four = _attr_run(pool, acts, 2)
    assert_same_bytes(four, _attr_run(pool, acts, 1)[1], "two-wavefront form")
    assert_same_bytes(four, _attr_run(pool, acts, "steps")[1], "single steps")
    H.assert_state_equal(H.download(env4), st, what="oracle, after a %d-step launch" % _T)
    H.assert_bits_equal(env4.human_act.cpu().numpy(), ref["human_act"], "human_act")
    assert np.array_equal(env4.rollout_buffers["fin_count"].cpu().numpy(), restarts)


# ---------------------------------------------------------------------------------------------------------------------
# 2. restart edges: with time_limit 2 and a robot that stands still every env times out at its fifth step
# (gtime 1.0 >= time_limit - 1), and again five steps later: steps 5 and 10 of 12
_LIMIT, _FINISH = 2, 5


def _edge_env(E, with_hvel, device_pool=None):
    """Pool of two cases with distinct attributes; the host pool carries start velocities (pool_hvel), the same pool
    handed over as device tensors does not (restarts at rest)."""
    from modelcrowdnav_amd.envs import scenarios as S
    env = H.make_vec_env(E, N, **{"env.time_limit": _LIMIT, "env.randomize_attributes": "true"})
    pool = S.scenario_pool(env.spec(), "test", range(2), N, "circle_crossing").copy()
    pool[:, :, S.VX] = 0.25 * pool[:, :, S.GX] / 4.0
    pool[:, :, S.VY] = 0.25 * pool[:, :, S.GY] / 4.0
    ids = np.arange(E)
    env.load_scenarios(pool[ids % 2])
    env.attach_rollout(gamma=0.9, pool=pool if with_hvel else as_device_pool(env, pool), case_stride=1,
                       first_cases=(ids + 1) % 2, fin_slots=3)
    return env, pool


@pytest.mark.gpu
@pytest.mark.parametrize("with_hvel", [True, False])
@pytest.mark.parametrize("E", [8, 9])
def test_restart_at_the_edges_of_a_launch(E, with_hvel, tuning):
    """12 steps as 5 + 7 (the first launch ends on the finishing step: its epilogue stores the new case's goal, radius
    and v_pref), as 4 + 8 (the second launch begins with it), as one launch and as 12 single steps: the same bytes."""
    torch = need_gpu()
    tuning(rollout_fused=1)
    T = 12
    acts = np.zeros((T, E, 2))
    ref_env, pool = _edge_env(E, with_hvel)
    acts_d = torch.from_numpy(acts).to(ref_env.device)
    for t in range(T):
        ref_env.step(acts_d[t])
        if t + 1 == _FINISH:                                   # the inputs are what they are meant to be
            assert bool(ref_env.done.all().item()), "not every env finishes at step %d" % _FINISH
    torch.cuda.synchronize()
    ref = snapshot(ref_env)
    assert int(ref_env.rollout_buffers["fin_count"].min().item()) == 2

    a, _ = _edge_env(E, with_hvel)
    launch_cuts(a, acts_d, 2, (0, _FINISH))
    torch.cuda.synchronize()
    assert bool(a.done.all().item())
    from modelcrowdnav_amd.envs import scenarios as S
    want = pool[(np.arange(E) + 1) % 2]                         # the epilogue stored the restarted case
    assert np.array_equal(a.hrad.cpu().numpy(), want[:, :, S.RAD])
    assert np.array_equal(a.hvpref.cpu().numpy(), want[:, :, S.VPREF])
    assert np.array_equal(a.hgoal.cpu().numpy(), want[:, :, [S.GX, S.GY]])
    assert np.array_equal(a.hpos.cpu().numpy(), want[:, :, [S.PX, S.PY]])
    assert np.array_equal(a.hvel.cpu().numpy(), want[:, :, [S.VX, S.VY]] if with_hvel else np.zeros((E, N, 2)))
    launch_cuts(a, acts_d, 2, (_FINISH, T))
    torch.cuda.synchronize()
    assert_same_bytes(snapshot(a), ref, "5 + 7")
    for cuts in ((0, _FINISH - 1, T), (0, T)):
        b, _ = _edge_env(E, with_hvel)
        launch_cuts(b, acts_d, 2, cuts)
        torch.cuda.synchronize()
        assert_same_bytes(snapshot(b), ref, str(cuts))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the benchmark's variant: human_times allocated but untracked, no human_act export
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
def test_optional_outputs_absent(kinematics, tuning):
    """track_human_times off and export_human_actions off, 9 envs, 40 steps in launches of 13 + 27 against single steps:
    the same bytes, human_times and human_act (which nobody may write: it keeps its fill) included."""
    torch = need_gpu()
    tuning(rollout_fused=1)
    E, T = 9, 40
    if kinematics == "unicycle":
        acts = random_actions(kinematics, T, E, 5)
    else:
        rng = np.random.RandomState(5)
        acts = np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
    snaps = []
    for how in ("steps", "launch"):
        env = H.make_vec_env(E, N, kinematics=kinematics)
        env.track_human_times = False; env.export_human_actions = False
        pool = packed_pool(env.spec(), _P, N)
        ids = np.arange(E)
        env.load_scenarios(pool[ids % _P])
        env.human_times.fill_(0.0)
        env.human_act.fill_(-7.0)
        env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % _P, fin_slots=2)
        acts_d = torch.from_numpy(acts).to(env.device)
        if how == "steps":
            for t in range(T):
                env.step(acts_d[t])
        else:
            launch_cuts(env, acts_d, 2, (0, 13, T))
        torch.cuda.synchronize()
        snaps.append(snapshot(env))
        assert (snaps[-1]["human_act"] == -7.0).all() and (snaps[-1]["human_times"] == 0.0).all()
        if kinematics == "holonomic":
            assert int(env.rollout_buffers["fin_count"].max().item()) >= 1        # some env restarts inside the run
    assert_same_bytes(snaps[1], snaps[0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the header split changed no other kernel
def test_header_split_keeps_every_other_quad_kernel():
    """Every env_rollout_quad_kernel<...> instantiation has the registers profiles/r13_kernel_resources.txt lists for it
    and runs without scratch, and no env_step_quad_kernel<...> instantiation uses scratch or differs from the recorded
    table of profiles/r14_kernel_resources.txt (the r13 file lists the rollout kernels only)."""
    quad = lambda rows: {k: v for k, v in rows.items() if re.match(r"void mcn::env_(rollout|step)_quad_kernel<", k)}
    built = quad(dict(kernel_resources("env_rollout_quad_kernel<"), **kernel_resources("env_step_quad_kernel<")))
    r13, r14 = (quad(parse_resources(open(os.path.join(ROOT, "profiles", "r%d_kernel_resources.txt" % r)).read()))
                for r in (13, 14))
    rollout = [k for k in built if k.startswith("void mcn::env_rollout_quad_kernel<")]
    steps = [k for k in built if k.startswith("void mcn::env_step_quad_kernel<")]
    assert len(rollout) == 36 and sorted(rollout) == sorted(r13), sorted(rollout)
    assert len(steps) > 0 and sorted(steps) == sorted(k for k in r14 if k.startswith("void mcn::env_step_quad_kernel<"))
    for k in rollout:
        assert built[k] == r13[k] and built[k][3] == 0 and built[k][5] == 0, (k, built[k], r13[k])
    for k in steps:
        assert built[k] == r14[k] and built[k][3] == 0 and built[k][5] == 0, (k, built[k], r14[k])
