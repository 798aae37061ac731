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
import subprocess
import sys

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H

N = 5
_FIELDS = ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal", "rtheta", "gtime", "human_times",
           "step_rec", "human_act")
_ROLL = ("state", "fin_return", "fin_time", "fin_info")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _snapshot(env):
    c = lambda t: t.detach().cpu().numpy().copy()
    snap = {k: c(getattr(env, k)) for k in _FIELDS}
    snap.update({"roll_" + k: c(v) for k, v in env.rollout_buffers.items() if k in _ROLL})
    return snap


def _assert_same_bytes(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _launch(env, acts_d, split, cuts):
    """The action sequence in launches acts_d[cuts[i]:cuts[i + 1]] of the forced form."""
    from modelcrowdnav_amd import _hip
    _hip.set_tuning(rollout_fused=1, rollout_split=split)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        env.rollout(acts_d[lo:hi])
        assert _hip.last_dispatch() == "env_rollout_quad_kernel" and _hip.last_rollout_form() == split


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-human attributes: 9 envs, so envs 3 and 6 have their quads on two ORCA wavefronts
_E, _T, _P = 9, 60, 16
_PACK = 0.12            # odd pool cases start with the crowd pulled into the centre: overlapping discs, the 3-D LP


def _attr_env():
    return H.make_vec_env(_E, N, **{"env.randomize_attributes": "true"})


def _attr_pool(spec):
    from modelcrowdnav_amd.envs import scenarios as S
    assert spec.randomize_attributes
    pool = S.scenario_pool(spec, "test", range(_P), N, "circle_crossing").copy()
    pool[1::2, :, S.PX] *= _PACK
    pool[1::2, :, S.PY] *= _PACK
    return pool


def _attr_actions():
    """The robot walks up the middle (into the packed crowds: collisions; through the open ones: the goal)."""
    rng = np.random.RandomState(11)
    return np.stack([rng.uniform(-0.15, 0.15, (_T, _E)), rng.uniform(0.8, 1.0, (_T, _E))], -1)


def _assert_run_is_discriminating(env, cfg, pool, acts):
    """From the oracle side, before any comparison: the five radii (and v_pref) of every case differ, some solve has a
    neighbour in range, some solve enters the 3-D LP and some env restarts from the pool -- the straddling envs 3 and 6
    among them.  The replay is that of tests/test_rollout_wg4_gpu.py: start case e % P, next (e + 7) % P, stride 3."""
    from modelcrowdnav_amd.envs import scenarios as S
    spec = env.spec()
    for col in (S.RAD, S.VPREF):
        assert all(len(set(case[:, col])) == N for case in pool), "two humans of a case share an attribute"
    assert pool[:, :, S.RAD].min() >= 0.3 and pool[:, :, S.RAD].max() < 0.5
    # in range: float32 squared distance below neighbor_dist^2, as the solve tests it, already in the start state
    p32 = pool[np.arange(_E) % _P][:, :, [S.PX, S.PY]].astype(np.float32)
    d2 = ((p32[:, :, None] - p32[:, None, :]) ** 2).sum(-1)[:, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]]
    assert (d2 < np.float32(env._orca.neighbor_dist) ** 2).any(), "no neighbour in range"
    st = cport.EnvState(_E, N)
    ids = np.arange(_E)

    def load(rows, cases):
        sc = pool[cases]
        st.hpx[rows], st.hpy[rows], st.hgx[rows], st.hgy[rows] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
        st.hvx[rows], st.hvy[rows] = sc[..., S.VX], sc[..., S.VY]
        st.hr[rows], st.hvpref[rows] = sc[..., S.RAD], sc[..., S.VPREF]
        st.human_times[rows] = 0
        rr = spec.robot_row()
        st.rpx[rows], st.rpy[rows], st.rgx[rows], st.rgy[rows] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
        st.rvx[rows], st.rvy[rows], st.rr[rows], st.gtime[rows] = 0.0, 0.0, rr[S.RAD], 0.0
    load(ids, ids % _P)
    next_case, restarts = (ids + 7) % _P, np.zeros(_E, int)
    cport.lp3_entries(reset=True)
    for t in range(_T):
        ref = cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        d = np.nonzero(ref["done"])[0]
        if len(d):
            load(d, next_case[d])
            next_case[d] = (next_case[d] + 3) % _P
            restarts[d] += 1
    assert cport.lp3_entries() > 0, "no solve enters the 3-D LP"
    assert restarts[3] > 0 and restarts[6] > 0, "the straddling envs never restart: %s" % restarts
    return st, ref, restarts


def _attr_run(pool, acts, how):
    torch = _torch()
    env = _attr_env()
    ids = np.arange(_E)
    env.load_scenarios(pool[ids % _P])
    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=(ids + 7) % _P, fin_slots=2)
    acts_d = torch.from_numpy(acts).to(env.device)
    if how == "steps":
        for t in range(_T):
            env.step(acts_d[t])
    else:
        _launch(env, acts_d, how, (0, _T))
    torch.cuda.synchronize()
    return env, _snapshot(env)


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
    _assert_same_bytes(four, _attr_run(pool, acts, 1)[1], "two-wavefront form")
    _assert_same_bytes(four, _attr_run(pool, acts, "steps")[1], "single steps")
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
    torch = _torch()
    from modelcrowdnav_amd.envs import scenarios as S
    env = H.make_vec_env(E, N, **{"env.time_limit": _LIMIT, "env.randomize_attributes": "true"})
    pool = S.scenario_pool(env.spec(), "test", range(2), N, "circle_crossing").copy()
    pool[:, :, S.VX] = 0.25 * pool[:, :, S.GX] / 4.0
    pool[:, :, S.VY] = 0.25 * pool[:, :, S.GY] / 4.0
    ids = np.arange(E)
    env.load_scenarios(pool[ids % 2])
    if with_hvel:
        dpool = pool
    else:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
        dpool = dict(hpos=up(pool[:, :, [S.PX, S.PY]]), hgoal=up(pool[:, :, [S.GX, S.GY]]),
                     hrad=up(pool[:, :, S.RAD]), hvpref=up(pool[:, :, S.VPREF]))
    env.attach_rollout(gamma=0.9, pool=dpool, case_stride=1, first_cases=(ids + 1) % 2, fin_slots=3)
    return env, pool


@pytest.mark.gpu
@pytest.mark.parametrize("with_hvel", [True, False])
@pytest.mark.parametrize("E", [8, 9])
def test_restart_at_the_edges_of_a_launch(E, with_hvel, tuning):
    """12 steps as 5 + 7 (the first launch ends on the finishing step: its epilogue stores the new case's goal, radius
    and v_pref), as 4 + 8 (the second launch begins with it), as one launch and as 12 single steps: the same bytes."""
    torch = _torch()
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
    ref = _snapshot(ref_env)
    assert int(ref_env.rollout_buffers["fin_count"].min().item()) == 2

    a, _ = _edge_env(E, with_hvel)
    _launch(a, acts_d, 2, (0, _FINISH))
    torch.cuda.synchronize()
    assert bool(a.done.all().item())
    from modelcrowdnav_amd.envs import scenarios as S
    want = pool[(np.arange(E) + 1) % 2]                         # the epilogue stored the restarted case
    assert np.array_equal(a.hrad.cpu().numpy(), want[:, :, S.RAD])
    assert np.array_equal(a.hvpref.cpu().numpy(), want[:, :, S.VPREF])
    assert np.array_equal(a.hgoal.cpu().numpy(), want[:, :, [S.GX, S.GY]])
    assert np.array_equal(a.hpos.cpu().numpy(), want[:, :, [S.PX, S.PY]])
    assert np.array_equal(a.hvel.cpu().numpy(), want[:, :, [S.VX, S.VY]] if with_hvel else np.zeros((E, N, 2)))
    _launch(a, acts_d, 2, (_FINISH, T))
    torch.cuda.synchronize()
    _assert_same_bytes(_snapshot(a), ref, "5 + 7")
    for cuts in ((0, _FINISH - 1, T), (0, T)):
        b, _ = _edge_env(E, with_hvel)
        _launch(b, acts_d, 2, cuts)
        torch.cuda.synchronize()
        _assert_same_bytes(_snapshot(b), ref, str(cuts))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the benchmark's variant: human_times allocated but untracked, no human_act export
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
def test_optional_outputs_absent(kinematics, tuning):
    """track_human_times off and export_human_actions off, 9 envs, 40 steps in launches of 13 + 27 against single steps:
    the same bytes, human_times and human_act (which nobody may write: it keeps its fill) included."""
    torch = _torch()
    from modelcrowdnav_amd.envs import scenarios as S
    tuning(rollout_fused=1)
    E, T = 9, 40
    rng = np.random.RandomState(5)
    if kinematics == "unicycle":
        acts = np.stack([rng.uniform(0, 1, (T, E)), rng.uniform(-np.pi / 4, np.pi / 4, (T, E))], -1)
    else:
        acts = np.stack([rng.uniform(-0.15, 0.15, (T, E)), rng.uniform(0.8, 1.0, (T, E))], -1)
    snaps = []
    for how in ("steps", "launch"):
        env = H.make_vec_env(E, N, kinematics=kinematics)
        env.track_human_times = False; env.export_human_actions = False
        pool = S.scenario_pool(env.spec(), "test", range(_P), N, "circle_crossing").copy()
        pool[1::2, :, S.PX] *= _PACK
        pool[1::2, :, S.PY] *= _PACK
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
            _launch(env, acts_d, 2, (0, 13, T))
        torch.cuda.synchronize()
        snaps.append(_snapshot(env))
        assert (snaps[-1]["human_act"] == -7.0).all() and (snaps[-1]["human_times"] == 0.0).all()
        if kinematics == "holonomic":
            assert int(env.rollout_buffers["fin_count"].max().item()) >= 1        # some env restarts inside the run
    _assert_same_bytes(snaps[1], snaps[0])


# ---------------------------------------------------------------------------------------------------------------------
# 4. the header split changed no other kernel
def test_header_split_keeps_every_other_quad_kernel():
    """Every env_rollout_quad_kernel<...> instantiation has the registers profiles/r13_kernel_resources.txt lists for it
    and runs without scratch, and no env_step_quad_kernel<...> instantiation uses scratch or differs from the recorded
    table of profiles/r14_kernel_resources.txt (the r13 file lists the rollout kernels only)."""
    from modelcrowdnav_amd import _hip
    assert os.path.exists(_hip.LIB_PATH)
    assert os.path.exists(os.path.join(_ROOT, "modelcrowdnav_amd", "csrc", "env_rollout_quad.o")), \
        "libmcn_hip.so is there but the objects it was linked from are not: rebuild (make -C modelcrowdnav_amd/csrc)"
    row = re.compile(r"^void mcn::(env_(?:rollout|step)_quad_kernel<[^>]*>)\(.*?vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) "
                     r"scratch\s+(\d+) lds\s+(\d+) vspill (\d+)", re.M)

    def table(text):
        return {m.group(1): tuple(int(x) for x in m.groups()[1:]) for m in row.finditer(text)}
    built = {}
    for name in ("env_rollout_quad_kernel<", "env_step_quad_kernel<"):
        built.update(table(subprocess.run([sys.executable, os.path.join(_ROOT, "tools", "kernel_resources.py"), name],
                                          capture_output=True, text=True, check=True).stdout))
    r13 = table(open(os.path.join(_ROOT, "profiles", "r13_kernel_resources.txt")).read())
    r14 = table(open(os.path.join(_ROOT, "profiles", "r14_kernel_resources.txt")).read())
    rollout = [k for k in built if k.startswith("env_rollout_quad_kernel<")]
    steps = [k for k in built if k.startswith("env_step_quad_kernel<")]
    assert len(rollout) == 36 and sorted(rollout) == sorted(r13), sorted(rollout)
    assert len(steps) > 0 and sorted(steps) == sorted(k for k in r14 if k.startswith("env_step_quad_kernel<"))
    for k in rollout:
        assert built[k] == r13[k] and built[k][3] == 0 and built[k][5] == 0, (k, built[k], r13[k])
    for k in steps:
        assert built[k] == r14[k] and built[k][3] == 0 and built[k][5] == 0, (k, built[k], r14[k])
