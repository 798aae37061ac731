"""Shared plumbing of the fused-rollout tests: the env on a scenario pool, the byte-for-byte comparison of whole envs,
forced launches, the single-step reference, the oracle replay with pool restarts, the built kernels' resource table.

Each helper exists once, here; the test files keep their inputs, cut lists, bounds and messages.  torch and the package
are imported inside the functions, as the tests do, so that collecting on a machine without a GPU stays cheap."""
import functools
import os
import re
import subprocess
import sys

import numpy as np

from oracle import cport
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNAP_FIELDS = ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal", "rtheta", "gtime", "human_times",
               "step_rec", "human_act")
ROLL_FIELDS = ("state", "fin_return", "fin_time", "fin_info")


def need_gpu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---------------------------------------------------------------------------------------------------------------------
# comparing whole envs
def snapshot(env):
    """Host copies of the env's state, step record and exported actions and, with a rollout attached, of the Explorer
    record and the finished-episode arrays (keys roll_*)."""
    c = lambda t: t.detach().cpu().numpy().copy()
    snap = {k: c(getattr(env, k)) for k in SNAP_FIELDS}
    if env._roll is not None:
        snap.update({"roll_" + k: c(v) for k, v in env.rollout_buffers.items() if k in ROLL_FIELDS})
    return snap


def assert_same_bytes(a, b, what=""):
    """Two snapshots hold the same arrays and every array the same bytes: -0.0 is not +0.0, a NaN only its own payload."""
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b)))
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def random_actions(kinematics, T, E, seed):
    """[T, E, 2] robot actions: (v, r) for a unicycle robot, a velocity inside the unit disc for a holonomic one."""
    rng = np.random.RandomState(seed)
    if kinematics == "unicycle":
        return np.stack([rng.uniform(0, 1, (T, E)), rng.uniform(-np.pi / 4, np.pi / 4, (T, E))], -1)
    sp, aa = rng.uniform(0, 1, (T, E)), rng.uniform(0, 2 * np.pi, (T, E))
    return np.stack([sp * np.cos(aa), sp * np.sin(aa)], -1)


def pool_env(E, N=5, visible=False, with_pool=True, kinematics="holonomic", fin_slots=2):
    """E envs on the 64 circle-crossing test cases: env e starts from case e % 64 and, with the pool, restarts from
    (e + 7) % 64 and every third case after it."""
    from modelcrowdnav_amd.envs import scenarios as S
    env = H.make_vec_env(E, N, robot_visible=visible, kinematics=kinematics)
    pool = S.scenario_pool(env.spec(), "test", range(64), N, "circle_crossing")
    ids = np.arange(E) % 64
    env.load_scenarios(pool[ids])
    env.attach_rollout(gamma=0.9, pool=pool if with_pool else None, case_stride=3, first_cases=(ids + 7) % 64,
                       fin_slots=fin_slots)
    return env


def packed_pool(spec, P, N, pack=0.12):
    """P circle-crossing cases; the odd ones start with the crowd pulled into the centre: overlapping discs, the 3-D LP."""
    from modelcrowdnav_amd.envs import scenarios as S
    pool = S.scenario_pool(spec, "test", range(P), N, "circle_crossing").copy()
    pool[1::2, :, S.PX] *= pack
    pool[1::2, :, S.PY] *= pack
    return pool


def as_device_pool(env, pool):
    """A host pool as the dict of device tensors attach_rollout uses in place: no start velocities (restarts at rest)."""
    import torch
    from modelcrowdnav_amd.envs import scenarios as S
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)
    return dict(hpos=up(pool[:, :, [S.PX, S.PY]]), hgoal=up(pool[:, :, [S.GX, S.GY]]), hrad=up(pool[:, :, S.RAD]),
                hvpref=up(pool[:, :, S.VPREF]))


def goal_seeking(env, t):
    """Deterministic, state-only robot policy whose arithmetic is exact on any IEEE machine: move at +-0.6 along
    each axis according to the sign of the remaining goal offset (0 inside a 0.2 band)."""
    import torch
    d = env.rgoal - env.rpos
    v, z = torch.full_like(d, 0.6), torch.zeros_like(d)          # float64 constants (python scalars would be f32)
    return (torch.where(d > 0.2, v, z) - torch.where(d < -0.2, v, z)).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# launches
def launch(env, acts, form):
    """env.rollout(acts); a quad path must have gone out as the form it forces (None: any other path): the three forms
    share one dispatch family and leave the same bytes, so nothing else would show that another kernel stood in."""
    from modelcrowdnav_amd import _hip
    env.rollout(acts)
    if form is not None:
        assert _hip.last_dispatch() == "env_rollout_quad_kernel", _hip.last_dispatch()
        assert _hip.last_rollout_form() == form, (_hip.last_rollout_form(), form)


def launch_cuts(env, acts_d, split, cuts):
    """The action sequence in launches acts_d[cuts[i]:cuts[i + 1]] of the forced form."""
    from modelcrowdnav_amd import _hip
    _hip.set_tuning(rollout_fused=1, rollout_split=split)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        launch(env, acts_d[lo:hi], split)


def single_steps(build, acts):
    """T mcn_env_step calls on build()'s env.  Returns the env, the snapshot after every step (snaps[t] = after step
    t), the snapshot before the first and the done flags [T, E]."""
    torch = need_gpu()
    env = build()
    acts_d = torch.from_numpy(acts).to(env.device)
    first, snaps, done = snapshot(env), [], []
    for t in range(len(acts)):
        env.step(acts_d[t])
        snaps.append(snapshot(env))
        done.append(env.done.cpu().numpy().astype(bool).copy())
    return env, snaps, first, np.array(done)


def launches_against(build, acts, split, cuts, snaps, what=""):
    """The sequence in launches acts[cuts[i]:cuts[i + 1]] of the forced form; after EVERY launch the bytes of the
    single-step run at that step."""
    torch = need_gpu()
    env = build()
    acts_d = torch.from_numpy(acts).to(env.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        launch_cuts(env, acts_d, split, (lo, hi))
        torch.cuda.synchronize()
        assert_same_bytes(snapshot(env), snaps[hi - 1], "%s form %d cuts %s after step %d" % (what, split, cuts, hi - 1))


def every_cut(T):
    """one launch, every two-launch cut, and T one-step launches"""
    cuts = [(0, T)] + [(0, c, T) for c in range(1, T)]
    if T > 2:
        cuts.append(tuple(range(T + 1)))
    return cuts


# ---------------------------------------------------------------------------------------------------------------------
# the oracle with the in-kernel restart replayed on the host
def oracle_rollout(spec, cfg, pool, env_ids, acts, first_offset, stride):
    """The oracle stepping envs `env_ids` through acts[:, env_ids]; on done an env restarts from the scenario pool
    exactly as the in-kernel reset does (mcn.h mcn_rollout: humans <- pool[next_case], first-arrival times cleared,
    robot back to its start pose at rest, clock 0, next_case += stride mod P).  Env e starts from case e % P and its
    first restart takes case (e + first_offset) % P.  Returns the final state, the last step's outputs, restarts per
    env, counted overlaps per env and the number of 3-D LP entries."""
    from modelcrowdnav_amd.envs import scenarios as S
    env_ids = np.asarray(env_ids)
    n, P = len(env_ids), len(pool)
    st = cport.EnvState(n, pool.shape[1])

    def load(rows, cases):
        sc = pool[cases]
        st.hpx[rows], st.hpy[rows], st.hgx[rows], st.hgy[rows] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
        st.hvx[rows], st.hvy[rows] = sc[..., S.VX], sc[..., S.VY]
        st.hr[rows], st.hvpref[rows] = sc[..., S.RAD], sc[..., S.VPREF]
        st.human_times[rows] = 0
        rr = spec.robot_row()
        st.rpx[rows], st.rpy[rows], st.rgx[rows], st.rgy[rows] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
        st.rvx[rows], st.rvy[rows], st.rr[rows], st.gtime[rows] = 0.0, 0.0, rr[S.RAD], 0.0
    load(np.arange(n), env_ids % P)
    next_case = (env_ids + first_offset) % P
    restarts, overlaps = np.zeros(n, int), np.zeros(n, int)
    cport.lp3_entries(reset=True)
    for t in range(acts.shape[0]):
        a = acts[t][env_ids]
        ref = cport.env_step(cfg, st, a[:, 0].copy(), a[:, 1].copy(), update=True)
        overlaps += ref["hh_count"]
        d = np.nonzero(ref["done"])[0]
        if len(d):
            load(d, next_case[d])
            next_case[d] = (next_case[d] + stride) % P
            restarts[d] += 1
    return st, ref, restarts, overlaps, cport.lp3_entries()


# ---------------------------------------------------------------------------------------------------------------------
# registers, scratch and LDS of the built kernels
_RESOURCE_ROW = re.compile(r"^(\S.*?)\s+vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(\d+) vspill (\d+)\s*$",
                           re.M)


def parse_resources(text):
    """{kernel signature as tools/kernel_resources.py prints it: (vgpr, agpr, sgpr, scratch, lds, vspill)}"""
    return {name.strip(): tuple(int(v) for v in vals) for name, *vals in _RESOURCE_ROW.findall(text)}


@functools.lru_cache(maxsize=None)
def kernel_resources(filter=None):
    """parse_resources of tools/kernel_resources.py [filter] on the built library's objects, run once per filter."""
    from modelcrowdnav_amd import _hip                     # the library is built and loads: so its objects must be there
    assert os.path.exists(_hip.LIB_PATH)
    assert os.path.exists(os.path.join(ROOT, "modelcrowdnav_amd", "csrc", "env_rollout_quad.o")), \
        "libmcn_hip.so is there but the objects it was linked from are not: rebuild (make -C modelcrowdnav_amd/csrc)"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py")] + ([filter] if filter else [])
    return parse_resources(subprocess.run(cmd, capture_output=True, text=True, check=True).stdout)
