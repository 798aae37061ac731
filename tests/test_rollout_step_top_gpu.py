"""The top of the ORCA wavefronts' step in the four-wavefront rollout form (env_rollout_wg4_kernel, rollout_split = 2).

On a normal step an ORCA wavefront reads only the two position packs behind hand-off 2: its own velocity is the (rx, ry)
its quad still holds from the solve, the candidate's velocity is read between the hand-offs, and frad, the maximum speed
and the candidate's frad stay in registers.  The float64 wavefront publishes a
workgroup flag before hand-off 1; when it is set (some env of the workgroup restarts) and on the first step of every
launch all four wavefronts take the slow path behind hand-off 2: every operand re-read from LDS, one more barrier.  What
can go wrong there and nowhere else:

  * the flag: a stale one (slow path not taken after a restart, or taken for ever), every transition between restart
    and quiet steps, a restart on the first and on the last step of a launch, launches of one and two steps -- a
    miscounted barrier hangs or reads early;
  * registers kept across a restart: frad, the maximum speed and the candidate's frad of the humans the slots held before
    (consecutive pool cases differ in every radius and v_pref), the quad's last (rx, ry) where the start velocity belongs;
  * a workgroup in which one env restarts and seven do not: everybody takes the slow path and must read what it held;
    envs 3 and 6 of a workgroup straddle two ORCA wavefronts, so the owner's quad and a candidate's sit in different
    wavefronts.  (An env restarts as a whole: owner and candidates of one solve always restart together.  "Owner only"
    and "candidate only" are therefore taken per WAVEFRONT: the restarting env's owner quad in one wavefront and its
    candidates' quads in the next, and the other way round, against an env that sits in one wavefront.)
  * the bits of a velocity that now stays in a register from one step to the next: denormals, -0, NaN.

Every comparison is of BYTES: full state, step record, Explorer record and finished-episode arrays of the forced
four-wavefront form after EVERY launch against single mcn_env_step calls at that step.  Every forced launch asserts
mcn_last_rollout_form() == 2 (rollout_harness.launch).  Each test first shows, from the single-step run, that its inputs
produce the situation it is about."""
import os
import subprocess

import numpy as np
import pytest

from oracle import cport
from tests import helpers as H
from tests.rollout_harness import (ROOT, as_device_pool, every_cut, kernel_resources, launches_against, parse_resources,
                                   single_steps)

N = 5
_P, _LIMIT = 8, 3               # pool cases; time_limit 3 s: an env whose clock reads 2 s at a step times out on it
NEVER = 100


def _env(E, kinematics, first_done, with_hvel=True):
    """E envs on an 8-case pool with randomised radii and v_pref and start velocities no float32 holds; the robot stands
    still far from everybody's path, so an env ends by its clock alone: env e at step first_done[e] (NEVER: not in
    these tests) and on the ninth step of every new episode.  Returns (env, pool)."""
    import torch
    from modelcrowdnav_amd.envs import scenarios as S
    env = H.make_vec_env(E, N, kinematics=kinematics, **{"env.time_limit": _LIMIT, "env.randomize_attributes": "true"})
    pool = S.scenario_pool(env.spec(), "test", range(_P), N, "circle_crossing").copy()
    pool[:, :, S.VX], pool[:, :, S.VY] = 0.1, -0.3
    ids = np.arange(E)
    env.load_scenarios(pool[ids % _P])
    far = torch.tensor([30.0, 30.0], dtype=torch.float64, device=env.device)
    env.rpos.copy_(far.expand(E, 2)); env.rgoal.copy_((far + 5.0).expand(E, 2))
    clock = 2.0 - 0.25 * np.asarray(first_done, dtype=np.float64)      # multiples of 1 / 4: exact
    env.gtime.copy_(torch.from_numpy(clock).to(env.device))
    env.attach_rollout(gamma=0.9, pool=pool if with_hvel else as_device_pool(env, pool), case_stride=1,
                       first_cases=(ids + 1) % _P, fin_slots=3)
    return env, pool


def _still(T, E):
    return np.zeros((T, E, 2))


def _wg_flags(done):
    """[T, workgroups]: some env of the workgroup (8 envs) restarts on that step"""
    T, E = done.shape
    pad = np.zeros((T, -(-E // 8) * 8), bool)
    pad[:, :E] = done
    return pad.reshape(T, -1, 8).any(2)


def _check(build, acts, snaps, cut_list, what):
    T = len(acts)
    for cuts in cut_list:
        assert cuts[0] == 0 and cuts[-1] <= T and all(a < b for a, b in zip(cuts[:-1], cuts[1:])), cuts
        launches_against(build, acts, 2, cuts, snaps, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the flag
@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
def test_flag_transitions_every_cut(kinematics, tuning):
    """9 envs, 12 steps.  Workgroup 0 restarts on steps 0 and 1 (two in a row), is quiet on 2-4, restarts on 5, is quiet
    on 6, restarts on 7, is quiet on 8, restarts on 9 and 10 (envs 0 and 1 again) and on the last step; workgroup 1
    (env 8) on step 3 alone.  One
    launch, every two-launch cut and twelve one-step launches: every step is once the first and once the last of a
    launch, a launch that follows a restart step starts clean, and the one-step launches run the slow path only.  Then
    the first one and two steps as sequences of their own."""
    tuning(rollout_fused=1)
    E, T = 9, 12
    first = [0, 1, 5, 5, 7, 11, NEVER, NEVER, 3]
    build = lambda: _env(E, kinematics, first)[0]
    acts = _still(T, E)
    _, snaps, _, done = single_steps(build, acts)
    want = np.zeros((T, E), bool)
    for e, s in enumerate(first):
        want[s::9, e] = True                                     # and on the ninth step of the new episode
    assert (done == want).all(), "the envs do not restart by their clocks alone:\n%s" % done.astype(int)
    f = _wg_flags(done)[:, 0]
    assert f[0] and f[1] and not f[2], "no restart on two consecutive steps followed by a quiet one"
    assert not f[4] and f[5] and not f[6] and f[7], "no quiet -> restart -> quiet -> restart"
    assert f[T - 1] and _wg_flags(done)[3, 1] and not f[3]
    _check(build, acts, snaps, every_cut(T), "flag %s" % kinematics)
    _check(build, acts[:1], snaps, [(0, 1)], "flag T=1 %s" % kinematics)
    _check(build, acts[:2], snaps, [(0, 2), (0, 1, 2)], "flag T=2 %s" % kinematics)


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 4. one env of a workgroup restarts, the others do not; what the slot held before must not survive
_LONE = {1: {0: 1},                                      # E: {env: step of its restart}
         8: {3: 1, 6: 3, 0: 5},
         9: {3: 1, 6: 3, 0: 5, 8: 2},
         19: {3: 1, 6: 3, 0: 5, 11: 2, 14: 4, 17: 1}}


@pytest.mark.gpu
@pytest.mark.parametrize("E,kinematics", [(1, "holonomic"), (8, "holonomic"), (9, "holonomic"), (19, "holonomic"),
                                          (9, "unicycle")])
def test_lone_restart_in_a_workgroup(E, kinematics, tuning):
    """7 steps.  On each restart step of a workgroup exactly ONE of its envs restarts: env 3 (its human 0 in ORCA wavefront
    0, humans 1-4 in wavefront 1), env 6 (humans 0-1 in wavefront 1, 2-4 in wavefront 2), env 0 (one wavefront); with 19
    envs also envs 11 and 14, the straddling ones of workgroup 1, and env 17 of the partial workgroup 2.  The restarted
    env's new case differs from the one it held in every human's radius and v_pref, so a kept frad, maximum speed or
    candidate's frad changes bytes; the seven others pass the slow path with unchanged operands."""
    from modelcrowdnav_amd.envs import scenarios as S
    tuning(rollout_fused=1)
    T = 7
    when = _LONE[E]
    first = [when.get(e, NEVER) for e in range(E)]
    build = lambda: _env(E, kinematics, first)[0]
    pool = _env(E, kinematics, first)[1]
    for col in (S.RAD, S.VPREF):
        assert (pool[:-1, :, col] != pool[1:, :, col]).all() and (pool[-1, :, col] != pool[0, :, col]).all(), \
            "consecutive cases share an attribute"
    acts = _still(T, E)
    _, snaps, start, done = single_steps(build, acts)
    want = np.zeros((T, E), bool)
    for e, s in when.items():
        want[s, e] = True
    assert (done == want).all(), done.astype(int)
    per_wg = np.add.reduceat(done.astype(int), np.arange(0, E, 8), axis=1)
    assert per_wg.max() == 1, "two envs of a workgroup restart on one step"
    for e, s in when.items():
        before = start if s == 0 else snaps[s - 1]
        for k in ("hrad", "hvpref"):
            assert (snaps[s][k][e] != before[k][e]).all(), "env %d restarts into the %s it had" % (e, k)
            others = [x for x in range(E) if x != e and not done[s, x]]
            assert (snaps[s][k][others] == before[k][others]).all()
    _check(build, acts, snaps, every_cut(T), "lone restart %s E=%d" % (kinematics, E))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the step after a restart solves with the start velocity
@pytest.mark.gpu
@pytest.mark.parametrize("with_hvel", [True, False])
def test_start_velocity_after_a_restart(with_hvel, tuning):
    """9 envs, 6 steps; envs 1, 3 and 8 restart on step 2.  With pool_hvel the start velocity is (0.1, -0.3), without it
    zero; either differs from the velocity the human's quad solved for on that step (exported as human_act) in every
    restarted human, so a step 3 solved with the quad's registers leaves other bytes.  Every cut: the step after the
    restart is also the first of a launch."""
    tuning(rollout_fused=1)
    E, T = 9, 6
    first = [NEVER, 2, NEVER, 2, NEVER, NEVER, NEVER, NEVER, 2]
    build = lambda: _env(E, "holonomic", first, with_hvel)[0]
    acts = _still(T, E)
    _, snaps, _, done = single_steps(build, acts)
    assert (done[2] == (np.array(first) == 2)).all() and not np.delete(done, 2, 0).any(), done.astype(int)
    vel, act = snaps[2]["hvel"][done[2]], snaps[2]["human_act"][done[2]]
    if with_hvel:
        assert (vel[..., 0] == 0.1).all() and (vel[..., 1] == -0.3).all()
    else:
        assert (vel == 0).all()
    assert (vel != act).any(-1).all(), "a restarted human's start velocity is the one its quad just solved for"
    quiet = snaps[2]["hvel"][~done[2]]
    assert (quiet == snaps[2]["human_act"][~done[2]]).all() and (quiet != 0).any()
    _check(build, acts, snaps, every_cut(T), "start velocity hvel=%s" % with_hvel)


# ---------------------------------------------------------------------------------------------------------------------
# 5. bits that stay in registers
_TINY = (1e-41, 1e-42, 1e-43, 1e-44, 1e-45, 1e-46, 1e-50)      # (float) of the last two is a zero


def _tiny_velocity_state():
    """9 envs.  Human 0 sits (+d, -d) off its goal at the origin, d = 1e-41 .. 1e-50 (envs 0-6) and 1e-41 (envs 7, 8), so
    its preferred and resulting velocity is (-d, +d) as float32: denormals, and -0 / +0 for the two smallest; humans
    1-4 stand 4 m away (in range) and walk outwards.  Env 7: a NaN goal for human 2, whose velocity and then position
    are NaN.  No pool: nothing restarts, so after the first step of a launch every velocity operand is a register."""
    E = 9
    st = cport.EnvState(E, N)
    out = np.array([(4.0, 0.0), (-4.0, 0.0), (0.0, 4.0), (0.0, -4.0)])
    for e in range(E):
        d = _TINY[e] if e < len(_TINY) else 1e-41
        st.hpx[e, 0], st.hpy[e, 0], st.hgx[e, 0], st.hgy[e, 0] = d, -d, 0.0, 0.0
        st.hpx[e, 1:], st.hpy[e, 1:] = out[:, 0], out[:, 1]
        st.hgx[e, 1:], st.hgy[e, 1:] = 2 * out[:, 0], 2 * out[:, 1]
    st.hvx[:] = 0; st.hvy[:] = 0
    st.hr[:] = 0.3; st.hvpref[:] = 1.0
    st.rpx[:], st.rpy[:], st.rgx[:], st.rgy[:] = 20.0, 20.0, 20.0, 25.0
    st.rvx[:] = 0; st.rvy[:] = 0; st.rr[:] = 0.3
    st.gtime[:] = 0
    st.hgx[7, 2] = np.nan
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
def test_register_velocities_keep_their_bits(kinematics, tuning):
    """Denormal, -0 and NaN velocities through 6 steps: the quad's (rx, ry) is the next step's own velocity without a
    trip through LDS, and the candidate's is read one interval earlier; same bytes, at every cut."""
    tuning(rollout_fused=1)
    st = _tiny_velocity_state()
    E, T = st.E, 6

    def build():
        env = H.make_vec_env(E, N, kinematics=kinematics)
        H.upload(env, st)
        env.attach_rollout(gamma=0.9, pool=None, fin_slots=2)
        return env
    acts = _still(T, E)
    _, snaps, _, done = single_steps(build, acts)
    assert not done.any()
    v = np.concatenate([s["human_act"].ravel() for s in snaps])
    v32 = v.astype(np.float32)
    assert (v32.astype(np.float64).view(np.uint64) == v.view(np.uint64))[~np.isnan(v)].all(), "a velocity is no float32"
    tiny = np.float32(2.0 ** -126)
    for t in range(1, T):                                        # on steps that carry them in registers, not only step 0
        w = snaps[t]["human_act"].astype(np.float32)
        assert ((np.abs(w) > 0) & (np.abs(w) < tiny)).any(), "no denormal velocity at step %d" % t
        assert ((w == 0) & np.signbit(w)).any(), "no -0 velocity at step %d" % t
        assert np.isnan(w).any(), "no NaN velocity at step %d" % t
    _check(build, acts, snaps, every_cut(T), "register bits %s" % kinematics)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
WG4_LDS = 5632


def test_step_top_kernel_resources():
    """Read from the built code objects: both env_rollout_wg4_kernel instantiations keep 5 632 B of LDS, use no scratch
    and spill nothing, in no more VGPRs than the parent's rows.  (profiles/r21_kernel_resources.txt lists only the
    three kernels that changed in that round and no row of this kernel; the parent's rows of this kernel are the
    `before` section of profiles/r22_kernel_resources.txt, 122 / 145 as DESIGN 3.1 (5) has had them since r18.)"""
    txt = open(os.path.join(ROOT, "profiles", "r22_kernel_resources.txt")).read()
    parent = parse_resources(txt[txt.index("# before"):txt.index("# after")])
    parent = {k: v for k, v in parent.items() if "env_rollout_wg4_kernel<" in k}
    assert sorted(v[0] for v in parent.values()) == [122, 145], parent
    now = {k: v for k, v in kernel_resources("env_rollout_wg4_kernel<").items() if "env_rollout_wg4_kernel<" in k}
    assert sorted(now) == sorted(parent), (sorted(now), sorted(parent))
    for name, (vgpr, agpr, sgpr, scratch, lds, vspill) in now.items():
        print("%s: vgpr %d sgpr %d scratch %d lds %d" % (name, vgpr, sgpr, scratch, lds))
        assert (agpr, scratch, vspill) == (0, 0, 0), (name, now[name])
        assert lds == WG4_LDS, (name, lds)
        assert vgpr <= parent[name][0], (name, vgpr, parent[name][0])


def test_diag_build_of_the_kernel_compiles(tmp_path):
    """The MCN_DIAG build of env_rollout_wg4.hip (time stamps and path counters inside the step loops) compiles with the
    Makefile's own rule and flags, into a directory of its own."""
    out = tmp_path / "env_rollout_wg4.o"
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "modelcrowdnav_amd", "csrc"), "DIAGDIR=%s" % tmp_path, str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "-DMCN_DIAG" in r.stdout and "-fno-slp-vectorize" in r.stdout, r.stdout
    assert out.exists() and out.stat().st_size > 0
