"""No GPU: the host side of the closed loop with an ORCA robot over social-force pedestrians -- mcn_env_rollout_orca_sf's
validation and ABI footprint, the Explorer's automatic rule, and the workloads of tests/test_closed_loop_sf_gpu.py's
host check (tests/closed_loop_sf_ref.py), forecast with the oracle alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = 0x1000                                 # never dereferenced: validation fails first
nan, inf = float("nan"), float("inf")


def cfg(policy=_hip.HUMANS_SOCIALFORCE, kin=_hip.KIN_HOLONOMIC, dt=0.25):
    return _hip.EnvCfg(dt, 25.0, 1.0, -0.25, 0.2, 0.5, 0.0, 10.0, 5.0, 10, 1, policy, kin, 1, 0)


st = _hip.EnvState(*([fake] * 13))
out = _hip.EnvOut(fake, None, fake, fake, None)


def call(c=None, sf=(4.0, 0.2, 2.0), st_=st, out_=out, roll=None, ss=0.15, nd=10.0, mn=10, th=5.0, T=8, E=4, N=5,
         traces=(None,) * 6):
    c = cfg() if c is None else c
    return lib.mcn_env_rollout_orca_sf(c, sf[0], sf[1], sf[2], st_, ss, nd, mn, th, T, out_, roll, *traces, E, N, None)


# positive control, made only once the runtime itself confirms that it sees no device (never a launch on fake
# addresses): the acceptable call gets past validation and fails at the launch
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert call() == _hip.MCN_ELAUNCH, call()
    assert call(sf=(0.0, 1e-3, 0.0), mn=0, N=_hip.MAX_HUMANS, T=1, traces=(fake,) * 6) == _hip.MCN_ELAUNCH
    print("POSITIVE_CONTROL_OK")
EINVAL = _hip.MCN_EINVAL
sfa = (4.0, 0.2, 2.0)
assert lib.mcn_env_rollout_orca_sf(None, *sfa, st, 0.15, 10.0, 10, 5.0, 8, out, None, *([None] * 6), 4, 5, None) == EINVAL
assert lib.mcn_env_rollout_orca_sf(cfg(), *sfa, None, 0.15, 10.0, 10, 5.0, 8, out, None, *([None] * 6), 4, 5, None) == EINVAL
assert lib.mcn_env_rollout_orca_sf(cfg(), *sfa, st, 0.15, 10.0, 10, 5.0, 8, None, None, *([None] * 6), 4, 5, None) == EINVAL
assert call(st_=_hip.EnvState()) == EINVAL and call(out_=_hip.EnvOut()) == EINVAL
for name in ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal", "rrad", "rvpref", "gtime"):
    one = _hip.EnvState(*([fake] * 13))
    setattr(one, name, None)
    assert call(st_=one) == EINVAL, name
assert call(T=0) == EINVAL and call(T=-3) == EINVAL
assert call(N=0) == EINVAL and call(N=_hip.MAX_HUMANS + 1) == EINVAL and call(N=-1) == EINVAL and call(E=0) == EINVAL
assert call(mn=-1) == EINVAL and call(mn=_hip.MAX_LINES + 1) == EINVAL
assert call(th=0.0) == EINVAL and call(th=-5.0) == EINVAL and call(th=nan) == EINVAL
assert call(c=cfg(dt=0.0)) == EINVAL and call(c=cfg(dt=-0.25)) == EINVAL and call(c=cfg(dt=1e-60)) == EINVAL
assert call(c=cfg(dt=nan)) == EINVAL
assert call(ss=nan) == EINVAL and call(ss=inf) == EINVAL and call(ss=-inf) == EINVAL
assert call(c=cfg(kin=_hip.KIN_UNICYCLE)) == EINVAL
for policy in (_hip.HUMANS_ORCA, _hip.HUMANS_LINEAR, _hip.HUMANS_GIVEN, 4, -1):
    assert call(c=cfg(policy)) == EINVAL, policy
for bad in (-1.0, nan, inf, -inf):
    assert call(sf=(bad, 0.2, 2.0)) == EINVAL, ("strength", bad)
    assert call(sf=(4.0, 0.2, bad)) == EINVAL, ("relaxation_rate", bad)
for bad in (0.0, -0.2, nan, inf):
    assert call(sf=(4.0, bad, 2.0)) == EINVAL, ("range", bad)
r = _hip.Rollout()
r.state, r.fin_slots = fake, 1                                                 # state without a discount table
assert call(roll=r) == EINVAL
# the ORCA / linear entry point still turns social-force humans away
assert lib.mcn_env_rollout_orca(cfg(), st, 0.15, 10.0, 10, 5.0, 8, out, None, *([None] * 6), 4, 5, None) == EINVAL
assert lib.mcn_abi_version() == 5 == _hip.ABI_VERSION
print("ORCA_SF_ROLLOUT_VALIDATION_OK")
"""


def test_entry_point_validates_on_host():
    """Each MCN_EINVAL case of mcn_env_rollout_orca_sf, in a fresh child process that sees NO device: the pointers are
    fakes, so a check that went missing would launch on them, which there fails with MCN_ELAUNCH instead of faulting a
    GPU that others share."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "ORCA_SF_ROLLOUT_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def test_abi_footprint():
    """A new entry point and nothing else: ABI 5, no new struct id, the name in the header and in the binding's list."""
    from modelcrowdnav_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "mcn.h")).read()
    assert int(re.search(r"#define\s+MCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _hip.lib.mcn_abi_version()
    assert _hip.lib.mcn_sizeof(15) == -1
    assert re.search(r"\bint\s+mcn_env_rollout_orca_sf\s*\(", hdr)
    assert "mcn_env_rollout_orca_sf" in _hip.EXPORTED and hasattr(_hip.lib, "mcn_env_rollout_orca_sf")
    # strength, range, relaxation_rate right after cfg, then mcn_env_rollout_orca's own arguments unchanged
    args = lambda name: [a.strip() for a in re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr).group(1).replace("\n", " ").split(",")]
    base, sf = args("mcn_env_rollout_orca"), args("mcn_env_rollout_orca_sf")
    assert sf == base[:1] + ["double strength", "double range", "double relaxation_rate"] + base[1:]
    assert (_hip.lib.mcn_env_rollout_orca_sf.argtypes[4:] == _hip.lib.mcn_env_rollout_orca.argtypes[1:]
            and len(_hip.lib.mcn_env_rollout_orca_sf.argtypes) == len(sf))


def _explorer(humans, kinematics="holonomic"):
    from modelcrowdnav_amd.envs.crowd_sim import VecCrowdSim
    from modelcrowdnav_amd.rollout import VecExplorer
    from tests import helpers as H
    env = H.make_vec_env(4, 5, kinematics=kinematics, cls=lambda E: VecCrowdSim(E, device="cpu"),
                         **{"humans.policy": humans})
    assert env.human_policy_name == humans
    return VecExplorer(env, env.robot, gamma=0.9, policy=env.robot.policy)


def test_explorer_rule_accepts_social_force_humans():
    """VecExplorer._closed_loop_ok: an ORCA robot choosing every action on a social-force env takes the closed loop, as
    on an ORCA env; a unicycle robot, an action_fn, an action_seq and a standing robot do not."""
    import torch
    from modelcrowdnav_amd import rollout
    from modelcrowdnav_amd.policy.lstm_rl import LstmRL
    from modelcrowdnav_amd.policy.sarl import SARL
    for humans in ("socialforce", "orca"):
        ex = _explorer(humans)
        assert ex._closed_loop_ok(None, None, None, False), humans
        assert not ex._closed_loop_ok(None, lambda env, t: None, None, False)
        assert not ex._closed_loop_ok(None, None, torch.zeros(3, 4, 2, dtype=torch.float64), False)
        assert not ex._closed_loop_ok(None, None, None, True)
        assert not _explorer(humans, "unicycle")._closed_loop_ok(None, None, None, False)
        # memory rows: served from the trace for SARL, not for what needs more than the trace
        sarl = SARL(); sarl.kinematics, sarl.with_om = "holonomic", False
        assert ex._closed_loop_ok(sarl, None, None, False)
        om = SARL(); om.kinematics, om.with_om = "holonomic", True
        assert not ex._closed_loop_ok(om, None, None, False) and not ex._closed_loop_ok(LstmRL(), None, None, False)
        # another robot policy stays per-step
        ex.policy = sarl
        assert not ex._closed_loop_ok(None, None, None, False)
    assert rollout.VecExplorer._closed_loop_ok.__doc__ and "social-force" in rollout.VecExplorer._closed_loop_ok.__doc__


def test_lds_sizing_restated():
    """The restated sizing against hand-counted values: the staging tiles are 104 bytes per lane, a row of lines 16; R
    rows of lines bring R - 1 rows of projected lines."""
    from tests import closed_loop_sf_ref as F
    assert F.lds_bytes(32, 10) == 64 * (16 * 19 + 104) == 26112      # the largest request
    assert F.lds_bytes(1, 10) == 64 * (16 + 104) and F.lds_bytes(5, 3) == 64 * (16 * 5 + 104)
    assert F.lds_bytes(5, 0) == 64 * 104
    assert F.lds_bytes(32, 10) <= 64 * 1024                           # one workgroup's LDS limit is far away


@pytest.mark.parametrize("visible", (False, True))
@pytest.mark.parametrize("N", (1, 5, 10))
def test_host_workloads_keep_clear_of_the_thresholds(N, visible):
    """The oracle alone (its own ORCA action, the restatement's velocities with libm's exp) on the workloads of the GPU
    test's host check: swept distances and the goal test stay far from the ladder's thresholds -- 1e-4, five orders
    above the 1e-9 the GPU test asks of the device run, which differs by ulps of exp -- and the run meets ReachGoal,
    Timeout and Danger or Collision, restarts from the pool and changes radii."""
    from tests import closed_loop_sf_ref as F
    ls = F.forecast(N, visible)
    assert ls.margin > 1e-4, ls.margin
    assert ls.covered(), sorted(ls.infos)
    ev = ls.rep.events
    assert ev["restart"] >= F.E and ev["timeout"] > 0 and ev["reach"] > 0 and ev["dropped"] > 0, dict(ev)
    assert ls.radii_changed
    assert ls.robot_lp3 > 0, "no robot solve goes into the 3-D LP"
    w = F.workload(N, visible)
    assert (w.st0.hr < 0.3).all() and len(np.unique(w.pool["hrad"])) > 1
