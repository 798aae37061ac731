"""No GPU: the host side of the closed loop with an ORCA robot -- mcn_env_rollout_orca's validation and ABI footprint,
and the step that turns a launch's trace into replay-memory rows."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = 0x1000                                 # never dereferenced: validation fails first


def cfg(policy=_hip.HUMANS_ORCA, kin=_hip.KIN_HOLONOMIC, dt=0.25):
    return _hip.EnvCfg(dt, 25.0, 1.0, -0.25, 0.2, 0.5, 0.0, 10.0, 5.0, 10, 1, policy, kin, 1, 0)


st = _hip.EnvState(*([fake] * 13))
out = _hip.EnvOut(fake, None, fake, fake, None)


def call(c=None, st_=st, out_=out, roll=None, ss=0.15, nd=10.0, mn=10, th=5.0, T=8, E=4, N=5, traces=(None,) * 6):
    c = cfg() if c is None else c
    return lib.mcn_env_rollout_orca(c, st_, ss, nd, mn, th, T, out_, roll, *traces, E, N, None)


# positive control, made only once the runtime itself confirms that it sees no device (never a launch on fake
# addresses): the acceptable call gets past validation and fails at the launch
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert call() == _hip.MCN_ELAUNCH, call()
    assert call(c=cfg(_hip.HUMANS_LINEAR), mn=0, N=_hip.MAX_HUMANS, T=1, traces=(fake,) * 6) == _hip.MCN_ELAUNCH
    print("POSITIVE_CONTROL_OK")
EINVAL = _hip.MCN_EINVAL
assert lib.mcn_env_rollout_orca(None, st, 0.15, 10.0, 10, 5.0, 8, out, None, *([None] * 6), 4, 5, None) == EINVAL
assert lib.mcn_env_rollout_orca(cfg(), None, 0.15, 10.0, 10, 5.0, 8, out, None, *([None] * 6), 4, 5, None) == EINVAL
assert lib.mcn_env_rollout_orca(cfg(), st, 0.15, 10.0, 10, 5.0, 8, None, None, *([None] * 6), 4, 5, None) == EINVAL
assert call(st_=_hip.EnvState()) == EINVAL and call(out_=_hip.EnvOut()) == EINVAL
no_vpref = _hip.EnvState(*([fake] * 13)); no_vpref.rvpref = None
assert call(st_=no_vpref) == EINVAL
assert call(T=0) == EINVAL and call(T=-3) == EINVAL
assert call(N=0) == EINVAL and call(N=_hip.MAX_HUMANS + 1) == EINVAL and call(E=0) == EINVAL
assert call(mn=-1) == EINVAL and call(mn=_hip.MAX_LINES + 1) == EINVAL
assert call(th=0.0) == EINVAL and call(th=-5.0) == EINVAL and call(th=float("nan")) == EINVAL
assert call(c=cfg(dt=0.0)) == EINVAL and call(c=cfg(dt=-0.25)) == EINVAL and call(c=cfg(dt=1e-60)) == EINVAL
assert call(ss=float("nan")) == EINVAL and call(ss=float("inf")) == EINVAL
assert call(c=cfg(kin=_hip.KIN_UNICYCLE)) == EINVAL
for policy in (_hip.HUMANS_GIVEN, _hip.HUMANS_SOCIALFORCE, 4, -1):
    assert call(c=cfg(policy)) == EINVAL, policy
r = _hip.Rollout()
r.state, r.fin_slots = fake, 1                                                 # state without a discount table
assert call(roll=r) == EINVAL
assert lib.mcn_abi_version() == 5 == _hip.ABI_VERSION
print("ORCA_ROLLOUT_VALIDATION_OK")
"""


def test_entry_point_validates_on_host():
    """Each MCN_EINVAL case of mcn_env_rollout_orca, in a fresh child process that sees NO device: the pointers are
    fakes, so a check that went missing would launch on them, which there fails with MCN_ELAUNCH instead of faulting a
    GPU that others share."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "ORCA_ROLLOUT_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def test_abi_footprint():
    """A new entry point and nothing else: ABI 5, no new struct id, the name in the header and in the binding's list."""
    from modelcrowdnav_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "mcn.h")).read()
    assert int(re.search(r"#define\s+MCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5 == _hip.lib.mcn_abi_version()
    assert _hip.lib.mcn_sizeof(15) == -1
    assert re.search(r"\bint\s+mcn_env_rollout_orca\s*\(", hdr)
    assert "mcn_env_rollout_orca" in _hip.EXPORTED and hasattr(_hip.lib, "mcn_env_rollout_orca")


def _random_trace(rng, T, E, N):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tr = dict(robot=t(rng.uniform(-4, 4, (T, E, 5))), humans=t(rng.uniform(-5, 5, (T, E, N, 4))),
              hrad=t(np.full((T, E, N), 0.3)))
    tr["hrad"][T // 2:, 1] = t(rng.uniform(0.3, 0.5, (T - T // 2, N)))[:, None, :].expand(-1, 1, -1)[:, 0]   # a restart
    tr["humans"][3, 0, :, 0:2] = tr["robot"][3, 0, 0:2]             # a human on the robot: da = 0
    return tr


def test_trace_rows_equal_per_step_rows():
    """transform_batch once over the stacked [T * E] view of a trace equals T per-step calls, bit for bit, for the
    policies whose rows are served from the trace (SARL's joint states, CADRL's one-human rows).
    64 envs on purpose: torch's CPU kernels run whole SIMD blocks through a vector math library and the remainder of a
    tensor through libm, whose float32 atan2 differs in the last bit, so on the CPU a row's bits depend on its position
    modulo the block (32 floats at most) -- with a multiple of 64 rows per step every row takes the vector path in both
    forms.  The device kernels have one atan2; tests/test_closed_loop_gpu.py compares the memory rows there at 8 x 5."""
    import torch
    from types import SimpleNamespace
    from modelcrowdnav_amd import rollout
    from modelcrowdnav_amd.policy.cadrl import CADRL
    from modelcrowdnav_amd.policy.lstm_rl import LstmRL
    from modelcrowdnav_amd.policy.sarl import SARL
    rng = np.random.RandomState(0)
    for cls, N in ((SARL, 5), (SARL, 7), (CADRL, 1)):
        T, E = 5, 64
        pol = cls()
        pol.kinematics, pol.with_om = "holonomic", False
        tr = _random_trace(rng, T, E, N)
        assert len(torch.unique(tr["hrad"])) > 1
        rrad, rvpref = torch.full((E,), 0.3, dtype=torch.float64), torch.ones(E, dtype=torch.float64)
        rgoal = torch.tensor([[0.0, 4.0]], dtype=torch.float64).repeat(E, 1)
        env = SimpleNamespace(hcount=None)
        assert rollout.rows_from_trace_ok(pol, env)
        got = rollout.trace_state_rows(pol, tr, rrad, rgoal, rvpref)
        for t in range(T):
            step = SimpleNamespace(num_envs=E, _alloc_N=N, device=torch.device("cpu"), rpos=tr["robot"][t, :, 0:2],
                                   rvel=tr["robot"][t, :, 2:4], rtheta=tr["robot"][t, :, 4], rrad=rrad, rgoal=rgoal,
                                   rvpref=rvpref, hpos=tr["humans"][t, :, :, 0:2], hvel=tr["humans"][t, :, :, 2:4],
                                   hrad=tr["hrad"][t])
            want = pol.transform_batch(step)
            assert got[t].dtype == want.dtype == torch.float32
            assert got[t].numpy().tobytes() == want.numpy().tobytes(), (cls.__name__, N, t)
    # what needs more than the trace stays on the per-step loop
    om = SARL(); om.with_om = True
    assert not rollout.rows_from_trace_ok(om, SimpleNamespace())
    assert not rollout.rows_from_trace_ok(LstmRL(), SimpleNamespace())
    assert not rollout.rows_from_trace_ok(pol, SimpleNamespace(hcount=torch.ones(3, dtype=torch.int32)))
