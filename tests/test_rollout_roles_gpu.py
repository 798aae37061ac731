"""The float64 wavefront's eight-lane layout in the four-wavefront rollout form (env_rollout_wg4_kernel,
mcn_tuning.rollout_split = 2).

The float64 wavefront holds an env on eight lanes (five humans, three idle lanes) and reduces the env's minimum
distance and overlap count inside them with three DPP exchanges, in another order than the lane order of the other
forms: NaN distances, an all-NaN env and two equal minima must not see the difference, and every workgroup filling
(less than one, exactly one, a ragged second, a ragged third) leaves the bytes of single mcn_env_step calls.

The per-workgroup choice of the float64 wave that was planned with this layout was not built: the census of
profiles/r13_rollout_roles.txt shows the float64 wavefronts of a CU on different SIMDs already, so there is no
placement to force and no rule to test."""
import numpy as np
import pytest

from tests import helpers as H
from tests import ladder_states as L
from tests.rollout_harness import assert_same_bytes, launch, launch_cuts, need_gpu, pool_env, random_actions, snapshot

N = 5

_single_steps = {}


def _single_step_reference(E, kinematics, T):
    """T mcn_env_step calls on the shared action sequence, computed once per configuration and left unchanged."""
    torch = need_gpu()
    key = (E, kinematics)
    if key not in _single_steps:
        b = pool_env(E, N, kinematics=kinematics)
        acts_d = torch.from_numpy(random_actions(kinematics, T, E, 5)).to(b.device)
        for t in range(T):
            b.step(acts_d[t])
        torch.cuda.synchronize()
        _single_steps[key] = snapshot(b)
    return _single_steps[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("E", [1, 8, 9, 17])
def test_eight_lane_layout_equals_single_steps(E, kinematics, tuning):
    """Less than a workgroup, exactly one, a ragged second, a ragged third: every byte of state, step record, Explorer
    record and finished-episode records after launches of 30 + 1 + 79 steps equals 110 single steps; every env
    finishes, and so restarts from the pool, inside them."""
    torch = need_gpu()
    T = 110
    ref = _single_step_reference(E, kinematics, T)
    tuning(rollout_fused=1)
    tuning(rollout_split=2)
    a = pool_env(E, N, kinematics=kinematics)
    acts_d = torch.from_numpy(random_actions(kinematics, T, E, 5)).to(a.device)
    for lo, hi in ((0, 30), (30, 31), (31, T)):
        launch(a, acts_d[lo:hi], 2)
    torch.cuda.synchronize()
    assert_same_bytes(snapshot(a), ref)
    assert int(a.rollout_buffers["fin_count"].min().item()) >= 1


# ---------------------------------------------------------------------------------------------------------------------
# reduction order: 9 envs on the constructions of tests/ladder_states.py (robot at the origin moving along +x, humans on
# a lattice out of everyone's way)
_E = 9
_ONE_NAN, _ALL_NAN, _TOUCH = 2, 4, 6


def _reduction_state():
    rng = np.random.RandomState(3)
    st, ax, _ = L._base(rng, _E, N, (0.3,), origin=True)
    st.gtime[:] = 0.0
    st.hpx[_ONE_NAN, 3] = np.nan                       # one distance NaN, in the env's second group of four lanes
    st.hpx[_ALL_NAN, :] = np.nan; st.hpy[_ALL_NAN, :] = np.nan
    # two humans whose swept distance minus the radii is exactly 0, in different groups of four lanes, on either side
    L._swept(st, _TOUCH, 1, ax[_TOUCH], 0.0, "perp", 1, 1 / 8)
    L._swept(st, _TOUCH, 4, ax[_TOUCH], 0.0, "perp", -1, 1 / 8)
    return st, ax


def _reduction_run(split, T):
    torch = need_gpu()
    st, ax = _reduction_state()
    env = pool_env(_E, N)
    H.upload(env, st)
    acts = np.zeros((T, _E, 2))
    acts[:, :, 0] = ax                                  # the velocity the constructions were laid out for
    launch_cuts(env, torch.from_numpy(acts).to(env.device), split, (0, T))
    torch.cuda.synchronize()
    return env, snapshot(env)


@pytest.mark.gpu
def test_reduction_order_is_not_seen(tuning):
    """One human at a NaN position, all five at NaN, and two humans exactly touching the robot's swept circle: three
    steps in the four-wavefront form leave the bytes of the two-wavefront form, which reduces in lane order.  The first
    step alone shows that the inputs are what they are meant to be: the all-NaN env's minimum is +inf, the one-NaN
    env's a number, the touching env's exactly 0 (DANGER, not a collision)."""
    from modelcrowdnav_amd import _hip
    tuning(rollout_fused=1)
    env1, one = _reduction_run(2, 1)
    dmin, info = env1.dmin.cpu().numpy(), env1.info.cpu().numpy()
    assert dmin[_ALL_NAN] == np.inf and np.isfinite(dmin[_ONE_NAN]), dmin
    assert dmin[_TOUCH] == 0.0 and not np.signbit(dmin[_TOUCH]) and info[_TOUCH] == _hip.INFO_DANGER, (dmin, info)
    assert_same_bytes(one, _reduction_run(1, 1)[1], "T = 1")
    assert_same_bytes(_reduction_run(2, 3)[1], _reduction_run(1, 3)[1], "T = 3")
