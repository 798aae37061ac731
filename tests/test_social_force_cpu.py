"""Social-force pedestrians without a GPU: the definition's restatement (tests/social_force_ref.py) on hand-computed
answers, the host policy against it bit for bit, the [social_force] configuration, the host-side argument validation of
mcn_env_step_sf / mcn_env_rollout_sf (in a child process that sees no device) and the sanity run behind the default
parameters (strength 4, range 0.2, relaxation_rate 2)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import social_force_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, K, DT = 4.0, 0.2, 2.0, 0.25


def _policy_velocity(p, v, g, r, s, others, prm=(A, B, K)):
    """The host policy (envs/policy/socialforce.py) on the same inputs."""
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.envs.utils.state import FullState, JointState, ObservableState
    pol = policy_factory["socialforce"]()
    pol.strength, pol.range, pol.relaxation_rate = prm
    pol.time_step = DT
    act = pol.predict(JointState(FullState(p[0], p[1], v[0], v[1], r, g[0], g[1], s, 0.0),
                                 [ObservableState(q[0], q[1], 0.0, 0.0, q[2]) for q in others]))
    return (act.vx, act.vy)


def _lone(p, v, g, r, s, others=()):
    """One human's velocity by the restatement; the host policy must give the same bits."""
    w = R.human_velocity(p, v, g, r, s, list(others), A, B, K, DT)[0]
    assert np.array(_policy_velocity(p, v, g, r, s, list(others))).tobytes() == np.array(w).tobytes()
    return w


def test_lone_human_known_answers():
    """No neighbour: relaxation only.  Every expected value below is exact in float64 (worked out by hand)."""
    # far from the goal: e = (3, 4) / 5 * 1 = (0.6, 0.8); a = 2 e = (1.2, 1.6); w = a / 4 = (0.3, 0.4), |w| = 0.5 < 1
    assert _lone((0.0, 0.0), (0.0, 0.0), (3.0, 4.0), 0.3, 1.0) == (0.3, 0.4)
    # within v_pref of the goal: e is the goal vector itself, (0.5, 0); a = (1, 0); w = (0.25, 0)
    assert _lone((0.0, 0.0), (0.0, 0.0), (0.5, 0.0), 0.3, 1.0) == (0.25, 0.0)
    # exactly on the goal: e = 0 (d = 0 is not > s, nothing is divided); a = -2 v = (-1, 0.5); w = v + a / 4
    assert _lone((1.0, 2.0), (0.5, -0.25), (1.0, 2.0), 0.3, 1.0) == (0.25, -0.125)
    # speed clip not engaged: e = (1, 0), a = 2 (1 - 0.75) = 0.5, w = 0.75 + 0.125 = 0.875 <= 1
    assert _lone((0.0, 0.0), (0.75, 0.0), (10.0, 0.0), 0.3, 1.0) == (0.875, 0.0)
    # ... and n == s exactly is not clipped either (strict >): v = 0, e = (1, 0) ... w = 0.5; with s = 0.5: e = (0.5, 0),
    # a = (1, 0), w = (0.25, 0); take v = (0.5, 0), s = 0.5: a = 0, w = (0.5, 0), n = 0.5 == s
    assert _lone((0.0, 0.0), (0.5, 0.0), (10.0, 0.0), 0.3, 0.5) == (0.5, 0.0)
    # speed clip engaged: on the goal with v = (3, 4): a = (-6, -8), w = (1.5, 2), n = 2.5 > 1, w = (1.5, 2) / 2.5 = (0.6, 0.8)
    assert _lone((0.0, 0.0), (3.0, 4.0), (0.0, 0.0), 0.3, 1.0) == (0.6, 0.8)


def test_zero_preferred_speed_stands_still():
    """v_pref = 0: the desired velocity is 0 and the speed clip multiplies whatever is left by 0."""
    for v in ((0.0, 0.0), (0.7, -0.2)):
        w = _lone((1.0, 1.0), v, (4.0, 5.0), 0.3, 0.0, [(1.5, 1.0, 0.3)])
        assert w[0] == 0.0 and w[1] == 0.0


def test_pair_known_answers():
    """One neighbour exactly touching (r + r_j == dist): exp(0) = 1, so m = A."""
    # human at the origin on its goal and at rest, neighbour at (1, 0), radii 0.5 + 0.5: a = (4 * (-1 / 1), 0), w = (-1, 0)
    assert _lone((0.0, 0.0), (0.0, 0.0), (0.0, 0.0), 0.5, 1.0, [(1.0, 0.0, 0.5)]) == (-1.0, 0.0)
    # the same with v_pref = 0.5: n = 1 > 0.5, w = (-1 / 1 * 0.5, 0 / 1 * 0.5)
    assert _lone((0.0, 0.0), (0.0, 0.0), (0.0, 0.0), 0.5, 0.5, [(1.0, 0.0, 0.5)]) == (-0.5, 0.0)
    # neighbour on the other axis, below: pushed up
    assert _lone((0.0, 0.0), (0.0, 0.0), (0.0, 0.0), 0.5, 1.0, [(0.0, -1.0, 0.5)]) == (0.0, 1.0)
    # a neighbour 800 m away: exp((0.6 - 800) / 0.2) underflows to 0, the lone answer is left
    assert _lone((0.0, 0.0), (0.0, 0.0), (3.0, 4.0), 0.3, 1.0, [(800.0, 0.0, 0.3)]) == (0.3, 0.4)
    assert math.exp((0.6 - 800.0) / 0.2) == 0.0


def test_coincident_agent_contributes_nothing():
    lone = _lone((1.0, -2.0), (0.2, 0.1), (3.0, 4.0), 0.3, 1.0)
    assert _lone((1.0, -2.0), (0.2, 0.1), (3.0, 4.0), 0.3, 1.0, [(1.0, -2.0, 0.4)]) == lone
    acts, _ = R.env_velocities([[1.0, -2.0], [1.0, -2.0]], [[0.2, 0.1], [0.0, 0.0]], [[3.0, 4.0], [-3.0, 0.0]],
                               [0.3, 0.4], [1.0, 1.0], A, B, K, DT)
    assert acts[0] == lone and acts[1] == _lone((1.0, -2.0), (0.0, 0.0), (-3.0, 0.0), 0.4, 1.0)


def test_robot_invisible_ignored_visible_added_last():
    pos, vel, goal = [[0.0, 0.0], [0.7, 0.1]], [[0.3, -0.2], [0.0, 0.0]], [[2.0, 1.0], [-2.0, 0.0]]
    rad, vpref, rob = [0.3, 0.3], [1.0, 1.0], (-0.2, 0.65, 0.35)
    without, _ = R.env_velocities(pos, vel, goal, rad, vpref, A, B, K, DT, robot=None)
    assert without[0] == _lone(pos[0], vel[0], goal[0], 0.3, 1.0, [(0.7, 0.1, 0.3)])
    seen, _ = R.env_velocities(pos, vel, goal, rad, vpref, A, B, K, DT, robot=rob)
    last = _lone(pos[0], vel[0], goal[0], 0.3, 1.0, [(0.7, 0.1, 0.3), rob])
    first = _lone(pos[0], vel[0], goal[0], 0.3, 1.0, [rob, (0.7, 0.1, 0.3)])
    assert seen[0] == last
    assert last != first, "these inputs were chosen so that the order of the sum shows in the last bit"
    assert seen[0] != without[0]
    # by hand, term by term, the robot's after the human's
    ex, ey = 2.0 / math.sqrt(5.0) * 1.0, 1.0 / math.sqrt(5.0) * 1.0
    ax, ay = K * (ex - 0.3), K * (ey + 0.2)
    for q in ((0.7, 0.1, 0.3), rob):
        dx, dy = 0.0 - q[0], 0.0 - q[1]
        dist = math.sqrt(dx * dx + dy * dy)
        m = A * math.exp((0.3 + q[2] - dist) / B)
        ax, ay = ax + m * (dx / dist), ay + m * (dy / dist)
    wx, wy = 0.3 + ax * DT, -0.2 + ay * DT
    n = math.sqrt(wx * wx + wy * wy)
    assert n <= 1.0 and seen[0] == (wx, wy)


def test_mirrored_head_on_pair_is_exactly_negated():
    """Every operation of the definition is odd in (p, v, g), so a point-mirrored pair gets exactly negated actions."""
    rng = np.random.RandomState(5)
    for _ in range(200):
        p, v, g = rng.uniform(-3, 3, 2), rng.uniform(-1, 1, 2), rng.uniform(-5, 5, 2)
        r, s = rng.uniform(0.3, 0.5), rng.uniform(0.5, 1.5)
        acts, mags = R.env_velocities([list(p), list(-p)], [list(v), list(-v)], [list(g), list(-g)], [r, r], [s, s],
                                      A, B, K, DT)
        assert acts[0][0] == -acts[1][0] and acts[0][1] == -acts[1][1] and mags[0] == mags[1]
        w0 = _policy_velocity(tuple(p), tuple(v), tuple(g), r, s, [(-p[0], -p[1], r)])
        w1 = _policy_velocity(tuple(-p), tuple(-v), tuple(-g), r, s, [(p[0], p[1], r)])
        assert w0 == acts[0] and w1 == acts[1] and w0[0] == -w1[0] and w0[1] == -w1[1]
    # the plain head-on case on one axis
    acts, _ = R.env_velocities([[-0.5, 0.0], [0.5, 0.0]], [[1.0, 0.0], [-1.0, 0.0]], [[4.0, 0.0], [-4.0, 0.0]],
                               [0.3, 0.3], [1.0, 1.0], A, B, K, DT)
    assert acts[0][0] == -acts[1][0] and acts[0][0] < 1.0 and acts[0][1] == 0.0 and acts[1][1] == 0.0


def test_policy_predict_equals_the_restatement_bitwise():
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.envs.utils.state import FullState, JointState, ObservableState
    pol = policy_factory["socialforce"]()
    assert (pol.strength, pol.range, pol.relaxation_rate) == (4.0, 0.2, 2.0) and pol.kinematics == "holonomic"
    pol.time_step = DT
    rng = np.random.RandomState(11)
    for trial in range(300):
        m = rng.randint(0, 7)
        p, v, g = rng.uniform(-4, 4, 2), rng.uniform(-1.2, 1.2, 2), rng.uniform(-5, 5, 2)
        r, s = rng.uniform(0.3, 0.5), rng.choice([0.0, 0.5, 1.0, rng.uniform(0.5, 1.5)])
        others = [(float(p[0] + rng.uniform(-1.5, 1.5)), float(p[1] + rng.uniform(-1.5, 1.5)), float(rng.uniform(0.3, 0.5)))
                  for _ in range(m)]
        if m and trial % 5 == 0:
            others[0] = (float(p[0]), float(p[1]), 0.3)                      # coincident
        if trial % 7 == 0:
            g = p.copy()                                                     # on the goal
        pol.strength, pol.range, pol.relaxation_rate = (A, B, K) if trial % 2 else (2.0, 1.0, 1.0)
        me = FullState(float(p[0]), float(p[1]), float(v[0]), float(v[1]), float(r), float(g[0]), float(g[1]), float(s), 0.0)
        act = pol.predict(JointState(me, [ObservableState(q[0], q[1], 0.1, -0.1, q[2]) for q in others]))
        want, _ = R.human_velocity((me.px, me.py), (me.vx, me.vy), (me.gx, me.gy), me.radius, me.v_pref, others,
                                   pol.strength, pol.range, pol.relaxation_rate, DT)
        got = np.array([act.vx, act.vy])
        assert got.tobytes() == np.array(want).tobytes(), (trial, got, want)


def _configured(**over):
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.envs.crowd_sim import VecCrowdSim
    cfg = configs.env_config(**{k: v for k, v in over.items() if not k.startswith("social_force.")})
    sf = {k: v for k, v in over.items() if k.startswith("social_force.")}
    if sf:
        cfg.add_section("social_force")
        for k, v in sf.items():
            cfg.set("social_force", k.split(".", 1)[1], str(v))
    env = VecCrowdSim(1, device="cpu")
    env.configure(cfg)
    return env


def test_configure_reads_the_section_and_its_defaults():
    from modelcrowdnav_amd import _hip
    env = _configured()
    assert env.human_policy_name == "orca"                                  # the shipped file is unchanged
    env = _configured(**{"humans.policy": "socialforce"})
    assert env.human_policy_name == "socialforce"
    assert (env._sf.strength, env._sf.range, env._sf.relaxation_rate) == (4.0, 0.2, 2.0)
    env = _configured(**{"humans.policy": "socialforce", "social_force.strength": 2.5, "social_force.range": 1.0})
    assert (env._sf.strength, env._sf.range, env._sf.relaxation_rate) == (2.5, 1.0, 2.0)
    env = _configured(**{"humans.policy": "socialforce", "social_force.relaxation_rate": 0.5})
    assert (env._sf.strength, env._sf.range, env._sf.relaxation_rate) == (4.0, 0.2, 0.5)

    class _Robot(object):
        visible, kinematics = True, "holonomic"
    env.set_robot(_Robot())
    assert env._cfg_struct().human_policy == _hip.HUMANS_SOCIALFORCE == 3
    assert env._cfg_struct("given").human_policy == _hip.HUMANS_GIVEN
    with pytest.raises(ValueError):
        _configured(**{"humans.policy": "socialforce", "social_force.range": 0.0})
    for name in ("linear", "social_force", "helbing"):
        with pytest.raises(NotImplementedError):
            _configured(**{"humans.policy": name})


def test_shipped_config_documents_the_section():
    text = open(os.path.join(ROOT, "modelcrowdnav_amd", "configs", "env.config")).read()
    for line in ("#[social_force]", "#strength = 4.0", "#range = 0.2", "#relaxation_rate = 2.0", "policy = orca"):
        assert line in text


_VALIDATION = r"""
import ctypes as C
from modelcrowdnav_amd import _hip
lib = _hip.lib
fake = 0x1000                                 # never dereferenced: validation fails first
SF = _hip.HUMANS_SOCIALFORCE
assert SF == 3


def cfg(policy=SF):
    return _hip.EnvCfg(0.25, 25.0, 1.0, -0.25, 0.2, 0.5, 0.0, 10.0, 5.0, 10, 1, policy, _hip.KIN_HOLONOMIC, 1, 0)


st = _hip.EnvState(*([fake] * 13))
out = _hip.EnvOut(fake, None, fake, fake, None)
acts = C.c_void_p(fake)
nan, inf = float("nan"), float("inf")


def both(c=None, prm=(4.0, 0.2, 2.0), st_=st, acts_=acts, out_=out, E=4, N=5, T=8, update=1):
    c = cfg() if c is None else c
    a = lib.mcn_env_step_sf(c, prm[0], prm[1], prm[2], st_, acts_, out_, None, E, N, update, None)
    b = lib.mcn_env_rollout_sf(c, prm[0], prm[1], prm[2], st_, acts_, T, out_, None, E, N, None)
    return a, b


# positive control, made only once the runtime itself confirms that it sees no device (never a launch on fake
# addresses): the acceptable call gets past validation and fails at the launch
count = C.c_int(-1)
err = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(count))
if err != 0 or count.value <= 0:
    assert both() == (_hip.MCN_ELAUNCH, _hip.MCN_ELAUNCH), both()
    assert both(prm=(0.0, 1e-300, 0.0)) == (_hip.MCN_ELAUNCH, _hip.MCN_ELAUNCH)      # the closed ends of the ranges
    print("POSITIVE_CONTROL_OK")
EINVAL = (_hip.MCN_EINVAL, _hip.MCN_EINVAL)
for policy in (_hip.HUMANS_ORCA, _hip.HUMANS_LINEAR, _hip.HUMANS_GIVEN, 4, -1):
    assert both(cfg(policy)) == EINVAL, policy
bad_params = {
    "range = 0": (4.0, 0.0, 2.0), "range = -0.0": (4.0, -0.0, 2.0), "range < 0": (4.0, -0.2, 2.0),
    "strength < 0": (-1e-9, 0.2, 2.0), "relaxation_rate < 0": (4.0, 0.2, -2.0),
    "strength nan": (nan, 0.2, 2.0), "range nan": (4.0, nan, 2.0), "relaxation_rate nan": (4.0, 0.2, nan),
    "strength inf": (inf, 0.2, 2.0), "range inf": (4.0, inf, 2.0), "relaxation_rate inf": (4.0, 0.2, inf),
    "strength -inf": (-inf, 0.2, 2.0),
}
for what, prm in bad_params.items():
    assert both(prm=prm) == EINVAL, what
# the pointer / size errors the ORCA entry points reject
assert both(acts_=None) == EINVAL
assert both(st_=_hip.EnvState()) == EINVAL
assert both(out_=_hip.EnvOut()) == EINVAL
assert both(E=0) == EINVAL and both(N=0) == EINVAL and both(N=_hip.MAX_HUMANS + 1) == EINVAL
assert lib.mcn_env_step_sf(None, 4.0, 0.2, 2.0, st, acts, out, None, 4, 5, 1, None) == _hip.MCN_EINVAL
assert lib.mcn_env_rollout_sf(None, 4.0, 0.2, 2.0, st, acts, 8, out, None, 4, 5, None) == _hip.MCN_EINVAL
assert both(T=0)[1] == _hip.MCN_EINVAL and both(T=-3)[1] == _hip.MCN_EINVAL
no_nobs = _hip.EnvOut(fake, None, None, None, None)
assert lib.mcn_env_step_sf(cfg(), 4.0, 0.2, 2.0, st, acts, no_nobs, None, 4, 5, 0, None) == _hip.MCN_EINVAL   # update = 0
r = _hip.Rollout()
r.state, r.fin_slots = fake, 1                                                 # state without a discount table
assert lib.mcn_env_step_sf(cfg(), 4.0, 0.2, 2.0, st, acts, out, r, 4, 5, 1, None) == _hip.MCN_EINVAL
assert lib.mcn_env_rollout_sf(cfg(), 4.0, 0.2, 2.0, st, acts, 8, out, r, 4, 5, None) == _hip.MCN_EINVAL
# the entry points without parameters keep rejecting the social-force value
assert lib.mcn_env_step(cfg(), st, acts, None, out, None, 4, 5, 1, None) == _hip.MCN_EINVAL
assert lib.mcn_env_step(cfg(), st, acts, acts, out, None, 4, 5, 1, None) == _hip.MCN_EINVAL
assert lib.mcn_env_rollout(cfg(), st, acts, 8, out, None, 4, 5, None) == _hip.MCN_EINVAL
assert lib.mcn_abi_version() == 5 == _hip.ABI_VERSION
assert "mcn_env_step_sf" in _hip.EXPORTED and "mcn_env_rollout_sf" in _hip.EXPORTED
print("SF_VALIDATION_OK")
"""


def test_entry_points_validate_on_host():
    """Each MCN_EINVAL case of mcn_env_step_sf / mcn_env_rollout_sf, in a fresh child process that sees NO device: the
    pointers are fakes, so a check that went missing would launch on them, which there fails with MCN_ELAUNCH instead of
    faulting a GPU that others share.  mcn_env_step / mcn_env_rollout still reject policy 3; the ABI version is 5."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1",
               PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _VALIDATION], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0 and "SF_VALIDATION_OK" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "POSITIVE_CONTROL_OK" in res.stdout, "the child process still saw a device: %s" % res.stdout[-500:]


def test_header_and_abi_unchanged_but_for_the_additions():
    import re
    hdr = open(os.path.join(ROOT, "include", "mcn.h")).read()
    assert re.search(r"MCN_HUMANS_SOCIALFORCE\s*=\s*3", hdr)
    assert int(re.search(r"#define\s+MCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 5
    from modelcrowdnav_amd import _hip
    assert _hip.lib.mcn_abi_version() == 5 and _hip.lib.mcn_sizeof(15) == -1
    assert _hip.lib.mcn_sizeof(0) == 7 * 8 + 2 * 4 + 6 * 4              # mcn_env_cfg did not grow


@pytest.mark.parametrize("n", (5, 10))
def test_default_parameters_sanity_run(n):
    """Circle-crossing test cases 0-29 with the crowd alone, dt 0.25, 100 steps (the time limit, 25 s), on the
    restatement: at least 95 % of the humans reach their goals, fewer than 0.5 % of the pair-steps overlap.  (The
    restatement gives 150 / 150 and 299 / 300 arrivals, 16 / 30 000 and 57 / 135 000 overlapping pair-steps.)"""
    from modelcrowdnav_amd.envs import scenarios as S
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    pol = policy_factory["socialforce"]()
    assert (pol.strength, pol.range, pol.relaxation_rate) == (A, B, K), "the shipped defaults are the ones this run is about"
    spec = S.ScenarioSpec(4.0, 10.0, 0.2, 0.3, 1.0, 0.3, False, False)
    pool = S.scenario_pool(spec, "test", list(range(30)), n, "circle_crossing")
    arrived = overlaps = pairs = 0
    for scen in pool:
        a, o, p, _ = R.sanity_run(scen, A, B, K, DT, 100)
        arrived, overlaps, pairs = arrived + a, overlaps + o, pairs + p
    assert pairs == 30 * 100 * n * (n - 1) // 2
    assert arrived >= 0.95 * 30 * n, (arrived, 30 * n)
    assert overlaps < 0.005 * pairs, (overlaps, pairs)


# ----------------------------------------------------------------- the inputs of the GPU batteries reach their events
def _ladder_events(params, Ns, update=True):
    """What the restatement plus the oracle's given-velocity step reach on the ladder batches, as
    tests/test_ladder_gpu.py::test_social_force_step_on_ladder_batches feeds them."""
    from oracle import cport
    from tests import kernel_paths as KP
    from tests import ladder_states as LS
    total = {}
    for N, visible, dd, count_hh in KP.ladder_configs(Ns, quad=False):
        st, ax, ay, _, names = LS.ladder_batch(N, visible, dd)
        want, _ = KP.sf_ladder_reference(N, visible, dd, params)
        cport.ladder_counts(reset=True)
        cport.env_step(LS.cfg(visible, dd, count_hh, policy=cport.HUMANS_GIVEN), st, ax, ay, update=update,
                       given_v=np.array(want))
        for k, v in cport.ladder_counts(reset=True).items():
            total[k] = total.get(k, 0) + v
    return total


def test_ladder_batches_reach_their_events_with_social_force_humans():
    """inert parameters (0, 0.2, 4): every step event, the first arrival at exactly one radius included (a human at rest
    gets w = e exactly); shipped parameters: every event but that one, which they never reach.  Also per crowd size of
    the rollout test (5 and 10 humans alone)."""
    from tests import kernel_paths as KP
    total = _ladder_events(KP.SF_INERT, KP.SF_COMPILED_NS + KP.SF_GENERIC_NS)
    assert all(total.get(k, 0) > 0 for k in KP.STEP_EVENTS), total
    total = _ladder_events(KP.SF_INERT, (1, 2, 5, 10))
    assert total["human_time_edge"] == 774, total["human_time_edge"]
    for N in KP.SF_COMPILED_NS:
        total = _ladder_events(KP.SF_INERT, (N,))
        assert all(total.get(k, 0) > 0 for k in KP.STEP_EVENTS), (N, total)
    total = _ladder_events(KP.SF_DEFAULT, KP.SF_COMPILED_NS + KP.SF_GENERIC_NS)
    assert all(total.get(k, 0) > 0 for k in KP.STEP_EVENTS if k != "human_time_edge"), total
    assert total.get("human_time_edge", 0) == 0, total
    total = _ladder_events(KP.SF_INERT, KP.SF_COMPILED_NS + KP.SF_GENERIC_NS, update=False)
    assert all(total.get(k, 0) > 0 for k in KP.STEP_EVENTS if k != "human_time_edge"), total


def test_inert_parameters_make_the_restatement_exact():
    """A = 0: the interaction terms are exactly 0 whatever exp returns, so the result does not depend on exp at all --
    replacing it by a function that is off by a factor leaves every bit."""
    from tests import kernel_paths as KP
    from tests import ladder_states as LS
    st = LS.ladder_batch(5, True, 0.25)[0]
    want, _ = KP.sf_ladder_reference(5, True, 0.25, KP.SF_INERT)
    real = R._exp
    try:
        R._exp = lambda x: 3.0 * real(x)
        other, _ = KP.sf_velocities(st, KP.SF_INERT, True)
    finally:
        R._exp = real
    assert other.tobytes() == np.array(want).tobytes()
    # a human at rest with k = 4 and dt = 0.25 gets w = e exactly
    w, _ = R.human_velocity((1.0, 2.0), (0.0, 0.0), (1.0, 2.5), 0.375, 0.5, [(1.25, 2.0, 0.3)], 0.0, 0.2, 4.0, 0.25)
    assert w == (0.0, 0.5)


def test_overlap_batches_overlap_well_inside_the_prefilter_margin():
    """tests/sf_edge_states.py overlap_batch: the oracle counts exactly the constructed pairs, none within 0.04 of
    touching (the float32 pre-filter's borderline band is 1e-3), every coordinate below 1024."""
    from oracle import cport
    from tests import sf_edge_states as SE
    for N in (2, 5, 10, 13):
        st, ax, ay, pairs = SE.overlap_batch(N)
        ref = cport.env_step(cport.default_cfg(count_hh=1, human_policy=cport.HUMANS_GIVEN), st.copy(), ax, ay,
                             update=False, given_v=np.zeros((st.E, N, 2)))
        assert (ref["hh_count"] == pairs).all() and (pairs > 0).all()
        g = SE.pair_gaps(st)[:, np.triu_indices(N, 1)[0], np.triu_indices(N, 1)[1]]
        assert (np.abs(g) > 0.04).all() and (g < -0.04).any()
        assert max(np.abs(st.hpx).max(), np.abs(st.hpy).max()) < 1024


# events every (N, visible) batch of the edge battery must hold, by the robot's visibility and the crowd size
_EDGE_ALWAYS = ("goal_tie", "goal_ulp_below", "goal_ulp_above", "on_goal", "vpref_zero", "neg_zero_e", "neg_zero_v",
                "neg_zero_w", "w_tie", "w_ulp_above", "nonfinite_self", "nonfinite_w", "clipped")
_EDGE_WITH_OTHERS = ("exp_subnormal", "exp_underflow", "exp_overflow", "nonfinite_other")


@pytest.mark.parametrize("N", (1, 2, 5, 10, 13))
def test_edge_batches_reach_their_events(N):
    """tests/sf_edge_states.py: what tests/test_social_force_edges_gpu.py claims of its inputs, from an instrumented walk
    through the definition over all parameter sets (N = 32 is built by the same code and left to the GPU test: its
    walk alone takes several seconds of host Python)."""
    from tests import kernel_paths as KP
    from tests import sf_edge_states as SE
    for visible in (0, 1):
        st, ax, ay, names = SE.edge_batch(N, visible)
        assert st.E == 11 * SE.BLOCK + SE.PAD and all(st.E % (64 // n) for n in SE.NS if n > 1)
        total, per = {}, {}
        for group, params in SE.PARAMS.items():
            ev = SE.trace(st, params, visible)
            per[group] = {k: int(v.sum()) for k, v in ev.items()}
            for k, v in per[group].items():
                total[k] = total.get(k, 0) + v
        need = list(_EDGE_ALWAYS)
        if N >= 2 or visible:
            need += _EDGE_WITH_OTHERS
        if N >= 2:
            need += ["coincident_human", "all_coincident"]
        if visible:
            need += ["coincident_robot"]
        need += ["no_term"] if (N == 1 and not visible) else []
        need += ["robot_only"] if (N == 1 and visible) else []
        missing = [k for k in need if total.get(k, 0) == 0]
        assert not missing, (N, visible, missing, total)
        # the exact |w| == v_pref tie and -0.0 results come from the set with A = 0 and k = 0; overflow from B = 2^-10
        assert per["still"]["w_tie"] > 0 and per["still"]["w_ulp_above"] > 0 and per["still"]["neg_zero_w"] > 0
        if N >= 2 or visible:
            assert per["B-small"]["exp_overflow"] > 0 and per["B-tiny"]["exp_overflow"] > 0
            assert per["default"]["exp_subnormal"] > 0 and per["default"]["exp_underflow"] > 0
        # the unseen robot's twins differ in nothing but the robot's position
        tw = [e for e, n in enumerate(names) if n == "nonfinite-robot"]
        assert len(tw) == 16 and not np.isfinite(st.rpx[tw[8:]] + st.rpy[tw[8:]]).any()
        assert (st.hpx[tw[8:]] == st.hpx[tw[:8]]).all() and (st.hvx[tw[8:]] == st.hvx[tw[:8]]).all()


def test_restatement_overflow_is_inf_not_an_exception():
    """exp beyond its range: m = inf; along an axis inf * 0 gives NaN in the other component, off the axes the clip's
    inf / inf gives NaN in both."""
    w, _ = R.human_velocity((0.0, 0.0), (0.0, 0.0), (1.0, 0.0), 0.375, 1.0, [(-1 / 32, 0.0, 0.375)], 4.0, 2.0 ** -10, 2.0, DT)
    assert w[0] == math.inf and math.isnan(w[1])
    w, _ = R.human_velocity((0.0, 0.0), (0.0, 0.0), (1.0, 0.0), 0.375, 1.0, [(-1 / 32, -1 / 32, 0.375)], 4.0, 2.0 ** -10, 2.0, DT)
    assert math.isnan(w[0]) and math.isnan(w[1])
    w, _ = R.human_velocity((0.0, 0.0), (0.0, 0.0), (1.0, 0.0), 0.375, 1.0, [(-1 / 32, 0.0, 0.375)], 0.0, 2.0 ** -10, 2.0, DT)
    assert math.isnan(w[0]) and math.isnan(w[1])              # 0 * inf
    assert R._exp(-math.inf) == 0.0 and math.isnan(R._exp(math.nan)) and R._exp(710.0) == math.inf
