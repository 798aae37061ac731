"""GPU: the launchers obey the plan.  A dozen rows of tests/test_env_dispatch_cpu.py's table, one per kernel family and
rollout form, are launched once through VecCrowdSim; mcn_last_dispatch() / mcn_last_rollout_form() must name what the
table plans for the row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests.rollout_harness import need_gpu  # noqa: E402
from tests.test_env_dispatch_cpu import TABLE  # noqa: E402

WORDS = dict(T=0, policy=0, E=1, N=5, vis=0, uni=0, maxn=10, update=1, hh=0, queue=0, times=0, hact=0, disc=0)
TUNING = dict(fg=("force_generic", 0), qmax=("quad_max_envs", -1), qsplit=("quad_split", -1),
              rfused=("rollout_fused", -1), rsplit=("rollout_split", -1), block=("step_block", -1),
              pstream=("pair_stream", -1), defer=("lp3_defer", -1))

ROWS = ["E=4200", "E=8401", "N=10 queue=1 E=98299", "policy=2 E=49152", "policy=2 E=49153",
        "T=20 E=1016", "T=20 E=1017", "T=20 E=4609", "T=20 uni=1 E=57", "T=20 rfused=1 rsplit=2 N=4 E=4096",
        "T=20 E=42001", "T=20 N=10 E=18432", "T=20 N=10 E=18433", "T=20 policy=3 E=49152", "T=20 policy=3 E=49153"]


def launch_row(problem, tuning):
    """Builds the env a row of the table describes (tests/env_dispatch_probe.cpp: its words), sets the row's tuning --
    every field, so that MCN_* overrides of the run do not reach it -- and launches it once.  Returns the env."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.envs import scenarios as S
    w = dict(WORDS, **{k: d for k, (_, d) in TUNING.items()})
    for word in problem.split():
        k, v = word.split("=")
        assert k in w, word
        w[k] = int(v)
    E, N, T = w["E"], w["N"], w["T"]
    over = {"humans.policy": "socialforce"} if w["policy"] == 3 else {}
    env = H.make_vec_env(E, N, robot_visible=bool(w["vis"]), kinematics="unicycle" if w["uni"] else "holonomic", **over)
    env._orca.max_neighbors = w["maxn"]
    env.count_hh, env.track_human_times, env.export_human_actions = bool(w["hh"]), bool(w["times"]), bool(w["hact"])
    if w["policy"] == 1:
        env.human_policy_name = "linear"
    pool = S.scenario_pool(env.spec(), "test", range(64), N, "circle_crossing")
    env.load_scenarios(pool[np.arange(E) % 64])
    if w["queue"]:
        # (no queue exists for crowds outside the deferred path's 2 .. 10 humans: there the plan must not look at it)
        assert env.lp3_queue is not None or not 2 <= N <= 10
        if env.lp3_queue is None:
            env.lp3_queue = torch.zeros(64, dtype=torch.uint8, device=env.device)
            env._out.lp3_queue = env._out_lean.lp3_queue = _hip.ptr(env.lp3_queue)
    else:
        env._out.lp3_queue = env._out_lean.lp3_queue = None
    if w["disc"]:
        env.time_limit = (w["disc"] - 2) * env.time_step          # attach_rollout: time_limit / time_step + 2 entries
        env.attach_rollout(gamma=0.9)
        assert env._roll.disc_len == w["disc"]
    tuning(**{name: w[k] for k, (name, _) in TUNING.items()})
    acts = torch.zeros(max(T, 1), E, 2, dtype=torch.float64, device=env.device)
    if T > 0:
        env.rollout(acts)
    else:
        given = torch.zeros(E, N, 2, dtype=torch.float64, device=env.device) if w["policy"] == 2 else None
        env.step(acts[0], update=bool(w["update"]), given_v=given)
    torch.cuda.synchronize()
    return env


@pytest.mark.parametrize("problem", ROWS)
def test_launchers_obey_the_plan(problem, tuning):
    from modelcrowdnav_amd import _hip
    want = dict(TABLE)[problem]
    launch_row(problem, tuning)
    assert _hip.last_dispatch() == want[0], (problem, _hip.last_dispatch())
    if "T=" in problem:
        assert _hip.last_rollout_form() == want[1], (problem, _hip.last_rollout_form())


def test_rows_cover_every_family_and_form():
    by = dict(TABLE)
    assert {by[p][0] for p in ROWS} == {"env_step_quad_kernel", "env_pair_kernel", "env_step_kernel",
                                        "env_rollout_quad_kernel", "env_step_loop_kernel", "env_step_loop_sf_kernel"}
    assert {by[p][1] for p in ROWS} == {-1, 0, 1, 2}
    assert any(by[p][5] for p in ROWS)                          # a deferred step: two kernels


def test_closed_loop_names_its_kernel_and_leaves_the_form(tuning):
    """mcn_env_rollout_orca has one path; like mcn_env_rollout_sf it leaves mcn_last_rollout_form() untouched."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    env = launch_row("T=2 rfused=1 rsplit=1 E=64", tuning)
    assert (_hip.last_dispatch(), _hip.last_rollout_form()) == ("env_rollout_quad_kernel", 1)
    env.rollout_orca(env._orca, 2)
    torch.cuda.synchronize()
    assert (_hip.last_dispatch(), _hip.last_rollout_form()) == ("env_step_loop_orca_kernel", 1)
    sf = launch_row("T=2 policy=3 E=64", tuning)
    assert (_hip.last_dispatch(), _hip.last_rollout_form()) == ("env_step_loop_sf_kernel", 1)
    del env, sf
