"""Every ORCA kernel path on exact ties, exact zeros and NaN half-planes (tests/edge_states.py), bit for bit.

Random float states almost never produce a line tangent to the speed disc, two neighbours at the same distance, a
neighbour at exactly neighborDist or a NaN half-plane inside the 3-D LP; the dyadic edge batches produce all of them
(tests/test_oracle_edges.py::test_edge_batches_reach_every_counter).  Here each mcn_env_step decomposition, each
mcn_env_rollout path and mcn_orca_batch run on them against the C oracle, and each test asserts that the oracle's
replay of its own inputs reached the events it is meant to cover.  Comparisons are bitwise (tests/helpers.py
bit_mismatch): -0.0 against +0.0 fails, NaN matches NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import edge_states as ES  # noqa: E402
from tests import helpers as H  # noqa: E402

STEP_KERNELS = ["auto", "lane-per-human", "lane-per-human-256", "deferred-lp3", "deferred-lp3-256", "run-time-N",
                "run-time-N-256", "quad", "quad-split"]
# what the quad kernels' inputs must reach (at most 4 neighbours and maxNeighbors >= 4: no cut of the neighbour list)
QUAD_EVENTS = ("disc_zero_lp2", "disc_zero_lp3", "dist_tie", "nonfinite_line", "nonfinite_line_in_lp3",
               "w_zero_collision", "parallel_lp1", "parallel_same_lp3", "parallel_opposite_lp3", "range_edge",
               "leg_det_zero", "pref_on_disc", "outside_fast_range")
ALL_EVENTS = cport.EDGE_NAMES


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _select_step_kernel(kernel, tuning):
    """As tests/test_env_step_gpu.py::test_step_matches_oracle_bitexact pins each decomposition."""
    if kernel.startswith("lane-per-human"):
        tuning(quad_max_envs=0, lp3_defer=0)
    elif kernel.startswith("deferred-lp3"):
        tuning(quad_max_envs=0, lp3_defer=1)
    elif kernel.startswith("run-time-N"):
        tuning(quad_max_envs=0, force_generic=1)
    elif kernel.startswith("quad"):
        tuning(quad_max_envs=1 << 30, quad_split=1 if kernel == "quad-split" else 0)
    if kernel.endswith("-256"):
        tuning(step_block=256)


def _configs(Ns, quad, variants=ES.ORCA_VARIANTS):
    """(N, visible, variant) triples; the quad kernels take at most 4 candidate neighbours and 4 line slots."""
    for N in Ns:
        for visible in (False, True):
            if quad and N - 1 + visible > 4:
                continue
            for variant in variants:
                if quad and ES.orca_cfg(variant)["max_neighbors"] < 4:
                    continue
                yield N, visible, variant


def _env(N, visible, variant, E):
    env = H.make_vec_env(E, N, robot_visible=visible)
    for k, v in ES.orca_cfg(variant).items():
        setattr(env._orca, k, v)
    return env


def _assert_reached(total, events, what):
    missing = [k for k in events if total.get(k, 0) == 0]
    assert not missing, "%s: the inputs never reached %s (%s)" % (what, missing, total)


def _where(names, bad):
    return sorted({names[int(i[0])] for i in bad})[:6]


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("kernel", STEP_KERNELS)
def test_step_on_edge_batches_matches_oracle_bitwise(kernel, update, tuning):
    torch = _torch()
    quad = kernel.startswith("quad")
    _select_step_kernel(kernel, tuning)
    total = dict.fromkeys(ALL_EVENTS, 0)
    Ns = range(1, 6) if quad else range(1, 11)
    for N, visible, variant in _configs(Ns, quad):
        st, ax, ay, names = ES.edge_batch(N, visible, variant)
        env = _env(N, visible, variant, st.E)
        H.upload(env, st)
        ob, reward, done, info = env.step(torch.from_numpy(np.stack([ax, ay], -1)).to(env.device), update=bool(update))
        torch.cuda.synchronize()
        got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy(), info=info.cpu().numpy(),
                   dmin=env.dmin.cpu().numpy(), hh_count=env.hh_count.cpu().numpy(),
                   human_act=env.human_act.cpu().numpy())
        if not update:
            got.update(nobs_px=ob.pos[..., 0].cpu().numpy(), nobs_py=ob.pos[..., 1].cpu().numpy(),
                       nobs_vx=ob.vel[..., 0].cpu().numpy(), nobs_vy=ob.vel[..., 1].cpu().numpy())
        ref_st = st.copy()
        cport.edge_counts(reset=True)
        ref = cport.env_step(H.oracle_cfg_for(env), ref_st, ax, ay, update=bool(update))
        for k, v in cport.edge_counts(reset=True).items():
            total[k] += v
        what = "%s N=%d visible=%d %s" % (kernel, N, visible, variant)
        assert set(got) == set(ref)
        for k in ref:
            bad = H.bit_mismatch(got[k], ref[k])
            assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
        H.assert_state_equal(H.download(env), ref_st if update else st, what=what)
    _assert_reached(total, QUAD_EVENTS if quad else ALL_EVENTS, kernel)


def _snapshot(env):
    c = lambda t: t.detach().cpu().numpy().copy()
    snap = {k: c(getattr(env, k)) for k in ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal",
                                            "rtheta", "gtime", "human_times", "step_rec", "human_act")}
    if env._roll is not None:
        snap.update({"roll_" + k: c(v) for k, v in env.rollout_buffers.items()
                     if k in ("state", "fin_return", "fin_time", "fin_info")})
    return snap


ROLLOUT_PATHS = {
    # name: (human counts, quad layout, tuning)
    "quad-rollout": (range(1, 6), True, dict(rollout_fused=1, rollout_split=0)),
    "quad-rollout-split": (range(1, 6), True, dict(rollout_fused=1, rollout_split=1)),
    "step-loop": (range(6, 11), False, dict(rollout_fused=1, lp3_defer=0)),
    "lp3-defer": (range(2, 11), False, dict(rollout_fused=1, lp3_defer=1)),
    "unfused": (range(1, 11), False, dict(rollout_fused=0)),
}


@pytest.mark.parametrize("path", sorted(ROLLOUT_PATHS))
def test_rollout_on_edge_batches_equals_single_steps_and_oracle(path, tuning):
    """mcn_env_rollout over 24 steps in two launches (10 + 14) == 24 mcn_env_step calls, every byte; without a scenario
    pool also == the oracle's 24-step trajectory, bitwise; with one (episodes that end restart from it) the launch and
    the single steps still agree byte for byte."""
    torch = _torch()
    from modelcrowdnav_amd.envs import scenarios as S
    Ns, quad, tu = ROLLOUT_PATHS[path]
    tuning(**tu)
    T = 24
    total = dict.fromkeys(ALL_EVENTS, 0)
    for N in Ns:
        # the default ORCA parameters and one of the others, in turn
        variants = (ES.ORCA_VARIANTS[0], ES.ORCA_VARIANTS[1 + N % 4])
        for n_, visible, variant in _configs([N], quad, variants):
            st, ax0, ay0, names = ES.edge_batch(N, visible, variant)
            E = st.E
            rng = np.random.RandomState(N * 2 + visible)
            ax = np.concatenate([ax0[None], rng.randint(-16, 17, (T - 1, E)) / 16.0])
            ay = np.concatenate([ay0[None], rng.randint(-16, 17, (T - 1, E)) / 16.0])
            acts = torch.from_numpy(np.stack([ax, ay], -1))
            what = "%s N=%d visible=%d %s" % (path, N, visible, variant)
            for with_pool in (False, True):
                a, b = _env(N, visible, variant, E), _env(N, visible, variant, E)
                for env in (a, b):
                    H.upload(env, st)
                    if with_pool:
                        pool = S.scenario_pool(env.spec(), "test", range(16), N, "circle_crossing")
                        env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=np.arange(E) % 16,
                                           fin_slots=2)
                acts_d = acts.to(a.device)
                a.rollout(acts_d[:10]); a.rollout(acts_d[10:])
                for t in range(T):
                    b.step(acts_d[t])
                torch.cuda.synchronize()
                sa, sb = _snapshot(a), _snapshot(b)
                for k in sa:
                    assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), (what, with_pool, k)
                if with_pool:
                    continue
                ref_st = st.copy()
                cfg = H.oracle_cfg_for(a)
                cport.edge_counts(reset=True)
                for t in range(T):
                    ref = cport.env_step(cfg, ref_st, ax[t], ay[t], update=True)
                for k, v in cport.edge_counts(reset=True).items():
                    total[k] += v
                H.assert_state_equal(H.download(a), ref_st, what=what)
                for k, v in (("reward", a.reward), ("done", a.done), ("info", a.info), ("dmin", a.dmin),
                             ("hh_count", a.hh_count), ("human_act", a.human_act)):
                    bad = H.bit_mismatch(v.cpu().numpy(), ref[k])
                    assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
    _assert_reached(total, QUAD_EVENTS if quad else ALL_EVENTS, path)


def _lattice_scene(rng, n, spacing, max_neighbors):
    """n agents on a lattice (1/8 grid), a coincident pair with equal velocities, one agent at exactly neighborDist
    (10) from agent 0 and, past maxNeighbors, agents at equal distances from agent 0 so that the cut falls on a tie."""
    side = int(np.ceil(np.sqrt(n))) + 1
    cells = rng.choice(side * side, n, replace=False)
    pos = np.stack([cells % side, cells // side], -1) * spacing
    vel = rng.randint(-16, 17, (n, 2)) / 16.0
    pos[1], vel[1] = pos[0], vel[0]                                       # coincident, same velocity: 0/0
    pos[2] = pos[0] + (6.0, 8.0)                                          # exactly neighborDist
    ring = np.array([(5, 0), (0, 5), (-5, 0), (0, -5), (3, 4), (-4, 3), (-3, -4), (4, -3)]) * 0.25
    for i, k in enumerate(range(3, min(n, 3 + max_neighbors + 2))):    # ties across the cut of agent 0's list
        pos[k] = pos[0] + ring[i % len(ring)]
    goal = pos[::-1].copy()
    return pos, vel, goal


@pytest.mark.parametrize("n,spacing", [(6, 0.75), (12, 0.5), (16, 0.75), (24, 0.5)])
def test_orca_batch_on_lattice_scenes_matches_oracle_simulator(n, spacing):
    """modelcrowdnav_amd.rvo2.PyRVOSimulator (doStep = mcn_orca_batch) against refshim's oracle simulator on lattice
    scenes: more agents than maxNeighbors (4) with a tie at the cut, an agent at exactly neighborDist, coincident agents
    (a NaN half-plane).  Velocities and positions after every doStep, bitwise."""
    from modelcrowdnav_amd import rvo2
    from tests.golden_tools.refshim import _PyRVOSimulator
    rng = np.random.RandomState(n)
    mn = 4
    pos, vel, goal = _lattice_scene(rng, n, spacing, mn)
    a, b = rvo2.PyRVOSimulator(0.25, 10, mn, 5, 5, 0.3125, 1), _PyRVOSimulator(0.25, 10, mn, 5, 5, 0.3125, 1)
    for sim in (a, b):
        for i in range(n):
            assert sim.addAgent(tuple(pos[i]), 10, mn, 5, 5, 0.3125, 1.0, tuple(vel[i])) == i
    for step in range(6):
        for sim in (a, b):
            for i in range(n):
                sim.setAgentPrefVelocity(i, tuple(np.clip(goal[i] - np.array(sim.getAgentPosition(i)), -1, 1) / 2))
            sim.doStep()
        for i in range(n):
            H.assert_bits_equal(np.array(a.getAgentVelocity(i)), np.array(b.getAgentVelocity(i)), "step %d v%d" % (step, i))
            H.assert_bits_equal(np.array(a.getAgentPosition(i)), np.array(b.getAgentPosition(i)), "step %d p%d" % (step, i))
    # the scene reaches what it is made for (agent 0's first solve, replayed)
    cport.edge_counts(reset=True)
    o = [j for j in range(n) if j != 0]
    cport.orca_agent(pos[0], vel[0], 0.3125, 1.0, np.clip(goal[0] - pos[0], -1, 1) / 2, pos[o], vel[o],
                     np.full(n - 1, 0.3125), max_neighbors=mn)
    c = cport.edge_counts(reset=True)
    assert c["range_edge"] and c["dist_tie"] and c["nonfinite_line"], c
    if n > 3 + mn:
        assert c["tie_at_cut"], c
