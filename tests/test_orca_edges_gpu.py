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
from tests.kernel_paths import (QUAD_EVENTS, ROLLOUT_PATHS, STEP_KERNELS, WG4_EDGE_CUTS, edge_configs,  # noqa: E402
                                forced_form, rolled_wg4_battery, select_step_kernel)
from tests.rollout_harness import assert_same_bytes, launch, need_gpu, snapshot  # noqa: E402

ALL_EVENTS = cport.EDGE_NAMES


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
    torch = need_gpu()
    quad = kernel.startswith("quad")
    select_step_kernel(kernel, tuning)
    total = dict.fromkeys(ALL_EVENTS, 0)
    Ns = range(1, 6) if quad else range(1, 11)
    for N, visible, variant in edge_configs(Ns, quad):
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


_STEP_KEYS = ("reward", "done", "info", "dmin", "hh_count", "human_act")


def _assert_step_equals_oracle(env, ref, ref_st, names, what, keys=_STEP_KEYS, fields=H.STATE_FIELDS):
    for k in keys:
        bad = H.bit_mismatch(getattr(env, k).cpu().numpy(), ref[k])
        assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
    H.assert_state_equal(H.download(env), ref_st, fields=fields, what=what)


@pytest.mark.parametrize("path", sorted(ROLLOUT_PATHS))
def test_rollout_on_edge_batches_equals_single_steps_and_oracle(path, tuning):
    """mcn_env_rollout over 24 steps in two launches (10 + 14; the four-wavefront form 9 + 1 + 14) == 24 mcn_env_step
    calls, every byte; without a scenario pool also == the oracle's 24-step trajectory, bitwise; with one (episodes that
    end restart from it) the launch and the single steps still agree byte for byte.  Every launch of a quad path asserts
    the form that went out.  The four-wavefront form has one shape only, so it runs every ORCA variant that shape takes,
    the parallel_same_lp3 supplement with the default one, and a one-step launch of its own against the oracle's first
    step."""
    torch = need_gpu()
    from modelcrowdnav_amd.envs import scenarios as S
    Ns, quad, tu = ROLLOUT_PATHS[path]
    form = forced_form(path)
    wg4 = form == 2
    tuning(**tu)
    T = 24
    cuts = WG4_EDGE_CUTS if wg4 else (0, 10, T)
    total = dict.fromkeys(ALL_EVENTS, 0)
    for N in Ns:
        # the default ORCA parameters and one of the others, in turn (at N = 5 that one is max_neighbors = 3, which no
        # quad path takes)
        variants = ES.WG4_VARIANTS if wg4 else (ES.ORCA_VARIANTS[0], ES.ORCA_VARIANTS[1 + N % 4])
        for n_, visible, variant in edge_configs([N], quad, variants):
            st, ax0, ay0, names = ES.edge_batch(N, visible, variant)
            if wg4 and not variant:
                st, ax0, ay0, names = ES.with_supplement((st, ax0, ay0, names))
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
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    launch(a, acts_d[lo:hi], form)
                for t in range(T):
                    b.step(acts_d[t])
                torch.cuda.synchronize()
                assert_same_bytes(snapshot(a), snapshot(b), (what, with_pool))
                if with_pool:
                    continue
                ref_st = st.copy()
                cfg = H.oracle_cfg_for(a)
                cport.edge_counts(reset=True)
                for t in range(T):
                    ref = cport.env_step(cfg, ref_st, ax[t], ay[t], update=True)
                    if t == 0:
                        ref0, ref_st0 = ref, ref_st.copy()
                for k, v in cport.edge_counts(reset=True).items():
                    total[k] += v
                _assert_step_equals_oracle(a, ref, ref_st, names, what)
                if wg4:
                    c = _env(N, visible, variant, E)
                    H.upload(c, st)
                    launch(c, acts_d[:1], form)
                    torch.cuda.synchronize()
                    _assert_step_equals_oracle(c, ref0, ref_st0, names, what + " first step")
    _assert_reached(total, QUAD_EVENTS if quad else ALL_EVENTS, path)


def test_wg4_rollout_on_rolled_edge_batch(tuning):
    """rolled_wg4_battery on the default-variant edge batch of 5 humans plus the parallel_same_lp3 supplement (E = 637,
    24 steps as 9 + 1 + 14); the oracle replays the unrolled batch once and its outputs are rolled."""
    N, T, variant = 5, 24, ES.ORCA_VARIANTS[0]
    tuning(rollout_fused=1, rollout_split=2)
    st, ax0, ay0, names = ES.with_supplement(ES.edge_batch(N, False, variant))
    E = st.E
    rng = np.random.RandomState(N * 2)
    ax = np.concatenate([ax0[None], rng.randint(-16, 17, (T - 1, E)) / 16.0])
    ay = np.concatenate([ay0[None], rng.randint(-16, 17, (T - 1, E)) / 16.0])
    ref_st = st.copy()
    cfg = H.oracle_cfg_for(_env(N, False, variant, E))
    cport.edge_counts(reset=True)
    for t in range(T):
        ref = cport.env_step(cfg, ref_st, ax[t], ay[t], update=True)
        if t == 0:
            ref0, ref_st0, first = ref, ref_st.copy(), cport.edge_counts(reset=False)
    total = cport.edge_counts(reset=True)
    # what the default variant reaches at N = 5 (tests/test_oracle_edges.py holds the counts); the one-step launches of
    # all eight rolls see every one of these but the events of later steps
    events = [k for k in QUAD_EVENTS if k != "parallel_opposite_lp3"]
    _assert_reached(first, events, "rolled edge batch, first step")
    _assert_reached(total, events, "rolled edge batch")

    def build():
        return _env(N, False, variant, E)

    def rolled_ref(r, perm):
        return {k: r[k][perm] for k in _STEP_KEYS}

    def check_first(env, perm, rolled, what):
        _assert_step_equals_oracle(env, rolled_ref(ref0, perm), ES.take(ref_st0, perm), rolled, what)

    def check_last(env, perm, rolled, what):
        _assert_step_equals_oracle(env, rolled_ref(ref, perm), ES.take(ref_st, perm), rolled, what)

    rolled_wg4_battery(build, ES.take, st, np.stack([ax, ay], -1), names, WG4_EDGE_CUTS, check_first, check_last,
                       "rolled edge batch")


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
