"""The float64 half of every step kernel on exact boundaries (tests/ladder_states.py), bit for bit against the C oracle:
the swept test (touching, a point segment, u exactly 0 or 1, tied humans), the overlap count at and within 1e-6 / 1e-3 of
touching (float32-rounded positions on the other side of touching included), the goal test at and within 1e-6 of the
radius, the timeout rung at and one ulp below time_limit - 1, the rung precedences, first arrivals at exactly one radius,
headings with a zero fmod remainder, and the look-ahead reward of mcn_sarl_predict, mcn_lstm_rl_predict and
mcn_cadrl_predict.  The social-force instantiations (mcn_env_step_sf / mcn_env_rollout_sf) run the same batches: their
velocity against tests/social_force_ref.py, everything after it against the oracle's given-velocity step.

Each test replays its own inputs through the oracle and asserts that they reached the ladder events it claims
(cport.ladder_counts); failures name the block of the first differing envs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import ladder_states as LS  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests.kernel_paths import (ROLLOUT_PATHS, SF_COMPILED_NS, SF_DEFAULT, SF_GENERIC_NS, SF_INERT, SF_TOL,  # noqa: E402
                                STEP_EVENTS, STEP_KERNELS, UNICYCLE_EVENTS, forced_form, ladder_configs,
                                rolled_wg4_battery, select_step_kernel, sf_ladder_reference, sf_oracle_step,
                                sf_step_forms)
from tests.rollout_harness import assert_same_bytes, launch, need_gpu, snapshot  # noqa: E402

LA_EVENTS = ("la_touch", "la_danger_edge", "la_reach_edge", "la_collision_after_min")
GENERIC_NS = (13, 32)          # only the run-time-N kernels (and the dispatcher) take more than 10 humans


def _env(N, visible, dd, count_hh, E, unicycle=False):
    env = H.make_vec_env(E, N, robot_visible=visible, kinematics="unicycle" if unicycle else "holonomic")
    env.discomfort_dist = dd
    env.count_hh = count_hh
    return env


def _where(names, bad):
    return sorted({names[int(i[0])] for i in bad})[:6]


def _assert_reached(total, events, what):
    missing = [k for k in events if total.get(k, 0) == 0]
    assert not missing, "%s: the inputs never reached %s (%s)" % (what, missing, total)


def _add(total):
    for k, v in cport.ladder_counts(reset=True).items():
        total[k] = total.get(k, 0) + v


def _step_and_compare(env, st, ax, ay, names, update, what, policy=cport.HUMANS_ORCA, given=None, total=None,
                      fields=H.STATE_FIELDS):
    torch = need_gpu()
    H.upload(env, st)
    gv = None if given is None else torch.from_numpy(np.ascontiguousarray(given)).to(env.device)
    ob, reward, done, info = env.step(torch.from_numpy(np.stack([ax, ay], -1)).to(env.device), update=bool(update),
                                      given_v=gv)
    torch.cuda.synchronize()
    got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy(), info=info.cpu().numpy(),
               dmin=env.dmin.cpu().numpy(), hh_count=env.hh_count.cpu().numpy())
    if env.export_human_actions:
        got["human_act"] = env.human_act.cpu().numpy()
    if not update:
        got.update(nobs_px=ob.pos[..., 0].cpu().numpy(), nobs_py=ob.pos[..., 1].cpu().numpy(),
                   nobs_vx=ob.vel[..., 0].cpu().numpy(), nobs_vy=ob.vel[..., 1].cpu().numpy())
    ref_st = st.copy()
    cport.ladder_counts(reset=True)
    ref = cport.env_step(H.oracle_cfg_for(env, policy), ref_st, ax, ay, update=bool(update), given_v=given)
    if total is not None:
        _add(total)
    for k in got:
        bad = H.bit_mismatch(got[k], ref[k])
        assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
    if fields:
        H.assert_state_equal(H.download(env), ref_st if update else st, fields=fields, what=what)
    return got, ref, ref_st


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("kernel", STEP_KERNELS)
def test_step_on_ladder_batches_matches_oracle_bitwise(kernel, update, tuning):
    """Reward, done, info, dmin, hh_count, human actions, the next observation or the state, first-arrival times."""
    quad = kernel.startswith("quad")
    select_step_kernel(kernel, tuning)
    total = {}
    Ns = list(range(1, 6)) if quad else list(range(1, 11))
    if kernel in ("auto", "run-time-N"):
        Ns += list(GENERIC_NS)
    for N, visible, dd, count_hh in ladder_configs(Ns, quad):
        st, ax, ay, _, names = LS.ladder_batch(N, visible, dd)
        env = _env(N, visible, dd, count_hh, st.E)
        _step_and_compare(env, st, ax, ay, names, update, "%s N=%d visible=%d dd=%g count_hh=%d" % (
            kernel, N, visible, dd, count_hh), total=total)
    _assert_reached(total, STEP_EVENTS if update else [k for k in STEP_EVENTS if k != "human_time_edge"], kernel)


@pytest.mark.parametrize("kernel", ["auto", "lane-per-human", "run-time-N", "quad"])
def test_unicycle_step_on_ladder_batches(kernel, tuning):
    """(v, r) robots: headings whose remainder is zero (either sign) or negative; rtheta and the ladder bitwise.  Where
    rtheta + r is +-0 cos and sin are exact, so everything is bitwise; elsewhere the robot's position and velocity come
    from device trig and are held to 1e-12 (as tests/test_env_step_gpu.py::test_unicycle_robot_matches_oracle_...)."""
    torch = need_gpu()
    quad = kernel.startswith("quad")
    select_step_kernel(kernel, tuning)
    total = {}
    for N, visible, dd, count_hh in ladder_configs(range(1, 6) if quad else (1, 3, 5, 8, 10), quad):
        st, ax, ay, _, names = LS.ladder_batch(N, visible, dd, unicycle=True)
        env = _env(N, visible, dd, count_hh, st.E, unicycle=True)
        what = "%s unicycle N=%d visible=%d dd=%g" % (kernel, N, visible, dd)
        trig = ["rpx", "rpy", "rvx", "rvy"]
        _, _, ref_st = _step_and_compare(env, st, ax, ay, names, 1, what, total=total,
                                         fields=[f for f in H.STATE_FIELDS if f not in trig] + ["rtheta"])
        got = H.download(env)
        exact = np.array([(st.rtheta[e] + ay[e]) == 0 for e in range(st.E)])
        assert exact.sum() > st.E // 2
        for k in trig:
            H.assert_bits_equal(getattr(got, k)[exact], getattr(ref_st, k)[exact], what + " " + k)
            np.testing.assert_allclose(getattr(got, k), getattr(ref_st, k), rtol=0, atol=1e-12, err_msg=what + k)
        # Python's % gives +0.0 for a zero remainder: the new heading and the velocity's y component are +0.0
        z = np.array([(st.rtheta[e] + ay[e]) % (2 * np.pi) == 0 for e in range(st.E)])
        assert z.any() and not np.signbit(got.rtheta[z]).any() and not np.signbit(got.rvy[z & exact]).any()
        del env
        torch.cuda.empty_cache()
    _assert_reached(total, UNICYCLE_EVENTS, kernel + " unicycle")


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_given_velocity_paths_on_ladder_batches(stream, tuning):
    """ModelCrowdSim.step's given-velocity step: the streaming kernel (env_pair.hip, pair_stream 1 / 2: N in {5, 10},
    no overlap count, no first arrivals, no exported actions) and env_step_kernel<GIVEN> (pair_stream 0, and the
    configurations the streaming kernel does not take); the ladder fields and the state bitwise."""
    from modelcrowdnav_amd import _hip
    total = {}
    for N in (1, 2, 5, 10):
        for visible in (False, True):
            for dd in LS.DISCOMFORT:
                st, ax, ay, gv, names = LS.ladder_batch(N, visible, dd)
                lean = N in (5, 10)
                env = _env(N, visible, dd, not lean, st.E)
                if lean:
                    env.track_human_times = False
                    env.export_human_actions = False
                tuning(pair_stream=stream)
                what = "given pair_stream=%d N=%d visible=%d dd=%g" % (stream, N, visible, dd)
                _step_and_compare(env, st, ax, ay, names, 1, what, cport.HUMANS_GIVEN, gv, total,
                                  fields=[f for f in H.STATE_FIELDS if not (lean and f == "human_times")])
                if lean and stream:
                    assert "pair" in _hip.last_dispatch(), (what, _hip.last_dispatch())
    _assert_reached(total, [k for k in STEP_EVENTS if not k.startswith("hh")], "given pair_stream=%d" % stream)


def test_linear_humans_on_ladder_batches():
    """Linear humans (device atan2 / cos / sin): the ladder fields bitwise (they do not depend on the humans' new
    velocities), the new positions within 1e-12."""
    torch = need_gpu()
    total = {}
    for N in (1, 4, 7, 10):
        for visible in (False, True):
            st, ax, ay, _, names = LS.ladder_batch(N, visible, 0.2)
            env = _env(N, visible, 0.2, True, st.E)
            env.human_policy_name = "linear"
            H.upload(env, st)
            ob, reward, done, info = env.step(torch.from_numpy(np.stack([ax, ay], -1)).to(env.device))
            torch.cuda.synchronize()
            ref_st = st.copy()
            cport.ladder_counts(reset=True)
            ref = cport.env_step(H.oracle_cfg_for(env, cport.HUMANS_LINEAR), ref_st, ax, ay, update=True)
            _add(total)
            what = "linear N=%d visible=%d" % (N, visible)
            for k, v in (("reward", reward), ("done", done), ("info", info), ("dmin", env.dmin),
                         ("hh_count", env.hh_count)):
                bad = H.bit_mismatch(v.cpu().numpy(), ref[k])
                assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
            got = H.download(env)
            np.testing.assert_allclose(got.hpx, ref_st.hpx, rtol=0, atol=1e-12, err_msg=what)
            np.testing.assert_allclose(got.hpy, ref_st.hpy, rtol=0, atol=1e-12, err_msg=what)
            H.assert_state_equal(got, ref_st, fields=("rpx", "rpy", "rvx", "rvy", "gtime"), what=what)
    _assert_reached(total, [k for k in STEP_EVENTS if k != "human_time_edge"], "linear")


@pytest.mark.parametrize("unicycle", [False, True])
@pytest.mark.parametrize("path", sorted(ROLLOUT_PATHS))
def test_rollout_on_ladder_batches_equals_single_steps_and_oracle(path, unicycle, tuning):
    """mcn_env_rollout over 8 steps (3 + 5) == 8 mcn_env_step calls, every byte, with and without a scenario pool
    (Explorer records: danger count and distance sum, fin_info / fin_time / fin_return); without a pool also == the
    oracle's trajectory (holonomic: bitwise; unicycle: the heading bitwise); a one-step launch == the oracle's boundary
    step, bitwise (unicycle: the ladder, the heading and the clock).  Every launch of a quad path asserts the form that
    went out.  The four-wavefront form double-buffers velocities by step parity, from 0 in every launch: 3 + 5 begins
    its second launch on an odd step of the sequence (tests/test_orca_edges_gpu.py cuts an even launch too)."""
    torch = need_gpu()
    from modelcrowdnav_amd.envs import scenarios as S
    Ns, quad, tu = ROLLOUT_PATHS[path]
    form = forced_form(path)
    tuning(**tu)
    T = 8
    total = {}
    for N, visible, dd, count_hh in ladder_configs(Ns, quad):
        st, ax0, ay0, _, names = LS.ladder_batch(N, visible, dd, unicycle)
        E = st.E
        rng = np.random.RandomState(N * 2 + visible)
        ax = np.concatenate([ax0[None], rng.randint(0, 17, (T - 1, E)) / 16.0])
        ay = np.concatenate([ay0[None], (rng.randint(-4, 5, (T - 1, E)) / 16.0) if not unicycle else
                             np.zeros((T - 1, E))])
        acts = torch.from_numpy(np.stack([ax, ay], -1))
        what = "%s N=%d visible=%d dd=%g unicycle=%d" % (path, N, visible, dd, unicycle)
        for with_pool in (False, True):
            a, b = (_env(N, visible, dd, count_hh, E, unicycle) for _ in range(2))
            for env in (a, b):
                H.upload(env, st)
                if with_pool:
                    pool = S.scenario_pool(env.spec(), "test", range(16), N, "circle_crossing")
                    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=np.arange(E) % 16, fin_slots=2)
            acts_d = acts.to(a.device)
            launch(a, acts_d[:3], form); launch(a, acts_d[3:], form)
            for t in range(T):
                b.step(acts_d[t])
            torch.cuda.synchronize()
            assert_same_bytes(snapshot(a), snapshot(b), (what, with_pool))
            if with_pool:
                assert int(a.rollout_buffers["fin_count"].sum().item()) > 0
                continue
            ref_st = st.copy()
            cfg = H.oracle_cfg_for(a)
            cport.ladder_counts(reset=True)
            for t in range(T):
                ref = cport.env_step(cfg, ref_st, ax[t], ay[t], update=True)
                if t == 0:
                    _add(total)
            cport.ladder_counts(reset=True)
            fields = H.STATE_FIELDS + ("rtheta",)
            if unicycle:
                fields = tuple(f for f in fields if f not in ("rpx", "rpy", "rvx", "rvy", "hpx", "hpy", "hvx", "hvy",
                                                              "human_times"))
            H.assert_state_equal(H.download(a), ref_st, fields=fields, what=what)
            if unicycle:
                continue        # later steps see device-trig robot positions: the first step is compared below
            for k, v in (("reward", a.reward), ("done", a.done), ("info", a.info), ("dmin", a.dmin),
                         ("hh_count", a.hh_count), ("human_act", a.human_act)):
                bad = H.bit_mismatch(v.cpu().numpy(), ref[k])
                assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
        # a one-step launch alone, bitwise against the oracle: the rungs of the boundary step itself (the
        # trajectories above only show the last step's record and what the Explorer accumulates)
        c = _env(N, visible, dd, count_hh, E, unicycle)
        H.upload(c, st)
        launch(c, acts.to(c.device)[:1], form)
        torch.cuda.synchronize()
        ref_st = st.copy()
        ref = cport.env_step(H.oracle_cfg_for(c), ref_st, ax[0], ay[0], update=True)
        for k, v in (("reward", c.reward), ("done", c.done), ("info", c.info), ("dmin", c.dmin),
                     ("hh_count", c.hh_count)):
            bad = H.bit_mismatch(v.cpu().numpy(), ref[k])
            assert len(bad) == 0, (what, "first step", k, len(bad), _where(names, bad))
        H.assert_state_equal(H.download(c), ref_st, fields=("rtheta", "gtime") if unicycle else H.STATE_FIELDS,
                             what=what + " first step")
    events = UNICYCLE_EVENTS if unicycle else STEP_EVENTS
    _assert_reached(total, events, path)


# ------------------------------------------------------------------------------------------ social-force humans
def _sf_env(N, visible, dd, count_hh, E, params):
    env = H.make_vec_env(E, N, robot_visible=visible, **{"humans.policy": "socialforce"})
    assert env.human_policy_name == "socialforce"
    env._sf.strength, env._sf.range, env._sf.relaxation_rate = params
    env.discomfort_dist = dd
    env.count_hh = count_hh
    return env


def _sf_hold_velocities(got, want, mag, exact, names, what):
    """human_act against the restatement: bitwise where it is exact (A = 0), else within SF_TOL * M.  Returns the
    largest error / tolerance."""
    if exact:
        bad = H.bit_mismatch(got, want)
        assert len(bad) == 0, (what, "human_act", len(bad), _where(names, bad))
        return 0.0
    assert np.isfinite(got).all() and np.isfinite(want).all(), what
    tol = SF_TOL * mag[..., None]
    err = np.abs(got - want)
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, (what, "human_act", len(bad), _where(names, bad), float((err / np.maximum(tol, 1e-300)).max()))
    return float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0)))


@pytest.mark.parametrize("update", [1, 0])
@pytest.mark.parametrize("params", [SF_INERT, SF_DEFAULT], ids=["inert", "default"])
def test_social_force_step_on_ladder_batches(params, update, tuning):
    """env_step_kernel<.., MCN_HUMANS_SOCIALFORCE, HH 0 / 1> on the ladder batches: 5 and 10 humans at compile-time N
    and force_generic, 1 .. 32 at run-time N, step_block 64 and 256.  The velocity against tests/social_force_ref.py;
    everything after it bitwise against the oracle's given-velocity step.

      inert    (A, B, k) = (0, 0.2, 4): every m = 0 * exp(..) is exactly 0, so the restatement is bit-exact and
               human_act is held to it bitwise; the oracle is fed the restatement's velocities.  A human at rest gets
               w = e exactly, so the first-arrival block ends exactly one radius from its goal (human_time_edge).
      default  (4, 0.2, 2): human_act within 8 * 2^-52 * M of the restatement; the oracle is fed the device's
               velocities.  (human_time_edge is not reached with these parameters: tests/test_social_force_cpu.py.)

    As for the ORCA kernels the oracle counts human_time_edge only on a step that updates the state."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    exact = params == SF_INERT
    total, worst, runs = {}, 0.0, 0
    for N, visible, dd, count_hh in ladder_configs(SF_COMPILED_NS + SF_GENERIC_NS, quad=False):
        st, ax, ay, _, names = LS.ladder_batch(N, visible, dd)
        want, mag = sf_ladder_reference(N, visible, dd, params)
        env = _sf_env(N, visible, dd, count_hh, st.E, params)
        act = torch.from_numpy(np.stack([ax, ay], -1)).to(env.device)
        for block, generic in sf_step_forms(N):
            tuning(step_block=block, force_generic=generic)
            what = "social force %s N=%d visible=%d dd=%g count_hh=%d block=%d generic=%d update=%d" % (
                "inert" if exact else "default", N, visible, dd, count_hh, block, generic, update)
            H.upload(env, st)
            env.human_act.fill_(float("nan"))
            ob, reward, done, info = env.step(act, update=bool(update))
            torch.cuda.synchronize()
            assert _hip.last_dispatch() == "env_step_kernel", what
            got = dict(reward=reward.cpu().numpy(), done=done.cpu().numpy(), info=info.cpu().numpy(),
                       dmin=env.dmin.cpu().numpy(), hh_count=env.hh_count.cpu().numpy(),
                       human_act=env.human_act.cpu().numpy())
            if not update:
                got.update(nobs_px=ob.pos[..., 0].cpu().numpy(), nobs_py=ob.pos[..., 1].cpu().numpy(),
                           nobs_vx=ob.vel[..., 0].cpu().numpy(), nobs_vy=ob.vel[..., 1].cpu().numpy())
            worst = max(worst, _sf_hold_velocities(got["human_act"], want, mag, exact, names, what))
            ref_st = st.copy()
            cport.ladder_counts(reset=True)
            ref = cport.env_step(H.oracle_cfg_for(env, cport.HUMANS_GIVEN), ref_st, ax, ay, update=bool(update),
                                 given_v=np.array(want) if exact else got["human_act"])
            if (block, generic) == sf_step_forms(N)[0]:
                _add(total)
            for k in got:
                bad = H.bit_mismatch(got[k], ref[k])
                assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
            H.assert_state_equal(H.download(env), ref_st if update else st, fields=H.STATE_FIELDS, what=what)
            runs += 1
    cport.ladder_counts(reset=True)
    events = [k for k in STEP_EVENTS if k != "human_time_edge" or (exact and update)]
    _assert_reached(total, events, "social force")
    print("social force %s update=%d: %d runs, largest error / tolerance %.4f, reached %s" % (
        "inert" if exact else "default", update, runs, worst, {k: total[k] for k in events}))


@pytest.mark.parametrize("N", SF_COMPILED_NS)
def test_social_force_rollout_on_ladder_batches(N, tuning):
    """mcn_env_rollout_sf with the inert parameters over 8 steps (3 + 5) == 8 mcn_env_step_sf calls, every byte, with
    and without a scenario pool; the multi-step launches go out as env_step_loop_sf_kernel.  Without a pool also == the
    host replay of 8 restatement + oracle steps (bit-exact: A = 0), and a one-step launch == the oracle's boundary
    step."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    from modelcrowdnav_amd.envs import scenarios as S
    T, params = 8, SF_INERT
    total = {}
    for N_, visible, dd, count_hh in ladder_configs((N,), quad=False):
        st, ax0, ay0, _, names = LS.ladder_batch(N, visible, dd)
        E = st.E
        rng = np.random.RandomState(N * 2 + visible)
        ax = np.concatenate([ax0[None], rng.randint(0, 17, (T - 1, E)) / 16.0])
        ay = np.concatenate([ay0[None], rng.randint(-4, 5, (T - 1, E)) / 16.0])
        acts = torch.from_numpy(np.stack([ax, ay], -1))
        what = "social force rollout N=%d visible=%d dd=%g count_hh=%d" % (N, visible, dd, count_hh)
        for with_pool in (False, True):
            a, b = (_sf_env(N, visible, dd, count_hh, E, params) for _ in range(2))
            for env in (a, b):
                H.upload(env, st)
                if with_pool:
                    pool = S.scenario_pool(env.spec(), "test", range(16), N, "circle_crossing")
                    env.attach_rollout(gamma=0.9, pool=pool, case_stride=3, first_cases=np.arange(E) % 16, fin_slots=2)
            acts_d = acts.to(a.device)
            for lo, hi in ((0, 3), (3, T)):
                a.rollout(acts_d[lo:hi])
                assert _hip.last_dispatch() == "env_step_loop_sf_kernel", (what, _hip.last_dispatch())
            for t in range(T):
                b.step(acts_d[t])
            assert _hip.last_dispatch() == "env_step_kernel"
            torch.cuda.synchronize()
            assert_same_bytes(snapshot(a), snapshot(b), (what, with_pool))
            if with_pool:
                assert int(a.rollout_buffers["fin_count"].sum().item()) > 0
                continue
            ref_st = st.copy()
            cfg = H.oracle_cfg_for(a, cport.HUMANS_GIVEN)
            cport.ladder_counts(reset=True)
            for t in range(T):
                ref, want, _ = sf_oracle_step(cfg, ref_st, ax[t], ay[t], params, visible)
                if t == 0:
                    _add(total)
            cport.ladder_counts(reset=True)
            H.assert_state_equal(H.download(a), ref_st, fields=H.STATE_FIELDS + ("rtheta",), what=what)
            for k, v in (("reward", a.reward), ("done", a.done), ("info", a.info), ("dmin", a.dmin),
                         ("hh_count", a.hh_count), ("human_act", a.human_act)):
                bad = H.bit_mismatch(v.cpu().numpy(), want if k == "human_act" else ref[k])
                assert len(bad) == 0, (what, k, len(bad), _where(names, bad))
        c = _sf_env(N, visible, dd, count_hh, E, params)
        H.upload(c, st)
        c.rollout(acts.to(c.device)[:1])
        torch.cuda.synchronize()
        assert _hip.last_dispatch() == "env_step_kernel", (what, _hip.last_dispatch())
        ref_st = st.copy()
        ref, want, _ = sf_oracle_step(H.oracle_cfg_for(c, cport.HUMANS_GIVEN), ref_st, ax[0], ay[0], params, visible)
        for k, v in (("reward", c.reward), ("done", c.done), ("info", c.info), ("dmin", c.dmin),
                     ("hh_count", c.hh_count), ("human_act", c.human_act)):
            bad = H.bit_mismatch(v.cpu().numpy(), want if k == "human_act" else ref[k])
            assert len(bad) == 0, (what, "first step", k, len(bad), _where(names, bad))
        H.assert_state_equal(H.download(c), ref_st, fields=H.STATE_FIELDS, what=what + " first step")
    cport.ladder_counts(reset=True)
    _assert_reached(total, STEP_EVENTS, "social force rollout")
    print("social force rollout N=%d: the first step reached %s" % (N, {k: total[k] for k in STEP_EVENTS}))


_LADDER_KEYS = ("reward", "done", "info", "dmin", "hh_count")
_TRIG_FIELDS =("rpx", "rpy", "rvx", "rvy", "hpx", "hpy", "hvx", "hvy", "human_times")


@pytest.mark.parametrize("unicycle", [False, True])
def test_wg4_rollout_on_rolled_ladder_batch(unicycle, tuning):
    """tests/test_orca_edges_gpu.py rolled_wg4_battery on the dyadic ladder batch of 5 humans (discomfort_dist 0.25,
    overlap count on: alone it reaches every rung event, E = 373), 8 steps as 3 + 1 + 4.  The boundary step is the first:
    the one-step launch of every roll is held to the equally rolled oracle step bitwise (unicycle: the ladder, the
    heading and the clock), the trajectories of two rolls to the rolled single steps byte for byte and to the oracle
    with the field exclusions of test_rollout_on_ladder_batches_equals_single_steps_and_oracle.  The oracle replays
    the unrolled batch once."""
    N, T, dd, count_hh = 5, 8, 0.25, True
    tuning(rollout_fused=1, rollout_split=2)
    st, ax0, ay0, _, names = LS.ladder_batch(N, False, dd, unicycle)
    E = st.E
    rng = np.random.RandomState(N * 2)
    ax = np.concatenate([ax0[None], rng.randint(0, 17, (T - 1, E)) / 16.0])
    ay = np.concatenate([ay0[None], (rng.randint(-4, 5, (T - 1, E)) / 16.0) if not unicycle else np.zeros((T - 1, E))])
    ref_st = st.copy()
    cfg = H.oracle_cfg_for(_env(N, False, dd, count_hh, E, unicycle))
    total = {}
    cport.ladder_counts(reset=True)
    for t in range(T):
        ref = cport.env_step(cfg, ref_st, ax[t], ay[t], update=True)
        if t == 0:
            ref0, ref_st0 = ref, ref_st.copy()
            _add(total)
    cport.ladder_counts(reset=True)
    _assert_reached(total, UNICYCLE_EVENTS if unicycle else STEP_EVENTS, "rolled ladder batch")

    def check(env, r, r_st, perm, rolled, what, keys, fields):
        for k in keys:
            bad = H.bit_mismatch(getattr(env, k).cpu().numpy(), r[k][perm])
            assert len(bad) == 0, (what, k, len(bad), _where(rolled, bad))
        H.assert_state_equal(H.download(env), LS.take(r_st, perm), fields=fields, what=what)

    def check_first(env, perm, rolled, what):
        check(env, ref0, ref_st0, perm, rolled, what, _LADDER_KEYS if unicycle else _LADDER_KEYS + ("human_act",),
              ("rtheta", "gtime") if unicycle else H.STATE_FIELDS + ("rtheta",))

    def check_last(env, perm, rolled, what):
        # unicycle: later steps see device-trig robot positions, so only the heading, the clock and what does not move
        fields = H.STATE_FIELDS + ("rtheta",)
        check(env, ref, ref_st, perm, rolled, what, () if unicycle else _LADDER_KEYS + ("human_act",),
              tuple(f for f in fields if f not in _TRIG_FIELDS) if unicycle else fields)

    rolled_wg4_battery(lambda: _env(N, False, dd, count_hh, E, unicycle), LS.take, st, np.stack([ax, ay], -1), names,
                       (0, 3, 4, T), check_first, check_last, "rolled ladder batch unicycle=%d" % unicycle)


def _lookahead_rewards_on_ladder_batches(body, what):
    """A zeroed network (lookahead_harness.zeroed: V == 0.0 exactly) on the look-ahead blocks, N = 1..10, 13 and 32 (all
    three MAXN variants of the LSTM-RL order): every value is cport.lookahead_reward bit for bit; the argmax goes on at
    |robot - goal| == rr and returns -1 inside."""
    pol = L.zeroed(L.policy(body, seed=0), body)
    pol.build_action_space(1.0)
    table = pol._action_table
    total = {}
    for N in list(range(1, 11)) + list(GENERIC_NS):
        st, names = LS.lookahead_batch(N, table)
        env = H.make_vec_env(st.E, N)
        H.upload(env, st)
        actions, best, values = pol.predict_batch(env, want_values=True)
        cport.ladder_counts(reset=True)
        ref = cport.lookahead_reward(st, table, 0.25)
        _add(total)
        values = values.cpu().numpy()
        bad = H.bit_mismatch(values, ref)
        assert len(bad) == 0, (body, N, len(bad), _where(names, bad))
        best, actions = best.cpu().numpy(), actions.cpu().numpy()
        for e, name in enumerate(names):
            if name in ("la-at-goal", "la-at-goal-edge"):       # (values == ref bitwise: best is ref's first maximum)
                L.check_choice(values[e], best[e], actions[e], ref[e], table, name == "la-at-goal", what=(N, e))
    _assert_reached(total, LA_EVENTS, what)


def test_sarl_lookahead_rewards_on_ladder_batches():
    """mcn_sarl_predict with a network whose V is exactly 0: values are exactly the look-ahead reward, bitwise against
    cport.lookahead_reward on the look-ahead blocks, N = 1..10, 13 and 32; the argmax goes on at |robot - goal| == rr and
    returns -1 inside."""
    _lookahead_rewards_on_ladder_batches("sarl", "mcn_sarl_predict")


@pytest.mark.parametrize("N", GENERIC_NS)
def test_sarl_predict_above_ten_humans_against_torch_reference(N):
    """N = 13 and 32 (mcn_sarl_predict takes N <= MCN_MAX_HUMANS = 32): a trained-size random network against
    pyref.sarl_predict at the suite's 1e-5 bar, on a few envs of the look-ahead batch."""
    from oracle import pyref
    pol = L.policy("sarl", seed=3)
    pol.build_action_space(1.0)
    table = pol._action_table
    st, names = LS.lookahead_batch(N, table)
    env = H.make_vec_env(st.E, N)
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    w = L.cpu_weights(pol)
    for e in range(0, st.E, 19):
        if names[e] == "la-at-goal":
            continue
        ref, idx = pyref.sarl_predict(w, L.self_row(st, e), L.humans(st, e), table)
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=L.TOL, err_msg="N=%d env %d (%s)" % (N, e, names[e]))


@pytest.mark.parametrize("body", ["lstm_rl", "cadrl"])
def test_lstm_rl_and_cadrl_lookahead_rewards_on_ladder_batches(body):
    """lstm_rl_value.hip's reward ladder, as test_sarl_lookahead_rewards_on_ladder_batches: with a zeroed network V is
    exactly 0 (LSTM-RL: every gate 1/2, the cell state and h stay 0), so every value is the look-ahead reward bit for
    bit, N = 1..10, 13 and 32 (all three MAXN variants of the order)."""
    _lookahead_rewards_on_ladder_batches(body, "mcn_%s_predict" % body)
