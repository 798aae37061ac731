"""GPU: the social-force step on the edges of its definition, and "the cfg's orca_* fields are not read".

  orca fields   include/mcn.h promises that mcn_env_step_sf does not read cfg->orca_*; the overlap count of every
                non-ORCA step (social force, given velocities, linear) goes through a float32 pre-filter that used to
                rebuild the plain radius from the ORCA-padded one.  Overlapping pairs well inside the pre-filter's
                margin (tests/sf_edge_states.py: overlap_batch), stepped with orca safety_space 0, 0.5, 1e6 and NaN and
                with default and odd neighbor_dist / time_horizon: every run leaves the bytes of the first, and
                hh_count is the oracle's.
  edges         tests/sf_edge_states.py edge_batch: |g - p| and |w| exactly v_pref and an ulp either side, v_pref = 0, a
                human on its goal, -0.0, coincident humans and robot, a lone human, exp subnormal / underflowing /
                overflowing, a human or the robot at +-inf or NaN, whole envs translated by 2^10 and 2^20 -- under seven
                parameter sets (A = 0, k = 0, B = 1e-300, 2^-10, 2^10 among them), N = 1 .. 32, every form of the step
                kernel, update 0 and 1.  Against tests/social_force_ref.py: bitwise where A = 0 (no exp survives),
                else within 8 * 2^-52 * M (M: the restatement's magnitude, tests/test_social_force_gpu.py part 1)
                wherever the definition's value is finite, and the same NaN / signed inf where it is not.  In the
                exp-range block the humans keep normal-sized e and v, so M is of order 1 there: a result that differs by
                an ulp of a subnormal exp passes, as the bound says; an exp that is 0 or inf at the wrong place does not.
                What the inputs reach is asserted from an instrumented walk through the definition in
                tests/test_social_force_cpu.py, and from the restatement's results here.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import kernel_paths as KP  # noqa: E402
from tests import sf_edge_states as SE  # noqa: E402
from tests.rollout_harness import assert_same_bytes, need_gpu, snapshot  # noqa: E402

SAFETY = (0.0, 0.5, 1e6, float("nan"))
ORCA_RANGES = ((None, None), (3.7, 1.3))                       # (neighbor_dist, time_horizon): the defaults, odd ones


def _sf_env(E, N, vis, params):
    env = H.make_vec_env(E, N, robot_visible=bool(vis), **{"humans.policy": "socialforce"})
    assert env.human_policy_name == "socialforce"
    env._sf.strength, env._sf.range, env._sf.relaxation_rate = params
    return env


# ------------------------------------------------------------------------------------------ the cfg's orca_* fields
@pytest.mark.parametrize("humans", ("socialforce", "given", "linear"))
def test_orca_fields_of_the_cfg_are_not_read(humans, tuning):
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    counted = 0
    for N in (2, 5, 10, 13):
        st, ax, ay, pairs = SE.overlap_batch(N)
        act = torch.from_numpy(np.stack([ax, ay], -1)).cuda()
        gv_host = np.random.RandomState(N).randint(-8, 9, (st.E, N, 2)) / 16.0
        ref = cport.env_step(cport.default_cfg(count_hh=1, track_human_times=1, human_policy=cport.HUMANS_GIVEN),
                             st.copy(), ax, ay, update=False, given_v=gv_host)
        assert (ref["hh_count"] == pairs).all() and (pairs > 0).all()
        counted += int(pairs.sum())
        if humans == "socialforce":
            env = _sf_env(st.E, N, N % 2, KP.SF_DEFAULT)
        else:
            env = H.make_vec_env(st.E, N, robot_visible=bool(N % 2))
            if humans == "linear":
                env.human_policy_name = "linear"
        env.count_hh = True
        gv = torch.from_numpy(gv_host).cuda() if humans == "given" else None
        nd0, th0 = env._orca.neighbor_dist, env._orca.time_horizon
        for block, generic in KP.sf_step_forms(N):
            tuning(step_block=block, force_generic=generic, pair_stream=0)
            for update in (1, 0):
                first = None
                for safety in SAFETY:
                    for nd, th in ORCA_RANGES:
                        env._orca.safety_space = safety
                        env._orca.neighbor_dist, env._orca.time_horizon = nd or nd0, th or th0
                        H.upload(env, st)
                        env.human_act.fill_(7.0); env.nobs_pos.fill_(7.0); env.nobs_vel.fill_(7.0)
                        env.step(act, update=bool(update), given_v=gv)
                        torch.cuda.synchronize()
                        assert _hip.last_dispatch() == "env_step_kernel"
                        what = "%s N=%d block=%d generic=%d update=%d safety_space=%r neighbor_dist=%r" % (
                            humans, N, block, generic, update, safety, nd)
                        got = snapshot(env)
                        got["nobs_pos"], got["nobs_vel"] = env.nobs_pos.cpu().numpy(), env.nobs_vel.cpu().numpy()
                        hh = env.hh_count.cpu().numpy()
                        bad = H.bit_mismatch(hh, ref["hh_count"])
                        assert len(bad) == 0, (what, "hh_count", len(bad), hh[bad[0][0]], ref["hh_count"][bad[0][0]])
                        if first is None:
                            first = got
                        assert_same_bytes(got, first, what)
    print("%s: %d overlapping pairs counted by the oracle per run" % (humans, counted))


# ------------------------------------------------------------------------------------------ edges of the definition
def _hold(got, want, mag, exact, names, what):
    """got against the restatement: bitwise for an exact parameter set; otherwise the same non-finite class at the same
    place (NaN where NaN, inf of the same sign where inf), within 8 * 2^-52 * M where the definition's value is finite,
    and the definition's sign on an exact zero.  Returns the largest error / tolerance over the finite values."""
    if exact:
        bad = H.bit_mismatch(got, want)
        assert len(bad) == 0, (what, len(bad), sorted({names[int(i[0])] for i in bad})[:6], bad[:3].tolist())
        return 0.0
    fin = np.isfinite(want)
    cls = (np.isnan(got) != np.isnan(want)) | (np.isinf(want) & (got != want)) | (fin & ~np.isfinite(got))
    assert not cls.any(), (what, "non-finite class", sorted({names[int(i[0])] for i in np.argwhere(cls)})[:6],
                           np.argwhere(cls)[:3].tolist())
    with np.errstate(invalid="ignore", over="ignore"):
        tol = np.where(np.isfinite(mag), 8 * 2.0 ** -52 * mag, np.inf)[..., None] * np.ones(2)
        err = np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, want, 0)), 0)
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, (what, len(bad), sorted({names[int(i[0])] for i in bad})[:6], bad[:3].tolist())
    zero = fin & (want == 0) & (got == 0)
    assert (np.signbit(got[zero]) == np.signbit(want[zero])).all(), (what, "sign of zero")
    ok = fin & (tol > 0) & np.isfinite(tol)
    return float((err[ok] / tol[ok]).max()) if ok.any() else 0.0


def _reached(st, want, names):
    """Counts over the restatement's results: NaN / inf components, exact and negative zeros, humans whose speed is
    exactly v_pref (a tie that was not clipped, or a clip that landed on it), NaNs of the deep-overlap block (exp
    overflow), finite results of the exp-range block (exp subnormal or underflowed)."""
    with np.errstate(invalid="ignore", over="ignore"):
        speed = np.sqrt((want ** 2).sum(-1))
    block = lambda b: np.array([n == b for n in names])
    return dict(nan=int(np.isnan(want).sum()), inf=int(np.isinf(want).sum()), zero=int((want == 0).sum()),
                neg_zero=int(((want == 0) & np.signbit(want)).sum()),
                speed_is_vpref=int(((speed == st.hvpref) & (st.hvpref > 0) & block("goal-clip")[:, None]).sum()
                                   + ((speed == st.hvpref) & (st.hvpref > 0) & block("w-clip")[:, None]).sum()),
                clipped_to_vpref=int((np.isfinite(speed) & (np.abs(speed - st.hvpref) <= 2.0 ** -52) & block("w-clip")[:, None]).sum()),
                nan_in_deep_overlap=int(np.isnan(want[block("deep-overlap")]).sum()),
                finite_in_exp_range=int(np.isfinite(want[block("exp-range")]).all(-1).sum()))


@pytest.mark.parametrize("visible", (0, 1))
@pytest.mark.parametrize("N", SE.NS)
def test_velocities_on_the_edges_of_the_definition(N, visible, tuning):
    """tests/sf_edge_states.py edge_batch under every parameter set of SE.PARAMS: the exported velocity against the
    restatement (bitwise for A = 0), and what the step does with it -- the state's velocity is that velocity and the
    position is pos + w dt (update = 1), or the look-ahead observation holds them and the state is left alone
    (update = 0) -- bit for bit, NaN and inf included.  Lane groups of 64 / N humans, idle lanes at 13, E = 181."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    st, ax, ay, names = SE.edge_batch(N, visible)
    act = torch.from_numpy(np.stack([ax, ay], -1)).cuda()
    pos0 = np.stack([st.hpx, st.hpy], -1)
    twin = [e for e, n in enumerate(names) if n == "nonfinite-robot"]
    worst, reached = {}, {}
    for group, params in SE.PARAMS.items():
        want, mag = KP.sf_velocities(st, params, visible)
        reached[group] = _reached(st, want, names)
        env = _sf_env(st.E, N, visible, params)
        for block, generic in KP.sf_step_forms(N):
            tuning(step_block=block, force_generic=generic)
            for update in (1, 0):
                what = "%s N=%d visible=%d block=%d generic=%d update=%d" % (group, N, visible, block, generic, update)
                H.upload(env, st)
                env.human_act.fill_(7.0); env.nobs_pos.fill_(7.0); env.nobs_vel.fill_(7.0)
                env.step(act, update=bool(update))
                torch.cuda.synchronize()
                assert _hip.last_dispatch() == "env_step_kernel"
                got = env.human_act.cpu().numpy()
                ratio = _hold(got, want, mag, group in SE.EXACT, names, what)
                worst[group] = max(worst.get(group, 0.0), ratio)
                with np.errstate(invalid="ignore", over="ignore"):
                    nxt = pos0 + got * SE.DT
                vel, pos = (env.hvel, env.hpos) if update else (env.nobs_vel, env.nobs_pos)
                H.assert_bits_equal(vel.cpu().numpy(), got, what + " velocity")
                H.assert_bits_equal(pos.cpu().numpy(), nxt, what + " position")
                if not update:
                    H.assert_state_equal(H.download(env), st, fields=H.STATE_FIELDS, what=what + " look-ahead")
                if not visible:         # a NaN or infinite robot position the humans do not see changes nothing
                    H.assert_bits_equal(got[twin[8:]], got[twin[:8]], what + " unseen robot")
    # what the restatement's own results say the inputs reached (the full classification of the inputs, from an
    # instrumented walk through the definition, is asserted without a GPU: tests/test_social_force_cpu.py)
    others = N >= 2 or visible
    assert all(r["nan"] > 0 for r in reached.values())
    assert reached["still"]["speed_is_vpref"] > 0 and reached["still"]["neg_zero"] > 0 and reached["still"]["clipped_to_vpref"] > 0
    assert reached["inert"]["speed_is_vpref"] > 0 and reached["default"]["zero"] > 0
    assert not others or (reached["B-small"]["nan_in_deep_overlap"] > 0 and reached["B-tiny"]["nan_in_deep_overlap"] > 0)
    assert not others or reached["default"]["finite_in_exp_range"] > 0
    print("N=%d visible=%d: largest error / tolerance per parameter set %s; the definition's results hold %s" % (
        N, visible, {k: round(v, 4) for k, v in worst.items()}, reached))
