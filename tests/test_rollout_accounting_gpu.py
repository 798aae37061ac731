"""Every step kernel's Explorer accounting (include/mcn.h: mcn_rollout) against a host replay, bit for bit.

The discounted return, the finished-episode records, the gated "too close" counters and the in-kernel restart from the
scenario pool exist in these forms in device code, each written differently: the memory-resident functions of
env_common.hpp (explorer_account for env_step.hip, of which env_step_quad.hip keeps a written-out copy;
restart_human_from_pool and the robot stores for both), env_pair.hip's form on the packed record, and the
register-resident twin of env_rollout_quad.hip and env_rollout_wg4.hip.  tests/rollout_ref.py replays the contract in plain Python on the C oracle's steps; here every
decomposition of mcn_env_step (ORCA humans and given velocities) and every path of mcn_env_rollout runs 130 steps of 251
envs under ten parameter sets and must leave the same bytes: the whole mcn_roll_rec, all of fin_return / fin_time /
fin_info (sentinel-filled before the run: NaN / 0xFF), every step record and the env state with the restarts replayed.
All comparisons are bitwise (tests/helpers.py bit_mismatch: -0.0 against +0.0 fails, NaN matches NaN); the robot is
holonomic throughout, so no value depends on device trigonometry: the restart of a unicycle robot (where the fused
kernels go on from the register copy of rtheta) is covered kernel against kernel by
tests/test_env_step_gpu.py::test_rollout_launch_unicycle_robot, not here.  Each test asserts from the replay's own event
counters (rollout_ref.REQUIRED, checked without a GPU in tests/test_rollout_ref_cpu.py) that its inputs reached what it
is there for.

Which test catches which break (value-only changes of one body; none of them moves a store):

  break                                                         caught by
  ------------------------------------------------------------  -----------------------------------------------------
  gate `e >= sf - 1` -> `e >= sf`                               explorer-mid / -last, short-table, table-128 / -129:
                                                                danger_count of env sf - 1 itself (boundary_gated; sf is
                                                                chosen per workload so that this env and env sf - 2
                                                                both meet a Danger step in their second episode)
  gate dropped for danger_episodes > 0, or `<` -> `<=`          every explorer-* set (danger_gated), explorer-none
                                                                (nothing may count)
  danger_episodes <= 0 not treated as "every step"              latest-wins, device-pool, no-pool (danger_counted)
  distance summed before the gate, or dmin of another step      danger_dist_sum of every explorer-* set
  timeout recorded with the clock instead of time_limit         fin_time of every set (timeout)
  fin_time taken before the step's dt is added                  fin_time of every set (reach, collision)
  return with a fused multiply-add, or the wrong table entry    ep_return / fin_return of every set
  no clamp at disc_len - 1 (reads past the table)               short-table (clamped)
  streaming kernel taken beyond its 128-entry table limit,      table-128 / table-129 on the given-velocity paths
  or a table entry >= 64 misread                                (mcn_last_dispatch; disc_index_ge64.  The kernel
                                                                reads the entry from global memory; the LDS copies
                                                                of the table that could be cut at 64 entries were
                                                                A/B forms and are no longer in the sources)
  episode k >= fin_slots overwrites a slot, or is counted out   explorer-*, device-pool, no-pool (dropped): sentinel
                                                                slots and fin_count
  one slot keeps the first episode instead of the latest        latest-wins (overwritten counts only records that change
                                                                the slot's bytes; first_wins_differs: >= 84 envs per
                                                                workload end on a record unlike their first episode's)
  next_case wrap `>=` -> `>`, stride applied twice or never     next_case of every pool set (wrap); latest-wins (stride 0,
                                                                pool of 1), device-pool (stride pool_size - 1)
  restart takes the advanced case, or the neighbour's           env state after a restart (humans of the wrong case)
  pool velocities ignored / zeros where a pool gives some       explorer-* (restart_moving) / device-pool (+0.0 exactly)
  rtheta, clock, first arrivals, robot velocity not reset       env state after a restart (rtheta == robot_theta0 = 0.625)
  a fin_* store not guarded by its pointer                      test_parts_off (would fault; read the guards first)
  accounting done although `state` is NULL                      test_parts_off: sentinel bytes of every buffer
  split-wavefront hand-off (s_dn / s_case) one step late        quad-split, quad-rollout-split: state after a restart
  record not written back between launches                      rollout paths: 1 + 37 + 92 steps, compared after each

The social-force instantiations (env_step_kernel<.., MCN_HUMANS_SOCIALFORCE, HH 1> at compile-time and run-time N, and
env_step_loop_sf_kernel) share the source of that tail but are other template instantiations: HH_T 1 where ORCA has 2, no
line slots in the LDS carve, and the loop restages its tiles around a restart.  They run the same replay twice over:

  sf-step / sf-rollout paths    strength 0 (rollout_ref.SF_PARAMS): the restatement is bit-exact, so the host replay runs
                                ahead as for ORCA humans and every set but latest-wins is compared as above
  test_social_force_accounting_in_lock_step
                                shipped strength: device exp may differ from the host's by an ulp, so the replay takes the
                                device's own velocities step by step (held to the restatement within 8 * 2^-52 * M)

  break in a social-force instantiation                         caught by
  ------------------------------------------------------------  -----------------------------------------------------
  any row of the table above                                    the same sets over the sf-step / sf-rollout paths;
                                                                latest-wins' rows (one slot keeps the first episode,
                                                                stride 0 on a pool of one) in lock step
  loop kernel keeps a finished env's humans in its LDS tiles    sf-rollout-loop: the velocities of the step after a
  (no restaging after the restart)                              restart (human_act, state) in every pool set
  loop kernel reads step t's action row for step t + 1          sf-rollout-loop: step records after each launch
  overlap count off in the HH 1 form, or on in the HH 0 form    hh_count of every step record (the replay counts)
  first arrivals not cleared by a restart, or stamped with      human_times in the state at 1 / 38 / 130 steps
  the clock before dt is added
  compile-time-N form sums the others in another order than     human_act at the checkpoints, bitwise (strength 0 keeps
  the run-time-N one                                            the sum exact: shown instead in lock step, where every
                                                                form must reproduce the first form's velocities bitwise)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import rollout_ref as R  # noqa: E402
from tests.kernel_paths import ROLLOUT_PATHS, SF_TOL, STEP_KERNELS, forced_form, select_step_kernel  # noqa: E402
from tests.rollout_harness import launch, need_gpu  # noqa: E402

STEP_DTYPE = np.dtype([("reward", "f8"), ("dmin", "f8"), ("done", "u1"), ("info", "u1"), ("reserved", "u2"),
                       ("hh_count", "i4")])                                             # mcn_step_rec
# mcn_env_step with ORCA humans: all nine decompositions at 5 humans (where the quad layout applies), the lane-per-human /
# deferred / run-time-N forms also at 7, and the three families at 10
ORCA_STEP = ([(k, 5) for k in STEP_KERNELS] + [(k, 7) for k in STEP_KERNELS if k != "auto" and not k.startswith("quad")] +
             [("auto", 10), ("deferred-lp3", 10), ("run-time-N-256", 10)])
GIVEN_STEP = [(ps, N) for N in (5, 10) for ps in (0, 1, 2)]
ROLLOUT = [("quad-rollout", 5), ("quad-rollout-split", 5), ("quad-rollout-wg4", 5), ("step-loop", 7), ("lp3-defer", 7),
           ("lp3-defer", 10), ("unfused", 5), ("unfused", 10)]
assert {p for p, _ in ROLLOUT} == set(ROLLOUT_PATHS) and all(N in ROLLOUT_PATHS[p][0] for p, N in ROLLOUT)
# social-force humans (mcn_env_step_sf / mcn_env_rollout_sf): the compile-time-N and force_generic instantiations at 5 and 10
# humans, the run-time-N one at 7, each at both block sizes; the looped kernel and its launch-per-step fallback
SF_FORMS = {"compiled-64": dict(step_block=64, force_generic=0), "compiled-256": dict(step_block=256, force_generic=0),
            "generic-64": dict(step_block=64, force_generic=1), "generic-256": dict(step_block=256, force_generic=1),
            "run-time-N-64": dict(step_block=64), "run-time-N-256": dict(step_block=256)}
SF_STEP = ([(f, N) for N in (5, 10) for f in ("compiled-64", "compiled-256", "generic-64", "generic-256")] +
           [("run-time-N-64", 7), ("run-time-N-256", 7)])
SF_ROLLOUT = [(which, N) for N in (5, 10) for which in ("loop", "launches")]
SF_PATHS = [("sf-step",) + c for c in SF_STEP] + [("sf-rollout",) + c for c in SF_ROLLOUT]
# a zero-strength crowd on a pool of one case never collides, so latest-wins cannot reach its `collision` requirement
# with the bit-exact parameters: that set runs in lock step with the shipped ones (below)
SF_SETS = [name for name in R.SETS if name != "latest-wins"]
PATHS = ([("step",) + c for c in ORCA_STEP] + [("given",) + c for c in GIVEN_STEP] + [("rollout",) + c for c in ROLLOUT] +
         SF_PATHS)
PATH_IDS = ["%s-%s-N%d" % p for p in PATHS]
SPLITS = ((0, 1), (1, 38), (38, R.T_ACC))                   # the launches of the rollout paths: 1 + 37 + 92 steps
assert tuple(b for _, b in SPLITS) == R.CHECKPOINTS


def _mode(path):
    return {"given": "given", "sf-step": "sf", "sf-rollout": "sf"}.get(path[0], "orca")


def _env(w):
    """A VecCrowdSim in the workload's initial state whose configuration is the one the replay's oracle ran with (for
    social-force humans: in every field but human_policy -- the oracle is handed their velocities)."""
    if w.mode == "sf":
        env = H.make_vec_env(w.E, w.N, **{"humans.policy": "socialforce"})
        assert env.human_policy_name == "socialforce"
        env._sf.strength, env._sf.range, env._sf.relaxation_rate = R.SF_PARAMS
    else:
        env = H.make_vec_env(w.E, w.N)
    env.time_limit = w.contract.time_limit
    if w.mode == "given":                         # what the streaming kernel takes (env_pair.hip)
        env.count_hh = env.track_human_times = env.export_human_actions = False
    H.upload(env, w.st0)
    from oracle import cport
    want = H.oracle_cfg_for(env, cport.HUMANS_ORCA if w.mode == "orca" else cport.HUMANS_GIVEN)
    for name, _ in want._fields_:
        assert getattr(want, name) == getattr(w.cfg, name), "the replay's oracle ran with another %s" % name
    return env


def _attach(env, w, null=()):
    """mcn_rollout as the parameter set says, every output buffer filled with a sentinel; `null`: pointers set to NULL."""
    torch = need_gpu()
    s = w.set
    pool = None
    if s["pool"] == "host":
        pool = w.scen
    elif s["pool"] == "device":                   # the dict form: used in place, pool_hvel NULL
        pool = {k: torch.from_numpy(w.pool[k]).to(env.device) for k in ("hpos", "hgoal", "hrad", "hvpref")}
    bufs = env.attach_rollout(gamma=0.9, pool=pool, case_stride=s["stride"], first_cases=w.first_cases,
                              fin_slots=s["fin_slots"], danger_episodes=s["danger_episodes"],
                              danger_short_from=w.contract.danger_short_from)
    roll = env._roll
    roll.robot_theta0 = R.THETA0
    assert H.bits_equal(bufs["disc"].cpu().numpy(), np.array(w.contract.disc))
    if "disc_len" in s:
        roll.disc_len = s["disc_len"]
    assert roll.disc_len == w.contract.disc_len and roll.pool_size == w.contract.pool_size
    assert bool(roll.pool_hvel) == (s["pool"] == "host") and roll.case_stride == w.contract.case_stride
    bufs["fin_return"].fill_(float("nan")); bufs["fin_time"].fill_(float("nan")); bufs["fin_info"].fill_(R.SENTINEL_INFO)
    for k in null:
        setattr(roll, k, None)
    if "state" in null:
        bufs["state"].fill_(float("nan"))
    return bufs


def _first(bad):
    return [tuple(int(x) for x in i) for i in bad[:4]]


def _compare(env, w, n, what, null=()):
    """Everything after n steps against the replay's snapshot."""
    torch = need_gpu()
    torch.cuda.synchronize()
    ref_st, snap = w.snaps[n]
    what = "%s after %d steps" % (what, n)
    got_st = H.download(env)
    H.assert_state_equal(got_st, ref_st, fields=H.STATE_FIELDS + ("rtheta",), what=what)
    bufs = env.rollout_buffers
    if "state" in null:                           # no accounting at all: not a byte of any buffer written
        assert np.isnan(bufs["state"].cpu().numpy()).all(), what
        for k in ("fin_return", "fin_time"):
            assert np.isnan(bufs[k].cpu().numpy()).all(), (what, k)
        assert (bufs["fin_info"].cpu().numpy() == R.SENTINEL_INFO).all(), what
        return
    if w.contract.pool is not None:               # a restarted robot faces robot_theta0, exactly
        restarted = snap["rec"]["fin_count"] > 0
        assert H.bits_equal(got_st.rtheta[restarted], np.full(int(restarted.sum()), R.THETA0)), what
        assert H.bits_equal(got_st.rtheta[~restarted], np.zeros(int((~restarted).sum()))), what
    rec = bufs["state"].cpu().numpy().view(R.ROLL_DTYPE).reshape(w.E)
    for f in R.ROLL_FIELDS:
        bad = H.bit_mismatch(rec[f], snap["rec"][f])
        assert len(bad) == 0, (what, f, len(bad), "envs", _first(bad), rec[f][bad[0][0]], snap["rec"][f][bad[0][0]])
    for k in ("fin_return", "fin_time", "fin_info"):
        got = bufs[k].cpu().numpy()
        if k in null:                             # that part is off: its buffer keeps the sentinel, the others do not care
            assert (np.isnan(got) if k != "fin_info" else got == R.SENTINEL_INFO).all(), (what, k)
            continue
        bad = H.bit_mismatch(got, snap[k])
        assert len(bad) == 0, (what, k, len(bad), "(slot, env)", _first(bad), got[tuple(bad[0])], snap[k][tuple(bad[0])])
    if env.export_human_actions:
        bad = H.bit_mismatch(env.human_act.cpu().numpy(), w.human_act[n])
        assert len(bad) == 0, (what, "human_act", len(bad), _first(bad))


def _compare_step_recs(recs, w, steps, what):
    """recs: [len(steps), E, 3] float64 copies of the step record, steps: the 0-based step each one belongs to."""
    got = np.ascontiguousarray(recs).view(STEP_DTYPE).reshape(len(steps), w.E)
    for f in ("reward", "dmin", "done", "info", "hh_count"):
        bad = H.bit_mismatch(got[f], w.recs[f][list(steps)])
        assert len(bad) == 0, (what, "step record", f, len(bad), "(step, env)", [(steps[i], e) for i, e in _first(bad)])
    assert (got["reserved"] == 0).all(), what


def _run(path, w, tuning, null=()):
    """One path over the workload, compared after 1, 38 and 130 steps; returns the kernel family that ran last."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    kind, which, N = path
    assert N == w.N and _mode(path) == w.mode
    what = "%s %s N=%d set %s%s" % (kind, which, N, w.name, " without %s" % "/".join(null) if null else "")
    if kind == "step":
        select_step_kernel(which, tuning)
    elif kind == "given":
        tuning(pair_stream=which)
    elif kind == "sf-step":
        tuning(**SF_FORMS[which])
    elif kind == "sf-rollout":
        tuning(**(dict(rollout_fused=0) if which == "launches" else {}))
    else:
        tuning(**ROLLOUT_PATHS[which][2])
    env = _env(w)
    _attach(env, w, null)
    acts = torch.from_numpy(w.acts).to(env.device)
    if kind in ("rollout", "sf-rollout"):
        for a, b in SPLITS:
            # a quad path: the forced form is the one that went out
            launch(env, acts[a:b], forced_form(which) if kind == "rollout" else None)
            _compare(env, w, b, what, null)
            _compare_step_recs(env.step_rec.cpu().numpy()[None], w, [b - 1], what)
        return _hip.last_dispatch()
    gv = None if w.given is None else torch.from_numpy(w.given).to(env.device)
    recs = []
    for t in range(w.T):
        env.step(acts[t], given_v=None if gv is None else gv[t])
        recs.append(env.step_rec.clone())
        if t + 1 in R.CHECKPOINTS:
            _compare(env, w, t + 1, what, null)
    _compare_step_recs(torch.stack(recs).cpu().numpy(), w, list(range(w.T)), what)
    return _hip.last_dispatch()


def _expected_dispatch(path, w):
    kind, which, N = path
    if kind == "sf-step":
        return "env_step_kernel"
    if kind == "sf-rollout":                      # (the last launch is 92 steps long)
        return "env_step_loop_sf_kernel" if which == "loop" else "env_step_kernel"
    if kind == "given":
        # the streaming kernel keeps at most 128 table entries: one more and it must leave the step to env_step_kernel
        return "env_pair_kernel" if which and w.contract.disc_len <= 128 else "env_step_kernel"
    if kind == "rollout":
        return {"quad-rollout": "env_rollout_quad_kernel", "quad-rollout-split": "env_rollout_quad_kernel",
                "quad-rollout-wg4": "env_rollout_quad_kernel", "step-loop": "env_step_loop_kernel",
                "lp3-defer": "env_step_kernel", "unfused": "env_step_quad_kernel" if N == 5 else "env_step_kernel"}[which]
    return "env_step_quad_kernel" if which.startswith("quad") or (which == "auto" and N == 5) else "env_step_kernel"


def _cases():
    """(set, path): every set over every path; the social-force paths without latest-wins (SF_SETS)."""
    return [pytest.param(name, path, id="%s-%s" % (name, PATH_IDS[i])) for name in R.SETS for i, path in enumerate(PATHS)
            if name in SF_SETS or not path[0].startswith("sf")]


@pytest.mark.parametrize("name,path", _cases())
def test_accounting_matches_host_replay_bitwise(name, path, tuning):
    """One parameter set over one kernel path: the whole mcn_roll_rec, every fin_* slot (sentinels included), every step
    record and the env state with restarts, against the host replay.  The sets and what each pins: rollout_ref.SETS /
    REQUIRED.  table-128 / table-129: the streaming kernel runs with a 128-entry discount table and declines 129."""
    w = R.workload(name, path[2], _mode(path))
    R.check_events(name, w.events)
    ran = _run(path, w, tuning)
    assert ran == _expected_dispatch(path, w), (path, name, ran)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_parts_off(path, tuning):
    """mcn.h: "Any pointer may be NULL to disable that part."  fin_return, fin_time and fin_info NULL one at a time: the
    other two and the record are what they were (the replay's), the buffer that was left out keeps its sentinel.  Then a
    mcn_rollout with `state` NULL and no pool: state and step records are the oracle's (what roll = NULL gives) and no
    byte of any accounting buffer is written.  (All four bodies guard every store by its pointer -- read before run.)"""
    mode = _mode(path)
    w = R.workload("explorer-mid", path[2], mode)
    R.check_events(w.name, w.events)
    for part in ("fin_return", "fin_time", "fin_info"):
        _run(path, w, tuning, null=(part,))
    w = R.workload("no-pool", path[2], mode)
    R.check_events(w.name, w.events)
    _run(path, w, tuning, null=("state",))


# ---------------------------------------------------------------------------------------------------------------------
# social-force humans with the shipped parameters: the replay in lock step with the device
LOCKSTEP_FORMS = ((64, 0), (64, 1), (256, 0), (256, 1))          # (step_block, force_generic); the first sets the trace


def _lockstep_env(ls, tuning, block, generic):
    tuning(step_block=block, force_generic=generic)
    env = H.make_vec_env(ls.E, ls.N, robot_visible=ls.visible, **{"humans.policy": "socialforce"})
    assert env.human_policy_name == "socialforce"
    env._sf.strength, env._sf.range, env._sf.relaxation_rate = ls.params
    env.time_limit = ls.contract.time_limit
    H.upload(env, ls.st0)
    from oracle import cport
    want = H.oracle_cfg_for(env, cport.HUMANS_GIVEN)
    for name, _ in want._fields_:
        assert getattr(want, name) == getattr(ls.cfg, name), "the replay's oracle runs with another %s" % name
    w = R.Workload()                                  # what _attach reads of a workload
    w.set, w.scen, w.pool, w.first_cases, w.contract = ls.set, ls.scen, ls.pool, ls.first_cases, ls.contract
    _attach(env, w)
    return env


@pytest.mark.parametrize("visible", (False, True), ids=("invisible", "visible"))
@pytest.mark.parametrize("N", (5, 10))
@pytest.mark.parametrize("name", R.LOCKSTEP_SETS)
def test_social_force_accounting_in_lock_step(name, N, visible, tuning):
    """Shipped parameters (4, 0.2, 2), 130 steps of 251 envs.  Per step: the host computes the robots' actions from ITS
    state (rollout_ref._simulate's rule) and uploads them; one mcn_env_step_sf; the device's human_act is held to the
    restatement on the host state within 8 * 2^-52 * M and goes into Replay.step as given velocities; the step record is
    compared bitwise; at rollout_ref.CHECKPOINTS the whole state, the mcn_roll_rec and the sentinel-filled fin_* arrays
    too.  The first form (compile-time N, block 64) runs in lock step and leaves its human_act trace; force_generic and
    block 256 must reproduce the trace, every step record and every checkpoint bitwise -- all forms perform the same IEEE
    operations in the same order (contraction off), so a difference is a finding, not a tolerance to widen."""
    torch = need_gpu()
    from modelcrowdnav_amd import _hip
    from tests.rollout_harness import assert_same_bytes, snapshot
    ls = R.LockStep(name, N, visible)
    w = R.Workload()
    w.E, w.contract, w.snaps, w.human_act = ls.E, ls.contract, {}, {}
    block, generic = LOCKSTEP_FORMS[0]
    env = _lockstep_env(ls, tuning, block, generic)
    what = "lock step %s N=%d visible=%d" % (name, N, visible)
    acts, trace, recs, snaps, worst = [], [], [], {}, 0.0
    for t in range(ls.T):
        a = ls.actions()
        want, mag = ls.restatement()
        env.step(torch.from_numpy(a).to(env.device))
        assert _hip.last_dispatch() == "env_step_kernel"
        hact = env.human_act.cpu().numpy()
        tol = SF_TOL * mag[..., None]
        err = np.abs(hact - want)
        assert np.isfinite(hact).all() and (err <= tol).all(), (what, "human_act at step", t, np.argwhere(~(err <= tol))[:4].tolist())
        worst = max(worst, float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0))))
        out = ls.advance(a, hact)
        rec = env.step_rec.cpu().numpy()
        got = np.ascontiguousarray(rec).view(STEP_DTYPE).reshape(ls.E)
        for f in ("reward", "dmin", "done", "info", "hh_count"):
            bad = H.bit_mismatch(got[f], out[f])
            assert len(bad) == 0, (what, "step record", f, "step", t, "envs", _first(bad))
        acts.append(a); trace.append(hact); recs.append(rec)
        if t + 1 in R.CHECKPOINTS:
            w.snaps[t + 1] = (ls.st.copy(), ls.rep.snapshot())
            w.human_act[t + 1] = hact
            _compare(env, w, t + 1, what)
            snaps[t + 1] = snapshot(env)
    events = ls.events()
    missing = [k for k in R.lockstep_required(name) if events.get(k, 0) == 0]
    assert not missing, "%s: the replay never reached %s (%s)" % (what, missing, events)
    print("%s: largest error / tolerance %.4f, events %s" % (what, worst, events))
    acts_d = torch.from_numpy(np.stack(acts)).to(env.device)
    for block, generic in LOCKSTEP_FORMS[1:]:
        env = _lockstep_env(ls, tuning, block, generic)
        for t in range(ls.T):
            env.step(acts_d[t])
            bad = H.bit_mismatch(env.human_act.cpu().numpy(), trace[t])
            assert len(bad) == 0, (what, "block", block, "generic", generic, "human_act at step", t, _first(bad))
            assert np.array_equal(env.step_rec.cpu().numpy().view(np.uint8), recs[t].view(np.uint8)), (what, block, generic, t)
            if t + 1 in R.CHECKPOINTS:
                assert_same_bytes(snapshot(env), snaps[t + 1], (what, block, generic, t + 1))
