"""Host replay of the mcn_rollout contract (include/mcn.h) -- the bookkeeping that turns a stream of env steps into what
Explorer.run_k_episodes reports (crowd_nav/utils/explorer.py:88-99,124) plus the in-kernel restart from a scenario pool.

Plain Python floats / ints per env on top of the C oracle's step (oracle.cport.env_step); written from the header and the
reference's explorer, not from the kernels, so that the four device copies of this block (env_step.hip, env_step_quad.hip,
env_rollout_quad.hip, env_pair.hip) have one independent yardstick.  A Python `a + b * c` on floats is two IEEE roundings,
which is what the library computes (it is built with -ffp-contract=off).

  Contract   the scalar fields of mcn_rollout + the host copy of the pool
  Replay     per-env records, the fin_* arrays (sentinel-filled: a stray or a missing store shows), event counters;
             account() is one env's bookkeeping for one step record, step() drives the oracle and replays the restarts
  Workload   the inputs of tests/test_rollout_accounting_gpu.py: parameter sets, action sequences computed on the host
             from the oracle's state, the replay's records per step and its snapshots at the launch boundaries
"""
import collections
import functools
import zlib

import numpy as np

from oracle import cport

ROLL_DTYPE = np.dtype([("ep_return", "f8"), ("ep_steps", "i4"), ("fin_count", "i4"), ("next_case", "i4"),
                       ("danger_count", "i4"), ("danger_dist_sum", "f8")])            # mcn_roll_rec
ROLL_FIELDS = ROLL_DTYPE.names
SENTINEL_INFO = 0xFF
PX, PY, GX, GY, VX, VY, TH, RAD, VPREF = range(9)          # scenario columns (modelcrowdnav_amd/envs/scenarios.py)


def disc_table(gamma, time_step, v_pref, length):
    """explorer.py:124's factors, as VecCrowdSim.attach_rollout tabulates them."""
    return np.array([pow(gamma, t * time_step * v_pref) for t in range(length)], np.float64)


def pool_arrays(scen, with_velocities=True):
    """[P,N,9] host scenarios -> the pool arrays of mcn_rollout (pool_hvel None: restarted humans stand still)."""
    scen = np.asarray(scen, np.float64)
    return dict(hpos=scen[:, :, [PX, PY]].copy(), hgoal=scen[:, :, [GX, GY]].copy(), hrad=scen[:, :, RAD].copy(),
                hvpref=scen[:, :, VPREF].copy(), hvel=scen[:, :, [VX, VY]].copy() if with_velocities else None)


class Contract(object):
    """mcn_rollout as the host sees it."""

    def __init__(self, disc, time_limit, fin_slots=1, danger_episodes=0, danger_short_from=0, pool=None, case_stride=0,
                 robot_start=(0.0, -4.0), robot_goal=(0.0, 4.0), robot_theta0=np.pi / 2, disc_len=None):
        self.disc = [float(x) for x in disc]
        self.disc_len = len(self.disc) if disc_len is None else int(disc_len)
        assert 1 <= self.disc_len <= len(self.disc) and fin_slots >= 1
        self.time_limit = float(time_limit)
        self.fin_slots, self.danger_episodes, self.danger_short_from = int(fin_slots), int(danger_episodes), int(danger_short_from)
        self.pool = pool
        self.pool_size = 0 if pool is None else int(pool["hpos"].shape[0])
        self.case_stride = int(case_stride)
        assert pool is None or 0 <= self.case_stride < self.pool_size
        self.robot_start, self.robot_goal, self.robot_theta0 = tuple(robot_start), tuple(robot_goal), float(robot_theta0)


class Replay(object):
    def __init__(self, E, contract, first_cases=None):
        c = self.c = contract
        self.E = E
        self.rec = np.zeros(E, ROLL_DTYPE)
        if c.pool is not None:
            self.rec["next_case"] = (np.arange(E) if first_cases is None else np.asarray(first_cases)) % c.pool_size
        self.fin_return = np.full((c.fin_slots, E), np.nan)
        self.fin_time = np.full((c.fin_slots, E), np.nan)
        self.fin_info = np.full((c.fin_slots, E), SENTINEL_INFO, np.uint8)
        self.events = collections.Counter()
        self.first = {}                  # env -> its first finished episode (return, time, info)
        self.last_danger = np.zeros(E, bool)     # a Danger step in episode number danger_episodes - 1, counted or not

    # ------------------------------------------------------------------ one env, one step record
    def account(self, e, reward, done, info, dmin, clock):
        """Book one step of env e: `clock` is the env's time after the step.  Returns the pool case the env restarts
        from, or None (not done, or no pool)."""
        c, r, ev = self.c, self.rec, self.events
        ep_steps, fin_count = int(r["ep_steps"][e]), int(r["fin_count"][e])
        reward, dmin = float(reward), float(dmin)
        # "too close" (explorer.py:88-90), over the env's first danger_episodes episodes only
        if info == cport.INFO_DANGER:
            short = c.danger_short_from > 0 and e >= c.danger_short_from - 1
            if c.danger_episodes > 0 and fin_count == c.danger_episodes - 1:
                self.last_danger[e] = True
            if c.danger_episodes <= 0 or fin_count < c.danger_episodes - (1 if short else 0):
                r["danger_count"][e] += 1
                r["danger_dist_sum"][e] = float(r["danger_dist_sum"][e]) + dmin
                ev["danger_counted"] += 1
                if c.danger_episodes > 0 and c.danger_short_from > 0 and fin_count == c.danger_episodes - 1:
                    ev["long_side_counted"] += 1           # an env below danger_short_from - 1 in its last counted episode
                    if e == c.danger_short_from - 2:
                        ev["below_boundary_counted"] += 1  # ... the env next to the boundary itself
            else:
                ev["danger_gated"] += 1
                if short and fin_count == c.danger_episodes - 1:
                    ev["short_side_gated"] += 1            # the episode an env from danger_short_from - 1 on leaves out
                    if e == c.danger_short_from - 1:
                        ev["boundary_gated"] += 1          # ... the boundary env itself: `e >= sf` would count this step
        # discounted return (explorer.py:124): the table entry of this step, the last one beyond the table
        idx = min(ep_steps, c.disc_len - 1)
        if idx != ep_steps:
            ev["clamped"] += 1
        if idx >= 64 and reward != 0.0:
            ev["disc_index_ge64"] += 1
        prod = c.disc[idx] * reward
        ret = float(r["ep_return"][e]) + prod
        if not done:
            r["ep_return"][e], r["ep_steps"][e] = ret, ep_steps + 1
            return None
        ev[{cport.INFO_REACHGOAL: "reach", cport.INFO_COLLISION: "collision", cport.INFO_TIMEOUT: "timeout"}[int(info)]] += 1
        when = c.time_limit if info == cport.INFO_TIMEOUT else float(clock)                   # explorer.py:98-106
        self.first.setdefault(e, (ret, when, int(info)))
        if c.fin_slots == 1:
            slot = 0
            if fin_count == 0:
                ev["recorded"] += 1
            elif (self.fin_return[0, e], self.fin_time[0, e], int(self.fin_info[0, e])) != (ret, when, int(info)):
                ev["overwritten"] += 1             # the slot's bytes change: keeping the earlier record would show
            else:
                ev["overwritten_same"] += 1
        elif fin_count < c.fin_slots:
            slot = fin_count
            ev["recorded"] += 1
        else:
            slot = None
            ev["dropped"] += 1
        if slot is not None:
            self.fin_return[slot, e] = ret
            self.fin_time[slot, e] = when
            self.fin_info[slot, e] = info
        r["fin_count"][e], r["ep_return"][e], r["ep_steps"][e] = fin_count + 1, 0.0, 0
        if c.pool is None:
            return None
        case = int(r["next_case"][e])
        nxt = case + c.case_stride
        if nxt >= c.pool_size:
            nxt -= c.pool_size
            ev["wrap"] += 1
        r["next_case"][e] = nxt
        return case

    # ------------------------------------------------------------------ the env state
    def restart(self, st, e, case):
        """Env e of the oracle state back to the start of pool case `case` (mcn.h: mcn_rollout)."""
        c, p = self.c, self.c.pool
        st.hpx[e], st.hpy[e] = p["hpos"][case, :, 0], p["hpos"][case, :, 1]
        st.hgx[e], st.hgy[e] = p["hgoal"][case, :, 0], p["hgoal"][case, :, 1]
        st.hr[e], st.hvpref[e] = p["hrad"][case], p["hvpref"][case]
        if p["hvel"] is None:
            st.hvx[e], st.hvy[e] = 0.0, 0.0
        else:
            st.hvx[e], st.hvy[e] = p["hvel"][case, :, 0], p["hvel"][case, :, 1]
            if np.any(p["hvel"][case] != 0):
                self.events["restart_moving"] += 1
        st.human_times[e] = 0.0
        st.rpx[e], st.rpy[e] = c.robot_start
        st.rgx[e], st.rgy[e] = c.robot_goal
        st.rvx[e], st.rvy[e] = 0.0, 0.0
        st.rtheta[e] = c.robot_theta0
        st.gtime[e] = 0.0
        self.events["restart"] += 1

    def step(self, cfg, st, ax, ay, given_v=None):
        """One oracle step of all envs, booked; finished envs restart from the pool.  Returns the oracle's outputs."""
        out = cport.env_step(cfg, st, ax, ay, update=True, given_v=given_v)
        for e in range(self.E):
            case = self.account(e, out["reward"][e], int(out["done"][e]), int(out["info"][e]), out["dmin"][e], st.gtime[e])
            if case is not None:
                self.restart(st, e, case)
        return out

    def snapshot(self):
        return dict(rec=self.rec.copy(), fin_return=self.fin_return.copy(), fin_time=self.fin_time.copy(),
                    fin_info=self.fin_info.copy())


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own loop on one case (explorer.py:62-125 with the exact goal-seeking robot)

def host_goal_seeking(st, speed=0.6):
    """tests/rollout_harness.py goal_seeking on the host: +-speed along each axis by the sign of the remaining goal
    offset, 0 inside a 0.2 band.  Exact on any IEEE machine."""
    dx, dy = st.rgx - st.rpx, st.rgy - st.rpy
    ax = np.where(dx > 0.2, speed, 0.0) - np.where(dx < -0.2, speed, 0.0)
    ay = np.where(dy > 0.2, speed, 0.0) - np.where(dy < -0.2, speed, 0.0)
    return ax, ay


def oracle_episode(scen, gamma=0.9):
    st = cport.EnvState(1, scen.shape[0])
    st.hpx[0], st.hpy[0], st.hgx[0], st.hgy[0] = scen[:, 0], scen[:, 1], scen[:, 2], scen[:, 3]
    st.hr[0], st.hvpref[0] = scen[:, 7], scen[:, 8]
    st.rpy[0], st.rgy[0], st.rr[0] = -4.0, 4.0, 0.3
    cfg = cport.default_cfg()
    rewards, too_close, min_dist = [], 0, 0.0
    while True:
        dx, dy = st.rgx[0] - st.rpx[0], st.rgy[0] - st.rpy[0]
        ax = 0.6 if dx > 0.2 else (-0.6 if dx < -0.2 else 0.0)
        ay = 0.6 if dy > 0.2 else (-0.6 if dy < -0.2 else 0.0)
        out = cport.env_step(cfg, st, np.array([ax]), np.array([ay]))
        rewards.append(float(out["reward"][0]))
        if out["info"][0] == cport.INFO_DANGER:                      # explorer.py:88-90
            too_close += 1
            min_dist += float(out["dmin"][0])
        if out["done"][0]:
            tm = 25.0 if out["info"][0] == cport.INFO_TIMEOUT else float(st.gtime[0])
            ret = sum([pow(gamma, t * 0.25 * 1.0) * r for t, r in enumerate(rewards)])
            return ret, int(out["info"][0]), tm, too_close, min_dist


def initial_state(pool, cases, robot_radius=0.3, robot_start=(0.0, -4.0), robot_goal=(0.0, 4.0)):
    """Oracle state of len(cases) envs at the start of those pool cases (robot heading 0, clock 0)."""
    cases = np.asarray(cases)
    st = cport.EnvState(len(cases), pool["hpos"].shape[1])
    st.hpx[:], st.hpy[:] = pool["hpos"][cases, :, 0], pool["hpos"][cases, :, 1]
    st.hgx[:], st.hgy[:] = pool["hgoal"][cases, :, 0], pool["hgoal"][cases, :, 1]
    st.hr[:], st.hvpref[:] = pool["hrad"][cases], pool["hvpref"][cases]
    if pool["hvel"] is not None:
        st.hvx[:], st.hvy[:] = pool["hvel"][cases, :, 0], pool["hvel"][cases, :, 1]
    st.rpx[:], st.rpy[:] = robot_start
    st.rgx[:], st.rgy[:] = robot_goal
    st.rr[:] = robot_radius
    return st


# ---------------------------------------------------------------------------------------------------------------------
# the workloads of tests/test_rollout_accounting_gpu.py

E_ACC, T_ACC = 251, 130                 # 251 is prime: no kernel family's envs-per-wavefront divides it
THETA0 = 0.625                          # robot_theta0 of every set: non-zero, dyadic, not the robot's initial heading (0)
SHORT_MID = 125                         # danger_short_from = "mid": the boundary env danger_short_from - 1 is chosen per
                                        # workload, as near to this as the replay allows (see workload())
CHECKPOINTS = (1, 38, T_ACC)            # steps after which everything is compared: the launches are 1 + 37 + 92 steps

# name: what mcn_rollout is given.  pool: "host" ([P,N,9] with velocities), "device" (dict: pool_hvel NULL), None
SETS = collections.OrderedDict([
    ("explorer-mid",   dict(fin_slots=3, danger_episodes=2, danger_short_from="mid", pool="host", P=16, stride=3, shift=5)),
    ("explorer-first", dict(fin_slots=3, danger_episodes=2, danger_short_from=1, pool="host", P=16, stride=3, shift=5)),
    ("explorer-last",  dict(fin_slots=3, danger_episodes=2, danger_short_from=E_ACC, pool="host", P=16, stride=3, shift=5)),
    ("explorer-none",  dict(fin_slots=3, danger_episodes=1, danger_short_from=1, pool="host", P=16, stride=3, shift=5)),
    ("latest-wins",    dict(fin_slots=1, danger_episodes=0, danger_short_from=0, pool="host", P=1, stride=0, shift=0)),
    ("device-pool",    dict(fin_slots=2, danger_episodes=0, danger_short_from=0, pool="device", P=16, stride=15, shift=0)),
    ("no-pool",        dict(fin_slots=2, danger_episodes=0, danger_short_from=0, pool=None, P=16, stride=0, shift=0)),
    ("short-table",    dict(fin_slots=3, danger_episodes=2, danger_short_from="mid", pool="host", P=16, stride=3, shift=5,
                            disc_len=5)),
    # time_limit 31.5 -> a 128-entry table, the streaming kernel's limit; 31.75 -> 129 entries: it must decline.  The
    # goal-seeking robots walk at 0.375 here, so that rewards are earned at step indices >= 64
    ("table-128",      dict(fin_slots=3, danger_episodes=2, danger_short_from="mid", pool="host", P=16, stride=3, shift=5,
                            time_limit=31.5, speed=0.375, wait=30)),
    ("table-129",      dict(fin_slots=3, danger_episodes=2, danger_short_from="mid", pool="host", P=16, stride=3, shift=5,
                            time_limit=31.75, speed=0.375, wait=30)),
])

# what the replay of each set must have passed through (conditions on the replay, not on the kernels)
_TERMINALS = ("reach", "collision", "timeout")
_EXPLORER = _TERMINALS + ("danger_counted", "danger_gated", "dropped", "wrap", "restart_moving")
# both sides of danger_short_from - 1, AT the boundary: env sf - 1 leaves a Danger step of its last episode out, env sf - 2
# counts one of the same episode number
_BOUNDARY = ("short_side_gated", "long_side_counted", "boundary_gated", "below_boundary_counted")
REQUIRED = {
    "explorer-mid": _EXPLORER + _BOUNDARY,
    "explorer-first": _EXPLORER + ("short_side_gated",),
    "explorer-last": _EXPLORER + ("short_side_gated", "long_side_counted", "boundary_gated"),
    "explorer-none": _TERMINALS + ("danger_gated", "dropped", "wrap", "restart_moving"),
    "latest-wins": _TERMINALS + ("danger_counted", "overwritten", "first_wins_differs", "restart"),
    "device-pool": _TERMINALS + ("danger_counted", "dropped", "wrap", "restart"),
    "no-pool": _TERMINALS + ("danger_counted", "dropped"),
    "short-table": _EXPLORER + _BOUNDARY + ("clamped",),
    # (the slow robots of these two finish too few episodes to overflow three slots: "dropped" is not theirs to reach)
    "table-128": tuple(k for k in _EXPLORER if k != "dropped") + _BOUNDARY + ("disc_index_ge64",),
    "table-129": tuple(k for k in _EXPLORER if k != "dropped") + _BOUNDARY + ("disc_index_ge64",),
}
FORBIDDEN = {"explorer-none": ("danger_counted",), "no-pool": ("restart",), "device-pool": ("restart_moving",)}


def check_events(name, events):
    missing = [k for k in REQUIRED[name] if events.get(k, 0) == 0]
    extra = [k for k in FORBIDDEN.get(name, ()) if events.get(k, 0) != 0]
    assert not missing and not extra, "%s: the replay never reached %s, reached %s (%s)" % (name, missing, extra, dict(events))


class Workload(object):
    pass


def _group_sizes(N):
    """Envs per wavefront / workgroup of the kernel families at N humans (quad, lane-per-human 64 and 256, streaming)."""
    return sorted({g for g in (64 // (4 * N), 64 // N, 4 * (64 // N)) if g > 1})


@functools.lru_cache(maxsize=None)
def workload(name, N, mode):
    """_simulate() with the set's danger_short_from.  "mid" is settled here from a first replay (the gate has no say in
    what the envs do): the boundary env sf - 1 nearest to SHORT_MID such that it AND env sf - 2 meet a Danger step in
    their last counted episode -- so the run pins the boundary itself -- and that does not open an env group of any
    kernel family (the boundary falls inside a wavefront's envs)."""
    sf = SETS[name]["danger_short_from"]
    if sf == E_ACC:
        # the last env is the only one shortened: the pool walk is shifted until it meets a Danger step in its last
        # counted episode (the set's own shift first)
        for shift in range(SETS[name]["shift"], SETS[name]["shift"] + SETS[name]["P"]):
            w = _simulate(name, N, mode, sf, shift)
            if w.last_danger[E_ACC - 1]:
                return w
        raise AssertionError("%s N=%d %s: the last env never meets a Danger step in its second episode" % (name, N, mode))
    if sf != "mid":
        return _simulate(name, N, mode, sf)
    flag = _simulate(name, N, mode, 0).last_danger
    ok = [e for e in range(2, E_ACC - 1) if flag[e] and flag[e - 1] and all(e % g for g in _group_sizes(N))]
    assert ok, "%s N=%d %s: no two neighbouring envs meet a Danger step in their second episode" % (name, N, mode)
    return _simulate(name, N, mode, min(ok, key=lambda e: abs(e - SHORT_MID)) + 1)


SF_PARAMS = (0.0, 0.2, 2.0)             # mode "sf": strength 0 -- every m = 0 * exp(..) is exactly 0, the replay bit-exact
SF_SHIPPED = (4.0, 0.2, 2.0)            # the lock-step runs (LockStep): the device's own velocities go into the replay


def _setup(name, N, mode, short_from, shift=None, visible=False):
    """The pool, the contract, the replay, the oracle's state and cfg of parameter set `name`, and the set's random
    stream (seeded by name, N and mode; the pool's start velocities are its first draws)."""
    from modelcrowdnav_amd.envs import scenarios as S
    s = SETS[name]
    E, P = E_ACC, s["P"]
    time_limit = s.get("time_limit", 25.0)
    rng = np.random.RandomState(zlib.crc32(("%s/%d/%s" % (name, N, mode)).encode()))
    scen = S.scenario_pool(S.ScenarioSpec(), "test", range(P), N, "circle_crossing")
    if s["pool"] == "host":
        v = rng.randint(1, 9, (P, N, 2)) * rng.choice([-1.0, 1.0], (P, N, 2)) / 16.0      # non-zero, dyadic
        scen[:, :, VX], scen[:, :, VY] = v[..., 0], v[..., 1]
    pool = pool_arrays(scen, with_velocities=s["pool"] == "host")
    horizon = int(round(time_limit / 0.25)) + 2                                           # VecCrowdSim.attach_rollout
    con = Contract(disc_table(0.9, 0.25, 1.0, horizon), time_limit, fin_slots=s["fin_slots"],
                   danger_episodes=s["danger_episodes"], danger_short_from=short_from,
                   pool=pool if s["pool"] else None, case_stride=s["stride"], robot_theta0=THETA0,
                   disc_len=s.get("disc_len"))
    start = np.arange(E) % P
    first = (start + (s["shift"] if shift is None else shift)) % P
    rep = Replay(E, con, first_cases=first)
    st = initial_state(pool, start)
    full = mode != "given"              # overlap count and first arrivals: all but the streaming kernel's lean step
    cfg = cport.default_cfg(time_limit=time_limit, human_policy=cport.HUMANS_ORCA if mode == "orca" else cport.HUMANS_GIVEN,
                            count_hh=1 if full else 0, track_human_times=1 if full else 0,
                            robot_visible=1 if visible else 0)
    return s, rng, scen, pool, con, first, rep, st, cfg


def _robot_actions(s, st, rep, rng):
    """[E, 2] actions of one step from the ORACLE's state and the replay's counters: _simulate's rule."""
    E = st.E
    role = (np.arange(E) + 2) % 3                  # (the last env, the one danger_short_from = E shortens, walks at once)
    seeker = role != 2
    late = role == 1                    # these stand still for the first `wait` steps of every episode
    gx, gy = host_goal_seeking(st, s.get("speed", 0.6))
    wait = np.where(late, s.get("wait", 40), 0) + 2 * (rep.rec["fin_count"] % 5)
    hold = rep.rec["ep_steps"] < wait
    gx, gy = np.where(hold, 0.0, gx), np.where(hold, 0.0, gy)
    acts = np.zeros((E, 2))
    acts[:, 0] = np.where(seeker, gx, rng.randint(-16, 17, E) / 16.0)
    acts[:, 1] = np.where(seeker, gy, rng.randint(-16, 17, E) / 16.0)
    return acts


def sf_velocities(st, params, visible, dt=0.25):
    """tests/social_force_ref.py on the oracle's state: ([E, N, 2] velocities, [E, N] magnitudes)."""
    from tests import social_force_ref as SF
    return SF.batch_velocities(np.stack([st.hpx, st.hpy], -1), np.stack([st.hvx, st.hvy], -1),
                               np.stack([st.hgx, st.hgy], -1), st.hr, st.hvpref, params[0], params[1], params[2], dt,
                               np.stack([st.rpx, st.rpy], -1) if visible else None, st.rr if visible else None)


def _simulate(name, N, mode, short_from, shift=None):
    """The inputs and the replay of parameter set `name` for N humans, mode 'orca' (ORCA humans, overlap count, first
    arrivals), 'given' (velocities handed in, neither of the two) or 'sf' (social-force humans with SF_PARAMS: each
    step's velocities are the restatement's on the oracle's state, handed to the oracle's given-velocity step with the
    overlap count and first arrivals on).  Two envs in three walk to the goal by the exact
    goal-seeking rule evaluated on the ORACLE's state -- every other one of them only after it has let the crowd cross
    for the first 40 steps of the episode, so that goals are reached in crowds of 10 too; the third takes random dyadic
    actions.  Every seeker also waits two more steps per episode it has finished (0, 2, .. 8, then again from 0), so that
    an env that restarts the same case -- a pool of one -- does not repeat its episode byte for byte.  Given velocities
    point at the human's goal, rounded to sixteenths, plus dyadic noise -- also computed from the oracle's state."""
    s, rng, scen, pool, con, first, rep, st, cfg = _setup(name, N, mode, short_from, shift)
    E, T = E_ACC, T_ACC
    w = Workload()
    w.name, w.N, w.mode, w.E, w.T, w.set, w.contract, w.cfg = name, N, mode, E, T, s, con, cfg
    w.scen, w.pool, w.first_cases, w.st0 = scen, pool, first, st.copy()
    w.acts = np.zeros((T, E, 2))
    w.given = np.zeros((T, E, N, 2)) if mode == "given" else None
    w.recs = {k: [] for k in ("reward", "dmin", "done", "info", "hh_count")}
    w.human_act, w.snaps = {}, {}
    for t in range(T):
        w.acts[t] = _robot_actions(s, st, rep, rng)
        gv = None
        if mode == "given":
            d = np.stack([st.hgx - st.hpx, st.hgy - st.hpy], -1)
            n = np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9)
            gv = w.given[t] = np.round(d / n * 12.0) / 16.0 + rng.randint(-3, 4, (E, N, 2)) / 16.0
        elif mode == "sf":
            gv = sf_velocities(st, SF_PARAMS, False)[0]
        out = rep.step(cfg, st, w.acts[t, :, 0].copy(), w.acts[t, :, 1].copy(), given_v=gv)
        for k in w.recs:
            w.recs[k].append(out[k].copy())
        if t + 1 in CHECKPOINTS:
            w.snaps[t + 1] = (st.copy(), rep.snapshot())
            w.human_act[t + 1] = out["human_act"].copy()
    w.recs = {k: np.stack(v) for k, v in w.recs.items()}
    _close_events(w, rep)
    return w


def _close_events(w, rep):
    con = rep.c
    w.events = dict(rep.events)
    w.last_danger = rep.last_danger.copy()
    # envs whose single slot would hold other bytes had it kept the FIRST episode (fin_slots == 1 only)
    if con.fin_slots == 1:
        w.events["first_wins_differs"] = sum(1 for e, f in rep.first.items()
                                             if f != (rep.fin_return[0, e], rep.fin_time[0, e], int(rep.fin_info[0, e])))
    w.events["max_fin_count"] = int(rep.rec["fin_count"].max())


# ---------------------------------------------------------------------------------------------------------------------
# social-force humans with the shipped parameters: the replay in lock step with the device

# the boundary entries that only danger_short_from = "mid" / E can reach
_MID_ONLY = ("long_side_counted", "boundary_gated", "below_boundary_counted")
LOCKSTEP_SETS = ("explorer-first", "latest-wins")


def lockstep_required(name):
    return tuple(k for k in REQUIRED[name] if k not in _MID_ONLY)


class LockStep(object):
    """Parameter set `name` with social-force humans of SF_SHIPPED strength, one step at a time.  exp on the device may
    differ from the host's by an ulp and 130 steps amplify that, so the host cannot run ahead: per step actions() gives
    the robots' actions from the HOST state (_simulate's rule), restatement() the definition's velocities on it, and
    advance() takes the velocities the humans actually chose (the device's, or the restatement's for a forecast) into
    Replay.step as given velocities."""

    def __init__(self, name, N, visible, params=SF_SHIPPED):
        assert name in LOCKSTEP_SETS
        (self.set, self.rng, self.scen, self.pool, self.contract, self.first_cases, self.rep, self.st,
         self.cfg) = _setup(name, N, "sf-lockstep", SETS[name]["danger_short_from"], visible=visible)
        self.name, self.N, self.E, self.T, self.visible, self.params = name, N, E_ACC, T_ACC, bool(visible), params
        self.st0 = self.st.copy()
        self.t = 0

    def actions(self):
        return _robot_actions(self.set, self.st, self.rep, self.rng)

    def restatement(self):
        return sf_velocities(self.st, self.params, self.visible)

    def advance(self, acts, human_act):
        out = self.rep.step(self.cfg, self.st, acts[:, 0].copy(), acts[:, 1].copy(),
                            given_v=np.ascontiguousarray(human_act, np.float64))
        self.t += 1
        return out

    def events(self):
        w = Workload()
        _close_events(w, self.rep)
        return w.events


@functools.lru_cache(maxsize=None)
def lockstep_forecast(name, N, visible):
    """The events of a LockStep run that takes the restatement's own velocities (libm's exp): what the device run, which
    differs by ulps of exp only, is expected to reach."""
    ls = LockStep(name, N, visible)
    for _ in range(ls.T):
        a = ls.actions()
        ls.advance(a, ls.restatement()[0])
    return ls.events()
