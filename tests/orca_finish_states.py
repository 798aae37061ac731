"""Edge and boundary batches for mcn_orca_finish (orca_finish.hip), in the layout of tests/orca_finish_ref.py.

Edge batches (edge_batch, edge_replay): the existing dyadic constructions converted to the all-ORCA simulation -- every
agent at its plain radius, sim_vel = float32(rvel, hvel), human_times 0, clocks as they are:
  closed_loop_states.edge_batch(N, max_neighbors, neighbor_dist)   341 envs, the robot (agent 0) in the middle
  edge_states.edge_batch(N, True, variant), N <= 10 only (its rings hold 12 points): the 208 untranslated envs, human 0
                  in the middle; they convert directly because here every human sees the robot
  lp2-tangent     16 envs around seeded-search finds of a two-agent state whose single half-plane is tangent to the
                  speed disc (disc_zero_lp2: the one counter the converted batches do not reach); radius 0.3125, the
                  agent a human in even envs and the robot in odd ones, everybody else out of range.  With
                  max_neighbors 0 there is no half-plane at all, so that config cannot reach it (REQUIRED below).
CONFIGS are (max_neighbors, neighbor_dist, time_horizon, time_step); every (N, config) of HUMAN_COUNTS x CONFIGS is run.

Boundary batches (boundary_batch): one named case per env for the float64 half of the kernel -- the strict arrival test
on the position from before the step, the caller's float64 position on the first step, the preferred velocity's
n > 1, human_times that are == 0 or not, the float64 clock, the select byte, float64 radius against float32 radius.
Radius 0.3125, offsets (0.1875, 0.25): |offset| == 0.3125 exactly.
"""
import functools

import numpy as np

from oracle import cport
from tests import closed_loop_states as CS
from tests import edge_states as ES
from tests import orca_finish_ref as R

f32, f64 = np.float32, np.float64

HUMAN_COUNTS = (1, 2, 3, 5, 7, 10, 15, 20, 21, 31, 32)        # A = N + 1 = 2 3 4 6 8 11 16 21 22 32 33
T_EDGE = 6
# (max_neighbors, neighbor_dist, time_horizon, time_step)
CONFIGS = ((10, 10.0, 5.0, 0.25), (3, 1.5, 2.0, 0.1), (2, 10.0, 5.0, 0.25), (0, 10.0, 5.0, 0.25))
DEFAULT = 0
RB = 0.3125
FAR = 64.0

# What each config's batches, summed over HUMAN_COUNTS, must reach: every counter of the oracle.  With max_neighbors 0 the
# oracle takes no neighbour at all (no distance is compared, no half-plane built), so only the bare speed disc's
# pref_on_disc can happen; that config is there for nl_cap = 1 and the empty solve.
REQUIRED = tuple(cport.EDGE_NAMES if mn > 0 else ("pref_on_disc",) for mn, nd, th, dt in CONFIGS)


def params(config):
    mn, nd, th, dt = CONFIGS[config]
    return dict(max_neighbors=mn, neighbor_dist=nd, time_horizon=th, time_step=dt)


def from_env_state(st, rvpref):
    """cport.EnvState -> (orca_finish_ref state, sim_vel): plain radii, pending times."""
    E = st.E
    out = dict(hpos=np.stack([st.hpx, st.hpy], -1), hgoal=np.stack([st.hgx, st.hgy], -1), hrad=st.hr, hvpref=st.hvpref,
               rpos=np.stack([st.rpx, st.rpy], -1), rgoal=np.stack([st.rgx, st.rgy], -1), rrad=st.rr,
               rvpref=np.broadcast_to(np.asarray(rvpref, f64), (E,)), gtime=st.gtime, human_times=np.zeros((E, st.N)))
    vel = np.concatenate([np.stack([st.rvx, st.rvy], -1)[:, None], np.stack([st.hvx, st.hvy], -1)], 1).astype(f32)
    return {k: np.ascontiguousarray(v, f64) for k, v in out.items()}, np.ascontiguousarray(vel)


@functools.lru_cache(maxsize=None)
def _search_lp2_tangent(nd, th, dt, want=4):
    """Two-agent dyadic states (agent, one neighbour, radius RB) whose solve counts disc_zero_lp2 under (nd, th, dt):
    a seeded search, about one random state in 3000 qualifies.  (pos, vel, v_pref, pref, other pos, other vel) each."""
    rng = np.random.RandomState(7)
    g = lambda lo, hi, step: rng.randint(int(round(lo / step)), int(round(hi / step)) + 1) * step
    found = []
    cport.edge_counts(reset=True)
    for _ in range(200000):
        pos, vel = (g(-2, 2, 1 / 8), g(-2, 2, 1 / 8)), (g(-1, 1, 1 / 16), g(-1, 1, 1 / 16))
        pref = (g(-1, 1, 1 / 8), g(-1, 1, 1 / 8))
        vp = float(rng.choice(ES.VPREF))
        op, ov = (pos[0] + g(-1.5, 1.5, 1 / 8), pos[1] + g(-1.5, 1.5, 1 / 8)), (g(-1, 1, 1 / 16), g(-1, 1, 1 / 16))
        if pref[0] ** 2 + pref[1] ** 2 > 1:             # the kernel would normalise it: keep goal - pos == pref
            continue
        cport.orca_agent(pos, vel, RB, vp, pref, [op], [ov], [RB], neighbor_dist=nd, max_neighbors=10, time_horizon=th,
                         time_step=f32(dt))
        if cport.edge_counts(reset=True)["disc_zero_lp2"]:
            found.append((pos, vel, vp, pref, op, ov))
            if len(found) == want:
                break
    return tuple(found)


def _lp2_tangent_block(N, nd, th, dt):
    """BLOCK envs: find i = e mod 4; the agent is human slot (e // 2) mod N in even envs (the robot its neighbour) and
    the robot in odd envs (that human its neighbour); the other humans stand on their goals FAR apart."""
    found = _search_lp2_tangent(float(nd), float(th), float(dt))
    E = ES.BLOCK
    st = cport.EnvState(E, N)
    vp = np.ones(E)
    st.hr[:] = RB; st.rr[:] = RB; st.hvpref[:] = 1.0
    st.hpx[:] = FAR * (2 + np.arange(N))[None]; st.hpy[:] = FAR
    st.hgx[:], st.hgy[:] = st.hpx, st.hpy
    for e in range(E if found else 0):
        pos, vel, v, pref, op, ov = found[e % len(found)]
        k = (e // 2) % N
        a = dict(p=pos, v=vel, g=(pos[0] + pref[0], pos[1] + pref[1]), vp=v)
        b = dict(p=op, v=ov, g=op, vp=1.0)
        hum, rob = (a, b) if e % 2 == 0 else (b, a)
        st.hpx[e, k], st.hpy[e, k], st.hvx[e, k], st.hvy[e, k] = hum["p"] + hum["v"]
        st.hgx[e, k], st.hgy[e, k], st.hvpref[e, k] = hum["g"] + (hum["vp"],)
        st.rpx[e], st.rpy[e], st.rvx[e], st.rvy[e] = rob["p"] + rob["v"]
        st.rgx[e], st.rgy[e], vp[e] = rob["g"] + (rob["vp"],)
    return st, vp


@functools.lru_cache(maxsize=None)
def _edge_batch(N, config):
    mn, nd, th, dt = CONFIGS[config]
    st, vp, names = CS.edge_batch(N, mn, nd)
    parts, vps, names = [st], [vp], ["robot/" + n for n in names]
    if N <= 10:
        hs, _, _, hn = ES.edge_batch(N, True, {"neighbor_dist": 1.5} if nd == 1.5 else {})
        n = 13 * ES.BLOCK                                  # the untranslated blocks
        parts.append(ES.take(hs, np.arange(n))); vps.append(np.ones(n)); names += ["human/" + x for x in hn[:n]]
    ts, tvp = _lp2_tangent_block(N, nd, th, dt)
    parts.append(ts); vps.append(tvp); names += ["lp2-tangent"] * ts.E
    st, vel = from_env_state(ES._concat(parts), np.concatenate(vps))
    return st, vel, tuple(names)


def edge_batch(N, config):
    """(state, sim_vel, names) of the N-human edge batch under CONFIGS[config]; names[e] is the block of env e.  Built
    once per process; the caller gets copies."""
    st, vel, names = _edge_batch(int(N), int(config))
    return {k: v.copy() for k, v in st.items()}, vel.copy(), list(names)


@functools.lru_cache(maxsize=None)
def edge_replay(N, config):
    """(replay of edge_batch(N, config) for T_EDGE steps, edge_counts, lp3_entries of that replay).  Once per process:
    treat the result as read-only."""
    st, vel, names = edge_batch(N, config)
    cport.edge_counts(reset=True); cport.lp3_entries()
    ref = R.replay(st, vel, max_steps=T_EDGE, **params(config))
    return ref, cport.edge_counts(reset=True), cport.lp3_entries()


# ---------------------------------------------------------------------------------------------------------------------
# the float64 half

BOUNDARY_COUNTS = (2, 5)
BOUNDARY_STEPS = 3
BOUNDARY_TIME_STEPS = (0.25, 0.1)
TOUCH = (0.1875, 0.25)                          # |TOUCH| == RB exactly
ODD_TIMES = (float("nan"), -1.0, float("inf"), 5e-324)
UP = lambda x: float(np.nextafter(f64(x), f64(np.inf)))


def _dist(p, g):
    dx, dy = f64(p[0]) - f64(g[0]), f64(p[1]) - f64(g[1])
    return np.sqrt(dx * dx + dy * dy)


@functools.lru_cache(maxsize=None)
def f64_entry_positions(shift=2.0 ** 10, rad=0.35):
    """Two positions next to a goal at (shift, shift), radius rad: the first inside the radius as a float64 and outside
    once rounded to float32, the second the other way round.  A deterministic search: for y offsets on the 1/16 grid,
    the float64 neighbours of the float32 midpoints around the x at which the circle is crossed."""
    goal = (shift, shift)
    inside = lambda p: bool(_dist(p, goal) < rad)
    rounded = lambda p: (float(f32(p[0])), float(f32(p[1])))
    only64 = only32 = None
    for j in range(1, 5):
        y = shift + j / 16
        a = f32(shift + np.sqrt(rad * rad - (j / 16) ** 2))
        for _ in range(3):
            a = np.nextafter(a, f32(-np.inf))
        for _ in range(6):
            b = np.nextafter(a, f32(np.inf))
            x = (f64(a) + f64(b)) / 2
            for _ in range(4):
                x = np.nextafter(x, -np.inf)
            for _ in range(9):
                p = (float(x), y)
                if only64 is None and inside(p) and not inside(rounded(p)):
                    only64 = p
                if only32 is None and inside(rounded(p)) and not inside(p):
                    only32 = p
                x = np.nextafter(x, np.inf)
            a = b
        if only64 and only32:
            return only64, only32
    raise AssertionError("no float64 / float32 arrival split found")


@functools.lru_cache(maxsize=None)
def unit_offsets():
    """(an off-axis offset of float64 length exactly 1, one of length 1 + 2^-52): Pythagorean triples over their
    hypotenuse, the first that qualify, nudged by ulps of the larger component if need be."""
    one, above = None, None
    for a, b, c in ((3, 4, 5), (5, 12, 13), (8, 15, 17), (7, 24, 25), (20, 21, 29)):
        x, y = a / c, b / c
        for _ in range(4):
            n = _dist((x, y), (0.0, 0.0))
            if one is None and n == 1:
                one = (x, y)
            if above is None and n == UP(1.0):
                above = (x, y)
            y = UP(y)
    assert one and above
    return one, above


def _parked(N):
    """One env in which nothing happens: everybody on its goal, FAR apart, every time set."""
    st = dict(hpos=np.zeros((1, N, 2)), hgoal=np.zeros((1, N, 2)), hrad=np.full((1, N), RB), hvpref=np.ones((1, N)),
              rpos=np.array([[-FAR, -FAR]]), rgoal=np.array([[-FAR, -FAR]]), rrad=np.array([RB]), rvpref=np.ones(1),
              gtime=np.zeros(1), human_times=np.ones((1, N)))
    st["hpos"][0, :, 0] = FAR * (1 + np.arange(N)); st["hpos"][0, :, 1] = FAR
    st["hgoal"][:] = st["hpos"]
    return st, np.zeros((1, N + 1, 2), f32)


def _human(st, i, goal, off, rad=RB, time=0.0, vpref=1.0):
    st["hgoal"][0, i] = goal
    st["hpos"][0, i] = (goal[0] + off[0], goal[1] + off[1])
    st["hrad"][0, i], st["human_times"][0, i], st["hvpref"][0, i] = rad, time, vpref


@functools.lru_cache(maxsize=None)
def _boundary_batch(N):
    cases = []

    def case(name, select=1):
        st, vel = _parked(N)
        cases.append((name, st, vel, select))
        return st, vel

    st, _ = case("arrival-touch"); _human(st, 0, (1.0, 2.0), TOUCH)
    st, _ = case("arrival-below"); _human(st, 0, (1.0, 2.0), TOUCH, rad=UP(RB))
    st, _ = case("arrival-before-move"); _human(st, N - 1, (-3.0, 0.5), (RB + 2.0 ** -20, 0.0))
    only64, only32 = f64_entry_positions()
    s = 2.0 ** 10
    st, _ = case("arrival-f64-entry/f64-only"); _human(st, 0, (s, s), (0.0, 0.0), rad=0.35); st["hpos"][0, 0] = only64
    st, _ = case("arrival-f64-entry/f32-only"); _human(st, 1, (s, s), (0.0, 0.0), rad=0.35); st["hpos"][0, 1] = only32
    one, above = unit_offsets()
    st, _ = case("pref-unit/axis"); _human(st, 0, (0.0, 0.0), (-1.0, 0.0)); _human(st, 1, (0.0, 40.0), (0.0, 1.0))
    st, _ = case("pref-unit/triple"); _human(st, 0, (0.0, 0.0), (-one[0], -one[1]))
    st, _ = case("pref-above/axis"); _human(st, 1, (0.0, 0.0), (UP(1.0), 0.0))
    st, _ = case("pref-above/triple"); _human(st, 0, (0.0, 0.0), above)
    # on its goal with a velocity, a second human under way keeps the env going: pref stays (0, 0) for three steps
    st, vel = case("pref-below"); _human(st, 0, (0.5, 0.5), (0.0, 0.0)); _human(st, 1, (0.0, 8.0), (3.0, 0.0))
    vel[0, 1] = (0.25, -0.125)
    for r in range(4):
        odd = [ODD_TIMES[(r + i) % 4] for i in range(N)]
        # -0.0 is pending: that human stands inside its radius, arrives on step 1 and the env stops
        st, _ = case("times-odd/neg-zero-%d" % r); st["human_times"][0] = odd; _human(st, 0, (2.0, 2.0), (0.125, 0.0), time=-0.0)
        st, _ = case("times-odd/all-set-%d" % r); st["human_times"][0] = odd
        st["hpos"][0, 0] = st["hgoal"][0, 0] + 3.0                        # under way, but its time is "set"
        st, _ = case("times-odd/one-zero-%d" % r); st["human_times"][0] = odd; _human(st, N - 1, (2.0, 2.0), (3.0, 0.0))
    for name, t0 in (("clock/2^53", 2.0 ** 53), ("clock/1e6+0.1", 1e6 + 0.1)):
        st, _ = case(name); st["gtime"][0] = t0
        _human(st, 0, (2.0, 2.0), (3.0, 0.0)); _human(st, 1, (0.0, 8.0), (0.125, 0.0))
    for b in (0, 1, 2, 255):
        st, _ = case("select-values/%d" % b, select=b); _human(st, 0, (2.0, 2.0), (0.125, 0.0)); _human(st, 1, (0.0, 8.0), (3.0, 0.0))
    # float32(0.35) < 0.35: at distance float32(0.35) the human has arrived by the float64 radius only; its neighbour
    # walks at it, so that the solve (float32 radius, float32(0.8) top speed) is not idle either
    st, vel = case("radius-rounding")
    _human(st, 0, (0.0, 0.0), (float(f32(0.35)), 0.0), rad=0.35, vpref=0.8)
    _human(st, 1, (-2.0, 0.0), (3.0, 0.0), rad=0.35, vpref=0.8)
    vel[0, 2] = (-0.8, 0.0)
    st, vel = R.stack([(c[1], c[2]) for c in cases])
    return st, vel, tuple(c[0] for c in cases), np.array([c[3] for c in cases], np.uint8)


def boundary_batch(N):
    """(state, sim_vel, names, select) of the N-human boundary batch: one case per env, names[e] its name.  It is run
    for BOUNDARY_STEPS steps under each of BOUNDARY_TIME_STEPS with the default ORCA parameters."""
    st, vel, names, select = _boundary_batch(int(N))
    return {k: v.copy() for k, v in st.items()}, vel.copy(), list(names), select.copy()


@functools.lru_cache(maxsize=None)
def boundary_replay(N, time_step):
    """(replay, events) of boundary_batch(N) for BOUNDARY_STEPS steps; read-only."""
    st, vel, names, select = boundary_batch(N)
    events = {}
    ref = R.replay(st, vel, select=select, max_steps=BOUNDARY_STEPS, time_step=time_step, events=events)
    return ref, events


def clock(t0, time_step, steps):
    """gtime after `steps` steps: plain float64 accumulation."""
    t = f64(t0)
    for _ in range(steps):
        t = t + f64(time_step)
    return t


def _case_table(N):
    """name prefix -> (steps taken, {human index: the step that sets its time}); every other entry keeps its bytes."""
    return {"arrival-touch": (2, {0: 2}), "arrival-below": (1, {0: 1}), "arrival-before-move": (2, {N - 1: 2}),
            "arrival-f64-entry/f64-only": (1, {0: 1}), "arrival-f64-entry/f32-only": (2, {1: 2}),
            "pref-unit": (3, {}), "pref-above": (3, {}), "pref-below": (3, {0: 1}),
            "times-odd/neg-zero": (1, {0: 1}), "times-odd/all-set": (0, {}), "times-odd/one-zero": (3, {}),
            "clock": (3, {1: 1}), "select-values/0": (0, {}), "select-values": (3, {0: 1}), "radius-rounding": (3, {0: 1})}


def boundary_expected(N, time_step):
    """What the header's text says of each named case, worked out by hand (_case_table), not by a replay:
    (steps [E], human_times [E,N], gtime [E])."""
    st, vel, names, select = boundary_batch(N)
    table = _case_table(N)
    steps, times, gtime = np.zeros(len(names), np.int32), st["human_times"].copy(), st["gtime"].copy()
    for e, name in enumerate(names):
        key = max((k for k in table if name.startswith(k)), key=len)
        steps[e], sets = table[key]
        for i, s in sets.items():
            assert st["human_times"][e, i] == 0
            times[e, i] = clock(st["gtime"][e], time_step, s)
        gtime[e] = clock(st["gtime"][e], time_step, steps[e])
    return steps, times, gtime


def assert_boundary_cases(res, N, time_step, what=""):
    """res (a replay or a kernel result: steps, human_times, gtime, sim_vel, hpos) against boundary_expected, with the
    exact bytes of human_times and gtime (a NaN's bytes too), and the exact velocities of the pref-* cases."""
    st, vel, names, select = boundary_batch(N)
    steps, times, gtime = boundary_expected(N, time_step)
    bits = lambda a: np.ascontiguousarray(a, f64).view(np.uint64)
    for e, name in enumerate(names):
        assert int(res["steps"][e]) == steps[e], (what, name, res["steps"][e])
        assert bits(res["human_times"][e]).tolist() == bits(times[e]).tolist(), (what, name, res["human_times"][e], times[e])
        assert bits(res["gtime"][e]).tolist() == bits(gtime[e]).tolist(), (what, name, res["gtime"][e])
        if steps[e] == 0:
            assert bits(res["hpos"][e]).tolist() == bits(st["hpos"][e]).tolist(), (what, name)
            assert np.array_equal(np.asarray(res["sim_vel"][e]).view(np.uint32), vel[e].view(np.uint32)), (what, name)
    # the first step's positions, p32 + pref * float32(time_step): pref is the unnormalised offset at n == 1, the offset
    # over n one ulp above, (0, 0) on the goal
    dt = f32(time_step)
    row = lambda name: res["traj"][names.index(name)][0] if isinstance(res["traj"], list) else res["traj"][0, names.index(name)]
    at = lambda name, agent: tuple(float(x) for x in row(name)[agent])
    step = lambda p, v: tuple(float(f32(a) + f32(f32(b) * dt)) for a, b in zip(p, v))
    one, above = unit_offsets()
    assert at("pref-unit/axis", 1) == step((-1.0, 0.0), (1.0, 0.0)) and at("pref-unit/axis", 2) == step((0.0, 41.0), (0.0, -1.0)), what
    assert at("pref-unit/triple", 1) == step((-one[0], -one[1]), one), what
    n = UP(1.0)
    assert at("pref-above/axis", 2) == step((n, 0.0), (-n / n, 0.0)), what
    assert at("pref-above/triple", 1) == step(above, (-above[0] / n, -above[1] / n)), what
    assert at("pref-below", 1) == (0.5, 0.5), what
    e = names.index("pref-below")
    assert tuple(res["hpos"][e, 0]) == (0.5, 0.5) and tuple(float(x) for x in res["sim_vel"][e, 1]) == (0.0, 0.0), what
