"""Small env batches around the question "does the clipped preferred velocity violate any of this human's half-planes?",
with their properties proved by the C oracle on the CPU.

When it violates none of the nl lines a human solves over, the 2-D LP takes nothing and the clipped preferred velocity
is the ORCA result.  The quad kernels (csrc/quad_common.hpp: quad_orca_velocity) decide that per lane and per take
step; a wavefront holds a *group* of 64 // (4 * N) envs plus, in a ragged batch, idle lanes that alias env 0 and must
hold no half-plane.  A wave-uniform gate that returns early when a whole group is free was measured and rejected
(DESIGN 9); these batches were written for it and stay, because they put that decision on both sides, per group, per
step and at its edges, whatever form the solve takes.  Every batch is stepped T = 6 times.  `trace` replays a batch
with the oracle and classifies every human-step from the oracle's own values: cport.orca_lines gives the human's
sorted lines, cport.orca_agent without neighbours the clipped preferred velocity, cport.env_step the result.
tests/test_lp2_gate_states_cpu.py asserts each family's property (and that it is reached: every count > 0);
tests/test_lp2_gate_gpu.py runs the kernels on the same batches against the same trace, bit for bit.

Families (one batch per shape in SHAPES):
  all_free   rings of humans with goals radially outward: nobody ever meets a violated line.  For the transitions
             inside one launch, one env has a pair that starts with velocities aimed at each other (its group takes at
             step 0) and one env has a pair that walks head-on from beyond neighbor_dist into range at step 5 (its group
             takes at step 5); in between the whole batch is free for 4 consecutive steps.
  one_quad   rings, except that in env 0 human 0's goal lies behind its ring neighbour: env 0 takes, every other env
             (its group mates included) stays free at every step.
  boundary   the preferred velocity exactly ON a line (det2 == 0: not violated, `>` is strict).  No grid search is
             needed for it: against a resting neighbour straight ahead the line is x = c with direction (+-0, 1), and a
             goal at pos + (c, 0), c read back from the oracle's line, makes (float)(goal - pos) == c and det2 exactly
             0.  So the exact zero is what is used, for every shape; the two nearest representable cases (c one ulp up:
             violated; one ulp down: free) ride along in the next envs where the batch has room (E >= 3).
  beyond_nl  max_neighbors 2, neighbor_dist 1.5: the only line the preferred velocity would violate belongs to a
             neighbour that is out of range (every shape) or the third-nearest of three in range (N >= 4), so it is not
             among the nl lines and the human is free.  (The dispatcher gives such configs to the lane-per-human
             kernels, which the batch then compares with the oracle.)
  nonfinite  rings, and in env 0 two humans that coincide with equal velocities and goals: their mutual half-plane is
             0/0 = NaN at every step, every test against it is false, the group stays free.
  ragged     env 0 is a small circle crossing (goals at the antipodes) and takes at EVERY step; all other envs are free
             rings.  With E = 4 or 7 at N = 5 the last group holds one real env and lanes that alias env 0.
  packed     env 0's humans overlap inside a disc of radius 0.3 so that a quad enters the 3-D LP; all other envs are
             free rings.
"""
import functools

import numpy as np

from oracle import cport

T = 6
# (E, N, robot visible)
SHAPES = ((1, 5, False), (3, 5, False), (4, 5, False), (7, 5, False), (4, 4, True), (4, 2, False))
FAMILIES = ("all_free", "one_quad", "boundary", "beyond_nl", "nonfinite", "ragged", "packed")
HR = 0.3
FAR = (40.0, 40.0)               # the robot's spot where it must not matter: beyond every neighbor_dist
_Z = np.zeros((0, 2))
FREE, TAKE = 0, 1


def orca_variant(family):
    return {"max_neighbors": 2, "neighbor_dist": 1.5} if family == "beyond_nl" else {}


def oracle_cfg(family, visible):
    v = dict(neighbor_dist=10.0, max_neighbors=10, safety_space=0.0)
    v.update(orca_variant(family))
    return cport.default_cfg(robot_visible=1 if visible else 0, orca_neighbor_dist=v["neighbor_dist"],
                             orca_max_neighbors=v["max_neighbors"], orca_safety_space=v["safety_space"])


def group_of(e, N):
    return e // (64 // (4 * N))


# ---- per-env scenes: each fills env e of st and returns the robot's spot when it is visible ----

def _rest(st, e, i, x, y):
    """human i at rest on its goal"""
    st.hpx[e, i], st.hpy[e, i], st.hgx[e, i], st.hgy[e, i] = x, y, x, y
    st.hvx[e, i] = st.hvy[e, i] = 0.0


def _ring(st, e, idx, cx=0.0, cy=0.0, r=2.0, phase=0.0, moving=True):
    """humans idx on a ring, goals 6 m further out along their ray, walking outward already (or still at rest)"""
    n = max(len(idx), 1)
    for q, i in enumerate(idx):
        a = phase + 2 * np.pi * q / n
        ux, uy = np.cos(a), np.sin(a)
        st.hpx[e, i], st.hpy[e, i] = cx + r * ux, cy + r * uy
        st.hgx[e, i], st.hgy[e, i] = cx + (r + 6) * ux, cy + (r + 6) * uy
        st.hvx[e, i], st.hvy[e, i] = (ux, uy) if moving else (0.0, 0.0)
    return cx, cy


def _scene_ring(st, e):
    return _ring(st, e, range(st.N), r=2.0 + 0.25 * (e % 3), phase=0.37 * e, moving=e % 2 == 0)


def _early_pair(st, e, i, j, cx, cy):
    """humans i, j 3 m apart, walking at each other (offset, so the nearer leg pushes sideways) with goals outward
    and to the other side of that push: the step-0 line is violated by the preferred velocity, then they part"""
    st.hpx[e, i], st.hpy[e, i], st.hvx[e, i], st.hvy[e, i] = cx - 1.5, cy, 1.0, 0.0
    st.hpx[e, j], st.hpy[e, j], st.hvx[e, j], st.hvy[e, j] = cx + 1.5, cy + 0.5, -1.0, 0.0
    st.hgx[e, i], st.hgy[e, i] = cx - 7.5, cy + 2.0
    st.hgx[e, j], st.hgy[e, j] = cx + 7.5, cy - 1.5


def _late_pair(st, e, i, j, cx, cy):
    """humans i, j head-on (offset by 0.25), 12.2 m apart, closing 0.5 m per step: in range (10) from step 5 on"""
    st.hpx[e, i], st.hpy[e, i], st.hvx[e, i], st.hvy[e, i] = cx - 6.1, cy, 1.0, 0.0
    st.hpx[e, j], st.hpy[e, j], st.hvx[e, j], st.hvy[e, j] = cx + 6.1, cy + 0.25, -1.0, 0.0
    st.hgx[e, i], st.hgy[e, i] = cx + 20.0, cy
    st.hgx[e, j], st.hgy[e, j] = cx - 20.0, cy + 0.25


def _scene_all_free(st, e):
    E, N = st.E, st.N
    late_env = min(1, E - 1)
    used = []
    if e == 0:
        _early_pair(st, e, 0, 1, 0.0, 0.0)
        used += [0, 1]
    if e == late_env:
        b = len(used)
        _late_pair(st, e, b, b + 1, 0.0, 30.0)
        used += [b, b + 1]
    if not used:
        return _scene_ring(st, e)
    # the others: a ring far from both pairs
    return _ring(st, e, [i for i in range(N) if i not in used], cx=0.0, cy=-30.0, r=2.0)


def _scene_through_neighbour(st, e):
    c = _ring(st, e, range(st.N), r=2.0, moving=False)
    if st.N >= 2:       # human 0's goal: 3 m behind human 1, on the line through both
        dx, dy = st.hpx[e, 1] - st.hpx[e, 0], st.hpy[e, 1] - st.hpy[e, 0]
        d = np.hypot(dx, dy)
        st.hgx[e, 0], st.hgy[e, 0] = st.hpx[e, 1] + 3 * dx / d, st.hpy[e, 1] + 3 * dy / d
    return c


def _scene_crossing(st, e):
    """circle crossing of radius 1.5: everybody's goal is the antipode"""
    for i in range(st.N):
        a = 0.2 + 2 * np.pi * i / st.N
        st.hpx[e, i], st.hpy[e, i] = 1.5 * np.cos(a), 1.5 * np.sin(a)
        st.hgx[e, i], st.hgy[e, i] = -1.5 * np.cos(a), -1.5 * np.sin(a)
        st.hvx[e, i] = st.hvy[e, i] = 0.0
    if st.N == 2:       # not exactly head-on
        st.hgy[e, 0] += 0.5
    return FAR


def _scene_packed(st, e):
    rng = np.random.RandomState(3)
    ang, d = rng.uniform(0, 2 * np.pi, st.N), rng.uniform(0.05, 0.3, st.N)
    if st.N == 2:       # one line only: 0.1 m apart the push-out alone exceeds v_pref and the 1-D LP is infeasible
        ang, d = np.array([0.0, np.pi]), np.array([0.05, 0.05])
    st.hpx[e], st.hpy[e] = d * np.cos(ang), d * np.sin(ang)
    st.hgx[e], st.hgy[e] = -6 * np.cos(ang), -6 * np.sin(ang)
    st.hvx[e] = 0.0; st.hvy[e] = 0.0
    return FAR


def _scene_coincident(st, e):
    c = _scene_ring(st, e)
    if st.N >= 2:
        for k in ("hpx", "hpy", "hvx", "hvy", "hgx", "hgy"):
            getattr(st, k)[e, 1] = getattr(st, k)[e, 0]
    return c


def _scene_boundary(st, e, ulps, cfg):
    """human 0 at the origin, at rest; human 1 at rest on its goal 3 m ahead; the rest at rest beyond neighbor_dist.
    Human 0's line against human 1 is x = c; its goal is (c moved by `ulps`, 0) and |c| < v_pref, so the preferred
    velocity is not clipped and lies exactly on (ulps = 0), just beyond (+1) or just inside (-1) the line."""
    N = st.N
    for i in range(N):
        _rest(st, e, i, 0.0, 20.0 + 3.0 * i)
    _rest(st, e, 0, 0.0, 0.0)
    if N >= 2:
        _rest(st, e, 1, 3.0, 0.0)
    lines = human_lines(cfg, st, e, 0, FAR)
    c = np.float32(lines[0][0]) if len(lines) else np.float32(0.25)
    for _ in range(abs(ulps)):
        c = np.nextafter(c, np.float32(np.inf if ulps > 0 else -np.inf))
    st.hgx[e, 0] = float(c)
    return FAR


def _scene_beyond_nl(st, e, cfg):
    """human 0 walks at human 1, which rests straight ahead: out of range (2 m, even envs and N < 4) or the
    third-nearest behind two resting humans 0.8 m away on the other side (1.2 m, odd envs, N >= 4)"""
    N = st.N
    for i in range(N):
        _rest(st, e, i, 0.0, 20.0 + 3.0 * i)
    _rest(st, e, 0, 0.0, 0.0)
    st.hgx[e, 0] = 8.0
    cut = N >= 4 and e % 2 == 1
    _rest(st, e, 1, 1.2 if cut else 2.0, 0.0)
    if cut:
        _rest(st, e, 2, -0.5, 0.625)
        _rest(st, e, 3, -0.5, -0.625)
    return FAR


@functools.lru_cache(maxsize=None)
def _batch(family, E, N, visible):
    cfg = oracle_cfg(family, visible)
    st = cport.EnvState(E, N)
    st.hr[:] = HR; st.hvpref[:] = 1.0; st.rr[:] = HR
    for e in range(E):
        if family == "all_free":
            spot = _scene_all_free(st, e)
        elif family == "one_quad":
            spot = _scene_through_neighbour(st, e) if e == 0 else _scene_ring(st, e)
        elif family == "boundary":
            spot = _scene_boundary(st, e, (0, 1, -1)[e % 3], cfg)
        elif family == "beyond_nl":
            spot = _scene_beyond_nl(st, e, cfg)
        elif family == "nonfinite":
            spot = _scene_coincident(st, e) if e == 0 else _scene_ring(st, e)
        elif family == "ragged":
            spot = _scene_crossing(st, e) if e == 0 else _scene_ring(st, e)
        elif family == "packed":
            spot = _scene_packed(st, e) if e == 0 else _scene_ring(st, e)
        else:
            raise KeyError(family)
        # a visible robot stands still at the scene's harmless spot; an invisible one wanders far away
        st.rpx[e], st.rpy[e] = spot if visible else FAR
        st.rgx[e], st.rgy[e] = st.rpx[e], st.rpy[e] + 25.0
    rng = np.random.RandomState(len(family) + 10 * E + N)
    if visible:
        ax, ay = np.zeros((T, E)), np.zeros((T, E))
    else:
        ax, ay = rng.randint(-16, 17, (T, E)) / 16.0, rng.randint(-16, 17, (T, E)) / 16.0
    return st, ax, ay


def batch(family, E, N, visible):
    """(EnvState, ax [T, E], ay [T, E]); the caller gets its own copy."""
    st, ax, ay = _batch(family, E, N, bool(visible))
    return st.copy(), ax.copy(), ay.copy()


# ---- the oracle's view of one human's solve ----

def _candidates(cfg, st, e, i, robot=None):
    o = [j for j in range(st.N) if j != i]
    opos = [(st.hpx[e, j], st.hpy[e, j]) for j in o]
    ovel = [(st.hvx[e, j], st.hvy[e, j]) for j in o]
    orad = [st.hr[e, j] + 0.01 + cfg.orca_safety_space for j in o]
    if cfg.robot_visible:
        opos.append(robot if robot is not None else (st.rpx[e], st.rpy[e]))
        ovel.append((0.0, 0.0) if robot is not None else (st.rvx[e], st.rvy[e]))
        orad.append(st.rr[e] + 0.01 + cfg.orca_safety_space)
    return (np.asarray(opos, np.float64).reshape(-1, 2), np.asarray(ovel, np.float64).reshape(-1, 2),
            np.asarray(orad, np.float64))


def human_lines(cfg, st, e, i, robot=None, neighbor_dist=None, max_neighbors=None):
    """The sorted half-planes (p.x, p.y, d.x, d.y) human i of env e solves over: the oracle's own construction."""
    opos, ovel, orad = _candidates(cfg, st, e, i, robot)
    return cport.orca_lines((st.hpx[e, i], st.hpy[e, i]), (st.hvx[e, i], st.hvy[e, i]),
                            st.hr[e, i] + 0.01 + cfg.orca_safety_space, opos, ovel, orad,
                            neighbor_dist=cfg.orca_neighbor_dist if neighbor_dist is None else neighbor_dist,
                            max_neighbors=cfg.orca_max_neighbors if max_neighbors is None else max_neighbors,
                            time_horizon=cfg.orca_time_horizon, time_step=cfg.time_step)


def clipped_pref(cfg, st, e, i):
    """The clipped preferred velocity: the oracle's solve without neighbours."""
    pref = (np.float32(st.hgx[e, i] - st.hpx[e, i]), np.float32(st.hgy[e, i] - st.hpy[e, i]))
    return cport.orca_agent((st.hpx[e, i], st.hpy[e, i]), (st.hvx[e, i], st.hvy[e, i]),
                            st.hr[e, i] + 0.01 + cfg.orca_safety_space, st.hvpref[e, i], pref, _Z, _Z, [],
                            time_horizon=cfg.orca_time_horizon, time_step=cfg.time_step)


def line_dets(lines, v):
    """det2(d, p - v) of every line in float32, operation by operation as the solvers evaluate it"""
    with np.errstate(all="ignore"):
        L = np.asarray(lines, np.float32).reshape(-1, 4)
        vx, vy = np.float32(v[0]), np.float32(v[1])
        return L[:, 2] * (L[:, 1] - vy) - L[:, 3] * (L[:, 0] - vx)


def _sub(st, e):
    o = cport.EnvState(1, st.N)
    for k in cport.EnvState.FIELDS_H + cport.EnvState.FIELDS_R + ("gtime", "rtheta", "human_times"):
        setattr(o, k, np.ascontiguousarray(getattr(st, k)[e:e + 1]))
    return o


@functools.lru_cache(maxsize=None)
def trace(family, E, N, visible):
    """The oracle's T-step replay of a batch.  Returns a dict:
      cls [T, E, N]   FREE / TAKE: whether the clipped preferred velocity violates one of the human's nl lines
      on_line [T, E, N]   the human has a finite line with det2 exactly 0
      wide [T, E, N]  as cls, over ALL candidates (neighbor_dist 10, max_neighbors 10): what nl leaves out
      pref [T, E, N, 2]   the clipped preferred velocity (float64 of the float32 value)
      lp3 [T, E]      3-D LP entries of the env's humans; nonfinite [T]: non-finite half-planes built in the step
      refs            cport.env_step's outputs of each step; states: the EnvState after each step
    Computed once per (family, shape); read-only for its users."""
    st, ax, ay = batch(family, E, N, visible)
    cfg = oracle_cfg(family, visible)
    out = dict(cls=np.zeros((T, E, N), int), on_line=np.zeros((T, E, N), bool), wide=np.zeros((T, E, N), int),
               pref=np.zeros((T, E, N, 2)), lp3=np.zeros((T, E), int), nonfinite=np.zeros(T, int), refs=[], states=[])
    for t in range(T):
        for e in range(E):
            for i in range(N):
                v = clipped_pref(cfg, st, e, i)
                out["pref"][t, e, i] = v
                d = line_dets(human_lines(cfg, st, e, i), v)
                out["cls"][t, e, i] = TAKE if np.any(d > 0) else FREE
                out["on_line"][t, e, i] = np.any(d == 0)
                dw = line_dets(human_lines(cfg, st, e, i, neighbor_dist=10.0, max_neighbors=10), v)
                out["wide"][t, e, i] = TAKE if np.any(dw > 0) else FREE
            cport.lp3_entries(reset=True)
            cport.env_step(cfg, _sub(st, e), ax[t, e:e + 1], ay[t, e:e + 1], update=False)
            out["lp3"][t, e] = cport.lp3_entries(reset=True)
        cport.edge_counts(reset=True)
        out["refs"].append(cport.env_step(cfg, st, ax[t], ay[t], update=True))
        out["nonfinite"][t] = cport.edge_counts(reset=True)["nonfinite_line"]
        out["states"].append(st.copy())
    return out
