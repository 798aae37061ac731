"""Robot-centred edge batches for the closed loop with an ORCA robot (mcn_env_rollout_orca), in the dyadic conventions of
tests/edge_states.py: positions on a 1/8 grid, velocities on a 1/16 grid, radius 0.3025, robot safety spaces 0 and 0.0625
(float32((0.3025 + 0.01) + s) is 0.3125 / 0.375), so that the robot's float32 solve meets exact ties, exact zeros and
non-finite half-planes.  tests/edge_states.py centres its blocks on human 0; here the ROBOT is the agent in the middle.

Blocks of 16 envs (edge_batch), for a robot policy (max_neighbors, neighbor_dist):
  ring            the robot in the middle of rings of humans at equal distances, shuffled over the indices: with more
                  humans than max_neighbors the cut falls on a tie and index order decides
  range-edge      one human at exactly neighbor_dist from the robot (strict <: left out), the others near
  coincident      the robot on a human: equal velocity (0/0, a NaN half-plane) in even envs, another velocity in odd ones
  on-goal         rgoal == rpos: a zero preferred velocity
  on-disc         |rgoal - rpos| == v_pref exactly: (0.375, 0.5) with v_pref 0.625, (0.75, 1) with 1.25
  packed          crowds around the robot with spacing below the radius sum: the robot's solve reaches the 3-D LP
  simple          everybody at rest, far apart
then the same blocks translated by 2^10 and 2^20, then PAD random envs (ragged E).

CONFIGS lists the robot policies the batches are run with: max_neighbors {10, 3, 2, 0} x neighbor_dist {10, 1.5}, the
safety space and the robot's visibility alternating.  edge_replay() is the host replay (tests/closed_loop_ref.py) of
one batch under one config, computed once per process.
"""
import functools
import itertools

import numpy as np

from oracle import cport
from tests import closed_loop_ref as CR
from tests.edge_states import BLOCK, HR, PAD, SHIFTS, VPREF, _RING, _concat, _grid, _lattice, _random, _take  # noqa: F401

HUMAN_COUNTS = (1, 2, 5, 7, 10, 13, 32)
T_EDGE = 6
# (max_neighbors, neighbor_dist, robot safety_space, robot visible to the humans)
CONFIGS = tuple((mn, nd, (0.0, 0.0625)[i % 2], bool((i + i // 2) % 2))
                for i, (mn, nd) in enumerate(itertools.product((10, 3, 2, 0), (10.0, 1.5))))
_AXES = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float64)
_DISC = np.array([(0.375, 0.5), (-0.5, 0.375), (0.375, -0.5), (-0.5, -0.375), (0.5, 0.375), (-0.375, 0.5)], np.float64)


def _blocks(rng, N, max_neighbors, neighbor_dist):
    """(name, EnvState [BLOCK], rvpref [BLOCK]) per block."""
    out = []

    def add(name, st, rvpref=None):
        out.append((name, st, rng.choice(VPREF, BLOCK) if rvpref is None else rvpref))

    # rings of 12 lattice points each at |p| = 5 s, 10 s, 15 s around the robot, the humans dealt over them in shuffled
    # index order (the innermost ring first: with 12 equidistant humans any max_neighbors < 12 cuts inside a tie)
    st = _random(rng, BLOCK, N, spread=2.0)
    for e in range(BLOCK):
        s = rng.choice([1 / 8, 1 / 4, 1 / 2, 3 / 8])
        pts = np.concatenate([_RING[rng.permutation(len(_RING))] * (s * k) for k in (1, 2, 3)])[:N]
        pts = pts[rng.permutation(N)]
        st.hpx[e], st.hpy[e] = st.rpx[e] + pts[:, 0], st.rpy[e] + pts[:, 1]
    add("ring", st)
    # one human at exactly neighbor_dist
    st = _random(rng, BLOCK, N, spread=1.0)
    offs = [a * neighbor_dist for a in _AXES] + ([p * 2 for p in _RING[[1, 2, 4, 5, 7, 8, 10, 11]]] if neighbor_dist == 10 else [])
    for e in range(BLOCK):
        off, k = offs[rng.randint(len(offs))], rng.randint(N)
        st.hpx[e, k], st.hpy[e, k] = st.rpx[e] + off[0], st.rpy[e] + off[1]
    add("range-edge", st)
    # the robot on a human
    st = _random(rng, BLOCK, N, spread=1.0)
    for e in range(BLOCK):
        k = rng.randint(N)
        st.rpx[e], st.rpy[e] = st.hpx[e, k], st.hpy[e, k]
        if e % 2 == 0:
            st.rvx[e], st.rvy[e] = st.hvx[e, k], st.hvy[e, k]
        elif (st.rvx[e], st.rvy[e]) == (st.hvx[e, k], st.hvy[e, k]):
            st.rvx[e] += 1 / 16
    add("coincident", st)
    st = _random(rng, BLOCK, N, spread=2.0); st.rgx[:], st.rgy[:] = st.rpx, st.rpy
    add("on-goal", st)
    st = _random(rng, BLOCK, N, spread=3.0)
    scale = np.where(np.arange(BLOCK) % 4 == 3, 2.0, 1.0)
    d = _DISC[np.arange(BLOCK) % len(_DISC)] * scale[:, None]
    st.rgx[:], st.rgy[:] = st.rpx + d[:, 0], st.rpy + d[:, 1]
    add("on-disc", st, 0.625 * scale)
    # packed: half of the block a lattice of spacing 0.5 with the robot on a lattice point, half a random crowd within
    # 0.625 of the origin with the robot among it
    a, b = _lattice(rng, BLOCK // 2, N, 0.5), _random(rng, BLOCK - BLOCK // 2, N, spread=0.625)
    add("packed", _concat([a, b]))
    st = _random(rng, BLOCK, N, spread=30.0)
    st.hvx[:] = 0; st.hvy[:] = 0; st.rvx[:] = 0; st.rvy[:] = 0
    add("simple", st)
    return out


@functools.lru_cache(maxsize=None)
def _edge_batch(N, max_neighbors, neighbor_dist, seed):
    rng = np.random.RandomState(seed * 7919 + 31 * N + 11 * max_neighbors + int(8 * neighbor_dist))
    blocks = _blocks(rng, N, max_neighbors, neighbor_dist)
    base = _concat([b[1] for b in blocks])
    vp = np.concatenate([b[2] for b in blocks])
    names = [b[0] for b in blocks for _ in range(b[1].E)]
    parts, vps, nms = [], [], []
    for s in SHIFTS:
        c = _concat([base])
        for k in ("hpx", "hpy", "hgx", "hgy", "rpx", "rpy", "rgx", "rgy"):
            getattr(c, k)[:] += s
        parts.append(c); vps.append(vp); nms += ["%s@%g" % (n, s) if s else n for n in names]
    st = _concat(parts + [_random(rng, PAD, N)])
    st.gtime[:] = 0.0                     # T_EDGE steps stay clear of the time limit: the ladder has its own batches
    return st, np.concatenate(vps + [rng.choice(VPREF, PAD)]), nms + ["pad"] * PAD


def edge_batch(N, max_neighbors, neighbor_dist, seed=0):
    """(EnvState, rvpref [E], names): names[e] is the block of env e.  Built once per process; the caller gets copies."""
    st, vp, names = _edge_batch(int(N), int(max_neighbors), float(neighbor_dist), seed)
    return st.copy(), vp.copy(), list(names)


def oracle_cfg(visible, **kw):
    """The env step's oracle config: the humans keep the default ORCA parameters (orca.py:59-62)."""
    return cport.default_cfg(robot_visible=1 if visible else 0, **kw)


class Result(object):
    pass


def replay(st0, rvpref, pol, cfg, T, roll=None, has_rtheta=True, count=True):
    """closed_loop_ref.ClosedLoop over T steps from a copy of st0: its traces, end state, records and counters."""
    st = st0.copy()
    cl = CR.ClosedLoop(cfg, st, rvpref, pol, roll=roll, has_rtheta=has_rtheta, count=count).run(T)
    r = Result()
    r.st0, r.st, r.rvpref, r.pol, r.cfg, r.T, r.roll = st0, st, np.asarray(rvpref, np.float64), pol, cfg, T, roll
    r.tr, r.robot_events, r.human_events = cl.traces(), dict(cl.robot_events), dict(cl.human_events)
    r.robot_events["lp3"] = cl.robot_lp3
    r.nan_actions, r.robot_lines = cl.nan_actions, cl.robot_lines
    return r


@functools.lru_cache(maxsize=None)
def edge_replay(N, config):
    """The replay of edge_batch(N, ...) under CONFIGS[config] for T_EDGE steps, no mcn_rollout (r.names: block per env)."""
    mn, nd, ss, visible = CONFIGS[config]
    st, vp, names = edge_batch(N, mn, nd)
    r = replay(st, vp, CR.RobotPolicy(ss, nd, mn, 5.0), oracle_cfg(visible), T_EDGE)
    r.names, r.visible = names, visible
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the order of the two additions of the ORCA margin (orca.py:100,103: `radius + 0.01 + safety_space`)

def reference_order(r, s):
    return np.float32((np.float64(r) + 0.01) + np.float64(s))


def summed_margin_order(r, s):
    return np.float32(np.float64(r) + (0.01 + np.float64(s)))


@functools.lru_cache(maxsize=None)
def radius_order_radii(s=0.1, lo=0.3, hi=0.5, want=12):
    """Radii in [lo, hi] at which the two orders round to different float32 values, found by a search next to float32
    midpoints: the float64 sums differ by an ulp or so, which shows after rounding only where a midpoint lies between
    them.  Deterministic: walks the float32 grid upwards from float32(lo + 0.01 + s)."""
    found = []
    a = np.float32(lo + 0.01 + s)
    while len(found) < want and a < hi + 0.01 + s:
        b = np.nextafter(a, np.float32(np.inf))
        mid = (np.float64(a) + np.float64(b)) / 2
        r = mid - (0.01 + s)
        for _ in range(4):
            r = np.nextafter(r, -np.inf)
        for _ in range(9):                                   # the few float64 neighbours of mid - margin
            if lo <= r <= hi and reference_order(r, s) != summed_margin_order(r, s):
                found.append(float(r))
                break
            r = np.nextafter(r, np.inf)
        a = b
    return tuple(found)


def radius_order_scene(r, s=0.1):
    """One human of radius r standing 1.25 m straight ahead of a robot that walks at it at full speed: its half-plane
    is active, so the robot's velocity depends on the last bit of the radius sum.  Returns (EnvState E = 1, rvpref)."""
    st = cport.EnvState(1, 1)
    st.rpx[0], st.rpy[0], st.rvx[0], st.rvy[0], st.rgx[0], st.rgy[0], st.rr[0] = 0.0, -1.0, 0.0, 1.0, 0.0, 4.0, 0.3
    st.hpx[0, 0], st.hpy[0, 0], st.hgx[0, 0], st.hgy[0, 0], st.hr[0, 0], st.hvpref[0, 0] = 0.0, 0.25, 0.0, 0.25, r, 1.0
    return st, np.ones(1)


def radius_order_actions(r, s=0.1):
    """The robot's action in radius_order_scene(r) with the human's margin added in the reference's order, and with the
    margin summed first (everything else equal): two float32 pairs."""
    st, vp = radius_order_scene(r, s)
    o = CR.robot_operands(st, 0, vp, CR.RobotPolicy(s, 10.0, 10, 5.0))
    assert o["orad"][0] == reference_order(r, s)
    solve = lambda orad: cport.orca_agent(o["pos"], o["vel"], o["radius"], o["max_speed"], o["pref"], o["opos"], o["ovel"],
                                          np.array([orad], np.float32), time_step=np.float32(0.25))
    return solve(reference_order(r, s)), solve(summed_margin_order(r, s))


@functools.lru_cache(maxsize=None)
def radius_order_cases(s=0.1):
    """The radii of radius_order_radii() at which the two orders also give different robot actions (the robot's own
    0.41000003 plus the human's radius is rounded once more, which hides the last bit for about half of them)."""
    return tuple(r for r in radius_order_radii(s) if radius_order_actions(r, s)[0] != radius_order_actions(r, s)[1])
