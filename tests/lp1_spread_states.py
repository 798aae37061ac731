"""States for tests/test_lp1_spread_gpu.py: a batch of dyadic scenes in envs 0 .. 18 that puts the 1-D LP's pair
(line 3, earlier line 2) -- the intersection the four-wavefront rollout form computes on lane 0 of the quad and hands to
lane 3 (quad_common.hpp: lp1_spread) -- into every state it can be in, and a float32 restatement of the LP that says
which solve met which.  The restatement is only believed where its velocity is the C oracle's, bit for bit.

Every coordinate, velocity and goal is a multiple of 1/64 (or NaN), so the float64 -> float32 conversions are exact.
"""
import functools

import numpy as np

from oracle import cport

N = 5
T_MAX = 8
FAR = (40.0, 40.0)
f32 = np.float32
EPS = f32(1e-5)

# what a solve can meet (the keys of `replay`'s "events")
S_TR, S_TL, S_PAR_NEG, S_PAR_OK, S_EMPTY = "tr_lowered", "tl_raised", "parallel_infeasible", "parallel_noop", "empty_at_2"
S_NAN2, S_NAN3, S_FEWER = "nan_rank2", "nan_rank3", "fewer_than_four"
S_LP3_21, S_LP3_ON2 = "lp3_on_3_pair_21", "lp3_on_2"
EVENTS = (S_TR, S_TL, S_PAR_NEG, S_PAR_OK, S_EMPTY, S_NAN2, S_NAN3, S_FEWER, S_LP3_21, S_LP3_ON2)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
def _axis(st, e, up, down, right, left, goal, v_right=0.0, v_left=0.0):
    """human 0 at the origin, the others on the axes at distinct distances; the two on the x axis stand further away
    than the two on the y axis, so their half-planes are ranks 2 and 3 and exactly antiparallel.  At rest the strip
    between them is feasible (pair (3, 2): den = 0, num >= 0); with v_right / v_left they walk at human 0 fast enough
    that each demands a retreat from itself: the strip is empty (num < 0)."""
    st.hpx[e], st.hpy[e] = (0.0, 0.0, 0.0, right, -left), (0.0, up, -down, 0.0, 0.0)
    st.hvx[e] = (0.0, 0.0, 0.0, -v_right, v_left)
    st.hgx[e], st.hgy[e] = (goal[0], 0.0, 0.0, -6.0, 6.0), (goal[1], -6.0, 6.0, 0.0, 0.0)


def _dyadic_packed(st, e, seed, cells):
    """every human inside a square of +-cells / 16 m, on a grid of 1/16 m, goals across: dense, the quads reach line 3 and
    the 3-D LP"""
    rng = np.random.RandomState(seed)
    while True:
        p = rng.randint(-cells, cells + 1, (N, 2))
        if len({tuple(r) for r in p}) == N:
            break
    st.hpx[e], st.hpy[e] = p[:, 0] / 16.0, p[:, 1] / 16.0
    g = rng.randint(-96, 97, (N, 2))
    st.hgx[e], st.hgy[e] = g[:, 0] / 16.0 - 4 * st.hpx[e], g[:, 1] / 16.0 - 4 * st.hpy[e]


def _nan_velocity(st, e, who, seed, cells):
    """a packed scene in which human `who` starts with a NaN velocity at a finite position: in range for everybody, so
    its half-plane is NaN at the rank its distance gives it"""
    _dyadic_packed(st, e, seed, cells)
    st.hvx[e, who] = np.nan


def _far(st, e, k):
    """k of human 0's four candidates stand more than neighbor_dist (10 m) away: ranks 4 - k .. 3 of its table hold lines
    that are not part of its LP"""
    ring = [(1.5, 0.0), (0.0, 1.25), (-1.75, 0.0), (0.0, -2.0)]
    away = [(12.0, 0.0), (0.0, 12.0), (-12.0, 0.0), (0.0, -12.0)]
    far_idx = set(range(k)) if k % 2 else set(range(4 - k, 4))
    st.hpx[e, 0], st.hpy[e, 0] = 0.0, 0.0
    st.hgx[e, 0], st.hgy[e, 0] = 4.0, 1.0
    for c in range(4):
        x, y = away[c] if c in far_idx else ring[c]
        st.hpx[e, c + 1], st.hpy[e, c + 1] = x, y
        st.hgx[e, c + 1], st.hgy[e, c + 1] = -x, -y + 0.25


# env e holds scene e.  Seeds and sizes of the packed scenes were searched for what `replay` then proves.
SCENES = (
    lambda st, e: _dyadic_packed(st, e, *PACKED[0]),                 # env 0: the lone env of E = 1
    lambda st, e: _axis(st, e, 1.0, 1.5, 2.0, 2.5, (-6.0, 0.0)),                                   # strip feasible
    lambda st, e: _axis(st, e, 1.0, 1.5, 2.0, 2.5, (6.0, 0.0), v_right=0.375, v_left=0.4375),      # strip empty
    lambda st, e: _far(st, e, 1),                                    # env 3 straddles ORCA wavefronts 0 and 1
    lambda st, e: _far(st, e, 2),
    lambda st, e: _nan_velocity(st, e, *NAN_V[0]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[1]),                 # env 6 straddles ORCA wavefronts 1 and 2
    lambda st, e: _nan_velocity(st, e, *NAN_V[1]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[2]),                 # env 8: the partial workgroup of E = 9
    lambda st, e: _axis(st, e, 1.25, 1.0, 2.5, 2.0, (6.0, 0.0)),
    lambda st, e: _axis(st, e, 1.25, 1.0, 2.5, 2.0, (-6.0, 0.0), v_right=0.4375, v_left=0.375),
    lambda st, e: _dyadic_packed(st, e, *PACKED[3]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[4]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[5]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[6]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[7]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[8]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[9]),
    lambda st, e: _dyadic_packed(st, e, *PACKED[10]),
)
PACKED = ((58, 12), (75, 8), (83, 16), (293, 8), (12, 12), (269, 16), (258, 8), (294, 12), (182, 12), (157, 16), (38, 16))
NAN_V = ((1, 0, 8), (2, 0, 8))


@functools.lru_cache(maxsize=None)
def _batch(E):
    st = cport.EnvState(E, N)
    st.hr[:] = 0.3; st.hvpref[:] = 1.0; st.rr[:] = 0.3
    for e in range(E):
        SCENES[e % len(SCENES)](st, e)
    st.rpx[:], st.rpy[:] = FAR
    st.rgx[:], st.rgy[:] = FAR[0], FAR[1] + 25.0
    rng = np.random.RandomState(200 + E)
    acts = rng.randint(-8, 9, (T_MAX, E, 2)) / 16.0
    return st, acts


def batch(E):
    st, acts = _batch(E)
    return st.copy(), acts.copy()


# ---------------------------------------------------------------------------------------------------------------------
# RVO2's linearProgram1-3 in float32, operation by operation as orca_device.hpp writes them, telling what the LAST
# earlier line did to the 1-D LP
def _det(ax, ay, bx, by):
    return ax * by - ay * bx


def _dot(ax, ay, bx, by):
    return ax * bx + ay * by


def lp1(L, no, radius, optx, opty, dir_opt):
    """-> (point or None, what earlier line no - 1 did: a set of "par_neg", "par_ok", "tr", "tl", "empty"; empty when
    the LP ended before it)"""
    px, py, dx, dy = L[no]
    dp = _dot(px, py, dx, dy)
    disc = dp * dp + radius * radius - _dot(px, py, px, py)
    did = set()
    if disc < 0:
        return None, did
    sq = np.sqrt(disc)
    tl, tr = -dp - sq, -dp + sq
    for i in range(no):
        last = i == no - 1
        qx, qy, ex, ey = L[i]
        den = _det(dx, dy, ex, ey)
        num = _det(ex, ey, px - qx, py - qy)
        if np.abs(den) <= EPS:
            if num < 0:
                if last:
                    did.add("par_neg")
                return None, did
            if last:
                did.add("par_ok")
            continue
        t = num / den
        if den >= 0:
            ntr = np.fmin(tr, t)
            if last and ntr < tr:
                did.add("tr")
            tr = ntr
        else:
            ntl = np.fmax(tl, t)
            if last and ntl > tl:
                did.add("tl")
            tl = ntl
        if tl > tr:
            if last:
                did.add("empty")
            return None, did
    if dir_opt:
        t = tr if _dot(optx, opty, dx, dy) > 0 else tl
    else:
        t = _dot(dx, dy, optx - px, opty - py)
        if t < tl:
            t = tl
        elif t > tr:
            t = tr
    return (px + t * dx, py + t * dy), did


def lp2(L, radius, optx, opty, dir_opt, watch, seen):
    """`seen` collects what earlier line watch - 1 did in the 1-D LP of line `watch`; "tr" / "tl" only where the LP then
    succeeded, i.e. line `watch`'s candidate was taken"""
    if dir_opt:
        rx, ry = radius * optx, radius * opty
    elif _dot(optx, opty, optx, opty) > radius * radius:
        inv = f32(1) / np.sqrt(_dot(optx, opty, optx, opty))
        rx, ry = radius * (optx * inv), radius * (opty * inv)
    else:
        rx, ry = optx, opty
    for i in range(len(L)):
        px, py, dx, dy = L[i]
        if _det(dx, dy, px - rx, py - ry) > 0:
            got, did = lp1(L, i, radius, optx, opty, dir_opt)
            if i == watch:
                seen |= did if got is not None else did - {"tr", "tl"}
            if got is None:
                return i, rx, ry
            rx, ry = got
    return len(L), rx, ry


def lp3(L, begin, radius, rx, ry, events):
    dist = f32(0)
    for i in range(begin, len(L)):
        px, py, dx, dy = L[i]
        if _det(dx, dy, px - rx, py - ry) > dist:
            P = []
            for j in range(i):
                qx, qy, ex, ey = L[j]
                dt = _det(dx, dy, ex, ey)
                if np.abs(dt) <= EPS:
                    if _dot(dx, dy, ex, ey) > 0:
                        continue
                    sx, sy = f32(0.5) * (px + qx), f32(0.5) * (py + qy)
                else:
                    s = _det(ex, ey, px - qx, py - qy) / dt
                    sx, sy = px + s * dx, py + s * dy
                ddx, ddy = ex - dx, ey - dy
                inv = f32(1) / np.sqrt(_dot(ddx, ddy, ddx, ddy))
                P.append((sx, sy, ddx * inv, ddy * inv))
            seen = set()
            fail, nx, ny = lp2(P, radius, -dy, dx, True, 2, seen)
            if fail == len(P):
                rx, ry = nx, ny
            # a round on line 3 with all three projections kept, in which projected line 1 moved a bound of projected
            # line 2's 1-D LP and line 2's candidate was taken
            if i == 3 and len(P) == 3 and seen & {"tr", "tl"}:
                events.add(S_LP3_21)
            if i == 2:
                events.add(S_LP3_ON2)
            dist = _det(dx, dy, px - rx, py - ry)
    return rx, ry


def solve(lines, ms, prefx, prefy):
    """(vx, vy, events) of one human over its sorted in-range half-planes, float32 throughout"""
    events = set()
    with np.errstate(all="ignore"):
        L = [tuple(f32(v) for v in l) for l in lines]
        if len(L) >= 3 and np.isnan(L[2]).any():
            events.add(S_NAN2)
        if len(L) >= 4 and np.isnan(L[3]).any():
            events.add(S_NAN3)
        if 2 <= len(L) < 4:
            events.add(S_FEWER)
        seen = set()
        fail, rx, ry = lp2(L, f32(ms), f32(prefx), f32(prefy), False, 3, seen)
        for key, ev in (("tr", S_TR), ("tl", S_TL), ("par_ok", S_PAR_OK), ("empty", S_EMPTY)):
            if key in seen:
                events.add(ev)
        if "par_neg" in seen:
            assert fail == 3
            events.add(S_PAR_NEG)                                # the 2-D LP fails at line 3: the 3-D LP runs from there
        if fail < len(L):
            rx, ry = lp3(L, fail, f32(ms), rx, ry, events)
    return rx, ry, events


def _same_f32(a, b):
    a, b = f32(a), f32(b)
    return a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b))


@functools.lru_cache(maxsize=None)
def replay(E):
    """T_MAX oracle steps of the batch.  -> dict: events {name: bool [T_MAX, E, N]}, states (EnvState after each step)"""
    from tests import lp2_gate_states as LG
    st, acts = batch(E)
    cfg = cport.default_cfg(robot_visible=0)
    out = dict(events={k: np.zeros((T_MAX, E, N), bool) for k in EVENTS}, states=[])
    for t in range(T_MAX):
        before = st.copy()
        ref = cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        with np.errstate(all="ignore"):
            for e in range(E):
                for i in range(N):
                    lines = LG.human_lines(cfg, before, e, i)
                    pref = (f32(before.hgx[e, i] - before.hpx[e, i]), f32(before.hgy[e, i] - before.hpy[e, i]))
                    vx, vy, ev = solve(lines, before.hvpref[e, i], pref[0], pref[1])
                    assert _same_f32(vx, ref["human_act"][e, i, 0]) and _same_f32(vy, ref["human_act"][e, i, 1]), \
                        "the restated LP leaves the oracle at step %d env %d human %d" % (t, e, i)
                    for k in ev:
                        out["events"][k][t, e, i] = True
        out["states"].append(st.copy())
    return out
