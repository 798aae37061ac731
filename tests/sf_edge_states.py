"""Constructed states for the social-force step (mcn_env_step_sf) and for the float32 overlap pre-filter that every
non-ORCA step shares.

  overlap_batch(N)   overlapping human pairs well inside the pre-filter's 1e-3 margin, nothing near touching
  edge_batch(N, ..)  named blocks of BLOCK envs on the edges of the definition itself (tests/social_force_ref.py), built
                     as tests/ladder_states.py builds its blocks: dyadic, axis-aligned, ties found with math.nextafter

Every block is described where it is built; `reached` says, from the restatement's own intermediate values, which
event an env of a block hits, so that tests can assert their inputs are what they claim."""
import functools
import math

import numpy as np

from oracle import cport
from tests import ladder_states as LS

DT = 0.25
BLOCK = 16
PAD = 5


# --------------------------------------------------------------------------------------------------- overlapping pairs
@functools.lru_cache(maxsize=None)
def _overlap_batch(N):
    assert N >= 2
    rng = np.random.RandomState(4000 + N)
    E = 2 * BLOCK + PAD
    st, ax, ay = LS._base(rng, E, N, (0.25, 0.3, 0.375))
    pairs = np.zeros(E, int)
    for e in range(E):
        # pairs (0, 1), (2, 3), .. leave the lattice for a row right of and above the robot, 2 apart; partners overlap
        # by 0.05 (every third pair by 0.25, every fifth is concentric)
        for k in range(1 + e % max(1, min(3, N // 2))):
            i, j = 2 * k, 2 * k + 1
            depth = 0.25 if (e + k) % 3 == 2 else 0.05
            D = 0.0 if (e + k) % 5 == 4 else st.hr[e, i] + st.hr[e, j] - depth
            st.hpx[e, i], st.hpy[e, i] = st.rpx[e] + 3 + 2 * k, st.rpy[e] + 3
            if (e + k) % 2:
                st.hpx[e, j], st.hpy[e, j] = st.hpx[e, i] + D, st.hpy[e, i]
            else:
                st.hpx[e, j], st.hpy[e, j] = st.hpx[e, i], st.hpy[e, i] + D
            pairs[e] += 1
    gaps = pair_gaps(st)
    iu = np.triu_indices(N, 1)
    g = gaps[:, iu[0], iu[1]]
    assert (np.abs(g) > 0.04).all(), "a pair within the float32 pre-filter's reach of touching"
    assert ((g < 0).sum(1) == pairs).all()
    assert max(np.abs(st.hpx).max(), np.abs(st.hpy).max()) < 16
    return st, ax, ay, pairs


def pair_gaps(st):
    """[E, N, N] float64 |p_i - p_j| - r_i - r_j, as the oracle's overlap test computes it."""
    dx, dy = st.hpx[:, :, None] - st.hpx[:, None], st.hpy[:, :, None] - st.hpy[:, None]
    return np.sqrt(dx * dx + dy * dy) - st.hr[:, :, None] - st.hr[:, None]


def overlap_batch(N):
    """(EnvState, ax, ay, overlapping pairs per env): 1 .. 3 overlapping pairs per env, gaps of -0.05, -0.25 and
    concentric discs; every other pair of humans is at least 0.04 from touching, every coordinate below 16."""
    st, ax, ay, pairs = _overlap_batch(N)
    return st.copy(), ax.copy(), ay.copy(), pairs.copy()


# ----------------------------------------------------------------------------------------- edges of the definition
# (A, B, k) sets every batch is stepped with.  Exact sets (A = 0): every m = 0 * exp(..) is exactly 0 (or NaN where exp
# overflows), so the restatement is bit-exact and the comparison is bitwise.
PARAMS = {
    "inert":   (0.0, 0.2, 4.0),         # A = 0; at rest w = e exactly (k dt = 1)
    "still":   (0.0, 0.2, 0.0),         # A = 0 and k = 0: w = v
    "default": (4.0, 0.2, 2.0),
    "k-zero":  (4.0, 0.2, 0.0),
    "B-tiny":  (4.0, 1e-300, 2.0),      # every exponent is +-inf (or a huge finite number): m is 0 or inf
    "B-big":   (4.0, 2.0 ** 10, 2.0),   # every exponent is ~0: m ~ A whatever the distance
    "B-small": (4.0, 2.0 ** -10, 2.0),  # deep overlaps overflow exp
}
EXACT = ("inert", "still")
NS = (1, 2, 5, 10, 13, 32)
# -(r + r_j - dist) / B of the "exp-range" block with B = 0.2: the normal range, its edge (-708.4), subnormal results
# (-708.4 .. -745.1) and underflow to 0
EXP_ARGS = (700.0, 708.0, 709.0, 712.0, 720.0, 730.0, 740.0, 744.0, 745.0, 745.5, 746.0, 750.0, 800.0, 1000.0, 704.0, 735.0)


def _ulps(x, k):
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def _blocks(rng, N, visible):
    radii = (0.25, 0.375)
    out = []

    def new():
        st, ax, ay = LS._base(rng, BLOCK, N, radii)
        return st

    # |g - p| == v_pref exactly (not clipped: the test is >) and one / two ulps of the goal's grid either side; the
    # human is at rest, so with k dt = 1 also |w| == v_pref exactly
    st = new()
    for e in range(BLOCK):
        k = e % N
        s = st.hvpref[e, k]
        st.hvx[e, k] = st.hvy[e, k] = 0.0
        axis, sign = (e // 2) % 2, (1, -1)[e % 2]
        p = (st.hpx, st.hpy)[axis][e, k]
        g = p + sign * s
        assert abs(g - p) == s
        g = _ulps(g, sign * (0, 0, 1, 1, -1, -1, 2, -2)[e % 8] if e >= 4 else 0)
        (st.hgx, st.hgy)[axis][e, k] = g
        (st.hgx, st.hgy)[1 - axis][e, k] = (st.hpx, st.hpy)[1 - axis][e, k]
    out.append(("goal-clip", st))
    # |v| == v_pref exactly and one ulp above, the human on its goal line far away: with k = 0 (and A = 0) w = v, so
    # |w| == v_pref exactly (not clipped) or one ulp above (clipped)
    st = new()
    for e in range(BLOCK):
        k = e % N
        sign = (1, -1)[e % 2]
        if e % 4 < 2:
            s = st.hvpref[e, k]
            v = [sign * (s if e < 8 else math.nextafter(s, math.inf)), 0.0]
            if (e // 4) % 2:
                v.reverse()
        else:
            st.hvpref[e, k] = 0.625                      # 3-4-5: (0.375, 0.5) has norm 0.625 exactly
            v = [sign * 0.375, (0.5 if e < 8 else math.nextafter(0.5, math.inf))]
        st.hvx[e, k], st.hvy[e, k] = v
    out.append(("w-clip", st))
    # v_pref = 0, a human on its goal, -0.0 components in e (goal x -0.0, position x +0.0), in v and -- with k = 0 --
    # in w
    st = new()
    for e in range(BLOCK):
        k = e % N
        kind = e % 4
        if kind == 0:
            st.hvpref[e, k] = 0.0
            if e % 8:
                st.hvx[e, k] = st.hvy[e, k] = 0.0
        elif kind == 1:
            st.hgx[e, k], st.hgy[e, k] = st.hpx[e, k], st.hpy[e, k]
            if e % 8 == 1:
                st.hvx[e, k], st.hvy[e, k] = -0.0, 0.0
            elif e == 5:
                st.hvx[e, k], st.hvy[e, k] = 0.0, 0.0
        elif kind == 2:
            st.hpx[e, k], st.hgx[e, k] = 0.0, -0.0       # e.x = -0.0 - 0.0 = -0.0
            st.hgy[e, k] = st.hpy[e, k] + (0.25, 3.0)[(e // 4) % 2]
            st.hvx[e, k] = (-0.0, 0.0)[(e // 8) % 2]
        else:
            st.hvx[e, k], st.hvy[e, k] = (-0.0, -0.0) if e < 8 else (-0.0, 0.25)
            st.hgx[e, k] = st.hpx[e, k] - (1.0 if e % 8 == 3 else 0.0)       # e.x - v.x < 0: a.x = -0.0 with k = 0
            st.hgy[e, k] = st.hpy[e, k]
    out.append(("zeros", st))
    # coincident agents contribute nothing: two humans at the front or the back of the index range, every other human
    # on human k, the robot on a human (it counts when the humans see it)
    st = new()
    for e in range(BLOCK):
        k = e % N
        kind = e % 4
        if kind == 0 and N >= 2:
            st.hpx[e, 1], st.hpy[e, 1] = st.hpx[e, 0], st.hpy[e, 0]
        elif kind == 1:
            st.hpx[e, :], st.hpy[e, :] = st.hpx[e, k], st.hpy[e, k]
        elif kind == 2:
            if N >= 2:
                st.hpx[e, N - 2], st.hpy[e, N - 2] = st.hpx[e, N - 1], st.hpy[e, N - 1]
            st.rpx[e], st.rpy[e] = st.hpx[e, k], st.hpy[e, k]
        else:
            st.hpx[e, N - 1], st.hpy[e, N - 1] = st.hpx[e, 0], st.hpy[e, 0]
            st.rpx[e], st.rpy[e] = st.hpx[e, 0], st.hpy[e, 0]
    out.append(("coincident", st))
    # one human at +-inf or NaN in even envs (odd envs are left alone)
    st = new()
    for e in range(0, BLOCK, 2):
        k = (e // 2) % N
        bad = (math.inf, -math.inf, math.nan, math.inf)[(e // 2) % 4]
        if (e // 8) % 2:
            st.hpy[e, k] = bad
        else:
            st.hpx[e, k] = bad
        if e == 14:
            st.hpx[e, k], st.hpy[e, k] = math.nan, -math.inf
    out.append(("nonfinite-human", st))
    # envs 8 .. 15 repeat envs 0 .. 7 with a NaN or infinite robot position: nothing changes unless the humans see it
    st = new()
    for e in range(8, BLOCK):
        for f in cport.EnvState.FIELDS_H + cport.EnvState.FIELDS_R + ("gtime",):
            getattr(st, f)[e] = getattr(st, f)[e - 8]
        bad = (math.nan, math.inf, -math.inf, math.nan)[e % 4]
        if e % 2:
            st.rpy[e] = bad
        else:
            st.rpx[e] = bad
    out.append(("nonfinite-robot", st))
    # exp in its subnormal range and underflowing to 0: human k's neighbour (the next human, or the robot for a lone
    # human) sits r + r_j + EXP_ARGS[e] * 0.2 away along an axis
    st = new()
    for e in range(BLOCK):
        k = e % N
        j = (k + 1) % N
        rj = st.hr[e, j] if N >= 2 else st.rr[e]
        D = st.hr[e, k] + rj + EXP_ARGS[e] * 0.2
        off = ((D, 0.0), (0.0, D), (-D, 0.0), (0.0, -D))[e % 4]
        if N >= 2:
            st.hpx[e, j], st.hpy[e, j] = st.hpx[e, k] + off[0], st.hpy[e, k] + off[1]
        else:
            st.rpx[e], st.rpy[e] = st.hpx[e, k] + off[0], st.hpy[e, k] + off[1]
    out.append(("exp-range", st))
    # deep overlaps: radii 0.375 + 0.375, centres 1/32 apart along an axis or a diagonal; with B = 2^-10 the exponent is
    # 736 or 722: exp overflows, m = inf, and the result is NaN after inf * 0 or the clip's inf / inf
    st = new()
    for e in range(BLOCK):
        k = e % N
        j = (k + 1) % N
        off = ((1 / 32, 0.0), (1 / 32, 1 / 32), (0.0, -1 / 32), (-1 / 32, 1 / 32))[e % 4]
        st.hr[e, k] = 0.375
        if N >= 2:
            st.hr[e, j] = 0.375
            st.hpx[e, j], st.hpy[e, j] = st.hpx[e, k] + off[0], st.hpy[e, k] + off[1]
        if N == 1 or e >= 8:
            st.rr[e] = 0.375
            st.rpx[e], st.rpy[e] = st.hpx[e, k] - off[0], st.hpy[e, k] - off[1]
    out.append(("deep-overlap", st))
    # a crowd pulled together (forces of every size), and the same envs translated by 2^10 and 2^20
    st = new()
    for e in range(BLOCK):
        cx, cy = st.hpx[e].mean(), st.hpy[e].mean()
        st.hpx[e] = cx + (st.hpx[e] - cx) * (0.5, 0.25, 0.75, 1.0)[e % 4]
        st.hpy[e] = cy + (st.hpy[e] - cy) * (0.5, 0.25, 0.75, 1.0)[e % 4]
        if e % 2:
            st.rpx[e], st.rpy[e] = cx + 0.5, cy - 0.25
    out.append(("crowded", st))
    for s in LS.SHIFTS:
        c = LS.take(st, np.arange(8 if s == LS.SHIFTS[0] else 0, 16 if s == LS.SHIFTS[0] else 8))
        c = LS.concat([c, LS.take(st, np.arange(8))])
        for f in ("hpx", "hpy", "hgx", "hgy", "rpx", "rpy", "rgx", "rgy"):
            getattr(c, f)[:] += s
        out.append(("crowded@%g" % s, c))
    return out


@functools.lru_cache(maxsize=None)
def _edge_batch(N, visible):
    rng = np.random.RandomState(9000 + 31 * N + visible)
    blocks = _blocks(rng, N, visible)
    pad, _, _ = LS._base(rng, PAD, N, (0.3,))
    parts = [st for _, st in blocks] + [pad]
    names = sum(([name] * st.E for name, st in blocks), []) + ["pad"] * PAD
    st = LS.concat(parts)
    ax, ay = rng.randint(0, 17, st.E) / 16.0, rng.randint(-4, 5, st.E) / 16.0
    return st, ax, ay, tuple(names)


def edge_batch(N, visible):
    """(EnvState, ax, ay, names): every block of BLOCK envs, then PAD plain envs (E is no multiple of any lane-group
    size).  The same states serve every parameter set of PARAMS."""
    st, ax, ay, names = _edge_batch(N, bool(visible))
    return st.copy(), ax.copy(), ay.copy(), list(names)


def trace(st, params, visible, dt=DT):
    """What each human of a batch meets, from a second, instrumented walk through the definition (plain Python floats):
    {event: [E, N] bool}.  Classifies inputs only; expected values come from tests/social_force_ref.py."""
    from tests import social_force_ref as SF
    A, B, K = params
    E, N = st.E, st.N
    keys = ("goal_tie", "goal_ulp_below", "goal_ulp_above", "on_goal", "vpref_zero", "neg_zero_e", "neg_zero_v",
            "neg_zero_w", "w_tie", "w_ulp_above", "coincident_human", "coincident_robot", "all_coincident",
            "exp_subnormal", "exp_underflow", "exp_overflow", "nonfinite_other", "nonfinite_self", "no_term",
            "robot_only", "nonfinite_w", "clipped")
    ev = {k: np.zeros((E, N), bool) for k in keys}
    P = np.stack([st.hpx, st.hpy], -1).tolist(); V = np.stack([st.hvx, st.hvy], -1).tolist()
    G = np.stack([st.hgx, st.hgy], -1).tolist(); R, S = st.hr.tolist(), st.hvpref.tolist()
    for e in range(E):
        rob = (float(st.rpx[e]), float(st.rpy[e]), float(st.rr[e])) if visible else None
        for i in range(N):
            p, v, g, r, s = P[e][i], V[e][i], G[e][i], R[e][i], S[e][i]
            ex, ey = g[0] - p[0], g[1] - p[1]
            d = math.sqrt(ex * ex + ey * ey)
            ev["goal_tie"][e, i] = d == s and s > 0
            ev["goal_ulp_below"][e, i] = 0 < s - d <= 4 * math.ulp(max(abs(g[0]), abs(g[1]), s))
            ev["goal_ulp_above"][e, i] = 0 < d - s <= 4 * math.ulp(max(abs(g[0]), abs(g[1]), s))
            ev["on_goal"][e, i] = d == 0
            ev["vpref_zero"][e, i] = s == 0
            if d > s:
                ex, ey = ex / d * s, ey / d * s
            ev["neg_zero_e"][e, i] = (ex == 0 and math.copysign(1, ex) < 0) or (ey == 0 and math.copysign(1, ey) < 0)
            ev["neg_zero_v"][e, i] = (v[0] == 0 and math.copysign(1, v[0]) < 0) or (v[1] == 0 and math.copysign(1, v[1]) < 0)
            ev["nonfinite_self"][e, i] = not (math.isfinite(p[0]) and math.isfinite(p[1]))
            others = [(P[e][j][0], P[e][j][1], R[e][j], "h") for j in range(N) if j != i]
            if rob is not None:
                others.append(rob + ("r",))
            ev["no_term"][e, i] = len(others) == 0
            ev["robot_only"][e, i] = len(others) == 1 and rob is not None
            same = 0
            for qx, qy, rj, who in others:
                if not (math.isfinite(qx) and math.isfinite(qy)):
                    ev["nonfinite_other"][e, i] = True
                dx, dy = p[0] - qx, p[1] - qy
                dist = math.sqrt(dx * dx + dy * dy)
                if dist == 0:
                    same += who == "h"
                    ev["coincident_human" if who == "h" else "coincident_robot"][e, i] = True
                elif dist > 0 and A > 0:
                    x = SF._exp((r + rj - dist) / B)
                    ev["exp_subnormal"][e, i] |= 0 < x < 2.0 ** -1022
                    ev["exp_underflow"][e, i] |= x == 0 and (r + rj - dist) / B > -1e6
                    ev["exp_overflow"][e, i] |= x == math.inf
            ev["all_coincident"][e, i] = N >= 2 and same == N - 1
            (wx, wy), _ = SF.human_velocity(p, v, g, r, s, [o[:3] for o in others], A, B, K, dt)
            ev["neg_zero_w"][e, i] = (wx == 0 and math.copysign(1, wx) < 0) or (wy == 0 and math.copysign(1, wy) < 0)
            ev["nonfinite_w"][e, i] = not (math.isfinite(wx) and math.isfinite(wy))
            if A == 0 and K == 0:                      # w = v before the clip
                n = math.sqrt(v[0] * v[0] + v[1] * v[1])
                ev["w_tie"][e, i] = n == s and s > 0
                ev["w_ulp_above"][e, i] = 0 < n - s <= 4 * math.ulp(s)
                ev["clipped"][e, i] = n > s
    return ev
