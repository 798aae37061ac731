"""Boundary batches for the float64 half of a step: the robot-human swept test, the human-human overlap count, the goal
test, the reward ladder, first-arrival times, the unicycle heading and the SARL look-ahead reward.

Random float states never land exactly on a rung.  Here every block puts one env after another on one:

  * axis-aligned relative geometry makes the norms exact (sqrt(fma(0, 0, x*x)) == |x|), and the swept segment is laid
    out so that the unclamped u is exactly 0 or 1, or the segment is a point;
  * with dyadic radii (0.25, 0.375) and the dyadic discomfort_dist 0.25 the ties are dyadic and stay exact when the
    block is translated by 2^10 and 2^20;
  * with the default radius 0.3 and discomfort_dist 0.2 the float64 neighbours of the target position are searched
    until the oracle's own expression ties, e.g. (|y - ry| - hr) - rr == 0.2; such blocks are never translated.

Every constructed human keeps the others far away, so each env decides the rung it was built for; the oracle's ladder
counters (cport.ladder_counts) confirm what a batch reaches, and tests/test_oracle_ladder.py asserts that every counter
is reached in both human-count families.
"""
import functools
import math

import numpy as np

from oracle import cport

DT = 0.25
BLOCK = 16                      # one quad-kernel wavefront of envs: the rollout kernel's screens are per wavefront
PAD = 5                         # ragged E
DISCOMFORT = (0.2, 0.25)        # the reference default and a dyadic variant (dyadic radii go with it)
SHIFTS = (2.0 ** 10, 2.0 ** 20)
TWO_PI = 2 * math.pi
# (rtheta, r) pairs of the unicycle "theta" block: rtheta + r is -0.0 or a negative multiple of 2 pi (a zero fmod
# remainder of either sign), a positive multiple, or negative (a negative remainder)
THETAS = ((-0.0, -0.0), (-TWO_PI, 0.0), (-math.pi, -math.pi), (-2 * TWO_PI, 0.0), (2 * TWO_PI, 0.0), (TWO_PI, -0.0),
          (-1.0, 0.25), (-0.0, -math.pi / 4), (-7.0, 0.5), (0.5, -math.pi / 4))
# headings of every other unicycle env: rtheta + r is +-0, so cos and sin are exact and the holonomic constructions
# (robot moving along +x) carry over
FLAT_THETAS = ((-0.0, -0.0), (0.0, -0.0), (0.0, 0.0), (-0.0, 0.0))


def _grid(rng, lo, hi, shape, step):
    return rng.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape) * step


def search(f, x0, target, span=400):
    """The float64 nearest x0 (within span ulps either way) with f(x) == target, or None."""
    if f(x0) == target:
        return x0
    up = down = x0
    for _ in range(span):
        up, down = math.nextafter(up, math.inf), math.nextafter(down, -math.inf)
        if f(up) == target:
            return up
        if f(down) == target:
            return down
    return None


def _must(x, what):
    assert x is not None, "no float64 tie found for " + what
    return x


def _base(rng, E, N, radii, origin=False):
    """Robots moving along +x towards nothing (goal 6 below), humans on a lattice 1 apart, 2.5 up and left of the
    robot: no rung is decided by them.  origin: the robot at (0, 0), so that a searched human coordinate is its own
    relative coordinate (relative to a robot elsewhere, the float64 grid rarely holds a tie with radius 0.3)."""
    st = cport.EnvState(E, N)
    st.rpx[:] = _grid(rng, -2, 2, E, 1 / 8); st.rpy[:] = _grid(rng, -2, 2, E, 1 / 8)
    if origin:
        st.rpx[:] = 0.0; st.rpy[:] = 0.0
    st.rvx[:] = _grid(rng, -1, 1, E, 1 / 16); st.rvy[:] = _grid(rng, -1, 1, E, 1 / 16)
    st.rgx[:] = st.rpx; st.rgy[:] = st.rpy - 6
    st.rr[:] = rng.choice(radii, E)
    i = np.arange(N)
    st.hpx[:] = st.rpx[:, None] - 2.5 - (i % 8); st.hpy[:] = st.rpy[:, None] + 2.5 + (i // 8)
    st.hvx[:] = _grid(rng, -0.5, 0.5, (E, N), 1 / 16); st.hvy[:] = _grid(rng, -0.5, 0.5, (E, N), 1 / 16)
    st.hgx[:] = _grid(rng, -5, 5, (E, N), 1 / 8); st.hgy[:] = _grid(rng, -5, 5, (E, N), 1 / 8)
    st.hr[:] = rng.choice(radii, (E, N)); st.hvpref[:] = rng.choice((0.5, 1.0), (E, N))
    st.gtime[:] = rng.choice((0.0, 2.5, 10.25), E)
    ax = _grid(rng, 0, 1, E, 1 / 16)
    return st, ax, np.zeros(E)


def _swept(st, e, k, ax, target, mode, sign, w):
    """Human k of env e with closest swept distance minus radii == target.  Relative geometry (robot velocity (ax, 0)):
      perp   position (0, +-D), relative velocity (w, 0): u == 0 exactly
      away   position (+-D, 0), relative velocity (+-w, 0): u < 0, clamped
      u_one  position (-a, +-D), relative velocity (4a, 0): the segment ends at the foot, u == 1 exactly
      still  position (+-D, 0), relative velocity 0: the segment is a point"""
    hr, rr, rx, ry = st.hr[e, k], st.rr[e], st.rpx[e], st.rpy[e]
    D = target + hr + rr
    rvx = {"perp": w, "away": sign * w, "u_one": 4 * w, "still": 0.0}[mode]
    st.hvx[e, k], st.hvy[e, k] = ax + rvx, 0.0
    if mode in ("perp", "u_one"):
        st.hpx[e, k] = rx - (w if mode == "u_one" else 0.0)
        st.hpy[e, k] = _must(search(lambda y: abs(y - ry) - hr - rr, ry + sign * D, target), mode)
    else:
        st.hpy[e, k] = ry
        st.hpx[e, k] = _must(search(lambda x: abs(x - rx) - hr - rr, rx + sign * D, target), mode)


def _nudge(x, ref, k):
    """x moved k ulps away from ref (k < 0: towards it)."""
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if (x > ref) == (k > 0) else -math.inf)
    return x


MODES = ("perp", "away", "u_one", "still")


def _blocks(rng, N, dd):
    """(name, shiftable, EnvState, ax, ay) blocks of BLOCK envs; shiftable blocks decide the same rungs when translated
    by 2^10 and 2^20."""
    radii = (0.25, 0.375) if dd == 0.25 else (0.3,)
    dyadic = dd == 0.25
    out = []
    W = (1 / 8, 1 / 4, 1 / 2)

    def new():
        return _base(rng, BLOCK, N, radii, origin=not dyadic)

    # touching: closest distance == radii, by each segment layout; in half the envs a second human ties with it
    st, ax, ay = new()
    for e in range(BLOCK):
        k = rng.randint(N)
        sign = (1, -1)[e % 2]
        _swept(st, e, k, ax[e], 0.0, MODES[e % 4], sign, W[e % 3])
        if N >= 2 and e % 2 == 0:
            k2 = (k + 1) % N
            st.hr[e, k2] = st.hr[e, k]
            _swept(st, e, k2, ax[e], 0.0, MODES[e % 4], -sign, W[e % 3])
    out.append(("swept-touch", dyadic, st, ax, ay))
    # dmin == discomfort_dist (NOTHING) and its neighbours one and two ulps either side; mirrored ties
    st, ax, ay = new()
    for e in range(BLOCK):
        k = rng.randint(N)
        mode, sign = MODES[(e // 2) % 4], (1, -1)[e % 2]
        _swept(st, e, k, ax[e], dd, mode, sign, W[e % 3])
        if e >= 8:
            kk = 1 if mode in ("perp", "u_one") else 0
            ref = (st.rpx[e], st.rpy[e])[kk]
            pos = (st.hpx, st.hpy)[kk]
            pos[e, k] = _nudge(pos[e, k], ref, (1, -1, 2, -2)[e % 4])
        elif N >= 2 and e % 4 == 0:
            k2 = (k + 1) % N
            st.hr[e, k2] = st.hr[e, k]
            _swept(st, e, k2, ax[e], dd, mode, -sign, W[e % 3])
    out.append(("danger-edge", False, st, ax, ay))
    # collisions by each layout (a segment that is a point included), some of them deep inside the robot
    st, ax, ay = new()
    for e in range(BLOCK):
        k = rng.randint(N)
        _swept(st, e, k, ax[e], (-0.125, -0.25, -1 / 64, 0.0625)[e % 4], MODES[(e // 4) % 4], (1, -1)[e % 2], W[e % 3])
    out.append(("swept-collision", True, st, ax, ay))
    # the goal disc: |end - goal| == rr exactly (not reaching), and within +-1e-6 of it (the rollout screen's band)
    st, ax, ay = new()
    for e in range(BLOCK):
        ex, ey = st.rpx[e] + ax[e] * DT, st.rpy[e] + 0.0 * DT
        sign = (1, -1)[e % 2]
        st.rgy[e] = ey
        if e < 4:
            st.rgx[e] = _must(search(lambda g: abs(ex - g), ex + sign * st.rr[e], st.rr[e]) or
                              search(lambda g: abs(ex - g), ex - sign * st.rr[e], st.rr[e]), "reach edge")
        else:
            st.rgx[e] = ex + sign * (st.rr[e] + (-9e-7, -5e-7, -1e-7, 1e-7, 5e-7, 9.9e-7)[e % 6])
    out.append(("reach-edge", False, st, ax, ay))
    # reaching while colliding (collision wins), timeouts at time_limit - 1 and one ulp below, timeout + collision
    st, ax, ay = new()
    for e in range(BLOCK):
        k = rng.randint(N)
        if e % 4 != 3:
            _swept(st, e, k, ax[e], -0.125, MODES[e % 4], 1, W[e % 3])
        if e % 4 == 0:
            st.rgx[e], st.rgy[e] = st.rpx[e] + ax[e] * DT, st.rpy[e]
        st.gtime[e] = (24.0, math.nextafter(24.0, 0.0), 10.25, 24.0)[(e // 4) % 4] if e % 2 else st.gtime[e]
    out.append(("ladder-mix", True, st, ax, ay))
    if N >= 2:
        # human-human gaps: exactly 0, and within 1e-6 of it either side (nothing else in the block overlaps)
        st, ax, ay = new()
        for e in range(BLOCK):
            # i moves to x == 0 in its row (right of the lattice, above the robot), j to the right of it
            i, j = N - 1, rng.randint(N - 1)
            hi, hj = st.hr[e, i], st.hr[e, j]
            st.hpx[e, i], st.hpy[e, j] = 0.0, st.hpy[e, i]
            if e < 6:
                st.hpx[e, j] = _must(search(lambda x: ((0.0 - x) * (0.0 - x)) ** 0.5 - hi - hj, hi + hj, 0.0),
                                     "hh touch")
            else:
                st.hpx[e, j] = hi + hj + (-9e-7, -5e-7, -1e-7, 1e-7, 5e-7)[e % 5]
        out.append(("hh-band6", False, st, ax, ay))
        # gaps 1e-6 .. 1e-3 either side: the float32 pre-filter's borderline band
        st, ax, ay = new()
        for e in range(BLOCK):
            i, j = N - 1, rng.randint(N - 1)
            g = (2e-6, 1e-5, 1e-4, 5e-4, 9.9e-4, 3e-6, 3e-5, 7e-4)[e % 8] * (1, -1)[(e // 8) % 2]
            st.hpx[e, j] = st.hpx[e, i]
            st.hpy[e, j] = st.hpy[e, i] + st.hr[e, i] + st.hr[e, j] + g
        out.append(("hh-band3", False, st, ax, ay))
        # non-dyadic pairs near 2^9 with float64 gaps of +-2e-7 whose float32-rounded positions fall on the other side
        # of touching
        out.append(("hh-f32-flip", False) + _f32_flip(rng, N, radii))
    # first arrival: a human (radius 0.375, v_pref 0.5, neighbours at rest) half a metre below its goal walks
    # 0.125 straight up and ends exactly one radius from it (not arrived)
    st, ax, ay = new()
    st.hvx[:] = 0; st.hvy[:] = 0
    for e in range(BLOCK):
        k = N - 1 - rng.randint(min(N, 8))
        st.hr[e, k], st.hvpref[e, k] = 0.375, 0.5
        st.hgx[e, k], st.hgy[e, k] = st.hpx[e, k], st.hpy[e, k] + 0.5
    out.append(("human-time-edge", True, st, ax, ay))
    # headings (unicycle): zero remainders of both signs, negative remainders
    st, ax, ay = new()
    out.append(("theta", True, st, ax, ay))
    st, ax, ay = new()
    out.append(("random", True, st, ax, ay))
    return out


def _f32_flip(rng, N, radii):
    st, ax, ay = _base(rng, BLOCK, N, radii)
    f32 = np.float32
    for e in range(BLOCK):
        i, j = N - 1, rng.randint(N - 1)
        g = (2e-7, -2e-7)[e % 2]
        hi, hj = st.hr[e, i], st.hr[e, j]
        R = f32(hi) + (f32(hj + 0.01) - f32(0.01) - f32(0.0))
        for _ in range(10000):
            cx, cy = 512 + rng.uniform(-4, 4), 512 + rng.uniform(-4, 4)
            phi = rng.uniform(0, 2 * np.pi)
            D = hi + hj + g
            qx, qy = cx + D * np.cos(phi), cy + D * np.sin(phi)
            gap64 = ((cx - qx) ** 2 + (cy - qy) ** 2) ** 0.5 - hi - hj
            dx, dy = f32(cx) - f32(qx), f32(cy) - f32(qy)
            gap32 = float(np.sqrt(f32(dx * dx + dy * dy))) - float(R)
            if gap64 != 0 and abs(gap64) <= 1e-6 and (gap64 < 0) != (gap32 < 0) and abs(gap32) > 1e-5:
                break
        else:
            raise AssertionError("no float32 sign flip found")
        # the whole env moves with the pair, keeping the rest of the layout
        off_x, off_y = cx - st.hpx[e, i], cy - st.hpy[e, i]
        for a in ("hpx", "hgx"):
            getattr(st, a)[e] += off_x
        for a in ("hpy", "hgy"):
            getattr(st, a)[e] += off_y
        st.rpx[e] += off_x; st.rgx[e] += off_x; st.rpy[e] += off_y; st.rgy[e] += off_y
        st.hpx[e, i], st.hpy[e, i], st.hpx[e, j], st.hpy[e, j] = cx, cy, qx, qy
    return st, ax, ay


def _fields():
    return cport.EnvState.FIELDS_H + cport.EnvState.FIELDS_R + ("gtime", "rtheta", "human_times")


def concat(sts):
    o = cport.EnvState(sum(s.E for s in sts), sts[0].N)
    for k in _fields():
        setattr(o, k, np.ascontiguousarray(np.concatenate([getattr(s, k) for s in sts], 0)))
    return o


def take(st, idx):
    o = cport.EnvState(len(idx), st.N)
    for k in _fields():
        setattr(o, k, np.ascontiguousarray(getattr(st, k)[idx]))
    return o


def cfg(visible, dd=0.2, count_hh=True, unicycle=False, policy=cport.HUMANS_ORCA):
    """The oracle config of a ladder batch (env defaults, track_human_times on)."""
    return cport.default_cfg(robot_visible=1 if visible else 0, discomfort_dist=dd, count_hh=1 if count_hh else 0,
                             track_human_times=1, robot_unicycle=1 if unicycle else 0, human_policy=policy)


@functools.lru_cache(maxsize=None)
def _ladder_batch(N, visible, dd, unicycle, seed):
    rng = np.random.RandomState(seed * 7919 + 37 * N + 13 * visible + int(dd * 100) + 3 * unicycle)
    blocks = _blocks(rng, N, dd)
    parts, axs, ays, names = [], [], [], []
    for name, _, st, ax, ay in blocks:
        parts.append(st); axs.append(ax); ays.append(ay); names += [name] * st.E
    for s in SHIFTS:
        for name, shiftable, st, ax, ay in blocks:
            if not shiftable:
                continue
            c = concat([st])
            for k in ("hpx", "hpy", "hgx", "hgy", "rpx", "rpy", "rgx", "rgy"):
                getattr(c, k)[:] += s
            parts.append(c); axs.append(ax); ays.append(ay); names += ["%s@%g" % (name, s)] * st.E
    pad, pax, pay = _base(rng, PAD, N, (0.3,))
    parts.append(pad); axs.append(pax); ays.append(pay); names += ["pad"] * PAD
    st = concat(parts)
    ax, ay = np.concatenate(axs), np.concatenate(ays)
    if unicycle:
        for e, name in enumerate(names):
            th = THETAS[e % len(THETAS)] if name.startswith("theta") else FLAT_THETAS[e % len(FLAT_THETAS)]
            st.rtheta[e], ay[e] = th
            if th[0] + th[1] != 0:
                ax[e] = 0.0         # turning on the spot: no rung depends on device against host trig
    # the humans' ORCA velocities, for the given-velocity paths (the same next positions, so the same arrivals)
    ref = cport.env_step(cfg(visible, dd, unicycle=unicycle), st.copy(), ax, ay, update=False)
    return st, ax, ay, ref["human_act"].copy(), tuple(names)


def ladder_batch(N, visible, dd=0.2, unicycle=False, seed=0):
    """One batch of N-human envs: every block, the dyadic ones also translated by 2^10 and 2^20, then PAD random envs
    (ragged E).  Returns (EnvState, ax, ay, given_v [E,N,2], names) with names[e] the block of env e; unicycle batches
    hold (v, r) actions and headings.  Built once per process; the caller gets its own copy."""
    st, ax, ay, gv, names = _ladder_batch(N, bool(visible), float(dd), bool(unicycle), seed)
    return st.copy(), ax.copy(), ay.copy(), gv.copy(), list(names)


# ----------------------------------------------------------------------------------------- look-ahead reward
def lookahead_table(speeds=5, rotations=16):
    """A holonomic action table shaped like cadrl.build_action_space (speed 0 first)."""
    sp = [(np.exp((i + 1) / speeds) - 1) / (np.e - 1) for i in range(speeds)]
    rot = np.linspace(0, 2 * np.pi, rotations, endpoint=False)
    return np.array([(0.0, 0.0)] + [(s * np.cos(r), s * np.sin(r)) for s in sp for r in rot])


@functools.lru_cache(maxsize=None)
def _lookahead_batch(N, table_key, seed):
    table = np.array(table_key).reshape(-1, 2)
    rng = np.random.RandomState(seed * 104729 + 41 * N)
    A = len(table)
    parts, names = [], []
    kinds = ["la-touch", "la-danger-edge", "la-reach-edge", "la-at-goal-edge", "la-at-goal", "random"]
    if N >= 3:
        kinds.insert(3, "la-collision-after-min")
    for kind in kinds:
        st, _, _ = _base(rng, BLOCK, N, (0.3, 0.25, 0.375))
        for e in range(BLOCK):
            rr = st.rr[e]
            k = rng.randint(N)
            sign = (1, -1)[e % 2]
            for _ in range(256):        # an action (and radii) whose next position admits the tie
                a = table[rng.randint(1, A)]
                nx, ny = st.rpx[e] + a[0] * DT, st.rpy[e] + a[1] * DT
                if kind in ("la-touch", "la-danger-edge"):
                    t = 0.0 if kind == "la-touch" else 0.2
                    rr, hr = rng.choice((0.3, 0.25, 0.375), 2)     # (not every pair of radii admits a tie)
                    x = search(lambda x: abs(nx - x) - rr - hr, nx + sign * (t + rr + hr), t)
                    if x is not None:
                        st.hvx[e, k], st.hvy[e, k], st.hpx[e, k], st.hpy[e, k] = 0.0, 0.0, x, ny
                        st.hr[e, k], st.rr[e] = hr, rr
                        break
                elif kind == "la-reach-edge":
                    rr = rng.choice((0.3, 0.25, 0.375))
                    g = search(lambda g: abs(nx - g), nx + sign * rr, rr)
                    if g is not None:
                        st.rgx[e], st.rgy[e], st.rr[e] = g, ny, rr
                        break
                else:
                    break
            else:
                raise AssertionError("no float64 tie found for " + kind)
            if kind == "la-collision-after-min":
                st.hvx[e, 1], st.hvy[e, 1] = 0.0, 0.0
                st.hpx[e, 1], st.hpy[e, 1] = nx + 0.125 * sign, ny
            elif kind == "la-at-goal-edge":
                st.rgy[e] = st.rpy[e]
                st.rr[e] = rr = (0.25, 0.375)[e % 2]
                f = lambda g: abs(st.rpx[e] - g)
                st.rgx[e] = _must(search(f, st.rpx[e] + sign * rr, rr) or search(f, st.rpx[e] - sign * rr, rr), kind)
            elif kind == "la-at-goal":
                st.rgx[e], st.rgy[e] = st.rpx[e] + 0.125 * sign, st.rpy[e]
        parts.append(st); names += [kind] * BLOCK
    pad, _, _ = _base(rng, PAD, N, (0.3,))
    parts.append(pad); names += ["pad"] * PAD
    return concat(parts), tuple(names)


def lookahead_batch(N, table, seed=0):
    """Envs whose look-ahead reward for one action of `table` sits on a rung: a human touching the robot's next
    position, dmin == 0.2, the next position exactly one radius from the goal, a collision behind a nearer human, and
    robots already exactly one radius from their goal (the argmax kernel goes on) or inside it (-1).
    Returns (EnvState, names)."""
    st, names = _lookahead_batch(N, tuple(np.asarray(table, np.float64).ravel()), seed)
    return st.copy(), list(names)
