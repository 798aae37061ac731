"""Which arm each range guard of the four-wavefront rollout's ORCA solve takes, restated on the host (no GPU).

quad_orca_core (csrc/quad_common.hpp, QuadTable path) has five wave-uniform range guards (csrc/fast_f32.hpp): a wavefront
takes a guard's IEEE arm when some lane that USES the result holds an operand outside the fast range.

    hp    the half-plane block (orca_u_dir_rel): used = candidate in range; |w|^2 on a cut-off-circle lane, the squared leg
          and dist^2 on a leg lane
    clip  the speed-disc clip: used = |pref|^2 > ms^2; operand |pref|^2
    lp1   the speculative 1-D LP's discriminant (lp1_spread): used = !(disc < 0) on EVERY lane, the lanes of out-of-range
          candidates and of idle quads included
    lp3r  lp3_candidate_quad's 1 / |dd| and
    lp3s  its discriminant: used = kept projections, per round of the 3-D LP

A wavefront of the four-wavefront form holds the quads of 3 (3, 2) envs of its 8-env workgroup and idle quads, which are
not empty: the kernel lets them alias hand-off slot 0 and quad 0 of their wavefront (env_rollout_wg4.hip).  An idle quad
therefore runs as a GHOST of human 0 of the wavefront's first env: its position and goal, but the velocity, radius and
maximum speed of human 0 of the WORKGROUP's first env, no candidate in range (so it moves with its clipped preferred
velocity), and on all four lanes the half-plane against the real human 0, which it coincides with until the two move
differently.  Where they coincide |w|^2 is 0 on an unused lane, the fast root of 0 is NaN (v_rsq_f32(0) = inf, 0 * inf), the
line is NaN and so is lp1's discriminant, which counts as used: the ghost sends its wavefront down lp1's IEEE arm.  The
model below follows the ghost of every wavefront whose first env exists.  Quads of envs >= E are not followed: a wavefront
that holds some proves nothing for the fast arm.

Everything is float32, operation by operation as the kernel writes it, with IEEE roots and quotients: inside the fast
ranges the kernel's fast forms return the same bits (profiles/r04_fast_math.txt).  An UNUSED lane whose operand is outside
the range gets whatever the fast form returns there; that is followed only for |w|^2 = 0 and otherwise makes the
wavefront-step `unknown` for lp1.

arms(cfg, st, steps) -> per step a dict {(workgroup, wavefront): {site: "ieee" | "fast" | "unknown" | None}} (None: the site
is not reached -- no 3-D LP in that wavefront) plus, per site, whether a forcing quad sits beside a real quad of the same
wavefront whose own operands are all inside the range (`mixed`)."""
import numpy as np

from oracle import cport
from tests import lp1_spread_states as LS

f32 = np.float32
N, EW, EPW = 5, 8, 3
SITES = ("hp", "clip", "lp1", "lp3r", "lp3s")


def _bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


def sqrt5_ok(x):
    """fast_f32.hpp: positive, biased exponent 25 .. 254"""
    return ((_bits(x) - (25 << 23)) & 0xffffffff) < (230 << 23)


def half_plane(px, py, vx, vy, frad, ox, oy, ovx, ovy, orad, inv_th, inv_ts):
    """orca_u_dir_rel + the line: -> (line, lane inside the guard's range, |w|^2 == 0 on the side the lane takes)"""
    with np.errstate(all="ignore"):
        rpx, rpy = ox - px, oy - py
        d = rpx * rpx + rpy * rpy
        rvx, rvy = vx - ovx, vy - ovy
        cr = frad + orad
        cr_sq = cr * cr
        apart = bool(d > cr_sq)
        inv = inv_th if apart else inv_ts
        wx, wy = rvx - inv * rpx, rvy - inv * rpy
        wl_sq = wx * wx + wy * wy
        dp1 = wx * rpx + wy * rpy
        circle = (not apart) or (bool(dp1 < 0) and bool(dp1 * dp1 > cr_sq * wl_sq))
        leg_sq = d - cr_sq
        ok = sqrt5_ok(wl_sq) if circle else (sqrt5_ok(leg_sq) and bool(d < f32(2.0 ** 126)))
        wl = np.sqrt(wl_sq); iw = f32(1) / wl; leg = np.sqrt(leg_sq); idd = f32(1) / d
        uwx, uwy = wx * iw, wy * iw
        sc = cr * inv - wl
        cux, cuy = sc * uwx, sc * uwy
        left = bool(rpx * wy - rpy * wx > 0)
        lx, ly = (rpx * leg - rpy * cr) * idd, (rpx * cr + rpy * leg) * idd
        rx, ry = -((rpx * leg + rpy * cr) * idd), -((-rpx * cr + rpy * leg) * idd)
        gx, gy = (lx, ly) if left else (rx, ry)
        dp2 = rvx * gx + rvy * gy
        lux, luy = dp2 * gx - rvx, dp2 * gy - rvy
        dx, dy = (uwy, -uwx) if circle else (gx, gy)
        ux, uy = (cux, cuy) if circle else (lux, luy)
        line = (vx + f32(0.5) * ux, vy + f32(0.5) * uy, dx, dy)
        if circle and wl_sq == 0:
            line = (f32(np.nan),) * 4                            # either arm: 0 * (1 / 0) or 0 * (0 * inf)
    return line, d, ok, bool(circle and wl_sq == 0)


def disc_of(line, ms):
    with np.errstate(all="ignore"):
        px, py, dx, dy = line
        dp = px * dx + py * dy
        return dp * dp + ms * ms - (px * px + py * py)


def _forces(disc):
    """a used discriminant outside sqrt5's range: lp1 / lp3s"""
    return (not bool(disc < 0)) and not sqrt5_ok(disc)


def clip_of(prefx, prefy, ms):
    """-> (clipped preferred velocity, clip used and outside the range)"""
    with np.errstate(all="ignore"):
        pp = prefx * prefx + prefy * prefy
        clip = bool(pp > ms * ms)
        if not clip:
            return (prefx, prefy), False
        inv = f32(1) / np.sqrt(pp)
        return (ms * (prefx * inv), ms * (prefy * inv)), not sqrt5_ok(pp)


def _lp3_rounds(L, fail, ms, rx, ry):
    """tests.lp1_spread_states.lp3, telling per round whether a kept projection forces lp3r / lp3s"""
    out = []
    with np.errstate(all="ignore"):
        dist = f32(0)
        for i in range(fail, len(L)):
            px, py, dx, dy = L[i]
            if LS._det(dx, dy, px - rx, py - ry) > dist:
                P, fr, fs = [], False, False
                for j in range(i):
                    qx, qy, ex, ey = L[j]
                    dt = LS._det(dx, dy, ex, ey)
                    if np.abs(dt) <= LS.EPS:
                        if LS._dot(dx, dy, ex, ey) > 0:
                            continue
                        sx, sy = f32(0.5) * (px + qx), f32(0.5) * (py + qy)
                    else:
                        s = LS._det(ex, ey, px - qx, py - qy) / dt
                        sx, sy = px + s * dx, py + s * dy
                    ddx, ddy = ex - dx, ey - dy
                    dd = LS._dot(ddx, ddy, ddx, ddy)
                    fr |= not sqrt5_ok(dd)
                    inv = f32(1) / np.sqrt(dd)
                    P.append((sx, sy, ddx * inv, ddy * inv))
                    fs |= _forces(disc_of(P[-1], ms))
                fail2, nx, ny = LS.lp2(P, ms, -dy, dx, True, 2, set())
                if fail2 == len(P):
                    rx, ry = nx, ny
                dist = LS._det(dx, dy, px - rx, py - ry)
                out.append((fr, fs))
    return out


def _real_quad(cfg, st, e, i, inv_th, inv_ts):
    """human i of env e -> per site: this quad forces the IEEE arm (lp3: per round), `unknown` for lp1, the new-velocity-free
    facts only: nothing here steps the state"""
    px, py, vx, vy = f32(st.hpx[e, i]), f32(st.hpy[e, i]), f32(st.hvx[e, i]), f32(st.hvy[e, i])
    frad, ms = f32(st.hr[e, i] + 0.01 + cfg.orca_safety_space), f32(st.hvpref[e, i])
    prefx, prefy = f32(st.hgx[e, i] - st.hpx[e, i]), f32(st.hgy[e, i] - st.hpy[e, i])
    rng2 = f32(cfg.orca_neighbor_dist) * f32(cfg.orca_neighbor_dist)
    hp = lp1 = unknown = False
    lines = []
    for j in (j for j in range(N) if j != i):
        line, d, ok, w0 = half_plane(px, py, vx, vy, frad, f32(st.hpx[e, j]), f32(st.hpy[e, j]), f32(st.hvx[e, j]),
                                     f32(st.hvy[e, j]), f32(st.hr[e, j] + 0.01 + cfg.orca_safety_space), inv_th, inv_ts)
        used = bool(d < rng2)
        hp |= used and not ok
        unknown |= (not used) and (not ok) and not w0
        lp1 |= _forces(disc_of(line, ms))
        if used:
            lines.append((d, line))
    (rx, ry), clip = clip_of(prefx, prefy, ms)
    lines = [l for _, l in sorted(lines, key=lambda t: _bits(t[0]))][:cfg.orca_max_neighbors]      # stable: ties keep lane order
    rounds = []
    with np.errstate(all="ignore"):
        fail, rx, ry = LS.lp2(lines, ms, prefx, prefy, False, 3, set())
        if fail < len(lines):
            rounds = _lp3_rounds(lines, fail, ms, rx, ry)
    return dict(hp=hp, clip=clip, lp1=lp1, unknown=unknown, rounds=rounds)


class _Ghost:
    """an idle quad of wavefront w of workgroup g (see the module's docstring)"""

    def __init__(self, cfg, st, g, w):
        e0, eq = g * EW, g * EW + w * EPW
        self.eq = eq
        self.pos = np.array([st.hpx[eq, 0], st.hpy[eq, 0]], np.float64)
        self.goal = np.array([st.hgx[eq, 0], st.hgy[eq, 0]], np.float64)
        self.v = (f32(st.hvx[e0, 0]), f32(st.hvy[e0, 0]))
        self.frad, self.ms = f32(st.hr[e0, 0] + 0.01 + cfg.orca_safety_space), f32(st.hvpref[e0, 0])
        self.cand = (f32(self.pos[0]), f32(self.pos[1])) + self.v

    def look(self, inv_th, inv_ts):
        """-> (forces clip, forces lp1, unknown) before the step"""
        P = (f32(self.pos[0]), f32(self.pos[1]), f32(self.goal[0] - self.pos[0]), f32(self.goal[1] - self.pos[1]))
        line, _, ok, w0 = half_plane(P[0], P[1], self.v[0], self.v[1], self.frad, *self.cand, self.frad, inv_th, inv_ts)
        self.r, clip = clip_of(P[2], P[3], self.ms)
        return clip, _forces(disc_of(line, self.ms)), (not ok) and not w0

    def step(self, st_after, dt):
        """the kernel's integrate of the copy; the real human 0 as its quad publishes it"""
        self.pos = self.pos + np.array([float(self.r[0]), float(self.r[1])]) * dt
        self.v = self.r
        e = self.eq
        self.cand = (f32(st_after.hpx[e, 0]), f32(st_after.hpy[e, 0]), f32(st_after.hvx[e, 0]), f32(st_after.hvy[e, 0]))


def arms(cfg, st, acts):
    """The oracle steps a copy of st through acts [T, E, 2] (no restarts: no scenario pool); before every step the arm of
    every site in every ORCA wavefront.  -> [per step {(g, w): {site: arm}}], {site: mixed}"""
    st = st.copy()
    E = st.E
    inv_th, inv_ts = f32(1) / f32(cfg.orca_time_horizon), f32(1) / f32(cfg.time_step)
    ghosts = {(g, w): _Ghost(cfg, st, g, w) for g in range((E + EW - 1) // EW) for w in range(3) if g * EW + w * EPW < E}
    out, mixed = [], dict.fromkeys(SITES, False)
    for t in range(acts.shape[0]):
        now = {}
        for (g, w), ghost in ghosts.items():
            envs = [g * EW + e for e in range(w * EPW, min(w * EPW + EPW, EW))]
            whole = all(e < E for e in envs)                         # no quads of envs >= E in this wavefront
            quads = [_real_quad(cfg, st, e, i, inv_th, inv_ts) for e in envs if e < E for i in range(N)]
            gclip, glp1, gunknown = ghost.look(inv_th, inv_ts)
            arm = {}
            for site in ("hp", "clip", "lp1"):
                forced = [q[site] for q in quads]
                if any(forced):
                    arm[site] = "ieee"
                    mixed[site] |= not all(forced)
                elif not whole or (site == "lp1" and (gunknown or any(q["unknown"] for q in quads))):
                    arm[site] = "unknown"
                elif (site == "clip" and gclip) or (site == "lp1" and glp1):
                    arm[site] = "ieee"                                # the ghost alone
                else:
                    arm[site] = "fast"
            # the 3-D LP's rounds run in lockstep over the quads that are in it: round r of each at once
            depth = max([len(q["rounds"]) for q in quads] + [0])
            for k, site in ((0, "lp3r"), (1, "lp3s")):
                per_round = [[q["rounds"][r][k] for q in quads if len(q["rounds"]) > r] for r in range(depth)]
                if not depth:
                    arm[site] = None
                elif any(any(r) for r in per_round):
                    arm[site] = "ieee"
                    mixed[site] |= any(any(r) and not all(r) for r in per_round)
                else:
                    arm[site] = "fast"
                # (a step with a forced round and an unforced one takes both arms: see arms_taken)
                arm[site + "_fast_too"] = bool(depth) and any(not any(r) for r in per_round)
            now[(g, w)] = arm
        out.append(now)
        cport.env_step(cfg, st, acts[t, :, 0].copy(), acts[t, :, 1].copy(), update=True)
        for ghost in ghosts.values():
            ghost.step(st, cfg.time_step)
    return out, mixed


def arms_taken(per_step):
    """{site: {"ieee": wavefront-steps, "fast": wavefront-steps}} over a battery, certain ones only"""
    n = {s: dict(ieee=0, fast=0) for s in SITES}
    for now in per_step:
        for arm in now.values():
            for s in SITES:
                if arm[s] in ("ieee", "fast"):
                    n[s][arm[s]] += 1
                if s.startswith("lp3") and arm[s] == "ieee" and arm[s + "_fast_too"]:
                    n[s]["fast"] += 1
    return n
