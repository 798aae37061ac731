"""Social-force pedestrians in plain Python float64: the definition the device step is tested against.

Circular form of Helbing, Farkas and Vicsek (2000) without body contact or friction.  Human i has position p, velocity
v, goal g, radius r and preferred speed s; A (m/s^2), B (m) and k (1/s) are the [social_force] strength, range and
relaxation_rate of env.config.  Every operation is one IEEE float64 operation, in this order:

  1  e = g - p; d = sqrt(e.x*e.x + e.y*e.y); if d > s: e = (e.x / d * s, e.y / d * s)
  2  a = (k*(e.x - v.x), k*(e.y - v.y))
  3  for every other human j in index order, then the robot if the humans see it:
         dx = p.x - q.x; dy = p.y - q.y; dist = sqrt(dx*dx + dy*dy)
         if dist > 0: m = A * exp((r + r_j - dist) / B); a.x = a.x + m * (dx / dist); a.y = a.y + m * (dy / dist)
  4  w = (v.x + a.x*dt, v.y + a.y*dt); n = sqrt(w.x*w.x + w.y*w.y)
  5  if n > s: w = (w.x / n * s, w.y / n * s)

The human's action is w.  Written from the definition, not from the kernel.
"""
import math


def _exp(x):
    """IEEE exp: +inf where the result overflows (math.exp raises there); NaN and -inf pass through math.exp."""
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def human_velocity(p, v, g, r, s, others, A, B, k, dt):
    """One human.  others: [(qx, qy, radius)] in the order they are added.  Returns ((wx, wy), M) with the magnitude
    M = |v| + dt * (k*(|e| + |v|) + sum_j m_ij) that an error bound of the result scales with."""
    ex, ey = g[0] - p[0], g[1] - p[1]
    d = math.sqrt(ex * ex + ey * ey)
    if d > s:
        ex, ey = ex / d * s, ey / d * s
    ax, ay = k * (ex - v[0]), k * (ey - v[1])
    msum = 0.0
    for qx, qy, rj in others:
        dx, dy = p[0] - qx, p[1] - qy
        dist = math.sqrt(dx * dx + dy * dy)
        if dist > 0:
            m = A * _exp((r + rj - dist) / B)
            ax = ax + m * (dx / dist)
            ay = ay + m * (dy / dist)
            msum += m
    wx, wy = v[0] + ax * dt, v[1] + ay * dt
    n = math.sqrt(wx * wx + wy * wy)
    if n > s:
        wx, wy = wx / n * s, wy / n * s
    vn = math.sqrt(v[0] * v[0] + v[1] * v[1])
    en = math.sqrt(ex * ex + ey * ey)
    return (wx, wy), vn + dt * (k * (en + vn) + msum)


def env_velocities(pos, vel, goal, rad, vpref, A, B, k, dt, robot=None):
    """All humans of one env.  pos / vel / goal: [N][2], rad / vpref: [N]; robot: (px, py, radius) when the humans see
    it, else None.  Returns ([N][2] actions, [N] magnitudes)."""
    n = len(pos)
    acts, mags = [], []
    for i in range(n):
        others = [(pos[j][0], pos[j][1], rad[j]) for j in range(n) if j != i]
        if robot is not None:
            others.append((robot[0], robot[1], robot[2]))
        w, m = human_velocity(pos[i], vel[i], goal[i], rad[i], vpref[i], others, A, B, k, dt)
        acts.append(w)
        mags.append(m)
    return acts, mags


def batch_velocities(hpos, hvel, hgoal, hrad, hvpref, A, B, k, dt, rpos=None, rrad=None):
    """[E,N,2] / [E,N] numpy arrays (robot: [E,2] / [E] or None) -> ([E,N,2] actions, [E,N] magnitudes)."""
    import numpy as np
    E, N = hrad.shape
    act, mag = np.zeros((E, N, 2)), np.zeros((E, N))
    P, V, G, R, S = hpos.tolist(), hvel.tolist(), hgoal.tolist(), hrad.tolist(), hvpref.tolist()
    RP = None if rpos is None else rpos.tolist()
    RR = None if rrad is None else rrad.tolist()
    for e in range(E):
        rob = None if RP is None else (RP[e][0], RP[e][1], RR[e])
        a, m = env_velocities(P[e], V[e], G[e], R[e], S[e], A, B, k, dt, rob)
        act[e], mag[e] = a, m
    return act, mag


def sanity_run(scen, A, B, k, dt, steps):
    """The crowd alone (no robot) from one scenario [N][9] (scenarios.py columns) for `steps` steps.  Returns
    (arrived humans, overlapping pair-steps, pair-steps, smallest gap)."""
    from modelcrowdnav_amd.envs import scenarios as S
    n = len(scen)
    pos = [[float(r[S.PX]), float(r[S.PY])] for r in scen]
    vel = [[float(r[S.VX]), float(r[S.VY])] for r in scen]
    goal = [[float(r[S.GX]), float(r[S.GY])] for r in scen]
    rad = [float(r[S.RAD]) for r in scen]
    vpref = [float(r[S.VPREF]) for r in scen]
    arrived = [False] * n
    overlaps, pairs, min_gap = 0, 0, float("inf")
    for _ in range(steps):
        acts, _ = env_velocities(pos, vel, goal, rad, vpref, A, B, k, dt)
        for i in range(n):
            pos[i] = [pos[i][0] + acts[i][0] * dt, pos[i][1] + acts[i][1] * dt]
            vel[i] = [acts[i][0], acts[i][1]]
            if math.hypot(pos[i][0] - goal[i][0], pos[i][1] - goal[i][1]) < rad[i]:
                arrived[i] = True
        for i in range(n):
            for j in range(i + 1, n):
                gap = math.hypot(pos[i][0] - pos[j][0], pos[i][1] - pos[j][1]) - rad[i] - rad[j]
                pairs += 1
                overlaps += gap < 0
                min_gap = min(min_gap, gap)
    return sum(arrived), overlaps, pairs, min_gap
