"""Edge batches for the LSTM-RL / CADRL look-ahead (lstm_rl_value.hip) and its human order (HumanOrder,
mcn_lstm_rl_order), as oracle EnvStates with one name per env.

  * order_batch: exact distance ties (mirrored, duplicated, a human on the robot), sub-ulp near-ties on which the fused
    norm sqrt(fma(y, y, x*x)) -- numpy's 2-vector norm, and norm2d on the device -- and the un-fused x*x + y*y disagree,
    +inf positions (one, and two tied), a NaN position at slot 0 / in the middle / at the end, every position NaN, a
    NaN robot, and NaN / +-inf humans beyond an env's hcount;
  * feature_batch: actions that land the robot exactly on its goal (dg == 0), a propagated human exactly on the robot's
    next position (feature 11 == 0), zero human velocities.

Every oracle here is numpy (policy_ref.stable_desc_order) or torch; the CPU self-tests (tests/test_policies_cpu.py)
confirm that the near-tie batch holds what it claims."""
import math
from fractions import Fraction

import numpy as np

from oracle import cport
from tests import helpers as H
from tests import ladder_states as LS

GRID = 2.0 ** -48               # coordinate grid of the tie constructions: robot + offset stays exact for |x| < 8


def fused_norm(x, y):
    """sqrt(fma(y, y, x*x)) in float64, the fma rounded once (exact rational arithmetic)."""
    if not (math.isfinite(x) and math.isfinite(y)):
        return math.sqrt(y * y + x * x) if not (math.isnan(x) or math.isnan(y)) else math.nan
    return math.sqrt(float(Fraction(y) * Fraction(y) + Fraction(x * x)))


def unfused_norm(x, y):
    return math.sqrt(x * x + y * y)


def desc_order(d):
    """First strict maximum, ties in index order, NaN last in index order (the rule of stable_desc_order)."""
    return np.argsort(-np.asarray(d, np.float64), kind="stable")


def orders(st, e, norm):
    """The human order of env e of st under the 2-vector norm `norm` (of the offsets human - robot)."""
    d = [norm(st.hpx[e, i] - st.rpx[e], st.hpy[e, i] - st.rpy[e]) for i in range(st.N)]
    return desc_order(d)


def _fresh(rng, E, N):
    st = H.random_state(rng, E, N, randomize=True)
    st.rpx[:] = rng.randint(-16, 17, E) / 8.0
    st.rpy[:] = rng.randint(-16, 17, E) / 8.0
    return st


def _offset(rng, v):
    """v rounded to GRID, with a random sign."""
    return float(np.round(v / GRID) * GRID) * rng.choice((-1.0, 1.0))


def _place(st, e, i, dx, dy):
    st.hpx[e, i], st.hpy[e, i] = st.rpx[e] + dx, st.rpy[e] + dy
    assert st.hpx[e, i] - st.rpx[e] == dx and st.hpy[e, i] - st.rpy[e] == dy


def _near_tie_env(rng, st, e):
    """Groups of humans whose distances are sub-ulp apart or equal: (x, y) and (y, x) tie under the un-fused norm
    (x*x + y*y == y*y + x*x) but, for about half of them, not under the fused one; (-x, y) ties under both.  The
    groups sit at different radii, in shuffled slots."""
    N = st.N
    slots = rng.permutation(N)
    k = 0
    while k < N:
        r0 = rng.uniform(0.5, 3.0)
        a = rng.uniform(0.1, 1.4)
        x, y = _offset(rng, r0 * math.cos(a)), _offset(rng, r0 * math.sin(a))
        for dx, dy in ((x, y), (y, x), (-x, y), (y, -x))[:min(4, N - k)]:
            _place(st, e, slots[k], dx, dy)
            k += 1


def near_tie_batch(N, E=48, seed=0):
    """E envs of near-tie groups.  The fused and un-fused orders differ in a good part of them."""
    rng = np.random.RandomState(seed * 7907 + N)
    st = _fresh(rng, E, N)
    for e in range(E):
        _near_tie_env(rng, st, e)
    return st


def tie_env(rng, st, e):
    """Exact ties under any norm: mirrored through the robot, duplicated, and a human on the robot."""
    N = st.N
    dx, dy = rng.randint(1, 12) / 8.0, rng.randint(1, 12) / 8.0
    _place(st, e, 0, dx, -dy)
    if N > 1:
        _place(st, e, 1, -dx, dy)
    if N > 2:
        _place(st, e, 2, dx, -dy)
    if N > 3:
        _place(st, e, N - 1, 0.0, 0.0)
    if N > 5:
        _place(st, e, N // 2, dy, dx)


def tie_state_eighth_grid(rng, E, N, kinematics="holonomic"):
    """random_state with tie_env in every 3rd env (robot as drawn, offsets on eighths).  tests/test_lookahead_edges_gpu.py."""
    st = H.random_state(rng, E, N, randomize=True)
    for e in range(0, E, 3):
        tie_env(rng, st, e)
    if kinematics == "unicycle":
        st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)
    return st


def tie_state_quarter_grid(rng, E, N):
    """random_state with exact distance ties in every 3rd env: the robot on a quarter grid, humans mirrored through it,
    duplicated, and one on the robot.  N >= 4.  tests/test_lstm_rl_gpu.py."""
    st = H.random_state(rng, E, N, randomize=True)
    for e in range(0, E, 3):
        st.rpx[e], st.rpy[e] = rng.randint(-8, 9, 2) * 0.25
        st.hpx[e, 0], st.hpy[e, 0] = st.rpx[e] + 0.625, st.rpy[e] - 1.25
        st.hpx[e, 1], st.hpy[e, 1] = st.rpx[e] - 0.625, st.rpy[e] + 1.25       # mirrored through the robot
        st.hpx[e, 2], st.hpy[e, 2] = st.hpx[e, 0], st.hpy[e, 0]                 # duplicate
        st.hpx[e, N - 1], st.hpy[e, N - 1] = st.rpx[e], st.rpy[e]               # on the robot
    return st


# the env kinds of order_batch; "mid" is slot N // 2, "end" slot N - 1
ORDER_KINDS = ("ties", "near-tie", "inf", "inf-tie", "nan-first", "nan-mid", "nan-end", "nan-first-and-end",
               "all-nan", "nan-robot", "nonfinite-beyond-hcount", "random")


def order_batch(N, per_kind=6, seed=0):
    """Returns (EnvState, hcount [E] int32, names): per_kind envs of every kind, the 'near-tie' kind as a whole
    near_tie_batch.  hcount is N except in the 'nonfinite-beyond-hcount' envs, whose humans from hcount on are NaN /
    +-inf, and in half of the 'random' ones."""
    rng = np.random.RandomState(seed * 104723 + 17 * N)
    kinds = [k for k in ORDER_KINDS if k != "near-tie" for _ in range(per_kind)]
    E = len(kinds)
    st = _fresh(rng, E, N)
    hc = np.full(E, N, np.int32)
    mid, end = N // 2, N - 1
    for e, kind in enumerate(kinds):
        if kind == "ties":
            tie_env(rng, st, e)
        elif kind == "inf":
            i = rng.randint(N)
            st.hpx[e, i] = (np.inf, -np.inf)[e % 2]
        elif kind == "inf-tie":
            tie_env(rng, st, e)
            st.hpx[e, 0] = np.inf
            st.hpy[e, end] = -np.inf
            if N > 2:
                st.hpy[e, mid] = np.inf
        elif kind.startswith("nan") and kind != "nan-robot":
            where = {"nan-first": [0], "nan-mid": [mid], "nan-end": [end], "nan-first-and-end": [0, end]}[kind]
            if e % 2 and N > 3:
                tie_env(rng, st, e)
            for i in where:
                (st.hpx, st.hpy)[e % 2][e, i] = np.nan
        elif kind == "all-nan":
            st.hpx[e, :] = np.nan
        elif kind == "nan-robot":
            (st.rpx, st.rpy)[e % 2][e] = np.nan
        elif kind == "nonfinite-beyond-hcount":
            n = 1 + (e % N) if N > 1 else 1
            hc[e] = n
            if n < N:
                st.hpx[e, n:] = np.nan
                st.hpy[e, n::2] = np.inf
                st.hpx[e, n + 1::3] = -np.inf
        elif kind == "random" and e % 2:
            hc[e] = rng.randint(1, N + 1)
    near = near_tie_batch(N, seed=seed)
    st = LS.concat([st, near])
    return st, np.concatenate([hc, np.full(near.E, N, np.int32)]), kinds + ["near-tie"] * near.E


def fused_unfused_disagreements(st):
    """Envs of st whose human order differs between the fused and the un-fused norm."""
    return [e for e in range(st.E) if not np.array_equal(orders(st, e, fused_norm), orders(st, e, unfused_norm))]


# ----------------------------------------------------------------------------------------- feature edges
FEATURE_KINDS = ("on-goal", "human-on-next", "human-on-next-moving", "still-humans", "random")


def feature_batch(N, table, kinematics="holonomic", per_kind=4, seed=0, dt=0.25):
    """Returns (EnvState, names, act [E]): in env e, action act[e] of `table` gives the edge named:
      on-goal               -- the robot's next position is exactly its goal (dg == 0: cr = 1, sr = 0; for unicycle
                               f_theta = nth - atan2(0, 0)); rr 0.2, so a speed-1 action leaves from outside the goal,
                               while row 0 (speed 0) of a unicycle table stays on the goal it already stands on;
      human-on-next         -- a still human exactly on the robot's next position (feature 11 == 0, a collision);
      human-on-next-moving  -- the same for a human moving by a dyadic step into it;
      still-humans          -- every human velocity zero.
    Unicycle headings are chosen so that rtheta + r == 0 for the chosen action: cos and sin are exact."""
    rng = np.random.RandomState(seed * 7919 + 31 * N + (kinematics == "unicycle"))
    kinds = [k for k in FEATURE_KINDS for _ in range(per_kind)]
    E = len(kinds)
    st = _fresh(rng, E, N)
    act = np.zeros(E, np.int64)
    table = np.asarray(table, np.float64)
    A = len(table)
    fast = [a for a in range(1, A) if (table[a, 0] if kinematics == "unicycle" else np.hypot(*table[a])) > 0.9]
    for e, kind in enumerate(kinds):
        a = int(fast[rng.randint(len(fast))])
        if kind == "on-goal" and kinematics == "unicycle" and e % 2:
            a = 0
        act[e] = a
        if kinematics == "unicycle":
            st.rtheta[e] = -table[a, 1] if a else rng.uniform(-3, 3)
            nth = st.rtheta[e] + table[a, 1]
            nvx, nvy = table[a, 0] * np.cos(nth), table[a, 0] * np.sin(nth)
            assert a == 0 or (nth == 0.0 and nvy == 0.0)
        else:
            nvx, nvy = table[a]
        npx, npy = st.rpx[e] + nvx * dt, st.rpy[e] + nvy * dt
        i = rng.randint(N)
        if kind == "on-goal":
            st.rr[e] = 0.2
            st.rgx[e], st.rgy[e] = npx, npy
        elif kind == "human-on-next":
            st.hpx[e, i], st.hpy[e, i], st.hvx[e, i], st.hvy[e, i] = npx, npy, 0.0, 0.0
        elif kind == "human-on-next-moving":
            vx, vy = rng.choice((-0.5, 0.5, 1.0)), rng.choice((-0.5, 0.0, 0.5))
            st.hpx[e, i], st.hpy[e, i] = npx - vx * dt, npy - vy * dt
            st.hvx[e, i], st.hvy[e, i] = vx, vy
            assert st.hpx[e, i] + vx * dt == npx and st.hpy[e, i] + vy * dt == npy
        elif kind == "still-humans":
            st.hvx[e, :] = 0.0
            st.hvy[e, :] = 0.0
    return st, kinds, act


def nonfinite_beyond(st, hc, seed=0):
    """A copy of st whose humans from hc[e] on are NaN, +inf or -inf (positions and velocities)."""
    rng = np.random.RandomState(seed)
    o = st.copy()
    for e in range(o.E):
        n = int(hc[e])
        for i in range(n, o.N):
            v = (np.nan, np.inf, -np.inf)[rng.randint(3)]
            for f in ("hpx", "hpy", "hvx", "hvy", "hr"):
                if rng.randint(2) or f == "hpx":
                    getattr(o, f)[e, i] = v
    return o

