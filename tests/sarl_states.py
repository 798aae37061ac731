"""Inputs and CPU references of the SARL edge suite (tests/test_sarl_edges_gpu.py; self-tests in
tests/test_sarl_states_cpu.py).

  * networks built from the recorded g5 weights (tests/golden/g5_sarl.npz, `w0__*`): `attention.4.bias` shifted so that the
    un-stabilised masked softmax of sarl.py:52-53 lands in each of its classes, every attention parameter zero (all
    scores exactly 0: 0 / 0), a hand-set unit that scores chosen humans exactly 0 among others, and a network whose V is
    exactly 0;
  * seeded state batches without a robot on its goal, non-finite values placed in one env's state or in action rows;
  * value rows for sarl_argmax_kernel: exact ties across the lanes and the 64-strides of its scan, +-inf, NaN, subnormal
    gaps;
  * the reference: oracle/pyref (rotate, sarl_forward, lookahead_reward) on the CPU, float32 as the reference runs it,
    float64 on the same float32 features as the yardstick."""
import os

import numpy as np
import torch

from oracle import pyref
from tests import helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DT, GAMMA = 0.25, 0.9
DISC = GAMMA ** (DT * 1.0)              # multi_human_rl.py:52 with v_pref = 1

# shifts of attention.4.bias and the class of the float32 reference's softmax there (scores of the g5 network are
# nearly constant, so the shift is the score).  Between +88 and +89 and between -100 and -104 one ulp of exp decides the
# class of the reference itself: nothing is asserted there.
FINITE_SHIFTS = (0.0, 80.0, -80.0, -90.0, -92.0)
YARDSTICK_SHIFTS = (0.0, 80.0, -80.0)       # 2 x torch-float32 error + 5e-7 against float64 holds here
NAN_SHIFTS = (100.0, -110.0)                # every exp overflows: inf / inf; every exp underflows to 0: 0 / 0
TINY_SUM = 2.0 ** -128                      # below it the float32 reciprocal of the sum overflows


def g5_weights(seed=0):
    """{state_dict name: float32 tensor} of the reference-side network recorded in g5_sarl.npz."""
    g = np.load(os.path.join(GOLDEN, "g5_sarl.npz"))
    prefix = "w%d__" % seed
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(g[k].copy()) for k in g.files if k.startswith(prefix)}


def shifted(w, shift):
    o = {k: v.clone() for k, v in w.items()}
    o["attention.4.bias"] += np.float32(shift)
    return o


def zero_attention(w):
    """Every attention parameter zero: every score is exactly 0, the masked softmax 0 / 0."""
    return {k: (torch.zeros_like(v) if k.startswith("attention.") else v.clone()) for k, v in w.items()}


def zero_value_network(w):
    """Every parameter zero except attention.4.bias = 1: every score 1, uniform weights, mlp2 and mlp3 zero: V == 0.0
    exactly, in the reference too (an all-zero network is 0 / 0 = NaN)."""
    o = {k: torch.zeros_like(v) for k, v in w.items()}
    o["attention.4.bias"] += 1.0
    return o


MIXED_RADIUS_EDGE, MIXED_GAIN = 0.375, 8.0


def mixed_network(w):
    """g5 with unit 0 of mlp1.0, mlp1.2, attention.0 and attention.2 set by hand: unit 0 carries relu(radius - 0.375)
    through one-hot rows (exact in float32 and in three bfloat16 pieces), attention.4 reads only that unit.  A human of
    radius 0.25 scores exactly 0 and drops out of the softmax, one of radius 0.5 scores 8 * 0.125 = 1."""
    o = {k: v.clone() for k, v in w.items()}

    def one_hot(name, col, bias):
        o[name + ".weight"][0].zero_()
        o[name + ".weight"][0, col] = 1.0
        o[name + ".bias"][0] = bias
    one_hot("mlp1.0", 10, -MIXED_RADIUS_EDGE)           # feature 10: the human's radius
    one_hot("mlp1.2", 0, 0.0)
    one_hot("attention.0", 0, 0.0)                      # column 0 of the local half
    one_hot("attention.2", 0, 0.0)
    o["attention.4.weight"].zero_()
    o["attention.4.weight"][0, 0] = MIXED_GAIN
    o["attention.4.bias"].zero_()
    return o


def mixed_radii(E, N, seed=0):
    """[E,N] radii 0.25 (score exactly 0) / 0.5: env 0 all 0.5, env 1 all 0.25 (0 / 0), the others mixed with at least
    one of each where N > 1."""
    rng = np.random.RandomState(900 + seed)
    r = np.where(rng.uniform(size=(E, N)) < 0.5, 0.25, 0.5)
    r[0, :] = 0.5
    if E > 1:
        r[1, :] = 0.25
    for e in range(2, E):
        if N > 1:
            r[e, e % N], r[e, (e + 1) % N] = 0.25, 0.5
    return r


# ------------------------------------------------------------------------------------------------ states
def reached(st):
    """policy.py:43-49 per env: the robot already stands on its goal, nothing is evaluated."""
    return np.array([float(np.linalg.norm((st.rpy[e] - st.rgy[e], st.rpx[e] - st.rgx[e]))) < st.rr[e] for e in range(st.E)])


def states(seed, E, N, kinematics="holonomic", on_goal=()):
    """helpers.random_state with every goal at least 0.5 from the robot (no env is skipped), except the envs listed in
    `on_goal`."""
    rng = np.random.RandomState(7000 + 131 * seed + N)
    st = H.random_state(rng, E, N, randomize=True)
    for e in range(E):
        if np.hypot(st.rgx[e] - st.rpx[e], st.rgy[e] - st.rpy[e]) < 0.5:
            st.rgx[e], st.rgy[e] = st.rpx[e] + 1.5, st.rpy[e] - 0.75
    for e in on_goal:
        st.rgx[e], st.rgy[e] = st.rpx[e] + 0.0625, st.rpy[e] - 0.0625
    if kinematics == "unicycle":
        st.rtheta[:] = rng.uniform(-3, 3, E)
    return st


SOFTMAX_NS, SOFTMAX_NAN_NS = (5, 10), (1, 5, 10)


def softmax_batch(N):
    """The states of the softmax-class tests (8 envs x 81 actions = 648 rows per N)."""
    return states(1, 8, N)


POISON_VALUES = (("nan+", np.nan), ("nan-", np.copysign(np.nan, -1.0)), ("inf+", np.inf), ("inf-", -np.inf))
POISON_PLACES = ("hpx", "hpy", "hvx", "hvy", "hr", "rpx", "rpy", "rgx", "rgy")
assert not np.signbit(POISON_VALUES[0][1]) and np.signbit(POISON_VALUES[1][1])


def poison_batch(N, seed=0):
    """Returns (clean, poisoned, names): names[e] is None for the clean even envs and "place:value" for the odd ones,
    each holding one non-finite value in a present human's position, velocity or radius or in the robot's position or
    goal.  With 81 actions an env's pairs start at 81 e, which is no multiple of 16 for odd e: every poisoned env
    shares its first 16-pair tile with the clean env before it (and, but for e = 15, its last with the one after)."""
    combos = [(p, v) for p in POISON_PLACES for v in POISON_VALUES]
    E = 2 * len(combos) + 1
    clean = states(50 + seed, E, N)
    bad = clean.copy()
    names = [None] * E
    for k, (place, (vname, v)) in enumerate(combos):
        e = 2 * k + 1
        if place.startswith("h"):
            getattr(bad, place)[e, k % N] = v
        else:
            getattr(bad, place)[e] = v
        names[e] = "%s:%s" % (place, vname)
    return clean, bad, names


def poison_beyond(st, hcount, seed=0):
    """A copy of st with every POISON_VALUES entry in the slots from hcount[e] on."""
    rng = np.random.RandomState(seed)
    o = st.copy()
    for e in range(o.E):
        for i in range(int(hcount[e]), o.N):
            for f in ("hpx", "hpy", "hvx", "hvy", "hr"):
                getattr(o, f)[e, i] = POISON_VALUES[rng.randint(4)][1]
    return o


POISON_ROWS = {3: 0, 17: 1, 40: 2, 80: 3}       # action-table row -> index into POISON_VALUES


def poison_table(table):
    t = np.array(table, np.float64)
    for row, k in POISON_ROWS.items():
        t[row, row % 2] = POISON_VALUES[k][1]
    return t


def classes(v):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 1, np.where(np.isposinf(v), 2, np.where(np.isneginf(v), 3, 0)))


# ------------------------------------------------------------------------------------------------ reference
def joint_rows(st, e, table, kinematics="holonomic", n=None, nexts=None):
    """([A,n,14] float64 rows of MultiHumanRL.predict for env e: the robot after each action beside each of the first n
    humans' next states (constant velocity, or nexts = ([N,2] positions, [N,2] velocities)); next humans [n,5])."""
    n = st.N if n is None else n
    table = np.asarray(table, np.float64)
    A = len(table)
    if nexts is None:
        hx, hy = st.hpx[e, :n] + st.hvx[e, :n] * DT, st.hpy[e, :n] + st.hvy[e, :n] * DT
        hvx, hvy = st.hvx[e, :n], st.hvy[e, :n]
    else:
        hx, hy, hvx, hvy = nexts[0][:n, 0], nexts[0][:n, 1], nexts[1][:n, 0], nexts[1][:n, 1]
    if kinematics == "unicycle":
        nth = st.rtheta[e] + table[:, 1]
        nvx, nvy = table[:, 0] * np.cos(nth), table[:, 0] * np.sin(nth)
    else:
        nth, nvx, nvy = np.full(A, st.rtheta[e]), table[:, 0], table[:, 1]
    rows = np.empty((A, n, 14))
    rows[:, :, 0] = (st.rpx[e] + nvx * DT)[:, None]
    rows[:, :, 1] = (st.rpy[e] + nvy * DT)[:, None]
    rows[:, :, 2], rows[:, :, 3] = nvx[:, None], nvy[:, None]
    rows[:, :, 4], rows[:, :, 5], rows[:, :, 6], rows[:, :, 7] = st.rr[e], st.rgx[e], st.rgy[e], 1.0
    rows[:, :, 8] = nth[:, None]
    rows[:, :, 9], rows[:, :, 10], rows[:, :, 11], rows[:, :, 12] = hx[None], hy[None], hvx[None], hvy[None]
    rows[:, :, 13] = st.hr[e, :n][None]
    return rows, np.stack([hx, hy, hvx, hvy, st.hr[e, :n]], 1)


def reference(w, st, e, table, kinematics="holonomic", n=None, nexts=None, rewards=None, float64=False):
    """The look-ahead of env e on the CPU.  Returns a dict: `values` [A] float64 = reward + gamma^(dt v_pref) V with V
    from the float32 network (pyref.sarl_forward on pyref.rotate of the float32 rows), `V` [A], `att` [A,n], `reward` [A]
    (pyref.lookahead_reward, or `rewards`) and, with float64=True, `V64`: the same network in float64 on the same float32
    features."""
    rows, nxt = joint_rows(st, e, table, kinematics, n, nexts)
    A, n_ = rows.shape[0], rows.shape[1]
    with torch.no_grad():
        feats = pyref.rotate(torch.from_numpy(rows.reshape(-1, 14)).float(), kinematics).view(A, n_, 13)
        V, att = pyref.sarl_forward(w, feats)
        out = {"V": V.double().numpy(), "att": att.numpy(), "feats": feats}
        if float64:
            out["V64"] = pyref.sarl_forward({k: v.double() for k, v in w.items()}, feats.double())[0].numpy()
    if rewards is None:
        rewards = [pyref.lookahead_reward(rows[a, 0, 0], rows[a, 0, 1], st.rr[e], st.rgx[e], st.rgy[e],
                                          [(h[0], h[1], h[4]) for h in nxt], DT) for a in range(A)]
    out["reward"] = np.array(rewards, np.float64)
    out["values"] = np.array([float(out["reward"][a]) + DISC * float(out["V"][a]) for a in range(A)])
    return out


def scores(w, feats):
    """The float32 attention scores [A,n] of pyref.sarl_forward's network on rotated features [A,n,13]."""
    A, n, _ = feats.shape
    with torch.no_grad():
        h = pyref._mlp(feats.reshape(A * n, -1), w, "mlp1", (0, 2), True)
        g = h.view(A, n, -1).mean(1, keepdim=True).expand(A, n, h.shape[1]).reshape(A * n, -1)
        return pyref._mlp(torch.cat([h, g], 1), w, "attention", (0, 2, 4), False).view(A, n)


def scan_argmax(values):
    """multi_human_rl.py:53-55: strict '>' from -inf, first maximum wins; -1 when no value wins (all NaN / -inf)."""
    best, idx = float("-inf"), -1
    for k, v in enumerate(values):
        if v > best:
            best, idx = float(v), k
    return idx, best


# ------------------------------------------------------------------------------------------------ argmax rows
ARGMAX_AS = (1, 2, 63, 64, 65, 81, 128, 129, 200)
SUB = 5e-324                            # the smallest float64 subnormal


def argmax_rows(A, seed=0):
    """Returns ([K,A] float64 value rows for sarl_argmax_kernel, names).  Lane l of its wavefront scans indices l, l + 64,
    ..., then lanes merge pairwise: ties sit in one lane's scan (k, k + 64), in neighbouring lanes, across the merge's
    halves (31 / 32) and at the two ends."""
    rng = np.random.RandomState(31 * A + seed)
    rows, names = [], []

    def base():
        return -1.0 - rng.uniform(0, 3, A)

    def add(name, v):
        rows.append(np.array(v, np.float64))
        names.append(name)

    def tie(name, idx, top=0.5, nan_at=()):
        if max(idx) < A and all(k < A for k in nan_at):
            v = base()
            v[list(idx)] = top
            v[list(nan_at)] = np.nan
            add(name, v)
    add("random", base())
    tie("tie-ends", (0, A - 1))
    tie("tie-stride-0", (0, 64))
    tie("tie-stride-last", (A - 65, A - 1) if A > 64 else (A,))
    tie("tie-stride-mid", (37, 101))
    tie("tie-stride-three", (5, 69, 133))
    for k in (0, 5, 15, 31, 32, 62, 63, 64, 127):
        tie("tie-neighbours-%d" % k, (k, k + 1))
    tie("tie-halves", (31, 32, 63))
    tie("tie-late-first", (A - 2, A - 1) if A > 1 else (A,))
    tie("all-equal", tuple(range(A)))
    tie("tie-minus-zero", (1, A - 1), top=-0.0)
    tie("inf", (A // 2,), top=np.inf)
    tie("inf-tie", (A // 3, A - 1), top=np.inf)
    tie("inf-tie-stride", (3, 67), top=np.inf)
    tie("nan-before", (A // 2, A - 1), nan_at=(0,))
    tie("nan-before-same-lane", (70, 100), nan_at=(6,))
    tie("nan-after", (0, A // 2), nan_at=(A - 1,))
    tie("nan-between", (1, A - 1), nan_at=tuple(range(2, A - 1)))
    tie("nan-between-stride", (2, 130), nan_at=(66,))
    tie("nan-neighbours", (33,), nan_at=(32, 34))
    add("all-nan", np.full(A, np.nan))
    add("all-minus-inf", np.full(A, -np.inf))
    v = np.full(A, -np.inf)
    v[A - 1] = -1e308
    add("minus-inf-but-last", v)
    v = np.full(A, np.nan)
    v[A // 2] = -np.inf
    add("nan-and-minus-inf", v)
    v = np.full(A, np.nan)
    v[A - 1] = -3.0
    add("nan-but-last", v)
    # subnormal gaps: neighbouring float64 values, positive and negative
    v = rng.randint(0, 3, A) * SUB
    add("subnormal-steps", v)
    add("subnormal-steps-negative", -v - SUB)
    v = np.full(A, 1.0)
    v[rng.randint(A)] = np.nextafter(1.0, 2.0)
    add("one-ulp-above", v)
    v = np.full(A, np.nextafter(1.0, 2.0))
    v[0 if A < 3 else 2] = 1.0
    add("one-ulp-below", v)
    return np.stack(rows), names


def feature_batch(N, table, kinematics="holonomic", seed=4):
    """lookahead_states.feature_batch (dg == 0, a human on the robot's next position, still humans) with, for a unicycle,
    its "random" envs turned into "heading-on-bearing": the goal straight ahead of the heading after the chosen action,
    so the theta feature nth - atan2(gdy, gdx) is exactly 0.  (The builder asserts that its constructions are exact in
    float64; with SARL's 81-row tables seed 4 satisfies it for N = 1 and N = 5.)"""
    from tests import lookahead_states as LS
    st, kinds, act = LS.feature_batch(N, table, kinematics, seed=seed, dt=DT)
    kinds = list(kinds)
    for e, kind in enumerate(kinds):
        far = np.hypot(st.rgx[e] - st.rpx[e], st.rgy[e] - st.rpy[e]) >= 0.5
        if kind == "random" and kinematics == "unicycle" and act[e]:
            v = float(np.asarray(table)[act[e], 0])
            st.rgx[e], st.rgy[e] = st.rpx[e] + v * DT + 2.0, st.rpy[e]           # nth == 0: straight along +x
            kinds[e] = "heading-on-bearing"
        elif kind != "on-goal" and not far:
            st.rgx[e], st.rgy[e] = st.rpx[e] + 1.5, st.rpy[e] - 0.75
    return st, kinds, act
