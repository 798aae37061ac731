"""Host replay of scenario_pool_kernel (modelcrowdnav_amd/csrc/scenario_gen.hip, mcn_scenario_pool): plain Python
integers for the counter-based stream, numpy scalars for the placement arithmetic.  No GPU, no torch.

The rules are those of modelcrowdnav_amd/envs/scenarios.py (the bit-exact host generator, which has no cap on its
rejection loops), with the same operand order, np.cos / np.sin and `norm` of a pair, so that on cases where no loop
reaches the cap the replay and `scenarios.generate` driven by the same stream agree bit for bit
(tests/test_scenario_gen_cpu.py).  What the kernel adds is restated here:

  * stream: key = seed ^ (uint64(case id) * 0xD1B54A32D192ED03), draw c (from 1) = splitmix64's output function of
    key + c * 0x9E3779B97F4A7C15, top 53 bits * 2^-53;
  * every rejection loop ends after MAX_TRIES tries and keeps the values of the last one; the stream simply goes on;
    in a square crossing the start loop and the goal loop are capped independently;
  * the robot's start and goal are the configuration's, not necessarily (0, -r) / (0, r).

`margin` is the smallest |dist - gap| over every comparison the replay made.  The device's cos / sin and its
sqrt(fma(y, y, x * x)) differ from numpy's by a few ulps (~1e-15 at these magnitudes), so the device can decide a
comparison differently only where the margin is of that order; the tests require 1e-9.
"""
from collections import namedtuple

import numpy as np
from numpy.linalg import norm

MASK = (1 << 64) - 1
KEY_MUL = 0xD1B54A32D192ED03
GOLDEN = 0x9E3779B97F4A7C15
MAX_TRIES = 4096
CIRCLE, SQUARE = "circle_crossing", "square_crossing"

Cfg = namedtuple("Cfg", "rule randomize_attributes circle_radius square_width discomfort_dist human_radius "
                        "human_v_pref robot_radius robot_start robot_goal")


def cfg(rule, randomize=False, circle_radius=4.0, square_width=10.0, discomfort_dist=0.2, human_radius=0.3,
        human_v_pref=1.0, robot_radius=0.3, robot_start=None, robot_goal=None):
    """The shipped env.config values unless overridden; the robot starts at (0, -r) and heads for (0, r)."""
    return Cfg(rule, bool(randomize), circle_radius, square_width, discomfort_dist, human_radius, human_v_pref,
               robot_radius, tuple(robot_start) if robot_start is not None else (0.0, -circle_radius),
               tuple(robot_goal) if robot_goal is not None else (0.0, circle_radius))


def case_key(seed, case_id):
    """`case_id` wraps as a 64-bit integer (negative ids are legal), `seed` is a uint64."""
    return (seed & MASK) ^ (((case_id & MASK) * KEY_MUL) & MASK)


def splitmix64_out(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class Stream(object):
    """One case's draws.  Has numpy's random() / uniform() so that scenarios.generate can consume it."""

    def __init__(self, key):
        self.key, self.ctr = key & MASK, 0

    def raw(self):
        self.ctr += 1
        return splitmix64_out((self.key + self.ctr * GOLDEN) & MASK)

    def random(self):
        return (self.raw() >> 11) * (1.0 / 9007199254740992.0)

    def uniform(self, low, high):                     # numpy's formula: low + (high - low) * u
        return low + (high - low) * self.random()


Case = namedtuple("Case", "pos goal rad vpref capped draws margin max_tries")


def replay_case(c, seed, case_id, N):
    """One case of N humans.  pos, goal [N,2]; rad, vpref [N]; capped [N] bool (a loop of that human, start or goal,
    ran out of tries); draws: the stream's counter at the end; margin: see the module docstring; max_tries: the
    longest loop."""
    rng = Stream(case_key(seed, case_id))
    draw = rng.random
    dd, rr = c.discomfort_dist, c.robot_radius
    rsx, rsy = c.robot_start
    rgx, rgy = c.robot_goal
    R, w = c.circle_radius, c.square_width
    sx, sy, ex, ey, rad, vpref = [], [], [], [], [], []           # starts, goals (ends), radii, preferred speeds
    capped = np.zeros(N, bool)
    margin, max_tries = [np.inf], 0

    def hit(x, y, qx, qy, gap):
        d = norm((x - qx, y - qy))
        m = abs(d - gap)
        if m < margin[0]:
            margin[0] = m
        return d < gap

    for h in range(N):
        v_pref, radius = c.human_v_pref, c.human_radius
        if c.randomize_attributes:                    # v_pref first, then radius
            v_pref = 0.5 + draw()
            radius = 0.3 + 0.2 * draw()
        gaps = [radius + rad[q] + dd for q in range(h)]
        rgap = radius + rr + dd
        if c.rule == CIRCLE:
            for tr in range(1, MAX_TRIES + 1):
                angle = draw() * np.pi * 2
                nx = (draw() - 0.5) * v_pref
                ny = (draw() - 0.5) * v_pref
                px = R * np.cos(angle) + nx
                py = R * np.sin(angle) + ny
                collide = hit(px, py, rsx, rsy, rgap) or hit(px, py, rgx, rgy, rgap)
                q = 0
                while q < h and not collide:
                    collide = hit(px, py, sx[q], sy[q], gaps[q]) or hit(px, py, ex[q], ey[q], gaps[q])
                    q += 1
                if not collide:
                    break
            capped[h] = collide
            max_tries = max(max_tries, tr)
            gx, gy = -px, -py
        elif c.rule == SQUARE:
            sign = -1 if draw() > 0.5 else 1
            for tr in range(1, MAX_TRIES + 1):
                px = draw() * w * 0.5 * sign
                py = (draw() - 0.5) * w
                collide = hit(px, py, rsx, rsy, rgap)
                q = 0
                while q < h and not collide:
                    collide = hit(px, py, sx[q], sy[q], gaps[q])
                    q += 1
                if not collide:
                    break
            capped[h] = collide
            max_tries = max(max_tries, tr)
            for tr in range(1, MAX_TRIES + 1):
                gx = draw() * w * 0.5 * -sign
                gy = (draw() - 0.5) * w
                collide = hit(gx, gy, rgx, rgy, rgap)
                q = 0
                while q < h and not collide:
                    collide = hit(gx, gy, ex[q], ey[q], gaps[q])
                    q += 1
                if not collide:
                    break
            capped[h] |= collide
            max_tries = max(max_tries, tr)
        else:
            raise ValueError("rule %r" % (c.rule,))
        sx.append(px); sy.append(py); ex.append(gx); ey.append(gy); rad.append(radius); vpref.append(v_pref)
    return Case(np.stack([sx, sy], -1), np.stack([ex, ey], -1), np.array(rad, np.float64), np.array(vpref, np.float64),
                capped, rng.ctr, float(margin[0]), max_tries)


Batch = namedtuple("Batch", "pos goal rad vpref capped draws margin max_tries")


def replay(c, seed, first_case, P, N):
    """Cases first_case .. first_case + P - 1: the arrays of replay_case stacked ([P,N,2], [P,N], draws [P]); margin
    and max_tries over the whole batch."""
    cases = [replay_case(c, seed, first_case + i, N) for i in range(P)]
    st = lambda k: np.stack([getattr(x, k) for x in cases])
    return Batch(st("pos"), st("goal"), st("rad"), st("vpref"), st("capped"), np.array([x.draws for x in cases]),
                 min(x.margin for x in cases), max(x.max_tries for x in cases))


def host_generate(c, seed, case_id, N):
    """scenarios.generate (no cap) over the same stream; only for configurations with the default robot pose, which
    is the only one that generator knows.  Returns ([N,9] scenario, draws)."""
    from modelcrowdnav_amd.envs import scenarios as S
    assert c.robot_start == (0.0, -c.circle_radius) and c.robot_goal == (0.0, c.circle_radius)
    spec = S.ScenarioSpec(c.circle_radius, c.square_width, c.discomfort_dist, c.human_radius, c.human_v_pref,
                          c.robot_radius, c.randomize_attributes)
    rng = Stream(case_key(seed, case_id))
    return S.generate(spec, rng, N, c.rule), rng.ctr


def unplaced(pos, goal, rad, c):
    """Which humans sit inside a comfort gap of the robot or of an EARLIER human, under the checks of their rule:
    circle crossing -- the start against starts and goals (robot's included); square crossing -- the start against
    starts and the robot's start, the goal against goals and the robot's goal.  pos, goal [...,N,2]; rad [...,N];
    returns bool [...,N].  By construction these are the humans whose rejection loop ran out of tries."""
    pos, goal, rad = np.asarray(pos, np.float64), np.asarray(goal, np.float64), np.asarray(rad, np.float64)
    N = rad.shape[-1]
    dist = lambda a, b: np.sqrt(((a - b) ** 2).sum(-1))
    rs, rg = np.array(c.robot_start), np.array(c.robot_goal)
    rgap = rad + c.robot_radius + c.discomfort_dist
    earlier = np.tri(N, N, -1, dtype=bool)                                      # [h, q]: q < h
    gap = rad[..., :, None] + rad[..., None, :] + c.discomfort_dist
    ss = dist(pos[..., :, None, :], pos[..., None, :, :]) < gap
    if c.rule == CIRCLE:
        sg = dist(pos[..., :, None, :], goal[..., None, :, :]) < gap
        bad = ((ss | sg) & earlier).any(-1) | (dist(pos, rs) < rgap) | (dist(pos, rg) < rgap)
    else:
        gg = dist(goal[..., :, None, :], goal[..., None, :, :]) < gap
        bad = ((ss | gg) & earlier).any(-1) | (dist(pos, rs) < rgap) | (dist(goal, rg) < rgap)
    return bad


# ---------------------------------------------------------------------------------------------------------------
# The cases both test files use (test_scenario_gen_cpu.py: margin and cap coverage; test_scenario_gen_gpu.py: kernel
# against replay).  Small on purpose: the replay is pure Python, and a capped human costs 3 * 4096 draws.
#   N: 1, 5, 10, 32 (20 for its dense row)    P: 1, 63, 64, 65, 130 -- below, at and across a wavefront, two workgroups
#   and a tail    seed: 0, 7, 2^64 - 1    first_case: 0, 2^32 - 2003 (the last ids of the train phase's capacity,
#   uint32max - 2000), 2^32 - 3 (crosses 2^32 inside the batch), 2^40, -3 (crosses zero inside the batch)
# `dense` entries hold at least one human whose loop runs out of tries (found with the replay from id 100 on, seed 7);
# the others hold none.
Entry = namedtuple("Entry", "name cfg seed first_case P N dense")
_OFF_AXIS = dict(robot_start=(2.0, -3.0), robot_goal=(-1.5, 3.5))
TABLE = [
    Entry("circle-fixed-N5-P130", cfg(CIRCLE), 7, 100, 130, 5, False),
    Entry("circle-fixed-N1-P63", cfg(CIRCLE), 0, 0, 63, 1, False),
    Entry("square-rand-N5-P64-train-end", cfg(SQUARE, True), MASK, (1 << 32) - 2003, 64, 5, False),
    Entry("circle-fixed-N5-P5-across-2^32", cfg(CIRCLE), MASK, (1 << 32) - 3, 5, 5, False),
    Entry("square-fixed-N10-P65-2^40", cfg(SQUARE), 7, 1 << 40, 65, 10, False),
    Entry("circle-rand-N5-P65-across-zero-robot-off-axis", cfg(CIRCLE, True, **_OFF_AXIS), 0, -3, 65, 5, False),
    Entry("square-fixed-N5-P65-robot-off-axis", cfg(SQUARE, **_OFF_AXIS), 0, -3, 65, 5, False),
    Entry("square-rand-N32-P2", cfg(SQUARE, True), 7, 100, 2, 32, False),
    Entry("circle-rand-N10-P3-dense", cfg(CIRCLE, True), 7, 103, 3, 10, True),
    Entry("circle-fixed-N20-P2-dense", cfg(CIRCLE), 7, 102, 2, 20, True),
    Entry("circle-fixed-N32-P1-dense", cfg(CIRCLE), 7, 100, 1, 32, True),
    Entry("circle-rand-N32-P1-dense", cfg(CIRCLE, True), 7, 100, 1, 32, True),
    Entry("circle-radius0.5-N5-P2-dense", cfg(CIRCLE, circle_radius=0.5), 7, 100, 2, 5, True),
    Entry("square-width0.8-N3-P2-dense", cfg(SQUARE, square_width=0.8), 7, 100, 2, 3, True),
]

_replayed = {}


def replay_entry(e):
    """The replay of a table entry, computed once per process and shared (treat it as read-only)."""
    if e.name not in _replayed:
        _replayed[e.name] = replay(e.cfg, e.seed, e.first_case, e.P, e.N)
    return _replayed[e.name]
