"""Host replay of the mcn_env_rollout_orca contract (include/mcn.h): T closed-loop steps with an ORCA-driven robot.

Written from the header's comment and from the reference's crowd_sim/envs/policy/orca.py:82-132, not from the kernel.  Per
step and per env:

  1  the robot's action: oracle.cport.orca_agent (RVO2's solve, float32) for the robot as agent 0 with all N humans of its
     env as candidates in index order.  Every operand goes float64 -> float32 with numpy exactly where the header says:
     position, velocity, float32((rrad + 0.01) + safety_space), float32(rvpref), float32(rgoal - rpos), the humans'
     positions and velocities, float32((hrad + 0.01) + safety_space) -- the margin is two float64 additions in the
     reference's order (orca.py:100,103) -- with the robot policy's neighbor_dist / max_neighbors / time_horizon and
     float32(time_step); the float32 result is widened to float64;
  2  the env step: tests/rollout_ref.Replay.step (the oracle's env_step, the mcn_rollout bookkeeping, the pool restart),
     or the bare oracle step when there is no mcn_rollout.

The six traces are recorded as the header lays them out.  ORCA humans only: linear humans use device trigonometry that the
oracle matches to 1e-12, not bit for bit.

Event counters: the oracle's edge counters (cport.edge_counts) are reset before every robot solve and collected after
it, so `robot_events` holds what the ROBOT's solves met and `human_events` what the humans' solves inside the env step
met; `robot_lp3` counts the robot solves that fell through to the 3-D LP and `robot_lines[t, e]` is the number of
half-planes the robot's solve of step t filled (cport.orca_lines).
"""
import collections

import numpy as np

from oracle import cport

STEP_DTYPE = np.dtype([("reward", "f8"), ("dmin", "f8"), ("done", "u1"), ("info", "u1"), ("reserved", "u2"),
                       ("hh_count", "i4")])                                             # mcn_step_rec
TRACES = ("robot", "humans", "hrad", "action", "rec", "human_act")

RobotPolicy = collections.namedtuple("RobotPolicy", "safety_space neighbor_dist max_neighbors time_horizon")
RobotPolicy.__new__.__defaults__ = (0.0, 10.0, 10, 5.0)          # orca.py:59-62


def margin_radius(radius, safety_space):
    """float32((radius + 0.01) + safety_space): orca.py:100,103's `radius + 0.01 + self.safety_space` in Python floats,
    rounded once where rvo2 takes it as a C float."""
    return np.float32((np.float64(radius) + np.float64(0.01)) + np.float64(safety_space))


def robot_operands(st, e, rvpref, pol):
    """The float32 operands of env e's robot solve, converted where the header says."""
    f = np.float32
    s = pol.safety_space
    return dict(pos=(f(st.rpx[e]), f(st.rpy[e])), vel=(f(st.rvx[e]), f(st.rvy[e])),
                radius=margin_radius(st.rr[e], s), max_speed=f(rvpref[e]),
                pref=(f(st.rgx[e] - st.rpx[e]), f(st.rgy[e] - st.rpy[e])),
                opos=np.stack([st.hpx[e], st.hpy[e]], -1).astype(f), ovel=np.stack([st.hvx[e], st.hvy[e]], -1).astype(f),
                orad=np.array([margin_radius(r, s) for r in st.hr[e]], f))


def robot_action(st, e, rvpref, pol, time_step):
    """Step 1 of the contract for env e: (vx, vy) as float64 (the float32 result widened)."""
    o = robot_operands(st, e, rvpref, pol)
    vx, vy = cport.orca_agent(o["pos"], o["vel"], o["radius"], o["max_speed"], o["pref"], o["opos"], o["ovel"], o["orad"],
                              neighbor_dist=np.float32(pol.neighbor_dist), max_neighbors=int(pol.max_neighbors),
                              time_horizon=np.float32(pol.time_horizon), time_step=np.float32(time_step))
    return np.float64(vx), np.float64(vy)


def robot_lines(st, e, rvpref, pol, time_step):
    """How many half-planes env e's robot solve fills."""
    o = robot_operands(st, e, rvpref, pol)
    return len(cport.orca_lines(o["pos"], o["vel"], o["radius"], o["opos"], o["ovel"], o["orad"],
                                neighbor_dist=np.float32(pol.neighbor_dist), max_neighbors=int(pol.max_neighbors),
                                time_horizon=np.float32(pol.time_horizon), time_step=np.float32(time_step)))


class ClosedLoop(object):
    """The replay.  cfg: the oracle's config of the env step (the HUMANS' ORCA parameters live there); st: the oracle
    EnvState, advanced in place; rvpref [E]: the robot's max speed (no restart changes it); pol: RobotPolicy; roll: a
    tests/rollout_ref.Replay (mcn_rollout with a `state`) or None (roll == NULL, or a mcn_rollout without `state`: no
    accounting, no restart); has_rtheta False: st->rtheta == NULL, the theta column of tr_robot is +0.0."""

    def __init__(self, cfg, st, rvpref, pol, roll=None, has_rtheta=True, count=True):
        assert cfg.human_policy == cport.HUMANS_ORCA and not cfg.robot_unicycle
        self.cfg, self.st, self.pol, self.roll = cfg, st, pol, roll
        self.rvpref = np.asarray(rvpref, np.float64).copy()
        self.has_rtheta, self.count = has_rtheta, count
        self.robot_events, self.human_events = collections.Counter(), collections.Counter()
        self.robot_lp3 = 0
        self.nan_actions = 0
        self.lines = []
        self.tr = {k: [] for k in TRACES}

    def step(self):
        st, E, N, dt = self.st, self.st.E, self.st.N, self.cfg.time_step
        tr = self.tr
        theta = st.rtheta.copy() if self.has_rtheta else np.zeros(E)
        tr["robot"].append(np.stack([st.rpx, st.rpy, st.rvx, st.rvy, theta], -1))
        tr["humans"].append(np.stack([st.hpx, st.hpy, st.hvx, st.hvy], -1))
        tr["hrad"].append(st.hr.copy())
        act = np.zeros((E, 2))
        nl = np.zeros(E, np.int32)
        for e in range(E):
            if self.count:
                cport.edge_counts(reset=True); cport.lp3_entries(reset=True)
            act[e] = robot_action(st, e, self.rvpref, self.pol, dt)
            if self.count:
                self.robot_events.update(cport.edge_counts(reset=True))
                self.robot_lp3 += cport.lp3_entries(reset=True)
                nl[e] = robot_lines(st, e, self.rvpref, self.pol, dt)
        self.nan_actions += int(np.isnan(act).any(1).sum())
        if self.count:
            cport.edge_counts(reset=True)
        ax, ay = act[:, 0].copy(), act[:, 1].copy()
        out = self.roll.step(self.cfg, st, ax, ay) if self.roll is not None else cport.env_step(self.cfg, st, ax, ay)
        if self.count:
            self.human_events.update(cport.edge_counts(reset=True))
        rec = np.zeros(E, STEP_DTYPE)
        for k in ("reward", "dmin", "done", "info", "hh_count"):
            rec[k] = out[k]
        tr["action"].append(act); tr["rec"].append(rec); tr["human_act"].append(out["human_act"].copy())
        self.lines.append(nl)
        return out

    def run(self, T):
        for _ in range(T):
            self.step()
        return self

    def traces(self):
        """tr_robot [T,E,5], tr_humans [T,E,N,4], tr_hrad [T,E,N], tr_action [T,E,2], tr_rec [T,E] (STEP_DTYPE),
        tr_human_act [T,E,N,2]."""
        return {k: np.stack(v) for k, v in self.tr.items()}

    @property
    def robot_lines(self):
        return np.stack(self.lines)
