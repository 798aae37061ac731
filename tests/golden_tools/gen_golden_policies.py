"""Golden fixtures for the LSTM-RL and CADRL robot policies, from the real reference (run in a container that has it):

    python -m tests.golden_tools.gen_golden_policies [--only g22,g23]

  g22_lstm_rl  ValueNetwork1 forward (lstm_rl.py:9-33) with seeded default-init weights on random [B, N, 13] inputs
               (N = 1, 5, 10); LstmRL.predict (lstm_rl.py:90-103 -> multi_human_rl.py:11-63): action_values, chosen
               action, the sorted human list and last_state, holonomic and unicycle, N = 5 and 10, including states
               with exact distance ties (mirrored humans, duplicated humans, a human on the robot); one train-phase
               run with epsilon 0.5 (numpy's global stream decides exploration).
  g23_cadrl    CADRL ValueNetwork forward (cadrl.py:21-29) on random [B, N, 13] inputs; CADRL.predict (cadrl.py:131-178):
               action_values, chosen action, holonomic and unicycle, N = 1 and 5; one train-phase run with epsilon 0.5
               and N = 1 (transform asserts one human, cadrl.py:260) with last_state.
Weights are saved as arrays (prefix w<seed>__, '.' -> '__').
"""
import argparse
import os

import numpy as np
import torch

from tests.golden_tools import gen_golden as G

OUT = G.OUT


def _policy(name, seed, kinematics="holonomic"):
    from crowd_nav.policy.policy_factory import policy_factory
    torch.manual_seed(seed)
    p = policy_factory[name]()
    p.configure(G.policy_config())
    p.kinematics = kinematics
    p.set_device(torch.device("cpu"))
    p.set_phase("test")
    p.time_step = 0.25
    return p


def _state_dict_arrays(model, prefix):
    return {prefix + k.replace(".", "__"): v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _states(rng, N, count, kinematics):
    """(self rows [S, 9], human rows [S, N, 5]); every 4th state has exact distance ties: the robot sits on a
    quarter grid and humans are mirrored through it / duplicated / placed on it (all differences exact in float64)."""
    from crowd_sim.envs.utils.state import FullState, ObservableState
    out = []
    for s in range(count):
        tie = s % 4 == 3
        if tie:
            rpx, rpy = rng.randint(-8, 9, 2) * 0.25
        else:
            rpx, rpy = rng.uniform(-3, 3, 2)
        near_goal = s % 8 == 7
        gx, gy = (rpx + rng.uniform(-0.2, 0.2), rpy + rng.uniform(-0.2, 0.2)) if near_goal else rng.uniform(-4, 4, 2)
        theta = rng.uniform(-np.pi, np.pi) if kinematics == "unicycle" else np.pi / 2
        me = FullState(rpx, rpy, rng.uniform(-1, 1), rng.uniform(-1, 1), 0.3, gx, gy, 1.0, theta)
        hs = []
        for i in range(N):
            if tie and N > 1 and i % 3 == 1 and hs:             # mirror of the previous human through the robot
                p = hs[-1]
                hx, hy = 2 * rpx - p.px, 2 * rpy - p.py
            elif tie and i % 3 == 2 and hs:                       # duplicate of an earlier human
                p = hs[rng.randint(len(hs))]
                hx, hy = p.px, p.py
            elif tie and i == N - 1:                              # on the robot
                hx, hy = rpx, rpy
            elif tie:
                hx, hy = rpx + rng.randint(-12, 13) * 0.125, rpy + rng.randint(-12, 13) * 0.125
            elif s % 3 == 0 and i < 2:
                a, d = rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 1.3)
                hx, hy = rpx + d * np.cos(a), rpy + d * np.sin(a)
            else:
                hx, hy = rng.uniform(-4, 4, 2)
            hs.append(ObservableState(hx, hy, rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0.3, 0.5)))
        out.append((me, hs))
    return out


def _rows(me, hs):
    return ([me.px, me.py, me.vx, me.vy, me.radius, me.gx, me.gy, me.v_pref, me.theta],
            [[h.px, h.py, h.vx, h.vy, h.radius] for h in hs])


def _forward(rec, rng, p, seed):
    for N in (1, 5, 10):
        x = rng.uniform(-2, 2, (64, N, 13)).astype(np.float32)
        x[:, :, 0] = np.abs(x[:, :, 0]); x[:, :, 2] = 0
        x[:, :, :6] = x[:, :1, :6]                # self part identical across humans, as transform() builds it
        with torch.no_grad():
            if p.name == "CADRL":
                v = p.model(torch.from_numpy(x.reshape(-1, 13))).numpy().reshape(64, N)
            else:
                v = p.model(torch.from_numpy(x)).numpy()
        rec["vn%d_in_N%d" % (seed, N)] = x
        rec["vn%d_out_N%d" % (seed, N)] = v


def _predict(rec, rng, name, seed, Ns, phase="test"):
    from crowd_sim.envs.utils.state import JointState
    for kin in ("holonomic", "unicycle"):
        for N in Ns:
            p = _policy(name, seed, kin)
            key = "pred%d_%s_N%d_" % (seed, kin, N)
            selfs, hums, sorted_h, vals, acts, lasts = [], [], [], [], [], []
            for me, hs in _states(rng, N, 32, kin):
                js = JointState(me, list(hs))
                p.action_values = None
                with torch.no_grad():
                    act = p.predict(js)
                s_row, h_rows = _rows(me, hs)
                selfs.append(s_row); hums.append(h_rows); sorted_h.append(_rows(me, js.human_states)[1])
                reached = p.reach_destination(js)
                vals.append(np.full(len(p.action_space), np.nan) if reached else np.array(p.action_values))
                acts.append([act.vx, act.vy] if kin == "holonomic" else [act.v, act.r])
            rec[key + "self"] = np.array(selfs)
            rec[key + "humans"] = np.array(hums)
            rec[key + "sorted"] = np.array(sorted_h)
            rec[key + "values"] = np.array(vals)
            rec[key + "action"] = np.array(acts)
            rec[key + "table"] = np.array([[a.vx, a.vy] if kin == "holonomic" else [a.v, a.r] for a in p.action_space])


def _epsilon(rec, rng, name, seed, N):
    from crowd_sim.envs.utils.state import FullState, ObservableState, JointState
    p = _policy(name, seed)
    p.set_phase("train")
    p.set_epsilon(0.5)
    selfs, hums, acts, lasts, explored = [], [], [], [], []
    np.random.seed(2200 + seed)
    for s_ in range(48):
        rpx, rpy = rng.uniform(-3, 3, 2)
        gx, gy = (rpx + 0.1, rpy - 0.1) if s_ % 12 == 11 else rng.uniform(-4, 4, 2)
        me = FullState(rpx, rpy, rng.uniform(-1, 1), rng.uniform(-1, 1), 0.3, gx, gy, 1.0, 0.0)
        hs = [ObservableState(*rng.uniform(-4, 4, 2), rng.uniform(-1, 1), rng.uniform(-1, 1), 0.3) for _ in range(N)]
        js = JointState(me, hs)
        p.action_values = None
        with torch.no_grad():
            act = p.predict(js)
        s_row, h_rows = _rows(me, hs)
        selfs.append(s_row); hums.append(h_rows)
        acts.append([act.vx, act.vy])
        lasts.append(p.last_state.numpy().copy())
        # 0: greedy (the look-ahead ran), 1: a random table row, 2: the robot stands on its goal (no draw at all)
        explored.append(2 if p.reach_destination(js) else int(p.action_values is None))
    rec.update(eps_selfs=np.array(selfs), eps_humans=np.array(hums), eps_actions=np.array(acts),
               eps_last_states=np.array(lasts), eps_explored=np.array(explored), eps_seed=np.array(seed))


def g22_lstm_rl():
    rng = np.random.RandomState(22)
    rec = {}
    for seed in (0, 1):
        p = _policy("lstm_rl", seed)
        rec.update(_state_dict_arrays(p.model, "w%d__" % seed))
        _forward(rec, rng, p, seed)
        _predict(rec, rng, "lstm_rl", seed, (5, 10))
    _epsilon(rec, rng, "lstm_rl", 0, 5)
    np.savez_compressed(os.path.join(OUT, "g22_lstm_rl.npz"), **rec)
    print("g22_lstm_rl: %d arrays" % len(rec))


def g23_cadrl():
    rng = np.random.RandomState(23)
    rec = {}
    for seed in (0, 1):
        p = _policy("cadrl", seed)
        rec.update(_state_dict_arrays(p.model, "w%d__" % seed))
        _forward(rec, rng, p, seed)
        _predict(rec, rng, "cadrl", seed, (1, 5))
    _epsilon(rec, rng, "cadrl", 0, 1)
    np.savez_compressed(os.path.join(OUT, "g23_cadrl.npz"), **rec)
    print("g23_cadrl: %d arrays" % len(rec))


FAMILIES = {"g22": g22_lstm_rl, "g23": g23_cadrl}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    for w in [w for w in args.only.split(",") if w] or list(FAMILIES):
        FAMILIES[w]()


if __name__ == "__main__":
    main()
