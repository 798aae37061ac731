"""Golden fixture for OM-SARL (`[sarl] with_om = true`), from the real reference (run in a container that has it):

    python -m tests.golden_tools.gen_golden_om

  g24_om_sarl  one seeded default-init OM-SARL state_dict (mlp1.0.weight [150, 61]);
               MultiHumanRL.build_occupancy_maps (multi_human_rl.py:109-163) for N = 2, 5, 10 on generic states and on
               constructed ones: two and three others in one cell (the mean), everyone outside the window (zero rows),
               a still human, stored velocities (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0) (arctan2 of signed zeros turns
               the frame by +-pi), an other exactly on top of the human;
               ValueNetwork forward on random [B, N, 61] inputs;
               SARL.predict (multi_human_rl.py:11-63): action_values and chosen action, holonomic and unicycle,
               N = 2, 5, 10, on gen_golden_policies' state generator;
               one train-phase run with epsilon 0.5 on numpy's global stream with last_state [N, 61].
Weights are saved as arrays (prefix w0__, '.' -> '__').
"""
import os

import numpy as np
import torch

from tests.golden_tools import gen_golden as G
from tests.golden_tools import gen_golden_policies as P

OUT = G.OUT
SEED = 0


def om_policy_config():
    cfg = G.policy_config()
    cfg.set("sarl", "with_om", "true")
    return cfg


def _policy(seed, kinematics="holonomic"):
    from crowd_nav.policy.policy_factory import policy_factory
    torch.manual_seed(seed)
    p = policy_factory["sarl"]()
    p.configure(om_policy_config())
    p.kinematics = kinematics
    p.set_device(torch.device("cpu"))
    p.set_phase("test")
    p.time_step = 0.25
    return p


def constructed_cases():
    """name -> [N,4] (px, py, vx, vy); human 0 is the one the case is about (every human gets a map all the same)."""
    nz = -0.0
    c = {}
    # human 0 heads along +x: its frame is the world's.  Others 1, 2 share cell (ix 3, iy 2), other 3 joins them below
    c["two_in_one_cell"] = [[0, 0, 1, 0], [1.25, 0.25, 0.5, 0.25], [1.75, 0.75, -0.25, 1.0], [-1.5, -1.5, 0.3, 0.4]]
    c["three_in_one_cell"] = [[0, 0, 1, 0], [1.25, 0.25, 0.5, 0.25], [1.75, 0.75, -0.25, 1.0], [1.5, 0.5, 0.125, -0.75],
                              [-0.5, 1.5, 1.0, 1.0]]
    c["all_outside"] = [[0, 0, 0.6, 0.8], [5.3, 5.1, 1, 0], [-6.3, 2.2, 0, 1], [2.5, -7, -1, -1]]
    c["still_human"] = [[0.5, -0.25, 0.0, 0.0], [1.0, 0.5, 0.5, 0.5], [-0.75, -1.0, -0.5, 0.25], [0.3125, 1.625, 0.0, 0.0]]
    c["neg_zero_vx"] = [[0.5, -0.25, nz, 0.0], [1.0, 0.5, 0.5, 0.5], [-0.75, -1.0, -0.5, 0.25], [0.3125, 1.625, nz, 0.0]]
    c["neg_zero_vy"] = [[0.5, -0.25, 0.0, nz], [1.0, 0.5, 0.5, 0.5], [-0.75, -1.0, -0.5, 0.25], [0.3125, 1.625, 0.0, nz]]
    c["neg_zero_both"] = [[0.5, -0.25, nz, nz], [1.0, 0.5, 0.5, 0.5], [-0.75, -1.0, -0.5, 0.25], [0.3125, 1.625, nz, nz]]
    c["on_top"] = [[0.375, -1.125, 0.6, -0.3], [0.375, -1.125, 0.2, 0.9], [1.0, -0.5, -0.4, 0.1]]
    c["on_top_still"] = [[0.375, -1.125, nz, 0.0], [0.375, -1.125, 0.0, 0.0]]
    return {k: np.array(v, np.float64) for k, v in c.items()}


def _maps(p, hum4):
    from crowd_sim.envs.utils.state import ObservableState
    return p.build_occupancy_maps([ObservableState(*row, 0.3) for row in hum4.tolist()]).numpy().copy()


def _om_maps(rec, rng, p):
    for N in (2, 5, 10):
        hums = []
        for s in range(16):
            pos = rng.uniform(-2.5, 2.5, (N, 2)) if s % 2 else rng.uniform(-1.2, 1.2, (N, 2))
            hums.append(np.concatenate([pos, rng.uniform(-1, 1, (N, 2))], 1))
        rec["om_in_N%d" % N] = np.array(hums)
        rec["om_out_N%d" % N] = np.array([_maps(p, h) for h in hums])
    from tests import om_ref
    for name, hum in constructed_cases().items():
        assert om_ref.edge_margin(hum) > 1e-6, name          # a constructed case must not sit on a cell edge
        rec["omc_in_" + name] = hum
        rec["omc_out_" + name] = _maps(p, hum)


def _forward(rec, rng, p):
    for N in (2, 5, 10):
        x = rng.uniform(-2, 2, (32, N, 61)).astype(np.float32)
        x[:, :, 0] = np.abs(x[:, :, 0]); x[:, :, 2] = 0
        x[:, :, :6] = x[:, :1, :6]
        x[:, :, 13:] = np.where(rng.uniform(size=(32, N, 48)) < 0.7, 0, x[:, :, 13:])      # maps are mostly empty
        with torch.no_grad():
            v = p.model(torch.from_numpy(x)).numpy()
        rec["vn_in_N%d" % N] = x
        rec["vn_out_N%d" % N] = v


def _predict(rec, rng):
    from crowd_sim.envs.utils.state import JointState
    for kin in ("holonomic", "unicycle"):
        for N in (2, 5, 10):
            p = _policy(SEED, kin)
            key = "pred_%s_N%d_" % (kin, N)
            selfs, hums, vals, acts = [], [], [], []
            for me, hs in P._states(rng, N, 32, kin):
                p.action_values = None
                with torch.no_grad():
                    act = p.predict(JointState(me, list(hs)))
                s_row, h_rows = P._rows(me, hs)
                selfs.append(s_row); hums.append(h_rows)
                reached = p.reach_destination(JointState(me, list(hs)))
                vals.append(np.full(len(p.action_space), np.nan) if reached else np.array(p.action_values))
                acts.append([act.vx, act.vy] if kin == "holonomic" else [act.v, act.r])
            rec[key + "self"] = np.array(selfs)
            rec[key + "humans"] = np.array(hums)
            rec[key + "values"] = np.array(vals)
            rec[key + "action"] = np.array(acts)


def _epsilon(rec, rng, N=5):
    from crowd_sim.envs.utils.state import FullState, ObservableState, JointState
    p = _policy(SEED)
    p.set_phase("train")
    p.set_epsilon(0.5)
    selfs, hums, acts, lasts, explored = [], [], [], [], []
    np.random.seed(2400 + SEED)
    for s_ in range(32):
        rpx, rpy = rng.uniform(-3, 3, 2)
        gx, gy = (rpx + 0.1, rpy - 0.1) if s_ % 12 == 11 else rng.uniform(-4, 4, 2)
        me = FullState(rpx, rpy, rng.uniform(-1, 1), rng.uniform(-1, 1), 0.3, gx, gy, 1.0, 0.0)
        hs = [ObservableState(*rng.uniform(-3, 3, 2), rng.uniform(-1, 1), rng.uniform(-1, 1), 0.3) for _ in range(N)]
        js = JointState(me, hs)
        p.action_values = None
        with torch.no_grad():
            act = p.predict(js)
        s_row, h_rows = P._rows(me, hs)
        selfs.append(s_row); hums.append(h_rows)
        acts.append([act.vx, act.vy])
        lasts.append(p.last_state.numpy().copy() if p.last_state is not None else np.zeros((N, 61), np.float32))
        explored.append(2 if p.reach_destination(js) else int(p.action_values is None))
    rec.update(eps_selfs=np.array(selfs), eps_humans=np.array(hums), eps_actions=np.array(acts),
               eps_last_states=np.array(lasts), eps_explored=np.array(explored), eps_seed=np.array(SEED))


def g24_om_sarl():
    rng = np.random.RandomState(24)
    rec = {}
    p = _policy(SEED)
    assert p.name == "OM-SARL" and p.input_dim() == 61
    rec.update(P._state_dict_arrays(p.model, "w%d__" % SEED))
    _om_maps(rec, rng, p)
    _forward(rec, rng, p)
    _predict(rec, rng)
    _epsilon(rec, rng)
    path = os.path.join(OUT, "g24_om_sarl.npz")
    np.savez_compressed(path, **rec)
    print("g24_om_sarl: %d arrays, %d bytes" % (len(rec), os.path.getsize(path)))


if __name__ == "__main__":
    g24_om_sarl()
