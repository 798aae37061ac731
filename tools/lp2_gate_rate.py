#!/usr/bin/env python3
"""How often the quad ORCA solve's 2-D LP gate (csrc/quad_common.hpp: quad_orca_velocity) can fire on the benchmark
workload.  CPU only: the C oracle replays the workload of bench.py's headline -- 4096 envs x 5 humans, scenarios
pool[i % 500], robot actions drawn from the 81-entry table by torch.Generator(seed=0), a finished env restarting from
the pool's next case exactly as attach_rollout(case_stride=1, first_cases=(i + 1) % 500) makes the kernel do.

    python tools/lp2_gate_rate.py [--steps 600] [--envs 4096] [--humans 5]

Prints four rates:
  free human-steps    the solve returns exactly (bitwise) the clipped preferred velocity
  free group-steps    all humans of a 3-env group do (a group is what one ORCA wavefront of the rollout kernel holds:
                      the envs 3c, 3c + 1, 3c + 2): the steps on which the gate skips the 2-D LP
  3-D LP entries      per human-step, for scale
  restarts            per group-step and per env-step, and the mean episode length
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cport  # noqa: E402
from modelcrowdnav_amd.envs import scenarios as S  # noqa: E402


def clipped_pref(st):
    """The clipped preferred velocity of every human, operation by operation as the oracle's lp2 computes it (float32)."""
    with np.errstate(all="ignore"):
        px, py = (st.hgx - st.hpx).astype(np.float32), (st.hgy - st.hpy).astype(np.float32)
        ms = st.hvpref.astype(np.float32)
        pp = px * px + py * py
        inv = np.float32(1.0) / np.sqrt(pp)
        clip = pp > ms * ms
        return np.where(clip, ms * (px * inv), px), np.where(clip, ms * (py * inv), py)


def load_case(st, envs, pool, cases, spec):
    rr = spec.robot_row()
    sc = pool[cases]
    st.hpx[envs], st.hpy[envs], st.hgx[envs], st.hgy[envs] = sc[..., S.PX], sc[..., S.PY], sc[..., S.GX], sc[..., S.GY]
    st.hvx[envs], st.hvy[envs], st.hr[envs], st.hvpref[envs] = sc[..., S.VX], sc[..., S.VY], sc[..., S.RAD], sc[..., S.VPREF]
    st.rpx[envs], st.rpy[envs], st.rgx[envs], st.rgy[envs] = rr[S.PX], rr[S.PY], rr[S.GX], rr[S.GY]
    st.rvx[envs] = 0.0; st.rvy[envs] = 0.0; st.rr[envs] = rr[S.RAD]
    st.gtime[envs] = 0.0; st.human_times[envs] = 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--humans", type=int, default=5)
    a = ap.parse_args()
    E, N, T = a.envs, a.humans, a.steps
    from bench import make_actions                         # the benchmark's own draw (torch.Generator, seed 0)
    acts = make_actions(T, E, E, 0, "cpu").numpy()
    spec = S.ScenarioSpec()
    pool = S.scenario_pool(spec, "test", range(500), N, "circle_crossing")
    st = cport.EnvState(E, N)
    ids = np.arange(E) % 500
    load_case(st, np.arange(E), pool, ids, spec)
    next_case = (ids + 1) % 500
    cfg = cport.default_cfg()
    G = 64 // (4 * N)
    grp = np.arange(E) // G
    n_groups = int(grp[-1]) + 1

    # self-check of the vectorised clipped preferred velocity against the oracle's solve without neighbours
    vx, vy = clipped_pref(st)
    for e, i in [(e, i) for e in range(0, E, max(1, E // 64)) for i in range(N)]:
        ox, oy = cport.orca_agent((st.hpx[e, i], st.hpy[e, i]), (0, 0), 0.31, st.hvpref[e, i],
                                  (np.float32(st.hgx[e, i] - st.hpx[e, i]), np.float32(st.hgy[e, i] - st.hpy[e, i])),
                                  np.zeros((0, 2)), np.zeros((0, 2)), [])
        assert ox.tobytes() == vx[e, i].tobytes() and oy.tobytes() == vy[e, i].tobytes(), (e, i)

    free_h = free_g = restarts_e = restarts_g = 0
    cport.lp3_entries(reset=True)
    for t in range(T):
        vx, vy = clipped_pref(st)
        o = cport.env_step(cfg, st, np.ascontiguousarray(acts[t, :, 0]), np.ascontiguousarray(acts[t, :, 1]))
        ha = o["human_act"].astype(np.float32)
        free = (ha[..., 0].view(np.uint32) == vx.view(np.uint32)) & (ha[..., 1].view(np.uint32) == vy.view(np.uint32))
        free_h += int(free.sum())
        free_g += int((np.bincount(grp, weights=(~free).sum(1), minlength=n_groups) == 0).sum())
        d = o["done"].astype(bool)
        restarts_e += int(d.sum())
        restarts_g += int((np.bincount(grp, weights=d, minlength=n_groups) > 0).sum())
        if d.any():
            load_case(st, np.flatnonzero(d), pool, next_case[d], spec)
            next_case[d] = (next_case[d] + 1) % 500
    lp3 = cport.lp3_entries(reset=True)
    hs, gs, es = T * E * N, T * n_groups, T * E
    print("workload: %d envs x %d humans, scenarios pool[i %% 500], table actions from seed 0, %d steps; a finished env "
          "restarts from the pool's next case" % (E, N, T))
    print("groups: %d envs per ORCA wavefront, %d groups (the last holds %d)" % (G, n_groups, E - (n_groups - 1) * G))
    print("free human-steps   %6.2f %%   (%d of %d return exactly the clipped preferred velocity)" % (100.0 * free_h / hs, free_h, hs))
    print("free group-steps   %6.2f %%   (%d of %d: every human of the group does)" % (100.0 * free_g / gs, free_g, gs))
    print("3-D LP entries     %6.2f %%   of human-steps (%d)" % (100.0 * lp3 / hs, lp3))
    print("restarts           %6.2f %%   of group-steps, %.2f %% of env-steps, mean episode %.1f steps"
          % (100.0 * restarts_g / gs, 100.0 * restarts_e / es, es / max(restarts_e, 1)))


if __name__ == "__main__":
    main()
