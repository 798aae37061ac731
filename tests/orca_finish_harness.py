"""What the GPU tests of mcn_orca_finish share: a host state (tests/orca_finish_ref.py layout) on the device with the
call itself, and the byte-for-byte comparison with a replay."""
import numpy as np

from tests import helpers as H
from tests import orca_finish_ref as R

HELD = -7.0          # what traj holds before a call: rows a call does not simulate must keep it
WRITTEN = ("hpos", "rpos", "gtime", "human_times")


class Batch(object):
    """A host state (orca_finish_ref layout) on the device, with velocity / heading fields the entry point must leave
    alone, and the call itself."""

    def __init__(self, st, vel, max_steps):
        import torch
        from modelcrowdnav_amd import _hip
        self.dev = torch.device("cuda", 0)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.E, self.N = st["hrad"].shape
        self.t = {k: up(st[k]) for k in R.STATE_KEYS}
        rng = np.random.RandomState(1)
        self.t["hvel"], self.t["rvel"] = up(rng.uniform(-1, 1, (self.E, self.N, 2))), up(rng.uniform(-1, 1, (self.E, 2)))
        self.t["rtheta"] = up(rng.uniform(-3, 3, self.E))
        self.before = {k: v.cpu().numpy().copy() for k, v in self.t.items()}
        self.sim_vel = up(vel)
        self.steps = torch.full((self.E,), -1, dtype=torch.int32, device=self.dev)
        self.traj = torch.full((max_steps, self.E, self.N + 1, 2), HELD, dtype=torch.float32, device=self.dev)
        self.st = _hip.EnvState(*[_hip.ptr(self.t[k]) for k in ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel",
                                                                "rgoal", "rrad", "rvpref", "rtheta", "gtime",
                                                                "human_times")])

    def run(self, max_steps, select=None, traj=True, time_step=0.25, neighbor_dist=10.0, max_neighbors=10,
            time_horizon=5.0):
        import torch
        from modelcrowdnav_amd import _hip
        assert max_steps <= self.traj.shape[0]
        sel = None if select is None else torch.from_numpy(np.asarray(select, np.uint8)).to(self.dev)
        self.traj.fill_(HELD)
        rc = _hip.lib.mcn_orca_finish(self.st, _hip.ptr(self.sim_vel), _hip.ptr(sel), max_steps, _hip.ptr(self.steps),
                                      _hip.ptr(self.traj) if traj else None, time_step, neighbor_dist, max_neighbors,
                                      time_horizon, self.E, self.N, _hip.stream_ptr(self.dev))
        assert rc == _hip.MCN_OK
        torch.cuda.synchronize()
        out = {k: self.t[k].cpu().numpy() for k in self.t}
        out.update(sim_vel=self.sim_vel.cpu().numpy(), steps=self.steps.cpu().numpy(), traj=self.traj.cpu().numpy())
        return out

    def untouched(self, out):
        for k in self.before:
            if k not in WRITTEN:
                H.assert_bits_equal(out[k], self.before[k], "input " + k)


def assert_matches(out, ref, what=""):
    for k in WRITTEN + ("sim_vel",):
        H.assert_bits_equal(out[k], ref[k], "%s %s" % (what, k))
    assert out["steps"].tolist() == ref["steps"].tolist(), what
    for e, rows in enumerate(ref["traj"]):
        H.assert_bits_equal(out["traj"][:len(rows), e], rows, "%s traj of env %d" % (what, e))
        assert np.all(out["traj"][len(rows):, e] == HELD), (what, e)


def tiled(ref, idx):
    """The replay of a few distinct scenes laid out as the batch idx[e] -> scene."""
    out = {k: ref[k][idx] for k in WRITTEN + ("sim_vel", "steps")}
    out["traj"] = [ref["traj"][i] for i in idx]
    return out
