"""One-step look-ahead over the action table for pairwise-state value networks
(reference: crowd_nav/policy/multi_human_rl.py:7-104).

`predict(JointState)` keeps the reference's contract -- including the draw from numpy's global
stream before the epsilon test, the reach-destination short cut, `action_values`, `last_state`
and the ValueError on an all-NaN network -- but the 81-iteration Python loop (propagate,
compute_reward, 5 tiny tensors, rotate, forward, .item()) is ONE look-ahead launch (the policy's `_launch` hook:
mcn_sarl_predict, mcn_lstm_rl_predict).  `predict_batch(env)` (policy/cadrl.py) is the same launch over all E
environments of a VecCrowdSim, reading the env's HBM-resident state in place.
"""
import numpy as np
import torch

from .. import _hip
from .cadrl import CADRL


OM_CELL_NUM, OM_CHANNELS = 4, 3           # the [om] geometry sarl_om.hip is built for (policy.config); any cell_size
OM_WIDTH = OM_CELL_NUM ** 2 * OM_CHANNELS


class MultiHumanRL(CADRL):
    """The [N,13]-rows policies (SARL, LSTM-RL).  The look-ahead plumbing (_lookahead, _query_env, predict_batch) is
    CADRL's; a subclass supplies `_pack` and the launch hook `_launch`."""

    _attention = False          # the network has per-human attention weights (SARL)

    def _pack(self, dev):
        raise NotImplementedError

    def _launch(self, net, st, b, A, E, N, dev, kin, gamma_pow, npos, nvel, rew, epsilon, seed, want_attention):
        raise NotImplementedError

    # ------------------------------------------------------------------ reference surface (E = 1)
    def _greedy_action(self, state):
        """multi_human_rl.py:31-57 as one look-ahead launch (`predict` itself is CADRL's): `action_values`, the
        attention weights, and the ValueError on an all-NaN network."""
        if self.with_om:
            self._om_needs_others(len(state.human_states))
        st, _stage, N, dev = self._stage_joint_state(state)
        values, best, _, att = self._lookahead(st, 1, N, dev, want_attention=self._attention,
                                               env_next=self._env_next_of_host_env())
        vals = values[0].cpu().numpy()
        self.action_values = vals.tolist()
        idx = int(best.item())
        if self._attention:
            # the reference's model keeps the weights of its LAST forward, i.e. of the last candidate action
            # (sarl.py:56,88-89), and that is what env.step stores per step; the chosen action's are kept beside them
            a_host = att[0].cpu().numpy()
            self._last_attention = a_host[-1].copy()
            self.chosen_attention_weights = a_host[max(idx, 0)].copy()
        if idx < 0 or not np.isfinite(vals[idx]):
            # every value NaN <=> `value > max_value` never fired in the reference loop
            raise ValueError("Value network is not well trained. ")
        return self.action_space[idx]

    def transform(self, state):
        """multi_human_rl.py:90-104: [N,13] rotated rows (float32) for the replay memory."""
        rows = torch.cat([torch.Tensor([state.self_state + h]).to(self.device) for h in state.human_states], dim=0)
        if self.with_om:
            om = self.build_occupancy_maps(state.human_states)            # of the CURRENT states (:99-101)
            return torch.cat([self.rotate(rows), om.to(self.device)], dim=1)
        return self.rotate(rows)

    def transform_batch(self, env):
        """`transform` for every env of a VecCrowdSim: [E,N,13] float32 rotated joint states (what the reference
        stores as `last_state` in train phase, multi_human_rl.py:60-61)."""
        E, N = env.num_envs, env._alloc_N
        f = torch.float32
        rob = torch.cat([env.rpos, env.rvel, env.rrad.unsqueeze(1), env.rgoal, env.rvpref.unsqueeze(1),
                         env.rtheta.unsqueeze(1)], 1).to(f)                                  # [E,9]
        hum = torch.cat([env.hpos, env.hvel, env.hrad.unsqueeze(2)], 2).to(f)                 # [E,N,5]
        rows = torch.cat([rob.unsqueeze(1).expand(E, N, 9), hum], 2).reshape(E * N, 14)
        rows = self.rotate(rows).view(E, N, 13)
        if self.with_om:
            # maps of the current states; env.hcount, when the env keeps one, masks as in the look-ahead
            st = _hip.with_hcount(env._st, getattr(env, "hcount", None))
            om = torch.empty(E, N, OM_WIDTH, dtype=f, device=env.device)
            self._om_prepare(st, 0.0, None, None, om, E, N, env.device)
            rows = torch.cat([rows, om.to(rows.device)], 2)
        return rows

    def input_dim(self):
        return self.joint_state_dim + (self.cell_num ** 2 * self.om_channel_size if self.with_om else 0)

    # ------------------------------------------------------------------ occupancy maps (with_om)
    @staticmethod
    def _om_needs_others(n):
        if n < 2:
            # the reference's np.concatenate of an empty list of other humans (multi_human_rl.py:117-118)
            raise ValueError("need at least one array to concatenate (an occupancy map needs another human)")

    def _om_geometry_check(self):
        if (self.cell_num, self.om_channel_size) != (OM_CELL_NUM, OM_CHANNELS) or not self.cell_size > 0:
            raise ValueError("sarl_om.hip is built for the shipped occupancy-map geometry (policy.config [om]: cell_num = "
                             "%d, om_channel_size = %d, a positive cell_size); got cell_num = %r, om_channel_size = %r, "
                             "cell_size = %r" % (OM_CELL_NUM, OM_CHANNELS, self.cell_num, self.om_channel_size,
                                                 self.cell_size))

    def _om_prepare(self, st, dt, npos, nvel, om, E, N, dev, net=None, init=None):
        """mcn_sarl_om_prepare: the maps of st's humans (after dt of constant velocity, or the given next states) into
        `om` [E,N,48] and, with the packed net, their share of mlp1.0 into `init` [E,N,160]."""
        self._om_geometry_check()
        rc = _hip.lib.mcn_sarl_om_prepare(st, float(dt), _hip.ptr(npos), _hip.ptr(nvel), float(self.cell_size),
                                          _hip.ptr(net.om_w) if net is not None else None,
                                          _hip.ptr(net.om_b) if net is not None else None, _hip.ptr(om),
                                          _hip.ptr(init), E, N, _hip.stream_ptr(dev))
        _hip.check(rc, "mcn_sarl_om_prepare")

    def build_occupancy_maps(self, human_states):
        """multi_human_rl.py:109-163: [N, cell_num^2 * om_channel_size] float32 (CPU tensor, as the reference's), one
        E = 1 mcn_sarl_om_prepare launch -- the maps have one definition, on the device."""
        N = len(human_states)
        self._om_needs_others(N)
        dev = self._gpu_device()
        stage = torch.tensor([c for h in human_states for c in (h.px, h.py)] +
                             [c for h in human_states for c in (h.vx, h.vy)], dtype=torch.float64).to(dev)
        st = _hip.EnvState()
        st.hpos, st.hvel = _hip.ptr(stage[:2 * N]), _hip.ptr(stage[2 * N:])
        om = torch.empty(1, N, OM_WIDTH, dtype=torch.float32, device=dev)
        self._om_prepare(st, 0.0, None, None, om, 1, N, dev)
        return om[0].cpu()
