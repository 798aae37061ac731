"""LSTM-RL (reference: crowd_nav/policy/lstm_rl.py:9-103).

ValueNetwork1 keeps the reference's module tree, so `state_dict()` keys are mlp.{0,2,4,6} and
lstm.{weight,bias}_{ih,hh}_l0 and `rl_model.pth` files load unchanged.  Its torch forward exists for training with the
default `Trainer`; `Trainer(fused=True)` trains it without autograd through csrc/value_train.hip
(`mcn_lstm_rl_loss_grad`: the LSTM forward and back through time, then the MLP).  Every inference on the rollout path (`LstmRL.predict`, `LstmRL.predict_batch`) is one lstm_rl_value.hip launch on weights
re-packed into MFMA operand order.  The humans are taken in the order LstmRL.predict sorts them in (decreasing distance
to the robot, stable); the batched path sorts on the device (mcn_lstm_rl_order / the look-ahead kernel: one
definition), the E = 1 path on the host exactly as the reference does.
"""
import ctypes as C
import logging

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from .._pack import ident as _ident, natural as _natural, pack_layers
from .cadrl import _state_arrays, mlp
from .multi_human_rl import MultiHumanRL


class ValueNetwork1(nn.Module):
    def __init__(self, input_dim, self_state_dim, mlp_dims, lstm_hidden_dim):
        super().__init__()
        self.self_state_dim = self_state_dim
        self.lstm_hidden_dim = lstm_hidden_dim
        self.mlp = mlp(self_state_dim + lstm_hidden_dim, mlp_dims)
        self.lstm = nn.LSTM(input_dim, lstm_hidden_dim, batch_first=True)

    def forward(self, state):
        """lstm_rl.py:17-33.  h0 / c0 are built on the input's device (the reference builds them on the CPU, which
        fails for a model on the GPU); the values are the same zeros."""
        B = state.shape[0]
        self_state = state[:, 0, :self.self_state_dim]
        h0 = torch.zeros(1, B, self.lstm_hidden_dim, device=state.device, dtype=state.dtype)
        c0 = torch.zeros(1, B, self.lstm_hidden_dim, device=state.device, dtype=state.dtype)
        _, (hn, _) = self.lstm(state, (h0, c0))
        return self.mlp(torch.cat([self_state, hn.squeeze(0)], dim=1))


def _gate_omap(hidden=50, tiles=4):
    """Output slot map of the gate layer: unit u of gate G (PyTorch order i, f, g, o) in output tile 4G + t, slot s,
    where (t, s) holds unit u of h (_ident(hidden, tiles)), so the cell update is element-wise per register."""
    h = _ident(hidden, tiles)
    om = np.full(4 * tiles * 16, -1, np.int32)
    for G in range(4):
        for t in range(tiles):
            blk = h[t * 16:(t + 1) * 16]
            om[(G * tiles + t) * 16:(G * tiles + t + 1) * 16] = np.where(blk >= 0, G * hidden + blk, -1)
    return om


def shipped_shapes():
    """Shapes of the shipped LSTM-RL ValueNetwork1 (policy.config [lstm_rl]), in state_dict order: the weight shapes of
    the MLP's layers by state_dict key prefix, then the LSTM's tensors by state_dict key.  What lstm_rl_value.hip and
    value_train.hip are built for."""
    return ({"mlp.0": (150, 56), "mlp.2": (100, 150), "mlp.4": (100, 100), "mlp.6": (1, 100)},
            {"lstm.weight_ih_l0": (200, 13), "lstm.weight_hh_l0": (200, 50), "lstm.bias_ih_l0": (200,),
             "lstm.bias_hh_l0": (200,)})


def pack_lstm_rl_network(model, dev):
    """ValueNetwork1 -> (ctypes mcn_lstm_rl_net, [device tensors kept alive])."""
    sd = _state_arrays(model)
    layers, lstm = shipped_shapes()
    expect = dict({k: shp for k, shp in lstm.items() if len(shp) == 2}, **{k + ".weight": shp for k, shp in layers.items()})
    for k, shp in expect.items():
        if k not in sd or tuple(sd[k].shape) != shp:
            raise ValueError("lstm_rl_value.hip is built for the shipped LSTM-RL dimensions (policy.config [lstm_rl]: "
                             "global_state_dim = 50, mlp2_dims = 150, 100, 100, 1); %s is %s, expected %s"
                             % (k, sd[k].shape if k in sd else None, shp))
    gate_w = np.concatenate([sd["lstm.weight_ih_l0"], sd["lstm.weight_hh_l0"]], 1)          # [200, 13 + 50]
    gate_b = sd["lstm.bias_ih_l0"] + sd["lstm.bias_hh_l0"]
    gate_k = np.concatenate([_natural(13, 1), _ident(50, 4, offset=13)])
    m0_k = np.concatenate([_ident(6, 1), _ident(50, 4, offset=6)])                           # self tile, then h
    plan = [("gate", gate_w, gate_b, gate_k, _gate_omap()),
            ("m0", sd["mlp.0.weight"], sd["mlp.0.bias"], m0_k, _ident(150, 10)),
            ("m1", sd["mlp.2.weight"], sd["mlp.2.bias"], _ident(150, 10), _ident(100, 7)),
            ("m2", sd["mlp.4.weight"], sd["mlp.4.bias"], _ident(100, 7), _ident(100, 7)),
            ("m3", sd["mlp.6.weight"], sd["mlp.6.bias"], _ident(100, 7), _ident(1, 1))]
    return pack_layers(_hip.LstmRLNet(), plan, dev)


def sort_humans(state):
    """lstm_rl.py:99-103: human states by decreasing distance to the robot (sorted() is stable)."""
    def dist(human):
        return np.linalg.norm(np.array(human.position) - np.array(state.self_state.position))
    return sorted(state.human_states, key=dist, reverse=True)


class LstmRL(MultiHumanRL):
    def __init__(self):
        super().__init__()
        self.name = "LSTM-RL"
        self.with_interaction_module = None
        self.interaction_module_dims = None

    def configure(self, config):
        self.set_common_parameters(config)
        mlp_dims = [int(x) for x in config.get("lstm_rl", "mlp2_dims").split(", ")]
        global_state_dim = config.getint("lstm_rl", "global_state_dim")
        self.with_om = config.getboolean("lstm_rl", "with_om")
        self.with_interaction_module = config.getboolean("lstm_rl", "with_interaction_module")
        if self.with_om:
            raise NotImplementedError("occupancy maps (with_om = true) are outside this build's scope "
                                      "(shipped config: false)")
        if self.with_interaction_module:
            raise NotImplementedError("ValueNetwork2 (with_interaction_module = true) has no device look-ahead in this "
                                      "build (shipped config: false)")
        self.model = ValueNetwork1(self.input_dim(), self.self_state_dim, mlp_dims, global_state_dim)
        self.multiagent_training = config.getboolean("lstm_rl", "multiagent_training")
        logging.info("Policy: LSTM-RL w/o pairwise interaction module")

    def predict(self, state):
        """lstm_rl.py:90-103: sort the humans on the host (the caller's JointState is re-ordered, as in the
        reference), then MultiHumanRL.predict -- `last_state` is the transform of the sorted state."""
        state.human_states = sort_humans(state)
        return super().predict(state)

    def _pack(self, dev):
        return pack_lstm_rl_network(self.model, dev)

    def _launch(self, net, st, b, A, E, N, dev, kin, gamma_pow, npos, nvel, rew, epsilon, seed, want_attention):
        if b.get("order") is None:
            b["order"] = torch.empty(E, N, dtype=torch.int32, device=dev)
        rc = _hip.lib.mcn_lstm_rl_predict(C.byref(net), st, _hip.ptr(b["table"]), A, float(self.time_step), gamma_pow,
                                          kin, _hip.ptr(b["values"]), _hip.ptr(b["best"]), _hip.ptr(b["best_val"]),
                                          _hip.ptr(b["order"]), _hip.ptr(npos), _hip.ptr(nvel), _hip.ptr(rew),
                                          _hip.ptr(b["action"]), float(epsilon), seed, E, N, _hip.stream_ptr(dev))
        _hip.check(rc, "mcn_lstm_rl_predict")

    def human_order(self, env, hcount=None):
        """[E,N] int32 device tensor: the human index at each LSTM step of every env of a VecCrowdSim (mcn_lstm_rl_order;
        the order the look-ahead kernel uses without query_env).  hcount: as predict_batch (slots >= hcount[e] keep
        their index)."""
        E, N = env.num_envs, env._alloc_N
        order = torch.empty(E, N, dtype=torch.int32, device=env.device)
        _hip.check(_hip.lib.mcn_lstm_rl_order(_hip.with_hcount(env._st, hcount), _hip.ptr(order), E, N,
                                              _hip.stream_ptr(env.device)), "mcn_lstm_rl_order")
        return order

    def transform_batch(self, env):
        """`transform` of the sorted state for every env of a VecCrowdSim: [E,N,13] float32 rotated rows in the
        device order (what the reference stores as `last_state`, lstm_rl.py:103 + multi_human_rl.py:60-61)."""
        rows = super().transform_batch(env)
        order = self.human_order(env, getattr(env, "hcount", None)).long()
        return torch.gather(rows, 1, order.unsqueeze(2).expand(-1, -1, rows.shape[2]))

    @property
    def last_order(self):
        """[E,N] int32 device tensor: the human order of the latest look-ahead launch (identity with query_env)."""
        return self._bufs.get("order")
