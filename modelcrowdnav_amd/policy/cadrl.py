"""Shared pieces of the value-based robot policies (reference: crowd_nav/policy/cadrl.py).

  mlp()                 cadrl.py:11-19   nn.Sequential of Linear/ReLU with the reference's key names
  build_action_space()  cadrl.py:82-102  the 1 + rotations x speeds action table (host, once)

The per-step arithmetic that the reference does in Python for each of the 81 candidate
actions (propagate :104-129, rotate :217-252, compute_reward multi_human_rl.py:65-88) runs on
the GPU in one look-ahead launch per step: sarl_value.hip (policy/sarl.py), lstm_rl_value.hip
(policy/lstm_rl.py and CADRL's own single-human network below).  The launch plumbing shared by
all of them (`_lookahead`, `_query_env`, `predict_batch`) lives in CADRL; each policy supplies
`_pack` (weights -> MFMA fragments) and the `_launch` hook.  Training: the default `Trainer` runs CADRL's own
ValueNetwork through torch autograd, `Trainer(fused=True)` through csrc/value_train.hip (`mcn_cadrl_loss_grad`).
"""
import ctypes as C
import itertools
import logging
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .. import _hip
from .._pack import ident as _ident, natural as _natural, pack_layers
from ..envs.policy.policy import Policy
from ..envs.utils.action import ActionRot, ActionXY
from ..envs.utils.state import FullState, ObservableState


def mlp(input_dim, mlp_dims, last_relu=False):
    dims = [input_dim] + list(mlp_dims)
    layers = []
    last = len(dims) - 2
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(nn.Linear(a, b))
        if i != last or last_relu:
            layers.append(nn.ReLU())
    return nn.Sequential(*layers)


def build_action_space(v_pref, kinematics="holonomic", speed_samples=5, rotation_samples=16):
    """Returns (table [1 + R*S, 2] float64, speeds list, rotations ndarray).

    Row 0 is the zero action; then rotations-major, speeds-minor (itertools.product order).
    Holonomic rows are (vx, vy); unicycle rows are (v, r).
    """
    holonomic = kinematics == "holonomic"
    speeds = [(np.exp((i + 1) / speed_samples) - 1) / (np.e - 1) * v_pref for i in range(speed_samples)]
    if holonomic:
        rotations = np.linspace(0, 2 * np.pi, rotation_samples, endpoint=False)
    else:
        rotations = np.linspace(-np.pi / 4, np.pi / 4, rotation_samples)
    rows = [(0.0, 0.0)]
    for rot, spd in itertools.product(rotations, speeds):
        rows.append((spd * np.cos(rot), spd * np.sin(rot)) if holonomic else (spd, rot))
    return np.array(rows, dtype=np.float64), speeds, rotations


def rotate(state, kinematics):
    """cadrl.py:217-252: [B,14] joint rows -> [B,13] agent-centric rows (torch, any device).

    Host-side use only (Explorer memory / `transform`); the look-ahead builds the same features inside
    sarl_value.hip.  Column order in : px py vx vy r gx gy v_pref theta | px1 py1 vx1 vy1 r1
    Column order out: dg v_pref theta r vx vy px1 py1 vx1 vy1 r1 da r+r1
    """
    px, py, vx, vy, r, gx, gy, vpref, theta, hx, hy, hvx, hvy, hr = state.unbind(1)
    dx, dy = gx - px, gy - py
    heading = torch.atan2(dy, dx)
    c, s = torch.cos(heading), torch.sin(heading)
    dg = torch.sqrt(dx * dx + dy * dy)
    th = theta - heading if kinematics == "unicycle" else torch.zeros_like(vpref)
    ox, oy = hx - px, hy - py
    da = torch.sqrt(ox * ox + oy * oy)
    return torch.stack([dg, vpref, th, r, vx * c + vy * s, vy * c - vx * s, ox * c + oy * s, oy * c - ox * s,
                        hvx * c + hvy * s, hvy * c - hvx * s, hr, da, r + hr], 1)


class ValueNetwork(nn.Module):
    """cadrl.py:21-29: state_dict keys value_network.{0,2,4,6}.weight/.bias."""

    def __init__(self, input_dim, mlp_dims):
        super().__init__()
        self.value_network = mlp(input_dim, mlp_dims)

    def forward(self, state):
        return self.value_network(state)


def _state_arrays(model):
    return {k: v.detach().to("cpu", torch.float32).contiguous().numpy() for k, v in model.state_dict().items()}


def shipped_shapes():
    """Weight shapes of the shipped CADRL ValueNetwork (policy.config [cadrl]) by state_dict key prefix, in state_dict
    order: what lstm_rl_value.hip and value_train.hip are built for."""
    return {"value_network.0": (150, 13), "value_network.2": (100, 150), "value_network.4": (100, 100),
            "value_network.6": (1, 100)}


def pack_cadrl_network(model, dev):
    """CADRL ValueNetwork -> (ctypes mcn_cadrl_net, [device tensors kept alive])."""
    sd = _state_arrays(model)
    for k, shp in shipped_shapes().items():
        if k + ".weight" not in sd or tuple(sd[k + ".weight"].shape) != shp:
            raise ValueError("lstm_rl_value.hip is built for the shipped CADRL dimensions (policy.config [cadrl] "
                             "mlp_dims = 150, 100, 100, 1); %s.weight is %s" % (k, sd.get(k + ".weight", np.zeros(0)).shape))
    plan = [("l0", "value_network.0", _natural(13, 1), _ident(150, 10)),
            ("l1", "value_network.2", _ident(150, 10), _ident(100, 7)),
            ("l2", "value_network.4", _ident(100, 7), _ident(100, 7)),
            ("l3", "value_network.6", _ident(100, 7), _ident(1, 1))]
    return pack_layers(_hip.CadrlNet(), [(name, sd[key + ".weight"], sd[key + ".bias"], kmap, omap)
                                         for name, key, kmap, omap in plan], dev)


class CADRL(Policy):
    """CADRL (cadrl.py:31-252), and the configuration / action-space / propagate / look-ahead surface shared by the
    value-based policies (SARL, LSTM-RL inherit it through MultiHumanRL)."""

    def __init__(self):
        super().__init__()
        self.name = "CADRL"
        self.trainable = True
        self.multiagent_training = None
        self.kinematics = None
        self.epsilon = None
        self.gamma = None
        self.sampling = None
        self.speed_samples = None
        self.rotation_samples = None
        self.query_env = None
        self.action_space = None
        self.speeds = None
        self.rotations = None
        self.action_values = None
        self.with_om = None
        self.cell_num = None
        self.cell_size = None
        self.om_channel_size = None
        self.self_state_dim = 6
        self.human_state_dim = 7
        self.joint_state_dim = self.self_state_dim + self.human_state_dim
        self._action_table = None
        self._table_dev = None    # (host table, device, its device copy): _table()
        self._frags = None       # packed MFMA operand fragments (device) + the weight stamp they were packed at
        self._ws = None
        self._bufs = {}

    def set_common_parameters(self, config):
        self.gamma = config.getfloat("rl", "gamma")
        self.sampling = config.get("action_space", "sampling")
        self.speed_samples = config.getint("action_space", "speed_samples")
        self.rotation_samples = config.getint("action_space", "rotation_samples")
        self.query_env = config.getboolean("action_space", "query_env")
        self.cell_num = config.getint("om", "cell_num")
        self.cell_size = config.getfloat("om", "cell_size")
        self.om_channel_size = config.getint("om", "om_channel_size")

    def configure(self, config):
        self.set_common_parameters(config)
        mlp_dims = [int(x) for x in config.get("cadrl", "mlp_dims").split(", ")]
        self.model = ValueNetwork(self.joint_state_dim, mlp_dims)
        self.multiagent_training = config.getboolean("cadrl", "multiagent_training")
        logging.info("Policy: CADRL without occupancy map")

    def set_device(self, device):
        self.device = device
        self.model.to(device)

    def set_epsilon(self, epsilon):
        self.epsilon = epsilon

    def build_action_space(self, v_pref):
        table, speeds, rotations = build_action_space(v_pref, self.kinematics, self.speed_samples, self.rotation_samples)
        make = ActionXY if self.kinematics == "holonomic" else ActionRot
        self.speeds, self.rotations = speeds, rotations
        self.action_space = [make(*row) for row in table.tolist()]
        self.action_space[0] = make(0, 0)
        self._action_table = table

    def propagate(self, state, action):
        """cadrl.py:104-129 (host value types; the batched look-ahead does this in sarl_value.hip)."""
        dt = self.time_step
        if isinstance(state, ObservableState):
            return ObservableState(state.px + action.vx * dt, state.py + action.vy * dt, action.vx, action.vy,
                                   state.radius)
        if not isinstance(state, FullState):
            raise ValueError("Type error")
        if self.kinematics == "holonomic":
            return FullState(state.px + action.vx * dt, state.py + action.vy * dt, action.vx, action.vy, state.radius,
                             state.gx, state.gy, state.v_pref, state.theta)
        import numpy as np
        th = state.theta + action.r
        nvx, nvy = action.v * np.cos(th), action.v * np.sin(th)
        return FullState(state.px + nvx * dt, state.py + nvy * dt, nvx, nvy, state.radius, state.gx, state.gy,
                         state.v_pref, th)

    def rotate(self, state):
        return rotate(state, self.kinematics)

    def transform(self, state):
        assert len(state.human_states) == 1
        row = torch.Tensor(state.self_state + state.human_states[0]).to(self.device)
        return self.rotate(row.unsqueeze(0)).squeeze(dim=0)

    def transform_batch(self, env):
        """`transform` for every env of a VecCrowdSim: [E,13] float32 rotated rows.  Like `transform` (its one-human
        assertion, cadrl.py:260) it refuses envs with more than one human instead of storing what the reference cannot."""
        if env._alloc_N != 1:
            raise AssertionError("CADRL.transform_batch: the reference's transform takes one human (N = %d)" % env._alloc_N)
        f = torch.float32
        rows = torch.cat([env.rpos, env.rvel, env.rrad.unsqueeze(1), env.rgoal, env.rvpref.unsqueeze(1),
                          env.rtheta.unsqueeze(1), env.hpos[:, 0], env.hvel[:, 0], env.hrad[:, :1]], 1).to(f)
        return self.rotate(rows)

    # ------------------------------------------------------------------ reference surface (E = 1)
    def predict(self, state):
        """cadrl.py:131-178 = multi_human_rl.py:14-63 around the look-ahead, in the reference's order: attribute
        checks, the reach-destination short cut, the action space, ONE draw from numpy's global stream (unconditional),
        the epsilon test or `_greedy_action` (one look-ahead launch), then `last_state` in phase 'train'."""
        if self.phase is None or self.device is None:
            raise AttributeError("Phase, device attributes have to be set!")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError("Epsilon attribute has to be set in training phase")
        if self.reach_destination(state):
            return ActionXY(0, 0) if self.kinematics == "holonomic" else ActionRot(0, 0)
        if self.action_space is None:
            self.build_action_space(state.self_state.v_pref)
        probability = np.random.random()
        if self.phase == "train" and probability < self.epsilon:
            max_action = self.action_space[np.random.choice(len(self.action_space))]
        else:
            max_action = self._greedy_action(state)
        if self.phase == "train":
            self.last_state = self.transform(state)
        return max_action

    def _greedy_action(self, state):
        """The minimum over the humans of the value network, maximised over the action table; one mcn_cadrl_predict
        launch.  None when every value is NaN (the reference's `max_action = None`)."""
        st, _stage, N, dev = self._stage_joint_state(state)
        values, _, _, _ = self._lookahead(st, 1, N, dev, env_next=self._env_next_of_host_env())
        self.action_values = values[0].cpu().numpy().tolist()
        idx = -1
        for i, v in enumerate(self.action_values):            # strict '>' from -inf: NaN never wins
            if v > (self.action_values[idx] if idx >= 0 else float("-inf")):
                idx = i
        return self.action_space[idx] if idx >= 0 else None

    def _stage_joint_state(self, state):
        """A host JointState as the E = 1 env state of a look-ahead: (EnvState, the staged device tensor its pointers
        point into -- keep it until the launch is issued --, N, device).  One host row, one host-to-device copy; the
        state arrays are views of it (16-byte aligned: pairs first)."""
        me, humans = state.self_state, state.human_states
        dev, N = self._gpu_device(), len(humans)
        row = [c for h in humans for c in (h.px, h.py)] + [c for h in humans for c in (h.vx, h.vy)] + \
              [me.px, me.py, me.vx, me.vy, me.gx, me.gy] + [h.radius for h in humans] + [me.radius, me.v_pref, me.theta]
        stage = torch.tensor(row, dtype=torch.float64).to(dev)
        names = ("hpos", "hvel", "rpos", "rvel", "rgoal", "hrad", "rrad", "rvpref", "rtheta")
        sizes = (2 * N, 2 * N, 2, 2, 2, N, 1, 1, 1)
        self._v_pref = me.v_pref
        return _hip.env_state_of(SimpleNamespace(**dict(zip(names, torch.split(stage, sizes))))), stage, N, dev

    def _env_next_of_host_env(self):
        """`query_env` at E = 1: the reference asks its env (whose internal state is the current one) once per action;
        here the E = 1 view's batched env answers for the whole table at once (`_query_env`).  None without query_env."""
        if not self.query_env:
            return None
        venv = self.env.__dict__.get("_vec") if hasattr(self.env, "__dict__") else None
        if venv is None:
            raise AttributeError("query_env needs set_env(CrowdSim)")
        self.env._push_host_state()
        return self._query_env(venv)

    def _pack(self, dev):
        return pack_cadrl_network(self.model, dev)

    def _launch(self, net, st, b, A, E, N, dev, kin, gamma_pow, npos, nvel, rew, epsilon, seed, want_attention):
        rc = _hip.lib.mcn_cadrl_predict(C.byref(net), st, _hip.ptr(b["table"]), A, float(self.time_step), gamma_pow, kin,
                                        _hip.ptr(b["values"]), _hip.ptr(b["best"]), _hip.ptr(b["best_val"]),
                                        _hip.ptr(npos), _hip.ptr(nvel), _hip.ptr(rew), _hip.ptr(b["action"]),
                                        float(epsilon), seed, E, N, _hip.stream_ptr(dev))
        _hip.check(rc, "mcn_cadrl_predict")

    # ------------------------------------------------------------------ device plumbing (every look-ahead policy)
    def _gpu_device(self):
        d = self.device if isinstance(self.device, torch.device) else torch.device(self.device or "cuda")
        if d.type != "cuda":
            # the reference accepts --device cpu; this build's look-ahead only exists as HIP kernels
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    def _packed(self, dev):
        """ctypes net struct of device fragments, re-packed when a parameter changed since they were made or the device
        changed (_hip.weights_stamp).  Writes through `p.data` (`p.data.copy_`) are invisible: call refresh() after
        them."""
        stamp = _hip.weights_stamp(self.model.parameters(), dev)
        if self._frags is None or self._frags[0] != stamp:
            net, keep = self._pack(dev)
            self._frags = (stamp, net, keep)
        return self._frags[1]

    def refresh(self):
        """Re-pack the network at the next look-ahead (after a write the weight stamp cannot see)."""
        self._frags = None

    def _workspace_bytes(self, E, N, A):
        return 0

    def _lookahead(self, st, E, N, dev, want_attention=False, env_next=None, epsilon=0.0):
        """Launch the policy's look-ahead (`_launch`: mcn_sarl_predict, mcn_lstm_rl_predict, mcn_cadrl_predict) on an
        EnvState struct; returns (values[E,A], best[E], best_val[E], att); the chosen
        actions [E,2] (table row of `best`, zero where the robot stands on its goal) are left in self._bufs["action"].
        env_next = (next_hpos [E,N,2], next_hvel [E,N,2], rewards [E,A]): the `query_env` form -- the env's
        look-ahead states and rewards instead of propagate + compute_reward."""
        if self.action_space is None:
            raise RuntimeError("action space not built")
        A = len(self.action_space)
        key = (E, N, A, dev)
        if self._bufs.get("key") != key:
            nbytes = self._workspace_bytes(E, N, A)
            self._bufs = {
                "key": key,
                "ws": torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None,
                "values": torch.empty(E, A, dtype=torch.float64, device=dev),
                "best": torch.empty(E, dtype=torch.int32, device=dev),
                "best_val": torch.empty(E, dtype=torch.float64, device=dev),
                "action": torch.empty(E, 2, dtype=torch.float64, device=dev),
                "table": self._table(dev),
                "att": None,
            }
        b = self._bufs
        if want_attention and b["att"] is None:
            b["att"] = torch.empty(E, A, N, dtype=torch.float32, device=dev)
        net = self._packed(dev)
        kin = _hip.KIN_UNICYCLE if self.kinematics == "unicycle" else _hip.KIN_HOLONOMIC
        gamma_pow = pow(self.gamma, self.time_step * self._v_pref)       # multi_human_rl.py:52
        npos, nvel, rew = env_next if env_next is not None else (None, None, None)
        # a fresh 63-bit seed per call from torch's host generator (no device launch): torch.manual_seed() makes
        # training rollouts reproducible
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if epsilon > 0 else 0
        self._launch(net, st, b, A, E, N, dev, kin, gamma_pow, npos, nvel, rew, epsilon, seed, want_attention)
        return b["values"], b["best"], b["best_val"], b["att"]

    def _table(self, dev):
        """The action table on `dev`: uploaded once per table and device."""
        c = self._table_dev
        if c is None or c[0] is not self._action_table or c[1] != dev:
            c = self._table_dev = (self._action_table, dev,
                                   torch.from_numpy(np.ascontiguousarray(self._action_table)).to(dev))
        return c[2]

    def _query_env(self, venv):
        """`query_env = true` (multi_human_rl.py:37-38): what `env.onestep_lookahead(action)` returns for every action
        of the table, for all E envs of the batched env `venv`.  The humans react to the robot's CURRENT state
        (crowd_sim.py:336-342), so their next states do not depend on the candidate action: ONE mcn_env_step(update = 0)
        gives them; the reward (swept-circle test against the candidate action, goal test, time limit) does, and comes
        from one given-velocity mcn_env_step over the E x A (env, action) pairs on a scratch copy of the state.
        Returns (next_hpos [E,N,2], next_hvel [E,N,2], rewards [E,A])."""
        E, N, dev = venv.num_envs, venv._alloc_N, venv.device
        A = len(self.action_space)
        ob, _, _, _ = venv.onestep_lookahead(torch.zeros(E, 2, dtype=torch.float64, device=dev))
        npos, nvel = ob.pos.clone(), ob.vel.clone()
        rep = lambda t: t.repeat_interleave(A, 0).contiguous()
        x = dict(hpos=rep(venv.hpos), hvel=rep(venv.hvel), hrad=rep(venv.hrad), rpos=rep(venv.rpos), rvel=rep(venv.rvel),
                 rgoal=rep(venv.rgoal), rrad=rep(venv.rrad), rvpref=rep(venv.rvpref), rtheta=rep(venv.rtheta),
                 gtime=rep(venv.gtime))
        st = _hip.env_state_of(SimpleNamespace(hgoal=x["hpos"], hvpref=x["hrad"], **x))  # not read with given velocities
        acts = self._table(dev).repeat(E, 1).contiguous()
        given = rep(nvel)
        rec = torch.zeros(E * A, 3, dtype=torch.float64, device=dev)
        out = _hip.EnvOut(_hip.ptr(rec), None, None, None)
        cfg = venv._cfg_struct("given")
        cfg.count_hh = 0
        cfg.track_human_times = 0
        _hip.check(_hip.lib.mcn_env_step(cfg, st, _hip.ptr(acts), _hip.ptr(given), out, None, E * A, N, 1,
                                         _hip.stream_ptr(dev)), "mcn_env_step")
        return npos, nvel, rec[:, 0].reshape(E, A).contiguous()

    # ------------------------------------------------------------------ batched surface
    def predict_batch(self, env, want_values=False, hcount=None):
        """Look-ahead for all E environments of a VecCrowdSim: greedy in phase 'test' / 'val'; in phase 'train' each
        env independently takes a uniformly random table action with probability `epsilon` (multi_human_rl.py:27-29,
        one draw per env per step from torch's device generator) -- `best` is -2 for those envs.

        Returns (actions [E,2] float64 device tensor, best [E] int32; -1 where the robot already
        stands on its goal and the zero action is returned, multi_human_rl.py:22-23).  Both (and `values`) are the
        policy's own output buffers, written by the look-ahead launch: valid until the next predict_batch call.
        hcount ([E] int32 device tensor, optional): env e shows only its first hcount[e] pedestrians to the policy
        (the reference simply hands `predict` a shorter list, e.g. datagen.py:347-363)."""
        if self.action_space is None:
            self.build_action_space(float(env.robot.v_pref))
        dev = env.device
        self._v_pref = float(env.robot.v_pref)
        if hcount is not None and (hcount.dtype != torch.int32 or not hcount.is_contiguous() or
                                   hcount.numel() != env.num_envs):
            raise ValueError("hcount must be a contiguous int32 tensor with one entry per env")
        st = _hip.with_hcount(env._st, hcount)
        env_next = None
        if self.query_env:
            if hcount is not None:
                raise NotImplementedError("query_env with per-env pedestrian counts")
            env_next = self._query_env(env)
        eps = float(getattr(self, "epsilon", 0) or 0) if self.phase == "train" else 0.0
        # epsilon-greedy happens inside the look-ahead's argmax kernel (one draw per env per step from a counter-based
        # stream seeded from torch's generator): best == -2 marks the envs that explored
        values, best, best_val, _ = self._lookahead(st, env.num_envs, env._alloc_N, dev, env_next=env_next, epsilon=eps)
        actions = self._bufs["action"]              # written by the argmax kernel: no torch launches
        if want_values:
            return actions, best, values
        return actions, best
