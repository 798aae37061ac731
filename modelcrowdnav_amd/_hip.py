"""ctypes binding of libmcn_hip.so (C ABI: include/mcn.h).

The library is the product: there is no CPU fallback.  If it is missing, importing this
module raises, and every env / policy entry point above it fails with it.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- FIRST: libmcn_hip.so must bind to the HIP runtime torch already loaded,
#                     otherwise two runtimes coexist and torch streams are meaningless to our launches

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCN_HIP_LIB: an explicit path to another build of the same library (the diagnostic build of
# `make -C modelcrowdnav_amd/csrc diag`, used by tools/fixed_cost.py); version() says which build is loaded
LIB_PATH = os.environ.get("MCN_HIP_LIB") or os.path.join(_HERE, "csrc", "libmcn_hip.so")

MCN_OK, MCN_EINVAL, MCN_ELAUNCH = 0, -1, -2
MAX_HUMANS, MAX_LINES = 32, 10
INFO_NOTHING, INFO_DANGER, INFO_REACHGOAL, INFO_COLLISION, INFO_TIMEOUT = range(5)
HUMANS_ORCA, HUMANS_LINEAR, HUMANS_GIVEN, HUMANS_SOCIALFORCE = range(4)
KIN_HOLONOMIC, KIN_UNICYCLE = 0, 1
# include/mcn.h: MCN_SIZEOF_* ids of the network structs
SIZEOF_SARL_NET, SIZEOF_SGAN_NET, SIZEOF_MLP_WORLD_NET, SIZEOF_ATTN_WORLD_NET = 7, 8, 10, 11
SIZEOF_SARL_X3, SIZEOF_LSTM_RL_NET, SIZEOF_CADRL_NET = 12, 13, 14

_vp, _d, _f, _i = C.c_void_p, C.c_double, C.c_float, C.c_int32


class EnvCfg(C.Structure):
    _fields_ = [
        ("time_step", _d), ("time_limit", _d), ("success_reward", _d), ("collision_penalty", _d),
        ("discomfort_dist", _d), ("discomfort_penalty_factor", _d), ("orca_safety_space", _d),
        ("orca_neighbor_dist", _f), ("orca_time_horizon", _f),
        ("orca_max_neighbors", _i), ("robot_visible", _i), ("human_policy", _i),
        ("robot_kinematics", _i), ("count_hh", _i), ("track_human_times", _i),
    ]


class EnvState(C.Structure):
    _fields_ = [(k, _vp) for k in ("hpos", "hvel", "hgoal", "hrad", "hvpref", "rpos", "rvel", "rgoal", "rrad", "rvpref",
                                   "rtheta", "gtime", "human_times", "hcount")]


class EnvOut(C.Structure):
    _fields_ = [(k, _vp) for k in ("rec", "human_act", "nobs_pos", "nobs_vel", "lp3_queue")]


class StepRec(C.Structure):
    """mcn_step_rec: what one env reports per step (24 bytes)."""
    _fields_ = [("reward", _d), ("dmin", _d), ("done", C.c_uint8), ("info", C.c_uint8), ("reserved", C.c_uint16),
                ("hh_count", _i)]


class RollRec(C.Structure):
    """mcn_roll_rec: rollout state of one env (32 bytes)."""
    _fields_ = [("ep_return", _d), ("ep_steps", _i), ("fin_count", _i), ("next_case", _i), ("danger_count", _i),
                ("danger_dist_sum", _d)]


def step_rec_views(rec):
    """Typed strided views of a [E,3] float64 tensor laid out as mcn_step_rec[E]."""
    import torch
    b, w = rec.view(torch.uint8), rec.view(torch.int32)
    return dict(reward=rec[:, 0], dmin=rec[:, 1], done=b[:, 16], info=b[:, 17], hh_count=w[:, 5])


def roll_rec_views(state):
    """Typed strided views of a [E,4] float64 tensor laid out as mcn_roll_rec[E]."""
    import torch
    w = state.view(torch.int32)
    return dict(ep_return=state[:, 0], ep_steps=w[:, 2], fin_count=w[:, 3], next_case=w[:, 4],
                danger_count=w[:, 5], danger_dist_sum=state[:, 3])


class Rollout(C.Structure):
    _fields_ = [
        ("disc_table", _vp), ("disc_len", _i), ("danger_episodes", _i),
        ("state", _vp),
        ("fin_return", _vp), ("fin_time", _vp), ("fin_info", _vp), ("fin_slots", _i), ("danger_short_from", _i),
        ("pool_hpos", _vp), ("pool_hgoal", _vp), ("pool_hrad", _vp), ("pool_hvpref", _vp), ("pool_hvel", _vp),
        ("pool_size", _i), ("case_stride", _i),
        ("robot_start", _d * 2), ("robot_goal", _d * 2), ("robot_theta0", _d),
    ]


class ScenarioCfg(C.Structure):
    _fields_ = [("circle_radius", _d), ("square_width", _d), ("discomfort_dist", _d), ("human_radius", _d),
                ("human_v_pref", _d), ("robot_radius", _d), ("robot_start", _d * 2), ("robot_goal", _d * 2),
                ("rule", _i), ("randomize_attributes", _i)]


RULE_CIRCLE, RULE_SQUARE = 0, 1


class Tuning(C.Structure):
    """mcn_tuning: dispatch overrides, -1 = automatic."""
    _fields_ = [(k, _i) for k in ("force_generic", "quad_max_envs", "quad_split", "rollout_fused", "rollout_split",
                                  "step_block", "diag_noop", "pair_stream", "lp3_defer", "sarl_x3")]


class LstmRLNet(C.Structure):
    """mcn_lstm_rl_net: device pointers to the packed fragments of one LSTM-RL ValueNetwork1."""
    _fields_ = [(n, _vp) for n in ("w_gate", "b_gate", "w_m0", "b_m0", "w_m1", "b_m1", "w_m2", "b_m2", "w_m3", "b_m3")]


class CadrlNet(C.Structure):
    """mcn_cadrl_net: device pointers to the packed fragments of one CADRL ValueNetwork."""
    _fields_ = [(n, _vp) for n in ("w_l0", "b_l0", "w_l1", "b_l1", "w_l2", "b_l2", "w_l3", "b_l3")]


class McnError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "modelcrowdnav_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C modelcrowdnav_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.mcn_version.restype = C.c_char_p
    lib.mcn_env_step.argtypes = [C.POINTER(EnvCfg), C.POINTER(EnvState), _vp, _vp, C.POINTER(EnvOut),
                                 C.POINTER(Rollout), _i, _i, _i, _vp]
    lib.mcn_env_step.restype = C.c_int
    lib.mcn_env_lp3_queue_bytes.argtypes = [_i, _i]
    lib.mcn_env_lp3_queue_bytes.restype = C.c_int64
    lib.mcn_env_rollout.argtypes = [C.POINTER(EnvCfg), C.POINTER(EnvState), _vp, _i, C.POINTER(EnvOut),
                                    C.POINTER(Rollout), _i, _i, _vp]
    lib.mcn_env_rollout.restype = C.c_int
    # social-force humans: the model's strength / range / relaxation_rate follow cfg, no given_v
    lib.mcn_env_step_sf.argtypes = [C.POINTER(EnvCfg), _d, _d, _d, C.POINTER(EnvState), _vp, C.POINTER(EnvOut),
                                    C.POINTER(Rollout), _i, _i, _i, _vp]
    lib.mcn_env_step_sf.restype = C.c_int
    lib.mcn_env_rollout_sf.argtypes = [C.POINTER(EnvCfg), _d, _d, _d, C.POINTER(EnvState), _vp, _i, C.POINTER(EnvOut),
                                       C.POINTER(Rollout), _i, _i, _vp]
    lib.mcn_env_rollout_sf.restype = C.c_int
    # cfg, st, robot safety_space / neighbor_dist / max_neighbors / time_horizon, T, out, roll, six traces, E, N, stream
    lib.mcn_env_rollout_orca.argtypes = [C.POINTER(EnvCfg), C.POINTER(EnvState), _d, _f, _i, _f, _i, C.POINTER(EnvOut),
                                         C.POINTER(Rollout), _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_env_rollout_orca.restype = C.c_int
    # the same over social-force humans: strength / range / relaxation_rate follow cfg, then mcn_env_rollout_orca's own
    lib.mcn_env_rollout_orca_sf.argtypes = [C.POINTER(EnvCfg), _d, _d, _d, C.POINTER(EnvState), _d, _f, _i, _f, _i,
                                            C.POINTER(EnvOut), C.POINTER(Rollout), _vp, _vp, _vp, _vp, _vp, _vp, _i, _i,
                                            _vp]
    lib.mcn_env_rollout_orca_sf.restype = C.c_int
    lib.mcn_set_tuning.argtypes = [C.POINTER(Tuning)]
    lib.mcn_set_tuning.restype = C.c_int
    lib.mcn_get_tuning.argtypes = [C.POINTER(Tuning)]
    lib.mcn_get_tuning.restype = C.c_int
    lib.mcn_scenario_pool.argtypes = [C.POINTER(ScenarioCfg), C.c_uint64, C.c_int64, _i, _i, _vp, _vp, _vp, _vp, _vp]
    lib.mcn_scenario_pool.restype = C.c_int
    lib.mcn_orca_batch.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _f, _i, _f, _f, _vp]
    lib.mcn_orca_batch.restype = C.c_int
    # st, sim_vel, select, max_steps, steps, traj, time_step, neighbor_dist, max_neighbors, time_horizon, E, N, stream
    lib.mcn_orca_finish.argtypes = [C.POINTER(EnvState), _vp, _vp, _i, _vp, _vp, _d, _f, _i, _f, _i, _i, _vp]
    lib.mcn_orca_finish.restype = C.c_int
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lib.mcn_pack_linear.argtypes = [fp, fp, _i, _i, ip, _i, ip, _i, fp, fp]
    lib.mcn_pack_linear.restype = C.c_int
    lib.mcn_sarl_workspace_bytes.argtypes = [_i, _i, _i]
    lib.mcn_sarl_workspace_bytes.restype = C.c_int64
    lib.mcn_sarl_lookahead.argtypes = [_vp, C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp,
                                       _i, _i, _vp]
    lib.mcn_sarl_lookahead.restype = C.c_int
    lib.mcn_sarl_lookahead_env.argtypes = [_vp, C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_sarl_lookahead_env.restype = C.c_int
    lib.mcn_sarl_predict.argtypes = [_vp, C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _d, C.c_uint64, _i, _i, _vp]
    lib.mcn_sarl_predict.restype = C.c_int
    lib.mcn_sarl_om_prepare.argtypes = [C.POINTER(EnvState), _d, _vp, _vp, _d, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_sarl_om_prepare.restype = C.c_int
    lib.mcn_sarl_predict_om.argtypes = [_vp, C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _d, C.c_uint64, _vp, _i, _i, _vp]
    lib.mcn_sarl_predict_om.restype = C.c_int
    lib.mcn_sarl_train_param_count.argtypes, lib.mcn_sarl_train_param_count.restype = [_i], C.c_int64
    lib.mcn_sarl_train_workspace_bytes.argtypes, lib.mcn_sarl_train_workspace_bytes.restype = [_i, _i, _i], C.c_int64
    # params, input_dim, states, values, rows, B, N, workspace, grad, loss, stream
    lib.mcn_sarl_loss_grad.argtypes = [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]
    lib.mcn_sarl_loss_grad.restype = C.c_int
    # params, momentum_buf, grad, count, lr, momentum, stream
    lib.mcn_sgd_momentum_step.argtypes = [_vp, _vp, _vp, C.c_int64, _f, _f, _vp]
    lib.mcn_sgd_momentum_step.restype = C.c_int
    lib.mcn_cadrl_train_param_count.argtypes, lib.mcn_cadrl_train_param_count.restype = [], C.c_int64
    lib.mcn_cadrl_train_workspace_bytes.argtypes, lib.mcn_cadrl_train_workspace_bytes.restype = [_i], C.c_int64
    # params, states, values, rows, B, workspace, grad, loss, stream
    lib.mcn_cadrl_loss_grad.argtypes, lib.mcn_cadrl_loss_grad.restype = [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp], C.c_int
    lib.mcn_lstm_rl_train_param_count.argtypes, lib.mcn_lstm_rl_train_param_count.restype = [], C.c_int64
    lib.mcn_lstm_rl_train_workspace_bytes.argtypes, lib.mcn_lstm_rl_train_workspace_bytes.restype = [_i, _i], C.c_int64
    # params, states, values, rows, B, N, workspace, grad, loss, stream
    lib.mcn_lstm_rl_loss_grad.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]
    lib.mcn_lstm_rl_loss_grad.restype = C.c_int
    lib.mcn_lstm_rl_predict.argtypes = [C.POINTER(LstmRLNet), C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _d, C.c_uint64, _i, _i, _vp]
    lib.mcn_lstm_rl_predict.restype = C.c_int
    lib.mcn_lstm_rl_order.argtypes, lib.mcn_lstm_rl_order.restype = [C.POINTER(EnvState), _vp, _i, _i, _vp], C.c_int
    lib.mcn_cadrl_predict.argtypes = [C.POINTER(CadrlNet), C.POINTER(EnvState), _vp, _i, _d, _d, _i, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _d, C.c_uint64, _i, _i, _vp]
    lib.mcn_cadrl_predict.restype = C.c_int
    lib.mcn_mlp_world_step.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_mlp_world_step.restype = C.c_int
    lib.mcn_attn_world_workspace_bytes.argtypes = [_i, _i]
    lib.mcn_attn_world_workspace_bytes.restype = C.c_int64
    lib.mcn_attn_world_step.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_attn_world_step.restype = C.c_int
    lib.mcn_attn_world_train_param_count.argtypes, lib.mcn_attn_world_train_param_count.restype = [], C.c_int64
    lib.mcn_attn_world_train_workspace_bytes.argtypes = [_i, _i]
    lib.mcn_attn_world_train_workspace_bytes.restype = C.c_int64
    # params, cur, nxt, rows, B, N, workspace, grad (or NULL), loss, stream
    lib.mcn_attn_world_loss_grad.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]
    lib.mcn_attn_world_loss_grad.restype = C.c_int
    # params, exp_avg, exp_avg_sq, grad, count, lr, beta1, beta2, eps, step, stream
    lib.mcn_adam_step.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, _f, _f, _f, _f, _i, _vp]
    lib.mcn_adam_step.restype = C.c_int
    lib.mcn_mlp_world_train_param_count.argtypes, lib.mcn_mlp_world_train_param_count.restype = [_i], C.c_int64
    lib.mcn_mlp_world_train_workspace_bytes.argtypes = [_i, _i]
    lib.mcn_mlp_world_train_workspace_bytes.restype = C.c_int64
    # params, cur, nxt, rows, B, N, drop_p, seed, step, workspace, grad (or NULL), loss, stream
    lib.mcn_mlp_world_loss_grad.argtypes = [_vp, _vp, _vp, _vp, _i, _i, _f, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _vp]
    lib.mcn_mlp_world_loss_grad.restype = C.c_int
    # seed, step, layer, B, width, p, keep (host)
    lib.mcn_dropout_mask.argtypes = [C.c_uint64, C.c_uint64, _i, _i, _i, _f, _vp]
    lib.mcn_dropout_mask.restype = C.c_int
    lib.mcn_sgan_workspace_bytes.argtypes = [_i, _i]
    lib.mcn_sgan_workspace_bytes.restype = C.c_int64
    lib.mcn_sgan_step.argtypes = [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _d, _i, _i, _vp]
    lib.mcn_sgan_step.restype = C.c_int
    lib.mcn_sgan_predict.argtypes = [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.mcn_sgan_predict.restype = C.c_int
    lib.mcn_pack_x3_bytes.argtypes, lib.mcn_pack_x3_bytes.restype = [_i, _i], C.c_int64
    lib.mcn_pack_x3.argtypes, lib.mcn_pack_x3.restype = [C.POINTER(C.c_float), _i, _i, _vp], C.c_int
    lib.mcn_abi_version.restype = _i
    lib.mcn_sizeof.argtypes, lib.mcn_sizeof.restype = [_i], C.c_int64
    lib.mcn_last_dispatch.restype = C.c_char_p
    lib.mcn_last_rollout_form.restype = _i
    _check_abi(lib)
    return lib


ABI_VERSION = 5          # include/mcn.h: MCN_ABI_VERSION this binding's struct mirrors were written against


def _check_abi(lib):
    """A library built from another header must not receive these struct mirrors (include/mcn.h: ABI guard)."""
    got = int(lib.mcn_abi_version())
    if got != ABI_VERSION:
        raise ImportError("modelcrowdnav_amd: %s has ABI %d, this binding was written for ABI %d -- rebuild the library "
                          "(make -C modelcrowdnav_amd/csrc)" % (LIB_PATH, got, ABI_VERSION))
    check_mirrors({0: EnvCfg, 1: EnvState, 2: EnvOut, 3: Rollout, 4: Tuning, 5: StepRec, 6: RollRec, 9: ScenarioCfg,
                   SIZEOF_LSTM_RL_NET: LstmRLNet, SIZEOF_CADRL_NET: CadrlNet}, lib)


def check_mirrors(mirrors, lib_=None):
    """{MCN_SIZEOF_* id: ctypes mirror}: each mirror must have the size of its C struct.  The policy modules check
    their own net mirrors with this when they are imported (this module does not import them)."""
    lib_ = lib if lib_ is None else lib_
    for which, cls in mirrors.items():
        if int(lib_.mcn_sizeof(which)) != C.sizeof(cls):
            raise ImportError("modelcrowdnav_amd: struct %s is %d bytes here, %d in %s" %
                              (cls.__name__, C.sizeof(cls), int(lib_.mcn_sizeof(which)), LIB_PATH))


def weights_stamp(params, dev):
    """What packed HIP weight fragments were made from: every parameter's identity, storage and version counter, and
    the target device.  It changes on in-place writes through the parameter itself (optimizer steps, load_state_dict,
    `p.add_` / `p.copy_` under no_grad), on `p.data = t` (new storage) and on a device move.  Writes through `p.data`
    (`p.data.copy_`, `p.data.mul_`) bypass the version counter and keep the storage: the adapters cannot see them, so
    call their `refresh()` afterwards."""
    return tuple((id(p), p.data_ptr(), p._version) for p in params) + (str(dev),)


def last_dispatch():
    """Kernel family the calling thread's latest mcn_env_step / mcn_env_rollout dispatched to (mcn_last_dispatch)."""
    return lib.mcn_last_dispatch().decode()


def last_rollout_form():
    """Form of the fused rollout kernel the calling thread's latest mcn_env_rollout launched: 0, 1 or 2 (four
    wavefronts); -1 when it did not take the fused quad path (mcn_last_rollout_form)."""
    return int(lib.mcn_last_rollout_form())


lib = _load()

# every symbol include/mcn.h declares; tests/test_abi.py checks the .so exports each one
EXPORTED = ["mcn_version", "mcn_abi_version", "mcn_sizeof", "mcn_last_dispatch", "mcn_last_rollout_form", "mcn_pack_x3", "mcn_pack_x3_bytes", "mcn_set_tuning", "mcn_get_tuning", "mcn_env_step", "mcn_env_lp3_queue_bytes", "mcn_env_rollout", "mcn_env_rollout_orca", "mcn_env_step_sf", "mcn_env_rollout_sf", "mcn_env_rollout_orca_sf", "mcn_scenario_pool", "mcn_orca_batch", "mcn_orca_finish", "mcn_pack_linear", "mcn_sarl_workspace_bytes",
            "mcn_sarl_lookahead", "mcn_sarl_lookahead_env", "mcn_sarl_predict", "mcn_sarl_om_prepare", "mcn_sarl_predict_om", "mcn_sgan_workspace_bytes", "mcn_sgan_step", "mcn_sgan_predict", "mcn_mlp_world_step", "mcn_attn_world_workspace_bytes",
            "mcn_attn_world_step", "mcn_lstm_rl_predict", "mcn_lstm_rl_order", "mcn_cadrl_predict",
            "mcn_sarl_train_param_count", "mcn_sarl_train_workspace_bytes", "mcn_sarl_loss_grad", "mcn_sgd_momentum_step",
            "mcn_attn_world_train_param_count", "mcn_attn_world_train_workspace_bytes", "mcn_attn_world_loss_grad", "mcn_adam_step",
            "mcn_dropout_mask", "mcn_mlp_world_train_param_count", "mcn_mlp_world_train_workspace_bytes", "mcn_mlp_world_loss_grad",
            "mcn_cadrl_train_param_count", "mcn_cadrl_train_workspace_bytes", "mcn_cadrl_loss_grad",
            "mcn_lstm_rl_train_param_count", "mcn_lstm_rl_train_workspace_bytes", "mcn_lstm_rl_loss_grad"]


def check(rc, what):
    if rc != MCN_OK:
        raise McnError("%s failed with code %d (%s)" % (what, rc, {-1: "MCN_EINVAL", -2: "MCN_ELAUNCH"}.get(rc, "?")))


def get_tuning():
    t = Tuning()
    check(lib.mcn_get_tuning(C.byref(t)), "mcn_get_tuning")
    return t


def set_tuning(**kw):
    """Override kernel dispatch (tests, tuning): set_tuning(quad_max_envs=0, force_generic=1); no arguments =
    back to the initial (automatic / environment) values.  The given fields are laid over the CURRENT settings.
    Returns the previous settings.  Process-wide; launches snapshot the settings under the library's lock."""
    prev = get_tuning()
    if not kw:
        check(lib.mcn_set_tuning(None), "mcn_set_tuning")
        return prev
    t = Tuning.from_buffer_copy(prev)            # overlay: a nested tuned(...) keeps the outer overrides
    for k, v in kw.items():
        if k not in dict(Tuning._fields_):
            raise TypeError("unknown tuning field %r" % k)
        setattr(t, k, int(v))
    check(lib.mcn_set_tuning(C.byref(t)), "mcn_set_tuning")
    return prev


class tuned:
    """Context manager: `with tuned(rollout_fused=1): ...` restores the previous dispatch on exit."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.prev = set_tuning(**self.kw)
        return self

    def __exit__(self, *exc):
        check(lib.mcn_set_tuning(C.byref(self.prev)), "mcn_set_tuning")
        return False


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def env_state_of(obj):
    """EnvState of an object that holds the state tensors as attributes named like the struct's fields (a VecCrowdSim,
    a shadow view of one); a missing or None attribute -- `hcount` of a plain env -- is a null pointer."""
    return EnvState(*[ptr(getattr(obj, k, None)) for k, _ in EnvState._fields_])


def with_hcount(st, hcount):
    """The EnvState `st` showing only the first hcount[e] pedestrians of env e ([E] int32 device tensor): a copy with
    that pointer; `st` itself for None."""
    if hcount is None:
        return st
    st = EnvState.from_buffer_copy(st)
    st.hcount = ptr(hcount)
    return st


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def version():
    return lib.mcn_version().decode()


def device_arch(device=None):
    """gcnArchName of the device the kernels will run on (queried through torch's runtime)."""
    return torch.cuda.get_device_properties(device if device is not None else torch.cuda.current_device()).gcnArchName
