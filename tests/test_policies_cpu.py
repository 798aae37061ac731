"""CPU: the LSTM-RL and CADRL policies resolve, build their reference module trees, reproduce the reference's torch
forwards (g22_lstm_rl / g23_cadrl) and sort humans as LstmRL.predict does; their ctypes mirrors match the library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from modelcrowdnav_amd import configs

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def _weights(g, prefix):
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def _make(name, cfg=None):
    from modelcrowdnav_amd.policy.policy_factory import policy_factory
    p = policy_factory[name]()
    p.configure(cfg or configs.policy_config())
    return p


def test_factory_and_dropin_resolve_both_policies():
    from modelcrowdnav_amd import dropin
    from modelcrowdnav_amd.policy.cadrl import CADRL
    from modelcrowdnav_amd.policy.lstm_rl import LstmRL
    dropin.install()
    from crowd_nav.policy.policy_factory import policy_factory
    import crowd_nav.policy.lstm_rl as ref_lstm
    assert policy_factory["lstm_rl"] is LstmRL and policy_factory["cadrl"] is CADRL
    assert ref_lstm.LstmRL is LstmRL
    assert hasattr(LstmRL, "predict_batch") and hasattr(LstmRL, "transform_batch")
    assert hasattr(CADRL, "predict_batch") and hasattr(CADRL, "transform_batch")


@pytest.mark.parametrize("name,fixture", [("lstm_rl", "g22_lstm_rl.npz"), ("cadrl", "g23_cadrl.npz")])
def test_state_dict_keys_match_fixture(name, fixture):
    g = _golden(fixture)
    want = sorted(_weights(g, "w0__"))
    p = _make(name)
    assert sorted(p.model.state_dict()) == want
    for k, v in p.model.state_dict().items():
        assert tuple(v.shape) == tuple(g["w0__" + k.replace(".", "__")].shape)


@pytest.mark.parametrize("name,fixture", [("lstm_rl", "g22_lstm_rl.npz"), ("cadrl", "g23_cadrl.npz")])
def test_torch_forward_matches_reference(name, fixture):
    g = _golden(fixture)
    for seed in (0, 1):
        p = _make(name)
        p.model.load_state_dict(_weights(g, "w%d__" % seed))
        for N in (1, 5, 10):
            x = torch.from_numpy(g["vn%d_in_N%d" % (seed, N)])
            with torch.no_grad():
                if name == "cadrl":
                    v = p.model(x.reshape(-1, 13)).reshape(x.shape[0], N)
                else:
                    v = p.model(x)
            np.testing.assert_allclose(v.numpy(), g["vn%d_out_N%d" % (seed, N)], rtol=0, atol=1e-6)


@pytest.mark.parametrize("key", ["with_om", "with_interaction_module"])
def test_unsupported_switches_raise(key):
    cfg = configs.policy_config()
    cfg.set("lstm_rl", key, "true")
    with pytest.raises(NotImplementedError):
        _make("lstm_rl", cfg)


def test_struct_mirrors_match_library():
    from modelcrowdnav_amd import _hip
    assert int(_hip.lib.mcn_sizeof(_hip.SIZEOF_LSTM_RL_NET)) == ctypes.sizeof(_hip.LstmRLNet) == 10 * 8
    assert int(_hip.lib.mcn_sizeof(_hip.SIZEOF_CADRL_NET)) == ctypes.sizeof(_hip.CadrlNet) == 8 * 8


def test_bad_arguments_are_rejected_on_host():
    from modelcrowdnav_amd import _hip
    st = _hip.EnvState()
    assert _hip.lib.mcn_lstm_rl_predict(None, st, None, 81, 0.25, 0.9, 0, None, None, None, None, None, None, None,
                                        None, 0.0, 0, 4, 5, None) == _hip.MCN_EINVAL
    assert _hip.lib.mcn_cadrl_predict(None, st, None, 81, 0.25, 0.9, 0, None, None, None, None, None, None,
                                      None, 0.0, 0, 4, 5, None) == _hip.MCN_EINVAL
    assert _hip.lib.mcn_lstm_rl_order(st, None, 4, 5, None) == _hip.MCN_EINVAL


def test_host_sort_equals_reference_order():
    """sort_humans (the E = 1 path's host sort) reproduces the order the reference's LstmRL.predict left in the state,
    tie states included (stable: equal distances keep their index order)."""
    from modelcrowdnav_amd.envs.utils.state import FullState, JointState, ObservableState
    from modelcrowdnav_amd.policy.lstm_rl import sort_humans
    g = _golden("g22_lstm_rl.npz")
    ties = 0
    for key in [k[:-4] for k in g.files if k.startswith("pred") and k.endswith("self")]:
        for s in range(g[key + "self"].shape[0]):
            me = FullState(*g[key + "self"][s].tolist())
            hs = [ObservableState(*row) for row in g[key + "humans"][s].tolist()]
            got = np.array([[h.px, h.py, h.vx, h.vy, h.radius] for h in sort_humans(JointState(me, hs))])
            assert np.array_equal(got, g[key + "sorted"][s])
            d = [np.linalg.norm(np.array(h.position) - np.array(me.position)) for h in hs]
            ties += len(d) - len(set(d))
    assert ties > 0, "the fixture has no exact distance ties"


def test_cadrl_transform_batch_refuses_several_humans():
    from modelcrowdnav_amd.policy.cadrl import CADRL

    class _Env:
        _alloc_N = 5
    with pytest.raises(AssertionError):
        CADRL.transform_batch(_make("cadrl"), _Env())


def _lookahead_args(_hip, body):
    """Arguments of mcn_lstm_rl_predict / mcn_cadrl_predict that pass every check of lookahead_args_ok: non-null
    dummy host pointers (never dereferenced: each call below breaks one check, so validation returns first)."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    net = _hip.LstmRLNet() if body == "lstm_rl" else _hip.CadrlNet()
    for name, _ in net._fields_:
        setattr(net, name, p)
    st = _hip.EnvState()
    for name, _ in st._fields_:
        setattr(st, name, p)
    args = dict(net=net, st=st, actions=p, A=81, time_step=0.25, gamma_pow=0.9, kinematics=_hip.KIN_HOLONOMIC,
                values=p, best=p, best_val=p, order=p, next_hpos=None, next_hvel=None, rewards=None, action_out=p,
                epsilon=0.0, seed=0, E=4, N=5, stream=None)
    return args, buf


def copy_struct(s):
    return type(s).from_buffer_copy(s)


def _call_lookahead(_hip, body, a):
    ref = lambda s: ctypes.byref(s) if s is not None else None
    head = (ref(a["net"]), ref(a["st"]), a["actions"], a["A"], a["time_step"], a["gamma_pow"], a["kinematics"],
            a["values"], a["best"], a["best_val"])
    tail = (a["next_hpos"], a["next_hvel"], a["rewards"], a["action_out"], a["epsilon"], a["seed"], a["E"], a["N"],
            a["stream"])
    if body == "lstm_rl":
        return _hip.lib.mcn_lstm_rl_predict(*head, a["order"], *tail)
    return _hip.lib.mcn_cadrl_predict(*head, *tail)


def _bad_lookahead_cases(body, p):
    """(what, {argument: bad value}, {EnvState / net field: None}) -- one check of lookahead_args_ok each."""
    nan = float("nan")
    cases = [("net", dict(net=None), {}), ("st", dict(st=None), {})]
    cases += [(k, {k: None}, {}) for k in ("actions", "values", "best", "best_val", "action_out")]
    cases += [("epsilon %r" % v, dict(epsilon=v), {}) for v in (-1e-9, 1.0 + 1e-9, nan, float("inf"))]
    cases += [("E %d" % v, dict(E=v), {}) for v in (0, -1)]
    cases += [("N %d" % v, dict(N=v), {}) for v in (0, -1, 33)]
    cases += [("A %d" % v, dict(A=v), {}) for v in (0, -1)]
    cases += [("st." + f, {}, {("st", f): None}) for f in ("hpos", "hvel", "hrad", "rpos", "rgoal", "rrad", "rvpref")]
    cases += [("kinematics %d" % v, dict(kinematics=v), {}) for v in (-1, 2)]
    cases += [("unicycle without rtheta", dict(kinematics=1), {("st", "rtheta"): None})]
    cases += [("next_hpos alone", dict(next_hpos=p), {}), ("next_hvel alone", dict(next_hvel=p), {}),
              ("rewards alone", dict(rewards=p), {}), ("next_hpos without rewards", dict(next_hpos=p, next_hvel=p), {}),
              ("next_hpos without next_hvel", dict(next_hpos=p, rewards=p), {}),
              ("rewards without next_hvel", dict(next_hvel=p, rewards=p), {})]
    cases += [("time_step %r" % v, dict(time_step=v), {}) for v in (0.0, -0.0, -0.25, nan, -float("inf"))]
    from modelcrowdnav_amd import _hip
    fields = [n for n, _ in (_hip.LstmRLNet if body == "lstm_rl" else _hip.CadrlNet)._fields_]
    cases += [("net." + f, {}, {("net", f): None}) for f in fields]
    return cases


@pytest.mark.parametrize("body", ["lstm_rl", "cadrl"])
def test_every_lookahead_argument_check_rejects_on_host(body):
    """Each check of lookahead_args_ok (mcn_api.hip) on its own: every other argument non-null and in range."""
    from modelcrowdnav_amd import _hip
    args, buf = _lookahead_args(_hip, body)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    cases = _bad_lookahead_cases(body, p)
    assert len(cases) > 40
    for what, over, fields in cases:
        a = dict(args, net=copy_struct(args["net"]), st=copy_struct(args["st"]))
        for (obj, f), v in fields.items():
            setattr(a[obj], f, v)
        a.update(over)
        assert _call_lookahead(_hip, body, a) == _hip.MCN_EINVAL, what


def test_every_order_argument_check_rejects_on_host():
    from modelcrowdnav_amd import _hip
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    st = _hip.EnvState()
    for name, _ in st._fields_:
        setattr(st, name, p)
    lib = _hip.lib
    for f in ("hpos", "rpos"):
        s = copy_struct(st)
        setattr(s, f, None)
        assert lib.mcn_lstm_rl_order(s, p, 4, 5, None) == _hip.MCN_EINVAL, f
    assert lib.mcn_lstm_rl_order(None, p, 4, 5, None) == _hip.MCN_EINVAL
    assert lib.mcn_lstm_rl_order(st, None, 4, 5, None) == _hip.MCN_EINVAL
    for E, N in ((0, 5), (-1, 5), (4, 0), (4, -1), (4, 33)):
        assert lib.mcn_lstm_rl_order(st, p, E, N, None) == _hip.MCN_EINVAL, (E, N)


def test_stable_desc_order_puts_inf_first_and_nan_last():
    """The order oracle's rule: first strict maximum, ties in index order, NaN distances last in index order, slots
    >= count untouched."""
    from tests import policy_ref as R
    inf, nan = float("inf"), float("nan")
    me = [0.0, 0.0]
    hum = lambda xs: np.array([[x, 0.0, 0.0, 0.0, 0.3] for x in xs])
    assert R.stable_desc_order(me, hum([nan, 1, 2, 3])).tolist() == [3, 2, 1, 0]
    assert R.stable_desc_order(me, hum([1, nan, 3, -inf, 3, inf, nan])).tolist() == [3, 5, 2, 4, 0, 1, 6]
    assert R.stable_desc_order(me, hum([nan, nan, nan])).tolist() == [0, 1, 2]
    assert R.stable_desc_order(me, hum([1, -2, 2, nan, inf]), 3).tolist() == [1, 2, 0, 3, 4]
    assert R.stable_desc_order([nan, 0.0], hum([1, 2])).tolist() == [0, 1]


@pytest.mark.parametrize("N", [5, 9, 32])
def test_order_batch_holds_near_ties_the_unfused_norm_orders_differently(N):
    """The GPU order test's teeth: its near-tie envs hold orders that an un-fused x*x + y*y norm gets wrong (so a
    re-contracted norm2d would fail), the order oracle (np.linalg.norm) is the fused sqrt(fma(y, y, x*x)) on every
    finite env, and exact ties, +inf and NaN distances occur where the batch names them."""
    from tests import lookahead_states as LS
    from tests import policy_ref as R
    st, hc, names = LS.order_batch(N)
    dis = LS.fused_unfused_disagreements(st)
    assert len(dis) >= 3 and all(names[e] == "near-tie" for e in dis), (len(dis), {names[e] for e in dis})
    kinds = {}
    for e in range(st.E):
        row = [st.rpx[e], st.rpy[e]]
        hum = np.stack([st.hpx[e], st.hpy[e]], 1)
        d = np.array([np.linalg.norm(hum[i] - np.array(row)) for i in range(N)])
        if np.isfinite(d).all():
            assert np.array_equal(R.stable_desc_order(row, hum), LS.orders(st, e, LS.fused_norm)), e
        u = [LS.unfused_norm(*(hum[i] - np.array(row))) for i in range(N)]
        k = kinds.setdefault(names[e], set())
        if len(set(d[np.isfinite(d)].tolist())) < np.isfinite(d).sum():
            k.add("tie")
        if np.isfinite(u).all() and len(set(u)) < len(set(d.tolist())):
            k.add("unfused-tie")
        if np.isposinf(d).sum() > 1:
            k.add("inf-tie")
        if np.isnan(d[0]):
            k.add("nan-first")
        if np.isnan(d).all():
            k.add("all-nan")
    if N > 3:
        assert "tie" in kinds["ties"]
    assert "unfused-tie" in kinds["near-tie"]
    assert "inf-tie" in kinds["inf-tie"] and "nan-first" in kinds["nan-first"] and "all-nan" in kinds["nan-robot"]
    assert "all-nan" in kinds["all-nan"]
    assert (hc[[e for e in range(st.E) if names[e] == "nonfinite-beyond-hcount"]] < N).any()
