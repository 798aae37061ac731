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
