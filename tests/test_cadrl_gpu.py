"""GPU: the CADRL look-ahead (lstm_rl_value.hip through mcn_cadrl_predict) against the reference's own CADRL.predict
(g23_cadrl.npz) and against a torch-float32 evaluation of the same module.

Bar: 1e-5 absolute on values; the chosen action must be identical wherever the top-2 gap exceeds it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import policy_ref as R  # noqa: E402

TOL = 1e-5


def _weights(g, prefix):
    import torch
    return {k[len(prefix):].replace("__", "."): torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def _policy(weights=None, seed=None, kinematics="holonomic", phase="test"):
    import torch
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.policy.cadrl import CADRL
    if seed is not None:
        torch.manual_seed(seed)
    p = CADRL()
    p.configure(configs.policy_config())
    p.kinematics = kinematics
    if weights is not None:
        p.model.load_state_dict(weights)
    p.set_device(torch.device("cuda", 0))
    p.set_phase(phase)
    p.time_step = 0.25
    return p


def _cpu_model(pol):
    import copy
    return copy.deepcopy(pol.model).cpu().float()


def _self_row(st, e):
    return [st.rpx[e], st.rpy[e], st.rvx[e], st.rvy[e], st.rr[e], st.rgx[e], st.rgy[e], 1.0, st.rtheta[e]]


def _hum(st, e):
    return np.stack([st.hpx[e], st.hpy[e], st.hvx[e], st.hvy[e], st.hr[e]], 1)


def _reached(st, e):
    return float(np.linalg.norm((st.rpy[e] - st.rgy[e], st.rpx[e] - st.rgx[e]))) < st.rr[e]


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_predict_matches_reference_fixture(kin, golden_dir):
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    g = np.load(os.path.join(golden_dir, "g23_cadrl.npz"))
    for seed in (0, 1):
        pol = _policy(_weights(g, "w%d__" % seed), kinematics=kin)
        for N in (1, 5):
            key = "pred%d_%s_N%d_" % (seed, kin, N)
            for s in range(g[key + "self"].shape[0]):
                me = FullState(*g[key + "self"][s].tolist())
                js = JointState(me, [ObservableState(*row) for row in g[key + "humans"][s].tolist()])
                act = pol.predict(js)
                want_vals, want_act = g[key + "values"][s], g[key + "action"][s]
                if np.isnan(want_vals[0]):
                    assert tuple(act) == (0, 0)
                    continue
                np.testing.assert_allclose(np.array(pol.action_values), want_vals, rtol=0, atol=TOL)
                top2 = np.sort(want_vals)[-2:]
                if top2[1] - top2[0] > 2 * TOL:
                    assert np.allclose(tuple(act), want_act, rtol=0, atol=0)


def test_train_phase_epsilon_and_last_state_match_reference(golden_dir):
    import torch
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    g = np.load(os.path.join(golden_dir, "g23_cadrl.npz"))
    pol = _policy(_weights(g, "w%d__" % int(g["eps_seed"])), phase="train")
    pol.set_epsilon(0.5)
    np.random.seed(2200 + int(g["eps_seed"]))
    for s in range(g["eps_selfs"].shape[0]):
        me = FullState(*g["eps_selfs"][s].tolist())
        js = JointState(me, [ObservableState(*row) for row in g["eps_humans"][s].tolist()])
        act = pol.predict(js)
        np.testing.assert_allclose([act.vx, act.vy], g["eps_actions"][s], rtol=0, atol=1e-12)
        torch.testing.assert_close(pol.last_state.cpu(), torch.from_numpy(g["eps_last_states"][s]), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size(N):
    import torch
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    rng = np.random.RandomState(230 + N)
    E = 4096
    pol = _policy(seed=3)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    torch.cuda.synchronize()
    values, best, actions = values.cpu().numpy().copy(), best.cpu().numpy().copy(), actions.cpu().numpy().copy()
    model, table = _cpu_model(pol), pol._action_table
    sample = sorted(set([0, 1, 15, 16, 17, 2047, 2048, E - 2, E - 1] + rng.choice(E, 60, replace=False).tolist()))
    for e in sample:
        if _reached(st, e):
            assert best[e] == -1 and tuple(actions[e]) == (0.0, 0.0)
        ref = R.policy_values(model, "cadrl", _self_row(st, e), _hum(st, e), table, "holonomic")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
        if best[e] >= 0:
            assert best[e] == int(np.argmax(values[e]))
            top2 = np.sort(ref)[-2:]
            if top2[1] - top2[0] > 2 * TOL:
                assert best[e] == int(np.argmax(ref))
    for e in sample[:8]:                       # the E = 1 path: same bits
        js = JointState(FullState(*_self_row(st, e)), [ObservableState(*row) for row in _hum(st, e).tolist()])
        pol.predict(js)
        if not _reached(st, e):
            assert np.array_equal(np.array(pol.action_values), values[e]), e


def test_hcount_masks_humans_out_of_the_min():
    import torch
    rng = np.random.RandomState(8)
    E, N = 300, 6
    pol = _policy(seed=5)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, crowded_frac=0.6)
    H.upload(env, st)
    hc = torch.from_numpy(rng.randint(1, N + 1, E).astype(np.int32)).cuda()
    _, _, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values, hcn = values.cpu().numpy(), hc.cpu().numpy()
    model = _cpu_model(pol)
    for e in range(0, E, 7):
        ref = R.policy_values(model, "cadrl", _self_row(st, e), _hum(st, e)[:int(hcn[e])], pol._action_table,
                              "holonomic")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_one_nan_human_makes_the_pair_nan():
    """torch.min propagates NaN (cadrl.py:164): one visible human with a NaN output makes every value of its env NaN;
    a NaN human beyond hcount does not."""
    import torch
    rng = np.random.RandomState(9)
    E, N = 40, 5
    pol = _policy(seed=6)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N)
    st.hvx[3, 2] = np.nan                       # env 3: human 2 visible
    st.hvx[5, 4] = np.nan                       # env 5: human 4, masked out below
    H.upload(env, st)
    hc = torch.full((E,), N, dtype=torch.int32, device="cuda")
    hc[5] = 4
    _, best, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values, best = values.cpu().numpy(), best.cpu().numpy()
    assert np.isnan(values[3]).all() and best[3] < 0
    assert np.isfinite(values[5]).all() and np.isfinite(values[4]).all()


def test_unicycle_and_query_env():
    import torch
    rng = np.random.RandomState(13)
    E, N = 64, 5
    pol = _policy(seed=8, kinematics="unicycle")
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = H.random_state(rng, E, N, randomize=True)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)
    H.upload(env, st)
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy().copy()
    model = _cpu_model(pol)
    for e in range(0, E, 5):
        ref = R.policy_values(model, "cadrl", _self_row(st, e), _hum(st, e), pol._action_table, "unicycle")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
    pol.query_env = True
    npos, nvel, rew = pol._query_env(env)
    npos, nvel, rew = npos.cpu().numpy(), nvel.cpu().numpy(), rew.cpu().numpy()
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    for e in range(0, E, 5):
        ref = R.policy_values(model, "cadrl", _self_row(st, e), _hum(st, e), pol._action_table, "unicycle",
                              nexts=np.concatenate([npos[e], nvel[e]], 1), rewards=rew[e])
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_epsilon_greedy_rate_and_rows():
    import torch
    rng = np.random.RandomState(4)
    E, N = 4096, 1
    pol = _policy(seed=2, phase="train")
    pol.set_epsilon(0.5)
    env = H.make_vec_env(E, N)
    H.upload(env, H.random_state(rng, E, N))
    torch.manual_seed(0)
    actions, best = pol.predict_batch(env)
    best, actions = best.cpu().numpy(), actions.cpu().numpy()
    live = best != -1
    rate = float((best[live] == -2).mean())
    assert abs(rate - 0.5) < 5 * np.sqrt(0.25 / live.sum())
    for e in np.nonzero(best == -2)[0]:
        assert (np.abs(pol._action_table - actions[e]).sum(1) == 0).any()
    rows = pol.transform_batch(env).cpu()
    assert rows.shape == (E, 13)
