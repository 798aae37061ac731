"""GPU: the LSTM-RL look-ahead (lstm_rl_value.hip through mcn_lstm_rl_predict) against the reference's own
LstmRL.predict (g22_lstm_rl.npz) and against a torch-float32 evaluation of the same module on rows sorted in the test.

Bar: 1e-5 absolute on values (BASELINE.json north_star); the chosen action must be identical wherever the top-2 gap
exceeds it."""
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
    from modelcrowdnav_amd.policy.lstm_rl import LstmRL
    if seed is not None:
        torch.manual_seed(seed)
    p = LstmRL()
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


def _tie_state(rng, E, N):
    """random_state with exact distance ties in every 3rd env: mirrored / duplicated humans, a human on the robot."""
    st = H.random_state(rng, E, N, randomize=True)
    for e in range(0, E, 3):
        st.rpx[e], st.rpy[e] = rng.randint(-8, 9, 2) * 0.25
        st.hpx[e, 0], st.hpy[e, 0] = st.rpx[e] + 0.625, st.rpy[e] - 1.25
        st.hpx[e, 1], st.hpy[e, 1] = st.rpx[e] - 0.625, st.rpy[e] + 1.25       # mirrored through the robot
        st.hpx[e, 2], st.hpy[e, 2] = st.hpx[e, 0], st.hpy[e, 0]                 # duplicate
        st.hpx[e, N - 1], st.hpy[e, N - 1] = st.rpx[e], st.rpy[e]               # on the robot
    return st


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_predict_matches_reference_fixture(kin, golden_dir):
    """LstmRL.predict(JointState): action_values, chosen action and the host-sorted human list of the reference."""
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    g = np.load(os.path.join(golden_dir, "g22_lstm_rl.npz"))
    for seed in (0, 1):
        pol = _policy(_weights(g, "w%d__" % seed), kinematics=kin)
        for N in (5, 10):
            key = "pred%d_%s_N%d_" % (seed, kin, N)
            for s in range(g[key + "self"].shape[0]):
                me = FullState(*g[key + "self"][s].tolist())
                js = JointState(me, [ObservableState(*row) for row in g[key + "humans"][s].tolist()])
                act = pol.predict(js)
                got_sorted = np.array([[h.px, h.py, h.vx, h.vy, h.radius] for h in js.human_states])
                assert np.array_equal(got_sorted, g[key + "sorted"][s])
                want_vals, want_act = g[key + "values"][s], g[key + "action"][s]
                if np.isnan(want_vals[0]):
                    assert tuple(act) == (0, 0)
                    continue
                got = np.array(pol.action_values)
                np.testing.assert_allclose(got, want_vals, rtol=0, atol=TOL)
                # the device sorted the host-sorted list again: identity (one order definition, same distances)
                assert pol.last_order[0].cpu().tolist() == list(range(N))
                top2 = np.sort(want_vals)[-2:]
                if top2[1] - top2[0] > 2 * TOL:
                    assert np.allclose(tuple(act), want_act, rtol=0, atol=0)


def test_train_phase_epsilon_and_last_state_match_reference(golden_dir):
    """epsilon 0.5 on numpy's global stream (multi_human_rl.py:27-29) and last_state = transform(sorted state)."""
    import torch
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    g = np.load(os.path.join(golden_dir, "g22_lstm_rl.npz"))
    pol = _policy(_weights(g, "w%d__" % int(g["eps_seed"])), phase="train")
    pol.set_epsilon(0.5)
    np.random.seed(2200 + int(g["eps_seed"]))
    for s in range(g["eps_selfs"].shape[0]):
        me = FullState(*g["eps_selfs"][s].tolist())
        js = JointState(me, [ObservableState(*row) for row in g["eps_humans"][s].tolist()])
        pol.action_values = None
        act = pol.predict(js)
        np.testing.assert_allclose([act.vx, act.vy], g["eps_actions"][s], rtol=0, atol=1e-12)
        torch.testing.assert_close(pol.last_state.cpu(), torch.from_numpy(g["eps_last_states"][s]), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size(N):
    """4096 envs x 81 actions: every value of >= 64 sampled envs (0, 15, 16, E-1 among them) against torch on rows
    sorted here; the device order against numpy's stable descending sort (tie envs included); transform_batch rows
    against the E = 1 transform of the sorted state; the E = 1 path gives the same bits for the same env."""
    import torch
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    rng = np.random.RandomState(220 + N)
    E = 4096
    pol = _policy(seed=3)
    env = H.make_vec_env(E, N)
    st = _tie_state(rng, E, N)
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    torch.cuda.synchronize()
    values, best, actions = values.cpu().numpy().copy(), best.cpu().numpy().copy(), actions.cpu().numpy().copy()
    order = pol.last_order.cpu().numpy().copy()
    assert np.array_equal(pol.human_order(env).cpu().numpy(), order)
    rows = pol.transform_batch(env).cpu()
    model, table = _cpu_model(pol), pol._action_table
    sample = sorted(set([0, 1, 3, 15, 16, 17, 2047, 2048, E - 2, E - 1] + rng.choice(E, 60, replace=False).tolist()))
    for e in sample:
        want_order = R.stable_desc_order(_self_row(st, e), _hum(st, e))
        assert order[e].tolist() == want_order.tolist(), e
        if _reached(st, e):
            assert best[e] == -1 and tuple(actions[e]) == (0.0, 0.0)
        ref = R.policy_values(model, "lstm_rl", _self_row(st, e), _hum(st, e)[want_order], table, "holonomic")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
        if best[e] >= 0:
            assert best[e] == int(np.argmax(values[e]))
            top2 = np.sort(ref)[-2:]
            if top2[1] - top2[0] > 2 * TOL:
                assert best[e] == int(np.argmax(ref))
    for e in sample[:12]:
        me = FullState(*_self_row(st, e))
        js = JointState(me, [ObservableState(*row) for row in _hum(st, e).tolist()])
        pol.last_state = None
        pol.set_phase("train"); pol.set_epsilon(0.0)
        pol.predict(js)
        pol.set_phase("test")
        if not _reached(st, e):
            assert np.array_equal(np.array(pol.action_values), values[e]), e            # same bits
            assert torch.equal(pol.last_state.cpu(), rows[e]), e


def test_hcount_masks_humans_out_of_the_lstm():
    import torch
    rng = np.random.RandomState(7)
    E, N = 300, 6
    pol = _policy(seed=5)
    env = H.make_vec_env(E, N)
    st = _tie_state(rng, E, N)
    H.upload(env, st)
    hc = torch.from_numpy(rng.randint(1, N + 1, E).astype(np.int32)).cuda()
    actions, best, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values, order, hcn = values.cpu().numpy().copy(), pol.last_order.cpu().numpy().copy(), hc.cpu().numpy()
    assert np.array_equal(pol.human_order(env, hc).cpu().numpy(), order)
    model = _cpu_model(pol)
    for e in range(0, E, 7):
        n = int(hcn[e])
        hum = _hum(st, e)[:n]
        want = R.stable_desc_order(_self_row(st, e), _hum(st, e), n)
        assert order[e].tolist() == want.tolist()
        ref = R.policy_values(model, "lstm_rl", _self_row(st, e), hum[want[:n]], pol._action_table, "holonomic")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_unicycle_batch():
    import torch
    rng = np.random.RandomState(12)
    E, N = 200, 5
    pol = _policy(seed=8, kinematics="unicycle")
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = _tie_state(rng, E, N)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)
    H.upload(env, st)
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    model = _cpu_model(pol)
    for e in range(0, E, 9):
        want = R.stable_desc_order(_self_row(st, e), _hum(st, e))
        ref = R.policy_values(model, "lstm_rl", _self_row(st, e), _hum(st, e)[want], pol._action_table, "unicycle")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_query_env_takes_the_envs_order():
    """query_env = true: next states from the env's one-step look-ahead, in the env's order (multi_human_rl.py:37-38)."""
    import torch
    rng = np.random.RandomState(31)
    E, N = 64, 5
    pol = _policy(seed=9)
    pol.query_env = True
    env = H.make_vec_env(E, N)
    st = _tie_state(rng, E, N)
    H.upload(env, st)
    pol.build_action_space(1.0)
    pol._bufs = {}
    npos, nvel, rew = pol._query_env(env)
    npos, nvel, rew = npos.cpu().numpy(), nvel.cpu().numpy(), rew.cpu().numpy()
    _, _, values = pol.predict_batch(env, want_values=True)
    values, order = values.cpu().numpy(), pol.last_order.cpu().numpy()
    model = _cpu_model(pol)
    for e in range(0, E, 5):
        assert order[e].tolist() == list(range(N))
        nexts = np.concatenate([npos[e], nvel[e]], 1)
        ref = R.policy_values(model, "lstm_rl", _self_row(st, e), _hum(st, e), pol._action_table, "holonomic",
                              nexts=nexts, rewards=rew[e])
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_epsilon_greedy_rate_and_rows():
    import torch
    rng = np.random.RandomState(4)
    E, N = 4096, 5
    pol = _policy(seed=2, phase="train")
    pol.set_epsilon(0.5)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N)
    H.upload(env, st)
    torch.manual_seed(0)
    actions, best = pol.predict_batch(env)
    best, actions = best.cpu().numpy(), actions.cpu().numpy()
    live = best != -1
    rate = float((best[live] == -2).mean())
    sd = np.sqrt(0.25 / live.sum())
    assert abs(rate - 0.5) < 5 * sd
    table = pol._action_table
    for e in np.nonzero(best == -2)[0]:
        assert (np.abs(table - actions[e]).sum(1) == 0).any()


def test_explorer_batched_equals_sequential():
    """Explorer.run_k_episodes(64, 'test') with an LSTM-RL robot: batched (VecExplorer) and batched = False give the
    same success / collision / timeout rates and navigation time."""
    import torch
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.envs import CrowdSim
    from modelcrowdnav_amd.envs.utils.robot import Robot
    from modelcrowdnav_amd.utils.explorer import Explorer
    res = []
    for batched in (True, False):
        cfg = configs.env_config(**{"sim.human_num": 5})
        env = CrowdSim()
        env.configure(cfg)
        robot = Robot(cfg, "robot")
        robot.set_policy(_policy(seed=11))
        env.set_robot(robot)
        ex = Explorer(env, robot, torch.device("cuda", 0), gamma=0.9)
        ex.batched = batched
        res.append(ex.run_k_episodes(64, "test", returnNav=True))
        assert ex.last_run_batched == batched
    a, b = res
    assert tuple(a[1:4]) == tuple(b[1:4]), (a, b)
    assert abs(a[4] - b[4]) < 1e-9 and abs(a[0] - b[0]) < 1e-9, (a, b)


def test_trainer_step_changes_weights_and_next_predict_uses_them():
    import torch
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    rng = np.random.RandomState(17)
    E, N = 128, 5
    pol = _policy(seed=21)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N)
    H.upload(env, st)
    mem = ReplayMemory(1000, device=torch.device("cuda", 0))
    rows = pol.transform_batch(env)
    for e in range(E):
        mem.push((rows[e], torch.tensor([rng.uniform(-1, 1)], dtype=torch.float32, device=rows.device)))
    before = {k: v.clone() for k, v in pol.model.state_dict().items()}
    _, _, v0 = pol.predict_batch(env, want_values=True)
    v0 = v0.cpu().numpy().copy()
    tr = Trainer(pol.model, mem, torch.device("cuda", 0), batch_size=32)
    tr.set_learning_rate(0.01)
    tr.optimize_batch(4)
    assert any(not torch.equal(before[k], v) for k, v in pol.model.state_dict().items())
    _, _, v1 = pol.predict_batch(env, want_values=True)
    v1 = v1.cpu().numpy()
    assert not np.array_equal(v0, v1)
    model = _cpu_model(pol)
    for e in range(0, E, 16):
        want = R.stable_desc_order(_self_row(st, e), _hum(st, e))
        ref = R.policy_values(model, "lstm_rl", _self_row(st, e), _hum(st, e)[want], pol._action_table, "holonomic")
        np.testing.assert_allclose(v1[e], ref, rtol=0, atol=TOL)
