"""GPU: the LSTM-RL look-ahead (lstm_rl_value.hip through mcn_lstm_rl_predict) against the reference's own
LstmRL.predict (g22_lstm_rl.npz) and against a torch-float32 evaluation of the same module on rows sorted in the test.

Bar: 1e-5 absolute on values (BASELINE.json north_star); the chosen action must be identical wherever the top-2 gap
exceeds it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests import policy_ref as R  # noqa: E402
from tests.lookahead_harness import TOL, cpu_model, humans, reached, self_row  # noqa: E402
from tests.lookahead_states import tie_state_quarter_grid as _tie_state  # noqa: E402


def _reference(model, pol, st, e, kinematics="holonomic"):
    """(torch float32 values on the humans in numpy's stable descending order, that order)."""
    want = R.stable_desc_order(self_row(st, e), humans(st, e))
    return R.policy_values(model, "lstm_rl", self_row(st, e), humans(st, e)[want], pol._action_table, kinematics), want


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_predict_matches_reference_fixture(kin, golden_dir):
    """LstmRL.predict(JointState): action_values, chosen action and the host-sorted human list of the reference."""
    g = np.load(os.path.join(golden_dir, "g22_lstm_rl.npz"))
    L.check_fixture_predictions("lstm_rl", g, (5, 10), "pred{seed}_{kin}_N{N}_", kin, check_sorted=True)


def test_train_phase_epsilon_and_last_state_match_reference(golden_dir):
    """epsilon 0.5 on numpy's global stream (multi_human_rl.py:27-29) and last_state = transform(sorted state)."""
    g = np.load(os.path.join(golden_dir, "g22_lstm_rl.npz"))
    L.check_epsilon_fixture("lstm_rl", g, int(g["eps_seed"]), 2200 + int(g["eps_seed"]), reset_values=True)


@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size(N):
    """4096 envs x 81 actions: every value of >= 64 sampled envs (0, 15, 16, E-1 among them) against torch on rows
    sorted here; the device order against numpy's stable descending sort (tie envs included); transform_batch rows
    against the E = 1 transform of the sorted state; the E = 1 path gives the same bits for the same env."""
    import torch
    rng = np.random.RandomState(220 + N)
    E = 4096
    pol = L.policy("lstm_rl", seed=3)
    st = _tie_state(rng, E, N)
    out = L.run_predict_batch(pol, st)
    rows = pol.transform_batch(out.env).cpu()
    model, table = cpu_model(pol), pol._action_table
    sample = L.sample_envs(rng, E, 60, always=(1, 3, 15, 16, 17, 2047, 2048, E - 2))
    for e in sample:
        ref, want_order = _reference(model, pol, st, e)
        assert out.order[e].tolist() == want_order.tolist(), e
        L.check_choice(out.values[e], out.best[e], out.actions[e], ref, table, reached(st, e), what=e)
    for e in sample[:12]:
        pol.last_state = None
        pol.set_phase("train"); pol.set_epsilon(0.0)
        pol.predict(L.joint_state(self_row(st, e), humans(st, e)))
        pol.set_phase("test")
        if not reached(st, e):
            assert np.array_equal(np.array(pol.action_values), out.values[e]), e            # same bits
            assert torch.equal(pol.last_state.cpu(), rows[e]), e


def test_hcount_masks_humans_out_of_the_lstm():
    rng = np.random.RandomState(7)
    E, N = 300, 6
    pol = L.policy("lstm_rl", seed=5)
    st = _tie_state(rng, E, N)
    hcn = rng.randint(1, N + 1, E).astype(np.int32)
    out = L.run_predict_batch(pol, st, hcount=hcn)
    model = cpu_model(pol)
    for e in range(0, E, 7):
        n = int(hcn[e])
        hum = humans(st, e)[:n]
        want = R.stable_desc_order(self_row(st, e), humans(st, e), n)
        assert out.order[e].tolist() == want.tolist()
        ref = R.policy_values(model, "lstm_rl", self_row(st, e), hum[want[:n]], pol._action_table, "holonomic")
        np.testing.assert_allclose(out.values[e], ref, rtol=0, atol=TOL)


def test_unicycle_batch():
    rng = np.random.RandomState(12)
    E, N = 200, 5
    pol = L.policy("lstm_rl", seed=8, kinematics="unicycle")
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = _tie_state(rng, E, N)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)
    H.upload(env, st)
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    model = cpu_model(pol)
    for e in range(0, E, 9):
        np.testing.assert_allclose(values[e], _reference(model, pol, st, e, "unicycle")[0], rtol=0, atol=TOL)


def test_query_env_takes_the_envs_order():
    """query_env = true: next states from the env's one-step look-ahead, in the env's order (multi_human_rl.py:37-38)."""
    rng = np.random.RandomState(31)
    E, N = 64, 5
    pol = L.policy("lstm_rl", seed=9)
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
    model = cpu_model(pol)
    for e in range(0, E, 5):
        assert order[e].tolist() == list(range(N))
        nexts = np.concatenate([npos[e], nvel[e]], 1)
        ref = R.policy_values(model, "lstm_rl", self_row(st, e), humans(st, e), pol._action_table, "holonomic",
                              nexts=nexts, rewards=rew[e])
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_epsilon_greedy_rate_and_rows():
    L.check_epsilon_rate("lstm_rl", N=5)


def test_explorer_batched_equals_sequential():
    """Explorer.run_k_episodes(64, 'test') with an LSTM-RL robot: batched (VecExplorer) and batched = False give the
    same success / collision / timeout rates and navigation time."""
    L.check_explorer_batched_equals_sequential("lstm_rl")


def test_trainer_step_changes_weights_and_next_predict_uses_them():
    def reference(pol):
        model = cpu_model(pol)
        return lambda st, e: _reference(model, pol, st, e)[0]
    L.check_trainer_step_is_seen("lstm_rl", reference)
