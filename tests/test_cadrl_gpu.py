"""GPU: the CADRL look-ahead (lstm_rl_value.hip through mcn_cadrl_predict) against the reference's own CADRL.predict
(g23_cadrl.npz) and against a torch-float32 evaluation of the same module.

Bar: 1e-5 absolute on values; the chosen action must be identical wherever the top-2 gap exceeds it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests import policy_ref as R  # noqa: E402
from tests.lookahead_harness import TOL, cpu_model, humans, reached, self_row  # noqa: E402


@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_predict_matches_reference_fixture(kin, golden_dir):
    g = np.load(os.path.join(golden_dir, "g23_cadrl.npz"))
    L.check_fixture_predictions("cadrl", g, (1, 5), "pred{seed}_{kin}_N{N}_", kin)


def test_train_phase_epsilon_and_last_state_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "g23_cadrl.npz"))
    L.check_epsilon_fixture("cadrl", g, int(g["eps_seed"]), 2200 + int(g["eps_seed"]), reset_values=False)


@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size(N):
    rng = np.random.RandomState(230 + N)
    E = 4096
    pol = L.policy("cadrl", seed=3)
    st = H.random_state(rng, E, N, randomize=True)
    out = L.run_predict_batch(pol, st)
    model, table = cpu_model(pol), pol._action_table
    sample = L.sample_envs(rng, E, 60, always=(1, 15, 16, 17, 2047, 2048, E - 2))
    for e in sample:
        ref = R.policy_values(model, "cadrl", self_row(st, e), humans(st, e), table, "holonomic")
        L.check_choice(out.values[e], out.best[e], out.actions[e], ref, table, reached(st, e), what=e)
    for e in sample[:8]:                       # the E = 1 path: same bits
        pol.predict(L.joint_state(self_row(st, e), humans(st, e)))
        if not reached(st, e):
            assert np.array_equal(np.array(pol.action_values), out.values[e]), e


def test_hcount_masks_humans_out_of_the_min():
    import torch
    rng = np.random.RandomState(8)
    E, N = 300, 6
    pol = L.policy("cadrl", seed=5)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, crowded_frac=0.6)
    H.upload(env, st)
    hc = torch.from_numpy(rng.randint(1, N + 1, E).astype(np.int32)).cuda()
    _, _, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values, hcn = values.cpu().numpy(), hc.cpu().numpy()
    model = cpu_model(pol)
    for e in range(0, E, 7):
        ref = R.policy_values(model, "cadrl", self_row(st, e), humans(st, e)[:int(hcn[e])], pol._action_table,
                              "holonomic")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_one_nan_human_makes_the_pair_nan():
    """torch.min propagates NaN (cadrl.py:164): one visible human with a NaN output makes every value of its env NaN;
    a NaN human beyond hcount does not."""
    import torch
    rng = np.random.RandomState(9)
    E, N = 40, 5
    pol = L.policy("cadrl", seed=6)
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
    pol = L.policy("cadrl", seed=8, kinematics="unicycle")
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = H.random_state(rng, E, N, randomize=True)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E)
    H.upload(env, st)
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy().copy()
    model = cpu_model(pol)
    for e in range(0, E, 5):
        ref = R.policy_values(model, "cadrl", self_row(st, e), humans(st, e), pol._action_table, "unicycle")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
    pol.query_env = True
    npos, nvel, rew = pol._query_env(env)
    npos, nvel, rew = npos.cpu().numpy(), nvel.cpu().numpy(), rew.cpu().numpy()
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    for e in range(0, E, 5):
        ref = R.policy_values(model, "cadrl", self_row(st, e), humans(st, e), pol._action_table, "unicycle",
                              nexts=np.concatenate([npos[e], nvel[e]], 1), rewards=rew[e])
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


def test_epsilon_greedy_rate_and_rows():
    pol, env = L.check_epsilon_rate("cadrl", N=1)
    rows = pol.transform_batch(env).cpu()
    assert rows.shape == (4096, 13)
