"""GPU: the LSTM-RL / CADRL look-ahead (lstm_rl_value.hip) away from the shipped shape and at its edges.

  * every lookahead_kernel variant (MAXN 8 / 16 / 32, N = 1 .. 32 across the boundaries), unicycle, action tables of
    2, 25 and 85 rows, ragged E x A, E x A < 16 and more groups than the persistent grid, against torch float32;
  * the network error against a float64 evaluation of the same module on the same float32 features, for the default
    initialisation and for saturating gates with a growing cell state;
  * the human order (mcn_lstm_rl_order and the look-ahead's order output) on exact ties, sub-ulp near-ties, +inf, NaN
    and masked-out non-finite humans (tests/lookahead_states.py) against policy_ref.stable_desc_order;
  * features at dg == 0, a human on the robot's next position, still humans; hcount masks and clamps.

Bar: 1e-5 absolute on values (BASELINE.json north_star), as tests/test_lstm_rl_gpu.py and tests/test_cadrl_gpu.py."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cport  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests import lookahead_states as LS  # noqa: E402
from tests import policy_ref as R  # noqa: E402
from tests.lookahead_harness import TOL, cpu_model, humans, reached, self_row  # noqa: E402
from tests.lookahead_states import tie_state_eighth_grid as _tie_state  # noqa: E402

BODIES = ("lstm_rl", "cadrl")
SHAPE_NS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32)


def _run(pol, st, kinematics="holonomic", hcount=None):
    """predict_batch on st (hcount: numpy int32 [E] or None) -> numpy (actions, best, values, order or None), env."""
    out = L.run_predict_batch(pol, st, kinematics, hcount)
    return [out.actions, out.best, out.values, out.order], out.env


def _check_env(body, model, pol, st, e, out, kinematics="holonomic", count=None):
    """values, best, the action (and order) of env e of out = (actions, best, values, order) against torch float32 on
    the first `count` humans, sorted for LSTM-RL."""
    actions, best, values, order = out
    n = st.N if count is None else int(count)
    hum = humans(st, e)
    if body == "lstm_rl":
        want = R.stable_desc_order(self_row(st, e), hum, n)
        assert order[e].tolist() == want.tolist(), (e, order[e], want)
        hum = hum[want[:n]]
    else:
        hum = hum[:n]
    ref = R.policy_values(model, body, self_row(st, e), hum, pol._action_table, kinematics)
    L.check_choice(values[e], best[e], actions[e], ref, pol._action_table, reached(st, e), what="env %d" % e)
    return ref


def _sample(rng, E, k=8):
    return L.sample_envs(rng, E, k)


# ------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("N", SHAPE_NS)
@pytest.mark.parametrize("body", BODIES)
def test_human_counts_across_the_kernel_variants(body, N):
    """lookahead_kernel<LSTM, 8 / 16 / 32> and mcn_lstm_rl_order<8 / 16 / 32> on both sides of every boundary; E = 37
    makes E x 81 = 2997 pairs, not a multiple of 16."""
    rng = np.random.RandomState(400 + N)
    E = 37
    pol = L.policy(body, seed=N)
    st = _tie_state(rng, E, N)
    out, _ = _run(pol, st)
    actions, best, values, order = out
    assert values.shape == (E, 81)
    model = cpu_model(pol)
    for e in _sample(rng, E):
        _check_env(body, model, pol, st, e, out)
    if body == "lstm_rl":                   # every env's order, not only the sampled ones
        for e in range(E):
            assert order[e].tolist() == R.stable_desc_order(self_row(st, e), humans(st, e)).tolist(), e


@pytest.mark.parametrize("N", [1, 9, 32])
@pytest.mark.parametrize("body", BODIES)
def test_unicycle_human_counts(body, N):
    rng = np.random.RandomState(500 + N)
    E = 21
    pol = L.policy(body, seed=40 + N, kinematics="unicycle")
    st = _tie_state(rng, E, N, "unicycle")
    out, _ = _run(pol, st, "unicycle")
    model = cpu_model(pol)
    for e in _sample(rng, E, 6):
        _check_env(body, model, pol, st, e, out, "unicycle")


@pytest.mark.parametrize("speeds,rotations,E", [(1, 1, 21), (1, 1, 1), (3, 8, 21), (7, 12, 21), (3, 8, 1333)])
@pytest.mark.parametrize("body", BODIES)
def test_other_action_tables_and_batch_sizes(body, speeds, rotations, E):
    """A = 2, 25, 85 ((env, action) pairs are tiled 16 at a time whatever A is): E x A = 42, 2, 525, 1785 -- none a
    multiple of 16, one below 16 -- and 1333 x 25 = 33325 pairs, 261 groups of 128: more than the 256-block persistent
    grid, so a workgroup takes a second group."""
    rng = np.random.RandomState(speeds * 100 + rotations + E)
    N = 5
    pol = L.with_action_grid(L.policy(body, seed=6), speeds, rotations)
    st = _tie_state(rng, E, N)
    out, _ = _run(pol, st)
    actions, best, values, order = out
    A = speeds * rotations + 1
    table = pol._action_table
    assert table.shape == (A, 2) and values.shape == (E, A)
    if E * A > 256 * 128:
        assert ((E * A + 15) // 16 + 7) // 8 > 256
    model = cpu_model(pol)
    sample = _sample(rng, E) + ([E - 2, E - 16, E - 17] if E > 32 else [])
    for e in sorted(set(sample)):
        _check_env(body, model, pol, st, e, out)


# ------------------------------------------------------------------------------------------------- float64
def _saturate(pol, body):
    """Gate weights x4 and the forget-gate bias at +5 (LSTM-RL): pre-activations reach ~10 and c grows with every
    human; CADRL: the first layer x4."""
    import torch
    m = pol.model
    with torch.no_grad():
        if body == "lstm_rl":
            m.lstm.weight_ih_l0.mul_(4.0)
            m.lstm.weight_hh_l0.mul_(4.0)
            H_ = m.lstm_hidden_dim
            m.lstm.bias_ih_l0[H_:2 * H_] = 5.0
            m.lstm.bias_hh_l0[H_:2 * H_] = 0.0
        else:
            m.value_network[0].weight.mul_(4.0)


@pytest.mark.parametrize("weights", ["default", "saturating"])
@pytest.mark.parametrize("N", [5, 10, 32])
@pytest.mark.parametrize("body", BODIES)
def test_network_error_against_a_float64_evaluation(body, N, weights):
    """The policy's module in float64 on the same float32 rotated features is the yardstick; the kernel's error
    |(value - reward) / gamma^(dt v_pref) - V64| may not exceed twice torch float32's own error + 5e-7 (the bound of
    tests/test_sarl_gpu.py), and every value is within 1e-5 of torch float32.  Rewards: cport.lookahead_reward."""
    import torch
    rng = np.random.RandomState(600 + N)
    E = 48
    pol = L.policy(body, seed=70 + N)
    if weights == "saturating":
        _saturate(pol, body)
    st = H.random_state(rng, E, N, randomize=True)
    (actions, best, values, order), _ = _run(pol, st)
    m32 = cpu_model(pol)
    m64 = copy.deepcopy(m32).double()
    table = pol._action_table
    rew = cport.lookahead_reward(st, table, 0.25)
    gpow = pow(pol.gamma, 0.25 * 1.0)
    err_k = err_t = 0.0
    cmax = 0.0
    for e in range(0, E, 3):
        hum = humans(st, e)
        if body == "lstm_rl":
            hum = hum[R.stable_desc_order(self_row(st, e), hum)]
        xr, _ = R.rotated_rows(self_row(st, e), hum, table, "holonomic")
        truth = R.network_value(m64, body, xr.double()).numpy()
        v32 = R.network_value(m32, body, xr).double().numpy()
        if body == "lstm_rl":
            with torch.no_grad():
                cmax = max(cmax, float(m64.lstm(xr.double())[1][1].abs().max()))
        np.testing.assert_allclose(values[e], rew[e] + gpow * v32, rtol=0, atol=TOL, err_msg="env %d" % e)
        err_k = max(err_k, float(np.abs((values[e] - rew[e]) / gpow - truth).max()))
        err_t = max(err_t, float(np.abs(v32 - truth).max()))
    print("%s N=%d %s weights: error vs float64: kernel %.2e, torch float32 %.2e%s"
          % (body, N, weights, err_k, err_t, (", max |c| %.1f" % cmax) if body == "lstm_rl" else ""))
    assert err_t > 0
    if body == "lstm_rl" and weights == "saturating" and N == 32:
        assert cmax > 10, cmax              # the cell state did grow
    assert err_k <= 2 * err_t + 5e-7, (err_k, err_t)


# ------------------------------------------------------------------------------------------------- order
@pytest.mark.parametrize("N", [5, 9, 32])
def test_human_order_edges(N):
    """mcn_lstm_rl_order and the look-ahead's order output on order_batch (ties, near-ties the un-fused norm orders
    differently, +inf, NaN at slot 0 / middle / end, all NaN, a NaN robot, non-finite humans beyond hcount): equal to
    stable_desc_order -- first strict maximum, ties in index order, NaN last in index order, slots >= hcount kept."""
    rng = np.random.RandomState(700 + N)
    st, hc, names = LS.order_batch(N)
    assert len(LS.fused_unfused_disagreements(st)) > 0
    pol = L.policy("lstm_rl", seed=12)
    out, _ = _run(pol, st, hcount=hc)
    actions, best, values, order = out
    bad = []
    for e in range(st.E):
        want = R.stable_desc_order(self_row(st, e), humans(st, e), int(hc[e]))
        if order[e].tolist() != want.tolist():
            bad.append((names[e], e, order[e].tolist(), want.tolist()))
    assert not bad, bad[:4]
    # values where every visible human is finite: against torch
    model = cpu_model(pol)
    fin = [e for e in range(st.E) if np.isfinite(humans(st, e)[:hc[e], :2]).all() and np.isfinite(st.rpx[e] + st.rpy[e])]
    for e in [fin[i] for i in sorted(set(rng.choice(len(fin), 8, replace=False)))]:
        _check_env("lstm_rl", model, pol, st, e, out, count=hc[e])


# ------------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
@pytest.mark.parametrize("body", BODIES)
def test_feature_edges(body, kinematics):
    """dg == 0 after the chosen action (cr = 1, sr = 0; unicycle: f_theta = nth - atan2(0, 0)), a propagated human on
    the robot's next position (feature 11 through sqrt_f32's guard), still humans: every value against torch."""
    N = 5
    pol = L.policy(body, seed=81, kinematics=kinematics)
    pol.build_action_space(1.0)
    st, names, act = LS.feature_batch(N, pol._action_table, kinematics)
    out, _ = _run(pol, st, kinematics)
    model = cpu_model(pol)
    for e in range(st.E):
        _check_env(body, model, pol, st, e, out, kinematics)
        xr, rew = R.rotated_rows(self_row(st, e), humans(st, e), pol._action_table, kinematics)
        a = int(act[e])
        if names[e] == "on-goal":                # the edge is reached: dg == 0 for the chosen action
            assert (xr[a, :, 0] == 0).all(), e
            assert reached(st, e) == (a == 0), e
        elif names[e].startswith("human-on-next"):
            assert (xr[a, :, 11] == 0).any() and rew[a] == -0.25, e
        elif names[e] == "still-humans":
            assert (xr[:, :, 8:10] == 0).all(), e


# ------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("body", BODIES)
def test_nonfinite_humans_beyond_hcount_stay_out(body):
    rng = np.random.RandomState(90)
    E, N = 40, 7
    pol = L.policy(body, seed=13)
    base = _tie_state(rng, E, N)
    hc = rng.randint(1, N, E).astype(np.int32)
    st = LS.nonfinite_beyond(base, hc)
    assert not np.isfinite(st.hpx).all()
    out, _ = _run(pol, st, hcount=hc)
    actions, best, values, order = out
    assert np.isfinite(values).all()
    (_, _, clean, clean_order), _ = _run(pol, base, hcount=hc)
    assert np.array_equal(values, clean)
    if order is not None:
        assert np.array_equal(order, clean_order)
    model = cpu_model(pol)
    for e in _sample(rng, E):
        _check_env(body, model, pol, st, e, out, count=hc[e])


@pytest.mark.parametrize("body", BODIES)
def test_hcount_is_clamped_to_one_and_n(body):
    """hcount 0 (and negative) behaves as 1, hcount N + 3 as N -- bit for bit, order included."""
    rng = np.random.RandomState(91)
    E, N = 24, 6
    pol = L.policy(body, seed=14)
    st = _tie_state(rng, E, N)
    run = lambda hc: _run(pol, st, hcount=np.asarray(hc, np.int32))[0]
    lo = run(np.where(np.arange(E) % 2, 0, -5))
    one = run(np.ones(E))
    hi = run(np.full(E, N + 3))
    full = _run(pol, st)[0]
    for a, b in ((lo, one), (hi, full)):
        assert H.bits_equal(a[2], b[2]) and np.array_equal(a[1], b[1])
        if a[3] is not None:
            assert np.array_equal(a[3], b[3])
    model = cpu_model(pol)
    for e in _sample(rng, E, 4):
        _check_env(body, model, pol, st, e, lo, count=1)
    if lo[3] is not None:
        assert (lo[3] == np.arange(N)).all()


@pytest.mark.parametrize("body", BODIES)
def test_hcount_at_thirty_two_humans(body):
    rng = np.random.RandomState(92)
    E, N = 40, 32
    pol = L.policy(body, seed=15)
    st = _tie_state(rng, E, N)
    hc = rng.randint(1, N + 1, E).astype(np.int32)
    hc[:4] = (1, 31, 32, 17)
    out, _ = _run(pol, st, hcount=hc)
    order = out[3]
    model = cpu_model(pol)
    if order is not None:
        for e in range(E):
            assert order[e].tolist() == R.stable_desc_order(self_row(st, e), humans(st, e), int(hc[e])).tolist(), e
    for e in sorted(set([0, 1, 2, 3] + _sample(rng, E, 6))):
        _check_env(body, model, pol, st, e, out, count=hc[e])
