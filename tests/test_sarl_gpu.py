"""GPU parity of the fused SARL look-ahead (mcn_sarl_lookahead through the C ABI).

Tolerance: the network is float32 in the reference (torch CPU); the kernel evaluates it with
float32 MFMA (exact fmaf chains) in a different summation order, so values agree to ~1e-6.
The test bar is 1e-5 (BASELINE.json north_star) on values; the chosen action must be identical
whenever the top-2 gap exceeds that tolerance."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyref  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests.lookahead_harness import TOL, cpu_weights, humans, reached, self_row  # noqa: E402


def test_predict_matches_reference_fixture(golden_dir):
    """SARL.predict(JointState) against action_values / chosen action recorded from the real reference."""
    g = np.load(os.path.join(golden_dir, "g5_sarl.npz"))
    L.check_fixture_predictions("sarl", g, (5, 10), "pred{seed}_N{N}_")


@pytest.mark.parametrize("N", [5, 10, 1, 3])
def test_predict_batch_matches_oracle(N):
    """predict_batch over a VecCrowdSim against the torch-fp32 restatement, env by env."""
    rng = np.random.RandomState(N)
    E = 37          # ragged vs the 16-pair wave tile
    pol = L.policy("sarl", seed=3)
    st = H.random_state(rng, E, N, randomize=True)
    st.rgx[0], st.rgy[0] = st.rpx[0] + 0.05, st.rpy[0] - 0.05        # env 0: robot already at its goal
    out = L.run_predict_batch(pol, st)
    w, table = cpu_weights(pol), pol._action_table
    assert out.best[0] == -1 and tuple(out.actions[0]) == (0.0, 0.0)
    for e in range(1, E, 3):
        ref, idx = pyref.sarl_predict(w, self_row(st, e), humans(st, e), table)
        # (a robot on its goal: policy.py:43-49 short cut, zero action)
        L.check_choice(out.values[e], out.best[e], out.actions[e], ref, table, reached(st, e), what=e)


@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size_matches_oracle(N):
    """The grids bench.py times (BASELINE configs 3 / 4: 4096 envs x 81 actions = 20 736 16-pair tiles, ten rounds
    of the resident workgroups): 64 sampled envs -- first, last, the tile-straddling ones and a random spread --
    against the torch-fp32 restatement (multi_human_rl.py:35-63, sarl.py:28-65)."""
    rng = np.random.RandomState(40 + N)
    E = 4096
    pol = L.policy("sarl", seed=3)
    st = H.random_state(rng, E, N, randomize=True)
    out = L.run_predict_batch(pol, st)
    values, best, actions = out.values, out.best, out.actions
    assert values.shape == (E, 81) and np.isfinite(values).all()
    w, table = cpu_weights(pol), pol._action_table
    sample = L.sample_envs(rng, E, 56, always=(1, 15, 16, 2047, 2048, E - 2))
    worst = 0.0
    for e in sample:
        ref, idx = pyref.sarl_predict(w, self_row(st, e), humans(st, e), table)
        L.check_choice(values[e], best[e], actions[e], ref, table, reached(st, e), what="env %d" % e)
        if not reached(st, e):
            worst = max(worst, float(np.abs(values[e] - ref).max()))
    # every env's action is the table row of its own argmax (the whole batch, not only the sample)
    moving = best >= 0
    assert np.array_equal(best[moving], np.argmax(values[moving], 1))
    assert np.array_equal(actions[moving], table[best[moving]])
    print("SARL 4096 x %d: max |value - reference| over %d sampled envs = %.3g" % (N, len(sample), worst))


def test_epsilon_greedy_in_train_phase():
    """multi_human_rl.py:27-29 per env: phase 'train' with epsilon = 1 replaces every choice by a uniformly drawn
    table action (except robots already on their goal, which return before the draw), epsilon = 0 is the greedy
    choice, and test phase ignores epsilon.  VecExplorer's training rollouts go through the same call."""
    import torch
    rng = np.random.RandomState(12)
    E, N = 2048, 5
    pol = L.policy("sarl", seed=3)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N)
    st.rgx[0], st.rgy[0] = st.rpx[0] + 0.05, st.rpy[0] - 0.05        # env 0: robot already at its goal
    H.upload(env, st)
    greedy_a, greedy_b = (x.clone() for x in pol.predict_batch(env))     # the outputs are the policy's own buffers
    pol.set_epsilon(1.0)
    a_test, b_test = pol.predict_batch(env)                          # phase 'test': epsilon is not looked at
    assert torch.equal(b_test, greedy_b) and torch.equal(a_test, greedy_a)
    pol.set_phase("train")
    torch.manual_seed(5)
    a1, b1 = (x.clone() for x in pol.predict_batch(env))
    assert int(b1[0]) == -1 and tuple(a1[0].tolist()) == (0.0, 0.0)
    moving = greedy_b >= 0
    assert bool((b1[moving] == -2).all())
    table = pol._bufs["table"]
    # every explored action is a table row, and the draw is spread over the table
    match = (a1[moving].unsqueeze(1) == table.unsqueeze(0)).all(2)
    assert bool(match.any(1).all())
    counts = match.float().sum(0)
    assert int((counts > 0).sum()) >= 75 and float(counts.max()) < 0.05 * float(moving.sum())
    assert float((a1[moving] != greedy_a[moving]).any(1).float().mean()) > 0.9
    pol.set_epsilon(0.25)
    a2, b2 = (x.clone() for x in pol.predict_batch(env))
    frac = float((b2[moving] == -2).float().mean())
    assert 0.2 < frac < 0.3
    keep = moving & (b2 != -2)
    assert torch.equal(a2[keep], greedy_a[keep]) and torch.equal(b2[keep], greedy_b[keep])
    pol.set_epsilon(0.0)
    a3, b3 = pol.predict_batch(env)
    assert torch.equal(b3, greedy_b) and torch.equal(a3, greedy_a)
    # reproducible under torch.manual_seed, different from call to call
    pol.set_epsilon(0.5)
    torch.manual_seed(9)
    x1 = pol.predict_batch(env)[0].clone()
    x2 = pol.predict_batch(env)[0].clone()
    torch.manual_seed(9)
    y1 = pol.predict_batch(env)[0].clone()
    assert torch.equal(x1, y1) and not torch.equal(x1, x2)


def test_rewards_are_float64_exact():
    """With a network whose V is exactly 0, values are exactly MultiHumanRL.compute_reward (float64).  Every parameter
    is zero except attention.4.bias = 1: uniform attention weights, mlp2 and mlp3 zero.  (All zero would make every score
    exactly 0, which the masked softmax of sarl.py:52-53 turns into 0 / 0 = NaN, in the reference and in the kernel.)"""
    import torch
    from oracle import cport
    rng = np.random.RandomState(9)
    E, N = 200, 5
    pol = L.zeroed(L.policy("sarl", seed=0), "sarl")
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, crowded_frac=0.6)
    H.upload(env, st)
    _, _, values = pol.predict_batch(env, want_values=True)
    ref = cport.lookahead_reward(st, pol._action_table, 0.25)
    assert np.array_equal(values.cpu().numpy(), ref)


@pytest.mark.parametrize("speeds,rotations", [(3, 8), (7, 12), (1, 1)])
def test_other_action_space_sizes(speeds, rotations):
    """policy.config [action_space] speed_samples / rotation_samples (cadrl.py:82-102): the table has
    speeds * rotations + 1 rows -- 25, 85 and 2 here instead of the shipped 81 -- and the kernels take A as an argument
    ((env, action) pairs are tiled 16 at a time whatever A is)."""
    import torch
    rng = np.random.RandomState(speeds * 100 + rotations)
    E, N = 21, 5
    pol = L.with_action_grid(L.policy("sarl", seed=6), speeds, rotations)
    st = H.random_state(rng, E, N, randomize=True)
    out = L.run_predict_batch(pol, st)
    table = pol._action_table
    A = speeds * rotations + 1
    assert table.shape == (A, 2) and out.values.shape == (E, A)
    w = cpu_weights(pol)
    for e in range(0, E, 3):
        ref, idx = pyref.sarl_predict(w, self_row(st, e), humans(st, e), table)
        L.check_choice(out.values[e], out.best[e], out.actions[e], ref, table, reached(st, e), what=e)
        if A == 2 and not reached(st, e):          # two rows: the reference's choice whatever the gap
            assert out.best[e] == idx and tuple(out.actions[e]) == tuple(table[idx])


def test_unicycle_lookahead_matches_oracle():
    """(v, r) action table, heading-dependent propagate and the theta feature (cadrl.py:97-99,118-124,236-237)."""
    import torch
    rng = np.random.RandomState(21)
    E, N = 24, 5
    pol = L.policy("sarl", seed=5, kinematics="unicycle")
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = H.random_state(rng, E, N)
    st.rtheta[:] = rng.uniform(-3, 3, E)
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    table = pol._action_table
    assert table.shape == (81, 2) and table[1, 1] == -np.pi / 4          # (speed, rotation) rows
    w = cpu_weights(pol)
    for e in range(0, E, 4):
        ref, idx = pyref.sarl_predict(w, self_row(st, e), humans(st, e), table, kinematics="unicycle")
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)


@pytest.mark.parametrize("N", [5, 10, 2])
def test_unicycle_predict_matches_reference_fixture(N, golden_dir):
    """g17_sarl_unicycle.npz = the REAL reference's predict with a unicycle robot: the 40 recorded states go through
    one predict_batch (mcn_sarl_predict, kinematics 1) -- 81 action values to the path's tolerance, the reference's
    (v, r) action wherever its top two values are further apart than that, (0, 0) where the robot stands on its goal."""
    import torch
    g = np.load(os.path.join(golden_dir, "g17_sarl_unicycle.npz"))
    pol = L.policy("sarl", L.weights(g, "w__"), kinematics="unicycle")
    me, hum = g["N%d_self" % N], g["N%d_humans" % N]
    E = me.shape[0]
    env = H.make_vec_env(E, N, kinematics="unicycle")
    st = H.random_state(np.random.RandomState(0), E, N)
    st.rpx[:], st.rpy[:], st.rvx[:], st.rvy[:], st.rr[:] = me[:, 0], me[:, 1], me[:, 2], me[:, 3], me[:, 4]
    st.rgx[:], st.rgy[:], st.rtheta[:] = me[:, 5], me[:, 6], me[:, 8]
    st.hpx[:], st.hpy[:], st.hvx[:], st.hvy[:], st.hr[:] = (hum[:, :, c] for c in range(5))
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    values, best, actions = values.cpu().numpy(), best.cpu().numpy(), actions.cpu().numpy()
    assert np.array_equal(pol._action_table, g["table"])
    checked = 0
    for e in range(E):
        want = g["N%d_values" % N][e]
        if np.isnan(want[0]):                 # the reference returned early: the robot stands on its goal
            assert reached(st, e)
            L.check_choice(values[e], best[e], actions[e], None, g["table"], True, what=e)
            continue
        L.check_choice(values[e], best[e], actions[e], want, g["table"], reached(st, e), what=e)
        top2 = np.sort(want)[-2:]
        if top2[1] - top2[0] > 2 * TOL:
            assert tuple(actions[e]) == tuple(g["N%d_action" % N][e]), e
            checked += 1
    assert checked > 25
    # the E = 1 surface on the same states: get_attention_weights() is what the reference's model holds after predict()
    # -- the weights of the last candidate action (sarl.py:56,88-89), unchanged where predict() returned early
    prev = None
    for e in range(0, E, 2):
        act = pol.predict(L.joint_state(me[e], hum[e]))
        want = g["N%d_attention" % N][e]
        if np.isnan(g["N%d_values" % N][e][0]):
            assert tuple(act) == (0, 0)
            assert prev is None or np.array_equal(pol.get_attention_weights(), prev)          # stale, as in the reference
            continue
        prev = pol.get_attention_weights()
        np.testing.assert_allclose(prev, want, rtol=0, atol=TOL)
        assert pol.chosen_attention_weights.shape == (N,) and abs(pol.chosen_attention_weights.sum() - 1) < 1e-5


def test_e1_epsilon_greedy_follows_numpys_stream_like_the_reference(golden_dir):
    """g21_epsilon.npz = the REAL reference's predict in the train phase with epsilon 0.5 under np.random.seed(2100):
    one uniform draw per call decides exploration, np.random.choice picks the table row (multi_human_rl.py:26-29), no
    draw where the robot stands on its goal (:22-23), `last_state` = transform(state) kept in the train phase only
    (:60-61).  The E = 1 predict() consumes numpy's global stream the same way: same explored calls, same random
    rows, same greedy actions, same stored states."""
    g = np.load(os.path.join(golden_dir, "g21_epsilon.npz"))
    pol = L.policy("sarl", L.weights(np.load(os.path.join(golden_dir, "g17_sarl_unicycle.npz")), "w__"))
    pol.set_phase("train")
    with pytest.raises(AttributeError):
        pol.predict(L.joint_state(g["selfs"][0], g["humans"][0]))
    pol.set_epsilon(0.5)
    np.random.seed(2100)
    kinds = np.bincount(g["explored"], minlength=3)
    assert kinds.min() >= 5
    for s in range(g["selfs"].shape[0]):
        js = L.joint_state(g["selfs"][s], g["humans"][s])
        pol.action_values = None
        act = pol.predict(js)
        kind = int(g["explored"][s])
        assert (2 if pol.reach_destination(js) else int(pol.action_values is None)) == kind, s
        if kind == 0:                 # greedy: compare unless the device's float32 values tie differently
            vals = np.sort(np.array(pol.action_values))[-2:]
            if vals[1] - vals[0] > 2 * TOL:
                assert (act.vx, act.vy) == tuple(g["actions"][s]), s
        else:
            assert (act.vx, act.vy) == tuple(g["actions"][s]), s
        if s > 0 or kind != 2:
            np.testing.assert_allclose(pol.last_state.cpu().numpy(), g["last_states"][s], rtol=2e-6, atol=2e-6)
    pol.set_phase("test")
    pol.last_state = None
    pol.predict(L.joint_state(g["selfs"][0], g["humans"][0]))
    assert pol.last_state is None                       # only the train phase keeps it


def test_per_env_pedestrian_counts():
    """mcn_env_state.hcount: env e shows only its first hcount[e] pedestrians to the policy.  Values must equal
    the reference network evaluated on the shorter list (attention sum, mean and distance test all ignore the
    absent slots), whatever sits in those slots."""
    import torch
    rng = np.random.RandomState(17)
    E, N = 41, 7
    pol = L.policy("sarl", seed=4)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    H.upload(env, st)
    counts = rng.randint(1, N + 1, E).astype(np.int32)
    counts[0], counts[1] = N, 1
    hc = torch.from_numpy(counts).to(env.device)
    actions, best, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values, best = values.cpu().numpy().copy(), best.cpu().numpy().copy()
    full = pol.predict_batch(env, want_values=True)[2].cpu().numpy()
    assert np.array_equal(values[0], full[0])                         # hcount == N is the unmasked path
    w = cpu_weights(pol)
    table = pol._action_table
    for e in range(0, E, 2):
        ref, idx = pyref.sarl_predict(w, self_row(st, e), humans(st, e)[:int(counts[e])], table)
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
    # garbage in the absent slots must not leak in
    env.hpos[:, 3:] = 1e6; env.hvel[:, 3:] = -7.0
    hc3 = torch.full((E,), 3, dtype=torch.int32, device=env.device)
    v3 = pol.predict_batch(env, want_values=True, hcount=hc3)[2].cpu().numpy()
    ref = pyref.sarl_predict(w, self_row(st, 5), humans(st, 5)[:3], table)[0]
    np.testing.assert_allclose(v3[5], ref, rtol=0, atol=TOL)
    with pytest.raises(ValueError):
        pol.predict_batch(env, hcount=hc.long())


@pytest.mark.parametrize("N", [5, 10, 3])
def test_bf16x3_layers_agree_with_the_float32_mfma_layers(N):
    """The look-ahead's layers run on the bf16 matrix pipe with every float32 operand split into three bfloat16 pieces
    (mcn_sarl_net.x3, csrc/mfma_chain.hpp: dense_flow_x3); mcn_tuning.sarl_x3 = 0 keeps the float32 MFMA layers.  Both
    are float32-accurate evaluations of the same network: on the same 1 024-env batch they agree to a few float32
    rounding steps of the values (|v| ~ 1: 3e-6), far inside the 1e-5 parity bar each holds against the reference, and
    the rewards -- float64, computed outside the network -- are identical."""
    import torch
    from modelcrowdnav_amd import _hip
    rng = np.random.RandomState(70 + N)
    E = 1024
    pol = L.policy("sarl", seed=5)
    env = H.make_vec_env(E, N)
    H.upload(env, H.random_state(rng, E, N, randomize=True))
    with _hip.tuned(sarl_x3=1):
        _, best_x3, v_x3 = pol.predict_batch(env, want_values=True)
        v_x3, best_x3 = v_x3.clone(), best_x3.clone()
    with _hip.tuned(sarl_x3=0):
        _, best_f32, v_f32 = pol.predict_batch(env, want_values=True)
        v_f32, best_f32 = v_f32.clone(), best_f32.clone()
    torch.cuda.synchronize()
    d = (v_x3 - v_f32).abs().max().item()
    assert d <= 3e-6, d
    assert d > 0.0, "the two paths should not be the same kernel"
    same = (best_x3 == best_f32)
    # a different argmax needs two candidate values closer than the two paths' own difference
    top2 = torch.topk(v_f32, 2, dim=1).values
    assert bool((same | ((top2[:, 0] - top2[:, 1]) < 2 * d)).all())
    assert same.float().mean().item() > 0.99


@pytest.mark.parametrize("weights", ["seed 9", "g17"])
def test_network_error_against_a_float64_evaluation(weights, golden_dir):
    """How accurate is "float32-accurate"?  The value network evaluated in float64 on the same float32 inputs and
    weights is the yardstick: the torch float32 evaluation (what the reference runs), the float32 MFMA layers and the
    bf16x3 layers are three different roundings of it.  The bf16x3 path -- six of nine piece products, float32
    accumulation -- must not be further from the float64 result than twice the float32 reference's own distance
    (+ 5e-7); two weight sets (this package's default initialisation, the reference-side network recorded in g17)."""
    import torch
    from modelcrowdnav_amd import _hip
    N, E = 5, 256
    rng = np.random.RandomState(11)
    if weights == "g17":
        g = np.load(os.path.join(golden_dir, "g17_sarl_unicycle.npz"))
        pol = L.policy("sarl", L.weights(g, "w__"))
    else:
        pol = L.policy("sarl", seed=9)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    H.upload(env, st)
    with _hip.tuned(sarl_x3=1):
        _, _, v_x3 = pol.predict_batch(env, want_values=True)
        v_x3 = v_x3.cpu().numpy().copy()
    with _hip.tuned(sarl_x3=0):
        _, _, v_f32 = pol.predict_batch(env, want_values=True)
        v_f32 = v_f32.cpu().numpy().copy()
    w32, w64 = cpu_weights(pol), cpu_weights(pol, torch.float64)
    table, dt = pol._action_table, 0.25
    err = dict(x3=0.0, f32_mfma=0.0, torch_f32=0.0)
    for e in range(0, E, 8):
        if reached(st, e):
            continue
        nxt = np.stack([st.hpx[e] + st.hvx[e] * dt, st.hpy[e] + st.hvy[e] * dt, st.hvx[e], st.hvy[e], st.hr[e]], 1)
        rows = np.zeros((len(table), N, 14))
        rows[:, :, 0] = (st.rpx[e] + table[:, 0] * dt)[:, None]; rows[:, :, 1] = (st.rpy[e] + table[:, 1] * dt)[:, None]
        rows[:, :, 2] = table[:, 0][:, None]; rows[:, :, 3] = table[:, 1][:, None]
        rows[:, :, 4] = st.rr[e]; rows[:, :, 5] = st.rgx[e]; rows[:, :, 6] = st.rgy[e]; rows[:, :, 7] = 1.0
        rows[:, :, 9:] = nxt[None]
        feats = pyref.rotate(torch.from_numpy(rows.reshape(-1, 14)).float()).view(len(table), N, 13)
        truth = pyref.sarl_forward(w64, feats.double())[0].numpy()
        ref32 = pyref.sarl_forward(w32, feats)[0].double().numpy()
        rew = np.array([pyref.lookahead_reward(rows[a, 0, 0], rows[a, 0, 1], st.rr[e], st.rgx[e], st.rgy[e],
                                               [(h[0], h[1], h[4]) for h in nxt], dt) for a in range(len(table))])
        disc = 0.9 ** (dt * 1.0)
        err["x3"] = max(err["x3"], float(np.abs((v_x3[e] - rew) / disc - truth).max()))
        err["f32_mfma"] = max(err["f32_mfma"], float(np.abs((v_f32[e] - rew) / disc - truth).max()))
        err["torch_f32"] = max(err["torch_f32"], float(np.abs(ref32 - truth).max()))
    print("SARL network error vs float64 (weights: %s): %s" % (weights, ", ".join("%s %.2e" % kv for kv in err.items())))
    assert err["torch_f32"] > 0
    assert err["x3"] <= 2 * err["torch_f32"] + 5e-7, err
    assert err["f32_mfma"] <= 2 * err["torch_f32"] + 5e-7, err


@pytest.mark.parametrize("N", [5, 10])
def test_benchmark_grid_every_pair_against_the_torch_reference(N):
    """BASELINE configs 3 / 4 in full: all 4096 x 81 (env, action) values of one predict_batch against the torch-fp32
    restatement of MultiHumanRL.predict (multi_human_rl.py:35-63: propagate, reward ladder, rotate, ValueNetwork.forward),
    evaluated batched on the CPU -- not a sample of envs.  Bar 1e-5 on every value; the chosen action is the reference's
    wherever its top two values are further apart than that."""
    import torch
    rng = np.random.RandomState(90 + N)
    E, dt, gamma = 4096, 0.25, 0.9
    pol = L.policy("sarl", seed=4)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    torch.cuda.synchronize()
    values, best = values.cpu().numpy(), best.cpu().numpy()
    table = np.asarray(pol._action_table, np.float64)
    A = len(table)
    w = cpu_weights(pol)
    # propagate (float64), one row per (env, action, human)
    npx = st.rpx[:, None] + table[None, :, 0] * dt; npy = st.rpy[:, None] + table[None, :, 1] * dt          # [E, A]
    hx, hy = st.hpx + st.hvx * dt, st.hpy + st.hvy * dt                                                      # [E, N]
    rows = np.empty((E, A, N, 14))
    rows[..., 0] = npx[:, :, None]; rows[..., 1] = npy[:, :, None]
    rows[..., 2] = table[None, :, None, 0]; rows[..., 3] = table[None, :, None, 1]
    rows[..., 4] = st.rr[:, None, None]; rows[..., 5] = st.rgx[:, None, None]; rows[..., 6] = st.rgy[:, None, None]
    rows[..., 7] = 1.0; rows[..., 8] = 0.0
    rows[..., 9] = hx[:, None, :]; rows[..., 10] = hy[:, None, :]
    rows[..., 11] = st.hvx[:, None, :]; rows[..., 12] = st.hvy[:, None, :]; rows[..., 13] = st.hr[:, None, :]
    # reward ladder (multi_human_rl.py:65-88), float64
    d = np.sqrt((npx[:, :, None] - hx[:, None, :]) ** 2 + (npy[:, :, None] - hy[:, None, :]) ** 2) \
        - st.rr[:, None, None] - st.hr[:, None, :]                                                          # [E, A, N]
    coll = (d < 0).any(2)
    dmin = d.min(2)
    reach = np.sqrt((npx - st.rgx[:, None]) ** 2 + (npy - st.rgy[:, None]) ** 2) < st.rr[:, None]
    rew = np.where(coll, -0.25, np.where(reach, 1.0, np.where(dmin < 0.2, (dmin - 0.2) * 0.5 * dt, 0.0)))
    on_edge = (np.abs(d) < 1e-9).any(2) | (np.abs(dmin - 0.2) < 1e-9)        # a rung decided by the last bit: not compared
    net = np.empty((E, A))
    flat = torch.from_numpy(rows.reshape(E * A, N, 14))
    with torch.no_grad():
        for lo in range(0, E * A, 1 << 15):
            chunk = flat[lo:lo + (1 << 15)].float()
            B = chunk.shape[0]
            feats = pyref.rotate(chunk.reshape(B * N, 14)).view(B, N, 13)
            net.reshape(-1)[lo:lo + B] = pyref.sarl_forward(w, feats)[0].double().numpy()
    ref = rew + gamma ** (dt * 1.0) * net
    reached = np.sqrt((st.rpx - st.rgx) ** 2 + (st.rpy - st.rgy) ** 2) < st.rr       # policy.py:43-49: nothing evaluated
    ok = ~reached[:, None] & ~on_edge
    err = np.abs(values - ref)[ok]
    print("SARL 4096 x 81 x %d: %d of %d values compared, max |value - reference| = %.3g" % (N, ok.sum(), E * A, err.max()))
    assert ok.mean() > 0.9            # (random_state puts ~6 % of the robots on their goal: nothing is evaluated there)
    assert err.max() <= TOL
    moving = ~reached & ~on_edge.any(1)
    top2 = np.sort(ref, 1)[:, -2:]
    clear = moving & (top2[:, 1] - top2[:, 0] > 2 * TOL)
    assert clear.sum() > E // 2
    assert np.array_equal(best[clear], ref[clear].argmax(1))
    assert np.all(best[reached] == -1)
