"""GPU: OM-SARL (`[sarl] with_om = true`) through the C ABI -- the occupancy-map kernel (sarl_om.hip,
mcn_sarl_om_prepare) and the look-ahead that starts mlp1.0 from its output (sarl_value.hip WITH_OM,
mcn_sarl_predict_om) -- against the reference's recorded maps and predictions (g24_om_sarl.npz) and against
tests/om_ref.py + the torch-float32 network.

Bars: occupancy channel exact, velocity channels within 2.4e-7 (two float32 ulps at |v| <= 2); 1e-5 on values
(BASELINE.json north_star), the chosen action identical wherever the reference's top-2 gap exceeds 2e-5; network error
against float64 at most twice torch-float32's own + 5e-7.  Maps are compared only outside the edge band of
tests/om_ref.py, and every test asserts that this leaves out nothing.

Which test catches which break of the new code:
  init row of the tile's first env instead of the lane's .. test_predict_batch_at_benchmark_size, test_pair_counts
  maps of the current instead of the next states in predict  test_predict_matches_reference_fixture, ..._benchmark_size
  others at index >= hcount not masked ....................... test_hcount_masks_maps_and_humans
  bias added twice (fragment and init) ....................... test_predict_matches_reference_fixture (every value)
  dot-product form on a -0.0 velocity ........................ test_maps_match_reference_fixture (neg_zero_vx / _both)
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests import om_ref  # noqa: E402
from tests.lookahead_harness import TOL, cpu_weights, humans, reached, self_row  # noqa: E402

VEL_TOL = 2.4e-7
# H.random_state seeds of the 4096-env batches, picked once on the CPU: no pre-floor coordinate of the next states
# within the edge band (the expected count per batch is ~1e-3)
BATCH_SEED = {5: 245, 10: 250}


def _hum4(st):
    return np.stack([st.hpx, st.hpy, st.hvx, st.hvy], -1)                  # [E,N,4]


def _next4(st, dt=0.25):
    return np.stack([st.hpx + st.hvx * dt, st.hpy + st.hvy * dt, st.hvx, st.hvy], -1)


def _prepare(pol, hum, dt=0.0, hcount=None, nexts=None):
    """mcn_sarl_om_prepare on hum [E,N,4] (px, py, vx, vy) -> maps [E,N,48] (numpy)."""
    import torch
    from modelcrowdnav_amd import _hip
    dev = torch.device("cuda", 0)
    hum = np.ascontiguousarray(hum, np.float64)
    E, N, _ = hum.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    hpos, hvel = t(hum[:, :, 0:2]), t(hum[:, :, 2:4])
    st = _hip.EnvState()
    st.hpos, st.hvel = _hip.ptr(hpos), _hip.ptr(hvel)
    hc = None
    if hcount is not None:
        hc = t(np.asarray(hcount, np.int32))
        st.hcount = _hip.ptr(hc)
    npos = nvel = None
    if nexts is not None:
        npos, nvel = t(nexts[:, :, 0:2]), t(nexts[:, :, 2:4])
    om = torch.full((E, N, om_ref.WIDTH), float("nan"), dtype=torch.float32, device=dev)
    pol._om_prepare(st, dt, npos, nvel, om, E, N, dev)
    torch.cuda.synchronize()
    return om.cpu().numpy()


def _assert_maps(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got[..., 0::3], want[..., 0::3]), what                        # occupancy: exact
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= VEL_TOL, what


def _humans(rows4):
    from modelcrowdnav_amd.envs.utils.state import ObservableState
    return [ObservableState(*row, 0.3) for row in np.asarray(rows4).tolist()]


# ------------------------------------------------------------------------------------------------ 1. maps
def test_maps_match_reference_fixture(golden_dir):
    """build_occupancy_maps (one E = 1 launch) and the batched prepare against the reference's maps, generic and
    constructed states; the batched launch gives the bits of the E = 1 launch for the same humans."""
    g = np.load(os.path.join(golden_dir, "g24_om_sarl.npz"))
    pol = L.policy("om_sarl")
    left_out = 0
    for N in (2, 5, 10):
        hums, want = g["om_in_N%d" % N], g["om_out_N%d" % N]
        left_out += int((om_ref.edge_margin_batch(hums) <= om_ref.EDGE_BAND).sum())
        batch = _prepare(pol, hums)
        _assert_maps(batch, want, "batched N=%d" % N)
        for s in range(hums.shape[0]):
            one = pol.build_occupancy_maps(_humans(hums[s]))
            assert one.dtype.is_floating_point and tuple(one.shape) == (N, 48) and one.device.type == "cpu"
            _assert_maps(one.numpy(), want[s], "E=1 N=%d state %d" % (N, s))
            assert H.bits_equal(one.numpy(), batch[s]), (N, s)
    for name in [k[7:] for k in g.files if k.startswith("omc_in_")]:
        hum, want = g["omc_in_" + name], g["omc_out_" + name]
        left_out += int(om_ref.edge_margin(hum) <= om_ref.EDGE_BAND)
        one = pol.build_occupancy_maps(_humans(hum)).numpy()
        _assert_maps(one, want, name)
        assert H.bits_equal(one, _prepare(pol, hum[None])[0]), name
    assert left_out == 0


def test_every_cell_edge_from_both_sides():
    """Others displaced across every inner edge and the outer boundary of both axes by +-1e-6 (eight orders above libm
    noise), a generic half-cell offset along the other axis; a human with a generic velocity direction and a still one.
    The exact cell on both sides: the comparison directions and cell = 4 iy + ix."""
    pol = L.policy("om_sarl")
    cases, want = [], []
    for vel in ((0.53, -0.71), (0.0, 0.0)):
        th = np.arctan2(vel[1], vel[0])
        c, s = np.cos(th), np.sin(th)
        for axis in (0, 1):
            for m in range(5):
                for side in (-1e-6, 1e-6):
                    along, other = m - 2 + side, 0.37 - 1.0 * (m % 2)             # other axis: grid coordinate 2.37 / 1.37
                    xp, yp = (along, other) if axis == 0 else (other, along)
                    p0 = np.array([0.4, -0.9])
                    p1 = p0 + np.array([c * xp - s * yp, s * xp + c * yp])
                    cases.append([[p0[0], p0[1], vel[0], vel[1]], [p1[0], p1[1], 0.2, 0.1]])
                    ia = m if side > 0 else m - 1
                    io = 2 if m % 2 == 0 else 1
                    ix, iy = (ia, io) if axis == 0 else (io, ia)
                    want.append(4 * iy + ix if 0 <= ia < 4 else -1)
    hum = np.array(cases)
    assert hum.shape == (40, 2, 4)
    # the walk itself is the only place a coordinate may be near an edge -- and there it is 1e-6 away, not 1e-9
    for e in range(len(hum)):
        _, gx, gy, _, _, _ = om_ref._turned(hum[e], 0, 1.0)
        assert np.abs(np.array([gx[0], gy[0]])[:, None] - np.arange(5)[None]).min() > 5e-7
    got = _prepare(pol, hum)
    for e, cell in enumerate(want):
        occ = np.zeros(16, np.float32)
        if cell >= 0:
            occ[cell] = 1
        assert np.array_equal(got[e, 0, 0::3], occ), (e, cell, got[e, 0, 0::3])
        assert np.array_equal(got[e, 0, 0::3], om_ref.maps(hum[e])[0, 0::3]), e


def test_non_finite_coordinates_fall_into_no_cell():
    pol = L.policy("om_sarl")
    base = np.array([[0.0, 0.0, 1.0, 0.0], [0.5, 0.5, 0.1, 0.2], [-0.5, 0.25, 0.3, -0.2]])
    assert om_ref.edge_margin(base) > om_ref.EDGE_BAND
    good = _prepare(pol, base[None])[0]
    for bad in (np.nan, np.inf, -np.inf):
        hum = base.copy()
        hum[2, 0] = bad                                   # human 2 is nowhere: in nobody's map, and nobody is in its
        got = _prepare(pol, hum[None])[0]
        assert np.array_equal(got[0, 0::3], om_ref.maps(base[:2])[0, 0::3])
        assert not got[2].any()
        assert np.isfinite(got).all() and got[0, 0::3].sum() == good[0, 0::3].sum() - 1


# ------------------------------------------------------------------------------------------------ 2. E = 1 predict
@pytest.mark.parametrize("kin", ["holonomic", "unicycle"])
def test_predict_matches_reference_fixture(kin, golden_dir):
    g = np.load(os.path.join(golden_dir, "g24_om_sarl.npz"))

    def each(pol, g, key, s, N, compared):
        if compared:
            assert pol.get_attention_weights().shape == (N,)
        else:
            assert om_ref.edge_margin(om_ref.next_humans(g[key + "humans"][s][:, :4])) > om_ref.EDGE_BAND
    compared = L.check_fixture_predictions("om_sarl", g, (2, 5, 10), "pred_{kin}_N{N}_", kin, seeds=(0,), each=each)
    assert compared > 60


def test_train_phase_epsilon_and_last_state_match_reference(golden_dir):
    """epsilon 0.5 on numpy's global stream; last_state = [rotate | maps of the CURRENT states], [N, 61]."""
    import torch
    g = np.load(os.path.join(golden_dir, "g24_om_sarl.npz"))
    for s in range(g["eps_selfs"].shape[0]):
        assert om_ref.edge_margin(g["eps_humans"][s][:, :4]) > om_ref.EDGE_BAND

    def each(pol, s, want):
        assert tuple(pol.last_state.shape) == (5, 61)
        assert torch.equal(pol.last_state.cpu()[:, 13::3], want[:, 13::3])
    L.check_epsilon_fixture("om_sarl", g, 0, 2400 + int(g["eps_seed"]), reset_values=True, each=each,
                            keeps_last_state=lambda s: int(g["eps_explored"][s]) != 2)
    assert set(g["eps_explored"].tolist()) >= {0, 1}


def test_one_human_raises_value_error():
    from modelcrowdnav_amd.envs.utils.state import FullState, ObservableState, JointState
    pol = L.policy("om_sarl", seed=1)
    one = [ObservableState(1.0, 1.0, 0.1, 0.2, 0.3)]
    js = JointState(FullState(0, 0, 0, 0, 0.3, 0, 4, 1.0, 0.0), one)
    for call in (lambda: pol.predict(js), lambda: pol.transform(js), lambda: pol.build_occupancy_maps(one)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------------ 3. benchmark size
@pytest.mark.parametrize("x3", [1, 0])
@pytest.mark.parametrize("N", [5, 10])
def test_predict_batch_at_benchmark_size(N, x3):
    """4096 envs x 81 actions, both layer forms: every value of >= 64 sampled envs (0, 1, 15, 16, 17, E-1 among them:
    both envs of a 16-pair tile that spans two) against om_ref + the torch-float32 network; best == argmax; transform_batch
    rows and the E = 1 path's values are the batch's bits for the same env."""
    import torch
    from modelcrowdnav_amd import _hip
    rng = np.random.RandomState(BATCH_SEED[N])
    E = 4096
    pol = L.policy("om_sarl", seed=3)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    assert int((om_ref.edge_margin_batch(_next4(st)) <= om_ref.EDGE_BAND).sum()) == 0
    assert int((om_ref.edge_margin_batch(_hum4(st)) <= om_ref.EDGE_BAND).sum()) == 0
    H.upload(env, st)
    with _hip.tuned(sarl_x3=x3):
        actions, best, values = pol.predict_batch(env, want_values=True)
        torch.cuda.synchronize()
        values, best, actions = values.cpu().numpy().copy(), best.cpu().numpy().copy(), actions.cpu().numpy().copy()
        rows = pol.transform_batch(env).cpu()
        assert tuple(rows.shape) == (E, N, 61)
        w, table = cpu_weights(pol), pol._action_table
        sample = L.sample_envs(rng, E, 58, always=(1, 15, 16, 17, 2047, 2048, E - 2))
        assert len(sample) >= 64
        for e in sample:
            ref = om_ref.values(w, self_row(st, e), humans(st, e), table, "holonomic")
            L.check_choice(values[e], best[e], actions[e], ref, table, reached(st, e), what="env %d" % e)
        for e in sample[:10]:
            pol.last_state = None
            pol.set_phase("train"); pol.set_epsilon(0.0)
            pol.predict(L.joint_state(self_row(st, e), humans(st, e)))
            pol.set_phase("test")
            if not reached(st, e):
                assert np.array_equal(np.array(pol.action_values), values[e]), e            # same bits
                assert torch.equal(pol.last_state.cpu(), rows[e]), e
                # current states, not next ones
                assert np.array_equal(rows[e][:, 13:].numpy()[:, 0::3], om_ref.maps(_hum4(st)[e])[:, 0::3])


# ------------------------------------------------------------------------------------------------ 4. float64 yardstick
@pytest.mark.parametrize("weights", ["g24", "seed 9"])
def test_network_error_against_a_float64_evaluation(weights, golden_dir):
    """The 61-input network in float64 on the same float32 inputs and weights is the yardstick; the hoisted mlp1.0 in
    either layer form must not be further from it than twice the torch float32 evaluation is (+ 5e-7)."""
    import torch
    from modelcrowdnav_amd import _hip
    N, E = 5, 256
    rng = np.random.RandomState(11)
    if weights == "g24":
        pol = L.policy("om_sarl", L.weights(np.load(os.path.join(golden_dir, "g24_om_sarl.npz")), "w0__"))
    else:
        pol = L.policy("om_sarl", seed=9)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    assert int((om_ref.edge_margin_batch(_next4(st)) <= om_ref.EDGE_BAND).sum()) == 0
    H.upload(env, st)
    got = {}
    for name, x3 in (("x3", 1), ("f32_mfma", 0)):
        with _hip.tuned(sarl_x3=x3):
            _, _, v = pol.predict_batch(env, want_values=True)
            got[name] = v.cpu().numpy().copy()
    assert not np.array_equal(got["x3"], got["f32_mfma"]), "the two layer forms should not be the same kernel"
    w32, w64 = cpu_weights(pol), cpu_weights(pol, torch.float64)
    table, disc = pol._action_table, 0.9 ** 0.25
    err = dict(x3=0.0, f32_mfma=0.0, torch_f32=0.0)
    for e in range(0, E, 8):
        if reached(st, e):
            continue
        x, rew = om_ref.rows61(self_row(st, e), humans(st, e), table, "holonomic")
        rew = np.array(rew, np.float64)
        with torch.no_grad():
            from oracle import pyref
            truth = pyref.sarl_forward(w64, x.double())[0].numpy()
            ref32 = pyref.sarl_forward(w32, x)[0].double().numpy()
        for name in ("x3", "f32_mfma"):
            err[name] = max(err[name], float(np.abs((got[name][e] - rew) / disc - truth).max()))
        err["torch_f32"] = max(err["torch_f32"], float(np.abs(ref32 - truth).max()))
    print("OM-SARL network error vs float64 (weights: %s): %s" % (weights, ", ".join("%s %.2e" % kv for kv in err.items())))
    assert err["torch_f32"] > 0
    assert err["x3"] <= 2 * err["torch_f32"] + 5e-7, err
    assert err["f32_mfma"] <= 2 * err["torch_f32"] + 5e-7, err


# ------------------------------------------------------------------------------------------------ 5. hcount
def test_hcount_masks_maps_and_humans():
    """Humans at index >= hcount[e] are in nobody's map and have none: NaN / +-inf there change no output bit;
    hcount[e] = 1 gives zero maps; counts are clamped to 1 .. N as everywhere."""
    import torch
    rng = np.random.RandomState(7)
    E, N = 300, 6
    pol = L.policy("om_sarl", seed=5)
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    hcn = rng.randint(1, N + 1, E).astype(np.int32)
    hcn[:6] = [0, N + 3, -2, 1, 2, N]
    seen = np.clip(hcn, 1, N)
    left_out = sum(om_ref.edge_margin(_next4(st)[e], count=seen[e]) <= om_ref.EDGE_BAND for e in range(E))
    assert left_out == 0
    H.upload(env, st)
    hc = torch.from_numpy(hcn).cuda()
    _, _, values = pol.predict_batch(env, want_values=True, hcount=hc)
    values = values.cpu().numpy().copy()
    om = pol._bufs["om"].cpu().numpy().copy()
    w = cpu_weights(pol)
    for e in list(range(6)) + list(range(6, E, 7)):
        n = int(seen[e])
        want = om_ref.maps(_next4(st)[e], count=n)
        _assert_maps(om[e], want, "env %d" % e)
        assert not om[e, n:].any()
        if n == 1:
            assert not om[e].any()
        if reached(st, e):
            continue
        if n >= 2:
            ref = om_ref.values(w, self_row(st, e), humans(st, e)[:n], pol._action_table, "holonomic")
        else:       # the reference has no answer for a lone human: the zero map is this build's rule (include/mcn.h)
            from tests import policy_ref as R
            from oracle import pyref
            xr, rew = R.rotated_rows(self_row(st, e), humans(st, e)[:1], pol._action_table, "holonomic")
            x = torch.cat([xr, torch.zeros(xr.shape[0], 1, 48)], 2)
            with torch.no_grad():
                ref = np.array(rew) + 0.9 ** 0.25 * pyref.sarl_forward(w, x)[0].double().numpy()
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL, err_msg="env %d" % e)
    # garbage in the slots the policy does not see changes no bit
    bad = np.array([np.nan, np.inf, -np.inf])
    for e in range(E):
        for i in range(int(seen[e]), N):
            st.hpx[e, i], st.hpy[e, i] = bad[(e + i) % 3], bad[(e + 2 * i) % 3]
            st.hvx[e, i], st.hvy[e, i] = bad[(e + i + 1) % 3], 1e300
    H.upload(env, st)
    _, _, values2 = pol.predict_batch(env, want_values=True, hcount=hc)
    assert H.bits_equal(values2.cpu().numpy(), values)
    assert H.bits_equal(pol._bufs["om"].cpu().numpy(), om)


# ------------------------------------------------------------------------------------------------ 6. query_env
def test_query_env_builds_the_maps_from_the_envs_next_states():
    import torch
    rng = np.random.RandomState(31)
    E, N = 64, 5
    pol = L.policy("om_sarl", seed=9)
    pol.query_env = True
    env = H.make_vec_env(E, N)
    st = H.random_state(rng, E, N, randomize=True)
    H.upload(env, st)
    pol.build_action_space(1.0)
    pol._bufs = {}
    npos, nvel, rew = pol._query_env(env)
    npos, nvel, rew = npos.cpu().numpy(), nvel.cpu().numpy(), rew.cpu().numpy()
    nexts = np.concatenate([npos, nvel], 2)
    assert int((om_ref.edge_margin_batch(nexts) <= om_ref.EDGE_BAND).sum()) == 0
    _, _, values = pol.predict_batch(env, want_values=True)
    values = values.cpu().numpy()
    om = pol._bufs["om"].cpu().numpy()
    w = cpu_weights(pol)
    moved = 0
    for e in range(0, E, 3):
        _assert_maps(om[e], om_ref.maps(nexts[e]), "env %d" % e)
        moved += int(not np.array_equal(om_ref.maps(nexts[e]), om_ref.maps(_next4(st)[e])))
        ref = om_ref.values(w, self_row(st, e), humans(st, e), pol._action_table, "holonomic", nexts=nexts[e],
                            rewards=rew[e])
        np.testing.assert_allclose(values[e], ref, rtol=0, atol=TOL)
    assert moved > 0, "the env's next states should differ from constant-velocity ones somewhere"


# ------------------------------------------------------------------------------------------------ 7. pair counts
@pytest.mark.parametrize("E,speeds,rotations,kin", [(1, 2, 4, "holonomic"), (3, 2, 4, "holonomic"), (37, 5, 16, "holonomic"),
                                                    (700, 5, 16, "holonomic"), (5, 3, 5, "unicycle")])
def test_pair_counts(E, speeds, rotations, kin):
    """E x A below one 16-pair tile, not a multiple of 16 (a tile spans two or three envs), more tile groups than the
    persistent grid walks at once, a second and third action table size: the init row follows the LANE's env."""
    import torch
    N = 4
    rng = np.random.RandomState(100 + E)
    pol = L.policy("om_sarl", seed=6, kinematics=kin)
    pol.speed_samples, pol.rotation_samples = speeds, rotations
    env = H.make_vec_env(E, N, kinematics=kin)
    st = H.random_state(rng, E, N, randomize=True)
    st.rtheta[:] = rng.uniform(-np.pi, np.pi, E) if kin == "unicycle" else 0.0
    assert int((om_ref.edge_margin_batch(_next4(st)) <= om_ref.EDGE_BAND).sum()) == 0
    H.upload(env, st)
    actions, best, values = pol.predict_batch(env, want_values=True)
    values, best, actions = values.cpu().numpy(), best.cpu().numpy(), actions.cpu().numpy()
    A = 1 + speeds * rotations
    assert values.shape == (E, A)
    w = cpu_weights(pol)
    for e in (range(E) if E <= 37 else [0, 1, 2, 3, 4, E - 1] + list(range(5, E, 29))):
        ref = om_ref.values(w, self_row(st, e), humans(st, e), pol._action_table, kin)
        L.check_choice(values[e], best[e], actions[e], ref, pol._action_table, reached(st, e), what="env %d" % e)


# ------------------------------------------------------------------------------------------------ 8. callers
def test_explorer_batched_equals_sequential():
    """Explorer.run_k_episodes(64, 'test') with an OM-SARL robot goes to the batched VecExplorer and reports what the
    sequential E = 1 loop reports."""
    L.check_explorer_batched_equals_sequential("om_sarl")


def test_update_memory_stores_61_wide_rows():
    """Imitation learning with the ORCA robot and an OM-SARL target policy: the memory holds [N, 61] rows whose map
    part is the map of the state the row was taken in."""
    import torch
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.rollout import VecExplorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    dev = torch.device("cuda", 0)
    E, N = 16, 5
    env = H.make_vec_env(E, N)
    env.track_human_times = False; env.export_human_actions = False
    om_sarl = L.policy("om_sarl", seed=0, phase="train")
    om_sarl.time_step = env.time_step
    mem = ReplayMemory(20000, device=dev)
    orca = policy_factory["orca"]()
    orca.multiagent_training = True
    orca.safety_space = 0.15
    env.robot.set_policy(orca)
    ex = VecExplorer(env, env.robot, gamma=0.9, policy=orca, memory=mem, target_policy=om_sarl)
    ex.run_k_episodes(E, "train", update_memory=True, imitation_learning=True)
    assert len(mem) > 0
    rows = torch.stack([mem[i][0] for i in range(len(mem))]).cpu()
    assert tuple(rows.shape[1:]) == (N, 61)
    occ = rows[:, :, 13::3]
    assert bool(((occ == 0) | (occ == 1)).all()) and occ.sum() > 0


def test_trainer_step_changes_weights_and_next_predict_uses_them():
    """An optimizer step re-packs both halves of mlp1.0 (columns 0..12 and the map fragment + bias)."""
    import torch

    def check_inputs(st, rows):
        assert int((om_ref.edge_margin_batch(_next4(st)) <= om_ref.EDGE_BAND).sum()) == 0
        assert tuple(rows.shape) == (st.E, st.N, 61)

    def check_changed(before, after):
        assert not torch.equal(before["mlp1.0.weight"][:, 13:], after["mlp1.0.weight"][:, 13:])
        assert not torch.equal(before["mlp1.0.bias"], after["mlp1.0.bias"])

    def reference(pol):
        w = cpu_weights(pol)
        return lambda st, e: om_ref.values(w, self_row(st, e), humans(st, e), pol._action_table, "holonomic")
    L.check_trainer_step_is_seen("om_sarl", reference, randomize=True, check_inputs=check_inputs,
                                 check_changed=check_changed)
