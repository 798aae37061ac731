"""GPU: the SARL look-ahead (sarl_value.hip: sarl_value_kernel in both variants, sarl_argmax_kernel) at its edges.

  * the classes of the reference's un-stabilised masked softmax (sarl.py:52-53): every score exactly 0 (0 / 0), an exp
    that overflows (inf / inf), every exp underflowing (0 / 0) are NaN; sums far below the float32 reciprocal's range
    are finite; humans that score exactly 0 drop out;
  * NaN of either sign and +-inf in a present human, the robot or an action row: the reference's class, neighbours in
    the same 16-pair tile untouched, nothing from beyond hcount;
  * hcount clamps and masks, the attention output, pair counts around a wavefront, a workgroup and a round of the
    persistent grid, stale workspace rows, the query_env form, feature edges;
  * sarl_argmax_kernel on exact values: ties, +-inf, NaN, subnormal gaps, epsilon = 1, a robot on its goal.

The reference everywhere is torch on the CPU (oracle/pyref through tests/sarl_states.reference): float32 for parity,
float64 on the same float32 features as the yardstick.  Bar: 1e-5 absolute on values and attention weights
(BASELINE.json north_star, TOL of tests/lookahead_harness.py).  Both variants of the kernel run every case: the bf16x3
layers (mcn_tuning.sarl_x3 = 1, the default) and the float32 MFMA layers (0)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402
from tests import lookahead_harness as L  # noqa: E402
from tests import sarl_states as S  # noqa: E402
from tests.lookahead_harness import SENTINEL, TOL, run_lookahead as _run  # noqa: E402

X3 = pytest.mark.parametrize("x3", [1, 0], ids=["bf16x3", "f32mfma"])


def _policy(w, kinematics="holonomic", table=None):
    pol = L.policy("sarl", weights=w, kinematics=kinematics)
    pol.build_action_space(1.0)
    return pol if table is None else L.with_table(pol, table)


def _check_argmax(out, e, table, reached=False, ref=None):
    """best and the action row of env e by L.check_choice (against ref [A] too where given), best_val against the
    strict-'>' scan of the kernel's own values."""
    L.check_choice(out["values"][e], out["best"][e], out["actions"][e], ref, table, reached, what="env %d" % e)
    if not reached:
        H.assert_bits_equal(out["best_val"][e], S.scan_argmax(out["values"][e])[1], "best_val of env %d" % e)


def _check_finite_env(out, ref, e, table, what="", att_tol=TOL):
    n = ref["att"].shape[1]
    np.testing.assert_allclose(out["att"][e][:, :n], ref["att"], rtol=0, atol=att_tol, err_msg="%s env %d attention" % (what, e))
    assert np.all(out["att"][e][:, n:] == 0.0), (what, e)
    assert np.all(np.abs(out["att"][e].sum(1) - 1.0) < TOL), (what, e)
    _check_argmax(out, e, table, ref=ref["values"])


def _check_nan_env(out, ref, e):
    """Every value of env e NaN, `best` as sarl_argmax_kernel documents for "no value wins" (-1, -inf, the zero
    action), attention NaN where the reference's weights are."""
    assert np.isnan(ref["values"]).all()
    assert np.isnan(out["values"][e]).all(), (e, out["values"][e])
    assert out["best"][e] == -1 and out["best_val"][e] == -np.inf and tuple(out["actions"][e]) == (0.0, 0.0), e
    n = ref["att"].shape[1]
    assert np.array_equal(np.isnan(out["att"][e][:, :n]), np.isnan(ref["att"])), e
    assert np.all(out["att"][e][:, n:] == 0.0), e


# ------------------------------------------------------------------------------------------------ 1. softmax classes
@X3
@pytest.mark.parametrize("shift", S.FINITE_SHIFTS)
def test_softmax_finite_classes(shift, x3):
    """attention.4.bias shifted by 0, +-80, -90, -92: the float32 reference is finite and so is the kernel, within 1e-5.
    At -92 every exp is ~1e-40 and the sum is below 2^-128, where a float32 reciprocal of it overflows.  Against the
    float64 evaluation the kernel stays under 2 x torch-float32's own distance + 5e-7 for shifts 0 and +-80; for -90 and
    -92 both distances are printed (DESIGN 3.2 records them).
    The attention weights hold the 1e-5 bar at shift 0.  A shifted score is a float32 sum of 101 terms of magnitude up to
    |shift| + 1, so two float32 summation orders may differ by 101 half-ulps of that magnitude, and a weight moves by
    no more than the scores do (d a_i / d s_j is at most 1/4 in size, summed over j at most 1/2): that is the bar there
    (3.9e-4 at |shift| >= 64); the measured distance is ~1.2e-5."""
    w = S.shifted(S.g5_weights(), shift)
    pol = _policy(w)
    table = pol._action_table
    att_tol = max(TOL, 101 * 0.5 * float(np.spacing(np.float32(abs(shift) + 1.0))))
    for N in S.SOFTMAX_NS:
        st = S.softmax_batch(N)
        out = _run(pol, st, x3)
        err_k, err_t, err_a = 0.0, 0.0, 0.0
        for e in range(st.E):
            ref = S.reference(w, st, e, table, float64=True)
            assert np.isfinite(ref["values"]).all()
            net = (out["values"][e] - ref["reward"]) / S.DISC
            err_k = max(err_k, float(np.abs(net - ref["V64"]).max()))
            err_t = max(err_t, float(np.abs(ref["V"] - ref["V64"]).max()))
            _check_finite_env(out, ref, e, table, "shift %g N %d" % (shift, N), att_tol)
            err_a = max(err_a, float(np.abs(out["att"][e] - ref["att"]).max()))
        print("SARL softmax shift %+g, N = %d, %s: |V - float64| kernel %.2e, torch float32 %.2e; |attention - torch| %.2e"
              % (shift, N, "bf16x3" if x3 else "float32 MFMA", err_k, err_t, err_a))
        assert err_t > 0
        if shift in S.YARDSTICK_SHIFTS:
            assert err_k <= 2 * err_t + 5e-7, (shift, N, err_k, err_t)


@X3
@pytest.mark.parametrize("case", ["zero-attention", "shift+100", "shift-110"])
def test_softmax_nan_classes(case, x3):
    """Every present score exactly 0, every exp overflowing, every exp underflowing: the reference's softmax is 0 / 0 or
    inf / inf and every value NaN; so are the kernel's, and no action wins."""
    w0 = S.g5_weights()
    w = S.zero_attention(w0) if case == "zero-attention" else S.shifted(w0, float(case[5:]))
    pol = _policy(w)
    for N in S.SOFTMAX_NAN_NS:
        st = S.softmax_batch(N)
        out = _run(pol, st, x3)
        for e in range(st.E):
            _check_nan_env(out, S.reference(w, st, e, pol._action_table), e)


@X3
def test_humans_scoring_exactly_zero_drop_out_of_the_softmax(x3):
    """The hand-set network scores a human of radius 0.25 exactly 0 and one of radius 0.5 exactly 1: the zero-scored ones
    get weight 0 (not exp(0) = 1), as `exp(s) * (s != 0)` does; an env of zero-scored humans only is 0 / 0."""
    w = S.mixed_network(S.g5_weights())
    pol = _policy(w)
    table = pol._action_table
    for N in (2, 5, 10):
        st = S.states(2, 8, N)
        st.hr[:] = S.mixed_radii(st.E, N)
        out = _run(pol, st, x3)
        mixed = 0
        for e in range(st.E):
            ref = S.reference(w, st, e, table)
            if (st.hr[e] == 0.25).all():
                _check_nan_env(out, ref, e)
                continue
            _check_finite_env(out, ref, e, table, "mixed N %d" % N)
            dropped = st.hr[e] == 0.25
            assert np.all(out["att"][e][:, dropped] == 0.0) and np.all(ref["att"][:, dropped] == 0.0), e
            assert np.all(out["att"][e][:, ~dropped] > 0.0), e
            mixed += int(dropped.any())
        assert mixed >= st.E - 2


# ------------------------------------------------------------------------------------------------ 2. non-finite state
@X3
@pytest.mark.parametrize("N", [5, 2])
def test_nonfinite_state_gives_the_reference_class_and_spares_the_tile(N, x3):
    """NaN of each sign, +inf and -inf in a present human's position, velocity and radius and in the robot's position
    and goal (one per odd env): every (env, action) value is in the reference's class -- NaN for the whole env -- and
    within 1e-5 where finite.  The clean even envs, which share 16-pair tiles with them, are bit for bit what a run
    without any poison gives."""
    w = S.g5_weights()
    pol = _policy(w)
    table = pol._action_table
    clean, bad, names = S.poison_batch(N)
    want = _run(pol, clean, x3)
    got = _run(pol, bad, x3)
    for e in range(bad.E):
        if names[e] is None:
            for k in ("values", "att", "best", "best_val", "actions"):
                H.assert_bits_equal(got[k][e], want[k][e], "%s of clean env %d beside %s" % (k, e, names[min(e + 1, bad.E - 2)]))
            continue
        ref = S.reference(w, bad, e, table)
        cls = S.classes(ref["values"])
        assert np.array_equal(S.classes(got["values"][e]), cls), (names[e], got["values"][e][:4], ref["values"][:4])
        fin = cls == 0
        np.testing.assert_allclose(got["values"][e][fin], ref["values"][fin], rtol=0, atol=TOL, err_msg=names[e])
        assert np.array_equal(np.isnan(got["att"][e]), np.isnan(ref["att"])), names[e]
        _check_argmax(got, e, table)
    for e in (0, 2, bad.E - 1):
        _check_finite_env(want, S.reference(w, clean, e, table), e, table, "clean")


@X3
def test_nonfinite_action_rows(x3):
    """NaN of each sign, +inf and -inf in four rows of the action table: those actions are in the reference's class for
    every env, every other action is bit for bit what the clean table gives, and the argmax passes over the NaN."""
    w = S.g5_weights()
    st = S.states(3, 6, 5)
    clean = _policy(w)
    table = S.poison_table(clean._action_table)
    want = _run(clean, st, x3)
    pol = _policy(w, table=table)
    got = _run(pol, st, x3)
    rows = sorted(S.POISON_ROWS)
    others = [a for a in range(len(table)) if a not in rows]
    for e in range(st.E):
        ref = S.reference(w, st, e, table)
        assert np.array_equal(S.classes(got["values"][e]), S.classes(ref["values"])), e
        assert S.classes(ref["values"])[rows].tolist() == [1, 1, 1, 1]
        H.assert_bits_equal(got["values"][e][others], want["values"][e][others], "untouched actions of env %d" % e)
        H.assert_bits_equal(got["att"][e][others], want["att"][e][others], "untouched attention of env %d" % e)
        assert np.array_equal(np.isnan(got["att"][e]), np.isnan(ref["att"])), e
        _check_argmax(got, e, table)
        assert got["best"][e] not in rows


@X3
def test_nonfinite_humans_beyond_hcount_change_nothing(x3):
    w = S.g5_weights()
    pol = _policy(w)
    N = 7
    st = S.states(4, 16, N)
    hc = (1 + np.arange(st.E) % N).astype(np.int32)
    want = _run(pol, st, x3, hcount=hc)
    got = _run(pol, S.poison_beyond(st, hc), x3, hcount=hc)
    for k in ("values", "att", "best", "best_val", "actions"):
        H.assert_bits_equal(got[k], want[k], k)
    assert np.isfinite(got["values"]).all()
    for e in (0, 3, N - 1, st.E - 1):
        _check_finite_env(got, S.reference(w, st, e, pol._action_table, n=int(hc[e])), e, pol._action_table, "hcount")


def test_bf16x3_input_range_ends_where_the_first_bfloat16_piece_is_infinite():
    """The documented input range of the bf16x3 layers (mcn.h, beside sarl_x3): below 2^128 - 2^119 = 3.3962e38 in size.
    From there on a float32 rounds to an infinite first bfloat16 piece and has no three-piece split; what the bf16x3
    variant returns for the env is not specified, while the float32 MFMA layers, like the reference, carry every finite
    float32.  Pinned with human radii whose two features (10 and 12) meet zero weights in mlp1.0: at 3.395e38 -- above
    the largest bfloat16 (3.3895e38), below the limit -- both variants are right; at 3.4e38 the float32 MFMA variant is
    right, and the bf16x3 variant still leaves every other env alone."""
    w = S.g5_weights()
    w["mlp1.0.weight"][:, 10] = 0.0
    w["mlp1.0.weight"][:, 12] = 0.0
    pol = _policy(w)
    table = pol._action_table
    st = S.states(15, 4, 5)
    st.hr[1, 2] = 3.4e38
    st.hr[2, 4] = 3.395e38
    limit = 2.0 ** 128 - 2.0 ** 119
    assert float(np.float32(0.3) + np.float32(3.395e38)) < limit < float(np.float32(3.4e38)) < np.finfo(np.float32).max
    assert np.isfinite(np.float32(0.3) + np.float32(3.4e38)) and float(np.float32(3.395e38)) > 3.3895e38
    f32, x3 = _run(pol, st, 0), _run(pol, st, 1)
    for e in range(st.E):
        ref = S.reference(w, st, e, table)
        assert np.isfinite(ref["values"]).all()
        _check_finite_env(f32, ref, e, table, "float32 MFMA")
        if e != 1:
            _check_finite_env(x3, ref, e, table, "bf16x3")


# ------------------------------------------------------------------------------------------------ 3. hcount, attention
@X3
def test_hcount_clamps_to_one_and_n_and_masks_the_attention(x3):
    """hcount 0 (and below) is 1, N + 3 is N; hcount = 1 with N = 32.  The attention output is exactly 0 in absent slots
    and sums to 1 over the present ones."""
    w = S.g5_weights()
    pol = _policy(w)
    table = pol._action_table
    for N in (6, 32):
        st = S.states(5, 10, N)
        hc = np.array([0, N + 3, 1, N, -4, 2, N - 1, 1, 3, N], np.int32)
        eff = np.clip(hc, 1, N)
        out = _run(pol, st, x3, hcount=hc)
        for e in range(st.E):
            _check_finite_env(out, S.reference(w, st, e, table, n=int(eff[e])), e, table, "hcount %d of %d" % (hc[e], N))
        one = out["att"][2]
        assert np.all(one[:, 0] == 1.0) and np.all(one[:, 1:] == 0.0)


@X3
@pytest.mark.parametrize("N", [1, 5, 32])
def test_attention_output_against_the_reference_weights(N, x3):
    """want_attention of CADRL._lookahead: [E,A,N] weights of every candidate action against pyref.sarl_forward's."""
    w = S.g5_weights(1)
    pol = _policy(w)
    st = S.states(6, 5, N)
    out = _run(pol, st, x3)
    for e in range(st.E):
        ref = S.reference(w, st, e, pol._action_table)
        _check_finite_env(out, ref, e, pol._action_table, "N %d" % N)
        if N > 1:
            assert ref["att"].std() * N > 1e-3        # (not the uniform weights a broken score would also give)


# ------------------------------------------------------------------------------------------------ 4. grid, workspace
def _grid():
    """(pairs per wavefront, wavefronts per workgroup, workgroups of the persistent grid) from the library itself: the
    workspace holds one slot per resident wavefront, N x 12 + 7 rows of 64 float4 each (mcn.h)."""
    from modelcrowdnav_amd import _hip
    slot = (1 * 12 + 7) * 64 * 16
    waves = _hip.lib.mcn_sarl_workspace_bytes(1, 1, 1) // slot
    blocks = _hip.lib.mcn_sarl_workspace_bytes(1 << 20, 1, 81) // slot // waves
    assert waves in (4, 8) and blocks >= 1
    return 16, int(waves), int(blocks)


@X3
@pytest.mark.parametrize("N", [1, 32])
def test_pair_counts_around_a_wavefront_and_a_workgroup(N, x3):
    """E x A = 1 pair, one short of / exactly / one more than a wavefront's 16 and a workgroup's pairs."""
    per_wave, waves, _ = _grid()
    group = per_wave * waves
    w = S.g5_weights()
    full = _policy(w)._action_table
    st = S.states(7, 1, N)
    for A in (1, per_wave - 1, per_wave, per_wave + 1, group - 1, group, group + 1):
        table = full[:A]
        pol = _policy(w, table=table)
        out = _run(pol, st, x3)
        assert out["values"].shape == (1, A)
        _check_finite_env(out, S.reference(w, st, 0, table), 0, table, "A %d N %d" % (A, N))
    # the same counts as E envs of one action
    for E in (per_wave + 1, group + 1):
        st = S.states(8, E, N)
        pol = _policy(w, table=full[5:6])
        out = _run(pol, st, x3)
        for e in range(E):
            _check_finite_env(out, S.reference(w, st, e, full[5:6]), e, full[5:6], "E %d N %d" % (E, N))


@X3
@pytest.mark.parametrize("N", [1, 32])
def test_more_than_one_round_of_the_persistent_grid(N, x3):
    """One round of the grid plus 37 pairs: the second round is one ragged workgroup (two full wavefronts, one of 5
    pairs, one idle).  The last env straddles the rounds; every value is written."""
    per_wave, waves, blocks = _grid()
    round_pairs = per_wave * waves * blocks
    E = round_pairs // 81 + 1
    assert 0 < E * 81 - round_pairs < per_wave * waves
    w = S.g5_weights()
    pol = _policy(w)
    table = pol._action_table
    st = S.states(9, E, N)
    out = _run(pol, st, x3)
    assert np.isfinite(out["values"]).all() and np.abs(out["values"]).max() < 100
    assert (out["att"] != SENTINEL).all() and (out["best"] >= 0).all()
    rng = np.random.RandomState(N)
    for e in L.sample_envs(rng, E, 6, always=(1, E - 3, E - 2)):
        _check_finite_env(out, S.reference(w, st, e, table), e, table, "E %d N %d" % (E, N))


@X3
def test_stale_workspace_rows_do_not_reach_a_later_launch(x3):
    """The workspace is indexed by resident wavefront and reused from launch to launch: a small batch right after a large
    one, and N = 1 right after N = 32, on the same policy object must be bit for bit what a fresh policy object gives."""
    per_wave, waves, blocks = _grid()
    w = S.g5_weights()
    used, fresh = _policy(w), _policy(w)
    big = S.states(10, per_wave * waves * blocks // 81 + 1, 32)
    _run(used, big, x3)
    for E, N in ((3, 32), (2, 1), (5, 5)):
        st = S.states(11, E, N)
        got, want = _run(used, st, x3), _run(fresh, st, x3)
        for k in ("values", "att", "best", "best_val", "actions"):
            H.assert_bits_equal(got[k], want[k], "%s at E %d N %d" % (k, E, N))
        _check_finite_env(got, S.reference(w, st, 0, used._action_table), 0, used._action_table, "after the large batch")
        fresh = _policy(w)


# ------------------------------------------------------------------------------------------------ 5. query_env form
@X3
def test_query_env_form_takes_the_given_next_states_and_rewards(x3):
    """env_next of _lookahead: values = rewards + gamma_pow * V with V from the reference on the GIVEN next states --
    one of them exactly on the robot's next position for one action (distance feature 0) -- and the given rewards,
    NaN and -0.0 among them, in place of the reward ladder."""
    w = S.g5_weights()
    pol = _policy(w)
    table = pol._action_table
    A = len(table)
    N, E = 5, 9
    st = S.states(12, E, N)
    rng = np.random.RandomState(5)
    npos = np.stack([st.hpx, st.hpy], -1) + rng.uniform(-0.3, 0.3, (E, N, 2))
    nvel = rng.uniform(-1, 1, (E, N, 2))
    on = {}
    for e in range(0, E, 2):
        a, i = int(rng.randint(1, A)), int(rng.randint(N))
        npos[e, i] = (st.rpx[e] + table[a, 0] * S.DT, st.rpy[e] + table[a, 1] * S.DT)
        on[e] = (a, i)
    rew = rng.uniform(-0.25, 1.0, (E, A))
    rew[:, 7] = -0.0
    rew[1, :] = -0.0
    rew[2, 11] = np.nan
    rew[3, :] = np.nan
    rew[4, 0] = np.inf
    out = _run(pol, st, x3, env_next=(npos, nvel, rew))
    for e in range(E):
        ref = S.reference(w, st, e, table, nexts=(npos[e], nvel[e]), rewards=rew[e])
        if e in on:
            a, i = on[e]
            assert float(ref["feats"][a, i, 11]) == 0.0
        cls = S.classes(ref["values"])
        assert np.array_equal(S.classes(out["values"][e]), cls), e
        fin = cls == 0
        np.testing.assert_allclose(out["values"][e][fin], ref["values"][fin], rtol=0, atol=TOL, err_msg="env %d" % e)
        np.testing.assert_allclose(out["att"][e], ref["att"], rtol=0, atol=TOL)
        _check_argmax(out, e, table)
    assert np.isnan(out["values"][3]).all() and out["best"][3] == -1 and out["best"][4] == 0


# ------------------------------------------------------------------------------------------------ 6. argmax
def _argmax_table(A):
    rng = np.random.RandomState(A)
    ang, spd = rng.uniform(0, 2 * np.pi, A), rng.uniform(0.1, 1.0, A)
    table = np.stack([spd * np.cos(ang), spd * np.sin(ang)], 1)
    table[0] = 0.0
    return table


@X3
@pytest.mark.parametrize("A", S.ARGMAX_AS)
def test_argmax_on_exact_value_rows(A, x3):
    """sarl_argmax_kernel (shared with LSTM-RL and CADRL) on values that are exact: the network's V is exactly 0 and the
    query_env rewards are the values.  Equal maxima in one lane's scan (k, k + 64), in neighbouring lanes, across the
    halves of the merge and at the two ends: the lowest index wins; +inf; NaN before, after and between the maxima; all
    NaN and all -inf (no value wins: -1, -inf, the zero action); neighbouring subnormals.  The reference is the
    strict-'>' scan from -inf of multi_human_rl.py:53-55 in plain Python."""
    w = S.zero_value_network(S.g5_weights())
    table = _argmax_table(A)
    rows, names = S.argmax_rows(A)
    E, N = len(rows), 3
    pol = _policy(w, table=table)
    st = S.states(13, E, N)
    npos = np.stack([st.hpx + st.hvx * S.DT, st.hpy + st.hvy * S.DT], -1)
    nvel = np.stack([st.hvx, st.hvy], -1)
    out = _run(pol, st, x3, env_next=(npos, nvel, rows))
    want = rows + S.DISC * 0.0                                         # (-0.0 + 0.0 is +0.0, as on the device)
    H.assert_bits_equal(out["values"], want, "values (V == 0)")
    for e, name in enumerate(names):
        idx, top = S.scan_argmax(want[e])
        assert out["best"][e] == idx, (A, name, out["best"][e], idx)
        H.assert_bits_equal(out["best_val"][e], top, "best_val of %s" % name)
        act = table[idx] if idx >= 0 else (0.0, 0.0)
        assert tuple(out["actions"][e]) == tuple(act), (A, name)


@X3
def test_epsilon_one_explores_everywhere_but_on_the_goal(x3):
    """epsilon = 1: every env whose robot is not on its goal reports -2 and a row of the table; a robot on its goal
    reports -1 and the zero action whatever epsilon is."""
    w = S.g5_weights()
    pol = _policy(w)
    table = pol._action_table
    E = 64
    on_goal = (0, 9, 31, 63)
    st = S.states(14, E, 5, on_goal=on_goal)
    assert S.reached(st).nonzero()[0].tolist() == list(on_goal)
    for eps in (1.0, 0.0):
        out = _run(pol, st, x3, epsilon=eps)
        for e in range(E):
            if e in on_goal:
                assert out["best"][e] == -1 and tuple(out["actions"][e]) == (0.0, 0.0), (eps, e)
            elif eps == 1.0:
                assert out["best"][e] == -2, e
                assert (table == out["actions"][e]).all(1).any(), e
            else:
                _check_argmax(out, e, table)
    assert len({tuple(a) for a in out["actions"]}) > 1


# ------------------------------------------------------------------------------------------------ 7. feature edges
@X3
@pytest.mark.parametrize("kinematics", ["holonomic", "unicycle"])
def test_feature_edges(kinematics, x3):
    """dg == 0 (the action lands exactly on the goal: cr = 1, sr = 0), a human exactly on the robot's next position
    (distance feature 0), still humans, and for a unicycle the heading exactly on the goal bearing (theta feature 0)."""
    w = S.g5_weights()
    pol = _policy(w, kinematics=kinematics)
    table = pol._action_table
    seen = set()
    for N in (1, 5):
        st, kinds, act = S.feature_batch(N, table, kinematics)
        out = _run(pol, st, x3)
        skipped = 0
        for e, kind in enumerate(kinds):
            if S.reached(st)[e]:
                _check_argmax(out, e, table, reached=True)
                skipped += 1
                continue
            ref = S.reference(w, st, e, table, kinematics)
            a = int(act[e])
            f = ref["feats"][a].numpy()
            if kind == "on-goal":
                assert f[0, 0] == 0.0
            elif kind.startswith("human-on-next"):
                assert (f[:, 11] == 0.0).any()
            elif kind == "still-humans":
                assert np.all(f[:, 8:10] == 0.0)
            elif kind == "heading-on-bearing":
                assert f[0, 2] == 0.0 and f[0, 0] > 1.0
            seen.add(kind)
            _check_finite_env(out, ref, e, table, "%s N %d" % (kind, N))
        assert skipped * 8 <= len(kinds)
    assert seen >= {"on-goal", "human-on-next", "human-on-next-moving", "still-humans"}
    assert kinematics == "holonomic" or "heading-on-bearing" in seen
