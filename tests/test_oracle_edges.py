"""The oracle's edge-event counters (mcn_oracle_edge_counts, cport.edge_counts) and the edge-state generator
(tests/edge_states.py).  CPU only.

Each hand-made case below is one agent's ORCA solve on dyadic inputs (exact float32 arithmetic) and must move exactly
the counters listed for it: the event it was made for, plus the ones that event implies (a zero |w| in the collision
branch is also a NaN half-plane and a root of 0; a tangent line is also a root of 0).  The cases marked "searched"
come from a seeded search over random dyadic agents (parameters inlined).  The counters only count: a build of the
same source without them returns the same bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import cport
from tests import edge_states as ES

R = 0.3125          # (float)(0.3025 + 0.01)
Z = np.zeros((0, 2))

# name: (pos, vel, radius, max_speed, pref, other pos, other vel, other radius, kwargs, counters that move)
CASES = {
    "disc_zero_lp2": ((-1.25, -1.75), (0.125, 0.5), R, 0.5, (0.9375, -1.0), [(-1.375, -2.375)], [(0.4375, 0.5)], [R],
                      {}, {"disc_zero_lp2", "outside_fast_range"}),                                       # searched
    "disc_zero_lp3": ((0.25, -0.625), (0.0, 0.125), R, 0.75, (-1.875, 4.0),
                      [(-0.25, 0.375), (0.125, 0.625), (0.375, 0.5), (0.125, -0.625)],
                      [(-0.625, 0.4375), (0.125, -0.125), (-0.5625, -0.75), (0.0625, -0.1875)], [R] * 4,
                      {}, {"disc_zero_lp3", "outside_fast_range"}),                                       # searched
    "w_zero_collision": ((0.0, 0.0), (0.5, 0.0), R, 1.0, (0.5, 0.25), [(0.125, 0.0)], [(0.0, 0.0)], [R],
                         {}, {"w_zero_collision", "nonfinite_line", "outside_fast_range"}),    # rv == rp / timeStep
    "nonfinite_line": ((0.5, 0.25), (0.25, 0.5), R, 1.0, (0.5, 0.25), [(0.5, 0.25)], [(0.25, 0.5)], [R],
                       {}, {"nonfinite_line", "w_zero_collision", "outside_fast_range"}),   # coincident, same velocity
    "nonfinite_line_in_lp3": ((-0.25, -0.375), (0.9375, -0.625), R, 1.0, (-0.25, 0.8125),
                              [(-0.25, -0.375), (-0.375, -0.5)], [(0.9375, -0.625), (0.5625, -0.6875)], [R, R],
                              {}, {"nonfinite_line_in_lp3", "nonfinite_line", "w_zero_collision",
                                   "outside_fast_range"}),                          # searched: coincident, same velocity
    "parallel_lp1": ((1.875, -0.125), (0.5625, -0.0625), R, 0.5, (0.125, -0.625), [(-2.0, 1.125), (2.5, -1.5)],
                     [(0.625, -0.3125), (0.3125, 1.0)], [R, R], {}, {"parallel_lp1"}),                   # searched
    "parallel_same_lp3": ((-1.75, 1.875), (0.1875, 1.0), R, 0.5, (0.6875, 0.125),
                          [(2.375, 1.125), (-0.25, 1.25), (0.5, 1.25)], [(0.25, 0.25), (-0.5, -0.9375), (-0.625, 0.875)],
                          [R] * 3, {}, {"parallel_same_lp3"}),                                          # searched
    "parallel_opposite_lp3": ((0.5, 0.5), (-0.125, -0.625), R, 0.5, (-0.9375, 1.0),
                              [(-0.5, -0.125), (1.75, 2.25), (-1.375, 2.625)],
                              [(0.875, -0.3125), (-0.375, -0.625), (0.3125, 0.0625)], [R] * 3,
                              {}, {"parallel_opposite_lp3"}),                                           # searched
    "dist_tie": ((0.0, 0.0), (0.0, 0.0), R, 1.0, (0.5, 0.25), [(3.0, 0.0), (0.0, 3.0)], [(0.0, 0.0)] * 2, [R, R],
                 {}, {"dist_tie"}),
    "range_edge": ((0.0, 0.0), (0.0, 0.0), R, 1.0, (0.5, 0.25), [(6.0, 8.0)], [(0.0, 0.0)], [R], {}, {"range_edge"}),
    "tie_at_cut": ((0.0, 0.0), (0.0, 0.0), R, 1.0, (0.5, 0.25), [(3.0, 0.0), (0.0, 3.0)], [(0.0, 0.0)] * 2, [R, R],
                   {"max_neighbors": 1}, {"dist_tie", "tie_at_cut"}),
    "leg_det_zero": ((0.0, 0.0), (0.5, 0.0), R, 1.0, (0.5, 0.25), [(2.0, 0.0)], [(0.0, 0.0)], [R],
                     {}, {"leg_det_zero"}),                                          # w along rp, pointing away
    "pref_on_disc": ((0.0, 0.0), (0.0, 0.0), R, 1.0, (-1.0, 0.0), Z, Z, [], {}, {"pref_on_disc"}),
    "outside_fast_range": ((0.0, 0.0), (0.0, 0.0), R, 2.0 ** -60, (2.0 ** -55, 0.0), Z, Z, [], {},
                           {"outside_fast_range"}),                        # |pref|^2 = 2^-110: below sqrt5's range
}


def _solve(lib_solve, case):
    pos, vel, rad, ms, pref, op, ov, orad, kw, _ = case
    return lib_solve(pos, vel, rad, ms, pref, np.asarray(op, np.float64).reshape(-1, 2),
                     np.asarray(ov, np.float64).reshape(-1, 2), np.asarray(orad, np.float64), **kw)


def test_every_counter_has_a_hand_made_case():
    assert set(CASES) == set(cport.EDGE_NAMES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_each_case_moves_exactly_its_counters(name):
    cport.edge_counts(reset=True)
    _solve(cport.orca_agent, CASES[name])
    moved = {k for k, v in cport.edge_counts(reset=True).items() if v}
    assert name in moved
    assert moved == CASES[name][-1], moved
    # and nothing else counts in between: a solve on plain inputs moves no counter
    cport.orca_agent((0.0, 0.0), (0.1, 0.2), 0.31, 1.0, (0.3, 0.4), [(1.7, 0.3)], [(0.05, -0.2)], [0.31])
    assert not any(cport.edge_counts(reset=True).values())


def test_reset_flag():
    cport.edge_counts(reset=True)
    _solve(cport.orca_agent, CASES["range_edge"])
    assert cport.edge_counts(reset=False)["range_edge"] == 1
    assert cport.edge_counts(reset=True)["range_edge"] == 1
    assert cport.edge_counts(reset=True)["range_edge"] == 0


@pytest.fixture(scope="module")
def plain_oracle(tmp_path_factory):
    """The oracle compiled from the same source without the counters (-DMCN_ORACLE_NO_EDGE_COUNTS)."""
    here = os.path.dirname(os.path.abspath(cport.__file__))
    so = str(tmp_path_factory.mktemp("plain") / "libmcn_oracle_plain.so")
    subprocess.check_call(["make", "-s", "-C", here, "-B", "OUT=" + so,
                           "CFLAGS=-O2 -fPIC -std=c11 -ffp-contract=off -fno-fast-math -DMCN_ORACLE_NO_EDGE_COUNTS"],
                          stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    return lib


def _with_lib(lib, fn, *a, **kw):
    saved = cport._lib
    cport._lib = lib
    try:
        return fn(*a, **kw)
    finally:
        cport._lib = saved


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32)


def test_counters_do_not_change_any_result(plain_oracle):
    """Every hand-made case and every env of one edge batch per human-count family: the same bits with and without
    the counters (NaN included: the counters must not change which NaN comes out either)."""
    for name, case in CASES.items():
        a = _solve(cport.orca_agent, case)
        b = _with_lib(plain_oracle, _solve, cport.orca_agent, case)
        assert np.array_equal(_bits(a), _bits(b)), name
    for N, visible in ((5, False), (4, True), (10, True)):
        for variant in ES.ORCA_VARIANTS:
            st, ax, ay, _ = ES.edge_batch(N, visible, variant)
            cfg = ES.oracle_cfg(visible, variant)
            sa, sb = st.copy(), st.copy()
            ra = cport.env_step(cfg, sa, ax, ay, update=True)
            rb = _with_lib(plain_oracle, cport.env_step, cfg, sb, ax, ay, update=True)
            for k in ra:
                assert np.array_equal(np.asarray(ra[k]).view(np.uint8), np.asarray(rb[k]).view(np.uint8)), (N, k)
            for k in ES._fields():
                assert np.array_equal(getattr(sa, k).view(np.uint8), getattr(sb, k).view(np.uint8)), (N, k)


@pytest.mark.parametrize("family", [(1, 2, 3, 4, 5), (6, 7, 8, 9, 10)])
def test_edge_batches_reach_every_counter(family):
    """The generated batches (every N of the family, robot visible and not, every ORCA variant) reach every counted
    event: if a change of the generator or of the oracle loses one, this fails instead of the GPU tests quietly
    covering less."""
    total = dict.fromkeys(cport.EDGE_NAMES, 0)
    for N in family:
        for visible in (False, True):
            for variant in ES.ORCA_VARIANTS:
                st, ax, ay, names = ES.edge_batch(N, visible, variant)
                assert st.E == len(names) == len(ax) and st.E % 2 == 1
                cport.edge_counts(reset=True)
                cport.env_step(ES.oracle_cfg(visible, variant), st, ax, ay, update=False)
                for k, v in cport.edge_counts(reset=True).items():
                    total[k] += v
    missing = [k for k, v in total.items() if v == 0]
    assert not missing, total


def test_edge_batches_are_the_recorded_ones(golden_dir):
    """edge_batch(N, visible, variant) returns the arrays and names it returned when tests/golden/edge_batch_sha256.json
    was recorded (before the supplement was added): other tests pick envs by block name and hold step ranges found on
    these scenes (tests/test_rollout_chain_gpu.py, tests/closed_loop_states.py), so the blocks must not move."""
    import hashlib
    import json
    with open(os.path.join(golden_dir, "edge_batch_sha256.json")) as f:
        want = json.load(f)
    assert len(want) == 10 * 2 * len(ES.ORCA_VARIANTS)
    for key in sorted(want):
        N, visible, vidx = (int(x) for x in key.split("-"))
        st, ax, ay, names = ES.edge_batch(N, bool(visible), ES.ORCA_VARIANTS[vidx])
        h = hashlib.sha256()
        for v in [getattr(st, k) for k in ES._fields()] + [ax, ay]:
            h.update(np.ascontiguousarray(v, dtype=np.float64).tobytes())
        h.update("|".join(names).encode())
        assert h.hexdigest() == want[key], key


def test_parallel_same_lp3_supplement():
    """Every env of the supplement moves parallel_same_lp3 on its first step, whichever human slot holds the agent, and
    nothing else; edge_batch(5, False, .) reaches it under no variant the quad kernels take (why the supplement exists)."""
    st, ax, ay, names = ES.lp3_parallel_supplement()
    assert st.E == ES.SUPPLEMENT == len(names) == len(ax) == 8 and st.N == 5
    for e in range(st.E):
        cport.edge_counts(reset=True)
        cport.env_step(ES.oracle_cfg(False), ES.take(st, [e]), ax[e:e + 1], ay[e:e + 1], update=False)
        moved = {k: v for k, v in cport.edge_counts(reset=True).items() if v}
        assert moved == {"parallel_same_lp3": 1}, (e, moved)
    for variant in ES.WG4_VARIANTS:
        b = ES.edge_batch(5, False, variant)
        cport.edge_counts(reset=True)
        cport.env_step(ES.oracle_cfg(False, variant), b[0], b[1], b[2], update=False)
        assert cport.edge_counts(reset=True)["parallel_same_lp3"] == 0, variant
    both = ES.with_supplement(ES.edge_batch(5, False))
    assert both[0].E == 629 + 8 == len(both[3]) == len(both[1]) and both[0].E % 8 == 5
    assert both[3][:629] == ES.edge_batch(5, False)[3]


def test_four_wavefront_inputs_reach_every_event():
    """The four-wavefront rollout form runs one shape only (5 humans, robot invisible, max_neighbors >= 4), so its GPU
    tests have no other human count to borrow an event from.  Its inputs alone -- edge_batch(5, False, .) under the three
    variants it takes plus the supplement, and ladder_batch(5, False, ., .) -- reach all 13 quad ORCA events on the first
    step, all 16 rung events, and with a unicycle robot the two heading events as well."""
    from tests.kernel_paths import QUAD_EVENTS, STEP_EVENTS, UNICYCLE_EVENTS, ladder_configs
    from tests import ladder_states as LS
    assert ES.WG4_VARIANTS == ({}, {"neighbor_dist": 1.5}, {"safety_space": 0.0625})
    total = dict.fromkeys(cport.EDGE_NAMES, 0)
    for variant in ES.WG4_VARIANTS:
        batch = ES.edge_batch(5, False, variant)
        st, ax, ay, names = ES.with_supplement(batch) if not variant else batch
        cport.edge_counts(reset=True)
        cport.env_step(ES.oracle_cfg(False, variant), st, ax, ay, update=False)
        for k, v in cport.edge_counts(reset=True).items():
            total[k] += v
    assert len(QUAD_EVENTS) == 13
    missing = [k for k in QUAD_EVENTS if total[k] == 0]
    assert not missing, total
    assert total["tie_at_cut"] == 0          # no cut of the neighbour list with max_neighbors >= 4 candidates
    for unicycle, events in ((False, STEP_EVENTS), (True, UNICYCLE_EVENTS)):
        total = {}
        sizes = []
        for N, visible, dd, count_hh in ladder_configs([5], True):
            assert not visible
            st, ax, ay, _, names = LS.ladder_batch(N, visible, dd, unicycle)
            sizes.append(st.E)
            cport.ladder_counts(reset=True)
            cport.env_step(LS.cfg(visible, dd, count_hh, unicycle), st, ax, ay, update=True)
            for k, v in cport.ladder_counts(reset=True).items():
                total[k] = total.get(k, 0) + v
        assert sizes == [341, 373]           # ragged against workgroups of 8 envs
        missing = [k for k in events if total.get(k, 0) == 0]
        assert not missing, (unicycle, total)
    assert len(STEP_EVENTS) == 16 and len(UNICYCLE_EVENTS) == 18


def test_edge_batches_are_dyadic_and_deterministic():
    st, ax, ay, names = ES.edge_batch(5, True)
    st2, ax2, ay2, _ = ES._build_batch(5, True, {}, 0)
    for k in ES._fields():
        assert np.array_equal(getattr(st, k), getattr(st2, k)), k
    # positions and goals on the 1/8 grid, velocities and actions on the 1/16 grid, float32-exact below 2^20
    for k in ("hpx", "hpy", "hgx", "hgy", "rpx", "rpy"):
        v = getattr(st, k)
        assert np.array_equal(v * 8, np.round(v * 8)), k
    for v in (st.hvx, st.hvy, ax, ay):
        assert np.array_equal(v * 16, np.round(v * 16))
    assert np.float32(ES.HR + 0.01) == 0.3125 and np.float32(ES.HR + 0.01 + 0.0625) == 0.375
