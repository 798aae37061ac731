"""CPU: the inputs of tests/test_orca_finish_edges_gpu.py are worth running.  The host replay of every edge batch
(tests/orca_finish_states.py) reaches the oracle's edge counters its config can reach, the boundary batches reach every
event of the float64 half, each named boundary case behaves as include/mcn.h says (worked out by hand in
orca_finish_states._case_table), and the replay's steps 5 and 6 agree with a second restatement written from the header
alone, so that the yardstick of the GPU test is not only checked against itself."""
import math
import struct

import numpy as np
import pytest

from oracle import cport
from tests import orca_finish_ref as R
from tests import orca_finish_states as S


def test_configs_cover_the_parameters_and_the_wavefront_layouts():
    mns, nds, ths, dts = (set(c[i] for c in S.CONFIGS) for i in range(4))
    assert mns == {10, 3, 2, 0} and nds == {10.0, 1.5} and ths == {5.0, 2.0} and dts == {0.25, 0.1}
    assert S.CONFIGS[S.DEFAULT] == (10, 10.0, 5.0, 0.25) and (3, 1.5, 2.0, 0.1) in S.CONFIGS
    assert float(np.float32(0.1)) != 0.1 and float(np.float32(0.25)) == 0.25
    A = [N + 1 for N in S.HUMAN_COUNTS]
    assert A == [2, 3, 4, 6, 8, 11, 16, 21, 22, 32, 33]
    assert [a for a in range(2, 34) if 64 % a == 0] == [2, 4, 8, 16, 32]          # no idle lanes: all of them are run
    assert 64 // 21 == 3 and 64 - 3 * 21 == 1 and 64 // 22 == 2 and 64 // 33 == 1
    for N in S.HUMAN_COUNTS:                       # every (N, config) is run: each N meets a cut and the defaults
        assert any(mn < N for mn, _, _, _ in S.CONFIGS)
        st, vel, names = S.edge_batch(N, S.DEFAULT)
        assert len(names) == st["hrad"].shape[0] == vel.shape[0] and st["hrad"].shape[1] == N


@pytest.mark.parametrize("config", range(len(S.CONFIGS)))
def test_edge_replays_reach_every_required_counter(config):
    """Summed over HUMAN_COUNTS, as tests/test_oracle_edges.py::test_edge_batches_reach_every_counter does; the cut of
    the neighbour list falls on a tie for every N > max_neighbors >= 2, every N enters the 3-D LP and meets the tangent
    line of the 2-D LP unless max_neighbors is 0, and no replay puts out a NaN."""
    mn = S.CONFIGS[config][0]
    total = dict.fromkeys(cport.EDGE_NAMES, 0)
    for N in S.HUMAN_COUNTS:
        ref, counts, lp3 = S.edge_replay(N, config)
        for k, v in counts.items():
            total[k] += v
        if mn > 0:
            assert lp3 > 0 and counts["disc_zero_lp2"] > 0, (N, lp3, counts)
        else:
            assert lp3 == 0
        if N > mn >= 2:
            assert counts["tie_at_cut"] > 0, (N, counts)
        assert ref["steps"].max() == S.T_EDGE and (N > 10 or ref["steps"].min() < S.T_EDGE)     # envs stop apart
        for k in ("sim_vel", "hpos", "rpos", "gtime", "human_times"):
            assert not np.isnan(ref[k]).any(), (N, k)
        assert not any(np.isnan(rows).any() for rows in ref["traj"]), N
    missing = [k for k in S.REQUIRED[config] if total[k] == 0]
    assert not missing, total


def test_required_counters_are_all_of_them_but_for_the_empty_neighbour_list():
    for (mn, _, _, _), req in zip(S.CONFIGS, S.REQUIRED):
        assert set(req) == (set(cport.EDGE_NAMES) if mn > 0 else {"pref_on_disc"})


def test_events_argument_changes_no_result():
    st, vel, names, select = S.boundary_batch(2)
    a = R.replay(st, vel, select=select, max_steps=3, time_step=0.1)
    b = R.replay(st, vel, select=select, max_steps=3, time_step=0.1, events={})
    for k in ("hpos", "rpos", "gtime", "human_times", "sim_vel", "steps"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["traj"], b["traj"]))


@pytest.mark.parametrize("time_step", S.BOUNDARY_TIME_STEPS)
@pytest.mark.parametrize("N", S.BOUNDARY_COUNTS)
def test_boundary_batch_reaches_every_event_and_behaves_as_the_header_says(N, time_step):
    ref, events = S.boundary_replay(N, time_step)
    st, vel, names, select = S.boundary_batch(N)
    missing = [k for k in R.EVENT_NAMES if events[k] == 0]
    assert not missing, events
    assert len(set(names)) == len(names) == len(events["per_env"])
    per = dict(zip(names, events["per_env"]))
    # each case moves the counter it was made for
    for name, ev in (("arrival-touch", "arrival_touch"), ("arrival-below", "arrival"), ("arrival-before-move", "arrival_after_move"),
                     ("arrival-f64-entry/f64-only", "arrival_f64_only"), ("arrival-f64-entry/f32-only", "arrival_f32_only"),
                     ("pref-unit/axis", "pref_unit"), ("pref-unit/triple", "pref_unit"), ("pref-above/axis", "pref_ulp_above"),
                     ("pref-above/triple", "pref_ulp_above"), ("pref-below", "pref_zero"), ("times-odd/neg-zero-0", "neg_zero_pending"),
                     ("times-odd/all-set-2", "odd_only_env"), ("times-odd/one-zero-1", "odd_time_kept"), ("clock/2^53", "clock_absorbed"),
                     ("select-values/0", "unselected_env"), ("select-values/2", "select_other_byte"),
                     ("select-values/255", "select_other_byte"), ("radius-rounding", "arrival_rad64_only")):
        assert per[name][ev] > 0, (name, per[name])
    assert per["clock/1e6+0.1"]["clock_rounded"] == (3 if time_step == 0.1 else 0)
    assert per["arrival-touch"]["arrival_f64_only"] == per["arrival-touch"]["arrival_f32_only"] == 0
    kept = set()
    for e, name in enumerate(names):
        if name.startswith("times-odd"):
            kept |= {struct.pack("<d", x) for x in st["human_times"][e] if x != 0}
    assert kept == {struct.pack("<d", x) for x in S.ODD_TIMES}
    # the exact construction
    e = names.index("arrival-touch")
    d = st["hpos"][e, 0] - st["hgoal"][e, 0]
    assert math.sqrt(d[0] * d[0] + d[1] * d[1]) == st["hrad"][e, 0] == 0.3125
    assert st["hrad"][names.index("arrival-below"), 0] == 0.3125 + 2.0 ** -54
    for name, i in (("arrival-f64-entry/f64-only", 0), ("arrival-f64-entry/f32-only", 1)):
        p = st["hpos"][names.index(name), i]
        assert not np.array_equal(p, p.astype(np.float32).astype(np.float64)) and p.min() > 2.0 ** 10
    assert float(np.float32(0.35)) != 0.35 and float(np.float32(0.8)) != 0.8
    S.assert_boundary_cases(ref, N, time_step, "replay")


def _steps_5_and_6(pos, goal, rad, times, gtime, rows, time_step, max_steps):
    """include/mcn.h, mcn_orca_finish, steps 4-6 and the loop condition in plain Python floats; steps 1-3 are not
    restated: rows[s] holds the float32 positions after step s."""
    times, steps = list(times), 0
    while any(x == 0 for x in times) and steps < max_steps:
        gtime = gtime + time_step
        for i in range(len(times)):
            dx, dy = pos[i][0] - goal[i][0], pos[i][1] - goal[i][1]
            if times[i] == 0 and math.sqrt(dx * dx + dy * dy) < rad[i]:
                times[i] = gtime
        pos = [(float(x), float(y)) for x, y in rows[steps]]
        steps += 1
    return pos, times, gtime, steps


@pytest.mark.parametrize("time_step", S.BOUNDARY_TIME_STEPS)
@pytest.mark.parametrize("N", S.BOUNDARY_COUNTS)
def test_replay_agrees_with_a_second_restatement_of_steps_5_and_6(N, time_step):
    ref, _ = S.boundary_replay(N, time_step)
    st, vel, names, select = S.boundary_batch(N)
    pack = lambda xs: [struct.pack("<d", float(x)) for x in xs]
    seen = 0
    for e, name in enumerate(names):
        if not select[e]:
            assert ref["steps"][e] == 0
            continue
        seen += name.startswith(("times-odd", "arrival-"))
        pos, times, gtime, steps = _steps_5_and_6(
            [tuple(map(float, p)) for p in st["hpos"][e]], [tuple(map(float, g)) for g in st["hgoal"][e]],
            [float(r) for r in st["hrad"][e]], [float(t) for t in st["human_times"][e]], float(st["gtime"][e]),
            [rows[1:] for rows in ref["traj"][e]], time_step, S.BOUNDARY_STEPS)
        assert steps == ref["steps"][e] == len(ref["traj"][e]), name
        assert pack(times) == pack(ref["human_times"][e]), (name, times, ref["human_times"][e])
        if steps:
            assert pack([gtime]) == pack([ref["gtime"][e]]), name
            assert pack(np.ravel(pos)) == pack(np.ravel(ref["hpos"][e])), name
    assert seen == 5 + 12
