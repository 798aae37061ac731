"""CPU: rollout.episode_plan -- the host arithmetic that says which pool row every env plays in every round -- replayed
with the kernel's documented restart rule (include/mcn.h, mcn_rollout: round 0 is the loaded row; every restart takes
the env's next_case and then advances it by case_stride modulo pool_size).  The grid covers counters that wrap, pools
smaller and larger than the case list, partial last rounds and uneven shards; it is also what shows that the row step
between rounds is one constant for every input, so run_k_episodes needs no second pool layout."""
import numpy as np

from modelcrowdnav_amd import dist as mdist
from modelcrowdnav_amd.rollout import episode_plan


def _grid():
    for size in (1, 2, 5, 7, 100):
        firsts = range(size) if size < 100 else (0, 1, 90, 97, 99)
        for first in firsts:
            for E_total in (1, 2, 3, 8):
                for ws in (1, 2, 3):
                    if E_total < ws:
                        continue
                    for k in range(1, 3 * E_total + 2):
                        for test_case in [None] + sorted({0, size - 1}):
                            yield size, first, E_total, ws, k, test_case


def _replay(plan):
    """[E_local, rounds] pool rows the kernel plays: the loaded row, then next_case advanced by the stride."""
    rows = np.empty_like(plan.mine)
    nxt = np.array(plan.next_case)
    for e in range(rows.shape[0]):
        rows[e, 0] = plan.mine[e, 0]
        for r in range(1, plan.rounds):
            rows[e, r] = nxt[e]
            nxt[e] = (nxt[e] + plan.stride) % plan.pool_size
    return rows


def _check(size, first, E_total, ws, k, test_case, contiguous):
    what = "size %d first %d E %d ws %d k %d test_case %r contiguous %r" % (size, first, E_total, ws, k, test_case,
                                                                            contiguous)
    seen = set()
    for rank in range(ws):
        lo, hi = mdist.shard(E_total, rank, ws)
        plan = episode_plan(first, size, k, E_total, lo, hi - lo, test_case, contiguous_pool=contiguous)
        rounds = plan.rounds
        assert rounds == -(-k // E_total) and len(plan.cases) == rounds * E_total, what
        assert plan.fin_slots == max(rounds, 2), what
        assert 0 <= plan.stride < plan.pool_size and plan.mine.shape == (hi - lo, rounds), what
        # the pool row -> case map of either layout
        case_of_row = {(c - plan.uniq[0] if contiguous else j): c for j, c in enumerate(plan.uniq)}
        assert plan.pool_size == (plan.uniq[-1] - plan.uniq[0] + 1 if contiguous else len(plan.uniq)), what
        # the step between rounds is one constant for every env and round
        steps = np.diff(plan.mine, axis=1) % plan.pool_size
        assert (steps == plan.stride).all(), what
        rows = _replay(plan)
        assert ((rows >= 0) & (rows < plan.pool_size)).all(), what
        for g in range(k):
            e, r = g % E_total, g // E_total
            if lo <= e < hi:
                want = test_case if test_case is not None else (first + g) % size
                assert case_of_row[int(rows[e - lo, r])] == want, "%s: episode %d" % (what, g)
                seen.add(g)
        # the "too close" counters cover `rounds` episodes of exactly the envs whose last round is one of the k
        full = [e for e in range(lo, hi) if (rounds - 1) * E_total + e < k]
        assert full == list(range(lo, lo + plan.n_full)), what
        assert plan.danger_short_from == (0 if plan.n_full == hi - lo else plan.n_full + 1), what
    assert seen == set(range(k)), what


def test_plan_reaches_every_case_by_the_kernels_restart_rule():
    n = 0
    for size, first, E_total, ws, k, test_case in _grid():
        _check(size, first, E_total, ws, k, test_case, contiguous=False)
        if test_case is None:                       # device scenarios take no test_case
            _check(size, first, E_total, ws, k, None, contiguous=True)
        n += 1
    assert n > 5000


def test_vec_explorer_case_counter_wraps_mid_run():
    """The case of tests/test_rollout_gpu.py's test of that name: the counter starts at 90 of 100 cases, 20 episodes
    over 8 envs -- three rounds whose cases wrap from 99 to 0 inside the second."""
    _check(100, 90, 8, 1, 20, None, contiguous=False)
    _check(100, 90, 8, 1, 20, None, contiguous=True)
    plan = episode_plan(90, 100, 20, 8, 0, 8)
    assert plan.rounds == 3 and plan.uniq == list(range(14)) + list(range(90, 100))
    assert plan.pool_size == 24 and plan.stride == 8 and plan.n_full == 4 and plan.danger_short_from == 5
    assert plan.mine[:, 0].tolist() == list(range(14, 22))          # cases 90..97 sit after the wrapped 0..13
    assert plan.next_case.tolist() == [22, 23, 0, 1, 2, 3, 4, 5]
