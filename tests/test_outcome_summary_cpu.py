"""CPU: rollout.summarize_episodes, the one end of VecExplorer.run_k_episodes, the sequential Explorer.run_k_episodes and
DataGen.gen_data_from_explore_in_mix (explorer.py:126-151): counts, the mean navigation time with its time_limit
fallback, the three return shapes and the log lines, on hand-written lists."""
import logging

from modelcrowdnav_amd import _hip
from modelcrowdnav_amd.rollout import average, summarize_episodes

OK, HIT, LATE = _hip.INFO_REACHGOAL, _hip.INFO_COLLISION, _hip.INFO_TIMEOUT


def test_all_success():
    result, stats = summarize_episodes([0.5, 0.25, 0.75], [OK, OK, OK], [10.0, 12.0, 11.0], 3, 25.0)
    assert result == (0.5, 1.0, 0.0, 0.0)
    assert stats == dict(success=3, collision=0, timeout=0, avg_nav_time=11.0)


def test_no_success_falls_back_to_the_time_limit():
    result, stats = summarize_episodes([-0.25, 0.0], [HIT, LATE], [3.0, 25.0], 2, 25.0, returnNav=True)
    assert result == (-0.125, 0.0, 0.5, 0.5, 25.0)
    assert stats == dict(success=0, collision=1, timeout=1, avg_nav_time=25.0)


def test_mix_and_the_three_return_shapes():
    returns, infos, times = [0.5, -0.25, 0.0, 0.25], [OK, HIT, LATE, OK], [8.0, 2.5, 25.0, 9.0]
    rates, stats = summarize_episodes(returns, infos, times, 4, 25.0)
    assert rates == (0.125, 0.5, 0.25, 0.25)
    assert stats == dict(success=2, collision=1, timeout=1, avg_nav_time=8.5)
    assert summarize_episodes(returns, infos, times, 4, 25.0, returnNav=True)[0] == (0.125, 0.5, 0.25, 0.25, 8.5)
    counts = summarize_episodes(returns, infos, times, 4, 25.0, returnRate=False)[0]
    assert counts == (0.125, 2, 1, 1) and all(type(c) is int for c in counts[1:])
    # returnNav alone changes nothing: the reference only looks at it together with returnRate
    assert summarize_episodes(returns, infos, times, 4, 25.0, returnRate=False, returnNav=True)[0] == counts
    assert average([]) == 0


def test_log_lines(caplog):
    returns, infos, times = [0.5, -0.25, 0.0, 0.25], [OK, HIT, LATE, OK], [8.0, 2.5, 25.0, 9.5]
    kw = dict(print_failure=True, danger=(9, 1.35), time_step=0.25)
    with caplog.at_level(logging.INFO):
        summarize_episodes(returns, infos, times, 4, 25.0, phase="val", **kw)
    assert caplog.messages == [
        "VAL   has success rate: 0.50, collision rate: 0.25, nav time: 8.75, total reward: 0.1250",
        "Frequency of being in danger: 0.05 and average min separate distance in danger: 0.15",
        "Collision cases: 1",
        "Timeout cases: 2"]
    caplog.clear()
    with caplog.at_level(logging.INFO):                      # train: no danger line; the episode number in the phase line
        summarize_episodes(returns, infos, times, 4, 25.0, phase="train", episode=7, danger=(9, 1.35), time_step=0.25)
    assert caplog.messages == [
        "TRAIN in episode 7 has success rate: 0.50, collision rate: 0.25, nav time: 8.75, total reward: 0.1250"]
    caplog.clear()
    with caplog.at_level(logging.INFO):                      # stay: no phase line; the others as before
        summarize_episodes(returns, infos, times, 4, 25.0, phase="test", stay=True, **kw)
    assert caplog.messages == [
        "Frequency of being in danger: 0.05 and average min separate distance in danger: 0.15",
        "Collision cases: 1",
        "Timeout cases: 2"]
    caplog.clear()
    with caplog.at_level(logging.INFO):                      # no phase (DataGen logs its own line): nothing
        summarize_episodes(returns, infos, times, 4, 25.0)
    assert caplog.messages == []


def test_danger_line_without_danger_steps_divides_by_nothing(caplog):
    with caplog.at_level(logging.INFO):
        summarize_episodes([0.5], [OK], [8.0], 1, 25.0, phase="test", danger=(0, 0.0), time_step=0.25)
    assert caplog.messages[1] == "Frequency of being in danger: 0.00 and average min separate distance in danger: 0.00"
