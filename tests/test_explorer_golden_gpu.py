"""The batched VecExplorer against g15_explorer.npz = the REAL reference's Explorer.run_k_episodes
(crowd_nav/utils/explorer.py:36-151) on the reference CrowdSim: returned statistics, replay-memory contents (imitation
learning with the ORCA demonstrator, RL value targets with a SARL robot and a target network) and the data-collection
side channels (raw_memory rows, world-model pairs, SGAN cache files).  The reference's ORCA humans were solved by the
rvo2 stand-in (= the C oracle): plumbing pinned, solver unpinned."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H  # noqa: E402


def _sarl(g, pref, dev, phase):
    from tests.lookahead_harness import policy, weights
    p = policy("sarl", weights(g, pref), phase=phase)
    assert p.device == dev
    p.multiagent_training = True
    return p


def _check_memory(mem, g, tag, ordered):
    """Memory rows against the reference's: same order when the batched explorer plays one env (its (env, time) order is
    then the reference's (episode, time) order); otherwise matched one to one by nearest state."""
    want_s, want_v = g[tag + "_mem_states"], g[tag + "_mem_values"]
    assert len(mem) == want_s.shape[0] > 0
    got_s = mem._states[:len(mem)].cpu().numpy()
    got_v = mem._values[:len(mem), 0].cpu().numpy()
    if not ordered:
        a, b = got_s.reshape(len(mem), -1), want_s.reshape(len(mem), -1)
        used, match = np.zeros(len(mem), bool), []
        for row in b:                                               # nearest row not taken yet (a fixed test_case
            d = np.abs(a - row).max(1)                              # repeats whole episodes)
            d[used] = np.inf
            match.append(int(d.argmin()))
            used[match[-1]] = True
        match = np.array(match)
        got_s, got_v = got_s[match], got_v[match]
    # states: float32 rotate() on another device: atan2 / cos / sin differ in the last place, which moves a rotated
    # coordinate of magnitude m by a few 1e-7 * m (seen: 2.1e-6 at 2.1); values: float32 sums
    np.testing.assert_allclose(got_s, want_s, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(got_v, want_v, rtol=0, atol=2e-6)


@pytest.mark.parametrize("E", [1, 4])
@pytest.mark.parametrize("tag,phase,k,kw", [("il_val", "val", 12, dict(returnNav=True)),
                                            ("il_train", "train", 9, dict(returnRate=False)),
                                            ("il_fixed_case", "test", 3, dict(test_case=3, returnNav=True))])
def test_imitation_learning_collection_matches_reference(tag, phase, k, kw, E, golden_dir):
    """train.py:150-160: the ORCA demonstrator (safety_space 0.15) drives, states are transformed by the target policy,
    values are discounted tail sums; only ReachGoal / Collision episodes feed the memory."""
    import torch
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.rollout import VecExplorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    dev = torch.device("cuda", 0)
    env = H.make_vec_env(E, 5)
    env.track_human_times = False; env.export_human_actions = False
    orca = policy_factory["orca"]()
    orca.multiagent_training = True
    orca.safety_space = 0.15
    env.robot.set_policy(orca)
    mem = ReplayMemory(100000, device=dev)
    ex = VecExplorer(env, env.robot, gamma=0.9, policy=orca, memory=mem, target_policy=_sarl(g, "target_w__", dev, "test"))
    out = ex.run_k_episodes(k, phase, update_memory=True, imitation_learning=True, **kw)
    want = g[tag + "_out"]
    assert len(out) == len(want) and tuple(out[1:]) == tuple(want[1:]), (out, want)
    assert abs(out[0] - want[0]) < 1e-12
    assert env.case_counter[phase] == int(g[tag + "_counter"])
    _check_memory(mem, g, tag, ordered=True)


@pytest.mark.parametrize("E", [1, 3])
def test_sarl_robot_with_rl_value_targets_matches_reference(E, golden_dir):
    """Greedy SARL robot in the train phase (epsilon 0), value targets r + gamma_bar * target_model(next state): the
    chosen actions decide the trajectories, so the returned statistics hold only if every look-ahead picks the
    reference's action (float32 value network on another device, strict-> argmax)."""
    import torch
    from modelcrowdnav_amd.rollout import VecExplorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    dev = torch.device("cuda", 0)
    env = H.make_vec_env(E, 5)
    env.track_human_times = False; env.export_human_actions = False
    sarl = _sarl(g, "sarl_w__", dev, "train")
    sarl.set_epsilon(0.0)
    env.robot.set_policy(sarl)
    sarl.set_env(env)
    mem = ReplayMemory(100000, device=dev)
    ex = VecExplorer(env, env.robot, gamma=0.9, policy=sarl, memory=mem)
    ex.update_target_model(_sarl(g, "target_w__", dev, "test").model)
    out = ex.run_k_episodes(6, "train", update_memory=True, imitation_learning=False, returnNav=True)
    want = g["sarl_train_out"]
    assert tuple(out[1:]) == tuple(want[1:]), (out, want)
    assert abs(out[0] - want[0]) < 1e-9
    _check_memory(mem, g, "sarl_train", ordered=True)


@pytest.mark.parametrize("E", [1, 4, 3])
@pytest.mark.parametrize("tag,stay", [("collect_stay", True), ("collect_orca", False)])
def test_data_collection_matches_reference(tag, stay, E, golden_dir, tmp_path):
    """explorer.py:60-85,112-121: raw_memory rows in episode order, world-model pairs of the steps where somebody
    moves, one SGAN text file per episode -- byte for byte what the reference wrote."""
    import torch
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.rollout import VecExplorer
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    env = H.make_vec_env(E, 5)
    env.track_human_times = False; env.export_human_actions = False
    orca = policy_factory["orca"]()
    orca.multiagent_training = True
    env.robot.set_policy(orca)
    ex = VecExplorer(env, env.robot, gamma=0.9, policy=orca)
    ex.raw_memory, ex.rawob = [], []
    out = ex.run_k_episodes(4, "val", stay=stay, update_raw_ob=True, cacheFile=str(tmp_path), returnNav=True)
    want = g[tag + "_out"]
    assert tuple(out[1:]) == tuple(want[1:]) and abs(out[0] - want[0]) < 1e-12, (out, want)
    assert len(ex.raw_memory) == g[tag + "_raw_ob"].shape[0]
    assert np.array_equal(np.stack([r[0] for r in ex.raw_memory]), g[tag + "_raw_ob"])
    assert np.array_equal(np.array([r[1] for r in ex.raw_memory]), g[tag + "_raw_reward"])
    assert np.array_equal(np.array([r[2] for r in ex.raw_memory], np.uint8), g[tag + "_raw_done"])
    assert np.array_equal(np.array([r[3] for r in ex.raw_memory], np.int32), g[tag + "_raw_info"])
    assert len(ex.rawob) == g[tag + "_pairs_cur"].shape[0]
    assert np.array_equal(torch.stack([p[0] for p in ex.rawob]).numpy(), g[tag + "_pairs_cur"])
    assert np.array_equal(torch.stack([p[1] for p in ex.rawob]).numpy(), g[tag + "_pairs_next"])
    for i in range(1, 5):
        assert open(tmp_path / ("%d.txt" % i)).read() == str(g["%s_cache%d" % (tag, i)]), i


# ---- the same fixtures through the DROP-IN class: crowd_nav.utils.explorer.Explorer on the E = 1 gym env, which hands
# ---- k > 1 episodes to the batched VecExplorer (utils/explorer.py); what the reference's drivers actually call

def _dropin_env_and_robot(policy):
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.envs import CrowdSim
    from modelcrowdnav_amd.envs.utils.robot import Robot
    cfg = configs.env_config(**{"sim.human_num": 5})
    env = CrowdSim()
    env.configure(cfg)
    robot = Robot(cfg, "robot")
    robot.set_policy(policy)
    env.set_robot(robot)
    return env, robot


@pytest.mark.parametrize("cap", [4096, 4])
@pytest.mark.parametrize("tag,phase,k,kw", [("il_val", "val", 12, dict(returnNav=True)),
                                            ("il_train", "train", 9, dict(returnRate=False)),
                                            ("il_fixed_case", "test", 3, dict(test_case=3, returnNav=True))])
def test_dropin_explorer_imitation_learning_matches_reference(tag, phase, k, kw, cap, golden_dir):
    """train.py:150-167 as the reference writes it: Explorer(env, robot, device, memory, gamma, target_policy) on the
    gym env, run_k_episodes(k, ..., update_memory=True, imitation_learning=True).  Statistics exact, the memory rows in
    the reference's (episode, time) ORDER -- also when an env plays several episodes (cap = 4)."""
    import torch
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.utils.explorer import Explorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    dev = torch.device("cuda", 0)
    orca = policy_factory["orca"]()
    orca.multiagent_training = True
    orca.safety_space = 0.15
    env, robot = _dropin_env_and_robot(orca)
    mem = ReplayMemory(100000, device=dev)
    ex = Explorer(env, robot, dev, mem, 0.9, target_policy=_sarl(g, "target_w__", dev, "test"))
    ex.max_batch_envs = cap
    out = ex.run_k_episodes(k, phase, update_memory=True, imitation_learning=True, **kw)
    assert ex.last_run_batched
    want = g[tag + "_out"]
    assert len(out) == len(want) and tuple(out[1:]) == tuple(want[1:]), (out, want)
    assert abs(out[0] - want[0]) < 1e-12
    assert env.case_counter[phase] == int(g[tag + "_counter"])          # the E = 1 env's own counter advanced
    _check_memory(mem, g, tag, ordered=True)


@pytest.mark.parametrize("cap", [4096, 3])
def test_dropin_explorer_sarl_robot_rl_targets_match_reference(cap, golden_dir):
    """train.py:188 / 249-style evaluation and memory fill with a greedy SARL robot (epsilon 0) and a target network."""
    import torch
    from modelcrowdnav_amd.utils.explorer import Explorer
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    dev = torch.device("cuda", 0)
    sarl = _sarl(g, "sarl_w__", dev, "train")
    sarl.set_epsilon(0.0)
    env, robot = _dropin_env_and_robot(sarl)
    sarl.set_env(env)
    mem = ReplayMemory(100000, device=dev)
    ex = Explorer(env, robot, dev, mem, 0.9)
    ex.max_batch_envs = cap
    ex.update_target_model(_sarl(g, "target_w__", dev, "test").model)
    out = ex.run_k_episodes(6, "train", update_memory=True, imitation_learning=False, returnNav=True)
    assert ex.last_run_batched
    want = g["sarl_train_out"]
    assert tuple(out[1:]) == tuple(want[1:]), (out, want)
    assert abs(out[0] - want[0]) < 1e-9
    _check_memory(mem, g, "sarl_train", ordered=True)
    # exploration on numpy's shared stream and single episodes stay on the sequential path
    sarl.set_epsilon(0.5)
    assert ex._batched_reason(6, "train", True, False, False) is not None
    assert ex._batched_reason(1, "val", False, False, False) == "k = 1"
    assert ex._batched_reason(6, "val", False, False, False) is None


@pytest.mark.parametrize("cap", [4096, 3])
@pytest.mark.parametrize("tag,stay", [("collect_stay", True), ("collect_orca", False)])
def test_dropin_explorer_data_collection_matches_reference(tag, stay, cap, golden_dir, tmp_path):
    """explorer.py:60-85,112-121 through the drop-in class: raw rows, world-model pairs and cache files byte for byte."""
    import torch
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.utils.explorer import Explorer
    g = np.load(os.path.join(golden_dir, "g15_explorer.npz"))
    orca = policy_factory["orca"]()
    orca.multiagent_training = True
    env, robot = _dropin_env_and_robot(orca)
    ex = Explorer(env, robot, torch.device("cuda", 0), gamma=0.9)
    ex.max_batch_envs = cap
    ex.raw_memory, ex.rawob = [], []
    out = ex.run_k_episodes(4, "val", stay=stay, update_raw_ob=True, cacheFile=str(tmp_path), returnNav=True)
    assert ex.last_run_batched
    want = g[tag + "_out"]
    assert tuple(out[1:]) == tuple(want[1:]) and abs(out[0] - want[0]) < 1e-12, (out, want)
    # rows carry the reference's value types (explorer.py:80-81): list[ObservableState], float, bool, Info object
    from modelcrowdnav_amd.envs.utils import info as I
    from modelcrowdnav_amd.envs.utils.state import ObservableState
    assert all(isinstance(h, ObservableState) for h in ex.raw_memory[0][0]) and isinstance(ex.raw_memory[0][3], I._Outcome)
    rows_ob = np.array([[[h.px, h.py, h.vx, h.vy, h.radius] for h in r[0]] for r in ex.raw_memory])
    assert np.array_equal(rows_ob, g[tag + "_raw_ob"])
    assert np.array_equal(np.array([r[1] for r in ex.raw_memory]), g[tag + "_raw_reward"])
    assert np.array_equal(np.array([r[2] for r in ex.raw_memory], np.uint8), g[tag + "_raw_done"])
    assert np.array_equal(np.array([r[3].code for r in ex.raw_memory], np.int32), g[tag + "_raw_info"])
    assert all(r[3].min_dist < 0.2 for r in ex.raw_memory if isinstance(r[3], I.Danger))
    assert np.array_equal(torch.stack([p[0] for p in ex.rawob]).numpy(), g[tag + "_pairs_cur"])
    assert np.array_equal(torch.stack([p[1] for p in ex.rawob]).numpy(), g[tag + "_pairs_next"])
    for i in range(1, 5):
        assert open(tmp_path / ("%d.txt" % i)).read() == str(g["%s_cache%d" % (tag, i)]), i
