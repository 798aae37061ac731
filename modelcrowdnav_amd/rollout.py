"""Batched Explorer: run k evaluation episodes over E environments resident in HBM
(reference: crowd_nav/utils/explorer.py:36-151, run_k_episodes).

The reference loop is `for i in range(k): ob = env.reset(); while not done: a = robot.act(ob);
ob, r, done, info = env.step(a)`.  Here episode i runs in env (i mod E): every env starts with case
`first + e`, and when it finishes an episode env_step.hip resets it in place from an HBM-resident pool
to case `+E`, so the k episodes use exactly the cases the sequential loop would have used.  Per step
there is one policy launch and one env launch, no host synchronisation; discounted returns
(explorer.py:124), outcomes, navigation times and the "too close" statistics (:88-90) are accumulated
in-kernel.  With several ranks, envs are sharded by global env id and the records are combined by ONE
all_gather (dist.gather_records).

`run_k_episodes` reads top to bottom: `episode_plan` (which case sits in which pool row, host arithmetic only),
attach, one of three drivers (closed-loop ORCA launch, `action_seq` launch, per-step loop -- each returns the steps
taken and one trace dict of stacked [T,E,...] tensors), `_push_memory`, `_emit_collected`, `summarize_episodes`, detach.
"""
import logging
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _hip
from . import dist as mdist
from .envs import scenarios as S


def average(xs):
    return sum(xs) / len(xs) if xs else 0


def summarize_episodes(returns, infos, times, k, time_limit, returnRate=True, returnNav=False, phase=None, stay=False,
                       episode=None, print_failure=False, danger=None, time_step=None):
    """The end of every run_k_episodes (explorer.py:126-151; datagen.py:505-518 is the same arithmetic): per-episode
    discounted returns, final info codes (_hip.INFO_*) and times -> (result, stats).  `result` is the reference's return
    tuple: (average return, success, collision, timeout[, average navigation time]), rates when returnRate else counts
    (returnNav is only honoured together with returnRate).  `stats` holds the counts and avg_nav_time, the mean time
    of the successful episodes or `time_limit` when there is none.
    Logging, in the reference's order (nothing without `phase`): the phase line unless `stay`; for phase val / test
    the danger line, from `danger` = (steps whose info was Danger, sum of their min_dist) over sum(times) / time_step
    steps; with print_failure the two failure-case lines."""
    success = sum(1 for c in infos if c == _hip.INFO_REACHGOAL)
    collision = sum(1 for c in infos if c == _hip.INFO_COLLISION)
    timeout = sum(1 for c in infos if c == _hip.INFO_TIMEOUT)
    assert success + collision + timeout == k
    success_times = [t for t, c in zip(times, infos) if c == _hip.INFO_REACHGOAL]
    avg_nav_time = sum(success_times) / len(success_times) if success_times else time_limit
    if phase is not None and not stay:                                      # explorer.py:132
        extra = "" if episode is None else "in episode {} ".format(episode)
        logging.info("%-5s %shas success rate: %.2f, collision rate: %.2f, nav time: %.2f, total reward: %.4f",
                     phase.upper(), extra, success / k, collision / k, avg_nav_time, average(returns))
    if phase in ("val", "test"):                                            # explorer.py:88-90,138-141
        too_close, dist_sum = danger
        logging.info("Frequency of being in danger: %.2f and average min separate distance in danger: %.2f",
                     too_close / (sum(times) / time_step), dist_sum / too_close if too_close else 0.0)
    if phase is not None and print_failure:
        logging.info("Collision cases: %s", " ".join(str(i) for i, c in enumerate(infos) if c == _hip.INFO_COLLISION))
        logging.info("Timeout cases: %s", " ".join(str(i) for i, c in enumerate(infos) if c == _hip.INFO_TIMEOUT))
    stats = dict(success=success, collision=collision, timeout=timeout, avg_nav_time=avg_nav_time)
    if not returnRate:
        return (average(returns), success, collision, k - success - collision), stats
    rates = (average(returns), success / k, collision / k, (k - success - collision) / k)
    return (rates + (avg_nav_time,) if returnNav else rates), stats


def episode_plan(first, size, k, E_total, lo, E_local, test_case=None, contiguous_pool=False):
    """Which case every env plays in every round, as pool rows -- pure host arithmetic, no device, no env.
    Global episode g < k is case (first + g) % size (or `test_case`, explorer.py:54) and runs in global env g % E_total
    as that env's round g // E_total; this rank holds the E_local envs from global env `lo` on.  The pool has one row
    per distinct case in increasing case order; contiguous_pool (the device generator makes a case range) instead has
    row c - uniq[0] for case c.  The kernel's rule (include/mcn.h, mcn_rollout): round 0 is the loaded row mine[:, 0];
    every restart takes the env's next_case and advances it by `stride` modulo `pool_size`.

    Returns a namespace: rounds, cases (rounds * E_total of them), uniq, mine [E_local, rounds], pool_size, stride,
    next_case [E_local], n_full (local envs whose last round is one of the k episodes), danger_short_from (what
    attach_rollout takes for it), fin_slots."""
    rounds = -(-k // E_total)                               # episodes per env (ceil)
    M = rounds * E_total
    cases = [test_case] * M if test_case is not None else [(first + i) % size for i in range(M)]
    uniq = sorted(set(cases))
    if contiguous_pool:
        pool_size, slot_of = uniq[-1] - uniq[0] + 1, {c: c - uniq[0] for c in uniq}
    else:
        pool_size, slot_of = len(uniq), {c: j for j, c in enumerate(uniq)}
    # env e of this rank plays global episodes (lo + e) + r * E_total, r = 0..rounds-1
    mine = np.array([[slot_of[cases[(lo + e) + r * E_total]] for r in range(rounds)] for e in range(E_local)],
                    np.int64).reshape(E_local, rounds)
    # The row step between rounds is one constant.  M <= size: the M cases are distinct and form a cyclic interval,
    # so a case's rank among them is a rotation of its episode number i, and i + E_total moves the row by E_total mod
    # M (= pool_size; a contiguous pool that wraps spans all `size` cases and its row is the case itself).  M > size:
    # every case occurs, the row is the case, the step is E_total mod size.  test_case: one row, step 0.
    steps = np.diff(mine, axis=1) % pool_size
    stride = int(steps.flat[0]) if steps.size else 0
    assert (steps == stride).all(), "pool rows do not advance by a constant stride"
    # at least two finished-episode slots: with one the kernel keeps the LATEST episode of an env (mcn.h), and an env
    # that finishes early keeps replaying its case until the slowest env is done -- with a stochastic robot
    # (epsilon-greedy, random action_fn) the record would then describe the last repeat instead of the first run.
    # The "too close" counters cover exactly the k episodes: env g (global) plays `rounds` of them if
    # (rounds - 1) * E_total + g < k, else one fewer
    n_full = min(max(k - (rounds - 1) * E_total - lo, 0), E_local)
    return SimpleNamespace(rounds=rounds, cases=cases, uniq=uniq, mine=mine, pool_size=pool_size, stride=stride,
                           next_case=mine[:, 1] if rounds > 1 else mine[:, 0], n_full=n_full,
                           danger_short_from=0 if n_full == E_local else n_full + 1, fin_slots=max(rounds, 2))


def value_targets(states, rewards, dones, infos, imitation_learning, gamma_bar, target_model=None, device=None,
                  return_index=False):
    """explorer.py:153-186 (= datagen.py:520-543) for a whole batched rollout.  states [T,E,N,13] f32, rewards
    [T,E] f64, dones [T,E] bool, infos [T,E] u8, gamma_bar = gamma ** (time_step * v_pref).  Returns
    (states [M,N,13], values [M]) of the steps that belong to episodes ending in ReachGoal or Collision (only
    those feed the memory, explorer.py:107-110 / datagen.py:482-484)."""
    T, E = rewards.shape
    gbar = gamma_bar
    keep = torch.zeros(T, E, dtype=torch.bool, device=rewards.device)
    values = torch.zeros(T, E, dtype=torch.float64, device=rewards.device)
    good_end = (infos == _hip.INFO_REACHGOAL) | (infos == _hip.INFO_COLLISION)
    if not imitation_learning:
        with torch.no_grad():
            nxt = target_model(states[1:].reshape(-1, states.shape[2], states.shape[3]).to(device or states.device))
        nxt = torch.cat([nxt.view(T - 1, E).double(), torch.zeros(1, E, dtype=torch.float64, device=nxt.device)], 0)
    ep_ok = torch.zeros(E, dtype=torch.bool, device=rewards.device)      # episode containing step t ends well
    run = torch.zeros(E, dtype=torch.float64, device=rewards.device)     # discounted tail sum (IL)
    for t in range(T - 1, -1, -1):
        d = dones[t]
        ep_ok = torch.where(d, good_end[t], ep_ok)          # a done at t starts (going backwards) a new episode
        if imitation_learning:
            run = torch.where(d, rewards[t], rewards[t] + gbar * run)
            values[t] = run
        else:
            values[t] = torch.where(d, rewards[t], rewards[t] + gbar * nxt[t])
        keep[t] = ep_ok
    # steps after the last done of an env belong to an unfinished episode: ep_ok is False there by construction
    idx = keep.t().reshape(-1).nonzero().squeeze(1)           # (env, time) order
    flat_states = states.permute(1, 0, 2, 3).reshape(T * E, states.shape[2], states.shape[3])
    flat_values = values.t().reshape(-1)
    if return_index:           # positions of the kept rows in the (env, time)-flattened trace: env * T + t
        return flat_states[idx], flat_values[idx].float(), idx
    return flat_states[idx], flat_values[idx].float()


def trace_env_view(tr, rrad, rgoal, rvpref):
    """The [T, E] states of a closed-loop trace (VecCrowdSim.rollout_orca) as ONE batch of T * E envs: an object with
    the attributes a policy's `transform_batch` reads from a VecCrowdSim.  rrad / rgoal / rvpref ([E] / [E,2] / [E]) are
    the robot fields no step changes (a pool restart puts the robot back at the same goal)."""
    T, E, N = tr["hrad"].shape
    rob, hum = tr["robot"].reshape(T * E, 5), tr["humans"].reshape(T * E, N, 4)
    const = lambda x: x.unsqueeze(0).expand(T, *x.shape).reshape(T * E, *x.shape[1:])
    return SimpleNamespace(num_envs=T * E, _alloc_N=N, device=tr["hrad"].device, rpos=rob[:, 0:2], rvel=rob[:, 2:4],
                           rtheta=rob[:, 4], rrad=const(rrad), rgoal=const(rgoal), rvpref=const(rvpref),
                           hpos=hum[:, :, 0:2], hvel=hum[:, :, 2:4], hrad=tr["hrad"].reshape(T * E, N))


def trace_state_rows(transformer, tr, rrad, rgoal, rvpref):
    """`transformer.transform_batch` once over the T * E states of a trace: [T,E,...] rows, equal bit for bit to T
    per-step calls because every torch op in it is element-wise (see rows_from_trace_ok)."""
    T, E = tr["hrad"].shape[:2]
    rows = transformer.transform_batch(trace_env_view(tr, rrad, rgoal, rvpref))
    return rows.view(T, E, *rows.shape[1:])


def rows_from_trace_ok(transformer, env):
    """Whether `transformer.transform_batch` needs nothing but the traced tensors and the constant robot fields: the
    plain rotated joint states of CADRL / MultiHumanRL (SARL).  Occupancy maps (a kernel on the env's own state struct),
    LSTM-RL's device-side human order and an env that keeps an `hcount` stay on the per-step loop."""
    from .policy.cadrl import CADRL
    from .policy.multi_human_rl import MultiHumanRL
    fn = getattr(type(transformer), "transform_batch", None)
    if fn is not CADRL.transform_batch and fn is not MultiHumanRL.transform_batch:
        return False
    return not getattr(transformer, "with_om", False) and getattr(env, "hcount", None) is None


class VecExplorer(object):
    def __init__(self, env, robot, device=None, gamma=0.9, policy=None, memory=None, target_policy=None):
        self.env, self.robot, self.gamma = env, robot, gamma
        self.device = device or env.device
        self.policy = policy if policy is not None else robot.policy
        self.memory = memory
        self.target_policy = target_policy       # supplies transform() in imitation learning (explorer.py:163)
        self.target_model = None
        self.raw_memory = None                   # list / ReplayMemory-like: rows (ob [N,5], reward, done, info code)
        self.rawob = None                        # list / ReplayMemory-like: (humans [N,4], next velocities [N,2])
        # True: raw_memory rows carry the reference's value types, (list[ObservableState], reward, done, Info object)
        # as explorer.py:80-81 pushes them (the drop-in Explorer sets it); False: arrays and integer codes
        self.raw_rows_as_objects = False

    def update_target_model(self, target_model):
        import copy
        self.target_model = copy.deepcopy(target_model)

    def _value_targets(self, states, rewards, dones, infos, imitation_learning):
        gbar = pow(self.gamma, self.env.time_step * float(self.robot.v_pref))
        return value_targets(states, rewards, dones, infos, imitation_learning, gbar, self.target_model, self.device,
                             return_index=True)

    def _emit_collected(self, trace, k, rounds, E_total, update_raw_ob, cache_dir):
        """Split the recorded [T,E,...] trace at the dones and hand the k episodes out in the reference's order
        (episode g = round * E + env): raw_memory rows, world-model pairs, SGAN cache files."""
        cur, ob, rew, done, info, dmin = (trace[f].cpu().numpy() for f in ("cur", "ob", "reward", "done", "info", "dmin"))
        T, E = done.shape
        bounds = []
        for e in range(E):
            ends = np.nonzero(done[:, e])[0][:rounds]
            starts = np.concatenate([[0], ends[:-1] + 1])
            bounds.append(list(zip(starts.tolist(), ends.tolist())))
        push = lambda store, item: (store.push if hasattr(store, "push") else store.append)(item)
        fcount = 0
        for g in range(k):
            e, r = g % E_total, g // E_total
            t0, t1 = bounds[e][r]
            frames = []
            for t in range(t0, t1 + 1):
                if self.raw_memory is not None and self.raw_rows_as_objects:
                    from .envs.utils import info as I
                    from .envs.utils.state import ObservableState
                    push(self.raw_memory, ([ObservableState(*[float(x) for x in row]) for row in ob[t, e]],
                                           float(rew[t, e]), bool(done[t, e]), I.from_code(info[t, e], float(dmin[t, e]))))
                elif self.raw_memory is not None:
                    push(self.raw_memory, (ob[t, e].copy(), float(rew[t, e]), bool(done[t, e]), int(info[t, e])))
                if update_raw_ob and (np.abs(ob[t, e, :, 2:4]) > 1e-3).any():        # someone_is_moving
                    push(self.rawob, (torch.from_numpy(cur[t, e]).float(), torch.from_numpy(ob[t, e, :, 2:4].copy()).float()))
                fid = 10 * (t - t0 + 1)
                frames += [[fid, p, ob[t, e, p, 0], ob[t, e, p, 1]] for p in range(ob.shape[2])]
            if cache_dir is not None:
                fcount += 1
                with open(os.path.join(cache_dir, str(fcount) + ".txt"), "w") as fh:
                    for fr in frames:
                        fh.write("%s\t%s\t%s\t%s\n" % (fr[0], fr[1], fr[2], fr[3]))

    def _closed_loop_ok(self, transformer, action_fn, action_seq, stay):
        """The automatic rule of run_k_episodes(closed_loop=None): an ORCA robot policy (holonomic) choosing every
        action, on a VecCrowdSim whose step is the plain mcn_env_step (or mcn_env_step_sf) with ORCA, linear or
        social-force humans, and -- when memory rows are wanted -- a transformer whose rows can be made from the trace."""
        from .envs.crowd_sim import VecCrowdSim
        from .envs.policy.orca import ORCA
        env = self.env
        if not isinstance(self.policy, ORCA) or action_fn is not None or action_seq is not None or stay:
            return False
        if type(self.policy).predict_batch is not ORCA.predict_batch:
            return False
        if type(env).step is not VecCrowdSim.step or env.human_policy_name not in ("orca", "linear", "socialforce"):
            return False
        if getattr(env.robot, "kinematics", "holonomic") == "unicycle":
            return False
        return transformer is None or rows_from_trace_ok(transformer, env)

    # ------------------------------------------------------------------ the three drivers
    # Each advances the env until every env has finished `rounds` episodes or `limit` steps are taken and returns
    # (steps taken, trace): one dict of stacked [T,E,...] tensors, None when nothing was asked for.  With a
    # `transformer` it holds the memory fields rows, reward, done, info; with `collect` the collection fields cur
    # (humans [px,py,vx,vy] before the step), ob (humans [px,py,vx,vy,radius] after it), reward, done, info, dmin.
    def _all_finished(self, rounds):
        return int(self.env.rollout_buffers["fin_count"].min().item()) >= rounds

    def _drive_chunks(self, launch, limit, rounds):
        """`launch(t, n)` for chunks of at most 128 steps (a launch's time is set by its slowest env group)."""
        t = 0
        while t < limit:
            n = min(128, limit - t)
            launch(t, n)
            t += n
            if self._all_finished(rounds):
                break
        return t

    def _drive_closed_loop(self, limit, rounds, transformer, collect):
        """The ORCA robot's solve and the env step, up to 128 steps per launch (VecCrowdSim.rollout_orca); the trace
        fields are the per-step driver's arithmetic over the launch's trace at once."""
        env, chunks = self.env, []

        def launch(t, n):
            tr = env.rollout_orca(self.policy, n, trace=transformer is not None or collect)
            if collect:
                tr["hrad_after"] = torch.cat([tr["hrad"][1:], env.hrad.unsqueeze(0)])      # radii after each step
            if tr is not None:
                chunks.append(tr)
        steps = self._drive_chunks(launch, limit, rounds)
        if not chunks:
            return steps, None
        tr = {f: torch.cat([c[f] for c in chunks]) for f in chunks[0]}
        trace = dict(reward=tr["reward"], done=tr["done"].bool(), info=tr["info"])
        if transformer is not None:
            trace["rows"] = trace_state_rows(transformer, tr, env.rrad, env.rgoal, env.rvpref)
        if collect:
            trace.update(cur=tr["humans"], dmin=tr["dmin"],
                         ob=torch.cat([tr["humans"][..., 0:2] + tr["human_act"] * env.time_step, tr["human_act"],
                                       tr["hrad_after"].unsqueeze(3)], 3))
        return steps, trace

    def _drive_action_seq(self, action_seq, limit, rounds):
        """A robot whose actions are known up front: 128 steps per mcn_env_rollout launch, nothing recorded."""
        limit = min(limit, int(action_seq.shape[0]))
        return self._drive_chunks(lambda t, n: self.env.rollout(action_seq[t:t + n]), limit, rounds), None

    def _drive_per_step(self, limit, rounds, transformer, collect, action_fn, stay):
        """One policy launch (or `action_fn(env, t)`, or the zero action of `stay`) and one env launch per step."""
        env = self.env
        fields = (["rows"] if transformer is not None else []) + (["cur", "ob", "dmin"] if collect else [])
        rec = {f: [] for f in fields + ["reward", "done", "info"]} if fields else {}
        t = 0
        while t < limit:
            if transformer is not None:
                rec["rows"].append(transformer.transform_batch(env))           # the state the action is chosen in
            if stay:
                a = torch.zeros(env.num_envs, 2, dtype=torch.float64, device=env.device)
            else:
                a = action_fn(env, t) if action_fn is not None else self.policy.predict_batch(env)[0]
            if collect:
                prev_pos = env.hpos.clone()
                rec["cur"].append(torch.cat([prev_pos, env.hvel], 2))
            env.step(a)
            if collect:
                # the observation the reference's step() returns, also for envs that finished and were restarted
                # in-kernel: humans moved by the velocity they chose (same two roundings as the kernel's integrate)
                pos = prev_pos + env.human_act * env.time_step
                rec["ob"].append(torch.cat([pos, env.human_act, env.hrad.unsqueeze(2)], 2))
                rec["dmin"].append(env.dmin.clone())
            if rec:
                rec["reward"].append(env.reward.clone()); rec["done"].append(env.done.bool())
                rec["info"].append(env.info.clone())
            t += 1
            if t % 32 == 0 and self._all_finished(rounds):
                break
        return t, ({f: torch.stack(v) for f, v in rec.items()} if rec and t else None)

    def _push_memory(self, trace, k, rounds, E_total, lo, imitation_learning):
        """Value targets of the trace's k episodes into the memory, in the reference's push order."""
        dones = trace["done"]
        # only the first `rounds` episodes of each env are the k requested ones: cut each env's trace there
        order = torch.cumsum(dones.long(), 0) - dones.long()          # episode number each step belongs to
        valid = order < rounds
        gidx = (order * E_total + lo + torch.arange(dones.shape[1], device=dones.device).unsqueeze(0))
        valid &= gidx < k
        s, v, idx = self._value_targets(trace["rows"], trace["reward"], dones & valid, trace["info"], imitation_learning)
        # the reference pushes episode by episode (explorer.py:107-110): rows go to the memory in global episode
        # order (episode g = round * E_total + env), time order inside an episode -- a stable sort of the
        # (env, time)-ordered rows by their episode number
        ep_of_row = gidx.t().reshape(-1)[idx]
        perm = torch.argsort(ep_of_row, stable=True)
        s, v = s[perm], v[perm]
        if hasattr(self.memory, "push_batch"):
            self.memory.push_batch(s, v)
        else:                                                         # any object with the reference's push()
            for row_s, row_v in zip(s, v):
                self.memory.push((row_s, row_v.reshape(1).to(self.device)))

    def _load_cases(self, plan, phase, n, rule, device_scenarios):
        """Build the plan's pool (host scenarios, or on the device from the seed `device_scenarios`) and put every
        env on its round-0 row; returns the pool attach_rollout takes."""
        env = self.env
        if device_scenarios is None:
            pool = S.scenario_pool(env.spec(), phase, plan.uniq, n, rule)
            env.load_scenarios(pool[plan.mine[:, 0]])
            return pool
        if rule not in ("circle_crossing", "square_crossing"):
            raise NotImplementedError("device scenarios: circle_crossing / square_crossing only")
        # case ids keyed like the reference's seeds: offset(phase) + case (crowd_sim.py:270-272)
        offset = {"train": env.case_capacity["val"] + env.case_capacity["test"], "val": 0,
                  "test": env.case_capacity["val"]}[phase]
        pool = env.device_pool(device_scenarios, offset + plan.uniq[0], plan.pool_size, n, rule)
        env.load_device_scenarios(pool, plan.mine[:, 0])
        return pool

    def run_k_episodes(self, k, phase, update_memory=False, imitation_learning=False, episode=None,
                       print_failure=False, returnRate=True, returnNav=False, action_fn=None, max_steps=None,
                       total_envs=None, action_seq=None, device_scenarios=None, stay=False, update_raw_ob=False,
                       cacheFile=None, test_case=None, closed_loop=None):
        """Returns what Explorer.run_k_episodes returns (explorer.py:146-151):
        (avg cumulative reward, success rate, collision rate, timeout rate[, avg nav time])
        or counts instead of rates when returnRate is False.  `action_fn(env, t) -> [E,2]` overrides the
        policy (e.g. a random-action baseline).  `action_seq` ([T,E,2] device tensor) is a robot whose actions do
        not depend on the observation: its steps go to the device 128 at a time through mcn_env_rollout (one launch,
        state in registers) instead of one launch per step; not combinable with update_memory.
        `device_scenarios=seed` builds the k scenarios on the device (mcn_scenario_pool: the reference's placement
        rules, counter-based random stream -- for training rollouts that need many distinct cases, not for parity
        runs) instead of generating them on the host with numpy's MT19937.
        Data collection (explorer.py:60-85,112-121), single process only: `stay` keeps the robot still; with
        `self.raw_memory` set every step pushes `(ob, reward, done, info)` (ob = [N,5] array of the humans after the
        step, info = code) in episode order; `update_raw_ob` pushes world-model pairs into `self.rawob`; `cacheFile`
        (a directory) gets one SGAN text file per episode.
        `test_case` plays that one case k times (explorer.py:54 hands it to every reset; the counter ends one past it).
        `closed_loop`: None = automatic -- with an ORCA robot policy (the imitation-learning demonstrator, `--policy orca`)
        and no action_fn / action_seq / stay, the robot's solve and the env step run up to 128 steps per launch
        (VecCrowdSim.rollout_orca: ORCA, linear or social-force humans); memory rows and collected rows then come from
        that launch's trace, and every result equals the per-step loop's.  False forces the per-step loop; True raises
        where the closed loop does not apply."""
        env = self.env
        rank, ws = mdist.world()
        E_local = env.num_envs
        E_total = total_envs if total_envs is not None else E_local * ws
        lo, hi = mdist.shard(E_total, rank, ws)                # shards may differ by one env (E_total % ws != 0)
        if hi - lo != E_local:
            raise ValueError("rank %d of %d holds %d envs; its shard of %d is [%d, %d)" % (rank, ws, E_local, E_total, lo, hi))
        if hasattr(self.policy, "set_phase"):
            self.policy.set_phase(phase)
        n, rule = env._phase_rule(phase)
        first, size = env.case_counter[phase], env.case_size[phase]
        if test_case is not None and device_scenarios is not None:
            raise NotImplementedError("test_case with device scenarios")
        plan = episode_plan(first, size, k, E_total, lo, E_local, test_case, contiguous_pool=device_scenarios is not None)
        rounds = plan.rounds
        pool = self._load_cases(plan, phase, n, rule, device_scenarios)
        bufs = env.attach_rollout(self.gamma, pool=pool, case_stride=plan.stride, first_cases=plan.next_case,
                                  fin_slots=plan.fin_slots, danger_episodes=rounds,
                                  danger_short_from=plan.danger_short_from)
        horizon = int(round(env.time_limit / env.time_step)) + 2
        limit = max_steps if max_steps is not None else rounds * horizon
        if update_memory and (self.memory is None or self.gamma is None):
            raise ValueError("Memory or gamma value is not set!")
        transformer = (self.target_policy if imitation_learning else self.policy) if update_memory else None
        collect = self.raw_memory is not None or update_raw_ob or cacheFile is not None
        if collect:
            if ws > 1 or action_seq is not None:
                raise NotImplementedError("data collection runs in one process, one launch per step")
            keep_export, env.export_human_actions = env.export_human_actions, True
        auto = self._closed_loop_ok(transformer, action_fn, action_seq, stay)
        if closed_loop and not auto:
            raise ValueError("closed_loop=True needs an ORCA robot policy choosing every action, ORCA, linear or "
                             "social-force humans, a holonomic robot and memory rows that can be made from the trace")
        self.last_run_closed_loop = auto if closed_loop is None else bool(closed_loop)
        if self.last_run_closed_loop:
            steps, trace = self._drive_closed_loop(limit, rounds, transformer, collect)
        elif action_seq is not None:
            if update_memory:
                raise ValueError("action_seq rollouts record no per-step states; use action_fn with update_memory")
            steps, trace = self._drive_action_seq(action_seq, limit, rounds)
        else:
            steps, trace = self._drive_per_step(limit, rounds, transformer, collect, action_fn, stay)
        if not self._all_finished(rounds):
            raise RuntimeError("rollout did not finish %d episodes per env within %d steps" % (rounds, steps))
        if update_memory:
            self._push_memory(trace, k, rounds, E_total, lo, imitation_learning)
        if collect:
            env.export_human_actions = keep_export
            self._emit_collected(trace, k, rounds, E_total, update_raw_ob, cacheFile)
        env.case_counter[phase] = (first + k) % size if test_case is None else (test_case + 1) % size
        # records in global episode order: episode g = r * E_total + global_env
        # (the envs' "too close" counters ride in the same collective, in the rows of their first episode)
        dng = torch.zeros(2, E_local, rounds, dtype=torch.float64, device=bufs["fin_return"].device)
        dng[0, :, 0], dng[1, :, 0] = bufs["danger_count"].double(), bufs["danger_dist_sum"]
        rec = mdist.gather_records(bufs["fin_return"][:rounds].t().contiguous(), bufs["fin_info"][:rounds].t().contiguous(),
                                   bufs["fin_time"][:rounds].t().contiguous(), extras=(dng[0], dng[1]),
                                   equal_shards=(E_total % ws == 0))
        ret = rec["return"].view(-1, rounds).cpu().numpy()        # [E_total, rounds]
        inf = rec["info"].view(-1, rounds).cpu().numpy()
        tim = rec["time"].view(-1, rounds).cpu().numpy()
        order = [(g % E_total, g // E_total) for g in range(k)]
        returns = [float(ret[e, r]) for e, r in order]
        infos = [int(inf[e, r]) for e, r in order]
        times = [float(tim[e, r]) for e, r in order]
        too_close, dist_sum = int(round(rec["extras"][0].sum().item())), float(rec["extras"][1].sum().item())
        result, _ = summarize_episodes(returns, infos, times, k, env.time_limit, returnRate, returnNav,
                                       phase=phase, stay=stay, episode=episode, print_failure=print_failure,
                                       danger=(too_close, dist_sum), time_step=env.time_step)
        self.last_records = dict(returns=returns, infos=infos, times=times, danger_steps=too_close,
                                 danger_dist_sum=dist_sum)
        env.detach_rollout()
        return result
