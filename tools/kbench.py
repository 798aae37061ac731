#!/usr/bin/env python3
"""Kernel micro-benchmark (GPU box): per-launch time of mcn_env_step at several batch sizes and
human-policy modes, measured with HIP events around a hipGraph of back-to-back launches.
    python tools/kbench.py [--humans 5] [--sizes 4096,65536,1048576] [--modes orca,given]
    python tools/kbench.py --human-policy socialforce [--rollout 128 [--unfused]]   (mcn_env_step_sf / mcn_env_rollout_sf)
    python tools/kbench.py --sgan-predict --sizes 4096 --humans 10,5 --samples 1,20 --steps 8,12
    python tools/kbench.py --lstm-rl|--cadrl [--humans 5,10]   (look-ahead launch vs the torch forward it replaces)
    python tools/kbench.py --finish [--humans 5,10] [--sizes 4096]   (mcn_orca_finish vs one mcn_orca_batch launch per step)
    python tools/kbench.py --trainer [--policy sarl|lstm_rl|cadrl] [--humans 5,10]
                                        (Trainer.optimize_batch(100): fused HIP step vs torch autograd; CADRL has one
                                        row per state whatever --humans says)
    python tools/kbench.py --world-trainer [--world mlp|attention] [--humans 5,10]   (Trainer_Sim.optimize_epoch(3): fused HIP step vs torch autograd)
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def sgan_bench(E, N, iters):
    """One SGANWorld call (ring push + encoder + pool-net + decoder) for E scenes of N pedestrians."""
    from modelcrowdnav_amd.policy.world_model import VecSGANWorld, generator_from_arrays
    dev = torch.device("cuda", 0)
    gen = generator_from_arrays(np.load(os.path.join(ROOT, "tests", "golden", "g6_sgan.npz")), "p", dev)
    world = VecSGANWorld(gen, E, N, dev, time_step=0.25, seed=0)
    g = torch.Generator(device="cpu").manual_seed(0)
    pos = (torch.rand(E, N, 2, dtype=torch.float64, generator=g) * 8 - 4).to(dev)
    vel = (torch.rand(E, N, 2, dtype=torch.float64, generator=g) - 0.5).to(dev)
    world.init_constant_velocity(pos, vel)
    for _ in range(3):
        world(pos)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        world(pos)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / iters
    tf = 0.69e6 * E * N / ms / 1e9
    print("SGAN step N=%d E=%d: %.1f us/call  %.1f TFLOP/s algorithmic (%.1f %% of the fp32 MFMA peak %.1f)" % (
        N, E, ms * 1e3, tf, 100 * tf / bench.MFMA_F32_PEAK_TFLOPS, bench.MFMA_F32_PEAK_TFLOPS), flush=True)


def sgan_predict_bench(E, N, K, T, iters):
    """One mcn_sgan_predict (encoder + pool-net once, K x T decoder cells) for E scenes of N pedestrians, beside
    mcn_sgan_step on the same ring (no push) and K T times that: what K T one-step calls would cost."""
    from modelcrowdnav_amd.policy.world_model import generator_from_arrays
    from modelcrowdnav_amd.sgan.models import sgan_predict, sgan_step
    dev = torch.device("cuda", 0)
    gen = generator_from_arrays(np.load(os.path.join(ROOT, "tests", "golden", "g6_sgan.npz")), "p", dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    pos = torch.rand(E, 1, N, 2, dtype=torch.float64, generator=g) * 8 - 4
    vel = torch.rand(E, 1, N, 2, dtype=torch.float64, generator=g) - 0.5
    k = torch.arange(7, -1, -1, dtype=torch.float64).view(1, 8, 1, 1)
    hist = (torch.round((pos - vel * 0.25 * k) * 1e4) / 1e4).to(dev)
    noise = torch.randn(K, E, 8, generator=g).to(dev)
    out_vel = torch.empty(E, N, 2, dtype=torch.float64, device=dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters * 1e3

    us_step = timed(lambda: sgan_step(gen, hist, 0, 0, None, noise[0], 0.25, want_rel=False, out_vel=out_vel))
    us = timed(lambda: sgan_predict(gen, hist, 0, noise, T))
    print("SGAN predict N=%d E=%d K=%d T=%d: %.1f us/call; mcn_sgan_step %.1f us/call, x K T = %.1f us (%.1f x)" % (
        N, E, K, T, us, us_step, us_step * K * T, us_step * K * T / us), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--humans", type=str, default="5", help="humans per env (a comma list with --sarl)")
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--modes", default="orca,given")
    ap.add_argument("--visible", action="store_true")
    ap.add_argument("--human-policy", default="orca", choices=("orca", "socialforce"),
                    help="the env's own humans in the 'orca' mode of --modes, in --rollout and in --closed-loop "
                         "(socialforce: default parameters)")
    ap.add_argument("--unfused", action="store_true", help="with --rollout: mcn_tuning.rollout_fused = 0 (T step launches)")
    ap.add_argument("--no-hh", action="store_true", help="no human-human overlap count (ModelCrowdSim.step does not count)")
    ap.add_argument("--pair-stream", type=int, default=-1, help="mcn_tuning.pair_stream")
    ap.add_argument("--lp3-defer", type=int, default=-1, help="mcn_tuning.lp3_defer")
    ap.add_argument("--step-block", type=int, default=-1, help="mcn_tuning.step_block (64 / 256)")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sarl", action="store_true")
    ap.add_argument("--om", action="store_true", help="with --sarl: OM-SARL ([sarl] with_om = true: mcn_sarl_om_prepare + mcn_sarl_predict_om)")
    ap.add_argument("--rollout", type=int, default=0, help="time mcn_env_rollout with this many steps per launch")
    ap.add_argument("--sgan", action="store_true", help="time mcn_sgan_step (shipped pool-net weights) at --sizes x --humans")
    ap.add_argument("--sgan-predict", action="store_true",
                    help="time mcn_sgan_predict at --sizes x --humans for --samples noise vectors and --steps decoder steps")
    ap.add_argument("--steps", default="8", help="with --sgan-predict: decoder steps T (a comma list)")
    ap.add_argument("--samples", default="1", help="with --sgan-predict: noise samples K per scene (a comma list)")
    ap.add_argument("--lstm-rl", action="store_true", help="time mcn_lstm_rl_predict at 4096 envs x --humans")
    ap.add_argument("--cadrl", action="store_true", help="time mcn_cadrl_predict at 4096 envs x --humans")
    ap.add_argument("--finish", action="store_true",
                    help="time VecCrowdSim.get_human_times (one mcn_orca_finish launch) at --sizes x --humans against one "
                         "mcn_orca_batch launch + torch update per simulated step, and the E = 1 CrowdSim method against "
                         "its former host loop")
    ap.add_argument("--closed-loop", action="store_true",
                    help="time one 128-step mcn_env_rollout_orca launch (--human-policy socialforce: mcn_env_rollout_orca_sf; "
                         "with and without traces) at --sizes x --humans "
                         "against 128 x (ORCA.predict_batch + env.step) and against the per-step Explorer loop body")
    ap.add_argument("--trainer", action="store_true",
                    help="time Trainer.optimize_batch(100) at batch 100 x --humans: fused HIP step (fused=True) against "
                         "the torch path, five alternating repeats")
    ap.add_argument("--policy", default="sarl", choices=("sarl", "lstm_rl", "cadrl"),
                    help="with --trainer: the value network that is trained")
    ap.add_argument("--world-trainer", action="store_true",
                    help="time Trainer_Sim.optimize_epoch(3) on 25 000 synthetic pairs at batch 100 x --humans: fused HIP "
                         "step (fused=True) against the torch path, five alternating repeats")
    ap.add_argument("--world", default="attention", choices=("attention", "mlp"),
                    help="with --world-trainer: the world model that is trained (mlp: MlpWorld with its default dropout 0.5)")
    a = ap.parse_args()
    if a.world_trainer:
        for N in [int(x) for x in str(a.humans).split(",")]:
            world_trainer_bench(N, world=a.world)
        return
    if a.trainer:
        for N in [1] if a.policy == "cadrl" else [int(x) for x in str(a.humans).split(",")]:
            trainer_bench(N, policy=a.policy)
        return
    if a.closed_loop:
        for N in [int(x) for x in str(a.humans).split(",")]:
            for E in [int(x) for x in a.sizes.split(",")]:
                closed_loop_bench(E, N, human_policy=a.human_policy)
        return
    if a.finish:
        for N in [int(x) for x in str(a.humans).split(",")]:
            for E in [int(x) for x in a.sizes.split(",")]:
                finish_bench(E, N)
            finish_bench_e1(N)
        return
    if a.lstm_rl or a.cadrl:
        for N in [int(x) for x in str(a.humans).split(",")]:
            policy_bench("lstm_rl" if a.lstm_rl else "cadrl", 4096, N)
        return
    if a.sgan_predict:
        for N in [int(x) for x in str(a.humans).split(",")]:
            for E in [int(x) for x in a.sizes.split(",")]:
                for K in [int(x) for x in a.samples.split(",")]:
                    for T in [int(x) for x in a.steps.split(",")]:
                        sgan_predict_bench(E, N, K, T, a.iters)
        return
    if a.sgan:
        for N in [int(x) for x in str(a.humans).split(",")]:
            for E in [int(x) for x in a.sizes.split(",")]:
                sgan_bench(E, N, a.iters)
        return
    if not a.sarl:
        a.humans = int(a.humans)
    if a.rollout:
        rollout_bench(a)
        return
    if a.sarl:
        for N in [int(x) for x in str(a.humans).split(",")]:
            sarl_bench(4096, N, om=a.om)
        return
    dev = torch.device("cuda", 0)
    N = a.humans
    if a.step_block > 0:
        from modelcrowdnav_amd import _hip
        _hip.set_tuning(step_block=a.step_block)
    if a.lp3_defer >= 0:                       # before the env allocates (or skips) its 3-D-LP queue
        from modelcrowdnav_amd import _hip
        _hip.set_tuning(lp3_defer=a.lp3_defer)
    for E in [int(x) for x in a.sizes.split(",")]:
        env, _ = bench.build_env(E, N, 0, dev)
        env.robot.visible = a.visible
        env.human_policy_name = a.human_policy
        if a.no_hh:
            env.count_hh = False
        if a.pair_stream >= 0:
            from modelcrowdnav_amd import _hip
            _hip.set_tuning(pair_stream=a.pair_stream)
        if a.lp3_defer >= 0:
            from modelcrowdnav_amd import _hip
            _hip.set_tuning(lp3_defer=a.lp3_defer)
        acts = bench.make_actions(16, E, E, 0, dev)
        gv = torch.rand(E, N, 2, dtype=torch.float64, device=dev) - 0.5
        for mode in a.modes.split(","):
            g = gv if mode.startswith("given") else None
            if mode.endswith("-noroll"):
                env.detach_rollout()        # no Explorer bookkeeping / auto-reset: fewer per-env streams
            if mode.endswith("-nopool"):
                env.detach_rollout()
                env.attach_rollout(gamma=0.9)   # Explorer record only, no restart from the pool
            for t in range(8):
                env.step(acts[t], given_v=g)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for t in range(a.iters):
                    env.step(acts[t % 16], given_v=g)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            best = 1e9
            for rep in range(3):
                s.record(); graph.replay(); e.record(); torch.cuda.synchronize()
                best = min(best, s.elapsed_time(e) / a.iters)
            nb = bench.pairwise_bytes_per_env_step(N) if mode.startswith("given") else bench.algorithmic_bytes_per_env_step(N)
            if mode.startswith("orca") and a.human_policy != "orca":
                mode = a.human_policy + mode[4:]
            print("N=%d E=%8d mode=%-12s  %9.2f us/launch  %8.1f M env-steps/s  %7.1f GB/s (%.1f%% of 8 TB/s)" % (
                N, E, mode, best * 1e3, E / best / 1e3, nb * E / best / 1e6, nb * E / best / 1e6 / 80.0))
        del env




def trainer_bench(N, batch=100, num_batches=100, rows=20000, reps=5, policy="sarl"):
    """Wall time of one Trainer.optimize_batch(num_batches) call -- what train.py makes after every episode -- with the
    fused HIP step and with torch autograd + optim.SGD, on the same seeded value network of `policy` (sarl, lstm_rl, or
    cadrl with its one 13-wide row per state) and device memory.  The two
    paths alternate within one process (fused, torch, fused, ...) so that clock and cache state drift hits both; one
    untimed call of each first.  The call ends with its own device-to-host copy of the losses, so host time is device
    time plus launch overhead: that overhead is what the fused step is about."""
    import copy
    import time
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.utils.memory import ReplayMemory
    from modelcrowdnav_amd.utils.trainer import Trainer
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pol = policy_factory[policy]()
    pol.configure(configs.policy_config())
    g = torch.Generator().manual_seed(1)
    states = torch.randn(rows, N, 13, generator=g)
    states[:, :, :6] = states[:, :1, :6]
    values = torch.tanh(states[:, :, 6].mean(1))
    tag = "trainer" if policy == "sarl" else "trainer %s" % policy
    if policy == "cadrl":
        states = states[:, 0]
    mem = ReplayMemory(rows, device=dev)
    mem.push_batch(states.to(dev), values.to(dev))
    trainers = {}
    for name, fused in (("fused", True), ("torch", False)):
        tr = Trainer(copy.deepcopy(pol.model).to(dev), mem, dev, batch, fused=fused)
        tr._gen.manual_seed(2)
        tr.set_learning_rate(0.001)
        tr.optimize_batch(num_batches)                       # untimed: allocations, module load, first-launch costs
        trainers[name] = tr
    times = {"fused": [], "torch": []}
    for _ in range(reps):
        for name in ("fused", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[name].optimize_batch(num_batches)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name in ("fused", "torch"):
        t = np.asarray(times[name])
        print("%s N=%d batch=%d optimize_batch(%d) %-5s: median %8.2f ms  min %8.2f  max %8.2f  (%d repeats; %.1f us / step)"
              % (tag, N, batch, num_batches, name, np.median(t), t.min(), t.max(), reps, np.median(t) * 1e3 / num_batches))
    print("%s N=%d: torch / fused = %.2f (medians)" % (tag, N, np.median(times["torch"]) / np.median(times["fused"])))


def world_trainer_bench(N, batch=100, epochs=3, rows=25000, reps=5, world="attention"):
    """Wall time of one Trainer_Sim.optimize_epoch(epochs) call -- what the model-based training loop makes once per
    training episode -- with the fused HIP step and with torch autograd + optim.Adam, on the same seeded AttentionWorld (or, with
    world="mlp", MlpWorld(N) with its default dropout) and a synthetic pair memory sized like the reference's `rawob` after its initial episodes (500 episodes of about 50
    steps).  A call is: shuffle and stack the memory (the same host work on both paths), then per epoch 200 training
    steps and 50 validation batches; 3 epochs cannot stop early (patience 7).  The two paths alternate within one
    process (fused, torch, fused, ...) so that clock and cache state drift hits both; one untimed call of each first.
    Also printed: the stacking alone, which both paths pay."""
    import copy
    import time
    from modelcrowdnav_amd.policy.world_model import AttentionWorld, MlpWorld
    from modelcrowdnav_amd.utils.trainer_sim import Trainer_Sim
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = MlpWorld(N) if world == "mlp" else AttentionWorld()
    tag = "world trainer" if world == "attention" else "world trainer (mlp)"
    g = torch.Generator().manual_seed(1)
    cur = torch.randn(rows, N, 4, generator=g) * torch.tensor([3.0, 3.0, 0.7, 0.7])
    nxt = 0.8 * cur[:, :, 2:4] + 0.1 * torch.randn(rows, N, 2, generator=g)
    memory = [(cur[i], nxt[i]) for i in range(rows)]
    trainers = {}
    for name, fused in (("fused", True), ("torch", False)):
        tr = Trainer_Sim(copy.deepcopy(model).to(dev), list(memory), dev, batch, fused=fused)
        tr.set_learning_rate(0.001)
        tr.optimize_epoch(1, reset=True)                     # untimed: allocations, module load, first-launch costs
        trainers[name] = tr
    times = {"fused": [], "torch": [], "stack": []}
    steps = epochs * -(-int(rows * 0.8) // batch)
    for _ in range(reps):
        for name in ("fused", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[name].optimize_epoch(epochs, reset=True)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        trainers["torch"]._pairs()
        torch.cuda.synchronize()
        times["stack"].append((time.perf_counter() - t0) * 1e3)
    for name in ("fused", "torch", "stack"):
        t = np.asarray(times[name])
        what = "optimize_epoch(%d) %-5s" % (epochs, name) if name != "stack" else "of which _pairs()      "
        print("%s N=%d batch=%d rows=%d %s: median %8.2f ms  min %8.2f  max %8.2f  (%d repeats)"
              % (tag, N, batch, rows, what, np.median(t), t.min(), t.max(), reps))
    f, t, k = (float(np.median(times[n])) for n in ("fused", "torch", "stack"))
    print("%s N=%d: torch / fused = %.2f (medians); without the stacking %.2f; per training step incl. its share "
          "of validation: fused %.1f us, torch %.1f us (%d steps)" % (tag, N, t / f, (t - k) / (f - k), (f - k) * 1e3 / steps,
                                                                   (t - k) * 1e3 / steps, steps))


def closed_loop_bench(E, N, T=128, reps=5, human_policy="orca"):
    """us per simulated step of the closed loop with an ORCA robot (safety_space 0.15, the imitation-learning
    demonstrator) over ORCA or social-force humans (--human-policy; socialforce: default parameters): one T-step
    mcn_env_rollout_orca / mcn_env_rollout_orca_sf launch without / with traces, T x (predict_batch + step), and the
    per-step loop body of VecExplorer.run_k_episodes(update_memory=True, imitation_learning=True) with a SARL target
    policy.  The four forms alternate inside every repeat; min / median / max over the repeats."""
    from modelcrowdnav_amd import _hip, configs
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    from modelcrowdnav_amd.policy.sarl import SARL
    dev = torch.device("cuda", 0)
    env, _ = bench.build_env(E, N, 0, dev)
    pol = policy_factory["orca"]()
    pol.multiagent_training, pol.safety_space = True, 0.15
    env.robot.set_policy(pol)
    env.human_policy_name = human_policy
    sarl = SARL(); sarl.configure(configs.policy_config()); sarl.kinematics = "holonomic"; sarl.set_device(dev)

    def per_step():
        for _ in range(T):
            a, _ = pol.predict_batch(env)
            env.step(a)

    def explorer_body():
        rows = []
        for _ in range(T):
            rows.append(sarl.transform_batch(env))
            a, _ = pol.predict_batch(env)
            env.step(a)
            rows.append((env.reward.clone(), env.done.bool(), env.info.clone()))

    forms = [("closed loop", lambda: env.rollout_orca(pol, T)), ("closed loop + traces", lambda: env.rollout_orca(pol, T, trace=True)),
             ("per step", per_step), ("explorer loop body", explorer_body)]
    times = {k: [] for k, _ in forms}
    ran = {}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps + 1):                       # the first repeat warms up
        for name, fn in forms:
            torch.cuda.synchronize()
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            ran[name] = _hip.last_dispatch()
            if rep:
                times[name].append(s.elapsed_time(e) * 1e3 / T)
    for name, _ in forms:
        v = sorted(times[name])
        print("N=%d E=%6d T=%d %s humans %-22s min %8.2f  median %8.2f  max %8.2f us/step  (%s)" % (
            N, E, T, human_policy, name, v[0], v[len(v) // 2], v[-1], ran[name]))


def rollout_bench(a):
    """Per-step time of the fused T-step launch (mcn_set_tuning(rollout_fused=1) forces it at any batch size)."""
    dev = torch.device("cuda", 0)
    N, T = a.humans, a.rollout
    from modelcrowdnav_amd import _hip
    _hip.set_tuning(rollout_fused=0 if a.unfused else 1)
    for E in [int(x) for x in a.sizes.split(",")]:
        env, _ = bench.build_env(E, N, 0, dev)
        env.robot.visible = a.visible
        env.human_policy_name = a.human_policy
        acts = bench.make_actions(T, E, E, 0, dev)
        env.rollout(acts)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for rep in range(5):
            s.record(); env.rollout(acts); e.record(); torch.cuda.synchronize()
            best = min(best, s.elapsed_time(e) / T)
        print("N=%d E=%8d %s rollout T=%d (%s)  %9.3f us/step  %8.1f M env-steps/s" % (
            N, E, a.human_policy, T, _hip.last_dispatch(), best * 1e3, E / best / 1e3))
        del env


def sarl_bench(E=4096, N=5, iters=5, om=False):
    """mcn_sarl_lookahead alone and SARL-driven env steps (BASELINE config 3).  om: OM-SARL -- the same look-ahead with
    mlp1.0 started from the occupancy maps' share, plus the launch that builds it."""
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.policy.sarl import SARL
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pol = SARL(); pol.configure(configs.policy_config(**({"sarl.with_om": "true"} if om else {}))); pol.kinematics = "holonomic"
    pol.set_device(dev); pol.set_phase("test"); pol.time_step = 0.25
    env, _ = bench.build_env(E, N, 0, dev)
    for _ in range(2):
        a, b = pol.predict_batch(env)
        env.step(a)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        pol.predict_batch(env)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / iters
    r = bench._sarl_roofline(E, N, ms)
    print(("OM-" if om else "") + "SARL lookahead N=%d E=%d: %.3f ms/launch  %.1f TFLOP/s executed = %.3f of the %.1f peak [%s]; float32-MFMA "
          "equivalent %.1f TFLOP/s = %.3f of the fp32 MFMA peak 157.3 (%.1f by the reference's FLOP count)  %.3f M env-steps/s" % (
              N, E, ms, r["achieved"], r["frac"], r["peak"], "bf16x3" if bench.sarl_uses_x3() else "f32", r["f32_mfma_equivalent_rate"],
              r["f32_mfma_equivalent_rate_over_f32_peak"], r["reference_flop_rate"], E / ms / 1e3))
    s.record()
    for _ in range(iters):
        a, b = pol.predict_batch(env)
        env.step(a)
    e.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(e) / iters
    print("SARL-driven env step N=%d E=%d: %.3f ms/step  %.3f M env-steps/s" % (N, E, ms, E / ms / 1e3))


def _finish_per_step(env, max_steps=8000):
    """get_human_times for a batch as it could be written without mcn_orca_finish: per simulated step one mcn_orca_batch
    launch over all E (N + 1) agents, a torch float32 position update, the float64 arrival test and one synchronising
    "is anybody left" read.  Same arithmetic; returns (human_times, steps taken by the slowest env)."""
    from modelcrowdnav_amd import _hip
    E, N, dev = env.num_envs, env._alloc_N, env.device
    A, f32 = N + 1, torch.float32
    pos64 = torch.cat([env.rpos.unsqueeze(1), env.hpos], 1)
    goal = torch.cat([env.rgoal.unsqueeze(1), env.hgoal], 1)
    rad64 = torch.cat([env.rrad.unsqueeze(1), env.hrad], 1)
    vmax = torch.cat([env.rvpref.unsqueeze(1), env.hvpref], 1).to(f32)
    pos, vel = pos64.to(f32), torch.cat([env.rvel.unsqueeze(1), env.hvel], 1).to(f32)
    rad = rad64.to(f32)
    others = torch.tensor([[j for j in range(A) if j != i] for i in range(A)], device=dev)        # [A, N]
    n_other = torch.full((E * A,), N, dtype=torch.int32, device=dev)
    out = torch.empty(E * A, 2, dtype=f32, device=dev)
    times, gtime = env.human_times.clone(), env.gtime.clone()
    live = (times == 0).any(1)
    steps, dt32 = 0, torch.tensor(env.time_step, dtype=f32, device=dev)
    while steps < max_steps and bool(live.any()):
        e = goal - pos64
        n = torch.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]).unsqueeze(-1)
        pref = torch.where(n > 1, e / n, e).to(f32)
        me = torch.cat([pos, vel, rad.unsqueeze(-1), vmax.unsqueeze(-1), pref], 2).reshape(E * A, 8).contiguous()
        oth = torch.cat([pos[:, others], vel[:, others], rad[:, others].unsqueeze(-1)], 3).reshape(E * A, N, 5).contiguous()
        _hip.check(_hip.lib.mcn_orca_batch(_hip.ptr(me), _hip.ptr(oth), _hip.ptr(n_other), _hip.ptr(out), E * A, N, 10.0,
                                           10, 5.0, float(env.time_step), _hip.stream_ptr(dev)), "mcn_orca_batch")
        lv = live.view(E, 1, 1)
        vel = torch.where(lv, out.view(E, A, 2), vel)
        pos = torch.where(lv, pos + vel * dt32, pos)
        gtime = torch.where(live, gtime + env.time_step, gtime)
        d = pos64[:, 1:] - goal[:, 1:]
        here = torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < rad64[:, 1:]
        times = torch.where(live.unsqueeze(1) & (times == 0) & here, gtime.unsqueeze(1), times)
        pos64 = pos.to(torch.float64)
        live = (times == 0).any(1)
        steps += 1
    return times, steps


def finish_bench(E, N, reps=5):
    """One VecCrowdSim.get_human_times call (mcn_orca_finish: the step loop inside the kernel) for E reset
    circle-crossing scenes with the robot on its goal, against _finish_per_step on the same scenes, alternating, `reps`
    times each; wall time around a device synchronise.  The two must return the same arrival times."""
    import time
    dev = torch.device("cuda", 0)
    env, _ = bench.build_env(E, N, 0, dev)
    env.detach_rollout()
    start = {k: getattr(env, k).clone() for k in ("hpos", "rpos", "gtime", "human_times")}

    def restart():
        for k, v in start.items():
            getattr(env, k).copy_(v)
        env.rpos.copy_(env.rgoal)
        torch.cuda.synchronize()

    one, per = [], []
    for rep in range(reps + 1):                      # the first round of each warms up
        restart()
        t0 = time.perf_counter()
        times, steps = env.get_human_times()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        times = times.clone()
        restart()
        t2 = time.perf_counter()
        times_ps, nsteps = _finish_per_step(env)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if not (torch.equal(times, times_ps) and int(steps.max()) == nsteps):
            print("finish N=%d E=%d: THE PER-STEP BASELINE DISAGREES (%d envs, %d vs %d steps)" % (
                N, E, int((times != times_ps).any(1).sum()), int(steps.max()), nsteps), flush=True)
        if rep:
            one.append((t1 - t0) * 1e3); per.append((t3 - t2) * 1e3)
    fmt = lambda v: "median %.2f ms (min %.2f, max %.2f)" % (sorted(v)[len(v) // 2], min(v), max(v))
    print("finish N=%d E=%d: %d env-steps in all, slowest env %d steps; one launch %s; per-step launches %s; ratio of "
          "medians %.1f x" % (N, E, int(steps.sum()), int(steps.max()), fmt(one), fmt(per),
                              sorted(per)[len(per) // 2] / sorted(one)[len(one) // 2]), flush=True)


def _e1_host_loop(env, max_steps=8000):
    """CrowdSim.get_human_times as it was before mcn_orca_finish: per simulated step a numpy pack, two host-to-device
    copies, one mcn_orca_batch launch, a synchronising copy back and the float32 update on the host."""
    from modelcrowdnav_amd import _hip
    v, robot = env._vec, env._vec.robot
    agents = [robot] + env.humans
    B, f32, dev = len(agents), np.float32, v.device
    M = B - 1
    pos = np.array([a.get_position() for a in agents], np.float64).astype(f32)
    vel = np.array([a.get_velocity() for a in agents], np.float64).astype(f32)
    rad = np.array([a.radius for a in agents], np.float64).astype(f32)
    vmax = np.array([a.v_pref for a in agents], np.float64).astype(f32)
    dt32 = f32(v.time_step)
    others_idx = np.array([[j for j in range(B) if j != i] for i in range(B)], np.int64).reshape(B, M)
    d_n = torch.full((B,), M, dtype=torch.int32, device=dev)
    d_out = torch.empty(B, 2, dtype=torch.float32, device=dev)
    steps = 0
    while not all(env.human_times):
        pref = np.zeros((B, 2), np.float64)
        for i, agent in enumerate(agents):
            vel_pref = np.array(agent.get_goal_position()) - np.array(agent.get_position())
            if np.linalg.norm(vel_pref) > 1:
                vel_pref /= np.linalg.norm(vel_pref)
            pref[i] = vel_pref
        me = np.concatenate([pos, vel, rad[:, None], vmax[:, None], pref.astype(f32)], 1).astype(f32)
        oth = np.concatenate([pos[others_idx], vel[others_idx], rad[others_idx][..., None]], 2).astype(f32)
        d_me, d_oth = torch.from_numpy(me).to(dev), torch.from_numpy(np.ascontiguousarray(oth)).to(dev)
        _hip.check(_hip.lib.mcn_orca_batch(_hip.ptr(d_me), _hip.ptr(d_oth), _hip.ptr(d_n), _hip.ptr(d_out), B, max(M, 1),
                                           10.0, 10, 5.0, float(v.time_step), _hip.stream_ptr(dev)), "mcn_orca_batch")
        vel = d_out.cpu().numpy().astype(f32)
        pos = (pos + vel * dt32).astype(f32)
        env.global_time += v.time_step
        steps += 1
        for i, human in enumerate(env.humans):
            if env.human_times[i] == 0 and human.reached_destination():
                env.human_times[i] = env.global_time
        robot.set_position((float(pos[0, 0]), float(pos[0, 1])))
        for i, human in enumerate(env.humans):
            human.set_position((float(pos[i + 1, 0]), float(pos[i + 1, 1])))
        env.states.append([robot.get_full_state(), [h.get_full_state() for h in env.humans]])
        if steps >= max_steps:
            break
    return env.human_times


def finish_bench_e1(N, reps=5, cases=(0, 3, 7, 11)):
    """CrowdSim.get_human_times (E = 1, through mcn_orca_finish) against its former host loop on the same scenes
    (`test` cases, robot put on its goal), alternating, `reps` times each: wall time per call over the cases."""
    import time
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.envs import CrowdSim
    from modelcrowdnav_amd.envs.utils.robot import Robot
    from modelcrowdnav_amd.envs.policy.policy_factory import policy_factory
    cfg = configs.env_config(**{"sim.human_num": N})
    env = CrowdSim()
    env.configure(cfg)
    robot = Robot(cfg, "robot")
    pol = policy_factory["orca"]()
    pol.configure(cfg)
    robot.set_policy(pol)
    env.set_robot(robot)

    def run(fn):
        total, got, nstates = 0.0, [], 0
        for case in cases:
            env.reset("test", case)
            robot.set_position(robot.get_goal_position())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got.append(list(fn()))
            total += time.perf_counter() - t0
            nstates += len(env.states)
        return total * 1e3 / len(cases), got, nstates

    new, old = [], []
    for rep in range(reps + 1):                      # the first round of each warms up
        a, got_a, na = run(env.get_human_times)
        b, got_b, nb = run(lambda: _e1_host_loop(env))
        if got_a != got_b or na != nb:
            print("finish E=1 N=%d: THE FORMER HOST LOOP DISAGREES" % N, flush=True)
        if rep:
            new.append(a); old.append(b)
    fmt = lambda v: "median %.2f ms (min %.2f, max %.2f)" % (sorted(v)[len(v) // 2], min(v), max(v))
    print("finish E=1 N=%d: %.1f steps per call; through mcn_orca_finish %s; former host loop %s; ratio of medians %.1f x" % (
        N, na / len(cases), fmt(new), fmt(old), sorted(old)[len(old) // 2] / sorted(new)[len(new) // 2]), flush=True)


def policy_bench(kind, E=4096, N=5, iters=20):
    """One LSTM-RL / CADRL look-ahead launch (mcn_*_predict + the argmax kernel) over E envs x 81 actions, and a torch
    float32 batched forward of the same module on the same-sized [E*A, N, 13] input (what it replaces), both timed
    with device events after warm-up.  Useful FLOP per (env, action): LSTM-RL N*2*200*63 + 2*33 500, CADRL N*54 100."""
    from modelcrowdnav_amd import configs
    from modelcrowdnav_amd.policy.policy_factory import policy_factory
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    pol = policy_factory[kind](); pol.configure(configs.policy_config()); pol.kinematics = "holonomic"
    pol.set_device(dev); pol.set_phase("test"); pol.time_step = 0.25
    env, _ = bench.build_env(E, N, 0, dev)
    pol.predict_batch(env)
    A = len(pol.action_space)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record(); torch.cuda.synchronize()
        return s.elapsed_time(e) / iters

    ms = timed(lambda: pol.predict_batch(env))
    x = torch.rand(E * A, N, 13, device=dev)
    with torch.no_grad():
        if kind == "cadrl":
            ms_t = timed(lambda: pol.model(x.view(-1, 13)).view(E * A, N).min(1))
        else:
            ms_t = timed(lambda: pol.model(x))
    flop = (N * 2 * 200 * 63 + 2 * 33500) if kind == "lstm_rl" else N * 54100
    tf = flop * E * A / ms / 1e9
    print("%s lookahead N=%d E=%d: %.3f ms/launch  %.1f TFLOP/s useful = %.3f of the fp32 MFMA peak %.1f "
          "(peak bound %.3f ms); torch fp32 forward of the same module on [%d, %d, 13]: %.3f ms (%.2fx)" % (
              kind, N, E, ms, tf, tf / bench.MFMA_F32_PEAK_TFLOPS, bench.MFMA_F32_PEAK_TFLOPS,
              flop * E * A / bench.MFMA_F32_PEAK_TFLOPS / 1e9, E * A, N, ms_t, ms_t / ms), flush=True)


if __name__ == "__main__":
    main()
