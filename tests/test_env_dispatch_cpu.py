"""CPU: the env kernels' dispatch plan (csrc/env_dispatch.hpp) against a literal table.

tests/env_dispatch_probe.cpp includes the header with the host C++ compiler alone and prints the plan of every problem
it reads.  The table holds both sides of every measured threshold and every mcn_tuning field forced each way (the
settings of tests/kernel_paths.py); it was derived from the rules as they stood before the plan was one function, and
tests/test_env_dispatch_gpu.py launches a dozen of its rows to show that the launchers obey the plan.  The Python
restatement bench.expected_kernel is held to the probe here too, so that it has a check that needs no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX", "c++")

QUAD, PAIR, LANE = "env_step_quad_kernel", "env_pair_kernel", "env_step_kernel"
FUSED, LOOP, LOOP_SF = "env_rollout_quad_kernel", "env_step_loop_kernel", "env_step_loop_sf_kernel"


def quad(split):
    return (QUAD, -1, split, 0, 0, 0, 0)


def lane(block, static_n=1, defer=0):
    return (LANE, -1, 0, block, static_n, defer, 0)


def pair(nontemporal):
    return (PAIR, -1, 0, 0, 0, 0, nontemporal)


def fused(form):
    return (FUSED, form, 0, 0, 0, 0, 0)


def one_launch(family):
    return (family, -1, 0, 0, 0, 0, 0)


# (problem in the probe's words, (family, form, quad_split, block, static_n, lp3_defer, pair_nontemporal))
GIVEN = "policy=2 pstream=1 E=4096 "          # the pairwise kernel forced wherever it applies, on a batch it would not take
TABLE = [
    # ---- single step, ORCA, 5 humans, invisible robot: 3 envs per quad wavefront, 12 per lane-per-human wavefront
    ("E=4200", quad(1)), ("E=4201", quad(0)),                         # split up to 1400 quad wavefronts
    ("E=8400", quad(0)), ("E=8401", lane(64)),                        # quad kernel up to 2800
    ("E=49152", lane(64)), ("E=49153", lane(256)),                    # one-wavefront workgroups up to 4096 wavefronts
    # ---- 10 humans: 6 envs per wavefront, 9 neighbours
    ("N=10 E=73728", lane(64)), ("N=10 E=73729", lane(256)),          # ... up to 12 288 from 8 neighbours
    ("N=10 queue=1 E=98298", lane(256)), ("N=10 queue=1 E=98299", lane(256, defer=1)),      # deferral from 16 384
    ("N=10 E=98298", lane(256)), ("N=10 E=98299", lane(256)),         # never without a queue
    ("N=8 queue=1 E=131072", lane(256)), ("N=9 queue=1 E=131072", lane(256, defer=1)),      # ... and 8 neighbours
    ("N=8 vis=1 queue=1 E=131072", lane(256, defer=1)),
    # ---- given velocities, pair conditions met
    ("policy=2 E=49152", lane(64, 0)), ("policy=2 E=49153", pair(0)),                   # pairwise above 4096 wavefronts
    ("policy=2 E=634920", pair(0)), ("policy=2 E=634921", pair(1)),                     # non-temporal above 400 MB
    ("policy=2 N=10 E=24576", lane(64, 0)), ("policy=2 N=10 E=24577", pair(0)),
    # ---- rollout, holonomic, 5 humans: forms by workgroups of 8 envs and by quad wavefronts
    ("T=20 E=1016", fused(1)), ("T=20 E=1017", fused(2)), ("T=20 E=4096", fused(2)), ("T=20 E=4097", fused(1)),
    ("T=20 E=4608", fused(1)), ("T=20 E=4609", fused(0)), ("T=20 E=6136", fused(0)), ("T=20 E=6137", fused(2)),
    ("T=20 E=8192", fused(2)), ("T=20 E=8193", fused(0)),
    ("T=20 E=42000", fused(0)), ("T=20 E=42001", lane(64)),           # fused up to 14 000 quad wavefronts
    ("T=1 E=4096", fused(2)),                                         # (a one-step rollout is fused too)
    # ---- rollout, unicycle
    ("T=20 uni=1 E=56", fused(1)), ("T=20 uni=1 E=57", fused(2)),
    ("T=20 uni=1 E=8192", fused(2)), ("T=20 uni=1 E=8193", fused(0)),
    # ---- rollout, other quad shapes: never the four-wavefront form
    ("T=20 N=4 E=4096", fused(1)), ("T=20 N=4 vis=1 E=4096", fused(1)), ("T=20 N=1 E=30000", fused(0)),
    # ---- step loop: up to 3072 wavefronts
    ("T=20 N=10 E=18432", one_launch(LOOP)), ("T=20 N=10 E=18433", lane(64)),
    ("T=20 N=7 E=27648", one_launch(LOOP)), ("T=20 N=7 E=27649", lane(64)),
    ("T=20 N=5 vis=1 E=36864", one_launch(LOOP)), ("T=20 N=5 vis=1 E=36865", lane(64)),
    ("T=20 N=6 E=4096", one_launch(LOOP)), ("T=20 N=11 E=4096", lane(64, 0)), ("T=1 N=10 E=4096", lane(64)),
    ("T=20 N=10 policy=1 E=4096", lane(64, 0)),                       # linear humans: T steps
    ("T=20 N=5 maxn=3 E=4096", lane(64)),                             # a cut neighbour list: neither quad nor loop
    # ---- social force: the loop while the step runs one-wavefront workgroups
    ("T=20 policy=3 E=49152", one_launch(LOOP_SF)), ("T=20 policy=3 E=49153", lane(256)),
    ("T=1 policy=3 E=4096", lane(64)), ("T=20 policy=3 N=7 E=4096", one_launch(LOOP_SF)),
    ("policy=3 E=4096", lane(64)), ("policy=3 N=10 E=4096", lane(64)), ("policy=3 N=7 E=4096", lane(64, 0)),
    ("policy=1 E=4096", lane(64, 0)),

    # ---- mcn_tuning, every field each way (tests/kernel_paths.py: select_step_kernel, ROLLOUT_PATHS)
    ("qmax=0 defer=0 E=4096", lane(64)), ("qmax=0 defer=0 queue=1 N=10 E=98299", lane(256)),
    ("qmax=0 defer=1 queue=1 E=4096", lane(64, defer=1)), ("qmax=0 defer=1 E=4096", lane(64)),
    ("qmax=0 defer=1 queue=1 N=1 E=4096", lane(64)), ("qmax=0 defer=1 queue=1 N=2 E=4096", lane(64, defer=1)),
    ("defer=1 queue=1 N=10 E=4096", lane(64, defer=1)), ("defer=1 queue=1 N=11 E=4096", lane(64, 0)),
    ("defer=1 queue=1 policy=1 N=10 E=4096", lane(64, 0)),
    ("qmax=0 fg=1 E=4096", lane(64, 0)), ("qmax=0 fg=1 defer=1 queue=1 E=4096", lane(64, 0)),
    ("fg=1 E=4096", quad(1)), ("fg=1 E=8401", lane(64, 0)),          # force_generic does not stop the quad kernel
    ("qmax=1073741824 qsplit=0 E=100000", quad(0)), ("qmax=1073741824 qsplit=1 E=100000", quad(1)),
    ("qmax=1073741824 E=100000", quad(0)), ("qmax=4096 E=4096", quad(1)), ("qmax=4095 E=4096", lane(64)),
    ("qsplit=0 E=4096", quad(0)), ("qsplit=1 E=8400", quad(1)),
    ("qmax=1073741824 vis=1 E=4096", lane(64)), ("qmax=1073741824 maxn=3 E=4096", lane(64)),
    ("qmax=1073741824 N=4 vis=1 E=4096", quad(1)), ("qmax=1073741824 N=6 E=4096", lane(64)),
    ("qmax=1073741824 policy=1 E=4096", lane(64, 0)),
    ("qmax=0 block=256 E=4096", lane(256)), ("block=64 E=1000000", lane(64)), ("block=256 N=10 E=4096", lane(256)),
    # rollout_fused / rollout_split
    ("T=20 rfused=1 rsplit=0 E=4096", fused(0)), ("T=20 rfused=1 rsplit=1 E=8193", fused(1)),
    ("T=20 rfused=1 rsplit=2 E=64", fused(2)), ("T=20 rsplit=2 uni=1 E=10000", fused(2)),
    ("T=20 rfused=1 rsplit=2 N=4 E=4096", fused(1)),                  # forced form 2 without the four-wavefront kernel
    ("T=20 rfused=1 rsplit=2 N=4 vis=1 E=4096", fused(1)),
    ("T=20 rfused=1 E=42001", fused(0)), ("T=20 rfused=1 E=4096", fused(2)),
    ("T=20 rfused=0 E=4096", quad(1)), ("T=20 rfused=0 E=8401", lane(64)),
    ("T=20 rfused=1 fg=1 E=4096", quad(1)), ("T=20 fg=1 E=8401", lane(64, 0)),
    ("T=20 rfused=1 vis=1 E=4096", one_launch(LOOP)), ("T=20 rfused=1 maxn=3 E=4096", lane(64)),
    # the step loop under the tuning
    ("T=20 rfused=1 defer=0 N=10 E=4096", one_launch(LOOP)), ("T=20 rfused=1 defer=0 N=10 E=18433", lane(64)),
    ("T=20 rfused=0 N=10 E=4096", lane(64)), ("T=20 fg=1 N=10 E=4096", lane(64, 0)),
    ("T=20 rfused=1 defer=1 queue=1 N=10 E=4096", lane(64, defer=1)),
    ("T=20 rfused=1 defer=1 N=10 E=4096", lane(64)),                  # forced deferral stops the loop even without a queue
    ("T=20 block=64 N=10 E=18433", one_launch(LOOP)), ("T=20 block=64 N=10 E=1000000", one_launch(LOOP)),
    ("T=20 block=256 N=10 E=4096", lane(256)),
    ("T=20 policy=3 rfused=0 E=4096", lane(64)), ("T=20 policy=3 rfused=1 E=49153", lane(256)),
    ("T=20 policy=3 block=64 E=49153", one_launch(LOOP_SF)), ("T=20 policy=3 block=256 E=4096", lane(256)),
    ("T=20 policy=3 fg=1 E=4096", one_launch(LOOP_SF)), ("policy=3 fg=1 E=4096", lane(64, 0)),
    # pair_stream, and each reason the pairwise kernel declines
    (GIVEN, pair(0)), (GIVEN + "N=10", pair(0)), ("policy=2 pstream=0 E=49153", lane(256, 0)),
    ("policy=2 pstream=2 E=4096", pair(1)), ("policy=2 pstream=3 E=634921", pair(0)),
    ("policy=2 pstream=3 E=4096", pair(0)),
    (GIVEN + "update=0", lane(64, 0)), (GIVEN + "hh=1", lane(64, 0)), (GIVEN + "uni=1", lane(64, 0)),
    (GIVEN + "times=1", lane(64, 0)), (GIVEN + "hact=1", lane(64, 0)), (GIVEN + "fg=1", lane(64, 0)),
    (GIVEN + "disc=128", pair(0)), (GIVEN + "disc=129", lane(64, 0)), (GIVEN + "N=7", lane(64, 0)),
    ("policy=0 pstream=1 qmax=0 E=4096", lane(64)), ("policy=3 pstream=1 E=4096", lane(64)),
]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """Runs the probe on a list of problems, one output row each."""
    cxx = CXX if os.path.exists(CXX) else shutil.which(CXX)
    if not cxx:
        pytest.skip("needs a host C++ compiler")
    exe = str(tmp_path_factory.mktemp("env_dispatch") / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "env_dispatch_probe.cpp"),
                    "-o", exe], check=True)

    def run(problems):
        out = subprocess.run([exe], input="".join(p + "\n" for p in problems), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(problems)
        return [(w[0],) + tuple(int(x) for x in w[1:]) for w in (line.split() for line in out)]
    return run


def test_plan_matches_the_table(probe):
    got = probe([p for p, _ in TABLE])
    wrong = [(p, want, g) for (p, want), g in zip(TABLE, got) if g != want]
    assert not wrong, wrong


def test_table_holds_both_sides_of_every_threshold():
    """The rows the thresholds were derived for are in the table, in pairs that differ."""
    by = dict(TABLE)
    assert len(by) == len(TABLE)
    for lo, hi in [("E=4200", "E=4201"), ("E=8400", "E=8401"), ("E=49152", "E=49153"), ("N=10 E=73728", "N=10 E=73729"),
                   ("N=10 queue=1 E=98298", "N=10 queue=1 E=98299"), ("policy=2 E=49152", "policy=2 E=49153"),
                   ("policy=2 E=634920", "policy=2 E=634921"), ("T=20 E=42000", "T=20 E=42001"),
                   ("T=20 uni=1 E=56", "T=20 uni=1 E=57"), ("T=20 uni=1 E=8192", "T=20 uni=1 E=8193"),
                   ("T=20 N=10 E=18432", "T=20 N=10 E=18433"), ("T=20 N=7 E=27648", "T=20 N=7 E=27649"),
                   ("T=20 N=5 vis=1 E=36864", "T=20 N=5 vis=1 E=36865"),
                   ("T=20 policy=3 E=49152", "T=20 policy=3 E=49153")]:
        assert by[lo] != by[hi], (lo, hi)
    forms = [by["T=20 E=%d" % E][1] for E in (1016, 1017, 4096, 4097, 4608, 4609, 6136, 6137, 8192, 8193)]
    assert forms == [1, 2, 2, 1, 1, 0, 0, 2, 2, 0]


# what bench.py launches: its own env (bench.build_env: invisible holonomic robot, Explorer record with a 102-entry
# discount table, an lp3 queue) at default tuning; the given-velocity sweep counts no human-human overlaps
BENCH_ORCA = [(4096, 5, 1), (4096, 5, 20), (4096, 5, 1000), (4096, 10, 1), (4096, 10, 500), (32768, 10, 1),
              (1 << 16, 5, 1), (1 << 18, 10, 1),                                  # test_env_step_gpu.py's attribution test
              (1 << 20, 5, 1), (16384, 10, 500), (32768, 10, 500), (4096, 7, 100), (65536, 7, 100),
              (1 << 18, 10, 100)]                                                 # tests/test_bench_helpers.py
BENCH_GIVEN = [(4096, 5), (1 << 18, 5), (1 << 17, 10), (1 << 20, 5)]


def test_bench_expected_kernel_names_the_planned_family(probe):
    import bench
    rows = ["queue=1 disc=102 hh=1 E=%d N=%d T=%d" % (E, N, spl if spl > 1 else 0) for E, N, spl in BENCH_ORCA]
    rows += ["policy=2 queue=1 disc=102 E=%d N=%d" % (E, N) for E, N in BENCH_GIVEN]
    want = [bench.expected_kernel(E, N, False, spl) for E, N, spl in BENCH_ORCA]
    want += [bench.expected_kernel(E, N, True, 1) for E, N in BENCH_GIVEN]
    got = [g[0] for g in probe(rows)]
    assert got == want, [(r, g, w) for r, g, w in zip(rows, got, want) if g != w]
