"""CPU: the barrier plan of the four-wavefront rollout form (csrc/wg4_barrier_plan.hpp) and the resources of the built
env_rollout_wg4_kernel code objects.

The kernel synchronises its four wavefronts with s_barrier alone, and both of its step loops take every barrier count
from one constexpr function.  tests/wg4_barrier_probe.cpp includes that header with the host C++ compiler alone, replays
both roles over every sequence of restart flags up to length 6 and fails when the roles differ after any step or at
kernel exit.  The resource test reads the built code objects (tools/kernel_resources.py): LDS exactly 5 632 B, at most
122 / 145 VGPRs, no AGPR, scratch or spill, exactly the two instantiations."""
import os
import shutil
import subprocess

from tests.rollout_harness import ROOT, kernel_resources

CXX = os.environ.get("CXX", "c++")


def test_both_roles_execute_the_same_barriers(tmp_path):
    cxx = CXX if os.path.exists(CXX) else shutil.which(CXX)
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "wg4_barrier_probe.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    # per launch: the seed and T hand-offs; a restart flag is set in half of the 2^T sequences at each of the T steps
    assert rows == [(T, 2 ** T, 2 ** T * (T + 1) + T * 2 ** (T - 1)) for T in range(1, 7)], rows


def test_the_kernel_includes_the_plan_and_has_no_other_barrier():
    """Every workgroup barrier of env_rollout_wg4.hip goes through wg4_sync with a count of wg4_step_barriers: the one
    __syncthreads() of the file is wg4_sync's own, and there is no raw s_barrier, spin-wait or sleep in it."""
    src = open(os.path.join(ROOT, "modelcrowdnav_amd", "csrc", "env_rollout_wg4.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert '#include "wg4_barrier_plan.hpp"' in code
    assert code.count("__syncthreads()") == 1 and "s_barrier" not in code and "s_sleep" not in code
    calls = [line.strip() for line in code.splitlines() if "wg4_sync(" in line and "void wg4_sync" not in line]
    assert len(calls) == 6, calls                 # seed, hand-off and staged of the ORCA role; the same of the float64 role
    for call in calls:
        arg = call[call.index("wg4_sync(") + len("wg4_sync("):]
        assert arg.startswith(("wg4_step_barriers(", "plan.handoff", "normal.handoff")), call


def test_one_handoff_kernel_resources():
    rows = {k: v for k, v in kernel_resources("env_rollout_wg4_kernel<").items() if "env_rollout_wg4_kernel<" in k}
    assert sorted(rows) == ["void mcn::env_rollout_wg4_kernel<5, 0, false>(mcn::StepParams, int)",
                            "void mcn::env_rollout_wg4_kernel<5, 0, true>(mcn::StepParams, int)"], sorted(rows)
    for name, (vgpr, agpr, sgpr, scratch, lds, vspill) in rows.items():
        print("%s: vgpr %d sgpr %d scratch %d lds %d" % (name, vgpr, sgpr, scratch, lds))
        assert (agpr, scratch, vspill) == (0, 0, 0), (name, rows[name])
        assert lds == 5632, (name, lds)
        assert vgpr <= (145 if "true" in name else 122), (name, vgpr)
