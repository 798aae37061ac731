"""CPU: the take step of the quad-parallel incremental LP (csrc/quad_take_plan.hpp).

The four-wavefront rollout form decides each of its four take steps from min(fail, code_i), which is known before the
step's test, instead of from `fail` behind it (take_step_lean); every other caller keeps the guarded form.
tests/quad_take_probe.cpp includes the header with the host C++ compiler alone and replays both forms over every input of
the four-line and the three-line sequence, comparing `fail` and the running point after every step.  The counts it prints
are held against a derivation that uses neither function: with every test bit and every verdict bit uniform and
independent, the walk "lowest violated line above the point; infeasible: stop and fail; else move there" is a small
Markov chain over the lines."""
import os
import shutil
import subprocess
from fractions import Fraction

from tests.rollout_harness import ROOT

CXX = os.environ.get("CXX", "c++")
CSRC = os.path.join(ROOT, "modelcrowdnav_amd", "csrc")


def _expected(nl):
    """(ended at the start, at c_0 .. c_3, failed) as fractions of all inputs for a sequence over lines 0 .. nl - 1: from a
    point with index j (-1: the start) line n > j is the lowest violated one with probability 2^-(n - j); half of those are
    infeasible (the walk ends where it is, failed), the other half move it to c_n; with 2^-(nl - 1 - j) none is violated."""
    reach = {j: Fraction(0) for j in range(-1, 4)}
    ends = {j: Fraction(0) for j in range(-1, 4)}
    reach[-1], failed = Fraction(1), Fraction(0)
    for j in range(-1, 4):
        stay = Fraction(1, 2 ** max(nl - 1 - j, 0))
        for n in range(j + 1, nl):
            p = reach[j] * Fraction(1, 2 ** (n - j))
            reach[n] += p / 2
            failed += p / 2
            stay += Fraction(1, 2 ** (n - j)) / 2
        ends[j] = reach[j] * stay
    assert sum(ends.values()) == 1
    return [ends[j] for j in range(-1, 4)], failed


def test_lean_and_guarded_steps_agree_on_every_input(tmp_path):
    cxx = CXX if os.path.exists(CXX) else shutil.which(CXX)
    assert cxx, "needs a host C++ compiler"
    exe = str(tmp_path / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "quad_take_probe.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    total = 16 * 2 ** 16
    want = []
    for lines, nl in [(4, 0), (4, 1), (4, 2), (4, 3), (4, 4), (3, 3)]:
        ends, failed = _expected(nl)
        want.append((lines, nl, total) + tuple(int(e * total) for e in ends) + (int(failed * total),))
        assert all((e * total).denominator == 1 for e in ends)
    assert rows == want, (rows, want)


def test_only_the_table_path_takes_the_lean_step():
    """QuadDpp, every caller but the four-wavefront form, keeps the guarded steps (their census is pinned by
    tests/test_quad_lp3_lean.py); QuadTable runs take_step_lean, the function the probe replays."""
    src = open(os.path.join(CSRC, "quad_common.hpp")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert '#include "quad_take_plan.hpp"' in code
    dpp = code[code.index("struct QuadDpp"):code.index("struct QuadTable")]
    tab = code[code.index("struct QuadTable"):code.index("struct QuadTable") + 200]
    assert "lean_take = false" in dpp and "lean_take = true" in tab
    assert code.count("take_step_lean(") == 1 and "if constexpr (Path::lean_take)" in code
    hdr = open(os.path.join(CSRC, "quad_take_plan.hpp")).read()
    assert "hip" not in "\n".join(line.split("//")[0] for line in hdr.splitlines()).lower()
