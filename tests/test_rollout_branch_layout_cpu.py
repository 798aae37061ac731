"""No GPU (needs hipcc): where the compiler puts the blocks of the four-wavefront rollout kernel's ORCA step once the range
guards compute their fast values first and replace them under a branch marked unlikely (quad_common.hpp: Path::straight;
fast_f32.hpp: FAST_FIRST).

env_rollout_wg4.hip is compiled to gfx950 assembly with the Makefile's flags (tools/isa_census.py) and, for both
instantiations, the instructions a normal step executes -- no restart, no 3-D LP, every used operand inside the fast
ranges -- are walked from the ORCA loop's header to the hand-off s_barrier:
  * no v_sqrt_f32 on the way (the IEEE roots are out of line);
  * no unconditional s_branch on the way (no trampoline that comes back);
  * every s_cbranch_* on the way whose target lies outside that text targets a label BEHIND the barrier and falls through;
  * ONE taken branch: the s_cbranch_execz over the 3-D LP's round loop, which stays in line.  Marking the 3-D LP entry
    unlikely puts the loop behind the barrier and makes the step a straight line (counted: 845 / 845), but on the GPU that
    part measured nothing on its own or on top of the guards, and it made the unicycle form 1.5 - 2 % slower per step (the
    changed block frequencies rearrange that form's float64 loop), so it is not in the tree
    (profiles/r32_rollout_branch_layout.txt).  The walk follows that one branch and allows no other;
  * the ORCA loop's static count is not above the parent's 852 (holonomic) / the standing cap of 861 (unicycle)."""
import os
import re
import shutil

import pytest

from tests.rollout_harness import ROOT
from tools import isa_census as IC

CSRC = os.path.join(ROOT, "modelcrowdnav_amd", "csrc")
ORCA_LOOP_CAP = {"false": 852, "true": 861}      # the parent's holonomic count; test_rollout_dpp_fold_cpu's cap


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(IC.HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    out = str(tmp_path_factory.mktemp("wg4") / "env_rollout_wg4.s")
    IC.compile_asm(os.path.join(CSRC, "env_rollout_wg4.hip"), out)
    return out


def _f64(blocks):
    return sum(1 for b in blocks for i in b[3] if re.match(r"^v_\w+_f64", i))


def _step(asm, unicycle):
    """(every block of the kernel, index of the ORCA loop's header block, (block, instruction) of the hand-off barrier,
    blocks of the ORCA loop's text range).  The ORCA loop is the outermost loop with the fewest float64 instructions, as in
    test_rollout_dpp_fold_cpu."""
    _, lines = IC.kernel_lines(asm, "env_rollout_wg4_kernel<5, 0, %s>" % unicycle)
    blocks = IC.parse_blocks(lines)
    loops = IC.outer_loops(blocks)
    hdr = min(loops, key=lambda h: _f64(loops[h]))
    first = next(n for n, b in enumerate(blocks) if b[0].replace("LBB", "BB") == hdr)
    bar = next((n, m) for n in range(first, len(blocks)) for m, i in enumerate(blocks[n][3]) if i.startswith("s_barrier"))
    return blocks, first, bar, loops[hdr]


def _walk(blocks, first, bar):
    """-> ([(block index, instruction)] a normal step executes from the loop header to the hand-off barrier, the taken
    branches among them).  A conditional branch to a later block of this text is followed only where it jumps over the 3-D
    LP's round loop (blocks of depth 2 in between); every other one falls through."""
    where = {b[0].replace("LBB", "BB"): n for n, b in enumerate(blocks)}
    path, taken, n = [], [], first
    while n <= bar[0]:
        jump = None
        for i in blocks[n][3]:
            path.append((n, i))
            if i.startswith("s_barrier"):
                return path, taken
            if i.startswith("s_cbranch_"):
                tgt = where[i.split()[1].lstrip(".").replace("LBB", "BB")]
                if first <= tgt <= bar[0]:
                    assert tgt > n, (i, "a backward branch inside the step")
                    if any(blocks[m][2] == 2 for m in range(n + 1, tgt)):
                        taken.append((n, i))
                        jump = tgt
                        break
                else:
                    assert tgt > bar[0], (i, "leaves the step to a block in front of it")
        n = jump if jump is not None else n + 1
    raise AssertionError("no s_barrier on the path")


@pytest.mark.parametrize("unicycle", ["false", "true"])
def test_normal_step_takes_one_branch(asm, unicycle):
    blocks, first, bar, loop = _step(asm, unicycle)
    path, taken = _walk(blocks, first, bar)
    print("unicycle=%s: %d instructions on a normal step's path from the loop header to the hand-off barrier" % (
        unicycle, len(path)))
    for n, i in path:
        if i.startswith("s_cbranch_"):
            print("    %-18s in %-9s %s" % (i.split()[0], blocks[n][0], "TAKEN (3-D LP skip)" if (n, i) in taken else "falls through"))
    assert not [i for _, i in path if i.startswith("v_sqrt_f32")]
    assert not [i for _, i in path if i.split()[0] == "s_branch"]
    assert len([i for _, i in path if i.startswith("s_cbranch_scc")]) >= 3      # the three guards of the 2-D LP path
    assert len(taken) == 1 and taken[0][1].startswith("s_cbranch_execz"), taken


@pytest.mark.parametrize("unicycle", ["false", "true"])
def test_orca_loop_census(asm, unicycle):
    _, _, _, loop = _step(asm, unicycle)
    total = sum(len(b[3]) for b in loop)
    print("ORCA loop, unicycle=%s: %d static instructions (cap %d)" % (unicycle, total, ORCA_LOOP_CAP[unicycle]))
    assert total <= ORCA_LOOP_CAP[unicycle]


def test_only_the_table_path_is_tagged():
    """QuadDpp, the path of every other kernel, has the tag false and the wrappers default to the parent's form."""
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, "quad_common.hpp")).read().splitlines())
    dpp = code[code.index("struct QuadDpp"):code.index("struct QuadTable")]
    tab = code[code.index("struct QuadTable"):]
    tab = tab[:tab.index("};")]
    assert re.search(r"\bstraight\s*=\s*false\b", dpp) and re.search(r"\bstraight\s*=\s*true\b", tab)
    fast = open(os.path.join(CSRC, "fast_f32.hpp")).read()
    assert len(re.findall(r"template <bool FAST_FIRST = false, class U = bool>", fast)) == 2      # sqrt_f32 and rcp_sqrt_f32: the two wrappers on this path
