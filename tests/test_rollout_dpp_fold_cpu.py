"""No GPU (needs hipcc): what the four-wavefront rollout kernel's translation unit compiles to after the quad broadcasts
of the rank were folded into their subtractions and the 3-D LP candidate's take steps went lean (quad_common.hpp:
Path::fold_rank, Path::lean_lp3).

env_rollout_wg4.hip is compiled to gfx950 assembly with the Makefile's flags (tools/isa_census.py reads them from the
Makefile) and both instantiations are held against the parent commit's figures (profiles/r31_rollout_dpp_fold.txt):
  * resources: at most 120 (holonomic) / 145 (unicycle) VGPRs, 5 632 B of LDS, no scratch, no spill;
  * the ORCA wavefronts' step loop (the outermost loop with the fewest float64 instructions) has no more static
    instructions than the parent's 861, in either instantiation;
  * the rank's four differences are four v_sub_u32_dpp, and the register they read through DPP is written by none of the
    two instructions in front of the first of them (the wait states a DPP read of a fresh VGPR needs, which the compiler
    places for instructions it emits itself);
  * no other translation unit takes the folded forms: QuadDpp has every tag false."""
import os
import re
import shutil

import pytest

from tests.rollout_harness import ROOT
from tools import isa_census as IC

CSRC = os.path.join(ROOT, "modelcrowdnav_amd", "csrc")
PARENT_ORCA_LOOP = 861           # both instantiations, counted at the parent commit
VGPR_CAP = {"false": 120, "true": 145}
LDS = 5632


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not (os.path.exists(IC.HIPCC) or shutil.which("hipcc")):
        pytest.skip("needs hipcc")
    out = str(tmp_path_factory.mktemp("wg4") / "env_rollout_wg4.s")
    IC.compile_asm(os.path.join(CSRC, "env_rollout_wg4.hip"), out)
    return out


def _kernel(asm, unicycle):
    return IC.kernel_lines(asm, "env_rollout_wg4_kernel<5, 0, %s>" % unicycle)


def _orca_loop(lines):
    """blocks of the outermost loop with the fewest float64 instructions: the ORCA role's step loop"""
    loops = IC.outer_loops(IC.parse_blocks(lines))
    f64 = lambda bl: sum(1 for b in bl for i in b[3] if re.match(r"^v_\w+_f64", i))
    return min(loops.values(), key=f64)


@pytest.mark.parametrize("unicycle", ["false", "true"])
def test_resources(asm, unicycle):
    name, _ = _kernel(asm, unicycle)
    text = open(asm).read()
    sym = next(l.split(":")[0] for l in text.split("\n") if re.match(r"^_Z\w+:", l) and
               IC.demangle([l.split(":")[0]])[0] == name)
    # the kernel's entry of the code object's metadata (amdhsa.kernels: one `- .args:` item per kernel)
    entry = next(e for e in text[text.index("amdhsa.kernels:"):].split("\n  - .a") if re.search(r"\.name:\s+%s\n" % sym, e))
    field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, entry).group(1))
    got = {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    print(name, got)
    assert got["vgpr_count"] <= VGPR_CAP[unicycle]
    assert got["vgpr_spill_count"] == 0 and got["private_segment_fixed_size"] == 0
    assert got["group_segment_fixed_size"] == LDS


@pytest.mark.parametrize("unicycle", ["false", "true"])
def test_orca_loop_census_not_above_the_parent(asm, unicycle):
    _, lines = _kernel(asm, unicycle)
    total = sum(len(b[3]) for b in _orca_loop(lines))
    print("ORCA loop, unicycle=%s: %d static instructions (parent %d)" % (unicycle, total, PARENT_ORCA_LOOP))
    assert total <= PARENT_ORCA_LOOP


@pytest.mark.parametrize("unicycle", ["false", "true"])
def test_rank_is_four_folded_subtractions_with_their_wait_states(asm, unicycle):
    _, lines = _kernel(asm, unicycle)
    ins = [i for b in _orca_loop(lines) for i in b[3]]
    subs = [n for n, i in enumerate(ins) if i.startswith("v_sub_u32_dpp")]
    assert len(subs) == 4 and subs == list(range(subs[0], subs[0] + 4)), [ins[n] for n in subs]
    perms = sorted(re.search(r"quad_perm:\[(\d),", ins[n]).group(1) for n in subs)
    assert perms == ["0", "1", "2", "3"]
    src = {re.match(r"v_sub_u32_dpp v\d+, (v\d+), (v\d+)", ins[n]).groups() for n in subs}
    assert len(src) == 1, src                                    # key(lane I) - key: one register, read both ways
    key = src.pop()[0]
    for back in (1, 2):
        dst = ins[subs[0] - back].split()[1].rstrip(",")
        assert dst != key, (ins[subs[0] - back], ins[subs[0]])
    # the plain broadcasts of the key are gone with them
    assert not [i for i in ins[max(subs[0] - 8, 0):subs[0]] if i.startswith("v_mov_b32_dpp") and key in i.split()[2]]


def test_only_the_table_path_is_tagged():
    """QuadDpp, the path of every other kernel, has both tags false (that their code is unchanged is shown by their object
    files, byte-identical to the parent's: profiles/r31_rollout_dpp_fold.txt)."""
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(CSRC, "quad_common.hpp")).read().splitlines())
    dpp = code[code.index("struct QuadDpp"):code.index("struct QuadTable")]
    tab = code[code.index("struct QuadTable"):]
    tab = tab[:tab.index("};")]
    for tag in ("fold_rank", "lean_lp3"):
        assert re.search(r"\b%s\s*=\s*false\b" % tag, dpp) and re.search(r"\b%s\s*=\s*true\b" % tag, tab), tag
