"""Static instruction census of a kernel's step loop, by instruction class (no GPU needed).

    python tools/isa_census.py [--src modelcrowdnav_amd/csrc/env_rollout_quad.hip]
                               [--kernel 'env_rollout_quad_kernel<5, 0, false, true>'] [--asm FILE] [--list]

Cross-compiles one translation unit for gfx950 with the Makefile's HIPFLAGS plus `--cuda-device-only -S`, takes the
kernel whose demangled name contains --kernel, and classifies the instructions of two regions of its step loop (the
outermost loop that has a child loop):

    common    every instruction from the step loop's header up to the first block of the child loop (for the quad
              rollout kernel: top of the step through the speculative 2-D LP to the 3-D LP entry)
    lp3 round every instruction in the blocks of the child loop (one round of the quad 3-D LP: next line, the
              quad's candidate, take)

Both are text ranges: the out-of-line IEEE fall-backs of fast_f32.hpp's range guards that the compiler places inside
them are counted too (column `fallback`: how many of the region's instructions sit in such blocks, i.e. blocks with a
v_sqrt_f32 or a v_div_scale_f32 of 1.0).  Static counts, not a measurement of time.

The default kernel is the two-wavefront form.  The four-wavefront form (env_rollout_wg4_kernel, what 4096 envs x 5
humans now run; --src modelcrowdnav_amd/csrc/env_rollout_wg4.hip) has one step loop per role and no single nest for
this census to pick: use --loops there, which
prints one row per outermost loop (text range from its first to its last block, child loops and rare blocks placed
inside it included) with the number of float64 instructions in it: the float64 role's step loop is the row with most.
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modelcrowdnav_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CLASSES = ["arith", "sel/mov", "v_cmp", "salu_mask", "salu_other", "s_nop", "dpp", "lds", "other"]
MASK_OP = re.compile(r"^s_(and|or|andn2|orn2|xor|xnor|nand|nor)_b64$")
ARITH = re.compile(r"^v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|min|max|min3|max3|med3|rcp|rsq|sqrt|div_\w+|ldexp|frexp_\w+|"
                   r"fract|floor|ceil|trunc|rndne|cvt_\w+|exp|log|sin|cos)(_legacy)?_(f32|f64|f16)(_e32|_e64|_dpp)?$")


def hipflags(src=None):
    """HIPFLAGS as the Makefile sets them (the Makefile is the one place the product flags live), with what it adds
    for the object of `src` alone (`<objects>: HIPFLAGS += ...`)."""
    txt = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", txt, re.M)
    flags = m.group(1).replace("$(ARCH)", "gfx950")
    if src:
        obj = os.path.splitext(os.path.basename(src))[0] + ".o"
        for targets, extra in re.findall(r"^([^#\n:]+):\s*HIPFLAGS\s*\+=\s*(.*)$", txt, re.M):
            if obj in targets.split():
                flags += " " + extra
    return shlex.split(flags)


def compile_asm(src, out):
    cmd = [HIPCC] + hipflags(src) + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC, stderr=subprocess.DEVNULL)


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.split("\n")


def kernel_lines(asm, want):
    lines = open(asm).read().split("\n")
    heads = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    dem = demangle([n for _, n in heads])
    hits = [(i, d) for (i, _), d in zip(heads, dem) if want in d]
    if len(hits) != 1:
        sys.exit("isa_census: %d kernels match %r: %s" % (len(hits), want, [d for _, d in hits][:8]))
    start, name = hits[0]
    # up to the end of the function, not the first s_endpgm: a kernel whose roles branch apart ends more than once
    end = next(j for j in range(start, len(lines)) if lines[j].startswith(".Lfunc_end"))
    return name, lines[start:end]


def parse_blocks(lines):
    """[(label, loop header it belongs to or None, depth, [instructions])] in text order."""
    blocks = []
    cur = None
    for l in lines:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):(.*)$", l)
        if m:
            label = m.group(1).lstrip(".").replace("; %", "")
            hdr = re.search(r"Header=(\w+) Depth=(\d+)", m.group(2))
            own = re.search(r"Loop Header: Depth=(\d+)", m.group(2))
            if own:
                cur = [label, label.replace("LBB", "BB"), int(own.group(1)), []]
            elif hdr:
                cur = [label, hdr.group(1), int(hdr.group(2)), []]
            else:
                cur = [label, None, 0, []]
            blocks.append(cur)
            continue
        own = re.search(r"Loop Header: Depth=(\d+)", l)
        if own and cur is not None and not cur[3] and l.lstrip().startswith(";"):
            cur[1], cur[2] = cur[0].replace("LBB", "BB"), int(own.group(1))      # header comment on its own line
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":") or cur is None:
            continue
        cur[3].append(t)
    return blocks


def classify(ins):
    op = ins.split()[0]
    if op.startswith("ds_"):
        return "lds"
    if "dpp" in op or re.search(r"\b(quad_perm|row_\w+):", ins):
        return "dpp"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("v_cmp"):
        return "v_cmp"
    if MASK_OP.match(op):
        return "salu_mask"
    if op.startswith("s_"):
        return "salu_other"
    if op.startswith("v_cndmask") or op.startswith("v_mov") or op.startswith("v_pk_mov"):
        return "sel/mov"
    if ARITH.match(op):
        return "arith"
    return "other"


def is_fallback(ins):
    return any(i.startswith("v_sqrt_f32") or (i.startswith("v_div_scale_f32") and i.endswith(", 1.0")) for i in ins)


def census(blocks):
    loops = {}
    for b in blocks:
        if b[1] is not None:
            loops.setdefault(b[1], b[2])
    inner = [h for h, d in loops.items() if d == 2]
    outer = [h for h, d in loops.items() if d == 1]
    if not inner or not outer:
        sys.exit("isa_census: no loop nest found (outer %s, inner %s)" % (outer, inner))
    inner_h = inner[0]
    parent = next(h for h in outer if any(b[1] == h for b in blocks))
    first_outer = next(i for i, b in enumerate(blocks) if b[1] == parent)
    in_inner = [i for i, b in enumerate(blocks) if b[1] == inner_h]
    common = range(first_outer, in_inner[0])
    return {"common": [blocks[i] for i in common], "lp3 round": [blocks[i] for i in in_inner]}


def outer_loops(blocks):
    """{header: blocks of the text range of that depth-1 loop}, in text order."""
    out = {}
    for h in [b[1] for b in blocks if b[1] is not None and b[2] == 1]:
        if h not in out:
            idx = [i for i, b in enumerate(blocks) if b[1] == h]
            out[h] = blocks[idx[0]:idx[-1] + 1]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--src", default=os.path.join(CSRC, "env_rollout_quad.hip"))
    ap.add_argument("--kernel", default="env_rollout_quad_kernel<5, 0, false, true>")
    ap.add_argument("--asm", help="use this gfx950 assembly file instead of compiling --src")
    ap.add_argument("--list", action="store_true", help="also print every block with its count")
    ap.add_argument("--loops", action="store_true", help="one row per outermost loop instead of the common / lp3 regions")
    args = ap.parse_args()
    if args.asm:
        asm = args.asm
    else:
        tmp = tempfile.mkdtemp(prefix="isa_census_")
        asm = os.path.join(tmp, "tu.s")
        compile_asm(os.path.abspath(args.src), asm)
    name, lines = kernel_lines(asm, args.kernel)
    regions = outer_loops(parse_blocks(lines)) if args.loops else census(parse_blocks(lines))
    print("kernel: %s" % name)
    print("%-10s %6s " % ("region", "total") + " ".join("%10s" % c for c in CLASSES) + " %9s" % "fallback" +
          (" %6s" % "f64" if args.loops else ""))
    for reg, bl in regions.items():
        counts = dict.fromkeys(CLASSES, 0)
        total = fb = 0
        for b in bl:
            for i in b[3]:
                counts[classify(i)] += 1
            total += len(b[3])
            fb += len(b[3]) if is_fallback(b[3]) else 0
        f64 = sum(1 for b in bl for i in b[3] if re.match(r"^v_\w+_f64", i))
        print("%-10s %6d " % (reg, total) + " ".join("%10d" % counts[c] for c in CLASSES) + " %9d" % fb +
              (" %6d" % f64 if args.loops else ""))
        if args.list:
            for b in bl:
                print("    %-12s %4d%s" % (b[0], len(b[3]), "  fallback" if is_fallback(b[3]) else ""))


if __name__ == "__main__":
    main()
