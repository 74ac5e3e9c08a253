#!/usr/bin/env python3
"""Instruction budget of the hand-written anchor loop of chain_dp_tile (csrc/chain_dp_tile.h, MM2C_SCAN_TILE_ASM): expands the string
macros of the header (for the headline's instantiation unless told otherwise: compact x / q ring, packed f / p ring, lean), cuts the sequence at its labels and counts the instructions of every block by issue class (the classes of
tools/ubench/issue_rate.hip: plain VALU / VALU that involves the scalar side / SALU / branch / LDS / VMEM / waits).  The blocks are then
summed along the paths an anchor takes, so that the per-anchor PMC figures of profiles/r2_mixed.md can be decomposed.
    python tools/isa_budget.py [--tab] [--far] [--wide | --pairs | --q24] > profiles/r2_isa_budget.md
The macros are expanded by the C preprocessor (cpp) from the header's own #define lines."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.environ.get("MM2C_TILE_HEADER") or os.path.join(ROOT, "minimap2-fpga_amd/csrc/chain_dp_tile.h")   # (another revision's header, to set two budgets side by side)
CPP = os.environ.get("CPP", "cpp")


def directives(src):
    """the preprocessor lines of the header (with their continuation lines), without #include and #pragma: every string macro the loop is made of"""
    out, cont = [], False
    for line in src.split("\n"):
        if cont or (line.startswith("#") and not line.startswith(("#include", "#pragma"))):
            out.append(line)
            cont = line.rstrip().endswith("\\")
        else:
            cont = False
    return "\n".join(out) + "\n"


def loop_text(tab, far, ring):
    """the instruction text of one instantiation of MM2C_SCAN_TILE_ASM, expanded by the C preprocessor itself (so the tool follows whatever the macros say)"""
    inst = "MM2C_SCAN_TILE_ASM_(scan, %s, 0, MM2C_RING_%s, MM2C_SCORE_%s, MM2C_ADDF_%s, %s, %s)\n" % (
        "true" if tab else "false", ring, "TAB" if tab else "CMP", "TAB" if tab else "CMP", "MM2C_SWAIT_TAB" if tab else '""', "MM2C_FARS" if far else "MM2C_LEAN")
    src = directives(open(HEADER).read())
    # the header's include guard closes at its end: the instantiation goes in front of the last #endif
    k = src.rstrip().rfind("#endif")
    out = subprocess.run([CPP, "-P", "-w", "-DMM2C_PROBE=0", "-"], input=src[:k] + inst + src[k:], capture_output=True, text=True, check=True).stdout
    body = out[out.index("asm volatile(") + len("asm volatile("):]
    body = body[:body.index(": [best]")]
    return "".join(m.group(1) for m in re.finditer(r'"((?:[^"\\]|\\.)*)"', body)).replace("\\n", "\n").replace("\\t", " ")


def classify(ins):
    op = ins.split()[0]
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("v_"):
        scalar_side = (op.startswith(("v_cmp", "v_readlane", "v_writelane", "v_readfirstlane", "v_mbcnt")) or "_dpp" in op or "row_" in ins or "wave_" in ins
                       or (op.startswith("v_cndmask") and "e64" in op))
        return "valu_s" if scalar_side else "valu"
    return "other"


def blocks(tab, far=False, ring="P"):
    """[(label, instructions)] in the order of the text; ring: W 32-bit x / q ring, C compact, P compact with the packed f / p ring (the headline's), Q q24"""
    out, cur = [], ("entry", [])
    for line in loop_text(tab, far, ring).split("\n"):
        line = line.strip()
        if not line:
            continue
        m = re.match(r"(L[a-z0-9]+)_%=:", line)
        if m:
            out.append(cur); cur = (m.group(1), [])
        else:
            cur[1].append(line)
    out.append(cur)
    return out


CLASSES = ("valu", "valu_s", "salu", "branch", "lds", "vmem", "wait")


def count(instrs):
    c = dict.fromkeys(CLASSES, 0)
    for i in instrs:
        c[classify(i)] += 1
    return c


def cut(instrs, until=None, after=None):
    """instructions up to and including the first one that starts with `until`, or those behind the first one starting with `after`"""
    if until:
        for k, i in enumerate(instrs):
            if i.startswith(until):
                return instrs[:k + 1]
    if after:
        for k, i in enumerate(instrs):
            if i.startswith(after):
                return instrs[k + 1:]
    return instrs


if __name__ == "__main__":
    tab, far = "--tab" in sys.argv, "--far" in sys.argv
    ring = "W" if "--wide" in sys.argv else "C" if "--pairs" in sys.argv else "Q" if "--q24" in sys.argv else "P"
    bl = blocks(tab, far, ring)
    B = dict(bl)
    order = [n for n, _ in bl]
    name = {"W": "32-bit x / q ring", "C": "compact x / q ring, f / p pairs", "P": "compact x / q ring, packed f / p ring", "Q": "q24 ring"}[ring]
    print(f"# Instruction budget of the hand-written anchor loop (`scan_tile_asm_{'tab' if tab else 'cmp'}{'_far' if far else ''}{ {'W': '', 'C': '_c', 'P': '_p', 'Q': '_q'}[ring] }`: {name}), from `tools/isa_budget.py`\n")
    print("Classes as measured by `tools/ubench/issue_rate.hip` (`profiles/r2_issue_rate.md`): plain VALU ≈0.84 per SIMD and ns; VALU that involves the scalar side")
    print("(`v_cmp`, `v_readlane`/`v_writelane`, DPP, `v_cndmask` with an SGPR mask, `v_mbcnt`) and SALU ≈0.55; `ds_read` 0.29.\n")
    print("## Blocks between labels (straight-line instruction counts)\n")
    print("| block | plain VALU | scalar-side VALU | SALU | branch | LDS | VMEM | waitcnt / nop |")
    print("|---|---|---|---|---|---|---|---|")
    for n in order:
        c = count(B[n])
        print(f"| `{n}` | " + " | ".join(str(c[k]) for k in CLASSES) + " |")

    def path(*parts):
        tot = dict.fromkeys(CLASSES, 0)
        for p in parts:
            for k, v in count(p).items():
                tot[k] += v
        return tot

    fixed = path(cut(B["Lk"], until="s_cbranch_scc0 Lloop"), cut(B["Ldone"], until="s_cbranch_scc0 Lk"))
    own = path(cut(cut(B["Lk"], after="s_cbranch_scc0 Lloop"), until="s_cbranch_scc0 Lloop"))
    own_scored = path(cut(cut(cut(B["Lk"], after="s_cbranch_scc0 Lloop"), after="s_cbranch_scc0 Lloop"), until="s_branch Lhf"))
    empty = path(cut(B["Lloop"], until="s_cbranch_vccz"))
    ring_scored = path(cut(B["Lloop"], after="s_cbranch_vccz"), B["Lold"])                                    # ... up to the fold (Lhf)
    back = [cut(B["Lfat"], until="s_cbranch_scc0 Lret"), cut(B["Lret"], until="s_cbranch_scc0 Lloop")] if far else [cut(B["Lfat"], until="s_cbranch_scc0 Lloop")]
    fold_a = path(B["Lhf"], *back)
    b0_exit = path(cut(B["Lhf"], until="s_cbranch_vccnz Limp"), cut(B["Limp"], until="s_cbranch_scc1 Ldone"))
    b0_stay = path(cut(B["Lhf"], until="s_cbranch_vccnz Limp"), B["Limp"], cut(B["Lb0s"], until="s_cbranch_scc0"))
    part = path(cut(B["Lpart"], until="s_cbranch_scc0 Lend"))
    part_scored = path(B["Lpart"])
    deep = path(cut(B["Lfg"], until="s_branch Lhf"))
    print("\n## Paths\n")
    print("| path | plain VALU | scalar-side VALU | SALU | branch | LDS | VMEM | waitcnt / nop |")
    print("|---|---|---|---|---|---|---|---|")
    for name, c in (("per anchor, fixed: scalars by `v_readfirstlane` under a one-hot exec, first x / q request, commit by `v_mov` under the same mask", fixed),
                    ("+ own-tile chunk, no lane passes the filters", own),
                    ("+ own-tile chunk with a surviving lane, up to the fold (`Lhf`)", own_scored),
                    ("per older tile, no lane passes (`Lloop` … `s_cbranch_vccz`)", empty),
                    ("per older tile with a surviving lane, f / p from the LDS ring, up to the fold", ring_scored),
                    ("... its f / p from memory instead (`Lfg`), in addition", deep),
                    ("fold A: stamps, marks, no lane beats the best, back to the loop", fold_a),
                    ("fold B0 that takes the score-bound exit (no stamps)", b0_exit),
                    ("fold B0 that stays: stamps, marks, closed-form counter, no mark", b0_stay),
                    ("the ring window runs out with no partly covered tile (`Lpart` … `Lend`)", part),
                    ("the partly covered tile with a surviving lane, up to `Lold`", part_scored)):
        print(f"| {name} | " + " | ".join(str(c[k]) for k in CLASSES) + " |")
