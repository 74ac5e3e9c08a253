"""Regions-to-hits cases at the limits of the kernel's own implementation (csrc/chain_hits.hip), in the shape of tests/hits_data.py: {"name", "opt", "regs"}.  The
fixture tests/golden/ref_hits_limits.npz stores what the reference's hit.o made of them (make_ref_hits_fixtures.py hits_limit_data ref_hits_limits.npz).

The one part of the kernel that is not the reference's algorithm is uncov_len: a measure over candidate gap starts (the region's start and every clipped interval's
end), 64 candidates per round, instead of a sort and a sweep.  The region's start is candidate number n_cov, so it has a round of its own exactly when n_cov is a
multiple of 64; of several intervals that end at one place only the first in w order may open the gap behind it.

A pair of cases pins uncov_len from both sides through mask_len (hit.c:165 asks uncov_len <= mask_len): with `un` the value of the sorted sweep, the same regions run
once at mask_len = un ("_child": the last region passes and is a child) and once at un - 1 ("_primary": it fails and becomes a primary).  A measure that comes out too
small flips the second, one that comes out too large the first.

FAMILY maps every case to its family; tests/test_cpu_hits_limit_data.py checks the population condition each family is named for."""
import re

from hits_data import LDS_CLASS, batch, cat, disjoint, groups as _groups, opt, opt_key, reg  # noqa: F401  (batch, opt_key: for the users of this module)

ROUND = 64                                                                     # candidates, and primaries, of one round of the wave
GAP_N = (63, 64, 65, 127, 128, 129, 192)
PASS_AT = (63, 64, 127, 128)

_CASES = None
FAMILY = {}                                                                    # case name -> its family: the name without its size and side
PIN = {}                                                                       # case stem -> (index of the pinned region, un of the sweep)


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = []

    def add(name, o, regs):
        C.append({"name": name, "opt": o, "regs": regs})
        FAMILY[name] = re.sub(r"(_\d+(_and_\d+)?)?(_child|_primary)?$", "", name) if not name.startswith(("kept_", "best_n_")) else name

    def pair(stem, regs, un, **kw):
        """the last region of regs at mask_len = un and un - 1"""
        PIN[stem] = (len(regs) - 1, un)
        add(stem + "_child", opt(mask_len=un, **kw), cat(*regs))
        add(stem + "_primary", opt(mask_len=un - 1, **kw), cat(*regs))

    for n in GAP_N:
        # n disjoint primaries of 90 with gaps of 10, the first at 100: the region's own start is uncovered, n_cov = n
        prim = [reg(100 + 100 * j, 190 + 100 * j, 5000 - j, cnt=5 + j % 7) for j in range(n)]
        pair(f"start_gap_{n}", prim + [reg(0, 100 * n + 100, 3000, cnt=9)], 100 + 10 * n)
        # the same with the first primary at the region's start: the candidate qs_i opens nothing
        prim = [reg(100 * j, 100 * j + 90, 5000 - j, cnt=5 + j % 7) for j in range(n)]
        pair(f"start_covered_{n}", prim + [reg(0, 100 * n, 3000, cnt=9)], 10 * n)
    # two primaries that end at 1000 (the second is one because its value against the first is exactly 0.5), a gap of 200 behind them
    pair("equal_ends", [reg(500, 1000, 900), reg(0, 1000, 800), reg(200, 1200, 700)], 200)
    # ... with 64 small primaries between the two in w order, inside the third region's extent: the two equal ends are candidates 0 and 65
    small = [reg(10100 + 20 * j, 10110 + 20 * j, 850 - j) for j in range(ROUND)]
    pair("equal_ends_across_rounds", [reg(5000, 10000, 900)] + small + [reg(0, 10000, 780), reg(2000, 12000, 700)], 100 + 10 * (ROUND - 1) + 630)
    # three primaries with one end; the third is a primary because its own uncov_len, 300, is above mask_len
    pair("equal_ends_triple", [reg(1500, 2000, 900), reg(1000, 2000, 800), reg(700, 2000, 750), reg(1200, 2200, 700)], 200)
    # two primaries that reach beyond qe_i: every clipped end is qe_i, only qs_i opens a gap
    pair("clipped_to_end", [reg(1000, 3000, 900), reg(2500, 5000, 800), reg(900, 2600, 700)], 100)
    for n in (65, 129):                                                        # touching primaries: uncov_len = 0 over more than one round of candidates
        add(f"tiled_{n}", opt(mask_len=0), cat(*([reg(100 * j, 100 * j + 100, 5000 - j, cnt=5 + j % 7) for j in range(n)] +
                                                   [reg(0, 100 * n, 3000, cnt=9), reg(50, 100 * n - 50, 2900, cnt=9)])))
    # the only passing primary at w index k: the last lane of a ballot and the first lane of the next; then one more primary and a child of the first
    for k in PASS_AT:
        add(f"passing_at_{k}", opt(), cat(*(disjoint(k + 1) + [reg(100 * k, 100 * k + 50, 90, cnt=30), reg(100 * k + 700, 100 * k + 750, 80), reg(0, 48, 70, cnt=1)])))
    # two passing primaries: in two ballots (the first ballot that holds one ends the walk), in one ballot (its lowest bit)
    for k in (63, 127):
        add(f"passing_at_{k}_and_{k + 1}", opt(), cat(*(disjoint(k + 2) + [reg(100 * k, 100 * k + 150, 90, cnt=30)])))
        add(f"passing_at_{k - 1}_and_{k}", opt(), cat(*(disjoint(k + 2) + [reg(100 * k - 100, 100 * k + 50, 90, cnt=30)])))
    # one overlap only, with the primary at w index 129: n_cov == 1 and the covered length comes out of the third round of 64
    pair("sole_overlap_round3", disjoint(130) + [reg(12910, 12960, 90, cnt=30)], 10)
    # one primary and 129 children beyond the LDS class: all of them dropped by score, all but one kept
    kids = lambda sc: [reg(0, 999 - j, sc(j), cnt=4 + j % 9) for j in range(129)]
    add("kept_1_of_130", opt(best_n=200), cat(*([reg(0, 1000, 1000)] + kids(lambda j: 700 - j))))
    add("kept_129_of_130", opt(best_n=200), cat(*([reg(0, 1000, 1000)] + kids(lambda j: 100 if j == 65 else 995 - j))))
    add("best_n_0", opt(best_n=0), cat(reg(0, 1000, 100), reg(0, 990, 99), reg(5, 1000, 98, rid=2), reg(2000, 3000, 97), reg(2000, 2990, 96), reg(0, 980, 95)))
    assert len(set(c["name"] for c in C)) == len(C)
    _CASES = C
    return C


def groups(cs=None):
    return _groups(cases() if cs is None else cs)
