"""The model of the alignment-task plan (tests/aln_model.py) against the reference's own mm_align1 (tests/golden/ref_aln.npz, made by
tests/golden/make_ref_aln_fixtures.py): every region's as1 / cnt1, anchor flags and recorded ksw calls -- scalars and FNV-1a of the bytes each call received -- and
every deliberately wrong variant of a rule differs on a named planted case."""
import os

import numpy as np
import pytest

import aln_data
import aln_model as M

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_aln.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(FX)


@pytest.fixture(scope="module")
def outs():
    ref = aln_data.reference()
    res = {}
    for name, (o, reads) in aln_data.cached_batches().items():
        u_off, regs, b_off, b, read_off, fwd, names = aln_data.csr(reads)
        res[name] = (M.run(o, ref, u_off, regs, b_off, b, read_off, fwd), names)
    return res


@pytest.mark.parametrize("name", sorted(aln_data.OPTS))
def test_model_reproduces_fixture(name, fx, outs):
    out, names = outs[name]
    assert M.fixture_mismatches(name, out, fx, names) == []


def test_fixture_cap_holds(fx):
    n, dropped, _ = (int(v) for v in fx["counts"])
    assert n >= 1000 and 4 * (n - dropped) >= 3 * n and dropped >= 2
    d = {str(nm) for nm, x in zip(fx["ont_names"], fx["ont_dropped"]) if x}
    assert {"spliced_in", "inversion"} <= d          # the prefix rule has planted cases of its own


def test_planted_mechanisms_occur(outs):
    """a self-check of the data, not of the library (it needs only aln_data and aln_model): the mechanisms the planted cases are named after do occur in them"""
    out, names = outs["ont"]
    ar, b = out["aln_regs"], out["b"]
    assert set(int(v) for v in ar["cnt1"]) >= {1, 2, 3} and (ar["status"] == 0).all()
    fl = b[:, 1] >> np.uint64(40)
    assert (fl & np.uint64(2)).any() and (fl & np.uint64(1)).any()              # IGNORE and LONG_JOIN were written
    regs = aln_data.csr(aln_data.cached_batches()["ont"][1])[1]
    assert ((ar["as1"] != regs["as"]) & (ar["cnt1"] > 0)).any() and ((ar["as1"] + ar["cnt1"] != regs["as"] + regs["cnt"]) & (ar["cnt1"] > 0)).any(), "mm_fix_bad_ends never trimmed an end"
    out20, _ = outs["asm20"]
    off = aln_data.reference()[0]
    b20 = aln_data.csr(aln_data.cached_batches()["asm20"][1])[3]
    regs20 = aln_data.csr(aln_data.cached_batches()["asm20"][1])[1]
    rid = np.array([int(b20[r["as"], 0] >> np.uint64(32)) & 0x7fffffff for r in regs20])
    res = {(int(off[rid[g]]) + int(out20["aln_regs"]["rs0"][g])) & 7 for g in range(len(rid))}
    assert res == set(range(8)), "rs0 does not meet every residue of the packed position mod 8"
    # the size classes of the long-gap list: exactly 2 048 and 2 049 gaps beyond 10
    nf, nf_names = outs["ont_noflt"]
    for nm, n in (("lg2048", 2048), ("lg2049", 2049)):
        r = nf["aln_regs"][nf_names.index(nm)]
        rd = [x for x in aln_data.cached_batches()["ont_noflt"][1] if x["name"] == nm][0]
        a = [[int(x), int(y)] for x, y in rd["a"]]
        assert sum(1 for i in range(1, int(r["cnt1"])) if abs(M.gap_at(a, int(r["as1"]) + i)) > 10) == n
    # a target span that ends at its contig's last base; a stretch at the chain's start, in its middle and at its end; the HPC walks that stop at i > 0 and at the offset
    b_ont = aln_data.csr(aln_data.cached_batches()["ont"][1])[3]
    lens = np.array(aln_data.CONTIG_LENS)
    assert any(r["cnt1"] > 0 and r["re0"] == lens[int(b_ont[g_["as"], 0] >> np.uint64(32)) & 0x7fffffff] for r, g_ in zip(ar, regs))
    sr, sr_names = outs["sr"]
    sr_regs = aln_data.csr(aln_data.cached_batches()["sr"][1])[1]
    rel = {nm: (int(sr["aln_regs"]["as1"][g]) - int(sr_regs["as"][g]), int(sr["aln_regs"]["cnt1"][g]), int(sr_regs["cnt"][g])) for g, nm in enumerate(sr_names)}
    assert rel["sr_start"][0] == 0 and rel["sr_start"][1] < rel["sr_start"][2] and 0 < rel["sr_middle"][0] and sum(rel["sr_middle"][:2]) < rel["sr_middle"][2]
    assert sum(rel["sr_end"][:2]) == rel["sr_end"][2] and rel["sr_end"][0] > 0 and rel["sr_equal"][0] == 0 and rel["sr_wave"][1] > 64
    assert (sr["items"]["kind"][:sr["totals"][0]] == M.UNGAPPED).sum() == len(sr_names)
    hp, hp_names = outs["hpc"]
    r = hp["aln_regs"][hp_names.index("hp_q1_ctg0")]
    assert (int(r["qs"]), int(r["rs"]), int(r["as1"])) == (1, 0, 0)
    sw, sw_names = outs["ont_sw"]
    kinds = [sorted(set(M.task_records(sw, g)[1])) for g in range(len(sw_names))]
    assert M.GAP | M.OVER not in kinds[sw_names.index("sw_at")] and M.GAP | M.OVER in kinds[sw_names.index("sw_above")]
    it = sw["items"][sw["aln_regs"]["item0"][0]:][:int(sw["aln_regs"]["n_items"][0])]
    assert ((it["qe"] - it["qs"]).astype(np.int64) * (it["re"] - it["rs"]) == 40000).any()      # an item exactly at max_sw_mat is not over


# the planted case each wrong variant must differ on, and the option set it lives in
WHERE = {
    "fix_ends_ignores_long_join": ("ont", ("lj_second", "lj_second_to_last")),
    "max_ext_cnt_off_by_one": ("ont", ("fbs5",)),
    "flush_only_at_end": ("ont", ("fbs4", "fbs1", "fbs2", "fbs3")),
    "rs0_without_final_min": ("ont", ("short_span",)),
    "nearby_counts_ge": ("ont", ("near_front3", "near_back3")),
    "bw1_not_widened": ("ont", ("alt1", "alt2", "alt4")),
    "tandem_skips_last": ("ont", ("tandem_last",)),
    "target_word_aligned": ("ont", None),
    "hpc_walk_to_zero": ("hpc", ("hp_q1_ctg0",)),
    "max_stretch_ge": ("sr", ("sr_equal",)),
}


@pytest.mark.parametrize("variant", M.VARIANTS)
def test_wrong_variant_differs(variant, fx):
    opt_name, where = WHERE[variant]
    o, reads = aln_data.cached_batches()[opt_name]
    if where is not None:
        reads = [r for r in reads if r["name"] in where]
    u_off, regs, b_off, b, read_off, fwd, names = aln_data.csr(reads)
    good = M.run(o, aln_data.reference(), u_off, regs, b_off, b, read_off, fwd)
    wrong = M.run(o, aln_data.reference(), u_off, regs, b_off, b, read_off, fwd, variant=variant)
    differs = [nm for g, nm in enumerate(names) if M.task_records(good, g) != M.task_records(wrong, g) or good["aln_regs"][g].tobytes() != wrong["aln_regs"][g].tobytes()]
    differs += ["<flags>"] if not np.array_equal(good["b"], wrong["b"]) else []
    assert differs, "the wrong variant %s agrees with the model on %s" % (variant, where)
    if where is not None:
        for w in where[:1]:
            assert any(d == w or d.startswith(w + "/") for d in differs), (variant, differs)
