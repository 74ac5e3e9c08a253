"""Chaining parameter presets, mirroring options.c of the reference (file:line cited per preset)."""
from ._native import Params, HitOpt, HitMultiOpt, MapqOpt, FinOpt, PairOpt, MM2C_F_IGNORE_SEG, MM2C_F_FORCE_GENERAL

INT32_MAX = 2**31 - 1


def make_params(max_dist_x=5000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, gap_scale=1.0,
                is_cdna=0, n_segs=1, q_span_override=-1, flags=0):
    return Params(max_dist_x, max_dist_y, bw, max_skip, max_iter, gap_scale, is_cdna, n_segs, q_span_override, flags)


def map_ont():
    """-x map-ont: options.c:24-31 defaults kept by :93-99; max_gap feeds both max_dist (map.c:305-316)."""
    return make_params()


def asm20():
    """-x asm20 (options.c:113-122): same chaining scalars as the defaults; k=19 changes only the anchor span."""
    return make_params()


def ava_ont():
    """-x ava-ont (options.c:83-86): bw=2000, max_gap=10000."""
    return make_params(max_dist_x=10000, max_dist_y=10000, bw=2000)


def splice():
    """-x splice (options.c:141-144): max_gap=2000 on the query, max_gap_ref=bw=200000 on the reference (map.c:308-310), MM_F_SPLICE -> is_cdna (map.c:275,316)."""
    return make_params(max_dist_x=200000, max_dist_y=2000, bw=200000, is_cdna=1)


def sr(qlen_sum=300, n_segs=2):
    """-x sr (options.c:123-132): max_gap=100, bw=100, max_frag_len=800.  map.c:306-307: the query gap is max(qlen_sum, max_gap); map.c:311-313: the
    reference gap is max(max_frag_len - qlen_sum, max_gap).  Default: a pair of 150-base reads chained as two segments."""
    return make_params(max_dist_x=max(800 - qlen_sum, 100), max_dist_y=max(qlen_sum, 100), bw=100, n_segs=n_segs)


def fpga_v2(max_dist_x=5000, max_dist_y=5000, bw=500, q_span=15):
    """What the reference's FPGA kernel computes for one run_chaining_on_hw call (device/minimap2_opencl.cl)."""
    return make_params(max_dist_x, max_dist_y, bw, INT32_MAX, 1024, 1.0, 0, 1, q_span, MM2C_F_IGNORE_SEG)


def hit_opts(k=15, **kw):
    """mm2c_hit_opt_t with the defaults of options.c:33-36: mask_level 0.5, mask_len INT_MAX, pri_ratio 0.8, best_n 5; min_diff = 2k as mm_map_frag passes it
    (map.c:253); hard_mask_level = opt->flag & MM_F_HARD_MLEVEL, off by default.  What the presets change (options.c:82-151; k is the index's):
    ava-ont: pri_ratio 0 (k 15) -- mm_select_sub then does nothing, and with MM_F_ALL_CHAINS chain_post skips both calls (map.c:251);  ava-pb: the same
    with k 19;  map-pb / map10k: k 19;  map-ont: k 15;
    asm5 / asm10 / asm20: best_n 50, k 19;  sr / short: pri_ratio 0.5, best_n 20, k 21;  splice / cdna: k 15.  Keywords override single fields."""
    v = dict(mask_level=0.5, mask_len=INT32_MAX, hard_mask_level=0, pri_ratio=0.8, min_diff=2 * k, best_n=5)
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"hit_opts: unknown field(s) {sorted(unknown)}")
    v.update(kw)
    return HitOpt(v["mask_level"], v["mask_len"], int(bool(v["hard_mask_level"])), v["pri_ratio"], v["min_diff"], v["best_n"])


def hit_multi_opts(n_segs=2, max_gap_ref=500, pri1=0.2, pri2=0.7):
    """mm2c_hit_multi_opt_t: pri1 and pri2 as mm_map_frag passes them to mm_select_sub_multi (map.c:254: 0.2f, 0.7f), the fragment's n_segs, and max_gap_ref for a
    run without per-fragment values (map.c:309-314; -x sr with 2 x 150 bases: max(800 - 300, 100) = 500)"""
    return HitMultiOpt(pri1, pri2, int(n_segs), int(max_gap_ref))


def mapq_opts(**kw):
    """mm2c_mapq_opt_t with the defaults of options.c: do_join 1 (map.c:255: off with MM_F_SPLICE, MM_F_SR or MM_F_NO_LJOIN, so the presets splice / cdna and
    sr / short pass do_join=0), max_join_long 20000, max_join_short 2000, min_join_flank_sc 1000, min_join_flank_ratio 0.5 (options.c:38-41), min_cnt 3 and
    min_chain_score 40 (options.c:24-25; sr: min_cnt 2, min_chain_score 25; ava-ont / ava-pb: min_chain_score 100).  Keywords override single fields."""
    v = dict(do_join=1, max_join_long=20000, max_join_short=2000, min_join_flank_sc=1000, min_join_flank_ratio=0.5, min_cnt=3, min_chain_score=40)
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"mapq_opts: unknown field(s) {sorted(unknown)}")
    v.update(kw)
    return MapqOpt(int(bool(v["do_join"])), v["max_join_long"], v["max_join_short"], v["min_join_flank_sc"], v["min_join_flank_ratio"], v["min_cnt"], v["min_chain_score"])


FIN_PRESETS = {   # min_cnt, min_chain_score, min_dp_max, pri_ratio, best_n, a, b, k, is_sr, all_chains (options.c:24-25, 33-36, 45, 49, 52 and the presets of :82-151)
    "map-ont": (3, 40, 80, 0.8, 5, 2, 4, 15, 0, 0), "map-pb": (3, 40, 80, 0.8, 5, 2, 4, 19, 0, 0), "ava-ont": (3, 100, 80, 0.0, 5, 2, 4, 15, 0, 1),
    "ava-pb": (3, 100, 80, 0.0, 5, 2, 4, 19, 0, 1),
    "asm5": (3, 40, 200, 0.8, 50, 1, 19, 19, 0, 0), "asm10": (3, 40, 200, 0.8, 50, 1, 9, 19, 0, 0), "asm20": (3, 40, 200, 0.8, 50, 1, 4, 19, 0, 0),
    "sr": (2, 25, 40, 0.5, 20, 2, 8, 21, 1, 0),
}


def fin_opts(preset="map-ont", **over):
    """mm2c_fin_opt_t as align_regs and mm_map_frag hand their options on (align.c:917, map.c:264-268, 361): min_cnt, min_chain_score, min_dp_max (options.c:49:
    min_chain_score * a = 80 at init; asm*: 200, sr: 40), max_clip_ratio 1.0 (:52), mask_level 0.5, mask_len INT_MAX, hard_mask_level 0, sub_diff = a * 2 + b,
    pri_ratio, min_diff = 2k (the index's k), best_n, match_sc = a, is_sr, all_chains (MM_F_ALL_CHAINS: ava-ont).  Keywords override single fields."""
    min_cnt, mcs, mdm, pri, best_n, a, b, k, is_sr, all_chains = FIN_PRESETS[preset]
    v = dict(min_cnt=min_cnt, min_chain_score=mcs, min_dp_max=mdm, max_clip_ratio=1.0, mask_level=0.5, mask_len=INT32_MAX, hard_mask_level=0, sub_diff=a * 2 + b,
             pri_ratio=pri, min_diff=2 * k, best_n=best_n, match_sc=a, is_sr=is_sr, all_chains=all_chains)
    unknown = set(over) - set(v)
    if unknown:
        raise TypeError(f"fin_opts: unknown field(s) {sorted(unknown)}")
    v.update(over)
    return FinOpt(v["min_cnt"], v["min_chain_score"], v["min_dp_max"], v["max_clip_ratio"], v["mask_level"], v["mask_len"], int(bool(v["hard_mask_level"])), v["sub_diff"],
                  v["pri_ratio"], v["min_diff"], v["best_n"], v["match_sc"], int(bool(v["is_sr"])), int(bool(v["all_chains"])))


def pair_opts(preset="sr", **over):
    """mm2c_pair_opt_t as mm_map_frag hands mm_pair its options (map.c:373-374): max_gap_ref (the scalar for a run without per-fragment values: -x sr with 2 x 150
    bases gives max(800 - 300, 100) = 500, map.c:311-313; otherwise the preset's bw), pe_bonus 33 (options.c:56), sub_diff = a * 2 + b and match_sc = a of the
    preset, pe_ori (options.c:55: 0 = FF; sr: 0 << 1 | 1 = FR, options.c:126) and flip = 1: the flip of map.c:455-466 runs.  Keywords override single fields."""
    a, b = FIN_PRESETS[preset][5:7]
    v = dict(max_gap_ref=500 if preset == "sr" else KSW_PRESETS[preset][10], pe_bonus=33, sub_diff=a * 2 + b, match_sc=a, pe_ori=1 if preset == "sr" else 0, flip=1)
    unknown = set(over) - set(v)
    if unknown:
        raise TypeError(f"pair_opts: unknown field(s) {sorted(unknown)}")
    v.update(over)
    return PairOpt(v["max_gap_ref"], v["pe_bonus"], v["sub_diff"], v["match_sc"], v["pe_ori"], int(bool(v["flip"])))


KSW_PRESETS = {   # a, b, q, e, q2, e2, sc_ambi, zdrop, zdrop_inv, end_bonus, bw (options.c:26,45-48 and the presets of :82-151)
    "map-ont": (2, 4, 4, 2, 24, 1, 1, 400, 200, -1, 500), "map-pb": (2, 4, 4, 2, 24, 1, 1, 400, 200, -1, 500),
    "ava-ont": (2, 4, 4, 2, 24, 1, 1, 400, 200, -1, 2000), "ava-pb": (2, 4, 4, 2, 24, 1, 1, 400, 200, -1, 2000),
    "asm5": (1, 19, 39, 3, 81, 1, 1, 200, 200, -1, 500), "asm10": (1, 9, 16, 2, 41, 1, 1, 200, 200, -1, 500), "asm20": (1, 4, 6, 2, 26, 1, 1, 200, 200, -1, 500),
    "sr": (2, 8, 12, 2, 24, 1, 1, 100, 100, 10, 100),
}


def ksw_scores(preset="map-ont", **kw):
    """The score set of a base-alignment call as mm_align_skeleton makes it: mat by ksw_gen_simple_mat (align.c:9-22, m = 5: a on the diagonal, -b off it, -sc_ambi in
    the last row and column) and the preset's scalars (options.c).  Returns dict(mat int8 list of 25, q, e, q2, e2, zdrop, zdrop_inv, end_bonus, bw); keywords
    (a, b, q, e, q2, e2, sc_ambi, zdrop, zdrop_inv, end_bonus, bw) override single values.  sr has q != q2, so it runs ksw_extd2 as well."""
    names = ("a", "b", "q", "e", "q2", "e2", "sc_ambi", "zdrop", "zdrop_inv", "end_bonus", "bw")
    v = dict(zip(names, KSW_PRESETS[preset]))
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"ksw_scores: unknown field(s) {sorted(unknown)}")
    v.update(kw)
    a, b, amb = abs(v["a"]), -abs(v["b"]), -abs(v["sc_ambi"])
    mat = [amb if (i == 4 or j == 4) else (a if i == j else b) for i in range(5) for j in range(5)]
    return dict(mat=mat, q=v["q"], e=v["e"], q2=v["q2"], e2=v["e2"], zdrop=v["zdrop"], zdrop_inv=v["zdrop_inv"], end_bonus=v["end_bonus"], bw=v["bw"])


def zdrop_opts(preset="map-ont", max_gap=5000, no_inv=None, **kw):
    """mm2c_zdrop_opt_t as mm_align1 hands it to mm_test_zdrop (align.c:47-89): the preset's zdrop and zdrop_inv (options.c), max_gap (5 000; sr: 100), and no_inv, which
    stands for opt->flag & (MM_F_SPLICE | MM_F_SR | MM_F_FOR_ONLY | MM_F_REV_ONLY) of :72 (set for sr).  Returns dict(zdrop, zdrop_inv, max_gap, no_inv)."""
    s = ksw_scores(preset, **kw)
    if preset == "sr" and max_gap == 5000:
        max_gap = 100
    return dict(zdrop=s["zdrop"], zdrop_inv=s["zdrop_inv"], max_gap=int(max_gap), no_inv=int(preset == "sr" if no_inv is None else bool(no_inv)))


ALN_PRESETS = {   # min_chain_score, max_gap, min_cnt, min_ksw_len, flag (MM2C_ALN_F_SR = 1), idx_flag (MM2C_ALN_I_HPC = 1), k (options.c:24-27, 50 and the presets)
    "map-ont": (40, 5000, 3, 200, 0, 0, 15), "map-pb": (40, 5000, 3, 200, 0, 1, 19), "asm20": (40, 5000, 3, 200, 0, 0, 19), "sr": (25, 100, 2, 200, 1, 0, 21),
}


def aln_opts(preset="map-ont", **kw):
    """mm2c_aln_opt_t as mm_align1 reads its options (align.c:565-771): the preset's scores, band and z-drops (ksw_scores), the chaining scalars of options.c, bw_ext =
    (int)(bw * 1.5 + 1.) of :580 computed here, max_sw_mat 0 (off), the preset's k and index flag.  Keywords override single fields.  Returns a dict of the struct's fields."""
    s = ksw_scores(preset)
    a, b = KSW_PRESETS[preset][:2]
    mcs, max_gap, min_cnt, mkl, flag, idx_flag, k = ALN_PRESETS[preset]
    v = dict(a=a, b=b, q=s["q"], e=s["e"], e2=s["e2"], bw=s["bw"], bw_ext=0, min_chain_score=mcs, max_gap=max_gap, min_cnt=min_cnt, min_ksw_len=mkl, end_bonus=s["end_bonus"],
             zdrop=s["zdrop"], zdrop_inv=s["zdrop_inv"], max_sw_mat=0, flag=flag, idx_flag=idx_flag, k=k, reserved=0)
    unknown = set(kw) - set(v)
    if unknown:
        raise TypeError(f"aln_opts: unknown field(s) {sorted(unknown)}")
    v.update(kw)
    if "bw_ext" not in kw:
        v["bw_ext"] = int(v["bw"] * 1.5 + 1.)
    return v


def as_dict(p):
    return {k: getattr(p, k) for k, _ in p._fields_}
