/* seg_dump.c -- the reference's own path behind mm_chain_dp for fragments of several segments mapped without CIGAR (map.c:344, 252-254, 365-370): mm_gen_regs,
 * mm_set_parent, mm_select_sub_multi (pe.o), mm_seg_gen, and per segment mm_set_parent and mm_set_mapq (hit.o), on cases read from a binary file.
 * Built by make_ref_seg_fixtures.py against oracle/_ref/{hit,pe,misc,kalloc}.o; test infrastructure, never part of the library.
 * in : int32 n_cases; per case { uint32 hash; int32 n_segs; int32 qlens[n_segs]; int32 n_u; int64 n_b; uint64 u[n_u]; mm128_t a[n_b];
 *                                float mask_level; int32 mask_len, hard_mask_level; float pri_ratio; int32 min_diff, best_n; float pri1, pri2; int32 max_gap_ref;
 *                                int32 min_chain_score, rep_len }
 * out: int32 sizeof(mm_reg1_t); per case { int32 n; mm_reg1_t r[n] (behind mm_select_sub_multi);
 *                                          per segment { int32 n_u; uint64 u[n_u]; int32 n_a; mm128_t a[n_a]; mm_reg1_t regs[n_u] (out of mm_seg_gen);
 *                                                        mm_reg1_t final[n_u] (behind mm_set_parent and mm_set_mapq) } } */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "mmpriv.h"

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, i, s, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (i = 0; i < n_cases; ++i) {
		uint32_t hash; int32_t n_segs, n_u, n, qlen_sum = 0; int64_t n_b;
		float mask_level, pri_ratio, pri1, pri2; int32_t mask_len, hard, min_diff, best_n, max_gap_ref, min_chain_score, rep_len;
		int qlens[MM_MAX_SEG], n_regs[MM_MAX_SEG], n_regs0;
		uint64_t *u; mm128_t *a; mm_reg1_t *r, *regs[MM_MAX_SEG];
		mm_seg_t *seg;
		rd(&hash, 4, in); rd(&n_segs, 4, in);
		if (n_segs < 1 || n_segs > MM_MAX_SEG) return 2;
		for (s = 0; s < n_segs; ++s) { int32_t q; rd(&q, 4, in); qlens[s] = q; qlen_sum += q; }
		rd(&n_u, 4, in); rd(&n_b, 8, in);
		u = (uint64_t*)malloc((size_t)n_u * 8 + 8); a = (mm128_t*)malloc((size_t)n_b * 16 + 16);
		rd(u, (size_t)n_u * 8, in); rd(a, (size_t)n_b * 16, in);
		rd(&mask_level, 4, in); rd(&mask_len, 4, in); rd(&hard, 4, in); rd(&pri_ratio, 4, in); rd(&min_diff, 4, in); rd(&best_n, 4, in);
		rd(&pri1, 4, in); rd(&pri2, 4, in); rd(&max_gap_ref, 4, in); rd(&min_chain_score, 4, in); rd(&rep_len, 4, in);
		r = mm_gen_regs(0, hash, qlen_sum, n_u, u, a);                         /* map.c:344 */
		n_regs0 = n_u;
		if (n_regs0 > 0) {
			mm_set_parent(0, mask_level, mask_len, n_regs0, r, 8, hard, 0.15f); /* map.c:252 */
			mm_select_sub_multi(0, pri_ratio, pri1, pri2, max_gap_ref, min_diff, best_n, n_segs, qlens, &n_regs0, r);   /* map.c:254 */
		}
		n = n_regs0;
		fwrite(&n, 4, 1, out);
		if (n > 0) fwrite(r, sizeof(mm_reg1_t), (size_t)n, out);
		seg = mm_seg_gen(0, hash, n_segs, qlens, n_regs0, r, n_regs, regs, a);  /* map.c:365 */
		for (s = 0; s < n_segs; ++s) {
			int32_t nu = seg[s].n_u, na = seg[s].n_a;
			if (nu != n_regs[s]) return 3;
			fwrite(&nu, 4, 1, out);
			if (nu > 0) fwrite(seg[s].u, 8, (size_t)nu, out);
			fwrite(&na, 4, 1, out);
			if (na > 0) fwrite(seg[s].a, 16, (size_t)na, out);
			if (nu > 0) fwrite(regs[s], sizeof(mm_reg1_t), (size_t)nu, out);
			mm_set_parent(0, mask_level, mask_len, n_regs[s], regs[s], 8, hard, 0.15f);          /* map.c:368 */
			mm_set_mapq(0, n_regs[s], regs[s], min_chain_score, 2, rep_len, 1);                  /* map.c:370 */
			if (nu > 0) fwrite(regs[s], sizeof(mm_reg1_t), (size_t)nu, out);
			free(regs[s]);
		}
		mm_seg_free(0, n_segs, seg);
		free(r); free(u); free(a);
	}
	fclose(in); fclose(out);
	return 0;
}
