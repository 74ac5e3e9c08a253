/* esterr_dump.c -- the reference's own mm_gen_regs, mm_set_parent, mm_select_sub, mm_join_long (hit.o), mm_est_err (esterr.o) and mm_set_mapq on cases read from a
 * binary file, in the order of mm_map_frag (map.c:344, 252-256, 357, 361).  Built by make_ref_esterr_fixtures.py against oracle/_ref/{hit,esterr,misc,kalloc}.o; test
 * infrastructure, never part of the library.  The index is a zeroed mm_idx_t whose seq[] carries only len: mm_est_err reads nothing else of it.
 * in : int32 n_cases; per case { uint32 hash; int32 qlen; int32 n_u; int64 n_b; int32 n_mini; int32 n_ref; uint64 u[n_u]; mm128_t a[n_b]; uint64 mini_pos[n_mini];
 *                                uint32 ref_len[n_ref]; float mask_level; int32 mask_len, hard_mask_level; float pri_ratio; int32 min_diff, best_n;
 *                                int32 do_join, max_join_long, max_join_short, min_join_flank_sc; float min_join_flank_ratio; int32 min_cnt, min_chain_score; int32 rep_len }
 * out: int32 sizeof(mm_reg1_t); per case { int32 n_out; mm_reg1_t r[n_out] (behind mm_set_mapq); int64 n_b_out; mm128_t a[n_b_out] } */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "mmpriv.h"

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, i, j, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (i = 0; i < n_cases; ++i) {
		uint32_t hash, *ref_len; int32_t qlen, n_u, n_mini, n_ref, n; int64_t n_b, n_b_out;
		float mask_level, pri_ratio; int32_t mask_len, hard, min_diff, best_n, do_join, rep_len, min_chain_score;
		uint64_t *u, *mini_pos; mm128_t *a; mm_reg1_t *r;
		mm_mapopt_t opt;
		mm_idx_t mi;
		int n_regs;
		memset(&opt, 0, sizeof opt);
		memset(&mi, 0, sizeof mi);
		rd(&hash, 4, in); rd(&qlen, 4, in); rd(&n_u, 4, in); rd(&n_b, 8, in); rd(&n_mini, 4, in); rd(&n_ref, 4, in);
		u = (uint64_t*)malloc((size_t)n_u * 8 + 8); a = (mm128_t*)malloc((size_t)n_b * 16 + 16);
		mini_pos = (uint64_t*)malloc((size_t)n_mini * 8 + 8); ref_len = (uint32_t*)malloc((size_t)n_ref * 4 + 4);
		rd(u, (size_t)n_u * 8, in); rd(a, (size_t)n_b * 16, in); rd(mini_pos, (size_t)n_mini * 8, in); rd(ref_len, (size_t)n_ref * 4, in);
		mi.n_seq = (uint32_t)n_ref;
		mi.seq = (mm_idx_seq_t*)calloc((size_t)n_ref + 1, sizeof(mm_idx_seq_t));
		for (j = 0; j < n_ref; ++j) mi.seq[j].len = ref_len[j];
		rd(&mask_level, 4, in); rd(&mask_len, 4, in); rd(&hard, 4, in); rd(&pri_ratio, 4, in); rd(&min_diff, 4, in); rd(&best_n, 4, in);
		rd(&do_join, 4, in); rd(&opt.max_join_long, 4, in); rd(&opt.max_join_short, 4, in); rd(&opt.min_join_flank_sc, 4, in); rd(&opt.min_join_flank_ratio, 4, in);
		rd(&opt.min_cnt, 4, in); rd(&min_chain_score, 4, in); rd(&rep_len, 4, in);
		opt.min_chain_score = min_chain_score;
		r = mm_gen_regs(0, hash, qlen, n_u, u, a);                             /* map.c:344 */
		n_regs = n_u;
		if (n_regs > 0) {
			mm_set_parent(0, mask_level, mask_len, n_regs, r, 8, hard, 0.15f);  /* map.c:252 */
			mm_select_sub(0, pri_ratio, min_diff, best_n, &n_regs, r);          /* map.c:253 */
		}
		n_b_out = n_b;
		if (do_join) {
			if (n_regs >= 2) for (j = 0, n_b_out = 0; j < n_regs; ++j) n_b_out += r[j].cnt;   /* what mm_squeeze_a returns (hit.c:312) */
			mm_join_long(0, &opt, qlen, &n_regs, r, a);                         /* map.c:255-256 */
		}
		mm_est_err(&mi, qlen, n_regs, r, a, n_mini, mini_pos);                 /* map.c:357 */
		mm_set_mapq(0, n_regs, r, min_chain_score, 2, rep_len, 0);             /* map.c:361 */
		n = n_regs;
		fwrite(&n, 4, 1, out);
		if (n > 0) fwrite(r, sizeof(mm_reg1_t), (size_t)n, out);
		fwrite(&n_b_out, 8, 1, out);
		if (n_b_out > 0) fwrite(a, 16, (size_t)n_b_out, out);
		free(r); free(u); free(a); free(mini_pos); free(ref_len); free(mi.seq);
	}
	fclose(in); fclose(out);
	return 0;
}
