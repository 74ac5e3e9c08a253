/* fin_dump.c -- the reference's own mm_filter_regs, mm_hit_sort, mm_set_parent, mm_select_sub, mm_set_sam_pri and mm_set_mapq (hit.o), in the order of align.c:917-918,
 * map.c:264-268 and map.c:361, on regions with r->p read from a binary file; and, in a second mode, its mm_split_reg.
 * Built by make_ref_fin_fixtures.py against oracle/_ref/{hit,misc,kalloc}.o; test infrastructure, never part of the library.
 * fin_dump regs in out
 *   in : int32 n_cases; per case { int32 qlen, rep_len; int32 min_cnt, min_chain_score, min_dp_max; float max_clip_ratio; float mask_level; int32 mask_len, hard_mask_level,
 *        sub_diff; float pri_ratio; int32 min_diff, best_n, match_sc, is_sr, all_chains; int32 n; mm_reg1_t r[n] (p: 0 or 1 + the index of a record); int32 n_pext;
 *        { int32 dp_score, dp_max, dp_max2; uint32 ambi_strand; int32 n_cigar, reserved; int64 cig0 } pext[n_pext] }
 *   out: int32 sizeof(mm_reg1_t); per case { int32 n1; int32 idx1[n1] (input indices behind mm_filter_regs); int32 n2; int32 idx2[n2] (behind mm_hit_sort); int32 n;
 *        mm_reg1_t r[n] (behind mm_set_mapq; as and p zeroed: the generator puts back what came in); int32 idx[n]; int32 dp_max2[n] }
 *   A region's input index travels in r->as, which none of the six functions reads or writes, and is put back before the array is written.
 * fin_dump split in out
 *   in : int32 n_cases; per case { mm_reg1_t r; int32 n, qlen, n_a; mm128_t a[n_a] }      out: per case { mm_reg1_t r, r2 } behind mm_split_reg(&r, &r2, n, qlen, a) */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "mmpriv.h"

typedef struct { int32_t dp_score, dp_max, dp_max2; uint32_t ambi_strand; int32_t n_cigar, reserved; int64_t cig0; } pext_t;

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

static void put_idx(FILE *out, int n, const mm_reg1_t *r)
{
	int32_t i, v = n;
	fwrite(&v, 4, 1, out);
	for (i = 0; i < n; ++i) { v = r[i].as; fwrite(&v, 4, 1, out); }
}

static int do_split(FILE *in, FILE *out)
{
	int32_t n_cases, i;
	rd(&n_cases, 4, in);
	for (i = 0; i < n_cases; ++i) {
		mm_reg1_t r, r2;
		int32_t n, qlen, n_a;
		mm128_t *a;
		rd(&r, sizeof r, in); rd(&n, 4, in); rd(&qlen, 4, in); rd(&n_a, 4, in);
		a = (mm128_t*)malloc((size_t)n_a * 16 + 16);
		rd(a, (size_t)n_a * 16, in);
		memset(&r2, 0, sizeof r2);
		mm_split_reg(&r, &r2, n, qlen, a);
		fwrite(&r, sizeof r, 1, out); fwrite(&r2, sizeof r2, 1, out);
		free(a);
	}
	return 0;
}

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, c, i, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 4 || !(in = fopen(argv[2], "rb")) || !(out = fopen(argv[3], "wb"))) return 1;
	if (strcmp(argv[1], "split") == 0) { c = do_split(in, out); fclose(in); fclose(out); return c; }
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (c = 0; c < n_cases; ++c) {
		int32_t qlen, rep_len, mask_len, hard, sub_diff, min_diff, best_n, match_sc, is_sr, all_chains, n, n_pext, v;
		float mask_level, pri_ratio;
		mm_mapopt_t opt;
		mm_reg1_t *r;
		pext_t *px;
		int n_regs;
		memset(&opt, 0, sizeof opt);
		rd(&qlen, 4, in); rd(&rep_len, 4, in);
		rd(&opt.min_cnt, 4, in); rd(&opt.min_chain_score, 4, in); rd(&opt.min_dp_max, 4, in); rd(&opt.max_clip_ratio, 4, in);
		rd(&mask_level, 4, in); rd(&mask_len, 4, in); rd(&hard, 4, in); rd(&sub_diff, 4, in); rd(&pri_ratio, 4, in); rd(&min_diff, 4, in); rd(&best_n, 4, in);
		rd(&match_sc, 4, in); rd(&is_sr, 4, in); rd(&all_chains, 4, in);
		rd(&n, 4, in);
		r = (mm_reg1_t*)malloc((size_t)n * sizeof(mm_reg1_t) + 16);
		rd(r, (size_t)n * sizeof(mm_reg1_t), in);
		rd(&n_pext, 4, in);
		px = (pext_t*)malloc((size_t)n_pext * sizeof(pext_t) + 16);
		rd(px, (size_t)n_pext * sizeof(pext_t), in);
		for (i = 0; i < n; ++i) {                                              /* an mm_extra_t of its own per region that has one: the reference frees the dropped ones */
			uint64_t k = (uint64_t)(uintptr_t)r[i].p;
			r[i].as = i;
			if (k) {
				mm_extra_t *e = (mm_extra_t*)calloc(1, sizeof(mm_extra_t) + 16);
				const pext_t *s = &px[k - 1];
				e->capacity = 4; e->dp_score = s->dp_score; e->dp_max = s->dp_max; e->dp_max2 = s->dp_max2;
				e->n_ambi = s->ambi_strand & 0x3fffffff; e->trans_strand = s->ambi_strand >> 30; e->n_cigar = (uint32_t)s->n_cigar;
				r[i].p = e;
			}
		}
		n_regs = n;
		mm_filter_regs(&opt, qlen, &n_regs, r);                                 /* align.c:917 */
		put_idx(out, n_regs, r);
		mm_hit_sort(0, &n_regs, r, 0.15f);                                      /* align.c:918 */
		put_idx(out, n_regs, r);
		if (!all_chains) {                                                      /* map.c:264-268 */
			mm_set_parent(0, mask_level, mask_len, n_regs, r, sub_diff, hard, 0.15f);
			mm_select_sub(0, pri_ratio, min_diff, best_n, &n_regs, r);
			mm_set_sam_pri(n_regs, r);
		}
		mm_set_mapq(0, n_regs, r, opt.min_chain_score, match_sc, rep_len, is_sr);   /* map.c:361 */
		v = n_regs; fwrite(&v, 4, 1, out);
		for (i = 0; i < n_regs; ++i) {
			mm_reg1_t t = r[i];
			t.as = 0; t.p = 0;
			fwrite(&t, sizeof t, 1, out);
		}
		put_idx(out, n_regs, r);
		for (i = 0; i < n_regs; ++i) { v = r[i].p ? r[i].p->dp_max2 : 0; fwrite(&v, 4, 1, out); }
		for (i = 0; i < n_regs; ++i) free(r[i].p);
		free(r); free(px);
	}
	fclose(in); fclose(out);
	return 0;
}
