/* pair_dump.c -- test infrastructure for make_ref_pair_fixtures.py: the reference's own mm_pair (pe.o) on regions with r->p read from a binary file, and, in a
 * second mode, its whole mm_map_frag (map.o) with n_segs = 2 under the -x sr option values with MM_F_CIGAR, recording what goes into and comes out of mm_pair.
 * Built against the objects build() leaves in oracle/_ref/; never part of the library.
 * pair_dump planted in out                      (links pe.o, hit.o, misc.o, kalloc.o)
 *   in : int32 n_cases; per case { int32 qlens[2], max_gap_ref, pe_bonus, sub_diff, match_sc; int32 n[2]; mm_reg1_t r0[n[0]], r1[n[1]] (p: 1 + the index of a record);
 *        int32 n_pext; { int32 dp_score, dp_max, dp_max2; uint32 ambi_strand; int32 n_cigar, reserved; int64 cig0 } pext[n_pext] }
 *   out: int32 sizeof(mm_reg1_t); per case { per mate: int32 n; mm_reg1_t r[n] behind mm_pair (as and p zeroed: the generator puts back what came in); int32 idx[n] }
 *   A region's input index travels in r->as, which mm_pair neither reads nor writes, and is put back before the array is written.
 * pair_dump real <k> <w> <ref.fa> <frags.bin> <out.bin>     (links the whole reference with -Wl,--wrap=mm_pair,--wrap=mm_filter_regs; mm_chain_dp is the oracle's)
 *   frags.bin: as frag_dump.c reads it, two segments per fragment, as a sequencer gives them: the mate pe_ori names is reverse-complemented in front of mm_map_frag.
 *   out: int32 sizeof(mm_reg1_t); per fragment { int32 qlens[2], rep_len, max_gap_ref (as mm_pair got it), called (mm_pair was reached);
 *        per mate: LIST as mm_align_skeleton holds it in front of mm_filter_regs; per mate: LIST in front of mm_pair; per mate: LIST behind mm_pair }
 *   LIST = int32 n; mm_reg1_t r[n] (p: 0 or 1 + the index in the list's records); int32 n_pext; pext[n_pext] */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "minimap.h"
#include "mmpriv.h"
#include "kalloc.h"

typedef struct { int32_t dp_score, dp_max, dp_max2; uint32_t ambi_strand; int32_t n_cigar, reserved; int64_t cig0; } pext_t;

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

#ifndef PAIR_DUMP_REAL
void mm_pair(void *km, int max_gap_ref, int pe_bonus, int sub_diff, int match_sc, const int *qlens, int *n_regs, mm_reg1_t **regs);

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, c, i, s, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 4 || strcmp(argv[1], "planted") != 0 || !(in = fopen(argv[2], "rb")) || !(out = fopen(argv[3], "wb"))) return 1;
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (c = 0; c < n_cases; ++c) {
		int32_t h[6], n[2], n_pext, v;
		int qlens[2], n_regs[2];
		mm_reg1_t *r[2];
		pext_t *px;
		rd(h, sizeof h, in); rd(n, sizeof n, in);
		for (s = 0; s < 2; ++s) {
			r[s] = (mm_reg1_t*)malloc((size_t)n[s] * sizeof(mm_reg1_t) + 16);
			rd(r[s], (size_t)n[s] * sizeof(mm_reg1_t), in);
		}
		rd(&n_pext, 4, in);
		px = (pext_t*)malloc((size_t)n_pext * sizeof(pext_t) + 16);
		rd(px, (size_t)n_pext * sizeof(pext_t), in);
		for (s = 0; s < 2; ++s)
			for (i = 0; i < n[s]; ++i) {                                       /* an mm_extra_t of its own per region */
				uint64_t k = (uint64_t)(uintptr_t)r[s][i].p;
				mm_extra_t *e = (mm_extra_t*)calloc(1, sizeof(mm_extra_t) + 16);
				const pext_t *x = &px[k - 1];
				e->capacity = 4; e->dp_score = x->dp_score; e->dp_max = x->dp_max; e->dp_max2 = x->dp_max2;
				e->n_ambi = x->ambi_strand & 0x3fffffff; e->trans_strand = x->ambi_strand >> 30; e->n_cigar = (uint32_t)x->n_cigar;
				r[s][i].as = i; r[s][i].p = e;
			}
		qlens[0] = h[0]; qlens[1] = h[1]; n_regs[0] = n[0]; n_regs[1] = n[1];
		mm_pair(0, h[2], h[3], h[4], h[5], qlens, n_regs, r);                   /* map.c:374 */
		for (s = 0; s < 2; ++s) {
			v = n_regs[s]; fwrite(&v, 4, 1, out);
			for (i = 0; i < n_regs[s]; ++i) { mm_reg1_t t = r[s][i]; t.as = 0; t.p = 0; fwrite(&t, sizeof t, 1, out); }
			for (i = 0; i < n_regs[s]; ++i) { v = r[s][i].as; fwrite(&v, 4, 1, out); }
			for (i = 0; i < n[s]; ++i) free(r[s][i].p);
			free(r[s]);
		}
		free(px);
	}
	fclose(in); fclose(out);
	return 0;
}

#else /* PAIR_DUMP_REAL */
#include "chain_oracle.h"

struct tbuf_mirror { void *km; int rep_len, frag_gap; };                       /* struct mm_tbuf_s (map.c:13-16) */

/* symbols of options.c that the library objects import */
void mm_mapopt_update(mm_mapopt_t *opt, const mm_idx_t *mi) { (void)opt; (void)mi; }
void mm_idxopt_init(mm_idxopt_t *io)
{
	memset(io, 0, sizeof(*io));
	io->k = 15; io->w = 10; io->flag = 0; io->bucket_bits = 14;
	io->mini_batch_size = 50000000; io->batch_size = 4000000000ULL;
}

/* the reference's chain.c cannot be compiled without the Xilinx headers (oracle/ref_host/Makefile): mm_chain_dp is the repo's CPU oracle, as in frag_dump.c */
mm128_t *mm_chain_dp(int max_dist_x, int max_dist_y, int bw, int max_skip, int max_iter, int min_cnt, int min_sc, float gap_scale,
                     int is_cdna, int n_segs, int64_t n, mm128_t *a, int *n_u_, uint64_t **_u, void *km, int tid)
{
	mm2o_params_t par = { max_dist_x, max_dist_y, bw, max_skip, max_iter, gap_scale, is_cdna, n_segs };
	uint64_t *u = 0;
	mm2o_anchor_t *b = 0;
	mm128_t *ret = 0;
	int64_t n_b = 0;
	int n_u;
	(void)tid;
	if (_u) *_u = 0, *n_u_ = 0;
	if (n == 0 || a == 0) { kfree(km, a); return 0; }
	n_u = mm2o_mm_chain_dp(&par, min_cnt, min_sc, n, (const mm2o_anchor_t *)a, &u, &b, &n_b);
	kfree(km, a);                                                              /* chain.c:421: the callee owns a */
	if (n_u > 0) {
		uint64_t *uk = (uint64_t *)kmalloc(km, (size_t)n_u * 8);
		ret = (mm128_t *)kmalloc(km, (size_t)n_b * sizeof(mm128_t));
		memcpy(uk, u, (size_t)n_u * 8);
		memcpy(ret, b, (size_t)n_b * sizeof(mm128_t));
		*n_u_ = n_u, *_u = uk;
	}
	free(u); free(b);
	return ret;
}

/* a recorded list: the regions with p turned into 1 + the index of its record */
typedef struct { int32_t n, n_pext; mm_reg1_t *r; pext_t *px; } list_t;
static list_t g_pre[2], g_before[2], g_after[2];
static int g_n_filter, g_called, g_gap;

static void record(list_t *L, int n, const mm_reg1_t *r)
{
	int i;
	L->n = n; L->n_pext = 0;
	L->r = (mm_reg1_t*)malloc((size_t)n * sizeof(mm_reg1_t) + 16);
	L->px = (pext_t*)calloc((size_t)n + 1, sizeof(pext_t));
	for (i = 0; i < n; ++i) {
		L->r[i] = r[i];
		if (r[i].p) {
			const mm_extra_t *e = r[i].p;
			pext_t *x = &L->px[L->n_pext++];
			x->dp_score = e->dp_score; x->dp_max = e->dp_max; x->dp_max2 = e->dp_max2; x->ambi_strand = e->n_ambi | (uint32_t)e->trans_strand << 30; x->n_cigar = (int32_t)e->n_cigar;
			L->r[i].p = (mm_extra_t*)(uintptr_t)L->n_pext;
		}
	}
}

static void put(FILE *out, list_t *L)
{
	fwrite(&L->n, 4, 1, out); fwrite(L->r, sizeof(mm_reg1_t), (size_t)L->n, out);
	fwrite(&L->n_pext, 4, 1, out); fwrite(L->px, sizeof(pext_t), (size_t)L->n_pext, out);
	free(L->r); free(L->px); memset(L, 0, sizeof *L);
}

void __real_mm_filter_regs(const mm_mapopt_t *opt, int qlen, int *n_regs, mm_reg1_t *regs);
void __wrap_mm_filter_regs(const mm_mapopt_t *opt, int qlen, int *n_regs, mm_reg1_t *regs)
{
	if (g_n_filter < 2) record(&g_pre[g_n_filter], *n_regs, regs);             /* align.c:917, mate by mate */
	++g_n_filter;
	__real_mm_filter_regs(opt, qlen, n_regs, regs);
}

void __real_mm_pair(void *km, int max_gap_ref, int pe_bonus, int sub_diff, int match_sc, const int *qlens, int *n_regs, mm_reg1_t **regs);
void __wrap_mm_pair(void *km, int max_gap_ref, int pe_bonus, int sub_diff, int match_sc, const int *qlens, int *n_regs, mm_reg1_t **regs)
{
	int s;
	g_called = 1; g_gap = max_gap_ref;
	for (s = 0; s < 2; ++s) record(&g_before[s], n_regs[s], regs[s]);
	__real_mm_pair(km, max_gap_ref, pe_bonus, sub_diff, match_sc, qlens, n_regs, regs);
	for (s = 0; s < 2; ++s) record(&g_after[s], n_regs[s], regs[s]);
}

static void sr_options(mm_idxopt_t *io, mm_mapopt_t *mo)
{
	mm_idxopt_init(io); memset(mo, 0, sizeof(*mo));
	mo->seed = 11; mo->mid_occ_frac = 2e-4f; mo->sdust_thres = 0;                                        /* options.c:20-22 */
	mo->max_chain_skip = 25; mo->max_chain_iter = 5000; mo->chain_gap_scale = 1.0f; mo->max_gap_ref = -1; /* :28-31 */
	mo->mask_level = 0.5f; mo->mask_len = INT_MAX;                                                       /* :33-34 */
	mo->max_join_long = 20000; mo->max_join_short = 2000; mo->min_join_flank_sc = 1000; mo->min_join_flank_ratio = 0.5f;
	mo->alt_drop = 0.15f; mo->sc_ambi = 1;
	mo->min_ksw_len = 200; mo->anchor_ext_len = 20; mo->anchor_ext_shift = 6; mo->max_clip_ratio = 1.0f;
	mo->pe_bonus = 33;
	/* -x sr, options.c:123-140 */
	io->flag = 0; io->k = 21; io->w = 11;
	mo->flag |= MM_F_SR | MM_F_FRAG_MODE | MM_F_NO_PRINT_2ND | MM_F_2_IO_THREADS | MM_F_HEAP_SORT | MM_F_CIGAR;
	mo->pe_ori = 0 << 1 | 1;
	mo->a = 2; mo->b = 8; mo->q = 12; mo->e = 2; mo->q2 = 24; mo->e2 = 1;
	mo->zdrop = mo->zdrop_inv = 100;
	mo->end_bonus = 10; mo->max_frag_len = 800; mo->max_gap = 100; mo->bw = 100; mo->pri_ratio = 0.5f;
	mo->min_cnt = 2; mo->min_chain_score = 25; mo->min_dp_max = 40; mo->best_n = 20;
	mo->mid_occ = 1000; mo->max_occ = 5000; mo->mini_batch_size = 50000000;
}

int main(int argc, char *argv[])
{
	mm_idxopt_t io;
	mm_mapopt_t mo;
	mm_idx_reader_t *rdr;
	mm_idx_t *mi;
	mm_tbuf_t *tb;
	int64_t n_frags, n_segs_all, *frag_off, *seq_off, g;
	int32_t sz = (int32_t)sizeof(mm_reg1_t);
	char *bases;
	FILE *f, *out;
	if (argc != 7 || strcmp(argv[1], "real") != 0) { fprintf(stderr, "usage: %s real <k> <w> <ref.fa> <frags.bin> <out.bin>\n", argv[0]); return 1; }
	mm_verbose = 1;
	sr_options(&io, &mo);
	io.k = atoi(argv[2]); io.w = atoi(argv[3]);
	rdr = mm_idx_reader_open(argv[4], &io, 0);
	if (!rdr || !(mi = mm_idx_reader_read(rdr, 1))) { fprintf(stderr, "cannot index %s\n", argv[4]); return 1; }
	f = fopen(argv[5], "rb");
	if (!f) return 1;
	rd(&n_frags, 8, f); rd(&n_segs_all, 8, f);
	frag_off = (int64_t *)malloc((size_t)(n_frags + 1) * 8); seq_off = (int64_t *)malloc((size_t)(n_segs_all + 1) * 8);
	rd(frag_off, (size_t)(n_frags + 1) * 8, f); rd(seq_off, (size_t)(n_segs_all + 1) * 8, f);
	bases = (char *)malloc((size_t)seq_off[n_segs_all] + 1);
	rd(bases, (size_t)seq_off[n_segs_all], f);
	fclose(f);
	out = fopen(argv[6], "wb");
	fwrite(&sz, 4, 1, out);
	tb = mm_tbuf_init();
	for (g = 0; g < n_frags; ++g) {
		int qlens[2], n_regs[2] = {0, 0}, s;
		int32_t h[5];
		const char *seqs[2];
		mm_reg1_t *regs[2] = {0, 0};
		if (frag_off[g + 1] - frag_off[g] != 2) { fprintf(stderr, "fragment %lld does not have two segments\n", (long long)g); return 1; }
		for (s = 0; s < 2; ++s) {
			qlens[s] = (int)(seq_off[frag_off[g] + s + 1] - seq_off[frag_off[g] + s]);
			seqs[s] = bases + seq_off[frag_off[g] + s];
			if ((s == 0 && (mo.pe_ori >> 1 & 1)) || (s == 1 && (mo.pe_ori & 1))) {   /* what worker_for does in front of mm_map_frag (map.c:437-438); this copy is not turned back */
				char *q = bases + seq_off[frag_off[g] + s];
				int i, j;
				for (i = 0, j = qlens[s] - 1; i <= j; ++i, --j) {
					const char ci = q[i], cj = q[j];
					q[j] = ci == 'A' ? 'T' : ci == 'C' ? 'G' : ci == 'G' ? 'C' : ci == 'T' ? 'A' : 'N';
					q[i] = cj == 'A' ? 'T' : cj == 'C' ? 'G' : cj == 'G' ? 'C' : cj == 'T' ? 'A' : 'N';
				}
			}
		}
		g_n_filter = g_called = g_gap = 0;
		((struct tbuf_mirror *)tb)->rep_len = 0;
		mm_map_frag(mi, 2, qlens, seqs, n_regs, regs, tb, &mo, 0, 0);             /* qname == NULL */
		if (g_n_filter != 2 || !g_called) { fprintf(stderr, "fragment %lld: %d mm_filter_regs calls, mm_pair %d\n", (long long)g, g_n_filter, g_called); return 1; }
		h[0] = qlens[0]; h[1] = qlens[1]; h[2] = ((struct tbuf_mirror *)tb)->rep_len; h[3] = g_gap; h[4] = g_called;
		fwrite(h, 4, 5, out);
		for (s = 0; s < 2; ++s) put(out, &g_pre[s]);
		for (s = 0; s < 2; ++s) put(out, &g_before[s]);
		for (s = 0; s < 2; ++s) put(out, &g_after[s]);
		for (s = 0; s < 2; ++s) {
			int i;
			for (i = 0; i < n_regs[s]; ++i) free(regs[s][i].p);
			free(regs[s]);
		}
	}
	mm_tbuf_destroy(tb);
	fclose(out);
	return 0;
}
#endif
