/* frag_dump.c -- test infrastructure for make_ref_frag_fixtures.py: runs the reference's own mm_map_frag (map.o) with n_segs > 1 under the -x sr option values
 * (options.c:123-140, set by hand as oracle/ref_host/driver.c does for map-ont) and records what goes into and comes out of its mm_chain_dp calls.  mm_chain_dp is
 * the repo's CPU oracle behind a recording wrapper (the reference's chain.c cannot be compiled without the Xilinx headers, oracle/ref_host/Makefile).
 *
 *   frag_dump <k> <w> <mid_occ> <max_occ> <flags> <ref.fa> <frags.bin> <out.bin>        flags: 1 = MM_F_HEAP_SORT, 2 = MM_F_FOR_ONLY, 4 = MM_I_HPC (the index and the sketch)
 *
 * frags.bin: int64 n_frags, int64 n_segs, int64 frag_off[n_frags + 1], int64 seq_off[n_segs + 1], then the bytes of the segments.
 * out.bin: the index's pool and key table as sketch_dump.c writes them (int64 n_pool, pool, int64 n_keys, n_keys x {uint64 key, int64 cr_off, uint32 n}), then per
 * fragment:
 *   int32 n_segs, qlen_sum
 *   int64 n_mini, n_mini x {x, y}                          collect_minimizers (map.c:64-77) restated over the reference's mm_sketch
 *   int32 rep_len1; int64 n_m, n_m x mm2c_match_t, n_m x uint64 mini_pos      collect_matches (map.c:90-123) restated, max_occ = mid_occ (the first pass)
 *   int32 n_calls                                          mm_chain_dp calls mm_map_frag made (2: re-chained, map.c:318-340; 0: qlen_sum == 0)
 *   int32 rep_len                                          mm_tbuf_t.rep_len as mm_map_frag left it (map.c:342), checked against the restated one
 *   int64 n_mp, n_mp x uint64 mini_pos                     the restated collect_matches with the occurrence cut-off of the LAST call
 *   per call (n_calls times): int32 h[9] = max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, is_cdna, n_segs; float gap_scale;
 *                             int64 n_a, n_a x anchors as handed in; int32 n_u, n_u x uint64 u; int64 n_b, n_b x anchors returned */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "minimap.h"
#include "mmpriv.h"
#include "kalloc.h"
#include "khash.h"
#include "chain_oracle.h"

__KHASH_TYPE(idx, uint64_t, uint64_t)
typedef struct { mm128_v a; int32_t n; uint64_t *p; void *h; } idx_bucket_t;   /* struct mm_idx_bucket_s (index.c:27-32), field for field */
struct tbuf_mirror { void *km; int rep_len, frag_gap; };                       /* struct mm_tbuf_s (map.c:13-16) */

/* symbols of options.c that the library objects import */
void mm_mapopt_update(mm_mapopt_t *opt, const mm_idx_t *mi) { (void)opt; (void)mi; }
void mm_idxopt_init(mm_idxopt_t *io)
{
	memset(io, 0, sizeof(*io));
	io->k = 15; io->w = 10; io->flag = 0; io->bucket_bits = 14;
	io->mini_batch_size = 50000000; io->batch_size = 4000000000ULL;
}

/* A segment of length 0: mm_sketch asserts len > 0 (sketch.c:84), so the reference as built aborts on it; with assertions off the function's loop does not run and
 * nothing is pushed.  Linked with -Wl,--wrap=mm_sketch, every call of mm_sketch (collect_minimizers in map.o, and the ones below) comes here first, and an empty
 * segment contributes nothing but keeps its id. */
void __real_mm_sketch(void *km, const char *str, int len, int w, int k, uint32_t rid, int is_hpc, mm128_v *p);
void __wrap_mm_sketch(void *km, const char *str, int len, int w, int k, uint32_t rid, int is_hpc, mm128_v *p)
{
	if (len > 0) __real_mm_sketch(km, str, len, w, k, rid, is_hpc, p);
}

/* the recording wrapper: every call of the current fragment */
typedef struct { int32_t h[9]; float gap_scale; int64_t n_a; mm128_t *a; int32_t n_u; uint64_t *u; int64_t n_b; mm128_t *b; } call_t;
static call_t g_calls[4];
static int g_n_calls;

mm128_t *mm_chain_dp(int max_dist_x, int max_dist_y, int bw, int max_skip, int max_iter, int min_cnt, int min_sc, float gap_scale,
                     int is_cdna, int n_segs, int64_t n, mm128_t *a, int *n_u_, uint64_t **_u, void *km, int tid)
{
	mm2o_params_t par = { max_dist_x, max_dist_y, bw, max_skip, max_iter, gap_scale, is_cdna, n_segs };
	call_t *c = &g_calls[g_n_calls++];
	int32_t h[9] = { max_dist_x, max_dist_y, bw, max_skip, max_iter, min_cnt, min_sc, is_cdna, n_segs };
	uint64_t *u = 0;
	mm2o_anchor_t *b = 0;
	mm128_t *ret = 0;
	(void)tid;
	if (g_n_calls > 4) { fprintf(stderr, "more than 4 mm_chain_dp calls for one fragment\n"); exit(1); }
	memset(c, 0, sizeof(*c));
	memcpy(c->h, h, sizeof(h)); c->gap_scale = gap_scale;
	if (_u) *_u = 0, *n_u_ = 0;
	if (n == 0 || a == 0) { kfree(km, a); return 0; }
	c->n_a = n;
	c->a = (mm128_t *)malloc((size_t)n * 16);
	memcpy(c->a, a, (size_t)n * 16);
	c->n_u = mm2o_mm_chain_dp(&par, min_cnt, min_sc, n, (const mm2o_anchor_t *)a, &u, &b, &c->n_b);
	kfree(km, a);                                                              /* chain.c:421: the callee owns a */
	c->u = u; c->b = (mm128_t *)b;
	if (c->n_u > 0) {
		uint64_t *uk = (uint64_t *)kmalloc(km, (size_t)c->n_u * 8);
		ret = (mm128_t *)kmalloc(km, (size_t)c->n_b * sizeof(mm128_t));
		memcpy(uk, u, (size_t)c->n_u * 8);
		memcpy(ret, b, (size_t)c->n_b * sizeof(mm128_t));
		*n_u_ = c->n_u, *_u = uk;
	} else c->n_u = 0, c->n_b = 0;
	return ret;
}

static void sr_options(mm_idxopt_t *io, mm_mapopt_t *mo)
{
	mm_idxopt_init(io); memset(mo, 0, sizeof(*mo));
	mo->seed = 11; mo->mid_occ_frac = 2e-4f; mo->sdust_thres = 0;                                        /* options.c:20-22 */
	mo->min_cnt = 3; mo->min_chain_score = 40; mo->bw = 500; mo->max_gap = 5000; mo->max_gap_ref = -1;   /* :24-28 */
	mo->max_chain_skip = 25; mo->max_chain_iter = 5000; mo->chain_gap_scale = 1.0f;                      /* :29-31 */
	mo->mask_level = 0.5f; mo->mask_len = INT_MAX; mo->pri_ratio = 0.8f; mo->best_n = 5;                 /* :33-36 */
	mo->max_join_long = 20000; mo->max_join_short = 2000; mo->min_join_flank_sc = 1000; mo->min_join_flank_ratio = 0.5f;
	mo->alt_drop = 0.15f;
	mo->a = 2; mo->b = 4; mo->q = 4; mo->e = 2; mo->q2 = 24; mo->e2 = 1; mo->sc_ambi = 1;
	mo->zdrop = 400; mo->zdrop_inv = 200; mo->end_bonus = -1; mo->min_dp_max = mo->min_chain_score * mo->a;
	mo->min_ksw_len = 200; mo->anchor_ext_len = 20; mo->anchor_ext_shift = 6; mo->max_clip_ratio = 1.0f;
	mo->mini_batch_size = 500000000; mo->pe_ori = 0; mo->pe_bonus = 33;
	/* -x sr, options.c:123-140 (k, w, mid_occ and max_occ come from the command line) */
	io->flag = 0; io->k = 21; io->w = 11;
	mo->flag |= MM_F_SR | MM_F_FRAG_MODE | MM_F_NO_PRINT_2ND | MM_F_2_IO_THREADS | MM_F_HEAP_SORT;
	mo->pe_ori = 0 << 1 | 1;
	mo->a = 2; mo->b = 8; mo->q = 12; mo->e = 2; mo->q2 = 24; mo->e2 = 1;
	mo->zdrop = mo->zdrop_inv = 100;
	mo->end_bonus = 10; mo->max_frag_len = 800; mo->max_gap = 100; mo->bw = 100; mo->pri_ratio = 0.5f;
	mo->min_cnt = 2; mo->min_chain_score = 25; mo->min_dp_max = 40; mo->best_n = 20;
	mo->mid_occ = 1000; mo->max_occ = 5000; mo->mini_batch_size = 50000000;
}

typedef struct { int64_t cr_off; uint32_t n, q_pos, q_span, seg_tandem; } match_t;

int main(int argc, char *argv[])
{
	mm_idxopt_t io;
	mm_mapopt_t mo;
	mm_idx_reader_t *rd;
	mm_idx_t *mi;
	mm_tbuf_t *tb;
	const idx_bucket_t *B;
	int64_t n_frags, n_segs_all, *frag_off, *seq_off, *base_p, *base_v, n_pool = 0, n_keys = 0, g;
	int nb, i, flags;
	char *bases;
	uint64_t *pool;
	FILE *f, *out;
	if (argc != 9) { fprintf(stderr, "usage: %s <k> <w> <mid_occ> <max_occ> <flags> <ref.fa> <frags.bin> <out.bin>\n", argv[0]); return 1; }
	mm_verbose = 1;
	sr_options(&io, &mo);
	io.k = atoi(argv[1]); io.w = atoi(argv[2]); mo.mid_occ = atoi(argv[3]); mo.max_occ = atoi(argv[4]); flags = atoi(argv[5]);
	if (!(flags & 1)) mo.flag &= ~(int64_t)MM_F_HEAP_SORT;
	if (flags & 2) mo.flag |= MM_F_FOR_ONLY;
	if (flags & 4) io.flag |= MM_I_HPC;
	io.flag |= MM_I_NO_SEQ;
	rd = mm_idx_reader_open(argv[6], &io, 0);
	if (!rd || !(mi = mm_idx_reader_read(rd, 1))) { fprintf(stderr, "cannot index %s\n", argv[6]); return 1; }
	f = fopen(argv[7], "rb");
	if (!f || fread(&n_frags, 8, 1, f) != 1 || fread(&n_segs_all, 8, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", argv[7]); return 1; }
	frag_off = (int64_t *)malloc((size_t)(n_frags + 1) * 8); seq_off = (int64_t *)malloc((size_t)(n_segs_all + 1) * 8);
	if (fread(frag_off, 8, (size_t)n_frags + 1, f) != (size_t)n_frags + 1 || fread(seq_off, 8, (size_t)n_segs_all + 1, f) != (size_t)n_segs_all + 1) return 1;
	bases = (char *)malloc((size_t)seq_off[n_segs_all] + 1);
	if (seq_off[n_segs_all] && fread(bases, 1, (size_t)seq_off[n_segs_all], f) != (size_t)seq_off[n_segs_all]) return 1;
	fclose(f);
	out = fopen(argv[8], "wb");

	/* the index as a pool and a key table (sketch_dump.c) */
	B = (const idx_bucket_t *)mi->B;
	nb = 1 << mi->b;
	base_p = (int64_t *)malloc((size_t)nb * 8); base_v = (int64_t *)malloc((size_t)nb * 8);
	for (i = 0; i < nb; ++i) {
		const kh_idx_t *h = (const kh_idx_t *)B[i].h;
		base_p[i] = n_pool; n_pool += B[i].n;
		base_v[i] = n_pool; n_pool += h ? h->n_buckets : 0;
		if (h) n_keys += h->size;
	}
	pool = (uint64_t *)calloc((size_t)n_pool + 1, 8);
	for (i = 0; i < nb; ++i) {
		const kh_idx_t *h = (const kh_idx_t *)B[i].h;
		khint_t j;
		if (B[i].n) memcpy(pool + base_p[i], B[i].p, (size_t)B[i].n * 8);
		if (h) for (j = 0; j < h->n_buckets; ++j) pool[base_v[i] + j] = kh_exist(h, j) ? h->vals[j] : 0;
	}
	fwrite(&n_pool, 8, 1, out); fwrite(pool, 8, (size_t)n_pool, out); fwrite(&n_keys, 8, 1, out);
	for (i = 0; i < nb; ++i) {
		const kh_idx_t *h = (const kh_idx_t *)B[i].h;
		khint_t j;
		if (!h) continue;
		for (j = 0; j < h->n_buckets; ++j) {
			uint64_t key, kk;
			int64_t cr;
			uint32_t n;
			if (!kh_exist(h, j)) continue;
			kk = h->keys[j];
			key = (kk >> 1) << mi->b | (uint64_t)i;
			if (kk & 1) { n = 1; cr = base_v[i] + j; }
			else { n = (uint32_t)h->vals[j]; cr = base_p[i] + (int64_t)(h->vals[j] >> 32); }
			fwrite(&key, 8, 1, out); fwrite(&cr, 8, 1, out); fwrite(&n, 4, 1, out);
		}
	}

	tb = mm_tbuf_init();
	for (g = 0; g < n_frags; ++g) {
		int32_t n_segs = (int32_t)(frag_off[g + 1] - frag_off[g]), qlen_sum = 0, s, pass, n_calls, rep_final = 0;
		int qlens[MM_MAX_SEG], n_regs[MM_MAX_SEG], sum = 0;
		const char *seqs[MM_MAX_SEG];
		mm_reg1_t *regs[MM_MAX_SEG];
		mm128_v mv = {0, 0, 0};
		size_t n0 = 0, j;
		int64_t n_mini;
		for (s = 0; s < n_segs; ++s) {
			qlens[s] = (int)(seq_off[frag_off[g] + s + 1] - seq_off[frag_off[g] + s]);
			seqs[s] = bases + seq_off[frag_off[g] + s];
			qlen_sum += qlens[s];
		}
		fwrite(&n_segs, 4, 1, out); fwrite(&qlen_sum, 4, 1, out);
		for (s = 0; s < n_segs; ++s) {                                         /* collect_minimizers, map.c:68-76 (sdust_thres = 0) */
			mm_sketch(0, seqs[s], qlens[s], mi->w, mi->k, s, mi->flag & MM_I_HPC, &mv);
			for (j = n0; j < mv.n; ++j) mv.a[j].y += sum << 1;
			sum += qlens[s]; n0 = mv.n;
		}
		n_mini = (int64_t)mv.n;
		fwrite(&n_mini, 8, 1, out); fwrite(mv.a, 16, mv.n, out);

		g_n_calls = 0;
		((struct tbuf_mirror *)tb)->rep_len = 0;
		mm_map_frag(mi, n_segs, qlens, seqs, n_regs, regs, tb, &mo, 0, 0);     /* qname == NULL, as the batch entries without name ranks */
		n_calls = g_n_calls;
		for (s = 0; s < n_segs; ++s) free(regs[s]);

		for (pass = 0; pass < 2; ++pass) {                                     /* collect_matches restated: the first pass, then the last call's cut-off */
			const int occ = pass == 0 || n_calls < 2 ? mo.mid_occ : mo.max_occ;
			match_t *m = (match_t *)calloc(mv.n + 1, sizeof(match_t));
			uint64_t *mini_pos = (uint64_t *)calloc(mv.n + 1, 8);
			int rep_st = 0, rep_en = 0, rep_len = 0;
			int64_t n_m = 0;
			for (j = 0; j < mv.n; ++j) {
				mm128_t *p = &mv.a[j];
				uint32_t q_pos = (uint32_t)p->y, q_span = p->x & 0xff;
				int t;
				const uint64_t *cr = mm_idx_get(mi, p->x >> 8, &t);
				if (t >= occ) {
					int en = (q_pos >> 1) + 1, st = en - q_span;
					if (st > rep_en) { rep_len += rep_en - rep_st; rep_st = st, rep_en = en; }
					else rep_en = en;
				} else {
					int ii = (int)((p->x >> 8) & ((1u << mi->b) - 1)), tandem = 0;
					const idx_bucket_t *b = &B[ii];
					int64_t cro = 0;
					if (t > 0) cro = (cr >= b->p && cr < b->p + b->n) ? base_p[ii] + (cr - b->p) : base_v[ii] + (cr - ((const kh_idx_t *)b->h)->vals);
					if (j > 0 && p->x >> 8 == mv.a[j - 1].x >> 8) tandem = 1;
					if (j < mv.n - 1 && p->x >> 8 == mv.a[j + 1].x >> 8) tandem = 1;
					m[n_m].cr_off = cro; m[n_m].n = (uint32_t)t; m[n_m].q_pos = q_pos; m[n_m].q_span = q_span;
					m[n_m].seg_tandem = (uint32_t)(p->y >> 32) << 1 | (uint32_t)tandem;
					mini_pos[n_m++] = (uint64_t)q_span << 32 | q_pos >> 1;
				}
			}
			rep_len += rep_en - rep_st;
			if (pass == 0) {
				fwrite(&rep_len, 4, 1, out); fwrite(&n_m, 8, 1, out);
				for (j = 0; j < (size_t)n_m; ++j) {
					fwrite(&m[j].cr_off, 8, 1, out); fwrite(&m[j].n, 4, 1, out); fwrite(&m[j].q_pos, 4, 1, out);
					fwrite(&m[j].q_span, 4, 1, out); fwrite(&m[j].seg_tandem, 4, 1, out);
				}
				fwrite(mini_pos, 8, (size_t)n_m, out);
				fwrite(&n_calls, 4, 1, out);
			} else {
				rep_final = n_calls ? ((struct tbuf_mirror *)tb)->rep_len : 0;
				if (n_calls && rep_final != rep_len) { fprintf(stderr, "fragment %lld: rep_len %d from mm_map_frag, %d restated\n", (long long)g, rep_final, rep_len); return 1; }
				fwrite(&rep_final, 4, 1, out); fwrite(&n_m, 8, 1, out); fwrite(mini_pos, 8, (size_t)n_m, out);
			}
			free(m); free(mini_pos);
		}
		for (i = 0; i < n_calls; ++i) {
			call_t *c = &g_calls[i];
			fwrite(c->h, 4, 9, out); fwrite(&c->gap_scale, 4, 1, out);
			fwrite(&c->n_a, 8, 1, out); fwrite(c->a, 16, (size_t)c->n_a, out);
			fwrite(&c->n_u, 4, 1, out); fwrite(c->u, 8, (size_t)c->n_u, out);
			fwrite(&c->n_b, 8, 1, out); fwrite(c->b, 16, (size_t)c->n_b, out);
			free(c->a); free(c->u); free(c->b);
		}
		kfree(0, mv.a);
	}
	mm_tbuf_destroy(tb);
	fclose(out);
	return 0;
}
