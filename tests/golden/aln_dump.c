/* aln_dump.c -- the reference's own mm_align1 (static in align.c) on regions read from a binary file, with every ksw call it makes recorded.  The reference's
 * align.c is included from its own directory (-I, at generation time only; nothing of it is copied); make_ref_aln_fixtures.py builds this against the objects in
 * oracle/_ref/ without align.o.  Test infrastructure, never part of the library.
 * The three ksw_ext*_sse names are redefined around the include, so each call from mm_align_pair lands in a recorder that notes the scalars and FNV-1a of the query
 * and of the target bytes, calls the real function and notes the eleven ez fields.  mm_fix_bad_ends is also called directly for as1, cnt1.
 * in : int32 n_seq; uint64 offset[n_seq]; uint32 len[n_seq]; int32 n_words; uint32 S[n_words]; int32 n_batches; per batch { int32 opt[20]: a, b, q, e, q2, e2, bw,
 *      min_chain_score, max_gap, min_cnt, min_ksw_len, end_bonus, zdrop, zdrop_inv, max_sw_mat, flag, idx_flag, k, sc_ambi, 0; int32 n_reads;
 *      per read { int32 qlen, n_a, n_regs; uint8 fwd[qlen]; uint64 a[2 n_a]; mm_reg1_t regs[n_regs] } }
 * out: per read { per region { int32 as1, cnt1, n_calls, dp_score; per call int32[19]: qlen, tlen, w, zdrop, end_bonus, flag, hash_q, hash_t, max, zdropped, max_q, max_t, mqe,
 *      mqe_t, mte, mte_q, score, n_cigar, reach_end }; uint8 (y >> 40 & 0xff)[n_a] behind all regions of the read } */
#include <stdio.h>
#define ksw_extd2_sse rec_extd2
#define ksw_extz2_sse rec_extz2
#define ksw_exts2_sse rec_exts2
#include "align.c"
#undef ksw_extd2_sse
#undef ksw_extz2_sse
#undef ksw_exts2_sse
void ksw_extd2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
                   int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
void ksw_extz2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e, int w, int zdrop, int end_bonus,
                   int flag, ksw_extz_t *ez);

static int32_t *rec;
static int n_rec, m_rec;

static uint32_t fnv(const uint8_t *s, int n)
{
	uint32_t h = 2166136261u;
	int i;
	for (i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
	return h;
}

static int32_t *rec_begin(int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int zdrop, int end_bonus, int flag)
{
	int32_t *o;
	if (n_rec == m_rec) { m_rec = m_rec ? m_rec * 2 : 64; rec = (int32_t*)realloc(rec, (size_t)m_rec * 19 * 4); }
	o = rec + (size_t)n_rec++ * 19;
	o[0] = qlen; o[1] = tlen; o[2] = w; o[3] = zdrop; o[4] = end_bonus; o[5] = flag; o[6] = (int32_t)fnv(q, qlen); o[7] = (int32_t)fnv(t, tlen);
	return o;
}

static void rec_end(int32_t *o, const ksw_extz_t *ez)
{
	o[8] = (int32_t)ez->max; o[9] = ez->zdropped; o[10] = ez->max_q; o[11] = ez->max_t; o[12] = ez->mqe; o[13] = ez->mqe_t; o[14] = ez->mte; o[15] = ez->mte_q;
	o[16] = ez->score; o[17] = ez->n_cigar; o[18] = ez->reach_end;
}

void rec_extd2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
               int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez)
{
	int32_t *o = rec_begin(qlen, query, tlen, target, w, zdrop, end_bonus, flag);
	ksw_extd2_sse(km, qlen, query, tlen, target, m, mat, gapo, gape, gapo2, gape2, w, zdrop, end_bonus, flag, ez);
	rec_end(rec + (o - rec), ez);
}

void rec_extz2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e, int w, int zdrop, int end_bonus,
               int flag, ksw_extz_t *ez)
{
	int32_t *o = rec_begin(qlen, query, tlen, target, w, zdrop, end_bonus, flag);
	ksw_extz2_sse(km, qlen, query, tlen, target, m, mat, q, e, w, zdrop, end_bonus, flag, ez);
	rec_end(rec + (o - rec), ez);
}

void rec_exts2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan,
               int zdrop, int8_t junc_bonus, int flag, const uint8_t *junc, ksw_extz_t *ez)
{
	fprintf(stderr, "splice is out of scope\n");
	exit(1);
}

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_seq, n_words, n_batches, bi, i;
	uint64_t *off;
	uint32_t *len;
	mm_idx_t mi;
	void *km;
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	memset(&mi, 0, sizeof(mi));
	rd(&n_seq, 4, in);
	off = (uint64_t*)malloc((size_t)n_seq * 8 + 8); len = (uint32_t*)malloc((size_t)n_seq * 4 + 4);
	rd(off, (size_t)n_seq * 8, in); rd(len, (size_t)n_seq * 4, in);
	rd(&n_words, 4, in);
	mi.S = (uint32_t*)malloc((size_t)n_words * 4 + 4);
	rd(mi.S, (size_t)n_words * 4, in);
	mi.n_seq = n_seq;
	mi.seq = (mm_idx_seq_t*)calloc(n_seq + 1, sizeof(mm_idx_seq_t));
	for (i = 0; i < n_seq; ++i) { mi.seq[i].offset = off[i]; mi.seq[i].len = len[i]; }
	km = km_init();
	rd(&n_batches, 4, in);
	for (bi = 0; bi < n_batches; ++bi) {
		int32_t o[20], n_reads, ri;
		mm_mapopt_t opt;
		rd(o, 80, in); rd(&n_reads, 4, in);
		memset(&opt, 0, sizeof(opt));
		opt.a = o[0]; opt.b = o[1]; opt.q = o[2]; opt.e = o[3]; opt.q2 = o[4]; opt.e2 = o[5]; opt.bw = o[6]; opt.min_chain_score = o[7]; opt.max_gap = o[8]; opt.min_cnt = o[9];
		opt.min_ksw_len = o[10]; opt.end_bonus = o[11]; opt.zdrop = o[12]; opt.zdrop_inv = o[13]; opt.max_sw_mat = o[14]; opt.flag = o[15]; opt.sc_ambi = o[18];
		mi.flag = o[16]; mi.k = o[17];
		for (ri = 0; ri < n_reads; ++ri) {
			int32_t h[3], g, j;
			uint8_t *qseq0[2], *fl;
			mm128_t *a;
			mm_reg1_t *regs;
			rd(h, 12, in);
			qseq0[0] = (uint8_t*)malloc((size_t)h[0] * 2 + 2); qseq0[1] = qseq0[0] + h[0];
			rd(qseq0[0], (size_t)h[0], in);
			for (j = 0; j < h[0]; ++j) qseq0[1][h[0] - 1 - j] = qseq0[0][j] < 4 ? 3 - qseq0[0][j] : 4;      /* as :876 */
			a = (mm128_t*)malloc((size_t)h[1] * 16 + 16);
			rd(a, (size_t)h[1] * 16, in);
			regs = (mm_reg1_t*)malloc((size_t)h[2] * sizeof(mm_reg1_t) + 8);
			rd(regs, (size_t)h[2] * sizeof(mm_reg1_t), in);
			for (g = 0; g < h[2]; ++g) {
				mm_reg1_t r = regs[g], r2;
				int32_t hd[4];
				ksw_extz_t ez;
				r.p = 0;
				memset(&r2, 0, sizeof(r2));
				memset(&ez, 0, sizeof(ez));
				if (opt.flag & MM_F_SR) mm_max_stretch(&r, a, &hd[0], &hd[1]);
				else if (!(opt.flag & MM_F_NO_END_FLT)) mm_fix_bad_ends(&r, a, opt.bw, opt.min_chain_score * 2, &hd[0], &hd[1]);
				else hd[0] = r.as, hd[1] = r.cnt;
				n_rec = 0;
				mm_align1(km, &opt, &mi, h[0], qseq0, &r, &r2, h[1], a, &ez, 0);
				hd[2] = n_rec;
				hd[3] = r.p ? r.p->dp_score : 0;
				fwrite(hd, 4, 4, out);
				fwrite(rec, 4, (size_t)n_rec * 19, out);
				kfree(km, ez.cigar);
				free(r.p);
			}
			fl = (uint8_t*)malloc((size_t)h[1] + 1);
			for (j = 0; j < h[1]; ++j) fl[j] = (uint8_t)(a[j].y >> 40 & 0xff);
			fwrite(fl, 1, (size_t)h[1], out);
			free(fl); free(regs); free(a); free(qseq0[0]);
		}
	}
	km_destroy(km);
	free(rec); free(mi.seq); free(mi.S); free(off); free(len);
	fclose(in); fclose(out);
	return 0;
}
