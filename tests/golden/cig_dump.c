/* cig_dump.c -- the reference's own mm_align1 (static in align.c) on regions read from a binary file, with every ksw call it makes recorded WITH its CIGAR words,
 * the region's CIGAR and dp_score in front of mm_update_extra, and what mm_align1 leaves in r, r->p and r2.  The reference's align.c is included from its own
 * directory (-I, at generation time only; nothing of it is copied); make_ref_cig_fixtures.py builds this against the objects in oracle/_ref/ without align.o.  Test
 * infrastructure, never part of the library.
 * The three ksw_ext*_sse names and mm_idx_getseq are redefined around the include.  A ksw call lands in a recorder that notes the scalars, FNV-1a of the query and
 * of the target bytes, calls the real function and notes the eleven ez fields and the words.  The mm_idx_getseq recorder snapshots r->p when it is set: the last
 * such call of a region is the one of :787, in front of mm_update_extra.
 * in : as aln_dump.c reads it.
 * out: per read { per region, then the region it splits off (at most two levels), each { int32 hd[30]: n_calls, rs, re, qs, qe, has_p, dp_score, dp_max, blen, mlen, n_ambi, n_cigar, r2.cnt, r2.as, r2.split_inv, r2.rs, r2.re, r2.qs,
 *      r2.qe, pre_has, pre_dp_score, pre_n_cigar, split, level, r2.score, r2.mlen, r2.blen, r2.parent, as1, cnt1; per call { int32[19] as aln_dump.c; uint32 words[n_cigar] }; uint32 pre[pre_n_cigar]; uint32 final[n_cigar] } } */
#include <stdio.h>
#define ksw_extd2_sse rec_extd2
#define ksw_extz2_sse rec_extz2
#define ksw_exts2_sse rec_exts2
#define mm_idx_getseq rec_getseq
#include "align.c"
#undef ksw_extd2_sse
#undef ksw_extz2_sse
#undef ksw_exts2_sse
#undef mm_idx_getseq
void ksw_extd2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
                   int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez);
void ksw_extz2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e, int w, int zdrop, int end_bonus,
                   int flag, ksw_extz_t *ez);
int mm_idx_getseq(const mm_idx_t *mi, uint32_t rid, uint32_t st, uint32_t en, uint8_t *seq);

static int32_t *rec;                       /* the region's calls, one behind the other: 19 words and the CIGAR */
static size_t n_rec, m_rec;
static int n_calls;
static mm_reg1_t *cur_r;
static uint32_t *pre;
static int32_t pre_has, pre_dp, pre_n, pre_m;

static uint32_t fnv(const uint8_t *s, int n)
{
	uint32_t h = 2166136261u;
	int i;
	for (i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
	return h;
}

static void room(size_t n)
{
	if (n_rec + n > m_rec) { m_rec = (n_rec + n) * 2 + 64; rec = (int32_t*)realloc(rec, m_rec * 4); }
}

static size_t rec_begin(int qlen, const uint8_t *q, int tlen, const uint8_t *t, int w, int zdrop, int end_bonus, int flag)
{
	int32_t *o;
	size_t at = n_rec;
	room(19);
	o = rec + n_rec; n_rec += 19; ++n_calls;
	o[0] = qlen; o[1] = tlen; o[2] = w; o[3] = zdrop; o[4] = end_bonus; o[5] = flag; o[6] = (int32_t)fnv(q, qlen); o[7] = (int32_t)fnv(t, tlen);
	return at;
}

static void rec_end(size_t at, const ksw_extz_t *ez)
{
	int32_t *o = rec + at;
	o[8] = (int32_t)ez->max; o[9] = ez->zdropped; o[10] = ez->max_q; o[11] = ez->max_t; o[12] = ez->mqe; o[13] = ez->mqe_t; o[14] = ez->mte; o[15] = ez->mte_q;
	o[16] = ez->score; o[17] = ez->n_cigar; o[18] = ez->reach_end;
	room((size_t)ez->n_cigar);
	if (ez->n_cigar > 0) memcpy(rec + n_rec, ez->cigar, (size_t)ez->n_cigar * 4);
	n_rec += (size_t)ez->n_cigar;
}

void rec_extd2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t gape2,
               int w, int zdrop, int end_bonus, int flag, ksw_extz_t *ez)
{
	const size_t at = rec_begin(qlen, query, tlen, target, w, zdrop, end_bonus, flag);
	ksw_extd2_sse(km, qlen, query, tlen, target, m, mat, gapo, gape, gapo2, gape2, w, zdrop, end_bonus, flag, ez);
	rec_end(at, ez);
}

void rec_extz2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t q, int8_t e, int w, int zdrop, int end_bonus,
               int flag, ksw_extz_t *ez)
{
	const size_t at = rec_begin(qlen, query, tlen, target, w, zdrop, end_bonus, flag);
	ksw_extz2_sse(km, qlen, query, tlen, target, m, mat, q, e, w, zdrop, end_bonus, flag, ez);
	rec_end(at, ez);
}

void rec_exts2(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo, int8_t gape, int8_t gapo2, int8_t noncan,
               int zdrop, int8_t junc_bonus, int flag, const uint8_t *junc, ksw_extz_t *ez)
{
	fprintf(stderr, "splice is out of scope\n");
	exit(1);
}

int rec_getseq(const mm_idx_t *mi, uint32_t rid, uint32_t st, uint32_t en, uint8_t *seq)
{
	if (cur_r && cur_r->p) {
		const mm_extra_t *p = cur_r->p;
		if ((int32_t)p->n_cigar > pre_m) { pre_m = (int32_t)p->n_cigar * 2 + 16; pre = (uint32_t*)realloc(pre, (size_t)pre_m * 4); }
		pre_has = 1; pre_dp = p->dp_score; pre_n = (int32_t)p->n_cigar;
		if (pre_n > 0) memcpy(pre, p->cigar, (size_t)pre_n * 4);
	}
	return mm_idx_getseq(mi, rid, st, en, seq);
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
			uint8_t *qseq0[2];
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
				mm_reg1_t cur = regs[g];
				int level;
				cur.p = 0;
				for (level = 0; level < 3; ++level) {                                          /* the region, then what it splits off, at most two levels deep */
					mm_reg1_t r = cur, r2;
					int32_t hd[30];
					ksw_extz_t ez;
					memset(&r2, 0, sizeof(r2));
					memset(&ez, 0, sizeof(ez));
					memset(hd, 0, sizeof(hd));
					if (opt.flag & MM_F_SR) mm_max_stretch(&r, a, &hd[28], &hd[29]);                 /* as1, cnt1 as mm_align1 will find them */
					else if (!(opt.flag & MM_F_NO_END_FLT)) mm_fix_bad_ends(&r, a, opt.bw, opt.min_chain_score * 2, &hd[28], &hd[29]);
					else hd[28] = r.as, hd[29] = r.cnt;
					n_rec = 0; n_calls = 0; pre_has = pre_dp = pre_n = 0;
					cur_r = &r;
					mm_align1(km, &opt, &mi, h[0], qseq0, &r, &r2, h[1], a, &ez, 0);
					cur_r = 0;
					hd[0] = n_calls; hd[1] = r.rs; hd[2] = r.re; hd[3] = r.qs; hd[4] = r.qe; hd[5] = r.p != 0;
					if (r.p) { hd[6] = r.p->dp_score; hd[7] = r.p->dp_max; hd[8] = r.blen; hd[9] = r.mlen; hd[10] = r.p->n_ambi; hd[11] = (int32_t)r.p->n_cigar; }
					hd[12] = r2.cnt; hd[13] = r2.as; hd[14] = r2.split_inv; hd[15] = r2.rs; hd[16] = r2.re; hd[17] = r2.qs; hd[18] = r2.qe;
					hd[19] = pre_has; hd[20] = pre_dp; hd[21] = pre_n; hd[22] = r.split;
					hd[23] = level; hd[24] = r2.score; hd[25] = r2.mlen; hd[26] = r2.blen; hd[27] = r2.parent;
					fwrite(hd, 4, 30, out);
					if (n_rec) fwrite(rec, 4, n_rec, out);
					if (pre_n) fwrite(pre, 4, (size_t)pre_n, out);
					if (r.p && r.p->n_cigar) fwrite(r.p->cigar, 4, r.p->n_cigar, out);
					kfree(km, ez.cigar);
					free(r.p);
					if (r2.cnt <= 0 || level == 2) break;
					cur = r2;
				}
			}
			free(regs); free(a); free(qseq0[0]);
		}
	}
	km_destroy(km);
	free(rec); free(pre); free(mi.seq); free(mi.S); free(off); free(len);
	fclose(in); fclose(out);
	return 0;
}
