/* extra_dump.c -- the reference's own mm_update_extra and mm_test_zdrop (both static in align.c) on cases read from a binary file.  The reference's align.c is
 * included from its own directory (-I, at generation time only); make_ref_extra_fixtures.py builds this against the objects in oracle/_ref/ without align.o and
 * ksw2_ll_sse.o.  Test infrastructure, never part of the library.
 * mm_test_zdrop shows its locals only through its return value and its calls, so ksw_ll_qinit and ksw_ll_i16 are defined here and record what they are given.
 * in : int32 n_upd; per case { int32 qlen, tlen, n_cigar, rev, is_eqx; int8 mat[25], q, e; uint32 cigar[n_cigar]; uint8 query[qlen], target[tlen] }
 *      int32 n_zd;  per case { int32 qlen, tlen, n_cigar, thr[2][4] = { zdrop, zdrop_inv, max_gap, flag } x 2; int8 mat[25], q, e; uint32 cigar[]; uint8 query[], target[] }
 * out: per update case { int32 n_cigar, qs - 1000, 1000 + qlen - qe, rs - 5000, re - 5000 - tlen, blen, mlen, n_ambi, dp_max; uint32 cigar[n_cigar] }
 *      per z-drop case { int32 max_zdrop, t0, t_len, q_len, fnv1a of the recorded query bytes, ret and called under thr[0], ret and called under thr[1] } */
#include <stdio.h>
#include <limits.h>
#include "align.c"

static int rec_called, rec_qlen, rec_tlen;
static const uint8_t *rec_target;
static uint32_t rec_hash;

void *ksw_ll_qinit(void *km, int size, int qlen, const uint8_t *query, int m, const int8_t *mat)
{
	int i;
	rec_called = 1; rec_qlen = qlen; rec_hash = 2166136261u;
	for (i = 0; i < qlen; ++i) rec_hash = (rec_hash ^ query[i]) * 16777619u;
	return kmalloc(km, 16);
}

int ksw_ll_i16(void *q, int tlen, const uint8_t *target, int gapo, int gape, int *qe, int *te)
{
	rec_tlen = tlen; rec_target = target; *qe = *te = -1;
	return -1;                                  /* never a potential inversion: the return is that of :88 */
}

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

static int zd(int zdrop, int zdrop_inv, int max_gap, int flag, int q, int e, const uint8_t *qs, const uint8_t *ts, int n, uint32_t *cig, const int8_t *mat)
{
	mm_mapopt_t opt;
	memset(&opt, 0, sizeof(opt));
	opt.zdrop = zdrop; opt.zdrop_inv = zdrop_inv; opt.max_gap = max_gap; opt.flag = flag; opt.q = q; opt.e = e;
	rec_called = 0;
	return mm_test_zdrop(0, &opt, qs, ts, n, cig, mat);
}

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n, i;
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	rd(&n, 4, in);
	for (i = 0; i < n; ++i) {
		int32_t h[5], o[9];
		int8_t sc[27];
		uint8_t *q, *t;
		mm_reg1_t r;
		rd(h, 20, in); rd(sc, 27, in);
		memset(&r, 0, sizeof(r));
		r.p = (mm_extra_t*)calloc((size_t)h[2] + sizeof(mm_extra_t) / 4 + 1, 4);
		r.p->capacity = h[2] + sizeof(mm_extra_t) / 4 + 1;
		r.p->n_cigar = h[2];
		rd(r.p->cigar, (size_t)h[2] * 4, in);
		q = (uint8_t*)malloc((size_t)h[0] + 1); t = (uint8_t*)malloc((size_t)h[1] + 1);
		rd(q, (size_t)h[0], in); rd(t, (size_t)h[1], in);
		r.qs = 1000; r.qe = 1000 + h[0]; r.rs = 5000; r.re = 5000 + h[1]; r.rev = h[3];
		mm_update_extra(&r, q, t, sc, sc[25], sc[26], h[4]);
		o[0] = r.p->n_cigar; o[1] = r.qs - 1000; o[2] = 1000 + h[0] - r.qe; o[3] = r.rs - 5000; o[4] = r.re - 5000 - h[1];
		o[5] = r.blen; o[6] = r.mlen; o[7] = r.p->n_ambi; o[8] = r.p->dp_max;
		fwrite(o, 4, 9, out);
		if (r.p->n_cigar > 0) fwrite(r.p->cigar, 4, r.p->n_cigar, out);
		free(r.p); free(q); free(t);
	}
	rd(&n, 4, in);
	for (i = 0; i < n; ++i) {
		int32_t h[11], o[9], lo, hi, k;
		int8_t sc[27];
		uint8_t *q, *t;
		uint32_t *cig;
		rd(h, 44, in); rd(sc, 27, in);
		cig = (uint32_t*)malloc((size_t)h[2] * 4 + 4);
		rd(cig, (size_t)h[2] * 4, in);
		q = (uint8_t*)malloc((size_t)h[0] + 1); t = (uint8_t*)malloc((size_t)h[1] + 1);
		rd(q, (size_t)h[0], in); rd(t, (size_t)h[1], in);
		/* the locals: the inversion test always entered, its arguments recorded */
		zd(INT_MAX, -1, INT_MAX, 0, sc[25], sc[26], q, t, h[2], cig, sc);
		o[1] = rec_called ? (int32_t)(rec_target - t) : -2; o[2] = rec_tlen; o[3] = rec_qlen; o[4] = (int32_t)rec_hash;
		/* max_zdrop: the smallest zdrop for which the function returns 0, the inversion test never entered */
		lo = 0; hi = 1 << 30;
		while (lo < hi) {
			int mid = lo + (hi - lo) / 2;
			if (zd(mid, INT_MAX, 0, 0, sc[25], sc[26], q, t, h[2], cig, sc) == 0) hi = mid; else lo = mid + 1;
		}
		o[0] = lo;
		for (k = 0; k < 2; ++k) {
			o[5 + 2 * k] = zd(h[3 + 4 * k], h[4 + 4 * k], h[5 + 4 * k], h[6 + 4 * k], sc[25], sc[26], q, t, h[2], cig, sc);
			o[6 + 2 * k] = rec_called;
		}
		fwrite(o, 4, 9, out);
		free(cig); free(q); free(t);
	}
	fclose(in); fclose(out);
	return 0;
}
