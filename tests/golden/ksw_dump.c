/* ksw_dump.c -- the reference's own ksw_extd2_sse (ksw2_extd2_sse.o) on tasks read from a binary file.  Built by make_ref_ksw_fixtures.py against
 * oracle/_ref/{ksw2_extd2_sse,kalloc}.o; test infrastructure, never part of the library.
 * Every task runs twice through a kalloc pool whose free memory was filled with argv[3] before the call (the function reads a few bytes behind what it allocates).
 * in : int32 n; per task { int32 qlen, tlen, w, zdrop, end_bonus, flag; int8 mat[25], q, e, q2, e2; uint8 query[qlen], target[tlen] }
 * out: per task { int32 max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end; uint32 cigar[n_cigar] } */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "kalloc.h"
#include "ksw2.h"

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n, i, fill;
	void *km;
	if (argc != 4 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	fill = atoi(argv[3]);
	km = km_init();
	rd(&n, 4, in);
	for (i = 0; i < n; ++i) {
		int32_t h[6], o[11];
		int8_t sc[29];
		uint8_t *q, *t;
		size_t pool;
		void *blk;
		ksw_extz_t ez;
		rd(h, 24, in); rd(sc, 29, in);
		q = (uint8_t*)malloc((size_t)h[0] + 1); t = (uint8_t*)malloc((size_t)h[1] + 1);
		rd(q, (size_t)h[0], in); rd(t, (size_t)h[1], in);
		pool = ((size_t)(h[0] + h[1]) * ((size_t)(h[0] < h[1]? h[0] : h[1]) / 16 + 2) * 16 + (size_t)(h[0] + h[1]) * 64 + 65536) * 2;   /* more than p, H and the image */
		blk = kmalloc(km, pool); memset(blk, fill, pool); kfree(km, blk);
		memset(&ez, 0, sizeof(ez));
		ksw_extd2_sse(km, h[0], q, h[1], t, 5, sc, sc[25], sc[26], sc[27], sc[28], h[2], h[3], h[4], h[5], &ez);
		o[0] = (int32_t)ez.max; o[1] = ez.zdropped; o[2] = ez.max_q; o[3] = ez.max_t; o[4] = ez.mqe; o[5] = ez.mqe_t; o[6] = ez.mte; o[7] = ez.mte_q;
		o[8] = ez.score; o[9] = ez.n_cigar; o[10] = ez.reach_end;
		fwrite(o, 4, 11, out);
		if (ez.n_cigar > 0) fwrite(ez.cigar, 4, (size_t)ez.n_cigar, out);
		kfree(km, ez.cigar);
		free(q); free(t);
	}
	km_destroy(km);
	fclose(in); fclose(out);
	return 0;
}
