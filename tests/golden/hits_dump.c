/* hits_dump.c -- the reference's own mm_set_parent and mm_select_sub (hit.o) on cases read from a binary file.
 * Built by make_ref_hits_fixtures.py against oracle/_ref/{hit,misc,kalloc}.o; test infrastructure, never part of the library.
 * in : int32 n_cases; per case { float mask_level; int32 mask_len; int32 hard_mask_level; float pri_ratio; int32 min_diff; int32 best_n; int32 n; mm_reg1_t r[n] (raw) }
 * out: int32 sizeof(mm_reg1_t); per case { int32 n_out; mm_reg1_t r[n_out] (raw) } */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "mmpriv.h"

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, i, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (i = 0; i < n_cases; ++i) {
		float mask_level, pri_ratio; int32_t mask_len, hard, min_diff, best_n, n;
		int n_regs;
		mm_reg1_t *r;
		rd(&mask_level, 4, in); rd(&mask_len, 4, in); rd(&hard, 4, in); rd(&pri_ratio, 4, in); rd(&min_diff, 4, in); rd(&best_n, 4, in); rd(&n, 4, in);
		r = (mm_reg1_t*)malloc((size_t)n * sizeof(mm_reg1_t) + 8);
		rd(r, (size_t)n * sizeof(mm_reg1_t), in);
		n_regs = n;
		mm_set_parent(0, mask_level, mask_len, n_regs, r, 8, hard, 0.15f);     /* map.c:252 (sub_diff and alt_drop only act on regions with p or is_alt) */
		mm_select_sub(0, pri_ratio, min_diff, best_n, &n_regs, r);             /* map.c:253 */
		n = n_regs;
		fwrite(&n, 4, 1, out);
		if (n > 0) fwrite(r, sizeof(mm_reg1_t), (size_t)n, out);
		free(r);
	}
	fclose(in); fclose(out);
	return 0;
}
