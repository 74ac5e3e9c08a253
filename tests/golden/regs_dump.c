/* regs_dump.c -- the reference's own mm_gen_regs (hit.o) and the read hash of map.c:290-292 (khash.h inlines) on cases read from a binary file.
 * Built by make_ref_regs_fixtures.py against oracle/_ref/{hit,misc,kalloc}.o; test infrastructure, never part of the library.
 * in : int32 n_cases; per case { uint32 hash; int32 qlen; int32 n_u; int64 n_b; uint64 u[n_u]; mm128_t a[n_b] };
 *      int32 n_hashes; per hash { int32 has_name; int32 len; char name[len]; int32 qlen_sum; int32 seed }
 * out: int32 sizeof(mm_reg1_t); per case mm_reg1_t r[n_u] (raw); uint32 hash[n_hashes] */
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "mmpriv.h"
#include "khash.h"

static void rd(void *p, size_t n, FILE *f) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read\n"); exit(1); } }

int main(int argc, char **argv)
{
	FILE *in, *out;
	int32_t n_cases, n_hashes, i, sz = (int32_t)sizeof(mm_reg1_t);
	if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 1;
	fwrite(&sz, 4, 1, out);
	rd(&n_cases, 4, in);
	for (i = 0; i < n_cases; ++i) {
		uint32_t hash; int32_t qlen, n_u; int64_t n_b;
		uint64_t *u; mm128_t *a; mm_reg1_t *r;
		rd(&hash, 4, in); rd(&qlen, 4, in); rd(&n_u, 4, in); rd(&n_b, 8, in);
		u = (uint64_t*)malloc((size_t)n_u * 8 + 8); a = (mm128_t*)malloc((size_t)n_b * 16 + 16);
		rd(u, (size_t)n_u * 8, in); rd(a, (size_t)n_b * 16, in);
		r = mm_gen_regs(0, hash, qlen, n_u, u, a);
		if (n_u > 0) fwrite(r, sizeof(mm_reg1_t), (size_t)n_u, out);
		free(r); free(u); free(a);
	}
	rd(&n_hashes, 4, in);
	for (i = 0; i < n_hashes; ++i) {
		int32_t has_name, len, qlen_sum, seed;
		char *name;
		uint32_t hash;
		rd(&has_name, 4, in); rd(&len, 4, in);
		name = (char*)calloc((size_t)len + 1, 1);
		rd(name, (size_t)len, in); rd(&qlen_sum, 4, in); rd(&seed, 4, in);
		hash  = has_name? __ac_X31_hash_string(name) : 0;                      /* map.c:290-292 */
		hash ^= __ac_Wang_hash(qlen_sum) + __ac_Wang_hash(seed);
		hash  = __ac_Wang_hash(hash);
		fwrite(&hash, 4, 1, out);
		free(name);
	}
	fclose(in); fclose(out);
	return 0;
}
