/* sketch_dump.c -- test infrastructure for make_ref_sketch_fixtures.py: runs the reference's own mm_sketch (sketch.o) and mm_idx_get (index.o) on reads
 * given as raw bytes, so that every byte value can be fed (FASTA cannot carry them all).
 *
 *   sketch_dump sketch <k> <w> <is_hpc> <reads.bin> <out.bin>
 *       per read: int64 n, then n x {uint64 x, y} -- what mm_sketch appends for that read with rid 0 (collect_minimizers, map.c:64-77, n_segs = 1)
 *   sketch_dump index <k> <w> <ref.fa> <reads.bin> <out.bin> [is_hpc]
 *       the first index part of <ref.fa> (mm_idx_reader_read, MM_I_NO_SEQ) and, against it, collect_matches per read (map.c:90-123, restated):
 *       int32 mid_occ (mm_idx_cal_max_occ(mi, 2e-4), options.c:21,62-63), int64 n_pool, n_pool x uint64 pool, int64 n_keys, n_keys x {uint64 key,
 *       int64 cr_off, uint32 n}, then per read: int64 n_mini, n_mini x {x, y}; int32 rep_len; int64 n_m, n_m x {int64 cr_off, uint32 n, q_pos, q_span,
 *       seg_tandem}; n_m x uint64 mini_pos.
 *       The pool is every bucket's p[] followed by the value array of its hash table (index.c:24-31,91-94); a key is (kh_key >> 1) << b | bucket, a
 *       kh_key & 1 row has n = 1 and its hit in the value array.
 * reads.bin: int64 n_reads, int64 off[n_reads + 1], then the bytes. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "minimap.h"
#include "mmpriv.h"
#include "khash.h"

__KHASH_TYPE(idx, uint64_t, uint64_t)
typedef struct { mm128_v a; int32_t n; uint64_t *p; void *h; } idx_bucket_t;   /* struct mm_idx_bucket_s (index.c:27-32), field for field */

void mm_idxopt_init(mm_idxopt_t *io)
{
	memset(io, 0, sizeof(*io));
	io->k = 15; io->w = 10; io->flag = 0; io->bucket_bits = 14;
	io->mini_batch_size = 50000000; io->batch_size = 4000000000ULL;
}

static int64_t n_reads, *off;
static char *bases;

static void load_reads(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f || fread(&n_reads, 8, 1, f) != 1) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
	off = (int64_t *)malloc((size_t)(n_reads + 1) * 8);
	if (fread(off, 8, (size_t)n_reads + 1, f) != (size_t)n_reads + 1) exit(1);
	bases = (char *)malloc((size_t)off[n_reads] + 1);
	if (off[n_reads] && fread(bases, 1, (size_t)off[n_reads], f) != (size_t)off[n_reads]) exit(1);
	fclose(f);
}

static void sketch_one(const mm_idx_t *mi, int k, int w, int hpc, int64_t r, mm128_v *mv)
{
	int len = (int)(off[r + 1] - off[r]);
	mv->n = 0;
	if (len > 0) mm_sketch(0, bases + off[r], len, w, k, 0, hpc, mv);
	(void)mi;
}

int main(int argc, char *argv[])
{
	if (argc == 7 && strcmp(argv[1], "sketch") == 0) {
		int k = atoi(argv[2]), w = atoi(argv[3]), hpc = atoi(argv[4]);
		int64_t r;
		FILE *out;
		load_reads(argv[5]);
		out = fopen(argv[6], "wb");
		for (r = 0; r < n_reads; ++r) {
			mm128_v mv = {0, 0, 0};
			int64_t n;
			sketch_one(0, k, w, hpc, r, &mv);
			n = (int64_t)mv.n;
			fwrite(&n, 8, 1, out);
			fwrite(mv.a, 16, mv.n, out);
			free(mv.a);
		}
		fclose(out);
		return 0;
	}
	if ((argc == 7 || argc == 8) && strcmp(argv[1], "index") == 0) {
		mm_idxopt_t io;
		mm_idx_reader_t *rd;
		mm_idx_t *mi;
		const idx_bucket_t *B;
		int64_t *base_p, *base_v, n_pool = 0, n_keys = 0, r;
		int nb, i, mid_occ;
		uint64_t *pool;
		FILE *out;
		mm_verbose = 1;
		mm_idxopt_init(&io);
		io.k = atoi(argv[2]); io.w = atoi(argv[3]); io.flag |= MM_I_NO_SEQ;
		if (argc == 8 && atoi(argv[7])) io.flag |= MM_I_HPC;
		rd = mm_idx_reader_open(argv[4], &io, 0);
		if (!rd || !(mi = mm_idx_reader_read(rd, 1))) { fprintf(stderr, "cannot index %s\n", argv[4]); return 1; }
		load_reads(argv[5]);
		out = fopen(argv[6], "wb");
		mid_occ = mm_idx_cal_max_occ(mi, 2e-4f);
		fwrite(&mid_occ, 4, 1, out);
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
			if (B[i].n) memcpy(pool + base_p[i], B[i].p, (size_t)B[i].n * 8);
			if (h && h->n_buckets) {
				khint_t j;
				for (j = 0; j < h->n_buckets; ++j) pool[base_v[i] + j] = kh_exist(h, j) ? h->vals[j] : 0;   /* empty slots hold nothing meaningful */
			}
		}
		fwrite(&n_pool, 8, 1, out);
		fwrite(pool, 8, (size_t)n_pool, out);
		fwrite(&n_keys, 8, 1, out);
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
		for (r = 0; r < n_reads; ++r) {
			mm128_v mv = {0, 0, 0};
			int64_t n_mini, n_m = 0;
			int rep_st = 0, rep_en = 0, rep_len = 0;
			size_t j;
			sketch_one(mi, mi->k, mi->w, mi->flag & MM_I_HPC, r, &mv);
			n_mini = (int64_t)mv.n;
			fwrite(&n_mini, 8, 1, out);
			fwrite(mv.a, 16, mv.n, out);
			/* collect_matches (map.c:90-123) with max_occ = mid_occ, the pointer into the index turned into an offset into the pool above */
			struct { int64_t cr_off; uint32_t n, q_pos, q_span, seg_tandem; } *m = calloc(mv.n + 1, 24);
			uint64_t *mini_pos = (uint64_t *)calloc(mv.n + 1, 8);
			for (j = 0; j < mv.n; ++j) {
				mm128_t *p = &mv.a[j];
				uint32_t q_pos = (uint32_t)p->y, q_span = p->x & 0xff;
				int t;
				const uint64_t *cr = mm_idx_get(mi, p->x >> 8, &t);
				if (t >= mid_occ) {
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
			fwrite(&rep_len, 4, 1, out);
			fwrite(&n_m, 8, 1, out);
			for (j = 0; j < (size_t)n_m; ++j) {
				fwrite(&m[j].cr_off, 8, 1, out); fwrite(&m[j].n, 4, 1, out); fwrite(&m[j].q_pos, 4, 1, out);
				fwrite(&m[j].q_span, 4, 1, out); fwrite(&m[j].seg_tandem, 4, 1, out);
			}
			fwrite(mini_pos, 8, (size_t)n_m, out);
			free(m); free(mini_pos); free(mv.a);
		}
		fclose(out);
		return 0;
	}
	fprintf(stderr, "usage: %s sketch <k> <w> <is_hpc> <reads.bin> <out.bin> | index <k> <w> <ref.fa> <reads.bin> <out.bin> [is_hpc]\n", argv[0]);
	return 1;
}
