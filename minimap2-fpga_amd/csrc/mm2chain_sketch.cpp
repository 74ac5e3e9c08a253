// Reads in: the minimizer index resident on the devices, the reads-in entries and their library-owned result object.  The sketch entries and the
// sketch-and-match entries are one path each (sketch_impl, sketch_match_impl) for reads and for fragments: a read is a fragment of one segment which skips the
// tagging step (struct Batch).  The chain entries (mm2c_read_chain_batch, frag_chain_impl) are still two.  The kernels are in sketch.hip; the seed hits, the DP
// and the epilogue are the seed / chain plans of the matches-in path.
#include "api_internal.h"

using namespace mm2c_api;

namespace mm2c_api {
int sketch_count(const uint8_t *seq, const int64_t *seq_off, const int64_t *chunk_off, const int64_t *sc_off, int64_t n_reads, int64_t n_chunks, int64_t n_sc,
                 int k, int w, int hpc, void *push, void *lsum, uint64_t *sx, uint64_t *sy, uint16_t *sl, int64_t *n_slots, int64_t *cnt, int64_t *mini_off,
                 void *scan_tmp, size_t scan_bytes, hipStream_t st);
int sketch_write(const uint8_t *seq, const int64_t *seq_off, const int64_t *sc_off, int64_t n_reads, int64_t n_sc, int k, int w,
                 const uint64_t *sx, const uint64_t *sy, const uint16_t *sl, const int64_t *n_slots, const int64_t *cnt, mm2c_anchor_t *out, hipStream_t st);
int lookup_run(const mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_reads, int64_t n_mini, const uint64_t *keys, const int64_t *key_cr,
               const uint32_t *key_n, int64_t n_keys, int mid_occ, int32_t *t, int64_t *cr, int64_t *keep, int64_t *acnt, mm2c_match_t *matches,
               uint64_t *mini_pos, int64_t *match_off, int64_t *anchor_off, int32_t *rep_len, void *scan_tmp, size_t scan_bytes, hipStream_t st);
size_t sketch_scan_bytes(int64_t n_chunks, int64_t n_sc);
size_t lookup_scan_bytes(int64_t n_mini);
size_t sketch_push_bytes();
size_t sketch_lsum_bytes();
int frag_tag(mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_segs, int64_t n_mini, const uint64_t *seg_tag, const int64_t *frag_off, int64_t n_frags,
             int64_t *frag_mini_off, hipStream_t st);
int frag_gaps(const int32_t *qlen, int64_t n_frags, const mm2c_frag_gaps_t *gaps, int32_t *dists, hipStream_t st);
size_t rechain_scan_bytes(int64_t n_frags);
int rechain_decide(const int64_t *u_off, const uint64_t *u, const int64_t *b_off, const mm2c_anchor_t *b, const int32_t *rep_len, const int64_t *mini_off,
                   int64_t n_frags, int n_segs, uint8_t *flag, int64_t *cnt, int64_t *sel, int64_t *mini_off2, void *scan_tmp, size_t scan_bytes, int64_t h_n[2],
                   hipStream_t st);
int rechain_gather(const mm2c_anchor_t *mini, const int64_t *mini_off, const int64_t *sel, const int64_t *mini_off2, int64_t n_sel, int64_t n_mini2, mm2c_anchor_t *mini2,
                   hipStream_t st);
int minidx_image(const uint64_t *h_keys, const int64_t *h_cr, const uint32_t *h_n, int64_t n, int key_bits, char *d_img, int *h_dup, hipStream_t st);
// index_build.hip
int index_tag(const mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_seqs, int64_t n_mini, int64_t rid0, uint64_t *key, uint64_t *y, hipStream_t st);
size_t index_tmp_bytes(int64_t n, int key_bits, int y_bits);
int index_sort(uint64_t *key, const uint64_t *y, uint64_t *key_tmp, uint64_t *y_tmp, uint64_t *pool, int64_t n, int key_bits, int y_bits, void *tmp, size_t tmp_bytes,
               hipStream_t st);
int index_heads(const uint64_t *key, const uint64_t *y, int64_t n, int64_t *head, int64_t *row, int *bad, void *tmp, size_t tmp_bytes, hipStream_t st);
int index_rows(const uint64_t *key, const int64_t *head, const int64_t *row, int64_t n, int64_t n_keys, char *img, int *bad, hipStream_t st);
int index_count_select(const uint32_t *d_n, int64_t n_keys, int64_t i, uint32_t *h_val, hipStream_t st);
}

namespace {

struct SketchStats { std::atomic<uint64_t> calls{0}, chunks{0}, bases{0}, minimizers{0}, matches{0}, h2d_ns{0}, sketch_ns{0}, lookup_ns{0}; } SK;
struct FragStats { std::atomic<uint64_t> calls{0}, fragments{0}, rechained{0}, rechain_ns{0}; } FR;
struct IndexStats { std::atomic<uint64_t> calls{0}, chunks{0}, bases{0}, minimizers{0}, keys{0}, h2d_ns{0}, sketch_ns{0}, sort_ns{0}, group_ns{0}, occ_ns{0}, replicate_ns{0}; } IX;

// grow-only host arrays: a result object that serves many calls keeps its pages (no zeroing, no page faults on the next call)
template <class T> struct Buf {
	T *p = nullptr; size_t n = 0, cap = 0;
	~Buf() { free(p); }
	void resize(size_t m)
	{
		if (m > cap) {
			const size_t c = std::max(m, cap + cap / 2);
			T *q = (T *)realloc(p, std::max<size_t>(c, 1) * sizeof(T));
			if (!q) throw std::bad_alloc();
			p = q; cap = c;
		}
		n = m;
	}
	void assign(size_t m, T v) { resize(m); std::fill(p, p + m, v); }
	void clear() { n = 0; }
	bool empty() const { return n == 0; }
	T *data() { return p; }
	T &back() { return p[n - 1]; }
	T &operator[](size_t i) { return p[i]; }
};

struct ResPriv {
	Buf<int64_t> sketch_off, match_off, anchor_off, mini_off, u_off, b_off;
	Buf<mm2c_anchor_t> sketch, b;
	Buf<mm2c_match_t> matches;
	Buf<int32_t> rep_len;
	Buf<uint64_t> mini_pos, u;
	Buf<uint8_t> rechained;
	Buf<int32_t> task_dists;                                   // mm2c_frag_chain_batch_gaps: (max_dist_x, max_dist_y) per fragment (mm2c_read_result_task_dists)
};

void publish(mm2c_read_result_t *res, int64_t n_reads)
{
	ResPriv &P = *(ResPriv *)res->priv;
	auto off = [&](Buf<int64_t> &v) { return v.empty() ? nullptr : v.data(); };
	res->n_reads = n_reads;
	res->sketch_off = off(P.sketch_off); res->n_sketch = P.sketch_off.empty() ? 0 : P.sketch_off.back(); res->sketch = P.sketch.data();
	res->match_off = off(P.match_off); res->n_matches = P.match_off.empty() ? 0 : P.match_off.back(); res->matches = P.matches.data();
	res->anchor_off = off(P.anchor_off); res->n_anchors = P.anchor_off.empty() ? 0 : P.anchor_off.back();
	res->rep_len = P.rep_len.data();
	res->mini_off = off(P.mini_off); res->n_mini_pos = P.mini_off.empty() ? 0 : P.mini_off.back(); res->mini_pos = P.mini_pos.data();
	res->u_off = off(P.u_off); res->n_u = P.u_off.empty() ? 0 : P.u_off.back(); res->u = P.u.data();
	res->b_off = off(P.b_off); res->n_b = P.b_off.empty() ? 0 : P.b_off.back(); res->b = P.b.data();
	res->n_rechained = 0; res->rechained = nullptr;            // mm2c_frag_chain_batch fills them after this
}

void clear(mm2c_read_result_t *res)
{
	ResPriv &P = *(ResPriv *)res->priv;
	for (auto *v : { &P.sketch_off, &P.match_off, &P.anchor_off, &P.mini_off, &P.u_off, &P.b_off }) v->clear();
	P.sketch.clear(); P.b.clear(); P.matches.clear(); P.rep_len.clear(); P.mini_pos.clear(); P.u.clear(); P.rechained.clear(); P.task_dists.clear();
}

int check_reads(int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res)
{
	if (!res || !res->priv) return fail(MM2C_E_ARG, "result object is NULL (mm2c_read_result_create)");
	if (n_reads < 0 || (n_reads > 0 && !seq_off)) return fail(MM2C_E_ARG, "bad argument");
	if (n_reads > 0 && seq_off[0] != 0) return fail(MM2C_E_ARG, "seq_off[0] must be 0");
	for (int64_t r = 0; r < n_reads; ++r)
		if (seq_off[r + 1] < seq_off[r]) return fail(MM2C_E_ARG, "sequence offsets not monotone at read %lld", (long long)r);
		else if (seq_off[r + 1] - seq_off[r] > INT32_MAX) return fail(MM2C_E_TOOBIG, "read %lld is longer than 2^31 - 1 bases", (long long)r);
	if (n_reads > 0 && seq_off[n_reads] > 0 && !seq) return fail(MM2C_E_ARG, "seq is NULL");
	return 0;
}

// the fragments of a batch whose segments check_reads has accepted: frag_off runs from 0 to n_reads, 1 .. MM_MAX_SEG segments each, a total length of 31 bits
int check_frags(int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off)
{
	if (n_frags < 0 || (n_frags > 0 && !frag_off)) return fail(MM2C_E_ARG, "bad argument");
	if (n_frags == 0) return n_reads == 0 && (!frag_off || frag_off[0] == 0) ? 0 : fail(MM2C_E_ARG, "frag_off must run from 0 to n_reads");
	if (frag_off[0] != 0 || frag_off[n_frags] != n_reads) return fail(MM2C_E_ARG, "frag_off must run from 0 to n_reads");
	for (int64_t g = 0; g < n_frags; ++g) {
		const int64_t n = frag_off[g + 1] - frag_off[g];
		if (n < 0) return fail(MM2C_E_ARG, "fragment offsets not monotone at fragment %lld", (long long)g);
		if (n == 0) return fail(MM2C_E_ARG, "fragment %lld has no segment", (long long)g);
		if (n > 255) return fail(MM2C_E_ARG, "fragment %lld has %lld segments: more than MM_MAX_SEG = 255 (map.c:287)", (long long)g, (long long)n);
	}
	for (int64_t g = 0; g < n_frags; ++g)                      // monotone from 0 to n_reads: every entry indexes seq_off
		if (seq_off[frag_off[g + 1]] - seq_off[frag_off[g]] > (int64_t)INT32_MAX)
			return fail(MM2C_E_TOOBIG, "fragment %lld is longer than 2^31 - 1 bases in all (qlen_sum is an int)", (long long)g);
	// `y += sum << 1` (map.c:72) overflows the reference's int once the segments before a non-empty one hold 2^30 bases, and would spill into the segment id
	for (int64_t g = 0; g < n_frags; ++g)
		for (int64_t s = frag_off[g]; s < frag_off[g + 1]; ++s)
			if (seq_off[s + 1] > seq_off[s] && seq_off[s] - seq_off[frag_off[g]] >= ((int64_t)1 << 30))
				return fail(MM2C_E_TOOBIG, "fragment %lld: segment %lld starts 2^30 bases or more into the fragment (sum << 1 must fit an int, map.c:72)",
				            (long long)g, (long long)(s - frag_off[g]));
	return 0;
}

int check_kw(int k, int w)
{
	if (k <= 0 || k > 28) return fail(MM2C_E_ARG, "k = %d: 0 < k <= 28 (sketch.c:91)", k);
	if (w <= 0 || w >= 256) return fail(MM2C_E_ARG, "w = %d: 0 < w < 256 (sketch.c:91)", w);
	return 0;
}

struct Evts {
	hipEvent_t e[4] = {};
	int make() { for (auto &x : e) HIP_TRY(hipEventCreate(&x)); return 0; }
	~Evts() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
	float ms(int a, int b) { float v = 0; (void)hipEventElapsedTime(&v, e[a], e[b]); return v; }
};

// One run of the sketch (and the lookups) over reads [r0, r1) of the caller's batch, on `st`.  Device memory from the cache, freed by release().
struct Run {
	hipStream_t st = nullptr;
	std::vector<void *> blocks;
	int64_t nr = 0, n_mini = 0, n_matches = 0;
	int64_t *d_seq_off = nullptr, *d_mini_off = nullptr;
	mm2c_anchor_t *d_mini = nullptr;
	mm2c_match_t *d_matches = nullptr;
	uint64_t *d_mini_pos = nullptr;
	int64_t *d_match_off = nullptr, *d_anchor_off = nullptr;
	int32_t *d_rep_len = nullptr;
	std::vector<int64_t> h_seq_off, h_frag_off;
	std::vector<uint64_t> h_seg_tag;
	Evts ev;
	bool for_index = false;                    // a chunk of mm2c_minidx_build: counted in the index statistics, not in the sketch's

	hipError_t take(void **p, size_t bytes) { hipError_t e = dev_alloc(p, bytes); if (e == hipSuccess) blocks.push_back(*p); return e; }
	void release() { for (void *p : blocks) dev_free(p); blocks.clear(); }
	~Run() { release(); }

	int sketch(int k, int w, int hpc, const int64_t *seq_off, const uint8_t *seq, int64_t r0, int64_t r1)
	{
		nr = r1 - r0;
		const int64_t b0 = seq_off[r0], nb = seq_off[r1] - b0;
		h_seq_off.resize((size_t)nr + 1);
		std::vector<int64_t> chunk_off((size_t)nr + 1, 0), sc_off((size_t)nr + 1, 0);
		for (int64_t r = 0; r <= nr; ++r) h_seq_off[(size_t)r] = seq_off[r0 + r] - b0;
		for (int64_t r = 0; r < nr; ++r) {
			const int64_t L = h_seq_off[(size_t)r + 1] - h_seq_off[(size_t)r];
			chunk_off[(size_t)r + 1] = chunk_off[(size_t)r] + (L + 63) / 64;
			sc_off[(size_t)r + 1] = sc_off[(size_t)r] + (L + 255) / 256;
		}
		const int64_t n_chunks = chunk_off[(size_t)nr], n_sc = sc_off[(size_t)nr];
		const size_t scan_bytes = sketch_scan_bytes(n_chunks, n_sc);
		Layout L;
		const size_t o_seq = L.take((size_t)nb), o_so = L.take(((size_t)nr + 1) * 8), o_co = L.take(((size_t)nr + 1) * 8), o_sco = L.take(((size_t)nr + 1) * 8),
		             o_push = L.take(2 * (size_t)n_chunks * sketch_push_bytes()), o_lsum = L.take(2 * (size_t)n_chunks * sketch_lsum_bytes()),
		             o_sx = L.take((size_t)nb * 8), o_sy = L.take((size_t)nb * 8), o_sl = L.take((size_t)nb * 2), o_ns = L.take(((size_t)nr + 1) * 8),
		             o_cnt = L.take(2 * ((size_t)n_sc + 1) * 8), o_mo = L.take(((size_t)nr + 1) * 8), o_tmp = L.take(scan_bytes);
		char *d = nullptr;
		HIP_TRY(take((void **)&d, L.at));
		if (int rc0 = ev.make()) return rc0;
		HIP_TRY(hipEventRecord(ev.e[0], st));
		if (nb > 0) HIP_TRY(hipMemcpyAsync(d + o_seq, seq + b0, (size_t)nb, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_so, h_seq_off.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_co, chunk_off.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_sco, sc_off.data(), ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipEventRecord(ev.e[1], st));
		const uint8_t *d_seq = (const uint8_t *)(d + o_seq);
		d_seq_off = (int64_t *)(d + o_so); d_mini_off = (int64_t *)(d + o_mo);
		const int64_t *d_sc_off = (const int64_t *)(d + o_sco);
		int rc;
		if ((rc = sketch_count(d_seq, d_seq_off, (const int64_t *)(d + o_co), d_sc_off, nr, n_chunks, n_sc, k, w, hpc, d + o_push, d + o_lsum, (uint64_t *)(d + o_sx),
		                       (uint64_t *)(d + o_sy), (uint16_t *)(d + o_sl), (int64_t *)(d + o_ns), (int64_t *)(d + o_cnt), d_mini_off, d + o_tmp, scan_bytes, st))) return rc;
		HIP_TRY(hipMemcpyAsync(&n_mini, d_mini_off + nr, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		HIP_TRY(take((void **)&d_mini, (size_t)std::max<int64_t>(n_mini, 1) * 16));
		if ((rc = sketch_write(d_seq, d_seq_off, d_sc_off, nr, n_sc, k, w, (const uint64_t *)(d + o_sx), (const uint64_t *)(d + o_sy), (const uint16_t *)(d + o_sl),
		                       (const int64_t *)(d + o_ns), (const int64_t *)(d + o_cnt), d_mini, st))) return rc;
		HIP_TRY(hipEventRecord(ev.e[2], st));
		if (!for_index) { SK.bases += (uint64_t)nb; SK.minimizers += (uint64_t)n_mini; }
		return 0;
	}

	// after sketch() over the segments [frag_off[g0], frag_off[g1]): collect_minimizers' tagging (rid = segment number, positions shifted by the lengths of the
	// segments before, map.c:70-72), and from here on the run's "reads" are the fragments [g0, g1) with their segments' lists joined
	int to_frags(const int64_t *frag_off, int64_t g0, int64_t g1)
	{
		const int64_t ns = nr, nf = g1 - g0, s0 = frag_off[g0];
		h_frag_off.resize((size_t)nf + 1); h_seg_tag.resize((size_t)std::max<int64_t>(ns, 1));
		for (int64_t g = 0; g <= nf; ++g) h_frag_off[(size_t)g] = frag_off[g0 + g] - s0;
		for (int64_t g = 0; g < nf; ++g) {
			int sum = 0;                                           // the reference's int (map.c:66)
			for (int64_t s = h_frag_off[(size_t)g], i = 0; s < h_frag_off[(size_t)g + 1]; ++s, ++i) {
				h_seg_tag[(size_t)s] = (uint64_t)i << 32;
				h_seg_tag[(size_t)s] += (uint64_t)sum << 1;           // y += sum << 1 (check_frags: no overflow of the reference's int)
				sum += (int)(h_seq_off[(size_t)s + 1] - h_seq_off[(size_t)s]);
			}
		}
		Layout L;
		const size_t o_tag = L.take((size_t)std::max<int64_t>(ns, 1) * 8), o_fo = L.take(((size_t)nf + 1) * 8), o_fmo = L.take(((size_t)nf + 1) * 8);
		char *d = nullptr;
		HIP_TRY(take((void **)&d, L.at));
		HIP_TRY(hipMemcpyAsync(d + o_tag, h_seg_tag.data(), (size_t)std::max<int64_t>(ns, 1) * 8, hipMemcpyHostToDevice, st));
		HIP_TRY(hipMemcpyAsync(d + o_fo, h_frag_off.data(), ((size_t)nf + 1) * 8, hipMemcpyHostToDevice, st));
		if (int rc = frag_tag(d_mini, d_mini_off, ns, n_mini, (const uint64_t *)(d + o_tag), (const int64_t *)(d + o_fo), nf, (int64_t *)(d + o_fmo), st)) return rc;
		d_mini_off = (int64_t *)(d + o_fmo); nr = nf;
		return 0;
	}

	int lookup(const mm2c_minidx_t *idx, int device, int mid_occ);   // after sketch(); below
	void time_it(bool looked_up)
	{
		(void)hipEventSynchronize(looked_up ? ev.e[3] : ev.e[2]);
		SK.h2d_ns += (uint64_t)(ev.ms(0, 1) * 1e6f); SK.sketch_ns += (uint64_t)(ev.ms(1, 2) * 1e6f);
		if (looked_up) SK.lookup_ns += (uint64_t)(ev.ms(2, 3) * 1e6f);
	}
};

} // namespace

struct mm2c_minidx {
	int k = 0, w = 0, hpc = 0;
	int64_t n = 0, n_hits = 0;                   // rows; the hits they hold (sum of n)
	const mm2c_hitpool_t *pool = nullptr;
	bool owns_pool = false;                      // mm2c_minidx_build: the pool was made with the index and goes with it
	PerDevice copies;                            // [keys sorted (8 B) | cr_off (8 B) | n (4 B)] per device
};

int Run::lookup(const mm2c_minidx_t *idx, int device, int mid_occ)
{
	const char *dk = (const char *)idx->copies.on(device);
	if (!dk) return fail(MM2C_E_ARG, "the minimizer index has no copy on device %d (created before mm2c_init_devices?)", device);
	const size_t nk = (size_t)idx->n, scan_bytes = lookup_scan_bytes(n_mini), nm = (size_t)n_mini;
	Layout L;
	const size_t o_t = L.take(nm * 4), o_cr = L.take((nm + 1) * 8), o_keep = L.take(2 * (nm + 1) * 8), o_acnt = L.take(2 * (nm + 1) * 8), o_m = L.take(nm * sizeof(mm2c_match_t)),
	             o_mp = L.take(nm * 8), o_mo = L.take(((size_t)nr + 1) * 8), o_ao = L.take(((size_t)nr + 1) * 8), o_rl = L.take((size_t)nr * 4), o_tmp = L.take(scan_bytes);
	char *d = nullptr;
	HIP_TRY(take((void **)&d, L.at));
	d_matches = (mm2c_match_t *)(d + o_m); d_mini_pos = (uint64_t *)(d + o_mp);
	d_match_off = (int64_t *)(d + o_mo); d_anchor_off = (int64_t *)(d + o_ao); d_rep_len = (int32_t *)(d + o_rl);
	int rc;
	if ((rc = lookup_run(d_mini, d_mini_off, nr, n_mini, (const uint64_t *)dk, (const int64_t *)(dk + nk * 8), (const uint32_t *)(dk + nk * 16), idx->n, mid_occ,
	                     (int32_t *)(d + o_t), (int64_t *)(d + o_cr), (int64_t *)(d + o_keep), (int64_t *)(d + o_acnt), d_matches, d_mini_pos, d_match_off,
	                     d_anchor_off, d_rep_len, d + o_tmp, scan_bytes, st))) return rc;
	HIP_TRY(hipEventRecord(ev.e[3], st));
	HIP_TRY(hipMemcpyAsync(&n_matches, d_match_off + nr, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	SK.matches += (uint64_t)n_matches;
	return 0;
}

namespace {
struct OwnStream {                               // a private stream of the calling thread's device for one call
	hipStream_t st = nullptr;
	int make() { HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); return 0; }
	~OwnStream() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } }
};

// One pass of seed hits -> DP -> epilogue over the reads (or fragments) of a Run that has looked its minimizers up: the per-chunk step of mm2c_read_chain_batch and
// of both passes of mm2c_frag_chain_batch.  The chains stay in the pass's arena on the device (u_off / b_off / u / b, where the re-chain decision reads them)
// until fetch_pass() brings them down.
struct ChainPass {
	size_t nr = 0;
	int64_t tot = 0;
	std::vector<int64_t> mo, cap, off;                     // match offsets, anchor capacities; [u_off | b_off | packed anchor_off]
	const int64_t *uo = nullptr, *bo = nullptr, *ao = nullptr;
	char *d = nullptr;
	ChunkLayout o{};
	// mm2c_frag_chain_batch_gaps: every fragment of the pass chains with its own (max_dist_x, max_dist_y), made on the device from the qlen the pass uploads
	// (fr_gaps) -- the second pass's from the gathered qlen, so the pairs follow the compacted fragments.  d_dists: 2 nr words in the pass's arena
	const mm2c_frag_gaps_t *gaps = nullptr;
	int32_t *d_dists = nullptr;

	// qlen / skip: of exactly these nr reads (skip's per-read arrays start at the first of them).  on_device: u_off / b_off are wanted on the device even when
	// the chunk has no anchor at all (the re-chain decision reads them)
	int run(Run &R, const mm2c_params_t *par, int min_cnt, int min_sc, const uint64_t *d_pool, int64_t n_hits, const int32_t *qlen, const mm2c_seed_skip_host_t *skip,
	        const int32_t *d_ref, size_t n_ref, hipEvent_t ev_epi, bool on_device)
	{
		hipStream_t st = R.st;
		nr = (size_t)R.nr;
		mo.resize(nr + 1); cap.resize(nr + 1); off.assign(3 * (nr + 1), 0);
		HIP_TRY(hipMemcpyAsync(mo.data(), R.d_match_off, (nr + 1) * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(cap.data(), R.d_anchor_off, (nr + 1) * 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		tot = cap[nr];
		if (tot >= (int64_t)INT32_MAX) return fail(MM2C_E_TOOBIG, "a chunk of reads with 2^31 anchors or more (lower read_chunk_bases)");
		uo = off.data(); bo = uo + nr + 1; ao = skip ? bo + nr + 1 : cap.data();
		if (tot == 0 && !on_device) return 0;                  // no anchors at all: no read has a chain
		Layout L;
		o = chunk_layout(L, nr, (size_t)tot, skip_per_read(skip), true);   // (room for the packed anchor_off with or without skip_seed)
		const size_t o_dd = gaps ? L.take(nr * 8) : 0;
		HIP_TRY(R.take((void **)&d, L.at));
		if (gaps) {                                               // (also for a pass without anchors: the caller reads the pairs back)
			d_dists = (int32_t *)(d + o_dd);
			HIP_TRY(hipMemcpyAsync(d + o.o_q, qlen, nr * 4, hipMemcpyHostToDevice, st));
			if (int r = frag_gaps((const int32_t *)(d + o.o_q), (int64_t)nr, gaps, d_dists, st)) return r;
		}
		if (tot == 0) {
			HIP_TRY(hipMemsetAsync(d + o.o_uo, 0, (nr + 1) * 8, st));
			HIP_TRY(hipMemsetAsync(d + o.o_bo, 0, (nr + 1) * 8, st));
			if (ev_epi) HIP_TRY(hipEventRecord(ev_epi, st));
			return 0;
		}
		mm2c_seedplan_t *sp = mm2c_seedplan_create((int64_t)nr, mo.data(), cap.data());
		if (!sp) return MM2C_E_HIP;
		mm2c_plan_t *pl = mm2c_plan_create(par, (int64_t)nr, cap.data());
		if (!pl) { mm2c_seedplan_destroy(sp); return MM2C_E_HIP; }
		auto body = [&]() -> int {
			int r;
			if (gaps) { if ((r = mm2c_plan_set_task_dists(pl, d_dists))) return r; }
			else HIP_TRY(hipMemcpyAsync(d + o.o_q, qlen, nr * 4, hipMemcpyHostToDevice, st));
			mm2c_seed_skip_t sk;
			if (skip) HIP_TRY(skip_upload_reads(skip, 0, (int64_t)nr, d_ref, d_ref + n_ref, (int32_t *)(d + o.o_lo), (int32_t *)(d + o.o_eq), st, &sk));
			Evts seed;                                                // [0], [1]: around the seed hits
			if ((r = seed.make())) return r;
			HIP_TRY(hipEventRecord(seed.e[0], st));
			if ((r = chunk_step(sp, pl, R.d_matches, d_pool, n_hits, skip ? &sk : nullptr, d, o, min_cnt, min_sc, st, seed.e[1], nullptr, ev_epi, off.data()))) return r;
			HIP_TRY(hipStreamSynchronize(st));
			if ((r = mm2c_seedplan_check(sp, nullptr))) return r;
			SS.seed_ns += (uint64_t)(seed.ms(0, 1) * 1e6f);
			float pre = 0.f, dp = 0.f;                                // the plan's own timers: window prepass (and cut), DP kernels
			if ((r = mm2c_plan_last_prepass_ms(pl, &pre)) || (r = mm2c_plan_last_kernel_ms(pl, &dp))) return r;
			SS.dp_ns += (uint64_t)((pre + dp) * 1e6f);
			return 0;
		};
		const int rc = body();
		mm2c_plan_destroy(pl);
		mm2c_seedplan_destroy(sp);
		return rc;
	}
};

// the chains of a pass, the mini_pos and the rep_len of its run, down to the host (room for C.uo[nr] / C.bo[nr] / R.n_matches / nr entries); waits
int fetch_pass(Run &R, const ChainPass &C, uint64_t *u, mm2c_anchor_t *b, uint64_t *mini_pos, int32_t *rep_len)
{
	const size_t nr = C.nr;
	if (C.uo[nr]) HIP_TRY(hipMemcpyAsync(u, C.d + C.o.o_u, (size_t)C.uo[nr] * 8, hipMemcpyDeviceToHost, R.st));
	if (C.bo[nr]) HIP_TRY(hipMemcpyAsync(b, C.d + C.o.o_b, (size_t)C.bo[nr] * 16, hipMemcpyDeviceToHost, R.st));
	if (R.n_matches) HIP_TRY(hipMemcpyAsync(mini_pos, R.d_mini_pos, (size_t)R.n_matches * 8, hipMemcpyDeviceToHost, R.st));
	HIP_TRY(hipMemcpyAsync(rep_len, R.d_rep_len, nr * 4, hipMemcpyDeviceToHost, R.st));
	HIP_TRY(hipStreamSynchronize(R.st));
	return 0;
}

// the per-read arrays of a skip description from read r0 on
inline mm2c_seed_skip_host_t skip_from(const mm2c_seed_skip_host_t *skip, int64_t r0)
{
	mm2c_seed_skip_host_t s{};
	if (skip) { s = *skip; if (s.q_lo) s.q_lo += r0; if (s.q_eq) s.q_eq += r0; }
	return s;
}
}

// ---- mm2c_minidx_build: the index made on the device from the sequences (kernels in index_build.hip)
namespace {

const char *code_name(int rc)
{
	return rc == MM2C_E_NODEVICE ? "MM2C_E_NODEVICE" : rc == MM2C_E_ARG ? "MM2C_E_ARG" : rc == MM2C_E_TOOBIG ? "MM2C_E_TOOBIG" : "MM2C_E_HIP";
}

// mm2c_minidx_build returns a pointer, so the code of a failure goes in front of the message
int named(int rc)
{
	if (rc) {
		char t[sizeof(g_err)];
		snprintf(t, sizeof(t), "%s: %s", code_name(rc), g_err);
		memcpy(g_err, t, sizeof(t));
	}
	return rc;
}

// everything that can be refused without a device
int check_build_args(int k, int w, int64_t n_seqs, const int64_t *seq_off, const uint8_t *seq)
{
	if (int rc = check_kw(k, w)) return rc;
	if (n_seqs < 0 || (n_seqs > 0 && !seq_off)) return fail(MM2C_E_ARG, "bad argument");
	if (n_seqs > (int64_t)INT32_MAX) return fail(MM2C_E_TOOBIG, "%lld sequences: more than 2^31 - 1 (rid is 31 bits wide where the hits are used)", (long long)n_seqs);
	if (n_seqs > 0 && seq_off[0] != 0) return fail(MM2C_E_ARG, "seq_off[0] must be 0");
	for (int64_t r = 0; r < n_seqs; ++r)
		if (seq_off[r + 1] < seq_off[r]) return fail(MM2C_E_ARG, "sequence offsets not monotone at sequence %lld", (long long)r);
		else if (seq_off[r + 1] - seq_off[r] > (int64_t)INT32_MAX) return fail(MM2C_E_TOOBIG, "sequence %lld has 2^31 bases or more (pos << 1 must fit 32 bits)", (long long)r);
	if (n_seqs > 0 && seq_off[n_seqs] > 0 && !seq) return fail(MM2C_E_ARG, "seq is NULL");
	return 0;
}

// the growing (key, y) list of the sequences sketched so far
struct PairList {
	uint64_t *key = nullptr, *y = nullptr;
	int64_t n = 0, cap = 0;
	~PairList() { if (key) dev_free(key); if (y) dev_free(y); }
	int reserve(int64_t need, int64_t hint, hipStream_t st)
	{
		if (need <= cap) return 0;
		const int64_t c = std::max(std::max(need, hint), cap + cap / 2);
		uint64_t *k2 = nullptr, *y2 = nullptr;
		HIP_TRY(dev_alloc((void **)&k2, (size_t)c * 8));
		if (hipError_t e = dev_alloc((void **)&y2, (size_t)c * 8)) { dev_free(k2); return fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)); }
		hipError_t e = hipSuccess;
		if (n > 0) {
			e = hipMemcpyAsync(k2, key, (size_t)n * 8, hipMemcpyDeviceToDevice, st);
			if (e == hipSuccess) e = hipMemcpyAsync(y2, y, (size_t)n * 8, hipMemcpyDeviceToDevice, st);
			if (e == hipSuccess) e = hipStreamSynchronize(st);
		}
		if (e != hipSuccess) { dev_free(k2); dev_free(y2); return fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)); }
		if (key) dev_free(key); if (y) dev_free(y);
		key = k2; y = y2; cap = c;
		return 0;
	}
};

struct Block {                                   // one cached device block for the length of a scope
	void *p = nullptr;
	~Block() { if (p) dev_free(p); }
	hipError_t take(size_t bytes) { return dev_alloc(&p, bytes); }
};

inline int bits_for(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

// mm_idx_cal_max_occ over the counts of the index's image on its first device
int cal_max_occ(const mm2c_minidx *ix, float frac, int *out)
{
	*out = INT32_MAX;
	if (!(frac > 0.f) || ix->n == 0) return 0;
	const double v = (1. - (double)frac) * (double)ix->n;           // f is a float widened to double (index.c:164-185)
	int64_t i = v > 0. ? (int64_t)(uint32_t)v : 0;
	if (i >= ix->n) i = ix->n - 1;
	DeviceScope on(ix->copies.dev[0]);
	HIP_TRY(on.err);
	OwnStream os;
	if (int rc = os.make()) return rc;
	uint32_t c = 0;
	if (int rc = index_count_select((const uint32_t *)((const char *)ix->copies.d[0] + (size_t)ix->n * 16), ix->n, i, &c, os.st)) return rc;
	*out = (int)std::min<int64_t>((int64_t)c + 1, INT32_MAX);
	return 0;
}

// one more copy of `bytes` at src (device src_dev) on the current device dst_dev: device to device, through the host where that is refused
hipError_t replicate(void *dst, int dst_dev, const void *src, int src_dev, size_t bytes)
{
	if (bytes == 0) return hipSuccess;
	if (hipMemcpyPeer(dst, dst_dev, src, src_dev, bytes) == hipSuccess) return hipSuccess;
	(void)hipGetLastError();
	std::vector<char> h(bytes);
	hipError_t e;
	{ DeviceScope from(src_dev); e = from.err; if (e == hipSuccess) e = hipMemcpy(h.data(), src, bytes, hipMemcpyDeviceToHost); }
	if (e == hipSuccess) e = hipMemcpy(dst, h.data(), bytes, hipMemcpyHostToDevice);
	return e;
}

int build_index(mm2c_minidx *ix, int64_t n_seqs, const int64_t *seq_off, const uint8_t *seq, float frac, int *occ)
{
	int rc;
	const std::vector<int> devs = distinct_devices(G.devices);
	const int dev0 = devs[0];
	DeviceScope on(dev0);
	HIP_TRY(on.err);
	OwnStream os;
	if ((rc = os.make())) return rc;
	hipStream_t st = os.st;
	const int64_t total_bases = n_seqs > 0 ? seq_off[n_seqs] : 0;
	++IX.calls; IX.bases += (uint64_t)total_bases;

	// 1. sketch in chunks of whole sequences, tag, append
	PairList P;
	const int64_t chunk_bases = std::max<int64_t>(G.index_chunk_bases.load(), 1);
	for (int64_t r0 = 0; r0 < n_seqs;) {
		int64_t r1 = r0 + 1;
		while (r1 < n_seqs && seq_off[r1 + 1] - seq_off[r0] <= chunk_bases) ++r1;
		Run R; R.st = st; R.for_index = true;
		if ((rc = R.sketch(ix->k, ix->w, ix->hpc, seq_off, seq, r0, r1))) return rc;
		// room for the rest at this chunk's density, with a margin: most builds then grow the list once
		const int64_t done = seq_off[r1], left = total_bases - done;
		const int64_t hint = P.n + R.n_mini + (done > 0 ? (int64_t)((double)(P.n + R.n_mini) / (double)done * (double)left * 1.05) + 1024 : 0);
		if ((rc = P.reserve(P.n + R.n_mini, r1 < n_seqs ? hint : 0, st))) return rc;
		if ((rc = index_tag(R.d_mini, R.d_mini_off, r1 - r0, R.n_mini, r0, P.key + P.n, P.y + P.n, st))) return rc;
		HIP_TRY(hipEventRecord(R.ev.e[3], st));
		HIP_TRY(hipEventSynchronize(R.ev.e[3]));
		IX.h2d_ns += (uint64_t)(R.ev.ms(0, 1) * 1e6f); IX.sketch_ns += (uint64_t)(R.ev.ms(1, 3) * 1e6f);
		P.n += R.n_mini;
		++IX.chunks;
		r0 = r1;
	}
	const int64_t N = P.n;
	IX.minimizers += (uint64_t)N;

	// 2. order by (key, y): the y column goes straight into the pool's copy on this device
	PerDevice pool;
	hipError_t e = pool.add(dev0, (size_t)std::max<int64_t>(N, 1) * 8);
	auto guard = [&](int code) { pool.destroy(); return code; };   // until the pool object owns the copies
	if (e != hipSuccess) return fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e));
	int64_t n_keys = 0, max_rid = -1;
	if (N > 0) {
		const int key_bits = 2 * ix->k, y_bits = 32 + std::max(bits_for((uint64_t)(n_seqs - 1)), 1);
		const size_t tmp_bytes = index_tmp_bytes(N, key_bits, y_bits);
		Layout L;                                                  // key_tmp / y_tmp (the sort's other halves) are head / row afterwards: N + 1 entries each
		const size_t o_kt = L.take(((size_t)N + 1) * 8), o_yt = L.take(((size_t)N + 1) * 8), o_bad = L.take(4), o_tmp = L.take(tmp_bytes);
		Block W;
		if ((e = W.take(L.at)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
		char *d = (char *)W.p;
		uint64_t *d_pool = (uint64_t *)pool.d[0];
		{
			ScopedNs timed(IX.sort_ns);
			if ((rc = index_sort(P.key, P.y, (uint64_t *)(d + o_kt), (uint64_t *)(d + o_yt), d_pool, N, key_bits, y_bits, d + o_tmp, tmp_bytes, st))) return guard(rc);
			uint64_t last = 0;                                     // sorted by y, the last one has the largest rid
			if ((e = hipMemcpyAsync(&last, (uint64_t *)(d + o_yt) + (N - 1), 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
			    (e = hipStreamSynchronize(st)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
			max_rid = (int64_t)(last >> 32);
		}
		// 3. group
		ScopedNs timed(IX.group_ns);
		int64_t *head = (int64_t *)(d + o_kt), *row = (int64_t *)(d + o_yt);
		int *d_bad = (int *)(d + o_bad), bad = 0;
		if ((rc = index_heads(P.key, d_pool, N, head, row, d_bad, d + o_tmp, tmp_bytes, st))) return guard(rc);
		if ((e = hipMemcpyAsync(&n_keys, row + N, 8, hipMemcpyDeviceToHost, st)) != hipSuccess ||
		    (e = hipStreamSynchronize(st)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
		if (n_keys > (int64_t)UINT32_MAX) return guard(fail(MM2C_E_TOOBIG, "more than 2^32 - 1 keys"));
		if ((e = ix->copies.add(dev0, (size_t)n_keys * 20)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
		if ((rc = index_rows(P.key, head, row, N, n_keys, (char *)ix->copies.d[0], d_bad, st))) return guard(rc);
		if ((e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
		    (e = hipStreamSynchronize(st)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
		if (bad & 1) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: the sorted minimizers are not in (key, y) order"));
		if (bad & 2) return guard(fail(MM2C_E_TOOBIG, "a key with 2^32 hits or more"));
	} else if ((e = ix->copies.add(dev0, 1)) != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
	ix->n = n_keys; ix->n_hits = N;
	IX.keys += (uint64_t)n_keys;

	// 4. mid_occ
	{
		ScopedNs timed(IX.occ_ns);
		if ((rc = cal_max_occ(ix, frac, occ))) return guard(rc);
	}

	// 5. a copy of the image and of the pool on every other device
	{
		ScopedNs timed(IX.replicate_ns);
		const size_t img_bytes = (size_t)n_keys * 20, pool_bytes = (size_t)N * 8;
		for (size_t j = 1; j < devs.size(); ++j) {
			DeviceScope there(devs[j]);
			e = there.err;
			if (e == hipSuccess) e = ix->copies.add(devs[j], std::max<size_t>(img_bytes, 1));
			if (e == hipSuccess) e = replicate(ix->copies.d.back(), devs[j], ix->copies.d[0], dev0, img_bytes);
			if (e == hipSuccess) e = pool.add(devs[j], std::max<size_t>(pool_bytes, 8));
			if (e == hipSuccess) e = replicate(pool.d.back(), devs[j], pool.d[0], dev0, pool_bytes);
			if (e != hipSuccess) return guard(fail(MM2C_E_HIP, "mm2c_minidx_build: %s", hipGetErrorString(e)));
		}
	}
	ix->pool = hitpool_adopt(N, max_rid, pool);
	ix->owns_pool = true;
	return 0;
}

} // namespace

extern "C" {

mm2c_minidx_t *mm2c_minidx_create(const mm2c_hitpool_t *pool, int k, int w, int is_hpc, int64_t n_keys, const uint64_t *keys,
                                  const int64_t *cr_off, const uint32_t *n)
{
	if (!lib_ready()) { fail_not_ready(); return nullptr; }
	if (!pool) { fail(MM2C_E_ARG, "pool is NULL"); return nullptr; }
	if (check_kw(k, w)) return nullptr;
	if (n_keys < 0 || (n_keys > 0 && (!keys || !cr_off || !n))) { fail(MM2C_E_ARG, "bad argument"); return nullptr; }
	const int64_t pool_n = mm2c_hitpool_size(pool);
	const uint64_t lim = 1ULL << 2 * k;
	for (int64_t i = 0; i < n_keys; ++i) {
		if (keys[i] >= lim) { fail(MM2C_E_ARG, "key %lld is %llu, not below 2^(2k) = %llu", (long long)i, (unsigned long long)keys[i], (unsigned long long)lim); return nullptr; }
		if (cr_off[i] < 0 || cr_off[i] + (int64_t)n[i] > pool_n) { fail(MM2C_E_ARG, "row %lld reaches beyond the pool of %lld hits", (long long)i, (long long)pool_n); return nullptr; }
	}
	if (n_keys > (int64_t)UINT32_MAX) { fail(MM2C_E_TOOBIG, "more than 2^32 - 1 keys"); return nullptr; }
	const size_t nk = (size_t)n_keys, img_bytes = std::max<size_t>(nk * 20, 1);
	std::vector<char> img;                                    // the sorted image, downloaded once when a second device needs a copy
	mm2c_minidx *ix = new mm2c_minidx();
	ix->k = k; ix->w = w; ix->hpc = is_hpc ? 1 : 0; ix->n = n_keys; ix->pool = pool;
	for (int64_t i = 0; i < n_keys; ++i) ix->n_hits += (int64_t)n[i];
	for (int dv : distinct_devices(G.devices)) {
		DeviceScope on(dv);
		hipError_t e = on.err;
		if (e == hipSuccess) e = ix->copies.add(dv, img_bytes);
		if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_minidx_create: %s", hipGetErrorString(e)); mm2c_minidx_destroy(ix); return nullptr; }
		void *p = ix->copies.d.back();
		if (ix->copies.d.size() == 1) {                        // sorted on the first device
			OwnStream os;
			int dup = 0, rc = os.make();
			if (rc == 0) rc = minidx_image(keys, cr_off, n, n_keys, 2 * k, (char *)p, &dup, os.st);
			if (rc == 0 && dup) rc = fail(MM2C_E_ARG, "duplicate key in the index");
			if (rc) { mm2c_minidx_destroy(ix); return nullptr; }
			continue;
		}
		if (img.empty()) {
			img.resize(img_bytes);
			DeviceScope first(ix->copies.dev[0]);
			e = first.err;
			if (e == hipSuccess) e = hipMemcpy(img.data(), ix->copies.d[0], img_bytes, hipMemcpyDeviceToHost);
		}
		if (e == hipSuccess) e = hipMemcpy(p, img.data(), img_bytes, hipMemcpyHostToDevice);
		if (e != hipSuccess) { fail(MM2C_E_HIP, "mm2c_minidx_create: %s", hipGetErrorString(e)); mm2c_minidx_destroy(ix); return nullptr; }
	}
	return ix;
}

void mm2c_minidx_destroy(mm2c_minidx_t *ix)
{
	if (!ix) return;
	ix->copies.destroy();
	if (ix->owns_pool) mm2c_hitpool_destroy(const_cast<mm2c_hitpool_t *>(ix->pool));
	delete ix;
}

mm2c_minidx_t *mm2c_minidx_build(int k, int w, int is_hpc, int64_t n_seqs, const int64_t *seq_off, const uint8_t *seq, float mid_occ_frac, int *mid_occ)
{
	if (named(check_build_args(k, w, n_seqs, seq_off, seq))) return nullptr;   // before any device work
	if (!lib_ready()) { named(fail_not_ready()); return nullptr; }
	mm2c_minidx *ix = new mm2c_minidx();
	ix->k = k; ix->w = w; ix->hpc = is_hpc ? 1 : 0;
	int occ = INT32_MAX, rc;
	try { rc = build_index(ix, n_seqs, seq_off, seq, mid_occ_frac, &occ); }
	catch (const std::bad_alloc &) { rc = fail(MM2C_E_HIP, "mm2c_minidx_build: out of host memory"); }
	if (named(rc)) { mm2c_minidx_destroy(ix); return nullptr; }
	if (mid_occ) *mid_occ = occ;
	return ix;
}

int64_t mm2c_minidx_n_keys(const mm2c_minidx_t *idx) { return idx ? idx->n : 0; }
int64_t mm2c_minidx_n_hits(const mm2c_minidx_t *idx) { return idx ? idx->n_hits : 0; }
const mm2c_hitpool_t *mm2c_minidx_pool(const mm2c_minidx_t *idx) { return idx ? idx->pool : nullptr; }

int mm2c_minidx_cal_max_occ(const mm2c_minidx_t *idx, float frac)
{
	if (!lib_ready()) return fail_not_ready();
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	int occ = INT32_MAX;
	if (int rc = cal_max_occ(idx, frac, &occ)) return rc;
	return occ;
}

int mm2c_minidx_export(const mm2c_minidx_t *idx, uint64_t *keys, int64_t *cr_off, uint32_t *n, uint64_t *pool)
{
	if (!lib_ready()) return fail_not_ready();
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	const int dev = idx->copies.dev[0];
	DeviceScope on(dev);
	HIP_TRY(on.err);
	const char *img = (const char *)idx->copies.d[0];
	const size_t nk = (size_t)idx->n;
	if (nk && keys) HIP_TRY(hipMemcpy(keys, img, nk * 8, hipMemcpyDeviceToHost));
	if (nk && cr_off) HIP_TRY(hipMemcpy(cr_off, img + nk * 8, nk * 8, hipMemcpyDeviceToHost));
	if (nk && n) HIP_TRY(hipMemcpy(n, img + nk * 16, nk * 4, hipMemcpyDeviceToHost));
	if (pool && idx->owns_pool && idx->n_hits > 0) {
		const uint64_t *d_pool = hitpool_on(idx->pool, dev);
		if (!d_pool) return fail(MM2C_E_ARG, "the hit pool has no copy on device %d", dev);
		HIP_TRY(hipMemcpy(pool, d_pool, (size_t)idx->n_hits * 8, hipMemcpyDeviceToHost));
	}
	return 0;
}

void mm2c_get_index_stats(mm2c_index_stats_t *out)
{
	if (!out) return;
	*out = mm2c_index_stats_t{ IX.calls, IX.chunks, IX.bases, IX.minimizers, IX.keys, IX.h2d_ns, IX.sketch_ns, IX.sort_ns, IX.group_ns, IX.occ_ns, IX.replicate_ns };
}

void mm2c_reset_index_stats(void)
{
	for (auto *a : { &IX.calls, &IX.chunks, &IX.bases, &IX.minimizers, &IX.keys, &IX.h2d_ns, &IX.sketch_ns, &IX.sort_ns, &IX.group_ns, &IX.occ_ns, &IX.replicate_ns }) *a = 0;
}

mm2c_read_result_t *mm2c_read_result_create(void)
{
	mm2c_read_result_t *res = new mm2c_read_result_t();
	res->priv = new ResPriv();
	return res;
}

void mm2c_read_result_free(mm2c_read_result_t *res)
{
	if (!res) return;
	delete (ResPriv *)res->priv;
	delete res;
}

int mm2c_minidx_lookup(const mm2c_minidx_t *idx, int64_t n_q, const uint64_t *keys, int64_t *cr_off, uint32_t *n)
{
	if (!lib_ready()) return fail_not_ready();
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	if (n_q < 0 || (n_q > 0 && (!keys || !cr_off || !n))) return fail(MM2C_E_ARG, "bad argument");
	if (n_q == 0) return 0;
	// the lookups of collect_matches on a made-up read whose minimizers are the keys (keys that no index of this k can hold are answered here)
	std::vector<int64_t> pos;
	std::vector<mm2c_anchor_t> mini;
	for (int64_t i = 0; i < n_q; ++i) {
		cr_off[i] = 0; n[i] = 0;
		if (keys[i] < (1ULL << 2 * idx->k)) { pos.push_back(i); mini.push_back(mm2c_anchor_t{ keys[i] << 8, 0 }); }
	}
	if (mini.empty()) return 0;
	const int device = cur_device();
	DeviceScope on(device);
	HIP_TRY(on.err);
	OwnStream os;
	int rc;
	if ((rc = os.make())) return rc;
	Run R; R.st = os.st; R.nr = 1; R.n_mini = (int64_t)mini.size();
	const int64_t mo[2] = { 0, R.n_mini };
	HIP_TRY(R.take((void **)&R.d_mini, mini.size() * 16));
	HIP_TRY(R.take((void **)&R.d_mini_off, 16));
	HIP_TRY(hipMemcpyAsync(R.d_mini, mini.data(), mini.size() * 16, hipMemcpyHostToDevice, os.st));
	HIP_TRY(hipMemcpyAsync(R.d_mini_off, mo, 16, hipMemcpyHostToDevice, os.st));
	if ((rc = R.ev.make())) return rc;
	HIP_TRY(hipEventRecord(R.ev.e[2], os.st));
	if ((rc = R.lookup(idx, device, INT32_MAX))) return rc;
	std::vector<mm2c_match_t> m((size_t)R.n_matches);
	HIP_TRY(hipMemcpy(m.data(), R.d_matches, m.size() * sizeof(mm2c_match_t), hipMemcpyDeviceToHost));
	for (size_t j = 0; j < m.size() && j < pos.size(); ++j) { cr_off[pos[j]] = m[j].cr_off; n[pos[j]] = m[j].n; }
	return 0;
}

int mm2c_read_chain_batch(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int64_t n_reads,
                          const int64_t *seq_off, const uint8_t *seq, const mm2c_seed_skip_host_t *skip, mm2c_read_result_t *res)
{
	int rc;
	if (!lib_ready()) return fail_not_ready();
	if ((rc = check_params(par))) return rc;
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	if ((rc = check_reads(n_reads, seq_off, seq, res))) return rc;
	if (skip && (rc = check_skip_pool(skip, n_reads, idx->pool))) return rc;
	ScopedNs timed_total(SS.total_ns);
	clear(res);
	ResPriv &P = *(ResPriv *)res->priv;
	for (auto *v : { &P.anchor_off, &P.mini_off, &P.u_off, &P.b_off }) v->assign((size_t)n_reads + 1, 0);
	P.rep_len.assign((size_t)n_reads, 0);
	if (n_reads == 0) { publish(res, 0); return 0; }
	const int device = cur_device();
	DeviceScope on(device);
	HIP_TRY(on.err);
	const uint64_t *d_pool = hitpool_on(idx->pool, device);
	if (!d_pool) return fail(MM2C_E_ARG, "the hit pool has no copy on device %d", device);
	const int64_t n_hits = mm2c_hitpool_size(idx->pool);
	OwnStream os;
	if ((rc = os.make())) return rc;
	hipStream_t st = os.st;
	++SS.calls;
	const size_t n_ref = skip_n_ref(skip);
	Run refs; refs.st = st;                                    // [ref_rank | ref_len] once per call
	int32_t *d_ref = nullptr;
	if (n_ref) {
		HIP_TRY(refs.take((void **)&d_ref, 2 * n_ref * 4));
		HIP_TRY(skip_upload_refs(skip, d_ref, d_ref + n_ref, st));
	}
	const int64_t chunk_bases = std::max<int64_t>(G.read_chunk_bases.load(), 1);
	int64_t A = 0, U = 0, B = 0, M = 0;
	for (int64_t r0 = 0; r0 < n_reads;) {
		int64_t r1 = r0 + 1;
		while (r1 < n_reads && seq_off[r1 + 1] - seq_off[r0] <= chunk_bases) ++r1;
		const size_t nr = (size_t)(r1 - r0);
		Run R; R.st = st;
		if ((rc = R.sketch(idx->k, idx->w, idx->hpc, seq_off, seq, r0, r1)) || (rc = R.lookup(idx, device, mid_occ))) return rc;
		R.time_it(true);
		std::vector<int32_t> qlen(nr);
		for (size_t r = 0; r < nr; ++r) qlen[r] = (int32_t)(seq_off[r0 + (int64_t)r + 1] - seq_off[r0 + (int64_t)r]);
		const mm2c_seed_skip_host_t sk = skip_from(skip, r0);
		ChainPass C;
		if ((rc = C.run(R, par, min_cnt, min_sc, d_pool, n_hits, qlen.data(), skip ? &sk : nullptr, d_ref, n_ref, nullptr, false))) return rc;
		P.u.resize((size_t)(U + C.uo[nr])); P.b.resize((size_t)(B + C.bo[nr])); P.mini_pos.resize((size_t)(M + R.n_matches));
		if ((rc = fetch_pass(R, C, P.u.data() + U, P.b.data() + B, P.mini_pos.data() + M, P.rep_len.data() + r0))) return rc;
		for (size_t k = 1; k <= nr; ++k) {
			P.mini_off[(size_t)r0 + k] = M + C.mo[k];
			P.u_off[(size_t)r0 + k] = U + C.uo[k]; P.b_off[(size_t)r0 + k] = B + C.bo[k]; P.anchor_off[(size_t)r0 + k] = A + C.ao[k];
		}
		M += R.n_matches; U += C.uo[nr]; B += C.bo[nr]; A += C.ao[nr];
		++SK.chunks; ++SS.chunks;
		r0 = r1;
	}
	++SK.calls;
	G.tasks += (uint64_t)n_reads; G.anchors += (uint64_t)A;
	publish(res, n_reads);
	return 0;
}

// ---- fragments of several segments and the max_occ re-chain
} // extern "C"

namespace {

// what one pass left for its fragments, on the host
struct PassHost {
	std::vector<uint64_t> u, mini_pos;
	std::vector<mm2c_anchor_t> b;
	std::vector<int32_t> rep_len;
	int fetch(Run &R, ChainPass &C)
	{
		u.resize((size_t)C.uo[C.nr]); b.resize((size_t)C.bo[C.nr]); mini_pos.resize((size_t)R.n_matches); rep_len.resize(C.nr);
		return fetch_pass(R, C, u.data(), b.data(), mini_pos.data(), rep_len.data());
	}
};

// the checks the three fragment entries share, before any device work
int check_frag_call(int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res)
{
	if (int rc = check_reads(n_reads, seq_off, seq, res)) return rc;
	return check_frags(n_frags, frag_off, n_reads, seq_off);
}

// The input of a reads-in call: n_items reads, or fragments of the segments frag_off groups.  A read is a fragment of one segment: with frag_off == NULL the
// segment of item g is g, and the tagging step (Run::to_frags) would add zero to every y and copy mini_off, so it is skipped.
struct Batch {
	int64_t n_items;
	const int64_t *frag_off;
	int64_t n_reads;                                           // segments
	const int64_t *seq_off;
	const uint8_t *seq;
	bool as_frags;                                             // a fragment entry's call: frag_off is checked (NULL is legal for an empty batch only), FR counts
	int64_t seg(int64_t g) const { return frag_off ? frag_off[g] : g; }                                  // items [g0, g1) are the segments [seg(g0), seg(g1))
	int64_t bases(int64_t g0, int64_t g1) const { return seq_off[seg(g1)] - seq_off[seg(g0)]; }
};

Batch reads_of(int64_t n_reads, const int64_t *seq_off, const uint8_t *seq) { return Batch{ n_reads, nullptr, n_reads, seq_off, seq, false }; }
Batch frags_of(int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq)
{
	return Batch{ n_frags, frag_off, n_reads, seq_off, seq, true };
}

// the checks the entries share, before any device work
int check_batch(const Batch &b, mm2c_read_result_t *res)
{
	if (int rc = check_reads(b.n_reads, b.seq_off, b.seq, res)) return rc;
	return b.as_frags ? check_frags(b.n_items, b.frag_off, b.n_reads, b.seq_off) : 0;
}

// R sketches the items [g0, g1) and, where they are fragments, joins their segments' lists
int sketch_items(Run &R, int k, int w, int hpc, const Batch &b, int64_t g0, int64_t g1)
{
	if (int rc = R.sketch(k, w, hpc, b.seq_off, b.seq, b.seg(g0), b.seg(g1))) return rc;
	return b.frag_off ? R.to_frags(b.frag_off, g0, g1) : 0;
}

// mm2c_sketch_batch and mm2c_sketch_frag_batch
int sketch_impl(int k, int w, int hpc, const Batch &b, mm2c_read_result_t *res)
{
	int rc;
	if ((rc = check_kw(k, w)) || (rc = check_batch(b, res))) return rc;
	if (!lib_ready()) return fail_not_ready();
	clear(res);
	ResPriv &P = *(ResPriv *)res->priv;
	const int64_t n = b.n_items;
	P.sketch_off.assign((size_t)n + 1, 0);
	if (n > 0) {
		DeviceScope on(cur_device());
		HIP_TRY(on.err);
		OwnStream os;
		if ((rc = os.make())) return rc;
		Run R; R.st = os.st;
		if ((rc = sketch_items(R, k, w, hpc, b, 0, n))) return rc;
		P.sketch.resize((size_t)R.n_mini);
		HIP_TRY(hipMemcpyAsync(P.sketch_off.data(), R.d_mini_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, os.st));
		if (R.n_mini) HIP_TRY(hipMemcpyAsync(P.sketch.data(), R.d_mini, (size_t)R.n_mini * 16, hipMemcpyDeviceToHost, os.st));
		HIP_TRY(hipStreamSynchronize(os.st));
		R.time_it(false);
		++SK.calls; ++SK.chunks;
	}
	if (b.as_frags) { ++FR.calls; FR.fragments += (uint64_t)n; }
	publish(res, n);
	return 0;
}

// mm2c_sketch_match_batch and mm2c_sketch_match_frag_batch
int sketch_match_impl(const mm2c_minidx_t *idx, int occ, const Batch &b, mm2c_read_result_t *res)
{
	int rc;
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	if ((rc = check_batch(b, res))) return rc;
	if (!lib_ready()) return fail_not_ready();
	clear(res);
	ResPriv &P = *(ResPriv *)res->priv;
	const int64_t n = b.n_items;
	P.match_off.assign((size_t)n + 1, 0); P.anchor_off.assign((size_t)n + 1, 0); P.mini_off.assign((size_t)n + 1, 0);
	P.rep_len.assign((size_t)n, 0);
	if (n > 0) {
		const int device = cur_device();
		DeviceScope on(device);
		HIP_TRY(on.err);
		OwnStream os;
		if ((rc = os.make())) return rc;
		Run R; R.st = os.st;
		if ((rc = sketch_items(R, idx->k, idx->w, idx->hpc, b, 0, n)) || (rc = R.lookup(idx, device, occ))) return rc;
		P.matches.resize((size_t)R.n_matches); P.mini_pos.resize((size_t)R.n_matches);
		HIP_TRY(hipMemcpyAsync(P.match_off.data(), R.d_match_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, os.st));
		HIP_TRY(hipMemcpyAsync(P.anchor_off.data(), R.d_anchor_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, os.st));
		HIP_TRY(hipMemcpyAsync(P.rep_len.data(), R.d_rep_len, (size_t)n * 4, hipMemcpyDeviceToHost, os.st));
		if (R.n_matches) {
			HIP_TRY(hipMemcpyAsync(P.matches.data(), R.d_matches, (size_t)R.n_matches * sizeof(mm2c_match_t), hipMemcpyDeviceToHost, os.st));
			HIP_TRY(hipMemcpyAsync(P.mini_pos.data(), R.d_mini_pos, (size_t)R.n_matches * 8, hipMemcpyDeviceToHost, os.st));
		}
		HIP_TRY(hipStreamSynchronize(os.st));
		std::copy(P.match_off.p, P.match_off.p + P.match_off.n, P.mini_off.p);   // one mini_pos per kept match
		R.time_it(true);
		++SK.calls; ++SK.chunks;
	}
	if (b.as_frags) { ++FR.calls; FR.fragments += (uint64_t)n; }
	publish(res, n);
	return 0;
}

} // namespace

extern "C" {

// The read entries answer "not initialised" before any argument check; the fragment entries check every argument first.
int mm2c_sketch_batch(int k, int w, int is_hpc, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res)
{
	if (!lib_ready()) return fail_not_ready();
	return sketch_impl(k, w, is_hpc ? 1 : 0, reads_of(n_reads, seq_off, seq), res);
}

int mm2c_sketch_frag_batch(int k, int w, int is_hpc, int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq,
                           mm2c_read_result_t *res)
{
	return sketch_impl(k, w, is_hpc ? 1 : 0, frags_of(n_frags, frag_off, n_reads, seq_off, seq), res);
}

int mm2c_sketch_match_batch(const mm2c_minidx_t *idx, int mid_occ, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, mm2c_read_result_t *res)
{
	if (!lib_ready()) return fail_not_ready();
	return sketch_match_impl(idx, mid_occ, reads_of(n_reads, seq_off, seq), res);
}

int mm2c_sketch_match_frag_batch(const mm2c_minidx_t *idx, int occ, int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off,
                                 const uint8_t *seq, mm2c_read_result_t *res)
{
	return sketch_match_impl(idx, occ, frags_of(n_frags, frag_off, n_reads, seq_off, seq), res);
}

// mm2c_frag_chain_batch (gaps == NULL: par's distances for every fragment) and mm2c_frag_chain_batch_gaps (every fragment its own pair, made on the device)
static int frag_chain_impl(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int max_occ, const mm2c_frag_gaps_t *gaps, int64_t n_frags,
                           const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, const mm2c_seed_skip_host_t *skip,
                           mm2c_read_result_t *res)
{
	int rc;
	if ((rc = check_params(par))) return rc;
	if (!idx) return fail(MM2C_E_ARG, "minimizer index is NULL");
	if ((rc = check_frag_call(n_frags, frag_off, n_reads, seq_off, seq, res))) return rc;
	for (int64_t g = 0; g < n_frags; ++g)
		if (frag_off[g + 1] - frag_off[g] != (int64_t)par->n_segs)
			return fail(MM2C_E_ARG, "fragment %lld has %lld segments, par->n_segs is %d (mm_chain_dp gets the fragment's own n_segs: one call per segment count)",
			            (long long)g, (long long)(frag_off[g + 1] - frag_off[g]), (int)par->n_segs);
	if (skip && (rc = check_skip_pool(skip, n_frags, idx->pool))) return rc;
	if (!lib_ready()) return fail_not_ready();
	ScopedNs timed_total(SS.total_ns);
	clear(res);
	ResPriv &P = *(ResPriv *)res->priv;
	for (auto *v : { &P.anchor_off, &P.mini_off, &P.u_off, &P.b_off }) v->assign((size_t)n_frags + 1, 0);
	P.rep_len.assign((size_t)n_frags, 0); P.rechained.assign((size_t)n_frags, 0);
	if (gaps) P.task_dists.assign(2 * (size_t)n_frags, 0);
	++FR.calls;
	if (n_frags == 0) { publish(res, 0); return 0; }
	const int device = cur_device();
	DeviceScope on(device);
	HIP_TRY(on.err);
	const uint64_t *d_pool = hitpool_on(idx->pool, device);
	if (!d_pool) return fail(MM2C_E_ARG, "the hit pool has no copy on device %d", device);
	const int64_t n_hits = mm2c_hitpool_size(idx->pool);
	OwnStream os;
	if ((rc = os.make())) return rc;
	hipStream_t st = os.st;
	++SS.calls;
	const size_t n_ref = skip_n_ref(skip);
	Run refs; refs.st = st;                                    // [ref_rank | ref_len] once per call
	int32_t *d_ref = nullptr;
	if (n_ref) {
		HIP_TRY(refs.take((void **)&d_ref, 2 * n_ref * 4));
		HIP_TRY(skip_upload_refs(skip, d_ref, d_ref + n_ref, st));
	}
	const bool two_pass = max_occ > mid_occ;                   // map.c:318
	const int64_t chunk_bases = std::max<int64_t>(G.read_chunk_bases.load(), 1);
	auto bases = [&](int64_t g0, int64_t g1) { return seq_off[frag_off[g1]] - seq_off[frag_off[g0]]; };
	int64_t A = 0, U = 0, B = 0, M = 0, n_rechained = 0;
	for (int64_t g0 = 0; g0 < n_frags;) {                      // chunks of whole fragments
		int64_t g1 = g0 + 1;
		while (g1 < n_frags && bases(g0, g1 + 1) <= chunk_bases) ++g1;
		const size_t nf = (size_t)(g1 - g0);
		Run R; R.st = st;
		if ((rc = R.sketch(idx->k, idx->w, idx->hpc, seq_off, seq, frag_off[g0], frag_off[g1])) || (rc = R.to_frags(frag_off, g0, g1)) ||
		    (rc = R.lookup(idx, device, mid_occ))) return rc;
		R.time_it(true);
		std::vector<int32_t> qlen(nf);
		for (size_t g = 0; g < nf; ++g) qlen[g] = (int32_t)bases(g0 + (int64_t)g, g0 + (int64_t)g + 1);   // qlen_sum
		const mm2c_seed_skip_host_t sk1 = skip_from(skip, g0);
		ChainPass C1, C2;
		C1.gaps = gaps; C2.gaps = gaps;
		if ((rc = C1.run(R, par, min_cnt, min_sc, d_pool, n_hits, qlen.data(), skip ? &sk1 : nullptr, d_ref, n_ref, nullptr, true))) return rc;

		// the second pass: decided and compacted on the device, looked up with max_occ, chained like the first
		Run R2; R2.st = st;
		int64_t n2[2] = { 0, 0 };
		std::vector<int64_t> sel;
		uint8_t *flags = P.rechained.data() + g0;
		if (two_pass) {
			Evts ev;
			if ((rc = ev.make())) return rc;
			HIP_TRY(hipEventRecord(ev.e[0], st));
			const size_t scan_bytes = rechain_scan_bytes((int64_t)nf);
			Layout L;
			const size_t o_flag = L.take(nf), o_cnt = L.take(4 * (nf + 1) * 8), o_sel = L.take(nf * 8), o_mo2 = L.take((nf + 1) * 8), o_tmp = L.take(scan_bytes);
			char *d = nullptr;
			HIP_TRY(R.take((void **)&d, L.at));
			if ((rc = rechain_decide((const int64_t *)(C1.d + C1.o.o_uo), (const uint64_t *)(C1.d + C1.o.o_u), (const int64_t *)(C1.d + C1.o.o_bo),
			                         (const mm2c_anchor_t *)(C1.d + C1.o.o_b), R.d_rep_len, R.d_mini_off, (int64_t)nf, par->n_segs, (uint8_t *)(d + o_flag),
			                         (int64_t *)(d + o_cnt), (int64_t *)(d + o_sel), (int64_t *)(d + o_mo2), d + o_tmp, scan_bytes, n2, st))) return rc;
			if (n2[0] > 0) {
				sel.resize((size_t)n2[0]);
				HIP_TRY(hipMemcpyAsync(flags, d + o_flag, nf, hipMemcpyDeviceToHost, st));
				HIP_TRY(hipMemcpyAsync(sel.data(), d + o_sel, sel.size() * 8, hipMemcpyDeviceToHost, st));
				R2.nr = n2[0]; R2.n_mini = n2[1]; R2.d_mini_off = (int64_t *)(d + o_mo2);
				HIP_TRY(R2.take((void **)&R2.d_mini, (size_t)std::max<int64_t>(n2[1], 1) * 16));
				if ((rc = rechain_gather(R.d_mini, R.d_mini_off, (const int64_t *)(d + o_sel), R2.d_mini_off, n2[0], n2[1], R2.d_mini, st))) return rc;
				if ((rc = R2.ev.make())) return rc;
				if ((rc = R2.lookup(idx, device, max_occ))) return rc;       // (waits for the stream: flags and sel are down)
				std::vector<int32_t> qlen2(sel.size()), lo2, eq2;
				for (size_t j = 0; j < sel.size(); ++j) qlen2[j] = qlen[(size_t)sel[j]];
				mm2c_seed_skip_host_t sk2{};
				if (skip) {
					sk2 = sk1;
					if (sk1.q_lo) { lo2.resize(sel.size()); for (size_t j = 0; j < sel.size(); ++j) lo2[j] = sk1.q_lo[sel[j]]; sk2.q_lo = lo2.data(); }
					if (sk1.q_eq) { eq2.resize(sel.size()); for (size_t j = 0; j < sel.size(); ++j) eq2[j] = sk1.q_eq[sel[j]]; sk2.q_eq = eq2.data(); }
				}
				if ((rc = C2.run(R2, par, min_cnt, min_sc, d_pool, n_hits, qlen2.data(), skip ? &sk2 : nullptr, d_ref, n_ref, ev.e[1], true))) return rc;
			} else HIP_TRY(hipEventRecord(ev.e[1], st));
			HIP_TRY(hipEventSynchronize(ev.e[1]));
			FR.rechain_ns += (uint64_t)(ev.ms(0, 1) * 1e6f);
		}

		// down, in fragment order: a re-chained fragment's second-pass results in the place of its first-pass ones
		PassHost H1, H2;
		if (gaps) HIP_TRY(hipMemcpyAsync(P.task_dists.data() + 2 * g0, C1.d_dists, nf * 8, hipMemcpyDeviceToHost, st));   // (the fetch below waits for the stream)
		if ((rc = H1.fetch(R, C1)) || (n2[0] > 0 && (rc = H2.fetch(R2, C2)))) return rc;
		size_t j = 0;
		for (size_t g = 0; g < nf; ++g) {
			const bool second = n2[0] > 0 && flags[g];
			const ChainPass &C = second ? C2 : C1;
			const PassHost &H = second ? H2 : H1;
			const size_t q = second ? j++ : g;
			const int64_t nu = C.uo[q + 1] - C.uo[q], nb = C.bo[q + 1] - C.bo[q], nm = C.mo[q + 1] - C.mo[q], na = C.ao[q + 1] - C.ao[q];
			P.u.resize((size_t)(U + nu)); P.b.resize((size_t)(B + nb)); P.mini_pos.resize((size_t)(M + nm));
			if (nu) memcpy(P.u.data() + U, H.u.data() + C.uo[q], (size_t)nu * 8);
			if (nb) memcpy(P.b.data() + B, H.b.data() + C.bo[q], (size_t)nb * 16);
			if (nm) memcpy(P.mini_pos.data() + M, H.mini_pos.data() + C.mo[q], (size_t)nm * 8);
			U += nu; B += nb; M += nm; A += na;
			const size_t at = (size_t)g0 + g;
			P.rep_len[at] = H.rep_len[q];
			P.u_off[at + 1] = U; P.b_off[at + 1] = B; P.mini_off[at + 1] = M; P.anchor_off[at + 1] = A;
		}
		n_rechained += n2[0];
		++SK.chunks; ++SS.chunks;
		g0 = g1;
	}
	++SK.calls;
	FR.fragments += (uint64_t)n_frags; FR.rechained += (uint64_t)n_rechained;
	G.tasks += (uint64_t)n_frags; G.anchors += (uint64_t)A;
	publish(res, n_frags);
	res->n_rechained = n_rechained; res->rechained = P.rechained.data();
	return 0;
}

int mm2c_frag_chain_batch(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int max_occ, int64_t n_frags,
                          const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq, const mm2c_seed_skip_host_t *skip,
                          mm2c_read_result_t *res)
{
	return frag_chain_impl(par, min_cnt, min_sc, idx, mid_occ, max_occ, nullptr, n_frags, frag_off, n_reads, seq_off, seq, skip, res);
}

int mm2c_frag_chain_batch_gaps(const mm2c_params_t *par, int min_cnt, int min_sc, const mm2c_minidx_t *idx, int mid_occ, int max_occ, const mm2c_frag_gaps_t *gaps,
                               int64_t n_frags, const int64_t *frag_off, int64_t n_reads, const int64_t *seq_off, const uint8_t *seq,
                               const mm2c_seed_skip_host_t *skip, mm2c_read_result_t *res)
{
	if (!gaps) return fail(MM2C_E_ARG, "gaps is NULL (mm2c_frag_chain_batch takes the distances from par)");
	if (gaps->max_gap < 0) return fail(MM2C_E_ARG, "max_gap must be >= 0 (got %d)", (int)gaps->max_gap);
	return frag_chain_impl(par, min_cnt, min_sc, idx, mid_occ, max_occ, gaps, n_frags, frag_off, n_reads, seq_off, seq, skip, res);
}

int mm2c_read_result_task_dists(const mm2c_read_result_t *res, const int32_t **dists, int64_t *n_frags)
{
	if (!res || !res->priv || !dists || !n_frags) return fail(MM2C_E_ARG, "NULL argument");
	ResPriv &P = *(ResPriv *)res->priv;
	*dists = P.task_dists.empty() ? nullptr : P.task_dists.data();
	*n_frags = (int64_t)(P.task_dists.n / 2);
	return 0;
}

void mm2c_get_frag_stats(mm2c_frag_stats_t *out)
{
	if (!out) return;
	*out = mm2c_frag_stats_t{ FR.calls, FR.fragments, FR.rechained, FR.rechain_ns };
}

void mm2c_reset_frag_stats(void)
{
	for (auto *a : { &FR.calls, &FR.fragments, &FR.rechained, &FR.rechain_ns }) *a = 0;
}

void mm2c_get_sketch_stats(mm2c_sketch_stats_t *out)
{
	if (!out) return;
	*out = mm2c_sketch_stats_t{ SK.calls, SK.chunks, SK.bases, SK.minimizers, SK.matches, SK.h2d_ns, SK.sketch_ns, SK.lookup_ns };
}

void mm2c_reset_sketch_stats(void)
{
	for (auto *a : { &SK.calls, &SK.chunks, &SK.bases, &SK.minimizers, &SK.matches, &SK.h2d_ns, &SK.sketch_ns, &SK.lookup_ns }) *a = 0;
}

} // extern "C"
