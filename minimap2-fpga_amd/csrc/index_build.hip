// Building the minimizer index on the device: what mm_idx_gen + worker_post (index.c:191-233) + mm_idx_cal_max_occ (index.c:164-185) yield for a list of
// sequences, laid out as mm2c_minidx keeps it (keys ascending | cr_off | n, one pool slot per hit).  DESIGN.md section 3.10 gives the exactness argument; in short:
//
//   1. tag.  The sketch kernels (sketch.hip) give every sequence of a chunk its mm128_t list with rid 0.  ib_tag splits each into the key (x >> 8: the span
//      in the low 8 bits is dropped, as mm_idx_add's buckets and worker_post's keys drop it) and y = rid << 32 | pos << 1 | strand, appended to the list.
//   2. order.  The index is the list sorted by (key, y): worker_post sorts a bucket by x and each key's p[] by radix_sort_64.  Two stable radix sorts
//      (rocPRIM): on y, then on the 2k key bits.  ib_heads checks the resulting order pair by pair, so a sort that was not stable is an error, not an index.
//   3. group.  Run heads over the sorted keys, their exclusive scan (the key's row), then per head the key and cr_off = the head's position (which IS the
//      exclusive scan of the counts), and n = the distance to the next head.  The sorted y column is the pool.
//   4. mid_occ.  The counts sorted (rocPRIM), the (uint32_t)((1. - f) * n_keys)-th read back: ks_ksmall's answer, any exact selection gives it.
#include "api_internal.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int TPB = 256;

inline unsigned blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// (key, y) of every minimizer of a chunk; rid = rid0 + the sequence whose range of mini_off holds it (the largest r with mini_off[r] <= m: sequences
// without minimizers share their offset with the next one)
__global__ void __launch_bounds__(TPB) ib_tag(const mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_seqs, int64_t n_mini, uint64_t rid0,
                                              uint64_t *key, uint64_t *y)
{
	const int64_t m = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (m >= n_mini) return;
	int64_t lo = 0, hi = n_seqs;
	while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (mini_off[mid] <= m) lo = mid; else hi = mid; }
	const mm2c_anchor_t p = mini[m];
	key[m] = p.x >> 8;
	y[m] = (rid0 + (uint64_t)lo) << 32 | (uint64_t)(uint32_t)p.y;
}

// head[i] = 1 where a key's run starts (n + 1 entries, the last one 0, so that the exclusive scan's last entry is the number of keys);
// *bad |= 1 where the pairs are not in (key, y) order
__global__ void __launch_bounds__(TPB) ib_heads(const uint64_t *key, const uint64_t *y, int64_t n, int64_t *head, int *bad)
{
	const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (i > n) return;
	if (i == n) { head[i] = 0; return; }
	int h = 1;
	if (i > 0) {
		const uint64_t k0 = key[i - 1], k1 = key[i];
		h = k0 != k1;
		if (k0 > k1 || (k0 == k1 && y[i - 1] > y[i])) *bad = 1;
	}
	head[i] = h;
}

// the key and cr_off of every row: written by the run's head
__global__ void __launch_bounds__(TPB) ib_rows(const uint64_t *key, const int64_t *head, const int64_t *row, int64_t n, uint64_t *keys_out, int64_t *cr_out)
{
	const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (i >= n || !head[i]) return;
	const int64_t j = row[i];
	keys_out[j] = key[i]; cr_out[j] = i;
}

// n of every row: up to the next row's first hit (the last row: up to the end of the pool); *bad |= 2 for a count that does not fit 32 bits
__global__ void __launch_bounds__(TPB) ib_counts(const int64_t *cr, int64_t n_keys, int64_t n, uint32_t *n_out, int *bad)
{
	const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
	if (j >= n_keys) return;
	const int64_t c = (j + 1 < n_keys ? cr[j + 1] : n) - cr[j];
	if (c > (int64_t)UINT32_MAX) *bad = 2;
	n_out[j] = (uint32_t)c;
}

} // namespace

namespace mm2c_api {

int index_tag(const mm2c_anchor_t *mini, const int64_t *mini_off, int64_t n_seqs, int64_t n_mini, int64_t rid0, uint64_t *key, uint64_t *y, hipStream_t st)
{
	if (n_mini <= 0) return 0;
	ib_tag<<<blocks(n_mini), TPB, 0, st>>>(mini, mini_off, n_seqs, n_mini, (uint64_t)rid0, key, y);
	HIP_TRY(hipGetLastError());
	return 0;
}

// workspace of index_sort / index_heads for n pairs
size_t index_tmp_bytes(int64_t n, int key_bits, int y_bits)
{
	size_t b1 = 0, b2 = 0, b3 = 0;
	(void)rocprim::radix_sort_pairs(nullptr, b1, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, y_bits);
	(void)rocprim::radix_sort_pairs(nullptr, b2, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, key_bits);
	(void)rocprim::exclusive_scan(nullptr, b3, (int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>());
	return std::max(b1, std::max(b2, b3));
}

// n > 0 pairs (key, y) -> sorted by y into (key_tmp, y_tmp), then stably by the key's low key_bits bits: keys back into `key`, the y column into `pool`
int index_sort(uint64_t *key, const uint64_t *y, uint64_t *key_tmp, uint64_t *y_tmp, uint64_t *pool, int64_t n, int key_bits, int y_bits, void *tmp, size_t tmp_bytes,
               hipStream_t st)
{
	size_t b = tmp_bytes;
	HIP_TRY(rocprim::radix_sort_pairs(tmp, b, y, y_tmp, (const uint64_t *)key, key_tmp, (size_t)n, 0, y_bits, st));
	b = tmp_bytes;
	HIP_TRY(rocprim::radix_sort_pairs(tmp, b, (const uint64_t *)key_tmp, key, (const uint64_t *)y_tmp, pool, (size_t)n, 0, key_bits, st));
	return 0;
}

// run heads of the sorted keys and their exclusive scan: head / row hold n + 1 entries, row[n] = the number of keys.  *bad (zeroed here) as ib_heads sets it
int index_heads(const uint64_t *key, const uint64_t *y, int64_t n, int64_t *head, int64_t *row, int *bad, void *tmp, size_t tmp_bytes, hipStream_t st)
{
	HIP_TRY(hipMemsetAsync(bad, 0, 4, st));
	ib_heads<<<blocks(n + 1), TPB, 0, st>>>(key, y, n, head, bad);
	HIP_TRY(hipGetLastError());
	size_t b = tmp_bytes;
	HIP_TRY(rocprim::exclusive_scan(tmp, b, head, row, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), st));
	return 0;
}

// the image [keys | cr_off | n] of n_keys > 0 rows from the sorted keys of n pairs
int index_rows(const uint64_t *key, const int64_t *head, const int64_t *row, int64_t n, int64_t n_keys, char *img, int *bad, hipStream_t st)
{
	uint64_t *keys_out = (uint64_t *)img;
	int64_t *cr_out = (int64_t *)(img + (size_t)n_keys * 8);
	uint32_t *n_out = (uint32_t *)(img + (size_t)n_keys * 16);
	ib_rows<<<blocks(n), TPB, 0, st>>>(key, head, row, n, keys_out, cr_out);
	HIP_TRY(hipGetLastError());
	ib_counts<<<blocks(n_keys), TPB, 0, st>>>(cr_out, n_keys, n, n_out, bad);
	HIP_TRY(hipGetLastError());
	return 0;
}

// the i-th smallest (from 0) of n_keys > i counts, by sorting a copy of them
int index_count_select(const uint32_t *d_n, int64_t n_keys, int64_t i, uint32_t *h_val, hipStream_t st)
{
	size_t sort_bytes = 0;
	HIP_TRY(rocprim::radix_sort_keys(nullptr, sort_bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)n_keys));
	Layout L;
	const size_t o_s = L.take((size_t)n_keys * 4), o_tmp = L.take(sort_bytes);
	char *d = nullptr;
	HIP_TRY(dev_alloc((void **)&d, L.at));
	auto body = [&]() -> int {
		size_t b = sort_bytes;
		HIP_TRY(rocprim::radix_sort_keys(d + o_tmp, b, d_n, (uint32_t *)(d + o_s), (size_t)n_keys, 0, 32, st));
		HIP_TRY(hipMemcpyAsync(h_val, d + o_s + (size_t)i * 4, 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		return 0;
	};
	const int rc = body();
	dev_free(d);
	return rc;
}

} // namespace mm2c_api
