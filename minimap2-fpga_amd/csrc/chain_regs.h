// chain_regs.h -- argument block and launcher of the chains-to-regions step (mm_gen_regs, hit.c:8-88), chain_regs.hip.
#ifndef MM2C_CHAIN_REGS_H
#define MM2C_CHAIN_REGS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mm2c {

constexpr int REG_WORDS = 10;          // a region (mm_reg1_t, minimap.h:85-100) is 80 bytes: ten 64-bit words

// ---- the region record, described once.  Kernels that take a record field by field read it through Reg; the word-wise kernels load 64-bit words and take
// the fields out of them with the accessors below.
struct Reg {                           // mm2c_reg_t
	int32_t id, cnt, rid, score, qs, qe, rs, re, parent, subsc, as, mlen, blen, n_sub, score0;
	uint32_t flags, hash; float div; uint64_t p;
};
// a field's index among the record's 32-bit words: 64-bit word F / 2, the high half when F is odd
enum RegField { REG_ID, REG_CNT, REG_RID, REG_SCORE, REG_QS, REG_QE, REG_RS, REG_RE, REG_PARENT, REG_SUBSC, REG_AS, REG_MLEN, REG_BLEN, REG_N_SUB, REG_SCORE0,
                REG_FLAGS, REG_HASH, REG_DIV };
static_assert(sizeof(Reg) == 8 * REG_WORDS && offsetof(Reg, cnt) == 4 * REG_CNT && offsetof(Reg, as) == 4 * REG_AS && offsetof(Reg, mlen) == 4 * REG_MLEN &&
              offsetof(Reg, blen) == 4 * REG_BLEN && offsetof(Reg, flags) == 4 * REG_FLAGS && offsetof(Reg, hash) == 4 * REG_HASH && REG_BLEN == REG_MLEN + 1,
              "Reg is mm2c_reg_t");
// the bit-field word `flags` (minimap.h:96): mapq:8, split:2, rev:1, inv:1, sam_pri:1, proper_frag:1, pe_thru:1, seg_split:1, seg_id:8, split_inv:1
constexpr int REG_REV_BIT = 10, REG_SEG_ID_SHIFT = 16, REG_SPLIT_INV_BIT = 24;
constexpr uint32_t REG_SAM_PRI = 1u << 12, REG_SEG_SPLIT = 1u << 15;

constexpr int reg_word(RegField f) { return f >> 1; }
// field F out of its loaded word; out of the record's words w[] (a loaded copy, or the record in memory)
template <RegField F> __host__ __device__ __forceinline__ int32_t reg_of(uint64_t word) { return (int32_t)(F & 1 ? word >> 32 : word); }
template <RegField F> __host__ __device__ __forceinline__ int32_t reg_get(const uint64_t *w) { return reg_of<F>(w[F >> 1]); }
__host__ __device__ __forceinline__ int32_t reg_rev(const uint64_t *w) { return (int32_t)((uint32_t)reg_get<REG_FLAGS>(w) >> REG_REV_BIT & 1u); }
// v as field F of its word, the other half 0; and word w with field F replaced by v
template <RegField F> __host__ __device__ __forceinline__ uint64_t reg_put(uint32_t v) { return F & 1 ? (uint64_t)v << 32 : (uint64_t)v; }
template <RegField F> __host__ __device__ __forceinline__ uint64_t reg_with(uint64_t w, uint32_t v) { return (w & (F & 1 ? 0xffffffffull : 0xffffffff00000000ull)) | reg_put<F>(v); }

constexpr int REGS_TS_MAX = 4096;      // regs_sort: reads of up to this many chains replay klib's sort with the arrangement in LDS, longer ones through memory
constexpr int REGS_FILL_ROWS = 16;     // regs_fill: a wave takes a slice of this many rows of 64 chain anchors ...
constexpr int REGS_FILL_WAVES = 4;     // ... and a workgroup this many slices

struct RegArgs {
	int64_t n_reads, n_u_cap, n_b_cap;
	// the device epilogue's compact output: chains of read r are u[u_off[r] .. u_off[r+1]), their anchors b[b_off[r] .. b_off[r+1])
	const int64_t *u_off, *b_off;      // n_reads + 1 each
	const uint64_t *u;
	const ulonglong2 *b;
	const int32_t *qlen;               // per read
	const uint32_t *hash;              // per read (map.c:290-292)
	uint64_t *regs;                    // out: REG_WORDS words per chain, indexed like u
	// scratch, n_u_cap entries each
	uint64_t *zkey, *key0, *key1;      // the sort keys z.x in chain order (never overwritten) / the two buffers of the sorts
	int64_t *cstart, *cend;            // per chain: its anchors are b[cstart .. cend), clamped to the read's extent
	int32_t *val0, *val1, *crank, *tiecnt, *stack, *moved;   // crank: chain -> its region
	int32_t *flags;                    // [0]: reads whose counts or offsets disagree, [1]: reads that hold equal keys, [2]: reads refused for their offsets (regs_fill
	                                   // then goes read by read); four words, zero on entry
};
// ev_mid (optional) is recorded between the two kernels
hipError_t launch_chain_regs(const RegArgs &A, hipStream_t st, hipEvent_t ev_mid, int *n_launches);

} // namespace mm2c
#endif
