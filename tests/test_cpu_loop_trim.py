"""Two pieces of the tile kernel's hand-written loop (csrc/chain_dp_tile.h) restated in NumPy and held against what they replace: the log term of the computed gap
cost in two instructions (MM2C_SCORE_CMP: v_ffbh_u32, then bits 1-4 of the count), and the layout of the per-anchor word that the tile set-up packs (tw_l in
chain_dp_tile) and the loop takes apart (Lk, Lloop, Lpart of MM2C_SCAN_TILE_ASM).  No GPU."""
import numpy as np

FLAG_BITS = (28, 29, 30, 31)     # scan goes on from memory (set by the loop) / no window / window clamped to the ring / not for the loop


def ffbh_u32(v):
    """v_ffbh_u32: the number of leading zero bits of a 32-bit value, all ones (0xffffffff) when the value is 0"""
    v = np.asarray(v, np.uint64)
    n = np.zeros(v.shape, np.uint64)
    for k in range(32):                                   # position of the highest set bit, by comparison (no floating point)
        n = np.where(v >= (np.uint64(1) << np.uint64(k)), np.uint64(31 - k), n)
    return np.where(v == 0, np.uint64(0xffffffff), n)


def bfe_u32(v, offset, width):
    """v_bfe_u32 / s_bfe_u32: `width` bits of v from bit `offset` on, zero-extended"""
    return (np.asarray(v, np.uint64) >> np.uint64(offset)) & np.uint64((1 << width) - 1)


def log_term(dd):
    """the two instructions of MM2C_SCORE_CMP"""
    return bfe_u32(ffbh_u32(dd), 1, 4)


def log_term_ref(dd):
    """clz(dd | 1) >> 1, the three instructions they replace (and FBIAS - (ilog2(dd) >> 1) of chain.c:209 for dd >= 1)"""
    v = np.asarray(dd, np.uint64) | np.uint64(1)
    clz = np.array([32 - int(x).bit_length() for x in v.ravel()], np.uint64).reshape(v.shape)
    return clz >> np.uint64(1)


def test_log_term_small_values():
    dd = np.arange(0, (1 << 16) + 1, dtype=np.uint64)
    assert np.array_equal(log_term(dd), log_term_ref(dd))
    assert int(log_term(np.uint64(0))) == 15 == int(log_term(np.uint64(1)))       # the all-ones count of 0 reads as clz(1) >> 1


def test_log_term_around_powers_of_two():
    dd = sorted({v for k in range(1, 32) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v <= (1 << 31) - 1})
    assert dd[-1] == (1 << 31) - 1 and (1 << 30) + 1 in dd
    dd = np.array(dd, np.uint64)
    assert np.array_equal(log_term(dd), log_term_ref(dd))
    # ... and the relation to chain.c:209: 14 - (ilog2(dd) >> 1), one more where the count is odd (FBIAS takes the 14)
    lg = np.array([int(v).bit_length() - 1 for v in dd], np.int64)
    assert np.array_equal(log_term(dd).astype(np.int64), (31 - lg) >> 1)


# ---- the per-anchor word
def pack_tw(bef, own, first, flags=0):
    """tw_l of chain_dp_tile: bef | own << 10 | first << 16 | flags"""
    return np.uint64(bef) | (np.uint64(own) << np.uint64(10)) | (np.uint64(first) << np.uint64(16)) | np.uint64(flags)


def unpack_tw(pk):
    """what the loop reads: s_and_b32 n, pk, 0x3c0; s_and_b32 part, pk, 63; s_bfe_u32 t0, pk, 0x6000a; s_bfe_u32 t1, pk, 0x70010"""
    pk = np.uint64(pk)
    return int(pk & np.uint64(0x3c0)), int(pk & np.uint64(63)), int(bfe_u32(pk, 10, 6)), int(bfe_u32(pk, 16, 7))


BEFS = (0, 1, 63, 64, 65, 959, 960)


def test_tw_round_trip():
    for bef in BEFS:
        for own in range(64):
            for first in range(1, 65):
                n64, part, own2, first2 = unpack_tw(pack_tw(bef, own, first))
                assert (n64, part, own2, first2) == (64 * (bef // 64), bef % 64, own, first), (bef, own, first)
                assert n64 + part == bef


def test_tw_loop_counts_in_anchors():
    """the count-down of Lloop (s_sub_u32 n, n, 64 with its borrow) visits bef // 64 whole tiles at depths 64, 128, ... (d = nfull - n), then the partly covered one
    at nfull + 64; the word without its low six bits (s_andn2_b32 at Lpart) says that tile is done"""
    for bef in BEFS:
        pk = pack_tw(bef, 5, 7)
        n, _, _, _ = unpack_tw(pk)
        nfull, depths = n, []
        while True:
            borrow = n < 64
            n = (n - 64) & 0xffffffff
            if borrow:
                break
            depths.append(nfull - n)
        assert depths == [64 * (k + 1) for k in range(bef // 64)], (bef, depths)
        part = unpack_tw(pk)[1]
        assert (part != 0) == (bef % 64 != 0)
        if part:
            assert nfull + 64 == 64 * (bef // 64 + 1)
        done = np.uint64(pk) & ~np.uint64(63)
        assert unpack_tw(done)[1] == 0 and unpack_tw(done)[0] == nfull and unpack_tw(done)[2:] == (5, 7)


def test_tw_flags_do_not_collide():
    fields = int(pack_tw(1023, 63, 127))                  # every bit the three fields can set (first lane <= 64 needs 7 bits)
    assert fields == (1 << 23) - 1
    for b in FLAG_BITS:
        assert not fields & (1 << b)
        for bef in BEFS:
            w = pack_tw(bef, 63, 64, 1 << b)
            assert unpack_tw(w) == (64 * (bef // 64), bef % 64, 63, 64) and int(w) >> b & 1
    w = pack_tw(960, 63, 64, sum(1 << b for b in FLAG_BITS))
    assert unpack_tw(w) == (960, 0, 63, 64) and int(w) >> 28 == 0xf
    assert unpack_tw(np.uint64(int(w) & ~63)) == (960, 0, 63, 64)


# ---- the packed f / p word of the lean form: the stamp slot from the word as it is (MM2C_STSLOT_FS4)
def test_stamp_slot_from_the_packed_word():
    """max(word, (lo - 1) << 18) as signed words, then ten bits from bit 18 on == max(p, lo - 1) & 1023 for every p the word can hold next to any f field"""
    FB, SB = 18, 10
    p = np.concatenate((np.arange(-1, 8192), [-1, 0, 8191])).astype(np.int64)
    for fbits in (0, 1, (1 << FB) - 1, 1 << (FB - 1), 12345):
        word = ((p << FB) | fbits).astype(np.int32 if False else np.int64)
        word = ((word + (1 << 31)) % (1 << 32)) - (1 << 31)                      # as a signed 32-bit register
        for lom1 in (-961, -1, 0, 1, 63, 1023, 1024, 7231, 8190):
            thr = lom1 << FB
            assert -(1 << 31) <= thr < (1 << 31)
            got = (np.maximum(word, thr) % (1 << 32)) >> FB & ((1 << SB) - 1)
            assert np.array_equal(got, np.maximum(p, lom1) & ((1 << SB) - 1)), (fbits, lom1)
        own = ((p << FB) + (1 << 31)) % (1 << 32) - (1 << 31)                     # the own tile's p << 18 (MM2C_OWNP_FS4_LEANF): the same slot
        assert np.array_equal((np.maximum(own, 0 << FB) % (1 << 32)) >> FB & 1023, np.maximum(p, 0) & 1023)
