"""Shared by test_vit_drop_cpu.py and test_vit_drop_gpu.py: a numpy Philox4x32-10 and the mask layout
of the dropout / stochastic-depth sites, written from the layout's specification and not from the
kernels.

Layout: key = (seed lo, seed hi); counter = (q, site + (rank << 16), step lo, step hi).
Element masks on an [M][N] matrix (N % 8 == 0): q = (row * N + col) / 8, element j of the 16-byte
chunk draws r = (w[j >> 1] >> (16 * (j & 1))) & 0xffff.  Row masks: q = row / rows_per_sample,
r = w[0] & 0xffff.  Keep iff r >= thr = round(p * 65536); multiplier 65536 / (65536 - thr) in fp32
when kept, 0 when dropped.  Sites: 8 * layer + kind."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

KIND_ATTN_DROP, KIND_GELU_DROP, KIND_MLP_DROP, KIND_ATTN_PATH, KIND_MLP_PATH = range(5)


def site(layer, kind):
    return 8 * layer + kind


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (or ints) holding 32-bit words, key: two ints -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK32) for x in ctr]
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    assert 0.0 <= p < 1.0
    return int(np.floor(p * 65536.0 + 0.5))


def _mult(r, thr):
    scale = np.float32(65536.0) / np.float32(65536 - thr)
    return np.where(r >= thr, scale, np.float32(0.0)).astype(np.float32)


def _ctr(q, st, rank, seed, step):
    q = np.asarray(q, dtype=np.uint64)
    one = np.ones_like(q)
    ctr = (q, one * np.uint64(st + (rank << 16)), one * np.uint64(step & MASK32), one * np.uint64((step >> 32) & MASK32))
    return philox4x32_10(ctr, (seed & MASK32, (seed >> 32) & MASK32))


def element_mask(M, N, p, seed, rank, step, st):
    """fp32 [M][N] multipliers of an element (dropout) site"""
    assert N % 8 == 0 and M * N // 8 < 2 ** 32
    thr = threshold(p)
    if thr == 0:
        return np.ones((M, N), np.float32)
    w = _ctr(np.arange(M * N // 8), st, rank, seed, step)
    r = np.empty((M * N // 8, 8), np.uint32)
    for j in range(8):
        r[:, j] = (w[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
    return _mult(r, thr).reshape(M, N)


def sample_mask(B, p, seed, rank, step, st):
    """fp32 [B] multipliers of a row (stochastic depth) site"""
    thr = threshold(p)
    if thr == 0:
        return np.ones(B, np.float32)
    w = _ctr(np.arange(B), st, rank, seed, step)
    return _mult(w[0] & np.uint32(0xFFFF), thr)


def row_mask(M, N, rows_per_sample, p, seed, rank, step, st):
    """the sample mask spread over the [M][N] matrix (row -> sample row / rows_per_sample)"""
    B = (M + rows_per_sample - 1) // rows_per_sample
    m = sample_mask(B, p, seed, rank, step, st)
    return np.repeat(np.repeat(m, rows_per_sample)[:M, None], N, axis=1)


def combined_mask(M, N, p_e, st_e, p_r, st_r, rows_per_sample, seed, rank, step):
    """element mask x row mask as one fp32 product (what the kernels multiply by)"""
    return (element_mask(M, N, p_e, seed, rank, step, st_e) *
            row_mask(M, N, rows_per_sample, p_r, seed, rank, step, st_r)).astype(np.float32)
