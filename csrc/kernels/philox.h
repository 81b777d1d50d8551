// Counter-based dropout / stochastic-depth masks: Philox4x32-10 (Random123 constants) and the mask
// layout shared by every kernel that drops (GEMM epilogues, drop.hip).  Plain C++: the same
// functions compile for the host.
//
// A mask is a pure function of (seed, rank, step, site, position):
//   key     = (seed lo, seed hi)
//   counter = (q, site + (rank << 16), step lo, step hi)          site, rank < 65536
//   element masks on an [M][N] bf16 matrix, N % 8 == 0: q = (row * N + col) / 8 -- one call per
//     16-byte chunk; element j of the chunk draws r = (w[j >> 1] >> (16 * (j & 1))) & 0xffff
//   row masks (stochastic depth): q = sample index row / rows_per_sample, r = w[0] & 0xffff
//   keep iff r >= thr, thr = round(p * 65536); multiplier 65536 / (65536 - thr) in fp32 when kept,
//   0 when dropped.  thr == 0: the site is inactive, no Philox work.
// seed and step live in a device state block (two 64-bit words) that kernels read through a
// pointer, so a captured graph draws new masks on every replay; the rest goes by value.
#pragma once
#include "common.h"
#include "epilogue.h"

#define MI_HD __host__ __device__ __forceinline__

MI_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

MI_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = philox_mulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
    const uint32_t h1 = philox_mulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = h1 ^ c[1] ^ k0, n2 = h0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = l1; c[2] = n2; c[3] = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// One dropped tensor: an element mask, a row (per-sample) mask, or both.  thr_* == 0: inactive.
struct DropArgs {
  const uint64_t* state;   // device: [seed, step]
  uint32_t thr_e, site_e;  // element mask (dropout)
  uint32_t thr_r, site_r;  // row mask (stochastic depth)
  uint32_t rank;
  float scale_e, scale_r;  // 65536 / (65536 - thr)
  FastDiv rps;             // rows per sample
};

static inline float drop_scale(uint32_t thr) { return 65536.f / (float)(65536u - thr); }

// seed / step of this launch, read once per thread
struct DropKey {
  uint32_t k0, k1, s0, s1;
};
__device__ __forceinline__ DropKey drop_key(const DropArgs& d) {
  const uint64_t seed = d.state[0], step = d.state[1];
  return DropKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
}

// multiplier of row `row`'s sample (thr_r != 0)
__device__ __forceinline__ float drop_row_mult(const DropArgs& d, const DropKey& k, uint32_t row) {
  uint32_t c[4] = {fdiv(row, d.rps), d.site_r + (d.rank << 16), k.s0, k.s1};
  philox4x32_10(c, k.k0, k.k1);
  return (c[0] & 0xffffu) >= d.thr_r ? d.scale_r : 0.f;
}

// multipliers m[0..7] of the 16-byte chunk q = (row * N + col) / 8: element mask x row mask, one
// fp32 product; returns the keep bits (bit j: element j is kept)
__device__ __forceinline__ uint32_t drop_chunk(const DropArgs& d, const DropKey& k, uint32_t row, uint32_t q,
                                               float (&m)[8]) {
  const float mr = d.thr_r ? drop_row_mult(d, k, row) : 1.f;
  uint32_t keep = mr != 0.f ? 0xffu : 0u;
  if (d.thr_e) {
    uint32_t c[4] = {q, d.site_e + (d.rank << 16), k.s0, k.s1};
    philox4x32_10(c, k.k0, k.k1);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool kp = ((c[j >> 1] >> (16 * (j & 1))) & 0xffffu) >= d.thr_e;
      m[j] = (kp ? d.scale_e : 0.f) * mr;
      if (!kp) keep &= ~(1u << j);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = mr;
  }
  return keep;
}

// host: fill the by-value part; false when an argument is outside the layout
static inline bool drop_args(DropArgs& d, const void* state, int thr_e, int site_e, int thr_r, int site_r, int rank,
                             int rows_per_sample, int64_t M, int64_t N) {
  if (!state || thr_e < 0 || thr_e >= 65536 || thr_r < 0 || thr_r >= 65536 || site_e < 0 || site_e >= 65536 ||
      site_r < 0 || site_r >= 65536 || rank < 0 || rank >= 65536 || (thr_r && rows_per_sample <= 0) || N % 8 != 0 ||
      M * N / 8 >= (1ll << 32))
    return false;
  d.state = (const uint64_t*)state;
  d.thr_e = (uint32_t)thr_e; d.site_e = (uint32_t)site_e;
  d.thr_r = (uint32_t)thr_r; d.site_r = (uint32_t)site_r;
  d.rank = (uint32_t)rank;
  d.scale_e = drop_scale(d.thr_e); d.scale_r = drop_scale(d.thr_r);
  d.rps = make_fastdiv((uint32_t)(thr_r ? rows_per_sample : 1));
  return true;
}

// ---- GEMM epilogue ops on one 16-byte chunk (v = the bf16-staged acc + bias, as epi 1 / 3 see it)
// residual-drop: C <- v * m + aux; a dropped element is aux bit for bit
__device__ __forceinline__ uint4 drop_residual_v(uint4 v, uint4 aux_v, const float (&m)[8], uint32_t keep) {
  float f[8], g[8];
  unpack8(v, f);
  unpack8(aux_v, g);
#pragma unroll
  for (int q = 0; q < 8; ++q) f[q] = ((keep >> q) & 1u) ? f[q] * m[q] + g[q] : g[q];
  return pack8(f);
}

// GELU-drop: C <- gelu(u) * m, aux <- gelu'(u) * m (epi 1 with the mask in both outputs, so the
// backward's epi 2 GEMM needs no change); a dropped element is +0 in both
__device__ __forceinline__ uint4 drop_gelu_v(uint4 v, bf16_t* aux, const float (&m)[8], uint32_t keep) {
  float f[8], d[8];
  unpack8(v, f);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const bool kp = (keep >> q) & 1u;
    const float y = gelu_fg(f[q], d[q]);
    f[q] = kp ? y * m[q] : 0.f;
    d[q] = kp ? d[q] * m[q] : 0.f;
  }
  *(uint4*)aux = pack8(d);
  return pack8(f);
}
