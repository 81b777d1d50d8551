// Dropout / stochastic depth outside the GEMM epilogues (mask layout and generator: philox.h):
//  * mi_drop_state_advance: the one-thread kernel that advances the step of the device state block
//    (the pattern of optim.hip's prep kernels: a captured graph advances it on every replay);
//  * mi_drop_bwd: dzm = bf16(float(dz) * m), the gradient a dropped residual branch hands to its
//    weight- and data-gradient GEMMs (one pass, 16-byte accesses);
//  * mi_drop_mask: the fp32 multiplier matrix of a site -- tests and debugging only.
#include "common.h"
#include "philox.h"

namespace {

// state: [seed, step] -> step + inc (0 or 1); snap (optional) <- the advanced [seed, step]: the block
// the kernels of one forward / backward pair read, untouched by later advances
__global__ void drop_advance_kernel(uint64_t* __restrict__ state, uint64_t* __restrict__ snap, int inc) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint64_t seed = state[0], step = state[1] + (uint64_t)inc;
  if (inc) state[1] = step;
  if (snap) {
    snap[0] = seed;
    snap[1] = step;
  }
}

// one thread per 16-byte chunk q of the [M][N] matrix (n8 = N / 8 chunks per row)
template <bool MASK>
__global__ __launch_bounds__(256) void drop_apply_kernel(DropArgs d, const bf16_t* __restrict__ x, void* __restrict__ out,
                                                        uint32_t chunks, FastDiv n8) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= chunks) return;
  const DropKey k = drop_key(d);
  float m[8];
  drop_chunk(d, k, fdiv(q, n8), q, m);
  if (MASK) {
    float4* o = (float4*)out + (size_t)q * 2;
    o[0] = make_float4(m[0], m[1], m[2], m[3]);
    o[1] = make_float4(m[4], m[5], m[6], m[7]);
  } else {
    float f[8];
    unpack8(ld_nt16(x, q), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= m[j];
    ((uint4*)out)[q] = pack8(f);
  }
}

}  // namespace

MI_API int mi_drop_state_advance(void* state, void* snap, int inc, hipStream_t st) {
  if (!state || (inc != 0 && inc != 1)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(64), 0, st, (uint64_t*)state, (uint64_t*)snap, inc);
  return (int)hipGetLastError();
}

// out[M][N] bf16 = bf16(float(dz[M][N]) * m), m = element mask x row mask (one fp32 product)
MI_API int mi_drop_bwd(const void* dz, void* out, int M, int N, const void* state, int thr_e, int site_e, int thr_r,
                       int site_r, int rank, int rows_per_sample, hipStream_t st) {
  DropArgs d{};
  if (M <= 0 || N <= 0 || !dz || !out || !drop_args(d, state, thr_e, site_e, thr_r, site_r, rank, rows_per_sample, M, N))
    return (int)hipErrorInvalidValue;
  const uint32_t chunks = (uint32_t)((int64_t)M * N / 8);
  hipLaunchKernelGGL(drop_apply_kernel<false>, dim3(cdiv(chunks, 256)), dim3(256), 0, st, d, (const bf16_t*)dz, out,
                     chunks, make_fastdiv((uint32_t)(N / 8)));
  return (int)hipGetLastError();
}

// out[M][N] fp32 = the multiplier matrix (tests / debugging; never launched in a training step)
MI_API int mi_drop_mask(float* out, int M, int N, const void* state, int thr_e, int site_e, int thr_r, int site_r,
                        int rank, int rows_per_sample, hipStream_t st) {
  DropArgs d{};
  if (M <= 0 || N <= 0 || !out || !drop_args(d, state, thr_e, site_e, thr_r, site_r, rank, rows_per_sample, M, N))
    return (int)hipErrorInvalidValue;
  const uint32_t chunks = (uint32_t)((int64_t)M * N / 8);
  hipLaunchKernelGGL(drop_apply_kernel<true>, dim3(cdiv(chunks, 256)), dim3(256), 0, st, d, (const bf16_t*)nullptr,
                     (void*)out, chunks, make_fastdiv((uint32_t)(N / 8)));
  return (int)hipGetLastError();
}
