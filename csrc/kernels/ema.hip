// Weight averaging on the flat buffer (FlatEMA, parallel/ema.py) for gfx950 (MI355X).
//
// Three kernels:
//   prep     one thread: call counter, update counter, this call's weight -> per-call scalars
//   update   ema[i] = fmaf(w, p[i] - ema[i], ema[i])      (12 B per element, nothing to reduce)
//   swap     a[i] <-> b[i] as 32-bit patterns             (evaluation with the averaged weights)
// Everything that changes from call to call lives in a small device-resident state block that the
// prep kernel advances, so a captured step replays with the right weight: the host passes only
// constants (warmup, every) by value.
//
// State block (doubles):
//   [0] calls c   [1] updates n   [2] w of this call (0 = this call skips)   [3] decay
//   [4] d_t of the last call that updated
//
// prep, all in fp64:
//   c += 1
//   if c % every != 0:            w = 0                      (n and d_t unchanged)
//   else: d_t = decay                                  if warmup <= 0 (no warm-up)
//             = min(decay, (1 + n) / (warmup + n))     otherwise
//         w = 1 - d_t ;  n += 1
//
// update and swap take pointers with 4-byte alignment only (the BatchNorm buffer block has
// arbitrary length and offset).  When both pointers sit at the same offset mod 16 a launch runs
// a scalar head up to the first 16-byte boundary, a 16-byte body and a scalar tail; when they
// differ, every element goes one by one.  Each element sees the same fmaf on either path, so the
// result does not depend on the alignment or on how a range is cut into launches.
#include "common.h"

namespace {
constexpr int NT = 256;

// Cache policy of the 16-byte body (both kernels): non-temporal.  Every operand is read once per
// call and the step's next kernels read the bf16 compute copy, not these fp32 buffers.  Measured
// with tools/bench_optim.py --suite ema (profiles/ema_flat.md): with the caches cold, as between
// two training steps, non-temporal is faster than plain accesses at the ViT-B/16 and, by more, at
// the ResNet-50 size; only back-to-back calls on buffers that fit the last-level cache favour plain.
// MI_EMA_NT=0 exists for that A/B build alone.
#ifndef MI_EMA_NT
#define MI_EMA_NT 1
#endif
constexpr bool kEmaNt = MI_EMA_NT != 0;

// same launch cap as the other elementwise kernels: 8192 blocks, grid-stride beyond
inline int ew_grid(int64_t n) {
  int64_t g = (n + NT - 1) / NT;
  return (int)(g < 1 ? 1 : (g < 8192 ? g : 8192));
}

__device__ __forceinline__ u32x4 ld16(const u32x4* q) {
  if (kEmaNt) return __builtin_nontemporal_load(q);
  return *q;
}

__device__ __forceinline__ void st16(u32x4* q, const u32x4& v) {
  if (kEmaNt)
    __builtin_nontemporal_store(v, q);
  else
    *q = v;
}

__device__ __forceinline__ float ema_one(float e, float p, float w) { return __builtin_fmaf(w, p - e, e); }

__device__ __forceinline__ u32x4 ema_four(const u32x4& eb, const u32x4& pb, float w) {
  f32x4 e = __builtin_bit_cast(f32x4, eb);
  const f32x4 q = __builtin_bit_cast(f32x4, pb);
  e.x = ema_one(e.x, q.x, w);
  e.y = ema_one(e.y, q.y, w);
  e.z = ema_one(e.z, q.z, w);
  e.w = ema_one(e.w, q.w, w);
  return __builtin_bit_cast(u32x4, e);
}

// elements before the first 16-byte boundary of x (x is 4-byte aligned), at most n
__device__ __forceinline__ int64_t head_of(const void* x, int64_t n) {
  const int64_t h = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) >> 2);
  return h < n ? h : n;
}

// ------------------------------------------------------------------------------------ prep
__global__ void ema_prep_kernel(double* __restrict__ st, double warmup, int64_t every) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double c = st[0] + 1.0;
  st[0] = c;
  if ((int64_t)c % every != 0) {
    st[2] = 0.0;
    return;
  }
  const double n = st[1], decay = st[3];
  double d = decay;
  if (warmup > 0.0) {
    const double r = (1.0 + n) / (warmup + n);
    d = r < decay ? r : decay;
  }
  st[1] = n + 1.0;
  st[2] = 1.0 - d;
  st[4] = d;
}

// ---------------------------------------------------------------------------------- update
// VEC: ema and p sit at the same offset mod 16.  w == 0 (a skipped call): every thread returns
// before touching memory -- the branch is uniform over the grid.
template <bool VEC>
__global__ __launch_bounds__(NT) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p,
                                                        int64_t n, const double* __restrict__ st) {
  const double wd = st[2];
  if (wd == 0.0) return;
  const float w = (float)wd;
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  if (!VEC) {
    for (int64_t i = tid; i < n; i += nthr) ema[i] = ema_one(ema[i], p[i], w);
    return;
  }
  const int64_t head = head_of(ema, n);
  const int64_t nvec = (n - head) >> 2;
  u32x4* ev = (u32x4*)(ema + head);
  const u32x4* pv = (const u32x4*)(p + head);
  for (int64_t v = tid; v < nvec; v += nthr) st16(ev + v, ema_four(ld16(ev + v), ld16(pv + v), w));
  // head [0, head) and tail [head + 4 nvec, n): fewer than 4 + 4 elements
  const int64_t tail0 = head + (nvec << 2);
  if (tid < head) ema[tid] = ema_one(ema[tid], p[tid], w);
  if (tid < n - tail0) ema[tail0 + tid] = ema_one(ema[tail0 + tid], p[tail0 + tid], w);
}

// ------------------------------------------------------------------------------------ swap
// 32-bit moves: NaN payloads, signed zeros and denormals pass through unchanged, so the exchange
// is its own inverse bit for bit.
template <bool VEC>
__global__ __launch_bounds__(NT) void ema_swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, int64_t n) {
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  if (!VEC) {
    for (int64_t i = tid; i < n; i += nthr) {
      const uint32_t x = a[i], y = b[i];
      a[i] = y;
      b[i] = x;
    }
    return;
  }
  const int64_t head = head_of(a, n);
  const int64_t nvec = (n - head) >> 2;
  u32x4* av = (u32x4*)(a + head);
  u32x4* bv = (u32x4*)(b + head);
  for (int64_t v = tid; v < nvec; v += nthr) {
    const u32x4 x = ld16(av + v), y = ld16(bv + v);
    st16(av + v, y);
    st16(bv + v, x);
  }
  const int64_t tail0 = head + (nvec << 2);
  if (tid < head) {
    const uint32_t x = a[tid], y = b[tid];
    a[tid] = y;
    b[tid] = x;
  }
  if (tid < n - tail0) {
    const uint32_t x = a[tail0 + tid], y = b[tail0 + tid];
    a[tail0 + tid] = y;
    b[tail0 + tid] = x;
  }
}

// both pointers at the same offset mod 16 (and 4-byte aligned): head / 16-byte body / tail
inline bool same_phase(const void* a, const void* b) {
  return (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0 && ((uintptr_t)a & 3) == 0;
}

inline bool aligned4(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 3) == 0; }

// one thread per 16-byte access (the first block's threads also take the < 8 head and tail
// elements) or one thread per element.  Four accesses per array in flight per thread (a quarter
// of the grid) measured slower at the ViT-B/16 and ResNet-50 sizes (profiles/ema_flat.md).
inline int body_grid(int64_t n, bool vec) { return ew_grid(vec ? (n + 3) / 4 : n); }

#define LAUNCH_EMA(kernel, vec, blocks, st, ...)                                           \
  do {                                                                                     \
    if (vec)                                                                               \
      hipLaunchKernelGGL(kernel<true>, dim3(blocks), dim3(NT), 0, st, __VA_ARGS__);        \
    else                                                                                   \
      hipLaunchKernelGGL(kernel<false>, dim3(blocks), dim3(NT), 0, st, __VA_ARGS__);       \
  } while (0)

}  // namespace

// 1 when the 16-byte body uses non-temporal accesses (the policy this library was built with)
MI_API int mi_ema_nontemporal() { return kEmaNt ? 1 : 0; }

// state: 5 doubles (layout at the top of this file); warmup <= 0: no warm-up; every >= 1
MI_API int mi_ema_prep(double* state, double warmup, int64_t every, hipStream_t st) {
  if (!state || every < 1) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ema_prep_kernel, dim3(1), dim3(64), 0, st, state, warmup, every);
  return (int)hipGetLastError();
}

// ema[i] = fmaf(w, p[i] - ema[i], ema[i]) over n elements with w = state[2]; 4-byte aligned pointers
MI_API int mi_ema_update(float* ema, const float* p, int64_t n, const double* state, hipStream_t st) {
  if (n < 0 || !state) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!ema || !p || !aligned4(ema, p)) return (int)hipErrorInvalidValue;
  const bool vec = same_phase(ema, p);
  LAUNCH_EMA(ema_update_kernel, vec, body_grid(n, vec), st, ema, p, n, state);
  return (int)hipGetLastError();
}

// a[i] <-> b[i] over n 32-bit elements; the ranges must not overlap; 4-byte aligned pointers
MI_API int mi_ema_swap(void* a, void* b, int64_t n, hipStream_t st) {
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!a || !b || !aligned4(a, b)) return (int)hipErrorInvalidValue;
  const bool vec = same_phase(a, b);
  LAUNCH_EMA(ema_swap_kernel, vec, body_grid(n, vec), st, (uint32_t*)a, (uint32_t*)b, n);
  return (int)hipGetLastError();
}
