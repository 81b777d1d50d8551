// Flat AdamW with on-device global-norm gradient clipping, and the layer-wise optimizers LARS and
// LAMB (second half of this file), for gfx950 (MI355X).
//
// Three kernels drive one optimizer step over the flat fp32 master buffer (parallel/optim.py):
//   sqnorm   sum of squares of the gradient segments, fp64, deterministic (fixed slots, no atomics)
//   prep     one thread: step counter, bias corrections, clip coefficient -> per-step scalars
//   update   torch.optim.AdamW (no amsgrad / maximize) + 1/world + clip + bf16 compute-copy refresh
// Everything that changes from step to step (t, lr, the bias corrections, the clip coefficient)
// lives in a small device-resident state block, so a captured step replays correctly: the host
// passes only constants (betas, eps, weight decay, max_norm, grad_scale) by value.
//
// State block (doubles):
//   [0] step t          [1] lr               [2] total_norm        [3] clip coefficient
//   [4] lr / bc1        [5] 1 / sqrt(bc2)    [6] grad_scale * coef [7] lr * wd
#include "common.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
constexpr int SQ_MAX_BLOCKS = 1024;

// same launch cap as the other elementwise kernels: 8192 blocks, grid-stride beyond
inline int ew_grid(int64_t n) {
  int64_t g = (n + NT - 1) / NT;
  return (int)(g < 1 ? 1 : (g < 8192 ? g : 8192));
}

// Sum of s over the block, valid in thread 0: a xor tree over the 64 lanes of every wave, then
// thread 0 adds the wave partials in index order.
template <int N>
__device__ __forceinline__ double block_sum(double s) {
  __shared__ double red[N / 64];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = red[0];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < N / 64; ++w) t += red[w];
  }
  return t;
}

// VEC: 16-byte accesses (bf16: 8-byte); otherwise the same four elements one by one
template <bool VEC>
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int64_t i) {
  if (VEC) return ((const float4*)p)[i];
  const float* q = p + (i << 2);
  return make_float4(q[0], q[1], q[2], q[3]);
}

template <bool VEC>
__device__ __forceinline__ void st4(float* __restrict__ p, int64_t i, const float4& v) {
  if (VEC) {
    ((float4*)p)[i] = v;
  } else {
    float* q = p + (i << 2);
    q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
  }
}

template <bool VEC>
__device__ __forceinline__ void st4bf(bf16_t* __restrict__ p16, int64_t i, const float4& v) {
  if (VEC) {
    uint2 o;
    o.x = pack2bf(v.x, v.y);
    o.y = pack2bf(v.z, v.w);
    ((uint2*)p16)[i] = o;
  } else {
    bf16_t* q = p16 + (i << 2);
    q[0] = f2bf(v.x), q[1] = f2bf(v.y), q[2] = f2bf(v.z), q[3] = f2bf(v.w);
  }
}

// -------------------------------------------------------------------- squared gradient norm
// Block b writes its fp64 partial to part[b]; sqnorm_final_kernel sums all slots of all segments
// in a fixed order.  16-byte loads over the aligned body, scalar loads for an unaligned head
// (x only 4-byte aligned) and the tail.
__global__ __launch_bounds__(NT) void sqnorm_partial_kernel(const float* __restrict__ x, int64_t n,
                                                            double* __restrict__ part) {
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  int64_t head = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) >> 2);
  if (head > n) head = n;
  const int64_t nvec = (n - head) >> 2;
  const float4* xv = (const float4*)(x + head);
  double s = 0.0;
  for (int64_t v = tid; v < nvec; v += nthr) {
    const float4 a = xv[v];
    s += (double)a.x * (double)a.x;
    s += (double)a.y * (double)a.y;
    s += (double)a.z * (double)a.z;
    s += (double)a.w * (double)a.w;
  }
  // head [0, head) and tail [head + 4 nvec, n): fewer than 4 + 4 elements
  const int64_t tail0 = head + (nvec << 2);
  if (tid < head) s += (double)x[tid] * (double)x[tid];
  if (tid < n - tail0) s += (double)x[tail0 + tid] * (double)x[tail0 + tid];
  s = block_sum<NT>(s);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(NT) void sqnorm_final_kernel(const double* __restrict__ part, int nparts,
                                                          double* __restrict__ out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
  s = block_sum<NT>(s);
  if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------ prep
// clip_grad_norm_ semantics: coef = min(1, max_norm / (total_norm + 1e-6)), a NaN norm gives a NaN
// coefficient (torch clamps with max=1, which keeps NaN), an infinite norm gives 0.  Both state
// blocks keep total_norm in [2]; without clipping it is left alone and the coefficient is 1.
__device__ __forceinline__ double clip_coef(double* __restrict__ st, const double* __restrict__ sumsq,
                                            double max_norm, double grad_scale, int clip) {
  if (!clip) return 1.0;
  const double total = grad_scale * sqrt(sumsq[0]);
  const double c = max_norm / (total + 1e-6);
  st[2] = total;
  return c > 1.0 ? 1.0 : c;
}

__global__ void adamw_prep_kernel(double* __restrict__ st, const double* __restrict__ sumsq, double beta1,
                                  double beta2, double wd, double max_norm, double grad_scale, int clip) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double t = st[0] + 1.0;
  const double lr = st[1];
  const double bc1 = 1.0 - pow(beta1, t);
  const double bc2 = 1.0 - pow(beta2, t);
  const double coef = clip_coef(st, sumsq, max_norm, grad_scale, clip);
  st[0] = t;
  st[3] = coef;
  st[4] = lr / bc1;
  st[5] = 1.0 / sqrt(bc2);
  st[6] = grad_scale * coef;
  st[7] = lr * wd;
}

// ---------------------------------------------------------------------------------- update
struct AdamScalars {
  float step_size, rsqrt_bc2, gscale, decay;
};

// constants of the run, rounded to fp32 from double on the host: 1 - beta is NOT 1.f - (float)beta
// (1.f - 0.99f is 9e-7 away from 0.01, a bias in every step)
struct AdamConsts {
  float beta1, beta2, omb1, omb2, eps;
};

__device__ __forceinline__ AdamScalars adam_scalars(const double* __restrict__ st) {
  AdamScalars s;
  s.step_size = (float)st[4];
  s.rsqrt_bc2 = (float)st[5];
  s.gscale = (float)st[6];
  s.decay = (float)(1.0 - st[7]);
  return s;
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, bool decay, const AdamScalars& s,
                                         const AdamConsts& c) {
  g *= s.gscale;
  if (decay) p *= s.decay;
  m = c.beta1 * m + c.omb1 * g;
  v = c.beta2 * v + c.omb2 * (g * g);
  p -= s.step_size * (m / (sqrtf(v) * s.rsqrt_bc2 + c.eps));
}

// One 64-element unit of the flat buffer belongs to one parameter (offsets and shard boundaries are
// multiples of 64): dmap[unit_base + i / 64] != 0 <=> the unit decays; dmap == nullptr: all decay.
// VEC: p, g, m, v are 16-byte aligned and p16 8-byte aligned -> float4 body + scalar tail.
template <bool VEC>
__global__ __launch_bounds__(NT) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        bf16_t* __restrict__ p16, int64_t n,
                                                        const double* __restrict__ st,
                                                        const uint8_t* __restrict__ dmap, int64_t unit_base,
                                                        const AdamConsts c) {
  const AdamScalars s = adam_scalars(st);
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  const int64_t nvec = VEC ? (n >> 2) : 0;
  if (VEC) {
    for (int64_t i = tid; i < nvec; i += nthr) {
      float4 pp = ((float4*)p)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i];
      const float4 gg = ((const float4*)g)[i];
      const bool dec = dmap ? dmap[unit_base + (i >> 4)] != 0 : true;
      adam_one(pp.x, gg.x, mm.x, vv.x, dec, s, c);
      adam_one(pp.y, gg.y, mm.y, vv.y, dec, s, c);
      adam_one(pp.z, gg.z, mm.z, vv.z, dec, s, c);
      adam_one(pp.w, gg.w, mm.w, vv.w, dec, s, c);
      ((float4*)p)[i] = pp;
      ((float4*)m)[i] = mm;
      ((float4*)v)[i] = vv;
      if (p16) st4bf<true>(p16, i, pp);
    }
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += nthr) {
    float pi = p[i], mi = m[i], vi = v[i];
    const bool dec = dmap ? dmap[unit_base + (i >> 6)] != 0 : true;
    adam_one(pi, g[i], mi, vi, dec, s, c);
    p[i] = pi;
    m[i] = mi;
    v[i] = vi;
    if (p16) p16[i] = f2bf(pi);
  }
}


// ================================================================ layer-wise optimizers
// FlatLARS / FlatLAMB (parallel/optim.py): every parameter gets its own trust ratio from L2 norms
// taken per parameter over the flat buffer.  All launches below cover whole 64-element units
// (n % 64 == 0); a unit belongs to one parameter or to none (pidx < 0: alignment padding).
//
// Segmented squared norms, two passes, no atomics:
//   1. one fp64 partial per unit: 16 lanes x 4 elements, each lane sums its four squares in
//      order, a 16-lane xor tree finishes the unit.  The bits of a unit's partial depend only on
//      the unit's 64 values -- not on the launch, the grid or the pointer alignment (the scalar
//      path loads the same four elements per lane).
//   2. one block per (parameter, norm): thread t sums the partials lo + t, lo + t + 1024, ... of
//      the parameter's owned range [lo, hi) and a fixed tree finishes.  The order depends only on
//      the range, so one launch over the whole buffer and one per bucket shard give the same bits.
// LAMB's moments kernel produces its u^2 and w^2 unit partials itself (same 16-lane scheme) instead
// of calling pass 1: u exists only in registers there, and storing it would cost 8 B per element.
//
// LARS state block (doubles):  [0] step t  [1] lr
// LAMB state block (doubles):  [0] step t  [1] lr  [2] total_norm  [3] clip coefficient
//                              [4] bc1     [5] bc2 [6] grad_scale * coef          [7] unused
__device__ __forceinline__ double sq4(const float4& a) {
  double s = (double)a.x * (double)a.x;
  s += (double)a.y * (double)a.y;
  s += (double)a.z * (double)a.z;
  s += (double)a.w * (double)a.w;
  return s;
}

// sum over the 16 lanes of a unit (lane groups are 16-aligned: nthr and nvec are multiples of 16,
// so a group is active or idle as a whole); every lane of the group ends with the same value
__device__ __forceinline__ double unit_sum(double s) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// pass 1: pa[u] = sum of squares of unit u of a (and pb[u] of b when b != nullptr)
template <bool VEC>
__global__ __launch_bounds__(NT) void seg_unit_sq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         int64_t nvec, double* __restrict__ pa,
                                                         double* __restrict__ pb) {
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t i = tid; i < nvec; i += nthr) {
    const double sa = unit_sum(sq4(ld4<VEC>(a, i)));
    double sb = 0.0;
    if (b) sb = unit_sum(sq4(ld4<VEC>(b, i)));
    if ((threadIdx.x & 15) == 0) {
      pa[i >> 4] = sa;
      if (b) pb[i >> 4] = sb;
    }
  }
}

// pass 2: out[set * P + p] = sum of upart[set * set_stride + u], u in [table[2p], table[2p + 1]).
// 1024 threads: the largest parameters have ~37k units and one block walks them alone.
constexpr int RT = 1024;
__global__ __launch_bounds__(RT) void seg_reduce_kernel(const double* __restrict__ upart, int64_t set_stride,
                                                        const int64_t* __restrict__ table, int P,
                                                        double* __restrict__ out) {
  const int p = blockIdx.x, set = blockIdx.y;
  const int64_t lo = table[2 * p], hi = table[2 * p + 1];
  const double* src = upart + set * set_stride;
  double s = 0.0;
#pragma unroll 4
  for (int64_t u = lo + threadIdx.x; u < hi; u += RT) s += src[u];
  s = block_sum<RT>(s);
  if (threadIdx.x == 0) out[(int64_t)set * P + p] = s;
}

// ---------------------------------------------------------------------------- trust ratios
// sums = [||w||^2 per parameter | ||g||^2 per parameter] (g unscaled); the > 0 tests are plain
// comparisons, so a NaN norm gives q = 1.  Thread 0 also advances the step counter.
__global__ void lars_trust_kernel(const double* __restrict__ sums, const uint8_t* __restrict__ excl,
                                  float* __restrict__ q, double* __restrict__ st, int P, double tc, double wd,
                                  double eps, double grad_scale) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) st[0] += 1.0;
  if (p >= P) return;
  const double wn = sqrt(sums[p]), gn = grad_scale * sqrt(sums[P + p]);
  double r = 1.0;
  if (!excl[p] && wn > 0.0 && gn > 0.0) r = tc * wn / (gn + wd * wn + eps);
  q[p] = (float)r;
}

// sums = [||w||^2 per parameter | ||u||^2 per parameter]
__global__ void lamb_trust_kernel(const double* __restrict__ sums, const uint8_t* __restrict__ excl,
                                  float* __restrict__ q, int P) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const double wn = sqrt(sums[p]), un = sqrt(sums[P + p]);
  double r = 1.0;
  if (!excl[p] && wn > 0.0 && un > 0.0) r = wn / un;
  q[p] = (float)r;
}

// ------------------------------------------------------------------------------------ LARS
struct LarsConsts {
  float momentum, wd, gscale;
};

__device__ __forceinline__ void lars_one(float& w, float g, float& buf, bool ex, float q, float lr,
                                         const LarsConsts& c) {
  g *= c.gscale;
  const float d = ex ? g : q * (g + c.wd * w);
  buf = c.momentum * buf + d;
  w -= lr * buf;
}

// pidx[unit_base + unit]: parameter of the unit (< 0: none -> treated as excluded, q = 1)
template <bool VEC>
__global__ __launch_bounds__(NT) void lars_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ buf, bf16_t* __restrict__ p16,
                                                       int64_t nvec, const double* __restrict__ st,
                                                       const int32_t* __restrict__ pidx,
                                                       const uint8_t* __restrict__ excl,
                                                       const float* __restrict__ qv, int64_t unit_base,
                                                       const LarsConsts c) {
  const float lr = (float)st[1];
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t i = tid; i < nvec; i += nthr) {
    float4 pp = ld4<VEC>(p, i), bb = ld4<VEC>(buf, i);
    const float4 gg = ld4<VEC>(g, i);
    const int pi = pidx[unit_base + (i >> 4)];
    const bool ex = pi < 0 || excl[pi] != 0;
    const float q = ex ? 1.f : qv[pi];
    lars_one(pp.x, gg.x, bb.x, ex, q, lr, c);
    lars_one(pp.y, gg.y, bb.y, ex, q, lr, c);
    lars_one(pp.z, gg.z, bb.z, ex, q, lr, c);
    lars_one(pp.w, gg.w, bb.w, ex, q, lr, c);
    st4<VEC>(p, i, pp);
    st4<VEC>(buf, i, bb);
    if (p16) st4bf<VEC>(p16, i, pp);
  }
}

// ------------------------------------------------------------------------------------ LAMB
__global__ void lamb_prep_kernel(double* __restrict__ st, const double* __restrict__ sumsq, double beta1,
                                 double beta2, double max_norm, double grad_scale, int clip) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double t = st[0] + 1.0;
  const double coef = clip_coef(st, sumsq, max_norm, grad_scale, clip);
  st[0] = t;
  st[3] = coef;
  st[4] = 1.0 - pow(beta1, t);
  st[5] = 1.0 - pow(beta2, t);
  st[6] = grad_scale * coef;
}

struct LambConsts {
  float beta1, beta2, omb1, omb2, eps, wd;
};

struct LambScalars {
  float lr, bc1, bc2, gscale;
};

__device__ __forceinline__ LambScalars lamb_scalars(const double* __restrict__ st) {
  LambScalars s;
  s.lr = (float)st[1];
  s.bc1 = (float)st[4];
  s.bc2 = (float)st[5];
  s.gscale = (float)st[6];
  return s;
}

// u of one element from the stored moments and the not yet updated weight: the moments and the
// apply kernel both call this, so the applied u is the u whose norm went into q
__device__ __forceinline__ float lamb_u(float w, float m, float v, bool ex, const LambScalars& s,
                                        const LambConsts& c) {
  const float r = (m / s.bc1) / (sqrtf(v / s.bc2) + c.eps);
  return ex ? r : r + c.wd * w;
}

__device__ __forceinline__ float lamb_moments_one(float w, float g, float& m, float& v, bool ex,
                                                  const LambScalars& s, const LambConsts& c) {
  g *= s.gscale;
  m = c.beta1 * m + c.omb1 * g;
  v = c.beta2 * v + c.omb2 * (g * g);
  return lamb_u(w, m, v, ex, s, c);
}

// moments: m, v updated; pw[u], pu[u] = sums of w^2, u^2 over unit u of this launch
template <bool VEC>
__global__ __launch_bounds__(NT) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          int64_t nvec, const double* __restrict__ st,
                                                          const int32_t* __restrict__ pidx,
                                                          const uint8_t* __restrict__ excl, int64_t unit_base,
                                                          double* __restrict__ pw, double* __restrict__ pu,
                                                          const LambConsts c) {
  const LambScalars s = lamb_scalars(st);
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t i = tid; i < nvec; i += nthr) {
    const float4 pp = ld4<VEC>(p, i), gg = ld4<VEC>(g, i);
    float4 mm = ld4<VEC>(m, i), vv = ld4<VEC>(v, i);
    const int pi = pidx[unit_base + (i >> 4)];
    const bool ex = pi < 0 || excl[pi] != 0;
    float4 uu;
    uu.x = lamb_moments_one(pp.x, gg.x, mm.x, vv.x, ex, s, c);
    uu.y = lamb_moments_one(pp.y, gg.y, mm.y, vv.y, ex, s, c);
    uu.z = lamb_moments_one(pp.z, gg.z, mm.z, vv.z, ex, s, c);
    uu.w = lamb_moments_one(pp.w, gg.w, mm.w, vv.w, ex, s, c);
    st4<VEC>(m, i, mm);
    st4<VEC>(v, i, vv);
    const double sw = unit_sum(sq4(pp)), su = unit_sum(sq4(uu));
    if ((threadIdx.x & 15) == 0) {
      pw[i >> 4] = sw;
      pu[i >> 4] = su;
    }
  }
}

// apply: w -= lr * q * u with u recomputed from m, v and the still unchanged w
template <bool VEC>
__global__ __launch_bounds__(NT) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                        const float* __restrict__ v, bf16_t* __restrict__ p16,
                                                        int64_t nvec, const double* __restrict__ st,
                                                        const int32_t* __restrict__ pidx,
                                                        const uint8_t* __restrict__ excl,
                                                        const float* __restrict__ qv, int64_t unit_base,
                                                        const LambConsts c) {
  const LambScalars s = lamb_scalars(st);
  const int64_t tid = blockIdx.x * (int64_t)NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  for (int64_t i = tid; i < nvec; i += nthr) {
    float4 pp = ld4<VEC>(p, i);
    const float4 mm = ld4<VEC>(m, i), vv = ld4<VEC>(v, i);
    const int pi = pidx[unit_base + (i >> 4)];
    const bool ex = pi < 0 || excl[pi] != 0;
    const float step = s.lr * (ex ? 1.f : qv[pi]);
    pp.x -= step * lamb_u(pp.x, mm.x, vv.x, ex, s, c);
    pp.y -= step * lamb_u(pp.y, mm.y, vv.y, ex, s, c);
    pp.z -= step * lamb_u(pp.z, mm.z, vv.z, ex, s, c);
    pp.w -= step * lamb_u(pp.w, mm.w, vv.w, ex, s, c);
    st4<VEC>(p, i, pp);
    if (p16) st4bf<VEC>(p16, i, pp);
  }
}

// a launch takes the VEC path when its fp32 arrays are 16-byte aligned and its bf16 copy (or null) 8-byte
inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

inline bool aligned8(const void* p16) { return ((uintptr_t)p16 & 7) == 0; }

// kernel<true> when vec, else kernel<false>: NT threads, `blocks` blocks, on stream st
#define LAUNCH_VEC(kernel, vec, blocks, st, ...)                                           \
  do {                                                                                     \
    if (vec)                                                                               \
      hipLaunchKernelGGL(kernel<true>, dim3(blocks), dim3(NT), 0, st, __VA_ARGS__);        \
    else                                                                                   \
      hipLaunchKernelGGL(kernel<false>, dim3(blocks), dim3(NT), 0, st, __VA_ARGS__);       \
  } while (0)

inline LambConsts lamb_consts(double beta1, double beta2, double eps, double wd) {
  return {(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)wd};
}

}  // namespace

// blocks a segment of n elements uses in mi_grad_sqnorm_partial (= slots it writes)
MI_API int mi_grad_sqnorm_blocks(int64_t n) {
  const int64_t b = (n / 4 + NT - 1) / NT;
  return (int)std::max<int64_t>(1, std::min<int64_t>(SQ_MAX_BLOCKS, b));
}

// part: mi_grad_sqnorm_blocks(n) doubles, this segment's own slots
MI_API int mi_grad_sqnorm_partial(const float* x, int64_t n, double* part, hipStream_t st) {
  if (n < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(mi_grad_sqnorm_blocks(n)), dim3(NT), 0, st, x, n, part);
  return (int)hipGetLastError();
}

// out[0] = part[0] + ... + part[nparts - 1] in a fixed order
MI_API int mi_grad_sqnorm_final(const double* part, int nparts, double* out, hipStream_t st) {
  if (nparts < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(NT), 0, st, part, nparts, out);
  return (int)hipGetLastError();
}

// state: 8 doubles (layout at the top of this file); sumsq: 1 double, read only when clip != 0
MI_API int mi_adamw_prep(double* state, const double* sumsq, double beta1, double beta2, double wd, double max_norm,
                         double grad_scale, int clip, hipStream_t st) {
  if (clip && !sumsq) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(adamw_prep_kernel, dim3(1), dim3(64), 0, st, state, sumsq, beta1, beta2, wd, max_norm,
                     grad_scale, clip);
  return (int)hipGetLastError();
}

// dmap: one byte per 64-element unit of the flat buffer or null; unit_base: unit index of p[0]
MI_API int mi_adamw_flat(float* p, const float* g, float* m, float* v, void* p16, int64_t n, const double* state,
                         const uint8_t* dmap, int64_t unit_base, double beta1, double beta2, double eps,
                         hipStream_t st) {
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const AdamConsts c = {(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
  const bool vec = aligned16(p, g, m, v) && aligned8(p16);
  LAUNCH_VEC(adamw_flat_kernel, vec, ew_grid(vec ? (n + 3) / 4 : n), st, p, g, m, v, (bf16_t*)p16, n, state, dmap,
             unit_base, c);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- layer-wise optimizers
// All of these take whole units: n % 64 == 0.

// pa[u] (and pb[u] when b != null) = sum of squares of elements [64 u, 64 u + 64) of a (b)
MI_API int mi_seg_sqnorm_units(const float* a, const float* b, int64_t n, double* pa, double* pb, hipStream_t st) {
  if (n < 0 || (n & 63) || (b && !pb)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int64_t nvec = n >> 2;
  LAUNCH_VEC(seg_unit_sq_kernel, aligned16(a, b), ew_grid(nvec), st, a, b, nvec, pa, pb);
  return (int)hipGetLastError();
}

// out[s * P + p] = sum of upart[s * set_stride + u] for u in [table[2 p], table[2 p + 1]), s < nsets
MI_API int mi_seg_sqnorm_reduce(const double* upart, int64_t set_stride, int nsets, const int64_t* table, int P,
                                double* out, hipStream_t st) {
  if (P < 0 || nsets < 1 || nsets > 65535) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  hipLaunchKernelGGL(seg_reduce_kernel, dim3(P, nsets), dim3(RT), 0, st, upart, set_stride, table, P, out);
  return (int)hipGetLastError();
}

// sums: 2 P doubles [w | g]; excl: P bytes; q: P floats; state: LARS block (step counter advanced)
MI_API int mi_lars_trust(const double* sums, const uint8_t* excl, float* q, double* state, int P, double tc,
                         double wd, double eps, double grad_scale, hipStream_t st) {
  if (P < 0) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lars_trust_kernel, dim3(std::max(1, (P + NT - 1) / NT)), dim3(NT), 0, st, sums, excl, q, state,
                     P, tc, wd, eps, grad_scale);
  return (int)hipGetLastError();
}

// sums: 2 P doubles [w | u]
MI_API int mi_lamb_trust(const double* sums, const uint8_t* excl, float* q, int P, hipStream_t st) {
  if (P < 0) return (int)hipErrorInvalidValue;
  if (P == 0) return 0;
  hipLaunchKernelGGL(lamb_trust_kernel, dim3((P + NT - 1) / NT), dim3(NT), 0, st, sums, excl, q, P);
  return (int)hipGetLastError();
}

// pidx: parameter index per 64-element unit of the flat buffer (< 0: none); unit_base: unit of p[0]
MI_API int mi_lars_flat(float* p, const float* g, float* buf, void* p16, int64_t n, const double* state,
                        const int32_t* pidx, const uint8_t* excl, const float* q, int64_t unit_base,
                        double momentum, double wd, double grad_scale, hipStream_t st) {
  if (n < 0 || (n & 63)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const LarsConsts c = {(float)momentum, (float)wd, (float)grad_scale};
  const int64_t nvec = n >> 2;
  LAUNCH_VEC(lars_flat_kernel, aligned16(p, g, buf) && aligned8(p16), ew_grid(nvec), st, p, g, buf, (bf16_t*)p16,
             nvec, state, pidx, excl, q, unit_base, c);
  return (int)hipGetLastError();
}

// state: LAMB block (8 doubles); sumsq: 1 double, read only when clip != 0
MI_API int mi_lamb_prep(double* state, const double* sumsq, double beta1, double beta2, double max_norm,
                        double grad_scale, int clip, hipStream_t st) {
  if (clip && !sumsq) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(lamb_prep_kernel, dim3(1), dim3(64), 0, st, state, sumsq, beta1, beta2, max_norm, grad_scale,
                     clip);
  return (int)hipGetLastError();
}

// pw, pu: n / 64 doubles each, the unit partials of w^2 and u^2 of this launch
MI_API int mi_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const double* state,
                           const int32_t* pidx, const uint8_t* excl, int64_t unit_base, double* pw, double* pu,
                           double beta1, double beta2, double eps, double wd, hipStream_t st) {
  if (n < 0 || (n & 63)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int64_t nvec = n >> 2;
  LAUNCH_VEC(lamb_moments_kernel, aligned16(p, g, m, v), ew_grid(nvec), st, p, g, m, v, nvec, state, pidx, excl,
             unit_base, pw, pu, lamb_consts(beta1, beta2, eps, wd));
  return (int)hipGetLastError();
}

MI_API int mi_lamb_apply(float* p, const float* m, const float* v, void* p16, int64_t n, const double* state,
                         const int32_t* pidx, const uint8_t* excl, const float* q, int64_t unit_base, double beta1,
                         double beta2, double eps, double wd, hipStream_t st) {
  if (n < 0 || (n & 63)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  const int64_t nvec = n >> 2;
  LAUNCH_VEC(lamb_apply_kernel, aligned16(p, m, v) && aligned8(p16), ew_grid(nvec), st, p, m, v, (bf16_t*)p16, nvec,
             state, pidx, excl, q, unit_base, lamb_consts(beta1, beta2, eps, wd));
  return (int)hipGetLastError();
}
