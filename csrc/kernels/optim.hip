// Flat AdamW with on-device global-norm gradient clipping for gfx950 (MI355X).
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

// -------------------------------------------------------------------- squared gradient norm
// Block b writes its fp64 partial to part[b]; sqnorm_final_kernel sums all slots of all segments
// in a fixed order.  16-byte loads over the aligned body, scalar loads for an unaligned head
// (x only 4-byte aligned) and the tail.
__global__ __launch_bounds__(NT) void sqnorm_partial_kernel(const float* __restrict__ x, int64_t n,
                                                            double* __restrict__ part) {
  __shared__ double red[NT / 64];
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
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(NT) void sqnorm_final_kernel(const double* __restrict__ part, int nparts,
                                                          double* __restrict__ out) {
  __shared__ double red[NT / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += NT) s += part[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------ prep
// clip_grad_norm_ semantics: coef = min(1, max_norm / (total_norm + 1e-6)), a NaN norm gives a NaN
// coefficient (torch clamps with max=1, which keeps NaN), an infinite norm gives 0.
__global__ void adamw_prep_kernel(double* __restrict__ st, const double* __restrict__ sumsq, double beta1,
                                  double beta2, double wd, double max_norm, double grad_scale, int clip) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double t = st[0] + 1.0;
  const double lr = st[1];
  const double bc1 = 1.0 - pow(beta1, t);
  const double bc2 = 1.0 - pow(beta2, t);
  double coef = 1.0;
  if (clip) {
    const double total = grad_scale * sqrt(sumsq[0]);
    const double c = max_norm / (total + 1e-6);
    coef = c > 1.0 ? 1.0 : c;
    st[2] = total;
  }
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
      if (p16) {
        uint2 o;
        o.x = pack2bf(pp.x, pp.y);
        o.y = pack2bf(pp.z, pp.w);
        ((uint2*)p16)[i] = o;
      }
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
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0 &&
                   ((uintptr_t)p16 & 7) == 0;
  if (vec)
    hipLaunchKernelGGL(adamw_flat_kernel<true>, dim3(ew_grid((n + 3) / 4)), dim3(NT), 0, st, p, g, m, v,
                       (bf16_t*)p16, n, state, dmap, unit_base, c);
  else
    hipLaunchKernelGGL(adamw_flat_kernel<false>, dim3(ew_grid(n)), dim3(NT), 0, st, p, g, m, v, (bf16_t*)p16, n,
                       state, dmap, unit_base, c);
  return (int)hipGetLastError();
}
