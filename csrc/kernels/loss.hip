// Soft-target cross entropy for gfx950 (MI355X): label smoothing, pair targets (Mixup / CutMix)
// and dense probability targets.  torch.nn.functional.cross_entropy semantics with mean reduction,
// smoothing applied to probability targets as q = (1 - eps) * t + eps / C.
//
//   pair  (a, b, lam):  q_c = eps/C + (1-eps) * (lam [c == a] + (1-lam) [c == b]),  sum_c q_c = 1
//          row loss = lse - (1-eps) (lam l[a] + (1-lam) l[b]) - (eps/C) sum_c l_c
//          gradient = g/N (softmax_c - q_c)
//          hard labels with smoothing are the pair (y, y, lam = 1) -- lam == nullptr.
//   dense t [N][C] (fp32 or bf16, rows need not sum to one):
//          row loss = lse sum_c q_c - sum_c q_c l_c
//          gradient = g/N (softmax_c sum q - q_c)
//
// Same shape as misc.hip's hard-label kernels: one 256-thread block per row, fp32 logits with a
// leading dimension, the gradient in the logits' own dtype with zeros in padding columns, the
// mean taken in row order (bit-reproducible).  [N][C] is never materialised for a pair target and
// the backward recomputes q from (a, b, lam, eps).  A class index outside [0, C) contributes
// nothing and is never used as an index.
#include "common.h"
#include <type_traits>

namespace {
constexpr int NT = 256;

// sum over the block's 4 waves in a fixed order; every thread gets the total
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ float ld_tgt(const float* t, int c) { return t[c]; }
__device__ __forceinline__ float ld_tgt(const bf16_t* t, int c) { return bf2f(t[c]); }

// ws: fp32 [2 * N] -- log-sum-exp per row (read by the backward), then the per-row losses
__global__ __launch_bounds__(NT) void ce_pair_fwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ ya,
                                                         const int64_t* __restrict__ yb,
                                                         const float* __restrict__ lam, float* __restrict__ ws,
                                                         int ncls, int ld, float eps) {
  __shared__ float red[NT / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* l = logits + (size_t)row * ld;
  float m = -INFINITY;
  for (int c = tid; c < ncls; c += NT) m = fmaxf(m, l[c]);
  m = block_max(m, red);
  float s = 0.f, sl = 0.f;  // the sum of the logits rides in the exp-sum pass
  for (int c = tid; c < ncls; c += NT) {
    const float v = l[c];
    s += __expf(v - m);
    sl += v;
  }
  s = block_sum(s, red);
  sl = block_sum(sl, red);
  if (tid == 0) {
    const float ls = m + __logf(s);
    const int64_t a = ya[row], b = yb[row];
    const float la = lam ? lam[row] : 1.f;
    float hit = 0.f;
    if (la != 0.f && a >= 0 && a < ncls) hit += la * l[a];
    if (la != 1.f && b >= 0 && b < ncls) hit += (1.f - la) * l[b];
    float r = ls - (1.f - eps) * hit;
    if (eps != 0.f) r -= eps / (float)ncls * sl;
    ws[row] = ls;
    ws[gridDim.x + row] = r;
  }
}

// ws: fp32 [3 * N] -- lse rows, per-row losses, sum_c q_c per row (read by the backward)
template <typename TT>
__global__ __launch_bounds__(NT) void ce_dense_fwd_kernel(const float* __restrict__ logits,
                                                          const TT* __restrict__ tgt, float* __restrict__ ws,
                                                          int ncls, int ld, int ldt, float eps) {
  __shared__ float red[NT / 64];
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* l = logits + (size_t)row * ld;
  const TT* t = tgt + (size_t)row * ldt;
  float m = -INFINITY;
  for (int c = tid; c < ncls; c += NT) m = fmaxf(m, l[c]);
  m = block_max(m, red);
  float s = 0.f, sl = 0.f, st = 0.f, stl = 0.f;
  for (int c = tid; c < ncls; c += NT) {
    const float v = l[c], tv = ld_tgt(t, c);
    s += __expf(v - m);
    sl += v;
    st += tv;
    if (tv != 0.f) stl += tv * v;
  }
  s = block_sum(s, red);
  sl = block_sum(sl, red);
  st = block_sum(st, red);
  stl = block_sum(stl, red);
  if (tid == 0) {
    const float ls = m + __logf(s);
    float sq = (1.f - eps) * st, sql = (1.f - eps) * stl;
    if (eps != 0.f) { sq += eps; sql += eps / (float)ncls * sl; }
    ws[row] = ls;
    ws[gridDim.x + row] = ls * sq - sql;
    ws[2 * gridDim.x + row] = sq;
  }
}

// mean of the per-row losses in a fixed order (the loss is bit-reproducible, unlike an atomic sum)
__global__ __launch_bounds__(NT) void ce_soft_sum_kernel(const float* __restrict__ rowloss, float* __restrict__ loss,
                                                         int n, float inv_n) {
  __shared__ float red[NT];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += NT) s += rowloss[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] * inv_n;
}

template <typename T>
__device__ __forceinline__ void st_grad(T* dl, size_t i, float v) {
  if constexpr (std::is_same<T, float>::value)
    dl[i] = v;
  else
    dl[i] = f2bf(v);
}

// dlogits[n][c] = g * inv_n * (softmax - q), [N][ldo] in the logits' own dtype, zero in padding columns
template <typename T>
__global__ __launch_bounds__(NT) void ce_pair_bwd_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ ya,
                                                         const int64_t* __restrict__ yb,
                                                         const float* __restrict__ lam, const float* __restrict__ ws,
                                                         const float* __restrict__ gout, T* __restrict__ dl, int ncls,
                                                         int ld, int ldo, float eps, float inv_n) {
  const int row = blockIdx.x;
  const float g = gout[0] * inv_n;
  const float ls = ws[row];
  const int64_t a = ya[row], b = yb[row];  // compared with c only, never an index
  const float la = lam ? lam[row] : 1.f;
  const float wa = (1.f - eps) * la, wb = (1.f - eps) * (1.f - la), u = eps / (float)ncls;
  const float* l = logits + (size_t)row * ld;
  for (int c = threadIdx.x; c < ldo; c += NT) {
    float v = 0.f;
    if (c < ncls) {
      float q = u;
      if (c == a) q += wa;
      if (c == b) q += wb;
      v = g * (__expf(l[c] - ls) - q);
    }
    st_grad(dl, (size_t)row * ldo + c, v);
  }
}

template <typename T, typename TT>
__global__ __launch_bounds__(NT) void ce_dense_bwd_kernel(const float* __restrict__ logits,
                                                          const TT* __restrict__ tgt, const float* __restrict__ ws,
                                                          const float* __restrict__ gout, T* __restrict__ dl, int ncls,
                                                          int ld, int ldt, int ldo, float eps, float inv_n) {
  const int row = blockIdx.x;
  const float g = gout[0] * inv_n;
  const float ls = ws[row], sq = ws[2 * gridDim.x + row];
  const float u = eps / (float)ncls;
  const float* l = logits + (size_t)row * ld;
  const TT* t = tgt + (size_t)row * ldt;
  for (int c = threadIdx.x; c < ldo; c += NT) {
    float v = 0.f;
    if (c < ncls) v = g * (__expf(l[c] - ls) * sq - ((1.f - eps) * ld_tgt(t, c) + u));
    st_grad(dl, (size_t)row * ldo + c, v);
  }
}

}  // namespace

// ws: fp32 [2 * N].  lam == nullptr: lam = 1 for every row (hard labels with smoothing, ya == yb).
MI_API int mi_ce_pair_fwd(const float* logits, const int64_t* ya, const int64_t* yb, const float* lam, float* ws,
                          float* loss, int N, int ncls, int ld, float eps, hipStream_t st) {
  if (N <= 0 || ncls <= 0 || ld < ncls) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ce_pair_fwd_kernel, dim3(N), dim3(NT), 0, st, logits, ya, yb, lam, ws, ncls, ld, eps);
  hipLaunchKernelGGL(ce_soft_sum_kernel, dim3(1), dim3(NT), 0, st, ws + N, loss, N, 1.f / N);
  return (int)hipGetLastError();
}

// out_f32: dl is fp32 (else bf16)
MI_API int mi_ce_pair_bwd(const float* logits, const int64_t* ya, const int64_t* yb, const float* lam,
                          const float* ws, const float* gout, void* dl, int N, int ncls, int ld, int ldo, float eps,
                          int out_f32, hipStream_t st) {
  if (N <= 0 || ncls <= 0 || ld < ncls || ldo < ncls) return (int)hipErrorInvalidValue;
  if (out_f32)
    hipLaunchKernelGGL(ce_pair_bwd_kernel<float>, dim3(N), dim3(NT), 0, st, logits, ya, yb, lam, ws, gout,
                       (float*)dl, ncls, ld, ldo, eps, 1.f / N);
  else
    hipLaunchKernelGGL(ce_pair_bwd_kernel<bf16_t>, dim3(N), dim3(NT), 0, st, logits, ya, yb, lam, ws, gout,
                       (bf16_t*)dl, ncls, ld, ldo, eps, 1.f / N);
  return (int)hipGetLastError();
}

// ws: fp32 [3 * N].  tgt_bf16: the targets are bf16 (else fp32), leading dimension ldt.
MI_API int mi_ce_dense_fwd(const float* logits, const void* tgt, int tgt_bf16, float* ws, float* loss, int N, int ncls,
                           int ld, int ldt, float eps, hipStream_t st) {
  if (N <= 0 || ncls <= 0 || ld < ncls || ldt < ncls) return (int)hipErrorInvalidValue;
  if (tgt_bf16)
    hipLaunchKernelGGL(ce_dense_fwd_kernel<bf16_t>, dim3(N), dim3(NT), 0, st, logits, (const bf16_t*)tgt, ws, ncls,
                       ld, ldt, eps);
  else
    hipLaunchKernelGGL(ce_dense_fwd_kernel<float>, dim3(N), dim3(NT), 0, st, logits, (const float*)tgt, ws, ncls, ld,
                       ldt, eps);
  hipLaunchKernelGGL(ce_soft_sum_kernel, dim3(1), dim3(NT), 0, st, ws + N, loss, N, 1.f / N);
  return (int)hipGetLastError();
}

MI_API int mi_ce_dense_bwd(const float* logits, const void* tgt, int tgt_bf16, const float* ws, const float* gout,
                           void* dl, int N, int ncls, int ld, int ldt, int ldo, float eps, int out_f32,
                           hipStream_t st) {
  if (N <= 0 || ncls <= 0 || ld < ncls || ldt < ncls || ldo < ncls) return (int)hipErrorInvalidValue;
#define MI_CE_DENSE_BWD(T, TT)                                                                                   \
  hipLaunchKernelGGL((ce_dense_bwd_kernel<T, TT>), dim3(N), dim3(NT), 0, st, logits, (const TT*)tgt, ws, gout, \
                     (T*)dl, ncls, ld, ldt, ldo, eps, 1.f / N)
  if (out_f32) {
    if (tgt_bf16) MI_CE_DENSE_BWD(float, bf16_t); else MI_CE_DENSE_BWD(float, float);
  } else {
    if (tgt_bf16) MI_CE_DENSE_BWD(bf16_t, bf16_t); else MI_CE_DENSE_BWD(bf16_t, float);
  }
#undef MI_CE_DENSE_BWD
  return (int)hipGetLastError();
}
