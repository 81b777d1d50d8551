// Input pipeline with a per-image crop box and a bilinear resample (gfx950, MI355X):
// RandomResizedCrop, resize + centre crop, RandomErasing, and Mixup / CutMix on top, in one
// uint8 NHWC -> bf16 NHWC pass.
//
// augment_resized is mix.hip's augment_mix whose source pixel is found by a box and a resample
// instead of by a shift.  Per-image parameters (device resident, data.crops.BatchCropper):
//   crop  int32 [N][4] = (top, left, height, width) in source pixels
//   flip  int32 [N]
//   erase int32 [N][4] = (y0, y1, x0, x1) in output pixels; an empty box erases nothing
// Every box is clipped to its domain here before use (the crop into the source with height and
// width >= 1, the erase and CutMix boxes into the output), so no parameter value can address
// memory outside the image.
//
// Value of image m at output pixel (h, w):  w' = flip[m] ? Wo - 1 - w : w, and per axis, in exact
// integer arithmetic,
//   num = max((2 * o + 1) * len - n_out, 0);  i0 = num / (2 * n_out);
//   lambda = (num % (2 * n_out)) / float(2 * n_out);  i1 = min(i0 + 1, len - 1)
// both offset by the box origin: "crop, then bilinear interpolation with half-pixel centres,
// clamped to the box, no antialiasing".  lambda carries no fp32 coordinate rounding, and a box of
// the output's size returns the source pixels exactly.  The four taps are blended in fp32,
// normalized with augment's expression, and the value is 0 (normalized space) inside the image's
// own erase box.
//
// Mixing is augment_mix's rule applied to those values (see mix.hip): image and partner each use
// their own crop, flip and erase box; a pixel that needs one source reads one source.  A null
// partner pointer means no mixing, and no target is written.
#include "common.h"

namespace {
constexpr int NT = 256;
constexpr int MAX_SIDE = 16384;  // (2 * o + 1) * len < 2^29 and 2 * Ho * Wo <= 2^29: int32 throughout

// the four taps of one output pixel in one source image; p00 == nullptr: erased, the value is 0
struct Taps {
  const uint8_t *p00, *p01, *p10, *p11;
  float lx, ly;
};

// one axis: first tap, second tap (clamped to the box) and the weight of the second; n_out2 = 2 * n_out
__device__ __forceinline__ void axis(int o, int len, int n_out, const FastDiv& n_out2, int& i0, int& i1, float& l) {
  const uint32_t num = (uint32_t)max((2 * o + 1) * len - n_out, 0);
  const uint32_t q = fdiv(num, n_out2);
  i0 = (int)q;
  i1 = min(i0 + 1, len - 1);
  l = (float)(num - q * n_out2.d) / (float)n_out2.d;
}

// taps of output pixel (h, w) in image m under that image's own crop, flip and erase box; all of
// m's parameters are wave-uniform
__device__ __forceinline__ Taps taps_of(const uint8_t* __restrict__ src, const int* __restrict__ crop,
                                        const int* __restrict__ flip, const int* __restrict__ erase, int m, int h,
                                        int w, int Hs, int Ws, int Ho, int Wo, const FastDiv& Ho2, const FastDiv& Wo2,
                                        int C) {
  Taps t;
  t.p00 = t.p01 = t.p10 = t.p11 = nullptr;
  t.lx = t.ly = 0.f;
  const int ey0 = max(erase[4 * m + 0], 0), ey1 = min(erase[4 * m + 1], Ho);
  const int ex0 = max(erase[4 * m + 2], 0), ex1 = min(erase[4 * m + 3], Wo);
  if (h >= ey0 && h < ey1 && w >= ex0 && w < ex1) return t;
  const int top = min(max(crop[4 * m + 0], 0), Hs - 1), left = min(max(crop[4 * m + 1], 0), Ws - 1);
  const int ch = min(max(crop[4 * m + 2], 1), Hs - top), cw = min(max(crop[4 * m + 3], 1), Ws - left);
  const int wf = flip[m] ? Wo - 1 - w : w;
  int y0, y1, x0, x1;
  axis(h, ch, Ho, Ho2, y0, y1, t.ly);
  axis(wf, cw, Wo, Wo2, x0, x1, t.lx);
  const uint8_t* r0 = src + ((size_t)m * Hs + (top + y0)) * Ws * C;
  const uint8_t* r1 = src + ((size_t)m * Hs + (top + y1)) * Ws * C;
  t.p00 = r0 + (size_t)(left + x0) * C;
  t.p01 = r0 + (size_t)(left + x1) * C;
  t.p10 = r1 + (size_t)(left + x0) * C;
  t.p11 = r1 + (size_t)(left + x1) * C;
  return t;
}

// channel c of the resampled pixel: fp32 blend of the four taps, then augment's normalisation, term
// for term (lambda == 0 returns the tap itself, so the identity geometry is bit-equal to augment)
__device__ __forceinline__ float value(const Taps& t, int c, const float* __restrict__ mean,
                                       const float* __restrict__ stdinv) {
  if (!t.p00) return 0.f;
  const float a = (float)t.p00[c], b = (float)t.p01[c], d = (float)t.p10[c], e = (float)t.p11[c];
  const float up = a + t.lx * (b - a);
  const float dn = d + t.lx * (e - d);
  const float v = up + t.ly * (dn - up);
  return (v * (1.f / 255.f) - mean[c]) * stdinv[c];
}

__global__ __launch_bounds__(NT) void augment_resized_kernel(
    const uint8_t* __restrict__ src, bf16_t* __restrict__ dst, const int* __restrict__ crop,
    const int* __restrict__ flip, const int* __restrict__ erase, const int64_t* __restrict__ labels,
    const int* __restrict__ partner, const float* __restrict__ lam, const int* __restrict__ box,
    int64_t* __restrict__ ya, int64_t* __restrict__ yb, float* __restrict__ lam_out, int Nb, int Hs, int Ws, int Ho,
    int Wo, FastDiv Ho2, FastDiv Wo2, int C, int Cout, const float* __restrict__ mean,
    const float* __restrict__ stdinv) {
  // one image per blockIdx.y: its parameters and the mode are wave-uniform (scalar loads, scalar
  // ALU); the only divisors are the kernel arguments Ho2 = 2 * Ho and Wo2 = 2 * Wo, and the quotients
  // are exact through their host-built reciprocals (common.h's FastDiv: a multiply-high and shifts)
  const int n = blockIdx.y;
  const int pix = blockIdx.x * NT + threadIdx.x;
  if (pix >= Ho * Wo) return;
  const int h = (int)fdiv((uint32_t)(2 * pix), Wo2);
  const int w = pix - h * Wo;
  const int64_t t = (int64_t)n * (Ho * Wo) + pix;
  int p = n;
  float la = 1.f;
  bool need_a = true, need_b = false;
  if (partner) {  // augment_mix's rule
    p = partner[n];
    la = lam[n];
    const int y0 = max(box[4 * n + 0], 0), y1 = min(box[4 * n + 1], Ho);
    const int x0 = max(box[4 * n + 2], 0), x1 = min(box[4 * n + 3], Wo);
    bool cut = y1 > y0 && x1 > x0;
    if ((unsigned)p >= (unsigned)Nb) { p = n; la = 1.f; cut = false; }  // no mixing; p is a valid index from here
    if (pix == 0) {  // one thread per image emits the loss target
      ya[n] = labels[n];
      yb[n] = labels[p];
      lam_out[n] = cut ? 1.f - (float)((y1 - y0) * (x1 - x0)) / (float)(Ho * Wo) : la;
    }
    if (cut) {
      need_b = h >= y0 && h < y1 && w >= x0 && w < x1;
      need_a = !need_b;
    } else {
      need_a = la != 0.f;
      need_b = la != 1.f;
    }
  }
  const bool blend = need_a && need_b;
  const Taps t1 = taps_of(src, crop, flip, erase, need_a ? n : p, h, w, Hs, Ws, Ho, Wo, Ho2, Wo2, C);
  Taps tb = t1;
  if (blend) tb = taps_of(src, crop, flip, erase, p, h, w, Hs, Ws, Ho, Wo, Ho2, Wo2, C);
  if (Cout == 8 && C <= 8) {
    // one 16-byte store per pixel (the stem's 8-channel layout)
    float f[8];
    if (!blend) {
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = c < C ? value(t1, c, mean, stdinv) : 0.f;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float va = c < C ? value(t1, c, mean, stdinv) : 0.f;
        const float vb = c < C ? value(tb, c, mean, stdinv) : 0.f;
        f[c] = la * va + (1.f - la) * vb;
      }
    }
    *(uint4*)(dst + (size_t)t * 8) = pack8(f);
    return;
  }
  bf16_t* o = dst + (size_t)t * Cout;
  for (int c = 0; c < Cout; ++c) {
    float v = 0.f;
    if (c < C) {
      if (!blend) {
        v = value(t1, c, mean, stdinv);
      } else {
        const float va = value(t1, c, mean, stdinv);
        const float vb = value(tb, c, mean, stdinv);
        v = la * va + (1.f - la) * vb;
      }
    }
    o[c] = f2bf(v);
  }
}

}  // namespace

// src uint8 [Nb][Hs][Ws][C] -> dst bf16 [Nb][Ho][Wo][Cout]; crop / erase int32 [Nb][4]; flip int32 [Nb];
// mean / stdinv fp32 [max(C, Cout)].  Mixing operands as in mi_augment_mix; partner == nullptr: no
// mixing, and labels / lam / box / ya / yb / lam_out are not touched.
MI_API int mi_augment_resized(const void* src, void* dst, const int* crop, const int* flip, const int* erase,
                              const int64_t* labels, const int* partner, const float* lam, const int* box,
                              int64_t* ya, int64_t* yb, float* lam_out, int Nb, int Hs, int Ws, int Ho, int Wo, int C,
                              int Cout, const float* mean, const float* stdinv, hipStream_t st) {
  if (Nb <= 0 || Nb > 65535 || Hs <= 0 || Hs > MAX_SIDE || Ws <= 0 || Ws > MAX_SIDE || Ho <= 0 || Ho > MAX_SIDE ||
      Wo <= 0 || Wo > MAX_SIDE || C <= 0 || Cout < C)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_resized_kernel, dim3(cdiv((int64_t)Ho * Wo, NT), Nb), dim3(NT), 0, st,
                     (const uint8_t*)src, (bf16_t*)dst, crop, flip, erase, labels, partner, lam, box, ya, yb, lam_out,
                     Nb, Hs, Ws, Ho, Wo, make_fastdiv(2u * Ho), make_fastdiv(2u * Wo), C, Cout, mean, stdinv);
  return (int)hipGetLastError();
}
