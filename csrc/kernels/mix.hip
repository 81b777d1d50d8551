// Input pipeline with Mixup / CutMix folded into the uint8 -> bf16 pass (gfx950, MI355X).
//
// augment_mix is misc.hip's augment (random crop with zero padding + hflip + normalize, uint8 NHWC
// -> bf16 NHWC) whose output pixel of image n is computed from image n and from its partner image
// partner[n].  Each of the two keeps its OWN crop and flip, drawn from the same counter hash of
// (seed, image) that augment uses, so for one seed they are the geometry augment gives that image.
//
// Per-sample parameters (device resident): partner int32 [N], lam fp32 [N], box int32 [N][4] =
// (y0, y1, x0, x1) in output coordinates, clipped to the image here.
//   empty box      Mixup:  out = lam * a + (1 - lam) * b, blended in fp32, one bf16 rounding
//   non-empty box  CutMix: b inside the box, a outside, no blend
// A pixel that needs one source reads one source (every CutMix pixel, and Mixup at lam == 1 or 0);
// only true Mixup pixels read two.  A partner outside [0, N) means "no mixing" for that sample and
// is never used as an index.
//
// The kernel also writes the loss target of the batch, so no ATen gather / arithmetic launch is
// needed for the labels: y_a[n] = labels[n], y_b[n] = labels[partner[n]] and the label-side lam
// (Mixup: lam; CutMix: 1 - box_area / (H * W) of the clipped box).
#include "common.h"

namespace {
constexpr int NT = 256;

// the counter hash of misc.hip's augment_kernel
__device__ __forceinline__ uint32_t hash32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}

// source pixel of output pixel (h, w) of image n under that image's own crop / flip; nullptr when
// the crop's zero padding is hit
__device__ __forceinline__ const uint8_t* src_pixel(const uint8_t* __restrict__ src, int n, int h, int w, int H, int W,
                                                    int C, int pad, int flip, uint32_t seed) {
  const uint32_t hv = hash32(seed * 0x9E3779B9u + (uint32_t)n);
  int dy = 0, dx = 0, fl = 0;
  if (pad > 0) { dy = (int)(hv % (2 * pad + 1)) - pad; dx = (int)((hv >> 8) % (2 * pad + 1)) - pad; }
  if (flip) fl = (hv >> 20) & 1;
  const int sh = h + dy;
  const int sw = (fl ? (W - 1 - w) : w) + dx;
  if ((unsigned)sh >= (unsigned)H || (unsigned)sw >= (unsigned)W) return nullptr;
  return src + (((size_t)n * H + sh) * W + sw) * C;
}

// augment's normalisation, term for term (the identity case is bit-equal to augment)
__device__ __forceinline__ float norm_px(const uint8_t* sp, int c, const float* __restrict__ mean,
                                         const float* __restrict__ stdinv) {
  return ((float)sp[c] * (1.f / 255.f) - mean[c]) * stdinv[c];
}

__global__ __launch_bounds__(NT) void augment_mix_kernel(
    const uint8_t* __restrict__ src, bf16_t* __restrict__ dst, const int64_t* __restrict__ labels,
    const int* __restrict__ partner, const float* __restrict__ lam, const int* __restrict__ box,
    int64_t* __restrict__ ya, int64_t* __restrict__ yb, float* __restrict__ lam_out, int Nb, int H, int W, int C,
    int Cout, int pad, int flip, uint32_t seed, const float* __restrict__ mean, const float* __restrict__ stdinv) {
  // one image per blockIdx.y: the image's parameters, its hash and the mode are wave-uniform (scalar
  // loads and scalar ALU), and the pixel index needs 32-bit arithmetic only
  const int n = blockIdx.y;
  const int pix = blockIdx.x * NT + threadIdx.x;
  if (pix >= H * W) return;
  const int w = pix % W;
  const int h = pix / W;
  const int64_t t = (int64_t)n * (H * W) + pix;
  int p = partner[n];
  float la = lam[n];
  int y0 = max(box[4 * n + 0], 0), y1 = min(box[4 * n + 1], H);
  int x0 = max(box[4 * n + 2], 0), x1 = min(box[4 * n + 3], W);
  bool cut = y1 > y0 && x1 > x0;
  if ((unsigned)p >= (unsigned)Nb) { p = n; la = 1.f; cut = false; }  // no mixing; p is a valid index from here
  if (pix == 0) {  // one thread per image emits the loss target
    ya[n] = labels[n];
    yb[n] = labels[p];
    lam_out[n] = cut ? 1.f - (float)((y1 - y0) * (x1 - x0)) / (float)(H * W) : la;
  }
  // which sources this pixel needs
  bool need_a, need_b;
  if (cut) {
    need_b = h >= y0 && h < y1 && w >= x0 && w < x1;
    need_a = !need_b;
  } else {
    need_a = la != 0.f;
    need_b = la != 1.f;
  }
  const uint8_t* pa = need_a ? src_pixel(src, n, h, w, H, W, C, pad, flip, seed) : nullptr;
  const uint8_t* pb = need_b ? src_pixel(src, p, h, w, H, W, C, pad, flip, seed) : nullptr;
  const bool blend = need_a && need_b;
  const uint8_t* p1 = need_a ? pa : pb;  // the only source of a one-source pixel
  if (Cout == 8 && C <= 8) {
    // one 16-byte store per pixel (the stem's 8-channel layout)
    float f[8];
    if (!blend) {
#pragma unroll
      for (int c = 0; c < 8; ++c) f[c] = (c < C && p1) ? norm_px(p1, c, mean, stdinv) : 0.f;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float va = (c < C && pa) ? norm_px(pa, c, mean, stdinv) : 0.f;
        const float vb = (c < C && pb) ? norm_px(pb, c, mean, stdinv) : 0.f;
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
        if (p1) v = norm_px(p1, c, mean, stdinv);
      } else {
        const float va = pa ? norm_px(pa, c, mean, stdinv) : 0.f;
        const float vb = pb ? norm_px(pb, c, mean, stdinv) : 0.f;
        v = la * va + (1.f - la) * vb;
      }
    }
    o[c] = f2bf(v);
  }
}

}  // namespace

// src uint8 [Nb][H][W][C] -> dst bf16 [Nb][H][W][Cout]; labels / ya / yb int64 [Nb]; partner int32 [Nb];
// lam / lam_out fp32 [Nb]; box int32 [Nb][4]; mean / stdinv fp32 [max(C, Cout)]
MI_API int mi_augment_mix(const void* src, void* dst, const int64_t* labels, const int* partner, const float* lam,
                          const int* box, int64_t* ya, int64_t* yb, float* lam_out, int Nb, int H, int W, int C,
                          int Cout, int pad, int flip, uint32_t seed, const float* mean, const float* stdinv,
                          hipStream_t st) {
  if (Nb <= 0 || Nb > 65535 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 30) || C <= 0 || Cout < C || pad < 0)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(augment_mix_kernel, dim3(cdiv((int64_t)H * W, NT), Nb), dim3(NT), 0, st, (const uint8_t*)src,
                     (bf16_t*)dst, labels, partner, lam, box, ya, yb, lam_out, Nb, H, W, C, Cout, pad, flip, seed, mean, stdinv);
  return (int)hipGetLastError();
}
