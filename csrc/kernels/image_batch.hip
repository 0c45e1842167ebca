// Input batch builder: one launch turns a uint8 image store into the network's
// input.  src [N][Hs][Ws][3] uint8 (NHWC, RGB) + a per-sample parameter table
// params [B][6] int32 = (index, y0, x0, h, w, flip)  ->  x [B][Ho][Wo][3] (the
// channels-last memory of a [B, 3, Ho, Wo] tensor) in bf16 or fp32, and
// y[b] = labels[index_b].  Gather, crop / pad, flip, resize, normalise, cast and
// layout in one pass: the source bytes are read once, the output written once.
//
// Per sample, by the box size:
//   direct   (h, w) == (Ho, Wo): out(i, j) = src(y0 + i, x0 + j'), j' = Wo-1-j under
//            flip; the box may overhang the image (pad-and-crop): a tap outside
//            [0, Hs) x [0, Ws) is pixel value 0 before normalisation.
//   resample otherwise: bilinear, align_corners = false, no antialias:
//            sy = (i + 0.5) h / Ho - 0.5 (exact, see tap()) clamped to [0, h-1], taps floor(sy) and
//            min(floor(sy) + 1, h-1) offset by y0 (same in x), flip applied after
//            resampling.  The box lies inside the image (the entry checks the
//            host copy of the table and refuses the launch otherwise).
// Value: (float(p) - mean_c) * inv_std_c, one subtract and one multiply in fp32
// (no contraction), rounded to nearest even for bf16.
//
// Memory: every byte offset into src is 64-bit.  Source loads are non-temporal
// (read once); output stores take the default policy (the stem reads the tensor
// right after).  Wo % 8 == 0: one thread per 8 output pixels = 3 x 16-B stores
// (bf16; 6 for fp32).  A direct-mode thread reads its 24 source bytes as 7
// address-aligned dwords; a dword that is not wholly inside the source ROW is
// assembled from byte loads of the in-row bytes only, so no load ever touches a
// byte of another image or outside the allocation, and the bytes beside the row
// read as the zero padding.  Resample taps and any other Wo use byte loads.
#include "common.h"

#pragma clang fp contract(off)

namespace {

struct ImgArgs {
  const uint8_t* src;
  const long* labels;
  const int* params;
  void* x;
  long* y;
  long N;
  int B, Hs, Ws, Ho, Wo;
  float mean[3], inv[3];
};

struct Box {
  long img;  // byte offset of image `index` in src
  int y0, x0, h, w;
  bool flip, direct;
};

__device__ __forceinline__ Box load_box(const ImgArgs& a, int b) {
  const int* p = a.params + (long)b * 6;
  Box r;
  long idx = p[0];
  idx = idx < 0 ? 0 : (idx >= a.N ? a.N - 1 : idx);  // the entry refused such a table; never index outside
  r.img = idx * a.Hs * a.Ws * 3;
  r.y0 = p[1];
  r.x0 = p[2];
  r.h = p[3];
  r.w = p[4];
  r.flip = p[5] != 0;
  r.direct = r.h == a.Ho && r.w == a.Wo;
  return r;
}

__device__ __forceinline__ uint32_t ldb(const uint8_t* p) { return (uint32_t)__builtin_nontemporal_load(p); }

// bilinear source coordinate of output position o over n source positions:
// s = (o + 0.5) n / no - 0.5 = ((2 o + 1) n - no) / (2 no), clamped to [0, n - 1].
// Taps t0 = floor(s), t1 = min(t0 + 1, n - 1) and the weight l = s - t0 of t1 come
// from the integer quotient and remainder, so the coordinate carries no rounding
// (in fp32 its error, ~no 2^-24, times a 255-step edge would exceed the output's
// own rounding at 224 outputs); l is rounded once.  (2 o + 1) n < 2^31 (the entry checks).
__device__ __forceinline__ void tap(int o, int n, int no, int& t0, int& t1, float& l) {
  const int num = (2 * o + 1) * n - no;
  const unsigned den = 2u * (unsigned)no;
  t0 = 0;
  l = 0.f;
  if (num > 0) {
    const unsigned q = (unsigned)num / den;
    t0 = (int)q;
    l = (float)((unsigned)num - q * den) / (float)den;
  }
  if (t0 >= n - 1) {
    t0 = n - 1;
    l = 0.f;
  }
  t1 = min(t0 + 1, n - 1);
}

// one resampled pixel: taps (ya, yb) x (xa, xb) are absolute image coordinates, clamped into the image
__device__ __forceinline__ void bilinear3(const ImgArgs& a, const Box& bx, int ya, int yb, float ly, int xa, int xb,
                                          float lx, float v[3]) {
  ya = min(max(ya, 0), a.Hs - 1);
  yb = min(max(yb, 0), a.Hs - 1);
  xa = min(max(xa, 0), a.Ws - 1);
  xb = min(max(xb, 0), a.Ws - 1);
  const uint8_t* ra = a.src + bx.img + (long)ya * a.Ws * 3;
  const uint8_t* rb = a.src + bx.img + (long)yb * a.Ws * 3;
  uint32_t p00[3], p01[3], p10[3], p11[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    p00[c] = ldb(ra + (long)xa * 3 + c);
    p01[c] = ldb(ra + (long)xb * 3 + c);
    p10[c] = ldb(rb + (long)xa * 3 + c);
    p11[c] = ldb(rb + (long)xb * 3 + c);
  }
  const float wy0 = 1.f - ly, wx0 = 1.f - lx;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float top = wx0 * (float)p00[c] + lx * (float)p01[c];
    const float bot = wx0 * (float)p10[c] + lx * (float)p11[c];
    v[c] = ((wy0 * top + ly * bot) - a.mean[c]) * a.inv[c];
  }
}

// 24 bytes starting at byte offset `at` from src (which may lie outside the row),
// as 6 dwords; bytes outside the row [lo, hi) read 0.  Loads are address-aligned
// dwords wholly inside the row, or single in-row bytes.
__device__ __forceinline__ void load24(const uint8_t* src, long at, long lo, long hi, uint32_t out[6]) {
  const uint32_t mis = (uint32_t)((unsigned long)(uintptr_t)src + (unsigned long)at) & 3u;
  const long wa = at - (long)mis;
  uint32_t w[7];
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const long o = wa + 4 * k;
    uint32_t v = 0;
    if (o >= lo && o + 4 <= hi) {
      v = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + o));
    } else if (o + 4 > lo && o < hi) {
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (o + t >= lo && o + t < hi) v |= ldb(src + o + t) << (8 * t);
    }
    w[k] = v;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) out[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], mis);
}

// Wo % 8 == 0 and a 16-B aligned x: one thread per 8 consecutive output pixels of a row.
template <bool F32>
__global__ __launch_bounds__(256) void image_batch_vec(ImgArgs a) {
  const unsigned gw = (unsigned)a.Wo / 8;
  const unsigned total = (unsigned)a.B * a.Ho * gw;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int jg = (int)(t % gw);
  unsigned q = t / gw;
  const int i = (int)(q % (unsigned)a.Ho);
  const int b = (int)(q / (unsigned)a.Ho);
  const Box bx = load_box(a, b);
  if (i == 0 && jg == 0) a.y[b] = a.labels[bx.img / ((long)a.Hs * a.Ws * 3)];
  const int j0 = jg * 8;
  float v[24];  // output order: pixel j0 + k, channel c at v[3 k + c]
  if (bx.direct) {
    const int y = bx.y0 + i;
    const int xs = bx.x0 + (bx.flip ? a.Wo - 8 - j0 : j0);  // first of 8 consecutive source pixels
    long lo = 0, hi = 0;                                     // an out-of-image row: empty, reads as zeros
    if (y >= 0 && y < a.Hs) {
      lo = bx.img + (long)y * a.Ws * 3;
      hi = lo + (long)a.Ws * 3;
    }
    const long at = bx.img + ((long)y * a.Ws + xs) * 3;
    uint32_t d[6];
    load24(a.src, at, lo, hi, d);
    float s[24];
#pragma unroll
    for (int e = 0; e < 24; e++) s[e] = (((float)((d[e >> 2] >> ((e & 3) * 8)) & 0xffu)) - a.mean[e % 3]) * a.inv[e % 3];
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) v[3 * k + c] = bx.flip ? s[3 * (7 - k) + c] : s[3 * k + c];
  } else {
    int ya, yb;
    float ly;
    tap(i, bx.h, a.Ho, ya, yb, ly);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int j = j0 + k;
      int xa, xb;
      float lx;
      tap(bx.flip ? a.Wo - 1 - j : j, bx.w, a.Wo, xa, xb, lx);
      bilinear3(a, bx, bx.y0 + ya, bx.y0 + yb, ly, bx.x0 + xa, bx.x0 + xb, lx, v + 3 * k);
    }
  }
  const long o = (long)t * 24;  // element offset: ((b Ho + i) Wo + j0) 3
  if (F32) {
    float4* dst = reinterpret_cast<float4*>(reinterpret_cast<float*>(a.x) + o);
#pragma unroll
    for (int k = 0; k < 6; k++) dst[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  } else {
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(a.x) + o);
    dst[0] = pack8(v);
    dst[1] = pack8(v + 8);
    dst[2] = pack8(v + 16);
  }
}

// any Wo: one thread per output pixel, byte loads, element stores
template <bool F32>
__global__ __launch_bounds__(256) void image_batch_scalar(ImgArgs a) {
  const unsigned total = (unsigned)a.B * a.Ho * a.Wo;
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = (int)(t % (unsigned)a.Wo);
  unsigned q = t / (unsigned)a.Wo;
  const int i = (int)(q % (unsigned)a.Ho);
  const int b = (int)(q / (unsigned)a.Ho);
  const Box bx = load_box(a, b);
  if (i == 0 && j == 0) a.y[b] = a.labels[bx.img / ((long)a.Hs * a.Ws * 3)];
  float v[3];
  if (bx.direct) {
    const int y = bx.y0 + i, x = bx.x0 + (bx.flip ? a.Wo - 1 - j : j);
    const bool in = y >= 0 && y < a.Hs && x >= 0 && x < a.Ws;
    const uint8_t* p = a.src + bx.img + ((long)(in ? y : 0) * a.Ws + (in ? x : 0)) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = ((float)(in ? ldb(p + c) : 0u) - a.mean[c]) * a.inv[c];
  } else {
    int ya, yb, xa, xb;
    float ly, lx;
    tap(i, bx.h, a.Ho, ya, yb, ly);
    tap(bx.flip ? a.Wo - 1 - j : j, bx.w, a.Wo, xa, xb, lx);
    bilinear3(a, bx, bx.y0 + ya, bx.y0 + yb, ly, bx.x0 + xa, bx.x0 + xb, lx, v);
  }
  const long o = (long)t * 3;
  if (F32) {
    float* dst = reinterpret_cast<float*>(a.x) + o;
    dst[0] = v[0];
    dst[1] = v[1];
    dst[2] = v[2];
  } else {
    bf16_t* dst = reinterpret_cast<bf16_t*>(a.x) + o;
    dst[0] = (bf16_t)f2bf(v[0]);
    dst[1] = (bf16_t)f2bf(v[1]);
    dst[2] = (bf16_t)f2bf(v[2]);
  }
}

}  // namespace

// Status: 0 ok (or the HIP launch error); -1 bad sizes / pointers; -2 a table row
// with an index outside [0, N), a non-positive box or an origin beyond +-2^24;
// -3 a resample box that does not lie inside the image.  params_host is the host
// copy of the table the device reads at params: it is checked here, before the
// launch, because the kernel trusts it for every source address.
KFA_API int kfa_image_batch(const uint8_t* src, const long* labels, const int* params, const int* params_host,
                            void* x, long* y, long N, int B, int Hs, int Ws, int Ho, int Wo, float mean0, float mean1,
                            float mean2, float inv0, float inv1, float inv2, int out_fp32, hipStream_t st) {
  if (!src || !labels || !params || !params_host || !x || !y) return -1;
  if (N <= 0 || B <= 0 || Hs <= 0 || Ws <= 0 || Ho <= 0 || Wo <= 0) return -1;
  if ((long)B * Ho * Wo >= (1L << 31) || (long)Hs * Ws * 3 >= (1L << 31)) return -1;
  for (int b = 0; b < B; b++) {
    const int* p = params_host + (long)b * 6;
    const long y0 = p[1], x0 = p[2], h = p[3], w = p[4];
    if (p[0] < 0 || p[0] >= N || h <= 0 || w <= 0) return -2;
    if (y0 < -(1L << 24) || y0 > (1L << 24) || x0 < -(1L << 24) || x0 > (1L << 24)) return -2;
    const bool direct = h == Ho && w == Wo;
    if (!direct && (y0 < 0 || x0 < 0 || y0 + h > Hs || x0 + w > Ws)) return -3;
    if (!direct && (2L * Ho * h >= (1L << 31) || 2L * Wo * w >= (1L << 31))) return -1;  // tap()'s 32-bit numerator
  }
  ImgArgs a{src, labels, params, x, y, N, B, Hs, Ws, Ho, Wo, {mean0, mean1, mean2}, {inv0, inv1, inv2}};
  const bool vec = Wo % 8 == 0 && ((uintptr_t)x & 15) == 0;
  const long work = vec ? (long)B * Ho * (Wo / 8) : (long)B * Ho * Wo;
  const dim3 grid((unsigned)((work + 255) / 256)), block(256);
  if (vec && out_fp32)
    hipLaunchKernelGGL(image_batch_vec<true>, grid, block, 0, st, a);
  else if (vec)
    hipLaunchKernelGGL(image_batch_vec<false>, grid, block, 0, st, a);
  else if (out_fp32)
    hipLaunchKernelGGL(image_batch_scalar<true>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(image_batch_scalar<false>, grid, block, 0, st, a);
  return kfa_status();
}
