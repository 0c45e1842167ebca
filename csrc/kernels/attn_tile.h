// Tile primitives shared by the attention kernels (attention.hip, attention_d128.hip):
// swizzled LDS images, 16x16x32 MFMA operand reads, the pair dropout hash and the
// register row operand of the packed kernels.  Everything is forceinline device code in
// an unnamed namespace: including it leaves each file's kernels as they were.
#pragma once

#include "common.h"

namespace {

typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

// [rows][64] images: chunk c of row r at c ^ m(r), m(r) = 2·((r>>1)&1) + 4·(((r>>2)^(r>>3))&1) + ((r>>3)&1).
// Conflict-free for the 16x16x32 row reads (ds_read_b128, 16-row groups) AND for
// both transposed-read row sets (8 consecutive rows; rows R..R+3 with R+8..R+11):
// within a parity the 4 rows' masks differ in bits 1-2, so the two logical
// chunks of a transposed read land in 8 distinct 16-B slots.  (The plain
// c ^ ((r>>1)&7) swizzle is 2-way on the transposed reads.)
__device__ __forceinline__ int off64(int row, int col) {
  const int m = (((row >> 1) & 1) << 1) | ((((row >> 2) ^ (row >> 3)) & 1) << 2) | ((row >> 3) & 1);
  return row * 128 + ((((col >> 3) ^ m) & 7) << 4) + (col & 7) * 2;
}
__device__ __forceinline__ int off128(int row, int col) {
  return row * 256 + ((((col >> 3) ^ row) & 15) << 4) + (col & 7) * 2;
}
template <int W>
__device__ __forceinline__ int ioff(int row, int col) {
  if constexpr (W == 64) return off64(row, col);
  else return off128(row, col);
}

// 16x16x32 operand: columns k0..k0+7 of `row`
template <int W>
__device__ __forceinline__ short8 rd_row(const char* img, int row, int k0) {
  return *reinterpret_cast<const short8*>(img + ioff<W>(row, k0));
}

// 16x16x32 operand from 8 consecutive ROWS: lane (g = lane>>4, i = lane&15) gets
// column cb + i of rows kb + 8g .. kb + 8g + 7 (two ds_read_b64_tr_b16)
template <int W>
__device__ __forceinline__ short8 rd_tr(const char* img, int kb, int cb, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const int col = cb + 4 * (i & 3), r0 = kb + 8 * g + (i >> 2);
  const v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + ioff<W>(r0, col)));
  const v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + ioff<W>(r0 + 4, col)));
  return short8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// D[i][j] += Σ_k A[i][k]·B[k][j]; lane l holds A[l&15][8(l>>4)+e], B[8(l>>4)+e][l&15],
// D[4(l>>4)+r][l&15]
__device__ __forceinline__ floatx4 mma(short8 a, short8 b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
  return make_uint2(pack2(a, b), pack2(c, d));
}

// rows ra..ra+3 and rb..rb+3 (any two 4-row groups) of column cb + (lane & 15):
// the 16x16x32 operand whose k index runs over a PERMUTED row order.  Used where
// the other operand comes straight from an MFMA result held in registers (lane
// = column, 4 consecutive rows per 16-row tile): k order is free in a dot
// product, so only the two operands have to agree on it.
template <int W>
__device__ __forceinline__ short8 rd_tr2(const char* img, int ra, int rb, int cb, int lane) {
  const int i = lane & 15;
  const int col = cb + 4 * (i & 3);
  const v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + ioff<W>(ra + (i >> 2), col)));
  const v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + ioff<W>(rb + (i >> 2), col)));
  return short8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

__device__ __forceinline__ short8 pack_pair(floatx4 x, floatx4 y) {
  const uint2 lo = pack4(x[0], x[1], x[2], x[3]), hi = pack4(y[0], y[1], y[2], y[3]);
  const uint4 u = make_uint4(lo.x, lo.y, hi.x, hi.y);
  return *reinterpret_cast<const short8*>(&u);
}

// Dropout of the attention probabilities (every attention kernel): ONE 32-bit
// counter hash per PAIR of scores (q, k) and (q, k + 16), k with bit 4 clear, whose
// 16-bit halves decide the two keeps: keep iff half >= t16 = round(p·2^16) (drop
// probability t16 / 2^16, kept values scaled by 2^16 / (2^16 − t16)).  Every lane
// layout holds both keys of a pair in one lane (key tiles kt and kt + 1 of 16),
// so a pair costs one hash — half the quarter-rate v_mul_lo_u32 work of a per-score
// hash, which was ~40 % of the forward's VALU cycles.
__device__ __forceinline__ uint32_t attn_pair_hash(uint64_t seed, uint64_t row, int S, int key_lo) {
  return drop_hash(seed, row * (uint64_t)S + (uint64_t)key_lo);
}
__device__ __forceinline__ bool keep_lo(uint32_t h, uint32_t t16) { return (h & 0xffffu) >= t16; }
__device__ __forceinline__ bool keep_hi(uint32_t h, uint32_t t16) { return (h >> 16) >= t16; }

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// score of a key past the sequence end (or above the causal diagonal), before the running max
constexpr float kMasked = -3.0e38f;
// the packed-varlen kernels are compiled without the packed fp32 VALU forms
#define KFA_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

// one 16x16x32 operand row piece straight from memory: 8 columns at src (+ bias)
// (· scale); a row that does not exist is zero and is not loaded
template <bool BIAS>
__device__ __forceinline__ short8 row_operand(const bf16_t* __restrict__ src, bool live, const float* __restrict__ bias,
                                              float scale) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (live) {
    v = *reinterpret_cast<const uint4*>(src);
    if constexpr (BIAS) {
      const float4 b0 = *reinterpret_cast<const float4*>(bias), b1 = *reinterpret_cast<const float4*>(bias + 4);
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      float f[8];
      unpack8(v, f);
#pragma unroll
      for (int e = 0; e < 8; e++) f[e] = (f[e] + bb[e]) * scale;
      v = pack8(f);
    }
  }
  return *reinterpret_cast<const short8*>(&v);
}

// key > query ? masked : x, as a bit select on the sign of query − key (no compare mask per element)
__device__ __forceinline__ float above_diag(int query, int key, float masked, float x) {
  const uint32_t m = (uint32_t)((query - key) >> 31);  // all ones: key > query
  return __uint_as_float((__float_as_uint(masked) & m) | (__float_as_uint(x) & ~m));
}

}  // namespace
