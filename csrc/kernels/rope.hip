// Rotary position embeddings (RoPE) for the packed attention layers: one bandwidth-bound
// pass that rotates the Q and K columns of the QKV projection in place, between the QKV
// GEMM and the attention kernel, and its transpose on the Q / K columns of dqkv after the
// attention backward.  The attention kernels are untouched (docs/kernels.md, "Rotary
// position embeddings": why the rotation is not fused into them).
//
// x [T, W] bf16, the first nrot heads of a row (Q | K, contiguous from column 0) are
// rotated; V columns and the unowned rows cu[B] .. T-1 are never read or written.  With
// the rotate-half pairing (Llama / NeoX), for j < D/2 and (cos, sin) = table[pos, j],
// pos = row - cu[sequence]:
//   forward   v = x + bias:   y[j] = v[j] cos - v[j+D/2] sin     y[j+D/2] = v[j+D/2] cos + v[j] sin
//   inverse   (no bias):      g[j] = dy[j] cos + dy[j+D/2] sin   g[j+D/2] = dy[j+D/2] cos - dy[j] sin
// fp32 math, round-to-nearest-even bf16 stores (pack2).  The table is fp32
// [max_position, D/2, 2], built on the host in fp64, so no sincosf runs here; the kernel
// trusts pos < max_position (the host checks max_seqlen against it).
//
// Work split: a workgroup owns R = 32 consecutive rows of one sequence (1-D grid of
// B * ceil(max_seqlen / R) blocks from host integers, as the packed attention kernels), so
// pos = block start + row offset with no search of cu; a block past its sequence's end
// exits at once.  One lane owns 16-byte chunk c of the low half and chunk c of the high
// half of a head — D/16 lanes per row, both elements of every pair lane-local, at
// D = 128 eight lanes cover a full 128-byte line in each half.  The lane's 8 cos + 8 sin
// stay in 16 registers across the loop over the nrot heads (table traffic = 1/nrot of the
// data traffic); the head loop issues RU heads' loads before the first use.  No LDS, no
// MFMA, default cache policy on the stores (the next kernel reads them).
#include "common.h"

namespace {

constexpr int ROPE_R = 32;   // rows of one sequence per workgroup
constexpr int ROPE_RU = 4;   // heads whose 16-byte loads are in flight together

template <bool INV>
__device__ __forceinline__ void rope_rot8(const float lo[8], const float hi[8], const float cs[8], const float sn[8],
                                          float ylo[8], float yhi[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (INV) {
      ylo[i] = fmaf(hi[i], sn[i], lo[i] * cs[i]);
      yhi[i] = fmaf(-lo[i], sn[i], hi[i] * cs[i]);
    } else {
      ylo[i] = fmaf(-hi[i], sn[i], lo[i] * cs[i]);
      yhi[i] = fmaf(lo[i], sn[i], hi[i] * cs[i]);
    }
  }
}

__device__ __forceinline__ void rope_add_bias8(float v[8], const float* __restrict__ b) {
  const float4 b0 = *reinterpret_cast<const float4*>(b);
  const float4 b1 = *reinterpret_cast<const float4*>(b + 4);
  v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
  v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
}

template <int D, bool INV>
__global__ __launch_bounds__(ROPE_R* D / 16) void rope_qk_kernel(bf16_t* __restrict__ x, const float* __restrict__ bias,
                                                                 float* __restrict__ bias_out,
                                                                 const int* __restrict__ cu,
                                                                 const float* __restrict__ table, int nblk, int W,
                                                                 int nrot) {
  constexpr int LPR = D / 16;  // lanes per row
  const int tid = threadIdx.x;
  if (!INV && bias_out != nullptr && blockIdx.x == 0) {
    // the bias the attention kernel adds afterwards: the rotated columns already hold theirs
    for (int i = tid; i < W; i += ROPE_R * LPR) bias_out[i] = (i < nrot * D || bias == nullptr) ? 0.f : bias[i];
  }
  const int seq = blockIdx.x / nblk;
  const int pos = (blockIdx.x - seq * nblk) * ROPE_R + tid / LPR;
  const int s0 = cu[seq];
  if (pos >= cu[seq + 1] - s0) return;  // whole blocks past the sequence's end, and the tail rows of its last block
  const int c = tid % LPR;

  float cs[8], sn[8];
  {
    const float4* tp = reinterpret_cast<const float4*>(table + ((long)pos * (D / 2) + 8 * c) * 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 t = tp[i];
      cs[2 * i] = t.x; sn[2 * i] = t.y; cs[2 * i + 1] = t.z; sn[2 * i + 1] = t.w;
    }
  }
  bf16_t* row = x + (long)(s0 + pos) * W + 8 * c;
  const bool has_bias = !INV && bias != nullptr;

  int h = 0;
  for (; h + ROPE_RU <= nrot; h += ROPE_RU) {
    uint4 lo[ROPE_RU], hi[ROPE_RU];
#pragma unroll
    for (int u = 0; u < ROPE_RU; ++u) {
      lo[u] = *reinterpret_cast<const uint4*>(row + (h + u) * D);
      hi[u] = *reinterpret_cast<const uint4*>(row + (h + u) * D + D / 2);
    }
#pragma unroll
    for (int u = 0; u < ROPE_RU; ++u) {
      float a[8], b[8], ya[8], yb[8];
      unpack8(lo[u], a);
      unpack8(hi[u], b);
      if (has_bias) {
        rope_add_bias8(a, bias + (h + u) * D + 8 * c);
        rope_add_bias8(b, bias + (h + u) * D + D / 2 + 8 * c);
      }
      rope_rot8<INV>(a, b, cs, sn, ya, yb);
      *reinterpret_cast<uint4*>(row + (h + u) * D) = pack8(ya);
      *reinterpret_cast<uint4*>(row + (h + u) * D + D / 2) = pack8(yb);
    }
  }
  for (; h < nrot; ++h) {
    float a[8], b[8], ya[8], yb[8];
    unpack8(*reinterpret_cast<const uint4*>(row + h * D), a);
    unpack8(*reinterpret_cast<const uint4*>(row + h * D + D / 2), b);
    if (has_bias) {
      rope_add_bias8(a, bias + h * D + 8 * c);
      rope_add_bias8(b, bias + h * D + D / 2 + 8 * c);
    }
    rope_rot8<INV>(a, b, cs, sn, ya, yb);
    *reinterpret_cast<uint4*>(row + h * D) = pack8(ya);
    *reinterpret_cast<uint4*>(row + h * D + D / 2) = pack8(yb);
  }
}

template <int D>
void rope_launch(void* x, const float* bias, float* bias_out, const int* cu, const float* table, int B, int nblk, int W,
                 int nrot, bool inverse, hipStream_t st) {
  const dim3 grid((unsigned)((long)B * nblk)), block(ROPE_R * D / 16);
  if (inverse)
    hipLaunchKernelGGL((rope_qk_kernel<D, true>), grid, block, 0, st, (bf16_t*)x, (const float*)nullptr,
                       (float*)nullptr, cu, table, nblk, W, nrot);
  else
    hipLaunchKernelGGL((rope_qk_kernel<D, false>), grid, block, 0, st, (bf16_t*)x, bias, bias_out, cu, table, nblk, W,
                       nrot);
}

}  // namespace

// x [T, W] bf16, rotated in place on its first nrot heads of d columns (see the header);
// bias (fp32 [W], nullable, forward only) is added before the rotation; bias_out (fp32 [W],
// nullable, forward only) receives 0 on the nrot*d rotated columns and bias elsewhere,
// written by the workgroup of (block 0, sequence 0).  cu: the B + 1 row offsets of the packed
// batch, every length <= max_seqlen <= the table's positions.  -1 without a launch for a
// shape the kernel does not take.
KFA_API int kfa_rope_qk(void* x, const float* bias, float* bias_out, const int* cu, const float* table, int B, int T,
                        int max_seqlen, int W, int nrot, int d, int inverse, hipStream_t st) {
  if (!x || !cu || !table || B <= 0 || T <= 0 || max_seqlen < 1 || (d != 64 && d != 128) || nrot < 1 || W % 8 != 0 ||
      (long)nrot * d > (long)W)
    return -1;
  const int nblk = kfa_ceil_div(max_seqlen, ROPE_R);
  if ((long)B * nblk >= (1L << 31)) return -1;
  if (d == 64)
    rope_launch<64>(x, bias, bias_out, cu, table, B, nblk, W, nrot, inverse != 0, st);
  else
    rope_launch<128>(x, bias, bias_out, cu, table, B, nblk, W, nrot, inverse != 0, st);
  return kfa_status();
}
