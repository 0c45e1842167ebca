// The output side shared by the implicit-GEMM convolution kernels (conv_igemm.hip)
// and the one-pass conv backward kernels (conv3_bwd.hip, conv2_bwd.hip): launch geometry, the fused
// BatchNorm operands, the LDS-staged epilogue of one wave tile, and the host side the two one-pass
// entries share (block cap, BnBwd construction and its refusal, status + slab reduce).  Internal
// linkage (one copy per translation unit), everything __forceinline__.
#pragma once
#include "common.h"
#include "tile.h"

int kfa_wgrad_reduce_launch(const float* part, int splits, long total, void* grad, int grad_f32, int accumulate,
                            hipStream_t s);  // wgrad.hip

namespace {
using namespace tile;

#ifndef KFA_CONV_STORE_AUX
#define KFA_CONV_STORE_AUX 2  // output stores non-temporal (streamed; +1.7 % ResNet-50 vs 0, docs/kernels.md)
#endif

constexpr int BK = 64;
constexpr int kBnSlots = 64;  // must match batchnorm.hip kSlots (fused statistics land in its slots)

// Backward BatchNorm statistics fused into a dgrad epilogue: the dgrad output is
// dL/dy of a BatchNorm(+ReLU) whose input x / output y / batch mean are given;
// the epilogue accumulates sum(dz) and sum(dz * (x - mean)), dz = dy * (y > 0),
// into the BN slots (what bn_bwd_partial computes), so the BN backward skips
// that pass.  x == nullptr: forward statistics (sum, sum of squares) instead.
struct BnBwd {
  const bf16_t* x;
  const bf16_t* y;   // ReLU mask source (forward output), or nullptr: mask from x with ss
  const float* ss;   // the BN forward's [scale | shift] (used when relu && !y && !mb)
  const uint8_t* mb; // the BN forward's output ReLU bit mask (BN + residual; used when relu && !y)
  const float* mean;
  int relu;
  const uint8_t* emb;  // addend E masked by these ReLU bits (E = a block output's raw gradient), or nullptr
};

struct Geo {
  int Nb, H, W, C;   // gathered tensor T
  int P, Q;          // GEMM row space (m = nb*P*Q + p*Q + q)
  int R, S;          // taps
  int sa, ra, oa, ob;  // gather: ih = p*sa + r*ra + oa, iw = q*sa + s*ra + ob
  int M, N, K;       // GEMM sizes (K = R*S*C)
  int OH, OW, os, oph, opw, ldd;  // output pixel mapping / row stride (elements)
  unsigned t_bytes, b_bytes, d_bytes;  // buffer extents: out-of-range lanes read 0 / drop stores
};

// ---- host side of the one-pass backward entries (conv3_bwd.hip, conv2_bwd.hip) ----
// A BatchNorm with a ReLU whose backward statistics are asked for (x given) needs a mask source the
// epilogue takes (ss or bits): the entries refuse it with -3 before anything is launched.
inline bool bn_bwd_mask_missing(const bf16_t* x, int relu, const float* ss, const uint8_t* mb) {
  return x && relu && !ss && !mb;
}
inline BnBwd bn_bwd_operands(const bf16_t* x, const float* mean, int relu, const float* ss, const uint8_t* mb) {
  return BnBwd{x, nullptr, ss, mb, mean, relu, nullptr};
}
// persistent blocks = fp32 partial slabs: one per whole tile, capped at max_blocks, or (max_blocks <= 0)
// at per_cu blocks per CU -- only that form asks the device
inline int capped_blocks(long ntiles, int max_blocks, int per_cu) {
  const long cap = max_blocks > 0 ? max_blocks : (long)per_cu * kfa_cu_count();
  return (int)(ntiles < cap ? ntiles : cap);
}
// after the kernel launch: its status, then the slabs summed into the flat gradient
inline int reduce_slabs(const float* part, int blocks, long slab_floats, void* grad, int grad_f32, int accumulate,
                        hipStream_t s) {
  const int rc = kfa_status();
  if (rc) return rc;
  return kfa_wgrad_reduce_launch(part, blocks, slab_floats, grad, grad_f32, accumulate, s);
}

#ifndef KFA_CONV_EPI_LOAD_AUX
#define KFA_CONV_EPI_LOAD_AUX 2  // epilogue addend / BN-input loads non-temporal (read once; +0.2 %)
#endif
#ifndef KFA_CONV_LOAD_AUX
#define KFA_CONV_LOAD_AUX 0  // cache policy of the gathered activation operand's DMA (each element used by one tile column only)
#endif

// WM x WN waves, each owning TM x TN MFMA 16x16 tiles (wave tile 16TM x 16TN)
// (8 waves: 256 x 256 tiles of 128 x 64 per wave, one block per CU — half the
// operand bytes per MFMA of the 4-wave 128 x 128 tile; the epilogue then stages
// the wave tile in NHALF passes so it fits the one ring buffer it may use.)
// EPI: epilogue features compiled in (kEpiE addend, kEpiStats fused BN statistics,
// kEpiBnBwd backward statistics of the BN this dgrad feeds, kEpiEmb ReLU-bit-masked
// addend).  A feature's runtime pointer may still be null; features not compiled in
// cost no registers — the all-features build spilled (256 VGPRs) and serialised the
// main loop's LDS fragment reads on a reused register.
constexpr unsigned kEpiE = 1, kEpiStats = 2, kEpiBnBwd = 4, kEpiEmb = 8, kEpiYMask = 16, kEpiAll = 31;

struct EpiRes {  // buffer resources of the epilogue's output / addend / BN input / BN output
  __amdgpu_buffer_rsrc_t d, e, bx, by;
};

// Epilogue of one wave tile through LDS: MFMA leaves each lane 4 consecutive
// channels of one pixel (acc[ni][mi][r] = D(m = mw + 16 mi + fr, n = nw + 16 ni
// + 4 fq + r)); staging the wave's tile in LDS (XOR-swizzled 16-B chunks,
// conflict-free both ways) lets every lane store 16 B and a wave cover 128-B row
// segments, so the HBM writes of the memory-bound layers (K = 64..256) coalesce.
// NHALF staging passes over the wave's rows (1 for 64-row wave tiles; 4 for the
// 128-row ones, keeping the epilogue's in-flight loads at 48 VGPRs).  `stage`:
// this wave's 256 * (TM / NHALF) * TN staged elements; `first_barrier`: the
// first pass waits at a workgroup barrier before its LDS writes (the stage
// aliases an operand buffer other waves may still be reading).  Also: the
// residual-gradient addend (kEpiE, masked by ReLU bits with kEpiEmb) and the
// fused BatchNorm statistics (kEpiStats; kEpiBnBwd: backward statistics of the
// BN this dgrad feeds).  The accumulators are zeroed for the next tile.
template <int TM, int TN, int NHALF, unsigned EPI>
__device__ __forceinline__ void conv_epilogue(const Geo& g, floatx4 (&acc)[TN][TM], char* stage, bool first_barrier,
                                              int lane, int mw, int nw, int PQ, float rPQ, float rQ, bool lin_d,
                                              const bf16_t* E, float* stats, const BnBwd& bnb, const EpiRes& er) {
  constexpr int TMH = TM / NHALF;     // MFMA row tiles per pass
  constexpr int RB = 32 * TN;         // staged row bytes
  constexpr int CPR = 2 * TN;         // 16-B chunks per staged row
  constexpr int IT = (16 * TMH * CPR) / 64;  // 16-B row pieces per lane per pass
  const int fr = lane & 15, fq = lane >> 4;
  const int c = lane % CPR;
  const int n = nw + c * 8;
  float mu[8] = {0, 0, 0, 0, 0, 0, 0, 0}, msc[8], msf[8];
  constexpr bool kE = EPI & kEpiE, kST = EPI & kEpiStats, kBS = EPI & kEpiBnBwd, kEM = EPI & kEpiEmb;
  constexpr bool kYM = EPI & kEpiYMask;  // ReLU mask read from the BN output (else bits / recomputed from x)
  const bool bstat = kBS && kST && stats && bnb.x;
  const bool ymask = kYM && bnb.relu && bnb.y;       // mask from the output y
  const bool bmask = bnb.relu && !bnb.y && bnb.mb;   // from the output bit mask
  // else (relu) recomputed from x with the saved scale / shift
  if (bstat)
#pragma unroll
    for (int j = 0; j < 8; j++) {
      mu[j] = n + j < g.N ? bnb.mean[n + j] : 0.f;
      msc[j] = (bnb.relu && !ymask && !bmask && n + j < g.N) ? bnb.ss[n + j] : 0.f;
      msf[j] = (bnb.relu && !ymask && !bmask && n + j < g.N) ? bnb.ss[g.N + n + j] : 0.f;
    }
  float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // fused BN statistics
#pragma unroll
  for (int hh = 0; hh < NHALF; hh++) {
    // output offsets first, so the epilogue's global loads (residual-grad addend,
    // BN input / output for the fused backward statistics) are all in flight
    // while the tile is staged through LDS
    unsigned offs[IT];
#pragma unroll
    for (int it = 0; it < IT; it++) {
      const int m = mw + hh * TMH * 16 + it * (64 / CPR) + lane / CPR;
      unsigned orow;  // byte offset of output row m
      if (lin_d) {
        orow = (unsigned)m * (unsigned)g.ldd * 2u;
      } else {
        const int nb = fdiv(m, PQ, rPQ), rem = m - nb * PQ;
        const int p = fdiv(rem, g.Q, rQ), q = rem - p * g.Q;
        orow = (unsigned)((nb * g.OH + p * g.os + g.oph) * g.OW + (q * g.os + g.opw)) * (unsigned)g.ldd * 2u;
      }
      offs[it] = (m >= g.M || n >= g.N) ? kOOB : orow + (unsigned)n * 2u;
    }
    uint4 ev[IT], bx[IT], by[IT];
    unsigned mbits[IT], ebits[IT];
    if (kE && E)
#pragma unroll
      for (int it = 0; it < IT; it++) {
        ev[it] = bload16<KFA_CONV_EPI_LOAD_AUX>(er.e, offs[it]);
        if (kEM && bnb.emb) ebits[it] = offs[it] != kOOB ? (unsigned)bnb.emb[offs[it] >> 4] : 0u;
      }
    if (bstat)
#pragma unroll
      for (int it = 0; it < IT; it++) {
        bx[it] = bload16<KFA_CONV_EPI_LOAD_AUX>(er.bx, offs[it]);
        if (ymask) by[it] = bload16<KFA_CONV_EPI_LOAD_AUX>(er.by, offs[it]);
        if (bmask) mbits[it] = offs[it] != kOOB ? (unsigned)bnb.mb[offs[it] >> 4] : 0u;  // 8 bf16 = 16 B per bit byte
      }

    if (hh == 0 && first_barrier) lds_barrier();  // every wave is done reading the operand buffer under `stage`
    else lgkm_wait<0>();  // this wave read back its previous pass
#pragma unroll
    for (int mj = 0; mj < TMH; mj++)
#pragma unroll
      for (int ni = 0; ni < TN; ni++) {
        const int mi = hh * TMH + mj;
        const int row = mj * 16 + fr, col = ni * 16 + fq * 4;
        const uint2 o = make_uint2(pack2(acc[ni][mi][0], acc[ni][mi][1]), pack2(acc[ni][mi][2], acc[ni][mi][3]));
        *reinterpret_cast<uint2*>(stage + row * RB + (((col >> 3) ^ (row & (CPR - 1))) << 4) + (col & 7) * 2) = o;
      }
    lgkm_wait<0>();
#pragma unroll
    for (int it = 0; it < IT; it++) {
      const int r = it * (64 / CPR) + lane / CPR;
      const uint4 v = *reinterpret_cast<const uint4*>(stage + r * RB + ((c ^ (r & (CPR - 1))) << 4));
      const unsigned off = offs[it];
      uint4 o = v;
      if (kE && E) {  // wave-uniform branch
        float f[8], h[8];
        unpack8(v, f);
        unpack8(ev[it], h);
        if (kEM && bnb.emb) {  // residual gradient dz = dy * relu-mask, formed here instead of by the BN backward
#pragma unroll
          for (int j = 0; j < 8; j++) f[j] += ((ebits[it] >> j) & 1u) ? h[j] : 0.f;
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) f[j] += h[j];
        }
        o = pack8(f);
      }
      __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<decltype(__builtin_amdgcn_raw_buffer_load_b128(er.d, 0, 0, 0))*>(&o), er.d, off, 0, KFA_CONV_STORE_AUX);
      if (kST && stats && off != kOOB) {  // wave-uniform pointer test; per-lane row mask
        float f[8];
        unpack8(o, f);  // the bf16-rounded values the BatchNorm will see
        if (bstat) {    // backward statistics of the BN this dgrad feeds
          float xf[8];
          unpack8(bx[it], xf);
          if (ymask) {
            float yf[8];
            unpack8(by[it], yf);
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = yf[j] > 0.f ? f[j] : 0.f;
          } else if (bmask) {
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = ((mbits[it] >> j) & 1u) ? f[j] : 0.f;
          } else if (bnb.relu) {  // y = relu(fma(x, sc, sh)) exactly as bn_apply evaluated it
#pragma unroll
            for (int j = 0; j < 8; j++) f[j] = fmaf(xf[j], msc[j], msf[j]) > 0.f ? f[j] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 8; j++) { s1[j] += f[j]; s2[j] += f[j] * (xf[j] - mu[j]); }
        } else {
#pragma unroll
          for (int j = 0; j < 8; j++) { s1[j] += f[j]; s2[j] += f[j] * f[j]; }
        }
      }
    }
  }
  if (kST && stats) {
    // Butterfly-reduce over the lanes sharing channel chunk c = lane % CPR (xor
    // 8, 16, 32): every lane ends with its chunk's wave totals.  Lane L then
    // publishes channel (L % 8) * 8 + L / 8 — its own chunk, register L / 8
    // (a select chain, no shuffles) — so ONE 64-lane atomic instruction per
    // statistic covers the wave's 64 channels (CPR == 8: TN == 4).
    static_assert(CPR == 8, "fused BN statistics assume 64-channel wave tiles");
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1)
#pragma unroll
      for (int j = 0; j < 8; j++) { s1[j] += __shfl_xor(s1[j], o, 64); s2[j] += __shfl_xor(s2[j], o, 64); }
    const int jj = lane >> 3;
    float a = s1[0], b = s2[0];
#pragma unroll
    for (int j = 1; j < 8; j++) {
      a = jj == j ? s1[j] : a;
      b = jj == j ? s2[j] : b;
    }
    const int nc = n + jj;
    if (nc < g.N) {
      float* slot = stats + (long)(blockIdx.x % kBnSlots) * 2 * g.N;
      __hip_atomic_fetch_add(slot + nc, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(slot + g.N + nc, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#pragma unroll
  for (int i = 0; i < TN; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace
