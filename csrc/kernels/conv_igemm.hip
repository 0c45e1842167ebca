// Implicit-GEMM convolution on MFMA (bf16 in, fp32 accumulate), NHWC.
// SURVEY §2.6 K7 (ResNet-50 conv2d fwd + dgrad) and K1 (plain GEMM = 1x1 conv).
//
// One kernel computes  D[m][n] = sum_k A[m][k] * B[n][k]  (+ E[m][n])  where
// (with bnb.emb: + E[m][n] * bit(emb, m*N + n), the residual gradient of a
// BN + residual + ReLU output formed from its raw gradient and ReLU bit mask)
//   A = implicit im2col of an NHWC tensor T[Nb][H][W][C]:
//         m = (nb, p, q) in [Nb][P][Q],  k = (r, s, c) in [R][S][C]
//         A[m][k] = T[nb][p*sa + r*ra + oa][q*sa + s*ra + ob][c]   (0 outside)
//   B = [N][K] row-major bf16 (K contiguous) — conv weights in [Cout][R][S][Cin]
//   D = bf16 rows, row m written at pixel (nb, p*os + oph, q*os + opw) of an
//       [Nb][OH][OW][ldd] tensor.
// Forward conv:   sa = stride, ra = +1, oa = -pad, os = 1.
// Dgrad stride 1: T = dY, ra = -1, oa = +pad, B = W transposed to [Cin][R][S][Cout].
// Dgrad stride 2: one launch per output parity class (ph, pw) over its tap subset
//                 (os = 2), B = the class's tap-subset weights (see conv.py).
//
// Tiling for CDNA4: 256 threads = 4 waves, each wave owns a 64x64 output tile
// (4x4 MFMA 16x16x32 bf16 tiles, 64 fp32 accumulator VGPRs).  Block tiles
// 128x128 (2x2 waves) or 256x64 (4x1, for Cout = 64 layers).  BK = 64 = one
// (r, s) tap slice (C % 64 == 0).  Global->register prefetch of tile k+1 is
// issued before the MFMAs of tile k (T14) — across tile boundaries too: the
// blocks are persistent (2 per CU) and sweep an XCD-local tile range, so the
// next tile's first slice loads under the current tile's last MFMAs and
// epilogue.  LDS is double-buffered (one barrier
// per k-tile) and XOR-swizzled (chunk ^= (row>>1)&7) so the 16-lane groups of
// each ds_read_b128 hit 16 distinct 16-B slots.  Operand roles are chosen so
// each lane's 4 accumulator rows are 4 CONSECUTIVE output channels (8-B stores).
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "tile.h"
#include "conv_epilogue.h"  // Geo, BnBwd, EpiRes, conv_epilogue (shared with conv3_bwd.hip)

namespace {
using namespace tile;

// BatchNorm-apply + ReLU prologue (PRO): T is a BatchNorm's RAW input x and the
// A operand is relu(x * scale[c] + shift[c]) (bf16, rounded exactly as bn_apply
// rounds it), applied on the register path between the global load and the LDS
// store; padding taps stay 0.  The blocks of tile column 0 also write the
// normalised value of every centre-tap slice to y (which then covers each input
// pixel once — stride 1, P == H, Q == W, host-checked), so the backward's weight
// gradient reads y as before and the BatchNorm's own apply pass is gone.
struct Pro {
  const float* ss;  // [scale | shift], 2C floats
  bf16_t* y;        // normalised activation (same layout as T), or nullptr
};

template <int WM, int WN, int TM, int TN, unsigned EPI, bool PRO = false>
__global__ __launch_bounds__(64 * WM * WN, 2) void conv_igemm_kernel(const bf16_t* __restrict__ T,
                                                                     const bf16_t* __restrict__ B,
                                                                     bf16_t* __restrict__ D, const bf16_t* __restrict__ E,
                                                                     const bf16_t* __restrict__ Z,
                                                                     float* __restrict__ stats, BnBwd bnb, Geo g,
                                                                     Pro pro = Pro{nullptr, nullptr}) {
  constexpr int NW = WM * WN, RPP = 8 * NW;  // waves; tile rows per staging pass (8 per wave)
  constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
  constexpr int AR = BM / RPP, BR = BN / RPP;  // 16-B chunks per thread per k-tile
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  bf16_t* As = smem;                  // [2][BM][BK]
  bf16_t* Bs = smem + 2 * BM * BK;    // [2][BN][BK]
  float* ssl = reinterpret_cast<float*>(smem + 2 * (BM + BN) * BK);  // PRO: [scale | shift] (2C floats)

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: LDS-DMA bases in SGPRs
  const int wm = wave % WM, wn = wave / WM;
  const int ntn = (g.N + BN - 1) / BN;
  const int ntiles = ((g.M + BM - 1) / BM) * ntn;

  // Persistent blocks.  XCD-aware assignment (T1): the blocks that share an
  // XCD (b % 8) sweep one contiguous range of tiles, so tiles in flight on an
  // XCD share A/B panels in its L2.
  const int nwg = gridDim.x;
  const int G = nwg < 8 ? nwg : 8;                        // XCD groups that have blocks
  const int xcd = blockIdx.x % G, slot = blockIdx.x / G;
  const int nslot = (nwg - xcd + G - 1) / G;               // blocks in this group
  const int t_lo = (int)((long)ntiles * xcd / G), t_hi = (int)((long)ntiles * (xcd + 1) / G);
  const int my_tiles = t_hi - t_lo > slot ? (t_hi - t_lo - slot + nslot - 1) / nslot : 0;
  auto tile_of = [&](int i) { return t_lo + slot + i * nslot; };

  const int kc = tid & 7;
  const int rbase = tid >> 3;  // 0..RPP-1
  const int PQ = g.P * g.Q;
  const float rPQ = 1.f / (float)PQ, rQ = 1.f / (float)g.Q;
  // pointwise fast paths: A row m is T[m] (1x1 / stride 1 / no pad) and/or D row m is D[m]
  const bool lin_a = g.R == 1 && g.S == 1 && g.sa == 1 && g.oa == 0 && g.ob == 0 && g.H == g.P && g.W == g.Q;
  const bool lin_d = g.os == 1 && g.oph == 0 && g.opw == 0 && g.OH == g.P && g.OW == g.Q;
  int a_hb[AR], a_wb[AR], a_vo[AR];  // a_vo: byte offset of the row at tap (0, 0) + swizzled chunk (< 2^31, host-checked)
  unsigned b_off[BR];
  const __amdgpu_buffer_rsrc_t rT = rsrc(T, g.t_bytes), rB = rsrc(B, g.b_bytes), rD = rsrc(D, g.d_bytes);
  const __amdgpu_buffer_rsrc_t rE = rsrc(E ? E : D, E ? g.d_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rBX = rsrc(bnb.x ? bnb.x : D, bnb.x ? g.d_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rBY = rsrc(bnb.y ? bnb.y : D, bnb.y ? g.d_bytes : 0u);
  auto setup = [&](int tile) {
    const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
#pragma unroll
    for (int i = 0; i < AR; i++) {
      const int m = m0 + rbase + RPP * i;
      const int cs = (kc ^ swz_chunk(i * RPP + rbase)) * 8;  // this lane's swizzled source chunk
      if (m < g.M && lin_a) {
        a_hb[i] = 0;
        a_wb[i] = 0;
        a_vo[i] = (m * g.C + cs) * 2;
      } else if (m < g.M) {  // a_vo: the row's offset at tap (0, 0) (may lie outside the image)
        const int nb = fdiv(m, PQ, rPQ), rem = m - nb * PQ;
        const int p = fdiv(rem, g.Q, rQ), q = rem - p * g.Q;
        a_hb[i] = p * g.sa + g.oa;
        a_wb[i] = q * g.sa + g.ob;
        a_vo[i] = ((nb * g.H * g.W + a_hb[i] * g.W + a_wb[i]) * g.C + cs) * 2;
      } else {
        a_hb[i] = -(1 << 28);  // forces out-of-range
        a_wb[i] = 0;
        a_vo[i] = (int)kOOB;
      }
    }
#pragma unroll
    for (int i = 0; i < BR; i++) {
      const int n = n0 + rbase + RPP * i;
      const int cs = (kc ^ swz_chunk(i * RPP + rbase)) * 8;
      b_off[i] = n < g.N ? (unsigned)(n * g.K + cs) * 2u : kOOB;
    }
  };

  // Operand staging: LDS-DMA (buf_dma16, tile.h).  Each wave-instruction
  // writes 1 KiB = 8 tile rows lane-linearly; the XOR swizzle is applied on the
  // per-lane SOURCE address (rule 21); padding taps / tails read as zero (range check).
  // No staging VGPRs, no ds_write pass; waits are counted by hand.
  const int nk = g.K / BK;
  const int total = my_tiles * nk;
  int setup_tile = -1;
  const int l8 = lane >> 3, pos = lane & 7;
  // DMA sources as 32-bit buffer offsets (buffer_load ... lds): the per-lane part
  // is fixed per tile (the swizzled chunk included), the k-slice's channel offset
  // goes in the SCALAR offset, padding taps / tails get an offset past the
  // buffer (read as 0 by the range check).  1x1 stride-1 layers then issue
  // their DMAs with no per-step vector math at all.
  // issue() runs for st = 0, 1, 2, ... in order: the (tile, k-slice, channel
  // offset, tap) of the next slice is carried incrementally (wave-uniform) instead
  // of four scalar divisions per k-step
  int nx_ti = 0, nx_kt = 0, nx_c0 = 0, nx_r = 0, nx_s = 0;
  // PRO register-path state of the slice in flight: raw A chunks, their source
  // offsets (for the y write), valid-tap bits, the slice's scalar offset / channel base
  uint4 pr_a[PRO ? AR : 1];
  int pr_vo[PRO ? AR : 1];
  unsigned pr_ok = 0;
  int pr_soff = 0, pr_ch = 0;
  bool pr_y = false;
  const int pr_cs = (kc ^ ((rbase >> 1) & 7)) * 8;  // this lane's source chunk (the same for every i: RPP % 16 == 0)
  auto ti_col0 = [&](int ti) { return tile_of(ti) % ntn == 0; };
  const __amdgpu_buffer_rsrc_t rY = rsrc(pro.y ? pro.y : D, pro.y ? g.t_bytes : 0u);
  auto issue = [&](int st, int buf) {
    (void)st;
    const int ti = nx_ti, k0 = nx_kt * BK, c0 = nx_c0;
    if (ti != setup_tile) { setup(tile_of(ti)); setup_tile = ti; }
    const int dh = nx_r * g.ra, dw = nx_s * g.ra;
    const int ta_off = (dh * g.W + dw) * g.C * 2;  // the tap's offset: one scalar add per DMA, no per-lane multiply
    nx_c0 += BK;  // advance to the next slice: BK channels of one tap, or BK / C whole taps (C < BK)
    while (nx_c0 >= g.C) {
      nx_c0 -= g.C;
      if (++nx_s == g.S) { nx_s = 0; nx_r++; }
    }
    if (++nx_kt == nk) { nx_kt = 0; nx_ti++; nx_c0 = 0; nx_r = 0; nx_s = 0; }
    if constexpr (PRO) {  // register path: loads now, normalised + stored to LDS by pro_store
      pr_soff = (lin_a ? k0 : c0) * 2;
      pr_ch = lin_a ? k0 : c0;
      pr_y = pro.y && (ti_col0(ti) && (lin_a || (dh + g.oa == 0 && dw + g.ob == 0)));
      pr_ok = 0;
#pragma unroll
      for (int i = 0; i < AR; i++) {
        int vo = a_vo[i];
        if (!lin_a) {
          const int ih = a_hb[i] + dh, iw = a_wb[i] + dw;
          const bool ok = (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
          vo = ok ? a_vo[i] + ta_off : (int)kOOB;
          pr_ok |= ok ? (1u << i) : 0u;
        } else {
          pr_ok |= 1u << i;
        }
        pr_vo[i] = vo;
        auto v = __builtin_amdgcn_raw_buffer_load_b128(rT, (unsigned)vo, (unsigned)pr_soff, KFA_CONV_LOAD_AUX);
        pr_a[i] = *reinterpret_cast<uint4*>(&v);
      }
    } else if (lin_a) {  // the whole offset but the slice's is fixed per tile (a_vo, setup)
#pragma unroll
      for (int i = 0; i < AR; i++)
        buf_dma16<KFA_CONV_LOAD_AUX>(rT, As + buf * BM * BK + (i * RPP + wave * 8) * BK, a_vo[i], k0 * 2);
    } else {
#pragma unroll
      for (int i = 0; i < AR; i++) {
        const int ih = a_hb[i] + dh, iw = a_wb[i] + dw;
        const bool ok = (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
        const int vo = ok ? a_vo[i] + ta_off : (int)kOOB;  // selects, no branch
        buf_dma16<KFA_CONV_LOAD_AUX>(rT, As + buf * BM * BK + (i * RPP + wave * 8) * BK, vo, c0 * 2);
      }
    }
#pragma unroll
    for (int i = 0; i < BR; i++)
      buf_dma16(rB, Bs + buf * BN * BK + (i * RPP + wave * 8) * BK, (int)b_off[i], k0 * 2);
  };
  floatx4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  // Fragment reads ahead of the MFMAs that use them: k-half 0's A and B plus
  // k-half 1's B fragments are issued before k-half 0's MFMAs, k-half 1's A
  // fragments between the two MFMA groups, each group preceded by a counted
  // lgkmcnt.  The reads are inline asm: with compiler-visible ds_reads hipcc
  // re-used a few fragment registers and waited lgkmcnt(0) between small MFMA
  // groups (its wait pass does not count these reads exactly), exposing the LDS
  // latency several times per k-step.  sched_barrier after each wait keeps the
  // MFMAs behind it (rule 18).  TM + 2 TN <= 15 reads in flight (4-bit counter);
  // the 8-wave 256x256 variant keeps the plain form.
  auto compute = [&](int buf) {
    const bf16_t* Ab = As + buf * BM * BK;
    const bf16_t* Bb = Bs + buf * BN * BK;
    short8 af[2][TM], bf[2][TN];
    auto mfma = [&](int ks) {
#pragma unroll
      for (int ni = 0; ni < TN; ni++)
#pragma unroll
        for (int mi = 0; mi < TM; mi++)
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][ni], af[ks][mi], acc[ni][mi], 0, 0, 0);
    };
    auto rd = [&](const bf16_t* p) {  // (lds_rd16<0> prints an `offset:0`: the same encoding, other text)
      short8 v;
      asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr(p)) : "memory");
      return v;
    };
    if constexpr (TM + 2 * TN <= 15) {
#pragma unroll
      for (int i = 0; i < TN; i++) bf[0][i] = rd(Bb + swz128(wn * TN * 16 + i * 16 + fr, fq));
#pragma unroll
      for (int i = 0; i < TM; i++) af[0][i] = rd(Ab + swz128(wm * TM * 16 + i * 16 + fr, fq));
#pragma unroll
      for (int i = 0; i < TN; i++) bf[1][i] = rd(Bb + swz128(wn * TN * 16 + i * 16 + fr, 4 + fq));
      lgkm_wait<TN>();  // k-half 0's fragments landed; k-half 1's B reads may still be in flight
      __builtin_amdgcn_sched_barrier(0);
      mfma(0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TM; i++) af[1][i] = rd(Ab + swz128(wm * TM * 16 + i * 16 + fr, 4 + fq));
      lgkm_wait<0>();
      __builtin_amdgcn_sched_barrier(0);
      mfma(1);
    } else if constexpr (PRO) {
      // 8-wave 256x256 tiles with the BatchNorm prologue: one k-half's 12 reads, wait,
      // its MFMAs.  Inline asm: with compiler-visible reads hipcc waited vmcnt(0) — the
      // NEXT slice's register loads and DMAs, issued at the top of the step — before
      // every step's first read (the plain variants keep the compiler's form below: no
      // such wait there, and its counted lgkmcnt interleave)
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
#pragma unroll
        for (int i = 0; i < TM; i++) af[ks][i] = rd(Ab + swz128(wm * TM * 16 + i * 16 + fr, ks * 4 + fq));
#pragma unroll
        for (int i = 0; i < TN; i++) bf[ks][i] = rd(Bb + swz128(wn * TN * 16 + i * 16 + fr, ks * 4 + fq));
        lgkm_wait<0>();
        __builtin_amdgcn_sched_barrier(0);
        mfma(ks);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
#pragma unroll
        for (int i = 0; i < TM; i++)
          af[ks][i] = *reinterpret_cast<const short8*>(Ab + swz128(wm * TM * 16 + i * 16 + fr, ks * 4 + fq));
#pragma unroll
        for (int i = 0; i < TN; i++)
          bf[ks][i] = *reinterpret_cast<const short8*>(Bb + swz128(wn * TN * 16 + i * 16 + fr, ks * 4 + fq));
        mfma(ks);
      }
    }
  };
  // Epilogue: conv_epilogue (below the kernel) over this wave's tile, staged in
  // ring buffer `buf` once every wave is done reading it (its first pass's barrier)
  constexpr int NHALF = NW == 4 ? 1 : TM / 2;
  constexpr int WT = 256 * (TM / NHALF) * TN;  // staged elements per wave per pass
  static_assert(NW * WT <= (BM + BN) * BK, "conv epilogue stage must fit one ring buffer");
  const EpiRes er{rD, rE, rBX, rBY};
  auto epilogue = [&](int tile, int buf) {
    const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
    const int e = wave * WT;
    char* stage = reinterpret_cast<char*>(e < BM * BK ? As + buf * BM * BK + e : Bs + buf * BN * BK + (e - BM * BK));
    conv_epilogue<TM, TN, NHALF, EPI>(g, acc, stage, true, lane, m0 + wm * TM * 16, n0 + wn * TN * 16, PQ, rPQ, rQ,
                                      lin_d, E, stats, bnb, er);
  };

  // PRO: the slice's A chunks landed -> relu(x * sc + sh) (0 on padding taps) into
  // LDS `buf` at the positions the LDS-DMA would have filled; centre-tap slices of
  // tile column 0 also go to y.
  auto pro_store = [&](int buf) {
    if constexpr (PRO) {
      const int c = pr_ch + pr_cs;
      float sc[8], sh[8];
      {
        // inline-asm reads: compiler-visible ones got an s_waitcnt vmcnt(0) (draining the
        // next slice's B DMAs) in front of them
        typedef __attribute__((ext_vector_type(4))) float f32x4;
        f32x4 v[4];
        const unsigned la = lds_addr(ssl + c), lb = lds_addr(ssl + g.C + c);
        asm volatile("ds_read_b128 %0, %1" : "=v"(v[0]) : "v"(la) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(v[1]) : "v"(la) : "memory");
        asm volatile("ds_read_b128 %0, %1" : "=v"(v[2]) : "v"(lb) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:16" : "=v"(v[3]) : "v"(lb) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) :: "memory");
        const float4 a0 = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]), a1 = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
        const float4 b0 = make_float4(v[2][0], v[2][1], v[2][2], v[2][3]), b1 = make_float4(v[3][0], v[3][1], v[3][2], v[3][3]);
        sc[0] = a0.x; sc[1] = a0.y; sc[2] = a0.z; sc[3] = a0.w; sc[4] = a1.x; sc[5] = a1.y; sc[6] = a1.z; sc[7] = a1.w;
        sh[0] = b0.x; sh[1] = b0.y; sh[2] = b0.z; sh[3] = b0.w; sh[4] = b1.x; sh[5] = b1.y; sh[6] = b1.z; sh[7] = b1.w;
      }
#pragma unroll
      for (int i = 0; i < AR; i++) {
        float f[8];
        unpack8(pr_a[i], f);
        const bool ok = (pr_ok >> i) & 1u;
#pragma unroll
        for (int j = 0; j < 8; j++) f[j] = ok ? fmaxf(fmaf(f[j], sc[j], sh[j]), 0.f) : 0.f;
        uint4 o = pack8(f);
        // (inline asm: a compiler-visible LDS store got an s_waitcnt vmcnt(0) for the DMAs in flight)
        lds_wr16(lds_addr(As + buf * BM * BK + (i * RPP + wave * 8) * BK + lane * 8), o);
        if (pr_y) {
          __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<decltype(__builtin_amdgcn_raw_buffer_load_b128(rY, 0, 0, 0))*>(&o),
                                                 rY, (unsigned)pr_vo[i], (unsigned)pr_soff, 0);
          // wait states for the store's data VGPRs before the next VALU write: hipcc's hazard
          // pass misses this store-data hazard across the branch join inside the k-loop (the
          // next chunk's first VALU op overwrote the 2nd data dword: tests/test_conv_gpu.py)
          asm volatile("s_nop 4" ::: "memory");
        }
      }
    }
  };
  auto pro_wait = [&]() {  // this slice's A loads retired (its BR B-operand DMAs may still be in flight)
    vm_wait<(BR == 4 || BR == 2) ? BR : 0>();
  };

  if (nk == 0) {  // no taps reach these outputs (strided dgrad parity class): D = 0 (+ E)
    for (int i = 0; i < my_tiles; i++) {
      epilogue(tile_of(i), 0);
      lds_barrier();
    }
    return;
  }
  if constexpr (PRO) {
    for (int i = tid; i < 2 * g.C; i += 64 * NW) ssl[i] = pro.ss[i];
    __syncthreads();
  }
  issue(0, 0);
  if constexpr (PRO) {
    if (total > 0) {
      pro_wait();
      pro_store(0);
      lgkm_wait<0>();  // the loop's first barrier publishes them
    }
  }
  for (int st = 0; st < total; st++) {
    const int buf = st & 1;
    if (st + 1 < total) {
      issue(st + 1, buf ^ 1);
      // slice st landed (and older stores retired); slice st+1 stays in flight
      if constexpr (AR + BR == 8) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
      else if constexpr (AR + BR == 6) asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
    compute(buf);
    if constexpr (PRO) {
      if (st + 1 < total) {
        pro_wait();
        pro_store(buf ^ 1);
      }
    }
    if ((st + 1) % nk == 0) epilogue(tile_of(st / nk), buf);
    lds_barrier();  // every wave is done reading `buf` before slice st+2 is DMA'd into it
  }
}

// ---------------------------------------------------------------------------
// Ping-pong implicit GEMM (256 x 256 tiles): gemm_pp_kernel's two-wave-group
// schedule (gemm.hip, "Ping-pong 256x256 kernel") with the A operand gathered
// from the NHWC activation as in conv_igemm_kernel.  512 threads = two wave
// GROUPS (waves 0-3: tile rows 0-127, waves 4-7: rows 128-255; wave w owns the
// 128 x 64 tile at (w >> 2, w & 3)), one block per CU, BK = 64 = one tap's 64
// channels.  Each k-tile is four 16 KB pieces ordered by first use
//   A0: A rows {0-63, 128-191}   B0: B rows {64c + 0..31}
//   B1: B rows {64c + 32..63}    A1: A rows {64-127, 192-255}
// consumed in four phases of 16 MFMAs per wave; group 1 runs one barrier
// behind group 0, so on every SIMD one wave's MFMAs run under the other's LDS
// fragment reads and DMA issue, and four pieces (8 DMAs per lane) stay in
// flight across the barriers (never vmcnt(0) in the main loop).  Compared
// with the 4-wave 128 x 128 conv_igemm_kernel (two blocks per CU, ONE k-step
// of prefetch, 19-24 % MFMA busy at 3.6-4.4 VALU per MFMA,
// profiles/pmc/r4_resnet50_step.md): 128 x 64 wave tiles read 0.375 LDS
// fragments per MFMA instead of 0.5, the tile moves half the L2 -> LDS bytes
// per FLOP, and the load latency is covered by ~a k-tile of work.
// Gather: the A piece of k-tile kt reads tap (r, s), channels c0..c0+63, at
// per-lane 32-bit offsets (rows past M and padding taps go past the buffer
// and read 0); the tap walk is carried incrementally (wave-uniform) — the A0
// piece of a k-tile advances it, its A1 piece (issued three phases later, no
// other A0 in between) reuses it.  Epilogue: conv_epilogue (LDS-staged 16-B
// stores + fused addend / BN statistics), 4 staging passes per 128-row wave tile.
#ifndef KFA_CONV_PP_NHALF
#define KFA_CONV_PP_NHALF 4  // epilogue staging passes over the 128-row wave tile (8 KB of LDS per wave per pass at 2)
#endif
// WR wave-rows x WC = 8 / WR wave-columns of 128 x 64 wave tiles: WR = 2 is the
// 256 x 256 tile above (one wave-row per group); WR = 4 the 512 x 128 tile of the
// 128-channel layers (two wave-rows per group, 2 x 2 waves), the SAME wave tile and
// phase schedule with A pieces of 256 rows (32 KB, 4 DMAs per lane) and B pieces of
// 64 rows (8 KB, 1 DMA): 2 x 80 KB = the whole 160 KB of LDS, 104 FLOP per operand
// byte (the 128 x 128 tile: 64).
template <int WR>
__device__ __forceinline__ void pp_vm_wait(int n) {  // s_waitcnt vmcnt(n), n in [0, 2*WR + 8/WR]
  switch (n) {
    KFA_VMW(0) KFA_VMW(1) KFA_VMW(2) KFA_VMW(3) KFA_VMW(4) KFA_VMW(5) KFA_VMW(6) KFA_VMW(7) KFA_VMW(8) KFA_VMW(9)
    default: vm_wait<10>(); break;
  }
}

template <unsigned EPI, int WR = 2>
__global__ __launch_bounds__(512, 1) void conv_pp_kernel(const bf16_t* __restrict__ T, const bf16_t* __restrict__ B,
                                                         bf16_t* __restrict__ D, const bf16_t* __restrict__ E,
                                                         float* __restrict__ stats, BnBwd bnb, Geo g) {
  constexpr int TM = 8, TN = 4, WC = 8 / WR, MT = 128 * WR, NT = 64 * WC;
  constexpr int AP = WR * 64 * 128, BP = WC * 32 * 128;  // A / B piece bytes (64-deep rows of 128 B)
  constexpr int KTB = 2 * (AP + BP);                     // one k-tile buffer: [A0][B0][B1][A1]
  constexpr int OFF[4] = {0, AP, AP + BP, AP + 2 * BP};
  constexpr int NDMA[4] = {WR, WC / 2, WC / 2, WR};      // DMA instructions per lane of each piece
  constexpr int STEADY = 2 * WR + WC;                    // DMAs of any four consecutive phases
  __shared__ __attribute__((aligned(16))) char smem[2 * KTB];  // 128 KB (WR 2) / 160 KB (WR 4)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = WR == 2 ? wave >> 2 : ((wave >> 2) << 1) | ((wave >> 1) & 1);  // group = wave >> 2
  const int wc = wave & (WC - 1);
  // T1 XCD remap + grouped raster (as gemm_pp_kernel): the blocks of one XCD take
  // consecutive tiles, GM row panels wide
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, x8 = bid & 7;
  const int wg = (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + (bid >> 3);
  const int ntn = (g.N + NT - 1) / NT, ntm = (g.M + MT - 1) / MT;
  constexpr int GM = 4;
  const int grp = wg / (GM * ntn), gm0 = grp * GM, gmn = min(GM, ntm - gm0), rem = wg - grp * GM * ntn;
  const int m0 = (gm0 + rem % gmn) * MT, n0 = (rem / gmn) * NT;

  const __amdgpu_buffer_rsrc_t rT = rsrc(T, g.t_bytes), rB = rsrc(B, g.b_bytes), rD = rsrc(D, g.d_bytes);
  const int PQ = g.P * g.Q;
  const float rPQ = 1.f / (float)PQ, rQ = 1.f / (float)g.Q;
  const bool lin_a = g.R == 1 && g.S == 1 && g.sa == 1 && g.oa == 0 && g.ob == 0 && g.H == g.P && g.W == g.Q;
  const bool lin_d = g.os == 1 && g.oph == 0 && g.opw == 0 && g.OH == g.P && g.OW == g.Q;
  // DMA plan: instruction j of wave w fills piece rows j*64 + w*8 + lane/8,
  // physical chunk lane&7 <- logical chunk (lane&7) ^ ((row >> 1) & 7).
  // A piece h, instruction j: wave-row j's rows h*64 + [0, 64);  B piece h,
  // instruction j: wave-columns 2j, 2j+1's columns h*32 + [0, 32).
  const int prow = wave * 8 + (lane >> 3);
  const int lc = (lane & 7) ^ swz_chunk(prow);
  int a_hb[2][WR], a_wb[2][WR], a_vo[2][WR];  // [h: A0 / A1][j]
  int b_vo[2][WC / 2];                        // [h: B0 / B1][j]
#pragma unroll
  for (int h = 0; h < 2; h++) {
#pragma unroll
    for (int j = 0; j < WR; j++) {
      const int m = m0 + j * 128 + h * 64 + prow;
      if (m < g.M && lin_a) {
        a_hb[h][j] = 0;
        a_wb[h][j] = 0;
        a_vo[h][j] = (m * g.C + lc * 8) * 2;
      } else if (m < g.M) {  // a_vo: the row's offset at tap (0, 0) (may lie outside the image)
        const int nb = fdiv(m, PQ, rPQ), rm = m - nb * PQ;
        const int p = fdiv(rm, g.Q, rQ), q = rm - p * g.Q;
        a_hb[h][j] = p * g.sa + g.oa;
        a_wb[h][j] = q * g.sa + g.ob;
        a_vo[h][j] = ((nb * g.H * g.W + a_hb[h][j] * g.W + a_wb[h][j]) * g.C + lc * 8) * 2;
      } else {
        a_hb[h][j] = -(1 << 28);  // forces out-of-range
        a_wb[h][j] = 0;
        a_vo[h][j] = (int)kOOB;
      }
    }
#pragma unroll
    for (int j = 0; j < WC / 2; j++) {
      const int n = n0 + (2 * j + (prow >> 5)) * 64 + h * 32 + (prow & 31);
      b_vo[h][j] = n < g.N ? (n * g.K + lc * 8) * 2 : (int)kOOB;
    }
  }
  const int nk = g.K / BK;
  const int plast = 4 * nk - 7;  // last phase that issues a piece
  // tap walk of the A pieces (wave-uniform): next k-tile's (channel offset, r, s)
  int tw_c0 = 0, tw_r = 0, tw_s = 0;
  int ta_dh = 0, ta_dw = 0, ta_off = 0, ta_soff = 0;  // the tap of the last A0 piece issued
  auto issue = [&](int P, auto pc, auto steady) __attribute__((always_inline)) {
    constexpr int p = decltype(pc)::value;
    const int kt = (P + 6) >> 2;
    if (decltype(steady)::value || kt < nk) {
      char* dst = smem + (kt & 1) * KTB + OFF[p] + wave * 8 * 128;
      if constexpr (p == 0 || p == 3) {
        constexpr int h = p == 3;
        if constexpr (h == 0) {  // A0 of k-tile kt: advance the tap walk
          ta_dh = tw_r * g.ra;
          ta_dw = tw_s * g.ra;
          ta_off = (ta_dh * g.W + ta_dw) * g.C * 2;
          ta_soff = (lin_a ? kt * BK : tw_c0) * 2;
          tw_c0 += BK;
          if (tw_c0 >= g.C) {
            tw_c0 = 0;
            if (++tw_s == g.S) { tw_s = 0; tw_r++; }
          }
        }
#pragma unroll
        for (int j = 0; j < WR; j++) {
          int vo = a_vo[h][j];
          if (!lin_a) {  // selects, no branch: the tap offset is one scalar add
            const int ih = a_hb[h][j] + ta_dh, iw = a_wb[h][j] + ta_dw;
            const bool ok = (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W;
            vo = ok ? vo + ta_off : (int)kOOB;
          }
          buf_dma16<KFA_CONV_LOAD_AUX>(rT, dst + j * 64 * 128, vo, ta_soff);
        }
      } else {
        constexpr int h = p == 2;
#pragma unroll
        for (int j = 0; j < WC / 2; j++)
          buf_dma16(rB, dst + j * 64 * 128, b_vo[h][j], kt * BK * 2);
      }
    }
  };
  auto retire = [&](int P, auto steady) __attribute__((always_inline)) {
    if constexpr (decltype(steady)::value) {
      pp_vm_wait<WR>(STEADY);
    } else {  // keep the pieces of phases [P - 3, min(P, plast)] in flight
      int n = 0;
#pragma unroll
      for (int d = 0; d < 4; d++) {
        const int q = P - d;
        if (q <= plast) n += NDMA[(q + 2) & 3];  // phase q issues piece (q + 2) & 3
      }
      pp_vm_wait<WR>(n);
    }
  };

  // this lane's fragment read offsets in a piece: row fr, logical chunk 4 ks + fq
  const int fr = lane & 15, fq = lane >> 4;
  const int ro0 = fr * 128 + ((fq ^ (fr >> 1)) << 4), ro1 = fr * 128 + (((4 + fq) ^ (fr >> 1)) << 4);
  floatx4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  short8 a[4][2], b0[2][2], b1[2][2];

  // prologue: pieces of phases -6..-1 (A0 B0 B1 A1 of k-tile 0, A0 B0 of k-tile 1)
  issue(-6, std::integral_constant<int, 0>{}, std::false_type{});
  issue(-5, std::integral_constant<int, 1>{}, std::false_type{});
  issue(-4, std::integral_constant<int, 2>{}, std::false_type{});
  issue(-3, std::integral_constant<int, 3>{}, std::false_type{});
  issue(-2, std::integral_constant<int, 0>{}, std::false_type{});
  issue(-1, std::integral_constant<int, 1>{}, std::false_type{});
  retire(-1, std::false_type{});
  asm volatile("s_barrier" ::: "memory");
  if (wave >> 2) asm volatile("s_barrier" ::: "memory");  // group 1 runs one barrier behind

  auto mfma_q = [&](short8 (&bb)[2][2], int mh, int nh) __attribute__((always_inline)) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
#pragma unroll
      for (int ni = 0; ni < 2; ni++)
#pragma unroll
        for (int mi = 0; mi < 4; mi++)
          acc[nh * 2 + ni][mh * 4 + mi] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(bb[ni][ks], a[mi][ks], acc[nh * 2 + ni][mh * 4 + mi], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  auto rd = [&](const char* p) -> short8 { return *reinterpret_cast<const short8*>(p); };

  // one k-tile = four phases (st: std::true_type when every phase of k-tile u
  // issues a piece, i.e. u + 2 < nk)
  auto ktile = [&](int u, auto st) __attribute__((always_inline)) {
    const char* buf = smem + (u & 1) * KTB;
    const int P = 4 * u;
    {  // s0: A0 + B0
      const char* pa = buf + OFF[0] + wr * 64 * 128;
      const char* pb = buf + OFF[1] + wc * 32 * 128;
#pragma unroll
      for (int ni = 0; ni < 2; ni++) {
        b0[ni][0] = rd(pb + ni * 16 * 128 + ro0);
        b0[ni][1] = rd(pb + ni * 16 * 128 + ro1);
      }
#pragma unroll
      for (int mi = 0; mi < 4; mi++) {
        a[mi][0] = rd(pa + mi * 16 * 128 + ro0);
        a[mi][1] = rd(pa + mi * 16 * 128 + ro1);
      }
      issue(P, std::integral_constant<int, 2>{}, st);
      retire(P, st);
      asm volatile("s_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_q(b0, 0, 0);
      asm volatile("s_barrier" ::: "memory");
    }
    {  // s1: B1
      const char* pb = buf + OFF[2] + wc * 32 * 128;
#pragma unroll
      for (int ni = 0; ni < 2; ni++) {
        b1[ni][0] = rd(pb + ni * 16 * 128 + ro0);
        b1[ni][1] = rd(pb + ni * 16 * 128 + ro1);
      }
      issue(P + 1, std::integral_constant<int, 3>{}, st);
      retire(P + 1, st);
      asm volatile("s_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_q(b1, 0, 1);
      asm volatile("s_barrier" ::: "memory");
    }
    {  // s2: A1
      const char* pa = buf + OFF[3] + wr * 64 * 128;
#pragma unroll
      for (int mi = 0; mi < 4; mi++) {
        a[mi][0] = rd(pa + mi * 16 * 128 + ro0);
        a[mi][1] = rd(pa + mi * 16 * 128 + ro1);
      }
      issue(P + 2, std::integral_constant<int, 0>{}, st);
      retire(P + 2, st);
      asm volatile("s_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_q(b1, 1, 1);
      asm volatile("s_barrier" ::: "memory");
    }
    {  // s3: registers only
      issue(P + 3, std::integral_constant<int, 1>{}, st);
      retire(P + 3, st);
      asm volatile("s_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
      mfma_q(b0, 1, 0);
      asm volatile("s_barrier" ::: "memory");
    }
  };
  int u = 0;
  for (; u + 2 < nk; u++) ktile(u, std::true_type{});
  for (; u < nk; u++) ktile(u, std::false_type{});
  if (!(wave >> 2)) asm volatile("s_barrier" ::: "memory");  // both groups at the same barrier count: the ring is idle
  const EpiRes er{rD, rsrc(E ? E : D, E ? g.d_bytes : 0u), rsrc(bnb.x ? bnb.x : D, bnb.x ? g.d_bytes : 0u),
                  rsrc(bnb.y ? bnb.y : D, bnb.y ? g.d_bytes : 0u)};
  conv_epilogue<TM, TN, KFA_CONV_PP_NHALF, EPI>(g, acc, smem + wave * (256 * (TM / KFA_CONV_PP_NHALF) * TN) * 2, false,
                                                lane, m0 + wr * 128, n0 + wc * 64, PQ, rPQ, rQ, lin_d, E, stats, bnb,
                                                er);
}

// ---------------------------------------------------------------------------
// Halo-staged implicit GEMM: stride-1 3x3 'same' convs with C = 64 / 128 (forward
// and the stride-1 dgrad: ra = +-1).  conv_igemm_kernel moves every input pixel
// L2 -> LDS once per tap (9x); the nine taps of a linear tile of BM output pixels
// m0 .. m0+BM-1 read the input pixels m0-(W+1) .. m0+BM-1+(W+1), so this kernel
// stages that run ONCE per tile (HR = BM + 2(W+1) rows, 1.23-1.45x the tile) and
// tap (r, s)'s A fragment of tile row i is LDS row i + (W+1) + dh*W + dw.
// Image: C/64 sub-images of [HRP][128 B] rows, chunk ^= halo_swz(row) keyed on
// the LDS row's own index.  Pixels before the tensor / past its end stage as zero
// (buffer range check); a tap that leaves the image (row edge, top / bottom row,
// neighbouring image) is zeroed at fragment time: each lane keeps a 9-bit validity
// mask per M sub-tile (computed once per tile) and an invalid lane reads a zero
// row (the image's padding) instead — one select on the LDS address, no branch.
// The weights stream through a ring of NS slots, NS - 1 k-tiles ahead, with ONE
// barrier per k-tile: slice st + NS - 1 is issued right after step st's barrier,
// into the slot step st - 1 read.  k-tiles (tap-major, 64 channels each) and their
// two k = 32 halves run in conv_igemm_kernel's order on the same MFMA, so every
// output element's fp32 accumulation sequence — and the output — is bit-identical.
// Two blocks per CU: one block's halo fetch and epilogue run under the other's
// MFMAs.  The epilogue stage aliases the halo.
//
// halo_swz: each 16-lane group of a ds_read_b128 fragment read covers rows
// {0-3, 12-15} at chunk c and rows {4-11} at chunk c ^ 1 (or the reverse) of 16
// consecutive rows: per row parity that is four consecutive row pairs with one
// chunk and four with the other, so the pair index mod 4, XORed into chunk bits
// 2:1, gives 16 distinct 16-B slots at ANY row shift (swz_chunk's 8-value key is
// conflict-free only for 16-aligned fragments: 24 % conflict cycles on the shifted
// reads, profiles/conv3x3_narrow.md).
__device__ __forceinline__ int halo_swz(int row) { return ((row >> 1) & 3) << 1; }

template <int WM, int WN, int TM, int TN, int NS, unsigned EPI>
__global__ __launch_bounds__(64 * WM * WN, 2) void conv_halo_kernel(const bf16_t* __restrict__ T,
                                                                    const bf16_t* __restrict__ B,
                                                                    bf16_t* __restrict__ D, float* __restrict__ stats,
                                                                    BnBwd bnb, Geo g, int HRP) {
  constexpr int NW = WM * WN, RPP = 8 * NW;
  constexpr int BM = WM * TM * 16, BN = WN * TN * 16, BR = BN / RPP;
  static_assert(NW == 4 && (BR == 2 || BR == 4), "halo kernel: 4 waves, 64- or 128-wide N tiles");
  extern __shared__ __attribute__((aligned(16))) bf16_t smem[];
  const int CH = g.C / BK;       // 64-channel sub-images (1 or 2)
  const int HW1 = g.W + 1;
  const int HR = BM + 2 * HW1;   // staged rows (HRP > HR: padded to whole rounds of 4 x 8-row DMA pieces)
  char* halo = reinterpret_cast<char*>(smem);  // [CH][HRP][128 B]; rows HR.. stage as zeros
  bf16_t* Bs = reinterpret_cast<bf16_t*>(halo + CH * HRP * 128);  // [NS][BN][BK]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = wave / WM;
  const int ntn = (g.N + BN - 1) / BN;
  const int ntiles = ((g.M + BM - 1) / BM) * ntn;
  // persistent blocks over XCD-local tile ranges (as conv_igemm_kernel)
  const int nwg = gridDim.x;
  const int G = nwg < 8 ? nwg : 8;
  const int xcd = blockIdx.x % G, slot = blockIdx.x / G;
  const int nslot = (nwg - xcd + G - 1) / G;
  const int t_lo = (int)((long)ntiles * xcd / G), t_hi = (int)((long)ntiles * (xcd + 1) / G);
  const int my_tiles = t_hi - t_lo > slot ? (t_hi - t_lo - slot + nslot - 1) / nslot : 0;
  auto tile_of = [&](int i) { return t_lo + slot + i * nslot; };
  if (my_tiles == 0) return;

  const int kc = tid & 7, rbase = tid >> 3;
  const int l8 = lane >> 3, pos = lane & 7;
  const int fr = lane & 15, fq = lane >> 4;
  const int PQ = g.P * g.Q;
  const float rPQ = 1.f / (float)PQ, rQ = 1.f / (float)g.Q;
  const __amdgpu_buffer_rsrc_t rT = rsrc(T, g.t_bytes), rB = rsrc(B, g.b_bytes), rD = rsrc(D, g.d_bytes);
  const __amdgpu_buffer_rsrc_t rBX = rsrc(bnb.x ? bnb.x : D, bnb.x ? g.d_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rBY = rsrc(bnb.y ? bnb.y : D, bnb.y ? g.d_bytes : 0u);
  const EpiRes er{rD, rsrc(D, 0u), rBX, rBY};
  const int nk = 9 * CH;
  const int total = my_tiles * nk;

  // weight ring: slice (tile, k-tile) -> slot, carried incrementally in issue order
  unsigned b_off[BR];
  int setup_tile = -1, nx_ti = 0, nx_kt = 0;
  auto issue_b = [&](int buf) {
    if (nx_ti != setup_tile) {
      const int n0 = (tile_of(nx_ti) % ntn) * BN;
#pragma unroll
      for (int i = 0; i < BR; i++) {
        const int n = n0 + rbase + RPP * i;
        const int cs = (kc ^ swz_chunk(i * RPP + rbase)) * 8;
        b_off[i] = n < g.N ? (unsigned)(n * g.K + cs) * 2u : kOOB;
      }
      setup_tile = nx_ti;
    }
#pragma unroll
    for (int i = 0; i < BR; i++)
      buf_dma16(rB, Bs + buf * BN * BK + (i * RPP + wave * 8) * BK, (int)b_off[i], nx_kt * BK * 2);
    if (++nx_kt == nk) { nx_kt = 0; nx_ti++; }
  };

  // halo of one tile: 1-KiB pieces (8 rows x 128 B) dealt round-robin to the waves,
  // CH * HRP / 32 per wave (the same count on every wave: counted vmcnt waits);
  // and this lane's tap-validity masks, one per M sub-tile
  unsigned amask[TM];
  const int npw = CH * HRP / 32;
  auto stage = [&](int tile) {
    const int m0 = (tile / ntn) * BM;
    for (int jj = 0; jj < npw; jj++) {
      const int j = jj * 4 + wave;
      const int h = j * 8 >= HRP ? 1 : 0;
      const int row = j * 8 - h * HRP + l8;
      const int pix = m0 - HW1 + row;
      const bool ok = row < HR && (unsigned)pix < (unsigned)g.M;
      const int vo = ok ? (pix * g.C + h * BK + ((pos ^ halo_swz(row)) << 3)) * 2 : (int)kOOB;
      buf_dma16<KFA_CONV_LOAD_AUX>(rT, halo + j * 1024, vo, 0);
    }
#pragma unroll
    for (int mi = 0; mi < TM; mi++) {
      const int m = m0 + wm * TM * 16 + mi * 16 + fr;
      const int nb = fdiv(m, PQ, rPQ), rem = m - nb * PQ;
      const int p = fdiv(rem, g.Q, rQ), q = rem - p * g.Q;
      unsigned mk = 0;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const bool ok = (unsigned)(p + r * g.ra + g.oa) < (unsigned)g.H && (unsigned)(q + s * g.ra + g.ob) < (unsigned)g.W;
          mk |= ok ? 1u << (r * 3 + s) : 0u;
        }
      amask[mi] = mk;
    }
  };

  floatx4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; i++)
#pragma unroll
    for (int j = 0; j < TM; j++) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  const unsigned halo_la = lds_addr(halo);
  const unsigned zero_la = halo_la + (unsigned)(((CH - 1) * HRP + HR) * 128 + fq * 16);  // padding row, restaged per tile
  int c_r = 0, c_s = 0, c_h = 0;  // the k-tile compute() runs next: tap (c_r, c_s), sub-image c_h
  // fragment reads ahead of the MFMAs, counted lgkmcnt, as conv_igemm_kernel's 4-wave form
  auto compute = [&](int buf) {
    const bf16_t* Bb = Bs + buf * BN * BK;
    const int row0 = wm * TM * 16 + fr + HW1 + (c_r * g.ra + g.oa) * g.W + (c_s * g.ra + g.ob);
    const int x = halo_swz(row0);  // rows row0 + 16 mi share it
    const unsigned base = halo_la + (unsigned)((c_h * HRP + row0) * 128);
    const unsigned a0 = base + (unsigned)((fq ^ x) << 4), a1 = base + (unsigned)(((4 + fq) ^ x) << 4);
    const unsigned bit = 1u << (c_r * 3 + c_s);
    if (++c_h == CH) {
      c_h = 0;
      if (++c_s == 3) { c_s = 0; if (++c_r == 3) c_r = 0; }
    }
    short8 af[2][TM], bf[2][TN];
    auto mfma = [&](int ks) {
#pragma unroll
      for (int ni = 0; ni < TN; ni++)
#pragma unroll
        for (int mi = 0; mi < TM; mi++)
          acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ks][ni], af[ks][mi], acc[ni][mi], 0, 0, 0);
    };
    auto rda = [&](unsigned la) {
      short8 v;
      asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(la) : "memory");
      return v;
    };
    auto rd = [&](const bf16_t* p) { return rda(lds_addr(p)); };
#pragma unroll
    for (int i = 0; i < TN; i++) bf[0][i] = rd(Bb + swz128(wn * TN * 16 + i * 16 + fr, fq));
#pragma unroll
    for (int i = 0; i < TM; i++) af[0][i] = rda((amask[i] & bit) ? a0 + i * 2048 : zero_la);
#pragma unroll
    for (int i = 0; i < TN; i++) bf[1][i] = rd(Bb + swz128(wn * TN * 16 + i * 16 + fr, 4 + fq));
    lgkm_wait<TN>();
    __builtin_amdgcn_sched_barrier(0);
    mfma(0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TM; i++) af[1][i] = rda((amask[i] & bit) ? a1 + i * 2048 : zero_la);
    lgkm_wait<0>();
    __builtin_amdgcn_sched_barrier(0);
    mfma(1);
  };
  constexpr int WT = 256 * TM * TN;  // staged elements per wave (one pass)
  auto epilogue = [&](int tile) {
    const int m0 = (tile / ntn) * BM, n0 = (tile % ntn) * BN;
    conv_epilogue<TM, TN, 1, EPI>(g, acc, halo + wave * WT * 2, true, lane, m0 + wm * TM * 16, n0 + wn * TN * 16, PQ,
                                  rPQ, rQ, true, nullptr, stats, bnb, er);
  };

  stage(tile_of(0));
#pragma unroll
  for (int i = 0; i < NS - 1; i++)
    if (i < total) issue_b(i);
  int kt = 0, ti = 0, buf = 0, nbuf = NS - 1;
  for (int st = 0; st < total; st++) {
    // slice st landed — and, at a tile's first step, its halo (nothing younger is in flight
    // then: the slices ahead were issued before it); up to NS - 2 slices ahead stay in flight
    if (kt == 0 || NS == 2 || st + 1 >= total) vm_wait<0>();
    else vm_wait<(NS - 2) * BR>();
    asm volatile("s_barrier" ::: "memory");  // ... for every wave, which is also done reading slot `nbuf` (step st-1)
    if (st + NS - 1 < total) issue_b(nbuf);
    compute(buf);
    buf = buf + 1 == NS ? 0 : buf + 1;
    nbuf = nbuf + 1 == NS ? 0 : nbuf + 1;
    if (++kt == nk) {
      kt = 0;
      epilogue(tile_of(ti));  // its first barrier: every wave is done reading the halo
      lds_barrier();          // the stage is read back: the next halo may land on it
      if (++ti < my_tiles) stage(tile_of(ti));
    }
  }
}

// zero-fill D rows of the output pixel mapping that the GEMM does not cover
__global__ void zero_bf16(bf16_t* __restrict__ p, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x)
    reinterpret_cast<uint4*>(p)[i] = make_uint4(0, 0, 0, 0);
}

// W[Cout][R][S][Cin] -> Wt[Cin][Rs][Ss][Cout] over the tap subset r = r0 + dr*i, s = s0 + ds*j
__global__ void weight_transpose(const bf16_t* __restrict__ W, bf16_t* __restrict__ Wt, int Cout, int R, int S,
                                 int Cin, int r0, int dr, int Rs, int s0, int ds, int Ss) {
  __shared__ bf16_t tile[32][33];
  const int tap = blockIdx.z;
  const int ri = tap / Ss, si = tap - ri * Ss;
  const int r = r0 + dr * ri, s = s0 + ds * si;
  const int co0 = blockIdx.y * 32, ci0 = blockIdx.x * 32;
  for (int y = threadIdx.y; y < 32; y += blockDim.y) {
    const int co = co0 + y, ci = ci0 + threadIdx.x;
    tile[y][threadIdx.x] = (co < Cout && ci < Cin) ? W[(((long)co * R + r) * S + s) * Cin + ci] : (bf16_t)0;
  }
  __syncthreads();
  for (int y = threadIdx.y; y < 32; y += blockDim.y) {
    const int ci = ci0 + y, co = co0 + threadIdx.x;
    if (ci < Cin && co < Cout) Wt[(((long)ci * Rs + ri) * Ss + si) * Cout + co] = tile[threadIdx.x][y];
  }
}

// Every dgrad weight transpose of a training step in ONE launch (the per-call
// transposes were 61 launches / 0.35 ms per ResNet-50 step): block b finds its
// descriptor by the prefix table, then runs weight_transpose's 32x32 tile.
struct TDesc {
  const bf16_t* W;
  bf16_t* Wt;
  int Cout, R, S, Cin, r0, dr, Rs, s0, ds, Ss, gx, gy;
};

// 64 x 64 tiles, 256 threads: rows of 8 input channels (16 B) in, rows of 8 output
// channels (16 B) out, the tile staged in LDS with a 2-element row pad (the column
// reads of the write-out then spread over the banks).  The 32 x 32 / 2-byte form this
// replaces moved 1.4 TB/s (BERT-base: 238 us per step for 85 M elements); partial
// tiles and channel counts that are not multiples of 8 take the element-wise path.
__global__ __launch_bounds__(256) void weight_transpose_multi(const TDesc* __restrict__ descs,
                                                              const int* __restrict__ first, int n) {
  constexpr int T = 64, P = T + 2;
  __shared__ bf16_t tile[T * P];
  __shared__ int which;
  if (threadIdx.x == 0) {
    int lo = 0, hi = n - 1;  // last descriptor whose first block <= blockIdx.x
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    which = lo;
  }
  __syncthreads();
  const TDesc d = descs[which];
  int b = (int)blockIdx.x - first[which];
  const int bx = b % d.gx;
  b /= d.gx;
  const int by = b % d.gy, tap = b / d.gy;
  const int ri = tap / d.Ss, si = tap - ri * d.Ss;
  const int r = d.r0 + d.dr * ri, s = d.s0 + d.ds * si;
  const int co0 = by * T, ci0 = bx * T;
  const long ws = (long)d.R * d.S * d.Cin;        // W stride between output channels
  const long ts = (long)d.Rs * d.Ss * d.Cout;     // Wt stride between input channels
  const bf16_t* src = d.W + ((long)r * d.S + s) * d.Cin;
  bf16_t* dst = d.Wt + ((long)ri * d.Ss + si) * d.Cout;
  const bool vec = (d.Cin % 8 == 0) && (d.Cout % 8 == 0) && co0 + T <= d.Cout && ci0 + T <= d.Cin &&
                   ((uintptr_t)d.W % 16 == 0) && ((uintptr_t)d.Wt % 16 == 0);
  const int t = threadIdx.x;
  if (vec) {
#pragma unroll
    for (int k = 0; k < 2; k++) {  // 64 rows x 8 chunks of 8 channels
      const int q = t + k * 256, row = q >> 3, ch = (q & 7) * 8;
      const uint4 v = *reinterpret_cast<const uint4*>(src + (co0 + row) * ws + ci0 + ch);
      uint32_t* tp = reinterpret_cast<uint32_t*>(tile + row * P + ch);  // 4-B aligned: P and ch even
      tp[0] = v.x; tp[1] = v.y; tp[2] = v.z; tp[3] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int q = t + k * 256, ci = q >> 3, co = (q & 7) * 8;
      uint32_t w[4];
#pragma unroll
      for (int e = 0; e < 4; e++)
        w[e] = (uint32_t)tile[(co + 2 * e) * P + ci] | ((uint32_t)tile[(co + 2 * e + 1) * P + ci] << 16);
      *reinterpret_cast<uint4*>(dst + (ci0 + ci) * ts + co0 + co) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return;
  }
  for (int q = t; q < T * T; q += 256) {
    const int row = q / T, ci = q % T;
    tile[row * P + ci] = (co0 + row < d.Cout && ci0 + ci < d.Cin) ? src[(co0 + row) * ws + ci0 + ci] : (bf16_t)0;
  }
  __syncthreads();
  for (int q = t; q < T * T; q += 256) {
    const int ci = q / T, co = q % T;
    if (ci0 + ci < d.Cin && co0 + co < d.Cout) dst[(ci0 + ci) * ts + co0 + co] = tile[co * P + ci];
  }
}

}  // namespace

// descs: n x 14 ints-worth descriptors (TDesc, host-packed; gx / gy = 64-wide tile counts
// over Cin / Cout), first: n block offsets, total blocks
KFA_API int kfa_tdesc_bytes() { return (int)sizeof(TDesc); }

KFA_API int kfa_weight_transpose_multi(const void* descs, const int* first, int n, int total_blocks, hipStream_t st) {
  if (n <= 0 || total_blocks <= 0) return 0;
  hipLaunchKernelGGL(weight_transpose_multi, dim3(total_blocks), dim3(256), 0, st,
                     reinterpret_cast<const TDesc*>(descs), first, n);
  return kfa_status();
}

static const bf16_t* zero_page() {
  static bf16_t* z = nullptr;
  if (!z) {
    if (hipMalloc(&z, 256) != hipSuccess) return nullptr;
    (void)hipMemset(z, 0, 256);
    (void)hipDeviceSynchronize();
  }
  return z;
}

// The epilogue sets a kernel family is compiled with (see conv_igemm_kernel's EPI), in the
// order with_epi tries them.
template <unsigned... EPI>
struct EpiList {};
using IgemmEpis = EpiList<0u, kEpiStats, kEpiE, kEpiE | kEpiEmb, kEpiStats | kEpiBnBwd, kEpiE | kEpiStats | kEpiBnBwd,
                          kEpiE | kEpiEmb | kEpiStats | kEpiBnBwd, kEpiAll>;  // conv_igemm_kernel, conv_pp_kernel
using ProEpis = EpiList<0u, kEpiStats>;  // PRO (forward convs reading a BatchNorm's raw input)
// halo-staged 3x3 (no addend; no kEpiYMask: host-checked): forward statistics, backward statistics
using HaloEpis = EpiList<0u, kEpiStats, kEpiStats | kEpiBnBwd>;

// f(std::integral_constant<unsigned, EP>) for the first set EP of the list covering `need`
// (the last one if none does); only the list's sets are instantiated
template <class F, unsigned EP, unsigned... REST>
static void with_epi(unsigned need, EpiList<EP, REST...>, F&& f) {
  if (sizeof...(REST) == 0 || (need & ~EP) == 0) f(std::integral_constant<unsigned, EP>{});
  else if constexpr (sizeof...(REST) > 0) with_epi(need, EpiList<REST...>{}, f);
}

// Launch KERNEL with `lds` bytes of dynamic LDS, first raising the kernel's limit to at least
// that (beyond the 64 KB every kernel may use; running maximum per instantiation).
template <auto KERNEL, class... Args>
static void launch(dim3 grid, dim3 block, int lds, hipStream_t st, Args... args) {
  static int limit = 65536;
  if (lds > limit) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    limit = lds;
  }
  hipLaunchKernelGGL(KERNEL, grid, block, lds, st, args...);
}

// Block tiles of conv_igemm_kernel (variants 0-3): WM x WN waves of 16 TM x 16 TN each, double-
// buffered operands in LDS, PER_CU resident blocks per CU (the persistent grid's cap);
// OVERSUB: KFA_CONV_OVERSUB scales that cap (plain launches only).
template <int WM_, int WN_, int TM_, int TN_, int PER_CU, bool OVERSUB>
struct Tile {
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, per_cu = PER_CU;
  static constexpr bool oversub = OVERSUB;
  static constexpr int bm = WM * TM * 16, bn = WN * TN * 16, threads = 64 * WM * WN, lds = 2 * (bm + bn) * BK * 2;
};

template <class F>
static void with_tile(int variant, F&& f) {
  switch (variant) {
    case 1: return f(Tile<4, 1, 2, 4, 3, false>{});  // 128 x 64 (Cout <= 64): 4 waves of 32x64, 48 KB LDS
    case 2: return f(Tile<2, 4, 8, 4, 1, false>{});  // 256 x 256: 2x4 waves of 128x64, 128 KiB LDS
    case 3: return f(Tile<4, 1, 4, 4, 2, true>{});   // 256 x 64 (Cout <= 64): 4 waves of 64x64, 80 KB LDS
    default: return f(Tile<2, 2, 4, 4, 2, true>{});  // 128 x 128: 2x2 waves of 64x64, 64 KB LDS
  }
}

static int capped(long tiles, long slots) { return (int)(tiles < slots ? tiles : slots); }

// The Geo of one launch; false when a buffer does not fit the 32-bit buffer offsets.
static bool make_geo(Geo& g, int Nb, int H, int W, int C, int P, int Q, int R, int S, int sa, int ra, int oa, int ob,
                     int N, int OH, int OW, int os, int oph, int opw, int ldd) {
  const long tb = (long)Nb * H * W * C * 2, bb = (long)N * R * S * C * 2, db = (long)Nb * OH * OW * ldd * 2;
  g = Geo{Nb, H, W, C, P, Q, R, S, sa, ra, oa, ob, Nb * P * Q, N, R * S * C, OH, OW, os, oph, opw, ldd,
          (unsigned)tb, (unsigned)bb, (unsigned)db};
  return tb < (long)kOOB && bb < (long)kOOB && db < (long)kOOB;
}

// variant: 0 = 128x128 tile, 1 = 128x64 tile (N <= 64), 2 = 256x256 tile (8 waves), 3 = 256x64 (N <= 64),
// 4 = 256x256 ping-pong (conv_pp_kernel: C % 64 == 0, K > 0; one block per tile),
// 6 = 512x128 ping-pong (conv_pp_kernel<.., 4>: the 128-channel layers, same conditions),
// 7 = halo-staged (conv_halo_kernel: 3x3, stride 1, 'same' padding, C = 64 / 128, no addend,
//     no ReLU mask read from bn_y; else -6)
KFA_API int kfa_conv_igemm(const bf16_t* T, const bf16_t* B, bf16_t* D, const bf16_t* E, int Nb, int H, int W, int C,
                           int P, int Q, int R, int S, int sa, int ra, int oa, int ob, int N, int OH, int OW, int os,
                           int oph, int opw, int ldd, int variant, float* stats, const bf16_t* bn_x,
                           const bf16_t* bn_y, const float* bn_mean, int bn_relu, const float* bn_ss,
                           const uint8_t* bn_mb, const uint8_t* add_mb, hipStream_t st) {
  const BnBwd bnb{bn_x, bn_y, bn_ss, bn_mb, bn_mean, bn_relu, E ? add_mb : nullptr};
  if (bn_x && bn_relu && !bn_y && !bn_ss && !bn_mb) return -3;
  if ((bn_mb || (E && add_mb)) && ldd != N) return -4;  // the bit masks index [M][N] rows
  // C < 64: a BK slice spans S*C/64 whole taps of one filter row — one contiguous run of the
  // input row when the gather is stride 1 / pad 0 along w (the space-to-depth stem, stem.hip)
  const bool multi_tap = C % 8 == 0 && C < BK && BK % C == 0 && (S * C) % BK == 0 && sa == 1 && ra == 1 &&
                         oa == 0 && ob == 0;
  if ((C % BK != 0 && !multi_tap) || N % 8 != 0 || ldd % 8 != 0) return -1;
  Geo g;
  if (!make_geo(g, Nb, H, W, C, P, Q, R, S, sa, ra, oa, ob, N, OH, OW, os, oph, opw, ldd)) return -2;
  if (g.K == 0) g.R = g.S = 1;  // keep index math defined; nk == 0 -> zero/addend-only epilogue
  if (g.M <= 0) return 0;
  const int cus = kfa_cu_count();
  // persistent grid: PER_CU resident blocks per CU.  KFA_CONV_OVERSUB=k caps the grid of the
  // 2-per-CU tiles at k x that (0: one block per tile), so the dispatcher, not the tile
  // ranges, balances the work when other kernels (RCCL) hold part of the CUs.
  static int oversub = -1;
  if (oversub < 0) {
    const char* e = getenv("KFA_CONV_OVERSUB");
    oversub = e ? atoi(e) : 1;
    if (oversub < 0) oversub = 1;
  }
  const unsigned epi = (E ? kEpiE : 0u) | (stats ? kEpiStats : 0u) | (bn_x ? kEpiBnBwd : 0u) |
                       ((E && add_mb) ? kEpiEmb : 0u) | ((bn_x && bn_y && bn_relu) ? kEpiYMask : 0u);
  auto tiles = [&](int bm, int bn) { return (long)kfa_ceil_div(g.M, bm) * kfa_ceil_div(N, bn); };
  if ((variant == 4 || variant == 6) && C % BK == 0 && g.K > 0) {
    // ping-pong 256 x 256 / 512 x 128 (grid = tiles, one block per CU resident)
    const bool wide = variant == 6;
    const dim3 grid((unsigned)(wide ? tiles(512, 128) : tiles(256, 256)));
    with_epi(epi, IgemmEpis{}, [&](auto ep) {
      constexpr unsigned EP = decltype(ep)::value;
      if (wide) launch<conv_pp_kernel<EP, 4>>(grid, dim3(512), 0, st, T, B, D, E, stats, bnb, g);
      else launch<conv_pp_kernel<EP, 2>>(grid, dim3(512), 0, st, T, B, D, E, stats, bnb, g);
    });
  } else if (variant == 7) {  // halo-staged 3x3 (conv_halo_kernel): 256 x 64 tiles at C = 64, 128 x 128 at C = 128
    const bool same3 = R == 3 && S == 3 && sa == 1 && (ra == 1 || ra == -1) && oa == -ra && ob == -ra && H == P &&
                       W == Q && os == 1 && oph == 0 && opw == 0 && OH == P && OW == Q;
    if (!same3 || E || (epi & kEpiYMask) || (C != 64 && C != 128)) return -6;
    const int bm = C == 64 ? 256 : 128, bn = C == 64 ? 64 : 128;
    const int hrp = (bm + 2 * (W + 1) + 1 + 31) & ~31;  // staged rows + a zero row, whole rounds of DMA pieces
    const int ns = C == 64 ? 3 : 2;  // weight ring slots (8 KB / 16 KB each)
    const int lds = (C / 64) * hrp * 128 + ns * bn * BK * 2;
    if (lds > 160 * 1024) return -6;
    const dim3 grid(capped(tiles(bm, bn), (lds <= 80 * 1024 ? 2L : 1L) * cus));
    with_epi(epi, HaloEpis{}, [&](auto ep) {
      constexpr unsigned EP = decltype(ep)::value;
      if (C == 64) launch<conv_halo_kernel<4, 1, 4, 4, 3, EP>>(grid, dim3(256), lds, st, T, B, D, stats, bnb, g, hrp);
      else launch<conv_halo_kernel<2, 2, 4, 4, 2, EP>>(grid, dim3(256), lds, st, T, B, D, stats, bnb, g, hrp);
    });
  } else {
    with_tile(variant, [&](auto t) {
      using TL = decltype(t);
      const long slots = !TL::oversub ? (long)TL::per_cu * cus : oversub == 0 ? (1L << 30) : 2L * cus * oversub;
      const dim3 grid(capped(tiles(TL::bm, TL::bn), slots));
      with_epi(epi, IgemmEpis{}, [&](auto ep) {
        launch<conv_igemm_kernel<TL::WM, TL::WN, TL::TM, TL::TN, decltype(ep)::value>>(
            grid, dim3(TL::threads), TL::lds, st, T, B, D, E, zero_page(), stats, bnb, g, Pro{nullptr, nullptr});
      });
    });
  }
  return kfa_status();
}

// Forward conv of relu(x * scale + shift) (a training BatchNorm + ReLU folded into
// the A operand, see Pro): T = the BN's raw input x [Nb][H][W][C], ss = its
// [scale | shift], y (optional) receives the normalised activation — only for
// stride 1 with P == H, Q == W (the centre taps then cover every pixel).  D is
// [Nb][P][Q][N]; stats as kfa_conv_igemm.
KFA_API int kfa_conv_igemm_bnpro(const bf16_t* T, const bf16_t* B, bf16_t* D, const float* ss, bf16_t* y, int Nb,
                                 int H, int W, int C, int P, int Q, int R, int S, int stride, int pad, int N,
                                 int variant, float* stats, hipStream_t st) {
  if (!ss || C % BK != 0 || N % 8 != 0 || C > 2048) return -1;
  if (y && !(stride == 1 && P == H && Q == W && 2 * pad == R - 1 && 2 * pad == S - 1)) return -5;
  Geo g;
  if (!make_geo(g, Nb, H, W, C, P, Q, R, S, stride, 1, -pad, -pad, N, P, Q, 1, 0, 0, N)) return -2;
  if (g.M <= 0) return 0;
  const int cus = kfa_cu_count();
  const Pro pro{ss, y};
  const BnBwd bnb{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr};
  with_tile(variant, [&](auto t) {
    using TL = decltype(t);
    const dim3 grid(capped((long)kfa_ceil_div(g.M, TL::bm) * kfa_ceil_div(N, TL::bn), (long)TL::per_cu * cus));
    const int lds = TL::lds + 8 * C;  // the [scale | shift] table behind the operand ring
    with_epi(stats ? kEpiStats : 0u, ProEpis{}, [&](auto ep) {
      launch<conv_igemm_kernel<TL::WM, TL::WN, TL::TM, TL::TN, decltype(ep)::value, true>>(
          grid, dim3(TL::threads), lds, st, T, B, D, nullptr, zero_page(), stats, bnb, g, pro);
    });
  });
  return kfa_status();
}

KFA_API int kfa_zero_bf16(bf16_t* p, long n, hipStream_t st) {
  if (n % 8) return -1;
  long n8 = n / 8;
  long b = (n8 + 255) / 256;
  hipLaunchKernelGGL(zero_bf16, dim3(b < 4096 ? (b < 1 ? 1 : b) : 4096), dim3(256), 0, st, p, n8);
  return kfa_status();
}

KFA_API int kfa_weight_transpose(const bf16_t* W, bf16_t* Wt, int Cout, int R, int S, int Cin, int r0, int dr, int Rs,
                                 int s0, int ds, int Ss, hipStream_t st) {
  dim3 grid(kfa_ceil_div(Cin, 32), kfa_ceil_div(Cout, 32), Rs * Ss);
  hipLaunchKernelGGL(weight_transpose, grid, dim3(32, 8), 0, st, W, Wt, Cout, R, S, Cin, r0, dr, Rs, s0, ds, Ss);
  return kfa_status();
}
