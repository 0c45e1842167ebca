// One-pass backward of a bottleneck's conv2: bn2's backward apply + conv2's data and weight
// gradients, for the 3x3 / stride-1 / pad-1 convs with 64 input and 64 output channels
// (the three stage-1 bottlenecks of ResNet-50, 56 x 56).
//
// The separate path runs three passes over the [M, 64] tensors (M = Nb*H*W pixels, t = 128 M bytes):
//   bn_bwd_apply<2,.>   reads g2, x2                writes dx2
//   conv2 dgrad (halo)  reads dx2 (x 1.45), x1      writes dX1 (+ bn1's backward statistics)
//   conv2 wgrad         reads dx2, y1 (nine times)  writes fp32 split-K partials
// dx2 = a[c]*(g2*mask) + b[c]*x2 + k[c], mask = fma(x2, scale, shift) > 0 (bn_bwd_finalize's coef,
// bn2's forward [scale | shift]), rounded to bf16, is pure intermediate.  Here each block forms the
// dx2 HALO image of a linear tile of 256 pixels in LDS once (bn_bwd_apply<2,.>'s expression and
// rounding: rows m0 - (W+1) .. m0 + 255 + (W+1), conv_halo_kernel's layout and halo_swz) and feeds
// both products from it.  Tap (r, s) of centre pixel q reads image row q - m0 + (W+1) + (1-r) W + (1-s)
// in BOTH products, and is valid iff (h + 1 - r, w + 1 - s) lies inside the image:
//   dX1[q][ci]        = sum_tap valid . dx2[row(q, tap)][co] . Wt[ci][tap][co]
//                       conv_halo_kernel's product exactly: tap-major k-tiles of 64 co, two k = 32
//                       halves, the same MFMA and operand order, an invalid tap reads the zero row
//                       (address select) -- every element's fp32 sequence, and dX1, is bit-identical
//   dW[co][tap][ci]  += sum_q valid . dx2[row(q, tap)][co] . y1[q][ci]
//                       both operands k(pixel)-major: dx2 from the SHIFTED image rows and y1 from a
//                       [256][128 B] centre tile (LDS-DMA, img_swz<64>) with ds_read_b64_tr_b16.  The
//                       transposed reads run with EXEC all ones; a tap that leaves the image is zeroed
//                       by AND-ing the dx2 fragment (one fragment per two MFMAs; garbage rows of the
//                       image are cleared with it) with 0xffff / 0 halves.  The masks come from a
//                       per-tile table in LDS (row above / below, column left / right valid, one u16
//                       per pixel each, filled by the first 256 threads): a lane's 8 pixels are one
//                       16-B read, so the main loop derives nothing from pixel coordinates.
// 5.9 t move instead of 8.5 t, in one launch plus the reduce.
//
// Blocks (512 threads) are persistent: block b owns one contiguous range of whole 256-pixel tiles, keeps
// dW (9 x 64 x 64 fp32 = 72 registers per lane: wave w owns co tile w / 2 and ci 32 (w % 2) .. + 31 of every
// tap) for its whole range and writes ONE fp32 slab [64][3][3][64] at the end; wgrad_reduce_kernel sums the
// slabs.  No block waits for another.
//
// LDS (one block per CU): halo image 48 KB (384 rows: 256 + 2 (W+1) + the zero row, W <= 62) + resident
// weight [9][64 ci][64 co] 72 KB (swz128) + y1 tile 32 KB + mask table 2 KB + coefficient tables 1.25 KB
// = 155.25 KB.  The epilogue stage (4 KB per wave) aliases the image.
//
// Loads in flight, per tile: image formed from the prefetched g2 / x2 registers (6 + 6 loads of 16 B per
// lane; every LDS access of the loop but the epilogue's is inline asm, so hipcc counts its waits for the
// registers alone) . vm_wait<0> (the y1 DMA landed) . the WHOLE next tile's g2 / x2 (past the block's
// last tile the same loads at an offset past the extents) . barrier . wgrad . dgrad . epilogue
// (conv_epilogue.h's: rounding, 16-B stores, bn1's backward statistics with the mask recomputed from x1;
// its x1 loads are younger than the prefetch, which by then has had the MFMA phase to land) . barrier
// . next y1 DMA (issued on every trip, under the next image's formation; hipcc's wait for the LAST pair
// of prefetched registers still comes out as vmcnt(0) and drains it: the last sixth of the image is
// formed behind the DMA).  Within the MFMA phases the fragment reads run one step ahead: the wgrad reads
// tap + 1's dx2 fragment under tap's two MFMAs, the dgrad one k = 32 half (six fragments) under the
// other half's eight.
// 253 VGPRs, no scratch, 158,976 B of LDS (67 SGPRs live in VGPR lanes).
#include "common.h"
#include "tile.h"
#include "conv_epilogue.h"

namespace {
using namespace tile;

constexpr int TP2 = 256;   // pixels per tile
constexpr int HRP2 = 384;  // image rows (48 KB)
constexpr int NT2 = 512;
constexpr int LR2 = HRP2 * 8 / NT2;  // 16-B g2 / x2 loads per lane per tile (6)

__device__ __forceinline__ int halo_swz2(int row) { return ((row >> 1) & 3) << 1; }  // conv_halo_kernel's halo_swz

__device__ __forceinline__ short8 and8(const short8 a, const short8 m) {
  const uint4 x = __builtin_bit_cast(uint4, a), y = __builtin_bit_cast(uint4, m);
  return __builtin_bit_cast(short8, make_uint4(x.x & y.x, x.y & y.y, x.z & y.z, x.w & y.w));
}

__global__ __launch_bounds__(NT2, 1) void conv2_bwd_fused_kernel(
    const bf16_t* __restrict__ G, const bf16_t* __restrict__ X2, const float* __restrict__ coef,
    const float* __restrict__ ss2, const bf16_t* __restrict__ Y1, const bf16_t* __restrict__ Wt,
    bf16_t* __restrict__ DX1, float* __restrict__ part, float* __restrict__ stats, BnBwd bnb, Geo g) {
  __shared__ __attribute__((aligned(16))) bf16_t s_halo[HRP2 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t s_w[9 * 64 * 64];
  __shared__ __attribute__((aligned(16))) bf16_t s_y[TP2 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_mask[4 * TP2];  // row above | row below | column left | column right
  __shared__ __attribute__((aligned(16))) float s_tab[5 * 64];       // a | b | k | scale | shift

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntiles = (g.M + TP2 - 1) / TP2, nb = gridDim.x, b = blockIdx.x;
  const TileRange own = tile_range(ntiles, nb, b);
  const int t0 = own.t0, nt = own.nt;
  if (nt == 0) return;

  const int HW1 = g.W + 1, HR = TP2 + 2 * HW1;  // staged rows; row HR is the zero row
  const int PQ = g.H * g.W;
  const float rPQ = 1.f / (float)PQ, rQ = 1.f / (float)g.W;
  const __amdgpu_buffer_rsrc_t rG = rsrc(G, g.t_bytes), rX = rsrc(X2, g.t_bytes);
  const __amdgpu_buffer_rsrc_t rY = rsrc(Y1, g.d_bytes), rD = rsrc(DX1, g.d_bytes);
  const bool bstat = stats && bnb.x;
  const EpiRes er{rD, rsrc(DX1, 0u), rsrc(bstat ? (const void*)bnb.x : DX1, bstat ? g.d_bytes : 0u), rsrc(DX1, 0u)};

  // resident weight: tap-major [9][64 ci][64 co], rows of 128 B with swz128 (conv_halo_kernel's ring slot layout)
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int id = i * NT2 + tid, tap = id >> 9, row = (id >> 3) & 63, c = id & 7;
    const uint4 v = *reinterpret_cast<const uint4*>(Wt + row * 576 + tap * 64 + c * 8);
    *reinterpret_cast<uint4*>(s_w + tap * 4096 + swz128(row, c)) = v;
  }
  if (tid < 192) s_tab[tid] = coef[tid];
  else if (tid < 320) s_tab[tid] = ss2[tid - 192];
  __syncthreads();

  const unsigned halo_la = lds_addr(s_halo), w_la = lds_addr(s_w), mask_la = lds_addr(s_mask);
  const unsigned tab_la = lds_addr(s_tab);
  const int fr = lane & 15, fq = lane >> 4;

  uint4 gv[LR2], xv[LR2];
  // (live: false past the block's last tile -- every offset then lies past the extents, so every trip
  // issues the same number of loads)
  auto issue_regs = [&](int t, bool live) __attribute__((always_inline)) {
    int lt = tid;
    asm volatile("" : "+v"(lt));
    const int fc = lt & 7, r0 = lt >> 3;
    const int p0 = t * TP2 - HW1 + r0;
#pragma unroll
    for (int i = 0; i < LR2; i++) {
      const int row = r0 + 64 * i, pix = p0 + 64 * i;
      const bool ok = live && row < HR && (unsigned)pix < (unsigned)g.M;
      const unsigned off = ok ? (unsigned)(pix * 64 + fc * 8) * 2u : kOOB;
      gv[i] = bload16<0>(rG, off);
      xv[i] = bload16<0>(rX, off);
    }
  };
  // y1 centre tile: 32 pieces of 1 KB (8 rows), four per wave; physical chunk lane % 8 <- logical
  // chunk ^ img_swz<64>(row), applied on the source address; rows past M read 0
  // (live: as issue_regs -- issued on every trip, so hipcc's counted waits for the registers always
  // leave these four in flight)
  auto issue_y = [&](int t, bool live) __attribute__((always_inline)) {
    int ly = lane;
    asm volatile("" : "+v"(ly));
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int row = (wave * 4 + i) * 8 + (ly >> 3);
      const int vo = (row * 64 + (((ly & 7) ^ img_swz<64>(row)) << 3)) * 2;
      buf_dma16(rY, s_y + (wave * 4 + i) * 512, live ? vo : (int)kOOB, live ? t * (TP2 * 128) : 0);
    }
  };

  floatx4 accw[9][2], accd[4][2];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) accd[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) accw[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  unsigned amask[2];  // dgrad: this lane's 9-bit tap validity per M sub-tile

  // wgrad: accw[tap][j] = dW(co 16 (wave / 2) + fr, tap, ci 32 (wave % 2) + 16 j + 4 fq + r), k = the tile's pixels
  auto wgrad = [&]() __attribute__((always_inline)) {
    int lw = lane;
    asm volatile("" : "+v"(lw));
    const int gq = lw >> 4, li = lw & 15, q4 = li >> 2, p4 = li & 3;
    const int col = (wave >> 1) * 16 + 4 * p4;
    const unsigned mla = mask_la + (unsigned)(gq * 16);
    const int cb0 = (wave & 1) * 32;
    static_for<8>([&](auto kc) __attribute__((always_inline)) {
      constexpr int ks = decltype(kc)::value;
      const short8 y0 = tr_operand_asm<64, ks>(s_y, cb0, lw);
      const short8 y1 = tr_operand_asm<64, ks>(s_y, cb0 + 16, lw);
      const short8 mr0 = lds_rd16<0 * 512 + ks * 64>(mla), mr2 = lds_rd16<1 * 512 + ks * 64>(mla);
      const short8 mc0 = lds_rd16<2 * 512 + ks * 64>(mla), mc2 = lds_rd16<3 * 512 + ks * 64>(mla);
      // the dx2 fragment of tap + 1 is read under tap's MFMAs (two reads in flight behind the wait)
      v4i16 a, c, an, cn;
      auto rd_tap = [&](auto tc, v4i16& ra, v4i16& rc) __attribute__((always_inline)) {
        constexpr int tap = decltype(tc)::value, r = tap / 3, s = tap % 3;
        // image row of this lane's transposed-read address: 8 gq + q4 (+ 4) of the k-step, shifted by the tap
        const int row = HW1 + (1 - r) * g.W + (1 - s) + 8 * gq + q4;
        const unsigned a_la = halo_la + (unsigned)(row * 128 + ((((col >> 3) ^ halo_swz2(row))) << 4) + (col & 7) * 2);
        const unsigned c_la =
            halo_la + (unsigned)((row + 4) * 128 + ((((col >> 3) ^ halo_swz2(row + 4))) << 4) + (col & 7) * 2);
        ra = ds_tr16<ks * 4096>(a_la);
        rc = ds_tr16<ks * 4096>(c_la);
      };
      rd_tap(std::integral_constant<int, 0>{}, a, c);
      static_for<9>([&](auto tc) __attribute__((always_inline)) {
        constexpr int tap = decltype(tc)::value, r = tap / 3, s = tap % 3;
        if constexpr (tap < 8) {
          rd_tap(std::integral_constant<int, tap + 1>{}, an, cn);
          lgkm_wait<2>();
        } else {
          lgkm_wait<0>();
        }
        __builtin_amdgcn_sched_barrier(0);
        short8 af = short8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
        a = an;
        c = cn;
        if constexpr (r == 0) af = and8(af, mr0);
        if constexpr (r == 2) af = and8(af, mr2);
        if constexpr (s == 0) af = and8(af, mc0);
        if constexpr (s == 2) af = and8(af, mc2);
        accw[tap][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y0, af, accw[tap][0], 0, 0, 0);
        accw[tap][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(y1, af, accw[tap][1], 0, 0, 0);
      });
    });
  };

  // dgrad: accd[ni][mi] = D(pixel 32 wave + 16 mi + fr, ci 16 ni + 4 fq + r); conv_halo_kernel's compute()
  auto dgrad = [&]() __attribute__((always_inline)) {
    int ld = lane;
    asm volatile("" : "+v"(ld));
    const int dr = ld & 15, dq = ld >> 4;
    const unsigned zero_la = halo_la + (unsigned)(HR * 128 + dq * 16);
    // the six fragments of one k = 32 half: (tap, half) -> registers; each half's reads are issued one
    // half ahead (under the other half's MFMAs), so every wait leaves six reads in flight
    short8 bf[2][4], af[2][2];
    auto rd_half = [&](auto tc, auto hc) __attribute__((always_inline)) {
      constexpr int tap = decltype(tc)::value, r = tap / 3, s = tap % 3, h = decltype(hc)::value;
      const int row0 = wave * 32 + dr + HW1 + (1 - r) * g.W + (1 - s);
      const int x = halo_swz2(row0);  // rows row0 + 16 mi share it
      const unsigned aa = halo_la + (unsigned)(row0 * 128) + (unsigned)(((4 * h + dq) ^ x) << 4);
      const unsigned bb = w_la + (unsigned)(tap * 8192 + swz128(dr, 4 * h + dq) * 2);
      const bool v0 = (amask[0] >> tap) & 1u, v1 = (amask[1] >> tap) & 1u;
      // (rows dr + 16 ni of the weight: swz_chunk(row + 16 ni) = swz_chunk(row), 16 rows = 2048 B)
      bf[h][0] = lds_rd16<0 * 2048>(bb);
      bf[h][1] = lds_rd16<1 * 2048>(bb);
      bf[h][2] = lds_rd16<2 * 2048>(bb);
      bf[h][3] = lds_rd16<3 * 2048>(bb);
      af[h][0] = lds_rd16<0>(v0 ? aa : zero_la);
      af[h][1] = lds_rd16<0>(v1 ? aa + 2048 : zero_la);
    };
    rd_half(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
    static_for<9>([&](auto tc) __attribute__((always_inline)) {
      constexpr int tap = decltype(tc)::value;
      rd_half(tc, std::integral_constant<int, 1>{});
      lgkm_wait<6>();
      __builtin_amdgcn_sched_barrier(0);
      static_for<8>([&](auto ic) __attribute__((always_inline)) {
        constexpr int ni = decltype(ic)::value >> 1, mi = decltype(ic)::value & 1;
        accd[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[0][ni], af[0][mi], accd[ni][mi], 0, 0, 0);
      });
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (tap < 8) {
        rd_half(std::integral_constant<int, tap + 1>{}, std::integral_constant<int, 0>{});
        lgkm_wait<6>();
      } else {
        lgkm_wait<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
      static_for<8>([&](auto ic) __attribute__((always_inline)) {
        constexpr int ni = decltype(ic)::value >> 1, mi = decltype(ic)::value & 1;
        accd[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[1][ni], af[1][mi], accd[ni][mi], 0, 0, 0);
      });
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  issue_regs(t0, true);
  issue_y(t0, true);
  for (int it = 0; it < nt; it++) {
    const int t = t0 + it, m0 = t * TP2;
    {
      // dx2 halo image (bn_bwd_apply<2,.>'s expression and rounding); rows from HR on are zero
      int lt = tid;
      asm volatile("" : "+v"(lt));
      const int fc = lt & 7, r0 = lt >> 3;
      const unsigned ta = tab_la + (unsigned)(fc * 32);
      const short8 t0a = lds_rd16<0>(ta), t0b = lds_rd16<16>(ta);
      const short8 t1a = lds_rd16<256>(ta), t1b = lds_rd16<256 + 16>(ta);
      const short8 t2a = lds_rd16<512>(ta), t2b = lds_rd16<512 + 16>(ta);
      const short8 t3a = lds_rd16<768>(ta), t3b = lds_rd16<768 + 16>(ta);
      const short8 t4a = lds_rd16<1024>(ta), t4b = lds_rd16<1024 + 16>(ta);
      lgkm_wait<0>();
      __builtin_amdgcn_sched_barrier(0);
      const floatx4 ca[2] = {__builtin_bit_cast(floatx4, t0a), __builtin_bit_cast(floatx4, t0b)};
      const floatx4 cb[2] = {__builtin_bit_cast(floatx4, t1a), __builtin_bit_cast(floatx4, t1b)};
      const floatx4 ck[2] = {__builtin_bit_cast(floatx4, t2a), __builtin_bit_cast(floatx4, t2b)};
      const floatx4 sc[2] = {__builtin_bit_cast(floatx4, t3a), __builtin_bit_cast(floatx4, t3b)};
      const floatx4 sf[2] = {__builtin_bit_cast(floatx4, t4a), __builtin_bit_cast(floatx4, t4b)};
#pragma unroll
      for (int i = 0; i < LR2; i++) {
        float gf[8], xf[8], o[8];
        unpack8(gv[i], gf);
        unpack8(xv[i], xf);
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const float dz = fmaf(xf[j], sc[j >> 2][j & 3], sf[j >> 2][j & 3]) > 0.f ? gf[j] : 0.f;
          o[j] = fmaf(ca[j >> 2][j & 3], dz, fmaf(cb[j >> 2][j & 3], xf[j], ck[j >> 2][j & 3]));
        }
        const int row = r0 + 64 * i;
        const uint4 pk = pack8(o);
        const uint4 v = row < HR ? pk : make_uint4(0u, 0u, 0u, 0u);
        lds_wr16(halo_la + (unsigned)(row * 128 + ((fc ^ halo_swz2(row)) << 4)), v);
      }
      // tap validity of the tile's pixels: the wgrad's mask table (one pixel per thread of the first
      // four waves; wave-uniform branch) ...
      if (wave < 4) {
        const int m = m0 + lt;
        const int n = fdiv(m, PQ, rPQ), rm = m - n * PQ;
        const int p = fdiv(rm, g.W, rQ), q = rm - p * g.W;
        const unsigned la = mask_la + (unsigned)(lt * 2);
        lds_wr2(la, p + 1 < g.H ? 0xffffu : 0u);         // r = 0 reads the row below
        lds_wr2(la + 512, p >= 1 ? 0xffffu : 0u);        // r = 2 the row above
        lds_wr2(la + 1024, q + 1 < g.W ? 0xffffu : 0u);  // s = 0 the column to the right
        lds_wr2(la + 1536, q >= 1 ? 0xffffu : 0u);       // s = 2 the column to the left
      }
      // ... and the dgrad's per-lane bits (conv_halo_kernel's stage())
#pragma unroll
      for (int mi = 0; mi < 2; mi++) {
        const int m = m0 + wave * 32 + mi * 16 + (lt & 15);
        const int n = fdiv(m, PQ, rPQ), rm = m - n * PQ;
        const int p = fdiv(rm, g.W, rQ), q = rm - p * g.W;
        unsigned mk = 0;
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
          for (int s = 0; s < 3; s++) {
            const bool ok = (unsigned)(p + 1 - r) < (unsigned)g.H && (unsigned)(q + 1 - s) < (unsigned)g.W;
            mk |= ok ? 1u << (r * 3 + s) : 0u;
          }
        amask[mi] = mk;
      }
    }
    vm_wait<0>();                        // this tile's y1 DMA landed (the last tile's stores drain too)
    issue_regs(t + 1, it + 1 < nt);      // the whole next tile in flight under this tile's MFMAs
    lds_barrier();                       // image, masks and y1 tile published

    wgrad();
    dgrad();

    // dX1 tile out (its first barrier: every wave is done reading the image and the y1 tile)
    conv_epilogue<2, 4, 1, kEpiStats | kEpiBnBwd>(g, accd, reinterpret_cast<char*>(s_halo) + wave * 4096, true, lane,
                                                 m0 + wave * 32, 0, PQ, rPQ, rQ, true, nullptr, stats, bnb, er);
    lds_barrier();  // the stage is read back: the next image may land on it
    issue_y(t + 1, it + 1 < nt);
  }

  // this block's complete dW partial (slab b): [co][tap][ci]
  float* slab = part + (long)b * (9 * 64 * 64);
  const int co = (wave >> 1) * 16 + fr;
#pragma unroll
  for (int tap = 0; tap < 9; tap++)
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int ci = (wave & 1) * 32 + j * 16 + fq * 4;
      *reinterpret_cast<floatx4*>(slab + (co * 9 + tap) * 64 + ci) = accw[tap][j];
    }
}

// 0: covered; -1: not 3x3 / stride 1 / pad 1 or C != 64; -2: 32-bit offset limits; -4: the halo of this W does not fit
int conv2_plan(long Nb, int H, int W, int C, int Co, int R, int S, int stride, int pad) {
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C != 64 || Co != 64) return -1;
  if (Nb <= 0 || H <= 0 || W <= 0) return -1;
  const long M = Nb * H * W;
  if (M >= (1L << 24) || (M + 2 * TP2) * 128 >= (long)kOOB) return -2;
  if (TP2 + 2 * (W + 1) + 1 > HRP2) return -4;
  return 0;
}

int conv2_blocks(long M, int max_blocks) {
  return capped_blocks((M + TP2 - 1) / TP2, max_blocks, 1);
}

}  // namespace

// floats of the partial workspace kfa_conv2_bwd_fused needs (0: shape not covered); max_blocks > 0 caps the
// grid (and asks the device nothing)
// (the pair in kfa_conv3_bwd_part_floats' order, Co then C; both must be 64, so nothing moves for a caller)
KFA_API long kfa_conv2_bwd_part_floats(int Nb, int H, int W, int Co, int C, int max_blocks) {
  if (conv2_plan(Nb, H, W, C, Co, 3, 3, 1, 1)) return 0;
  return (long)conv2_blocks((long)Nb * H * W, max_blocks) * 9 * 64 * 64;
}

// bn2 backward apply + conv2 dgrad + conv2 wgrad in one pass (see the top of this file).
//   g2, x2 [M][64] bf16, coef [3][64] (kfa_bn_bwd_finalize_only), ss2: bn2's forward [scale | shift],
//   y1 [M][64], wt [64 ci][3][3][64 co] (the dgrad's transposed weight), dx1 [M][64] out,
//   grad [64][3][3][64] (bf16 / fp32; accumulate as kfa_conv_wgrad), part: kfa_conv2_bwd_part_floats floats,
//   stats + bn_*: bn1's slot workspace and backward-statistics operands (all null: no statistics),
//   max_blocks: 0 = one block per CU.
// Refusals (nothing is launched): conv2_plan's codes; -1 also for a missing operand; -3: bn1's ReLU mask
// has no source the epilogue takes.
KFA_API int kfa_conv2_bwd_fused(const bf16_t* g2, const bf16_t* x2, const float* ss2, const float* coef,
                                const bf16_t* y1, const bf16_t* wt, bf16_t* dx1, void* grad, int grad_f32,
                                int accumulate, float* part, int Nb, int H, int W, int C, int Co, int R, int S,
                                int stride, int pad, float* stats, const bf16_t* bn_x, const float* bn_mean,
                                int bn_relu, const float* bn_ss, const uint8_t* bn_mb, int max_blocks,
                                hipStream_t s) {
  const int rc0 = conv2_plan(Nb, H, W, C, Co, R, S, stride, pad);
  if (rc0) return rc0;
  if (!g2 || !x2 || !ss2 || !coef || !y1 || !wt || !dx1 || !grad || !part) return -1;
  if (bn_bwd_mask_missing(bn_x, bn_relu, bn_ss, bn_mb)) return -3;
  const long M = (long)Nb * H * W;
  const unsigned bytes = (unsigned)(M * 128);
  Geo geo{Nb, H, W, 64, H, W, 3, 3, 1, -1, 1, 1, (int)M, 64, 576, H, W, 1, 0, 0, 64, bytes, 9u * 64u * 64u * 2u, bytes};
  const BnBwd bnb = bn_bwd_operands(bn_x, bn_mean, bn_relu, bn_ss, bn_mb);
  const int blocks = conv2_blocks(M, max_blocks);
  hipLaunchKernelGGL(conv2_bwd_fused_kernel, dim3(blocks), dim3(NT2), 0, s, g2, x2, coef, ss2, y1, wt, dx1, part,
                     bn_x ? stats : nullptr, bnb, geo);
  return reduce_slabs(part, blocks, 9L * 64 * 64, grad, grad_f32, accumulate, s);
}
