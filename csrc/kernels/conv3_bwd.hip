// One-pass backward of a bottleneck tail: bn3's backward apply + conv3's data and
// weight gradients, for identity blocks whose conv3 is a 1x1 / stride-1 conv with
// Ci = 64 or 128 input and Co = 4 Ci output channels (ResNet-50 stages 1 and 2).
//
// The separate path runs three passes over the [K, Co] tensors (K = Nb*P*Q pixels):
//   bn_bwd_apply   reads g, x3 (+ ReLU bits)  writes dx3
//   conv3 dgrad    reads dx3                  writes dX2 (+ bn2's backward statistics)
//   conv3 wgrad    reads dx3, y2              writes fp32 split-K partials
// dx3 = a[c]*(g*mask) + b[c]*x3 + k[c] (bn_bwd_finalize's coef), rounded to bf16, is pure
// intermediate.  Here each block streams g and x3 ONCE: per 64-pixel tile it forms the
// bf16 dx3 tile in LDS (the same expression and rounding as bn_bwd_apply) and feeds both
// products from that image:
//   dX2 tile  = dx3 . W      pixel rows = A operand (ds_read_b128), k = co ascending in
//                            steps of 32 as conv_igemm_kernel walks it; W = the dgrad's
//                            transposed weight [Ci][Co], in LDS (below)
//   dW       += dx3^T . y2   both operands k(pixel)-major, read with ds_read_b64_tr_b16 as
//                            in wgrad.hip; y2 tile by LDS-DMA; dW lives in registers for the
//                            block's whole pixel range (64 / 128 fp32 per lane)
// so 2T + 3t bytes move instead of 5T + 3t (T = K*Co*2, t = T/4).
//
// Blocks (4 Ci threads) are persistent: block b owns one contiguous range of whole 64-pixel
// tiles and writes ONE complete fp32 dW partial [Co][Ci] at the end (slab b);
// wgrad_reduce_kernel then sums the slabs into the flat gradient.  No block waits for another.
//
// LDS image of the dx3 tile: Co / 128 [64 pixel][128 co] sub-images with tile.h's img_swz<128>
// chunk swizzle.  Both read patterns are conflict-free under it: the transposed reads by
// construction (wgrad.hip), and the 16 pixel rows of a ds_read_b128 fragment read (one
// logical chunk, 16 consecutive rows) land in 16 distinct chunks of the 256-B bank cycle,
// because img_swz<128> is a bijection of row & 15.
//
// Weight: a [Ci][256 co] slot (512-B rows, chunk ^ (ci & 15)).  Ci = 64: the whole weight
// (32 KB), loaded once, resident.  Ci = 128: the 128 KB weight does not fit beside the tiles;
// its two 256-co halves (64 KB each) pass through the slot once per tile from L2 by
// LDS-DMA, the first under the wgrad's MFMAs, the second exposed (one slot).
//
// LDS: Ci = 64: image 32 + W 32 + y2 8 + coef 3 + bn2 0.75 = 75.75 KB, two blocks per CU;
//      Ci = 128: image 64 + W slot 64 + y2 16 + coef 6 + bn2 1.5 = 151.5 KB, one block (8 waves) per CU.
// (bn2: mean | scale | shift of the BatchNorm whose backward statistics the epilogue gathers.)
//
// Epilogue (this file's own; conv_epilogue.h's staging, rounding and statistics): each wave stages
// its dX2 rows in the image rows that wave itself wrote (no other wave writes there, and every
// wave's reads of the image are behind a barrier by then) with inline-asm ds_write_b64 /
// ds_read_b128 under its own lgkmcnt, so hipcc sees no LDS access there and places no vmcnt(0)
// for the LDS-DMA and the loads in flight.  Its x2 operand (2 x 16 B + 2 bit bytes per lane) is
// loaded BEFORE the next tile's prefetch: vmcnt retires in order, the wait hipcc counts for it
// (vmcnt(24) or more) leaves everything younger in flight.
//
// Loads in flight, per tile (vm_wait<0> = the kernel's own full wait):
//   Ci = 64   image formed from gv / xv / bits (hipcc's counted waits) . vm_wait<0> (y2 DMA landed)
//             . x2 loads . the WHOLE next tile's g / x3 / bits (24 loads, 72 VGPRs; past the block's
//             last tile the same loads at an offset past the extents, so every trip counts alike)
//             . barrier . dgrad + wgrad MFMAs . barrier . next y2 DMA . epilogue . back edge:
//             the prefetch and the DMA stay in flight from their issue to the next image.
//             226 VGPRs, no scratch.
//   Ci = 128  128 dW registers per lane of 256 (two waves per SIMD): image . vm_wait<0> . barrier
//             . W half 0 DMA . wgrad . vm_wait<0> . x2 loads . dgrad half 0 . barrier . W half 1 DMA
//             . the FIRST HALF of the next tile's loads (12 loads, 36 VGPRs: what is free from here
//             to the end of the epilogue) . vm_wait<12> (the DMA, not the loads) . dgrad half 1
//             . barrier . next y2 DMA . epilogue . the second half of the loads (nothing over it).
//             The load plans are re-formed per use from the lane id (held across the tile they
//             went to scratch, and a scratch reload is a vmcnt(0)).  256 VGPRs, 13 spilled dwords
//             (two dW fragments parked across the dgrad and the epilogue, one dword outside the loop).
// Rows past K: g / x3 / y2 read 0 through the buffer range check (the dx3 rows are then
// k[c], multiplied by y2 = 0 in dW; their dX2 rows are dropped by the epilogue's range check
// and masked out of the statistics).
#include "common.h"
#include "tile.h"
#include "conv_epilogue.h"

namespace {
using namespace tile;

constexpr int TP = 64;  // pixels per tile

__device__ __forceinline__ void unpack8f(const short8 v, float f[8]) {
  unpack8(__builtin_bit_cast(uint4, v), f);
}

template <int CI>
__global__ __launch_bounds__(4 * CI, CI == 64 ? 2 : 1) void conv3_bwd_fused_kernel(
    const bf16_t* __restrict__ G, const bf16_t* __restrict__ X3, const uint8_t* __restrict__ MB,
    const float* __restrict__ coef, const bf16_t* __restrict__ Y2, const bf16_t* __restrict__ Wt,
    bf16_t* __restrict__ DX2, float* __restrict__ part, float* __restrict__ stats, BnBwd bnb, Geo g) {
  static_assert(CI == 64 || CI == 128, "LDS and register budgets are laid out for Ci = 64 / 128");
  constexpr int CO = 4 * CI, NT = 4 * CI, NW = NT / 64;
  constexpr int CPR = CO / 8;             // 16-B chunks per dx3 row (32 / 64)
  constexpr int LR = TP * CPR / NT;       // 16-B g / x3 loads per lane per tile (8)
  constexpr int RPW = TP / NW;            // image rows a wave fills (16 / 8)
  constexpr int RSTEP = 64 / CPR;         // rows one wave instruction covers (2 / 1)
  constexpr int SUB = TP * 128;           // elements of one [64][128] sub-image
  constexpr int WH = CO / 256;            // 256-co weight halves passing through the slot (1: resident)
  constexpr int WL = CI * 32 / NT;        // 16-B loads per lane per weight half (8)
  constexpr int TNW = CI / 16;            // wgrad ci tiles per wave (4 / 8)
  constexpr bool PREFETCH = CI == 64;     // next tile's register loads under this tile's MFMAs + epilogue
  static_assert(LR * RSTEP == RPW, "a wave's loads cover its own image rows");
  __shared__ __attribute__((aligned(16))) bf16_t s_img[TP * CO];
  __shared__ __attribute__((aligned(16))) bf16_t s_w[CI * 256];
  __shared__ __attribute__((aligned(16))) bf16_t s_y[TP * CI];
  __shared__ __attribute__((aligned(16))) float s_coef[3 * CO];
  __shared__ __attribute__((aligned(16))) float s_bn[3 * CI];  // bn2: mean | scale | shift (0 where not given)

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wp = wave & 3, wc = wave >> 2;  // dgrad wave tile: pixels 16 wp .., ci 64 wc ..
  // pixel ownership: whole tiles, dealt contiguously (the first `rem` blocks get one more)
  const int ntiles = (g.M + TP - 1) / TP, nb = gridDim.x, b = blockIdx.x;
  const TileRange own = tile_range(ntiles, nb, b);
  const int t0 = own.t0, nt = own.nt;
  if (nt == 0) return;

  const unsigned big_bytes = (unsigned)g.M * (unsigned)CO * 2u;
  const __amdgpu_buffer_rsrc_t rG = rsrc(G, big_bytes), rX = rsrc(X3, big_bytes);
  const __amdgpu_buffer_rsrc_t rM = rsrc(MB, big_bytes >> 4);
  const __amdgpu_buffer_rsrc_t rY = rsrc(Y2, g.d_bytes), rD = rsrc(DX2, g.d_bytes);
  // bn2's backward statistics (the epilogue below): its input x2 and, where the ReLU mask is kept as
  // bits, the bit bytes (one per 16-B chunk); zero extents read 0 without a branch
  const bool bstat = stats && bnb.x;
  const bool bmask = bstat && bnb.relu && bnb.mb, xmask = bstat && bnb.relu && !bnb.mb;
  const __amdgpu_buffer_rsrc_t rBX = rsrc(bstat ? (const void*)bnb.x : DX2, bstat ? g.d_bytes : 0u);
  const __amdgpu_buffer_rsrc_t rBM = rsrc(bmask ? (const void*)bnb.mb : DX2, bmask ? g.d_bytes >> 4 : 0u);

  // weight half h into the slot: row ci, 16-B chunk c (of the half's 32) stored at c ^ (ci & 15)
  // (the 16 rows of a fragment read then hit 16 distinct chunks of one 256-B bank cycle)
  // (Ci = 128: by LDS-DMA, no registers: wave instruction j = WL wave + i fills rows 2j, 2j + 1
  // lane-linearly, the swizzle applied on the per-lane source address)
  const __amdgpu_buffer_rsrc_t rW = rsrc(Wt, g.b_bytes);
  auto w_dma = [&](int h) __attribute__((always_inline)) {
    int lx = lane;  // source offsets formed per use, not carried across the tile loop
    asm volatile("" : "+v"(lx));
    static_for<WL>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int row = (wave * WL + i) * 2 + (lx >> 5);
      const int vo = (row * CO + (((lx & 31) ^ (row & 15)) << 3)) * 2;
      buf_dma16(rW, s_w + (wave * WL + i) * 512, vo, h * 512);
    });
  };
  if constexpr (WH == 1) {  // resident: straight through (the staged form's register array would sit in scratch here)
#pragma unroll
    for (int i = 0; i < WL; i++) {
      const int id = i * NT + tid, row = id >> 5, c = id & 31;
      const uint4 v = *reinterpret_cast<const uint4*>(Wt + row * CO + c * 8);
      *reinterpret_cast<uint4*>(s_w + row * 256 + ((c ^ (row & 15)) << 3)) = v;
    }
  }
  for (int i = tid; i < 3 * CO; i += NT) s_coef[i] = coef[i];
  if (tid < 3 * CI) {
    const int a = tid / CI, n = tid % CI;
    s_bn[tid] = !bstat ? 0.f : a == 0 ? bnb.mean[n] : xmask ? bnb.ss[(a - 1) * CI + n] : 0.f;
  }
  __syncthreads();
  // prologue plan: load i of a lane is row RPW*wave + RSTEP*i + lane / CPR, chunk lane % CPR (fixed
  // per lane: its 8 channels' coefficients are re-read from LDS per tile, not held in registers)
  const unsigned pvo = (unsigned)((RPW * wave + lane / CPR) * CO + (lane % CPR) * 8) * 2u;  // byte offset within a tile
  // y2 plan (wgrad.hip's staging): a wave instruction fills 1 KB = 512 / CI rows, physical chunk
  // lane % (CI/8) <- logical chunk ^ img_swz<CI>(row), applied on the source address
  constexpr int YRPI = 512 / CI, YCPR = CI / 8;
  constexpr int YI = TP / YRPI / NW;  // y2 DMA instructions per wave per tile (2)
  int y_vo[YI];
#pragma unroll
  for (int i = 0; i < YI; i++) {
    const int row = (wave * YI + i) * YRPI + lane / YCPR;
    y_vo[i] = (row * CI + (((lane % YCPR) ^ img_swz<CI>(row)) << 3)) * 2;
  }

  uint4 gv[LR], xv[LR];
  unsigned bits[LR];
  // (live: false past the block's last tile -- every offset then lies past the extents, the loads
  // return 0 without traffic, and the loop body issues the same number of loads on every trip,
  // so the waits hipcc counts for them never fall back to vmcnt(0))
  auto issue_regs = [&](int t, bool live, auto i0c, auto i1c) __attribute__((always_inline)) {
    constexpr int I0 = decltype(i0c)::value, I1 = decltype(i1c)::value;  // loads [I0, I1) of the tile
    const unsigned so = live ? (unsigned)t * (unsigned)(TP * CO * 2) : kOOB;
    unsigned pv = pvo;
    if constexpr (!PREFETCH) {  // (Ci = 128: the plan formed per use from the lane id; held across the tile it went to scratch)
      int lp = lane;
      asm volatile("" : "+v"(lp));
      pv = (unsigned)((RPW * wave + lp / CPR) * CO + (lp % CPR) * 8) * 2u;
    }
#pragma unroll
    for (int i = I0; i < I1; i++) {
      const unsigned vo = pv + (unsigned)(i * RSTEP * CO * 2);
      gv[i] = bload16<2>(rG, vo + so);
      bits[i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rM, (vo + so) >> 4, 0, 0);
    }
#pragma unroll
    for (int i = I0; i < I1; i++) xv[i] = bload16<2>(rX, pv + (unsigned)(i * RSTEP * CO * 2) + so);
  };
  constexpr std::integral_constant<int, 0> kL0{};
  constexpr std::integral_constant<int, CI == 64 ? LR : LR / 2> kLE{};  // loads issued early (Ci = 128: half the tile)
  constexpr std::integral_constant<int, LR> kLR{};
  auto issue_y = [&](int t) __attribute__((always_inline)) {
    int ly = lane;
    if constexpr (!PREFETCH) asm volatile("" : "+v"(ly));  // (as above)
#pragma unroll
    for (int i = 0; i < YI; i++) {
      const int row = (wave * YI + i) * YRPI + ly / YCPR;
      const int vo = PREFETCH ? y_vo[i] : (row * CI + (((ly % YCPR) ^ img_swz<CI>(row)) << 3)) * 2;
      buf_dma16(rY, s_y + (wave * YI + i) * YRPI * CI, vo, t * (TP * CI * 2));
    }
  };
  // epilogue plan of a wave tile (16 pixels x 64 ci): 16-B piece i of a lane is row 8 i + lane / 8,
  // chunk lane % 8.  Its x2 operand (and bit byte) is loaded at the top of the tile, BEFORE the next
  // tile's prefetch: vmcnt retires in order, so the epilogue's wait for it leaves the prefetch in flight
  uint4 bxv[2];
  unsigned bmv[2];
  auto epi_off = [&](int t, int i, int le) __attribute__((always_inline)) {
    const int m = t * TP + wp * 16 + i * 8 + (le >> 3);
    return m < g.M ? (unsigned)(m * CI + wc * 64 + (le & 7) * 8) * 2u : kOOB;
  };
  auto issue_bx = [&](int t) __attribute__((always_inline)) {
    int le = lane;
    asm volatile("" : "+v"(le));
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const unsigned off = epi_off(t, i, le);
      bxv[i] = bload16<KFA_CONV_EPI_LOAD_AUX>(rBX, off);
      bmv[i] = (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rBM, off >> 4, 0, 0);
    }
  };

  floatx4 accw[TNW][4], accd[4][1];
#pragma unroll
  for (int i = 0; i < 4; i++) accd[i][0] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < TNW; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) accw[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};

  // dgrad over weight half h: accd[ni][0] = D(pixel 16 wp + fr, ci 64 wc + 16 ni + 4 fq + r),
  // k = co ascending.  k-step j of the half reads logical chunk 4 j + fq of the pixel / weight
  // rows: the swizzles touch the chunk's low 4 bits only, so j & 3 picks one of four per-lane
  // bases and the sub-image, the weight row's second 256 B and ni are immediates
  auto dgrad_half = [&](auto hc) __attribute__((always_inline)) {
    constexpr int h = decltype(hc)::value;
    int ld = lane;  // fragment bases formed per use, not carried across the tile loop
    asm volatile("" : "+v"(ld));
    const int fr = ld & 15, fq = ld >> 4;
    static_for<8>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, q = j & 3, hi = j >> 2;
      const unsigned ch = (unsigned)(q * 4 + fq);
      const unsigned a_la = lds_addr(s_img) + (unsigned)img_off<128>(wp * 16 + fr, (int)ch * 8);
      const unsigned w_la = lds_addr(s_w) + (unsigned)((wc * 64 + fr) * 512) + ((ch ^ (unsigned)fr) << 4);
      short8 bf[4];
      const short8 af = lds_rd16<(h * 2 + hi) * SUB * 2>(a_la);
      bf[0] = lds_rd16<hi * 256 + 0 * 16 * 512>(w_la);
      bf[1] = lds_rd16<hi * 256 + 1 * 16 * 512>(w_la);
      bf[2] = lds_rd16<hi * 256 + 2 * 16 * 512>(w_la);
      bf[3] = lds_rd16<hi * 256 + 3 * 16 * 512>(w_la);
      lgkm_wait<0>();
      __builtin_amdgcn_sched_barrier(0);
      // (spelled out: inside nested lambdas `#pragma unroll` is not honoured, and a runtime
      // index sends the arrays to scratch)
      accd[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[0], af, accd[0][0], 0, 0, 0);
      accd[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[1], af, accd[1][0], 0, 0, 0);
      accd[2][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[2], af, accd[2][0], 0, 0, 0);
      accd[3][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[3], af, accd[3][0], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  // wgrad: accw[ni][mi] = dW(co 64 wave + 16 mi + fr, ci 16 ni + 4 fq + r), k = the tile's pixels
  auto wgrad = [&]() __attribute__((always_inline)) {
    const bf16_t* asub = s_img + (wave >> 1) * SUB;
    const int cb0 = (wave & 1) * 64;
    int lw = lane;  // operand addresses formed per tile, not carried across the tile loop
    asm volatile("" : "+v"(lw));
    static_for<2>([&](auto kc) __attribute__((always_inline)) {
      constexpr int ks = decltype(kc)::value;
      short8 af[4];
      static_for<4>([&](auto mc) __attribute__((always_inline)) {
        constexpr int mi = decltype(mc)::value;
        af[mi] = tr_operand_asm<128, ks>(asub, cb0 + mi * 16, lw);
      });
      constexpr int NG = CI == 64 ? 4 : 2;  // ci tiles per group of reads (Ci = 128 is at the VGPR limit)
      static_for<TNW / NG>([&](auto nc) __attribute__((always_inline)) {
        constexpr int n0 = decltype(nc)::value * NG;
        short8 bf[NG];
        static_for<NG>([&](auto ic) __attribute__((always_inline)) {
          constexpr int ni = decltype(ic)::value;
          bf[ni] = tr_operand_asm<CI, ks>(s_y, (n0 + ni) * 16, lw);
        });
        lgkm_wait<0>();
        __builtin_amdgcn_sched_barrier(0);
        static_for<4 * NG>([&](auto ic) __attribute__((always_inline)) {
          constexpr int ni = decltype(ic)::value >> 2, mi = decltype(ic)::value & 3;
          accw[n0 + ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[ni], af[mi], accw[n0 + ni][mi], 0, 0, 0);
        });
        __builtin_amdgcn_sched_barrier(0);
      });
    });
  };

  // dX2 wave tile out: conv_epilogue<1, 4, 1, kEpiStats | kEpiBnBwd>'s staging, rounding, stores and
  // statistics (conv_epilogue.h), with the LDS traffic as inline asm under the kernel's own lgkmcnt
  // and bn2's per-channel operands from s_bn.  MFMA leaves lane (fr, fq) 4 consecutive ci of pixel fr
  // per ni; staged as [16 pixel][64 ci] rows of 128 B (chunk ^ (row & 7)) in the wave's own image
  // rows, every lane then stores two 16-B pieces.  No vector-memory wait but the one hipcc counts
  // for bxv / bmv.
  auto epilogue = [&](int t) __attribute__((always_inline)) {
    int le = lane;
    asm volatile("" : "+v"(le));
    const int fr = le & 15, fq = le >> 4, c = le & 7, r0 = le >> 3;
    const unsigned st = lds_addr(s_img) + (unsigned)(RPW * wave * 256);
    const unsigned wa = st + (unsigned)(fr * 128 + (fq & 1) * 8), wx = (unsigned)((fq >> 1) ^ (fr & 7));
    lds_wr8(wa + ((0u ^ wx) << 4), uintx2{pack2(accd[0][0][0], accd[0][0][1]), pack2(accd[0][0][2], accd[0][0][3])});
    lds_wr8(wa + ((2u ^ wx) << 4), uintx2{pack2(accd[1][0][0], accd[1][0][1]), pack2(accd[1][0][2], accd[1][0][3])});
    lds_wr8(wa + ((4u ^ wx) << 4), uintx2{pack2(accd[2][0][0], accd[2][0][1]), pack2(accd[2][0][2], accd[2][0][3])});
    lds_wr8(wa + ((6u ^ wx) << 4), uintx2{pack2(accd[3][0][0], accd[3][0][1]), pack2(accd[3][0][2], accd[3][0][3])});
    const unsigned ra = st + (unsigned)(r0 * 128 + ((c ^ r0) << 4));
    short8 ov[2];
    ov[0] = lds_rd16<0>(ra);  // (LDS serves one wave's requests in order: the reads see the writes)
    ov[1] = lds_rd16<1024>(ra);
    if (!bstat) {  // wave-uniform
      lgkm_wait<0>();
      __builtin_amdgcn_sched_barrier(0);
      bstore16<KFA_CONV_STORE_AUX>(rD, epi_off(t, 0, le), __builtin_bit_cast(uint4, ov[0]));
      bstore16<KFA_CONV_STORE_AUX>(rD, epi_off(t, 1, le), __builtin_bit_cast(uint4, ov[1]));
    } else {
      const unsigned ba = lds_addr(s_bn) + (unsigned)((wc * 64 + c * 8) * 4);
      const short8 m0 = lds_rd16<0>(ba), m1 = lds_rd16<16>(ba);
      const short8 a0 = lds_rd16<CI * 4>(ba), a1 = lds_rd16<CI * 4 + 16>(ba);
      const short8 b0 = lds_rd16<CI * 8>(ba), b1 = lds_rd16<CI * 8 + 16>(ba);
      lgkm_wait<0>();
      __builtin_amdgcn_sched_barrier(0);
      const floatx4 mu[2] = {__builtin_bit_cast(floatx4, m0), __builtin_bit_cast(floatx4, m1)};
      const floatx4 sc[2] = {__builtin_bit_cast(floatx4, a0), __builtin_bit_cast(floatx4, a1)};
      const floatx4 sf[2] = {__builtin_bit_cast(floatx4, b0), __builtin_bit_cast(floatx4, b1)};
      float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const unsigned off = epi_off(t, i, le);
        bstore16<KFA_CONV_STORE_AUX>(rD, off, __builtin_bit_cast(uint4, ov[i]));
        float f[8], xf[8];
        unpack8f(ov[i], f);  // the bf16-rounded values the BatchNorm will see
        unpack8(bxv[i], xf);
        // ReLU mask: the bit byte, or y > 0 recomputed as bn_apply evaluated it, or none (the form is
        // wave-uniform: selected with mask arithmetic, not branches); rows past K take no part
        const unsigned mbits = off == kOOB ? 0u : bmask ? bmv[i] : 0xffu;
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const bool pos = fmaf(xf[j], sc[j >> 2][j & 3], sf[j >> 2][j & 3]) > 0.f;
          const bool keep = (((mbits >> j) & 1u) != 0u) & (pos | !xmask);
          const float dz = keep ? f[j] : 0.f;
          s1[j] += dz;
          s2[j] += dz * (xf[j] - mu[j >> 2][j & 3]);
        }
      }
      // lanes sharing chunk c (xor 8, 16, 32) reduced by butterfly; lane L then publishes channel
      // (L % 8) * 8 + L / 8: one 64-lane atomic per statistic covers the wave's 64 channels
#pragma unroll
      for (int o = 8; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < 8; j++) {
          s1[j] += __shfl_xor(s1[j], o, 64);
          s2[j] += __shfl_xor(s2[j], o, 64);
        }
      float a = s1[0], b = s2[0];
#pragma unroll
      for (int j = 1; j < 8; j++) {
        a = r0 == j ? s1[j] : a;
        b = r0 == j ? s2[j] : b;
      }
      float* slot = stats + (long)(blockIdx.x % kBnSlots) * 2 * CI + (wc * 64 + c * 8 + r0);
      __hip_atomic_fetch_add(slot, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(slot + CI, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) accd[i][0] = floatx4{0.f, 0.f, 0.f, 0.f};
  };

  issue_y(t0);
  issue_regs(t0, true, kL0, kLR);
  for (int it = 0; it < nt; it++) {
    const int t = t0 + it;
    // dx3 tile -> LDS image (bn_bwd_apply's expression and rounding)
    int lc = lane;  // (image addresses formed per tile)
    asm volatile("" : "+v"(lc));
    const int pc = lc % CPR, pr = RPW * wave + lc / CPR;
    float ca[8], cb[8], ck[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      ca[j] = s_coef[pc * 8 + j];
      cb[j] = s_coef[CO + pc * 8 + j];
      ck[j] = s_coef[2 * CO + pc * 8 + j];
    }
#pragma unroll
    for (int i = 0; i < LR; i++) {
      float gf[8], xf[8], o[8];
      unpack8(gv[i], gf);
      unpack8(xv[i], xf);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float dz = ((bits[i] >> j) & 1u) ? gf[j] : 0.f;
        o[j] = fmaf(ca[j], dz, fmaf(cb[j], xf[j], ck[j]));
      }
      const int row = i * RSTEP + pr;
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(s_img + (pc >> 4) * SUB) + img_off<128>(row, (pc & 15) * 8)) =
          pack8(o);
    }
    vm_wait<0>();  // this tile's y2 DMA landed (the youngest load in flight; the last tile's stores drain too)
    if constexpr (PREFETCH) {
      issue_bx(t);                        // the epilogue's x2 operand: older than the prefetch, so waiting for it leaves the prefetch alone
      issue_regs(t + 1, it + 1 < nt, kL0, kLR);  // the whole next tile in flight under this tile's MFMAs and epilogue
    }
    lds_barrier();                                           // image and y2 tile published (also the resident weight)

    if constexpr (WH == 1) {
      dgrad_half(std::integral_constant<int, 0>{});
      wgrad();
    } else {
      // (every wave left the last tile's second-half reads of the slot behind that tile's last barrier)
      w_dma(0);
      wgrad();  // half 0 lands under the wgrad's MFMAs
      vm_wait<0>();
      lds_barrier();
#pragma unroll
      for (int i = 0; i < 4; i++) accd[i][0] = floatx4{0.f, 0.f, 0.f, 0.f};  // (not live across the wgrad)
      issue_bx(t);  // (not held across the wgrad, where the registers run out; lands under the dgrad and the second half's DMA)
      dgrad_half(std::integral_constant<int, 0>{});
      lds_barrier();  // every wave is done reading half 0
      w_dma(1);       // (one slot: this half's L2 latency is exposed)
      // the first half of the next tile's loads (36 registers: what is free beside dW from here to the
      // end of the epilogue), younger than the DMA so that its wait leaves them in flight
      issue_regs(t + 1, it + 1 < nt, kL0, kLE);
      vm_wait<3 * (LR / 2)>();
      lds_barrier();
      dgrad_half(std::integral_constant<int, 1>{});
    }
    lds_barrier();  // every wave is done reading the image, the y2 tile and the weight slot
    if (it + 1 < nt) issue_y(t + 1);
    // dX2 tile out (LDS-staged 16-B stores, bn2's backward statistics), staged in this wave's own image rows
    epilogue(t);
    if constexpr (!PREFETCH)
      if (it + 1 < nt) issue_regs(t + 1, true, kLE, kLR);  // the second half: nothing over it
  }

  // this block's complete dW partial (slab b)
  float* slab = part + (long)b * (CO * CI);
#pragma unroll
  for (int ni = 0; ni < TNW; ni++)
#pragma unroll
    for (int mi = 0; mi < 4; mi++) {
      const int m = wave * 64 + mi * 16 + (lane & 15), n = ni * 16 + (lane >> 4) * 4;
      *reinterpret_cast<floatx4*>(slab + m * CI + n) = accw[ni][mi];
    }
}

bool fused_shape_ok(int Ci, int Co, int R, int S, int stride, int pad) {
  return R == 1 && S == 1 && stride == 1 && pad == 0 && (Ci == 64 || Ci == 128) && Co == 4 * Ci;
}

// blocks with a non-empty pixel range = fp32 partial slabs
int fused_blocks(long K, int Ci, int max_blocks) {
  return capped_blocks((K + TP - 1) / TP, max_blocks, Ci == 64 ? 2 : 1);
}

}  // namespace

// floats of the split-K partial workspace kfa_conv3_bwd_fused needs (0: shape not covered)
KFA_API long kfa_conv3_bwd_part_floats(int Nb, int P, int Q, int Co, int Ci, int max_blocks) {
  if (!fused_shape_ok(Ci, Co, 1, 1, 1, 0)) return 0;
  return (long)fused_blocks((long)Nb * P * Q, Ci, max_blocks) * Co * Ci;
}

// bn3 backward apply + conv3 dgrad + conv3 wgrad in one pass (see the top of this file).
//   g, x3 [K][Co] bf16, mb: bn3's ReLU bits (K*Co/8 bytes), coef [3][Co] (kfa_bn_bwd_finalize_only),
//   y2 [K][Ci], wt [Ci][Co] (the dgrad's transposed weight), dx2 [K][Ci] out,
//   grad [Co][Ci] (bf16 / fp32; accumulate as kfa_conv_wgrad), part: kfa_conv3_bwd_part_floats floats,
//   stats + bn_*: bn2's slot workspace and backward-statistics operands (all null: no statistics),
//   max_blocks: 0 = two blocks per CU (Ci = 64) / one (Ci = 128).
// -1: shape not covered (1x1 / stride 1 / pad 0, Ci = 64 / 128, Co = 4 Ci only), -2: 32-bit offset limits.
KFA_API int kfa_conv3_bwd_fused(const bf16_t* g, const bf16_t* x3, const uint8_t* mb, const float* coef,
                                const bf16_t* y2, const bf16_t* wt, bf16_t* dx2, void* grad, int grad_f32,
                                int accumulate, float* part, int Nb, int P, int Q, int Ci, int Co, int R, int S,
                                int stride, int pad, float* stats, const bf16_t* bn_x, const float* bn_mean,
                                int bn_relu, const float* bn_ss, const uint8_t* bn_mb, int max_blocks,
                                hipStream_t s) {
  if (!fused_shape_ok(Ci, Co, R, S, stride, pad)) return -1;
  if (!g || !x3 || !mb || !coef || !y2 || !wt || !dx2 || !grad || !part) return -1;
  if (bn_bwd_mask_missing(bn_x, bn_relu, bn_ss, bn_mb)) return -3;
  const long K = (long)Nb * P * Q;
  if (K <= 0) return 0;
  if (K >= (1L << 24) || K * Co * 2 >= (long)kOOB) return -2;
  Geo geo{Nb, P, Q, Co, P, Q, 1, 1, 1, 1, 0, 0, (int)K, Ci, Co, P, Q, 1, 0, 0, Ci,
          (unsigned)(K * Co * 2), (unsigned)((long)Ci * Co * 2), (unsigned)(K * Ci * 2)};
  const BnBwd bnb = bn_bwd_operands(bn_x, bn_mean, bn_relu, bn_ss, bn_mb);
  const int blocks = fused_blocks(K, Ci, max_blocks);
  float* st = bn_x ? stats : nullptr;
  if (Ci == 64)
    hipLaunchKernelGGL(conv3_bwd_fused_kernel<64>, dim3(blocks), dim3(256), 0, s, g, x3, mb, coef, y2, wt, dx2, part,
                       st, bnb, geo);
  else
    hipLaunchKernelGGL(conv3_bwd_fused_kernel<128>, dim3(blocks), dim3(512), 0, s, g, x3, mb, coef, y2, wt, dx2,
                       part, st, bnb, geo);
  return reduce_slabs(part, blocks, (long)Co * Ci, grad, grad_f32, accumulate, s);
}
