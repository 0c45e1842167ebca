// Tile primitives shared by the MFMA matrix kernels (gemm.hip, gemm_ppp.hip,
// gemm_skinny.hip, conv_igemm.hip, wgrad.hip, conv3_bwd.hip, conv2_bwd.hip): one definition of each rule
// those kernels are built on.  Everything is __forceinline__ and stateless;
// the files pull the names in with `using namespace tile;`.
#pragma once
#include "common.h"

#include <utility>

namespace tile {

// ---- buffer resources ------------------------------------------------------
// Operands and outputs are addressed through buffer resources: the hardware
// range check turns padding taps, tile tails and rows past M / N into zero
// loads / dropped stores with NO branch, so hipcc keeps counted vmcnt waits
// instead of draining to vmcnt(0) around each guarded access.  kOOB is an
// offset past every extent (extents are host-checked to stay below it).
constexpr unsigned kOOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}

// 16-B buffer load / store.  AUX: cache policy (0 default, 2 = non-temporal: streamed past the caches)
template <int AUX = 0>
__device__ __forceinline__ uint4 bload16(__amdgpu_buffer_rsrc_t r, unsigned off) {
  auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, AUX);
  return *reinterpret_cast<uint4*>(&v);
}
template <int AUX = 0>
__device__ __forceinline__ void bstore16(__amdgpu_buffer_rsrc_t r, unsigned off, uint4 v) {
  using V = decltype(__builtin_amdgcn_raw_buffer_load_b128(r, 0, 0, 0));
  __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<V*>(&v), r, off, 0, AUX);
}

// ---- HBM/L2 -> LDS DMA, 16 B per lane --------------------------------------
// Plain device functions: either builtin named directly inside a templated
// kernel's lambda stops clang's host pass from emitting the kernel's launch
// stub (the library then fails at load time; _build.py checks for it).
// Buffer form (buffer_load_dwordx4 ... lds): voff per lane, soff wave-uniform, AUX as above.
template <int AUX = 0>
__device__ __forceinline__ void buf_dma16(__amdgpu_buffer_rsrc_t r, void* lds, int voff, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, AUX);
}
// Flat-pointer form (global_load_lds).
__device__ __forceinline__ void lds_dma16(const bf16_t* src, bf16_t* dst) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// ---- counted waits -----------------------------------------------------------
// DMAs and stores retire in order on vmcnt, LDS reads on lgkmcnt: a main loop
// waits for "all but the N youngest", never vmcnt(0).
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void lgkm_wait() {
  static_assert(N >= 0 && N < 16, "lgkmcnt is 4 bits");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
// s_waitcnt vmcnt(n) for a wave-uniform runtime n: a switch over the immediates.
// KFA_VMW(N) is one case (a kernel with a short range lists its own);
// KFA_VM_WAIT_RT(n) covers 0..62 and drains for anything else.  Statement macros:
// as an inlined function the same switch came out with another block layout.
#define KFA_VMW(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
#define KFA_VM_WAIT_RT(n)                                                                                  \
  switch (n) {                                                                                             \
    KFA_VMW(0) KFA_VMW(1) KFA_VMW(2) KFA_VMW(3) KFA_VMW(4) KFA_VMW(5) KFA_VMW(6) KFA_VMW(7)                \
    KFA_VMW(8) KFA_VMW(9) KFA_VMW(10) KFA_VMW(11) KFA_VMW(12) KFA_VMW(13) KFA_VMW(14) KFA_VMW(15)          \
    KFA_VMW(16) KFA_VMW(17) KFA_VMW(18) KFA_VMW(19) KFA_VMW(20) KFA_VMW(21) KFA_VMW(22) KFA_VMW(23)        \
    KFA_VMW(24) KFA_VMW(25) KFA_VMW(26) KFA_VMW(27) KFA_VMW(28) KFA_VMW(29) KFA_VMW(30) KFA_VMW(31)        \
    KFA_VMW(32) KFA_VMW(33) KFA_VMW(34) KFA_VMW(35) KFA_VMW(36) KFA_VMW(37) KFA_VMW(38) KFA_VMW(39)        \
    KFA_VMW(40) KFA_VMW(41) KFA_VMW(42) KFA_VMW(43) KFA_VMW(44) KFA_VMW(45) KFA_VMW(46) KFA_VMW(47)        \
    KFA_VMW(48) KFA_VMW(49) KFA_VMW(50) KFA_VMW(51) KFA_VMW(52) KFA_VMW(53) KFA_VMW(54) KFA_VMW(55)        \
    KFA_VMW(56) KFA_VMW(57) KFA_VMW(58) KFA_VMW(59) KFA_VMW(60) KFA_VMW(61) KFA_VMW(62)                    \
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;                                       \
  }
// Ping-pong kernels: retire every DMA except the pieces (PER_PHASE DMAs per lane
// each) issued in the `younger` (0..4) most recent phases.
template <int PER_PHASE = 2>
__device__ __forceinline__ void retire(int younger) {
  if (younger >= 4) vm_wait<4 * PER_PHASE>();
  else if (younger == 3) vm_wait<3 * PER_PHASE>();
  else if (younger == 2) vm_wait<2 * PER_PHASE>();
  else if (younger == 1) vm_wait<PER_PHASE>();
  else vm_wait<0>();
}

// Workgroup barrier for LDS hand-off only.  __syncthreads() is a workgroup
// release fence too, which makes hipcc drain vmcnt(0) for the epilogue's
// global stores — and with them the prefetch loads in flight.  Nothing in
// these kernels needs global-memory ordering between waves, only LDS.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- LDS accesses outside hipcc's sight ----------------------------------------
// Inline asm, for hand-counted kernels: the access is ordered by the kernel's own
// lgkmcnt waits and barriers, and hipcc -- which cannot tell an LDS-DMA's
// destination from any other LDS address -- sees no LDS access in front of which
// it would drain vmcnt(0), i.e. the loads, stores and DMAs in flight.
__device__ __forceinline__ unsigned lds_addr(const void* p) {  // the 32-bit LDS address the ds_ instructions take
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
// ds_read_b128 at la + OFF (OFF folded into the instruction: a fragment costs no address VGPR)
template <int OFF>
__device__ __forceinline__ short8 lds_rd16(unsigned la) {
  short8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(la), "i"(OFF) : "memory");
  return v;
}
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_wr16(unsigned la, uint4 v) {
  const uintx4 w = {v.x, v.y, v.z, v.w};
  asm volatile("ds_write_b128 %0, %1" ::"v"(la), "v"(w) : "memory");
}
__device__ __forceinline__ void lds_wr8(unsigned la, uintx2 v) {
  asm volatile("ds_write_b64 %0, %1" ::"v"(la), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_wr2(unsigned la, unsigned v) {  // the low 16 bits of v
  asm volatile("ds_write_b16 %0, %1" ::"v"(la), "v"(v) : "memory");
}

// ---- index helpers -----------------------------------------------------------
// Persistent blocks over whole tiles: block b of nb owns the contiguous tiles
// [t0, t0 + nt) of ntiles (the first ntiles % nb blocks get one more).
struct TileRange {
  int t0, nt;
};
__device__ __forceinline__ TileRange tile_range(int ntiles, int nb, int b) {
  const int base = ntiles / nb, rem = ntiles % nb;
  return {b * base + (b < rem ? b : rem), base + (b < rem ? 1 : 0)};
}

// x / d for 0 <= x < 2^24 via an fp32 reciprocal + one correction step
// (hipcc's int32 division is a ~40-instruction sequence; these run per row).
__device__ __forceinline__ int fdiv(int x, int d, float rcp) {
  int q = (int)((float)x * rcp);
  const int r = x - q * d;
  q += (r >= d) - (r < 0);
  return q;
}

// LDS images with 128-B rows (64 bf16): 16-B chunk c of row r is stored at
// c ^ swz_chunk(r), applied on the per-lane SOURCE address of the DMA, so the
// 16-lane groups of each ds_read_b128 fragment read hit 16 distinct slots.
__device__ __forceinline__ int swz_chunk(int row) { return (row >> 1) & 7; }
// element offset of (row, logical 16-B chunk) in such an image
__device__ __forceinline__ int swz128(int row, int chunk) { return row * 64 + ((chunk ^ swz_chunk(row)) << 3); }

// ---- k-major operand images (wgrad.hip, conv3_bwd.hip) -------------------------
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

// [k][WIDTH] bf16 LDS images (WIDTH = 128 or 64 elements = 256 / 128-B rows),
// 16-B chunks XOR-swizzled so both the lane-linear DMA fill and the
// ds_read_b64_tr_b16 operand reads are conflict-free:
//   256-B rows: chunk ^ (((row&3)<<2) | ((row>>2)&3))           (16 chunks)
//   128-B rows: chunk ^ 2*(((row>>1)&1) | (((row>>3)&1)<<1))     (8 chunks; keeps 32-B pairs)
template <int WIDTH>
__device__ __forceinline__ int img_swz(int row) {
  if constexpr (WIDTH == 128) return ((row & 3) << 2) | ((row >> 2) & 3);
  else return 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}
template <int WIDTH>
__device__ __forceinline__ int img_off(int row, int col) {  // byte offset of element (row, col)
  return WIDTH * 2 * row + 16 * ((col >> 3) ^ img_swz<WIDTH>(row)) + 2 * (col & 7);
}

// The transposed read as inline asm, for hand-counted kernels:
// hipcc puts an s_waitcnt vmcnt(0) in front of every compiler-visible
// ds_read_b64_tr_b16 that follows an LDS-DMA into the same array (it cannot tell
// the pieces apart), draining the whole DMA pipeline once per phase; the asm form
// is ordered by the kernel's own counted vmcnt + s_barrier + lgkmcnt(0) instead.
// OFF: the read's constant byte offset (piece and k-half), folded into the instruction.
template <int OFF>
__device__ __forceinline__ v4i16 ds_tr16(unsigned addr) {
  v4i16 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
  return v;
}

// MFMA operand (8 consecutive k of one column: rows 8g + q and 8g + 4 + q, columns
// cb + 4p, T10 lane map) through ds_tr16: k-half KS's row offset (32 rows; the
// swizzle repeats every 16) as the immediate
template <int WIDTH, int KS>
__device__ __forceinline__ short8 tr_operand_asm(const bf16_t* tile, int cb, int lane) {
  const int g = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
  const int col = cb + 4 * p, r0 = 8 * g + q;
  const unsigned b = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const bf16_t*)tile;
  const v4i16 a = ds_tr16<KS * 32 * WIDTH * 2>(b + (unsigned)img_off<WIDTH>(r0, col));
  const v4i16 c = ds_tr16<KS * 32 * WIDTH * 2>(b + (unsigned)img_off<WIDTH>(r0 + 4, col));
  return short8{a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3]};
}

// Compile-time loop: f(std::integral_constant<int, 0>) ... f(<N-1>) — keeps
// register-array indices constant where `#pragma unroll` is not honoured
// (a runtime index sends the whole accumulator array to scratch).
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// ---- tile order ----------------------------------------------------------------
// Blocks are dealt round-robin to the 8 XCDs (block b runs on XCD b % 8); this
// bijective remap gives the blocks of one XCD consecutive positions in the tile
// order, so they share operand panels in that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q8 = nwg >> 3, r8 = nwg & 7, x8 = bid & 7;
  return (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + (bid >> 3);
}
// Grouped raster: consecutive positions walk GM row-panels column-major, so the
// ~32 tiles an XCD runs at once form a GM x (32/GM) block whose A and B panels
// fit its 4 MB L2 together (row-major order would stream all of B past every A
// panel).  Position wg of an ntm x ntn tile grid -> (tile row, tile column).
// (The row sum's operand order reaches the ISA as written; this order is the one
// the persistent kernels were compiled with, profiles/isa_diff_tile_h.md.)
__device__ __forceinline__ int2 raster_tile(int wg, int ntm, int ntn, int GM) {
  const int grp = wg / (GM * ntn), gm0 = grp * GM, gmn = min(GM, ntm - gm0), rem = wg - grp * GM * ntn;
  return make_int2(rem % gmn + gm0, rem / gmn);
}

}  // namespace tile
