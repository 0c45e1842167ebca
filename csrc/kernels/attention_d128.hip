// Packed variable-length and causal attention at head dim 128 (the decoder sizes
// above ~1B parameters).  The contracts are those of the d = 64 packed kernels of
// attention.hip: qkv [T, 3·heads·128] bf16, cu int32 [B + 1], out [T, heads·128],
// lse / D [heads, T]; any length 1..8192 at any row offset; rows at or past a
// sequence end are zero in LDS and in register operands and are never loaded; the
// unowned rows cu[B]..T-1 are never read and written as zeros; scores in log2 units,
// lse in natural-log units; the same attn_pair_hash decisions in all three kernels.
//
// Design (one body per kernel, templated on CAUSAL and on RT, the 16-row tiles a
// wave owns):
//
// Registers.  Two workgroups of 256 threads per CU (__launch_bounds__(256, 2), a
//   256-register budget, no AGPR split to manage) rather than one at 512: one wave
//   per SIMD cannot hide its own softmax / hash VALU work, LDS latency or the image
//   loads behind another wave's MFMAs.  The budget is met by shape instead:
//     forward   owner block 128 queries, a wave owns 32 (RT = 2): 32 Q operand
//               registers, 64 O accumulators, and only 4 x 2 score tiles (32) live
//               because the streamed block is 64 keys, not 128;
//     dQ        owner block 128 queries, a wave owns 32 (RT = 2): 32 + 32 Q / dO
//               operand registers, 64 accumulators, and one 32-key slice at a time
//               (2 x 2 score and 2 x 2 dP tiles);
//     dK / dV   owner block 64 keys, a wave owns 16 (RT = 1): 16 + 16 K / V operand
//               registers, 2 x 32 accumulators.
//               (32 keys per wave would need 64 + 128 registers before any score tile.)
//   The lane's indices are formed again in each streamed block (an empty asm on the
//   lane id), so the swizzled LDS addresses are computed where they are used: hoisted
//   out of the loop they cost 40 more registers and spilled.  Nothing but the operands,
//   the accumulators and the softmax state lives across the streamed loop.
// LDS.  Only the streamed operand lives in LDS, in blocks of 64 rows: two
//   [64][128] bf16 images, 32 KiB per workgroup (K, V or Q, dO).  They use offd, a
//   256-B-row swizzle of its own: 16-B chunk c of row r sits at c ^ m(r),
//   m(r) = 2·(r & 7) + ((r >> 3) & 1).  A row is exactly the 64 banks, so a slot
//   (16 B) is 4 banks and 16 distinct slots are conflict-free.
//     row reads (ds_read_b128, 16 lanes = rows R..R+15 of one chunk): m is a
//       bijection of r & 15, so the 16 lanes hit 16 distinct slots;
//     transposed reads (ds_read_b64_tr_b16, 32 lanes = rows R..R+7, logical chunks c
//       and c ^ 1, both 8-B halves): the slots are c ^ m(r) and c ^ m(r) ^ 1, and m(r)
//       of 8 consecutive rows are 8 distinct values with the same bit 0: 16 distinct
//       slots.  off128's m(r) = r & 15 puts rows r and r ^ 1 on the same two slots
//       (2-way), which is why it is not used here: P·V, dQ, dK and dV all read
//       transposed, half of this file's LDS traffic;
//     image fill (16 lanes write the 16 chunks of one row): 16 distinct slots.
//   The output stage reuses the images after the last barrier.
// Causal work split.  One workgroup per owner block with a triangular loop, the grid
//   ordered heaviest block first (block index major, sequence-head minor), instead of
//   the d = 64 pairing (p, nbs-1-p): a second pass would have to rebuild operands and
//   accumulators inside the same register budget, which is what spilled at d = 64,
//   and with 64-row streamed blocks the triangle is cut at 64-key granularity.  The
//   last workgroups to start are the lightest, so the tail is at most one light block.
// Tile skipping.  len is uniform per workgroup and the causal bound uniform per wave:
//   no MFMA is issued for a 16-key score tile, a 32-key P·V / dQ slice or a 32-query
//   dK / dV step wholly past len or wholly past the wave's diagonal bound; only tiles
//   the diagonal crosses select on key > query.
// Grouped-query attention (the GQA = true instances; kv_heads K / V heads for `heads`
//   query heads, g = heads / kv_heads, qkv [T, (heads + 2·kv_heads)·128] = Q | K | V).
//   Forward and dQ keep the work split above; only the streamed K / V images come from
//   head h / g at the narrower row stride, both scalar.  dK / dV is owned by the KV
//   head: one workgroup per (sequence, KV head, 64-key block) keeps its keys' K and V in
//   registers and streams the Q / dO blocks of its g query heads one after the other
//   in ONE flattened loop (still one image load and two barriers per streamed block),
//   taking lse, D, the Q / dO columns and the dropout hash row from the current query
//   head.  dK / dV accumulate in the same registers over the whole group and are stored
//   once: no atomics, no fp32 scratch, no second pass, bit-repeatable.  (A workgroup per
//   query head would need g-way fp32 atomics into a scratch and a convert pass.)  The
//   GQA = false instances compile to the instructions they had before the template
//   argument existed; their trailing kv_heads argument is not read.
// Sliding window (the WIN = true instances, causal only: query i sees keys max(0, i - window + 1) .. i;
//   1 <= window < max_seqlen, a wider one runs the causal instances).  The window is a loop bound first:
//   a 128-query block starts its key loop at block max(0, blk·128 - (window - 1)) / 64, a 64-key block
//   ends its query loop (GQA: per query head) at the block of query `last key + window - 1`, so a
//   workgroup streams at most (OB + window - 1) / 64 + 1 blocks whatever the length, and loads no image
//   that none of its rows sees.  Per wave, tiles / slices / steps wholly below the band are skipped
//   like those above the diagonal, and only tiles the lower edge crosses select on query - key >=
//   window.  Forward: a wave's first blocks can lie wholly before a later row's window; such a row
//   subtracts 0 instead of its (still kMasked) maximum, so P = 0 and alpha acts on zeros until its first
//   visible key.  Grid: the bidirectional order (blocks of one (sequence, head) are neighbours: they
//   stream overlapping bands, and the work per block is nearly uniform, so heaviest-first has no
//   purpose), each (sequence, head) from its heavier end (queries: last block first; keys: first).
//   The other instances compile to the instructions they had before; their trailing window is not read.
#include "attn_tile.h"

namespace {

constexpr int HD = 128;  // head dim
constexpr int SB = 64;   // rows of a streamed block (one LDS image)
constexpr int IMG = SB * HD * 2;

__device__ __forceinline__ int offd(int row, int col) {
  const int m = ((row & 7) << 1) | ((row >> 3) & 1);
  return row * 256 + ((((col >> 3) ^ m) & 15) << 4) + (col & 7) * 2;
}
// 16x16x32 operand: columns k0..k0+7 of `row`
__device__ __forceinline__ short8 rd_rowd(const char* img, int row, int k0) {
  return *reinterpret_cast<const short8*>(img + offd(row, k0));
}
// rd_tr2 of attn_tile.h over an offd image: rows ra..ra+3 and rb..rb+3 of column cb + (lane & 15)
__device__ __forceinline__ short8 rd_tr2d(const char* img, int ra, int rb, int cb, int lane) {
  const int i = lane & 15;
  const int col = cb + 4 * (i & 3);
  const v4i16 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + offd(ra + (i >> 2), col)));
  const v4i16 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16*)(img + offd(rb + (i >> 2), col)));
  return short8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// two [64 rows][128] images: image i = columns col[i].. of rows row0.. of src[i] (row stride
// ld[i]), (+ bias[col]) (· scale[i]) where tf[i].  Thread t moves chunk t & 15 of rows
// (t >> 4) + 16k; only rows < live are loaded (and transformed), the others are zero.  Every
// load is issued before the first LDS store.
__device__ __forceinline__ void load_images(const bf16_t* const (&src)[2], const long (&ld)[2], long row0,
                                            const int (&col)[2], const float* __restrict__ bias, const bool (&tf)[2],
                                            const float (&scale)[2], int live, char* const (&img)[2], int tid) {
  const int r0 = tid >> 4, c = tid & 15;
  float bb[2][8];
  uint4 raw[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
    if (tf[i]) {  // compile-time after unrolling
      const float4 b0 = *reinterpret_cast<const float4*>(bias + col[i] + c * 8);
      const float4 b1 = *reinterpret_cast<const float4*>(bias + col[i] + c * 8 + 4);
      bb[i][0] = b0.x; bb[i][1] = b0.y; bb[i][2] = b0.z; bb[i][3] = b0.w;
      bb[i][4] = b1.x; bb[i][5] = b1.y; bb[i][6] = b1.z; bb[i][7] = b1.w;
    }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      raw[i][k] = make_uint4(0u, 0u, 0u, 0u);
      if (r0 + 16 * k < live)
        raw[i][k] = *reinterpret_cast<const uint4*>(src[i] + (row0 + r0 + 16 * k) * ld[i] + col[i] + c * 8);
    }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint4 v = raw[i][k];
      if (tf[i] && r0 + 16 * k < live) {
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int e = 0; e < 8; e++) f[e] = (f[e] + bb[i][e]) * scale[i];
        v = pack8(f);
      }
      *reinterpret_cast<uint4*>(img[i] + offd(r0 + 16 * k, c * 8)) = v;
    }
}

// zeros into columns colb..colb+127 of rows r0..r1-1 (the unowned rows), whole workgroup
__device__ __forceinline__ void zero_rows_d(bf16_t* __restrict__ dst, long ld, int colb, long r0, long r1, int tid) {
  for (long r = r0 + (tid >> 4); r < r1; r += 16)
    *reinterpret_cast<uint4*>(dst + r * ld + colb + (tid & 15) * 8) = make_uint4(0u, 0u, 0u, 0u);
}

// stage a wave's [16·RT rows][128] fp32 tiles t[dt][t2] (rows 16·t2 + fr, cols 16·dt + 4fq + r), scaled, as bf16
template <int RT>
__device__ __forceinline__ void stage_tile_d(char* st, const floatx4 (&t)[8][RT], float scale, int fr, int fq) {
#pragma unroll
  for (int dt = 0; dt < 8; dt++)
#pragma unroll
    for (int t2 = 0; t2 < RT; t2++)
      *reinterpret_cast<uint2*>(st + offd(t2 * 16 + fr, dt * 16 + 4 * fq)) =
          pack4(t[dt][t2][0] * scale, t[dt][t2][1] * scale, t[dt][t2][2] * scale, t[dt][t2][3] * scale);
}

// write the staged tile's rows < nrows to rows row0.. of dst column block colb (the others do not
// exist: neither stored nor summed); their column sums -> dbias[colb..] (nullable)
template <int RT>
__device__ __forceinline__ void store_tile_d(const char* st, bf16_t* __restrict__ dst, long row0, long ld, int colb,
                                             int nrows, float* __restrict__ dbias, int lane) {
  const int c = lane & 15;
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int it = 0; it < 4 * RT; it++) {
    const int r = it * 4 + (lane >> 4);
    if (r < nrows) {
      const uint4 v = *reinterpret_cast<const uint4*>(st + offd(r, c * 8));
      *reinterpret_cast<uint4*>(dst + (row0 + r) * ld + colb + c * 8) = v;
      float f[8];
      unpack8(v, f);
#pragma unroll
      for (int e = 0; e < 8; e++) cs[e] += f[e];
    }
  }
  if (dbias) {
#pragma unroll
    for (int o = 16; o < 64; o <<= 1)
#pragma unroll
      for (int e = 0; e < 8; e++) cs[e] += __shfl_xor(cs[e], o, 64);
    if (lane < 16)
#pragma unroll
      for (int e = 0; e < 8; e++) atomicAdd(dbias + colb + c * 8 + e, cs[e]);
  }
}

// the workgroup's owner block of OB rows; false: the block starts past its sequence.
// Bidirectional: blocks of one (sequence, head) are neighbours in the grid (they stream the
// same K / V).  Causal: block index major, heaviest first (HIGH_FIRST: the last query block
// streams the most keys; for dK / dV the first key block streams the most queries).  Window: the
// bidirectional order (neighbouring blocks stream overlapping bands), within one (sequence, head)
// from the end that can be heavier (HIGH_FIRST; the band is cut short at the sequence start for
// queries, at its end for keys), so that the grid does not end on the heaviest blocks.
struct OwnBlock {
  int blk, b, h, s0, len;
};
template <int OB, bool CAUSAL, bool HIGH_FIRST, bool WIN = false>
__device__ __forceinline__ bool own_block(const int* __restrict__ cu, int B, int T, int heads, int max_seqlen,
                                          OwnBlock& w) {
  const int nb = (max_seqlen + OB - 1) / OB;
  int sh;
  if constexpr (CAUSAL) {
    const int i = blockIdx.x / (B * heads);
    sh = blockIdx.x - i * (B * heads);
    w.blk = HIGH_FIRST ? nb - 1 - i : i;
  } else {
    sh = blockIdx.x / nb;
    w.blk = blockIdx.x - sh * nb;
    if constexpr (WIN && HIGH_FIRST) w.blk = nb - 1 - w.blk;
  }
  w.b = sh / heads;
  w.h = sh - w.b * heads;
  w.s0 = max(cu[w.b], 0);
  w.len = min(cu[w.b + 1], T) - w.s0;  // a table the host validated; the clamps only keep a stale one in bounds
  return w.blk * OB < w.len;
}

// Grouped-query attention (GQA instances): qkv rows hold `heads` query heads, then kv_heads K heads,
// then kv_heads V heads; query head h reads KV head h / g, g = heads / kv_heads.  The row width and
// the K / V columns are uniform over the workgroup (scalar registers).  Multi-head instances
// (GQA = false) ignore kv_heads.
template <bool GQA>
__device__ __forceinline__ int kv_head(int h, int heads, int kv_heads) {
  if constexpr (GQA) return h / (heads / kv_heads);
  return h;
}

// forward: workgroup per (sequence, head, block of 64·RT queries); wave w owns queries 16·RT·w.. as
// register operands, streams 64-key blocks (K, V images), online softmax per block, P feeds P·V
// from registers
template <int RT, bool CAUSAL, bool GQA, bool WIN>
__global__ __launch_bounds__(256, 2) KFA_NO_PK_F32 void attn_d128_fwd_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ bqkv, const int* __restrict__ cu,
    bf16_t* __restrict__ out, float* __restrict__ lse, int B, int T, int heads, int max_seqlen, float qscale,
    uint32_t thresh, float dscale, uint64_t seed, int kv_heads, int window) {
  static_assert(CAUSAL || !WIN, "a window is a band below the diagonal");
  constexpr int OB = 64 * RT, WR = 16 * RT;
  __shared__ __attribute__((aligned(16))) char sm[2 * IMG];  // K, V images (32 KiB)
  char* Ki = sm;
  char* Vi = sm + IMG;
  const int tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6, fr0 = lane0 & 15, fq0 = lane0 >> 4;
  OwnBlock w;
  if (!own_block<OB, CAUSAL && !WIN, true, WIN>(cu, B, T, heads, max_seqlen, w)) return;  // uniform, before any barrier
  const int h = w.h, H = heads * HD;
  const int hk = kv_head<GQA>(h, heads, kv_heads), VC = GQA ? H + kv_heads * HD : 2 * H;  // KV head, V's first column
  const long W3 = GQA ? (long)H + 2L * kv_heads * HD : 3L * H, q0 = (long)w.s0 + (long)w.blk * OB;
  if (w.blk == 0 && w.b == B - 1) zero_rows_d(out, H, h * HD, (long)w.s0 + w.len, T, tid);
  const int qlive = min(OB, w.len - w.blk * OB);
  const int qb = wave * WR, qabs = w.blk * OB + qb;  // the wave's first query: in the block, in the sequence
  const bool wlive = qb < qlive;                     // else: this wave's queries do not exist
  short8 qreg[RT][4] = {};
  if (wlive) {
#pragma unroll
    for (int qt = 0; qt < RT; qt++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const int row = qb + 16 * qt + fr0, c = h * HD + ks * 32 + fq0 * 8;
        // scores in log2 units: the softmax exponent is one subtraction + v_exp_f32
        qreg[qt][ks] = row_operand<true>(qkv + (q0 + row) * W3 + c, row < qlive, bqkv + c, qscale * kLog2e);
      }
  }
  float m[RT], l[RT];
  floatx4 o[8][RT];
#pragma unroll
  for (int qt = 0; qt < RT; qt++) {
    m[qt] = kMasked;
    l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 8; dt++) o[dt][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // keys some query of the block sees: the loop bound is the causal mask below the diagonal, and
  // (window) the first block is the one that holds the first key of the block's first query
  const int nkb = ((CAUSAL ? w.blk * OB + qlive : w.len) + SB - 1) / SB;
  const int j0 = WIN ? max(0, w.blk * OB - (window - 1)) / SB : 0;
  for (int j = j0; j < nkb; j++) {
    const int klive = min(SB, w.len - j * SB);  // >= 1
    if (j > j0) __syncthreads();                // every wave is done with key block j-1
    {
      const int col[2] = {H + hk * HD, VC + hk * HD};
      const bool tf[2] = {true, true};
      const float sc[2] = {1.f, 1.f};
      char* const img[2] = {Ki, Vi};
      const bf16_t* const src[2] = {qkv, qkv};
      const long ld[2] = {W3, W3};
      load_images(src, ld, (long)w.s0 + (long)j * SB, col, bqkv, tf, sc, klive, img, tid);
    }
    __syncthreads();
    // keys of this block the wave's queries can see: the live ones, causal: up to its last query
    const int kend = CAUSAL ? min(klive, qabs + WR - j * SB) : klive;
    // window: keys of this block before kbeg are before the window of the wave's first query, so of all
    const int kbeg = WIN ? qabs - (window - 1) - j * SB : 0;
    if (!wlive || kend <= 0 || (WIN && kbeg >= kend)) continue;
    // the lane's indices are formed again in each block: hoisted out of the loop, the LDS addresses
    // derived from them would not fit the register budget
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int fr = lane & 15, fq = lane >> 4;
    // s[kt][qt][r] = score(q = qb + 16qt + fr, key = 16kt + 4fq + r); tiles past kend (window: or
    // before kbeg) stay 0 until masked
    floatx4 s[4][RT];
#pragma unroll
    for (int kt = 0; kt < 4; kt++) {
#pragma unroll
      for (int qt = 0; qt < RT; qt++) s[kt][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
      if (kt * 16 < kend && (!WIN || kt * 16 + 15 >= kbeg)) {
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
          const short8 a = rd_rowd(Ki, kt * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
          for (int qt = 0; qt < RT; qt++) s[kt][qt] = mma(a, qreg[qt][ks], s[kt][qt]);
        }
      }
    }
    if constexpr (CAUSAL) {
      // tiles the diagonal crosses or that lie above it: key > query is masked.  A live query's keys
      // at or past klive are past the query too, so this is the tail rule as well.
      if (j * SB + SB - 1 > qabs) {
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
          if (j * SB + kt * 16 + 15 > qabs) {
#pragma unroll
            for (int qt = 0; qt < RT; qt++)
#pragma unroll
              for (int r = 0; r < 4; r++)
                s[kt][qt][r] = above_diag(qabs + 16 * qt + fr, j * SB + kt * 16 + 4 * fq + r, kMasked, s[kt][qt][r]);
          }
      }
      if constexpr (WIN) {
        // tiles the lower window edge crosses or that lie before it (the wave's last query does not see
        // the tile's first key): query - key >= window is masked
        if (qabs + WR - 1 - j * SB >= window) {
#pragma unroll
          for (int kt = 0; kt < 4; kt++)
            if (qabs + WR - 1 - (j * SB + kt * 16) >= window) {
#pragma unroll
              for (int qt = 0; qt < RT; qt++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                  s[kt][qt][r] = above_diag(window - 1, qabs + 16 * qt + fr - (j * SB + kt * 16 + 4 * fq + r), kMasked,
                                            s[kt][qt][r]);
            }
        }
      }
    } else if (klive < SB) {
#pragma unroll
      for (int kt = 0; kt < 4; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (kt * 16 + 4 * fq + r >= klive) {
#pragma unroll
            for (int qt = 0; qt < RT; qt++) s[kt][qt][r] = kMasked;
          }
    }
#pragma unroll
    for (int qt = 0; qt < RT; qt++) {
      float mx = kMasked;
#pragma unroll
      for (int kt = 0; kt < 4; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) mx = fmaxf(mx, s[kt][qt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // finite: key 0 of the sequence is live and visible to every query, and block 0 comes first.
      // Window: the wave's first blocks can lie wholly before a later row's window; while such a row has
      // seen no key (mn == kMasked) 0 is subtracted instead, so P = exp2(kMasked) = 0 and alpha = 0 on
      // l = 0, O = 0, until its first visible key makes mn finite (every query sees itself)
      const float mn = fmaxf(m[qt], mx);
      const float sub = WIN && mn == kMasked ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(m[qt] - sub);
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; kt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float e = __builtin_amdgcn_exp2f(s[kt][qt][r] - sub);
          s[kt][qt][r] = e;
          sum += e;
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l[qt] = l[qt] * alpha + sum;
      m[qt] = mn;
#pragma unroll
      for (int dt = 0; dt < 8; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[dt][qt][r] *= alpha;
      if (thresh) {
        const uint64_t row = (uint64_t)h * T + (uint64_t)(q0 + qb + qt * 16 + fr);
#pragma unroll
        for (int kp = 0; kp < 2; kp++)
          if (kp * 32 < kend && (!WIN || kp * 32 + 31 >= kbeg)) {  // a slice past kend (before kbeg) holds P = 0 only
#pragma unroll
            for (int r = 0; r < 4; r++) {
              const uint32_t hh = attn_pair_hash(seed, row, max_seqlen, j * SB + 32 * kp + 4 * fq + r);
              s[2 * kp][qt][r] = keep_lo(hh, thresh) ? s[2 * kp][qt][r] * dscale : 0.f;
              s[2 * kp + 1][qt][r] = keep_hi(hh, thresh) ? s[2 * kp + 1][qt][r] * dscale : 0.f;
            }
          }
      }
    }
    // Oᵀ += Vᵀ·Pdᵀ from registers: tiles 2ks, 2ks+1 give this lane keys {32ks + 4fq + r,
    // 32ks + 16 + 4fq + r}, V's rows are read in the same order
#pragma unroll
    for (int ks = 0; ks < 2; ks++)
      if (ks * 32 < kend && (!WIN || ks * 32 + 31 >= kbeg)) {
        short8 b[RT];
#pragma unroll
        for (int qt = 0; qt < RT; qt++) b[qt] = pack_pair(s[2 * ks][qt], s[2 * ks + 1][qt]);
        const int ra = 32 * ks + 4 * fq;
#pragma unroll
        for (int dt = 0; dt < 8; dt++) {
          const short8 a = rd_tr2d(Vi, ra, ra + 16, dt * 16, lane);
#pragma unroll
          for (int qt = 0; qt < RT; qt++) o[dt][qt] = mma(a, b[qt], o[dt][qt]);
        }
      }
  }
  __syncthreads();  // every wave is done with the images: they become the O stage
  if (!wlive) return;
#pragma unroll
  for (int qt = 0; qt < RT; qt++) {
    const int q = qb + qt * 16 + fr0;
    const float inv = 1.f / l[qt];
    if (fq0 == 0 && q < qlive) lse[(long)h * T + q0 + q] = (m[qt] + __log2f(l[qt])) * kLn2;  // natural-log units
#pragma unroll
    for (int dt = 0; dt < 8; dt++)
#pragma unroll
      for (int r = 0; r < 4; r++) o[dt][qt][r] *= inv;
  }
  char* st = sm + wave * (WR * HD * 2);
  stage_tile_d<RT>(st, o, 1.f, fr0, fq0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  store_tile_d<RT>(st, out, q0 + qb, H, h * HD, qlive - qb, nullptr, lane0);
}

// D[h][t] = Σ_d dO[t][h·128 + d]·O[t][h·128 + d] of the owned rows t < cu[B]; one thread per (row, head)
__global__ KFA_NO_PK_F32 void attn_d128_rowdot_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
                                                      const int* __restrict__ cu, float* __restrict__ D, int B, int T,
                                                      int heads) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)min(cu[B], T) * heads) return;
  const long tok = t / heads;
  const int h = (int)(t - tok * heads), H = heads * HD;
  const uint4* g = reinterpret_cast<const uint4*>(dout + tok * H + h * HD);
  const uint4* o = reinterpret_cast<const uint4*>(out + tok * H + h * HD);
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < HD / 8; c++) {
    float a[8], b[8];
    unpack8(g[c], a);
    unpack8(o[c], b);
#pragma unroll
    for (int e = 0; e < 8; e++) acc += a[e] * b[e];
  }
  D[(long)h * T + tok] = acc;
}

// key-owner dK / dV: workgroup per (sequence, head, block of 64·RT keys); wave w owns keys 16·RT·w..
// (K and V rows as register operands) and streams 64-query blocks (Q, dO images); causal: from the
// query block that holds its first key on.  GQA: the owner is a KV head and the Q / dO blocks of
// its g query heads stream past the same K / V registers and accumulators
template <int RT, bool CAUSAL, bool GQA, bool WIN>
__global__ __launch_bounds__(256, 2) KFA_NO_PK_F32 void attn_d128_bwd_kv_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ bqkv, const int* __restrict__ cu,
    const float* __restrict__ lse, const float* __restrict__ Dq, const bf16_t* __restrict__ dout,
    bf16_t* __restrict__ dqkv, float* __restrict__ dbqkv, int B, int T, int heads, int max_seqlen, float qscale,
    uint32_t thresh, float dscale, uint64_t seed, int kv_heads, int window) {
  static_assert(CAUSAL || !WIN, "a window is a band below the diagonal");
  constexpr int OB = 64 * RT, WR = 16 * RT;
  __shared__ __attribute__((aligned(16))) char sm[2 * IMG];  // Q, dO images (32 KiB)
  char* Qi = sm;
  char* Gi = sm + IMG;
  const int tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6, fr0 = lane0 & 15, fq0 = lane0 >> 4;
  OwnBlock w;
  // GQA: the owner is a KV head; w.h counts KV heads and the query heads w.h·g .. w.h·g + g-1 stream past it
  if (!own_block<OB, CAUSAL && !WIN, false, WIN>(cu, B, T, GQA ? kv_heads : heads, max_seqlen, w)) return;  // uniform, before any barrier
  const int hk = w.h, H = heads * HD, g = GQA ? heads / kv_heads : 1, VC = GQA ? H + kv_heads * HD : 2 * H;
  const long W3 = GQA ? (long)H + 2L * kv_heads * HD : 3L * H, k0 = (long)w.s0 + (long)w.blk * OB;
  if (w.blk == 0 && w.b == B - 1) {
    zero_rows_d(dqkv, W3, H + hk * HD, (long)w.s0 + w.len, T, tid);
    zero_rows_d(dqkv, W3, VC + hk * HD, (long)w.s0 + w.len, T, tid);
  }
  const int klive = min(OB, w.len - w.blk * OB), nqb = (w.len + SB - 1) / SB;
  const int kw = wave * WR, kabs = w.blk * OB + kw;  // the wave's first key: in the block, in the sequence
  const bool wlive = kw < klive;                     // else: this wave's keys do not exist
  short8 kreg[RT][4] = {}, vreg[RT][4] = {};
  bool keyok[RT];
#pragma unroll
  for (int kt = 0; kt < RT; kt++) {
    const int row = kw + 16 * kt + fr0;
    keyok[kt] = wlive && row < klive;
    if (wlive) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const int c = hk * HD + ks * 32 + fq0 * 8;
        kreg[kt][ks] = row_operand<true>(qkv + (k0 + row) * W3 + H + c, keyok[kt], bqkv + H + c, 1.f);
        vreg[kt][ks] = row_operand<true>(qkv + (k0 + row) * W3 + VC + c, keyok[kt], bqkv + VC + c, 1.f);
      }
    }
  }
  floatx4 dvT[8][RT], dkT[8][RT];
#pragma unroll
  for (int dt = 0; dt < 8; dt++)
#pragma unroll
    for (int kt = 0; kt < RT; kt++) dvT[dt][kt] = dkT[dt][kt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int i0 = CAUSAL ? (w.blk * OB) / SB : 0;  // the loop bound is the causal mask above the diagonal
  // window: the last streamed block holds the last query that sees the block's last key (or the sequence end)
  const int nqe = WIN ? min(w.len - 1, w.blk * OB + klive - 1 + window - 1) / SB + 1 : nqb;
  // one flattened loop over (query head of the group, query block): the accumulators, the barriers
  // and the image loads do not know where one query head ends and the next begins
  const int nq = nqe - i0;       // query blocks streamed per query head
  int h = hk * g, wrap = nqe;    // the streamed block's query head; the counter at which the next one begins
  for (int u = i0; u < i0 + nq * g; u++) {
    int i = u;  // the streamed query block
    if constexpr (GQA) {
      if (u == wrap) {
        wrap += nq;
        h++;
      }
      i = u - (wrap - nqe);
    }
    const int qlive = min(SB, w.len - i * SB);
    const long qrow0 = (long)w.s0 + (long)i * SB;
    if (u > i0) __syncthreads();  // every wave is done with the previous Q / dO images
    {
      const int col[2] = {h * HD, h * HD};
      const bool tf[2] = {true, false};
      const float sc[2] = {qscale, 1.f};
      char* const img[2] = {Qi, Gi};
      const bf16_t* const src[2] = {qkv, dout};
      const long ld[2] = {W3, (long)H};
      load_images(src, ld, qrow0, col, bqkv, tf, sc, qlive, img, tid);
    }
    // lse·log2(e) and D of query `lane` of the block (0 where there is no query)
    float lqv = 0.f, ddv = 0.f;
    if (wlive && lane0 < qlive) {
      lqv = lse[(long)h * T + qrow0 + lane0] * kLog2e;
      ddv = Dq[(long)h * T + qrow0 + lane0];
    }
    __syncthreads();
    if (!wlive) continue;
    int lane = lane0;  // as in the forward
    asm volatile("" : "+v"(lane));
    const int fr = lane & 15, fq = lane >> 4;
#pragma unroll
    for (int j = 0; j < 2; j++) {  // 32-query steps that hold a query the wave's keys are visible to
      if (32 * j >= qlive) break;
      const int qa = i * SB + 32 * j;  // the step's first query in the sequence
      if (CAUSAL && qa + 31 < kabs) continue;
      if (WIN && qa - (kabs + WR - 1) >= window) break;  // no query of this or a later step sees a key of the wave
      const bool diag = CAUSAL && qa < kabs + WR - 1;  // some pair of the step has key > query
      const bool low = WIN && qa + 31 - kabs >= window;  // some pair of the step has query - key >= window
      // s / dp[qt][kt][r]: (q = 32j + 16qt + 4fq + r, key = kw + 16kt + fr)
      floatx4 s[2][RT], dp[2][RT];
#pragma unroll
      for (int qt = 0; qt < 2; qt++)
#pragma unroll
        for (int kt = 0; kt < RT; kt++) s[qt][kt] = dp[qt][kt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ks++)
#pragma unroll
        for (int qt = 0; qt < 2; qt++) {
          const short8 aq = rd_rowd(Qi, 32 * j + 16 * qt + fr, ks * 32 + fq * 8);
          const short8 ag = rd_rowd(Gi, 32 * j + 16 * qt + fr, ks * 32 + fq * 8);
#pragma unroll
          for (int kt = 0; kt < RT; kt++) {
            s[qt][kt] = mma(aq, kreg[kt][ks], s[qt][kt]);
            dp[qt][kt] = mma(ag, vreg[kt][ks], dp[qt][kt]);
          }
        }
      floatx4 pd[2][RT], ds[2][RT];
#pragma unroll
      for (int qt = 0; qt < 2; qt++) {
        const int qb4 = 32 * j + 16 * qt + 4 * fq;  // query within the block
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const float D = __shfl(ddv, qb4 + r, 64);
          const float lq = __shfl(lqv, qb4 + r, 64);
          const bool qok = qb4 + r < qlive;
          // one hash per pair (key with bit 4 clear, key + 16): tile kt holds its low or its high half
          const uint32_t hh = thresh ? attn_pair_hash(seed, (uint64_t)h * T + (uint64_t)(qrow0 + qb4 + r), max_seqlen,
                                                      (kabs + fr) & ~16)
                                     : 0u;
#pragma unroll
          for (int kt = 0; kt < RT; kt++) {
            // a pair with no query or no key (or, causal, above the diagonal) has P = 0, whatever lse holds
            bool ok = qok && keyok[kt];
            if (diag) ok = ok && kabs + 16 * kt + fr <= i * SB + qb4 + r;
            if (low) ok = ok && i * SB + qb4 + r - (kabs + 16 * kt + fr) < window;
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[qt][kt][r], kLog2e, -lq)) : 0.f;
            float g = dp[qt][kt][r], pv = p;
            if (thresh) {
              const bool keep = (((kw >> 4) + kt) & 1) ? keep_hi(hh, thresh) : keep_lo(hh, thresh);
              pv = keep ? p * dscale : 0.f;
              g = keep ? g * dscale : 0.f;
            }
            pd[qt][kt][r] = pv;
            ds[qt][kt][r] = p * (g - D);
          }
        }
      }
      const int ra = 32 * j + 4 * fq, rb = ra + 16;
      short8 bp[RT], bs[RT];
#pragma unroll
      for (int kt = 0; kt < RT; kt++) {
        bp[kt] = pack_pair(pd[0][kt], pd[1][kt]);
        bs[kt] = pack_pair(ds[0][kt], ds[1][kt]);
      }
#pragma unroll
      for (int dt = 0; dt < 8; dt++) {
        const short8 gtr = rd_tr2d(Gi, ra, rb, dt * 16, lane);
        const short8 qtr = rd_tr2d(Qi, ra, rb, dt * 16, lane);
#pragma unroll
        for (int kt = 0; kt < RT; kt++) {
          dvT[dt][kt] = mma(gtr, bp[kt], dvT[dt][kt]);
          dkT[dt][kt] = mma(qtr, bs[kt], dkT[dt][kt]);
        }
      }
    }
  }
  __syncthreads();  // the images become the output stage
  if (!wlive) return;
  char* st = sm + wave * (2 * WR * HD * 2);
  stage_tile_d<RT>(st, dkT, 1.f, fr0, fq0);
  stage_tile_d<RT>(st + WR * HD * 2, dvT, 1.f, fr0, fq0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  store_tile_d<RT>(st, dqkv, k0 + kw, W3, H + hk * HD, klive - kw, dbqkv, lane0);
  store_tile_d<RT>(st + WR * HD * 2, dqkv, k0 + kw, W3, VC + hk * HD, klive - kw, dbqkv, lane0);
}

// query-owner dQ = dS·K: workgroup per (sequence, head, block of 64·RT queries); wave w owns queries
// 16·RT·w.. (Q and dO rows as register operands) and streams 64-key blocks (K, V images), one 32-key
// slice (a dropout hash pair and one dQ k-step) at a time
template <int RT, bool CAUSAL, bool GQA, bool WIN>
__global__ __launch_bounds__(256, 2) KFA_NO_PK_F32 void attn_d128_bwd_q_kernel(
    const bf16_t* __restrict__ qkv, const float* __restrict__ bqkv, const int* __restrict__ cu,
    const float* __restrict__ lse, const float* __restrict__ Dq, const bf16_t* __restrict__ dout,
    bf16_t* __restrict__ dqkv, float* __restrict__ dbqkv, int B, int T, int heads, int max_seqlen, float qscale,
    uint32_t thresh, float dscale, uint64_t seed, int kv_heads, int window) {
  static_assert(CAUSAL || !WIN, "a window is a band below the diagonal");
  constexpr int OB = 64 * RT, WR = 16 * RT;
  __shared__ __attribute__((aligned(16))) char sm[2 * IMG];  // K, V images (32 KiB)
  char* Ki = sm;
  char* Vi = sm + IMG;
  const int tid = threadIdx.x, lane0 = tid & 63, wave = tid >> 6, fr0 = lane0 & 15, fq0 = lane0 >> 4;
  OwnBlock w;
  if (!own_block<OB, CAUSAL && !WIN, true, WIN>(cu, B, T, heads, max_seqlen, w)) return;  // uniform, before any barrier
  const int h = w.h, H = heads * HD;
  const int hk = kv_head<GQA>(h, heads, kv_heads), VC = GQA ? H + kv_heads * HD : 2 * H;  // KV head, V's first column
  const long W3 = GQA ? (long)H + 2L * kv_heads * HD : 3L * H, q0 = (long)w.s0 + (long)w.blk * OB;
  if (w.blk == 0 && w.b == B - 1) zero_rows_d(dqkv, W3, h * HD, (long)w.s0 + w.len, T, tid);
  const int qlive = min(OB, w.len - w.blk * OB);
  const int qb = wave * WR, qabs = w.blk * OB + qb;
  const bool wlive = qb < qlive;
  short8 qreg[RT][4] = {}, greg[RT][4] = {};
  float lq[RT], Dv[RT];
  bool qok[RT];
#pragma unroll
  for (int qt = 0; qt < RT; qt++) {
    const int row = qb + 16 * qt + fr0;
    qok[qt] = wlive && row < qlive;
    lq[qt] = Dv[qt] = 0.f;
    if (wlive) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const int c = h * HD + ks * 32 + fq0 * 8;
        qreg[qt][ks] = row_operand<true>(qkv + (q0 + row) * W3 + c, qok[qt], bqkv + c, qscale);
        greg[qt][ks] = row_operand<false>(dout + (q0 + row) * H + c, qok[qt], nullptr, 1.f);
      }
    }
    if (qok[qt]) {
      lq[qt] = lse[(long)h * T + q0 + row] * kLog2e;
      Dv[qt] = Dq[(long)h * T + q0 + row];
    }
  }
  floatx4 dqT[8][RT];
#pragma unroll
  for (int dt = 0; dt < 8; dt++)
#pragma unroll
    for (int qt = 0; qt < RT; qt++) dqT[dt][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int nkb = ((CAUSAL ? w.blk * OB + qlive : w.len) + SB - 1) / SB;
  const int j0 = WIN ? max(0, w.blk * OB - (window - 1)) / SB : 0;  // as in the forward
  for (int j = j0; j < nkb; j++) {
    const int klive = min(SB, w.len - j * SB);
    if (j > j0) __syncthreads();  // every wave is done with key block j-1
    {
      const int col[2] = {H + hk * HD, VC + hk * HD};
      const bool tf[2] = {true, true};
      const float sc[2] = {1.f, 1.f};
      char* const img[2] = {Ki, Vi};
      const bf16_t* const src[2] = {qkv, qkv};
      const long ld[2] = {W3, W3};
      load_images(src, ld, (long)w.s0 + (long)j * SB, col, bqkv, tf, sc, klive, img, tid);
    }
    __syncthreads();
    const int kend = CAUSAL ? min(klive, qabs + WR - j * SB) : klive;
    const int kbeg = WIN ? qabs - (window - 1) - j * SB : 0;  // as in the forward
    if (!wlive || kend <= 0 || (WIN && kbeg >= kend)) continue;
    int lane = lane0;  // as in the forward
    asm volatile("" : "+v"(lane));
    const int fr = lane & 15, fq = lane >> 4;
    // s / dp[u][qt][r]: (q = qb + 16qt + fr, key = 32c + 16u + 4fq + r), dP(q, key) = dO[q]·V[key]
#pragma unroll
    for (int c = 0; c < 2; c++) {
      if (c * 32 >= kend) break;
      if (WIN && c * 32 + 31 < kbeg) continue;
      const bool diag = CAUSAL && j * SB + c * 32 + 31 > qabs;  // some pair of the slice has key > query
      const bool low = WIN && qabs + WR - 1 - (j * SB + c * 32) >= window;  // some pair has query - key >= window
      floatx4 s[2][RT], dp[2][RT];
#pragma unroll
      for (int u = 0; u < 2; u++) {
#pragma unroll
        for (int qt = 0; qt < RT; qt++) s[u][qt] = dp[u][qt] = floatx4{0.f, 0.f, 0.f, 0.f};
        if (c * 32 + u * 16 < kend && (!WIN || c * 32 + u * 16 + 15 >= kbeg)) {
#pragma unroll
          for (int ks = 0; ks < 4; ks++) {
            const short8 ak = rd_rowd(Ki, c * 32 + u * 16 + fr, ks * 32 + fq * 8);
            const short8 av = rd_rowd(Vi, c * 32 + u * 16 + fr, ks * 32 + fq * 8);
#pragma unroll
            for (int qt = 0; qt < RT; qt++) {
              s[u][qt] = mma(ak, qreg[qt][ks], s[u][qt]);
              dp[u][qt] = mma(av, greg[qt][ks], dp[u][qt]);
            }
          }
        }
      }
#pragma unroll
      for (int qt = 0; qt < RT; qt++) {
        const uint64_t row = (uint64_t)h * T + (uint64_t)(q0 + qb + qt * 16 + fr);
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int key = c * 32 + 4 * fq + r;
          const uint32_t hh = thresh ? attn_pair_hash(seed, row, max_seqlen, j * SB + key) : 0u;
#pragma unroll
          for (int u = 0; u < 2; u++) {
            bool ok = qok[qt] && key + 16 * u < klive;  // else P = 0, whatever lse holds
            if (diag) ok = ok && j * SB + key + 16 * u <= qabs + 16 * qt + fr;
            if (low) ok = ok && qabs + 16 * qt + fr - (j * SB + key + 16 * u) < window;
            const float p = ok ? __builtin_amdgcn_exp2f(fmaf(s[u][qt][r], kLog2e, -lq[qt])) : 0.f;
            float g = dp[u][qt][r];
            if (thresh) g = (u ? keep_hi(hh, thresh) : keep_lo(hh, thresh)) ? g * dscale : 0.f;
            s[u][qt][r] = p * (g - Dv[qt]);  // dS
          }
        }
      }
      const int ra = 32 * c + 4 * fq, rb = ra + 16;
      short8 bs[RT];
#pragma unroll
      for (int qt = 0; qt < RT; qt++) bs[qt] = pack_pair(s[0][qt], s[1][qt]);
#pragma unroll
      for (int dt = 0; dt < 8; dt++) {
        const short8 ktr = rd_tr2d(Ki, ra, rb, dt * 16, lane);
#pragma unroll
        for (int qt = 0; qt < RT; qt++) dqT[dt][qt] = mma(ktr, bs[qt], dqT[dt][qt]);
      }
    }
  }
  __syncthreads();  // the images become the output stage
  if (!wlive) return;
  char* st = sm + wave * (WR * HD * 2);
  stage_tile_d<RT>(st, dqT, qscale, fr0, fq0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  store_tile_d<RT>(st, dqkv, q0 + qb, W3, h * HD, qlive - qb, dbqkv, lane0);
}

// 16-row tiles per wave: owner blocks of 128 queries (forward, dQ) and of 64 keys (dK / dV)
constexpr int FWD_RT = 2, DQ_RT = 2, KV_RT = 1;

template <bool CAUSAL>
void launch_fwd(const void* qkv, const float* bqkv, const int* cu, void* out, float* lse, int B, int T, int max_seqlen,
                int heads, int kv_heads, float qscale, uint32_t th, float ds, uint64_t seed, hipStream_t st) {
  const dim3 grid((unsigned)((long)B * heads * ((max_seqlen + 64 * FWD_RT - 1) / (64 * FWD_RT))));
  if (kv_heads == heads)
    hipLaunchKernelGGL((attn_d128_fwd_kernel<FWD_RT, CAUSAL, false, false>), grid, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, (bf16_t*)out, lse, B, T, heads, max_seqlen, qscale, th, ds, seed, kv_heads, 0);
  else
    hipLaunchKernelGGL((attn_d128_fwd_kernel<FWD_RT, CAUSAL, true, false>), grid, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, (bf16_t*)out, lse, B, T, heads, max_seqlen, qscale, th, ds, seed, kv_heads, 0);
}

// dK / dV then dQ.  GQA: the dK / dV grid is over KV heads, a workgroup does its group's g query heads
template <bool CAUSAL>
void launch_bwd(const void* qkv, const float* bqkv, const int* cu, const float* lse, const float* work,
                const void* dout, void* dqkv, float* dbqkv, int B, int T, int max_seqlen, int heads, int kv_heads,
                float qscale, uint32_t th, float ds, uint64_t seed, hipStream_t st) {
  const dim3 gkv((unsigned)((long)B * kv_heads * ((max_seqlen + 64 * KV_RT - 1) / (64 * KV_RT))));
  const dim3 gq((unsigned)((long)B * heads * ((max_seqlen + 64 * DQ_RT - 1) / (64 * DQ_RT))));
  if (kv_heads == heads) {
    hipLaunchKernelGGL((attn_d128_bwd_kv_kernel<KV_RT, CAUSAL, false, false>), gkv, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale, th,
                       ds, seed, kv_heads, 0);
    hipLaunchKernelGGL((attn_d128_bwd_q_kernel<DQ_RT, CAUSAL, false, false>), gq, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale, th,
                       ds, seed, kv_heads, 0);
  } else {
    hipLaunchKernelGGL((attn_d128_bwd_kv_kernel<KV_RT, CAUSAL, true, false>), gkv, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale, th,
                       ds, seed, kv_heads, 0);
    hipLaunchKernelGGL((attn_d128_bwd_q_kernel<DQ_RT, CAUSAL, true, false>), gq, dim3(256), 0, st, (const bf16_t*)qkv, bqkv,
                       cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale, th,
                       ds, seed, kv_heads, 0);
  }
}

// The windowed instances (causal, 1 <= window < max_seqlen): the same grids in the bidirectional order
void launch_fwd_window(const void* qkv, const float* bqkv, const int* cu, void* out, float* lse, int B, int T,
                       int max_seqlen, int heads, int kv_heads, int window, float qscale, uint32_t th, float ds,
                       uint64_t seed, hipStream_t st) {
  const dim3 grid((unsigned)((long)B * heads * ((max_seqlen + 64 * FWD_RT - 1) / (64 * FWD_RT))));
  if (kv_heads == heads)
    hipLaunchKernelGGL((attn_d128_fwd_kernel<FWD_RT, true, false, true>), grid, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, (bf16_t*)out, lse, B, T, heads, max_seqlen, qscale, th, ds, seed, kv_heads, window);
  else
    hipLaunchKernelGGL((attn_d128_fwd_kernel<FWD_RT, true, true, true>), grid, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, (bf16_t*)out, lse, B, T, heads, max_seqlen, qscale, th, ds, seed, kv_heads, window);
}

void launch_bwd_window(const void* qkv, const float* bqkv, const int* cu, const float* lse, const float* work,
                       const void* dout, void* dqkv, float* dbqkv, int B, int T, int max_seqlen, int heads,
                       int kv_heads, int window, float qscale, uint32_t th, float ds, uint64_t seed, hipStream_t st) {
  const dim3 gkv((unsigned)((long)B * kv_heads * ((max_seqlen + 64 * KV_RT - 1) / (64 * KV_RT))));
  const dim3 gq((unsigned)((long)B * heads * ((max_seqlen + 64 * DQ_RT - 1) / (64 * DQ_RT))));
  if (kv_heads == heads) {
    hipLaunchKernelGGL((attn_d128_bwd_kv_kernel<KV_RT, true, false, true>), gkv, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale,
                       th, ds, seed, kv_heads, window);
    hipLaunchKernelGGL((attn_d128_bwd_q_kernel<DQ_RT, true, false, true>), gq, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale,
                       th, ds, seed, kv_heads, window);
  } else {
    hipLaunchKernelGGL((attn_d128_bwd_kv_kernel<KV_RT, true, true, true>), gkv, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale,
                       th, ds, seed, kv_heads, window);
    hipLaunchKernelGGL((attn_d128_bwd_q_kernel<DQ_RT, true, true, true>), gq, dim3(256), 0, st, (const bf16_t*)qkv,
                       bqkv, cu, lse, work, (const bf16_t*)dout, (bf16_t*)dqkv, dbqkv, B, T, heads, max_seqlen, qscale,
                       th, ds, seed, kv_heads, window);
  }
}

}  // namespace

// blocks of the largest d = 128 grid (attention.hip's entry points check it against 2^31): the
// 64-key dK / dV blocks of `heads` heads, which is also above the 128-query grids of a GQA launch
long kfa_attn_d128_blocks(int B, int max_seqlen, int heads) {
  return (long)B * heads * ((max_seqlen + 64 * KV_RT - 1) / (64 * KV_RT));
}

// The d = 128 side of kfa_attn_varlen_fwd / kfa_attn_causal_fwd / kfa_attn_gqa_fwd / kfa_attn_window_fwd:
// arguments already checked there; kv_heads == heads: the multi-head kernels; window: 0 for none, else
// >= 1 with causal.  A window that covers every sequence (>= max_seqlen) masks nothing below the
// diagonal: it runs the causal instances.
int kfa_attn_d128_fwd(bool causal, int window, const void* qkv, const float* bqkv, const int* cu, void* out,
                      float* lse, int B, int T, int max_seqlen, int heads, int kv_heads, float qscale, uint32_t th,
                      float ds, uint64_t seed, hipStream_t st) {
  if (causal && window > 0 && window < max_seqlen)
    launch_fwd_window(qkv, bqkv, cu, out, lse, B, T, max_seqlen, heads, kv_heads, window, qscale, th, ds, seed, st);
  else if (causal)
    launch_fwd<true>(qkv, bqkv, cu, out, lse, B, T, max_seqlen, heads, kv_heads, qscale, th, ds, seed, st);
  else
    launch_fwd<false>(qkv, bqkv, cu, out, lse, B, T, max_seqlen, heads, kv_heads, qscale, th, ds, seed, st);
  return kfa_status();
}

// The d = 128 side of kfa_attn_varlen_bwd / kfa_attn_causal_bwd / kfa_attn_gqa_bwd / kfa_attn_window_bwd;
// work: heads·T floats; window as the forward's
int kfa_attn_d128_bwd(bool causal, int window, const void* qkv, const float* bqkv, const int* cu, const void* out,
                      const float* lse, const void* dout, void* dqkv, float* dbqkv, int B, int T, int max_seqlen,
                      int heads, int kv_heads, float qscale, uint32_t th, float ds, uint64_t seed, float* work,
                      hipStream_t st) {
  hipLaunchKernelGGL(attn_d128_rowdot_kernel, dim3((unsigned)(((long)T * heads + 255) / 256)), dim3(256), 0, st,
                     (const bf16_t*)dout, (const bf16_t*)out, cu, work, B, T, heads);
  if (causal && window > 0 && window < max_seqlen)
    launch_bwd_window(qkv, bqkv, cu, lse, work, dout, dqkv, dbqkv, B, T, max_seqlen, heads, kv_heads, window, qscale,
                      th, ds, seed, st);
  else if (causal)
    launch_bwd<true>(qkv, bqkv, cu, lse, work, dout, dqkv, dbqkv, B, T, max_seqlen, heads, kv_heads, qscale, th, ds,
                     seed, st);
  else
    launch_bwd<false>(qkv, bqkv, cu, lse, work, dout, dqkv, dbqkv, B, T, max_seqlen, heads, kv_heads, qscale, th, ds,
                      seed, st);
  return kfa_status();
}
