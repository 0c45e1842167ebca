// Sender side of the sharded embedding exchange (parallel/sparse_exchange.py;
// SURVEY §7.3 H6): dedup of a lookup's ids, expansion of the returned rows and
// the per-distinct-row gradient pre-sum, all on the device.
//
// A lookup of n global row ids on a table interleaved over O owners of R rows:
//
//   plan     key = (id % O) * R + id / O  (owner-major, the host plan's formula),
//            radix-sorted with its position (radix_sort.h), segment heads marked
//            (key differs from its predecessor) and an exclusive prefix sum of
//            the head flags over all n entries gives every sorted entry the index
//            u of its distinct key.  The scan is three launches - heads per tile
//            of 4096, one block scanning the tile counts with a carry, the tile
//            again - so no block waits on another.  Compaction writes
//              rows[u]       local row on the owner (key - owner * R), key order
//              inv[pos]      u for every original position
//              seg_start[u]  first sorted entry of u's run (seg_start[U] = n)
//            and a last launch finds counts[p] (distinct keys owned by rank p) by
//            a binary search of the owner boundaries p * R in the sorted keys.
//            Every store is indexed by an entry position or a scan result: no id
//            value reaches an address.  Ids outside [0, num_rows) raise a flag
//            (their key is 0) that the host reads with the counts.
//   expand   out[i, :] = back[inv[i], :], one 16-byte vector per lane.
//   presum   d_send[u, :] = bf16(sum of float(dout[pos, :]) over u's run), fp32.
//            The ids are power-law: a few runs hold thousands of entries, most
//            one.  The sorted list is cut into chunks of 64 entries, one
//            workgroup each: the chunk's gradient rows are gathered into LDS and
//            every run inside it is summed by a segmented wave scan.  A run that
//            lies inside one chunk is rounded and stored at once; the piece of a
//            run that crosses a chunk edge is stored as an fp32 partial (two
//            slots per chunk: the run entering it and the run leaving it), and a
//            second pass adds each such run's partials in chunk order.  No
//            atomics, a fixed order of additions: bitwise reproducible.  Every
//            row of d_send is written exactly once, so it needs no zeroing.
#include "common.h"

#include "radix_sort.h"

namespace {

constexpr int CH = 64;      // sorted entries per pre-sum chunk (one wave of keys)
constexpr int MAXD = 248;   // CH x (D + 4) fp32 rows in LDS: 64 KB at most
constexpr int SB = 256;     // scan block: 4 waves
constexpr int SW = SB / 64;
constexpr int SR = 16;      // rounds of 64 consecutive entries per wave
constexpr int STILE = SW * SR * 64;   // 4096 entries per scan tile

inline long align256(long x) { return (x + 255) & ~255L; }
inline int scan_tiles(long n) { return (int)((n + STILE - 1) / STILE); }

// key / position of every id; ids outside the table raise *err and take key 0
__global__ __launch_bounds__(256) void xchg_key_kernel(const long* __restrict__ ids, int n, unsigned owners,
                                                       unsigned long long R, long num_rows,
                                                       unsigned* __restrict__ keys, int* __restrict__ pos,
                                                       int* __restrict__ err) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const long id = ids[i];
    unsigned key = 0u;
    if (id < 0 || id >= num_rows) {
      *err = 1;
    } else {   // num_rows <= O * R <= 2^32: the id fits 32 bits
      const unsigned uid = (unsigned)id;
      key = (unsigned)((unsigned long long)(uid % owners) * R + uid / owners);
    }
    keys[i] = key;
    pos[i] = i;
  }
}

__device__ __forceinline__ bool head_at(const unsigned* __restrict__ sk, long i, int n) {
  return i < n && (i == 0 || sk[i] != sk[i - 1]);
}

// tsum[tile] = segment heads among the tile's sorted entries
__global__ __launch_bounds__(SB) void xchg_head_count_kernel(const unsigned* __restrict__ sk, int n,
                                                             int* __restrict__ tsum) {
  __shared__ int wc[SW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long base = (long)blockIdx.x * STILE + w * (SR * 64);
  int c = 0;
#pragma unroll
  for (int r = 0; r < SR; ++r) c += __popcll(__ballot(head_at(sk, base + r * 64 + lane, n)));
  if (lane == 0) wc[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) tsum[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive prefix sum of the tile counts in place (one block, carried across its
// chunks of 256); the total is U: *u_out = U, seg_start[U] = n
__global__ __launch_bounds__(256) void xchg_tile_scan_kernel(int* __restrict__ tsum, int ntiles, int n,
                                                             int* __restrict__ u_out, int* __restrict__ seg_start) {
  __shared__ int red[4];
  int carry = 0;
  for (int b0 = 0; b0 < ntiles; b0 += 256) {
    const int t = b0 + threadIdx.x;
    const int x = t < ntiles ? tsum[t] : 0;
    int s;
    const int e = kfa_radix::block_excl_sum256(x, red, s);
    if (t < ntiles) tsum[t] = carry + e;
    carry += s;
  }
  if (threadIdx.x == 0) {
    *u_out = carry;
    seg_start[carry] = n;   // carry <= n: seg_start holds n + 1 entries
  }
}

// the tile again: u of every sorted entry = heads before it (tile offset + waves
// before + rounds before + lanes before), then the compaction
__global__ __launch_bounds__(SB) void xchg_compact_kernel(const unsigned* __restrict__ sk,
                                                          const int* __restrict__ pos, int n,
                                                          const int* __restrict__ toff, unsigned long long R,
                                                          long* __restrict__ rows, int* __restrict__ inv,
                                                          int* __restrict__ seg_start) {
  __shared__ int wc[SW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long base = (long)blockIdx.x * STILE + w * (SR * 64);
  unsigned long long masks[SR];
  int c = 0;
#pragma unroll
  for (int r = 0; r < SR; ++r) {
    masks[r] = __ballot(head_at(sk, base + r * 64 + lane, n));
    c += __popcll(masks[r]);
  }
  if (lane == 0) wc[w] = c;
  __syncthreads();
  int off = toff[blockIdx.x];
  for (int q = 0; q < w; ++q) off += wc[q];
  const unsigned long long upto = (2ull << lane) - 1ull;   // lanes 0 .. lane
#pragma unroll
  for (int r = 0; r < SR; ++r) {
    const long i = base + r * 64 + lane;
    if (i < n) {
      const int u = off + __popcll(masks[r] & upto) - 1;   // entry 0 is a head: u >= 0
      inv[pos[i]] = u;
      if ((masks[r] >> lane) & 1ull) {
        const unsigned k = sk[i];
        const unsigned owner = (R >> 32) ? 0u : k / (unsigned)R;
        rows[u] = (long)(k - (unsigned long long)owner * R);
        seg_start[u] = (int)i;
      }
    }
    off += __popcll(masks[r]);
  }
}

// index of the first distinct key >= bound: the first sorted entry with such a key
// is a head, and seg_start lists the heads in order
__device__ int distinct_below(const unsigned* __restrict__ sk, int n, const int* __restrict__ seg_start, int U,
                              unsigned long long bound) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((unsigned long long)sk[mid] < bound) lo = mid + 1; else hi = mid;
  }
  if (lo >= n) return U;
  const int f = lo;
  lo = 0; hi = U;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (seg_start[mid] < f) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// counts[p] = distinct keys in [p R, (p + 1) R)
__global__ __launch_bounds__(64) void xchg_counts_kernel(const unsigned* __restrict__ sk, int n,
                                                         const int* __restrict__ seg_start,
                                                         const int* __restrict__ u_in, int world,
                                                         unsigned long long R, int* __restrict__ counts) {
  const int U = *u_in;
  for (int p = threadIdx.x; p < world; p += 64)
    counts[p] = distinct_below(sk, n, seg_start, U, (unsigned long long)(p + 1) * R) -
                distinct_below(sk, n, seg_start, U, (unsigned long long)p * R);
}

// out[i, :] = back[inv[i], :]; one 16-byte vector per thread
__global__ __launch_bounds__(256) void xchg_expand_kernel(const uint4* __restrict__ back, long nback,
                                                          const int* __restrict__ inv, long total, int V,
                                                          uint4* __restrict__ out) {
  for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
    const long i = it / V;
    const int v = (int)(it - i * V);
    const long u = inv[i];
    out[it] = (u >= 0 && u < nback) ? back[u * V + v] : make_uint4(0u, 0u, 0u, 0u);
  }
}

// One chunk of CH sorted entries per workgroup (the reduction of seg_apply_kernel in
// segsparse.hip: rows gathered into LDS, a segmented inclusive scan across the lanes
// of a wave per 8-column slice, each run's sum left over its first row).  Runs inside
// the chunk go out as bf16; the chunk's pieces of runs that cross its edges go to
// part[c][0] (its first run) / part[c][1] (a later run that leaves the chunk).
__global__ __launch_bounds__(256) void xchg_presum_kernel(const unsigned* __restrict__ sk, const int* __restrict__ pos,
                                                          const int* __restrict__ inv, const bf16_t* __restrict__ g,
                                                          float* __restrict__ part, bf16_t* __restrict__ dsend,
                                                          int n, int D, long U) {
  extern __shared__ float rows[];   // [CH][D + 4] fp32 (row padding spreads the lanes' LDS banks)
  __shared__ int sstart[CH + 1];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int c = blockIdx.x;
  const int c0 = c * CH;
  const int cnt = min(CH, n - c0);
  const int V = D >> 3, RS = D + 4;
  for (int it = t; it < cnt * V; it += 256) {
    const int e = it / V, vv = it - e * V;
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(g + (long)pos[c0 + e] * D + vv * 8), f);
    float4* dst = reinterpret_cast<float4*>(rows + e * RS + vv * 8);
    dst[0] = make_float4(f[0], f[1], f[2], f[3]);
    dst[1] = make_float4(f[4], f[5], f[6], f[7]);
  }
  const bool in = lane < cnt;
  const unsigned k = in ? sk[c0 + lane] : 0u;
  const unsigned kp = __shfl_up(k, 1);
  const bool head = in && (lane == 0 || k != kp);
  const unsigned long long mask = __ballot(head);
  const unsigned long long upto = (2ull << lane) - 1ull;
  const int sbeg = 63 - __clzll(mask & upto);          // first lane of this lane's run
  const bool tail = in && (lane == cnt - 1 || ((mask >> (lane + 1)) & 1ull));
  const int nseg = __popcll(mask);
  if (wv == 0) {
    if (head) sstart[__popcll(mask & upto) - 1] = lane;
    if (lane == 0) sstart[nseg] = cnt;
  }
  __syncthreads();
  for (int vv = wv; vv < V; vv += 4) {
    float x[8];
    if (in) {
      const float4* src = reinterpret_cast<const float4*>(rows + lane * RS + vv * 8);
      *reinterpret_cast<float4*>(x) = src[0];
      *reinterpret_cast<float4*>(x + 4) = src[1];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) x[i] = 0.f;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = lane - d >= sbeg;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float y = __shfl_up(x[i], d);
        if (take) x[i] += y;
      }
    }
    if (tail && lane != sbeg) {   // run sum over its first row (a wave only touches its own slice)
      float4* dst = reinterpret_cast<float4*>(rows + sbeg * RS + vv * 8);
      dst[0] = *reinterpret_cast<float4*>(x);
      dst[1] = *reinterpret_cast<float4*>(x + 4);
    }
  }
  __syncthreads();
  const bool cont_prev = c0 > 0 && sk[c0 - 1] == sk[c0];
  const bool cont_next = c0 + cnt < n && sk[c0 + cnt] == sk[c0 + cnt - 1];
  for (int it = t; it < nseg * V; it += 256) {
    const int s = it / V, q = it - s * V;
    const int b = sstart[s];
    const float4* src = reinterpret_cast<const float4*>(rows + b * RS + q * 8);
    const float4 lo = src[0], hi = src[1];
    const bool cross = (s == 0 && cont_prev) || (s == nseg - 1 && cont_next);
    if (!cross) {
      const long u = inv[pos[c0 + b]];
      if (u >= 0 && u < U) {
        const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        *reinterpret_cast<uint4*>(dsend + u * D + q * 8) = pack8(f);
      }
    } else {
      float4* dst = reinterpret_cast<float4*>(part + ((long)c * 2 + (s == 0 ? 0 : 1)) * D + q * 8);
      dst[0] = lo;
      dst[1] = hi;
    }
  }
}

// One wave per chunk; the chunk in which a crossing run STARTS adds that run's
// partials in chunk order (its own piece, then slot 0 of every chunk the run enters).
__global__ __launch_bounds__(256) void xchg_presum_cross_kernel(const unsigned* __restrict__ sk,
                                                                const int* __restrict__ pos,
                                                                const int* __restrict__ inv,
                                                                const int* __restrict__ seg_start,
                                                                const float* __restrict__ part,
                                                                bf16_t* __restrict__ dsend, int n, int nch, int D,
                                                                long U) {
  const int lane = threadIdx.x & 63;
  const int V = D >> 3;
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < nch; c += gridDim.x * 4) {
    const long c1 = (long)(c + 1) * CH;
    if (c1 >= n || sk[c1] != sk[c1 - 1]) continue;   // no run leaves this chunk
    const long u = inv[pos[c1 - 1]];
    if (u < 0 || u >= U) continue;
    const int a = seg_start[u], b = seg_start[u + 1];
    if (a < c * CH) continue;                         // the run started in an earlier chunk
    const int clast = (b - 1) / CH;
    if (lane >= V) continue;
    const float4* p0 = reinterpret_cast<const float4*>(part + ((long)c * 2 + (a == c * CH ? 0 : 1)) * D + lane * 8);
    float4 lo = p0[0], hi = p0[1];
    for (int cc = c + 1; cc <= clast; ++cc) {
      const float4* p = reinterpret_cast<const float4*>(part + (long)cc * 2 * D + lane * 8);
      const float4 l = p[0], h = p[1];
      lo.x += l.x; lo.y += l.y; lo.z += l.z; lo.w += l.w;
      hi.x += h.x; hi.y += h.y; hi.z += h.z; hi.w += h.w;
    }
    const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    *reinterpret_cast<uint4*>(dsend + u * D + lane * 8) = pack8(f);
  }
}

struct XWs {
  unsigned *keys_in, *keys;
  int *pos_in, *pos, *tsum, *hist;
};

XWs xlayout(void* ws, long n) {
  char* p = (char*)ws;
  XWs L;
  L.keys_in = (unsigned*)p; p += align256(n * 4);
  L.pos_in = (int*)p;       p += align256(n * 4);
  L.keys = (unsigned*)p;    p += align256(n * 4);
  L.pos = (int*)p;          p += align256(n * 4);
  L.tsum = (int*)p;         p += align256((long)scan_tiles(n) * 4);
  L.hist = (int*)p;
  return L;
}

}  // namespace

// workspace of one plan (sorted keys and positions stay in it for kfa_xchg_presum)
KFA_API long kfa_xchg_ws_bytes(long n) {
  if (n <= 0 || n > 0x7fffffffL) return 0;
  return 4 * align256(n * 4) + align256((long)scan_tiles(n) * 4) + kfa_radix::hist_bytes(n);
}

// fp32 scratch of kfa_xchg_presum: two partial rows per chunk of 64 entries
KFA_API long kfa_xchg_part_floats(long n, int D) {
  if (n <= 0 || D <= 0) return 0;
  return ((n + CH - 1) / CH) * 2 * (long)D;
}

// ids: int64 [n].  rows: int64 [n], inv: int32 [n], seg_start: int32 [n + 1] (the
// first U / U + 1 entries are written), meta: int32 [2 world + 2] =
// [counts (world) | left to the caller (world) | U | error flag].  Launches only.
KFA_API int kfa_xchg_plan(const long* ids, long n, int world, int owners, long rows_per_owner, long num_rows,
                          void* ws, long ws_bytes, long* rows, int* inv, int* seg_start, int* meta, hipStream_t s) {
  if (n > 0x7fffffffL || world < 1 || owners < 1 || owners > world || rows_per_owner < 1 || num_rows < 0 ||
      rows_per_owner > (1L << 32) || (long)owners * rows_per_owner > (1L << 32) ||
      num_rows > (long)owners * rows_per_owner)
    return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (!ids || !ws || !rows || !inv || !seg_start || !meta || ws_bytes < kfa_xchg_ws_bytes(n))
    return (int)hipErrorInvalidValue;
  const int ni = (int)n;
  const unsigned long long R = (unsigned long long)rows_per_owner;
  const unsigned long long span = (unsigned long long)owners * R - 1ull;
  int nbits = 1;
  while (nbits < 32 && (span >> nbits)) ++nbits;
  XWs L = xlayout(ws, n);
  int e = (int)hipMemsetAsync(meta, 0, (size_t)(2 * world + 2) * 4, s);
  if (e) return e;
  hipLaunchKernelGGL(xchg_key_kernel, dim3(min(16384, (ni + 255) / 256)), dim3(256), 0, s, ids, ni, (unsigned)owners,
                     R, num_rows, L.keys_in, L.pos_in, meta + 2 * world + 1);
  e = kfa_radix::sort_pairs(L.keys_in, L.pos_in, L.keys, L.pos, ni, nbits, L.hist, s);
  if (e) return e;
  const int nt = scan_tiles(n);
  hipLaunchKernelGGL(xchg_head_count_kernel, dim3(nt), dim3(SB), 0, s, L.keys, ni, L.tsum);
  hipLaunchKernelGGL(xchg_tile_scan_kernel, dim3(1), dim3(256), 0, s, L.tsum, nt, ni, meta + 2 * world, seg_start);
  hipLaunchKernelGGL(xchg_compact_kernel, dim3(nt), dim3(SB), 0, s, L.keys, L.pos, ni, L.tsum, R, rows, inv,
                     seg_start);
  hipLaunchKernelGGL(xchg_counts_kernel, dim3(1), dim3(64), 0, s, L.keys, ni, seg_start, meta + 2 * world, world, R,
                     meta);
  return kfa_status();
}

// out [n, D] = back [nback, D] rows by inv [n] (bf16, 16-B aligned rows: D % 8 == 0)
KFA_API int kfa_xchg_expand(const void* back, long nback, const int* inv, long n, int D, void* out, hipStream_t s) {
  if (n > 0x7fffffffL || nback < 0 || D <= 0 || D % 8 != 0) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (!back || !inv || !out || nback < 1) return (int)hipErrorInvalidValue;
  const int V = D >> 3;
  const long total = n * V;
  hipLaunchKernelGGL(xchg_expand_kernel, dim3((unsigned)min(1L << 20, (total + 255) / 256)), dim3(256), 0, s,
                     (const uint4*)back, nback, inv, total, V, (uint4*)out);
  return kfa_status();
}

// d_send [U, D] bf16 = per-distinct-row fp32 sums of dout [n, D] bf16, on the ws /
// inv / seg_start of kfa_xchg_plan for the same ids; part: kfa_xchg_part_floats(n, D)
KFA_API int kfa_xchg_presum(const void* dout, long n, int D, long U, const void* ws, long ws_bytes, const int* inv,
                            const int* seg_start, float* part, long part_floats, void* d_send, hipStream_t s) {
  if (n > 0x7fffffffL || D <= 0 || D % 8 != 0 || D > MAXD || U < 0 || U > n) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  if (!dout || !ws || !inv || !seg_start || !part || !d_send || U < 1 || ws_bytes < kfa_xchg_ws_bytes(n) ||
      part_floats < kfa_xchg_part_floats(n, D))
    return (int)hipErrorInvalidValue;
  const int ni = (int)n;
  const int nch = (ni + CH - 1) / CH;
  XWs L = xlayout(const_cast<void*>(ws), n);
  const size_t lds = (size_t)CH * (D + 4) * sizeof(float);
  hipLaunchKernelGGL(xchg_presum_kernel, dim3(nch), dim3(256), lds, s, L.keys, L.pos, inv, (const bf16_t*)dout, part,
                     (bf16_t*)d_send, ni, D, U);
  hipLaunchKernelGGL(xchg_presum_cross_kernel, dim3(min(16384, (nch + 3) / 4)), dim3(256), 0, s, L.keys, L.pos, inv,
                     seg_start, part, (bf16_t*)d_send, ni, nch, D, U);
  return kfa_status();
}
