// Fused optimizer apply over FLAT parameter buckets (SURVEY §2.6 K4 Adam, K5 SGD).
//
// One launch updates a whole bucket (every parameter of a dtype group lives in
// one contiguous buffer, see parallel/flat.py), instead of one launch per
// tensor.  Mixed precision: the fp32 master copy is updated and the bf16
// compute copy (if any) is rewritten in the same pass; grads may be bf16
// (the all-reduced bucket) or fp32.  8 elements per lane, 16-B loads for
// bf16, 2x16-B for fp32.  LAMB, LARS and the global-norm clip coefficient (further down) add
// per-tensor and whole-gradient norms as fixed-order segmented reductions over the same
// buffers; every scalar they produce stays in device memory.
#include "common.h"

namespace {

template <bool GBF16>
__device__ __forceinline__ void load_grad8(const void* g, long i, float out[8], float scale) {
  if (GBF16) {
    unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(g) + i), out);
  } else {
    const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g) + i);
    const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g) + i + 4);
    out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w; out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
  }
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] *= scale;
}

__device__ __forceinline__ void load8(const float* p, float o[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void store8(float* p, const float o[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

template <bool GBF16>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ w, bf16_t* __restrict__ wb,
                                                  const void* __restrict__ g, float* __restrict__ mom, long n8,
                                                  float lr, float momentum, float dampening, float wd, int nesterov,
                                                  float gscale, int first) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n8; v += (long)gridDim.x * blockDim.x) {
    const long i = v * 8;
    float gr[8], p[8];
    load_grad8<GBF16>(g, i, gr, gscale);
    load8(w + i, p);
#pragma unroll
    for (int j = 0; j < 8; j++) gr[j] = fmaf(wd, p[j], gr[j]);
    if (mom) {
      float m[8];
      if (first) {
#pragma unroll
        for (int j = 0; j < 8; j++) m[j] = gr[j];
      } else {
        load8(mom + i, m);
#pragma unroll
        for (int j = 0; j < 8; j++) m[j] = fmaf(momentum, m[j], (1.f - dampening) * gr[j]);
      }
      store8(mom + i, m);
#pragma unroll
      for (int j = 0; j < 8; j++) gr[j] = nesterov ? fmaf(momentum, m[j], gr[j]) : m[j];
    }
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = fmaf(-lr, gr[j], p[j]);
    store8(w + i, p);
    if (wb) *reinterpret_cast<uint4*>(wb + i) = pack8(p);
  }
}

// AdamW (decoupled weight decay; wd = 0 gives Adam).  bc1 = 1 - b1^t, bc2 = 1 - b2^t.
// One 8-element vector at element i: the body of adam_kernel and adam_clip_kernel.
template <bool GBF16>
__device__ __forceinline__ void adam_vec8(float* __restrict__ w, bf16_t* __restrict__ wb,
                                          const void* __restrict__ g, float* __restrict__ m_,
                                          float* __restrict__ v_, long i, float lr, float b1, float b2, float eps,
                                          float wd, float step, float rbc2, float gscale) {
  float gr[8], p[8], m[8], s[8];
  load_grad8<GBF16>(g, i, gr, gscale);
  load8(w + i, p);
  load8(m_ + i, m);
  load8(v_ + i, s);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    m[j] = fmaf(b1, m[j], (1.f - b1) * gr[j]);
    s[j] = fmaf(b2, s[j], (1.f - b2) * gr[j] * gr[j]);
    const float denom = sqrtf(s[j]) * rbc2 + eps;
    p[j] = p[j] * (1.f - lr * wd) - step * m[j] / denom;
  }
  store8(m_ + i, m);
  store8(v_ + i, s);
  store8(w + i, p);
  if (wb) *reinterpret_cast<uint4*>(wb + i) = pack8(p);
}

template <bool GBF16>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, bf16_t* __restrict__ wb,
                                                   const void* __restrict__ g, float* __restrict__ m_,
                                                   float* __restrict__ v_, long n8, float lr, float b1, float b2,
                                                   float eps, float wd, float bc1, float bc2, float gscale,
                                                   const float* __restrict__ dbc) {
  if (dbc) {  // bias corrections produced on the device (adam_bc_kernel): replayable in a HIP graph
    bc1 = dbc[0];
    bc2 = dbc[1];
  }
  const float step = lr / bc1;
  const float rbc2 = rsqrtf(bc2);
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n8; v += (long)gridDim.x * blockDim.x)
    adam_vec8<GBF16>(w, wb, g, m_, v_, v * 8, lr, b1, b2, eps, wd, step, rbc2, gscale);
}

// The same step with the gradient scale multiplied by a device scalar: the global-norm
// clip coefficient clip_finish_kernel wrote earlier in this step.  It is exactly 1.0f
// when the norm is under the threshold, and the step is then adam_kernel's bit for bit.
template <bool GBF16>
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ w, bf16_t* __restrict__ wb,
                                                        const void* __restrict__ g, float* __restrict__ m_,
                                                        float* __restrict__ v_, long n8, float lr, float b1,
                                                        float b2, float eps, float wd, float gscale,
                                                        const float* __restrict__ dbc,
                                                        const float* __restrict__ dcoef) {
  const float step = lr / dbc[0];
  const float rbc2 = rsqrtf(dbc[1]);
  gscale *= dcoef[0];
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n8; v += (long)gridDim.x * blockDim.x)
    adam_vec8<GBF16>(w, wb, g, m_, v_, v * 8, lr, b1, b2, eps, wd, step, rbc2, gscale);
}

// t += 1; bc = (1 - b1^t, 1 - b2^t): the per-step scalars of Adam kept on the
// device, so a captured step needs no host value that changes per step
// seed >= 0 (an eager step): the host's step count replaces the device one first — the
// re-seed that used to be a separate fill launch; seed < 0 (graph replay): t advances
__global__ void adam_bc_kernel(int* __restrict__ t, float* __restrict__ bc, float b1, float b2, int seed) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int s = (seed >= 0 ? seed : t[0]) + 1;
    t[0] = s;
    bc[0] = 1.f - powf(b1, (float)s);
    bc[1] = 1.f - powf(b2, (float)s);
  }
}

// master fp32 -> bf16 copy (initial sync / after broadcast)
__global__ void f32_to_bf16_kernel(const float* __restrict__ a, bf16_t* __restrict__ b, long n8) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < n8; v += (long)gridDim.x * blockDim.x) {
    float p[8];
    load8(a + v * 8, p);
    *reinterpret_cast<uint4*>(b + v * 8) = pack8(p);
  }
}

// ---------------------------------------------------------------- LAMB + global-norm clipping
// Norms are segmented reductions over the flat buffer in a FIXED order (no float atomics,
// no zero-fill): the host cuts every tensor into chunks of at most CHUNK elements, a chunk
// never crossing a tensor boundary, and keeps the table on the device as rows of three
// longs (tensor id, start, length).  start is a multiple of 8 and the buffer is padded to
// 8 past every tensor, so the last vector of a tensor may be loaded whole; its elements
// at or past `length` are padding: they hold 0, take no part in a sum and are written
// back unchanged.  One block reduces one chunk — lanes over vectors in address order,
// the xor tree of wave_sum, the four waves in order — and stores its partial with a
// plain store, so every step overwrites every partial.

// block-wide sums of a and b in thread 0 (valid there only); fixed order
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*sh)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();  // sh from the previous chunk has been read
  if ((threadIdx.x & 63) == 0) {
    sh[threadIdx.x >> 6][0] = a;
    sh[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
    b = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
  }
}

// per-chunk sum of squares of the (unscaled) gradient: part[c]
template <bool GBF16>
__global__ __launch_bounds__(256) void chunk_sumsq_kernel(const void* __restrict__ g, const long* __restrict__ chunks,
                                                          int nchunks, float* __restrict__ part) {
  __shared__ float sh[4][2];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long start = chunks[3 * c + 1], len = chunks[3 * c + 2];
    float acc = 0.f, unused = 0.f;
    for (long o = (long)threadIdx.x * 8; o < len; o += 256 * 8) {
      float gr[8];
      load_grad8<GBF16>(g, start + o, gr, 1.f);
      const long valid = len - o;
#pragma unroll
      for (int j = 0; j < 8; j++) acc = j < valid ? fmaf(gr[j], gr[j], acc) : acc;
    }
    block_sum2(acc, unused, sh);
    if (threadIdx.x == 0) part[c] = acc;
  }
}

// out[0] = norm = gscale * sqrt(sum of every partial), out[1] = min(1, max_norm / (norm + 1e-6)):
// torch.nn.utils.clip_grad_norm_'s coefficient.  One wave: lane l sums partials l, l + 64, ...
// in order, then the xor tree; lane 0 writes.
__global__ __launch_bounds__(64) void clip_finish_kernel(const float* __restrict__ part, int nparts, float gscale,
                                                         float max_norm, float* __restrict__ out) {
  float acc = 0.f;
  for (int k = threadIdx.x; k < nparts; k += 64) acc += part[k];
  acc = wave_sum(acc);
  if (threadIdx.x == 0) {
    const float norm = gscale * sqrtf(acc);
    out[0] = norm;
    out[1] = fminf(1.f, max_norm / (norm + 1e-6f));
  }
}

// u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * w with rbc1 = 1 / bc1, rbc2 = rsqrt(bc2):
// stage 1 takes its norm and stage 2 recomputes it from the stored m, v, w by this one expression
__device__ __forceinline__ float lamb_u(float m, float v, float w, float rbc1, float rbc2, float eps, float wd) {
  return fmaf(wd, w, (m * rbc1) / fmaf(sqrtf(v), rbc2, eps));
}

// Stage 1: the Adam moments from g * gscale * dcoef, and per chunk the partial sums of
// w^2 and u^2: part[2c], part[2c + 1] (part == nullptr: a space that takes r = 1).
template <bool GBF16>
__global__ __launch_bounds__(256) void lamb_stage1_kernel(const float* __restrict__ w, const void* __restrict__ g,
                                                          float* __restrict__ m_, float* __restrict__ v_,
                                                          const long* __restrict__ chunks, int nchunks,
                                                          float* __restrict__ part, float b1, float b2, float eps,
                                                          float wd, float gscale, const float* __restrict__ dbc,
                                                          const float* __restrict__ dcoef) {
  __shared__ float sh[4][2];
  const float rbc1 = 1.f / dbc[0];
  const float rbc2 = rsqrtf(dbc[1]);
  if (dcoef) gscale *= dcoef[0];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long start = chunks[3 * c + 1], len = chunks[3 * c + 2];
    float sw = 0.f, su = 0.f;
    for (long o = (long)threadIdx.x * 8; o < len; o += 256 * 8) {
      const long i = start + o, valid = len - o;
      float gr[8], p[8], m[8], s[8];
      load_grad8<GBF16>(g, i, gr, gscale);
      load8(w + i, p);
      load8(m_ + i, m);
      load8(v_ + i, s);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (j < valid) {
          m[j] = fmaf(b1, m[j], (1.f - b1) * gr[j]);
          s[j] = fmaf(b2, s[j], (1.f - b2) * gr[j] * gr[j]);
          const float u = lamb_u(m[j], s[j], p[j], rbc1, rbc2, eps, wd);
          sw = fmaf(p[j], p[j], sw);
          su = fmaf(u, u, su);
        }
      }
      store8(m_ + i, m);
      store8(v_ + i, s);
    }
    if (part) {
      block_sum2(sw, su, sh);
      if (threadIdx.x == 0) {
        part[2 * c] = sw;
        part[2 * c + 1] = su;
      }
    }
  }
}

// ratio[t] = |w_t| / |u_t| from the partials of tensor t's chunks [tens[2t], tens[2t] + tens[2t + 1]),
// 1 when either norm is 0.  One wave per tensor: lane l sums chunks l, l + 64, ... in order, then the xor tree.
__global__ __launch_bounds__(64) void lamb_ratio_kernel(const float* __restrict__ part, const long* __restrict__ tens,
                                                        float* __restrict__ ratio) {
  const long first = tens[2 * blockIdx.x], count = tens[2 * blockIdx.x + 1];
  float sw = 0.f, su = 0.f;
  for (long k = threadIdx.x; k < count; k += 64) {
    sw += part[2 * (first + k)];
    su += part[2 * (first + k) + 1];
  }
  sw = wave_sum(sw);
  su = wave_sum(su);
  if (threadIdx.x == 0) ratio[blockIdx.x] = (sw > 0.f && su > 0.f) ? sqrtf(sw) / sqrtf(su) : 1.f;
}

// Stage 2: w -= lr * r_t * u, u recomputed from the stored m, v and the still un-updated w
// (no per-element scratch); the bf16 compute copy rewritten from w.  ratio == nullptr: r = 1.
__global__ __launch_bounds__(256) void lamb_stage2_kernel(float* __restrict__ w, bf16_t* __restrict__ wb,
                                                          const float* __restrict__ m_, const float* __restrict__ v_,
                                                          const long* __restrict__ chunks, int nchunks,
                                                          const float* __restrict__ ratio, float lr, float eps,
                                                          float wd, const float* __restrict__ dbc) {
  const float rbc1 = 1.f / dbc[0];
  const float rbc2 = rsqrtf(dbc[1]);
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long start = chunks[3 * c + 1], len = chunks[3 * c + 2];
    const float step = ratio ? lr * ratio[chunks[3 * c]] : lr;
    for (long o = (long)threadIdx.x * 8; o < len; o += 256 * 8) {
      const long i = start + o, valid = len - o;
      float p[8], m[8], s[8];
      load8(w + i, p);
      load8(m_ + i, m);
      load8(v_ + i, s);
#pragma unroll
      for (int j = 0; j < 8; j++)
        if (j < valid) p[j] = fmaf(-step, lamb_u(m[j], s[j], p[j], rbc1, rbc2, eps, wd), p[j]);
      store8(w + i, p);
      if (wb) *reinterpret_cast<uint4*>(wb + i) = pack8(p);
    }
  }
}

// ---------------------------------------------------------------- LARS
// Momentum SGD whose update of tensor t is scaled by a layer-wise rate (You, Gitman, Ginsburg 2017):
//   lambda_t = trust * |w_t| / (|g~_t| + wd * |w_t| + eps),  g~ = g * gscale * clip (1 when either norm is 0)
//   d = lambda_t * (g~ + wd * w),  mom = momentum * mom + d,  w -= lr * (nesterov ? d + momentum * mom : mom)
// over the chunk table above.  The norms pass reads g and w once for both per-tensor norms and
// leaves the g^2 partials where clip_finish_kernel takes its own, so a clipped step reads the
// gradient once for the global norm and the per-tensor ones.

// per-chunk sums of w^2 and of the (unscaled) gradient's squares: wpart[c], gpart[c]
template <bool GBF16>
__global__ __launch_bounds__(256) void lars_norms_kernel(const float* __restrict__ w, const void* __restrict__ g,
                                                         const long* __restrict__ chunks, int nchunks,
                                                         float* __restrict__ wpart, float* __restrict__ gpart) {
  __shared__ float sh[4][2];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long start = chunks[3 * c + 1], len = chunks[3 * c + 2];
    float sw = 0.f, sg = 0.f;
    for (long o = (long)threadIdx.x * 8; o < len; o += 256 * 8) {
      const long i = start + o, valid = len - o;
      float gr[8], p[8];
      load_grad8<GBF16>(g, i, gr, 1.f);
      load8(w + i, p);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        sw = j < valid ? fmaf(p[j], p[j], sw) : sw;
        sg = j < valid ? fmaf(gr[j], gr[j], sg) : sg;
      }
    }
    block_sum2(sw, sg, sh);
    if (threadIdx.x == 0) {
      wpart[c] = sw;
      gpart[c] = sg;
    }
  }
}

// ratio[t] = lambda_t from the partials of tensor t's chunks [tens[2t], tens[2t] + tens[2t + 1]); |g~_t| is
// |gscale * dcoef[0]| * sqrt(sum g^2) (dcoef == nullptr: no clipping).  One wave per tensor, summing as
// lamb_ratio_kernel does: lane l takes chunks l, l + 64, ... in order, then the xor tree.
__global__ __launch_bounds__(64) void lars_ratio_kernel(const float* __restrict__ wpart,
                                                        const float* __restrict__ gpart,
                                                        const long* __restrict__ tens, float* __restrict__ ratio,
                                                        float gscale, const float* __restrict__ dcoef, float trust,
                                                        float wd, float eps) {
  const long first = tens[2 * blockIdx.x], count = tens[2 * blockIdx.x + 1];
  float sw = 0.f, sg = 0.f;
  for (long k = threadIdx.x; k < count; k += 64) {
    sw += wpart[first + k];
    sg += gpart[first + k];
  }
  sw = wave_sum(sw);
  sg = wave_sum(sg);
  if (threadIdx.x == 0) {
    if (dcoef) gscale *= dcoef[0];
    const float wn = sqrtf(sw), gn = fabsf(gscale) * sqrtf(sg);
    ratio[blockIdx.x] = (wn > 0.f && gn > 0.f) ? trust * wn / (gn + wd * wn + eps) : 1.f;
  }
}

// The update, chunk by chunk, with ratio[tensor id] from the chunk row (ratio == nullptr: lambda = 1 and
// no multiply, which makes the arithmetic sgd_kernel's at dampening 0, operation for operation).  mom
// starts at 0, so the first step needs no flag.  Lanes past a tensor's length are written back as loaded.
template <bool GBF16>
__global__ __launch_bounds__(256) void lars_apply_kernel(float* __restrict__ w, bf16_t* __restrict__ wb,
                                                         const void* __restrict__ g, float* __restrict__ mom,
                                                         const long* __restrict__ chunks, int nchunks,
                                                         const float* __restrict__ ratio, float lr, float momentum,
                                                         float wd, int nesterov, float gscale,
                                                         const float* __restrict__ dcoef) {
  if (dcoef) gscale *= dcoef[0];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const long start = chunks[3 * c + 1], len = chunks[3 * c + 2];
    const float lam = ratio ? ratio[chunks[3 * c]] : 1.f;
    for (long o = (long)threadIdx.x * 8; o < len; o += 256 * 8) {
      const long i = start + o, valid = len - o;
      float gr[8], p[8], m[8];
      load_grad8<GBF16>(g, i, gr, gscale);
      load8(w + i, p);
      load8(mom + i, m);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (j < valid) {
          float d = fmaf(wd, p[j], gr[j]);
          if (ratio) d *= lam;
          m[j] = fmaf(momentum, m[j], d);
          p[j] = fmaf(-lr, nesterov ? fmaf(momentum, m[j], d) : m[j], p[j]);
        }
      }
      store8(mom + i, m);
      store8(w + i, p);
      if (wb) *reinterpret_cast<uint4*>(wb + i) = pack8(p);
    }
  }
}

int chunk_grid(int nchunks) { return nchunks < 2048 ? nchunks : 2048; }

int grid_for(long n8) {
  long b = (n8 + 255) / 256;
  return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

// The guard of an entry over a flat bucket: n a multiple of 8 (buckets are padded) and every operand it
// cannot do without; the entry returns -1 otherwise.
bool whole_vectors(long n, bool operands = true) { return n % 8 == 0 && operands; }

// The guard of an entry over a chunk (or tensor) table of `count` rows: 1 = launch; otherwise the entry's
// return value: 0 for an empty table (nothing to do, whatever the operands), -1 for a negative count or a
// missing operand.
int table_guard(int count, bool operands = true) { return count > 0 && operands ? 1 : (count ? -1 : 0); }

// One launch of a kernel templated on the gradient's dtype: the <true> instantiation for bf16 gradients,
// the <false> one for fp32, the arguments written once.
template <class... P, class... A>
void launch_g(void (*bf16)(P...), void (*f32)(P...), int g_is_bf16, int grid, hipStream_t s, A... args) {
  hipLaunchKernelGGL(g_is_bf16 ? bf16 : f32, dim3(grid), dim3(256), 0, s, args...);
}

}  // namespace

// n must be a multiple of 8 (flat buckets are padded); pointers 16-B aligned.
KFA_API int kfa_sgd_step(float* w, bf16_t* wb, const void* g, int g_is_bf16, float* mom, long n, float lr,
                         float momentum, float dampening, float wd, int nesterov, float gscale, int first,
                         hipStream_t s) {
  if (!whole_vectors(n)) return -1;
  launch_g(sgd_kernel<true>, sgd_kernel<false>, g_is_bf16, grid_for(n / 8), s, w, wb, g, mom, n / 8, lr, momentum,
           dampening, wd, nesterov, gscale, first);
  return kfa_status();
}

// dbc: nullptr (bc1 / bc2 as given) or the device pair written by kfa_adam_bc
KFA_API int kfa_adam_step(float* w, bf16_t* wb, const void* g, int g_is_bf16, float* m, float* v, long n, float lr,
                          float b1, float b2, float eps, float wd, float bc1, float bc2, float gscale, const float* dbc,
                          hipStream_t s) {
  if (!whole_vectors(n)) return -1;
  launch_g(adam_kernel<true>, adam_kernel<false>, g_is_bf16, grid_for(n / 8), s, w, wb, g, m, v, n / 8, lr, b1, b2, eps,
           wd, bc1, bc2, gscale, dbc);
  return kfa_status();
}

// t += 1 and bc = (1 - b1^t, 1 - b2^t) on the device; seed >= 0 (eager steps, resumes): the device
// count is first set to `seed`; seed < 0 (a captured step): it advances from what the device holds
KFA_API int kfa_adam_bc(int* t, float* bc, float b1, float b2, int seed, hipStream_t s) {
  hipLaunchKernelGGL(adam_bc_kernel, dim3(1), dim3(64), 0, s, t, bc, b1, b2, seed);
  return kfa_status();
}

KFA_API int kfa_f32_to_bf16(const float* a, bf16_t* b, long n, hipStream_t s) {
  if (!whole_vectors(n)) return -1;
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n / 8)), dim3(256), 0, s, a, b, n / 8);
  return kfa_status();
}

// kfa_adam_step with gscale * dcoef[0] as the gradient scale; dbc and dcoef are device scalars
KFA_API int kfa_adam_step_clip(float* w, bf16_t* wb, const void* g, int g_is_bf16, float* m, float* v, long n,
                               float lr, float b1, float b2, float eps, float wd, float gscale, const float* dbc,
                               const float* dcoef, hipStream_t s) {
  if (!whole_vectors(n, dbc && dcoef)) return -1;
  launch_g(adam_clip_kernel<true>, adam_clip_kernel<false>, g_is_bf16, grid_for(n / 8), s, w, wb, g, m, v, n / 8, lr,
           b1, b2, eps, wd, gscale, dbc, dcoef);
  return kfa_status();
}

// chunks: nchunks device rows of three longs: tensor id, start, length; start % 8 == 0, the buffers
// readable up to the next multiple of 8 past start + length, length <= 65536.  part[nchunks].
KFA_API int kfa_chunk_sumsq(const void* g, int g_is_bf16, const long* chunks, int nchunks, float* part,
                            hipStream_t s) {
  if (const int go = table_guard(nchunks); go <= 0) return go;
  launch_g(chunk_sumsq_kernel<true>, chunk_sumsq_kernel<false>, g_is_bf16, chunk_grid(nchunks), s, g, chunks, nchunks,
           part);
  return kfa_status();
}

// out[0] = gscale * sqrt of the sum of part[0..nparts), out[1] = the clip coefficient for max_norm
KFA_API int kfa_clip_finish(const float* part, int nparts, float gscale, float max_norm, float* out,
                            hipStream_t s) {
  if (nparts < 0) return -1;
  hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(64), 0, s, part, nparts, gscale, max_norm, out);
  return kfa_status();
}

// LAMB stage 1: m, v updated; part[2 * nchunks] = per-chunk sums of w^2, u^2 or nullptr.
// dbc: the device pair of kfa_adam_bc; dcoef: nullptr or the device clip coefficient.
KFA_API int kfa_lamb_stage1(const float* w, const void* g, int g_is_bf16, float* m, float* v, const long* chunks,
                            int nchunks, float* part, float b1, float b2, float eps, float wd, float gscale,
                            const float* dbc, const float* dcoef, hipStream_t s) {
  if (const int go = table_guard(nchunks, dbc); go <= 0) return go;
  launch_g(lamb_stage1_kernel<true>, lamb_stage1_kernel<false>, g_is_bf16, chunk_grid(nchunks), s, w, g, m, v, chunks,
           nchunks, part, b1, b2, eps, wd, gscale, dbc, dcoef);
  return kfa_status();
}

// tens: ntens device rows of two longs: first chunk, chunk count.  ratio[ntens].
KFA_API int kfa_lamb_ratio(const float* part, const long* tens, int ntens, float* ratio, hipStream_t s) {
  if (const int go = table_guard(ntens); go <= 0) return go;
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3(ntens), dim3(64), 0, s, part, tens, ratio);
  return kfa_status();
}

// LAMB stage 2: w (and wb, if any) updated with ratio[tensor id] (nullptr: 1) from the m, v of stage 1
KFA_API int kfa_lamb_stage2(float* w, bf16_t* wb, const float* m, const float* v, const long* chunks, int nchunks,
                            const float* ratio, float lr, float eps, float wd, const float* dbc, hipStream_t s) {
  if (const int go = table_guard(nchunks, dbc); go <= 0) return go;
  hipLaunchKernelGGL(lamb_stage2_kernel, dim3(chunk_grid(nchunks)), dim3(256), 0, s, w, wb, m, v, chunks, nchunks,
                     ratio, lr, eps, wd, dbc);
  return kfa_status();
}

// LARS norms: wpart[nchunks], gpart[nchunks] = per-chunk sums of w^2 and of g^2 (g unscaled; gpart may
// point into the buffer kfa_clip_finish reduces).  Chunk table as for kfa_chunk_sumsq.
KFA_API int kfa_lars_norms(const float* w, const void* g, int g_is_bf16, const long* chunks, int nchunks,
                           float* wpart, float* gpart, hipStream_t s) {
  if (const int go = table_guard(nchunks, wpart && gpart); go <= 0) return go;
  launch_g(lars_norms_kernel<true>, lars_norms_kernel<false>, g_is_bf16, chunk_grid(nchunks), s, w, g, chunks, nchunks,
           wpart, gpart);
  return kfa_status();
}

// tens: ntens device rows of two longs: first chunk, chunk count.  ratio[ntens] = the layer-wise rates;
// dcoef: nullptr or the device clip coefficient.
KFA_API int kfa_lars_ratio(const float* wpart, const float* gpart, const long* tens, int ntens, float* ratio,
                           float gscale, const float* dcoef, float trust, float wd, float eps, hipStream_t s) {
  if (const int go = table_guard(ntens); go <= 0) return go;
  hipLaunchKernelGGL(lars_ratio_kernel, dim3(ntens), dim3(64), 0, s, wpart, gpart, tens, ratio, gscale, dcoef, trust,
                     wd, eps);
  return kfa_status();
}

// LARS update: mom, w (and wb, if any) updated with ratio[tensor id] (nullptr: 1, plain momentum SGD)
KFA_API int kfa_lars_apply(float* w, bf16_t* wb, const void* g, int g_is_bf16, float* mom, const long* chunks,
                           int nchunks, const float* ratio, float lr, float momentum, float wd, int nesterov,
                           float gscale, const float* dcoef, hipStream_t s) {
  if (const int go = table_guard(nchunks, mom); go <= 0) return go;
  launch_g(lars_apply_kernel<true>, lars_apply_kernel<false>, g_is_bf16, chunk_grid(nchunks), s, w, wb, g, mom, chunks,
           nchunks, ratio, lr, momentum, wd, nesterov, gscale, dcoef);
  return kfa_status();
}
