// Normalisation kernels (HBM-bound): train-mode BatchNorm2d fwd/bwd with fused ReLU / residual,
// LayerNorm fused with residual-add + dropout (post-LN transformer layer), AdaptiveInstanceNorm3d.
// Reference sites: timm ResNet BN (mile.py:24,81), common.py:102-130 (DecoderDS), layers.py:9-66,
// nn.TransformerEncoderLayer norm1/norm2 (mile.py:96-101), common.py:227-246 (AdaIN3d).
// Statistics are block-reduced in fp32 and combined across blocks with fp64 atomics.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// generic per-"group" moments: group g owns `cnt` elements addressed as
//   x[(i / S) * outer_stride + g * S + (i % S)], i in [0, cnt)   (BN: outer = n; IN: outer unused)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) moments_kernel(const float* __restrict__ x, double* __restrict__ sums,
                                                      long S, long outer_stride, long cnt, int vec4) {
  __shared__ double red[2][4];
  const int g = blockIdx.x;
  const long per = (((cnt + gridDim.y - 1) / gridDim.y) + 3) & ~3L;
  const long i0 = blockIdx.y * per;
  long i1 = i0 + per;
  if (i1 > cnt) i1 = cnt;
  float s = 0.f, q = 0.f;
  double ds = 0.0, dq = 0.0;
  int k = 0;
  if (vec4) {
    // S % 4 == 0, chunk bounds multiples of 4, 16-byte aligned base: one float4 per lane and step.  Four steps per pass with
    // all four loads issued before the first is consumed (clamped address, masked value): the incremental one-load-per-
    // iteration loop paid one memory round trip per 16 bytes and lane
    for (long base = i0 + 4L * threadIdx.x; base < i1; base += 4096) {
      float4 v[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long i = base + 1024 * u;
        ok[u] = i < i1;
        const long ic = ok[u] ? i : i0;
        const long o = ic / S, r = ic - o * S;
        v[u] = *reinterpret_cast<const float4*>(x + o * outer_stride + (long)g * S + r);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!ok[u]) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
        q += (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
      }
      if (++k == 4) { ds += s; dq += q; s = 0.f; q = 0.f; k = 0; }
    }
  } else {
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
      const long o = i / S, r = i - o * S;
      const float v = x[o * outer_stride + (long)g * S + r];
      s += v;
      q += v * v;
      if (++k == 64) { ds += s; dq += q; s = 0.f; q = 0.f; k = 0; }
    }
  }
  ds += s; dq += q;
  ds = wave_sum_d(ds);
  dq = wave_sum_d(dq);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[0][w] = ds; red[1][w] = dq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&sums[2 * g], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd(&sums[2 * g + 1], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

// two-term backward reductions per group: s1 = sum(dz), s2 = sum(dz * xhat)
// mask_mode: 0 none, 1 mask = y > 0 (y given), 2 mask = bn(x) > 0 recomputed with the forward kernel's expression x*sc + sh
__global__ void __launch_bounds__(256) bwd_moments_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ dy, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, double* __restrict__ sums,
                                                          long S, long outer_stride, long x_outer_stride, long cnt,
                                                          int mask_mode, int group_mod, int vec4) {
  __shared__ double red[2][4];
  const int g = blockIdx.x;
  const int ch = group_mod > 0 ? g % group_mod : g;
  const long per = (((cnt + gridDim.y - 1) / gridDim.y) + 3) & ~3L;
  const long i0 = blockIdx.y * per;
  long i1 = i0 + per;
  if (i1 > cnt) i1 = cnt;
  const float mu = mean[g], rs = rstd[g];
  const float ga = gamma ? gamma[ch] : 1.f, be = beta ? beta[ch] : 0.f;
  float s = 0.f, q = 0.f;
  double ds = 0.0, dq = 0.0;
  int k = 0;
  if (vec4) {    // as in moments_kernel: float4 per lane, four steps per pass with all loads in flight together
    for (long base = i0 + 4L * threadIdx.x; base < i1; base += 4096) {
      float4 xv[4], dv[4], yv[4];
      long yoff[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long i = base + 1024 * u;
        ok[u] = i < i1;
        const long ic = ok[u] ? i : i0;
        const long o = ic / S, r = ic - o * S;
        const long idx = o * outer_stride + (long)g * S + r;
        xv[u] = *reinterpret_cast<const float4*>(x + o * x_outer_stride + (long)g * S + r);
        dv[u] = *reinterpret_cast<const float4*>(dy + idx);
        yv[u] = make_float4(1.f, 1.f, 1.f, 1.f);
        yoff[u] = idx;
      }
      if (mask_mode == 1) {      // (uniform) one block with all four loads
#pragma unroll
        for (int u = 0; u < 4; ++u) yv[u] = *reinterpret_cast<const float4*>(y + yoff[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w}, dd[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
        const float ys[4] = {yv[u].x, yv[u].y, yv[u].z, yv[u].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xh = (xs[e] - mu) * rs;
          float d = ok[u] ? dd[e] : 0.f;
          if (mask_mode == 1) d = ys[e] > 0.f ? d : 0.f;
          else if (mask_mode == 2) d = (xs[e] * (rs * ga) + (be - mu * (rs * ga))) > 0.f ? d : 0.f;   /* the forward's own expression: same sign bit */
          s += d;
          q += d * xh;
        }
      }
      if (++k == 4) { ds += s; dq += q; s = 0.f; q = 0.f; k = 0; }
    }
  } else {
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
      const long o = i / S, r = i - o * S;
      const long idx = o * outer_stride + (long)g * S + r;
      const long xidx = o * x_outer_stride + (long)g * S + r;
      const float xh = (x[xidx] - mu) * rs;
      float d = dy[idx];
      if (mask_mode == 1) d = y[idx] > 0.f ? d : 0.f;
      else if (mask_mode == 2) d = (x[xidx] * (rs * ga) + (be - mu * (rs * ga))) > 0.f ? d : 0.f;   /* the forward's own expression: same sign bit */
      s += d;
      q += d * xh;
      if (++k == 64) { ds += s; dq += q; s = 0.f; q = 0.f; k = 0; }
    }
  }
  ds += s; dq += q;
  ds = wave_sum_d(ds);
  dq = wave_sum_d(dq);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[0][w] = ds; red[1][w] = dq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&sums[2 * g], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd(&sums[2 * g + 1], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

static int norm_max_chunks(int dflt) {
  if (muvo_det()) return 1;          // deterministic mode: one workgroup per statistics group = one contributor per double
  static const int v = getenv("MUVO_NORM_MAXCHUNKS") ? atoi(getenv("MUVO_NORM_MAXCHUNKS")) : 0;
  return v > 0 ? v : dflt;
}
static long norm_chunk_elems() {
  static const long v = getenv("MUVO_NORM_CHUNK") ? atol(getenv("MUVO_NORM_CHUNK")) : 4096;   // elements per statistics workgroup: 16384 -> 4096 was worth 1.3 ms/step
  return v;
}

// Library-owned accumulators are PER HIP STREAM: independent branches of the model run on side streams (muvo_amd/ops.py:
// branch) and two streams must never add into / clear the same words.  A handful of streams per process: linear search.
#define NORM_MAX_STREAMS 16
struct NormStreamBufs {
  hipStream_t st;
  bool used;
  double* sums; size_t sums_cap;      // statistics accumulator of the instance / layer norm passes
  double* ring; size_t ring_pos;      // BatchNorm statistics slots
};
static NormStreamBufs g_norm_bufs[NORM_MAX_STREAMS];
static NormStreamBufs* norm_bufs(hipStream_t st) {
  for (int i = 0; i < NORM_MAX_STREAMS; ++i)
    if (g_norm_bufs[i].used && g_norm_bufs[i].st == st) return &g_norm_bufs[i];
  for (int i = 0; i < NORM_MAX_STREAMS; ++i)
    if (!g_norm_bufs[i].used) {
      g_norm_bufs[i] = {st, true, nullptr, 0, nullptr, 0};
      return &g_norm_bufs[i];
    }
  return nullptr;
}

// Statistics accumulator of all norm operations on one stream: a device buffer that is all-zero between operations - the
// moments passes add into it with double atomics and the finalize kernels clear what they read - so no operation needs a
// memset in front of its statistics pass (that was ~180 memsets per step).
static double* norm_sums(size_t n_doubles, hipStream_t st) {
  NormStreamBufs* b = norm_bufs(st);
  if (!b) return nullptr;
  if (n_doubles > b->sums_cap) {
    if (b->sums) hipFree(b->sums);                   // synchronises the device: nobody is using the old buffer any more
    b->sums_cap = n_doubles < 65536 ? 65536 : 2 * n_doubles;
    // cleared ON THE STREAM that uses it: PyTorch's side streams are non-blocking, a null-stream hipMemset is not ordered
    // with them (the first statistics pass on a new stream raced with its own buffer's initialisation)
    if (hipMalloc((void**)&b->sums, b->sums_cap * sizeof(double)) != hipSuccess ||
        hipMemsetAsync(b->sums, 0, b->sums_cap * sizeof(double), st) != hipSuccess) {
      b->sums = nullptr;
      b->sums_cap = 0;
    }
  }
  return b->sums;
}

// BatchNorm statistics slots: a ring of zeroed doubles per stream.  Every BatchNorm pass takes a fresh slot for its (sum, sum
// of squares) or (sum dz, sum dz*xhat), its statistics kernel adds into it and its apply kernel reads the totals straight from
// the slot (mean / rstd / running statistics / dgamma / dbeta are written by the first thread of each channel) - no finalize
// launch between the two (152 four-microsecond launches per step).  When the ring wraps it is cleared with one memset on the
// stream, behind every kernel that read the old slots.
static const size_t BN_RING = 1u << 20;
static double* bn_slot(size_t n_doubles, hipStream_t st) {
  if (n_doubles > BN_RING) return nullptr;
  NormStreamBufs* b = norm_bufs(st);
  if (!b) return nullptr;
  if (!b->ring) {
    if (hipMalloc((void**)&b->ring, BN_RING * sizeof(double)) != hipSuccess) { b->ring = nullptr; return nullptr; }
    if (hipMemsetAsync(b->ring, 0, BN_RING * sizeof(double), st) != hipSuccess) return nullptr;
    b->ring_pos = 0;
  }
  if (b->ring_pos + n_doubles > BN_RING) {
    if (hipMemsetAsync(b->ring, 0, BN_RING * sizeof(double), st) != hipSuccess) return nullptr;
    b->ring_pos = 0;
  }
  double* p = b->ring + b->ring_pos;
  b->ring_pos += (n_doubles + 15) & ~(size_t)15;
  return p;
}

// After a failed step (exception between a statistics pass and the kernel that consumes and clears its sums) the accumulators
// may hold stale partial sums: clear every stream's accumulator and ring, each on its own stream (include/muvo_hip.h).
extern "C" int muvo_reset_accumulators(void) {
  for (int i = 0; i < NORM_MAX_STREAMS; ++i) {
    NormStreamBufs* b = &g_norm_bufs[i];
    if (!b->used) continue;
    if (b->sums && hipMemsetAsync(b->sums, 0, b->sums_cap * sizeof(double), b->st) != hipSuccess) return MUVO_ERR_HIP;
    if (b->ring && hipMemsetAsync(b->ring, 0, BN_RING * sizeof(double), b->st) != hipSuccess) return MUVO_ERR_HIP;
    b->ring_pos = 0;
  }
  return MUVO_OK;
}

// ------------------------------------------------------------------------------------------ BN
// per-channel statistics from the slot totals; `first` (one thread per channel) also stores them for the backward pass and
// updates the running statistics (nn.BatchNorm2d train mode: unbiased variance, momentum)
struct BnStat { float mean, rstd; };
__device__ __forceinline__ BnStat bn_stat(const double* __restrict__ sums, int c, double cnt, float eps, bool first,
                                          float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ run_mean,
                                          float* __restrict__ run_var, float momentum) {
  const double m = sums[2 * c] / cnt;
  double var = sums[2 * c + 1] / cnt - m * m;
  if (var < 0) var = 0;
  BnStat r;
  r.mean = (float)m;
  r.rstd = (float)(1.0 / sqrt(var + (double)eps));
  if (first) {
    mean[c] = r.mean;
    rstd[c] = r.rstd;
    if (run_mean) {
      const double unb = cnt > 1 ? var * cnt / (cnt - 1.0) : var;
      run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)m;
      run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
    }
  }
  return r;
}
#define BN_STAT_PARAMS const double* __restrict__ sums, double cnt, float eps, float* __restrict__ run_mean, \
                       float* __restrict__ run_var, float momentum
// y = act((x-mean)*rstd*gamma+beta [+res before act]) [+res after act]
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                       float* __restrict__ y, float* __restrict__ mean,
                                                       float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, int C, long S, long total4,
                                                       int res_mode, int relu, BN_STAT_PARAMS) {
  // S % 4 == 0 path (vectorised); the host falls back to total4 = total, vec = 1 otherwise via template below
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const long e = i * 4;
    const long row = e / S;
    const int c = (int)(row % C);
    const BnStat bs = bn_stat(sums, c, cnt, eps, row < C && e == row * S, mean, rstd, run_mean, run_var, momentum);
    const float sc = bs.rstd * gamma[c], sh = beta[c] - bs.mean * sc;
    float4 v = *(const float4*)(x + e);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (res_mode) r = *(const float4*)(res + e);
    float o[4] = {v.x * sc + sh, v.y * sc + sh, v.z * sc + sh, v.w * sc + sh};
    const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (res_mode == 1) o[k] += rr[k];
      if (relu) o[k] = o[k] > 0.f ? o[k] : 0.f;
      if (res_mode == 2) o[k] += rr[k];
    }
    *(float4*)(y + e) = make_float4(o[0], o[1], o[2], o[3]);
  }
}
__global__ void __launch_bounds__(256) bn_apply_scalar_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                              float* __restrict__ y, float* __restrict__ mean,
                                                              float* __restrict__ rstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int C, long S, long total,
                                                              int res_mode, int relu, BN_STAT_PARAMS) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / S;
    const int c = (int)(row % C);
    const BnStat bs = bn_stat(sums, c, cnt, eps, row < C && e == row * S, mean, rstd, run_mean, run_var, momentum);
    const float sc = bs.rstd * gamma[c], sh = beta[c] - bs.mean * sc;
    float o = x[e] * sc + sh;
    if (res_mode == 1) o += res[e];
    if (relu) o = o > 0.f ? o : 0.f;
    if (res_mode == 2) o += res[e];
    y[e] = o;
  }
}

// dx = gamma*rstd*(dz - s1/cnt - xhat*s2/cnt); dres = dz (res_mode 1 only)
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ dy, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const double* __restrict__ sums,
                                                           float* __restrict__ dx, float* __restrict__ dres, int C, long S,
                                                           long total, double cnt, int mask_mode, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long row = e / S;
    const int c = (int)(row % C);
    const float mu = mean[c], rs = rstd[c], ga = gamma[c];
    const double s1 = sums[2 * c], s2 = sums[2 * c + 1];
    if (row < C && e == row * S) {      // first element of the channel: the parameter gradients (accumulated into .grad)
      dbeta[c] += (float)s1;
      dgamma[c] += (float)s2;
    }
    const float m1 = (float)(s1 / cnt), m2 = (float)(s2 / cnt);
    const float xh = (x[e] - mu) * rs;
    float d = dy[e];
    if (mask_mode == 1) d = y[e] > 0.f ? d : 0.f;
    else if (mask_mode == 2) d = (x[e] * (rs * ga) + (beta[c] - mu * (rs * ga))) > 0.f ? d : 0.f;
    if (dres) dres[e] = d;
    dx[e] = ga * rs * (d - m1 - xh * m2);
  }
}

// float4 variants (S % 4 == 0, 16-byte aligned tensors, N*C <= 65535): grid = (chunks, N*C), one (n, c) row per workgroup row
__global__ void __launch_bounds__(256) bn_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           float* __restrict__ y, float* __restrict__ mean,
                                                           float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int C, long S, int res_mode,
                                                           int relu, BN_STAT_PARAMS) {
  const long g = blockIdx.y;
  const int c = (int)(g % C);
  const BnStat bs = bn_stat(sums, c, cnt, eps, g < C && blockIdx.x == 0 && threadIdx.x == 0, mean, rstd, run_mean, run_var,
                            momentum);
  const float sc = bs.rstd * gamma[c], sh = beta[c] - bs.mean * sc;
  const float4* xp = reinterpret_cast<const float4*>(x + g * S);
  const float4* rp = reinterpret_cast<const float4*>(res + g * S);
  float4* yp = reinterpret_cast<float4*>(y + g * S);
  const long S4 = S >> 2;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < S4; i += (long)gridDim.x * 256) {
    const float4 v = xp[i];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (res_mode) r = rp[i];
    float o[4] = {v.x * sc + sh, v.y * sc + sh, v.z * sc + sh, v.w * sc + sh};
    const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (res_mode == 1) o[k] += rr[k];
      if (relu) o[k] = o[k] > 0.f ? o[k] : 0.f;
      if (res_mode == 2) o[k] += rr[k];
    }
    yp[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

__global__ void __launch_bounds__(256) bn_bwd_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ dy, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, const double* __restrict__ sums,
                                                               float* __restrict__ dx, float* __restrict__ dres, int C, long S,
                                                               double cnt, int mask_mode, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  const long g = blockIdx.y;
  const int c = (int)(g % C);
  const float mu = mean[c], rs = rstd[c], ga = gamma[c], be = beta[c];
  const double s1 = sums[2 * c], s2 = sums[2 * c + 1];
  if (g < C && blockIdx.x == 0 && threadIdx.x == 0) {      // the parameter gradients (accumulated into .grad)
    dbeta[c] += (float)s1;
    dgamma[c] += (float)s2;
  }
  const float m1 = (float)(s1 / cnt), m2 = (float)(s2 / cnt);
  const float4* xp = reinterpret_cast<const float4*>(x + g * S);
  const float4* yp = reinterpret_cast<const float4*>(y + g * S);
  const float4* gp = reinterpret_cast<const float4*>(dy + g * S);
  float4* op = reinterpret_cast<float4*>(dx + g * S);
  float4* rp = reinterpret_cast<float4*>(dres + g * S);
  const long S4 = S >> 2;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < S4; i += (long)gridDim.x * 256) {
    const float4 xv = xp[i], dv = gp[i];
    float4 yv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (mask_mode == 1) yv = yp[i];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, dd[4] = {dv.x, dv.y, dv.z, dv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
    float o[4], dm[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = (xs[e] - mu) * rs;
      float d = dd[e];
      if (mask_mode == 1) d = ys[e] > 0.f ? d : 0.f;
      else if (mask_mode == 2) d = (xs[e] * (rs * ga) + (be - mu * (rs * ga))) > 0.f ? d : 0.f;   /* the forward's own expression: same sign bit */
      dm[e] = d;
      o[e] = ga * rs * (d - m1 - xh * m2);
    }
    if (dres) rp[i] = make_float4(dm[0], dm[1], dm[2], dm[3]);
    op[i] = make_float4(o[0], o[1], o[2], o[3]);
  }
}

extern "C" int muvo_bn_train_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                                 float* y, float* save_mean, float* save_rstd, float* running_mean,
                                 float* running_var, double* ws, int N, int C, int64_t S, float eps, float momentum,
                                 int res_mode, int relu, void* stream) {
  MUVO_CHECK_ARG(x && gamma && beta && y && save_mean && save_rstd && ws, "bn_train_fwd: null pointer");
  MUVO_CHECK_ARG(N > 0 && C > 0 && S > 0, "bn_train_fwd: bad sizes");
  MUVO_CHECK_ARG(res_mode >= 0 && res_mode <= 2 && (res_mode == 0 || residual), "bn_train_fwd: bad residual mode");
  hipStream_t st = (hipStream_t)stream;
  const long cnt = (long)N * S;
  int chunks = cdiv(cnt, norm_chunk_elems());
  if (chunks > norm_max_chunks(256)) chunks = norm_max_chunks(256);
  double* sums = bn_slot(2 * (size_t)C, st);
  MUVO_CHECK_ARG(sums != nullptr, "bn_train_fwd: cannot allocate the statistics ring");
  hipLaunchKernelGGL(moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, sums, (long)S, (long)C * S, cnt,
                     (int)(S % 4 == 0 && ((uintptr_t)x & 15) == 0));
  const long total = cnt * C;
  const bool aligned = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)(residual ? residual : x)) & 15) == 0;
  if (S % 4 == 0 && S >= 1024 && (long)N * C <= 65535 && aligned) {
    int gx = cdiv(S / 4, 256 * 4);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(bn_apply_vec_kernel, dim3(gx, N * C), dim3(256), 0, st, x, residual, y, save_mean, save_rstd, gamma, beta,
                       C, (long)S, res_mode, relu, (const double*)sums, (double)cnt, eps, running_mean, running_var, momentum);
  } else if (S % 4 == 0 && aligned)      // float4 loads and stores here too: a view at an odd element offset takes the scalar kernel
    hipLaunchKernelGGL(bn_apply_kernel, dim3(ew_grid(total / 4)), dim3(256), 0, st, x, residual, y, save_mean,
                       save_rstd, gamma, beta, C, (long)S, total / 4, res_mode, relu, (const double*)sums, (double)cnt, eps,
                       running_mean, running_var, momentum);
  else
    hipLaunchKernelGGL(bn_apply_scalar_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x, residual, y, save_mean,
                       save_rstd, gamma, beta, C, (long)S, total, res_mode, relu, (const double*)sums, (double)cnt, eps,
                       running_mean, running_var, momentum);
  MUVO_CHECK_LAUNCH("bn_train_fwd");
  return MUVO_OK;
}

// mask_mode: 0 none, 1 = (y > 0) [relu after (bn + residual) or plain relu], 2 = (bn(x) > 0) [relu before residual add]
extern "C" int muvo_bn_train_bwd(const float* x, const float* y, const float* dy, const float* gamma,
                                 const float* beta, const float* save_mean, const float* save_rstd, float* dx,
                                 float* dres, float* dgamma, float* dbeta, double* ws, int N, int C, int64_t S,
                                 int mask_mode, void* stream) {
  MUVO_CHECK_ARG(x && dy && gamma && beta && save_mean && save_rstd && dx && dgamma && dbeta && ws,
                 "bn_train_bwd: null pointer");
  MUVO_CHECK_ARG(mask_mode >= 0 && mask_mode <= 2 && (mask_mode != 1 || y), "bn_train_bwd: bad mask mode");
  hipStream_t st = (hipStream_t)stream;
  const long cnt = (long)N * S;
  int chunks = cdiv(cnt, norm_chunk_elems());
  if (chunks > norm_max_chunks(256)) chunks = norm_max_chunks(256);
  double* sums = bn_slot(2 * (size_t)C, st);
  MUVO_CHECK_ARG(sums != nullptr, "bn_train_bwd: cannot allocate the statistics ring");
  hipLaunchKernelGGL(bwd_moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, y, dy, save_mean, save_rstd, gamma, beta,
                     sums, (long)S, (long)C * S, (long)C * S, cnt, mask_mode, 0,
                     (int)(S % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)(mask_mode == 1 ? y : x)) & 15) == 0));
  const long total = cnt * C;
  if (S % 4 == 0 && S >= 1024 && (long)N * C <= 65535 &&
      (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx | (uintptr_t)(mask_mode == 1 ? y : x) | (uintptr_t)(dres ? dres : dx)) & 15) == 0) {
    int gx = cdiv(S / 4, 256 * 4);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(bn_bwd_apply_vec_kernel, dim3(gx, N * C), dim3(256), 0, st, x, y, dy, save_mean, save_rstd, gamma, beta,
                       (const double*)sums, dx, dres, C, (long)S, (double)cnt, mask_mode, dgamma, dbeta);
  } else
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x, y, dy, save_mean, save_rstd, gamma,
                       beta, (const double*)sums, dx, dres, C, (long)S, total, (double)cnt, mask_mode, dgamma, dbeta);
  MUVO_CHECK_LAUNCH("bn_train_bwd");
  return MUVO_OK;
}

// ------------------------------------------------------------------------------------------------
// BatchNorm apply that WRITES THE CONSUMER'S OPERAND FORMAT (round 4): the convolution that follows a BatchNorm on the bf16x3
// kernels reads channels-last bf16 hi / lo planes of its input, which used to be made by a separate pass over the fp32 NCHW
// result (nchw_split_nhwc_*, conv_bf3.hip).  These kernels apply the normalisation (+ residual, + ReLU) on the 64-channel x
// 256-pixel tile of that split pass and store the planes directly - the fp32 tensor is written only when somebody else needs it
// (y == nullptr: not at all).  The backward form does the same for dx = gamma * rstd * (dz - mean(dz) - xhat * mean(dz * xhat)):
// the planes are what the data- and weight-gradient kernels of the PRODUCING convolution read (muvo_conv_prepare_dy disappears).
// Arithmetic per element is the expression of bn_apply_vec_kernel / bn_bwd_apply_vec_kernel: results are bit-identical.
// Layout of `planes` = bf3_workspace_bytes (conv_bf3.hip): hi plane [N][S][Cp] bf16, lo plane, one zero uint4.
typedef __bf16 nbf16x2 __attribute__((ext_vector_type(2)));
typedef float nf32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void nsplit2(float x0, float x1, unsigned& hi, unsigned& lo) {
  const nbf16x2 h = __builtin_convertvector((nf32x2){x0, x1}, nbf16x2);
  hi = __builtin_bit_cast(unsigned, h);
  const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
  const nbf16x2 l = __builtin_convertvector((nf32x2){x0 - h0, x1 - h1}, nbf16x2);
  lo = __builtin_bit_cast(unsigned, l);
}
#define NSPLIT_PS 258
struct BnSplitArgs {
  const float* x; const float* res; const float* yin; const float* dy;      // fwd: x, res;  bwd: x, yin (mask_mode 1), dy
  float* out; float* dres;                                                 // fp32 result (y / dx) or nullptr; bwd: dres or nullptr
  uint4* hi; uint4* lo;
  const float* gamma; const float* beta; float* mean; float* rstd;         // fwd writes mean / rstd, bwd reads them
  float* run_mean; float* run_var; float* dgamma; float* dbeta;
  const double* sums; double cnt; float eps, momentum;
  int C, Cp, res_mode, relu, mask_mode;
  long S;
};
// per-channel constants of the 64 channels of this workgroup: fwd (sc, sh); bwd (mu, rs, ga, be, m1, m2)
template <bool BWD>
__device__ __forceinline__ void bn_split_consts(const BnSplitArgs& a, int c0, float* s_k) {
  const int t = threadIdx.x;
  if (t < 64) {
    const int c = c0 + t;
    float k[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < a.C) {
      const bool first = blockIdx.x == 0 && blockIdx.z == 0;
      if (!BWD) {
        const BnStat bs = bn_stat(a.sums, c, a.cnt, a.eps, first, a.mean, a.rstd, a.run_mean, a.run_var, a.momentum);
        k[0] = bs.rstd * a.gamma[c];
        k[1] = a.beta[c] - bs.mean * k[0];
      } else {
        const double s1 = a.sums[2 * c], s2 = a.sums[2 * c + 1];
        if (first) {
          a.dbeta[c] += (float)s1;
          a.dgamma[c] += (float)s2;
        }
        k[0] = a.mean[c]; k[1] = a.rstd[c]; k[2] = a.gamma[c]; k[3] = a.beta[c];
        k[4] = (float)(s1 / a.cnt); k[5] = (float)(s2 / a.cnt);
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) s_k[i * 64 + t] = k[i];
  }
  __syncthreads();
}
template <bool BWD>
__device__ __forceinline__ float bn_split_value(const BnSplitArgs& a, const float* s_k, int cl, float xv, float rv, float yv, float dv,
                                                float& dm) {
  if (!BWD) {
    const float sc = s_k[cl], sh = s_k[64 + cl];
    float o = xv * sc + sh;
    if (a.res_mode == 1) o += rv;
    if (a.relu) o = o > 0.f ? o : 0.f;
    if (a.res_mode == 2) o += rv;
    return o;
  } else {
    const float mu = s_k[cl], rs = s_k[64 + cl], ga = s_k[128 + cl], be = s_k[192 + cl], m1 = s_k[256 + cl], m2 = s_k[320 + cl];
    const float xh = (xv - mu) * rs;
    float d = dv;
    if (a.mask_mode == 1) d = yv > 0.f ? d : 0.f;
    else if (a.mask_mode == 2) d = (xv * (rs * ga) + (be - mu * (rs * ga))) > 0.f ? d : 0.f;
    dm = d;
    return ga * rs * (d - m1 - xh * m2);
  }
}
// S % 4 == 0, S >= 1024, 16-byte aligned tensors: 64 channels x 256 pixels per workgroup, float4 per lane and channel
template <bool BWD>
__global__ void __launch_bounds__(256) bn_split_v4_kernel(const BnSplitArgs a) {
  extern __shared__ unsigned nsp_lds[];
  __shared__ float s_k[6 * 64];
  unsigned* th = nsp_lds;
  unsigned* tl = nsp_lds + 32 * NSPLIT_PS;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.y * 64, n = blockIdx.z;
  const long S = a.S, s0 = (long)blockIdx.x * 256, s = s0 + 4 * lane;
  const bool sin = s < S;
  const long sc = sin ? s : s0;
  bn_split_consts<BWD>(a, c0, s_k);
  const size_t nbase = (size_t)n * a.C * S;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x4 xv[8], rv[8], yv[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int c = c0 + 16 * w + 8 * h + r;
      const size_t o = nbase + (size_t)(c < a.C ? c : a.C - 1) * S + sc;
      xv[r] = *(const f32x4*)(a.x + o);
      rv[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
      yv[r] = (f32x4){1.f, 1.f, 1.f, 1.f};
      if (!BWD) { if (a.res_mode) rv[r] = *(const f32x4*)(a.res + o); }
      else {
        rv[r] = *(const f32x4*)(a.dy + o);
        if (a.mask_mode == 1) yv[r] = *(const f32x4*)(a.yin + o);
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cl = 16 * w + 8 * h + r, c = c0 + cl;
      const bool ok = sin && c < a.C;
      f32x4 o, dm;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = 0.f;
        o[j] = bn_split_value<BWD>(a, s_k, cl, xv[r][j], BWD ? 0.f : rv[r][j], yv[r][j], BWD ? rv[r][j] : 0.f, d);
        dm[j] = d;
      }
      if (ok) {
        const size_t oo = nbase + (size_t)c * S + s;
        if (a.out) *(f32x4*)(a.out + oo) = o;
        if (BWD && a.dres) *(f32x4*)(a.dres + oo) = dm;
      } else {
        o = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      xv[r] = o;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = w * 8 + 4 * h + r;
      unsigned hi[4], lo[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) nsplit2(xv[2 * r][j], xv[2 * r + 1][j], hi[j], lo[j]);
      uint2* ph = (uint2*)(th + k * NSPLIT_PS + 4 * lane);
      uint2* pq = (uint2*)(tl + k * NSPLIT_PS + 4 * lane);
      ph[0] = make_uint2(hi[0], hi[1]);
      ph[1] = make_uint2(hi[2], hi[3]);
      pq[0] = make_uint2(lo[0], lo[1]);
      pq[1] = make_uint2(lo[2], lo[3]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int item = tid + 256 * r;
    const int pix = item >> 3, ch = item & 7;
    const long so = s0 + pix;
    const int c = c0 + ch * 8;
    if (so < S && c < a.Cp) {
      const unsigned* ph = th + (4 * ch) * NSPLIT_PS + pix;
      const unsigned* pq = tl + (4 * ch) * NSPLIT_PS + pix;
      const size_t o = (((size_t)n * S + so) * a.Cp + c) >> 3;
      a.hi[o] = make_uint4(ph[0], ph[NSPLIT_PS], ph[2 * NSPLIT_PS], ph[3 * NSPLIT_PS]);
      a.lo[o] = make_uint4(pq[0], pq[NSPLIT_PS], pq[2 * NSPLIT_PS], pq[3 * NSPLIT_PS]);
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0)
    a.hi[2 * ((size_t)gridDim.z * S * a.Cp >> 3)] = make_uint4(0u, 0u, 0u, 0u);       // zero page behind the two planes
}
// any S: 64 channels x 64 pixels per workgroup, one pixel per lane
template <bool BWD>
__global__ void __launch_bounds__(256) bn_split_kernel(const BnSplitArgs a) {
  constexpr int RS = 33;
  __shared__ unsigned th[64 * RS], tl[64 * RS];
  __shared__ float s_k[6 * 64];
  const int tid = threadIdx.x, pl = tid & 63, w = tid >> 6;
  const int c0 = blockIdx.y * 64, n = blockIdx.z;
  const long S = a.S, s0 = (long)blockIdx.x * 64, s = s0 + pl;
  bn_split_consts<BWD>(a, c0, s_k);
  const size_t nbase = (size_t)n * a.C * S;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = w + 4 * r;
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int cl = 2 * k + e, c = c0 + cl;
      const bool ok = c < a.C && s < S;
      const size_t o = nbase + (size_t)(c < a.C ? c : a.C - 1) * S + (s < S ? s : s0);
      const float xv = a.x[o];
      float rv = 0.f, yv = 1.f, dv = 0.f;
      if (!BWD) { if (a.res_mode) rv = a.res[o]; }
      else {
        dv = a.dy[o];
        if (a.mask_mode == 1) yv = a.yin[o];
      }
      float dm = 0.f;
      float t = bn_split_value<BWD>(a, s_k, cl, xv, rv, yv, dv, dm);
      if (ok) {
        if (a.out) a.out[o] = t;
        if (BWD && a.dres) a.dres[o] = dm;
      } else {
        t = 0.f;
      }
      v[e] = t;
    }
    unsigned hi, lo;
    nsplit2(v[0], v[1], hi, lo);
    th[pl * RS + k] = hi;
    tl[pl * RS + k] = lo;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int item = tid + 256 * r;
    const int pix = item >> 3, ch = item & 7;
    const long so = s0 + pix;
    const int c = c0 + ch * 8;
    if (so < S && c < a.Cp) {
      const unsigned* ph = th + pix * RS + ch * 4;
      const unsigned* pq = tl + pix * RS + ch * 4;
      const size_t o = (((size_t)n * S + so) * a.Cp + c) >> 3;
      a.hi[o] = make_uint4(ph[0], ph[1], ph[2], ph[3]);
      a.lo[o] = make_uint4(pq[0], pq[1], pq[2], pq[3]);
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0)
    a.hi[2 * ((size_t)gridDim.z * S * a.Cp >> 3)] = make_uint4(0u, 0u, 0u, 0u);
}
template <bool BWD>
static int bn_split_launch(BnSplitArgs& a, int N, void* planes, hipStream_t st) {
  a.Cp = (a.C + 7) & ~7;
  a.hi = (uint4*)planes;
  a.lo = a.hi + (size_t)N * a.S * a.Cp / 8;
  const uintptr_t al = (uintptr_t)a.x | (uintptr_t)(a.res ? a.res : a.x) | (uintptr_t)(a.yin ? a.yin : a.x) |
                       (uintptr_t)(a.dy ? a.dy : a.x) | (uintptr_t)(a.out ? a.out : a.x) | (uintptr_t)(a.dres ? a.dres : a.x);
  if (a.S % 4 == 0 && a.S >= 1024 && (al & 15) == 0) {
    constexpr int lds = 2 * 32 * NSPLIT_PS * 4;
    static bool attr_set[2] = {false, false};
    if (!attr_set[BWD]) {
      hipFuncSetAttribute((const void*)bn_split_v4_kernel<BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      attr_set[BWD] = true;
    }
    hipLaunchKernelGGL(bn_split_v4_kernel<BWD>, dim3(cdiv(a.S, 256), cdiv(a.Cp, 64), N), dim3(256), lds, st, a);
  } else {
    hipLaunchKernelGGL(bn_split_kernel<BWD>, dim3(cdiv(a.S, 64), cdiv(a.Cp, 64), N), dim3(256), 0, st, a);
  }
  MUVO_CHECK_LAUNCH("bn_split_kernel");
  return MUVO_OK;
}

extern "C" int muvo_bn_train_fwd_planes(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                                        float* save_mean, float* save_rstd, float* running_mean, float* running_var, int N, int C,
                                        int64_t S, float eps, float momentum, int res_mode, int relu, void* planes, void* stream) {
  MUVO_CHECK_ARG(x && gamma && beta && save_mean && save_rstd && planes, "bn_train_fwd_planes: null pointer");
  MUVO_CHECK_ARG(N > 0 && C > 0 && S > 0 && N <= 65535, "bn_train_fwd_planes: bad sizes");
  MUVO_CHECK_ARG(res_mode >= 0 && res_mode <= 2 && (res_mode == 0 || residual), "bn_train_fwd_planes: bad residual mode");
  hipStream_t st = (hipStream_t)stream;
  const long cnt = (long)N * S;
  int chunks = cdiv(cnt, norm_chunk_elems());
  if (chunks > norm_max_chunks(256)) chunks = norm_max_chunks(256);
  double* sums = bn_slot(2 * (size_t)C, st);
  MUVO_CHECK_ARG(sums != nullptr, "bn_train_fwd_planes: cannot allocate the statistics ring");
  hipLaunchKernelGGL(moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, sums, (long)S, (long)C * S, cnt,
                     (int)(S % 4 == 0 && ((uintptr_t)x & 15) == 0));
  BnSplitArgs a = {};
  a.x = x; a.res = res_mode ? residual : nullptr; a.out = y;
  a.gamma = gamma; a.beta = beta; a.mean = save_mean; a.rstd = save_rstd; a.run_mean = running_mean; a.run_var = running_var;
  a.sums = sums; a.cnt = (double)cnt; a.eps = eps; a.momentum = momentum;
  a.C = C; a.res_mode = res_mode; a.relu = relu; a.S = (long)S;
  return bn_split_launch<false>(a, N, planes, st);
}

extern "C" int muvo_bn_train_bwd_planes(const float* x, const float* y, const float* dy, const float* gamma, const float* beta,
                                        const float* save_mean, const float* save_rstd, float* dx, float* dres, float* dgamma,
                                        float* dbeta, int N, int C, int64_t S, int mask_mode, void* planes, void* stream) {
  MUVO_CHECK_ARG(x && dy && gamma && beta && save_mean && save_rstd && dgamma && dbeta && planes, "bn_train_bwd_planes: null pointer");
  MUVO_CHECK_ARG(mask_mode >= 0 && mask_mode <= 2 && (mask_mode != 1 || y) && N > 0 && N <= 65535 && C > 0 && S > 0,
                 "bn_train_bwd_planes: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  const long cnt = (long)N * S;
  int chunks = cdiv(cnt, norm_chunk_elems());
  if (chunks > norm_max_chunks(256)) chunks = norm_max_chunks(256);
  double* sums = bn_slot(2 * (size_t)C, st);
  MUVO_CHECK_ARG(sums != nullptr, "bn_train_bwd_planes: cannot allocate the statistics ring");
  hipLaunchKernelGGL(bwd_moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, y, dy, save_mean, save_rstd, gamma, beta,
                     sums, (long)S, (long)C * S, (long)C * S, cnt, mask_mode, 0,
                     (int)(S % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)(mask_mode == 1 ? y : x)) & 15) == 0));
  BnSplitArgs a = {};
  a.x = x; a.yin = mask_mode == 1 ? y : nullptr; a.dy = dy; a.out = dx; a.dres = dres;
  a.gamma = gamma; a.beta = beta; a.mean = (float*)save_mean; a.rstd = (float*)save_rstd; a.dgamma = dgamma; a.dbeta = dbeta;
  a.sums = sums; a.cnt = (double)cnt; a.C = C; a.mask_mode = mask_mode; a.S = (long)S;
  return bn_split_launch<true>(a, N, planes, st);
}

// ------------------------------------------------------------------------------------- AdaIN3d
__global__ void in_finalize_kernel(double* __restrict__ sums, float* __restrict__ mean, float* __restrict__ rstd,
                                   int G, double cnt, float eps) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const double m = sums[2 * g] / cnt;
  double var = sums[2 * g + 1] / cnt - m * m;
  sums[2 * g] = 0.0;
  sums[2 * g + 1] = 0.0;
  if (var < 0) var = 0;
  mean[g] = (float)m;
  rstd[g] = (float)(1.0 / sqrt(var + (double)eps));
}

// y[n][c][s] = style[n][c] * (x - mean)*rstd + style[n][C + c];  x may be batch-broadcast (x_bs = 0)
__global__ void __launch_bounds__(256) adain_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ style,
                                                          float* __restrict__ y, int C, long S, long x_bs, long total) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long g = e / S;  // n*C + c
    const long n = g / C;
    const int c = (int)(g - n * C);
    const long s = e - g * S;
    const float xv = x[n * x_bs + (long)c * S + s];
    y[e] = style[n * 2 * C + c] * ((xv - mean[g]) * rstd[g]) + style[n * 2 * C + C + c];
  }
}

#define VEC_U 4
// grid.x of the float4 apply kernels: one pass of VEC_U float4 per lane (MUVO_NORM_GX_CAP: A/B switch for the old capped grids)
static int vec_gx(long S4) {
  static const long cap = getenv("MUVO_NORM_GX_CAP") ? atol(getenv("MUVO_NORM_GX_CAP")) : (1l << 22);
  long gx = cdiv(S4, 256l * VEC_U);
  if (gx > cap) gx = cap;
  return (int)(gx < 1 ? 1 : gx);
}

// float4 variants of the AdaIN apply kernels (S % 4 == 0, 16-byte aligned tensors): grid = (chunks, N*C); a workgroup stays
// inside one (n, c) instance, so the per-instance scalars are loaded once and there is no index division per element.
__global__ void __launch_bounds__(256) adain_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ style,
                                                              float* __restrict__ y, int C, long S, long x_bs) {
  const long g = blockIdx.y;
  const long n = g / C;
  const int c = (int)(g - n * C);
  const float st = style[n * 2 * C + c], sh = style[n * 2 * C + C + c];
  const float mu = mean[g], rs = rstd[g];
  const float4* xp = reinterpret_cast<const float4*>(x + n * x_bs + (long)c * S);
  float4* yp = reinterpret_cast<float4*>(y + g * S);
  const long S4 = S >> 2;
  // VEC_U float4 per lane and pass, all loads issued before the first store (a load behind a store of the same wave waits for
  // that store's acknowledgement: vmcnt is in issue order), grid sized so that a workgroup normally makes one pass
  for (long i0 = blockIdx.x * (256L * VEC_U) + threadIdx.x; i0 < S4; i0 += (long)gridDim.x * 256 * VEC_U) {
    float4 v[VEC_U];
#pragma unroll
    for (int u = 0; u < VEC_U; ++u) { const long i = i0 + 256 * u; v[u] = xp[i < S4 ? i : S4 - 1]; }
#pragma unroll
    for (int u = 0; u < VEC_U; ++u) {
      const long i = i0 + 256 * u;
      // same operation order as the scalar kernel: style * ((x - mean) * rstd) + bias
      if (i < S4)
        yp[i] = make_float4(st * ((v[u].x - mu) * rs) + sh, st * ((v[u].y - mu) * rs) + sh, st * ((v[u].z - mu) * rs) + sh,
                            st * ((v[u].w - mu) * rs) + sh);
    }
  }
}

__global__ void adain_bwd_finalize_kernel(double* __restrict__ sums, double* __restrict__ fin, float* __restrict__ dstyle,
                                          int N, int C) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N * C) return;
  const int n = g / C, c = g - n * C;
  const double s1 = sums[2 * g], s2 = sums[2 * g + 1];
  dstyle[(long)n * 2 * C + c] = (float)s2;      // d scale = sum(dy * xhat)
  dstyle[(long)n * 2 * C + C + c] = (float)s1;  // d bias  = sum(dy)
  fin[2 * g] = s1;                              // copy for the apply pass, then clear
  fin[2 * g + 1] = s2;
  sums[2 * g] = 0.0;
  sums[2 * g + 1] = 0.0;
}

__global__ void __launch_bounds__(256) adain_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ style,
                                                              const double* __restrict__ sums, float* __restrict__ dx,
                                                              int C, long S, long x_bs, long total, int act, float slope) {
  for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long g = e / S;
    const long n = g / C;
    const int c = (int)(g - n * C);
    const long s = e - g * S;
    const float rs = rstd[g];
    const float xv = x[n * x_bs + (long)c * S + s];
    const float xh = (xv - mean[g]) * rs;
    const float m1 = (float)(sums[2 * g] / (double)S), m2 = (float)(sums[2 * g + 1] / (double)S);
    // act != NONE: x is the output of that activation (conv + LeakyReLU feeding the norm): chain its derivative here
    dx[e] = style[n * 2 * C + c] * rs * (dy[e] - m1 - xh * m2) * act_grad_from_out(xv, act, slope);
  }
}

__global__ void __launch_bounds__(256) adain_bwd_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd,
                                                                  const float* __restrict__ style,
                                                                  const double* __restrict__ sums, float* __restrict__ dx,
                                                                  int C, long S, long x_bs, int act, float slope) {
  const long g = blockIdx.y;
  const long n = g / C;
  const int c = (int)(g - n * C);
  const float rs = rstd[g], mu = mean[g], st = style[n * 2 * C + c];
  const float m1 = (float)(sums[2 * g] / (double)S), m2 = (float)(sums[2 * g + 1] / (double)S);
  const float4* xp = reinterpret_cast<const float4*>(x + n * x_bs + (long)c * S);
  const float4* gp = reinterpret_cast<const float4*>(dy + g * S);
  float4* op = reinterpret_cast<float4*>(dx + g * S);
  const long S4 = S >> 2;
  for (long i0 = blockIdx.x * (256L * VEC_U) + threadIdx.x; i0 < S4; i0 += (long)gridDim.x * 256 * VEC_U) {
    float4 xv[VEC_U], dv[VEC_U];
#pragma unroll
    for (int u = 0; u < VEC_U; ++u) {
      const long i = i0 + 256 * u, ic = i < S4 ? i : S4 - 1;
      xv[u] = xp[ic];
      dv[u] = gp[ic];
    }
#pragma unroll
    for (int u = 0; u < VEC_U; ++u) {
      const long i = i0 + 256 * u;
      const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w}, dd[4] = {dv[u].x, dv[u].y, dv[u].z, dv[u].w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xs[e] - mu) * rs;
        o[e] = st * rs * (dd[e] - m1 - xh * m2) * act_grad_from_out(xs[e], act, slope);
      }
      if (i < S4) op[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
  }
}

extern "C" int muvo_adain_fwd(const float* x, const float* style, float* y, float* save_mean, float* save_rstd,
                              double* ws, int N, int C, int64_t S, int64_t x_batch_stride, float eps, void* stream) {
  MUVO_CHECK_ARG(x && style && y && save_mean && save_rstd && ws, "adain_fwd: null pointer");
  MUVO_CHECK_ARG(N > 0 && C > 0 && S > 0 && (x_batch_stride == 0 || x_batch_stride == (int64_t)C * S),
                 "adain_fwd: bad sizes");
  hipStream_t st = (hipStream_t)stream;
  const int G = N * C;
  int chunks = cdiv(S, norm_chunk_elems());
  if (chunks > norm_max_chunks(128)) chunks = norm_max_chunks(128);
  double* sums = norm_sums(2 * (size_t)G, st);
  MUVO_CHECK_ARG(sums != nullptr, "adain_fwd: cannot allocate the statistics buffer");
  if (x_batch_stride == 0) {
    // broadcast input: stats of instance (n,c) equal those of (0,c); compute C groups then replicate via kernel launch per n
    for (int n = 0; n < N; ++n)
      hipLaunchKernelGGL(moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, sums + 2L * n * C, (long)S, 0L, (long)S,
                         (int)(S % 4 == 0 && ((uintptr_t)x & 15) == 0));
  } else {
    hipLaunchKernelGGL(moments_kernel, dim3(G, chunks), dim3(256), 0, st, x, sums, (long)S, 0L, (long)S,
                       (int)(S % 4 == 0 && ((uintptr_t)x & 15) == 0));
  }
  hipLaunchKernelGGL(in_finalize_kernel, dim3(cdiv(G, 64)), dim3(64), 0, st, sums, save_mean, save_rstd, G, (double)S, eps);
  const long total = (long)G * S;
  if (S % 4 == 0 && S >= 1024 && G <= 65535 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int gx = vec_gx(S / 4);
    hipLaunchKernelGGL(adain_apply_vec_kernel, dim3(gx, G), dim3(256), 0, st, x, save_mean, save_rstd, style, y, C, (long)S,
                       (long)x_batch_stride);
  } else
    hipLaunchKernelGGL(adain_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x, save_mean, save_rstd, style, y, C,
                       (long)S, (long)x_batch_stride, total);
  MUVO_CHECK_LAUNCH("adain_fwd");
  return MUVO_OK;
}

// the same with the (sum, sum of squares) per (n, c) already accumulated by the producing convolution's epilogue
// (muvo_conv_forward_moments): no statistics pass over x.  `moments` is left all-zero for the next use.
extern "C" int muvo_adain_fwd_moments(const float* x, const float* style, float* y, float* save_mean, float* save_rstd,
                                      double* moments, int N, int C, int64_t S, float eps, void* stream) {
  MUVO_CHECK_ARG(x && style && y && save_mean && save_rstd && moments && N > 0 && C > 0 && S > 0, "adain_fwd_moments: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int G = N * C;
  hipLaunchKernelGGL(in_finalize_kernel, dim3(cdiv(G, 64)), dim3(64), 0, st, moments, save_mean, save_rstd, G, (double)S, eps);
  const long total = (long)G * S;
  if (S % 4 == 0 && S >= 1024 && G <= 65535 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const int gx = vec_gx(S / 4);
    hipLaunchKernelGGL(adain_apply_vec_kernel, dim3(gx, G), dim3(256), 0, st, x, save_mean, save_rstd, style, y, C, (long)S,
                       (long)C * S);
  } else
    hipLaunchKernelGGL(adain_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x, save_mean, save_rstd, style, y, C,
                       (long)S, (long)C * S, total);
  MUVO_CHECK_LAUNCH("adain_fwd_moments");
  return MUVO_OK;
}

// statistics -> (mean, rstd) and the affine map of the AdaIN, y = st * ((x - mean) * rstd) + sh = a * x + b, for a consumer
// that applies it while staging (muvo_conv_forward_affine); the moments are cleared for the next use
__global__ void adain_affine_kernel(double* __restrict__ sums, const float* __restrict__ style, float* __restrict__ mean,
                                    float* __restrict__ rstd, float* __restrict__ aff, int N, int C, double cnt, float eps) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= N * C) return;
  const int n = g / C, c = g - n * C;
  const double m = sums[2 * g] / cnt;
  double var = sums[2 * g + 1] / cnt - m * m;
  sums[2 * g] = 0.0;
  sums[2 * g + 1] = 0.0;
  if (var < 0) var = 0;
  const float mu = (float)m, rs = (float)(1.0 / sqrt(var + (double)eps));
  mean[g] = mu;
  rstd[g] = rs;
  const float a = style[(long)n * 2 * C + c] * rs;
  aff[2 * g] = a;
  aff[2 * g + 1] = style[(long)n * 2 * C + C + c] - a * mu;
}
extern "C" int muvo_adain_affine(const float* style, double* moments, float* save_mean, float* save_rstd, float* aff, int N, int C,
                                 int64_t S, float eps, void* stream) {
  MUVO_CHECK_ARG(style && moments && save_mean && save_rstd && aff && N > 0 && C > 0 && S > 0, "adain_affine: bad args");
  hipLaunchKernelGGL(adain_affine_kernel, dim3(cdiv((long)N * C, 64)), dim3(64), 0, (hipStream_t)stream, moments, style, save_mean,
                     save_rstd, aff, N, C, (double)S, eps);
  MUVO_CHECK_LAUNCH("adain_affine");
  return MUVO_OK;
}

// ================================================================================================
// Last stage of VoxelDecoder1 (common.py:541-545): AdaIN of the last 3x3x3 convolution, then the 1x1x1 class head
// (VoxelSemHead :354-367).  The normalised tensor (8 channels x 2.36 M voxels x 20 frames = 1.5 GB) has ONE consumer, the head,
// so it is never written: forward reads the convolution output once and writes the logits; backward recomputes it, and forms
// dy = W^T dlogits on the fly in both of its passes (statistics + head weight gradient; apply) instead of a head data-gradient
// pass that writes dy and two passes that read it back.  Thread = 4 consecutive voxels x all C channels.
//   y_c = st_c ((x_c - mu_c) rs_c) + sh_c        logit_o = b_o + sum_c W[o][c] y_c      (operation order of the unfused kernels)
// ================================================================================================
template <int C, int CO>
__global__ void __launch_bounds__(256) adain_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, const float* __restrict__ style,
                                                             const float* __restrict__ wh, const float* __restrict__ bh,
                                                             float* __restrict__ logits, long S) {
  const long n = blockIdx.y, S4 = S >> 2;
  float st[C], sh[C], mu[C], rs[C], w[CO][C], b[CO];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    st[c] = style[n * 2 * C + c]; sh[c] = style[n * 2 * C + C + c]; mu[c] = mean[n * C + c]; rs[c] = rstd[n * C + c];
#pragma unroll
    for (int o = 0; o < CO; ++o) w[o][c] = wh[o * C + c];
  }
#pragma unroll
  for (int o = 0; o < CO; ++o) b[o] = bh ? bh[o] : 0.f;
  const float4* xp = reinterpret_cast<const float4*>(x + n * C * S);
  float4* lp = reinterpret_cast<float4*>(logits + n * CO * S);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < S4; i += (long)gridDim.x * 256) {
    float4 acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = make_float4(b[o], b[o], b[o], b[o]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 v = xp[(long)c * S4 + i];
      const float4 y = make_float4(st[c] * ((v.x - mu[c]) * rs[c]) + sh[c], st[c] * ((v.y - mu[c]) * rs[c]) + sh[c],
                                   st[c] * ((v.z - mu[c]) * rs[c]) + sh[c], st[c] * ((v.w - mu[c]) * rs[c]) + sh[c]);
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        acc[o].x += w[o][c] * y.x; acc[o].y += w[o][c] * y.y; acc[o].z += w[o][c] * y.z; acc[o].w += w[o][c] * y.w;
      }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) lp[(long)o * S4 + i] = acc[o];
  }
}

// backward pass 1: per (n, c) sums of dy and dy * xhat (dy = W^T dlogits), head weight / bias gradient
template <int C, int CO>
__global__ void __launch_bounds__(256) adain_head_bwd_stats_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, const float* __restrict__ style,
                                                                   const float* __restrict__ wh, const float* __restrict__ dl,
                                                                   double* __restrict__ sums, double* __restrict__ hsum, long S) {
  constexpr int NV = 2 * C + CO * C + CO;
  __shared__ float red[4][NV];
  const long n = blockIdx.y, S4 = S >> 2;
  float st[C], sh[C], mu[C], rs[C], w[CO][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    st[c] = style[n * 2 * C + c]; sh[c] = style[n * 2 * C + C + c]; mu[c] = mean[n * C + c]; rs[c] = rstd[n * C + c];
#pragma unroll
    for (int o = 0; o < CO; ++o) w[o][c] = wh[o * C + c];
  }
  float s1[C], s2[C], gw[CO][C], gb[CO];
#pragma unroll
  for (int c = 0; c < C; ++c) { s1[c] = 0.f; s2[c] = 0.f; }
#pragma unroll
  for (int o = 0; o < CO; ++o) { gb[o] = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) gw[o][c] = 0.f; }
  const float4* xp = reinterpret_cast<const float4*>(x + n * C * S);
  const float4* gp = reinterpret_cast<const float4*>(dl + n * CO * S);
  // <= 4096 voxels per thread block trip count keeps the fp32 partial sums short (same budget as bwd_moments_kernel)
  for (long i = blockIdx.x * 256L + threadIdx.x; i < S4; i += (long)gridDim.x * 256) {
    float4 g[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) { g[o] = gp[(long)o * S4 + i]; gb[o] += (g[o].x + g[o].y) + (g[o].z + g[o].w); }
    float ge[CO][4];
#pragma unroll
    for (int o = 0; o < CO; ++o) { ge[o][0] = g[o].x; ge[o][1] = g[o].y; ge[o][2] = g[o].z; ge[o][3] = g[o].w; }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 v = xp[(long)c * S4 + i];
      const float xs[4] = {v.x, v.y, v.z, v.w};
      float dy[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < CO; ++o)
#pragma unroll
        for (int e = 0; e < 4; ++e) dy[e] += w[o][c] * ge[o][e];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xs[e] - mu[c]) * rs[c];
        s1[c] += dy[e];
        s2[c] += dy[e] * xh;
        const float y = st[c] * xh + sh[c];
#pragma unroll
        for (int o = 0; o < CO; ++o) gw[o][c] += ge[o][e] * y;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float a = wave_sum(s1[c]), b2 = wave_sum(s2[c]);
    if (lane == 0) { red[wave][2 * c] = a; red[wave][2 * c + 1] = b2; }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
      const float t = wave_sum(gw[o][c]);
      if (lane == 0) red[wave][2 * C + o * C + c] = t;
    }
  }
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    const float t = wave_sum(gb[o]);
    if (lane == 0) red[wave][2 * C + CO * C + o] = t;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    const int k = threadIdx.x;
    const float t = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    if (k < 2 * C) atomicAdd(&sums[2 * (n * C) + k], (double)t);         // [n][c][2]: k = 2 c + which
    else atomicAdd(&hsum[n * (CO * C + CO) + (k - 2 * C)], (double)t);  // per frame: <= gridDim.x adds per address
  }
}
// dW_head[o][c] += sum over frames, db_head[o] likewise; clears the partials
__global__ void adain_head_finalize_kernel(double* __restrict__ hsum, float* __restrict__ dwh, float* __restrict__ dbh, int N, int nw,
                                           int nb) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nw + nb) return;
  double t = 0.0;
  for (int n = 0; n < N; ++n) { t += hsum[(long)n * (nw + nb) + k]; hsum[(long)n * (nw + nb) + k] = 0.0; }
  if (k < nw) dwh[k] += (float)t;
  else if (dbh) dbh[k - nw] += (float)t;
}

// backward pass 2: dx = st rs (dy - m1 - xhat m2) act'(x)
template <int C, int CO>
__global__ void __launch_bounds__(256) adain_head_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, const float* __restrict__ style,
                                                                   const float* __restrict__ wh, const float* __restrict__ dl,
                                                                   const double* __restrict__ fin, float* __restrict__ dx, long S,
                                                                   int act, float slope) {
  const long n = blockIdx.y, S4 = S >> 2;
  float st[C], mu[C], rs[C], m1[C], m2[C], w[CO][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    st[c] = style[n * 2 * C + c]; mu[c] = mean[n * C + c]; rs[c] = rstd[n * C + c];
    m1[c] = (float)(fin[2 * (n * C + c)] / (double)S); m2[c] = (float)(fin[2 * (n * C + c) + 1] / (double)S);
#pragma unroll
    for (int o = 0; o < CO; ++o) w[o][c] = wh[o * C + c];
  }
  const float4* xp = reinterpret_cast<const float4*>(x + n * C * S);
  const float4* gp = reinterpret_cast<const float4*>(dl + n * CO * S);
  float4* op = reinterpret_cast<float4*>(dx + n * C * S);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < S4; i += (long)gridDim.x * 256) {
    float4 g[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) g[o] = gp[(long)o * S4 + i];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float4 v = xp[(long)c * S4 + i];
      const float xs[4] = {v.x, v.y, v.z, v.w};
      float dy[4] = {0.f, 0.f, 0.f, 0.f}, o4[4];
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        dy[0] += w[o][c] * g[o].x; dy[1] += w[o][c] * g[o].y; dy[2] += w[o][c] * g[o].z; dy[3] += w[o][c] * g[o].w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = (xs[e] - mu[c]) * rs[c];
        o4[e] = st[c] * rs[c] * (dy[e] - m1[c] - xh * m2[c]) * act_grad_from_out(xs[e], act, slope);
      }
      op[(long)c * S4 + i] = make_float4(o4[0], o4[1], o4[2], o4[3]);
    }
  }
}

template <int C, int CO>
static int adain_head_run(int which, const float* x, const float* style, float* mean, float* rstd, double* moments, const float* wh,
                          const float* bh, float* logits, const float* dl, float* dx, float* dstyle, float* dwh, float* dbh,
                          double* ws, int N, long S, float eps, int act, float slope, hipStream_t st) {
  const int G = N * C;
  const long S4 = S >> 2;
  if (which == 0) {
    hipLaunchKernelGGL(in_finalize_kernel, dim3(cdiv(G, 64)), dim3(64), 0, st, moments, mean, rstd, G, (double)S, eps);
    int gx = cdiv(S4, 256 * 4);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL((adain_head_fwd_kernel<C, CO>), dim3(gx, N), dim3(256), 0, st, x, (const float*)mean, (const float*)rstd, style,
                       wh, bh, logits, S);
  } else {
    double* sums = norm_sums(2 * (size_t)G + (size_t)N * (CO * C + CO), st);
    if (!sums) { muvo_set_error("adain_head_bwd: cannot allocate the statistics buffer"); return MUVO_ERR_HIP; }
    double* hsum = sums + 2 * (size_t)G;
    int gx = cdiv(S4, 1024);                 // 4096 voxels per workgroup
    if (gx > 128) gx = 128;
    if (muvo_det()) gx = 1;                  // one contributor per statistics word
    hipLaunchKernelGGL((adain_head_bwd_stats_kernel<C, CO>), dim3(gx, N), dim3(256), 0, st, x, (const float*)mean, (const float*)rstd,
                       style, wh, dl, sums, hsum, S);
    hipLaunchKernelGGL(adain_bwd_finalize_kernel, dim3(cdiv(G, 64)), dim3(64), 0, st, sums, ws, dstyle, N, C);
    hipLaunchKernelGGL(adain_head_finalize_kernel, dim3(1), dim3(64), 0, st, hsum, dwh, dbh, N, CO * C, CO);
    gx = cdiv(S4, 256 * 4);
    if (gx > 128) gx = 128;
    hipLaunchKernelGGL((adain_head_bwd_apply_kernel<C, CO>), dim3(gx, N), dim3(256), 0, st, x, (const float*)mean, (const float*)rstd,
                       style, wh, dl, (const double*)ws, dx, S, act, slope);
  }
  return MUVO_OK;
}

extern "C" int muvo_adain_head_supported(int C, int CO, int64_t S) {
  return (C == 8 && CO == 2 && S % 4 == 0 && S >= 1024) ? 1 : 0;
}
extern "C" int muvo_adain_head_fwd(const float* x, const float* style, float* save_mean, float* save_rstd, double* moments,
                                   const float* head_w, const float* head_b, float* logits, int N, int C, int CO, int64_t S,
                                   float eps, void* stream) {
  MUVO_CHECK_ARG(x && style && save_mean && save_rstd && moments && head_w && logits && N > 0 && N <= 65535, "adain_head_fwd: bad args");
  MUVO_CHECK_ARG(muvo_adain_head_supported(C, CO, S) && (((uintptr_t)x | (uintptr_t)logits) & 15) == 0, "adain_head_fwd: shape");
  const int rc = adain_head_run<8, 2>(0, x, style, save_mean, save_rstd, moments, head_w, head_b, logits, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, N, (long)S, eps, 0, 0.f, (hipStream_t)stream);
  if (rc) return rc;
  MUVO_CHECK_LAUNCH("adain_head_fwd");
  return MUVO_OK;
}
extern "C" int muvo_adain_head_bwd(const float* x, const float* style, const float* save_mean, const float* save_rstd,
                                   const float* head_w, const float* dlogits, float* dx, float* dstyle, float* dhead_w,
                                   float* dhead_b, double* ws, int N, int C, int CO, int64_t S, int act, float slope, void* stream) {
  MUVO_CHECK_ARG(x && style && save_mean && save_rstd && head_w && dlogits && dx && dstyle && dhead_w && ws && N > 0 && N <= 65535,
                 "adain_head_bwd: bad args");
  MUVO_CHECK_ARG(muvo_adain_head_supported(C, CO, S) && (((uintptr_t)x | (uintptr_t)dlogits | (uintptr_t)dx) & 15) == 0,
                 "adain_head_bwd: shape");
  const int rc = adain_head_run<8, 2>(1, x, style, (float*)save_mean, (float*)save_rstd, nullptr, head_w, nullptr, nullptr, dlogits, dx,
                                      dstyle, dhead_w, dhead_b, ws, N, (long)S, 0.f, act, slope, (hipStream_t)stream);
  if (rc) return rc;
  MUVO_CHECK_LAUNCH("adain_head_bwd");
  return MUVO_OK;
}

// dx: (N,C,S) always dense (caller reduces over batch when the input was broadcast); dstyle: (N, 2C) overwritten
extern "C" int muvo_adain_bwd(const float* x, const float* style, const float* dy, const float* save_mean,
                              const float* save_rstd, float* dx, float* dstyle, double* ws, int N, int C, int64_t S,
                              int64_t x_batch_stride, int act, float slope, void* stream) {
  MUVO_CHECK_ARG(x && style && dy && save_mean && save_rstd && dx && dstyle && ws, "adain_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int G = N * C;
  int chunks = cdiv(S, norm_chunk_elems());
  if (chunks > norm_max_chunks(128)) chunks = norm_max_chunks(128);
  double* sums = norm_sums(2 * (size_t)G, st);
  MUVO_CHECK_ARG(sums != nullptr, "adain_bwd: cannot allocate the statistics buffer");
  // groups are (n,c) instances: x index = n*x_bs + c*S + s.  With outer_stride==0 trick the group index
  // addresses dy densely (g*S) and x through x_outer/g mapping: handle broadcast by per-n launches.
  if (x_batch_stride == 0) {
    for (int n = 0; n < N; ++n)
      hipLaunchKernelGGL(bwd_moments_kernel, dim3(C, chunks), dim3(256), 0, st, x, (const float*)nullptr,
                         dy + (long)n * C * S, save_mean + (long)n * C, save_rstd + (long)n * C, (const float*)nullptr,
                         (const float*)nullptr, sums + 2L * n * C, (long)S, 0L, 0L, (long)S, 0, 0,
                         (int)(S % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy) & 15) == 0));
  } else {
    hipLaunchKernelGGL(bwd_moments_kernel, dim3(G, chunks), dim3(256), 0, st, x, (const float*)nullptr, dy, save_mean,
                       save_rstd, (const float*)nullptr, (const float*)nullptr, sums, (long)S, 0L, 0L, (long)S, 0, 0,
                       (int)(S % 4 == 0 && (((uintptr_t)x | (uintptr_t)dy) & 15) == 0));
  }
  hipLaunchKernelGGL(adain_bwd_finalize_kernel, dim3(cdiv(G, 64)), dim3(64), 0, st, sums, ws, dstyle, N, C);
  const long total = (long)G * S;
  if (S % 4 == 0 && S >= 1024 && G <= 65535 && (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15) == 0) {
    const int gx = vec_gx(S / 4);
    hipLaunchKernelGGL(adain_bwd_apply_vec_kernel, dim3(gx, G), dim3(256), 0, st, x, dy, save_mean, save_rstd, style, ws, dx, C,
                       (long)S, (long)x_batch_stride, act, slope);
  } else
    hipLaunchKernelGGL(adain_bwd_apply_kernel, dim3(ew_grid(total)), dim3(256), 0, st, x, dy, save_mean, save_rstd, style,
                       ws, dx, C, (long)S, (long)x_batch_stride, total, act, slope);
  MUVO_CHECK_LAUNCH("adain_bwd");
  return MUVO_OK;
}

// ---------------------------------------------------------------------------------- LayerNorm
// z = x + dropout(a); y = LN(z).  One wave per row, E <= 64*MAXV.
template <int MAXV>
__global__ void __launch_bounds__(256) add_dropout_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ y,
                                                                 float* __restrict__ z, float* __restrict__ mean,
                                                                 float* __restrict__ rstd, int rows, int E, float eps,
                                                                 float p, uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int e = lane + 64 * k;
    float t = 0.f;
    if (e < E) {
      const long idx = (long)row * E + e;
      t = x[idx] + (a ? a[idx] * dropout_scale(seed, (uint64_t)idx, p) : 0.f);
      z[idx] = t;
    }
    v[k] = t;
    s += t;
  }
  const float mu = wave_sum(s) / E;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int e = lane + 64 * k;
    if (e < E) { const float d = v[k] - mu; q += d * d; }
  }
  const float rs = rsqrtf(wave_sum(q) / E + eps);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int e = lane + 64 * k;
    if (e < E) y[(long)row * E + e] = (v[k] - mu) * rs * gamma[e] + beta[e];
  }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// dz = rstd*(dy*g - mean(dy*g) - xhat*mean(dy*g*xhat)); dx = dz; da = dz*dropmask; dgamma/dbeta via LDS + atomics
template <int MAXV>
__global__ void __launch_bounds__(256) add_dropout_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, float* __restrict__ dx,
                                                                 float* __restrict__ da, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, int rows, int E,
                                                                 int rows_per_block, float p, uint64_t seed) {
  extern __shared__ float sm[];  // [4 waves][2][E]: per-wave partial sums, added in wave order (no LDS atomics: their order varies)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* sg = sm + (size_t)w * 2 * E;
  float* sb = sg + E;
  const int r0 = blockIdx.x * rows_per_block;
  float ag[MAXV], ab[MAXV];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) { ag[k] = 0.f; ab[k] = 0.f; }
  float gm[MAXV];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) gm[k] = gamma[lane + 64 * k < E ? lane + 64 * k : 0];
  // A wave takes its rows four at a time: all loads of the four rows first (unconditional: clamped index, masked value), the
  // eight row sums reduced in ONE interleaved butterfly, the stores last.  Row by row, every row paid the previous row's
  // store acknowledgement (loads behind stores wait for them), its own load round trip and two dependent shuffle chains.
  constexpr int RPW = 4;
  for (int rr0 = w * RPW; rr0 < rows_per_block; rr0 += 4 * RPW) {
    float gv[RPW][MAXV], zv[RPW][MAXV], mu[RPW], rs[RPW];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int row = r0 + rr0 + j, rc = row < rows && rr0 + j < rows_per_block ? row : rows - 1;
      mu[j] = mean[rc];
      rs[j] = rstd[rc];
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int e = lane + 64 * k;
        const long idx = (long)rc * E + (e < E ? e : 0);
        gv[j][k] = dy[idx];
        zv[j][k] = z[idx];
      }
    }
    float s[2 * RPW];
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const bool rok = r0 + rr0 + j < rows && rr0 + j < rows_per_block;
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const bool ok = rok && lane + 64 * k < E;
        const float g = ok ? gv[j][k] : 0.f;
        const float xh = ok ? (zv[j][k] - mu[j]) * rs[j] : 0.f;
        ag[k] += g * xh;
        ab[k] += g;
        const float d = g * gm[k];
        gv[j][k] = d;            // d and xhat replace the loaded values
        zv[j][k] = xh;
        s1 += d;
        s2 += d * xh;
      }
      s[2 * j] = s1;
      s[2 * j + 1] = s2;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int q = 0; q < 2 * RPW; ++q) s[q] += __shfl_xor(s[q], o, 64);
#pragma unroll
    for (int j = 0; j < RPW; ++j) {
      const int row = r0 + rr0 + j;
      if (row < rows && rr0 + j < rows_per_block) {      // (uniform)
        const float s1 = s[2 * j] / E, s2 = s[2 * j + 1] / E;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
          const int e = lane + 64 * k;
          if (e < E) {
            const long idx = (long)row * E + e;
            const float dz = rs[j] * (gv[j][k] - s1 - zv[j][k] * s2);
            dx[idx] = dz;
            if (da) da[idx] = dz * dropout_scale(seed, (uint64_t)idx, p);
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int e = lane + 64 * k;
    if (e < E) { sg[e] = ag[k]; sb[e] = ab[k]; }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < E; e += 256) {
    atomicAdd(&dgamma[e], (sm[e] + sm[2 * E + e]) + (sm[4 * E + e] + sm[6 * E + e]));
    atomicAdd(&dbeta[e], (sm[E + e] + sm[3 * E + e]) + (sm[5 * E + e] + sm[7 * E + e]));
  }
}

extern "C" int muvo_add_dropout_layernorm_fwd(const float* x, const float* a, const float* gamma, const float* beta,
                                              float* y, float* z, float* mean, float* rstd, int rows, int E, float eps,
                                              float p, uint64_t seed, void* stream) {
  MUVO_CHECK_ARG(x && gamma && beta && y && z && mean && rstd, "layernorm_fwd: null pointer");
  MUVO_CHECK_ARG(rows > 0 && E > 0 && E <= 512, "layernorm_fwd: E=%d unsupported (max 512)", E);
  hipLaunchKernelGGL((add_dropout_ln_fwd_kernel<8>), dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, a, gamma,
                     beta, y, z, mean, rstd, rows, E, eps, p, seed);
  MUVO_CHECK_LAUNCH("layernorm_fwd");
  return MUVO_OK;
}

extern "C" int muvo_add_dropout_layernorm_bwd(const float* dy, const float* z, const float* mean, const float* rstd,
                                              const float* gamma, float* dx, float* da, float* dgamma, float* dbeta,
                                              int rows, int E, float p, uint64_t seed, void* stream) {
  MUVO_CHECK_ARG(dy && z && mean && rstd && gamma && dx && dgamma && dbeta, "layernorm_bwd: null pointer");
  MUVO_CHECK_ARG(rows > 0 && E > 0 && E <= 512, "layernorm_bwd: E=%d unsupported (max 512)", E);
  const int rpb = muvo_det() ? rows : 16;       // four rows per wave; 6500 token rows -> 407 workgroups (deterministic mode: one workgroup, one contributor per dgamma / dbeta element)
  hipLaunchKernelGGL((add_dropout_ln_bwd_kernel<8>), dim3(cdiv(rows, rpb)), dim3(256), 8 * E * sizeof(float),
                     (hipStream_t)stream, dy, z, mean, rstd, gamma, dx, da, dgamma, dbeta, rows, E, rpb, p, seed);
  MUVO_CHECK_LAUNCH("layernorm_bwd");
  return MUVO_OK;
}
