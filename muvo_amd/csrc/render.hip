// Rendered first-hit depth loss of the voxel head along lidar rays (an extension, the reference has no such
// loss).  include/muvo_hip.h (muvo_render_fwd) is the definition; tests/render_reference.py restates it.
//   occupancy pass  logits -> q = P(free), a = P(occupied) per cell, (F, V) pairs of fp32, 4 consecutive voxels per lane
//   march           one thread per (ray, frame): the cell sequence of muvo_raycast through a grid in which nothing is occupied -
//                   the walk raycast.hip takes, vg_start / vg_step of voxel_grid.h - composited front to back:
//                   T in fp32, the depth sum in fp64.  |D - t*| leaves as one fp64 partial per workgroup.
//   finish          one workgroup adds the partials in a fixed order and writes the fp32 scalar (vg_finish_kernel of voxel_grid.h).
//   backward        the occupancy pass again (q and a are recomputed, not kept: 8 bytes a voxel and frame), then the same march
//                   with D from the forward pass, adding sign (T_{k+1} t_k - Q_k) per visited cell into an (F, V) accumulator
//                   of 64-bit integers in fixed point, then one dense pass accumulator -> dlogits.
// Integer atomics are order-free, so loss and gradient have the same bits on every call, in both modes of muvo_set_deterministic.
// Before the atomic a wave combines neighbouring lanes that sit in the same cell: the rays of a wave are neighbours of the table,
// next to the origin all 64 are in one cell and further out equal cells form runs of neighbouring lanes.  chamfer.hip loops over the
// distinct destinations of a wave; inside a march that loop would run up to 64 times per step once the rays have spread, so here
// the runs are summed by a segmented shuffle reduction of fixed cost (6 steps) and the head of each run issues the atomic.  Equal
// cells in different runs simply issue one atomic each - integer sums, the result is the same.
// The march loop has the hard bound X + Y + Z + 3 whatever the input.
#include "voxel_grid.h"

#define RN_THREADS 256
#define RN_VOX (RN_THREADS * 4)          // voxels per workgroup of the dense passes (4 consecutive per lane)
#define RN_FIX_BITS 26                    // see the header: 2^24 rays x 2048 sqrt(3) x 2^26 < 2^62
#define RN_FIX_CLAMP 4096.0               // a contribution is clamped to +-4096 before conversion (unit directions stay below 3548)

typedef long long rn_i64x2 __attribute__((ext_vector_type(2)));

// qa[cell] = (q, a) = (e0 / (e0 + occ), occ / (e0 + occ)), interleaved: a march step takes both with one 8-byte load.
// grid = (voxel blocks, frames)
__global__ void __launch_bounds__(RN_THREADS) render_occ_kernel(const float* __restrict__ logits, int C, long V, int vec, float2* __restrict__ qa) {
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * RN_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  const VgSoftmax st = vg_softmax_stats(logits + (size_t)f * C * V, C, V, h0, v4);
  const f32x4 e0 = st.e0, occ = st.rest, s = e0 + occ;
  float2* __restrict__ o = qa + (size_t)f * V + h0;
  if (v4) {                                          // (f V + h0) 8 bytes is a multiple of 32
    *(f32x4*)o = f32x4{e0.x / s.x, occ.x / s.x, e0.y / s.y, occ.y / s.y};
    *(f32x4*)(o + 2) = f32x4{e0.z / s.z, occ.z / s.z, e0.w / s.w, occ.w / s.w};
    return;
  }
  o[0] = float2{e0.x / s.x, occ.x / s.x};
  if (h0 + 1 < V) o[1] = float2{e0.y / s.y, occ.y / s.y};
  if (h0 + 2 < V) o[2] = float2{e0.z / s.z, occ.z / s.z};
  if (h0 + 3 < V) o[3] = float2{e0.w / s.w, occ.w / s.w};
}

// ---- forward march.  grid = (ray blocks, frames).  ALL: no early stop at T == 0, so that the cells of every ray are counted (the
// terms added behind T == 0 are exact zeros: D has the same bits either way).
template <bool ALL>
__global__ void __launch_bounds__(RN_THREADS)
render_march_kernel(const float2* __restrict__ qa, const float* __restrict__ rays, long R, int X, int Y, int Z,
                    const int32_t* __restrict__ lhit, const float* __restrict__ lt, double* __restrict__ D, float* __restrict__ tstar,
                    float* __restrict__ Tn, int32_t* __restrict__ ncell, float* __restrict__ texit, double* __restrict__ part) {
  __shared__ double red[4];
  const long r = (long)blockIdx.x * RN_THREADS + threadIdx.x;
  const int f = blockIdx.y;
  const size_t V = (size_t)X * Y * Z;
  double err = 0.0;
  if (r < R) {
    VgRay s;
    int entry;
    const bool valid = vg_start(s, rays + r * 7, X, Y, Z, entry);
    const size_t o = (size_t)f * R + r;
    float T = 1.f;
    double P = 0.0, Dv = 0.0;
    float ts = 0.f;
    int n = 0;
    if (valid) {
      const float2* __restrict__ qf = qa + (size_t)f * V;
      const int bound = X + Y + Z + 3;
      for (int it = 0; it < bound; ++it) {
        const size_t cell = ((size_t)s.cx * Y + s.cy) * Z + s.cz;
        const float2 c = qf[cell];
        const float w = T * c.y;
        P += (double)w * (double)s.t;
        T = T * c.x;
        ++n;
        if (!ALL && T == 0.f) break;
        if (vg_step(s, X, Y, Z) < 0) break;
      }
      Dv = P + (double)T * (double)s.t1;
      ts = lhit[o] >= 0 ? lt[o] : s.t1;
      err = fabs(Dv - (double)ts);
    }
    D[o] = Dv;
    tstar[o] = ts;
    if (ALL) {
      if (Tn != nullptr) Tn[o] = valid ? T : 0.f;
      if (ncell != nullptr) ncell[o] = valid ? n : -1;
      if (texit != nullptr) texit[o] = valid ? s.t1 : 0.f;
    }
  }
  err = wave_sum_d(err);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = err;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)f * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- backward march.  The loop is wave-uniform (it ends when no lane of the wave marches any more): every lane takes part in the
// shuffles of the combine.  COMBINE = false (MUVO_RENDER_COMBINE=0, for measurements: DESIGN.md section 12) issues one atomic per
// lane and step instead; the sums are integers, the results are the same bits.
template <bool COMBINE>
__global__ void __launch_bounds__(RN_THREADS)
render_bwd_march_kernel(const float2* __restrict__ qa, const float* __restrict__ rays, long R, int X, int Y, int Z,
                        const double* __restrict__ D, const float* __restrict__ tstar, unsigned long long* __restrict__ acc) {
  const long r = (long)blockIdx.x * RN_THREADS + threadIdx.x;
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const long V = (long)X * Y * Z;
  VgRay s = {};
  int entry;
  bool active = false;
  double Dv = 0.0, sg = 0.0;
  if (r < R && vg_start(s, rays + r * 7, X, Y, Z, entry)) {
    const size_t o = (size_t)f * R + r;
    Dv = D[o];
    const double d = Dv - (double)tstar[o];
    sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    active = sg != 0.0;
  }
  const float2* __restrict__ qf = qa + (size_t)f * V;
  unsigned long long* __restrict__ accf = acc + (size_t)f * V;
  float T = 1.f;
  double P = 0.0;
  const int bound = X + Y + Z + 3;
  for (int it = 0; it < bound; ++it) {
    if (__ballot(active) == 0ull) break;
    int cell = -1;
    long long val = 0;
    if (active) {
      cell = (s.cx * Y + s.cy) * Z + s.cz;
      const float2 c = qf[cell];
      const float w = T * c.y;
      const double wt = (double)w * (double)s.t;
      const float Tk = T * c.x;
      double g = sg * ((double)Tk * (double)s.t - ((Dv - P) - wt));
      P += wt;
      T = Tk;
      g = g > RN_FIX_CLAMP ? RN_FIX_CLAMP : (g < -RN_FIX_CLAMP ? -RN_FIX_CLAMP : (g == g ? g : 0.0));
      val = __double2ll_rn(g * (double)(1ll << RN_FIX_BITS));
      if (T == 0.f || vg_step(s, X, Y, Z) < 0) active = false;      // behind T == 0 every contribution is exactly 0
    }
    if (!COMBINE) {
      if (cell >= 0 && (long)cell < V && val != 0) atomicAdd(accf + cell, (unsigned long long)val);
      continue;
    }
    const int prev = __shfl_up(cell, 1, 64);                                    // runs of neighbouring lanes in the same cell
    const bool head = lane == 0 || prev != cell;
    val = vg_run_sum(val, head, lane);
    if (head && cell >= 0 && (long)cell < V && val != 0) atomicAdd(accf + cell, (unsigned long long)val);
  }
}

// dlogits[c] = acc 2^-26 x gout weight / (F N) x (p_c - [c == 0]); every element is written.  grid = (voxel blocks, frames)
__global__ void __launch_bounds__(RN_THREADS)
render_dense_kernel(const float* __restrict__ logits, const long long* __restrict__ acc, int C, long V, int vec, float weight, const float* __restrict__ gout,
                    long N, float* __restrict__ dlogits) {
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * RN_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  const double sc = N > 0 ? (double)gout[0] * (double)weight / ((double)gridDim.y * (double)N) / (double)(1ll << RN_FIX_BITS) : 0.0;
  const long long* __restrict__ ap = acc + (size_t)f * V + h0;
  long long k0 = 0, k1 = 0, k2 = 0, k3 = 0;
  if (v4) {
    const rn_i64x2 u = *(const rn_i64x2*)ap, w = *(const rn_i64x2*)(ap + 2);
    k0 = u.x; k1 = u.y; k2 = w.x; k3 = w.y;
  } else {
    k0 = ap[0];
    if (h0 + 1 < V) k1 = ap[1];
    if (h0 + 2 < V) k2 = ap[2];
    if (h0 + 3 < V) k3 = ap[3];
  }
  const double g0 = (double)k0 * sc, g1 = (double)k1 * sc, g2 = (double)k2 * sc, g3 = (double)k3 * sc;
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  float* __restrict__ df = dlogits + (size_t)f * C * V;
  const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
  const f32x4 occ = st.rest, s = st.e0 + occ;
  // class 0: p_0 - 1 = -a, from the same sum as the forward pass
  vg_st4(df, h0, V, v4, f32x4{(float)(g0 * -(double)(occ.x / s.x)), (float)(g1 * -(double)(occ.y / s.y)), (float)(g2 * -(double)(occ.z / s.z)),
                              (float)(g3 * -(double)(occ.w / s.w))});
  for (int c = 1; c < C; ++c) {
    const f32x4 p = vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), st.m, s);
    vg_st4(df + (size_t)c * V, h0, V, v4, f32x4{(float)(g0 * (double)p.x), (float)(g1 * (double)p.y), (float)(g2 * (double)p.z), (float)(g3 * (double)p.w)});
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

static inline int64_t rn_up16(int64_t n) { return (n + 15) & ~(int64_t)15; }

struct RnWs {
  float2* qa;
  long long* acc;
  double* part;
};
static RnWs rn_ws(void* ws, int64_t F, int64_t V) {
  char* p = (char*)ws;
  const int64_t qa = rn_up16(F * V * 8);
  return RnWs{(float2*)p, (long long*)(p + qa), (double*)(p + qa + F * V * 8)};
}

static int rn_check(const char* who, int64_t F, int C, int X, int Y, int Z, int64_t R, int64_t n_valid, const void* ws, int64_t ws_bytes) {
  if (int rc = vg_check_frames(who, F)) return rc;
  if (int rc = vg_check_classes(who, C)) return rc;
  if (int rc = vg_check_grid(who, X, Y, Z)) return rc;
  if (int rc = vg_check_rays(who, R)) return rc;
  MUVO_CHECK_ARG(n_valid >= 0 && n_valid <= R, "%s: %lld valid rays of %lld", who, (long long)n_valid, (long long)R);
  const int64_t need = muvo_render_ws_bytes(F, (int64_t)X * Y * Z, R);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (16-byte aligned)", who,
                 (long long)ws_bytes, (long long)need);
  return MUVO_OK;
}

static void rn_occupancy(const float* logits, int64_t F, int C, int64_t V, const RnWs& w, hipStream_t st) {
  const int vec = (V % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0;       // the workspace is 16-byte aligned
  hipLaunchKernelGGL(render_occ_kernel, dim3((unsigned)((V + RN_VOX - 1) / RN_VOX), (unsigned)F), dim3(RN_THREADS), 0, st, logits, C, (long)V, vec, w.qa);
}

extern "C" {

int64_t muvo_render_ws_bytes(int64_t F, int64_t V, int64_t R) {
  if (!(vg_frames_ok(F) && vg_voxels_ok(V) && vg_rays_ok(R))) return -1;
  return rn_up16(F * V * 8) + F * V * 8 + F * ((R + RN_THREADS - 1) / RN_THREADS) * 8;
}

int muvo_render_fwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const int32_t* label_hit,
                    const float* label_t, float weight, void* ws, int64_t ws_bytes, double* depth, float* target, float* t_last, int32_t* cells,
                    float* t_exit, float* loss, void* stream) {
  if (int rc = rn_check("render_fwd", F, C, X, Y, Z, R, n_valid, ws, ws_bytes)) return rc;
  MUVO_CHECK_ARG(logits && rays && label_hit && label_t && depth && target && loss, "render_fwd: null pointer");
  MUVO_CHECK_ARG(((uintptr_t)depth & 7) == 0, "render_fwd: depth is not 8-byte aligned");
  const int64_t V = (int64_t)X * Y * Z;
  const RnWs w = rn_ws(ws, F, V);
  rn_occupancy(logits, F, C, V, w, ST);
  const unsigned nb = (unsigned)((R + RN_THREADS - 1) / RN_THREADS);
  if (t_last || cells || t_exit)
    hipLaunchKernelGGL(render_march_kernel<true>, dim3(nb, (unsigned)F), dim3(RN_THREADS), 0, ST, (const float2*)w.qa, rays, (long)R, X, Y, Z,
                       label_hit, label_t, depth, target, t_last, cells, t_exit, w.part);
  else
    hipLaunchKernelGGL(render_march_kernel<false>, dim3(nb, (unsigned)F), dim3(RN_THREADS), 0, ST, (const float2*)w.qa, rays, (long)R, X, Y, Z,
                       label_hit, label_t, depth, target, (float*)nullptr, (int32_t*)nullptr, (float*)nullptr, w.part);
  hipLaunchKernelGGL(vg_finish_kernel, dim3(1), dim3(256), 0, ST, (const double*)w.part, (long)nb * (long)F, weight, (long)F, (long)n_valid, loss);
  MUVO_CHECK_LAUNCH("render_fwd");
  return MUVO_OK;
}

int muvo_render_bwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const double* depth,
                    const float* target, float weight, const float* gout, void* ws, int64_t ws_bytes, float* dlogits, void* stream) {
  if (int rc = rn_check("render_bwd", F, C, X, Y, Z, R, n_valid, ws, ws_bytes)) return rc;
  MUVO_CHECK_ARG(logits && rays && depth && target && gout && dlogits, "render_bwd: null pointer");
  MUVO_CHECK_ARG(((uintptr_t)depth & 7) == 0, "render_bwd: depth is not 8-byte aligned");
  const int64_t V = (int64_t)X * Y * Z;
  const RnWs w = rn_ws(ws, F, V);
  if (hipMemsetAsync(w.acc, 0, (size_t)F * V * 8, ST) != hipSuccess) {
    muvo_set_error("render_bwd: clearing the accumulator failed");
    return MUVO_ERR_HIP;
  }
  const dim3 dense((unsigned)((V + RN_VOX - 1) / RN_VOX), (unsigned)F);
  if (n_valid > 0) {                       // without a valid ray nothing is marched: the dense pass writes zeros
    rn_occupancy(logits, F, C, V, w, ST);
    static const bool combine = env_int("MUVO_RENDER_COMBINE", 1) != 0;
    const dim3 grd((unsigned)((R + RN_THREADS - 1) / RN_THREADS), (unsigned)F);
    if (combine)
      hipLaunchKernelGGL(render_bwd_march_kernel<true>, grd, dim3(RN_THREADS), 0, ST, (const float2*)w.qa, rays, (long)R, X, Y, Z, depth, target,
                         (unsigned long long*)w.acc);
    else
      hipLaunchKernelGGL(render_bwd_march_kernel<false>, grd, dim3(RN_THREADS), 0, ST, (const float2*)w.qa, rays, (long)R, X, Y, Z, depth, target,
                         (unsigned long long*)w.acc);
  }
  const int vec = (V % 4 == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(render_dense_kernel, dense, dim3(RN_THREADS), 0, ST, logits, (const long long*)w.acc, C, (long)V, vec, weight, gout, (long)n_valid, dlogits);
  MUVO_CHECK_LAUNCH("render_bwd");
  return MUVO_OK;
}

}  // extern "C"
