// Rendered first-hit class loss of the voxel head along lidar rays (an extension, the reference has no such
// loss).  include/muvo_hip.h (muvo_render_class_fwd) is the definition; tests/render_class_reference.py restates it.
//   probability pass  logits -> p_c per cell, CELL-MAJOR (F, V, C) fp32: a march step needs q = p_0 and p_y of one cell, y differs
//                     from ray to ray - cell-major puts both into one span of 4 C bytes (one 8-byte load at C = 2, two dwords of
//                     one or two 64-byte lines otherwise) and keeps p_c = e_c / s to the bit, with no expf in the march.  The
//                     transposition goes through LDS, so that the pass stores contiguous spans.
//   march             one thread per (ray, frame), the walk of render.hip (vg_start / vg_step of voxel_grid.h): T in fp32,
//                     S_y = sum_k T_k p_{k,y} in fp64.  -log((S_y + eps) / (1 + eps)) leaves as one fp64 partial per workgroup.
//   finish            one workgroup adds the partials in a fixed order and writes the fp32 scalar.
//   backward          the probability pass again, then the same march with S_y from the forward pass, adding -A_j r to slot y and
//                     -B_j r to slot 0 (r = 1 / (S_y + eps)) of an (F, C, V) accumulator of 64-bit integers in fixed point, then one
//                     dense pass accumulator -> dlogits.
// Integer atomics are order-free, so loss and gradient have the same bits on every call, in both modes of muvo_set_deterministic.
// Before the atomics a wave combines neighbouring lanes as render_bwd_march_kernel does (vg_run_sum of voxel_grid.h): the slot-0
// values over runs of equal cell, the slot-y values over runs of equal (cell, y).  Both were measured against one atomic per lane
// (DESIGN.md section 14): 3.1 ms instead of 7.8 (slot 0 only) and 11.5 (none) for a call at C = 2, factor 1.
// The march loop has the hard bound X + Y + Z + 3 whatever the input.
#include "voxel_grid.h"

#define RC_THREADS 256
#define RC_VOX (RC_THREADS * 4)           // voxels per workgroup of the dense passes (4 consecutive per lane)
#define RC_FIX_BITS 37                     // see the header: 2^24 rays x 1 x 2^37 < 2^62
#define RC_EPS 0.0009765625                // 2^-10, a constant of the definition

typedef long long rc_i64x2 __attribute__((ext_vector_type(2)));

// prob[(f V + cell) C + c] = p_c = e_c / (e_0 + rest).  grid = (voxel blocks, frames), RC_PROB_THREADS lanes with 4 consecutive voxels
// each.  The planes are read with the accesses of the other dense passes; the probabilities go through an LDS tile of one row per
// voxel (C | 1 floats: an odd stride) and leave as the block's contiguous span of C floats per voxel in lane order - written
// straight from the registers, a lane's stores would lie 16 C bytes apart (measured at C = 9, factor 1: 3.6 ms instead of 0.4).
#define RC_PROB_THREADS 128
#define RC_PROB_VOX (RC_PROB_THREADS * 4)
__global__ void __launch_bounds__(RC_PROB_THREADS)
render_class_prob_kernel(const float* __restrict__ logits, int C, long V, int vec, int vec_out, float* __restrict__ prob) {
  extern __shared__ float rc_tile[];                   // RC_PROB_VOX rows of Cp floats
  const long f = blockIdx.y;
  const long b0 = (long)blockIdx.x * RC_PROB_VOX;
  const long h0 = b0 + threadIdx.x * 4;
  const int Cp = C | 1;
  if (h0 < V) {
    const bool v4 = vec && h0 + 3 < V;
    const float* __restrict__ lf = logits + (size_t)f * C * V;
    const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
    const f32x4 s = st.e0 + st.rest;
    float* __restrict__ row = rc_tile + threadIdx.x * 4 * Cp;
    for (int c = 0; c < C; ++c) {                      // voxels past V hold the values of zero logits: never read below
      const f32x4 p = c == 0 ? f32x4{st.e0.x / s.x, st.e0.y / s.y, st.e0.z / s.z, st.e0.w / s.w}
                             : vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), st.m, s);
      row[c] = p.x;
      row[Cp + c] = p.y;
      row[2 * Cp + c] = p.z;
      row[3 * Cp + c] = p.w;
    }
  }
  __syncthreads();
  const long left = V - b0;
  const int n = (int)(left < RC_PROB_VOX ? left : RC_PROB_VOX) * C;              // floats of this block
  float* __restrict__ o = prob + ((size_t)f * V + b0) * C;
  if (vec_out) {                                       // V C % 4 == 0: n % 4 == 0 and o is 16-byte aligned
    for (int i = threadIdx.x * 4; i < n; i += RC_PROB_THREADS * 4) {
      int v = i / C, c = i - v * C;
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        e[k] = rc_tile[v * Cp + c];
        if (++c == C) { c = 0; ++v; }
      }
      *(f32x4*)(o + i) = f32x4{e[0], e[1], e[2], e[3]};
    }
  } else {
    for (int i = threadIdx.x; i < n; i += RC_PROB_THREADS) {
      const int v = i / C;
      o[i] = rc_tile[v * Cp + (i - v * C)];
    }
  }
}

// q = p_0 and p_y of one cell (p_y unused for y == 0)
__device__ __forceinline__ void rc_cell(const float* __restrict__ pf, int C, size_t cell, int y, float& q, float& py) {
  if (C == 2) {
    const float2 c = *(const float2*)(pf + cell * 2);
    q = c.x;
    py = c.y;
  } else {
    q = pf[cell * C];
    py = y >= 1 ? pf[cell * C + y] : 0.f;
  }
}

// ---- forward march.  grid = (ray blocks, frames).  ALL: no early stop at T == 0, so that the cells of every ray are counted (the
// terms added behind T == 0 are exact zeros: S has the same bits either way).
template <bool ALL>
__global__ void __launch_bounds__(RC_THREADS)
render_class_march_kernel(const float* __restrict__ prob, int C, const float* __restrict__ rays, long R, int X, int Y, int Z,
                          const uint8_t* __restrict__ labels, const int32_t* __restrict__ lhit, double* __restrict__ S, int32_t* __restrict__ yout,
                          float* __restrict__ Tn, int32_t* __restrict__ ncell, double* __restrict__ part) {
  __shared__ double red[4];
  const long r = (long)blockIdx.x * RC_THREADS + threadIdx.x;
  const int f = blockIdx.y;
  const size_t V = (size_t)X * Y * Z;
  double cost = 0.0;
  if (r < R) {
    VgRay s;
    int entry;
    const bool valid = vg_start(s, rays + r * 7, X, Y, Z, entry);
    const size_t o = (size_t)f * R + r;
    float T = 1.f;
    double Sv = 0.0;
    int n = 0, y = -1;
    if (valid) {
      const int32_t h = lhit[o];
      y = h >= 0 && (size_t)h < V ? (int)labels[(size_t)f * V + h] : 0;
      if (y >= C) y = -1;                               // a label class the head does not have: the ray takes no part
      const float* __restrict__ pf = prob + (size_t)f * V * C;
      const int bound = X + Y + Z + 3;
      for (int it = 0; it < bound; ++it) {
        const size_t cell = ((size_t)s.cx * Y + s.cy) * Z + s.cz;
        float q, py;
        rc_cell(pf, C, cell, y, q, py);
        if (y >= 1) Sv += (double)T * (double)py;
        T = T * q;
        ++n;
        if (!ALL && T == 0.f) break;
        if (vg_step(s, X, Y, Z) < 0) break;
      }
      if (y == 0) Sv = (double)T;
      if (y >= 0) cost = -log((Sv + RC_EPS) / (1.0 + RC_EPS));
      else Sv = 0.0;
    }
    S[o] = Sv;
    yout[o] = y;
    if (ALL) {
      if (Tn != nullptr) Tn[o] = valid ? T : 0.f;
      if (ncell != nullptr) ncell[o] = valid ? n : -1;
    }
  }
  cost = wave_sum_d(cost);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)f * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// a contribution in fixed point: clamped to +-1, NaN -> 0, rounded to nearest
__device__ __forceinline__ long long rc_fix(double g) {
  g = g > 1.0 ? 1.0 : (g < -1.0 ? -1.0 : (g == g ? g : 0.0));
  return __double2ll_rn(g * (double)(1ll << RC_FIX_BITS));
}

// ---- backward march.  The loop is wave-uniform (it ends when no lane of the wave marches any more): every lane takes part in the
// shuffles of the combine: slot 0 summed over runs of equal cell, slot y over runs of equal (cell, y).
__global__ void __launch_bounds__(RC_THREADS)
render_class_bwd_march_kernel(const float* __restrict__ prob, int C, const float* __restrict__ rays, long R, int X, int Y, int Z,
                              const double* __restrict__ S, const int32_t* __restrict__ yin, unsigned long long* __restrict__ acc) {
  const long r = (long)blockIdx.x * RC_THREADS + threadIdx.x;
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const long V = (long)X * Y * Z;
  VgRay s = {};
  int entry;
  bool active = false;
  double Sv = 0.0, nr = 0.0;
  int y = 0;
  if (r < R && vg_start(s, rays + r * 7, X, Y, Z, entry)) {
    const size_t o = (size_t)f * R + r;
    Sv = S[o];
    y = yin[o];
    active = y >= 0 && y < C && Sv > 0.0;              // S == 0: every A_j and B_j is exactly 0
    if (!active) y = 0;
    nr = -1.0 / (Sv + RC_EPS);
  }
  const float* __restrict__ pf = prob + (size_t)f * V * C;
  unsigned long long* __restrict__ accf = acc + (size_t)f * C * V;
  const long long b0 = rc_fix(Sv * nr);                // y == 0: B_j = T_n = S_0 in every cell
  float T = 1.f;
  double P = 0.0;
  const int bound = X + Y + Z + 3;
  for (int it = 0; it < bound; ++it) {
    if (__ballot(active) == 0ull) break;
    int cell = -1;
    long long va = 0, vb = 0;
    if (active) {
      cell = (s.cx * Y + s.cy) * Z + s.cz;
      float q, py;
      rc_cell(pf, C, (size_t)cell, y, q, py);
      if (y >= 1) {
        const double A = (double)T * (double)py;
        P += A;
        va = rc_fix(A * nr);
        vb = rc_fix((Sv - P) * nr);
      } else {
        vb = b0;
      }
      T = T * q;
      if (T == 0.f || vg_step(s, X, Y, Z) < 0) active = false;      // behind T == 0 every contribution is exactly 0
    }
    const bool in = cell >= 0 && (long)cell < V;
    const int prev = __shfl_up(cell, 1, 64), prevy = __shfl_up(y, 1, 64);
    const bool head = lane == 0 || prev != cell, heady = head || prevy != y;
    vb = vg_run_sum(vb, head, lane);
    va = vg_run_sum(va, heady, lane);
    if (head && in && vb != 0) atomicAdd(accf + cell, (unsigned long long)vb);
    if (heady && in && va != 0) atomicAdd(accf + (size_t)y * V + cell, (unsigned long long)va);
  }
}

__device__ __forceinline__ void rc_ld4(const long long* __restrict__ ap, long h0, long V, bool v4, long long k[4]) {
  if (v4) {
    const rc_i64x2 u = *(const rc_i64x2*)ap, w = *(const rc_i64x2*)(ap + 2);
    k[0] = u.x; k[1] = u.y; k[2] = w.x; k[3] = w.y;
    return;
  }
  k[0] = ap[0];
  k[1] = h0 + 1 < V ? ap[1] : 0;
  k[2] = h0 + 2 < V ? ap[2] : 0;
  k[3] = h0 + 3 < V ? ap[3] : 0;
}

// dlogits[c] = (acc_c - p_c sum_c' acc_c') 2^-37 x gout weight / (F N); the sum over the slots in integers (exact); every element
// is written.  grid = (voxel blocks, frames)
__global__ void __launch_bounds__(RC_THREADS)
render_class_dense_kernel(const float* __restrict__ logits, const long long* __restrict__ acc, int C, long V, int vec, float weight,
                          const float* __restrict__ gout, long N, float* __restrict__ dlogits) {
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * RC_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  const double sc = N > 0 ? (double)gout[0] * (double)weight / ((double)gridDim.y * (double)N) / (double)(1ll << RC_FIX_BITS) : 0.0;
  const long long* __restrict__ af = acc + (size_t)f * C * V + h0;
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  float* __restrict__ df = dlogits + (size_t)f * C * V;
  long long t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  for (int c = 0; c < C; ++c) {
    long long k[4];
    rc_ld4(af + (size_t)c * V, h0, V, v4, k);
    t0 += k[0]; t1 += k[1]; t2 += k[2]; t3 += k[3];
  }
  const double s0 = (double)t0, s1 = (double)t1, s2 = (double)t2, s3 = (double)t3;
  const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
  const f32x4 s = st.e0 + st.rest;
  for (int c = 0; c < C; ++c) {
    const f32x4 p = c == 0 ? f32x4{st.e0.x / s.x, st.e0.y / s.y, st.e0.z / s.z, st.e0.w / s.w}
                           : vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), st.m, s);
    long long k[4];
    rc_ld4(af + (size_t)c * V, h0, V, v4, k);
    vg_st4(df + (size_t)c * V, h0, V, v4,
           f32x4{(float)(((double)k[0] - (double)p.x * s0) * sc), (float)(((double)k[1] - (double)p.y * s1) * sc),
                 (float)(((double)k[2] - (double)p.z * s2) * sc), (float)(((double)k[3] - (double)p.w * s3) * sc)});
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

static inline int64_t rc_up16(int64_t n) { return (n + 15) & ~(int64_t)15; }

struct RcWs {
  float* prob;
  long long* acc;
  double* part;
};
static RcWs rc_ws(void* ws, int64_t F, int64_t C, int64_t V) {
  char* p = (char*)ws;
  const int64_t pb = rc_up16(F * V * C * 4);
  return RcWs{(float*)p, (long long*)(p + pb), (double*)(p + pb + F * C * V * 8)};
}

static int rc_check(const char* who, int64_t F, int C, int X, int Y, int Z, int64_t R, int64_t n_valid, const void* ws, int64_t ws_bytes) {
  if (int rc = vg_check_frames(who, F)) return rc;
  if (int rc = vg_check_classes(who, C)) return rc;
  if (int rc = vg_check_grid(who, X, Y, Z)) return rc;
  if (int rc = vg_check_rays(who, R)) return rc;
  MUVO_CHECK_ARG(n_valid >= 0 && n_valid <= R, "%s: %lld valid rays of %lld", who, (long long)n_valid, (long long)R);
  const int64_t need = muvo_render_class_ws_bytes(F, C, (int64_t)X * Y * Z, R);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need, "%s: workspace of %lld bytes, %lld needed (16-byte aligned)", who,
                 (long long)ws_bytes, (long long)need);
  return MUVO_OK;
}

static void rc_probabilities(const float* logits, int64_t F, int C, int64_t V, const RcWs& w, hipStream_t st) {
  const int vec = (V % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0;       // the workspace is 16-byte aligned
  const int vec_out = (V * C) % 4 == 0 ? 1 : 0;
  hipLaunchKernelGGL(render_class_prob_kernel, dim3((unsigned)((V + RC_PROB_VOX - 1) / RC_PROB_VOX), (unsigned)F), dim3(RC_PROB_THREADS),
                     (size_t)RC_PROB_VOX * (C | 1) * sizeof(float), st, logits, C, (long)V, vec, vec_out, w.prob);
}

extern "C" {

int64_t muvo_render_class_ws_bytes(int64_t F, int C, int64_t V, int64_t R) {
  if (!(vg_frames_ok(F) && C >= 2 && C <= VG_MAXC && vg_voxels_ok(V) && vg_rays_ok(R))) return -1;
  return rc_up16(F * V * C * 4) + F * C * V * 8 + F * ((R + RC_THREADS - 1) / RC_THREADS) * 8;
}

int muvo_render_class_fwd(const float* logits, const uint8_t* labels, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid,
                          const int32_t* label_hit, float weight, void* ws, int64_t ws_bytes, double* mass, int32_t* target, float* t_last,
                          int32_t* cells, float* loss, void* stream) {
  if (int rc = rc_check("render_class_fwd", F, C, X, Y, Z, R, n_valid, ws, ws_bytes)) return rc;
  MUVO_CHECK_ARG(logits && labels && rays && label_hit && mass && target && loss, "render_class_fwd: null pointer");
  MUVO_CHECK_ARG(((uintptr_t)mass & 7) == 0, "render_class_fwd: mass is not 8-byte aligned");
  const int64_t V = (int64_t)X * Y * Z;
  const RcWs w = rc_ws(ws, F, C, V);
  rc_probabilities(logits, F, C, V, w, ST);
  const unsigned nb = (unsigned)((R + RC_THREADS - 1) / RC_THREADS);
  if (t_last || cells)
    hipLaunchKernelGGL(render_class_march_kernel<true>, dim3(nb, (unsigned)F), dim3(RC_THREADS), 0, ST, (const float*)w.prob, C, rays, (long)R, X, Y, Z,
                       labels, label_hit, mass, target, t_last, cells, w.part);
  else
    hipLaunchKernelGGL(render_class_march_kernel<false>, dim3(nb, (unsigned)F), dim3(RC_THREADS), 0, ST, (const float*)w.prob, C, rays, (long)R, X, Y, Z,
                       labels, label_hit, mass, target, (float*)nullptr, (int32_t*)nullptr, w.part);
  hipLaunchKernelGGL(vg_finish_kernel, dim3(1), dim3(256), 0, ST, (const double*)w.part, (long)nb * (long)F, weight, (long)F, (long)n_valid,
                     loss);
  MUVO_CHECK_LAUNCH("render_class_fwd");
  return MUVO_OK;
}

int muvo_render_class_bwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const double* mass,
                          const int32_t* target, float weight, const float* gout, void* ws, int64_t ws_bytes, float* dlogits, void* stream) {
  if (int rc = rc_check("render_class_bwd", F, C, X, Y, Z, R, n_valid, ws, ws_bytes)) return rc;
  MUVO_CHECK_ARG(logits && rays && mass && target && gout && dlogits, "render_class_bwd: null pointer");
  MUVO_CHECK_ARG(((uintptr_t)mass & 7) == 0, "render_class_bwd: mass is not 8-byte aligned");
  const int64_t V = (int64_t)X * Y * Z;
  const RcWs w = rc_ws(ws, F, C, V);
  if (hipMemsetAsync(w.acc, 0, (size_t)F * C * V * 8, ST) != hipSuccess) {
    muvo_set_error("render_class_bwd: clearing the accumulator failed");
    return MUVO_ERR_HIP;
  }
  if (n_valid > 0) {                       // without a valid ray nothing is marched: the dense pass writes zeros
    rc_probabilities(logits, F, C, V, w, ST);
    hipLaunchKernelGGL(render_class_bwd_march_kernel, dim3((unsigned)((R + RC_THREADS - 1) / RC_THREADS), (unsigned)F), dim3(RC_THREADS), 0, ST,
                       (const float*)w.prob, C, rays, (long)R, X, Y, Z, mass, target, (unsigned long long*)w.acc);
  }
  const int vec = (V % 4 == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(render_class_dense_kernel, dim3((unsigned)((V + RC_VOX - 1) / RC_VOX), (unsigned)F), dim3(RC_THREADS), 0, ST, logits,
                     (const long long*)w.acc, C, (long)V, vec, weight, gout, (long)n_valid, dlogits);
  MUVO_CHECK_LAUNCH("render_class_bwd");
  return MUVO_OK;
}

}  // extern "C"
