// Point-to-point ICP between lidar frames, all on the device: the registration of the reference's ego-trajectory panel
// (compute_pcd_transformation, muvo/utils/geometry_utils.py:248-267 -> open3d registration_icp) over a work list of P frame
// pairs.  The inputs are the head's / the batch's tensors as they are: channel-planar fp32 (F, C >= 4, n), x / y / z = planes
// 0 / 1 / 2, range = plane 3; a point is valid iff range > 0 (NaN: invalid); coordinates of invalid points never reach a result.
// Per iteration and pair two kernels:
//   icp_correspond_kernel  every valid source point, moved by the pair's T, searches the valid target points exhaustively (LDS
//                          tiles as in chamfer.hip: fp32 differences, lowest index wins a tie), gates the winner by d^2 <= thr^2
//                          and the workgroup stores 17 fp64 sums over its inliers (plain stores, fixed order: no atomics).
//   icp_update_kernel      sums the workgroups' partials in block order, then one lane in fp64: fitness, inlier rmse, the stop
//                          rule of open3d (both deltas < 1e-6), else the rigid fit (icp_fit.h) and T <- U T.
// The state of a pair (ICP_STATE doubles) and its `done` word live on the device; workgroups of a done pair return at once, so
// the host queues iterations in chunks and looks at the P done words once per chunk.
#include "common.h"
#include "icp_fit.h"

#define ICP_THREADS 256
#define ICP_Q 4
#define ICP_QB (ICP_THREADS * ICP_Q)
#define ICP_TILE 1024
#define ICP_STATE 24
// state slots (doubles)
#define ICP_S_FIT 12
#define ICP_S_RMSE 13
#define ICP_S_PFIT 14
#define ICP_S_PRMSE 15
#define ICP_S_INL 16
#define ICP_S_ITER 17
#define ICP_S_STATUS 18
#define ICP_S_EVALS 19
#define ICP_S_NSRC 20
#define ICP_S_NTGT 21
#define ICP_MAX_N (1 << 24)

__device__ __forceinline__ bool icp_valid(float range) { return range > 0.f; }      // false for NaN

// grid = (P).  Counts the valid query points (every stride-th source point) and the valid target points of the pair and writes
// its initial state: T = init or the identity, status running - or empty (identity, done at iteration 0) when either count is
// 0 or a frame index lies outside its tensor.
__global__ void __launch_bounds__(ICP_THREADS) icp_init_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int Fs, int Ft,
                                                               int Cs, int Ct, int n, const int* __restrict__ src_frames,
                                                               const int* __restrict__ tgt_frames, int stride,
                                                               const double* __restrict__ init, double* __restrict__ state,
                                                               int* __restrict__ done) {
  __shared__ int red[2][ICP_THREADS / 64];
  const int p = blockIdx.x;
  const int fs = src_frames[p], ft = tgt_frames[p];
  const bool ok = fs >= 0 && fs < Fs && ft >= 0 && ft < Ft;
  int ns = 0, nt = 0;
  if (ok) {
    const float* sr = src + ((long)fs * Cs + 3) * n;
    const float* tr = tgt + ((long)ft * Ct + 3) * n;
    for (long i = (long)threadIdx.x * stride; i < n; i += (long)ICP_THREADS * stride) ns += icp_valid(sr[i]) ? 1 : 0;
    for (int j = threadIdx.x; j < n; j += ICP_THREADS) nt += icp_valid(tr[j]) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ns += __shfl_xor(ns, o, 64);
    nt += __shfl_xor(nt, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = ns;
    red[1][threadIdx.x >> 6] = nt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ns = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    nt = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    double* st = state + (long)p * ICP_STATE;
    const bool empty = ns == 0 || nt == 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) st[k] = (init != nullptr && !empty) ? init[(long)p * 12 + k] : ((k % 5 == 0) ? 1.0 : 0.0);
#pragma unroll
    for (int k = 12; k < ICP_STATE; ++k) st[k] = 0.0;
    st[ICP_S_STATUS] = empty ? (ok ? MUVO_ICP_EMPTY : MUVO_ICP_BAD_FRAME) : MUVO_ICP_RUNNING;
    st[ICP_S_NSRC] = ns;
    st[ICP_S_NTGT] = nt;
    done[p] = empty ? 1 : 0;
  }
}

// grid = (query blocks, P).  partial[(p * gridDim.x + x) * 17 + k]; corr (P, n) int32 or nullptr: the target index of query
// point i at corr[p * n + i], -1 where the point is invalid or gated out (points that are no query are not written).
__global__ void __launch_bounds__(ICP_THREADS) icp_correspond_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int Cs,
                                                                     int Ct, int n, const int* __restrict__ src_frames,
                                                                     const int* __restrict__ tgt_frames, float scale, float thr2,
                                                                     int stride, const double* __restrict__ state,
                                                                     const int* __restrict__ done, double* __restrict__ partial,
                                                                     int* __restrict__ corr) {
  __shared__ float4 tile[ICP_TILE];
  __shared__ double red[ICP_THREADS / 64][ICP_SUMS];
  const int p = blockIdx.y;
  if (done[p] != 0) return;                                  // uniform over the workgroup
  const float* sf = src + (long)src_frames[p] * Cs * n;      // frames were range-checked by icp_init_kernel (else done)
  const float* tf = tgt + (long)tgt_frames[p] * Ct * n;
  const double* T = state + (long)p * ICP_STATE;
  const double t00 = T[0], t01 = T[1], t02 = T[2], t03 = T[3], t10 = T[4], t11 = T[5], t12 = T[6], t13 = T[7], t20 = T[8], t21 = T[9],
               t22 = T[10], t23 = T[11];
  const int nq = (n + stride - 1) / stride;                  // queries: source points 0, stride, 2 stride, ...
  const int q0 = blockIdx.x * ICP_QB + threadIdx.x;
  float qx[ICP_Q], qy[ICP_Q], qz[ICP_Q], best[ICP_Q];
  int bj[ICP_Q];
  bool live[ICP_Q];
#pragma unroll
  for (int k = 0; k < ICP_Q; ++k) {
    const int iq = q0 + k * ICP_THREADS;
    const long i = (long)(iq < nq ? iq : nq - 1) * stride;   // lanes past the end load the last query; never counted
    live[k] = iq < nq && icp_valid(sf[3l * n + i]);
    const float x = live[k] ? sf[i] * scale : 0.f, y = live[k] ? sf[(long)n + i] * scale : 0.f, z = live[k] ? sf[2l * n + i] * scale : 0.f;
    qx[k] = (float)(t00 * x + t01 * y + t02 * z + t03);
    qy[k] = (float)(t10 * x + t11 * y + t12 * z + t13);
    qz[k] = (float)(t20 * x + t21 * y + t22 * z + t23);
    best[k] = INFINITY;
    bj[k] = -1;
  }
  for (int j0 = 0; j0 < n; j0 += ICP_TILE) {
    const int len = n - j0 < ICP_TILE ? n - j0 : ICP_TILE;
    __syncthreads();
    for (int t = threadIdx.x; t < len; t += ICP_THREADS) {
      const bool v = icp_valid(tf[3l * n + j0 + t]);         // an invalid target sits at +inf: its distance is inf, never < best
      tile[t] = v ? make_float4(tf[j0 + t] * scale, tf[(long)n + j0 + t] * scale, tf[2l * n + j0 + t] * scale, 0.f)
                  : make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < len; ++t) {
      const float4 c = tile[t];
      const int j = j0 + t;
#pragma unroll
      for (int k = 0; k < ICP_Q; ++k) {
        const float dx = qx[k] - c.x, dy = qy[k] - c.y, dz = qz[k] - c.z;
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool lt = d < best[k];
        best[k] = lt ? d : best[k];
        bj[k] = lt ? j : bj[k];
      }
    }
  }
  double acc[ICP_SUMS];
#pragma unroll
  for (int m = 0; m < ICP_SUMS; ++m) acc[m] = 0.0;
#pragma unroll
  for (int k = 0; k < ICP_Q; ++k) {
    const int iq = q0 + k * ICP_THREADS;
    const bool in = live[k] && bj[k] >= 0 && best[k] <= thr2;
    if (in) {
      const int j = bj[k];
      const double s0 = qx[k], s1 = qy[k], s2 = qz[k];
      const double c0 = tf[j] * scale, c1 = tf[(long)n + j] * scale, c2 = tf[2l * n + j] * scale;
      acc[0] += 1.0;
      acc[1] += (double)best[k];
      acc[2] += s0; acc[3] += s1; acc[4] += s2;
      acc[5] += c0; acc[6] += c1; acc[7] += c2;
      acc[8] += s0 * c0; acc[9] += s0 * c1; acc[10] += s0 * c2;
      acc[11] += s1 * c0; acc[12] += s1 * c1; acc[13] += s1 * c2;
      acc[14] += s2 * c0; acc[15] += s2 * c1; acc[16] += s2 * c2;
    }
    if (corr != nullptr && iq < nq) corr[(long)p * n + (long)iq * stride] = in ? bj[k] : -1;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < ICP_SUMS; ++m) {
    const double v = wave_sum_d(acc[m]);
    if (lane == 0) red[w][m] = v;
  }
  __syncthreads();
  if (threadIdx.x < ICP_SUMS)
    partial[((long)p * gridDim.x + blockIdx.x) * ICP_SUMS + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// grid = (P), one wave.  sums (P, 17) or nullptr: the reduced sums of this evaluation (tests).
__global__ void __launch_bounds__(64) icp_update_kernel(const double* __restrict__ partial, int nb, int max_iteration,
                                                        double* __restrict__ state, int* __restrict__ done, double* __restrict__ sums) {
  __shared__ double tot[ICP_SUMS];
  const int p = blockIdx.x;
  if (done[p] != 0) return;
  if (threadIdx.x < ICP_SUMS) {
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += partial[((long)p * nb + b) * ICP_SUMS + threadIdx.x];      // block order: fixed
    tot[threadIdx.x] = s;
    if (sums != nullptr) sums[(long)p * ICP_SUMS + threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double* st = state + (long)p * ICP_STATE;
  const double inl = tot[0];
  const double fit = inl / st[ICP_S_NSRC], rmse = inl > 0.0 ? sqrt(tot[1] / inl) : 0.0;
  const double pfit = st[ICP_S_FIT], prmse = st[ICP_S_RMSE];
  const int evals = (int)st[ICP_S_EVALS], iters = (int)st[ICP_S_ITER];
  st[ICP_S_PFIT] = pfit;
  st[ICP_S_PRMSE] = prmse;
  st[ICP_S_FIT] = fit;
  st[ICP_S_RMSE] = rmse;
  st[ICP_S_INL] = inl;
  st[ICP_S_EVALS] = evals + 1;
  int status = MUVO_ICP_RUNNING;
  if (inl < 3.0) status = MUVO_ICP_FEW_INLIERS;
  else if (evals > 0 && fabs(fit - pfit) < 1e-6 && fabs(rmse - prmse) < 1e-6) status = MUVO_ICP_CONVERGED;
  else if (iters >= max_iteration) status = MUVO_ICP_MAX_ITERATION;
  if (status != MUVO_ICP_RUNNING) {
    st[ICP_S_STATUS] = status;
    done[p] = 1;
    return;
  }
  double U[12], T[12];
  icp_rigid_fit(tot, U);
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = st[k];
  icp_compose(U, T);
#pragma unroll
  for (int k = 0; k < 12; ++k) st[k] = T[k];
  st[ICP_S_ITER] = iters + 1;
}

#define ST ((hipStream_t)stream)
extern "C" {

int64_t muvo_icp_state_doubles(void) { return ICP_STATE; }

int64_t muvo_icp_ws_doubles(int64_t P, int64_t n, int64_t stride) {
  if (P <= 0 || n <= 0 || stride <= 0) return 0;
  const int64_t nq = (n + stride - 1) / stride;
  return P * ((nq + ICP_QB - 1) / ICP_QB) * ICP_SUMS;
}

static int icp_check(const char* who, const void* src, const void* tgt, int Cs, int Ct, int64_t n, const void* sfr, const void* tfr, int64_t P,
                     int64_t stride, const void* state, const void* done) {
  MUVO_CHECK_ARG(src && tgt && sfr && tfr && state && done, "%s: null pointer", who);
  MUVO_CHECK_ARG(Cs >= 4 && Ct >= 4, "%s: Cs=%d Ct=%d (x y z range are planes 0..3)", who, Cs, Ct);
  MUVO_CHECK_ARG(n > 0 && n <= ICP_MAX_N, "%s: n=%lld outside [1, 2^24]", who, (long long)n);
  MUVO_CHECK_ARG(P > 0 && P <= 65535, "%s: P=%lld outside [1, 65535]", who, (long long)P);
  MUVO_CHECK_ARG(stride >= 1 && stride <= n, "%s: source_stride=%lld outside [1, n]", who, (long long)stride);
  return MUVO_OK;
}

int muvo_icp_init(const float* src, const float* tgt, int64_t Fs, int64_t Ft, int Cs, int Ct, int64_t n, const int32_t* src_frames,
                  const int32_t* tgt_frames, int64_t P, int64_t stride, const double* init, double* state, int32_t* done, void* stream) {
  const int rc = icp_check("icp_init", src, tgt, Cs, Ct, n, src_frames, tgt_frames, P, stride, state, done);
  if (rc != MUVO_OK) return rc;
  MUVO_CHECK_ARG(Fs > 0 && Ft > 0 && Fs <= INT32_MAX && Ft <= INT32_MAX, "icp_init: Fs=%lld Ft=%lld", (long long)Fs, (long long)Ft);
  hipLaunchKernelGGL(icp_init_kernel, dim3((unsigned)P), dim3(ICP_THREADS), 0, ST, src, tgt, (int)Fs, (int)Ft, Cs, Ct, (int)n, src_frames,
                     tgt_frames, (int)stride, init, state, done);
  MUVO_CHECK_LAUNCH("icp_init");
  return MUVO_OK;
}

int muvo_icp_iterate(const float* src, const float* tgt, int Cs, int Ct, int64_t n, const int32_t* src_frames, const int32_t* tgt_frames,
                     int64_t P, float scale, float threshold, int64_t stride, int max_iteration, int count, double* ws, double* state,
                     int32_t* done, int32_t* corr, double* sums, void* stream) {
  const int rc = icp_check("icp_iterate", src, tgt, Cs, Ct, n, src_frames, tgt_frames, P, stride, state, done);
  if (rc != MUVO_OK) return rc;
  MUVO_CHECK_ARG(ws != nullptr, "icp_iterate: null workspace");
  MUVO_CHECK_ARG(scale > 0.f && threshold > 0.f && max_iteration >= 0 && count >= 1,
                 "icp_iterate: scale=%g threshold=%g max_iteration=%d count=%d", (double)scale, (double)threshold, max_iteration, count);
  const int64_t nq = (n + stride - 1) / stride;
  const unsigned nb = (unsigned)((nq + ICP_QB - 1) / ICP_QB);
  for (int it = 0; it < count; ++it) {
    hipLaunchKernelGGL(icp_correspond_kernel, dim3(nb, (unsigned)P), dim3(ICP_THREADS), 0, ST, src, tgt, Cs, Ct, (int)n, src_frames,
                       tgt_frames, scale, threshold * threshold, (int)stride, state, done, ws, corr);
    hipLaunchKernelGGL(icp_update_kernel, dim3((unsigned)P), dim3(64), 0, ST, ws, (int)nb, max_iteration, state, done, sums);
  }
  MUVO_CHECK_LAUNCH("icp_iterate");
  return MUVO_OK;
}

}  // extern "C"
