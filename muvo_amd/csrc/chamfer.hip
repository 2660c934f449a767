// Chamfer-distance training loss of the lidar reconstruction head (CDLoss, muvo/losses.py:352-367, reducer = mean):
//   loss = weight * mean over frames of ( mean_j min_i |p_i - t_j| + mean_i min_j |p_i - t_j| ),  gradient to the prediction only.
// The inputs are the head's tensors as they are: channel-planar (F, C, n) fp32, x / y / z = planes 0 / 1 / 2, further planes never
// read.  No n x n tensor and no interleaved copy: a brute-force nearest-neighbour search that stages the searched set through LDS
// in tiles and keeps, per query point, the smallest squared distance (differences in fp32, never |p|^2 - 2 p.t + |t|^2) and the
// index that achieves it.  Rules: the LOWEST index wins a tie (every lane walks the searched set in ascending order and replaces
// on `<` only); the square root is taken once, for the winner; the gradient of a distance of exactly 0 is exactly 0.
#include "common.h"

#define CD_THREADS 256
#define CD_Q 4                          // query points per lane: one LDS broadcast read serves 4 x 64 pairs
#define CD_QB (CD_THREADS * CD_Q)       // query points per workgroup
#define CD_TILE 1024                    // searched points per LDS tile (16 KB as float4)

// grid = (query blocks, frames, 2 directions).  z = 0: queries = prediction points, searched = target points (idx0, the
// `mean_i min_j` term); z = 1: queries = target points, searched = prediction points (idx1, the `mean_j min_i` term).
// partial[(z * F + f) * gridDim.x + x] = this workgroup's sum of nearest distances (fp64): a plain store, summed in a fixed
// order by chamfer_finalize_kernel - the loss value does not depend on the order in which workgroups finish, nor on whether
// the indices are written.
__global__ void __launch_bounds__(CD_THREADS) chamfer_nn_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                int Cp, int Ct, int n, int* __restrict__ idx0,
                                                                int* __restrict__ idx1, double* __restrict__ partial) {
  __shared__ float4 tile[CD_TILE];
  __shared__ double red[CD_THREADS / 64];
  const int f = blockIdx.y, dir = blockIdx.z;
  const long F = gridDim.y;
  const float* q = dir == 0 ? pred + (long)f * Cp * n : target + (long)f * Ct * n;
  const float* s = dir == 0 ? target + (long)f * Ct * n : pred + (long)f * Cp * n;
  int* idx = dir == 0 ? idx0 : idx1;
  const int q0 = blockIdx.x * CD_QB + threadIdx.x;
  float qx[CD_Q], qy[CD_Q], qz[CD_Q], best[CD_Q];
  int bj[CD_Q];
#pragma unroll
  for (int k = 0; k < CD_Q; ++k) {
    const int i = q0 + k * CD_THREADS, ic = i < n ? i : n - 1;      // lanes past the end search for the last point; never stored
    qx[k] = q[ic]; qy[k] = q[(long)n + ic]; qz[k] = q[2l * n + ic];
    best[k] = INFINITY;
    bj[k] = 0;
  }
  for (int j0 = 0; j0 < n; j0 += CD_TILE) {
    const int len = n - j0 < CD_TILE ? n - j0 : CD_TILE;
    __syncthreads();
    for (int t = threadIdx.x; t < len; t += CD_THREADS) tile[t] = make_float4(s[j0 + t], s[(long)n + j0 + t], s[2l * n + j0 + t], 0.f);
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < len; ++t) {
      const float4 p = tile[t];
      const int j = j0 + t;
#pragma unroll
      for (int k = 0; k < CD_Q; ++k) {
        const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
        const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool lt = d < best[k];
        best[k] = lt ? d : best[k];
        bj[k] = lt ? j : bj[k];
      }
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < CD_Q; ++k) {
    const int i = q0 + k * CD_THREADS;
    if (i < n) {
      sum += (double)sqrtf(best[k]);
      if (idx != nullptr) idx[(long)f * n + i] = bj[k];
    }
  }
  sum = wave_sum_d(sum);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[((long)dir * F + f) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss = weight * (sum of all partial sums) / (F n): one workgroup, a fixed summation tree
__global__ void __launch_bounds__(256) chamfer_finalize_kernel(const double* __restrict__ partial, long count, double inv, float weight,
                                                               float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < count; i += 256) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)((double)weight * red[0] * inv);
}

__device__ __forceinline__ float cd_scale(float weight, const float* gout, long F, int n) {
  return (float)((double)weight * (double)gout[0] / ((double)F * (double)n));
}
// scale * (a - b) / |a - b| per component, exactly 0 where the two points coincide
__device__ __forceinline__ void cd_unit(float ax, float ay, float az, float bx, float by, float bz, float scale, float& gx, float& gy,
                                        float& gz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float d = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
  const float inv = d > 0.f ? scale / d : 0.f;
  gx = dx * inv; gy = dy * inv; gz = dz * inv;
}

// The `mean_i min_j` term is a gather: prediction point i reads its own nearest target idx0[i].  Writes EVERY element of dpred:
// planes 0..2 the gather term, planes >= 3 zero.  grid = (point blocks, frames).
// SCAN (the deterministic mode): the `mean_j min_i` term as a gather too - the workgroup stages (target point, idx1) in tiles,
// every prediction point compares each staged index with its own and sums its senders in ascending index order, so the result
// is bit-reproducible.  CD_Q points per lane as in the search kernel.
template <bool SCAN>
__global__ void __launch_bounds__(CD_THREADS) chamfer_bwd_gather_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                        const int* __restrict__ idx0, const int* __restrict__ idx1,
                                                                        float* __restrict__ dpred, int Cp, int Ct, int n, float weight,
                                                                        const float* __restrict__ gout) {
  __shared__ float4 tile[SCAN ? CD_TILE : 1];
  const int f = blockIdx.y;
  const float scale = cd_scale(weight, gout, gridDim.y, n);
  const float* pf = pred + (long)f * Cp * n;
  const float* tf = target + (long)f * Ct * n;
  float* df = dpred + (long)f * Cp * n;
  constexpr int Q = SCAN ? CD_Q : 1;
  const int i0 = blockIdx.x * (CD_THREADS * Q) + threadIdx.x;
  float px[Q], py[Q], pz[Q], gx[Q], gy[Q], gz[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int i = i0 + k * CD_THREADS, ic = i < n ? i : n - 1;
    px[k] = pf[ic]; py[k] = pf[(long)n + ic]; pz[k] = pf[2l * n + ic];
    int a = idx0[(long)f * n + ic];
    a = a < 0 ? 0 : (a < n ? a : n - 1);              // indices come from the caller's memory: never read outside the frame
    cd_unit(px[k], py[k], pz[k], tf[a], tf[(long)n + a], tf[2l * n + a], scale, gx[k], gy[k], gz[k]);
  }
  if (SCAN) {
    for (int j0 = 0; j0 < n; j0 += CD_TILE) {
      const int len = n - j0 < CD_TILE ? n - j0 : CD_TILE;
      __syncthreads();
      for (int t = threadIdx.x; t < len; t += CD_THREADS)
        tile[t] = make_float4(tf[j0 + t], tf[(long)n + j0 + t], tf[2l * n + j0 + t], __int_as_float(idx1[(long)f * n + j0 + t]));
      __syncthreads();
      for (int t = 0; t < len; ++t) {
        const float4 p = tile[t];
        const int b = __float_as_int(p.w);
#pragma unroll
        for (int k = 0; k < Q; ++k)
          if (b == i0 + k * CD_THREADS) {
            float ux, uy, uz;
            cd_unit(px[k], py[k], pz[k], p.x, p.y, p.z, scale, ux, uy, uz);
            gx[k] += ux; gy[k] += uy; gz[k] += uz;
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int i = i0 + k * CD_THREADS;
    if (i < n) {
      df[i] = gx[k]; df[(long)n + i] = gy[k]; df[2l * n + i] = gz[k];
      for (int c = 3; c < Cp; ++c) df[(long)c * n + i] = 0.f;
    }
  }
}

// The `mean_j min_i` term as a scatter (normal mode): target j adds into its nearest prediction point idx1[j], behind
// chamfer_bwd_gather_kernel<false> in stream order.  Real labels collide heavily - every label pixel without a lidar return
// is the point (0, 0, 0) and all of them pick the same prediction point - so equal destinations are combined within the wave
// first: the wave takes the destination of its first remaining lane, sums the lanes that share it, and that one lane issues
// the three atomics.  grid = (point blocks, frames).
__global__ void __launch_bounds__(CD_THREADS) chamfer_bwd_scatter_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                         const int* __restrict__ idx1, float* __restrict__ dpred, int Cp,
                                                                         int Ct, int n, float weight, const float* __restrict__ gout) {
  const int f = blockIdx.y;
  const float scale = cd_scale(weight, gout, gridDim.y, n);
  const float* pf = pred + (long)f * Cp * n;
  const float* tf = target + (long)f * Ct * n;
  float* df = dpred + (long)f * Cp * n;
  const int j = blockIdx.x * CD_THREADS + threadIdx.x;
  const bool valid = j < n;
  int dst = -1;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (valid) {
    dst = idx1[(long)f * n + j];
    dst = dst < 0 ? 0 : (dst < n ? dst : n - 1);
    cd_unit(pf[dst], pf[(long)n + dst], pf[2l * n + dst], tf[j], tf[(long)n + j], tf[2l * n + j], scale, gx, gy, gz);
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {                                       // wave-uniform loop: one destination per trip
    const int leader = __ffsll((long long)todo) - 1;
    const int d = __shfl(dst, leader, 64);
    const bool mine = valid && dst == d;
    const unsigned long long grp = __ballot(mine);
    float sx = gx, sy = gy, sz = gz;
    if (grp & (grp - 1)) {                             // more than one lane: sum the group (in lane order: a fixed tree)
      sx = wave_sum(mine ? gx : 0.f);
      sy = wave_sum(mine ? gy : 0.f);
      sz = wave_sum(mine ? gz : 0.f);
    }
    if (lane == leader) {
      atomicAdd(df + d, sx);
      atomicAdd(df + (long)n + d, sy);
      atomicAdd(df + 2l * n + d, sz);
    }
    todo &= ~grp;
  }
}

#define ST ((hipStream_t)stream)
#define CD_MAX_N (1 << 30)
extern "C" {

int64_t muvo_chamfer_loss_ws_doubles(int64_t F, int64_t n) {
  if (F <= 0 || n <= 0) return 0;
  return 2 * F * ((n + CD_QB - 1) / CD_QB);
}

int muvo_chamfer_loss_fwd(const float* pred, const float* target, int64_t F, int Cp, int Ct, int64_t n, float weight, double* ws,
                          int32_t* idx_pt, int32_t* idx_tp, float* loss, void* stream) {
  MUVO_CHECK_ARG(pred && target && ws && loss, "chamfer_loss_fwd: null pointer");
  MUVO_CHECK_ARG((idx_pt == nullptr) == (idx_tp == nullptr), "chamfer_loss_fwd: both index arrays or none");
  MUVO_CHECK_ARG(F > 0 && n > 0 && Cp >= 3 && Ct >= 3, "chamfer_loss_fwd: bad args (F=%lld n=%lld Cp=%d Ct=%d, x y z are planes 0..2)",
                 (long long)F, (long long)n, Cp, Ct);
  MUVO_CHECK_ARG(F <= 65535, "chamfer_loss_fwd: more than 65535 frames");
  MUVO_CHECK_ARG(n <= CD_MAX_N, "chamfer_loss_fwd: more than 2^30 points per frame");
  const unsigned nb = (unsigned)((n + CD_QB - 1) / CD_QB);
  hipLaunchKernelGGL(chamfer_nn_kernel, dim3(nb, (unsigned)F, 2), dim3(CD_THREADS), 0, ST, pred, target, Cp, Ct, (int)n, idx_pt, idx_tp, ws);
  hipLaunchKernelGGL(chamfer_finalize_kernel, dim3(1), dim3(256), 0, ST, ws, 2l * F * nb, 1.0 / ((double)F * (double)n), weight, loss);
  MUVO_CHECK_LAUNCH("chamfer_loss_fwd");
  return MUVO_OK;
}

int muvo_chamfer_loss_bwd(const float* pred, const float* target, const int32_t* idx_pt, const int32_t* idx_tp, float* dpred, int64_t F,
                          int Cp, int Ct, int64_t n, float weight, const float* gout, void* stream) {
  MUVO_CHECK_ARG(pred && target && idx_pt && idx_tp && dpred && gout, "chamfer_loss_bwd: null pointer");
  MUVO_CHECK_ARG(F > 0 && n > 0 && Cp >= 3 && Ct >= 3, "chamfer_loss_bwd: bad args (F=%lld n=%lld Cp=%d Ct=%d)", (long long)F,
                 (long long)n, Cp, Ct);
  MUVO_CHECK_ARG(F <= 65535, "chamfer_loss_bwd: more than 65535 frames");
  MUVO_CHECK_ARG(n <= CD_MAX_N, "chamfer_loss_bwd: more than 2^30 points per frame");
  if (muvo_det()) {
    hipLaunchKernelGGL(chamfer_bwd_gather_kernel<true>, dim3((unsigned)((n + CD_QB - 1) / CD_QB), (unsigned)F), dim3(CD_THREADS), 0, ST,
                       pred, target, idx_pt, idx_tp, dpred, Cp, Ct, (int)n, weight, gout);
  } else {
    const dim3 grid((unsigned)((n + CD_THREADS - 1) / CD_THREADS), (unsigned)F);
    hipLaunchKernelGGL(chamfer_bwd_gather_kernel<false>, grid, dim3(CD_THREADS), 0, ST, pred, target, idx_pt, idx_tp, dpred, Cp, Ct,
                       (int)n, weight, gout);
    hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, grid, dim3(CD_THREADS), 0, ST, pred, target, idx_tp, dpred, Cp, Ct, (int)n, weight,
                       gout);
  }
  MUVO_CHECK_LAUNCH("chamfer_loss_bwd");
  return MUVO_OK;
}

}  // extern "C"
