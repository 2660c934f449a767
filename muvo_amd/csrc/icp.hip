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
// Two searches give the same bits: the exhaustive one above and icp_correspond_grid_kernel over a uniform cell grid of the
// target points (built once per registration, "grid search" below).  Both end in the same icp_gate_add / icp_reduce_store.
// Atomics only in the grid build, where only the order inside a cell depends on them: no result depends on scheduling.
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

// ---- the steps both correspond kernels share ------------------------------------------------------------------------------
// query point i of the pair, scaled in fp32, moved by T in fp64 and rounded to fp32 (a point that is not live: the origin)
__device__ __forceinline__ void icp_move_query(const float* __restrict__ sf, int n, long i, bool live, float scale, const double* __restrict__ T,
                                               float& qx, float& qy, float& qz) {
  const float x = live ? sf[i] * scale : 0.f, y = live ? sf[(long)n + i] * scale : 0.f, z = live ? sf[2l * n + i] * scale : 0.f;
  qx = (float)(T[0] * x + T[1] * y + T[2] * z + T[3]);
  qy = (float)(T[4] * x + T[5] * y + T[6] * z + T[7]);
  qz = (float)(T[8] * x + T[9] * y + T[10] * z + T[11]);
}

// gate of one query by d^2 <= thr^2, its 17 terms, its corr entry (iq: the query's number, written iff iq < nq)
__device__ __forceinline__ void icp_gate_add(double (&acc)[ICP_SUMS], bool live, int bj, float best, float thr2, float qx, float qy, float qz,
                                             const float* __restrict__ tf, int n, float scale, int* __restrict__ corr, int p, int iq, int nq,
                                             int stride) {
  const bool in = live && bj >= 0 && best <= thr2;
  if (in) {
    const int j = bj;
    const double s0 = qx, s1 = qy, s2 = qz;
    const double c0 = tf[j] * scale, c1 = tf[(long)n + j] * scale, c2 = tf[2l * n + j] * scale;
    acc[0] += 1.0;
    acc[1] += (double)best;
    acc[2] += s0; acc[3] += s1; acc[4] += s2;
    acc[5] += c0; acc[6] += c1; acc[7] += c2;
    acc[8] += s0 * c0; acc[9] += s0 * c1; acc[10] += s0 * c2;
    acc[11] += s1 * c0; acc[12] += s1 * c1; acc[13] += s1 * c2;
    acc[14] += s2 * c0; acc[15] += s2 * c1; acc[16] += s2 * c2;
  }
  if (corr != nullptr && iq < nq) corr[(long)p * n + (long)iq * stride] = in ? bj : -1;
}

// wave sums, then the four waves in a fixed order, one plain store per sum
__device__ __forceinline__ void icp_reduce_store(const double (&acc)[ICP_SUMS], double (*red)[ICP_SUMS], double* __restrict__ partial, int p) {
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
    icp_move_query(sf, n, i, live[k], scale, T, qx[k], qy[k], qz[k]);
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
  for (int k = 0; k < ICP_Q; ++k)
    icp_gate_add(acc, live[k], bj[k], best[k], thr2, qx[k], qy[k], qz[k], tf, n, scale, corr, p, q0 + k * ICP_THREADS, nq, stride);
  icp_reduce_store(acc, red, partial, p);
}

// ---- grid search ---------------------------------------------------------------------------------------------------------------
// What the exhaustive search contributes is, per query, the lexicographic minimum of (fp32 d^2, target index) over the valid
// targets - and only where that d^2 <= thr^2.  So it is enough to find that minimum among the targets that CAN have d^2 <= thr^2.
// The valid targets of a pair whose three scaled coordinates are finite (any other has d = NaN or +inf against every query and
// never wins above) are binned once per registration - the pose moves only the sources - into cubic cells of edge h over their
// bounding box:
//     cell(v) = clamp(floor((v - lo) * (1 / h)), 0, dim - 1) per axis, all in fp32, the clamp on integers         (icp_cell)
// which is monotone in v whatever lo, h and dim are: every step (subtract a constant, multiply by a positive constant, floor,
// clamp) is.  Everything below uses only that and the monotony of fp32 rounding - no exact-arithmetic geometry.
// Cell edge: h = thr / 8, doubled until the box has at most ICP_GRID_CELLS cells (dim = floor(extent / h) + 2 per axis, fp64 on
// one lane).  Consecutive lidar frames put the nearest neighbour of most queries within a ring spacing (decimetres near the
// sensor, 1-2 m far out) while the reference's threshold is 5 m: cells of the threshold's size would make every query read 27
// cells of several hundred points, an eighth lets most queries stop after the 27 or 125 cells around them, a few dozen
// points.  The cap bounds the workspace (4 B per cell) and the scan; a cloud spread far beyond thr / 8 x 2^17 gets larger
// cells, one at 1e30 among ordinary points leaves those in a single cell (the exhaustive search again, correct all the same).
// Layout per pair (icp_grid_pair_bytes): 16 header words {lo x y z, h, 1 / h, dim x y z}, ICP_GRID_CELLS + 16 ints `cend`, n
// records float4 {x, y, z, index bits}.  cend[c + 1] is the counter of cell c (x fastest): the histogram counts into it, the
// exclusive scan turns it into the cell's first record, the scatter's atomic cursor leaves it at the cell's end = the next
// cell's start; cend[0] = 0.  A run of cells c0..c1 of one x row is the records cend[c0] .. cend[c1 + 1].
// The order of the records inside a cell depends on the arrival of the atomics and nothing else does; the winner rule is
// lexicographic, so no result depends on it.
#define ICP_GRID_CELLS (1 << 17)
#define ICP_GRID_HEAD 16
#define ICP_GRID_CEND (ICP_GRID_CELLS + 16)
#define ICP_GRID_THREADS 256
#define ICP_SCAN_THREADS 1024
#define ICP_GRID_BATCH 8

__host__ __device__ __forceinline__ long icp_grid_pair_bytes(long n) { return 4l * (ICP_GRID_HEAD + ICP_GRID_CEND) + 16l * n; }

__device__ __forceinline__ bool icp_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// The one cell function of the build and the query.  t is +-inf where v is (the ends q -+ r of a query box with r = inf) or
// where v - lo overflows: the test in the float domain sends everything beyond +-2^24 (dim <= 2^17) and NaN to a defined
// integer before the conversion, the clamp itself is on integers.
__device__ __forceinline__ int icp_cell(float v, float lo, float inv, int dim) {
  const float t = floorf((v - lo) * inv);
  const int c = t >= 16777216.f ? (1 << 24) : (t > -16777216.f ? (int)t : -(1 << 24));
  return min(max(c, 0), dim - 1);
}

struct IcpGrid {
  float lx, ly, lz, h, inv;
  int dx, dy, dz;
};

// the header as the query reads it: dims cut to what the cend array can index, whatever the words hold
__device__ __forceinline__ IcpGrid icp_grid_head(const int* __restrict__ head) {
  IcpGrid g;
  g.lx = __int_as_float(head[0]); g.ly = __int_as_float(head[1]); g.lz = __int_as_float(head[2]);
  g.h = __int_as_float(head[3]); g.inv = __int_as_float(head[4]);
  g.dx = min(max(head[5], 1), ICP_GRID_CELLS);
  g.dy = min(max(head[6], 1), ICP_GRID_CELLS / g.dx);
  g.dz = min(max(head[7], 1), ICP_GRID_CELLS / (g.dx * g.dy));
  return g;
}

// target j of the frame: true iff it is in the grid; its scaled coordinates as the exhaustive search loads them
__device__ __forceinline__ bool icp_grid_point(const float* __restrict__ tf, int n, int j, float scale, float& x, float& y, float& z) {
  if (!icp_valid(tf[3l * n + j])) return false;
  x = tf[j] * scale; y = tf[(long)n + j] * scale; z = tf[2l * n + j] * scale;
  return icp_finite(x) && icp_finite(y) && icp_finite(z);
}

__device__ __forceinline__ int icp_grid_cell_of(const IcpGrid& g, float x, float y, float z) {
  return (icp_cell(z, g.lz, g.inv, g.dz) * g.dy + icp_cell(y, g.ly, g.inv, g.dy)) * g.dx + icp_cell(x, g.lx, g.inv, g.dx);
}

// grid = (P).  Bounding box of the pair's grid points, the cell edge, the header; zeroes the cell counters.
__global__ void __launch_bounds__(ICP_GRID_THREADS) icp_grid_box_kernel(const float* __restrict__ tgt, int Ct, int n, const int* __restrict__ tgt_frames,
                                                                         float scale, float thr, const int* __restrict__ done,
                                                                         char* __restrict__ grid) {
  __shared__ float red[6][ICP_GRID_THREADS / 64];
  __shared__ int cells;
  const int p = blockIdx.x;
  if (done[p] != 0) return;
  const float* tf = tgt + (long)tgt_frames[p] * Ct * n;
  int* head = (int*)(grid + (long)p * icp_grid_pair_bytes(n));
  float lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY;
  for (int j = threadIdx.x; j < n; j += ICP_GRID_THREADS) {
    float x, y, z;
    if (icp_grid_point(tf, n, j, scale, x, y, z)) {
      lo0 = fminf(lo0, x); lo1 = fminf(lo1, y); lo2 = fminf(lo2, z);
      hi0 = fmaxf(hi0, x); hi1 = fmaxf(hi1, y); hi2 = fmaxf(hi2, z);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo0 = fminf(lo0, __shfl_xor(lo0, o, 64)); lo1 = fminf(lo1, __shfl_xor(lo1, o, 64)); lo2 = fminf(lo2, __shfl_xor(lo2, o, 64));
    hi0 = fmaxf(hi0, __shfl_xor(hi0, o, 64)); hi1 = fmaxf(hi1, __shfl_xor(hi1, o, 64)); hi2 = fmaxf(hi2, __shfl_xor(hi2, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[0][w] = lo0; red[1][w] = lo1; red[2][w] = lo2; red[3][w] = hi0; red[4][w] = hi1; red[5][w] = hi2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo0 = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    lo1 = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
    lo2 = fminf(fminf(red[2][0], red[2][1]), fminf(red[2][2], red[2][3]));
    hi0 = fmaxf(fmaxf(red[3][0], red[3][1]), fmaxf(red[3][2], red[3][3]));
    hi1 = fmaxf(fmaxf(red[4][0], red[4][1]), fmaxf(red[4][2], red[4][3]));
    hi2 = fmaxf(fmaxf(red[5][0], red[5][1]), fmaxf(red[5][2], red[5][3]));
    if (!(lo0 <= hi0)) lo0 = lo1 = lo2 = hi0 = hi1 = hi2 = 0.f;           // no grid point at all: an empty grid at the origin
    const double e0 = (double)hi0 - lo0, e1 = (double)hi1 - lo1, e2 = (double)hi2 - lo2;      // fp64: finite for all fp32 ends
    // h in [2^-100, 2^126]: 1 / h is a normal fp32 number; a power of two times thr / 8 (or a bound): exact in fp32
    double h = fmin(fmax((double)(thr * 0.125f), 0x1p-100), 0x1p126);
    double d0, d1, d2;
    for (;;) {                                                             // ends at h = 2^126 at the latest: extents < 2^129
      d0 = floor(e0 / h) + 2.0; d1 = floor(e1 / h) + 2.0; d2 = floor(e2 / h) + 2.0;
      if (d0 * d1 * d2 <= (double)ICP_GRID_CELLS || h >= 0x1p126) break;
      h = fmin(h * 2.0, 0x1p126);
    }
    const float hf = (float)h;
    head[0] = __float_as_int(lo0); head[1] = __float_as_int(lo1); head[2] = __float_as_int(lo2);
    head[3] = __float_as_int(hf); head[4] = __float_as_int(1.f / hf);
    head[5] = (int)d0; head[6] = (int)d1; head[7] = (int)d2;
    cells = (int)(d0 * d1 * d2);
  }
  __syncthreads();
  int* cend = head + ICP_GRID_HEAD;
  const int nc = min(cells, ICP_GRID_CELLS);
  for (int c = threadIdx.x; c <= nc; c += ICP_GRID_THREADS) cend[c] = 0;
}

// grid = (target blocks, P).  scatter = false: counts the points per cell; true: writes the records behind the cells' cursors.
template <bool SCATTER>
__global__ void __launch_bounds__(ICP_GRID_THREADS) icp_grid_bin_kernel(const float* __restrict__ tgt, int Ct, int n, const int* __restrict__ tgt_frames,
                                                                         float scale, const int* __restrict__ done, char* __restrict__ grid) {
  const int p = blockIdx.y;
  if (done[p] != 0) return;
  const int j = blockIdx.x * ICP_GRID_THREADS + threadIdx.x;
  if (j >= n) return;
  const float* tf = tgt + (long)tgt_frames[p] * Ct * n;
  int* head = (int*)(grid + (long)p * icp_grid_pair_bytes(n));
  int* cend = head + ICP_GRID_HEAD;
  float x, y, z;
  if (!icp_grid_point(tf, n, j, scale, x, y, z)) return;
  const IcpGrid g = icp_grid_head(head);
  const int c = icp_grid_cell_of(g, x, y, z);                  // in [0, ICP_GRID_CELLS): the dims are cut to that
  if (!SCATTER) {
    atomicAdd(&cend[c + 1], 1);
  } else {
    const int at = atomicAdd(&cend[c + 1], 1);                 // < the number of grid points <= n: the same points were counted
    float4* rec = (float4*)(cend + ICP_GRID_CEND);
    if (at >= 0 && at < n) rec[at] = make_float4(x, y, z, __int_as_float(j));
  }
}

// grid = (P).  cend[1 .. cells] counts -> exclusive prefix sums (the first record of every cell), in place: every lane sums a
// contiguous piece, the pieces' sums are scanned through LDS, every lane writes its piece.
__global__ void __launch_bounds__(ICP_SCAN_THREADS) icp_grid_scan_kernel(int n, const int* __restrict__ done, char* __restrict__ grid) {
  __shared__ int part[ICP_SCAN_THREADS];
  const int p = blockIdx.x;
  if (done[p] != 0) return;
  int* head = (int*)(grid + (long)p * icp_grid_pair_bytes(n));
  int* cnt = head + ICP_GRID_HEAD + 1;
  const IcpGrid g = icp_grid_head(head);
  const int nc = g.dx * g.dy * g.dz;
  const int per = (nc + ICP_SCAN_THREADS - 1) / ICP_SCAN_THREADS;
  const int a = min((int)threadIdx.x * per, nc), b = min(a + per, nc);
  int s = 0;
  for (int c = a; c < b; ++c) s += cnt[c];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < ICP_SCAN_THREADS; o <<= 1) {             // inclusive scan of the pieces
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int c = a; c < b; ++c) {
    const int v = cnt[c];
    cnt[c] = run;
    run += v;
  }
}

// The nearest grid point of one query: (best, bj) = the lexicographic minimum of (d, index) over the cells walked.
// COVERAGE.  A target with fp32 d <= thr2 is in a walked cell unless the walk stops early (below).  d = fl(dz^2 + fl(dy^2 +
// fl(dx^2))) is >= fl(da^2) for each axis a (the other terms are >= 0 and rounding is monotone), so fl(da^2) <= thr2 =
// fl(thr^2): where da^2 is a normal number |da| <= thr (1 + 2^-23), where it is not |da| < 2^-63; da = fl(q_a - p_a) has a
// relative error of 2^-24 at most, so the real |q_a - p_a| <= r = max(thr (1 + 2^-12), 2^-60) with a wide margin.  q_a - r <=
// p_a <= q_a + r in the reals, p_a is an fp32 number and rounding is monotone: fl(q_a - r) <= p_a <= fl(q_a + r), and cell() is
// monotone: cell(fl(q_a - r)) <= cell(p_a) <= cell(fl(q_a + r)) - the walked range per axis, clamps included, r = inf included.
// EARLY EXIT.  After ring k (all cells of the range within Chebyshev distance k of the query's cell c) an unvisited grid point p
// of the range lies, on some axis a, in a cell above e = c_a + k or below e = c_a - k (icp_side_gap, six sides).  Above: with a
// guess G of the border the lane TESTS cell(prev(G)) <= e with the same cell(), prev = the next fp32 number below: then monotony
// gives p_a > prev(G), that is p_a >= G, and |fl(q_a - p_a)| >= fl(G - q_a).  Below: cell(next(G)) >= e gives p_a <= G and
// |fl(q_a - p_a)| >= fl(q_a - G).  G is the border lo + (e + 1) h or lo + e h itself and, if the test fails there (rounding),
// the border moved by h / 64 towards the query; if that fails too the side gives 0 and the walk goes on.  A side with no
// cell of the range left gives +inf.  With m the smallest of the six, d >= fl(da^2) >= fl(m^2) = L: inequalities between
// rounded values - the rounding of d is inside them, there is no margin to add.  The walk stops only if best < L: every
// unvisited point of the range then has d >= L > best and can neither win nor tie.  The comparison that CONTINUES is L <= best:
// a point exactly on the upper border G is in the next cell, can have d = L = best and a lower index, and must still win.
// It also stops if thr2 < L: no unvisited point is an inlier, and the best so far is the true minimum or above thr2 like it.
__device__ __forceinline__ float icp_side_gap(float q, float lo, float inv, float h, int dim, int e, bool above) {
  const float border = lo + (float)(above ? e + 1 : e) * h;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float s = t == 0 ? 0.f : h * 0.015625f;
    const float G = above ? border - s : border + s;
    const int c = icp_cell(nextafterf(G, above ? -INFINITY : INFINITY), lo, inv, dim);
    if (above ? c <= e : c >= e) return fmaxf(above ? G - q : q - G, 0.f);
  }
  return 0.f;
}

// one candidate record against the best so far: smaller d wins, on equal d the lower target index
__device__ __forceinline__ void icp_grid_candidate(const float4 c, float qx, float qy, float qz, float& best, int& bj) {
  const int j = __float_as_int(c.w);
  const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
  const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
  const bool lt = d < best || (d == best && j < bj);
  best = lt ? d : best;
  bj = lt ? j : bj;
}

__device__ __forceinline__ void icp_grid_nearest(const IcpGrid& g, const int* __restrict__ cend, const float4* __restrict__ rec, int n, float qx,
                                                 float qy, float qz, float r, float thr2, float& best, int& bj) {
  best = INFINITY;
  bj = -1;
  if (!(icp_finite(qx) && icp_finite(qy) && icp_finite(qz))) return;      // no candidate: every d is NaN or inf
  const int cx = icp_cell(qx, g.lx, g.inv, g.dx), cy = icp_cell(qy, g.ly, g.inv, g.dy), cz = icp_cell(qz, g.lz, g.inv, g.dz);
  const int x0 = icp_cell(qx - r, g.lx, g.inv, g.dx), x1 = icp_cell(qx + r, g.lx, g.inv, g.dx);
  const int y0 = icp_cell(qy - r, g.ly, g.inv, g.dy), y1 = icp_cell(qy + r, g.ly, g.inv, g.dy);
  const int z0 = icp_cell(qz - r, g.lz, g.inv, g.dz), z1 = icp_cell(qz + r, g.lz, g.inv, g.dz);
  const int kmax = max(max(max(cx - x0, x1 - cx), max(cy - y0, y1 - cy)), max(cz - z0, z1 - cz));
#pragma unroll 1
  for (int k = 0; k <= kmax; ++k) {
    const int za = max(z0, cz - k), zb = min(z1, cz + k), ya = max(y0, cy - k), yb = min(y1, cy + k);
    const int xa = max(x0, cx - k), xb = min(x1, cx + k);
#pragma unroll 1
    for (int z = za; z <= zb; ++z) {
#pragma unroll 1
      for (int y = ya; y <= yb; ++y) {
        const int row = (z * g.dy + y) * g.dx;
        const bool face = z - cz == k || cz - z == k || y - cy == k || cy - y == k;      // the whole x run belongs to ring k
        // else the two ends cx - k and cx + k, each if inside the range (k > 0 here: k = 0 is a face)
#pragma unroll 1
        for (int e = 0; e < (face ? 1 : 2); ++e) {
          const int a = face ? xa : (e == 0 ? cx - k : cx + k), b = face ? xb : a;
          if (a < x0 || b > x1) continue;
          const int first = max(cend[row + a], 0), last = min(cend[row + b + 1], n);
          // eight independent 16-byte loads in flight per lane: the walk is bound by the latency of these loads (L2), most of all
          // at source_stride > 1 where a SIMD holds one wave; the order of the candidates does not matter to the winner
          int i = first;
#pragma unroll 1
          for (; i + ICP_GRID_BATCH <= last; i += ICP_GRID_BATCH) {
            float4 c[ICP_GRID_BATCH];
#pragma unroll
            for (int u = 0; u < ICP_GRID_BATCH; ++u) c[u] = rec[i + u];
#pragma unroll
            for (int u = 0; u < ICP_GRID_BATCH; ++u) icp_grid_candidate(c[u], qx, qy, qz, best, bj);
          }
#pragma unroll 1
          for (; i < last; ++i) icp_grid_candidate(rec[i], qx, qy, qz, best, bj);
        }
      }
    }
    if (k == kmax) break;
    const float m = fminf(fminf(fminf(cx + k >= x1 ? INFINITY : icp_side_gap(qx, g.lx, g.inv, g.h, g.dx, cx + k, true),
                                      cx - k <= x0 ? INFINITY : icp_side_gap(qx, g.lx, g.inv, g.h, g.dx, cx - k, false)),
                                fminf(cy + k >= y1 ? INFINITY : icp_side_gap(qy, g.ly, g.inv, g.h, g.dy, cy + k, true),
                                      cy - k <= y0 ? INFINITY : icp_side_gap(qy, g.ly, g.inv, g.h, g.dy, cy - k, false))),
                          fminf(cz + k >= z1 ? INFINITY : icp_side_gap(qz, g.lz, g.inv, g.h, g.dz, cz + k, true),
                                cz - k <= z0 ? INFINITY : icp_side_gap(qz, g.lz, g.inv, g.h, g.dz, cz - k, false)));
    const float L = m * m;
    if (best < L || thr2 < L) break;
  }
}

// grid = (query blocks, P) as icp_correspond_kernel, the same queries per workgroup and lane, the same order of a lane's
// ICP_Q queries in its sums; one lane walks the cells of one query at a time and reads the records from global memory (1 MB
// per pair at n = 65,536: L2).
__global__ void __launch_bounds__(ICP_THREADS) icp_correspond_grid_kernel(const float* __restrict__ src, const float* __restrict__ tgt, int Cs,
                                                                          int Ct, int n, const int* __restrict__ src_frames,
                                                                          const int* __restrict__ tgt_frames, float scale, float thr,
                                                                          float thr2, int stride, const double* __restrict__ state,
                                                                          const int* __restrict__ done, const char* __restrict__ grid,
                                                                          double* __restrict__ partial, int* __restrict__ corr) {
  __shared__ double red[ICP_THREADS / 64][ICP_SUMS];
  const int p = blockIdx.y;
  if (done[p] != 0) return;                                  // uniform over the workgroup
  const float* sf = src + (long)src_frames[p] * Cs * n;
  const float* tf = tgt + (long)tgt_frames[p] * Ct * n;
  const double* T = state + (long)p * ICP_STATE;
  const int* head = (const int*)(grid + (long)p * icp_grid_pair_bytes(n));
  const int* cend = head + ICP_GRID_HEAD;
  const float4* rec = (const float4*)(cend + ICP_GRID_CEND);
  const IcpGrid g = icp_grid_head(head);
  const float r = fmaxf(thr * (1.f + 0x1p-12f), 0x1p-60f);
  const int nq = (n + stride - 1) / stride;
  const int q0 = blockIdx.x * ICP_QB + threadIdx.x;
  double acc[ICP_SUMS];
#pragma unroll
  for (int m = 0; m < ICP_SUMS; ++m) acc[m] = 0.0;
#pragma unroll 1
  for (int k = 0; k < ICP_Q; ++k) {
    const int iq = q0 + k * ICP_THREADS;
    const long i = (long)(iq < nq ? iq : nq - 1) * stride;
    const bool live = iq < nq && icp_valid(sf[3l * n + i]);
    float qx, qy, qz, best = INFINITY;
    int bj = -1;
    icp_move_query(sf, n, i, live, scale, T, qx, qy, qz);
    if (live) icp_grid_nearest(g, cend, rec, n, qx, qy, qz, r, thr2, best, bj);
    if ((unsigned)bj >= (unsigned)n) bj = -1;                // a record of a built grid never is: the index reads the target frame
    icp_gate_add(acc, live, bj, best, thr2, qx, qy, qz, tf, n, scale, corr, p, iq, nq, stride);
  }
  icp_reduce_store(acc, red, partial, p);
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

int64_t muvo_icp_grid_bytes(int64_t P, int64_t n) {
  if (P <= 0 || n <= 0 || n > ICP_MAX_N) return 0;
  return P * (int64_t)icp_grid_pair_bytes((long)n);
}

static int icp_grid_check(const char* who, int64_t P, int64_t n, const void* grid, int64_t grid_bytes) {
  MUVO_CHECK_ARG(grid != nullptr && ((uintptr_t)grid & 15) == 0, "%s: the grid workspace is null or not 16-byte aligned", who);
  MUVO_CHECK_ARG(grid_bytes >= muvo_icp_grid_bytes(P, n), "%s: grid_bytes=%lld below muvo_icp_grid_bytes(%lld, %lld)=%lld", who,
                 (long long)grid_bytes, (long long)P, (long long)n, (long long)muvo_icp_grid_bytes(P, n));
  return MUVO_OK;
}

int muvo_icp_grid_build(const float* tgt, int Ct, int64_t n, const int32_t* tgt_frames, int64_t P, float scale, float threshold,
                        const int32_t* done, void* grid, int64_t grid_bytes, void* stream) {
  MUVO_CHECK_ARG(tgt && tgt_frames && done, "icp_grid_build: null pointer");
  MUVO_CHECK_ARG(Ct >= 4, "icp_grid_build: Ct=%d (x y z range are planes 0..3)", Ct);
  MUVO_CHECK_ARG(n > 0 && n <= ICP_MAX_N, "icp_grid_build: n=%lld outside [1, 2^24]", (long long)n);
  MUVO_CHECK_ARG(P > 0 && P <= 65535, "icp_grid_build: P=%lld outside [1, 65535]", (long long)P);
  MUVO_CHECK_ARG(scale > 0.f && threshold > 0.f, "icp_grid_build: scale=%g threshold=%g", (double)scale, (double)threshold);
  const int rc = icp_grid_check("icp_grid_build", P, n, grid, grid_bytes);
  if (rc != MUVO_OK) return rc;
  const dim3 bins((unsigned)((n + ICP_GRID_THREADS - 1) / ICP_GRID_THREADS), (unsigned)P);
  hipLaunchKernelGGL(icp_grid_box_kernel, dim3((unsigned)P), dim3(ICP_GRID_THREADS), 0, ST, tgt, Ct, (int)n, tgt_frames, scale, threshold, done,
                     (char*)grid);
  hipLaunchKernelGGL(icp_grid_bin_kernel<false>, bins, dim3(ICP_GRID_THREADS), 0, ST, tgt, Ct, (int)n, tgt_frames, scale, done, (char*)grid);
  hipLaunchKernelGGL(icp_grid_scan_kernel, dim3((unsigned)P), dim3(ICP_SCAN_THREADS), 0, ST, (int)n, done, (char*)grid);
  hipLaunchKernelGGL(icp_grid_bin_kernel<true>, bins, dim3(ICP_GRID_THREADS), 0, ST, tgt, Ct, (int)n, tgt_frames, scale, done, (char*)grid);
  MUVO_CHECK_LAUNCH("icp_grid_build");
  return MUVO_OK;
}

int muvo_icp_iterate_grid(const float* src, const float* tgt, int Cs, int Ct, int64_t n, const int32_t* src_frames, const int32_t* tgt_frames,
                          int64_t P, float scale, float threshold, int64_t stride, int max_iteration, int count, double* ws, double* state,
                          int32_t* done, int32_t* corr, double* sums, const void* grid, int64_t grid_bytes, void* stream) {
  int rc = icp_check("icp_iterate_grid", src, tgt, Cs, Ct, n, src_frames, tgt_frames, P, stride, state, done);
  if (rc != MUVO_OK) return rc;
  MUVO_CHECK_ARG(ws != nullptr, "icp_iterate_grid: null workspace");
  MUVO_CHECK_ARG(scale > 0.f && threshold > 0.f && max_iteration >= 0 && count >= 1,
                 "icp_iterate_grid: scale=%g threshold=%g max_iteration=%d count=%d", (double)scale, (double)threshold, max_iteration, count);
  rc = icp_grid_check("icp_iterate_grid", P, n, grid, grid_bytes);
  if (rc != MUVO_OK) return rc;
  const int64_t nq = (n + stride - 1) / stride;
  const unsigned nb = (unsigned)((nq + ICP_QB - 1) / ICP_QB);
  for (int it = 0; it < count; ++it) {
    hipLaunchKernelGGL(icp_correspond_grid_kernel, dim3(nb, (unsigned)P), dim3(ICP_THREADS), 0, ST, src, tgt, Cs, Ct, (int)n, src_frames,
                       tgt_frames, scale, threshold, threshold * threshold, (int)stride, state, done, (const char*)grid, ws, corr);
    hipLaunchKernelGGL(icp_update_kernel, dim3((unsigned)P), dim3(64), 0, ST, ws, (int)nb, max_iteration, state, done, sums);
  }
  MUVO_CHECK_LAUNCH("icp_iterate_grid");
  return MUVO_OK;
}

}  // extern "C"
