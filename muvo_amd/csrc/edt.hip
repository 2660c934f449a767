// Exact Euclidean distance transform of voxel class grids and its two users, the distance-transform boundary loss of the voxel head
// and the voxel Chamfer / F-score counts (extensions, the reference has none of them).  include/muvo_hip.h
// (muvo_voxel_edt, muvo_voxel_boundary_forward, muvo_voxel_cd_counts) holds the definitions; tests/edt_reference.py restates them.
//   transform   three separable min-plus passes d(i) = min_j (i - j)^2 + d(j) in 32-bit integers, z then y then x, capped after each
//               pass.  ONE kernel serves the three: a pass sees the array as `cols` independent columns of N elements, `inner` apart
//               (z: inner 1, y: inner Z, x: inner Y Z).  A workgroup owns 64 neighbouring columns x 32 output rows; the input rows
//               it needs - its own and `radius` rows either side, radius^2 < cap <= radius^2 + 2 radius + 1: an offset beyond it
//               cannot beat the cap, so a truncated call is a window and the untruncated one (radius = N - 1) the whole column -
//               pass through an LDS tile of 32 rows x 64 columns (row stride 65 words).  Tile <-> memory copies run along the
//               direction that is contiguous in memory (z pass: down the column, the 64 columns of a tile being one span of
//               memory when Z <= 32; y and x pass: across the columns), the min-plus loop reads the tile one column per lane - both
//               without bank conflicts at stride 65.  A thread keeps 8 output rows of one column in registers; the results leave
//               through the same tile.  The first pass reads the uint8 grid and seeds 0 / cap itself.
//   boundary    forward: one dense pass over logits, labels and both transforms, one fp64 partial and one count per workgroup,
//               then one workgroup adds them in a fixed order (frame by frame, lanes by a fixed butterfly) and writes n_G and the
//               loss: the same bits on every call, in both modes of muvo_set_deterministic.  backward: one dense elementwise pass.
//   cd counts   one pass over both grids and both transforms: integer counts are combined per wave and per workgroup before the
//               64-bit atomics (order-free), the fp64 sums leave as per-workgroup partials that one wave adds in a fixed order.
// Plain C++ only; every store is a vector store.
#include "voxel_grid.h"

#define EDT_COLS 64
#define EDT_ROWS 32                        // output rows of a workgroup = rows of one staged chunk
#define EDT_PER 8                          // output rows per thread: 4 waves x 8
#define EDT_LD 65                          // row stride of the tile in words: odd, so both copy directions spread over the banks
#define EDT_MAXDIM 46340                   // 46340^2 < 2^31 <= 46341^2

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool edt_occupied(unsigned v) { return v - 1u < 254u; }      // 1..254; 0 is free, 255 unknown

// One min-plus pass.  grid = (column tiles, row tiles).  ZPASS: src is the uint8 grid, inner == 1.  Values are unsigned: an
// offset^2 < 2^31 plus a value <= capi < 2^31 stays below 2^32.  `fill` is written where the result reaches capi (capi itself
// but for the last pass of a call whose cap exceeds X^2 + Y^2 + Z^2).
template <bool ZPASS>
__global__ void __launch_bounds__(256)
edt_pass_kernel(const void* __restrict__ src, int32_t* __restrict__ dst, long cols, int N, long inner, int radius, uint32_t capi, uint32_t fill) {
  __shared__ uint32_t tile[EDT_ROWS * EDT_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long c0 = (long)blockIdx.x * EDT_COLS;
  const int n0 = (int)blockIdx.y * EDT_ROWS;
  // the element (row, col) of the tile a thread copies in step `it` of 8: ZPASS (tid & 31, (tid >> 5) + 8 it), else (w + 4 it, lane)
  long base = -1;                                        // !ZPASS: where this thread's column starts
  if (!ZPASS && c0 + lane < cols) {
    const long c = c0 + lane, q = c / inner;
    base = q * N * inner + (c - q * inner);
  }
  const int jlo = n0 - radius > 0 ? n0 - radius : 0;
  const int jhi = n0 + EDT_ROWS + radius < N ? n0 + EDT_ROWS + radius : N;
  const int i0 = n0 + w * EDT_PER;
  uint32_t m[EDT_PER];
#pragma unroll
  for (int k = 0; k < EDT_PER; ++k) m[k] = capi;
  for (int j0 = jlo; j0 < jhi; j0 += EDT_ROWS) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int row = ZPASS ? (tid & 31) : w + 4 * it, col = ZPASS ? (tid >> 5) + 8 * it : lane;
      const int n = j0 + row;
      uint32_t v = capi;
      if (ZPASS) {
        if (n < jhi && c0 + col < cols) v = edt_occupied(((const uint8_t*)src)[(size_t)(c0 + col) * N + n]) ? 0u : capi;
      } else {
        if (n < jhi && base >= 0) v = (uint32_t)((const int32_t*)src)[(size_t)base + (size_t)n * inner];
      }
      tile[row * EDT_LD + col] = v;
    }
    __syncthreads();
    const int rows = jhi - j0 < EDT_ROWS ? jhi - j0 : EDT_ROWS;
    for (int jj = 0; jj < rows; ++jj) {
      const uint32_t d = tile[jj * EDT_LD + lane];
      const int b = i0 - (j0 + jj);
#pragma unroll
      for (int k = 0; k < EDT_PER; ++k) {
        const int o = b + k;
        const uint32_t v = (uint32_t)(o * o) + d;
        m[k] = v < m[k] ? v : m[k];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EDT_PER; ++k) tile[(w * EDT_PER + k) * EDT_LD + lane] = m[k] >= capi ? fill : m[k];
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int row = ZPASS ? (tid & 31) : w + 4 * it, col = ZPASS ? (tid >> 5) + 8 * it : lane;
    const int n = n0 + row;
    if (n >= N) continue;
    if (ZPASS) {
      if (c0 + col < cols) dst[(size_t)(c0 + col) * N + n] = (int32_t)tile[row * EDT_LD + col];
    } else {
      if (base >= 0) dst[(size_t)base + (size_t)n * inner] = (int32_t)tile[row * EDT_LD + col];
    }
  }
}

// ---- the dense passes: 4 consecutive voxels per lane, as the sibling units ---------------------------------------------------------
#define BD_THREADS 256
#define BD_VOX (BD_THREADS * 4)

__device__ __forceinline__ void edt_ld4(const int32_t* __restrict__ p, long h0, long V, bool vec, int e[4]) {
  if (vec) {
    const i32x4 u = *(const i32x4*)(p + h0);
    e[0] = u.x; e[1] = u.y; e[2] = u.z; e[3] = u.w;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) e[k] = h0 + k < V ? p[h0 + k] : 0;
}

// sqrt(edt2) / T in fp32, in [0, 1]
__device__ __forceinline__ float bd_dist(int e, float T) { return sqrtf((float)e) / T; }

// One term per voxel: q = s_0 = e_0 / sum, p = 1 - q; free known cell: p dG, occupied label cell: q dP (q = 1 - p), 255: nothing.
// part[f NB + block] = the workgroup's fp64 sum (lanes by a fixed butterfly, the four waves in order), cnt[...] = its label cells.
__global__ void __launch_bounds__(BD_THREADS)
boundary_fwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, const int32_t* __restrict__ eg, const int32_t* __restrict__ ep, int C,
                    long V, int vec, float T, double* __restrict__ part, int32_t* __restrict__ cnt) {
  __shared__ double red[4];
  __shared__ int redn[4];
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * BD_THREADS + threadIdx.x) * 4;
  double acc = 0.0;
  int ng = 0;
  if (h0 < V) {
    const bool v4 = vec && h0 + 3 < V;
    const VgSoftmax st = vg_softmax_stats(logits + (size_t)f * C * V, C, V, h0, v4);
    unsigned l[4];
    int g4[4], p4[4];
    vg_ld4(labels + (size_t)f * V, h0, V, v4, 255u, l);
    edt_ld4(eg + (size_t)f * V, h0, V, v4, g4);
    edt_ld4(ep + (size_t)f * V, h0, V, v4, p4);
    const float q[4] = {st.e0.x / st.sum.x, st.e0.y / st.sum.y, st.e0.z / st.sum.z, st.e0.w / st.sum.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool g = edt_occupied(l[k]);
      float t = 0.f;
      if (g) t = q[k] * bd_dist(p4[k], T);
      else if (l[k] != 255u) t = (1.f - q[k]) * bd_dist(g4[k], T);
      acc += (double)t;
      ng += g ? 1 : 0;
    }
  }
  acc = wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ng += __shfl_xor(ng, o, 64);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = acc; redn[threadIdx.x >> 6] = ng; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(size_t)f * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    cnt[(size_t)f * gridDim.x + blockIdx.x] = redn[0] + redn[1] + redn[2] + redn[3];
  }
}

// One workgroup of 256.  Wave w takes the frames w, w + 4, ...: lane l adds the partials l, l + 64, ... of a frame in order, the
// lanes are added by a fixed butterfly, L_f = sum / n_G joins the wave's total where n_G > 0; the four totals are added in their
// order.  n_g[f] = n_G, n_g[F] = the number of frames that counted, loss[0] = weight x mean L_f (0 without such a frame).
__global__ void __launch_bounds__(256)
boundary_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ cnt, long NB, int F, float weight, int32_t* __restrict__ n_g,
                       float* __restrict__ loss) {
  __shared__ double red[4];
  __shared__ int redc[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double total = 0.0;
  int frames = 0;
  for (int f = w; f < F; f += 4) {
    double s = 0.0;
    long long n = 0;
    for (long p = lane; p < NB; p += 64) {
      s += part[(size_t)f * NB + p];
      n += cnt[(size_t)f * NB + p];
    }
    s = wave_sum_d(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (n > 0) {
      total += s / (double)n;
      ++frames;
    }
    if (lane == 0) n_g[f] = (int32_t)n;
  }
  if (lane == 0) { red[w] = total; redc[w] = frames; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = redc[0] + redc[1] + redc[2] + redc[3];
    n_g[F] = c;
    loss[0] = c > 0 ? (float)((double)weight * (((red[0] + red[1]) + red[2]) + red[3]) / (double)c) : 0.f;
  }
}

// dlogits[c] = a dp/dz_c with a = gout weight / (frames n_G) x (dG on a free known cell, -dP on an occupied label cell, 0 on 255),
// dp/dz_0 = -q p, dp/dz_c = q s_c.  Every element is written; a frame with n_G = 0 gets zeros.
__global__ void __launch_bounds__(BD_THREADS)
boundary_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, const int32_t* __restrict__ eg, const int32_t* __restrict__ ep,
                    const int32_t* __restrict__ n_g, int C, long V, int vec, float T, float weight, const float* __restrict__ gout, float* __restrict__ dlogits) {
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * BD_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  const int n = n_g[f], frames = n_g[gridDim.y];
  const float sc = n > 0 && frames > 0 ? (float)((double)gout[0] * (double)weight / ((double)frames * (double)n)) : 0.f;
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  float* __restrict__ df = dlogits + (size_t)f * C * V;
  const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
  unsigned l[4];
  int g4[4], p4[4];
  vg_ld4(labels + (size_t)f * V, h0, V, v4, 255u, l);
  edt_ld4(eg + (size_t)f * V, h0, V, v4, g4);
  edt_ld4(ep + (size_t)f * V, h0, V, v4, p4);
  float a[4], q[4];
  q[0] = st.e0.x / st.sum.x; q[1] = st.e0.y / st.sum.y; q[2] = st.e0.z / st.sum.z; q[3] = st.e0.w / st.sum.w;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float wv = 0.f;
    if (edt_occupied(l[k])) wv = -bd_dist(p4[k], T);
    else if (l[k] != 255u) wv = bd_dist(g4[k], T);
    a[k] = sc * wv * q[k];                                // every derivative carries the factor q = s_0
  }
  vg_st4(df, h0, V, v4, f32x4{-(a[0] * (1.f - q[0])), -(a[1] * (1.f - q[1])), -(a[2] * (1.f - q[2])), -(a[3] * (1.f - q[3]))});
  for (int c = 1; c < C; ++c) {
    const f32x4 s = vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), st.m, st.sum);
    vg_st4(df + (size_t)c * V, h0, V, v4, f32x4{a[0] * s.x, a[1] * s.y, a[2] * s.z, a[3] * s.w});
  }
}

// ---- Chamfer / F-score counts.  grid = (blocks of CD_ITER x 1024 voxels, frames).  counts: [0] frames, [1] skipped frames, [2] n_P,
// [3] n_G, [4..6] hits_P, [7..9] hits_G.  A frame one of whose sets is empty - its transform at cell 0 reaches `empty` = X^2 + Y^2
// + Z^2, beyond every real distance - adds 1 to [1] and nothing else.  part[(f NB + block) 2 + k]: the fp64 partial of sum_PG / sum_GP.
#define CD_ITER 8
__global__ void __launch_bounds__(BD_THREADS)
cd_counts_kernel(const uint8_t* __restrict__ label, const uint8_t* __restrict__ pred, const int32_t* __restrict__ eg, const int32_t* __restrict__ ep, long V,
                 int vec, int k0, int k1, int k2, int empty, unsigned long long* __restrict__ counts, double* __restrict__ part) {
  __shared__ unsigned cnt[8];
  __shared__ double red[2][4];
  const long f = blockIdx.y;
  const size_t slot = ((size_t)f * gridDim.x + blockIdx.x) * 2;
  if (eg[(size_t)f * V] >= empty || ep[(size_t)f * V] >= empty) {         // the same for every thread of the frame
    if (threadIdx.x < 2) part[slot + threadIdx.x] = 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counts[1], 1ull);
    return;
  }
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
  __syncthreads();
  unsigned c[8] = {0, 0, 0, 0, 0, 0, 0, 0};              // n_P, n_G, hits_P[3], hits_G[3]
  double spg = 0.0, sgp = 0.0;
  for (int it = 0; it < CD_ITER; ++it) {
    const long h0 = (((long)blockIdx.x * CD_ITER + it) * BD_THREADS + threadIdx.x) * 4;
    if (h0 >= V) break;
    const bool v4 = vec && h0 + 3 < V;
    unsigned lg[4], lp[4];
    int g4[4], p4[4];
    vg_ld4(label + (size_t)f * V, h0, V, v4, 0u, lg);
    vg_ld4(pred + (size_t)f * V, h0, V, v4, 0u, lp);
    edt_ld4(eg + (size_t)f * V, h0, V, v4, g4);
    edt_ld4(ep + (size_t)f * V, h0, V, v4, p4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (edt_occupied(lp[k])) {
        const int d = g4[k];
        c[0] += 1; c[2] += d <= k0; c[3] += d <= k1; c[4] += d <= k2;
        spg += sqrt((double)d);
      }
      if (edt_occupied(lg[k])) {
        const int d = p4[k];
        c[1] += 1; c[5] += d <= k0; c[6] += d <= k1; c[7] += d <= k2;
        sgp += sqrt((double)d);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
  }
  spg = wave_sum_d(spg);
  sgp = wave_sum_d(sgp);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (c[k]) atomicAdd(&cnt[k], c[k]);
    red[0][threadIdx.x >> 6] = spg;
    red[1][threadIdx.x >> 6] = sgp;
  }
  __syncthreads();
  if (threadIdx.x < 8 && cnt[threadIdx.x]) atomicAdd(&counts[2 + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  if (threadIdx.x < 2) part[slot + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&counts[0], 1ull);
}

// one wave: lane l adds the partials l, l + 64, ... in order, the lanes are added by a fixed butterfly, sums[k] += total
__global__ void __launch_bounds__(64) cd_sum_kernel(const double* __restrict__ part, long P, double* __restrict__ sums) {
  for (int k = 0; k < 2; ++k) {
    double s = 0.0;
    for (long p = threadIdx.x; p < P; p += 64) s += part[p * 2 + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) sums[k] += s;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

static inline int64_t edt_up16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// the sizes the transform takes: 1..65535 frames, every axis >= 1, X^2 + Y^2 + Z^2 < 2^31, fewer than 2^36 cells in all
static inline bool edt_sizes_ok(int64_t F, int X, int Y, int Z) {
  if (!(vg_frames_ok(F) && X >= 1 && Y >= 1 && Z >= 1 && X <= EDT_MAXDIM && Y <= EDT_MAXDIM && Z <= EDT_MAXDIM)) return false;
  if ((int64_t)X * X + (int64_t)Y * Y + (int64_t)Z * Z >= (1ll << 31)) return false;
  return F * ((int64_t)X * Y * Z) < (1ll << 36);
}

static inline int edt_isqrt(int64_t n) {                 // floor(sqrt(n)), n >= 0
  int64_t r = (int64_t)sqrt((double)n);
  while (r * r > n) --r;
  while ((r + 1) * (r + 1) <= n) ++r;
  return (int)r;
}

static void edt_pass(bool zpass, const void* src, int32_t* dst, int64_t cols, int N, int64_t inner, int radius, uint32_t capi, uint32_t fill, hipStream_t st) {
  const dim3 grd((unsigned)((cols + EDT_COLS - 1) / EDT_COLS), (unsigned)((N + EDT_ROWS - 1) / EDT_ROWS));
  const int r = radius < N - 1 ? radius : N - 1;
  if (zpass) hipLaunchKernelGGL(edt_pass_kernel<true>, grd, dim3(256), 0, st, src, dst, (long)cols, N, (long)inner, r, capi, fill);
  else hipLaunchKernelGGL(edt_pass_kernel<false>, grd, dim3(256), 0, st, src, dst, (long)cols, N, (long)inner, r, capi, fill);
}

static int bd_check(const char* who, int64_t F, int C, int X, int Y, int Z, int truncate) {
  if (int rc = vg_check_frames(who, F)) return rc;
  if (int rc = vg_check_classes(who, C)) return rc;
  if (int rc = vg_check_grid(who, X, Y, Z)) return rc;
  MUVO_CHECK_ARG(truncate >= 1 && truncate <= EDT_MAXDIM, "%s: truncation of %d cells outside 1..%d", who, truncate, EDT_MAXDIM);
  return MUVO_OK;
}

static inline int bd_vec(int64_t V, const void* a, const void* b, const void* c, const void* d, const void* e) {
  return (V % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0 && ((uintptr_t)e & 3) == 0) ? 1 : 0;
}

extern "C" {

int64_t muvo_voxel_edt_ws_bytes(int64_t F, int X, int Y, int Z) { return edt_sizes_ok(F, X, Y, Z) ? F * ((int64_t)X * Y * Z) * 4 : -1; }

int muvo_voxel_edt(const uint8_t* grid, int64_t F, int X, int Y, int Z, int32_t cap, void* ws, int64_t ws_bytes, int32_t* out, void* stream) {
  MUVO_CHECK_ARG(edt_sizes_ok(F, X, Y, Z), "voxel_edt: %lld frames of %d x %d x %d (1..65535 frames, every axis >= 1, X^2 + Y^2 + Z^2 < 2^31, fewer than 2^36 cells)",
                 (long long)F, X, Y, Z);
  MUVO_CHECK_ARG(cap >= 1, "voxel_edt: cap %d below 1", (int)cap);
  MUVO_CHECK_ARG(grid && out && ws, "voxel_edt: null pointer");
  const int64_t need = muvo_voxel_edt_ws_bytes(F, X, Y, Z);
  MUVO_CHECK_ARG((((uintptr_t)ws | (uintptr_t)out) & 3) == 0 && ws_bytes >= need, "voxel_edt: workspace of %lld bytes, %lld needed (4-byte aligned, as the output)",
                 (long long)ws_bytes, (long long)need);
  const int64_t full = (int64_t)X * X + (int64_t)Y * Y + (int64_t)Z * Z;
  const uint32_t capi = (uint32_t)(cap < full ? cap : full);
  const int radius = edt_isqrt((int64_t)capi - 1);
  edt_pass(true, grid, out, F * X * Y, Z, 1, radius, capi, capi, ST);
  edt_pass(false, out, (int32_t*)ws, F * X * Z, Y, Z, radius, capi, capi, ST);
  edt_pass(false, ws, out, F * Y * Z, X, (int64_t)Y * Z, radius, capi, (uint32_t)cap, ST);
  MUVO_CHECK_LAUNCH("voxel_edt");
  return MUVO_OK;
}

int64_t muvo_voxel_boundary_ws_bytes(int64_t F, int64_t V) {
  if (!(vg_frames_ok(F) && vg_voxels_ok(V))) return -1;
  const int64_t nb = (V + BD_VOX - 1) / BD_VOX;
  return edt_up16(F * nb * 8) + edt_up16(F * nb * 4);
}

int muvo_voxel_boundary_forward(const float* logits, const uint8_t* labels, const int32_t* edt_label, const int32_t* edt_pred, int64_t F, int C, int X, int Y, int Z,
                                int truncate, float weight, void* ws, int64_t ws_bytes, int32_t* n_g, float* loss, void* stream) {
  if (int rc = bd_check("voxel_boundary_forward", F, C, X, Y, Z, truncate)) return rc;
  MUVO_CHECK_ARG(logits && labels && edt_label && edt_pred && n_g && loss, "voxel_boundary_forward: null pointer");
  const int64_t V = (int64_t)X * Y * Z, need = muvo_voxel_boundary_ws_bytes(F, V);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 15) == 0 && ws_bytes >= need, "voxel_boundary_forward: workspace of %lld bytes, %lld needed (16-byte aligned)",
                 (long long)ws_bytes, (long long)need);
  MUVO_CHECK_ARG((((uintptr_t)edt_label | (uintptr_t)edt_pred | (uintptr_t)n_g) & 3) == 0, "voxel_boundary_forward: a 32-bit buffer is not 4-byte aligned");
  const int64_t nb = (V + BD_VOX - 1) / BD_VOX;
  double* part = (double*)ws;
  int32_t* cnt = (int32_t*)((char*)ws + edt_up16(F * nb * 8));
  hipLaunchKernelGGL(boundary_fwd_kernel, dim3((unsigned)nb, (unsigned)F), dim3(BD_THREADS), 0, ST, logits, labels, edt_label, edt_pred, C, (long)V,
                     bd_vec(V, logits, edt_label, edt_pred, logits, labels), (float)truncate, part, cnt);
  hipLaunchKernelGGL(boundary_finish_kernel, dim3(1), dim3(256), 0, ST, (const double*)part, (const int32_t*)cnt, (long)nb, (int)F, weight, n_g, loss);
  MUVO_CHECK_LAUNCH("voxel_boundary_forward");
  return MUVO_OK;
}

int muvo_voxel_boundary_backward(const float* logits, const uint8_t* labels, const int32_t* edt_label, const int32_t* edt_pred, const int32_t* n_g, int64_t F, int C,
                                 int X, int Y, int Z, int truncate, float weight, const float* gout, float* dlogits, void* stream) {
  if (int rc = bd_check("voxel_boundary_backward", F, C, X, Y, Z, truncate)) return rc;
  MUVO_CHECK_ARG(logits && labels && edt_label && edt_pred && n_g && gout && dlogits, "voxel_boundary_backward: null pointer");
  MUVO_CHECK_ARG((((uintptr_t)edt_label | (uintptr_t)edt_pred | (uintptr_t)n_g) & 3) == 0, "voxel_boundary_backward: a 32-bit buffer is not 4-byte aligned");
  const int64_t V = (int64_t)X * Y * Z;
  hipLaunchKernelGGL(boundary_bwd_kernel, dim3((unsigned)((V + BD_VOX - 1) / BD_VOX), (unsigned)F), dim3(BD_THREADS), 0, ST, logits, labels, edt_label, edt_pred,
                     n_g, C, (long)V, bd_vec(V, logits, edt_label, edt_pred, dlogits, labels), (float)truncate, weight, gout, dlogits);
  MUVO_CHECK_LAUNCH("voxel_boundary_backward");
  return MUVO_OK;
}

int64_t muvo_voxel_cd_ws_bytes(int64_t F, int64_t V) {
  if (!(vg_frames_ok(F) && vg_voxels_ok(V))) return -1;
  return F * ((V + (int64_t)CD_ITER * BD_VOX - 1) / ((int64_t)CD_ITER * BD_VOX)) * 16;
}

int muvo_voxel_cd_counts(const uint8_t* label, const uint8_t* pred, const int32_t* edt_label, const int32_t* edt_pred, int64_t F, int X, int Y, int Z,
                         const int32_t* thresholds2, uint64_t* counts, double* sums, void* ws, int64_t ws_bytes, void* stream) {
  if (int rc = vg_check_frames("voxel_cd_counts", F)) return rc;
  if (int rc = vg_check_grid("voxel_cd_counts", X, Y, Z)) return rc;
  MUVO_CHECK_ARG(label && pred && edt_label && edt_pred && thresholds2 && counts && sums, "voxel_cd_counts: null pointer");
  MUVO_CHECK_ARG(thresholds2[0] >= 0 && thresholds2[1] >= 0 && thresholds2[2] >= 0, "voxel_cd_counts: a negative squared threshold");
  const int64_t V = (int64_t)X * Y * Z, need = muvo_voxel_cd_ws_bytes(F, V);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need, "voxel_cd_counts: workspace of %lld bytes, %lld needed (8-byte aligned)",
                 (long long)ws_bytes, (long long)need);
  MUVO_CHECK_ARG((((uintptr_t)counts | (uintptr_t)sums) & 7) == 0 && (((uintptr_t)edt_label | (uintptr_t)edt_pred) & 3) == 0,
                 "voxel_cd_counts: the accumulators are not 8-byte aligned or a transform is not 4-byte aligned");
  const int64_t nb = need / 16 / F;
  const int vec = (V % 4 == 0 && (((uintptr_t)edt_label | (uintptr_t)edt_pred) & 15) == 0 && (((uintptr_t)label | (uintptr_t)pred) & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(cd_counts_kernel, dim3((unsigned)nb, (unsigned)F), dim3(BD_THREADS), 0, ST, label, pred, edt_label, edt_pred, (long)V, vec, (int)thresholds2[0],
                     (int)thresholds2[1], (int)thresholds2[2], X * X + Y * Y + Z * Z, (unsigned long long*)counts, (double*)ws);
  hipLaunchKernelGGL(cd_sum_kernel, dim3(1), dim3(64), 0, ST, (const double*)ws, (long)(nb * F), sums);
  MUVO_CHECK_LAUNCH("voxel_cd_counts");
  return MUVO_OK;
}

}  // extern "C"
