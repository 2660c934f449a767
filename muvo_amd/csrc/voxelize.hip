// Voxel labels from raw sensor data on the device: the reference's offline step data/generate_voxels.py::voxelize_one ->
// data_preprocessing.py::merge_pcd + voxel_filter (depth+semantic camera image and semantic lidar sweep -> ego frame -> ego-box
// mask -> voxel bins; every occupied voxel gets the tag of the point nearest to its lower corner, or "road line" if any of its
// points is one).  A scatter / select / compact problem, HBM- and atomic-bound.  The arithmetic is the reference's float64
// arithmetic operation by operation (the unit is built with -ffp-contract=off); the selection uses integer atomics only, so the
// result does not depend on the arrival order: 64-bit atomicMin on the bit pattern of the distance, then 32-bit atomicMin on
// the global point index among the points at that distance (camera pixels row-major first, lidar points after them).
#include "common.h"

#define VOX_CHUNK 2048          // slots per workgroup in the label / rows kernels: 8 rounds of 256
#define VOX_EMPTY 0xffffu       // label of a slot without a point
#define VOX_ROADLINE 6          // LABEL_CLASS == 'roadlines'

struct VoxArgs {
  muvo_voxelize_geom g;
  long HW, Pmax, N, Np;         // pixels per frame, padded lidar points per frame, slots per frame, slots rounded up to 16
  int nblk;                     // cdiv(N, VOX_CHUNK)
};

// np.divmod(b, res) for b >= 0, res > 0 (numpy's npy_divmod: fmod-based, the quotient snapped to the nearest integer).  The
// point passed b < size * res, but the snap can still give `size` for b within an ulp of the upper face: clamped, the grid has
// no such voxel.
__device__ __forceinline__ unsigned vox_divmod(double b, double res, int D, double& m) {
  m = fmod(b, res);
  const double d = (b - m) / res;
  double q = floor(d);
  if (d - q > 0.5) q += 1.0;
  const unsigned u = (unsigned)q;
  return u < (unsigned)D ? u : (unsigned)(D - 1);
}

// Steps 6-8 of the chain for one ego-frame point: ego box, grid test, bin and squared distance to the voxel's lower corner.
__device__ __forceinline__ bool vox_bin(const muvo_voxelize_geom& g, double ex, double ey, double ez, unsigned& h, unsigned long long& key) {
  if (g.mask_ego && g.ego_lo[0] < ex && ex < g.ego_hi[0] && g.ego_lo[1] < ey && ey < g.ego_hi[1] && g.ego_lo[2] < ez && ez < g.ego_hi[2])
    return false;
  const double b0 = ex + g.off[0], b1 = ey + g.off[1], b2 = ez + g.off[2];
  if (!(0.0 <= b0 && b0 < g.hi[0] && 0.0 <= b1 && b1 < g.hi[1] && 0.0 <= b2 && b2 < g.hi[2])) return false;   // NaN: out
  double m0, m1, m2;
  const unsigned q0 = vox_divmod(b0, g.res, g.Dx, m0), q1 = vox_divmod(b1, g.res, g.Dy, m1), q2 = vox_divmod(b2, g.res, g.Dz, m2);
  h = q0 + (q1 + q2 * (unsigned)g.Dy) * (unsigned)g.Dx;
  key = (unsigned long long)__double_as_longlong((m0 * m0 + m1 * m1) + m2 * m2);     // >= 0: ordered like its bits
  return true;
}

// Point `i` of frame `f` (camera pixels 0 .. HW-1, then lidar points): slot, distance key, raw tag.  false: the point is dropped.
__device__ __forceinline__ bool vox_point(const VoxArgs& a, const uint32_t* __restrict__ img, const float* __restrict__ pts,
                                          const uint8_t* __restrict__ tags, long f, long i, unsigned& h, unsigned long long& key,
                                          unsigned& tag) {
  const muvo_voxelize_geom& g = a.g;
  if (i < a.HW) {
    const uint32_t px = img[f * a.HW + i];                     // R, G, B = 24-bit depth code, A = semantic tag
    const uint32_t code = ((px & 0xffu) << 16) | (px & 0xff00u) | ((px >> 16) & 0xffu);
    tag = px >> 24;
    const double depth = 1000.0 * ((double)code / 16777215.0);
    if (!(depth < 1000.0)) return false;
    // depth2pcd: pinhole unprojection, range filter in the camera frame
    const double xx = (double)(i % g.W), yy = (double)(i / g.W);
    const double x = ((xx - g.cx) * depth) / g.f, y = ((yy - g.cy) * depth) / g.f;
    if (!(sqrt((x * x + y * y) + depth * depth) < g.max_range)) return false;
    // convert_coor_img: the float32 camera matrix, widened
    return vox_bin(g, depth + g.cam[0], -x + g.cam[1], -y + g.cam[2], h, key);
  }
  const long j = f * a.Pmax + (i - a.HW);
  tag = tags[j];
  // convert_coor_lidar: in-place float32 update, y mirrored
  const float p0 = (float)((double)pts[j * 3] + g.lidar[0]), p1 = -(float)((double)pts[j * 3 + 1] + g.lidar[1]),
              p2 = (float)((double)pts[j * 3 + 2] + g.lidar[2]);
  return vox_bin(g, (double)p0, (double)p1, (double)p2, h, key);
}

// pass 1: best[slot] = smallest distance key of the slot's points, road[slot] = 1 if one of them is a road line.
// Neighbouring pixels of an image row often share a voxel (8 points per occupied voxel on average): a segmented min-scan over
// runs of equal slots among the lanes of the wave leaves one atomic per run (the last lane of the run carries the run's
// minimum).  Measured against one atomic per point: this pass 3.3x, the whole call 1.4-1.5x faster
// (profiles/r05a_voxelize_times.txt).
__global__ void __launch_bounds__(256)
voxelize_min_kernel(VoxArgs a, const uint32_t* __restrict__ img, const float* __restrict__ pts, const uint8_t* __restrict__ tags,
                    const int32_t* __restrict__ num_points, unsigned long long* __restrict__ best, uint8_t* __restrict__ road) {
  const long f = blockIdx.y;
  const long total = a.HW + (num_points ? min(max((long)num_points[f], 0L), a.Pmax) : a.Pmax);
  unsigned long long* bf = best + f * a.Np;
  uint8_t* rf = road + f * a.Np;
  for (long base = blockIdx.x * 256L; base < total; base += (long)gridDim.x * 256) {   // uniform trip count per wave
    const long i = base + threadIdx.x;
    unsigned h = 0xffffffffu, tag = 0;
    unsigned long long key = ~0ull;
    const bool ok = i < total && vox_point(a, img, pts, tags, f, i, h, key, tag);
    if (!ok) h = 0xffffffffu;
    if (ok && tag == VOX_ROADLINE) rf[h] = 1;            // every writer writes the same value
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned hh = __shfl_up(h, o, 64);
      const unsigned long long kk = __shfl_up(key, o, 64);
      if (lane >= o && hh == h && kk < key) key = kk;
    }
    const unsigned hn = __shfl_down(h, 1, 64);
    if (ok && (lane == 63 || hn != h)) atomicMin(bf + h, key);
  }
}

// pass 2: among the points at the smallest distance of a slot the lowest global index wins
__global__ void __launch_bounds__(256)
voxelize_winner_kernel(VoxArgs a, const uint32_t* __restrict__ img, const float* __restrict__ pts, const uint8_t* __restrict__ tags,
                       const int32_t* __restrict__ num_points, const unsigned long long* __restrict__ best,
                       unsigned int* __restrict__ winner) {
  const long f = blockIdx.y;
  const long total = a.HW + (num_points ? min(max((long)num_points[f], 0L), a.Pmax) : a.Pmax);
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    unsigned h, tag;
    unsigned long long key;
    if (!vox_point(a, img, pts, tags, f, i, h, key, tag)) continue;
    if (key == best[f * a.Np + h]) atomicMin(winner + f * a.Np + h, (unsigned int)i);
  }
}

// pass 3: lab[slot] = VOX_EMPTY, 6 for a slot with a road line, else the winner's raw tag; occupied slots per chunk of
// VOX_CHUNK slots -> cnt[f][chunk]
__global__ void __launch_bounds__(256)
voxelize_label_kernel(VoxArgs a, const uint8_t* __restrict__ img, const uint8_t* __restrict__ tags, const unsigned int* __restrict__ winner,
                      const uint8_t* __restrict__ road, uint16_t* __restrict__ lab, int32_t* __restrict__ cnt) {
  __shared__ int wsum[4];
  const long f = blockIdx.y;
  int n = 0;
#pragma unroll
  for (int k = 0; k < VOX_CHUNK / 256; ++k) {
    const long h = (long)blockIdx.x * VOX_CHUNK + k * 256 + threadIdx.x;
    bool occ = false;
    if (h < a.N) {
      const unsigned int w = winner[f * a.Np + h];
      unsigned t = VOX_EMPTY;
      if (w != 0xffffffffu) {
        occ = true;
        t = road[f * a.Np + h] ? VOX_ROADLINE : (w < a.HW ? img[(f * a.HW + w) * 4 + 3] : tags[f * a.Pmax + (w - a.HW)]);
      }
      lab[f * a.Np + h] = (uint16_t)t;
    }
    n += __popcll(__ballot(occ));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) cnt[f * a.nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 4: one workgroup per frame: chunk counts -> exclusive offsets (in place), total -> counts[f]
__global__ void __launch_bounds__(256)
voxelize_scan_kernel(int nblk, int32_t* __restrict__ cnt, int32_t* __restrict__ counts) {
  __shared__ int part[256];
  int32_t* c = cnt + (long)blockIdx.x * nblk;
  const int per = (nblk + 255) / 256, lo = threadIdx.x * per, hi = min(lo + per, nblk);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += c[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                    // inclusive scan of the 256 partial sums
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int i = lo; i < hi; ++i) {
    const int v = c[i];
    c[i] = run;
    run += v;
  }
  if (threadIdx.x == 255) counts[blockIdx.x] = part[255];
}

// pass 5: ordered compaction: the occupied slots of a chunk, in slot order, to rows[f][off[chunk] ...] as x, y, z, tag
__global__ void __launch_bounds__(256)
voxelize_rows_kernel(VoxArgs a, const uint16_t* __restrict__ lab, const int32_t* __restrict__ off, long long* __restrict__ rows, long cap) {
  __shared__ int wcnt[VOX_CHUNK / 64];
  const long f = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned t[VOX_CHUNK / 256];
  unsigned long long m[VOX_CHUNK / 256];
#pragma unroll
  for (int k = 0; k < VOX_CHUNK / 256; ++k) {
    const long h = (long)blockIdx.x * VOX_CHUNK + k * 256 + threadIdx.x;
    t[k] = h < a.N ? lab[f * a.Np + h] : VOX_EMPTY;
    m[k] = __ballot(t[k] != VOX_EMPTY);
    if (lane == 0) wcnt[k * 4 + wave] = __popcll(m[k]);
  }
  __syncthreads();
  int pos = off[f * a.nblk + blockIdx.x];
#pragma unroll
  for (int k = 0; k < VOX_CHUNK / 256; ++k) {
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wcnt[k * 4 + w];
      if (w < wave) before += c;
      all += c;
    }
    if (t[k] != VOX_EMPTY) {
      const long r = pos + before + __popcll(m[k] & ((1ull << lane) - 1ull));
      if (r < cap) {                                     // the caller's cap is min(points, slots): the bound of its buffer
        const unsigned h = (unsigned)(blockIdx.x * (long)VOX_CHUNK + k * 256 + threadIdx.x);
        const unsigned Dx = (unsigned)a.g.Dx, Dy = (unsigned)a.g.Dy;
        long long* o = rows + (f * cap + r) * 4;
        o[0] = h % Dx; o[1] = (h / Dx) % Dy; o[2] = h / (Dx * Dy); o[3] = t[k];
      }
    }
    pos += all;
  }
}

// dense[f][x][y][z] = remap[tag == 255 ? 0 : tag] (0 for an empty slot).  lab is in slot order (x fastest), the grid is z
// fastest: one workgroup moves a 64 (x) x 64 (z) tile of one y through LDS, so that loads run along x and stores along z.
__global__ void __launch_bounds__(256)
voxelize_dense_kernel(VoxArgs a, const uint16_t* __restrict__ lab, const uint8_t* __restrict__ remap, uint8_t* __restrict__ dense) {
  __shared__ uint8_t tile[64][65];
  const int Dx = a.g.Dx, Dy = a.g.Dy, Dz = a.g.Dz;
  const int xt = (Dx + 63) / 64;
  const int x0 = (blockIdx.x % xt) * 64, z0 = (blockIdx.x / xt) * 64, y = blockIdx.y;
  const long f = blockIdx.z;
  const int c = threadIdx.x & 63, r4 = threadIdx.x >> 6;
  for (int r = r4; r < 64; r += 4) {                     // r: z within the tile, c: x within the tile
    const int x = x0 + c, z = z0 + r;
    uint8_t v = 0;
    if (x < Dx && z < Dz) {
      const unsigned t = lab[f * a.Np + ((long)z * Dy + y) * Dx + x];
      if (t != VOX_EMPTY) v = remap[t == 255 ? 0 : t];
    }
    tile[c][r] = v;
  }
  __syncthreads();
  for (int r = r4; r < 64; r += 4) {                     // r: x within the tile, c: z within the tile
    const int x = x0 + r, z = z0 + c;
    if (x < Dx && z < Dz) dense[((f * Dx + x) * Dy + y) * Dz + z] = tile[r][c];
  }
}

#define ST ((hipStream_t)stream)
extern "C" {

int64_t muvo_voxelize_scratch_bytes(int F, int Dx, int Dy, int Dz) {
  if (F <= 0 || Dx <= 0 || Dy <= 0 || Dz <= 0 || (int64_t)Dx * Dy * Dz >= (1ll << 31)) return -1;
  const int64_t N = (int64_t)Dx * Dy * Dz, Np = (N + 15) / 16 * 16, nblk = (N + VOX_CHUNK - 1) / VOX_CHUNK;
  return (int64_t)F * (15 * Np + 4 * nblk);
}

int muvo_voxelize_frames(const uint8_t* depth_semantic, const float* points_xyz, const uint8_t* obj_tag, const int32_t* num_points, int F,
                         int64_t Pmax, const muvo_voxelize_geom* geom, const uint8_t* remap, void* scratch, int64_t* rows, int64_t cap,
                         int32_t* counts, uint8_t* dense, void* stream) {
  MUVO_CHECK_ARG(depth_semantic && geom && scratch, "voxelize: null pointer (depth_semantic, geom, scratch)");
  MUVO_CHECK_ARG(rows || dense, "voxelize: null pointer (neither rows nor dense requested)");
  MUVO_CHECK_ARG(Pmax >= 0 && (Pmax == 0 || (points_xyz && obj_tag)), "voxelize: null pointer (points_xyz, obj_tag) or Pmax < 0");
  MUVO_CHECK_ARG(!rows || (counts && cap > 0), "voxelize: rows need counts and cap > 0");
  MUVO_CHECK_ARG(!dense || remap, "voxelize: null pointer (dense needs remap)");
  const muvo_voxelize_geom& g = *geom;
  MUVO_CHECK_ARG(F > 0 && F <= 65535 && g.H > 0 && g.W > 0 && g.Dx > 0 && g.Dy > 0 && g.Dz > 0,
                 "voxelize: bad sizes (F %d in 1..65535, H %d, W %d, grid %d %d %d must be positive)", F, g.H, g.W, g.Dx, g.Dy, g.Dz);
  MUVO_CHECK_ARG(g.Dx <= 65535 && g.Dy <= 65535 && g.Dz <= 65535, "voxelize: grid %d %d %d beyond 65535 per axis (uint16 rows)", g.Dx, g.Dy, g.Dz);
  MUVO_CHECK_ARG((int64_t)g.Dx * g.Dy * g.Dz < (1ll << 31), "voxelize: grid %d %d %d has 2^31 slots or more", g.Dx, g.Dy, g.Dz);
  MUVO_CHECK_ARG((int64_t)g.H * g.W + Pmax < (1ll << 32) - 1, "voxelize: H*W + Pmax = %lld does not fit the 32-bit point index",
                 (long long)((int64_t)g.H * g.W + Pmax));
  MUVO_CHECK_ARG(g.res > 0.0 && g.f > 0.0, "voxelize: resolution %g and focal length %g must be positive", g.res, g.f);
  VoxArgs a;
  a.g = g;
  a.HW = (long)g.H * g.W; a.Pmax = (long)Pmax; a.N = (long)g.Dx * g.Dy * g.Dz; a.Np = (a.N + 15) / 16 * 16;
  a.nblk = (int)((a.N + VOX_CHUNK - 1) / VOX_CHUNK);
  const long FN = (long)F * a.Np;
  unsigned long long* best = (unsigned long long*)scratch;
  unsigned int* winner = (unsigned int*)(best + FN);
  uint16_t* lab = (uint16_t*)(winner + FN);
  uint8_t* road = (uint8_t*)(lab + FN);
  int32_t* cnt = (int32_t*)(road + FN);
  if (hipMemsetAsync(best, 0xff, (size_t)FN * 12, ST) != hipSuccess || hipMemsetAsync(road, 0, (size_t)FN, ST) != hipSuccess) {
    muvo_set_error("voxelize: memset failed");
    return MUVO_ERR_HIP;
  }
  const uint32_t* img = (const uint32_t*)depth_semantic;
  const dim3 pg((unsigned)ew_grid(a.HW + a.Pmax), (unsigned)F);
  hipLaunchKernelGGL(voxelize_min_kernel, pg, dim3(256), 0, ST, a, img, points_xyz, obj_tag, num_points, best, road);
  hipLaunchKernelGGL(voxelize_winner_kernel, pg, dim3(256), 0, ST, a, img, points_xyz, obj_tag, num_points, best, winner);
  hipLaunchKernelGGL(voxelize_label_kernel, dim3((unsigned)a.nblk, (unsigned)F), dim3(256), 0, ST, a, depth_semantic, obj_tag, winner, road, lab, cnt);
  if (rows) {
    hipLaunchKernelGGL(voxelize_scan_kernel, dim3((unsigned)F), dim3(256), 0, ST, a.nblk, cnt, counts);
    hipLaunchKernelGGL(voxelize_rows_kernel, dim3((unsigned)a.nblk, (unsigned)F), dim3(256), 0, ST, a, lab, cnt, (long long*)rows, (long)cap);
  }
  if (dense) {
    const unsigned tiles = (unsigned)(((g.Dx + 63) / 64) * ((g.Dz + 63) / 64));
    hipLaunchKernelGGL(voxelize_dense_kernel, dim3(tiles, (unsigned)g.Dy, (unsigned)F), dim3(256), 0, ST, a, lab, remap, dense);
  }
  MUVO_CHECK_LAUNCH("voxelize");
  return MUVO_OK;
}

}  // extern "C"
