// Frame preparation of the dataset on the device (muvo/data/dataset.py:231-369): a whole batch of F = b*s raw frames, as the
// host read them from the files of a recording, becomes the reference's batch dict in a handful of launches.  Frames are a grid
// dimension of every kernel; nothing loops over frames on the host and nothing syncs with it.  All results are specified bit
// for bit: integer work, or float64 in the reference's order of operations.  HBM-bound streaming kernels.
#include "common.h"
#include "input_dev.h"

// ---- bird's-eye view: bit planes, label = highest set bit, instance mask (dataset.py:253-266, dataset_utils.py:23-59) ------
__global__ void __launch_bounds__(256)
birdview_decode_kernel(const int* __restrict__ bev, int n_classes, long HW, float* __restrict__ planes, long long* __restrict__ label,
                       unsigned char* __restrict__ mask) {
  const long f = blockIdx.y;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const int v = bev[f * HW + p];
    int top = -1;
    for (int c = 0; c < n_classes; ++c) {
      const int bit = (v >> c) & 1;
      planes[(f * n_classes + c) * HW + p] = (float)bit;
      if (bit) top = c;
    }
    // (n-1) - argmax(flipped planes): the highest set plane; all planes zero: argmax = 0, so n-1
    label[f * HW + p] = top < 0 ? n_classes - 1 : top;
    mask[f * HW + p] = (unsigned char)(((v >> 3) | (v >> 4)) & 1);
  }
}

// ---- connected components (scipy.ndimage.label of a (1, H, W) array, default structure = 4-connectivity in the plane) -------
// A forest over the pixels of one frame: parent[p] <= p, a root is the smallest linear index of its set, background = -1.
// Parents only ever decrease (atomicMin), so every chain of parents is strictly decreasing and ends after at most n steps.
#define CC_T 32                      // tile edge: CC_T * CC_T labels (4 KB) of LDS per workgroup
#define CC_N (CC_T * CC_T)

// root of p.  parent values are strictly decreasing along the chain: at most `n` steps (n = number of nodes of the forest)
__device__ __forceinline__ int cc_find(const int* L, int p, int n) {
  for (int it = 0; it < n; ++it) {
    const int q = __hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == p) break;
    p = q;
  }
  return p;
}
// Joins the sets of a and b: the larger root is hung under the smaller one.  A failed attempt means another thread lowered
// the parent of the larger root meanwhile; we continue from that lower value.  Every failed attempt strictly lowers a or b,
// both stay in [0, n): at most 2n attempts.  The final forest has the same sets whatever the order of the attempts.
__device__ __forceinline__ void cc_union(int* L, int a, int b, int n) {
  for (int it = 0; it < 2 * n; ++it) {
    a = cc_find(L, a, n);
    b = cc_find(L, b, n);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

// pass 1: union-find inside a CC_T x CC_T tile in LDS, flattened; written out as frame-linear indices of the tile-local roots
__global__ void __launch_bounds__(256)
cc_tile_kernel(const unsigned char* __restrict__ mask, int H, int W, int* __restrict__ labels) {
  __shared__ int L[CC_N];
  __shared__ unsigned char M[CC_N];
  const long f = blockIdx.z;
  const int x0 = blockIdx.x * CC_T, y0 = blockIdx.y * CC_T;
  const unsigned char* m = mask + f * (long)H * W;
  for (int k = threadIdx.x; k < CC_N; k += 256) {
    const int x = x0 + (k % CC_T), y = y0 + (k / CC_T);
    M[k] = (x < W && y < H && m[(long)y * W + x]) ? 1 : 0;
    L[k] = k;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CC_N; k += 256) {
    if (!M[k]) continue;
    if ((k % CC_T) > 0 && M[k - 1]) cc_union(L, k, k - 1, CC_N);
    if (k >= CC_T && M[k - CC_T]) cc_union(L, k, k - CC_T, CC_N);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < CC_N; k += 256) {
    const int x = x0 + (k % CC_T), y = y0 + (k / CC_T);
    if (x >= W || y >= H) continue;
    int out = -1;
    if (M[k]) {
      const int r = cc_find(L, k, CC_N);
      out = (y0 + r / CC_T) * W + x0 + (r % CC_T);   // row-major order inside the tile = row-major order in the frame
    }
    labels[f * (long)H * W + (long)y * W + x] = out;
  }
}
// pass 2: join across tile borders (pixels of a tile's first column with their left neighbour, first row with the one above)
__global__ void __launch_bounds__(256)
cc_border_kernel(int H, int W, int* labels) {
  const long f = blockIdx.y;
  int* L = labels + f * (long)H * W;
  const int n = H * W;
  const int ncol = (W - 1) / CC_T, nrow = (H - 1) / CC_T;          // interior tile borders
  const long total = (long)ncol * H + (long)nrow * W;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int p, q;
    if (i < (long)ncol * H) {
      const int y = (int)(i % H), x = ((int)(i / H) + 1) * CC_T;
      p = y * W + x; q = p - 1;
    } else {
      const long j = i - (long)ncol * H;
      const int x = (int)(j % W), y = ((int)(j / W) + 1) * CC_T;
      p = y * W + x; q = p - W;
    }
    if (L[p] >= 0 && L[q] >= 0) cc_union(L, p, q, n);
  }
}
// pass 3: every pixel points at the root of its set (a pixel may read a parent another thread is shortening: any value it
// sees is an ancestor, and the find still ends at the root)
__global__ void __launch_bounds__(256)
cc_flatten_kernel(int n, int* labels) {
  int* L = labels + (long)blockIdx.y * n;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    if (__hip_atomic_load(L + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) continue;
    const int r = cc_find(L, p, n);
    __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// pass 4: one workgroup per frame numbers the roots 1, 2, ... in row-major order (exclusive scan over the "is root" flags in
// chunks of 1024 pixels with a running carry: ceil(n / 1024) rounds), then every pixel takes the number of its root
__global__ void __launch_bounds__(1024)
cc_number_kernel(int n, const int* __restrict__ labels, int* __restrict__ rank, int* __restrict__ out) {
  __shared__ int wsum[16];
  __shared__ int carry;
  const int* L = labels + (long)blockIdx.x * n;
  int* R = rank + (long)blockIdx.x * n;
  int* O = out + (long)blockIdx.x * n;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int p = base + threadIdx.x;
    const int flag = (p < n && L[p] == p) ? 1 : 0;
    int v = flag;                                      // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    int before = carry;
    for (int i = 0; i < w; ++i) before += wsum[i];
    if (flag) R[p] = before + v;                       // the component's number
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + v;
    __syncthreads();
  }
  // the ranks were written by this workgroup: visible to all its threads after the barrier above
  for (int p = threadIdx.x; p < n; p += 1024) {
    const int r = L[p];
    O[p] = r < 0 ? 0 : R[r];
  }
}

// ---- depth + semantic camera image (dataset.py:330-352) -------------------------------------------------------------------
__global__ void __launch_bounds__(256)
depth_semantic_decode_kernel(const uchar4* __restrict__ img, const unsigned char* __restrict__ remap, int vehicle, int pedestrian,
                             long HW, long long* __restrict__ semantic, unsigned char* __restrict__ inst, double* __restrict__ color,
                             double* __restrict__ depth) {
  const long f = blockIdx.y;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const uchar4 v = img[f * HW + p];
    if (semantic) semantic[f * HW + p] = remap[v.w];
    if (inst) inst[f * HW + p] = (v.w == vehicle || v.w == pedestrian) ? 1 : 0;
    const double r = (double)v.x, g = (double)v.y, b = (double)v.z;
    if (color) {
      color[(f * 3) * HW + p] = r / 255.0;
      color[(f * 3 + 1) * HW + p] = g / 255.0;
      color[(f * 3 + 2) * HW + p] = b / 255.0;
    }
    if (depth) {
      const double d = (65536.0 * r + 256.0 * g + b) / 16777215.0;      // exact integers up to the one division
      depth[f * HW + p] = d > 0.999 ? -1.0 : d;
    }
  }
}

// ---- batched range projection: the three passes of input.hip with the frame as grid dimension y -------------------------------
__global__ void __launch_bounds__(256)
range_min_depth_frames_kernel(const float* __restrict__ raw, const int* __restrict__ count, long Pmax, RangeArgs a,
                              unsigned long long* __restrict__ best) {
  const long f = blockIdx.y, HW = (long)a.H * a.W;
  const long P = count[f] < Pmax ? count[f] : Pmax;      // never past the padded array
  const float* pts = raw + f * Pmax * 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
    float p[3]; double depth; int ph, pw;
    if (!range_point(pts, i, a, p, depth, ph, pw)) continue;
    atomicMin(best + f * HW + (long)ph * a.W + pw, (unsigned long long)__double_as_longlong(depth));
  }
}
__global__ void __launch_bounds__(256)
range_min_index_frames_kernel(const float* __restrict__ raw, const int* __restrict__ count, long Pmax, RangeArgs a,
                              const unsigned long long* __restrict__ best, unsigned int* __restrict__ winner) {
  const long f = blockIdx.y, HW = (long)a.H * a.W;
  const long P = count[f] < Pmax ? count[f] : Pmax;      // never past the padded array
  const float* pts = raw + f * Pmax * 3;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
    float p[3]; double depth; int ph, pw;
    if (!range_point(pts, i, a, p, depth, ph, pw)) continue;
    const long px = f * HW + (long)ph * a.W + pw;
    if ((unsigned long long)__double_as_longlong(depth) == best[px]) atomicMin(winner + px, (unsigned int)i);
  }
}
__global__ void __launch_bounds__(256)
range_write_frames_kernel(const float* __restrict__ raw, const unsigned char* __restrict__ tag, const unsigned char* __restrict__ remap,
                          long Pmax, RangeArgs a, const unsigned int* __restrict__ winner, float* __restrict__ xyzd,
                          long long* __restrict__ seg) {
  const long f = blockIdx.y, HW = (long)a.H * a.W;
  for (long px = blockIdx.x * 256L + threadIdx.x; px < HW; px += (long)gridDim.x * 256) {
    float p[3], d;
    unsigned char s;
    range_pixel(raw + f * Pmax * 3, tag + f * Pmax, remap, a, winner[f * HW + px], p, d, s);
    float* o = xyzd + f * 4 * HW;
    o[px] = p[0]; o[HW + px] = p[1]; o[2 * HW + px] = p[2]; o[3 * HW + px] = d;
    if (seg) seg[f * HW + px] = s;
  }
}

// ---- batched voxel densification --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
voxel_scatter_frames_kernel(const long long* __restrict__ rows, const int* __restrict__ count, long Qmax,
                            const unsigned char* __restrict__ remap, int X, int Y, int Z, unsigned int* __restrict__ key) {
  const long f = blockIdx.y;
  const long Q = count[f] < Qmax ? count[f] : Qmax;      // never past the padded array
  for (long i = blockIdx.x * 256L + threadIdx.x; i < Q; i += (long)gridDim.x * 256)
    voxel_scatter_row(rows + f * Qmax * 4, i, remap, X, Y, Z, key + f * (long)X * Y * Z);
}
__global__ void __launch_bounds__(256)
voxel_decode_frames_kernel(const unsigned int* __restrict__ key, unsigned char* __restrict__ vox, long n) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) vox[i] = (unsigned char)(key[i] & 0xffu);
}

#define ST ((hipStream_t)stream)
#define MAX_FRAMES 65535
static inline unsigned frame_grid(long n_per_frame, int F) {
  long g = (ew_grid(n_per_frame * F) + F - 1) / F;      // the blocks an elementwise launch would get, spread over the frames
  return (unsigned)(g < 1 ? 1 : g);
}

extern "C" {

int muvo_birdview_decode_frames(const int32_t* birdview_int, int F, int H, int W, int n_classes, float* birdview, int64_t* label,
                                uint8_t* instance_mask, void* stream) {
  MUVO_CHECK_ARG(birdview_int && birdview && label && instance_mask, "birdview_decode_frames: null pointer");
  MUVO_CHECK_ARG(F > 0 && F <= MAX_FRAMES && H > 0 && W > 0 && n_classes > 0 && n_classes <= 31, "birdview_decode_frames: bad sizes");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(birdview_decode_kernel, dim3(frame_grid(HW, F), F), dim3(256), 0, ST, birdview_int, n_classes, HW, birdview,
                     (long long*)label, instance_mask);
  MUVO_CHECK_LAUNCH("birdview_decode_frames");
  return MUVO_OK;
}

int muvo_label_components_frames(const uint8_t* mask, int F, int H, int W, int32_t* scratch, int32_t* labels, void* stream) {
  MUVO_CHECK_ARG(mask && scratch && labels, "label_components_frames: null pointer");
  MUVO_CHECK_ARG(F > 0 && F <= MAX_FRAMES && H > 0 && W > 0 && (long)H * W < (1l << 30) && (H + CC_T - 1) / CC_T <= 65535,
                 "label_components_frames: bad sizes");
  const int n = H * W;
  int* parent = scratch;
  int* rank = scratch + (long)F * n;
  hipLaunchKernelGGL(cc_tile_kernel, dim3((W + CC_T - 1) / CC_T, (H + CC_T - 1) / CC_T, F), dim3(256), 0, ST, mask, H, W, parent);
  const long nborder = (long)((W - 1) / CC_T) * H + (long)((H - 1) / CC_T) * W;
  if (nborder > 0)
    hipLaunchKernelGGL(cc_border_kernel, dim3(frame_grid(nborder, F), F), dim3(256), 0, ST, H, W, parent);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(frame_grid(n, F), F), dim3(256), 0, ST, n, parent);
  hipLaunchKernelGGL(cc_number_kernel, dim3(F), dim3(1024), 0, ST, n, parent, rank, labels);
  MUVO_CHECK_LAUNCH("label_components_frames");
  return MUVO_OK;
}

int muvo_depth_semantic_decode_frames(const uint8_t* depth_semantic, int F, int H, int W, const uint8_t* remap, int vehicle_tag,
                                      int pedestrian_tag, int64_t* semantic_image, uint8_t* image_instance_mask, double* depth_color,
                                      double* depth, void* stream) {
  MUVO_CHECK_ARG(depth_semantic && remap, "depth_semantic_decode_frames: null pointer");
  MUVO_CHECK_ARG(semantic_image || image_instance_mask || depth_color || depth, "depth_semantic_decode_frames: no output asked for");
  MUVO_CHECK_ARG(F > 0 && F <= MAX_FRAMES && H > 0 && W > 0, "depth_semantic_decode_frames: bad sizes");
  const long HW = (long)H * W;
  hipLaunchKernelGGL(depth_semantic_decode_kernel, dim3(frame_grid(HW, F), F), dim3(256), 0, ST, (const uchar4*)depth_semantic, remap,
                     vehicle_tag, pedestrian_tag, HW, (long long*)semantic_image, image_instance_mask, depth_color, depth);
  MUVO_CHECK_LAUNCH("depth_semantic_decode_frames");
  return MUVO_OK;
}

int muvo_range_projection_frames(const float* points_xyz, const uint8_t* obj_tag, const int32_t* num_points, const uint8_t* remap, int F,
                                 int64_t Pmax, const double* lidar_pos, const double* ego_dim, double fov_down_deg, double fov_up_deg,
                                 int H, int W, void* scratch, float* xyzd, int64_t* seg, void* stream) {
  MUVO_CHECK_ARG(num_points && remap && lidar_pos && ego_dim && scratch && xyzd && (Pmax == 0 || (points_xyz && obj_tag)),
                 "range_projection_frames: null pointer");
  MUVO_CHECK_ARG(F > 0 && F <= MAX_FRAMES && Pmax >= 0 && Pmax < 0x7fffffffll && H > 0 && W > 0, "range_projection_frames: bad sizes");
  const RangeArgs a = range_args(lidar_pos, ego_dim, fov_down_deg, fov_up_deg, H, W);
  const long HW = (long)H * W;
  unsigned long long* best = (unsigned long long*)scratch;
  unsigned int* winner = (unsigned int*)(best + HW * F);
  if (hipMemsetAsync(scratch, 0xff, (size_t)HW * F * 12, ST) != hipSuccess) {
    muvo_set_error("range_projection_frames: memset failed");
    return MUVO_ERR_HIP;
  }
  if (Pmax > 0) {
    const dim3 g(frame_grid(Pmax, F), F);
    hipLaunchKernelGGL(range_min_depth_frames_kernel, g, dim3(256), 0, ST, points_xyz, num_points, (long)Pmax, a, best);
    hipLaunchKernelGGL(range_min_index_frames_kernel, g, dim3(256), 0, ST, points_xyz, num_points, (long)Pmax, a, best, winner);
  }
  hipLaunchKernelGGL(range_write_frames_kernel, dim3(frame_grid(HW, F), F), dim3(256), 0, ST, points_xyz, obj_tag, remap, (long)Pmax, a,
                     winner, xyzd, (long long*)seg);
  MUVO_CHECK_LAUNCH("range_projection_frames");
  return MUVO_OK;
}

int muvo_voxel_grid_frames(const int64_t* rows, const int32_t* num_rows, const uint8_t* remap, int F, int64_t Qmax, int X, int Y, int Z,
                           uint32_t* scratch, uint8_t* voxels, void* stream) {
  MUVO_CHECK_ARG(num_rows && remap && scratch && voxels && (Qmax == 0 || rows), "voxel_grid_frames: null pointer");
  MUVO_CHECK_ARG(F > 0 && F <= MAX_FRAMES && Qmax >= 0 && Qmax < (1 << 24) && X > 0 && Y > 0 && Z > 0, "voxel_grid_frames: bad sizes (Qmax < 2^24)");
  const long n = (long)X * Y * Z * F;
  if (hipMemsetAsync(scratch, 0, sizeof(uint32_t) * (size_t)n, ST) != hipSuccess) {
    muvo_set_error("voxel_grid_frames: memset failed");
    return MUVO_ERR_HIP;
  }
  if (Qmax > 0)
    hipLaunchKernelGGL(voxel_scatter_frames_kernel, dim3(frame_grid(Qmax, F), F), dim3(256), 0, ST, (const long long*)rows, num_rows,
                       (long)Qmax, remap, X, Y, Z, scratch);
  hipLaunchKernelGGL(voxel_decode_frames_kernel, dim3(ew_grid(n)), dim3(256), 0, ST, scratch, voxels, n);
  MUVO_CHECK_LAUNCH("voxel_grid_frames");
  return MUVO_OK;
}

}  // extern "C"
