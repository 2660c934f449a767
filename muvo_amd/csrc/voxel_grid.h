// What the voxel-head units (raycast.hip, render.hip, render_class.hip, lovasz.hip) share: the limits and their host checks, the ray
// walk of muvo_raycast, the access to 4 consecutive voxels per lane, the per-voxel softmax statistics over the class planes, and
// what the two rendered losses share: the sum over runs of lanes before an atomic and the finish of the loss.
#pragma once
#include "common.h"

#define VG_MAXC 16
#define VG_MAXDIM 2048          // (float)N is exact and (x Y + y) Z + z stays far below 2^31 together with the voxel bound below

// ---- host: the size bounds of the entries, with the texts they refuse with ---------------------------------------------------
static inline bool vg_frames_ok(int64_t F) { return F >= 1 && F <= 65535; }
static inline bool vg_axes_ok(int X, int Y, int Z) { return X >= 1 && Y >= 1 && Z >= 1 && X <= VG_MAXDIM && Y <= VG_MAXDIM && Z <= VG_MAXDIM; }
static inline bool vg_voxels_ok(int64_t V) { return V >= 1 && V < (1ll << 30); }
static inline bool vg_rays_ok(int64_t R) { return R >= 1 && R <= (1ll << 24); }

static inline int vg_check_frames(const char* who, int64_t F) {
  MUVO_CHECK_ARG(vg_frames_ok(F), "%s: %lld frames outside 1..65535", who, (long long)F);
  return MUVO_OK;
}
static inline int vg_check_classes(const char* who, int C) {
  MUVO_CHECK_ARG(C >= 2 && C <= VG_MAXC, "%s: C = %d outside 2..%d", who, C, VG_MAXC);
  return MUVO_OK;
}
static inline int vg_check_grid(const char* who, int X, int Y, int Z) {
  MUVO_CHECK_ARG(vg_axes_ok(X, Y, Z) && vg_voxels_ok((int64_t)X * Y * Z), "%s: grid %d x %d x %d (1..%d per axis, below 2^30 voxels)", who, X, Y, Z,
                 VG_MAXDIM);
  return MUVO_OK;
}
static inline int vg_check_rays(const char* who, int64_t R) {
  MUVO_CHECK_ARG(vg_rays_ok(R), "%s: %lld rays outside 1..2^24", who, (long long)R);
  return MUVO_OK;
}

// ---- the walk: steps 1 - 3 of the definition of include/muvo_hip.h (muvo_raycast), statement by statement and in its order.
// tests/raycast_reference.py restates it in numpy float32 and the kernels are compared with it bit for bit: fp32 only, nothing
// reassociated or contracted, division only as 1.0f / d.  The three axes are handled by the same macro three times and selected
// with compares: no local array is indexed dynamically (the build refuses scratch memory).
struct VgRay {
  float ox, oy, oz, dx, dy, dz, ix, iy, iz;
  float t1;                                // exit depth
  float t;                                 // entry depth of the current cell
  int cx, cy, cz;
};

__device__ __forceinline__ int vg_cell(float p, int N) {
  const float f = floorf(p);
  return !(f >= 0.f) ? 0 : (f > (float)(N - 1) ? N - 1 : (int)f);
}

#define VG_SLAB(o, d, inv, N, a)                                                   \
  if (d != 0.f) {                                                                  \
    inv = 1.0f / d;                                                                \
    const float ta = (0.0f - o) * inv, tb = ((float)(N) - o) * inv;                \
    const bool asc = ta <= tb;                                                     \
    const float lo = asc ? ta : tb, hi = asc ? tb : ta;                            \
    if (!(lo <= hi)) ok = false;                                                   \
    if (lo > t0) { t0 = lo; entry = a; }                                           \
    if (hi < t1) t1 = hi;                                                          \
    any = true;                                                                    \
  } else if (!(0.0f <= o && o < (float)(N))) {                                     \
    ok = false;                                                                    \
  }

#define VG_NEXT(o, d, inv, c, a)                                                   \
  if (d != 0.f) {                                                                  \
    const float tn = ((float)(c + (d > 0.f ? 1 : 0)) - o) * inv;                   \
    if (tn < best) { best = tn; axis = a; }                                        \
  }

// steps 1 and 2 for the ray q = (o, d, tmax): the slab test, t0 / t1, the start cell; entry = the face the ray enters through
// (3: it starts inside).  false: the ray is invalid (muvo_raycast calls it a miss before its step 2).
__device__ __forceinline__ bool vg_start(VgRay& s, const float* __restrict__ q, int X, int Y, int Z, int& entry) {
  s.ox = q[0]; s.oy = q[1]; s.oz = q[2]; s.dx = q[3]; s.dy = q[4]; s.dz = q[5];
  float t0 = 0.f, t1 = q[6];
  s.ix = 0.f; s.iy = 0.f; s.iz = 0.f;
  entry = 3;
  bool ok = true, any = false;
  VG_SLAB(s.ox, s.dx, s.ix, X, 0)
  VG_SLAB(s.oy, s.dy, s.iy, Y, 1)
  VG_SLAB(s.oz, s.dz, s.iz, Z, 2)
  s.t1 = t1;
  s.t = t0;
  s.cx = 0; s.cy = 0; s.cz = 0;
  if (!ok || !any || !(t0 < t1)) return false;
  s.cx = vg_cell(s.ox + s.dx * t0, X);
  s.cy = vg_cell(s.oy + s.dy * t0, Y);
  s.cz = vg_cell(s.oz + s.dz * t0, Z);
  return true;
}

// step 3 behind the occupancy test: to the next cell.  Returns the axis crossed, -1: the walk has ended (best > t1, or the ray
// left the grid).  The bounds tests of the three axes meet in one exit: with a return inside each of them the compiler moved the
// three moves off the loop's straight path, two taken branches more per step (ray_iou_counts 5 % slower, DESIGN.md 8d's case).
// The cell moves in local copies: moved inside the struct, the three branches become one dynamically indexed access - scratch.
__device__ __forceinline__ int vg_step(VgRay& s, int X, int Y, int Z) {
  float best = __builtin_inff();
  int axis = -1;
  VG_NEXT(s.ox, s.dx, s.ix, s.cx, 0)
  VG_NEXT(s.oy, s.dy, s.iy, s.cy, 1)
  VG_NEXT(s.oz, s.dz, s.iz, s.cz, 2)
  if (axis < 0 || best > s.t1) return -1;
  int cx = s.cx, cy = s.cy, cz = s.cz;
  bool in;
  if (axis == 0) {
    cx += s.dx > 0.f ? 1 : -1;
    in = cx >= 0 && cx < X;
  } else if (axis == 1) {
    cy += s.dy > 0.f ? 1 : -1;
    in = cy >= 0 && cy < Y;
  } else {
    cz += s.dz > 0.f ? 1 : -1;
    in = cz >= 0 && cz < Z;
  }
  s.cx = cx; s.cy = cy; s.cz = cz;
  if (!in) return -1;
  s.t = best;
  return axis;
}
#undef VG_SLAB
#undef VG_NEXT

// ---- the 4 x 4 x 4 bricks (occupancy: raycast.hip; SEEN: visibility.hip; both: voxel_aggregate.hip): one uint64 per brick, word
// ((x>>2) BY + (y>>2)) BZ + (z>>2) of the frame, bit (x&3) 16 + (y&3) 4 + (z&3)
__device__ __forceinline__ int vg_brick_word(int x, int y, int z, int BY, int BZ) { return ((x >> 2) * BY + (y >> 2)) * BZ + (z >> 2); }
__device__ __forceinline__ int vg_brick_shift(int x, int y, int z) { return ((x & 3) << 4) | ((y & 3) << 2) | (z & 3); }

// ---- 4 consecutive voxels per lane: one 16-byte access (4 bytes for labels) when `vec` - aligned bases, V % 4 == 0, so that
// h0 + 3 < V - guarded scalars otherwise
__device__ __forceinline__ f32x4 vg_ld4(const float* __restrict__ p, long h0, long V, bool vec) {
  if (vec) return *(const f32x4*)(p + h0);
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (h0 < V) r.x = p[h0];
  if (h0 + 1 < V) r.y = p[h0 + 1];
  if (h0 + 2 < V) r.z = p[h0 + 2];
  if (h0 + 3 < V) r.w = p[h0 + 3];
  return r;
}
template <class T, class T4>                     // (float, f32x4) and (uint32_t, uint4)
__device__ __forceinline__ void vg_st4(T* __restrict__ p, long h0, long V, bool vec, T4 v) {
  if (vec) { *(T4*)(p + h0) = v; return; }
  if (h0 < V) p[h0] = v.x;
  if (h0 + 1 < V) p[h0 + 1] = v.y;
  if (h0 + 2 < V) p[h0 + 2] = v.z;
  if (h0 + 3 < V) p[h0 + 3] = v.w;
}
// the labels of the 4 voxels, `fill` past the end
__device__ __forceinline__ void vg_ld4(const uint8_t* __restrict__ lab, long h0, long V, bool vec, unsigned fill, unsigned l[4]) {
  if (vec) {
    const uint32_t w = *(const uint32_t*)(lab + h0);
    l[0] = w & 255u; l[1] = (w >> 8) & 255u; l[2] = (w >> 16) & 255u; l[3] = w >> 24;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) l[k] = h0 + k < V ? lab[h0 + k] : fill;
}

// ---- softmax statistics of the 4 voxels over the C planes (fp32, as torch.softmax): m = the maximum, e0 = exp(x_0 - m),
// rest = sum_{c >= 1} exp(x_c - m) and sum = sum_{c >= 0} exp(x_c - m), both in ascending c.  sum = ((e0 + e_1) + e_2) + ... and
// e0 + rest = e0 + ((e_1 + e_2) + ...) differ in the last bit from C = 3 on, so each user keeps the sum its results are made
// of: render.hip e0 and rest, lovasz.hip sum.  The one a caller ignores costs nothing once this is inlined.
struct VgSoftmax {
  f32x4 m, e0, rest, sum;
};
__device__ __forceinline__ VgSoftmax vg_softmax_stats(const float* __restrict__ lf, int C, long V, long h0, bool vec) {
  const f32x4 x0 = vg_ld4(lf, h0, V, vec);
  VgSoftmax r;
  r.m = x0;
  for (int c = 1; c < C; ++c) {
    const f32x4 x = vg_ld4(lf + (size_t)c * V, h0, V, vec);
    r.m.x = fmaxf(r.m.x, x.x); r.m.y = fmaxf(r.m.y, x.y); r.m.z = fmaxf(r.m.z, x.z); r.m.w = fmaxf(r.m.w, x.w);
  }
  r.e0 = f32x4{expf(x0.x - r.m.x), expf(x0.y - r.m.y), expf(x0.z - r.m.z), expf(x0.w - r.m.w)};
  r.rest = f32x4{0.f, 0.f, 0.f, 0.f};
  r.sum = r.e0;
  for (int c = 1; c < C; ++c) {
    const f32x4 x = vg_ld4(lf + (size_t)c * V, h0, V, vec);
    const f32x4 e = {expf(x.x - r.m.x), expf(x.y - r.m.y), expf(x.z - r.m.z), expf(x.w - r.m.w)};
    r.rest += e;
    r.sum += e;
  }
  return r;
}
__device__ __forceinline__ f32x4 vg_prob(f32x4 x, f32x4 m, f32x4 s) {
  return f32x4{expf(x.x - m.x) / s.x, expf(x.y - m.y) / s.y, expf(x.z - m.z) / s.z, expf(x.w - m.w) / s.w};
}

// ---- the rendered losses (render.hip, render_class.hip) ---------------------------------------------------------------------------
// Sums `val` over runs of neighbouring lanes - a run starts at every lane with `head` - by a segmented shuffle reduction of fixed
// cost (6 steps); the head lane of a run holds its sum.  Every lane of the wave must take part.
__device__ __forceinline__ long long vg_run_sum(long long val, bool head, int lane) {
  const unsigned long long heads = __ballot(head);
  const unsigned long long after = lane < 63 ? heads >> (lane + 1) : 0ull;      // lane i + o belongs to the run of lane i iff no run starts in (i, i + o]
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_down(val, o, 64);
    if (lane + o < 64 && (after & ((1ull << o) - 1ull)) == 0ull) val += u;
  }
  return val;
}

// loss[0] = weight / (F N) x the sum of the P fp64 partials.  One workgroup of 256: thread l adds the partials l, l + 256, ... in
// order, the lanes of a wave are added by a fixed butterfly, the four waves in their order
static __global__ void __launch_bounds__(256) vg_finish_kernel(const double* __restrict__ part, long P, float weight, long F, long N, float* __restrict__ loss) {
  __shared__ double red[4];
  double s = 0.0;
  for (long p = threadIdx.x; p < P; p += 256) s += part[p];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = N > 0 ? (float)((double)weight * (((red[0] + red[1]) + red[2]) + red[3]) / ((double)F * (double)N)) : 0.f;
}
