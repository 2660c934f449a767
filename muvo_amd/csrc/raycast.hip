// First-hit ray casting through voxel class grids (muvo_amd/voxel_view.py): the `_voxel` panel and the RayIoU metric.  The march
// is the definition of include/muvo_hip.h (muvo_raycast): its walk from cell to cell is vg_start / vg_step of voxel_grid.h, which
// render.hip takes too.
// One thread owns one ray of one frame; the rays of a wave are neighbours of the table (adjacent pixels of the camera, adjacent
// azimuths of a lidar beam), so they enter the grid together and diverge only where the surfaces they meet differ.  Occupancy
// comes from 4 x 4 x 4 bricks, one uint64 each (bit (x&3) 16 + (y&3) 4 + (z&3)): the word of the current brick stays in registers
// and is loaded again only when the ray leaves the brick - one 8-byte load per up to ~10 steps instead of one byte load per
// step - and a frame's words (288 KiB at 192 x 192 x 64) stay in the L2 of every XCD that marches it.  The class byte is read once, at
// the hit.  Measured against the same march testing the class bytes directly: 10 - 25 % less time, equal results.
// The loop has the hard bound X + Y + Z + 3 whatever the input.
#include <algorithm>

#include "voxel_grid.h"

struct RcGrid {
  const uint8_t* __restrict__ cls;       // (X, Y, Z) classes of this frame
  const uint64_t* __restrict__ bricks;   // its words
  int X, Y, Z, BY, BZ;
};

struct RcHit {
  int idx;                      // (x Y + y) Z + z, -1: miss
  float t;
  int face;
};

// the walk of voxel_grid.h with the occupancy test in front of every step: hit.t = the entry depth of the occupied cell, hit.face =
// the axis of the boundary crossed last (the entry face in the start cell)
__device__ __forceinline__ RcHit rc_march(const RcGrid& g, const float* __restrict__ q) {
  const RcHit miss{-1, 0.f, 0};
  VgRay s;
  int face;
  if (!vg_start(s, q, g.X, g.Y, g.Z, face)) return miss;
  int held = -1;
  uint64_t word = 0;
  const int bound = g.X + g.Y + g.Z + 3;
  for (int it = 0; it < bound; ++it) {
    const int b = vg_brick_word(s.cx, s.cy, s.cz, g.BY, g.BZ);
    if (b != held) { word = g.bricks[b]; held = b; }
    const bool occupied = (word >> vg_brick_shift(s.cx, s.cy, s.cz)) & 1ull;
    if (occupied) return RcHit{(s.cx * g.Y + s.cy) * g.Z + s.cz, s.t, face};
    face = vg_step(s, g.X, g.Y, g.Z);
    if (face < 0) return miss;
  }
  return miss;
}

struct RcFrames {               // F frames of one grid size
  const uint8_t* __restrict__ cls;
  const uint64_t* __restrict__ bricks;
  int X, Y, Z, BX, BY, BZ;
  __device__ __forceinline__ RcGrid frame(int f) const {
    return RcGrid{cls + (size_t)f * X * Y * Z, bricks + (size_t)f * BX * BY * BZ, X, Y, Z, BY, BZ};
  }
};

// ---- bricks --------------------------------------------------------------------------------------------------------------------
// One thread per brick, bz fastest: for a fixed column (x, y) the lanes of a wave read consecutive 4-z groups - 16 bytes each per class
// plane of the logits (one dword of the uint8 grid) when `vec`, i.e. Z % 4 == 0 and the base is aligned - so every load
// instruction takes whole lines.  The logits form also writes the class bytes it has just decided.
template <bool LOGITS>
__global__ void __launch_bounds__(256) rc_bricks_kernel(const void* __restrict__ src, int C, int X, int Y, int Z, int BX, int BY, int BZ, int vec,
                                                        uint8_t* __restrict__ cls_out, uint64_t* __restrict__ bricks) {
  const long nb = (long)BX * BY * BZ;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= nb) return;
  const int bz = (int)(i % BZ), by = (int)((i / BZ) % BY), bx = (int)(i / ((long)BZ * BY));
  const size_t V = (size_t)X * Y * Z;
  const int z0 = bz * 4;
  uint64_t word = 0;
  for (int k = 0; k < 16; ++k) {
    const int x = bx * 4 + (k >> 2), y = by * 4 + (k & 3);
    if (x >= X || y >= Y) continue;
    const size_t at = ((size_t)x * Y + y) * Z + z0;
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    const bool v1 = z0 + 1 < Z, v2 = z0 + 2 < Z, v3 = z0 + 3 < Z;
    if (LOGITS) {
      const float* __restrict__ q = (const float*)src + (size_t)f * C * V + at;
      if (vec) {
        f32x4 b = *(const f32x4*)q;
        for (int c = 1; c < C; ++c) {
          const f32x4 v = *(const f32x4*)(q + (size_t)c * V);
          if (v.x > b.x) { b.x = v.x; c0 = c; }
          if (v.y > b.y) { b.y = v.y; c1 = c; }
          if (v.z > b.z) { b.z = v.z; c2 = c; }
          if (v.w > b.w) { b.w = v.w; c3 = c; }
        }
        *(uint32_t*)(cls_out + (size_t)f * V + at) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
      } else {
        float b0 = q[0], b1 = v1 ? q[1] : 0.f, b2 = v2 ? q[2] : 0.f, b3 = v3 ? q[3] : 0.f;
        for (int c = 1; c < C; ++c) {
          const float* __restrict__ qc = q + (size_t)c * V;
          const float a0 = qc[0];
          if (a0 > b0) { b0 = a0; c0 = c; }
          if (v1) { const float a = qc[1]; if (a > b1) { b1 = a; c1 = c; } }
          if (v2) { const float a = qc[2]; if (a > b2) { b2 = a; c2 = c; } }
          if (v3) { const float a = qc[3]; if (a > b3) { b3 = a; c3 = c; } }
        }
        uint8_t* __restrict__ o = cls_out + (size_t)f * V + at;
        o[0] = (uint8_t)c0;
        if (v1) o[1] = (uint8_t)c1;
        if (v2) o[2] = (uint8_t)c2;
        if (v3) o[3] = (uint8_t)c3;
      }
    } else {
      const uint8_t* __restrict__ q = (const uint8_t*)src + (size_t)f * V + at;
      if (vec) {
        const uint32_t w = *(const uint32_t*)q;
        c0 = w & 255u; c1 = (w >> 8) & 255u; c2 = (w >> 16) & 255u; c3 = w >> 24;
      } else {
        c0 = q[0];
        if (v1) c1 = q[1];
        if (v2) c2 = q[2];
        if (v3) c3 = q[3];
      }
    }
    const uint64_t bits = (c0 ? 1ull : 0ull) | (c1 ? 2ull : 0ull) | (c2 ? 4ull : 0ull) | (c3 ? 8ull : 0ull);
    word |= bits << (4 * k);                               // bit (x&3) 16 + (y&3) 4 + (z&3), k = (x&3) 4 + (y&3)
  }
  bricks[(size_t)f * nb + i] = word;
}

// ---- the three users of the march ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) rc_cast_kernel(RcFrames g, const float* __restrict__ rays, long R, int32_t* __restrict__ hit,
                                                      float* __restrict__ t, uint8_t* __restrict__ face) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (r >= R) return;
  const float* __restrict__ q = rays + r * 7;
  const RcHit h = rc_march(g.frame(f), q);
  const size_t o = (size_t)f * R + r;
  hit[o] = h.idx;
  t[o] = h.t;
  face[o] = (uint8_t)h.face;
}

// a thread owns one pixel of the padded tile; ray i R + j is pixel (i, j) of the interior
__global__ void __launch_bounds__(256) rc_view_kernel(RcFrames g, const float* __restrict__ rays, int R, const uint8_t* __restrict__ palette, int pad,
                                                      int padbyte, MuvoTilePlace pl, uint8_t* __restrict__ panel) {
  const int T = R + 2 * pad;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (idx >= (long)T * T) return;
  const int pi = (int)(idx / T), pj = (int)(idx % T);
  const int smp = f / pl.T, step = pl.t0 + f % pl.T;
  const int row0 = pl.y0 + step * pl.ystep, col0 = pl.x0 + step * pl.xstep + (step >= pl.tsep ? pl.sepw : 0);
  const long a = (long)smp * pl.sample_stride + (long)(row0 + pi) * pl.PW + col0 + pj;
  const int i = pi - pad, j = pj - pad;
  unsigned cr = (unsigned)padbyte, cg = cr, cb = cr;
  if (i >= 0 && i < R && j >= 0 && j < R) {
    const float* __restrict__ q = rays + ((long)i * R + j) * 7;
    const RcGrid fr = g.frame(f);
    const RcHit h = rc_march(fr, q);
    if (h.idx < 0) {
      cr = palette[0]; cg = palette[1]; cb = palette[2];
    } else {
      const unsigned cls = fr.cls[h.idx], z = (unsigned)(h.idx % g.Z);
      const unsigned s = (h.face == 0 ? 176u : (h.face == 1 ? 208u : 255u)) * (96u + (159u * z) / (unsigned)max(g.Z - 1, 1));
      cr = (palette[3 * cls] * s) / 65025u; cg = (palette[3 * cls + 1] * s) / 65025u; cb = (palette[3 * cls + 2] * s) / 65025u;
    }
  }
  panel[a] = (uint8_t)cr;
  panel[a + pl.chan_stride] = (uint8_t)cg;
  panel[a + 2 * pl.chan_stride] = (uint8_t)cb;
}

// Both grids along the same ray.  counts (3, C, 3) in LDS first, one 64-bit atomic per non-zero cell and workgroup afterwards:
// integer sums, order-free.  The depth sums leave as one fp64 partial pair per workgroup (part[(f NB + block) 2 + k]).
__global__ void __launch_bounds__(256) rc_iou_kernel(RcFrames gl, RcFrames gp, const float* __restrict__ rays, long R, int C, float res, float thr0,
                                                     float thr1, float thr2, unsigned long long* __restrict__ counts, double* __restrict__ part) {
  __shared__ unsigned cnt[3 * VG_MAXC * 3];
  __shared__ double red[2][4];
  for (int k = threadIdx.x; k < 9 * C; k += 256) cnt[k] = 0;
  __syncthreads();
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  double sum = 0.0, n = 0.0;
  if (r < R) {
    const float* __restrict__ q = rays + r * 7;
    const RcGrid fl = gl.frame(f), fp = gp.frame(f);
    const RcHit hl = rc_march(fl, q);
    const RcHit hp = rc_march(fp, q);
    const int cl = hl.idx >= 0 ? (int)fl.cls[hl.idx] : -1, cp = hp.idx >= 0 ? (int)fp.cls[hp.idx] : -1;
    const bool both = cl >= 0 && cp >= 0;
    const float err = both ? fabsf(hp.t - hl.t) * res : 0.f;
    if (both) { sum = (double)err; n = 1.0; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float thr = k == 0 ? thr0 : (k == 1 ? thr1 : thr2);
      if (both && cl == cp && err <= thr) {
        if (cl < C) atomicAdd(&cnt[(k * C + cl) * 3], 1u);
      } else {
        if (cl >= 0 && cl < C) atomicAdd(&cnt[(k * C + cl) * 3 + 2], 1u);
        if (cp >= 0 && cp < C) atomicAdd(&cnt[(k * C + cp) * 3 + 1], 1u);
      }
    }
  }
  sum = wave_sum_d(sum);
  n = wave_sum_d(n);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sum; red[1][threadIdx.x >> 6] = n; }
  __syncthreads();
  for (int k = threadIdx.x; k < 9 * C; k += 256)
    if (cnt[k]) atomicAdd(&counts[k], (unsigned long long)cnt[k]);
  if (threadIdx.x < 2)
    part[((size_t)f * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// one wave: lane l adds the partials l, l + 64, ... in order, the lanes are added by a fixed butterfly, acc[k] += total
__global__ void __launch_bounds__(64) rc_iou_sum_kernel(const double* __restrict__ part, long P, double* __restrict__ acc) {
  for (int k = 0; k < 2; ++k) {
    double s = 0.0;
    for (long p = threadIdx.x; p < P; p += 64) s += part[p * 2 + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) acc[k] += s;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

static int rc_sizes(const char* who, int F, int X, int Y, int Z) {
  if (int rc = vg_check_frames(who, F)) return rc;
  return vg_check_grid(who, X, Y, Z);
}

static RcFrames rc_frames(const uint8_t* cls, const uint64_t* bricks, int X, int Y, int Z) {
  return RcFrames{cls, bricks, X, Y, Z, (X + 3) / 4, (Y + 3) / 4, (Z + 3) / 4};
}

static int rc_bricks(const char* who, const void* src, bool logits, int F, int C, int X, int Y, int Z, uint8_t* grid, uint64_t* bricks, int64_t words,
                     hipStream_t st) {
  if (int rc = rc_sizes(who, F, X, Y, Z)) return rc;
  MUVO_CHECK_ARG(src && bricks && (grid || !logits), "%s: null pointer", who);
  MUVO_CHECK_ARG(words >= muvo_raycast_brick_words(F, X, Y, Z) && ((uintptr_t)bricks & 7) == 0, "%s: %lld brick words, %lld needed (8-byte aligned)", who,
                 (long long)words, (long long)muvo_raycast_brick_words(F, X, Y, Z));
  const int BX = (X + 3) / 4, BY = (Y + 3) / 4, BZ = (Z + 3) / 4;
  const long nb = (long)BX * BY * BZ;
  const dim3 grd((unsigned)((nb + 255) / 256), (unsigned)F);
  if (logits) {
    const int vec = (Z % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)grid & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(rc_bricks_kernel<true>, grd, dim3(256), 0, st, src, C, X, Y, Z, BX, BY, BZ, vec, grid, bricks);
  } else {
    const int vec = (Z % 4 == 0 && ((uintptr_t)src & 3) == 0) ? 1 : 0;
    hipLaunchKernelGGL(rc_bricks_kernel<false>, grd, dim3(256), 0, st, src, 0, X, Y, Z, BX, BY, BZ, vec, (uint8_t*)nullptr, bricks);
  }
  MUVO_CHECK_LAUNCH(who);
  return MUVO_OK;
}

extern "C" {

int64_t muvo_raycast_brick_words(int F, int X, int Y, int Z) {
  if (!(vg_frames_ok(F) && vg_axes_ok(X, Y, Z))) return -1;
  return (int64_t)F * ((X + 3) / 4) * ((Y + 3) / 4) * ((Z + 3) / 4);
}

int muvo_raycast_bricks_grid(const uint8_t* grid, int F, int X, int Y, int Z, uint64_t* bricks, int64_t words, void* stream) {
  return rc_bricks("raycast_bricks_grid", grid, false, F, 0, X, Y, Z, nullptr, bricks, words, ST);
}

int muvo_raycast_bricks_logits(const float* logits, int F, int C, int X, int Y, int Z, uint8_t* grid, uint64_t* bricks, int64_t words, void* stream) {
  if (int rc = vg_check_classes("raycast_bricks_logits", C)) return rc;
  return rc_bricks("raycast_bricks_logits", logits, true, F, C, X, Y, Z, grid, bricks, words, ST);
}

int muvo_raycast(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int64_t R, int32_t* hit, float* t,
                 uint8_t* face, void* stream) {
  if (int rc = rc_sizes("raycast", F, X, Y, Z)) return rc;
  if (int rc = vg_check_rays("raycast", R)) return rc;
  MUVO_CHECK_ARG(grid && bricks && rays && hit && t && face, "raycast: null pointer");
  hipLaunchKernelGGL(rc_cast_kernel, dim3((unsigned)((R + 255) / 256), (unsigned)F), dim3(256), 0, ST, rc_frames(grid, bricks, X, Y, Z), rays, (long)R, hit, t,
                     face);
  MUVO_CHECK_LAUNCH("raycast");
  return MUVO_OK;
}

int muvo_panel_voxel_view(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int R, const uint8_t* palette, int pad,
                          int padbyte, uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  if (int rc = rc_sizes("panel_voxel_view", F, X, Y, Z)) return rc;
  MUVO_CHECK_ARG(R >= 1 && R <= 4096, "panel_voxel_view: a tile of R = %d rays a side outside 1..4096", R);
  MUVO_CHECK_ARG(grid && bricks && rays && palette && panel && place, "panel_voxel_view: null pointer");
  MUVO_CHECK_ARG(pad >= 0 && pad <= 64 && padbyte >= 0 && padbyte <= 255, "panel_voxel_view: pad %d outside 0..64 or pad byte %d outside 0..255", pad, padbyte);
  const MuvoTilePlace& p = *place;
  MUVO_CHECK_ARG(p.T > 0 && F % p.T == 0 && p.t0 >= 0 && p.t0 < (1 << 20) && p.T < (1 << 20), "panel_voxel_view: %d frames are no multiple of T = %d (or t0 %d < 0)",
                 F, p.T, p.t0);
  MUVO_CHECK_ARG(p.PH > 0 && p.PW > 0 && p.chan_stride >= (int64_t)p.PH * p.PW && p.sample_stride >= 3 * p.chan_stride,
                 "panel_voxel_view: panel %d x %d does not fit its strides (channel %lld, sample %lld, 3 channels)", p.PH, p.PW, (long long)p.chan_stride,
                 (long long)p.sample_stride);
  const int64_t b = F / p.T;
  MUVO_CHECK_ARG(panel_bytes >= (b - 1) * p.sample_stride + 2 * p.chan_stride + (int64_t)p.PH * p.PW, "panel_voxel_view: panel of %lld bytes is too small for %lld samples",
                 (long long)panel_bytes, (long long)b);
  const int T = R + 2 * pad;
  for (int s = p.t0; s < p.t0 + p.T; ++s) {
    const int64_t row0 = p.y0 + (int64_t)s * p.ystep, col0 = p.x0 + (int64_t)s * p.xstep + (s >= p.tsep ? p.sepw : 0);
    MUVO_CHECK_ARG(row0 >= 0 && col0 >= 0 && row0 + T <= p.PH && col0 + T <= p.PW, "panel_voxel_view: the %d x %d tile of step %d at (%lld, %lld) leaves the %d x %d panel",
                   T, T, s, (long long)row0, (long long)col0, p.PH, p.PW);
  }
  const long n = (long)T * T;
  hipLaunchKernelGGL(rc_view_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)F), dim3(256), 0, ST, rc_frames(grid, bricks, X, Y, Z), rays, R, palette, pad,
                     padbyte, p, panel);
  MUVO_CHECK_LAUNCH("panel_voxel_view");
  return MUVO_OK;
}

int64_t muvo_ray_iou_ws_doubles(int64_t F, int64_t R) { return vg_frames_ok(F) && vg_rays_ok(R) ? F * ((R + 255) / 256) * 2 : -1; }

int muvo_ray_iou_counts(const uint8_t* label, const uint64_t* label_bricks, const uint8_t* pred, const uint64_t* pred_bricks, int F, int C, int X, int Y,
                        int Z, const float* rays, int64_t R, float res, const float* thresholds, uint64_t* counts, double* ws, int64_t ws_doubles,
                        double* depth, void* stream) {
  if (int rc = rc_sizes("ray_iou_counts", F, X, Y, Z)) return rc;
  if (int rc = vg_check_classes("ray_iou_counts", C)) return rc;
  if (int rc = vg_check_rays("ray_iou_counts", R)) return rc;
  MUVO_CHECK_ARG(label && label_bricks && pred && pred_bricks && rays && thresholds && counts && ws && depth, "ray_iou_counts: null pointer");
  MUVO_CHECK_ARG(res > 0.f && thresholds[0] >= 0.f && thresholds[1] >= 0.f && thresholds[2] >= 0.f, "ray_iou_counts: resolution %g not positive or a negative threshold",
                 (double)res);
  MUVO_CHECK_ARG(ws_doubles >= muvo_ray_iou_ws_doubles(F, R) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)depth & 7) == 0 && ((uintptr_t)counts & 7) == 0,
                 "ray_iou_counts: workspace of %lld doubles, %lld needed (8-byte aligned)", (long long)ws_doubles, (long long)muvo_ray_iou_ws_doubles(F, R));
  const unsigned nb = (unsigned)((R + 255) / 256);
  hipLaunchKernelGGL(rc_iou_kernel, dim3(nb, (unsigned)F), dim3(256), 0, ST, rc_frames(label, label_bricks, X, Y, Z), rc_frames(pred, pred_bricks, X, Y, Z), rays,
                     (long)R, C, res, thresholds[0], thresholds[1], thresholds[2], (unsigned long long*)counts, ws);
  hipLaunchKernelGGL(rc_iou_sum_kernel, dim3(1), dim3(64), 0, ST, (const double*)ws, (long)nb * F, depth);
  MUVO_CHECK_LAUNCH("ray_iou_counts");
  return MUVO_OK;
}

}  // extern "C"
