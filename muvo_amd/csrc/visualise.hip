// Prediction panels on the device (muvo_amd/visualise.py): the image grids the reference's `visualise` (trainer.py:569-1007)
// assembles on the host from `.cpu()` copies of every output tensor - argmax, palette indexing, F.pad, torch.cat, rot90, numpy
// loops.  Here every tile of a panel is written straight from the model's tensors into a caller-allocated uint8 panel, at a
// position computed from (sample, time step): no class tensor, no float image and no padded copy exists in HBM.
//   tile kinds: float image, class logits (first maximum + palette), class labels (palette), constant, bird's-eye scatter of a
//   range view, action bars, top view of a voxel grid.
// Thread-to-pixel mapping of the tile kernels: a thread owns one 4-byte-aligned group of the PANEL row (not of the tile), so the
// interior of a tile row leaves as dword stores whatever the tile's origin - pads of 2, 3 and 5 pixels make most origins odd -
// and only the first and last group of a row, or a panel whose base / channel stride is not a multiple of 4, fall back to byte
// stores.  The source side of a group is four dword loads per plane at consecutive addresses: neighbouring lanes continue
// each other, the wave reads whole lines.  Rotated tiles (rot90 k = 1, the bird's-eye-view strip) let the lanes run along the
// output rows instead: consecutive lanes then read consecutive source columns, the (12 x smaller) write side takes the stride.
// Pure streaming: no atomics, every byte of a tile is written by exactly one thread (scatter: idempotent 255s), so the result
// is independent of the execution order.
#include <algorithm>

#include "common.h"

#define VIS_MAXC 16             // EXP_MAXC of export.hip

struct VisGeom {
  MuvoTilePlace p;
  int h, w;                     // source tile (unpadded, source orientation)
  int pad, padbyte, rot;
  int TH, TW, NG;               // padded tile in panel orientation; 4-byte groups per tile row (one more than TW / 4: misalignment)
  int nch, vec;                 // panel channels (1 or 3); vec: panel base is 4-byte aligned
};

// y = saturate(trunc(x * 255)): the rule of export.hip's exp_u8 (NaN and everything <= 0 -> 0, everything >= 255 -> 255)
__device__ __forceinline__ unsigned vis_u8(float x) {
  const float t = x * 255.0f;
  return !(t > 0.f) ? 0u : (t >= 255.f ? 255u : (unsigned)t);
}

__device__ __forceinline__ long vis_origin(const MuvoTilePlace& p, int f, int& row0, int& col0) {
  const int smp = f / p.T, t = p.t0 + f % p.T;
  row0 = p.y0 + t * p.ystep;
  col0 = p.x0 + t * p.xstep + (t >= p.tsep ? p.sepw : 0);
  return (long)smp * p.sample_stride;
}

// four bytes v (little endian) at byte offset a of the panel, those of `mask`: one dword store when all four are there and the
// address allows it
__device__ __forceinline__ void vis_put4(uint8_t* __restrict__ panel, long a, unsigned v, unsigned mask, int vec) {
  if (mask == 0xfu && vec && (a & 3) == 0) {
    *(uint32_t*)(panel + a) = v;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((mask >> k) & 1u) panel[a + k] = (uint8_t)(v >> (8 * k));
  }
}

// ---- pixel sources: rgb(f, i, j) = 0x00BBGGRR of source pixel (i, j) of frame f (grey sources: all three equal) -----------------
struct VisImageSrc {            // channels c0 .. c0 + n - 1 (n = 1 or 3) of (F, C, h, w) fp32
  const float* __restrict__ x;
  int C, c0, n, h, w;
  __device__ __forceinline__ unsigned rgb(const unsigned*, int f, int i, int j) const {
    const float* __restrict__ q = x + (((size_t)f * C + c0) * h + i) * w + j;
    const unsigned r = vis_u8(q[0]);
    if (n == 1) return r * 0x010101u;
    const size_t hw = (size_t)h * w;
    return r | (vis_u8(q[hw]) << 8) | (vis_u8(q[2 * hw]) << 16);
  }
};

struct VisLogitsSrc {           // (F, C, h, w) fp32: first maximum over C (strict >), then the palette
  const float* __restrict__ x;
  int C, h, w;
  __device__ __forceinline__ unsigned rgb(const unsigned* pal, int f, int i, int j) const {
    const size_t hw = (size_t)h * w;
    const float* __restrict__ q = x + (size_t)f * C * hw + (size_t)i * w + j;
    float b = q[0];
    unsigned cls = 0;
    for (int c = 1; c < C; ++c) {
      const float v = q[c * hw];
      if (v > b) { b = v; cls = c; }
    }
    return pal[cls];
  }
};

template <typename T>
struct VisLabelSrc {            // (F, h, w) uint8 / int64: the palette entry of the value's low byte
  const T* __restrict__ x;
  int h, w;
  __device__ __forceinline__ unsigned rgb(const unsigned* pal, int f, int i, int j) const {
    return pal[(unsigned)x[((size_t)f * h + i) * w + j] & 255u];
  }
};

struct VisConstSrc {
  unsigned v;
  __device__ __forceinline__ unsigned rgb(const unsigned*, int, int, int) const { return v; }
};

// action bar (trainer.py:679-706 without the text): tile (int(h/4), w + 10) all 255, the bar over rows [5, int(h/4) - 5) and
// columns [mid, mid + k) (v >= 0) or [mid + k, mid) (v < 0), k = (int)((float)(w / 2.0) * v), mid = int(w/2) + 5
struct VisBarSrc {
  const float* __restrict__ v;
  int bh, w, kind;              // bh = int(h/4); kind 0: throttle_brake (green / red), 1: steering (blue)
  __device__ __forceinline__ unsigned rgb(const unsigned*, int f, int i, int j) const {
    const float val = v[f];
    const float half = (float)(w / 2.0);
    float kf = half * val;
    kf = kf != kf ? 0.f : fminf(fmaxf(kf, -1.0e6f), 1.0e6f);          // NaN draws nothing; the clamp keeps the cast defined
    const int k = (int)kf, mid = w / 2 + 5;
    const bool pos = val >= 0.f;
    const int lo = pos ? mid : mid + k, hi = pos ? mid + k : mid;
    if (i >= 5 && i < bh - 5 && j >= lo && j < hi) return kind ? (200u << 16) : (pos ? (200u << 8) : 200u);
    return 0xffffffu;
  }
};

template <class Src, bool PAL>
__global__ void __launch_bounds__(256) vis_tile_kernel(Src s, VisGeom g, const uint8_t* __restrict__ palette, uint8_t* __restrict__ panel) {
  __shared__ unsigned pal[256];
  if (PAL) {
    const int t = threadIdx.x;
    pal[t] = palette[3 * t] | ((unsigned)palette[3 * t + 1] << 8) | ((unsigned)palette[3 * t + 2] << 16);
    __syncthreads();
  }
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int f = blockIdx.y;
  int i, j;
  if (g.rot) { i = (int)(idx % g.TH); j = (int)(idx / g.TH); } else { j = (int)(idx % g.NG); i = (int)(idx / g.NG); }
  if (i >= g.TH || j >= g.NG) return;
  int row0, col0;
  const long soff = vis_origin(g.p, f, row0, col0);
  const long A0 = soff + (long)(row0 + i) * g.p.PW + col0;              // first byte of this tile row, channel 0
  const long a = ((A0 >> 2) + j) << 2;
  unsigned r = 0, gg = 0, b = 0, mask = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long jj = a + k - A0;
    if (jj < 0 || jj >= g.TW) continue;
    const int pi = g.rot ? (int)jj : i, pj = g.rot ? g.TH - 1 - i : (int)jj;      // out[i][j] = in[j][Wp - 1 - i], Wp = TH
    const int si = pi - g.pad, sj = pj - g.pad;
    const unsigned c = (si >= 0 && si < g.h && sj >= 0 && sj < g.w) ? s.rgb(pal, f, si, sj) : (unsigned)g.padbyte * 0x010101u;
    mask |= 1u << k;
    r |= (c & 255u) << (8 * k);
    gg |= ((c >> 8) & 255u) << (8 * k);
    b |= ((c >> 16) & 255u) << (8 * k);
  }
  if (!mask) return;
  vis_put4(panel, a, r, mask, g.vec);
  if (g.nch == 3) {
    vis_put4(panel, a + g.p.chan_stride, gg, mask, g.vec);
    vis_put4(panel, a + 2 * g.p.chan_stride, b, mask, g.vec);
  }
}

// Range view (F, C, H, W) of scaled x, y, ..., d -> 255 on the three channels of pixel ((int)r, (int)c) of a 256 x 256 tile whose
// background the constant-tile kernel has written (pcd_xy_image, trainer.py:980-1007).  fp32 in this order, no contraction:
// X = x * 50, r = (-X) * 2.56 + 128; a point draws when D = d * 50 > 0 and 0 < r < 256 and 0 < c < 256 (all strict).
__global__ void __launch_bounds__(256) vis_scatter_kernel(const float* __restrict__ rv, int C, long HW, float scale, VisGeom g,
                                                          uint8_t* __restrict__ panel) {
  const int f = blockIdx.y;
  const float* __restrict__ q = rv + (size_t)f * C * HW;
  int row0, col0;
  const long base = vis_origin(g.p, f, row0, col0) + (long)(row0 + g.pad) * g.p.PW + col0 + g.pad;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long)gridDim.x * 256) {
    const float X = q[p] * scale, Y = q[HW + p] * scale, D = q[(size_t)(C - 1) * HW + p] * scale;
    const float r = (-X) * 2.56f + 128.0f, c = (-Y) * 2.56f + 128.0f;
    if (D > 0.f && 0.f < r && r < 256.f && 0.f < c && c < 256.f) {
      const long a = base + (long)(int)r * g.p.PW + (int)c;
      panel[a] = 255;
      panel[a + g.p.chan_stride] = 255;
      panel[a + 2 * g.p.chan_stride] = 255;
    }
  }
}

// Top view of a voxel grid (our own definition, see include/muvo_hip.h): L lanes (a power of two <= 64) share one column (x, y);
// a lane takes 4 consecutive z per round - one 16-byte load per class plane (logits) or one dword (uint8 grid) when `vec` - keeps
// the highest occupied z of its own, and a butterfly over the L lanes leaves the column's z* and class in every lane.  Lane 0
// writes the pixel; the border and the rest of the tile were written by the constant-tile kernel.
template <bool LOGITS>
__global__ void __launch_bounds__(256) vis_voxel_top_kernel(const void* __restrict__ src, int C, int X, int Y, int Z, int L, int vec,
                                                            const uint8_t* __restrict__ palette, VisGeom g, uint8_t* __restrict__ panel) {
  const int f = blockIdx.y, per = 256 / L, l = threadIdx.x % L;
  const long ncol = (long)X * Y;
  long col = (long)blockIdx.x * per + threadIdx.x / L;
  const bool live = col < ncol;
  if (!live) col = ncol - 1;                              // every lane stays in the butterfly
  unsigned key = 0;                                       // ((z << 8) | class) + 1 of the highest occupied voxel seen, 0: none
  for (int z0 = l * 4; z0 < Z; z0 += L * 4) {
    unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (LOGITS) {
      const size_t V = (size_t)ncol * Z;
      const float* __restrict__ q = (const float*)src + (size_t)f * C * V + (size_t)col * Z + z0;
      if (vec) {                                          // Z % 4 == 0: the four z exist
        f32x4 b = *(const f32x4*)q;
        for (int c = 1; c < C; ++c) {
          const f32x4 x = *(const f32x4*)(q + (size_t)c * V);
          if (x.x > b.x) { b.x = x.x; c0 = c; }
          if (x.y > b.y) { b.y = x.y; c1 = c; }
          if (x.z > b.z) { b.z = x.z; c2 = c; }
          if (x.w > b.w) { b.w = x.w; c3 = c; }
        }
      } else {
        const bool v1 = z0 + 1 < Z, v2 = z0 + 2 < Z, v3 = z0 + 3 < Z;
        float b0 = q[0], b1 = v1 ? q[1] : 0.f, b2 = v2 ? q[2] : 0.f, b3 = v3 ? q[3] : 0.f;
        for (int c = 1; c < C; ++c) {
          const float* __restrict__ qc = q + (size_t)c * V;
          const float x0 = qc[0];
          if (x0 > b0) { b0 = x0; c0 = c; }
          if (v1) { const float x = qc[1]; if (x > b1) { b1 = x; c1 = c; } }
          if (v2) { const float x = qc[2]; if (x > b2) { b2 = x; c2 = c; } }
          if (v3) { const float x = qc[3]; if (x > b3) { b3 = x; c3 = c; } }
        }
      }
    } else {
      const uint8_t* __restrict__ q = (const uint8_t*)src + ((size_t)f * ncol + col) * Z + z0;
      if (vec) {
        const uint32_t w = *(const uint32_t*)q;
        c0 = w & 255u; c1 = (w >> 8) & 255u; c2 = (w >> 16) & 255u; c3 = w >> 24;
      } else {
        c0 = q[0];
        if (z0 + 1 < Z) c1 = q[1];
        if (z0 + 2 < Z) c2 = q[2];
        if (z0 + 3 < Z) c3 = q[3];
      }
    }
    if (c0) key = (((unsigned)z0 << 8) | c0) + 1u;          // ascending z: a later hit replaces an earlier one
    if (c1) key = (((unsigned)(z0 + 1) << 8) | c1) + 1u;
    if (c2) key = (((unsigned)(z0 + 2) << 8) | c2) + 1u;
    if (c3) key = (((unsigned)(z0 + 3) << 8) | c3) + 1u;
  }
  for (int o = L >> 1; o > 0; o >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, o, 64));
  if (!live || l != 0) return;
  unsigned cr, cg, cb;
  if (key == 0) {
    cr = palette[0]; cg = palette[1]; cb = palette[2];
  } else {
    const unsigned cls = (key - 1u) & 255u, z = (key - 1u) >> 8;
    const unsigned s = 96u + (159u * z) / (unsigned)max(Z - 1, 1);
    cr = (palette[3 * cls] * s) / 255u; cg = (palette[3 * cls + 1] * s) / 255u; cb = (palette[3 * cls + 2] * s) / 255u;
  }
  const int x = (int)(col / Y), y = (int)(col % Y);
  int row0, col0;
  const long a = vis_origin(g.p, f, row0, col0) + (long)(row0 + g.pad + X - 1 - x) * g.p.PW + col0 + g.pad + y;
  panel[a] = (uint8_t)cr;
  panel[a + g.p.chan_stride] = (uint8_t)cg;
  panel[a + 2 * g.p.chan_stride] = (uint8_t)cb;
}

#define ST ((hipStream_t)stream)

// Everything a tile kernel may touch lies inside the panel: checked here for every frame, before any launch.
static int vis_geom(const char* who, int F, int h, int w, int pad, int padbyte, int rot, int nch, const uint8_t* panel, int64_t panel_bytes,
                    const MuvoTilePlace* pl, VisGeom& g) {
  MUVO_CHECK_ARG(panel && pl, "%s: null pointer (panel, place)", who);
  MUVO_CHECK_ARG(F > 0 && F <= 65535 && h > 0 && w > 0 && h <= 32768 && w <= 32768, "%s: bad sizes (F %d in 1..65535, tile %d x %d in 1..32768)",
                 who, F, h, w);
  MUVO_CHECK_ARG(pad >= 0 && pad <= 64 && padbyte >= 0 && padbyte <= 255, "%s: pad %d outside 0..64 or pad byte %d outside 0..255", who, pad,
                 padbyte);
  MUVO_CHECK_ARG(nch == 1 || nch == 3, "%s: %d panel channels (1 or 3)", who, nch);
  const MuvoTilePlace& p = *pl;
  MUVO_CHECK_ARG(p.T > 0 && F % p.T == 0 && p.t0 >= 0 && p.t0 < (1 << 20) && p.T < (1 << 20), "%s: %d frames are no multiple of T = %d (or t0 %d < 0)", who, F,
                 p.T, p.t0);
  MUVO_CHECK_ARG(p.PH > 0 && p.PW > 0 && p.chan_stride >= (int64_t)p.PH * p.PW && p.sample_stride >= nch * p.chan_stride,
                 "%s: panel %d x %d does not fit its strides (channel %lld, sample %lld, %d channels)", who, p.PH, p.PW,
                 (long long)p.chan_stride, (long long)p.sample_stride, nch);
  const int64_t b = F / p.T;
  MUVO_CHECK_ARG(panel_bytes >= (b - 1) * p.sample_stride + (nch - 1) * p.chan_stride + (int64_t)p.PH * p.PW,
                 "%s: panel of %lld bytes is too small for %lld samples", who, (long long)panel_bytes, (long long)b);
  g.p = p;
  g.h = h; g.w = w; g.pad = pad; g.padbyte = padbyte; g.rot = rot ? 1 : 0; g.nch = nch;
  const int Hp = h + 2 * pad, Wp = w + 2 * pad;
  g.TH = rot ? Wp : Hp;
  g.TW = rot ? Hp : Wp;
  g.NG = (g.TW + 3) / 4 + 1;
  g.vec = ((uintptr_t)panel & 3) == 0 ? 1 : 0;
  for (int t = p.t0; t < p.t0 + p.T; ++t) {
    const int64_t row0 = p.y0 + (int64_t)t * p.ystep, col0 = p.x0 + (int64_t)t * p.xstep + (t >= p.tsep ? p.sepw : 0);
    MUVO_CHECK_ARG(row0 >= 0 && col0 >= 0 && row0 + g.TH <= p.PH && col0 + g.TW <= p.PW,
                   "%s: the %d x %d tile of step %d at (%lld, %lld) leaves the %d x %d panel", who, g.TH, g.TW, t, (long long)row0,
                   (long long)col0, p.PH, p.PW);
  }
  return MUVO_OK;
}

template <class Src, bool PAL>
static void vis_launch(const Src& s, const VisGeom& g, int F, const uint8_t* palette, uint8_t* panel, hipStream_t st) {
  const long n = (long)g.TH * g.NG;
  hipLaunchKernelGGL((vis_tile_kernel<Src, PAL>), dim3((unsigned)((n + 255) / 256), (unsigned)F), dim3(256), 0, st, s, g, palette, panel);
}

extern "C" {

int muvo_panel_image(const float* src, int F, int C, int c0, int h, int w, int pad, int padbyte, int nch, uint8_t* panel, int64_t panel_bytes,
                     const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(src && (nch == 1 || nch == 3) && c0 >= 0 && C > 0 && c0 + nch <= C,
                 "panel_image: null source, or channels %d .. %d + %d outside the source's %d (1 or 3 panel channels)", c0, c0, nch, C);
  VisGeom g;
  if (int rc = vis_geom("panel_image", F, h, w, pad, padbyte, 0, nch, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisImageSrc, false>(VisImageSrc{src, C, c0, nch, h, w}, g, F, nullptr, panel, ST);
  MUVO_CHECK_LAUNCH("panel_image");
  return MUVO_OK;
}

int muvo_panel_logits(const float* src, int F, int C, int h, int w, const uint8_t* palette, int pad, int padbyte, int rotate, uint8_t* panel,
                      int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(src && palette, "panel_logits: null pointer (source, palette)");
  MUVO_CHECK_ARG(C >= 2 && C <= VIS_MAXC, "panel_logits: C = %d outside 2..%d", C, VIS_MAXC);
  VisGeom g;
  if (int rc = vis_geom("panel_logits", F, h, w, pad, padbyte, rotate, 3, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisLogitsSrc, true>(VisLogitsSrc{src, C, h, w}, g, F, palette, panel, ST);
  MUVO_CHECK_LAUNCH("panel_logits");
  return MUVO_OK;
}

int muvo_panel_labels(const void* src, int is_int64, int F, int h, int w, const uint8_t* palette, int pad, int padbyte, int rotate,
                      uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(src && palette, "panel_labels: null pointer (source, palette)");
  VisGeom g;
  if (int rc = vis_geom("panel_labels", F, h, w, pad, padbyte, rotate, 3, panel, panel_bytes, place, g)) return rc;
  if (is_int64)
    vis_launch<VisLabelSrc<int64_t>, true>(VisLabelSrc<int64_t>{(const int64_t*)src, h, w}, g, F, palette, panel, ST);
  else
    vis_launch<VisLabelSrc<uint8_t>, true>(VisLabelSrc<uint8_t>{(const uint8_t*)src, h, w}, g, F, palette, panel, ST);
  MUVO_CHECK_LAUNCH("panel_labels");
  return MUVO_OK;
}

int muvo_panel_fill(int F, int h, int w, int value, int pad, int padbyte, int nch, uint8_t* panel, int64_t panel_bytes,
                    const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(value >= 0 && value <= 255, "panel_fill: value %d outside 0..255", value);
  VisGeom g;
  if (int rc = vis_geom("panel_fill", F, h, w, pad, padbyte, 0, nch, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisConstSrc, false>(VisConstSrc{(unsigned)value * 0x010101u}, g, F, nullptr, panel, ST);
  MUVO_CHECK_LAUNCH("panel_fill");
  return MUVO_OK;
}

int muvo_panel_bars(const float* values, int kind, int F, int h, int w, uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place,
                    void* stream) {
  MUVO_CHECK_ARG(values && (kind == 0 || kind == 1), "panel_bars: null values or kind %d (0 throttle_brake, 1 steering)", kind);
  MUVO_CHECK_ARG(h >= 4, "panel_bars: image height %d below 4 (the bar is int(h / 4) rows)", h);
  VisGeom g;
  if (int rc = vis_geom("panel_bars", F, h / 4, w + 10, 0, 0, 0, 3, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisBarSrc, false>(VisBarSrc{values, h / 4, w, kind}, g, F, nullptr, panel, ST);
  MUVO_CHECK_LAUNCH("panel_bars");
  return MUVO_OK;
}

int muvo_panel_scatter(const float* range_view, int F, int C, int H, int W, float scale, int pad, int padbyte, uint8_t* panel,
                       int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(range_view && C >= 3 && C <= 64 && H > 0 && W > 0, "panel_scatter: null source or bad sizes (C %d in 3..64, %d x %d)", C, H, W);
  VisGeom g;
  if (int rc = vis_geom("panel_scatter", F, 256, 256, pad, padbyte, 0, 3, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisConstSrc, false>(VisConstSrc{0u}, g, F, nullptr, panel, ST);
  const long HW = (long)H * W;
  hipLaunchKernelGGL(vis_scatter_kernel, dim3((unsigned)std::min<long>((HW + 255) / 256, 1024), (unsigned)F), dim3(256), 0, ST, range_view, C, HW,
                     scale, g, panel);
  MUVO_CHECK_LAUNCH("panel_scatter");
  return MUVO_OK;
}

static int vis_voxel_top(const char* who, const void* src, bool logits, int F, int C, int X, int Y, int Z, const uint8_t* palette, int pad,
                         int padbyte, uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, hipStream_t st) {
  MUVO_CHECK_ARG(src && palette, "%s: null pointer (source, palette)", who);
  MUVO_CHECK_ARG(Z > 0 && Z <= 65536 && X > 0 && Y > 0 && (int64_t)X * Y * Z < (1ll << 31), "%s: grid %d %d %d (Z in 1..65536, below 2^31 voxels)", who,
                 X, Y, Z);
  VisGeom g;
  if (int rc = vis_geom(who, F, X, Y, pad, padbyte, 0, 3, panel, panel_bytes, place, g)) return rc;
  vis_launch<VisConstSrc, false>(VisConstSrc{(unsigned)padbyte * 0x010101u}, g, F, nullptr, panel, st);
  int L = 1;
  while (L < 64 && L * 4 < Z) L <<= 1;
  const int vec = (Z % 4 == 0 && ((uintptr_t)src & (logits ? 15 : 3)) == 0) ? 1 : 0;
  const long ncol = (long)X * Y;
  const dim3 grid((unsigned)((ncol + 256 / L - 1) / (256 / L)), (unsigned)F);
  if (logits)
    hipLaunchKernelGGL(vis_voxel_top_kernel<true>, grid, dim3(256), 0, st, src, C, X, Y, Z, L, vec, palette, g, panel);
  else
    hipLaunchKernelGGL(vis_voxel_top_kernel<false>, grid, dim3(256), 0, st, src, C, X, Y, Z, L, vec, palette, g, panel);
  MUVO_CHECK_LAUNCH(who);
  return MUVO_OK;
}

int muvo_panel_voxel_top_logits(const float* logits, int F, int C, int X, int Y, int Z, const uint8_t* palette, int pad, int padbyte,
                                uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(C >= 2 && C <= VIS_MAXC, "panel_voxel_top_logits: C = %d outside 2..%d", C, VIS_MAXC);
  return vis_voxel_top("panel_voxel_top_logits", logits, true, F, C, X, Y, Z, palette, pad, padbyte, panel, panel_bytes, place, ST);
}

int muvo_panel_voxel_top_grid(const uint8_t* grid, int F, int X, int Y, int Z, const uint8_t* palette, int pad, int padbyte, uint8_t* panel,
                              int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  return vis_voxel_top("panel_voxel_top_grid", grid, false, F, 0, X, Y, Z, palette, pad, padbyte, panel, panel_bytes, place, ST);
}

}  // extern "C"
