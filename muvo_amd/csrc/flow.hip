// Dense optical flow between camera frames (muvo_amd/flow.py: the `_flow` panel and the flow metric): Farneback's two-frame
// method (polynomial expansion, SCIA 2003) as the reference asks cv2 for it (trainer.py:1009-1020: pyramid scale 0.5, 3 levels,
// window 15, 3 iterations, neighbourhood 5, sigma 1.2, box window).  The exact definition - ours, not cv2's - stands in
// include/muvo_hip.h; tests/flow_reference.py restates it in numpy.
// All frame pairs of a call run in every launch (grid z = the pair); per level:
//   flow_poly_kernel     separable 11-tap stencil: a 26 x 74 LDS tile (16 x 64 pixels + 5 halo), three vertical moments per
//                        column, then the six horizontal sums and the five coefficients of a pixel from one read of the tile
//   flow_iterate_kernel  x 3: the matrix update of a 30 x 46 patch (16 x 32 pixels + 7 halo: the second frame's coefficients
//                        sampled bilinearly at x + d) into LDS, the 15 x 15 box as vertical then horizontal sums, the closed
//                        2 x 2 solve; the five products never reach HBM
// and between levels one launch each for the blurred + resized image and the resized flow.  fp32 throughout, built without
// contraction, every sum in a fixed ascending order that does not depend on the tiling and no atomics: a pair's result is
// bit-reproducible and independent of the other pairs of the call.  The pair indices are validated on the host and travel
// as kernel arguments (no device memory, no copy): at most FLOW_MAXP pairs per call.
#include <algorithm>
#include <cmath>

#include "common.h"

#define FLOW_MAXP 64
#define FLOW_PART 64            // workgroups per pair of the reductions (min / max, endpoint error)
#define ST ((hipStream_t)stream)

struct FlowPairs { int a[FLOW_MAXP], b[FLOW_MAXP]; };
struct FlowBlurK { float t[9]; int n; };
struct FlowPolyK { float t0[11], t1[11], t2[11], kb, ka0, ka1, ka2, kxy; };

__device__ __forceinline__ int flow_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned flow_u8(float x) {          // the rule of muvo_image_u8
  const float t = x * 255.0f;
  return !(t > 0.f) ? 0u : (t >= 255.f ? 255u : (unsigned)t);
}

// grey level 0 of both frames of every pair: ws[p][which][N]
__global__ void __launch_bounds__(256) flow_grey_kernel(const float* __restrict__ fa, const float* __restrict__ fb, FlowPairs pr, long N,
                                                        float* __restrict__ ws, long stride) {
  const int p = blockIdx.z, which = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int f = which ? pr.b[p] : pr.a[p];
  float g = 255.0f;
  if (f >= 0) {
    const float* __restrict__ q = (which ? fb : fa) + (size_t)f * 3 * N + i;
    g = (float)((4899u * flow_u8(q[0]) + 9617u * flow_u8(q[N]) + 1868u * flow_u8(q[2 * N]) + 8192u) >> 14);
  }
  ws[(size_t)p * stride + (size_t)which * N + i] = g;
}

// source coordinate of a bilinear resize with half-pixel centres, clamped
__device__ __forceinline__ void flow_src(int o, float s, int n_in, int& i0, int& i1, float& f) {
  float c = ((float)o + 0.5f) * s - 0.5f;
  c = fminf(fmaxf(c, 0.0f), (float)(n_in - 1));
  i0 = (int)floorf(c);
  i1 = min(i0 + 1, n_in - 1);
  f = c - (float)i0;
}

__device__ __forceinline__ float flow_blurred(const float* __restrict__ g, int h, int w, int y, int x, const FlowBlurK& k) {
  const int r = k.n >> 1;
  float acc = 0.f;
  for (int j = 0; j < k.n; ++j) {
    const float* __restrict__ row = g + (size_t)flow_clamp(y + j - r, h - 1) * w;
    float a = k.t[0] * row[flow_clamp(x - r, w - 1)];
    for (int i = 1; i < k.n; ++i) a += k.t[i] * row[flow_clamp(x + i - r, w - 1)];
    const float term = k.t[j] * a;
    acc = j ? acc + term : term;
  }
  return acc;
}

// level k > 0 of both frames: the level-0 grey image blurred (along x, then along y) and resized to hk x wk
__global__ void __launch_bounds__(256) flow_pyramid_kernel(const float* __restrict__ ws, long stride, int h, int w, int hk, int wk, FlowBlurK k,
                                                           float* __restrict__ out) {
  const int p = blockIdx.z, which = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)hk * wk) return;
  const int y = (int)(i / wk), x = (int)(i % wk);
  const float* __restrict__ g = ws + (size_t)p * stride + (size_t)which * h * w;
  int y0, y1, x0, x1;
  float fy, fx;
  flow_src(y, (float)h / (float)hk, h, y0, y1, fy);
  flow_src(x, (float)w / (float)wk, w, x0, x1, fx);
  const float v00 = flow_blurred(g, h, w, y0, x0, k), v01 = flow_blurred(g, h, w, y0, x1, k);
  const float v10 = flow_blurred(g, h, w, y1, x0, k), v11 = flow_blurred(g, h, w, y1, x1, k);
  const float top = (1.0f - fx) * v00 + fx * v01, bot = (1.0f - fx) * v10 + fx * v11;
  out[(size_t)p * stride + (size_t)which * hk * wk + i] = (1.0f - fy) * top + fy * bot;
}

// the flow of the coarser level resized to hk x wk and doubled (src == nullptr: the coarsest level starts from zero)
__global__ void __launch_bounds__(256) flow_upsample_kernel(const float* __restrict__ src, int hc, int wc, float* __restrict__ dst, int hk, int wk,
                                                            long stride) {
  const int p = blockIdx.z, c = blockIdx.y;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)hk * wk) return;
  float v = 0.f;
  if (src) {
    const int y = (int)(i / wk), x = (int)(i % wk);
    const float* __restrict__ g = src + (size_t)p * stride + (size_t)c * hc * wc;
    int y0, y1, x0, x1;
    float fy, fx;
    flow_src(y, (float)hc / (float)hk, hc, y0, y1, fy);
    flow_src(x, (float)wc / (float)wk, wc, x0, x1, fx);
    const float top = (1.0f - fx) * g[(size_t)y0 * wc + x0] + fx * g[(size_t)y0 * wc + x1];
    const float bot = (1.0f - fx) * g[(size_t)y1 * wc + x0] + fx * g[(size_t)y1 * wc + x1];
    v = ((1.0f - fy) * top + fy * bot) * 2.0f;
  }
  dst[(size_t)p * stride + (size_t)c * hk * wk + i] = v;
}

#define PT_H 16
#define PT_W 64
#define PT_LW (PT_W + 10)
// polynomial expansion of both frames: img[p][which][h*w] -> R[p][which][5][h*w] = b_x, b_y, A_xx, A_yy, A_xy
__global__ void __launch_bounds__(256) flow_poly_kernel(const float* __restrict__ img, float* __restrict__ R, long stride, int h, int w,
                                                        FlowPolyK k) {
  __shared__ float in[PT_H + 10][PT_LW];
  __shared__ float v[3][PT_H][PT_LW];
  const int p = blockIdx.z >> 1, which = blockIdx.z & 1, tid = threadIdx.x;
  const int y0 = blockIdx.y * PT_H, x0 = blockIdx.x * PT_W;
  const long N = (long)h * w;
  const float* __restrict__ g = img + (size_t)p * stride + (size_t)which * N;
  for (int i = tid; i < (PT_H + 10) * PT_LW; i += 256) {
    const int ty = i / PT_LW, tx = i % PT_LW;
    in[ty][tx] = g[(size_t)flow_clamp(y0 + ty - 5, h - 1) * w + flow_clamp(x0 + tx - 5, w - 1)];
  }
  __syncthreads();
  for (int i = tid; i < PT_H * PT_LW; i += 256) {
    const int r = i / PT_LW, c = i % PT_LW;
    float f = in[r][c];
    float s0 = k.t0[0] * f, s1 = k.t1[0] * f, s2 = k.t2[0] * f;
#pragma unroll
    for (int j = 1; j < 11; ++j) {
      f = in[r + j][c];
      s0 += k.t0[j] * f;
      s1 += k.t1[j] * f;
      s2 += k.t2[j] * f;
    }
    v[0][r][c] = s0;
    v[1][r][c] = s1;
    v[2][r][c] = s2;
  }
  __syncthreads();
  float* __restrict__ out = R + (size_t)p * stride + (size_t)which * 5 * N;
#pragma unroll
  for (int q = 0; q < PT_H * PT_W / 256; ++q) {
    const int px = tid + 256 * q, r = px / PT_W, c = px % PT_W;
    const int y = y0 + r, x = x0 + c;
    if (y >= h || x >= w) continue;
    float a = v[0][r][c], b = v[1][r][c], d = v[2][r][c];
    float m00 = k.t0[0] * a, m10 = k.t1[0] * a, m20 = k.t2[0] * a, m01 = k.t0[0] * b, m11 = k.t1[0] * b, m02 = k.t0[0] * d;
#pragma unroll
    for (int i = 1; i < 11; ++i) {
      a = v[0][r][c + i]; b = v[1][r][c + i]; d = v[2][r][c + i];
      m00 += k.t0[i] * a;
      m10 += k.t1[i] * a;
      m20 += k.t2[i] * a;
      m01 += k.t0[i] * b;
      m11 += k.t1[i] * b;
      m02 += k.t0[i] * d;
    }
    const size_t o = (size_t)y * w + x;
    out[o] = k.kb * m10;
    out[N + o] = k.kb * m01;
    out[2 * N + o] = k.ka0 * m00 + k.ka1 * m20 + k.ka2 * m02;
    out[3 * N + o] = k.ka0 * m00 + k.ka2 * m20 + k.ka1 * m02;
    out[4 * N + o] = k.kxy * m11;
  }
}

__device__ __forceinline__ float flow_border(int i, int n) {
  const int k = min(i, n - 1 - i);
  return k < 2 ? 0.14f : (k < 5 ? 0.4472f : 1.0f);
}

#define IT_H 16
#define IT_W 32
#define IT_LH (IT_H + 14)
#define IT_LW (IT_W + 14)
// one iteration: R[p][2][5][N], flow din[p][2][N] -> dout[p * out_stride][2][N]
__global__ void __launch_bounds__(256) flow_iterate_kernel(const float* __restrict__ R, const float* __restrict__ din, long stride, int h, int w,
                                                           float* __restrict__ dout, long out_stride) {
  __shared__ float M[5][IT_LH][IT_LW];
  __shared__ float V[5][IT_H][IT_LW];
  const int p = blockIdx.z, tid = threadIdx.x;
  const int y0 = blockIdx.y * IT_H, x0 = blockIdx.x * IT_W;
  const long N = (long)h * w;
  const float* __restrict__ R0 = R + (size_t)p * stride;
  const float* __restrict__ R1 = R0 + 5 * N;
  const float* __restrict__ d = din + (size_t)p * stride;
  for (int i = tid; i < IT_LH * IT_LW; i += 256) {
    const int ty = i / IT_LW, tx = i % IT_LW;
    const int y = flow_clamp(y0 + ty - 7, h - 1), x = flow_clamp(x0 + tx - 7, w - 1);     // replicated border
    const size_t o = (size_t)y * w + x;
    const float dx = d[o], dy = d[N + o];
    const float fx = (float)x + dx, fy = (float)y + dy;
    float axx = R0[2 * N + o], ayy = R0[3 * N + o], axy = R0[4 * N + o], dbx = 0.f, dby = 0.f;
    if (fx >= 0.f && fx < (float)(w - 1) && fy >= 0.f && fy < (float)(h - 1)) {
      const int x1 = (int)floorf(fx), y1 = (int)floorf(fy);
      const float a = fx - (float)x1, b = fy - (float)y1;
      const float w00 = (1.0f - a) * (1.0f - b), w01 = a * (1.0f - b), w10 = (1.0f - a) * b, w11 = a * b;
      const size_t o00 = (size_t)y1 * w + x1, o01 = o00 + 1, o10 = o00 + w, o11 = o10 + 1;      // x1 + 1 <= w - 1, y1 + 1 <= h - 1
      float s[5];
#pragma unroll
      for (int c = 0; c < 5; ++c) {
        const float* __restrict__ q = R1 + c * N;
        s[c] = w00 * q[o00] + w01 * q[o01] + w10 * q[o10] + w11 * q[o11];
      }
      dbx = (R0[o] - s[0]) * 0.5f;
      dby = (R0[N + o] - s[1]) * 0.5f;
      axx = (axx + s[2]) * 0.5f;
      ayy = (ayy + s[3]) * 0.5f;
      axy = (axy + s[4]) * 0.5f;
    }
    float bx = dbx + (axx * dx + axy * dy), by = dby + (axy * dx + ayy * dy);
    const float sc = flow_border(y, h) * flow_border(x, w);
    axx *= sc; ayy *= sc; axy *= sc; bx *= sc; by *= sc;
    M[0][ty][tx] = axx * axx + axy * axy;
    M[1][ty][tx] = axy * (axx + ayy);
    M[2][ty][tx] = ayy * ayy + axy * axy;
    M[3][ty][tx] = axx * bx + axy * by;
    M[4][ty][tx] = axy * bx + ayy * by;
  }
  __syncthreads();
  for (int i = tid; i < IT_H * IT_LW; i += 256) {
    const int r = i / IT_LW, c = i % IT_LW;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float s = M[k][r][c];
#pragma unroll
      for (int j = 1; j < 15; ++j) s += M[k][r + j][c];
      V[k][r][c] = s;
    }
  }
  __syncthreads();
  float* __restrict__ o = dout + (size_t)p * out_stride;
#pragma unroll
  for (int q = 0; q < IT_H * IT_W / 256; ++q) {
    const int px = tid + 256 * q, r = px / IT_W, c = px % IT_W;
    const int y = y0 + r, x = x0 + c;
    if (y >= h || x >= w) continue;
    float g[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      float s = V[k][r][c];
#pragma unroll
      for (int i = 1; i < 15; ++i) s += V[k][r][c + i];
      g[k] = s * (float)(1.0 / 225.0);
    }
    const float idet = 1.0f / (g[0] * g[2] - g[1] * g[1] + 1e-3f);
    o[(size_t)y * w + x] = (g[2] * g[3] - g[1] * g[4]) * idet;
    o[N + (size_t)y * w + x] = (g[0] * g[4] - g[1] * g[3]) * idet;
  }
}

// ---- colour coding -----------------------------------------------------------------------------------------------------------
// per pair FLOW_PART x (min, max) of the flow magnitude; min / max do not depend on the order
__global__ void __launch_bounds__(256) flow_minmax_kernel(const float* __restrict__ flow, long N, float* __restrict__ part) {
  __shared__ float red[2][4];
  const int p = blockIdx.y;
  const float* __restrict__ f = flow + (size_t)p * 2 * N;
  float mn = INFINITY, mx = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)FLOW_PART * 256) {
    const float dx = f[i], dy = f[N + i];
    const float m = sqrtf(dx * dx + dy * dy);
    mn = fminf(mn, m);
    mx = fmaxf(mx, m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = mn; red[1][threadIdx.x >> 6] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* __restrict__ q = part + ((size_t)p * FLOW_PART + blockIdx.x) * 2;
    q[0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    q[1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

// value 255, hue in units of 2 degrees, in integers, rounded to nearest -> 0x00BBGGRR
__device__ __forceinline__ unsigned flow_hsv(int hue, int sat) {
  const int i = hue / 30, r = hue % 30;
  const unsigned v = 255u, pp = 255u - sat, q = 255u - (2u * sat * r + 30u) / 60u, t = 255u - (2u * sat * (30 - r) + 30u) / 60u;
  unsigned R, G, B;
  switch (i) {
    case 0: R = v; G = t; B = pp; break;
    case 1: R = q; G = v; B = pp; break;
    case 2: R = pp; G = v; B = t; break;
    case 3: R = pp; G = q; B = v; break;
    case 4: R = t; G = pp; B = v; break;
    default: R = v; G = pp; B = q; break;
  }
  return R | (G << 8) | (B << 16);
}

// a thread owns two horizontally adjacent pixels of the padded tile; tile columns start on even panel columns (checked by the
// entry), so with an even panel base the pair is one 2-byte store per channel
__global__ void __launch_bounds__(256) flow_colour_kernel(const float* __restrict__ flow, const float* __restrict__ part, int h, int w, int pad,
                                                          int padbyte, MuvoTilePlace pl, int vec, uint8_t* __restrict__ panel) {
  __shared__ float lim[2];
  const int p = blockIdx.y;
  if (threadIdx.x < 64) {
    float mn = part[((size_t)p * FLOW_PART + threadIdx.x) * 2], mx = part[((size_t)p * FLOW_PART + threadIdx.x) * 2 + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (threadIdx.x == 0) { lim[0] = mn; lim[1] = mx; }
  }
  __syncthreads();
  const float mn = lim[0], mx = lim[1];
  const int TH = h + 2 * pad, TW = w + 2 * pad, NG = (TW + 1) / 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int i = (int)(idx / NG), j = (int)(idx % NG) * 2;
  if (i >= TH) return;
  const int smp = p / pl.T, t = pl.t0 + p % pl.T;
  const int row0 = pl.y0 + t * pl.ystep, col0 = pl.x0 + t * pl.xstep + (t >= pl.tsep ? pl.sepw : 0);
  const long a = (long)smp * pl.sample_stride + (long)(row0 + i) * pl.PW + col0 + j;
  const long N = (long)h * w;
  const float* __restrict__ f = flow + (size_t)p * 2 * N;
  unsigned c[2] = {0u, 0u};
  const int n = j + 1 < TW ? 2 : 1;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int si = i - pad, sj = j + k - pad;
    if (k >= n) continue;
    if (si < 0 || si >= h || sj < 0 || sj >= w) { c[k] = (unsigned)padbyte * 0x010101u; continue; }
    const float dx = f[(size_t)si * w + sj], dy = f[N + (size_t)si * w + sj];
    const float mag = sqrtf(dx * dx + dy * dy);
    float ang = atan2f(dy, dx) * (float)(180.0 / 3.14159265358979323846);
    if (ang < 0.f) ang += 360.0f;
    const int hue = min(max((int)(ang * 0.5f), 0), 179);
    const int sat = mx > mn ? min(max((int)((mag - mn) * 255.0f / (mx - mn)), 0), 255) : 0;
    c[k] = flow_hsv(hue, sat);
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const long ac = a + ch * pl.chan_stride;
    const unsigned b0 = (c[0] >> (8 * ch)) & 255u;
    if (n == 2) {
      const unsigned b1 = (c[1] >> (8 * ch)) & 255u;
      if (vec && (ac & 1) == 0) {
        *(uint16_t*)(panel + ac) = (uint16_t)(b0 | (b1 << 8));
      } else {
        panel[ac] = (uint8_t)b0;
        panel[ac + 1] = (uint8_t)b1;
      }
    } else {
      panel[ac] = (uint8_t)b0;
    }
  }
}

// ---- endpoint error ----------------------------------------------------------------------------------------------------------
// per pair and workgroup three fp64 sums over the pixels at least 5 from the border: |a - b|, |a|, 1
__global__ void __launch_bounds__(256) flow_epe_kernel(const float* __restrict__ fa, const float* __restrict__ fb, int h, int w, double* __restrict__ part) {
  __shared__ double red[3][4];
  const int p = blockIdx.y, ih = h - 10, iw = w - 10;
  const long N = (long)h * w, n = (long)ih * iw;
  const float* __restrict__ a = fa + (size_t)p * 2 * N;
  const float* __restrict__ b = fb + (size_t)p * 2 * N;
  double s[3] = {0.0, 0.0, 0.0};
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)FLOW_PART * 256) {
    const size_t o = (size_t)(5 + i / iw) * w + 5 + i % iw;
    const float ax = a[o], ay = a[N + o], ex = ax - b[o], ey = ay - b[N + o];
    s[0] += (double)sqrtf(ex * ex + ey * ey);
    s[1] += (double)sqrtf(ax * ax + ay * ay);
    s[2] += 1.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = wave_sum_d(s[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 3) part[((size_t)p * FLOW_PART + blockIdx.x) * 3 + threadIdx.x] =
      ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// one wave: lane l adds the sums of workgroup l over the pairs in order, the lanes are added by a fixed butterfly, acc[k] += total
__global__ void __launch_bounds__(64) flow_epe_sum_kernel(const double* __restrict__ part, int P, double* __restrict__ acc) {
  for (int k = 0; k < 3; ++k) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += part[((size_t)p * FLOW_PART + threadIdx.x) * 3 + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) acc[k] += s;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int flow_levels(int h, int w) {
  int n = 3;
  while (n > 1 && std::min(h, w) * std::pow(0.5, n - 1) < 32.0) --n;
  return n;
}
static int flow_level_size(int n, int k) { return (n + ((1 << k) >> 1)) >> k; }

static void flow_gauss(double sigma, int n, double* g) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = i - n / 2;
    g[i] = std::exp(-x * x / (2.0 * sigma * sigma));
    s += g[i];
  }
  for (int i = 0; i < n; ++i) g[i] /= s;
}

// the taps and the rows of the inverse 6 x 6 normal matrix (basis 1, x, y, x^2, y^2, xy) the expansion needs, in float64
static FlowPolyK flow_poly_constants() {
  double g[11], G[6][12];
  flow_gauss(1.2, 11, g);
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 12; ++j) G[i][j] = j == i + 6 ? 1.0 : 0.0;
  for (int iy = 0; iy < 11; ++iy)
    for (int ix = 0; ix < 11; ++ix) {
      const double x = ix - 5, y = iy - 5, phi[6] = {1.0, x, y, x * x, y * y, x * y}, wgt = g[iy] * g[ix];
      for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) G[i][j] += wgt * phi[i] * phi[j];
    }
  for (int c = 0; c < 6; ++c) {                   // Gauss-Jordan with partial pivoting on [G | I]
    int piv = c;
    for (int r = c + 1; r < 6; ++r)
      if (std::fabs(G[r][c]) > std::fabs(G[piv][c])) piv = r;
    for (int j = 0; j < 12; ++j) std::swap(G[c][j], G[piv][j]);
    const double d = G[c][c];
    for (int j = 0; j < 12; ++j) G[c][j] /= d;
    for (int r = 0; r < 6; ++r) {
      if (r == c) continue;
      const double f = G[r][c];
      for (int j = 0; j < 12; ++j) G[r][j] -= f * G[c][j];
    }
  }
  FlowPolyK k;
  for (int i = 0; i < 11; ++i) {
    const double x = i - 5;
    k.t0[i] = (float)g[i];
    k.t1[i] = (float)(g[i] * x);
    k.t2[i] = (float)(g[i] * x * x);
  }
  k.kb = (float)G[1][7];
  k.ka0 = (float)G[3][6];
  k.ka1 = (float)G[3][9];
  k.ka2 = (float)G[3][10];
  k.kxy = (float)(G[5][11] / 2.0);
  return k;
}

static int64_t flow_pair_floats(int h, int w) {
  const int64_t N = (int64_t)h * w, N1 = (int64_t)flow_level_size(h, 1) * flow_level_size(w, 1);
  return 2 * N + 2 * N1 + 10 * N + 4 * N;         // grey, level image, coefficients, two flow fields
}

static int flow_sizes(const char* who, int64_t P, int h, int w) {
  MUVO_CHECK_ARG(P >= 1 && P <= FLOW_MAXP, "%s: %lld pairs outside 1..%d", who, (long long)P, FLOW_MAXP);
  MUVO_CHECK_ARG(h >= 16 && w >= 16 && h <= 8192 && w <= 8192, "%s: frames of %d x %d (16..8192 on both axes)", who, h, w);
  return MUVO_OK;
}

extern "C" {

int64_t muvo_flow_max_pairs(void) { return FLOW_MAXP; }

int64_t muvo_flow_workspace_bytes(int64_t P, int h, int w) {
  if (P < 1 || P > FLOW_MAXP || h < 16 || w < 16 || h > 8192 || w > 8192) return -1;
  return P * flow_pair_floats(h, w) * (int64_t)sizeof(float);
}

int muvo_flow_farneback(const float* frames_a, int64_t Fa, const float* frames_b, int64_t Fb, int h, int w, const int32_t* pairs_a,
                        const int32_t* pairs_b, int64_t P, void* ws, int64_t ws_bytes, float* flow, void* stream) {
  if (int rc = flow_sizes("flow_farneback", P, h, w)) return rc;
  MUVO_CHECK_ARG(frames_a && frames_b && pairs_a && pairs_b && ws && flow, "flow_farneback: null pointer");
  MUVO_CHECK_ARG(ws_bytes >= muvo_flow_workspace_bytes(P, h, w), "flow_farneback: workspace of %lld bytes, %lld needed", (long long)ws_bytes,
                 (long long)muvo_flow_workspace_bytes(P, h, w));
  MUVO_CHECK_ARG(((uintptr_t)ws & 3) == 0, "flow_farneback: workspace not 4-byte aligned");
  FlowPairs pr;
  for (int64_t p = 0; p < P; ++p) {
    MUVO_CHECK_ARG(pairs_a[p] >= -1 && pairs_a[p] < Fa && pairs_b[p] >= -1 && pairs_b[p] < Fb,
                   "flow_farneback: pair %lld = (%d, %d) outside its stacks of %lld and %lld frames (-1: a white frame)", (long long)p, pairs_a[p],
                   pairs_b[p], (long long)Fa, (long long)Fb);
    pr.a[p] = pairs_a[p];
    pr.b[p] = pairs_b[p];
  }
  static const FlowPolyK pk = flow_poly_constants();
  const long N = (long)h * w, stride = (long)flow_pair_floats(h, w);
  const long N1 = (long)flow_level_size(h, 1) * flow_level_size(w, 1);
  float* G0 = (float*)ws;                 // [p][2][N]
  float* I = G0 + 2 * N;                  // [p][2][Nk]
  float* R = I + 2 * N1;                  // [p][2][5][Nk]
  float* F[2] = {R + 10 * N, R + 12 * N}; // [p][2][Nk]
  const unsigned Pz = (unsigned)P;
  hipLaunchKernelGGL(flow_grey_kernel, dim3(cdiv(N, 256), 2, Pz), dim3(256), 0, ST, frames_a, frames_b, pr, N, G0, stride);
  const int L = flow_levels(h, w);
  int cur = 0, hc = 0, wc = 0;
  for (int k = L - 1; k >= 0; --k) {
    const int hk = flow_level_size(h, k), wk = flow_level_size(w, k);
    const long Nk = (long)hk * wk;
    const float* img = G0;
    if (k > 0) {
      FlowBlurK bk;
      const double sigma = (std::pow(2.0, k) - 1.0) / 2.0;
      bk.n = std::max((int)std::floor(5.0 * sigma + 0.5) | 1, 3);
      double g[9];
      flow_gauss(sigma, bk.n, g);
      for (int i = 0; i < 9; ++i) bk.t[i] = i < bk.n ? (float)g[i] : 0.f;
      hipLaunchKernelGGL(flow_pyramid_kernel, dim3(cdiv(Nk, 256), 2, Pz), dim3(256), 0, ST, G0, stride, h, w, hk, wk, bk, I);
      img = I;
    }
    // the start of the level: zero, or the coarser level's flow (in F[cur]) resized into F[1 - cur]
    const bool first = k == L - 1;
    hipLaunchKernelGGL(flow_upsample_kernel, dim3(cdiv(Nk, 256), 2, Pz), dim3(256), 0, ST, first ? nullptr : F[cur], hc, wc, F[1 - cur], hk, wk, stride);
    cur = 1 - cur;
    hipLaunchKernelGGL(flow_poly_kernel, dim3(cdiv(wk, PT_W), cdiv(hk, PT_H), 2 * Pz), dim3(256), 0, ST, img, R, stride, hk, wk, pk);
    for (int it = 0; it < 3; ++it) {
      const bool last = k == 0 && it == 2;
      hipLaunchKernelGGL(flow_iterate_kernel, dim3(cdiv(wk, IT_W), cdiv(hk, IT_H), Pz), dim3(256), 0, ST, R, F[cur], stride, hk, wk,
                         last ? flow : F[1 - cur], last ? 2 * N : stride);
      cur = 1 - cur;
    }
    hc = hk;
    wc = wk;
  }
  MUVO_CHECK_LAUNCH("flow_farneback");
  return MUVO_OK;
}

int64_t muvo_flow_colour_ws_bytes(int64_t P) { return P < 1 ? -1 : P * FLOW_PART * 2 * (int64_t)sizeof(float); }

int muvo_flow_colour(const float* flow, int64_t P, int h, int w, void* ws, int64_t ws_bytes, int pad, int padbyte, uint8_t* panel,
                     int64_t panel_bytes, const MuvoTilePlace* place, void* stream) {
  MUVO_CHECK_ARG(P >= 1 && P <= 65535, "flow_colour: %lld pairs outside 1..65535", (long long)P);
  MUVO_CHECK_ARG(h >= 1 && w >= 1 && h <= 8192 && w <= 8192, "flow_colour: tiles of %d x %d (1..8192)", h, w);
  MUVO_CHECK_ARG(flow && ws && panel && place, "flow_colour: null pointer");
  MUVO_CHECK_ARG(ws_bytes >= muvo_flow_colour_ws_bytes(P) && ((uintptr_t)ws & 3) == 0, "flow_colour: workspace of %lld bytes, %lld needed (4-byte aligned)",
                 (long long)ws_bytes, (long long)muvo_flow_colour_ws_bytes(P));
  MUVO_CHECK_ARG(pad >= 0 && pad <= 64 && padbyte >= 0 && padbyte <= 255, "flow_colour: pad %d outside 0..64 or pad byte %d outside 0..255", pad, padbyte);
  const MuvoTilePlace& p = *place;
  MUVO_CHECK_ARG(p.T > 0 && P % p.T == 0 && p.t0 >= 0 && p.t0 < (1 << 20) && p.T < (1 << 20), "flow_colour: %lld pairs are no multiple of T = %d (or t0 %d < 0)",
                 (long long)P, p.T, p.t0);
  MUVO_CHECK_ARG(p.PH > 0 && p.PW > 0 && p.chan_stride >= (int64_t)p.PH * p.PW && p.sample_stride >= 3 * p.chan_stride,
                 "flow_colour: panel %d x %d does not fit its strides (channel %lld, sample %lld, 3 channels)", p.PH, p.PW, (long long)p.chan_stride,
                 (long long)p.sample_stride);
  const int64_t b = P / p.T;
  MUVO_CHECK_ARG(panel_bytes >= (b - 1) * p.sample_stride + 2 * p.chan_stride + (int64_t)p.PH * p.PW, "flow_colour: panel of %lld bytes is too small for %lld samples",
                 (long long)panel_bytes, (long long)b);
  const int TH = h + 2 * pad, TW = w + 2 * pad;
  for (int t = p.t0; t < p.t0 + p.T; ++t) {
    const int64_t row0 = p.y0 + (int64_t)t * p.ystep, col0 = p.x0 + (int64_t)t * p.xstep + (t >= p.tsep ? p.sepw : 0);
    MUVO_CHECK_ARG(row0 >= 0 && col0 >= 0 && row0 + TH <= p.PH && col0 + TW <= p.PW, "flow_colour: the %d x %d tile of step %d at (%lld, %lld) leaves the %d x %d panel",
                   TH, TW, t, (long long)row0, (long long)col0, p.PH, p.PW);
    MUVO_CHECK_ARG((col0 & 1) == 0, "flow_colour: the tile of step %d starts at the odd column %lld (tiles are written in 2-pixel groups)", t, (long long)col0);
  }
  const int vec = ((uintptr_t)panel & 1) == 0 && (p.PW & 1) == 0 && (p.chan_stride & 1) == 0 && (p.sample_stride & 1) == 0;
  const long N = (long)h * w;
  hipLaunchKernelGGL(flow_minmax_kernel, dim3(FLOW_PART, (unsigned)P), dim3(256), 0, ST, flow, N, (float*)ws);
  const long n = (long)TH * ((TW + 1) / 2);
  hipLaunchKernelGGL(flow_colour_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)P), dim3(256), 0, ST, flow, (const float*)ws, h, w, pad, padbyte, p, vec, panel);
  MUVO_CHECK_LAUNCH("flow_colour");
  return MUVO_OK;
}

int64_t muvo_flow_epe_ws_doubles(int64_t P) { return P < 1 ? -1 : P * FLOW_PART * 3; }

int muvo_flow_epe(const float* flow_a, const float* flow_b, int64_t P, int h, int w, double* ws, int64_t ws_doubles, double* acc, void* stream) {
  MUVO_CHECK_ARG(P >= 1 && P <= 65535, "flow_epe: %lld pairs outside 1..65535", (long long)P);
  MUVO_CHECK_ARG(h >= 16 && w >= 16 && h <= 8192 && w <= 8192, "flow_epe: fields of %d x %d (16..8192 on both axes)", h, w);
  MUVO_CHECK_ARG(flow_a && flow_b && ws && acc, "flow_epe: null pointer");
  MUVO_CHECK_ARG(ws_doubles >= muvo_flow_epe_ws_doubles(P) && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)acc & 7) == 0,
                 "flow_epe: workspace of %lld doubles, %lld needed (8-byte aligned)", (long long)ws_doubles, (long long)muvo_flow_epe_ws_doubles(P));
  hipLaunchKernelGGL(flow_epe_kernel, dim3(FLOW_PART, (unsigned)P), dim3(256), 0, ST, flow_a, flow_b, h, w, ws);
  hipLaunchKernelGGL(flow_epe_sum_kernel, dim3(1), dim3(64), 0, ST, (const double*)ws, (int)P, acc);
  MUVO_CHECK_LAUNCH("flow_epe");
  return MUVO_OK;
}

}  // extern "C"
