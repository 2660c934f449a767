// HBM-bound glue kernels of the training step: activation backward, dropout, strided copies (cat/split),
// column sums (bias grads), NCHW<->token transposes with positional/type embedding (mile.py:542-569),
// max/avg pooling (timm ResNet stem, common.py:127, mile.py:107), trilinear x2 upsampling
// (common.py:169), PreProcess (preprocess.py:102-225), attention softmax(+dropout), GRU / RSSM pointwise
// math (transition.py:18-24,160-181).  All coalesced, grid-stride.
#include "resample.h"
#include "rssm_cell.h"

#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// ------------------------------------------------------------------------------------------ basic
__global__ void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx, long n,
                               int act, float slope) {
  GRID_STRIDE(i, n) dx[i] = dy[i] * act_grad_from_out(y[i], act, slope);
}
__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long n, int act, float slope) {
  GRID_STRIDE(i, n) y[i] = act_apply(x[i], act, slope);
}
__global__ void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float p, uint64_t seed) {
  GRID_STRIDE(i, n) y[i] = x[i] * dropout_scale(seed, (uint64_t)i, p);
}
__global__ void axpby_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n,
                             float alpha, float beta) {
  GRID_STRIDE(i, n) out[i] = alpha * a[i] + (b ? beta * b[i] : 0.f);
}
__global__ void copy2d_kernel(const float* __restrict__ src, float* __restrict__ dst, long rows, long cols, long lds,
                              long ldd, int accumulate) {
  const long n = rows * cols;
  GRID_STRIDE(i, n) {
    const long r = i / cols, c = i - r * cols;
    if (accumulate) dst[r * ldd + c] += src[r * lds + c];
    else dst[r * ldd + c] = src[r * lds + c];
  }
}
// out[c] += sum_r x[r*ld + c]
__global__ void __launch_bounds__(256) colsum_kernel(const float* __restrict__ x, float* __restrict__ out, long rows,
                                                     long cols, long ld) {
  // block handles 64 columns x a row chunk; 4 row-lanes per column
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long c = blockIdx.x * 64L + cl;
  const long per = (rows + gridDim.y - 1) / gridDim.y;
  const long r0 = blockIdx.y * per;
  long r1 = r0 + per;
  if (r1 > rows) r1 = rows;
  // eight independent loads per pass (the plain `s += x[..]` loop ran one dependent L2 round trip per row: 19 us for the bias
  // gradient of a 6500-row token matrix)
  float s = 0.f;
  if (c < cols) {
    long r = r0 + rl;
    for (; r + 28 < r1; r += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = x[(r + 4 * u) * ld + c];
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    for (; r < r1; r += 4) s += x[r * ld + c];
  }
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) atomicAdd(&out[c], red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
}
// out[j] = sum_n x[n*inner + j]  (batch reduction for broadcast parameters)
__global__ void batchsum_kernel(const float* __restrict__ x, float* __restrict__ out, int N, long inner, int accumulate) {
  GRID_STRIDE(j, inner) {
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += x[(long)n * inner + j];
    if (accumulate) out[j] += s; else out[j] = s;
  }
}

// -------------------------------------------------------------------------- NCHW <-> tokens (L,N,C)
// tokens[(l0+l)*N*C + n*C + c] = x[n][c][l] + pos[c][l] + temb[c*temb_stride]
__global__ void __launch_bounds__(256) nchw_to_tokens_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                             const float* __restrict__ temb, int temb_stride,
                                                             float* __restrict__ tok, int N, int C, int L, int l0) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * 32, lb = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, l = lb + tx;
    float v = 0.f;
    if (c < C && l < L) {
      v = x[((long)n * C + c) * L + l];
      if (pos) v += pos[(long)c * L + l];
      if (temb) v += temb[(long)c * temb_stride];
    }
    tile[k][tx] = v;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int l = lb + k, c = c0 + tx;
    if (c < C && l < L) tok[((long)(l0 + l) * N + n) * C + c] = tile[tx][k];
  }
}
// x[n][c][l] = tokens[(l0+l)*N*C + n*C + c]
__global__ void __launch_bounds__(256) tokens_to_nchw_kernel(const float* __restrict__ tok, float* __restrict__ x, int N,
                                                             int C, int L, int l0) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int c0 = blockIdx.y * 32, lb = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int l = lb + k, c = c0 + tx;
    tile[k][tx] = (c < C && l < L) ? tok[((long)(l0 + l) * N + n) * C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, l = lb + tx;
    if (c < C && l < L) x[((long)n * C + c) * L + l] = tile[tx][k];
  }
}

// ---------------------------------------------------------------------------------------- pooling
// max_pool2d (ResNet stem 3x3 s2 p1, DecoderDS 2x2 s2): the winner of each window is remembered as ONE BYTE (its position
// a*K + b inside the window; first maximum wins like PyTorch), so the backward pass moves 1 instead of 4 index bytes per
// output.  Thread = (4 consecutive columns, 1 row); no integer division per element (3-D grid).
template <int K, int S, int P>
__global__ void __launch_bounds__(256) maxpool2d_fwd_t_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              uint8_t* __restrict__ idx, int H, int W, int OH, int OW,
                                                              int load16) {
  const int ow0 = (blockIdx.x * 64 + threadIdx.x) * 4, oh = blockIdx.y * 4 + threadIdx.y;
  if (ow0 >= OW || oh >= OH) return;
  const long nc = blockIdx.z;
  const float* xp = x + nc * (long)H * W;
  float best[4];
  int bi[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { best[e] = -INFINITY; bi[e] = -1; }
#pragma unroll
  for (int a = 0; a < K; ++a) {
    const int h = oh * S - P + a;
    if ((unsigned)h >= (unsigned)H) continue;
    const float* row = xp + (long)h * W;
    constexpr int SPAN = 3 * S + K;                 // columns touched by 4 consecutive windows
    float v[SPAN];
    const int w0 = ow0 * S - P;
    if (S == 2 && load16) {
      // (uniform; maxpool2d_route: W % 8 == 0, OW * 2 == W, x 16-byte aligned)
      // the eight columns 2 * ow0 .. + 7 as two aligned 16-byte loads, plus the left neighbour for the 3-wide
      // window: unconditional (clamped address, masked value) instead of nine predicated 4-byte loads per row
      const float4 q0 = *reinterpret_cast<const float4*>(row + 2 * ow0), q1 = *reinterpret_cast<const float4*>(row + 2 * ow0 + 4);
      const float qs[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      if (P == 1) {
        const float l = row[ow0 > 0 ? 2 * ow0 - 1 : 0];
        v[0] = ow0 > 0 ? l : -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[1 + j] = qs[j];
      } else {
#pragma unroll
        for (int j = 0; j < SPAN && j < 8; ++j) v[j] = qs[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < SPAN; ++j) v[j] = ((unsigned)(w0 + j) < (unsigned)W) ? row[w0 + j] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int b = 0; b < K; ++b) {
        const bool in = (unsigned)(w0 + e * S + b) < (unsigned)W;
        const float t = v[e * S + b];
        if (in && (t > best[e] || bi[e] < 0)) { best[e] = t; bi[e] = a * K + b; }
      }
  }
  const long o = (nc * OH + oh) * (long)OW + ow0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (ow0 + e < OW) { y[o + e] = best[e]; idx[o + e] = (uint8_t)bi[e]; }
}
template <int K, int S, int P>
__global__ void __launch_bounds__(256) maxpool2d_bwd_t_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                              float* __restrict__ dx, int H, int W, int OH, int OW) {
  const int w0 = (blockIdx.x * 64 + threadIdx.x) * 4, h = blockIdx.y * 4 + threadIdx.y;
  if (w0 >= W || h >= H) return;
  const long nc = blockIdx.z;
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  // windows that contain row h: oh with oh*S - P <= h <= oh*S - P + K - 1
  const int oh_lo = (h + P - K + 1 <= 0) ? 0 : (h + P - K + S) / S, oh_hi = min((h + P) / S, OH - 1);
  const int ow_lo = (w0 + P - K + 1 <= 0) ? 0 : (w0 + P - K + S) / S, ow_hi = min((w0 + 3 + P) / S, OW - 1);
  // at most NOH x NOW windows touch the four columns of this lane: all their (winner byte, gradient) loads are issued up front
  // with clamped indices and masked afterwards (the two nested runtime loops made every load wait for the previous one)
  constexpr int NOH = (K + S - 1) / S, NOW = (3 + K - 1) / S + 1;
  int wv[NOH][NOW];
  float dv[NOH][NOW];
#pragma unroll
  for (int i = 0; i < NOH; ++i) {
    const int oh = oh_lo + i, ohc = min(oh <= oh_hi ? oh : oh_lo, OH - 1);     // (rows below the last window: nothing live, any valid address)
    const long ro = (nc * OH + ohc) * (long)OW;
#pragma unroll
    for (int j = 0; j < NOW; ++j) {
      const int ow = ow_lo + j, owc = min(ow <= ow_hi ? ow : ow_lo, OW - 1);
      wv[i][j] = idx[ro + owc];
      dv[i][j] = dy[ro + owc];
    }
  }
#pragma unroll
  for (int i = 0; i < NOH; ++i) {
    const int oh = oh_lo + i;
    const int a = h - (oh * S - P);
#pragma unroll
    for (int j = 0; j < NOW; ++j) {
      const int ow = ow_lo + j;
      const bool live = oh <= oh_hi && ow <= ow_hi;
      const int b0 = w0 - (ow * S - P);            // position of column w0 inside window ow
      const int win = wv[i][j] - a * K;            // winning column offset if the winner lies in row a
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (live && win == b0 + e && (unsigned)(b0 + e) < (unsigned)K) g[e] += dv[i][j];
    }
  }
  float* o = dx + (nc * H + h) * (long)W + w0;
  if (w0 + 3 < W && (((uintptr_t)o) & 15) == 0) {
    *(float4*)o = make_float4(g[0], g[1], g[2], g[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) if (w0 + e < W) o[e] = g[e];
  }
}
// 3x3 stride-2 pad-1 form for W % 8 == 0, OW % 4 == 0, H = 2 OH (the ResNet stems): a lane owns EIGHT consecutive input columns
// of the ROW PAIR (2r, 2r+1).  They are touched by the five windows 4l .. 4l+4 of the window rows r (rows 2r-1 .. 2r+1) and r+1
// (row 2r+1 only): per window row one 16-byte gradient load, one 4-byte winner load and one scalar pair for the fifth window -
// instead of 2 x 3 scalar pairs per four columns of one row - and four 16-byte stores.  Standalone on 20 x 64 x 160 x 416:
// 96 us against 134 us with one row per lane (tools/dev/maxpool_bwd_probe.hip; stores alone 54 us); it is the last memory-bound
// pass on the main stream before the stem's weight gradient.
__global__ void __launch_bounds__(256) maxpool3s2_bwd_v8_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                                 float* __restrict__ dx, int H, int W, int OH, int OW) {
  const int l = blockIdx.x * 64 + threadIdx.x, w0 = 8 * l, r = blockIdx.y * 4 + threadIdx.y;
  if (w0 >= W || 2 * r >= H) return;
  const long nc = blockIdx.z;
  float g0[8], g1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) g0[e] = g1[e] = 0.f;
  const int j4 = min(4 * l + 4, OW - 1);                              // fifth window (clamped; masked below)
  const bool live4 = 4 * l + 4 <= OW - 1;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int oh = min(r + i, OH - 1);
    const bool live = r + i <= OH - 1;
    const long ro = (nc * OH + oh) * (long)OW;
    const float4 d4 = *(const float4*)(dy + ro + 4 * l);
    const uchar4 i4 = *(const uchar4*)(idx + ro + 4 * l);
    const float dd[5] = {d4.x, d4.y, d4.z, d4.w, dy[ro + j4]};
    const int ww[5] = {i4.x, i4.y, i4.z, i4.w, idx[ro + j4]};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const bool lv = live && (j < 4 || live4);
      const int a0 = ww[j] / 3, b0 = ww[j] - 3 * a0;                   // winner (row, column) inside the window
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int e = 2 * j - 1 + b;                                   // window 4l+j covers columns 2j-1 .. 2j+1 of this lane
        if (e >= 0 && e < 8 && lv && b0 == b) {
          // window row r: input rows 2r-1 (a = 0, another lane's pair), 2r (a = 1), 2r+1 (a = 2); window row r+1: row 2r+1 is a = 0
          if (i == 0) {
            if (a0 == 1) g0[e] += dd[j];
            if (a0 == 2) g1[e] += dd[j];
          } else if (a0 == 0) {
            g1[e] += dd[j];
          }
        }
      }
    }
  }
  float* o = dx + (nc * H + 2 * r) * (long)W + w0;
  *(float4*)o = make_float4(g0[0], g0[1], g0[2], g0[3]);
  *(float4*)(o + 4) = make_float4(g0[4], g0[5], g0[6], g0[7]);
  *(float4*)(o + W) = make_float4(g1[0], g1[1], g1[2], g1[3]);
  *(float4*)(o + W + 4) = make_float4(g1[4], g1[5], g1[6], g1[7]);
}
// y[g] = mean_s x[g*S + s]; one wave per group
__global__ void __launch_bounds__(256) avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long G, long S) {
  const long g = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  float s = 0.f;
  for (long i = lane; i < S; i += 64) s += x[g * S + i];
  s = wave_sum(s);
  if (lane == 0) y[g] = s / (float)S;
}
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long G, long S) {
  const long n = G * S;
  const float inv = 1.f / (float)S;
  GRID_STRIDE(i, n) dx[i] = dy[i / S] * inv;
}

// ------------------------------------------------------------------------- trilinear x2 upsample
// The per-element steps of this section.  The x2 source coordinate is lin_src / lin_w of resample.h with the scale 0.5f.
// The eight corners [d][h][w] of an output combined in the nested form a (b (c v + fw v) + fh (..)) + fd (..)
__device__ __forceinline__ float trilerp(float fd, float fh, float fw, float v000, float v001, float v010, float v011, float v100,
                                         float v101, float v110, float v111) {
  const float a = 1.f - fd, b = 1.f - fh, c = 1.f - fw;
  return a * (b * (c * v000 + fw * v001) + fh * (c * v010 + fw * v011)) +
         fd * (b * (c * v100 + fw * v101) + fh * (c * v110 + fw * v111));
}
// weights with which input index i (of n) receives output indices 2i-1 .. 2i+2 (out-of-range outputs get 0)
__device__ __forceinline__ void up2_bwd_weights(int i, int n, float (&w)[4]) {
  w[0] = i > 0 ? 0.25f : 0.f;
  w[1] = i > 0 ? 0.75f : 1.f;
  w[2] = i < n - 1 ? 0.75f : 1.f;
  w[3] = i < n - 1 ? 0.25f : 0.f;
}
// the column adjoint of the vectorised backward kernels: coarse column w (of W) receives the fine columns 2w-1 .. 2w+2 = g0 .. g3,
// a fine column that does not exist passed as 0; the two inner weights are 1 where the forward clamps
__device__ __forceinline__ float up2_col_adjoint(int w, int W, float g0, float g1, float g2, float g3) {
  const float w1 = w > 0 ? 0.75f : 1.f, w2 = w < W - 1 ? 0.75f : 1.f;
  return (0.25f * g0 + w1 * g1) + (w2 * g2 + 0.25f * g3);
}

__global__ void upsample3d_x2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long NC, int D, int H, int W) {
  const int OD = 2 * D, OH = 2 * H, OW = 2 * W;
  const long n = NC * OD * OH * OW;
  GRID_STRIDE(i, n) {
    int od, oh, ow;
    const long nc = split_index(i, OD, OH, OW, od, oh, ow);
    int d0, d1, h0, h1, w0, w1;
    float fd, fh, fw;
    lin_src(od, D, 0.5f, d0, d1, fd);
    lin_src(oh, H, 0.5f, h0, h1, fh);
    lin_src(ow, W, 0.5f, w0, w1, fw);
    const float* xp = x + nc * D * H * W;
    y[i] = trilerp(fd, fh, fw, xp[(d0 * H + h0) * W + w0], xp[(d0 * H + h0) * W + w1], xp[(d0 * H + h1) * W + w0],
                   xp[(d0 * H + h1) * W + w1], xp[(d1 * H + h0) * W + w0], xp[(d1 * H + h0) * W + w1],
                   xp[(d1 * H + h1) * W + w0], xp[(d1 * H + h1) * W + w1]);
  }
}
__global__ void upsample3d_x2_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long NC, int D, int H, int W) {
  const int OD = 2 * D, OH = 2 * H, OW = 2 * W;
  const long n = NC * D * H * W;
  GRID_STRIDE(i, n) {
    int d, h, w;
    const long nc = split_index(i, D, H, W, d, h, w);
    const float* gp = dy + nc * OD * OH * OW;
    float acc = 0.f;
    for (int a = 2 * d - 1; a <= 2 * d + 2; ++a) {
      if ((unsigned)a >= (unsigned)OD) continue;
      const float wa = lin_w(a, d, D, 0.5f);
      if (wa == 0.f) continue;
      for (int b = 2 * h - 1; b <= 2 * h + 2; ++b) {
        if ((unsigned)b >= (unsigned)OH) continue;
        const float wb = lin_w(b, h, H, 0.5f);
        if (wb == 0.f) continue;
        float row = 0.f;
        for (int c = 2 * w - 1; c <= 2 * w + 2; ++c) {
          if ((unsigned)c >= (unsigned)OW) continue;
          row += lin_w(c, w, W, 0.5f) * gp[((long)a * OH + b) * OW + c];
        }
        acc += wa * wb * row;
      }
    }
    dx[i] = acc;
  }
}

// Vectorised variants (W even resp. W % 4 == 0): one float4 of outputs per lane, 3-D grid instead of 64-bit index
// decomposition.  grid = (ceil(OH*OW/4 / 256), OD, NC) forward; (ceil(H*W/4 / 256), D, NC) backward.
__global__ void __launch_bounds__(256) upsample3d_x2_fwd_vec_kernel(const float* __restrict__ x, float* __restrict__ y, int D,
                                                                    int H, int W) {
  const int OH = 2 * H, OW = 2 * W, Q = OW / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= OH * Q) return;
  const int oh = idx / Q, j = idx - oh * Q;
  const int od = blockIdx.y;
  const long nc = blockIdx.z;
  int d0, d1, h0, h1;
  float fd, fh;
  lin_src(od, D, 0.5f, d0, d1, fd);
  lin_src(oh, H, 0.5f, h0, h1, fh);
  const float* xp = x + nc * D * H * W;
  // input columns 2j-1 .. 2j+2 (clamped): the four outputs 4j+e read slots (0,1) (1,2) (1,2) (2,3)
  int wi[4];
#pragma unroll
  for (int s4 = 0; s4 < 4; ++s4) {
    int w = 2 * j - 1 + s4;
    wi[s4] = w < 0 ? 0 : (w > W - 1 ? W - 1 : w);
  }
  float r[4][4];  // [corner row][slot]
  const float* rows[4] = {xp + (d0 * H + h0) * W, xp + (d0 * H + h1) * W, xp + (d1 * H + h0) * W, xp + (d1 * H + h1) * W};
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) r[q][s4] = rows[q][wi[s4]];
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int i0, i1;
    float fw;
    lin_src(4 * j + e, W, 0.5f, i0, i1, fw);   // only the weight is used; the slots hold x[i0], x[i1]
    const int s0 = (e + 1) >> 1, s1 = s0 + 1;
    o[e] = trilerp(fd, fh, fw, r[0][s0], r[0][s1], r[1][s0], r[1][s1], r[2][s0], r[2][s1], r[3][s0], r[3][s1]);
  }
  float4* yp = (float4*)(y + ((nc * (2 * D) + od) * OH + oh) * (long)OW) + j;
  *yp = make_float4(o[0], o[1], o[2], o[3]);
}

// A 2 x 2 block of output (depth, row) positions per lane, ONE output float4 per position: lane = (row block ph, output float4
// f).  Outputs od = 2 pd - 1 and 2 pd read the SAME two input planes (pd - 1, pd, clamped) with weights (0.75, 0.25) and
// (0.25, 0.75), and likewise for rows: four float4 loads feed four float4 stores, and every store instruction of a wave
// writes whole 256-byte output rows: 5.4 TB/s on the 3-GB top level (a plain fill: 6.9; the four-outputs kernel above, with its
// 16 strided dword loads per float4 store: 1.9).
// Output columns 4 f .. 4 f + 3 come from input columns 2 f - 1 .. 2 f + 2: the lane pair (f, f ^ 1) loads the same aligned
// input float4 f >> 1 and takes the one missing column from its neighbour lane.  Blocks pd = 0 .. D, ph = 0 .. H; the
// positions that fall outside the output are skipped.
__global__ void __launch_bounds__(256) upsample3d_x2_fwd_row_kernel(const float* __restrict__ x, float* __restrict__ y, int D,
                                                                    int H, int W) {
  const int OH = 2 * H, OW = 2 * W, OQ = W / 2;      // output float4 per row
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < (H + 1) * OQ;
  const int ph = live ? idx / OQ : 0, f = live ? idx - ph * OQ : 0;
  const int pd = blockIdx.y;
  const long nc = blockIdx.z;
  const int d0 = pd > 0 ? pd - 1 : 0, d1 = pd < D ? pd : D - 1;
  const int h0 = ph > 0 ? ph - 1 : 0, h1 = ph < H ? ph : H - 1;
  const float* xp = x + nc * D * H * W + 4 * (f >> 1);
  const float4 r00 = *(const float4*)(xp + (d0 * H + h0) * W), r01 = *(const float4*)(xp + (d0 * H + h1) * W);
  const float4 r10 = *(const float4*)(xp + (d1 * H + h0) * W), r11 = *(const float4*)(xp + (d1 * H + h1) * W);
  typedef float nt_f4 __attribute__((ext_vector_type(4)));
  const bool odd = f & 1;
#pragma unroll
  for (int a = 0; a < 2; ++a) {              // od = 2 pd - 1 + a
    const float wd0 = a ? 0.25f : 0.75f, wd1 = 1.f - wd0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {            // oh = 2 ph - 1 + b
      const float wh0 = b ? 0.25f : 0.75f, wh1 = 1.f - wh0;
      const float w00 = wd0 * wh0, w01 = wd0 * wh1, w10 = wd1 * wh0, w11 = wd1 * wh1;
      const float cx = w00 * r00.x + w01 * r01.x + w10 * r10.x + w11 * r11.x;
      const float cy = w00 * r00.y + w01 * r01.y + w10 * r10.y + w11 * r11.y;
      const float cz = w00 * r00.z + w01 * r01.z + w10 * r10.z + w11 * r11.z;
      const float cw = w00 * r00.w + w01 * r01.w + w10 * r10.w + w11 * r11.w;
      const float lft = __shfl_up(cw, 1), rgt = __shfl_down(cx, 1);     // lane f - 1 holds input float4 (f - 1) >> 1, lane f + 1: (f + 1) >> 1
      const float q0 = odd ? cy : (f > 0 ? lft : cx);
      const float q1 = odd ? cz : cx;
      const float q2 = odd ? cw : cy;
      const float q3 = odd ? (f < OQ - 1 ? rgt : cw) : cz;
      const int od = 2 * pd - 1 + a, oh = 2 * ph - 1 + b;
      if (live && od >= 0 && od < 2 * D && oh >= 0 && oh < OH) {
        float4* yp = (float4*)(y + ((nc * (2 * D) + od) * OH + oh) * (long)OW) + f;
        __builtin_nontemporal_store((nt_f4){0.25f * q0 + 0.75f * q1, 0.75f * q1 + 0.25f * q2, 0.25f * q1 + 0.75f * q2, 0.75f * q2 + 0.25f * q3},
                                    (nt_f4*)yp);
      }
    }
  }
}

__global__ void __launch_bounds__(256) upsample3d_x2_bwd_vec_kernel(const float* __restrict__ dy, float* __restrict__ dx, int D,
                                                                    int H, int W) {
  const int OH = 2 * H, OW = 2 * W, Q = W / 4;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * Q) return;
  const int h = idx / Q, j = idx - h * Q;
  const int d = blockIdx.y;
  const long nc = blockIdx.z;
  float wa[4], wb[4];
  up2_bwd_weights(d, D, wa);
  up2_bwd_weights(h, H, wb);
  const float* gp = dy + nc * (2 * D) * (long)OH * OW;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const bool left = j > 0, right = 8 * j + 8 < OW;
#pragma unroll
  for (int ia = 0; ia < 4; ++ia) {
    const int a = 2 * d - 1 + ia;
    if (wa[ia] == 0.f) continue;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
      const int b = 2 * h - 1 + ib;
      if (wb[ib] == 0.f) continue;
      const float* row = gp + ((long)a * OH + b) * OW + 8 * j;
      const float4 m0 = *(const float4*)row, m1 = *(const float4*)(row + 4);
      const float gl = left ? row[-1] : 0.f, gr = right ? row[8] : 0.f;
      const float g[10] = {gl, m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, gr};
      const float wab = wa[ia] * wb[ib];
#pragma unroll
      for (int e = 0; e < 4; ++e)       // input column w = 4j+e receives outputs 2w-1 .. 2w+2 = g[2e .. 2e+3]
        acc[e] += wab * up2_col_adjoint(4 * j + e, W, g[2 * e], g[2 * e + 1], g[2 * e + 2], g[2 * e + 3]);
    }
  }
  float4* xp = (float4*)(dx + ((nc * D + d) * H + h) * (long)W) + j;
  *xp = make_float4(acc[0], acc[1], acc[2], acc[3]);
}

// The same adjoint with every fine element fetched from HBM once: a workgroup WALKS along d.  A lane keeps the (w, h)-reduced
// contributions P_a of the last two fine planes in registers; coarse plane d = 0.25 P_{2d-1} + 0.75 P_{2d} + 0.75 P_{2d+1} +
// 0.25 P_{2d+2} needs only the two new planes per step (the gather form above reads each fine row four times over and ran at
// 1.85 TB/s).  One FINE float4 per lane and row: lane = (coarse row h, fine float4 f), so a load instruction of a wave reads
// whole 256-byte fine rows and the coarse result leaves as a float2 per lane, i.e. whole coarse rows per store instruction.  Fine columns 4 f .. 4 f + 3 feed
// the coarse columns 2 f and 2 f + 1; the two missing fine neighbours (4 f - 1, 4 f + 4) come from the adjacent lanes.
// 256 threads = 256 / (W / 2) coarse rows; grid = (row groups, d segments, N * C).
__global__ void __launch_bounds__(256) upsample3d_x2_bwd_row_kernel(const float* __restrict__ dy, float* __restrict__ dx, int D,
                                                                    int H, int W, int dseg) {
  const int OH = 2 * H, OW = 2 * W, OQ = W / 2;
  const int f = threadIdx.x % OQ;
  const int hr = blockIdx.x * (256 / OQ) + threadIdx.x / OQ;
  const bool live = hr < H;
  const int h = live ? hr : H - 1;
  const long nc = blockIdx.z;
  const int d0 = blockIdx.y * dseg, d1 = min(d0 + dseg, D);
  float wb[4];
  up2_bwd_weights(h, H, wb);
  const float* gp = dy + nc * (2L * D) * OH * OW + 4 * f;
  const long ps = (long)OH * OW;
  // the four fine rows of plane a that this lane's coarse row receives (clamped row / plane: masked by the weights below)
  auto load_rows = [&](int a, float4 (&g)[4]) {
    const int ac = a < 0 ? 0 : (a >= 2 * D ? 2 * D - 1 : a);
    const float* plane = gp + (long)ac * ps;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
      int r = 2 * h - 1 + ib;
      r = r < 0 ? 0 : (r > OH - 1 ? OH - 1 : r);
      g[ib] = *(const float4*)(plane + (long)r * OW);
    }
  };
  auto reduce_rows = [&](int a, const float4 (&g)[4]) -> float2 {
    float2 acc = make_float2(0.f, 0.f);
    const float pw = (a < 0 || a >= 2 * D) ? 0.f : 1.f;      // (uniform) the plane does not exist
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
      const float lft = __shfl_up(g[ib].w, 1), rgt = __shfl_down(g[ib].x, 1);
      const float gl = f > 0 ? lft : 0.f, gr = f < OQ - 1 ? rgt : 0.f;
      const float wgt = wb[ib] * pw;                          // 0 for the rows that do not exist
      acc.x += wgt * up2_col_adjoint(2 * f, W, gl, g[ib].x, g[ib].y, g[ib].z);
      acc.y += wgt * up2_col_adjoint(2 * f + 1, W, g[ib].y, g[ib].z, g[ib].w, gr);
    }
    return acc;
  };
  // Walk along d with the loads of the NEXT coarse plane issued before the store of the current one (a load behind a store
  // waits for the store's acknowledgement): eight unconditional float4 loads in flight per lane while a result leaves.
  float4 ga[4], gb[4];
  load_rows(2 * d0 - 1, ga); load_rows(2 * d0, gb);
  float2 pm1 = reduce_rows(2 * d0 - 1, ga), p0 = reduce_rows(2 * d0, gb);
  load_rows(2 * d0 + 1, ga); load_rows(2 * d0 + 2, gb);
  for (int d = d0; d < d1; ++d) {
    const float2 p1 = reduce_rows(2 * d + 1, ga), p2 = reduce_rows(2 * d + 2, gb);
    if (d + 1 < d1) { load_rows(2 * d + 3, ga); load_rows(2 * d + 4, gb); }     // (uniform)
    float wa[4];
    up2_bwd_weights(d, D, wa);
    float2 o;
    o.x = (wa[0] * pm1.x + wa[1] * p0.x) + (wa[2] * p1.x + wa[3] * p2.x);
    o.y = (wa[0] * pm1.y + wa[1] * p0.y) + (wa[2] * p1.y + wa[3] * p2.y);
    // rows past H (partial last workgroup) recompute row H - 1 and store the identical value
    *((float2*)(dx + ((nc * D + d) * H + h) * (long)W) + f) = o;
    pm1 = p1; p0 = p2;
  }
}

// ------------------------------------------------------------------------------------ preprocess
// u8 (NC, H, W) -> crop (top,left,CH,CW) -> /255 -> label ; (label-mean[c])/std[c] -> normalised
__global__ void preprocess_image_kernel(const uint8_t* __restrict__ img, float* __restrict__ label,
                                        float* __restrict__ norm, long NC, int C, int H, int W, int top, int left, int CH,
                                        int CW, Norm3 ms) {
  const long n = NC * CH * CW;
  GRID_STRIDE(i, n) {
    int y, x;
    const long nc = split_index(i, CH, CW, y, x);
    const float v = (float)img[(nc * H + (y + top)) * W + (x + left)] / 255.f;
    if (label) label[i] = v;
    norm[i] = normalise3(ms, (int)(nc % C), v);
  }
}
// route map: u8 (NC,H,W) -> /255 -> nearest resize (OH,OW) -> normalise
__global__ void preprocess_route_kernel(const uint8_t* __restrict__ img, float* __restrict__ norm, long NC, int C, int H,
                                        int W, int OH, int OW, Norm3 ms) {
  const long n = NC * OH * OW;
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  GRID_STRIDE(i, n) {
    int y, x;
    const long nc = split_index(i, OH, OW, y, x);
    const float v = (float)img[(nc * H + nearest_src(y, H, sh)) * W + nearest_src(x, W, sw)] / 255.f;
    norm[i] = normalise3(ms, (int)(nc % C), v);
  }
}
__global__ void scale_kernel(const float* __restrict__ x, float* __restrict__ y, long n, float inv) {
  GRID_STRIDE(i, n) y[i] = x[i] / inv;
}
// bilinear, align_corners=False, no antialias (torchvision 0.15 tensor resize / F.interpolate)
__global__ void resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, long NC, int H, int W, int OH,
                                       int OW) {
  const long n = NC * OH * OW;
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  GRID_STRIDE(i, n) {
    int oy, ox, y0, y1, x0, x1;
    float ly, lx;
    const long nc = split_index(i, OH, OW, oy, ox);
    lin_src(oy, H, sh, y0, y1, ly);
    lin_src(ox, W, sw, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* xp = x + nc * H * W;
    y[i] = hy * (hx * xp[y0 * W + x0] + lx * xp[y0 * W + x1]) + ly * (hx * xp[y1 * W + x0] + lx * xp[y1 * W + x1]);
  }
}
// nearest (legacy 'nearest': src = floor(dst * in/out)), up to 3 spatial dims, element size 1 or 4 bytes
template <typename T>
__global__ void resize_nearest_kernel(const T* __restrict__ x, T* __restrict__ y, long NC, int D, int H, int W, int OD,
                                      int OH, int OW) {
  const long n = NC * OD * OH * OW;
  const float sd = (float)D / (float)OD, sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  GRID_STRIDE(i, n) {
    int oz, oy, ox;
    const long nc = split_index(i, OD, OH, OW, oz, oy, ox);
    y[i] = x[((nc * D + nearest_src(oz, D, sd)) * H + nearest_src(oy, H, sh)) * W + nearest_src(ox, W, sw)];
  }
}
// Antialiased linear resize of (NC, H, W) float planes (include/muvo_hip.h: muvo_resize_bilinear_aa): EVAL.RESOLUTION of
// PreProcess.forward (preprocess.py:209-210,252-273: torchvision 0.15.2 resize(antialias=True) = ATen _upsample_bilinear2d_aa).
// One thread per output pixel; per axis the taps [lo, hi) and triangle weights of ATen's _compute_indices_min_size_weights_aa in
// float32, normalised; horizontal sums first, then the vertical combination (the order of the separable reference kernel).
struct AaTaps { int lo, n; float center, inv, total; };
__device__ __forceinline__ AaTaps aa_taps(int o, int in_size, float scale) {
  const float support = scale >= 1.f ? scale : 1.f;
  AaTaps t;
  t.inv = scale >= 1.f ? 1.f / scale : 1.f;
  t.center = scale * ((float)o + 0.5f);
  int lo = (int)(t.center - support + 0.5f), hi = (int)(t.center + support + 0.5f);
  lo = lo < 0 ? 0 : lo;
  hi = hi > in_size ? in_size : hi;
  t.lo = lo;
  t.n = hi - lo;
  float tot = 0.f;
  for (int j = 0; j < t.n; ++j) {
    const float w = 1.f - fabsf(((float)(j + lo) - t.center + 0.5f) * t.inv);
    tot += w > 0.f ? w : 0.f;
  }
  t.total = tot;
  return t;
}
__device__ __forceinline__ float aa_weight(const AaTaps& t, int j) {
  const float w = 1.f - fabsf(((float)(j + t.lo) - t.center + 0.5f) * t.inv);
  return (w > 0.f ? w : 0.f) / t.total;
}
__global__ void __launch_bounds__(256) resize_bilinear_aa_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 float* __restrict__ ynorm, Norm3 ms, long NC, int C, int H, int W,
                                                                 int OH, int OW) {
  const float sh = (float)H / (float)OH, sw = (float)W / (float)OW;
  const long total = NC * OH * OW;
  GRID_STRIDE(i, total) {
    int oy, ox;
    const long nc = split_index(i, OH, OW, oy, ox);
    const AaTaps tx = aa_taps(ox, W, sw), ty = aa_taps(oy, H, sh);
    const float* p = x + nc * (long)H * W;
    float acc = 0.f;
    for (int r = 0; r < ty.n; ++r) {
      const float* row = p + (long)(ty.lo + r) * W + tx.lo;
      float rs = 0.f;
      for (int j = 0; j < tx.n; ++j) rs += row[j] * aa_weight(tx, j);
      acc += rs * aa_weight(ty, r);
    }
    y[i] = acc;
    if (ynorm) ynorm[i] = normalise3(ms, (int)(nc % C), acc);
  }
}

// ----------------------------------------------------------------------------------- attention
// P = softmax(S) over cols (S already scaled); Pd = dropout(P).  One wave per row, cols <= 64*MAXV.  Rows of up to 512 columns
// use MAXV = 8; longer ones, up to 64 * SOFTMAX_MAXV = 1088 (the unfused path as a comparison for the streamed attention kernels
// at 517 and 1037 tokens), the wider instance.
#define SOFTMAX_MAXV 17
template <int MAXV>
__global__ void __launch_bounds__(256) softmax_dropout_fwd_kernel(const float* __restrict__ S, float* __restrict__ P,
                                                                  float* __restrict__ Pd, long rows, int cols, float p,
                                                                  uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[MAXV];
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < cols ? S[row * cols + c] : -INFINITY;
    mx = fmaxf(mx, v[k]);
  }
  mx = wave_max(mx);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < cols ? expf(v[k] - mx) : 0.f;
    s += v[k];
  }
  const float inv = 1.f / wave_sum(s);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c = lane + 64 * k;
    if (c < cols) {
      const long idx = row * cols + c;
      const float pv = v[k] * inv;
      P[idx] = pv;
      if (Pd) Pd[idx] = pv * dropout_scale(seed, (uint64_t)idx, p);
    }
  }
}
// dS = P * (dP - sum(dP*P)), dP = dPd * dropmask
template <int MAXV>
__global__ void __launch_bounds__(256) softmax_dropout_bwd_kernel(const float* __restrict__ P, const float* __restrict__ dPd,
                                                                  float* __restrict__ dS, long rows, int cols, float p,
                                                                  uint64_t seed) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= rows) return;
  float pv[MAXV], g[MAXV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c = lane + 64 * k;
    pv[k] = 0.f; g[k] = 0.f;
    if (c < cols) {
      const long idx = row * cols + c;
      pv[k] = P[idx];
      g[k] = dPd[idx] * dropout_scale(seed, (uint64_t)idx, p);
      s += pv[k] * g[k];
    }
  }
  s = wave_sum(s);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int c = lane + 64 * k;
    if (c < cols) dS[row * cols + c] = pv[k] * (g[k] - s);
  }
}

// ---------------------------------------------------------------------------------------- RSSM
// the per-op path of the GRU cell and the sample step (rssm_cell.h); rows of gi / gh are 3 H floats: r | z | n
__global__ void gru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                               float* __restrict__ hn, int B, int H) {
  const long n = (long)B * H;
  GRID_STRIDE(i, n) {
    const long b = i / H, j = i - b * H;
    const float *a = gi + b * 3 * H, *c = gh + b * 3 * H;
    hn[i] = gru_combine(gru_gates(a[j], a[H + j], a[2 * H + j], c[j], c[H + j], c[2 * H + j]), h[i]);
  }
}
__global__ void gru_bwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh, const float* __restrict__ h,
                               const float* __restrict__ dhn, float* __restrict__ dgi, float* __restrict__ dgh,
                               float* __restrict__ dh, int B, int H) {
  const long n = (long)B * H;
  GRID_STRIDE(i, n) {
    const long b = i / H, j = i - b * H;
    const float *a = gi + b * 3 * H, *c = gh + b * 3 * H;
    const float ghn = c[2 * H + j];
    const GruAdjoint d = gru_adjoint(gru_gates(a[j], a[H + j], a[2 * H + j], c[j], c[H + j], ghn), ghn, h[i], dhn[i]);
    float* da = dgi + b * 3 * H;
    float* dc = dgh + b * 3 * H;
    da[j] = d.dpre_r; dc[j] = d.dpre_r;
    da[H + j] = d.dpre_z; dc[H + j] = d.dpre_z;
    da[2 * H + j] = d.dpre_n; dc[2 * H + j] = d.dgh_n;
    dh[i] = d.dh;
  }
}
// (mu | log_sigma) (B, 2S) -> mu, sigma, sample; eps == nullptr: no noise
__global__ void rssm_sample_fwd_kernel(const float* __restrict__ mls, const float* __restrict__ eps, long eps_ld,
                                       float* __restrict__ mu, float* __restrict__ sigma, float* __restrict__ sample,
                                       int B, int S, float min_std) {
  const long n = (long)B * S;
  GRID_STRIDE(i, n) {
    const long b = i / S, j = i - b * S;
    const float m = mls[b * 2 * S + j];
    const float sg = rssm_sigma(mls[b * 2 * S + S + j], min_std);
    mu[i] = m;
    sigma[i] = sg;
    sample[i] = rssm_sample(m, sg, eps ? eps[b * eps_ld + j] : 0.f);
  }
}
__global__ void rssm_sample_bwd_kernel(const float* __restrict__ mls, const float* __restrict__ eps, long eps_ld,
                                       const float* __restrict__ dmu, const float* __restrict__ dsigma,
                                       const float* __restrict__ dsample, float* __restrict__ dmls, int B, int S) {
  const long n = (long)B * S;
  GRID_STRIDE(i, n) {
    const long b = i / S, j = i - b * S;
    const SampleAdjoint d = rssm_sample_adjoint(mls[b * 2 * S + S + j], eps ? eps[b * eps_ld + j] : 0.f, dmu ? dmu[i] : 0.f,
                                                dsigma ? dsigma[i] : 0.f, dsample ? dsample[i] : 0.f);
    dmls[b * 2 * S + j] = d.dmu;
    dmls[b * 2 * S + S + j] = d.dls;
  }
}

// =============================================================================================== ABI
#define ST ((hipStream_t)stream)
// The launch step of the flat grid-stride kernels: ew_grid(n) workgroups of 256 threads on the stream, then the launch check
// under `name`.  The arguments are converted to the kernel's parameter types (the int64_t sizes of the ABI to long).  Argument
// checks and the behaviour at n == 0 stay with each entry point.
template <typename... P, typename... A>
static int launch_flat(const char* name, void (*kernel)(P...), long n, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3(ew_grid(n)), dim3(256), 0, ST, static_cast<P>(args)...);
  MUVO_CHECK_LAUNCH(name);
  return MUVO_OK;
}
// the template instance of a checked max-pool window (3x3 / 2 / 1 or 2x2 / 2 / 0) resp. of a checked softmax row length
#define MAXPOOL_INSTANCE(kernel, k) ((k) == 3 ? kernel<3, 2, 1> : kernel<2, 2, 0>)
#define SOFTMAX_INSTANCE(kernel, cols) (softmax_dropout_maxv(cols) == 8 ? kernel<8> : kernel<SOFTMAX_MAXV>)

extern "C" {

int muvo_act_bwd(const float* y, const float* dy, float* dx, int64_t n, int act, float slope, void* stream) {
  MUVO_CHECK_ARG(y && dy && dx && n >= 0, "act_bwd: bad args");
  if (n == 0) return MUVO_OK;
  return launch_flat("act_bwd", act_bwd_kernel, n, stream, y, dy, dx, n, act, slope);
}
int muvo_act_fwd(const float* x, float* y, int64_t n, int act, float slope, void* stream) {
  MUVO_CHECK_ARG(x && y && n >= 0, "act_fwd: bad args");
  if (n == 0) return MUVO_OK;
  return launch_flat("act_fwd", act_fwd_kernel, n, stream, x, y, n, act, slope);
}
int muvo_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream) {
  MUVO_CHECK_ARG(x && y && n >= 0 && p >= 0.f && p < 1.f, "dropout: bad args");
  if (n == 0) return MUVO_OK;
  return launch_flat("dropout", dropout_kernel, n, stream, x, y, n, p, seed);
}
int muvo_axpby(const float* a, const float* b, float* out, int64_t n, float alpha, float beta, void* stream) {
  MUVO_CHECK_ARG(a && out && n >= 0, "axpby: bad args");
  if (n == 0) return MUVO_OK;
  return launch_flat("axpby", axpby_kernel, n, stream, a, b, out, n, alpha, beta);
}
int muvo_copy2d(const float* src, float* dst, int64_t rows, int64_t cols, int64_t ld_src, int64_t ld_dst, int accumulate,
                void* stream) {
  MUVO_CHECK_ARG(src && dst && rows >= 0 && cols >= 0 && ld_src >= cols && ld_dst >= cols, "copy2d: bad args");
  if (rows * cols == 0) return MUVO_OK;
  return launch_flat("copy2d", copy2d_kernel, rows * cols, stream, src, dst, rows, cols, ld_src, ld_dst, accumulate);
}
int muvo_colsum_acc(const float* x, float* out, int64_t rows, int64_t cols, int64_t ld, void* stream) {
  MUVO_CHECK_ARG(x && out && rows > 0 && cols > 0 && ld >= cols, "colsum: bad args");
  int chunks = cdiv(rows, 64);           // 16 rows per lane: enough workgroups to cover the chip even for 384 columns
  if (chunks > 1024) chunks = 1024;
  if (muvo_det()) chunks = 1;
  hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(cols, 64), chunks), dim3(256), 0, ST, x, out, (long)rows, (long)cols, (long)ld);
  MUVO_CHECK_LAUNCH("colsum");
  return MUVO_OK;
}
int muvo_batchsum(const float* x, float* out, int N, int64_t inner, int accumulate, void* stream) {
  MUVO_CHECK_ARG(x && out && N > 0 && inner > 0, "batchsum: bad args");
  return launch_flat("batchsum", batchsum_kernel, inner, stream, x, out, N, inner, accumulate);
}
int muvo_nchw_to_tokens(const float* x, const float* pos, const float* temb, int temb_stride, float* tokens, int N, int C,
                        int L, int l0, void* stream) {
  MUVO_CHECK_ARG(x && tokens && N > 0 && C > 0 && L > 0 && l0 >= 0, "nchw_to_tokens: bad args");
  hipLaunchKernelGGL(nchw_to_tokens_kernel, dim3(cdiv(L, 32), cdiv(C, 32), N), dim3(256), 0, ST, x, pos, temb, temb_stride,
                     tokens, N, C, L, l0);
  MUVO_CHECK_LAUNCH("nchw_to_tokens");
  return MUVO_OK;
}
int muvo_tokens_to_nchw(const float* tokens, float* x, int N, int C, int L, int l0, void* stream) {
  MUVO_CHECK_ARG(x && tokens && N > 0 && C > 0 && L > 0 && l0 >= 0, "tokens_to_nchw: bad args");
  hipLaunchKernelGGL(tokens_to_nchw_kernel, dim3(cdiv(L, 32), cdiv(C, 32), N), dim3(256), 0, ST, tokens, x, N, C, L, l0);
  MUVO_CHECK_LAUNCH("tokens_to_nchw");
  return MUVO_OK;
}
// The host decisions of muvo_maxpool2d_fwd / _bwd for checked arguments (the pointers count only by their alignment): the
// launchers launch from it, muvo_maxpool2d_route reports it.
static void maxpool2d_route(bool backward, int64_t NC, int H, int W, int k, int s, int p, const void* in, const void* idx,
                            const void* out, muvo_maxpool2d_route_info* r) {
  const int OH = (H + 2 * p - k) / s + 1, OW = (W + 2 * p - k) / s + 1;
  r->k = k;
  r->load16 = r->v8 = 0;
  r->block[0] = 64; r->block[1] = 4; r->block[2] = 1;
  r->grid[2] = (int32_t)NC;
  if (!backward) {
    r->load16 = s == 2 && (W & 7) == 0 && OW * 2 == W && (((uintptr_t)in) & 15) == 0;
    r->grid[0] = cdiv(OW, 256); r->grid[1] = cdiv(OH, 4);
    return;
  }
  if (k == 3 && W % 8 == 0 && OW % 4 == 0 && 2 * OW == W && 2 * OH == H && ((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0 &&
      (((uintptr_t)idx) & 3) == 0) {
    r->v8 = 1;
    r->grid[0] = cdiv(W / 8, 64); r->grid[1] = cdiv(H / 2, 4);
    return;
  }
  r->grid[0] = cdiv(W, 256); r->grid[1] = cdiv(H, 4);
}
// out: the (OH, OW) a launcher was given (the route query has none)
static int maxpool2d_check(int64_t NC, int H, int W, int k, int s, int p, const int* out = nullptr) {
  MUVO_CHECK_ARG(NC > 0 && NC <= 2147483647L && H > 0 && W > 0, "maxpool2d: bad sizes");
  MUVO_CHECK_ARG((k == 3 && s == 2 && p == 1) || (k == 2 && s == 2 && p == 0), "maxpool2d: only 3x3 s2 p1 and 2x2 s2 p0 are on the path");
  MUVO_CHECK_ARG(H + 2 * p >= k && W + 2 * p >= k, "maxpool2d: window larger than the padded image");
  MUVO_CHECK_ARG(!out || (out[0] == (H + 2 * p - k) / s + 1 && out[1] == (W + 2 * p - k) / s + 1), "maxpool2d: output size");
  return MUVO_OK;
}
int muvo_maxpool2d_route(int backward, int64_t NC, int H, int W, int k, int s, int p, const void* in, const void* idx,
                         const void* out, muvo_maxpool2d_route_info* r) {
  MUVO_CHECK_ARG(r, "maxpool2d_route: null pointer");
  int rc = maxpool2d_check(NC, H, W, k, s, p);
  if (rc) return rc;
  maxpool2d_route(backward != 0, NC, H, W, k, s, p, in, idx, out, r);
  return MUVO_OK;
}
int muvo_maxpool2d_fwd(const float* x, float* y, uint8_t* idx, int64_t NC, int H, int W, int OH, int OW, int k, int s, int p,
                       void* stream) {
  MUVO_CHECK_ARG(x && y && idx, "maxpool2d_fwd: bad args");
  const int out[2] = {OH, OW};
  int rc = maxpool2d_check(NC, H, W, k, s, p, out);
  if (rc) return rc;
  MUVO_CHECK_ARG(cdiv(OH, 4) <= 65535, "maxpool2d_fwd: image too tall");
  muvo_maxpool2d_route_info r;
  maxpool2d_route(false, NC, H, W, k, s, p, x, idx, y, &r);
  hipLaunchKernelGGL(MAXPOOL_INSTANCE(maxpool2d_fwd_t_kernel, r.k), dim3(r.grid[0], r.grid[1], r.grid[2]), dim3(r.block[0], r.block[1]), 0,
                     ST, x, y, idx, H, W, OH, OW, r.load16);
  MUVO_CHECK_LAUNCH("maxpool2d_fwd");
  return MUVO_OK;
}
int muvo_maxpool2d_bwd(const float* dy, const uint8_t* idx, float* dx, int64_t NC, int H, int W, int OH, int OW, int k,
                       int s, int p, void* stream) {
  MUVO_CHECK_ARG(dy && dx && idx, "maxpool2d_bwd: bad args");
  const int out[2] = {OH, OW};
  int rc = maxpool2d_check(NC, H, W, k, s, p, out);
  if (rc) return rc;
  MUVO_CHECK_ARG(cdiv(H, 4) <= 65535, "maxpool2d_bwd: image too tall");
  muvo_maxpool2d_route_info r;
  maxpool2d_route(true, NC, H, W, k, s, p, dy, idx, dx, &r);
  hipLaunchKernelGGL((r.v8 ? maxpool3s2_bwd_v8_kernel : MAXPOOL_INSTANCE(maxpool2d_bwd_t_kernel, r.k)), dim3(r.grid[0], r.grid[1], r.grid[2]),
                     dim3(r.block[0], r.block[1]), 0, ST, dy, idx, dx, H, W, OH, OW);
  MUVO_CHECK_LAUNCH("maxpool2d_bwd");
  return MUVO_OK;
}
int muvo_avgpool_fwd(const float* x, float* y, int64_t G, int64_t S, void* stream) {
  MUVO_CHECK_ARG(x && y && G > 0 && S > 0, "avgpool_fwd: bad args");
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(cdiv(G, 4)), dim3(256), 0, ST, x, y, (long)G, (long)S);
  MUVO_CHECK_LAUNCH("avgpool_fwd");
  return MUVO_OK;
}
int muvo_avgpool_bwd(const float* dy, float* dx, int64_t G, int64_t S, void* stream) {
  MUVO_CHECK_ARG(dy && dx && G > 0 && S > 0, "avgpool_bwd: bad args");
  return launch_flat("avgpool_bwd", avgpool_bwd_kernel, G * S, stream, dy, dx, G, S);
}
// The host decision of muvo_upsample3d_x2_fwd / _bwd for checked sizes: kernel, grid, block and the d segments of the walking
// backward kernel.  The pointers count only by their alignment: a kernel is chosen only if every pointer it accesses with 16-byte
// instructions is 16-byte aligned (W % 4 == 0 resp. W % 2 == 0 keeps every row start as aligned as the base), anything else
// goes to the next kernel down, ultimately the scalar ones.  The launchers launch from it, muvo_upsample3d_route reports it.
static void upsample3d_route(bool backward, int64_t NC, int D, int H, int W, const void* in, const void* out,
                             muvo_upsample3d_route_info* r) {
  const bool in16 = (((uintptr_t)in) & 15) == 0, out16 = (((uintptr_t)out) & 15) == 0;
  const int oq = W / 2;                     // fine float4 per row
  const bool oq_ok = W % 4 == 0 && oq <= 64 && (oq & (oq - 1)) == 0;
  r->segs = 1; r->dseg = D;
  r->grid[1] = r->grid[2] = 1;
  r->block[0] = 256; r->block[1] = r->block[2] = 1;
  if (!backward) {
    if (oq_ok && D + 1 <= 65535 && NC <= 65535 && in16 && out16) {          // float4 loads of x, 16-byte stores of y
      r->kernel = MUVO_UPSAMPLE_ROW;
      r->grid[0] = cdiv((long)(H + 1) * oq, 256); r->grid[1] = D + 1; r->grid[2] = (int32_t)NC;
    } else if (W % 2 == 0 && 2 * D <= 65535 && NC <= 65535 && out16) {      // dword loads of x, float4 stores of y
      r->kernel = MUVO_UPSAMPLE_VEC;
      r->grid[0] = cdiv((long)2 * H * (2 * W / 4), 256); r->grid[1] = 2 * D; r->grid[2] = (int32_t)NC;
    } else {
      r->kernel = MUVO_UPSAMPLE_SCALAR;
      r->grid[0] = ew_grid(NC * D * H * W * 8);
    }
    return;
  }
  if (oq_ok && NC <= 65535 && in16 && out16) {                              // float4 loads of dy, float2 stores of dx
    // enough workgroups to fill the chip: split the d range (each segment recomputes its two lead-in planes)
    const int rgroups = cdiv(H, 256 / oq);
    int segs = 1;
    while ((long)NC * rgroups * segs < 4096 && segs * 16 <= D) segs *= 2;
    r->kernel = MUVO_UPSAMPLE_ROW;
    r->dseg = cdiv(D, segs);
    r->segs = cdiv(D, r->dseg);
    r->grid[0] = rgroups; r->grid[1] = r->segs; r->grid[2] = (int32_t)NC;
  } else if (W % 4 == 0 && D <= 65535 && NC <= 65535 && in16 && out16) {    // float4 loads of dy, float4 stores of dx
    r->kernel = MUVO_UPSAMPLE_VEC;
    r->grid[0] = cdiv((long)H * (W / 4), 256); r->grid[1] = D; r->grid[2] = (int32_t)NC;
  } else {
    r->kernel = MUVO_UPSAMPLE_SCALAR;
    r->grid[0] = ew_grid(NC * D * H * W);
  }
}
int muvo_upsample3d_route(int backward, int64_t NC, int D, int H, int W, const void* in, const void* out,
                          muvo_upsample3d_route_info* r) {
  MUVO_CHECK_ARG(r && NC > 0 && D > 0 && H > 0 && W > 0, "upsample3d_route: bad args");
  upsample3d_route(backward != 0, NC, D, H, W, in, out, r);
  return MUVO_OK;
}
int muvo_upsample3d_x2_fwd(const float* x, float* y, int64_t NC, int D, int H, int W, void* stream) {
  MUVO_CHECK_ARG(x && y && NC > 0 && D > 0 && H > 0 && W > 0, "upsample3d_fwd: bad args");
  muvo_upsample3d_route_info r;
  upsample3d_route(false, NC, D, H, W, x, y, &r);
  const dim3 grid(r.grid[0], r.grid[1], r.grid[2]), block(r.block[0], r.block[1], r.block[2]);
  if (r.kernel == MUVO_UPSAMPLE_ROW) hipLaunchKernelGGL(upsample3d_x2_fwd_row_kernel, grid, block, 0, ST, x, y, D, H, W);
  else if (r.kernel == MUVO_UPSAMPLE_VEC) hipLaunchKernelGGL(upsample3d_x2_fwd_vec_kernel, grid, block, 0, ST, x, y, D, H, W);
  else hipLaunchKernelGGL(upsample3d_x2_fwd_kernel, grid, block, 0, ST, x, y, (long)NC, D, H, W);
  MUVO_CHECK_LAUNCH("upsample3d_fwd");
  return MUVO_OK;
}
int muvo_upsample3d_x2_bwd(const float* dy, float* dx, int64_t NC, int D, int H, int W, void* stream) {
  MUVO_CHECK_ARG(dy && dx && NC > 0 && D > 0 && H > 0 && W > 0, "upsample3d_bwd: bad args");
  muvo_upsample3d_route_info r;
  upsample3d_route(true, NC, D, H, W, dy, dx, &r);
  const dim3 grid(r.grid[0], r.grid[1], r.grid[2]), block(r.block[0], r.block[1], r.block[2]);
  if (r.kernel == MUVO_UPSAMPLE_ROW) hipLaunchKernelGGL(upsample3d_x2_bwd_row_kernel, grid, block, 0, ST, dy, dx, D, H, W, r.dseg);
  else if (r.kernel == MUVO_UPSAMPLE_VEC) hipLaunchKernelGGL(upsample3d_x2_bwd_vec_kernel, grid, block, 0, ST, dy, dx, D, H, W);
  else hipLaunchKernelGGL(upsample3d_x2_bwd_kernel, grid, block, 0, ST, dy, dx, (long)NC, D, H, W);
  MUVO_CHECK_LAUNCH("upsample3d_bwd");
  return MUVO_OK;
}
int muvo_preprocess_image(const uint8_t* img, float* label, float* norm, int64_t NC, int C, int H, int W, int top, int left,
                          int CH, int CW, const float* mean3, const float* std3, void* stream) {
  MUVO_CHECK_ARG(img && norm && mean3 && std3 && C == 3, "preprocess_image: bad args");
  MUVO_CHECK_ARG(top >= 0 && left >= 0 && top + CH <= H && left + CW <= W, "preprocess_image: crop outside the image");
  return launch_flat("preprocess_image", preprocess_image_kernel, NC * CH * CW, stream, img, label, norm, NC, C, H, W, top, left, CH,
                     CW, norm3_of(mean3, std3));
}
int muvo_preprocess_route(const uint8_t* img, float* norm, int64_t NC, int C, int H, int W, int OH, int OW,
                          const float* mean3, const float* std3, void* stream) {
  MUVO_CHECK_ARG(img && norm && mean3 && std3 && C == 3, "preprocess_route: bad args");
  return launch_flat("preprocess_route", preprocess_route_kernel, NC * OH * OW, stream, img, norm, NC, C, H, W, OH, OW,
                     norm3_of(mean3, std3));
}
int muvo_divide_scalar(const float* x, float* y, int64_t n, float divisor, void* stream) {
  MUVO_CHECK_ARG(x && y && n > 0 && divisor != 0.f, "divide_scalar: bad args");
  return launch_flat("divide_scalar", scale_kernel, n, stream, x, y, n, divisor);
}
int muvo_resize_bilinear(const float* x, float* y, int64_t NC, int H, int W, int OH, int OW, void* stream) {
  MUVO_CHECK_ARG(x && y && NC > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "resize_bilinear: bad args");
  return launch_flat("resize_bilinear", resize_bilinear_kernel, NC * OH * OW, stream, x, y, NC, H, W, OH, OW);
}
int muvo_resize_bilinear_aa(const float* x, float* y, float* ynorm, const float* mean, const float* std, int64_t NC, int C, int H,
                            int W, int OH, int OW, void* stream) {
  MUVO_CHECK_ARG(x && y && NC > 0 && C > 0 && H > 0 && W > 0 && OH > 0 && OW > 0, "resize_bilinear_aa: bad args");
  MUVO_CHECK_ARG(ynorm == nullptr || (mean && std && C <= 3), "resize_bilinear_aa: the normalised copy needs mean / std of <= 3 channels");
  float m[3] = {0.f, 0.f, 0.f}, s[3] = {1.f, 1.f, 1.f};
  if (ynorm) for (int c = 0; c < C; ++c) { m[c] = mean[c]; s[c] = std[c]; }
  return launch_flat("resize_bilinear_aa_kernel", resize_bilinear_aa_kernel, NC * OH * OW, stream, x, y, ynorm, norm3_of(m, s), NC, C, H, W,
                     OH, OW);
}
int muvo_resize_nearest_f32(const float* x, float* y, int64_t NC, int D, int H, int W, int OD, int OH, int OW, void* stream) {
  MUVO_CHECK_ARG(x && y && NC > 0, "resize_nearest_f32: bad args");
  return launch_flat("resize_nearest_f32", resize_nearest_kernel<float>, NC * OD * OH * OW, stream, x, y, NC, D, H, W, OD, OH, OW);
}
int muvo_resize_nearest_u8(const uint8_t* x, uint8_t* y, int64_t NC, int D, int H, int W, int OD, int OH, int OW,
                           void* stream) {
  MUVO_CHECK_ARG(x && y && NC > 0, "resize_nearest_u8: bad args");
  return launch_flat("resize_nearest_u8", resize_nearest_kernel<uint8_t>, NC * OD * OH * OW, stream, x, y, NC, D, H, W, OD, OH, OW);
}
// the MAXV instance of the softmax kernels for a checked row length (SOFTMAX_INSTANCE and muvo_softmax_dropout_route)
static int softmax_dropout_maxv(int cols) { return cols <= 512 ? 8 : SOFTMAX_MAXV; }
int muvo_softmax_dropout_route(int cols) {
  MUVO_CHECK_ARG(cols > 0 && cols <= 64 * SOFTMAX_MAXV, "softmax_route: bad args (cols=%d, max %d)", cols, 64 * SOFTMAX_MAXV);
  return softmax_dropout_maxv(cols);
}
int muvo_softmax_dropout_fwd(const float* S, float* P, float* Pd, int64_t rows, int cols, float p, uint64_t seed,
                             void* stream) {
  MUVO_CHECK_ARG(S && P && rows > 0 && cols > 0 && cols <= 64 * SOFTMAX_MAXV, "softmax_fwd: bad args (cols=%d, max %d)", cols, 64 * SOFTMAX_MAXV);
  hipLaunchKernelGGL(SOFTMAX_INSTANCE(softmax_dropout_fwd_kernel, cols), dim3(cdiv(rows, 4)), dim3(256), 0, ST, S, P, Pd, (long)rows, cols,
                     p, seed);
  MUVO_CHECK_LAUNCH("softmax_fwd");
  return MUVO_OK;
}
int muvo_softmax_dropout_bwd(const float* P, const float* dPd, float* dS, int64_t rows, int cols, float p, uint64_t seed,
                             void* stream) {
  MUVO_CHECK_ARG(P && dPd && dS && rows > 0 && cols > 0 && cols <= 64 * SOFTMAX_MAXV, "softmax_bwd: bad args");
  hipLaunchKernelGGL(SOFTMAX_INSTANCE(softmax_dropout_bwd_kernel, cols), dim3(cdiv(rows, 4)), dim3(256), 0, ST, P, dPd, dS, (long)rows, cols,
                     p, seed);
  MUVO_CHECK_LAUNCH("softmax_bwd");
  return MUVO_OK;
}
int muvo_gru_fwd(const float* gi, const float* gh, const float* h, float* hnew, int B, int H, void* stream) {
  MUVO_CHECK_ARG(gi && gh && h && hnew && B > 0 && H > 0, "gru_fwd: bad args");
  return launch_flat("gru_fwd", gru_fwd_kernel, (long)B * H, stream, gi, gh, h, hnew, B, H);
}
int muvo_gru_bwd(const float* gi, const float* gh, const float* h, const float* dhnew, float* dgi, float* dgh, float* dh,
                 int B, int H, void* stream) {
  MUVO_CHECK_ARG(gi && gh && h && dhnew && dgi && dgh && dh && B > 0 && H > 0, "gru_bwd: bad args");
  return launch_flat("gru_bwd", gru_bwd_kernel, (long)B * H, stream, gi, gh, h, dhnew, dgi, dgh, dh, B, H);
}
int muvo_rssm_sample_fwd(const float* mu_logsigma, const float* eps, int64_t eps_ld, float* mu, float* sigma, float* sample,
                         int B, int S, float min_std, void* stream) {
  MUVO_CHECK_ARG(mu_logsigma && mu && sigma && sample && B > 0 && S > 0, "rssm_sample_fwd: bad args");
  return launch_flat("rssm_sample_fwd", rssm_sample_fwd_kernel, (long)B * S, stream, mu_logsigma, eps, eps_ld, mu, sigma, sample, B, S,
                     min_std);
}
int muvo_rssm_sample_bwd(const float* mu_logsigma, const float* eps, int64_t eps_ld, const float* dmu, const float* dsigma,
                         const float* dsample, float* dmls, int B, int S, void* stream) {
  MUVO_CHECK_ARG(mu_logsigma && dmls && B > 0 && S > 0, "rssm_sample_bwd: bad args");
  return launch_flat("rssm_sample_bwd", rssm_sample_bwd_kernel, (long)B * S, stream, mu_logsigma, eps, eps_ld, dmu, dsigma, dsample, dmls,
                     B, S);
}

}  // extern "C"

// ================================================================================== not an element-wise operation of the model
// Stand-in for the local footprint of a ring all-reduce on a one-GPU box (include/muvo_hip.h: muvo_fake_allreduce)
__global__ void __launch_bounds__(256) fake_allreduce_kernel(f32x4* __restrict__ buf, long n4, int sleep) {
  const long stride = (long)gridDim.x * 256;
  for (long i0 = (long)blockIdx.x * 256; i0 < n4; i0 += 4 * stride) {
    f32x4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = i0 + u * stride + threadIdx.x;
      const long ic = i < n4 ? i : 0;
      a[u] = __builtin_nontemporal_load(buf + ic);
      b[u] = *(volatile f32x4*)(buf + ic);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long i = i0 + u * stride + threadIdx.x;
      if (i < n4) __builtin_nontemporal_store(0.5f * (a[u] + b[u]), buf + i);
    }
    for (int k = 0; k < sleep; ++k) __builtin_amdgcn_s_sleep(1);
  }
}
extern "C" int muvo_fake_allreduce(float* buf, int64_t n, int workgroups, int sleep, void* stream) {
  MUVO_CHECK_ARG(buf && n > 0 && n % 4 == 0 && ((uintptr_t)buf & 15) == 0, "fake_allreduce: n %% 4 == 0 and a 16-byte aligned buffer");
  MUVO_CHECK_ARG(workgroups >= 1 && workgroups <= 256 && sleep >= 0 && sleep <= 100000, "fake_allreduce: bad launch parameters");
  hipLaunchKernelGGL(fake_allreduce_kernel, dim3(workgroups), dim3(256), 0, ST, (f32x4*)buf, (long)(n / 4), sleep);
  MUVO_CHECK_LAUNCH("fake_allreduce_kernel");
  return MUVO_OK;
}
