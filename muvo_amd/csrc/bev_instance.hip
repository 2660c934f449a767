// BEV instances from the centre / offset heads and their panoptic quality (extensions).  include/muvo_hip.h
// (muvo_bev_instance_decode, muvo_bev_pq_counts) holds the definitions; tests/bev_instance_reference.py restates them.
//
// Decode, 3 launches after one memset of the per-frame counters, frames along grid.y:
//   peaks    one thread per pixel: a peak appends its 64-bit key to the frame's candidate list (an integer atomic gives the slot;
//            the ORDER of the list is arbitrary, the SET is not, and nothing below depends on the order)
//   select   one workgroup per frame: the K-th largest key by an 8-bit radix select over the list (LDS histogram), the keys at or
//            above it gathered in LDS and ranked among themselves.  Keys are unique (they hold the pixel index), so the result
//            does not depend on the list's order: score descending, then row-major index ascending
//   group    one thread per pixel, the frame's centres in LDS: foreground test, nearest centre to pixel + offset
// Counting, 3 launches after one memset of the overlap tables:
//   overlap  one thread per pixel: n[g][q] += 1 in the frame's 256 x 256 table in global scratch (integer atomics; the pair (0, 0)
//            is never needed and is skipped)
//   match    one workgroup per frame: row and column sums = the areas, the matches, integer atomics into the caller's counts,
//            the frame's fp64 IoU sum (added in a fixed order) into a slot of its own
//   sum      one wave adds the slots in a fixed order into the caller's fp64 accumulator
#include "common.h"

#define BI_THREADS 256
#define BI_SELECT_THREADS 1024
#define BI_MAXK 254
#define BI_MAXDIM 4096
#define BI_MAXPIX (1 << 24)

// fp32 -> uint32 whose unsigned order is the float order; -0 and +0 get one key (the caller adds 0.f first)
__device__ __forceinline__ uint32_t bi_order(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(BI_THREADS)
bi_peaks_kernel(const float* __restrict__ center, int H, int W, float threshold, int radius, unsigned* __restrict__ count,
                unsigned long long* __restrict__ cand) {
  const long HW = (long)H * W, f = blockIdx.y;
  const long p = (long)blockIdx.x * BI_THREADS + threadIdx.x;
  if (p >= HW) return;
  const float* c = center + f * HW;
  const float v = c[p];
  if (!(v > threshold)) return;                     // a NaN is never a peak
  const int y = (int)(p / W), x = (int)(p % W);
  const int y0 = max(y - radius, 0), y1 = min(y + radius, H - 1), x0 = max(x - radius, 0), x1 = min(x + radius, W - 1);
  bool peak = true;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx) peak = peak && !(c[(long)yy * W + xx] > v);      // a NaN neighbour never suppresses
  if (!peak) return;
  const unsigned slot = atomicAdd(&count[f], 1u);   // < HW: a pixel appends once
  cand[f * HW + slot] = ((unsigned long long)bi_order(v + 0.f) << 32) | (unsigned long long)(0xffffffffu - (unsigned)p);
}

__global__ void __launch_bounds__(BI_SELECT_THREADS)
bi_select_kernel(const unsigned* __restrict__ count, const unsigned long long* __restrict__ cand, long HW, int W, int K, int32_t* __restrict__ centres,
                 int32_t* __restrict__ n_out, int32_t* __restrict__ capped) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long win[256];
  __shared__ unsigned sel, remaining, nwin;
  const long f = blockIdx.x;
  const unsigned n = min(count[f], (unsigned)HW);
  const unsigned long long* list = cand + f * HW;
  const int kept = (int)min(n, (unsigned)K);
  unsigned long long thresh = 0ull;
  if (n > (unsigned)K) {                            // the K-th largest key, 8 bits a round from the top
    unsigned long long prefix = 0ull, mask = 0ull;
    if (threadIdx.x == 0) remaining = (unsigned)K;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
      __syncthreads();
      for (unsigned i = threadIdx.x; i < n; i += BI_SELECT_THREADS) {
        const unsigned long long key = list[i];
        if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        unsigned acc = 0u, want = remaining;
        int b = 255;
        for (; b > 0; --b) {
          if (acc + hist[b] >= want) break;
          acc += hist[b];
        }
        sel = (unsigned)b;
        remaining = want - acc;
      }
      __syncthreads();
      prefix |= (unsigned long long)sel << shift;
      mask |= 0xffull << shift;
    }
    thresh = prefix;
  }
  if (threadIdx.x == 0) nwin = 0u;
  __syncthreads();
  for (unsigned i = threadIdx.x; i < n; i += BI_SELECT_THREADS) {
    const unsigned long long key = list[i];
    if (key >= thresh) {
      const unsigned slot = atomicAdd(&nwin, 1u);
      if (slot < 256u) win[slot] = key;             // exactly `kept` keys pass: the keys are unique
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    int32_t* out = centres + (f * K) * 2;
    if ((int)threadIdx.x < kept) {
      const unsigned long long key = win[threadIdx.x];
      int rank = 0;
      for (int j = 0; j < kept; ++j) rank += win[j] > key;
      const unsigned p = 0xffffffffu - (unsigned)(key & 0xffffffffull);
      out[rank * 2] = (int32_t)(p / (unsigned)W);
      out[rank * 2 + 1] = (int32_t)(p % (unsigned)W);
    } else {
      out[threadIdx.x * 2] = -1;
      out[threadIdx.x * 2 + 1] = -1;
    }
  }
  if (threadIdx.x == 0) {
    n_out[f] = kept;
    capped[f] = n > (unsigned)K ? 1 : 0;
  }
}

// foreground of one pixel from the logits: the first maximum over the classes (upward, replaced on strictly greater: a NaN never
// replaces the running maximum) is a thing class
__device__ __forceinline__ bool bi_foreground(const float* __restrict__ logits, long HW, long p, int C, uint32_t things) {
  float best = logits[p];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = logits[(long)c * HW + p];
    if (v > best) {
      best = v;
      arg = c;
    }
  }
  return (things >> arg) & 1u;
}

__global__ void __launch_bounds__(BI_THREADS)
bi_group_kernel(const float* __restrict__ offset, const float* __restrict__ logits, int C, uint32_t things, const uint8_t* __restrict__ foreground,
                int H, int W, int K, const int32_t* __restrict__ centres, const int32_t* __restrict__ n_in, uint8_t* __restrict__ ids) {
  __shared__ float cy[256], cx[256];
  const long HW = (long)H * W, f = blockIdx.y;
  const int n = min(n_in[f], K);
  if ((int)threadIdx.x < n) {
    cy[threadIdx.x] = (float)centres[(f * K + threadIdx.x) * 2];
    cx[threadIdx.x] = (float)centres[(f * K + threadIdx.x) * 2 + 1];
  }
  __syncthreads();
  const long p = (long)blockIdx.x * BI_THREADS + threadIdx.x;
  if (p >= HW) return;
  const bool fg = logits ? bi_foreground(logits + f * C * HW, HW, p, C, things) : foreground[f * HW + p] != 0;
  int id = 0;
  if (fg && n > 0) {
    const float ty = (float)(int)(p / W) + offset[(f * 2) * HW + p];
    const float tx = (float)(int)(p % W) + offset[(f * 2 + 1) * HW + p];
    float best = __builtin_inff();
    for (int k = 0; k < n; ++k) {
      const float dy = ty - cy[k], dx = tx - cx[k];
      const float d = dy * dy + dx * dx;           // -ffp-contract=off: two products, one sum
      if (d < best) {                              // a NaN or an infinite distance never wins; the lowest k wins a tie
        best = d;
        id = k + 1;
      }
    }
  }
  ids[f * HW + p] = (uint8_t)id;
}

// ---- panoptic quality ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BI_THREADS)
pq_overlap_kernel(const uint8_t* __restrict__ label, const uint8_t* __restrict__ pred, long HW, unsigned* __restrict__ table) {
  const long f = blockIdx.y;
  unsigned* tab = table + f * 65536;
  for (long p = (long)blockIdx.x * BI_THREADS + threadIdx.x; p < HW; p += (long)gridDim.x * BI_THREADS) {
    const unsigned g = label[f * HW + p], q = pred[f * HW + p];
    if (g | q) atomicAdd(&tab[g * 256u + q], 1u);
  }
}

// counts: [0] frames, [1] capped frames, [2] label segments, [3] predicted segments, [4] tp, [5] fp, [6] fn.  Thread t owns column
// t (predicted id t); the rows (label ids) are walked in order.
__global__ void __launch_bounds__(BI_THREADS)
pq_match_kernel(const unsigned* __restrict__ table, const int32_t* __restrict__ capped, unsigned long long* __restrict__ counts, double* __restrict__ part) {
  __shared__ unsigned area[256], cnt[3];
  __shared__ double red[BI_THREADS / 64];
  const long f = blockIdx.x;
  const unsigned* tab = table + f * 65536;
  const int t = threadIdx.x, lane = t & 63;
  area[t] = 0u;
  if (t < 3) cnt[t] = 0u;
  __syncthreads();
  unsigned b = 0u;                                  // area of predicted segment t
  for (int r = 0; r < 256; ++r) {
    const unsigned v = tab[r * 256 + t];
    b += v;
    unsigned s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && s) atomicAdd(&area[r], s);
  }
  __syncthreads();
  double iou = 0.0;
  unsigned matched = 0u;
  if (t > 0 && b > 0u) {
    for (int r = 1; r < 256; ++r) {
      const unsigned nij = tab[r * 256 + t], a = area[r];
      if (nij > 0u && 3ull * nij > (unsigned long long)a + b) {          // IoU > 1/2: at most one r per t and one t per r
        matched = 1u;
        iou += (double)nij / (double)((unsigned long long)a + b - nij);
      }
    }
  }
  const unsigned is_label = (t > 0 && area[t] > 0u) ? 1u : 0u, is_pred = (t > 0 && b > 0u) ? 1u : 0u;
  unsigned c0 = is_label, c1 = is_pred, c2 = matched;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64);
    c1 += __shfl_xor(c1, o, 64);
    c2 += __shfl_xor(c2, o, 64);
  }
  iou = wave_sum_d(iou);
  if (lane == 0) {
    atomicAdd(&cnt[0], c0);
    atomicAdd(&cnt[1], c1);
    atomicAdd(&cnt[2], c2);
    red[t >> 6] = iou;
  }
  __syncthreads();
  if (t == 0) {
    const unsigned nl = cnt[0], np = cnt[1], tp = cnt[2];
    atomicAdd(&counts[0], 1ull);
    if (capped && capped[f]) atomicAdd(&counts[1], 1ull);
    if (nl) atomicAdd(&counts[2], (unsigned long long)nl);
    if (np) atomicAdd(&counts[3], (unsigned long long)np);
    if (tp) atomicAdd(&counts[4], (unsigned long long)tp);
    if (np - tp) atomicAdd(&counts[5], (unsigned long long)(np - tp));
    if (nl - tp) atomicAdd(&counts[6], (unsigned long long)(nl - tp));
    part[f] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// one wave: lane l adds the slots l, l + 64, ... in order, the lanes are added by a fixed butterfly, sum[0] += total
__global__ void __launch_bounds__(64) pq_sum_kernel(const double* __restrict__ part, long P, double* __restrict__ sum) {
  double s = 0.0;
  for (long p = threadIdx.x; p < P; p += 64) s += part[p];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) sum[0] += s;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

static inline bool bi_sizes_ok(int64_t F, int H, int W) {
  return F >= 1 && F <= 65535 && H >= 1 && W >= 1 && H <= BI_MAXDIM && W <= BI_MAXDIM && (int64_t)H * W <= BI_MAXPIX;
}
static inline int64_t bi_count_bytes(int64_t F) { return (F * 4 + 7) & ~(int64_t)7; }

extern "C" {

int64_t muvo_bev_instance_ws_bytes(int64_t F, int H, int W) {
  if (!bi_sizes_ok(F, H, W)) return -1;
  return bi_count_bytes(F) + F * (int64_t)H * W * 8;
}

int muvo_bev_instance_decode(const float* center, const float* offset, const float* logits, int C, uint32_t things, const uint8_t* foreground, int64_t F,
                             int H, int W, float threshold, int radius, int K, void* ws, int64_t ws_bytes, uint8_t* ids, int32_t* centres, int32_t* n,
                             int32_t* capped, void* stream) {
  MUVO_CHECK_ARG(bi_sizes_ok(F, H, W), "bev_instance_decode: %lld frames of %d x %d (1..65535 frames, 1..%d a side, at most 2^24 pixels)", (long long)F, H,
                 W, BI_MAXDIM);
  MUVO_CHECK_ARG(K >= 1 && K <= BI_MAXK, "bev_instance_decode: %d centres outside 1..%d", K, BI_MAXK);
  MUVO_CHECK_ARG(radius >= 1 && radius <= 3, "bev_instance_decode: radius %d outside 1..3", radius);
  MUVO_CHECK_ARG(threshold == threshold, "bev_instance_decode: the threshold is NaN");
  MUVO_CHECK_ARG((logits != nullptr) != (foreground != nullptr), "bev_instance_decode: either logits or a foreground mask");
  MUVO_CHECK_ARG(!logits || (C >= 2 && C <= 32), "bev_instance_decode: %d classes outside 2..32", C);
  MUVO_CHECK_ARG(center && offset && ids && centres && n && capped, "bev_instance_decode: null pointer");
  const int64_t need = muvo_bev_instance_ws_bytes(F, H, W);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need, "bev_instance_decode: workspace of %lld bytes, %lld needed (8-byte aligned)",
                 (long long)ws_bytes, (long long)need);
  MUVO_CHECK_ARG((((uintptr_t)center | (uintptr_t)offset | (uintptr_t)logits | (uintptr_t)centres | (uintptr_t)n | (uintptr_t)capped) & 3) == 0,
                 "bev_instance_decode: a 32-bit buffer is not 4-byte aligned");
  unsigned* count = (unsigned*)ws;
  unsigned long long* cand = (unsigned long long*)((char*)ws + bi_count_bytes(F));
  if (hipMemsetAsync(count, 0, (size_t)bi_count_bytes(F), ST) != hipSuccess) {
    muvo_set_error("bev_instance_decode: memset failed");
    return MUVO_ERR_HIP;
  }
  const long HW = (long)H * W;
  const dim3 grid((unsigned)cdiv(HW, BI_THREADS), (unsigned)F);
  hipLaunchKernelGGL(bi_peaks_kernel, grid, dim3(BI_THREADS), 0, ST, center, H, W, threshold, radius, count, cand);
  hipLaunchKernelGGL(bi_select_kernel, dim3((unsigned)F), dim3(BI_SELECT_THREADS), 0, ST, (const unsigned*)count, (const unsigned long long*)cand, HW, W, K,
                     centres, n, capped);
  hipLaunchKernelGGL(bi_group_kernel, grid, dim3(BI_THREADS), 0, ST, offset, logits, C, things, foreground, H, W, K, (const int32_t*)centres,
                     (const int32_t*)n, ids);
  MUVO_CHECK_LAUNCH("bev_instance_decode");
  return MUVO_OK;
}

int64_t muvo_bev_pq_ws_bytes(int64_t F) {
  if (F < 1 || F > 65535) return -1;
  return F * (65536 * 4 + 8);
}

int muvo_bev_pq_counts(const uint8_t* label, const uint8_t* pred, const int32_t* capped, int64_t F, int H, int W, uint64_t* counts, double* iou_sum, void* ws,
                       int64_t ws_bytes, void* stream) {
  MUVO_CHECK_ARG(bi_sizes_ok(F, H, W), "bev_pq_counts: %lld frames of %d x %d (1..65535 frames, 1..%d a side, at most 2^24 pixels)", (long long)F, H, W,
                 BI_MAXDIM);
  MUVO_CHECK_ARG(label && pred && counts && iou_sum, "bev_pq_counts: null pointer");
  const int64_t need = muvo_bev_pq_ws_bytes(F);
  MUVO_CHECK_ARG(ws != nullptr && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need, "bev_pq_counts: workspace of %lld bytes, %lld needed (8-byte aligned)",
                 (long long)ws_bytes, (long long)need);
  MUVO_CHECK_ARG((((uintptr_t)counts | (uintptr_t)iou_sum) & 7) == 0 && ((uintptr_t)capped & 3) == 0,
                 "bev_pq_counts: the accumulators are not 8-byte aligned or the capped flags are not 4-byte aligned");
  double* part = (double*)ws;                       // F slots, then the F tables
  unsigned* table = (unsigned*)(part + F);
  if (hipMemsetAsync(table, 0, (size_t)F * 65536 * 4, ST) != hipSuccess) {
    muvo_set_error("bev_pq_counts: memset failed");
    return MUVO_ERR_HIP;
  }
  const long HW = (long)H * W;
  const int nb = cdiv(HW, BI_THREADS) < 256 ? cdiv(HW, BI_THREADS) : 256;
  hipLaunchKernelGGL(pq_overlap_kernel, dim3((unsigned)nb, (unsigned)F), dim3(BI_THREADS), 0, ST, label, pred, HW, table);
  hipLaunchKernelGGL(pq_match_kernel, dim3((unsigned)F), dim3(BI_THREADS), 0, ST, (const unsigned*)table, capped, (unsigned long long*)counts, part);
  hipLaunchKernelGGL(pq_sum_kernel, dim3(1), dim3(64), 0, ST, (const double*)part, (long)F, iou_sum);
  MUVO_CHECK_LAUNCH("bev_pq_counts");
  return MUVO_OK;
}

}  // extern "C"
