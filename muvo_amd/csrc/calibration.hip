// Calibration and uncertainty of an ensemble of class-logit samples against a label grid (an extension; the
// definitions: include/muvo_hip.h, muvo_voxel_calibration).  One pass for gfx950: every logit is read once (again only for the
// rare voxel whose decision is re-taken in fp64, CAL_CLOSE below), what leaves is a few hundred bytes of integer counters and, on
// request, byte maps.  Measured at 0.7 - 2.2 TB/s of logits: bound by the per-voxel arithmetic, not by HBM.
//
// Shape.  z is the contiguous axis and the top-view maps are maxima over z, so the unit of work is a z-column.  A wave owns
// 64 / ZP columns at a time, ZP = the power of two >= min(Z, 64): lane = slot * ZP + zl reads voxel z = z0 + zl of column
// `slot` (Z = 64: one column per wave, 256 contiguous bytes per class plane; Z = 7: eight columns per wave, 56 of 64 lanes busy;
// Z > 64: the column in rounds of 64).  The C logits of one sample and the running mean probability live in registers (C is a
// template parameter: every class loop is unrolled, nothing is indexed at run time, no scratch).  Every accumulator is an integer:
// the per-lane ones (counts, completion counts, the six fixed-point sums) stay in registers over the whole grid-stride loop and are
// reduced by wave shuffles at the end; the two histograms (reliability table by bin, SSC counts by class) go through 64-bit LDS
// atomics; each workgroup ends with one 64-bit global atomic per non-zero word.  Integer sums are order-free: the same bits on
// every call, in every mode.
#include "common.h"

#define CAL_MAXC 16
#define CAL_MAXK 8
#define CAL_MAXB 32
#define CAL_THREADS 256
#define CAL_MAX_BLOCKS 2048
#define CAL_FIX 16777216.f            // 2^24: the unit of the fixed-point sums
#define CAL_NLANE 13                  // per-lane accumulators: counts[4], completion[3], sums[6]
// A decision - which class is the maximum, which bin holds conf - that fp32 rounding could turn (fp32 softmax means of <= 16 classes
// are good to ~1e-6) is taken again in fp64: the integer outputs then do not depend on fp32 rounding and equal a float64 reference.
#define CAL_CLOSE 1e-5f

struct CalSamples { const float* p[CAL_MAXK]; };

// -sum p ln p with 0 ln 0 = 0, classes in ascending order
template <int C>
__device__ __forceinline__ float cal_entropy(const float* p) {
  float h = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) h -= p[c] > 0.f ? p[c] * logf(p[c]) : 0.f;
  return h;
}

__device__ __forceinline__ unsigned long long cal_fix(float v) { return (unsigned long long)(unsigned int)rintf(fmaxf(v, 0.f) * CAL_FIX); }
__device__ __forceinline__ int cal_byte(float v, float inv_lnc) { return (int)rintf(255.f * fminf(1.f, v * inv_lnc)); }

__device__ __forceinline__ unsigned long long cal_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}

template <int C>
__global__ void __launch_bounds__(CAL_THREADS)
calibration_kernel(CalSamples s, int K, const unsigned char* __restrict__ label, long ncols, long XY, int Z, int ZP, int B, float inv_lnc,
                   unsigned long long* __restrict__ table, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ ssc,
                   unsigned long long* __restrict__ sums, unsigned char* __restrict__ ens, unsigned char* __restrict__ top_h,
                   unsigned char* __restrict__ top_mi) {
  __shared__ unsigned long long ltab[CAL_MAXB * 3], lssc[3 * CAL_MAXC], lacc[CAL_NLANE];
  for (int i = threadIdx.x; i < CAL_MAXB * 3; i += CAL_THREADS) ltab[i] = 0ull;
  for (int i = threadIdx.x; i < 3 * CAL_MAXC; i += CAL_THREADS) lssc[i] = 0ull;
  if (threadIdx.x < CAL_NLANE) lacc[threadIdx.x] = 0ull;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cpw = 64 / ZP, slot = lane / ZP, zl = lane - slot * ZP;
  const long V = XY * Z;
  const bool maps = top_h != nullptr || top_mi != nullptr;
  const float fK = (float)K;
  // [0] voxels [1] ignored [2] skipped_nonfinite [3] correct [4..6] completion tp fp fn [7..12] brier nll Hc Hw MIc MIw
  unsigned long long acc[CAL_NLANE];
#pragma unroll
  for (int i = 0; i < CAL_NLANE; ++i) acc[i] = 0ull;
  const long ngroups = (ncols + cpw - 1) / cpw;
  // g is the same in every lane of a wave: all 64 lanes run every round, so the shuffles below always see whole waves
  for (long g = blockIdx.x * (long)(CAL_THREADS / 64) + wave; g < ngroups; g += (long)gridDim.x * (CAL_THREADS / 64)) {
    const long col = g * cpw + slot;
    const bool col_ok = col < ncols;
    const long f = col_ok ? col / XY : 0, cxy = col_ok ? col - f * XY : 0;
    int hmax = 0, mimax = 0;
    for (int z0 = 0; z0 < Z; z0 += ZP) {
      const int z = z0 + zl;
      if (!(col_ok && z < Z)) continue;                       // no shuffle inside this loop
      const size_t vi = (size_t)col * Z + z;
      const int tl = label[vi];
      if (tl == 255) {
        acc[1] += 1ull;
        if (ens) ens[vi] = 255;
        if (!maps) continue;
      }
      const size_t off = (size_t)f * C * V + (size_t)cxy * Z + z;
      float pbar[C];
#pragma unroll
      for (int c = 0; c < C; ++c) pbar[c] = 0.f;
      float ebar = 0.f;
      bool bad = false;
      int am = 0;                                             // argmax of the logits of the last sample (used at K == 1)
      for (int k = 0; k < K; ++k) {
        const float* q;
        switch (k) {                                          // a run-time index into a by-value argument would go through scratch
          case 0: q = s.p[0]; break;
          case 1: q = s.p[1]; break;
          case 2: q = s.p[2]; break;
          case 3: q = s.p[3]; break;
          case 4: q = s.p[4]; break;
          case 5: q = s.p[5]; break;
          case 6: q = s.p[6]; break;
          default: q = s.p[7]; break;
        }
        q += off;
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = q[(size_t)c * V];
        float m = x[0];
        bool nan = x[0] != x[0];
        am = 0;
#pragma unroll
        for (int c = 1; c < C; ++c) {
          nan = nan || x[c] != x[c];
          if (x[c] > m) { m = x[c]; am = c; }
        }
        bad = bad || nan || m == INFINITY || m == -INFINITY;
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) { x[c] = expf(x[c] - m); sum += x[c]; }
        const float inv = 1.f / sum;
#pragma unroll
        for (int c = 0; c < C; ++c) { x[c] *= inv; pbar[c] += x[c]; }
        ebar += cal_entropy<C>(x);
      }
      if (bad) {                                              // contributes to nothing else; map bytes stay 0
        if (tl != 255) { acc[2] += 1ull; if (ens) ens[vi] = 255; }
        continue;
      }
#pragma unroll
      for (int c = 0; c < C; ++c) pbar[c] = pbar[c] / fK;
      const float H = cal_entropy<C>(pbar), mi = fmaxf(0.f, H - ebar / fK);
      if (top_h) hmax = max(hmax, cal_byte(H, inv_lnc));
      if (top_mi) mimax = max(mimax, cal_byte(mi, inv_lnc));
      if (tl == 255) continue;
      int pr = 0;
      float conf = pbar[0], second = -1.f;
#pragma unroll
      for (int c = 1; c < C; ++c) {
        if (pbar[c] > conf) { second = conf; conf = pbar[c]; pr = c; }
        else second = fmaxf(second, pbar[c]);
      }
      const float scaled = conf * (float)B;
      int bin = (int)floorf(scaled);
      if (conf - second < CAL_CLOSE || fabsf(scaled - rintf(scaled)) < CAL_CLOSE * (float)B) {      // rare: decide in fp64
        double pd[C];
#pragma unroll
        for (int c = 0; c < C; ++c) pd[c] = 0.0;
        for (int k = 0; k < K; ++k) {
          const float* q;
          switch (k) {
            case 0: q = s.p[0]; break;
            case 1: q = s.p[1]; break;
            case 2: q = s.p[2]; break;
            case 3: q = s.p[3]; break;
            case 4: q = s.p[4]; break;
            case 5: q = s.p[5]; break;
            case 6: q = s.p[6]; break;
            default: q = s.p[7]; break;
          }
          q += off;
          float x[C];
#pragma unroll
          for (int c = 0; c < C; ++c) x[c] = q[(size_t)c * V];
          float m = x[0];
#pragma unroll
          for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
          double sum = 0.0;
#pragma unroll
          for (int c = 0; c < C; ++c) sum += exp((double)x[c] - (double)m);
          const double inv = 1.0 / sum;
#pragma unroll
          for (int c = 0; c < C; ++c) pd[c] += exp((double)x[c] - (double)m) * inv;
        }
        double cd = pd[0];
        pr = 0;
#pragma unroll
        for (int c = 1; c < C; ++c)
          if (pd[c] > cd) { cd = pd[c]; pr = c; }
        bin = (int)floor(cd / (double)K * (double)B);
      }
      if (K == 1) pr = am;                                    // exp is monotone: the logits' first maximum is a maximum of p, and it
                                                              // is the prediction of muvo_ssc_counts whatever rounding made equal
#pragma unroll
      for (int c = 0; c < C; ++c) conf = c == pr ? pbar[c] : conf;
      float py = 0.f, brier = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float d = pbar[c] - (c == tl ? 1.f : 0.f);
        brier += d * d;
        py = c == tl ? pbar[c] : py;
      }
      const float nll = py > 1e-12f ? -logf(py) : 27.631021115928547f;      // at the floor: -ln 1e-12, rounded once
      const bool ok = pr == tl;
      if (ens) ens[vi] = (unsigned char)pr;
      acc[0] += 1ull;
      acc[3] += ok ? 1ull : 0ull;
      acc[7] += cal_fix(brier);
      acc[8] += cal_fix(nll);
      const unsigned long long hq = cal_fix(H), mq = cal_fix(mi);
      acc[9] += ok ? hq : 0ull;  acc[10] += ok ? 0ull : hq;
      acc[11] += ok ? mq : 0ull; acc[12] += ok ? 0ull : mq;
      bin = bin > B - 1 ? B - 1 : bin;
      atomicAdd(&ltab[3 * bin], 1ull);
      if (ok) atomicAdd(&ltab[3 * bin + 1], 1ull);
      atomicAdd(&ltab[3 * bin + 2], cal_fix(conf));
      // the counting rule of ssc_counts_kernel (metrics.hip), on pr
      if (tl > 0 && pr > 0) acc[4] += 1ull;
      else if (tl == 0 && pr > 0) acc[5] += 1ull;
      else if (tl > 0 && pr == 0) acc[6] += 1ull;
      if (ok) atomicAdd(&lssc[3 * tl], 1ull);
      else {
        atomicAdd(&lssc[3 * pr + 1], 1ull);
        if (tl < C) atomicAdd(&lssc[3 * tl + 2], 1ull);
      }
    }
    if (maps) {                                               // maximum over the ZP lanes of a column
      for (int o = ZP >> 1; o > 0; o >>= 1) {
        hmax = max(hmax, __shfl_xor(hmax, o, 64));
        mimax = max(mimax, __shfl_xor(mimax, o, 64));
      }
      if (col_ok && zl == 0) {
        if (top_h) top_h[col] = (unsigned char)hmax;
        if (top_mi) top_mi[col] = (unsigned char)mimax;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CAL_NLANE; ++i) {
    const unsigned long long v = cal_wave_sum(acc[i]);
    if (lane == 0 && v) atomicAdd(&lacc[i], v);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * B; i += CAL_THREADS)
    if (ltab[i]) atomicAdd(table + i, ltab[i]);
  for (int i = threadIdx.x; i < 3 * C; i += CAL_THREADS)
    if (lssc[i]) atomicAdd(ssc + 3 + i, lssc[i]);
  if (threadIdx.x < CAL_NLANE && lacc[threadIdx.x]) {
    const int i = threadIdx.x;
    atomicAdd(i < 4 ? counts + i : i < 7 ? ssc + (i - 4) : sums + (i - 7), lacc[i]);
  }
}

extern "C" {

int muvo_voxel_calibration(const float* const* logits, int K, const uint8_t* label, int64_t F, int C, int X, int Y, int Z, int B,
                           int64_t* table, int64_t* counts, uint64_t* ssc, int64_t* sums, uint8_t* ens, uint8_t* top_entropy, uint8_t* top_mi,
                           void* stream) {
  MUVO_CHECK_ARG(K >= 1 && K <= CAL_MAXK, "voxel_calibration: K=%d samples unsupported (1..%d)", K, CAL_MAXK);
  MUVO_CHECK_ARG(C >= 2 && C <= CAL_MAXC, "voxel_calibration: C=%d unsupported (2..%d)", C, CAL_MAXC);
  MUVO_CHECK_ARG(B >= 1 && B <= CAL_MAXB, "voxel_calibration: B=%d bins unsupported (1..%d)", B, CAL_MAXB);
  MUVO_CHECK_ARG(F >= 1, "voxel_calibration: F=%ld frames (need >= 1)", (long)F);
  MUVO_CHECK_ARG(X >= 1 && Y >= 1 && Z >= 1, "voxel_calibration: grid X=%d Y=%d Z=%d (need >= 1 each)", X, Y, Z);
  const long XY = (long)X * Y;
  MUVO_CHECK_ARG(XY <= (1L << 40) / Z && F <= (1L << 40) / (XY * Z), "voxel_calibration: F*X*Y*Z = %ld x %d x %d x %d exceeds 2^40 voxels",
                 (long)F, X, Y, Z);
  MUVO_CHECK_ARG(logits != nullptr, "voxel_calibration: logits is null");
  CalSamples s;
  for (int k = 0; k < CAL_MAXK; ++k) {
    MUVO_CHECK_ARG(k >= K || logits[k] != nullptr, "voxel_calibration: logits[%d] is null", k);
    s.p[k] = k < K ? logits[k] : nullptr;
  }
  MUVO_CHECK_ARG(label != nullptr, "voxel_calibration: label is null");
  MUVO_CHECK_ARG(table != nullptr, "voxel_calibration: table is null");
  MUVO_CHECK_ARG(counts != nullptr, "voxel_calibration: counts is null");
  MUVO_CHECK_ARG(ssc != nullptr, "voxel_calibration: ssc is null");
  MUVO_CHECK_ARG(sums != nullptr, "voxel_calibration: sums is null");
  int ZP = 1;
  while (ZP < Z && ZP < 64) ZP <<= 1;
  const long ncols = (long)F * XY, ngroups = (ncols + 64 / ZP - 1) / (64 / ZP);
  long nb = (ngroups + CAL_THREADS / 64 - 1) / (CAL_THREADS / 64);
  if (nb > CAL_MAX_BLOCKS) nb = CAL_MAX_BLOCKS;
  const float inv_lnc = 1.f / logf((float)C);
  switch (C) {
#define CAL_CASE(c)                                                                                                                  \
  case c:                                                                                                                            \
    hipLaunchKernelGGL((calibration_kernel<c>), dim3((int)nb), dim3(CAL_THREADS), 0, (hipStream_t)stream, s, K, label, ncols, XY, Z, ZP, B, \
                       inv_lnc, (unsigned long long*)table, (unsigned long long*)counts, (unsigned long long*)ssc,                  \
                       (unsigned long long*)sums, ens, top_entropy, top_mi);                                                         \
    break;
    CAL_CASE(2) CAL_CASE(3) CAL_CASE(4) CAL_CASE(5) CAL_CASE(6) CAL_CASE(7) CAL_CASE(8) CAL_CASE(9) CAL_CASE(10)
    CAL_CASE(11) CAL_CASE(12) CAL_CASE(13) CAL_CASE(14) CAL_CASE(15) CAL_CASE(16)
#undef CAL_CASE
  }
  MUVO_CHECK_LAUNCH("calibration_kernel");
  return MUVO_OK;
}

}  // extern "C"
