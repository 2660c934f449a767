// Prediction export on the device (muvo_amd/predict.py): what the reference's sim_run.py:75-92 does on the host after copying
// whole tensors over - torch.argmax + torch.where on the voxel logits, `(image * 255).astype(np.uint8)` on the float images.
//   occupied-voxel rows: class argmax fused with an ordered stream compaction, the layout of voxelize.hip's label -> scan ->
//     rows passes.  The logits are read once; one class byte per voxel is written and read back; what leaves is (Q, 4) uint16.
//   image bytes: fp32 -> uint8 with the product's saturation rule.
// Both are pure streaming: HBM-bound, no LDS beyond a few counters, no atomics - the result is independent of the execution order.
#include <algorithm>

#include "common.h"

#define EXP_CHUNK 2048          // voxels per workgroup: 256 threads x 8
#define EXP_MAXC 16             // the SSC_MAXC limit of ssc_counts_kernel (metrics.hip)

__device__ __forceinline__ void exp_chunk_count(int n, int32_t* __restrict__ cnt, int nblk, int* wsum) {
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;            // n is wave-uniform (sums of ballot popcounts)
  __syncthreads();
  if (threadIdx.x == 0) cnt[(long)blockIdx.y * nblk + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 1, logits: cls[f][h] = first maximum over the C planes (strict >: torch.argmax on finite input, ssc_counts_kernel),
// cnt[f][chunk] = voxels of the chunk with a class != 0.  A thread owns 4 consecutive voxels of each half chunk: 16-byte loads
// per plane when V % 4 == 0 and the base is aligned (vec), one 4-byte store of the class bytes either way (the frame stride Vp
// of cls is a multiple of 16; bytes between V and Vp are written as 0 and never read).
__global__ void __launch_bounds__(256)
export_classify_kernel(const float* __restrict__ logits, int C, long V, long Vp, int nblk, int vec, uint8_t* __restrict__ cls,
                       int32_t* __restrict__ cnt) {
  __shared__ int wsum[4];
  const long f = blockIdx.y;
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  int n = 0;
#pragma unroll
  for (int k = 0; k < EXP_CHUNK / 1024; ++k) {
    const long h0 = (long)blockIdx.x * EXP_CHUNK + (long)(k * 256 + threadIdx.x) * 4;
    unsigned p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    if (vec && h0 + 3 < V) {
      f32x4 b = *(const f32x4*)(lf + h0);
      for (int c = 1; c < C; ++c) {
        const f32x4 x = *(const f32x4*)(lf + (size_t)c * V + h0);
        if (x.x > b.x) { b.x = x.x; p0 = c; }
        if (x.y > b.y) { b.y = x.y; p1 = c; }
        if (x.z > b.z) { b.z = x.z; p2 = c; }
        if (x.w > b.w) { b.w = x.w; p3 = c; }
      }
    } else if (h0 < V) {
      const bool v1 = h0 + 1 < V, v2 = h0 + 2 < V, v3 = h0 + 3 < V;
      float b0 = lf[h0], b1 = v1 ? lf[h0 + 1] : 0.f, b2 = v2 ? lf[h0 + 2] : 0.f, b3 = v3 ? lf[h0 + 3] : 0.f;
      for (int c = 1; c < C; ++c) {
        const float* __restrict__ lc = lf + (size_t)c * V + h0;
        const float x0 = lc[0];
        if (x0 > b0) { b0 = x0; p0 = c; }
        if (v1) { const float x = lc[1]; if (x > b1) { b1 = x; p1 = c; } }
        if (v2) { const float x = lc[2]; if (x > b2) { b2 = x; p2 = c; } }
        if (v3) { const float x = lc[3]; if (x > b3) { b3 = x; p3 = c; } }
      }
    }
    if (h0 < V) *(uint32_t*)(cls + f * Vp + h0) = p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
    n += __popcll(__ballot(p0 != 0)) + __popcll(__ballot(p1 != 0)) + __popcll(__ballot(p2 != 0)) + __popcll(__ballot(p3 != 0));
  }
  exp_chunk_count(n, cnt, nblk, wsum);
}

// pass 1, integral grid (labels): only the counts; pass 2 reads the grid itself (frame stride V)
__global__ void __launch_bounds__(256)
export_count_kernel(const uint8_t* __restrict__ grid, long V, int nblk, int32_t* __restrict__ cnt) {
  __shared__ int wsum[4];
  const uint8_t* __restrict__ gf = grid + (size_t)blockIdx.y * V;
  int n = 0;
#pragma unroll
  for (int k = 0; k < EXP_CHUNK / 256; ++k) {
    const long h = (long)blockIdx.x * EXP_CHUNK + k * 256 + threadIdx.x;
    const bool occ = h < V && gf[h] != 0;
    n += __popcll(__ballot(occ));
  }
  exp_chunk_count(n, cnt, nblk, wsum);
}

// scan: one workgroup per frame: chunk counts -> exclusive offsets within the frame (in place), total -> counts[f]
__global__ void __launch_bounds__(256)
export_scan_kernel(int nblk, int32_t* __restrict__ cnt, int64_t* __restrict__ counts) {
  __shared__ int part[256];
  int32_t* c = cnt + (long)blockIdx.x * nblk;
  const int per = (nblk + 255) / 256, lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
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

// n / d for n < 2^31 with m = min(floor(2^32 / d), 2^32 - 1) from the host: the estimate umulhi(n, m) is floor(n / d) or one less
// (n * m / 2^32 > n / d - 1 / 2), one correction makes it exact.  r: the remainder.
__device__ __forceinline__ unsigned exp_div(unsigned n, unsigned d, unsigned m, unsigned& r) {
  unsigned q = __umulhi(n, m);
  r = n - q * d;
  if (r >= d) { ++q; r -= d; }
  return q;
}

// pass 2: ordered compaction.  The voxels of a chunk with a class != 0, in ascending h = (x * Y + y) * Z + z, to
// rows[base(f) + off[f][chunk] ...] as x, y, z, class (one 8-byte store per row); base(f) = counts[0] + ... + counts[f - 1],
// summed by every wave for itself (F <= 65535 values, usually a handful: no LDS round, no barrier).  Every load is issued before
// the one barrier.  Nothing is written at or beyond row `cap`.
__global__ void __launch_bounds__(256)
export_rows_kernel(const uint8_t* __restrict__ cls, long stride, long V, unsigned Y, unsigned Z, unsigned my, unsigned mz, int nblk,
                   const int32_t* __restrict__ off, const int64_t* __restrict__ counts, uint16_t* __restrict__ rows, long cap) {
  __shared__ int wcnt[EXP_CHUNK / 64];
  const long f = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* __restrict__ cf = cls + (size_t)f * stride;
  const int off0 = off[f * nblk + blockIdx.x];
  long long s = 0;
  for (long i = lane; i < f; i += 64) s += counts[i];
  unsigned t[EXP_CHUNK / 256];
  unsigned long long m[EXP_CHUNK / 256];
#pragma unroll
  for (int k = 0; k < EXP_CHUNK / 256; ++k) {
    const long h = (long)blockIdx.x * EXP_CHUNK + k * 256 + threadIdx.x;
    t[k] = h < V ? cf[h] : 0u;
  }
#pragma unroll
  for (int k = 0; k < EXP_CHUNK / 256; ++k) {
    m[k] = __ballot(t[k] != 0u);
    if (lane == 0) wcnt[k * 4 + wave] = __popcll(m[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  __syncthreads();
  long long pos = s + off0;
#pragma unroll
  for (int k = 0; k < EXP_CHUNK / 256; ++k) {
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = wcnt[k * 4 + w];
      if (w < wave) before += c;
      all += c;
    }
    if (t[k] != 0u) {
      const long long r = pos + before + __popcll(m[k] & ((1ull << lane) - 1ull));
      if (r < cap) {
        const unsigned h = (unsigned)((long)blockIdx.x * EXP_CHUNK + k * 256 + threadIdx.x);     // V < 2^31
        unsigned x, y, z;
        const unsigned xy = exp_div(h, Z, mz, z);
        x = exp_div(xy, Y, my, y);
        const unsigned long long row = (unsigned long long)x | ((unsigned long long)y << 16) | ((unsigned long long)z << 32) |
                                       ((unsigned long long)t[k] << 48);
        *(unsigned long long*)(rows + r * 4) = row;      // little endian: x, y, z, class as four uint16
      }
    }
    pos += all;
  }
}

// y = saturate(trunc(x * 255)): NaN and everything <= 0 -> 0, everything >= 255 -> 255 (+inf included)
__device__ __forceinline__ unsigned exp_u8(float x) {
  const float t = x * 255.0f;
  return !(t > 0.f) ? 0u : (t >= 255.f ? 255u : (unsigned)t);
}

// n4 groups of four elements: one 16-byte load, one 4-byte store; the last n - 4 * n4 (< 4, or all of them when the pointers
// are not aligned for the wide form) one by one
__global__ void __launch_bounds__(256)
export_image_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, long n4, long n) {
  const long step = (long)gridDim.x * 256;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n4; i += step) {
    const f32x4 v = ((const f32x4*)x)[i];
    ((uint32_t*)y)[i] = exp_u8(v.x) | (exp_u8(v.y) << 8) | (exp_u8(v.z) << 16) | (exp_u8(v.w) << 24);
  }
  for (long i = n4 * 4 + blockIdx.x * 256L + threadIdx.x; i < n; i += step) y[i] = (uint8_t)exp_u8(x[i]);
}

#define ST ((hipStream_t)stream)

struct ExpDims {
  long V, Vp;
  int nblk;
};

static int exp_dims(const char* who, int F, int X, int Y, int Z, ExpDims& d) {
  MUVO_CHECK_ARG(F > 0 && F <= 65535 && X > 0 && Y > 0 && Z > 0, "%s: bad sizes (F %d in 1..65535, grid %d %d %d must be positive)", who, F,
                 X, Y, Z);
  MUVO_CHECK_ARG(X <= 65536 && Y <= 65536 && Z <= 65536, "%s: grid %d %d %d beyond 65536 per axis (uint16 rows)", who, X, Y, Z);
  MUVO_CHECK_ARG((int64_t)X * Y * Z < (1ll << 31), "%s: grid %d %d %d has 2^31 voxels or more", who, X, Y, Z);
  d.V = (long)X * Y * Z;
  d.Vp = (d.V + 15) / 16 * 16;
  d.nblk = (int)((d.V + EXP_CHUNK - 1) / EXP_CHUNK);
  return MUVO_OK;
}

static int exp_rows(const uint8_t* cls, long stride, int F, unsigned Y, unsigned Z, const ExpDims& d, int32_t* cnt, uint16_t* rows,
                    int64_t cap, int64_t* counts, bool scan, hipStream_t st) {
  if (scan) hipLaunchKernelGGL(export_scan_kernel, dim3((unsigned)F), dim3(256), 0, st, d.nblk, cnt, counts);
  if (rows && cap > 0) {
    const unsigned my = (unsigned)std::min<uint64_t>((1ull << 32) / Y, 0xffffffffull), mz = (unsigned)std::min<uint64_t>((1ull << 32) / Z, 0xffffffffull);
    hipLaunchKernelGGL(export_rows_kernel, dim3((unsigned)d.nblk, (unsigned)F), dim3(256), 0, st, cls, stride, d.V, Y, Z, my, mz, d.nblk, cnt,
                       counts, rows, (long)cap);
  }
  MUVO_CHECK_LAUNCH("voxel_rows");
  return MUVO_OK;
}

extern "C" {

int64_t muvo_voxel_rows_scratch_bytes(int F, int X, int Y, int Z) {
  if (F <= 0 || X <= 0 || Y <= 0 || Z <= 0 || (int64_t)X * Y * Z >= (1ll << 31)) return -1;
  const int64_t V = (int64_t)X * Y * Z, Vp = (V + 15) / 16 * 16, nblk = (V + EXP_CHUNK - 1) / EXP_CHUNK;
  return (int64_t)F * (Vp + 4 * nblk);
}

int muvo_voxel_rows_logits(const float* logits, int F, int C, int X, int Y, int Z, void* scratch, uint16_t* rows, int64_t cap,
                           int64_t* counts, void* stream) {
  MUVO_CHECK_ARG(logits && scratch && counts, "voxel_rows_logits: null pointer (logits, scratch, counts)");
  MUVO_CHECK_ARG(C >= 2 && C <= EXP_MAXC, "voxel_rows_logits: C = %d outside 2..%d", C, EXP_MAXC);
  MUVO_CHECK_ARG(cap >= 0 && ((uintptr_t)rows & 7) == 0, "voxel_rows_logits: cap %lld < 0 or rows not 8-byte aligned", (long long)cap);
  ExpDims d;
  if (int rc = exp_dims("voxel_rows_logits", F, X, Y, Z, d)) return rc;
  uint8_t* cls = (uint8_t*)scratch;
  int32_t* cnt = (int32_t*)(cls + (size_t)F * d.Vp);
  const int vec = (d.V % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(export_classify_kernel, dim3((unsigned)d.nblk, (unsigned)F), dim3(256), 0, ST, logits, C, d.V, d.Vp, d.nblk, vec, cls, cnt);
  return exp_rows(cls, d.Vp, F, (unsigned)Y, (unsigned)Z, d, cnt, rows, cap, counts, true, ST);
}

int muvo_voxel_rows_grid(const uint8_t* grid, int F, int X, int Y, int Z, void* scratch, uint16_t* rows, int64_t cap, int64_t* counts,
                         void* stream) {
  MUVO_CHECK_ARG(grid && scratch && counts, "voxel_rows_grid: null pointer (grid, scratch, counts)");
  MUVO_CHECK_ARG(cap >= 0 && ((uintptr_t)rows & 7) == 0, "voxel_rows_grid: cap %lld < 0 or rows not 8-byte aligned", (long long)cap);
  ExpDims d;
  if (int rc = exp_dims("voxel_rows_grid", F, X, Y, Z, d)) return rc;
  int32_t* cnt = (int32_t*)((uint8_t*)scratch + (size_t)F * d.Vp);
  hipLaunchKernelGGL(export_count_kernel, dim3((unsigned)d.nblk, (unsigned)F), dim3(256), 0, ST, grid, d.V, d.nblk, cnt);
  return exp_rows(grid, d.V, F, (unsigned)Y, (unsigned)Z, d, cnt, rows, cap, counts, true, ST);
}

int muvo_voxel_rows_write(const uint8_t* grid, int F, int X, int Y, int Z, const void* scratch, const int64_t* counts, uint16_t* rows,
                          int64_t cap, void* stream) {
  MUVO_CHECK_ARG(scratch && counts && rows, "voxel_rows_write: null pointer (scratch, counts, rows)");
  MUVO_CHECK_ARG(cap >= 0 && ((uintptr_t)rows & 7) == 0, "voxel_rows_write: cap %lld < 0 or rows not 8-byte aligned", (long long)cap);
  ExpDims d;
  if (int rc = exp_dims("voxel_rows_write", F, X, Y, Z, d)) return rc;
  const uint8_t* cls = (const uint8_t*)scratch;
  int32_t* cnt = (int32_t*)(cls + (size_t)F * d.Vp);
  return exp_rows(grid ? grid : cls, grid ? d.V : d.Vp, F, (unsigned)Y, (unsigned)Z, d, cnt, rows, cap, const_cast<int64_t*>(counts), false, ST);
}

int muvo_image_u8(const float* x, uint8_t* y, int64_t n, void* stream) {
  MUVO_CHECK_ARG(x && y && n > 0, "image_u8: null pointer or n = %lld <= 0", (long long)n);
  const bool wide = ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 3) == 0;
  const long n4 = wide ? (long)(n / 4) : 0;
  hipLaunchKernelGGL(export_image_u8_kernel, dim3((unsigned)ew_grid(wide ? n4 + 3 : (long)n)), dim3(256), 0, ST, x, y, n4, (long)n);
  MUVO_CHECK_LAUNCH("image_u8");
  return MUVO_OK;
}

}  // extern "C"
