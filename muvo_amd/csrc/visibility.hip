// Sensor-visibility mask of the voxel labels (an extension, the reference has no such mask).
// include/muvo_hip.h (muvo_visibility_mark) is the definition; tests/visibility_reference.py restates it.
//   mark    one thread per (ray, frame): the walk of muvo_raycast - vg_start / vg_step of voxel_grid.h, occupancy from the 4 x 4 x 4
//           bricks as in raycast.hip - that marks every cell it visits up to and including the first occupied one.  `seen` has the
//           layout of the bricks: the bits of consecutive cells of one brick are collected in a register and leave as ONE 64-bit
//           OR atomic when the ray changes the brick and at its end - one atomic per up to ~10 steps - and not even that when
//           the word already holds the bits (vs_flush).
//   apply   4 consecutive voxels per lane: label != 0 stays, a free cell becomes 0 when SEEN and 255 otherwise; the two kinds of
//           free cells are counted (registers, LDS, then one 64-bit atomic per workgroup and counter).
// OR and integer sums are order-free: the same bits on every call, in both modes of muvo_set_deterministic.
// The march loop has the hard bound X + Y + Z + 3 whatever the input.
#include <algorithm>

#include "voxel_grid.h"

#define VS_THREADS 256
#define VS_VOX (VS_THREADS * 4)          // voxels per workgroup and round of the apply pass (4 consecutive per lane)
#define VS_APPLY_GROUPS 1024             // workgroups of the apply pass, all frames together: 4 per compute unit

// One OR for the bits a ray collected in brick `b`.  PROBE: read the word first and skip the atomic when it already holds the bits.
// Bits are only ever set during a call, so a stale read can only show too few of them and costs an atomic that was not needed;
// the result is the same.  All rays of a table leave one origin: without the probe every one of them sends its first atomic to the
// same word, and same-address atomics are served one after the other (8.8 ms -> 2.2 ms a call).
// PROBE = false (MUVO_VISIBILITY_PROBE=0) is kept for that measurement.
template <bool PROBE>
__device__ __forceinline__ void vs_flush(unsigned long long* __restrict__ sf, int b, uint64_t bits) {
  if (bits == 0) return;
  if (PROBE) {
    const unsigned long long have = __hip_atomic_load(sf + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((have & bits) == bits) return;
  }
  atomicOr(sf + b, (unsigned long long)bits);
}

// grid = (ray blocks, frames), one lane per ray; nb = the words of one frame
template <bool PROBE>
__global__ void __launch_bounds__(VS_THREADS)
vis_mark_kernel(const uint64_t* __restrict__ bricks, const float* __restrict__ rays, long R, int X, int Y, int Z, int BY, int BZ, long nb,
                unsigned long long* __restrict__ seen) {
  // workgroups are dispatched x first: with f = blockIdx.y the ~1000 workgroups that start together all march ONE frame out of
  // one origin cell and meet in one word.  Frames innermost spreads them over F words
  const long id = (long)blockIdx.y * gridDim.x + blockIdx.x;
  const int f = (int)(id % gridDim.y);
  const long r = (id / gridDim.y) * VS_THREADS + threadIdx.x;
  if (r >= R) return;
  VgRay s;
  int entry;
  if (!vg_start(s, rays + r * 7, X, Y, Z, entry)) return;
  const uint64_t* __restrict__ bf = bricks + (size_t)f * nb;
  unsigned long long* __restrict__ sf = seen + (size_t)f * nb;
  int held = 0;
  uint64_t word = 0, bits = 0;
  const int bound = X + Y + Z + 3;
  for (int it = 0; it < bound; ++it) {
    const int b = vg_brick_word(s.cx, s.cy, s.cz, BY, BZ);
    if (b != held || it == 0) {
      vs_flush<PROBE>(sf, held, bits);
      bits = 0;
      word = bf[b];
      held = b;
    }
    const uint64_t bit = 1ull << vg_brick_shift(s.cx, s.cy, s.cz);
    bits |= bit;
    if (word & bit) break;
    if (vg_step(s, X, Y, Z) < 0) break;
  }
  vs_flush<PROBE>(sf, held, bits);
}

// grid = (voxel blocks, frames); a workgroup strides over the chunks of its frame, so that the call ends with about two thousand
// atomics on the two counters and not one pair per 1024 voxels (same-address atomics are served one after the other: 0.56 ms
// of a 0.6 ms call at 20 frames of 192 x 192 x 64).  A workgroup sees fewer than 2^30 voxels: the 32-bit counters hold.
// vec: Z % 4 == 0 and aligned bases - the 4 cells share (x, y) and the 4-z group, one word serves them
__global__ void __launch_bounds__(VS_THREADS)
vis_apply_kernel(const uint8_t* __restrict__ label, const uint64_t* __restrict__ seen, int Y, int Z, int BY, int BZ, long nb, long V, int vec,
                 uint8_t* __restrict__ out, unsigned long long* __restrict__ counts) {
  __shared__ unsigned cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const long f = blockIdx.y;
  unsigned nfree = 0, nunknown = 0;
  for (long h0 = ((long)blockIdx.x * VS_THREADS + threadIdx.x) * 4; h0 < V; h0 += (long)gridDim.x * VS_VOX) {
    const uint64_t* __restrict__ sf = seen + (size_t)f * nb;
    unsigned l[4];
    vg_ld4(label + (size_t)f * V, h0, V, vec != 0, 1u, l);            // past the end: occupied, neither counted nor stored
    unsigned sn[4];
    if (vec) {
      const int z = (int)(h0 % Z), y = (int)((h0 / Z) % Y), x = (int)(h0 / ((long)Z * Y));
      const uint64_t w = sf[vg_brick_word(x, y, z, BY, BZ)] >> vg_brick_shift(x, y, 0);
      sn[0] = (unsigned)(w & 1ull); sn[1] = (unsigned)((w >> 1) & 1ull); sn[2] = (unsigned)((w >> 2) & 1ull); sn[3] = (unsigned)((w >> 3) & 1ull);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long h = h0 + k < V ? h0 + k : V - 1;
        const int z = (int)(h % Z), y = (int)((h / Z) % Y), x = (int)(h / ((long)Z * Y));
        sn[k] = (unsigned)((sf[vg_brick_word(x, y, z, BY, BZ)] >> vg_brick_shift(x, y, z)) & 1ull);
      }
    }
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool free_cell = l[k] == 0u;
      o[k] = free_cell ? (sn[k] ? 0u : 255u) : l[k];
      nfree += free_cell && sn[k] ? 1u : 0u;
      nunknown += free_cell && !sn[k] ? 1u : 0u;
    }
    vg_st4(out + (size_t)f * V, h0, V, vec != 0, uchar4{(unsigned char)o[0], (unsigned char)o[1], (unsigned char)o[2], (unsigned char)o[3]});
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nfree += __shfl_down(nfree, d, 64);
    nunknown += __shfl_down(nunknown, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nfree) atomicAdd(&cnt[0], nfree);
    if (nunknown) atomicAdd(&cnt[1], nunknown);
  }
  __syncthreads();
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

extern "C" {

int muvo_visibility_mark(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int64_t R, uint64_t* seen,
                         int64_t words, void* stream) {
  if (int rc = vg_check_frames("visibility_mark", F)) return rc;
  if (int rc = vg_check_grid("visibility_mark", X, Y, Z)) return rc;
  if (int rc = vg_check_rays("visibility_mark", R)) return rc;
  MUVO_CHECK_ARG(grid && bricks && rays && seen, "visibility_mark: null pointer");
  const int BX = (X + 3) / 4, BY = (Y + 3) / 4, BZ = (Z + 3) / 4;
  const int64_t nb = (int64_t)BX * BY * BZ;
  MUVO_CHECK_ARG(words >= F * nb && ((uintptr_t)seen & 7) == 0 && ((uintptr_t)bricks & 7) == 0, "visibility_mark: %lld seen words, %lld needed (8-byte aligned)",
                 (long long)words, (long long)(F * nb));
  if (hipMemsetAsync(seen, 0, (size_t)F * nb * 8, ST) != hipSuccess) {
    muvo_set_error("visibility_mark: clearing the seen words failed");
    return MUVO_ERR_HIP;
  }
  static const bool probe = env_int("MUVO_VISIBILITY_PROBE", 1) != 0;
  const dim3 grd((unsigned)((R + VS_THREADS - 1) / VS_THREADS), (unsigned)F);
  if (probe)
    hipLaunchKernelGGL(vis_mark_kernel<true>, grd, dim3(VS_THREADS), 0, ST, bricks, rays, (long)R, X, Y, Z, BY, BZ, (long)nb, (unsigned long long*)seen);
  else
    hipLaunchKernelGGL(vis_mark_kernel<false>, grd, dim3(VS_THREADS), 0, ST, bricks, rays, (long)R, X, Y, Z, BY, BZ, (long)nb, (unsigned long long*)seen);
  MUVO_CHECK_LAUNCH("visibility_mark");
  return MUVO_OK;
}

int muvo_visibility_apply(const uint8_t* label, const uint64_t* seen, int F, int X, int Y, int Z, uint8_t* out, uint64_t* counts, void* stream) {
  if (int rc = vg_check_frames("visibility_apply", F)) return rc;
  if (int rc = vg_check_grid("visibility_apply", X, Y, Z)) return rc;
  MUVO_CHECK_ARG(label && seen && out && counts, "visibility_apply: null pointer");
  MUVO_CHECK_ARG(((uintptr_t)seen & 7) == 0 && ((uintptr_t)counts & 7) == 0, "visibility_apply: seen or counts is not 8-byte aligned");
  const int BY = (Y + 3) / 4, BZ = (Z + 3) / 4;
  const int64_t nb = (int64_t)((X + 3) / 4) * BY * BZ, V = (int64_t)X * Y * Z;
  const int vec = (Z % 4 == 0 && ((uintptr_t)label & 3) == 0 && ((uintptr_t)out & 3) == 0) ? 1 : 0;
  const int64_t chunks = (V + VS_VOX - 1) / VS_VOX;
  const int64_t per_frame = std::min<int64_t>(chunks, std::max<int64_t>(1, VS_APPLY_GROUPS / F));
  hipLaunchKernelGGL(vis_apply_kernel, dim3((unsigned)per_frame, (unsigned)F), dim3(VS_THREADS), 0, ST, label, seen, Y, Z, BY, BZ, (long)nb, (long)V, vec, out,
                     (unsigned long long*)counts);
  MUVO_CHECK_LAUNCH("visibility_apply");
  return MUVO_OK;
}

}  // extern "C"
