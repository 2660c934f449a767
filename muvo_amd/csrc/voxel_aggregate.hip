// Voxel labels filled from the neighbouring frames of their sequence (an extension, the reference has none).
// include/muvo_hip.h (muvo_voxel_pose_chain, muvo_voxel_aggregate) is the definition; tests/voxel_aggregate_reference.py restates it.
//   chain      one workgroup of 64: a lane per (frame, direction) walks d = 1 .. window along the links of its sequence, keeps the
//              product in 12 fp64 registers, and writes every step conjugated into cell coordinates.  A few hundred matrices: the
//              launch is its cost.
//   aggregate  the dense pass of vis_apply_kernel (4 consecutive voxels per lane, vg_ld4 / vg_st4) that, for every cell it would
//              write 255 to, walks the usable slots of its frame: three fp64 rows, floor, two bit tests in the brick words of the
//              source frame (occupancy, SEEN) and one byte load when occupied.  The matrices and flags of a frame are the same
//              for the whole workgroup (blockIdx.y is the frame): they arrive through scalar loads and the fp64 products take
//              them as scalar operands.  No LDS but the three counters, no atomics but one per workgroup and counter.
// A pure gather: the bytes do not depend on scheduling or on muvo_set_deterministic.
#include <algorithm>

#include "voxel_grid.h"

#define VA_THREADS 256
#define VA_VOX (VA_THREADS * 4)          // voxels per workgroup and round (4 consecutive per lane)
#define VA_GROUPS 2048                   // workgroups of the aggregate pass, all frames together: 8 per compute unit
#define VA_MAXWINDOW 64

struct VaMap {
  double a[3], o[3];                     // g = a r + o: range-view coordinates -> grid coordinates of one scale
};

__device__ __forceinline__ bool va_finite(double v) { return v - v == 0.0; }

// ---- chain -----------------------------------------------------------------------------------------------------------------------
// grid = 1, block = 64.  m = L m with L a link (dir 0: towards the past) or its rigid inverse (dir 1: towards the future)
__global__ void __launch_bounds__(64)
va_chain_kernel(const double* __restrict__ T, const double* __restrict__ fitness, const long long* __restrict__ status, int B, int S, double min_fitness,
                int window, VaMap mp, double* __restrict__ mats, uint8_t* __restrict__ usable) {
  const long n = (long)B * S * 2;
  for (long idx = threadIdx.x; idx < n; idx += 64) {
    const long f = idx >> 1;
    const int dir = (int)(idx & 1);
    const int i = (int)(f / S), t = (int)(f % S);
    double m0 = 1.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, m5 = 1.0, m6 = 0.0, m7 = 0.0, m8 = 0.0, m9 = 0.0, m10 = 1.0, m11 = 0.0;
    bool ok = true;
    for (int d = 1; d <= window; ++d) {
      const int tp = dir ? t + d : t - d;
      ok = ok && tp >= 0 && tp < S;
      if (ok) {
        const long link = (long)i * (S - 1) + (dir ? t + d - 1 : t - d);
        const double* __restrict__ L = T + link * 16;
        double l0 = L[0], l1 = L[1], l2 = L[2], l3 = L[3], l4 = L[4], l5 = L[5], l6 = L[6], l7 = L[7], l8 = L[8], l9 = L[9], l10 = L[10], l11 = L[11];
        bool valid = va_finite(l0) && va_finite(l1) && va_finite(l2) && va_finite(l3) && va_finite(l4) && va_finite(l5) && va_finite(l6) &&
                     va_finite(l7) && va_finite(l8) && va_finite(l9) && va_finite(l10) && va_finite(l11);
        if (fitness) valid = valid && fitness[link] >= min_fitness;                       // NaN: invalid
        if (status) {
          const long long st = status[link];
          valid = valid && st != MUVO_ICP_FEW_INLIERS && st != MUVO_ICP_EMPTY && st != MUVO_ICP_BAD_FRAME;
        }
        ok = valid;
        if (ok) {
          if (dir) {                                                                      // [R^T, -R^T tau]
            const double i3 = -((l0 * l3 + l4 * l7) + l8 * l11), i7 = -((l1 * l3 + l5 * l7) + l9 * l11), i11 = -((l2 * l3 + l6 * l7) + l10 * l11);
            const double r1 = l4, r2 = l8, r4 = l1, r6 = l9, r8 = l2, r9 = l6;
            l1 = r1; l2 = r2; l4 = r4; l6 = r6; l8 = r8; l9 = r9;
            l3 = i3; l7 = i7; l11 = i11;
          }
          const double n0 = (l0 * m0 + l1 * m4) + l2 * m8, n1 = (l0 * m1 + l1 * m5) + l2 * m9, n2 = (l0 * m2 + l1 * m6) + l2 * m10,
                       n3 = ((l0 * m3 + l1 * m7) + l2 * m11) + l3;
          const double n4 = (l4 * m0 + l5 * m4) + l6 * m8, n5 = (l4 * m1 + l5 * m5) + l6 * m9, n6 = (l4 * m2 + l5 * m6) + l6 * m10,
                       n7 = ((l4 * m3 + l5 * m7) + l6 * m11) + l7;
          const double n8 = (l8 * m0 + l9 * m4) + l10 * m8, n9 = (l8 * m1 + l9 * m5) + l10 * m9, n10 = (l8 * m2 + l9 * m6) + l10 * m10,
                       n11 = ((l8 * m3 + l9 * m7) + l10 * m11) + l11;
          m0 = n0; m1 = n1; m2 = n2; m3 = n3; m4 = n4; m5 = n5; m6 = n6; m7 = n7; m8 = n8; m9 = n9; m10 = n10; m11 = n11;
        }
      }
      const long slot = f * (2 * window) + 2 * (d - 1) + dir;
      double* __restrict__ o = mats + slot * 12;
      usable[slot] = ok ? 1 : 0;
      if (ok) {                                                                           // into the cells of the scale
        const double c0 = (mp.a[0] * m0) / mp.a[0], c1 = (mp.a[0] * m1) / mp.a[1], c2 = (mp.a[0] * m2) / mp.a[2];
        const double c4 = (mp.a[1] * m4) / mp.a[0], c5 = (mp.a[1] * m5) / mp.a[1], c6 = (mp.a[1] * m6) / mp.a[2];
        const double c8 = (mp.a[2] * m8) / mp.a[0], c9 = (mp.a[2] * m9) / mp.a[1], c10 = (mp.a[2] * m10) / mp.a[2];
        o[0] = c0; o[1] = c1; o[2] = c2; o[3] = (mp.a[0] * m3 + mp.o[0]) - ((c0 * mp.o[0] + c1 * mp.o[1]) + c2 * mp.o[2]);
        o[4] = c4; o[5] = c5; o[6] = c6; o[7] = (mp.a[1] * m7 + mp.o[1]) - ((c4 * mp.o[0] + c5 * mp.o[1]) + c6 * mp.o[2]);
        o[8] = c8; o[9] = c9; o[10] = c10; o[11] = (mp.a[2] * m11 + mp.o[2]) - ((c8 * mp.o[0] + c9 * mp.o[1]) + c10 * mp.o[2]);
      } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = 0.0;
      }
    }
  }
}

// ---- aggregate -------------------------------------------------------------------------------------------------------------------
// The state of cell floor(M (c + 1/2)) of the source frame: -1 = UNK or outside, else the class (0 = free and seen)
__device__ __forceinline__ int va_lookup(const double* __restrict__ m, double cx, double cy, double cz, const uint8_t* __restrict__ gs,
                                         const uint64_t* __restrict__ bs, const uint64_t* __restrict__ ss, int X, int Y, int Z, int BY, int BZ) {
  const double q0 = ((m[0] * cx + m[1] * cy) + m[2] * cz) + m[3];
  const double q1 = ((m[4] * cx + m[5] * cy) + m[6] * cz) + m[7];
  const double q2 = ((m[8] * cx + m[9] * cy) + m[10] * cz) + m[11];
  // floor(q) in [0, N) <=> 0 <= q < N; a NaN fails both; inside, truncation is the floor
  if (!(q0 >= 0.0 && q0 < (double)X && q1 >= 0.0 && q1 < (double)Y && q2 >= 0.0 && q2 < (double)Z)) return -1;
  const int jx = (int)q0, jy = (int)q1, jz = (int)q2;
  const int b = vg_brick_word(jx, jy, jz, BY, BZ), sh = vg_brick_shift(jx, jy, jz);
  if ((bs[b] >> sh) & 1ull) return (int)gs[((long)jx * Y + jy) * Z + jz];
  return ((ss[b] >> sh) & 1ull) ? 0 : -1;
}

// grid = (voxel blocks, frames) as vis_apply_kernel: a workgroup strides over the chunks of its frame.  A workgroup sees fewer than
// 2^30 voxels: the 32-bit counters hold.  VEC: Z % 4 == 0 and aligned bases - the 4 cells share (x, y) and one word of SEEN
template <bool VEC>
__global__ void __launch_bounds__(VA_THREADS)
va_aggregate_kernel(const uint8_t* __restrict__ grid, const uint64_t* __restrict__ bricks, const uint64_t* __restrict__ seen, int S, int X, int Y, int Z,
                    int BY, int BZ, long nb, long V, int slots, const double* __restrict__ mats, const uint8_t* __restrict__ usable,
                    uint8_t* __restrict__ out, unsigned long long* __restrict__ counts) {
  __shared__ unsigned cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const long f = blockIdx.y, ts = f % S;
  const uint64_t* __restrict__ sf = seen + (size_t)f * nb;
  const double* __restrict__ mf = mats + (size_t)f * slots * 12;
  const uint8_t* __restrict__ uf = usable + (size_t)f * slots;
  unsigned nocc = 0, nfree = 0, nunknown = 0;
  for (long h0 = ((long)blockIdx.x * VA_THREADS + threadIdx.x) * 4; h0 < V; h0 += (long)gridDim.x * VA_VOX) {
    unsigned l[4];
    vg_ld4(grid + (size_t)f * V, h0, V, VEC, 1u, l);                  // past the end: occupied, neither counted nor stored
    int xs[4], ys[4], zs[4];
    unsigned sn[4];
    if (VEC) {
      const int z = (int)(h0 % Z), y = (int)((h0 / Z) % Y), x = (int)(h0 / ((long)Z * Y));
      const uint64_t w = sf[vg_brick_word(x, y, z, BY, BZ)] >> vg_brick_shift(x, y, 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        xs[k] = x; ys[k] = y; zs[k] = z + k;
        sn[k] = (unsigned)((w >> k) & 1ull);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long h = h0 + k < V ? h0 + k : V - 1;
        zs[k] = (int)(h % Z); ys[k] = (int)((h / Z) % Y); xs[k] = (int)(h / ((long)Z * Y));
        sn[k] = (unsigned)((sf[vg_brick_word(xs[k], ys[k], zs[k], BY, BZ)] >> vg_brick_shift(xs[k], ys[k], zs[k])) & 1ull);
      }
    }
    unsigned o[4];
    unsigned pending = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool free_cell = l[k] == 0u;
      o[k] = free_cell ? (sn[k] ? 0u : 255u) : l[k];
      pending |= free_cell && !sn[k] ? 1u << k : 0u;
    }
    if (pending) {
      for (int s = 0; s < slots; ++s) {
        if (!uf[s]) continue;                                         // the same for the whole workgroup
        const int d = (s >> 1) + 1;
        const long tp = (s & 1) ? ts + d : ts - d;
        if (tp < 0 || tp >= S) continue;                              // never with the flags of the chain: no read outside the sequence
        const long fs = f - ts + tp;
        const double* __restrict__ m = mf + (size_t)s * 12;
        const uint8_t* __restrict__ gs = grid + (size_t)fs * V;
        const uint64_t* __restrict__ bs = bricks + (size_t)fs * nb;
        const uint64_t* __restrict__ ss = seen + (size_t)fs * nb;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (pending & (1u << k)) {
            const int v = va_lookup(m, (double)xs[k] + 0.5, (double)ys[k] + 0.5, (double)zs[k] + 0.5, gs, bs, ss, X, Y, Z, BY, BZ);
            if (v >= 0) {
              o[k] = (unsigned)v;
              pending &= ~(1u << k);
              nocc += v != 0 ? 1u : 0u;
              nfree += v == 0 ? 1u : 0u;
            }
          }
        }
        if (!pending) break;
      }
      nunknown += __popc(pending);
    }
    vg_st4(out + (size_t)f * V, h0, V, VEC, uchar4{(unsigned char)o[0], (unsigned char)o[1], (unsigned char)o[2], (unsigned char)o[3]});
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    nocc += __shfl_down(nocc, d, 64);
    nfree += __shfl_down(nfree, d, 64);
    nunknown += __shfl_down(nunknown, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (nocc) atomicAdd(&cnt[0], nocc);
    if (nfree) atomicAdd(&cnt[1], nfree);
    if (nunknown) atomicAdd(&cnt[2], nunknown);
  }
  __syncthreads();
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
#define ST ((hipStream_t)stream)

extern "C" {

int muvo_voxel_pose_chain(const double* T, const double* fitness, const int64_t* status, int B, int S, double min_fitness, int window,
                          const double* map, double* mats, uint8_t* usable, void* stream) {
  MUVO_CHECK_ARG(B >= 1 && S >= 1 && S <= 65535, "voxel_pose_chain: %d sequences of %d frames (1..65535 frames each)", B, S);
  if (int rc = vg_check_frames("voxel_pose_chain", (int64_t)B * S)) return rc;
  MUVO_CHECK_ARG(window >= 1 && window <= VA_MAXWINDOW, "voxel_pose_chain: window %d outside 1..%d", window, VA_MAXWINDOW);
  MUVO_CHECK_ARG((T || S == 1) && map && mats && usable, "voxel_pose_chain: null pointer");
  MUVO_CHECK_ARG((fitness == nullptr) == (status == nullptr), "voxel_pose_chain: fitness and status come together or not at all");
  MUVO_CHECK_ARG(min_fitness == min_fitness, "voxel_pose_chain: min_fitness is NaN");
  MUVO_CHECK_ARG(((uintptr_t)T & 7) == 0 && ((uintptr_t)fitness & 7) == 0 && ((uintptr_t)status & 7) == 0 && ((uintptr_t)mats & 7) == 0,
                 "voxel_pose_chain: a pointer is not 8-byte aligned");
  VaMap mp;
  for (int a = 0; a < 3; ++a) {
    mp.a[a] = map[a];
    mp.o[a] = map[3 + a];
    MUVO_CHECK_ARG(mp.a[a] != 0.0 && mp.a[a] - mp.a[a] == 0.0 && mp.o[a] - mp.o[a] == 0.0, "voxel_pose_chain: map entry %d is zero or not finite", a);
  }
  hipLaunchKernelGGL(va_chain_kernel, dim3(1), dim3(64), 0, ST, T, fitness, (const long long*)status, B, S, min_fitness, window, mp, mats, usable);
  MUVO_CHECK_LAUNCH("voxel_pose_chain");
  return MUVO_OK;
}

int muvo_voxel_aggregate(const uint8_t* grid, const uint64_t* bricks, const uint64_t* seen, int F, int S, int X, int Y, int Z, int window,
                         const double* mats, const uint8_t* usable, uint8_t* out, int64_t* counts, void* stream) {
  if (int rc = vg_check_frames("voxel_aggregate", F)) return rc;
  if (int rc = vg_check_grid("voxel_aggregate", X, Y, Z)) return rc;
  MUVO_CHECK_ARG(S >= 1 && F % S == 0, "voxel_aggregate: %d frames are not sequences of %d", F, S);
  MUVO_CHECK_ARG(window >= 1 && window <= VA_MAXWINDOW, "voxel_aggregate: window %d outside 1..%d", window, VA_MAXWINDOW);
  MUVO_CHECK_ARG(grid && bricks && seen && mats && usable && out && counts, "voxel_aggregate: null pointer");
  MUVO_CHECK_ARG(out != grid, "voxel_aggregate: out aliases grid");
  MUVO_CHECK_ARG(((uintptr_t)bricks & 7) == 0 && ((uintptr_t)seen & 7) == 0 && ((uintptr_t)mats & 7) == 0 && ((uintptr_t)counts & 7) == 0,
                 "voxel_aggregate: bricks, seen, mats or counts is not 8-byte aligned");
  const int BY = (Y + 3) / 4, BZ = (Z + 3) / 4;
  const int64_t nb = (int64_t)((X + 3) / 4) * BY * BZ, V = (int64_t)X * Y * Z;
  const bool vec = Z % 4 == 0 && ((uintptr_t)grid & 3) == 0 && ((uintptr_t)out & 3) == 0;
  const int64_t chunks = (V + VA_VOX - 1) / VA_VOX;
  const int64_t per_frame = std::min<int64_t>(chunks, std::max<int64_t>(1, VA_GROUPS / F));
  const dim3 grd((unsigned)per_frame, (unsigned)F);
  if (vec)
    hipLaunchKernelGGL(va_aggregate_kernel<true>, grd, dim3(VA_THREADS), 0, ST, grid, bricks, seen, S, X, Y, Z, BY, BZ, (long)nb, (long)V, 2 * window, mats,
                       usable, out, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(va_aggregate_kernel<false>, grd, dim3(VA_THREADS), 0, ST, grid, bricks, seen, S, X, Y, Z, BY, BZ, (long)nb, (long)V, 2 * window, mats,
                       usable, out, (unsigned long long*)counts);
  MUVO_CHECK_LAUNCH("voxel_aggregate");
  return MUVO_OK;
}

}  // extern "C"
