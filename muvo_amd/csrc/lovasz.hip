// Lovasz-softmax training loss of the voxel head (an extension, the reference has no such loss):
//   per frame f and class c, over the voxels with label < C:  e_v = |[label_v == c] - softmax(logits_v)_c|, ranked descending
//   (ties: ascending voxel index), L_fc = sum_i e_(i) g_i with g the increment of the Jaccard loss along the ranking;
//   loss = weight / F * sum_f 1 / max(1, #present_f) * sum_{c present in f} L_fc.
// The hot path is a stable segmented LSD radix sort: one segment per (frame, class), 8-bit digits, 4 passes over 32-bit keys.
//   key  = 0x3F800000 - bits(e): ascending keys = descending errors (the bit pattern of a float in [0, 1] is monotone);
//          ignored voxels carry LV_SENTINEL, above every real key: they end up behind the ranking and take no part in it.
//   load = voxel index | foreground << 31 (V <= 2^30).
// Per pass: digit histogram per (segment, tile) -> exclusive scan per segment in (digit, tile) order -> scatter, where the rank
// of a key among the keys of its tile with the same digit comes from wave ballots (64 consecutive keys per wave round, a
// running count per wave and digit in LDS).  No atomics anywhere: every result is independent of the execution order.
// Behind the sort: foreground count per tile -> scan -> g from the closed forms in fp64, e * g summed per tile into a slot,
// g scattered back to voxel order; one workgroup adds the slots in a fixed order and applies the present-class rule.
#include "voxel_grid.h"

#define LV_THREADS 256
#define LV_ROUNDS 8
#define LV_WAVE_KEYS (64 * LV_ROUNDS)          // consecutive keys per wave
#define LV_TILE (LV_THREADS * LV_ROUNDS)       // keys per workgroup of the sort and of the passes behind it
#define LV_VOX (LV_THREADS * 4)                // voxels per workgroup of the key and gradient passes (4 consecutive per lane)
#define LV_ONE 0x3F800000u
#define LV_SENTINEL 0x3FFFFFFFu
#define LV_MAX_V (1l << 30)
#define LV_GROUP_KEYS (1l << 26)               // keys sorted per round of launches: bounds the ping-pong buffers to 1 GiB

// ---- key pass.  grid = (voxel blocks, frames of the group); f0 = the group's first frame.  keys / load: the group's buffers.
__global__ void __launch_bounds__(LV_THREADS)
lovasz_key_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int C, long V, int f0, int vec,
                  float* __restrict__ errors, uint32_t* __restrict__ keys, uint32_t* __restrict__ load) {
  const long f = f0 + blockIdx.y;
  const long h0 = ((long)blockIdx.x * LV_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  unsigned l[4];
  vg_ld4(labels + (size_t)f * V, h0, V, v4, 255u, l);          // 255: ignored
  const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
  const f32x4 m = st.m, s = st.sum;
  for (int c = 0; c < C; ++c) {
    const f32x4 p = vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), m, s);
    const float pk[4] = {p.x, p.y, p.z, p.w};
    float e[4];
    uint32_t k[4], w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = l[j] < (unsigned)C, fg = l[j] == (unsigned)c;
      e[j] = valid ? (fg ? 1.f - pk[j] : pk[j]) : 0.f;
      k[j] = valid ? LV_ONE - __float_as_uint(e[j]) : LV_SENTINEL;
      w[j] = (uint32_t)(h0 + j) | (fg ? 0x80000000u : 0u);
    }
    if (errors != nullptr) vg_st4(errors + ((size_t)f * C + c) * V, h0, V, v4, f32x4{e[0], e[1], e[2], e[3]});
    const size_t seg = (size_t)blockIdx.y * C + c;
    vg_st4(keys + seg * V, h0, V, v4, uint4{k[0], k[1], k[2], k[3]});
    vg_st4(load + seg * V, h0, V, v4, uint4{w[0], w[1], w[2], w[3]});
  }
}

// ---- the sort
// the lanes of the wave that are `valid` and hold the same 8-bit digit as this lane
__device__ __forceinline__ unsigned long long lv_match(unsigned d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long s = __ballot(bit);
    m &= bit ? s : ~s;
  }
  return m;
}

// hist[(seg * nblk + tile) * 256 + digit] = keys of the tile with that digit.  grid = (tiles, segments).
__global__ void __launch_bounds__(LV_THREADS)
lovasz_hist_kernel(const uint32_t* __restrict__ keys, long V, int nblk, int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t wc[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t seg = blockIdx.y;
  const uint32_t* __restrict__ ks = keys + seg * V;
#pragma unroll
  for (int w = 0; w < 4; ++w) wc[w][threadIdx.x] = 0u;
  const long i0 = (long)blockIdx.x * LV_TILE + wave * LV_WAVE_KEYS + lane;
  uint32_t k[LV_ROUNDS];
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) k[r] = i0 + r * 64 < V ? ks[i0 + r * 64] : 0u;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool valid = i0 + r * 64 < V;
    const unsigned d = (k[r] >> shift) & 255u;
    const unsigned long long m = lv_match(d, valid);
    if (valid && lane == __ffsll((long long)m) - 1) wc[wave][d] += (uint32_t)__popcll(m);     // one lane per digit: no conflict
  }
  __syncthreads();
  hist[(seg * nblk + blockIdx.x) * 256 + threadIdx.x] = (wc[0][threadIdx.x] + wc[1][threadIdx.x]) + (wc[2][threadIdx.x] + wc[3][threadIdx.x]);
}

// In place: hist -> the first output position of (digit, tile) within the segment, i.e. the exclusive scan in digit-major order.
// One workgroup of 1024 threads per segment: thread (q, d) owns digit d over the q-th quarter of the tiles.
__global__ void __launch_bounds__(1024) lovasz_offsets_kernel(uint32_t* __restrict__ hist, int nblk) {
  __shared__ uint32_t tot[4][256];
  __shared__ uint32_t sc[256];
  uint32_t* __restrict__ h = hist + (size_t)blockIdx.x * nblk * 256;
  const int q = threadIdx.x >> 8, d = threadIdx.x & 255;
  const int per = (nblk + 3) / 4, lo = min(q * per, nblk), hi = min(lo + per, nblk);
  uint32_t s = 0;
#pragma unroll 4
  for (int b = lo; b < hi; ++b) s += h[(size_t)b * 256 + d];
  tot[q][d] = s;
  __syncthreads();
  const uint32_t T = (tot[0][d] + tot[1][d]) + (tot[2][d] + tot[3][d]);
  if (q == 0) sc[d] = T;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {                     // inclusive scan of the 256 digit totals
    const uint32_t v = (q == 0 && d >= o) ? sc[d - o] : 0u;
    __syncthreads();
    if (q == 0) sc[d] += v;
    __syncthreads();
  }
  uint32_t run = sc[d] - T;
  for (int j = 0; j < q; ++j) run += tot[j][d];
#pragma unroll 4
  for (int b = lo; b < hi; ++b) {
    const uint32_t v = h[(size_t)b * 256 + d];
    h[(size_t)b * 256 + d] = run;
    run += v;
  }
}

// One stable pass: key i of the tile goes to offs[digit] + (keys of the tile before i with the same digit).
__global__ void __launch_bounds__(LV_THREADS)
lovasz_scatter_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ load, uint32_t* __restrict__ keys_out,
                      uint32_t* __restrict__ load_out, long V, int nblk, int shift, const uint32_t* __restrict__ offs) {
  __shared__ uint32_t wc[4][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t seg = blockIdx.y;
  const uint32_t* __restrict__ ks = keys + seg * V;
  const uint32_t* __restrict__ ws = load + seg * V;
#pragma unroll
  for (int w = 0; w < 4; ++w) wc[w][threadIdx.x] = 0u;
  const long i0 = (long)blockIdx.x * LV_TILE + wave * LV_WAVE_KEYS + lane;
  uint32_t k[LV_ROUNDS], w[LV_ROUNDS], rank[LV_ROUNDS];
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool valid = i0 + r * 64 < V;
    k[r] = valid ? ks[i0 + r * 64] : 0u;
    w[r] = valid ? ws[i0 + r * 64] : 0u;
  }
  const uint32_t first = offs[(seg * nblk + blockIdx.x) * 256 + threadIdx.x];
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool valid = i0 + r * 64 < V;
    const unsigned d = (k[r] >> shift) & 255u;
    const unsigned long long m = lv_match(d, valid);
    const uint32_t before = valid ? wc[wave][d] : 0u;                 // the wave's keys of earlier rounds with this digit
    rank[r] = before + (uint32_t)__popcll(m & below);
    __builtin_amdgcn_wave_barrier();
    if (valid && lane == __ffsll((long long)m) - 1) wc[wave][d] = before + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {                                                                   // thread = digit: counts per wave -> first position per wave
    const uint32_t c0 = wc[0][threadIdx.x], c1 = wc[1][threadIdx.x], c2 = wc[2][threadIdx.x];
    wc[0][threadIdx.x] = first;
    wc[1][threadIdx.x] = first + c0;
    wc[2][threadIdx.x] = first + c0 + c1;
    wc[3][threadIdx.x] = first + c0 + c1 + c2;
  }
  __syncthreads();
  uint32_t* __restrict__ ko = keys_out + seg * V;
  uint32_t* __restrict__ wo = load_out + seg * V;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool valid = i0 + r * 64 < V;
    const unsigned d = (k[r] >> shift) & 255u;
    const long pos = (long)wc[wave][d] + rank[r];
    if (valid && pos < V) {                                           // pos < V by construction; never write outside the segment
      ko[pos] = k[r];
      wo[pos] = w[r];
    }
  }
}

// ---- behind the sort: the Jaccard increments along the ranking
// cnt[seg * nblk + tile] = foreground voxels among the tile's sorted positions
__global__ void __launch_bounds__(LV_THREADS) lovasz_fgcount_kernel(const uint32_t* __restrict__ load, long V, int nblk, int32_t* __restrict__ cnt) {
  __shared__ int wsum[4];
  const uint32_t* __restrict__ ws = load + (size_t)blockIdx.y * V;
  int n = 0;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const long i = (long)blockIdx.x * LV_TILE + r * LV_THREADS + threadIdx.x;
    n += __popcll(__ballot(i < V && (ws[i] >> 31)));
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(size_t)blockIdx.y * nblk + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one workgroup per segment: tile counts -> exclusive offsets (in place), G[segment] = the total
__global__ void __launch_bounds__(256) lovasz_fgscan_kernel(int nblk, int32_t* __restrict__ cnt, int32_t* __restrict__ G) {
  __shared__ int part[256];
  int32_t* c = cnt + (size_t)blockIdx.x * nblk;
  const int per = (nblk + 255) / 256, lo = min((int)threadIdx.x * per, nblk), hi = min(lo + per, nblk);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += c[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
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
  if (threadIdx.x == 255) G[blockIdx.x] = part[255];
}

// Rank i (1-based) holds the voxel load[i - 1]; with n_fg = foreground among ranks <= i:  I = G - n_fg, U = G + (i - n_fg),
// g = 1 / U (foreground) or I / (U (U - 1)) (background), in fp64.  slot[seg * nblk + tile] = sum e g over the tile (fp64, a fixed
// tree); dlde[voxel] = (float)g, 0 for ignored voxels and for a class that is absent from the frame (G = 0).
__global__ void __launch_bounds__(LV_THREADS)
lovasz_grad_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ load, long V, int nblk, const int32_t* __restrict__ fgoff,
                   const int32_t* __restrict__ G, float* __restrict__ dlde, double* __restrict__ slot) {
  __shared__ int wcnt[LV_ROUNDS * 4];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t seg = blockIdx.y;
  const uint32_t* __restrict__ ks = keys + seg * V;
  const uint32_t* __restrict__ ws = load + seg * V;
  const long i0 = (long)blockIdx.x * LV_TILE + threadIdx.x;
  const int g_all = G[seg];
  uint32_t k[LV_ROUNDS], w[LV_ROUNDS];
  int incl[LV_ROUNDS];
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const bool in = i0 + r * LV_THREADS < V;
    k[r] = in ? ks[i0 + r * LV_THREADS] : LV_SENTINEL;
    w[r] = in ? ws[i0 + r * LV_THREADS] : 0u;
  }
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    const unsigned long long m = __ballot((w[r] >> 31) != 0u);
    incl[r] = __popcll(m & ((2ull << lane) - 1ull));
    if (lane == 0) wcnt[r * 4 + wave] = __popcll(m);
  }
  __syncthreads();
  int run = fgoff[seg * nblk + blockIdx.x];
  double sum = 0.0;
  float* __restrict__ ds = dlde != nullptr ? dlde + seg * V : nullptr;
#pragma unroll
  for (int r = 0; r < LV_ROUNDS; ++r) {
    int before = run;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = wcnt[r * 4 + j];
      before += j < wave ? c : 0;
      run += c;
    }
    const long i = i0 + r * LV_THREADS;
    const bool in = i < V, real = in && k[r] != LV_SENTINEL && g_all > 0;
    double g = 0.0;
    if (real) {
      const int nfg = before + incl[r];
      const double I = (double)(g_all - nfg), U = (double)g_all + (double)(i + 1 - nfg);
      g = (w[r] >> 31) ? 1.0 / U : I / (U * (U - 1.0));
      sum += (double)__uint_as_float(LV_ONE - k[r]) * g;
    }
    const long vox = (long)(w[r] & 0x7FFFFFFFu);
    if (ds != nullptr && in && vox < V) ds[vox] = (float)g;
  }
  sum = wave_sum_d(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) slot[seg * nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One workgroup.  lfc[f * C + c] = the slots of the segment added in a fixed order (one wave per segment: lane-strided partial
// sums, then the shuffle tree); present = G > 0; loss = weight / F * sum_f (sum_{c present} L_fc) / max(1, #present_f).
__global__ void __launch_bounds__(256)
lovasz_finish_kernel(const double* __restrict__ slot, const int32_t* __restrict__ G, int F, int C, int nblk, float weight,
                     double* __restrict__ lfc, uint8_t* __restrict__ present, float* __restrict__ loss) {
  __shared__ double red[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = F * C;
  for (int seg = wave; seg < S; seg += 4) {
    double s = 0.0;
    for (int b = lane; b < nblk; b += 64) s += slot[(size_t)seg * nblk + b];
    s = wave_sum_d(s);
    if (lane == 0) {
      lfc[seg] = s;
      present[seg] = G[seg] > 0 ? 1 : 0;
    }
  }
  __threadfence_block();
  __syncthreads();
  double t = 0.0;
  for (int f = threadIdx.x; f < F; f += 256) {
    double s = 0.0;
    int np = 0;
    for (int c = 0; c < C; ++c)
      if (G[f * C + c] > 0) {
        s += lfc[f * C + c];
        ++np;
      }
    t += s / (double)(np > 0 ? np : 1);
  }
  red[threadIdx.x] = t;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)((double)weight * red[0] / (double)F);
}

// ---- backward: dz_k = p_k (q_k - sum_c q_c p_c), q_c = scale_f * present_fc * (fg ? -1 : +1) * dlde_fc, zeros at ignored voxels
__global__ void __launch_bounds__(LV_THREADS)
lovasz_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, const float* __restrict__ dlde,
                  const uint8_t* __restrict__ present, float* __restrict__ dlogits, int C, long V, int vec, float weight,
                  const float* __restrict__ gout) {
  const long f = blockIdx.y;
  const long h0 = ((long)blockIdx.x * LV_THREADS + threadIdx.x) * 4;
  if (h0 >= V) return;
  const bool v4 = vec && h0 + 3 < V;
  unsigned pmask = 0u;
  for (int c = 0; c < C; ++c) pmask |= present[f * C + c] ? 1u << c : 0u;
  const int np = __popc(pmask);
  const float scale = (float)((double)weight * (double)gout[0] / ((double)gridDim.y * (double)(np > 0 ? np : 1)));
  const float* __restrict__ lf = logits + (size_t)f * C * V;
  const float* __restrict__ gf = dlde + (size_t)f * C * V;
  float* __restrict__ df = dlogits + (size_t)f * C * V;
  unsigned l[4];
  vg_ld4(labels + (size_t)f * V, h0, V, v4, 255u, l);          // 255: ignored
  const VgSoftmax st = vg_softmax_stats(lf, C, V, h0, v4);
  const f32x4 m = st.m, s = st.sum;
  f32x4 dot = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const f32x4 p = vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), m, s);
    const f32x4 g = vg_ld4(gf + (size_t)c * V, h0, V, v4);
    const float sc = (pmask >> c) & 1u ? scale : 0.f;
    dot.x += (l[0] == (unsigned)c ? -sc : sc) * g.x * p.x;
    dot.y += (l[1] == (unsigned)c ? -sc : sc) * g.y * p.y;
    dot.z += (l[2] == (unsigned)c ? -sc : sc) * g.z * p.z;
    dot.w += (l[3] == (unsigned)c ? -sc : sc) * g.w * p.w;
  }
  for (int c = 0; c < C; ++c) {
    const f32x4 p = vg_prob(vg_ld4(lf + (size_t)c * V, h0, V, v4), m, s);
    const f32x4 g = vg_ld4(gf + (size_t)c * V, h0, V, v4);
    const float sc = (pmask >> c) & 1u ? scale : 0.f;
    f32x4 d;
    d.x = l[0] < (unsigned)C ? p.x * ((l[0] == (unsigned)c ? -sc : sc) * g.x - dot.x) : 0.f;
    d.y = l[1] < (unsigned)C ? p.y * ((l[1] == (unsigned)c ? -sc : sc) * g.y - dot.y) : 0.f;
    d.z = l[2] < (unsigned)C ? p.z * ((l[2] == (unsigned)c ? -sc : sc) * g.z - dot.z) : 0.f;
    d.w = l[3] < (unsigned)C ? p.w * ((l[3] == (unsigned)c ? -sc : sc) * g.w - dot.w) : 0.f;
    vg_st4(df + (size_t)c * V, h0, V, v4, d);
  }
}

// ---- host side
#define ST ((hipStream_t)stream)
namespace {
inline int64_t lv_align(int64_t b) { return (b + 255) / 256 * 256; }
// frames sorted per round of launches, balanced over the rounds
inline int64_t lv_group_frames(int64_t F, int64_t C, int64_t V) {
  int64_t fpg = LV_GROUP_KEYS / (C * V);
  fpg = fpg < 1 ? 1 : (fpg > F ? F : fpg);
  const int64_t rounds = (F + fpg - 1) / fpg;
  return (F + rounds - 1) / rounds;
}
struct LvLayout {
  int64_t nblk, fpg, lfc, slot, G, keys[2], load[2], hist, fgcnt, total;
};
inline LvLayout lv_layout(int64_t F, int64_t C, int64_t V) {
  LvLayout L;
  L.nblk = (V + LV_TILE - 1) / LV_TILE;
  L.fpg = lv_group_frames(F, C, V);
  const int64_t S = F * C, Sg = L.fpg * C;
  int64_t o = 0;
  L.lfc = o; o += lv_align(S * 8);
  L.slot = o; o += lv_align(S * L.nblk * 8);
  L.G = o; o += lv_align(S * 4);
  for (int i = 0; i < 2; ++i) { L.keys[i] = o; o += lv_align(Sg * V * 4); }
  for (int i = 0; i < 2; ++i) { L.load[i] = o; o += lv_align(Sg * V * 4); }
  L.hist = o; o += lv_align(Sg * L.nblk * 256 * 4);
  L.fgcnt = o; o += lv_align(Sg * L.nblk * 4);
  L.total = o;
  return L;
}
inline bool lv_args_ok(int64_t F, int C, int64_t V) { return F > 0 && V > 0 && C >= 2 && C <= VG_MAXC && F * C <= 65535 && V <= LV_MAX_V; }
inline bool lv_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

extern "C" {

int64_t muvo_lovasz_ws_bytes(int64_t F, int C, int64_t V) {
  if (!lv_args_ok(F, C, V)) return 0;
  return lv_layout(F, C, V).total;
}

int muvo_lovasz_fwd(const float* logits, const uint8_t* labels, int64_t F, int C, int64_t V, float weight, void* ws, float* errors,
                    float* dlde, uint8_t* present, float* loss, void* stream) {
  MUVO_CHECK_ARG(logits && labels && ws && present && loss, "lovasz_fwd: null pointer");
  MUVO_CHECK_ARG(C >= 2 && C <= VG_MAXC, "lovasz_fwd: %d classes (2..16)", C);
  MUVO_CHECK_ARG(F > 0 && V > 0, "lovasz_fwd: bad args (F=%lld V=%lld)", (long long)F, (long long)V);
  MUVO_CHECK_ARG(F * C <= 65535, "lovasz_fwd: more than 65535 (frame, class) segments");
  MUVO_CHECK_ARG(V <= LV_MAX_V, "lovasz_fwd: more than 2^30 voxels per frame");
  MUVO_CHECK_ARG(lv_al16(ws), "lovasz_fwd: the scratch buffer must be 16-byte aligned");
  const LvLayout L = lv_layout(F, C, V);
  char* base = (char*)ws;
  double* lfc = (double*)(base + L.lfc);
  double* slot = (double*)(base + L.slot);
  int32_t* G = (int32_t*)(base + L.G);
  uint32_t* keys[2] = {(uint32_t*)(base + L.keys[0]), (uint32_t*)(base + L.keys[1])};
  uint32_t* load[2] = {(uint32_t*)(base + L.load[0]), (uint32_t*)(base + L.load[1])};
  uint32_t* hist = (uint32_t*)(base + L.hist);
  int32_t* fgcnt = (int32_t*)(base + L.fgcnt);
  const int nblk = (int)L.nblk;
  const int vec = V % 4 == 0 && lv_al16(logits) && ((uintptr_t)labels & 3u) == 0 && (errors == nullptr || lv_al16(errors));
  for (int64_t f0 = 0; f0 < F; f0 += L.fpg) {
    const int64_t nf = F - f0 < L.fpg ? F - f0 : L.fpg;
    const unsigned Sg = (unsigned)(nf * C);
    const size_t seg0 = (size_t)f0 * C;
    hipLaunchKernelGGL(lovasz_key_kernel, dim3((unsigned)((V + LV_VOX - 1) / LV_VOX), (unsigned)nf), dim3(LV_THREADS), 0, ST, logits, labels,
                       C, (long)V, (int)f0, vec, errors, keys[0], load[0]);
    for (int pass = 0; pass < 4; ++pass) {
      const int a = pass & 1, b = a ^ 1;
      hipLaunchKernelGGL(lovasz_hist_kernel, dim3(nblk, Sg), dim3(LV_THREADS), 0, ST, keys[a], (long)V, nblk, 8 * pass, hist);
      hipLaunchKernelGGL(lovasz_offsets_kernel, dim3(Sg), dim3(1024), 0, ST, hist, nblk);
      hipLaunchKernelGGL(lovasz_scatter_kernel, dim3(nblk, Sg), dim3(LV_THREADS), 0, ST, keys[a], load[a], keys[b], load[b], (long)V, nblk,
                         8 * pass, hist);
    }
    hipLaunchKernelGGL(lovasz_fgcount_kernel, dim3(nblk, Sg), dim3(LV_THREADS), 0, ST, load[0], (long)V, nblk, fgcnt);
    hipLaunchKernelGGL(lovasz_fgscan_kernel, dim3(Sg), dim3(256), 0, ST, nblk, fgcnt, G + seg0);
    hipLaunchKernelGGL(lovasz_grad_kernel, dim3(nblk, Sg), dim3(LV_THREADS), 0, ST, keys[0], load[0], (long)V, nblk, fgcnt, G + seg0,
                       dlde != nullptr ? dlde + seg0 * V : nullptr, slot + seg0 * nblk);
  }
  hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, ST, slot, G, (int)F, C, nblk, weight, lfc, present, loss);
  MUVO_CHECK_LAUNCH("lovasz_fwd");
  return MUVO_OK;
}

int muvo_lovasz_bwd(const float* logits, const uint8_t* labels, const float* dlde, const uint8_t* present, float* dlogits, int64_t F, int C,
                    int64_t V, float weight, const float* gout, void* stream) {
  MUVO_CHECK_ARG(logits && labels && dlde && present && dlogits && gout, "lovasz_bwd: null pointer");
  MUVO_CHECK_ARG(C >= 2 && C <= VG_MAXC, "lovasz_bwd: %d classes (2..16)", C);
  MUVO_CHECK_ARG(F > 0 && V > 0, "lovasz_bwd: bad args (F=%lld V=%lld)", (long long)F, (long long)V);
  MUVO_CHECK_ARG(F * C <= 65535, "lovasz_bwd: more than 65535 (frame, class) segments");
  MUVO_CHECK_ARG(V <= LV_MAX_V, "lovasz_bwd: more than 2^30 voxels per frame");
  const int vec = V % 4 == 0 && lv_al16(logits) && ((uintptr_t)labels & 3u) == 0 && lv_al16(dlde) && lv_al16(dlogits);
  hipLaunchKernelGGL(lovasz_bwd_kernel, dim3((unsigned)((V + LV_VOX - 1) / LV_VOX), (unsigned)F), dim3(LV_THREADS), 0, ST, logits, labels, dlde,
                     present, dlogits, C, (long)V, vec, weight, gout);
  MUVO_CHECK_LAUNCH("lovasz_bwd");
  return MUVO_OK;
}

}  // extern "C"
