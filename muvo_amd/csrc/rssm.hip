// The recurrent state-space model of MUVO (muvo/models/transition.py:76-173: RSSM.forward / observe_step / imagine_step,
// RepresentationModel :5-25) as TWO persistent kernels — one walks the T time steps forward, one walks them back.
//
// Per time step the reference runs ~25 tiny ops on a batch of b <= 4 sequences: Linear 512->1024, GRUCell(1024), two
// 2-layer MLPs (1088 and 1600 wide), sigma = 2 sigmoid(./2) + 0.1, z = mu + sigma eps, and feeds z / h to the next step.  With
// so few rows every layer is a matrix-VECTOR product: 53 MB of weights stream past per step, the arithmetic is nothing, and
// the old path's ~15 launches per step (x T x forward/backward = ~300 per training step) were pure launch + dependency
// latency.  Here one workgroup per CU stays resident for the whole sequence; a layer = every wave takes output rows, reads
// each weight row once with 16-byte loads and dots it with the (<= 4) input vectors held in LDS; layers are separated by a
// grid barrier (one atomic counter, agent-scope fences), 4 per time step.  Outputs are written straight into their
// (b, T, .) tensors (no stack / unstack / cat copies); the "which sample feeds the next step" choice (posterior, or prior
// with the reference's 15 % coin, transition.py:118-124) is a bit mask.  `nn.LeakyReLU(True)` in the reference has slope 1:
// there is NO nonlinearity between the Linear layers, reproduced as is.
//
// Backward: reverse time with the transposed weights (made once per call, 53 MB), same structure; the weight gradients are
// NOT formed per step — every per-step input / output gradient is kept (b*T rows) and the caller forms dW = dY^T X with one
// skinny GEMM per weight after the loop.
#include "common.h"
#include "rssm_cell.h"

#define ST ((hipStream_t)stream)
#define RSSM_THREADS 512
#define RSSM_WPB (RSSM_THREADS / 64)
#define RSSM_BM 4                 // batch rows held per wave accumulator set

// The order of every pointer table of the C ABI (include/muvo_hip.h) is stated here and nowhere else in this unit: the kernels
// and the host code name the entries, rssm_widths gives each (B, T, .) tensor's last-axis width under the same names.
enum { W_PRE, B_PRE, W_IH, W_HH, B_IH, B_HH, W_PA, B_PA, W_QA, B_QA, W_P0, B_P0, W_P2, B_P2, W_Q0, B_Q0, W_Q2, B_Q2, W_N };   // weights[18]
enum { O_H, O_MU_P, O_SG_P, O_Z_P, O_MU_Q, O_SG_Q, O_Z_Q, O_N };                       // out7, and upstream7: their gradients
enum { K_HPREV, K_ZPREV, K_APREV, K_U, K_GI, K_GH, K_XP, K_XQ, K_Y1P, K_Y1Q, K_MLS_P, K_MLS_Q, K_N };                       // keep12
enum { KP_HPREV, KP_GI, KP_GH, KP_MLS_P, KP_MLS_Q, KP_N };                             // kept5: what the backward reads of keep12
static const int KEPT5[KP_N] = {K_HPREV, K_GI, K_GH, K_MLS_P, K_MLS_Q};
enum { G_EMB, G_MLS_P, G_MLS_Q, G_Y1P, G_Y1Q, G_GI, G_GH, G_U, G_LA_P, G_LA_Q, G_N };  // grads10
enum { WT_PRE, WT_IH, WT_HH, WT_P0, WT_P2, WT_Q0, WT_Q2, WT_N };                       // the big matrices the backward reads transposed

struct RssmDims { int B, T, H, S, E, A, AD; };
struct RssmWidths { long out[O_N], keep[K_N], kept[KP_N], grad[G_N]; };
static RssmWidths rssm_widths(const RssmDims& d) {
  const long H = d.H, S = d.S, HP = d.H + d.A, HQ = d.H + d.E + d.A;
  RssmWidths w;
  w.out[O_H] = H;
  for (int i = O_MU_P; i < O_N; ++i) w.out[i] = S;
  w.keep[K_HPREV] = w.keep[K_U] = H; w.keep[K_ZPREV] = S; w.keep[K_APREV] = d.AD; w.keep[K_GI] = w.keep[K_GH] = 3 * H;
  w.keep[K_XP] = w.keep[K_Y1P] = HP; w.keep[K_XQ] = w.keep[K_Y1Q] = HQ; w.keep[K_MLS_P] = w.keep[K_MLS_Q] = 2 * S;
  for (int i = 0; i < KP_N; ++i) w.kept[i] = w.keep[KEPT5[i]];
  w.grad[G_EMB] = d.E; w.grad[G_MLS_P] = w.grad[G_MLS_Q] = 2 * S; w.grad[G_Y1P] = HP; w.grad[G_Y1Q] = HQ;
  w.grad[G_GI] = w.grad[G_GH] = 3 * H; w.grad[G_U] = H; w.grad[G_LA_P] = w.grad[G_LA_Q] = d.A;
  return w;
}
// The kernels index these arrays with constants only (a by-value argument array indexed at run time goes to scratch).
struct RssmFwdArgs {
  RssmDims d;
  const float* w[W_N];                          // PyTorch layouts [out][in]
  const float *emb, *act, *noise;               // (B,T,E) (B,T,AD) (B,T,2,S)
  unsigned long long use_prior;                 // bit t: step t+1 continues from the PRIOR sample of step t
  float* out[O_N];                              // outputs (B,T,.)
  float* keep[K_N];                             // kept for backward (B,T,.)
  unsigned* bar;
  float min_std;
};
struct RssmBwdArgs {
  RssmDims d;
  const float* wt[WT_N];                        // the TRANSPOSES [in][out]
  const float* noise;
  const float* kept[KP_N];
  unsigned long long use_prior;
  const float* up[O_N];                         // upstream (B,T,.), may be NULL
  float* grad[G_N];                             // per-step gradients kept (B,T,.)
  float *dxp, *dxq, *dh_carry, *dz_carry;       // scratch: (B,HP) (B,HQ) 2 x (B,H) (B,S)
  unsigned* bar;
};

// Dynamic LDS of a launch, in floats: the kernels carve their buffers from these offsets, the host sizes the launch and answers
// muvo_rssm_supported from the totals (tests/rssm_reference.py restates them: fwd_lds, bwd_lds).  A launch holds one slab of at
// most RSSM_BM of the d.B sequences.
struct RssmFwdLds { long xa, xb, hs, as, total; };
__host__ __device__ inline RssmFwdLds rssm_fwd_lds(const RssmDims& d) {
  const long B = d.B < RSSM_BM ? d.B : RSSM_BM, H = d.H, S = d.S, HP = H + d.A, HQ = H + d.E + d.A;
  RssmFwdLds l;
  l.xa = 0;                                     // stage inputs: [B][<= max(HQ, S)] (stage 0 holds z_{t-1}: S floats per sequence)
  l.xb = l.xa + B * (HQ > S ? HQ : S);          //               [B][<= HP]
  l.hs = l.xb + B * HP;                         // h_{t-1}: [B][H], kept through stage 1
  l.as = l.hs + B * H;                          // a_{t-1}: [B][AD]
  l.total = l.as + B * d.AD + 16;
  return l;
}
struct RssmBwdLds { long xa, xb, dd, total; };
__host__ __device__ inline RssmBwdLds rssm_bwd_lds(const RssmDims& d) {
  const long B = d.B < RSSM_BM ? d.B : RSSM_BM, H = d.H, S = d.S, HP = H + d.A, HQ = H + d.E + d.A;
  const long M3 = 3 * H > 2 * S ? 3 * H : 2 * S;             // B2 holds dgi / dgh (3H), B0 holds dmls (2S) in both buffers
  RssmBwdLds l;
  l.xa = 0;                                     // [B][<= max(HQ, 3H, 2S)]
  l.xb = l.xa + B * (HQ > M3 ? HQ : M3);        // [B][<= max(HP, 3H, 2S)]
  l.dd = l.xb + B * (HP > M3 ? HP : M3);        // direct dh_{t-1} path: [B][H]
  l.total = l.dd + B * H + 16;
  return l;
}

// Data that one workgroup writes and another reads across a grid barrier moves through agent-scope relaxed atomics (32-bit
// loads / stores that are coherent across the 8 XCDs by themselves), so the barrier needs NO L2 write-back / invalidate:
// a device-scope fence per wave cost ~90 us per barrier here (512 buffer_wbl2 + buffer_inv per XCD), 3.9 ms per sequence.
__device__ __forceinline__ void coh_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float coh_load(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// all workgroups are resident (grid <= occupancy x CUs, checked on the host before the launch): counter barrier.  Every wave
// first waits until its own (write-through) stores are acknowledged, the workgroup barrier collects the waves, one thread signs
// in and spins.  The spin is BOUNDED: if the grid is not co-resident after all (another persistent kernel holding CUs, a CU
// mask) the spinning thread gives up after RSSM_BARRIER_TIMEOUT_TICKS of the 100-MHz constant clock, raises the sticky error
// word bar[1] and every workgroup leaves the kernel (late workgroups see the word at their first barrier): the step ends with
// an error the host reads (ops.rssm_check) instead of a hung GPU.  Returns false when the kernel has to exit.
#define RSSM_BARRIER_TIMEOUT_TICKS 200000000ull /* 2 s */
__device__ __forceinline__ bool grid_barrier(unsigned* bar, unsigned target) {
  __shared__ unsigned s_ok;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned ok = 1u, spins = 0u;
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 255u) == 0u &&
          (__hip_atomic_load(bar + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u ||
           __builtin_amdgcn_s_memrealtime() - t0 > RSSM_BARRIER_TIMEOUT_TICKS)) {
        __hip_atomic_store(bar + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0u;
        break;
      }
    }
    s_ok = ok;
  }
  __syncthreads();
  return s_ok != 0u;
}
#define GRID_BARRIER(bar, target) \
  do {                            \
    if (!grid_barrier(bar, target)) return; \
  } while (0)

// NR weight rows (each K floats, 16-byte aligned, K % 4 == 0) dotted with the B input vectors xs[r*ldx + k] in LDS
template <int NR>
__device__ __forceinline__ void wave_dots(const float* const (&w)[NR], const float* __restrict__ xs, int ldx, int K, int B,
                                          float (&acc)[NR][RSSM_BM]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int r = 0; r < RSSM_BM; ++r) acc[q][r] = 0.f;
  for (int k0 = 4 * lane; k0 < K; k0 += 1024) {
    f32x4 wv[4][NR];
#pragma unroll
    for (int u = 0; u < 4; ++u)                 // up to 4 x NR independent 16-byte loads in flight per lane
#pragma unroll
      for (int q = 0; q < NR; ++q) {
        wv[u][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (k0 + 256 * u < K) wv[u][q] = __builtin_nontemporal_load((const f32x4*)(w[q] + k0 + 256 * u));
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + 256 * u < K) {
#pragma unroll
        for (int r = 0; r < RSSM_BM; ++r)
          if (r < B) {
            const f32x4 xv = *(const f32x4*)(xs + r * ldx + k0 + 256 * u);
#pragma unroll
            for (int q = 0; q < NR; ++q)
              acc[q][r] += (wv[u][q][0] * xv[0] + wv[u][q][1] * xv[1]) + (wv[u][q][2] * xv[2] + wv[u][q][3] * xv[3]);
          }
      }
  }
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int r = 0; r < RSSM_BM; ++r)
      if (r < B) acc[q][r] = wave_sum(acc[q][r]);
}

// acc[lane] without dynamic register indexing (lane < RSSM_BM)
__device__ __forceinline__ float pick(const float (&a)[RSSM_BM], int lane) {
  float v = a[0];
#pragma unroll
  for (int r = 1; r < RSSM_BM; ++r) v = lane == r ? a[r] : v;
  return v;
}

__device__ __forceinline__ void lds_load(float* dst, const float* __restrict__ src, int B, int n, long src_ld) {
  for (int i = threadIdx.x; i < B * n; i += RSSM_THREADS) {
    const int b = i / n, j = i - b * n;
    dst[i] = src ? coh_load(src + (long)b * src_ld + j) : 0.f;
  }
}

// What one output row of a layer needs.  The NR weight rows of K floats are dotted with the input vectors xs[r * K + k] in LDS
// (xs == nullptr: no dot product, the epilogue does the row's whole work); `part` says which of the stage's concatenated row
// ranges the row lies in (prior 0 | posterior 1 where a stage has the two branches) and j is its index inside that range.
template <int NR> struct LayerRow { const float* w[NR]; const float* xs; int K, part, j; };
// row o of a stage of n prior rows followed by the posterior rows: the weight rows j, n + j, ... of the branch's matrix
template <int NR>
__device__ __forceinline__ LayerRow<NR> pq_row(int o, int n, const float* wp, const float* wq, int Kp, int Kq, const float* xp,
                                               const float* xq) {
  LayerRow<NR> r;
  r.part = o >= n; r.j = r.part ? o - n : o; r.K = r.part ? Kq : Kp; r.xs = r.part ? xq : xp;
#pragma unroll
  for (int q = 0; q < NR; ++q) r.w[q] = (r.part ? wq : wp) + (long)(q * n + r.j) * r.K;
  return r;
}
// One layer.  The `rows` output rows are dealt to the waves of the whole grid, row o to wave o % NW; a wave forms the NR dot
// products of its row for all B sequences, then lane b < B ends the row for sequence b: epi(row, v), v[q] the q-th dot product.
template <int NR, class Row, class Epi>
__device__ __forceinline__ void layer(int rows, int B, Row row, Epi epi) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * RSSM_WPB + (threadIdx.x >> 6), NW = gridDim.x * RSSM_WPB;
  for (int o = gw; o < rows; o += NW) {
    const LayerRow<NR> r = row(o);
    float acc[NR][RSSM_BM] = {};
    if (r.xs) wave_dots<NR>(r.w, r.xs, r.K, r.K, B, acc);
    if (lane < B) {
      float v[NR];
#pragma unroll
      for (int q = 0; q < NR; ++q) v[q] = pick(acc[q], lane);
      epi(r, v);
    }
  }
}

__global__ void __launch_bounds__(RSSM_THREADS) rssm_fwd_kernel(const RssmFwdArgs a) {
  extern __shared__ float lds[];
  const int B = a.d.B, T = a.d.T, H = a.d.H, S = a.d.S, E = a.d.E, A = a.d.A, AD = a.d.AD;
  const int HP = H + A, HQ = H + E + A;
  const int tid = threadIdx.x, lane = tid & 63;
  const long gtid = (long)blockIdx.x * RSSM_THREADS + tid, gthreads = (long)gridDim.x * RSSM_THREADS;
  const RssmFwdLds l = rssm_fwd_lds(a.d);
  float *xa = lds + l.xa, *xb = lds + l.xb, *hs = lds + l.hs, *as = lds + l.as;
  unsigned target = 0;
  for (int t = 0; t < T; ++t) {
    const long lrow = (long)lane * T + t;        // row of sequence `lane` (< B: the epilogues) in the (B T, .) tensors
    // ------------------------------------------------------------------ stage 0: u = W_pre z, gh = W_hh h, action latents
    const float* zsrc = t == 0 ? nullptr : (((a.use_prior >> (t - 1)) & 1ull) ? a.out[O_Z_P] : a.out[O_Z_Q]) + (long)(t - 1) * S;
    lds_load(xa, zsrc, B, S, (long)T * S);
    lds_load(hs, t == 0 ? nullptr : a.out[O_H] + (long)(t - 1) * H, B, H, (long)T * H);
    lds_load(as, t == 0 ? nullptr : a.act + (long)(t - 1) * AD, B, AD, (long)T * AD);
    __syncthreads();
    if (blockIdx.x == 0) {         // the step's inputs, kept for the weight gradients
      for (int i = tid; i < B * S; i += RSSM_THREADS) a.keep[K_ZPREV][((long)(i / S) * T + t) * S + i % S] = xa[i];
      for (int i = tid; i < B * H; i += RSSM_THREADS) a.keep[K_HPREV][((long)(i / H) * T + t) * H + i % H] = hs[i];
      for (int i = tid; i < B * AD; i += RSSM_THREADS) a.keep[K_APREV][((long)(i / AD) * T + t) * AD + i % AD] = as[i];
    }
    layer<1>(4 * H + 2 * A, B,
             [&](int o) -> LayerRow<1> {         // H rows of u | 3H of gh | A prior, A posterior action latents
               if (o < 4 * H) return pq_row<1>(o, H, a.w[W_PRE], a.w[W_HH], S, H, xa, hs);
               const int post = o - 4 * H >= A;
               return {{nullptr}, nullptr, 0, 2 + post, o - 4 * H - (post ? A : 0)};
             },
             [&](const LayerRow<1>& r, const float (&v)[1]) {
               const int post = r.part == 3, j = r.j;
               if (r.part == 0) coh_store(&a.keep[K_U][lrow * H + j], v[0] + a.w[B_PRE][j]);
               else if (r.part == 1) coh_store(&a.keep[K_GH][lrow * 3 * H + j], v[0] + a.w[B_HH][j]);
               else {                             // AD terms: the lane sums them serially, starting at the bias
                 const float* wj = (post ? a.w[W_QA] : a.w[W_PA]) + (long)j * AD;
                 float s = (post ? a.w[B_QA] : a.w[B_PA])[j];
                 for (int k = 0; k < AD; ++k) s += wj[k] * as[lane * AD + k];
                 if (post) coh_store(&a.keep[K_XQ][lrow * HQ + H + E + j], s);
                 else coh_store(&a.keep[K_XP][lrow * HP + H + j], s);
               }
             });
    for (long i = gtid; i < (long)B * E; i += gthreads) {      // the embedding slice of the posterior input
      const int b = (int)(i / E), e = (int)(i - (long)b * E);
      coh_store(&a.keep[K_XQ][((long)b * T + t) * HQ + H + e], a.emb[((long)b * T + t) * E + e]);
    }
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ stage 1: gi = W_ih u, GRU cell -> h_t
    lds_load(xa, a.keep[K_U] + (long)t * H, B, H, (long)T * H);
    __syncthreads();
    layer<3>(H, B, [&](int o) { return pq_row<3>(o, H, a.w[W_IH], a.w[W_IH], H, H, xa, xa); },
             [&](const LayerRow<3>& r, const float (&v)[3]) {
               const int j = r.j;
               const float* gh = a.keep[K_GH] + lrow * 3 * H;
               float* gi = a.keep[K_GI] + lrow * 3 * H;
               const float ir = v[0] + a.w[B_IH][j], iz = v[1] + a.w[B_IH][H + j], in_ = v[2] + a.w[B_IH][2 * H + j];
               gi[j] = ir; gi[H + j] = iz; gi[2 * H + j] = in_;
               const GruGates q = gru_gates(ir, iz, in_, coh_load(&gh[j]), coh_load(&gh[H + j]), coh_load(&gh[2 * H + j]));
               const float hn = gru_combine(q, hs[lane * H + j]);
               coh_store(&a.out[O_H][lrow * H + j], hn);
               coh_store(&a.keep[K_XP][lrow * HP + j], hn);
               coh_store(&a.keep[K_XQ][lrow * HQ + j], hn);
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ stage 2: first MLP layers (no activation: slope 1)
    lds_load(xa, a.keep[K_XQ] + (long)t * HQ, B, HQ, (long)T * HQ);
    lds_load(xb, a.keep[K_XP] + (long)t * HP, B, HP, (long)T * HP);
    __syncthreads();
    layer<1>(HP + HQ, B, [&](int o) { return pq_row<1>(o, HP, a.w[W_P0], a.w[W_Q0], HP, HQ, xb, xa); },
             [&](const LayerRow<1>& r, const float (&v)[1]) {
               float* y1 = r.part ? a.keep[K_Y1Q] : a.keep[K_Y1P];
               coh_store(&y1[lrow * r.K + r.j], v[0] + (r.part ? a.w[B_Q0] : a.w[B_P0])[r.j]);
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ stage 3: (mu | log sigma), sample
    lds_load(xa, a.keep[K_Y1Q] + (long)t * HQ, B, HQ, (long)T * HQ);
    lds_load(xb, a.keep[K_Y1P] + (long)t * HP, B, HP, (long)T * HP);
    __syncthreads();
    layer<2>(2 * S, B, [&](int o) { return pq_row<2>(o, S, a.w[W_P2], a.w[W_Q2], HP, HQ, xb, xa); },
             [&](const LayerRow<2>& r, const float (&v)[2]) {
               const int post = r.part, j = r.j;
               const float* bias = post ? a.w[B_Q2] : a.w[B_P2];
               const float m = v[0] + bias[j], ls = v[1] + bias[S + j];
               float* mls = post ? a.keep[K_MLS_Q] : a.keep[K_MLS_P];
               mls[lrow * 2 * S + j] = m;
               mls[lrow * 2 * S + S + j] = ls;
               const float sg = rssm_sigma(ls, a.min_std);
               (post ? a.out[O_MU_Q] : a.out[O_MU_P])[lrow * S + j] = m;
               (post ? a.out[O_SG_Q] : a.out[O_SG_P])[lrow * S + j] = sg;
               coh_store(&(post ? a.out[O_Z_Q] : a.out[O_Z_P])[lrow * S + j], rssm_sample(m, sg, a.noise[(lrow * 2 + post) * S + j]));
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
  }
}

__global__ void __launch_bounds__(RSSM_THREADS) rssm_bwd_kernel(const RssmBwdArgs a) {
  extern __shared__ float lds[];
  const int B = a.d.B, T = a.d.T, H = a.d.H, S = a.d.S, E = a.d.E, A = a.d.A;
  const int HP = H + A, HQ = H + E + A;
  const int tid = threadIdx.x, lane = tid & 63;
  const RssmBwdLds l = rssm_bwd_lds(a.d);
  float *xa = lds + l.xa, *xb = lds + l.xb, *dd = lds + l.dd;
  unsigned target = 0;
  for (int t = T - 1; t >= 0; --t) {
    const bool up = (a.use_prior >> t) & 1ull;       // the carry dz of step t+1 belongs to the prior (else posterior) sample
    const bool has_carry = t < T - 1;
    const long lrow = (long)lane * T + t;        // row of sequence `lane` (< B: the epilogues) in the (B T, .) tensors
    // ------------------------------------------------------------------ B0: d(mu | log sigma), then dy1 = W2^T dmls
    for (int i = tid; i < B * S * 2; i += RSSM_THREADS) {
      const int post = i >= B * S, ii = post ? i - B * S : i;
      const int b = ii / S, j = ii - b * S;
      const long bt = (long)b * T + t;
      const float* mls = post ? a.kept[KP_MLS_Q] : a.kept[KP_MLS_P];
      const float* gmu = post ? a.up[O_MU_Q] : a.up[O_MU_P];
      const float* gsg = post ? a.up[O_SG_Q] : a.up[O_SG_P];
      const float* gz = post ? a.up[O_Z_Q] : a.up[O_Z_P];
      float dz = gz ? gz[bt * S + j] : 0.f;
      if (has_carry && (up != (bool)post)) dz += coh_load(&a.dz_carry[b * S + j]);
      const SampleAdjoint d = rssm_sample_adjoint(mls[bt * 2 * S + S + j], a.noise[(bt * 2 + post) * S + j],
                                                  gmu ? gmu[bt * S + j] : 0.f, gsg ? gsg[bt * S + j] : 0.f, dz);
      float* x = post ? xa : xb;
      x[b * 2 * S + j] = d.dmu;
      x[b * 2 * S + S + j] = d.dls;
      if (blockIdx.x == 0) {
        float* o = post ? a.grad[G_MLS_Q] : a.grad[G_MLS_P];
        o[bt * 2 * S + j] = d.dmu;
        o[bt * 2 * S + S + j] = d.dls;
      }
    }
    __syncthreads();
    layer<1>(HP + HQ, B, [&](int o) { return pq_row<1>(o, HP, a.wt[WT_P2], a.wt[WT_Q2], 2 * S, 2 * S, xb, xa); },
             [&](const LayerRow<1>& r, const float (&v)[1]) {
               coh_store(&(r.part ? a.grad[G_Y1Q] : a.grad[G_Y1P])[lrow * (r.part ? HQ : HP) + r.j], v[0]);
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ B1: dx = W0^T dy1
    lds_load(xa, a.grad[G_Y1Q] + (long)t * HQ, B, HQ, (long)T * HQ);
    lds_load(xb, a.grad[G_Y1P] + (long)t * HP, B, HP, (long)T * HP);
    __syncthreads();
    layer<1>(HP + HQ, B, [&](int o) { return pq_row<1>(o, HP, a.wt[WT_P0], a.wt[WT_Q0], HP, HQ, xb, xa); },
             [&](const LayerRow<1>& r, const float (&v)[1]) {      // x = (h | action latent) resp. (h | embedding | action latent)
               const int j = r.j, la = r.part ? H + E : H;
               coh_store(&(r.part ? a.dxq : a.dxp)[lane * r.K + j], v[0]);
               if (j >= la) (r.part ? a.grad[G_LA_Q] : a.grad[G_LA_P])[lrow * A + (j - la)] = v[0];
               else if (j >= H) a.grad[G_EMB][lrow * E + (j - H)] = v[0];
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ B2: GRU cell backward, du = W_ih^T dgi, dh_{t-1}
    const float* carry_in = a.dh_carry + (long)(t & 1) * B * H;
    float* carry_out = a.dh_carry + (long)((t + 1) & 1) * B * H;
    for (int i = tid; i < B * H; i += RSSM_THREADS) {
      const int b = i / H, j = i - b * H;
      const long bt = (long)b * T + t, base = bt * 3 * H;
      const float *gi = a.kept[KP_GI] + base, *gh = a.kept[KP_GH] + base;
      float g = (a.up[O_H] ? a.up[O_H][bt * H + j] : 0.f) + coh_load(&a.dxp[b * HP + j]) + coh_load(&a.dxq[b * HQ + j]);
      if (has_carry) g += coh_load(&carry_in[i]);
      const float ghn = gh[2 * H + j];
      const GruAdjoint d = gru_adjoint(gru_gates(gi[j], gi[H + j], gi[2 * H + j], gh[j], gh[H + j], ghn), ghn,
                                       a.kept[KP_HPREV][bt * H + j], g);
      xa[b * 3 * H + j] = d.dpre_r; xa[b * 3 * H + H + j] = d.dpre_z; xa[b * 3 * H + 2 * H + j] = d.dpre_n;      // dgi
      xb[b * 3 * H + j] = d.dpre_r; xb[b * 3 * H + H + j] = d.dpre_z; xb[b * 3 * H + 2 * H + j] = d.dgh_n;       // dgh
      dd[i] = d.dh;
      if (blockIdx.x == 0) {
        float *dgi = a.grad[G_GI] + base, *dgh = a.grad[G_GH] + base;
        dgi[j] = d.dpre_r; dgi[H + j] = d.dpre_z; dgi[2 * H + j] = d.dpre_n;
        dgh[j] = d.dpre_r; dgh[H + j] = d.dpre_z; dgh[2 * H + j] = d.dgh_n;
      }
    }
    __syncthreads();
    layer<1>(2 * H, B, [&](int o) { return pq_row<1>(o, H, a.wt[WT_IH], a.wt[WT_HH], 3 * H, 3 * H, xa, xb); },      // du | dh_{t-1}
             [&](const LayerRow<1>& r, const float (&v)[1]) {
               if (r.part) coh_store(&carry_out[lane * H + r.j], v[0] + dd[lane * H + r.j]);
               else coh_store(&a.grad[G_U][lrow * H + r.j], v[0]);
             });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
    // ------------------------------------------------------------------ B3: dz_{t-1} = W_pre^T du
    lds_load(xa, a.grad[G_U] + (long)t * H, B, H, (long)T * H);
    __syncthreads();
    layer<1>(S, B, [&](int o) { return pq_row<1>(o, S, a.wt[WT_PRE], a.wt[WT_PRE], H, H, xa, xa); },
             [&](const LayerRow<1>& r, const float (&v)[1]) { coh_store(&a.dz_carry[lane * S + r.j], v[0]); });
    target += gridDim.x;
    GRID_BARRIER(a.bar, target);
  }
}

// out[c][r] = in[r][c] for up to 7 matrices in one launch (blockIdx.z = matrix)
struct TransItem { const float* in; float* out; int rows, cols; };
struct TransTable { TransItem m[7]; };
__global__ void __launch_bounds__(256) rssm_transpose_kernel(const TransTable tb) {
  __shared__ float tile[32][33];
  const TransItem it = tb.m[blockIdx.z];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int tiles_c = (it.cols + 31) / 32, tiles_r = (it.rows + 31) / 32;
  for (int tid = blockIdx.x; tid < tiles_c * tiles_r; tid += gridDim.x) {
    const int r0 = (tid / tiles_c) * 32, c0 = (tid % tiles_c) * 32;
    for (int k = ty; k < 32; k += 8)
      tile[k][tx] = (r0 + k < it.rows && c0 + tx < it.cols) ? it.in[(long)(r0 + k) * it.cols + c0 + tx] : 0.f;
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
      if (c0 + k < it.cols && r0 + tx < it.rows) it.out[(long)(c0 + k) * it.rows + r0 + tx] = tile[tx][k];
    __syncthreads();
  }
}

// The seven transposed matrices, in the order of RssmBwdArgs::wt and of their places in wt_scratch: {weight, rows, cols} of the
// original.  Returns their floats; with a table to fill, tb gets weights[.] as input and consecutive pieces of `out` as output.
static int64_t rssm_transposes(int H, int S, int E, int A, const float* const* weights, float* out, TransTable* tb) {
  const int HP = H + A, HQ = H + E + A;
  const int m[WT_N][3] = {{W_PRE, H, S}, {W_IH, 3 * H, H}, {W_HH, 3 * H, H}, {W_P0, HP, HP}, {W_P2, 2 * S, HP}, {W_Q0, HQ, HQ},
                          {W_Q2, 2 * S, HQ}};
  int64_t n = 0;
  for (int i = 0; i < WT_N; ++i) {
    if (tb) tb->m[i] = {weights[m[i][0]], out + n, m[i][1], m[i][2]};
    n += (int64_t)m[i][1] * m[i][2];
  }
  return n;
}
// The backward kernel's global scratch for a launch over B sequences: dxp (B,HP) | dxq (B,HQ) | dh_carry 2 x (B,H), the steps
// alternate between the halves | dz_carry (B,S).  Returns its floats; with arguments to fill, `a` gets the pieces of `base`.
static int64_t rssm_bwd_scratch(int64_t B, int H, int S, int E, int A, float* base, RssmBwdArgs* a) {
  const int64_t n[4] = {B * (H + A), B * (H + E + A), 2 * B * H, B * S};
  if (a) { a->dxp = base; a->dxq = a->dxp + n[0]; a->dh_carry = a->dxq + n[1]; a->dz_carry = a->dh_carry + n[2]; }
  return n[0] + n[1] + n[2] + n[3];
}

// Per-device launch state: CU count, and per kernel the number of co-resident workgroups the occupancy calculator grants
// for the dynamic-LDS size in use (the grid barrier needs the WHOLE grid resident; the grid is clamped to that number).
#define RSSM_MAX_DEV 16
#define RSSM_MAX_DYN_LDS (160 * 1024 - 256)   /* the kernels also hold a few bytes of static LDS */
struct RssmDev { int cus, attr_fwd, attr_bwd; };
static RssmDev g_rssm_dev[RSSM_MAX_DEV];
static RssmDev* rssm_dev() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= RSSM_MAX_DEV) return nullptr;
  RssmDev* d = &g_rssm_dev[dev];
  if (!d->cus) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return nullptr;
    d->cus = p.multiProcessorCount;
  }
  return d;
}
// workgroups to launch: MUVO_RSSM_GRID or one per CU, never more than fit the chip at once
static int rssm_grid(const void* kernel, size_t ldsb) {
  RssmDev* d = rssm_dev();
  if (!d) return 0;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, RSSM_THREADS, ldsb) != hipSuccess || per_cu < 1) return 0;
  static const int want = getenv("MUVO_RSSM_GRID") ? atoi(getenv("MUVO_RSSM_GRID")) : 0;
  int g = want > 0 ? want : d->cus;
  if (g > per_cu * d->cus) g = per_cu * d->cus;
  return g;
}
static bool rssm_dims_ok(const RssmDims& d) {
  return d.B >= 1 && d.B <= 64 && d.T >= 1 && d.T <= 64 && d.H % 4 == 0 && d.S % 4 == 0 && d.E % 4 == 0 && d.A % 4 == 0 &&
         d.AD >= 1 && d.H > 0 && d.S > 0 && d.E > 0 && d.A > 0;
}

// dst[i] = src[i] + rows * width[i]: a table of (B, T, .) tensors moved to a slab's first row (a NULL entry stays NULL)
template <int N, class P>
static void rssm_offset(P* (&dst)[N], P* const* src, const long (&width)[N], long rows) {
  for (int i = 0; i < N; ++i) dst[i] = src[i] ? src[i] + rows * width[i] : nullptr;
}

// The launch path of both kernels, entered after the argument checks: the LDS limit, the device, the dynamic-LDS attribute (raised
// once per device), the grid, the transposes (backward: tb), then one launch per slab of <= RSSM_BM sequences: slab(a, rows, Bc)
// points the arguments at the slab, which starts at row `rows` of the (B T, .) tensors, the barrier counter is zeroed, the
// kernel launched.  `a` arrives with everything that does not depend on the slab filled in.
template <class Args, class Slab>
static int rssm_launch(const char* name, void (*kernel)(Args), int RssmDev::*attr, size_t ldsb, const TransTable* tb, Args a,
                       uint32_t* barrier_word, Slab slab, void* stream) {
  MUVO_CHECK_ARG(ldsb <= RSSM_MAX_DYN_LDS, "%s: LDS", name);
  RssmDev* dv = rssm_dev();
  MUVO_CHECK_ARG(dv, "%s: cannot query the device", name);
  if (!(dv->*attr)) {        // (static LDS of the kernel: the barrier's 4-byte flag; static + dynamic <= 160 KB)
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RSSM_MAX_DYN_LDS) != hipSuccess) {
      (void)hipGetLastError();
      muvo_set_error("%s: cannot raise the dynamic LDS limit", name);
      return MUVO_ERR_HIP;
    }
    dv->*attr = 1;
  }
  const int G = rssm_grid((const void*)kernel, ldsb);
  MUVO_CHECK_ARG(G > 0, "%s: the occupancy calculator grants no resident workgroup (LDS %zu B)", name, ldsb);
  if (tb) {
    hipLaunchKernelGGL(rssm_transpose_kernel, dim3(512, 1, WT_N), dim3(256), 0, ST, *tb);
    MUVO_CHECK_LAUNCH(name);
  }
  const int B = a.d.B;
  a.bar = barrier_word;
  for (int b0 = 0; b0 < B; b0 += RSSM_BM) {
    a.d.B = B - b0 < RSSM_BM ? B - b0 : RSSM_BM;
    slab(a, (long)b0 * a.d.T, a.d.B);
    if (hipMemsetAsync(barrier_word, 0, 4, ST) != hipSuccess) { muvo_set_error("%s: memset failed", name); return MUVO_ERR_HIP; }
    hipLaunchKernelGGL(kernel, dim3(G), dim3(RSSM_THREADS), ldsb, ST, a);
    MUVO_CHECK_LAUNCH(name);
  }
  return MUVO_OK;
}

extern "C" {
/* pointer tables (see include/muvo_hip.h): weights[18], out7, keep12, kept5, upstream7, grads10.  Sequences are independent
   (transition.py:76-127 loops over t, never over b): more than RSSM_BM of them run as consecutive launches over slabs of
   <= RSSM_BM sequences of the same (B, T, .) tensors. */
int muvo_rssm_supported(int B, int T, int H, int S, int E, int A, int AD) {
  const RssmDims d = {B, T, H, S, E, A, AD};
  if (!rssm_dims_ok(d) || !rssm_dev()) return 0;
  return sizeof(float) * rssm_fwd_lds(d).total <= RSSM_MAX_DYN_LDS && sizeof(float) * rssm_bwd_lds(d).total <= RSSM_MAX_DYN_LDS ? 1 : 0;
}
int64_t muvo_rssm_transposed_floats(int H, int S, int E, int A) { return rssm_transposes(H, S, E, A, nullptr, nullptr, nullptr); }
int64_t muvo_rssm_scratch_floats(int B, int H, int S, int E, int A) { return rssm_bwd_scratch(B, H, S, E, A, nullptr, nullptr); }
int muvo_rssm_forward(int B, int T, int H, int S, int E, int A, int AD, const float* const* weights, const float* emb,
                      const float* act, const float* noise, uint64_t use_prior_mask, float* const* out7, float* const* keep12,
                      uint32_t* barrier_word, float min_std, void* stream) {
  RssmFwdArgs a;
  a.d = {B, T, H, S, E, A, AD};
  MUVO_CHECK_ARG(rssm_dims_ok(a.d), "rssm_forward: dims (B=%d <= 64, T=%d <= 64, sizes %% 4) outside the fused kernel's range", B, T);
  MUVO_CHECK_ARG(weights && emb && act && noise && out7 && keep12 && barrier_word, "rssm_forward: null pointer");
  for (int i = 0; i < W_N; ++i) { MUVO_CHECK_ARG(weights[i], "rssm_forward: weight %d is NULL", i); a.w[i] = weights[i]; }
  for (int i = 0; i < O_N; ++i) MUVO_CHECK_ARG(out7[i], "rssm_forward: output %d is NULL", i);
  for (int i = 0; i < K_N; ++i) MUVO_CHECK_ARG(keep12[i], "rssm_forward: workspace %d is NULL", i);
  a.use_prior = use_prior_mask; a.min_std = min_std;
  const RssmWidths wd = rssm_widths(a.d);
  return rssm_launch("rssm_forward", rssm_fwd_kernel, &RssmDev::attr_fwd, sizeof(float) * rssm_fwd_lds(a.d).total, nullptr, a, barrier_word,
                     [&](RssmFwdArgs& s, long rows, int) {
                       s.emb = emb + rows * E; s.act = act + rows * AD; s.noise = noise + rows * 2 * S;
                       rssm_offset(s.out, out7, wd.out, rows);
                       rssm_offset(s.keep, keep12, wd.keep, rows);
                     }, stream);
}
int muvo_rssm_backward(int B, int T, int H, int S, int E, int A, int AD, const float* const* weights, float* wt_scratch,
                       const float* noise, uint64_t use_prior_mask, const float* const* kept5, const float* const* upstream7,
                       float* const* grads10, float* scratch, uint32_t* barrier_word, void* stream) {
  RssmBwdArgs a;
  a.d = {B, T, H, S, E, A, AD};
  MUVO_CHECK_ARG(rssm_dims_ok(a.d), "rssm_backward: dims outside the fused kernel's range");
  MUVO_CHECK_ARG(weights && wt_scratch && noise && kept5 && upstream7 && grads10 && scratch && barrier_word, "rssm_backward: null pointer");
  TransTable tb;
  rssm_transposes(H, S, E, A, weights, wt_scratch, &tb);
  for (int i = 0; i < WT_N; ++i) { MUVO_CHECK_ARG(tb.m[i].in, "rssm_backward: a weight is NULL"); a.wt[i] = tb.m[i].out; }
  for (int i = 0; i < KP_N; ++i) MUVO_CHECK_ARG(kept5[i], "rssm_backward: kept tensor %d is NULL", i);
  for (int i = 0; i < G_N; ++i) MUVO_CHECK_ARG(grads10[i], "rssm_backward: gradient buffer %d is NULL", i);
  a.use_prior = use_prior_mask;
  const RssmWidths wd = rssm_widths(a.d);
  return rssm_launch("rssm_backward", rssm_bwd_kernel, &RssmDev::attr_bwd, sizeof(float) * rssm_bwd_lds(a.d).total, &tb, a, barrier_word,
                     [&](RssmBwdArgs& s, long rows, int Bc) {
                       s.noise = noise + rows * 2 * S;
                       rssm_offset(s.kept, kept5, wd.kept, rows);
                       rssm_offset(s.up, upstream7, wd.out, rows);
                       rssm_offset(s.grad, grads10, wd.grad, rows);
                       rssm_bwd_scratch(Bc, H, S, E, A, scratch, &s);
                     }, stream);
}
}
