// Fused multi-head self-attention of the sensor-fusion transformer (muvo/models/mile.py:96-101,558:
// nn.TransformerEncoderLayer(384, 8) -> F.multi_head_attention_forward: softmax(q k^T / sqrt(dh)) -> dropout -> @ v), forward
// and backward, on the packed (L, N, 3E) projection.  L = 324 tokens, dh = 48: K and V of one (frame, head) are 2 x 62 KB,
// so the WHOLE key/value set of a head sits in LDS (one workgroup per CU) and nothing of size L x L ever goes to HBM:
//   * exact fp32 arithmetic on v_mfma_f32_16x16x4_f32 (dh = 48 = 3 x 16: no tile padding along dh);
//   * a wave owns 16 queries.  It computes S^T = K Q^T tile by tile (16 keys x 16 queries), so that a lane holds ONE query
//     column: the softmax reductions over the keys are register-local plus two wave shuffles (xor 16, 32);
//   * the accumulator layout of S^T (lane = query, 4 registers = keys 4g..4g+3) IS the A-operand layout of the next MFMA
//     (P V, P dO, dS K, dS Q), so the probabilities never pass through LDS or HBM;
//   * backward recomputes the probabilities from the saved row log-sum-exp (L floats per head instead of L x L) and
//     regenerates the dropout mask from (seed, index) — the same counter-based hash and index convention
//     ((n*H + h)*L + query)*L + key as the unfused softmax_dropout kernels;
//   * two backward kernels (dQ per query block; dK, dV per key block): no atomics, deterministic.
// LDS rows are DH + 4 floats: 16-byte fragment reads of 8 consecutive rows and 4-byte reads of 4 rows x 16 columns both
// spread over all 32 banks.
#include "common.h"

#define ST ((hipStream_t)stream)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)
#define ATTN_MAXT 24          // key tiles of 16 held in registers by the forward kernel: L <= 384
#define ATTN_WAVES 8

template <int DH>
__device__ __forceinline__ void attn_stage(float* __restrict__ dst, const float* __restrict__ src, long row_stride, int L,
                                           int Lp, int tid) {
  constexpr int C4 = DH / 4, RS = DH + 4;
  for (int idx = tid; idx < Lp * C4; idx += 64 * ATTN_WAVES) {
    const int row = idx / C4, c4 = idx - row * C4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < L) v = *(const f32x4*)(src + (long)row * row_stride + 4 * c4);
    *(f32x4*)(dst + row * RS + 4 * c4) = v;
  }
}
// DQ = DH/4 consecutive floats of row `row` starting at column DQ*g (zeros when the row is outside)
template <int DH>
__device__ __forceinline__ void attn_frag(float* f, const float* __restrict__ src, long row_stride, int row, int L, int g) {
  constexpr int DQ = DH / 4;
#pragma unroll
  for (int k = 0; k < DQ; k += 4) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < L) v = *(const f32x4*)(src + (long)row * row_stride + DQ * g + k);
    f[k] = v[0]; f[k + 1] = v[1]; f[k + 2] = v[2]; f[k + 3] = v[3];
  }
}
template <int DH>
__device__ __forceinline__ void attn_lds_frag(float* f, const float* __restrict__ lds_row, int g) {
  constexpr int DQ = DH / 4;
#pragma unroll
  for (int k = 0; k < DQ; k += 4) {
    const f32x4 v = *(const f32x4*)(lds_row + DQ * g + k);
    f[k] = v[0]; f[k + 1] = v[1]; f[k + 2] = v[2]; f[k + 3] = v[3];
  }
}
__device__ __forceinline__ float quad_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// ================================================================================================ two paths, one set of steps
// Resident (L <= 16 ATTN_MAXT): K and V (forward, dQ) or Q and dO (dK, dV) of the head are staged whole, as ONE block of
// roundup(L, 16) rows.  Streamed (any L): the same kernels with the keys (forward, dQ) or the queries (dK, dV) walked in LDS
// blocks of ATTN_SBK rows instead of held whole: nothing is bounded by L but the loop count.  The streamed forward carries a
// running maximum m and running sum l per query (online softmax): per block  m' = max(m, block max), O *= exp(m - m'), l = l exp(m - m') + sum exp(s - m'), O += P V, and
// divides by l once at the end.  m starts at -inf, but m' is finite from the first block on (key k0 of every block is < L), so
// exp(m - m') is exp(-inf) = 0 there and never inf - inf; keys >= L of the tail block get s = -inf, p = 0.  The rescale factor
// lives on lane = query while the O accumulator rows are (g, r): four wave shuffles per block bring it over.  The rescale is
// unconditional (no data-dependent branch).  The streamed dQ additionally writes D = dO . O per query into the caller's (N*H, L)
// workspace; dK, dV (launched after it on the same stream) reads D from there instead of re-reading `out` once per key block.
// One LDS buffer, two barriers per block, every wave takes part in every barrier: a wave whose 16 rows lie beyond L skips the
// arithmetic between the barriers and its stores, never the barriers.  70 KB at DH = 64: two workgroups share a CU and one
// computes while the other stages.  Workgroups are independent, loop bounds depend on L alone, no atomics: bit-reproducible.
// Every tile step below takes the index of the block's first row (k0 / q0) and works on k0 + local; resident passes 0.
#define ATTN_SBK 128                     // rows per streamed LDS block
#define ATTN_SBQ (16 * ATTN_WAVES)       // rows a workgroup owns
// Register budget: up to DH = 48 the streamed forward and dK/dV kernels fit 128 registers (4 waves per SIMD = two workgroups per
// CU); at DH = 64 that cap spills to scratch, so those two run one workgroup per CU there.  0 = no hint (the resident dK/dV).
#define ATTN_STREAM_WAVES(DH) ((DH) <= 48 ? 4 : 2)
#define ATTN_DKV_WAVES(DH, STREAM) ((STREAM) ? ATTN_STREAM_WAVES(DH) : 0)

// What a wave knows about its (frame, head) and its 16 rows: queries in forward and dQ, keys in dK/dV
struct AttnCtx {
  int tid, g, c;        // thread of the workgroup; lane = 16 g + c
  int nh, n, h;         // blockIdx.y = n * H + h
  int E;                // H * DH: a qkv row is q | k | v of E floats each
  long rs, ro;          // floats from one token's row to the next in qkv / dqkv and in out / dout
  long hq, ho;          // where the head starts in token 0's row of qkv / dqkv (its q part) and of out / dout
  int r0, row;          // first of the wave's 16 rows; this lane's row r0 + c
};
template <int DH>
__device__ __forceinline__ AttnCtx attn_ctx(int N, int H) {
  AttnCtx x;
  x.tid = threadIdx.x;
  const int lane = x.tid & 63, wave = x.tid >> 6;
  x.g = lane >> 4; x.c = lane & 15;
  x.nh = blockIdx.y; x.n = x.nh / H; x.h = x.nh - x.n * H;
  x.E = H * DH;
  x.rs = (long)N * 3 * x.E; x.ro = (long)N * x.E;
  x.hq = (long)x.n * 3 * x.E + x.h * DH; x.ho = (long)x.n * x.E + x.h * DH;
  x.r0 = (blockIdx.x * ATTN_WAVES + wave) * 16; x.row = x.r0 + x.c;
  return x;
}
// rows of one LDS block; the kernels carve their LDS by it and the host sizes it by it
__host__ __device__ __forceinline__ int attn_block_rows(bool stream, int L) { return stream ? ATTN_SBK : (L + 15) & ~15; }
// dropout mask index of (query, key 0): ((n*H + h)*L + query)*L
__device__ __forceinline__ uint64_t attn_mask_row(int nh, int query, int L) { return ((uint64_t)nh * L + query) * (uint64_t)L; }
// Key mask (MASK instantiations only; the others are the kernels as they were): key_mask (N, L) bytes, row stride mstride, shared by
// the heads of a frame, non-zero = the key is ignored.  It is read from global memory - a frame's row is a few hundred bytes
// that every workgroup of the frame re-reads from cache - so the LDS carving is the unmasked one.  A lane's four keys of a tile are
// four consecutive bytes at a multiple of 4: one aligned dword (the host checks the alignment of base and stride), byte r = key
// key4 + r; 0 beyond L, where the `key < L` test already decides.  A masked key is dead exactly like a key >= L: score -inf before
// the maximum, p = 0 selected (never computed from exp(s - lse)) in backward.  New with a mask: a block, or a whole row, may have
// no live key, so the maximum may stay -inf; attn_finite_max() keeps exp(-inf - (-inf)) out of the recurrence and the final 1 / l
// and lse are selected for l = 0 (o = 0, lse = -inf).
__device__ __forceinline__ uint32_t attn_mask_word(const uint8_t* __restrict__ mrow, int key4, int L) {
  return key4 < L ? *(const uint32_t*)(mrow + key4) : 0u;
}
__device__ __forceinline__ bool attn_mask_bit(uint32_t mw, int r) { return ((mw >> (8 * r)) & 0xffu) != 0u; }
// the maximum to subtract: 0 instead of -inf when nothing is live yet, so every exp(-inf - 0) is 0 and none is NaN
template <bool MASK>
__device__ __forceinline__ float attn_finite_max(float m) {
  if constexpr (MASK) return m == -INFINITY ? 0.f : m;
  return m;
}
template <int DT>
__device__ __forceinline__ void attn_zero(f32x4* a) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) a[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// Score tile t of the staged keys: S^T = K Q^T (16 keys x the wave's 16 queries), scaled, keys >= L (and masked keys, mw = their
// mask word) at -inf; mx takes its maximum
template <int DH, bool MASK>
__device__ __forceinline__ f32x4 attn_score_tile(const float* Ks, int t, const float* qf, int k0, int L, float scale,
                                                 const AttnCtx& x, float& mx, uint32_t mw) {
  constexpr int DQ = DH / 4, RS = DH + 4;
  float kf[DQ];
  attn_lds_frag<DH>(kf, Ks + (t * 16 + x.c) * RS, x.g);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < DQ; ++k) acc = MFMA16(kf[k], qf[k], acc);      // S^T[key 4g+r][query c]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + t * 16 + 4 * x.g + r;
    bool live = key < L;
    if constexpr (MASK) live = live && !attn_mask_bit(mw, r);
    acc[r] = live ? acc[r] * scale : -INFINITY;
    mx = fmaxf(mx, acc[r]);
  }
  return acc;
}
// s -> exp(s - mx) in place, added to sum
__device__ __forceinline__ void attn_exp_tile(f32x4& s, float mx, float& sum) {
#pragma unroll
  for (int r = 0; r < 4; ++r) { s[r] = expf(s[r] - mx); sum += s[r]; }
}
// O += P V for tile t of the staged values, p (laid out as the score tile) times the dropout factor
template <int DH>
__device__ __forceinline__ void attn_pv_tile(f32x4* o, const float* Vs, int t, f32x4 p, int k0, uint64_t maskrow, float pdrop,
                                             uint64_t seed, const AttnCtx& x) {
  constexpr int RS = DH + 4, DT = DH / 16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kl = t * 16 + 4 * x.g + r;
    float pr = p[r];
    if (pdrop > 0.f) pr *= dropout_scale(seed, maskrow + (uint64_t)(k0 + kl), pdrop);
    const float* vrow = Vs + kl * RS + x.c;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = MFMA16(pr, vrow[dt * 16], o[dt]);   // O[query 4g'+r'][d = 16 dt + c]
  }
}
// The wave's accumulator rows r0 + 4g + r (< L), columns 16 dt + c, to dst + row * stride
template <int DH>
__device__ __forceinline__ void attn_store_rows(float* dst, long stride, const f32x4* acc, const AttnCtx& x, int L) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = x.r0 + 4 * x.g + r;
    if (row < L) {
      float* p = dst + (long)row * stride + x.c;
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) p[dt * 16] = acc[dt][r];
    }
  }
}
// accumulator row r times f (a float) or f[r] (an f32x4)
template <int DT, class F>
__device__ __forceinline__ void attn_scale_rows(f32x4* a, F f) {
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) a[dt] = a[dt] * f;
}
// D[query] = dO . O = sum_j dP_j P_j of this lane's query, from the quad's fragments
template <int DH>
__device__ __forceinline__ float attn_d_frag(const float* dof, const float* __restrict__ out, const AttnCtx& x, int L) {
  constexpr int DQ = DH / 4;
  float of[DQ];
  attn_frag<DH>(of, out + x.ho, x.ro, x.row, L, x.g);
  float dsum = 0.f;
#pragma unroll
  for (int k = 0; k < DQ; ++k) dsum += dof[k] * of[k];
  return quad_group_sum(dsum);
}
// dQ += dS K for tile t of the staged keys and values; the probabilities come back from the row log-sum-exp lq
template <int DH, bool MASK>
__device__ __forceinline__ void attn_dq_tile(f32x4* dq, const float* Ks, const float* Vs, int t, const float* qf, const float* dof,
                                             float lq, float dsum, int k0, uint64_t maskrow, int L, float scale, float pdrop,
                                             uint64_t seed, const AttnCtx& x, uint32_t mw) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16;
  float kf[DQ], vf[DQ];
  attn_lds_frag<DH>(kf, Ks + (t * 16 + x.c) * RS, x.g);
  attn_lds_frag<DH>(vf, Vs + (t * 16 + x.c) * RS, x.g);
  f32x4 st = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < DQ; ++k) {
    st = MFMA16(kf[k], qf[k], st);                // S^T[key][query]
    dp = MFMA16(vf[k], dof[k], dp);               // dPd^T[key][query] = V[key] . dO[query]
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kl = t * 16 + 4 * x.g + r, key = k0 + kl;
    bool live = key < L && x.row < L;
    if constexpr (MASK) live = live && !attn_mask_bit(mw, r);
    const float p = live ? expf(st[r] * scale - lq) : 0.f;
    const float mk = pdrop > 0.f ? dropout_scale(seed, maskrow + (uint64_t)key, pdrop) : 1.f;
    const float ds = p * (dp[r] * mk - dsum);
    const float* krow = Ks + kl * RS + x.c;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = MFMA16(ds, krow[dt * 16], dq[dt]);
  }
}
// dV += Pd^T dO, dK += dS^T Q for tile t of the staged queries (Q, dO, lse and D per query in LDS); the keys are in registers
// (MASK: keylive = this lane's key x.row is not masked)
template <int DH, bool MASK>
__device__ __forceinline__ void attn_dkv_tile(f32x4* dk, f32x4* dv, const float* Qs, const float* Gs, const float* Ls,
                                              const float* Ds, int t, const float* kf, const float* vf, int q0, int L, float scale,
                                              float pdrop, uint64_t seed, const AttnCtx& x, bool keylive) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16;
  float qv[DQ], gv[DQ];
  attn_lds_frag<DH>(qv, Qs + (t * 16 + x.c) * RS, x.g);
  attn_lds_frag<DH>(gv, Gs + (t * 16 + x.c) * RS, x.g);
  f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < DQ; ++k) {
    sv = MFMA16(qv[k], kf[k], sv);                // S[query 4g+r][key c]
    dp = MFMA16(gv[k], vf[k], dp);                // dPd[query][key]
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ql = t * 16 + 4 * x.g + r, q = q0 + ql;
    bool valid = q < L && x.row < L;
    if constexpr (MASK) valid = valid && keylive;
    const float p = valid ? expf(sv[r] * scale - Ls[ql]) : 0.f;
    const float mk = (pdrop > 0.f && valid) ? dropout_scale(seed, attn_mask_row(x.nh, q, L) + (uint64_t)x.row, pdrop) : 1.f;
    const float pd = p * mk;
    const float ds = p * (dp[r] * mk - Ds[ql]);
    const float* grow = Gs + ql * RS + x.c;
    const float* qrow = Qs + ql * RS + x.c;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      dv[dt] = MFMA16(pd, grow[dt * 16], dv[dt]);  // dV[key 4g'+r'][d]
      dk[dt] = MFMA16(ds, qrow[dt * 16], dk[dt]);
    }
  }
}

// ================================================================================================ forward: out (L, N, E), lse (N*H, L)
// Resident: two passes over the ATTN_MAXT register tiles of the whole score row (maximum, then exp and sum)
template <int DH, bool MASK>
__global__ void __launch_bounds__(64 * ATTN_WAVES)
attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse, int L, int N, int H,
                float scale, float pdrop, uint64_t seed, const uint8_t* __restrict__ key_mask, long mstride) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16;
  extern __shared__ float smem[];
  const int Lp = attn_block_rows(false, L), NT = Lp >> 4;
  float* Ks = smem;
  float* Vs = smem + Lp * RS;
  const AttnCtx x = attn_ctx<DH>(N, H);
  const float* base = qkv + x.hq;
  attn_stage<DH>(Ks, base + x.E, x.rs, L, Lp, x.tid);
  attn_stage<DH>(Vs, base + 2 * x.E, x.rs, L, Lp, x.tid);
  float qf[DQ];
  attn_frag<DH>(qf, base, x.rs, x.row, L, x.g);
  __syncthreads();
  if (x.r0 >= L) return;                                         // after the only barrier
  f32x4 s[ATTN_MAXT];
  float mx = -INFINITY;
  const uint8_t* mrow = MASK ? key_mask + (long)x.n * mstride : nullptr;
#pragma unroll
  for (int t = 0; t < ATTN_MAXT; ++t)
    if (t < NT) s[t] = attn_score_tile<DH, MASK>(Ks, t, qf, 0, L, scale, x, mx, MASK ? attn_mask_word(mrow, t * 16 + 4 * x.g, L) : 0u);
  mx = attn_finite_max<MASK>(quad_group_max(mx));                // no live key: 0, every exp below is exp(-inf) = 0
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < ATTN_MAXT; ++t)
    if (t < NT) attn_exp_tile(s[t], mx, sum);
  sum = quad_group_sum(sum);
  const bool dead = MASK && !(sum > 0.f);                        // no live key: o = 0, lse = -inf
  const float inv = dead ? 0.f : 1.f / sum;
  if (x.g == 0 && x.row < L) lse[(long)x.nh * L + x.row] = dead ? -INFINITY : mx + logf(sum);
  f32x4 o[DT];
  attn_zero<DT>(o);
  const uint64_t maskrow = attn_mask_row(x.nh, x.row < L ? x.row : 0, L);
#pragma unroll
  for (int t = 0; t < ATTN_MAXT; ++t)                            // p is normalised BEFORE P V here; streamed divides O by l at the end
    if (t < NT) attn_pv_tile<DH>(o, Vs, t, s[t] * inv, 0, maskrow, pdrop, seed, x);
  attn_store_rows<DH>(out + x.ho, x.ro, o, x, L);
}

// Streamed: the online softmax over key blocks
// With a mask a block may hold no live key: m' = max(m, -inf) is then m; while nothing has been live yet, m' = -inf and the
// exponentials subtract attn_finite_max(m') = 0 instead: a = exp(-inf - 0) = 0 on l = 0 and O = 0, p = exp(-inf - 0) = 0.  A
// later live block finds m = -inf, a = 0, as the first block of the unmasked kernel does.  l = 0 at the end: no live key at all.
template <int DH, bool MASK>
__global__ void __launch_bounds__(64 * ATTN_WAVES) __attribute__((amdgpu_waves_per_eu(ATTN_STREAM_WAVES(DH))))
attn_stream_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse, int L, int N, int H,
                       float scale, float pdrop, uint64_t seed, const uint8_t* __restrict__ key_mask, long mstride) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16, KT = ATTN_SBK / 16;
  extern __shared__ float smem[];
  float* Ks = smem;
  float* Vs = smem + ATTN_SBK * RS;
  const AttnCtx x = attn_ctx<DH>(N, H);
  const float* base = qkv + x.hq;
  float qf[DQ];
  attn_frag<DH>(qf, base, x.rs, x.row, L, x.g);
  f32x4 o[DT];
  attn_zero<DT>(o);
  float m = -INFINITY, l = 0.f;
  const uint64_t maskrow = attn_mask_row(x.nh, x.row < L ? x.row : 0, L);
  const uint8_t* mrow = MASK ? key_mask + (long)x.n * mstride : nullptr;
  for (int k0 = 0; k0 < L; k0 += ATTN_SBK) {
    if (k0) __syncthreads();                                   // every wave has read the previous block
    attn_stage<DH>(Ks, base + x.E + (long)k0 * x.rs, x.rs, L - k0, ATTN_SBK, x.tid);
    attn_stage<DH>(Vs, base + 2 * x.E + (long)k0 * x.rs, x.rs, L - k0, ATTN_SBK, x.tid);
    __syncthreads();
    if (x.r0 < L) {                                            // wave-uniform; no barrier inside
      f32x4 s[KT];
      float bm = -INFINITY;
#pragma unroll
      for (int t = 0; t < KT; ++t)
        s[t] = attn_score_tile<DH, MASK>(Ks, t, qf, k0, L, scale, x, bm, MASK ? attn_mask_word(mrow, k0 + t * 16 + 4 * x.g, L) : 0u);
      const float mn = fmaxf(m, quad_group_max(bm));           // finite without a mask: key k0 < L is in this block
      const float ms = attn_finite_max<MASK>(mn);              // what the exponentials subtract
      const float alpha = expf(m - ms);                        // first live block: exp(-inf) = 0
      float bs = 0.f;
#pragma unroll
      for (int t = 0; t < KT; ++t) attn_exp_tile(s[t], ms, bs);
      l = l * alpha + quad_group_sum(bs);
      m = mn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float a = __shfl(alpha, 4 * x.g + r, 64);        // factor of query 4g+r, from the lane that holds that query
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt][r] *= a;
      }
#pragma unroll
      for (int t = 0; t < KT; ++t) attn_pv_tile<DH>(o, Vs, t, s[t], k0, maskrow, pdrop, seed, x);
    }
  }
  const bool dead = MASK && !(l > 0.f);                          // no live key: o = 0, lse = -inf
  if (x.g == 0 && x.row < L) lse[(long)x.nh * L + x.row] = dead ? -INFINITY : m + logf(l);
  const float inv = dead ? 0.f : 1.f / l;
  f32x4 iv;
#pragma unroll
  for (int r = 0; r < 4; ++r) iv[r] = __shfl(inv, 4 * x.g + r, 64);
  attn_scale_rows<DT>(o, iv);
  attn_store_rows<DH>(out + x.ho, x.ro, o, x, L);
}

// ================================================================================================ backward, both paths
// Two kernels, no atomics: dQ per 16-query wave over the staged K / V blocks, dK and dV per 16-key wave over the staged
// Q / dO blocks.  STREAM = false: one block of roundup(L, 16) rows, the loop runs once.  The first block is staged before the
// wave's own rows are fetched, so those loads overlap; every wave takes part in every barrier.
// dqkv rows like qkv; the streamed dQ also writes D[query] = dO . O -> dws (N*H, L)
template <int DH, bool STREAM, bool MASK>
__global__ void __launch_bounds__(64 * ATTN_WAVES)
attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout,
                   const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ dws, int L, int N, int H, float scale,
                   float pdrop, uint64_t seed, const uint8_t* __restrict__ key_mask, long mstride) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16;
  extern __shared__ float smem[];
  const int BR = attn_block_rows(STREAM, L), NT = BR >> 4;
  float* Ks = smem;
  float* Vs = smem + BR * RS;
  const AttnCtx x = attn_ctx<DH>(N, H);
  const float* base = qkv + x.hq;
  auto stage = [&](int k0) {
    attn_stage<DH>(Ks, base + x.E + (long)k0 * x.rs, x.rs, L - k0, BR, x.tid);
    attn_stage<DH>(Vs, base + 2 * x.E + (long)k0 * x.rs, x.rs, L - k0, BR, x.tid);
  };
  int k0 = 0;
  stage(k0);
  float qf[DQ], dof[DQ];
  attn_frag<DH>(qf, base, x.rs, x.row, L, x.g);
  attn_frag<DH>(dof, dout + x.ho, x.ro, x.row, L, x.g);
  const float dsum = attn_d_frag<DH>(dof, out, x, L);
  const float lq = x.row < L ? lse[(long)x.nh * L + x.row] : 0.f;
  if constexpr (STREAM)                                          // the resident dK/dV sums D itself (see there)
    if (x.g == 0 && x.row < L) dws[(long)x.nh * L + x.row] = dsum;
  f32x4 dq[DT];
  attn_zero<DT>(dq);
  const uint64_t maskrow = attn_mask_row(x.nh, x.row < L ? x.row : 0, L);
  const uint8_t* mrow = MASK ? key_mask + (long)x.n * mstride : nullptr;
  // the mask word of tile t is fetched one tile ahead (the tile loops are not unrolled): mnext is tile t + 1's while t runs
  uint32_t mnext = MASK ? attn_mask_word(mrow, 4 * x.g, L) : 0u;
  auto mword = [&](int t) {
    const uint32_t mw = mnext;
    if constexpr (MASK) mnext = attn_mask_word(mrow, k0 + (t + 1) * 16 + 4 * x.g, L);   // t + 1 = NT: tile 0 of the next block
    return mw;
  };
  for (;;) {
    __syncthreads();                                             // the block is staged
    if (x.r0 < L) {                                              // wave-uniform; no barrier inside
      if constexpr (STREAM) {                                    // blocked summation: a block's sum is added to the total once
        f32x4 dqb[DT];
        attn_zero<DT>(dqb);
        for (int t = 0; t < NT; ++t) attn_dq_tile<DH, MASK>(dqb, Ks, Vs, t, qf, dof, lq, dsum, k0, maskrow, L, scale, pdrop, seed, x, mword(t));
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) dq[dt] += dqb[dt];
      } else {                                                   // one block: straight into dq (0 + x would turn a -0 into +0)
        for (int t = 0; t < NT; ++t) attn_dq_tile<DH, MASK>(dq, Ks, Vs, t, qf, dof, lq, dsum, k0, maskrow, L, scale, pdrop, seed, x, mword(t));
      }
    }
    if (!STREAM || (k0 += BR) >= L) break;                       // the same for every wave; resident: the one block was all
    __syncthreads();                                             // every wave has read the previous block
    stage(k0);
  }
  attn_scale_rows<DT>(dq, scale);
  attn_store_rows<DH>(dqkv + x.hq, x.rs, dq, x, L);
}

// dK, dV: the wave's 16 keys in registers; Q, dO, lse and D per query of a block in LDS.  MASK: the lane's own key is masked or
// not, one byte read once; a masked key's p is selected 0 for every query, so its dK and dV rows are exactly 0
template <int DH, bool STREAM, bool MASK>
__global__ void __launch_bounds__(64 * ATTN_WAVES) __attribute__((amdgpu_waves_per_eu(ATTN_DKV_WAVES(DH, STREAM))))
attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ out, const float* __restrict__ dout,
                    const float* __restrict__ lse, float* __restrict__ dqkv, float* __restrict__ dws, int L, int N, int H, float scale,
                    float pdrop, uint64_t seed, const uint8_t* __restrict__ key_mask, long mstride) {
  constexpr int DQ = DH / 4, RS = DH + 4, DT = DH / 16;
  extern __shared__ float smem[];
  const int BR = attn_block_rows(STREAM, L), NT = BR >> 4;
  float* Qs = smem;
  float* Gs = smem + BR * RS;          // dO
  float* Ls = Gs + BR * RS;            // lse per query
  float* Ds = Ls + BR;                 // dO . O per query
  const AttnCtx x = attn_ctx<DH>(N, H);
  const float* base = qkv + x.hq;
  const float* dob = dout + x.ho;
  auto stage = [&](int q0) {
    attn_stage<DH>(Qs, base + (long)q0 * x.rs, x.rs, L - q0, BR, x.tid);
    attn_stage<DH>(Gs, dob + (long)q0 * x.ro, x.ro, L - q0, BR, x.tid);
    for (int ql = x.tid; ql < BR; ql += 64 * ATTN_WAVES) {
      const int q = q0 + ql;
      float d = 0.f, l = 0.f;
      if (q < L) {
        l = lse[(long)x.nh * L + q];
        if constexpr (STREAM) {                                  // what the dQ kernel stored: a quad-partial sum plus two shuffles
          d = dws[(long)x.nh * L + q];
        } else {                                                 // summed here, serially over DH: another last bit than dQ's D
          const float* ob = out + x.ho;
#pragma unroll
          for (int k = 0; k < DH; k += 4) {
            const f32x4 a = *(const f32x4*)(dob + (long)q * x.ro + k), b = *(const f32x4*)(ob + (long)q * x.ro + k);
            d += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
          }
        }
      }
      Ls[ql] = l;
      Ds[ql] = d;
    }
  };
  int q0 = 0;
  stage(q0);
  float kf[DQ], vf[DQ];
  attn_frag<DH>(kf, base + x.E, x.rs, x.row, L, x.g);
  attn_frag<DH>(vf, base + 2 * x.E, x.rs, x.row, L, x.g);
  f32x4 dk[DT], dv[DT];
  attn_zero<DT>(dk);
  attn_zero<DT>(dv);
  bool keylive = true;
  if constexpr (MASK)
    if (x.row < L) keylive = key_mask[(long)x.n * mstride + x.row] == 0;
  for (;;) {
    __syncthreads();                                             // the block is staged
    if (x.r0 < L)                                                // wave-uniform; no barrier inside
      for (int t = 0; t < NT; ++t) attn_dkv_tile<DH, MASK>(dk, dv, Qs, Gs, Ls, Ds, t, kf, vf, q0, L, scale, pdrop, seed, x, keylive);
    if (!STREAM || (q0 += BR) >= L) break;                       // the same for every wave; resident: the one block was all
    __syncthreads();                                             // every wave has read the previous block
    stage(q0);
  }
  attn_scale_rows<DT>(dk, scale);
  attn_store_rows<DH>(dqkv + x.hq + x.E, x.rs, dk, x, L);
  attn_store_rows<DH>(dqkv + x.hq + 2 * x.E, x.rs, dv, x, L);
}

// ================================================================================================ host
static bool attn_dh_ok(int DH) { return DH == 16 || DH == 32 || DH == 48 || DH == 64; }
// dynamic LDS of kernel `which` (0 forward, 1 dQ, 2 dK/dV): two matrices of one block's rows, dK/dV also lse and D per row
static size_t attn_lds_bytes(int L, int DH, int which, bool stream) {
  const int rows = attn_block_rows(stream, L);
  return (size_t)2 * rows * (DH + 4) * 4 + (which == 2 ? (size_t)2 * rows * 4 : 0);
}

// the key mask of a call: key (N, L) bytes, `stride` bytes from one frame's row to the next; key == nullptr: no mask
struct AttnMask {
  const uint8_t* key;
  long stride;
};

template <int DH, bool STREAM, bool MASK>
static int attn_launch(int which, const float* qkv, const float* out, const float* dout, float* lse, float* dst,
                       float* dws, int L, int N, int H, float p, uint64_t seed, AttnMask mk, hipStream_t st) {
  const float scale = 1.0f / sqrtf((float)DH);
  const dim3 grid(cdiv(L, 16 * ATTN_WAVES), N * H), block(64 * ATTN_WAVES);
  static bool attr[3] = {false, false, false};
  const size_t lds = attn_lds_bytes(L, DH, which, STREAM);
  const auto fwd = STREAM ? attn_stream_fwd_kernel<DH, MASK> : attn_fwd_kernel<DH, MASK>;
  const auto bwd = which == 1 ? attn_bwd_dq_kernel<DH, STREAM, MASK> : attn_bwd_dkv_kernel<DH, STREAM, MASK>;
  if (!attr[which]) {
    if (hipFuncSetAttribute(which == 0 ? (const void*)fwd : (const void*)bwd, hipFuncAttributeMaxDynamicSharedMemorySize,
                            160 * 1024) != hipSuccess) {
      muvo_set_error("%s: cannot raise the dynamic LDS limit", STREAM ? "attention_stream" : "attention");
      return MUVO_ERR_HIP;
    }
    attr[which] = true;
  }
  if (which == 0)
    hipLaunchKernelGGL(fwd, grid, block, lds, st, qkv, dst, lse, L, N, H, scale, p, seed, mk.key, mk.stride);
  else
    hipLaunchKernelGGL(bwd, grid, block, lds, st, qkv, out, dout, (const float*)lse, dst, dws, L, N, H, scale, p, seed, mk.key,
                       mk.stride);
  return MUVO_OK;
}

template <bool STREAM, bool MASK>
static int attn_dispatch(int which, const float* qkv, const float* out, const float* dout, float* lse, float* dst,
                         float* dws, int L, int N, int H, int DH, float p, uint64_t seed, AttnMask mk, hipStream_t st) {
  switch (DH) {
    case 16: return attn_launch<16, STREAM, MASK>(which, qkv, out, dout, lse, dst, dws, L, N, H, p, seed, mk, st);
    case 32: return attn_launch<32, STREAM, MASK>(which, qkv, out, dout, lse, dst, dws, L, N, H, p, seed, mk, st);
    case 48: return attn_launch<48, STREAM, MASK>(which, qkv, out, dout, lse, dst, dws, L, N, H, p, seed, mk, st);
    case 64: return attn_launch<64, STREAM, MASK>(which, qkv, out, dout, lse, dst, dws, L, N, H, p, seed, mk, st);
  }
  muvo_set_error("%s: head dimension %d not supported", STREAM ? "attention_stream" : "attention", DH);
  return MUVO_ERR_INVALID_ARG;
}

// One entry point: the argument check, then kernels first .. last (0 forward, 1 dQ, 2 dK/dV) of the path, queued on st.
// ptrs: the entry point's own pointers are all there.  mk.key == nullptr runs the unmasked instantiations, the kernels as they
// were; a mask must let a lane read its four keys as one aligned dword: base and stride multiples of 4, stride >= roundup(L, 4)
static int attn_run(const char* name, bool stream, int first, int last, bool ptrs, const float* qkv, const float* out,
                    const float* dout, float* lse, float* dst, float* dws, int L, int N, int H, int DH, float p, uint64_t seed,
                    hipStream_t st, AttnMask mk = {nullptr, 0}) {
  MUVO_CHECK_ARG(ptrs && N > 0 && H > 0 && (long)N * H <= 65535, "%s: bad args", name);
  if (stream)
    MUVO_CHECK_ARG(muvo_attention_stream_supported(L, DH), "%s: L = %d, head dim = %d not supported", name, L, DH);
  else
    MUVO_CHECK_ARG(muvo_attention_supported(L, DH), "%s: L = %d, head dim = %d outside the fused kernel's range", name, L, DH);
  MUVO_CHECK_ARG(p >= 0.f && p < 1.f, "%s: dropout probability", name);
  if (mk.key)
    MUVO_CHECK_ARG(((uintptr_t)mk.key & 3) == 0 && (mk.stride & 3) == 0 && mk.stride >= (((long)L + 3) & ~3L),
                   "%s: key mask base and row stride (%ld) must be multiples of 4 bytes, stride >= roundup(L, 4)", name, mk.stride);
  for (int which = first; which <= last; ++which) {
    int rc;
    if (mk.key)
      rc = stream ? attn_dispatch<true, true>(which, qkv, out, dout, lse, dst, dws, L, N, H, DH, p, seed, mk, st)
                  : attn_dispatch<false, true>(which, qkv, out, dout, lse, dst, dws, L, N, H, DH, p, seed, mk, st);
    else
      rc = stream ? attn_dispatch<true, false>(which, qkv, out, dout, lse, dst, dws, L, N, H, DH, p, seed, mk, st)
                  : attn_dispatch<false, false>(which, qkv, out, dout, lse, dst, dws, L, N, H, DH, p, seed, mk, st);
    if (rc) return rc;
  }
  MUVO_CHECK_LAUNCH(name);
  return MUVO_OK;
}

extern "C" {
int muvo_attention_supported(int L, int DH) {
  if (!attn_dh_ok(DH)) return 0;
  if (L < 1 || L > 16 * ATTN_MAXT) return 0;
  return attn_lds_bytes(L, DH, 2, false) <= (size_t)160 * 1024 ? 1 : 0;
}
int muvo_attention_stream_supported(int L, int DH) { return attn_dh_ok(DH) && L >= 1 ? 1 : 0; }
int muvo_attention_stream_blocks(int* bq, int* bk) {
  MUVO_CHECK_ARG(bq && bk, "attention_stream_blocks: null pointer");
  *bq = ATTN_SBQ;
  *bk = ATTN_SBK;
  return MUVO_OK;
}
int muvo_attention_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                       void* stream) {
  return attn_run("attention_fwd", false, 0, 0, qkv && out && lse, qkv, nullptr, nullptr, lse, out, nullptr, L, N, H, DH, p, seed, ST);
}
int muvo_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int L, int N, int H,
                       int DH, float p, uint64_t seed, void* stream) {
  return attn_run("attention_bwd", false, 1, 2, qkv && out && dout && lse && dqkv, qkv, out, dout, (float*)lse, dqkv, nullptr, L, N,
                  H, DH, p, seed, ST);
}
int muvo_attention_stream_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                              void* stream) {
  return attn_run("attention_stream_fwd", true, 0, 0, qkv && out && lse, qkv, nullptr, nullptr, lse, out, nullptr, L, N, H, DH, p,
                  seed, ST);
}
int muvo_attention_stream_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* dws,
                              int L, int N, int H, int DH, float p, uint64_t seed, void* stream) {
  return attn_run("attention_stream_bwd", true, 1, 2, qkv && out && dout && lse && dqkv && dws, qkv, out, dout, (float*)lse, dqkv,
                  dws, L, N, H, DH, p, seed, ST);
}
int muvo_attention_mask_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                            void* stream, const uint8_t* key_mask, int64_t mask_stride) {
  return attn_run("attention_mask_fwd", false, 0, 0, qkv && out && lse, qkv, nullptr, nullptr, lse, out, nullptr, L, N, H, DH, p,
                  seed, ST, {key_mask, (long)mask_stride});
}
int muvo_attention_mask_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int L, int N,
                            int H, int DH, float p, uint64_t seed, void* stream, const uint8_t* key_mask, int64_t mask_stride) {
  return attn_run("attention_mask_bwd", false, 1, 2, qkv && out && dout && lse && dqkv, qkv, out, dout, (float*)lse, dqkv, nullptr,
                  L, N, H, DH, p, seed, ST, {key_mask, (long)mask_stride});
}
int muvo_attention_stream_mask_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                                   void* stream, const uint8_t* key_mask, int64_t mask_stride) {
  return attn_run("attention_stream_mask_fwd", true, 0, 0, qkv && out && lse, qkv, nullptr, nullptr, lse, out, nullptr, L, N, H, DH,
                  p, seed, ST, {key_mask, (long)mask_stride});
}
int muvo_attention_stream_mask_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                   float* dws, int L, int N, int H, int DH, float p, uint64_t seed, void* stream,
                                   const uint8_t* key_mask, int64_t mask_stride) {
  return attn_run("attention_stream_mask_bwd", true, 1, 2, qkv && out && dout && lse && dqkv && dws, qkv, out, dout, (float*)lse,
                  dqkv, dws, L, N, H, DH, p, seed, ST, {key_mask, (long)mask_stride});
}
}
