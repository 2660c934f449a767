// Per-element steps of the RSSM: the GRU cell and the (mu | log sigma) -> sigma, sample step with their adjoints, one copy for
// the per-op kernels of elementwise.hip and the persistent kernels of rssm.hip.  The helpers take LOADED values: the persistent
// kernels read what another workgroup wrote through coh_load, the per-op kernels read plainly, so the load stays with the caller.
// The library is built with -ffp-contract=off: each helper fixes the order of its float32 operations, and the emulations in
// tests/elementwise_reference.py (gru_eval, sample_eval) restate that order.
#pragma once
#include "common.h"

// torch.nn.GRUCell: r = s(gi_r+gh_r), z = s(gi_z+gh_z), n = tanh(gi_n + r*gh_n), h' = (1-z)*n + z*h
struct GruGates { float r, z, n; };
__device__ __forceinline__ GruGates gru_gates(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n) {
  GruGates q;
  q.r = sigmoidf_(gi_r + gh_r);
  q.z = sigmoidf_(gi_z + gh_z);
  q.n = tanhf(gi_n + q.r * gh_n);
  return q;
}
__device__ __forceinline__ float gru_combine(const GruGates& q, float h) { return (1.f - q.z) * q.n + q.z * h; }
// g = dL/dh': dgi = (dpre_r, dpre_z, dpre_n), dgh = (dpre_r, dpre_z, dgh_n), and dh, the direct g z path to h
struct GruAdjoint { float dpre_r, dpre_z, dpre_n, dgh_n, dh; };
__device__ __forceinline__ GruAdjoint gru_adjoint(const GruGates& q, float gh_n, float h, float g) {
  const float dn = g * (1.f - q.z);
  const float dz = g * (h - q.n);
  GruAdjoint d;
  d.dpre_n = dn * (1.f - q.n * q.n);
  d.dpre_r = d.dpre_n * gh_n * q.r * (1.f - q.r);
  d.dpre_z = dz * q.z * (1.f - q.z);
  d.dgh_n = d.dpre_n * q.r;
  d.dh = g * q.z;
  return d;
}

// sigma = 2*sigmoid(ls/2) + min_std, sample = mu + sigma*eps   (transition.py:18-24,176-181)
__device__ __forceinline__ float rssm_sigma(float ls, float min_std) { return 2.f * sigmoidf_(ls * 0.5f) + min_std; }
__device__ __forceinline__ float rssm_sample(float mu, float sigma, float eps) { return mu + sigma * eps; }
// the gradients of (mu | log sigma) from those of mu, sigma and the sample (an absent one is passed as 0)
struct SampleAdjoint { float dmu, dls; };
__device__ __forceinline__ SampleAdjoint rssm_sample_adjoint(float ls, float eps, float dmu, float dsigma, float dsample) {
  const float s = sigmoidf_(ls * 0.5f);
  SampleAdjoint d;
  d.dmu = dmu + dsample;
  d.dls = (dsigma + dsample * eps) * s * (1.f - s);
  return d;
}
