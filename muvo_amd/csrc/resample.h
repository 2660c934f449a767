// Per-element steps of the resampling and normalising kernels, one copy for elementwise.hip, bev.hip and augment.hip.
// The library is built with -ffp-contract=off: each helper fixes the order of its float32 operations, and the emulations in
// tests/elementwise_reference.py restate that order.
#pragma once
#include "common.h"

// flat index of a contiguous (nc, y, x) resp. (nc, z, y, x) array -> its coordinates; returns nc
__device__ __forceinline__ long split_index(long i, int Y, int X, int& y, int& x) {
  x = (int)(i % X);
  const long r = i / X;
  y = (int)(r % Y);
  return r / Y;
}
__device__ __forceinline__ long split_index(long i, int Z, int Y, int X, int& z, int& y, int& x) {
  x = (int)(i % X);
  long r = i / X;
  y = (int)(r % Y);
  r /= Y;
  z = (int)(r % Z);
  return r / Z;
}

// linear interpolation, align_corners=False: output index o reads the inputs i0 and i1 (of n_in) with weights 1 - w1 and w1;
// scale = n_in / n_out in float32 (the x2 upsample passes the literal 0.5f)
__device__ __forceinline__ void lin_src(int o, int n_in, float scale, int& i0, int& i1, float& w1) {
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  w1 = src - (float)i0;
}
// the weight with which output index o reads input index i (the adjoint gathers)
__device__ __forceinline__ float lin_w(int o, int i, int n_in, float scale) {
  int i0, i1;
  float w1;
  lin_src(o, n_in, scale, i0, i1, w1);
  return (i0 == i ? 1.f - w1 : 0.f) + (i1 == i ? w1 : 0.f);
}
// legacy 'nearest': src = floor(o * n_in / n_out), clamped to the last input
__device__ __forceinline__ int nearest_src(int o, int n_in, float scale) {
  const int s = (int)floorf((float)o * scale);
  return s > n_in - 1 ? n_in - 1 : s;
}

// per-channel mean / std of a three-channel image (a by-value kernel argument: six floats, as the six scalars before it)
struct Norm3 { float m0, m1, m2, s0, s1, s2; };
static inline Norm3 norm3_of(const float* mean3, const float* std3) {
  return Norm3{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
}
__device__ __forceinline__ float normalise3(const Norm3& k, int c, float v) {
  const float m = c == 0 ? k.m0 : (c == 1 ? k.m1 : k.m2), s = c == 0 ? k.s0 : (c == 1 ? k.s1 : k.s2);
  return (v - m) / s;
}
