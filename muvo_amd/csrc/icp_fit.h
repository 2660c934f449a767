// Rigid fit of one ICP step from the 17 inlier sums (icp.hip): Horn's closed form.  With the centred cross-covariance
// M = sum (s - ms)(q - mq)^T the unit quaternion of the rotation that maximises sum (R s) . q is the eigenvector of the largest
// eigenvalue of a symmetric 4 x 4 matrix built from M (Horn 1987, eq. 25).  A quaternion is always a proper rotation, so the
// reflection the SVD form has to guard against (det = -1 for mirrored or planar data) cannot come out, and rank-deficient M
// (three points, a plane) needs no special case.  The eigenvector comes from cyclic Jacobi rotations in fp64.  Every array
// index below is a compile-time constant after unrolling: the matrices stay in registers (the build refuses scratch).
#pragma once
#include <math.h>

#ifndef ICP_HD
#ifdef __HIPCC__
#define ICP_HD __host__ __device__ __forceinline__
#else
#define ICP_HD inline
#endif
#endif

#define ICP_SUMS 17         // count, sum d^2, sum s (3), sum q (3), sum s q^T (9, row = s component)
#define ICP_SWEEPS 16

// one Jacobi rotation of the symmetric a (4 x 4) in the (P, Q) plane, accumulated into v (columns = eigenvectors)
template <int P, int Q>
ICP_HD void icp_jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#define ICP_ROT_COLS(m, k)                      \
  {                                             \
    const double kp = m[k][P], kq = m[k][Q];    \
    m[k][P] = c * kp - s * kq;                  \
    m[k][Q] = s * kp + c * kq;                  \
  }
#define ICP_ROT_ROWS(m, k)                      \
  {                                             \
    const double pk = m[P][k], qk = m[Q][k];    \
    m[P][k] = c * pk - s * qk;                  \
    m[Q][k] = s * pk + c * qk;                  \
  }
  ICP_ROT_COLS(a, 0) ICP_ROT_COLS(a, 1) ICP_ROT_COLS(a, 2) ICP_ROT_COLS(a, 3)      // A <- A J
  ICP_ROT_ROWS(a, 0) ICP_ROT_ROWS(a, 1) ICP_ROT_ROWS(a, 2) ICP_ROT_ROWS(a, 3)      // A <- J^T A
  a[P][Q] = 0.0;
  a[Q][P] = 0.0;
  ICP_ROT_COLS(v, 0) ICP_ROT_COLS(v, 1) ICP_ROT_COLS(v, 2) ICP_ROT_COLS(v, 3)
#undef ICP_ROT_COLS
#undef ICP_ROT_ROWS
}

// sums[17] over the inliers (count >= 3) -> U (3 x 4, row-major): q ~ U [s; 1]
ICP_HD void icp_rigid_fit(const double* sums, double (&U)[12]) {
  const double inv = 1.0 / sums[0];
  const double ms0 = sums[2] * inv, ms1 = sums[3] * inv, ms2 = sums[4] * inv;
  const double mq0 = sums[5] * inv, mq1 = sums[6] * inv, mq2 = sums[7] * inv;
  const double Sxx = sums[8] * inv - ms0 * mq0, Sxy = sums[9] * inv - ms0 * mq1, Sxz = sums[10] * inv - ms0 * mq2;
  const double Syx = sums[11] * inv - ms1 * mq0, Syy = sums[12] * inv - ms1 * mq1, Syz = sums[13] * inv - ms1 * mq2;
  const double Szx = sums[14] * inv - ms2 * mq0, Szy = sums[15] * inv - ms2 * mq1, Szz = sums[16] * inv - ms2 * mq2;
  double a[4][4], v[4][4];
  a[0][0] = Sxx + Syy + Szz; a[0][1] = Syz - Szy;       a[0][2] = Szx - Sxz;        a[0][3] = Sxy - Syx;
  a[1][0] = a[0][1];         a[1][1] = Sxx - Syy - Szz; a[1][2] = Sxy + Syx;        a[1][3] = Szx + Sxz;
  a[2][0] = a[0][2];         a[2][1] = a[1][2];         a[2][2] = -Sxx + Syy - Szz; a[2][3] = Syz + Szy;
  a[3][0] = a[0][3];         a[3][1] = a[1][3];         a[3][2] = a[2][3];          a[3][3] = -Sxx - Syy + Szz;
  v[0][0] = 1.0; v[0][1] = 0.0; v[0][2] = 0.0; v[0][3] = 0.0;
  v[1][0] = 0.0; v[1][1] = 1.0; v[1][2] = 0.0; v[1][3] = 0.0;
  v[2][0] = 0.0; v[2][1] = 0.0; v[2][2] = 1.0; v[2][3] = 0.0;
  v[3][0] = 0.0; v[3][1] = 0.0; v[3][2] = 0.0; v[3][3] = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < ICP_SWEEPS; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] + a[2][3] * a[2][3];
    const double diag = a[0][0] * a[0][0] + a[1][1] * a[1][1] + a[2][2] * a[2][2] + a[3][3] * a[3][3];
    if (off <= 1e-40 * diag) break;             // off-diagonal below 1e-20 relative: converged (quadratically, 5-7 sweeps)
    icp_jacobi_rotate<0, 1>(a, v);
    icp_jacobi_rotate<0, 2>(a, v);
    icp_jacobi_rotate<0, 3>(a, v);
    icp_jacobi_rotate<1, 2>(a, v);
    icp_jacobi_rotate<1, 3>(a, v);
    icp_jacobi_rotate<2, 3>(a, v);
  }
  // eigenvector of the largest eigenvalue (the lowest column on a tie), selected without a runtime index
  const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2], d3 = a[3][3];
  const double v00 = v[0][0], v10 = v[1][0], v20 = v[2][0], v30 = v[3][0], v01 = v[0][1], v11 = v[1][1], v21 = v[2][1], v31 = v[3][1];
  const double v02 = v[0][2], v12 = v[1][2], v22 = v[2][2], v32 = v[3][2], v03 = v[0][3], v13 = v[1][3], v23 = v[2][3], v33 = v[3][3];
  double best = d0, w = v00, x = v10, y = v20, z = v30;
  const bool b1 = d1 > best;
  best = b1 ? d1 : best; w = b1 ? v01 : w; x = b1 ? v11 : x; y = b1 ? v21 : y; z = b1 ? v31 : z;
  const bool b2 = d2 > best;
  best = b2 ? d2 : best; w = b2 ? v02 : w; x = b2 ? v12 : x; y = b2 ? v22 : y; z = b2 ? v32 : z;
  const bool b3 = d3 > best;
  w = b3 ? v03 : w; x = b3 ? v13 : x; y = b3 ? v23 : y; z = b3 ? v33 : z;
  const double nrm = 1.0 / sqrt(w * w + x * x + y * y + z * z);
  w *= nrm; x *= nrm; y *= nrm; z *= nrm;
  const double r00 = 1.0 - 2.0 * (y * y + z * z), r01 = 2.0 * (x * y - w * z), r02 = 2.0 * (x * z + w * y);
  const double r10 = 2.0 * (x * y + w * z), r11 = 1.0 - 2.0 * (x * x + z * z), r12 = 2.0 * (y * z - w * x);
  const double r20 = 2.0 * (x * z - w * y), r21 = 2.0 * (y * z + w * x), r22 = 1.0 - 2.0 * (x * x + y * y);
  U[0] = r00; U[1] = r01; U[2] = r02;  U[3] = mq0 - (r00 * ms0 + r01 * ms1 + r02 * ms2);
  U[4] = r10; U[5] = r11; U[6] = r12;  U[7] = mq1 - (r10 * ms0 + r11 * ms1 + r12 * ms2);
  U[8] = r20; U[9] = r21; U[10] = r22; U[11] = mq2 - (r20 * ms0 + r21 * ms1 + r22 * ms2);
}

// T <- U T on 3 x 4 row-major affine matrices
ICP_HD void icp_compose(const double (&U)[12], double (&T)[12]) {
  double R[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      R[i * 4 + j] = U[i * 4 + 0] * T[0 * 4 + j] + U[i * 4 + 1] * T[1 * 4 + j] + U[i * 4 + 2] * T[2 * 4 + j] + (j == 3 ? U[i * 4 + 3] : 0.0);
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = R[k];
}
