// Device functions of the input pipeline shared by the per-frame entry points (input.hip) and the batched ones (dataset.hip).
#pragma once
#include "common.h"

struct RangeArgs {
  double lidar[3];        // POINTS.LIDAR_POSITION
  double ego_lo[3], ego_hi[3];
  double fov_down_abs, fov;   // |fov_down|, fov_up - fov_down  (radians)
  int H, W;
};

// Geometry of one point exactly as the reference does it: float32 conversion to the ego frame, float64 projection.
__device__ __forceinline__ bool range_point(const float* __restrict__ raw, long i, const RangeArgs& a, float (&p)[3], double& depth,
                                            int& ph, int& pw) {
  // convert_coor_lidar (data_preprocessing.py:119-122): float32 += position, y mirrored
  p[0] = (float)((double)raw[i * 3] + a.lidar[0]);
  p[1] = -(float)((double)raw[i * 3 + 1] + a.lidar[1]);
  p[2] = (float)((double)raw[i * 3 + 2] + a.lidar[2]);
  // ego-vehicle box (dataset.py:286-290), strict inequalities in float64
  const bool ego = a.ego_lo[0] < (double)p[0] && (double)p[0] < a.ego_hi[0] && a.ego_lo[1] < (double)p[1] &&
                   (double)p[1] < a.ego_hi[1] && a.ego_lo[2] < (double)p[2] && (double)p[2] < a.ego_hi[2];
  if (ego) return false;
  // do_range_projection (geometry_utils.py:176-198)
  const double cx = (double)p[0] - a.lidar[0], cy = -(double)p[1] - a.lidar[1], cz = (double)p[2] - a.lidar[2];
  depth = sqrt(cx * cx + cy * cy + cz * cz);
  const double yaw = atan2(-cy, cx), pitch = asin(cz / depth);
  double fw = floor(0.5 * (1.0 - yaw / M_PI) * (double)a.W), fh = floor((1.0 - (pitch + a.fov_down_abs) / a.fov) * (double)a.H);
  fw = fmin((double)(a.W - 1), fw); fw = fmax(0.0, fw);
  fh = fmin((double)(a.H - 1), fh); fh = fmax(0.0, fh);
  pw = (int)fw; ph = (int)fh;
  return true;
}

// what a range-view pixel holds: x, y, z, depth and the remapped label of its winning point, or the fill values
__device__ __forceinline__ void range_pixel(const float* __restrict__ raw, const unsigned char* __restrict__ tag,
                                            const unsigned char* __restrict__ remap, const RangeArgs& a, unsigned int w, float (&p)[3],
                                            float& d, unsigned char& s) {
  p[0] = p[1] = p[2] = 0.f;
  d = -1.f;
  s = 0;
  if (w != 0xffffffffu) {
    double depth; int ph, pw;
    range_point(raw, (long)w, a, p, depth, ph, pw);
    d = (float)depth;
    s = remap[tag[w]];
  }
}

// voxels[x][y][z] = remap[tag] of the LAST row that names the voxel (numpy fancy assignment): atomicMax on (row << 8 | value)
__device__ __forceinline__ void voxel_scatter_row(const long long* __restrict__ rows, long i, const unsigned char* __restrict__ remap,
                                                  int X, int Y, int Z, unsigned int* __restrict__ key) {
  const long long x = rows[i * 4], y = rows[i * 4 + 1], z = rows[i * 4 + 2];
  long long t = rows[i * 4 + 3];
  if (x < 0 || x >= X || y < 0 || y >= Y || z < 0 || z >= Z) return;
  if (t == 255) t = 0;
  atomicMax(key + ((x * Y + y) * Z + z), ((unsigned int)(i + 1) << 8) | (unsigned int)remap[t]);
}

static inline RangeArgs range_args(const double* lidar_pos, const double* ego_dim, double fov_down_deg, double fov_up_deg, int H, int W) {
  RangeArgs a;
  for (int k = 0; k < 3; ++k) a.lidar[k] = lidar_pos[k];
  a.ego_lo[0] = -ego_dim[0] / 2; a.ego_lo[1] = -ego_dim[1] / 2; a.ego_lo[2] = 0.0;
  a.ego_hi[0] = ego_dim[0] / 2; a.ego_hi[1] = ego_dim[1] / 2; a.ego_hi[2] = ego_dim[2];
  const double fd = fov_down_deg / 180.0 * M_PI, fu = fov_up_deg / 180.0 * M_PI;
  a.fov_down_abs = fabs(fd); a.fov = fu - fd; a.H = H; a.W = W;
  return a;
}
