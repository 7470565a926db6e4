// Drive slicing on the GPU: the reference's data preparation (tools/generate_train_data.py:134-182,
// 247-273; tools/augment_train_data.py:18-54), whose per-slice loop makes a full numpy pass over
// the merged cloud for every slice.
//   drv_pose_kernel     per slice: float32 pose x/y for the radius test, fp64 translation and the
//                       inverse rotation matrix of the normalised quaternion [qx,qy,qz,qw]
//   drv_slice_kernel    COUNT: per (256-point unit, slice) the number of points that pass the
//                       float32 radius test and the fp64 x-crop; FILL: the same tests again, the
//                       survivors written in cloud order at offsets[s] + tile base + unit prefix +
//                       rank inside the wave (64-bit ballot + popcount of the lower lanes)
//   drv_tile_scan_kernel / drv_tile_base_kernel   exclusive scans of those counts: units inside
//                       a tile, tiles inside a slice, slices -> offsets
//   drv_clip_kernel     one thread per (slice, polyline): transform + clip_polyline_by_x
//   drv_centroid_kernel / drv_noise_kernel   generate_noisy_line with the draws taken from a
//                       counter hash of (seed, line, candidate, vertex, component), or supplied
// A unit is owned by ONE wave (4 rounds of 64 points), so ranking needs neither LDS nor a barrier,
// and no atomics are used anywhere: every output is bitwise reproducible from run to run.
// The radius test is float32 with every operation rounded separately, everything else fp64; FMA
// contraction is off throughout so the clip's p1 + t * (p2 - p1) rounds as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_context.hpp"      // ctx_mix / ctx_hash: the library's counter hash

namespace prh {

constexpr int DRV_UNIT = 256;        // consecutive cloud points one wave owns (4 rounds of 64)
constexpr int DRV_ROUNDS = DRV_UNIT / 64;
constexpr int DRV_TILE = 256;        // units per scan tile
constexpr int DRV_MAX_SCALES = 8;    // noise scales (candidates per line) per call

struct DrvPose {
  double t[3];       // pose position
  double m[9];       // inverse rotation, row major: local = m * (p - t)
  float fx, fy;      // float32(pose x / y): the radius pre-filter runs in float32
};
struct DrvScales { double s[DRV_MAX_SCALES]; };

// poses [S,7] = x y z qx qy qz qw
__global__ __launch_bounds__(256) void drv_pose_kernel(const double* __restrict__ poses, int S,
                                                       DrvPose* __restrict__ out) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  const double* p = poses + (size_t)s * 7;
  DrvPose o;
  o.t[0] = p[0]; o.t[1] = p[1]; o.t[2] = p[2];
  o.fx = (float)p[0]; o.fy = (float)p[1];
  double x = p[3], y = p[4], z = p[5], w = p[6];
  const double nrm = sqrt(x * x + y * y + z * z + w * w);
  x /= nrm; y /= nrm; z /= nrm; w /= nrm;
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  // rotation matrix r of the quaternion; its inverse is the transpose
  const double r00 = x2 - y2 - z2 + w2, r01 = 2.0 * (xy - zw), r02 = 2.0 * (xz + yw);
  const double r10 = 2.0 * (xy + zw), r11 = -x2 + y2 - z2 + w2, r12 = 2.0 * (yz - xw);
  const double r20 = 2.0 * (xz - yw), r21 = 2.0 * (yz + xw), r22 = -x2 - y2 + z2 + w2;
  o.m[0] = r00; o.m[1] = r10; o.m[2] = r20;
  o.m[3] = r01; o.m[4] = r11; o.m[5] = r21;
  o.m[6] = r02; o.m[7] = r12; o.m[8] = r22;
  out[s] = o;
}

__device__ __forceinline__ void drv_local(const DrvPose& ps, double gx, double gy, double gz, double& lx,
                                          double& ly, double& lz) {
#pragma clang fp contract(off)
  const double cx = gx - ps.t[0], cy = gy - ps.t[1], cz = gz - ps.t[2];
  lx = (ps.m[0] * cx + ps.m[1] * cy) + ps.m[2] * cz;
  ly = (ps.m[3] * cx + ps.m[4] * cy) + ps.m[5] * cz;
  lz = (ps.m[6] * cx + ps.m[7] * cy) + ps.m[8] * cz;
}

// One wave per unit of 256 consecutive points; a block is 4 independent waves (no barrier).
//   cnt [n_units,S]: COUNT writes the unit's count per slice; FILL reads the exclusive prefix of
//                    the unit inside its tile that drv_tile_scan_kernel left there
//   tile_base [n_tiles,S], offsets [S+1]: FILL only
//   out_pts [capacity,4] local xyz + intensity, out_idx [capacity] cloud row of each emitted point
template <bool FILL>
__global__ __launch_bounds__(256) void drv_slice_kernel(const float4* __restrict__ cloud, int npts,
                                                        const DrvPose* __restrict__ pose, int S, float r2,
                                                        double half, int* __restrict__ cnt,
                                                        const long long* __restrict__ tile_base,
                                                        const long long* __restrict__ offsets,
                                                        double* __restrict__ out_pts,
                                                        long long* __restrict__ out_idx, long long capacity) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const long long unit = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long p0 = unit * DRV_UNIT;
  if (p0 >= npts) return;                          // the whole wave leaves together
  float4 v[DRV_ROUNDS];
  bool live[DRV_ROUNDS];
#pragma unroll
  for (int r = 0; r < DRV_ROUNDS; ++r) {
    const long long p = p0 + r * 64 + lane;
    live[r] = p < npts;
    v[r] = live[r] ? cloud[p] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const unsigned long long lower = (1ull << lane) - 1ull;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int ns = S - s0 < 64 ? S - s0 : 64;
    long long base = 0;
    int mine = 0;
    if (FILL && lane < ns)
      base = offsets[s0 + lane] + tile_base[(size_t)(unit / DRV_TILE) * S + s0 + lane] +
             (long long)cnt[(size_t)unit * S + s0 + lane];
    for (int j = 0; j < ns; ++j) {
      const DrvPose& ps = pose[s0 + j];
      const float fx = ps.fx, fy = ps.fy;
      long long run = FILL ? __shfl(base, j) : 0;
      int c = 0;
#pragma unroll
      for (int r = 0; r < DRV_ROUNDS; ++r) {
        bool in = false;
        double lx = 0.0, ly = 0.0, lz = 0.0;
        if (live[r]) {
          const float dx = v[r].x - fx, dy = v[r].y - fy;
          const float dx2 = dx * dx, dy2 = dy * dy;
          if (dx2 + dy2 < r2) {
            drv_local(ps, (double)v[r].x, (double)v[r].y, (double)v[r].z, lx, ly, lz);
            in = lx >= -half && lx <= half;
          }
        }
        const unsigned long long bal = __ballot(in);
        if (FILL) {
          const long long pos = run + __popcll(bal & lower);
          if (in && pos < capacity) {
            double2* o = reinterpret_cast<double2*>(out_pts + 4 * pos);
            o[0] = make_double2(lx, ly);
            o[1] = make_double2(lz, (double)v[r].w);
            out_idx[pos] = p0 + r * 64 + lane;
          }
          run += __popcll(bal);
        } else {
          c += __popcll(bal);
        }
      }
      if (!FILL && lane == j) mine = c;
    }
    if (!FILL && lane < ns) cnt[(size_t)unit * S + s0 + lane] = mine;
  }
}

// cnt [n_units,S] -> exclusive prefix over the units of each tile, in place; tile_tot [n_tiles,S]
__global__ __launch_bounds__(256) void drv_tile_scan_kernel(int* __restrict__ cnt, long long n_units, int S,
                                                            long long* __restrict__ tile_tot) {
  const int s = blockIdx.y * 256 + threadIdx.x;
  if (s >= S) return;
  const long long u0 = (long long)blockIdx.x * DRV_TILE;
  const long long u1 = u0 + DRV_TILE < n_units ? u0 + DRV_TILE : n_units;
  int run = 0;
  for (long long u = u0; u < u1; ++u) {
    const int t = cnt[(size_t)u * S + s];
    cnt[(size_t)u * S + s] = run;
    run += t;
  }
  tile_tot[(size_t)blockIdx.x * S + s] = run;
}

// one block: tile totals -> exclusive tile bases per slice (in place), slice totals -> offsets [S+1]
__global__ __launch_bounds__(256) void drv_tile_base_kernel(long long* __restrict__ tile, long long n_tiles, int S,
                                                            long long* __restrict__ offsets) {
  for (int s = threadIdx.x; s < S; s += 256) {
    long long run = 0;
    for (long long t = 0; t < n_tiles; ++t) {
      const long long c = tile[(size_t)t * S + s];
      tile[(size_t)t * S + s] = run;
      run += c;
    }
    offsets[s + 1] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long run = 0;
    offsets[0] = 0;
    for (int s = 0; s < S; ++s) { run += offsets[s + 1]; offsets[s + 1] = run; }
  }
}

// clip_polyline_by_x (generate_train_data.py:145-182) of polyline l in the frame of slice s, one
// thread per (s, l), vertices walked in order (the append rule depends on the previous output).
//   verts [*,3] with CSR line_off [NL+1]; counts [S*NL] output vertices (both passes compute it);
//   WRITE: vertices to out + 3 * out_off[s*NL + l]
template <bool WRITE>
__global__ __launch_bounds__(256) void drv_clip_kernel(const double* __restrict__ verts,
                                                       const long long* __restrict__ line_off, int NL,
                                                       const DrvPose* __restrict__ pose, int S, double half,
                                                       int* __restrict__ counts,
                                                       const long long* __restrict__ out_off,
                                                       double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)S * NL) return;
  const int s = (int)(i / NL), l = (int)(i % NL);
  const DrvPose ps = pose[s];
  const long long n = line_off[l + 1] - line_off[l];
  const double* v = verts + 3 * line_off[l];
  double* o = WRITE ? out + 3 * out_off[i] : nullptr;
  const double x_min = -half, x_max = half;
  int k = 0;
  if (n == 1) {
    double x, y, z;
    drv_local(ps, v[0], v[1], v[2], x, y, z);
    if (x_min <= x && x <= x_max) {
      if (WRITE) { o[0] = x; o[1] = y; o[2] = z; }
      k = 1;
    }
  } else if (n >= 2) {
    double ax, ay, az, lx = 0.0, ly = 0.0, lz = 0.0;          // l*: the last vertex appended
    drv_local(ps, v[0], v[1], v[2], ax, ay, az);
    for (long long q = 1; q < n; ++q) {
      double bx, by, bz;
      drv_local(ps, v[3 * q], v[3 * q + 1], v[3 * q + 2], bx, by, bz);
      double t0 = 0.0, t1 = 1.0;
      const double dx = bx - ax;
      bool keep = true;
      if (fabs(dx) < 1e-6) {
        if (ax < x_min || ax > x_max) keep = false;
      } else {
        const double t_min = (x_min - ax) / dx, t_max = (x_max - ax) / dx;
        if (dx > 0) { t0 = fmax(t0, t_min); t1 = fmin(t1, t_max); }
        else        { t0 = fmax(t0, t_max); t1 = fmin(t1, t_min); }
      }
      if (keep && t0 <= t1) {
        const double ex = bx - ax, ey = by - ay, ez = bz - az;
        const double sx = ax + t0 * ex, sy = ay + t0 * ey, sz = az + t0 * ez;
        const double fx = ax + t1 * ex, fy = ay + t1 * ey, fz = az + t1 * ez;
        bool first = k == 0;
        if (!first) {
          const double ux = lx - sx, uy = ly - sy, uz = lz - sz;
          first = sqrt((ux * ux + uy * uy) + uz * uz) > 1e-6;
        }
        if (first) {
          if (WRITE) { o[3 * k] = sx; o[3 * k + 1] = sy; o[3 * k + 2] = sz; }
          ++k;
        }
        if (WRITE) { o[3 * k] = fx; o[3 * k + 1] = fy; o[3 * k + 2] = fz; }
        ++k;
        lx = fx; ly = fy; lz = fz;
      }
      ax = bx; ay = by; az = bz;
    }
  }
  if (!WRITE) counts[i] = k;
}

// centroid [L,3]: np.mean(pts, axis=0), rows added in order
__global__ __launch_bounds__(256) void drv_centroid_kernel(const double* __restrict__ verts,
                                                           const long long* __restrict__ line_off, int L,
                                                           double* __restrict__ centroid) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 3 * L) return;
  const int l = i / 3, c = i % 3;
  const long long a = line_off[l], b = line_off[l + 1];
  double acc = 0.0;
  for (long long q = a; q < b; ++q) acc += verts[3 * q + c];
  centroid[i] = b > a ? acc / (double)(b - a) : 0.0;
}

__device__ __forceinline__ uint64_t drv_hash(uint64_t seed, unsigned line, unsigned cand, unsigned vertex_slot,
                                             unsigned comp) {
  return ctx_hash(ctx_mix(seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(cand + 1))), line, vertex_slot * 4u + comp);
}
__device__ __forceinline__ double drv_sym(uint64_t h) {          // uniform in [-1, 1), 53 bits
  return 2.0 * ((double)(h >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}
__device__ __forceinline__ double drv_normal(uint64_t h) {       // Box-Muller from the two halves of one hash
  const double u1 = ((double)(h >> 32) + 1.0) * (1.0 / 4294967296.0);            // (0, 1]
  const double u2 = (double)(h & 0xFFFFFFFFull) * (1.0 / 4294967296.0);          // [0, 1)
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925 * u2);
}

// generate_noisy_line (augment_train_data.py:18-54) for vertex q of line l under scale k:
//   out[k][q] = (p - c) @ R(yaw).T + c + shift + jitter.
// DRAW: yaw ~ U(+-5 deg * s), dx, dy ~ U(+-s), dz ~ U(+-0.1), jitter ~ N(0, 0.05 / 0.05 / 0.025)
// from drv_hash(seed, line id, k, vertex, component), also stored to draws_u [L,K,4] (yaw in rad,
// dx, dy, dz) and draws_j [K,V,3]; otherwise both are read.  line_of [V] line of each vertex;
// line_ids [L] or NULL (= the line's position) is the line number the hash sees.
template <bool DRAW>
__global__ __launch_bounds__(256) void drv_noise_kernel(const double* __restrict__ verts,
                                                        const long long* __restrict__ line_off,
                                                        const int* __restrict__ line_of, long long V, int L,
                                                        const int* __restrict__ line_ids, DrvScales scales, int K,
                                                        uint64_t seed, const double* __restrict__ centroid,
                                                        double* __restrict__ draws_u, double* __restrict__ draws_j,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= V * K) return;
  const int k = (int)(i / V);
  const long long q = i % V;
  const int l = line_of[q];
  const long long local = q - line_off[l];
  double u[4], jit[3];
  if (DRAW) {
    const unsigned id = line_ids ? (unsigned)line_ids[l] : (unsigned)l;
    const double s = scales.s[k];
    u[0] = ((5.0 * s) * drv_sym(drv_hash(seed, id, (unsigned)k, 0u, 0u))) * (3.14159265358979323846 / 180.0);
    u[1] = s * drv_sym(drv_hash(seed, id, (unsigned)k, 0u, 1u));
    u[2] = s * drv_sym(drv_hash(seed, id, (unsigned)k, 0u, 2u));
    u[3] = 0.1 * drv_sym(drv_hash(seed, id, (unsigned)k, 0u, 3u));
    const unsigned slot = (unsigned)local + 1u;
    jit[0] = 0.05 * drv_normal(drv_hash(seed, id, (unsigned)k, slot, 0u));
    jit[1] = 0.05 * drv_normal(drv_hash(seed, id, (unsigned)k, slot, 1u));
    jit[2] = 0.025 * drv_normal(drv_hash(seed, id, (unsigned)k, slot, 2u));
    if (local == 0)
      for (int c = 0; c < 4; ++c) draws_u[((size_t)l * K + k) * 4 + c] = u[c];
    for (int c = 0; c < 3; ++c) draws_j[((size_t)k * V + q) * 3 + c] = jit[c];
  } else {
    for (int c = 0; c < 4; ++c) u[c] = draws_u[((size_t)l * K + k) * 4 + c];
    for (int c = 0; c < 3; ++c) jit[c] = draws_j[((size_t)k * V + q) * 3 + c];
  }
  const double cs = cos(u[0]), sn = sin(u[0]);
  const double* c0 = centroid + 3 * (size_t)l;
  const double px = verts[3 * q] - c0[0], py = verts[3 * q + 1] - c0[1], pz = verts[3 * q + 2] - c0[2];
  const double rx = px * cs + py * (-sn), ry = px * sn + py * cs;
  double* o = out + ((size_t)k * V + q) * 3;
  o[0] = ((rx + c0[0]) + u[1]) + jit[0];
  o[1] = ((ry + c0[1]) + u[2]) + jit[1];
  o[2] = ((pz + c0[2]) + u[3]) + jit[2];
}

}  // namespace prh
