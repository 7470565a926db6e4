// Map fusion on the GPU: the refined pieces of a drive (M points each, in the ego frame of their
// slice) merged into one polyline per carrier line in the drive frame.  The rule is written out in
// include/pointnet_refine_hip.h ("Map fusion - the rule"); tests/_fuse_oracle.py restates it.
//   fuse_project_kernel  one thread per piece point: ego -> drive frame (DrvPose of prh_drive.hpp,
//                        applied transposed), then the nearest point of the piece's carrier; the
//                        carrier's vertices and arc lengths go through LDS FUSE_TILE segments at a
//                        time, and every lane of a wave reads the same LDS address (a broadcast)
//   fuse_range_kernel    per piece [min s, max s]: what fuse_gather rejects a piece by
//   fuse_gather_kernel   one thread per node: walks the line's pieces in order, FUSE_PIECES of them
//                        staged in LDS at a time, and sums the contributions of the piece segments
//                        whose arc interval holds the node - a gather, so there is no atomic and no
//                        sort, and the sums run in the rule's order whatever the launch shape
// Everything is fp64 with FMA contraction off: one rounding per operation, as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_drive.hpp"        // DrvPose / drv_pose_kernel: the library's pose code

namespace prh {

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_TILE = 512;          // carrier segments per LDS round (FUSE_TILE + 1 vertices: 16.4 KB)
constexpr int FUSE_MAX_POINTS = 64;     // points per piece fuse_gather takes
constexpr int FUSE_PIECES = 32;         // pieces per LDS round of fuse_gather (32 * 64 * 8 B = 16 KB)

// w = R p + t: DrvPose keeps the inverse rotation (local = m * (p - t)), so R = m transposed
__device__ __forceinline__ void fuse_world(const DrvPose& ps, double px, double py, double pz, double& wx,
                                           double& wy, double& wz) {
#pragma clang fp contract(off)
  wx = ((ps.m[0] * px + ps.m[3] * py) + ps.m[6] * pz) + ps.t[0];
  wy = ((ps.m[1] * px + ps.m[4] * py) + ps.m[7] * pz) + ps.t[1];
  wz = ((ps.m[2] * px + ps.m[5] * py) + ps.m[8] * pz) + ps.t[2];
}

// pieces [n_pieces*M,3]; piece_pose [n_pieces] or NULL (the points are in the drive frame already);
// piece_line [n_pieces] or NULL (transform only: s, d, seg are not written).  verts [*,3] and cum [*]
// with CSR line_off [n_lines+1].  A block's points may belong to several lines: the block walks
// the lines between the lowest and the highest index it holds and skips those none of its points use.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_project_kernel(
    const double* __restrict__ pieces, long long n_points, int M, const int* __restrict__ piece_line,
    const int* __restrict__ piece_pose, const DrvPose* __restrict__ pose, int n_poses,
    const double* __restrict__ verts, const long long* __restrict__ line_off, const double* __restrict__ cum,
    int n_lines, double* __restrict__ world, double* __restrict__ s_out, double* __restrict__ d_out,
    int* __restrict__ seg_out) {
#pragma clang fp contract(off)
  __shared__ double tile[(FUSE_TILE + 1) * 4];        // x y z cum of FUSE_TILE + 1 consecutive vertices
  __shared__ int range[2];
  const int tid = threadIdx.x;
  const long long gid = (long long)blockIdx.x * FUSE_THREADS + tid;
  const bool live = gid < n_points;
  const long long piece = live ? gid / M : 0;
  double wx = 0.0, wy = 0.0, wz = 0.0;
  if (live) {
    const double px = pieces[3 * gid], py = pieces[3 * gid + 1], pz = pieces[3 * gid + 2];
    if (piece_pose) {
      const int q = piece_pose[piece];
      if (q >= 0 && q < n_poses) {
        fuse_world(pose[q], px, py, pz, wx, wy, wz);
      } else {
        wx = wy = wz = __longlong_as_double(0x7ff8000000000000ll);      // no such pose: NaN
      }
    } else {
      wx = px; wy = py; wz = pz;
    }
    world[3 * gid] = wx; world[3 * gid + 1] = wy; world[3 * gid + 2] = wz;
  }
  if (!piece_line) return;                             // the whole grid leaves together
  int line = live ? piece_line[piece] : -1;
  if (line < 0 || line >= n_lines) line = -1;
  if (tid == 0) { range[0] = n_lines; range[1] = -1; }
  __syncthreads();
  if (line >= 0) { atomicMin(&range[0], line); atomicMax(&range[1], line); }
  __syncthreads();
  const int lo = range[0], hi = range[1];
  double best = __longlong_as_double(0x7ff0000000000000ll), best_u = 0.0;      // +inf
  long long best_k = -1;
  for (int l = lo; l <= hi; ++l) {
    const bool mine = line == l;
    if (!__syncthreads_or(mine)) continue;
    const long long v0 = line_off[l], n_seg = line_off[l + 1] - v0 - 1;
    for (long long k0 = 0; k0 < n_seg; k0 += FUSE_TILE) {
      const int cnt = (int)(n_seg - k0 < FUSE_TILE ? n_seg - k0 : FUSE_TILE);
      for (int i = tid; i <= cnt; i += FUSE_THREADS) {
        const long long v = v0 + k0 + i;
        tile[4 * i] = verts[3 * v]; tile[4 * i + 1] = verts[3 * v + 1]; tile[4 * i + 2] = verts[3 * v + 2];
        tile[4 * i + 3] = cum[v];
      }
      __syncthreads();
      if (mine) {
        double ax = tile[0], ay = tile[1], az = tile[2];
        for (int k = 0; k < cnt; ++k) {
          const double bx = tile[4 * k + 4], by = tile[4 * k + 5], bz = tile[4 * k + 6];
          const double ex = bx - ax, ey = by - ay, ez = bz - az;
          const double l2 = (ex * ex + ey * ey) + ez * ez;
          if (l2 > 0.0) {
            const double gx = wx - ax, gy = wy - ay, gz = wz - az;
            const double dot = (gx * ex + gy * ey) + gz * ez;
            // clamp(dot / l2, 0, 1) without the division where the clamp decides: dot / l2 rounds
            // to a value in (0, 1) exactly when 0 < dot < l2
            double u;
            if (dot <= 0.0) u = 0.0;
            else if (dot >= l2) u = 1.0;
            else u = dot / l2;
            const double cx = ax + u * ex, cy = ay + u * ey, cz = az + u * ez;
            const double hx = wx - cx, hy = wy - cy, hz = wz - cz;
            const double d2 = (hx * hx + hy * hy) + hz * hz;
            if (d2 < best) { best = d2; best_u = u; best_k = k0 + k; }
          }
          ax = bx; ay = by; az = bz;
        }
      }
      __syncthreads();
    }
  }
  if (!live) return;
  double s = 0.0, d = 0.0;
  if (best_k >= 0) {
    const long long v0 = line_off[line];
    const double c0 = cum[v0 + best_k], c1 = cum[v0 + best_k + 1];
    s = c0 + best_u * (c1 - c0);
    d = sqrt(best);
  } else if (line >= 0 && line_off[line + 1] > line_off[line]) {
    const double* v = verts + 3 * line_off[line];
    const double hx = wx - v[0], hy = wy - v[1], hz = wz - v[2];
    d = sqrt((hx * hx + hy * hy) + hz * hz);
  }
  s_out[gid] = s; d_out[gid] = d; seg_out[gid] = (int)best_k;
}

// range [n_pieces,2] = min and max of the piece's M values of s
__global__ __launch_bounds__(FUSE_THREADS) void fuse_range_kernel(const double* __restrict__ s, long long n_pieces,
                                                                  int M, double* __restrict__ range) {
  const long long p = (long long)blockIdx.x * FUSE_THREADS + threadIdx.x;
  if (p >= n_pieces) return;
  const double* v = s + p * M;
  double lo = v[0], hi = v[0];
  for (int i = 1; i < M; ++i) { lo = fmin(lo, v[i]); hi = fmax(hi, v[i]); }
  range[2 * p] = lo; range[2 * p + 1] = hi;
}

// the largest l with off[l] <= i, for a non-decreasing off [n+1] with off[0] <= i < off[n]
__device__ __forceinline__ int fuse_owner(const long long* __restrict__ off, int n, long long i) {
  int lo = 0, hi = n;                  // invariant: off[lo] <= i < off[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// Nodes are numbered line after line (node_off [n_lines+1]); node j of a line sits at arc position
// (double)j * ds.  Pieces are grouped by line (line_piece_off [n_lines+1]) in the caller's order.
// world [n_pieces*M,3], s [n_pieces*M], range from fuse_range_kernel.
// Out: X [n_nodes,3], W, spread [n_nodes], C [n_nodes]; a node without a contribution gets zeros.
__global__ __launch_bounds__(FUSE_THREADS) void fuse_gather_kernel(
    const double* __restrict__ world, const double* __restrict__ s, const double* __restrict__ range, int M,
    const long long* __restrict__ line_piece_off, int n_lines, const long long* __restrict__ node_off,
    long long n_nodes, double ds, double* __restrict__ X, double* __restrict__ W, int* __restrict__ C,
    double* __restrict__ spread) {
#pragma clang fp contract(off)
  __shared__ double sh_s[FUSE_PIECES * FUSE_MAX_POINTS];
  __shared__ double sh_range[FUSE_PIECES * 2];
  const int tid = threadIdx.x;
  const long long n0 = (long long)blockIdx.x * FUSE_THREADS;
  const long long n1 = n0 + FUSE_THREADS < n_nodes ? n0 + FUSE_THREADS : n_nodes;      // n0 < n1 by the grid
  const long long node = n0 + tid;
  const bool live = node < n1;
  const int l_first = fuse_owner(node_off, n_lines, n0), l_last = fuse_owner(node_off, n_lines, n1 - 1);
  const int line = live ? fuse_owner(node_off, n_lines, node) : -1;
  const double pos = live ? (double)(node - node_off[line]) * ds : 0.0;
  int cnt = 0;
  double w_sum = 0.0, ax = 0.0, ay = 0.0, az = 0.0, mx = 0.0, my = 0.0, mz = 0.0, var = 0.0;
  for (int sweep = 0; sweep < 2; ++sweep) {
    if (sweep == 1) {
      if (cnt > 0) { mx = ax / w_sum; my = ay / w_sum; mz = az / w_sum; }
      if (!__syncthreads_or(cnt > 0)) break;
    }
    for (int l = l_first; l <= l_last; ++l) {
      const bool mine = line == l;
      const long long p0 = line_piece_off[l], p1 = line_piece_off[l + 1];
      for (long long t0 = p0; t0 < p1; t0 += FUSE_PIECES) {
        const int np = (int)(p1 - t0 < FUSE_PIECES ? p1 - t0 : FUSE_PIECES);
        for (int i = tid; i < np * M; i += FUSE_THREADS) sh_s[i] = s[t0 * M + i];
        for (int i = tid; i < np * 2; i += FUSE_THREADS) sh_range[i] = range[t0 * 2 + i];
        __syncthreads();
        if (mine && (sweep == 0 || cnt > 0)) {
          for (int q = 0; q < np; ++q) {
            if (!(sh_range[2 * q] <= pos && pos < sh_range[2 * q + 1])) continue;
            const double* sq = sh_s + q * M;
            const double* wq = world + (t0 + q) * M * 3;
            for (int i = 0; i + 1 < M; ++i) {
              const double sa = sq[i], sb = sq[i + 1];
              if (!(sb > sa && sa <= pos && pos < sb)) continue;
              const double u = (pos - sa) / (sb - sa);
              const double ta = (double)(i + 1 < M - i ? i + 1 : M - i);
              const double tb = (double)(i + 2 < M - i - 1 ? i + 2 : M - i - 1);
              const double om = ta + u * (tb - ta);
              const double* a = wq + 3 * i;
              const double x = a[0] + u * (a[3] - a[0]), y = a[1] + u * (a[4] - a[1]), z = a[2] + u * (a[5] - a[2]);
              if (sweep == 0) {
                ++cnt;
                w_sum = w_sum + om;
                ax = ax + om * x; ay = ay + om * y; az = az + om * z;
              } else {
                const double hx = x - mx, hy = y - my, hz = z - mz;
                var = var + om * ((hx * hx + hy * hy) + hz * hz);
              }
            }
          }
        }
        __syncthreads();
      }
    }
  }
  if (!live) return;
  X[3 * node] = mx; X[3 * node + 1] = my; X[3 * node + 2] = mz;
  W[node] = w_sum; C[node] = cnt;
  spread[node] = cnt > 0 ? sqrt(var / w_sum) : 0.0;
}

}  // namespace prh
