// Cloud support on the GPU: what the merged cloud holds in the tube around every station of every
// map polyline - how many points, how bright, on which side, how high.  The rule is written out in
// include/pointnet_refine_hip.h ("Cloud support - the rule"); tests/_support_oracle.py restates it.
//   support_kernel   one thread per cloud point, one 16-byte load.  The host laid a uniform xy grid
//                    over the lines and listed, per cell, the (line, segment) pairs whose
//                    radius-expanded box overlaps the cell, sorted by line, then by segment.  A
//                    thread finds its cell, leaves when it is outside the grid or the cell is empty,
//                    walks the cell's list keeping the best segment per line and flushes a hit when
//                    the line changes.  Every segment within the radius of a point is in the point's
//                    list, so the first strictly smallest d2 of the list is the rule's minimum over
//                    all segments whenever the point is a hit.
// Hits are accumulated in fixed point with 64-bit integer atomics: the sums are integers, so they
// do not depend on the order of arrival and the result is bitwise reproducible.
// The geometry is fp64 with FMA contraction off: one rounding per operation, as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prh {

constexpr int SUPPORT_THREADS = 256;
constexpr int SUPPORT_COLS = 8;          // int64 columns of a node row: 64 bytes

struct SupportGrid {
  double x0, y0, cell;                   // cell index = floor((x - x0) / cell), the host's expression
  int nx, ny;
};

// one hit of point w on segment k = (a, a + e) of line `line`, with the projection's u and hz
__device__ __forceinline__ void support_flush(
    int line, long long k, double u, double hz, double wx, double wy, double intensity,
    const double* __restrict__ verts, const long long* __restrict__ line_off, const double* __restrict__ cum,
    const long long* __restrict__ node_off, double step, double intensity_floor, unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
  const long long v = line_off[line] + k;
  const double ax = verts[3 * v], ay = verts[3 * v + 1];
  const double ex = verts[3 * v + 3] - ax, ey = verts[3 * v + 4] - ay;
  const double c0 = cum[v], c1 = cum[v + 1];
  const double s = c0 + u * (c1 - c0);
  const long long n_nodes = node_off[line + 1] - node_off[line];
  long long j = (long long)floor(s / step + 0.5);
  if (j > n_nodes - 1) j = n_nodes - 1;
  if (j < 0) return;                     // a line without nodes: cannot happen with the host's offsets
  const double gx = wx - ax, gy = wy - ay;
  const double exy2 = ex * ex + ey * ey;
  const double t = exy2 > 0.0 ? (ex * gy - ey * gx) / sqrt(exy2) : 0.0;
  const double wi = fmin(fmax(intensity - intensity_floor, 0.0), 4096.0);
  const long long qi = (long long)rint(wi * 256.0);
  const long long qt = (long long)rint(t * 65536.0);
  const long long qz = (long long)rint(hz * 65536.0);
  unsigned long long* row = acc + (node_off[line] + j) * SUPPORT_COLS;
  atomicAdd(row + 0, 1ull);
  if (qi > 0) {
    atomicAdd(row + 1, 1ull);
    atomicAdd(row + 2, (unsigned long long)qi);
    atomicAdd(row + 5, (unsigned long long)(qi * qt));
  }
  if (qt != 0) {
    atomicAdd(row + 3, (unsigned long long)qt);
    atomicAdd(row + 4, (unsigned long long)(qt * qt));
  }
  if (qz != 0) atomicAdd(row + 6, (unsigned long long)qz);
}

// cloud [n_points] of x y z intensity; cell_off [nx*ny+1] and entries [*] = (line, segment) from
// the host's grid; verts [*,3] and cum [*] with CSR line_off [n_lines+1]; node_off [n_lines+1];
// acc [n_nodes,8] zeroed by the caller.
__global__ __launch_bounds__(SUPPORT_THREADS) void support_kernel(
    const float4* __restrict__ cloud, long long n_points, double ox, double oy, double oz, SupportGrid grid,
    const int* __restrict__ cell_off, const int2* __restrict__ entries, const double* __restrict__ verts,
    const long long* __restrict__ line_off, const double* __restrict__ cum, const long long* __restrict__ node_off,
    int n_lines, double step, double r2, double intensity_floor, unsigned long long* __restrict__ acc) {
#pragma clang fp contract(off)
  const long long gid = (long long)blockIdx.x * SUPPORT_THREADS + threadIdx.x;
  if (gid >= n_points) return;
  const float4 p = cloud[gid];
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w))) return;
  const double wx = (double)p.x - ox, wy = (double)p.y - oy, wz = (double)p.z - oz;
  const double fx = floor((wx - grid.x0) / grid.cell), fy = floor((wy - grid.y0) / grid.cell);
  if (!(fx >= 0.0 && fx < (double)grid.nx && fy >= 0.0 && fy < (double)grid.ny)) return;
  const long long cell = (long long)fy * grid.nx + (long long)fx;
  const int e0 = cell_off[cell], e1 = cell_off[cell + 1];
  if (e0 == e1) return;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  int line = -1;
  double best = inf, best_u = 0.0, best_hz = 0.0;
  long long best_k = -1;
  for (int i = e0; i < e1; ++i) {
    const int2 en = entries[i];
    if (en.x < 0 || en.x >= n_lines || en.y < 0 || line_off[en.x] + en.y + 1 >= line_off[en.x + 1]) continue;
    if (en.x != line) {
      if (best_k >= 0 && best <= r2)
        support_flush(line, best_k, best_u, best_hz, wx, wy, (double)p.w, verts, line_off, cum, node_off, step,
                      intensity_floor, acc);
      line = en.x; best = inf; best_k = -1;
    }
    const double* a = verts + 3 * (line_off[line] + en.y);
    const double ax = a[0], ay = a[1], az = a[2];
    const double ex = a[3] - ax, ey = a[4] - ay, ez = a[5] - az;
    const double l2 = (ex * ex + ey * ey) + ez * ez;
    if (!(l2 > 0.0)) continue;
    const double gx = wx - ax, gy = wy - ay, gz = wz - az;
    const double dot = (gx * ex + gy * ey) + gz * ez;
    // clamp(dot / l2, 0, 1) without the division where the clamp decides (as fuse_project_kernel)
    double u;
    if (dot <= 0.0) u = 0.0;
    else if (dot >= l2) u = 1.0;
    else u = dot / l2;
    const double hx = wx - (ax + u * ex), hy = wy - (ay + u * ey), hz = wz - (az + u * ez);
    const double d2 = (hx * hx + hy * hy) + hz * hz;
    if (d2 < best) { best = d2; best_u = u; best_hz = hz; best_k = en.y; }
  }
  if (best_k >= 0 && best <= r2)
    support_flush(line, best_k, best_u, best_hz, wx, wy, (double)p.w, verts, line_off, cum, node_off, step,
                  intensity_floor, acc);
}

}  // namespace prh
