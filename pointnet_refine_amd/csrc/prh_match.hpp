// Prediction scenes on the GPU: the per-frame work of the reference's tools/generate_inference_data_vma.py
// (:265-315 clipping, :400-402 the keep rule, :434-448 cost matrices, :451-459 the assignment),
// which the reference does with a Python double loop and one scipy call per frame.
//   mt_clip_kernel      one thread per (frame, GT polyline): ego transform (drv_local), the "some
//                       vertex strictly inside the slab" gate and the two half-plane passes of
//                       clip_polygon_against_plane chained in registers (pass 2 consumes what pass 1
//                       emits, vertex by vertex; nothing is buffered)
//   mt_line_frame_kernel  prediction line -> frame map for the cost kernel
//   mt_cost_kernel      one workgroup per prediction line, a wave per GT line of its frame, lanes
//                       over prediction vertices: min of the squared xy distance over the GT line's
//                       vertices (wave-uniform reads), sqrt once per prediction vertex, per-lane sums
//                       in vertex order, then the butterfly wave sum
//   mt_assign_kernel    one wave64 per frame: shortest augmenting paths with row / column
//                       potentials (the Jonker-Volgenant form of the Hungarian method).  The matrix
//                       sits in LDS with rows <= columns (transposed while staging when P > G),
//                       lanes own columns, the minimum reduced cost over unvisited columns is one
//                       wave-wide (value, index) min with the lowest index winning ties.
// Every loop of the solver is bounded by the row / column counts; a frame with a non-finite cost
// never enters it (status MT_INVALID).  No atomics anywhere: outputs are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_drive.hpp"        // DrvPose, drv_local
#include "prh_metrics.hpp"      // met_wave_sum, met_wave_argmin

namespace prh {

constexpr int MT_MAX_SIDE = 128;                 // lines per side per frame the solver takes
constexpr int MT_COLS_PER_LANE = MT_MAX_SIDE / 64;
constexpr int MT_COST_THREADS = 256;
constexpr int MT_OK = 0, MT_INVALID = 1, MT_TOO_LARGE = 2;     // per-frame status words

// dynamic LDS of mt_assign_kernel for a launch whose largest frame has max_cells = P * G entries
inline size_t mt_assign_lds(long max_cells) {
  return (size_t)max_cells * sizeof(double) + (size_t)(MT_MAX_SIDE + 2) * (sizeof(double) + 2 * sizeof(int));
}

// pass 2 of clip_polyline_by_x (x <= x_max) fed one vertex at a time
struct MtClipOut {
  double px, py, pz;     // previous vertex pass 2 saw
  int seen, k;           // vertices pass 2 saw / emitted
  double* o;             // output or nullptr
};
__device__ __forceinline__ void mt_emit(MtClipOut& s, double x, double y, double z) {
  if (s.o) { s.o[3 * s.k] = x; s.o[3 * s.k + 1] = y; s.o[3 * s.k + 2] = z; }
  ++s.k;
}
// the reference's intersection(a, b): a itself when |b.x - a.x| < 1e-6
__device__ __forceinline__ void mt_cross(double ax, double ay, double az, double bx, double by, double bz,
                                         double plane, double& x, double& y, double& z) {
#pragma clang fp contract(off)
  const double denom = bx - ax;
  if (fabs(denom) < 1e-6) { x = ax; y = ay; z = az; return; }
  const double t = (plane - ax) / denom;
  x = ax + t * (bx - ax); y = ay + t * (by - ay); z = az + t * (bz - az);
}
__device__ __forceinline__ void mt_push2(MtClipOut& s, double x, double y, double z, double x_max) {
  const bool in2 = x <= x_max;
  if (s.seen == 0) {
    if (in2) mt_emit(s, x, y, z);
  } else {
    const bool in1 = s.px <= x_max;
    if (in1 && in2) {
      mt_emit(s, x, y, z);
    } else if (in1 != in2) {
      double ix, iy, iz;
      mt_cross(s.px, s.py, s.pz, x, y, z, x_max, ix, iy, iz);
      mt_emit(s, ix, iy, iz);
      if (in2) mt_emit(s, x, y, z);
    }
  }
  s.px = x; s.py = y; s.pz = z;
  ++s.seen;
}

// verts [*,3] with CSR line_off [NL+1]; counts [F*NL]: vertices clip_polyline_by_x leaves of line l
// in frame f, 0 when no vertex has -half < x < half; WRITE: vertices to out + 3 * out_off[f*NL + l]
template <bool WRITE>
__global__ __launch_bounds__(256) void mt_clip_kernel(const double* __restrict__ verts,
                                                      const long long* __restrict__ line_off, int NL,
                                                      const DrvPose* __restrict__ pose, int F, double half,
                                                      int* __restrict__ counts,
                                                      const long long* __restrict__ out_off,
                                                      double* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)F * NL) return;
  const int f = (int)(i / NL), l = (int)(i % NL);
  const DrvPose ps = pose[f];
  const long long n = line_off[l + 1] - line_off[l];
  const double* v = verts + 3 * line_off[l];
  const double x_min = -half, x_max = half;
  if (WRITE && out_off[i + 1] == out_off[i]) return;          // gated out or empty: nothing to write
  bool any = false;
  if (!WRITE) {
    for (long long q = 0; q < n; ++q) {
      double x, y, z;
      drv_local(ps, v[3 * q], v[3 * q + 1], v[3 * q + 2], x, y, z);
      any = any || (x > x_min && x < x_max);
    }
    if (!any) { counts[i] = 0; return; }
  }
  MtClipOut s;
  s.px = s.py = s.pz = 0.0; s.seen = 0; s.k = 0;
  s.o = WRITE ? out + 3 * out_off[i] : nullptr;
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (long long q = 0; q < n; ++q) {
    double bx, by, bz;
    drv_local(ps, v[3 * q], v[3 * q + 1], v[3 * q + 2], bx, by, bz);
    const bool in2 = bx >= x_min;
    if (q == 0) {
      if (in2) mt_push2(s, bx, by, bz, x_max);
    } else {
      const bool in1 = ax >= x_min;
      if (in1 && in2) {
        mt_push2(s, bx, by, bz, x_max);
      } else if (in1 != in2) {
        double ix, iy, iz;
        mt_cross(ax, ay, az, bx, by, bz, x_min, ix, iy, iz);
        mt_push2(s, ix, iy, iz, x_max);
        if (in2) mt_push2(s, bx, by, bz, x_max);
      }
    }
    ax = bx; ay = by; az = bz;
  }
  if (!WRITE) counts[i] = s.k;
}

// line_frame [n_lines]: the frame of each line, from the frames' CSR over lines
__global__ __launch_bounds__(256) void mt_line_frame_kernel(const long long* __restrict__ frame_off, int F,
                                                            int* __restrict__ line_frame) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  for (long long l = frame_off[f]; l < frame_off[f + 1]; ++l) line_frame[l] = f;
}

// cost[i,j] = mean_p min_g |pred_i[p].xy - gt_j[g].xy| for prediction line blockIdx.x (= i of its
// frame f) and every GT line j of f.  pred_xy / gt_xy [*,2]; *_line_off: vertex CSR over lines;
// *_frame_off: line CSR over frames; costs + cost_off[f]: the frame's (P_f, G_f) matrix, row major.
// A line without vertices gives NaN (0 / 0) for a prediction and +inf for a GT line.
__global__ __launch_bounds__(MT_COST_THREADS) void mt_cost_kernel(
    const double* __restrict__ pred_xy, const long long* __restrict__ pred_line_off,
    const long long* __restrict__ pred_frame_off, const int* __restrict__ pred_line_frame,
    const double* __restrict__ gt_xy, const long long* __restrict__ gt_line_off,
    const long long* __restrict__ gt_frame_off, const long long* __restrict__ cost_off,
    double* __restrict__ costs) {
#pragma clang fp contract(off)
  const long long line = blockIdx.x;
  const int f = pred_line_frame[line];
  const long long g0 = gt_frame_off[f], G = gt_frame_off[f + 1] - g0;
  const long long i = line - pred_frame_off[f];
  const long long p0 = pred_line_off[line], np = pred_line_off[line + 1] - p0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* row = costs + cost_off[f] + i * G;
  for (long long j = wave; j < G; j += MT_COST_THREADS / 64) {
    const long long a = gt_line_off[g0 + j], b = gt_line_off[g0 + j + 1];
    double acc = 0.0;
    for (long long p = lane; p < np; p += 64) {
      const double2 pv = reinterpret_cast<const double2*>(pred_xy)[p0 + p];
      double best = INFINITY;
      for (long long g = a; g < b; ++g) {
        const double2 gv = reinterpret_cast<const double2*>(gt_xy)[g];
        const double dx = pv.x - gv.x, dy = pv.y - gv.y;
        best = fmin(best, dx * dx + dy * dy);
      }
      acc += sqrt(best);
    }
    acc = met_wave_sum(acc);
    if (lane == 0) row[j] = acc / (double)np;
  }
}

// One wave64 per frame f: minimum-cost assignment of the (P, G) = shapes[f] matrix at costs +
// cost_off[f].  match + row_off[f] [P]: the GT column of each prediction or -1 (also -1 when
// use_threshold and the pair's cost is not < threshold); total[f]: the optimal sum before the
// threshold; status[f]: MT_OK / MT_INVALID (a non-finite cost: all -1, total NaN) / MT_TOO_LARGE
// (a side above MT_MAX_SIDE or P * G above max_cells); row_dual + row_off[f] [P], col_dual +
// col_off[f] [G] (both may be NULL): potentials with cost[i,j] - row_dual[i] - col_dual[j] >= 0
// everywhere and = 0 on the assigned pairs.
// LDS: c [nr*nc] (rows <= columns), u [nr+1], col_row [nc+1], way [nc+1]; rows and columns are
// 1-based inside, column 0 being the virtual start of every path.  Lane l owns columns l+1, l+65.
__global__ __launch_bounds__(64) void mt_assign_kernel(const double* __restrict__ costs,
                                                       const long long* __restrict__ cost_off,
                                                       const int* __restrict__ shapes,
                                                       const long long* __restrict__ row_off,
                                                       const long long* __restrict__ col_off, long long max_cells,
                                                       double threshold, int use_threshold,
                                                       int* __restrict__ match, double* __restrict__ total,
                                                       int* __restrict__ status, double* __restrict__ row_dual,
                                                       double* __restrict__ col_dual) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char mt_lds[];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int P = shapes[2 * f], G = shapes[2 * f + 1];
  int* m_out = match + row_off[f];
  double* rd = row_dual ? row_dual + row_off[f] : nullptr;
  double* cd = col_dual ? col_dual + col_off[f] : nullptr;
  // every way out that is not a solution: no match, zero potentials
  auto leave = [&](int st, double tot) {
    for (int r = lane; r < P; r += 64) { m_out[r] = -1; if (rd) rd[r] = 0.0; }
    for (int g = lane; g < G; g += 64) if (cd) cd[g] = 0.0;
    if (lane == 0) { total[f] = tot; status[f] = st; }
  };
  if (P <= 0 || G <= 0) { leave(MT_OK, 0.0); return; }
  if (P > MT_MAX_SIDE || G > MT_MAX_SIDE || (long long)P * G > max_cells) { leave(MT_TOO_LARGE, NAN); return; }
  const bool tr = P > G;                       // rows <= columns, as scipy transposes
  const int nr = tr ? G : P, nc = tr ? P : G;
  double* c = reinterpret_cast<double*>(mt_lds);
  double* u = c + max_cells;
  int* col_row = reinterpret_cast<int*>(u + MT_MAX_SIDE + 2);
  int* way = col_row + MT_MAX_SIDE + 2;
  const double* src = costs + cost_off[f];
  bool bad = false;
  for (int e = lane; e < P * G; e += 64) {
    const double val = src[e];
    bad = bad || !isfinite(val);
    const int pi = e / G, gi = e - pi * G;
    c[tr ? gi * nc + pi : e] = val;
  }
  for (int r = lane; r <= nr; r += 64) u[r] = 0.0;
  for (int j = lane; j <= nc; j += 64) { col_row[j] = 0; way[j] = 0; }
  if (__ballot(bad) != 0ull) { leave(MT_INVALID, NAN); return; }     // wave-uniform: the whole wave leaves
  __syncthreads();
  double v[MT_COLS_PER_LANE], minv[MT_COLS_PER_LANE];
  bool used[MT_COLS_PER_LANE];
#pragma unroll
  for (int k = 0; k < MT_COLS_PER_LANE; ++k) v[k] = 0.0;
  bool broken = false;
  for (int i = 1; i <= nr && !broken; ++i) {
    if (lane == 0) col_row[0] = i;
#pragma unroll
    for (int k = 0; k < MT_COLS_PER_LANE; ++k) { minv[k] = INFINITY; used[k] = false; }
    __syncthreads();
    int j0 = 0;
    // a path visits the virtual column and at most i - 1 assigned columns before a free one
    for (int step = 0; step < i; ++step) {
      const int i0 = col_row[j0];
      const double ui0 = u[i0];
      const double* crow = c + (i0 - 1) * nc;
      double delta = INFINITY;
      int j1 = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < MT_COLS_PER_LANE; ++k) {
        const int j = 1 + lane + 64 * k;
        if (j == j0) used[k] = true;
        if (j <= nc && !used[k]) {
          const double cur = (crow[j - 1] - ui0) - v[k];
          if (cur < minv[k]) { minv[k] = cur; way[j] = j0; }
          if (minv[k] < delta) { delta = minv[k]; j1 = j; }     // k ascending: the lower column on a tie
        }
      }
      met_wave_argmin(delta, j1);
      delta = __shfl(delta, 0); j1 = __shfl(j1, 0);             // one copy (+0 and -0 compare equal)
      if (!(delta < INFINITY) || j1 > nc) { broken = true; break; }     // only overflowed potentials get here
      if (lane == 0) u[i] += delta;            // the virtual column carries row i
#pragma unroll
      for (int k = 0; k < MT_COLS_PER_LANE; ++k) {
        const int j = 1 + lane + 64 * k;
        if (j <= nc) {
          if (used[k]) { u[col_row[j]] += delta; v[k] -= delta; }
          else minv[k] -= delta;
        }
      }
      __syncthreads();
      j0 = j1;
      if (col_row[j0] == 0) break;             // a free column: the path is complete
    }
    if (broken || col_row[j0] != 0) { broken = true; break; }
    __syncthreads();
    if (lane == 0) {
      for (int step = 0; step <= nc && j0 != 0; ++step) {       // flip the path back to the virtual column
        const int j1 = way[j0];
        col_row[j0] = col_row[j1];
        j0 = j1;
      }
    }
    __syncthreads();
  }
  if (broken) { leave(MT_INVALID, NAN); return; }
  // the sum in column order, one lane: the same bits every run
  if (lane == 0) {
    double sum = 0.0;
    for (int j = 1; j <= nc; ++j)
      if (col_row[j] > 0) sum += c[(col_row[j] - 1) * nc + (j - 1)];
    total[f] = sum;
    status[f] = MT_OK;
  }
  for (int r = lane; r <= nr; r += 64) way[r] = 0;               // from here: the column of each row, 1-based
  __syncthreads();
#pragma unroll
  for (int k = 0; k < MT_COLS_PER_LANE; ++k) {
    const int j = 1 + lane + 64 * k;
    if (j > nc) continue;
    const int r = col_row[j];
    const bool keep = r > 0 && (!use_threshold || c[(r - 1) * nc + (j - 1)] < threshold);
    if (tr) {
      m_out[j - 1] = keep ? r - 1 : -1;
      if (rd) rd[j - 1] = v[k];
    } else {
      if (keep) way[r] = j;
      if (cd) cd[j - 1] = v[k];
    }
  }
  __syncthreads();
  for (int r = lane; r < nr; r += 64) {
    if (tr) {
      if (cd) cd[r] = u[r + 1];
    } else {
      m_out[r] = way[r + 1] - 1;
      if (rd) rd[r] = u[r + 1];
    }
  }
}

}  // namespace prh
