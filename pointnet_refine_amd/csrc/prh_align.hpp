// Paint alignment on the GPU: for every (slice, xy shift) how much bright cloud lies on the slice's
// detector lines once they are moved by the shift.  The rule is written out in
// include/pointnet_refine_hip.h ("Paint alignment - the rule"); tests/_align_oracle.py restates it.
//   align_select_kernel<WRITE=false>  one thread per point: one aligned load, step 1 (finite x y z,
//                    qi > 0), the slice of the point, one lookup in that slice's cell bitmap (the
//                    host set every cell the reach-expanded box of a segment touches).  Survivors
//                    are counted per slice: one integer atomic per wave where the wave's survivors
//                    share a slice (ballot / popcount), one per lane where they do not.
//   align_select_kernel<WRITE=true>   the same walk; a survivor's record (x y z fp64, qi int64) goes
//                    to records[cand_offsets[s] + cursor[s]++], the cursor advanced per wave.  The
//                    order inside a slice is the order of arrival: the rule does not see it.
//   align_score_kernel   one block per work item (slice, 256 candidates, 16 shifts).  A thread holds
//                    one candidate and its 16 shifted xy in registers.  The slice's vertices go
//                    through LDS ALIGN_TILE at a time, each slot holding the segment that starts at
//                    that vertex (a, b, L2, line id; L2 = 0 where the line ends there).  d2min per
//                    shift is carried across tiles and flushed when the line id changes or the list
//                    ends.  Per shift: integer wave reduction, LDS, one 64-bit integer atomicAdd per
//                    (block, shift, column).  align_score_kernel<RIGID=true> is the same kernel
//                    for "Rigid paint alignment - the rule": the table's rows are dx dy c s, the
//                    slice has a pivot, and the 16 (wx, wy) come from the inverse pose; the
//                    segment loop does not know the difference.
//   align_select_cells_kernel<WRITE>  the select walk with one counter per bitmap cell instead of
//                    one per slice: count, the caller's scan, write with a per-cell cursor.  A
//                    slice's survivors then lie in ascending cell order (arrival order inside a
//                    cell), so a wave of the score kernel holds neighbours on the road.
// Every accumulated quantity is an integer, so no output depends on the order of the candidates,
// on the filter, on the tiles or on the launch shape.  The geometry is fp64 with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_bev.hpp"          // bev_slice_of: the slice of a flat row

namespace prh {

constexpr int ALIGN_THREADS = 256;       // points per select block, candidates per work item
constexpr int ALIGN_WAVES = ALIGN_THREADS / 64;
constexpr int ALIGN_SHIFTS = 16;         // shifts per work item
constexpr int ALIGN_TILE = 512;          // vertex slots per LDS round (8 doubles each: 32 KB)
constexpr int ALIGN_MAX_SHIFTS = 4096;   // shifts per slice
constexpr int ALIGN_MAX_POSES = 32768;   // pose rows per slice

struct AlignRecord { double x, y, z; long long qi; };      // 32 bytes, 16-byte aligned

template <typename T> struct AlignPoint;
template <> struct AlignPoint<double> {
  static __device__ __forceinline__ void load(const double* p, double& x, double& y, double& z, double& w) {
    const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
    x = a.x; y = a.y; z = b.x; w = b.y;
  }
};
template <> struct AlignPoint<float> {
  static __device__ __forceinline__ void load(const float* p, double& x, double& y, double& z, double& w) {
    const float4 a = reinterpret_cast<const float4*>(p)[0];
    x = (double)a.x; y = (double)a.y; z = (double)a.z; w = (double)a.w;
  }
};

// step 1: the fixed-point intensity weight; 0 for a non-finite intensity
__device__ __forceinline__ long long align_qi(double intensity, double intensity_floor) {
#pragma clang fp contract(off)
  if (!isfinite(intensity)) return 0;
  const double wi = fmin(fmax(intensity - intensity_floor, 0.0), 4096.0);
  return (long long)rint(wi * 256.0);
}

// steps 1 of the rule and the bitmap lookup for flat row i: true for a survivor, with its slice s,
// its cell c (global, < n_cells), x y z and qi
template <typename T>
__device__ __forceinline__ bool align_select_test(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long n, long long i,
    const double* __restrict__ origin, const int* __restrict__ shape, const long long* __restrict__ cell_base,
    const unsigned* __restrict__ bitmap, long long n_cells, double cell, double intensity_floor, int& s, long long& c,
    double& x, double& y, double& z, long long& qi) {
#pragma clang fp contract(off)
  if (i >= n) return false;
  double w;
  AlignPoint<T>::load(pts + 4 * i, x, y, z, w);
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  qi = align_qi(w, intensity_floor);
  if (qi <= 0) return false;
  s = bev_slice_of(slice_off, S, i);
  const int nx = shape[2 * s], ny = shape[2 * s + 1];
  const double fx = floor((x - origin[2 * s]) / cell), fy = floor((y - origin[2 * s + 1]) / cell);
  if (!(fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny)) return false;
  c = cell_base[s] + (long long)fy * nx + (long long)fx;
  if (c < 0 || c >= n_cells) return false;
  return (bitmap[c >> 5] >> (unsigned)(c & 31)) & 1u;
}

// grid of slice s: origin[2s], origin[2s+1] = x0 y0, shape[2s], shape[2s+1] = nx ny, cell
// cell_base[s] + iy * nx + ix is bit (c & 31) of bitmap[c >> 5].  counter [S]: the counts, or the cursors.
template <typename T, bool WRITE>
__global__ __launch_bounds__(ALIGN_THREADS) void align_select_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long n,
    const double* __restrict__ origin, const int* __restrict__ shape, const long long* __restrict__ cell_base,
    const unsigned* __restrict__ bitmap, long long n_cells, double cell, double intensity_floor,
    int* __restrict__ counter, const long long* __restrict__ cand_off, AlignRecord* __restrict__ rec,
    long long capacity) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * ALIGN_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int s = 0;
  long long c = 0, qi = 0;
  double x = 0.0, y = 0.0, z = 0.0;
  const bool keep = align_select_test<T>(pts, slice_off, S, n, i, origin, shape, cell_base, bitmap, n_cells, cell,
                                         intensity_floor, s, c, x, y, z, qi);
  const unsigned long long m = __ballot(keep);
  if (m == 0ull) return;                                 // wave-uniform
  const int lead = __ffsll((long long)m) - 1;
  const int s_lead = __shfl(s, lead);
  const bool uniform = __ballot(keep && s != s_lead) == 0ull;
  int k = 0;
  if (uniform) {
    int base = 0;
    if (lane == lead) base = atomicAdd(counter + s_lead, __popcll(m));
    base = __shfl(base, lead);
    k = base + __popcll(m & ((1ull << lane) - 1ull));
  } else if (keep) {
    k = atomicAdd(counter + s, 1);
  }
  if (WRITE && keep) {
    const long long pos = cand_off[s] + k;
    if (pos < cand_off[s + 1] && pos < capacity) {
      double2* r = reinterpret_cast<double2*>(rec + pos);
      r[0] = make_double2(x, y);
      r[1] = make_double2(z, __longlong_as_double(qi));
    }
  }
}

// counter [n_cells]: the counts, or the cursors; cell_off [n_cells+1]: the exclusive prefix of the
// counts.  Cells of a slice are contiguous, so rows cell_off[cell_base[s]] .. are slice s's.
template <typename T, bool WRITE>
__global__ __launch_bounds__(ALIGN_THREADS) void align_select_cells_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long n,
    const double* __restrict__ origin, const int* __restrict__ shape, const long long* __restrict__ cell_base,
    const unsigned* __restrict__ bitmap, long long n_cells, double cell, double intensity_floor,
    int* __restrict__ counter, const long long* __restrict__ cell_off, AlignRecord* __restrict__ rec,
    long long capacity) {
  const long long i = (long long)blockIdx.x * ALIGN_THREADS + threadIdx.x;
  int s = 0;
  long long c = 0, qi = 0;
  double x = 0.0, y = 0.0, z = 0.0;
  if (!align_select_test<T>(pts, slice_off, S, n, i, origin, shape, cell_base, bitmap, n_cells, cell, intensity_floor, s,
                            c, x, y, z, qi))
    return;
  const int k = atomicAdd(counter + c, 1);
  if (WRITE) {
    const long long pos = cell_off[c] + k;
    if (pos < cell_off[c + 1] && pos < capacity) {
      double2* r = reinterpret_cast<double2*>(rec + pos);
      r[0] = make_double2(x, y);
      r[1] = make_double2(z, __longlong_as_double(qi));
    }
  }
}

// the line of vertex v among lines lo .. hi-1 (line_off[lo] <= v < line_off[hi]): the last whose first vertex is <= v
__device__ __forceinline__ int align_line_of(const long long* __restrict__ line_off, int lo, int hi, long long v) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (line_off[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// items [n_items,3] int64 = (slice, first candidate, first shift): the candidates are rows of rec,
// the shifts rows of shifts; the counts are what the slice has left, at most 256 and 16.
// acc [n_shifts,2] int64 = score, hits; added to.
// RIGID: shifts is the pose table [n_shifts,4] = dx dy c s and pivots [S,2] the slices' pivots; the
// point is moved by the inverse pose ("Rigid paint alignment - the rule", step 2), once, before the loop.
template <bool RIGID>
__global__ __launch_bounds__(ALIGN_THREADS) void align_score_kernel(
    const AlignRecord* __restrict__ rec, const long long* __restrict__ cand_off, long long n_cand,
    const double* __restrict__ verts, long long n_verts, const long long* __restrict__ line_off, int n_lines,
    const long long* __restrict__ slice_line_off, const double* __restrict__ shifts,
    const long long* __restrict__ shift_off, long long n_shifts, const double* __restrict__ reach, int S,
    const long long* __restrict__ items, double r2, unsigned long long* __restrict__ acc,
    const double* __restrict__ pivots) {
#pragma clang fp contract(off)
  __shared__ double tile[ALIGN_TILE * 8];                // ax ay az bx by bz L2 line
  __shared__ long long red[ALIGN_WAVES][ALIGN_SHIFTS][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long* item = items + 3 * (long long)blockIdx.x;
  const long long sl = item[0], c0 = item[1], k0 = item[2];
  // a plan that does not fit the offsets is refused block by block (block-uniform): cannot happen with the host's plan
  if (sl < 0 || sl >= S) return;
  const int s = (int)sl;
  const long long c_end = cand_off[s + 1], k_end = shift_off[s + 1];
  if (c0 < cand_off[s] || c0 >= c_end || c_end > n_cand || k0 < shift_off[s] || k0 >= k_end || k_end > n_shifts) return;
  const int l_lo = (int)slice_line_off[s], l_hi = (int)slice_line_off[s + 1];
  if (l_lo < 0 || l_hi > n_lines || l_lo >= l_hi) return;
  const long long v_lo = line_off[l_lo], v_hi = line_off[l_hi];
  if (v_lo < 0 || v_hi > n_verts || v_lo >= v_hi) return;
  const int nc = (int)(c_end - c0 < ALIGN_THREADS ? c_end - c0 : ALIGN_THREADS);
  const int nk = (int)(k_end - k0 < ALIGN_SHIFTS ? k_end - k0 : ALIGN_SHIFTS);
  const double rch = reach[s];
  const double inf = __longlong_as_double(0x7ff0000000000000ll);

  const bool live = tid < nc;
  double x = 0.0, y = 0.0, z = 0.0;
  long long qi = 0;
  if (live) {
    const double2* r = reinterpret_cast<const double2*>(rec + c0 + tid);
    const double2 a = r[0], b = r[1];
    x = a.x; y = a.y; z = b.x; qi = __double_as_longlong(b.y);
  }
  const double pvx = RIGID ? pivots[2 * s] : 0.0, pvy = RIGID ? pivots[2 * s + 1] : 0.0;
  double wx[ALIGN_SHIFTS], wy[ALIGN_SHIFTS], d2m[ALIGN_SHIFTS];
  long long score[ALIGN_SHIFTS];
  int hits[ALIGN_SHIFTS];
#pragma unroll
  for (int k = 0; k < ALIGN_SHIFTS; ++k) {
    const long long row = k0 + (k < nk ? k : 0);         // a short tile repeats its first shift; not stored
    if (RIGID) {
      const double2* pose = reinterpret_cast<const double2*>(shifts) + 2 * row;
      const double2 d = pose[0], cs = pose[1];
      const double gx = (x - d.x) - pvx, gy = (y - d.y) - pvy;
      wx[k] = (cs.x * gx + cs.y * gy) + pvx; wy[k] = (cs.x * gy - cs.y * gx) + pvy;
    } else {
      wx[k] = x - shifts[2 * row]; wy[k] = y - shifts[2 * row + 1];
    }
    d2m[k] = inf; score[k] = 0; hits[k] = 0;
  }

  int cur_line = -1;
  for (long long t0 = v_lo; t0 < v_hi; t0 += ALIGN_TILE) {
    const int cnt = (int)(v_hi - t0 < ALIGN_TILE ? v_hi - t0 : ALIGN_TILE);
    for (int i = tid; i < cnt; i += ALIGN_THREADS) {
      const long long v = t0 + i;
      const int line = align_line_of(line_off, l_lo, l_hi, v);
      const double ax = verts[3 * v], ay = verts[3 * v + 1], az = verts[3 * v + 2];
      double bx = ax, by = ay, bz = az, l2 = 0.0;
      if (v + 1 < line_off[line + 1]) {                  // the segment that starts at v; none at a line's last vertex
        bx = verts[3 * v + 3]; by = verts[3 * v + 4]; bz = verts[3 * v + 5];
        const double ex = bx - ax, ey = by - ay, ez = bz - az;
        l2 = (ex * ex + ey * ey) + ez * ez;
      }
      double* t = tile + 8 * i;
      t[0] = ax; t[1] = ay; t[2] = az; t[3] = bx; t[4] = by; t[5] = bz; t[6] = l2;
      t[7] = __longlong_as_double((long long)line);
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const double* t = tile + 8 * j;
      const int line = (int)__double_as_longlong(t[7]);
      if (line != cur_line) {                            // block-uniform: step 4-5 for the line that ended
        if (cur_line >= 0) {
#pragma unroll
          for (int k = 0; k < ALIGN_SHIFTS; ++k) {
            if (d2m[k] <= r2) {
              score[k] += qi * (long long)rint((1.0 - d2m[k] / r2) * 1024.0);
              hits[k] += 1;
            }
            d2m[k] = inf;
          }
        }
        cur_line = line;
      }
      const double l2 = t[6];
      if (!(l2 > 0.0)) continue;                         // block-uniform
      const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5];
      // cost only: a hit at any shift of the slice lies inside the segment's box expanded by the reach
      if (!live || x < fmin(ax, bx) - rch || x > fmax(ax, bx) + rch || y < fmin(ay, by) - rch || y > fmax(ay, by) + rch)
        continue;
      const double ex = bx - ax, ey = by - ay, ez = bz - az;
      const double gz = z - az, gzez = gz * ez;
#pragma unroll
      for (int k = 0; k < ALIGN_SHIFTS; ++k) {
        const double gx = wx[k] - ax, gy = wy[k] - ay;
        const double dot = (gx * ex + gy * ey) + gzez;
        // clamp(dot / l2, 0, 1) without the division where the clamp decides (as fuse_project_kernel)
        double u;
        if (dot <= 0.0) u = 0.0;
        else if (dot >= l2) u = 1.0;
        else u = dot / l2;
        const double hx = wx[k] - (ax + u * ex), hy = wy[k] - (ay + u * ey), hz = z - (az + u * ez);
        const double d2 = (hx * hx + hy * hy) + hz * hz;
        d2m[k] = d2 < d2m[k] ? d2 : d2m[k];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < ALIGN_SHIFTS; ++k) {
    if (cur_line >= 0 && d2m[k] <= r2) {
      score[k] += qi * (long long)rint((1.0 - d2m[k] / r2) * 1024.0);
      hits[k] += 1;
    }
  }

#pragma unroll
  for (int k = 0; k < ALIGN_SHIFTS; ++k) {
    long long sc = score[k], ht = (long long)hits[k];
    for (int o = 32; o > 0; o >>= 1) { sc += __shfl_xor(sc, o); ht += __shfl_xor(ht, o); }
    if (lane == 0) { red[wave][k][0] = sc; red[wave][k][1] = ht; }
  }
  __syncthreads();
  if (tid < 2 * nk) {
    const int k = tid >> 1, col = tid & 1;
    long long sum = 0;
#pragma unroll
    for (int wv = 0; wv < ALIGN_WAVES; ++wv) sum += red[wv][k][col];
    if (sum != 0) atomicAdd(acc + 2 * (k0 + k) + col, (unsigned long long)sum);
  }
}

}  // namespace prh
