// Paint tracing on the GPU: lane candidates read from the bright ridges of every slice's own cloud,
// with no detector.  The rule is written out in include/pointnet_refine_hip.h ("Paint tracing - the
// rule"); tests/_trace_oracle.py restates it.
//   trace_hist_kernel      one thread per point: x y in one aligned load, the cell (ix, iy) of the
//                    slice's grid, z and I only for a point inside the grid, the slice by binary
//                    search (once per block where the block lies in one slice), then one 32-bit and
//                    four 64-bit integer atomics on the cell's sums.
//                    The hot pass: it reads every point once.
//   trace_hist_surface_kernel   the same point function with the surface gate compiled in ("Paint
//                    tracing - the rule: surface gate"): after qi > 0, the ground cell of the point and
//                    one fp64 gather from the road-height table; a point off the surface touches no
//                    table and is counted per slice, one 64-bit integer atomic per wave and slice.
//   trace_peaks_kernel<WRITE=false>   one wave per (slice, column).  The column's w goes through LDS
//                    TRACE_TILE cells at a time with a halo of TRACE_HALO cells on both sides; the box
//                    sums b are formed in LDS; a lane tests one cell against its 2 * nms neighbours;
//                    ballot / popcount counts the peaks of the column.
//   trace_peaks_kernel<WRITE=true>    the same walk; a peak goes to row col_offsets[column] + (peaks
//                    before it in the column), so the output is ordered by (slice, ix, iy) with no
//                    sort and no atomic.
//   trace_link_kernel      one thread per peak: succ and pred by walking at most max_gap_cols + 1
//                    column runs of the CSR each way, and once more from the partner to keep a link
//                    only where it is mutual.
// Every accumulated quantity is an integer, so no output depends on the order of the points, on the
// chunking of the slices or on the launch shape.  The geometry is fp64 with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_align.hpp"        // align_qi: the alignment rule's weight
#include "prh_bev.hpp"          // bev_slice_of: the slice of a flat row

namespace prh {

constexpr int TRACE_THREADS = 256;       // points per hist block, peaks per link block
constexpr int TRACE_TILE = 256;          // cells of a column per LDS round
constexpr int TRACE_MAX_NMS = 31;
constexpr int TRACE_HALO = TRACE_MAX_NMS + 1;
constexpr int TRACE_SLOTS = TRACE_TILE + 2 * TRACE_HALO;
constexpr int TRACE_MAX_CELLS = 4096;    // nx and ny

struct TraceGrid {
  double half_length, col, half_width, cell, intensity_floor;
  int nx, ny;
};

// the five tables of n_cells = S * nx * ny cells, cell (s, ix, iy) at (s * nx + ix) * ny + iy
struct TraceTables {
  int* n;
  unsigned long long *w, *wx, *wy, *wz;   // two's complement: the sums are signed
};

template <typename T> struct TracePair;
template <> struct TracePair<double> { typedef double2 type; };
template <> struct TracePair<float> { typedef float2 type; };

// the surface gate ("Paint tracing - the rule: surface gate"): the ground window and its table's shape
struct TraceSurface {
  double half_length, half_width, cell, band;
  int gx, gy;
};

// One point of the hist pass, for both kernels below.  SURFACE = false is trace_hist_kernel as it was:
// the gate's arguments are not read.  SURFACE = true: a point that passed every test up to qi > 0 is
// tested against ground [S][gx][gy] (the rows of the same slices as slice_off); the function returns
// true for a point off the surface, with its slice in s_out, and such a point touches no table.
// rows row0 .. row0 + n of pts; slice_off [S+1] holds absolute rows with slice_off[0] <= row0 and
// row0 + n <= slice_off[S]
template <typename T, bool SURFACE>
__device__ __forceinline__ bool trace_hist_point(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long row0, long long n,
    const TraceGrid& g, const TraceTables& t, const TraceSurface& sg, const double* __restrict__ ground, int& s_out) {
#pragma clang fp contract(off)
  typedef typename TracePair<T>::type pair_t;
  const long long k = (long long)blockIdx.x * TRACE_THREADS + threadIdx.x;
  if (k >= n) return false;
  const long long i = row0 + k;
  // the rows of a block lie in one slice far more often than not: one search per block, on uniform
  // addresses and in flight with the point's own loads, instead of one at the end of every wave's chain
  const long long b0 = row0 + (long long)blockIdx.x * TRACE_THREADS;
  const int s_block = bev_slice_of(slice_off, S, b0);
  const bool one_slice = slice_off[s_block + 1] >= b0 + TRACE_THREADS;
  const pair_t xy = reinterpret_cast<const pair_t*>(pts + 4 * i)[0];
  const double x = (double)xy.x, y = (double)xy.y;
  const double fx = floor((x + g.half_length) / g.col), fy = floor((y + g.half_width) / g.cell);
  if (!(fx >= 0.0 && fx < (double)g.nx && fy >= 0.0 && fy < (double)g.ny)) return false;      // NaN and inf leave here
  const pair_t zi = reinterpret_cast<const pair_t*>(pts + 4 * i)[1];
  const double z = (double)zi.x;
  if (!(isfinite(z) && fabs(z) <= 512.0)) return false;
  const long long qi = align_qi((double)zi.y, g.intensity_floor);
  if (qi <= 0) return false;
  const int s = one_slice ? s_block : bev_slice_of(slice_off, S, i);
  if constexpr (SURFACE) {
    // only a bright point comes here: the gather is paid by the paint and what is as bright
    const double gfx = floor((x + sg.half_length) / sg.cell), gfy = floor((y + sg.half_width) / sg.cell);
    bool on = gfx >= 0.0 && gfx < (double)sg.gx && gfy >= 0.0 && gfy < (double)sg.gy;
    if (on) {
      const double gz = ground[((long long)s * sg.gx + (long long)gfx) * sg.gy + (long long)gfy];
      on = gz == gz && fabs(z - gz) <= sg.band;
    }
    if (!on) {
      s_out = s;
      return true;
    }
  }
  const long long c = ((long long)s * g.nx + (long long)fx) * g.ny + (long long)fy;
  const long long qx = (long long)rint(x * 1024.0), qy = (long long)rint(y * 1024.0), qz = (long long)rint(z * 1024.0);
  atomicAdd(t.n + c, 1);
  atomicAdd(t.w + c, (unsigned long long)qi);
  atomicAdd(t.wx + c, (unsigned long long)(qi * qx));
  atomicAdd(t.wy + c, (unsigned long long)(qi * qy));
  atomicAdd(t.wz + c, (unsigned long long)(qi * qz));
  return false;
}

template <typename T>
__global__ __launch_bounds__(TRACE_THREADS) void trace_hist_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long row0, long long n, TraceGrid g,
    TraceTables t) {
  int s = 0;
  trace_hist_point<T, false>(pts, slice_off, S, row0, n, g, t, TraceSurface{}, nullptr, s);
}

// off_surface [S], zeroed by the caller.  Every lane of the wave is back here after its point: the
// lanes off the surface are counted per slice with ballot / popcount and their first lane adds the
// count, so a wave that straddles slice boundaries counts each side into its own slice.
template <typename T>
__global__ __launch_bounds__(TRACE_THREADS) void trace_hist_surface_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long row0, long long n, TraceGrid g,
    TraceTables t, TraceSurface sg, const double* __restrict__ ground, unsigned long long* __restrict__ off_surface) {
  int s = -1;
  const bool off = trace_hist_point<T, true>(pts, slice_off, S, row0, n, g, t, sg, ground, s);
  const int lane = threadIdx.x & 63;
  unsigned long long left = __ballot(off);
  while (left) {                           // uniform over the wave: one round per slice touched
    const int first = __ffsll((long long)left) - 1;
    const int s_first = __shfl(s, first, 64);
    const unsigned long long same = __ballot(off && s == s_first);
    if (lane == first) atomicAdd(off_surface + s_first, (unsigned long long)__popcll(same));
    left &= ~same;
  }
}

// the sum of tab over cells iy - 1, iy, iy + 1 of the column that starts at base
__device__ __forceinline__ long long trace_box(const unsigned long long* __restrict__ tab, long long base, int iy, int ny) {
  long long b = (long long)tab[base + iy];
  if (iy > 0) b += (long long)tab[base + iy - 1];
  if (iy + 1 < ny) b += (long long)tab[base + iy + 1];
  return b;
}

// one 64-lane block per column; col_base: the number of the launch's first column in the caller's
// count of all columns (what out_col holds)
template <bool WRITE>
__global__ __launch_bounds__(64) void trace_peaks_kernel(
    TraceTables t, int ny, int nms, int min_points, long long min_weight, int* __restrict__ col_counts,
    const long long* __restrict__ col_off, long long capacity, int col_base, int* __restrict__ out_iy,
    long long* __restrict__ out_b, int* __restrict__ out_n3, double* __restrict__ out_xyz, int* __restrict__ out_col) {
#pragma clang fp contract(off)
  __shared__ long long wl[TRACE_SLOTS];    // w of cells t0 - HALO .. t0 + TILE + HALO - 1, 0 outside the grid
  __shared__ long long bl[TRACE_SLOTS];    // b of the same cells, 0 outside the grid
  const int lane = threadIdx.x;
  const int column = blockIdx.x;
  const long long base = (long long)column * ny;
  const long long out0 = WRITE ? col_off[column] : 0, out1 = WRITE ? col_off[column + 1] : 0;
  int found = 0;
  for (int t0 = 0; t0 < ny; t0 += TRACE_TILE) {
    for (int j = lane; j < TRACE_SLOTS; j += 64) {
      const int cell = t0 - TRACE_HALO + j;
      wl[j] = (cell >= 0 && cell < ny) ? (long long)t.w[base + cell] : 0ll;
    }
    __syncthreads();
    // slots 0 and TRACE_SLOTS - 1 lack a neighbour; no test reads them (nms < HALO)
    for (int j = lane; j < TRACE_SLOTS; j += 64) {
      const int cell = t0 - TRACE_HALO + j;
      long long b = 0;
      if (cell >= 0 && cell < ny) b = (j > 0 ? wl[j - 1] : 0ll) + wl[j] + (j + 1 < TRACE_SLOTS ? wl[j + 1] : 0ll);
      bl[j] = b;
    }
    __syncthreads();
    for (int r = 0; r < TRACE_TILE && t0 + r < ny; r += 64) {
      const int cell = t0 + r + lane, j = TRACE_HALO + r + lane;
      bool peak = false;
      long long b = 0;
      int n3 = 0;
      if (cell < ny) {
        b = bl[j];
        peak = b >= min_weight;
        for (int k = 1; k <= nms && peak; ++k) peak = b > bl[j - k] && b >= bl[j + k];
        if (peak) {
          n3 = t.n[base + cell] + (cell > 0 ? t.n[base + cell - 1] : 0) + (cell + 1 < ny ? t.n[base + cell + 1] : 0);
          peak = n3 >= min_points;
        }
      }
      const unsigned long long m = __ballot(peak);
      if (WRITE && peak) {
        const long long pos = out0 + found + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < out1 && pos < capacity) {
          const double fb = (double)b;
          out_iy[pos] = cell;
          out_b[pos] = b;
          out_n3[pos] = n3;
          out_col[pos] = col_base + column;
          out_xyz[3 * pos] = ((double)trace_box(t.wx, base, cell, ny) / fb) / 1024.0;
          out_xyz[3 * pos + 1] = ((double)trace_box(t.wy, base, cell, ny) / fb) / 1024.0;
          out_xyz[3 * pos + 2] = ((double)trace_box(t.wz, base, cell, ny) / fb) / 1024.0;
        }
      }
      found += __popcll(m);
    }
    __syncthreads();                       // the next round overwrites wl and bl
  }
  if (!WRITE && lane == 0) col_counts[column] = found;
}

// succ (dir = +1) or pred (dir = -1) of a peak at (ix, iy) of the slice whose columns start at col0
__device__ __forceinline__ int trace_walk(const long long* __restrict__ col_off, const int* __restrict__ iy_of,
                                          long long n_peaks, long long col0, int nx, int ix, int iy, int dir,
                                          int link_cells, int gap_slope, int max_gap_cols) {
  for (int dc = 1; dc <= max_gap_cols + 1; ++dc) {
    const int c = ix + dir * dc;
    if (c < 0 || c >= nx) break;
    long long a = col_off[col0 + c], b = col_off[col0 + c + 1];
    if (a < 0) a = 0;
    if (b > n_peaks) b = n_peaks;
    if (a >= b) continue;
    const long long tol = (long long)link_cells + (long long)gap_slope * (dc - 1);
    long long best = -1, best_d = 0x7fffffffll;
    for (long long q = a; q < b; ++q) {      // ascending iy: the first of two equal distances is the smaller iy
      const long long d = iy_of[q] >= iy ? (long long)iy_of[q] - iy : (long long)iy - iy_of[q];
      if (d < best_d) { best_d = d; best = q; }
      else if (iy_of[q] >= iy) break;
    }
    if (best_d <= tol) return (int)best;
  }
  return -1;
}

__global__ __launch_bounds__(TRACE_THREADS) void trace_link_kernel(
    const long long* __restrict__ col_off, long long n_cols, int nx, const int* __restrict__ iy_of,
    const int* __restrict__ col_of, long long n_peaks, int link_cells, int gap_slope, int max_gap_cols,
    int* __restrict__ succ, int* __restrict__ pred) {
  const long long p = (long long)blockIdx.x * TRACE_THREADS + threadIdx.x;
  if (p >= n_peaks) return;
  int out[2] = {-1, -1};
  const long long column = col_of[p];
  if (column >= 0 && column < n_cols) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int dir = side == 0 ? 1 : -1;
      const long long col0 = column / nx * nx;
      const int q = trace_walk(col_off, iy_of, n_peaks, col0, nx, (int)(column - col0), iy_of[p], dir, link_cells,
                               gap_slope, max_gap_cols);
      if (q >= 0) {
        const long long qc = col_of[q];
        const int back = trace_walk(col_off, iy_of, n_peaks, col0, nx, (int)(qc - col0), iy_of[q], -dir, link_cells,
                                    gap_slope, max_gap_cols);
        if ((long long)back == p) out[side] = q;
      }
    }
  }
  succ[p] = out[0];
  pred[p] = out[1];
}

}  // namespace prh
