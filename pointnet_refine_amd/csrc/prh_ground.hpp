// Ground lift on the GPU: the height of the road surface under an xy, read from the slice's own
// cloud, for every query of every slice in one ragged pass.  The rule is written out in
// include/pointnet_refine_hip.h ("Ground lift - the rule"); tests/_ground_oracle.py restates it.
//   ground_bin_kernel<WRITE=false>   one thread per point: the slice of the point (binary search in
//                    slice_offsets), its cell in that slice's uniform xy grid, one integer atomic
//                    on the cell's counter.  Points outside the grid (the slice's queries expanded
//                    by the reach) or with a non-finite x, y or z are dropped here.
//   ground_bin_kernel<WRITE=true>    the same walk; the point's row inside its slice goes to
//                    rows[cell_offsets[cell] + cursor[cell]++].  The order inside a cell is the
//                    order of arrival: the rule does not see it.
//   ground_query_kernel   one 64-lane wave per query, four queries per block.  The cells the
//                    interval [q - reach, q + reach] touches are, per grid row, one contiguous run
//                    of `rows`; lanes stride over the runs, load x y, and z only for hits.  Sweep 1
//                    fills the wave's 256-bin histogram in LDS with integer atomics; c3, the peak,
//                    g and the climb are found across the wave; sweep 2 walks the same runs
//                    (L2-hot) for the integer sum and count of the mode.  Lane 0 stores the four
//                    outputs.
// Every accumulated quantity is an integer, so no output depends on the order of the points, on
// the cell size or on the launch shape.  The geometry is fp64 with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_bev.hpp"          // bev_slice_of: the slice of a flat row

namespace prh {

constexpr int GROUND_THREADS = 256;
constexpr int GROUND_WAVES = GROUND_THREADS / 64;
constexpr int GROUND_MAX_BINS = 256;     // 64 lanes x 4 bins

template <typename T> struct GroundXY;
template <> struct GroundXY<double> { typedef double2 type; };
template <> struct GroundXY<float> { typedef float2 type; };

// grid of slice s: origin[2s], origin[2s+1] = x0 y0, shape[2s], shape[2s+1] = nx ny, cells
// cell_base[s] + iy * nx + ix.  The cell index is floor((x - x0) / cell) in fp64, the host's expression.
template <typename T, bool WRITE>
__global__ __launch_bounds__(GROUND_THREADS) void ground_bin_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long n,
    const double* __restrict__ origin, const int* __restrict__ shape, const long long* __restrict__ cell_base,
    long long n_cells, double cell, int* __restrict__ counter, const long long* __restrict__ cell_off,
    int* __restrict__ rows, long long capacity) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * GROUND_THREADS + threadIdx.x;
  if (i >= n) return;
  const typename GroundXY<T>::type p = reinterpret_cast<const typename GroundXY<T>::type*>(pts + 4 * i)[0];
  const double x = (double)p.x, y = (double)p.y, z = (double)pts[4 * i + 2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return;
  const int s = bev_slice_of(slice_off, S, i);
  const int nx = shape[2 * s], ny = shape[2 * s + 1];
  const double fx = floor((x - origin[2 * s]) / cell), fy = floor((y - origin[2 * s + 1]) / cell);
  if (!(fx >= 0.0 && fx < (double)nx && fy >= 0.0 && fy < (double)ny)) return;
  const long long c = cell_base[s] + (long long)fy * nx + (long long)fx;
  if (c < 0 || c >= n_cells) return;                     // cannot happen with the host's cell_base
  const int k = atomicAdd(counter + c, 1);
  if (WRITE) {
    const long long pos = cell_off[c] + k;
    if (pos < cell_off[c + 1] && pos < capacity) rows[pos] = (int)(i - slice_off[s]);
  }
}

struct GroundParams {
  double r2, reach, cell, z_lo, bin;
  int n_bins, min_points, peak_num, peak_den;
};

// the run of `rows` that grid row iy of the query's cell range owns, clipped to [0, n_rows]
__device__ __forceinline__ void ground_run(const long long* __restrict__ cell_off, long long row0, int ix_lo, int ix_hi,
                                           long long n_rows, long long& a, long long& b) {
  a = cell_off[row0 + ix_lo];
  b = cell_off[row0 + ix_hi + 1];
  if (a < 0) a = 0;
  if (b > n_rows) b = n_rows;
}

template <typename T>
__global__ __launch_bounds__(GROUND_THREADS) void ground_query_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, const double* __restrict__ queries,
    const long long* __restrict__ query_off, long long Q, const double* __restrict__ origin,
    const int* __restrict__ shape, const long long* __restrict__ cell_base, const long long* __restrict__ cell_off,
    const int* __restrict__ rows, long long n_rows, long long n_cells, GroundParams prm, double* __restrict__ height,
    int* __restrict__ count, int* __restrict__ hits_out, int* __restrict__ bin_out) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[GROUND_WAVES][GROUND_MAX_BINS + 2];   // [0] and [257] stay 0: the missing neighbours
  __shared__ unsigned c3s[GROUND_WAVES][GROUND_MAX_BINS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * GROUND_WAVES + w;
  const bool live = q < Q;                               // wave-uniform; every wave meets every barrier
  for (int b = lane; b < GROUND_MAX_BINS + 2; b += 64) hist[w][b] = 0u;
  __syncthreads();

  int ix_lo = 0, ix_hi = -1, iy_lo = 0, iy_hi = -1, nx = 0;
  long long base = 0, p0 = 0, plen = 0;
  double qx = 0.0, qy = 0.0;
  if (live) {
    const int s = bev_slice_of(query_off, S, q);
    qx = queries[2 * q]; qy = queries[2 * q + 1];
    nx = shape[2 * s];
    const int ny = shape[2 * s + 1];
    p0 = slice_off[s]; plen = slice_off[s + 1] - p0;
    base = cell_base[s];
    if (nx > 0 && ny > 0 && base >= 0 && base + (long long)nx * ny <= n_cells) {
      const double x0 = origin[2 * s], y0 = origin[2 * s + 1];
      // the same monotone floor as the binning: a hit's cell lies between the cells of q -+ reach
      const double ax = fmax(floor(((qx - prm.reach) - x0) / prm.cell), 0.0);
      const double bx = fmin(floor(((qx + prm.reach) - x0) / prm.cell), (double)(nx - 1));
      const double ay = fmax(floor(((qy - prm.reach) - y0) / prm.cell), 0.0);
      const double by = fmin(floor(((qy + prm.reach) - y0) / prm.cell), (double)(ny - 1));
      if (ax <= bx && ay <= by) { ix_lo = (int)ax; ix_hi = (int)bx; iy_lo = (int)ay; iy_hi = (int)by; }
    }
  }

  // sweep 1: hits and the histogram
  int hits = 0;
  for (int iy = iy_lo; iy <= iy_hi && ix_lo <= ix_hi; ++iy) {
    long long a, b;
    ground_run(cell_off, base + (long long)iy * nx, ix_lo, ix_hi, n_rows, a, b);
    for (long long i = a + lane; i < b; i += 64) {
      const unsigned r = (unsigned)rows[i];
      if ((long long)r >= plen) continue;                // cannot happen with bin_write's rows
      const T* p = pts + 4 * (p0 + r);
      const typename GroundXY<T>::type xy = reinterpret_cast<const typename GroundXY<T>::type*>(p)[0];
      const double dx = (double)xy.x - qx, dy = (double)xy.y - qy;
      const double d2 = dx * dx + dy * dy;
      if (!(d2 <= prm.r2)) continue;
      const double z = (double)p[2];
      if (!isfinite(z)) continue;
      ++hits;
      const double f = floor((z - prm.z_lo) / prm.bin);
      if (f >= 0.0 && f < (double)prm.n_bins) atomicAdd(&hist[w][(int)f + 1], 1u);
    }
  }
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o);
  __syncthreads();

  // c3 of the lane's four bins, the peak, the threshold, the lowest bin that reaches it
  unsigned c3[4];
  unsigned peak = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int b = 4 * lane + k;
    c3[k] = b < prm.n_bins ? hist[w][b] + hist[w][b + 1] + hist[w][b + 2] : 0u;
    c3s[w][b] = c3[k];
    peak = c3[k] > peak ? c3[k] : peak;
  }
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(peak, o); peak = t > peak ? t : peak; }
  __syncthreads();
  const bool ground = live && (long long)peak >= (long long)prm.min_points;
  int g = -1;
  if (ground) {
    long long thr = ((long long)peak * prm.peak_num + prm.peak_den - 1) / prm.peak_den;
    if (thr < prm.min_points) thr = prm.min_points;
    int first = GROUND_MAX_BINS;
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if ((long long)c3[k] >= thr) first = 4 * lane + k;
    for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(first, o); first = t < first ? t : first; }
    g = first;                                           // < n_bins: the peak's bin reaches thr
    while (g + 1 < prm.n_bins && c3s[w][g + 1] > c3s[w][g]) ++g;      // wave-uniform
  }

  // sweep 2: the integer sum over the mode's three bins
  long long sum = 0;
  int n = 0;
  if (ground) {
    const double f_lo = (double)(g - 1 < 0 ? 0 : g - 1);
    const double f_hi = (double)(g + 1 > prm.n_bins - 1 ? prm.n_bins - 1 : g + 1);
    for (int iy = iy_lo; iy <= iy_hi; ++iy) {
      long long a, b;
      ground_run(cell_off, base + (long long)iy * nx, ix_lo, ix_hi, n_rows, a, b);
      for (long long i = a + lane; i < b; i += 64) {
        const unsigned r = (unsigned)rows[i];
        if ((long long)r >= plen) continue;
        const T* p = pts + 4 * (p0 + r);
        const typename GroundXY<T>::type xy = reinterpret_cast<const typename GroundXY<T>::type*>(p)[0];
        const double dx = (double)xy.x - qx, dy = (double)xy.y - qy;
        const double d2 = dx * dx + dy * dy;
        if (!(d2 <= prm.r2)) continue;
        const double z = (double)p[2];
        if (!isfinite(z)) continue;
        const double f = floor((z - prm.z_lo) / prm.bin);
        if (f >= f_lo && f <= f_hi) { sum += (long long)rint(z * 65536.0); ++n; }
      }
    }
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); n += __shfl_xor(n, o); }
  }
  if (live && lane == 0) {
    height[q] = ground ? ((double)sum / (double)n) / 65536.0 : __longlong_as_double(0x7ff8000000000000ll);
    count[q] = ground ? n : 0;
    hits_out[q] = hits;
    bin_out[q] = g;
  }
}

}  // namespace prh
