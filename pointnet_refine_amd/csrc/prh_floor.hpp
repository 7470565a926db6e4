// Paint floor on the GPU: the intensity threshold between asphalt and paint, read from the points on
// the road surface of every slice.  The rule is written out in include/pointnet_refine_hip.h ("Paint
// floor - the rule"); tests/_floor_oracle.py restates it.
//   floor_hist_kernel<T, COPIES>   a block of 256 threads walks FLOOR_RUN rows, 256 at a time: x y in one
//                    aligned load, the cell (ix, iy) of the surface grid, z and I only for a point inside
//                    the window, the slice by binary search (once per block where the block lies in one
//                    slice), one fp64 gather from the ground table, the surface gate, then one LDS atomic
//                    on the block's private histogram of its first slice (COPIES lane-interleaved copies);
//                    a point of another slice in a block that straddles a boundary goes straight to
//                    the global table.  The non-zero bins are flushed with 64-bit integer atomics.
//                    The hot pass: it reads every point once.
//   floor_otsu_kernel   one wave per histogram row: isqrt of every count, the three integer prefix
//                    sums by a wave scan into LDS, every lane scores its own thresholds by the
//                    written operation sequence, the wave takes the arg-max with the smallest t
//                    winning and finds the end of the plateau with ballots.  No atomics.
// Every accumulated quantity is an integer, so no output depends on the order of the points, on their
// dtype or on the launch shape.  The geometry is fp64 with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_bev.hpp"          // bev_slice_of: the slice of a flat row
#include "prh_trace.hpp"        // TracePair: the two-coordinate load

namespace prh {

constexpr int FLOOR_THREADS = 256;
constexpr int FLOOR_ROUNDS = 8;                               // rows per thread
constexpr int FLOOR_RUN = FLOOR_THREADS * FLOOR_ROUNDS;       // rows per block
constexpr int FLOOR_MAX_BINS = 1024;
constexpr int FLOOR_MAX_CELLS = 1024;                         // gx and gy
constexpr int FLOOR_COPIES = 8;                               // LDS copies of a block's histogram: the fastest of 1, 2, 4, 8

struct FloorGrid {
  double half_length, half_width, cell, band, bin_width;
  int gx, gy, n_bins;
};

// rows 0 .. n of pts; slice_off [S+1] with slice_off[0] = 0 and n <= slice_off[S]; ground [S][gx][gy];
// hist [S][n_bins], zeroed by the caller
template <typename T, int COPIES>
__global__ __launch_bounds__(FLOOR_THREADS) void floor_hist_kernel(
    const T* __restrict__ pts, const long long* __restrict__ slice_off, int S, long long n, FloorGrid g,
    const double* __restrict__ ground, unsigned long long* __restrict__ hist) {
#pragma clang fp contract(off)
  typedef typename TracePair<T>::type pair_t;
  __shared__ unsigned lh[FLOOR_MAX_BINS * COPIES];           // bin b of copy c at b * COPIES + c
  const int tid = threadIdx.x;
  const int used = g.n_bins * COPIES;
  for (int j = tid; j < used; j += FLOOR_THREADS) lh[j] = 0u;
  const long long b0 = (long long)blockIdx.x * FLOOR_RUN;
  const int s_block = bev_slice_of(slice_off, S, b0);
  const bool one_slice = slice_off[s_block + 1] >= b0 + FLOOR_RUN;
  const int copy = tid & (COPIES - 1);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < FLOOR_ROUNDS; ++r) {
    const long long i = b0 + r * FLOOR_THREADS + tid;
    if (i >= n) continue;
    const pair_t xy = reinterpret_cast<const pair_t*>(pts + 4 * i)[0];
    const double fx = floor(((double)xy.x + g.half_length) / g.cell), fy = floor(((double)xy.y + g.half_width) / g.cell);
    if (!(fx >= 0.0 && fx < (double)g.gx && fy >= 0.0 && fy < (double)g.gy)) continue;    // NaN and inf leave here
    const pair_t zi = reinterpret_cast<const pair_t*>(pts + 4 * i)[1];
    const int s = one_slice ? s_block : bev_slice_of(slice_off, S, i);
    const double gz = ground[((long long)s * g.gx + (long long)fx) * g.gy + (long long)fy];
    const double z = (double)zi.x, in = (double)zi.y;
    if (!(gz == gz) || !isfinite(z) || !(fabs(z - gz) <= g.band)) continue;
    if (!isfinite(in) || !(in >= 0.0)) continue;
    const double fb = floor(in / g.bin_width);
    const int b = fb >= (double)g.n_bins ? g.n_bins - 1 : (int)fb;
    if (s == s_block) atomicAdd(&lh[b * COPIES + copy], 1u);
    else atomicAdd(hist + (long long)s * g.n_bins + b, 1ull);
  }
  __syncthreads();
  for (int b = tid; b < g.n_bins; b += FLOOR_THREADS) {
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < COPIES; ++k) c += lh[b * COPIES + k];
    if (c) atomicAdd(hist + (long long)s_block * g.n_bins + b, (unsigned long long)c);
  }
}

// the exact integer floor square root; a count below 1 gives 0
__device__ __forceinline__ long long floor_isqrt(long long h) {
  if (h <= 0) return 0;
  const unsigned long long u = (unsigned long long)h;
  unsigned long long r = (unsigned long long)sqrt((double)h);
  while (r * r > u) --r;
  while ((r + 1) * (r + 1) <= u) ++r;
  return (long long)r;
}

__device__ __forceinline__ long long floor_wave_inclusive(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// one 64-lane block per row of hist [R][n]; a count below 0 counts as 0
__global__ __launch_bounds__(64) void floor_otsu_kernel(
    const long long* __restrict__ hist, int n, long long min_points, int* __restrict__ t_lo_out, int* __restrict__ t_hi_out,
    int* __restrict__ t_out, long long* __restrict__ total, long long* __restrict__ above, long long* __restrict__ w0_out,
    long long* __restrict__ m0_out, long long* __restrict__ wr_out, long long* __restrict__ mr_out,
    double* __restrict__ score_out) {
#pragma clang fp contract(off)
  __shared__ long long pw[FLOOR_MAX_BINS + 1], pm[FLOOR_MAX_BINS + 1], pc[FLOOR_MAX_BINS + 1];   // sums over b < t
  __shared__ double sc[FLOOR_MAX_BINS];                      // the score of t, -1 where t is no candidate
  const int lane = threadIdx.x;
  const long long row = blockIdx.x;
  const long long* __restrict__ h = hist + row * n;
  const int per = (n + 63) / 64;
  const int first = lane * per, last = first + per < n ? first + per : n;
  long long lw = 0, lm = 0, lc = 0;
  for (int b = first; b < last; ++b) {
    const long long c = h[b] > 0 ? h[b] : 0, r = floor_isqrt(c);
    lw += r;
    lm += (long long)b * r;
    lc += c;
  }
  const long long iw = floor_wave_inclusive(lw, lane), im = floor_wave_inclusive(lm, lane), ic = floor_wave_inclusive(lc, lane);
  const long long Wr = __shfl(iw, 63, 64), Mr = __shfl(im, 63, 64), W = __shfl(ic, 63, 64);
  long long w = iw - lw, m = im - lm, c0 = ic - lc;
  for (int b = first; b < last; ++b) {
    pw[b] = w;
    pm[b] = m;
    pc[b] = c0;
    const long long c = h[b] > 0 ? h[b] : 0, r = floor_isqrt(c);
    w += r;
    m += (long long)b * r;
    c0 += c;
  }
  if (lane == 63) { pw[n] = Wr; pm[n] = Mr; pc[n] = W; }
  __syncthreads();
  double best = -1.0;
  int best_t = 0x7fffffff;
  for (int t = lane; t < n; t += 64) {
    double s = -1.0;
    const long long w0 = pw[t], w1 = Wr - w0;
    if (t >= 1 && pc[t] >= min_points && W - pc[t] >= min_points && w0 > 0 && w1 > 0) {
      const long long m0 = pm[t], m1 = Mr - m0;
      const double d = (double)m1 / (double)w1 - (double)m0 / (double)w0;
      const double p = (double)w0 * (double)w1;
      s = p * (d * d);
    }
    sc[t] = s;
    if (s > best) { best = s; best_t = t; }                  // ascending t: the first of equal scores stays
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double os = __shfl_xor(best, d, 64);
    const int ot = __shfl_xor(best_t, d, 64);
    if (os > best || (os == best && ot < best_t)) { best = os; best_t = ot; }
  }
  __syncthreads();
  int t_lo = -1, t_hi = -1, ts = -1;
  if (best > 0.0) {
    t_lo = best_t;
    t_hi = n - 1;
    for (int base = t_lo + 1; base < n; base += 64) {
      const int u = base + lane;
      const unsigned long long ok = __ballot(u < n && sc[u] == best);
      if (ok != ~0ull) {
        t_hi = base + (__ffsll((long long)~ok) - 1) - 1;
        break;
      }
    }
    ts = (t_lo + t_hi) >> 1;
  }
  if (lane == 0) {
    t_lo_out[row] = t_lo;
    t_hi_out[row] = t_hi;
    t_out[row] = ts;
    total[row] = W;
    above[row] = ts >= 0 ? W - pc[ts] : 0;
    w0_out[row] = t_lo >= 0 ? pw[t_lo] : 0;
    m0_out[row] = t_lo >= 0 ? pm[t_lo] : 0;
    wr_out[row] = Wr;
    mr_out[row] = Mr;
    score_out[row] = t_lo >= 0 ? best : 0.0;
  }
}

}  // namespace prh
