// Piece linking on the GPU: which refined pieces of a drive are the same lane, without a carrier.
// The rule is written out in include/pointnet_refine_hip.h ("Piece linking - the rule");
// tests/_link_oracle.py restates it.
//   link_box_kernel     one thread per piece: lo / hi over its points, per axis (step 1)
//   link_pairs_kernel   steps 2: a block owns LINK_ROWS pieces i (LINK_ROWS / 4 per wave) and walks
//                       the boxes of the j side LINK_TILE at a time through LDS; a wave tests 64 j
//                       per instruction and compacts with __ballot / popcount, so a row's j come out
//                       ascending with no sort and no atomic.  <false> counts, <true> writes.
//   link_scan_kernel    one block: exclusive scan of the row counts into pair_offsets
//   link_stats_kernel   steps 3-4: one wave per candidate pair, LINK_PAIRS pairs per block; both
//                       pieces and their cum in LDS, one lane per point (M <= 32: both directions at
//                       once in the wave's halves), every lane's contribution to LDS, then six lanes
//                       each run one serial sum in the rule's order
// Everything is fp64 with FMA contraction off: one rounding per operation, as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_fuse.hpp"         // FUSE_MAX_POINTS, fuse_owner

namespace prh {

constexpr int LINK_THREADS = 256;
constexpr int LINK_TILE = 256;          // boxes of the j side per LDS round (6 doubles + frame: 13 KB)
constexpr int LINK_ROWS = 32;           // pieces i per block of link_pairs_kernel (8 per wave)
constexpr int LINK_PAIRS = LINK_THREADS / 64;          // pairs per block of link_stats_kernel
constexpr int LINK_SLOTS = 2 * FUSE_MAX_POINTS + 2;    // contributions of a pair, padded: the four sum
                                                       // lanes read rows 1040 B apart, on different banks
constexpr int LINK_SCAN_THREADS = 1024;

// box [n_pieces,6] = lo x y z, hi x y z
__global__ __launch_bounds__(LINK_THREADS) void link_box_kernel(const double* __restrict__ world, int n_pieces, int M,
                                                                double* __restrict__ box) {
  const int p = blockIdx.x * LINK_THREADS + threadIdx.x;
  if (p >= n_pieces) return;
  const double* v = world + (long long)p * M * 3;
  double lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
  for (int k = 1; k < M; ++k)
    for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], v[3 * k + c]); hi[c] = fmax(hi[c], v[3 * k + c]); }
  for (int c = 0; c < 3; ++c) { box[6 * (long long)p + c] = lo[c]; box[6 * (long long)p + 3 + c] = hi[c]; }
}

// WRITE false: row_count [n_pieces] = candidates (i, j > i) of row i.  WRITE true: pair_j filled from
// pair_offsets[i] on, ascending j.
template <bool WRITE>
__global__ __launch_bounds__(LINK_THREADS) void link_pairs_kernel(const double* __restrict__ box,
                                                                  const int* __restrict__ frame, int n_pieces,
                                                                  double gate, long long* __restrict__ row_count,
                                                                  const long long* __restrict__ pair_offsets,
                                                                  int* __restrict__ pair_j) {
#pragma clang fp contract(off)
  __shared__ double sh_box[6][LINK_TILE];
  __shared__ int sh_frame[LINK_TILE];
  constexpr int PER_WAVE = LINK_ROWS / (LINK_THREADS / 64);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.x * LINK_ROWS;             // row0 < n_pieces by the grid
  long long at[PER_WAVE], end[PER_WAVE];               // end: a row never writes past its own share
#pragma unroll
  for (int r = 0; r < PER_WAVE; ++r) {
    const int i = row0 + wave * PER_WAVE + r;
    at[r] = (WRITE && i < n_pieces) ? pair_offsets[i] : 0;
    end[r] = (WRITE && i < n_pieces) ? pair_offsets[i + 1] : 0;
  }
  for (int base = (row0 + 1) / LINK_TILE * LINK_TILE; base < n_pieces; base += LINK_TILE) {
    const int jt = base + tid;
    if (jt < n_pieces) {
      for (int c = 0; c < 6; ++c) sh_box[c][tid] = box[6 * (long long)jt + c];
      sh_frame[tid] = frame[jt];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PER_WAVE; ++r) {
      const int i = row0 + wave * PER_WAVE + r;        // the same for the whole wave
      if (i >= n_pieces || base + LINK_TILE <= i + 1) continue;
      const double* bi = box + 6 * (long long)i;
      const double lx = bi[0] - gate, ly = bi[1] - gate, lz = bi[2] - gate, hx = bi[3], hy = bi[4], hz = bi[5];
      const int fi = frame[i];
      for (int t = lane; t < LINK_TILE; t += 64) {
        const int j = base + t;
        bool ok = j > i && j < n_pieces;
        if (ok) {
          ok = sh_frame[t] != fi && lx <= sh_box[3][t] && ly <= sh_box[4][t] && lz <= sh_box[5][t] &&
               sh_box[0][t] - gate <= hx && sh_box[1][t] - gate <= hy && sh_box[2][t] - gate <= hz;
        }
        const unsigned long long mask = __ballot(ok);
        if (WRITE && ok) {
          const long long slot = at[r] + __popcll(mask & ((1ull << lane) - 1ull));
          if (slot < end[r]) pair_j[slot] = j;
        }
        at[r] += __popcll(mask);
      }
    }
    __syncthreads();
  }
  if (!WRITE && lane == 0) {
#pragma unroll
    for (int r = 0; r < PER_WAVE; ++r) {
      const int i = row0 + wave * PER_WAVE + r;
      if (i < n_pieces) row_count[i] = at[r];
    }
  }
}

// pair_offsets [n+1] = exclusive scan of row_count [n]; one block, a contiguous run of rows per thread
__global__ __launch_bounds__(LINK_SCAN_THREADS) void link_scan_kernel(const long long* __restrict__ row_count, int n,
                                                                      long long* __restrict__ pair_offsets) {
  __shared__ long long part[LINK_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int per = (n + LINK_SCAN_THREADS - 1) / LINK_SCAN_THREADS;
  const int a = tid * per < n ? tid * per : n, b = a + per < n ? a + per : n;
  long long sum = 0;
  for (int i = a; i < b; ++i) sum += row_count[i];
  part[tid] = sum;
  __syncthreads();
  for (int d = 1; d < LINK_SCAN_THREADS; d <<= 1) {                // inclusive scan of the partial sums
    const long long add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  long long run = part[tid] - sum;
  for (int i = a; i < b; ++i) { pair_offsets[i] = run; run += row_count[i]; }
  if (tid == LINK_SCAN_THREADS - 1) pair_offsets[n] = part[tid];
}

// world [n_pieces*M,3], cum [n_pieces*M]; pair p is (i, j) with pair_offsets[i] <= p < pair_offsets[i+1]
// and j = pair_j[p].  pair_count [n_pairs,2] = n_in n_out, pair_sum [n_pairs,4] = sum_d sum_self
// sum_other sum_dot.  A j outside 0..n_pieces-1 gives -1 counts and NaN sums.
__global__ __launch_bounds__(LINK_THREADS) void link_stats_kernel(
    const double* __restrict__ world, const double* __restrict__ cum, int n_pieces, int M,
    const long long* __restrict__ pair_offsets, const int* __restrict__ pair_j, long long n_pairs, double gate,
    int* __restrict__ pair_count, double* __restrict__ pair_sum) {
#pragma clang fp contract(off)
  __shared__ double sh_pt[LINK_PAIRS][2][4][FUSE_MAX_POINTS];      // piece (0: i, 1: j), x y z cum, point
  __shared__ double sh_val[LINK_PAIRS][4][LINK_SLOTS];             // d, self, other, dot per contribution
  __shared__ int sh_flag[LINK_PAIRS][2 * FUSE_MAX_POINTS];         // 0 clamped, 1 in, 2 out
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long pair = (long long)blockIdx.x * LINK_PAIRS + wave;
  const bool live = pair < n_pairs;                    // the same for a whole wave
  const int i = live ? fuse_owner(pair_offsets, n_pieces, pair) : 0;
  const int j = live ? pair_j[pair] : 0;
  const bool valid = live && j >= 0 && j < n_pieces;
  if (live && !valid) {
    if (lane < 2) pair_count[2 * pair + lane] = -1;
    if (lane < 4) pair_sum[4 * pair + lane] = __longlong_as_double(0x7ff8000000000000ll);
  }
  // stage both pieces: lane k holds point k of each
  if (valid && lane < M) {
    const int pc[2] = {i, j};
    for (int h = 0; h < 2; ++h) {
      const long long g = (long long)pc[h] * M + lane;
      sh_pt[wave][h][0][lane] = world[3 * g]; sh_pt[wave][h][1][lane] = world[3 * g + 1];
      sh_pt[wave][h][2][lane] = world[3 * g + 2]; sh_pt[wave][h][3][lane] = cum[g];
    }
  }
  __syncthreads();
  const bool both = M <= 32;                           // both directions at once, one per half wave
  const int k = both ? (lane & 31) : lane;
  for (int round = 0; round < (both ? 1 : 2); ++round) {
    const int dir = both ? (lane >> 5) : round;        // 0: i -> j, 1: j -> i
    if (valid && k < M) {
      const double(*A)[FUSE_MAX_POINTS] = sh_pt[wave][dir];
      const double(*B)[FUSE_MAX_POINTS] = sh_pt[wave][1 - dir];
      const double wx = A[0][k], wy = A[1][k], wz = A[2][k];
      double best = __longlong_as_double(0x7ff0000000000000ll), best_u = 0.0;      // +inf
      int best_k = -1, first = -1, last = -1;
      double ax = B[0][0], ay = B[1][0], az = B[2][0];
      for (int s = 0; s + 1 < M; ++s) {
        const double bx = B[0][s + 1], by = B[1][s + 1], bz = B[2][s + 1];
        const double ex = bx - ax, ey = by - ay, ez = bz - az;
        const double l2 = (ex * ex + ey * ey) + ez * ez;
        if (l2 > 0.0) {
          if (first < 0) first = s;
          last = s;
          const double gx = wx - ax, gy = wy - ay, gz = wz - az;
          const double dot = (gx * ex + gy * ey) + gz * ez;
          double u;                                    // clamp(dot / l2, 0, 1), as fuse_project_kernel
          if (dot <= 0.0) u = 0.0;
          else if (dot >= l2) u = 1.0;
          else u = dot / l2;
          const double cx = ax + u * ex, cy = ay + u * ey, cz = az + u * ez;
          const double hx = wx - cx, hy = wy - cy, hz = wz - cz;
          const double d2 = (hx * hx + hy * hy) + hz * hz;
          if (d2 < best) { best = d2; best_u = u; best_k = s; }
        }
        ax = bx; ay = by; az = bz;
      }
      const bool clamped = best_k < 0 || (best_k == first && best_u == 0.0) || (best_k == last && best_u == 1.0);
      const int slot = dir * M + k;
      int flag = 0;
      if (!clamped) {
        const double d = sqrt(best);
        if (d <= gate) {
          flag = 1;
          const double c0 = B[3][best_k], c1 = B[3][best_k + 1];
          const double sb = c0 + best_u * (c1 - c0), sa = A[3][k];
          const int q = k < M - 2 ? k : M - 2;
          const double eax = A[0][q + 1] - A[0][q], eay = A[1][q + 1] - A[1][q], eaz = A[2][q + 1] - A[2][q];
          const double ebx = B[0][best_k + 1] - B[0][best_k], eby = B[1][best_k + 1] - B[1][best_k],
                       ebz = B[2][best_k + 1] - B[2][best_k];
          sh_val[wave][0][slot] = d;
          sh_val[wave][1][slot] = dir == 0 ? sa : sb;              // the coordinate along i
          sh_val[wave][2][slot] = dir == 0 ? sb : sa;              // the coordinate along j
          sh_val[wave][3][slot] = (eax * ebx + eay * eby) + eaz * ebz;
        } else {
          flag = 2;
        }
      }
      sh_flag[wave][slot] = flag;
    }
  }
  __syncthreads();
  if (!valid) return;
  // the rule's order: i -> j in ascending k, then j -> i; one quantity per lane
  if (lane < 4) {
    double sum = 0.0;
    for (int s = 0; s < 2 * M; ++s)
      if (sh_flag[wave][s] == 1) sum = sum + sh_val[wave][lane][s];
    pair_sum[4 * pair + lane] = sum;
  } else if (lane < 6) {
    const int want = lane - 3;                         // lane 4 counts the ins, lane 5 the outs
    int n = 0;
    for (int s = 0; s < 2 * M; ++s) n += sh_flag[wave][s] == want;
    pair_count[2 * pair + (lane - 4)] = n;
  }
}

}  // namespace prh
