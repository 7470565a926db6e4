// Scene evaluation on the GPU: the metric half of the reference's whole-scene script
// (inference_whole_scene.py:26-92,170-193,299-387), scipy KDTree code there, brute force here.
//   met_line_kernel   one wave per (item, candidate) line: crop_gt_to_pred_range (:26-70), the
//                     crop resampled to M points (src/dataset.py:8-29), ADE against that
//                     resample, Chamfer and "Lat" (mean pred->GT nearest distance) against the
//                     raw crop vertices (compute_chamfer_distance, :72-92), for the noisy and the
//                     refined line
//   met_sweep_kernel  calibrate_alignment's inner loop (:170-193) for S shifts in one launch:
//                     per-block partial sums of min_g |pred_p + (dx_s,dy_s,0) - gt_g| over the
//                     block's queries; met_sweep_reduce_kernel adds them in a fixed order
//   met_sweep_ragged_kernel   many such sweeps in one launch: a flat grid of (problem, query tile,
//                     shift tile) items over CSR buffers; it and met_sweep_kernel both drive
//                     met_sweep_block / met_sweep_mean, so a problem gets the same bytes either way
// All arithmetic is fp64 with FMA contraction off, and every distance is
// sqrt((dx*dx + dy*dy) + dz*dz), the order np.linalg.norm(axis=1) uses: scene coordinates can be
// UTM-sized (1e5..1e6 m), where fp32 - or the |q|^2 + |r|^2 - 2 q.r expansion - loses the
// centimetres being measured.  Argmin ties resolve to the first index, as np.argmin does.
// No atomics: every result is bitwise reproducible from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prh {

constexpr int MET_MAX_M = 128;       // points per resampled line
constexpr int MET_CHUNK = 128;       // crop vertices staged in LDS at a time
constexpr int SW_THREADS = 256;      // queries per sweep block (one per thread)
constexpr int SW_SB = 16;            // shifts per sweep block (a register block per thread)
constexpr int SW_TILE = 512;         // GT points staged in LDS per sweep step

__device__ __forceinline__ double met_d2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double met_wave_sum(double v) {     // butterfly: every lane ends with the same sum
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// lexicographic (distance, index) minimum over the wave: the first index wins a tie
__device__ __forceinline__ void met_wave_argmin(double& d, int& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const int oi = __shfl_xor(i, o);
    if (od < d || (od == d && oi < i)) { d = od; i = oi; }
  }
}

// One 64-lane block per line.
//   noisy, refined [L,M,3]; gt [*,3] with CSR offsets gt_off [n_gt+1]; gt_index [L] (-1: none)
//   info [L,4] = crop_start, crop_end, reversed, valid; resampled [L,M,3]; metrics [L,6] =
//   ade_noisy, ade_refined, cd_noisy, cd_refined, lat_noisy, lat_refined
// Lines without a usable GT (index -1 or fewer than 2 vertices) get info {-1,-1,0,0}, a zero
// resample and NaN metrics.
__global__ __launch_bounds__(64) void met_line_kernel(const double* __restrict__ noisy,
                                                      const double* __restrict__ refined, int M,
                                                      const double* __restrict__ gt,
                                                      const long long* __restrict__ gt_off, int n_gt,
                                                      const int* __restrict__ gt_index, int* __restrict__ info,
                                                      double* __restrict__ resampled,
                                                      double* __restrict__ metrics) {
#pragma clang fp contract(off)
  __shared__ double sp[2][3 * MET_MAX_M];            // noisy, refined
  __shared__ double sc[3][MET_CHUNK];                // crop vertices, SoA, in crop order
  const int line = blockIdx.x, lane = threadIdx.x;
  const size_t lbase = (size_t)line * M * 3;
  for (int i = lane; i < 3 * M; i += 64) {
    sp[0][i] = noisy[lbase + i];
    sp[1][i] = refined[lbase + i];
  }
  const int g = gt_index[line];
  const long long n = (g >= 0 && g < n_gt) ? gt_off[g + 1] - gt_off[g] : 0;
  if (n < 2) {
    for (int i = lane; i < 3 * M; i += 64) resampled[lbase + i] = 0.0;
    if (lane < 6) metrics[(size_t)line * 6 + lane] = __builtin_nan("");
    if (lane < 4) info[(size_t)line * 4 + lane] = lane < 2 ? -1 : 0;
    return;
  }
  __syncthreads();
  const double* v = gt + 3 * gt_off[g];
  // 1. nearest GT vertex to the line's first and last point
  const double psx = sp[0][0], psy = sp[0][1], psz = sp[0][2];
  const double pex = sp[0][3 * (M - 1)], pey = sp[0][3 * (M - 1) + 1], pez = sp[0][3 * (M - 1) + 2];
  double ds = __builtin_inf(), de = __builtin_inf();
  int is = 0x7fffffff, ie = 0x7fffffff;
  for (long long j = lane; j < n; j += 64) {
    const double x = v[3 * j], y = v[3 * j + 1], z = v[3 * j + 2];
    const double a = sqrt(met_d2(x, y, z, psx, psy, psz)), b = sqrt(met_d2(x, y, z, pex, pey, pez));
    if (a < ds) { ds = a; is = (int)j; }
    if (b < de) { de = b; ie = (int)j; }
  }
  met_wave_argmin(ds, is);
  met_wave_argmin(de, ie);
  // 2. crop range, widened around a single index
  int i0 = is < ie ? is : ie, i1 = is < ie ? ie : is;
  if (i0 == i1) {
    i0 = i0 - 1 > 0 ? i0 - 1 : 0;
    i1 = i1 + 1 < (int)n - 1 ? i1 + 1 : (int)n - 1;
  }
  // 3. direction: reverse the crop if that matches the line's ends strictly better
  const double* c0 = v + 3 * (size_t)i0;
  const double* c1 = v + 3 * (size_t)i1;
  const double dn = sqrt(met_d2(c0[0], c0[1], c0[2], psx, psy, psz)) + sqrt(met_d2(c1[0], c1[1], c1[2], pex, pey, pez));
  const double dr = sqrt(met_d2(c0[0], c0[1], c0[2], pex, pey, pez)) + sqrt(met_d2(c1[0], c1[1], c1[2], psx, psy, psz));
  const bool rev = dr < dn;
  const int K = i1 - i0 + 1;
  auto vtx = [&](int k) -> const double* { return v + 3 * (size_t)(rev ? i1 - k : i0 + k); };
  auto stage = [&](int k0, int cnt) {
    __syncthreads();
    for (int k = lane; k < cnt; k += 64) {
      const double* p = vtx(k0 + k);
      sc[0][k] = p[0]; sc[1][k] = p[1]; sc[2][k] = p[2];
    }
    __syncthreads();
  };
  // pass 1 over the crop: arc length (sequential, as np.cumsum) and the Chamfer minima.
  // Lane owns line points lane and lane + 64 (M <= 128) of both lines, and crop vertices k0 + lane, k0 + lane + 64.
  const int nq = (lane < M) + (lane + 64 < M);
  double qmin[2][2] = {{__builtin_inf(), __builtin_inf()}, {__builtin_inf(), __builtin_inf()}};
  double g2p[2] = {0.0, 0.0};
  double total = 0.0, px = 0.0, py = 0.0, pz = 0.0;
  for (int k0 = 0; k0 < K; k0 += MET_CHUNK) {
    const int cnt = K - k0 < MET_CHUNK ? K - k0 : MET_CHUNK;
    stage(k0, cnt);
    for (int k = 0; k < cnt; ++k) {
      const double x = sc[0][k], y = sc[1][k], z = sc[2][k];
      if (k0 + k > 0) total = total + sqrt(met_d2(x, y, z, px, py, pz));
      px = x; py = y; pz = z;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (h < nq) {
            const double* q = &sp[t][3 * (lane + 64 * h)];
            qmin[t][h] = fmin(qmin[t][h], met_d2(q[0], q[1], q[2], x, y, z));
          }
    }
    for (int k = lane; k < cnt; k += 64) {
      const double x = sc[0][k], y = sc[1][k], z = sc[2][k];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double b = __builtin_inf();
        for (int i = 0; i < M; ++i) b = fmin(b, met_d2(x, y, z, sp[t][3 * i], sp[t][3 * i + 1], sp[t][3 * i + 2]));
        g2p[t] += sqrt(b);
      }
    }
  }
  // pass 2: np.linspace(0, total, M) and np.interp over the crop's cumulative arc length
  const double step = total / (double)(M - 1);
  double tq[2] = {0.0, 0.0}, cj[2] = {0.0, 0.0}, cj1[2] = {0.0, 0.0};
  int jq[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = lane + 64 * h;
    if (i >= M) break;
    tq[h] = step == 0.0 ? ((double)i / (double)(M - 1)) * total : (double)i * step + 0.0;
    if (i == M - 1) tq[h] = total;
  }
  double cum = 0.0;
  for (int k0 = 0; k0 < K; k0 += MET_CHUNK) {
    const int cnt = K - k0 < MET_CHUNK ? K - k0 : MET_CHUNK;
    stage(k0, cnt);
    for (int k = 0; k < cnt; ++k) {
      const double x = sc[0][k], y = sc[1][k], z = sc[2][k];
      if (k0 + k > 0) cum = cum + sqrt(met_d2(x, y, z, px, py, pz));
      px = x; py = y; pz = z;
#pragma unroll
      for (int h = 0; h < 2; ++h) {                // rightmost knot <= t, and the knot after it
        if (h >= nq) break;
        if (cum <= tq[h]) { jq[h] = k0 + k; cj[h] = cum; }
        else if (k0 + k == jq[h] + 1) cj1[h] = cum;
      }
    }
  }
  double ade[2] = {0.0, 0.0};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h >= nq) break;
    const int i = lane + 64 * h, j = jq[h];
    const double* a = vtx(j);
    double r[3];
    if (j == K - 1 || cj[h] == tq[h]) {
      r[0] = a[0]; r[1] = a[1]; r[2] = a[2];
    } else {
      const double* b = vtx(j + 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double slope = (b[c] - a[c]) / (cj1[h] - cj[h]);
        double y = slope * (tq[h] - cj[h]) + a[c];
        if (__builtin_isnan(y)) {
          y = slope * (tq[h] - cj1[h]) + b[c];
          if (__builtin_isnan(y) && a[c] == b[c]) y = a[c];
        }
        r[c] = y;
      }
    }
    for (int c = 0; c < 3; ++c) resampled[lbase + 3 * i + c] = r[c];
    for (int t = 0; t < 2; ++t)
      ade[t] += sqrt(met_d2(sp[t][3 * i], sp[t][3 * i + 1], sp[t][3 * i + 2], r[0], r[1], r[2]));
  }
  double p2g[2] = {0.0, 0.0};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (h < nq) p2g[t] += sqrt(qmin[t][h]);
  double* mo = metrics + (size_t)line * 6;
  for (int t = 0; t < 2; ++t) {
    const double a = met_wave_sum(ade[t]) / (double)M;
    const double lat = met_wave_sum(p2g[t]) / (double)M;
    const double back = met_wave_sum(g2p[t]) / (double)K;
    if (lane == 0) { mo[t] = a; mo[2 + t] = lat + back; mo[4 + t] = lat; }
  }
  if (lane == 0) {
    int* io = info + (size_t)line * 4;
    io[0] = i0; io[1] = i1; io[2] = rev ? 1 : 0; io[3] = 1;
  }
}

// Sweep block (qt, st) of one problem: queries qt*256 + tid against shifts st*16 .. st*16+15, every
// GT point.  partial[s * n_qt + qt] = sum over the block's queries of sqrt(min_g d^2), in a fixed
// order.  The shifted query is formed first (pred + (dx,dy,0)), as the reference does before its
// KDTree query.  pred / gt / shifts / partial point at the problem's own first point, shift and
// partial, so the per-problem and the ragged kernels hand a block the same operands in the same
// order: their results are the same bytes.
__device__ __forceinline__ void met_sweep_block(const double* __restrict__ pred, int P,
                                                const double* __restrict__ gt, int G,
                                                const double* __restrict__ shifts, int S,
                                                double* __restrict__ partial, int n_qt, int qt, int st) {
#pragma clang fp contract(off)
  __shared__ double gx[SW_TILE], gy[SW_TILE], gz[SW_TILE];
  __shared__ double red[SW_SB][SW_THREADS / 64];
  const int tid = threadIdx.x, q = qt * SW_THREADS + tid, s0 = st * SW_SB;
  const bool live = q < P;
  const int qc = live ? q : P - 1;
  const double px = pred[3 * (size_t)qc], py = pred[3 * (size_t)qc + 1], qz = pred[3 * (size_t)qc + 2] + 0.0;
  double qx[SW_SB], qy[SW_SB], best[SW_SB];
#pragma unroll
  for (int s = 0; s < SW_SB; ++s) {
    const int sc = s0 + s < S ? s0 + s : S - 1;
    qx[s] = px + shifts[2 * (size_t)sc];
    qy[s] = py + shifts[2 * (size_t)sc + 1];
    best[s] = __builtin_inf();
  }
  for (int t0 = 0; t0 < G; t0 += SW_TILE) {
    const int cnt = G - t0 < SW_TILE ? G - t0 : SW_TILE;
    __syncthreads();
    for (int i = tid; i < cnt; i += SW_THREADS) {
      const double* p = gt + 3 * (size_t)(t0 + i);
      gx[i] = p[0]; gy[i] = p[1]; gz[i] = p[2];
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < cnt; ++j) {
      const double x = gx[j], y = gy[j], dz = qz - gz[j];
      const double dz2 = dz * dz;
#pragma unroll
      for (int s = 0; s < SW_SB; ++s) {
        const double dx = qx[s] - x, dy = qy[s] - y;
        best[s] = fmin(best[s], (dx * dx + dy * dy) + dz2);
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 0; s < SW_SB; ++s) {
    const double w = met_wave_sum(live ? sqrt(best[s]) : 0.0);
    if (lane == 0) red[s][wave] = w;
  }
  __syncthreads();
  if (tid < SW_SB && s0 + tid < S)
    partial[(size_t)(s0 + tid) * n_qt + qt] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// (sum of shift s's block partials, in block order) / P
__device__ __forceinline__ double met_sweep_mean(const double* __restrict__ partial, int n_qt, int s, int P) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int b = 0; b < n_qt; ++b) acc += partial[(size_t)s * n_qt + b];
  return acc / (double)P;
}

// One problem: grid (n_qt, ceil(S/16)).
__global__ __launch_bounds__(SW_THREADS) void met_sweep_kernel(const double* __restrict__ pred, int P,
                                                               const double* __restrict__ gt, int G,
                                                               const double* __restrict__ shifts, int S,
                                                               double* __restrict__ partial, int n_qt) {
  met_sweep_block(pred, P, gt, G, shifts, S, partial, n_qt, (int)blockIdx.x, (int)blockIdx.y);
}

// out[s] = (sum of the shift's block partials, in block order) / P
__global__ __launch_bounds__(256) void met_sweep_reduce_kernel(const double* __restrict__ partial, int n_qt, int S,
                                                               int P, double* __restrict__ out) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  out[s] = met_sweep_mean(partial, n_qt, s, P);
}

// ---- ragged sweep: many independent problems in one launch pair
// Problem p: predictions pred[pred0 .. pred0+P), GT points gt[gt0 .. gt0+G), shifts and outputs
// [sh0 .. sh0+S), block partials partial[part0 .. part0 + n_qt*S) - rows of the flat buffers.
struct MetSweepProblem {
  long long pred0, gt0, sh0, part0;
  int P, G, S, n_qt;
};

// The last entry of offsets[lo..hi) that is <= at (offsets strictly increase: no problem is empty)
__device__ __forceinline__ int met_find(const long long* __restrict__ offsets, int lo, int hi, long long at) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= at) lo = mid; else hi = mid;
  }
  return lo;
}

// Flat 1-D grid of (problem, query tile, shift tile) work items.  item_offsets (n+1): exclusive scan
// of n_qt_p * ceil(S_p/16); within a problem the query tile runs fastest.
__global__ __launch_bounds__(SW_THREADS) void met_sweep_ragged_kernel(const double* __restrict__ pred,
                                                                      const double* __restrict__ gt,
                                                                      const double* __restrict__ shifts,
                                                                      const MetSweepProblem* __restrict__ prob,
                                                                      const long long* __restrict__ item_offsets,
                                                                      int n_problems, double* __restrict__ partial) {
  const long long item = (long long)blockIdx.x;
  const int p = met_find(item_offsets, 0, n_problems, item);
  const MetSweepProblem pr = prob[p];
  const long long r = item - item_offsets[p];
  const int st = (int)(r / pr.n_qt), qt = (int)(r - (long long)st * pr.n_qt);
  met_sweep_block(pred + 3 * (size_t)pr.pred0, pr.P, gt + 3 * (size_t)pr.gt0, pr.G, shifts + 2 * (size_t)pr.sh0, pr.S,
                  partial + (size_t)pr.part0, pr.n_qt, qt, st);
}

// One thread per (problem, shift) of the flat shift buffer; shift_offsets (n+1) finds the problem.
__global__ __launch_bounds__(256) void met_sweep_ragged_reduce_kernel(const double* __restrict__ partial,
                                                                      const MetSweepProblem* __restrict__ prob,
                                                                      const long long* __restrict__ shift_offsets,
                                                                      int n_problems, long long total_shifts,
                                                                      double* __restrict__ out) {
  const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
  if (at >= total_shifts) return;
  const int p = met_find(shift_offsets, 0, n_problems, at);
  const MetSweepProblem pr = prob[p];
  out[at] = met_sweep_mean(partial + (size_t)pr.part0, pr.n_qt, (int)(at - pr.sh0), pr.P);
}

}  // namespace prh
