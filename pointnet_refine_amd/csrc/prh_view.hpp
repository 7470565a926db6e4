// 3-D scene views on the GPU: depth-buffered point splats and polylines under orbit cameras, by the
// rule declared in include/pointnet_refine_hip.h ("3-D views - the rule").  The reference's viewers
// (inference_whole_scene.py:242-404, tools/visualize_data.py, check_global_align.py,
// visualize_sampled_pointcloud.py) subsample the cloud for Plotly / matplotlib; here every point is
// drawn in one pass over the cloud.
//   view_bounds_kernel / view_bounds_final   min / max of x, y, z and a non-finite flag, two stages
//   view_clear_kernel    every depth word = all ones (empty)
//   view_splat_kernel    each point loaded once, projected by every camera of the call (rows held
//                        in LDS) in fp64 with one rounding per operation, its k x k pixels written
//                        with a 64-bit unsigned atomicMin of (float32 depth bits << 32 | payload).
//                        A minimum does not depend on arrival order, so the buffer is the same
//                        bits every run.  A plain load first skips the atomic when the pixel already
//                        holds a smaller word (words only shrink, so a stale value can only
//                        over-estimate the pixel).
//   view_lines_kernel    one workgroup per segment walks the segment's bounding box (grown by
//                        max(width, marker) / 2, clipped to the image), tests each pixel centre and
//                        writes the same kind of word with the line's index as payload
//   view_resolve_kernel  word -> RGBA (table / line colour / background) and float32 depth
// No trigonometric function and no square root is evaluated here: the host builds the camera rows
// and the segments' lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_bev.hpp"

namespace prh {

constexpr int VIEW_THREADS = 256;
constexpr int VIEW_BOUNDS_BLOCKS = 2048;
constexpr int VIEW_POINTS_PER_THREAD = 4;
constexpr int VIEW_MAX_VIEWS = 64;           // cameras of one splat call (16 doubles each, in LDS)
constexpr int VIEW_MAX_SPLAT = 9;
constexpr int VIEW_CAM_DOUBLES = 16;         // eye[3] r[3] u[3] f[3] s near ortho 0
constexpr int VIEW_SEG_DOUBLES = 8;          // ax ay bx by (pixels), arc length at a, length, wa, wb
constexpr int VIEW_STYLE_DOUBLES = 8;        // r g b (0..255), width, marker, dash on, dash off (pixels), bias (metres)
constexpr unsigned long long VIEW_EMPTY = ~0ull;
constexpr unsigned VIEW_POINT_FLAG = 0x01000000u;

template <typename T> struct ViewPoint { T x, y, z, i; };
__device__ __forceinline__ ViewPoint<float> view_load(const float* p, long long n) {
  const float4 v = reinterpret_cast<const float4*>(p)[n];
  return {v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ ViewPoint<double> view_load(const double* p, long long n) {
  const double2 a = reinterpret_cast<const double2*>(p)[2 * n], b = reinterpret_cast<const double2*>(p)[2 * n + 1];
  return {a.x, a.y, b.x, b.y};
}

// depth (metres) -> the high half of a depth word: the bits of the float32 depth, negative depths
// (a bias larger than the depth) taken as +0 so that the bits order as unsigned integers
__device__ __forceinline__ unsigned long long view_word(double depth, unsigned payload) {
  const double d = depth > 0.0 ? depth : 0.0;
  return ((unsigned long long)__float_as_uint((float)d) << 32) | payload;
}
__device__ __forceinline__ void view_put(unsigned long long* cell, unsigned long long word) {
  if (*cell > word) atomicMin(cell, word);
}

// partial [VIEW_BOUNDS_BLOCKS][6] (x_min x_max y_min y_max z_min z_max) and bad [VIEW_BOUNDS_BLOCKS]
template <typename T>
__global__ __launch_bounds__(VIEW_THREADS) void view_bounds_kernel(const T* __restrict__ pts, long long n,
                                                                   T* __restrict__ partial, int* __restrict__ bad) {
  __shared__ T red[6][VIEW_THREADS];
  __shared__ int red_bad[VIEW_THREADS];
  T v[6] = {(T)INFINITY, (T)-INFINITY, (T)INFINITY, (T)-INFINITY, (T)INFINITY, (T)-INFINITY};
  int b = 0;
  for (long long i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * VIEW_THREADS) {
    const ViewPoint<T> p = view_load(pts, i);
    b |= !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.i));
    v[0] = p.x < v[0] ? p.x : v[0]; v[1] = p.x > v[1] ? p.x : v[1];
    v[2] = p.y < v[2] ? p.y : v[2]; v[3] = p.y > v[3] ? p.y : v[3];
    v[4] = p.z < v[4] ? p.z : v[4]; v[5] = p.z > v[5] ? p.z : v[5];
  }
  const int t = threadIdx.x;
  for (int c = 0; c < 6; ++c) red[c][t] = v[c];
  red_bad[t] = b;
  __syncthreads();
  for (int s = VIEW_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      for (int c = 0; c < 6; c += 2) {
        red[c][t] = red[c][t + s] < red[c][t] ? red[c][t + s] : red[c][t];
        red[c + 1][t] = red[c + 1][t + s] > red[c + 1][t] ? red[c + 1][t + s] : red[c + 1][t];
      }
      red_bad[t] |= red_bad[t + s];
    }
    __syncthreads();
  }
  if (t < 6) partial[6 * blockIdx.x + t] = red[t][0];
  if (t == 0) bad[blockIdx.x] = red_bad[0];
}

// info [7] fp64: x_min x_max y_min y_max z_min z_max (exact: every T is a double) and 1.0 when a value is not finite
template <typename T>
__global__ __launch_bounds__(VIEW_THREADS) void view_bounds_final(const T* __restrict__ partial,
                                                                  const int* __restrict__ bad, int nblk,
                                                                  double* __restrict__ info) {
  __shared__ T red[6][VIEW_THREADS];
  __shared__ int red_bad[VIEW_THREADS];
  const int t = threadIdx.x;
  T v[6] = {(T)INFINITY, (T)-INFINITY, (T)INFINITY, (T)-INFINITY, (T)INFINITY, (T)-INFINITY};
  int b = 0;
  for (int k = t; k < nblk; k += VIEW_THREADS) {
    const T* p = partial + 6 * k;
    for (int c = 0; c < 6; c += 2) {
      v[c] = p[c] < v[c] ? p[c] : v[c];
      v[c + 1] = p[c + 1] > v[c + 1] ? p[c + 1] : v[c + 1];
    }
    b |= bad[k];
  }
  for (int c = 0; c < 6; ++c) red[c][t] = v[c];
  red_bad[t] = b;
  __syncthreads();
  for (int s = VIEW_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      for (int c = 0; c < 6; c += 2) {
        red[c][t] = red[c][t + s] < red[c][t] ? red[c][t + s] : red[c][t];
        red[c + 1][t] = red[c + 1][t + s] > red[c + 1][t] ? red[c + 1][t + s] : red[c + 1][t];
      }
      red_bad[t] |= red_bad[t + s];
    }
    __syncthreads();
  }
  if (t < 6) info[t] = (double)red[t][0];
  if (t == 0) info[6] = red_bad[0] ? 1.0 : 0.0;
}

__global__ __launch_bounds__(VIEW_THREADS) void view_clear_kernel(unsigned long long* __restrict__ zbuf, long long n) {
  const long long i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (i < n) zbuf[i] = VIEW_EMPTY;
}

// zbuf [V][H][W] depth words.  cams [V][16].  offsets == nullptr: every point goes into every view;
// otherwise point i belongs to slice s (offsets [S+1]) and goes into view v when slice_mask[s * V + v] != 0.
// *bad = 1 on a non-finite x, y, z or intensity.
template <typename T>
__global__ __launch_bounds__(VIEW_THREADS) void view_splat_kernel(const T* __restrict__ pts, long long n,
                                                                  const double* __restrict__ cams, int V,
                                                                  const long long* __restrict__ offsets, int S,
                                                                  const unsigned char* __restrict__ slice_mask,
                                                                  int size, double cmin, double cmax, int H, int W,
                                                                  unsigned long long* __restrict__ zbuf,
                                                                  int* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ double cam[VIEW_MAX_VIEWS * VIEW_CAM_DOUBLES];
  for (int k = threadIdx.x; k < V * VIEW_CAM_DOUBLES; k += VIEW_THREADS) cam[k] = cams[k];
  __syncthreads();
  const double half_w = 0.5 * (double)W, half_h = 0.5 * (double)H;   // exact
  const double range = cmax - cmin;
  const int lo = size / 2;
  const long long first = (long long)blockIdx.x * (VIEW_THREADS * VIEW_POINTS_PER_THREAD) + threadIdx.x;
  for (int it = 0; it < VIEW_POINTS_PER_THREAD; ++it) {
    const long long i = first + (long long)it * VIEW_THREADS;
    if (i >= n) break;
    const ViewPoint<T> pt = view_load(pts, i);
    if (!(isfinite(pt.x) && isfinite(pt.y) && isfinite(pt.z) && isfinite(pt.i))) { *bad = 1; continue; }
    const double px = (double)pt.x, py = (double)pt.y, pz = (double)pt.z;
    double c = ((double)pt.i - cmin) / range;
    c = floor(c * 256.0);
    c = c < 0.0 ? 0.0 : (c > 255.0 ? 255.0 : c);           // clamp, then convert; NaN (cmax == cmin) -> 255
    const unsigned payload = VIEW_POINT_FLAG | (unsigned)(c == c ? (int)c : 255);
    const unsigned char* mask = offsets ? slice_mask + (long long)bev_slice_of(offsets, S, i) * V : nullptr;
    for (int v = 0; v < V; ++v) {
      if (mask && !mask[v]) continue;
      const double* cm = cam + VIEW_CAM_DOUBLES * v;
      const double q0 = px - cm[0], q1 = py - cm[1], q2 = pz - cm[2];
      const double xr = (q0 * cm[3] + q1 * cm[4]) + q2 * cm[5];
      const double yu = (q0 * cm[6] + q1 * cm[7]) + q2 * cm[8];
      const double d = (q0 * cm[9] + q1 * cm[10]) + q2 * cm[11];
      if (!(d >= cm[13])) continue;
      const double k = cm[14] != 0.0 ? cm[12] : cm[12] / d;
      const double X = half_w + xr * k, Y = half_h - yu * k;
      const double fx = floor(X), fy = floor(Y);
      // the splat reaches [f - lo, f - lo + size - 1]; this also drops NaN and keeps the int conversion in range
      if (!(fx >= -(double)VIEW_MAX_SPLAT && fx < (double)(W + VIEW_MAX_SPLAT) && fy >= -(double)VIEW_MAX_SPLAT &&
            fy < (double)(H + VIEW_MAX_SPLAT)))
        continue;
      const int u0 = (int)fx - lo, v0 = (int)fy - lo;
      const unsigned long long word = view_word(d, payload);
      unsigned long long* img = zbuf + (long long)v * H * W;
      for (int a = 0; a < size; ++a) {
        const int row = v0 + a;
        if (row < 0 || row >= H) continue;
        for (int b = 0; b < size; ++b) {
          const int col = u0 + b;
          if (col < 0 || col >= W) continue;
          view_put(img + (long long)row * W + col, word);
        }
      }
    }
  }
}

// seg [n][8], seg_id [n][2] = line, view (a pair out of range is skipped); style [n_lines][8]; cams [V][16]
// (only the ortho flag is read)
__global__ __launch_bounds__(VIEW_THREADS) void view_lines_kernel(const double* __restrict__ seg,
                                                                  const int* __restrict__ seg_id,
                                                                  const double* __restrict__ style, int n_lines,
                                                                  const double* __restrict__ cams, int V, int H, int W,
                                                                  unsigned long long* __restrict__ zbuf) {
#pragma clang fp contract(off)
  const long long e = blockIdx.x;
  const double* g = seg + VIEW_SEG_DOUBLES * e;
  const int line = seg_id[2 * e], view = seg_id[2 * e + 1];
  if (line < 0 || line >= n_lines || view < 0 || view >= V) return;
  const double* st = style + (long long)VIEW_STYLE_DOUBLES * line;
  const double width = st[3], marker = st[4], on = st[5], off = st[6], bias = st[7];
  const bool ortho = cams[(long long)VIEW_CAM_DOUBLES * view + 14] != 0.0;
  const double ax = g[0], ay = g[1], bx = g[2], by = g[3], arc = g[4], len = g[5], wa = g[6], wb = g[7];
  const double r = 0.5 * (width > marker ? width : marker);
  if (!(r > 0.0)) return;
  const double lo_x = fmin(ax, bx) - r, hi_x = fmax(ax, bx) + r;
  const double lo_y = fmin(ay, by) - r, hi_y = fmax(ay, by) + r;
  if (!(hi_x > 0.0 && lo_x < (double)W && hi_y > 0.0 && lo_y < (double)H)) return;    // also drops NaN
  // pixel centres are at half-integers: column u can be covered when lo_x <= u + 0.5 <= hi_x
  const int u0 = (int)fmax(floor(lo_x - 0.5), 0.0), u1 = (int)fmin(ceil(hi_x - 0.5), (double)(W - 1));
  const int v0 = (int)fmax(floor(lo_y - 0.5), 0.0), v1 = (int)fmin(ceil(hi_y - 0.5), (double)(H - 1));
  if (u1 < u0 || v1 < v0) return;
  const int bw = u1 - u0 + 1;
  const long long cells = (long long)bw * (v1 - v0 + 1);
  const double ex = bx - ax, ey = by - ay;
  const double len2 = ex * ex + ey * ey;
  const double hw = 0.5 * width, hm = 0.5 * marker;
  const double hw2 = hw * hw, hm2 = hm * hm;
  const double da = ortho ? wa : 1.0 / wa, db = ortho ? wb : 1.0 / wb;
  unsigned long long* img = zbuf + (long long)view * H * W;
  for (long long c = threadIdx.x; c < cells; c += VIEW_THREADS) {
    const int row = v0 + (int)(c / bw), col = u0 + (int)(c % bw);
    const double cx = col + 0.5, cy = row + 0.5;
    double depth = INFINITY;
    bool hit = false;
    if (width > 0.0) {
      double t = 0.0;
      if (len2 > 0.0) {
        t = ((cx - ax) * ex + (cy - ay) * ey) / len2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
      }
      const double nx = ax + t * ex, ny = ay + t * ey;
      const double dx = cx - nx, dy = cy - ny;
      if (dx * dx + dy * dy <= hw2) {
        bool lit = true;
        if (off > 0.0) {
          const double s = arc + t * len;
          if (fmod(s, on + off) >= on) lit = false;
        }
        if (lit) {
          const double w = (1.0 - t) * wa + t * wb;
          depth = ortho ? w : 1.0 / w;
          hit = true;
        }
      }
    }
    if (marker > 0.0) {
      const double pax = cx - ax, pay = cy - ay, pbx = cx - bx, pby = cy - by;
      if (pax * pax + pay * pay <= hm2) { depth = (!hit || da < depth) ? da : depth; hit = true; }
      if (pbx * pbx + pby * pby <= hm2) { depth = (!hit || db < depth) ? db : depth; hit = true; }
    }
    if (!hit || !(depth == depth)) continue;
    view_put(img + (long long)row * W + col, view_word(depth - bias, (unsigned)line));
  }
}

// table [256] and line_colour [n_lines] packed RGBA (R in the low byte); a line index past n_lines shows the background
__global__ __launch_bounds__(VIEW_THREADS) void view_resolve_kernel(const unsigned long long* __restrict__ zbuf, long long n,
                                                                    const unsigned* __restrict__ table,
                                                                    const unsigned* __restrict__ line_colour,
                                                                    int n_lines, unsigned background,
                                                                    unsigned* __restrict__ rgba,
                                                                    float* __restrict__ depth) {
  const long long i = (long long)blockIdx.x * VIEW_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long w = zbuf[i];
  unsigned c = background;
  float d = INFINITY;
  if (w != VIEW_EMPTY) {
    const unsigned payload = (unsigned)w;
    d = __uint_as_float((unsigned)(w >> 32));
    if (payload & VIEW_POINT_FLAG) c = table[payload & 255u];
    else if (payload < (unsigned)n_lines) c = line_colour[payload];
  }
  rgba[i] = c | 0xff000000u;
  depth[i] = d;
}

}  // namespace prh
