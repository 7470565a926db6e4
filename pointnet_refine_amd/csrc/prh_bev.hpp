// Bird's-eye-view rendering on the GPU: the reference's tools/vis_inference_bev.py (:74-104 the
// intensity image, :142-151 tone map and colours) and the overlay rule of this project (declared in
// include/pointnet_refine_hip.h).
//   bev_bounds_kernel / bev_bounds_final   min / max of x and y and a non-finite flag, two stages
//   bev_raster_kernel    one thread per point: u, v as numpy computes them (one rounding per
//                        operation, in the input's dtype), then an integer atomicMax of an
//                        order-preserving key of the float32 intensity.  A maximum does not depend
//                        on arrival order, so the image is the same bits every run; key 0 is no
//                        finite float's key and marks an empty pixel.  A plain load first skips the
//                        atomic when the pixel already holds a larger key (keys only grow, so a
//                        stale value can only under-estimate the pixel).
//   bev_finalize_kernel  key -> float32 in place, empty -> 0.0
//   bev_hist_kernel / bev_pick_kernel   radix select (4 passes of 8 bits over the float bits of the
//                        positive pixels) of the two order statistics numpy's linear percentile
//                        interpolates between; integer counts only
//   bev_tone_kernel      clip(image / p, 0, 1) ** gamma in float32
//   bev_colorize_kernel  256-entry table lookup, opaque black where image == 0
//   bev_crop_kernel      integer-shifted copies of the scene image into packed views
//   bev_bin_kernel<FILL> segments -> the 16 x 16 pixel tiles their padded bounding boxes touch
//                        (count, then fill through a cursor)
//   bev_draw_kernel      one workgroup per tile, one thread per pixel: the tile's segments put in
//                        line order (rank sort: the fill order is not fixed, the sorted list is),
//                        coverage = max over a line's segments, lines composited in order in fp64,
//                        one rounding at the end.  Pixels no line covers are not written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prh {

constexpr int BEV_THREADS = 256;
constexpr int BEV_BOUNDS_BLOCKS = 2048;
constexpr int BEV_TILE = 16;                 // tile side in pixels; BEV_TILE^2 == BEV_THREADS
constexpr int BEV_SEG_DOUBLES = 5;           // ax ay bx by (pixels), arc length at a (pixels)
constexpr int BEV_STYLE_DOUBLES = 7;         // r g b (0..255), opacity, width, dash on, dash off (pixels)

__device__ __forceinline__ unsigned bev_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float bev_unkey(unsigned k) {
  return k == 0u ? 0.0f : __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <typename T> struct BevPoint { T x, y, i; };
__device__ __forceinline__ BevPoint<float> bev_load(const float* p, long long n) {
  const float4 v = reinterpret_cast<const float4*>(p)[n];
  return {v.x, v.y, v.w};
}
__device__ __forceinline__ BevPoint<double> bev_load(const double* p, long long n) {
  const double2 a = reinterpret_cast<const double2*>(p)[2 * n], b = reinterpret_cast<const double2*>(p)[2 * n + 1];
  return {a.x, a.y, b.y};
}

// partial [BEV_BOUNDS_BLOCKS][4] (x_min x_max y_min y_max) and bad [BEV_BOUNDS_BLOCKS]
template <typename T>
__global__ __launch_bounds__(BEV_THREADS) void bev_bounds_kernel(const T* __restrict__ pts, long long n,
                                                                 T* __restrict__ partial, int* __restrict__ bad) {
  __shared__ T red[4][BEV_THREADS];
  __shared__ int red_bad[BEV_THREADS];
  T lo_x = INFINITY, hi_x = -INFINITY, lo_y = INFINITY, hi_y = -INFINITY;
  int b = 0;
  for (long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BEV_THREADS) {
    const BevPoint<T> p = bev_load(pts, i);
    b |= !(isfinite(p.x) && isfinite(p.y) && isfinite(p.i));
    lo_x = p.x < lo_x ? p.x : lo_x; hi_x = p.x > hi_x ? p.x : hi_x;
    lo_y = p.y < lo_y ? p.y : lo_y; hi_y = p.y > hi_y ? p.y : hi_y;
  }
  const int t = threadIdx.x;
  red[0][t] = lo_x; red[1][t] = hi_x; red[2][t] = lo_y; red[3][t] = hi_y; red_bad[t] = b;
  __syncthreads();
  for (int s = BEV_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] = red[0][t + s] < red[0][t] ? red[0][t + s] : red[0][t];
      red[1][t] = red[1][t + s] > red[1][t] ? red[1][t + s] : red[1][t];
      red[2][t] = red[2][t + s] < red[2][t] ? red[2][t + s] : red[2][t];
      red[3][t] = red[3][t + s] > red[3][t] ? red[3][t + s] : red[3][t];
      red_bad[t] |= red_bad[t + s];
    }
    __syncthreads();
  }
  if (t < 4) partial[4 * blockIdx.x + t] = red[t][0];
  if (t == 0) bad[blockIdx.x] = red_bad[0];
}

// info [5] fp64: x_min x_max y_min y_max (exact: every T is a double) and 1.0 when a value is not finite
template <typename T>
__global__ __launch_bounds__(BEV_THREADS) void bev_bounds_final(const T* __restrict__ partial,
                                                                const int* __restrict__ bad, int nblk,
                                                                double* __restrict__ info) {
  __shared__ T red[4][BEV_THREADS];
  __shared__ int red_bad[BEV_THREADS];
  const int t = threadIdx.x;
  T v[4] = {(T)INFINITY, (T)-INFINITY, (T)INFINITY, (T)-INFINITY};
  int b = 0;
  for (int k = t; k < nblk; k += BEV_THREADS) {
    const T* p = partial + 4 * k;
    v[0] = p[0] < v[0] ? p[0] : v[0]; v[1] = p[1] > v[1] ? p[1] : v[1];
    v[2] = p[2] < v[2] ? p[2] : v[2]; v[3] = p[3] > v[3] ? p[3] : v[3];
    b |= bad[k];
  }
  for (int c = 0; c < 4; ++c) red[c][t] = v[c];
  red_bad[t] = b;
  __syncthreads();
  for (int s = BEV_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] = red[0][t + s] < red[0][t] ? red[0][t + s] : red[0][t];
      red[1][t] = red[1][t + s] > red[1][t] ? red[1][t + s] : red[1][t];
      red[2][t] = red[2][t + s] < red[2][t] ? red[2][t + s] : red[2][t];
      red[3][t] = red[3][t + s] > red[3][t] ? red[3][t + s] : red[3][t];
      red_bad[t] |= red_bad[t + s];
    }
    __syncthreads();
  }
  if (t < 4) info[t] = (double)red[t][0];
  if (t == 0) info[4] = red_bad[0] ? 1.0 : 0.0;
}

// the slice of point i: the last s with offsets[s] <= i (empty slices are stepped over)
__device__ __forceinline__ int bev_slice_of(const long long* __restrict__ offsets, int S, long long i) {
  int lo = 0, hi = S;                      // invariant: offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// keys [S][H][W], zeroed by the caller.  offsets == nullptr: one slice.  *bad = 1 on a non-finite value.
template <typename T>
__global__ __launch_bounds__(BEV_THREADS) void bev_raster_kernel(const T* __restrict__ pts,
                                                                 const long long* __restrict__ offsets, int S,
                                                                 long long n, T y_min, T x_max, T res, int H, int W,
                                                                 unsigned* __restrict__ keys, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (i >= n) return;
  const BevPoint<T> p = bev_load(pts, i);
  if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.i))) { *bad = 1; return; }
  const T dy = p.y - y_min, dx = x_max - p.x;        // one rounding each, then one per division
  const T qu = dy / res, qv = dx / res;
  const int u = (int)qu, v = (int)qv;                // toward zero; out of range saturates and is dropped below
  if (u < 0 || u >= W || v < 0 || v >= H) return;
  const int s = offsets ? bev_slice_of(offsets, S, i) : 0;
  unsigned* cell = keys + ((long long)s * H + v) * W + u;
  const unsigned key = bev_key((float)p.i);
  if (*cell < key) atomicMax(cell, key);
}

__global__ __launch_bounds__(BEV_THREADS) void bev_finalize_kernel(unsigned* __restrict__ keys, long long n) {
  const long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (i < n) reinterpret_cast<float*>(keys)[i] = bev_unkey(keys[i]);
}

// ---- percentile: radix select of two ranks per slice
struct BevSel {
  unsigned long long m;        // positive pixels
  unsigned long long k[2];     // rank still to find inside the current prefix
  unsigned prefix[2];          // bits fixed so far
  double gamma;                // numpy's interpolation weight
};
// hist [S][2][256]; pass p fixes bits [24 - 8p, 32 - 8p)
__global__ __launch_bounds__(BEV_THREADS) void bev_hist_kernel(const float* __restrict__ img, long long npix, int pass,
                                                               const BevSel* __restrict__ sel,
                                                               unsigned* __restrict__ hist) {
  __shared__ unsigned h[2][256];
  const int s = blockIdx.y, t = threadIdx.x;
  h[0][t] = 0; h[1][t] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const unsigned p0 = sel[s].prefix[0], p1 = sel[s].prefix[1];
  const float* src = img + (long long)s * npix;
  for (long long i = (long long)blockIdx.x * BEV_THREADS + t; i < npix; i += (long long)gridDim.x * BEV_THREADS) {
    const float f = src[i];
    if (!(f > 0.0f)) continue;
    const unsigned b = __float_as_uint(f);
    const unsigned bucket = (b >> shift) & 255u;
    if (pass == 0) { atomicAdd(&h[0][bucket], 1u); atomicAdd(&h[1][bucket], 1u); continue; }
    const unsigned hi = b >> (shift + 8);
    if (hi == (p0 >> (shift + 8))) atomicAdd(&h[0][bucket], 1u);
    if (hi == (p1 >> (shift + 8))) atomicAdd(&h[1][bucket], 1u);
  }
  __syncthreads();
  unsigned* g = hist + (long long)s * 512;
  if (h[0][t]) atomicAdd(&g[t], h[0][t]);
  if (h[1][t]) atomicAdd(&g[256 + t], h[1][t]);
}
// one thread per (slice, rank): walk the 256 counts, fix the next 8 bits, clear the counts
__global__ __launch_bounds__(64) void bev_pick_kernel(BevSel* __restrict__ sel, unsigned* __restrict__ hist, int S,
                                                      int pass, float quantile, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= 2 * S) return;
  const int s = id >> 1, r = id & 1;
  unsigned* h = hist + (long long)s * 512 + 256 * r;
  BevSel* q = sel + s;
  unsigned long long k;
  if (pass == 0) {
    unsigned long long m = 0;
    for (int b = 0; b < 256; ++b) m += h[b];
    double gamma = 0.0;
    unsigned long long lo = 0, hi = 0;
    if (m > 0) {
      const float top = (float)(m - 1);
      const float vi = top * quantile;                     // numpy: (n - 1) * q, in the image's dtype
      if (vi >= top) { lo = hi = m - 1; }
      else if (vi < 0.0f) { lo = hi = 0; }
      else { lo = (unsigned long long)floorf(vi); hi = lo + 1; gamma = (double)(vi - floorf(vi)); }
    }
    k = r ? hi : lo;
    if (r == 0) { q->m = m; q->gamma = gamma; }
    q->prefix[r] = 0;
    if (m == 0) { q->k[r] = 0; for (int b = 0; b < 256; ++b) h[b] = 0; return; }
  } else {
    k = q->k[r];
    if (q->m == 0) return;
  }
  unsigned long long c = 0;
  int pick = 255;
  for (int b = 0; b < 256; ++b) {
    if (c + h[b] > k) { pick = b; break; }
    c += h[b];
  }
  for (int b = 0; b < 256; ++b) h[b] = 0;
  q->k[r] = k - c;
  q->prefix[r] |= (unsigned)pick << (24 - 8 * pass);
  if (pass == 3) {
    out[4 * s + 1 + r] = (double)__uint_as_float(q->prefix[r]);
    if (r == 0) { out[4 * s] = (double)q->m; out[4 * s + 3] = q->gamma; }
  }
}

// out = p[s] > 0 ? clip(img / p[s], 0, 1) ** gamma : img
__global__ __launch_bounds__(BEV_THREADS) void bev_tone_kernel(const float* __restrict__ img, long long npix,
                                                               const float* __restrict__ p, float gamma,
                                                               float* __restrict__ out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (i >= npix) return;
  const int s = blockIdx.y;
  const float ps = p[s], f = img[(long long)s * npix + i];
  float r = f;
  if (ps > 0.0f) {
    float q = f / ps;
    q = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
    r = powf(q, gamma);
  }
  out[(long long)s * npix + i] = r;
}

// lut [256] packed RGBA (R in the low byte); out packed the same way
__global__ __launch_bounds__(BEV_THREADS) void bev_colorize_kernel(const float* __restrict__ norm,
                                                                   const float* __restrict__ img, long long n,
                                                                   const unsigned* __restrict__ lut,
                                                                   unsigned* __restrict__ out) {
  const long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (i >= n) return;
  unsigned c = 0xff000000u;
  if (img[i] != 0.0f) {
    const float x = norm[i] * 256.0f;
    int k = x < 0.0f ? 0 : (x >= 256.0f ? 255 : (int)x);      // 1.0 -> 256 -> 255; NaN -> 0
    c = lut[k];
  }
  out[i] = c;
}

// view k: out + pix_off[k], (H_k, W_k) = view[4k+2], view[4k+3], source pixel of (v, u) = (v + view[4k+1], u + view[4k])
__global__ __launch_bounds__(BEV_THREADS) void bev_crop_kernel(const unsigned* __restrict__ src, int Hs, int Ws,
                                                               const int* __restrict__ view,
                                                               const long long* __restrict__ pix_off, int nv,
                                                               long long total, unsigned* __restrict__ out) {
  const long long i = (long long)blockIdx.x * BEV_THREADS + threadIdx.x;
  if (i >= total) return;
  const int k = bev_slice_of(pix_off, nv, i);
  const long long loc = i - pix_off[k];
  const int W = view[4 * k + 3];
  const int v = (int)(loc / W), u = (int)(loc - (long long)v * W);
  const long long sv = (long long)v + view[4 * k + 1], su = (long long)u + view[4 * k];
  out[i] = (sv >= 0 && sv < Hs && su >= 0 && su < Ws) ? src[sv * Ws + su] : 0xff000000u;
}

// ---- overlays
// tiles [tx0, tx1] x [ty0, ty1] of the view that segment seg can cover; false when none
__device__ __forceinline__ bool bev_seg_tiles(const double* __restrict__ g, double width, int H, int W, int& tx0,
                                              int& tx1, int& ty0, int& ty1) {
  const double r = 0.5 * width + 0.5;                 // coverage is zero at and beyond this distance
  const double lo_x = fmin(g[0], g[2]) - r, hi_x = fmax(g[0], g[2]) + r;
  const double lo_y = fmin(g[1], g[3]) - r, hi_y = fmax(g[1], g[3]) + r;
  if (!(hi_x > 0.0 && lo_x < (double)W && hi_y > 0.0 && lo_y < (double)H)) return false;   // also drops NaN
  // pixel centres are at half-integers: column u can be covered when lo_x < u + 0.5 < hi_x
  const int u0 = (int)fmax(floor(lo_x - 0.5), 0.0), u1 = (int)fmin(ceil(hi_x - 0.5), (double)(W - 1));
  const int v0 = (int)fmax(floor(lo_y - 0.5), 0.0), v1 = (int)fmin(ceil(hi_y - 0.5), (double)(H - 1));
  tx0 = u0 / BEV_TILE; tx1 = u1 / BEV_TILE; ty0 = v0 / BEV_TILE; ty1 = v1 / BEV_TILE;
  return true;
}

// view_dims [nv][4]: H, W, tiles across, tiles down; tile_base [nv]: first tile of the view.
// FILL false: tile_count[tile] += 1 per (segment, tile).  FILL true: items[tile_off[tile] + cursor++] = segment.
template <bool FILL>
__global__ __launch_bounds__(BEV_THREADS) void bev_bin_kernel(const double* __restrict__ seg, const int* __restrict__ seg_line,
                                                              int n_seg, const double* __restrict__ style,
                                                              const int* __restrict__ line_view,
                                                              const int* __restrict__ view_dims,
                                                              const long long* __restrict__ tile_base,
                                                              int* __restrict__ tile_count,
                                                              const long long* __restrict__ tile_off,
                                                              int* __restrict__ items) {
  const int e = blockIdx.x * BEV_THREADS + threadIdx.x;
  if (e >= n_seg) return;
  const int l = seg_line[e], k = line_view[l];
  const int* d = view_dims + 4 * k;
  int tx0, tx1, ty0, ty1;
  if (!bev_seg_tiles(seg + (long long)BEV_SEG_DOUBLES * e, style[BEV_STYLE_DOUBLES * l + 4], d[0], d[1], tx0, tx1, ty0, ty1))
    return;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) {
      const long long tile = tile_base[k] + (long long)ty * d[2] + tx;
      const int slot = atomicAdd(&tile_count[tile], 1);
      if (FILL) items[tile_off[tile] + slot] = e;
    }
}

// coverage of the pixel centre (cx, cy) by one segment: clamp(w/2 + 0.5 - d, 0, 1), zero where the
// nearest point of the segment lies in an "off" stretch of the dash pattern
__device__ __forceinline__ double bev_coverage(const double* __restrict__ g, double width, double on, double off,
                                               double cx, double cy) {
#pragma clang fp contract(off)
  const double ex = g[2] - g[0], ey = g[3] - g[1];
  const double len2 = ex * ex + ey * ey;
  double t = 0.0;
  if (len2 > 0.0) {
    t = ((cx - g[0]) * ex + (cy - g[1]) * ey) / len2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  }
  const double nx = g[0] + t * ex, ny = g[1] + t * ey;
  const double dx = cx - nx, dy = cy - ny;
  const double d = sqrt(dx * dx + dy * dy);
  double c = 0.5 * width + 0.5 - d;
  c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
  if (off > 0.0 && c > 0.0) {
    const double s = g[4] + t * sqrt(len2);
    if (fmod(s, on + off) >= on) c = 0.0;
  }
  return c;
}

// canvas: packed RGBA views, view k at canvas + pix_off[k].  tile_view [n_tiles]: the view of each tile.
// items / sorted [tile_off[n_tiles]]: the tile's segments as filled / in ascending (= line) order.
__global__ __launch_bounds__(BEV_THREADS) void bev_draw_kernel(const double* __restrict__ seg, const int* __restrict__ seg_line,
                                                               const double* __restrict__ style,
                                                               const int* __restrict__ view_dims,
                                                               const long long* __restrict__ tile_base,
                                                               const long long* __restrict__ pix_off,
                                                               const int* __restrict__ tile_view,
                                                               const long long* __restrict__ tile_off,
                                                               const int* __restrict__ items, int* __restrict__ sorted,
                                                               unsigned* __restrict__ canvas) {
#pragma clang fp contract(off)
  const long long tile = blockIdx.x;
  const long long first = tile_off[tile];
  const int n = (int)(tile_off[tile + 1] - first);
  if (n == 0) return;
  const int t = threadIdx.x;
  for (int e = t; e < n; e += BEV_THREADS) {          // segment ids are distinct inside a tile
    const int id = items[first + e];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += items[first + j] < id;
    sorted[first + rank] = id;
  }
  __syncthreads();
  const int k = tile_view[tile];
  const int* dm = view_dims + 4 * k;
  const long long loc = tile - tile_base[k];
  const int ty = (int)(loc / dm[2]), tx = (int)(loc - (long long)ty * dm[2]);
  const int u = tx * BEV_TILE + (t & (BEV_TILE - 1)), v = ty * BEV_TILE + t / BEV_TILE;
  if (u >= dm[1] || v >= dm[0]) return;
  unsigned* px = canvas + pix_off[k] + (long long)v * dm[1] + u;
  const unsigned old = *px;
  double rgb[3] = {(double)(old & 255u), (double)((old >> 8) & 255u), (double)((old >> 16) & 255u)};
  const double cx = u + 0.5, cy = v + 0.5;
  bool touched = false;
  int cur = -1;
  double cmax = 0.0;
  for (int e = 0; e <= n; ++e) {
    const int id = e < n ? sorted[first + e] : -1;
    const int l = e < n ? seg_line[id] : -1;
    if (l != cur) {
      if (cur >= 0 && cmax > 0.0) {
        const double* st = style + BEV_STYLE_DOUBLES * cur;
        const double a = st[3] * cmax;
        for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * (1.0 - a) + st[c] * a;
        touched = true;
      }
      cur = l; cmax = 0.0;
    }
    if (e < n) {
      const double* st = style + BEV_STYLE_DOUBLES * l;
      const double c = bev_coverage(seg + (long long)BEV_SEG_DOUBLES * id, st[4], st[5], st[6], cx, cy);
      cmax = c > cmax ? c : cmax;
    }
  }
  if (!touched) return;
  unsigned outp = old & 0xff000000u;
  for (int c = 0; c < 3; ++c) {
    double r = rint(rgb[c]);
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    outp |= (unsigned)r << (8 * c);
  }
  *px = outp;
}

}  // namespace prh
