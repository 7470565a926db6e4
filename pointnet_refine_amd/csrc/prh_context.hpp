// Per-line context builder on the GPU: for every polyline of a scene,
// crop the point cloud to a tube around the line, weight the candidates by distance and
// intensity, draw N of them and centre the block on the line - the hot loop of the reference's
// whole-scene inference and of every dataset item:
//   crop     : distance to the polyline densified to 200 points < radius
//              (src/dataset.py:210-222, inference_whole_scene.py:104-110; KDTree there, brute
//               force here: L x P x 200 distance evaluations are ~1e11 fp32 ops per scene)
//   weights  : exp(-d/decay) * (0.5 + (I-Imin)/(Imax-Imin+1e-6)), d to the nearest of the line's
//              32 points, 0.5 for a constant intensity (src/dataset.py:93-111)
//   sampling : K = 0 -> zeros; K <= N -> N uniform draws with replacement; K > N -> N draws
//              without replacement proportional to the weights (uniform if they sum to < 1e-6)
//              (src/dataset.py:86-91,115-130).  numpy.random.choice is replaced by counter-based
//              hashing of (seed, line, point): Gumbel-top-k, i.e. the same Plackett-Luce law as
//              sequential weighted draws without replacement - parity is distributional.
//   centring : xyz minus the mean of the line's points, raw intensity (src/dataset.py:229-234).
// Everything is deterministic for a given seed: candidates are compacted in cloud order by a
// two-pass count / scan / fill (no atomics), the top-N keys by an exact radix select, ties in
// cloud order.  HBM-light, VALU-bound: one thread per (point, line) in the crop passes.
//
// Two drivers share the per-item / per-line bodies (ctx_crop_item, ctx_scan_line, ctx_select_line):
// the per-scene kernels (one cloud, every line cropped from it, max_candidates slots per line) and
// the ragged kernels (one point buffer of slices back to back, every line cropped from its own
// slice, candidates in CSR sized from the counts).  A line gets the same arithmetic in the same
// order from both, so the ragged builder's bytes are the per-slice builder's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prh {

constexpr int CTX_MAX_DENSE = 256;    // polyline samples held in LDS by the crop kernels
constexpr int CTX_MAX_LINE = 64;

__device__ __forceinline__ uint64_t ctx_mix(uint64_t x) {      // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t ctx_hash(uint64_t seed, unsigned line, unsigned idx) {
  return ctx_mix(ctx_mix(seed ^ ((uint64_t)line << 32 | idx)));
}
// uniform strictly inside (0,1), 23 bits: (k + 0.5) / 2^23 is exact in fp32 for every k < 2^23
// (24 bits would need 25 significant bits from 2^23 on and round the top value to 1.0f, G = +inf)
__device__ __forceinline__ float ctx_u01(uint64_t h) { return ((float)(h >> 41) + 0.5f) * (1.0f / 8388608.0f); }
// order-preserving map float -> uint32
__device__ __forceinline__ unsigned ctx_sortable(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float ctx_min_d2(float x, float y, float z, const float* pts, int n) {
  float best = 3.0e38f;
  for (int j = 0; j < n; ++j) {
    const float dx = x - pts[3 * j], dy = y - pts[3 * j + 1], dz = z - pts[3 * j + 2];
    best = fminf(best, fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
  }
  return best;
}

// pass 0: bounding box of each line's tube (polyline samples +- radius)
__global__ __launch_bounds__(64) void ctx_bbox_kernel(const float* __restrict__ dense, int nd, float radius,
                                                      float* __restrict__ box) {
  const int line = blockIdx.x, lane = threadIdx.x;
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int j = lane; j < nd; j += 64)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = dense[((size_t)line * nd + j) * 3 + c];
      lo[c] = fminf(lo[c], v); hi[c] = fmaxf(hi[c], v);
    }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    for (int o = 32; o > 0; o >>= 1) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], o));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o));
    }
  const float r = radius * 1.0001f + 1e-6f;
  if (lane < 3) { box[line * 6 + lane] = lo[lane] - r; box[line * 6 + 3 + lane] = hi[lane] + r; }
}

// One (256-point block, line) work item of the crop passes, shared by the per-scene and the ragged
// kernels so that a line over the same points gives the same candidates in the same order:
// the tube's bounding box, the distance to the dense samples, ballot / popcount ranks (no atomics).
//   FILL = false: *cnt_slot = number of the block's points inside the tube
//   FILL = true : the same test again, points written to cl[*off_slot + rank] (rows of `cloud`)
template <bool FILL>
__device__ __forceinline__ void ctx_crop_item(const float* __restrict__ cloud, int npts,
                                              const float* __restrict__ dline, int nd,
                                              const float* __restrict__ bx, float r2, int blk,
                                              int* __restrict__ cnt_slot, const int* __restrict__ off_slot,
                                              int* __restrict__ cl, int max_cand) {
  __shared__ float pts[3 * CTX_MAX_DENSE];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x;
  const int p = blk * 256 + tid;
  // the tube's bounding box first: most (point, line) pairs - and most whole blocks - end here
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  bool near = false;
  if (p < npts) {
    v = *reinterpret_cast<const float4*>(cloud + (size_t)p * 4);
    near = v.x >= bx[0] && v.x <= bx[3] && v.y >= bx[1] && v.y <= bx[4] && v.z >= bx[2] && v.z <= bx[5];
  }
  if (!__syncthreads_or(near)) {
    if (!FILL && tid == 0) *cnt_slot = 0;
    return;
  }
  for (int i = tid; i < 3 * nd; i += 256) pts[i] = dline[i];
  __syncthreads();
  bool in = false;
  if (near) in = ctx_min_d2(v.x, v.y, v.z, pts, nd) < r2;
  const unsigned long long bal = __ballot(in);
  const int lane = tid & 63, wave = tid >> 6;
  if (lane == 0) wcnt[wave] = __popcll(bal);
  __syncthreads();
  if (!FILL) {
    if (tid == 0) *cnt_slot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return;
  }
  if (in) {
    int pos = *off_slot + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcnt[w];
    if (pos < max_cand) cl[pos] = p;
  }
}

// pass 1 (FILL = false): per (256-point block, line) number of points inside the tube;
// pass 3 (FILL = true): the same test again, points written to cand[line][offset + rank]
template <bool FILL>
__global__ __launch_bounds__(256) void ctx_crop_kernel(const float* __restrict__ cloud, int npts,
                                                       const float* __restrict__ dense, int nd,
                                                       const float* __restrict__ box, float r2, int nblk,
                                                       int* __restrict__ blkcnt,
                                                       const int* __restrict__ blkoff,
                                                       int* __restrict__ cand, int max_cand) {
  const int line = blockIdx.y, blk = blockIdx.x;
  const size_t slot = (size_t)line * nblk + blk;
  ctx_crop_item<FILL>(cloud, npts, dense + (size_t)line * nd * 3, nd, box + line * 6, r2, blk, blkcnt + slot,
                      FILL ? blkoff + slot : nullptr, FILL ? cand + (size_t)line * max_cand : nullptr, max_cand);
}

// The ragged builder's line of a work item: the last line of [lo, hi) whose first item is <= item
// (lines without blocks repeat their neighbour's offset and are never found)
__device__ __forceinline__ int ctx_item_line(const long long* __restrict__ blk_offsets, int lo, int hi,
                                             long long item) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_offsets[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

// Ragged crop passes: flat 1-D grid of (line, 256-point block of that line's slice) work items
// over the lines [line0, line0 + n_run).  line_base / line_npts: first row and number of rows of
// the line's slice in `points`; blk_offsets (L+1): exclusive scan of ceil(line_npts / 256);
// blkcnt / blkoff are indexed by work item; candidates are rows relative to line_base, written to
// cand + (cand_offsets[line] - cand_offsets[line0]).
template <bool FILL>
__global__ __launch_bounds__(256) void ctx_ragged_crop_kernel(
    const float* __restrict__ points, const int* __restrict__ line_base, const int* __restrict__ line_npts,
    const long long* __restrict__ blk_offsets, int line0, int n_run, const float* __restrict__ dense, int nd,
    const float* __restrict__ box, float r2, int* __restrict__ blkcnt, const int* __restrict__ blkoff,
    const long long* __restrict__ cand_offsets, int* __restrict__ cand, long long capacity) {
  const long long item = blk_offsets[line0] + (long long)blockIdx.x;
  const int line = ctx_item_line(blk_offsets, line0, line0 + n_run, item);
  const int blk = (int)(item - blk_offsets[line]);
  int* cl = nullptr;
  int room = 0;
  if (FILL) {
    const long long at = cand_offsets[line] - cand_offsets[line0];
    cl = cand + at;
    room = (int)max(0ll, min(cand_offsets[line + 1] - cand_offsets[line], capacity - at));   // never past the buffer
  }
  ctx_crop_item<FILL>(points + (size_t)line_base[line] * 4, line_npts[line], dense + (size_t)line * nd * 3, nd,
                      box + (size_t)line * 6, r2, blk, blkcnt + item, FILL ? blkoff + item : nullptr, cl, room);
}

// Exclusive scan of one line's nblk block counts by one workgroup; *count = total inside the tube
__device__ __forceinline__ void ctx_scan_line(const int* __restrict__ blkcnt, int nblk, int* __restrict__ blkoff,
                                              int* __restrict__ count) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (nblk + 255) / 256;
  const int b0 = tid * per, b1 = min(b0 + per, nblk);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += blkcnt[b];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int t = part[i]; part[i] = run; run += t; }
    *count = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int b = b0; b < b1; ++b) {
    blkoff[b] = run;
    run += blkcnt[b];
  }
}

// pass 2: exclusive scan of a line's block counts; counts[line] = total inside the tube
__global__ __launch_bounds__(256) void ctx_scan_kernel(const int* __restrict__ blkcnt, int nblk,
                                                       int* __restrict__ blkoff, int* __restrict__ counts) {
  const int line = blockIdx.x;
  ctx_scan_line(blkcnt + (size_t)line * nblk, nblk, blkoff + (size_t)line * nblk, counts + line);
}

// ragged: a line's blocks are the work items blk_offsets[line] .. blk_offsets[line + 1] (none for a
// slice without points: counts = 0)
__global__ __launch_bounds__(256) void ctx_ragged_scan_kernel(const int* __restrict__ blkcnt,
                                                              const long long* __restrict__ blk_offsets,
                                                              int* __restrict__ blkoff, int* __restrict__ counts) {
  const int line = blockIdx.x;
  const long long b0 = blk_offsets[line];
  ctx_scan_line(blkcnt + b0, (int)(blk_offsets[line + 1] - b0), blkoff + b0, counts + line);
}

// ragged: cand_offsets (L+1) = exclusive scan of counts (L), one workgroup
__global__ __launch_bounds__(256) void ctx_ragged_offsets_kernel(const int* __restrict__ counts, int n_lines,
                                                                 long long* __restrict__ cand_offsets) {
  __shared__ long long part[256];
  const int tid = threadIdx.x;
  const int per = (n_lines + 255) / 256;
  const int l0 = min(tid * per, n_lines), l1 = min(l0 + per, n_lines);
  long long s = 0;
  for (int l = l0; l < l1; ++l) s += counts[l];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < 256; ++i) { const long long t = part[i]; part[i] = run; run += t; }
    cand_offsets[n_lines] = run;
  }
  __syncthreads();
  long long run = part[tid];
  for (int l = l0; l < l1; ++l) {
    cand_offsets[l] = run;
    run += counts[l];
  }
}

// One line's weights, keys, exact top-N, gather + centre by one workgroup, shared by the per-scene
// and the ragged kernel.  cloud: the points the K candidate rows cl[] index; hline: the line's index
// in the hash; kb: K key slots (the weights are kept there as floats first); o: the line's N rows;
// dbg_w: K weight slots or null.
__device__ __forceinline__ void ctx_select_line(const float* __restrict__ cloud, const float* __restrict__ linepts,
                                                int m, int K, const int* __restrict__ cl, float decay, int N,
                                                uint64_t seed, unsigned hline, unsigned* __restrict__ kb,
                                                float* __restrict__ o, float* __restrict__ dbg_w) {
  __shared__ float lp[3 * CTX_MAX_LINE];
  __shared__ float red[256];
  __shared__ float red2[256];
  __shared__ int hist[256];
  __shared__ int sh_i[4];
  __shared__ float sh_f[4];
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * m; i += 256) lp[i] = linepts[i];
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int j = 0; j < m; ++j) s += lp[3 * j + tid];
    sh_f[tid] = s / (float)m;
  }
  __syncthreads();
  const float cx = sh_f[0], cy = sh_f[1], cz = sh_f[2];
  if (K <= N) {        // zeros, or uniform draws with replacement
    for (int i = tid; i < N; i += 256) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (K > 0) {
        const int j = (int)(ctx_hash(seed, hline, 0x40000000u + (unsigned)i) % (uint64_t)K);
        v = *reinterpret_cast<const float4*>(cloud + (size_t)cl[j] * 4);
      }
      *reinterpret_cast<float4*>(o + (size_t)i * 4) = make_float4(v.x - cx, v.y - cy, v.z - cz, v.w);
    }
    return;
  }
  // intensity range of the candidates
  float lo = 3.0e38f, hi = -3.0e38f;
  for (int j = tid; j < K; j += 256) {
    const float I = cloud[(size_t)cl[j] * 4 + 3];
    lo = fminf(lo, I); hi = fmaxf(hi, I);
  }
  red[tid] = lo; red2[tid] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) { red[tid] = fminf(red[tid], red[tid + s]); red2[tid] = fmaxf(red2[tid], red2[tid + s]); }
    __syncthreads();
  }
  lo = red[0]; hi = red2[0];
  __syncthreads();
  const bool flat = !(hi > lo);
  const float inv = 1.f / (hi - lo + 1e-6f);
  // weights (kept in the key buffer as floats for now) and their sum
  float* wbuf = reinterpret_cast<float*>(kb);
  float wsum = 0.f;
  for (int j = tid; j < K; j += 256) {
    const float4 v = *reinterpret_cast<const float4*>(cloud + (size_t)cl[j] * 4);
    const float d = sqrtf(ctx_min_d2(v.x, v.y, v.z, lp, m));
    const float w = expf(-d / decay) * (0.5f + (flat ? 0.5f : (v.w - lo) * inv));
    wbuf[j] = w;
    if (dbg_w != nullptr) dbg_w[j] = w;
    wsum += w;
  }
  red[tid] = wsum;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const bool uniform = red[0] < 1e-6f;
  __syncthreads();
  // Gumbel-top-k keys: log w + G,  G = -log(-log u)   (uniform weights: G alone)
  for (int j = tid; j < K; j += 256) {
    const float u = ctx_u01(ctx_hash(seed, hline, (unsigned)cl[j]));
    const float g = -logf(-logf(u));
    const float w = wbuf[j];
    kb[j] = ctx_sortable(uniform ? g : (w > 0.f ? logf(w) + g : -3.0e38f));
  }
  __syncthreads();
  // exact radix select of the N-th largest key: 4 passes of 8 bits, most significant first
  unsigned prefix = 0, pmask = 0;
  int need = N;                        // how many keys still to take from the current bucket
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < K; j += 256) {
      const unsigned k = kb[j];
      if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int b = 255, acc = 0;
      while (b > 0 && acc + hist[b] < need) { acc += hist[b]; --b; }
      sh_i[0] = b; sh_i[1] = need - acc;
    }
    __syncthreads();
    prefix |= (unsigned)sh_i[0] << shift;
    pmask |= 255u << shift;
    need = sh_i[1];
    __syncthreads();
  }
  const unsigned T = prefix;           // N-th largest key; `need` keys equal to T are taken
  // ordered compaction in candidate (= cloud) order
  int base = 0, eq_seen = 0;
  for (int j0 = 0; j0 < K; j0 += 256) {
    const int j = j0 + tid;
    const unsigned k = j < K ? kb[j] : 0u;
    const bool gt = j < K && k > T, eq = j < K && k == T;
    // rank of this thread among the block's gt / eq flags
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) { hist[wave] = __popcll(bg); hist[4 + wave] = __popcll(be); }
    __syncthreads();
    int eq_before = eq_seen + __popcll(be & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) eq_before += hist[4 + w];
    const bool take = gt || (eq && eq_before < need);
    const int eq_tot = hist[4] + hist[5] + hist[6] + hist[7];
    __syncthreads();
    const unsigned long long bt = __ballot(take);
    if (lane == 0) hist[8 + wave] = __popcll(bt);
    __syncthreads();
    if (take) {
      int pos = base + __popcll(bt & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; ++w) pos += hist[8 + w];
      const float4 v = *reinterpret_cast<const float4*>(cloud + (size_t)cl[j] * 4);
      if (pos < N) *reinterpret_cast<float4*>(o + (size_t)pos * 4) = make_float4(v.x - cx, v.y - cy, v.z - cz, v.w);
    }
    base += hist[8] + hist[9] + hist[10] + hist[11];
    eq_seen += eq_tot;
    __syncthreads();
  }
}

// pass 4: one workgroup per line - weights, keys, exact top-N, gather + centre
__global__ __launch_bounds__(256) void ctx_select_kernel(
    const float* __restrict__ cloud, const float* __restrict__ linepts, int m, const int* __restrict__ counts,
    const int* __restrict__ cand, int max_cand, float decay, int N, uint64_t seed, unsigned* __restrict__ keys,
    float* __restrict__ out, float* __restrict__ dbg_w) {
  const int line = blockIdx.x;
  ctx_select_line(cloud, linepts + (size_t)line * m * 3, m, min(counts[line], max_cand), cand + (size_t)line * max_cand,
                  decay, N, seed, (unsigned)line, keys + (size_t)line * max_cand, out + (size_t)line * N * 4,
                  dbg_w != nullptr ? dbg_w + (size_t)line * max_cand : nullptr);
}

// ragged: line line0 + blockIdx.x draws from its own slice (rows relative to line_base) with its
// slice's seed and its position among its slice's lines in the hash - what a per-slice call of
// ctx_select_kernel uses.  cand / keys hold the run's candidates from cand_offsets[line0] on.
__global__ __launch_bounds__(256) void ctx_ragged_select_kernel(
    const float* __restrict__ points, const int* __restrict__ line_base, const int* __restrict__ line_local,
    const uint64_t* __restrict__ line_seed, const float* __restrict__ linepts, int m, const int* __restrict__ counts,
    const long long* __restrict__ cand_offsets, int line0, const int* __restrict__ cand, float decay, int N,
    unsigned* __restrict__ keys, long long capacity, float* __restrict__ out) {
  const int line = line0 + blockIdx.x;
  const long long at = cand_offsets[line] - cand_offsets[line0];
  const int K = (int)max(0ll, min((long long)counts[line], capacity - at));                    // never past the buffer
  ctx_select_line(points + (size_t)line_base[line] * 4, linepts + (size_t)line * m * 3, m, K, cand + at,
                  decay, N, line_seed[line], (unsigned)line_local[line], keys + at, out + (size_t)line * N * 4, nullptr);
}

}  // namespace prh
