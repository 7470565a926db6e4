// PCD text codec on the GPU: the bytes between "the cloud is on the device" and the reference's
// ASCII scene files (save_pcd, tools/generate_train_data.py:184-190: "%.4f %.4f %.4f %d" rows;
// src/dataset.py:31-76: np.loadtxt / the 14-byte binary records of merged.pcd).
//   pcd_format_kernel<T, false>  COUNT: one wave per group of 64 rows; per row the byte length of
//                       its text, per group the byte total and the first row outside the domain
//   pcd_format_kernel<T, true>   WRITE: the same integers again (they are cheaper to recompute than
//                       to keep: 32 B per row), a wave prefix sum of the row lengths, the 64 rows
//                       assembled in LDS at the alignment phase of their place in the file, then
//                       the contiguous span stored with aligned 16-byte stores + a byte head / tail
//   pcd_slice_bytes_kernel       byte_offsets [S+1] of the slices from the group offsets
//   pcd_lines_kernel<false/true> newline index of a payload: threads read 16 aligned bytes each;
//                       COUNT leaves newlines per 4096-byte block, WRITE the start of every row
//   pcd_parse_kernel    one thread per row: tokens -> correctly rounded double -> float32
//   pcd_unpack14_kernel 14-byte xyz-f32 + u16-intensity records -> [P,4] float32 through LDS
//   pcd_first_kernel    smallest flagged row of the per-group / per-block candidates -> status word
// Between the passes the wrapper runs one prefix sum (torch.cumsum) over the group / block totals.
// Integer arithmetic throughout, one fp64 multiply or divide per parsed token, no atomics and no
// inline assembly: two runs give the same bytes.
//
// Formatter domain: finite x, y, z with |v| < 2^40 and finite intensity with |v| < 2^53.  The
// arithmetic itself would carry |v| < 2^50 (M * 625 * 2^(E+4) < 2^64) and |intensity| < 2^63; the
// narrower bounds keep a row at most PCD_ROW_MAX = 78 bytes, so a wave's 64 rows fit 5 KB of LDS.
// A row outside the domain has length 0 in both passes (no byte is written for it) and is
// reported through the status word; the caller falls back to the host formatter.
//
// "%.4f" exactly: |v| = M * 2^E with M < 2^53, so |v| * 10^4 = (M * 625) * 2^(E+4) and M * 625 <
// 2^63 is an exact integer.  Inside the domain E + 4 <= -9, a right shift; the bits shifted out
// are compared with one half (guard) and the kept integer's parity decides a tie: round half to
// even on the exact binary value, which is what printf does.
//
// Parser fast path (per token [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)?): the digits after leading zeros
// form an integer m <= 2^53 (at most 19 digits are accumulated, more flag the row) and the decimal
// exponent k = exponent - fraction digits has |k| <= 22.  m and 10^|k| are exact doubles, so
// m * 10^k or m / 10^-k is ONE correctly rounded fp64 operation - the double np.loadtxt makes -
// and the cast to float32 rounds a second time exactly as numpy's cast does.  Anything else (longer
// digit strings, larger exponents, nan / inf, any other byte, a blank line, '#', a row whose field
// count differs from ncols) flags the row: the device path never guesses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace prh {

constexpr int PCD_GROUP = 64;                 // rows one wave formats
constexpr int PCD_FIELD_MAX = 19;             // '-' + 13 integer digits + '.' + 4
constexpr int PCD_INT_MAX = 17;               // '-' + 16 digits (|v| < 2^53)
constexpr int PCD_ROW_MAX = 3 * PCD_FIELD_MAX + PCD_INT_MAX + 4;       // 3 blanks + '\n' = 78
constexpr int PCD_WAVE_LDS = PCD_GROUP * PCD_ROW_MAX + 16;            // + the alignment phase
constexpr int PCD_BLOCK_BYTES = 4096;         // payload bytes one 256-thread block indexes
constexpr int PCD_UNPACK_POINTS = 256;        // 14-byte records per block: 3584 bytes = 224 x 16
constexpr long long PCD_NONE = 0x7fffffffffffffffll;
static_assert(PCD_WAVE_LDS % 16 == 0, "a wave's staging area is a whole number of 16-byte chunks");

// |v| * 10^4 rounded half to even on the exact value; false outside the domain.
__device__ __forceinline__ bool pcd_scale4(double v, unsigned long long& n, bool& neg) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  neg = (b >> 63) != 0;
  const int ex = (int)((b >> 52) & 0x7ff);
  const unsigned long long fr = b & ((1ull << 52) - 1);
  if (ex >= 1023 + 40) return false;                    // |v| >= 2^40, inf, nan
  const unsigned long long m = ex == 0 ? fr : (fr | (1ull << 52));
  const int e = ex == 0 ? -1074 : ex - 1075;             // |v| = m * 2^e
  const unsigned long long p = m * 625ull;               // < 2^63, exact
  const int s = -(e + 4);                                // >= 9 inside the domain
  if (s >= 64) { n = 0; return true; }                   // p / 2^s < 1/2
  unsigned long long q = p >> s;
  const unsigned long long rem = p & ((1ull << s) - 1), half = 1ull << (s - 1);
  if (rem > half || (rem == half && (q & 1ull))) ++q;
  n = q;
  return true;
}

// int(v) as "%d" takes it (truncation toward zero); false outside the domain.
__device__ __forceinline__ bool pcd_trunc(double v, unsigned long long& a, bool& neg) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const int ex = (int)((b >> 52) & 0x7ff);
  if (ex >= 1023 + 53) return false;                    // |v| >= 2^53, inf, nan
  const long long t = (long long)v;
  neg = t < 0;                                           // (-1, 0) prints "0"
  a = (unsigned long long)(t < 0 ? -t : t);
  return true;
}

__device__ __forceinline__ int pcd_ndigits(unsigned long long x) {
  int nd = 1;
  unsigned long long p = 10ull;
#pragma unroll
  for (int k = 1; k < 17; ++k) { nd += x >= p ? 1 : 0; p *= 10ull; }
  return nd;                                             // x < 10^17
}

// decimal digits of x written backwards from end; returns the new front
__device__ __forceinline__ unsigned char* pcd_put(unsigned char* end, unsigned long long x) {
  while (x >= 100000000ull) {
    const unsigned long long q = x / 100000000ull;
    unsigned r = (unsigned)(x - q * 100000000ull);
#pragma unroll
    for (int k = 0; k < 8; ++k) { *--end = (unsigned char)('0' + r % 10u); r /= 10u; }
    x = q;
  }
  unsigned y = (unsigned)x;
  do { *--end = (unsigned char)('0' + y % 10u); y /= 10u; } while (y != 0u);
  return end;
}

template <typename T> struct PcdLoad;
template <> struct PcdLoad<double> {
  static __device__ __forceinline__ void row(const double* p, long long r, double v[4]) {
    const double2* q = reinterpret_cast<const double2*>(p + 4 * r);
    const double2 a = q[0], b = q[1];
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  }
};
template <> struct PcdLoad<float> {
  static __device__ __forceinline__ void row(const float* p, long long r, double v[4]) {
    const float4 a = *reinterpret_cast<const float4*>(p + 4 * r);
    v[0] = (double)a.x; v[1] = (double)a.y; v[2] = (double)a.z; v[3] = (double)a.w;
  }
};

// One wave per group of 64 rows, 4 groups per block.
//   COUNT: row_bytes [n_rows] u8 text length of each row (0: outside the domain), group_bytes [G]
//          their sum, group_bad [G] the first row outside the domain or PCD_NONE
//   WRITE: group_off [G+1] exclusive prefix of group_bytes; text[group_off[g] ...] the rows' text;
//          bytes at or beyond capacity are never written
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void pcd_format_kernel(const T* __restrict__ points, long long n_rows,
                                                         unsigned char* __restrict__ row_bytes,
                                                         int* __restrict__ group_bytes,
                                                         long long* __restrict__ group_bad,
                                                         const long long* __restrict__ group_off,
                                                         unsigned char* __restrict__ text, long long capacity) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[WRITE ? 4 * PCD_WAVE_LDS : 16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long g = (long long)blockIdx.x * 4 + wv;
  const long long r = g * PCD_GROUP + lane;
  const bool live = r < n_rows;                          // a dead group still walks to the barrier
  unsigned long long n[4] = {0, 0, 0, 0};
  bool neg[4] = {false, false, false, false};
  bool ok = true;
  int fl[4] = {0, 0, 0, 0};
  int len = 0;
  if (live) {
    double v[4];
    PcdLoad<T>::row(points, r, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = pcd_scale4(v[c], n[c], neg[c]) && ok;
    ok = pcd_trunc(v[3], n[3], neg[3]) && ok;
    if (ok) {
#pragma unroll
      for (int c = 0; c < 3; ++c) fl[c] = (neg[c] ? 1 : 0) + pcd_ndigits(n[c] / 10000ull) + 5;
      fl[3] = (neg[3] ? 1 : 0) + pcd_ndigits(n[3]);
      len = fl[0] + fl[1] + fl[2] + fl[3] + 4;
    }
  }
  // inclusive prefix of len over the wave
  int incl = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const int total = __shfl(incl, 63);
  if (!WRITE) {
    if (live) row_bytes[r] = (unsigned char)len;
    const unsigned long long badmask = __ballot(live && !ok);
    if (lane == 0 && g * PCD_GROUP < n_rows) {
      group_bytes[g] = total;
      group_bad[g] = badmask ? g * PCD_GROUP + (__ffsll((long long)badmask) - 1) : PCD_NONE;
    }
    return;
  }
  const long long gbase = g * PCD_GROUP < n_rows ? group_off[g] : 0;
  const int ph = (int)((uintptr_t)(text + gbase) & 15);
  unsigned char* buf = stage + wv * PCD_WAVE_LDS;
  if (live && ok) {
    unsigned char* e = buf + ph + (incl - len);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      e += fl[c];
      const unsigned long long ip = n[c] / 10000ull;
      unsigned f = (unsigned)(n[c] - ip * 10000ull);
      unsigned char* q = e;
#pragma unroll
      for (int k = 0; k < 4; ++k) { *--q = (unsigned char)('0' + f % 10u); f /= 10u; }
      *--q = '.';
      q = pcd_put(q, ip);
      if (neg[c]) *--q = '-';
      *e++ = ' ';
    }
    e += fl[3];
    unsigned char* q = pcd_put(e, n[3]);
    if (neg[3]) *--q = '-';
    *e = '\n';
  }
  __syncthreads();
  const int end = ph + total, nchunk = (end + 15) >> 4;
  unsigned char* gal = text + gbase - ph;                // 16-byte aligned
  for (int c = lane; c < nchunk; c += 64) {
    const int lo = c << 4;
    const long long g0 = gbase - ph + lo;                // index in text of the chunk's first byte
    if (lo >= ph && lo + 16 <= end && g0 + 16 <= capacity) {
      *reinterpret_cast<uint4*>(gal + lo) = *reinterpret_cast<const uint4*>(buf + lo);
    } else {
      const int a = lo > ph ? lo : ph, b = lo + 16 < end ? lo + 16 : end;
      for (int j = a; j < b; ++j)
        if (gbase - ph + j < capacity) gal[j] = buf[j];
    }
  }
}

// byte_offsets[s] = byte at which row offsets[s] starts (s = 0..S): its group's offset + the
// lengths of the rows before it in the group.  offsets may be NULL for one slice [0, n_rows].
__global__ __launch_bounds__(256) void pcd_slice_bytes_kernel(const long long* __restrict__ offsets, int S,
                                                              long long n_rows,
                                                              const unsigned char* __restrict__ row_bytes,
                                                              const long long* __restrict__ group_off,
                                                              long long* __restrict__ byte_offsets) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s > S) return;
  long long r = offsets ? offsets[s] : (s == 0 ? 0 : n_rows);
  r = r < 0 ? 0 : (r > n_rows ? n_rows : r);
  const long long g = r / PCD_GROUP;
  long long b = n_rows > 0 ? group_off[g] : 0;          // group_off has ceil(n_rows / 64) + 1 entries
  for (long long q = g * PCD_GROUP; q < r; ++q) b += row_bytes[q];
  byte_offsets[s] = b;
}

// status[0] = the smallest candidate that is not PCD_NONE, or -1.  One block, fixed order.
__global__ __launch_bounds__(256) void pcd_first_kernel(const long long* __restrict__ cand, long long n,
                                                        long long* __restrict__ status) {
  __shared__ long long part[256];
  long long m = PCD_NONE;
  for (long long i = threadIdx.x; i < n; i += 256) { const long long c = cand[i]; m = c < m ? c : m; }
  part[threadIdx.x] = m;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) { const long long o = part[threadIdx.x + d]; if (o < part[threadIdx.x]) part[threadIdx.x] = o; }
    __syncthreads();
  }
  if (threadIdx.x == 0) status[0] = part[0] == PCD_NONE ? -1 : part[0];
}

// The 16 bytes at the aligned address al of which only those inside [lo, hi) may be touched:
// one 16-byte load when all are, byte loads of the valid ones (zeros elsewhere) otherwise.
__device__ __forceinline__ uint4 pcd_load16(const unsigned char* al, const unsigned char* lo, const unsigned char* hi) {
  if (al >= lo && al + 16 <= hi) return *reinterpret_cast<const uint4*>(al);
  unsigned w[4] = {0u, 0u, 0u, 0u};
  for (int j = 0; j < 16; ++j)
    if (al + j >= lo && al + j < hi) w[j >> 2] |= (unsigned)al[j] << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ unsigned pcd_byte(const uint4& v, int j) {
  const unsigned w = j < 8 ? (j < 4 ? v.x : v.y) : (j < 12 ? v.z : v.w);
  return (w >> (8 * (j & 3))) & 0xffu;
}

// Newline index.  Blocks tile the 16-byte aligned address grid from (payload & ~15): block b owns
// 256 chunks, thread t chunk b * 256 + t, so every full chunk is one aligned 16-byte load whatever
// the payload's own alignment and length.
//   COUNT: block_lines [NB] newlines in the block
//   WRITE: block_off [NB+1] exclusive prefix; the k-th newline (from 0) at byte p sets
//          row_start[k + 1] = p + 1; row_start[0] = 0 and row_start[n_rows] = n_bytes
template <bool WRITE>
__global__ __launch_bounds__(256) void pcd_lines_kernel(const unsigned char* __restrict__ payload, long long n_bytes,
                                                        int* __restrict__ block_lines,
                                                        const long long* __restrict__ block_off,
                                                        long long* __restrict__ row_start, long long n_rows) {
  __shared__ int wave_tot[4];
  const int ph = (int)((uintptr_t)payload & 15);
  const unsigned char* al = payload - ph + ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  const unsigned char* hi = payload + n_bytes;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (al < hi) v = pcd_load16(al, payload, hi);          // bytes outside the payload read as 0
  int c = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) c += pcd_byte(v, j) == (unsigned)'\n' ? 1 : 0;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wv; ++w) before += wave_tot[w];
  if (!WRITE) {
    if (threadIdx.x == 255) block_lines[blockIdx.x] = before + incl;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { row_start[0] = 0; row_start[n_rows] = n_bytes; }
  long long k = block_off[blockIdx.x] + before + (incl - c);
  const long long p0 = al - payload;                     // payload index of the chunk's first byte
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (pcd_byte(v, j) == (unsigned)'\n') {
      if (k + 1 <= n_rows) row_start[k + 1] = p0 + j + 1;
      ++k;
    }
}

__device__ const double PCD_P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                       1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__device__ __forceinline__ bool pcd_blank(unsigned c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool pcd_digit(unsigned c) { return c - '0' < 10u; }

// One token at p[i..e); on success i is one past it.
__device__ __forceinline__ bool pcd_token(const unsigned char* __restrict__ p, long long& i, long long e, float& out) {
  bool neg = false;
  if (p[i] == '+' || p[i] == '-') { neg = p[i] == '-'; ++i; }
  unsigned long long m = 0;
  int nd = 0, fd = 0;
  bool any = false, over = false;
  for (; i < e && pcd_digit(p[i]); ++i) {
    const unsigned d = p[i] - '0';
    any = true;
    if (m != 0 || d != 0) { if (nd < 19) { m = m * 10ull + d; ++nd; } else over = true; }
  }
  if (i < e && p[i] == '.') {
    ++i;
    for (; i < e && pcd_digit(p[i]); ++i) {
      const unsigned d = p[i] - '0';
      any = true;
      if (fd < 100000) ++fd;
      if (m != 0 || d != 0) { if (nd < 19) { m = m * 10ull + d; ++nd; } else over = true; }
    }
  }
  if (!any) return false;
  int ex = 0;
  if (i < e && (p[i] == 'e' || p[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < e && (p[i] == '+' || p[i] == '-')) { eneg = p[i] == '-'; ++i; }
    if (!(i < e && pcd_digit(p[i]))) return false;
    for (; i < e && pcd_digit(p[i]); ++i)
      if (ex < 100000) ex = ex * 10 + (int)(p[i] - '0');
    if (eneg) ex = -ex;
  }
  const int k = ex - fd;
  if (over || m > (1ull << 53) || k > 22 || k < -22) return false;
  const double dm = (double)(long long)m;                // exact
  const double d = k >= 0 ? dm * PCD_P10[k] : dm / PCD_P10[-k];          // the one rounding to double
  out = (float)(neg ? -d : d);                           // the second rounding, as numpy's cast
  return true;
}

// One thread per row.  out [n_rows, ncols]; block_bad [blocks] the first flagged row of each block.
__global__ __launch_bounds__(256) void pcd_parse_kernel(const unsigned char* __restrict__ p,
                                                        const long long* __restrict__ row_start, long long n_rows,
                                                        int ncols, float* __restrict__ out,
                                                        long long* __restrict__ block_bad) {
  __shared__ long long part[4];
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  long long mine = PCD_NONE;
  if (r < n_rows) {
    long long i = row_start[r], e = row_start[r + 1];
    if (e > i && p[e - 1] == '\n') --e;
    if (e > i && p[e - 1] == '\r') --e;
    int col = 0;
    bool bad = false;
    while (true) {
      while (i < e && pcd_blank(p[i])) ++i;
      if (i >= e) break;
      float v;
      if (col >= ncols || !pcd_token(p, i, e, v) || (i < e && !pcd_blank(p[i]))) { bad = true; break; }
      out[r * ncols + col] = v;
      ++col;
    }
    if (bad || col != ncols) mine = r;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const long long o = __shfl_xor(mine, d);
    mine = o < mine ? o : mine;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long m = part[0];
    for (int w = 1; w < 4; ++w) m = part[w] < m ? part[w] : m;
    block_bad[blockIdx.x] = m;
  }
}

// 14-byte records (x y z float32, intensity u16, little endian) -> out [n,4] float32.  A block's
// 256 records are 3584 bytes; they are staged in LDS at the payload's alignment phase with aligned
// 16-byte loads (byte loads at the ends), then every thread assembles its record from LDS.
__global__ __launch_bounds__(256) void pcd_unpack14_kernel(const unsigned char* __restrict__ payload,
                                                           long long n_points, float4* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[PCD_UNPACK_POINTS * 14 + 16];
  const long long p0 = (long long)blockIdx.x * PCD_UNPACK_POINTS;
  const long long left = n_points - p0;
  const int np = left < PCD_UNPACK_POINTS ? (int)left : PCD_UNPACK_POINTS;
  const unsigned char* src = payload + p0 * 14;
  const unsigned char* hi = src + (long long)np * 14;
  const int ph = (int)((uintptr_t)src & 15);
  const int nchunk = (ph + np * 14 + 15) >> 4;           // <= 225
  if ((int)threadIdx.x < nchunk)
    *reinterpret_cast<uint4*>(stage + 16 * threadIdx.x) = pcd_load16(src - ph + 16 * threadIdx.x, src, hi);
  __syncthreads();
  if ((int)threadIdx.x >= np) return;
  const unsigned char* q = stage + ph + 14 * threadIdx.x;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 14; ++j) w[j >> 2] |= (unsigned)q[j] << (8 * (j & 3));
  out[p0 + threadIdx.x] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]),
                                      (float)w[3]);
}

}  // namespace prh
