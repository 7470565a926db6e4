// C-ABI entry points of libpointnet_refine_hip.so (see include/pointnet_refine_hip.h).
// Host-side orchestration only: argument checks, workspace carving, kernel launches on the
// caller's stream.  No allocation, no synchronisation, no state kept between calls, so a
// whole forward or backward can be captured into a hipGraph by the caller.
#include "../../include/pointnet_refine_hip.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include <stdlib.h>

#include "prh_gemm.hpp"
#include "prh_attn.hpp"
#include "prh_attn16.hpp"
#include "prh_gemm_s3.hpp"
#include "prh_gemm_h2.hpp"
#include "prh_b16.hpp"
#include "prh_small.hpp"
#include "prh_attnfold.hpp"
#include "prh_fused.hpp"
#include "prh_context.hpp"
#include "prh_metrics.hpp"
#include "prh_drive.hpp"
#include "prh_match.hpp"
#include "prh_bev.hpp"
#include "prh_view.hpp"
#include "prh_fuse.hpp"
#include "prh_link.hpp"
#include "prh_link_sync.hpp"
#include "prh_support.hpp"
#include "prh_ground.hpp"
#include "prh_align.hpp"
#include "prh_trace.hpp"
#include "prh_floor.hpp"
#include "prh_pcd.hpp"
#include "prh_kernels.hpp"

using namespace prh;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(PRH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                  __FILE__, __LINE__);                                                 \
  } while (0)

#define LAUNCH_CHECK() HIP_TRY(hipGetLastError())
#define TRY_RC(x)                  \
  do {                             \
    int rc_ = (x);                 \
    if (rc_ != PRH_OK) return rc_; \
  } while (0)
#ifndef PRH_GEMM_DEFAULT
#define PRH_GEMM_DEFAULT 3
#endif

// ------------------------------------------------------------------ optional profiler
// bench.py brackets every GEMM launch with HIP events ON THE LAUNCH STREAM so it can quote
// the dominant kernel's live duration next to its algorithmic FLOPs/bytes (roofline object
// of the bench line).  Off by default; the entry points stay stateless when it is off.
struct ProfRec { hipEvent_t e0, e1; char name[64]; double flops, bytes; };
struct Profiler {
  std::mutex mu;
  std::vector<ProfRec> recs;
  size_t used = 0;
  bool on = false;
} g_prof;

struct ProfScope {
  ProfRec* r = nullptr; hipStream_t st;
  ProfScope(const char* name, double flops, double bytes, hipStream_t s) : st(s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.used >= g_prof.recs.size()) return;
    r = &g_prof.recs[g_prof.used++];
    snprintf(r->name, sizeof(r->name), "%s", name);
    r->flops = flops; r->bytes = bytes;
    (void)hipEventRecord(r->e0, st);
  }
  ~ProfScope() { if (r) (void)hipEventRecord(r->e1, st); }
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------ second-stage reductions
// One launcher per reduction kind: it picks the grid, so every call site - and the raw test entry
// points prh_test_reduce_* - runs the same launch.
//
// out[rows, cols] (ld ldout) = sum over S slabs; with cslab, cout[ccols] = sum over S column-sum
// slabs in the same launch.  An output is one fp64 chain over the slabs, so a short output list
// cannot be spread over more lanes: it takes 64-thread workgroups, one wave per CU.
int reduce_slabs(const float* slab, int S, int rows, int cols, float* out, long ldout, const float* cslab,
                 int ccols, float* cout, hipStream_t st) {
  const long len = (long)rows * cols + (cslab != nullptr ? ccols : 0);
  if (len <= 0) return PRH_OK;
  const int bs = len <= 64 * 256 ? 64 : 256;
  if (cslab != nullptr)
    hipLaunchKernelGGL(slab_reduce2_kernel, dim3((unsigned)cdiv(len, bs)), dim3(bs), 0, st, slab, S, rows, cols, out,
                       ldout, cslab, ccols, cout);
  else
    hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)cdiv(len, bs)), dim3(bs), 0, st, slab, S, rows, cols, out,
                       ldout);
  LAUNCH_CHECK();
  return PRH_OK;
}
// the three cases of a wgrad's slabs: weights and column sums in one launch, or either alone
int reduce_wgrad_slabs(const float* slab, const float* colsum_slab, int S, int Mo, int Ni, float* C, long ldc,
                       float* colsum_out, hipStream_t st) {
  if (C != nullptr && colsum_out != nullptr) return reduce_slabs(slab, S, Mo, Ni, C, ldc, colsum_slab, Mo, colsum_out, st);
  if (C != nullptr) return reduce_slabs(slab, S, Mo, Ni, C, ldc, nullptr, 0, nullptr, st);
  if (colsum_out != nullptr) return reduce_slabs(colsum_slab, S, 1, Mo, colsum_out, (long)Mo, nullptr, 0, nullptr, st);
  return PRH_OK;
}
// BatchNorm statistics stage 1: partials [R][ld] -> slice records out[BN_SLICES][3][N]
int reduce_bn_stage1(const float* ws_a, const float* ws_b, int R, long ld, int N, int tile_rows, int P, int forward,
                     double* out, hipStream_t st) {
  hipLaunchKernelGGL(bn_stage1_kernel, dim3(cdiv(N, 32), BN_SLICES), dim3(256), 0, st, ws_a, ws_b, R, ld, N, tile_rows,
                     P, forward, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
// out_a[c] = sum_i ws_a[i][c], out_b likewise (ws_b may be null; either output may be null)
int reduce_partials(const float* ws_a, const float* ws_b, int R2, int N, float* out_a, float* out_b, hipStream_t st) {
  hipLaunchKernelGGL(partials_reduce_kernel, dim3(cdiv(N, 32)), dim3(1024), 0, st, ws_a, ws_b, R2, N, out_a, out_b);
  LAUNCH_CHECK();
  return PRH_OK;
}
int reduce_ln_param_grad(const float* part_g, const float* part_b, int nb, float* dgamma, float* dbeta, hipStream_t st) {
  hipLaunchKernelGGL(ln_param_grad_kernel, dim3(LN_C / 64), dim3(256), 0, st, part_g, part_b, nb, dgamma, dbeta);
  LAUNCH_CHECK();
  return PRH_OK;
}
int reduce_pos_hidden_final(const float* part, int nblk, int hidden, float* dw0, float* db0, hipStream_t st) {
  hipLaunchKernelGGL(pos_hidden_final_kernel, dim3((unsigned)cdiv(4 * hidden, 16)), dim3(256), 0, st, part, nblk, hidden,
                     dw0, db0);
  LAUNCH_CHECK();
  return PRH_OK;
}
int reduce_partial_rows_final(const float* part, int nblk, int n_el, float* out0, int n0, float* out1, hipStream_t st) {
  hipLaunchKernelGGL(partial_rows_final_kernel, dim3((unsigned)cdiv(n_el, 16)), dim3(256), 0, st, part, nblk, n_el, out0,
                     n0, out1);
  LAUNCH_CHECK();
  return PRH_OK;
}
// amax_slot[0] = max relu(z * scale + shift) from the column maxima / minima ws_c / ws_d [R][ld];
// apart: ABSMAX_MAX_BLOCKS floats.  A layer wider than ABSMAX_MAX_BLOCKS / BN_SLICES 32-column
// blocks has each block walk several column groups.
int reduce_act_amax(const float* ws_c, const float* ws_d, int R, long ld, int N, const float* scale, const float* shift,
                    float* apart, float* amax_slot, hipStream_t st) {
  int gx = cdiv(N, 32);
  gx = gx > ABSMAX_MAX_BLOCKS / BN_SLICES ? ABSMAX_MAX_BLOCKS / BN_SLICES : gx;
  hipLaunchKernelGGL(act_amax_kernel, dim3(gx, BN_SLICES), dim3(256), 0, st, ws_c, ws_d, R, ld, N, scale, shift, apart);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)apart, gx * BN_SLICES, amax_slot);
  LAUNCH_CHECK();
  return PRH_OK;
}

// bump allocator over the caller's workspace (256-B aligned carves).  With base == nullptr
// it only measures: the *_workspace_bytes queries run the SAME carve functions as the entry
// points, so the two can never disagree.
struct Arena {
  char* base; size_t size; size_t off = 0; bool ok = true;
  Arena(void* b, size_t s) : base((char*)b), size(s) {}
  Arena() : base(nullptr), size((size_t)-1) {}
  float* f(size_t n) {
    off = align_up(off, 256);
    const size_t bytes = n * sizeof(float);
    if (base != nullptr && off + bytes > size) { ok = false; return nullptr; }
    float* p = base ? (float*)(base + off) : nullptr;
    off += bytes;
    return p;
  }
};

// Which GEMM core serves a launch.  PRH_GEMM=fp32 forces the exact fp32 MFMA cores
// everywhere; the default "split16" routes large GEMMs to the two-plane fp16 cores (fp32-level
// error, 3 MFMA products per MAC: 5.3x the fp32 matrix ceiling), "split" to the three-plane
// bf16 cores (6 products, no range assumption); small / odd-shaped GEMMs stay on the fp32 cores.
// -1: not initialised, 0: fp32 cores only, 1: split-bf16 (3 planes, 6 products, fp32-accurate)
// for large GEMMs, 2: plain bf16 operands (1 plane) for large GEMMs - reduced precision,
// opt-in only, 3: split-fp16 (2 scaled planes, 3 products, fp32-accurate) for large GEMMs,
// 4: bf16 operands and storage.  An exported entry point reads the mode once and passes Cores down.
const unsigned* g_seed_src = nullptr;   // device word mixed into every dropout seed (prh_set_dropout_seed_source)
int g_gemm_mode = -1;
inline int gemm_mode() {
  if (g_gemm_mode < 0) {
    const char* e = getenv("PRH_GEMM");
    g_gemm_mode = PRH_GEMM_DEFAULT;
    // one spelling table for PRH_GEMM, ops.set_gemm_mode() and bench.py --gemm (ops.GEMM_MODES):
    // fp32 0, split 1, bf16op 2, split16 3, bf16 4 ("bf16s": round-2 alias of mode 4)
    if (e != nullptr && strcmp(e, "fp32") == 0) g_gemm_mode = 0;
    else if (e != nullptr && strcmp(e, "split") == 0) g_gemm_mode = 1;
    else if (e != nullptr && strcmp(e, "bf16op") == 0) g_gemm_mode = 2;
    else if (e != nullptr && strcmp(e, "split16") == 0) g_gemm_mode = 3;
    else if (e != nullptr && (strcmp(e, "bf16") == 0 || strcmp(e, "bf16s") == 0)) g_gemm_mode = 4;
  }
  return g_gemm_mode;
}
// What one call runs on.  core: the family of the generic fp32-storage launchers (launch_nt /
// launch_tn), 0 fp32, 1 three bf16 planes, 2 one bf16 plane, 3 split-fp16.  Mode 4 has its own
// encoder / Linear entry points; odd shapes that still reach the generic launchers are served like
// mode 2, the point_mlp stack like mode 3 (stack_cores).
struct Cores {
  int mode, core;
  bool split() const { return core != 0; }      // large GEMMs may leave the fp32 cores
  // Attention cores: 16-bit MFMA (two fp16 planes / three products) in every GEMM mode but 0, the bf16
  // modes included: at B=4096 one bf16 plane saved 12 ms of a 300 ms step and tripled the worst
  // per-tensor gradient error (0.29 against 0.064 vs the exact cores).  GEMM mode 0 keeps the exact
  // fp32 MFMA kernels.  -1: exact fp32 kernels; 0: two fp16 planes
  int attn_prec() const { return mode == 0 ? -1 : 0; }
  const char* tag() const { return core == 2 ? "b1" : (core == 3 ? "h2" : "s3"); }
};
inline Cores cores_of(int mode) { return Cores{mode, mode == 4 ? 2 : mode}; }
// the point_mlp stack, i.e. the line encoder (Conv1d(3,64) on coordinates of +-25 m, src/model.py:150-152):
// in mode 4 it keeps fp32-accurate operands on the split-fp16 cores - 131 k rows at B=4096, nothing
// to gain from 8-bit mantissas
inline Cores stack_cores(int mode) { return mode == 4 ? Cores{4, 3} : cores_of(mode); }
// PRH_H2_PP=1: phase-split ("ping-pong") k-loop of the second-generation NT core (prh_gemm_h2.hpp)
bool g_h2_pp = [] { const char* e = getenv("PRH_H2_PP"); return e && strcmp(e, "1") == 0; }();

// largest |pro(A)| over [rows, cols] into *slot; part: ABSMAX_MAX_BLOCKS floats of scratch
template <int PRO>
int measure_absmax(const float* A, long lda, const float* A2, long lda2, const float* pa,
                   const float* pb, const float* pc, long rows, int cols, float* slot, float* part,
                   hipStream_t st) {
  if (rows <= 0 || cols <= 0) {
    hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, part, 0, slot);
    LAUNCH_CHECK();
    return PRH_OK;
  }
  const int vec = ((cols & 3) == 0 && (PRO == PRO_GATE1 || (lda & 3) == 0) &&
                   (PRO != PRO_BNBWD || (lda2 & 3) == 0)) ? 1 : 0;
  long blocks = cdiv(rows, 4L * 8);      // >= 8 rows per thread column, at most 8 blocks per CU
  blocks = blocks < 1 ? 1 : (blocks > ABSMAX_MAX_BLOCKS ? ABSMAX_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL((absmax_kernel<PRO>), dim3((unsigned)blocks), dim3(256), 0, st, A, lda, A2, lda2,
                     pa, pb, pc, rows, cols, vec, part);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, part, (int)blocks, slot);
  LAUNCH_CHECK();
  return PRH_OK;
}
inline bool nt_use_s3(Cores c, int M, int N, int K) {
  // K cap: coefficient LDS image.  Grid floor: a 256x256-tile grid of a few workgroups is
  // latency-bound (53 us for 4 workgroups measured); small GEMMs go to the 128x128 fp32 core.
  return c.split() && K >= 64 && K <= 4096 && N >= 128 && M >= 512 &&
         (long)cdiv(M, S3_BM) * cdiv(N, S3_BN) >= 32;
}
// Does the intensity-gate launch <PRO_GATE1, EPI_GATE> over [P, od] (K = 64) land on the second-generation
// split-fp16 core with the vector epilogue?  Only there can the backward compute the gate again
// (<PRO_GATE1, EPI_GATE_BWD>) with the forward's bits; mirrors the conditions of launch_nt_core.
inline bool gate_on_h2(Cores c, int P, int od, int in_channel) {
  return c.mode == 3 && c.core == 3 && nt_use_s3(c, P, od, 64) && (od & 3) == 0 && in_channel <= 65536;
}
inline bool tn_use_s3(Cores c, int P, int Mo, int Ni) { return c.split() && Mo >= 128 && Ni >= 64 && P >= 8192; }

// dy <- dz in place (split-fp16 mode), largest |dz| into hdr[0]; hdr: S3_HDR_FLOATS floats
int materialize_dz(float* dy, long lddy, const float* z, long ldz, const float* ka, const float* kb,
                   const float* kc, long rows, int cols, float* hdr, hipStream_t st) {
  long blocks = cdiv(rows, 4L * 8);
  blocks = blocks < 1 ? 1 : (blocks > ABSMAX_MAX_BLOCKS ? ABSMAX_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dy, lddy, z, ldz, ka,
                     kb, kc, rows, cols, hdr + 64);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, hdr + 64, (int)blocks, hdr);
  LAUNCH_CHECK();
  return PRH_OK;
}
// dz is materialised when the layer is aligned for 16-B accesses and the split-fp16 cores are on
inline bool dz_in_place(Cores c, int cols, long lddy, long ldz) {
  return c.core == 3 && (cols & 3) == 0 && (lddy & 3) == 0 && (ldz & 3) == 0;
}

// Statistics partials: `count` tiles of `rows` rows each
struct StatInfo { int count = 0; int rows = 64; long ld = 0; long off = 0; };   // ld 0: = layer width
inline int stat_tiles_max(int P) { return 2 * cdiv(P, BM); }   // largest count any producer writes

template <typename K, typename... More>
int allow_big_lds(K kernel, More... more) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if constexpr (sizeof...(more) > 0) return allow_big_lds(more...);
  else return PRH_OK;
}
// dynamic LDS of the NT split core: two stages + the prologue coefficient vectors
inline size_t nt_s3_lds(int K, int pro) {
  const int KP = (cdiv(K, S3_BK) + 2) * S3_BK;
  return (size_t)S3_LDS + (pro == PRO_NONE ? 0 : (pro == PRO_BNBWD ? 3 : 2) * (size_t)KP * 4);
}
// the split cores' launch sites; launch_nt / launch_tn pick the plane count from Cores::core:
// one bf16 plane (2), two fp16 planes (3), three bf16 planes (1)
template <int PRO, int EPI, int PLANES>
void launch_nt_s3(const NTParams& p, long tiles, const char* img, hipStream_t st) {
  hipLaunchKernelGGL((gemm_nt_s3_kernel<PRO, EPI, PLANES>), dim3((unsigned)tiles), dim3(512), nt_s3_lds(p.K, PRO), st, p, img);
}
template <int PROA, int PROB, int PLANES>
void launch_tn_s3(const TNParams& p, long blocks, hipStream_t st) {
  hipLaunchKernelGGL((gemm_tn_s3_kernel<PROA, PROB, PLANES>), dim3((unsigned)blocks), dim3(512), S3_LDS, st, p);
}
static_assert(8 * 32 * EPI_LDW * 4 <= S3_LDS, "epilogue scratch must fit in the stage buffers");

// ------------------------------------------------------------------ bf16 mode launchers (prh_b16.hpp)
// C[M,N] = pro(A) W^T on the bf16 NT core.  A bf16 (A16) or fp32, C / C2 / matrix E1 bf16 (C16)
// or fp32.  p.wprep must hold b16_weight_bytes(N, K).  Leading dimensions in elements.
// dynamic LDS of the bf16 NT core: two stages + (with a prologue) the two coefficient vectors
inline size_t nt_b16_lds(int K, int pro) {
  return (size_t)H2_LDS + (pro == PRO_NONE ? 0 : 2 * (size_t)(cdiv(K, B16_BK) + 2) * B16_BK * 4);
}
inline bool nt_b16_depth_ok(int K, int pro) { return nt_b16_lds(K, pro) <= 160 * 1024; }
template <int PRO, int EPI, bool A16, bool C16>
int launch_nt_b16(NTParams& p, hipStream_t st, StatInfo* si = nullptr) {
  if (p.M <= 0 || p.N <= 0) return PRH_OK;
  const bool rowvec = (p.flags & F_E1_ROWVEC) != 0;
  if ((p.K & 7) || (PRO != PRO_GATE1 && (p.lda & (A16 ? 7 : 3))) || (p.ldw & 3) || (p.N & 3) || (p.ldc & 3) ||
      (p.E1 != nullptr && !rowvec && (p.lde1 & 3)) || (p.C2 != nullptr && (p.ldc2 & 3)) || p.wprep == nullptr)
    return fail(PRH_ERR_ARG, "gemm_nt_b16: K %% 8, N %% 4 and aligned leading dimensions required (K=%d N=%d lda=%ld ldc=%ld)",
                p.K, p.N, p.lda, p.ldc);
  if (rowvec && C16) return fail(PRH_ERR_ARG, "gemm_nt_b16: a row-vector E1 comes with fp32 outputs");
  const int KT = cdiv(p.K, B16_BK), NTl = cdiv(p.N, 256);
  const size_t lds = nt_b16_lds(p.K, PRO);
  if (!nt_b16_depth_ok(p.K, PRO)) return fail(PRH_ERR_ARG, "gemm_nt_b16: K=%d too deep for the prologue coefficient image", p.K);
  const long th = (long)NTl * 256 * KT * 8;
  hipLaunchKernelGGL(prep_weights_b16_kernel, dim3((unsigned)cdiv(th, 256)), dim3(256), 0, st, p.W, p.N, p.K, p.ldw,
                     p.wprep + S3_WHDR);
  LAUNCH_CHECK();
  p.tiles_n = NTl;
  static const int attr = allow_big_lds(gemm_nt_b16_kernel<PRO, EPI, A16, C16>);
  if (attr != PRH_OK) return attr;
  char nm[64];
  snprintf(nm, sizeof(nm), "gemm_nt_b16<%d,%d> K=%d N=%d", PRO, EPI, p.K, p.N);
  const double ea = A16 ? 2.0 : 4.0, ec = C16 ? 2.0 : 4.0;
  const double by = ea * (double)p.M * p.K * (PRO == PRO_GATE1 ? 0 : 1) +
                    ec * (double)p.M * p.N * (EPI == EPI_GATE ? 3 : (EPI == EPI_DGRAD ? 2 : 1)) + 4.0 * (double)p.N * p.K;
  ProfScope ps(nm, 2.0 * p.M * (double)p.N * p.K, by, st);
  if constexpr (PRO == PRO_NONE && A16) {
    // plain bf16 operand: both operands by LDS-DMA, phase-split loop (gemm_nt_b16d_kernel)
    if ((p.K % B16_BK) == 0 && (reinterpret_cast<uintptr_t>(p.A) & 15) == 0) {
      static const int attr_d = allow_big_lds(gemm_nt_b16d_kernel<EPI, C16>);
      if (attr_d != PRH_OK) return attr_d;
      hipLaunchKernelGGL((gemm_nt_b16d_kernel<EPI, C16>), dim3((unsigned)(NTl * cdiv(p.M, 256))), dim3(512), (size_t)B16D_LDS, st,
                         p, (const char*)(p.wprep + S3_WHDR));
      LAUNCH_CHECK();
      if (si) { si->count = 2 * cdiv(p.M, 256); si->rows = 128; }
      return PRH_OK;
    }
  }
  hipLaunchKernelGGL((gemm_nt_b16_kernel<PRO, EPI, A16, C16>), dim3((unsigned)(NTl * cdiv(p.M, 256))), dim3(512), lds, st,
                     p, (const char*)(p.wprep + S3_WHDR));
  LAUNCH_CHECK();
  if (si) { si->count = 2 * cdiv(p.M, 256); si->rows = 128; }
  return PRH_OK;
}
inline bool nt_b16_generic_ok(const NTParams& p) {      // fp32-storage Linear served by the bf16 core in mode 4
  return p.wprep != nullptr && (p.K & 7) == 0 && p.K >= 64 && p.K <= 8192 && (p.lda & 3) == 0 && (p.N & 3) == 0 &&
         (p.ldc & 3) == 0 && (p.E1 == nullptr || (p.lde1 & 3) == 0) && p.M >= 512 && p.N >= 64 &&
         (long)cdiv(p.M, 256) * cdiv(p.N, 256) >= 16;
}

struct TNPlan16 { int tiles_m, tiles_n, splits, rows_per_split; };
inline TNPlan16 tn_plan_b16(int P, int Mo, int Ni, long maxld) {
  TNPlan16 pl;
  pl.tiles_m = cdiv(Mo, 256); pl.tiles_n = cdiv(Ni, 256);
  const int tiles = pl.tiles_m * pl.tiles_n;
  int s = cdiv(P >= 262144 ? 768 : 256, tiles);
  int best = s; double bw = 1e9;       // whole rounds of the 256 CUs (see tn_plan)
  for (int c = (s > 3 ? s - 2 : 1); c <= s + 4; ++c) {
    const double blocks = (double)tiles * c, w = (double)cdiv((long)blocks, 256L) * 256.0 / blocks;
    if (w < bw - 1e-3) { bw = w; best = c; }
  }
  s = best;
  const int smax = cdiv(P, 512) < 1 ? 1 : cdiv(P, 512);
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  int rps = cdiv(cdiv(P, s), TB_BK) * TB_BK;
  if (rps < TB_BK) rps = TB_BK;
  const int cap = (int)((2147483647L / (4L * (maxld < 4 ? 4 : maxld))) / TB_BK * TB_BK);   // 32-bit buffer offsets
  if (rps > cap) rps = cap;
  pl.splits = cdiv(P, rps) < 1 ? 1 : cdiv(P, rps);
  pl.rows_per_split = rps;
  return pl;
}
inline size_t tn16_splits_bound(int P, int Mo, int Ni) {
  const size_t a = (size_t)tn_plan_b16(P, Mo, Ni, 4).splits, b = (size_t)tn_plan_b16(P, Mo, Ni, 8192).splits;
  return a > b ? a : b;
}
inline size_t tn16_slab_floats(int P, int Mo, int Ni) { return tn16_splits_bound(P, Mo, Ni) * Mo * Ni + ABSMAX_MAX_BLOCKS + 64; }
inline size_t tn16_colsum_floats(int P, int Mo, int Ni) { return tn16_splits_bound(P, Mo, Ni) * Mo; }

// C[Mo,Ni] (ld ldc) = A^T proB(B), A [P,Mo] bf16, B [P,Ni] bf16 (GATE1: fp32 scalar per row);
// colsum_out[Mo] = column sums of A (optional).  Slabs are fp32, summed in fp64.
template <int PROB>
int launch_tn_b16(TNParams& p, float* slab, float* colsum_slab, float* C, long ldc, float* colsum_out, hipStream_t st) {
  if (p.Mo <= 0 || p.Ni <= 0) return PRH_OK;
  if ((p.Mo & 7) || (p.Ni & 7) || (p.lda & 7) || (PROB != PRO_GATE1 && (p.ldb & 7)))
    return fail(PRH_ERR_ARG, "gemm_tn_b16: Mo, Ni and the leading dimensions must be multiples of 8 (Mo=%d Ni=%d)", p.Mo, p.Ni);
  long maxld = p.lda > p.ldb ? p.lda : p.ldb;
  const TNPlan16 pl = tn_plan_b16(p.P, p.Mo, p.Ni, maxld);
  p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.splits = pl.splits; p.rows_per_split = pl.rows_per_split;
  p.slab = slab;
  p.colsum = colsum_out != nullptr ? colsum_slab : nullptr;
  p.pace = nullptr;
  if (pl.tiles_m * pl.tiles_n >= 8 && pl.splits <= ABSMAX_MAX_BLOCKS && pl.rows_per_split >= 16384) {
    p.pace = reinterpret_cast<int*>(slab + (size_t)pl.splits * p.Mo * p.Ni + 64);
    if (hipMemsetAsync(p.pace, 0, sizeof(int) * pl.splits, st) != hipSuccess)
      return fail(PRH_ERR_HIP, "gemm_tn_b16: memset of the pacing counters failed");
  }
  const long blocks = (long)pl.tiles_m * pl.tiles_n * pl.splits;
  static const int attr = allow_big_lds(gemm_tn_b16_kernel<PROB>);
  if (attr != PRH_OK) return attr;
  {
    char nm[64];
    snprintf(nm, sizeof(nm), "gemm_tn_b16<0,%d> Mo=%d Ni=%d", PROB, p.Mo, p.Ni);
    const double by = 2.0 * (double)p.P * p.Mo + (PROB == PRO_GATE1 ? 4.0 * p.P : 2.0 * (double)p.P * p.Ni) + 4.0 * (double)p.Mo * p.Ni;
    ProfScope ps(nm, 2.0 * p.P * (double)p.Mo * p.Ni, by, st);
    hipLaunchKernelGGL((gemm_tn_b16_kernel<PROB>), dim3((unsigned)blocks), dim3(512), TB_LDS, st, p);
    LAUNCH_CHECK();
  }
  return reduce_wgrad_slabs(slab, colsum_slab, pl.splits, p.Mo, p.Ni, C, ldc, colsum_out, st);
}

// ------------------------------------------------------------------ small-problem cores
inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
// launches the 128 x 128 tiling would turn into less than ~3/4 of a round of workgroups
inline bool small_nt_ok(const NTParams& p, bool nn) {
  if (p.M < 1 || (p.K % SM_BK) != 0 || (p.lda & 3) || (p.ldw & 3) || !al16(p.A) || !al16(p.W)) return false;
  if ((long)cdiv(p.M, BM) * cdiv(p.N, BN) >= 192) return false;
  if (nn && (p.N & 31)) return false;
  return true;
}
template <int TM, int TN, int KS, bool NN, int EPI = EPI_BIAS>
int launch_small_cfg(NTParams& p, hipStream_t st) {
  static const int attr = allow_big_lds(gemm_small_kernel<TM, TN, KS, NN, EPI>);
  if (attr != PRH_OK) return attr;
  p.tiles_n = cdiv(p.N, TN * 32);
  const long tiles = (long)p.tiles_n * cdiv(p.M, TM * 32);
  char nm[64];
  snprintf(nm, sizeof(nm), "gemm_small<%d%d%d,%s,%d> K=%d N=%d", TM, TN, KS, NN ? "nn" : "nt", EPI, p.K, p.N);
  const double by = 4.0 * ((double)p.M * p.K + (double)p.M * p.N * ((p.flags & F_RESID) || EPI == EPI_DGRAD ? 2 : 1) + (double)p.N * p.K);
  ProfScope ps(nm, 2.0 * p.M * (double)p.N * p.K, by, st);
  hipLaunchKernelGGL((gemm_small_kernel<TM, TN, KS, NN, EPI>), dim3((unsigned)tiles), dim3(256), (small_lds<TM, TN, KS>()), st, p);
  LAUNCH_CHECK();
  return PRH_OK;
}
template <bool NN, int EPI = EPI_BIAS>
int launch_small(NTParams& p, hipStream_t st) {
  p.flags &= ~F_POOL;
  const bool n64 = !NN || (p.N & 63) == 0;
  if (n64 && (long)cdiv(p.M, 64) * cdiv(p.N, 64) >= 192) return launch_small_cfg<2, 2, 1, NN, EPI>(p, st);
  if (n64 && (long)cdiv(p.M, 32) * cdiv(p.N, 64) >= 192) return launch_small_cfg<1, 2, 2, NN, EPI>(p, st);
  return launch_small_cfg<1, 1, 4, NN, EPI>(p, st);
}
// wgrad: 64 x 64 tiles, rows split in multiples of 64 until ~2 rounds of workgroups exist
constexpr int TN_SMALL_MAX_P = 16384;
inline bool small_tn_dims_ok(int P, int Mo, int Ni) {
  return P >= 64 && P <= TN_SMALL_MAX_P && (P & 63) == 0 && (Mo & 63) == 0 && (Ni & 63) == 0;
}
inline void small_tn_plan(int P, int Mo, int Ni, int& splits, int& rps) {
  const int tiles = (Mo / 64) * (Ni / 64), chunks = P / 64;
  int s = cdiv(512, tiles);
  s = s > chunks ? chunks : (s < 1 ? 1 : s);
  rps = cdiv(chunks, s) * 64;
  splits = cdiv(P, rps);
}

// ------------------------------------------------------------------ launch helpers
// amax_part (plain EPI_BIAS launches): scratch of nt_amax_part_floats(M, N) floats; when the launch lands on
// the second-generation split-fp16 core it runs the instantiation whose epilogue keeps the largest |C| it
// stores, one partial per workgroup, and *amax_tiles is their number (0: this core has no such epilogue)
inline size_t nt_amax_part_floats(int M, int N) {
  const size_t t = (size_t)cdiv(M < 1 ? 1 : M, S3_BM) * cdiv(N < 1 ? 1 : N, S3_BN);
  return (t > (size_t)ABSMAX_MAX_BLOCKS ? t : (size_t)ABSMAX_MAX_BLOCKS) + 64;
}
template <int PRO, int EPI>
int launch_nt_core(Cores c, NTParams& p, hipStream_t st, StatInfo* si, float* amax_part, long* amax_tiles) {   // p.amaxA is filled in when measured
  if (p.M <= 0 || p.N <= 0) return PRH_OK;
  if ((p.K & 3) || (PRO != PRO_GATE1 && (p.lda & 3)) || (p.ldw & 3) ||
      (PRO == PRO_BNBWD && (p.lda2 & 3)))
    return fail(PRH_ERR_ARG, "gemm_nt: K/lda/ldw must be multiples of 4 (K=%d lda=%ld ldw=%ld)",
                p.K, p.lda, p.ldw);
  if constexpr (PRO == PRO_NONE && EPI == EPI_BIAS) {     // a mode-4 Linear (not the point_mlp stack)
    if (c.mode == 4 && c.core == 2 && nt_b16_generic_ok(p)) return launch_nt_b16<PRO_NONE, EPI_BIAS, false, false>(p, st, si);
  }
  // F_POOL is honoured by the vector epilogue only: cleared here, set again by the branch that
  // launches a kernel with that epilogue, so the caller can tell whether the partials exist
  const bool want_pool = (p.flags & F_POOL) != 0;
  p.flags &= ~F_POOL;
  char nm[64];
  // algorithmic traffic: A (+A2) read once, C written once (+E1/C_old reads), W read once
  const double by = 4.0 * ((double)p.M * p.K * (PRO == PRO_BNBWD ? 2 : (PRO == PRO_GATE1 ? 0 : 1)) +
                           (double)p.M * p.N * (EPI == EPI_GATE_BWD ? 4 : (EPI == EPI_GATE ? 3 : (EPI == EPI_DGRAD ? 2 : 1))) +
                           (double)p.N * p.K);
  {
    if (p.wprep != nullptr && nt_use_s3(c, p.M, p.N, p.K) && p.lda <= 65536 && p.lda2 <= 65536 &&
        !((EPI == EPI_GATE || EPI == EPI_GATE_BWD) && ((p.N | (int)p.ldc | (int)p.lde1 | (int)p.ldc2) & 3) != 0)) {
      const int KT = cdiv(p.K, S3_BK), NTl = cdiv(p.N, S3_BN);
      const long th = (long)NTl * 256 * KT * 2;
      float* hdr = reinterpret_cast<float*>(p.wprep);
      const char* img = p.wprep + S3_WHDR;
      if (c.core == 3) {      // operand scales of the fp16-plane core
        if (p.amaxW == nullptr) {
          TRY_RC((measure_absmax<PRO_NONE>(p.W, p.ldw, nullptr, 0, nullptr, nullptr, nullptr, p.N, p.K, hdr, hdr + 64, st)));
          p.amaxW = hdr;
        }
        if (p.amaxA == nullptr) {
          TRY_RC((measure_absmax<PRO>(p.A, p.lda, p.A2, p.lda2, p.pa, p.pb, p.pc, p.M, p.K, hdr + 1, hdr + 64, st)));
          p.amaxA = hdr + 1;
        }
      }
      // second-generation split-fp16 core (16x16x32 MFMA, 32-deep k-tiles): plain / BN+ReLU /
      // gate prologues with a 16-B aligned output; anything else stays on the first generation
      if constexpr (PRO == PRO_NONE || PRO == PRO_BNRELU || PRO == PRO_GATE1) {
        const bool vec_ok = ((p.N | (int)p.ldc) & 3) == 0 && (p.E1 == nullptr || ((int)p.lde1 & 3) == 0) &&
                            (p.flags & F_E1_ROWVEC) == 0 && (p.C2 == nullptr || ((int)p.ldc2 & 3) == 0);
        const int KT2 = cdiv(p.K, H2_BK);
        const size_t lds = (size_t)H2_LDS + (PRO == PRO_NONE ? 0 : 2 * (size_t)(KT2 + 2) * H2_BK * 4);
        if (c.core == 3 && vec_ok && lds <= 160 * 1024) {
          const long th2 = (long)NTl * 256 * KT2 * 4;
          hipLaunchKernelGGL(prep_weights_h2_kernel, dim3((unsigned)cdiv(th2, 256)), dim3(256), 0, st, p.W,
                             p.N, p.K, p.ldw, p.wprep + S3_WHDR, p.amaxW);
          LAUNCH_CHECK();
          p.tiles_n = NTl;
          if (want_pool) p.flags |= F_POOL;
          static const int attr_h2 = allow_big_lds(gemm_nt_h2_kernel<PRO, EPI>, gemm_nt_h2_kernel<PRO, EPI, true>);
          if (attr_h2 != PRH_OK) return attr_h2;
          snprintf(nm, sizeof(nm), "gemm_nt_h2<%d,%d> K=%d N=%d", PRO, EPI, p.K, p.N);
          ProfScope ps(nm, 2.0 * p.M * (double)p.N * p.K, by, st);
          if constexpr (PRO == PRO_NONE && EPI == EPI_BIAS) {
            if (amax_part != nullptr) {
              static const int attr_am = allow_big_lds(gemm_nt_h2_kernel<PRO, EPI, false, true>);
              if (attr_am != PRH_OK) return attr_am;
              const long wgs = (long)NTl * cdiv(p.M, 256);
              p.ws_a = amax_part;
              hipLaunchKernelGGL((gemm_nt_h2_kernel<PRO, EPI, false, true>), dim3((unsigned)wgs), dim3(512), lds, st, p, img);
              LAUNCH_CHECK();
              *amax_tiles = wgs;
              return PRH_OK;
            }
          }
          if (g_h2_pp)
            hipLaunchKernelGGL((gemm_nt_h2_kernel<PRO, EPI, true>), dim3((unsigned)(NTl * cdiv(p.M, 256))), dim3(512),
                               lds, st, p, img);
          else
            hipLaunchKernelGGL((gemm_nt_h2_kernel<PRO, EPI>), dim3((unsigned)(NTl * cdiv(p.M, 256))), dim3(512),
                               lds, st, p, img);
          LAUNCH_CHECK();
          if (si) { si->count = 2 * cdiv(p.M, S3_BM); si->rows = 128; }
          return PRH_OK;
        }
      }
      if constexpr (EPI != EPI_GATE_BWD) {
        hipLaunchKernelGGL(prep_weights_s3_kernel, dim3((unsigned)cdiv(th, 256)), dim3(256), 0, st,
                           p.W, p.N, p.K, p.ldw, 0, p.wprep + S3_WHDR, c.core == 3 ? p.amaxW : nullptr);
        LAUNCH_CHECK();
        p.tiles_n = NTl;
        const long tiles = (long)NTl * cdiv(p.M, S3_BM);
        static const int attr_rc = allow_big_lds(gemm_nt_s3_kernel<PRO, EPI, 3>, gemm_nt_s3_kernel<PRO, EPI, 1>,
                                                 gemm_nt_s3_kernel<PRO, EPI, 2>);
        if (attr_rc != PRH_OK) return attr_rc;
        snprintf(nm, sizeof(nm), "gemm_nt_%s<%d,%d> K=%d N=%d", c.core == 3 ? "h2g1" : c.tag(), PRO, EPI, p.K, p.N);
        ProfScope ps(nm, 2.0 * p.M * (double)p.N * p.K, by, st);
        switch (c.core) {
          case 2: launch_nt_s3<PRO, EPI, 1>(p, tiles, img, st); break;
          case 3: launch_nt_s3<PRO, EPI, 2>(p, tiles, img, st); break;
          default: launch_nt_s3<PRO, EPI, 3>(p, tiles, img, st);
        }
        LAUNCH_CHECK();
        if (si) { si->count = 2 * cdiv(p.M, S3_BM); si->rows = 128; }
        return PRH_OK;
      }
    }
  }
  // the gate backward exists on the second-generation split-fp16 core only (gate_on_h2 says when): its
  // caller runs combine_bwd_kernel on a stored gate everywhere else
  if constexpr (EPI == EPI_GATE_BWD) {
    return fail(PRH_ERR_ARG, "gemm_nt: the gate-recompute backward needs the split-fp16 core (M=%d N=%d)", p.M, p.N);
  } else {
    if constexpr (PRO == PRO_NONE && EPI == EPI_BIAS) {
      if (small_nt_ok(p, false)) return launch_small<false>(p, st);
    }
    p.tiles_n = cdiv(p.N, BN);
    const long tiles = (long)p.tiles_n * cdiv(p.M, BM);
    snprintf(nm, sizeof(nm), "gemm_nt<%d,%d> K=%d N=%d", PRO, EPI, p.K, p.N);
    ProfScope ps(nm, 2.0 * p.M * (double)p.N * p.K, by, st);
    if (p.N <= 64)      // one column tile: 64 x 32 wave tiles
      hipLaunchKernelGGL((gemm_nt_kernel<PRO, EPI, true>), dim3((unsigned)tiles), dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((gemm_nt_kernel<PRO, EPI>), dim3((unsigned)tiles), dim3(256), 0, st, p);
    LAUNCH_CHECK();
    if (si) { si->count = 2 * cdiv(p.M, BM); si->rows = 64; }
    return PRH_OK;
  }
}

// amax_out: the largest |C| of the launch is valid there on return - from the epilogue where the core has that
// form, else from a read pass over C (small core, first-generation and fp32 cores, modes other than 3)
template <int PRO, int EPI>
int launch_nt(Cores c, NTParams& p, hipStream_t st, StatInfo* si = nullptr, float* amax_out = nullptr,
              float* amax_part = nullptr) {
  long tiles = 0;
  TRY_RC((launch_nt_core<PRO, EPI>(c, p, st, si, amax_part, &tiles)));
  if (amax_out == nullptr) return PRH_OK;
  if (tiles > 0) {
    hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)amax_part, (int)tiles, amax_out);
    LAUNCH_CHECK();
    return PRH_OK;
  }
  return measure_absmax<PRO_NONE>(p.C, p.ldc, nullptr, 0, nullptr, nullptr, nullptr, p.M, p.N, amax_out, amax_part, st);
}

constexpr int TN_S3_MAX_LD = 4096;   // widest operand row the split TN core accepts
struct TNPlan { int tiles_m, tiles_n, splits, rows_per_split; bool s3; };
inline TNPlan tn_plan(Cores c, int P, int Mo, int Ni, bool allow_s3, long maxld = TN_S3_MAX_LD) {
  TNPlan pl;
  pl.s3 = allow_s3 && tn_use_s3(c, P, Mo, Ni);
  const int tile = pl.s3 ? 256 : 128, bk = pl.s3 ? S3_BK : BK;
  pl.tiles_m = cdiv(Mo, tile);
  pl.tiles_n = cdiv(Ni, tile);
  const int tiles = pl.tiles_m * pl.tiles_n;
  // three rounds of workgroups where the GEMM is long; one where the slab reduction that follows
  // (splits x Mo x Ni floats) would cost a sizeable part of it (P < 256 k rows)
  int s = cdiv(pl.s3 ? (P >= 262144 ? 768 : 256) : 1024, tiles);
  if (pl.s3) {
    // one workgroup per CU: the launch runs in rounds of 256 workgroups, so pick the split
    // count near the target whose last round is fullest (33 splits x 32 tiles = 4.1 rounds
    // cost the fusion wgrad 17 % at B=4096)
    int best = s; double bw = 1e9;
    for (int c = (s > 3 ? s - 2 : 1); c <= s + 4; ++c) {
      const double blocks = (double)tiles * c, w = (double)cdiv((long)blocks, 256L) * 256.0 / blocks;
      if (w < bw - 1e-3) { bw = w; best = c; }
    }
    s = best;
  }
  const int minrows = pl.s3 ? 512 : 128;
  const int smax = cdiv(P, minrows) < 1 ? 1 : cdiv(P, minrows);
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  int rps = cdiv(P, s);
  rps = cdiv(rps, bk) * bk;
  if (rps < bk) rps = bk;
  // the split core addresses a split's rows through 32-bit buffer offsets: keep
  // rows_per_split * leading_dimension * 4 below 2^31 for any ld <= TN_S3_MAX_LD
  const int cap = (int)((2147483647L / (4L * (maxld < 4 ? 4 : maxld))) / bk * bk);
  if (pl.s3 && rps > cap) rps = cap;
  pl.splits = cdiv(P, rps) < 1 ? 1 : cdiv(P, rps);
  pl.rows_per_split = rps;
  return pl;
}
// floats behind a slab: [0] largest |proA(A)|, [1] largest |proB(B)|, [64..) per-block maxima
constexpr int TN_HDR = S3_HDR_FLOATS;
inline size_t tn_splits_bound(Cores cores, int P, int Mo, int Ni) {   // over both cores and any leading dimension
  const size_t a = (size_t)tn_plan(cores, P, Mo, Ni, true).splits, b = (size_t)tn_plan(cores, P, Mo, Ni, false).splits;
  size_t c = (size_t)tn_plan(cores, P, Mo, Ni, true, 4).splits;
  if (small_tn_dims_ok(P, Mo, Ni)) {
    int ss, rr; small_tn_plan(P, Mo, Ni, ss, rr);
    if ((size_t)ss > c) c = (size_t)ss;
  }
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
inline size_t tn_slab_floats(Cores c, int P, int Mo, int Ni) { return tn_splits_bound(c, P, Mo, Ni) * Mo * Ni + TN_HDR; }
inline size_t tn_colsum_floats(Cores c, int P, int Mo, int Ni) { return tn_splits_bound(c, P, Mo, Ni) * Mo; }

// Can the wgrad p (plain A, B plain or BN+ReLU) carry the side job s?  True exactly when launch_tn
// serves p on the transposed-read core and the job fits it: one partial maximum per workgroup,
// 16-B accesses, coefficients within the LDS image, 32-bit offsets within a row group.
inline bool tn_side_ok(Cores c, const TNParams& p, const TNSide& s) {
  if (c.core != 3 || p.Mo <= 0 || p.Ni <= 0) return false;
  if (p.lda > TN_S3_MAX_LD || p.ldb > TN_S3_MAX_LD || p.lda2 > TN_S3_MAX_LD) return false;
  const TNPlan pl = tn_plan(c, p.P, p.Mo, p.Ni, true, p.lda > p.ldb ? p.lda : p.ldb);
  if (!pl.s3 || ((p.Mo | p.Ni | (int)p.lda | (int)p.ldb) & 3) != 0) return false;
  if ((long)pl.tiles_m * pl.tiles_n * pl.splits > ABSMAX_MAX_BLOCKS) return false;
  return s.dy != nullptr && s.z != nullptr && s.part != nullptr && s.amax != nullptr && s.rows > 0 && s.cols > 0 &&
         s.cols <= TR_SIDE_MAX_COLS && ((s.cols | (int)s.lddy | (int)s.ldz) & 3) == 0 && s.lddy <= 65536 &&
         s.ldz <= 65536 && al16(s.dy) && al16(s.z);
}

// k-tiles between two items of a thread's side walk: the largest of 4, 2, 1 at which the launch's
// waves, one item each per period over a split's k-tiles, still reach every item of the job -
// the job spread over the whole k-loop instead of packed into the head of it.  Counted over the
// launch (period * items <= k-tiles * waves), not per wave with the items rounded up: at B=4096
// the fusion wgrad has 2730.67 items per wave for 10923 k-tiles, and a rounded-up 2731 would
// halve its period for the sake of one item, which the drain takes.  A job larger than its
// carrier's k-loop runs at 1 and drains the rest, as it always has.
inline int tn_side_period(const TNPlan& pl, const TNSide& s) {
  const int c4s = s.cols >> 2;
  int lpr = 64;                                          // lanes per row, as in the kernel
  while (lpr > 1 && (lpr >> 1) >= c4s) lpr >>= 1;
  const long rpw = 64 / lpr, groups = (s.rows + rpw - 1) / rpw, chunks = (c4s + 63) >> 6;
  const long items = groups * chunks;
  const long slots = (long)(pl.rows_per_split / S3_BK) * pl.tiles_m * pl.tiles_n * pl.splits * 8;
  return 4 * items <= slots ? 4 : (2 * items <= slots ? 2 : 1);
}
template <int PROB, int Q>
int launch_tn_tr_side(const TNParams& p, long blocks, hipStream_t st) {
  static const int attr_sd = allow_big_lds(gemm_tn_tr_kernel<PROB, true, Q>);
  if (attr_sd != PRH_OK) return attr_sd;
  hipLaunchKernelGGL((gemm_tn_tr_kernel<PROB, true, Q>), dim3((unsigned)blocks), dim3(512),
                     TR_LDS + tr_side_lds(p.side.cols), st, p);
  LAUNCH_CHECK();
  return PRH_OK;
}

// C[Mo,Ni] (ld ldc) = proA(A)^T proB(B); colsum_out[Mo] = column sums of proA(A) (optional)
template <int PROA, int PROB>
int launch_tn(Cores c, TNParams& p, float* slab, float* colsum_slab, float* C, long ldc, float* colsum_out,
              hipStream_t st) {   // p.amaxA / p.amaxB are filled in when the fp16-plane core measured them
  const bool side = p.side.dy != nullptr;     // a missing carrier is an error, never a skipped pass
  if (side && !((PROA == PRO_NONE && (PROB == PRO_NONE || PROB == PRO_BNRELU)) && tn_side_ok(c, p, p.side)))
    return fail(PRH_ERR_ARG, "gemm_tn: this launch cannot carry a side job (Mo=%d Ni=%d P=%d)", p.Mo, p.Ni, p.P);
  if (p.Mo <= 0 || p.Ni <= 0) return PRH_OK;
  const bool ld_ok = p.lda <= TN_S3_MAX_LD && p.ldb <= TN_S3_MAX_LD && p.lda2 <= TN_S3_MAX_LD;
  long maxld = p.lda > p.ldb ? p.lda : p.ldb;
  if (PROA == PRO_BNBWD && p.lda2 > maxld) maxld = p.lda2;
  TNPlan pl = tn_plan(c, p.P, p.Mo, p.Ni, PROB != PRO_GATE1 && ld_ok, maxld);
  if (!pl.s3 && ((p.Mo & 3) || (p.Ni & 3) || (p.lda & 3) || (PROB != PRO_GATE1 && (p.ldb & 3))))
    return fail(PRH_ERR_ARG, "gemm_tn: Mo/Ni/lda/ldb must be multiples of 4 (Mo=%d Ni=%d)", p.Mo,
                p.Ni);
  p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.splits = pl.splits;
  p.rows_per_split = pl.rows_per_split;
  p.slab = slab;
  p.colsum = colsum_out != nullptr ? colsum_slab : nullptr;
  const long blocks = (long)pl.tiles_m * pl.tiles_n * pl.splits;
  {
    char nm[64];
    const double by = 4.0 * ((double)p.P * p.Mo * (PROA == PRO_BNBWD ? 2 : 1) +
                             (double)p.P * (PROB == PRO_GATE1 ? 1 : p.Ni) + (double)p.Mo * p.Ni);
    bool done = false;
    if constexpr (PROB != PRO_GATE1) {
      if (pl.s3) {
        static const int attr_rc = allow_big_lds(gemm_tn_s3_kernel<PROA, PROB, 3>, gemm_tn_s3_kernel<PROA, PROB, 1>,
                                                 gemm_tn_s3_kernel<PROA, PROB, 2>);
        if (attr_rc != PRH_OK) return attr_rc;
        if (c.core == 3) {
          float* hdr = slab + (size_t)pl.splits * p.Mo * p.Ni;
          if (p.amaxA == nullptr) {
            TRY_RC((measure_absmax<PROA>(p.A, p.lda, p.A2, p.lda2, p.pa, p.pb, p.pc, p.P, p.Mo, hdr, hdr + 64, st)));
            p.amaxA = hdr;
          }
          if (p.amaxB == nullptr) {
            TRY_RC((measure_absmax<PROB>(p.B, p.ldb, nullptr, 0, p.qa, p.qb, nullptr, p.P, p.Ni, hdr + 1, hdr + 64, st)));
            p.amaxB = hdr + 1;
          }
        }
        bool tr = false;
        if constexpr (PROA == PRO_NONE && (PROB == PRO_NONE || PROB == PRO_BNRELU))
          tr = c.core == 3 && ((p.Mo | p.Ni | (int)p.lda | (int)p.ldb) & 3) == 0;
        p.pace = nullptr;
        // (only where many tiles share long splits: with 6 tiles per split the waits cost the
        // attention K/V wgrad 7 % and there is little to share)
        if (tr && pl.tiles_m * pl.tiles_n >= 8 && pl.splits <= ABSMAX_MAX_BLOCKS &&
            pl.rows_per_split >= 16384) {
          // progress counters live where the (already consumed) per-block maxima were
          p.pace = reinterpret_cast<int*>(slab + (size_t)pl.splits * p.Mo * p.Ni + 64);
          if (hipMemsetAsync(p.pace, 0, sizeof(int) * pl.splits, st) != hipSuccess)
            return fail(PRH_ERR_HIP, "gemm_tn: memset of the pacing counters failed");
        }
        snprintf(nm, sizeof(nm), "gemm_tn_%s<%d,%d>%s Mo=%d Ni=%d", tr ? "h2tr" : c.tag(), PROA, PROB,
                 side ? "+apply" : "", p.Mo, p.Ni);
        ProfScope ps(nm, 2.0 * p.P * (double)p.Mo * p.Ni, by, st);
        if constexpr (PROA == PRO_NONE && (PROB == PRO_NONE || PROB == PRO_BNRELU)) {
          if (tr && side) {
            if (p.side.period == 0) p.side.period = tn_side_period(pl, p.side);
            switch (p.side.period) {
              case 4: TRY_RC((launch_tn_tr_side<PROB, 4>(p, blocks, st))); break;
              case 2: TRY_RC((launch_tn_tr_side<PROB, 2>(p, blocks, st))); break;
              case 1: TRY_RC((launch_tn_tr_side<PROB, 1>(p, blocks, st))); break;
              default: return fail(PRH_ERR_ARG, "gemm_tn: side period %d (1, 2 or 4)", p.side.period);
            }
            hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)p.side.part, (int)blocks,
                               p.side.amax);
          } else if (tr) {
            static const int attr_tr = allow_big_lds(gemm_tn_tr_kernel<PROB>);
            if (attr_tr != PRH_OK) return attr_tr;
            hipLaunchKernelGGL((gemm_tn_tr_kernel<PROB>), dim3((unsigned)blocks), dim3(512), TR_LDS, st, p);
          }
        }
        if (side && !tr) return fail(PRH_ERR_ARG, "gemm_tn: side job without the transposed-read core");
        if (!tr) switch (c.core) {
          case 2: launch_tn_s3<PROA, PROB, 1>(p, blocks, st); break;
          case 3: launch_tn_s3<PROA, PROB, 2>(p, blocks, st); break;
          default: launch_tn_s3<PROA, PROB, 3>(p, blocks, st);
        }
        done = true;
      }
    }
    if constexpr (PROA == PRO_NONE && PROB == PRO_NONE) {
      // short row ranges: one launch, no slab (prh_small.hpp, gemm_tn_direct_kernel)
      if (!done && C != nullptr && p.P >= 64 && p.P <= 4096 && (p.P & 63) == 0 && (p.Mo & 31) == 0 &&
          (p.Ni & 31) == 0 && (p.lda & 3) == 0 && (p.ldb & 3) == 0 && al16(p.A) && al16(p.B)) {
        p.tiles_m = p.Mo / 32; p.tiles_n = p.Ni / 32; p.splits = 1; p.rows_per_split = p.P;
        snprintf(nm, sizeof(nm), "gemm_tn_direct Mo=%d Ni=%d", p.Mo, p.Ni);
        ProfScope ps(nm, 2.0 * p.P * (double)p.Mo * p.Ni, by, st);
        hipLaunchKernelGGL(gemm_tn_direct_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(256), 0, st, p, C, ldc,
                           colsum_out);
        LAUNCH_CHECK();
        return PRH_OK;
      }
      if (!done && small_tn_dims_ok(p.P, p.Mo, p.Ni) && (p.lda & 3) == 0 && (p.ldb & 3) == 0 && al16(p.A) && al16(p.B)) {
        static const int attr_sm = allow_big_lds(gemm_tn_small_kernel);
        if (attr_sm != PRH_OK) return attr_sm;
        small_tn_plan(p.P, p.Mo, p.Ni, pl.splits, pl.rows_per_split);
        pl.tiles_m = p.Mo / 64; pl.tiles_n = p.Ni / 64;
        p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.splits = pl.splits; p.rows_per_split = pl.rows_per_split;
        snprintf(nm, sizeof(nm), "gemm_tn_small Mo=%d Ni=%d", p.Mo, p.Ni);
        ProfScope ps(nm, 2.0 * p.P * (double)p.Mo * p.Ni, by, st);
        hipLaunchKernelGGL(gemm_tn_small_kernel, dim3((unsigned)(pl.tiles_m * pl.tiles_n * pl.splits)), dim3(256), 65536, st, p);
        done = true;
      }
    }
    if (!done) {
      snprintf(nm, sizeof(nm), "gemm_tn<%d,%d> Mo=%d Ni=%d", PROA, PROB, p.Mo, p.Ni);
      ProfScope ps(nm, 2.0 * p.P * (double)p.Mo * p.Ni, by, st);
      if (p.Ni <= 64)
        hipLaunchKernelGGL((gemm_tn_kernel<PROA, PROB, true>), dim3((unsigned)blocks), dim3(256), 0, st, p);
      else
        hipLaunchKernelGGL((gemm_tn_kernel<PROA, PROB>), dim3((unsigned)blocks), dim3(256), 0, st, p);
    }
  }
  LAUNCH_CHECK();
  // (weights and column sums of a Linear's wgrad go in one launch)
  return reduce_wgrad_slabs(slab, colsum_slab, pl.splits, p.Mo, p.Ni, C, ldc, colsum_out, st);
}

int transpose(const float* in, int R, int C, float* out, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), 0, st, in, R, C,
                     (long)C, out, (long)R);
  LAUNCH_CHECK();
  return PRH_OK;
}

int copy_cols(const float* src, long lds_, int cs, float* dst, long ldd, int cd, size_t rows,
              hipStream_t st) {
  const size_t n = rows * (size_t)cd;
  if (n == 0) return PRH_OK;
  hipLaunchKernelGGL(copy_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src,
                     lds_, cs, dst, ldd, cd, rows);
  LAUNCH_CHECK();
  return PRH_OK;
}

#define TRY(x)                \
  do {                        \
    int rc_ = (x);            \
    if (rc_ != PRH_OK) return rc_; \
  } while (0)

// ------------------------------------------------------------------ shared-MLP stack
// Layers l = 0..L-1:  z_l = h_{l-1} W_l^T + b_l ;  h_l = relu(BN_l(z_l)), h_{-1} = x.
// z_l live side by side in z_cat [P, sum cout] (column offset off_l); BN coefficient vectors
// are concatenated the same way.  h_l is never stored: consumers re-apply BN+ReLU on load.
struct StackDims {
  int L; int off[PRH_MAX_LAYERS + 1]; int cin0, cin0p;
};
StackDims stack_dims(const prh_bn_layer* ly, int L) {
  StackDims d;
  d.L = L;
  d.off[0] = 0;
  for (int l = 0; l < L; ++l) d.off[l + 1] = d.off[l] + ly[l].cout;
  d.cin0 = ly[0].cin;
  d.cin0p = (int)align_up((size_t)d.cin0, 4);
  return d;
}

int check_stack(const prh_bn_layer* ly, int L) {
  if (L < 1 || L > PRH_MAX_LAYERS) return fail(PRH_ERR_ARG, "n_layers %d out of range", L);
  for (int l = 0; l < L; ++l) {
    if (ly[l].cout % 4) return fail(PRH_ERR_ARG, "layer %d: cout=%d must be a multiple of 4", l, ly[l].cout);
    if (l > 0 && ly[l].cin != ly[l - 1].cout)
      return fail(PRH_ERR_ARG, "layer %d: cin=%d != previous cout=%d", l, ly[l].cin, ly[l - 1].cout);
    if (!ly[l].w || !ly[l].b || !ly[l].gamma || !ly[l].beta || !ly[l].running_mean || !ly[l].running_var)
      return fail(PRH_ERR_ARG, "layer %d: null parameter pointer", l);
  }
  return PRH_OK;
}

// workspace carve shared by forward/backward of a stack
struct StackWS {
  float* xpad = nullptr;    // [P, cin0p] when cin0 % 4 != 0
  float* w0pad = nullptr;   // [cout0, cin0p]
  float* ws_a = nullptr;    // stats partials [stat_tiles_max][maxc]
  float* ws_b = nullptr;
  float* ws_c = nullptr;    // forward: per-column max / min of z per row block [stat_tiles_max][max cout]
  float* ws_d = nullptr;
  float* apart = nullptr;   // per-block maxima of act_amax_kernel [ABSMAX_MAX_BLOCKS]
  double* stat2 = nullptr;  // stage-1 slice records [BN_SLICES][3][maxc]
  char* wprep = nullptr;    // split-bf16 weight image of the layer being run
};
inline size_t wprep_floats(const prh_bn_layer* ly, int L, int extra_n, int extra_k) {
  size_t m = s3_weight_bytes(extra_n, extra_k), t = s3_weight_bytes(extra_k, extra_n);
  m = t > m ? t : m;
  for (int l = 0; l < L; ++l) {
    const int ci = (int)align_up((size_t)ly[l].cin, 4);
    size_t a = s3_weight_bytes(ly[l].cout, ci), b = s3_weight_bytes(ci, ly[l].cout);
    m = a > m ? a : m; m = b > m ? b : m;
  }
  return m / sizeof(float) + 64;
}
bool stack_ws_carve(Arena& a, StackWS& w, int P, const prh_bn_layer* ly, int L, int maxc,
                    int extra_n = 0, int extra_k = 0) {
  StackDims d = stack_dims(ly, L);
  if (d.cin0p != d.cin0) { w.xpad = a.f((size_t)P * d.cin0p); w.w0pad = a.f((size_t)ly[0].cout * d.cin0p); }
  w.ws_a = a.f((size_t)stat_tiles_max(P) * maxc);
  w.ws_b = a.f((size_t)stat_tiles_max(P) * maxc);
  {
    int mco = extra_n;
    for (int l = 0; l < L; ++l) mco = ly[l].cout > mco ? ly[l].cout : mco;
    w.ws_c = a.f((size_t)stat_tiles_max(P) * mco);
    w.ws_d = a.f((size_t)stat_tiles_max(P) * mco);
    w.apart = a.f(ABSMAX_MAX_BLOCKS);
  }
  w.stat2 = (double*)a.f((size_t)BN_SLICES * 3 * maxc * 2);
  w.wprep = (char*)a.f(wprep_floats(ly, L, extra_n, extra_k));
  return a.ok;
}

// amax_slot (training, optional): receives the largest value of relu(BN(z)) from the column
// maxima / minima in ws_c / ws_d - the operand maximum of the GEMMs that consume this layer
int bn_coeffs(const prh_bn_layer& ly, int P, int training, float momentum, float eps,
              const float* ws_a, const float* ws_b, double* stat2, StatInfo si, float* mean,
              float* rstd, float* scale, float* shift, hipStream_t st, const float* ws_c = nullptr,
              const float* ws_d = nullptr, float* apart = nullptr, float* amax_slot = nullptr) {
  if (training) {
    TRY_RC(reduce_bn_stage1(ws_a, ws_b, si.count, (long)ly.cout, ly.cout, si.rows, P, 1, stat2, st));
    hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3(cdiv(ly.cout, 128)), dim3(128), 0, st, stat2, P,
                       ly.cout, ly.gamma, ly.beta, ly.running_mean, ly.running_var,
                       ly.num_batches_tracked, momentum, eps, mean, rstd, scale, shift);
    if (amax_slot != nullptr && ws_c != nullptr) {
      // every requested slot is written: its consumers do not measure
      LAUNCH_CHECK();
      TRY_RC(reduce_act_amax(ws_c, ws_d, si.count, (long)ly.cout, ly.cout, scale, shift, apart, amax_slot, st));
    }
  } else {
    hipLaunchKernelGGL(bn_eval_coeffs_kernel, dim3(cdiv(ly.cout, 256)), dim3(256), 0, st, ly.gamma,
                       ly.beta, ly.running_mean, ly.running_var, eps, ly.cout, mean, rstd, scale,
                       shift);
  }
  LAUNCH_CHECK();
  return PRH_OK;
}

// forward of the stack into z_cat (ld = ldz); coefficient vectors indexed by off_l
int stack_forward(Cores c, const prh_bn_layer* ly, int L, const float* x, int P, int training,
                  float momentum, float eps, float* z_cat, long ldz, float* scale, float* shift,
                  float* mean, float* rstd, StackWS& w, hipStream_t st, float* op_amax = nullptr) {
  // op_amax (training): slot l receives the maximum of layer l's activation relu(BN_l(z_l)),
  // taken from the statistics epilogue - the operand scale of layer l+1's split-fp16 GEMM and,
  // kept by the caller, of the wgrads in backward: no pass over the activations
  if (!training || c.mode != 3) op_amax = nullptr;
  StackDims d = stack_dims(ly, L);
  const float* x0 = x; long ldx = d.cin0; const float* w0 = ly[0].w; int k0 = d.cin0;
  if (d.cin0p != d.cin0) {
    TRY(copy_cols(x, d.cin0, d.cin0, w.xpad, d.cin0p, d.cin0p, (size_t)P, st));
    TRY(copy_cols(ly[0].w, d.cin0, d.cin0, w.w0pad, d.cin0p, d.cin0p, (size_t)ly[0].cout, st));
    x0 = w.xpad; ldx = d.cin0p; w0 = w.w0pad; k0 = d.cin0p;
  }
  for (int l = 0; l < L; ++l) {
    NTParams p; memset(&p, 0, sizeof(p));
    p.M = P; p.N = ly[l].cout; p.bias = ly[l].b;
    p.C = z_cat + d.off[l]; p.ldc = ldz;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
    if (op_amax != nullptr) { p.ws_c = w.ws_c; p.ws_d = w.ws_d; if (l > 0) p.amaxA = op_amax + (l - 1); }
    StatInfo si;
    if (l == 0) {
      p.A = x0; p.lda = ldx; p.W = w0; p.ldw = k0; p.K = k0;
      if (training) TRY((launch_nt<PRO_NONE, EPI_BIAS_STATS>(c, p, st, &si)));
      else TRY((launch_nt<PRO_NONE, EPI_BIAS>(c, p, st)));
    } else {
      p.A = z_cat + d.off[l - 1]; p.lda = ldz; p.W = ly[l].w; p.ldw = ly[l].cin; p.K = ly[l].cin;
      p.pa = scale + d.off[l - 1]; p.pb = shift + d.off[l - 1];
      if (training) TRY((launch_nt<PRO_BNRELU, EPI_BIAS_STATS>(c, p, st, &si)));
      else TRY((launch_nt<PRO_BNRELU, EPI_BIAS>(c, p, st)));
    }
    TRY(bn_coeffs(ly[l], P, training, momentum, eps, w.ws_a, w.ws_b, w.stat2, si, mean + d.off[l],
                  rstd + d.off[l], scale + d.off[l], shift + d.off[l], st, w.ws_c, w.ws_d, w.apart,
                  op_amax ? op_amax + l : nullptr));
  }
  return PRH_OK;
}

// Backward through layers L-1..0 of a stack.
//   dy_cat [P, sum cout] (ld lddy): on entry column block l holds the ReLU-masked gradient
//   w.r.t. BN_l output coming from OUTSIDE the stack (zero if none) for l < L-1, and the
//   complete masked gradient for l = L-1.  stats_ready: BN-backward partials of layer L-1
//   are already in w.ws_a/ws_b.
// Scratch: coef [3*maxc], wT [max cin*cout], slab, colslab.
// hdr[2]: two headers (largest |dz| in [0], per-block maxima from [64]) - while a held wgrad still
// reads its own layer's maximum from one, the apply pass it carries fills the other
struct StackBwdScratch { float* ca; float* cb; float* cc; float* wT; float* slab; float* colslab; float* dxpad; float* hdr[2]; };

// A wgrad <PRO_NONE, PRO_BNRELU> of materialised dz whose launch is held back until the layer below
// has its BN-backward coefficients, so that this layer's apply pass can ride in it (TNSide)
struct HeldWgrad { bool on = false; TNParams t; float* slab; float* colslab; float* out; long ldc; };
int launch_held(Cores c, HeldWgrad& h, hipStream_t st) {
  h.on = false;
  return launch_tn<PRO_NONE, PRO_BNRELU>(c, h.t, h.slab, h.colslab, h.out, h.ldc, nullptr, st);
}
inline TNSide side_job(float* dy, long lddy, const float* z, long ldz, const StackBwdScratch& sc, long rows, int cols,
                       float* hdr) {
  TNSide s;
  s.dy = dy; s.lddy = lddy; s.z = z; s.ldz = ldz; s.ka = sc.ca; s.kb = sc.cb; s.kc = sc.cc;
  s.rows = rows; s.cols = cols; s.part = hdr + 64; s.amax = hdr; s.period = 0;
  return s;
}

int stack_backward(Cores c, const prh_bn_layer* ly, int L, const float* x, int P, int training,
                   float* dy_cat, long lddy, const float* z_cat, long ldz, const float* scale,
                   const float* shift, const float* mean, const float* rstd,
                   const prh_bn_layer_grad* gr, float* dx, StackWS& w, StackBwdScratch& sc,
                   StatInfo si, hipStream_t st, const float* op_amax = nullptr, const HeldWgrad* held = nullptr) {
  if (!training || c.mode != 3) op_amax = nullptr;   // slots as filled by stack_forward
  StackDims d = stack_dims(ly, L);
  // Split-fp16 mode: the apply pass of layer l rides in the wgrad of layer l+1 (the caller's held
  // wgrad for l = L-1), so each layer runs  finalize(l); wgrad(l+1) + apply(l); dgrad(l)  and its own
  // wgrad waits for layer l-1.  What that moves across the other launches:
  //  * the held wgrad reads dz_{l+1} (materialised, untouched by dgrad(l+1), which only reads it and
  //    writes block l), its layer's maximum in sc.hdr[cur] - the apply it carries writes
  //    sc.hdr[cur ^ 1] - and the saved activations; it reads none of ca/cb/cc, which finalize(l) has
  //    by then overwritten with layer l's, exactly what the carried apply needs;
  //  * its slab (sc.slab, the caller's for the held fusion wgrad) is written and reduced inside
  //    launch_tn, back to back, so no slab is live across another wgrad; its pacing counters and, when
  //    op_amax is absent, its measured B maximum sit behind that same slab;
  //  * ws_a / ws_b / stat2 are produced by dgrad(l+1) and consumed by finalize(l) before the held
  //    wgrad starts, and no wgrad touches them, wprep or wT (layer 0, whose padded wgrad borrows wT,
  //    is never held).
  HeldWgrad hw;
  if (held != nullptr) hw = *held;
  int cur = 0;                        // sc.hdr[cur]: where the newest dz maximum is (the caller's: 0)
  const float* x0 = x; long ldx = d.cin0; int k0 = d.cin0;
  if (d.cin0p != d.cin0) { x0 = w.xpad; ldx = d.cin0p; k0 = d.cin0p; }   // xpad filled by caller
  for (int l = L - 1; l >= 0; --l) {
    const int co = ly[l].cout, o = d.off[l];
    // 1. statistics -> BN-backward coefficients, dgamma, dbeta, dbias
    TRY(reduce_bn_stage1(w.ws_a + si.off, w.ws_b + si.off, si.count, si.ld ? si.ld : (long)co, co, 64, P, 0, w.stat2, st));
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(co, 128)), dim3(128), 0, st, w.stat2, P, co,
                       ly[l].gamma, mean + o, rstd + o, training,
                       sc.ca, sc.cb, sc.cc, gr ? gr[l].dgamma : nullptr, gr ? gr[l].dbeta : nullptr,
                       gr ? gr[l].db : nullptr);
    LAUNCH_CHECK();
    // 1b. split-fp16 mode: dy_l <- dz_l in place, so wgrad and dgrad read one plain operand
    const bool mat = dz_in_place(c, co, lddy, ldz);
    const float* dz_amax = nullptr;     // largest |dz_l| once known
    if (hw.on) {
      const TNSide s = side_job(dy_cat + o, lddy, z_cat + o, ldz, sc, P, co, sc.hdr[cur ^ 1]);
      if (mat && tn_side_ok(c, hw.t, s)) {
        hw.t.side = s;
        cur ^= 1;
        dz_amax = sc.hdr[cur];
      }
      TRY(launch_held(c, hw, st));
    }
    if (mat && dz_amax == nullptr) {
      TRY(materialize_dz(dy_cat + o, lddy, z_cat + o, ldz, sc.ca, sc.cb, sc.cc, P, co, sc.hdr[cur], st));
      dz_amax = sc.hdr[cur];
    }
    // 2. wgrad: dW_l = dz_l^T h_{l-1}
    if (gr && gr[l].dw) {
      TNParams t; memset(&t, 0, sizeof(t));
      t.A = dy_cat + o; t.lda = lddy; t.A2 = z_cat + o; t.lda2 = ldz;
      t.P = P; t.Mo = co; t.pa = sc.ca; t.pb = sc.cb; t.pc = sc.cc;
      t.amaxA = dz_amax;
      if (l == 0) {
        t.B = x0; t.ldb = ldx; t.Ni = k0;
        float* out = k0 == d.cin0 ? gr[l].dw : sc.wT;   // padded input: reduce into scratch ...
        if (mat) TRY((launch_tn<PRO_NONE, PRO_NONE>(c, t, sc.slab, sc.colslab, out, (long)k0, nullptr, st)));
        else TRY((launch_tn<PRO_BNBWD, PRO_NONE>(c, t, sc.slab, sc.colslab, out, (long)k0, nullptr, st)));
        if (k0 != d.cin0)                                // ... then drop the pad columns
          TRY(copy_cols(sc.wT, k0, d.cin0, gr[l].dw, d.cin0, d.cin0, (size_t)co, st));
      } else {
        t.B = z_cat + d.off[l - 1]; t.ldb = ldz; t.Ni = ly[l].cin;
        t.qa = scale + d.off[l - 1]; t.qb = shift + d.off[l - 1];
        if (op_amax != nullptr) t.amaxB = op_amax + (l - 1);
        // hold it for apply(l-1) if that pass can ride (decided again, with the real job, at launch)
        if (mat && dz_in_place(c, ly[l - 1].cout, lddy, ldz) &&
            tn_side_ok(c, t, side_job(dy_cat + d.off[l - 1], lddy, z_cat + d.off[l - 1], ldz, sc, P, ly[l - 1].cout, sc.hdr[cur ^ 1]))) {
          hw.on = true; hw.t = t; hw.slab = sc.slab; hw.colslab = sc.colslab; hw.out = gr[l].dw; hw.ldc = (long)ly[l].cin;
        } else if (mat) TRY((launch_tn<PRO_NONE, PRO_BNRELU>(c, t, sc.slab, sc.colslab, gr[l].dw, (long)ly[l].cin, nullptr, st)));
        else TRY((launch_tn<PRO_BNBWD, PRO_BNRELU>(c, t, sc.slab, sc.colslab, gr[l].dw, (long)ly[l].cin, nullptr, st)));
      }
      dz_amax = t.amaxA;
    }
    // 3. dgrad into the previous layer's block (accumulate + mask + its statistics)
    if (l > 0) {
      TRY(transpose(ly[l].w, co, ly[l].cin, sc.wT, st));     // wT [cin, cout]
      NTParams p; memset(&p, 0, sizeof(p));
      p.amaxA = dz_amax;
      p.A = dy_cat + o; p.lda = lddy; p.A2 = z_cat + o; p.lda2 = ldz;
      p.pa = sc.ca; p.pb = sc.cb; p.pc = sc.cc;
      p.W = sc.wT; p.ldw = co; p.M = P; p.N = ly[l].cin; p.K = co;
      p.C = dy_cat + d.off[l - 1]; p.ldc = lddy;
      p.E1 = z_cat + d.off[l - 1]; p.lde1 = ldz;
      p.es = scale + d.off[l - 1]; p.et = shift + d.off[l - 1];
      p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
      p.flags = F_ACCUM | F_MASK | F_STATS;
      if (mat) TRY((launch_nt<PRO_NONE, EPI_DGRAD>(c, p, st, &si)));
      else TRY((launch_nt<PRO_BNBWD, EPI_DGRAD>(c, p, st, &si)));
      si.ld = 0; si.off = 0;
    } else if (dx != nullptr) {
      // dx = dz_0 W_0  (W_0^T is [cin0p, cout] with zero pad rows)
      const float* w0 = ly[0].w; int kk = d.cin0;
      if (d.cin0p != d.cin0) { w0 = w.w0pad; kk = d.cin0p; }
      TRY(transpose(w0, co, kk, sc.wT, st));
      NTParams p; memset(&p, 0, sizeof(p));
      p.A = dy_cat + o; p.lda = lddy; p.A2 = z_cat + o; p.lda2 = ldz;
      p.pa = sc.ca; p.pb = sc.cb; p.pc = sc.cc;
      p.W = sc.wT; p.ldw = co; p.M = P; p.N = d.cin0; p.K = co;
      p.C = dx; p.ldc = d.cin0;
      p.flags = 0;
      p.amaxA = dz_amax;
      if (mat) TRY((launch_nt<PRO_NONE, EPI_DGRAD>(c, p, st)));
      else TRY((launch_nt<PRO_BNBWD, EPI_DGRAD>(c, p, st)));
    }
  }
  if (hw.on) TRY(launch_held(c, hw, st));     // (layer 0 is never held: nothing below it to carry)
  return PRH_OK;
}

int max_cout(const prh_bn_layer* ly, int L) {
  int m = 0;
  for (int l = 0; l < L; ++l) m = ly[l].cout > m ? ly[l].cout : m;
  return m;
}
size_t max_w(const prh_bn_layer* ly, int L) {
  size_t m = 0;
  for (int l = 0; l < L; ++l) {
    size_t s = (size_t)ly[l].cout * align_up((size_t)ly[l].cin, 4);
    m = s > m ? s : m;
  }
  return m;
}
void stack_bwd_scratch_carve(Cores c, Arena& a, StackBwdScratch& sc, int P, const prh_bn_layer* ly, int L,
                             size_t extra_w, int extra_c) {
  int mc = max_cout(ly, L); if (extra_c > mc) mc = extra_c;
  size_t mw = max_w(ly, L); if (extra_w > mw) mw = extra_w;
  sc.ca = a.f(mc); sc.cb = a.f(mc); sc.cc = a.f(mc);
  sc.hdr[0] = a.f(S3_HDR_FLOATS); sc.hdr[1] = a.f(S3_HDR_FLOATS);
  sc.wT = a.f(mw);
  size_t slab = 0, cs = 0;
  for (int l = 0; l < L; ++l) {
    const int ci = (int)align_up((size_t)ly[l].cin, 4);
    size_t s1 = tn_slab_floats(c, P, ly[l].cout, ci), s2 = tn_colsum_floats(c, P, ly[l].cout, ci);
    slab = s1 > slab ? s1 : slab; cs = s2 > cs ? s2 : cs;
  }
  sc.slab = a.f(slab); sc.colslab = a.f(cs);
}

// ---- workspace layouts of the entry points (measure with Arena(), carve with Arena(ptr,n))
struct LinearBwdWS { float* wT; float* slab; float* cslab; char* wprep; float* dxpart; };
void linear_bwd_carve(Cores c, Arena& a, LinearBwdWS& w, int rows, int k, int n) {
  w.wprep = (char*)a.f(s3_weight_bytes(k, n) / sizeof(float) + 64);
  w.dxpart = a.f(nt_amax_part_floats(rows, k));      // partial maxima of dx (prh_linear_backward_amax)
  w.wT = a.f((size_t)k * n);
  w.slab = a.f(tn_slab_floats(c, rows, n, k));
  w.cslab = a.f(tn_colsum_floats(c, rows, n, k));
}
struct MlpWS { StackWS w; StackBwdScratch sc; float* dy_cat; };
void mlp_carve(Cores c, Arena& a, MlpWS& m, int P, const prh_bn_layer* ly, int L) {
  StackDims d = stack_dims(ly, L);
  stack_ws_carve(a, m.w, P, ly, L, max_cout(ly, L));
  stack_bwd_scratch_carve(c, a, m.sc, P, ly, L, 0, 0);
  m.dy_cat = a.f((size_t)P * d.off[L]);
}
struct EncWS { StackWS w; StackBwdScratch sc; float* fslab; float* fcslab; float* dy_cat; float* dyf; float* dU; float* gsum_a; float* gsum_b; };
void enc_carve(Cores c, Arena& a, EncWS& e, int P, const prh_bn_layer* conv, int cat, int od, int backward) {   // 2: no dyf carve
  stack_ws_carve(a, e.w, P, conv, 5, cat > od ? cat : od, od, cat);
  if (!backward) return;
  stack_bwd_scratch_carve(c, a, e.sc, P, conv, 5, (size_t)od * cat, cat > od ? cat : od);
  const size_t fs = tn_slab_floats(c, P, od, cat), gs = tn_slab_floats(c, P, od, 64);
  const size_t fc = tn_colsum_floats(c, P, od, cat), gc = tn_colsum_floats(c, P, od, 64);
  e.fslab = a.f(fs > gs ? fs : gs);
  e.fcslab = a.f(fc > gc ? fc : gc);
  e.dy_cat = a.f((size_t)P * cat);
  e.dyf = backward == 2 ? nullptr : a.f((size_t)P * od);      // 2: the caller's d_fused buffer serves (d_fused_scratch)
  e.dU = a.f((size_t)P * 64);
  e.gsum_a = a.f(64);
  e.gsum_b = a.f(64);
}

// ---- bf16 mode: workspace layouts and small launch helpers
typedef unsigned short u16;
struct Enc16WS {
  u16* xpad; float* w0pad; float* ws_a; float* ws_b; float* ws_c; double* stat2; char* wprep;
  float *ca, *cb, *cc, *wT, *slab, *cslab, *dU, *gsum_a, *gsum_b; u16 *dy_cat, *dyf;
  float* c1part;      // conv1 weight-gradient partials [C1_WGRAD_BLOCKS][cout][cin]
};
constexpr int C1_WGRAD_BLOCKS = 1024;
inline bool conv_in_fp32_ok(int cin, int cout) { return cin <= 8 && cout == 64; }
inline int cin_pad8(int c) { return (c + 7) / 8 * 8; }
void enc16_carve(Arena& a, Enc16WS& e, int P, const int* ch /*[6]: cin, 64..od*/, int cat, int od, bool backward) {
  const int c0p = cin_pad8(ch[0]);
  const int maxc = cat > od ? cat : od;
  e.xpad = (u16*)a.f(((size_t)P * c0p + 1) / 2);
  e.w0pad = a.f((size_t)ch[1] * c0p);
  e.ws_a = a.f((size_t)stat_tiles_max(P) * maxc);
  e.ws_b = a.f((size_t)stat_tiles_max(P) * maxc);
  e.ws_c = a.f((size_t)stat_tiles_max(P) * od);          // pooling partials (arg-max rows)
  e.stat2 = (double*)a.f((size_t)BN_SLICES * 3 * maxc * 2);
  size_t wb = b16_weight_bytes(od, cat), t = b16_weight_bytes(cat, od);
  wb = t > wb ? t : wb;
  t = b16_weight_bytes(od, 64); wb = t > wb ? t : wb;
  t = b16_weight_bytes(64, od); wb = t > wb ? t : wb;
  for (int l = 0; l < 5; ++l) {
    const int ci = l == 0 ? c0p : ch[l];
    t = b16_weight_bytes(ch[l + 1], ci); wb = t > wb ? t : wb;
    t = b16_weight_bytes(ci, ch[l + 1]); wb = t > wb ? t : wb;
  }
  e.wprep = (char*)a.f(wb / sizeof(float) + 64);
  if (!backward) return;
  e.ca = a.f(maxc); e.cb = a.f(maxc); e.cc = a.f(maxc);
  e.wT = a.f((size_t)od * cat);
  size_t sl = tn16_slab_floats(P, od, cat), cs = tn16_colsum_floats(P, od, cat);
  t = tn16_slab_floats(P, od, 64); sl = t > sl ? t : sl;
  t = tn16_colsum_floats(P, od, 64); cs = t > cs ? t : cs;
  for (int l = 0; l < 5; ++l) {
    const int ci = l == 0 ? c0p : ch[l];
    t = tn16_slab_floats(P, ch[l + 1], ci); sl = t > sl ? t : sl;
    t = tn16_colsum_floats(P, ch[l + 1], ci); cs = t > cs ? t : cs;
  }
  e.slab = a.f(sl); e.cslab = a.f(cs);
  e.dy_cat = (u16*)a.f(((size_t)P * cat + 1) / 2);
  e.dyf = (u16*)a.f(((size_t)P * od + 1) / 2);
  e.dU = a.f((size_t)P * 64);
  e.gsum_a = a.f(64); e.gsum_b = a.f(64);
  e.c1part = a.f((size_t)C1_WGRAD_BLOCKS * ch[1] * 8);
}
int cast_b16(const float* src, long lds_, int cs, u16* dst, long ldd, int cd, size_t rows, hipStream_t st) {
  const size_t n = rows * (size_t)(cd / 2);
  if (n == 0) return PRH_OK;
  hipLaunchKernelGGL(cast_b16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, lds_, cs, dst, ldd, cd, rows);
  LAUNCH_CHECK();
  return PRH_OK;
}
int bn_bwd_apply16(u16* dy, long lddy, const u16* z, long ldz, const float* ka, const float* kb, const float* kc,
                   long rows, int cols, hipStream_t st) {
  long blocks = cdiv(rows, 4L * 8);
  blocks = blocks < 1 ? 1 : (blocks > ABSMAX_MAX_BLOCKS ? ABSMAX_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(bn_bwd_apply_b16_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dy, lddy, z, ldz, ka, kb, kc, rows, cols);
  LAUNCH_CHECK();
  return PRH_OK;
}
inline const float* f16p(const u16* p) { return reinterpret_cast<const float*>(p); }   // NTParams/TNParams carry typed-less pointers
inline float* f16p(u16* p) { return reinterpret_cast<float*>(p); }
struct Lin16WS { char* wprep; float* wT; float* slab; float* cslab; u16* dy16; };
void lin16_carve(Arena& a, Lin16WS& w, int rows, int k, int n, bool backward) {
  size_t wb = b16_weight_bytes(n, k), t = b16_weight_bytes(k, n);
  w.wprep = (char*)a.f((t > wb ? t : wb) / sizeof(float) + 64);
  if (!backward) return;
  w.wT = a.f((size_t)k * n);
  w.slab = a.f(tn16_slab_floats(rows, n, k));
  w.cslab = a.f(tn16_colsum_floats(rows, n, k));
  w.dy16 = (u16*)a.f(((size_t)rows * (n > k ? n : k) + 1) / 2);      // dy cast, or (dy16 entry) the x cast
}
// what an entry point demands of the caller's workspace: present, and no smaller than what
// prh_linear_bf16_workspace_bytes reports (the carve plus 256 bytes) - one rule for the size and the check
inline bool lin16_ws_ok(const Arena& a, const void* workspace, size_t workspace_bytes) {
  return workspace != nullptr && a.ok && workspace_bytes >= a.off + 256;
}
// f(T{}) with T = double or float: the kernel instantiation a points buffer of that type takes (ground lift, paint alignment)
template <typename F> void for_points(int is_double, F f) {
  if (is_double) f(double{}); else f(float{});
}

}  // namespace

// =======================================================================================
extern "C" {

const char* prh_last_error(void) { return g_err; }
int prh_set_gemm_mode(int mode) {
  if (mode < 0 || mode > 4)
    return fail(PRH_ERR_ARG, "gemm mode must be 0 (fp32), 1 (split-bf16), 2 (bf16 operands), 3 (split-fp16) or 4 (bf16 operands and storage)");
  g_gemm_mode = mode;
  return PRH_OK;
}
int prh_get_gemm_mode(void) { return gemm_mode(); }
int prh_set_dropout_seed_source(const unsigned* device_word) {
  g_seed_src = device_word;
  return PRH_OK;
}
const char* prh_version(void) { return "pointnet_refine_hip 0.3 (gfx950: fp32 MFMA 32x32x2 + split-fp16 / split-bf16 MFMA 32x32x16 cores)"; }

// ------------------------------------------------------------------ Linear
size_t prh_linear_forward_workspace_bytes(int rows, int k, int n) {
  // weight image, then the partial output maxima of prh_linear_forward_amax
  return align_up(s3_weight_bytes(n, k) + 512, 256) + nt_amax_part_floats(rows, n) * sizeof(float) + 256;
}

int prh_linear_forward_ex(const float* x, long ldx, const float* w, const float* b, float* y,
                          int rows, int k, int n, int relu, const float* x_amax, void* workspace,
                          size_t workspace_bytes, int device, void* stream) {
  return prh_linear_forward_full(x, ldx, w, b, nullptr, 0, y, rows, k, n, relu, x_amax, nullptr, 0.f, 0u, workspace,
                                 workspace_bytes, device, stream);
}
int prh_linear_forward_full(const float* x, long ldx, const float* w, const float* b, const float* resid,
                            long ldres, float* y, int rows, int k, int n, int relu, const float* x_amax,
                            const float* w_amax, float dropout_p, unsigned dropout_seed, void* workspace,
                            size_t workspace_bytes, int device, void* stream) {
  return prh_linear_forward_amax(x, ldx, w, b, resid, ldres, y, rows, k, n, relu, x_amax, w_amax, dropout_p,
                                 dropout_seed, nullptr, workspace, workspace_bytes, device, stream);
}
int prh_linear_forward_amax(const float* x, long ldx, const float* w, const float* b, const float* resid,
                            long ldres, float* y, int rows, int k, int n, int relu, const float* x_amax,
                            const float* w_amax, float dropout_p, unsigned dropout_seed, float* y_amax_out,
                            void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!x || !w || !y || rows < 0 || k <= 0 || n <= 0 || (resid != nullptr && ldres < n))
    return fail(PRH_ERR_ARG, "linear_forward_full: bad argument");
  if (y_amax_out != nullptr && (workspace == nullptr || workspace_bytes < prh_linear_forward_workspace_bytes(rows, k, n)))
    return fail(PRH_ERR_WORKSPACE, "linear_forward_amax: workspace too small (%zu bytes)", workspace_bytes);
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(PRH_ERR_ARG, "linear_forward_full: dropout_p must be in [0,1)");
  HIP_TRY(hipSetDevice(device));
  NTParams p; memset(&p, 0, sizeof(p));
  p.A = x; p.lda = ldx; p.W = w; p.ldw = k; p.C = y; p.ldc = n;
  p.M = rows; p.N = n; p.K = k; p.bias = b; p.flags = (relu ? F_RELU_OUT : 0) | (resid ? F_RESID : 0);
  p.E1 = resid; p.lde1 = ldres;
  if (dropout_p > 0.f) {
    p.flags |= F_DROPOUT;
    p.drop_seed = dropout_seed; p.drop_thresh = (unsigned)((double)dropout_p * 4294967296.0);
    p.drop_scale = 1.f / (1.f - dropout_p); p.seed_src = g_seed_src;
  }
  p.amaxW = w_amax;
  if (workspace != nullptr && workspace_bytes >= s3_weight_bytes(n, k) + 256)
    p.wprep = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  p.amaxA = x_amax;
  float* part = nullptr;
  if (y_amax_out != nullptr)
    part = reinterpret_cast<float*>((((uintptr_t)workspace + 255) & ~(uintptr_t)255) + align_up(s3_weight_bytes(n, k) + 512, 256));
  return launch_nt<PRO_NONE, EPI_BIAS>(cores_of(gemm_mode()), p, (hipStream_t)stream, nullptr, y_amax_out, part);
}
int prh_linear_forward(const float* x, long ldx, const float* w, const float* b, float* y,
                       int rows, int k, int n, int relu, void* workspace, size_t workspace_bytes,
                       int device, void* stream) {
  return prh_linear_forward_ex(x, ldx, w, b, y, rows, k, n, relu, nullptr, workspace, workspace_bytes, device,
                               stream);
}

// ---- operand maxima for the split-fp16 cores, measured once by the caller ---------------
size_t prh_operand_absmax_workspace_bytes(void) { return (size_t)ABSMAX_MAX_BLOCKS * sizeof(float) + 256; }
int prh_operand_absmax(const float* x, long ld, long rows, int cols, float* out, void* workspace,
                       size_t workspace_bytes, int device, void* stream) {
  if (!x || !out || rows < 0 || cols <= 0 || ld < cols) return fail(PRH_ERR_ARG, "operand_absmax: bad argument");
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes);
  float* part = a.f(ABSMAX_MAX_BLOCKS);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "operand_absmax: workspace too small (%zu bytes)", workspace_bytes);
  TRY_RC((measure_absmax<PRO_NONE>(x, ld, nullptr, 0, nullptr, nullptr, nullptr, rows, cols, out, part,
                                   (hipStream_t)stream)));
  return PRH_OK;
}
// out = (y > 0 ? dy : 0), amax_out[0] = max|out|: ReLU backward of a Linear with a fused ReLU
// (src/model.py:131,164 - linear1 + activation, reg_branches[i][0:2]); n = element count, % 4 == 0,
// all three buffers contiguous and 16-B aligned.  Workspace: prh_operand_absmax_workspace_bytes().
int prh_relu_mask_absmax(const float* dy, const float* y, float* out, long n, float scale, float* amax_out, void* workspace,
                         size_t workspace_bytes, int device, void* stream) {
  if (!dy || !y || !out || !amax_out || n < 0 || (n & 3)) return fail(PRH_ERR_ARG, "relu_mask_absmax: bad argument");
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes);
  float* part = a.f(ABSMAX_MAX_BLOCKS);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "relu_mask_absmax: workspace too small (%zu bytes)", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  long blocks = cdiv(n / 4, 256L * 4);
  blocks = blocks < 1 ? 1 : (blocks > ABSMAX_MAX_BLOCKS ? ABSMAX_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL(relu_mask_amax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dy, y, out, (size_t)(n / 4), scale, part);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int)blocks, amax_out);
  LAUNCH_CHECK();
  return PRH_OK;
}
// 1 when a [rows,k] x [n,k]^T Linear GEMM (and its backward GEMMs) run on the split-fp16 cores,
// i.e. when operand maxima are consumed at all
int prh_linear_uses_operand_maxima(int rows, int k, int n) {
  const Cores c = cores_of(gemm_mode());
  return (c.mode == 3 && (nt_use_s3(c, rows, n, k) || nt_use_s3(c, rows, k, n) || tn_use_s3(c, rows, n, k))) ? 1 : 0;
}

// ---- positional-encoding MLP, first layer (src/model.py:64-75) -------------------------
static int pos_hidden_blocks(long P, int H) {
  const long rpp = 256 / (H / 4);
  long nb = (P + rpp * 16 - 1) / (rpp * 16);
  return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}
static bool pos_hidden_ok(int H) { return H >= 4 && H <= 1024 && (H & (H - 1)) == 0; }
int prh_pos_hidden_forward(const float* xyz, long ld, const float* w0, const float* b0, float* h,
                           long rows, int hidden, int device, void* stream) {
  if (!xyz || !w0 || !h || rows < 0 || ld < 3) return fail(PRH_ERR_ARG, "pos_hidden_forward: bad argument");
  if (!pos_hidden_ok(hidden))
    return fail(PRH_ERR_ARG, "pos_hidden_forward: hidden=%d must be a power of two in [4, 1024]", hidden);
  HIP_TRY(hipSetDevice(device));
  if (rows == 0) return PRH_OK;
  const long rpp = 256 / (hidden / 4);
  long nb = (rows + rpp * 4 - 1) / (rpp * 4);
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(pos_hidden_fwd_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, xyz, ld,
                     w0, b0, h, rows, hidden);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_pos_hidden_forward_workspace_bytes(void) { return (size_t)8192 * sizeof(float) + 256; }
int prh_pos_hidden_forward_amax(const float* xyz, long ld, const float* w0, const float* b0, float* h,
                                long rows, int hidden, float* h_amax_out, void* workspace, size_t workspace_bytes,
                                int device, void* stream) {
  if (h_amax_out == nullptr) return prh_pos_hidden_forward(xyz, ld, w0, b0, h, rows, hidden, device, stream);
  if (!xyz || !w0 || !h || rows < 0 || ld < 3) return fail(PRH_ERR_ARG, "pos_hidden_forward: bad argument");
  if (!pos_hidden_ok(hidden))
    return fail(PRH_ERR_ARG, "pos_hidden_forward: hidden=%d must be a power of two in [4, 1024]", hidden);
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes);
  float* part = a.f(8192);
  if (!a.ok || workspace == nullptr) return fail(PRH_ERR_WORKSPACE, "pos_hidden_forward_amax: workspace too small (%zu bytes)", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const long rpp = 256 / (hidden / 4);
  long nb = (rows + rpp * 4 - 1) / (rpp * 4);
  if (nb > 8192) nb = 8192;
  if (rows > 0) {
    hipLaunchKernelGGL(pos_hidden_fwd_amax_kernel, dim3((unsigned)nb), dim3(256), 0, st, xyz, ld, w0, b0, h, rows,
                       hidden, part);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(absmax_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int)(rows > 0 ? nb : 0), h_amax_out);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_pos_hidden_backward_workspace_bytes(long rows, int hidden) {
  if (!pos_hidden_ok(hidden)) return 0;
  return (size_t)pos_hidden_blocks(rows, hidden) * 4 * hidden * sizeof(float) + 256;
}
int prh_pos_hidden_backward(const float* xyz, long ld, const float* h, const float* dh, const float* w0,
                            float* dxyz, float* dw0, float* db0, long rows, int hidden, void* workspace,
                            size_t workspace_bytes, int device, void* stream) {
  if (!xyz || !h || !dh || rows < 0 || ld < 3) return fail(PRH_ERR_ARG, "pos_hidden_backward: bad argument");
  if (dxyz != nullptr && (w0 == nullptr || hidden > 256))
    return fail(PRH_ERR_ARG, "pos_hidden_backward: point gradients need w0 and hidden <= 256 (hidden=%d)", hidden);
  if (!pos_hidden_ok(hidden))
    return fail(PRH_ERR_ARG, "pos_hidden_backward: hidden=%d must be a power of two in [4, 1024]", hidden);
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes);
  const int nb = pos_hidden_blocks(rows, hidden);
  float* part = a.f((size_t)nb * 4 * hidden);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "pos_hidden_backward: workspace too small (%zu bytes)", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dxyz != nullptr ? pos_hidden_bwd_kernel<true> : pos_hidden_bwd_kernel<false>, dim3((unsigned)nb),
                     dim3(256), 0, st, xyz, ld, h, dh, part, rows, hidden, w0, dxyz);
  LAUNCH_CHECK();
  return reduce_pos_hidden_final(part, nb, hidden, dw0, db0, st);
}

// ---- nn.Linear with <= 4 outputs (regression heads' last layer, src/model.py:162-166) ----
static bool linear_small_ok(int k, int n) {
  const int lpr = k / 4;
  return n >= 1 && n <= 4 && (k & 3) == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0;
}
static int linear_small_blocks(long rows, int k) {
  const long rpp = 256 / (k / 4);
  long nb = (rows + rpp * 8 - 1) / (rpp * 8);
  return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}
int prh_linear_small_forward(const float* x, const float* w, const float* b, float* y, long rows, int k,
                             int n, int device, void* stream) {
  if (!x || !w || !y || rows < 0) return fail(PRH_ERR_ARG, "linear_small_forward: bad argument");
  if (!linear_small_ok(k, n))
    return fail(PRH_ERR_ARG, "linear_small_forward: needs n <= 4 and k/4 a power of two <= 64 (k=%d n=%d)", k, n);
  HIP_TRY(hipSetDevice(device));
  if (rows == 0) return PRH_OK;
  const long rpp = 256 / (k / 4);
  long nb = (rows + rpp * 4 - 1) / (rpp * 4);
  if (nb > 4096) nb = 4096;
  hipStream_t st = (hipStream_t)stream;
  switch (n) {
    case 1: hipLaunchKernelGGL(linear_small_fwd_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, x, w, b, y, rows, k); break;
    case 2: hipLaunchKernelGGL(linear_small_fwd_kernel<2>, dim3((unsigned)nb), dim3(256), 0, st, x, w, b, y, rows, k); break;
    case 3: hipLaunchKernelGGL(linear_small_fwd_kernel<3>, dim3((unsigned)nb), dim3(256), 0, st, x, w, b, y, rows, k); break;
    default: hipLaunchKernelGGL(linear_small_fwd_kernel<4>, dim3((unsigned)nb), dim3(256), 0, st, x, w, b, y, rows, k); break;
  }
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_linear_small_backward_workspace_bytes(long rows, int k, int n) {
  if (!linear_small_ok(k, n)) return 0;
  return (size_t)linear_small_blocks(rows, k) * ((size_t)n * k + n) * sizeof(float) + 256;
}
int prh_linear_small_backward(const float* x, const float* w, const float* dy, float* dx, float* dw,
                              float* db, long rows, int k, int n, void* workspace, size_t workspace_bytes,
                              int device, void* stream) {
  if (!x || !w || !dy || rows < 0) return fail(PRH_ERR_ARG, "linear_small_backward: bad argument");
  if (!linear_small_ok(k, n))
    return fail(PRH_ERR_ARG, "linear_small_backward: needs n <= 4 and k/4 a power of two <= 64 (k=%d n=%d)", k, n);
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes);
  const int nb = linear_small_blocks(rows, k);
  const int n_el = n * k + n;
  float* part = a.f((size_t)nb * n_el);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "linear_small_backward: workspace too small (%zu bytes)", workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  switch (n) {
    case 1: hipLaunchKernelGGL(linear_small_bwd_kernel<1>, dim3((unsigned)nb), dim3(256), 0, st, x, w, dy, dx, part, rows, k); break;
    case 2: hipLaunchKernelGGL(linear_small_bwd_kernel<2>, dim3((unsigned)nb), dim3(256), 0, st, x, w, dy, dx, part, rows, k); break;
    case 3: hipLaunchKernelGGL(linear_small_bwd_kernel<3>, dim3((unsigned)nb), dim3(256), 0, st, x, w, dy, dx, part, rows, k); break;
    default: hipLaunchKernelGGL(linear_small_bwd_kernel<4>, dim3((unsigned)nb), dim3(256), 0, st, x, w, dy, dx, part, rows, k); break;
  }
  LAUNCH_CHECK();
  return reduce_partial_rows_final(part, nb, n_el, dw, n * k, db, st);
}

size_t prh_linear_backward_workspace_bytes(int rows, int k, int n) {
  Arena a; LinearBwdWS w;
  linear_bwd_carve(cores_of(gemm_mode()), a, w, rows, k, n);
  return a.off + 256;
}

int prh_linear_backward_ex(const float* x, long ldx, const float* w, const float* dy, float* dx,
                           float* dw, float* db, int rows, int k, int n, const float* x_amax,
                           const float* dy_amax_in, void* workspace, size_t workspace_bytes, int device,
                           void* stream) {
  return prh_linear_backward_full(x, ldx, w, dy, dx, dw, db, rows, k, n, x_amax, dy_amax_in, nullptr, workspace,
                                  workspace_bytes, device, stream);
}
int prh_linear_backward_full(const float* x, long ldx, const float* w, const float* dy, float* dx,
                             float* dw, float* db, int rows, int k, int n, const float* x_amax,
                             const float* dy_amax_in, const float* w_amax, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  return prh_linear_backward_amax(x, ldx, w, dy, dx, dw, db, rows, k, n, x_amax, dy_amax_in, w_amax, 0, nullptr,
                                  workspace, workspace_bytes, device, stream);
}
int prh_linear_backward_amax(const float* x, long ldx, const float* w, const float* dy, float* dx,
                             float* dw, float* db, int rows, int k, int n, const float* x_amax,
                             const float* dy_amax_in, const float* w_amax, int dx_accumulate, float* dx_amax_out,
                             void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!x || !w || !dy || rows < 0 || k <= 0 || n <= 0) return fail(PRH_ERR_ARG, "linear_backward: bad argument");
  if ((dx_accumulate || dx_amax_out != nullptr) && dx == nullptr)
    return fail(PRH_ERR_ARG, "linear_backward_amax: dx_accumulate / dx_amax_out need dx");
  if ((k & 3) || (n & 3)) return fail(PRH_ERR_ARG, "linear_backward: k=%d and n=%d must be multiples of 4", k, n);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const Cores c = cores_of(gemm_mode());
  Arena a(workspace, workspace_bytes);
  LinearBwdWS lw;
  linear_bwd_carve(c, a, lw, rows, k, n);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "linear_backward: workspace too small (%zu bytes)", workspace_bytes);
  float *wT = lw.wT, *slab = lw.slab, *cslab = lw.cslab;
  const float* dy_amax = dy_amax_in;
  bool dx_done = false;
  const bool big16 = c.mode == 4 && rows >= 512 && (long)cdiv(rows, 256) * cdiv(k, 256) >= 16;
  if (dx != nullptr && !big16) {      // small problem: dgrad with the weight as stored (no transposed copy)
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = dy; p.lda = n; p.W = w; p.ldw = k; p.C = dx; p.ldc = k; p.M = rows; p.N = k; p.K = n;
    if (dx_accumulate) { p.flags = F_RESID; p.E1 = dx; p.lde1 = k; }
    if (small_nt_ok(p, true) && !(nt_use_s3(c, rows, k, n))) {
      TRY((launch_small<true>(p, st)));
      if (dx_amax_out != nullptr)
        TRY_RC((measure_absmax<PRO_NONE>(dx, k, nullptr, 0, nullptr, nullptr, nullptr, rows, k, dx_amax_out, lw.dxpart, st)));
      dx_done = true;
    }
  }
  if (dx != nullptr && !dx_done) {
    TRY(transpose(w, n, k, wT, st));   // wT [k, n]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = dy; p.lda = n; p.W = wT; p.ldw = n; p.C = dx; p.ldc = k; p.M = rows; p.N = k; p.K = n;
    p.wprep = lw.wprep;
    p.amaxA = dy_amax;
    p.amaxW = w_amax;        // max |W^T| = max |W|
    // dx += dy W: the old dx is the epilogue's residual operand; the instantiation with the output maximum is
    // the one whose epilogue may read and write the same buffer, so an accumulating call takes it as well
    if (dx_accumulate) { p.flags = F_RESID; p.E1 = dx; p.lde1 = k; }
    TRY((launch_nt<PRO_NONE, EPI_BIAS>(c, p, st, nullptr, dx_amax_out,
                                      (dx_accumulate || dx_amax_out != nullptr) ? lw.dxpart : nullptr)));
    dy_amax = p.amaxA;       // measured once for both GEMMs (lives in the head of lw.wprep)
  }
  if (dw != nullptr || db != nullptr) {
    TNParams t; memset(&t, 0, sizeof(t));
    t.amaxA = dy_amax;
    t.amaxB = x_amax;
    t.A = dy; t.lda = n; t.B = x; t.ldb = ldx; t.P = rows; t.Mo = n; t.Ni = k;
    TRY((launch_tn<PRO_NONE, PRO_NONE>(c, t, slab, cslab, dw, (long)k, db, st)));
  }
  return PRH_OK;
}
int prh_linear_backward(const float* x, long ldx, const float* w, const float* dy, float* dx,
                        float* dw, float* db, int rows, int k, int n, void* workspace,
                        size_t workspace_bytes, int device, void* stream) {
  return prh_linear_backward_ex(x, ldx, w, dy, dx, dw, db, rows, k, n, nullptr, nullptr, workspace,
                                workspace_bytes, device, stream);
}

// ------------------------------------------------------------------ MLP stack (point_mlp)
size_t prh_mlp_stack_workspace_bytes(int P, int n_layers, const prh_bn_layer* layers) {
  if (n_layers < 1 || n_layers > PRH_MAX_LAYERS) return 0;
  Arena a; MlpWS m;
  mlp_carve(stack_cores(gemm_mode()), a, m, P, layers, n_layers);
  return a.off + 256;
}

int prh_mlp_stack_forward(const prh_bn_layer* layers, int n_layers, int relu_last,
                          const float* x, int P, int training, float momentum, float eps,
                          float* z_cat, float* y, float* bn_scale, float* bn_shift,
                          float* bn_mean, float* bn_rstd, void* workspace,
                          size_t workspace_bytes, int device, void* stream) {
  TRY(check_stack(layers, n_layers));
  const Cores c = stack_cores(gemm_mode());
  if (!x || !z_cat || !y || !bn_scale || !bn_shift || !bn_mean || !bn_rstd || P <= 0)
    return fail(PRH_ERR_ARG, "mlp_stack_forward: bad argument");
  if (training && P < 2) return fail(PRH_ERR_ARG, "Expected more than 1 value per channel when training");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackDims d = stack_dims(layers, n_layers);
  Arena a(workspace, workspace_bytes);
  MlpWS m;
  mlp_carve(c, a, m, P, layers, n_layers);
  // present, and no smaller than prh_mlp_stack_workspace_bytes reports (the carve plus 256 bytes): lin16_ws_ok's rule
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "mlp_stack_forward: workspace too small (%zu bytes)", workspace_bytes);
  StackWS& w = m.w;
  const long ldz = d.off[n_layers];
  TRY(stack_forward(c, layers, n_layers, x, P, training, momentum, eps, z_cat, ldz, bn_scale,
                    bn_shift, bn_mean, bn_rstd, w, st));
  const int L = n_layers, co = layers[L - 1].cout;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(cdiv(P, 64), cdiv(co, 64)), dim3(256), 0, st,
                     z_cat + d.off[L - 1], ldz, bn_scale + d.off[L - 1], bn_shift + d.off[L - 1], P,
                     co, relu_last, y, (long)co);
  LAUNCH_CHECK();
  return PRH_OK;
}

int prh_mlp_stack_backward(const prh_bn_layer* layers, int n_layers, int relu_last,
                           const float* x, int P, int training, const float* dy,
                           const float* z_cat, const float* bn_scale, const float* bn_shift,
                           const float* bn_mean, const float* bn_rstd,
                           const prh_bn_layer_grad* grads, float* dx, void* workspace,
                           size_t workspace_bytes, int device, void* stream) {
  TRY(check_stack(layers, n_layers));
  const Cores c = stack_cores(gemm_mode());
  if (!x || !dy || !z_cat || P <= 0) return fail(PRH_ERR_ARG, "mlp_stack_backward: bad argument");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackDims d = stack_dims(layers, n_layers);
  const int L = n_layers;
  Arena a(workspace, workspace_bytes);
  MlpWS m;
  mlp_carve(c, a, m, P, layers, L);
  StackWS& w = m.w;
  StackBwdScratch& sc = m.sc;
  const long ldz = d.off[L];
  float* dy_cat = m.dy_cat;
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "mlp_stack_backward: workspace too small (%zu bytes)", workspace_bytes);
  if (d.cin0p != d.cin0) {
    TRY(copy_cols(x, d.cin0, d.cin0, w.xpad, d.cin0p, d.cin0p, (size_t)P, st));
    TRY(copy_cols(layers[0].w, d.cin0, d.cin0, w.w0pad, d.cin0p, d.cin0p, (size_t)layers[0].cout, st));
  }
  if (L > 1) HIP_TRY(hipMemsetAsync(dy_cat, 0, (size_t)P * ldz * sizeof(float), st));
  const int co = layers[L - 1].cout, o = d.off[L - 1];
  hipLaunchKernelGGL(bn_dy_stats_kernel, dim3(cdiv(P, 64), cdiv(co, 64)), dim3(256), 0, st, dy,
                     (long)co, z_cat + o, ldz, bn_scale + o, bn_shift + o, P, co, relu_last,
                     dy_cat + o, ldz, w.ws_a, w.ws_b);
  LAUNCH_CHECK();
  StatInfo si; si.count = cdiv(P, 64); si.rows = 64;
  return stack_backward(c, layers, L, x, P, training, dy_cat, ldz, z_cat, ldz, bn_scale, bn_shift,
                        bn_mean, bn_rstd, grads, dx, w, sc, si, st);
}

// ------------------------------------------------------------------ encoder
static int enc_cat(const prh_encoder_params* prm) {
  int c = 0;
  for (int l = 0; l < 5; ++l) c += prm->conv[l].cout;
  return c;
}

size_t prh_encoder_workspace_bytes(int B, int N, int in_channel, int out_dim, int backward) {
  const int P = B * N;
  prh_bn_layer ly[5];
  const int ch[6] = {in_channel, 64, 128, 256, 512, out_dim};
  for (int l = 0; l < 5; ++l) { ly[l].cin = ch[l]; ly[l].cout = ch[l + 1]; }
  const int cat = 64 + 128 + 256 + 512 + out_dim;
  Arena a; EncWS e;
  enc_carve(cores_of(gemm_mode()), a, e, P, ly, cat, out_dim, backward);
  return a.off + 256;
}

static int check_encoder(const prh_encoder_params* prm) {
  if (!prm) return fail(PRH_ERR_ARG, "encoder: null params");
  if (prm->in_channel < 4) return fail(PRH_ERR_ARG, "encoder: expected input to have at least 4 channels (x,y,z,intensity), got %d", prm->in_channel);
  if (prm->conv[0].cin != prm->in_channel) return fail(PRH_ERR_ARG, "encoder: conv1.cin != in_channel");
  TRY(check_stack(prm->conv, 5));
  if (prm->conv[4].cout != prm->out_dim) return fail(PRH_ERR_ARG, "encoder: conv5.cout != out_dim");
  if (prm->fusion.cin != enc_cat(prm) || prm->fusion.cout != prm->out_dim)
    return fail(PRH_ERR_ARG, "encoder: fusion layer shape mismatch");
  if (prm->out_dim % 4) return fail(PRH_ERR_ARG, "encoder: out_dim must be a multiple of 4");
  if (!prm->fusion.w || !prm->fusion.b || !prm->fusion.gamma || !prm->fusion.beta ||
      !prm->fusion.running_mean || !prm->fusion.running_var || !prm->gate_w1 || !prm->gate_b1 ||
      !prm->gate_w2 || !prm->gate_b2)
    return fail(PRH_ERR_ARG, "encoder: null parameter pointer");
  return PRH_OK;
}

// Step (1) of the encoder backward, through F = relu(bn(zf)) * m and the pooling: dy_f -> dyf (may be d_fused
// itself), dG -> gate, BatchNorm-backward partials [cdiv(P,64)][od] -> ws_a / ws_b.
//   recompute == 0: `gate` holds the forward's m; combine_bwd_kernel reads it and writes dG over it.
//   recompute != 0: `gate` holds nothing.  The forward's gate launch runs again with the backward epilogue, which
//     forms m from the accumulators (same core, weight image and operand scales: same bits), turns dyf from d
//     into dy_f in place, writes dG and combine_bwd_kernel's partials in its order.  Needs gate_on_h2() and no
//     pooled gradient.
int gate_combine_backward(Cores c, const float* inten, int C, int B, int N, int od, const float* gate_w1,
                          const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* z_fus,
                          const float* es, const float* et, const float* d_fused, const float* d_gfeat,
                          const int32_t* argmax, float* gate, int recompute, float* dyf, float* ws_a, float* ws_b,
                          char* wprep, hipStream_t st) {
  const int P = B * N;
  if (!recompute) {
    hipLaunchKernelGGL(combine_bwd_kernel, dim3(cdiv(P, 64), cdiv(od, 64)), dim3(256), 0, st, d_fused, d_gfeat,
                       argmax, z_fus, gate, es, et, P, N, od, dyf, ws_a, ws_b);
    LAUNCH_CHECK();
    return PRH_OK;
  }
  if (dyf != d_fused)
    HIP_TRY(hipMemcpyAsync(dyf, d_fused, (size_t)P * od * sizeof(float), hipMemcpyDeviceToDevice, st));
  NTParams p; memset(&p, 0, sizeof(p));
  p.A = inten; p.lda = C; p.pa = gate_w1; p.pb = gate_b1;
  p.W = gate_w2; p.ldw = 64; p.K = 64; p.M = P; p.N = od; p.bias = gate_b2;
  p.E1 = z_fus; p.lde1 = od; p.es = es; p.et = et;
  p.C = dyf; p.ldc = od; p.C2 = gate; p.ldc2 = od;
  p.ws_a = ws_a; p.ws_b = ws_b; p.wprep = wprep;
  return launch_nt<PRO_GATE1, EPI_GATE_BWD>(c, p, st);
}

int prh_encoder_gate_recompute(int B, int N, int in_channel, int out_dim, int want_global) {
  if (B <= 0 || N <= 0 || in_channel < 4 || out_dim <= 0 || (long)B * N > 2000000000L) return 0;
  return (!want_global && gate_on_h2(cores_of(gemm_mode()), B * N, out_dim, in_channel)) ? 1 : 0;
}

int prh_encoder_forward(const prh_encoder_params* prm, const float* ctx, int B, int N,
                        int training, float momentum, float eps, float* fused, float* gfeat,
                        const prh_encoder_saved* sv, void* workspace, size_t workspace_bytes,
                        int device, void* stream) {
  TRY(check_encoder(prm));
  if (!ctx || !fused || !sv || !sv->z_cat || !sv->z_fus || !sv->bn_scale || !sv->bn_shift ||
      !sv->bn_mean || !sv->bn_rstd || B <= 0 || N <= 0)
    return fail(PRH_ERR_ARG, "encoder_forward: bad argument");
  if ((long)B * N > 2000000000L) return fail(PRH_ERR_ARG, "encoder_forward: B*N too large");
  const int P = B * N;
  if (training && P < 2) return fail(PRH_ERR_ARG, "Expected more than 1 value per channel when training");
  const int cat = enc_cat(prm), od = prm->out_dim, C = prm->in_channel;
  const Cores c = cores_of(gemm_mode());
  Arena a(workspace, workspace_bytes);
  EncWS ews;
  enc_carve(c, a, ews, P, prm->conv, cat, od, 0);
  // present, and no smaller than prh_encoder_workspace_bytes reports (the carve plus 256 bytes): lin16_ws_ok's rule,
  // before the device is touched
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "encoder_forward: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackWS& w = ews.w;

  // conv1..5 (+bn, relu applied on load by the consumer)           src/model.py:43-47
  // operand maxima from the statistics epilogues (training, split-fp16 cores): slots 0..4 =
  // activations of conv1..5, slot 5 = their maximum = the fusion conv's operand
  float* op_amax = (training && c.mode == 3) ? sv->op_amax : nullptr;
  TRY(stack_forward(c, prm->conv, 5, ctx, P, training, momentum, eps, sv->z_cat, (long)cat,
                    sv->bn_scale, sv->bn_shift, sv->bn_mean, sv->bn_rstd, w, st, op_amax));
  // fusion conv over the (never materialised) concat               src/model.py:50-51
  {
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = sv->z_cat; p.lda = cat; p.W = prm->fusion.w; p.ldw = cat; p.K = cat;
    p.pa = sv->bn_scale; p.pb = sv->bn_shift;
    p.M = P; p.N = od; p.bias = prm->fusion.b; p.C = sv->z_fus; p.ldc = od;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
    if (op_amax != nullptr) {
      hipLaunchKernelGGL(max_of_kernel, dim3(1), dim3(1), 0, st, (const float*)op_amax, 5, op_amax + 5);
      LAUNCH_CHECK();
      p.amaxA = op_amax + 5;
      p.ws_c = w.ws_c; p.ws_d = w.ws_d;      // slot 6: max relu(BN(zf)) >= max of the gated output
    }
    StatInfo si;
    if (training) TRY((launch_nt<PRO_BNRELU, EPI_BIAS_STATS>(c, p, st, &si)));
    else TRY((launch_nt<PRO_BNRELU, EPI_BIAS>(c, p, st)));
    TRY(bn_coeffs(prm->fusion, P, training, momentum, eps, w.ws_a, w.ws_b, w.stat2, si, sv->bn_mean + cat,
                  sv->bn_rstd + cat, sv->bn_scale + cat, sv->bn_shift + cat, st, w.ws_c, w.ws_d, w.apart,
                  op_amax ? op_amax + 6 : nullptr));
  }
  // intensity gate GEMM + BN/ReLU/gate combine                     src/model.py:42,51,54-55
  {
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = ctx + 3; p.lda = C; p.pa = prm->gate_w1; p.pb = prm->gate_b1;
    p.W = prm->gate_w2; p.ldw = 64; p.K = 64; p.M = P; p.N = od; p.bias = prm->gate_b2;
    p.E1 = sv->z_fus; p.lde1 = od; p.es = sv->bn_scale + cat; p.et = sv->bn_shift + cat;
    p.C = fused; p.ldc = od; p.C2 = sv->gate; p.ldc2 = od;
    p.wprep = w.wprep;
    p.flags = sv->gate ? F_STORE_GATE : 0;
    // dual pooling (src/model.py:58-60) on the epilogue that writes `fused`, when a segment is a
    // whole number of 128-row wave tiles and the vector epilogue serves the launch
    const bool fuse_pool = gfeat != nullptr && (N % 128) == 0 && c.mode == 3 &&
                           nt_use_s3(c, P, od, 64) && (od & 3) == 0;
    if (fuse_pool) { p.flags |= F_POOL; p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.ws_c = w.ws_c; }
    TRY((launch_nt<PRO_GATE1, EPI_GATE>(c, p, st)));
    if ((p.flags & F_POOL) != 0) {
      hipLaunchKernelGGL(pool_tiles_kernel, dim3(cdiv(od, 256), B), dim3(256), 0, st, (const float*)w.ws_a,
                         (const float*)w.ws_b, (const int*)w.ws_c, N / 128, N, od, gfeat, sv->argmax);
      LAUNCH_CHECK();
      return PRH_OK;
    }
  }
  // dual pooling as a pass of its own                              src/model.py:58-60
  if (gfeat != nullptr) {
    hipLaunchKernelGGL(pool_kernel, dim3(cdiv(od, 64), B), dim3(256), 0, st, fused, N, od, gfeat,
                       sv->argmax);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}

int prh_encoder_backward(const prh_encoder_params* prm, const float* ctx, int B, int N,
                         int training, float* d_fused, const float* d_gfeat, int d_fused_scratch,
                         const prh_encoder_saved* sv, const prh_encoder_grads* gr, float* d_ctx,
                         void* workspace, size_t workspace_bytes, int device, void* stream) {
  TRY(check_encoder(prm));
  if (!ctx || !sv || !gr || !sv->z_cat || !sv->z_fus || !sv->gate || (!d_fused && !d_gfeat) || B <= 0 || N <= 0)
    return fail(PRH_ERR_ARG, "encoder_backward: bad argument (a gradient and saved.gate are required)");
  if (d_gfeat && !sv->argmax) return fail(PRH_ERR_ARG, "encoder_backward: d_gfeat needs saved.argmax");
  const int P = B * N;
  const int cat = enc_cat(prm), od = prm->out_dim, C = prm->in_channel;
  const Cores c = cores_of(gemm_mode());
  Arena a(workspace, workspace_bytes);
  EncWS ews;
  if (d_fused_scratch && (d_fused == nullptr || d_gfeat != nullptr))
    return fail(PRH_ERR_ARG, "encoder_backward: d_fused_scratch needs d_fused and no d_gfeat");
  enc_carve(c, a, ews, P, prm->conv, cat, od, d_fused_scratch ? 2 : 1);
  StackWS& w = ews.w;
  StackBwdScratch& sc = ews.sc;
  // combine_bwd_kernel reads dF[i] and writes dy[i] from the same thread: dy_f may live in the caller's d_fused
  float *fslab = ews.fslab, *fcslab = ews.fcslab, *dy_cat = ews.dy_cat, *dU = ews.dU, *dyf = d_fused_scratch ? d_fused : ews.dyf;
  float *gsum_a = ews.gsum_a, *gsum_b = ews.gsum_b;
  // lin16_ws_ok's rule against prh_encoder_workspace_bytes(.., d_fused_scratch ? 2 : 1), before the device is touched
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "encoder_backward: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackDims d = stack_dims(prm->conv, 5);
  if (d.cin0p != d.cin0) {
    TRY(copy_cols(ctx, d.cin0, d.cin0, w.xpad, d.cin0p, d.cin0p, (size_t)P, st));
    TRY(copy_cols(prm->conv[0].w, d.cin0, d.cin0, w.w0pad, d.cin0p, d.cin0p, (size_t)prm->conv[0].cout, st));
  }

  // (1) through F = relu(bn(zf)) * m and the pooling: dy_f -> dyf (workspace),
  //     dG -> saved.gate (in place), fusion-BN backward partials
  if (sv->gate_recompute && (d_gfeat != nullptr || !gate_on_h2(c, P, od, C)))
    return fail(PRH_ERR_ARG, "encoder_backward: saved.gate_recompute without prh_encoder_gate_recompute() "
                             "(pooled gradient, GEMM mode or shape)");
  TRY(gate_combine_backward(c, ctx + 3, C, B, N, od, prm->gate_w1, prm->gate_b1, prm->gate_w2, prm->gate_b2, sv->z_fus,
                            sv->bn_scale + cat, sv->bn_shift + cat, d_fused, d_gfeat, sv->argmax, sv->gate,
                            sv->gate_recompute, dyf, w.ws_a, w.ws_b, w.wprep, st));
  TRY(reduce_bn_stage1(w.ws_a, w.ws_b, cdiv(P, 64), (long)od, od, 64, P, 0, w.stat2, st));
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(od, 128)), dim3(128), 0, st, w.stat2, P, od,
                     prm->fusion.gamma, sv->bn_mean + cat, sv->bn_rstd + cat,
                     training, sc.ca, sc.cb, sc.cc, gr->fusion.dgamma, gr->fusion.dbeta,
                     gr->fusion.db);
  LAUNCH_CHECK();
  float* dG = sv->gate;

  // (2) fusion conv: wgrad over the virtual concat, dgrad into dy_cat (masked per layer),
  //     with layer-5 BN-backward partials (the only block that is complete here)
  StatInfo si5;
  const float* dzf_amax = nullptr;
  const bool matf = dz_in_place(c, od, (long)od, (long)od);
  if (matf) {       // split-fp16 mode: dyf <- dz_f in place
    TRY(materialize_dz(dyf, (long)od, sv->z_fus, (long)od, sc.ca, sc.cb, sc.cc, P, od, sc.hdr[0], st));
    dzf_amax = sc.hdr[0];
  }
  HeldWgrad hf;       // the fusion wgrad waits for conv5's coefficients and carries its apply pass (stack_backward)
  if (gr->fusion.dw) {
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = dyf; t.lda = od; t.A2 = sv->z_fus; t.lda2 = od; t.pa = sc.ca; t.pb = sc.cb; t.pc = sc.cc;
    t.B = sv->z_cat; t.ldb = cat; t.qa = sv->bn_scale; t.qb = sv->bn_shift;
    t.P = P; t.Mo = od; t.Ni = cat;
    t.amaxA = dzf_amax;
    if (training && c.mode == 3 && sv->op_amax != nullptr) t.amaxB = sv->op_amax + 5;
    if (matf && dz_in_place(c, od, (long)cat, (long)cat) &&
        tn_side_ok(c, t, side_job(dy_cat + d.off[4], (long)cat, sv->z_cat + d.off[4], (long)cat, sc, P, od, sc.hdr[1]))) {
      hf.on = true; hf.t = t; hf.slab = fslab; hf.colslab = fcslab; hf.out = gr->fusion.dw; hf.ldc = (long)cat;
    } else if (matf) TRY((launch_tn<PRO_NONE, PRO_BNRELU>(c, t, fslab, fcslab, gr->fusion.dw, (long)cat, nullptr, st)));
    else TRY((launch_tn<PRO_BNBWD, PRO_BNRELU>(c, t, fslab, fcslab, gr->fusion.dw, (long)cat, nullptr, st)));
    dzf_amax = t.amaxA;
  }
  {
    TRY(transpose(prm->fusion.w, od, cat, sc.wT, st));   // [cat, od]
    NTParams p; memset(&p, 0, sizeof(p));
    p.amaxA = dzf_amax;
    p.A = dyf; p.lda = od; p.A2 = sv->z_fus; p.lda2 = od; p.pa = sc.ca; p.pb = sc.cb; p.pc = sc.cc;
    p.W = sc.wT; p.ldw = od; p.M = P; p.N = cat; p.K = od;
    p.C = dy_cat; p.ldc = cat; p.E1 = sv->z_cat; p.lde1 = cat; p.es = sv->bn_scale; p.et = sv->bn_shift;
    p.wprep = w.wprep;
    // BN-backward partial sums of every column ride on the epilogue; only layer 5's block of
    // them is final here (no later conv adds into it) and is consumed below - the blocks of
    // layers 1..4 are recomputed by the dgrad that completes them
    p.ws_a = w.ws_a; p.ws_b = w.ws_b;
    p.flags = F_MASK | F_STATS;
    if (matf) TRY((launch_nt<PRO_NONE, EPI_DGRAD>(c, p, st, &si5)));
    else TRY((launch_nt<PRO_BNBWD, EPI_DGRAD>(c, p, st, &si5)));
    si5.ld = cat; si5.off = d.off[4];
  }
  // (3) conv5..conv1
  float* dx = d_ctx;
  TRY(stack_backward(c, prm->conv, 5, ctx, P, training, dy_cat, (long)cat, sv->z_cat, (long)cat,
                     sv->bn_scale, sv->bn_shift, sv->bn_mean, sv->bn_rstd, gr->conv, dx, w, sc, si5,
                     st, sv->op_amax, &hf));

  // (4) intensity gate: dW2 = dG^T u, db2 = colsum dG; dU = dG W2 masked by u>0 with
  //     column sums (db1) and intensity-weighted column sums (dw1)
  {
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = dG; t.lda = od; t.B = ctx + 3; t.ldb = C; t.qa = prm->gate_w1; t.qb = prm->gate_b1;
    t.P = P; t.Mo = od; t.Ni = 64;
    TRY((launch_tn<PRO_NONE, PRO_GATE1>(c, t, fslab, fcslab, gr->d_gate_w2, 64L, gr->d_gate_b2, st)));
    TRY(transpose(prm->gate_w2, od, 64, sc.wT, st));   // [64, od]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = dG; p.lda = od; p.W = sc.wT; p.ldw = od; p.M = P; p.N = 64; p.K = od;
    p.C = dU; p.ldc = 64; p.E1 = ctx + 3; p.lde1 = C; p.es = prm->gate_w1; p.et = prm->gate_b1;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b;
    p.flags = F_MASK | F_STATS | F_E1_ROWVEC;
    StatInfo sig;
    TRY((launch_nt<PRO_NONE, EPI_DGRAD>(c, p, st, &sig)));
    TRY(reduce_partials(w.ws_a, w.ws_b, sig.count, 64, gr->d_gate_b1 ? gr->d_gate_b1 : gsum_a,
                        gr->d_gate_w1 ? gr->d_gate_w1 : gsum_b, st));
    if (d_ctx != nullptr) {
      hipLaunchKernelGGL(gate1_dctx_kernel, dim3(cdiv(P, 4)), dim3(256), 0, st, dU, P, 64,
                         prm->gate_w1, d_ctx, (long)C);
      LAUNCH_CHECK();
    }
  }
  return PRH_OK;
}

// ------------------------------------------------------------------ bf16 mode (BASELINE config 3)
// Encoder with bf16 activation storage on the bf16 cores (prh_b16.hpp); same arithmetic and
// the same order of operations as prh_encoder_forward / prh_encoder_backward.

// Every shape rule of the launches inside the two entry points (launch_nt_b16, launch_tn_b16, bn_bwd_apply16, the
// combine kernels), so that a shape is refused before the device is touched and before anything is written:
// 8-element vectors of bf16 on every width, the fusion conv's K = cat within the LDS image of its BN+ReLU prologue
// (cat <= 3968, i.e. out_dim <= 3008), and - backward, when d_ctx is asked for - in_channel % 4 == 0 for the fp32
// vector stores of the conv1 dgrad.
static int check_encoder_bf16(const prh_encoder_params* prm, long P, bool want_dctx, const char* who) {
  if (P > 1000000000L) return fail(PRH_ERR_ARG, "%s: B*N too large", who);
  for (int l = 0; l < 5; ++l)
    if (prm->conv[l].cout % 8) return fail(PRH_ERR_ARG, "%s: channel widths must be multiples of 8", who);
  if (prm->out_dim % 8) return fail(PRH_ERR_ARG, "%s: out_dim must be a multiple of 8", who);
  if (!nt_b16_depth_ok(enc_cat(prm), PRO_BNRELU))
    return fail(PRH_ERR_ARG, "%s: out_dim=%d puts the fusion conv's K=%d beyond the prologue coefficient image (K <= 3968)",
                who, prm->out_dim, enc_cat(prm));
  if (want_dctx && prm->in_channel % 4) return fail(PRH_ERR_ARG, "%s: d_ctx needs in_channel %% 4 == 0", who);
  return PRH_OK;
}

size_t prh_encoder_bf16_workspace_bytes(int B, int N, int in_channel, int out_dim, int backward) {
  const int ch[6] = {in_channel, 64, 128, 256, 512, out_dim};
  Arena a; Enc16WS e;
  enc16_carve(a, e, B * N, ch, 64 + 128 + 256 + 512 + out_dim, out_dim, backward != 0);
  return a.off + 256;
}

int prh_encoder_forward_bf16(const prh_encoder_params* prm, const float* ctx, int B, int N, int training,
                             float momentum, float eps, uint16_t* fused, float* gfeat,
                             const prh_encoder_saved_bf16* sv, void* workspace, size_t workspace_bytes,
                             int device, void* stream) {
  TRY(check_encoder(prm));
  if (!ctx || !fused || !sv || !sv->z_cat || !sv->z_fus || !sv->bn_scale || !sv->bn_shift || !sv->bn_mean ||
      !sv->bn_rstd || B <= 0 || N <= 0)
    return fail(PRH_ERR_ARG, "encoder_forward_bf16: bad argument");
  TRY(check_encoder_bf16(prm, (long)B * N, false, "encoder_forward_bf16"));
  const int P = B * N;
  if (training && P < 2) return fail(PRH_ERR_ARG, "Expected more than 1 value per channel when training");
  const int cat = enc_cat(prm), od = prm->out_dim, C = prm->in_channel, c0p = cin_pad8(C);
  const int ch[6] = {C, prm->conv[0].cout, prm->conv[1].cout, prm->conv[2].cout, prm->conv[3].cout, od};
  Arena a(workspace, workspace_bytes);
  Enc16WS w;
  enc16_carve(a, w, P, ch, cat, od, false);
  // lin16_ws_ok's rule against prh_encoder_bf16_workspace_bytes, before the device is touched
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "encoder_forward_bf16: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackDims d = stack_dims(prm->conv, 5);
  u16* z_cat = sv->z_cat;
  // conv1 on fp32 operands (VALU, K = in_channel): x, y, z in metres and the raw intensity are never
  // rounded to bf16.  Other first-layer shapes: context rows -> bf16 padded to 8 channels, bf16 core
  const bool c1_fp32 = conv_in_fp32_ok(C, prm->conv[0].cout);
  if (!c1_fp32) {
    TRY(cast_b16(ctx, C, C, w.xpad, c0p, c0p, (size_t)P, st));
    TRY(copy_cols(prm->conv[0].w, C, C, w.w0pad, c0p, c0p, (size_t)prm->conv[0].cout, st));
  }
  for (int l = 0; l < 5; ++l) {                       // conv1..5, BN+ReLU applied on load by the consumer
    const prh_bn_layer& ly = prm->conv[l];
    NTParams p; memset(&p, 0, sizeof(p));
    p.M = P; p.N = ly.cout; p.bias = ly.b; p.C = f16p(z_cat + d.off[l]); p.ldc = cat;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
    StatInfo si;
    if (l == 0 && c1_fp32) {
      hipLaunchKernelGGL((conv_in_b16_kernel<64>), dim3(cdiv(P, 128)), dim3(256), 0, st, ctx, C, ly.w, ly.b, z_cat, (long)cat, P,
                         training, w.ws_a, w.ws_b);
      LAUNCH_CHECK();
      si.count = cdiv(P, 128); si.rows = 128;
    } else if (l == 0) {
      p.A = f16p(w.xpad); p.lda = c0p; p.W = w.w0pad; p.ldw = c0p; p.K = c0p;
      if (training) TRY((launch_nt_b16<PRO_NONE, EPI_BIAS_STATS, true, true>(p, st, &si)));
      else TRY((launch_nt_b16<PRO_NONE, EPI_BIAS, true, true>(p, st)));
    } else {
      p.A = f16p(z_cat + d.off[l - 1]); p.lda = cat; p.W = ly.w; p.ldw = ly.cin; p.K = ly.cin;
      p.pa = sv->bn_scale + d.off[l - 1]; p.pb = sv->bn_shift + d.off[l - 1];
      if (training) TRY((launch_nt_b16<PRO_BNRELU, EPI_BIAS_STATS, true, true>(p, st, &si)));
      else TRY((launch_nt_b16<PRO_BNRELU, EPI_BIAS, true, true>(p, st)));
    }
    TRY(bn_coeffs(ly, P, training, momentum, eps, w.ws_a, w.ws_b, w.stat2, si, sv->bn_mean + d.off[l],
                  sv->bn_rstd + d.off[l], sv->bn_scale + d.off[l], sv->bn_shift + d.off[l], st));
  }
  {                                                   // fusion conv over the virtual concat
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = f16p(z_cat); p.lda = cat; p.W = prm->fusion.w; p.ldw = cat; p.K = cat;
    p.pa = sv->bn_scale; p.pb = sv->bn_shift;
    p.M = P; p.N = od; p.bias = prm->fusion.b; p.C = f16p(sv->z_fus); p.ldc = od;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
    StatInfo si;
    if (training) TRY((launch_nt_b16<PRO_BNRELU, EPI_BIAS_STATS, true, true>(p, st, &si)));
    else TRY((launch_nt_b16<PRO_BNRELU, EPI_BIAS, true, true>(p, st)));
    TRY(bn_coeffs(prm->fusion, P, training, momentum, eps, w.ws_a, w.ws_b, w.stat2, si, sv->bn_mean + cat,
                  sv->bn_rstd + cat, sv->bn_scale + cat, sv->bn_shift + cat, st));
  }
  {                                                   // intensity gate GEMM + BN/ReLU/gate combine
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = ctx + 3; p.lda = C; p.pa = prm->gate_w1; p.pb = prm->gate_b1;
    p.W = prm->gate_w2; p.ldw = 64; p.K = 64; p.M = P; p.N = od; p.bias = prm->gate_b2;
    p.E1 = f16p(sv->z_fus); p.lde1 = od; p.es = sv->bn_scale + cat; p.et = sv->bn_shift + cat;
    p.C = f16p(fused); p.ldc = od; p.C2 = f16p(sv->gate); p.ldc2 = od;
    p.wprep = w.wprep;
    p.flags = sv->gate ? F_STORE_GATE : 0;
    const bool fuse_pool = gfeat != nullptr && (N % 128) == 0;
    if (fuse_pool) { p.flags |= F_POOL; p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.ws_c = w.ws_c; }
    TRY((launch_nt_b16<PRO_GATE1, EPI_GATE, true, true>(p, st)));
    if (fuse_pool) {
      hipLaunchKernelGGL(pool_tiles_kernel, dim3(cdiv(od, 256), B), dim3(256), 0, st, (const float*)w.ws_a,
                         (const float*)w.ws_b, (const int*)w.ws_c, N / 128, N, od, gfeat, sv->argmax);
      LAUNCH_CHECK();
      return PRH_OK;
    }
  }
  if (gfeat != nullptr) {
    hipLaunchKernelGGL(pool_b16_kernel, dim3(cdiv(od, 64), B), dim3(256), 0, st, (const u16*)fused, N, od, gfeat, sv->argmax);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}

int prh_encoder_backward_bf16(const prh_encoder_params* prm, const float* ctx, int B, int N, int training,
                              const uint16_t* d_fused, const float* d_gfeat, const prh_encoder_saved_bf16* sv,
                              const prh_encoder_grads* gr, float* d_ctx, void* workspace, size_t workspace_bytes,
                              int device, void* stream) {
  TRY(check_encoder(prm));
  if (!ctx || !sv || !gr || !sv->z_cat || !sv->z_fus || !sv->gate || (!d_fused && !d_gfeat) || B <= 0 || N <= 0)
    return fail(PRH_ERR_ARG, "encoder_backward_bf16: bad argument (a gradient and saved.gate are required)");
  if (d_gfeat && !sv->argmax) return fail(PRH_ERR_ARG, "encoder_backward_bf16: d_gfeat needs saved.argmax");
  // every shape refusal of the launches below, before the device is touched: saved.gate is overwritten by step (1)
  TRY(check_encoder_bf16(prm, (long)B * N, d_ctx != nullptr, "encoder_backward_bf16"));
  const int P = B * N;
  const int cat = enc_cat(prm), od = prm->out_dim, C = prm->in_channel, c0p = cin_pad8(C);
  const int ch[6] = {C, prm->conv[0].cout, prm->conv[1].cout, prm->conv[2].cout, prm->conv[3].cout, od};
  Arena a(workspace, workspace_bytes);
  Enc16WS w;
  enc16_carve(a, w, P, ch, cat, od, true);
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "encoder_backward_bf16: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  StackDims d = stack_dims(prm->conv, 5);
  const u16* z_cat = sv->z_cat;
  const bool c1_fp32 = conv_in_fp32_ok(C, prm->conv[0].cout);
  if (!c1_fp32) TRY(cast_b16(ctx, C, C, w.xpad, c0p, c0p, (size_t)P, st));
  if (!c1_fp32 || d_ctx != nullptr) TRY(copy_cols(prm->conv[0].w, C, C, w.w0pad, c0p, c0p, (size_t)prm->conv[0].cout, st));

  // (1) through F = relu(bn(zf)) * m and the pooling: dy_f, dG (over saved.gate), fusion-BN partials
  if (od == 256 || od == 512 || od == 1024 || od == 2048)      // 16-byte accesses: od / 8 threads per row
    hipLaunchKernelGGL(combine_bwd_b16v_kernel, dim3(cdiv(P, 64)), dim3(256), 0, st, (const u16*)d_fused, d_gfeat,
                       sv->argmax, (const u16*)sv->z_fus, (u16*)sv->gate, sv->bn_scale + cat, sv->bn_shift + cat, P, N, od,
                       w.dyf, w.ws_a, w.ws_b);
  else
    hipLaunchKernelGGL(combine_bwd_b16_kernel, dim3(cdiv(P, 64), cdiv(od, 64)), dim3(256), 0, st, (const u16*)d_fused,
                       d_gfeat, sv->argmax, (const u16*)sv->z_fus, (u16*)sv->gate, sv->bn_scale + cat, sv->bn_shift + cat,
                       P, N, od, w.dyf, w.ws_a, w.ws_b);
  LAUNCH_CHECK();
  TRY(reduce_bn_stage1(w.ws_a, w.ws_b, cdiv(P, 64), (long)od, od, 64, P, 0, w.stat2, st));
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(od, 128)), dim3(128), 0, st, w.stat2, P, od, prm->fusion.gamma,
                     sv->bn_mean + cat, sv->bn_rstd + cat, training, w.ca, w.cb, w.cc, gr->fusion.dgamma,
                     gr->fusion.dbeta, gr->fusion.db);
  LAUNCH_CHECK();
  u16* dG = sv->gate;
  // (2) fusion conv: dz_f in place, wgrad over the virtual concat, dgrad into dy_cat (masked per layer)
  TRY(bn_bwd_apply16(w.dyf, od, sv->z_fus, od, w.ca, w.cb, w.cc, P, od, st));
  if (gr->fusion.dw) {
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = f16p(w.dyf); t.lda = od; t.B = f16p(z_cat); t.ldb = cat; t.qa = sv->bn_scale; t.qb = sv->bn_shift;
    t.P = P; t.Mo = od; t.Ni = cat;
    TRY((launch_tn_b16<PRO_BNRELU>(t, w.slab, w.cslab, gr->fusion.dw, (long)cat, nullptr, st)));
  }
  StatInfo si;
  {
    TRY(transpose(prm->fusion.w, od, cat, w.wT, st));   // [cat, od]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = f16p(w.dyf); p.lda = od; p.W = w.wT; p.ldw = od; p.M = P; p.N = cat; p.K = od;
    p.C = f16p(w.dy_cat); p.ldc = cat; p.E1 = f16p(z_cat); p.lde1 = cat; p.es = sv->bn_scale; p.et = sv->bn_shift;
    p.wprep = w.wprep; p.ws_a = w.ws_a; p.ws_b = w.ws_b;
    p.flags = F_MASK | F_STATS;
    TRY((launch_nt_b16<PRO_NONE, EPI_DGRAD, true, true>(p, st, &si)));
    si.ld = cat; si.off = d.off[4];
  }
  // (3) conv5..conv1
  for (int l = 4; l >= 0; --l) {
    const prh_bn_layer& ly = prm->conv[l];
    const int co = ly.cout, o = d.off[l];
    TRY(reduce_bn_stage1(w.ws_a + si.off, w.ws_b + si.off, si.count, si.ld ? si.ld : (long)co, co, 64, P, 0, w.stat2, st));
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(co, 128)), dim3(128), 0, st, w.stat2, P, co, ly.gamma,
                       sv->bn_mean + o, sv->bn_rstd + o, training, w.ca, w.cb, w.cc, gr->conv[l].dgamma,
                       gr->conv[l].dbeta, gr->conv[l].db);
    LAUNCH_CHECK();
    TRY(bn_bwd_apply16(w.dy_cat + o, cat, z_cat + o, cat, w.ca, w.cb, w.cc, P, co, st));
    if (gr->conv[l].dw) {
      TNParams t; memset(&t, 0, sizeof(t));
      t.A = f16p(w.dy_cat + o); t.lda = cat; t.P = P; t.Mo = co;
      if (l == 0 && c1_fp32) {       // fp32 context rows as the second operand (VALU reduction)
        const int rpb = cdiv(cdiv(P, C1_WGRAD_BLOCKS), 4) * 4, nb = cdiv(P, rpb);
        hipLaunchKernelGGL((conv_in_wgrad_b16_kernel<64>), dim3(nb), dim3(256), 0, st, (const u16*)(w.dy_cat + o), (long)cat,
                           ctx, C, P, rpb, w.c1part);
        LAUNCH_CHECK();
        TRY(reduce_slabs(w.c1part, nb, co, C, gr->conv[0].dw, (long)C, nullptr, 0, nullptr, st));
      } else if (l == 0) {
        t.B = f16p(w.xpad); t.ldb = c0p; t.Ni = c0p;
        float* out = c0p == C ? gr->conv[0].dw : w.wT;        // padded input: reduce into scratch, drop the pad columns
        TRY((launch_tn_b16<PRO_NONE>(t, w.slab, w.cslab, out, (long)c0p, nullptr, st)));
        if (c0p != C) TRY(copy_cols(w.wT, c0p, C, gr->conv[0].dw, C, C, (size_t)co, st));
      } else {
        t.B = f16p(z_cat + d.off[l - 1]); t.ldb = cat; t.Ni = ly.cin;
        t.qa = sv->bn_scale + d.off[l - 1]; t.qb = sv->bn_shift + d.off[l - 1];
        TRY((launch_tn_b16<PRO_BNRELU>(t, w.slab, w.cslab, gr->conv[l].dw, (long)ly.cin, nullptr, st)));
      }
    }
    if (l > 0) {
      TRY(transpose(ly.w, co, ly.cin, w.wT, st));        // wT [cin, cout]
      NTParams p; memset(&p, 0, sizeof(p));
      p.A = f16p(w.dy_cat + o); p.lda = cat; p.W = w.wT; p.ldw = co; p.M = P; p.N = ly.cin; p.K = co;
      p.C = f16p(w.dy_cat + d.off[l - 1]); p.ldc = cat;
      p.E1 = f16p(z_cat + d.off[l - 1]); p.lde1 = cat;
      p.es = sv->bn_scale + d.off[l - 1]; p.et = sv->bn_shift + d.off[l - 1];
      p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
      p.flags = F_ACCUM | F_MASK | F_STATS;
      TRY((launch_nt_b16<PRO_NONE, EPI_DGRAD, true, true>(p, st, &si)));
      si.ld = 0; si.off = 0;
    } else if (d_ctx != nullptr) {
      TRY(transpose(w.w0pad, co, c0p, w.wT, st));        // [c0p, cout], zero pad rows
      NTParams p; memset(&p, 0, sizeof(p));
      p.A = f16p(w.dy_cat + o); p.lda = cat; p.W = w.wT; p.ldw = co; p.M = P; p.N = C; p.K = co;
      p.C = d_ctx; p.ldc = C; p.wprep = w.wprep; p.flags = 0;
      TRY((launch_nt_b16<PRO_NONE, EPI_DGRAD, true, false>(p, st)));
    }
  }
  // (4) intensity gate: dW2 = dG^T u, db2 = colsum dG; dU = dG W2 masked by u > 0 with column
  //     sums (db1) and intensity-weighted column sums (dw1)
  {
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = f16p(dG); t.lda = od; t.B = ctx + 3; t.ldb = C; t.qa = prm->gate_w1; t.qb = prm->gate_b1;
    t.P = P; t.Mo = od; t.Ni = 64;
    TRY((launch_tn_b16<PRO_GATE1>(t, w.slab, w.cslab, gr->d_gate_w2, 64L, gr->d_gate_b2, st)));
    TRY(transpose(prm->gate_w2, od, 64, w.wT, st));   // [64, od]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = f16p(dG); p.lda = od; p.W = w.wT; p.ldw = od; p.M = P; p.N = 64; p.K = od;
    p.C = w.dU; p.ldc = 64; p.E1 = ctx + 3; p.lde1 = C; p.es = prm->gate_w1; p.et = prm->gate_b1;
    p.ws_a = w.ws_a; p.ws_b = w.ws_b; p.wprep = w.wprep;
    p.flags = F_MASK | F_STATS | F_E1_ROWVEC;
    StatInfo sig;
    TRY((launch_nt_b16<PRO_NONE, EPI_DGRAD, true, false>(p, st, &sig)));
    TRY(reduce_partials(w.ws_a, w.ws_b, sig.count, 64, gr->d_gate_b1 ? gr->d_gate_b1 : w.gsum_a,
                        gr->d_gate_w1 ? gr->d_gate_w1 : w.gsum_b, st));
    if (d_ctx != nullptr) {
      hipLaunchKernelGGL(gate1_dctx_kernel, dim3(cdiv(P, 4)), dim3(256), 0, st, w.dU, P, 64, prm->gate_w1, d_ctx, (long)C);
      LAUNCH_CHECK();
    }
  }
  return PRH_OK;
}

// nn.Linear whose input is a bf16 activation (context_proj on the bf16 `fused`): y fp32
size_t prh_linear_bf16_workspace_bytes(int rows, int k, int n, int backward) {
  Arena a; Lin16WS w;
  lin16_carve(a, w, rows, k, n, backward != 0);
  return a.off + 256;
}
int prh_linear_forward_bf16(const uint16_t* x, long ldx, const float* w, const float* b, float* y, int rows, int k,
                            int n, int relu, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!x || !w || !y || rows < 0 || k <= 0 || n <= 0) return fail(PRH_ERR_ARG, "linear_forward_bf16: bad argument");
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes); Lin16WS lw;
  lin16_carve(a, lw, rows, k, n, false);
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "linear_forward_bf16: workspace too small (%zu bytes)", workspace_bytes);
  NTParams p; memset(&p, 0, sizeof(p));
  p.A = f16p(x); p.lda = ldx; p.W = w; p.ldw = k; p.C = y; p.ldc = n; p.M = rows; p.N = n; p.K = k; p.bias = b;
  p.flags = relu ? F_RELU_OUT : 0; p.wprep = lw.wprep;
  return launch_nt_b16<PRO_NONE, EPI_BIAS, true, false>(p, (hipStream_t)stream);
}
int prh_linear_backward_bf16(const uint16_t* x, long ldx, const float* w, const float* dy, uint16_t* dx, float* dw,
                             float* db, int rows, int k, int n, void* workspace, size_t workspace_bytes, int device,
                             void* stream) {
  if (!x || !w || !dy || rows < 0 || k <= 0 || n <= 0) return fail(PRH_ERR_ARG, "linear_backward_bf16: bad argument");
  if ((k & 7) || (n & 7)) return fail(PRH_ERR_ARG, "linear_backward_bf16: k=%d and n=%d must be multiples of 8", k, n);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  Arena a(workspace, workspace_bytes); Lin16WS lw;
  lin16_carve(a, lw, rows, k, n, true);
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "linear_backward_bf16: workspace too small (%zu bytes)", workspace_bytes);
  TRY(cast_b16(dy, n, n, lw.dy16, n, n, (size_t)rows, st));      // one operand for both GEMMs
  if (dx != nullptr) {
    TRY(transpose(w, n, k, lw.wT, st));   // wT [k, n]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = f16p(lw.dy16); p.lda = n; p.W = lw.wT; p.ldw = n; p.C = f16p(dx); p.ldc = k; p.M = rows; p.N = k; p.K = n;
    p.wprep = lw.wprep;
    TRY((launch_nt_b16<PRO_NONE, EPI_BIAS, true, true>(p, st)));
  }
  if (dw != nullptr || db != nullptr) {
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = f16p(lw.dy16); t.lda = n; t.B = f16p(x); t.ldb = ldx; t.P = rows; t.Mo = n; t.Ni = k;
    TRY((launch_tn_b16<PRO_NONE>(t, lw.slab, lw.cslab, dw, (long)k, db, st)));
  }
  return PRH_OK;
}

// nn.Linear from an fp32 input to a bf16 OUTPUT, and its backward from a bf16 gradient: the wide
// cross-attention key / value projections of the bf16 mode (src/model.py:123-126 for all six layers),
// whose outputs and gradients live in bf16
int prh_linear_forward_out16(const float* x, long ldx, const float* w, const float* b, uint16_t* y, int rows, int k,
                             int n, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!x || !w || !y || rows < 0 || k <= 0 || n <= 0) return fail(PRH_ERR_ARG, "linear_forward_out16: bad argument");
  HIP_TRY(hipSetDevice(device));
  Arena a(workspace, workspace_bytes); Lin16WS lw;
  lin16_carve(a, lw, rows, k, n, false);
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "linear_forward_out16: workspace too small (%zu bytes)", workspace_bytes);
  NTParams p; memset(&p, 0, sizeof(p));
  p.A = x; p.lda = ldx; p.W = w; p.ldw = k; p.C = f16p(y); p.ldc = n; p.M = rows; p.N = n; p.K = k; p.bias = b;
  p.wprep = lw.wprep;
  return launch_nt_b16<PRO_NONE, EPI_BIAS, false, true>(p, (hipStream_t)stream);
}
int prh_linear_backward_dy16(const float* x, long ldx, const float* w, const uint16_t* dy, float* dx, float* dw,
                             float* db, int rows, int k, int n, void* workspace, size_t workspace_bytes, int device,
                             void* stream) {
  if (!x || !w || !dy || rows < 0 || k <= 0 || n <= 0) return fail(PRH_ERR_ARG, "linear_backward_dy16: bad argument");
  if ((k & 7) || (n & 7)) return fail(PRH_ERR_ARG, "linear_backward_dy16: k=%d and n=%d must be multiples of 8", k, n);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  Arena a(workspace, workspace_bytes); Lin16WS lw;
  lin16_carve(a, lw, rows, k, n, true);
  if (!lin16_ws_ok(a, workspace, workspace_bytes))
    return fail(PRH_ERR_WORKSPACE, "linear_backward_dy16: workspace too small (%zu bytes)", workspace_bytes);
  if (dx != nullptr) {
    TRY(transpose(w, n, k, lw.wT, st));   // wT [k, n]
    NTParams p; memset(&p, 0, sizeof(p));
    p.A = f16p(dy); p.lda = n; p.W = lw.wT; p.ldw = n; p.C = dx; p.ldc = k; p.M = rows; p.N = k; p.K = n;
    p.wprep = lw.wprep;
    TRY((launch_nt_b16<PRO_NONE, EPI_BIAS, true, false>(p, st)));
  }
  if (dw != nullptr || db != nullptr) {
    TRY(cast_b16(x, ldx, k, lw.dy16, k, k, (size_t)rows, st));      // x in bf16: the wgrad's B operand
    TNParams t; memset(&t, 0, sizeof(t));
    t.A = f16p(dy); t.lda = n; t.B = f16p(lw.dy16); t.ldb = k; t.P = rows; t.Mo = n; t.Ni = k;
    TRY((launch_tn_b16<PRO_NONE>(t, lw.slab, lw.cslab, dw, (long)k, db, st)));
  }
  return PRH_OK;
}

// ------------------------------------------------------------------ fused eval encoder (prh_fused.hpp)
size_t prh_encoder_fused_image_bytes(int planes, int in_channel) {
  if ((planes != 1 && planes != 2) || in_channel < 4 || in_channel > 64) return 0;
  return fused_layout(planes, in_channel).total + 256;
}
int prh_encoder_fused_prepare(const prh_encoder_params* prm, float eps, const float* proj_w, const float* proj_b,
                              int planes, void* image, size_t image_bytes, int device, void* stream) {
  TRY(check_encoder(prm));
  if (planes != 1 && planes != 2) return fail(PRH_ERR_ARG, "encoder_fused_prepare: planes must be 1 (fp16) or 2 (split fp16)");
  if (prm->in_channel > 64) return fail(PRH_ERR_ARG, "encoder_fused_prepare: at most 64 input channels");
  static const int want[5] = {64, 128, 256, 512, 1024};
  for (int l = 0; l < 5; ++l)
    if (prm->conv[l].cout != want[l])
      return fail(PRH_ERR_ARG, "encoder_fused_prepare: the fused kernel is built for widths 64/128/256/512/1024 (conv%d has %d)",
                  l + 1, prm->conv[l].cout);
  if (prm->out_dim != 1024) return fail(PRH_ERR_ARG, "encoder_fused_prepare: out_dim must be 1024");
  if (!image || ((uintptr_t)image & 255)) return fail(PRH_ERR_ARG, "encoder_fused_prepare: image must be 256-byte aligned");
  const FusedLayout L = fused_layout(planes, prm->in_channel);
  if (image_bytes < L.total) return fail(PRH_ERR_WORKSPACE, "encoder_fused_prepare: image buffer too small (%zu < %zu)", image_bytes, L.total);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  char* img = (char*)image;
  const int C = prm->in_channel;
  auto f32 = [&](size_t off) { return reinterpret_cast<float*>(img + off); };
  HIP_TRY(hipMemsetAsync(img + L.amax, 0, 32, st));
  // conv1 (VALU layer) and the gate's hidden layer: fp32
  hipLaunchKernelGGL(fe_conv1_kernel, dim3(cdiv(64 * C, 256)), dim3(256), 0, st, prm->conv[0].w, prm->conv[0].gamma,
                     (const float*)prm->conv[0].running_var, eps, 64, C, f32(L.c1w));
  LAUNCH_CHECK();
  hipLaunchKernelGGL(fe_bias_kernel, dim3(1), dim3(64), 0, st, prm->conv[0].b, prm->conv[0].gamma, prm->conv[0].beta,
                     (const float*)prm->conv[0].running_mean, (const float*)prm->conv[0].running_var, eps, 64, f32(L.c1b));
  LAUNCH_CHECK();
  HIP_TRY(hipMemcpyAsync(f32(L.g1w), prm->gate_w1, 64 * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(f32(L.g1b), prm->gate_b1, 64 * 4, hipMemcpyDeviceToDevice, st));
  struct Src { const float* w; const float* b; const float* gamma; const float* beta; const float* rm; const float* rv; };
  Src src[FE_NL];
  for (int l = 0; l < 4; ++l) {
    const prh_bn_layer& y = prm->conv[l + 1];
    src[l] = {y.w, y.b, y.gamma, y.beta, y.running_mean, y.running_var};
  }
  src[4] = {prm->fusion.w, prm->fusion.b, prm->fusion.gamma, prm->fusion.beta, prm->fusion.running_mean, prm->fusion.running_var};
  src[5] = {prm->gate_w2, prm->gate_b2, nullptr, nullptr, nullptr, nullptr};
  src[6] = {proj_w, proj_b, nullptr, nullptr, nullptr, nullptr};
  for (int l = 0; l < FE_NL; ++l) {
    if (src[l].w == nullptr) continue;                      // no context_proj: image slot left unused
    const int N = FE_N[l], K = FE_K[l];
    hipLaunchKernelGGL(fe_bias_kernel, dim3(cdiv(N, 256)), dim3(256), 0, st, src[l].b, src[l].gamma, src[l].beta, src[l].rm,
                       src[l].rv, eps, N, f32(L.bias[l]));
    LAUNCH_CHECK();
    float* amax = f32(L.amax) + l;
    if (planes == 2) {
      hipLaunchKernelGGL(fe_amax_kernel, dim3(256), dim3(256), 0, st, src[l].w, (long)K, N, K, src[l].gamma, src[l].rv, eps,
                         reinterpret_cast<unsigned*>(amax));
      LAUNCH_CHECK();
    }
    const long th = (long)(N / 16) * (K / 32) * 64;
    if (planes == 2)
      hipLaunchKernelGGL(fe_image_kernel<2>, dim3((unsigned)cdiv(th, 256)), dim3(256), 0, st, src[l].w, (long)K, N, K,
                         src[l].gamma, src[l].rv, eps, (const float*)amax, f32(L.invs) + l, img + L.w[l]);
    else
      hipLaunchKernelGGL(fe_image_kernel<1>, dim3((unsigned)cdiv(th, 256)), dim3(256), 0, st, src[l].w, (long)K, N, K,
                         src[l].gamma, src[l].rv, eps, (const float*)amax, f32(L.invs) + l, img + L.w[l]);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}
size_t prh_encoder_fused_workspace_bytes(int B, int N, int planes) {
  if (B <= 0 || N <= 0 || (planes != 1 && planes != 2)) return 0;
  const int mt = planes == 1 ? 64 : 32;
  return (size_t)B * cdiv(N, mt) * 2048 * sizeof(float) + 256;
}
int prh_encoder_fused_forward(const void* image, int planes, int in_channel, int has_proj, const float* ctx, int B,
                              int N, float* memory, float* fused, float* gfeat, unsigned* saturated, void* workspace,
                              size_t workspace_bytes, int device, void* stream) {
  if (!image || !ctx || B <= 0 || N <= 0 || (planes != 1 && planes != 2) || in_channel < 4 || in_channel > 64)
    return fail(PRH_ERR_ARG, "encoder_fused_forward: bad argument");
  if (memory != nullptr && !has_proj) return fail(PRH_ERR_ARG, "encoder_fused_forward: memory wanted but the image has no context_proj");
  if (!memory && !fused && !gfeat) return fail(PRH_ERR_ARG, "encoder_fused_forward: no output requested");
  if ((long)B * N > 2000000000L) return fail(PRH_ERR_ARG, "encoder_fused_forward: B*N too large");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  FusedParams p; memset(&p, 0, sizeof(p));
  p.L = fused_layout(planes, in_channel);
  p.ctx = ctx; p.img = (const char*)image; p.B = B; p.N = N;
  const int mt = planes == 1 ? 64 : 32;
  p.tiles_per_seg = cdiv(N, mt);
  p.memory = memory; p.fused = fused; p.sat = saturated;
  if (gfeat != nullptr) {
    Arena a(workspace, workspace_bytes);
    p.pool_ws = a.f((size_t)B * p.tiles_per_seg * 2048);
    if (!a.ok) return fail(PRH_ERR_WORKSPACE, "encoder_fused_forward: workspace too small (%zu bytes)", workspace_bytes);
  }
  const unsigned grid = (unsigned)((long)B * p.tiles_per_seg);
  {
    const double P = (double)B * N;
    ProfScope ps(planes == 1 ? "encoder_fused<1>" : "encoder_fused<2>", 2.0 * P * (2793792.0 + (memory ? 262144.0 : 0.0)),
                 P * (4.0 * in_channel + (memory ? 1024.0 : 0.0) + (fused ? 4096.0 : 0.0)), st);
    if (planes == 1) {
      static const int attr = allow_big_lds(encoder_fused_kernel<1>);
      if (attr != PRH_OK) return attr;
      hipLaunchKernelGGL(encoder_fused_kernel<1>, dim3(grid), dim3(512), FE_LDS, st, p);
    } else {
      static const int attr = allow_big_lds(encoder_fused_kernel<2>);
      if (attr != PRH_OK) return attr;
      hipLaunchKernelGGL(encoder_fused_kernel<2>, dim3(grid), dim3(512), FE_LDS, st, p);
    }
    LAUNCH_CHECK();
  }
  if (gfeat != nullptr) {
    hipLaunchKernelGGL(fe_pool_final_kernel, dim3(4, B), dim3(256), 0, st, (const float*)p.pool_ws, p.tiles_per_seg, N, gfeat);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}

// ------------------------------------------------------------------ residual + dropout + LayerNorm (row f1)
static int ln_check(long rows, int channels, float p) {
  if (rows < 0 || channels != LN_C) return fail(PRH_ERR_ARG, "add_dropout_layernorm: channels must be %d", LN_C);
  if (p < 0.f || p >= 1.f) return fail(PRH_ERR_ARG, "add_dropout_layernorm: dropout_p must be in [0,1)");
  return PRH_OK;
}
int prh_add_dropout_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta,
                                      long rows, int channels, float eps, float dropout_p, unsigned seed,
                                      float* y, float* mean, float* rstd, int device, void* stream) {
  if (!x || !r || !gamma || !beta || !y) return fail(PRH_ERR_ARG, "add_dropout_layernorm_forward: null pointer");
  TRY(ln_check(rows, channels, dropout_p));
  if (rows == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  const unsigned thresh = dropout_p > 0.f ? (unsigned)((double)dropout_p * 4294967296.0) : 0u;
  hipLaunchKernelGGL(add_dropout_ln_fwd_kernel, dim3((unsigned)cdiv(rows, 4L)), dim3(256), 0, (hipStream_t)stream, x, r,
                     gamma, beta, rows, eps, seed, (const unsigned*)g_seed_src, thresh, 1.f / (1.f - dropout_p), y, mean,
                     rstd);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_add_dropout_layernorm_workspace_bytes(void) { return (size_t)2 * LN_BWD_BLOCKS * LN_C * sizeof(float) + 256; }
int prh_add_dropout_layernorm_backward(const float* dy, const float* x, const float* r, const float* gamma,
                                       const float* mean, const float* rstd, long rows, int channels,
                                       float dropout_p, unsigned seed, float* dx, float* dr, float* dgamma,
                                       float* dbeta, void* workspace, size_t workspace_bytes, int device,
                                       void* stream) {
  if (!dy || !x || !r || !gamma || !mean || !rstd || !dx || !dr || !dgamma || !dbeta)
    return fail(PRH_ERR_ARG, "add_dropout_layernorm_backward: null pointer");
  TRY(ln_check(rows, channels, dropout_p));
  Arena a(workspace, workspace_bytes);
  float* pg = a.f((size_t)LN_BWD_BLOCKS * LN_C);
  float* pb = a.f((size_t)LN_BWD_BLOCKS * LN_C);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "add_dropout_layernorm_backward: workspace too small");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  long nb = cdiv(rows, 4L * 8);
  nb = nb < 1 ? 1 : (nb > LN_BWD_BLOCKS ? LN_BWD_BLOCKS : nb);
  const unsigned thresh = dropout_p > 0.f ? (unsigned)((double)dropout_p * 4294967296.0) : 0u;
  hipLaunchKernelGGL(add_dropout_ln_bwd_kernel, dim3((unsigned)nb), dim3(256), 0, st, dy, x, r, gamma, mean, rstd, rows,
                     seed, (const unsigned*)g_seed_src, thresh, 1.f / (1.f - dropout_p), dx, dr, pg, pb);
  LAUNCH_CHECK();
  return reduce_ln_param_grad(pg, pb, (int)nb, dgamma, dbeta, st);
}

// ------------------------------------------------------------------ loss + optimiser (row f3)
constexpr int L1_BLOCKS = 1024;
size_t prh_l1_loss_workspace_bytes(void) { return (size_t)3 * L1_BLOCKS * sizeof(float) + 256; }
int prh_l1_loss(const float* pred, const float* target, int n_layers, long elems, double denom,
                int accumulate, float* loss, float* d_pred, float* geometry, double points,
                void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!pred || !target || !loss || n_layers <= 0 || elems <= 0 || !(denom > 0.0))
    return fail(PRH_ERR_ARG, "l1_loss: bad argument");
  if (geometry != nullptr && (elems % 3 != 0 || !(points > 0.0)))
    return fail(PRH_ERR_ARG, "l1_loss: geometry metrics need xyz triples and a point count");
  Arena a(workspace, workspace_bytes);
  float* part = a.f(3 * L1_BLOCKS);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "l1_loss: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  long blocks = cdiv(elems, 256L);
  blocks = blocks > L1_BLOCKS ? L1_BLOCKS : blocks;
  const float inv = (float)(1.0 / denom);
  hipLaunchKernelGGL(geometry != nullptr ? l1_deep_kernel<true> : l1_deep_kernel<false>, dim3((unsigned)blocks),
                     dim3(256), 0, st, pred, target, n_layers, elems, inv, d_pred, part);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, st, (const float*)part, (int)blocks, inv, accumulate, loss);
  LAUNCH_CHECK();
  if (geometry != nullptr) {
    const float ip = (float)(1.0 / points);
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, st, (const float*)(part + blocks), (int)blocks, ip,
                       accumulate, geometry);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(256), 0, st, (const float*)(part + 2 * blocks), (int)blocks,
                       ip, accumulate, geometry + 1);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}
int prh_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, int device,
                  void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1)
    return fail(PRH_ERR_ARG, "adam_step: bad argument (step counts from 1)");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
    return fail(PRH_ERR_ARG, "adam_step: buffers must be 16-byte aligned");
  if (n == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)cdiv(cdiv(n, 4L), 256L)), dim3(256), 0, (hipStream_t)stream, param,
                     grad, exp_avg, exp_avg_sq, n, (float)(lr / bc1), beta1, beta2, eps, weight_decay,
                     (float)(1.0 / sqrt(bc2)));
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ context builder (row f2)
struct CtxWS { int* blkcnt; int* blkoff; int* cand; unsigned* keys; float* box; };
// 256-point blocks of the crop passes: at least one, so that an empty cloud still has a count per line
int ctx_nblk(int npts) { return cdiv(npts, 256) < 1 ? 1 : cdiv(npts, 256); }
void ctx_carve(Arena& a, CtxWS& w, int npts, int L, int max_cand) {
  const size_t nblk = (size_t)ctx_nblk(npts);
  w.blkcnt = (int*)a.f(nblk * L);
  w.blkoff = (int*)a.f(nblk * L);
  w.cand = (int*)a.f((size_t)L * max_cand);
  w.keys = (unsigned*)a.f((size_t)L * max_cand);
  w.box = a.f((size_t)L * 6);
}
size_t prh_context_workspace_bytes(int npts, int n_lines, int max_candidates) {
  if (npts < 0 || n_lines <= 0 || max_candidates <= 0) return 0;
  Arena a; CtxWS w;
  ctx_carve(a, w, npts, n_lines, max_candidates);
  return a.off + 256;
}
int prh_context_build(const float* cloud, int npts, const float* dense, int n_dense, const float* line,
                      int m, int n_lines, float radius, float decay_scale, int n_samples,
                      int max_candidates, unsigned long long seed, float* out, int32_t* counts,
                      float* dbg_weights, void* workspace, size_t workspace_bytes, int device,
                      void* stream) {
  if (!dense || !line || !out || !counts || (npts > 0 && !cloud) || npts < 0 || n_lines <= 0 || n_samples <= 0)
    return fail(PRH_ERR_ARG, "context_build: bad argument");
  if (n_dense < 1 || n_dense > CTX_MAX_DENSE || m < 1 || m > CTX_MAX_LINE)
    return fail(PRH_ERR_ARG, "context_build: n_dense must be 1..%d and m 1..%d", CTX_MAX_DENSE, CTX_MAX_LINE);
  if (n_lines > 65535) return fail(PRH_ERR_ARG, "context_build: at most 65535 lines per call");
  if (max_candidates < n_samples + 1)
    return fail(PRH_ERR_ARG, "context_build: max_candidates must exceed n_samples");
  if (!(decay_scale > 0.f) || !(radius >= 0.f)) return fail(PRH_ERR_ARG, "context_build: radius/decay_scale");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  Arena a(workspace, workspace_bytes);
  CtxWS w;
  ctx_carve(a, w, npts, n_lines, max_candidates);
  if (!a.ok) return fail(PRH_ERR_WORKSPACE, "context_build: workspace too small (%zu bytes)", workspace_bytes);
  const int nblk = ctx_nblk(npts);
  const float r2 = radius * radius;
  hipLaunchKernelGGL(ctx_bbox_kernel, dim3(n_lines), dim3(64), 0, st, dense, n_dense, radius, w.box);
  LAUNCH_CHECK();
  hipLaunchKernelGGL((ctx_crop_kernel<false>), dim3(nblk, n_lines), dim3(256), 0, st, cloud, npts, dense, n_dense,
                     (const float*)w.box, r2, nblk, w.blkcnt, (const int*)nullptr, (int*)nullptr, max_candidates);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(ctx_scan_kernel, dim3(n_lines), dim3(256), 0, st, w.blkcnt, nblk, w.blkoff, counts);
  LAUNCH_CHECK();
  hipLaunchKernelGGL((ctx_crop_kernel<true>), dim3(nblk, n_lines), dim3(256), 0, st, cloud, npts, dense, n_dense,
                     (const float*)w.box, r2, nblk, w.blkcnt, (const int*)w.blkoff, w.cand, max_candidates);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(ctx_select_kernel, dim3(n_lines), dim3(256), 0, st, cloud, line, m, (const int*)counts,
                     (const int*)w.cand, max_candidates, decay_scale, n_samples, (uint64_t)seed, w.keys, out,
                     dbg_weights);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ragged builder: every line cropped from its own slice of one point buffer, candidates in CSR
struct CtxRaggedWS {
  int* line_base; int* line_npts; int* line_local; uint64_t* line_seed; long long* blk_offsets;
  float* box; int* blkcnt; int* blkoff;
};
void ctx_ragged_carve(Arena& a, CtxRaggedWS& w, int L, long long n_items) {
  w.line_base = (int*)a.f((size_t)L);
  w.line_npts = (int*)a.f((size_t)L);
  w.line_local = (int*)a.f((size_t)L);
  w.line_seed = (uint64_t*)a.f(2 * (size_t)L);
  w.blk_offsets = (long long*)a.f(2 * ((size_t)L + 1));
  w.box = a.f((size_t)L * 6);
  w.blkcnt = (int*)a.f((size_t)n_items);
  w.blkoff = (int*)a.f((size_t)n_items);
}
// Host arrays checked; blk_offsets (n_lines + 1) = exclusive scan of the 256-point blocks of each
// line's slice.  Returns PRH_OK or the error of the first rule broken.
static int ctx_ragged_plan(const char* what, const long long* slice_offsets, int n_slices, const int* line_slice,
                           int n_lines, std::vector<long long>& blk_offsets) {
  if (!slice_offsets || !line_slice || n_slices <= 0 || n_lines <= 0)
    return fail(PRH_ERR_ARG, "%s: bad argument (slice_offsets, line_slice, at least one slice and one line)", what);
  if (slice_offsets[0] != 0) return fail(PRH_ERR_ARG, "%s: slice_offsets must start at 0", what);
  for (int s = 0; s < n_slices; ++s)
    if (slice_offsets[s + 1] < slice_offsets[s])
      return fail(PRH_ERR_ARG, "%s: slice_offsets must not decrease (slice %d)", what, s);
  if (slice_offsets[n_slices] >= (1ll << 31)) return fail(PRH_ERR_ARG, "%s: at most 2^31 - 1 points per call", what);
  blk_offsets.assign((size_t)n_lines + 1, 0);
  for (int l = 0; l < n_lines; ++l) {
    const int s = line_slice[l];
    if (s < 0 || s >= n_slices) return fail(PRH_ERR_ARG, "%s: line %d names slice %d of %d", what, l, s, n_slices);
    if (l > 0 && s < line_slice[l - 1])
      return fail(PRH_ERR_ARG, "%s: line_slice must not decrease (line %d): lines are grouped by slice", what, l);
    blk_offsets[l + 1] = blk_offsets[l] + (slice_offsets[s + 1] - slice_offsets[s] + 255) / 256;
  }
  if (blk_offsets[n_lines] > 0x7fffffffll)
    return fail(PRH_ERR_ARG, "%s: %lld (line, block) work items do not fit one grid", what, blk_offsets[n_lines]);
  return PRH_OK;
}
size_t prh_context_ragged_workspace_bytes(int n_lines, long long n_items) {
  if (n_lines <= 0 || n_items < 0 || n_items > 0x7fffffffll) return 0;
  Arena a; CtxRaggedWS w;
  ctx_ragged_carve(a, w, n_lines, n_items);
  return a.off + 256;
}
static int ctx_ragged_shapes(const char* what, int n_dense, int m, float radius) {
  if (n_dense < 1 || n_dense > CTX_MAX_DENSE || m < 1 || m > CTX_MAX_LINE)
    return fail(PRH_ERR_ARG, "%s: n_dense must be 1..%d and m 1..%d", what, CTX_MAX_DENSE, CTX_MAX_LINE);
  if (!(radius >= 0.f)) return fail(PRH_ERR_ARG, "%s: radius", what);
  return PRH_OK;
}
int prh_context_ragged_count(const float* points, const long long* slice_offsets, int n_slices, const float* dense,
                             int n_dense, const int* line_slice, const unsigned long long* slice_seed, int n_lines,
                             float radius, int32_t* counts, long long* cand_offsets, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  const char* what = "context_ragged_count";
  std::vector<long long> blk;
  TRY(ctx_ragged_plan(what, slice_offsets, n_slices, line_slice, n_lines, blk));
  TRY(ctx_ragged_shapes(what, n_dense, 1, radius));
  if (!dense || !slice_seed || !counts || !cand_offsets || (slice_offsets[n_slices] > 0 && !points))
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  const long long n_items = blk[n_lines];
  Arena a(workspace, workspace_bytes);
  CtxRaggedWS w;
  ctx_ragged_carve(a, w, n_lines, n_items);
  if (!workspace || !a.ok) return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  // per-line tables: first row and rows of the line's slice, the line's position among its slice's
  // lines and its slice's seed - the indices and the seed a per-slice call would hash
  const size_t L = (size_t)n_lines;
  std::vector<int> base(L), npts(L), local(L);
  std::vector<uint64_t> seed(L);
  for (size_t l = 0; l < L; ++l) {
    const int s = line_slice[l];
    base[l] = (int)slice_offsets[s];
    npts[l] = (int)(slice_offsets[s + 1] - slice_offsets[s]);
    local[l] = l > 0 && line_slice[l - 1] == s ? local[l - 1] + 1 : 0;
    seed[l] = (uint64_t)slice_seed[s];
  }
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(w.line_base, base.data(), L * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.line_npts, npts.data(), L * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.line_local, local.data(), L * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.line_seed, seed.data(), L * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.blk_offsets, blk.data(), (L + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));               // the host tables above go out of scope on return
  hipLaunchKernelGGL(ctx_bbox_kernel, dim3(n_lines), dim3(64), 0, st, dense, n_dense, radius, w.box);
  LAUNCH_CHECK();
  if (n_items > 0) {
    hipLaunchKernelGGL((ctx_ragged_crop_kernel<false>), dim3((unsigned)n_items), dim3(256), 0, st, points,
                       (const int*)w.line_base, (const int*)w.line_npts, (const long long*)w.blk_offsets, 0, n_lines,
                       dense, n_dense, (const float*)w.box, radius * radius, w.blkcnt, (const int*)nullptr,
                       (const long long*)nullptr, (int*)nullptr, 0ll);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ctx_ragged_scan_kernel, dim3(n_lines), dim3(256), 0, st, (const int*)w.blkcnt,
                     (const long long*)w.blk_offsets, w.blkoff, counts);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(ctx_ragged_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)counts, n_lines, cand_offsets);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_context_ragged_select(const float* points, const long long* slice_offsets, int n_slices, const float* dense,
                              int n_dense, const float* line, int m, const int* line_slice, int n_lines, float radius,
                              float decay_scale, int n_samples, const int32_t* counts, const long long* cand_offsets,
                              int line0, int line1, int* cand, unsigned* keys, long long cand_capacity, float* out,
                              void* workspace, size_t workspace_bytes, int device, void* stream) {
  const char* what = "context_ragged_select";
  std::vector<long long> blk;
  TRY(ctx_ragged_plan(what, slice_offsets, n_slices, line_slice, n_lines, blk));
  TRY(ctx_ragged_shapes(what, n_dense, m, radius));
  if (!dense || !line || !counts || !cand_offsets || !out || (slice_offsets[n_slices] > 0 && !points))
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if (n_samples <= 0 || !(decay_scale > 0.f)) return fail(PRH_ERR_ARG, "%s: n_samples/decay_scale", what);
  if (line0 < 0 || line1 <= line0 || line1 > n_lines)
    return fail(PRH_ERR_ARG, "%s: lines %d..%d of %d", what, line0, line1, n_lines);
  if (cand_capacity < 0 || (cand_capacity > 0 && (!cand || !keys)))
    return fail(PRH_ERR_ARG, "%s: candidate buffers", what);
  Arena a(workspace, workspace_bytes);
  CtxRaggedWS w;
  ctx_ragged_carve(a, w, n_lines, blk[n_lines]);
  if (!workspace || !a.ok) return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const long long run_items = blk[line1] - blk[line0];
  if (run_items > 0 && cand_capacity > 0) {
    hipLaunchKernelGGL((ctx_ragged_crop_kernel<true>), dim3((unsigned)run_items), dim3(256), 0, st, points,
                       (const int*)w.line_base, (const int*)w.line_npts, (const long long*)w.blk_offsets, line0,
                       line1 - line0, dense, n_dense, (const float*)w.box, radius * radius, w.blkcnt,
                       (const int*)w.blkoff, cand_offsets, cand, cand_capacity);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ctx_ragged_select_kernel, dim3(line1 - line0), dim3(256), 0, st, points, (const int*)w.line_base,
                     (const int*)w.line_local, (const uint64_t*)w.line_seed, line, m, counts, cand_offsets, line0,
                     (const int*)cand, decay_scale, n_samples, keys, cand_capacity, out);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ scene evaluation metrics
int prh_line_metrics(const double* noisy, const double* refined, int n_lines, int m, const double* gt,
                     const long long* gt_offsets, int n_gt, const int* gt_index, int* info, double* resampled,
                     double* metrics, int device, void* stream) {
  if (n_lines < 0 || n_gt < 0 || (n_lines > 0 && (!noisy || !refined || !gt_index || !info || !resampled || !metrics)) ||
      (n_gt > 0 && (!gt || !gt_offsets)))
    return fail(PRH_ERR_ARG, "line_metrics: bad argument");
  if (m < 2 || m > MET_MAX_M) return fail(PRH_ERR_ARG, "line_metrics: m must be 2..%d", MET_MAX_M);
  if (n_lines == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(met_line_kernel, dim3(n_lines), dim3(64), 0, st, noisy, refined, m, gt, gt_offsets, n_gt,
                     gt_index, info, resampled, metrics);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_shift_sweep_workspace_bytes(int n_pred, int n_gt, int n_shifts) {
  (void)n_gt;
  if (n_pred <= 0 || n_shifts <= 0) return 0;
  return (size_t)cdiv(n_pred, SW_THREADS) * (size_t)n_shifts * sizeof(double) + 256;
}
int prh_shift_sweep(const double* pred, int n_pred, const double* gt, int n_gt, const double* shifts, int n_shifts,
                    double* out, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!pred || !gt || !shifts || !out || n_pred <= 0 || n_gt <= 0 || n_shifts <= 0)
    return fail(PRH_ERR_ARG, "shift_sweep: bad argument (needs at least one point, one GT point and one shift)");
  if (cdiv(n_shifts, SW_SB) > 65535) return fail(PRH_ERR_ARG, "shift_sweep: at most %d shifts per call", 65535 * SW_SB);
  if (workspace == nullptr || workspace_bytes < prh_shift_sweep_workspace_bytes(n_pred, n_gt, n_shifts))
    return fail(PRH_ERR_WORKSPACE, "shift_sweep: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int n_qt = cdiv(n_pred, SW_THREADS);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(met_sweep_kernel, dim3(n_qt, cdiv(n_shifts, SW_SB)), dim3(SW_THREADS), 0, st, pred, n_pred, gt,
                     n_gt, shifts, n_shifts, partial, n_qt);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(met_sweep_reduce_kernel, dim3(cdiv(n_shifts, 256)), dim3(256), 0, st, (const double*)partial,
                     n_qt, n_shifts, n_pred, out);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ragged sweep: host plan shared by the workspace query and the entry point.  Checks every offset
// array and builds the per-problem table, the work-item scan and the partial-sum CSR.
struct SweepRaggedWS { MetSweepProblem* prob; long long* item_offsets; long long* shift_offsets; double* partial; };
static void sweep_ragged_carve(Arena& a, SweepRaggedWS& w, int n, long long n_partial) {
  w.prob = (MetSweepProblem*)a.f((size_t)n * sizeof(MetSweepProblem) / sizeof(float));
  w.item_offsets = (long long*)a.f(2 * ((size_t)n + 1));
  w.shift_offsets = (long long*)a.f(2 * ((size_t)n + 1));
  w.partial = (double*)a.f(2 * (size_t)n_partial);
}
static int sweep_ragged_plan(const char* what, const long long* pred_offsets, const long long* gt_offsets,
                             int n_gt_sets, const int* gt_index, const long long* shift_offsets, int n,
                             std::vector<MetSweepProblem>* prob, std::vector<long long>* items, long long* n_partial) {
  if (!pred_offsets || !shift_offsets || n <= 0 || (gt_offsets == nullptr) != (gt_index == nullptr) ||
      (gt_offsets && n_gt_sets <= 0))
    return fail(PRH_ERR_ARG, "%s: bad argument (offset arrays and at least one problem)", what);
  if (pred_offsets[0] != 0 || shift_offsets[0] != 0 || (gt_offsets && gt_offsets[0] != 0))
    return fail(PRH_ERR_ARG, "%s: offsets must start at 0", what);
  if (gt_offsets)
    for (int g = 0; g < n_gt_sets; ++g)
      if (gt_offsets[g + 1] < gt_offsets[g]) return fail(PRH_ERR_ARG, "%s: gt_offsets must not decrease (set %d)", what, g);
  if (prob) prob->resize((size_t)n);
  if (items) items->assign((size_t)n + 1, 0);
  long long n_items = 0, part = 0;
  for (int p = 0; p < n; ++p) {
    const long long P = pred_offsets[p + 1] - pred_offsets[p], S = shift_offsets[p + 1] - shift_offsets[p];
    long long G = 1, g0 = 0;
    if (gt_offsets) {
      const int g = gt_index[p];
      if (g < 0 || g >= n_gt_sets) return fail(PRH_ERR_ARG, "%s: problem %d names GT set %d of %d", what, p, g, n_gt_sets);
      G = gt_offsets[g + 1] - gt_offsets[g];
      g0 = gt_offsets[g];
    }
    if (P <= 0 || G <= 0 || S <= 0)
      return fail(PRH_ERR_ARG, "%s: problem %d needs at least one point, one GT point and one shift", what, p);
    if (P > 0x7fffffffll || G > 0x7fffffffll || S > 0x7fffffffll)
      return fail(PRH_ERR_ARG, "%s: problem %d: at most 2^31 - 1 points, GT points and shifts per problem", what, p);
    const long long n_qt = (P + SW_THREADS - 1) / SW_THREADS, n_st = (S + SW_SB - 1) / SW_SB;
    if (prob) (*prob)[(size_t)p] = MetSweepProblem{pred_offsets[p], g0, shift_offsets[p], part, (int)P, (int)G, (int)S, (int)n_qt};
    n_items += n_qt * n_st;                              // < 2^23 * 2^27: no overflow before the check
    if (n_items > 0x7fffffffll)
      return fail(PRH_ERR_ARG, "%s: more than 2^31 - 1 (problem, query tile, shift tile) work items", what);
    if (items) (*items)[(size_t)p + 1] = n_items;
    part += n_qt * S;
  }
  *n_partial = part;
  return PRH_OK;
}
size_t prh_shift_sweep_ragged_workspace_bytes(const long long* pred_offsets, const long long* shift_offsets,
                                              int n_problems) {
  long long n_partial = 0;
  if (sweep_ragged_plan("shift_sweep_ragged", pred_offsets, nullptr, 0, nullptr, shift_offsets, n_problems, nullptr,
                        nullptr, &n_partial) != PRH_OK)
    return 0;
  Arena a; SweepRaggedWS w;
  sweep_ragged_carve(a, w, n_problems, n_partial);
  return a.off + 256;
}
int prh_shift_sweep_ragged(const double* pred, const long long* pred_offsets, const double* gt,
                           const long long* gt_offsets, int n_gt_sets, const int* gt_index, const double* shifts,
                           const long long* shift_offsets, int n_problems, double* out, void* workspace,
                           size_t workspace_bytes, int device, void* stream) {
  const char* what = "shift_sweep_ragged";
  if (!pred || !gt || !shifts || !out || !gt_offsets || !gt_index) return fail(PRH_ERR_ARG, "%s: null pointer", what);
  std::vector<MetSweepProblem> prob;
  std::vector<long long> items;
  long long n_partial = 0;
  TRY(sweep_ragged_plan(what, pred_offsets, gt_offsets, n_gt_sets, gt_index, shift_offsets, n_problems, &prob, &items,
                        &n_partial));
  Arena a(workspace, workspace_bytes);
  SweepRaggedWS w;
  sweep_ragged_carve(a, w, n_problems, n_partial);
  if (!workspace || !a.ok) return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  const size_t n = (size_t)n_problems;
  const long long n_items = items[n], total_shifts = shift_offsets[n];
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(w.prob, prob.data(), n * sizeof(MetSweepProblem), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.item_offsets, items.data(), (n + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w.shift_offsets, shift_offsets, (n + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));                 // the host tables above go out of scope on return
  hipLaunchKernelGGL(met_sweep_ragged_kernel, dim3((unsigned)n_items), dim3(SW_THREADS), 0, st, pred, gt, shifts,
                     (const MetSweepProblem*)w.prob, (const long long*)w.item_offsets, n_problems, w.partial);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(met_sweep_ragged_reduce_kernel, dim3((unsigned)((total_shifts + 255) / 256)), dim3(256), 0, st,
                     (const double*)w.partial, (const MetSweepProblem*)w.prob, (const long long*)w.shift_offsets,
                     n_problems, total_shifts, out);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ drive slicing
struct DrvWS { DrvPose* pose; int* cnt; long long* tile; };
void drv_carve(Arena& a, DrvWS& w, int npts, int S) {
  const size_t n_units = (size_t)cdiv(npts, DRV_UNIT), n_tiles = (size_t)cdiv((long)n_units, DRV_TILE);
  w.pose = (DrvPose*)a.f((size_t)S * sizeof(DrvPose) / sizeof(float));
  w.cnt = (int*)a.f(n_units * S);
  w.tile = (long long*)a.f(n_tiles * S * 2);
}
size_t prh_drive_slice_workspace_bytes(int npts, int n_slices) {
  if (npts < 0 || n_slices < 0) return 0;
  Arena a; DrvWS w;
  drv_carve(a, w, npts, n_slices);
  return a.off + 256;
}
static int drv_slice(bool fill, const float* cloud, int npts, const double* poses, int S, double segment_len,
                     double radius, long long* offsets, double* points, long long* source_index,
                     long long capacity, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const char* what = fill ? "drive_slice_write" : "drive_slice_count";
  if (npts < 0 || S < 0 || !offsets || (npts > 0 && !cloud) || (S > 0 && !poses) || !(segment_len >= 0.0) ||
      !(radius >= 0.0))
    return fail(PRH_ERR_ARG, "%s: bad argument", what);
  if (fill && (capacity < 0 || (capacity > 0 && (!points || !source_index))))
    return fail(PRH_ERR_ARG, "%s: bad output buffer", what);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (S == 0 || npts == 0) {
    if (!fill) HIP_TRY(hipMemsetAsync(offsets, 0, (size_t)(S + 1) * sizeof(long long), st));
    return PRH_OK;
  }
  Arena a(workspace, workspace_bytes);
  DrvWS w;
  drv_carve(a, w, npts, S);
  if (!workspace || !a.ok) return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  const long n_units = cdiv(npts, DRV_UNIT), n_tiles = cdiv(n_units, DRV_TILE);
  const float r2 = (float)(radius * radius);
  const double half = segment_len / 2;
  const int nblk = cdiv(n_units, 4);
  if (!fill) {
    hipLaunchKernelGGL(drv_pose_kernel, dim3(cdiv(S, 256)), dim3(256), 0, st, poses, S, w.pose);
    LAUNCH_CHECK();
    hipLaunchKernelGGL((drv_slice_kernel<false>), dim3(nblk), dim3(256), 0, st, (const float4*)cloud, npts,
                       (const DrvPose*)w.pose, S, r2, half, w.cnt, (const long long*)nullptr,
                       (const long long*)nullptr, (double*)nullptr, (long long*)nullptr, 0ll);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(drv_tile_scan_kernel, dim3((unsigned)n_tiles, cdiv(S, 256)), dim3(256), 0, st, w.cnt,
                       (long long)n_units, S, w.tile);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(drv_tile_base_kernel, dim3(1), dim3(256), 0, st, w.tile, (long long)n_tiles, S, offsets);
    LAUNCH_CHECK();
    return PRH_OK;
  }
  if (capacity == 0) return PRH_OK;
  hipLaunchKernelGGL((drv_slice_kernel<true>), dim3(nblk), dim3(256), 0, st, (const float4*)cloud, npts,
                     (const DrvPose*)w.pose, S, r2, half, w.cnt, (const long long*)w.tile,
                     (const long long*)offsets, points, source_index, capacity);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_drive_slice_count(const float* cloud, int npts, const double* poses, int n_slices, double segment_len,
                          double radius, long long* offsets, void* workspace, size_t workspace_bytes, int device,
                          void* stream) {
  return drv_slice(false, cloud, npts, poses, n_slices, segment_len, radius, offsets, nullptr, nullptr, 0, workspace,
                   workspace_bytes, device, stream);
}
int prh_drive_slice_write(const float* cloud, int npts, const double* poses, int n_slices, double segment_len,
                          double radius, const long long* offsets, double* points, long long* source_index,
                          long long capacity, void* workspace, size_t workspace_bytes, int device, void* stream) {
  return drv_slice(true, cloud, npts, poses, n_slices, segment_len, radius, (long long*)offsets, points,
                   source_index, capacity, workspace, workspace_bytes, device, stream);
}
size_t prh_drive_clip_workspace_bytes(int n_slices) {
  if (n_slices < 0) return 0;
  return align_up((size_t)n_slices * sizeof(DrvPose), 256) + 256;
}
// The two-pass polyline clip of the slicer and of the prediction scenes: one thread per (pose, line),
// a count call and a write call over the same workspace.  kernel is the <WRITE> instantiation of the
// tool's own rule (drv_clip_kernel, mt_clip_kernel), what the entry point's name, unit its word for a pose.
using ClipKernel = void (*)(const double*, const long long*, int, const DrvPose*, int, double, int*,
                            const long long*, double*);
static int clip_lines(ClipKernel kernel, bool write, const char* what, const char* unit, const double* lines,
                      const long long* line_offsets, int n_lines, const double* poses, int S, double segment_len,
                      int* counts, const long long* out_offsets, double* out, void* workspace,
                      size_t workspace_bytes, int device, void* stream) {
  if (n_lines < 0 || S < 0 || !(segment_len >= 0.0)) return fail(PRH_ERR_ARG, "%s: bad argument", what);
  if (n_lines == 0 || S == 0) return PRH_OK;
  if (!lines || !line_offsets || !poses || (write ? (!out_offsets || !out) : !counts))
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if ((long long)S * n_lines > 256ll * 0x7fffffff)
    return fail(PRH_ERR_ARG, "%s: too many (%s, line) pairs", what, unit);
  if (!workspace || workspace_bytes < prh_drive_clip_workspace_bytes(S))
    return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  DrvPose* pose = (DrvPose*)workspace;
  hipLaunchKernelGGL(drv_pose_kernel, dim3(cdiv(S, 256)), dim3(256), 0, st, poses, S, pose);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(kernel, dim3(cdiv((long)S * n_lines, 256)), dim3(256), 0, st, lines, line_offsets, n_lines,
                     (const DrvPose*)pose, S, segment_len / 2, counts, out_offsets, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_drive_clip_count(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_slices, double segment_len, int* counts, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  return clip_lines(drv_clip_kernel<false>, false, "drive_clip_count", "slice", lines, line_offsets, n_lines, poses,
                    n_slices, segment_len, counts, nullptr, nullptr, workspace, workspace_bytes, device, stream);
}
int prh_drive_clip_write(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_slices, double segment_len, const long long* out_offsets, double* out,
                         void* workspace, size_t workspace_bytes, int device, void* stream) {
  return clip_lines(drv_clip_kernel<true>, true, "drive_clip_write", "slice", lines, line_offsets, n_lines, poses,
                    n_slices, segment_len, nullptr, out_offsets, out, workspace, workspace_bytes, device, stream);
}
size_t prh_drive_noise_workspace_bytes(int n_lines) {
  if (n_lines < 0) return 0;
  return align_up((size_t)n_lines * 3 * sizeof(double), 256) + 256;
}
int prh_drive_noise(const double* lines, const long long* line_offsets, const int* vertex_line, long long n_verts,
                    int n_lines, const int* line_ids, const double* scales, int n_scales, unsigned long long seed,
                    int draw, double* draws_u, double* draws_j, double* out, void* workspace,
                    size_t workspace_bytes, int device, void* stream) {
  if (n_lines < 0 || n_verts < 0 || n_scales < 1 || n_scales > DRV_MAX_SCALES || (draw && !scales))
    return fail(PRH_ERR_ARG, "drive_noise: bad argument (1..%d scales)", DRV_MAX_SCALES);
  if (n_lines == 0 || n_verts == 0) return PRH_OK;
  if (!lines || !line_offsets || !vertex_line || !draws_u || !draws_j || !out)
    return fail(PRH_ERR_ARG, "drive_noise: null pointer");
  if (n_verts * n_scales > 256ll * 0x7fffffff) return fail(PRH_ERR_ARG, "drive_noise: too many vertices");
  if (!workspace || workspace_bytes < prh_drive_noise_workspace_bytes(n_lines))
    return fail(PRH_ERR_WORKSPACE, "drive_noise: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  double* centroid = (double*)workspace;
  DrvScales sc;
  for (int k = 0; k < DRV_MAX_SCALES; ++k) sc.s[k] = (draw && k < n_scales) ? scales[k] : 0.0;
  hipLaunchKernelGGL(drv_centroid_kernel, dim3(cdiv(3l * n_lines, 256)), dim3(256), 0, st, lines, line_offsets,
                     n_lines, centroid);
  LAUNCH_CHECK();
  const int nblk = cdiv(n_verts * n_scales, 256);
  hipLaunchKernelGGL(draw ? drv_noise_kernel<true> : drv_noise_kernel<false>, dim3(nblk), dim3(256), 0, st, lines,
                     line_offsets, vertex_line, n_verts, n_lines, line_ids, sc, n_scales, (uint64_t)seed,
                     (const double*)centroid, draws_u, draws_j, out);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ PCD text codec
int prh_pcd_group_rows(void) { return PCD_GROUP; }
size_t prh_pcd_format_workspace_bytes(long long n_rows) {
  if (n_rows < 0) return 0;
  return align_up((size_t)((n_rows + PCD_GROUP - 1) / PCD_GROUP) * sizeof(long long), 256) + 256;
}
int prh_pcd_format_count(const void* points, int is_fp64, long long n_rows, unsigned char* row_bytes,
                         int* group_bytes, long long* status, void* workspace, size_t workspace_bytes, int device,
                         void* stream) {
  if (n_rows < 0 || !status || (n_rows > 0 && (!points || !row_bytes || !group_bytes)))
    return fail(PRH_ERR_ARG, "pcd_format_count: bad argument");
  const long long G = (n_rows + PCD_GROUP - 1) / PCD_GROUP;
  if (G > 4ll * 0x7fffffff) return fail(PRH_ERR_ARG, "pcd_format_count: too many rows");
  if (n_rows > 0 && (!workspace || workspace_bytes < prh_pcd_format_workspace_bytes(n_rows)))
    return fail(PRH_ERR_WORKSPACE, "pcd_format_count: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  long long* bad = (long long*)workspace;
  if (n_rows > 0) {
    const unsigned nblk = (unsigned)((G + 3) / 4);
    if (is_fp64)
      hipLaunchKernelGGL((pcd_format_kernel<double, false>), dim3(nblk), dim3(256), 0, st, (const double*)points,
                         n_rows, row_bytes, group_bytes, bad, (const long long*)nullptr, (unsigned char*)nullptr, 0ll);
    else
      hipLaunchKernelGGL((pcd_format_kernel<float, false>), dim3(nblk), dim3(256), 0, st, (const float*)points,
                         n_rows, row_bytes, group_bytes, bad, (const long long*)nullptr, (unsigned char*)nullptr, 0ll);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pcd_first_kernel, dim3(1), dim3(256), 0, st, (const long long*)bad, G, status);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_pcd_format_write(const void* points, int is_fp64, long long n_rows, const unsigned char* row_bytes,
                         const long long* group_offsets, const long long* offsets, int n_slices,
                         unsigned char* text, long long capacity, long long* byte_offsets, int device,
                         void* stream) {
  if (n_rows < 0 || n_slices < 0 || capacity < 0 || !byte_offsets ||
      (n_rows > 0 && (!points || !row_bytes || !group_offsets)) || (capacity > 0 && !text))
    return fail(PRH_ERR_ARG, "pcd_format_write: bad argument");
  const long long G = (n_rows + PCD_GROUP - 1) / PCD_GROUP;
  if (G > 4ll * 0x7fffffff) return fail(PRH_ERR_ARG, "pcd_format_write: too many rows");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int S = offsets ? n_slices : 1;
  hipLaunchKernelGGL(pcd_slice_bytes_kernel, dim3(cdiv(S + 1, 256)), dim3(256), 0, st, offsets, S, n_rows, row_bytes,
                     group_offsets, byte_offsets);
  LAUNCH_CHECK();
  if (n_rows == 0 || capacity == 0) return PRH_OK;
  const unsigned nblk = (unsigned)((G + 3) / 4);
  if (is_fp64)
    hipLaunchKernelGGL((pcd_format_kernel<double, true>), dim3(nblk), dim3(256), 0, st, (const double*)points, n_rows,
                       (unsigned char*)nullptr, (int*)nullptr, (long long*)nullptr, group_offsets, text, capacity);
  else
    hipLaunchKernelGGL((pcd_format_kernel<float, true>), dim3(nblk), dim3(256), 0, st, (const float*)points, n_rows,
                       (unsigned char*)nullptr, (int*)nullptr, (long long*)nullptr, group_offsets, text, capacity);
  LAUNCH_CHECK();
  return PRH_OK;
}
long long prh_pcd_index_blocks(const void* payload, long long n_bytes) {
  if (n_bytes <= 0) return 0;
  return (((long long)((uintptr_t)payload & 15)) + n_bytes + PCD_BLOCK_BYTES - 1) / PCD_BLOCK_BYTES;
}
int prh_pcd_index_count(const unsigned char* payload, long long n_bytes, int* block_lines, int device,
                        void* stream) {
  if (n_bytes < 0 || (n_bytes > 0 && (!payload || !block_lines)))
    return fail(PRH_ERR_ARG, "pcd_index_count: bad argument");
  const long long nb = prh_pcd_index_blocks(payload, n_bytes);
  if (nb > 0x7fffffffll) return fail(PRH_ERR_ARG, "pcd_index_count: payload too large");
  if (nb == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL((pcd_lines_kernel<false>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, payload, n_bytes,
                     block_lines, (const long long*)nullptr, (long long*)nullptr, 0ll);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_pcd_index_write(const unsigned char* payload, long long n_bytes, const long long* block_offsets,
                        long long* row_start, long long n_rows, int device, void* stream) {
  if (n_bytes < 0 || n_rows < 0 || !row_start || (n_bytes > 0 && (!payload || !block_offsets)))
    return fail(PRH_ERR_ARG, "pcd_index_write: bad argument");
  const long long nb = prh_pcd_index_blocks(payload, n_bytes);
  if (nb > 0x7fffffffll) return fail(PRH_ERR_ARG, "pcd_index_write: payload too large");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  if (nb == 0) {
    HIP_TRY(hipMemsetAsync(row_start, 0, (size_t)(n_rows + 1) * sizeof(long long), st));
    return PRH_OK;
  }
  hipLaunchKernelGGL((pcd_lines_kernel<true>), dim3((unsigned)nb), dim3(256), 0, st, payload, n_bytes, (int*)nullptr,
                     block_offsets, row_start, n_rows);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_pcd_parse_workspace_bytes(long long n_rows) {
  if (n_rows < 0) return 0;
  return align_up((size_t)((n_rows + 255) / 256) * sizeof(long long), 256) + 256;
}
int prh_pcd_parse(const unsigned char* payload, long long n_bytes, const long long* row_start, long long n_rows,
                  int ncols, float* out, long long* status, void* workspace, size_t workspace_bytes, int device,
                  void* stream) {
  if (n_bytes < 0 || n_rows < 0 || ncols < 1 || !status || (n_rows > 0 && (!payload || !row_start || !out)))
    return fail(PRH_ERR_ARG, "pcd_parse: bad argument");
  const long long nb = (n_rows + 255) / 256;
  if (nb > 0x7fffffffll) return fail(PRH_ERR_ARG, "pcd_parse: too many rows");
  if (n_rows > 0 && (!workspace || workspace_bytes < prh_pcd_parse_workspace_bytes(n_rows)))
    return fail(PRH_ERR_WORKSPACE, "pcd_parse: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  long long* bad = (long long*)workspace;
  if (n_rows > 0) {
    hipLaunchKernelGGL(pcd_parse_kernel, dim3((unsigned)nb), dim3(256), 0, st, payload, row_start, n_rows, ncols, out,
                       bad);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pcd_first_kernel, dim3(1), dim3(256), 0, st, (const long long*)bad, nb, status);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_pcd_unpack14(const unsigned char* payload, long long n_points, float* out, int device, void* stream) {
  if (n_points < 0 || (n_points > 0 && (!payload || !out))) return fail(PRH_ERR_ARG, "pcd_unpack14: bad argument");
  const long long nb = (n_points + PCD_UNPACK_POINTS - 1) / PCD_UNPACK_POINTS;
  if (nb > 0x7fffffffll) return fail(PRH_ERR_ARG, "pcd_unpack14: too many points");
  if (nb == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(pcd_unpack14_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, payload, n_points,
                     (float4*)out);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ prediction scenes
size_t prh_match_clip_workspace_bytes(int n_frames) { return prh_drive_clip_workspace_bytes(n_frames); }
int prh_match_clip_count(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_frames, double segment_len, int* counts, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  return clip_lines(mt_clip_kernel<false>, false, "match_clip_count", "frame", lines, line_offsets, n_lines, poses,
                    n_frames, segment_len, counts, nullptr, nullptr, workspace, workspace_bytes, device, stream);
}
int prh_match_clip_write(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_frames, double segment_len, const long long* out_offsets, double* out,
                         void* workspace, size_t workspace_bytes, int device, void* stream) {
  return clip_lines(mt_clip_kernel<true>, true, "match_clip_write", "frame", lines, line_offsets, n_lines, poses,
                    n_frames, segment_len, nullptr, out_offsets, out, workspace, workspace_bytes, device, stream);
}
size_t prh_match_costs_workspace_bytes(long long n_pred_lines) {
  if (n_pred_lines < 0) return 0;
  return align_up((size_t)n_pred_lines * sizeof(int), 256) + 256;
}
int prh_match_costs(const double* pred_xy, const long long* pred_line_offsets, const long long* pred_frame_offsets,
                    long long n_pred_lines, const double* gt_xy, const long long* gt_line_offsets,
                    const long long* gt_frame_offsets, int n_frames, const long long* cost_offsets, double* costs,
                    void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (n_frames < 0 || n_pred_lines < 0) return fail(PRH_ERR_ARG, "match_costs: bad argument");
  if (n_frames == 0 || n_pred_lines == 0) return PRH_OK;
  if (n_pred_lines > 0x7fffffffll) return fail(PRH_ERR_ARG, "match_costs: at most 2^31 - 1 prediction lines per call");
  if (!pred_line_offsets || !pred_frame_offsets || !gt_line_offsets || !gt_frame_offsets || !cost_offsets)
    return fail(PRH_ERR_ARG, "match_costs: null pointer");
  if (!workspace || workspace_bytes < prh_match_costs_workspace_bytes(n_pred_lines))
    return fail(PRH_ERR_WORKSPACE, "match_costs: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* line_frame = (int*)workspace;
  hipLaunchKernelGGL(mt_line_frame_kernel, dim3(cdiv(n_frames, 256)), dim3(256), 0, st, pred_frame_offsets, n_frames,
                     line_frame);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(mt_cost_kernel, dim3((unsigned)n_pred_lines), dim3(MT_COST_THREADS), 0, st, pred_xy,
                     pred_line_offsets, pred_frame_offsets, (const int*)line_frame, gt_xy, gt_line_offsets,
                     gt_frame_offsets, cost_offsets, costs);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_match_max_side(void) { return MT_MAX_SIDE; }
int prh_match_assign(const double* costs, const long long* cost_offsets, const int* shapes, const long long* row_offsets,
                     const long long* col_offsets, int n_frames, long long max_cells, double threshold,
                     int use_threshold, int* match, double* total, int* status, double* row_dual, double* col_dual,
                     int device, void* stream) {
  if (n_frames < 0 || max_cells < 0 || max_cells > (long long)MT_MAX_SIDE * MT_MAX_SIDE)
    return fail(PRH_ERR_ARG, "match_assign: bad argument (at most %d lines per side per frame)", MT_MAX_SIDE);
  if (n_frames == 0) return PRH_OK;
  if (!cost_offsets || !shapes || !row_offsets || !col_offsets || !total || !status)
    return fail(PRH_ERR_ARG, "match_assign: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = mt_assign_lds(max_cells);
  if (lds > 64 * 1024) TRY_RC(allow_big_lds(mt_assign_kernel));
  hipLaunchKernelGGL(mt_assign_kernel, dim3(n_frames), dim3(64), lds, st, costs, cost_offsets, shapes, row_offsets,
                     col_offsets, max_cells, threshold, use_threshold, match, total, status, row_dual, col_dual);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ BEV rendering
size_t prh_bev_bounds_workspace_bytes(void) {
  return align_up((size_t)BEV_BOUNDS_BLOCKS * 4 * sizeof(double), 256) + align_up((size_t)BEV_BOUNDS_BLOCKS * sizeof(int), 256);
}
int prh_bev_bounds(const void* points, long long n, int is_double, double* info, void* workspace,
                   size_t workspace_bytes, int device, void* stream) {
  if (n <= 0 || !points || !info) return fail(PRH_ERR_ARG, "bev_bounds: bad argument");
  if (!workspace || workspace_bytes < prh_bev_bounds_workspace_bytes())
    return fail(PRH_ERR_WORKSPACE, "bev_bounds: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* bad = (int*)((char*)workspace + align_up((size_t)BEV_BOUNDS_BLOCKS * 4 * sizeof(double), 256));
  const long want = (n + BEV_THREADS - 1) / BEV_THREADS;
  const int nblk = (int)(want < BEV_BOUNDS_BLOCKS ? want : BEV_BOUNDS_BLOCKS);
  if (is_double) {
    hipLaunchKernelGGL(bev_bounds_kernel<double>, dim3(nblk), dim3(BEV_THREADS), 0, st, (const double*)points, n,
                       (double*)workspace, bad);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_bounds_final<double>, dim3(1), dim3(BEV_THREADS), 0, st, (const double*)workspace,
                       (const int*)bad, nblk, info);
  } else {
    hipLaunchKernelGGL(bev_bounds_kernel<float>, dim3(nblk), dim3(BEV_THREADS), 0, st, (const float*)points, n,
                       (float*)workspace, bad);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_bounds_final<float>, dim3(1), dim3(BEV_THREADS), 0, st, (const float*)workspace,
                       (const int*)bad, nblk, info);
  }
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_bev_raster(const void* points, const long long* offsets, int n_slices, long long n, int is_double,
                   double y_min, double x_max, double resolution, int height, int width, float* image, int* bad,
                   int device, void* stream) {
  if (n < 0 || n_slices < 0 || height < 0 || width < 0 || !bad) return fail(PRH_ERR_ARG, "bev_raster: bad argument");
  const long long cells = (long long)n_slices * height * width;
  if (cells >= 256ll * 0x7fffffff || n >= 256ll * 0x7fffffff) return fail(PRH_ERR_ARG, "bev_raster: too large");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
  if (cells == 0) return PRH_OK;
  if (!image || (n > 0 && !points)) return fail(PRH_ERR_ARG, "bev_raster: null pointer");
  HIP_TRY(hipMemsetAsync(image, 0, (size_t)cells * sizeof(float), st));
  if (n > 0) {
    const unsigned nblk = (unsigned)((n + BEV_THREADS - 1) / BEV_THREADS);
    if (is_double)
      hipLaunchKernelGGL(bev_raster_kernel<double>, dim3(nblk), dim3(BEV_THREADS), 0, st, (const double*)points,
                         offsets, n_slices, n, y_min, x_max, resolution, height, width, (unsigned*)image, bad);
    else
      hipLaunchKernelGGL(bev_raster_kernel<float>, dim3(nblk), dim3(BEV_THREADS), 0, st, (const float*)points, offsets,
                         n_slices, n, (float)y_min, (float)x_max, (float)resolution, height, width, (unsigned*)image,
                         bad);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(bev_finalize_kernel, dim3((unsigned)((cells + BEV_THREADS - 1) / BEV_THREADS)), dim3(BEV_THREADS),
                     0, st, (unsigned*)image, cells);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_bev_select_workspace_bytes(int n_slices) {
  if (n_slices < 0) return 0;
  return align_up((size_t)n_slices * sizeof(BevSel), 256) + align_up((size_t)n_slices * 512 * sizeof(unsigned), 256);
}
int prh_bev_select(const float* image, int n_slices, long long pixels, float quantile, double* out, void* workspace,
                   size_t workspace_bytes, int device, void* stream) {
  if (n_slices < 0 || pixels < 0 || !(quantile >= 0.f && quantile <= 1.f) || n_slices > 65535)
    return fail(PRH_ERR_ARG, "bev_select: bad argument");
  if (n_slices == 0) return PRH_OK;
  if (!out || (pixels > 0 && !image)) return fail(PRH_ERR_ARG, "bev_select: null pointer");
  if (!workspace || workspace_bytes < prh_bev_select_workspace_bytes(n_slices))
    return fail(PRH_ERR_WORKSPACE, "bev_select: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  BevSel* sel = (BevSel*)workspace;
  unsigned* hist = (unsigned*)((char*)workspace + align_up((size_t)n_slices * sizeof(BevSel), 256));
  HIP_TRY(hipMemsetAsync(workspace, 0, prh_bev_select_workspace_bytes(n_slices), st));
  HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_slices * 4 * sizeof(double), st));
  long want = (pixels + 4L * BEV_THREADS - 1) / (4L * BEV_THREADS);
  const int bx = (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(bev_hist_kernel, dim3(bx, n_slices), dim3(BEV_THREADS), 0, st, image, pixels, pass,
                       (const BevSel*)sel, hist);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(bev_pick_kernel, dim3(cdiv(2L * n_slices, 64)), dim3(64), 0, st, sel, hist, n_slices, pass,
                       quantile, out);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}
int prh_bev_tone(const float* image, int n_slices, long long pixels, const float* p, float gamma, float* out,
                 int device, void* stream) {
  if (n_slices < 0 || pixels < 0 || n_slices > 65535 || pixels >= 256ll * 0x7fffffff)
    return fail(PRH_ERR_ARG, "bev_tone: bad argument");
  if (n_slices == 0 || pixels == 0) return PRH_OK;
  if (!image || !p || !out) return fail(PRH_ERR_ARG, "bev_tone: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(bev_tone_kernel, dim3((unsigned)((pixels + BEV_THREADS - 1) / BEV_THREADS), n_slices),
                     dim3(BEV_THREADS), 0, (hipStream_t)stream, image, pixels, p, gamma, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_bev_colorize(const float* norm, const float* image, long long pixels, const unsigned* table, unsigned* out,
                     int device, void* stream) {
  if (pixels < 0 || pixels >= 256ll * 0x7fffffff) return fail(PRH_ERR_ARG, "bev_colorize: bad argument");
  if (pixels == 0) return PRH_OK;
  if (!norm || !image || !table || !out) return fail(PRH_ERR_ARG, "bev_colorize: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(bev_colorize_kernel, dim3((unsigned)((pixels + BEV_THREADS - 1) / BEV_THREADS)),
                     dim3(BEV_THREADS), 0, (hipStream_t)stream, norm, image, pixels, table, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_bev_crop(const unsigned* rgba, int height, int width, const int* views, const long long* pixel_offsets,
                 int n_views, long long total_pixels, unsigned* out, int device, void* stream) {
  if (height < 0 || width < 0 || n_views < 0 || total_pixels < 0 || total_pixels >= 256ll * 0x7fffffff)
    return fail(PRH_ERR_ARG, "bev_crop: bad argument");
  if (n_views == 0 || total_pixels == 0) return PRH_OK;
  if (!views || !pixel_offsets || !out || ((long long)height * width > 0 && !rgba))
    return fail(PRH_ERR_ARG, "bev_crop: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(bev_crop_kernel, dim3((unsigned)((total_pixels + BEV_THREADS - 1) / BEV_THREADS)),
                     dim3(BEV_THREADS), 0, (hipStream_t)stream, rgba, height, width, views, pixel_offsets, n_views,
                     total_pixels, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_bev_tile(void) { return BEV_TILE; }
int prh_bev_draw_count(const double* segments, const int* segment_line, int n_segments, const double* styles,
                       const int* line_view, const int* view_dims, const long long* tile_base, long long n_tiles,
                       int* tile_count, int device, void* stream) {
  if (n_segments < 0 || n_tiles < 0) return fail(PRH_ERR_ARG, "bev_draw_count: bad argument");
  if (n_tiles == 0) return PRH_OK;
  if (!tile_count) return fail(PRH_ERR_ARG, "bev_draw_count: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(tile_count, 0, (size_t)n_tiles * sizeof(int), st));
  if (n_segments == 0) return PRH_OK;
  if (!segments || !segment_line || !styles || !line_view || !view_dims || !tile_base)
    return fail(PRH_ERR_ARG, "bev_draw_count: null pointer");
  hipLaunchKernelGGL((bev_bin_kernel<false>), dim3(cdiv(n_segments, BEV_THREADS)), dim3(BEV_THREADS), 0, st, segments,
                     segment_line, n_segments, styles, line_view, view_dims, tile_base, tile_count,
                     (const long long*)nullptr, (int*)nullptr);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_bev_draw_workspace_bytes(long long n_tiles, long long n_items) {
  if (n_tiles < 0 || n_items < 0) return 0;
  return align_up((size_t)n_tiles * sizeof(int), 256) + 2 * align_up((size_t)n_items * sizeof(int), 256) + 256;
}
int prh_bev_draw(const double* segments, const int* segment_line, int n_segments, const double* styles,
                 const int* line_view, const int* view_dims, const long long* tile_base,
                 const long long* pixel_offsets, const int* tile_view, const long long* tile_offsets,
                 long long n_tiles, long long n_items, unsigned* canvas, void* workspace, size_t workspace_bytes,
                 int device, void* stream) {
  if (n_segments < 0 || n_tiles < 0 || n_items < 0 || n_tiles > 0x7fffffffll)
    return fail(PRH_ERR_ARG, "bev_draw: bad argument");
  if (n_segments == 0 || n_tiles == 0 || n_items == 0) return PRH_OK;
  if (!segments || !segment_line || !styles || !line_view || !view_dims || !tile_base || !pixel_offsets ||
      !tile_view || !tile_offsets || !canvas)
    return fail(PRH_ERR_ARG, "bev_draw: null pointer");
  if (!workspace || workspace_bytes < prh_bev_draw_workspace_bytes(n_tiles, n_items))
    return fail(PRH_ERR_WORKSPACE, "bev_draw: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* cursor = (int*)workspace;
  int* items = (int*)((char*)workspace + align_up((size_t)n_tiles * sizeof(int), 256));
  int* sorted = (int*)((char*)items + align_up((size_t)n_items * sizeof(int), 256));
  HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)n_tiles * sizeof(int), st));
  hipLaunchKernelGGL((bev_bin_kernel<true>), dim3(cdiv(n_segments, BEV_THREADS)), dim3(BEV_THREADS), 0, st, segments,
                     segment_line, n_segments, styles, line_view, view_dims, tile_base, cursor, tile_offsets, items);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(bev_draw_kernel, dim3((unsigned)n_tiles), dim3(BEV_THREADS), 0, st, segments, segment_line, styles,
                     view_dims, tile_base, pixel_offsets, tile_view, tile_offsets, (const int*)items, sorted, canvas);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ 3-D views
size_t prh_view_bounds_workspace_bytes(void) {
  return align_up((size_t)VIEW_BOUNDS_BLOCKS * 6 * sizeof(double), 256) + align_up((size_t)VIEW_BOUNDS_BLOCKS * sizeof(int), 256);
}
int prh_view_bounds(const void* points, long long n, int is_double, double* info, void* workspace,
                    size_t workspace_bytes, int device, void* stream) {
  if (n <= 0 || !points || !info) return fail(PRH_ERR_ARG, "view_bounds: bad argument");
  if (!workspace || workspace_bytes < prh_view_bounds_workspace_bytes())
    return fail(PRH_ERR_WORKSPACE, "view_bounds: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* bad = (int*)((char*)workspace + align_up((size_t)VIEW_BOUNDS_BLOCKS * 6 * sizeof(double), 256));
  const long long want = (n + VIEW_THREADS - 1) / VIEW_THREADS;
  const int nblk = (int)(want < VIEW_BOUNDS_BLOCKS ? want : VIEW_BOUNDS_BLOCKS);
  if (is_double) {
    hipLaunchKernelGGL(view_bounds_kernel<double>, dim3(nblk), dim3(VIEW_THREADS), 0, st, (const double*)points, n,
                       (double*)workspace, bad);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(view_bounds_final<double>, dim3(1), dim3(VIEW_THREADS), 0, st, (const double*)workspace,
                       (const int*)bad, nblk, info);
  } else {
    hipLaunchKernelGGL(view_bounds_kernel<float>, dim3(nblk), dim3(VIEW_THREADS), 0, st, (const float*)points, n,
                       (float*)workspace, bad);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(view_bounds_final<float>, dim3(1), dim3(VIEW_THREADS), 0, st, (const float*)workspace,
                       (const int*)bad, nblk, info);
  }
  LAUNCH_CHECK();
  return PRH_OK;
}
static bool view_image_ok(int n_views, int height, int width) {
  return n_views >= 0 && height >= 0 && width >= 0 && height < (1 << 24) && width < (1 << 24) &&
         (long long)n_views * height * width < 256ll * 0x7fffffff;
}
int prh_view_clear(unsigned long long* zbuf, int n_views, int height, int width, int device, void* stream) {
  if (!view_image_ok(n_views, height, width)) return fail(PRH_ERR_ARG, "view_clear: bad argument");
  const long long cells = (long long)n_views * height * width;
  if (cells == 0) return PRH_OK;
  if (!zbuf) return fail(PRH_ERR_ARG, "view_clear: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(view_clear_kernel, dim3((unsigned)((cells + VIEW_THREADS - 1) / VIEW_THREADS)), dim3(VIEW_THREADS),
                     0, (hipStream_t)stream, zbuf, cells);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_view_max_views(void) { return VIEW_MAX_VIEWS; }
int prh_view_splat(const void* points, long long n, int is_double, const double* cameras, int n_views,
                   const long long* offsets, int n_slices, const unsigned char* slice_mask, int size, double cmin,
                   double cmax, int height, int width, unsigned long long* zbuf, int* bad, int device, void* stream) {
  if (n < 0 || !view_image_ok(n_views, height, width) || n_views > VIEW_MAX_VIEWS || size < 1 || size > VIEW_MAX_SPLAT ||
      n_slices < 0 || !bad || n >= 256ll * 0x7fffffff)
    return fail(PRH_ERR_ARG, "view_splat: bad argument");
  if ((offsets != nullptr) != (slice_mask != nullptr) || (offsets && n_slices < 1))
    return fail(PRH_ERR_ARG, "view_splat: offsets and slice_mask go together");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), st));
  if (n == 0 || (long long)n_views * height * width == 0) return PRH_OK;
  if (!points || !cameras || !zbuf) return fail(PRH_ERR_ARG, "view_splat: null pointer");
  const long long per_block = (long long)VIEW_THREADS * VIEW_POINTS_PER_THREAD;
  const unsigned nblk = (unsigned)((n + per_block - 1) / per_block);
  if (is_double)
    hipLaunchKernelGGL(view_splat_kernel<double>, dim3(nblk), dim3(VIEW_THREADS), 0, st, (const double*)points, n, cameras,
                       n_views, offsets, n_slices, slice_mask, size, cmin, cmax, height, width, zbuf, bad);
  else
    hipLaunchKernelGGL(view_splat_kernel<float>, dim3(nblk), dim3(VIEW_THREADS), 0, st, (const float*)points, n, cameras,
                       n_views, offsets, n_slices, slice_mask, size, cmin, cmax, height, width, zbuf, bad);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_view_lines(const double* segments, const int* segment_ids, int n_segments, const double* styles,
                   int n_lines, const double* cameras, int n_views, int height, int width, unsigned long long* zbuf,
                   int device, void* stream) {
  if (n_segments < 0 || n_lines < 0 || n_lines > (1 << 24) || !view_image_ok(n_views, height, width)) return fail(PRH_ERR_ARG, "view_lines: bad argument");
  if (n_segments == 0 || (long long)n_views * height * width == 0) return PRH_OK;
  if (!segments || !segment_ids || !styles || !cameras || !zbuf) return fail(PRH_ERR_ARG, "view_lines: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(view_lines_kernel, dim3((unsigned)n_segments), dim3(VIEW_THREADS), 0, (hipStream_t)stream, segments,
                     segment_ids, styles, n_lines, cameras, n_views, height, width, zbuf);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_view_resolve(const unsigned long long* zbuf, long long pixels, const unsigned* table,
                     const unsigned* line_colours, int n_lines, unsigned background, unsigned* rgba, float* depth,
                     int device, void* stream) {
  if (pixels < 0 || pixels >= 256ll * 0x7fffffff || n_lines < 0) return fail(PRH_ERR_ARG, "view_resolve: bad argument");
  if (pixels == 0) return PRH_OK;
  if (!zbuf || !table || !rgba || !depth || (n_lines > 0 && !line_colours))
    return fail(PRH_ERR_ARG, "view_resolve: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(view_resolve_kernel, dim3((unsigned)((pixels + VIEW_THREADS - 1) / VIEW_THREADS)), dim3(VIEW_THREADS),
                     0, (hipStream_t)stream, zbuf, pixels, table, line_colours, n_lines, background, rgba, depth);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ map fusion
int prh_fuse_max_points(void) { return FUSE_MAX_POINTS; }
int prh_fuse_tile(void) { return FUSE_TILE; }
size_t prh_fuse_project_workspace_bytes(int n_poses) {
  if (n_poses < 0) return 0;
  return align_up((size_t)n_poses * sizeof(DrvPose), 256) + 256;
}
int prh_fuse_project(const double* pieces, long long n_pieces, int points_per_piece, const int* piece_line,
                     const int* piece_pose, const double* poses, int n_poses, const double* line_vertices,
                     const long long* line_offsets, const double* line_cum, int n_lines, double* world, double* s,
                     double* d, int* seg, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const int M = points_per_piece;
  if (n_pieces < 0 || M < 1 || n_poses < 0 || n_lines < 0) return fail(PRH_ERR_ARG, "fuse_project: bad argument");
  if (n_pieces > (long long)FUSE_THREADS * 0x7fffffff / M) return fail(PRH_ERR_ARG, "fuse_project: too many points");
  if (n_pieces == 0) return PRH_OK;
  if (!pieces || !world) return fail(PRH_ERR_ARG, "fuse_project: null pointer");
  if (piece_pose && (!poses || n_poses == 0)) return fail(PRH_ERR_ARG, "fuse_project: piece_pose without poses");
  if (piece_line && (!s || !d || !seg || (n_lines > 0 && (!line_offsets || !line_vertices || !line_cum))))
    return fail(PRH_ERR_ARG, "fuse_project: null pointer");
  if (piece_pose && (!workspace || workspace_bytes < prh_fuse_project_workspace_bytes(n_poses)))
    return fail(PRH_ERR_WORKSPACE, "fuse_project: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  DrvPose* pose = (DrvPose*)workspace;
  if (piece_pose) {
    hipLaunchKernelGGL(drv_pose_kernel, dim3(cdiv(n_poses, 256)), dim3(256), 0, st, poses, n_poses, pose);
    LAUNCH_CHECK();
  }
  const long long n_points = n_pieces * M;
  hipLaunchKernelGGL(fuse_project_kernel, dim3((unsigned)((n_points + FUSE_THREADS - 1) / FUSE_THREADS)),
                     dim3(FUSE_THREADS), 0, st, pieces, n_points, M, piece_line, piece_pose, (const DrvPose*)pose,
                     n_poses, line_vertices, line_offsets, line_cum, n_lines, world, s, d, seg);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_fuse_gather_workspace_bytes(long long n_pieces) {
  if (n_pieces < 0) return 0;
  return align_up((size_t)n_pieces * 2 * sizeof(double), 256) + 256;
}
int prh_fuse_gather(const double* world, const double* s, long long n_pieces, int points_per_piece,
                    const long long* line_piece_offsets, int n_lines, const long long* node_offsets,
                    long long n_nodes, double ds, double* node_x, double* node_w, int* node_count,
                    double* node_spread, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const int M = points_per_piece;
  if (n_pieces < 0 || n_lines < 0 || n_nodes < 0 || M < 2 || M > FUSE_MAX_POINTS || !(ds > 0.0))
    return fail(PRH_ERR_ARG, "fuse_gather: bad argument (2..%d points per piece, ds > 0)", FUSE_MAX_POINTS);
  if (n_nodes >= (long long)FUSE_THREADS * 0x7fffffff || n_pieces >= (long long)FUSE_THREADS * 0x7fffffff)
    return fail(PRH_ERR_ARG, "fuse_gather: too many nodes or pieces");
  if (n_nodes == 0) return PRH_OK;
  if (n_lines == 0 || !line_piece_offsets || !node_offsets || !node_x || !node_w || !node_count || !node_spread ||
      (n_pieces > 0 && (!world || !s)))
    return fail(PRH_ERR_ARG, "fuse_gather: null pointer");
  if (!workspace || workspace_bytes < prh_fuse_gather_workspace_bytes(n_pieces))
    return fail(PRH_ERR_WORKSPACE, "fuse_gather: workspace too small (%zu bytes)", workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  double* range = (double*)workspace;
  if (n_pieces > 0) {
    hipLaunchKernelGGL(fuse_range_kernel, dim3((unsigned)((n_pieces + FUSE_THREADS - 1) / FUSE_THREADS)),
                       dim3(FUSE_THREADS), 0, st, s, n_pieces, M, range);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fuse_gather_kernel, dim3((unsigned)((n_nodes + FUSE_THREADS - 1) / FUSE_THREADS)),
                     dim3(FUSE_THREADS), 0, st, world, s, (const double*)range, M, line_piece_offsets, n_lines,
                     node_offsets, n_nodes, ds, node_x, node_w, node_count, node_spread);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ piece linking
int prh_link_tile(void) { return LINK_TILE; }
int prh_link_pairs_per_block(void) { return LINK_PAIRS; }
size_t prh_link_pairs_workspace_bytes(long long n_pieces) {
  if (n_pieces < 0) return 0;
  return align_up((size_t)n_pieces * 6 * sizeof(double), 256) + align_up((size_t)n_pieces * sizeof(long long), 256) + 256;
}
// boxes, then <WRITE> of link_pairs_kernel; the count call also scans the row counts on the device
static int link_pairs(bool write, const char* what, const double* world, long long n_pieces, int M,
                      const int* piece_frame, double gate, long long* pair_offsets, int* pair_j, void* workspace,
                      size_t workspace_bytes, int device, void* stream) {
  if (n_pieces < 0 || n_pieces > (1ll << 24) || M < 2 || M > FUSE_MAX_POINTS || !(gate >= 0.0))
    return fail(PRH_ERR_ARG, "%s: bad argument (at most 2^24 pieces of 2..%d points, gate >= 0)", what, FUSE_MAX_POINTS);
  if (!pair_offsets) return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if (n_pieces > 0 && (!world || !piece_frame || (write && !pair_j))) return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if (!workspace || workspace_bytes < prh_link_pairs_workspace_bytes(n_pieces))
    return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const int P = (int)n_pieces;
  double* box = (double*)workspace;
  long long* row_count = (long long*)((char*)workspace + align_up((size_t)n_pieces * 6 * sizeof(double), 256));
  if (P > 0) {
    hipLaunchKernelGGL(link_box_kernel, dim3(cdiv(P, LINK_THREADS)), dim3(LINK_THREADS), 0, st, world, P, M, box);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(write ? link_pairs_kernel<true> : link_pairs_kernel<false>, dim3(cdiv(P, LINK_ROWS)),
                       dim3(LINK_THREADS), 0, st, (const double*)box, piece_frame, P, gate, row_count,
                       (const long long*)pair_offsets, pair_j);
    LAUNCH_CHECK();
  }
  if (!write) {
    hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(LINK_SCAN_THREADS), 0, st, (const long long*)row_count, P,
                       pair_offsets);
    LAUNCH_CHECK();
  }
  return PRH_OK;
}
int prh_link_pairs_count(const double* world, long long n_pieces, int points_per_piece, const int* piece_frame,
                         double gate, long long* pair_offsets, void* workspace, size_t workspace_bytes, int device,
                         void* stream) {
  return link_pairs(false, "link_pairs_count", world, n_pieces, points_per_piece, piece_frame, gate, pair_offsets,
                    nullptr, workspace, workspace_bytes, device, stream);
}
int prh_link_pairs_write(const double* world, long long n_pieces, int points_per_piece, const int* piece_frame,
                         double gate, const long long* pair_offsets, int* pair_j, void* workspace,
                         size_t workspace_bytes, int device, void* stream) {
  return link_pairs(true, "link_pairs_write", world, n_pieces, points_per_piece, piece_frame, gate,
                    (long long*)pair_offsets, pair_j, workspace, workspace_bytes, device, stream);
}
int prh_link_stats(const double* world, const double* cum, long long n_pieces, int points_per_piece,
                   const long long* pair_offsets, const int* pair_j, long long n_pairs, double gate, int* pair_count,
                   double* pair_sum, int device, void* stream) {
  const int M = points_per_piece;
  if (n_pieces < 0 || n_pieces > (1ll << 24) || n_pairs < 0 || M < 2 || M > FUSE_MAX_POINTS || !(gate >= 0.0))
    return fail(PRH_ERR_ARG, "link_stats: bad argument (at most 2^24 pieces of 2..%d points, gate >= 0)", FUSE_MAX_POINTS);
  if (n_pairs >= (long long)LINK_PAIRS * 0x7fffffff) return fail(PRH_ERR_ARG, "link_stats: too many pairs");
  if (n_pairs == 0) return PRH_OK;
  if (n_pieces == 0) return fail(PRH_ERR_ARG, "link_stats: pairs without pieces");
  if (!world || !cum || !pair_offsets || !pair_j || !pair_count || !pair_sum)
    return fail(PRH_ERR_ARG, "link_stats: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(link_stats_kernel, dim3((unsigned)((n_pairs + LINK_PAIRS - 1) / LINK_PAIRS)), dim3(LINK_THREADS), 0,
                     (hipStream_t)stream, world, cum, (int)n_pieces, M, pair_offsets, pair_j, n_pairs, gate, pair_count,
                     pair_sum);
  LAUNCH_CHECK();
  return PRH_OK;
}

// steps 5-6 and cum on the device (prh_link_sync.hpp)
static inline bool link_size_bad(long long n_pieces) { return n_pieces < 0 || n_pieces > (1ll << 24); }
static inline unsigned sync_grid(long long n) { return (unsigned)((n + SYNC_THREADS - 1) / SYNC_THREADS); }
int prh_link_cum(const double* world, long long n_pieces, int points_per_piece, double* cum, int device, void* stream) {
  if (link_size_bad(n_pieces) || points_per_piece < 2 || points_per_piece > FUSE_MAX_POINTS)
    return fail(PRH_ERR_ARG, "link_cum: bad argument (at most 2^24 pieces of 2..%d points)", FUSE_MAX_POINTS);
  if (n_pieces == 0) return PRH_OK;
  if (!world || !cum) return fail(PRH_ERR_ARG, "link_cum: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(link_cum_kernel, dim3(sync_grid(n_pieces)), dim3(SYNC_THREADS), 0, (hipStream_t)stream, world,
                     (int)n_pieces, points_per_piece, cum);
  LAUNCH_CHECK();
  return PRH_OK;
}
long long prh_link_edges_blocks(long long n_pairs) {
  return n_pairs < 0 ? 0 : (n_pairs + SYNC_THREADS - 1) / SYNC_THREADS;
}
// edge_scan: [0 .. blocks] the exclusive scan of the blocks' edge counts, [blocks + 1 .. 2 blocks] the counts
int prh_link_edges(const long long* pair_offsets, long long n_pieces, const int* pair_count, const double* pair_sum,
                   long long n_pairs, long long min_in, long long out_ratio, int* pair_i, unsigned char* edge,
                   signed char* rho, double* delta, long long* edge_scan, int device, void* stream) {
  if (link_size_bad(n_pieces) || n_pairs < 0 || min_in < 1 || out_ratio < 0 ||
      n_pairs >= (long long)SYNC_THREADS * 0x7fffffff)
    return fail(PRH_ERR_ARG, "link_edges: bad argument (at most 2^24 pieces, min_in >= 1, out_ratio >= 0)");
  if (!edge_scan) return fail(PRH_ERR_ARG, "link_edges: null pointer");
  if (n_pairs > 0 && (n_pieces == 0 || !pair_offsets || !pair_count || !pair_sum || !pair_i || !edge || !rho || !delta))
    return fail(PRH_ERR_ARG, "link_edges: null pointer, or pairs without pieces");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  const long long blocks = prh_link_edges_blocks(n_pairs);
  long long* block_count = edge_scan + blocks + 1;
  if (blocks > 0) {
    hipLaunchKernelGGL(link_edges_kernel, dim3((unsigned)blocks), dim3(SYNC_THREADS), 0, st, pair_offsets, (int)n_pieces,
                       pair_count, pair_sum, n_pairs, min_in, out_ratio, pair_i, edge, rho, delta, block_count);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(link_scan_kernel, dim3(1), dim3(LINK_SCAN_THREADS), 0, st, (const long long*)block_count,
                     (int)blocks, edge_scan);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_link_edges_compact(const int* pair_i, const int* pair_j, const int* pair_count, const unsigned char* edge,
                           const signed char* rho, const double* delta, long long n_pairs, const long long* edge_scan,
                           long long n_edges, int* edge_ij, int* edge_w, double* edge_delta, int device, void* stream) {
  if (n_pairs < 0 || n_edges < 0 || n_edges > n_pairs || n_pairs >= (long long)SYNC_THREADS * 0x7fffffff)
    return fail(PRH_ERR_ARG, "link_edges_compact: bad argument (0 <= n_edges <= n_pairs)");
  if (n_edges == 0) return PRH_OK;
  if (!pair_i || !pair_j || !pair_count || !edge || !rho || !delta || !edge_scan || !edge_ij || !edge_w || !edge_delta)
    return fail(PRH_ERR_ARG, "link_edges_compact: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(link_compact_kernel, dim3((unsigned)prh_link_edges_blocks(n_pairs)), dim3(SYNC_THREADS), 0,
                     (hipStream_t)stream, pair_i, pair_j, pair_count, edge, rho, delta, n_pairs, edge_scan, n_edges, edge_ij,
                     edge_w, edge_delta);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_link_label_round(const int* edge_ij, long long n_edges, long long n_pieces, int* label, int* changed, int device,
                         void* stream) {
  if (link_size_bad(n_pieces) || n_edges < 0 || n_edges >= (long long)SYNC_THREADS * 0x7fffffff)
    return fail(PRH_ERR_ARG, "link_label_round: bad argument (at most 2^24 pieces)");
  if (!changed || (n_pieces > 0 && !label) || (n_edges > 0 && !edge_ij))
    return fail(PRH_ERR_ARG, "link_label_round: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(changed, 0, sizeof(int), st));
  if (n_edges == 0 || n_pieces == 0) return PRH_OK;
  hipLaunchKernelGGL(link_hook_kernel, dim3(sync_grid(n_edges)), dim3(SYNC_THREADS), 0, st, edge_ij, n_edges, (int)n_pieces,
                     label, changed);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(link_jump_kernel, dim3(sync_grid(n_pieces)), dim3(SYNC_THREADS), 0, st, (int)n_pieces, label);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_link_tree_init(const int* label, long long n_pieces, int* level, int* parent, int* sign, double* offset,
                       unsigned long long* key, int device, void* stream) {
  if (link_size_bad(n_pieces)) return fail(PRH_ERR_ARG, "link_tree_init: at most 2^24 pieces");
  if (n_pieces == 0) return PRH_OK;
  if (!label || !level || !parent || !sign || !offset || !key) return fail(PRH_ERR_ARG, "link_tree_init: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(link_tree_init_kernel, dim3(sync_grid(n_pieces)), dim3(SYNC_THREADS), 0, (hipStream_t)stream, label,
                     (int)n_pieces, level, parent, sign, offset, key);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_link_tree_level(const int* edge_ij, const int* edge_w, const double* edge_delta, long long n_edges,
                        long long n_pieces, int n, int* level, int* parent, int* sign, double* offset,
                        unsigned long long* key, int* placed, int device, void* stream) {
  if (link_size_bad(n_pieces) || n_edges < 0 || n < 0 || n_edges >= (long long)SYNC_THREADS * 0x7fffffff)
    return fail(PRH_ERR_ARG, "link_tree_level: bad argument (at most 2^24 pieces, level >= 0)");
  if (!placed || (n_edges > 0 && (!edge_ij || !edge_w || !edge_delta || !level || !parent || !sign || !offset || !key)))
    return fail(PRH_ERR_ARG, "link_tree_level: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(placed, 0, sizeof(int), st));
  if (n_edges == 0 || n_pieces == 0) return PRH_OK;
  hipLaunchKernelGGL(link_propose_kernel, dim3(sync_grid(n_edges)), dim3(SYNC_THREADS), 0, st, edge_ij, edge_w, n_edges,
                     (int)n_pieces, n, (const int*)level, key);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(link_place_kernel, dim3(sync_grid(n_edges)), dim3(SYNC_THREADS), 0, st, edge_ij, edge_w, edge_delta,
                     n_edges, (int)n_pieces, n, (const unsigned long long*)key, level, parent, sign, offset, placed);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ cloud support
int prh_support_max_cells(void) { return 1 << 22; }
int prh_support_accumulate(const float* cloud, long long n_points, double origin_x, double origin_y, double origin_z,
                           double grid_x0, double grid_y0, double grid_cell, int grid_nx, int grid_ny,
                           const int* cell_offsets, const int* cell_entries, long long n_entries,
                           const double* line_vertices, const long long* line_offsets, const double* line_cum,
                           int n_lines, const long long* node_offsets, long long n_nodes, double step, double r2,
                           double intensity_floor, long long* acc, int device, void* stream) {
  if (n_points < 0 || n_points > 0x7fffffffll || n_lines < 0 || n_nodes < 0 || n_entries < 0 || n_entries > 0x7fffffffll ||
      grid_nx < 0 || grid_ny < 0 || !(step > 0.0) || !(r2 > 0.0) || !(r2 <= 64.0) || !(intensity_floor == intensity_floor))
    return fail(PRH_ERR_ARG, "support_accumulate: bad argument (fewer than 2^31 points, step > 0, 0 < radius <= 8)");
  if ((long long)grid_nx * grid_ny > (long long)prh_support_max_cells())
    return fail(PRH_ERR_ARG, "support_accumulate: at most %d grid cells", prh_support_max_cells());
  if (n_points == 0 || n_nodes == 0 || n_entries == 0 || grid_nx == 0 || grid_ny == 0) return PRH_OK;
  if (!(grid_cell > 0.0) || !(grid_x0 == grid_x0) || !(grid_y0 == grid_y0))
    return fail(PRH_ERR_ARG, "support_accumulate: bad grid");
  if (((uintptr_t)cloud & 15) != 0) return fail(PRH_ERR_ARG, "support_accumulate: cloud must be 16-byte aligned");
  if (!cloud || !cell_offsets || !cell_entries || !line_vertices || !line_offsets || !line_cum || !node_offsets || !acc ||
      n_lines == 0)
    return fail(PRH_ERR_ARG, "support_accumulate: null pointer");
  HIP_TRY(hipSetDevice(device));
  SupportGrid grid{grid_x0, grid_y0, grid_cell, grid_nx, grid_ny};
  hipLaunchKernelGGL(support_kernel, dim3((unsigned)((n_points + SUPPORT_THREADS - 1) / SUPPORT_THREADS)),
                     dim3(SUPPORT_THREADS), 0, (hipStream_t)stream, (const float4*)cloud, n_points, origin_x, origin_y,
                     origin_z, grid, cell_offsets, (const int2*)cell_entries, line_vertices, line_offsets, line_cum,
                     node_offsets, n_lines, step, r2, intensity_floor, (unsigned long long*)acc);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ ground lift, paint alignment
// What every entry that takes a slice grid checks first, in one order.  align_mask and align_text: the points'
// alignment rule; floor_ok and bitmap_ok: the two checks the paint-alignment entries add in their places
// (ground lift has neither).
static int check_grid(const char* what, const void* points, unsigned align_mask, const char* align_text,
                      const long long* slice_offsets, int n_slices, long long n_points, const double* grid_origin,
                      const int* grid_shape, const long long* cell_base, long long n_cells, double cell,
                      bool floor_ok = true, bool bitmap_ok = true) {
  if (n_slices < 0 || n_points < 0 || n_cells < 0 || n_cells > 0x7fffffffll || n_points >= 256ll * 0x7fffffff)
    return fail(PRH_ERR_ARG, "%s: bad argument (at most 2^31 - 1 cells)", what);
  if (!(cell > 0.0) || !(cell < 1e300)) return fail(PRH_ERR_ARG, "%s: cell must be positive and finite", what);
  if (!floor_ok) return fail(PRH_ERR_ARG, "%s: intensity_floor must be finite", what);
  if ((n_slices > 0 && (!slice_offsets || !grid_origin || !grid_shape || !cell_base)) || !bitmap_ok)
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if (n_points > 0 && (!points || n_slices == 0)) return fail(PRH_ERR_ARG, "%s: points without a slice", what);
  if (((uintptr_t)points & align_mask) != 0) return fail(PRH_ERR_ARG, "%s: points must be %s", what, align_text);
  return PRH_OK;
}

int prh_ground_max_bins(void) { return GROUND_MAX_BINS; }
size_t prh_ground_bin_workspace_bytes(long long n_cells) {
  return n_cells < 0 ? 0 : align_up((size_t)n_cells * sizeof(int), 256);
}
static int ground_check_grid(const char* what, const void* points, int is_double, const long long* slice_offsets,
                             int n_slices, long long n_points, const double* grid_origin, const int* grid_shape,
                             const long long* cell_base, long long n_cells, double cell) {
  return check_grid(what, points, is_double ? 15 : 7,
                    is_double ? "aligned to two coordinates (16 bytes)" : "aligned to two coordinates (8 bytes)",
                    slice_offsets, n_slices, n_points, grid_origin, grid_shape, cell_base, n_cells, cell);
}
// count (counter: the caller's cell_counts, zeroed here) or write (counter: the cursors, in the workspace)
static int ground_bin(bool write, const void* points, int is_double, const long long* slice_offsets, int n_slices,
                      long long n_points, const double* grid_origin, const int* grid_shape, const long long* cell_base,
                      long long n_cells, double cell, int* cell_counts, const long long* cell_offsets, int* rows,
                      long long capacity, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const char* what = write ? "ground_bin_write" : "ground_bin_count";
  TRY_RC(ground_check_grid(what, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                           cell_base, n_cells, cell));
  if (write) {
    if (capacity < 0) return fail(PRH_ERR_ARG, "%s: bad capacity", what);
    if (n_cells == 0 || n_points == 0 || capacity == 0) return PRH_OK;
    if (!cell_offsets || !rows) return fail(PRH_ERR_ARG, "%s: null pointer", what);
    if (!workspace || workspace_bytes < prh_ground_bin_workspace_bytes(n_cells))
      return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  } else {
    if (n_cells == 0) return PRH_OK;
    if (!cell_counts) return fail(PRH_ERR_ARG, "%s: null pointer", what);
  }
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* counter = write ? (int*)workspace : cell_counts;
  HIP_TRY(hipMemsetAsync(counter, 0, (size_t)n_cells * sizeof(int), st));
  if (n_points == 0) return PRH_OK;
  const unsigned nblk = (unsigned)((n_points + GROUND_THREADS - 1) / GROUND_THREADS);
  for_points(is_double, [&](auto t) {
    using T = decltype(t);
    auto kernel = write ? ground_bin_kernel<T, true> : ground_bin_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(GROUND_THREADS), 0, st, (const T*)points, slice_offsets, n_slices,
                       n_points, grid_origin, grid_shape, cell_base, n_cells, cell, counter, cell_offsets, rows, capacity);
  });
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_ground_bin_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                         long long n_points, const double* grid_origin, const int* grid_shape,
                         const long long* cell_base, long long n_cells, double cell, int* cell_counts, int device,
                         void* stream) {
  return ground_bin(false, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape, cell_base,
                    n_cells, cell, cell_counts, nullptr, nullptr, 0, nullptr, 0, device, stream);
}
int prh_ground_bin_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                         long long n_points, const double* grid_origin, const int* grid_shape,
                         const long long* cell_base, long long n_cells, double cell, const long long* cell_offsets,
                         int* rows, long long capacity, void* workspace, size_t workspace_bytes, int device,
                         void* stream) {
  return ground_bin(true, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape, cell_base,
                    n_cells, cell, nullptr, cell_offsets, rows, capacity, workspace, workspace_bytes, device, stream);
}
int prh_ground_query(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long n_points,
                     const double* queries, const long long* query_offsets, long long n_queries,
                     const double* grid_origin, const int* grid_shape, const long long* cell_base, long long n_cells,
                     double cell, const long long* cell_offsets, const int* rows, long long n_rows, double r2,
                     double reach, double z_lo, double bin, int n_bins, int min_points, int peak_num, int peak_den,
                     double* height, int* count, int* hits, int* bin_index, int device, void* stream) {
  TRY_RC(ground_check_grid("ground_query", points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                           cell_base, n_cells, cell));
  if (n_queries < 0 || n_queries >= 4ll * 0x7fffffff || n_rows < 0 || n_rows > n_points)
    return fail(PRH_ERR_ARG, "ground_query: bad argument");
  if (!(r2 > 0.0) || !(r2 <= 16.0) || !(reach > 0.0) || !(reach * reach >= r2) || !(reach <= 8.0))
    return fail(PRH_ERR_ARG, "ground_query: 0 < radius <= 4 and radius <= reach <= 8");
  if (n_bins < 1 || n_bins > GROUND_MAX_BINS || !(bin > 0.0) || !(z_lo >= -256.0) || !(z_lo + n_bins * bin <= 256.0))
    return fail(PRH_ERR_ARG, "ground_query: 1 <= n_bins <= %d, bin > 0 and the histogram inside [-256, 256]",
                GROUND_MAX_BINS);
  if (min_points < 1 || peak_num < 1 || peak_num > peak_den || peak_den > 65536)
    return fail(PRH_ERR_ARG, "ground_query: min_points >= 1 and 1 <= peak_num <= peak_den <= 65536");
  if (n_queries == 0) return PRH_OK;
  if (!queries || !query_offsets || n_slices == 0 || !height || !count || !hits || !bin_index ||
      (n_cells > 0 && !cell_offsets) || (n_rows > 0 && !rows))
    return fail(PRH_ERR_ARG, "ground_query: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  GroundParams prm{r2, reach, cell, z_lo, bin, n_bins, min_points, peak_num, peak_den};
  const unsigned nblk = (unsigned)((n_queries + GROUND_WAVES - 1) / GROUND_WAVES);
  for_points(is_double, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(ground_query_kernel<T>, dim3(nblk), dim3(GROUND_THREADS), 0, st, (const T*)points, slice_offsets,
                       n_slices, queries, query_offsets, n_queries, grid_origin, grid_shape, cell_base, cell_offsets, rows,
                       n_rows, n_cells, prm, height, count, hits, bin_index);
  });
  LAUNCH_CHECK();
  return PRH_OK;
}

int prh_align_tile(void) { return ALIGN_TILE; }
int prh_align_max_shifts(void) { return ALIGN_MAX_SHIFTS; }
int prh_align_max_poses(void) { return ALIGN_MAX_POSES; }
size_t prh_align_select_workspace_bytes(int n_slices) {
  return n_slices < 0 ? 0 : align_up((size_t)n_slices * sizeof(int), 256);
}
size_t prh_align_select_cells_workspace_bytes(long long n_cells) {
  return n_cells < 0 ? 0 : align_up((size_t)n_cells * sizeof(int), 256);
}
// The candidate filter in arrival order (one counter per slice) or, by_cell, in cell order (one per bitmap cell):
// count (counter: the caller's counts, zeroed here) or write (counter: the cursors, in the workspace; offsets: the
// exclusive scan of the counts).
static int align_select(bool by_cell, bool write, const void* points, int is_double, const long long* slice_offsets,
                        int n_slices, long long n_points, const double* grid_origin, const int* grid_shape,
                        const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                        double intensity_floor, int* counts, const long long* offsets, void* records,
                        long long capacity, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const char* what = by_cell ? (write ? "align_select_cells_write" : "align_select_cells_count")
                             : (write ? "align_select_write" : "align_select_count");
  TRY_RC(check_grid(what, points, 15, "16-byte aligned", slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                    cell_base, n_cells, cell, intensity_floor > -1e300 && intensity_floor < 1e300,
                    !(n_cells > 0 && !bitmap)));
  const long long n_counters = by_cell ? n_cells : n_slices;
  if (write) {
    if (capacity < 0) return fail(PRH_ERR_ARG, "%s: bad capacity", what);
    if (n_slices == 0 || n_points == 0 || n_cells == 0 || capacity == 0) return PRH_OK;
    if (!offsets || !records) return fail(PRH_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)records & 15) != 0) return fail(PRH_ERR_ARG, "%s: records must be 16-byte aligned", what);
    if (!workspace || workspace_bytes < (by_cell ? prh_align_select_cells_workspace_bytes(n_cells)
                                                 : prh_align_select_workspace_bytes(n_slices)))
      return fail(PRH_ERR_WORKSPACE, "%s: workspace too small (%zu bytes)", what, workspace_bytes);
  } else {
    if (n_counters == 0 || n_slices == 0) return PRH_OK;
    if (!counts) return fail(PRH_ERR_ARG, "%s: null pointer", what);
  }
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  int* counter = write ? (int*)workspace : counts;
  HIP_TRY(hipMemsetAsync(counter, 0, (size_t)n_counters * sizeof(int), st));
  if (n_points == 0 || n_cells == 0) return PRH_OK;
  const unsigned nblk = (unsigned)((n_points + ALIGN_THREADS - 1) / ALIGN_THREADS);
  for_points(is_double, [&](auto t) {
    using T = decltype(t);
    auto kernel = by_cell ? (write ? align_select_cells_kernel<T, true> : align_select_cells_kernel<T, false>)
                          : (write ? align_select_kernel<T, true> : align_select_kernel<T, false>);
    hipLaunchKernelGGL(kernel, dim3(nblk), dim3(ALIGN_THREADS), 0, st, (const T*)points, slice_offsets, n_slices,
                       n_points, grid_origin, grid_shape, cell_base, bitmap, n_cells, cell, intensity_floor, counter,
                       offsets, (AlignRecord*)records, capacity);
  });
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_align_select_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long n_points, const double* grid_origin, const int* grid_shape,
                           const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                           double intensity_floor, int* slice_counts, int device, void* stream) {
  return align_select(false, false, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                      cell_base, bitmap, n_cells, cell, intensity_floor, slice_counts, nullptr, nullptr, 0, nullptr, 0,
                      device, stream);
}
int prh_align_select_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long n_points, const double* grid_origin, const int* grid_shape,
                           const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                           double intensity_floor, const long long* cand_offsets, void* records, long long capacity,
                           void* workspace, size_t workspace_bytes, int device, void* stream) {
  return align_select(false, true, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                      cell_base, bitmap, n_cells, cell, intensity_floor, nullptr, cand_offsets, records, capacity,
                      workspace, workspace_bytes, device, stream);
}
int prh_align_select_cells_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                                 long long n_points, const double* grid_origin, const int* grid_shape,
                                 const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                                 double intensity_floor, int* cell_counts, int device, void* stream) {
  return align_select(true, false, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                      cell_base, bitmap, n_cells, cell, intensity_floor, cell_counts, nullptr, nullptr, 0, nullptr, 0,
                      device, stream);
}
int prh_align_select_cells_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                                 long long n_points, const double* grid_origin, const int* grid_shape,
                                 const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                                 double intensity_floor, const long long* cell_offsets, void* records,
                                 long long capacity, void* workspace, size_t workspace_bytes, int device,
                                 void* stream) {
  return align_select(true, true, points, is_double, slice_offsets, n_slices, n_points, grid_origin, grid_shape,
                      cell_base, bitmap, n_cells, cell, intensity_floor, nullptr, cell_offsets, records, capacity,
                      workspace, workspace_bytes, device, stream);
}
// the score sweep over a shift table (K,2) or, rigid, a pose table (K,4) with the slices' pivots
static int align_score(bool rigid, const void* records, const long long* cand_offsets, long long n_candidates,
                       const double* line_vertices, long long n_vertices, const long long* line_offsets, int n_lines,
                       const long long* slice_line_offsets, const double* table, const long long* table_offsets,
                       long long n_rows, const double* pivots, const double* reach, int n_slices, const long long* items,
                       long long n_items, double r2, long long* acc, int device, void* stream) {
  const char* what = rigid ? "align_score_rigid" : "align_score";
  if (n_candidates < 0 || n_vertices < 0 || n_lines < 0 || n_rows < 0 || n_slices < 0 || n_items < 0 ||
      n_items > 0x7fffffffll)
    return fail(PRH_ERR_ARG, "%s: bad argument (at most 2^31 - 1 work items)", what);
  if (!(r2 > 0.0) || !(r2 <= 1.0)) return fail(PRH_ERR_ARG, "%s: 0 < radius <= 1", what);
  if (n_items == 0) return PRH_OK;
  if (!records || !cand_offsets || !line_vertices || !line_offsets || !slice_line_offsets || !table || !table_offsets ||
      (rigid && !pivots) || !reach || !items || !acc || n_slices == 0)
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  if (((uintptr_t)records & 15) != 0 || (rigid && ((uintptr_t)table & 15) != 0))
    return fail(PRH_ERR_ARG, "%s: %s must be 16-byte aligned", what, rigid ? "records and poses" : "records");
  HIP_TRY(hipSetDevice(device));
  auto kernel = rigid ? align_score_kernel<true> : align_score_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_items), dim3(ALIGN_THREADS), 0, (hipStream_t)stream,
                     (const AlignRecord*)records, cand_offsets, n_candidates, line_vertices, n_vertices, line_offsets,
                     n_lines, slice_line_offsets, table, table_offsets, n_rows, reach, n_slices, items, r2,
                     (unsigned long long*)acc, pivots);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_align_score(const void* records, const long long* cand_offsets, long long n_candidates,
                    const double* line_vertices, long long n_vertices, const long long* line_offsets, int n_lines,
                    const long long* slice_line_offsets, const double* shifts, const long long* shift_offsets,
                    long long n_shifts, const double* reach, int n_slices, const long long* items, long long n_items,
                    double r2, long long* acc, int device, void* stream) {
  return align_score(false, records, cand_offsets, n_candidates, line_vertices, n_vertices, line_offsets, n_lines,
                     slice_line_offsets, shifts, shift_offsets, n_shifts, nullptr, reach, n_slices, items, n_items, r2, acc,
                     device, stream);
}
int prh_align_score_rigid(const void* records, const long long* cand_offsets, long long n_candidates,
                          const double* line_vertices, long long n_vertices, const long long* line_offsets, int n_lines,
                          const long long* slice_line_offsets, const double* poses, const long long* pose_offsets,
                          long long n_poses, const double* pivots, const double* reach, int n_slices,
                          const long long* items, long long n_items, double r2, long long* acc, int device,
                          void* stream) {
  return align_score(true, records, cand_offsets, n_candidates, line_vertices, n_vertices, line_offsets, n_lines,
                     slice_line_offsets, poses, pose_offsets, n_poses, pivots, reach, n_slices, items, n_items, r2, acc,
                     device, stream);
}

// ------------------------------------------------------------------ paint tracing
int prh_trace_max_nms(void) { return TRACE_MAX_NMS; }
static bool trace_shape_ok(int n_slices, int nx, int ny) {
  return n_slices >= 0 && nx >= 1 && nx <= TRACE_MAX_CELLS && ny >= 1 && ny <= TRACE_MAX_CELLS &&
         (long long)n_slices * nx <= 0x7fffffffll;
}
// n [C] int32 first, then w, wx, wy, wz [C] int64, each on a 256-byte boundary; C = n_slices * nx * ny
size_t prh_trace_workspace_bytes(int n_slices, int nx, int ny) {
  if (!trace_shape_ok(n_slices, nx, ny)) return 0;
  const size_t cells = (size_t)n_slices * (size_t)nx * (size_t)ny;
  return align_up(cells * sizeof(int), 256) + 4 * align_up(cells * sizeof(long long), 256);
}
static int trace_tables(const char* what, void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny,
                        TraceTables& t) {
  if (!trace_shape_ok(n_slices, nx, ny))
    return fail(PRH_ERR_ARG, "%s: 1 <= nx, ny <= %d and fewer than 2^31 columns", what, TRACE_MAX_CELLS);
  if (n_slices == 0) return PRH_OK;
  if (!workspace || ((uintptr_t)workspace & 255) != 0 || workspace_bytes < prh_trace_workspace_bytes(n_slices, nx, ny))
    return fail(PRH_ERR_WORKSPACE, "%s: workspace missing, not 256-byte aligned or too small (%zu bytes)", what,
                workspace_bytes);
  const size_t cells = (size_t)n_slices * (size_t)nx * (size_t)ny;
  char* p = (char*)workspace;
  t.n = (int*)p;
  p += align_up(cells * sizeof(int), 256);
  unsigned long long** tabs[4] = {&t.w, &t.wx, &t.wy, &t.wz};
  for (auto tab : tabs) {
    *tab = (unsigned long long*)p;
    p += align_up(cells * sizeof(long long), 256);
  }
  return PRH_OK;
}
// sg == nullptr: the ungated pass.  Else the surface gate with ground [n_slices][gx][gy] and off_surface [n_slices].
static int trace_hist(const char* what, const void* points, int is_double, const long long* slice_offsets, int n_slices,
                      long long first_row, long long n_rows, double half_length, double col, int nx, double half_width,
                      double cell, int ny, double intensity_floor, void* workspace, size_t workspace_bytes,
                      const TraceSurface* sg, const double* ground, long long* off_surface, int device, void* stream) {
  TraceTables t{};
  TRY_RC(trace_tables(what, workspace, workspace_bytes, n_slices, nx, ny, t));
  if (first_row < 0 || n_rows < 0 || n_rows >= 256ll * 0x7fffffff) return fail(PRH_ERR_ARG, "%s: bad argument", what);
  if (!(half_length > 0.0) || !(half_length <= 128.0) || !(half_width > 0.0) || !(half_width <= 128.0) || !(col > 0.0) ||
      !(cell > 0.0) || !(col < 1e300) || !(cell < 1e300))
    return fail(PRH_ERR_ARG, "%s: 0 < half_length, half_width <= 128 and col, cell positive and finite", what);
  if (!(intensity_floor == intensity_floor) || !(fabs(intensity_floor) < 1e300))
    return fail(PRH_ERR_ARG, "%s: intensity_floor must be finite", what);
  if (sg) {
    if (sg->gx < 1 || sg->gx > FLOOR_MAX_CELLS || sg->gy < 1 || sg->gy > FLOOR_MAX_CELLS)
      return fail(PRH_ERR_ARG, "%s: 1 <= gx, gy <= %d", what, FLOOR_MAX_CELLS);
    if (!(sg->half_length > 0.0) || !(sg->half_length < 1e300) || !(sg->half_width > 0.0) || !(sg->half_width < 1e300) ||
        !(sg->cell > 0.0) || !(sg->cell < 1e300) || !(sg->band >= 0.0) || !(sg->band < 1e300))
      return fail(PRH_ERR_ARG, "%s: g_half_length, g_half_width, ground_cell positive, band >= 0, all finite", what);
    if (n_slices > 0 && !off_surface) return fail(PRH_ERR_ARG, "%s: null pointer", what);
    if (n_rows > 0 && !ground) return fail(PRH_ERR_ARG, "%s: points without a ground table", what);
  }
  if (n_rows > 0 && (!points || !slice_offsets || n_slices == 0)) return fail(PRH_ERR_ARG, "%s: points without a slice", what);
  if (((uintptr_t)points & (is_double ? 15 : 7)) != 0)
    return fail(PRH_ERR_ARG, "%s: points must be aligned to two coordinates (%d bytes)", what, is_double ? 16 : 8);
  if (n_slices == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(workspace, 0, prh_trace_workspace_bytes(n_slices, nx, ny), st));
  if (sg) HIP_TRY(hipMemsetAsync(off_surface, 0, (size_t)n_slices * sizeof(long long), st));
  if (n_rows == 0) return PRH_OK;
  const TraceGrid g{half_length, col, half_width, cell, intensity_floor, nx, ny};
  const unsigned nblk = (unsigned)((n_rows + TRACE_THREADS - 1) / TRACE_THREADS);
  for_points(is_double, [&](auto v) {
    using T = decltype(v);
    if (sg)
      hipLaunchKernelGGL(trace_hist_surface_kernel<T>, dim3(nblk), dim3(TRACE_THREADS), 0, st, (const T*)points,
                         slice_offsets, n_slices, first_row, n_rows, g, t, *sg, ground, (unsigned long long*)off_surface);
    else
      hipLaunchKernelGGL(trace_hist_kernel<T>, dim3(nblk), dim3(TRACE_THREADS), 0, st, (const T*)points, slice_offsets,
                         n_slices, first_row, n_rows, g, t);
  });
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_trace_hist(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long first_row,
                   long long n_rows, double half_length, double col, int nx, double half_width, double cell, int ny,
                   double intensity_floor, void* workspace, size_t workspace_bytes, int device, void* stream) {
  return trace_hist("trace_hist", points, is_double, slice_offsets, n_slices, first_row, n_rows, half_length, col, nx,
                    half_width, cell, ny, intensity_floor, workspace, workspace_bytes, nullptr, nullptr, nullptr, device,
                    stream);
}
int prh_trace_hist_surface(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long first_row, long long n_rows, double half_length, double col, int nx,
                           double half_width, double cell, int ny, double intensity_floor, void* workspace,
                           size_t workspace_bytes, double g_half_length, double g_half_width, double ground_cell, int gx,
                           int gy, const double* ground, double band, long long* off_surface, int device, void* stream) {
  const TraceSurface sg{g_half_length, g_half_width, ground_cell, band, gx, gy};
  return trace_hist("trace_hist_surface", points, is_double, slice_offsets, n_slices, first_row, n_rows, half_length, col,
                    nx, half_width, cell, ny, intensity_floor, workspace, workspace_bytes, &sg, ground, off_surface, device,
                    stream);
}
static int trace_peaks(bool write, void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny, int nms,
                       int min_points, long long min_weight, int* col_counts, const long long* col_offsets,
                       long long capacity, int col_base, int* iy, long long* weight, int* count, double* xyz, int* col,
                       int device, void* stream) {
  const char* what = write ? "trace_peaks_write" : "trace_peaks_count";
  TraceTables t{};
  TRY_RC(trace_tables(what, workspace, workspace_bytes, n_slices, nx, ny, t));
  if (nms < 0 || nms > TRACE_MAX_NMS || min_points < 1 || min_weight < 1)
    return fail(PRH_ERR_ARG, "%s: 0 <= nms <= %d, min_points >= 1 and min_weight >= 1", what, TRACE_MAX_NMS);
  if (col_base < 0 || capacity < 0 || capacity > 0x7fffffffll) return fail(PRH_ERR_ARG, "%s: bad argument", what);
  if (n_slices == 0 || (write && capacity == 0)) return PRH_OK;
  if (write ? (!col_offsets || !iy || !weight || !count || !xyz || !col) : !col_counts)
    return fail(PRH_ERR_ARG, "%s: null pointer", what);
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  auto kernel = write ? trace_peaks_kernel<true> : trace_peaks_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(n_slices * nx)), dim3(64), 0, st, t, ny, nms, min_points, min_weight,
                     col_counts, col_offsets, capacity, col_base, iy, weight, count, xyz, col);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_trace_peaks_count(void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny, int nms, int min_points,
                          long long min_weight, int* col_counts, int device, void* stream) {
  return trace_peaks(false, workspace, workspace_bytes, n_slices, nx, ny, nms, min_points, min_weight, col_counts, nullptr,
                     0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, device, stream);
}
int prh_trace_peaks_write(void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny, int nms, int min_points,
                          long long min_weight, const long long* col_offsets, long long capacity, int col_base, int* iy,
                          long long* weight, int* count, double* xyz, int* col, int device, void* stream) {
  return trace_peaks(true, workspace, workspace_bytes, n_slices, nx, ny, nms, min_points, min_weight, nullptr, col_offsets,
                     capacity, col_base, iy, weight, count, xyz, col, device, stream);
}
int prh_trace_link(const long long* col_offsets, long long n_cols, int nx, const int* iy, const int* col,
                   long long n_peaks, int link_cells, int gap_slope, int max_gap_cols, int* succ, int* pred, int device,
                   void* stream) {
  if (nx < 1 || nx > TRACE_MAX_CELLS || n_cols < 0 || n_cols > 0x7fffffffll || n_cols % nx != 0 || n_peaks < 0 ||
      n_peaks > 0x7fffffffll)
    return fail(PRH_ERR_ARG, "trace_link: bad argument (whole slices of nx columns, fewer than 2^31 peaks)");
  if (link_cells < 0 || link_cells > TRACE_MAX_CELLS || gap_slope < 0 || gap_slope > TRACE_MAX_CELLS || max_gap_cols < 0 ||
      max_gap_cols >= TRACE_MAX_CELLS)
    return fail(PRH_ERR_ARG, "trace_link: 0 <= link_cells, gap_slope <= %d and 0 <= max_gap_cols < %d", TRACE_MAX_CELLS,
                TRACE_MAX_CELLS);
  if (n_peaks == 0) return PRH_OK;
  if (!col_offsets || !iy || !col || !succ || !pred || n_cols == 0) return fail(PRH_ERR_ARG, "trace_link: null pointer");
  HIP_TRY(hipSetDevice(device));
  const unsigned nblk = (unsigned)((n_peaks + TRACE_THREADS - 1) / TRACE_THREADS);
  hipLaunchKernelGGL(trace_link_kernel, dim3(nblk), dim3(TRACE_THREADS), 0, (hipStream_t)stream, col_offsets, n_cols, nx,
                     iy, col, n_peaks, link_cells, gap_slope, max_gap_cols, succ, pred);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ paint floor
int prh_floor_max_bins(void) { return FLOOR_MAX_BINS; }
static int floor_hist(int copies, const void* points, int is_double, const long long* slice_offsets, int n_slices,
                      long long n_rows, double half_length, double half_width, double ground_cell, int gx, int gy,
                      const double* ground, double band, double bin_width, int n_bins, long long* hist, int device,
                      void* stream) {
  if (n_slices < 0 || n_rows < 0 || n_rows >= (long long)FLOOR_RUN * 0x7fffffff)
    return fail(PRH_ERR_ARG, "floor_hist: bad argument");
  if (gx < 1 || gx > FLOOR_MAX_CELLS || gy < 1 || gy > FLOOR_MAX_CELLS)
    return fail(PRH_ERR_ARG, "floor_hist: 1 <= gx, gy <= %d", FLOOR_MAX_CELLS);
  if (n_bins < 2 || n_bins > FLOOR_MAX_BINS) return fail(PRH_ERR_ARG, "floor_hist: 2 <= n_bins <= %d", FLOOR_MAX_BINS);
  if (!(half_length > 0.0) || !(half_length < 1e300) || !(half_width > 0.0) || !(half_width < 1e300) ||
      !(ground_cell > 0.0) || !(ground_cell < 1e300) || !(bin_width > 0.0) || !(bin_width < 1e300) || !(band >= 0.0) ||
      !(band < 1e300))
    return fail(PRH_ERR_ARG, "floor_hist: half_length, half_width, ground_cell, bin_width positive, band >= 0, all finite");
  if (copies != 1 && copies != 2 && copies != 4 && copies != 8) return fail(PRH_ERR_ARG, "floor_hist: 1, 2, 4 or 8 copies");
  if (n_slices > 0 && !hist) return fail(PRH_ERR_ARG, "floor_hist: null pointer");
  if (n_rows > 0 && (!points || !slice_offsets || !ground || n_slices == 0))
    return fail(PRH_ERR_ARG, "floor_hist: points without a slice or a ground table");
  if (((uintptr_t)points & (is_double ? 15 : 7)) != 0)
    return fail(PRH_ERR_ARG, "floor_hist: points must be aligned to two coordinates (%d bytes)", is_double ? 16 : 8);
  if (n_slices == 0) return PRH_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(hist, 0, (size_t)n_slices * (size_t)n_bins * sizeof(long long), st));
  if (n_rows == 0) return PRH_OK;
  const FloorGrid g{half_length, half_width, ground_cell, band, bin_width, gx, gy, n_bins};
  const unsigned nblk = (unsigned)((n_rows + FLOOR_RUN - 1) / FLOOR_RUN);
  auto launch = [&](auto copies_c) {                          // extern "C" holds no template: a generic lambda does
    for_points(is_double, [&](auto v) {
      using T = decltype(v);
      hipLaunchKernelGGL((floor_hist_kernel<T, decltype(copies_c)::value>), dim3(nblk), dim3(FLOOR_THREADS), 0, st,
                         (const T*)points, slice_offsets, n_slices, n_rows, g, ground, (unsigned long long*)hist);
    });
  };
  switch (copies) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_floor_hist(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long n_rows,
                   double half_length, double half_width, double ground_cell, int gx, int gy, const double* ground,
                   double band, double bin_width, int n_bins, long long* hist, int device, void* stream) {
  return floor_hist(FLOOR_COPIES, points, is_double, slice_offsets, n_slices, n_rows, half_length, half_width, ground_cell,
                    gx, gy, ground, band, bin_width, n_bins, hist, device, stream);
}
int prh_test_floor_hist(int copies, const void* points, int is_double, const long long* slice_offsets, int n_slices,
                        long long n_rows, double half_length, double half_width, double ground_cell, int gx, int gy,
                        const double* ground, double band, double bin_width, int n_bins, long long* hist, int device,
                        void* stream) {
  return floor_hist(copies, points, is_double, slice_offsets, n_slices, n_rows, half_length, half_width, ground_cell, gx, gy,
                    ground, band, bin_width, n_bins, hist, device, stream);
}
int prh_floor_otsu(const long long* hist, int n_rows, int n_bins, long long min_points, int* t_lo, int* t_hi, int* t,
                   long long* total, long long* above, long long* w0, long long* m0, long long* wr, long long* mr,
                   double* score, int device, void* stream) {
  if (n_rows < 0) return fail(PRH_ERR_ARG, "floor_otsu: bad argument");
  if (n_bins < 2 || n_bins > FLOOR_MAX_BINS) return fail(PRH_ERR_ARG, "floor_otsu: 2 <= n_bins <= %d", FLOOR_MAX_BINS);
  if (min_points < 1) return fail(PRH_ERR_ARG, "floor_otsu: min_points >= 1");
  if (n_rows == 0) return PRH_OK;
  if (!hist || !t_lo || !t_hi || !t || !total || !above || !w0 || !m0 || !wr || !mr || !score)
    return fail(PRH_ERR_ARG, "floor_otsu: null pointer");
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(floor_otsu_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, hist, n_bins, min_points,
                     t_lo, t_hi, t, total, above, w0, m0, wr, mr, score);
  LAUNCH_CHECK();
  return PRH_OK;
}

// ------------------------------------------------------------------ fused cross-attention
// small batches (B x H heads would occupy a fraction of the chip's wave slots) with long key
// ranges: up to eight waves per head, each a multiple of 32 keys
static bool attn_ksplit(int B, int H, int N, int& keys_per_wave) {
  keys_per_wave = 0;
  if ((long)B * H > 1024 || N < 128) return false;
  int nw = cdiv(N, 32) < 8 ? cdiv(N, 32) : 8;
  keys_per_wave = cdiv(cdiv(N, 32), nw) * 32;
  return true;
}
// dropout fields of a call, and the checks every attention launch needs
static int attn_prepare(AttnParams& a, float dropout_p) {
  a.seed_src = g_seed_src;
  if (dropout_p < 0.f || dropout_p >= 1.f) return fail(PRH_ERR_ARG, "attention: dropout_p must be in [0,1)");
  a.keep_scale = 1.f / (1.f - dropout_p);
  a.drop_thresh = dropout_p > 0.f ? (unsigned)((double)dropout_p * 4294967296.0) : 0u;
  if (!a.q || !a.k || !a.v || !a.o || !a.lse || a.B <= 0 || a.M <= 0 || a.N <= 0)
    return fail(PRH_ERR_ARG, "attention: bad argument");
  if (a.H <= 0 || a.H % 4) return fail(PRH_ERR_ARG, "attention: heads (%d) must be a multiple of 4", a.H);
  if ((a.ldq | a.ldk | a.ldv | a.ldo) & 3) return fail(PRH_ERR_ARG, "attention: leading dimensions must be multiples of 4");
  return PRH_OK;
}

// Launch code of the fp32 and the bf16 K / V entry points.  a: pointers, shapes, scale and seed of the
// call (kv16: K / V, and dK / dV, hold bf16 bits); prec: Cores::attn_prec() of the call.
static int attn_forward(AttnParams& a, bool kv16, int prec, float dropout_p, int device, hipStream_t st) {
  TRY(attn_prepare(a, dropout_p));
  HIP_TRY(hipSetDevice(device));
  const int B = a.B, M = a.M, N = a.N, H = a.H;
  ProfScope ps(prec < 0 ? "attn_fwd" : "attn16_fwd<split>",
               4.0 * B * H * (double)M * N * 32, 4.0 * (2.0 * B * N * H * 32 + 2.0 * B * M * H * 32), st);
  int wpb = (long)B * (H / 4) < 512 ? 1 : 4;      // one head per workgroup while the grid would not fill the chip
  if (kv16 && prec < 0) return fail(PRH_ERR_ARG, "attention: bf16 K/V need the 16-bit attention cores");
  unsigned grid = (unsigned)(B * (H / wpb));
  if (prec >= 0 && attn_ksplit(B, H, N, a.ksplit)) { wpb = cdiv(N, a.ksplit); grid = (unsigned)(B * H); }
  const size_t ldsf = (size_t)wpb * a16_fwd_wave_lds<0>();
  if (prec >= 0 && kv16)
    hipLaunchKernelGGL((attn16_fwd_kernel<0, true>), dim3(grid), dim3(64 * wpb), ldsf, st, a);
  else if (prec >= 0)
    hipLaunchKernelGGL(attn16_fwd_kernel<0>, dim3(grid), dim3(64 * wpb), ldsf, st, a);
  else
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(grid), dim3(64 * wpb), 0, st, a);
  LAUNCH_CHECK();
  return PRH_OK;
}

static int attn_backward(AttnParams& a, bool kv16, int prec, float dropout_p, int device, hipStream_t st) {
  TRY(attn_prepare(a, dropout_p));
  if (!a.dout || !a.dq || !a.dk || !a.dv) return fail(PRH_ERR_ARG, "attention_backward: null gradient pointer");
  if ((a.lddo | a.lddq | a.lddk | a.lddv) & 3) return fail(PRH_ERR_ARG, "attention_backward: leading dimensions must be multiples of 4");
  HIP_TRY(hipSetDevice(device));
  const int B = a.B, M = a.M, N = a.N, H = a.H;
  int wpb = (long)B * (H / 4) < 512 ? 1 : 4;
  if (prec >= 0) {
    unsigned grid = (unsigned)(B * (H / wpb));
    if (attn_ksplit(B, H, N, a.ksplit)) { wpb = cdiv(N, a.ksplit); grid = (unsigned)(B * H); }
    const size_t lds16 = (size_t)wpb * 4 * 2 * A16_IMG;
    static const int attr16 = allow_big_lds(attn16_bwd_kernel<0>, attn16_bwd_kernel<0, true>);
    if (attr16 != PRH_OK) return attr16;
    const double kvb = kv16 ? 2.0 : 4.0;
    ProfScope ps("attn16_bwd<split>", 14.0 * B * H * (double)M * N * 32,
                 kvb * 4.0 * B * N * H * 32 + 4.0 * 4.0 * B * M * H * 32, st);
    if (a.ksplit > 0) {
      static const int attr16s = allow_big_lds(attn16_bwd_kernel<0, false, true>, attn16_bwd_kernel<0, true, true>);
      if (attr16s != PRH_OK) return attr16s;
      if (kv16)
        hipLaunchKernelGGL((attn16_bwd_kernel<0, true, true>), dim3(grid), dim3(64 * wpb), lds16, st, a);
      else
        hipLaunchKernelGGL((attn16_bwd_kernel<0, false, true>), dim3(grid), dim3(64 * wpb), lds16, st, a);
    } else if (kv16)
      hipLaunchKernelGGL((attn16_bwd_kernel<0, true>), dim3(grid), dim3(64 * wpb), lds16, st, a);
    else
      hipLaunchKernelGGL(attn16_bwd_kernel<0>, dim3(grid), dim3(64 * wpb), lds16, st, a);
    LAUNCH_CHECK();
    return PRH_OK;
  }
  const size_t lds = (size_t)wpb * 4 * AT_TILE * sizeof(float);
  static const int attr_rc = allow_big_lds(attn_bwd_kernel);
  if (attr_rc != PRH_OK) return attr_rc;
  ProfScope ps("attn_bwd", 14.0 * B * H * (double)M * N * 32, 4.0 * (4.0 * B * N * H * 32 + 4.0 * B * M * H * 32), st);
  hipLaunchKernelGGL(attn_bwd_kernel, dim3((unsigned)(B * (H / wpb))), dim3(64 * wpb), lds, st, a);
  LAUNCH_CHECK();
  return PRH_OK;
}

int prh_attn_forward(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                     float* o, long ldo, float* lse, int B, int M, int N, int H, float scale,
                     float dropout_p, unsigned seed, int device, void* stream) {
  AttnParams a; memset(&a, 0, sizeof(a));
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.o = o; a.ldo = ldo; a.lse = lse;
  a.B = B; a.M = M; a.N = N; a.H = H; a.scale = scale; a.seed = seed;
  return attn_forward(a, false, cores_of(gemm_mode()).attn_prec(), dropout_p, device, (hipStream_t)stream);
}

int prh_attn_backward_ex(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                         const float* o, long ldo, const float* lse, const float* dout, long lddo,
                         float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, int B, int M,
                         int N, int H, float scale, float dropout_p, unsigned seed, float* kv_amax_part,
                         int device, void* stream) {
  AttnParams a; memset(&a, 0, sizeof(a));
  a.kv_amax_part = kv_amax_part;
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.o = (float*)o; a.ldo = ldo;
  a.lse = (float*)lse; a.dout = dout; a.lddo = lddo; a.dq = dq; a.lddq = lddq; a.dk = dk; a.lddk = lddk;
  a.dv = dv; a.lddv = lddv;
  a.B = B; a.M = M; a.N = N; a.H = H; a.scale = scale; a.seed = seed;
  return attn_backward(a, false, cores_of(gemm_mode()).attn_prec(), dropout_p, device, (hipStream_t)stream);
}
/* Inference-only cross-attention over the RAW memory rows with the layer's key / value projections
 * folded in (csrc/prh_attnfold.hpp).  prh_cast_perm_bf16: fp32 [rows, 256] (ld) -> the bf16 row image
 * the kernel reads (channels permuted inside groups of 16).  prh_attn_fold_forward: q [B*M, 256]
 * projected queries, x16 / y16 the images of memory + pos and of memory ([B*N, 256]), wk / wv / bv the
 * key and value rows of the layer's packed in_proj parameters; o [B*M, 256].  8 heads of 32, M <= 32. */
int prh_cast_perm_bf16(const float* src, long ld, uint16_t* dst, long rows, int device, void* stream) {
  if (!src || !dst || rows < 0 || ld < 256 || (ld & 3)) return fail(PRH_ERR_ARG, "cast_perm_bf16: bad argument");
  HIP_TRY(hipSetDevice(device));
  if (rows == 0) return PRH_OK;
  hipLaunchKernelGGL(cast_perm_b16_kernel, dim3((unsigned)cdiv(rows * 16, 256L)), dim3(256), 0, (hipStream_t)stream, src, ld,
                     dst, (size_t)rows);
  LAUNCH_CHECK();
  return PRH_OK;
}
/* Both row images of the folded attention from their sources in one pass (csrc/prh_attnfold.hpp):
 * x16 = bf16(memory + pos_emb(xyz)), y16 = bf16(memory) with pos_emb = Linear(3,256) + ReLU + Linear(256,256)
 * (src/model.py:64-75).  xyz rows are read in place (ld >= 3), memory [rows, 256] (ld >= 256, a multiple of 4:
 * the rows are read with 16-byte loads). */
int prh_posmem_images(const float* xyz, long ldx, const float* w0, const float* b0, const float* w2, const float* b2,
                      const float* memory, long ldm, long rows, uint16_t* x16, uint16_t* y16, int device, void* stream) {
  if (!xyz || !w0 || !w2 || !memory || !x16 || !y16 || rows < 0 || ldx < 3 || ldm < 256 || (ldm & 3))
    return fail(PRH_ERR_ARG, "posmem_images: bad argument");
  HIP_TRY(hipSetDevice(device));
  if (rows == 0) return PRH_OK;
  static const int attr = allow_big_lds(posmem_images_kernel);
  if (attr != PRH_OK) return attr;
  static const int n_cu = [] {
    int dev = 0, cu = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev);
    return cu > 0 ? cu : 256;
  }();
  const long tiles = (rows + 255) / 256;
  const unsigned grid = (unsigned)(tiles < n_cu ? tiles : n_cu);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("posmem_images", 2.0 * rows * 256.0 * 256.0, (double)rows * (16.0 + 1024.0 + 1024.0), st);
  hipLaunchKernelGGL(posmem_images_kernel, dim3(grid), dim3(512), PM_LDS, st, xyz, ldx, w0, b0, w2, b2, memory, ldm, rows,
                     x16, y16);
  LAUNCH_CHECK();
  return PRH_OK;
}
int prh_attn_fold_forward(const float* q, long ldq, const uint16_t* x16, const uint16_t* y16, const float* wk, long ldwk,
                          const float* wv, long ldwv, const float* bv, float* o, long ldo, int B, int M, int N, int H,
                          float scale, int device, void* stream) {
  if (!q || !x16 || !y16 || !wk || !wv || !bv || !o || B <= 0 || M <= 0 || N <= 0)
    return fail(PRH_ERR_ARG, "attn_fold_forward: bad argument");
  if (H != 8 || M > 32) return fail(PRH_ERR_ARG, "attn_fold_forward: built for 8 heads of 32 channels and M <= 32 (H=%d M=%d)", H, M);
  if ((ldq | ldo | ldwk | ldwv) & 3) return fail(PRH_ERR_ARG, "attn_fold_forward: leading dimensions must be multiples of 4");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = (hipStream_t)stream;
  AttnFoldParams a;
  a.q = q; a.ldq = ldq; a.x16 = x16; a.y16 = y16; a.wk = wk; a.ldwk = ldwk; a.wv = wv; a.ldwv = ldwv; a.bv = bv;
  a.o = o; a.ldo = ldo; a.B = B; a.M = M; a.N = N; a.H = H; a.scale = scale;
  static const int attr = allow_big_lds(attn_fold_fwd_kernel);
  if (attr != PRH_OK) return attr;
  ProfScope ps("attn_fold_fwd", 2.0 * 2.0 * B * H * 32.0 * N * 256, 2.0 * 2.0 * B * (double)N * 256, st);
  hipLaunchKernelGGL(attn_fold_fwd_kernel, dim3((unsigned)B), dim3(512), AF_LDS, st, a);
  LAUNCH_CHECK();
  return PRH_OK;
}
/* K / V (and dK / dV) in bf16 storage: bf16 mode's wide projection buffers (uint16_t = raw bf16 bits) */
int prh_attn_forward_kv16(const float* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv, float* o,
                          long ldo, float* lse, int B, int M, int N, int H, float scale, float dropout_p,
                          unsigned seed, int device, void* stream) {
  if ((ldk | ldv) & 7) return fail(PRH_ERR_ARG, "attention (bf16 K/V): leading dimensions must be multiples of 8");
  AttnParams a; memset(&a, 0, sizeof(a));
  a.q = q; a.ldq = ldq; a.k = reinterpret_cast<const float*>(k); a.ldk = ldk; a.v = reinterpret_cast<const float*>(v);
  a.ldv = ldv; a.o = o; a.ldo = ldo; a.lse = lse;
  a.B = B; a.M = M; a.N = N; a.H = H; a.scale = scale; a.seed = seed;
  return attn_forward(a, true, cores_of(gemm_mode()).attn_prec(), dropout_p, device, (hipStream_t)stream);
}
int prh_attn_backward_kv16(const float* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv,
                           const float* o, long ldo, const float* lse, const float* dout, long lddo, float* dq,
                           long lddq, uint16_t* dk, long lddk, uint16_t* dv, long lddv, int B, int M, int N, int H,
                           float scale, float dropout_p, unsigned seed, int device, void* stream) {
  if ((ldk | ldv | lddk | lddv) & 7) return fail(PRH_ERR_ARG, "attention (bf16 K/V): leading dimensions must be multiples of 8");
  const int prec = cores_of(gemm_mode()).attn_prec();
  if (prec < 0) return fail(PRH_ERR_ARG, "attention: bf16 K/V need the 16-bit attention cores");
  AttnParams a; memset(&a, 0, sizeof(a));
  a.q = q; a.ldq = ldq; a.k = reinterpret_cast<const float*>(k); a.ldk = ldk; a.v = reinterpret_cast<const float*>(v);
  a.ldv = ldv; a.o = (float*)o; a.ldo = ldo; a.lse = (float*)lse; a.dout = dout; a.lddo = lddo; a.dq = dq; a.lddq = lddq;
  a.dk = reinterpret_cast<float*>(dk); a.lddk = lddk; a.dv = reinterpret_cast<float*>(dv); a.lddv = lddv;
  a.B = B; a.M = M; a.N = N; a.H = H; a.scale = scale; a.seed = seed;
  return attn_backward(a, true, prec, dropout_p, device, (hipStream_t)stream);
}
int prh_attn_backward(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                      const float* o, long ldo, const float* lse, const float* dout, long lddo,
                      float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, int B, int M,
                      int N, int H, float scale, float dropout_p, unsigned seed, int device,
                      void* stream) {
  return prh_attn_backward_ex(q, ldq, k, ldk, v, ldv, o, ldo, lse, dout, lddo, dq, lddq, dk, lddk, dv, lddv, B, M, N,
                              H, scale, dropout_p, seed, nullptr, device, stream);
}

// ------------------------------------------------------------------ profiler
int prh_profile_enable(int capacity) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  for (auto& r : g_prof.recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_prof.recs.clear();
  g_prof.used = 0;
  g_prof.on = false;
  if (capacity <= 0) return PRH_OK;
  g_prof.recs.resize((size_t)capacity);
  for (auto& r : g_prof.recs) {
    HIP_TRY(hipEventCreate(&r.e0));
    HIP_TRY(hipEventCreate(&r.e1));
  }
  g_prof.on = true;
  return PRH_OK;
}
int prh_profile_count(void) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  return (int)g_prof.used;
}
int prh_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.used = 0;
  return PRH_OK;
}
int prh_profile_read(int i, char* name, int name_len, float* ms, double* flops, double* bytes) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (i < 0 || (size_t)i >= g_prof.used) return fail(PRH_ERR_ARG, "profile_read: index %d out of range", i);
  ProfRec& r = g_prof.recs[(size_t)i];
  HIP_TRY(hipEventSynchronize(r.e1));
  HIP_TRY(hipEventElapsedTime(ms, r.e0, r.e1));
  snprintf(name, (size_t)name_len, "%s", r.name);
  *flops = r.flops; *bytes = r.bytes;
  return PRH_OK;
}

// ------------------------------------------------------------------ raw cores for tests
int prh_test_gemm_nt(const float* a, const float* w, float* c, int m, int n, int k, void* workspace,
                     size_t workspace_bytes, int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  NTParams p; memset(&p, 0, sizeof(p));
  p.A = a; p.lda = k; p.W = w; p.ldw = k; p.C = c; p.ldc = n; p.M = m; p.N = n; p.K = k;
  if (workspace != nullptr && workspace_bytes >= s3_weight_bytes(n, k) + 256)
    p.wprep = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  return launch_nt<PRO_NONE, EPI_BIAS>(cores_of(gemm_mode()), p, (hipStream_t)stream);
}
size_t prh_test_gate_backward_workspace_bytes(int out_dim) { return s3_weight_bytes(out_dim, 64) + 512; }
int prh_test_gate_backward(const float* ctx, int B, int N, int in_channel, int out_dim, const float* gate_w1,
                           const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* z_fus,
                           const float* bn_scale, const float* bn_shift, float* d_fused, float* gate, int recompute,
                           float* ws_a, float* ws_b, void* workspace, size_t workspace_bytes, int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  if (!ctx || !gate_w1 || !gate_b1 || !gate_w2 || !gate_b2 || !z_fus || !bn_scale || !bn_shift || !d_fused || !gate ||
      !ws_a || !ws_b || B <= 0 || N <= 0 || in_channel < 4 || out_dim <= 0 || (long)B * N > 2000000000L)
    return fail(PRH_ERR_ARG, "test_gate_backward: bad argument");
  const Cores c = cores_of(gemm_mode());
  if (recompute && !gate_on_h2(c, B * N, out_dim, in_channel))
    return fail(PRH_ERR_ARG, "test_gate_backward: recompute without prh_encoder_gate_recompute()");
  if (workspace == nullptr || workspace_bytes < prh_test_gate_backward_workspace_bytes(out_dim))
    return fail(PRH_ERR_WORKSPACE, "test_gate_backward: workspace too small");
  char* wprep = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  return gate_combine_backward(c, ctx + 3, in_channel, B, N, out_dim, gate_w1, gate_b1, gate_w2, gate_b2, z_fus, bn_scale,
                               bn_shift, d_fused, nullptr, nullptr, gate, recompute, d_fused, ws_a, ws_b, wprep,
                               (hipStream_t)stream);
}
int prh_test_xcc_map(int blocks, int lds_bytes, int* out, int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  if (blocks <= 0 || lds_bytes < 0 || lds_bytes > 160 * 1024 || out == nullptr)
    return fail(PRH_ERR_ARG, "test_xcc_map: bad arguments");
  static const int attr_rc = allow_big_lds(xcc_probe_kernel);
  if (attr_rc != PRH_OK) return attr_rc;
  hipLaunchKernelGGL(xcc_probe_kernel, dim3((unsigned)blocks), dim3(512), (size_t)lds_bytes,
                     (hipStream_t)stream, out);
  LAUNCH_CHECK();
  return PRH_OK;
}
size_t prh_test_gemm_tn_workspace_bytes(int p, int mo, int ni) {
  const Cores c = cores_of(gemm_mode());
  Arena a;
  a.f(tn_slab_floats(c, p, mo, ni));
  a.f(tn_colsum_floats(c, p, mo, ni));
  return a.off + 256;
}
int prh_test_gemm_tn(const float* a, const float* b, float* c, float* colsum, int p, int mo, int ni,
                     void* workspace, size_t workspace_bytes, int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  const Cores cores = cores_of(gemm_mode());
  Arena ar(workspace, workspace_bytes);
  float* slab = ar.f(tn_slab_floats(cores, p, mo, ni));
  float* cs = ar.f(tn_colsum_floats(cores, p, mo, ni));
  if (!ar.ok) return fail(PRH_ERR_WORKSPACE, "test_gemm_tn: workspace too small");
  TNParams t; memset(&t, 0, sizeof(t));
  t.A = a; t.lda = mo; t.B = b; t.ldb = ni; t.P = p; t.Mo = mo; t.Ni = ni;
  return launch_tn<PRO_NONE, PRO_NONE>(cores, t, slab, cs, c, (long)ni, colsum, (hipStream_t)stream);
}
// The same raw wgrad with a BatchNorm-backward apply pass over dy [rows, cols]: side != 0, carried by
// the wgrad launch (an error where the transposed-read core does not serve it); side == 0, the
// stand-alone pass (materialize_dz) followed by the plain wgrad.  amax_out (device): max|dz|.
size_t prh_test_gemm_tn_side_workspace_bytes(int p, int mo, int ni) {
  return prh_test_gemm_tn_workspace_bytes(p, mo, ni) + (size_t)S3_HDR_FLOATS * sizeof(float) + 256;
}
int prh_test_gemm_tn_side(const float* a, const float* b, float* c, float* colsum, int p, int mo, int ni,
                          float* dy, long lddy, const float* z, long ldz, const float* ka, const float* kb,
                          const float* kc, long rows, int cols, int side, float* amax_out, void* workspace,
                          size_t workspace_bytes, int device, void* stream) {
  return prh_test_gemm_tn_side_ex(a, b, c, colsum, p, mo, ni, nullptr, nullptr, dy, lddy, z, ldz, ka, kb, kc, rows, cols,
                                  side, 0, nullptr, amax_out, workspace, workspace_bytes, device, stream);
}
// ... with BN+ReLU coefficients qa / qb [ni] on b (both or neither), and the side walk's period: 0 planned,
// 1 / 2 / 4 forced; *period_used (host, optional): the period the carrier ran with, 0 where nothing was carried.
int prh_test_gemm_tn_side_ex(const float* a, const float* b, float* c, float* colsum, int p, int mo, int ni,
                             const float* qa, const float* qb, float* dy, long lddy, const float* z, long ldz,
                             const float* ka, const float* kb, const float* kc, long rows, int cols, int side,
                             int period, int* period_used, float* amax_out, void* workspace, size_t workspace_bytes,
                             int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  if ((qa == nullptr) != (qb == nullptr)) return fail(PRH_ERR_ARG, "test_gemm_tn_side: qa and qb go together");
  if (period != 0 && period != 1 && period != 2 && period != 4)
    return fail(PRH_ERR_ARG, "test_gemm_tn_side: period %d (0, 1, 2 or 4)", period);
  if (period_used) *period_used = 0;
  if (!dy || !z || !ka || !kb || !kc || !amax_out || rows <= 0 || cols <= 0 || (cols & 3) || (lddy & 3) || (ldz & 3) ||
      lddy < cols || ldz < cols)
    return fail(PRH_ERR_ARG, "test_gemm_tn_side: bad side matrix");
  const Cores cores = cores_of(gemm_mode());
  hipStream_t st = (hipStream_t)stream;
  Arena ar(workspace, workspace_bytes);
  float* slab = ar.f(tn_slab_floats(cores, p, mo, ni));
  float* cs = ar.f(tn_colsum_floats(cores, p, mo, ni));
  float* hdr = ar.f(S3_HDR_FLOATS);
  if (!ar.ok) return fail(PRH_ERR_WORKSPACE, "test_gemm_tn_side: workspace too small");
  TNParams t; memset(&t, 0, sizeof(t));
  t.A = a; t.lda = mo; t.B = b; t.ldb = ni; t.P = p; t.Mo = mo; t.Ni = ni;
  if (side) {
    t.side.dy = dy; t.side.lddy = lddy; t.side.z = z; t.side.ldz = ldz; t.side.ka = ka; t.side.kb = kb; t.side.kc = kc;
    t.side.rows = rows; t.side.cols = cols; t.side.part = hdr + 64; t.side.amax = hdr; t.side.period = period;
  } else {
    TRY(materialize_dz(dy, lddy, z, ldz, ka, kb, kc, rows, cols, hdr, st));
  }
  if (qa != nullptr) {
    t.qa = qa; t.qb = qb;
    TRY((launch_tn<PRO_NONE, PRO_BNRELU>(cores, t, slab, cs, c, (long)ni, colsum, st)));
  } else {
    TRY((launch_tn<PRO_NONE, PRO_NONE>(cores, t, slab, cs, c, (long)ni, colsum, st)));
  }
  if (period_used) *period_used = t.side.period;
  HIP_TRY(hipMemcpyAsync(amax_out, hdr, sizeof(float), hipMemcpyDeviceToDevice, st));
  return PRH_OK;
}

// Raw second-stage reductions: device pointers in, through the launchers the library calls.
int prh_test_reduce_depth(int kind) {
  switch (kind) {
    case PRH_REDUCE_SLABS: return SLAB_D;
    case PRH_REDUCE_BN_STAGE1: return BN1_D;
    case PRH_REDUCE_PARTIALS: return PARTIALS_D;
    case PRH_REDUCE_LN_PARAM_GRAD: return LN_D;
    case PRH_REDUCE_FINAL: return FINAL_D;
    case PRH_REDUCE_ACT_AMAX: return AMAX_D;
    default: return 0;
  }
}
int prh_test_reduce_slabs(const float* slab, int s, int rows, int cols, float* out, long ldout, const float* cslab,
                          int ccols, float* cout, int device, void* stream) {
  if (!slab || !out || s < 1 || rows < 1 || cols < 1 || ldout < cols || (cslab != nullptr && (!cout || ccols < 1)))
    return fail(PRH_ERR_ARG, "test_reduce_slabs: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_slabs(slab, s, rows, cols, out, ldout, cslab, ccols, cout, (hipStream_t)stream);
}
int prh_test_reduce_bn_stage1(const float* ws_a, const float* ws_b, int r, long ld, int n, int tile_rows, int p,
                              int forward, double* out, int device, void* stream) {
  if (!ws_a || !ws_b || !out || r < 1 || n < 1 || ld < n || tile_rows < 1 || p < 1)
    return fail(PRH_ERR_ARG, "test_reduce_bn_stage1: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_bn_stage1(ws_a, ws_b, r, ld, n, tile_rows, p, forward, out, (hipStream_t)stream);
}
int prh_test_reduce_partials(const float* ws_a, const float* ws_b, int r2, int n, float* out_a, float* out_b,
                             int device, void* stream) {
  if (!ws_a || r2 < 1 || n < 1) return fail(PRH_ERR_ARG, "test_reduce_partials: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_partials(ws_a, ws_b, r2, n, out_a, out_b, (hipStream_t)stream);
}
int prh_test_reduce_ln_param_grad(const float* part_g, const float* part_b, int nb, float* dgamma, float* dbeta,
                                  int device, void* stream) {
  if (!part_g || !part_b || !dgamma || !dbeta || nb < 1) return fail(PRH_ERR_ARG, "test_reduce_ln_param_grad: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_ln_param_grad(part_g, part_b, nb, dgamma, dbeta, (hipStream_t)stream);
}
int prh_test_reduce_pos_hidden_final(const float* part, int nblk, int hidden, float* dw0, float* db0, int device,
                                     void* stream) {
  if (!part || nblk < 1 || hidden < 1) return fail(PRH_ERR_ARG, "test_reduce_pos_hidden_final: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_pos_hidden_final(part, nblk, hidden, dw0, db0, (hipStream_t)stream);
}
int prh_test_reduce_partial_rows_final(const float* part, int nblk, int n_el, float* out0, int n0, float* out1,
                                       int device, void* stream) {
  if (!part || nblk < 1 || n_el < 1 || n0 < 0 || n0 > n_el)
    return fail(PRH_ERR_ARG, "test_reduce_partial_rows_final: bad argument");
  HIP_TRY(hipSetDevice(device));
  return reduce_partial_rows_final(part, nblk, n_el, out0, n0, out1, (hipStream_t)stream);
}
size_t prh_test_reduce_act_amax_workspace_bytes(void) { return (size_t)ABSMAX_MAX_BLOCKS * sizeof(float) + 256; }
int prh_test_reduce_act_amax(const float* ws_c, const float* ws_d, int r, long ld, int n, const float* scale,
                             const float* shift, float* amax_out, void* workspace, size_t workspace_bytes, int device,
                             void* stream) {
  if (!ws_c || !ws_d || !scale || !shift || !amax_out || r < 1 || n < 1 || ld < n)
    return fail(PRH_ERR_ARG, "test_reduce_act_amax: bad argument");
  Arena ar(workspace, workspace_bytes);
  float* apart = ar.f(ABSMAX_MAX_BLOCKS);
  if (!ar.ok) return fail(PRH_ERR_WORKSPACE, "test_reduce_act_amax: workspace too small");
  HIP_TRY(hipSetDevice(device));
  return reduce_act_amax(ws_c, ws_d, r, ld, n, scale, shift, apart, amax_out, (hipStream_t)stream);
}

}  // extern "C"

#ifdef PRH_STAMP
// diagnostic build only: where the stamped kernel dumps its cycle accumulators (2 x 32 unsigned)
extern "C" int prh_debug_stamp_buffer(void* buf) {
  unsigned* b = reinterpret_cast<unsigned*>(buf);
  return hipMemcpyToSymbol(HIP_SYMBOL(prh::g_prh_stamp), &b, sizeof(b)) == hipSuccess ? 0 : -1;
}
#endif
