/* pointnet_refine_hip.h - C ABI of the MI355X (gfx950) LineRefineNet hot-path library.
 *
 * The reference (1pathplanningzzj/pointnet_refine) has no FFI or plugin interface:
 * its hot path is the Python nn.Module surface of src/model.py.  This library is the
 * native layer the replacement nn.Modules (pointnet_refine_amd/model.py) call through
 * ctypes.  Every entry point below names the reference code it replaces.
 *
 * Conventions
 *  - all tensors are fp32, POINT-MAJOR: rows = B*N points, columns = channels,
 *    row-major with the stated leading dimension;
 *  - every pointer is DEVICE memory owned by the caller (PyTorch); the library
 *    allocates nothing, keeps no pointer after return and launches only on `stream`;
 *  - return 0 on success, a negative code otherwise; prh_last_error() gives the text
 *    (thread-local);
 *  - re-entrant; the autograd engine calls the backward entry points from its own
 *    thread, so each call sets the device from `device` before launching.
 */
#ifndef POINTNET_REFINE_HIP_H
#define POINTNET_REFINE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRH_OK 0
#define PRH_ERR_ARG (-1)
#define PRH_ERR_WORKSPACE (-2)
#define PRH_ERR_HIP (-3)

#define PRH_MAX_LAYERS 8

/* One shared-MLP layer: 1x1 Conv1d (= Linear over points) + BatchNorm1d (+ ReLU).
 * Reference: nn.Conv1d/nn.BatchNorm1d pairs of src/model.py:10-20 (encoder),
 * :23-27 (fusion), :150-159 (point_mlp). */
typedef struct {
  const float* w;        /* [cout, cin]  (Conv1d weight (cout,cin,1) viewed 2-D) */
  const float* b;        /* [cout] */
  const float* gamma;    /* [cout] BatchNorm weight */
  const float* beta;     /* [cout] BatchNorm bias */
  float* running_mean;   /* [cout] updated in train mode */
  float* running_var;    /* [cout] updated in train mode (unbiased variance) */
  int64_t* num_batches_tracked; /* scalar, +1 in train mode; may be NULL */
  int cin, cout;
} prh_bn_layer;

/* Gradients of one shared-MLP layer (any pointer may be NULL = not wanted). */
typedef struct {
  float* dw;      /* [cout, cin] */
  float* db;      /* [cout] */
  float* dgamma;  /* [cout] */
  float* dbeta;   /* [cout] */
} prh_bn_layer_grad;

/* MultiScalePointNetEncoder parameters, src/model.py:7-37. */
typedef struct {
  int in_channel;          /* C (4 in LineRefineNet; any C>=4 for the bare encoder) */
  int out_dim;             /* 1024 */
  prh_bn_layer conv[5];    /* conv1..5 + bn1..5 */
  prh_bn_layer fusion;     /* fusion.0 (cin = 64+128+256+512+out_dim) + fusion.1 */
  const float* gate_w1;    /* intensity_gate.0.weight [64] (Conv1d(1,64,1)) */
  const float* gate_b1;    /* [64] */
  const float* gate_w2;    /* intensity_gate.2.weight [out_dim, 64] */
  const float* gate_b2;    /* [out_dim] */
} prh_encoder_params;

typedef struct {
  prh_bn_layer_grad conv[5];
  prh_bn_layer_grad fusion;
  float* d_gate_w1; float* d_gate_b1; float* d_gate_w2; float* d_gate_b2;
} prh_encoder_grads;

/* Activations the forward keeps for the backward (caller-allocated).
 *   cat = 64+128+256+512+out_dim                                            */
typedef struct {
  float* z_cat;      /* [P, cat]      pre-BN outputs of conv1..5, concatenated by column */
  float* z_fus;      /* [P, out_dim]  pre-BN output of the fusion conv */
  float* gate;       /* [P, out_dim]  0.5+0.5*sigmoid(.) ; may be NULL in the forward when no backward
                      * follows or when the backward computes it again (gate_recompute below) */
  float* bn_scale;   /* [cat+out_dim] gamma*rstd            (BN as y = z*scale+shift) */
  float* bn_shift;   /* [cat+out_dim] beta - mean*scale */
  float* bn_mean;    /* [cat+out_dim] */
  float* bn_rstd;    /* [cat+out_dim] */
  int32_t* argmax;   /* [B, out_dim]  first arg-max point of the max-pool; NULL = skip */
  float* op_amax;    /* [8] or NULL.  Training with the split-fp16 cores: the forward writes the
                      * largest activation of conv1..5 ([0..4]), their maximum ([5]) and an upper
                      * bound of max(fused) ([6]) here, taken from the statistics epilogues, and
                      * the backward reads them as operand scales of its wgrads instead of
                      * re-measuring.  Pass the same buffer to both calls
                      * (and keep the GEMM mode unchanged in between), or NULL to both. */
  int gate_recompute; /* prh_encoder_backward only (the forward ignores it).  0: `gate` holds the forward's
                      * gate.  1: `gate` is uninitialised scratch for dG - the backward runs the gate GEMM again
                      * and forms the gate in its epilogue, bit for bit the forward's; allowed only where
                      * prh_encoder_gate_recompute() returns 1 under the GEMM mode of the backward call
                      * (the forward may then have been called with gate = NULL).  Last field: callers
                      * that zero-initialise the struct keep the stored-gate path. */
} prh_encoder_saved;

/* 1 when prh_encoder_backward can compute the intensity gate again instead of reading a stored copy
 * (4 * out_dim bytes per point neither written by the forward nor read back): no pooled output / gradient
 * (want_global = 0) and, under the current GEMM mode, the gate launch of this shape runs on the
 * second-generation split-fp16 core with the vector epilogue (mode 3, out_dim % 4 == 0 and at least 32 tiles
 * of 256 x 256 with B*N >= 512).  0 otherwise: pass `gate` to the forward and leave gate_recompute 0. */
int prh_encoder_gate_recompute(int B, int N, int in_channel, int out_dim, int want_global);

/* Bytes of scratch the encoder entry points need for P = B*N points
 * (backward = 0: prh_encoder_forward only; 1: also prh_encoder_backward; 2: prh_encoder_backward with
 * d_fused_scratch = 1, which needs 4 * out_dim bytes per point less).  prh_encoder_forward and
 * prh_encoder_backward refuse a NULL workspace, and one smaller than this reports for their call, with
 * PRH_ERR_WORKSPACE before they touch the device. */
size_t prh_encoder_workspace_bytes(int B, int N, int in_channel, int out_dim, int backward);

/* MultiScalePointNetEncoder.forward, src/model.py:39-62.
 *   ctx      [B,N,C] point-major (the reference takes the (B,C,N) transpose view)
 *   fused    [B,N,out_dim]          (reference returns its (B,out_dim,N) transpose)
 *   gfeat    [B,2*out_dim] = [max over N | mean over N]; NULL = skip pooling
 *   training 1: batch statistics + running-stat update, 0: running statistics */
int prh_encoder_forward(const prh_encoder_params* prm, const float* ctx, int B, int N,
                        int training, float momentum, float eps,
                        float* fused, float* gfeat, const prh_encoder_saved* saved,
                        void* workspace, size_t workspace_bytes, int device, void* stream);

/* Backward of the above (autograd of src/model.py:39-62).
 *   d_fused [B,N,out_dim] or NULL, d_gfeat [B,2*out_dim] or NULL (at least one)
 *   d_ctx   [B,N,C] or NULL
 *   training must equal the forward's flag.
 * d_gfeat is read only; saved.gate is consumed (overwritten in place by dG; with saved.gate_recompute = 1 it
 * is only written).  d_fused is read only unless
 * d_fused_scratch = 1 (needs d_fused != NULL and d_gfeat == NULL - the path LineRefineNet takes): then the
 * library turns the caller's d_fused buffer into the fusion layer's gradient scratch (dy_f, then dz_f, in place)
 * instead of carving one from the workspace - 17 GB less at 4.19 M points; its content is undefined afterwards. */
int prh_encoder_backward(const prh_encoder_params* prm, const float* ctx, int B, int N,
                         int training, float* d_fused, const float* d_gfeat, int d_fused_scratch,
                         const prh_encoder_saved* saved, const prh_encoder_grads* grads,
                         float* d_ctx, void* workspace, size_t workspace_bytes, int device,
                         void* stream);

/* ---- bf16 mode (BASELINE config 3, "bf16 training"; prh_set_gemm_mode(4)) -----------------
 * Same encoder (src/model.py:39-62) with ONE bf16 MFMA product per MAC and the activations the
 * forward keeps - and `fused`, and the gradient buffers of the backward - STORED in bf16
 * (uint16_t = raw bf16 bits).  Accumulation, BatchNorm statistics (taken from the rounded
 * values), parameters and parameter gradients are fp32.  Channel widths must be multiples of 8
 * (the context rows are padded to 8 channels internally).
 *
 * The rounding contract: bf16() is round to nearest even (v_cvt_pk_bf16_f32) and is applied exactly
 * here; everything else is fp32 arithmetic.  tests/_encoder_ref.py states the same with store=bf16
 * and tests/test_encoder16_abi_gpu.py holds the two entry points to it.
 *   forward
 *     conv1, in_channel <= 8   z1 = bf16(b + W x): fp32 operands, fmaf chain in channel order
 *     conv1, in_channel > 8    x and W rounded to bf16, rows zero-padded to a multiple of 8 channels;
 *                              z1 = bf16(acc + b)
 *     conv2..5, fusion         A = bf16(relu(fmaf(z_prev, scale, shift))), W = bf16(W), z = bf16(acc + b)
 *     BatchNorm statistics     of the ROUNDED z; rstd, scale, shift and the running statistics as in
 *                              the fp32 contract
 *     gate                     u = bf16(relu(fmaf(intensity, w1, b1))), W2 = bf16(W2),
 *                              m = 0.5 + 0.5*sigmoid(acc + b2) in fp32; saved.gate = bf16(m);
 *                              fused = bf16(relu(fmaf(zf, s, t)) * m) with the UNROUNDED m
 *     pooling                  max and first arg-max over the bf16 `fused`; mean = fp32 sum / N
 *   backward
 *     combine step             d = d_fused (bf16) + d_gfeat's mean term / N + its max term at the arg-max;
 *                              dy_f = bf16(pre > 0 ? d*m : 0) with m = saved.gate as stored, sig = 2m - 1,
 *                              dG = bf16(d * relu(pre) * 0.5*sig*(1 - sig)) written over saved.gate;
 *                              the BatchNorm sums are taken from the rounded dy_f
 *     BatchNorm apply          dz = bf16(fmaf(ka, dy, fmaf(kb, z, kc))) in place; db comes from the two
 *                              sums (the sum of the UNROUNDED dz: analytically zero in training)
 *     wgrads                   operands: the bf16 dz and the bf16 prologue activations A of the forward;
 *                              fp32 slabs summed in fp64
 *     fusion dgrad             its block of dy_cat = bf16(mask(dz_f . bf16(W)))
 *     conv dgrads              accumulate, new = bf16(mask(old_bf16 + dz . bf16(W))); the sums for the
 *                              layer below are taken from the rounded result
 *     conv1                    dW from the fp32 ctx rows (in_channel <= 8) or the bf16 padded rows with
 *                              the pad columns dropped; d_ctx = dz_1 . bf16(W1), fp32
 *     gate part                the bf16 dG is the operand of both GEMMs (dW2 against the bf16 u);
 *                              dU = mask(dG . bf16(W2)) and what follows it are fp32
 * Shapes: d_ctx needs in_channel % 4 == 0, and out_dim <= 3008 (the fusion conv's K = 960 + out_dim
 * must fit the LDS image of its prologue coefficients).  Every shape either entry point cannot serve
 * is refused with PRH_ERR_ARG before the device is touched: nothing is written, saved.gate included. */
typedef struct {
  uint16_t* z_cat;   /* [P, cat]      bf16 pre-BN outputs of conv1..5 */
  uint16_t* z_fus;   /* [P, out_dim]  bf16 pre-BN output of the fusion conv */
  uint16_t* gate;    /* [P, out_dim]  bf16 0.5+0.5*sigmoid(.) ; may be NULL when no backward */
  float* bn_scale;   /* [cat+out_dim] as in prh_encoder_saved */
  float* bn_shift;
  float* bn_mean;
  float* bn_rstd;
  int32_t* argmax;   /* [B, out_dim] or NULL */
} prh_encoder_saved_bf16;
/* backward = 0: prh_encoder_forward_bf16 only; 1: also prh_encoder_backward_bf16.  A NULL workspace, or one smaller
 * than this reports, is refused (PRH_ERR_WORKSPACE) before the device is touched. */
size_t prh_encoder_bf16_workspace_bytes(int B, int N, int in_channel, int out_dim, int backward);
/* fused [B,N,out_dim] bf16; everything else as prh_encoder_forward */
int prh_encoder_forward_bf16(const prh_encoder_params* prm, const float* ctx, int B, int N, int training,
                             float momentum, float eps, uint16_t* fused, float* gfeat,
                             const prh_encoder_saved_bf16* saved, void* workspace, size_t workspace_bytes,
                             int device, void* stream);
/* d_fused [B,N,out_dim] bf16 or NULL; everything else as prh_encoder_backward */
int prh_encoder_backward_bf16(const prh_encoder_params* prm, const float* ctx, int B, int N, int training,
                              const uint16_t* d_fused, const float* d_gfeat, const prh_encoder_saved_bf16* saved,
                              const prh_encoder_grads* grads, float* d_ctx, void* workspace,
                              size_t workspace_bytes, int device, void* stream);
/* nn.Linear on a bf16 input (context_proj applied to the bf16 `fused`, src/model.py:147,194):
 * y fp32 [rows,n] = act(x W^T + b); backward: dy fp32 -> dx bf16 [rows,k], dw [n,k], db [n]
 * (any may be NULL).  k, n, ldx multiples of 8.  A workspace smaller than prh_linear_bf16_workspace_bytes
 * reports is refused (PRH_ERR_WORKSPACE), by these two and by the out16 / dy16 entries below. */
size_t prh_linear_bf16_workspace_bytes(int rows, int k, int n, int backward);
int prh_linear_forward_bf16(const uint16_t* x, long ldx, const float* w, const float* b, float* y, int rows, int k,
                            int n, int relu, void* workspace, size_t workspace_bytes, int device, void* stream);
int prh_linear_backward_bf16(const uint16_t* x, long ldx, const float* w, const float* dy, uint16_t* dx, float* dw,
                             float* db, int rows, int k, int n, void* workspace, size_t workspace_bytes, int device,
                             void* stream);

/* Inference-only cross-attention with the key / value projections folded in (src/model.py:119-128
 * in eval mode): attention over the RAW rows X = memory + pos and Y = memory, which
 * are the same for all six layers, instead of over per-layer projected buffers -
 *   softmax(Q_h K_h^T) V_h = softmax((Q_h Wk_h) X^T) Y Wv_h^T + bv_h
 * (the key bias is constant along the keys and drops out of the softmax).  prh_cast_perm_bf16 makes
 * the bf16 row image the kernel reads from fp32 [rows, 256] (ld >= 256); prh_attn_fold_forward:
 * q [B*M, 256] projected (unscaled) queries, wk / wv [256, 256] and bv [256] = rows d..2d and 2d..3d
 * of the layer's packed in_proj parameters, o [B*M, 256] (before out_proj).  8 heads of 32 channels,
 * M <= 32, bf16 products with fp32 accumulation (BASELINE config 5). */
int prh_cast_perm_bf16(const float* src, long ld, uint16_t* dst, long rows, int device, void* stream);
/* ... or both images in one pass from their sources: x16 = bf16(memory + pos), y16 = bf16(memory) with
 * pos = PositionalEncoding(xyz) = relu(xyz W0^T + b0) W2^T + b2 (src/model.py:64-75; W0 [256,3], W2 [256,256]).
 * The hidden layer and memory + pos never exist in fp32: 2 KB per point instead of 7 (pos_hidden, Linear
 * with residual, two casts).  xyz rows read in place (ld >= 3), memory [rows, 256] (ld >= 256 and a multiple of 4,
 * as for prh_cast_perm_bf16: the rows are read with 16-byte loads; anything else is refused with PRH_ERR_ARG).  A NULL
 * b0 or b2 is read as zero.  Every rounding, in order: h = bf16(relu(fma(z, w0z, fma(y, w0y, fma(x, w0x, b0))))) in fp32,
 * pos = bf16(W2) h accumulated in fp32, x16 = bf16((memory + pos) + b2), y16 = bf16(memory). */
int prh_posmem_images(const float* xyz, long ldx, const float* w0, const float* b0, const float* w2, const float* b2,
                      const float* memory, long ldm, long rows, uint16_t* x16, uint16_t* y16, int device, void* stream);
int prh_attn_fold_forward(const float* q, long ldq, const uint16_t* x16, const uint16_t* y16, const float* wk, long ldwk,
                          const float* wv, long ldwv, const float* bv, float* o, long ldo, int B, int M, int N, int H,
                          float scale, int device, void* stream);
/* bf16 mode, decoder side: the cross-attention key / value projections of all six layers
 * (src/model.py:123-126) write their [rows, 6*256] outputs in bf16 and receive bf16 gradients.
 *   prh_linear_forward_out16: y bf16 [rows,n] = x W^T + b from an fp32 x;
 *   prh_linear_backward_dy16: dy bf16 -> dx fp32 [rows,k], dw [n,k], db [n] (any may be NULL);
 *   workspace: prh_linear_bf16_workspace_bytes(rows, k, n, backward).
 *   prh_attn_forward_kv16 / prh_attn_backward_kv16: prh_attn_forward / prh_attn_backward with K, V
 *   (and dK, dV) in bf16 storage - leading dimensions in elements, multiples of 8. */
int prh_linear_forward_out16(const float* x, long ldx, const float* w, const float* b, uint16_t* y, int rows, int k,
                             int n, void* workspace, size_t workspace_bytes, int device, void* stream);
int prh_linear_backward_dy16(const float* x, long ldx, const float* w, const uint16_t* dy, float* dx, float* dw,
                             float* db, int rows, int k, int n, void* workspace, size_t workspace_bytes, int device,
                             void* stream);
int prh_attn_forward_kv16(const float* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv, float* o,
                          long ldo, float* lse, int B, int M, int N, int H, float scale, float dropout_p,
                          unsigned seed, int device, void* stream);
int prh_attn_backward_kv16(const float* q, long ldq, const uint16_t* k, long ldk, const uint16_t* v, long ldv,
                           const float* o, long ldo, const float* lse, const float* dout, long lddo, float* dq,
                           long lddq, uint16_t* dk, long lddk, uint16_t* dv, long lddv, int B, int M, int N, int H,
                           float scale, float dropout_p, unsigned seed, int device, void* stream);

/* ---- fused EVAL-mode encoder (src/model.py:39-62 with every BatchNorm in eval mode, + :147,194)
 * One kernel takes context [B,N,C] to memory [B,N,256] = context_proj(fused) - and, optionally,
 * fused [B,N,1024] and global_feat [B,2048] - with BatchNorm folded into the conv weights: a
 * tile of points stays resident on the CU, the weights stream from L2, no activation touches
 * HBM.  planes = 1: fp16 operands (BASELINE config 5, "batched fp16 forward"; parity gate 5e-2);
 * planes = 2: two fp16 planes, three MFMA products, fp32-level error (parity gate 1e-4).
 * Built for the reference's widths (64/128/256/512/1024, gate hidden 64, context_proj 256).
 *   prepare: fold + split the weights ONCE per set of weights into `image`
 *            (prh_encoder_fused_image_bytes bytes, 256-byte aligned); proj_w/proj_b [256,1024]/[256]
 *            or NULL (encoder API only);
 *   forward: any of memory / fused / gfeat may be NULL (at least one given); workspace
 *            (prh_encoder_fused_workspace_bytes) is needed for gfeat only.  Activations travel between
 *            the layers as fp16 planes: `saturated` (device word, may be NULL) is INCREMENTED for every
 *            group of four activations holding a value above 65504 (clamped) - a non-zero count means
 *            the result is not the module's and must be discarded (the caller zeroes the word). */
size_t prh_encoder_fused_image_bytes(int planes, int in_channel);
int prh_encoder_fused_prepare(const prh_encoder_params* prm, float eps, const float* proj_w, const float* proj_b,
                              int planes, void* image, size_t image_bytes, int device, void* stream);
size_t prh_encoder_fused_workspace_bytes(int B, int N, int planes);
int prh_encoder_fused_forward(const void* image, int planes, int in_channel, int has_proj, const float* ctx, int B,
                              int N, float* memory, float* fused, float* gfeat, unsigned* saturated, void* workspace,
                              size_t workspace_bytes, int device, void* stream);

/* nn.Linear forward y = act(x W^T + b): context_proj (src/model.py:147,194) and any
 * other Linear on the path.  x [rows,k] (ld ldx), w [n,k], y [rows,n]; relu: 0/1.
 * k and ldx must be multiples of 4.  workspace (may be NULL: exact fp32 MFMA core only) holds the
 * split weight image (and the operand-scale words) of the large-GEMM cores. */
size_t prh_linear_forward_workspace_bytes(int rows, int k, int n);
int prh_linear_forward(const float* x, long ldx, const float* w, const float* b, float* y,
                       int rows, int k, int n, int relu, void* workspace, size_t workspace_bytes,
                       int device, void* stream);

/* Same with a caller-supplied device scalar x_amax >= max|x| (NULL = measured by a read pass when
 * the split-fp16 core serves the GEMM): e.g. prh_encoder_saved.op_amax[6] for context_proj. */
int prh_linear_forward_ex(const float* x, long ldx, const float* w, const float* b, float* y,
                          int rows, int k, int n, int relu, const float* x_amax, void* workspace,
                          size_t workspace_bytes, int device, void* stream);

/* Same plus an optional residual input added in the GEMM epilogue: y = act(x W^T + b + resid),
 * resid [rows,n] (ld ldres; NULL = none) - e.g. k-input = memory + pos_emb(xyz)
 * (src/model.py:123-126) with the addition riding on the second Linear of the
 * positional-encoding MLP - and an optional device scalar w_amax = max|w|. */
int prh_linear_forward_full(const float* x, long ldx, const float* w, const float* b, const float* resid,
                            long ldres, float* y, int rows, int k, int n, int relu, const float* x_amax,
                            const float* w_amax, float dropout_p, unsigned dropout_seed, void* workspace,
                            size_t workspace_bytes, int device, void* stream);
/* dropout_p > 0: y = dropout(act(x W^T + b + resid)) with the keep decision a counter hash of
 * (dropout_seed, row, column) and survivors scaled by 1 / (1 - p) - the FFN hidden layer of the decoder
 * (src/model.py:131) leaves the GEMM epilogue already dropped out; no mask tensor exists, the backward
 * reads the decision off the output (prh_relu_mask_absmax with scale = 1 / (1 - p)). */

/* Same plus the output's largest magnitude as a by-product: y_amax_out[0] = max|y| over exactly the elements
 * written (after bias, residual, ReLU and dropout; a NaN is dropped as by fmaxf, rows = 0 gives 0) - the x_amax
 * of the GEMM that reads y next, without a read pass over y.  On the second-generation split-fp16 core (GEMM
 * mode 3, large 16-B aligned shapes) the maximum comes out of the GEMM epilogue plus one tiny reduction
 * launch; every other core measures y after the GEMM, so the value is valid on return either way.
 * y_amax_out NULL: exactly prh_linear_forward_full.  Otherwise the workspace is required
 * (prh_linear_forward_workspace_bytes). */
int prh_linear_forward_amax(const float* x, long ldx, const float* w, const float* b, const float* resid,
                            long ldres, float* y, int rows, int k, int n, int relu, const float* x_amax,
                            const float* w_amax, float dropout_p, unsigned dropout_seed, float* y_amax_out,
                            void* workspace, size_t workspace_bytes, int device, void* stream);

/* Operand maxima for the split-fp16 cores, measured once by the caller and handed to every GEMM
 * that reads the operand (x_amax / w_amax / dy_amax arguments; NULL = the launch measures it):
 * out[0] = max |x| over [rows, cols] (ld >= cols).  prh_linear_uses_operand_maxima: 1 when a
 * Linear of this shape runs on those cores in the current GEMM mode (otherwise the maxima are
 * not read and need not be measured). */
size_t prh_operand_absmax_workspace_bytes(void);
int prh_operand_absmax(const float* x, long ld, long rows, int cols, float* out, void* workspace,
                       size_t workspace_bytes, int device, void* stream);
/* ReLU backward of a Linear with the ReLU fused into its epilogue (src/model.py:131 linear1 +
 * activation; :162-166 reg_branches): out = y > 0 ? dy : 0 and amax_out[0] = max|out| (the operand
 * maximum of the split-fp16 backward GEMMs) in one pass.  n elements, n % 4 == 0, contiguous.
 * Workspace: prh_operand_absmax_workspace_bytes(). */
int prh_relu_mask_absmax(const float* dy, const float* y, float* out, long n, float scale, float* amax_out,
                         void* workspace, size_t workspace_bytes, int device, void* stream);
/* scale: 1 for a plain ReLU; 1 / (1 - p) when y came out of a ReLU + dropout epilogue (out = y > 0 ? dy * scale : 0). */
int prh_linear_uses_operand_maxima(int rows, int k, int n);

/* First layer of the positional-encoding MLP (src/model.py:64-75, nn.Linear(3, hidden) + ReLU)
 * as one elementwise pass: h[r,c] = relu(b0[c] + sum_j xyz[r*ld + j] w0[c*3 + j]), j < 3.
 * xyz rows are read in place with leading dimension ld >= 3 (ld = C for (B,N,C) context rows);
 * hidden: a power of two in [4, 1024].  backward: dw0 [hidden,3] and db0 [hidden] (either may be
 * NULL) from dh [rows,hidden] masked by h > 0; dxyz [rows,3] (contiguous; NULL = skip; needs w0
 * and hidden <= 256) for the decoder's query positions, which carry gradients. */
int prh_pos_hidden_forward(const float* xyz, long ld, const float* w0, const float* b0, float* h,
                           long rows, int hidden, int device, void* stream);
/* ... with h_amax_out[0] = max h (h >= 0) from the same pass plus one tiny reduction launch (NULL: exactly
 * prh_pos_hidden_forward, no workspace needed). */
size_t prh_pos_hidden_forward_workspace_bytes(void);
int prh_pos_hidden_forward_amax(const float* xyz, long ld, const float* w0, const float* b0, float* h,
                                long rows, int hidden, float* h_amax_out, void* workspace, size_t workspace_bytes,
                                int device, void* stream);
size_t prh_pos_hidden_backward_workspace_bytes(long rows, int hidden);
int prh_pos_hidden_backward(const float* xyz, long ld, const float* h, const float* dh, const float* w0,
                            float* dxyz, float* dw0, float* db0, long rows, int hidden, void* workspace,
                            size_t workspace_bytes, int device, void* stream);

/* nn.Linear with n <= 4 outputs as one HBM pass (the regression heads' Linear(128, 3),
 * src/model.py:162-166): y [rows,n] = x [rows,k] w[n,k]^T + b.  k/4 must be a power of two
 * <= 64 (k = 4 ... 256); x, y, dx contiguous.  backward: dx (NULL = skip), dw [n,k], db [n]
 * (either may be NULL). */
int prh_linear_small_forward(const float* x, const float* w, const float* b, float* y, long rows, int k,
                             int n, int device, void* stream);
size_t prh_linear_small_backward_workspace_bytes(long rows, int k, int n);
int prh_linear_small_backward(const float* x, const float* w, const float* dy, float* dx, float* dw,
                              float* db, long rows, int k, int n, void* workspace, size_t workspace_bytes,
                              int device, void* stream);

/* nn.Linear backward: dx = dy W (NULL = skip), dw = dy^T x, db = colsum(dy).
 * n and k multiples of 4. */
size_t prh_linear_backward_workspace_bytes(int rows, int k, int n);
int prh_linear_backward(const float* x, long ldx, const float* w, const float* dy, float* dx,
                        float* dw, float* db, int rows, int k, int n, void* workspace,
                        size_t workspace_bytes, int device, void* stream);

/* x_amax, dy_amax: optional device scalars bounding max|x| / max|dy| from above (NULL = measured) */
int prh_linear_backward_ex(const float* x, long ldx, const float* w, const float* dy, float* dx,
                           float* dw, float* db, int rows, int k, int n, const float* x_amax,
                           const float* dy_amax, void* workspace, size_t workspace_bytes, int device,
                           void* stream);
/* ... and w_amax = max|w| (the dgrad reads W^T, whose maximum is the same) */
int prh_linear_backward_full(const float* x, long ldx, const float* w, const float* dy, float* dx,
                             float* dw, float* db, int rows, int k, int n, const float* x_amax,
                             const float* dy_amax, const float* w_amax, void* workspace,
                             size_t workspace_bytes, int device, void* stream);
/* ... dx_accumulate != 0: dx += dy W (dx holds the addend on entry: the gradient fan-in of a tensor two
 * Linears read is summed in the second one's dgrad epilogue, one fp32 addition per element, instead of a
 * separate add pass), and dx_amax_out[0] = max|dx| of what dx holds afterwards (NULL = not wanted; produced
 * by the epilogue or measured, as in prh_linear_forward_amax).  Both off: exactly prh_linear_backward_full. */
int prh_linear_backward_amax(const float* x, long ldx, const float* w, const float* dy, float* dx,
                             float* dw, float* db, int rows, int k, int n, const float* x_amax,
                             const float* dy_amax, const float* w_amax, int dx_accumulate, float* dx_amax_out,
                             void* workspace, size_t workspace_bytes, int device, void* stream);

/* Stack of <= PRH_MAX_LAYERS shared-MLP layers applied to x [P,cin0]:
 * LineRefineNet.point_mlp, src/model.py:150-159,200-201 (relu_last = 0).
 *   z_cat [P, sum(cout)] pre-BN outputs (kept for backward), y [P, cout_last].
 * A workspace that is NULL or smaller than prh_mlp_stack_workspace_bytes reports is refused
 * (PRH_ERR_WORKSPACE) by both entry points. */
size_t prh_mlp_stack_workspace_bytes(int P, int n_layers, const prh_bn_layer* layers);
int prh_mlp_stack_forward(const prh_bn_layer* layers, int n_layers, int relu_last,
                          const float* x, int P, int training, float momentum, float eps,
                          float* z_cat, float* y, float* bn_scale, float* bn_shift,
                          float* bn_mean, float* bn_rstd, void* workspace,
                          size_t workspace_bytes, int device, void* stream);
int prh_mlp_stack_backward(const prh_bn_layer* layers, int n_layers, int relu_last,
                           const float* x, int P, int training, const float* dy,
                           const float* z_cat, const float* bn_scale, const float* bn_shift,
                           const float* bn_mean, const float* bn_rstd,
                           const prh_bn_layer_grad* grads, float* dx, void* workspace,
                           size_t workspace_bytes, int device, void* stream);

/* Fused cross-attention core of DetrTransformerDecoderLayer.cross_attn (src/model.py:84,123-126:
 * nn.MultiheadAttention(256, 8 heads, dropout on the attention weights), everything between
 * the in-projections and the out-projection): o = dropout(softmax(q k^T * scale)) v per head
 * of 32 channels, exact fp32 MFMA, online softmax.
 *   q [B*M, H*32] (ld ldq), k/v [B*N, H*32] (ld ldk/ldv: may be column blocks of a wider
 *   projection buffer), o [B*M, H*32], lse [B,H,M] (kept for the backward).
 * dropout_p = 0 in eval mode; the mask is a counter-based hash of (seed, b, h, query, key). */
int prh_attn_forward(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                     float* o, long ldo, float* lse, int B, int M, int N, int H, float scale,
                     float dropout_p, unsigned seed, int device, void* stream);
int prh_attn_backward(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                      const float* o, long ldo, const float* lse, const float* dout, long lddo,
                      float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, int B, int M,
                      int N, int H, float scale, float dropout_p, unsigned seed, int device,
                      void* stream);

/* Per-line context builder: the crop / weight / sample / centre step of
 * LaneRefineDataset.__getitem__ (src/dataset.py:210-234) and process_single_line
 * (inference_whole_scene.py:98-121), weighted_sampling (src/dataset.py:78-130), batched over the
 * lines of one scene.
 *   cloud  [npts,4] xyz + intensity          dense [n_lines,n_dense,3] polyline resampled to
 *   line   [n_lines,m,3] resampled to m pts        n_dense points (200 in the reference)
 *   out    [n_lines,n_samples,4] xyz centred on the line's mean, raw intensity
 *   counts [n_lines] points inside the tube (before the max_candidates cap)
 *   dbg_weights [n_lines,max_candidates] or NULL: unnormalised sampling weights of the
 *               candidates in cloud order (lines with counts > n_samples only)
 * Crop masks and weights match the reference to fp32 rounding; the draws replace
 * numpy.random.choice by hashing (seed, line, point index): same distribution, not the same
 * sample.  Deterministic for a given seed.  Lines with more than max_candidates points in the
 * tube use the first max_candidates in cloud order (counts still reports the true number). */
size_t prh_context_workspace_bytes(int npts, int n_lines, int max_candidates);
int prh_context_build(const float* cloud, int npts, const float* dense, int n_dense, const float* line,
                      int m, int n_lines, float radius, float decay_scale, int n_samples,
                      int max_candidates, unsigned long long seed, float* out, int32_t* counts,
                      float* dbg_weights, void* workspace, size_t workspace_bytes, int device,
                      void* stream);

/* Ragged context builder: the contexts of the lines of MANY slices (a drive's slices, a detector
 * run's frames) in one pass.  Every line is cropped from its own slice; per line the arithmetic and
 * its order are those of prh_context_build, so the bytes of out and counts equal a
 * prh_context_build call per slice (with that slice's seed and a candidate buffer large enough).
 *   points        [T,4] device: the slices back to back, T < 2^31
 *   slice_offsets [n_slices+1] HOST: slice s is rows slice_offsets[s] .. slice_offsets[s+1]; starts at
 *                 0 and never decreases (a slice may be empty: its lines get counts 0, zero contexts)
 *   dense [n_lines,n_dense,3], line [n_lines,m,3] device, as in prh_context_build
 *   line_slice    [n_lines] HOST: the slice of each line, never decreasing (lines grouped by slice)
 *   slice_seed    [n_slices] HOST: one seed per slice
 * Index convention of the hash: a line's index is its position among the lines of its own slice
 * (the first line of every slice is line 0), a point's index is its row relative to
 * slice_offsets[s] - what a per-slice prh_context_build call uses, so the draws coincide.
 * Work items are (line, 256-point block of the line's slice) on a flat 1-D grid: their number, the
 * sum over the lines of ceil(slice points / 256), must stay below 2^31; n_lines itself is only
 * bounded by that.
 * prh_context_ragged_count: counts [n_lines] points inside each tube and cand_offsets [n_lines+1]
 *   (device, int64) their exclusive scan; the caller reads cand_offsets[n_lines] (or the whole
 *   array) and sizes the candidate buffers.  It also leaves the per-line tables and per-block
 *   counts in the workspace: prh_context_ragged_select must get the same workspace, untouched, and
 *   the same host arrays.
 * prh_context_ragged_select: fills and draws the lines line0 .. line1-1 (any run; the runs of a
 *   call sequence may reuse cand / keys).  cand (int32, slice-local rows in cloud order) and keys
 *   (uint32; the weights share it) hold cand_capacity entries each, at least
 *   cand_offsets[line1] - cand_offsets[line0]: no cap, no truncation (a shorter buffer is never
 *   written past its end: the lines that do not fit are drawn from what fits).  Writes
 *   out [n_lines,n_samples,4] rows of the run.
 * prh_context_ragged_workspace_bytes: n_items is that number of work items; 0 for n_lines <= 0 or
 *   n_items outside 0 .. 2^31 - 1.  The entry points recompute n_items from the host arrays and
 *   refuse a workspace that is too small. */
size_t prh_context_ragged_workspace_bytes(int n_lines, long long n_items);
int prh_context_ragged_count(const float* points, const long long* slice_offsets, int n_slices, const float* dense,
                             int n_dense, const int* line_slice, const unsigned long long* slice_seed, int n_lines,
                             float radius, int32_t* counts, long long* cand_offsets, void* workspace,
                             size_t workspace_bytes, int device, void* stream);
int prh_context_ragged_select(const float* points, const long long* slice_offsets, int n_slices, const float* dense,
                              int n_dense, const float* line, int m, const int* line_slice, int n_lines, float radius,
                              float decay_scale, int n_samples, const int32_t* counts, const long long* cand_offsets,
                              int line0, int line1, int* cand, unsigned* keys, long long cand_capacity, float* out,
                              void* workspace, size_t workspace_bytes, int device, void* stream);

/* Scene evaluation (inference_whole_scene.py:26-92,299-365), fp64 throughout, FMA contraction off,
 * distances as sqrt((dx*dx + dy*dy) + dz*dz) - the numpy order - so results match the
 * reference's float64 numpy / scipy code to rounding even at UTM-sized coordinates.
 * Per line (one wave each):
 *   noisy, refined [n_lines,m,3] (m = 2..128; noisy is the resampled line the crop is matched to)
 *   gt [*,3] ground-truth polylines as CSR with gt_offsets [n_gt+1] (int64);
 *   gt_index [n_lines] polyline of each line, -1 = none
 *   info [n_lines,4] int32: crop_start, crop_end, reversed, valid (crop_gt_to_pred_range, :26-70;
 *        argmin ties to the first index)
 *   resampled [n_lines,m,3] the crop resampled to m points (src/dataset.py:8-29)
 *   metrics [n_lines,6]: ade_noisy, ade_refined, cd_noisy, cd_refined, lat_noisy, lat_refined
 *        (ADE against the resample; Chamfer and lat = mean line->crop nearest distance against
 *        the crop vertices, compute_chamfer_distance :72-92)
 * Lines whose polyline has fewer than 2 vertices (or index -1) get valid = 0, crop -1/-1, a
 * zero resample and NaN metrics. */
int prh_line_metrics(const double* noisy, const double* refined, int n_lines, int m, const double* gt,
                     const long long* gt_offsets, int n_gt, const int* gt_index, int* info, double* resampled,
                     double* metrics, int device, void* stream);
/* Alignment sweep (calibrate_alignment's inner loop, :170-193) for n_shifts shifts in one call:
 *   out[s] = mean_p min_g |pred_p + (dx_s, dy_s, 0) - gt_g|,  pred [n_pred,3], gt [n_gt,3],
 *   shifts [n_shifts,2] (dx, dy), out [n_shifts], all fp64.  Brute force over gt; per-block
 * partial sums reduced in a fixed order: bitwise identical from run to run. */
size_t prh_shift_sweep_workspace_bytes(int n_pred, int n_gt, int n_shifts);
int prh_shift_sweep(const double* pred, int n_pred, const double* gt, int n_gt, const double* shifts, int n_shifts,
                    double* out, void* workspace, size_t workspace_bytes, int device, void* stream);

/* Ragged alignment sweep: n_problems independent prh_shift_sweep problems in one launch pair.
 *   pred [*,3], shifts [*,2], out [*] are flat fp64 device buffers; problem p owns the rows
 *   pred_offsets[p] .. pred_offsets[p+1] of pred and shift_offsets[p] .. shift_offsets[p+1] of
 *   shifts and out.  gt [*,3] holds n_gt_sets point sets cut by gt_offsets [n_gt_sets+1]; problem p
 *   measures against set gt_index[p], so problems may share a set.  All offset and index arrays
 *   are HOST arrays (int64 offsets starting at 0, int32 indices): the call checks them, uploads a
 *   per-problem table and synchronises the stream once before it launches.
 *   out[shift_offsets[p] + s] = mean_q min_g |pred_q + (dx_s, dy_s, 0) - gt_g| over p's rows.
 * Bitwise equal to one prh_shift_sweep call per problem: both run the same block routine (256
 * queries x 16 shifts, tiles counted from the problem's own first point and shift) and the same
 * in-order reduction of the block partials, in fp64 without contraction.
 * Work items (problem, query tile, shift tile) form a flat 1-D grid: at most 2^31 - 1 items per
 * call and fewer than 2^31 points, GT points and shifts per problem; no other per-problem limit.
 * PRH_ERR_ARG for a problem without a prediction point, a GT point or a shift and for a GT index
 * out of range; PRH_ERR_WORKSPACE below ..._workspace_bytes (0 there means the arrays are refused). */
size_t prh_shift_sweep_ragged_workspace_bytes(const long long* pred_offsets, const long long* shift_offsets,
                                              int n_problems);
int prh_shift_sweep_ragged(const double* pred, const long long* pred_offsets, const double* gt,
                           const long long* gt_offsets, int n_gt_sets, const int* gt_index, const double* shifts,
                           const long long* shift_offsets, int n_problems, double* out, void* workspace,
                           size_t workspace_bytes, int device, void* stream);

/* Drive slicing (tools/generate_train_data.py:134-182,247-273; tools/augment_train_data.py:18-54).
 * poses [n_slices,7] fp64 = x y z qx qy qz qw (the quaternion is normalised).  A point of cloud
 * [npts,4] float32 belongs to slice s when, in float32 with every operation rounded separately,
 * (x - f32(pose.x))^2 + (y - f32(pose.y))^2 < f32(radius^2), and its fp64 local x (inverse
 * rotation of xyz - pose.xyz) lies in [-segment_len/2, segment_len/2].
 *   prh_drive_slice_count  offsets [n_slices+1] int64: slice s owns rows offsets[s]..offsets[s+1]
 *   prh_drive_slice_write  points [capacity,4] fp64 local xyz + the untouched intensity, in cloud
 *                          order inside each slice; source_index [capacity] int64 cloud row of
 *                          each emitted point.  Needs the SAME arguments, offsets and workspace
 *                          (contents untouched) as the count call before it, and capacity >=
 *                          offsets[n_slices]; rows beyond capacity are never written.
 * No atomics: bitwise identical from run to run.  n_slices = 0 or npts = 0 give zero offsets. */
size_t prh_drive_slice_workspace_bytes(int npts, int n_slices);
int prh_drive_slice_count(const float* cloud, int npts, const double* poses, int n_slices, double segment_len,
                          double radius, long long* offsets, void* workspace, size_t workspace_bytes, int device,
                          void* stream);
int prh_drive_slice_write(const float* cloud, int npts, const double* poses, int n_slices, double segment_len,
                          double radius, const long long* offsets, double* points, long long* source_index,
                          long long capacity, void* workspace, size_t workspace_bytes, int device, void* stream);
/* clip_polyline_by_x (:145-182) of every polyline in every slice frame, fp64, one thread per
 * (slice, line).  lines [*,3] with CSR line_offsets [n_lines+1] (int64).
 *   prh_drive_clip_count  counts [n_slices*n_lines] int32: output vertices of pair s*n_lines + l
 *                         (0- and 1-vertex inputs as the reference; the caller keeps counts > 1)
 *   prh_drive_clip_write  out [*,3] at 3 * out_offsets[pair] (int64 exclusive prefix of counts) */
size_t prh_drive_clip_workspace_bytes(int n_slices);
int prh_drive_clip_count(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_slices, double segment_len, int* counts, void* workspace, size_t workspace_bytes,
                         int device, void* stream);
int prh_drive_clip_write(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_slices, double segment_len, const long long* out_offsets, double* out,
                         void* workspace, size_t workspace_bytes, int device, void* stream);
/* generate_noisy_line (augment_train_data.py:18-54) for n_scales (1..8) candidates of every line:
 *   out [n_scales,n_verts,3] = (p - centroid) @ R(yaw).T + centroid + shift + jitter, fp64.
 * lines [n_verts,3] with CSR line_offsets [n_lines+1]; vertex_line [n_verts] int32 line of each
 * vertex.  draw != 0: yaw ~ U(+-5 deg * s) (stored in rad), dx, dy ~ U(+-s), dz ~ U(+-0.1),
 * jitter ~ N(0, 0.05 / 0.05 / 0.025) from a counter hash of (seed, line id, candidate, vertex,
 * component) - line id = line_ids[l], or l when line_ids is NULL - written to draws_u
 * [n_lines,n_scales,4] and draws_j [n_scales,n_verts,3]; draw == 0: both are inputs and scales
 * and seed are ignored.  Same distribution as numpy's generator, not the same numbers. */
size_t prh_drive_noise_workspace_bytes(int n_lines);
int prh_drive_noise(const double* lines, const long long* line_offsets, const int* vertex_line, long long n_verts,
                    int n_lines, const int* line_ids, const double* scales, int n_scales, unsigned long long seed,
                    int draw, double* draws_u, double* draws_j, double* out, void* workspace,
                    size_t workspace_bytes, int device, void* stream);

/* ---- PCD text codec (save_pcd, tools/generate_train_data.py:184-190; src/dataset.py:31-76) ----
 * Integer arithmetic, no atomics: every output is bitwise reproducible.
 *
 * Formatter.  points [n_rows,4] fp64 (is_fp64 != 0) or fp32, 16-byte aligned.  The text of a row
 * is "%.4f %.4f %.4f %d\n" byte for byte as C printf / Python's % operator write it: %.4f rounds
 * half to even on the exact binary value, a negative value that rounds to zero and -0.0 keep
 * their sign, %d truncates toward zero.  Domain: finite x, y, z with |v| < 2^40 and finite
 * intensity with |v| < 2^53; a row outside it has length 0 and no byte is written for it.
 * Rows are formatted in groups of prh_pcd_group_rows() (64), G = ceil(n_rows / 64).
 *   prh_pcd_format_count  row_bytes [n_rows] u8 length of each row, group_bytes [G] int32 their
 *                         sums; status [1] int64 = the first row outside the domain, or -1
 *   prh_pcd_format_write  group_offsets [G+1] int64 = exclusive prefix sum of group_bytes (the
 *                         caller's scan); text [capacity] the rows back to back (bytes at or past
 *                         capacity are never written); offsets [n_slices+1] int64 rows of each
 *                         slice (NULL: one slice of all rows) -> byte_offsets [n_slices+1] int64,
 *                         slice s is text[byte_offsets[s] .. byte_offsets[s+1])
 *
 * Parser.  payload [n_bytes] is the text after the header, any alignment, any length.
 *   prh_pcd_index_blocks  NB, blocks of 4096 bytes on the 16-byte aligned address grid (pure)
 *   prh_pcd_index_count   block_lines [NB] int32 newlines per block
 *   prh_pcd_index_write   block_offsets [NB+1] int64 = exclusive prefix sum of block_lines;
 *                         row_start [n_rows+1] int64: row r is payload[row_start[r] ..
 *                         row_start[r+1]); n_rows = newlines + 1 if the last byte is not one
 *   prh_pcd_parse         out [n_rows,ncols] float32 = float32(correctly rounded double), the bits
 *                         np.loadtxt(dtype=float32) returns.  Fields are separated by runs of
 *                         blanks or tabs, "\r\n" is accepted.  Served: tokens
 *                         [+-]?(d+(.d*)?|.d+)([eE][+-]?d+)? whose digits after leading zeros are
 *                         an integer <= 2^53 (at most 19 digits) and whose decimal exponent minus
 *                         fraction digits lies in [-22, 22].  status [1] int64 = the first row
 *                         with any other token or byte, no field (blank line) or a field count
 *                         other than ncols, else -1; out is then not to be used.
 *
 * prh_pcd_unpack14: payload of n_points 14-byte records (x y z float32, intensity uint16, little
 * endian, any alignment) -> out [n_points,4] float32. */
int prh_pcd_group_rows(void);
size_t prh_pcd_format_workspace_bytes(long long n_rows);
int prh_pcd_format_count(const void* points, int is_fp64, long long n_rows, unsigned char* row_bytes,
                         int* group_bytes, long long* status, void* workspace, size_t workspace_bytes, int device,
                         void* stream);
int prh_pcd_format_write(const void* points, int is_fp64, long long n_rows, const unsigned char* row_bytes,
                         const long long* group_offsets, const long long* offsets, int n_slices,
                         unsigned char* text, long long capacity, long long* byte_offsets, int device,
                         void* stream);
long long prh_pcd_index_blocks(const void* payload, long long n_bytes);
int prh_pcd_index_count(const unsigned char* payload, long long n_bytes, int* block_lines, int device,
                        void* stream);
int prh_pcd_index_write(const unsigned char* payload, long long n_bytes, const long long* block_offsets,
                        long long* row_start, long long n_rows, int device, void* stream);
size_t prh_pcd_parse_workspace_bytes(long long n_rows);
int prh_pcd_parse(const unsigned char* payload, long long n_bytes, const long long* row_start, long long n_rows,
                  int ncols, float* out, long long* status, void* workspace, size_t workspace_bytes, int device,
                  void* stream);
int prh_pcd_unpack14(const unsigned char* payload, long long n_points, float* out, int device, void* stream);

/* ---- prediction scenes (tools/generate_inference_data_vma.py of the reference) ---------------
 * Per camera frame: GT polylines clipped into the ego frame by that tool's rule, a (prediction x
 * GT) matrix of one-way xy Chamfer costs, and the minimum-cost assignment.  fp64 throughout, no
 * atomics: every output is bitwise reproducible.
 *
 * Clipping: as prh_drive_clip_* (same buffers, poses [n_frames,7]), with this tool's rule: a line
 * counts only if some vertex has -segment_len/2 < local x < segment_len/2 (else count 0), and is
 * cut by two half-plane passes without de-duplication, an edge with |dx| < 1e-6 giving its first
 * vertex as the intersection. */
size_t prh_match_clip_workspace_bytes(int n_frames);
int prh_match_clip_count(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_frames, double segment_len, int* counts, void* workspace, size_t workspace_bytes,
                         int device, void* stream);
int prh_match_clip_write(const double* lines, const long long* line_offsets, int n_lines, const double* poses,
                         int n_frames, double segment_len, const long long* out_offsets, double* out,
                         void* workspace, size_t workspace_bytes, int device, void* stream);
/* Costs: pred_xy / gt_xy [*,2] fp64 vertices; *_line_offsets int64 vertex CSR over lines;
 * *_frame_offsets [n_frames+1] int64 line CSR over frames; frame f's (P_f, G_f) row-major matrix
 * goes to costs + cost_offsets[f]: cost[i,j] = mean over the vertices of prediction i of the
 * distance to the nearest vertex of GT line j. */
size_t prh_match_costs_workspace_bytes(long long n_pred_lines);
int prh_match_costs(const double* pred_xy, const long long* pred_line_offsets, const long long* pred_frame_offsets,
                    long long n_pred_lines, const double* gt_xy, const long long* gt_line_offsets,
                    const long long* gt_frame_offsets, int n_frames, const long long* cost_offsets, double* costs,
                    void* workspace, size_t workspace_bytes, int device, void* stream);
/* Assignment (needs no workspace): shapes [n_frames,2] int32 (P_f, G_f), each side at most
 * prh_match_max_side(); max_cells >= the largest P_f * G_f of the call (it sizes the LDS image).
 * match + row_offsets[f] [P_f] int32: the GT column of each prediction or -1, also -1 where
 * use_threshold and the pair's cost is not < threshold; total [n_frames]: the optimal sum before
 * the threshold; status [n_frames] int32: 0 solved, 1 a non-finite cost (all -1, total NaN),
 * 2 above the size bound.  row_dual (at row_offsets) / col_dual (at col_offsets), both optional:
 * the potentials u, v the solver ended with, cost[i,j] - u[i] - v[j] >= 0 with equality on the
 * assigned pairs. */
int prh_match_max_side(void);
int prh_match_assign(const double* costs, const long long* cost_offsets, const int* shapes, const long long* row_offsets,
                     const long long* col_offsets, int n_frames, long long max_cells, double threshold,
                     int use_threshold, int* match, double* total, int* status, double* row_dual, double* col_dual,
                     int device, void* stream);

/* ---- BEV rendering (tools/vis_inference_bev.py and train_dist.py:18-56 of the reference) -----
 * Intensity image (:74-104).  points [n,4] x y z intensity, fp32 or fp64 (is_double), contiguous.
 * prh_bev_bounds: info [5] fp64 = x_min x_max y_min y_max of the points (exact) and 1.0 when an x,
 * y or intensity is NaN or infinite.  prh_bev_raster: image [n_slices,height,width] fp32; slice s
 * owns points offsets[s]..offsets[s+1] (offsets NULL: one slice).  In the dtype of the points,
 * one rounding per operation: u = int32((y - y_min) / resolution), v = int32((x_max - x) /
 * resolution), toward zero; points outside 0 <= u < width, 0 <= v < height are dropped; a pixel
 * holds the maximum float32 intensity of its points and 0.0 when it has none (integer atomicMax of
 * an order-preserving key: the same bits every run).  *bad (device int) = 1 when a value is not
 * finite; the image is then unspecified. */
size_t prh_bev_bounds_workspace_bytes(void);
int prh_bev_bounds(const void* points, long long n, int is_double, double* info, void* workspace,
                   size_t workspace_bytes, int device, void* stream);
int prh_bev_raster(const void* points, const long long* offsets, int n_slices, long long n, int is_double,
                   double y_min, double x_max, double resolution, int height, int width, float* image, int* bad,
                   int device, void* stream);
/* Tone map (:143-148).  prh_bev_select: per slice of image [n_slices,pixels] the two order
 * statistics of the pixels > 0 that numpy's percentile (method 'linear') interpolates between, by
 * an exact radix select over the float bits: out [n_slices,4] fp64 = count of positive pixels,
 * a[floor(i)], a[floor(i) + 1] (or a[count - 1] twice at the top), weight i - floor(i), with
 * i = (count - 1) * quantile in fp32, as numpy computes it for an fp32 array; all zero for a slice
 * without a positive pixel.
 * prh_bev_tone: out = p[s] > 0 ? powf(clip(image / p[s], 0, 1), gamma) : image, fp32.
 * prh_bev_colorize: out RGBA bytes = table[min(int(norm * 256), 255)] (table [256] packed RGBA, R
 * in the low byte), opaque black where image == 0. */
size_t prh_bev_select_workspace_bytes(int n_slices);
int prh_bev_select(const float* image, int n_slices, long long pixels, float quantile, double* out, void* workspace,
                   size_t workspace_bytes, int device, void* stream);
int prh_bev_tone(const float* image, int n_slices, long long pixels, const float* p, float gamma, float* out,
                 int device, void* stream);
int prh_bev_colorize(const float* norm, const float* image, long long pixels, const unsigned* table, unsigned* out,
                     int device, void* stream);
/* Views.  Packed views: view k is an (H_k, W_k) RGBA image at pixel_offsets[k] of one buffer.
 * prh_bev_crop: views [n_views,4] int32 = u0, v0, H_k, W_k; pixel (v, u) of view k is pixel
 * (v + v0, u + u0) of rgba [height,width], opaque black outside it.
 *
 * Overlays - the rule.  A view shows a window (y_lo, y_hi, x_lo, x_hi) in metres at `resolution`
 * metres per pixel: column u grows with y, row v grows with decreasing x, pixel (v, u) has its
 * centre at (u + 0.5, v + 0.5) in pixel units, so a point (x, y) lies at ((y - y_lo) / resolution,
 * (x_hi - x) / resolution).  A polyline has a colour (RGB, 0..255), a width w in pixels, an
 * opacity a and a dash (on, off) in pixels measured along the line from its first vertex (off = 0:
 * solid).  For a pixel centre at distance d from the nearest point of a segment, that segment
 * covers the pixel by clamp(w / 2 + 0.5 - d, 0, 1), and by zero when that nearest point lies in an
 * "off" stretch (arc length modulo (on + off) >= on).  A line covers a pixel by the maximum c over
 * its segments.  Lines are composited in the order given: rgb = rgb * (1 - a * c) + colour * (a *
 * c), in fp64, rounded to the nearest integer once after the last line; alpha is kept.  A pixel
 * no line covers is not written.
 * segments [n_segments,5] fp64 = ax ay bx by in the pixel units of the line's view and the arc
 * length at a; segment_line the line of each (ascending); styles [n_lines,7] fp64 = r g b a w on
 * off; line_view the view of each line; view_dims [n_views,4] int32 = H, W, tiles across, tiles
 * down (tiles of prh_bev_tile() pixels); tile_base [n_views] the first tile of each view;
 * tile_view [n_tiles] the view of each tile.  prh_bev_draw_count: tile_count [n_tiles] = segments
 * whose bounding box, grown by w / 2 + 0.5, touches the tile; the caller's exclusive scan of it is
 * tile_offsets [n_tiles+1], n_items its last entry.  prh_bev_draw composites into canvas (packed
 * views).  Work: one bounding-box walk per segment and, per pixel, the segments binned to its
 * tile.  Bitwise reproducible. */
int prh_bev_crop(const unsigned* rgba, int height, int width, const int* views, const long long* pixel_offsets,
                 int n_views, long long total_pixels, unsigned* out, int device, void* stream);
int prh_bev_tile(void);
int prh_bev_draw_count(const double* segments, const int* segment_line, int n_segments, const double* styles,
                       const int* line_view, const int* view_dims, const long long* tile_base, long long n_tiles,
                       int* tile_count, int device, void* stream);
size_t prh_bev_draw_workspace_bytes(long long n_tiles, long long n_items);
int prh_bev_draw(const double* segments, const int* segment_line, int n_segments, const double* styles,
                 const int* line_view, const int* view_dims, const long long* tile_base,
                 const long long* pixel_offsets, const int* tile_view, const long long* tile_offsets,
                 long long n_tiles, long long n_items, unsigned* canvas, void* workspace, size_t workspace_bytes,
                 int device, void* stream);

/* ---- 3-D scene views (inference_whole_scene.py:242-404, tools/visualize_data.py,
 * check_global_align.py and visualize_sampled_pointcloud.py of the reference) ------------------
 * Depth-buffered point splats and polylines under orbit cameras; every point of the cloud is drawn.
 *
 * 3-D views - the rule.
 * Camera.  A camera is an fp64 row of 16 values: eye[3], r[3], u[3], f[3], s, near, ortho, 0.  An
 * orbit camera about a target c at elevation e, azimuth a (matplotlib's view_init convention) and
 * distance D has eye = c + D * (cos e cos a, cos e sin a, sin e), right r = (-sin a, cos a, 0), up
 * u = (-sin e cos a, -sin e sin a, cos e), forward f = -(cos e cos a, cos e sin a, sin e); nothing
 * is singular at e = +-90 degrees.  Perspective (ortho = 0): s = (H / 2) / tan(fov / 2) pixels.
 * Orthographic (ortho != 0): s = pixels per metre.  The host builds the rows; the device evaluates
 * no trigonometric function and no square root.
 * Projection of a point p, all in fp64, no contraction, one rounding per operation, in this order:
 * q = p - eye; xr = (q0 * r0 + q1 * r1) + q2 * r2, yu and d likewise with u and f; the point is
 * dropped unless d >= near; k = ortho ? s : s / d; X = W / 2 + xr * k, Y = H / 2 - yu * k; the
 * pixel is (row floor(Y), column floor(X)), pixel centres at (+0.5, +0.5).  float32 inputs are
 * promoted exactly.
 * Depth word.  A pixel holds one 64-bit word (bits(float32(depth)) << 32) | payload; the empty
 * word is all ones; every write is a 64-bit unsigned atomic minimum, so the buffer does not depend
 * on arrival order.  A depth below zero (possible only through a line's bias) counts as +0.  Point
 * payload: 0x01000000 | lut, lut = clamp(floor((I - cmin) / (cmax - cmin) * 256), 0, 255), clamped
 * before the integer conversion.  Line payload: the line's index (< 2^24).  At equal depth a line
 * beats a point, a lower line index a higher one, a lower colour index a higher one.
 * Splat.  A point covers the size x size pixels at offsets i - size / 2 (integer division), i = 0 ..
 * size - 1, on both axes, size 1..9, all with the point's depth word; pixels outside the image are
 * skipped.  A NaN or infinite x, y, z or intensity sets *bad and is skipped.
 * Lines.  The host cuts every segment of a (polyline, view) pair to d >= near by linear
 * interpolation in view space and projects it without the floor.  A segment is ax ay bx by
 * (pixels), arc_a (screen arc length at a from the line's first drawn vertex), L (its screen
 * length), wa, wb (1 / d in a perspective view, d in an orthographic one), with its line and view.
 * A style is r g b, width, marker, dash_on, dash_off (pixels) and bias (metres).  For a pixel
 * centre c: t = clamp(((c - a).(b - a)) / |b - a|^2, 0, 1), t = 0 for a zero-length segment.  With
 * width > 0 the segment covers the pixel when |c - (a + t (b - a))|^2 <= (width / 2)^2 and
 * (dash_off == 0 or fmod(arc_a + t * L, dash_on + dash_off) < dash_on), at depth 1 / ((1 - t) * wa
 * + t * wb) (perspective-correct) or (1 - t) * wa + t * wb (orthographic).  With marker > 0 vertex a
 * covers it when |c - a|^2 <= (marker / 2)^2, at a's depth (1 / wa or wa), and b likewise.  The
 * smallest of these depths, minus bias, forms the word.  Edges are hard: no blending, no
 * transparency; order-independent transparency is out of scope.
 * Resolve.  Empty -> the background colour; a point word -> table[lut]; a line word -> the line's
 * colour; alpha 255.  The depth image is float32, +inf where the pixel is empty.
 *
 * points [n,4] x y z intensity, fp32 or fp64 (is_double), contiguous.  prh_view_bounds: info [7]
 * fp64 = x_min x_max y_min y_max z_min z_max (exact) and 1.0 when a value is NaN or infinite.
 * zbuf [n_views,height,width] 64-bit words.  prh_view_splat: cameras [n_views,16], at most
 * prh_view_max_views() per call; offsets NULL: every point into every view; else point i of slice
 * s (offsets [n_slices+1]) goes into view v when slice_mask[s * n_views + v] != 0.  One pass over
 * the points.  prh_view_lines: segments [n_segments,8], segment_ids [n_segments,2] int32 = line,
 * view; styles [n_lines,8]; one workgroup per segment walks its bounding box grown by max(width,
 * marker) / 2.  prh_view_resolve: table [256] and line_colours [n_lines] packed RGBA (R in the low
 * byte), background likewise; rgba [pixels], depth [pixels].  Bitwise reproducible. */
size_t prh_view_bounds_workspace_bytes(void);
int prh_view_bounds(const void* points, long long n, int is_double, double* info, void* workspace,
                    size_t workspace_bytes, int device, void* stream);
int prh_view_clear(unsigned long long* zbuf, int n_views, int height, int width, int device, void* stream);
int prh_view_max_views(void);
int prh_view_splat(const void* points, long long n, int is_double, const double* cameras, int n_views,
                   const long long* offsets, int n_slices, const unsigned char* slice_mask, int size, double cmin,
                   double cmax, int height, int width, unsigned long long* zbuf, int* bad, int device, void* stream);
int prh_view_lines(const double* segments, const int* segment_ids, int n_segments, const double* styles,
                   int n_lines, const double* cameras, int n_views, int height, int width, unsigned long long* zbuf,
                   int device, void* stream);
int prh_view_resolve(const unsigned long long* zbuf, long long pixels, const unsigned* table,
                     const unsigned* line_colours, int n_lines, unsigned background, unsigned* rgba, float* depth,
                     int device, void* stream);

/* ---- map fusion: the refined pieces of a drive merged into one map in the drive frame --------
 * The reference stops at per-slice arrays in per-slice ego frames; it has no counterpart of this
 * stage, so the rule below is the specification (tests/_fuse_oracle.py restates it in numpy).
 *
 * Map fusion - the rule.
 * All arithmetic is fp64, one rounding per operation, no contraction; a dot product of two
 * 3-vectors is (p0 * q0 + p1 * q1) + p2 * q2, |p|^2 = p.p.  The host subtracts an origin from every
 * carrier vertex and every pose translation before the upload and adds it back to the fused
 * vertices; the default origin is the first pose's translation with each component rounded down
 * to a multiple of 1000 m, so device coordinates stay within a few km of zero.
 * Inputs.  n_lines carrier polylines in CSR form (line_offsets [n_lines+1]) with the cumulative
 * 3-D arc length cum of each, computed on the host from the shifted vertices: cum[0] = 0, cum[k+1]
 * = cum[k] + sqrt(|V[k+1] - V[k]|^2), sequentially; the same bits go to the device and to the
 * oracle.  n_pieces pieces of M points each (2 <= M <= prh_fuse_max_points() = 64) in ego
 * coordinates, each with a line and a pose index; poses [S,7] = x y z qx qy qz qw.  Pieces are
 * grouped by line in ascending line order, and the caller's order within a line is kept.
 * 1. To the drive frame.  w = R(q) p + t, each component ((R0 p0 + R1 p1) + R2 p2) + t, with R the
 *    rotation matrix of the normalised quaternion: the transpose of the matrix the drive slicer
 *    applies (local = R^T (p - t)), built by the same code.
 * 2. Projection of w onto its carrier.  For every segment k = (a, b) = (V[k], V[k+1]) with e = b - a
 *    and L2 = e.e > 0: u = clamp(((w - a).e) / L2, 0, 1), c = a + u e, d2 = |w - c|^2.  The first k
 *    with the strictly smallest d2 wins (seg = k); s = cum[k] + u (cum[k+1] - cum[k]), d = sqrt(d2).
 *    A carrier without such a segment gives seg = -1, s = 0 and d = sqrt(|w - V[0]|^2).
 * 3. Taper.  Point i of a piece weighs t_i = min(i + 1, M - i): piece ends sit at slice edges,
 *    where the context tube is cut off, so they count least.
 * 4. Nodes.  A line with at least one vertex has the nodes j = 0 .. floor(cum_total / ds) at arc
 *    position (double)j * ds (a line without vertices has none).  Piece segment i = (point i, point
 *    i + 1) is used only if s[i+1] > s[i]; it contributes to every node with s[i] <= j ds < s[i+1]:
 *    u = (j ds - s[i]) / (s[i+1] - s[i]), weight om = t_i + u (t_{i+1} - t_i), position x = w_i + u
 *    (w_{i+1} - w_i).  A piece that runs against its carrier contributes nothing and one that
 *    doubles back contributes more than once; both follow from the rule and are kept.
 * 5. Node result.  C = number of contributions, W = sum om, X = (sum om x) / W, spread = sqrt((sum
 *    om |x - X|^2) / W), the last taken in a second sweep once X is known; every sum starts at 0
 *    and runs over the line's pieces in the caller's order, then ascending i, so the output is
 *    bitwise reproducible and independent of the launch shape.  A node with C = 0 gets X = 0, W =
 *    0, spread = 0.
 * 6. Polylines (host).  The fused polylines of a line are its nodes with C >= min_count (default
 *    1) in node order; two consecutive used nodes j < j' with (j' - j) ds > max_gap (default 5.0
 *    m) belong to different polylines; polylines of fewer than 2 nodes are dropped.
 *
 * prh_fuse_project: one thread per piece point, steps 1-2.  pieces [n_pieces*M,3]; piece_pose NULL:
 * the points are in the drive frame already (M >= 1 is enough here); piece_line NULL: step 1 only,
 * s / d / seg are not written.  world [n_pieces*M,3], s, d [n_pieces*M] fp64, seg [n_pieces*M]
 * int32.  Carrier vertices and cum go through LDS prh_fuse_tile() segments at a time, so a carrier
 * may be of any length.  A piece whose line index is outside 0..n_lines-1 gets seg = -1, s = d = 0;
 * one whose pose index is outside 0..n_poses-1 gets NaN.
 * prh_fuse_gather: one thread per node, steps 3-5 as a gather over the line's pieces: no atomics,
 * no sort.  line_piece_offsets [n_lines+1]: line l owns pieces line_piece_offsets[l] ..
 * line_piece_offsets[l+1]; node_offsets [n_lines+1] likewise for the nodes, node j of line l at
 * (double)j * ds.  node_x [n_nodes,3], node_w, node_spread [n_nodes] fp64, node_count [n_nodes]
 * int32. */
int prh_fuse_max_points(void);
int prh_fuse_tile(void);
size_t prh_fuse_project_workspace_bytes(int n_poses);
int prh_fuse_project(const double* pieces, long long n_pieces, int points_per_piece, const int* piece_line,
                     const int* piece_pose, const double* poses, int n_poses, const double* line_vertices,
                     const long long* line_offsets, const double* line_cum, int n_lines, double* world, double* s,
                     double* d, int* seg, void* workspace, size_t workspace_bytes, int device, void* stream);
size_t prh_fuse_gather_workspace_bytes(long long n_pieces);
int prh_fuse_gather(const double* world, const double* s, long long n_pieces, int points_per_piece,
                    const long long* line_piece_offsets, int n_lines, const long long* node_offsets,
                    long long n_nodes, double ds, double* node_x, double* node_w, int* node_count,
                    double* node_spread, void* workspace, size_t workspace_bytes, int device, void* stream);

/* Piece linking - the rule.
 * Which refined pieces of a drive are the same lane, when no carrier says so (detector output).
 * The conventions are those of "Map fusion - the rule": fp64, one rounding per operation, no
 * contraction, a 3-vector dot is (p0 * q0 + p1 * q1) + p2 * q2, the origin is shifted on the host.
 * Inputs.  P pieces of M points each (2 <= M <= 64) in the shifted drive frame: the world output of
 * prh_fuse_project with piece_line NULL.  A frame index per piece.  Per piece cum[M], the
 * cumulative arc length of its points computed on the host (cum[0] = 0, cum[k+1] = cum[k] +
 * sqrt(|A[k+1] - A[k]|^2), sequentially); the same bits go to the device and to the oracle.
 * Parameters gate (metres, default 1.0), min_in (default 4), out_ratio (default 4).
 * 1. Boxes.  Per piece, lo[c] and hi[c] are the min and max over its points, per axis.
 * 2. Candidates.  A candidate is a pair (i, j) with i < j, frame[i] != frame[j] and, for every
 *    axis, lo_i[c] - gate <= hi_j[c] and lo_j[c] - gate <= hi_i[c].  Candidates are listed by
 *    ascending i, then ascending j; that order is part of the rule.  Pieces of one frame are never
 *    linked directly: two detections in one frame are two objects, or two fragments that do not
 *    overlap.
 * 3. Directed statistics of a -> b.  Every point k of a, in ascending k, is projected onto the
 *    polyline b exactly as in fusion step 2 (segments with L2 > 0, clamped u, the first strictly
 *    smallest d2), which gives seg, u, d = sqrt(d2) and s_b = cum_b[seg] + u (cum_b[seg+1] -
 *    cum_b[seg]).  The point is end-clamped if b has no usable segment, or seg is b's first usable
 *    segment and u == 0, or seg is b's last usable segment and u == 1: it lies beyond b, outside
 *    the overlap, and counts nowhere.  An interior point with d <= gate is in: n_in += 1, sum_d +=
 *    d, sum_a += cum_a[k], sum_b += s_b, sum_dot += e_a . e_b with e_a = A[q+1] - A[q], q = min(k,
 *    M - 2), and e_b the winning segment's vector.  An interior point with d > gate is out:
 *    n_out += 1.
 * 4. Pair statistics.  n_in, n_out, sum_d and sum_dot of the pair (i, j) are the totals of i -> j
 *    and then j -> i; sum_self, the coordinate along i, is sum_a of i -> j plus sum_b of j -> i;
 *    sum_other, the coordinate along j, is sum_b of i -> j plus sum_a of j -> i.  Every sum starts
 *    at 0 and runs over i -> j in ascending k, then j -> i in ascending k, so the result is bitwise
 *    reproducible and independent of the launch shape.
 * 5. Edges (host, or prh_link_edges).  A candidate is an edge iff n_in >= min_in and out_ratio * n_out <= n_in, in
 *    integers.  rho = +1 if sum_dot >= 0, else -1; delta = (sum_self - rho * sum_other) / n_in: the
 *    arc coordinate along i of a point is delta + rho times its coordinate along j.
 * 6. Clusters and arc synchronisation (host, or prh_link_label_round and prh_link_tree_level).  Clusters are the connected components of the edge
 *    graph, numbered by ascending smallest member.  That member is the root: level 0, sigma = +1,
 *    o = 0.  A piece at level n + 1 takes as parent, among its neighbours at level n, the one with
 *    the largest n_in; ties go to the smallest index.  For child b, parent a and their edge (i, j):
 *    sigma_b = rho * sigma_a; if a == i, o_b = o_a + sigma_a * delta, otherwise o_b = o_a - sigma_b *
 *    delta.  Point k of piece p gets g = o_p + sigma_p * cum_p[k].  A piece with sigma_p < 0 has its
 *    points and its g reversed, so g ascends along every piece (detector polylines come in either
 *    direction).  Per cluster, the smallest g is subtracted.
 * 7. Draft carriers.  The clusters with at least min_pieces pieces (default 2) are kept: a lane
 *    seen once is not evidence.  prh_fuse_gather runs on them with s := g, every cluster a line with
 *    the nodes 0 .. floor(max g / step).  A cluster's draft carrier is its nodes with C >= 1 in node
 *    order, as one polyline (gaps are bridged); a cluster with fewer than 2 such nodes is dropped
 *    like a small one.
 * 8. Map.  The standard fusion (steps 1-6 of "Map fusion - the rule") of the kept pieces, the
 *    reversed ones reversed, with the draft carriers as lines and the cluster as piece_line.  The
 *    second pass removes what arc drift the spanning tree left.
 *
 * prh_link_pairs_count / prh_link_pairs_write: steps 1-2 in two calls over the same inputs.  world
 * [n_pieces*M,3] fp64, piece_frame [n_pieces] int32.  Count fills pair_offsets [n_pieces+1]: the
 * exclusive scan, taken on the device, of the number of candidates (i, j > i) per i.  The caller
 * reads pair_offsets[n_pieces], sizes pair_j (int32) by it, and write fills pair_j with the
 * ascending j of every i from pair_offsets[i] on.  The boxes of the j side go through LDS
 * prh_link_tile() at a time and a row is compacted with ballot / popcount: no sort, no atomic.
 * O(n_pieces^2) box tests; at most 2^24 pieces.
 * prh_link_stats: steps 3-4 for every candidate, one wave per pair, prh_link_pairs_per_block()
 * pairs per block.  cum [n_pieces*M].  pair_count [n_pairs,2] int32 = n_in n_out; pair_sum
 * [n_pairs,4] fp64 = sum_d sum_self sum_other sum_dot.  Pair p belongs to the i with
 * pair_offsets[i] <= p < pair_offsets[i+1]; a pair_j[p] outside 0..n_pieces-1 gives counts of -1
 * and NaN sums. */
int prh_link_tile(void);
int prh_link_pairs_per_block(void);
size_t prh_link_pairs_workspace_bytes(long long n_pieces);
int prh_link_pairs_count(const double* world, long long n_pieces, int points_per_piece, const int* piece_frame,
                         double gate, long long* pair_offsets, void* workspace, size_t workspace_bytes, int device,
                         void* stream);
int prh_link_pairs_write(const double* world, long long n_pieces, int points_per_piece, const int* piece_frame,
                         double gate, const long long* pair_offsets, int* pair_j, void* workspace,
                         size_t workspace_bytes, int device, void* stream);
int prh_link_stats(const double* world, const double* cum, long long n_pieces, int points_per_piece,
                   const long long* pair_offsets, const int* pair_j, long long n_pairs, double gate, int* pair_count,
                   double* pair_sum, int device, void* stream);

/* Steps 5-6 and cum on the device (csrc/prh_link_sync.hpp).  The rule above is unchanged; these give
 * the bits of its host statement (link.piece_cums, link.edges_of, link.sync_pieces), so the
 * candidates' statistics need not leave the device.  No float atomic, no sort, and no atomic whose
 * arrival order can show in a result.  At most 2^24 pieces everywhere.
 * prh_link_cum: world [n_pieces*M,3] fp64 -> cum [n_pieces*M] fp64, one thread per piece: cum[0] = 0,
 * cum[k+1] = cum[k] + sqrt((e0 * e0 + e1 * e1) + e2 * e2) with e = A[k+1] - A[k], sequentially, no
 * contraction.  Subtraction, multiplication, addition and sqrt are correctly rounded on both sides,
 * so the bits are those of the host's cum.
 * prh_link_edges: step 5 for every candidate, one thread each.  pair_count [n_pairs,2] int32 and
 * pair_sum [n_pairs,4] fp64 are prh_link_stats' outputs.  Out: pair_i [n_pairs] int32, the i with
 * pair_offsets[i] <= p < pair_offsets[i+1]; edge [n_pairs] uint8 = n_in >= min_in && out_ratio *
 * n_out <= n_in in 64-bit integers (counts of -1, a bad pair_j, are no edge); rho [n_pairs] int8 = +1
 * if sum_dot >= 0.0 (so for -0.0), else -1 (so for NaN); delta [n_pairs] fp64 = (sum_self - rho *
 * sum_other) / (double)n_in where n_in > 0, else 0: rho * sum_other is exact, the subtraction and the
 * division round once each, as on the host.  edge_scan [2 * prh_link_edges_blocks(n_pairs) + 1]
 * int64 is scratch that prh_link_edges_compact reads; edge_scan[prh_link_edges_blocks(n_pairs)] is
 * the number of edges, which the caller reads to size the next call's buffers.
 * prh_link_edges_compact: the edges in candidate order (ballot / popcount behind the scanned block
 * counts: the order is the candidates', whatever the launch does).  edge_ij [n_edges,2] int32 = i j,
 * edge_w [n_edges,2] int32 = n_in rho, edge_delta [n_edges] fp64.  The later calls read only these.
 * prh_link_label_round: one round of the components.  label [n_pieces] int32 starts as 0 .. n_pieces
 * - 1, filled by the caller.  The first kernel does, per edge, atomicMin(label[i], label[j]) and the
 * other way round, and sets *changed (a device int32, zeroed by the call) when an atomic lowered a
 * label; the second chases every label to a label that is its own.  The caller repeats the call until
 * it reads *changed == 0.  Then label[p] is the smallest member of p's component, bitwise the same in
 * every run: every stored label is a member of the component and labels only fall; a round that
 * lowered nothing changed no word of label, so its plain loads next to the atomics all read the value
 * the launch before left, label is equal across every edge and its own label everywhere, and the
 * smallest member m, whose label is a member <= m, holds m.  The number of rounds may differ from run
 * to run; the fixed point cannot.  The cluster number is the rank of label[p] among the p with
 * label[p] == p.
 * prh_link_tree_init / prh_link_tree_level: the spanning trees, a level per call.  init sets level
 * [n_pieces] int32 to 0 at the roots (label[p] == p) and -1 elsewhere, parent int32 to -1, sign int32
 * to +1, offset fp64 to 0 and key uint64 to 0.  level(n) runs two kernels over the edges: per
 * directed edge a -> b with level[a] == n and b unplaced, atomicMax(key[b], (n_in << 32) |
 * (0xFFFFFFFF - a)) - the largest n_in, ties to the smallest a, and a maximum does not depend on
 * the order it is taken in (n_in <= 128 and a < 2^24, so the key fits; 0 means none); then the one
 * directed edge whose key won (a pair occurs once among the candidates) writes level[b] = n + 1,
 * parent[b] = a, sign[b] = rho * sign[a] and offset[b] = offset[a] + sign[a] * delta if a is the
 * edge's i, else offset[a] - sign[b] * delta: sign * delta is exact, so one rounding per offset, as
 * on the host.  *placed (device int32, zeroed by the call) is set when a piece was placed; the
 * caller calls n = 0, 1, .. until it reads 0, after at most n_pieces levels. */
int prh_link_cum(const double* world, long long n_pieces, int points_per_piece, double* cum, int device, void* stream);
long long prh_link_edges_blocks(long long n_pairs);
int prh_link_edges(const long long* pair_offsets, long long n_pieces, const int* pair_count, const double* pair_sum,
                   long long n_pairs, long long min_in, long long out_ratio, int* pair_i, unsigned char* edge,
                   signed char* rho, double* delta, long long* edge_scan, int device, void* stream);
int prh_link_edges_compact(const int* pair_i, const int* pair_j, const int* pair_count, const unsigned char* edge,
                           const signed char* rho, const double* delta, long long n_pairs, const long long* edge_scan,
                           long long n_edges, int* edge_ij, int* edge_w, double* edge_delta, int device, void* stream);
int prh_link_label_round(const int* edge_ij, long long n_edges, long long n_pieces, int* label, int* changed, int device,
                         void* stream);
int prh_link_tree_init(const int* label, long long n_pieces, int* level, int* parent, int* sign, double* offset,
                       unsigned long long* key, int device, void* stream);
int prh_link_tree_level(const int* edge_ij, const int* edge_w, const double* edge_delta, long long n_edges,
                        long long n_pieces, int n, int* level, int* parent, int* sign, double* offset,
                        unsigned long long* key, int* placed, int device, void* stream);

/* Cloud support - the rule.
 * What the merged cloud holds in the tube around every station of every map polyline: how many
 * points, how bright, on which side, how high.  It needs no ground truth.  The conventions are
 * those of "Map fusion - the rule": fp64, one rounding per operation, no contraction, a 3-vector
 * dot is (p0 * q0 + p1 * q1) + p2 * q2, the origin is subtracted from the line vertices on the
 * host, cum is the cumulative arc length of the shifted vertices computed on the host; the same
 * bits go to the device and to the oracle (tests/_support_oracle.py).
 * Inputs.  A cloud [T,4] float32 = x y z intensity in the drive frame, T < 2^31.  n_lines polylines
 * in CSR form.  Parameters step (default 0.5 m, the station spacing), radius (default 0.3 m, 0 <
 * radius <= 8, the tube radius) and intensity_floor (default 0), subtracted from the intensity
 * before weighting.
 * Nodes.  A line with at least one vertex has the nodes j = 0 .. floor(cum_total / step), as in
 * fusion step 4; node_offsets [n_lines+1] numbers them line after line.
 * Per point.  A point with a non-finite field is skipped.  Otherwise w[c] = (double)p[c] -
 * origin[c].
 * Per (point, line), independently for every line:
 * 1. Projection.  Exactly fusion step 2: segments k = (a, b) with e = b - a and L2 = e.e > 0 are
 *    usable; u = clamp(((w - a).e) / L2, 0, 1), c = a + u e, h = w - c, d2 = |h|^2.  The first k
 *    with the strictly smallest d2 wins.  A line without a usable segment gets no hit.
 * 2. Hit.  A hit iff d2 <= r2, where r2 = radius * radius is computed once on the host and passed
 *    in: membership needs no sqrt.
 * 3. Station.  s = cum[k] + u (cum[k+1] - cum[k]); j = min((long long)floor(s / step + 0.5),
 *    n_nodes_l - 1).
 * 4. Lateral offset.  With g = w - a and exy2 = e0 e0 + e1 e1: t = exy2 > 0 ? (e0 g1 - e1 g0) /
 *    sqrt(exy2) : 0.  Positive is left of the line's direction seen from above.
 * 5. Height.  hz = h[2].
 * 6. Weight.  wI = min(max((double)I - intensity_floor, 0), 4096).
 * 7. Fixed point, round-half-even (rint): qi = rint(wI * 256), qt = rint(t * 65536), qz =
 *    rint(hz * 65536).
 * 8. Accumulate into row node_offsets[l] + j of acc [n_nodes,8] int64: [0] += 1, [1] += (qi > 0),
 *    [2] += qi, [3] += qt, [4] += qt * qt, [5] += qi * qt, [6] += qz.  Column [7] stays 0.
 * A point inside the tubes of two lines counts for both.
 * The sums are integers, so the result does not depend on the order of the points or on the
 * launch shape: it is bitwise reproducible by construction.  With radius <= 8 and the weight clamp
 * every addend is below 2^40; the host raises OverflowError when a node counts 2^22 points or
 * more, so no column can pass 2^62.
 *
 * prh_support_accumulate: one thread per point, steps 1-8.  The host lays a uniform xy grid over the
 * lines' bounding box expanded by the radius: cell (ix, iy) = (floor((x - grid_x0) / grid_cell),
 * floor((y - grid_y0) / grid_cell)) in fp64, the same monotone expression on host and device, 0 <=
 * ix < grid_nx, 0 <= iy < grid_ny, at most prh_support_max_cells() = 2^22 cells.  cell_offsets
 * [grid_nx*grid_ny+1] int32 is the CSR of cell_entries [n_entries,2] int32 = (line, segment), cell
 * iy * grid_nx + ix listing every segment whose radius-expanded box overlaps the cell, sorted by
 * line, then by segment.  A thread leaves when its point is outside the grid or its cell is empty;
 * otherwise it walks the list, keeps the best segment per line and flushes a hit when the line
 * changes.  Every segment within radius of a point is in that point's list, so the first strictly
 * smallest d2 of the list is step 1's whenever the point is a hit: the grid changes the cost, never
 * the result.  cloud must be 16-byte aligned; acc is added to, so the caller zeroes it.  The adds
 * are 64-bit integer atomics. */
int prh_support_max_cells(void);
int prh_support_accumulate(const float* cloud, long long n_points, double origin_x, double origin_y, double origin_z,
                           double grid_x0, double grid_y0, double grid_cell, int grid_nx, int grid_ny,
                           const int* cell_offsets, const int* cell_entries, long long n_entries,
                           const double* line_vertices, const long long* line_offsets, const double* line_cum,
                           int n_lines, const long long* node_offsets, long long n_nodes, double step, double r2,
                           double intensity_floor, long long* acc, int device, void* stream);

/* Ground lift - the rule.
 * The height of the road surface under an xy, read from the cloud: the detector's lines come with
 * z = 0 (tools/generate_inference_data_vma.py:262), the context builder's tube is 3-D, so a line
 * has to be put on the road before the tube can hold anything.  The conventions are those of "Map
 * fusion - the rule" and "Cloud support - the rule": fp64 throughout, one rounding per operation,
 * no contraction, and every constant that decides membership is computed once on the host and
 * passed in; the same bits go to the device and to the oracle (tests/_ground_oracle.py).
 * Inputs.  points [T,4] = x y z intensity in the ego frame of their slice, float64 (is_double != 0,
 * what drive.slice_cloud returns) or float32; a float32 coordinate is converted to fp64 first, which
 * is exact.  slice_offsets [S+1] int64: slice s owns rows slice_offsets[s] .. slice_offsets[s+1],
 * fewer than 2^31 of them.  queries [Q,2] fp64 xy, finite, |coordinate| <= 1e6, with query_offsets
 * [S+1] int64: the queries are grouped by slice and a query sees only its own slice's points.
 * Parameters.  radius (default 0.5 m, 0 < radius <= 4) enters as r2 = radius * radius; z_lo
 * (default -8) and bin (default 0.0625, exact in binary) and n_bins (default 256, 1 <= n_bins <=
 * prh_ground_max_bins() = 256) lay the height histogram over [z_lo, z_lo + n_bins * bin), which
 * must lie inside [-256, 256]; min_points (default 5, >= 1); peak_num / peak_den (default 1 / 2,
 * integers, 1 <= peak_num <= peak_den <= 65536).
 * Per (query, point of the same slice).  A point with a non-finite x, y or z is skipped.  dx = x -
 * qx, dy = y - qy, d2 = dx * dx + dy * dy; the pair is a hit iff d2 <= r2: there is no sqrt.  The
 * hit's bin is b = (long long)floor((z - z_lo) / bin); whether 0 <= b < n_bins is decided on the
 * floor in fp64, before the conversion.  A hit with b < 0 or b >= n_bins counts in `hits` and
 * nowhere else.
 * Per query.
 * 1. hist[b] = the hits of bin b, 0 <= b < n_bins.
 * 2. c3[b] = hist[b-1] + hist[b] + hist[b+1], a neighbour outside 0 .. n_bins - 1 taken as 0.
 * 3. peak = max c3.
 * 4. If peak < min_points there is no ground: height = NaN (the quiet NaN 0x7ff8000000000000), bin
 *    = -1, count = 0.
 * 5. Otherwise thr = max(min_points, ceil(peak * peak_num / peak_den)), in integers.
 * 6. g = the lowest b with c3[b] >= thr.
 * 7. While g + 1 < n_bins and c3[g+1] > c3[g]: g = g + 1.
 * 8. That is the lowest mode that holds at least peak_num / peak_den of the strongest one: the road
 *    under a vehicle, a sign gantry or a bridge wins unless the thing above returns more than
 *    peak_den / peak_num times the road's points.
 * 9. Over the hits with max(g - 1, 0) <= b <= min(g + 1, n_bins - 1): qz = (long long)rint(z *
 *    65536) (half to even), sum = the sum of qz and n = their number, both in integers; height =
 *    ((double)sum / (double)n) / 65536.0.  n = c3[g] >= 1.
 * 10. Outputs per query: height fp64, count = n int32, hits int32 (every hit, binned or not), bin =
 *    g int32.
 * All sums are integers, so the result does not depend on the order of the points, on how they are
 * binned into cells or on the launch shape: it is bitwise reproducible by construction.  Overflow:
 * a summed z lies inside [-256, 256], so |qz| <= 2^24 = 2^20 * 16, and n < 2^31, so |sum| < 2^55.
 *
 * The grid changes the cost, never the result.  reach = radius + 1e-6, computed on the host, covers
 * the rounding of d2: a hit has |x - qx| <= reach and |y - qy| <= reach as real numbers (|q| <=
 * 1e6, so an endpoint's rounding is below 1.2e-10).  Slice s has a uniform grid of square cells,
 * `cell` metres wide (cell >= radius, one value for the call): grid_origin [S,2] fp64 = x0 y0 =
 * (min qx - reach, min qy - reach) over the slice's queries, grid_shape [S,2] int32 = nx ny with nx
 * = floor(((max qx + reach) - x0) / cell) + 1 (a slice without a query: 0 0), cell_base [S] int64:
 * cell (ix, iy) of slice s is number cell_base[s] + iy * nx + ix of n_cells < 2^31 in all.  ix =
 * floor((x - x0) / cell) in fp64, the same monotone expression on host and device.
 *   prh_ground_bin_count  cell_counts [n_cells] int32: the points of each cell.  A point outside its
 *                         slice's grid, or with a non-finite x, y or z, is dropped: it can be no hit.
 *   prh_ground_bin_write  rows [capacity] int32: with cell_offsets [n_cells+1] int64 the exclusive
 *                         prefix of cell_counts (the caller scans), rows[cell_offsets[c] ..
 *                         cell_offsets[c+1]] are the rows, counted from the slice's first, of the
 *                         points of cell c, in the order of arrival (an atomic cursor in the
 *                         workspace: the rule does not see the order).  Same arguments as the count.
 *   prh_ground_query      one wave per query: it walks the cells from floor(((q - reach) - x0) /
 *                         cell) to floor(((q + reach) - x0) / cell) in x and y, clipped to the grid -
 *                         by monotonicity every hit's cell is among them; 3 x 3 cells when cell >=
 *                         radius + 1e-6, at most 4 x 4 down to cell = radius - twice: once for the
 *                         histogram (integer LDS atomics), once for sum and n.  No float atomics.
 * points must be aligned to two coordinates (16 bytes for fp64, 8 for float32).  PRH_ERR_ARG for a
 * parameter outside the limits above; PRH_ERR_WORKSPACE below prh_ground_bin_workspace_bytes. */
int prh_ground_max_bins(void);
size_t prh_ground_bin_workspace_bytes(long long n_cells);
int prh_ground_bin_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                         long long n_points, const double* grid_origin, const int* grid_shape,
                         const long long* cell_base, long long n_cells, double cell, int* cell_counts, int device,
                         void* stream);
int prh_ground_bin_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                         long long n_points, const double* grid_origin, const int* grid_shape,
                         const long long* cell_base, long long n_cells, double cell, const long long* cell_offsets,
                         int* rows, long long capacity, void* workspace, size_t workspace_bytes, int device,
                         void* stream);
int prh_ground_query(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long n_points,
                     const double* queries, const long long* query_offsets, long long n_queries,
                     const double* grid_origin, const int* grid_shape, const long long* cell_base, long long n_cells,
                     double cell, const long long* cell_offsets, const int* rows, long long n_rows, double r2,
                     double reach, double z_lo, double bin, int n_bins, int min_points, int peak_num, int peak_den,
                     double* height, int* count, int* hits, int* bin_index, int device, void* stream);

/* Paint alignment - the rule.
 * The xy shift that puts the detector's lines on the paint, read from the cloud without GT: camera
 * lines reach the ego frame through an extrinsic and a nearest-pose match, so a few tenths of a
 * metre of offset are normal, and beyond the context builder's 0.3 m tube the model refines against
 * bare asphalt.  It is the xy twin of the ground lift.  The conventions are those of "Cloud support -
 * the rule" and "Ground lift - the rule": fp64 throughout, one rounding per operation, no
 * contraction, a 3-vector dot is (p0 * q0 + p1 * q1) + p2 * q2, every constant that decides
 * membership is computed once on the host and passed in; the same bits go to the device and to the
 * oracle (tests/_align_oracle.py).
 * Inputs.  points [T,4] = x y z intensity in the ego frame of their slice, float64 (is_double != 0,
 * what drive.slice_cloud returns) or float32, converted to fp64 first, which is exact.
 * slice_offsets [S+1] int64.  The lines of every slice in CSR form: line_vertices [V,3] fp64,
 * finite, |coordinate| <= 1e6, line_offsets [L+1] int64, slice_line_offsets [S+1] int64: slice s
 * owns lines slice_line_offsets[s] .. slice_line_offsets[s+1] and sees no other.  shifts [K,2] fp64
 * = dx dy with shift_offsets [S+1] int64: every slice has its own table (slices may hold the same
 * values), |component| <= 4, at most prh_align_max_shifts() = 4096 rows per slice.  radius (default
 * 0.15 m, 0 < radius <= 1) enters as r2 = radius * radius; intensity_floor (default 0).  The host
 * raises OverflowError when a slice has 2^31 or more (candidate, line) pairs.
 * Per (slice s, shift k = (dx, dy), point p of s, line l of s).
 * 1. A point with a non-finite x, y or z is skipped.  wI = min(max((double)I - intensity_floor, 0),
 *    4096), qi = (long long)rint(wI * 256) (half to even); a non-finite I gives qi = 0; a point with
 *    qi == 0 is skipped.
 * 2. The shifted point is w = (x - dx, y - dy, z): moving the point by -shift is moving the line by
 *    +shift.
 * 3. Projection, exactly fusion step 2 as support's step 1 computes it: segments k = (a, b) with e
 *    = b - a and L2 = e.e > 0 are usable; u = clamp(((w - a).e) / L2, 0, 1), c = a + u e, h = w - c,
 *    d2 = |h|^2.  d2min is the minimum of d2 over the line's usable segments: a minimum has no
 *    order, so tiling the segments never shows.  A line without a usable segment has no hit.
 * 4. The pair is a hit iff d2min <= r2.  Its taper is qk = (long long)rint((1.0 - d2min / r2) *
 *    1024.0), 0 <= qk <= 1024: it peaks on the line, so a tube wider than the paint still has one
 *    best position.
 * 5. score[s,k] += qi * qk, hits[s,k] += 1, both int64.  A point inside the tubes of two lines
 *    counts for both.  An addend is at most 2^20 * 2^10 = 2^30 and a slice has fewer than 2^31
 *    pairs, so a sum stays below 2^61.
 * Per slice, on the host (align.pick_shift).
 * 6. The table must hold the shift (0, 0); k0 is its first row.
 * 7. best = max score.  If best == 0, or hits at the first best row is below min_points (default
 *    32), the shift is (0, 0) and the slice is "unaligned".
 * 8. Near-best: the rows with score * keep_den >= best * keep_num in exact integers (default keep =
 *    63 / 64); of these the one with the smallest dx * dx + dy * dy in fp64, ties to the lowest
 *    row.  On straight lanes the along-lane component is unobservable: a plain arg-max returns an
 *    arbitrary one, the shortest near-best shift returns none.
 * 9. Bias.  For a paint band of half-width w <= r / 2 the expected score falls with the lateral
 *    error e as (e / r)^2 / (1 - w^2 / (3 r^2)), so keep = 63 / 64 moves the pick by at most 0.13 r
 *    towards zero: 0.02 m at the default radius, below one fine step.
 * 10. Gain: the row is accepted iff score[row] * gain_den > score[k0] * gain_num (default gain = 5
 *    / 4); otherwise the shift is (0, 0), "unaligned".
 * Grids.  shift_grid(centre, half, step) = centre + j * step for j = -n .. n, n = round(half /
 * step), x outer, y inner.  Coarse: centre (0, 0), half = max_shift (default 1.0), step 0.1.  Fine:
 * centred on the coarse pick, half 0.1, step 0.02, the row (0, 0) appended; the final pick runs over
 * the fine table.  scope = 'drive': one table for all slices, the slices' integer tables added up
 * (exact, order-free), steps 7-10 once on the sums, in both stages.
 * All sums are integers, so the result does not depend on the order of the points, on the filter,
 * on the tiles or on the launch shape: it is bitwise reproducible by construction.
 *
 * The filter changes the cost, never the result: any superset of the true hitters gives the same
 * sums.  reach [S] fp64 = radius + max_k max(|dx|, |dy|) + 1e-6 per slice, computed on the host: a
 * hit at any shift of the slice lies, in x and in y, within reach of the box of the segment it
 * hits (the 1e-6 covers the rounding of d2 for |coordinate| <= 1e6).  Slice s has a grid of square
 * cells, `cell` metres wide (about 1 m): grid_origin [S,2] = (min x - reach, min y - reach) over
 * the slice's vertices, grid_shape [S,2] int32 = nx ny (a slice without a vertex: 0 0), cell_base
 * [S] int64: cell (ix, iy) of slice s is bit (c & 31) of bitmap[c >> 5], c = cell_base[s] + iy * nx
 * + ix < n_cells < 2^31.  ix = floor((x - x0) / cell) in fp64, the same monotone expression on host
 * and device; the host sets every cell from floor(((lo - reach) - x0) / cell) to floor(((hi +
 * reach) - x0) / cell) of every segment's box, so by monotonicity a hitter's cell is set.
 *   prh_align_select_count  one thread per point: one aligned load, step 1, one bitmap lookup;
 *                           slice_counts [S] int32 (zeroed here): the survivors of each slice.
 *   prh_align_select_write  records [capacity] of 32 bytes (x y z fp64, qi int64): with cand_offsets
 *                           [S+1] int64 the exclusive prefix of slice_counts (the caller scans),
 *                           rows cand_offsets[s] .. cand_offsets[s+1] are slice s's survivors in
 *                           the order of arrival (ballot / popcount and an atomic cursor in the
 *                           workspace: the rule does not see the order).
 *   prh_align_score         one block per work item; items [n_items,3] int64 = (slice, first
 *                           candidate row, first shift row), the host's plan of (slice, tile of 256
 *                           candidates, tile of 16 shifts).  A thread holds one candidate; the
 *                           slice's vertices go through LDS prh_align_tile() = 512 at a time, each
 *                           slot holding the segment that starts at its vertex and the line id;
 *                           d2min is carried across tiles and a line's hit is flushed when the line
 *                           id changes or the list ends.  Before the projection a candidate is
 *                           compared with the segment's reach-expanded box (cost only).  Per shift:
 *                           integer wave reduction, LDS, one 64-bit integer atomicAdd per (block,
 *                           shift, column) into acc [K,2] int64 = score, hits, which the caller
 *                           zeroes.  No float atomics, no sort.
 * points and records must be 16-byte aligned.  PRH_ERR_ARG for a scalar parameter outside the limits
 * above (radius, cell, intensity_floor, the sizes); the limits on the shift tables and the vertices
 * concern device data and are the caller's to check (align.paint_scores raises ValueError); a work
 * item that does not fit the offsets is skipped by its block.  PRH_ERR_WORKSPACE below
 * prh_align_select_workspace_bytes. */
int prh_align_tile(void);
int prh_align_max_shifts(void);
size_t prh_align_select_workspace_bytes(int n_slices);
int prh_align_select_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long n_points, const double* grid_origin, const int* grid_shape,
                           const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                           double intensity_floor, int* slice_counts, int device, void* stream);
int prh_align_select_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long n_points, const double* grid_origin, const int* grid_shape,
                           const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                           double intensity_floor, const long long* cand_offsets, void* records, long long capacity,
                           void* workspace, size_t workspace_bytes, int device, void* stream);
int prh_align_score(const void* records, const long long* cand_offsets, long long n_candidates,
                    const double* line_vertices, long long n_vertices, const long long* line_offsets, int n_lines,
                    const long long* slice_line_offsets, const double* shifts, const long long* shift_offsets,
                    long long n_shifts, const double* reach, int n_slices, const long long* items, long long n_items,
                    double r2, long long* acc, int device, void* stream);

/* Rigid paint alignment - the rule.
 * A shift cannot take out a rotation: a heading error of the camera-lidar extrinsic, or of the
 * matched pose, turns every line of a frame about the sensor, and at 15 mrad a line end 24 m out
 * lies 0.36 m beside the paint.  This rule extends "Paint alignment - the rule" from shifts to poses
 * (yaw about z plus an xy shift); its steps 1 and 3-5 hold verbatim (qi, the projection, d2min, qk,
 * the int64 score and hits), and so do its conventions.  tests/_align_rigid_oracle.py restates it.
 * Pose.  A pose row is (dx, dy, theta).  It moves a line vertex p to R(theta)(p - pivot) + pivot +
 * (dx, dy); z never changes.  pivots [S,2] fp64, one per slice, default (0, 0): the sensor, which is
 * where an extrinsic heading error turns the lines.  c = cos(theta) and s = sin(theta) are computed
 * once on the host and go to the device and to the oracle as the same bits, in the table poses
 * [K,4] fp64 = dx dy c s with pose_offsets [S+1] int64: the device never evaluates a sine.
 * Limits: |theta| <= 0.1 rad, |dx|, |dy| <= 4, |pivot component| <= 1e6, at most
 * prh_align_max_poses() = 32768 rows per slice (the default coarse table has 4851).
 * 2'. Step 2 becomes: the point is moved by the inverse pose, one rounding per operation,
 *       gx = (x - dx) - px            gy = (y - dy) - py
 *       wx = (c * gx + s * gy) + px   wy = (c * gy - s * gx) + py        w = (wx, wy, z).
 *    With pivot (0, 0), c = 1 and s = 0 this is w = (x - dx, y - dy, z) up to the sign of a zero,
 *    which no later step sees: a table whose rows all have theta = 0 gives exactly
 *    prh_align_score's integers.
 * Per slice, on the host (align.pick_pose): steps 6-10 with three changes.
 * 6'. The table must hold the pose (0, 0, 0); k0 is its first row.
 * 8'. Of the near-best rows (keep = 63 / 64, exact integers) the one with the smallest dx * dx + dy *
 *    dy + (lever * theta) * (lever * theta) in fp64, summed left to right, ties to the lowest row.
 *    lever (default 25 m, the half length of a slice) turns a yaw into the lateral move of a line end.
 * 9'. Bias.  With a lateral offset e0 and a yaw error phi a point at arc position t of a line (t
 *    from the pivot, uniform over |t| <= lever) lies e0 + phi t beside the paint; the mean of its
 *    square is e0^2 + phi^2 lever^2 / 3, so step 9's fall of the score reads (e0^2 + phi^2 lever^2 /
 *    3) / r^2 / (1 - w^2 / (3 r^2)) and keep = 63 / 64 bounds it by 1 / 64: |e0| <= 0.13 r as
 *    before and |phi| <= 0.13 r sqrt(3) / lever, 1.35 mrad at the defaults (r = 0.15, lever = 25),
 *    just above one fine yaw step.  Both pull towards zero.  At a line end 24 m out the residual is
 *    at most 0.13 r + 24 * 0.13 r sqrt(3) / lever + 24 * (half a fine yaw step) = 0.0195 + 0.0324 +
 *    0.012 = 0.064 m.
 * min_points (step 7) and gain (step 10) are unchanged.
 * Grids (align.pose_grid: the yaw index outer, then shift_grid's x outer, y inner).  Coarse:
 * shift_grid((0, 0), max_shift, 0.1) crossed with theta = j * 0.004, |theta| <= max_yaw (default
 * 0.02: 441 x 11 = 4851 rows).  Fine: shift_grid(coarse pick, 0.1, 0.02) crossed with coarse theta
 * + j * 0.001, |j| <= 4, the row (0, 0, 0) appended (1090 rows).  max_yaw = 0 gives the yaw grid {0}
 * in both stages, and the whole procedure is then align_lines' bit for bit.  scope = 'drive' as in
 * the shift rule.
 * Applying the pick (align.apply_pose), with gx = x - px, gy = y - py:
 *       x' = ((c * gx - s * gy) + px) + dx      y' = ((s * gx + c * gy) + py) + dy.
 * Reach (cost only, but conservative).  reach [S] fp64 = ((radius + m) + a * (rho + radius)) + 1e-6
 * with m = max_k max(|dx|, |dy|), a = max_k |theta| and rho the largest xy distance of a vertex of
 * the slice from its pivot.  A hitter's w lies within radius of a point c of a segment, so |w -
 * pivot| <= rho + radius (both ends of the segment are within rho of the pivot, and so is c); the
 * rotation moves w by 2 sin(|theta| / 2) |w - pivot| <= a (rho + radius) and the shift by at most
 * m per axis, so the unmoved x and y lie within reach of the box of the segment.  The 1e-6: every
 * operation of step 2' and of the projection works on magnitudes up to 2e6 + 4 and rounds by at
 * most ulp(2e6) / 2 = 1.2e-10; c and s carry 1.1e-16 relative each, 2.4e-10 at that magnitude; w
 * takes six operations, h four more, rho one square root: below 3e-9 in all, and 1e-6 is kept from
 * the shift rule with that margin.  With a = 0 the expression has slice_reach's bits.  The bitmaps
 * and prh_align_select_count / _write are used unchanged with this reach.
 *   prh_align_score_rigid   prh_align_score with the pose table and pivots [S,2]: the same work
 *                           item (slice, 256 candidates, 16 poses); a thread computes its 16 (wx,
 *                           wy) once from the pose rows, before the segment loop, and the loop is
 *                           prh_align_score's.  poses must be 16-byte aligned.
 *   prh_align_select_cells_count / _write   the select passes with one counter per bitmap cell:
 *                           cell_counts [n_cells] int32 (zeroed here); with cell_offsets [n_cells+1]
 *                           int64 their exclusive prefix (the caller scans), rows cell_offsets[c] ..
 *                           cell_offsets[c+1] of records are cell c's survivors in the order of
 *                           arrival.  Cells of a slice are contiguous from cell_base[s], so
 *                           cand_offsets[s] = cell_offsets[cell_base[s]] and the records stay
 *                           grouped by slice: a wave of the score kernel then holds neighbours on
 *                           the road.  The rule does not see the order: the tables are bitwise
 *                           equal either way.  PRH_ERR_WORKSPACE below
 *                           prh_align_select_cells_workspace_bytes(n_cells). */
int prh_align_max_poses(void);
size_t prh_align_select_cells_workspace_bytes(long long n_cells);
int prh_align_select_cells_count(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                                 long long n_points, const double* grid_origin, const int* grid_shape,
                                 const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                                 double intensity_floor, int* cell_counts, int device, void* stream);
int prh_align_select_cells_write(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                                 long long n_points, const double* grid_origin, const int* grid_shape,
                                 const long long* cell_base, const unsigned* bitmap, long long n_cells, double cell,
                                 double intensity_floor, const long long* cell_offsets, void* records,
                                 long long capacity, void* workspace, size_t workspace_bytes, int device,
                                 void* stream);
int prh_align_score_rigid(const void* records, const long long* cand_offsets, long long n_candidates,
                          const double* line_vertices, long long n_vertices, const long long* line_offsets, int n_lines,
                          const long long* slice_line_offsets, const double* poses, const long long* pose_offsets,
                          long long n_poses, const double* pivots, const double* reach, int n_slices,
                          const long long* items, long long n_items, double r2, long long* acc, int device,
                          void* stream);

/* Paint tracing - the rule.
 * Lane candidates read from the cloud itself: per slice, polylines along the bright ridges of its
 * points, with no detector and no GT.  The lines are 3-D and lie on the paint, so they go to the
 * slice refinement as they are, with no lift and no alignment.  The conventions are those of "Ground
 * lift - the rule" and "Paint alignment - the rule": fp64 throughout, one rounding per operation, no
 * contraction, every constant computed once on the host and passed in; the same bits go to the
 * device and to the oracle (tests/_trace_oracle.py).
 * Inputs.  points [T,4] = x y z intensity in the ego frame of their slice, float64 (is_double != 0,
 * what drive.slice_cloud returns) or float32, converted to fp64 first, which is exact.  slice_offsets
 * [S+1] int64; a slice has fewer than 2^22 points (the host raises ValueError).
 * Grid.  Columns along ego x: nx = rint(2 * half_length / col) (half_length 25.0, col 0.5: 100);
 * cells along y: ny = rint(2 * half_width / cell) (half_width 12.8, cell 0.05: 512); both computed
 * on the host, 1 <= nx, ny <= 4096, 0 < half_length, half_width <= 128.  ix = floor((x + half_length)
 * / col), iy = floor((y + half_width) / cell), decided on the floor in fp64; a point with ix outside
 * 0 .. nx - 1 or iy outside 0 .. ny - 1 is dropped (a non-finite x or y is).
 * Point weight.  Step 1 of the alignment rule: wI = min(max((double)I - intensity_floor, 0), 4096), qi
 * = (long long)rint(wI * 256), a non-finite I gives 0.  A point with a non-finite z, with |z| > 512
 * or with qi == 0 is dropped.  qx = (long long)rint(x * 1024), qy and qz likewise (half to even).
 * Tables.  Per (slice, ix, iy): n (int32, the points kept), w = sum qi, wx = sum qi * qx, wy = sum
 * qi * qy, wz = sum qi * qz (int64).  |x| < 3 * 128 and |z| <= 512 give |q| <= 2^19, qi <= 2^20, an
 * addend below 2^39, and with fewer than 2^22 points per slice three cells stay below 2^63.
 * Box.  b[iy] = w[iy-1] + w[iy] + w[iy+1] within the column, a cell outside 0 .. ny - 1 counting 0;
 * n3, bx, by, bz likewise from n, wx, wy, wz.  b of a cell outside the grid is 0.
 * Peak.  Cell (ix, iy) is a peak iff n3 >= min_points (default 3, >= 1), b >= min_weight (default
 * 1, >= 1) and for every k = 1 .. nms (default 4, 0 <= nms <= prh_trace_max_nms() = 31): b > b[iy-k]
 * and b >= b[iy+k].  The strict lower side makes the lower cell of a plateau the peak.  Its position
 * is x = ((double)bx / (double)b) / 1024.0, y and z likewise: the weighted centroid of the box.  The
 * peaks are ordered by (slice, ix, iy): peak_offsets [S*nx+1] is the CSR over all columns.
 * Links.  tol(dc) = link_cells + gap_slope * (dc - 1) in integers (defaults 3 and 1).  succ(p), p at
 * (ix, iy): the smallest dc in 1 .. max_gap_cols + 1 (default 24: 12 m, the gap of a dashed line)
 * for which column ix + dc of the same slice holds a peak with |iy' - iy| <= tol(dc); within that
 * column the peak with the smallest |iy' - iy|, of two the one with the smaller iy'; -1 where there
 * is none.  pred(q) is the mirror image towards lower columns.  The link p -> q exists iff succ(p)
 * == q and pred(q) == p; the outputs succ and pred hold mutual links only, -1 elsewhere.
 * Lines (host, trace.chain_lines).  The maximal chains of links; a chain is kept iff it has at least
 * min_peaks (3) peaks and x_last - x_first >= min_length (5.0 m) in fp64; the lines of a slice are
 * ordered by their head's (ix, iy); their vertices are the peaks' x y z.
 * Scope.  The rule follows ridges that run within about atan(link_cells * cell / col) of the ego x
 * axis (17 degrees at the defaults); stop lines and crosswalks are not traced.  Without an
 * intensity_floor that separates paint from asphalt it traces asphalt texture.  A point is taken
 * whatever its height, so bright things above the road are traced with the paint unless the surface
 * gate is on ("Paint tracing - the rule: surface gate", below).
 * All sums are integers, so the result does not depend on the order of the points, on their dtype,
 * on the chunking of the slices or on the launch shape: it is bitwise reproducible by construction.
 *   prh_trace_workspace_bytes  the tables of n_slices slices: n [C] int32 first, then w, wx, wy, wz
 *                         [C] int64, each on a 256-byte boundary, C = n_slices * nx * ny, cell (s,
 *                         ix, iy) at (s * nx + ix) * ny + iy; 0 for a shape outside the limits.  The
 *                         caller may cut its slices into chunks that fit its memory: the tables of
 *                         one chunk are filled, read by the two peak passes and dropped.
 *   prh_trace_hist        zeroes the workspace, then one thread per point of rows first_row ..
 *                         first_row + n_rows: slice_offsets [n_slices+1] holds the absolute rows of
 *                         the chunk's slices (slice_offsets[0] <= first_row, first_row + n_rows <=
 *                         slice_offsets[n_slices]).  x y in one load, z and I only inside the grid,
 *                         one 32-bit and four 64-bit integer atomics per kept point.
 *   prh_trace_peaks_count col_counts [n_slices*nx] int32: the peaks of every column.  One wave per
 *                         column; w goes through LDS 256 cells at a time with a halo of 32.
 *   prh_trace_peaks_write with col_offsets [n_slices*nx+1] int64 the exclusive prefix of col_counts
 *                         (the caller scans): rows col_offsets[c] .. col_offsets[c+1] of iy (int32),
 *                         weight = b (int64), count = n3 (int32), xyz [.,3] fp64 and col (int32:
 *                         col_base + c, the column's number among all chunks' columns) are column c's
 *                         peaks in ascending iy (ballot / popcount: no sort, no atomic).
 *   prh_trace_link        one thread per peak over all chunks: col_offsets [n_cols+1] with n_cols a
 *                         multiple of nx, iy and col as written above; succ and pred [n_peaks] int32.
 * points must be aligned to two coordinates (16 bytes for fp64, 8 for float32), the workspace to 256
 * bytes.  PRH_ERR_ARG for a parameter outside the limits above, PRH_ERR_WORKSPACE below
 * prh_trace_workspace_bytes; both before the device is touched.  No float atomics. */
int prh_trace_max_nms(void);
size_t prh_trace_workspace_bytes(int n_slices, int nx, int ny);
int prh_trace_hist(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long first_row,
                   long long n_rows, double half_length, double col, int nx, double half_width, double cell, int ny,
                   double intensity_floor, void* workspace, size_t workspace_bytes, int device, void* stream);
/* Paint tracing - the rule: surface gate.
 * A merged cloud holds bright things that are not paint - the plate and reflectors of a followed
 * vehicle smeared into a trail half a metre above the lane, guard-rail reflectors, signs and gantries
 * over the carriageway - and the weight min(I - floor, 4096) favours them.  With the gate the tables
 * see the points on the road surface only.  It is off unless asked for (trace.paint_peaks with a
 * ground table, trace.refine_cloud with surface=True); without it every bit is as above.  The
 * conventions are those of "Paint tracing - the rule" and "Paint floor - the rule": fp64, one
 * rounding per operation, no contraction, every constant computed once on the host and passed in;
 * tests/_trace_surface_oracle.py restates the gate.
 * Gate.  A point that passes every test of "Grid" and "Point weight" above (inside the trace grid, z
 * finite, |z| <= 512, qi > 0) is tested further.  gix = floor((x + g_half_length) / ground_cell), giy
 * = floor((y + g_half_width) / ground_cell): the expressions of "Paint floor - the rule: Surface
 * grid", decided on the floor in fp64, over ground [S,gx,gy] fp64, the road height of every cell, NaN
 * where there is none (paintfloor.surface_ground; 1 <= gx, gy <= 1024, g_half_length, g_half_width and
 * ground_cell positive and finite; trace.paint_peaks passes its own half_length and half_width and
 * ground_cell 1.0).  The point is off the surface iff gix lies outside 0 .. gx - 1, or giy outside 0
 * .. gy - 1, or g = ground[s][gix][giy] is NaN, or !(fabs(z - g) <= band); band 0.15
 * (paintfloor.BAND), finite and >= 0.  A point off the surface adds nothing to the tables and 1 to
 * off_surface[s] (int64).  The intensity clauses of the floor rule's "Surface point" do not apply:
 * qi > 0 has decided them already, and with a negative intensity_floor the two would disagree.
 * A point that fails an earlier test (outside the trace grid, a bad z, qi == 0) is dropped as
 * before and is not counted in off_surface.  Box, peak, links and lines are unchanged; all sums stay
 * integers, so the bits do not depend on point order, dtype, chunking or launch shape.
 * Scope.  The ground table has constant cells of ground_cell (1 m): the gate is as good as "Ground
 * lift - the rule" is on that cell.  A point outside the ground window is off the surface.  Paint on
 * a structure the ground rule does not call road - a bridge deck above the lowest mode of its cell -
 * is gated out with the structure.
 *   prh_trace_hist_surface  prh_trace_hist with the gate: its arguments up to workspace_bytes, then
 *                         the ground window and ground [n_slices][gx][gy], the rows of the chunk's
 *                         slices, band, and off_surface [n_slices], zeroed here.  The same point
 *                         function as prh_trace_hist, the gate compiled in: x y in one load, the
 *                         grid test, z and I, qi, and only then the ground cell and one fp64 gather
 *                         (bright points only), the band test, the five atomics.  off_surface is
 *                         reduced within the wave by ballot / popcount: one 64-bit integer atomic per
 *                         wave and slice touched.  PRH_ERR_ARG as prh_trace_hist and prh_floor_hist
 *                         give it, before the device is touched.  No float atomics. */
int prh_trace_hist_surface(const void* points, int is_double, const long long* slice_offsets, int n_slices,
                           long long first_row, long long n_rows, double half_length, double col, int nx,
                           double half_width, double cell, int ny, double intensity_floor, void* workspace,
                           size_t workspace_bytes, double g_half_length, double g_half_width, double ground_cell, int gx,
                           int gy, const double* ground, double band, long long* off_surface, int device, void* stream);
int prh_trace_peaks_count(void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny, int nms, int min_points,
                          long long min_weight, int* col_counts, int device, void* stream);
int prh_trace_peaks_write(void* workspace, size_t workspace_bytes, int n_slices, int nx, int ny, int nms, int min_points,
                          long long min_weight, const long long* col_offsets, long long capacity, int col_base, int* iy,
                          long long* weight, int* count, double* xyz, int* col, int device, void* stream);
int prh_trace_link(const long long* col_offsets, long long n_cols, int nx, const int* iy, const int* col,
                   long long n_peaks, int link_cells, int gap_slope, int max_gap_cols, int* succ, int* pred, int device,
                   void* stream);

/* Paint floor - the rule.
 * The intensity threshold between asphalt and paint, read from the cloud: what trace.paint_peaks,
 * align.paint_scores and support.node_support take as intensity_floor.  The conventions are those of
 * "Ground lift - the rule" and "Paint tracing - the rule": fp64 for geometry, one rounding per
 * operation, no contraction, every constant computed once on the host and passed in; all
 * accumulated quantities are integers, so nothing depends on point order, dtype, chunking or launch
 * shape.  tests/_floor_oracle.py restates the rule in plain Python.
 * Inputs.  points [T,4] = x y z intensity in the ego frame of their slice, float64 (is_double != 0)
 * or float32, converted to fp64 first, which is exact.  slice_offsets [S+1] int64, what
 * drive.slice_cloud returns; a slice holds fewer than 2^31 points.
 * Surface grid.  The window is |x| < half_length (25.0), |y| < half_width (12.8), in cells ground_cell
 * (1.0 m) wide: gx = ceil(2 * half_length / ground_cell), gy likewise, both on the host, 1 <= gx, gy
 * <= 1024.  ix = floor((x + half_length) / ground_cell), iy = floor((y + half_width) / ground_cell),
 * decided on the floor in fp64; a point with ix outside 0 .. gx - 1 or iy outside 0 .. gy - 1 is
 * dropped (a non-finite x or y is).  ground [S,gx,gy] fp64 is the road height of every cell, NaN where
 * there is none; the host fills it with one call of "Ground lift - the rule" (ground.ground_heights)
 * whose queries are the cell centres (-half_length + (ix + 0.5) * ground_cell, -half_width + (iy +
 * 0.5) * ground_cell), with radius = ground_radius (0.75, which covers the cell's corners) and
 * ground's own defaults otherwise.
 * Surface point.  A point is a surface point iff its cell's ground g is not NaN, z is finite and
 * fabs(z - g) <= band (0.15), and I is finite and I >= 0 (-0.0 is).
 * Histogram.  fb = floor(I / bin_width); the bin is n_bins - 1 if fb >= n_bins, else (int)fb - the
 * comparison is made in fp64 before the conversion, so 1e30 clamps.  n_bins 256, 2 <= n_bins <=
 * prh_floor_max_bins() = 1024; bin_width 1.0, positive and finite.  hist[s][b] (int64) counts the
 * surface points of slice s.
 * Threshold of one histogram row h[0 .. n-1] (a count below 0 counts as 0).  r[b] = isqrt(h[b]), the
 * exact integer floor square root: Otsu's rule over the raw counts cuts the asphalt in half once the
 * paint is below about 2 % of the surface points, over the square roots it stays between the two
 * populations.  Wr = sum r, Mr = sum b * r, W = sum h.  For t = 1 .. n - 1: w0 = sum_{b<t}
 * r, m0 = sum_{b<t} b * r, w1 = Wr - w0, m1 = Mr - m0, and over the raw counts c0 = sum_{b<t} h, c1 =
 * W - c0.  t is a candidate iff c0 >= min_points and c1 >= min_points (16, >= 1) and w0 > 0 and w1 >
 * 0.  Its score, in fp64 in exactly this order: d = (double)m1 / (double)w1 - (double)m0 /
 * (double)w0; p = (double)w0 * (double)w1; score = p * (d * d).  t_lo is the smallest candidate with
 * the largest score, provided that score is > 0.  t_hi is the largest t >= t_lo such that every u
 * in t_lo .. t is a candidate with a score equal to score(t_lo): the plateau - between two separated
 * populations the sums do not change, so the bits are equal.  t* = (t_lo + t_hi) >> 1 and floor =
 * (double)t* * bin_width.  A row with no candidate, or with a largest score of 0, has no floor: t_lo
 * = t_hi = t* = -1, and above, w0, m0 and score are 0.
 * Drive floor.  The row that is the integer sum of all slice rows goes through the same kernel as
 * one more row; paintfloor.paint_floor returns that row's floor, the slices' own go into its report.
 * Scope.  The rule always splits: a road with no paint still gets a floor.  paint_share = c1 / W and
 * contrast = mu1 - mu0 (the means, in intensity units, of the raw counts at and above t* and below
 * it, computed on the host) are reported so the caller can judge; nothing is gated on them.
 * Intensity is taken as it is: there is no range or incidence correction.
 *   prh_floor_hist   zeroes hist [n_slices][n_bins], then reads rows 0 .. n_rows (n_rows <=
 *                    slice_offsets[n_slices]) once: blocks of 256 threads walk 2048 rows each, x y in
 *                    one load, z and I only inside the window, one fp64 gather from ground, one LDS
 *                    atomic on the block's private histogram of its first slice (a point of another
 *                    slice in a block that straddles a boundary goes to hist itself), and the
 *                    non-zero bins are flushed with 64-bit integer atomics.
 *   prh_test_floor_hist   the same with 1, 2, 4 or 8 lane-interleaved LDS copies of the block's
 *                    histogram: the same bits, for the measurement that chose prh_floor_hist's count.
 *   prh_floor_otsu   one wave per row of hist [n_rows][n_bins] (any int64 rows, slice or drive):
 *                    t_lo, t_hi, t (int32), total = W, above = c1 at t*, w0, m0 at t_lo, wr, mr
 *                    (int64) and score (fp64), each [n_rows].  No atomics.
 * points must be aligned to two coordinates (16 bytes for fp64, 8 for float32).  PRH_ERR_ARG for a
 * parameter outside the limits above, before the device is touched.  No float atomics. */
int prh_floor_max_bins(void);
int prh_floor_hist(const void* points, int is_double, const long long* slice_offsets, int n_slices, long long n_rows,
                   double half_length, double half_width, double ground_cell, int gx, int gy, const double* ground,
                   double band, double bin_width, int n_bins, long long* hist, int device, void* stream);
int prh_test_floor_hist(int copies, const void* points, int is_double, const long long* slice_offsets, int n_slices,
                        long long n_rows, double half_length, double half_width, double ground_cell, int gx, int gy,
                        const double* ground, double band, double bin_width, int n_bins, long long* hist, int device,
                        void* stream);
int prh_floor_otsu(const long long* hist, int n_rows, int n_bins, long long min_points, int* t_lo, int* t_hi, int* t,
                   long long* total, long long* above, long long* w0, long long* m0, long long* wr, long long* mr,
                   double* score, int device, void* stream);

/* Row f1, query side of DetrTransformerDecoderLayer (src/model.py:117,128,133):
 *   y = LayerNorm(x + dropout(r)), nn.LayerNorm(256) semantics (eps, biased variance, affine),
 * rows x 256 fp32, one pass forward and one backward.  The dropout decision is a counter hash of
 * (seed, row, channel) - same distribution as nn.Dropout, not the same mask; dropout_p = 0 in
 * eval mode.  mean/rstd [rows] are saved by the forward for the backward (NULL = not kept).
 * The backward also produces dgamma / dbeta (sums over rows). */
int prh_add_dropout_layernorm_forward(const float* x, const float* r, const float* gamma, const float* beta,
                                      long rows, int channels, float eps, float dropout_p, unsigned seed,
                                      float* y, float* mean, float* rstd, int device, void* stream);
size_t prh_add_dropout_layernorm_workspace_bytes(void);
int prh_add_dropout_layernorm_backward(const float* dy, const float* x, const float* r, const float* gamma,
                                       const float* mean, const float* rstd, long rows, int channels,
                                       float dropout_p, unsigned seed, float* dx, float* dr, float* dgamma,
                                       float* dbeta, void* workspace, size_t workspace_bytes, int device,
                                       void* stream);

/* Row f3.  Deep-supervision L1 loss with its gradient in one pass (train.py:63-68,
 * train_dist.py:180-186: (1/L) sum_l nn.L1Loss(pred_l, target)):
 *   *loss (+)= sum_{l,e} |pred[l,e] - target[e]| / denom      d_pred[l,e] = sign(.) / denom
 * pred [n_layers, elems], target [elems]; denom = n_layers * elems of the full batch (a
 * micro-batched caller passes the full-batch denominator and accumulate = 1 from the second
 * chunk on); d_pred may be NULL.  loss is a device scalar.
 * geometry (device float[2] or NULL; elems must be xyz triples): the metrics the reference logs
 * every step (train_dist.py:190-203): [0] (+)= sum over points |target| / points (initial
 * point-to-point error), [1] (+)= sum |pred_last - target| / points (refined error). */
size_t prh_l1_loss_workspace_bytes(void);
int prh_l1_loss(const float* pred, const float* target, int n_layers, long elems, double denom,
                int accumulate, float* loss, float* d_pred, float* geometry, double points,
                void* workspace, size_t workspace_bytes, int device, void* stream);

/* torch.optim.Adam step (amsgrad off; train.py:40, train_dist.py:150) over flat, 16-byte
 * aligned fp32 buffers of n elements; step counts from 1. */
int prh_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, int device,
                  void* stream);

/* prh_attn_backward that also reports, per wave, the largest |dV| and |dK| it stored:
 * kv_amax_part [B*(H/4)*4][2] (or NULL) - reduced by the caller, it bounds the gradient operand
 * of the K/V projection's backward GEMMs (prh_linear_backward_ex dy_amax). */
int prh_attn_backward_ex(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv,
                         const float* o, long ldo, const float* lse, const float* dout, long lddo,
                         float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, int B, int M,
                         int N, int H, float scale, float dropout_p, unsigned seed, float* kv_amax_part,
                         int device, void* stream);

/* GEMM core selection (environment PRH_GEMM, or prh_set_gemm_mode at run time):
 *   split16 / 3 (default): large GEMMs on the split-fp16 cores - two fp16 planes per fp32 operand
 *            placed by a power-of-two scale from the operand's largest magnitude, three
 *            v_mfma_f32_16x16x32_f16 / 32x32x16 products, fp32 accumulation, fp32-level error;
 *   split / 1: split-bf16 cores - three bf16 planes, six v_mfma_f32_32x32x16_bf16 products,
 *            fp32-level error with no range assumption;
 *   fp32 / 0: the exact fp32 MFMA cores (v_mfma_f32_32x32x2_f32) everywhere.
 * All three are checked against the oracle at the same 1e-4 gate.
 *   bf16 / 2: opt-in REDUCED-PRECISION mode: plain bf16 operands, one MFMA product on the
 *            first-generation cores, fp32 accumulate and fp32 storage; parity gate 5e-2, not 1e-4.
 *   bf16s / 4: BASELINE config 3 ("bf16 training"): bf16 operands AND bf16 activation storage.
 *            The encoder and the Linear fed by it go through the *_bf16 entry points above; plain
 *            fp32-storage Linears of at least 512 x 64 x 64 run on the same bf16 core with their
 *            input converted in flight; everything else behaves as mode 2.  Parity gate 5e-2.
 * The mode is process-wide; set it before launching work, not concurrently with it, and keep
 * it unchanged between a forward call and its backward. */
int prh_set_gemm_mode(int mode);
int prh_get_gemm_mode(void);

/* Dropout under graph replay.  The attention and LayerNorm entry points take their dropout seed
 * as a host value, which a captured graph would freeze.  Register a device word here (process-
 * wide, like the GEMM mode; NULL = none): every dropout decision then hashes seed ^ f(*word),
 * read at kernel run time, so a caller that advances the word on the device before each replay
 * gets fresh masks while forward and backward of one step still agree. */
int prh_set_dropout_seed_source(const unsigned* device_word);

/* Raw GEMM cores, exported for the unit tests (tests/test_gemm_gpu.py).
 *   nt: c[m,n] = a[m,k] w[n,k]^T     tn: c[mo,ni] = a[p,mo]^T b[p,ni]          */
int prh_test_gemm_nt(const float* a, const float* w, float* c, int m, int n, int k,
                     void* workspace, size_t workspace_bytes, int device, void* stream);
size_t prh_test_gemm_tn_workspace_bytes(int p, int mo, int ni);
/* Step (1) of prh_encoder_backward on its own (tests/test_gate_recompute_gpu.py), without a pooled gradient:
 * d_fused [P, out_dim] becomes dy_f in place, gate [P, out_dim] (recompute == 0: the forward's gate on entry;
 * != 0: uninitialised) becomes dG, ws_a / ws_b [ceil(P/64), out_dim] take the BatchNorm-backward partials
 * (sum dy, sum dy * z_fus per 64-row block).  bn_scale / bn_shift [out_dim]: the fusion BatchNorm. */
size_t prh_test_gate_backward_workspace_bytes(int out_dim);
int prh_test_gate_backward(const float* ctx, int B, int N, int in_channel, int out_dim, const float* gate_w1,
                           const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* z_fus,
                           const float* bn_scale, const float* bn_shift, float* d_fused, float* gate, int recompute,
                           float* ws_a, float* ws_b, void* workspace, size_t workspace_bytes, int device, void* stream);
int prh_test_gemm_tn(const float* a, const float* b, float* c, float* colsum, int p, int mo,
                     int ni, void* workspace, size_t workspace_bytes, int device, void* stream);
/* The tn core with a BatchNorm-backward apply pass, dy[rows,cols] <- ka*dy + kb*z + kc in place:
 * side != 0 carried inside the wgrad launch (split-fp16 mode, transposed-read core; an error
 * elsewhere), side == 0 as the stand-alone pass ahead of the plain wgrad.  amax_out (device
 * float): largest |dz|.  cols, lddy, ldz multiples of 4. */
size_t prh_test_gemm_tn_side_workspace_bytes(int p, int mo, int ni);
int prh_test_gemm_tn_side(const float* a, const float* b, float* c, float* colsum, int p, int mo,
                          int ni, float* dy, long lddy, const float* z, long ldz, const float* ka,
                          const float* kb, const float* kc, long rows, int cols, int side,
                          float* amax_out, void* workspace, size_t workspace_bytes, int device,
                          void* stream);
/* The same (same workspace), reaching the rest of the carrier: qa / qb [ni] (device, both or
 * neither) make the B operand relu(qa * b + qb), the wgrad of a layer behind BatchNorm + ReLU.
 * period: k-tiles between two items of a thread's walk over the carried pass - 0 as the library
 * plans it, 1 / 2 / 4 forced (whatever the k-loop does not reach is drained behind it; the
 * results do not depend on the period).  *period_used (host, may be NULL): the period the
 * carrier ran with, 0 where nothing was carried (side == 0). */
int prh_test_gemm_tn_side_ex(const float* a, const float* b, float* c, float* colsum, int p, int mo,
                             int ni, const float* qa, const float* qb, float* dy, long lddy,
                             const float* z, long ldz, const float* ka, const float* kb,
                             const float* kc, long rows, int cols, int side, int period,
                             int* period_used, float* amax_out, void* workspace,
                             size_t workspace_bytes, int device, void* stream);

/* Raw second-stage reductions, exported for the unit tests (tests/test_ordered_reductions_gpu.py).
 * Each goes through the launcher the library itself calls, so a test runs the library's grid.
 * Every output is an ordered sum: its additions, their order and their precision are a contract
 * (DESIGN.md section 4), restated in tests/test_ordered_reductions_cpu.py.
 *   slabs        out[rows,cols] (ld ldout) = sum_s slab[s][rows*cols]; with cslab,
 *                cout[ccols] = sum_s cslab[s][ccols] in the same launch.  fp64, s = 0..S-1.
 *   bn_stage1    partials ws_a / ws_b [r][ld] -> out[32 slices][3][n] doubles:
 *                forward (count, sum, M2 about the slice mean), backward (sum a, sum b, 0).
 *   partials     out_a[n] = sum_i ws_a[i][n], out_b likewise (ws_b, out_a, out_b may be NULL).
 *   ln_param_grad      dgamma[256] = sum_i part_g[i][256], dbeta likewise.
 *   pos_hidden_final   part[nblk][4*hidden] -> dw0[hidden,3], db0[hidden] (either may be NULL).
 *   partial_rows_final part[nblk][n_el] -> out0[n0], out1[n_el - n0] (either may be NULL).
 *   act_amax     amax_out[0] = max over columns of max(relu(mx*scale+shift), relu(mn*scale+shift))
 *                with mx / mn the column maxima / minima of ws_c / ws_d [r][ld].
 * prh_test_reduce_depth(kind): how many loads a lane of that kernel keeps in flight. */
enum {
  PRH_REDUCE_SLABS = 0, PRH_REDUCE_BN_STAGE1 = 1, PRH_REDUCE_PARTIALS = 2, PRH_REDUCE_LN_PARAM_GRAD = 3,
  PRH_REDUCE_FINAL = 4, PRH_REDUCE_ACT_AMAX = 5
};
int prh_test_reduce_depth(int kind);
int prh_test_reduce_slabs(const float* slab, int s, int rows, int cols, float* out, long ldout,
                          const float* cslab, int ccols, float* cout, int device, void* stream);
int prh_test_reduce_bn_stage1(const float* ws_a, const float* ws_b, int r, long ld, int n,
                              int tile_rows, int p, int forward, double* out, int device,
                              void* stream);
int prh_test_reduce_partials(const float* ws_a, const float* ws_b, int r2, int n, float* out_a,
                             float* out_b, int device, void* stream);
int prh_test_reduce_ln_param_grad(const float* part_g, const float* part_b, int nb, float* dgamma,
                                  float* dbeta, int device, void* stream);
int prh_test_reduce_pos_hidden_final(const float* part, int nblk, int hidden, float* dw0,
                                     float* db0, int device, void* stream);
int prh_test_reduce_partial_rows_final(const float* part, int nblk, int n_el, float* out0, int n0,
                                       float* out1, int device, void* stream);
size_t prh_test_reduce_act_amax_workspace_bytes(void);
int prh_test_reduce_act_amax(const float* ws_c, const float* ws_d, int r, long ld, int n,
                             const float* scale, const float* shift, float* amax_out,
                             void* workspace, size_t workspace_bytes, int device, void* stream);

/* Diagnostic: which XCD (XCC_ID) and CU (HW_ID) each workgroup of a `blocks` x 512-thread
 * launch with `lds_bytes` of dynamic LDS lands on; out[2*b] = XCC_ID, out[2*b+1] = HW_ID.
 * The GEMM kernels assume workgroup b runs on XCD b % 8 (xcd_remap); this checks it. */
int prh_test_xcc_map(int blocks, int lds_bytes, int* out, int device, void* stream);

/* Optional launch profiler used by bench.py: when enabled (capacity > 0) every GEMM launch is
 * bracketed by HIP events on the launch stream; prh_profile_read returns its duration and
 * the algorithmic FLOPs / bytes of that launch.  capacity 0 disables and frees the events. */
int prh_profile_enable(int capacity);
int prh_profile_count(void);
int prh_profile_reset(void);
int prh_profile_read(int i, char* name, int name_len, float* ms, double* flops, double* bytes);

const char* prh_last_error(void);
const char* prh_version(void);

#ifdef __cplusplus
}
#endif
#endif
