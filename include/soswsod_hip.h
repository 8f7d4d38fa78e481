/*
 * soswsod_hip.h — C ABI of the MI355X-native (gfx950) kernels behind SoS-WSOD's Stage-1 OICR+ hot path.
 *
 * The reference has no C FFI on this path: its operator boundary is a pybind11 module called from
 * torch.autograd.Function (uwsod/projects/WSL/wsl/layers/roi_loop_pool.py:9-35 <->
 * uwsod/projects/WSL/wsl/layers/csrc/vision.cpp:21-23 <-> .../ROILoopPool/ROILoopPool.h:48-107), plus the
 * third-party ops it calls (torchvision RoIPool / nms, cuDNN conv, cuBLAS GEMM).  This header is the plain-C
 * replacement of that operator tier; each entry cites the reference code it stands in for.
 *
 * Conventions (all entry points):
 *   - extern "C", return 0 on success, a positive hipError_t from the launch, or a negative argument error
 *     (-1 bad dtype, -2 split-K without atomic accumulate, -3 unsupported operand layout, -4 pointer not
 *     16-byte aligned, -5 leading dimension / extent not a multiple of the 16-byte chunk, -6 size limit).
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated, freed or synchronised
 *     inside; work is enqueued on `stream`; no global state => thread-compatible.
 *   - dtype: SW_F32 (0) or SW_BF16 (1; raw 16-bit words).  Activations are NHWC.
 */
#ifndef SOSWSOD_HIP_H
#define SOSWSOD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef SW_F32
#define SW_F32 0
#define SW_BF16 1
#endif

typedef struct ihipStream_t* sw_stream_t; /* == hipStream_t */

/* Fused GEMM / implicit-GEMM epilogue:  v = acc (+bias[n]); relu; dropout; relu-backward mask; store. */
typedef struct sw_epilogue {
  const float* bias;          /* [N] or NULL */
  int relu;                   /* v = max(v, 0) */
  const uint8_t* drop_mask;   /* [M][ld_drop] keep mask or NULL: v = keep ? v*drop_scale : 0   (F.dropout, box_head.py:90) */
  long ld_drop;
  float drop_scale;
  const void* relu_ref;       /* [M][ld_ref] or NULL: v = ref>0 ? v*ref_scale : 0   (ReLU(+dropout) backward) */
  long ld_ref;
  float ref_scale;
  int ref_dtype;
  int out_dtype;              /* dtype of C */
  int accumulate_atomic;      /* C is f32 and is atomically accumulated (required when splitk > 1) */
  float* absmax_out;          /* optional device scalar (caller zero-fills): atomicMax of |stored value| (sw_gemm only) */
  /* in-epilogue dropout (drop_mask == NULL, drop_hash_p > 0): element (m, n) is kept iff the keep mask that
   * sw_dropout_mask(seed, offset, p) writes at index m*N + n is 1 — the same Bernoulli stream without the mask tensor */
  uint64_t drop_seed, drop_offset;
  float drop_hash_p;
  /* optional DEVICE counter added to drop_offset when the kernel runs: the stream position then lives on the device
   * (sw_counter_add advances it in-stream), so a captured hipGraph replays with a fresh dropout mask every time */
  const uint64_t* drop_offset_dev;
  /* deterministic split-K (sw_gemm, f32 C, no other epilogue option): every K-split stores its partial tile into its own
   * slab of this workspace (sw_gemm_splitk_workspace_floats floats), a second kernel adds the slabs in fixed order into C
   * (overwritten) — no atomics.  Also used, when given, for the tail peel of the large f32-output GEMMs (see sw_gemm).
   * With OTHER epilogue options set (bias, residual, relu, relu_ref, out_dtype bf16; not the dropout / atomic / absmax ones) and
   * effective splits > 1 the slabs stay plain f32 and the fold applies the epilogue in the GEMM's own order:
   * x = fold_row_scale[m] * sum + bias[n] + residual[m][n]; ReLU; ReLU-mask; convert.  An f32 residual may be C itself (C += A B: a
   * gradient added to one that exists).  One slab is legal when fold_row_scale meets a residual.  Requires N % 4 == 0, ldc % 4 == 0. */
  float* splitk_workspace;
  /* residual [M][ld_res] or NULL (dtype res_dtype): v = v + bias + residual before the ReLU — the shortcut add of a ResNet
   * bottleneck (detectron2/modeling/backbone/resnet.py:205-212 `out += shortcut; out = F.relu_(out)`) inside the 1x1 conv3 GEMM */
  const void* residual;
  long ld_res;
  int res_dtype;
  /* deterministic split-K only (splitk_workspace given, effective splits > 1): the ordered fold writes C[m][n] = fold_row_scale[m] *
   * sum of the slabs (DEVICE [M] or NULL) — the FrozenBN fold of a 1x1 convolution's weight gradient, dW = scale * dW_eff
   * (detectron2/layers/batch_norm.py:52-58), without a pass of its own.  Without a fold (one split, plain f32 C) it runs as a
   * row-scaling pass after the GEMM; sw_gemm returns -5 for any other combination that does not end in a fold. */
  const float* fold_row_scale;
  /* Fused SGD update (round 6; sw_gemm only, bf16 operands, f32 "output", no other epilogue option, the 256x256 ping-pong tile: K-contiguous
   * A, M % 32 == 0, N % 64 == 0 — sw_gemm_sgd_fused_supported answers for a shape): C = A B is the GRADIENT of the [M][N] float32 parameter
   * sgd_fused->param (row pitch = ldc; stage_kind 3: row-major copy stage0 [M][ld0] and transposed copy stage1 [N][ld1], bf16).  The
   * epilogue applies torch.optim.SGD's momentum update (sw_sgd_multi's arithmetic, bit for bit) to the parameter, its momentum buffer and
   * both copies; the gradient is NOT written, except the peeled tail columns (see sw_gemm), which go through C and the tiled update kernel.
   * What it removes: the 411 MB write + read of fc1.weight's gradient and a serialized HBM-bound optimizer launch (the reference:
   * optimizer.step() after the backward, train_net_multi.py:157-164; single GPU, ITER_SIZE 1 only — a data-parallel step needs the
   * all-reduced gradient).  sgd_fused->grad, ->n, ->d1, ->d2 are ignored; ->d0 must equal N. */
  const struct sw_sgd_tensor_s* sgd_fused;
  float sgd_momentum, sgd_grad_scale;
} sw_epilogue;

/* ---- dense contractions (reference: cuBLAS via torch Linear — box_head.py:88-90,
 *      fast_rcnn_wsddn.py:558-559, fast_rcnn_oicr.py:517-519, and their autograd backward) ----------------
 * C[m][n] = sum_k A(m,k) B(k,n).  a_kstrided=0: A[m*lda+k], 1: A[k*lda+m];  b_kstrided=0: B[n*ldb+k], 1: B[k*ldb+n].
 * Supported (a,b): (0,0) forward, (0,1) data gradient, (1,1) weight gradient. */
int sw_gemm(int dtype, int a_kstrided, int b_kstrided, int M, int N, int K, const void* A, long lda, const void* B,
            long ldb, void* C, long ldc, const sw_epilogue* ep, int splitk, sw_stream_t stream);
/* floats of sw_epilogue.splitk_workspace that sw_gemm(M, N, K, splitk) may use (its own tail peel included) */
long sw_gemm_splitk_workspace_floats(int M, int N, int K, int splitk);

/* ---- 3x3 convolution, stride 1, padding = dilation (reference: torch Conv2d/cuDNN, wsl/modeling/backbone/vgg.py:44-97,104-122)
 * in  [nimg][H][W][Cin], wk [Cout][3*3][Cin] (see sw_conv_weight_prep), out [nimg][H][W][Cout].
 * Used for forward (ep: bias+relu) and for the data gradient (wk = flipped/transposed weights, ep: relu_ref). */
int sw_conv3x3_igemm(int dtype, int nimg, int H, int W, int Cin, int Cout, int dilation, const void* in,
                     const void* wk, void* out, const sw_epilogue* ep, sw_stream_t stream);
/* 3x3 convolution (stride 1, dilation 1, bf16, Cin % 32 == 0 and >= 64, Cout % 64 == 0) + bias + ReLU + 2x2 / stride-2 max pool as ONE
 * launch; out_pooled [nimg][(H-2)/2+1][(W-2)/2+1][Cout].  For layers nothing differentiates through (vgg.py:104-122 below FREEZE_AT):
 * the unpooled map is never written.  Returns 1 = launched, 0 = not covered (run sw_conv3x3_igemm + sw_maxpool2x2_fwd), < 0 error;
 * bit-identical to that pair. */
int sw_conv3x3_relu_pool2(int dtype, int nimg, int H, int W, int Cin, int Cout, const void* in, const void* wk, const float* bias,
                          void* out_pooled, sw_stream_t stream);
/* n stride-1, dilation-1 3x3 convolutions of different maps (and possibly different weights) in ONE launch of the direct kernel:
 * the FPN levels of a detector (reference: the per-level loops of detectron2/modeling/proposal_generator/rpn.py:118-133 and
 * detectron2/modeling/backbone/fpn.py:131-160).  `probs` is a HOST array, n <= 8; every epilogue like sw_conv3x3_igemm's (bias,
 * relu, relu_ref; bf16 only).  Returns 1 = launched, 0 = a problem is not covered (launch them one by one), < 0 = error. */
typedef struct sw_conv_problem {
  int32_t nimg, H, W, Cin, Cout;
  const void* in; const void* wk; void* out;
  const sw_epilogue* ep;
} sw_conv_problem;
int sw_conv3x3_multi(int dtype, int n, const sw_conv_problem* probs, sw_stream_t stream);
/* dW (OIHW f32) from x [nimg][H][W][Cin] and dy [nimg][H][W][Cout]: dw = (accumulate ? dw : 0) + cout_scale[co] * sum.  workspace: at
 * least sw_conv3x3_wgrad_workspace_floats(...) floats: every K-split stores its partial [co][tap][ci] tile into its own slab (plain
 * stores), a second kernel adds the slabs in fixed order, scales and permutes to OIHW (deterministic).  cout_scale (DEVICE [Cout]
 * or NULL): the FrozenBN fold of a 3x3 convolution's weight gradient.  accumulate != 0: the second use of a convolution inside one
 * backward pass (the Stage-3 student runs two forward passes per iteration; unbias/ubteacher/engine/trainer.py:527-538 leaves that
 * sum to autograd). */
long sw_conv3x3_wgrad_workspace_floats(int dtype, int nimg, int H, int W, int Cin, int Cout, int splitk);
int sw_conv3x3_wgrad(int dtype, int nimg, int H, int W, int Cin, int Cout, int dilation, const void* x, const void* dy,
                     float* dw_oihw, float* workspace, int splitk, const float* cout_scale, int accumulate, sw_stream_t stream);
/* the same weight gradient (dilation 1) for maps of a few pixels (nimg * H * W <= 4096: FPN p5 / p6 of small images, below the tile
 * geometry of the MFMA loader: sw_conv3x3_wgrad returns -6 there): one thread per (co, ci), plain f32 sums in pixel order. */
int sw_conv3x3_wgrad_small(int dtype, int nimg, int H, int W, int Cin, int Cout, const void* x, const void* dy,
                           const float* cout_scale, float* dw_oihw, int accumulate, sw_stream_t stream);
/* The second half of sw_conv3x3_wgrad on its own: adds `nslab` consecutive slabs (Cout*9*Cin floats each, as sw_conv3x3_wgrad's
 * K-splits write them) in fixed order into dW (OIHW), with cout_scale and accumulate as above.  Several problems with the same weight
 * (the (x, dy) pairs written by sw_conv3x3_wgrad_grouped: the views of one iteration, or the RPN head's convolution on 5 FPN levels in
 * each of the student's two passes, rpn.py:118-133) put their slabs back to back and share ONE fold: the sum that autograd would
 * otherwise form with one add per parameter. */
int sw_conv3x3_wgrad_fold(int Cin, int Cout, int nslab, const float* workspace, float* dw_oihw, const float* cout_scale,
                          int accumulate, sw_stream_t stream);
/* ALL weight gradients of a backward pass in ONE launch: problem i writes the slabs of sw_conv3x3_wgrad(..., splitk = nsplit)
 * (sw_conv3x3_wgrad_workspace_floats(...) floats at `slabs`), computed by resident workgroups walking the
 * (problem, split, tile) list — instead of one launch of 128x128 tiles per layer and view, each cut into many K-splits to fill the
 * chip.  bf16 lists whose every problem has Cin % 64 == 0, Cout % 64 == 0, dilation 1 or 2, H >= 8 and >= 8 strip rows per split run
 * the direct weight-gradient kernel (conv_wgrad_direct.hip: an input row staged once for all nine taps; the splits are ranges of
 * (image, 32-pixel strip, row) steps — same slab count and layout, another order of additions inside a slab); every other list the
 * implicit GEMM on 256x256 tiles.  `problems` is a HOST array.  Fold with sw_conv3x3_wgrad_fold. */
typedef struct {
  int nimg, H, W, Cin, Cout, dilation, nsplit;
  const void* x;      /* [nimg][H][W][Cin] */
  const void* dy;     /* [nimg][H][W][Cout] */
  float* slabs;
} sw_wgrad_problem;
int sw_conv3x3_wgrad_grouped(int dtype, int n_problems, const sw_wgrad_problem* problems, sw_stream_t stream);
/* The same resident-grid launch for a list of PLAIN weight-gradient GEMMs, slabs[z][M][N] = sum over the z-th K range of
 * A[k][m] * B[k][n] (A [K][lda], B [K][ldb], both K-strided; M, N, lda, ldb multiples of 16 bytes): the 1x1 convolutions of a ResNet
 * bottleneck (reference: autograd's conv2d backward, detectron2/modeling/backbone/resnet.py:155-213) — several weights, each used
 * by every forward pass of an iteration.  `problems` is a HOST array.  sw_gemm_kk_grouped_slabs(dtype, K, nsplit) = slabs a problem
 * writes.  Fold with sw_splitk_fold_multi. */
typedef struct sw_gemm_kk_problem {
  const void* A; const void* B; float* slabs;
  int32_t M, N, K, nsplit;
  long lda, ldb;
} sw_gemm_kk_problem;
int sw_gemm_kk_grouped(int dtype, int n_problems, const sw_gemm_kk_problem* problems, sw_stream_t stream);
long sw_gemm_kk_grouped_slabs(int dtype, int K, int nsplit);
/* n ordered slab folds in ONE launch: C[m][n] = (accumulate ? C[m][n] : 0) + row_scale[m] * sum_z workspace[z][m][n] (row_scale
 * DEVICE [M] or NULL; N % 4 == 0, ldc % 4 == 0, 16-byte aligned).  `folds` is a HOST array. */
typedef struct sw_splitk_fold { int32_t M, N, nslab, accumulate; const float* workspace; float* C; long ldc; const float* row_scale; } sw_splitk_fold;
int sw_splitk_fold_multi(int n, const sw_splitk_fold* folds, sw_stream_t stream);
/* n folds (sw_conv3x3_wgrad_fold without scale, overwriting) in ONE launch; `folds` is a HOST array */
typedef struct { int Cin, Cout, nslab; const float* workspace; float* dw_oihw; } sw_wgrad_fold;
int sw_conv3x3_wgrad_fold_multi(int n, const sw_wgrad_fold* folds, sw_stream_t stream);
/* OIHW f32 master weights -> kernel layout.  mode 0: wk[co][tap][ci_pad] (forward, ci zero padded to cin_pad);
 * mode 1: wk[ci][8-tap][co] (data gradient: taps flipped, in/out swapped). */
int sw_conv_weight_prep(int dtype, int mode, int Cout, int Cin, int cin_pad, const float* w_oihw, void* wk,
                        sw_stream_t stream);

/* ---- 2x2 max pooling, stride 1 or 2, no padding (reference: nn.MaxPool2d, vgg.py:99-100,119-120) --------- */
int sw_maxpool2x2_fwd(int dtype, int nimg, int H, int W, int C, int stride, const void* in, void* out,
                      sw_stream_t stream);
/* din = route(dout) to the first max of each window (scan order, strict >), times (in > 0) when relu_mask. */
int sw_maxpool2x2_bwd(int dtype, int nimg, int H, int W, int C, int stride, const void* in, const void* dout,
                      void* din, int relu_mask, sw_stream_t stream);

/* ---- image normalisation (reference: MultiInputRCNN.preprocess_image, rcnn_multi.py:256-269) -------------
 * img u8 [3][H][W] -> out [H][W][cpad] = (img - mean) / std, channels >= 3 zero.
 * mean3/std3 are HOST float[3] (configuration constants, passed by value into the launch). */
int sw_preprocess(int dtype, int H, int W, int cpad, const uint8_t* img_chw, const float* mean3,
                  const float* std3, void* out_nhwc, sw_stream_t stream);
/* The same for n images of one size in ONE launch (a view batch): imgs_chw = HOST array of n device pointers,
 * out_nhwc [n][H][W][cpad]. */
int sw_preprocess_multi(int dtype, int n, int H, int W, int cpad, const uint8_t* const* imgs_chw, const float* mean3,
                        const float* std3, void* out_nhwc, sw_stream_t stream);

/* ---- max ROI pooling (reference: torchvision.ops.RoIPool called at wsl/modeling/poolers.py:183-186,267-270;
 *      arithmetic as stated in wsl/layers/csrc/ROILoopPool/ROILoopPool_cpu.cpp:26-79 fwd, :98-123 bwd) -------
 * feat [nimg][H][W][C]; rois [R][5] f32 (batch, x1,y1,x2,y2); out [R][C][PH][PW] (reference flatten order),
 * argmax [R][C][PH][PW]: argmax_bits == 32 -> int32 (h*W+w or -1, the reference's tensor); argmax_bits == 16 ->
 * uint16 (h*W+w or 0xFFFF; maps of < 65535 pixels, else -6): a third less output traffic, half the backward's index
 * traffic.  row_scale (may be NULL): out *= (row_scale[r] + row_scale_add) = the objectness prior of
 * roi_heads_oicrplus.py:200-221.  A +NaN map value never wins a bin (reference: 'val > maxval').
 * ld_out: row pitch (elements) of out AND argmax, 0 = C*PH*PW.  The fc6 GEMM reads `out` fastest when the pitch is not a
 * multiple of 1 KiB (HBM channel / L2 set spread): the hot path passes C*PH*PW + 64.
 * workspace: NULL, or a device buffer of >= sw_roi_pool_fwd_workspace_bytes(nimg, R, PH, PW) bytes (16-byte aligned; contents need
 * not survive the call).  With it, on bf16 maps of < 65535 pixels (H, W <= 255; PH, PW <= 8; C % 8 == 0) the ROI geometry — bin
 * ranges, size classes, the (image, row band, class) task lists — is computed ONCE per call by a small kernel instead of once per
 * channel slab inside the pooling kernel (large maps: half of that kernel's cycles).  The results are identical either way. */
long sw_roi_pool_fwd_workspace_bytes(int nimg, int R, int PH, int PW);
int sw_roi_pool_fwd(int dtype, int nimg, int H, int W, int C, int PH, int PW, float spatial_scale, const void* feat,
                    const float* rois, int R, const float* row_scale, float row_scale_add, void* out,
                    void* argmax, int argmax_bits, long ld_out, void* workspace, long workspace_bytes, sw_stream_t stream);
/* dfeat [nimg][H][W][C] (dtype, fully overwritten) = scatter-add of dout by argmax, times the same row scale,
 * times (relu_ref > 0) when relu_ref != NULL (relu_ref has feat's layout/dtype).
 * dout_absmax (device scalar >= max|dout|, e.g. from sw_absmax or a GEMM epilogue; may be NULL): selects the fixed-point LDS
 * accumulation (one 64-bit word per pixel-channel in f32 mode, a hi / lo pair of 32-bit words in bf16 mode: >= 25 bits per term;
 * bitwise reproducible, ~3x faster than LDS float atomics); NULL => f32 atomics.
 * A NaN or Inf anywhere in dout (through dout_absmax) or in row_scale + row_scale_add makes the fixed-point path write NaN to
 * every element of dfeat; the f32 atomics carry it to the elements it reaches.
 * ld_in: row pitch (elements) of dout AND argmax, 0 = C*PH*PW.
 * spatial_scale: the forward's scale, or 0.  With it, on maps whose accumulators need several pixel ranges per plane, a
 * workgroup streams only the ROIs whose bin rows, formed as the forward forms them, reach its range (0 streams all ROIs; the
 * forward's scale and 0 yield the same bits). */
int sw_roi_pool_bwd(int dtype, int nimg, int H, int W, int C, int PH, int PW, const void* dout,
                    const void* argmax, int argmax_bits, long ld_in, const float* rois, int R, const float* row_scale,
                    float row_scale_add, const void* relu_ref, const float* dout_absmax, void* dfeat, float spatial_scale,
                    sw_stream_t stream);
/* out[0] = max |x[i]| (f32 device scalar, overwritten). */
int sw_absmax(int dtype, long n, const void* x, float* out, sw_stream_t stream);

/* ---- WSDDN MIL head: scores, image-level BCE, gradient (reference: fast_rcnn_wsddn.py:556-567 forward,
 *      :340-375 loss; autograd backward) -------------------------------------------------------------------
 * logits f32 [V*R][ld]: cls logits at columns [cls_col, cls_col+K), det logits at [det_col, det_col+K);
 * per view v: scores[v][r][k] = softmax_k(cls) * softmax_r(det); loss_view[v] = BCE(clamp(sum_r scores), onehot)/K.
 * If dlogits != NULL (f32): dlogits[(v*R+r)*ld_d + col] = grad_scale[0]/V * d loss_view[v] / d logit, where
 * grad_scale is a DEVICE scalar (the cotangent of the mean-over-views loss) so that no host sync is needed.
 * mean_scores (may be NULL): [R] rows of pitch ld_mean, columns [0,K) = mean over views of scores, summed in view
 * order (roi_heads_oicrplus.py:290-294) — the mining input of refinement round 0.
 * workspace: >= sw_wsddn_workspace_floats(V, R, K) floats (chunk statistics; the softmax over proposals is cut into
 * 256-row chunks that run on separate CUs).  Limits: V <= 8, K <= 128. */
long sw_wsddn_workspace_floats(int V, int R, int K);
int sw_wsddn_mil(int V, int R, int K, const float* logits, long ld, int cls_col, int det_col, const float* gt_onehot,
                 float* scores, float* loss_view, float* dlogits, long ld_d, const float* grad_scale,
                 float* mean_scores, long ld_mean, float* workspace, sw_stream_t stream);

/* General backward of the WSDDN scores (fast_rcnn_wsddn.py:564-567: scores = softmax(C, dim=1) * softmax(D, dim=0), ONE image's R
 * proposals): logits [R][ld] = [C (K) | D (K) | ...], g_scores [R][ld_g] the cotangent of the scores -> dlogits [R][ld_d] columns
 * 0..2K-1 (others untouched): dC = A (gB - sum_k A g B), dD = B (gA - sum_r B g A).  For callers of the stand-alone predictor API
 * that build their own loss on the scores; the training path's loss gradient comes from sw_wsddn_mil.  Sums in double, fixed order:
 * deterministic.  K <= 159 (64-bit row products in LDS); workspace 8-byte aligned. */
long sw_wsddn_scores_bwd_workspace_floats(int R, int K);
int sw_wsddn_scores_bwd(int R, int K, const float* logits, long ld, const float* g_scores, long ld_g, float* dlogits, long ld_d,
                        float* workspace, sw_stream_t stream);
/* ---- mean over V score matrices (reference: roi_heads_oicrplus.py:290-294,390-395) ----------------------- */
int sw_mean_views(int V, long n, const float* in, float* out, sw_stream_t stream);

/* ---- view-mean softmax scores of the refinement heads (reference: predict_probs fast_rcnn_oicr.py:702-716 +
 *      the view average roi_heads_oicrplus.py:390-395) -------------------------------------------------------
 * out[k][r][j] = mean_v softmax_j(logits[(v*R+r)*ld + cls_col0 + k*col_stride + j]), j in [0,K], k in [0,n_rounds).
 * These are round k+1's mining scores; they depend on the logits only, so every round comes from one launch. */
int sw_oicr_mean_probs(int V, int R, int K, int n_rounds, const float* logits, long ld, int cls_col0, int col_stride,
                       float* out, sw_stream_t stream);

/* ---- pseudo-GT mining + proposal labelling, all device side (reference: get_pgt_top_k
 *      roi_heads_oicrplus.py:607-757, get_pgt_mist :560-605 incl. torchvision batched_nms, pairwise_iou
 *      structures/boxes.py:329-361, Matcher matcher.py:63-111, label_and_sample_proposals roi_heads.py:266-375)
 * n_rounds independent problems (one workgroup each, concurrently), laid out back to back:
 * scores [n_rounds][R][ncol] f32; gt_classes [G] int32 sorted unique; boxes [R][4] f32 (shared).
 * Outputs per round: lab_class (class | K background | -1 ignore), lab_weight, lab_index [n_rounds][R]; the kept
 * pseudo-GT list (score-descending): pgt_count [n_rounds], pgt_index/pgt_class/pgt_score [n_rounds][top_k*G].
 * top_k = max(int(R * MIST_P), 1) is computed by the host exactly as the reference does (:659-660).
 * workspace: >= n_rounds * sw_mine_workspace_bytes(R, top_k, G) bytes.  The sort keys live in LDS while R and top_k*G
 * are <= 16384; beyond that (COCO: PRECOMPUTED_PROPOSAL_TOPK_TRAIN 10000 with >= 17 image-level classes,
 * coco_oicr_plus.yaml:67) the workspace carries them.  Limits: R, top_k*G <= 2^22, top_k*G bytes of LDS (<= 144 KiB).
 * The reference's other mining rules (all NULL / 0: the behaviour above, bit for bit, by the same kernel code):
 *  cand_boxes, cand_from  OICRPLUS.BBOX_UPDATE True (roi_heads_oicrplus.py:398-425): class-specific candidate boxes
 *              [n_rounds - cand_from][R][G][4] f32, 16-byte aligned (sw_oicr_update_boxes' output).  A round k >= cand_from
 *              takes the box of the slot (rank, g) from cand_boxes[k - cand_from][row][g] instead of boxes[row]
 *              (index_select + gather, :650-653, :675-678): the NMS runs on those boxes, and the labels' pairwise_iou is
 *              taken between those pseudo boxes and the proposal boxes.  Rounds below cand_from read `boxes`.
 *  seed_rule   0: top-p% + score threshold + NMS (WSL.REFINE_MIST True, get_pgt_mist :560-605).  1: WSL.REFINE_MIST False,
 *              get_pgt_top_k with top_k = 1 (:320-323, :607-757): one seed per image-level class, the pseudo-GT list is
 *              exactly G entries in CLASS order (score ties: lowest proposal index), score_thresh and nms_thresh are not
 *              read and nothing is sorted by score; needs top_k == 1 (else -6).  Two classes that seed one proposal tie in
 *              every IoU, and the first list entry = the lower class id wins the label (matcher.py: first maximum).
 *  lab_box     [n_rounds][R][4] f32, 16-byte aligned, nullable: the matched pseudo box of every proposal, bit for bit the
 *              box its IoU was taken with (label_and_sample_proposals' gt_boxes, roi_heads.py:327-330).
 *  pgt_box     [n_rounds][top_k*G][4] f32, 16-byte aligned, nullable: the boxes of the kept list (first pgt_count rows).
 * In these forms an IoU that is NaN (a pseudo box with a NaN coordinate) counts as 0, as the reference's NaN-propagating
 * min / max / clamp and where(inter > 0, ., 0) make it (structures/boxes.py:329-361). */
long sw_mine_workspace_bytes(int R, int top_k, int G);
int sw_oicr_mine_label(int R, int ncol, int K, int n_rounds, const float* scores, const int32_t* gt_classes, int G,
                       const float* boxes, int top_k, float score_thresh, float nms_thresh, float iou_bg,
                       float iou_fg, int32_t* lab_class, float* lab_weight, int32_t* lab_index, int32_t* pgt_count,
                       int32_t* pgt_index, int32_t* pgt_class, float* pgt_score, void* workspace,
                       const float* cand_boxes, int cand_from, int seed_rule, float* lab_box, float* pgt_box,
                       sw_stream_t stream);

/* ---- box update: the candidate boxes of the next round (reference: OICRPLUS.BBOX_UPDATE roi_heads_oicrplus.py:398-425,
 *      predict_boxes fast_rcnn_oicr.py, Box2BoxTransform.apply_deltas box_regression.py:73-110) ----------------------
 * out[k][r][g][4] = apply_deltas(d, boxes[r]) for refinement head k in [0, n_heads), image-level class gt_classes[g],
 * d = (d_0 -+ d_1 + ... -+ d_{V-1}) / V in float32, left to right, d_v = logits[(v*R+r)*ld + box_col + k*col_stride +
 * 4*gt_classes[g] ..+4]; a view with dx_sign[v] < 0 (a flipped view) enters dx, and dx only, with a minus sign (:407-410).
 * boxes [R][4]: view 0's proposals (the only decoded boxes the reference uses: :419-421 are dropped).  dx_sign: DEVICE
 * int32[V] ({1,-1,1,-1}).  reg_weights4: HOST float[4]; dw, dh clamped to scale_clamp; the result is NOT clipped.
 * Only the G image-level classes are decoded (the mining reads nothing else): out is n_heads*R*G*16 bytes, 16-byte
 * aligned, and is sw_oicr_mine_label's cand_boxes with cand_from = 1.  A gt_classes[g] outside [0, K) gives a NaN box. */
int sw_oicr_update_boxes(int V, int R, int K, int G, int n_heads, const float* logits, long ld, int box_col,
                         int col_stride, const float* boxes, const int32_t* gt_classes, const int32_t* dx_sign,
                         const float* reg_weights4, float scale_clamp, float* out, sw_stream_t stream);

/* ---- OICR refinement losses + gradient (reference: OICROutputs.__init__/softmax_cross_entropy_loss/
 *      box_reg_loss fast_rcnn_oicr.py:157-226,258-273,276-352; get_deltas box_regression.py:38-71; cross-view
 *      targets and the predictions_k2 quirk roi_heads_oicrplus.py:327-381) -----------------------------------
 * n_rounds refinement heads in one launch.  logits f32 [V*R][ld]: round k has its class logits at
 * [cls_col + k*col_stride, +K+1) and its box deltas at [box_col + k*col_stride, +4K).  boxes [V][R][4].
 * lab_class / lab_weight / lab_index [n_rounds][R] (sw_oicr_mine_label's outputs).
 * pred_view[v] = which view's predictions are paired with view v's targets ({0,1,2,2}).
 * loss_view [n_rounds][2][V] (cls then box, already divided by R).
 * dlogits (f32, may be NULL): the columns of every round are overwritten with
 * (grad_scale[2k]*dcls + grad_scale[2k+1]*dbox)/V; grad_scale is a DEVICE float[2*n_rounds]; reg_weights4 is a HOST
 * float[4] (BBOX_REG_WEIGHTS, a configuration constant passed by value into the launch); workspace:
 * n_rounds*2*V*R floats (per-row loss terms, summed in fixed order => deterministic losses).
 * tgt_box0 (nullable; NULL: as above, bit for bit): [n_rounds][R][4] f32, the regression target box of view 0
 * (sw_oicr_mine_label's lab_box).  With OICRPLUS.BBOX_UPDATE the matched pseudo box is a refined box and no row of the
 * proposal list: view 0 regresses towards it (roi_heads.py:327-330), the other views keep boxes[v][lab_index]
 * (roi_heads_oicrplus.py:327-371). */
int sw_oicr_refine_loss(int V, int R, int K, int n_rounds, const float* logits, long ld, int cls_col, int box_col,
                        int col_stride, const float* boxes, const int32_t* lab_class, const float* lab_weight,
                        const int32_t* lab_index, const int32_t* pred_view, const float* reg_weights4,
                        float* loss_view, float* dlogits, long ld_d, const float* grad_scale, float* workspace,
                        const float* tgt_box0, sw_stream_t stream);

/* Stage-3 (Unbiased-Teacher) focal classification loss of the ROI heads, replaces FastRCNNFocalLoss.comput_focal_loss +
 * FocalLoss.forward (unbias/ubteacher/modeling/roi_heads/fast_rcnn.py:73-105):
 *   loss[0] = sum_r (1 - p_r)^gamma * CE_r / N,  CE_r = cross_entropy(logits[r], targets[r]),  p_r = exp(-CE_r);
 * dlogits (nullable, N x C, pitch ld_d) receives dloss/dlogits.  workspace: N floats.  Rows are summed in a fixed order. */
int sw_focal_loss(int N, int C, const float* logits, long ld, const int32_t* targets, float gamma, float* loss,
                  float* dlogits, long ld_d, float* workspace, sw_stream_t stream);
/* ---- inference (reference: OICRPlusHeads._forward_box_test roi_heads_oicrplus.py:432-475, predict_probs_K /
 *      predict_boxes_K fast_rcnn_oicr.py:674-735, Box2BoxTransform.apply_deltas box_regression.py:73-110,
 *      fast_rcnn_inference_single_image fast_rcnn_oicr.py:86-148 incl. torchvision batched_nms) ----------------
 * sw_oicr_predict: logits f32 [R][ld] with refine_k blocks (cls_score K+1 | bbox_pred 4K) starting at base_col, one
 * every round_stride columns; boxes [R][4].  all_scores [R][K+1] = mean softmax, all_boxes [R][4K] = decoded mean
 * deltas (dw, dh clamped to scale_clamp), NOT clipped.  reg_weights4: HOST float[4]. */
int sw_oicr_predict(int R, int K, int refine_k, const float* logits, long ld, int base_col, int round_stride,
                    const float* boxes, const float* reg_weights4, float scale_clamp, float* all_scores,
                    float* all_boxes, sw_stream_t stream);
/* sw_detect_postprocess: clip boxes to the image, keep score > score_thresh (background column excluded), per-class
 * greedy NMS (IoU > nms_thresh on boxes offset by class*(max_coord+1), as batched_nms forms them), first topk by
 * score.  Outputs det_count[1], det_boxes [topk][4], det_scores, det_classes, det_rows (proposal index).
 * Limits: R <= 16384, K*topk <= 16384, topk >= 1 (else -6, nothing written); R <= 0: det_count = 0.
 * Order: inside a class by score descending, then proposal index ascending; the final list by score descending, then r*K + c
 * ascending (the position in the reference's nonzero() list).  Scores rank by VALUE: -0.0 and +0.0 are one score, the position
 * decides between them, and a zero score is returned as +0.0; every other score is returned bit for bit.
 * Where this entry differs from the reference on purpose:
 *  - rows with a non-finite box or score are NOT dropped (fast_rcnn_oicr.py:110-114 drops them): the callers pass finite rows;
 *  - NMS runs per class.  batched_nms makes ONE greedy pass over all classes; after the class offset boxes of different classes
 *    have IoU 0 (or NaN), which never exceeds nms_thresh >= 0, so the keep set is the same.  With nms_thresh < 0 it is not: here
 *    every class keeps its best box (plus the boxes whose IoU with every kept one is NaN: two empty boxes), the one-pass form
 *    would let the best box of the image suppress every other class.
 * Only the first det_count rows of the four output arrays are written.
 * workspace_bytes says how large the workspace is.  With >= sw_detect_workspace_bytes(R, K, topk) bytes the per-class NMS of every
 * class that holds >= 256 candidates runs in its mask form — candidates sorted per class, the 64 x 64 IoU tiles of every class
 * computed over all CUs, one wave per class resolving the chunks in order (the RPN's per-level lists of detectron2's
 * find_top_rpn_proposals, proposal_utils.py:20-130: 2000 candidates per level; 20-80 classes of fast_rcnn_inference_single_image).
 * Below that size the per-class form runs: one workgroup per class doing its N^2 / 2 tests alone.  It needs
 * sw_detect_workspace_bytes(0, K, topk) bytes, which is also all that sw_detect_workspace_bytes(R, K, topk) returns when the mask
 * matrices would exceed 96 MiB.  Identical outputs in both forms. */
long sw_detect_workspace_bytes(int R, int K, int topk);
int sw_detect_postprocess(int R, int K, const float* all_scores, const float* all_boxes, int img_h, int img_w,
                          float score_thresh, float nms_thresh, int topk, int32_t* det_count, float* det_boxes,
                          float* det_scores, int32_t* det_classes, int32_t* det_rows, void* workspace,
                          long workspace_bytes, sw_stream_t stream);
/* sw_tta_merge: the merge of Stage-3 test-time augmentation for one image in one launch, without workspace or host read (reference:
 * GeneralizedRCNNWithTTA._get_augmented_boxes / _merge_detections, detectron2/detectron2/modeling/test_time_augmentation.py:218-259,
 * with fast_rcnn_inference_single_image, detectron2/detectron2/modeling/roi_heads/fast_rcnn.py:118-179, at score_thresh 1e-8).
 * Inputs: the V views' PADDED detections boxes [V][T][4] f32 (16-byte aligned), scores [V][T], classes [V][T] i32, DEVICE counts [V]
 * (row (v, s) counts iff s < counts[v]; nothing beyond a count influences the result), DEVICE view_tab [V][6] f32 = {flip (0 / 1), view
 * width, x and y ratio view -> loader image, x and y ratio loader image -> dataset image (1 when the shapes are equal)}, the dataset
 * image's (img_h, img_w).  Per row in float32, one rounding per step: un-flip (x -> width - x, corners re-sorted by min / max), times the
 * first ratios, times the second; rows with a non-finite box or score are dropped; clip to the image; keep score > 1e-8 (empty boxes
 * stay, a class outside [0, K) goes); per-class NMS (IoU > nms_thresh on boxes offset by class * (max_coord + 1), 0 / 0 suppresses
 * nothing).  Order: inside a class score descending then union index (v * T + s) ascending; the output the survivors by score
 * descending then union index ascending, the first topk.  Outputs det_count[1], then det_boxes [topk][4], det_scores, det_classes and
 * det_src (union index); only the first det_count rows are written.  A counts[v] outside [0, T] gives det_count = -1 and writes nothing
 * else.  Limits: V * T <= 2048, 1 <= K <= 1024, topk >= 1 (else -6). */
int sw_tta_merge(int V, int T, int K, const float* boxes, const float* scores, const int32_t* classes, const int32_t* counts,
                 const float* view_tab, int img_h, int img_w, float nms_thresh, int topk, int32_t* det_count, float* det_boxes,
                 float* det_scores, int32_t* det_classes, int32_t* det_src, sw_stream_t stream);

/* ---- small utilities ------------------------------------------------------------------------------------ */
/* dst[c][r] = src[r][c] (rows x cols elements of `dtype`, row pitches in elements, multiples of 16 bytes).  The weight-gradient
 * GEMMs of the box head read dZ^T through it: with A K-contiguous they run the forward-style kernel (1.2-1.3 PFLOP/s) instead of
 * transposing both operands on the fly inside LDS (1.0). */
int sw_transpose_2d(int dtype, int rows, int cols, const void* src, long ld_src, void* dst, long ld_dst, sw_stream_t stream);
/* ---- Stage-3 (Unbiased-Teacher semi-supervised step, unbias/ubteacher/engine/trainer.py:436-604) building blocks ------------
 * sw_ema_multi: teacher[i] = student[i] * (1 - keep_rate) + teacher[i] * keep_rate for n_tensors f32 tensors in as few
 * launches as 48-tensor batches allow (_update_teacher_model :588-604; keep_rate 0 = the copy at the end of burn-in).
 * teacher / student / numel are HOST arrays (of device pointers / element counts). */
int sw_ema_multi(int n_tensors, float* const* teacher, const float* const* student, const long* numel, double keep_rate,
                 sw_stream_t stream);
/* Weighted sum of n <= 32 scalar losses living anywhere on the device (unbias/ubteacher/engine/trainer.py:520-540: every loss of the
 * record times its weight — 0 for the two pseudo box-regression losses, UNSUP_LOSS_WEIGHT for the other pseudo losses, 1 otherwise —
 * then `sum(loss_dict.values())`): out[i] = values[i][0] * weights[i], out[n] = ((out[0] + out[1]) + out[2]) + ... in that order
 * (the f32 additions of Python's sum over the dict).  values / weights: host arrays.  sw_scale_scalars is its backward:
 * out[i] = g[0] * weights[i].  One launch each instead of 2 n (+ n backward) framework launches per iteration. */
int sw_weighted_sum(int n, const float* const* values, const float* weights, float* out, sw_stream_t stream);
int sw_scale_scalars(int n, const float* g, const float* weights, float* out, sw_stream_t stream);

/* sw_threshold_select: pseudo-label thresholding (threshold_bbox :361-400): keeps detection i iff scores[i] > thres (and, when
 * allowed_classes != NULL, classes[i] is one of the n_allowed image-level labels: the "multi_label" filter), compacted in input
 * order.  allowed_classes == NULL: no class filter; allowed_classes != NULL with n_allowed == 0: an empty label set, nothing is kept
 * (no class is in it, trainer.py:381-386); with a filter `classes` must be given.  out_count[1]; out_boxes [n][4], out_classes [n]
 * (optional: the "rpn" branch has none), out_scores [n], out_index [n] (optional: source positions); rows from out_count[0] on are
 * not written.  One workgroup; n is a few hundred teacher detections per image. */
int sw_threshold_select(int n, const float* scores, const int32_t* classes, const float* boxes, float thres,
                        const int32_t* allowed_classes, int n_allowed, int32_t* out_count, float* out_boxes,
                        int32_t* out_classes, float* out_scores, int32_t* out_index, sw_stream_t stream);
/* sw_stage_weights_multi: the compute-dtype copies of EVERY weight of a detector in one launch (replaces, per layer and per
 * forward call, the reference's implicit `conv.weight` reads + FrozenBatchNorm2d.forward's scale / bias arithmetic,
 * detectron2/layers/batch_norm.py:52-60, wrappers.py Conv2d.forward).  `descs_dev` is a DEVICE array of n entries ordered by
 * block_start (entry i owns workgroups [block_start_i, block_start_i + sw_stage_blocks(kind, rows, cols))); total_blocks = their sum.
 * kind 0: (rows, cols) f32 -> dst rows of pitch cols; 1: OIHW 3x3 -> [co][tap][ci]; 2: OIHW 3x3 -> [ci][8 - tap][co] (data
 * gradient); 3: f32 copy.  rows = Cout, cols = Cin.  bn_* (all four or none): the folded weight w * scale[co] is staged and
 * scale / shift (optional outputs, rows floats) are written: scale = bn_weight * rsqrt(bn_var + eps), shift = bn_bias - bn_mean * scale. */
typedef struct sw_stage_desc {
  const float* w;
  const float* bn_weight; const float* bn_bias; const float* bn_mean; const float* bn_var;
  float* scale; float* shift;
  void* dst;
  int32_t kind, rows, cols, block_start;
} sw_stage_desc;
int sw_stage_blocks(int kind, int rows, int cols);
int sw_stage_weights_multi(int dtype, int n, const sw_stage_desc* descs_dev, int total_blocks, float eps, sw_stream_t stream);
/* *counter += increment, in stream order (one thread): the dropout stream position of sw_epilogue.drop_offset_dev */
int sw_counter_add(uint64_t* counter, uint64_t increment, sw_stream_t stream);
/* n device-to-device byte copies in one launch (input staging into a captured step's static buffers; replaces n
 * `Tensor.copy_` calls of DatasetMapperMultiInput-shaped batches, dataset_mapper.py:272-439).  Regions must not overlap. */
typedef struct sw_copy_desc { const void* src; void* dst; long bytes; } sw_copy_desc;
int sw_copy_multi(int n, const sw_copy_desc* copies, sw_stream_t stream);
/* out[n] = (accumulate ? out[n] : 0) + sum_m X[m][ld..] (column sums; the bias gradients of the reference's conv / Linear
 * backward; accumulate != 0: a bias gradient that exists already inside one backward pass, see sw_conv3x3_wgrad).  out f32.  With
 * `workspace` (sw_colsum_workspace_floats floats) the sum is deterministic: partial rows per row chunk, then an ordered fold.
 * workspace NULL (or N / ld not a multiple of 16 bytes): zero fill (unless accumulating) + one f32 atomic per column and row chunk. */
long sw_colsum_workspace_floats(int dtype, int M, int N);
int sw_colsum(int dtype, int M, int N, const void* X, long ld, float* out, float* workspace, int accumulate, sw_stream_t stream);
/* the two halves of the workspace form for n matrices in ONE launch each (every bias gradient of a backward pass: conv layers x view
 * batches); `parts` is a HOST array; problem i writes sw_colsum_workspace_floats(dtype, M, N) / N partial rows at its workspace */
typedef struct { int M, N; const void* X; long ld; float* workspace; } sw_colsum_part_desc;
int sw_colsum_partial_multi(int dtype, int n, const sw_colsum_part_desc* parts, sw_stream_t stream);
/* n folds in ONE launch, each adding n_partial_rows consecutive rows (of one or several matrices) in fixed order; `folds` is a HOST array */
typedef struct { int N, n_partial_rows; const float* workspace; float* out; } sw_colsum_fold_desc;
int sw_colsum_fold_multi(int n, const sw_colsum_fold_desc* folds, sw_stream_t stream);
/* rows x cols copy/convert f32 -> dtype with independent leading dimensions (weight staging). */
int sw_convert_2d(int dtype, int rows, int cols, const float* src, long ld_src, void* dst, long ld_dst,
                  sw_stream_t stream);
/* Reference-precision GEMMs on the bf16 MFMA (the fp32 mode's fc layers, W/roi_heads/box_head.py:82-91 and their autograd backward):
 * an f32 matrix as three bf16 pieces a = a1 + a2 + a3 (a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)), laid out as one
 * operand of a six-product GEMM  a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1)  = ONE bf16 sw_gemm over K' = 6 K with f32
 * accumulation (the dropped products are below 2^-24 |a||b|).  side 0: blocks [a1|a1|a2|a1|a2|a3]; side 1: [b1|b2|b1|b3|b2|b1].
 * along_rows 0: the K blocks follow each other along the columns (dst: rows x 6 cols); 1: along the rows (dst: 6 rows x cols). */
int sw_split_bf16x3(int rows, int cols, const float* src, long ld_src, void* dst, long ld_dst, int side, int along_rows,
                    sw_stream_t stream);
/* dst[c][r] = src[r][c] converted to dtype (rows x cols f32 source; dst has cols rows of pitch ld_dst): the eager form of
 * sw_sgd_multi's stage_kind 3 transposed copy (first step / after a checkpoint load). */
int sw_convert_2d_t(int dtype, int rows, int cols, const float* src, long ld_src, void* dst, long ld_dst,
                    sw_stream_t stream);
/* f32 NCHW -> dtype NHWC, channels zero padded to cpad (generic backbone entry, vgg.py:216-223 takes NCHW). */
int sw_nchw_to_nhwc(int dtype, int N, int C, int H, int W, int cpad, const float* in_nchw, void* out_nhwc,
                    sw_stream_t stream);
/* ReLU backward: out = ref > 0 ? grad : 0  (F.relu_ backward, vgg.py:105-116).  out == grad is the in-place form; a separate out
 * leaves grad alone (the backbone's entry gradient belongs to autograd). */
int sw_relu_bwd(int dtype, long n, const void* ref, const void* grad, void* out, sw_stream_t stream);
/* out[m][n] = in[m][n] * colscale[n] (f32 -> dtype): applies each loss term's cotangent to its logit columns. */
int sw_scale_cols(int dtype, int M, int N, const float* in, long ld_in, const float* colscale, void* out,
                  long ld_out, sw_stream_t stream);
int sw_fill_zero(void* p, long bytes, sw_stream_t stream);
/* keep[i] = hash(seed, offset+i) >= p   (Bernoulli keep mask for F.dropout, box_head.py:90) */
int sw_dropout_mask(uint8_t* keep, long n, uint64_t seed, uint64_t offset, float p, sw_stream_t stream);
/* SGD with momentum + weight decay, torch.optim.SGD semantics (reference: solver/build.py:191-215,
 * train_net_multi.py:157-164):  g += wd*p;  buf = first ? g : mom*buf + g;  p -= lr*buf. */
int sw_sgd_momentum_step(float* param, const float* grad, float* momentum_buf, long n, float lr, float momentum,
                         float weight_decay, int first_step, float grad_scale, sw_stream_t stream);
/* The whole optimizer step in one launch per <= SW_SGD_MAX_TENSORS parameter tensors, with the compute-dtype kernel-layout
 * copies the next forward needs ("weight staging") written from the freshly updated values in the same pass — the f32
 * master is read once instead of once by the optimizer and once more by every staging kernel.
 * tensors: HOST array (copied into the launch).  stage_kind 0: none.  1: the parameter is a (n/d0) x d0 matrix, stage0
 * receives it in stage_dtype with row pitch ld0 (fc / predictor weights).  2: the parameter is an OIHW 3x3 conv weight
 * (Cout=d0, Cin=d1): stage0 (may be NULL) = forward layout [co][tap][d2=cin_pad] and stage1 (may be NULL) = data-gradient
 * layout [ci][8-tap][co], exactly what sw_conv_weight_prep modes 0 / 1 produce.  3: as 1, plus stage1 = the TRANSPOSED
 * matrix (d0 rows of pitch ld1) — fc6's weight is read K-contiguous by the forward AND by the data-gradient GEMM this
 * way (a K-strided operand of 49 KiB pitch costs that GEMM 25 %); n/d0 and d0 must be multiples of 64. */
#define SW_SGD_MAX_TENSORS 24
typedef struct sw_sgd_tensor_s {
  float* param;
  const float* grad;
  float* momentum_buf;
  long n;
  float lr, weight_decay;
  int first_step;
  int stage_kind, stage_dtype;
  void* stage0;
  void* stage1;
  int d0, d1, d2;
  long ld0, ld1;
  const float* hyper_dev;   /* optional DEVICE pointer to {lr, weight_decay}: read by the kernel instead of the two fields above, so
                             * that a captured hipGraph of the step survives learning-rate schedule changes */
} sw_sgd_tensor;
int sw_sgd_multi(int n_tensors, const sw_sgd_tensor* tensors, float momentum, float grad_scale, sw_stream_t stream);
/* 1 if sw_gemm(dtype, a_kstrided, b_kstrided, M, N, K, ...) accepts sw_epilogue.sgd_fused for this shape, else 0 */
int sw_gemm_sgd_fused_supported(int dtype, int a_kstrided, int b_kstrided, int M, int N, int K);
/* out[i] = mean over the n_images images of (sum_v loss_view[b][i][v] / V)   (loss assembly, roi_heads_oicrplus.py:283-288,
 * 384-388; the reference runs one image per GPU, n_images > 1 is the mean DDP would form over as many ranks);
 * total (optional, 2 floats): [0] = sum_i out[i] in index order (train_net_multi.py:129 sum(loss_dict.values())),
 * [1] = 1.0 if that sum is finite else 0.0 (train_loop.py:253-259 _detect_anomaly without a host round trip). */
int sw_loss_finalize(int n_losses, int V, int n_images, const float* loss_view, float* out, float* total,
                     sw_stream_t stream);
/* sw_scale_cols with the column scale formed from the cotangents: ((g_losses ? g_losses[col_to_loss[n]] : 0) +
 * (g_total ? g_total[0] : 0)) * mul for n < n_valid, 0 for the padding columns (never read from `in`). */
int sw_scale_cols_loss(int dtype, int M, int N, int n_valid, const float* in, long ld_in, const float* g_losses,
                       const float* g_total, const int32_t* col_to_loss, float mul, void* out, long ld_out,
                       sw_stream_t stream);
/* One pass of Pillow's 8-bit separable resize over a planar (C, H, W) u8 image — the arithmetic of the reference's
 * ResizeTransform.apply_image (PIL Image.resize(..., BILINEAR), used by DatasetMapperMultiInput dataset_mapper.py:303-352 and
 * DatasetMapperTTAAVG test_time_augmentation_avg.py:199-310): out = clip8((2^21 + sum_t in[first + t] * kk[o][t]) >> 22) along
 * x (horizontal != 0: out (C, H, out_size)) or y (out (C, out_size, W)).  bounds int32 [out_size][2] = (first input index, tap
 * count), kk int32 [out_size][ksize] = 22-bit fixed-point weights, both DEVICE arrays computed by the caller as Pillow's
 * precompute_coeffs does.  in_ld / in_plane: row and plane strides of `in` in bytes (a crop window of a larger image — the mapper's
 * CropTransform, dataset_mapper.py:278-285 — is `in` offset to its first pixel with the parent's strides).  out_flip (optional): the
 * same rows mirrored in x.  Bit exact with Pillow (tests/golden/resize_*.npz). */
int sw_resize_pass_u8(int C, int H, int W, long in_ld, long in_plane, int out_size, int horizontal, const uint8_t* in,
                      const int32_t* bounds, const int32_t* kk, int ksize, uint8_t* out, uint8_t* out_flip, sw_stream_t stream);
/* RandomBrightness + RandomSaturation of the 4-view training mapper (uwsod/detectron2/data/transforms/augmentation_impl.py:403-455
 * through fvcore's BlendTransform on a uint8 image): mode bit 0 = brightness `u8(clip(f32(w_bright) * px))`, bit 1 = saturation
 * `u8(clip(src_w_sat * grey + f64(f32(w_sat) * px)))` with grey = px0 * 0.299 + px1 * 0.587 + px2 * 0.114 in double on the
 * brightened pixels, src_w_sat = 1 - w (host double).  in / out planar u8 [3][H][W]; out_flip (optional): rows mirrored in x. */
int sw_color_jitter_u8(int H, int W, int mode, const uint8_t* in, float w_bright, double src_w_sat, float w_sat, uint8_t* out,
                       uint8_t* out_flip, sw_stream_t stream);
/* The four views' (R,4) proposal boxes and (R,) objectness logits of one image (box_ptrs4 / obj_ptrs4: HOST arrays of 4
 * device pointers) -> boxes [4][R][4], obj [4][R], rois [2][2R][5] = (batch index 0 | 1, box) per scale
 * (poolers.py:81-108 convert_boxes_to_pooler_format for the view / flipped-view pair of a scale). */
int sw_pack_views(int R, const float* const* box_ptrs4, const float* const* obj_ptrs4, float* boxes, float* obj,
                  float* rois, sw_stream_t stream);

/* ==== Stage-3 detector: the ResNet-50-FPN Faster R-CNN of the Unbiased-Teacher step =====================
 * Reference: unbias/ubteacher/modeling/ over the second tree's detectron2/detectron2/modeling/ (v0.4).  Dense layers
 * reuse sw_gemm (1x1 convolutions on NHWC pixels, fc) and sw_conv3x3_igemm / _wgrad; the entry points below are what that
 * model needs on top (csrc/detector.hip).  All activations NHWC. */
/* img u8 [3][h][w] -> out [H][W][4] = (img - mean) / std inside the image, 0 in the padding (ImageList.from_tensors pads at the
 * bottom / right to the size divisibility) and in channel 3 (meta_arch/rcnn.py:220-228, structures/image_list.py:60-124). */
int sw_preprocess_pad(int dtype, int h, int w, int H, int W, const uint8_t* img_chw, const float* mean3, const float* std3,
                      void* out_nhwc4, sw_stream_t stream);
/* BasicStem.conv1 (backbone/resnet.py:334-359): 7x7, stride 2, padding 3, 3 -> 64 channels, then y * scale[c] + bias[c] (the
 * FrozenBatchNorm2d fold, layers/batch_norm.py:52-58) and ReLU.  in [N][H][W][4], w f32 OIHW [64][3][7][7], out [N][OH][OW][64]
 * with OH = (H - 1) / 2 + 1.  Forward only: the stem is frozen (FREEZE_AT 2). */
int sw_stem_conv7x7(int dtype, int N, int H, int W, const void* in_nhwc4, const float* w_oihw, const float* scale,
                    const float* bias, void* out_nhwc64, sw_stream_t stream);
/* F.max_pool2d(kernel 3, stride 2, padding 1) (resnet.py:358): out [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C] */
int sw_maxpool3x3s2(int dtype, int N, int H, int W, int C, const void* in, void* out, sw_stream_t stream);
/* out[n][y][x][:] = in[n][2y][2x][:], out [N][(H + 1) / 2][(W + 1) / 2][C]: the pixels a 1x1 stride-2 convolution reads (bottleneck
 * conv1 / shortcut with STRIDE_IN_1X1, resnet.py:146-166) and FPN's p6 = max_pool2d(p5, kernel 1, stride 2) (fpn.py:188-189);
 * sw_scatter2x is its backward: out [N][H][W][C] = g at the even pixels, 0 elsewhere (fully written). */
int sw_subsample2x(int dtype, int N, int H, int W, int C, const void* in, void* out, sw_stream_t stream);
int sw_scatter2x(int dtype, int N, int H, int W, int C, const void* g, void* out, sw_stream_t stream);
/* A 3x3 convolution (padding 1, stride 1 or 2) as sw_gemm over an explicit column matrix (csrc/conv_col.hip): the stride-2 conv2 of a
 * torchvision-style bottleneck (detectron2/modeling/backbone/resnet.py:146-166, the `stride_in_1x1 = False` branch: conv1 keeps the
 * resolution, the 3x3 conv2 carries the stride) and the 3x3 convolutions of FastRCNNConvFCHead on the (R, 7, 7, C) ROI maps
 * (detectron2/modeling/roi_heads/box_head.py:25-92, the conv part).  in [nimg][H][W][C]; Ho = (H - 1) / stride + 1, Wo likewise;
 *   col[(n * Ho + oy) * Wo + ox][(3 * ky + kx) * C + c] = in[n][stride * oy + ky - 1][stride * ox + kx - 1][c], 0 outside the map
 * with row pitch ldcol: the [tap][ci] order of the staged [co][tap][ci] weight (sw_stage_weights_multi kind 1), which is therefore
 * the (Cout, 9 C) B operand of sw_gemm as it stands.  All 9 C columns of every row are written, columns beyond are not touched;
 * values are copied as bits.  sw_col2im3x3 is the adjoint in gather form: dx[n][iy][ix][c] = the sum, in ascending tap order in f32,
 * of the cells of dcol that sw_im2col3x3 fills from that element (at most 9, stride 2: at most 4), set to 0 where relu_ref
 * [nimg][H][W][C] (same dtype; may be NULL) is not > 0 (sw_relu_bwd's rule), rounded once; every element of dx is written, no
 * atomics (two runs are bit-identical).  Contract: C % 8 == 0, ldcol >= 9 C, ldcol % 8 == 0 (else -5), stride 1 or 2 (else -3),
 * 16-byte aligned pointers (else -4), fewer than 2^31 elements in col (else -6). */
int sw_im2col3x3(int dtype, int nimg, int H, int W, int C, int stride, const void* in, void* col, long ldcol, sw_stream_t stream);
int sw_col2im3x3(int dtype, int nimg, int H, int W, int C, int stride, const void* dcol, long ldcol, const void* relu_ref, void* dx,
                 sw_stream_t stream);
/* out = a + b, with ReLU when relu != 0 (the residual join of a bottleneck block, resnet.py:209-211) */
int sw_add_relu(int dtype, long n, const void* a, const void* b, void* out, int relu, sw_stream_t stream);
/* FPN top-down pathway (fpn.py:142-144): out [N][2h][2w][C] = lateral + nearest-neighbour 2x upsampling of top [N][h][w][C];
 * sw_downsample2x_sum is the upsampling's backward: out [N][h][w][C] = sum over each 2x2 block of g [N][2h][2w][C]. */
int sw_upsample2x_add(int dtype, int N, int h, int w, int C, const void* lateral, const void* top, void* out, sw_stream_t stream);
int sw_downsample2x_sum(int dtype, int N, int h, int w, int C, const void* g, void* out, sw_stream_t stream);
/* ROIAlign, aligned = True (poolers.py:204-213 "ROIAlignV2" -> layers/roi_align.py:7-74 -> torchvision.ops.roi_align; the
 * arithmetic as stated in-tree at uwsod/detectron2/layers/csrc/ROIAlign/ROIAlign_cpu.cpp:20-400).  feat [N][H][W][C] of ONE
 * FPN level; rois [R][5] (batch, x1, y1, x2, y2); sel [n_sel] int32 = the rows of `rois` / `out` assigned to this level
 * (poolers.py:232-250 loops over the levels); out [R][C][PH][PW] with row pitch ld_out (rows not in `sel` are not touched).
 * n_sel_dev (may be NULL): DEVICE int holding the real length of `sel` (sw_roi_assign_levels' sel_cnt); n_sel is then its host bound.
 * Backward: dfeat_f32 [N][H][W][C] float32, zero-filled by the caller, accumulated with f32 atomics. */
int sw_roi_align_fwd(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio, const void* feat,
                     const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev, void* out, long ld_out,
                     sw_stream_t stream);
int sw_roi_align_bwd(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio, const void* gout,
                     long ld, const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev, float* dfeat_f32,
                     sw_stream_t stream);
/* The deterministic backward of ROIAlign (the reference's CPU path, ROIAlign_cpu.cpp:286-400, is a sequential loop: reproducible; f32
 * atomics are not): the same contributions as sw_roi_align_bwd accumulated as 64-bit fixed-point integers, llrint(v * 2^(40 - e)) with
 * max|gout| = f * 2^e, f in [0.5, 1) — integer addition commutes, two runs give the same bits.  gout_absmax: DEVICE float holding
 * max|gout| over the whole gradient (sw_absmax); acc_i64 [N][H][W][C] int64, zero-filled by the caller.  sw_fx_to_float:
 * out[i] = acc[i] * 2^(e - 40) (f32 / bf16; every element NaN when absmax is NaN / Inf). */
int sw_roi_align_bwd_fx(int dtype, int H, int W, int C, int PH, int PW, float spatial_scale, int sampling_ratio, const void* gout,
                        long ld, const float* rois, const int32_t* sel, int n_sel, const int32_t* n_sel_dev, const float* gout_absmax,
                        long long* acc_i64, sw_stream_t stream);
int sw_fx_to_float(int out_dtype, long n, const long long* acc_i64, const float* absmax, void* out, sw_stream_t stream);
/* ---- Stage-3 detector, index side (csrc/proposals.hip): the reference's torch sort / nonzero / randperm logic as device code.
 * RPN proposal selection (detectron2/detectron2/modeling/proposal_generator/proposal_utils.py:22-130 find_top_rpn_proposals, up to its
 * batched_nms): for every image and level the pre_topk highest objectness logits (= sort(descending, stable)[:k]: ties -> ascending
 * anchor index), their boxes decoded (box_regression.py:88-116, weights4, scale_clamp), and the candidate rows written in the form
 * sw_detect_postprocess takes with "class" = level: image `i` owns rows [i * L * pre_topk, (i + 1) * L * pre_topk), level l the
 * pre_topk rows from l * pre_topk, in descending score order; cand_scores [rows][L + 1] = -inf except column l (-inf there too for
 * unused rows and for boxes that are empty after clipping to img_hw_dev[i] = (h, w): proposal_utils.py:96-106), cand_boxes
 * [rows][4 L] the box repeated.  finite_dev[i] = 0 if a selected box / logit is not finite (:86-94), else nonzero.
 * logits / deltas / anchors: HOST arrays of L device pointers, level l: logits [N][n_l], deltas [N][n_l][4], anchors [n_l][4];
 * img_stride != 0: image i's row of level l starts img_stride anchors after image i-1's (the levels are column ranges of ONE
 * [N][sum n_l] array, sw_rpn_unpack's output), 0: every level is dense on its own.
 * sel_idx: int32 [N * L][pre_topk] scratch.  pre_topk <= 16384, N * L <= 40. */
long sw_rpn_select_workspace_bytes(int N, int L, const int* n_per_level);
int sw_rpn_select_pack(int N, int L, const float* const* logits, const float* const* deltas, const float* const* anchors,
                       const int* n_per_level, long img_stride, int pre_topk, const float* weights4, float scale_clamp,
                       const int* img_hw_dev, float* cand_scores, float* cand_boxes, int* finite_dev, int* sel_idx, void* workspace,
                       long workspace_bytes, sw_stream_t stream);
/* RPN anchor labels (detectron2/.../proposal_generator/rpn.py:305-360 label_and_sample_anchors): IoU of every anchor [A][4] with the
 * image's ground-truth boxes (gt_boxes: the images' boxes back to back, gt_count_per_image HOST array), Matcher thresholds
 * [thr_lo, thr_hi] with labels [0, -1, 1] and low-quality matches (matcher.py:60-126), then subsample_labels (sampling.py:8-54):
 * up to max_pos = int(batch_size * positive_fraction) positives and batch_size - that many negatives per image, drawn as the
 * candidates with the smallest random keys  key(position in the ascending-index candidate list) = splitmix64(seed + position) >> 40
 * (= argsort(keys, stable)[:num], the fixtures' closed-form stand-in for torch.randperm); seeds: HOST u64 [2 N] = (positives,
 * negatives) per image.  labels int8 [N][A] in {-1, 0, 1}; matched f32 [N][A][4] = the box of the arg-max-IoU gt (0 without gt). */
long sw_rpn_label_workspace_bytes(int N, long A, int total_gt);
int sw_rpn_label_anchors(int N, long A, const float* anchors, const float* gt_boxes, const int* gt_count_per_image, float thr_lo,
                         float thr_hi, int batch_size, int max_pos, const uint64_t* seeds, int8_t* labels, float* matched,
                         void* workspace, long workspace_bytes, sw_stream_t stream);
/* ROI-head label + sample (unbias/ubteacher/modeling/roi_heads/roi_heads.py:324-375 label_and_sample_proposals): image i's
 * proposals are the first p_cnt_dev[i] rows (a DEVICE count: it comes from the RPN's NMS) of proposals [n_img][p_stride][4] (+ its
 * ground-truth boxes appended when append_gt); IoU >= iou_thresh -> foreground with the matched box's class, else background
 * `num_classes`; up to max_pos foreground and batch_size - that many background rows by the random-key rule of sw_rpn_label_anchors
 * (seeds: HOST u64 [2 n_img]), foreground list first, each list in key order.  gt_boxes / gt_classes: the images' ground truth back to
 * back, g_off / g_cnt HOST int arrays.  p_stride + g_cnt[i] <= 4096, n_img <= 8.  Outputs, image i at rows [i * out_stride, ...):
 * out_count [n_img], out_index (row in the image's candidate list), out_classes, out_boxes [..][4], out_gt_boxes [..][4]. */
int sw_roi_label_sample(int n_img, const int* p_cnt_dev, int p_stride, const float* proposals, const int* g_off, const int* g_cnt,
                        const float* gt_boxes, const int32_t* gt_classes, int append_gt, float iou_thresh, int num_classes,
                        int batch_size, int max_pos, const uint64_t* seeds, int out_stride, int32_t* out_count, int32_t* out_index,
                        int32_t* out_classes, float* out_boxes, float* out_gt_boxes, sw_stream_t stream);
/* The RPN head's output in anchor order.  y [rows][ld] f32 is ONE GEMM over the pixels of all levels (row = level offset + image *
 * hw_per_level[l] + pixel; columns [objectness a | delta 4 a + b], A anchors per location); logits [N][At], deltas [N][At][4] with
 * At = A * sum hw: level-major, location-major, anchor-minor — the order of rpn.py:230-260 / anchor_generator.py.  _bwd: dy from the
 * two gradients (either may be NULL), each times its DEVICE scalar g_*_dev (NULL = 1: the losses' cotangents), every column written
 * (padding 0). */
int sw_rpn_unpack(int N, int L, int A, const int* hw_per_level, const float* y, long ld, float* logits, float* deltas, sw_stream_t stream);
int sw_rpn_unpack_bwd(int N, int L, int A, const int* hw_per_level, const float* dlogits, const float* ddeltas,
                      const float* g_logits_dev, const float* g_deltas_dev, float* dy, long ld, sw_stream_t stream);
/* FPN level of every ROI (poolers.py:17-50,196-250): image i contributes row_cnt[i] boxes starting at boxes + box_off_floats[i]
 * (HOST arrays); rois [R][5] = (image, box) dense, level_of [R] in 0..3 (= level 2..5), sel [4][R] the rows of each level in ascending
 * order, sel_cnt [4] their counts (DEVICE: sw_roi_align_* read them).  R <= 8192. */
int sw_roi_assign_levels(int n_img, const int* row_cnt, const long* box_off_floats, const float* boxes, float* rois, int32_t* level_of,
                         int32_t* sel, int32_t* sel_cnt, sw_stream_t stream);
/* out[m][n] = in[m][n] * (n < split ? g0_dev[0] : g1_dev[0]) for n < N, 0 for the padding columns N <= n < ld (in and out share the row
 * pitch ld): the cotangents of the ROI heads' two losses (fast_rcnn.py:73-105) applied to the unit gradient of the packed logits. */
int sw_scale_col_blocks(long M, int N, int split, const float* in, long ld, const float* g0_dev, const float* g1_dev, float* out,
                        sw_stream_t stream);
/* RPN losses (proposal_generator/rpn.py:362-420, box_regression.py:229-260) over n = N * A anchors: losses2[0] = sum over
 * label >= 0 of BCE-with-logits(logit, label) * inv_norm, losses2[1] = sum over label == 1 of |delta - get_deltas(anchor, gt)|_1
 * * inv_norm (smooth-L1 with beta 0), and their unit gradients dlogits [n], ddeltas [n][4] (either may be NULL).  anchors
 * [n_anchors][4] repeat over the images (row i uses anchor i % n_anchors), matched_gt_boxes [n][4], labels int8 in {-1, 0, 1}.
 * Ordered two-stage reduction: deterministic.  workspace: sw_rpn_loss_workspace_floats() floats. */
long sw_rpn_loss_workspace_floats(void);
int sw_rpn_loss(long n, long n_anchors, const float* logits, const float* deltas, const int8_t* labels, const float* anchors,
                const float* matched_gt_boxes, const float* weights4, float inv_norm, float* losses2, float* dlogits,
                float* ddeltas, float* workspace, sw_stream_t stream);
/* Per-image detector losses for the Stage-3 split (unbias/split_single.py:66-75: one training forward per image, the four losses
 * summed), for n_img images scored in one batch, each normalised as if it were alone: out [n_img][5] f32 = loss_cls,
 * loss_box_reg, loss_rpn_cls, loss_rpn_loc and their sum, added left to right (split_single.py:74).
 *   RPN (proposal_generator/rpn.py:395-425, box_regression.py:229-268): rpn_logits [n_img * n_anchors], rpn_deltas / rpn_matched
 *   [n_img * n_anchors][4], rpn_labels int8 in {-1, 0, 1}, anchors [n_anchors][4] shared by the images.  loss_rpn_cls = BCE sum /
 *   rpn_batch_size; loss_rpn_loc = L1 sum / rpn_batch_size (rpn_loss_type 0, smooth_l1 with beta 0) or the mean over the
 *   4 x (foreground anchors) elements / rpn_batch_size (1, smooth_l1_mean).
 *   ROI (roi_heads/fast_rcnn.py:73-105 + detectron2 fast_rcnn.py:497-564): roi_logits [roi_rows][ld] = [K + 1 class | 4K box],
 *   roi_classes [roi_rows], roi_boxes / roi_gt_boxes [roi_rows][4], image i's rows packed after those of images < i, their
 *   number roi_counts[i] read from device memory, at most max_rows (the sampler's batch_size_per_image; the rows are spread over
 *   ceil(max_rows / 64) workgroups per image).  loss_cls = sum (1 - p)^gamma CE / rows (gamma 0: cross-entropy, mean over the
 *   rows, 0 without rows: layers/wrappers.py:26-33); loss_box_reg = class-specific L1 sum / max(rows, 1) (roi_loss_type 0) or the
 *   mean over the 4 x (foreground rows) elements (1).  An empty foreground set under type 1 gives NaN (torch's empty mean); counts
 *   that overrun roi_rows or exceed max_rows give NaN, a class outside [0, K] a NaN loss_cls.
 * Grid (anchor chunks + 1, n_img), partials folded in chunk order: deterministic.  workspace: sw_det_loss_workspace_floats(). */
long sw_det_loss_workspace_floats(int n_img, long n_anchors, long max_rows);
int sw_det_loss_per_image(int n_img, long n_anchors, const float* rpn_logits, const float* rpn_deltas, const int8_t* rpn_labels,
                          const float* anchors, const float* rpn_matched, const float* rpn_weights4, int rpn_batch_size,
                          int rpn_loss_type, const float* roi_logits, long ld, int K, const int32_t* roi_classes,
                          const float* roi_boxes, const float* roi_gt_boxes, const int32_t* roi_counts, long roi_rows,
                          long max_rows, const float* roi_weights4, float gamma, int roi_loss_type, float* out, float* workspace,
                          sw_stream_t stream);

/* Stage-2 pseudo-ground-truth filtering of one split (tools/pgf.py: class_filter :273-292 and the two loops of pgf :221-271 with
 * contain_cal :209-219; these replace the per-image Python double loop).  Detections are grouped per image in list order (CSR):
 * image i owns rows [det_off[i], det_off[i + 1]) of boxes [N][4] f64 (16-byte aligned; read as [x, y, w, h] as contain_cal does),
 * scores [N] f64 and classes [N] i32 in [0, K).  gt_mask [n_img][(K + 31) / 32] and diff_mask [(K + 31) / 32] are class bitmasks.
 * Stage 3 keeps a detection whose class is in its image's gt_mask; stage 4 keeps the first stage-3 survivor of each class and a
 * later one iff !(score < t_keep); stage 5 drops a stage-4 survivor i when another stage-4 survivor j of its class has
 * contain_cal(box_i, box_j) >= t_con, unless use_diff == 0 and the class is in diff_mask.  keep [N] u8: 1 = kept; workspace [N]
 * u8: used by images of more than SW_PGF_LDS_CAP detections; counts [4] (8-byte aligned, zeroed here): detections before stage 3,
 * after stage 3, after stage 4, after stage 5.  K <= SW_PGF_MAX_CLASSES.  All f64 arithmetic follows contain_cal's operations. */
#define SW_PGF_LDS_CAP 256
#define SW_PGF_MAX_CLASSES 256
int sw_pgf_keep(int n_img, const int64_t* det_off, const double* boxes, const double* scores, const int32_t* classes, int K,
                const uint32_t* gt_mask, const uint32_t* diff_mask, double t_keep, double t_con, int use_diff, uint8_t* keep,
                uint8_t* workspace, long long* counts, sw_stream_t stream);
/* The same filter at every cell of a grid t_keep[nk] x t_con[nc], each cell's kept detections matched against the split's ground
 * truth at iou[nt] and counted per class (replaces one run of the loops of tools/pgf.py pgf :221-271 per cell, and for the matching
 * the detection loop of evaluation/pascal_voc_evaluation.py voc_eval :357-397, whose rule is used free of detection order).
 * Detections, K, gt_mask, diff_mask and use_diff as for sw_pgf_keep (N: the number of rows); t_keep, t_con and iou are HOST
 * arrays of finite values, in any order, repeats allowed.  Ground truth per image (CSR): image i owns rows [gt_off[i],
 * gt_off[i + 1]) of gt_box [G][4] f64 corners (16-byte aligned), gt_cls [G] i32 and gt_ign [G] u8 (VOC difficult / COCO iscrowd),
 * in annotation order.  xywh != 0: a detection row is [x, y, w, h] and its matching box (x, y, x + w, y + h); otherwise the row is
 * a VOC record [x1 + 1, y1 + 1, x2, y2] and is its own matching box (the filter reads it as [x, y, w, h] in both modes, as the
 * reference does).  plus_one != 0: extents are VOC's `+ 1.0`.  Cell (a, b) keeps exactly what sw_pgf_keep keeps at t_keep[a],
 * t_con[b].  A kept detection's candidates are its image's objects of its class; ovmax / jmax are numpy's max / argmax of
 * inters / (area_det + area_gt - inters) in voc_eval's f64 operations.  With ovmax > iou[t] it counts into ign when object jmax is
 * ignored and claims the object otherwise.  Outputs, i64, 8-byte aligned, zeroed here: kept [nk][nc][K]; tp [nt][nk][nc][K],
 * the claimed objects; ign [nt][nk][nc][K]; npos [K], the non-ignored objects.  Integer atomic adds only: the tables do not
 * depend on launch order.  workspace [N][SW_PGF_SWEEP_WS_WORDS] u32: used by images of more than SW_PGF_LDS_CAP detections.
 * Refused before anything is written: -4 a misaligned pointer, -5 a negative count, -6 K, -7 a grid size outside
 * [1, SW_PGF_SWEEP_MAX_*] or a value that is not finite. */
#define SW_PGF_SWEEP_MAX_KEEP 32
#define SW_PGF_SWEEP_MAX_CON 32
#define SW_PGF_SWEEP_MAX_IOU 10
#define SW_PGF_SWEEP_WS_WORDS 12
int sw_pgf_sweep(int n_img, long long N, const int64_t* det_off, const double* boxes, const double* scores, const int32_t* classes,
                 int K, const uint32_t* gt_mask, const uint32_t* diff_mask, int use_diff, int nk, const double* t_keep, int nc,
                 const double* t_con, int nt, const double* iou, const int64_t* gt_off, const double* gt_box, const int32_t* gt_cls,
                 const uint8_t* gt_ign, int xywh, int plus_one, uint32_t* workspace, long long* kept, long long* tp, long long* ign,
                 long long* npos, sw_stream_t stream);

/* VOC AP and CorLoc of one split at the ten IoU thresholds (evaluation/pascal_voc_evaluation.py: the detection loops, cumulative
 * sums, precision / recall and voc_ap of voc_eval :295-408 and voc_ap :263-292, and the loop of voc_eval_corloc :411-505; these
 * replace the 2 x 10 Python walks per class).  Detections of class c are rows [det_off[c], det_off[c + 1]) in rank order
 * (descending score, ties in line order): det_img [N] i32 image index in [0, n_img), det_box [N][4] f64 [xmin, ymin, xmax, ymax]
 * (16-byte aligned).  The ground truth of image i and class c is rows [gt_off[i * K + c], gt_off[i * K + c + 1]) of gt_box [G][4]
 * f64 (16-byte aligned) and gt_diff [G] u8, in annotation order.  npos [K] / npos_im [K] i64: non-difficult objects / images with
 * at least one, counted over the split's lines.  thr [SW_VOC_THRESHOLDS] f64: IoU thresholds (a match needs IoU > thr);
 * t11 [11] f64: the 11-point recall levels.  out [3][K][SW_VOC_THRESHOLDS] f64 (8-byte aligned): area AP, 11-point AP, CorLoc
 * (0 for a class without detections; npos_im == 0 gives NaN, which callers reject).  workspace: sw_voc_eval_workspace_bytes(...)
 * bytes, 256-byte aligned.  K <= SW_VOC_MAX_CLASSES, N <= SW_VOC_MAX_DETS, G * SW_VOC_THRESHOLDS < 2^31.  The f64 arithmetic
 * follows numpy's operations and summation order, so each value is bit-identical to the reference run in stable tie order. */
#define SW_VOC_MAX_CLASSES 256
#define SW_VOC_THRESHOLDS 10
#define SW_VOC_MAX_DETS (1LL << 30)
long long sw_voc_eval_workspace_bytes(int K, int n_img, long long N, long long G);
int sw_voc_eval(int K, int n_img, long long N, long long G, const int64_t* det_off, const int32_t* det_img, const double* det_box,
                const int64_t* gt_off, const double* gt_box, const uint8_t* gt_diff, const int64_t* npos, const int64_t* npos_im,
                const double* thr, const double* t11, double* out, void* workspace, sw_stream_t stream);

/* COCO bbox evaluation of one split (evaluation/fast_eval_api.py COCOeval_opt over layers/csrc/cocoeval/cocoeval.cpp:
 * MatchDetectionsToGroundTruth :61-140 with SortInstancesByIgnore :33-56, Accumulate :223-371; the IoU is pycocotools' maskApi.c
 * bbIou).  A pair is an (image, category) that has detections.  Detections are grouped by pair, the pairs of a category
 * contiguous and in image order, each pair's detections in stable descending score order and at most SW_COCO_MAX_PAIR_DETS of
 * them (the evaluator cuts at 100): pair p owns rows [pair_off[p], pair_off[p + 1]) of det_box [N][4] f64 [x, y, w, h] (16-byte
 * aligned), det_rank [N] u8 (the row's position in its pair) and det_score [N] f64; category c owns rows [cat_off[c],
 * cat_off[c + 1]), and order [N] i32 lists each category's rows stably sorted by descending score (order[cat_off[c] ..] are rows
 * of c).  The pair's ground truth is rows [gt_off[pair_gt[p]], gt_off[pair_gt[p] + 1]) of gt_box [G][4] f64 [x, y, w, h] (16-byte
 * aligned), gt_area [G] f64 (the annotation's own area) and gt_flags [G] u8 (bit 0: iscrowd, which is also its ignore flag; bit 1:
 * annotation id > 0), in annotation order.  area_rng [SW_COCO_AREAS][2], iou_thr [SW_COCO_THRESHOLDS], rec_thr [SW_COCO_RECALLS] f64,
 * max_dets [SW_COCO_MAXDETS] i32 ascending; npig [K][SW_COCO_AREAS] i64: the non-ignored ground truth of a category and area range
 * over all images.  A pair with G <= 64 and D * G <= lds_doubles (<= SW_COCO_LDS_DOUBLES) is matched in LDS; any other pair needs
 * sw_coco_eval_workspace_bytes(D, G, lds_doubles) bytes (0 for a pair that fits) starting at 8 * pair_ws[p] bytes behind the
 * workspace's SW_COCO_WS_HEADER-byte header (pair_ws [P] i64, read only for such pairs); ws_bytes is the size of the whole
 * workspace (256-byte aligned), header included.  A region outside it is not touched and turns every output into NaN; so does a
 * pair of more than SW_COCO_MAX_PAIR_DETS detections or SW_COCO_MAX_PAIR_GT ground truths (within them D * G fits an int).
 * match [N][2] u64: bit a * SW_COCO_THRESHOLDS + t of word 0 / 1 is the detection's matched / ignored flag in area range a at
 * threshold t.  out f64: precision [T][R][K][A][M], scores [T][R][K][A][M], recall [T][K][A][M], one after the other, each value
 * bit-identical to the reference's.  Kept from the reference: "matched" means the ground truth's id is > 0. */
#define SW_COCO_MAX_CLASSES 4096
#define SW_COCO_THRESHOLDS 10
#define SW_COCO_RECALLS 101
#define SW_COCO_AREAS 4
#define SW_COCO_MAXDETS 3
#define SW_COCO_MAX_PAIR_DETS 255
#define SW_COCO_MAX_PAIR_GT ((1 << 23) - 1)
#define SW_COCO_MAX_DETS ((1LL << 31) - 1)
#define SW_COCO_LDS_DOUBLES 1600
#define SW_COCO_WS_HEADER 256
long long sw_coco_eval_workspace_bytes(int D, long long G, int lds_doubles);
int sw_coco_eval(int K, long long N, long long P, const int64_t* pair_off, const int64_t* pair_gt, const int64_t* pair_ws,
                 long long ws_bytes, int lds_doubles, const double* det_box, const int64_t* gt_off, const double* gt_box,
                 const double* gt_area, const uint8_t* gt_flags, const double* area_rng, const double* iou_thr, const double* rec_thr,
                 const int32_t* max_dets, const int64_t* cat_off, const int32_t* order, const uint8_t* det_rank,
                 const double* det_score, const int64_t* npig, unsigned long long* match, double* out, void* workspace,
                 sw_stream_t stream);

/* Proposal recall of one split for every budget at once (replaces the overlap block of uwsod/projects/WSL/tools/proposal_recall.py:
 * recall_mcg :204-225, the same lines in recall_ss :277-297 and recall_eb :356-376, and the ten passes of its budget loop
 * :389-399).  CSR over images: image i owns rows [prop_off[i], prop_off[i + 1]) of prop_box [P][4] f64 [xmin, ymin, xmax, ymax]
 * (16-byte aligned), already in rank order, and rows [gt_off[i], gt_off[i + 1]) of gt_box [G][4] f64 (16-byte aligned).
 * cuts [n_cut] i32: the budgets, strictly ascending, cuts[0] >= 1 (device memory, so not checked here: the caller's
 * contract, which the Python wrapper asserts; cuts out of order read nothing out of bounds but give wrong rows); thr [n_thr] f64: the IoU thresholds.  For ground-truth row g
 * and cut c, over the first min(cuts[c], n_i) proposals of its image: ovmax [G][n_cut] f64 is np.max of the overlaps (a NaN
 * among them gives NaN) and jmax [G][n_cut] i32 np.argmax (the first index of the maximum, or of the first NaN), an index into the
 * image's ranked list; rows of other images are not touched.  cnt_yes [n_cut][n_thr] i64 (8-byte aligned; zeroed here) counts the
 * rows with ovmax >= thr[t]: a NaN never counts.  An image without ground truth contributes nothing; one with ground truth and
 * no proposals (callers reject it, as np.max of an empty array raises) gets NaN and -1.  Each overlap is the reference's f64
 * arithmetic with its inclusive `+ 1.0` widths, so every value is bit-identical to the reference's. */
#define SW_PROPOSAL_RECALL_MAX_CUTS 16
#define SW_PROPOSAL_RECALL_MAX_THRESHOLDS 16
#define SW_PROPOSAL_RECALL_LDS_BOXES 1024 /* proposals staged per pass; more are taken in further passes */
int sw_proposal_recall(int n_img, const int64_t* prop_off, const double* prop_box, const int64_t* gt_off, const double* gt_box,
                       int n_cut, const int32_t* cuts, int n_thr, const double* thr, double* ovmax, int32_t* jmax,
                       long long* cnt_yes, sw_stream_t stream);

/* Box-proposal AR of one split for every (limit, area range) at once (replaces the per-image loop of _evaluate_box_proposals,
 * detectron2/detectron2/evaluation/coco_evaluation.py:482-514, with pairwise_iou of structures/boxes.py:322-368, and the eight
 * passes of _eval_box_proposals :286-290).  CSR over images: image i owns rows [prop_off[i], prop_off[i + 1]) of prop_box
 * [n_prop][4] f32 [x1, y1, x2, y2] (16-byte aligned), already ranked by descending objectness, and rows [gt_off[i],
 * gt_off[i + 1]) of its non-crowd ground truth in file order: gt_box [n_gt][4] f32 (16-byte aligned) and gt_area [n_gt] f32
 * (the annotation's own area).  area_rng [n_area][2] f32, limits [n_lim] i32 (0: no limit) and thr [n_thr] f32 are HOST arrays.
 * Item (l, a, i) is limit l and area range a of image i: its valid boxes are those with area_rng[a][0] <= gt_area <=
 * area_rng[a][1], G' of them, its proposals the first P' = min(limits[l] or all, n_i).  An image without proposals or without
 * ground truth has no items (:479).  Item (l, a, i) owns elements [item_off[(l * n_area + a) * n_img + i], item_off[.. + 1]) of
 * the three outputs (item_off [n_item_off = n_lim * n_area * n_img + 1] i64, device memory, G' elements per item and 0 for an
 * image without items): element r holds what round r of the greedy matching took — the pair that is best under (largest IoU,
 * smallest box index, smallest proposal index) among pairs whose proposal and box are both unused — as overlap [n_out] f32 (its
 * IoU), match_gt [n_out] i32 (the box's index among the item's valid boxes) and match_box [n_out] i32 (the proposal's rank);
 * min(P', G') rounds run, the elements behind them hold 0, -1, -1.  cnt_yes [n_lim][n_area][n_thr] i64 (8-byte aligned; zeroed
 * here) counts the elements with overlap >= thr[t].  Every IoU is the reference's float32 arithmetic in its order, so every value
 * is bit-identical to the reference's, and so are two launches.
 * An item of P' <= SW_BOXAR_LDS_BOXES and G' <= SW_BOXAR_LDS_GT runs in LDS.  Any other needs the workspace (16-byte aligned,
 * sw_box_proposal_ar_workspace_bytes(n_img, ws_boxes, ws_props) bytes for items of up to ws_boxes valid boxes and ws_props
 * proposals; 0 bytes, and NULL is allowed, when every item fits LDS).
 * Returns -1 NULL host array, -4 alignment, -5 negative count, -6 n_area / n_lim / n_thr outside 1..SW_BOXAR_MAX_*, a negative
 * limit or n_item_off of another split, -7 ws_bytes too small; nothing is written then.  status [1] i32 (device; zeroed here) is
 * 0 after a clean launch, else the last SW_BOXAR_* refusal: such an image or item is skipped, never written. */
#define SW_BOXAR_MAX_AREAS 8
#define SW_BOXAR_MAX_LIMITS 8
#define SW_BOXAR_MAX_THRESHOLDS 16
#define SW_BOXAR_LDS_BOXES 1024 /* ranked proposals staged per image */
#define SW_BOXAR_LDS_GT 128     /* valid boxes whose state a wave keeps in LDS */
#define SW_BOXAR_BAD_OFFSETS 1  /* prop_off / gt_off decrease or leave [0, n_prop] / [0, n_gt] */
#define SW_BOXAR_BAD_LAYOUT 2   /* an item's region is not G' long or leaves [0, n_out] */
#define SW_BOXAR_WORKSPACE 3    /* an item needs more than ws_boxes / ws_props (or there is no workspace) */
long long sw_box_proposal_ar_workspace_bytes(int n_img, long long max_boxes, long long max_props);
int sw_box_proposal_ar(int n_img, const int64_t* prop_off, const float* prop_box, long long n_prop, const int64_t* gt_off,
                       const float* gt_box, const float* gt_area, long long n_gt, int n_area, const float* area_rng, int n_lim,
                       const int32_t* limits, int n_thr, const float* thr, const int64_t* item_off, long long n_item_off,
                       long long n_out, float* overlap, int32_t* match_gt, int32_t* match_box, long long* cnt_yes, void* workspace,
                       long long ws_bytes, long long ws_boxes, long long ws_props, int32_t* status, sw_stream_t stream);

/* Stage-3 strong augmentation of a planar u8 [3][H][W] image, every pixel operation bit-identical to Pillow's (replaces
 * build_strong_augmentation, unbias/ubteacher/data/detection_utils.py:9-46, applied by DatasetMapperTwoCropSeparate.__call__,
 * unbias/ubteacher/data/dataset_mapper.py:141-149; the blur is unbias/ubteacher/data/transforms/augmentation_impl.py GaussianBlur):
 *   colour jitter   order[s] = the op of slot s (SW_AUG_*; -1 = empty slot), applied s = 0..3.  brightness / contrast / saturation
 *                   are ImageEnhance blends `u8(clip(d + f * (x - d)))` in float32 with d = 0 / int(mean(L) + 0.5) of the image at
 *                   that point / L of the pixel, f = factor[op]; hue is convert("HSV"), H += hue_shift (0..255, modulo 256),
 *                   convert("RGB") with Pillow's float / double widths;
 *   grayscale       convert("L") replicated to three channels: (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16;
 *   blur            ImageFilter.GaussianBlur: three box passes along x, then three along y, each rounding to u8, with the integer
 *                   weights of sw_gaussian_blur_weights (blur_r < 0: no blur);
 *   erasing         rect[e] = (top, left, h, w), h = 0: none; e = 0..2 in turn, a later rectangle overwrites an earlier one.  Each
 *                   sample is byte(255 * n) truncated toward zero and wrapped modulo 256 (RandomErasing(value="random") between
 *                   ToTensor and ToPILImage), n ~ N(0, 1) from splitmix64 over (seed, key, e * 4 + channel, (y - top) << 32 |
 *                   (x - left)) and Box-Muller: reproducible, independent of launch geometry.  Pixels outside pass through.
 * The image is always read as R, G, B planes, as the reference's Image.fromarray(..., "RGB") does whatever INPUT.FORMAT says. */
#define SW_AUG_BRIGHTNESS 0
#define SW_AUG_CONTRAST 1
#define SW_AUG_SATURATION 2
#define SW_AUG_HUE 3
typedef struct sw_aug_recipe {
  uint64_t seed, key;
  int32_t order[4];
  float factor[4];            /* by op code; [SW_AUG_HUE] is not read (hue_shift is) */
  int32_t hue_shift;
  int32_t grayscale;
  int32_t blur_r;
  uint32_t blur_ww, blur_fw;
  int32_t rect[3][4];
  int32_t pad_;
} sw_aug_recipe;
/* one image of a batch: tmp = 3 * H * W bytes (read only when the recipe blurs), lsum = one u64 (only with contrast); both lie in
 * a workspace of sw_strong_aug_workspace_bytes(H, W) bytes per image */
typedef struct sw_aug_item {
  const uint8_t* in; uint8_t* out; uint8_t* tmp; uint64_t* lsum;
  int32_t H, W;
  sw_aug_recipe recipe;
} sw_aug_item;
#define SW_AUG_STAGE_CONTRAST 1 /* some image's recipe has contrast */
#define SW_AUG_STAGE_BLUR 2     /* some image's recipe blurs */
#define SW_AUG_STAGE_POINT 4    /* some image's recipe does not blur */
/* HOST arithmetic, no GPU work: sigma -> radius r and the 24-bit fixed-point weights of one box pass (Pillow's
 * _gaussian_blur_radius and ImagingLineBoxBlur8's ww, both in float32).  -1: sigma <= 0; -6: 3 * (r + 1) > 9 (sigma >~ 3.4). */
int sw_gaussian_blur_weights(float sigma, int32_t* r, uint32_t* ww, uint32_t* fw);
long sw_strong_aug_workspace_bytes(int H, int W);
/* one image; `recipe` is a HOST pointer; workspace 256-byte aligned; out must not alias in */
int sw_strong_aug_u8(int H, int W, const uint8_t* in, const sw_aug_recipe* recipe, uint8_t* out, void* workspace,
                     sw_stream_t stream);
/* a batch of images of different sizes in one launch sequence: items_dev is a DEVICE array of n entries; max_h / max_w: the
 * largest H and W among them; stages: SW_AUG_STAGE_* bits, which launches the batch needs.  Same bytes as n single calls. */
int sw_strong_aug_multi_u8(int n, const sw_aug_item* items_dev, int max_h, int max_w, int stages, sw_stream_t stream);

/* Baseline JPEG reader, every pixel equal to Pillow's (libjpeg's defaults: the "islow" integer IDCT, "fancy" chroma upsampling,
 * the 16-bit fixed-point YCbCr -> RGB rule).  Replaces the pixel side of detection_utils.read_image
 * (detectron2/data/detection_utils.py:162-185: Image.open, convert("RGB"), the plane reversal for BGR); the EXIF orientation it
 * reports is applied by the caller.  The HOST parses the markers and undoes the Huffman coding (two plain C functions, no GPU
 * call, no globals: callable from any number of threads); dequantisation, IDCT, upsampling, colour and plane order are two
 * kernels over a whole batch of images of mixed sizes and samplings.
 *
 * Covered (sw_jpeg_probe returns 1): 8-bit SOF0 / SOF1, Huffman coding, one interleaved scan, 1 component (sampling 1x1) or 3
 * YCbCr components with luma 1x1, 2x1 or 2x2 and chroma 1x1.  Not covered (returns 0, `info` undefined): every other SOF,
 * 12-bit samples, a scan without all components, 2 or 4 components, any other sampling, height 0 (DNL), an Adobe APP14 marker whose
 * transform is not 1, component ids 'R' 'G' 'B' without JFIF.  Negative: -1 argument, -2 no SOI (not a JPEG), -3 the marker
 * segments end early, -4 malformed segment, -5 a table or the frame is missing, -6 the entropy-coded data ends early, -7 invalid
 * Huffman code or coefficient index, -8 restart marker missing or wrong, -9 `info` does not describe this stream;
 * sw_jpeg_strerror names them.
 * Stricter than libjpeg, which warns and decodes on: entropy data that ends early, or bytes between the last MCU of a restart
 * interval and its RSTn, are errors here. */
typedef struct sw_jpeg_info {
  int32_t width, height;
  int32_t ncomp;                      /* 1 or 3 */
  int32_t restart_interval;           /* in MCUs; 0: none */
  int32_t orientation;                /* EXIF tag 274 of the first APP1 "Exif" segment's IFD0 if in 1..8, else 1 */
  int32_t mcus_x, mcus_y;
  int32_t hsamp[3], vsamp[3], qtable[3];
  int32_t blocks_w[3], blocks_h[3];   /* the component's padded grid in 8 x 8 blocks: mcus_x * hsamp, mcus_y * vsamp */
  int64_t coef_bytes;                 /* 128 * sum(blocks_w * blocks_h) */
} sw_jpeg_info;
int sw_jpeg_probe(const uint8_t* bytes, long n, sw_jpeg_info* info);
/* coef: info->coef_bytes bytes; quantised coefficients, 64 per block in natural (de-zigzagged) order, blocks in raster order over
 * component 0's padded grid, then component 1's, then 2's.  qtables: uint16[4][64] by table index, natural order, an undefined
 * table all 0.  Reads bytes[0 .. n) only.  coef is zeroed first, so on a negative return every block is defined: the blocks decoded
 * before the error hold their coefficients (the block the error fell in holds those decoded so far), all later ones are 0. */
int sw_jpeg_entropy_decode(const uint8_t* bytes, long n, const sw_jpeg_info* info, int16_t* coef, uint16_t* qtables);
const char* sw_jpeg_strerror(int code);
/* one image of a batch, as the kernels read it */
typedef struct sw_jpeg_desc {
  uint8_t* out;                       /* (3, height, width) u8; exactly these 3 * height * width bytes are written */
  int64_t coef_off;                   /* int16 elements from `coef` to this image's first block */
  int64_t qtab_off;                   /* uint16 elements from `qtables` to this image's four tables */
  int64_t plane_off;                  /* bytes from `workspace` to component 0's padded plane; the others follow */
  int32_t block_start, quad_start;    /* blocks / 4-pixel row pieces of the images before this one */
  int32_t width, height, ncomp, hsamp, vsamp, bgr;
  int32_t blocks_w[3], blocks_h[3], qtable[3];
  int32_t pad_;
} sw_jpeg_desc;
/* HOST arithmetic: the batch layout.  Image i's coefficients start where image i-1's end (the first at 0), its tables at
 * uint16 256 * i, its planes at 64 bytes per block in the same order: sw_jpeg_workspace_bytes = 64 * all blocks.  bgr: plane order of
 * every output (0: R, G, B).  -6: 2^31 blocks or 4-pixel pieces or more. */
long sw_jpeg_workspace_bytes(int n_images, const sw_jpeg_info* infos);
int sw_jpeg_describe_batch(int n_images, const sw_jpeg_info* infos, void* const* outs, int bgr, sw_jpeg_desc* descs,
                           long* total_blocks, long* total_quads);
/* Two launches whatever n_images is: blocks -> padded component planes in `workspace` (dequantise, IDCT, +128, limit), then planes ->
 * pixels (upsample, convert, plane order).  descs: DEVICE array of n_images entries as sw_jpeg_describe_batch fills them, with the
 * totals it returned; coef, qtables: DEVICE copies of what sw_jpeg_entropy_decode wrote, 16-byte aligned; workspace: 256-byte
 * aligned.  Integer arithmetic only: the same bytes on every run. */
int sw_jpeg_decode_batch(int n_images, const sw_jpeg_desc* descs, long total_blocks, long total_quads, const int16_t* coef,
                         const uint16_t* qtables, uint8_t* workspace, sw_stream_t stream);

const char* sw_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SOSWSOD_HIP_H */
