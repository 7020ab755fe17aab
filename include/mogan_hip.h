/* mogan_hip.h -- C ABI of libmogan_hip.so: the MI355X (gfx950) kernels under the AttnGAN G+D
 * train step of tohinz/multiple-objects-gan.
 *
 * The reference has no FFI: its hot path is stock torch.nn ops composed in python
 * (code/coco/attngan/model.py, GlobalAttention.py, miscc/losses.py, trainer.py:281-342).  Each
 * entry point below replaces the torch op(s) at the cited reference lines; the python package
 * binds them with ctypes (multiple-objects-gan_amd/hip/lib.py) and wraps them in
 * torch.autograd.Function (hip/ops.py).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - arithmetic: fp32 tensors, fp32 accumulation.  The matrix kernels form every fp32 product from the exact three-piece bf16
 *     split of both operands on the bf16 MFMA pipe (six partial products, dropped terms <= 2^-23 |a b|; csrc/mogan_mma.h):
 *     error against fp64 at the level of the native fp32 MFMA instruction, not bit-identical to an fmaf
 *     chain.  mogan_mfma_form() reports the form; -DMOGAN_X6=0 builds the native one;
 *   - all tensors are dense fp32, NCHW, device pointers, borrowed for the duration of the call
 *     (the caller -- PyTorch -- owns the memory); uint8 masks / int32 lengths where stated;
 *   - every call is asynchronous on `stream` (pass torch.cuda.current_stream().cuda_stream) and
 *     allocates nothing: scratch comes from the caller as (ws, ws_bytes); a null/short workspace
 *     only disables split-K (slower, never wrong) unless stated;
 *   - return 0 on success, negative MOGAN_ERR_* otherwise (no exceptions cross the boundary);
 *   - operators keep no state between calls and are thread-safe / re-entrant.  What the library does
 *     hold is TUNING state, never data: a split-K block target (process default + per-stream override,
 *     mogan_gemm_set_split_target / mogan_stream_set_split_target) and the tuned (tile, split-K) table
 *     (mogan_gemm_tune_set), both read under a mutex -- results do not depend on them beyond the
 *     summation order across K-splits; plus the test / measurement hooks marked as such below
 *     (mogan_gemm_debug_force, mogan_prof_*), which are process-wide and
 *     not meant for concurrent use.
 *
 * Arithmetic.  fp32 in, fp32 out, fp32 accumulators everywhere.  In the default build the MFMA kernels (convolutions, bmm)
 * form every product a*b on the bf16 matrix pipe from the exact three-piece bf16 split of both operands (csrc/mogan_mma.h:
 * six partial products, the dropped ones <= 2^-23 |a b|), mogan_mfma_form() == 6.  Measured against fp64 this is within
 * +-25 % of the native fp32 MFMA (libmogan_hip_f32.so, mogan_mfma_form() == 1) on ordinary and on wide-dynamic-range data;
 * the forward error bound  |err| <= 2^-24 * sum |a||b|  holds in every measured case, but under engineered cancellation
 * (result ~1e-4 of the terms) the error relative to the tiny RESULT is up to 17x the native form's, whose fma chain profits
 * from the exact cancellation of adjacent terms (profiles/r02_precision_*.txt).  Input domain of the split form:
 * |x| <= 3.3895e38 (the largest bf16; larger finite values and +-inf give inf / NaN where the native form may stay finite);
 * |x| >= 2^-110 or 0 for full accuracy (below, the third / second piece drops under the smallest normal bf16 and the product
 * keeps 16 / 8 significant bits -- on values whose products are below fp32's normal range anyway).
 * tests/test_kernels_gpu.py::test_fp32_products_on_the_bf16_pipe_* keep these statements under test.
 */
#ifndef MOGAN_HIP_H
#define MOGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* identical to the typedef in <hip/hip_runtime_api.h>; repeated so plain C / ctypes-side tools can
 * include this header without the HIP SDK */
typedef struct ihipStream_t* hipStream_t;

#define MOGAN_ERR_SHAPE (-1)  /* unsupported / inconsistent dimensions */
#define MOGAN_ERR_LAUNCH (-2) /* hip launch error */
#define MOGAN_ERR_WS (-3)     /* workspace required but too small */

/* activation codes shared by the norm / elementwise families */
#define MOGAN_ACT_NONE 0
#define MOGAN_ACT_RELU 1
#define MOGAN_ACT_LRELU 2 /* LeakyReLU(slope) */
#define MOGAN_ACT_GLU 3   /* x[:, :C/2] * sigmoid(x[:, C/2:])   (model.py:24-32) */
#define MOGAN_ACT_TANH 4
#define MOGAN_ACT_SIGMOID 5

int mogan_abi_version(void);
/* split-K of the implicit-GEMM kernels aims at `blocks` workgroups per launch (default 768 = three per CU for a kernel
 * that has the GPU to itself; a caller that keeps several streams busy lowers it to 384: fewer slabs to reduce). */
int mogan_gemm_set_split_target(int blocks);
/* the same per stream (0 = back to the process default): launches on `stream` use this target.  The owner of a stream
 * knows whether its kernels run alone (768) or beside other streams' kernels (384); two engines / threads with their own
 * streams do not interfere. */
int mogan_stream_set_split_target(hipStream_t stream, int blocks);

/* Tuned dispatch of the implicit-GEMM kernel: for the GEMM (mode 0 conv fwd / 1 conv dgrad / 2 conv wgrad / 3 bmm; M, N, K,
 * nz = batch or parity classes, exactly as the kernel sees them) use tile config `cfg` (0..4) and split-K factor `split`
 * instead of the heuristic.  Entries come from timing every (cfg, split) pair on the device (tools/tune_gemm.py ->
 * multiple-objects-gan_amd/hip/tuned_gemm_gfx950.csv); the host registers them once after loading the library.
 * mogan_gemm_tune_clear() drops all entries.  Results do not depend on the entry (same sums per split, fixed order). */
int mogan_gemm_tune_set(int mode, int M, int N, int K, int nz, int cfg, int split);
int mogan_gemm_tune_clear(void);

/* Process set-up, not an operator: create `n` idle non-blocking HIP streams that live until the process ends.  HIP
 * multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues in the order the streams are created, and
 * streams that share a queue are processed in order; the multi-stream train step calls this once, right after selecting
 * the device and before any other stream exists, so that its own streams (and RCCL's) land on the queues in the measured
 * arrangement ("hardware queues").  Returns the number of streams held, or a negative error. */
int mogan_reserve_streams(int n);

/* test hook: force a GEMM tile config (0..4; -1 = the default dispatch; -2 = the default dispatch without the Winograd kernels, so
 * that 3x3 stride-1 shapes reach the direct kernels) and a split-K factor (0 = heuristic) */
int mogan_gemm_debug_force(int cfg, int split);
/* tuning hook: grouped launches (mogan_conv2d_*_group) with fewer tiles than this run their members one by one (default 1600, see csrc/mogan_gemm.hip) */
int mogan_gemm_group_min_tiles(int tiles);
/* which matrix instruction the MFMA kernels of this build use for their fp32 products: 6 = split-bf16 form (three bf16 pieces
 * per operand, six v_mfma_f32_32x32x16_bf16 partial products per 16 k; csrc/mogan_mma.h -- the default), 1 = native
 * v_mfma_f32_32x32x2_f32 (-DMOGAN_X6=0).  bench.py prices its roofline against the matching peak. */
int mogan_mfma_form(void);

/* measurement hook (bench.py roofline leg): with profiling enabled every gemm_kernel launch is bracketed by
 * HIP events on its own stream; collect() returns rows of 5 doubles {mode (0 fwd,1 dgrad,2 wgrad,3 bmm),
 * tile config, launches, algorithmic flops = sum 2*M*N*K of the true GEMM dims, milliseconds} and the row count.
 * Not for use under hipGraph capture. */
int mogan_prof_enable(int on);
int mogan_prof_collect(double* out, int max_rows);
/* same records as one CSV row per launch (geometry, algorithmic GFLOP, ms); consumes them */
int mogan_prof_dump(const char* path);

/* ---------------------------------------------------------------- convolution (fp32 MFMA implicit GEMM)
 * x (B,Cin,Hs,Ws), w (Cout,Cin,KH,KW), y (B,Cout,OH,OW), no bias.  up=1 fuses nn.Upsample(x2,nearest)
 * in front of the conv (upBlock, model.py:48-55): the conv then sees H=2Hs, W=2Ws.
 * OH = (H + 2*ph - KH)/stride + 1.  Replaces nn.Conv2d at model.py:35-44,92-99,587,598-609,626,664-677. */
int mogan_conv2d_out_dims(int Hs, int Ws, int KH, int KW, int stride, int ph, int pw, int up, int* OH, int* OW);
int mogan_conv2d_fwd(const float* x, const float* w, float* y, int B, int Cin, int Hs, int Ws, int Cout, int KH,
                     int KW, int stride, int ph, int pw, int up, void* ws, size_t ws_bytes, hipStream_t stream);
/* The discriminators' logits head in one launch each way: p (B,Cout) = sigmoid(<x[b], w[co]> + bias[co]) over K = Cin*KH*KW --
 * nn.Conv2d(8 ndf, 1, kernel_size=4, stride=4) (with bias) on a 4x4 map followed by nn.Sigmoid (model.py:626-627, 640-641);
 * x (B,K) and w (Cout,K) dense, K % 4 == 0, Cout <= 4.  Backward from dp and p: dx (B,K) (NULL = not wanted), dw (Cout,K) and
 * db (Cout) written or accumulated (NULL = not wanted; the images are summed in order).
 * MOGAN_ERR_SHAPE before any HIP call: B or K <= 0, Cout outside 1..4, a NULL x / w / p (fwd; bias alone is nullable: no bias) or
 * dp / p / x / w (bwd; dx / dw / db are nullable); in the forward also K % 4 != 0 and an x or w that is not 16-byte aligned; in the
 * backward B K >= 2^31.  dx, dw and db all NULL: returns 0 and launches nothing.
 * tests/test_loss_entry_points_gpu.py holds both entries per element against fp64 (tests/loss_cases.py), under the memory contract
 * of tests/memguard.py; tests/test_loss_rejections_cpu.py holds the rejections. */
int mogan_logits_head_fwd(const float* x, const float* w, const float* bias, float* p, int B, int K, int Cout,
                          hipStream_t stream);
int mogan_logits_head_bwd(const float* dp, const float* p, const float* x, const float* w, float* dx, float* dw, float* db,
                          int B, int K, int Cout, int accumulate, hipStream_t stream);
/* z = LeakyReLU_slope(conv2d(x, w)) in one launch: the first layer of every discriminator -- nn.Conv2d(3, ndf, 4, 2, 1)
 * followed by nn.LeakyReLU(0.2) with no BatchNorm in between (model.py:597-598, 660-661).  Returns 0 = done, 1 = not a geometry
 * for this kernel (run mogan_conv2d_fwd + mogan_act_fwd), < 0 = error.  Backward: mogan_act_bwd with z in place of the
 * pre-activation (same sign), then the convolution's gradients. */
int mogan_conv2d_lrelu_fwd(const float* x, const float* w, float* z, int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW,
                           int stride, int ph, int pw, float slope, void* ws, size_t ws_bytes, hipStream_t stream);
/* conv (no upsample) with y = relu?(scale[co]*conv + shift[co]) applied in the kernel epilogue: BasicConv2d of the frozen,
 * eval-mode Inception trunk (conv -> BN on running statistics -> ReLU; model.py:258-299) in one pass over the output */
int mogan_conv2d_affine_fwd(const float* x, const float* w, const float* scale, const float* shift, float* y, int B,
                            int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int relu,
                            void* ws, size_t ws_bytes, hipStream_t stream);
/* its backward up to the conv: dx = dy * scale[c] * (y > 0), from the saved OUTPUT y (B,C,HW) */
int mogan_affine_relu_bwd_out(const float* y, const float* dy, const float* scale, float* dx, int B, int C, int HW,
                              hipStream_t stream);
/* dx: gradient w.r.t. the conv input in the H x W domain, (B,Cin,H,W); for up=1 follow with mogan_down2_sum */
/* Grouped launches for the frozen trunk: up to 4 INDEPENDENT convolutions of one dependency level of a Mixed block (same
 * direction, arbitrary geometries) run as one launch whose 1-D grid is the concatenation of the problems' tile grids -- at
 * B = 16 each of them alone needs split-K (+ a reduction launch) to fill the chip.  Field meaning = the arguments of
 * mogan_conv2d_affine_fwd_ex / mogan_conv2d_dgrad_ex.  Outputs of a group must not overlap. */
typedef struct MoganConvFwdArgs {
    const float* x; long long x_bstride; const float* w; const float* scale; const float* shift;
    float* y; long long y_bstride; float* y2; long long y2_bstride; int msplit;
    int B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw, relu;
} MoganConvFwdArgs;
typedef struct MoganConvDgradArgs {
    const float* dy; long long dy_bstride; const float* w; float* dx; long long dx_bstride;
    const float* relu_of; long long relu_bstride; int accumulate;
    int B, Cin, Hs, Ws, Cout, KH, KW, stride, ph, pw;
} MoganConvDgradArgs;
int mogan_conv2d_affine_fwd_group(int n, const MoganConvFwdArgs* args, void* ws, size_t ws_bytes, hipStream_t stream);
int mogan_conv2d_dgrad_group(int n, const MoganConvDgradArgs* args, void* ws, size_t ws_bytes, hipStream_t stream);
/* Channel-slice addressing for the frozen Inception trunk (model.py:258-299): x is a slice (batch stride x_bstride
 * elements) of a larger NCHW tensor; output channels [0, msplit) go to y (batch stride y_bstride, -1 = dense), channels
 * [msplit, Cout) to y2 (y2 nullable: everything to y).  One launch then serves a group of same-input 1x1 convolutions whose
 * parts land in different tensors, and every branch of a Mixed block writes straight into the block's concatenated
 * output. */
int mogan_conv2d_affine_fwd_ex(const float* x, long long x_bstride, const float* w, const float* scale, const float* shift,
                               float* y, long long y_bstride, float* y2, long long y2_bstride, int msplit, int B, int Cin,
                               int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int relu, void* ws,
                               size_t ws_bytes, hipStream_t stream);
/* Plain forward convolution with channel-slice addressing, a ReLU mask on the result (relu_of: shaped like y, nullable) and
 * accumulation into y.  Used as the data gradient of the frozen trunk's stride-1 convolutions: dX = conv(dY, flipped and
 * (ci,co)-transposed filters, pad K-1-pad) reads the filter operand K-contiguously (the data-gradient mode gathers it with a
 * stride of KH*KW floats). */
int mogan_conv2d_fwd_ex(const float* x, long long x_bstride, const float* w, float* y, long long y_bstride,
                        const float* relu_of, long long relu_bstride, int accumulate, int B, int Cin, int Hs, int Ws,
                        int Cout, int KH, int KW, int stride, int ph, int pw, void* ws, size_t ws_bytes, hipStream_t stream);
/* Data gradient with channel-slice addressing and a fused ReLU backward: dy is a slice with batch stride dy_bstride, the
 * result is written (accumulate 0) or added (1) to the slice dx (batch stride dx_bstride); where relu_of[...] <= 0 (a
 * slice shaped like dx with batch stride relu_bstride; nullable) the new contribution is zeroed first. */
int mogan_conv2d_dgrad_ex(const float* dy, long long dy_bstride, const float* w, float* dx, long long dx_bstride,
                          const float* relu_of, long long relu_bstride, int accumulate, int B, int Cin, int Hs, int Ws,
                          int Cout, int KH, int KW, int stride, int ph, int pw, void* ws, size_t ws_bytes,
                          hipStream_t stream);
int mogan_conv2d_dgrad(const float* dy, const float* w, float* dx, int B, int Cin, int Hs, int Ws, int Cout, int KH,
                       int KW, int stride, int ph, int pw, int up, void* ws, size_t ws_bytes, hipStream_t stream);
/* ---- Prepared filter images for the Winograd convolutions (round 6; csrc/mogan_wino.hip).  The 3x3 stride-1 convolutions of the
 * generator's ResBlocks (code/coco/attngan/model.py:67-81) run as fused Winograd F(2x2,3x3); their filters enter the kernel
 * transformed (G g G^t) and pre-split into bf16 pieces.  mogan_conv2d_fwd / mogan_conv2d_dgrad build that image per call at the
 * head of the workspace -- one more launch on the convolution's own chain, per use.  A caller that owns the weights (the
 * optimizer) keeps the image instead, one per weight and direction, rebuilds ALL images of a network in one launch right after
 * its optimizer step, and hands it to the *_wp entry points; the library keeps no weight state.
 *   mogan_wino_prep_bytes   size of the image for this convolution geometry and direction (dgrad = 0 forward, 1 data gradient);
 *                           0 = this convolution does not take the Winograd kernels (no image is needed, wprep stays NULL)
 *   mogan_wino_prep_group   images of n (weight, direction) pairs in one launch (32 per launch beyond that); prep[i] 16-byte aligned
 *   mogan_conv2d_fwd_wp /   mogan_conv2d_fwd / mogan_conv2d_dgrad with the caller's image of w for that direction (wprep NULL: the
 *   mogan_conv2d_dgrad_wp   plain entry points' behaviour).  The image must have been built from the current values of w. */
size_t mogan_wino_prep_bytes(int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int up, int dgrad);
int mogan_wino_prep_group(int n, const float* const* w, void* const* prep, const int* Cout, const int* Cin, const int* dgrad,
                          hipStream_t stream);
/* The same for whichever kernel a convolution's geometry takes (round 6, third session): besides the Winograd image of a 3x3 s1 p1
 * convolution, the pre-split filter image of dconv2_fwd_kernel for the discriminators' 4x4 s2 p1 convolutions
 * (code/coco/attngan/model.py:575-613: forward over the space-to-depth image, data gradient by parity classes; csrc/mogan_dconv2.hip),
 * which mogan_conv2d_fwd / _dgrad otherwise rebuild per call (44 prep launches per train step for weights that change once).
 *   mogan_conv_prep_bytes   as mogan_wino_prep_bytes for any geometry: the size of the image mogan_conv2d_fwd_wp / _dgrad_wp expect as
 *                           wprep for it (found by a dry run of the same dispatch), 0 = none
 *   mogan_conv_prep_group   as mogan_wino_prep_group with the filter size KH[i] (3 or 4) per member: one launch per kind and 32 members */
size_t mogan_conv_prep_bytes(int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int up, int dgrad);
int mogan_conv_prep_group(int n, const float* const* w, void* const* prep, const int* Cout, const int* Cin, const int* KH,
                          const int* dgrad, hipStream_t stream);
int mogan_conv2d_fwd_wp(const float* x, const float* w, const void* wprep, float* y, int B, int Cin, int Hs, int Ws, int Cout, int KH,
                        int KW, int stride, int ph, int pw, int up, void* ws, size_t ws_bytes, hipStream_t stream);
int mogan_conv2d_dgrad_wp(const float* dy, const float* w, const void* wprep, float* dx, int B, int Cin, int Hs, int Ws, int Cout,
                          int KH, int KW, int stride, int ph, int pw, int up, void* ws, size_t ws_bytes, hipStream_t stream);
/* dw (Cout,Cin,KH,KW); accumulate != 0 adds into dw */
int mogan_conv2d_wgrad(const float* dy, const float* x, float* dw, int B, int Cin, int Hs, int Ws, int Cout, int KH,
                       int KW, int stride, int ph, int pw, int up, int accumulate, void* ws, size_t ws_bytes,
                       hipStream_t stream);

/* ---- Weight-heavy convolutions on pre-split "panels" (csrc/mogan_pgemm.hip): the deep discriminator layers
 * (code/coco/attngan/model.py:594-613, 616-642, 738-760) are GEMMs with 768..3072 x 6144..27648 weights against a few hundred
 * pixels.  Their weights change once per optimizer step but are used by the real, the fake and the generator pass, so the
 * caller keeps -- next to the fp32 master -- a PACKED copy per direction: the three bf16 pieces of every weight (see
 * "Arithmetic" above) in the order the matrix instruction consumes them.  The convolution entry points below read the packed
 * copy with plain 16-byte loads and pack the activations per call into the workspace (channels-last bf16 pieces); results are
 * the same fp32 products as mogan_conv2d_fwd / mogan_conv2d_dgrad up to the summation order.
 *   mogan_pk_conv_eligible   1 if the geometry meets the panel formats' constraints (forward: Cin % 32 == 0; data gradient:
 *                            Cout % 32 == 0, KH, KW, Hs, Ws multiples of the stride) AND the layer is weight-heavy enough for
 *                            the path to pay (<= 64 output pixels per image and parity class, K >= 1024, >= 128 rows); else 0
 *   mogan_pk_weight_bytes    size of the packed copy for one direction (dgrad = 0 forward, 1 data gradient); 0 = not packable
 *   mogan_pk_weight_pack     w (Cout,Cin,KH,KW) fp32 -> packed copy; the caller re-packs after every change of w (it owns the
 *                            buffer and the bookkeeping: the library keeps no weight state)
 *   mogan_conv2d_fwd_pk      y = conv2d(x, w) from the forward-packed weights;  workspace: B*Hs*Ws*Cin*6 bytes + split-K slabs
 *   mogan_conv2d_dgrad_pk    dx = conv2d data gradient from the dgrad-packed weights; workspace: B*OH*OW*Cout*6 bytes + slabs
 *                            (both need the workspace for the packed activations: where it is NULL or smaller than that panel,
 *                            rounded up to 256 bytes, they return MOGAN_ERR_WS and write nothing; a workspace that holds the
 *                            panel but not two slabs only disables the K-split)
 *   mogan_pk_debug_force     test hook (process-wide): take_all != 0 drops the size heuristic of mogan_pk_conv_eligible (hard
 *                            constraints stay); cfg in 0..2 forces a tile shape (-1 = heuristic), split > 0 a K-split count */
int mogan_pk_conv_eligible(int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int dgrad);
size_t mogan_pk_weight_bytes(int Cout, int Cin, int KH, int KW, int stride, int dgrad);
int mogan_pk_weight_pack(const float* w, void* wpk, int Cout, int Cin, int KH, int KW, int stride, int ph, int pw, int dgrad,
                         hipStream_t stream);
/* both copies from one read of w (Cin % 32 == 0 and Cout % 32 == 0): what the owner of the weight calls after its optimizer step */
int mogan_pk_weight_pack_both(const float* w, void* wpk_fwd, void* wpk_dgrad, int Cout, int Cin, int KH, int KW, int stride, int ph,
                              int pw, hipStream_t stream);
/* the optimizer step of ONE such weight and both copies in one pass: p, m, v (and ema, nullable) are updated exactly as
 * mogan_adam_step updates them (same arithmetic, csrc/mogan_adam.h), both panels are written from the new p exactly as
 * mogan_pk_weight_pack_both writes them, and g is cleared behind its read when zero_g != 0 (left as it is otherwise).
 * p / g / m / v / ema: (Cout, Cin, KH, KW) dense, 16-byte aligned.  dev_state != NULL: step size and bias correction are read
 * from it as mogan_adam_prep left them (lr and step are ignored; the count is NOT advanced here: one mogan_adam_prep per bucket
 * step, in front of all its launches); NULL: from lr and the 1-based step.  MOGAN_ERR_SHAPE before any launch: a NULL or
 * misaligned pointer, step < 1 without dev_state, a geometry mogan_pk_weight_bytes declines in either direction,
 * Cin % 32 != 0, Cout % 32 != 0, KH * KW not in {16, 9, 1}. */
int mogan_pk_adam_pack_both(float* p, float* g, float* m, float* v, float* ema, void* wpk_fwd, void* wpk_dgrad, int Cout, int Cin,
                            int KH, int KW, int stride, int ph, int pw, float lr, float beta1, float beta2, float eps, int step,
                            const float* dev_state, int eps_mode, float grad_scale, float ema_decay, int zero_g,
                            hipStream_t stream);
int mogan_conv2d_fwd_pk(const float* x, const void* wpk, float* y, int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW,
                        int stride, int ph, int pw, void* ws, size_t ws_bytes, hipStream_t stream);
int mogan_conv2d_dgrad_pk(const float* dy, const void* wpk, float* dx, int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW,
                          int stride, int ph, int pw, void* ws, size_t ws_bytes, hipStream_t stream);
int mogan_pk_debug_force(int take_all, int cfg, int split);
/* weight gradient of the same weight-heavy layers on the packed kernels: dY and the transposed im2col matrix of x are packed per
 * call into the workspace (ws_bytes >= what mogan_pk_wgrad_eligible checks: ~ (Cout + Cin*KH*KW) * B*OH*OW * 6 bytes), dW
 * (Cout,Cin,KH,KW) is written or (accumulate != 0) added to.  Same fp32 products as mogan_conv2d_wgrad, other summation order.
 * A workspace that does not hold both packed operands: MOGAN_ERR_WS, dW untouched. */
int mogan_pk_wgrad_eligible(int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, size_t ws_bytes);
int mogan_conv2d_wgrad_pk(const float* dy, const float* x, float* dw, int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW,
                          int stride, int ph, int pw, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);

/* Deep block = conv -> BatchNorm2d (training statistics) -> LeakyReLU / ReLU / nothing on a map with B*OH*OW <= 2048 values per
 * channel (downBlock / Block3x3_leakRelu of the deep discriminator layers, model.py:575-613, 616-642): the packed-weight GEMM
 * followed by ONE tail kernel that sums the K-split slabs, computes the batch statistics (8 channels per block, a channel's
 * values stay in registers), updates the running statistics, applies BN + activation and writes the NEXT layer's pixel panel --
 * 2 launches where conv + split-K reduce + bn_stats (2) + bn_act_fwd + the activation pack took 6; the backward is one tail
 * kernel (activation + BN backward, d gamma / d beta, the gradient's pixel panel) + the packed data-gradient GEMM.
 *   forward   x (B,Cin,Hs,Ws) fp32 and/or its pixel panel xpanel (nullable: packed here into the workspace), wpk = forward
 *             packed weights; outputs y = conv(x) (B,Cout,OH,OW: the BN input, kept for the backward), stats = mean[Cout] |
 *             invstd[Cout], z = act(BN(y)), zpanel (nullable) = pixel panel of z, mogan_pk_panel_bytes(B, Cout, OH*OW) bytes;
 *             rmean / rvar updated like nn.BatchNorm (momentum, unbiased variance), nullable
 *   backward  dz -> dy (B,Cout,OH,OW: gradient at the conv output, what the weight gradient needs), dgamma / dbeta (nullable;
 *             accumulate != 0 adds), dx (nullable: no data gradient) from wpk_dgrad = data-gradient packed weights
 *   groups    1, or 2 (round 5): the B images are `groups` batches of B / groups images one behind the other which the reference
 *             passes through the layer in separate calls -- D(real) and D(fake.detach()) of a discriminator update,
 *             miscc/losses.py:136-174 --: ONE convolution over all B images (the weights stream once), batch statistics per
 *             group (stats = mean[groups][Cout] | invstd[groups][Cout]), running statistics updated group after group in that
 *             order, d gamma / d beta = the groups' sums.  B / groups * OH*OW <= 2048.
 * Same arithmetic as mogan_bn_stats / mogan_bn_act_fwd / mogan_bn_act_bwd (fp64 sums).
 * Nullable: x or xpanel (not both), rmean, rvar, zpanel (forward); dgamma, dbeta, dx -- and with dx NULL also wpk_dgrad and ws
 * (backward).  Every rejection precedes the first launch, so a declined call has written nothing: MOGAN_ERR_SHAPE for B <= 0,
 * groups outside 1..2, B % groups, Cin % 32, Cout % 32, stride <= 0, an empty output map, B / groups * OH*OW > 2048 / groups, an
 * activation other than NONE / RELU / LRELU, KH*KW > 25, a NULL required pointer (forward: wpk, gamma, beta, y, stats, z, and x
 * with xpanel; backward: dz, y, stats, gamma, beta, dy) and, where dx is wanted, KH, KW, Hs or Ws no multiple of the stride or
 * Cin <= 0; MOGAN_ERR_WS for a workspace that is NULL or does not hold the panel that has to be packed (forward without xpanel:
 * B*Hs*Ws*Cin*6 bytes, backward with dx: B*OH*OW*Cout*6, each rounded up to 256) and, with dx, a NULL wpk_dgrad.  Behind the
 * panel the forward keeps its K-split slabs (4*B*Cout*OH*OW bytes each); room for fewer than two only disables the split. */
size_t mogan_pk_panel_bytes(int B, int C, int HW);
int mogan_deep_block_eligible(int B, int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int act,
                              int groups);
int mogan_deep_conv_bn_act_fwd(const float* x, const void* xpanel, const void* wpk, const float* gamma, const float* beta,
                               float* rmean, float* rvar, float* y, float* stats, float* z, void* zpanel, int B, int Cin, int Hs,
                               int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, float eps, float momentum, int act,
                               float slope, int groups, void* ws, size_t ws_bytes, hipStream_t stream);
int mogan_deep_conv_bn_act_bwd(const float* dz, const float* y, const float* stats, const float* gamma, const float* beta,
                               const void* wpk_dgrad, float* dy, float* dgamma, float* dbeta, int accumulate, float* dx, int B,
                               int Cin, int Hs, int Ws, int Cout, int KH, int KW, int stride, int ph, int pw, int act, float slope,
                               int groups, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- Frozen CNN_ENCODER trunk on pixel panels (code/coco/attngan/model.py:258-299: Mixed_5b .. Mixed_7c of the frozen, eval-mode
 * Inception-v3; trainer.py:329-333 sends only the image gradient through it).  With frozen weights every filter is packed ONCE
 * (mogan_pk_weight_pack of the, where needed zero-padded, filters); activations and gradients travel between the layers as pixel
 * panels (channels-last bf16 pieces, 192 bytes per pixel and group of 32 channels; a tensor's channel slices start at multiples
 * of 32), so a convolution is the packed-operand GEMM alone and everything around it -- K-split sum, eval-mode BatchNorm affine,
 * ReLU / ReLU mask, the 3x3 average pool of the pool branch (moved behind the 1x1 convolution: both are linear), accumulation of a
 * gradient with several contributors, the fp32 copy and the next layer's panel -- is ONE tail launch per dependency level.
 *   mogan_pk_group          n <= 8 independent GEMMs in one launch: forward (dgrad = 0: rows = Cout, K = KH*KW*Cp, tap-major) or
 *                           stride-1 data gradient (dgrad = 1: rows = Cin, K = KH*KW*Cp over the dY panel).  raw receives
 *                           nsplit slabs of (B, M, outH, outW) fp32; nsplit is in/out (asked for / written).
 *   mogan_panel_tail_group  n <= 8 slices: v = sum of the sources' slabs; [box, below]; [v = v * scale[c] + shift[c]]; [relu];
 *                           [v += add]; [v = 0 where mask <= 0]; -> dst (fp32, nullable) and the panel slice (nullable;
 *                           channels n .. roundup32(n) are written as zeros).
 *                           box = 0: none.  box = 1: 3x3 sum with zero padding, x 1/9 (F.avg_pool2d(x, 3, 1, 1)).
 *                           box = 2: 3x3 sum over the taps inside the map, divided (a true fp32 division) by their number, 1, 2,
 *                           3, 4, 6 or 9 (count_include_pad=False; still a per-pixel linear map, so it commutes with a 1x1
 *                           convolution as box = 1 does).  box = 3: maximum over the taps inside the map (F.max_pool2d(x, 3, 1, 1);
 *                           NaN inputs undefined): exactly one source of one slab, else MOGAN_ERR_SHAPE; it does not commute
 *                           with a convolution.  Any other value is MOGAN_ERR_SHAPE.  Groups whose members all have box <= 1
 *                           run the kernels they always ran; box 2 / 3 are the pool branches of the published FID network
 *                           (attngan/inception.py, variant "fid"), forward only. */
typedef struct MoganPkArgs {
    const void* wpk; const void* panel; float* raw;
    int B, M;                 /* images, rows of the result */
    int Cp, CGp, cg0;         /* channels of the K range per tap (multiple of 32); channel groups per pixel of the panel; first group */
    int PH, PW, outH, outW;   /* image dims of the panel / of the result */
    int KH, KW, stride, ph, pw, dgrad;
    int nsplit;
} MoganPkArgs;
#define MOGAN_TAIL_MAXSRC 3
typedef struct MoganTailArgs {
    const float* src[MOGAN_TAIL_MAXSRC]; long long src_bs[MOGAN_TAIL_MAXSRC]; long long src_slab[MOGAN_TAIL_MAXSRC];
    int src_nsplit[MOGAN_TAIL_MAXSRC]; int nsrc;
    const float* add; long long add_bs;
    const float* mask; long long mask_bs;
    const float* scale; const float* shift;
    int relu, box;
    float* dst; long long dst_bs;
    void* panel; int CGp, cg0;
    int B, n, H, W;           /* images, channels of the slice, map */
} MoganTailArgs;
int mogan_pk_group(int n, MoganPkArgs* args, hipStream_t stream);
int mogan_panel_tail_group(int n, const MoganTailArgs* args, hipStream_t stream);

/* nn.Upsample(scale_factor=2, mode='nearest') + conv3x3(padding 1, no bias) -- every upBlock of the reference
 * (code/coco/attngan/model.py:48-55, code/coco/stackgan/model.py:16-22) -- evaluated as the TRANSPOSED 4x4
 * stride-2 pad-1 convolution with kernel K = T w T^t, T = [[0,0,1],[0,1,1],[1,1,0],[1,0,0]]: each phase of the
 * upsampled grid sees only 2x2 distinct source pixels, so 4 multiply-adds per output pixel replace 9 (same result up
 * to the fp32 rounding of the pre-summed weights).  x (B,Cin,Hs,Ws), w (Cout,Cin,3,3), y (B,Cout,2Hs,2Ws).
 * dgrad returns dx at the SOURCE resolution (B,Cin,Hs,Ws) (no mogan_down2_sum).  The workspace must hold
 * mogan_upconv3x3_ws_bytes(Cout,Cin) for K (dK in wgrad) in front of the split-K scratch of the inner conv; where it does not
 * (or is NULL) fwd / dgrad / wgrad return MOGAN_ERR_WS and write nothing. */
size_t mogan_upconv3x3_ws_bytes(int Cout, int Cin);
/* K (Cin, Cout, 4, 4) of w alone: a caller that owns w keeps K per weight version (and, with mogan_conv_prep_*, the filter image of
 * the kernel that runs the virtual 4x4 s2 convolution) and then calls mogan_conv2d_dgrad_wp(x, K, image, y, B, Cout, 2 Hs, 2 Ws, Cin,
 * 4, 4, 2, 1, 1, 0, ...) for the forward / mogan_conv2d_fwd_wp(dy, K, image, dx, ...) for the data gradient -- the calls
 * mogan_upconv3x3_fwd / _dgrad make after building K per call (same results) */
int mogan_upconv3x3_k4(const float* w, float* k4, int Cout, int Cin, hipStream_t stream);
/* the K of n weights in one launch (what an owner calls behind its optimizer step) */
int mogan_upconv3x3_k4_group(int n, const float* const* w, float* const* k4, const int* Cout, const int* Cin, hipStream_t stream);
int mogan_upconv3x3_fwd(const float* x, const float* w, float* y, int B, int Cin, int Hs, int Ws, int Cout, void* ws,
                        size_t ws_bytes, hipStream_t stream);
int mogan_upconv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int Cin, int Hs, int Ws, int Cout, void* ws,
                          size_t ws_bytes, hipStream_t stream);
int mogan_upconv3x3_wgrad(const float* dy, const float* x, float* dw, int B, int Cin, int Hs, int Ws, int Cout,
                          int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);
/* backward of nearest x2 upsample: dx[b,c,y,x] = sum of the 2x2 block of du (B*C planes of 2H x 2W).
 * MOGAN_ERR_SHAPE before any HIP call: planes, H or W <= 0, a NULL du or dx. */
int mogan_down2_sum(const float* du, float* dx, int planes, int H, int W, hipStream_t stream);

/* generic strided batched GEMM: C[z][m][n] (+)= sum_k A[z][m][k] * B[z][k][n]; strides in elements.
 * Replaces nn.Linear (model.py:324,365,371) and torch.bmm (GlobalAttention.py:46,66,100,118). */
int mogan_bmm(const float* a, const float* b, float* c, int batch, int M, int N, int K, long long sAb, long long sAm,
              long long sAk, long long sBb, long long sBk, long long sBn, long long sCb, long long sCm, long long sCn,
              int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---------------------------------------------------------------- batch norm (+ fused activation)
 * x (B,C,HW) [HW=1: BatchNorm1d].  Training-mode statistics: mean[C], invstd[C] = 1/sqrt(var_biased+eps);
 * running_mean/var (nullable) updated with `momentum` (unbiased var), as nn.BatchNorm*d does.
 * ws: >= mogan_bn_ws_bytes(B,C,HW) bytes, REQUIRED. */
size_t mogan_bn_ws_bytes(int B, int C, int HW);
int mogan_bn_stats(const float* x, int B, int C, int HW, float eps, float momentum, float* mean, float* invstd,
                   float* running_mean, float* running_var, void* ws, size_t ws_bytes, hipStream_t stream);
/* y = act(gamma*(x-mean)*invstd + beta) (+ residual).  GLU: y has C/2 channels. residual nullable, shaped like y.
 * BN+GLU: model.py:52-54,62-63,72-73,366-367; BN+LeakyReLU: 96-101,579,588-589,602-611; BN+ReLU: 372-373;
 * BN+residual: 75,80. */
int mogan_bn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* residual, float* y, int B, int C, int HW, int act, float slope, hipStream_t stream);
/* The running-statistics update of a BatchNorm call that was made with running_mean = running_var = NULL, from the batch
 * statistics that call wrote (mean / invstd, n = B*HW values per channel): nn.BatchNorm's momentum update with the unbiased
 * variance.  Lets a call's arithmetic run EARLIER than its place in the reference's call order while the running buffers are
 * updated in that order: round 5 evaluates the real-image terms of discriminator_loss (miscc/losses.py:146-160: D(real), the
 * conditional head on real and on the "wrong" pairs) and back-propagates them before the fake images exist; the reference
 * calls COND_DNET on the fake features BEFORE the wrong pairs, so the wrong call's update is deferred behind the fake call's. */
int mogan_bn_running_update(const float* mean, const float* invstd, float* running_mean, float* running_var, int C, long long n,
                            float eps, float momentum, hipStream_t stream);

/* mogan_bn_stats + mogan_bn_act_fwd in one call (training-mode BatchNorm + activation, model.py:48-81, 575-613): maps with
 * B*HW <= 4096 values per channel (and HW >= 16) take ONE launch -- a block per output channel reduces, finalises and applies --,
 * larger ones the three launches of the two calls above; mean / invstd [C] are written for mogan_bn_act_bwd either way (which
 * takes the matching one-launch kernel for the same shapes).  ws as for mogan_bn_stats on the larger maps (MOGAN_ERR_WS, nothing
 * written, where it is NULL or short); the one-launch shapes do not need it and do not look at it (NULL / 0 is fine there). */
int mogan_bn_act_fwd_fused(const float* x, const float* gamma, const float* beta, const float* residual, float* running_mean,
                           float* running_var, float* mean, float* invstd, float* y, int B, int C, int HW, int act, float slope,
                           float eps, float momentum, void* ws, size_t ws_bytes, hipStream_t stream);
/* G BatchNorm(train)+activation calls on the G groups of B images of one (G*B, C, HW) tensor, one launch each way (the object
 * pathways of INIT_STAGE_G / D_NET64, model.py:395-407, 662-672: one BatchNorm call per object): group g uses its own
 * batch statistics (mean / invstd: G x C floats, group-major), the running statistics are updated G times in group order, d gamma /
 * d beta sum over the groups.  B*HW <= 4096 per group (mogan_bn_act_grouped_eligible), any HW >= 1. */
int mogan_bn_act_grouped_eligible(int G, int B, int C, int HW);
int mogan_bn_act_grouped_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* mean,
                             float* invstd, float* y, int G, int B, int C, int HW, int act, float slope, float eps, float momentum,
                             hipStream_t stream);
int mogan_bn_act_grouped_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             float* dx, float* dgamma, float* dbeta, int G, int B, int C, int HW, int act, float slope, int accumulate,
                             hipStream_t stream);
/* dy (B,Cy,HW) -> dx (B,C,HW), dgamma[C], dbeta[C] (accumulate != 0 adds into dgamma/dbeta).
 * The residual branch's gradient is dy itself. ws REQUIRED (mogan_bn_ws_bytes). */
int mogan_bn_act_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int act,
                     float slope, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream);
/* eval-mode BN / per-channel affine fused with an activation: y = act(x*scale[c] + shift[c]);
 * bwd: dx = dy * act'(.) * scale[c].  (frozen Inception BasicConv2d under CNN_ENCODER, model.py:227-242) */
int mogan_affine_act_fwd(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                         int act, float slope, hipStream_t stream);
int mogan_affine_act_bwd(const float* x, const float* dy, const float* scale, const float* shift, float* dx, int B,
                         int C, int HW, int act, float slope, hipStream_t stream);

/* ---------------------------------------------------------------- elementwise
 * act in {RELU, LRELU, GLU (over channel dim: x (B,C,HW) -> y (B,C/2,HW)), TANH, SIGMOID}.
 * bwd takes the forward INPUT x (and recomputes).  model.py:93,328,373,470,599,627,659 */
int mogan_act_fwd(const float* x, float* y, int B, int C, int HW, int act, float slope, hipStream_t stream);
int mogan_act_bwd(const float* x, const float* dy, float* dx, int B, int C, int HW, int act, float slope,
                  hipStream_t stream);
/* y (rows,C,HW) += bias[C];  dbias[c] (+)= sum over rows,HW of dy */
int mogan_bias_add(float* y, const float* bias, int rows, int C, int HW, hipStream_t stream);
int mogan_bias_grad(const float* dy, float* dbias, int rows, int C, int HW, int accumulate, hipStream_t stream);
/* y = a + b (n elements); y = a*alpha.  These two and the group pair below: plain IEEE fp32 operations, one per element and
 * group.  n == 0 is answered first, with 0 and without a launch (an empty tensor's pointer is NULL).
 * MOGAN_ERR_SHAPE before any HIP call: n < 0, G <= 0, a NULL pointer. */
int mogan_add(const float* a, const float* b, float* y, long long n, hipStream_t stream);
/* y = ((x_0 + x_1) + x_2) + ... over the G groups of n values of x (G*n values); backward: dx_g = dy for every group */
int mogan_group_sum(const float* x, float* y, long long n, int G, hipStream_t stream);
int mogan_group_bcast(const float* dy, float* dx, long long n, int G, hipStream_t stream);
int mogan_scale(const float* a, float alpha, float* y, long long n, hipStream_t stream);

/* softmax over L of x viewed as (outer, L, inner), y = softmax(scale*x) restricted to the first
 * lens[o*inner+i] entries (lens nullable = all L); masked entries get 0.  bwd: dx = scale*y*(dy - sum(y*dy)).
 * GlobalAttention.py:50,58 (func_attention, DAMSM).  lens is clamped to [0, L]; a column with no entry left is all zeros.
 * MOGAN_ERR_SHAPE before any HIP call: outer, L or inner <= 0, a NULL x / y (fwd), y / dy / dx (bwd). */
int mogan_softmax_fwd(const float* x, float* y, const int32_t* lens, long long outer, int L, long long inner,
                      float scale, hipStream_t stream);
int mogan_softmax_bwd(const float* y, const float* dy, float* dx, const int32_t* lens, long long outer, int L,
                      long long inner, float scale, hipStream_t stream);

/* ---------------------------------------------------------------- spatial transformer (object pathway)
 * y[b,c] = grid_sample(x[b,c], affine_grid(theta[b])) bilinear, zero padding (model.py:17-21).
 * align_corners: 0 = torch>=1.3 default, 1 = torch 0.4.1 semantics.
 * bwd gathers: one thread per source pixel writes dx once, with no atomics and no zero-fill (see "Determinism" below); every
 * element of dx is written, the ones no output pixel reaches with 0.
 * MOGAN_ERR_SHAPE before any HIP call: a NULL x / dy, theta or y / dx, a dimension <= 0, B > 65535, Hin * Win or Hout * Wout
 * beyond 2^31 - 256 (the _ex forms also: xB <= 0, B % xB, theta_G < 0, B % theta_G; the gather: C > 8 * 65535). */
int mogan_stn_fwd(const float* x, const float* theta, float* y, int B, int C, int Hin, int Win, int Hout, int Wout,
                  int align_corners, hipStream_t stream);
int mogan_stn_bwd(const float* dy, const float* theta, float* dx, int B, int C, int Hin, int Win, int Hout,
                  int Wout, int align_corners, hipStream_t stream);
/* The same with a shared / constant source (round 4; the object pathways' inputs without their materialised copies):
 *   xB       x holds xB images and output sample b reads image b % xB -- `stn(image, transf_matrices[:, idx], ...)` for every
 *            object idx from ONE copy of the image batch (model.py:663-665); dx then has xB images and collects all objects;
 *   x_plane  x is (xB, C): one value per (image, channel), constant over the Hin x Win plane -- the label vector the
 *            reference first .repeat()s over 16 x 16 (model.py:109-111); dx is (xB, C);
 *   theta_G  > 0: theta is stored (B / theta_G, theta_G, 2, 3) -- the loader's (image, object) order -- while the batch is
 *            object-major, sample b = g (B / theta_G) + b' using theta[b'][g] (the batched object loops); 0: theta[b].
 * Determinism: mogan_stn_bwd / _ex gather rather than scatter: every source pixel sums the contributions of the output
 * pixels whose taps land on it, samples in batch order and output pixels in row-major order, with no atomics, so dx is the
 * same bit for bit from run to run (the shared-source forms add the objects in object order, as the reference does).
 * tests/test_kernels_gpu.py::test_stn_shared_source_gradient_is_order_independent_to_rounding pins that, and
 * tests/test_pathway_entry_points_gpu.py repeats every backward call of its table into re-poisoned memory and compares the bits. */
int mogan_stn_fwd_ex(const float* x, const float* theta, float* y, int B, int C, int Hin, int Win, int Hout, int Wout,
                     int align_corners, int xB, int x_plane, int theta_G, hipStream_t stream);
int mogan_stn_bwd_ex(const float* dy, const float* theta, float* dx, int B, int C, int Hin, int Win, int Hout, int Wout,
                     int align_corners, int xB, int x_plane, int theta_G, hipStream_t stream);
/* ---------------------------------------------------------------- channel concat with broadcast sources (round 4)
 * dst (N, C_0 + ... + C_{nsrc-1}, HW) = the sources side by side along the channel axis -- torch.cat(..., 1) of model.py:
 * 400-401, 418, 457, 633-634, 666, 703 together with the .repeat() / per-object indexing that feeds it, in ONE launch.
 * Source i (C[i] channels) is addressed as
 *     value(n, c, hw) = src[i][(n % rows[i]) * sb[i] + (n / rows[i]) * sg[i] + c * (bcast[i] ? 1 : HW) + (bcast[i] ? 0 : hw)]
 *   plain (N, C, HW) tensor:                     rows = N,     sb = C HW, sg = 0, bcast = 0
 *   (N, C) code repeated over the plane:         rows = N,     sb = C,    sg = 0, bcast = 1
 *   (N/G, C, HW) tensor repeated for G objects:  rows = N / G, sb = C HW, sg = 0
 *   label[:, g] of a (B, G, C) tensor, batch n = g B + b (object-major): rows = B, sb = G C, sg = C  (x HW when bcast = 0)
 * mogan_concat_bwd: dsrc[i] (NULL = not wanted), in the source's own layout, = the sum of ddst over everything that read it
 * (its channel slice; summed over the plane when bcast; summed over the repeats when rows < N and sg = 0).  nsrc <= MOGAN_CAT_MAX.
 * MOGAN_ERR_SHAPE before any HIP call: a NULL table, dst / ddst or src[i] (dsrc[i] alone is nullable), nsrc outside
 * 1..MOGAN_CAT_MAX, N or HW <= 0, C[i] or rows[i] <= 0, N % rows[i], and with sg[i] > 0 an sb[i] that is no positive multiple of
 * sg[i] or holds fewer than N / rows[i] objects (sb[i] / sg[i]); in the backward also a wanted dsrc[i] with sg[i] > 0 whose
 * tensor holds MORE objects than the batch reads (it is written whole, one row per batch index: N / rows[i] == sb[i] / sg[i]).
 * Every dsrc[i] NULL: returns 0 and launches nothing. */
#define MOGAN_CAT_MAX 4
int mogan_concat_fwd(const void* const* src, const int* C, const int* rows, const long long* sb, const long long* sg,
                     const int* bcast, int nsrc, float* dst, int N, int HW, hipStream_t stream);
int mogan_concat_bwd(const float* ddst, void* const* dsrc, const int* C, const int* rows, const long long* sb,
                     const long long* sg, const int* bcast, int nsrc, int N, int HW, hipStream_t stream);
/* bbox (N,4)=(x,y,w,h) -> theta (N,2,3), theta_inv (N,2,3)   (miscc/utils.py:16-49, its operation order, no contraction).
 * MOGAN_ERR_SHAPE before any HIP call: N <= 0, a NULL pointer. */
int mogan_bbox_to_theta(const float* bbox, float* theta, float* theta_inv, int N, hipStream_t stream);

/* ---------------------------------------------------------------- word attention over image regions
 * GlobalAttentionGeneral.forward core (GlobalAttention.py:96-121) after conv_context:
 * h (B,idf,Q), src (B,idf,T), mask (B,T) uint8 nullable -> wc (B,idf,Q), attn (B,T,Q).
 * mask_mode 0 = reference indexing (row b*Q+q is masked with mask[(b*Q+q) mod B]),
 *           1 = mask[b].   Limits: idf <= 128, T <= 32.
 * MOGAN_ERR_SHAPE before any HIP call (fwd and bwd): a dimension <= 0, idf > 128, T > 32, B > 65535, a NULL pointer other than
 * mask / dattn. */
int mogan_attn_fwd(const float* h, const float* src, const uint8_t* mask, float* wc, float* attn, int B, int idf,
                   int Q, int T, int mask_mode, hipStream_t stream);
/* -> dh (B,idf,Q) and dscore (B,T,Q) (gradient w.r.t. the pre-softmax scores).  dattn nullable.
 * dsrc is then two mogan_bmm calls: dsrc = h . dscore^T + dwc . attn^T. */
int mogan_attn_bwd(const float* src, const float* attn, const float* dwc, const float* dattn, float* dh,
                   float* dscore, int B, int idf, int Q, int T, hipStream_t stream);

/* ---------------------------------------------------------------- losses
 * Every entry of this section, the matching losses and the optimizer below: MOGAN_ERR_SHAPE before any HIP call for n <= 0 and
 * for a NULL pointer (none of the pointers of the BCE / KL / reparametrisation entries is nullable).  Per element against fp64,
 * in guard-banded memory: tests/test_loss_entry_points_gpu.py; the rejections: tests/test_loss_rejections_cpu.py.
 * BCE (mean) of probabilities p[n] against a constant target (nn.BCELoss with torch's log clamp at -100;
 * miscc/losses.py:158-168,198-201): loss[0] (+)= weight * mean(...); bwd: dp = gout[0]*weight/n * d/dp */
int mogan_bce_fwd(const float* p, float target, float weight, float* loss, int n, int accumulate,
                  hipStream_t stream);
int mogan_bce_bwd(const float* p, float target, float weight, const float* gout, float* dp, int n,
                  hipStream_t stream);
/* BCEWithLogits (mean) of raw logits x[n] against a constant target, torch's stable form
 * max(x,0) - x*t + log1p(exp(-|x|)) -- the StackGAN-family losses (code/coco/stackgan/miscc/utils.py:68-125,
 * code/clevr/miscc/utils.py:91-144, code/multi-mnist/miscc/utils.py:71-123).  bwd: dx = gout*w*(sigmoid(x)-t)/n */
int mogan_bce_logits_fwd(const float* x, float target, float weight, float* loss, int n, int accumulate,
                         hipStream_t stream);
int mogan_bce_logits_bwd(const float* x, float target, float weight, const float* gout, float* dx, int n,
                         hipStream_t stream);
/* KL_loss (miscc/losses.py:230-234): loss = -0.5*mean(1 + logvar - mu^2 - exp(logvar)) */
int mogan_kl_fwd(const float* mu, const float* logvar, float* loss, int n, hipStream_t stream);
int mogan_kl_bwd(const float* mu, const float* logvar, const float* gout, float* dmu, float* dlogvar, int n,
                 hipStream_t stream);

/* CA_NET.reparametrize (model.py:333-340): c = eps*exp(0.5*logvar) + mu; bwd: dmu = dc, dlogvar = dc*eps*0.5*exp(0.5*logvar) */
int mogan_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* c, int n, hipStream_t stream);
int mogan_reparam_bwd(const float* logvar, const float* eps, const float* dc, float* dmu, float* dlogvar, int n,
                      hipStream_t stream);

/* ---------------------------------------------------------------- DAMSM matching losses (generator step)
 * words_loss (miscc/losses.py:62-132 + GlobalAttention.py:31-69 func_attention, which the reference calls once per
 * caption in a python loop) for ALL (image b, caption i) pairs in one launch.
 *   ctx (B,C,S) region features, words (Bc,C,T) word embeddings, cap_lens (Bc) int32 valid words per caption.
 *   fwd -> sim (B,Bc) = gamma3 * log sum_t exp(gamma2 * cos(word_{i,t}, context_{b,i,t})), and for the backward pass
 *          a1 (B,Bc,S,T) softmax over the words, a2 (B,Bc,T,S) softmax over the regions (= the attention maps of
 *          losses.py:87-91), wc (B,C,Bc,T) weighted contexts, wt (C,Bc,T) the word embeddings in GEMM layout
 *          (nullable: not wanted); exactly zero behind each caption's end.
 *          Limits: T <= 32, (C*T + T*(S+1) + 1088) * 4 bytes of LDS <= 64 KB (1088 = 960 + 128 floats of reduction scratch:
 *          what the backward needs, and the forward is held to the same figure so that every forward has its backward but for
 *          the backward's own limit on S).  No limit on S besides: the forward's loops take any S.
 *          cap_lens[i] is clamped to [0, T]; only the valid words words[i, :, t < cap_lens[i]] enter a result (the slots behind
 *          them may hold anything, NaN included), and a1, a2, wc, wt (and dwc, dscore_t) are exactly zero at t >= cap_lens[i].
 *          A caption of length 0 has sim[b,i] = gamma3 * log(0) = -inf (for gamma3 > 0) and zeros in all its other slots.
 *   bwd: dsim (B,Bc) -> dwc (B,C,Bc,T), dscore_t (B,Bc,T,S); the region-feature gradient is then two mogan_bmm calls:
 *          dctx[b] (C,S) = dwc[b] (C, Bc*T) . a2[b] (Bc*T, S)  +  wt (C, Bc*T) . dscore_t[b] (Bc*T, S).
 *        (the image side; the text side is mogan_damsm_words_bwd_text, further down).  The backward alone has S <= 640
 *        (at most two regions per thread).
 * MOGAN_ERR_SHAPE before any HIP call (fwd and bwd): a dimension <= 0, T > 32, B > 65535, more LDS than 64 KB by the formula
 * above, a NULL pointer other than wt; in the backward also S > 640. */
int mogan_damsm_words_fwd(const float* ctx, const float* words, const int32_t* cap_lens, int B, int Bc, int C, int S, int T,
                          float gamma1, float gamma2, float gamma3, float* sim, float* a1, float* a2, float* wc, float* wt,
                          hipStream_t stream);
int mogan_damsm_words_bwd(const float* ctx, const float* words, const int32_t* cap_lens, const float* a1, const float* a2,
                          const float* wc, const float* dsim, int B, int Bc, int C, int S, int T, float gamma1,
                          float gamma2, float gamma3, float* dwc, float* dscore_t, hipStream_t stream);
/* The two cross-entropies over a square similarity matrix sim (R,R) (losses.py:45-58,116-130): rows against labels
 * (image -> caption) and columns against labels (caption -> image), entries with mask[r,q] != 0 (same class, nullable)
 * set to -inf first.  fwd -> prow, pcol (R,R) softmax probabilities, nll (2R) scratch, out2 = {loss0, loss1} (means).
 * bwd: g0, g1 (device scalars, gradients of loss0 / loss1; nullable = 0) -> dsim (R,R).
 * labels[r] is clamped to [0, R - 1] on the device, in both directions (like the token ids and the idx of
 * mogan_retrieval_rank).  A masked entry of sim is not read into any result.
 * MOGAN_ERR_SHAPE before any HIP call: R or Q <= 0, R != Q, a NULL pointer other than mask / g0 / g1. */
int mogan_damsm_ce_fwd(const float* sim, const int64_t* labels, const uint8_t* mask, int R, int Q, float* prow,
                       float* pcol, float* nll, float* out2, hipStream_t stream);
int mogan_damsm_ce_bwd(const float* prow, const float* pcol, const int64_t* labels, const float* g0, const float* g1, int R,
                       int Q, float* dsim, hipStream_t stream);
/* sent_loss similarity (losses.py:36-44): sim[b,i] = gamma3 * <cnn_b, rnn_i> / max(|cnn_b| |rnn_i|, eps); bwd -> dcnn
 * (where |cnn_b| |rnn_i| < eps: the gradient of the clamped quotient, dsim gamma3 rnn_i / eps).
 * MOGAN_ERR_SHAPE before any HIP call: B, Bc or C <= 0, a NULL pointer; in the backward also Bc > 8192 (LDS). */
int mogan_damsm_sent_fwd(const float* cnn, const float* rnn, int B, int Bc, int C, float gamma3, float eps, float* sim,
                         hipStream_t stream);
int mogan_damsm_sent_bwd(const float* cnn, const float* rnn, const float* dsim, int B, int Bc, int C, float gamma3,
                         float eps, float* dcnn, hipStream_t stream);
/* out[0] = sum_k weights[k] * in[k][0] for n <= 8 device scalars (the loss sums of losses.py:169-174,203,221 and
 * trainer.py:330 in one launch); scalar_scale is its gradient: out[k][0] = weights[k] * g[0].  `in` / `out` / `weights`
 * are HOST arrays (read during the call).
 * MOGAN_ERR_SHAPE before any HIP call: n outside 1..8, a NULL in / out / weights / g, a NULL in[k] or out[k] for k < n. */
int mogan_scalar_sum(const float* const* in, const float* weights, int n, float* out, hipStream_t stream);
int mogan_scalar_scale(const float* g, const float* weights, int n, float* const* out, hipStream_t stream);

/* ---------------------------------------------------------------- pooling / resize (CNN_ENCODER trunk)
 * max_pool2d(k,s, no padding): fwd records the offset of the first maximum of each window in idx (uint8,
 * same shape as y; nullable), bwd gathers through it (ties -> first, like torch),
 * avg_pool2d(k,s,pad, count_include_pad), bilinear resize (align_corners=0) -- model.py:256,264,271,301
 * MOGAN_ERR_SHAPE before any HIP call:
 *   mogan_maxpool_fwd(_ex): planes (B, C), k or s <= 0, H < k, W < k, k*k > 255 (idx holds a*k+b in a byte), a NULL x or y;
 *   mogan_maxpool_bwd(_ex): the same list, k > 2 s (the gather form reads at most 2 x 2 windows), a NULL idx, dy or dx
 *                           (relu_of is nullable);
 *   mogan_avgpool_fwd, mogan_avgpool_bwd(_ex): k or s <= 0 (before anything is divided), pad < 0, 2 pad > k (as torch),
 *                           planes, H or W <= 0, H + 2 pad < k, W + 2 pad < k, a NULL x / y or dy / dx (relu_of is nullable);
 *   mogan_bilinear_fwd, mogan_bilinear_bwd: planes, H, W, OH or OW <= 0, a NULL pointer. */
int mogan_maxpool_fwd(const float* x, float* y, uint8_t* idx, int planes, int H, int W, int k, int s,
                      hipStream_t stream);
int mogan_maxpool_bwd(const uint8_t* idx, const float* dy, float* dx, int planes, int H, int W, int k, int s,
                      hipStream_t stream);
int mogan_avgpool_fwd(const float* x, float* y, int planes, int H, int W, int k, int s, int pad, hipStream_t stream);
int mogan_avgpool_bwd(const float* dy, float* dx, int planes, int H, int W, int k, int s, int pad,
                      hipStream_t stream);
/* Channel-slice variants for the frozen encoder's explicit forward / backward (attngan/inception.py): y / dy are slices
 * of tensors with the given batch stride (elements; -1 = dense), the pooling gradients are added to dx when
 * accumulate != 0 after being zeroed where relu_of <= 0 (relu_of: dense, shaped like dx; nullable) -- the ReLU backward
 * of the layer that produced the pooled tensor. */
int mogan_maxpool_fwd_ex(const float* x, float* y, long long y_bstride, uint8_t* idx, int B, int C, int H, int W, int k,
                         int s, hipStream_t stream);
int mogan_maxpool_bwd_ex(const uint8_t* idx, const float* dy, long long dy_bstride, float* dx, const float* relu_of,
                         int accumulate, int B, int C, int H, int W, int k, int s, hipStream_t stream);
int mogan_avgpool_bwd_ex(const float* dy, float* dx, const float* relu_of, int accumulate, int planes, int H, int W, int k,
                         int s, int pad, hipStream_t stream);
/* dx (+)= dz where z > 0 (z: the ReLU's output).  MOGAN_ERR_SHAPE before any HIP call: n <= 0, a NULL pointer. */
int mogan_relu_bwd(const float* z, const float* dz, float* dx, long long n, int accumulate, hipStream_t stream);
/* B rows of n contiguous floats between two batch-strided tensors.  MOGAN_ERR_SHAPE before any HIP call: B or n <= 0,
 * a NULL src or dst. */
int mogan_copy_strided(const float* src, long long src_bstride, float* dst, long long dst_bstride, int B, long long n,
                       hipStream_t stream);
int mogan_bilinear_fwd(const float* x, float* y, int planes, int H, int W, int OH, int OW, hipStream_t stream);
int mogan_bilinear_bwd(const float* dy, float* dx, int planes, int H, int W, int OH, int OW, hipStream_t stream);

/* ---------------------------------------------------------------- input pipeline (device side)
 * datasets.py:70-137 (get_imgs / crop_imgs) after the JPEG decode + resize to `ori` x `ori` (268): the host uploads u8
 * HWC images and the (column offset h1, row offset w1, flip) it drew per sample.
 * crop_flip: src (B,ori,ori,3) u8, params (B,3) int32 -> q (B,size,size,3) u8 (the crop, = ToPILImage of it) and
 *            out (B,3,size,size) f32 = ((u8/255) - 0.5) / 0.5 (ToTensor + Normalize).
 * resample:  Pillow's antialiased BILINEAR resize of the square u8 image `in` (B,S,S,3) to OS x OS (transforms.Resize),
 *            then ToTensor + Normalize -> out (B,3,OS,OS) f32.  bounds (OS,2) / kk (OS,ksize): Pillow's coefficient
 *            tables (precompute_coeffs + normalize_coeffs_8bpc, 22-bit fixed point; the same table serves both passes of
 *            a square resize), built by the host (attngan/feeder.py); tmp (B,S,OS,3) u8 scratch.  Bit-identical to PIL.
 * MOGAN_ERR_SHAPE before any HIP call: crop_flip: B or size <= 0, ori < size, a NULL src, params, q or out;
 *            resample: B, S, OS or ksize <= 0, a NULL in, tmp, out, bounds or kk.
 * The crop offsets live on the device and cannot be checked by the host: 0 <= h1, w1 <= ori - size is the caller's
 * contract (attngan/feeder.draw_crop keeps it). */
int mogan_feed_crop_flip(const uint8_t* src, const int32_t* params, uint8_t* q, float* out, int B, int ori, int size,
                         hipStream_t stream);
int mogan_feed_resample(const uint8_t* in, uint8_t* tmp, float* out, const int32_t* bounds, const int32_t* kk, int ksize,
                        int B, int S, int OS, hipStream_t stream);

/* ---------------------------------------------------------------- optimizer
 * One fused Adam step over a flat fp32 bucket (trainer.py:137-148: lr 2e-4, betas (0.5,0.999), eps 1e-8),
 * optionally followed by the EMA of trainer.py:341-342: ema = ema_decay*ema + (1-ema_decay)*p (ema nullable).
 * `step` is the 1-based step count; if dev_state (3 floats on the device, zero-initialised) is given it
 * replaces `step`: the count lives in dev_state[0] and is incremented on the device, so the call can be
 * captured in a hipGraph and replayed.  eps_mode 0: denom = sqrt(v)/sqrt(1-b2^t) + eps (torch>=1.x);
 * 1: denom = sqrt(v) + eps with step size lr*sqrt(1-b2^t)/(1-b1^t) (torch 0.4.1).  grad_scale multiplies g
 * first (1/world_size after an RCCL sum all-reduce).  n need not be a multiple of 4: nothing behind element n - 1 is touched.
 * MOGAN_ERR_SHAPE before any HIP call -- so a rejected call leaves dev_state[0] where it was --: n <= 0, step < 1 without
 * dev_state, a NULL p / g / m / v, a p / g / m / v / ema that is not 16-byte aligned (ema and dev_state are nullable). */
int mogan_adam_step(float* p, const float* g, float* m, float* v, float* ema, long long n, float lr, float beta1,
                    float beta2, float eps, int step, float* dev_state, int eps_mode, float grad_scale,
                    float ema_decay, hipStream_t stream);
/* The same step in two parts, for a bucket that is updated by several launches (its deep convolution weights by
 * mogan_pk_adam_pack_both, the ranges between them here): mogan_adam_prep advances the device-resident count once and leaves
 * step size and bias correction in dev_state; mogan_adam_apply is mogan_adam_step's element pass over one range, reading them.
 * MOGAN_ERR_SHAPE before any launch: a NULL dev_state; for mogan_adam_apply also what mogan_adam_step rejects. */
int mogan_adam_prep(float* dev_state, float lr, float beta1, float beta2, int eps_mode, hipStream_t stream);
int mogan_adam_apply(float* p, const float* g, float* m, float* v, float* ema, long long n, float beta1, float beta2, float eps,
                     const float* dev_state, int eps_mode, float grad_scale, float ema_decay, hipStream_t stream);

/* ---- text encoder (round 6, third session; csrc/mogan_rnn.hip): nn.Embedding + one-layer bidirectional nn.LSTM over packed
 * captions in eval mode, without gradients -- RNN_ENCODER.forward, code/coco/attngan/model.py:183-204 (pack_padded_sequence,
 * self.rnn, pad_packed_sequence, the transposes) -- as ONE launch instead of the 119 of the stock module (MIOpen).
 *   captions (B, T) int64 token ids (clamped to [0, V)), lens[B] on the HOST (sorted or not; 0 <= lens[i] <= Tmax <= T, Tmax <= 32),
 *   emb (V, E) (E % 4 == 0, E <= 320), per direction d = 0 forward / 1 reverse: w_ih[d] (4H, E), w_hh[d] (4H, H), b_ih[d], b_hh[d]
 *   (4H) in PyTorch's gate order i, f, g, o (16-byte aligned weights), H = 128, B <= 64; h0 / c0 (2, B, H) or NULL (zeros);
 *   words (B, 2H, Tmax): the hidden states, zero for t >= lens[b]; sent (B, 2H): the final states (forward | reverse). */
int mogan_lstm_encoder_fwd(const long long* captions, const int* lens, const float* emb, const float* const* w_ih,
                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                           const float* c0, float* words, float* sent, int B, int T, int Tmax, int V, int E, int H,
                           hipStream_t stream);

/* ---- DAMSM pre-training (attngan/pretrain_DAMSM.py): the text encoder under training, and the text side of the matching losses.
 * mogan_lstm_encoder_train_fwd: the forward above with embedding dropout and the tensors the backward needs.  Same arguments and
 * limits, plus
 *   keep_mask (B, T, E) uint8 or NULL (keep everything), scale: the embedded row is multiplied by scale where the mask is 1 and by
 *   0 where it is 0 (nn.Dropout: scale = 1 / (1 - p); the mask is drawn by the host side),
 *   x (B, Tmax, E): the masked, scaled embedding rows (the GEMM operand of dW_ih), gates (2, B, Tmax, 4H): the post-activation
 *   gates i, f, g, o, cells (2, B, Tmax, H): c_t, hprev (2, B, Tmax, H): the hidden state that ENTERED step t in walk order (the
 *   reverse direction's "previous" step is t + 1).  All four are written everywhere, zero at t >= lens[b].
 * mogan_lstm_encoder_bwd: back-propagation through time, one block per (direction, caption).
 *   dwords (B, 2H, Tmax), dsent (B, 2H) (either nullable = 0), gates / cells / hprev as saved, c0 as in the forward (nullable),
 *   w_hh[d] -> dgates (2, B, Tmax, 4H): the gradients of the PRE-activation gates, exactly zero at t >= lens[b], and
 *   dbias (2, 4H) (nullable): their sums over (b, t) = d b_ih = d b_hh, summed in index order.  h0 / c0 get no gradient.
 *   The weight gradients are GEMMs over the dense (B * Tmax) axis (mogan_bmm): dW_ih[d] = dgates[d]^T . x,
 *   dW_hh[d] = dgates[d]^T . hprev[d], dx = sum_d dgates[d] . W_ih[d].
 * mogan_embedding_bwd: demb[tok] += sum over the positions (b, t < lens[b]) that hold tok of (mask ? scale : 0) * dx[b, t, :].
 *   Deterministic and free of atomics: the first position that holds a token owns its row and adds the later positions in index
 *   order.  demb (V, E) is accumulated into (the optimizer's gradient bucket); rows of absent tokens are not touched. */
int mogan_lstm_encoder_train_fwd(const long long* captions, const int* lens, const float* emb, const float* const* w_ih,
                                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                 const float* c0, const uint8_t* keep_mask, float scale, float* words, float* sent, float* x,
                                 float* gates, float* cells, float* hprev, int B, int T, int Tmax, int V, int E, int H,
                                 hipStream_t stream);
int mogan_lstm_encoder_bwd(const float* dwords, const float* dsent, const int* lens, const float* gates, const float* cells,
                           const float* hprev, const float* c0, const float* const* w_hh, float* dgates, float* dbias, int B,
                           int Tmax, int H, hipStream_t stream);
int mogan_embedding_bwd(const long long* captions, const int* lens, const float* dx, const uint8_t* keep_mask, float scale,
                        float* demb, int B, int T, int Tmax, int V, int E, hipStream_t stream);

/* ---- text encoder with cfg.RNN_TYPE = 'GRU' (csrc/mogan_rnn.hip): nn.Embedding + one-layer bidirectional nn.GRU over packed
 * captions, the three LSTM entries above restated for PyTorch's GRU (gate order r, z, n):
 *   r = s(W_ir x + b_ir + W_hr h + b_hr), z = s(W_iz x + b_iz + W_hz h + b_hz), hn = W_hn h + b_hn,
 *   n = tanh(W_in x + b_in + r * hn), h' = (1 - z) * n + z * h.
 * mogan_gru_encoder_fwd: eval mode, no gradients, ONE launch.  Arguments and limits as mogan_lstm_encoder_fwd:
 *   captions (B, T) int64 token ids (clamped to [0, V)), lens[B] on the HOST (0 <= lens[i] <= Tmax <= T, Tmax <= 32), emb (V, E)
 *   (E % 4 == 0, E <= 320), per direction d = 0 forward / 1 reverse: w_ih[d] (3H, E), w_hh[d] (3H, H), b_ih[d], b_hh[d] (3H)
 *   (16-byte aligned weights), H = 128, B <= 64; h0 (2, B, H) or NULL (zeros); words (B, 2H, Tmax): the hidden states, zero for
 *   t >= lens[b]; sent (B, 2H): the final states (forward | reverse); a caption of length 0 gives a zero row and sent = h0.
 * mogan_gru_encoder_train_fwd: the same with embedding dropout (keep_mask (B, T, E) uint8 or NULL, scale, as in the LSTM entry) and
 *   the tensors the backward needs: x (B, Tmax, E): the masked, scaled embedding rows, gates (2, B, Tmax, 3H): the post-activation
 *   r, z, n, hn (2, B, Tmax, H), hprev (2, B, Tmax, H): the hidden state that ENTERED step t in walk order.  All four are written
 *   everywhere, zero at t >= lens[b].
 * mogan_gru_encoder_bwd: back-propagation through time, one block per (direction, caption).
 *   dwords (B, 2H, Tmax), dsent (B, 2H) (either nullable = 0), gates / hn / hprev as saved, w_hh[d] ->
 *   dgi (2, B, Tmax, 3H) = (dr, dz, dn): the gradients of the input-side pre-activations, dgh (2, B, Tmax, 3H) = (dr, dz, dn * r):
 *   those of the hidden side (b_hn and W_hn sit inside r * (...)); both exactly zero at t >= lens[b];
 *   dbias_ih, dbias_hh (2, 3H) (each nullable): their sums over (b, t) in index order -- d b_ih != d b_hh in the n block.
 *   h0 gets no gradient.  The weight gradients are GEMMs over the dense (B * Tmax) axis (mogan_bmm): dW_ih[d] = dgi[d]^T . x,
 *   dW_hh[d] = dgh[d]^T . hprev[d], dx = sum_d dgi[d] . W_ih[d]; the table's gradient is mogan_embedding_bwd.
 * An out-of-range argument or a NULL required pointer returns MOGAN_ERR_SHAPE and nothing is written. */
int mogan_gru_encoder_fwd(const long long* captions, const int* lens, const float* emb, const float* const* w_ih,
                          const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                          float* words, float* sent, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream);
int mogan_gru_encoder_train_fwd(const long long* captions, const int* lens, const float* emb, const float* const* w_ih,
                                const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, const float* h0,
                                const uint8_t* keep_mask, float scale, float* words, float* sent, float* x, float* gates, float* hn,
                                float* hprev, int B, int T, int Tmax, int V, int E, int H, hipStream_t stream);
int mogan_gru_encoder_bwd(const float* dwords, const float* dsent, const int* lens, const float* gates, const float* hn,
                          const float* hprev, const float* const* w_hh, float* dgi, float* dgh, float* dbias_ih, float* dbias_hh,
                          int B, int Tmax, int H, hipStream_t stream);

/* The text side of mogan_damsm_words_bwd / mogan_damsm_sent_bwd (same clamp rules).
 * words: dwords (Bc,C,T) = sum_b of the gradient of pair (b,i)'s cosines with respect to the word itself,
 *          k1[t] * wc[b,:,i,t] + k3[t] * w[i,:,t],  k1 = dcos / max(den, 1e-8),  k3 = -dcos * cos / |w|^2,
 *        summed over b in index order, exactly zero at t >= cap_lens[i].  The path through the attention scores is added by the
 *        caller, one mogan_bmm per image b over the caption axis: dwords[i] (C,T) += ctx[b] (C,S) . dscore_t[b,i] (T,S)^T.
 * sent:  drnn[i] = sum_b dsim[b,i] * gamma3 * (cnn_b / den - cos * rnn_i / |rnn_i|^2). */
int mogan_damsm_words_bwd_text(const float* words, const int32_t* cap_lens, const float* wc, const float* dsim, int B, int Bc,
                               int C, int T, float gamma2, float gamma3, float* dwords, hipStream_t stream);
int mogan_damsm_sent_bwd_text(const float* cnn, const float* rnn, const float* dsim, int B, int Bc, int C, float gamma3,
                              float eps, float* drnn, hipStream_t stream);

/* R-precision ranking (the AttnGAN paper's text-image metric; the reference has no code for it -- DESIGN.md section 9c).
 * Query q = image code code[q] (C floats).  Candidate 0 = pos[q] (its caption's sentence code), candidates 1..Rn = rows
 * idx[q, r-1] of bank (N, C).
 *   score[q, r] = <code_q, cand_r> / max(|code_q| * |cand_r|, eps)          (miscc/losses.py cosine_similarity)
 *   rank[q]     = number of r in 1..Rn with score[q, r] > score[q, 0]       (0 = retrieved first; a tie counts for the match,
 *                                                                            as argmax's first index does)
 * One launch, one block per query; fp32 fmaf chains over lane-strided channels; every candidate, pos included, runs through the
 * same instruction sequence, so equal candidate bits give equal score bits, and the same inputs give the same bits on every call.
 * idx entries are clamped to [0, N-1] (as the caption kernels clamp token ids).  score (Q, Rn+1) is nullable; rank (Q) int32.
 * MOGAN_ERR_SHAPE before any HIP call: Q, Rn, C or N <= 0, Rn > 1023, N > 2^31-1, a NULL code / pos / bank / idx / rank. */
int mogan_retrieval_rank(const float* code, const float* pos, const float* bank, const int32_t* idx, int Q, int Rn, int C,
                         long long N, float eps, float* score, int32_t* rank, hipStream_t stream);

/* fp64 moments of a set of feature codes: what the Frechet distance is computed from (the reference has no code for it --
 * DESIGN.md section 9d; csrc/mogan_stats.hip).  x is fp32 (N, D), dense, widened exactly; mean (D) and cov (D, D) are fp64 -- with
 * the sums of mogan_poly3_mmd_f64, the radii of mogan_knn_sqdist_f64, the distances of mogan_knn_cross_f64, the moments and sums of mogan_swd_*, the terms of mogan_ssim_level_f64 and the twiddle table and sums of mogan_radial_power_f64 below the only fp64 tensors of this ABI.  No workspace, no atomics, nothing handed from
 * workgroup to workgroup: every sum over n runs in one fixed order, so the same inputs give the same bits on every call.
 *   mean[j]   = (sum_n (double)x[n][j]) / N
 *   cov[i][j] = (sum_n (x[n][i] - mean[i]) (x[n][j] - mean[j])) / (N - 1)       (numpy.cov(x, rowvar=False))
 * mogan_cov_f64 centres in fp64 with the caller's mean (mogan_col_mean_f64's, for the covariance), forms products and sums on
 * v_mfma_f64_16x16x4_f64 for the 64 x 64 tiles on and above the diagonal, ends with a true division by N - 1 and writes every
 * element and its mirror image from one register: cov[i][j] and cov[j][i] have the same bits.  Rows past N and columns past D enter
 * the last tiles as zeros and are never stored.
 * Limits of the index arithmetic: N <= 2^31 - 1, D <= 65536 (x is indexed in 64 bits; the covariance grid holds
 * ceil(D / 64) (ceil(D / 64) + 1) / 2 <= 524 800 blocks).
 * MOGAN_ERR_SHAPE before any HIP call: a NULL x / mean / cov, D < 1, D > 65536, N > 2^31 - 1, N < 1 (mean) or N < 2 (cov). */
int mogan_col_mean_f64(const float* x, long long N, int D, double* mean, hipStream_t stream);
int mogan_cov_f64(const float* x, const double* mean, long long N, int D, double* cov, hipStream_t stream);

/* The sums of the kernel Inception distance (csrc/mogan_mmd.hip; the reference has no code for it): for S
 * subset pairs of s rows of x (Nx, D) and s rows of y (Ny, D), fp32, dense, widened exactly, gathered through the int32 tables
 * ix (S, s) and iy (S, s), under k(a, b) = (gamma <a, b> + coef0)^3:
 *   sums[k][0] = sum_{i != j} k(x_ix[k][i], x_ix[k][j])       ordered pairs, i != j by POSITION in the subset
 *   sums[k][1] = sum_{i != j} k(y_iy[k][i], y_iy[k][j])
 *   sums[k][2] = sum_{i, j}   k(x_ix[k][i], y_iy[k][j])
 * sums (S, 3) is fp64.  Products and sums over the features run on v_mfma_f64_16x16x4_f64 in index order, one 64 x 64 tile of one
 * subset's kernel matrix per workgroup (for xx / yy only the tiles on and above the diagonal, doubled; a diagonal tile keeps
 * i < j); t = acc * gamma + coef0, value (t * t) * t, no pow, no contraction.  No kernel matrix is ever written: a workgroup
 * reduces its tile in a fixed order to ONE double in ws[subset][tile] and a second launch of the same call adds a subset's tile
 * partials in tile order.  No atomics: the same inputs give the same bits on every call, and a subset's sums do not depend on
 * which other subsets share the call.  Index entries outside [0, N) are clamped to [0, N - 1] (as mogan_retrieval_rank does).
 * The workspace is required: mogan_poly3_mmd_ws_bytes(S, s) = S * (2 T^2 + T) * 8 bytes, T = ceil(s / 64), 8-byte aligned (0 for an
 * S or s the call rejects); MOGAN_ERR_WS where ws is NULL, misaligned or shorter, nothing launched.
 * MOGAN_ERR_SHAPE before any HIP call (and before the workspace is looked at): a NULL x / y / ix / iy / sums, S < 1, S > 65535 (the
 * grid), s < 2, s > 2^20, D < 1, D > 65536, Nx or Ny < 1 or > 2^31 - 1, a non-finite gamma or coef0. */
size_t mogan_poly3_mmd_ws_bytes(int S, int s);
int mogan_poly3_mmd_f64(const float* x, long long Nx, const float* y, long long Ny, int D, const int32_t* ix, const int32_t* iy,
                        int S, int s, double gamma, double coef0, double* sums, void* ws, size_t ws_bytes, hipStream_t stream);

/* Nearest-neighbour radii and ball membership for precision / recall and density / coverage (DESIGN.md section 9f;
 * csrc/mogan_knn.hip; the reference has no code for it), on squared Euclidean distances of fp32 rows, dense, widened exactly:
 *   d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0)                                  everything after the load in fp64
 * <a, b> on v_mfma_f64_16x16x4_f64 in 64 x 64 tiles, K steps along the features in index order; the row norms are the diagonal of
 * the same tile loop run on a 64-row group against itself (one small launch per set, into the workspace).  A distance's bits
 * therefore depend on the two rows only -- not on the tile, the wave or which operand a row is: a bit copy of a row is at exactly 0,
 * d2(i, j) = d2(j, i) bitwise, and a permutation of the rows permutes the results bitwise.  No distance matrix is written, there
 * are no atomics, and the same inputs give the same bits on every call.
 * mogan_knn_sqdist_f64: out (N, K) fp64, row i = the K smallest d2(x_i, x_j) over j != i, ascending; j != i by POSITION (a duplicate
 *   of row i elsewhere is a neighbour at distance 0).  1 <= K <= 8, N >= K + 1.
 * mogan_ball_count_f64: count (M, R) int32, count[j][c] = #{ i : d2(q_j, p_i) <= r2[.][c] } for queries q (M, D) and support points
 *   p (N, D); side 0: the radius is the support point's, r2 (N, R) indexed by i; side 1: the query's, r2 (M, R) indexed by j.
 *   1 <= R <= 4; <= includes equality; a NaN radius counts nothing.
 * A workgroup owns a stripe of 64 rows / queries and walks the column / support tiles; where the stripes alone would not fill the
 * device the tiles are split into `shares` = min(ceil(512 / Tr), Tc, 64) parts (Tr, Tc = ceil(rows / 64), ceil(columns / 64)), each
 * leaving its K smallest / its counts in the workspace, merged by a last launch of the same call (the K smallest of a multiset and a
 * sum of integers do not depend on the partition).  The workspace is required, 8-byte aligned:
 *   mogan_knn_sqdist_ws_bytes(N, K)    = 8 (N + shares N K)
 *   mogan_ball_count_ws_bytes(M, N, R) = 8 (M + N) + 4 shares M R rounded up to 8            (0 for arguments the call rejects)
 * MOGAN_ERR_WS where ws is NULL, misaligned or shorter, nothing launched.  MOGAN_ERR_SHAPE before any HIP call (and before the
 * workspace is looked at): a NULL x / out / q / p / r2 / count, K < 1, K > 8, N < K + 1, R < 1, R > 4, M < 1, N < 1, M or N >
 * 2^31 - 1, D < 1, D > 65536, a side other than 0 / 1. */
size_t mogan_knn_sqdist_ws_bytes(long long N, int K);
int mogan_knn_sqdist_f64(const float* x, long long N, int D, int K, double* out, void* ws, size_t ws_bytes, hipStream_t stream);
size_t mogan_ball_count_ws_bytes(long long M, long long N, int R);
int mogan_ball_count_f64(const float* q, long long M, const float* p, long long N, int D, const double* r2, int R, int side,
                         int32_t* count, void* ws, size_t ws_bytes, hipStream_t stream);

/* Nearest neighbours BETWEEN two sets, with their positions: what the memorisation figures of DESIGN.md section 9j are computed
 * from (csrc/mogan_knn.hip; the reference has no code for it).  For every query row q_j of q (M, D), d2 (M, K) fp64 and idx (M, K)
 * int32 hold the K smallest d2(q_j, p_i) over all rows i of p (N, D), ascending, and the positions i.  The distances are the ones
 * above -- the same tile loop, the same row norms, the same one expression -- so their bits depend on the two rows only, a bit copy
 * is at exactly 0, and they equal what mogan_knn_sqdist_f64 and mogan_ball_count_f64 form for the same two rows.  Where two
 * distances are equal bit for bit the lower position comes first: the order is the lexicographic order of (d2, i), a total order,
 * so the result does not depend on how the support tiles are split into shares.  1 <= K <= 8, N >= K.  A NaN distance (non-finite
 * inputs) is never a neighbour; a query that has fewer than K others keeps d2 = +inf, idx = 2^31 - 1 in the slots left over.
 * A workgroup owns a stripe of 64 queries and walks the support tiles of its share, `shares` = min(ceil(512 / Tr), Tc, 64) as above
 * with Tr = ceil(M / 64), Tc = ceil(N / 64); one thread per query keeps the 8 first pairs in registers; a last launch of the same
 * call merges the shares' lists per query under the same order.  No distance matrix is written, there are no atomics, and the same
 * inputs give the same bits on every call.  The workspace is required, 8-byte aligned:
 *   mogan_knn_cross_ws_bytes(M, N, K) = 8 (M + N + shares M K) + 4 shares M K rounded up to 8     (0 for arguments the call rejects)
 * MOGAN_ERR_WS where ws is NULL, misaligned or shorter, nothing launched.  MOGAN_ERR_SHAPE before any HIP call (and before the
 * workspace is looked at): a NULL q / p / d2 / idx, K < 1, K > 8, N < K, M < 1, M or N > 2^31 - 1, D < 1, D > 65536. */
size_t mogan_knn_cross_ws_bytes(long long M, long long N, int K);
int mogan_knn_cross_f64(const float* q, long long M, const float* p, long long N, int D, int K, double* d2, int32_t* idx, void* ws,
                        size_t ws_bytes, hipStream_t stream);

/* mogan_knn_cross_f64 with a label per row: what object accuracy by nearest labelled training crops is computed from (DESIGN.md
 * section 9m; csrc/mogan_knn.hip, the same two kernels under a template flag; the reference has no code for it).  qlabel (M) and
 * plabel (N) are int32, arbitrary: a negative label has no special meaning.
 *   d2, idx (M, K)          exactly mogan_knn_cross_f64's for the same q, p, K, bit for bit; the labels play no part in them
 *   same_d2, same_idx (M)   the first pair (d2(q_j, p_i), i) under the order above (distance, equal bits by position) among the
 *                           rows with plabel[i] == qlabel[j]
 *   other_d2, other_idx (M) the same among the rows with plabel[i] != qlabel[j]
 * The distances are the ones above (a bit copy is at exactly 0).  An empty set -- a query label the bank does not hold, a bank that
 * is all of the query's label -- gives +inf and 2^31 - 1; a NaN distance is never listed.  The order is total, so no result depends
 * on how the support tiles are split into shares; no atomics, no distance matrix, the same bits on every call.  1 <= K <= 8, N >= K.
 * The workspace is required, 8-byte aligned: mogan_knn_cross_f64's followed by the shares' two pairs per query,
 *   mogan_knn_label_ws_bytes(M, N, K) = mogan_knn_cross_ws_bytes(M, N, K) + 24 shares M             (0 for arguments the call rejects)
 * MOGAN_ERR_WS where ws is NULL, misaligned or shorter, nothing launched.  MOGAN_ERR_SHAPE before any HIP call (and before the
 * workspace is looked at): a NULL q / qlabel / p / plabel / d2 / idx / same_d2 / same_idx / other_d2 / other_idx, K < 1, K > 8,
 * N < K, M < 1, M or N > 2^31 - 1, D < 1, D > 65536. */
size_t mogan_knn_label_ws_bytes(long long M, long long N, int K);
int mogan_knn_label_f64(const float* q, const int32_t* qlabel, long long M, const float* p, const int32_t* plabel, long long N, int D,
                        int K, double* d2, int32_t* idx, double* same_d2, int32_t* same_idx, double* other_d2, int32_t* other_idx,
                        void* ws, size_t ws_bytes, hipStream_t stream);

/* The sliced Wasserstein distance of Karras et al. 2018 between real and generated images (DESIGN.md section 9g;
 * csrc/mogan_swd.hip; the reference has no code for it): Laplacian pyramid, 7 x 7 descriptors, their moments, their projections
 * and the sum of |a - b| per direction; the sort in between is the caller's.  All images and descriptors are fp32 and dense.  No
 * atomics, every sum runs in one fixed order: the same inputs give the same bits on every call.
 *   w = (1, 4, 6, 4, 1) / 16; mirrored index m(i, n) = -i for i < 0, 2 n - 2 - i for i >= n (the edge sample is not repeated).
 * mogan_pyr_down: x (NC, H, W) -> out (NC, H / 2, W / 2), out[oy][ox] = sum_{dy, dx = -2..2} w[dy] w[dx] x[m(2 oy + dy, H)][m(2 ox + dx, W)].
 * mogan_lap_residual: out = x - pyr_up(down) in one launch, x and out (NC, H, W), down (NC, H / 2, W / 2); pyr_up is the same
 *   filter times 4 over the zero-inserted image z (z[2 y][2 x] = down[y][x]) under the same mirror rule on z's indices -- a
 *   mirrored index on an odd row or column contributes zero.  out may alias neither x nor down.
 *   Both: H and W even and >= 4 (they need not be equal), NC >= 1, NC H W <= 2^31 - 1.
 * mogan_swd_gather: level (N, C, H, W); centres (R, 3) int32 = (image, cy, cx) per descriptor; writes rows [row0, row0 + R) of
 *   desc (rows_total, 49 C), a row = the 7 x 7 neighbourhood of (cy, cx) over all channels in (channel, y, x) order.  A copy.  The
 *   caller keeps cy in [3, H - 3) and cx in [3, W - 3); what lies outside is clamped into the level (image to [0, N)).
 *   1 <= C <= 4, H and W >= 7, N C H W <= 2^31 - 1, R >= 1, row0 >= 0, row0 + R <= rows_total <= 2^31 - 1.
 * mogan_swd_moments_f64: desc (rows, 49 C) -> moments (C, 2) fp64 = (mean, population standard deviation) per channel over all rows
 *   and the 49 positions of that channel; two passes (sum x; sum (x - mean)^2) over P = min(ceil(rows / 64), 2048) contiguous
 *   shares of the rows, the shares added in share order.  A constant channel has a standard deviation of exactly 0.  The workspace
 *   is required, 8-byte aligned: mogan_swd_moments_ws_bytes(rows, C) = 8 P C (0 for arguments the call rejects); MOGAN_ERR_WS where
 *   ws is NULL, misaligned or shorter, nothing launched.
 * mogan_swd_project: desc (rows, K = 49 C), moments (C, 2) fp64, dirs (K, D) -> out (D, rows):
 *   out[d][r] = sum_k z[r][k] dirs[k][d], z = (float)(((double)desc[r][k] - mean_c) / std_c), the product on the matrix pipe
 *   (csrc/mogan_mma.h), every 16 values of k into an fp32 accumulator of their own, the groups added in fp64 in index order and
 *   rounded to fp32 once; a result's bits depend on its row and direction only.
 *   1 <= D <= 1024.
 * mogan_swd_absdiff_f64: a, b (D, rows) -> out (D) fp64, out[d] = sum_r |(double)a[d][r] - (double)b[d][r]|.  1 <= D <= 1024.
 * MOGAN_ERR_SHAPE before any HIP call (and before the workspace is looked at): a NULL pointer (ws apart), any dimension outside the
 * ranges above, rows < 1 or > 2^31 - 1, C outside 1..4. */
int mogan_pyr_down(const float* x, long long NC, int H, int W, float* out, hipStream_t stream);
int mogan_lap_residual(const float* x, const float* down, long long NC, int H, int W, float* out, hipStream_t stream);
int mogan_swd_gather(const float* level, int N, int C, int H, int W, const int32_t* centres, long long R, float* desc,
                     long long row0, long long rows_total, hipStream_t stream);
size_t mogan_swd_moments_ws_bytes(long long rows, int C);
int mogan_swd_moments_f64(const float* desc, long long rows, int C, double* moments, void* ws, size_t ws_bytes,
                          hipStream_t stream);
int mogan_swd_project(const float* desc, long long rows, int C, const double* moments, const float* dirs, int D, float* out,
                      hipStream_t stream);
int mogan_swd_absdiff_f64(const float* a, const float* b, long long rows, int D, double* out, hipStream_t stream);

/* One level of the multi-scale structural similarity of pairs of images (Wang et al. 2003, as Odena et al. 2017 use it for GAN
 * diversity; csrc/mogan_ssim.hip; attngan/msssim.py has the whole definition; the reference has no code for
 * it).  All images are fp32 and dense.  No atomics, every sum runs in one fixed order: the same inputs give the same bits on every
 * call.
 * mogan_avg_down2: x (NC, H, W) -> out (NC, H / 2, W / 2), the aligned 2 x 2 mean
 *   out[y][x] = ((x[2y][2x] + x[2y][2x + 1]) + (x[2y + 1][2x] + x[2y + 1][2x + 1])) * 0.25f.
 *   H and W even and >= 2 (they need not be equal), NC >= 1, NC H W <= 2^31 - 1.
 * mogan_ssim_level_f64: a, b (P, C, S, S) = P pairs; win (n) the separable window, fp32, on the device; M = S - n + 1 valid
 *   positions per axis.  Per channel, in fp32 without contraction, on the centred values d = 127.5f x, with G* the window applied
 *   along x first and then along y, both sums from zero in index order:
 *     m_a = G*d_a, m_b = G*d_b, s_aa = G*(d_a d_a) - m_a m_a, s_bb = G*(d_b d_b) - m_b m_b, s_ab = G*(d_a d_b) - m_a m_b,
 *     mu_a = 127.5f + m_a, mu_b = 127.5f + m_b, C1 = 6.5025f, C2 = 58.5225f,
 *     cs   = (2 s_ab + C2) / ((s_aa + s_bb) + C2)
 *     l    = (2 (mu_a mu_b) + C1) / ((mu_a mu_a + mu_b mu_b) + C1)
 *     ssim = l cs                                  (IEEE division)
 *   so a pair of bit-identical images gives ssim = cs = 1.0f at every position, and exchanging a and b leaves every bit as it is.
 *   terms (P, 2) fp64 = (mean ssim, mean cs) over the C M M values of a pair: a workgroup owns a 32 x 32 tile of positions of one
 *   channel of one pair, stages the tile and its n - 1 halo of both images in LDS, filters along x into LDS and along y in
 *   registers (the five filtered planes never reach memory), adds its values in fp64 in a fixed tree and leaves two doubles in the
 *   workspace; a second launch of the same call adds a pair's C T T partials (T = ceil(M / 32)) in index order and divides by
 *   C M M.  ssim_map and cs_map, (P, C, M, M) fp32, are written where they are not NULL.  The workspace is required, 8-byte
 *   aligned: mogan_ssim_level_ws_bytes(P, C, S, n) = 16 P C T T (0 for arguments the call rejects); MOGAN_ERR_WS where ws is NULL,
 *   misaligned or shorter, nothing launched.
 *   P >= 1, 1 <= C <= 4, S >= 2, 1 <= n <= min(11, S), P C S S <= 2^31 - 1.
 * MOGAN_ERR_SHAPE before any HIP call (and before the workspace is looked at): a NULL pointer (the maps and ws apart), any
 * dimension outside the ranges above. */
int mogan_avg_down2(const float* x, long long NC, int H, int W, float* out, hipStream_t stream);
size_t mogan_ssim_level_ws_bytes(long long P, int C, int S, int n);
int mogan_ssim_level_f64(const float* a, const float* b, long long P, int C, int S, const float* win, int n, double* terms,
                         float* ssim_map, float* cs_map, void* ws, size_t ws_bytes, hipStream_t stream);

/* Crop, compaction and resize of a ragged list of boxes in one launch: what the object-level Frechet distance feeds the trunk
 * (SceneFID, Sylvain et al. 2021; csrc/mogan_roi.hip; attngan/scenefid.py has the score's definition; the
 * reference has no code for it).  x (B, C, H, W) fp32; boxes (R, 4) fp32, relative (x, y, w, h), the data set's convention;
 * image_index (R) int32; y (R, C, OH, OW) fp32; all dense and on the device.  ROI r is box r of image image_index[r].
 * Per axis (x shown; y alike with H, OH, box[1], box[3]), fp32 with ONE rounding per operation in this order, never contracted:
 *     p0 = box.x * W                 pl = box.w * W                 scale = pl / OW
 *     src(j) = p0 + (((float)j + 0.5f) * scale - 0.5f)     then clamped to [0, W - 1]
 *     i0 = floor(src)    i1 = min(i0 + 1, W - 1)    l = src - (float)i0
 *   y[r][c][oy][ox] = (1 - ly) * ((1 - lx) * x[y0][x0] + lx * x[y0][x1]) + ly * ((1 - lx) * x[y1][x0] + lx * x[y1][x1])
 * on channel c of image image_index[r] (the blend may be contracted; this build does not).  The clamp repeats the edge pixel: what
 * a box reaches past the image, and the half pixel around a box at the edge, is the edge's value, not zero.  The full box
 * (0, 0, 1, 1) is bilinear interpolation with align_corners = False.
 * Safe by construction: a ROI with w <= 0 or h <= 0 (the data set's absent object is (-1, -1, -1, -1)), with a box value that is
 * not finite, or with image_index outside [0, B) reads nothing of x and gets zeros in its whole (C, OH, OW) slab; every other ROI's
 * taps are clamped into the image.  Every element of y is written on every call, nothing outside y is written, and the same
 * inputs give the same bits on every call.  One thread per output pixel, looping over the channels; no LDS, no atomics, no
 * workspace.
 * MOGAN_ERR_SHAPE before any HIP call: a NULL pointer; B, H, W, OH or OW < 1; C < 1 or C > 4; R < 0; any of B C H W, H W or
 * R C OH OW above 2^31 - 1.  R = 0 returns 0 without a launch. */
int mogan_roi_resize(const float* x, int B, int C, int H, int W, const float* boxes, const int* image_index, long long R,
                     float* y, int OH, int OW, hipStream_t stream);

/* Radial power spectrum of a batch of images: what the spectral-artefact score is computed from (the azimuthally averaged power
 * spectrum of Durall et al. 2020, Dzanic et al. 2020, Schwarz et al. 2021; csrc/mogan_spectrum.hip;
 * attngan/spectrum.py has the whole definition; the reference has no code for it).  x (B, C, S, S) fp32, dense; weight (C) and
 * window (S, or NULL for all ones) fp32; twiddle S / 2 pairs (cos, -sin)(2 pi k / S) fp64, built by the host and 16-byte aligned --
 * the device calls no trigonometric function; bins (S, S / 2 + 1) int32 over the half plane v in [0, S / 2], an entry < 0 or
 * >= n_bins leaves its frequency out; out (B, n_bins) fp64.  All on the device.  Per image b, everything after the loads in fp64:
 *     y[i][j]   = (sum_c weight[c] x[b][c][i][j]) (window[i] window[j])               (c ascending)
 *     F[u][v]   = sum_ij y[i][j] exp(-2 pi i (u i + v j) / S)                           (unnormalised)
 *     out[b][k] = sum over (u, v) of the half plane with bins[u][v] = k of m(v) |F[u][v]|^2,    m = 1 for v in {0, S / 2}, else 2
 *   (the Hermitian symmetry of a real plane: the sum over the full plane of a table that is symmetric under (u, v) -> (-u, -v)).
 *   Three launches per round of at most 64 images: radix-2 transforms of the rows in LDS, the half spectrum to the workspace with
 *   its columns contiguous; transforms of a group of columns in LDS, one thread per bin adding the group's members in (column, u)
 *   order, n_bins partial sums per group to the workspace; a last sum over the groups in index order.  No atomics, no 2-D power
 *   plane in memory, and every workgroup works on ONE image:
 *     (a) the same inputs give the same bits on every call;
 *     (b) row b of out depends on image b only -- the same bits at B = 1 and at any position of any batch;
 *     (c) an all-zero image gives exactly 0.0 in every bin.
 *   Every element of out is written (0.0 for a bin without members).  The workspace is required, 16-byte aligned:
 *   mogan_radial_power_ws_bytes(B, S) = min(B, 64) ((S / 2 + 1) S 16 + G 2048), G = ceil((S / 2 + 1) / min(S / 2 + 1, 2048 / S))
 *   column groups (0 for arguments the call rejects): it does not grow with B past 64 images.  MOGAN_ERR_WS where ws is NULL,
 *   misaligned or shorter, nothing launched.
 *   B >= 1, 1 <= C <= 4, S a power of two in [8, 256], 1 <= n_bins <= 256, B C S S <= 2^31 - 1.
 * MOGAN_ERR_SHAPE before any HIP call (and before the workspace is looked at): a NULL pointer (window and ws apart), a misaligned
 * twiddle or out, any dimension outside the ranges above. */
size_t mogan_radial_power_ws_bytes(int B, int S);
int mogan_radial_power_f64(const float* x, int B, int C, int S, const float* weight, const float* window, const double* twiddle,
                           const int* bins, int n_bins, double* out, void* ws, size_t ws_bytes, hipStream_t stream);

/* The sums of the layout-shift score: what changes between an image generated under the data's layout and the image generated from
 * the same noise, text and labels with ONE box moved (csrc/mogan_layout.hip; attngan/layoutshift.py has the
 * whole definition and the numpy oracle; the reference has no code for it).  a, b (P, C, S, S) fp32, dense: P pairs, a under the
 * data's layout, b under the edit; edit (P, 6) int32 = (x0, y0, x1, y1, dx, dy): the moved object's pixel rectangle [x0, x1) x
 * [y0, y1) and its offset in pixels; others (P, G, 4) int32 = (x0, y0, x1, y1), the rectangles of the image's other objects, one
 * with x1 <= x0 is absent, and they may reach past the image; sums (P, 7) fp64; counts (P, 5) int32.  All on the device.
 * A pixel's class: 0 the old rectangle only, 1 the new one (old + (dx, dy)) only, 2 both, 3 neither and inside a rectangle of
 * `others`, 4 the rest.  Per pair, everything after the loads in fp64:
 *     sums[k]   = sum over the pixels p of class k and the channels of (a[p] - b[p])^2                      k = 0..4
 *     sums[5]   = sum over the pixels p of the old rectangle and the channels of (a[p] - b[p + delta])^2    "moved"
 *     sums[6]   = the same with a[p + delta] in the place of b[p + delta]                                   "baseline"
 *     counts[k] = pixels of class k (they add up to S S)
 *   One workgroup per pair, its threads striding over the pixels with seven fp64 partials and five counts each, added in LDS in a
 *   fixed tree; no atomics, no workspace:
 *     (a) the same inputs give the same bits on every call;
 *     (b) a pair's outputs depend on its own rows only -- the same bits at P = 1 and at any position of any batch;
 *     (c) b a bit copy of a gives sums[0..4] == 0.0 exactly and sums[5] == sums[6] bit for bit;
 *     (d) exchanging a and b changes no bit of sums[0..4];
 *     (e) delta = (0, 0) gives sums[6] == 0.0.
 *   Safe by construction: a pair whose edit rectangle is empty or not inside the image, or whose shifted copy is not inside it,
 *   reads no image data and gets zeros in all twelve outputs.  Every element of sums and counts is written on every call.
 *   P >= 1, 1 <= C <= 4, 2 <= S <= 1024, 0 <= G <= 8, P C S S <= 2^31 - 1.
 * MOGAN_ERR_SHAPE before any HIP call: a NULL pointer (others apart where G = 0), any dimension outside the ranges above. */
int mogan_box_shift_sums_f64(const float* a, const float* b, long long P, int C, int S, const int* edit, const int* others, int G,
                             double* sums, int* counts, hipStream_t stream);

/* The sums of the Inception Score: the softmax of a classifier head over pool codes, reduced per row and per split without the
 * (row, class) matrix ever reaching memory (csrc/mogan_softmax_head.hip; attngan/inception_score.py has the
 * whole definition and the numpy oracle; the reference has no code for it).  x (n, D) codes, w (C, D) and bias (C) the head, all
 * fp32, dense, widened exactly; row_lse (n, or NULL), row_h (n) and psum (S, C) fp64.  All on the device.  The n rows are cut into
 * S contiguous splits, split s = [floor(s n / S), floor((s + 1) n / S)) -- the rule is part of this contract.  Everything after the
 * loads in fp64:
 *     z[i][y]    = <x_i, w_y> + bias[y]             on v_mfma_f64_16x16x4_f64 in 64 x 64 tiles, k along D in index order
 *     row_lse[i] = log sum_y exp(z[i][y])           the maximum subtracted
 *     p[i][y]    = exp(z[i][y] - row_lse[i])
 *     row_h[i]   = sum_y p[i][y] (z[i][y] - row_lse[i])         a p of exactly 0 adds exactly 0, never a NaN
 *     psum[s][y] = sum_{i in split s} p[i][y]
 *   A workgroup owns a stripe of 64 rows -- the stripes of a split start at the split's first row -- and walks the head's column
 *   tiles twice, recomputing the logits: once for the log-sum-exp, once for p; one double per (stripe, class) goes to the
 *   workspace and a last launch of the same call adds a split's stripes in stripe order.  No atomics, every sum in one fixed order:
 *     (a) the same inputs give the same bits on every call;
 *     (b) row_lse[i] and row_h[i] depend on row i, the head, D and C only -- not on n, S or the row's position;
 *     (c) psum[s] depends on the split's rows in order and on the head only: it is, bit for bit, psum of the S = 1 call on those
 *         rows alone;
 *     (d) C = 1 gives row_h == 0.0, row_lse == z and psum == the split's row count, exactly.
 *   Every element of the outputs is written.  Non-finite inputs give non-finite outputs in their rows and splits, nothing else.
 *   The workspace is required, 8-byte aligned: mogan_softmax_head_ws_bytes(n, C, S) = 8 S T C, T = ceil(ceil(n / S) / 64) (0 for
 *   arguments the call rejects); MOGAN_ERR_WS where ws is NULL, misaligned or shorter, nothing launched.
 *   1 <= n <= 2^31 - 1, 1 <= D <= 65536, 1 <= C <= 2^20, 1 <= S <= min(n, 65535).
 * MOGAN_ERR_SHAPE before any HIP call (and before the workspace is looked at): a NULL x / w / bias / row_h / psum, an x, w or bias
 * that is not 4-byte aligned, a row_lse, row_h or psum that is not 8-byte aligned, any dimension outside the ranges above. */
size_t mogan_softmax_head_ws_bytes(long long n, int C, int S);
int mogan_softmax_head_f64(const float* x, long long n, int D, const float* w, const float* bias, int C, int S, double* row_lse,
                           double* row_h, double* psum, void* ws, size_t ws_bytes, hipStream_t stream);

/* The attention sheets of a generated image: what miscc/vis.build_super_images2 does per word on the host, on the device (DESIGN.md
 * section 9p; csrc/mogan_attn_sheet.hip; attngan/attnsheet.py has the whole definition and the numpy oracle).  attn (B, T, att,
 * att) fp32 >= 0, the generator's word attention; cap_lens (B) int32; img (B, 3, vis, vis) fp32 in [-1, 1]; table (vis, att) fp64,
 * the bilinear upscaling followed by the reflecting Gaussian as ONE matrix M the host builds (attnsheet.table; the kernel never
 * sees sigma); pick (P, 2) int32 = (sample, word).  All dense, all on the device.  Everything after the fp32 loads in fp64; both
 * thresholds are compared in fp32, t = (float) (2.0 / len):
 *     conf[b][t]  = sum a [a > 2 t]  for t < cap_lens[b], 0.0 otherwise          (the reference's conf_score / 3: its top-K order)
 *     A           = a [a > t]                          S = M A M^T               (vis, vis)
 *     lo = min S, hi = max S                           v = (S - lo) / (hi - lo) * 255        q = (u8) floor(v)
 *     image byte  = (u8) clamp(((x + 1) / 2) * 255, 0, 255)   in fp32, the roundings of the host's vis._to_uint8_range
 *     sheet[p][y][x][c] = Pillow's paste of q over the image byte through the constant mask alpha:
 *                         t = image (255 - alpha) + q alpha + 128, ((t >> 8) + t) >> 8
 *   sheet (P, vis, vis, 3) u8; stats (P, 2) fp64 = (lo, hi); flags (P) int32: 0 a sheet, 1 a flat map (hi == lo: q = 0 everywhere;
 *   the reference divides 0 by 0), 2 a map that holds a non-finite value (answered as a flat map with stats (0, 0)), 3 a pick that
 *   should never be sent.
 *   conf: one workgroup per (sample, word), partials added in LDS in a fixed tree.  sheet: one workgroup per pick; U = M A in strips
 *   of 32 output rows, S = U M^T in registers, every sum one fma per term in index order, the product walked twice in the same
 *   order (min and max, then quantise and blend); no atomics, no workspace, the (vis, vis) fp64 map never reaches memory:
 *     (a) the same inputs give the same bits on every call;
 *     (b) a pick's sheet, stats and flag depend on its own map, caption length, image and the table only -- the same bits alone
 *         and at any position of any pick list, for any B;
 *     (c) the bits do not depend on the alignment of attn or img beyond 4 bytes;
 *     (d) a map where nothing passes the threshold gives q == 0 everywhere, lo == hi == 0.0 bitwise and flag 1;
 *     (e) with the identity table S is A exactly: the sheet is the oracle's byte for byte.
 *   Safe by construction: a pick whose sample is outside [0, B), whose word is outside [0, T) or >= cap_lens[sample] reads nothing
 *   but its own pick row and that length, and gets a zero sheet, zero stats and flag 3.  Every element of the outputs is written.
 *   B >= 1, 1 <= T <= 32, 2 <= att <= 128, vis a multiple of att, att <= vis <= 256, 0 <= alpha <= 255, P >= 1,
 *   B T att att, 3 B vis vis and 3 P vis vis <= 2^31 - 1.
 * MOGAN_ERR_SHAPE before any HIP call: a NULL pointer, a table or stats that is not 8-byte aligned, any value outside the ranges. */
int mogan_attn_conf_f64(const float* attn, const int* cap_lens, int B, int T, int att, double* conf, hipStream_t stream);
int mogan_attn_sheet_f64(const float* attn, const int* cap_lens, const float* img, const double* table, const int* pick, int P, int B,
                         int T, int att, int vis, int alpha, unsigned char* sheet, double* stats, int* flags, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOGAN_HIP_H */
