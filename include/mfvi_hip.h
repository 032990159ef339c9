/*
 * mfvi_hip.h — C ABI of libmfvi_hip.so: the MI355X (gfx950) implementation of the
 * mean-field-VI deep-image-prior hot path of Cardio-AI/mfvi-dip-mia.
 *
 * The reference is pure Python/PyTorch, so there is no existing FFI to mirror; these entry points are
 * what a ctypes/cffi binding of the reference's path binds (see INTEGRATION.md for the stub).  Each
 * one names the reference code it replaces (paths relative to the reference repo root).
 *
 * Conventions
 *  - plain C: opaque handles, raw DEVICE pointers, sizes, a hipStream_t passed as void*.
 *  - every call is asynchronous on `stream` and allocates nothing; the caller owns all buffers.  One exception: mfvi_plan_create
 *    hipMallocs the plan's small device tables (BatchNorm, weight-sampling, gradient-reduction, Dropout2d entries; a few KB) and the
 *    plan lazily creates one low-priority side stream with its events; mfvi_plan_destroy releases them.
 *  - return value: 0 = ok, <0 = argument/shape error, >0 = hipError_t.  mfvi_last_error() returns a
 *    thread-local message for the last non-zero return.  Nothing throws across the boundary.
 *  - tensors are fp32, NCHW with N = MC sample index; parameters live in three flat fp32 blocks
 *    MU[n_vi], RHO[n_vi], BN[n_bn] (per VI layer: W then bias, in module order; per BatchNorm: gamma
 *    then beta).  Gradients use the same layout.
 *  - random numbers follow "RNG spec v1" (DESIGN.md): Philox4x32-10 keyed by seed, counter
 *    (block, domain<<24|stream, sample, step); eps of VI layer l, tensor t (0 = W, 1 = bias),
 *    element j is lane j&3 of block j>>2 of stream 2l+t in domain 0.
 *  - process-wide switches.  The library holds no mutable global state, but it reads the environment variables below ONCE (first use,
 *    function-local statics); none of them changes a result beyond summation-order rounding, all exist for A/B timing and for the
 *    cross-check tests.  Per-plan state has setters (mfvi_plan_set_*) instead.
 *      MFVI_DISABLE_MFMA=1     every convolution on the generic fp32 VALU kernels
 *      MFVI_AUTOTUNE=0         mfvi_plan_autotune returns at once (heuristic tilings)
 *      MFVI_TUNE=mf,th,T       force one tiling of the round-2 MFMA forward / backward-data kernels where the plan holds none
 *      MFVI_TUNE_W=nb,w,tgt    the same for the backward-weight kernels
 *      MFVI_RP=0               keep the 3x3 stride-1 layers on the round-2 kernels (row-phase kernels of conv_rp.hip off)
 *      MFVI_X6=0               heuristic tilings (no autotune): backward-weight never on the bf16x6 kernel (conv_bww_x6.hip); the autotuner's
 *                              candidates and explicit tilings (w = 11; forward: tune bit 25, conv_x6.hip) are not affected
 *      MFVI_TUNE_RP=mf,r,T[,rem[,ks]]  force one row-phase tiling where the plan holds none
 *      MFVI_RP_INTERLEAVE=0    row-phase kernels: a block takes a contiguous run of T tiles (default: tiles b, b + nx, b + 2 nx, ... so that the
 *                              blocks of an XCD work on adjacent tiles at every moment: halo rows and straddled cache lines are L2 hits)
 *      MFVI_PHASE=0            stride-2 backward-data: zero-stuffed formulation instead of the phase decomposition
 *      MFVI_FOLD_FUSION=0      1x1 backward-data writes the padded gradient + a finalize_dx launch (fold not fused)
 *      MFVI_FOLD_FUSION3=0     the same for the 3x3 stride-1 layers
 *      MFVI_SIDE_STREAM=0      backward-weight kernels on the caller's stream (default: the plan's side stream; mfvi_plan_set_side_stream)
 *      MFVI_SIDE_MAXPIX=n      only layers with at most n output pixels fork onto the side stream
 *      MFVI_SIDE_PRIO=0        side stream at default priority (default: lowest)
 *      MFVI_FWD_FORK=n         forward pass: skip-branch 1x1 convolutions on maps of up to n pixels run on the side stream (default 16384, 0 = off)
 *      MFVI_FORK_ON_PACKET=0   fork / join events as separate hipEventRecord packets instead of riding on kernel dispatch packets
 *      MFVI_FUSE_SKIP_BWD=0    the narrow 1x1 skip convolutions keep their own backward-data launch (default: formed inside the fold of the
 *                              tensor they share with the scale's stride-2 convolution, kernel family 5)
 *      MFVI_CONCAT_TILED=w     concat forward: LDS-tiled kernel for maps at least w wide (default 128; 0 = never)
 *      MFVI_CONCAT_TPB=n       concat forward, tiled kernel: tiles per block (default 4)
 *      MFVI_CONCAT_BWD_TILE=w  concat backward: force the 16 x 64 / 32 x 32 / 16 x 16 low-res tile (w = 64 / 32 / 16; default: by map width)
 *      MFVI_INKERNEL_MAX_W     (compile-time, csrc/common.h) largest layer the autotuner tries on the in-kernel-eps generic kernels (tune bit 27)
 *      MFVI_DEBUG_FIN          print the gradient-reduction table to stderr
 */
#ifndef MFVI_HIP_H
#define MFVI_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFVI_ABI_VERSION 6

typedef struct mfvi_plan mfvi_plan;

enum { MFVI_OP_CONV = 1, MFVI_OP_CONCAT_UP = 2, MFVI_OP_CONV_LRT = 3 };
enum { MFVI_UP_BILINEAR = 0, MFVI_UP_NEAREST = 1 };   /* nn.Upsample(scale_factor=2, mode=...) (models/skip.py:102) */
enum { MFVI_TASK_DENOISE = 0, MFVI_TASK_SR = 1 };
enum { MFVI_PARAM_F32 = 0, MFVI_PARAM_BF16 = 1 };     /* storage of the MU / RHO blocks (mfvi_plan_set_param_dtype) */

/* An activation tensor of the layer program, [C][H][W] per MC sample, stored RAW (conv output or
 * concat result).  Consumers read view(T) = LeakyReLU?(BatchNorm_train?(T)): the BatchNorm2d (training
 * mode, batch 1: models/common.py:96-97) and LeakyReLU(0.2) (models/common.py:83) that follow T in
 * models/skip.py:68-119 are folded into the loads of whatever consumes T. */
typedef struct {
    int32_t C, H, W;
    int32_t has_bn;      /* train-mode BN with per-sample statistics over H*W */
    int32_t has_act;     /* LeakyReLU(slope) after the BN */
    float   slope;
    float   eps;
    float   drop_p;      /* > 0: nn.Dropout2d(p) between the producing conv and the BN (models/common.py:125-131, the
                          * MC-dropout sibling's nets); needs has_bn.  Channel c of sample k is kept iff u >= p with u the
                          * U[0,1) of element c of stream <producing layer_id> in RNG domain 5, and scaled by 1/(1-p). */
    int64_t bn_off;      /* offset of gamma[C] (beta[C] follows) inside the BN block */
} mfvi_tensor_desc;

/* One fused op.
 * MFVI_OP_CONV       out = conv2d(reflection_pad(view(in0), ksize/2), w, b, stride), w = mu + softplus(rho)*eps
 *                    = ReflectionPad2d + Conv2dRT: models/common.py:100-135, BayTorch/modules/reparam_layers.py:26-37,
 *                      BayTorch/modules/module.py:82-85.
 * MFVI_OP_CONV_LRT   the same layer with the LOCAL reparameterisation (Conv2dLRT: BayTorch/modules/reparam_layers.py:39-72, conv.py:74-106;
 *                    MeanFieldVI(reparam='local')): with v = reflection_pad(view(in0)),
 *                        out = conv2d(v, mu, mu_b) + sqrt(1e-16 + conv2d(v**2, softplus(rho)**2, softplus(rho_b)**2)) * eps,
 *                    eps ~ N(0,1) in OUTPUT space: element j of [Cout][Ho][Wo] = lane j & 3 of block j >> 2 of RNG domain 7, stream
 *                    layer_id.  sample_weights = 0: out = conv2d(v, mu, mu_b) (LRTLayer's eval branch).  Same parameters, same KL.
 * MFVI_OP_CONCAT_UP  out = cat(view(in0), upsample2x_bilinear(view(in1)))  (in0 = -1: upsample only)
 *                    = Concat + nn.Upsample: models/common.py:23-43, models/skip.py:102.  out has in0's H x W, which may be one
 *                    row / column short of 2 x in1's (odd sizes): Concat's centre-crop (models/common.py:31-41) then drops the
 *                    up-sampled branch's last row / column.  Any other size relation is rejected. */
typedef struct {
    int32_t type;
    int32_t in0, in1, out;
    int32_t ksize, stride;
    int32_t layer_id;        /* VI layer index = RNG stream / 2 */
    int32_t up_mode;
    int64_t w_off, b_off;    /* offsets of W and bias inside MU / RHO; b_off < 0: no bias */
} mfvi_op_desc;

/* ---- layer program (replaces MeanFieldVI.forward / autograd of it: BayTorch/freq_to_bayes.py:40-41) ---- */
int mfvi_plan_create(const mfvi_tensor_desc* tensors, int n_tensors, const mfvi_op_desc* ops, int n_ops,
                     int input_tensor, int output_tensor, int64_t n_vi, int64_t n_bn, int max_samples,
                     mfvi_plan** plan);
void mfvi_plan_destroy(mfvi_plan* plan);
/* mfvi_backward runs the backward-weight kernels on a low-priority side stream owned by the plan (forked per layer behind the event
 * "dy of this layer is final" on the caller's stream, joined before the gradient reduction), so they overlap the backward-data /
 * fold chain that carries the critical path.  Results are unchanged.  enabled = 0 keeps every launch on the caller's stream
 * (e.g. to time a kernel alone); MFVI_SIDE_STREAM=0 in the environment does the same for every plan.  Once that stream exists,
 * mfvi_forward uses it too: a skip-branch convolution on a small map (<= MFVI_FWD_FORK pixels, default 128 x 128; 0 = never) runs there
 * beside the down path of its scale and is joined in front of its concat. */
int mfvi_plan_set_side_stream(mfvi_plan* plan, int enabled);
/* Device-resident iteration (ABI v6).  The reference's hot loop draws fresh noise every iteration from the loop index i
 * (bayesian_optimization.py:1360-1372); here that index is the `step` word of the counter RNG.  With a step source set, the plan's
 * kernels read the counter from DEVICE memory at run time (counter = step argument + *step_dev), so ONE captured HIP graph of an
 * iteration can be replayed for every i: the caller advances *step_dev on the device (one tiny launch inside the graph) and passes
 * step = 0.  nullptr (default): the `step` argument is the counter itself.  Results are bit-identical to passing the same counter
 * values from the host. */
int mfvi_plan_set_step_source(mfvi_plan* plan, const int32_t* step_dev);
/* enabled != 0 while the caller captures mfvi_forward / mfvi_backward into a HIP graph (hipStreamBeginCapture on `stream`): fork / join
 * events between the caller's stream and the plan's side stream are plain hipEventRecord / hipStreamWaitEvent pairs, which stream capture
 * turns into graph edges (default: they ride on the kernels' dispatch packets, hipExtLaunchKernelGGL, which capture does not record).
 * The plan must have run once un-captured (tables uploaded, events and the side stream created: none of that may happen under capture). */
int mfvi_plan_set_capture_mode(mfvi_plan* plan, int enabled);
/* Gradient split for an overlapped exchange (K sharded over ranks: DESIGN.md section 7; the reference has one process per fit and no exchange,
 * bayesian_optimization.py:3760-3775).  The flat layout is in op order and the backward pass runs the ops last to first, so the weight /
 * bias gradients of the ops >= first_op — the tail [offset, n_vi) of dmu and of drho — are complete long before the pass ends.  With a
 * split set, mfvi_backward reduces that group into dmu / drho on comm_stream as soon as the kernels producing it are enqueued (comm_stream
 * waits for them through events), and the rest at the end on the caller's stream as before: a collective enqueued on comm_stream after
 * mfvi_backward returns runs under the tail of the pass.  The caller joins comm_stream before it reads the gradients and before the
 * next mfvi_backward.  Results are bit-identical with and without a split.  first_op < 0 removes the split.  Not available for plans with
 * local-reparameterisation layers (their d rho is completed in one pass at the end).  mfvi_plan_grad_split_offset returns the tail's
 * first parameter index (-1 and an error if the ops >= first_op do not own a tail of the layout). */
int mfvi_plan_set_grad_split(mfvi_plan* plan, int first_op, void* comm_stream);
int mfvi_plan_grad_split_offset(const mfvi_plan* plan, int first_op, int64_t* offset);
/* Dropout2d layers of the program are active by default (the reference keeps its MC-dropout nets in train mode);
 * enabled = 0 makes them the identity (nn.Dropout2d in eval mode). */
int mfvi_plan_set_dropout(mfvi_plan* plan, int enabled);
/* nn.BatchNorm2d's running statistics (models/common.py:96-97: momentum 0.1, unbiased variance; the reference never reads them, but they
 * are part of the state_dict a reference run produces).  `running`: n_bn floats laid out like the BN block — running_mean at the gamma
 * slots, running_var at the beta slots.  mfvi_plan_bn_update_running applies the update of the n_samples batch-1 forwards just run by
 * mfvi_forward (their batch sums are still in the workspace), sample by sample in order.  mfvi_plan_set_bn_eval(plan, running) makes
 * mfvi_forward normalise with these statistics instead (module.eval(); NULL: back to batch statistics); forward only — mfvi_backward
 * refuses while it is set.  The pointer is kept, the caller keeps the buffer alive. */
int mfvi_plan_bn_update_running(const mfvi_plan* plan, const void* workspace, int n_samples, float momentum, float* running, void* stream);
int mfvi_plan_set_bn_eval(mfvi_plan* plan, const float* running);
/* bfloat16 storage of mu / rho (BASELINE configs[4]: "bf16 mu/rho with fp32 KL accumulate"; the reference keeps float32 Parameters:
 * BayTorch/modules/module.py:45-62).  With MFVI_PARAM_BF16 the `mu` / `rho` arguments of mfvi_forward / mfvi_backward / mfvi_plan_autotune
 * point to arrays of n_vi bf16 values (uint16_t: the upper half of the float32 pattern); the reparameterisation draw reads them directly
 * (half the parameter bytes per pass) and every value computed from them — sampled weights, activations, gradients, KL — is float32
 * exactly as with float32 storage of the same (bf16-representable) numbers.  Gradients, Adam moments and the BatchNorm block stay
 * float32.  The update rule is mfvi_elbo_update_bf16: no float32 master copy, stochastic rounding.  mu and rho must be 8-byte aligned. */
int mfvi_plan_set_param_dtype(mfvi_plan* plan, int dtype);
/* Fits mode: one call of mfvi_forward / mfvi_backward advances MANY independent fits.  With S = samples_per_fit > 0
 * the n_samples of a call (a multiple of S) are n_samples / S fits of S samples each: sample i belongs to fit i / S and still uses eps of
 * global sample index k0 + i (the RNG is unchanged; mfvi_plan_set_fits_sample_stride below changes the index).  mu / rho / bn point at fit 0, fit j's blocks lie j * param_stride floats further on
 * (one flat row [MU | RHO | BN] per fit works with a single stride); dmu / drho / dbn
 * likewise with grad_stride.  z is [n_fits][Cin][H][W], one input per fit; out / dout / dz stay [n_samples][C][H][W].  Every weight gradient is
 * summed over the samples of its fit only; on the matrix-core kernels in a fixed order, no atomics.  A layer those decline (a map not a
 * multiple of 4 wide) runs on the generic fp32 kernels with the fit's mu / rho, as in single-fit mode: their weight gradient uses fp32
 * atomicAdd over samples and tiles in both modes, so a net that reaches them is not bit-reproducible from call to call.  S = 0 (the default) switches the mode off: one fit, as before.
 * S > 1 grows the workspace by one copy of the net input per sample: ask mfvi_plan_workspace_bytes again afterwards.
 * Not served, and refused with MFVI_ERR_FITS_UNSUPPORTED and a message (never run with fit 0's parameters): bf16 parameter storage, plans
 * with local-reparameterisation layers, sample_weights = 0 (unless mfvi_plan_set_fits_points), BatchNorm eval mode and mfvi_plan_bn_update_running, a gradient split, a device
 * step source, layers outside the sampled-weight slab (input channels / weight offsets not multiples of 4) and MFVI_DISABLE_MFMA.
 * mfvi_plan_autotune runs BEFORE the mode is switched on (tilings do not depend on it); in-kernel-eps tilings (tune bit 27) fall back to the
 * heuristic when it is. */
#define MFVI_ERR_FITS_UNSUPPORTED (-5)
int mfvi_plan_set_fits(mfvi_plan* plan, int samples_per_fit, int64_t param_stride, int64_t grad_stride);
/* Point weights in fits mode (the DIP / MC-dropout / SGLD siblings run w = mu).  Off by default: fits mode refuses
 * sample_weights = 0.  While on, a fits-mode pass with sample_weights = 0 writes every sample's row of the sampled-weight slab with its own
 * fit's mu (eps = 0, weights and biases), every conv family reads the rows as in a sampled pass, each fit's samples are reduced into that
 * fit's dmu row and drho is not touched.  No effect outside fits mode.  Refused (MFVI_ERR_FITS_UNSUPPORTED) for what fits mode refuses. */
int mfvi_plan_set_fits_points(mfvi_plan* plan, int enabled);
/* Dropout2d probability per fit (fits mode): sample k of a pass draws the factors of every tensor created with dropout with p[k / S]
 * instead of the tensor's own drop_p -- same Philox counter, same comparison u >= p, same scale 1.0f / (1.0f - p), so a fit whose p equals
 * the tensor's gets bit-identical masks; p = 0 gives factors of 1.  p: HOST array of n_fits values in [0, 1) (copied); NULL or n_fits = 0
 * clears it.  A fits-mode pass whose n_samples / S differs from n_fits is refused before any launch. */
int mfvi_plan_set_fit_dropout(mfvi_plan* plan, const float* p, int n_fits);
/* The eps / Dropout2d sample index of a fit (fits mode): afterwards sample i of a pass (fit j = i / S, draw s = i % S) uses
 * global sample k0 + j * stride + s.  The default, restored by every mfvi_plan_set_fits call, is stride = S: k0 + i, as described above.
 * stride = 0 makes every fit draw the samples k0 .. k0 + S - 1, the indices a single-fit plan uses for the same call -- what a batched
 * posterior prediction needs to reproduce each fit's stand-alone draws.  -1 (and a message) for a negative stride or a plan outside fits
 * mode.  Forward only: mfvi_backward on a plan whose stride differs from S is refused with MFVI_ERR_FITS_UNSUPPORTED before any launch. */
int mfvi_plan_set_fits_sample_stride(mfvi_plan* plan, int64_t stride);
/* bytes of caller-provided device workspace (activations, gradients, BN statistics) for max_samples */
int64_t mfvi_plan_workspace_bytes(const mfvi_plan* plan);

/* n_samples MC forwards of the net on the SAME input z[Cin][H][W]; sample i uses eps of global sample
 * index k0+i.  sample_weights = 0 reproduces RTLayer's eval branch (w = mu).  out: [n_samples][Cout][H][W]. */
int mfvi_forward(mfvi_plan* plan, const void* mu, const void* rho, const float* bn, const float* z,
                 uint64_t seed, uint32_t step, uint32_t k0, int n_samples, int sample_weights,
                 void* workspace, float* out, void* stream);
/* Backward of the same call (workspace must still hold its activations).  dout: [n_samples][Cout][H][W].
 * dmu/drho/dbn are ACCUMULATED into (+=).  dz (optional): [n_samples][Cin][H][W].
 * mu / rho / bn must still hold the values the forward saw: the first backward after a forward with the same (pointers, seed, step,
 * k0, n_samples) re-uses the weights that forward drew (they are in the workspace) instead of drawing them again; any further
 * backward of the same forward draws them afresh from mu / rho. */
int mfvi_backward(mfvi_plan* plan, const void* mu, const void* rho, const float* bn, const float* z,
                  uint64_t seed, uint32_t step, uint32_t k0, int n_samples, int sample_weights,
                  void* workspace, const float* dout, float* dmu, float* drho, float* dbn, float* dz, void* stream);
/* Debug/parity access: copy tensor `tensor_id` of sample `sample` from the workspace to dst (device):
 * which = 0: raw activation [C][H][W]; 1: gradient wrt its BN output (valid after mfvi_backward);
 * 2: its forward BN sums as doubles [C][2] (dst must hold 2*C doubles). */
int mfvi_plan_read_tensor(const mfvi_plan* plan, const void* workspace, int tensor_id, int sample, int which, void* dst, void* stream);

/* Optional per-kernel timing with HIP events recorded on the caller's stream around the plan's launches.
 * mode 0: off; 1: every kernel; 2: only kernel (op, pass).  pass: 0 forward, 1 backward-weight, 2 backward-data,
 * 3 fold/finalize, 4 concat backward, 5 gradient finalize, 6 weight sampling (both op -1).  mfvi_plan_profile_read synchronises the recorded events, writes up to
 * `capacity` records (op index, pass, milliseconds) and clears the log. */
int mfvi_plan_profile(mfvi_plan* plan, int mode, int op, int pass);
int mfvi_plan_profile_read(mfvi_plan* plan, int capacity, int* n_records, int* ops, int* passes, float* ms);

/* Optional, once per plan: run one forward + backward, then time every valid MFMA tiling (output-channel fragments x tile
 * rows x tiles per block) of every conv op's forward, backward-data and backward-weight kernel with HIP events on `stream` and keep the
 * fastest per (op, pass).  Tilings do not change the forward result (same accumulation order per output element); gradients agree to
 * summation-order rounding (partial sums per pixel strip, the 4x4x1 variant below).
 * out_scratch: 2 * n_samples * numel(output tensor) floats; grad_scratch: 2 * n_vi + n_bn floats.  Synchronises `stream`.
 * Contents of workspace / scratch are undefined afterwards.  MFVI_AUTOTUNE=0 in the environment makes this a no-op. */
int mfvi_plan_autotune(mfvi_plan* plan, const void* mu, const void* rho, const float* bn, const float* z, int n_samples,
                       void* workspace, float* out_scratch, float* grad_scratch, void* stream);
/* Tiling in use for conv op `op`: which 0 forward, 1 backward-data (mf | th << 8 | T << 16; th bit 128 = tiles of whole rows for
 * narrow maps, th bit 64 (backward-data of layers with 16n + 4 input channels) = the last 4 channels on the 4x4x1 matrix instruction
 * instead of a padded 16-channel fragment), 2 backward-weight (input tiles | waves << 8 | block target/256 << 16; waves: 4, 8, 9 = 8 waves
 * producer/consumer specialised, 10 = the fragment-split variant with input tiles = 2: one block per 32-36 input channels, the accumulator
 * fragments dealt to the consumer waves); 0 = built-in heuristic. */
int mfvi_plan_get_tune(const mfvi_plan* plan, int op, int which);
int mfvi_plan_set_tune(mfvi_plan* plan, int op, int which, int tune);
/* Kernel family that served conv op `op` in its last forward (which 0) / backward-data (1) / backward-weight (2) launch: 0 = generic fp32
 * VALU kernels (also: a tiling the shape does not admit falls back to them), 1 = fp32 MFMA kernels, 2 = row-phase fp32 MFMA kernels
 * (3x3 stride 1, maps a multiple of 64 wide or exactly 32 / 16 wide), 3 = bf16x6 kernels (fp32 operands as three bf16 pieces on the bf16
 * matrix instruction: forward tune bit 25 = mf | rows << 8 | strips per block << 16, bit 12 = the 4-channel remainder plane rides on the
 * last 32-channel group's pass (mf = 1, Cin = 32 n + 4); backward-data with the fold tune bit 25 = strips per block | rows per strip << 8
 * (8 / 4 / 2 for 16 / 32 / 64 output channels), bit 16 = the strip-resident form for 32 (+ 4) -> 16 layers (conv_bwd_x6s.hip);
 * backward-weight w = 11, input tiles field = output fragments per block), 4 = one-stage kernels with the block's whole reduction in LDS
 * (tune = 1 | 1 << 26: 3x3 stride 1 on 8- / 16-wide maps with <= 144 reduction channels, conv_small.hip; 1x1 layers with 16 | Cin, Cout <= 128
 * and 2 / 4 / 8 output fragments on maps of 64 n pixels, conv_1x1.hip), 5 (backward-data slot only) = no launch of its own: the gradient of a
 * narrow 1x1 convolution (<= 8 output channels) wrt an input it shares with one other convolution is formed inside that tensor's fold
 * (finalize_dx_vec1_kernel; MFVI_FUSE_SKIP_BWD=0 keeps the separate launch), 6 (forward slot only) = streaming forward of a narrow 1x1
 * layer (tune = 1 | 1 << 28: Cin in {4 ... 16, 32, 64}, at most 16 output channels (32 for 16 or 32 input channels), maps of 64 n pixels; conv_1x1.hip).  -1: bad arguments.  Tests use it to prove that the kernel
 * under test is the one that ran. */
int mfvi_plan_last_kernel(const mfvi_plan* plan, int op, int which);

/* ---- losses -------------------------------------------------------------------------------------------- */
/* gaussian_nll (utils/bayesian_utils.py:29-32) for n samples of out[n][2][H][W] against target[H/f][W/f];
 * f > 1 applies the SR projection out[..., ::f, ::f] first (bayesian_optimization.py:2095-2099,2182-2185).
 * nll_sum (device double) += sum_i nll_i.  dout (optional) = grad_scale * d nll_i / d out_i. */
int mfvi_gaussian_nll(const float* out, const float* target, int n, int H, int W, int factor,
                      float grad_scale, float* dout, double* nll_sum, void* stream);
/* gaussian_nll(D(out)[:, :1], D(out)[:, 1:], target) (bayesian_optimization.py:2182-2185, utils/bayesian_utils.py:29-32) with D the
 * downsampler of mfvi_downsample (models/downsampler.py:6-136) applied to BOTH channels of out[n][2][H][W]; target[H/factor][W/factor].
 * Accumulation and gradient contract of mfvi_gaussian_nll: nll_sum += sum_i nll_i (mean over the low-resolution pixels);
 * dout (optional) = grad_scale * d nll_i / d out_i, dense (every element written, fixed summation order).  scratch: n * 2 * (H/factor) *
 * (W/factor) floats (the low-resolution gradient; needed with dout).  Two launches: filter + NLL + low-resolution gradient, the adjoint. */
int mfvi_gaussian_nll_filtered(const float* out, const float* target, int n, int H, int W, int factor, const float* taps, int n_taps,
                               float grad_scale, float* scratch, float* dout, double* nll_sum, void* stream);
/* mse_loss(radon(out), sino) (bayesian_optimization.py:576, radon/radon.py:49-53): out[n][1][H][W],
 * theta_deg[T], sino[T][W]; scratch: n*T*W floats.  mse_sum += sum_i mse_i; dout = grad_scale * d mse_i/d out_i. */
/* gaussian_nll_inpainting (utils/bayesian_utils.py:35-39) with the runner's sigmoid on the colour channels
 * (bayesian_optimization.py:3033-3036): out[n][4][H][W] = 3 colour logits + 1 shared neg-log-variance, target[3][H][W],
 * mask[mask_channels][H][W] (1 or 3, broadcast); mean over the 3*H*W elements.  Same accumulation / gradient contract as
 * mfvi_gaussian_nll. */
int mfvi_gaussian_nll_inpainting(const float* out, const float* target, const float* mask, int mask_channels, int n, int H, int W,
                                 float grad_scale, float* dout, double* nll_sum, void* stream);
/* The same two losses in the call shape of the reference's functions — separate tensors, as the drop-in `gaussian_nll(out[:, :1],
 * out[:, 1:], target)` / `gaussian_nll_inpainting(out_pred, out[:, 3:], img, mask)` hand them over (utils/bayesian_utils.py:29-39):
 * mu / target [C][HW], neg_logvar [Cs][HW] with Cs == C or 1 (broadcast over channels), mask NULL or [Cm][HW] with Cm == C or 1.
 * loss_out (device double, overwritten) = mean (reduction_mean) or sum of (exp(s) (target - mu)^2 - s) * mask, s = clamp(neg_logvar, -20, 20).
 * The backward multiplies by the upstream gradient read from DEVICE memory (grad_out[0]): no host sync inside autograd. */
int mfvi_gaussian_nll_tensors(const float* mu, const float* neg_logvar, const float* target, const float* mask, int C, int Cs, int Cm, int64_t HW,
                              int reduction_mean, double* loss_out, void* stream);
int mfvi_gaussian_nll_tensors_backward(const float* mu, const float* neg_logvar, const float* target, const float* mask, int C, int Cs, int Cm,
                                       int64_t HW, int reduction_mean, const float* grad_out, float* dmu, float* dneg_logvar, void* stream);
int mfvi_radon_mse(const float* out, const float* sino, const float* theta_deg, int n, int H, int W, int T,
                   float grad_scale, float* scratch, float* dout, double* mse_sum, void* stream);
int mfvi_radon_forward(const float* img, const float* theta_deg, int n, int H, int W, int T, float* sino, void* stream);
int mfvi_radon_adjoint(const float* dsino, const float* theta_deg, int n, int H, int W, int T, float* dimg, void* stream);
/* The same operator on n independent square planes, built for the drop-in FastRadonTransform (radon/radon.py:23-55 as the CT runners
 * call it, bayesian_optimization.py:546, :576): the rows of a ray (project) and the angles of a pixel (backproject) are split over the
 * waves of a block and combined through LDS in a fixed order, so one plane fills the device.  theta_deg[T] in degrees (device memory).
 * Bit-identical from call to call.  Null pointers, n < 1 or > 65535, S or T < 1 or > 32768: -1 and mfvi_last_error(). */
int mfvi_radon_project(const float* img, const float* theta_deg, int n, int S, int T, float* sino, void* stream);       /* img[n][S][S] -> sino[n][T][S] */
int mfvi_radon_backproject(const float* dsino, const float* theta_deg, int n, int S, int T, float* dimg, void* stream); /* exact-neighbourhood transpose */

/* ---- KL (VIModule._kl / MeanFieldVI.kl: BayTorch/modules/module.py:64-80, freq_to_bayes.py:43-48) ------- */
/* kl_out (device double, overwritten) = sum_j log(s_j/s0) + (s0^2 + (mu_j-m0)^2)/(2 s_j^2) - 1/2 */
int mfvi_kl(const float* mu, const float* rho, int64_t n, float prior_mu, float prior_sigma, double* kl_out, void* stream);
/* dmu += scale * dKL/dmu, drho += scale * dKL/drho */
int mfvi_kl_backward(const float* mu, const float* rho, int64_t n, float prior_mu, float prior_sigma, float scale,
                     float* dmu, float* drho, void* stream);
/* The direction of the KL term.  The reference's VIModule carries a kl_type (BayTorch/modules/module.py:17, 40, 64-80; handed down by
 * MeanFieldVI, freq_to_bayes.py:9-16), named the opposite way round from what one would guess:
 *   MFVI_KL_REVERSE  kl_type == 'reverse' (the default, what all runners use): kl_divergence(prior, posterior) = KL(p || q), the term above;
 *   MFVI_KL_FORWARD  any other kl_type: kl_divergence(posterior, prior) = KL(q || p), the KL term of the textbook ELBO.  Per (mu, rho) pair,
 *                    s = softplus(rho), d = mu - m0:
 *                        kl = log(s0) - log(s) + (s^2 + d^2) / (2 s0^2) - 1/2,   dkl/dmu = d / s0^2,   dkl/drho = (s / s0^2 - 1 / s) sigmoid(rho)
 * float32 per element, summed in float64 in the order of the reverse kernels.  Each *_typed entry is its twin below / above with the
 * direction as an argument: MFVI_KL_REVERSE runs the twin itself (bit-identical), MFVI_KL_FORWARD the forward kernels with the same
 * launches, scratch and reduction order.  Refused with -1 and mfvi_last_error() before any launch: kl_type outside {0, 1}, prior_sigma
 * not finite or <= 0, for forward a prior_sigma^2 that is not a normal float32, null pointers, n < 1. */
#define MFVI_KL_REVERSE 0
#define MFVI_KL_FORWARD 1
int mfvi_kl_typed(const float* mu, const float* rho, int64_t n, float prior_mu, float prior_sigma, int kl_type, double* kl_out, void* stream);
int mfvi_kl_backward_typed(const float* mu, const float* rho, int64_t n, float prior_mu, float prior_sigma, float scale, int kl_type,
                           float* dmu, float* drho, void* stream);

/* ---- optimizer (torch.optim.AdamW(lr, weight_decay=0): bayesian_optimization.py:1356-1357,1372) --------- */
int mfvi_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                   float eps, int t, void* stream);
/* The deterministic tail of one ELBO iteration in one pass over the parameters (bayesian_optimization.py:1368-1372): kl_out = KL of all n_vi
 * (mu, rho) pairs, grads += temp * dKL (written back), then AdamW(weight_decay = 0) on the flat blocks [MU | RHO | BN] of
 * params / grads / m / v (2*n_vi + n_bn floats each).  Same per-element arithmetic as mfvi_kl + mfvi_kl_backward +
 * mfvi_adam_step; the KL sum is reduced in a fixed order (bit-reproducible).  scratch: mfvi_elbo_update_scratch_bytes()
 * bytes of device memory (per-block partial sums; contents need not be preserved between calls). */
int64_t mfvi_elbo_update_scratch_bytes(void);
int mfvi_elbo_update(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu, float prior_sigma,
                     float temp, float lr, float beta1, float beta2, float eps, int t, double* kl_out, void* scratch, void* stream);
/* mfvi_elbo_update for bf16 mu / rho: mu_bf16 / rho_bf16 = n_vi bf16 values each, bn = the float32 BatchNorm block; grads / m / v
 * keep the float32 layout [MU | RHO | BN].  KL terms and the gradient in float32 on the values the bf16 parameters denote, KL summed in
 * float64, Adam in float32; the new mu / rho are rounded to bf16 STOCHASTICALLY (an fp32 master copy would double the parameter state;
 * round-to-nearest would freeze rho: lr = 1e-3 against ulp_bf16(-3) = 1.6e-2): magnitude rounded up with probability
 * (discarded 16 bits) / 2^16, the 16-bit word = upper half of lane j & 3 of Philox block j >> 2, RNG domain 6, stream 0 (MU) / 1 (RHO),
 * sample 0, step t — deterministic and reproducible on the CPU (oracle/). */
int mfvi_elbo_update_bf16(void* mu_bf16, void* rho_bf16, float* bn, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu,
                          float prior_sigma, float temp, float lr, float beta1, float beta2, float eps, int t, uint64_t seed, double* kl_out,
                          void* scratch, void* stream);
/* bf16 <-> float32 copies of n values (float32 -> bf16 rounds to nearest even) */
int mfvi_bf16_to_f32(const void* src, int64_t n, float* dst, void* stream);
int mfvi_f32_to_bf16(const float* src, int64_t n, void* dst, void* stream);
/* The CT runners' NaN guard, `if not torch.isnan(loss): optimizer.step()` (bayesian_optimization.py:380, 581-582, 792, 994), without a host
 * sync.  loss = data term + temp * KL, and KL is a function of the parameters alone (finite while every earlier update was), so the guard
 * reads the DATA-TERM scalar of this iteration on the device: loss_d (the double accumulator of mfvi_radon_mse & co) and / or loss_f (the
 * float that rode the K-sharded all-reduce); either may be NULL.  NaN there: params / m / v are left untouched (kl_out is still written)
 * and *t_applied — the device counter of APPLIED updates that sets Adam's bias corrections, like torch's per-parameter state['step'] —
 * is not advanced.  Otherwise the update is number *t_applied + 1 and mfvi_elbo_update_guarded advances the counter itself;
 * mfvi_adamw_step_guarded only reads it (one optimizer step may cover several parameter blocks): call mfvi_step_advance once after them. */
int mfvi_elbo_update_guarded(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu, float prior_sigma,
                             float temp, float lr, float beta1, float beta2, float eps, int32_t* t_applied, const double* loss_d,
                             const float* loss_f, double* kl_out, void* scratch, void* stream);
/* mfvi_elbo_update / _guarded / _bf16 with the direction of the KL term (MFVI_KL_REVERSE / MFVI_KL_FORWARD above; BayTorch/modules/module.py:64-80)
 * as a by-value argument behind temp: the same launches and scratch, so the device-resident and the captured iteration take it as they are. */
int mfvi_elbo_update_typed(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu, float prior_sigma,
                           float temp, int kl_type, float lr, float beta1, float beta2, float eps, int t, double* kl_out, void* scratch, void* stream);
int mfvi_elbo_update_guarded_typed(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu, float prior_sigma,
                                   float temp, int kl_type, float lr, float beta1, float beta2, float eps, int32_t* t_applied, const double* loss_d,
                                   const float* loss_f, double* kl_out, void* scratch, void* stream);
int mfvi_elbo_update_bf16_typed(void* mu_bf16, void* rho_bf16, float* bn, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, float prior_mu,
                                float prior_sigma, float temp, int kl_type, float lr, float beta1, float beta2, float eps, int t, uint64_t seed,
                                double* kl_out, void* scratch, void* stream);
/* ---- scale-mixture prior: the Monte-Carlo KL term -------------------------------------------------------------
 * With prior = {'mu': [...], 'sigma': [...], 'pi': [...]} the reference's layers carry p(w) = sum_j pi_j N(w; m_j, sigma_j^2)
 * (MixtureNormal, BayTorch/modules/module.py:32-35, distributions/distributions.py:6-28; the pi as given, not normalised) and, with a
 * kl_type other than 'reverse', estimate KL(q || p) from ONE reparametrised draw per weight (mc_kl_divergence, distributions.py:30-35).
 * Per (mu, rho, eps), s = softplus(rho), w = mu + s eps:
 *     a_j = log pi_j - log sigma_j - (w - m_j)^2 / (2 sigma_j^2)        L = max_j a_j + log sum_j exp(a_j - max)
 *     term = (-eps^2 / 2 - log s) - L        r_j = exp(a_j - L)        G = sum_j r_j (w - m_j) / sigma_j^2
 *     dterm/dmu = G        dterm/drho = (G eps - 1 / s) sigmoid(rho)
 * float32 per element, summed in float64.  The log-sum-exp keeps the term finite where the reference's literal log(sum pi_j exp(..))
 * underflows.  sigma holds the FINAL scales (the reference's prior['sigma'] + 1e-6, rounded to float32).
 * The draw: RNG domain 8 (KLMC), stream 0; element i of the flat MU block is lane i & 3 of Philox block i >> 2; sample = the row of a
 * batch (0 for one fit), step = the iteration's counter word.  Nothing of the rank or of K enters the key.
 * Refused with -1 and mfvi_last_error() before any launch: null pointers, n < 1, i0 < 0, prior->n outside 1..MFVI_MIXTURE_MAX, a pi or
 * sigma that is not finite or not > 0, a 1 / sigma^2 that is not a normal float32, an m that is not finite.
 * The reverse direction against a mixture is not built: the reference's MixtureNormal.rsample (distributions.py:17-22) yields one scalar
 * shared by all weights that is no draw from the mixture. */
#define MFVI_MIXTURE_MAX 4
typedef struct { int32_t n; float pi[MFVI_MIXTURE_MAX], mu[MFVI_MIXTURE_MAX], sigma[MFVI_MIXTURE_MAX]; } mfvi_mixture_prior;
/* The unfused pair on n (mu, rho) pairs that are elements i0 .. i0 + n - 1 of the stream: a layer's slice of the flat block draws what the
 * whole block draws there.  prior: a HOST pointer, copied into the launch.  eps: n normals in device memory to use instead, or NULL to
 * draw.  kl_out (device double) is overwritten; dmu += scale * dterm/dmu, drho += scale * dterm/drho. */
int mfvi_kl_mixture(const float* mu, const float* rho, int64_t n, int64_t i0, const mfvi_mixture_prior* prior, const float* eps, uint64_t seed,
                    uint32_t sample, uint32_t step, double* kl_out, void* stream);
int mfvi_kl_mixture_backward(const float* mu, const float* rho, int64_t n, int64_t i0, const mfvi_mixture_prior* prior, const float* eps, uint64_t seed,
                             uint32_t sample, uint32_t step, float scale, float* dmu, float* drho, void* stream);
/* mfvi_elbo_update / mfvi_elbo_update_guarded with the mixture term in place of the Gaussian KL: the same Adam, partial sums, finish kernel
 * and scratch.  The counter word of the draw is step + (step_dev ? *step_dev : 0), step_dev read on the device (the convention of
 * mfvi_perturb_input_dev), so the device-resident iteration and a captured graph replay with a fresh draw. */
int mfvi_elbo_update_mixture(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, const mfvi_mixture_prior* prior, float temp,
                             float lr, float beta1, float beta2, float eps, int t, uint64_t seed, uint32_t sample, uint32_t step, const int32_t* step_dev,
                             double* kl_out, void* scratch, void* stream);
int mfvi_elbo_update_guarded_mixture(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, const mfvi_mixture_prior* prior,
                                     float temp, float lr, float beta1, float beta2, float eps, int32_t* t_applied, const double* loss_d,
                                     const float* loss_f, uint64_t seed, uint32_t sample, uint32_t step, const int32_t* step_dev, double* kl_out,
                                     void* scratch, void* stream);
int mfvi_adamw_step_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                            const int32_t* t_applied, const double* loss_d, const float* loss_f, float weight_decay, void* stream);
int mfvi_step_advance(int32_t* t_applied, const double* loss_d, const float* loss_f, void* stream);
/* AdamW with decoupled weight decay (the SGLD sibling: bayesian_optimization.py:1765-1766): p *= 1 - lr*weight_decay first */
int mfvi_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, int t, float weight_decay, void* stream);
/* run_inp_dip's loss (bayesian_optimization.py:2824-2826): F.mse_loss(out[:, :3].sigmoid() * mask, img * mask), mean over 3*H*W;
 * out[n][4][H][W], target[3][H][W], mask[mask_channels][H][W] (1 or 3).  Same accumulation / gradient contract as
 * mfvi_gaussian_nll_inpainting (the 4th output channel gets a zero gradient). */
int mfvi_mse_sigmoid_masked(const float* out, const float* target, const float* mask, int mask_channels, int n, int H, int W,
                            float grad_scale, float* dout, double* mse_sum, void* stream);
/* F.mse_loss(out[:, channel], target) of the non-Bayesian siblings (bayesian_optimization.py:1177, 1780; SR :1983-1985 with
 * factor > 1 = the projection out[..., ::f, ::f] first): out[n][C][H][W], target[H/f][W/f]; mse_sum += sum_i mse_i;
 * dout (optional, all C channels written) = grad_scale * d mse_i / d out_i. */
int mfvi_mse_channel(const float* out, const float* target, int n, int C, int H, int W, int channel, int factor, float grad_scale,
                     float* dout, double* mse_sum, void* stream);

/* ---- RNG spec v1 on the device ----------------------------------------------------------------------------- */
/* out[j] = a + b * N(0,1)  (e.g. z = z0 + 0.1*noise uses mfvi_axpy_normal) */
int mfvi_normal_fill(uint64_t seed, uint32_t domain, uint32_t stream_id, uint32_t sample, uint32_t step, int64_t n,
                     float a, float b, float* out, void* stream);
int mfvi_uniform_fill(uint64_t seed, uint32_t stream_id, uint32_t sample, uint32_t step, int64_t n, float scale,
                      float* out, void* stream);
/* out[j] = lo + (hi - lo) * U[0,1)  (RNG domain 3): nn.Conv2d's default kaiming-uniform init of the DIP / SGLD siblings */
int mfvi_uniform_fill_range(uint64_t seed, uint32_t stream_id, uint32_t sample, uint32_t step, int64_t n, float lo, float hi,
                            float* out, void* stream);
/* x[j] += std * N(0,1), RNG domain 4 (SGLD's add_noise on the conv weights: bayesian_optimization.py:166-170) */
int mfvi_add_normal(float* x, uint64_t seed, uint32_t stream_id, uint32_t step, int64_t n, float std, void* stream);
/* net_input = net_input_saved + std * N(0,1)  (bayesian_optimization.py:1363-1364), RNG domain 1 */
int mfvi_perturb_input(const float* z0, uint64_t seed, uint32_t step, int64_t n, float std, float* z, void* stream);
/* the same with the counter word read on the device: step = step_offset + *step_dev (mfvi_plan_set_step_source's convention) */
int mfvi_perturb_input_dev(const float* z0, uint64_t seed, const int32_t* step_dev, uint32_t step_offset, int64_t n, float std, float* z,
                           void* stream);

/* ---- per-iteration bookkeeping (bayesian_optimization.py:1374-1406; utils/common_utils.py:297-353) --------- */
/* acc[0] += mse(a,b) numerator pieces: returns sum (a-b)^2 over n elements into sum_out (device double, overwritten) */
int mfvi_sq_err_sum(const float* a, const float* b, int64_t n, double* sum_out, void* stream);
/* SSIM map mean (11x11 Gaussian sigma 1.5, zero padding) of two [H][W] images; ssim_sum overwritten with the
 * sum of the SSIM map (divide by H*W). */
int mfvi_ssim_sum(const float* a, const float* b, int H, int W, double* ssim_sum, void* stream);
/* dst[h][w] = src[y*factor][x*factor]: the SR runner's nearest-neighbour downsampler (bayesian_optimization.py:2095-2099) applied to the
 * smoothed / clipped outputs for the low-resolution metrics (:2203, :2207, :2214-2217); h = H / factor, w = W / factor. */
int mfvi_decimate(const float* src, int H, int W, int factor, float* dst, void* stream);
/* The anti-aliasing downsampler of models/downsampler.py:6-136 — Downsampler(n_planes, factor, 'lanczos2' | 'lanczos3', phase=0.5,
 * preserve_size=True): ReplicationPad2d(P) (:55-62) then the stride-`factor` convolution with the normalised 2-D kernel of get_kernel
 * (:74-136), which is the outer product of its 1-D taps k1 — applied per plane as dst = A_H . src . A_W^T with
 * A_N[y][clamp(y * factor + i - P, 0, N - 1)] += k1[i], P = (n_taps - factor) / 2.  src [n][C][H][W] -> dst [n][C][H/factor][W/factor];
 * factor 2, 4 or 8 dividing H and W; taps: HOST pointer to the n_taps <= 48 values of k1 (passed to the kernel by value), n_taps - factor
 * even; n, C <= 65535.  Used for the low-resolution target, the SR runner's low-resolution metrics (bayesian_optimization.py:2203, :2207,
 * :2214-2217 with this operator as `downsampler`) and the drop-in module. */
int mfvi_downsample(const float* src, int n, int C, int H, int W, int factor, const float* taps, int n_taps, float* dst, void* stream);
/* Its adjoint (what autograd returns for the module's input, models/downsampler.py:66-72): dsrc [n][C][H][W] = A_H^T . ddst . A_W, every
 * element written, the fold of the replication pad at the borders included.  A gather — no floating-point atomics, a fixed summation order:
 * bit-identical from call to call. */
int mfvi_downsample_adjoint(const float* ddst, int n, int C, int H, int W, int factor, const float* taps, int n_taps, float* dsrc, void* stream);
/* One pass of the runner's per-iteration bookkeeping (bayesian_optimization.py:1374-1396) with no host sync: sample means of
 * out[:,0] and exp(-out[:,1]), EMA (weight w; first = 1 copies), clipped copies for the metrics, ring-buffer slot writes
 * (slot pointers may be NULL).  C = 2 (den/SR) or 1 (CT: no aleatoric channel). */
int mfvi_bookkeep(const float* out, int n, int C, int H, int W, float* ema, float ema_weight, int first, float* out_clip,
                  float* ale_clip, float* avg_clip, float* ring_epi_slot, float* ring_ale_slot, void* stream);
/* The same pass for the inpainting runner (bayesian_optimization.py:3039-3064): out[n][4][H][W] = 3 colour logits + 1 log-precision;
 * m = mean_k sigmoid(out[k][:3]), a = mean_k exp(-out[k][3]); ema[4][HW]; out_clip[3][HW], ale_clip[HW], avg_clip[3][HW] clipped to
 * [0,1]; masked copies (x * mask, mask[mask_channels][HW]) of img, out_clip and avg_clip for the masked PSNR/SSIM; ring slots [3][HW] / [HW]. */
int mfvi_bookkeep_inpainting(const float* out, int n, int H, int W, const float* img, const float* mask, int mask_channels, float* ema,
                             float ema_weight, int first, float* out_clip, float* ale_clip, float* avg_clip, float* img_masked,
                             float* out_masked, float* avg_masked, float* ring_epi_slot, float* ring_ale_slot, void* stream);
/* torch.var(ring, dim=0) (unbiased) / torch.mean(ring, dim=0) over R ring-buffer slots (bayesian_optimization.py:1412-1413) */
int mfvi_ring_stats(const float* ring, int R, int H, int W, float* var_out, float* mean_out, void* stream);
/* post-step output handling: mean[n][HW] kept, out[:,1] <- exp(-out[:,1]); ema = ema*w + out*(1-w) (first: copy) */
int mfvi_post_step(float* out, int n, int C, int H, int W, float* ema, float ema_weight, int first, void* stream);

/* ---- posterior predictive statistics (BayTorch/inference/utils.py:11-24 uncert_regression_gal) ----------- */
/* N draws y_k[C][H][W] of the fitted net map to image channels m_k[c] and an aleatoric variance a_k by `mode`:
 *   MFVI_PRED_RAW        C >= 2: m = y[0..C-2], a = y[C-1]            (uncert_regression_gal's input: the last channel already a variance)
 *   MFVI_PRED_LOGPREC    C == 2: m = y[0], a = exp(-y[1])             (den / SR: bayesian_optimization.py:1376-1377)
 *   MFVI_PRED_INP        C == 4: m = sigmoid(y[0..2]), a = exp(-y[3]) (inpainting: bayesian_optimization.py:3039-3041)
 *   MFVI_PRED_MEAN_ONLY  C == 1: m = y[0], no a                       (CT)
 * clip = 1 clips m_k and a_k to [0, 1] per draw (what the runner's ring stores). */
#define MFVI_PRED_RAW 0
#define MFVI_PRED_LOGPREC 1
#define MFVI_PRED_INP 2
#define MFVI_PRED_MEAN_ONLY 3
/* length in doubles of the accumulator: [sum m (Cimg*H*W) | sum m^2 (Cimg*H*W) | sum a (H*W; not in MEAN_ONLY) | finalize partials];
 * -1 for an invalid (C, mode).  Only the part before the partials carries state between calls (what a K-sharded job all-reduces):
 * (2*Cimg + has_ale)*H*W doubles. */
int64_t mfvi_predictive_acc_doubles(int C, int H, int W, int mode);
/* Fold one chunk out[n][C][H][W] (fp32, contiguous) into the accumulator (uncert_regression_gal's sums over img_list, utils.py:13-16):
 * first = 1 overwrites instead of adding (no zeroing launch).  Every pixel adds its samples in increasing k, so the sums over several
 * calls are bit-identical for any chunking of the same draws.  No atomics. */
int mfvi_predictive_accumulate(const float* out, int n, int C, int H, int W, int mode, int clip, int first, double* acc, void* stream);
/* The maps of utils.py:13-24 from the sums of n_total >= 2 draws (fp32 [H][W] unless noted): mean [Cimg][H][W] = sum m / N;
 * epi = mean over c of the unbiased variance (clamped at >= 0); ale = sum a / N (NULL in MEAN_ONLY); total = ale + epi.  With a ground
 * truth ref [Cimg][H][W] (else NULL): err2 = mean_c (mean[c] - ref[c])^2 and mse_mc = err2 + (N-1)/N * epi, the per-pixel
 * (1/N) sum_k mean_c (m_k[c] - ref[c])^2 of the evaluation notebooks' uceloss input (err2 / mse_mc may be NULL).  sums: 3 device
 * doubles, overwritten with sum ale, sum epi, sum total over the pixels (reduction 'sum'; / (H*W) is 'mean'), reduced in a fixed
 * order (per-block partials in the accumulator's tail, then one block): deterministic. */
int mfvi_predictive_finalize(double* acc, int n_total, int C, int H, int W, int mode, const float* ref, float* mean, float* epi, float* ale,
                             float* total, float* err2, float* mse_mc, double* sums, void* stream);

/* The same statistics for MANY fits in one set of launches: the fit is a grid dimension, each fit's accumulator is a row
 * of acc_stride doubles.  Per fit the maps and sum ale / sum epi / sum total are bit-equal to the single-fit entry points run on that fit's
 * slice of out.  No atomics; bit-identical from call to call.  n_fits and n_fits * S must be below 65536.
 * Length in doubles of ONE fit's accumulator row: the state part first, laid out as mfvi_predictive_acc_doubles describes, then the finalize
 * partials (4 per block); -1 for an invalid (C, mode).  acc_stride may be larger; nothing is written between the rows. */
int64_t mfvi_predictive_acc_doubles_fits(int C, int H, int W, int mode);
/* out[n_fits * S][C][H][W] as a fits-mode mfvi_forward writes it: fit f folds its samples f*S .. f*S + n_use - 1 (1 <= n_use <= S; a partial
 * last chunk leaves the rest unread) into acc + f * acc_stride; first as in mfvi_predictive_accumulate.  One launch whatever n_fits is. */
int mfvi_predictive_accumulate_fits(const float* out, int n_fits, int S, int n_use, int C, int H, int W, int mode, int clip, int first,
                                    double* acc, int64_t acc_stride, void* stream);
/* ref: NULL, or [Cimg][H][W] per fit, ref_stride floats from one fit's to the next (0: one ground truth shared by all fits).
 * mean [n_fits][Cimg][H][W]; epi, ale (NULL in MEAN_ONLY), total, err2, mse_mc (either may be NULL) [n_fits][H][W].  sums: [n_fits][4] device
 * doubles, overwritten with sum ale, sum epi, sum total, sum err2 (of the fp32 values of the maps; the last is 0 without ref), through
 * per-block partials and then one block per fit in block order.  Two launches whatever n_fits is. */
int mfvi_predictive_finalize_fits(double* acc, int64_t acc_stride, int n_fits, int n_total, int C, int H, int W, int mode, const float* ref,
                                  int64_t ref_stride, float* mean, float* epi, float* ale, float* total, float* err2, float* mse_mc, double* sums,
                                  void* stream);

/* ---- uncertainty calibration (utils/uce.py uceloss, the evaluation notebooks' "UCE" cells) ------------------ */
/* Bin k of the n_bins bins given by the n_bins + 1 device floats bounds[] (used as given, non-decreasing) holds the elements with
 * unc > bounds[k] && unc <= bounds[k+1], decided by comparisons only.  An element equal to bounds[0], outside the range or NaN is in no
 * bin but counts in n (uceloss's behaviour).  No floating-point atomics; results are bit-identical from call to call. */
#define MFVI_UCE_MAX_BINS 256
/* bytes of the scratch region of mfvi_uce_bins / mfvi_uce_minmax for n elements; -1 (and mfvi_last_error) for n < 1 or n_bins outside
 * 1..MFVI_UCE_MAX_BINS */
int64_t mfvi_uce_scratch_bytes(int64_t n, int n_bins);
/* minmax[0], minmax[1] = exact fp32 min and max of unc[n], NaN ignored (per-block partials in scratch, then one block) */
int mfvi_uce_minmax(const float* unc, int64_t n, float* minmax, void* scratch, void* stream);
/* Per bin, over err[n] / unc[n] (fp32): count[k] (exact; count[n_bins] = n, so count holds n_bins + 1 words), sums = [n_bins] sum err |
 * [n_bins] sum unc | sum unc over ALL elements (2 n_bins + 1 doubles), and in fp64 rounded once to fp32 prop = count / n,
 * err_in_bin = sum err / count, unc_in_bin = sum unc / count (NaN where count == 0), unc_mean[0] = sum unc / n.
 * Returns -2 for n_bins outside 1..MFVI_UCE_MAX_BINS. */
int mfvi_uce_bins(const float* err, const float* unc, int64_t n, const float* bounds, int n_bins, void* scratch, int64_t* count, double* sums,
                  float* prop, float* err_in_bin, float* unc_in_bin, float* unc_mean, void* stream);
/* uce[0] = sum over the bins with prop > outlier (the fp32 prop against the double, as uceloss compares prop.item()) of
 * |unc_in_bin - err_in_bin| * prop, in bin order */
int mfvi_uce_value(const float* prop, const float* err_in_bin, const float* unc_in_bin, int n_bins, double outlier, float* uce, void* stream);
/* The notebooks' uceloss inputs from a run's arrays: err[i] = mean over the S snapshots rec[S][n] of (rec[s][i] - gt[i])^2 (fp64, rounded
 * once), times mask[i % mask_len] (mask may be NULL); unc[i] = epi[i] + ale[i % ale_len] (fp32; ale may be NULL). */
int mfvi_uce_ring_inputs(const float* rec, int S, int64_t n, const float* gt, const float* mask, int64_t mask_len, const float* epi,
                         const float* ale, int64_t ale_len, float* err, float* unc, void* stream);

/* ---- many independent fits per launch (the plan side is mfvi_plan_set_fits) --------------------------------- */
/* The reference runs its (temp, sigma) candidates and its slices as one process per fit (bayesian_optimization.py:3760-3775, 1328-1372).
 * These entry points run the element-wise passes of one iteration for n_fits fits in ONE launch each, whatever n_fits is; per fit they
 * compute what the single-fit entry point named below computes (the kernels share its per-element code).  n_fits (and n_fits * S) < 65536. */
/* z[f] = z0[f] + std * N(0,1), f < n_fits, n_per_fit floats each: RNG domain 1, stream 0, sample fit0 + f — the numbers of
 * mfvi_normal_fill(seed, 1, 0, fit0 + f, step, ...); fit 0 with fit0 = 0 is mfvi_perturb_input. */
int mfvi_perturb_input_fits(const float* z0, uint64_t seed, uint32_t step, int64_t n_per_fit, int n_fits, uint32_t fit0, float std, float* z,
                            void* stream);
/* mfvi_gaussian_nll per fit: out / dout [n_fits * S][2][H][W], fit f against targets + f * target_stride ([H/factor][W/factor]);
 * nll[f] (device doubles) += sum over the fit's S samples. */
int mfvi_gaussian_nll_fits(const float* out, const float* targets, int64_t target_stride, int n_fits, int S, int H, int W, int factor,
                           float grad_scale, float* dout, double* nll, void* stream);
/* mfvi_elbo_update per fit on rows of params / m / v (param_stride floats apart) and grads (grad_stride), each laid out [MU | RHO | BN],
 * with the fit's own prior, temperature and learning rate read from DEVICE memory.  kl_out[f] (overwritten) is reduced in a fixed order
 * (bit-reproducible; the order of mfvi_elbo_update).  NaN isolation: a fit whose nll[f] is not finite, or whose dead[f] is already set,
 * keeps parameters and moments untouched; a non-finite nll[f] sets dead[f] = 1 (sticky; the caller clears it).  The other fits are unaffected.
 * scratch: mfvi_elbo_update_fits_scratch_bytes(n_fits) bytes. */
typedef struct { float prior_mu, prior_sigma, temp, lr; } mfvi_fit_hyper;
int64_t mfvi_elbo_update_fits_scratch_bytes(int n_fits);
int mfvi_elbo_update_fits(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                          int n_fits, const mfvi_fit_hyper* hyper_dev, float beta1, float beta2, float eps, int t, const double* nll, int32_t* dead,
                          double* kl_out, void* scratch, void* stream);
/* mfvi_elbo_update_fits with the direction of every fit's KL term (BayTorch/modules/module.py:64-80): kl_type_dev[n_fits] in DEVICE memory,
 * MFVI_KL_REVERSE or MFVI_KL_FORWARD per fit, chosen once per block; NULL = all reverse (mfvi_elbo_update_fits itself).  A value outside
 * {0, 1} cannot be refused on the host: that fit is marked dead (dead[f] = 1) and nothing else is written for it, kl_out[f] included. */
int mfvi_elbo_update_fits_typed(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                                int n_fits, const mfvi_fit_hyper* hyper_dev, const int32_t* kl_type_dev, float beta1, float beta2, float eps, int t,
                                const double* nll, int32_t* dead, double* kl_out, void* scratch, void* stream);
/* mfvi_elbo_update_fits_typed with a prior table: mix_dev[n_fits] in DEVICE memory.  A row with n == 0 runs its Gaussian prior of hyper_dev
 * in its direction of kl_type_dev (NULL: reverse), exactly as _typed does; a row with n in 1..MFVI_MIXTURE_MAX runs the mixture term
 * (temp and lr still from hyper_dev; its kl_type entry is not read) and draws with sample sample0 + f and counter word
 * step + (step_dev ? *step_dev : 0).  The choice is made once per block.  mix_dev == NULL calls _typed itself.  A row whose table entry
 * mfvi_kl_mixture would refuse can only be met on the device: it writes nothing and gets dead[f] = 1. */
int mfvi_elbo_update_fits_mixture(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                                  int n_fits, const mfvi_fit_hyper* hyper_dev, const int32_t* kl_type_dev, const mfvi_mixture_prior* mix_dev, uint64_t seed,
                                  uint32_t sample0, uint32_t step, const int32_t* step_dev, float beta1, float beta2, float eps, int t, const double* nll,
                                  int32_t* dead, double* kl_out, void* scratch, void* stream);
/* The EMA part of mfvi_bookkeep per fit: sample means of out[:, 0] and exp(-out[:, 1]) over the fit's S samples (out [n_fits * S][C][H][W],
 * C = 1 or 2) and ema[f] = first ? mean : ema[f] * weight + mean * (1 - weight); ema [n_fits][C][H][W]. */
int mfvi_ema_fits(const float* out, int n_fits, int S, int C, int H, int W, float* ema, float weight, int first, void* stream);
/* Inpainting per fit.  mfvi_gaussian_nll_inpainting per fit: out / dout [n_fits * S][4][H][W], fit f against
 * targets + f * target_stride ([3][H][W]) under masks + f * mask_stride ([mask_channels][H][W], mask_channels 1 or 3; mask_stride 0: one
 * mask for every fit); nll[f] (device doubles) += sum over the fit's S samples; dout may be NULL.  The per-pixel code is
 * mfvi_gaussian_nll_inpainting's own: dout of a fit is bit-equal to that entry point's. */
int mfvi_gaussian_nll_inpainting_fits(const float* out, const float* targets, int64_t target_stride, const float* masks, int64_t mask_stride,
                                      int mask_channels, int n_fits, int S, int H, int W, float grad_scale, float* dout, double* nll, void* stream);
/* The EMA part of mfvi_bookkeep_inpainting per fit: sample means of sigmoid(out[:, c]), c < 3, and of exp(-out[:, 3]) over the fit's S
 * samples (out [n_fits * S][4][H][W]); ema[f] = first ? mean : ema[f] * weight + mean * (1 - weight); ema [n_fits][4][H][W]. */
int mfvi_ema_inpainting_fits(const float* out, int n_fits, int S, int H, int W, float* ema, float weight, int first, void* stream);
/* acc[f] (device doubles, overwritten) = sum over [3][H][W] of (clip(ema_f, 0, 1) * mask_f - img_f * mask_f)^2 with ema_f = ema + f * ema_stride,
 * img_f = img + f * img_stride, mask_f = masks + f * mask_stride ([mask_channels][H][W]; stride 0: shared): the squared error behind the
 * inpainting runner's masked PSNR of the smoothed output.  fp32 per element, fp64 sums; per-block partials in scratch
 * (n_fits * MFVI_MASKED_SQ_ERR_BLOCKS doubles), then one block per fit adds them in block order: no floating-point atomics, bit-identical
 * from call to call.  Two launches whatever n_fits is. */
#define MFVI_MASKED_SQ_ERR_BLOCKS 64
int mfvi_masked_sq_err_fits(const float* ema, int64_t ema_stride, const float* img, int64_t img_stride, const float* masks, int64_t mask_stride,
                            int mask_channels, int n_fits, int H, int W, double* acc, void* scratch, void* stream);

/* mfvi_radon_mse per fit on the plane kernels: out / dout [n_fits * S_per_fit][1][S][S], fit f against the sinogram
 * sinos + f * sino_stride ([T][S]); mse[f] (device doubles) += sum over the fit's samples of mean((R out_k - sino_f)^2),
 * dout_k = grad_scale * d mse_k / d out_k; dout may be NULL (loss only, nothing else is written but scratch).  Three launches whatever
 * n_fits is: mfvi_radon_project's row loop with a residual epilogue (one fp64 partial per block, no atomics), one block per fit that adds
 * the fit's partials in a fixed order, mfvi_radon_backproject of the residual planes.  Bit-identical from call to call.  scratch:
 * mfvi_radon_mse_fits_scratch_bytes(...) bytes, 8-byte aligned.  Null pointers, n_fits * S_per_fit outside 1..65535, S or T outside
 * 1..32768, sino_stride < T * S: -1 and mfvi_last_error(), before any launch (the size query returns -1). */
int64_t mfvi_radon_mse_fits_scratch_bytes(int n_fits, int S_per_fit, int S, int T);
int mfvi_radon_mse_fits(const float* out, const float* sinos, int64_t sino_stride, const float* theta_deg, int n_fits, int S_per_fit, int S, int T,
                        float grad_scale, void* scratch, float* dout, double* mse, void* stream);

/* ---- the non-Bayesian siblings (DIP, MC dropout, SGLD) for many fits per launch ------------------------------- */
/* mfvi_mse_channel per fit: out / dout [n_fits * S][C][H][W], fit f against targets + f * target_stride ([H/factor][W/factor]);
 * mse_acc[f] (device doubles) += sum over the fit's S samples of their mean squared error, summed in fp64 by one block per fit in a fixed
 * order (no atomics: two calls are bit-identical); dout (optional, all C channels written) = grad_scale * d mse / d out.  -1 and a message
 * for target_stride < (H/factor) * (W/factor) and other bad arguments, before any launch. */
int mfvi_mse_channel_fits(const float* out, const float* targets, int64_t target_stride, int n_fits, int S, int C, int H, int W, int channel,
                          int factor, float grad_scale, float* dout, double* mse_acc, void* stream);
/* mfvi_adamw_step (decoupled weight decay) on the MU block [0, n_vi) and the BN block [2 n_vi, 2 n_vi + n_bn) of every fit's row in one
 * launch; the RHO block is neither read nor written.  Per-fit hyper-parameters in DEVICE memory: the update uses (float)lr, as a caller
 * of mfvi_adamw_step passes it.  A fit whose loss_acc[f] is not finite, or whose dead[f] is set, keeps parameters, moments and lr; a
 * non-finite loss_acc[f] sets dead[f] = 1 (sticky).  Behind the update a one-block launch multiplies the lr of every live fit with
 * lr > lr_floor by gamma, in fp64 (ExponentialLR while the rate is above the floor; gamma = 1: a constant rate). */
typedef struct { double lr, gamma; float weight_decay, lr_floor; } mfvi_sibling_hyper;
int mfvi_sibling_update_fits(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride,
                             int64_t grad_stride, int n_fits, mfvi_sibling_hyper* hyper_dev, float beta1, float beta2, float eps, int t,
                             const double* loss_acc, int32_t* dead, void* stream);
/* SGLD's add_noise for every fit in one launch: x[j] = fma(std[f], N(0,1), x[j]) for j in [layer_off[l], layer_off[l] + layer_n[l]) of the
 * row params + f * param_stride, l < n_layers (device tables of int64; the conv weights -- biases and BatchNorm parameters are not listed).
 * RNG: domain 4, stream l, sample fit0 + f, step, element index inside the layer -- fit 0 with fit0 = 0 draws the numbers of
 * mfvi_add_normal(x + layer_off[l], seed, l, step, layer_n[l], ...).  std[f], dead[f] in device memory; dead fits are skipped. */
int mfvi_add_normal_fits(float* params, int64_t param_stride, int n_fits, uint32_t fit0, const int64_t* layer_off, const int64_t* layer_n,
                         int n_layers, uint64_t seed, uint32_t step, const float* std, const int32_t* dead, void* stream);

/* ---- batched bookkeeping: the runner's per-iteration records for many fits per launch ---------------------------- */
/* mfvi_bookkeep per fit in one launch (grid = pixels x fit): out [n_fits * S][C][H][W], ema [n_fits][C][H][W], every map buffer
 * [n_fits][H][W].  Fit f gets exactly what mfvi_bookkeep(out + f S C HW, S, C, H, W, ema + f C HW, ...) writes (the same per-pixel code),
 * so ema is bit-equal to mfvi_ema_fits.  ale_clip / ring_ale are unused (may be NULL) for C = 1; ring_epi / ring_ale may be NULL.  Null
 * out / ema / out_clip / avg_clip, n_fits outside 1..65535, S < 1, C outside 1..2, H or W < 1: -1 and mfvi_last_error(), no launch. */
int mfvi_bookkeep_fits(const float* out, int n_fits, int S, int C, int H, int W, float* ema, float weight, int first, float* out_clip,
                       float* avg_clip, float* ale_clip, float* ring_epi, float* ring_ale, void* stream);
/* Squared-error and SSIM sums of n_pairs pairs of [H][W] maps, x_p = x + p * x_stride, y_p = y + p * y_stride (a stride of 0 shares one
 * map, e.g. a common ground truth).  Both overwritten, no memset, no atomics:
 *   sums[p * sums_stride + 0] = sum (double)((x - y) * (x - y))     difference and product in float, as mfvi_sq_err_sum
 *   sums[p * sums_stride + 1] = sum of the SSIM map                   only with want_ssim (otherwise untouched); the map of mfvi_ssim_sum:
 *                                                                      11-tap sigma 1.5 Gaussian, zero padding 5, C1 = 0.01^2, C2 = 0.03^2
 * One block stages a 16 x 64 tile of a pair with its 5-pixel halo in LDS, filters the five moment planes horizontally then vertically
 * (separable: rounding differs from the 121-tap form of mfvi_ssim_sum by a few 1e-6 of the mean), reduces its two sums in fp64 in a fixed
 * order and writes them to its own slot of scratch; one block per pair then adds the tile partials in index order.  Two launches whatever
 * n_pairs is; bit-identical from call to call; pair p's sums depend neither on n_pairs nor on the other pairs (a NaN stays in its pair).
 * scratch: mfvi_pair_metrics_scratch_bytes(n_pairs, H, W) bytes, 8-byte aligned (0 for arguments mfvi_pair_metrics refuses).  Null
 * pointers, n_pairs outside 1..65535, H or W < 1, a stride between 1 and H W - 1, sums_stride < 1 (2 with want_ssim): -1 and
 * mfvi_last_error(), no launch. */
size_t mfvi_pair_metrics_scratch_bytes(int n_pairs, int H, int W);
int mfvi_pair_metrics(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int n_pairs, int H, int W, int want_ssim,
                      void* scratch, double* sums, int64_t sums_stride, void* stream);

/* ---- total-variation regulariser (utils/sr_utils.py:84-94 tv_loss) ------------------------------------------------- */
/* Per plane x[H][W] and every cell (i < H-1, j < W-1): dh = x[i][j+1] - x[i][j], dw = x[i+1][j] - x[i][j], u = dh^2 + dw^2,
 *   TV_beta(x) = sum over the cells of u^beta                           (a sum, not a mean; beta = 0.5 is the isotropic TV)
 *   dTV/dx[i][j] = g(i,j) (-dh(i,j) - dw(i,j)) + g(i,j-1) dh(i,j-1) + g(i-1,j) dw(i-1,j),        g = 2 beta u^(beta-1)
 * The last row's horizontal and the last column's vertical differences belong to no cell, x[H-1][W-1] has gradient 0, and H == 1 or
 * W == 1 gives 0 and a zero gradient.  ONE DEPARTURE from the reference: for beta < 1 its autograd returns NaN (inf * 0) at every pixel
 * that touches a cell with u == 0; here g = 0 where u == 0.  The value is unaffected.
 * out / dout [n_fits * S][C][H][W]; the term acts on channel `channel` of every sample, fit f owns the samples f S .. f S + S - 1:
 *   dout[:, channel]  = (accumulate ? dout[:, channel] : 0) + grad_scale * weight[f * weight_stride] * dTV/dout     (dout may be NULL)
 *   tv[f]            += sum over the fit's S samples of TV_beta, unweighted                                         (tv may be NULL)
 * weight is read from DEVICE memory (weight_stride 1: one float per fit, 0: one for all): per-fit weights, the upstream gradient of an
 * autograd backward without a host sync, and graph capture.  With accumulate, a fit whose grad_scale * weight is exactly 0 keeps its dout
 * to the bit (nothing is added, not even 0 * NaN).  The other channels of dout are never touched.  The gradient is a gather over
 * the three cells of a pixel in the order above: no atomics, bit-identical from call to call.  The value: fp32 per cell, fp64 sums; each
 * block (a 16 x 64 tile of one plane) writes one partial to its own slot of scratch and a second launch with one block per fit adds the
 * fit's partials in index order (skipped when tv is NULL): no floating-point atomics.  Fit f's results depend neither on n_fits nor on the
 * other fits (a NaN stays in its fit).  beta == 0.5 and beta == 1 take cheap paths (rsqrt / none), any other beta > 0 uses powf.
 * scratch: mfvi_tv_term_scratch_bytes(n_fits, S, H, W) bytes, 8-byte aligned (0 for a shape mfvi_tv_term refuses).  Null out, weight or
 * scratch, dout and tv both NULL, n_fits * S outside 1..65535, channel outside 0..C-1, beta <= 0 or not finite, H or W < 1, weight_stride
 * not 0 or 1: -1 and mfvi_last_error(), no launch. */
size_t mfvi_tv_term_scratch_bytes(int n_fits, int S, int H, int W);
int mfvi_tv_term(const float* out, int n_fits, int S, int C, int H, int W, int channel, float beta, const float* weight, int weight_stride,
                 float grad_scale, int accumulate, float* dout, double* tv, void* scratch, void* stream);

/* ---- signal-to-noise pruning of the fitted posterior (BayTorch/inference/utils.py:104-166 L1UnstructuredFFG / prune_weights_ffg, the SNR
 * histograms of BayTorch/visualize) --------------------------------------------------------------------------------- */
/* Parameter rows are laid out [MU n_vi | RHO n_vi | ...], row r `stride` floats behind row r - 1 (one engine: rows = 1).  Everything below
 * works on the float32 keys key[r][j] = |mu| / softplus(rho) in the total order "unsigned compare of bits(key) & 0x7fffffff, ties by
 * ascending j": the order of the floats with NaN (0 / 0, or a NaN parameter) above +inf, which is the order of a stable argsort of the
 * reference's log(snr) (inference/utils.py:116-123, 139-142).  Group 0 = the convolution weights, group 1 = the biases: the reference ranks them in
 * separate calls (inference/utils.py:159-166).  Membership comes from a DEVICE table of segments sorted by offset; an element in no segment,
 * or in a segment of another group number, is never pruned.  rows in 1..65535; n_vi >= 2^31 is refused (-2).  Integer atomics only and no
 * host round-trip: results are bit-identical from call to call. */
#define MFVI_PRUNE_GROUPS 2
#define MFVI_PRUNE_MAX_SEGMENTS 512
#define MFVI_SNR_MAX_BINS 510
typedef struct { int64_t offset; int64_t count; int32_t group; int32_t pad; } mfvi_prune_segment;
/* keys [rows][n_vi] (dense) = fabsf(mu) / softplus(rho), softplus as torch's (threshold 20), one IEEE division (inference/utils.py:116-118
 * ranks by log(|mu| / softplus(rho)), the same order).  -1 for null pointers, rows outside 1..65535 or stride < 2 n_vi. */
int mfvi_snr_keys(const float* params, int rows, int64_t stride, int64_t n_vi, float* keys, void* stream);
/* bytes of the scratch region of mfvi_snr_select (8-byte aligned); -1 for rows outside 1..65535 */
int64_t mfvi_snr_select_scratch_bytes(int rows);
/* Per row r and group g: mask[r][j] = 0 for the k[r][g] smallest keys of the group in the order above (the reference's
 * mask[argsort(log snr)[:int(amount * n)]] = 0, inference/utils.py:120-123, 139-142), 1 for every other j < n_vi.  k: int64 [rows][2] on the DEVICE, clamped there
 * to 0..the group's size.  threshold[r][g] = bits of the largest pruned key and ties[r][g] = the number of pruned keys equal to it (those of
 * the lowest indices); both 0 where nothing is pruned.  An MSB-first radix select (four digits, LDS histograms, integer atomics), then a
 * count of the threshold's tie class per block and a fixed-order prefix over blocks: 11 small launches on `stream` whatever rows is.
 * -2 for n_vi or n_seg (0..MFVI_PRUNE_MAX_SEGMENTS) out of range, -1 for null pointers, a misaligned scratch or rows outside 1..65535. */
int mfvi_snr_select(const float* keys, int rows, int64_t n_vi, const mfvi_prune_segment* segs, int n_seg, const int64_t* k, uint8_t* mask,
                    uint32_t* threshold, int64_t* ties, void* scratch, void* stream);
/* dst rows = src rows over row_floats floats each (2 n_vi <= row_floats <= stride: the BN tail included), except mu = +0 and
 * rho = -200 (MFVI_PRUNED_RHO of csrc/common.h: softplus(-200) is exactly +0 in every kernel of the library) where mask[r][j] == 0.  The
 * reference multiplies rho by the mask instead (W_rho is pruned like W_mu, inference/utils.py:159-166), leaving sigma = softplus(0) = 0.69 on a "pruned" weight.
 * src is only read; dst == src is refused (-1). */
int mfvi_prune_apply(const float* src, float* dst, const uint8_t* mask, int rows, int64_t stride, int64_t n_vi, int64_t row_floats, void* stream);
/* counts [rows][2][n_bins + 2] (int64, overwritten): per row and group the keys per bin of the n_bins + 1 non-decreasing DEVICE floats
 * bounds[] in key space -- slot s holds the keys with exactly s boundaries <= key (numpy.searchsorted(bounds, key, 'right')): slot 0 is the
 * underflow, slot n_bins + 1 the overflow, where NaN keys count too.  Comparisons only, as mfvi_uce_bins.  -2 for n_bins outside
 * 1..MFVI_SNR_MAX_BINS. */
int mfvi_snr_histogram(const float* keys, int rows, int64_t n_vi, const mfvi_prune_segment* segs, int n_seg, const float* bounds, int n_bins,
                       int64_t* counts, void* stream);

const char* mfvi_last_error(void);
int mfvi_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
