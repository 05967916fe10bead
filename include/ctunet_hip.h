/*
 * ctunet_hip.h -- C ABI of libctunet_hip.so: the MI355X (gfx950) kernels behind the
 * ctunet 3D U-Net hot path.
 *
 * The reference (vfmatzkin/ct-unet) has no FFI of its own: every device operation is a
 * stock torch.nn call inside ctunet/pytorch/models.py, utilities.py and ProblemHandler.py.
 * Each entry point below replaces one such call site (cited per function, paths relative
 * to the reference root).  The host side (ct-unet_amd/ctunet_amd) binds these with ctypes.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch types.  All pointers are DEVICE
 *    pointers unless a parameter says "host".
 *  - Ownership: the library never allocates or frees tensor memory.  Outputs, saved
 *    statistics and workspaces are caller allocations.
 *  - Streams: kernels are enqueued on `stream` (a hipStream_t passed as void*) and the
 *    call returns without synchronising; calls are safe under stream capture.
 *  - Errors: return 0 on success, a negative CTU_E* code otherwise; ctu_last_error()
 *    returns a thread-local message for the last failing call on this thread.
 *  - Activations are fp32, channels-last-3d ("NDHWC") with a CHANNEL STRIDE `cs`
 *    (number of floats between consecutive voxels), so a tensor may be a channel slice
 *    of a wider buffer (the skip-concat buffers).  Channel counts `*_p` are padded to a
 *    multiple of 8; padded channels hold zeros.  Only ctu_ncdhw_to_ndhwc / ctu_head_*
 *    / ctu_loss_* touch the caller-visible NCDHW layout.
 *  - "Lazy BatchNorm": a conv writes its RAW output plus per-block sum / sum-of-squares
 *    partials; ctu_bn_finalize turns those into per-channel scale/shift; every consumer
 *    applies  a = relu(raw*scale + shift)  while loading (`in_scale`,`in_shift`,
 *    `in_relu`; NULL scale = identity).  Raw tensors are what backward re-reads.
 *  - Post-processing (ctu_*_components, ctu_binary_morphology, ctu_distance_transform: exact Euclidean distance, signed
 *    distance and ball morphology in physical units; ctu_local_thickness: the diameter of the largest inscribed ball
 *    through every voxel) works on contiguous label maps [N,D,H,W], each item on its own.
 */
#ifndef CTUNET_HIP_H
#define CTUNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTU_OK 0
#define CTU_EINVAL (-1)   /* bad argument / unsupported shape */
#define CTU_ELAUNCH (-2)  /* HIP launch or runtime error       */

/* storage types of activation tensors: the fp32 entry points take float*; the ctu_lp_* (reduced precision) ones take a
 * dtype code and void* tensors of 16-bit elements (arithmetic stays fp32: MFMA accumulators, BatchNorm statistics,
 * weight gradients, master weights) */
#define CTU_F32 0
#define CTU_BF16 1
#define CTU_F16 2

/* In-launch BatchNorm finalize ("tail"), optional on every entry point that writes BatchNorm partial rows: with a
 * non-NULL tail the block of that launch that finishes last reduces the rows itself and writes what the separate
 * ctu_bn_finalize (forward rows) / ctu_bn_bwd_finalize (backward rows) launch would have written, with the same
 * arithmetic -- one launch less per BatchNorm layer and direction (34 per UNet() train step).  The fields are those
 * calls' arguments.  counter: one zero-initialised 32-bit word in device memory per layer and direction; the tail leaves
 * it zero, so a replayed graph needs no memset.  NULL tail = rows only (finalize with the separate call).
 * Reference: nn.BatchNorm3d in train mode and its autograd (ctunet/pytorch/models.py:27-32,39-44). */
typedef struct ctu_bn_tail {
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;          /* NULL: no running-statistics update */
    float* scale; float* shift; float* mean; float* invstd;
    long long* num_batches_tracked;                   /* NULL: none */
    unsigned int* counter;
    double count;                                     /* N*D*H*W of the normalised tensor */
    float momentum, eps;
    int C, n_updates;
} ctu_bn_tail;
typedef struct ctu_bn_bwd_tail {
    const float* gamma; const float* invstd;
    float* dgamma; float* dbeta; float* coef;         /* coef [5][cp] as ctu_bn_bwd_finalize */
    const float* mean; float* running_mean; float* running_var;   /* the replayed update; NULL running_mean: none */
    long long* num_batches_tracked;
    unsigned int* counter;
    double count;
    float momentum, eps;
    int C;
} ctu_bn_bwd_tail;

const char* ctu_last_error(void);
/* Library/ABI version (bumped on any signature change). */
int ctu_abi_version(void);
/* Name of the code object target this library was compiled for ("gfx950"). */
const char* ctu_arch(void);

/* ---------------------------------------------------------------- layout ---- */
/* NCDHW [N,C,D,H,W] -> NDHWC [N,D,H,W,cs], channels C..cp-1 zero-filled.
 * Host boundary of Model.forward_pass (ctunet/pytorch/Model.py:343-352). */
int ctu_ncdhw_to_ndhwc(const float* src, float* dst, int N, int C, int D, int H, int W,
                       int cp, int cs, void* stream);
/* NDHWC (channel stride cs) -> NCDHW, first C channels. */
int ctu_ndhwc_to_ncdhw(const float* src, float* dst, int N, int C, int D, int H, int W,
                       int cs, void* stream);

/* ------------------------------------------------------- conv3d (k=3 / k=5) ---- */
/* Packed-weight layouts.  0: [8-ch chunk][tap][16-wide out tile][kq][n][j].  1 ("pair", only k = 3 with
 * nout_p = 8): the MFMA N axis carries (w-shift, out channel) and M carries voxel pairs, 36 taps with
 * zero-filled entries -- 1.5x fewer MFMAs than padding 8 channels to 16.  ctu_conv3d_layout returns the
 * layout the forward kernel is fastest with for a volume of width W; pack and forward must agree.
 * Geometry helpers: packed-weight size (floats) and number of spatial blocks (= rows of the
 * stats-partials buffer) of a conv call. */
int ctu_conv3d_layout(int k, int nout_p, int W);
/* Name of the device kernel a ctu_conv3d_fwd / ctu_conv3d_wgrad call with this geometry launches (as it
 * appears in a rocprofv3 kernel trace; thread-local string) -- used to match timings with profiles. */
const char* ctu_conv3d_fwd_kernel_name(int N, int D, int H, int W, int k, int nout_p, int layout);
const char* ctu_conv3d_wgrad_kernel_name(int W, int k, int cin_p, int cout_p);
size_t ctu_conv3d_packed_floats(int k, int rin_p, int nout_p, int layout);
int ctu_conv3d_num_blocks(int N, int D, int H, int W, int k, int nout_p, int layout);

/* Re-layout a torch Conv3d weight [Co,Ci,k,k,k] for the implicit-GEMM kernels.
 *  mode 0 (forward): reduction side = padded input channels, output side = co.
 *  mode 1 (data gradient): reduction side = co, output side = padded input channels, taps flipped.
 * Channel maps (int32, device, NULL = identity) come in two directions throughout this header:
 *   imap[logical channel]   -> position in the padded channels-last buffer
 *   cinv[padded position]   -> logical channel, -1 for a padding slot
 * (the concat buffers hold [C real | pad | C real | pad]).  rin_p / nout_p: padded channel
 * counts of the reduction and output sides of THIS packing (multiples of 8).  Every element of
 * wp is written (padding slots get 0), no prior memset needed.
 * nn.Conv3d weights: ctunet/pytorch/models.py:26,29,38,41,71,76,403,407,430,434,482-488. */
int ctu_pack_conv3d_weight(const float* w, float* wp, int Co, int Ci, int k,
                           const int32_t* cinv, int rin_p, int nout_p, int mode, int layout,
                           void* stream);

/* Every weight tensor of a network in ONE launch (the job table travels in the kernel arguments).
 * jobs: HOST array; kind 0 = Conv3d (ctu_pack_conv3d_weight semantics: w [Co,Ci,k,k,k], k, layout),
 * kind 1 = ConvTranspose3d (ctu_pack_convt_weight semantics: w [Ci,Co,2,2,2]; k/layout ignored). */
typedef struct {
    const float* w;
    float* wp;
    const int32_t* cinv;
    int kind, Co, Ci, k, rin_p, nout_p, mode, layout;
} ctu_pack_job;
int ctu_pack_batch(const ctu_pack_job* jobs, int n, void* stream);

/* Implicit-GEMM 3D convolution on MFMA (v_mfma_f32_16x16x4_f32), stride 1, zero padding
 * (k-1)/2, NDHWC.  out[v, o] = bias[o] + sum_{tap,r} A(in[v+tap, r]) * wp[tap, r, o] with
 * A() the lazy-BN input transform.  Used for nn.Conv3d forward (models.py call sites
 * above) and, with a mode-1 packing, for its data gradient.
 *  in/in_cs/rin_p ...... input tensor, channel stride, channels to contract (mult. of 8)
 *  in_scale/in_shift ... per-channel transform of `in` (NULL = identity); in_relu 0/1
 *  bias/nbias .......... [nbias] (logical, unpadded) or NULL
 *  out/out_cs/nout_p ... output tensor (channel slice base), stride, channels written
 *  stats ............... NULL or [ctu_conv3d_num_blocks()][2][nout_p]: per-block sum and
 *                        sum of squares of the written output (train-mode BatchNorm3d,
 *                        models.py:27,31,39,43,74,79,405,409,432,436,485,490) */
int ctu_conv3d_fwd(const float* in, int in_cs, int rin_p,
                   const float* in_scale, const float* in_shift, int in_relu,
                   const float* wp, const float* bias, int nbias,
                   float* out, int out_cs, int nout_p, float* stats,
                   int N, int D, int H, int W, int k, int layout, const ctu_bn_tail* tail, void* stream);

/* Weight gradient of nn.Conv3d: dW[co,ci,tap] = sum_v A(in[v+tap, pos(ci)]) * gout[v, co],
 * pos = inverse of cinv.
 * ws: workspace of ctu_conv3d_wgrad_ws_floats() floats (per-wave partial slabs, reduced
 * deterministically by a second kernel; no float atomics).  dw: torch layout [Co,Ci,k,k,k].
 * dbias: NULL or [Co] = sum_v gout[v,co]. */
size_t ctu_conv3d_wgrad_ws_floats(int N, int D, int H, int W, int k, int cin_p, int cout_p);
int ctu_conv3d_wgrad(const float* in, int in_cs, int cin_p,
                     const float* in_scale, const float* in_shift, int in_relu,
                     const float* gout, int g_cs, int cout_p,
                     float* dw, float* dbias, int Co, int Ci, const int32_t* cinv,
                     float* ws, int N, int D, int H, int W, int k, void* stream);
/* The same with the BatchNorm3d + ReLU backward of the layer (models.py:27-32, torch autograd) folded in: ga is the
 * gradient w.r.t. the ACTIVATED output, y the layer's raw output (same geometry and channel stride g_cs as ga), bn_scale /
 * bn_shift its ctu_bn_finalize vectors, coef the [5][cout_p] rows of ctu_bn_bwd_finalize.  The kernel forms the raw-output
 * gradient gy while staging ga, uses it for dW and writes it to gy_out (geometry of ga, must not alias it) for the
 * data-gradient call that follows -- the ctu_bn_relu_bwd_apply pass over the layer disappears.  Only for the geometries
 * ctu_conv3d_wgrad_bn_supported accepts (k = 3, volume a multiple of the 4 x 4 x 8|16 box, full channel tiles). */
int ctu_conv3d_wgrad_bn_supported(int N, int D, int H, int W, int k, int cin_p, int cout_p);
int ctu_conv3d_wgrad_bn(const float* in, int in_cs, int cin_p,
                        const float* in_scale, const float* in_shift, int in_relu,
                        const float* ga, int g_cs, int cout_p, const float* y,
                        const float* bn_scale, const float* bn_shift, const float* coef, float* gy_out,
                        float* dw, int Co, int Ci, const int32_t* cinv,
                        float* ws, int N, int D, int H, int W, int k, void* stream);

/* First encoder convolution: C_in = 1 or 2, k = 3, at most 8 output channels (nn.Conv3d(input_channels, i_size, 3),
 * models.py:26 with the channel plan of :175,272-296).  K = 27*C_in is too short for the implicit-GEMM tile and the
 * layer is HBM-bound, so it gets direct kernels that read / write the caller's NCDHW planes in place (no padded
 * channels-last copy of the input):
 *   fwd ....... x [N,cin,D,H,W] (NCDHW) * w [Co,cin,3,3,3] (torch layout, unpacked) -> out channels-last (8 padded
 *               channels, stride out_cs) + one BN partial row [2][8] per block (ctu_conv3d_first_num_blocks rows)
 *   bwd_data .. g channels-last (8 padded channels) -> dx [N,cin,D,H,W] (NCDHW)
 *   wgrad ..... dw [Co,cin,3,3,3]; ws: ctu_conv3d_first_wgrad_ws_floats() floats
 * ctu_conv3d_first_supported tells whether a layer qualifies (k = 3, cin <= 2, nout_p = 8, W >= 16). */
int ctu_conv3d_first_supported(int k, int cin, int nout_p, int W);
int ctu_conv3d_first_num_blocks(int N, int D, int H, int W);
int ctu_conv3d_first_fwd(const float* x, int cin, const float* w, const float* bias, int nbias,
                         float* out, int out_cs, int Co, float* stats,
                         int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream);
int ctu_conv3d_first_bwd_data(const float* g, int g_cs, const float* w, int cin, int Co, float* dx,
                              int N, int D, int H, int W, void* stream);
size_t ctu_conv3d_first_wgrad_ws_floats(int N, int D, int H, int W, int cin);
int ctu_conv3d_first_wgrad(const float* x, int cin, const float* g, int g_cs, float* dw, int Co,
                           float* ws, int N, int D, int H, int W, void* stream);
/* ctu_conv3d_first_wgrad with the layer's BatchNorm + ReLU backward folded in (see ctu_conv3d_wgrad_bn): ga = gradient
 * w.r.t. the ACTIVATED output, y = the raw output, coef = ctu_bn_bwd_finalize's [5][8] rows; the raw-output gradient is
 * written to gy_out (geometry of ga) for ctu_conv3d_first_bwd_data. */
int ctu_conv3d_first_wgrad_bn(const float* x, int cin, const float* ga, int g_cs, const float* y, const float* bn_scale,
                              const float* bn_shift, const float* coef, float* gy_out, float* dw, int Co, float* ws,
                              int N, int D, int H, int W, void* stream);

/* ------------------------------------------------------------ BatchNorm3d ---- */
/* Train mode: reduce the per-block partials written by ctu_conv3d_fwd into batch
 * statistics and the lazy transform.  count = N*D*H*W.  C logical channels, cp padded.
 *  scale = gamma*invstd, shift = beta - mean*scale (0 for padded channels)
 *  running_mean/var updated `n_updates` times with momentum (unbiased var), as
 *  nn.BatchNorm3d does; n_updates = 2 reproduces the double update that
 *  torch.utils.checkpoint causes (models.py:232-255).
 * mean_out/invstd_out [cp] are saved for backward. */
int ctu_bn_finalize(const float* stats, int nblocks, int C, int cp, double count,
                    const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps,
                    int n_updates, float* scale, float* shift, float* mean_out,
                    float* invstd_out, long long* num_batches_tracked, void* stream);
/* (num_batches_tracked: the BatchNorm's int64 counter on the device, += n_updates by the same launch; NULL = none.
 *  ctu_bn_bwd_finalize takes it too and adds 1 when it replays the running-stat update.) */
/* Eval mode: scale/shift from the running statistics. */
int ctu_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, int C, int cp,
                       float* scale, float* shift, void* stream);

/* Backward of  a = relu(bn(y))  for one conv output.
 * Pass 1: partials[nb][2][cp] of  sum(gz)  and  sum(gz * yhat),  gz = ga * (a > 0).
 * Pass 2 (after ctu_bn_bwd_finalize): gy = gamma*invstd*(gz - dbeta/n - yhat*dgamma/n),
 * written IN PLACE over ga.  y/ga are channels-last with strides.  */
int ctu_bn_bwd_num_blocks(int64_t nvox);
int ctu_bn_relu_bwd_reduce(const float* y, int y_cs, const float* ga, int g_cs, int cp,
                           const float* scale, const float* shift, const float* mean,
                           const float* invstd, int64_t nvox, float* partials, const ctu_bn_bwd_tail* tail, void* stream);
/* coef [5][cp]: rows k0 = gamma*invstd, k1 = dbeta/n, k2 = dgamma/n (what ctu_bn_relu_bwd_apply reads) and the same
 * backward as one affine map of the raw output, A = -k0*k2*invstd, B = -k0*(k1 - k2*mean*invstd):
 *     gy = (y*scale + shift > 0 ? k0*ga : 0) + A*y + B
 * (what the weight-gradient kernels of ctu_conv3d_wgrad_bn / ctu_upconv_fused_wgrad_bn apply while staging ga).
 * running_mean/running_var non-NULL: additionally replay the running-statistics update once, with the batch
 * statistics saved by ctu_bn_finalize (mean, invstd) -- the second update torch.utils.checkpoint's recompute
 * performs in backward when use_checkpoint=True (models.py:232-255). */
int ctu_bn_bwd_finalize(const float* partials, int nb, int C, int cp, double count,
                        const float* gamma, const float* invstd,
                        float* dgamma, float* dbeta, float* coef, const float* mean,
                        float* running_mean, float* running_var, float momentum, float eps,
                        long long* num_batches_tracked, void* stream);
int ctu_bn_relu_bwd_apply(const float* y, int y_cs, float* ga, int g_cs, int cp,
                          const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* coef, int64_t nvox, void* stream);

/* ------------------------------------- deferred weight-gradient slab reductions ---- */
/* Nothing reads dW before the optimizer (or a gradient exchange), so the small launch that reduces a weight-gradient
 * kernel's per-block slabs need not sit on the backward chain.  The *_slabs entries below run the weight-gradient kernel
 * exactly as ctu_conv3d_wgrad / ctu_conv3d_wgrad_bn / ctu_conv3d_first_wgrad(_bn) / ctu_convt2_wgrad do (same plan, grid,
 * workspace layout, kernel) and, instead of launching the reduction, describe it in *job (HOST memory).  The caller hands
 * the pending jobs, at most CTU_WGRAD_JOBS_MAX of them, to
 *   ctu_bn_bwd_finalize_jobs ... ctu_bn_bwd_finalize's arguments + jobs: ONE launch whose first cp blocks finalize the
 *                                BatchNorm backward and whose other blocks run the jobs' reductions (the two kinds of
 *                                blocks exchange nothing); njobs = 0: exactly ctu_bn_bwd_finalize
 *   ctu_wgrad_reduce_jobs ...... one launch for the pending jobs alone (njobs = 0: nothing)
 * Every float is the one the immediate entry writes (same kernels' block bodies, same summation order).  Until its job has
 * run, ws must not be written and dw / dbias hold nothing.  A route without a deferred form (k = 5, the generic k = 3
 * kernel, a conv bias gradient, whose channel sum reuses ws) reduces immediately and returns job->kind = 0, which the two
 * calls skip.  The fields are filled by the *_slabs entries and are not meant to be edited. */
#define CTU_WGRAD_JOBS_MAX 4
typedef struct ctu_wgrad_job {
    const float* ws;                                  /* the slabs */
    float* dw; float* db;                             /* db: ConvTranspose bias gradient or NULL */
    const int32_t* cinv;                              /* conv: cinv, ConvTranspose: imap (NULL = identity) */
    int kind;                                         /* 0 = empty */
    int Co, Ci, cin_p, n_ci_g, gx, pairs, nmf;
} ctu_wgrad_job;
int ctu_conv3d_wgrad_slabs(const float* in, int in_cs, int cin_p,
                           const float* in_scale, const float* in_shift, int in_relu,
                           const float* gout, int g_cs, int cout_p,
                           float* dw, float* dbias, int Co, int Ci, const int32_t* cinv,
                           float* ws, int N, int D, int H, int W, int k, ctu_wgrad_job* job, void* stream);
int ctu_conv3d_wgrad_bn_slabs(const float* in, int in_cs, int cin_p,
                              const float* in_scale, const float* in_shift, int in_relu,
                              const float* ga, int g_cs, int cout_p, const float* y,
                              const float* bn_scale, const float* bn_shift, const float* coef, float* gy_out,
                              float* dw, int Co, int Ci, const int32_t* cinv,
                              float* ws, int N, int D, int H, int W, int k, ctu_wgrad_job* job, void* stream);
int ctu_conv3d_first_wgrad_slabs(const float* x, int cin, const float* g, int g_cs, float* dw, int Co,
                                 float* ws, int N, int D, int H, int W, ctu_wgrad_job* job, void* stream);
int ctu_conv3d_first_wgrad_bn_slabs(const float* x, int cin, const float* ga, int g_cs, const float* y, const float* bn_scale,
                                    const float* bn_shift, const float* coef, float* gy_out, float* dw, int Co, float* ws,
                                    int N, int D, int H, int W, ctu_wgrad_job* job, void* stream);
int ctu_convt2_wgrad_slabs(const float* in, int in_cs, int cin_p, const float* in_scale,
                           const float* in_shift, int in_relu, const float* gout, int g_cs,
                           int cout_p, float* dw, float* dbias, int Ci, int Co,
                           const int32_t* imap, float* ws, int N, int D, int H, int W, ctu_wgrad_job* job, void* stream);
int ctu_bn_bwd_finalize_jobs(const float* partials, int nb, int C, int cp, double count,
                             const float* gamma, const float* invstd,
                             float* dgamma, float* dbeta, float* coef, const float* mean,
                             float* running_mean, float* running_var, float momentum, float eps,
                             long long* num_batches_tracked, const ctu_wgrad_job* jobs, int njobs, void* stream);
int ctu_wgrad_reduce_jobs(const ctu_wgrad_job* jobs, int njobs, void* stream);

/* -------------------------------------------------------------- MaxPool3d ---- */
/* nn.MaxPool3d(2, stride 2) (models.py:190-191,233,469-470) of a = A(in); writes the
 * pooled ACTIVATED values (no transform needed downstream). */
int ctu_maxpool2_fwd(const float* in, int in_cs, int cp, const float* in_scale,
                     const float* in_shift, int in_relu, float* out, int out_cs,
                     int N, int D, int H, int W, void* stream);
/* Backward: routes gout (pooled grid) to the first max of each 2x2x2 window of A(in)
 * (recomputed, no stored indices) and ADDS it into gin (full grid, stride gin_cs). */
int ctu_maxpool2_bwd(const float* in, int in_cs, int cp, const float* in_scale,
                     const float* in_shift, int in_relu, const float* gout, int gout_cs,
                     float* gin, int gin_cs, int accumulate, int N, int D, int H, int W,
                     void* stream);
/* The same, when in is the raw output of a conv whose train-mode BatchNorm + ReLU (in_scale/in_shift, mean/invstd) the
 * pooled tensor is, and gin is complete after this call (the reference's encoder: pool(block(x)), models.py:233-246,
 * with the skip's share already in gin): also emits that BatchNorm's backward reduction -- one row {sum gz[c], sum
 * gz[c]*xhat[c]} per block, ctu_maxpool2_bwd_bn_num_blocks rows of 2*cp floats, consumed by ctu_bn_bwd_finalize in place
 * of ctu_bn_relu_bwd_reduce's rows (saves one pass over y and the gradient).  ctu_maxpool2_bwd_bn_num_blocks returns 0
 * for channel counts the fused form does not take (cp/4 must divide 256): use ctu_maxpool2_bwd + the separate reduce. */
int ctu_maxpool2_bwd_bn_num_blocks(int N, int D, int H, int W, int cp);
int ctu_maxpool2_bwd_bn(const float* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                        const float* mean, const float* invstd, const float* gout, int gout_cs, float* gin,
                        int gin_cs, int accumulate, int N, int D, int H, int W, float* partials, const ctu_bn_bwd_tail* tail, void* stream);

/* -------------------------------------------------- ConvTranspose3d k2 s2 ---- */
/* nn.ConvTranspose3d(C, C, 2, 2) with bias (models.py:37,427-429):
 * out[2v+tap, o] = b[o] + sum_r A(in[v, r]) * w[r, o, tap];  w torch layout [Ci,Co,2,2,2].
 * Packing: mode 0 forward (reduction = padded input channels, output = co),
 *          mode 1 data gradient (reduction = co, output = padded input channels); cinv as above. */
size_t ctu_convt_packed_floats(int rin_p, int nout_p);
int ctu_pack_convt_weight(const float* w, float* wp, int Ci, int Co, const int32_t* cinv,
                          int rin_p, int nout_p, int mode, void* stream);
int ctu_convt2_fwd(const float* in, int in_cs, int rin_p, const float* in_scale,
                   const float* in_shift, int in_relu, const float* wp, const float* bias,
                   int nbias, float* out, int out_cs, int nout_p, int N, int D, int H, int W,
                   void* stream);      /* D,H,W: INPUT grid; output grid is 2D,2H,2W */
/* gin[v, r] = sum_{tap,o} gout[2v+tap, o] * w[r, o, tap]  (wp from mode 1). */
int ctu_convt2_bwd_data(const float* gout, int g_cs, int rout_p, const float* wp,
                        float* gin, int gin_cs, int nin_p, int N, int D, int H, int W,
                        void* stream);
/* dw[ci,co,tap] = sum_v A(in[v, imap[ci]]) * gout[2v+tap, co];  dbias[co] = sum gout. */
size_t ctu_convt2_wgrad_ws_floats(int N, int D, int H, int W, int cin_p, int cout_p);
int ctu_convt2_wgrad(const float* in, int in_cs, int cin_p, const float* in_scale,
                     const float* in_shift, int in_relu, const float* gout, int g_cs,
                     int cout_p, float* dw, float* dbias, int Ci, int Co,
                     const int32_t* imap, float* ws, int N, int D, int H, int W, void* stream);
/* Launch plans (host only, no GPU needed; the launchers read the same plan functions).  Each returns the kernel
 * instantiation a call of this geometry launches, e.g. "convt2_kernel<4, 0>", or NULL for a geometry the call refuses,
 * and fills plan[] when it is not NULL.  mode 0 forward, 1 data gradient (rin_p = the reduction side).
 *  ctu_convt2_plan ......... plan[4] = grid.x, grid.y, taps staged per barrier pair, dynamic LDS bytes
 *  ctu_convt2_wgrad_plan ... plan[3] = grid.x (slabs per channel group), grid.y, 64-voxel tiles the grid.x blocks share */
const char* ctu_convt2_plan(int mode, int rin_p, int nout_p, int N, int D, int H, int W, int* plan);
const char* ctu_convt2_wgrad_plan(int cin_p, int cout_p, int N, int D, int H, int W, int* plan);

/* ------------------------------------------------------------------- head ---- */
/* last_conv 1x1x1 + bias, optional softmax(dim=1), optional sigmoid, optional SP
 * re-encoding, written NCDHW (models.py:223-224,255-259,317-330,364-365,507,538).
 *  w [Co,Ci] torch layout, imap as above, act: bit0 softmax, bit1 sigmoid.  Co <= 4.
 *  head_mode 0: out0 = y [N,Co,...].
 *  head_mode 1 (UNetSP/UNetDO): out0 = [y0, y1+y2], out1 = [1-y1, y1]  (Co must be 3).
 *  head_mode 2 (UNetSPSmall): mode 1 followed by softmax of each pair. */
int ctu_head_fwd(const float* in, int in_cs, int cin_p, const float* in_scale,
                 const float* in_shift, int in_relu, const float* w, const float* bias,
                 const int32_t* imap, int Ci, int Co, int act, int head_mode,
                 float* out0, float* out1, int N, int64_t nvox_per_item, void* stream);
/* Backward of the head; the forward values are recomputed from `in` (nothing saved).
 * g0/g1: gradients of out0/out1 (NCDHW, g1 NULL for mode 0).  Produces gin (channels-last,
 * stride gin_cs, cin_p channels = gradient w.r.t. the ACTIVATED input), dw [Co,Ci], db [Co].
 * ws: workspace of ctu_head_bwd_ws_floats() floats. */
size_t ctu_head_bwd_ws_floats(int N, int64_t nvox_per_item, int cin_p, int Co);
int ctu_head_bwd(const float* in, int in_cs, int cin_p, const float* in_scale,
                 const float* in_shift, int in_relu, const float* w, const float* bias,
                 const int32_t* imap, int Ci, int Co, int act, int head_mode,
                 const float* g0, const float* g1, float* gin, int gin_cs,
                 float* dw, float* db, float* ws, int N, int64_t nvox_per_item, void* stream);
/* The same, when the first bn_cp input channels are the train-mode BatchNorm + ReLU output of one conv (in_scale/in_shift,
 * bn_mean/bn_invstd) and nothing else consumes that tensor (the decoder's last block feeding the head, models.py:252-255):
 * also emits that BatchNorm's backward reduction, ctu_head_bwd_num_blocks rows of 2*bn_cp floats {sum gz, sum gz*xhat},
 * consumed by ctu_bn_bwd_finalize in place of ctu_bn_relu_bwd_reduce's rows. */
int ctu_head_bwd_num_blocks(int N, int64_t nvox_per_item);
int ctu_head_bwd_bn(const float* in, int in_cs, int cin_p, const float* in_scale,
                    const float* in_shift, int in_relu, const float* w, const float* bias,
                    const int32_t* imap, int Ci, int Co, int act, int head_mode,
                    const float* g0, const float* g1, float* gin, int gin_cs,
                    float* dw, float* db, float* ws, int N, int64_t nvox_per_item,
                    const float* bn_mean, const float* bn_invstd, int bn_cp, float* bn_partials, const ctu_bn_bwd_tail* tail, void* stream);
/* Two-segment forms: the head's 2*cp padded input channels live in two buffers, (in_a, cs_a) holding channels [0, cp) and
 * (in_b, cs_b) holding [cp, 2*cp); the input gradient is written the same way to (gin_a, gcs_a) / (gin_b, gcs_b).  cp is
 * 4, 8 or 16.  Everything else -- in_scale / in_shift [2*cp], w, imap (values in [0, 2*cp)), ws (sized for cin_p = 2*cp),
 * dw, db, the BatchNorm rows and tail -- is what the one-buffer entry takes with cin_p = 2*cp, and every output is bit for
 * bit what that entry writes for the same values (same loads per lane, same arithmetic, same reduction order).
 * ctu_head_bwd_bn_seg2 with bn_partials NULL is the plain head backward.
 * Refused before any launch (CTU_EINVAL): a null segment, a segment that is not 16-byte aligned, a stride below cp or not a
 * multiple of 4, cp outside {4, 8, 16}, and whatever the one-buffer entries refuse. */
int ctu_head_fwd_seg2(const float* in_a, int cs_a, const float* in_b, int cs_b, int cp, const float* in_scale,
                      const float* in_shift, int in_relu, const float* w, const float* bias, const int32_t* imap,
                      int Ci, int Co, int act, int head_mode, float* out0, float* out1, int N,
                      int64_t nvox_per_item, void* stream);
int ctu_head_bwd_bn_seg2(const float* in_a, int cs_a, const float* in_b, int cs_b, int cp, const float* in_scale,
                         const float* in_shift, int in_relu, const float* w, const float* bias, const int32_t* imap,
                         int Ci, int Co, int act, int head_mode, const float* g0, const float* g1, float* gin_a,
                         int gcs_a, float* gin_b, int gcs_b, float* dw, float* db, float* ws, int N,
                         int64_t nvox_per_item, const float* bn_mean, const float* bn_invstd, int bn_cp,
                         float* bn_partials, const ctu_bn_bwd_tail* tail, void* stream);

/* ------------------------------------------------------------------- loss ---- */
/* Fused Dice + cross-entropy on one 2-channel NCDHW map (utilities.py:35-50,
 * ProblemHandler.py:59-88,228-298).  pred/target [N,2,V].
 *  ce term   = ce_lambda   * CrossEntropy(pred as logits, argmax(target,1)), mean over N*V
 *  dice term = dice_lambda * dice_loss(P, target), P = softmax(pred,1) if dice_softmax else pred
 * terms (device, float[2]) = {ce term, dice term}.  ws: ctu_loss_ws_floats(N, V) floats,
 * kept until ctu_loss_bwd, which writes
 *   gpred = gscale_ce[0] * d(ce term)/dpred + gscale_dice[0] * d(dice term)/dpred
 * (gscale_*: one device float each -- the two upstream gradients autograd hands over, read in place; NULL = 1;
 *  accumulate != 0: gpred += ). */
size_t ctu_loss_ws_floats(int N, int64_t V);
int ctu_loss_fwd(const float* pred, const float* target, int N, int64_t V, float ce_lambda,
                 float dice_lambda, int dice_softmax, float* terms, float* ws, void* stream);
int ctu_loss_bwd(const float* pred, const float* target, int N, int64_t V, float ce_lambda,
                 float dice_lambda, int dice_softmax, const float* ws, const float* gscale_ce,
                 const float* gscale_dice, float* gpred, int accumulate, void* stream);

/* Loss family on the same 2-channel map (csrc/loss_family.hip): class-weighted / focal cross-entropy, the Dice term
 * above, a Tversky term on the foreground channel and a boundary term over a signed distance map.  With c the target
 * class of a voxel (1 where t1 > t0, else 0), p = softmax(pred), P as above, q = P[:,1], g = target[:,1], eps = 1e-7:
 *  ce term       = ce_lambda * sum w_c (1 - p_c)^focal_gamma (-log p_c) / sum w_c, over all N*V voxels
 *  dice term     = as ctu_loss_fwd
 *  tversky term  = tversky_lambda * (1 - mean_n (TP + eps) / (TP + alpha FP + beta FN + eps)),
 *                  TP = sum q g, FP = sum q - TP, FN = sum g - TP per item
 *  boundary term = boundary_lambda * sum q phi / (N V); phi [N,V] float32 (positive outside the object, negative
 *                  inside), a non-finite entry counts as 0.  phi may be NULL when boundary_lambda == 0 (it is not read then).
 * terms (device, float[4]) in that order; a term whose lambda is 0 is 0 and gets no gradient.  ws: ctu_seg_loss_ws_floats
 * floats, 16-byte aligned, kept until ctu_seg_loss_bwd, which writes the sum of the four terms' gradients, each times its
 * upstream gradient g_* (one device float, read in place; NULL = 1); accumulate != 0: gpred +=.
 * Refused: N <= 0, V <= 0, w <= 0, focal_gamma < 0, alpha or beta < 0, a missing required pointer. */
typedef struct ctu_seg_loss_cfg {
    float ce_lambda, dice_lambda, tversky_lambda, boundary_lambda;
    float w0, w1;            /* class weights of the cross-entropy */
    float focal_gamma;
    float tversky_alpha, tversky_beta;
    int dice_softmax;
} ctu_seg_loss_cfg;
size_t ctu_seg_loss_ws_floats(int N, int64_t V);
int ctu_seg_loss_fwd(const float* pred, const float* target, const float* phi, int N, int64_t V,
                     const ctu_seg_loss_cfg* cfg, float* terms, float* ws, void* stream);
int ctu_seg_loss_bwd(const float* pred, const float* target, const float* phi, int N, int64_t V,
                     const ctu_seg_loss_cfg* cfg, const float* ws, const float* g_ce, const float* g_dice,
                     const float* g_tversky, const float* g_boundary, float* gpred, int accumulate, void* stream);

/* -------------------------------------------------------------- utilities ---- */
/* Additive skip connection, UNet(cat=False): out = act_a(a) + act_b(b) on channels-last tensors, where act_x is the
 * lazy BatchNorm(+ReLU) transform of that operand (scale/shift NULL: identity).  b == NULL: out = act_a(a), which is
 * also the strided channel-slice copy the backward of the add uses (/root/reference/ctunet/pytorch/models.py:250-251). */
int ctu_skip_add(const float* a, int a_cs, const float* a_scale, const float* a_shift, int a_relu,
                 const float* b, int b_cs, const float* b_scale, const float* b_shift, int b_relu,
                 float* out, int out_cs, int cp, int64_t nvox, void* stream);
/* ------------------------------------------- fused up-convolution (decoder) ---- */
/* ConvTranspose3d(C, C, 2, 2, bias) followed by Conv3d(C, Co, 3, padding 1, no bias) -- the first two layers of
 * every decoder block (/root/reference/ctunet/pytorch/models.py:37-38) -- as ONE convolution on the coarse grid:
 * per output parity a 2x2x2 convolution with composite weights W_eff = WT o W3 and a bias that only differs on the
 * volume faces (27 border classes).  Same result as the two layers up to fp32 summation order; 8 taps instead of
 * 27 + the transposed conv, and the fine-grid intermediate is never materialised.
 *   ctu_upconv_fused_pack: wt [C][C][2][2][2], bt [C], w3 [Co][C][3][3][3] (torch layouts) -> wp (packed_floats)
 *     and beff [27][nout_p]; cinv maps padded input positions to logical channels (concat layout), NULL = identity;
 *     ws = pack_ws_floats scratch (transposed copies of the two weight tensors).
 *   ctu_upconv_fused_pack_all: the same plus wpd (ctu_upconv_fused_pack_bwd's data-gradient packing, bwd_packed_floats; NULL =
 *     none) in three launches -- transposes, composite weights + beff, gathers (PW packing + wpd).  Every element of every
 *     output is written on every call.
 *   ctu_upconv_fused_fwd: in = COARSE activations [N,D,H,W,in_cs] with the lazy BatchNorm transform, out = RAW
 *     fine-grid output [N,2D,2H,2W,out_cs]; stats = num_blocks rows of [2][nout_p] partial sums for ctu_bn_finalize. */
int ctu_upconv_fused_supported(int k, int D, int H, int W, int cin_p, int nout_p);
size_t ctu_upconv_fused_packed_floats(int cin_p, int nout_p);
int ctu_upconv_fused_num_blocks(int N, int D, int H, int W, int nout_p);
size_t ctu_upconv_fused_pack_ws_floats(int C, int nout_p);
int ctu_upconv_fused_pack(const float* wt, const float* bt, const float* w3, int C, int Co, const int32_t* cinv,
                          int cin_p, int nout_p, float* wp, float* beff, float* ws, void* stream);
int ctu_upconv_fused_pack_all(const float* wt, const float* bt, const float* w3, int C, int Co, const int32_t* cinv,
                              int cin_p, int nout_p, float* wp, float* beff, float* ws, float* wpd, void* stream);
int ctu_upconv_fused_fwd(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                         int in_relu, const float* wp, const float* beff, float* out, int out_cs, int nout_p,
                         float* stats, int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream);

/* Backward of the fused up-convolution w.r.t. the three parameter tensors (its data gradient: ctu_upconv_fused_bwd_data
 * below).  ctu_upconv_fused_wgrad: dweff [8 parities][8 taps][cin_p][nout_p] = sum_i x[i+d]^T dy[2i+p]
 * (in = COARSE activations with the lazy transform, gout = fine-grid gradient of the fused op's raw output).
 * ctu_upconv_fused_project: dWT, dbT, dW3 (torch layouts) from dweff and the border-aware sums of gout; pack_ws is
 * the scratch ctu_upconv_fused_pack filled in this step's forward, imap maps logical input channels to padded positions. */
size_t ctu_upconv_fused_wgrad_ws_floats(int N, int D, int H, int W, int cin_p, int nout_p);
int ctu_upconv_fused_wgrad(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                           int in_relu, const float* gout, int g_cs, int nout_p, float* dweff, float* ws,
                           int N, int D, int H, int W, void* stream);
/* ctu_upconv_fused_wgrad with the BatchNorm + ReLU backward of the fused op's output folded in (as ctu_conv3d_wgrad_bn):
 * ga = fine-grid gradient w.r.t. the ACTIVATED output, y = the fused op's raw output, gy_out = the raw-output gradient the
 * ctu_upconv_fused_project and ctu_upconv_fused_bwd_data calls that follow read.  N, D, H, W: COARSE dims. */
int ctu_upconv_fused_wgrad_bn_supported(int N, int D, int H, int W, int cin_p, int nout_p);
int ctu_upconv_fused_wgrad_bn(const float* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                              int in_relu, const float* ga, int g_cs, int nout_p, const float* y,
                              const float* bn_scale, const float* bn_shift, const float* coef, float* gy_out,
                              float* dweff, float* ws, int N, int D, int H, int W, void* stream);
size_t ctu_upconv_fused_project_ws_floats(int nout_p, int64_t fine_nvox);
int ctu_upconv_fused_project(const float* dweff, const float* gout, int g_cs, int nout_p, int N, int D, int H, int W,
                             const float* bt, const float* pack_ws, const int32_t* imap, int C, int Co, int cin_p,
                             float* dwt, float* dbt, float* dw3, float* ws, void* stream);

/* Data gradient of the fused up-convolution: gin (COARSE, [N,D,H,W,gin_cs], cin_p padded channels in the input's
 * layout) from gout (fine grid, gradient of the raw output) -- the adjoint parity convolutions, no fine-grid
 * intermediate.  wpd = ctu_upconv_fused_pack_bwd(wp): the forward packing re-gathered for the transposed product. */
size_t ctu_upconv_fused_bwd_packed_floats(int cin_p, int nout_p);
int ctu_upconv_fused_pack_bwd(const float* wp, int cin_p, int nout_p, float* wpd, void* stream);
int ctu_upconv_fused_bwd_data(const float* gout, int g_cs, int nout_p, const float* wpd, float* gin, int gin_cs,
                              int cin_p, int N, int D, int H, int W, void* stream);

/* Two-segment forms of the four entries that touch a whole COARSE voxel: its cin_p padded channels live in two buffers of
 * the same voxel stride cs, (in0, cs) holding channels [0, seg_c) and (in1, cs) holding [seg_c, cin_p), seg_c = cin_p / 2
 * (the two dense halves of a concat level); ctu_upconv_fused_bwd_data_seg2 writes the coarse gradient the same way.
 * Everything else -- in_scale / in_shift [cin_p], the packed weights, channel maps, partial rows, workspaces, dweff, gy_out --
 * is what the one-buffer entry takes, and every output is bit for bit what that entry writes for the same values: an
 * 8-channel chunk of the forward and a 16-channel tile of the two gradients lie in one segment, so the kernels only pick a
 * base pointer per chunk / tile; loads, arithmetic and summation order are unchanged.
 * Refused before any launch (CTU_EINVAL): a null segment, a segment that is not 16-byte aligned, cs < seg_c or not a
 * multiple of 4, 2 * seg_c != cin_p, seg_c not a multiple of 8 (forward) or 16 (weight and data gradient), and whatever
 * the one-buffer entries refuse.  ctu_upconv_fused_seg2_supported: all four entries take this geometry. */
int ctu_upconv_fused_seg2_supported(int k, int D, int H, int W, int cin_p, int nout_p, int seg_c);
int ctu_upconv_fused_fwd_seg2(const float* in0, const float* in1, int seg_c, int cs, int cin_p, const float* in_scale,
                              const float* in_shift, int in_relu, const float* wp, const float* beff, float* out, int out_cs,
                              int nout_p, float* stats, int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream);
int ctu_upconv_fused_wgrad_seg2(const float* in0, const float* in1, int seg_c, int cs, int cin_p, const float* in_scale,
                                const float* in_shift, int in_relu, const float* gout, int g_cs, int nout_p, float* dweff,
                                float* ws, int N, int D, int H, int W, void* stream);
int ctu_upconv_fused_wgrad_bn_seg2(const float* in0, const float* in1, int seg_c, int cs, int cin_p, const float* in_scale,
                                   const float* in_shift, int in_relu, const float* ga, int g_cs, int nout_p, const float* y,
                                   const float* bn_scale, const float* bn_shift, const float* coef, float* gy_out,
                                   float* dweff, float* ws, int N, int D, int H, int W, void* stream);
int ctu_upconv_fused_bwd_data_seg2(const float* gout, int g_cs, int nout_p, const float* wpd, float* gin0, float* gin1,
                                   int seg_c, int cs, int cin_p, int N, int D, int H, int W, void* stream);

/* -------------------------------------------------- inference tail / sample schema ---- */
/* hard_segm_from_tensor (/root/reference/ctunet/utilities.py:103-124): seg[n,v] = (float)argmax_c prob[n,c,v] over an
 * NCDHW map; the first maximum wins (torch.argmax). */
int ctu_hard_segm(const float* prob, int N, int C, int64_t nvox_per_item, float* seg, void* stream);
/* one_hot(label.long(), C).movedim(-1, 1).float() of the reference datasets (ctunet/pytorch/datasets.py:107-110,
 * 212-217): label [N,V] float -> out [N,C,V].  Labels outside [0,C) give an all-zero voxel (torch raises). */
int ctu_one_hot(const float* label, int N, int C, int64_t nvox_per_item, float* out, void* stream);
/* dice_coeff (ctunet/utilities.py:53-59 = monai compute_meandice on one_hot(argmax(pred,1))): counts[n][c] =
 * { sum hard_c*target_c, sum hard_c, sum target_c } in double (exact integers for one-hot targets), two-stage
 * fixed-order reduction.  C <= 8.  The Dice ratio itself (and the empty-vs-empty convention) is the caller's. */
size_t ctu_hard_dice_ws_doubles(int N);
int ctu_hard_dice_counts(const float* pred, const float* target, int N, int C, int64_t nvox_per_item,
                         double* counts, double* ws, void* stream);

/* hausdorff (ctunet/utilities.py:62-70 = monai compute_hausdorff_distance on one_hot(argmax(pred,1)), background
 * excluded, Euclidean, symmetric, no percentile): out[n][c-1], c = 1..C-1 = max over the surface voxels of either set of
 * the distance to the other set's surface; surface = mask & ~erode(mask) (6-neighbourhood, background outside the
 * volume); the distances come from an exact integer squared-distance transform.  NaN where either surface is empty (the
 * caller maps it, utilities.py:69).  A composition: ctu_hard_segm(pred) into a float label map, ctu_surface_metrics of it
 * against the one-hot target at unit spacing, the HD row copied to out; no host sync, capture-safe.  pred / target
 * [N,C,D,H,W], C in 2..8, every side <= 1024, N*(C-1)*2 <= 65535; ws: ctu_hausdorff_ws_bytes() bytes (the label map, 4
 * bytes per voxel per item, and ctu_surface_ws_bytes).  PARITY UNPINNED (monai is not in the reference tree); tested
 * against the same definition on scipy.ndimage. */
size_t ctu_hausdorff_ws_bytes(int N, int C, int D, int H, int W);
int ctu_hausdorff(const float* pred, const float* target, int N, int C, int D, int H, int W, float* out, void* ws,
                  void* stream);

/* Surface-distance metrics with voxel spacing (no reference counterpart: ctunet/utilities.py:62-70 has only the voxel-unit
 * maximum, ctu_hausdorff above, which is one row of these; definitions pinned in ctunet_amd/metrics.py).  One (item n,
 * class c) pair per scored class c = cls0 .. cls0+Cs-1 of each item; per side the mask is p[n][c] != 0 for a one-hot tensor
 * [N,C,D,H,W] (onehot = 1) or p[n] == c for a label map [N,D,H,W] (onehot = 0); dtype CTU_U8, CTU_I64 or CTU_F32 per side.
 * spacing: HOST float [N][3] (z, y, x spacing of each item; NULL = unit: exact int32 squared distances), tau: HOST double
 * [Cs] surface-Dice tolerances (NULL: no NSD), percentile in [0, 100] (< 0: none).  out: DEVICE float [8][N*Cs], row r of
 * pair n*Cs + (c-cls0): 0 hard Dice, 1 HD, 2 directed HD (P->G), 3 HD_p, 4 directed HD_p, 5 ASSD (symmetric),
 * 6 directed ASD (mean P->G), 7 NSD.  NaN where undefined (empty surface, no percentile, no tau).
 * ws: ctu_surface_ws_bytes() bytes (pairs processed in groups; about 5 bytes per voxel per plane).  Deterministic, no
 * host sync, capture-safe.  Cs <= 16, every side <= 1024. */
#define CTU_U8 3
#define CTU_I64 4
size_t ctu_surface_ws_bytes(int N, int Cs, int D, int H, int W);
int ctu_surface_metrics(const void* pred, int pred_dtype, int pred_onehot, const void* target, int target_dtype,
                        int target_onehot, int N, int C, int cls0, int Cs, int D, int H, int W, const float* spacing,
                        const double* tau, double percentile, float* out, void* ws, void* stream);

/* Connected components of label maps (no reference counterpart; definitions pinned in ctunet_amd/postprocess.py).
 * in: DEVICE label map [N,D,H,W] of dtype CTU_U8 or CTU_I64.  A voxel is foreground if its label is nonzero and, when
 * n_applied > 0, in the HOST list applied[n_applied] (1..16 distinct nonzero labels).  Two neighbours are connected iff
 * both are foreground and carry the same label; connectivity 1 / 2 / 3 = 6 / 18 / 26 neighbours (scipy's rank), nothing
 * across the border.  A component's root is its first voxel in C order.
 *   label:  labels (DEVICE int32 [N,D,H,W], may be NULL) = 1 + rank of the component's root in C order per item, 0 for
 *           background (scipy.ndimage.label's numbering); num: DEVICE int32 [N] = components per item.
 *   filter: out (DEVICE, the input dtype, may alias in) = in, except foreground voxels of dropped components, which are 0.
 *           mode CTU_CC_LARGEST: per (item, class) keep the param (1..8) largest components, ties to the earlier root;
 *           the classes are the applied labels, or with n_applied = 0 the labels 1..255 (other labels are never dropped).
 *           mode CTU_CC_MIN_SIZE: keep a component iff its voxel count >= param (>= 0).
 * ws: ctu_components_ws_bytes() bytes (about 8 per voxel; 0 for invalid geometry).  Each item's D*H*W < 2^31, N <= 65535.
 * Deterministic, no host sync, capture-safe. */
#define CTU_CC_LARGEST 0
#define CTU_CC_MIN_SIZE 1
size_t ctu_components_ws_bytes(int N, int D, int H, int W);
int ctu_label_components(const void* in, int dtype, int N, int D, int H, int W, int connectivity, const int64_t* applied,
                         int n_applied, int32_t* labels, int32_t* num, void* ws, void* stream);
int ctu_filter_components(const void* in, int dtype, int N, int D, int H, int W, int connectivity,
                          const int64_t* applied, int n_applied, int mode, int param, void* out, void* ws, void* stream);

/* Region properties of label maps (no reference counterpart: users would copy the label map to the host for scipy.ndimage;
 * rule pinned in ctunet_amd/postprocess.py, "Region properties").  labels: DEVICE contiguous [N,D,H,W] of dtype CTU_U8,
 * CTU_I32 (what ctu_label_components writes) or CTU_I64.  Region r (1 <= r <= R) of an item is the set of voxels whose value
 * is r; 0 is background; a negative value or one above R belongs to no region and is counted in overflow.
 *   moments:  DEVICE int64 [N][R][10] = (count, Sz, Sy, Sx, Szz, Szy, Szx, Syy, Syx, Sxx) over the voxel indices, exact.
 *   boxes:    DEVICE int32 [N][R][6] = (z0, y0, x0, z1, y1, x1), half open; six zeros for an empty region.
 *   overflow: DEVICE int64 [N].
 * Every side <= 1024 and D*H*W < 2^31, so every sum stays below 2^51 and converts to float64 exactly; N <= 65535,
 * R <= CTU_REGION_MAX.  ws: ctu_region_moments_ws_bytes() bytes (the box accumulators, 24 per region; 0 for N or R out of
 * range).  Three memsets, one pass over the map (64-bit integer atomics only: the result does not depend on the order of
 * arrival and two calls are bit-equal), one launch that decodes the boxes.  No host sync, capture-safe.
 * ctu_region_derive: the float64 fields of moments, one lane per region, every operation rounded on its own.  frame: HOST
 * [N][6] = (sampling z, y, x, origin z, y, x) per item, or NULL for sampling 1 and origin 0.  With n = count, m_a = S_a / n:
 *   centroid [N][R][3]      origin_a + sampling_a * m_a
 *   covariance [N][R][3][3] ((S_ab / n - m_a * m_b) * sampling_min(a,b)) * sampling_max(a,b)
 *   extent [N][R][3], axes [N][R][3][3]: eigenvalues in descending order and unit eigenvectors as columns, by
 *     CTU_REGION_SWEEPS cyclic Jacobi sweeps; the first two axes are signed so that their component of largest magnitude
 *     (the first one of equals) is positive, the third is their cross product.
 * An empty region gives NaN everywhere; a region of one voxel NaN axes.  One launch per 64 items. */
#define CTU_REGION_MAX 65536
#define CTU_REGION_SWEEPS 8
size_t ctu_region_moments_ws_bytes(int N, int R);
int ctu_region_moments(const void* labels, int dtype, int N, int D, int H, int W, int R, int64_t* moments, int32_t* boxes,
                       int64_t* overflow, void* ws, void* stream);
int ctu_region_derive(const int64_t* moments, int N, int R, const double* frame, double* centroid, double* covariance,
                      double* extent, double* axes, void* stream);

/* Binary morphology of masks on bit images, hole filling and the implant mask (reference: erode / dilate / ErodeDilate of
 * ctunet/pytorch/transforms.py:97-127,356-377 through SimpleITK; pinned here on scipy.ndimage, definitions in
 * ctunet_amd/postprocess.py).  in: DEVICE [N,D,H,W] of dtype CTU_U8 or CTU_I64; a voxel is foreground if it is nonzero or,
 * with has_label != 0, equal to label.  out: DEVICE uint8 [N,D,H,W] of 0 / 1, a buffer of its own unless stated.
 * structure: 27-bit code, bit (i*3+j)*3+k set iff structure[i][j][k] (z, y, x; nonzero).  With S the offsets
 * (i-1, j-1, k-1) of the set bits and every voxel outside the volume reading as the border value (0 / 1):
 *   CTU_MORPH_ERODE:  out[v] = AND_{s in S} in[v+s], `iterations` (1..64) times;  CTU_MORPH_DILATE: out[v] = OR in[v-s];
 *   CTU_MORPH_OPEN:   `iterations` erosions, then as many dilations;  CTU_MORPH_CLOSE: dilations, then erosions (pass
 *                     border 0 for scipy's binary_opening / binary_closing).
 *   fill_holes:   out (may alias in) = in OR the background voxels whose background component (connectivity 1 / 2 / 3)
 *                 touches no face of the volume.
 *   implant_mask: m = (full != 0) AND (defective == 0); opening_iterations (0..64) > 0: opened with structure, border 0;
 *                 fill_holes != 0: holes filled at connectivity 1; then the num_components (1..8) largest components at
 *                 `connectivity` are kept (ctu_filter_components).
 * ws: ctu_morphology_ws_bytes(kind) bytes, 0 for invalid geometry: CTU_MORPH_WS_MORPH (binary_morphology) two bit
 * images, 1/8 byte per voxel each, rows padded to 64 voxels; CTU_MORPH_WS_FILL (fill_holes) the components workspace
 * plus one byte per voxel; CTU_MORPH_WS_IMPLANT (implant_mask) both.  Each item's D*H*W < 2^31, N <= 65535.
 * Deterministic, no atomics in the morphology kernels, no host sync, capture-safe. */
#define CTU_MORPH_ERODE 0
#define CTU_MORPH_DILATE 1
#define CTU_MORPH_OPEN 2
#define CTU_MORPH_CLOSE 3
#define CTU_MORPH_WS_MORPH 0
#define CTU_MORPH_WS_FILL 1
#define CTU_MORPH_WS_IMPLANT 2
size_t ctu_morphology_ws_bytes(int N, int D, int H, int W, int kind);
int ctu_binary_morphology(const void* in, int dtype, int N, int D, int H, int W, int mode, uint32_t structure,
                          int iterations, int border, int has_label, int64_t label, uint8_t* out, void* ws, void* stream);
int ctu_fill_holes(const void* in, int dtype, int N, int D, int H, int W, int connectivity, int has_label, int64_t label,
                   uint8_t* out, void* ws, void* stream);
int ctu_implant_mask(const void* full, int full_dtype, const void* defective, int defective_dtype, int N, int D, int H,
                     int W, uint32_t structure, int opening_iterations, int fill_holes, int connectivity,
                     int num_components, uint8_t* out, void* ws, void* stream);

/* Exact Euclidean distance transform of masks, signed distance and the ball threshold behind ball erosion / dilation (no
 * reference counterpart: the reference erodes / dilates with SimpleITK balls on the host, ctunet/pytorch/transforms.py:97-127;
 * pinned here on scipy.ndimage.distance_transform_edt, definitions in ctunet_amd/postprocess.py).  in: DEVICE [N,D,H,W] of
 * dtype CTU_U8 or CTU_I64; a voxel is foreground if it is nonzero or, with has_label != 0, equal to label.  The SITES are the
 * background voxels (invert != 0: the foreground voxels) and, with border_background != 0, every voxel outside the volume;
 * each voxel gets the distance to its nearest site, a site 0.  spacing: HOST float [N][3] = (z, y, x) per item, NULL or all
 * 1 = unit: int32 squared distances, exact; otherwise fp32 sum (k_i s_i)^2.  An item without a site gets +inf / INT32_MAX
 * and indices -1 (scipy leaves that case undefined).  out, one buffer of [N,D,H,W] by out_kind:
 *   CTU_DIST_EDT:     float32 distance = sqrt of the squared distance;
 *   CTU_DIST_SQUARED: the squared distance, int32 at unit spacing, float32 otherwise;
 *   CTU_DIST_SIGNED:  float32 edt(sites = foreground) - edt(sites = background): > 0 outside, < 0 inside (invert ignored);
 *   CTU_DIST_BALL:    uint8 0 / 1: invert != 0: d2 <= ball_r2 (dilation by the ball), else d2 > ball_r2 (erosion; pass
 *                     border_background = 1 for a border value of 0).
 * indices (NULL: none; CTU_DIST_EDT / CTU_DIST_SQUARED without the virtual border only): DEVICE int32 [N][3][D,H,W], the
 * (z, y, x) of a nearest site of every voxel.  ws: ctu_distance_ws_bytes() bytes, 0 for an invalid shape or kind: 4 bytes
 * per voxel for CTU_DIST_SIGNED / CTU_DIST_BALL (the other kinds work inside out), plus 6 per voxel with indices.
 * Limits: every side <= 1024 (a line pass stacks 6 bytes per line element in LDS), D*H*W < 2^31, N <= 65535; anything
 * beyond is refused, never truncated.  Deterministic, no atomics, no host sync, capture-safe. */
#define CTU_DIST_EDT 0
#define CTU_DIST_SQUARED 1
#define CTU_DIST_SIGNED 2
#define CTU_DIST_BALL 3
size_t ctu_distance_ws_bytes(int N, int D, int H, int W, int out_kind, int want_indices);
int ctu_distance_transform(const void* in, int dtype, int N, int D, int H, int W, int has_label, int64_t label, int invert,
                           int border_background, const float* spacing, int out_kind, void* out, int32_t* indices,
                           float ball_r2, void* ws, void* stream);

/* Local thickness (Hildebrand and Ruegsegger 1997; no reference counterpart: users would run ImageJ / BoneJ on the host;
 * rule pinned in ctunet_amd/postprocess.py).  d2: DEVICE [N,D,H,W], the CTU_DIST_SQUARED map of ctu_distance_transform
 * without the virtual border: int32 (is_float = 0, unit spacing only) or float32 (is_float = 1); 0 marks background, so the
 * mask is not read again; INT32_MAX / +inf everywhere in an item without background.  spacing: HOST float [N][3] = (z, y, x)
 * per item, NULL = unit.  The centre q covers p iff dd(p, q) < d2(q), strictly (the open ball; p covers itself), with dd the
 * integer dz^2 + dy^2 + dx^2 on the int32 path and on the float32 path t_a = float(k_a) s_a, dd = (t_z t_z + t_y t_y) +
 * t_x t_x, every product and sum rounded on its own.  out: DEVICE float32 [N,D,H,W] = 2 sqrtf(max {d2(q) : q covers p}), the
 * correctly rounded root as CTU_DIST_EDT's; 0 on background, +inf in an item without background.  Voxel-centre convention: a
 * plate of k voxels reads 2 ceil(k / 2), i.e. the true thickness plus 0 to 1 voxel; not corrected.
 * ws: ctu_thickness_ws_bytes() bytes (0 for an invalid shape or is_float): 4 bytes per voxel for the pruned candidate map,
 * which is its first plane [N,D,H,W] (0 = background or dropped as dominated), plus 4 per 8^3 cell and per item.
 * Three launches per 64 items (float32) or per call (int32), grids fixed by the shape; no atomics, no host sync,
 * capture-safe, two calls bit-equal.  Limits: every side <= 1024, D*H*W < 2^31, N <= 65535.
 * ctu_thickness_summary: thickness DEVICE float32 [N][V] -> out DEVICE float64 [N][5] = (foreground count, min, max, mean,
 * count below min_thickness); foreground is thickness > 0, below is t < min_thickness in float32 (min_thickness >= 0; 0 counts
 * nothing); the mean is a float64 sum in a fixed order over the count.  An item without foreground: 0, +inf, 0, NaN, 0.
 * ws: ctu_thickness_summary_ws_bytes() bytes (0 for N outside 1..65535 or V < 1).  Two launches, deterministic. */
size_t ctu_thickness_ws_bytes(int N, int D, int H, int W, int is_float);
int ctu_local_thickness(const void* d2, int is_float, int N, int D, int H, int W, const float* spacing, void* out, void* ws,
                        void* stream);
size_t ctu_thickness_summary_ws_bytes(int N, int64_t V);
int ctu_thickness_summary(const float* thickness, int N, int64_t V, float min_thickness, double* out, void* ws, void* stream);

/* Resampling of volumes between voxel grids (no reference counterpart: the reference resizes on the host in its datasets,
 * ctunet/pytorch/datasets.py:89-112; rule and tables pinned in ctunet_amd/resample.py).  in: DEVICE [N,D,H,W], out: DEVICE
 * [N,d,h,w], both contiguous, a buffer each.  Tables: DEVICE arrays of d + h + w entries each, the z, y and x tables one
 * after the other, every entry an input index of its axis (non-decreasing along an axis):
 *   i0 (int32) and wt (float32): lower neighbour and weight of the upper one (the upper neighbour is min(i0 + 1, n - 1));
 *   near (int32): the nearest-exact source index.
 *   CTU_RESAMPLE_NEAREST:      out[k,j,i] = in[near_z[k], near_y[j], near_x[i]]; dtype CTU_U8 (bool too), CTU_I16, CTU_I32,
 *                              CTU_I64 or CTU_F32, the same dtype out.
 *   CTU_RESAMPLE_LINEAR:       lerp(p, q, w) = p + w (q - p), each float32 operation rounded on its own; four lerps along
 *                              x, two along y, one along z; dtype CTU_F32, CTU_I16 or CTU_U8 (converted in the kernel),
 *                              float32 out.
 *   CTU_RESAMPLE_LABEL_LINEAR: the linear rule on the indicator in == c of every class c < num_classes (2..16); out = the
 *                              smallest c of the largest score; a voxel >= num_classes belongs to no class; dtype CTU_U8 or
 *                              CTU_I64, the same dtype out.
 * One launch per 65535 items, no workspace, no atomics, no host sync, capture-safe, bitwise reproducible.  D*H*W < 2^31
 * on either grid; offsets across the batch are 64-bit. */
#define CTU_I16 5
#define CTU_I32 6
#define CTU_RESAMPLE_NEAREST 0
#define CTU_RESAMPLE_LINEAR 1
#define CTU_RESAMPLE_LABEL_LINEAR 2
int ctu_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W, int d, int h, int w,
                 const int32_t* i0, const float* wt, const int32_t* near, void* out, void* stream);

/* Affine resampling of volumes through a matrix in DEVICE memory (no reference counterpart: the reference expects scans
 * registered to its atlas by a host tool, ctunet/pytorch/datasets.py:22-45; rule pinned in ctunet_amd/resample.py).  in:
 * DEVICE [N,D,H,W], out: DEVICE [N,d,h,w], both contiguous, a buffer each.  out_to_in: DEVICE double, row-major [3][4] (or
 * the first three rows of a [4][4]): world (z, y, x) of the OUTPUT grid -> world of the INPUT grid, read by the kernel.
 * spacing, origin (input grid), out_spacing, out_origin (output grid): HOST double [3] in (z, y, x), NULL = 1 / 0; the world
 * coordinate of voxel index k is origin + k spacing.  Per output voxel, in float64 with every operation rounded on its own:
 *   w_a = out_origin_a + idx_a out_spacing_a;  s_a = ((m_a0 w_0 + m_a1 w_1) + m_a2 w_2) + m_a3;  u_a = (s_a - origin_a) / spacing_a
 *   CTU_RESAMPLE_NEAREST:      in[n], n_a = floor(u_a + 0.5); fill where an n_a lies outside [0, size_a) or u is not finite;
 *                              dtype CTU_U8, CTU_I16 or CTU_F32, the same dtype out.
 *   CTU_RESAMPLE_LINEAR:       i0_a = floor(u_a), weight float32(u_a - i0_a), the 8 neighbours i0 + {0,1}^3, one outside the
 *                              volume reading as float32(fill); ctu_resample's lerps, x then y then z; fill where a u_a lies
 *                              outside [-1, size_a) or is not finite; dtype CTU_F32, CTU_I16 or CTU_U8, float32 out.
 *   CTU_RESAMPLE_LABEL_LINEAR: ctu_resample's rule on those 8 neighbours, one outside the volume carrying the label fill;
 *                              dtype CTU_U8, num_classes in 2..16.
 * fill must be representable in the output dtype (finite in float32).  One launch per 65535 items, no workspace, no atomics,
 * no host sync, capture-safe, bitwise reproducible; every read is bounded whatever the matrix holds.  D*H*W < 2^31 on
 * either grid; offsets across the batch are 64-bit. */
int ctu_affine_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W, int d, int h,
                        int w, const double* out_to_in, const double* spacing, const double* origin,
                        const double* out_spacing, const double* out_origin, double fill, void* out, void* stream);

/* Rigid registration of a point set to a distance field: Levenberg-Marquardt on the directed chamfer cost (no reference
 * counterpart, as above; rule pinned in ctunet_amd/registration.py).  points: DEVICE float32 [P][3], world (z, y, x) of the
 * moving frame; field: DEVICE float32 [D][H][W], the distance to the fixed object on the fixed grid (spacing, origin: HOST
 * double [3], NULL = 1 / 0; every side >= 2).  All state lives in ws (ctu_registration_ws_bytes(P) bytes, 0 for P < 1; 8-byte
 * aligned): a head of 1024 bytes of doubles -- M [16], candidate M_c [16], H [21] (upper triangle, row by row), b [6],
 * pivot [3], candidate pivot [3], mean of the finite points [3], cost, lambda, inlier count (int64) -- then one slab row of
 * 32 doubles per block of the accumulation: min(ceil(P / 256), CTU_REG_MAX_BLOCKS) rows of (H [21], b [6], cost, count
 * (int64), padding).
 *   init:       the mean and the start state (M = M_c = init, DEVICE double [4][4], NULL = identity; cost = +inf,
 *               lambda = 1e-3); once per registration.
 *   accumulate: the sums at M_c about the candidate's pivot into the slab, one row per block, no float atomics;
 *               max_distance = +inf: no bound.
 *   update:     iteration `it`: sums the slab in block order, accepts the candidate iff its cost is lower (lambda / 3,
 *               at least 1e-9; otherwise lambda * 10, at most 1e9), solves (H + lambda diag(H) + 1e-12 I) delta = -b by
 *               Cholesky and forms the next candidate; with fewer than CTU_REG_MIN_INLIERS inliers, a pivot that is not
 *               positive or a result that is not finite the candidate stays and the row's flag is -1.  Writes matrix and
 *               inverse (DEVICE double [4][4]: the accepted matrix, (R^T, -R^T t)) and history[it] = (cost / P, inliers,
 *               lambda, 1 accepted / 0 rejected / -1), history DEVICE double [history_rows][4].
 * A registration is init, then (accumulate, update) for it = 0 .. iterations: no host sync, capture-safe, two runs bitwise
 * equal. */
#define CTU_REG_MAX_BLOCKS 1024
#define CTU_REG_MIN_INLIERS 6
size_t ctu_registration_ws_bytes(int64_t P);
int ctu_registration_init(const float* points, int64_t P, const double* init, void* ws, void* stream);
int ctu_registration_accumulate(const float* points, int64_t P, const float* field, int D, int H, int W,
                                const double* spacing, const double* origin, double max_distance, void* ws, void* stream);
int ctu_registration_update(int64_t P, int it, double* matrix, double* inverse, double* history, int history_rows, void* ws,
                            void* stream);

/* Similarity (dof = 7: rotation, translation, isotropic scale) or rigid (dof = 6) registration with the symmetric chamfer
 * cost (rule pinned in ctunet_amd/registration.py): the forward term is the one above; the backward term takes the fixed
 * object's surface points (fixed_points: DEVICE float32 [Q][3], fixed world) through the candidate's inverse into the
 * distance field of the moving object (moving_field: DEVICE float32 [d][h][w] on the moving grid of moving_spacing /
 * moving_origin).  Q = 0: the forward term alone (fixed_points, moving_field and its frame are then ignored).  The calls and
 * their order are those above with the same dof, P and Q throughout; ws holds ctu_similarity_ws_bytes(P, Q) bytes (0 for
 * P < 1 or Q < 0): a head of 1024 bytes -- M [16], M_c [16], their inverses [16] [16], H [28], b [7], pivot [3], candidate
 * pivot [3], mean [3], cost, lambda, det, candidate det, inliers and backward inliers (int64), alive (int64) -- then one slab
 * row of 40 doubles per block: min(ceil((P + Q) / 256), CTU_REG_MAX_BLOCKS) rows of (H [dof (dof + 1) / 2], b [dof], cost,
 * inliers (int64), backward inliers (int64), padding).
 *   init:       the mean of the finite moving points, the start state and the adjugate inverse of init; an init whose
 *               determinant is not finite and positive (or whose inverse is not finite) leaves alive = 0: backward points
 *               are non-inliers, every step is refused, inverse reads the identity and the scale column 0.
 *   accumulate: one launch over P + Q items (forward, then backward) into the slab; no float atomics.
 *   update:     as above with a Cholesky of size dof and the increment [L, pivot - L pivot + delta_t], L = exp(delta_s)
 *               Rod(delta_w) (dof 6: Rod(delta_w)); the step is also refused when the candidate's determinant is not finite
 *               and positive or its inverse not finite.  Writes matrix, inverse (adjugate) and history[it] = (cost / (P + Q),
 *               inliers, lambda, flag, backward inliers, cbrt(det)), history DEVICE double [history_rows][6]. */
size_t ctu_similarity_ws_bytes(int64_t P, int64_t Q);
int ctu_similarity_init(const float* points, int64_t P, const double* init, void* ws, void* stream);
int ctu_similarity_accumulate(int dof, const float* points, int64_t P, const float* field, int D, int H, int W,
                              const double* spacing, const double* origin, const float* fixed_points, int64_t Q,
                              const float* moving_field, int d, int h, int w, const double* moving_spacing,
                              const double* moving_origin, double max_distance, void* ws, void* stream);
int ctu_similarity_update(int dof, int64_t P, int64_t Q, int it, double* matrix, double* inverse, double* history,
                          int history_rows, void* ws, void* stream);

/* B-spline free-form deformation behind a frozen affine matrix (rule pinned in ctunet_amd/registration.py):
 * T(p) = q0 + u(q0), q0 = matrix p (DEVICE double, the first 12 entries of a row-major [3][4] / [4][4]); u the uniform cubic
 * B-spline over control: DEVICE double [3][Gz][Gy][Gx] (mm, fixed frame).  G: HOST int [3], each in 4..CTU_FFD_MAX_G;
 * control_spacing, box_origin: HOST double [3]; control index i sits at box_origin + (i - 1) control_spacing and the lattice
 * has G - 3 cells per axis.  A knot is clamped into the lattice (NaN -> 0) before it indexes a control.
 *   cells:      cells[i] = the lattice cell (cz * ncy + cy) * ncx + cx of point i (DEVICE int32 [P]); the caller sorts the
 *               points by it (stably) and cuts each cell's run into segments of at most CTU_FFD_SEGMENT points:
 *               perm [P] (sorted position -> point), seg_cell / seg_begin / seg_count [S] (begin: a sorted position) and
 *               cell_seg [cells + 1] (the first segment of every cell, ascending), all DEVICE int32.  Every index read from
 *               them is checked against its range; a bad one counts as an absent point.
 *   ws:         ctu_ffd_ws_bytes(G, S) bytes (0 for a bad G or S < 1), 8-byte aligned: a head of 1024 bytes, the accepted
 *               controls, two candidate buffers, gradient and diagonal of the accepted controls, one cost and one inlier
 *               count per segment, and one slab row of 256 doubles (64 controls x gradient z, y, x, diagonal) per segment.
 *   init:       the start state (controls = init_control, DEVICE double [3][Gz][Gy][Gx] or NULL = 0; cost = +inf,
 *               lambda = 1e-3, regulariser weight `weight`), and control = the start controls.
 *   accumulate: one block per segment at the current candidate; no float atomics.
 *   update:     iteration `it`: reduces cost and regulariser, accepts iff the total cost is lower (lambda / 3, at least 1e-9;
 *               otherwise lambda * 10, at most 1e9), then a wave per control point gathers gradient and diagonal (on an
 *               accept), stores the accepted controls into `control` and writes the next candidate
 *               c - grad / ((1 + lambda) d + 1e-12).  history[it] = (total cost / P, data rms, regulariser energy, inliers,
 *               lambda, 1 accepted / 0 rejected / -1 refused), history DEVICE double [history_rows][6]; a step is refused
 *               without an inlier or with a candidate entry that is not finite (that entry is never written).
 * A fit is cells, init, then (accumulate, update) for it = 0 .. history_rows - 1: no host sync after the tables are built,
 * capture-safe, two runs bitwise equal.
 *   transform_points: out (DEVICE float32 [P][3] or NULL) = float32(T(p)); jacobian (DEVICE double [P] or NULL) =
 *               det(I + du/dq0); at least one of the two.
 *   resample:   ctu_affine_resample with s = T(w) in place of s = out_to_in w: per output voxel w is its world coordinate,
 *               u_a = (s_a - origin_a) / spacing_a, then that entry point's rule per mode; same dtypes, limits and fill. */
#define CTU_FFD_SEGMENT 256
#define CTU_FFD_MAX_G 64
size_t ctu_ffd_ws_bytes(const int* G, int64_t S);
int ctu_ffd_cells(const float* points, int64_t P, const double* matrix, const int* G, const double* control_spacing,
                  const double* box_origin, int* cells, void* stream);
int ctu_ffd_init(const int* G, int64_t S, const double* init_control, double weight, void* ws, double* control, void* stream);
int ctu_ffd_accumulate(const float* points, int64_t P, const double* matrix, const float* field, int D, int H, int W,
                       const double* spacing, const double* origin, const int* G, const double* control_spacing,
                       const double* box_origin, double max_distance, const int* perm, const int* seg_cell,
                       const int* seg_begin, const int* seg_count, int64_t S, void* ws, void* stream);
int ctu_ffd_update(int64_t P, const int* G, const double* control_spacing, const double* box_origin, const int* cell_seg,
                   int64_t S, int it, double* control, double* history, int history_rows, void* ws, void* stream);
int ctu_ffd_transform_points(const float* points, int64_t P, const double* matrix, const double* control, const int* G,
                             const double* control_spacing, const double* box_origin, float* out, double* jacobian,
                             void* stream);
int ctu_ffd_resample(const void* in, int dtype, int mode, int num_classes, int64_t N, int D, int H, int W, int d, int h, int w,
                     const double* matrix, const double* control, const int* G, const double* control_spacing,
                     const double* box_origin, const double* spacing, const double* origin, const double* out_spacing,
                     const double* out_origin, double fill, void* out, void* stream);

/* Surface meshes of label volumes and scalar fields (no reference counterpart: the reference writes NIfTI volumes only;
 * rule pinned in ctunet_amd/mesh.py): marching tetrahedra on the Kuhn split of the cells of the grid padded by one layer of
 * outside points, welded (shared vertex indices) and closed.  volume: DEVICE contiguous [D,H,W] of dtype CTU_U8 or CTU_I64
 * (inside = nonzero or, with has_label != 0, equal to label; the corner values are 1 / 0 against level 0.5, fill 0) or
 * CTU_F32 (inside = value > level; the virtual layer holds fill_value <= level).
 *   count:   classifies the (D+1)(H+1)(W+1) cells, numbers vertices and faces (cells in C order, then owned edges / then
 *            tetrahedra) with a fixed-order scan and leaves the int64 totals (V, F) in the first 16 bytes of ws, which the
 *            caller reads after synchronising the stream: the one host synchronisation of an extraction.
 *   emit:    with the ws that count filled and the same volume: vertices DEVICE float32 [V][3] = (z, y, x) =
 *            origin + (index + t * d) * spacing (HOST float [3] each, NULL = 0 / 1; each operation rounded on its own),
 *            faces DEVICE int32 [F][3], the right-hand normal in (x, y, z) pointing from inside to outside.  V and F are the
 *            totals count left; V or F >= 2^31 is refused, never truncated.
 *   measure: out DEVICE double [2] = (area, enclosed volume = sum p0 . (p1 x p2) / 6 in (x, y, z)), float64 arithmetic on the
 *            float32 vertices, summed in a fixed order; normals (NULL: none) DEVICE float32 [F][3] unit normals in (z, y, x),
 *            0 for a face without area.  ws: CTU_MESH_MEASURE_WS bytes.
 * ws of count / emit: ctu_mesh_ws_bytes() bytes, 0 for an invalid shape: 5 bytes per cell of the row-padded cell grid (rows
 * of W+1 cells rounded up to 16) + 12 per cell row + 256; 16-byte aligned.  Cell rows are the blocks of the scan:
 * CTU_MESH_SCAN_BLOCK threads scan them, several rows per thread beyond that many rows.
 * Limits: every side <= 1024, (D+1)(H+1)(W+1) < 2^31.  No atomics; two calls are bitwise equal. */
#define CTU_MESH_SCAN_BLOCK 1024
#define CTU_MESH_MEASURE_WS 16384
size_t ctu_mesh_ws_bytes(int D, int H, int W);
int ctu_mesh_count(const void* volume, int dtype, int D, int H, int W, int has_label, int64_t label, float level, void* ws,
                   void* stream);
int ctu_mesh_emit(const void* volume, int dtype, int D, int H, int W, float level, float fill_value, const float* spacing,
                  const float* origin, int64_t V, int64_t F, float* vertices, int32_t* faces, void* ws, void* stream);
int ctu_mesh_measure(const float* vertices, int64_t V, const int32_t* faces, int64_t F, double* out, float* normals, void* ws,
                     void* stream);

/* Vertex adjacency (CSR) and Taubin / Laplacian smoothing of surface meshes (no reference counterpart; rule pinned in
 * ctunet_amd/mesh.py).  faces: DEVICE int32 [F][3]; N(i) = the distinct vertices j != i that share a face with i, ascending;
 * offsets int32 [V+1], neighbours int32 [E] hold the sets in vertex order.
 *   build: counts, scans, fills, sorts and de-duplicates into ws, writes offsets [V+1] and, at the head of ws, two int64:
 *          (E, the number of faces with an index outside [0, V)).  Such faces are skipped, never read through.  The caller
 *          reads the head (one synchronisation), refuses the mesh if the second word is non-zero, allocates neighbours [E]
 *          and calls emit with the same ws.
 *   emit:  neighbours [E] from ws; every write is bounded by E.
 *   V = 0 or F = 0 (E = 0 for emit): nothing is launched or written; the table is empty (offsets all zero, E = 0).
 *   ws: ctu_mesh_adjacency_ws_bytes(V, F) bytes, 0 outside the limits: 256 + 8 V + 24 F + 8 per scan chunk, each array
 *       rounded up to 256; 16-byte aligned.  CTU_MESH_ADJ_SCAN_CHUNK vertices are one block of the scan; beyond that the
 *       chunk sums are scanned by one block.
 *   smooth: `iterations` times a step with factor lambda and, with has_mu != 0, a step with factor mu (Taubin); per step and
 *          vertex with neighbours and fixed[i] == 0 (fixed NULL: none): v' = v + s * (sum of N(i) in order / |N(i)| - v) in
 *          float32, every operation rounded on its own, all reads from the previous positions.  vertices, out: DEVICE float32
 *          [V][3], distinct; fixed: DEVICE uint8 [V].  Offsets are bounded against E and neighbours against V before use.
 *          0 < lambda <= 1; mu finite and < -lambda; iterations in 0..CTU_MESH_SMOOTH_MAX_ITERATIONS (0: a copy).
 *          ws: ctu_mesh_smooth_ws_bytes(V) = two staged copies of 16 bytes per vertex; 16-byte aligned.
 * Limits: V < 2^31 and 6 F < 2^31 (so E and every offset fit an int32).  Integer atomics only where the final value does
 * not depend on arrival order; two calls are bitwise equal. */
#define CTU_MESH_ADJ_SCAN_CHUNK 4096
#define CTU_MESH_SMOOTH_MAX_ITERATIONS 10000
size_t ctu_mesh_adjacency_ws_bytes(int64_t V, int64_t F);
int ctu_mesh_adjacency_build(const int32_t* faces, int64_t V, int64_t F, int32_t* offsets, void* ws, void* stream);
int ctu_mesh_adjacency_emit(int64_t V, int64_t F, int64_t E, const int32_t* offsets, int32_t* neighbours, void* ws,
                            void* stream);
size_t ctu_mesh_smooth_ws_bytes(int64_t V);
int ctu_mesh_smooth(const float* vertices, int64_t V, const int32_t* offsets, const int32_t* neighbours, int64_t E,
                    const uint8_t* fixed, int iterations, float lambda, int has_mu, float mu, float* out, void* ws,
                    void* stream);

/* Voxelisation of a surface mesh onto a [D,H,W] grid (no reference counterpart; rule pinned in ctunet_amd/mesh.py): the
 * winding number of the mesh around every voxel centre origin + (i, j, k) * spacing, by rays along x, float64 arithmetic on
 * the float32 vertices.  vertices: DEVICE float32 [V][3] in (z, y, x); faces: DEVICE int32 [F][3]; spacing, origin: HOST
 * float [3] in (z, y, x) (NULL: 1 and 0).  out: DEVICE uint8 [D][H][W] (1 where the winding number is not 0) or, with
 * want_winding != 0, int32 [D][H][W] (the numbers).  A face with an index outside [0, V) or a vertex that is not finite is
 * skipped, never read through, and counted: the head of ws holds that count as one int64, which the caller reads after
 * the call (its one synchronisation) and refuses the mesh on.  F = 0: out and the head are cleared, no kernel is launched.
 *   ws: ctu_mesh_voxelize_ws_bytes() bytes, 0 for an invalid shape: 256 + 4 per voxel (rounded up to 256); 16-byte aligned.
 * Limits: every side <= 1024, D*H*W < 2^31, V < 2^31, F < 2^31.  Integer atomics only (the sums do not depend on arrival
 * order); two calls are bitwise equal. */
size_t ctu_mesh_voxelize_ws_bytes(int D, int H, int W);
int ctu_mesh_voxelize(const float* vertices, int64_t V, const int32_t* faces, int64_t F, int D, int H, int W,
                      const float* spacing, const float* origin, int want_winding, void* out, void* ws, void* stream);

/* Exact distances from points to a surface mesh (no reference counterpart; rule pinned in ctunet_amd/mesh.py): a uniform grid
 * of face lists over the bounding box of the mesh, and a nearest-triangle query in float64 on the float32 vertices.
 *   grid_build: vertices DEVICE float32 [V][3] in (z, y, x), faces DEVICE int32 [F][3], F >= 1.  Writes corners DEVICE float32
 *          [F][12] (the nine coordinates of every face and three words of padding; 16-byte aligned), fixes the grid (cell
 *          size: cell_size, or with cell_size = 0 twice the mean largest extent of a face, doubled until the grid has at most
 *          max_cells cells; floor(extent / size) + 1 cells per axis, 1 for an axis without extent), counts the faces of every
 *          cell its bounding box overlaps and scans the counts.  A face with an index outside [0, V) or a vertex that is not
 *          finite is refused: counted, listed nowhere, never read through.  The head of ws then holds 13 words the caller
 *          reads after synchronising (the build's one synchronisation): int64 pairs, refused faces, cells, overflow (1: the
 *          given cell_size needs more than max_cells cells; the grid is then one cell and must be refused), nz, ny, nx, then
 *          double lower corner (z, y, x) and cell size (z, y, x): the `frame` of a query.
 *   grid_emit: with the ws and corners of grid_build: offsets DEVICE int32 [cells + 1], items DEVICE int32 [pairs]: the faces
 *          of cell c are items[offsets[c] .. offsets[c + 1]), in no particular order.  pairs >= 2^31 is refused.
 *   ws: ctu_mesh_grid_ws_bytes(F, max_cells) bytes, 0 outside the limits: 256 + 64 per block of 256 faces + 8 max_cells + 8
 *       per scan chunk of 4096 cells, each array rounded up to 256; 16-byte aligned.  max_cells in 1..CTU_MESH_GRID_MAX_CELLS.
 *   distance: dist DEVICE float32 [Q] = the distance from every query to the nearest face; face (NULL: none) DEVICE int32 [Q] =
 *          the lowest index among the nearest faces; closest (NULL: none) DEVICE float32 [Q][3] = that face's closest point.
 *          Queries: points DEVICE float32 [Q][3], or with points = NULL the Q = D*H*W centres origin + (i, j, k) * spacing of a
 *          grid (HOST float [3] each, NULL = 1 and 0; every side <= 1024, D*H*W < 2^31) in C order.  max_distance > 0: a query
 *          farther than that gets far_value, face -1 and closest NaN; 0: unbounded.  A query that is not finite gets NaN, -1,
 *          NaN.  Every offset is bounded against pairs and every listed face against F before use.  No workspace, no
 *          synchronisation; capture-safe.
 * Limits: V, F, pairs, Q < 2^31.  Integer atomics only for counts and fill cursors; float64 with contraction off; the
 * result does not depend on the cell size and two calls are bitwise equal. */
#define CTU_MESH_GRID_MAX_CELLS 16777216
size_t ctu_mesh_grid_ws_bytes(int64_t F, int64_t max_cells);
int ctu_mesh_grid_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, float cell_size, int64_t max_cells,
                        float* corners, void* ws, void* stream);
int ctu_mesh_grid_emit(const float* corners, int64_t F, int64_t max_cells, int64_t cells, int64_t pairs, int32_t* offsets,
                       int32_t* items, void* ws, void* stream);
int ctu_mesh_distance(const float* corners, int64_t F, const int32_t* offsets, const int32_t* items, int64_t pairs,
                      const double* frame, int nz, int ny, int nx, const float* points, int64_t Q, int D, int H, int W,
                      const float* spacing, const float* origin, float max_distance, float far_value, float* dist,
                      int32_t* face, float* closest, void* stream);

/* Decimation of a surface mesh by vertex clustering on a uniform grid (no reference counterpart; rule pinned in
 * ctunet_amd/simplify.py).  vertices: DEVICE float32 [V][3] in (z, y, x); faces: DEVICE int32 [F][3], F >= 1.  A face with an
 * index outside [0, V) or a vertex that is not finite is refused: counted, never read through.  A member is a vertex of an
 * accepted face.  lo, hi, cell_size: HOST float [3] in (z, y, x).
 *   bounds: the box of the members.  The head of ws then holds, for the caller to read after synchronising (the first of the
 *          two synchronisations): int64 refused faces, then float32 lo (z, y, x) and hi (z, y, x).  The caller refuses the
 *          mesh if the count is not 0, and otherwise fixes the grid: n_a = floor((hi_a - lo_a) / cell_a) + 1 cells per axis
 *          in float64, cells = n_z n_y n_x <= CTU_MESH_DECIMATE_MAX_CELLS.
 *   build: with lo and hi as bounds gave them and `cells` as above (checked against cell_size): the cell of every member,
 *          the occupied cells numbered in ascending order, the faces whose corners lie in three different cells bucketed by
 *          their lowest cell, with cancel != 0 the cancellation of faces with the same three cells and opposite orientation,
 *          the cells the surviving faces use numbered in ascending order, the surviving faces numbered in input order, and
 *          the integer sums of the members' quantised positions per used cell.  A face whose bucket holds more than
 *          CTU_MESH_DECIMATE_MAX_BUCKET faces is not compared and sets the overflow word: no thread loops over more than that
 *          many items.  The head of ws then holds three int64 for the caller to read after synchronising (the second
 *          synchronisation): V', F', overflow (refuse the mesh if it is not 0).
 *   emit:  with the faces and the ws of build, Vp = V' and Fp = F': out_vertices DEVICE float32 [V'][3] (per used cell and axis
 *          float32(lo + (sum / count) / S), float64), out_faces DEVICE int32 [F'][3] (the surviving faces in input order and
 *          corner order, renumbered), out_map (NULL: none) DEVICE int32 [V]: the output vertex of every input vertex's cell, -1
 *          for a vertex in no accepted face or in a cell no surviving face uses.  Every write is bounded by Vp and Fp.
 *   ws: ctu_mesh_decimate_ws_bytes(V, F, cells) bytes, 0 outside the limits; 16-byte aligned.  cells = 0: the workspace of
 *       bounds, 256 bytes.  cells >= 1: the workspace of build and emit: 256 + 5 per cell + 49 per vertex + 24 per face + 8 per
 *       scan chunk of 4096 of the largest of the three, each array rounded up to 256.
 * Limits: V, F < 2^31, cells <= CTU_MESH_DECIMATE_MAX_CELLS.  Integer atomics only (min, max, counts, fill cursors, sums); float64
 * with contraction off; two calls are bitwise equal. */
#define CTU_MESH_DECIMATE_MAX_CELLS 268435456
#define CTU_MESH_DECIMATE_MAX_BUCKET 4096
size_t ctu_mesh_decimate_ws_bytes(int64_t V, int64_t F, int64_t cells);
int ctu_mesh_decimate_bounds(const float* vertices, int64_t V, const int32_t* faces, int64_t F, void* ws, void* stream);
int ctu_mesh_decimate_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const float* lo, const float* hi,
                            const float* cell_size, int64_t cells, int cancel, void* ws, void* stream);
int ctu_mesh_decimate_emit(const int32_t* faces, int64_t V, int64_t F, int64_t Vp, int64_t Fp, const float* lo, const float* hi,
                           float* out_vertices, int32_t* out_faces, int32_t* out_map, void* ws, void* stream);

/* CT preprocessing: from a scanner's volume to a binary skull (no reference counterpart: the reference's datasets load skulls
 * that were thresholded beforehand, ctunet/pytorch/datasets.py:22-45; rules pinned in ctunet_amd/preprocess.py).  Every input
 * `in` is a DEVICE contiguous array of dtype CTU_F32, CTU_I16 or CTU_U8, converted in the kernel.  No entry point allocates
 * or synchronises, each is capture-safe, and two calls are bitwise equal (the only atomics add integers).
 *   gaussian_filter: in [N,D,H,W] -> out float32 [N,D,H,W], separable, axes in the order x, y, z.  radius: HOST int [3] in
 *                    (z, y, x), each 0..CTU_GAUSS_MAX_RADIUS; weights: HOST float, w_0..w_R of z, then of y, then of x.  One
 *                    axis: acc = w_0 v[i]; acc = acc + w_k (v[i-k] + v[i+k]) for k = 1..R, every float32 operation rounded
 *                    on its own.  mode: what v reads outside the axis (clamp; scipy's reflect, period 2 n; cval).
 *                    ws: ctu_gaussian_ws_bytes() bytes (0 for an invalid shape or rz = 0), 16-byte aligned: the volume after
 *                    x and y.  Every side <= 1024, D*H*W < 2^31.
 *   finite_minmax:   range [2] (DEVICE double) = the smallest and the largest finite element of in [n] (+inf, -inf if none);
 *                    ws: ctu_minmax_ws_bytes(n) bytes.
 *   histogram:       hist [bins] (DEVICE int64, cleared by the call) over in [n], bins in 2..CTU_HISTOGRAM_MAX_BINS.  The range
 *                    is DEVICE double [2] = (lo, hi) when `range` is given, else the HOST values lo <= hi.  In float64:
 *                    hi == lo widens both by 0.5; scale = bins / (hi - lo); v in [lo, hi] counts in
 *                    min(floor((v - lo) scale), bins - 1); anything else, NaN included, is not counted.  n < 2^38.
 *   threshold_otsu:  on hist [bins] with N = sum h, S = sum k h_k and the exact int64 prefixes w1_k, s1_k (k = 0..bins-2):
 *                    var_k = (double(w1) double(N - w1)) ((m1 - m2) (m1 - m2)), m1 = s1 / w1, m2 = (S - s1) / (N - w1), 0
 *                    where w1 = 0 or w1 = N; index = the first maximum k*; threshold = lo + (k* + 0.5) ((hi - lo) / bins)
 *                    with the range as in histogram.  threshold: DEVICE double [1]; index: DEVICE int64 [1] or NULL.
 *   binarize:        out [n] (uint8 0 / 1) = in > lower && in <= upper, compared in float64.  Each bound is DEVICE double [1]
 *                    when its pointer is given, else the HOST value (upper = +inf: no upper bound). */
#define CTU_GAUSS_NEAREST 0
#define CTU_GAUSS_REFLECT 1
#define CTU_GAUSS_CONSTANT 2
#define CTU_GAUSS_MAX_RADIUS 32
#define CTU_HISTOGRAM_MAX_BINS 4096
size_t ctu_gaussian_ws_bytes(int64_t N, int D, int H, int W, int rz);
int ctu_gaussian_filter(const void* in, int dtype, int64_t N, int D, int H, int W, const int* radius, const float* weights,
                        int mode, float cval, float* out, void* ws, void* stream);
size_t ctu_minmax_ws_bytes(int64_t n);
int ctu_finite_minmax(const void* in, int dtype, int64_t n, double* range, void* ws, void* stream);
int ctu_histogram(const void* in, int dtype, int64_t n, int bins, const double* range, double lo, double hi, int64_t* hist,
                  void* stream);
int ctu_threshold_otsu(const int64_t* hist, int bins, const double* range, double lo, double hi, double* threshold,
                       int64_t* index, void* stream);
int ctu_binarize(const void* in, int dtype, int64_t n, const double* lower_dev, double lower, const double* upper_dev,
                 double upper, uint8_t* out, void* stream);

/* Rank filters over a box: median, percentile, grey minimum and maximum (no reference counterpart; rule pinned in
 * ctunet_amd/preprocess.py, "rank filters").  in: DEVICE contiguous [N,D,H,W] of dtype CTU_F32, CTU_I16 or CTU_U8; out: the
 * same shape and dtype, a buffer of its own.  size: HOST int [3] = (z, y, x), each odd and in 1..CTU_RANK_MAX_SIZE; the
 * window of a voxel is the size[0] * size[1] * size[2] = n elements centred on it, a position outside the volume read through
 * mode per axis (CTU_GAUSS_NEAREST / _REFLECT / _CONSTANT; the constant is cval, which must be representable in the dtype:
 * an integer in range, or finite as a float32).  Every element maps to an unsigned key that keeps the order and its bits
 * (uint8: the value; int16: value + 32768; float32 with bits b: ~b if the sign is set, else b | 0x80000000); out is the
 * element whose key is the rank-th smallest (0-based, 0 <= rank < n) of the window, with its own bits.  The order is
 * total: NaNs of negative sign < -inf < .. < -0 < +0 < .. < +inf < NaNs of positive sign.
 * A block owns CTU_RANK_TILE_Z x _Y x _X outputs.  One launch per 65535 items, no workspace (ws_bytes is 0, ws may be
 * NULL), no atomics, no host sync, capture-safe, bitwise reproducible.  Every side in 1..1024.
 * Refused before any launch (CTU_EINVAL): null in / out / size, another dtype or mode, a size that is even, < 1 or
 * > CTU_RANK_MAX_SIZE, rank outside [0, n), a side outside 1..1024, N < 1, a cval the dtype cannot hold. */
#define CTU_RANK_MAX_SIZE 7
#define CTU_RANK_TILE_Z 8
#define CTU_RANK_TILE_Y 4
#define CTU_RANK_TILE_X 64
size_t ctu_rank_filter_ws_bytes(int64_t N, int D, int H, int W, const int* size);
int ctu_rank_filter(const void* in, int dtype, int64_t N, int D, int H, int W, const int* size, int rank, int mode,
                    double cval, void* out, void* ws, void* stream);

/* Patch tiling of whole volumes (BASELINE config 4: skull volumes tiled to 192^3 patches; the tiles carry the sample
 * schema of ctunet/pytorch/datasets.py:89-112,195-235).  coords: DEVICE int32 [P][3] = (z0, y0, x0) of each patch.
 *   extract: out [P,C,pd,ph,pw] = vol [C,D,H,W] windows, zero-filled outside the volume
 *   stitch:  out [C,D,H,W] = mean over the patches covering each voxel (fixed patch order, no atomics), 0 if none */
int ctu_extract_patches(const float* vol, const int32_t* coords, int P, int C, int D, int H, int W, int pd, int ph,
                        int pw, float* out, void* stream);
int ctu_stitch_patches(const float* patches, const int32_t* coords, int P, int C, int D, int H, int W, int pd, int ph,
                       int pw, float* out, void* stream);

/* Sliding-window inference (whole-volume prediction from patch-sized forwards; the reference resizes whole volumes to the
 * network size instead, ctunet/pytorch/datasets.py:89-112,195-235).  One batch of B patch predictions at a time is blended
 * into whole-volume fp32 accumulators num [K,D,H,W] and wsum [D,H,W]:
 *   for each valid patch p of the batch, in order, and each voxel v = (z0+i, y0+j, x0+k) it covers inside the volume:
 *     w = max(wz[i] * wy[j] * wx[k], wmin);  num[c][v] += w * patches[p][c][i][j][k];  wsum[v] += w
 *   (1-D tables of pd / ph / pw floats: Gaussian for the Gaussian blend, all ones for the plain mean).
 *   coords: DEVICE int32 [B][3] = (z0, y0, x0); valid: DEVICE int32 [B], 0 = padding slot (skipped, coords still read).
 *   box: DEVICE int32 [3] = origin of the batch's bounding box, box[2] a multiple of 4; bz/by/bx (bx a multiple of 4): the
 *   extents the launch covers from that origin -- at least those of the batch's box.  Everything that changes between
 *   batches is read from device memory, so one captured launch serves every batch of a volume.
 *   Gather form (one thread per 4 x-consecutive voxels of the box), no atomics: bitwise reproducible.  wsum NULL: num only
 *   (a second output head sharing the first head's weight sum).  B <= 64, K <= 4, pw a multiple of 4; patches, wx, num
 *   and wsum 16-byte aligned.
 * finalize: probs[c][v] = num[c][v] / wsum[v] (0 where wsum == 0) and, if labels is non-NULL, labels[v] = the first c of the
 *   largest probability (the rule of ctu_hard_segm), uint8.  probs may be num itself (in place).  V = D*H*W. */
int ctu_window_accumulate(const float* patches, const int32_t* coords, const int32_t* valid, const int32_t* box, int B,
                          int K, int D, int H, int W, int pd, int ph, int pw, const float* wz, const float* wy,
                          const float* wx, float wmin, int bz, int by, int bx, float* num, float* wsum, void* stream);
int ctu_window_finalize(const float* num, const float* wsum, int K, int64_t V, float* probs, uint8_t* labels,
                        void* stream);

/* Test-time mirroring, ensembles and uncertainty for sliding-window inference (rule: ctunet_amd/inference.py).  The three
 * entry points above with a flip word, flip: DEVICE int32 [1], bit 0 = x, bit 1 = y, bit 2 = z (only the low 3 bits are
 * read; on a mirrored axis a patch-local index a becomes P_a - 1 - a), so one captured launch serves every pass.
 *   extract_patches_flip: out [P,C,pd,ph,pw] = the zero-padded window of ctu_extract_patches, mirrored; at flip 0 the
 *     same bits.  16-byte row reads where W % 4 == 0, vol is 16-byte aligned and the source quad starts at a multiple of
 *     4 inside its row, scalar reads otherwise.  pw a multiple of 4, P * C <= 65535, pd * ph * pw < 2^31; out 16-byte
 *     aligned, vol at any float address.
 *   window_accumulate_flip: ctu_window_accumulate reading patches[p][c] at the mirrored local index (the weight tables
 *     stay indexed by the un-mirrored position), and, per valid patch in order,
 *       sq [K,D,H,W] += w * (y * y)   if sq is non-NULL
 *       sh [D,H,W]   += w * h(y)      if sh is non-NULL (K >= 2),  h(y) = -sum_k q_k ln q_k / ln K,
 *                                     q_k = max(y_k, 0) / sum_j max(y_j, 0), 0 for a zero sum, 0 ln 0 = 0.
 *     Limits and alignment as ctu_window_accumulate; sq and sh 16-byte aligned.
 *   window_finalize_stats: probs and labels as ctu_window_finalize, and where the pointer is non-NULL
 *       var [K,V] = max(sq / wsum - probs^2, 0)  (needs sq; var may be sq itself)
 *       ent [V]   = h(probs)                     (K >= 2)
 *       mi  [V]   = max(h(probs) - sh / wsum, 0) (needs sh, K >= 2);   all 0 where wsum == 0. */
int ctu_extract_patches_flip(const float* vol, const int32_t* coords, const int32_t* flip, int P, int C, int D, int H,
                             int W, int pd, int ph, int pw, float* out, void* stream);
int ctu_window_accumulate_flip(const float* patches, const int32_t* coords, const int32_t* valid, const int32_t* box,
                               const int32_t* flip, int B, int K, int D, int H, int W, int pd, int ph, int pw,
                               const float* wz, const float* wy, const float* wx, float wmin, int bz, int by, int bx,
                               float* num, float* wsum, float* sq, float* sh, void* stream);
int ctu_window_finalize_stats(const float* num, const float* wsum, const float* sq, const float* sh, int K, int64_t V,
                              float* probs, uint8_t* labels, float* var, float* ent, float* mi, void* stream);

/* Flap-reconstruction augmentation (SkullRandomHole + SaltAndPepper of ctunet/pytorch/transforms.py:13-95,131-134 and
 * ctunet/utilities.py:127-178, on the device; rules pinned in ctunet_amd/transforms.py).  Batch of N skulls
 * [N,1,D,H,W], float32 (u8 = 0) or uint8 (u8 = 1); a voxel's value is its uint8 cast (truncation, float values in
 * [0, 256)) and it is bone iff that is nonzero.  Three launches, no atomics, no host sync:
 *   count: counts [N][ceil(V / CTU_FLAP_CHUNK)] int32 = bone voxels per chunk of CTU_FLAP_CHUNK voxels in C order.
 *   draw:  one block per sample: writes params [N][CTU_FLAP_RECORD] int32 from the DEVICE counters (int64 [1]) and
 *          density (float32 [1]) of the hole / noise instances; sample n of the batch uses sequence number counter + n.
 *          mode: CTU_FLAP_HOLE | CTU_FLAP_NOISE.  shapes = count | code_i << (2 + 2 i), codes CTU_FLAP_SPHERE / BOX / FLAP.
 *          Hole sizes are drawn in [size_lo, size_hi).  counts may be NULL without CTU_FLAP_HOLE.
 *   apply: one pass over the batch (4 x-consecutive voxels per thread): x [N,C,D,H,W] float32 gets the image in channel 0
 *          and a copy of atlas [D,H,W] in channel 1 (C = 2 iff atlas); full / flap [N,2,D,H,W] float32 (either may be
 *          NULL) get the one-hot full skull and flap.  Advances the device counters by N and, with decay, stores the
 *          last sample's density.  skull may be x itself (C = 1, in place).
 * record: 0 hole drawn (u < p_hole)  1 bone count  2 k  3-5 centre z, y, x (-1 without bone)  6 size  7 shape
 *         8 c_diam (float bits)  9 hole cut (drawn and count > 0)  10 noise drawn  11 density nd' (float bits)
 *         12 zero threshold nd' (1 - salt_ratio)  13 salt threshold nd' salt_ratio (float bits)  14-15 noise sequence lo, hi */
#define CTU_FLAP_CHUNK 8192
#define CTU_FLAP_RECORD 16
#define CTU_FLAP_HOLE 1
#define CTU_FLAP_NOISE 2
#define CTU_FLAP_SPHERE 0
#define CTU_FLAP_BOX 1
#define CTU_FLAP_FLAP 2
int ctu_flap_count(const void* skull, int u8, int N, int64_t V, int32_t* counts, void* stream);
int ctu_flap_draw(const void* skull, int u8, int N, int D, int H, int W, const int32_t* counts, int mode,
                  const int64_t* hole_seq, uint64_t hole_seed, float p_hole, int size_lo, int size_hi, int shapes,
                  const int64_t* noise_seq, const float* noise_nd, uint64_t noise_seed, float p_noise, float salt_ratio,
                  int decay, int32_t* params, void* stream);
int ctu_flap_apply(const void* skull, int u8, const float* atlas, int N, int D, int H, int W, const int32_t* params,
                   int mode, int64_t* hole_seq, int64_t* noise_seq, float* noise_nd, uint64_t noise_seed, int decay,
                   float* x, int C, float* full, float* flap, void* stream);

/* Class-balanced random patch sampling for training (no reference counterpart: its datasets feed whole resized volumes;
 * rule pinned in ctunet_amd/sampling.py).  labels: DEVICE uint8 [M][D][H][W] (bool as its bytes), V = D H W < 2^31,
 * M <= 65535.  K classes, 1 <= K <= CTU_PATCH_MAX_CLASSES: classes = HOST int [K], class i holds the voxels == classes[i]
 * (0..255); classes = NULL: K = 1 and the class holds the voxels != 0.  Three entry points, no atomics, no host sync,
 * capture-safe, bitwise reproducible.
 *   index: counts [M][K][ceil(V / CTU_PATCH_CHUNK)] int32 = voxels of class i per chunk of CTU_PATCH_CHUNK flat C-order
 *          indices of item m.  One read of the labels for all K classes, in 16-byte loads on the 16-byte grid of each item's
 *          own address (an item of odd V starts anywhere); built once for a static dataset.
 *   draw:  one block per patch j < P, from volume items[j] (DEVICE int32 [P]).  seq = counter[0] + j (counter: DEVICE
 *          int64 [1]); Philox4x32-10 keyed by seed, stream 0: c0 = 0 -> (r_class, r_k, -, -), c0 = 1 -> (r_z, r_y, r_x, -);
 *          draw_int(r, lo, span) = lo + ((r span) >> 32).  u = (r_class >> 8) 2^-24 as a double; cum: HOST double [K], the
 *          rising running sums of the class probabilities, cum[K-1] <= 1; class i is chosen iff cum[i-1] <= u < cum[i],
 *          otherwise the patch is uniform.  Per axis a (volume side n_a, patch side p_a = patch[a], J_a = jitter[a], HOST
 *          int [3] each, 0 <= J_a <= (p_a - 1) / 2), hi_a = max(0, n_a - p_a):
 *            uniform patch: s_a = draw_int(r_a, 0, hi_a + 1)
 *            class patch:   count = voxels of the class in the item (sum of its counts); count == 0: the uniform rule with
 *                           the same words, and fallback = 1; else k = draw_int(r_k, 0, count), centre c = the k-th voxel
 *                           of the class in C order, j_a = draw_int(r_a, -J_a, 2 J_a + 1),
 *                           s_a = min(max(c_a - p_a / 2 + j_a, 0), hi_a)  -- the centre always lies inside the patch.
 *          An item outside [0, M) reads nothing: its coords are (-1, 0, 0, 0) and its record is item -1, starts 0, class
 *          -1, centre -1, the rest 0.  After the draw launch a one-thread launch adds P to counter[0].
 *          coords:  [P][4] int32 = (item, z0, y0, x0).
 *          records: [P][CTU_PATCH_RECORD] int32 = 0 item  1-3 start z, y, x  4 class index (-1 = uniform)  5 fallback
 *                   6 count  7 k  8-10 centre z, y, x (-1 without one)  11 zero.
 *   crop:  out [P][Ctot][pd][ph][pw], channels [out_channel, out_channel + C) = the window at (z0, y0, x0) of channel c of
 *          src [Ms][C][D][H][W] item coords[p][0] (Ms == 1: one source shared by every patch with an item >= 0).  dtype
 *          CTU_U8, CTU_I16 or CTU_F32; the output's is the source's or CTU_F32 (exact conversions).  coords may hold any
 *          int32: a voxel outside the volume, and every voxel of a patch whose item is negative or (Ms > 1) >= Ms, is
 *          fill, which the output dtype must hold exactly; no address outside src is formed.  One output row is one span
 *          of a source row; whole 16-byte chunks of an output row are 16-byte stores at any pw and alignment.  The other
 *          channels of out are not written.  P C is not bounded by a grid dimension; pd ph pw < 2^31.
 * Refused before any launch (CTU_EINVAL): null pointers, shapes and sizes outside the above, K outside its range, a class
 * outside 0..255, cum not rising within [0, 1], a jitter outside its bound, a dtype pair or fill outside the above. */
#define CTU_PATCH_CHUNK 8192
#define CTU_PATCH_MAX_CLASSES 4
#define CTU_PATCH_RECORD 12
int ctu_patch_index(const uint8_t* labels, int M, int64_t V, int K, const int* classes, int32_t* counts, void* stream);
int ctu_patch_draw(const uint8_t* labels, const int32_t* counts, int M, int D, int H, int W, int K, const int* classes,
                   const int32_t* items, int P, int64_t* counter, uint64_t seed, const int* patch, const int* jitter,
                   const double* cum, int32_t* coords, int32_t* records, void* stream);
int ctu_patch_crop(const void* src, int src_dtype, int Ms, int C, int D, int H, int W, const int32_t* coords, int P, int pd,
                   int ph, int pw, double fill, void* out, int out_dtype, int Ctot, int out_channel, void* stream);

/* Random spatial augmentation (flip, cubic B-spline elastic deformation, affine) of a batch in[N][C][D][H][W], uint8
 * (CTU_U8) or float32 (CTU_F32), nearest-neighbour with fill 0; rule, Philox streams and arithmetic order are pinned in
 * ctunet_amd/transforms.py ("RandomSpatial").  Two launches, no atomics, no host sync:
 *   draw: one block per sample writes record [N][CTU_SPATIAL_RECORD] and control [N][3][gz][gy][gx] (float64, DEVICE) from
 *         the DEVICE sample counter seq (int64 [1], read only); sample n uses sequence number seq + n.  spacing: HOST
 *         (z, y, x) mm.  flip_mask: bit a set = axis a may flip.  ranges: HOST double [11] = scale lo, hi, degrees (z, y, x),
 *         translation (z, y, x) mm, max_displacement (z, y, x) mm.  locked: outer control layers held at 0 (0..2, 2 locked <
 *         every g).  CTU_SPATIAL_MIN_POINTS <= g <= CTU_SPATIAL_MAX_POINTS per axis.
 *   warp: one pass; all C <= 64 channels of a sample share its warp.  Reads record and control, advances seq by N.
 *         out may not be in.  Dynamic LDS: 3 gz gy gx doubles.
 * record: 0-2 flip z, y, x (0 / 1)  3 affine applied  4 elastic applied  5-7 scales  8-10 angles about z, y, x (degrees)
 *         11-13 translation (mm)  14-25 M [3][4] row-major, output world -> input world (the exact identity when 3 is 0) */
#define CTU_SPATIAL_RECORD 26
#define CTU_SPATIAL_MIN_POINTS 4
#define CTU_SPATIAL_MAX_POINTS 12
int ctu_spatial_draw(int N, int D, int H, int W, const double* spacing, const int64_t* seq, uint64_t seed, int flip_mask,
                     double flip_p, double affine_p, double elastic_p, const double* ranges, int gz, int gy, int gx,
                     int locked, double* record, double* control, void* stream);
int ctu_spatial_warp(const void* in, int dtype, int N, int C, int D, int H, int W, const double* spacing, int gz, int gy,
                     int gx, const double* record, const double* control, int64_t* seq, void* out, void* stream);

/* Irregular craniectomy defects (a union of rough balls, in millimetres) and random dilation of binary skulls; rules,
 * Philox streams and arithmetic order are pinned in ctunet_amd/transforms.py ("SkullRandomDefect", "RandomDilate").  Skulls
 * as for the flap entry points above: [N,1,D,H,W] float32 (u8 = 0) or uint8 (u8 = 1), bone = nonzero uint8 cast.
 *   draw:  after ctu_flap_count (counts).  One block per sample writes record [N][CTU_DEFECT_RECORD] and lattice
 *          [N][gz][gy][gx] (float64, DEVICE) from the DEVICE sample counter seq (int64 [1], read only); sample n uses
 *          sequence number seq + n.  spacing: HOST (z, y, x) mm.  ranges: HOST double [6] = radius lo, hi (mm), spread,
 *          shrink lo, hi, roughness amplitude (mm).  balls_lo .. balls_hi (inclusive) within 1..CTU_DEFECT_MAX_BALLS;
 *          2 <= g <= CTU_DEFECT_MAX_LATTICE per axis.
 *   apply: ctu_flap_apply's pass (same x / atlas / full / flap / counters / density contract) with the record's defect as
 *          the hole.  mode: CTU_FLAP_HOLE, or CTU_FLAP_HOLE | CTU_FLAP_NOISE with params = ctu_flap_draw's records in
 *          CTU_FLAP_NOISE mode.  scale: the lattice pitch (mm), amp: the roughness amplitude (mm).  Advances hole_seq
 *          (the defect's counter) and the noise state.
 * record (float64): 0 drawn (u < p)  1 bone count  2 k  3-5 centre z, y, x (-1 without bone)  6 balls K  7 cut (drawn
 *         and count > 0)  8-10 box lo z, y, x  11-13 box hi z, y, x (inclusive; lo 0, hi -1 without bone)  14-15 zero
 *         16 + 4 j .. 19 + 4 j: ball j < K = centre z, y, x and radius (mm), zero for j >= K and without bone
 *   dilate: out [N,1,D,H,W] uint8 = bone dilated by `iterations` (1..CTU_DILATE_MAX_ITERATIONS) steps of the 6-neighbour
 *          cross (the L1 ball of that radius, border 0) for the samples whose draw u < p, bone itself for the others.  in:
 *          CTU_U8 or CTU_F32, not out.  One gather launch, then a one-thread launch that advances seq by N. */
#define CTU_DEFECT_RECORD 64
#define CTU_DEFECT_MAX_BALLS 12
#define CTU_DEFECT_MAX_LATTICE 64
#define CTU_DILATE_MAX_ITERATIONS 3
int ctu_defect_draw(const void* skull, int u8, int N, int D, int H, int W, const double* spacing, const int32_t* counts,
                    const int64_t* seq, uint64_t seed, double p, const double* ranges, int balls_lo, int balls_hi, int gz,
                    int gy, int gx, double* record, double* lattice, void* stream);
int ctu_defect_apply(const void* skull, int u8, const float* atlas, int N, int D, int H, int W, const double* spacing,
                     const double* record, const double* lattice, int gz, int gy, int gx, double scale, double amp,
                     const int32_t* params, int mode, int64_t* hole_seq, int64_t* noise_seq, float* noise_nd,
                     uint64_t noise_seed, int decay, float* x, int C, float* full, float* flap, void* stream);
int ctu_random_dilate(const void* in, int dtype, int N, int D, int H, int W, int iterations, int64_t* seq, uint64_t seed,
                      double p, uint8_t* out, void* stream);

/* ------------------------------------------------ reduced precision (bf16 / fp16 activations) ---- */
/* BASELINE configs 4 ("bf16, 192^3 patches") and 5 ("fp16 MFMA conv path, 256^3 patches").  Same operations, call sites
 * and argument meaning as the fp32 entry points above, with
 *   dtype ............ CTU_BF16 | CTU_F16: element type of every ACTIVATION / activation-gradient tensor (void*), still
 *                      channels-last with channel counts padded to 8 and channel strides in ELEMENTS (multiples of 8)
 *   arithmetic ....... fp32: MFMA accumulators (v_mfma_f32_16x16x32_{bf16,f16}), lazy BatchNorm transform, statistics
 *                      (taken from the ROUNDED outputs), weight / bias / BatchNorm gradients, master weights
 *   packed weights ... 16-bit copies in MFMA fragment order, re-packed from the fp32 masters (ctu_lp_pack_*)
 * fp16 gradients need the caller's loss scaling (the per-voxel loss gradient of a 256^3 patch is 6e-8); bf16 does not. */
/* packed-weight layouts: 0 = [K-step][16-wide out tile][lane][8]; 1 ("pair": k = 3, 8 padded channels on both sides, W >= 32) =
 * (w-shift, channel) rows, a K-step = the 4 w offsets of one (kd, kh) row.  ctu_lp_conv3d_layout returns the layout the forward /
 * data-gradient kernel wants; pack, num_blocks and forward must be given the same one. */
int ctu_lp_conv3d_layout(int k, int rin_p, int nout_p, int W);
size_t ctu_lp_conv3d_packed_elems(int k, int rin_p, int nout_p);
int ctu_lp_conv3d_num_blocks(int N, int D, int H, int W, int k, int rin_p, int nout_p, int layout);
int ctu_lp_pack_conv3d_weight(int dtype, const float* w, void* wp, int Co, int Ci, int k, const int32_t* cinv,
                              int rin_p, int nout_p, int mode, int layout, void* stream);
/* every 16-bit weight copy of a network in ONE launch (ctu_pack_job as above; `layout` unused, kind 1 = ConvTranspose3d) */
int ctu_lp_pack_batch(int dtype, const ctu_pack_job* jobs, int n, void* stream);
/* nn.Conv3d forward (mode-0 packing) / data gradient (mode-1 packing); stats: [ctu_lp_conv3d_num_blocks()][2][nout_p]
 * (the voxel box of a launch grows when rin_p is small, so the row count depends on it) */
int ctu_lp_conv3d_fwd(int dtype, const void* in, int in_cs, int rin_p, const float* in_scale, const float* in_shift,
                      int in_relu, const void* wp, const float* bias, int nbias, void* out, int out_cs, int nout_p,
                      float* stats, int N, int D, int H, int W, int k, int layout, const ctu_bn_tail* tail, void* stream);
/* weight gradient -> dw fp32 [Co,Ci,k,k,k] (torch layout); ws: ctu_lp_conv3d_wgrad_ws_floats() floats */
size_t ctu_lp_conv3d_wgrad_ws_floats(int N, int D, int H, int W, int k, int cin_p, int cout_p);
int ctu_lp_conv3d_wgrad(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                        int in_relu, const void* gout, int g_cs, int cout_p, float* dw, int Co, int Ci,
                        const int32_t* cinv, float* ws, int N, int D, int H, int W, int k, void* stream);
/* ctu_conv3d_wgrad_bn for 16-bit tensors (BatchNorm + ReLU backward folded into the weight-gradient kernel's staging; the
 * raw-output gradient is rounded once to the storage type and written to gy_out): k = 3, volumes at least 16 wide that are
 * multiples of the 4 x 4*(32/bw) x bw box (ctu_lp_conv3d_wgrad_bn_supported). */
int ctu_lp_conv3d_wgrad_bn_supported(int N, int D, int H, int W, int k, int cin_p, int cout_p);
int ctu_lp_conv3d_wgrad_bn(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                           int in_relu, const void* ga, int g_cs, int cout_p, const void* y, const float* bn_scale,
                           const float* bn_shift, const float* coef, void* gy_out, float* dw, int Co, int Ci,
                           const int32_t* cinv, float* ws, int N, int D, int H, int W, int k, void* stream);

/* first encoder convolution (C_in <= 2): the input x and dx stay fp32 NCDHW, the 8-channel side tensor is 16-bit */
int ctu_lp_conv3d_first_fwd(int dtype, const float* x, int cin, const float* w, const float* bias, int nbias, void* out,
                            int out_cs, int Co, float* stats, int N, int D, int H, int W, const ctu_bn_tail* tail, void* stream);
int ctu_lp_conv3d_first_bwd_data(int dtype, const void* g, int g_cs, const float* w, int cin, int Co, float* dx, int N,
                                 int D, int H, int W, void* stream);
int ctu_lp_conv3d_first_wgrad(int dtype, const float* x, int cin, const void* g, int g_cs, float* dw, int Co, float* ws,
                              int N, int D, int H, int W, void* stream);
/* the same data gradient on the matrix pipe (volumes at least 32 wide, cin <= 4): an 8 -> 8 "pair"-layout launch whose first
 * cin outputs are stored as the float32 planes of dx.  wp = ctu_lp_pack_conv3d_weight(w, Co, Ci = cin, k = 3, rin_p = 8,
 * nout_p = 8, mode 1, layout 1).  78 -> 33 us at 128^3 (cin 1), 0.70 -> 0.29 ms at 256^3 (cin 2), measured. */
/* kernel symbol a 16-bit forward / weight-gradient launch of this geometry runs (measurement tags, as ctu_conv3d_*_kernel_name) */
const char* ctu_lp_conv3d_fwd_kernel_name(int N, int D, int H, int W, int k, int rin_p, int nout_p, int layout);
const char* ctu_lp_conv3d_wgrad_kernel_name(int D, int H, int W, int k, int cin_p, int cout_p);
int ctu_lp_conv3d_first_bwd_data_pair_supported(int cin, int W);
int ctu_lp_conv3d_first_bwd_data_pair(int dtype, const void* g, int g_cs, const void* wp, int cin, float* dx,
                                      int N, int D, int H, int W, void* stream);
/* ConvTranspose3d(C, C, 2, 2) + bias; packing mode 0 forward / 1 data gradient (different sizes: packed_elems(mode)) */
size_t ctu_lp_convt_packed_elems(int rin_p, int nout_p, int mode);
int ctu_lp_pack_convt_weight(int dtype, const float* w, void* wp, int Ci, int Co, const int32_t* cinv, int rin_p,
                             int nout_p, int mode, void* stream);
int ctu_lp_convt2_fwd(int dtype, const void* in, int in_cs, int rin_p, const float* in_scale, const float* in_shift,
                      int in_relu, const void* wp, const float* bias, int nbias, void* out, int out_cs, int nout_p,
                      int N, int D, int H, int W, void* stream);
int ctu_lp_convt2_bwd_data(int dtype, const void* gout, int g_cs, int rout_p, const void* wp, void* gin, int gin_cs,
                           int nin_p, int N, int D, int H, int W, void* stream);
size_t ctu_lp_convt2_wgrad_ws_floats(int N, int D, int H, int W, int cin_p, int cout_p);
/* dw only (fp32 [Ci,Co,2,2,2]); the bias gradient is ctu_lp_channel_sum of gout */
int ctu_lp_convt2_wgrad(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                        int in_relu, const void* gout, int g_cs, int cout_p, float* dw, int Ci, int Co,
                        const int32_t* imap, float* ws, int N, int D, int H, int W, void* stream);
/* Launch plans of the three (host only, as ctu_convt2_plan; T in the name stands for the 16-bit type).
 *  ctu_lp_convt2_plan ......... plan[2] = grid.x, grid.y
 *  ctu_lp_convt2_wgrad_plan ... plan[4] = grid.x (slabs per tile pair), grid.y, 128-voxel chunks per block, dynamic LDS bytes */
const char* ctu_lp_convt2_plan(int mode, int rin_p, int nout_p, int N, int D, int H, int W, int* plan);
const char* ctu_lp_convt2_wgrad_plan(int cin_p, int cout_p, int N, int D, int H, int W, int* plan);
/* HBM-bound glue: same kernels as the fp32 entry points, instantiated for 16-bit storage */
/* 16-bit fused decoder up-convolution (upconv_lp.hip; ConvTranspose3d(C,C,2,2) -> Conv3d(C,Co<=8,3,p=1), models.py:37-38) on
 * v_mfma_f32_16x16x32_{bf16,f16}: the twins of ctu_upconv_fused_fwd / _wgrad / _project / _bwd_data for 16-bit tensors.
 * Supported: 8 padded output channels, input channels a multiple of 32, coarse width >= 16 (the decoder's top level of the
 * shipped nets); other geometries take the unfused ctu_lp_convt2_* + ctu_lp_conv3d_* kernels.  N, D, H, W: COARSE dims.
 *  pack ....... wp32 = ctu_upconv_fused_pack's fp32 packing (cin_p, nout_p = 8) -> wp16 [ctu_lp_upconv_fused_packed_elems]
 *               (forward fragments, then data-gradient fragments), rounded once from the fp32 composite weights
 *  fwd ........ out (fine grid, 8 channels, raw) + stats [ctu_lp_upconv_fused_num_blocks][2][8] of the ROUNDED outputs
 *  wgrad ...... dweff fp32 [8][8][cin_p][8] (gradient channel stride must be 8); then ctu_lp_upconv_fused_project
 *  bwd_data ... gin (coarse, cin_p channels) from the fine-grid raw-output gradient */
int ctu_lp_upconv_fused_supported(int k, int D, int H, int W, int cin_p, int nout_p);
size_t ctu_lp_upconv_fused_packed_elems(int cin_p);
int ctu_lp_upconv_fused_num_blocks(int N, int D, int H, int W);
int ctu_lp_upconv_fused_pack(int dtype, const float* wp32, int cin_p, void* wp16, void* stream);
int ctu_lp_upconv_fused_fwd(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                            int in_relu, const void* wp16, const float* beff, void* out, int out_cs, float* stats,
                            int N, int D, int H, int W, void* stream);
size_t ctu_lp_upconv_fused_wgrad_ws_floats(int N, int D, int H, int W, int cin_p);
int ctu_lp_upconv_fused_wgrad(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                              int in_relu, const void* gout, int g_cs, float* dweff, float* ws, int N, int D, int H,
                              int W, void* stream);
/* ... with the BatchNorm + ReLU backward of the fused op's output folded in (as ctu_lp_conv3d_wgrad_bn): gy_out feeds
 * ctu_lp_upconv_fused_project and ctu_lp_upconv_fused_bwd_data */
int ctu_lp_upconv_fused_wgrad_bn_supported(int N, int D, int H, int W, int cin_p);
int ctu_lp_upconv_fused_wgrad_bn(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                                 int in_relu, const void* ga, int g_cs, const void* y, const float* bn_scale,
                                 const float* bn_shift, const float* coef, void* gy_out, float* dweff, float* ws,
                                 int N, int D, int H, int W, void* stream);
int ctu_lp_upconv_fused_project(int dtype, const float* dweff, const void* gout, int g_cs, int nout_p, int N, int D, int H,
                                int W, const float* bt, const float* pack_ws, const int32_t* imap, int C, int Co, int cin_p,
                                float* dwt, float* dbt, float* dw3, float* ws, void* stream);
int ctu_lp_upconv_fused_bwd_data(int dtype, const void* gout, int g_cs, const void* wp16, void* gin, int gin_cs, int cin_p,
                                 int N, int D, int H, int W, void* stream);
int ctu_lp_ncdhw_to_ndhwc(int dtype, const float* src, void* dst, int N, int C, int D, int H, int W, int cp, int cs,
                          void* stream);
int ctu_lp_ndhwc_to_ncdhw(int dtype, const void* src, float* dst, int N, int C, int D, int H, int W, int cs,
                          void* stream);
int ctu_lp_bn_relu_bwd_reduce(int dtype, const void* y, int y_cs, const void* ga, int g_cs, int cp, const float* scale,
                              const float* shift, const float* mean, const float* invstd, int64_t nvox,
                              float* partials, const ctu_bn_bwd_tail* tail, void* stream);
int ctu_lp_bn_relu_bwd_apply(int dtype, const void* y, int y_cs, void* ga, int g_cs, int cp, const float* scale,
                             const float* shift, const float* mean, const float* invstd, const float* coef,
                             int64_t nvox, void* stream);
int ctu_lp_maxpool2_fwd(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                        int in_relu, void* out, int out_cs, int N, int D, int H, int W, void* stream);
int ctu_lp_maxpool2_bwd(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                        int in_relu, const void* gout, int gout_cs, void* gin, int gin_cs, int accumulate,
                        int N, int D, int H, int W, void* stream);
int ctu_lp_maxpool2_bwd_bn(int dtype, const void* in, int in_cs, int cp, const float* in_scale, const float* in_shift,
                           const float* mean, const float* invstd, const void* gout, int gout_cs, void* gin,
                           int gin_cs, int accumulate, int N, int D, int H, int W, float* partials, const ctu_bn_bwd_tail* tail, void* stream);
int ctu_lp_skip_add(int dtype, const void* a, int a_cs, const float* a_scale, const float* a_shift, int a_relu,
                    const void* b, int b_cs, const float* b_scale, const float* b_shift, int b_relu,
                    void* out, int out_cs, int cp, int64_t nvox, void* stream);
int ctu_lp_channel_sum(int dtype, const void* x, int cs, int cp, int64_t nvox, float* partials, float* out, int C,
                       void* stream);
/* head: 16-bit input / input gradient, fp32 NCDHW outputs and output gradients (the loss stays fp32).
 * ctu_lp_head_bwd_bn's gscale multiplies the incoming output gradients g0 / g1 as they are read: the float16 loss scale
 * (1 otherwise) -- everything the launch produces is linear in them, so no scaled copy of the two output-sized maps is made. */
int ctu_lp_head_fwd(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                    int in_relu, const float* w, const float* bias, const int32_t* imap, int Ci, int Co, int act,
                    int head_mode, float* out0, float* out1, int N, int64_t nvox_per_item, void* stream);
int ctu_lp_head_bwd_bn(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                       int in_relu, const float* w, const float* bias, const int32_t* imap, int Ci, int Co, int act,
                       int head_mode, const float* g0, const float* g1, void* gin, int gin_cs, float* dw,
                       float* db, float* ws, int N, int64_t nvox_per_item, const float* bn_mean,
                       const float* bn_invstd, int bn_cp, float* bn_partials, const ctu_bn_bwd_tail* tail, float gscale,
                       void* stream);
/* ctu_lp_head_bwd_bn with the loss scale read from DEVICE memory (gscale: float[1], the dynamic loss scale of
 * ctu_loss_scale_update), so a captured graph multiplies by the scale current at replay time. */
int ctu_lp_head_bwd_bn_dscale(int dtype, const void* in, int in_cs, int cin_p, const float* in_scale, const float* in_shift,
                              int in_relu, const float* w, const float* bias, const int32_t* imap, int Ci, int Co, int act,
                              int head_mode, const float* g0, const float* g1, void* gin, int gin_cs, float* dw,
                              float* db, float* ws, int N, int64_t nvox_per_item, const float* bn_mean,
                              const float* bn_invstd, int bn_cp, float* bn_partials, const ctu_bn_bwd_tail* tail,
                              const float* gscale, void* stream);
/* The two-segment forms of the three entries above (see ctu_head_fwd_seg2). */
int ctu_lp_head_fwd_seg2(int dtype, const void* in_a, int cs_a, const void* in_b, int cs_b, int cp,
                         const float* in_scale, const float* in_shift, int in_relu, const float* w, const float* bias,
                         const int32_t* imap, int Ci, int Co, int act, int head_mode, float* out0, float* out1, int N,
                         int64_t nvox_per_item, void* stream);
int ctu_lp_head_bwd_bn_seg2(int dtype, const void* in_a, int cs_a, const void* in_b, int cs_b, int cp,
                            const float* in_scale, const float* in_shift, int in_relu, const float* w, const float* bias,
                            const int32_t* imap, int Ci, int Co, int act, int head_mode, const float* g0,
                            const float* g1, void* gin_a, int gcs_a, void* gin_b, int gcs_b, float* dw, float* db,
                            float* ws, int N, int64_t nvox_per_item, const float* bn_mean, const float* bn_invstd,
                            int bn_cp, float* bn_partials, const ctu_bn_bwd_tail* tail, float gscale, void* stream);
int ctu_lp_head_bwd_bn_dscale_seg2(int dtype, const void* in_a, int cs_a, const void* in_b, int cs_b, int cp,
                                   const float* in_scale, const float* in_shift, int in_relu, const float* w,
                                   const float* bias, const int32_t* imap, int Ci, int Co, int act, int head_mode,
                                   const float* g0, const float* g1, void* gin_a, int gcs_a, void* gin_b, int gcs_b,
                                   float* dw, float* db, float* ws, int N, int64_t nvox_per_item, const float* bn_mean,
                                   const float* bn_invstd, int bn_cp, float* bn_partials, const ctu_bn_bwd_tail* tail,
                                   const float* gscale, void* stream);
/* Every tensor of a list scaled in place by s (one launch): un-scaling of loss-scaled fp16 gradients.
 * ptrs: HOST array of n DEVICE float pointers, sizes: HOST int64[n].  nonfinite_flag: NULL or a DEVICE float[1] that is set
 * to 1 when any scaled value is inf / NaN (the fp16 backward overflowed; the caller zeroes it per step and hands it to
 * ctu_adam_amsgrad as skip_flag, what torch.amp.GradScaler does with found_inf).
 * Refused before any launch (CTU_EINVAL; no tensor of the list is touched, ctu_unscale_tensors likewise): null ptrs /
 * sizes, n <= 0, and for ANY tensor of the list a null pointer, a negative size or a pointer that is not 4-byte aligned. */
int ctu_scale_tensors(void* const* ptrs, const int64_t* sizes, int n, float s, float* nonfinite_flag, void* stream);
/* Dynamic loss scaling (float16), the device-resident form of torch.amp.GradScaler; every operand is DEVICE memory, so
 * the calls work unchanged inside a replayed graph.
 *   ctu_unscale_tensors ... ctu_scale_tensors by 1 / scale[0] (formed as float(1.0 / (double)scale[0]), GradScaler's
 *                           reciprocal); SETS found_inf (float[1]) on inf / NaN and never clears it, so several backward
 *                           passes of one step accumulate into it
 *   ctu_loss_scale_update . torch._amp_update_scale_ (one thread): found_inf != 0 -> scale *= backoff, growth_tracker = 0;
 *                           else growth_tracker += 1, and when it reaches `interval`: scale *= growth if the product is
 *                           finite in float32, growth_tracker = 0.  Then skipped[0] += 1 if found_inf was set, and
 *                           found_inf = 0 (the only place it is cleared).  growth > 1, 0 < backoff < 1, interval >= 1. */
int ctu_unscale_tensors(void* const* ptrs, const int64_t* sizes, int n, const float* scale, float* found_inf, void* stream);
int ctu_loss_scale_update(float* scale, int32_t* growth_tracker, float* found_inf, float* skipped, float growth,
                          float backoff, int interval, void* stream);

/* --------------------------------------------------------------- gradient exchange (RCCL over xGMI) ---- */
/* One process per GPU; the only cross-GPU step of the path is the mean of the parameter gradients before the optimizer
 * step.  Replaces nn.DataParallel's replicate / scatter / gather / reduce-add (ctunet/pytorch/Model.py:481-487).
 *   ctu_comm_available ... 1 if librccl could be bound (it is dlopen'ed by soname on first use; no link-time dependency)
 *   ctu_comm_unique_id ... HOST buffer of CTU_COMM_ID_BYTES, filled on ONE rank and handed to the others by the caller
 *                          (any side channel: a torch.distributed store / broadcast, MPI, a file)
 *   ctu_comm_init ........ collective over all ranks (ncclCommInitRank) on the calling thread's current HIP device
 *   ctu_comm_allreduce_f32 ncclAllReduce(sum | avg) of `count` floats on the caller's stream; send == recv allowed;
 *                          returns without synchronising.  Not capturable: launch it between graph segments.
 *   ctu_comm_destroy ..... ncclCommDestroy */
#define CTU_COMM_ID_BYTES 128
int ctu_comm_available(void);
int ctu_comm_unique_id(void* id_host);
int ctu_comm_init(void** comm, int world, int rank, const void* id_host);
int ctu_comm_allreduce_f32(void* comm, const float* send, float* recv, size_t count, int average, void* stream);
int ctu_comm_destroy(void* comm);

/* Per-channel sum over voxels of a channels-last tensor: out[c] = sum_v x[v,c] (bias grads). */
int ctu_channel_sum_num_blocks(int64_t nvox);
int ctu_channel_sum(const float* x, int cs, int cp, int64_t nvox, float* partials,
                    float* out, int C, void* stream);
/* Fused multi-tensor Adam / AdamW with amsgrad (torch.optim.Adam(amsgrad=True) and optim.AdamW,
 * Model.py:514-527).  ptrs: HOST array of 5*n DEVICE pointers {param, grad, exp_avg, exp_avg_sq,
 * max_exp_avg_sq} (copied into the kernel arguments, 64 tensors per launch); sizes: HOST int64[n].
 * step: DEVICE float[1] step counter, incremented by this call before it is used (so a captured graph
 * keeps advancing the bias corrections).  decoupled != 0: AdamW weight decay.  skip_flag: NULL or a DEVICE float[1];
 * non-zero = skip this update entirely (parameters, moments and the step counter untouched): an overflowed fp16 step.
 * Refused before any launch (CTU_EINVAL; neither the step counter nor any tensor is touched): null ptrs / sizes / step,
 * n <= 0, and for ANY tensor of the list a null pointer in one of its five slots, a negative size or a pointer that is
 * not 4-byte aligned.  The rule of every entry point that takes a tensor list (ctu_adam_amsgrad_dev, ctu_sgd, ctu_rmsprop,
 * ctu_grad_clip_coef, ctu_scale_tensors, ctu_unscale_tensors): the whole list is checked first. */
int ctu_adam_amsgrad(void* const* ptrs, const int64_t* sizes, int n, float* step,
                     double lr, double beta1, double beta2, double eps, double weight_decay,
                     int decoupled, const float* skip_flag, void* stream);

/* --------------------------------------------------------------- train controls kept on the device ---- */
/* Learning rate, gradient clipping and the plateau schedule as DEVICE operands, so a captured graph replays the values
 * current at replay time.  No allocation, no host sync, no float atomics; results are reproducible call to call.
 *   ctu_adam_amsgrad_dev ..... ctu_adam_amsgrad with lr = (float)lr[0] read on the device (lr: DEVICE double[1], rounded
 *                              where the host call rounds its argument).  grad_coef: NULL or a DEVICE float[1]; every
 *                              gradient value is multiplied by it (one IEEE multiply) before weight decay, what
 *                              clip_grad_norm_ does to p.grad.  With grad_coef NULL or *grad_coef == 1 the result is
 *                              bit-equal to ctu_adam_amsgrad at the same learning rate.  Refuses what ctu_adam_amsgrad
 *                              refuses, and a null lr, before any launch.
 *   ctu_grad_norm_num_blocks . number of floats ctu_grad_clip_coef needs in partials_ws for these sizes (0: bad argument)
 *   ctu_grad_clip_coef ....... global 2-norm of n gradient tensors (gptrs: HOST array of n DEVICE float pointers, 4-byte
 *                              aligned; sizes: HOST int64[n]) and torch's clip coefficient:
 *                              norm_out[0] = (float)sqrt(sum g*g), summed in double in a fixed order;
 *                              coef_out[0] = min(1, max_norm / (norm + 1e-6f)) in float32, NaN if the norm is NaN and 0 if
 *                              it is inf (clip_grad_norm_ with error_if_nonfinite=False).  A null or misaligned pointer
 *                              or a negative size anywhere in the list is refused before any launch.
 *   ctu_plateau_update ....... torch.optim.lr_scheduler.ReduceLROnPlateau.step((double)metric[0]) for one parameter group
 *                              on one thread, in double.  lr: DEVICE double[1]; state: DEVICE double[1] = best (the host
 *                              seeds +inf for min mode, -inf for max mode); counters: DEVICE int32[4] = {num_bad_epochs,
 *                              cooldown_counter, last_epoch, reductions applied}.  mode_max / threshold_rel select the
 *                              four is-better forms; the reduced rate max(lr * factor, min_lr) is applied only if
 *                              lr - new > eps. */
int ctu_adam_amsgrad_dev(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr, double beta1,
                         double beta2, double eps, double weight_decay, int decoupled, const float* grad_coef,
                         const float* skip_flag, void* stream);
int ctu_grad_norm_num_blocks(const int64_t* sizes, int n);
int ctu_grad_clip_coef(void* const* gptrs, const int64_t* sizes, int n, float max_norm, float* partials_ws, float* norm_out,
                       float* coef_out, void* stream);
int ctu_plateau_update(const float* metric, double* lr, double* state, int32_t* counters, int mode_max, int threshold_rel,
                       double factor, int patience, double threshold, int cooldown, double min_lr, double eps, void* stream);

/* --------------------------------------------------------------- SGD and RMSprop ---- */
/* torch.optim.SGD and torch.optim.RMSprop over a list of float32 tensors with the device-side train controls of
 * ctu_adam_amsgrad_dev: one step-counter launch plus one launch per 64 tensors, graph-capturable, fp32 arithmetic in the
 * order written below (g + wd*p is one fused multiply-add, as in ctu_adam_amsgrad; nothing else is contracted).
 *   ptrs ....... HOST array of K*n DEVICE pointers, K per tensor: {param, grad, momentum_buffer} for ctu_sgd (K = 3),
 *                {param, grad, square_avg, momentum_buffer, grad_avg} for ctu_rmsprop (K = 5).  4-byte alignment is
 *                enough (a view at an odd float offset); 16-byte accesses are used where a tensor's pointers share their
 *                offset within 16 bytes.  A state slot the options do not use (momentum == 0, not centered) may be NULL and
 *                is never dereferenced.
 *   sizes ...... HOST int64[n], elements per tensor (0 allowed).
 *   step ....... DEVICE float[1], incremented by this call before it is used: it counts the APPLIED steps, this one included.
 *   lr_dev, lr . lr_dev != NULL: DEVICE double[1], lr = (float)lr_dev[0], rounded where the host call rounds `lr`;
 *                NULL: the host argument.  Both give bit-equal results at the same rate.
 *   grad_coef .. NULL or DEVICE float[1]: every gradient value is multiplied by it first (ctu_grad_clip_coef's coefficient).
 *   skip_flag .. NULL or DEVICE float[1]; non-zero = nothing is written: no parameter, no state, no step counter.
 * ctu_sgd, per element:      g = coef*grad;  if maximize: g = -g;  if wd != 0: g = g + wd*p
 *                            if momentum != 0:  buf = g on the first applied step (step[0] == 1), which a skipped first
 *                                               step leaves to the next one;  buf = momentum*buf + (1-dampening)*g after it;
 *                                               g = g + momentum*buf if nesterov, else buf
 *                            p = p - lr*g
 * ctu_rmsprop, per element:  g as above;  sq = alpha*sq + (1-alpha)*g*g
 *                            centered: ga = ga + (1-alpha)*(g - ga), avg = sqrtf(sq - ga*ga) + eps;  else avg = sqrtf(sq) + eps
 *                            momentum > 0: buf = momentum*buf + g/avg, p = p - lr*buf;  else p = p - lr*(g/avg)
 * Refused before any launch (non-zero status): null ptrs / sizes / step, n <= 0, a negative size, a null param or grad, a
 * null state pointer the options need, a pointer that is not 4-byte aligned, nesterov without momentum or with dampening. */
int ctu_sgd(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr_dev, double lr, double momentum,
            double dampening, double weight_decay, int nesterov, int maximize, const float* grad_coef,
            const float* skip_flag, void* stream);
int ctu_rmsprop(void* const* ptrs, const int64_t* sizes, int n, float* step, const double* lr_dev, double lr, double alpha,
                double eps, double weight_decay, double momentum, int centered, int maximize, const float* grad_coef,
                const float* skip_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTUNET_HIP_H */
