/* libmia_hip.so -- C ABI of the MI355X (gfx950) UNet-2D training hot path.
 *
 * The reference (trnKhanh/medical-image-analysis) is pure Python on top of torch / torchvision library
 * kernels: it has NO FFI layer of its own for this path.  Each entry point below therefore cites the
 * reference call site whose library kernel(s) it replaces; the Python classes that bind them
 * (medical-image-analysis_amd/{models,losses,transforms,...}) keep the reference's class / argument
 * surface, and INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions
 *   - every pointer is a raw DEVICE pointer unless named host_*; the caller owns all memory
 *     (inputs, outputs, saved statistics, workspaces); the library never allocates or frees
 *   - `stream` is a hipStream_t (0 = null stream); all work is enqueued, nothing synchronises
 *   - activations are NHWC; `dtype` is MIA_F32 or MIA_BF16 and applies to activations and packed
 *     weights; statistics, parameters, gradients of parameters and logits are always fp32
 *   - return 0 on success, negative for argument errors (MIA_EARG / MIA_EUNSUPPORTED), positive =
 *     hipError_t; mia_last_error() returns a thread-local message
 */
#ifndef MIA_HIP_H
#define MIA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MIA_F32 0
#define MIA_BF16 1

int mia_version(void);
const char* mia_last_error(void);

/* ------------------------------------------------------------------ weights / layout */
/* fp32 parameter [D0][D1][taps] -> packed [taps][npad][kpad] (zero padded) in `dtype`.
 * Replaces the cuDNN/MIOpen filter transform behind nn.Conv2d / nn.ConvTranspose2d
 * (src/models/unet/blocks.py:83-90, unet.py:142).  n_from_d0: n indexes D0 (else D1). */
int mia_pack_weight(const float* src, void* dst, int dtype, int d0, int d1, int taps, int npad, int kpad,
                    int n_from_d0, void* stream);
/* The same for every weight of a model in ONE launch (the optimizer rewrites all parameters each step).  descs_dev: device
 * array of `count` records of mia_pack_desc_bytes() bytes each:
 *   { const float* src; void* dst; int d0, d1, taps, npad, kpad, n_from_d0; int brick_begin, bricks_x; }
 * a brick is 16 x 64 (n_from_d0) or 64 x 16 (D0 x D1) source elements; brick_begin = running brick count, bricks_x =
 * bricks along D1; total_bricks = sum over records; bricks cover the PADDED extents. */
int mia_pack_desc_bytes(void);
int mia_pack_weight_batch(const void* descs_dev, int count, int total_bricks, int max_taps, int dtype, void* stream);
/* generic strided (n, c, p) copy with dtype conversion: NCHW <-> NHWC, fp32 <-> bf16
 * (replaces .to(dtype)/.contiguous() at al_trainer.py:1366-1368). */
int mia_relayout(const void* src, int src_dtype, void* dst, int dst_dtype, int n, int c, int64_t hw,
                 int64_t ssn, int64_t ssc, int64_t ssp, int64_t dsn, int64_t dsc, int64_t dsp, void* stream);
/* out = a + b: the residual connection of ResidualBlock (blocks.py:164) */
int mia_add(const void* a, const void* b, void* out, int dtype, int64_t n, void* stream);
/* out[c] (+)= sum over p rows of x[p][c]: bias gradients of Conv2d / ConvTranspose2d. */
/* Dropout2d channel masks (blocks.py:92-96): out[i] = 1/keep with probability keep, else 0 (Philox4x32-10 keyed by seed, offset) */
int mia_dropout_mask(float* out, int64_t n, float keep, uint64_t seed, uint64_t offset, void* stream);
/* the same with seed and base offset read from device memory (seed_base[0], seed_base[1]; the launch uses offset seed_base[1] +
 * rel_offset): for a train step replayed from a captured hipGraph, whose kernel arguments are frozen (training/engine.py graph mode) */
int mia_dropout_mask_dyn(float* out, int64_t n, float keep, const uint64_t* seed_base, uint64_t rel_offset, void* stream);
/* optimizer.zero_grad() (al_trainer.py:1375) on a flat buffer: bytes % 16 == 0, 16-byte aligned */
int mia_zero(void* p, int64_t bytes, void* stream);
/* dst[i] = src[i * stride], fp32 (per-channel sums out of interleaved statistics) */
int mia_gather_f32(const float* src, int64_t stride, float* dst, int n, void* stream);
int mia_colsum_workspace(int64_t p, int c); /* floats */
int mia_colsum(const void* x, int dtype, int64_t p, int c, float* workspace, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------ dense conv products (MFMA) */
#define MIA_CONV_G3S1 0 /* gather 3x3 s1 p1: Conv2d fwd (blocks.py:83-90) and its input gradient (flip_taps=1) */
#define MIA_CONV_G3S2 1 /* gather 3x3 s2 p1: strided Conv2d fwd (unet.py:58-66, first block of each level) */
#define MIA_CONV_G2S2 2 /* gather 2x2 s2 p0: ConvTranspose2d input gradient (unet.py:142) */
#define MIA_CONV_T3S2 3 /* transposed 3x3 s2: strided Conv2d input gradient */
#define MIA_CONV_T2S2 4 /* transposed 2x2 s2: ConvTranspose2d fwd (unet.py:142, :212) */
#define MIA_CONV_G1 5   /* 1x1: ResidualBlock skip conv (blocks.py:147-153) */
/* Library options: kernel-selection / launch-shape knobs for A/B measurements (process-wide, not part of any reference
 * interface; results never depend on one beyond fp32 summation order).  ONE table (csrc/options.h), each entry read from its
 * environment variable once at first use, stored in an atomic, changed only by mia_set_option; every entry point takes one
 * snapshot per call.  Thread-safe.  Names (env var, default):
 *   conv_bt (MIA_CONV_BT, 1)       wide stride-1 3x3 bf16 convs on the 512-thread big-tile LDS-DMA kernel (0: tile kernel)
 *   conv_bt_order (MIA_CONV_BT_ORDER, 1)   its work-item order: 1 = the channel blocks of a pixel tile run together on one XCD
 *   conv64 (MIA_CONV64, 1)         64 -> 64 channel bf16 3x3 stride-1 launches on the persistent register-weight kernel
 *   conv64_dma (MIA_CONV64_DMA, 1) the 512-thread LDS-DMA 64-channel kernel: 1 = the 64 -> (64 | 64) two-destination input
 *                                  gradient in one pass (measured 7 % faster than two conv64 passes), 2 = also plain
 *                                  64 -> 64 launches (measured 6-11 % slower than conv64_persist_kernel), 0 = never
 *   conv_s2_wide (MIA_CONV_S2_WIDE, 1)   stride-2 3x3 bf16 forward with 128-multiples of output channels on 512-thread
 *                                  workgroups / 16-row tiles: 1 = from 128 input channels on, 2 = always, 0 = never
 *   conv_pw (MIA_CONV_PW, 1)       ConvTranspose 2x2 / stride 2 forward and input gradient (bf16) as one pointwise GEMM on the
 *                                  512-thread LDS-DMA ring (0: the tile kernel, one parity class per workgroup)
 *   conv_pw_s2 (MIA_CONV_PW_S2, 1) stride-2 3x3 bf16 forward as a tap-gathered GEMM on the same ring (needs conv_pw; 1: up to 256
 *                                  input channels, 2: always, 0: tile kernels -- default: -0.16 ms per step in isolation, none inside the step)
 *   conv_xcd / wgrad_xcd (MIA_CONV_XCD / MIA_WGRAD_XCD, 1)   blocks sharing an input tile run on one XCD (0: plain grid order)
 *   wgrad_bt (MIA_WGRAD_BT, 1)     bf16 3x3 stride-1 weight gradients with >= 128 output channels on the 512-thread 128 x 64 block kernel
 *   wgrad_t2 (MIA_WGRAD_T2, 1)     ConvTranspose 2x2 weight gradient (bf16, >= 128 coarse channels) on the 512-thread three-stage ring
 *   wgrad_dma (MIA_WGRAD_DMA, 1)   bf16 3x3 stride-1 weight gradients on the LDS-DMA ring kernel; 0: the register-staged
 *                                  two-workgroups-per-CU kernel
 *   stream_blocks (MIA_STREAM_BLOCKS, 32768)   target block count of the norm / activation streaming passes
 *   stem_mfma (MIA_STEM_MFMA, 1)   matrix-core stem kernel for fp32 images
 *   f32_split (MIA_F32_SPLIT, 2)      fp32 convs / weight gradients of the branch-free tile kernels on the f16 matrix cores: every
 *                                  operand element, scaled by a per-tensor power of two taken from the tensor's max |x| (the amax_*
 *                                  arguments below), enters as h + l (two fp16: 22-23 significand bits), four exact products (value 1) or, in
 *                                  the convs with >= 32 output channels under value 2, the three that matter (h H + h L + l H on
 *                                  32 x 32 tiles; l L <= 2^-24 of the product), fp32 accumulation, exact rescaling.  Accuracy of the exact fp32 MFMA kernels (not bit-identical to
 *                                  them), ~2x on the fp32 training step.  Tensors stay fp32.  A call without the maxima, or value 0,
 *                                  runs the exact fp32 MFMA kernels.
 *   reserve_cus (MIA_RESERVE_CUS, 0)   CUs the persistent kernels leave free (0..64, rounded so that the grids stay
 *                                  multiples of 8): the grids of conv_bt / conv_pw / conv64 / conv64_dma shrink to CUs - k
 *                                  workgroups (same work items: bit-identical results) and mia_wgrad_target_blocks follows
 *                                  (different split-K count: deterministic, not bit-identical across settings).  Set by
 *                                  the data-parallel trainer (training/engine.py) so that RCCL's ring kernels find CUs
 *                                  while a persistent kernel runs (all-reduce overlapped with backward)
 * (16 options.  The measured-and-rejected experiments of rounds 3-4 -- Winograd conv64, conv_pw T3S2, conv_t3_wide, wgrad_narrow, conv_mt8, the
 * column-reduce epilogue -- are no longer in the shipping library: records under profiles/, entry points of the ones a probe still builds in
 * include/mia_hip_experiments.h, compiled with -DMIA_EXPERIMENTS.)
 * Do not change wgrad_* between mia_wgrad_geometry and the mia_conv_wgrad it sizes.  The Python loader applies
 * MIA_OPTIONS="name=value,..." through mia_set_option.  Unknown name: MIA_EARG. */
int mia_set_option(const char* name, int value);
int mia_get_option(const char* name, int* value);
/* out[p][n] = bias[n] + sum_taps sum_k in[p*s + tap - pad][k] * wpack[tap][n][k].
 * in1|in2 are concatenated along channels (c1 + c2) -- this is how torch.cat([skip, up], 1)
 * (unet.py:213) is eliminated; out1|out2 are split along channels (o1 + o2) for its gradient.
 * stat_partials (optional): [N][tiles][o1+o2][2] per-tile sum / sum-of-squares of the output
 * (feeds mia_norm_finalize; replaces the statistics pass of InstanceNorm2d/BatchNorm2d, blocks.py:98).
 * tiles = tiles_y * tiles_x from mia_conv_mma_tiles().  Gather modes only: MIA_EARG with MIA_CONV_T3S2 / MIA_CONV_T2S2, whose four
 * parity classes share one entry per tile. */
int mia_conv_mma_tiles(int mode, int hout, int wout, int* tiles_y, int* tiles_x, int* tile_h);
/* amax_in1 / amax_in2 / amax_w (optional, fp32 tensors only): device pointers to max |x| of in1 / in2 / the weight tensor as fp32
 * bit patterns (mia_amax / mia_amax_batch).  All present (amax_in2 only when c2 > 0) and option f32_split on: the products run on the
 * f16 matrix cores from two-part split operands (see f32_split above); any of them NULL: exact fp32 MFMAs.
 * amax_out1 / amax_out2 (optional, fp32): ZEROED 4-byte slots that receive max |out1| / max |out2| as a by-product (epilogue of the
 * tile kernel, a separate pass for generic shapes) -- for outputs another conv consumes directly (unet.py:142 -> :213 and back). */
int mia_conv_mma(int mode, int dtype, const void* in1, int c1, const void* in2, int c2, const void* wpack, int npad,
                 int kpad, int flip_taps, const float* bias, void* out1, int o1, void* out2, int o2,
                 float* stat_partials, int n, int hin, int win, int hout, int wout, const void* amax_in1, const void* amax_in2,
                 const void* amax_w, const void* wpack_split, void* amax_out1, void* amax_out2, void* stream);
/* Which kernel family mia_conv_mma (variant 0), mia_conv_mma_nl (1) or mia_conv_mma_acc (2) launches for a shape, under the options
 * as they are at the call: the launch path and this query share one selection function, and the query launches nothing.  OR
 * MIA_CONV_VAR_STATS into `variant` for a launch with stat_partials, MIA_CONV_VAR_BIAS for one with a bias (two kernels' contracts
 * read them).  split != 0: the fp32 operand maxima are passed.  Assumes 16-byte aligned tensors of one image (no 2^31-byte limit
 * reached).  Returns MIA_CONV_FAM_*, or a negative error code for a shape the variant rejects. */
#define MIA_CONV_FAM_GENERIC 0    /* conv_mma_kernel: any shape */
#define MIA_CONV_FAM_FAST 1       /* conv_mma_fast: the branch-free tile kernel */
#define MIA_CONV_FAM_S2_WIDE 2    /* conv_mma_fast on 512-thread workgroups / 16-row tiles (option conv_s2_wide) */
#define MIA_CONV_FAM_CONV64 3     /* conv64_persist_kernel */
#define MIA_CONV_FAM_CONV64_DMA 4 /* conv64_dma_kernel */
#define MIA_CONV_FAM_CONV_BT 5    /* conv_bt_kernel */
#define MIA_CONV_FAM_CONV_PW 6    /* conv_pw_kernel */
#define MIA_CONV_FAM_NL 7         /* conv64_persist_kernel, normalise-on-load */
#define MIA_CONV_FAM_ACC 8        /* conv_mma_fast, out += result */
#define MIA_CONV_VAR_STATS 4
#define MIA_CONV_VAR_BIAS 8
int mia_conv_mma_family(int mode, int dtype, int c1, int c2, int o1, int o2, int npad, int kpad, int hout, int wout, int variant,
                        int split);
/* wpack_split (optional, with the maxima): the packed weights already split into (h | l << 16) fp16 words of w * 2^e (e from amax_w's
 * slot) by mia_split_f16_batch -- same [tap][npad][kpad] layout, 4 bytes per weight; the split kernels then stage them as they are instead
 * of splitting them once per tile.  Device table of `count` {const float* src; void* dst; int64_t n; const void* amax;} records
 * (mia_split_desc_bytes() each; n a multiple of 4, 16-byte aligned buffers). */
int mia_split_desc_bytes(void);
int mia_split_f16_batch(const void* descs_dev, int count, void* stream);
/* max |x| of an fp32 tensor of n elements, folded (atomic unsigned maximum of the fp32 bit pattern: order-independent, deterministic)
 * into *slot; reset != 0 zeroes the slot first (stream-ordered, by a kernel: hipMemsetAsync nodes on graph-pool memory were seen to
 * replay wrongly inside a captured step).  The batched form takes a device table of `count`
 * {const float* src; int64_t n;} records (mia_amax_desc_bytes() each) and writes slots[0 .. count): every weight of a model in one
 * launch after the optimizer step.  These maxima are the scale source of the split-f16 products (no reference counterpart: the
 * reference multiplies in fp32, blocks.py:83-90). */
int mia_amax(const float* x, int64_t n, void* slot, int reset, void* stream);
/* dst[i] = src[i], uint8 -> int64: label maps travel host -> device as bytes (1/8 of the int64 tensor `label.to(device)` moves,
 * al_trainer.py:1368) and are widened here for the loss kernels; src 8-byte, dst 16-byte aligned (training/feed.py). */
int mia_widen_u8_i64(const void* src, void* dst, int64_t n, void* stream);
/* HOST helper of the same feed (no device work): dst[i] = (uint8) src[i] over host memory in one multi-threaded pass; returns 1 when
 * every label lies in 0 .. 255 (dst valid), 0 when some label does not fit (ship the int64 tensor instead), < 0 on bad arguments.
 * threads <= 0: 8. */
int mia_host_narrow_labels(const int64_t* src, uint8_t* dst, int64_t n, int threads);
int mia_host_copy(void* dst, const void* src, int64_t bytes, int threads); /* pageable -> pinned memcpy on `threads` (<= 0: 4) plain threads */
int mia_amax_desc_bytes(void);
int mia_amax_batch(const void* descs_dev, int count, void* slots, void* stream);

/* Fused PlainBlock, consumer side ("normalise-on-load"; SURVEY 8b export list: conv3x3 with "optional fused normalise +
 * LeakyReLU on load taking per-(n,c) scale/shift").  Replaces, for a PlainBlock whose only consumer is the next block's conv
 * (the two blocks of one encoder / decoder level, unet.py:54-76, 157-173), the producer's InstanceNorm/BatchNorm + LeakyReLU
 * pass (blocks.py:98-102): y_in is the producer's RAW conv output [N][H][W][c1] and the conv stages
 * x = lrelu(in_scale[n][c] * y + in_shift[n][c]) (fp32 fma, select, round to nearest even: bit for bit what
 * mia_norm_act_fwd would have written), zero padding applied to x.  in_scale / in_shift = the `scale` / `shift` rows that
 * mia_norm_finalize wrote ([N][c1], Dropout2d multipliers folded in).  One source, one destination, forward taps.
 * mia_conv_nl_supported: 1 if a kernel serves the shape (today: 3x3 stride 1, bf16, 64 -> 64 channels, H > 8), else 0 --
 * the caller then materialises the activation with mia_norm_act_fwd and uses mia_conv_mma. */
int mia_conv_nl_supported(int mode, int dtype, int c1, int nout, int hout, int wout);
int mia_conv_mma_nl(int mode, int dtype, const void* y_in, int c1, const float* in_scale, const float* in_shift, float slope,
                    const void* wpack, int npad, int kpad, const float* bias, void* out, int nout, float* stat_partials,
                    int n, int hin, int win, int hout, int wout, void* stream);

/* Fused PlainBlock, backward: the input-gradient conv of the CONSUMING block with the producing block's norm-backward reduction
 * in its epilogue.  out = dz, the gradient w.r.t. the producing block's activated output (what mia_conv_mma computes with
 * flip_taps = 1); y_prod / scale / shift / xa / xb = that block's raw conv output and coefficient rows (mia_norm_finalize).
 * While a tile's accumulators are in registers the kernel adds up g = dz * lrelu'(scale * y + shift) and g * (xa * y + xb) from
 * the bf16-rounded dz it stores, and writes partials [N][tiles][nout][2] (tiles as mia_conv_mma_tiles) -- the input of
 * mia_norm_act_bwd_pre, which then skips its own reduction pass over dz and y (blocks.py:98-102 backward).  3x3 stride 1, bf16,
 * 64 -> 64 channels (mia_conv_cr_supported). */
/* mia_conv_mma with out += result (no bias, one source, one destination; the tile kernel: returns MIA_EUNSUPPORTED outside its
 * contract).  Use: a skip tensor has two consumers (unet.py:213 and the next encoder level), so its gradient arrives in two pieces;
 * the piece computed second -- the stride-2 conv's input gradient, mode CONV_T3S2 -- is added into the first in this launch's
 * epilogue (read-modify-write), and the skip block's norm backward reads one gradient tensor instead of two. */
int mia_conv_acc_supported(int mode, int dtype, int c1, int nout);
int mia_conv_mma_acc(int mode, int dtype, const void* in1, int c1, const void* wpack, int npad, int kpad, int flip_taps,
                     void* out_inout, int nout, int n, int hin, int win, int hout, int wout, const void* amax_in, const void* amax_w,
                     const void* wpack_split, void* stream);


/* Stem: Conv2d(1, C0, 3, padding=1) (first encoder block, unet.py:54-66 with input_channels=1): HBM-streaming VALU
 * kernels (9 FMAs per output; MFMA would idle 31/32 of its K).  x is the [N][H][W] image in x_dtype (fp32 or bf16),
 * y / dy are NHWC in `dtype`; stat_partials [N][mia_stem_slabs()][C0][2]; grad is the [C0][1][3][3] parameter layout. */
int mia_stem_slabs(void);
int mia_stem_wgrad_workspace(int c0); /* floats */
int mia_stem_fwd(const void* x, int x_dtype, const float* w, const float* bias, void* y, int dtype, float* stat_partials, int n,
                 int h, int wd, int c0, void* stream);
int mia_stem_wgrad(const void* x, int x_dtype, const void* dy, int dtype, float* workspace, float* grad, int n, int h, int wd,
                   int c0, int accumulate, void* stream);
/* mia_stem_wgrad with the block's norm + LeakyReLU backward folded in: dz is the gradient w.r.t. the stem block's ACTIVATED
 * output, y its raw conv output, and the kernel forms dy = scale * (g - c1 - xhat * c2), g = dz * lrelu'(scale * y + shift), on
 * load (rounded to `dtype` like the stored dy of mia_norm_act_bwd: same bits).  The stem has no input gradient, so this weight
 * gradient is the only consumer of dy: pair it with mia_norm_bwd_sums and the backward apply pass (read dz + y, write dy) and the
 * read of dy disappear.  scale / shift / xa / xb: mia_norm_finalize's rows; c1 / c2: mia_norm_bwd_sums' outputs. */
int mia_stem_wgrad_fused(const void* x, int x_dtype, const void* dz, const void* y, int dtype, const float* scale,
                         const float* shift, const float* xa, const float* xb, const float* c1, const float* c2, float slope,
                         float* workspace, float* grad, int n, int h, int wd, int c0, int accumulate, void* stream);
/* Input gradient of the stem (csrc/stem_dgrad.hip): dx[n][y][x] = sum_co sum_(a,b) w[co][3a+b] * dy[n][y+1-a][x+1-b][co], dy outside
 * the image = 0; dy NHWC in `dtype` (16-byte aligned), w the [C0][9] fp32 parameter, dx the fp32 [N][H][W] image gradient; fp32
 * accumulation on the matrix cores (bf16: w enters as two bf16 parts, hi + lo).  Eligibility is mia_stem_fwd's: c0 % 8 == 0 (bf16) /
 * c0 % 4 == 0 (fp32), c0 <= 256, any h, wd >= 1.  One stream over dy, no float atomics: bit-identical from run to run.  Every check
 * happens before any launch.  Not fused with the norm backward: the caller materialises dy (mia_norm_act_bwd) first. */
int mia_stem_dgrad(const void* dy, int dtype, const float* w, float* dx, int n, int h, int wd, int c0, void* stream);

#define MIA_WGRAD_3S1 0
#define MIA_WGRAD_3S2 1
#define MIA_WGRAD_2S2 2 /* ConvTranspose2d: x := grad_output (fine grid), dy := layer input (coarse grid) */
/* slabs[z][tap][npad][kpad] = sum over the z-th share of output pixels of dy[p][n] * x[p*s+tap-pad][k]
 * (autograd weight gradient of the layers above); mia_wgrad_reduce sums the ksplit slabs in a fixed
 * order into grad[nn][kk][taps] (= OIHW for Conv2d, [Cin][Cout][2][2] for ConvTranspose2d). */
int mia_wgrad_target_blocks(int mode, int dtype); /* split-K workgroups to aim for (ksplit = target / (npad/64 * kpad/64)) */
int mia_wgrad_geometry(int mode, int dtype, int hy, int wy, int* tiles_y, int* tiles_x);
/* What the caller needs to size ksplit for THIS shape: the column blocks of one split-K slice, the workgroup count to aim for and the
 * tile height (rows of 16 output pixels per split-K step) of the kernel mia_conv_wgrad will pick -- 64-wide channel blocks cut per
 * source, or the 96-wide blocks of 3x3 stride-1 bf16 layers whose channel counts are multiples of 96 and not of 64 (768 threads, one
 * block where the 64-wide form needs 2 x 2).  Supersedes the two queries above for callers that know the channel counts. */
int mia_wgrad_plan(int mode, int dtype, int c1, int c2, int cdy, int npad, int hy, int* column_blocks, int* target_blocks, int* tile_h);
/* Which kernel family mia_conv_wgrad (variant 0) or mia_conv_wgrad_nl (1) launches for a shape, under the options as they are at the
 * call (one selection function shared with the launch path; nothing is launched; 16-byte aligned tensors below 2^31 bytes per image
 * assumed; `split` as for mia_conv_mma_family -- the split product form runs inside the fp32 families).  Returns MIA_WGRAD_FAM_*, or a
 * negative error code for a shape the variant rejects. */
#define MIA_WGRAD_FAM_DMA96 0      /* wgrad_bf16_dma96_kernel */
#define MIA_WGRAD_FAM_BT 1         /* wgrad_bf16_bt_kernel / _s2 / _t2 */
#define MIA_WGRAD_FAM_DMA 2        /* wgrad_bf16_dma_kernel */
#define MIA_WGRAD_FAM_2WG 3        /* wgrad_bf16_2wg_kernel */
#define MIA_WGRAD_FAM_2WG_NL 4     /* wgrad_bf16_2wg_kernel, normalise-on-load */
#define MIA_WGRAD_FAM_TILE_FAST 5  /* wgrad_bf16_fast_kernel */
#define MIA_WGRAD_FAM_F32_FAST 6   /* wgrad_f32_fast_kernel (exact fp32 or split-f16 products) */
#define MIA_WGRAD_FAM_F32_NARROW 7 /* wgrad_f32_fast_kernel on half-width blocks (every channel count <= 32) */
#define MIA_WGRAD_FAM_GENERIC 8    /* wgrad_bf16_kernel / wgrad_f32_kernel: any shape */
int mia_wgrad_family(int mode, int dtype, int c1, int c2, int cdy, int npad, int variant, int split);
int mia_conv_wgrad(int mode, int dtype, const void* x1, int c1, const void* x2, int c2, const void* dy, int cdy,
                   float* slabs, int ksplit, int npad, int kpad, int n, int hx, int wx, int hy, int wy, const void* amax_x1,
                   const void* amax_x2, const void* amax_dy, void* stream); /* amax_*: as for mia_conv_mma */
/* mia_conv_wgrad with normalise-on-load of x (backward half of the fused PlainBlock, see mia_conv_mma_nl): y_in is the raw
 * conv output of the PRODUCING block, x = lrelu(in_scale[n][k] * y + in_shift[n][k]) is formed while the tile is staged (zero
 * outside the image), so the activation the weight gradient of blocks.py:83-90 contracts with is never read from memory.
 * 3x3 stride 1, bf16, one source; slabs / ksplit / reduce exactly as for mia_conv_wgrad. */
int mia_wgrad_nl_supported(int mode, int dtype, int c1, int cdy);
int mia_conv_wgrad_nl(int mode, int dtype, const void* y_in, int c1, const float* in_scale, const float* in_shift, float slope,
                      const void* dy, int cdy, float* slabs, int ksplit, int npad, int kpad, int n, int hx, int wx, int hy,
                      int wy, void* stream);
int mia_wgrad_reduce(const float* slabs, int ksplit, int taps, int npad, int kpad, float* grad, int nn, int kk,
                     int accumulate, void* stream);

/* ------------------------------------------------------------------ Dropout2d + norm + LeakyReLU */
#define MIA_NORM_INSTANCE 0
#define MIA_NORM_BATCH 1
/* per-(n,c) coefficients from conv-epilogue partials: xhat = xa*y + xb, z = lrelu(scale*y + shift).
 * drop_scale [N][C] (0 or 1/(1-p)) folds nn.Dropout2d (blocks.py:92-96); batch mode updates
 * running_mean/var (momentum, unbiased var) and num_batches_tracked like nn.BatchNorm2d. */
int mia_norm_finalize(const float* partials, int n, int tiles, int c, int64_t hw, int mode, int training,
                      const float* drop_scale, const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, long long* num_batches, float* xa, float* xb,
                      float* scale, float* shift, float* ysum, void* stream);
/* stand-alone statistics partials [N][slabs][C][2] when no conv epilogue produced them */
int mia_norm_stats(const void* y, int dtype, int n, int64_t hw, int c, int slabs, float* partials, void* stream);
/* amax_out (nullable; here and in the backward forms below): 4-byte device slot, ZEROED by the caller, into which max |output| is
 * folded as an fp32 bit pattern during the same pass (atomic unsigned maximum; fp32 tensors, ignored for bf16) -- the scale source
 * of the split-f16 convs that consume the output (mia_conv_mma amax_*), so no separate mia_amax pass over it is needed. */
int mia_norm_act_fwd(const void* y, void* z, int dtype, const float* scale, const float* shift, int n, int64_t hw, int c,
                     float slope, void* amax_out, void* stream);
/* dz2 (nullable, here and in the _reduce / _apply_sync forms): a second piece of the output gradient, summed on load --
 * the two consumers of a skip tensor (unet.py:213 and the next encoder level) each deliver one; needs c % 32 == 0
 * (mia_norm_two_piece_ok). */
int mia_norm_two_piece_ok(int dtype, int c);
/* backward of (dropout . norm . lrelu): dy, dgamma, dbeta.  partials: [N][slabs][C][2]; c1, c2: [N][C].
 * dbias (optional, with ysum [N][C] from mia_norm_finalize) = gradient of the Conv2d bias in front of the norm
 * (= sum over pixels of dy) in closed form from the reduction sums: no extra pass over dy. */
int mia_norm_act_bwd(const void* dz, const void* dz2, const void* y, void* dy, int dtype, const float* scale, const float* shift,
                     const float* xa, const float* xb, const float* ysum, int n, int64_t hw, int c, int mode,
                     int fixed_stats, float slope, int slabs, float* partials, float* c1, float* c2, float* dgamma,
                     float* dbeta, float* dbias, int accumulate, void* amax_out, void* stream);
/* mia_norm_act_bwd without its apply pass (no dy is written): reduction + finalize only -- c1 / c2 (group means of g and
 * g * xhat), dgamma, dbeta, dbias.  For a block whose only consumer of dy forms it on load (mia_stem_wgrad_fused). */
int mia_norm_bwd_sums(const void* dz, const void* dz2, const void* y, int dtype, const float* scale, const float* shift,
                      const float* xa, const float* xb, const float* ysum, int n, int64_t hw, int c, int mode,
                      int fixed_stats, float slope, int slabs, float* partials, float* c1, float* c2, float* dgamma,
                      float* dbeta, float* dbias, int accumulate, void* stream);
/* mia_norm_act_bwd with the reduction already done: partials [n][parts][c][2] come from mia_conv_mma_cr.  Sums + finalize; the
 * apply pass (dy = ...) runs only when dy != NULL (NULL: the consumer forms dy on load, mia_stem_wgrad_fused). */

/* Synchronised batch norm for data-parallel runs (build-side addition; SURVEY.md 8e: "a second, small collective"):
 * the caller moves 3*C floats (forward, all-gather) and 2*C floats (backward, all-reduce sum) per layer over RCCL and
 * these entry points do the device work on either side of it, so N ranks x bs reproduce one process at N*bs
 * (BatchNorm2d batch statistics, blocks.py:98).
 *   mia_bn_sync_local_stats : conv-epilogue partials -> per-(n,c) sums parked in xa/xb + local[3][C] = mean, M2, count
 *   mia_norm_finalize_sync  : gathered[world][3][C] -> coefficients / running statistics as mia_norm_finalize(training)
 *   mia_norm_act_bwd_reduce : per-(n,c) sums in c1/c2 + tot[3][C] = local (sum g, sum g*xhat, pixel count)
 *   mia_norm_act_bwd_apply_sync : group_tot[3][C] = the all-reduced (summed) totals; dgamma, dbeta and dbias stay
 *                             LOCAL sums (the gradient all-reduce adds them up). */
int mia_bn_sync_local_stats(const float* partials, int n, int tiles, int c, int64_t hw, const float* drop_scale, float* xa,
                            float* xb, float* local, void* stream);
int mia_norm_finalize_sync(const float* gathered, int world, int n, int c, int64_t hw, const float* drop_scale,
                           const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                           float* running_var, long long* num_batches, float* xa, float* xb, float* scale, float* shift,
                           float* ysum, void* stream);
int mia_norm_act_bwd_reduce(const void* dz, const void* dz2, const void* y, int dtype, const float* scale, const float* shift, const float* xa,
                            const float* xb, int n, int64_t hw, int c, float slope, int slabs, float* partials, float* c1,
                            float* c2, float* tot, void* stream);
int mia_norm_act_bwd_apply_sync(const void* dz, const void* dz2, const void* y, void* dy, int dtype, const float* scale, const float* shift,
                                const float* xa, const float* xb, const float* ysum, int n, int64_t hw, int c, float slope,
                                float* c1, float* c2, const float* group_tot, float* dgamma, float* dbeta, float* dbias,
                                int accumulate, void* amax_out, void* stream);

/* ------------------------------------------------------------------ 1x1 head + Dice/CE loss */
/* seg_output = Conv2d(c0, K1, 1) (unet.py:176), K1 <= 8.  Logits are fp32 with element strides (osn, osk, osp).  mia_head_bwd: dx may
 * be NULL (no input gradient); dw == db == NULL with dx given computes the input gradient alone (workspace is then unused). */
int mia_head_fwd(const void* x, int dtype, const float* w, const float* b, float* logits, int n, int64_t hw, int c0, int k1,
                 int64_t osn, int64_t osk, int64_t osp, void* stream);
int mia_head_bwd_workspace(int c0, int k1); /* floats */
int mia_head_bwd(const float* dlogits, const void* x, int dtype, const float* w, void* dx, float* dw, float* db,
                 float* workspace, int n, int64_t hw, int c0, int k1, int64_t gsn, int64_t gsk, int64_t gsp, int accumulate,
                 void* stream);
#define MIA_LOSS_SOFTMAX 1
#define MIA_LOSS_DO_BG 2
#define MIA_LOSS_BATCH 4
#define MIA_LOSS_SQUARED 8
#define MIA_LOSS_DENSE 16 /* `labels` is a dense fp32 target [B][K1][HW] (already one-hot / class probabilities) instead of int64
                           * indices: DiceLoss skips its one-hot encoder when shapes match (dice_loss.py:40-41) and
                           * torch.nn.CrossEntropyLoss treats such a target as probabilities.  Pass the float pointer cast to
                           * `const long long*`; same strides as the logits (sn, sk, sp). */
/* out[0] = ce_w*CE + dice_w*Dice, out[1] = CE (mean over pixels), out[2] = Dice
 * (DiceLoss.forward dice_loss.py:32-76, DiceAndCELoss.forward compound_losses.py:33-49).
 * sums [B][K1][3] = (I, sum p, sum t); coef [B][K1][2] feeds the backward; bad_label = int[2], zero before the first call: [1] is SET (never
 * cleared by the library: sticky until the caller zeroes it) by a call that met a label outside [0,K1) (loss and coef of THAT call are
 * NaN), [0] = scratch re-armed by every call. */
int mia_dice_ce_workspace(int nb, int k1, int slabs); /* floats */
int mia_dice_ce_fwd(const float* logits, const long long* labels, int nb, int64_t hw, int k1, int64_t sn, int64_t sk,
                    int64_t sp, int flags, float smooth, float dice_w, float ce_w, int slabs, float* workspace, float* sums,
                    float* coef, float* out, int* bad_label, void* stream);
int mia_dice_ce_bwd(const float* logits, const long long* labels, const float* coef, const float* grad_out, float* dlogits,
                    int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp,
                    int flags, float dice_w, float ce_w, void* stream);

/* Deep supervision: the same Dice + CE of an auxiliary head's LOW-resolution logits z [nb][k1][h*w] (element strides sn, sk, sp as above)
 * against FULL-resolution int64 labels [nb][H*W], H = h*factor, W = w*factor, factor in {2, 4, 8, 16}, k1 in 1..8.  The logits are
 * upsampled in registers, u = Uy z Ux^T with U = torch interpolate(scale_factor=factor, mode="bilinear", align_corners=False); the loss is
 * what mia_dice_ce_fwd computes on u (same sums, coef, out, bad_label protocol; MIA_LOSS_DENSE is refused), and the backward writes
 * dz = Uy^T du Ux (du = what mia_dice_ce_bwd would write for u) by gather through dz's own strides (gsn, gsk, gsp).  Neither u nor du is
 * ever stored.  No float atomics: out, sums and dz are bit-identical run to run; no host sync. */
int mia_ds_loss_workspace(int nb, int k1, int slabs); /* floats */
int mia_ds_loss_fwd(const float* z, const long long* labels, int nb, int h, int w, int factor, int k1, int64_t sn, int64_t sk,
                    int64_t sp, int flags, float smooth, float dice_w, float ce_w, int slabs, float* workspace, float* sums,
                    float* coef, float* out, int* bad_label, void* stream);
int mia_ds_loss_bwd(const float* z, const long long* labels, const float* coef, const float* grad_out, float* dz, int nb, int h,
                    int w, int factor, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp, int flags,
                    float dice_w, float ce_w, void* stream);

/* Head fused with the last decoder block (unet.py:176 behind blocks.py:98-100): the block's activation
 * z = lrelu(scale*y + shift) has one consumer, the 1x1 head, so it is never materialised -- the head recomputes it from the
 * raw conv output y on load, and the block's norm backward recomputes dz = W^T dlogits instead of reading it.
 * mia_head_norm_eligible: 0 or the units per pixel; contract c0 in {4,8,12,16} 16-byte units (12 = 96 bf16 channels, on sixteen-lane groups), 2 <= k1 <= 4. */
int mia_head_norm_eligible(int dtype, int n, int64_t hw, int c0, int k1);
int mia_head_norm_fwd(const void* y, int dtype, const float* scale, const float* shift, float slope, const float* w,
                      const float* b, float* logits, int n, int64_t hw, int c0, int k1, int64_t osn, int64_t osk, int64_t osp,
                      void* stream);
int mia_head_norm_wgrad(const float* dlogits, const void* y, int dtype, const float* scale, const float* shift, float slope,
                        float* dw, float* db, float* workspace, int n, int64_t hw, int c0, int k1, int64_t gsn, int64_t gsk,
                        int64_t gsp, int accumulate, void* stream);
int mia_norm_act_bwd_head(const float* dlogits, const float* w, int k1, int64_t gsn, int64_t gsk, int64_t gsp, const void* y,
                          void* dy, int dtype, const float* scale, const float* shift, const float* xa, const float* xb,
                          const float* ysum, int n, int64_t hw, int c, int mode, int fixed_stats, float slope, int slabs,
                          float* partials, float* c1, float* c2, float* dgamma, float* dbeta, float* dbias, int accumulate,
                          void* amax_out, void* stream);
/* mia_norm_act_bwd_head + mia_head_norm_wgrad in ONE reduction pass (both read exactly dlogits and y): the kernel that adds up the
 * block's norm-backward sums also accumulates the head's dW[k][c] = sum_p dl[p][k] * lrelu(scale * y + shift) and db[k] (unet.py:176
 * backward).  c == 64 (mia_head_w_supported); head_workspace: n * slabs * k1 * (c + 1) floats. */
int mia_head_w_supported(int dtype, int c, int k1);
int mia_norm_act_bwd_head_w(const float* dlogits, const float* w, int k1, int64_t gsn, int64_t gsk, int64_t gsp,
                            const void* y, void* dy, int dtype, const float* scale, const float* shift, const float* xa,
                            const float* xb, const float* ysum, int n, int64_t hw, int c, int mode, int fixed_stats,
                            float slope, int slabs, float* partials, float* c1, float* c2, float* dgamma, float* dbeta,
                            float* dbias, int accumulate, float* head_workspace, float* dw_head, float* db_head,
                            int accumulate_head, void* amax_out, void* stream);

/* ------------------------------------------------------------------ fold-trainer losses (src/losses: DC_and_CE_loss, TopKLoss) */
/* Masked soft Dice + (weighted) cross-entropy in one pass, with an ignore label and the hard tp/fp/fn of the arg-max prediction:
 *   valid = (label != ignore_label), p = softmax(logits) (MIA_SEGLOSS_SOFTMAX) or the logits, t = onehot(label) where valid
 *   I = sum valid p t, P = sum valid p, G = #{valid, label = k} per (image, class);  CE = sum valid w[label] nll / sum valid w[label]
 *   dc = -mean_k (2I + smooth) / max(G + P + smooth, 1e-8)  (MemoryEfficientSoftDiceLoss, dice_loss.py:100-165; class 0 dropped without
 *   MIA_SEGLOSS_DO_BG; I, P, G summed over the batch first with MIA_SEGLOSS_BATCH)
 * out[0] = ce_w*CE + dice_w*dc, out[1] = CE (0 when no pixel is valid), out[2] = dc; counts [B][K1][3] = int64 (tp, fp, fn);
 * coef: nb*k1*2 + 1 floats for the backward.  labels: int64 [B][HW], or uint8 with MIA_SEGLOSS_LABEL_U8; class_w: K1 floats or NULL;
 * ignore_label is read only with MIA_SEGLOSS_IGNORE.  A label that is neither a class nor the ignore label: NaN results and the sticky
 * verdict in bad_label[1], exactly as mia_dice_ce_fwd.  Results are bit-identical run to run (no float atomics); no host sync. */
#define MIA_SEGLOSS_SOFTMAX 1
#define MIA_SEGLOSS_DO_BG 2
#define MIA_SEGLOSS_BATCH 4
#define MIA_SEGLOSS_LABEL_U8 8
#define MIA_SEGLOSS_IGNORE 16
int mia_seg_loss_workspace(int nb, int k1, int slabs); /* floats; the buffer must be 8-byte aligned */
int mia_seg_loss_fwd(const float* logits, const void* labels, const float* class_w, int nb, int64_t hw, int k1, int64_t sn,
                     int64_t sk, int64_t sp, int flags, int64_t ignore_label, float smooth, float dice_w, float ce_w, int slabs,
                     float* workspace, float* coef, float* out, int64_t* counts, int* bad_label, void* stream);
int mia_seg_loss_bwd(const float* logits, const void* labels, const float* class_w, const float* coef, const float* grad_out,
                     float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk,
                     int64_t gsp, int flags, int64_t ignore_label, void* stream);
/* TopKLoss (ce_loss.py:18-32): mean of the n_top largest per-pixel losses nll = valid w[label] (logsumexp - logit[label]); ignored
 * pixels count as 0.  The n_top-th largest value tau is found by a radix select over the bit patterns (integer atomics only), then
 * out[0] = (sum_{nll > tau} nll + (n_top - #{nll > tau}) tau) / n_top.  Backward: nll > tau -> w[label] (p - t) / n_top; the m pixels
 * with nll == tau share the remaining n_top - #{nll > tau} slots equally (m = 1 unless values tie exactly).  n_top = 0: NaN.
 * The workspace of the forward (floats, mia_topk_ce_workspace) is handed to the backward unchanged.  flags: LABEL_U8, IGNORE. */
int mia_topk_ce_workspace(int64_t n_pixels); /* floats; 0 = too many pixels */
int mia_topk_ce_fwd(const float* logits, const void* labels, const float* class_w, int nb, int64_t hw, int k1, int64_t sn,
                    int64_t sk, int64_t sp, int flags, int64_t ignore_label, int64_t n_top, float* workspace, float* out,
                    int* bad_label, void* stream);
int mia_topk_ce_bwd(const float* logits, const void* labels, const float* class_w, const float* workspace, const float* grad_out,
                    float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk,
                    int64_t gsp, int flags, int64_t ignore_label, void* stream);
/* Region-based loss (compound_losses.py:178-233, DC_and_BCE_loss: sigmoid soft Dice + BCEWithLogitsLoss): one sigmoid output per
 * region, regions may overlap, multi-label target with an optional ignore channel.  Per valid pixel and channel, p = sigmoid(z):
 *   I += p t, P += p, G += t;  bce += pos_weight[c] t softplus(-z) + (1 - t) softplus(z)
 *   dc = -mean (2I + smooth) / max(G + P + smooth, 1e-8)  (channel 0 dropped without MIA_REGLOSS_DO_BG; I, P, G summed over the batch
 *   first with MIA_REGLOSS_BATCH, else the mean runs over (image, channel))
 *   CE = bce / (nb c hw) without MIA_REGLOSS_IGNORE; with it bce / max(#valid pixels, 1e-8): the sum runs over the valid pixels and
 *   ALL c channels, the divisor counts PIXELS (the reference's mask broadcasts over the channels)
 * out[0] = ce_w*CE + dice_w*dc, out[1] = CE, out[2] = dc; counts [B][C][3] = int64 (tp, fp, fn) of (z > 0) against (t > 0.5) over
 * the valid pixels; coef: nb*c*2 + 1 floats for the backward (workspace: mia_region_loss_workspace floats, 8-byte aligned).
 * Logits [B][C][HW] fp32 addressed by (sn, sk, sp) element strides like mia_seg_loss_fwd, 1 <= c <= 8 (c == 1 needs DO_BG).
 * Target, dense form: contiguous planar [B][c (+1)][HW] of fp32 or, with MIA_REGLOSS_TARGET_U8, 1-byte elements (bool and uint8),
 * values used as they are; with MIA_REGLOSS_IGNORE the extra last channel is the ignore channel, valid = (last == 0); region_bits
 * and n_labels are not read.  Index form (MIA_REGLOSS_INDEX): a label map [B][HW] of int64 or (TARGET_U8) uint8 plus the device
 * table region_bits[n_labels], bit c of entry l set when label l belongs to region c; with MIA_REGLOSS_IGNORE pixels labelled
 * ignore_label are invalid; a label outside [0, n_labels) that is not the ignore label: NaN results and the sticky verdict in
 * bad_label[1], exactly as mia_seg_loss_fwd.  pos_weight: c floats or NULL.
 * Backward, one pass: dlogits (own strides gsn, gsk, gsp) = grad_out * valid * [ce_w (p (1 + (pw - 1) t) - pw t) / N +
 * dice_w p (1 - p) (a t + b)] with N the divisor of CE and (a, b) from coef, both 0 where the Dice denominator was clipped; invalid
 * pixels get exact zeros.  The index form and the dense form of the same target give bit-identical out, counts and gradients, as do
 * the 16-byte and the scalar access paths: a thread owns the same four pixels and every sum runs in the same order in all of them.
 * Results are bit-identical run to run (no float atomics); no host sync. */
#define MIA_REGLOSS_DO_BG 1
#define MIA_REGLOSS_BATCH 2
#define MIA_REGLOSS_IGNORE 4
#define MIA_REGLOSS_INDEX 8
#define MIA_REGLOSS_TARGET_U8 16
int mia_region_loss_workspace(int nb, int c, int slabs); /* floats; the buffer must be 8-byte aligned */
int mia_region_loss_fwd(const float* logits, const void* target, const unsigned* region_bits, int n_labels, const float* pos_weight,
                        int nb, int64_t hw, int c, int64_t sn, int64_t sk, int64_t sp, int flags, int64_t ignore_label, float smooth,
                        float dice_w, float ce_w, int slabs, float* workspace, float* coef, float* out, int64_t* counts,
                        int* bad_label, void* stream);
int mia_region_loss_bwd(const float* logits, const void* target, const unsigned* region_bits, int n_labels, const float* pos_weight,
                        const float* coef, const float* grad_out, float* dlogits, int nb, int64_t hw, int c, int64_t sn, int64_t sk,
                        int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp, int flags, int64_t ignore_label, void* stream);

/* ------------------------------------------------------------------ optimizer (al_trainer.py:1374-1379) */
#define MIA_OPT_ADAM 0
#define MIA_OPT_ADAMW 1
#define MIA_OPT_SGD 2
int mia_grad_norm_workspace(void); /* floats */
/* out[0] = L2 norm of grad_scale*grad, out[1] = min(1, max_norm/(norm+1e-6)) (torch.nn.utils.clip_grad_norm_);
 * grad_scale = 1/world_size when `grad` holds the all-reduced SUM of per-rank gradients */
int mia_grad_norm(const float* grad, int64_t n, float max_norm, float grad_scale, float* workspace, float* out, void* stream);
int mia_scale_by_clip(float* x, int64_t n, const float* clip, void* stream);
int mia_optim_step(float* param, const float* grad, float* m, float* v, int64_t n, int kind, float lr, float beta1,
                   float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, int first_step,
                   const float* clip, float grad_scale, void* stream);
/* mia_optim_step with the per-step scalars read from device memory: dyn = {lr, bias_corr1, bias_corr2, first_step != 0} (fp32[4]),
 * rewritten by the host before every replay of a captured step (PolyLRScheduler, al_trainer.py:1366-1379) */
/* writes dyn (32 bytes, 16-byte aligned: fp32 {lr, bias_corr1, bias_corr2, first_step}, u64 {Philox seed, base offset}) from kernel
 * ARGUMENTS -- safe however far the host runs ahead of the device; the u64 half is what mia_dropout_mask_dyn reads */
int mia_step_dyn_set(void* dyn32, float lr, float bias_corr1, float bias_corr2, int first_step, uint64_t seed, uint64_t offset, void* stream);
int mia_optim_step_dyn(float* param, const float* grad, float* m, float* v, int64_t n, int kind, float beta1, float beta2, float eps,
                       float weight_decay, const float* dyn, const float* clip, float grad_scale, void* stream);

/* ------------------------------------------------------------------ augmentation / resize / normalisation (src/transforms) */
/* images [B][C][H][W] fp32, labels [B][H][W] int64, per-sample parameter arrays on the device;
 * apply[b] == 0 (apply may be NULL = all) copies sample b through unchanged. */
/* RandomAffine / RandomRotation (joint_transform.py:158-206, :100-127): torchvision F.affine / F.rotate tensor path
 * = inverse matrix mats[b][6] -> base grid -> grid_sample(nearest, zeros, align_corners=False); image and label in one launch. */
int mia_affine_nearest(const float* img_in, float* img_out, const long long* lab_in, long long* lab_out, int nb, int c, int h,
                       int w, const float* mats, const int* apply, void* stream);
/* Elastic deformation (north_star; NO reference counterpart -- SURVEY 0 row 2 -- own spec, see csrc/augment.hip): displacement
 * vectors disp[B][2][gh][gw] (pixels; component 0 = x, 1 = y) on a coarse control grid spanning the image corner to corner,
 * bilinearly interpolated per pixel; image sampled bilinearly with zero padding, label at the nearest source pixel. */
int mia_elastic_warp(const float* img_in, float* img_out, const long long* lab_in, long long* lab_out, int nb, int c, int h,
                     int w, const float* disp, int gh, int gw, const int* apply, void* stream);
/* RandomRotation90 / MirrorTransform (joint_transform.py:40-97): torch.rot90(k) then optional flips; 4- or 8-byte elements */
int mia_rot90_flip(const void* in, void* out, int elem_bytes, int nb, int c, int h, int w, int k, int flip_h, int flip_w,
                   void* stream);
/* RandomCrop2D (joint_transform.py:130-155): F.crop with per-sample window origins top[b], left[b] (device int arrays);
 * the window lies inside the image (T.RandomCrop.get_params draws it so); 4- or 8-byte elements */
int mia_crop(const void* in, void* out, int elem_bytes, int nb, int c, int h, int w, int oh, int ow, const int* top,
             const int* left, void* stream);
/* RandomGaussianBlur (image_transform.py:145-193): F.gaussian_blur = k x k outer-product kernel, reflect pad */
int mia_gaussian_blur(const float* in, float* out, int nb, int c, int h, int w, const float* sigma, const int* ksize,
                      int max_ksize, const int* apply, void* stream);
/* per-sample (mean, unbiased std) over C*H*W (gray=1, C=3: of the luma image): feeds contrast and z-score */
int mia_sample_stats_workspace(int nb); /* floats */
int mia_sample_stats(const float* in, int nb, int c, int64_t hw, int gray, float* workspace, float* mean_std, void* stream);
/* Selected-sample forms for the batched pipeline (al_trainer.py:670-697: every stage is drawn per sample with p = 0.1 .. 0.2).
 * In every augmentation entry point `apply[b]` > 0 transforms sample b, 0 copies it through, < 0 SKIPS it (not read, not
 * written).  mia_sample_stats_sel: statistics of the samples with apply[b] >= 0 only.  mia_copy_selected: out[b] = in[b] for
 * apply[b] > 0 (bytes_per_sample % 16 == 0) -- the copy-back of a neighbourhood stage run into a scratch buffer. */
int mia_sample_stats_sel(const float* in, int nb, int c, int64_t hw, int gray, float* workspace, float* mean_std,
                         const int* apply, void* stream);
int mia_copy_selected(const void* in, void* out, int64_t bytes_per_sample, int nb, const int* apply, void* stream);
#define MIA_EW_GAMMA 0    /* RandomGamma            image_transform.py:31 */
#define MIA_EW_CONTRAST 1 /* RandomContrast / RandomBrightness (both ColorJitter(contrast=)) image_transform.py:62,:93 */
#define MIA_EW_NOISE 2    /* RandomGaussianNoise with an explicit noise tensor image_transform.py:130-132 */
#define MIA_EW_ZSCORE 3   /* ZScoreNormalize        normalization.py:17-21 */
int mia_elementwise(const float* in, float* out, int64_t per_sample, int nb, int op, const float* p0, const float* mean_std,
                    const float* aux, const int* apply, void* stream);
/* RandomGaussianNoise with on-device Philox4x32-10 normal noise (sigma[b]) */
int mia_noise_clip(const float* in, float* out, int64_t per_sample, int nb, const float* sigma, uint64_t seed, uint64_t offset,
                   const int* apply, void* stream);
/* JointResize image path / UnetProcessor.preprocess / deep-supervision Upsample: interpolate(bilinear, align_corners=False);
 * lowres_hw[b][2] != NULL = SimulateLowRes (image_transform.py:218-225: nearest-exact down, bilinear up) fused in one pass */
int mia_resize_bilinear(const float* in, float* out, int nb, int c, int h, int w, int oh, int ow, const int* lowres_hw,
                        const int* apply, void* stream);
int mia_resize_bilinear_bwd(const float* dout, float* din_zeroed, int nb, int c, int h, int w, int oh, int ow, void* stream);
/* torchvision >= 0.17 default antialias=True on the tensor path: separable triangle filter (two passes, tmp = [B][C][H][OW]) */
int mia_resize_bilinear_aa(const float* in, float* tmp, float* out, int nb, int c, int h, int w, int oh, int ow, void* stream);
/* JointResize label path / UnetProcessor.postprocess: interpolate(nearest) */
int mia_resize_nearest(const void* in, void* out, int elem_bytes, int64_t planes, int h, int w, int oh, int ow, void* stream);

/* ------------------------------------------------------------------ validation / selection reductions */
/* pred = output.softmax(1).argmax(1) (al_trainer.py:1430-1431) + per-(image, class) hard Dice of calculate_metric_percase
 * (:1539-1556, medpy.metric.dc: 2|A&B|/(|A|+|B|), 0 for an empty prediction).  pred / (labels, workspace, counts[B][K1][3],
 * dice[B][K1]) are each optional.  logits == NULL = label-map mode: `pred` is an INPUT label map (the post-processed
 * prediction of valid_slices, al_trainer.py:1442-1446) and only the counts / Dice against `labels` are computed. */
int mia_argmax_dice_workspace(int nb, int k1, int slabs); /* floats */
int mia_argmax_dice(const float* logits, const long long* labels, long long* pred, int nb, int64_t hw, int k1, int64_t sn, int64_t sk,
                    int64_t sp, int slabs, float* workspace, float* counts, float* dice, void* stream);
/* scores[B][3] = (entropy, least-confidence, margin) acquisition scores of the active-learning selectors
 * (entropy_selector.py:42-49, confidence_selector.py:42-47, margin_selector.py:42-48); smooth = the entropy selector's
 * log2(p + smooth) guard (1e-8 in al_train) */
int mia_selector_scores_workspace(int nb, int slabs); /* floats */
int mia_selector_scores(const float* logits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, float smooth, int slabs,
                        float* workspace, float* scores, void* stream);
/* BADGE gradient embeddings of a batch (badge_selector.py:19-35 `image_wise_grad` and :80-96, the loss it differentiates, which
 * the reference evaluates one image at a time through autograd): embed[nb][k1 * c0] = d(CE(logits, a) + DiceLoss(logits, a)) /
 * d(weight of the 1x1 head) per image, a = the image's own arg-max labels (ties to the lowest class), entry c * c0 + k like
 * decoder.seg_output.weight flattened; loss[nb] = that loss per image.  logits fp32 addressed by (sn, sk, sp) element strides like
 * mia_selector_scores; feat = the head's input, NHWC [nb][hw][c0], dtype MIA_F32 (16-byte aligned) or MIA_BF16 (8-byte aligned);
 * smooth / do_bg / squared = DiceLoss's (softmax=True; `batch` makes no difference at one image per loss).  1 <= k1 <= 8
 * (k1 >= 2 unless do_bg), c0 a multiple of 4 up to 128, hw < 2^31.  No atomics, fixed summation order: bit-identical run to run,
 * and an image's result does not depend on nb or on its position.  The workspace query also returns the number of pixel slabs per
 * image (a function of hw alone; slabs may be NULL); it returns 0 for an unsupported shape. */
int mia_badge_embed_workspace(int nb, int64_t hw, int k1, int c0, int dtype, int* slabs); /* floats */
int mia_badge_embed(const float* logits, const void* feat, int dtype, int nb, int64_t hw, int k1, int c0, int64_t sn, int64_t sk,
                    int64_t sp, float smooth, int do_bg, int squared, float* workspace, float* embed, float* loss, void* stream);
/* HD (ITK HausdorffDistanceImageFilter) and ASD (medpy asd, connectivity 1) of calculate_metric_percase
 * (al_trainer.py:1539-1556) for k1 mask pairs per volume: mask 0 = (pred > 0, labels > 0), mask c = (pred == c, labels == c).
 * ndim 2: d == 1, 4-neighbour borders, sd unused; ndim 3: 6-neighbour borders.  hd / asd [nvol][k1];
 * NaN where the prediction mask is empty, +inf where only the label mask is.  pred / labels int64 [nvol][d][h][w]; spacing
 * (sd, sh, sw) in array axis order, finite, > 0, with s^2 a normal fp32.  Limits: d <= 1024, h, w <= 4096, nvol * k1 <= 209715.
 * Workspace: 3 floats + 1 byte per voxel + <= 2^20 floats of partials, whatever k1 (masks run one at a time). */
int mia_surface_distance_workspace(int nvol, int d, int h, int w, int k1); /* floats; < 0 if it does not fit an int */
int mia_surface_distance(const long long* pred, const long long* labels, int nvol, int ndim, int d, int h, int w, int k1,
                         float sd, float sh, float sw, float* workspace, float* hd, float* asd, void* stream);
/* The same hd / asd (bit for bit) plus the symmetric surface metrics of the same mask pairs, over the multisets
 * S1 = {d(a, dB) : a in dA} and S2 = {d(b, dA) : b in dB} (dX = the border of mia_surface_distance), n = |dA| + |dB|:
 *   hd_pct = numpy's linear percentile of S1 u S2 (medpy hd95 at percentile 95): pos = (double)(n - 1) * (percentile / 100.0),
 *            k = floor(pos), v[k] + (v[min(k + 1, n - 1)] - v[k]) * (pos - k) over the ascending order v; 0 < percentile <= 100
 *   assd   = (mean S1 + mean S2) / 2 (medpy assd; mean S1 is asd)
 *   nsd    = (|{s in S1 : s <= tolerance[m]}| + |{s in S2 : s <= tolerance[m]}|) / n, the voxel-count surface Dice; tolerance: k1
 *            HOST floats, finite and >= 0, in the units of the spacing; the kernels compare fp32 squared distances with tolerance^2
 * hd_pct = assd = NaN where the prediction mask is empty, +inf where only the label mask is; nsd = 0 in both cases.  All outputs
 * [nvol][k1] fp32.  The order statistic is exact (a radix select over the fp32 squared distances, integer atomics only): results are
 * bit-identical from run to run and a volume's do not depend on the rest of the batch.  Arguments and limits as for
 * mia_surface_distance, and nvol <= 4096; every check happens before any launch.
 * Workspace: 4 floats + 1 byte per voxel + partials and select scratch: <= 5 floats per voxel + 2^22 floats, whatever k1. */
int mia_surface_metrics_workspace(int nvol, int d, int h, int w, int k1); /* floats; < 0 outside the limits */
int mia_surface_metrics(const long long* pred, const long long* labels, int nvol, int ndim, int d, int h, int w, int k1,
                        float sd, float sh, float sw, double percentile, const float* tolerance, float* workspace, float* hd,
                        float* asd, float* hd_pct, float* assd, float* nsd, void* stream);
/* Signed distance maps of Kervadec et al.'s boundary loss (`one_hot2dist`; csrc/boundary.hip) for index labels [nb][h][w], int64
 * or (label_u8 != 0) uint8, and the classes selected by bit k of class_mask (0 <= k < k1 <= 8, at least one):
 *   phi[b][ci] = edt(~G) * ~G - (edt(G) - 1) * G,  G = (labels[b] == k), ci = the rank of k among the selected classes,
 * edt the exact Euclidean distance transform with spacing (sh, sw) in array axis order (finite, > 0, s^2 a normal fp32); the `- 1`
 * is literal whatever the spacing.  Pixels outside the array do not exist (an object that touches the image edge has no boundary
 * there, scipy's rule -- the opposite of mia_surface_distance's border test).  A class that is absent from an image, or fills it,
 * gets phi = 0 there, decided on the device.  A label outside [0, k1) is a member of no class.  phi: fp32 [nb][nc][h][w], nc = the
 * number of selected classes; workspace: mia_sdm_workspace floats (one per phi element).  Limits: h, w <= 4096, nb * nc <= 65535,
 * nb * nc * h * w < 2^31; every check happens before any launch.  No atomics: bit-identical from run to run, and an image's map does
 * not depend on the rest of the batch. */
int mia_sdm_workspace(int nb, int h, int w, int k1, int class_mask); /* floats; < 0 outside the limits */
int mia_signed_distance_map(const void* labels, int label_u8, int nb, int h, int w, int k1, int class_mask, float sh, float sw,
                            float* workspace, float* phi, void* stream);
/* Boundary loss on those maps: L = (1/N) sum over images, selected classes and pixels of softmax(logits)_k * phi_k with
 * N = nb * nc * hw.  Logits fp32 addressed by (sn, sk, sp) element strides like mia_seg_loss_fwd; phi [nb][nc][hw] as written by
 * mia_signed_distance_map (or any fp32 map of that shape); labels are read for the range check only.  weight_dev: a DEVICE pointer
 * to one fp32 multiplier read by the kernels at run time, or NULL for 1 -- a captured step can change it between replays.
 * out[0] = weight * L, out[1] = L, out[2] = weight; coef: one float for the backward.  A label outside [0, k1) raises
 * bad_label[0] / bad_label[1] exactly as mia_seg_loss_fwd: out and every gradient become NaN.  The backward writes
 *   dlogits_j = grad_out * weight * s_j * (w_j - sum_k w_k s_k),  w_k = phi_k / N for a selected class, else 0
 * to (gsn, gsk, gsp) strides; grad_out: device pointer to one float or NULL for 1.  Sums in double in a fixed order, no atomics:
 * bit-identical from run to run.  slabs = blocks per image of the forward; workspace: mia_boundary_loss_workspace floats. */
int mia_boundary_loss_workspace(int nb, int slabs); /* floats; < 0 for a bad shape */
int mia_boundary_loss_fwd(const float* logits, const void* labels, int label_u8, const float* phi, const float* weight_dev, int nb,
                          int64_t hw, int k1, int class_mask, int64_t sn, int64_t sk, int64_t sp, int slabs, float* workspace,
                          float* coef, float* out, int* bad_label, void* stream);
int mia_boundary_loss_bwd(const float* logits, const float* phi, const float* coef, const float* weight_dev, const float* grad_out,
                          float* dlogits, int nb, int64_t hw, int k1, int class_mask, int64_t sn, int64_t sk, int64_t sp,
                          int64_t gsn, int64_t gsk, int64_t gsp, void* stream);
/* Mean-teacher consistency (csrc/consistency.hip; Tarvainen & Valpola 2017, UA-MT of Yu et al. 2019; the reference has no such
 * code): softmax-MSE between student logits zs and teacher logits zt, both fp32, each addressed by its own (sn, sk, sp) /
 * (tsn, tsk, tsp) element strides like mia_seg_loss_fwd (the layouts may differ; a batch slice of a larger tensor works), 1 <= k1 <= 8.
 * With ps = softmax(zs), pt = softmax(zt), e_k = ps_k - pt_k, d = sum_k e_k^2 per pixel:
 *   prob_mean == NULL (plain):  L = sum d / (nb * k1 * hw)  -- torch.mean((ps - pt)**2)
 *   prob_mean != NULL (masked): prob_mean planar fp32 [nb][k1][hw] (what mia_softmax_accum leaves after T passes of weight 1/T),
 *     u = -sum_k prob_mean_k * log(prob_mean_k + 1e-6), keep = (u < threshold), n_keep = sum keep,
 *     L = sum keep * d / (den_scale * n_keep + 1e-16);  n_keep == 0 gives L = 0 and a zero gradient, not NaN
 * dyn_dev: DEVICE array {weight, threshold} of two fp32 values read by the kernels at run time (a captured step follows later
 * writes), or NULL for weight 1 -- the plain form only: prob_mean needs dyn_dev.  out[0] = weight * L, out[1] = L, out[2] = weight;
 * n_keep[0] = the kept pixels as an exact integer (nb * hw in the plain form); keep: byte map [nb][hw] (1 = kept) that the backward
 * reads, so both directions agree on every pixel and the backward does not read prob_mean (may be NULL in the plain form); coef[0] =
 * 1 / denominator.  The backward writes
 *   dzs_j = grad_out * weight * coef * keep * 2 * ps_j * (e_j - sum_k ps_k e_k)
 * to (gsn, gsk, gsp) strides (grad_out: device pointer to one float or NULL for 1; keep NULL = every pixel); zt and prob_mean get no
 * gradient.  Block partials, then one finalize block in double / int64, in a fixed order, no atomics: bit-identical from run to run,
 * and an image's keep map does not depend on the rest of the batch.  Four pixels per thread with 16-byte accesses for planar
 * (sp == 1) and channels-last (sk == 1, sp == k1) tensors when hw % 4 == 0 and pointers / strides are 16-byte aligned (the rule of
 * mia_softmax_accum; the gradient must then have the student's layout class), one pixel per thread otherwise.  slabs = blocks per
 * image of the forward; workspace: mia_consistency_workspace 4-byte words.  Limits: nb * hw < 2^31.  Every check happens before any
 * launch. */
int mia_consistency_workspace(int nb, int slabs); /* 4-byte words; < 0 for a bad shape */
int mia_consistency_fwd(const float* zs, const float* zt, const float* prob_mean, const float* dyn_dev, int nb, int64_t hw, int k1,
                        int64_t sn, int64_t sk, int64_t sp, int64_t tsn, int64_t tsk, int64_t tsp, float den_scale, int slabs,
                        float* workspace, unsigned char* keep, float* coef, float* out, long long* n_keep, void* stream);
int mia_consistency_bwd(const float* zs, const float* zt, const unsigned char* keep, const float* coef, const float* dyn_dev,
                        const float* grad_out, float* dzs, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                        int64_t tsn, int64_t tsk, int64_t tsp, int64_t gsn, int64_t gsk, int64_t gsp, void* stream);
/* teacher[i] = alpha * teacher[i] + (1 - alpha) * student[i] over n fp32 values (the mean teacher's exponential moving average over
 * FlatOptimizer.flat_param), evaluated in double and rounded once.  alpha_dev: DEVICE pointer to one float read at run time, or
 * NULL to use the host value `alpha` (then 0 <= alpha <= 1).  alpha == 0 copies the student bit for bit.  16-byte accesses where
 * both buffers are 16-byte aligned at the same element, one element at a time for the head, the tail and differently aligned
 * buffers; both must be 4-byte aligned and must not overlap. */
int mia_ema_update(float* teacher, const float* student, int64_t n, float alpha, const float* alpha_dev, void* stream);
/* Uncertainty rectified pyramid consistency (csrc/urpc.hip; URPC: Luo et al., MICCAI 2021 / MedIA 2022; the reference has no such
 * code) between the ns outputs one network makes at several decoder scales, on unlabelled images.  z, factors, strides (and dz,
 * gstrides) are HOST arrays of ns entries, read during the call: z[s] = DEVICE pointer to fp32 logits [nb][k1][(H / f_s) * (W / f_s)]
 * addressed by strides[3 s ..] = (sn, sk, sp) in elements like mia_ds_loss_fwd (planar, channels-last, padded, a batch slice; sk and
 * sp below 2^31); factors[0] = 1 (the full-resolution output), every other factor one of 2, 4, 8, 16 (any order) and a divisor of H
 * and W; 2 <= ns <= 5, 1 <= k1 <= 8, nb * H * W < 2^31.  Per full-resolution pixel, P = nb * H * W:
 *   u_s = up(z_s) (torch interpolate(scale_factor=f_s, mode="bilinear", align_corners=False), in registers; identity for f_s = 1)
 *   p_s = softmax(u_s), lp_s = u_s - logsumexp(u_s), m = (1/ns) sum_s p_s
 *   v_s = sum_k m_k (log m_k - lp_sk)  (a class with m_k == 0 adds 0),  w_s = exp(-v_s),  D_s = sum_k (m_k - p_sk)^2
 *   sums[s] = (sum D_s w_s, sum w_s, sum v_s) over all pixels;  terms[s] = L_s = (sums[s][0] / (P k1)) / (sums[s][1] / P + 1e-8)
 *   + sums[s][2] / P;  L = (1/ns) sum_s L_s;  out[0] = weight * L, out[1] = L, weight = dyn_dev[0] read on the device when the
 *   finalize kernel runs (dyn_dev NULL: 1).
 * The backward recomputes everything from the logits and `sums` (nothing of full-resolution size is kept) and writes, for every
 * scale, dz[s] = grad_out * weight * dL/dz_s through gstrides[3 s ..]: plain autograd of the expression above, the mean m
 * included (grad_out: device pointer to one float or NULL for 1).  The full-resolution scale takes one streaming pass, every other
 * one launch of the gather mia_ds_loss_bwd uses.  No float atomics, every sum in a fixed order: out, sums, terms and every dz are
 * bit-identical run to run; no host sync.  slabs = blocks per image of the forward; workspace: mia_urpc_workspace floats.  Every
 * check happens before any launch. */
int mia_urpc_workspace(int nb, int ns, int slabs); /* floats; < 0 for a bad shape */
int mia_urpc_fwd(const float* const* z, const int* factors, const int64_t* strides, int ns, int nb, int H, int W, int k1,
                 const float* dyn_dev, int slabs, float* workspace, float* sums, float* terms, float* out, void* stream);
int mia_urpc_bwd(const float* const* z, const int* factors, const int64_t* strides, float* const* dz, const int64_t* gstrides, int ns,
                 int nb, int H, int W, int k1, const float* sums, const float* dyn_dev, const float* grad_out, void* stream);
/* Cross pseudo supervision (csrc/cps.hip; CPS: Chen et al., CVPR 2021; the reference has no such code): two networks' logits za and
 * zb, both fp32, each addressed by its own (asn, ask, asp) / (bsn, bsk, bsp) element strides like mia_consistency_fwd (the layouts
 * may differ; a batch slice of a larger tensor works), 1 <= k1 <= 8, N = nb * hw.  Per pixel:
 *   ya = argmax_k za_k, yb = argmax_k zb_k on the fp32 logits themselves, a tie goes to the lowest index (numpy.argmax)
 *   ca = (max_k softmax(za)_k >= tau), cb = (max_k softmax(zb)_k >= tau)   -- the confidence of the label's source
 *   LA = (1/N) sum cb * (logsumexp(za) - za[yb]),  LB = (1/N) sum ca * (logsumexp(zb) - zb[ya])
 * The denominator is always N: tau = 0 is F.cross_entropy(za, yb) + F.cross_entropy(zb, ya), and an empty mask gives 0, not NaN;
 * the term is formed without the probability of the label, so a label whose soft-max is 0 in fp32 still has a finite term.
 * dyn_dev: DEVICE array {weight, tau} of two fp32 values read by the kernels at run time (a captured step follows later writes), or
 * NULL for weight 1, tau 0.  out[0] = weight * (LA + LB), out[1] = LA, out[2] = LB, out[3] = weight; counts = {sum ca, sum cb,
 * sum (ya == yb)} as exact integers; code: byte map [nb][hw] = ya | yb << 3 | ca << 6 | cb << 7 that the backward reads instead of
 * recomputing arg-max and threshold, so both directions agree on every pixel.  The backward writes, in ONE launch,
 *   dza_j = grad_out * weight / N * cb * (softmax(za)_j - [j == yb])   to (gasn, gask, gasp) strides
 *   dzb_j = grad_out * weight / N * ca * (softmax(zb)_j - [j == ya])   to (gbsn, gbsk, gbsp) strides
 * (grad_out: device pointer to one float or NULL for 1); a pixel whose flag is clear gets exactly 0; labels and flags carry no
 * gradient.  Block partials, then one finalize block in double / int64, in a fixed order, no atomics: bit-identical from run to run,
 * and an image's code does not depend on the rest of the batch.  Four pixels per thread with 16-byte accesses for planar (sp == 1)
 * and channels-last (sk == 1, sp == k1) tensors when hw % 4 == 0 and pointers / strides are 16-byte aligned (the rule of
 * mia_consistency_fwd; each gradient must then have the layout class of its logits), one pixel per thread otherwise.  slabs =
 * blocks per image of the forward; workspace: mia_cps_workspace 4-byte words.  Limits: nb * hw < 2^31.  Every check happens before
 * any launch; nothing synchronises with the host. */
int mia_cps_workspace(int nb, int slabs); /* 4-byte words; < 0 for a bad shape */
int mia_cps_fwd(const float* za, const float* zb, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t asn, int64_t ask,
                int64_t asp, int64_t bsn, int64_t bsk, int64_t bsp, int slabs, float* workspace, unsigned char* code, float* out,
                long long* counts, void* stream);
int mia_cps_bwd(const float* za, const float* zb, const unsigned char* code, const float* dyn_dev, const float* grad_out, float* dza,
                float* dzb, int nb, int64_t hw, int k1, int64_t asn, int64_t ask, int64_t asp, int64_t bsn, int64_t bsk, int64_t bsp,
                int64_t gasn, int64_t gask, int64_t gasp, int64_t gbsn, int64_t gbsk, int64_t gbsp, void* stream);
/* Bidirectional copy-paste (csrc/bcp.hip; BCP: Bai et al., CVPR 2023; the reference has no such code; definition:
 * losses/copy_paste.py).
 * Mix: out[n][c][p] = mask[n][p] != 0 ? fg[n][c][p] : bg[n][c][p] over contiguous fp32 [nb][c][hw] batches; mask: bytes, image n at
 * mask + n * mask_sn with mask_sn == hw (one mask per image) or 0 (one mask for the batch); out: image n at out + n * out_sn, out_sn
 * >= c * hw (a batch slice of a larger contiguous tensor).  A selection, not a blend: the bits of the chosen operand pass through
 * (NaN payloads, -0.0).  16-byte accesses when hw % 4 == 0, fg / bg / out are 16-byte and mask 4-byte aligned and out_sn % 4 == 0; one
 * element per thread otherwise; both give the same bits. */
int mia_bcp_mix(const float* fg, const float* bg, const unsigned char* mask, float* out, int nb, int c, int64_t hw, int64_t mask_sn,
                int64_t out_sn, void* stream);
/* Two-source loss of a mixed image: logits fp32 by (sn, sk, sp) like mia_cps_fwd, 1 <= k1 <= 8; label_a, label_b: contiguous [nb][hw]
 * index maps, both int64 or (labels_u8) both uint8; mask as for the mix.  Region A (mask != 0) reads label_a, region B label_b; a pixel
 * reads ONLY its own region's label.  Per region r, over all images and pixels of the call, with p = softmax(z):
 *   I_rk = sum p_k [y_r = k], Z_rk = sum p_k^2, Y_rk = sum [y_r = k], N_r = pixels of r (Y, N exact integers)
 *   D_r = (1/k1) sum_k (1 - (2 I_rk + smooth) / (Z_rk + Y_rk + smooth)),  C_r = sum (logsumexp(z) - z[y_r]) / (N_r + 1e-16)
 *   an empty region: D_r = C_r = 0.   L = weight_a (D_A + C_A) / 2 + weight_b (D_B + C_B) / 2
 * out[5] = {L, D_A, C_A, D_B, C_B}; counts[2] = {N_A, N_B}; coef[2 (2 k1 + 1)]: what the backward reads.  A selected label outside
 * [0, k1) follows mia_seg_loss_fwd: NaN out / coef and the sticky verdict in bad_label[1] (bad_label: the int32[2] of the other
 * losses).  The backward recomputes the soft-max and writes dlogits = grad_out * dL/dz by (gsn, gsk, gsp) (grad_out: device pointer
 * to one float or NULL for 1).  A thread owns the same four consecutive pixels on the 16-byte path (planar / channels-last logits, hw
 * % 4 == 0, 16-byte aligned logits and int64 labels, 4-byte aligned uint8 labels and mask; dlogits in the layout class of the logits)
 * and on the scalar path, and every sum runs in one fixed order: the two paths give the same bits, and every result is bit-identical
 * from run to run (no float atomics).  slabs = blocks per image of the forward; workspace: mia_bcp_loss_workspace 4-byte words.
 * Limits: nb * hw < 2^31.  Every check happens before any launch; nothing synchronises with the host. */
int mia_bcp_loss_workspace(int nb, int k1, int slabs); /* 4-byte words; < 0 for a bad shape */
int mia_bcp_loss_fwd(const float* logits, const void* label_a, const void* label_b, const unsigned char* mask, int nb, int64_t hw,
                     int k1, int64_t sn, int64_t sk, int64_t sp, int64_t mask_sn, int labels_u8, float smooth, float weight_a,
                     float weight_b, int slabs, float* workspace, float* coef, float* out, long long* counts, int* bad_label,
                     void* stream);
int mia_bcp_loss_bwd(const float* logits, const void* label_a, const void* label_b, const unsigned char* mask, const float* coef,
                     const float* grad_out, float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                     int64_t gsn, int64_t gsk, int64_t gsp, int64_t mask_sn, int labels_u8, void* stream);
/* Weak-to-strong consistency (csrc/w2s.hip; FixMatch: Sohn et al., NeurIPS 2020; UniMatch: Yang et al., CVPR 2023; CutMix-CPS; the
 * reference has no such code; definition: losses/weak_strong.py). */
#define MIA_W2S_MAX_CLASSES 8
/* Pseudo-labels of the weak view: logits fp32 [nb][k1][hw] by (sn, sk, sp) like mia_cps_fwd, 1 <= k1 <= 8.  Per pixel
 *   y = argmax_k z_k (on the fp32 logits, a tie to the LOWEST index),  keep = (max_k softmax(z)_k >= tau),  code = y | keep << 7
 * tau = dyn_dev[1] read on the device (dyn_dev: DEVICE {weight, tau}; NULL = tau 0, every pixel kept; a NaN keeps nothing).  code:
 * contiguous bytes [nb][hw]; kept[0] = sum keep as an exact int64.  An image's code does not depend on the rest of the batch.  Four
 * pixels per thread under the rule of mia_cps_fwd (code 4-byte aligned), one otherwise.  slabs = blocks per image; workspace: nb * slabs
 * 4-byte words. */
int mia_w2s_labels(const float* logits, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int slabs,
                   int* workspace, unsigned char* code, long long* kept, void* stream);
/* CutMix of a batch with itself: out[n][c][p] = mask[n][p] != 0 ? x[src][c][p] : x[n][c][p] over contiguous fp32 x [nb][c][hw];
 * perm: DEVICE int32[nb], src = (unsigned)perm[n] < nb ? perm[n] : n -- an entry outside the batch is never used as an index: the
 * image is mixed with itself and the sticky verdict bad_perm[1] is set (bad_perm: DEVICE int32[2] laid out like bad_label; nothing
 * on the device clears [1]).  mask, mask_sn, out, out_sn as mia_bcp_mix; out must not overlap x (checked from the address ranges).
 * A selection: the bits of the chosen operand pass through.  16-byte accesses when hw % 4 == 0, x / out are 16-byte and mask 4-byte
 * aligned and out_sn % 4 == 0; one element per thread otherwise; both give the same bits. */
int mia_cutmix_perm(const float* x, const int* perm, const unsigned char* mask, float* out, int nb, int c, int64_t hw, int64_t mask_sn,
                    int64_t out_sn, int* bad_perm, void* stream);
/* The loss of the strong view: logits fp32 by (sn, sk, sp), 1 <= k1 <= 8; code: the byte map of mia_w2s_labels [nb][hw]; mask / perm as
 * for mia_cutmix_perm, or either NULL for no mix (plain FixMatch).  For pixel (n, p): c = code[mask[n][p] ? src : n][p], y = c & 7,
 * m = c >> 7 (a label >= k1 counts as not kept), q = softmax(z), N = nb * hw, sums over the whole call:
 *   CE = (1/N) sum m (logsumexp(z) - z[y])              the denominator is always N; no kept pixel: 0
 *   I_k = sum m q_k [y = k], Z_k = sum m q_k^2, Y_k = sum m [y = k] (exact integers)
 *   D = (1/k1) sum_k (1 - (2 I_k + smooth) / (Z_k + Y_k + smooth))          no kept pixel: 0
 *   L = weight (ce_weight CE + dice_weight D),  weight = dyn_dev[0] (NULL: 1)
 * out[4] = {L, CE, D, weight}; counts[2] = {sum m over the mixed view, pixels whose mask byte is set (0 without a mix)}; coef[2 k1 +
 * 1]: what the backward reads.  The backward recomputes the soft-max, re-reads code through mask / perm and writes dlogits =
 * grad_out * dL/dz by (gsn, gsk, gsp) (grad_out: device pointer to one float or NULL for 1); a pixel with m = 0 gets exactly 0.  The
 * perm guard and bad_perm are those of mia_cutmix_perm.  A thread owns the same four consecutive pixels on the 16-byte path (planar /
 * channels-last logits, hw % 4 == 0, 16-byte aligned logits, 4-byte aligned code and mask; dlogits in the layout class of the logits)
 * and on the scalar path, and every sum runs in one fixed order: the two paths give the same bits, and every result is bit-identical
 * from run to run (no float atomics).  slabs = blocks per image of the forward; workspace: mia_w2s_loss_workspace 4-byte words.
 * Limits: nb * hw < 2^31.  Every check happens before any launch; nothing synchronises with the host. */
int mia_w2s_loss_workspace(int nb, int k1, int slabs); /* 4-byte words; < 0 for a bad shape */
int mia_w2s_loss_fwd(const float* logits, const unsigned char* code, const unsigned char* mask, const int* perm, const float* dyn_dev,
                     int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t mask_sn, float smooth, float ce_weight,
                     float dice_weight, int slabs, float* workspace, float* coef, float* out, long long* counts, int* bad_perm,
                     void* stream);
int mia_w2s_loss_bwd(const float* logits, const unsigned char* code, const unsigned char* mask, const int* perm, const float* coef,
                     const float* grad_out, float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                     int64_t gsn, int64_t gsk, int64_t gsp, int64_t mask_sn, void* stream);
/* UniMatch's feature-perturbation stream (csrc/feat_drop.hip; the reference has no such code): the decoder reads an encoder output x
 * [n][hw][c] (contiguous NHWC, dtype MIA_F32 or MIA_BF16) followed along the batch axis by channel-dropped copies of its rows row0 ..
 * row0 + nu - 1.  mask: fp32 [nu][c], any values (Dropout2d: 0 or 1 / (1 - p)), 0 = dropped; out / dy: contiguous [n + nu][hw][c].
 *   forward   out[i] = x[i] (bit copy, i < n);   out[n + u] = m[u][ch] == 0 ? +0.0 : rnd(x[row0 + u] * m[u][ch])        (u < nu)
 *   backward  dx[i] = dy[i] (bit copy) where i is outside [row0, row0 + nu) or m[i - row0][ch] == 0, otherwise
 *             dx[i] = rnd(dy[i] + rnd(dy[n + i - row0] * m[i - row0][ch]))
 * The product is formed in fp32; rnd is the identity for fp32 and round-to-nearest-even for bf16.  A dropped channel is a SELECTION,
 * like mia_bcp_mix / mia_cutmix_perm: a NaN or inf under it does not spread, the forward gives +0.0 (never -0.0), the backward passes
 * dy[i]'s bits through.  In the backward the product and the sum are TWO separately rounded operations, never one fused multiply-add:
 * dx has the bits of the tensor-op form `cat(x, where(m == 0, 0, x[rows].float() * m).to(dtype))` under autograd, which multiplies in
 * one kernel -- and, for bf16, rounds the product to bf16 where the gradient of the cast leaves fp32 -- and adds in another.
 * amax_out: NULL, or (fp32 only; ignored for bf16) a ZEROED 4-byte slot that receives max |out| / max |dx| as an fp32 bit pattern --
 * the amax_out convention of the norm kernels: an integer maximum of the bit patterns of |v|, exact and independent of the order, no
 * float atomics; a NaN counts as mia_amax counts it.  Each pass reads and writes every element once: (2 n + nu) hw c elements of
 * traffic; the work item that reads a row of [row0, row0 + nu) writes (forward) or reads (backward) both of its images.  16-byte
 * accesses (4 fp32 / 8 bf16 channels of one pixel, the mask as aligned float4 loads) when c * element size is a multiple of 16 and
 * x / dy, out / dx and mask are 16-byte aligned; one element per thread otherwise; both give the same bits, and every result is
 * bit-identical from run to run.  Element counts are 64-bit; the grid is capped and a block strides over tiles of whole pixels.
 * Errors (< 0, nothing is launched): nu < 1, row0 < 0, row0 + nu > n, c < 1, hw < 1, a bad dtype, a NULL x / dy, mask or out / dx,
 * out overlapping x (dx overlapping dy).  Nothing synchronises with the host. */
int mia_feat_drop_cat_fwd(int dtype, const void* x, const float* mask, void* out, int n, int64_t hw, int c, int row0, int nu,
                          void* amax_out, void* stream);
int mia_feat_drop_cat_bwd(int dtype, const void* dy, const float* mask, void* dx, int n, int64_t hw, int c, int row0, int nu,
                          void* amax_out, void* stream);
/* The launch shape, for tests and byte counts: returns the block cap of the grid (> 0) and sets tile_pixels[0] to the pixels one block
 * handles per stride on the 16-byte (wide != 0) or the one-element path; < 0 for bad arguments. */
int mia_feat_drop_cat_sweep(int dtype, int c, int wide, int* tile_pixels);

/* ------------------------------------------------------------------ dual-task consistency (csrc/dtc.hip) */
/* DTC (Luo et al., AAAI 2021; the reference has no such code; definition: losses/dual_task.py).  z: segmentation logits fp32
 * [nb][k1][hw] by (sn, sk, sp), r: level-set logits fp32 [nb][k1 - 1][hw] by (rsn, rsk, rsp), each addressed like mia_consistency_fwd
 * (planar, channels-last and scalar layout classes, batch slices); 2 <= k1 <= 8; channel c of r belongs to class c + 1.  The first lb
 * images are labelled: phi is the contiguous fp32 [lb][k1 - 1][hw] map of mia_signed_distance_map at unit spacing, extent the
 * [lb][k1 - 1][2] of mia_sdm_extent; both may be NULL when lb = 0.  With s = softmax(z), t = tanh(r), q = sigmoid(-k t) and the
 * normalised target T = phi / m_out (phi > 0), -(1 - phi) / (1 + m_in) (phi < 0), 0 (phi = 0), computed per pixel and never stored:
 *   L_cons = mean over all (n, c, p) of (q_c - s_{c+1})^2,   L_sdf = mean over (n < lb, c, p) of (t - T)^2   (0 when lb = 0)
 *   L = dyn_dev[0] L_cons + dyn_dev[1] L_sdf     (dyn_dev NULL: 1, 1; read on the device when the kernels run)
 * Soft-max, tanh and sigmoid are evaluated in double from the fp32 logits in a form that stays finite for |k t| in the thousands.
 * A thread owns the same four consecutive pixels on the 16-byte path (z and r both planar / channels-last, hw % 4 == 0, 16-byte aligned
 * phi; in the backward each gradient in the layout class of its logits) and on the scalar path, and every sum runs in one fixed order:
 * the two paths give the same bits, and every result is bit-identical from run to run (no float atomics).  Limits: nb * hw < 2^31.
 * Every check happens before any launch; nothing synchronises with the host. */
/* extent [planes][2] = {max phi, max -phi} per plane of hw elements, both >= +0: integer max on the bit patterns of non-negative
 * floats, exact and independent of the order.  planes * hw < 2^31. */
int mia_sdm_extent(const float* phi, int planes, int64_t hw, float* extent, void* stream);
/* The streaming pass: workspace [nb * slabs][2][2] receives the (hi, lo) float pairs of every block's sums of the two terms (slabs =
 * blocks per image; nb * slabs * 4 4-byte words). */
int mia_dtc_fwd(const float* z, const float* r, const float* phi, const float* extent, int nb, int lb, int64_t hw, int k1, float k,
                int64_t sn, int64_t sk, int64_t sp, int64_t rsn, int64_t rsk, int64_t rsp, int slabs, float* workspace, void* stream);
/* One block, in double, in a fixed order: out[3] = {L, L_cons, L_sdf}; coef[2] = {2 dyn[0] / (nb C hw), 2 dyn[1] / (lb C hw) or 0},
 * each rounded once to fp32: what the backward reads. */
int mia_dtc_finalize(const float* workspace, const float* dyn_dev, int nb, int lb, int64_t hw, int k1, int slabs, float* coef,
                     float* out, void* stream);
/* One pass: recomputes s, t, q and T; writes dz = grad_out dL/dz by (gsn, gsk, gsp) and dr = grad_out dL/dr by (hsn, hsk, hsp)
 * (grad_out: device pointer to one float or NULL for 1).  dr of an image n >= lb has no L_sdf part. */
int mia_dtc_bwd(const float* z, const float* r, const float* phi, const float* extent, const float* coef, const float* grad_out,
                float* dz, float* dr, int nb, int lb, int64_t hw, int k1, float k, int64_t sn, int64_t sk, int64_t sp, int64_t rsn,
                int64_t rsk, int64_t rsp, int64_t gsn, int64_t gsk, int64_t gsp, int64_t hsn, int64_t hsk, int64_t hsp, void* stream);

/* ------------------------------------------------------------------ virtual adversarial training (csrc/vat.hip) */
/* KL distance between two fp32 logits tensors [nb][k1][hw], each addressed by its own (sn, sk, sp) / (tsn, tsk, tsp) element strides
 * like mia_consistency_fwd (planar, channels-last and scalar layout classes, batch slices):
 *   p = softmax(zt) (the target: no gradient), log q = z - logsumexp(z), log p likewise
 *   L = coef * sum_pix sum_k p_k (log p_k - log q_k),  coef = 1 / den;  a term with p_k == 0 contributes 0
 * den is the caller's: nb * hw for the per-pixel mean, nb for "batchmean".  dyn_dev = {weight, ...} (device, read when the kernels
 * run; NULL = weight 1).  out = {weight * L, L, weight}; coef[0] = 1 / den for the backward.  Both soft-maxes and every partial sum
 * are in double; one finalize block adds the block partials in a fixed order; no float atomics.
 * Backward: dz_j = grad_out * weight * coef * (q_j - p_j), written by (gsn, gsk, gsp); grad_out: device fp32 (NULL = 1).
 * slabs = blocks per image of the forward; workspace: mia_kl_workspace 4-byte words.  Limits: 1 <= k1 <= 8, nb * hw < 2^31.  Every
 * check happens before any launch. */
int mia_kl_workspace(int nb, int slabs); /* 4-byte words; < 0 for a bad shape */
int mia_kl_fwd(const float* z, const float* zt, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
               int64_t tsn, int64_t tsk, int64_t tsp, double den, int slabs, float* workspace, float* coef, float* out, void* stream);
int mia_kl_bwd(const float* z, const float* zt, const float* coef, const float* dyn_dev, const float* grad_out, float* dz, int nb,
               int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t tsn, int64_t tsk, int64_t tsp, int64_t gsn, int64_t gsk,
               int64_t gsp, void* stream);
/* u[nb * per] ~ U[-0.5, 0.5) (24 bits, every value exact) from Philox4x32-10, the generator of mia_dropout_mask: element i is word
 * i & 3 of counter (i >> 2, offset) under key `seed`, so it depends on (seed, offset, i) only -- a sample's values do not depend on nb. */
int mia_vat_noise(float* u, int nb, int64_t per, uint64_t seed, uint64_t offset, void* stream);
/* out[n] = sum of x[n][0 .. per)^2 in double, rounded once.  workspace: mia_sample_sumsq_workspace 4-byte words. */
int mia_sample_sumsq_workspace(int nb, int64_t per); /* 4-byte words; < 0 for a bad shape */
int mia_sample_sumsq(const float* x, int nb, int64_t per, float* workspace, float* out, void* stream);
/* out = x + s * (gscale * g) / (gscale * sqrt(sumsq[n]) + 1e-8) over [nb][per] fp32 buffers, in double, rounded once; s = *scale_dev
 * (device) when given, else `scale`.  With gscale = xi this is the published `_l2_normalize(d.grad)` times s when g is the gradient
 * with respect to x + xi d rather than d.  g == 0 gives out = x.  16-byte accesses when x, g and out are 16-byte aligned. */
int mia_vat_perturb(const float* x, const float* g, const float* sumsq, float gscale, float scale, const float* scale_dev, float* out,
                    int nb, int64_t per, void* stream);

/* ------------------------------------------------------------------ prediction (entry/fugc2025/predict.py) */
/* Ensemble reduction of predict.py:144-161 (`P = P + seg.softmax(1)` per fold model) and the arg-max of :55-57, one pass per
 * model: prob_sum[nb][k1][hw] (planar fp32) = (first ? 0 : prob_sum) + weight * softmax_k(logits); pred != NULL also receives the
 * arg-max over classes of the updated sum as int64 [nb][hw], ties to the lowest class (torch.argmax).  prob_sum may be NULL only
 * with `first` set and pred given (one model: the plain arg-max).  Logits are addressed by (sn, sk, sp) element strides like
 * mia_argmax_dice; 1 <= k1 <= 8.  One thread owns a pixel, models accumulate in call order, no atomics: bit-identical run to run.
 * Four pixels per thread with 16-byte accesses for planar (sp == 1) and channels-last (sk == 1, sp == k1) logits when hw % 4 == 0
 * and the pointers / strides are 16-byte aligned; one pixel per thread otherwise. */
int mia_softmax_accum(const float* logits, float* prob_sum, long long* pred, int nb, int64_t hw, int k1, int64_t sn, int64_t sk,
                      int64_t sp, float weight, int first, void* stream);
/* The same reduction for region-based models (one sigmoid output per region, regions may overlap): prob_sum[nb][c][hw] = (first ? 0 :
 * prob_sum) + weight * sigmoid(logits); pred != NULL also receives nnU-Net's region-to-label rule on the updated sum as int64
 * [nb][hw]: pred = 0; for i in 0 .. c-1: if prob_sum[i] > threshold: pred = class_order[i] -- later regions overwrite earlier ones.
 * class_order: device array of c int64 values (read only with pred).  Everything else as mia_softmax_accum: prob_sum may be NULL
 * only with `first` set and pred given, one thread owns a pixel, models accumulate in call order, the same alignment rule decides
 * between four pixels per thread and one; 1 <= c <= 8. */
int mia_sigmoid_accum(const float* logits, float* prob_sum, long long* pred, const long long* class_order, int nb, int64_t hw, int c,
                      int64_t sn, int64_t sk, int64_t sp, float weight, float threshold, int first, void* stream);
/* Sliding-window prediction: one pass per (model, mirror combination, window).  For 0 <= i < ph, 0 <= j < pw
 *   canvas[n][k][y0+i][x0+j] += weight * gy[i] * gx[j] * softmax_k(logits[n][:, i', j']),  i' = flip_h ? ph-1-i : i, j' = flip_w ? pw-1-j : j
 * logits [nb][k1][ph][pw] fp32 addressed by (sn, sk, sp) element strides like mia_softmax_accum (pixel index i' * pw + j'), canvas
 * contiguous [nb][k1][h][w] fp32, gy[ph] / gx[pw] fp32 device arrays (the importance map is their outer product), 1 <= k1 <= 8.
 * The window must lie inside the canvas (MIA_EARG otherwise; nothing is clipped); canvas pixels outside it are not touched.  One
 * thread owns a canvas pixel, no atomics; a pixel's bits do not depend on the branch that computed it (four pixels per thread with
 * 16-byte accesses when pw, x0 and w are multiples of 4 and pointers / strides are 16-byte aligned, one pixel otherwise). */
int mia_window_accum(const float* logits, float* canvas, const float* gy, const float* gx, int nb, int k1, int ph, int pw, int h,
                     int w, int y0, int x0, int64_t sn, int64_t sk, int64_t sp, float weight, int flip_h, int flip_w, void* stream);
/* One pass over the canvas: pred (int64 [nb][h][w], may be NULL) = arg-max over k of the raw canvas, ties to the lowest class, taken
 * before any scaling; with normalise != 0, canvas[n][k][y][x] *= (scale * ry[y]) * rx[x] in place (ry[h], rx[w] fp32 device arrays:
 * the reciprocal of the separable coverage, sum over window starts of gy[y - y0] resp. gx[x - x0]). */
int mia_window_finalize(float* canvas, long long* pred, const float* ry, const float* rx, int nb, int k1, int h, int w, float scale,
                        int normalise, void* stream);
/* UnetProcessor.denoise_masks = denoise_one_mask (predict.py:55-90, models/unet/unet_processor.py:72-160) for nb int64 label maps
 * [nb][h][w] in one launch.  Each of the binary masks `in > 0` and `in == 1` is zero-padded by max(dilate, erode), dilated, eroded,
 * eroded and dilated with (2r+1)^2 rectangles clipped to the padded domain, cropped, blurred with the smooth_k-tap 8.8 fixed-point
 * Gaussian (BORDER_REFLECT_101) and thresholded at 1/2; out = 2, 1 where the cleaned class-1 mask is set, 0 where the cleaned object
 * mask is empty.  Bit-exact integer arithmetic.  in != out.  Supported: 0 <= dilate, erode <= 8, smooth_k in {1, 3, 5, 7},
 * smooth_k / 2 < h, w <= 2^20; mia_mask_denoise returns MIA_EUNSUPPORTED where mia_mask_denoise_supported returns 0. */
int mia_mask_denoise_supported(int h, int w, int dilate, int erode, int smooth_k);
int mia_mask_denoise(const long long* in, long long* out, int nb, int h, int w, int dilate, int erode, int smooth_k, void* stream);
/* Connected components of int64 label maps [nvol][d][h][w] (csrc/components.hip): what `UnetProcessor.remove_cc`
 * (models/unet/unet_processor.py:121-125, inside denoise_one_mask :72-113) only approximates with a morphological opening.  ndim 2:
 * every [h][w] slice is an image of its own; ndim 3: every [d][h][w] volume.  Two voxels are joined when they are neighbours
 * (connectivity 1: 4 / 6 face neighbours; connectivity == ndim: all 8 / 26) and hold the same label in [1, n_classes) -- with
 * `foreground`, when both hold any label in that range (the reference's object mask).  A label outside [0, n_classes) belongs to no
 * component.  roots (int32, the labels' shape) = 1 + the smallest linear index, within its image, of the voxel's component, 0
 * elsewhere: a function of the input alone, bit-identical from run to run.  Limits: voxels per image < 2^31 - 1, 1 <= n_classes <=
 * 256.  status: one device int32, zeroed by the call; non-zero afterwards means a union-find walk hit its iteration cap (1) or met
 * a parent above its child (2) -- impossible unless the kernels are wrong, and then the results are not to be used. */
int mia_cc_label(const long long* labels, int* roots, int nvol, int ndim, int d, int h, int w, int connectivity, int n_classes,
                 int foreground, int* status, void* stream);
/* The clean-up on those components (nnU-Net's "remove all but the largest component", which unet_processor.py:121-125 stands in
 * for): out (int64, != labels) = fill on every voxel of a component whose exact size is < min_size, or -- with keep_largest -- which
 * is not the winner of its (image, class), of its image with `foreground`: the largest size, ties to the lowest root (np.argmax over
 * scipy's raster-ordered numbering).  Everything else is copied through, so kept voxels keep their class.  class_mask: HOST array of
 * n_classes bytes read during the call, non-zero = filter that class (NULL = every class; ignored with `foreground`).  workspace:
 * mia_cc_workspace floats, 8-byte aligned; status as for mia_cc_label. */
int mia_cc_workspace(int nvol, int ndim, int d, int h, int w, int n_classes); /* floats; < 0 if it does not fit an int */
int mia_cc_filter(const long long* labels, long long* out, int nvol, int ndim, int d, int h, int w, int connectivity, int n_classes,
                  int foreground, int keep_largest, int min_size, const unsigned char* class_mask, int64_t fill, float* workspace,
                  int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
