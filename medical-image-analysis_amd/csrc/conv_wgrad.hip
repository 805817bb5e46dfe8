// Weight-gradient kernels on MFMA for gfx950 (NHWC activations).
//
//   dW[tap][n][k] = sum over output pixels p of  dy[p][n] * x[p*stride + tap - pad][k]
//
// (reference: autograd of nn.Conv2d at src/models/unet/blocks.py:83-90 and of
// nn.ConvTranspose2d at unet.py:142).  The contraction index is the PIXEL, which is the slow
// dimension of both NHWC operands, so:
//   * bf16: tiles are staged to LDS in their natural [pixel][channel] order (XOR-swizzled 8-row x
//     32-column subtiles) and both MFMA operands are fetched with ds_read_b64_tr_b16 (hardware
//     transposing read) -> v_mfma_f32_16x16x32_bf16, K = 32 pixels per instruction.
//   * fp32: v_mfma_f32_16x16x4_f32 takes one scalar per lane; [pixel][channel] LDS rows padded to
//     80 dwords make the b32 fragment reads conflict free.
// A workgroup (4 waves) owns a 64(n) x 64(k) block of dW for ALL taps; wave w owns k-tile w and keeps
// taps x 4 accumulators in registers while it walks its share of the pixel tiles (split-K over
// gridDim.y).  Partials go to per-split slabs; mia_wgrad_reduce sums the slabs in a fixed order
// (bitwise reproducible, no float atomics) straight into the parameter's native OIHW / IOHW layout.
//   MODE_W3S1: 3x3 stride 1 pad 1;  MODE_W3S2: 3x3 stride 2 pad 1;  MODE_W2S2: 2x2 stride 2 pad 0
//   (MODE_W2S2 is ConvTranspose2d's wgrad with x := grad_output (fine grid), dy := input (coarse)).
// This file: the slab reduce, the planner, the dispatcher and the C entry points.  The kernels live in wgrad_tile.hip (register-staged
// tiles, every mode and dtype), wgrad_ring.hip (stride-1 bf16: two-workgroup kernel, 64- and 96-wide LDS-DMA rings) and wgrad_bt.hip
// (bf16, 512-thread 128 n x 64 k blocks); wgrad_common.h holds what they share.
#include "wgrad_common.h"
#include <stdlib.h>

// ---------------------------------------------------------------- slab reduce -> native parameter layout
// layout 0: conv   grad[n][k][kh][kw]  (OIHW, n = Cout, k = Cin)
// layout 1: convT  grad[n][k][kh][kw] where the parameter is [Cin_T][Cout_T][2][2] and the GEMM ran with
//           n := Cin_T (coarse-side channels, "dy" operand) and k := Cout_T (fine-side channels, "x" operand)
// Small gradients (few (n, k) pairs, many split-K slabs): 32 elements x 8 slab lanes per block -- every thread sums an
// eighth of the slabs for one element (elements ordered k-fastest so the slab reads coalesce), LDS combines the lanes in
// a fixed order.
__global__ __launch_bounds__(256) void wgrad_reduce_small_kernel(const float* __restrict__ slabs, int ksplit, int taps, int npad,
                                                                 int kpad, float* __restrict__ grad, int nn, int kk, int accumulate) {
  __shared__ float sh[8][33];
  const int e = threadIdx.x & 31, zl = threadIdx.x >> 5;
  const int total = nn * kk * taps;
  const int i = blockIdx.x * 32 + e;  // (t, n, k), k fastest
  const size_t sstride = (size_t)taps * npad * kpad;
  float s = 0.f;
  int t = 0, n = 0, k = 0;
  if (i < total) {
    k = i % kk; n = (i / kk) % nn; t = i / (kk * nn);
    const float* src = slabs + ((size_t)t * npad + n) * kpad + k;
    // eight slab loads in flight per thread, added in the same order as a plain loop (latency-bound: 24 us at 512 slabs before)
    int z = zl;
    for (; z + 56 < ksplit; z += 64) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(z + 8 * j) * sstride];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; z < ksplit; z += 8) s += src[(size_t)z * sstride];
  }
  sh[zl][e] = s;
  __syncthreads();
  if (zl == 0 && i < total) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) r += sh[j][e];
    float* dst = grad + ((size_t)n * kk + k) * taps + t;
    *dst = accumulate ? *dst + r : r;
  }
}

// The same with four consecutive k per thread (16-byte slab loads; kk % 4 == 0): the 64-channel level's 75 MB of slabs took 52 us with
// 4-byte loads.  Per element the slabs are added in the same order as in wgrad_reduce_small_kernel.
__global__ __launch_bounds__(256) void wgrad_reduce_small4_kernel(const float* __restrict__ slabs, int ksplit, int taps, int npad,
                                                                  int kpad, float* __restrict__ grad, int nn, int kk, int accumulate) {
  __shared__ f32x4 sh[8][33];
  const int e = threadIdx.x & 31, zl = threadIdx.x >> 5;
  const int kq = kk >> 2, total = nn * kq * taps;
  const int i = blockIdx.x * 32 + e;  // (t, n, k / 4), k fastest
  const size_t sstride = (size_t)taps * npad * kpad;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  int t = 0, n = 0, k4 = 0;
  if (i < total) {
    k4 = i % kq; n = (i / kq) % nn; t = i / (kq * nn);
    const float* src = slabs + ((size_t)t * npad + n) * kpad + 4 * k4;
    int z = zl;
    for (; z + 24 < ksplit; z += 32) {
      f32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(z + 8 * j) * sstride);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += v[j];
    }
    for (; z < ksplit; z += 8) s += *reinterpret_cast<const f32x4*>(src + (size_t)z * sstride);
  }
  sh[zl][e] = s;
  __syncthreads();
  if (zl == 0 && i < total) {
    f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) r += sh[j][e];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float* dst = grad + ((size_t)n * kk + 4 * k4 + c) * taps + t;
      *dst = accumulate ? *dst + r[c] : r[c];
    }
  }
}

// One thread per (n, k): consecutive lanes walk consecutive k, so every slab read is a coalesced row segment; the taps
// of one (n, k) are adjacent in the parameter layout [n][k][taps], so a wave's stores tile a contiguous span.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, int ksplit, int taps, int npad,
                                                           int kpad, float* __restrict__ grad, int nn, int kk, int accumulate) {
  const int total = nn * kk;
  const size_t plane = (size_t)npad * kpad, sstride = (size_t)taps * plane;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = i / kk, k = i - n * kk;
    const float* src = slabs + (size_t)n * kpad + k;
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = 0.f;
    for (int z = 0; z < ksplit; ++z) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (t < taps) s[t] += src[z * sstride + t * plane];
    }
    float* dst = grad + (size_t)i * taps;
#pragma unroll
    for (int t = 0; t < 9; ++t)
      if (t < taps) dst[t] = accumulate ? dst[t] + s[t] : s[t];
  }
}

// tile heights (rows of 16 output pixels per split-K step)
static int wgrad_tile_h(const MiaOptions& o, int mode, int dtype, bool fast) {
  const int s = mode == MODE_W3S1 ? 1 : 2;
  if (dtype != MIA_BF16) return s == 1 ? 4 : 2;
  // (16-row tiles measured slower -- more VGPRs, partial unroll: 575 vs 621 TFLOP/s at 64ch 512x512 -- whatever the image height)
  if (s == 1 && fast && o.wgrad_dma) return 4;  // wgrad_bf16_dma_kernel
  return s == 1 ? 8 : 4;
}

static bool wgrad_two_wg(int mode, int dtype) { return mode == MODE_W3S1 && dtype == MIA_BF16; }

/* split-K workgroups to aim for: one per CU, or two where the kernel is built for two workgroups per CU */
extern "C" int mia_wgrad_target_blocks(int mode, int dtype) {
  const MiaOptions o = mia_options();
  int per_cu = 1;
  if (wgrad_two_wg(mode, dtype)) per_cu = 2;
  else if (mode == MODE_W3S2 && dtype == MIA_BF16 && o.wgrad_bt && o.wgrad_dma) per_cu = 2;  // 128 n x 64 k blocks: half as many column blocks
  else if (mode == MODE_W2S2 && dtype == MIA_BF16) per_cu = 2;  // 4 taps: 172 registers, 40 KB LDS -> two workgroups fit a CU
  // option reserve_cus: the split count follows the CUs left to the persistent kernels (a different split count is a
  // different -- still fixed -- fp32 summation order of the slabs: deterministic per setting, not bit-identical across settings)
  const int cus = o.reserve_cus > 0 ? ((256 - o.reserve_cus) & ~7) : 256;
  return per_cu * (cus < 8 ? 8 : cus);
}

#ifdef CONV64_STAMPS
/* Diagnostic build only: workgroups of each persistent weight-gradient kernel the runtime keeps resident on one CU. */
extern "C" int mia_wgrad_debug_occupancy(int which) {
  if (which == 0) return wgrad_ring_debug_occupancy(WG_RING_DMA);
  if (which == 1) return wgrad_bt_debug_occupancy(MODE_W3S1);
  if (which == 2) return wgrad_bt_debug_occupancy(MODE_W3S2);
  if (which == 3) return wgrad_ring_debug_occupancy(WG_RING_2WG);
  return -1;
}
#endif

// 96-wide blocks (wgrad_bf16_dma96_kernel): 3x3 stride 1, bf16, every channel count a multiple of 96 and at least one of them not a
// multiple of 64 (cfg5's level 0: 96 -> 96 and (96 | 96) -> 96).
#ifndef MIA_WGRAD_W96
#define MIA_WGRAD_W96 1  /* 0: probe builds that A/B against the 64-wide blocks */
#endif
static bool wgrad_w96(const MiaOptions& o, int mode, int dtype, int c1, int c2, int cdy) {
  if (!MIA_WGRAD_W96 || dtype != MIA_BF16 || mode != MODE_W3S1 || !o.wgrad_dma) return false;
  if (c1 % 96 != 0 || c2 % 96 != 0 || cdy % 96 != 0) return false;
  return c1 % 64 != 0 || cdy % 64 != 0 || (c2 != 0 && c2 % 64 != 0);
}

/* Column blocks of one split-K slice, the workgroup count to aim for and the tile height of the kernel mia_conv_wgrad will pick for THIS
   shape (the caller sizes ksplit from them: ops.conv_wgrad). */
extern "C" int mia_wgrad_plan(int mode, int dtype, int c1, int c2, int cdy, int npad, int hy, int* column_blocks, int* target_blocks,
                              int* tile_h) {
  const MiaOptions o = mia_options();
  const int cus = o.reserve_cus > 0 ? ((256 - o.reserve_cus) & ~7) : 256;
  if (wgrad_w96(o, mode, dtype, c1, c2, cdy)) {
    if (column_blocks) *column_blocks = ceil_div(cdy, 96) * (ceil_div(c1, 96) + ceil_div(c2, 96));
    if (target_blocks) *target_blocks = cus < 8 ? 8 : cus;  // one 768-thread workgroup per CU
    if (tile_h) *tile_h = 4;
    return MIA_OK;
  }
  if (column_blocks) *column_blocks = (npad / 64) * (ceil_div(c1, 64) + ceil_div(c2, 64));
  if (target_blocks) *target_blocks = mia_wgrad_target_blocks(mode, dtype);
  if (tile_h) *tile_h = wgrad_tile_h(o, mode, dtype, true);
  return MIA_OK;
}

extern "C" int mia_wgrad_geometry(int mode, int dtype, int hy, int wy, int* tiles_y, int* tiles_x) {
  const int th = wgrad_tile_h(mia_options(), mode, dtype, true);  // the finest tiling any kernel of this mode uses (bounds ksplit)
  if (tiles_y) *tiles_y = ceil_div(hy, th);
  if (tiles_x) *tiles_x = ceil_div(wy, 16);
  return MIA_OK;
}

// Which kernel family serves a weight gradient: ONE pure function of the options snapshot and the launch description, shared by the
// launch path (conv_wgrad_run switches on its result) and by the query mia_wgrad_family.  chan_ok: every channel count a whole number
// of 16-byte units on aligned tensors; fast: the bf16 branch-free contract (chan_ok and 32-bit byte offsets); fits32: the same
// offset bound for fp32 tensors; nl: normalise-on-load variant (MIA_EUNSUPPORTED outside its kernel's contract).
static int wgrad_select(const MiaOptions& o, int mode, int dtype, int c1, int c2, int cdy, int npad, bool chan_ok, bool fast,
                        bool fits32, bool nl) {
  if (nl) return (fast && mode == MODE_W3S1 && c2 == 0) ? MIA_WGRAD_FAM_2WG_NL : MIA_EUNSUPPORTED;
  const int th = wgrad_tile_h(o, mode, dtype, fast);
  const bool bt = fast && th == 4 && cdy % 128 == 0 && npad % 128 == 0 &&  // 512-thread workgroups on 128 n x 64 k blocks
                  (mode == MODE_W2S2 ? o.wgrad_bt >= 1 && o.wgrad_t2 : o.wgrad_bt);
  if (fast && wgrad_w96(o, mode, dtype, c1, c2, cdy)) return MIA_WGRAD_FAM_DMA96;
  if (bt) return MIA_WGRAD_FAM_BT;
  if (fast && th == 4 && mode == MODE_W3S1) return MIA_WGRAD_FAM_DMA;
  if (fast && wgrad_two_wg(mode, dtype)) return MIA_WGRAD_FAM_2WG;  // stride-2 / transposed shapes stay on the one-workgroup-per-CU kernel
  if (fast) return MIA_WGRAD_FAM_TILE_FAST;
  if (dtype == MIA_F32 && chan_ok && fits32) return (cdy <= 32 && c1 <= 32 && c2 <= 32) ? MIA_WGRAD_FAM_F32_NARROW : MIA_WGRAD_FAM_F32_FAST;
  return MIA_WGRAD_FAM_GENERIC;
}

// The family mia_conv_wgrad / _nl would launch for a shape under the options as they are now: see include/mia_hip.h.
extern "C" int mia_wgrad_family(int mode, int dtype, int c1, int c2, int cdy, int npad, int variant, int split) {
  MIA_CHECK_ARG(mode >= 0 && mode <= MODE_W2S2, "mia_wgrad_family: bad mode %d", mode);
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "mia_wgrad_family: bad dtype");
  MIA_CHECK_ARG(c1 > 0 && c2 >= 0 && cdy > 0 && npad % 64 == 0 && npad >= cdy, "mia_wgrad_family: bad shape");
  MIA_CHECK_ARG(variant == 0 || variant == 1, "mia_wgrad_family: bad variant %d", variant);
  (void)split;  // the split-f16 product form is a template argument of the fp32 families' kernel, not a family of its own
  const int epu = dtype == MIA_BF16 ? 8 : 4;
  const bool chan_ok = c1 % epu == 0 && c2 % epu == 0 && cdy % epu == 0;
  return wgrad_select(mia_options(), mode, dtype, c1, c2, cdy, npad, chan_ok, dtype == MIA_BF16 && chan_ok, true, variant == 1);
}

static int conv_wgrad_run(int mode, int dtype, const void* x1, int c1, const void* x2, int c2, const void* dy,
                          int cdy, float* slabs, int ksplit, int npad, int kpad, int n, int hx, int wx, int hy,
                          int wy, void* stream, const float* nl_scale, const float* nl_shift, float nl_slope,
                          const void* amax_x1 = nullptr, const void* amax_x2 = nullptr, const void* amax_dy = nullptr) {
  MIA_CHECK_ARG(mode >= 0 && mode <= MODE_W2S2, "mia_conv_wgrad: bad mode %d", mode);
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "mia_conv_wgrad: bad dtype");
  MIA_CHECK_ARG(x1 && dy && slabs && c1 > 0 && c2 >= 0 && cdy > 0, "mia_conv_wgrad: null/empty operand");
  MIA_CHECK_ARG((c2 == 0) == (x2 == nullptr), "mia_conv_wgrad: split operand mismatch");
  MIA_CHECK_ARG(npad % 64 == 0 && kpad % 64 == 0 && npad >= cdy && kpad >= c1 + c2, "mia_conv_wgrad: bad padding");
  MIA_CHECK_ARG(ksplit >= 1 && ksplit <= 65535, "mia_conv_wgrad: bad ksplit %d", ksplit);
  bool ok = mode == MODE_W3S1 ? (hx == hy && wx == wy)
          : mode == MODE_W3S2 ? (hy == (hx + 1) / 2 && wy == (wx + 1) / 2) : (hx == 2 * hy && wx == 2 * wy);
  MIA_CHECK_ARG(ok, "mia_conv_wgrad: mode %d shape mismatch x %dx%d dy %dx%d", mode, hx, wx, hy, wy);
  const MiaOptions o = mia_options();  // one snapshot per call
  WgArgs a;
  a.x1 = x1; a.x2 = x2; a.c1 = c1; a.c2 = c2; a.dy = dy; a.cdy = cdy; a.slabs = slabs;
  a.N = n; a.Hx = hx; a.Wx = wx; a.Hy = hy; a.Wy = wy; a.npad = npad; a.kpad = kpad; a.ksplit = ksplit;
  a.nl_scale = nl_scale; a.nl_shift = nl_shift; a.nl_slope = nl_slope;
  a.amax_x1 = static_cast<const unsigned*>(amax_x1); a.amax_x2 = static_cast<const unsigned*>(amax_x2);
  a.amax_dy = static_cast<const unsigned*>(amax_dy);
  // fp32: split f16 products when the caller knows every operand's maximum (otherwise, or with the option off, exact fp32 MFMAs)
  const bool split = dtype == MIA_F32 && o.f32_split && amax_x1 != nullptr && amax_dy != nullptr && (c2 == 0 || amax_x2 != nullptr);
  const int epu = dtype == MIA_BF16 ? 8 : 4;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  a.vec_x = (c1 % epu == 0) && (c2 % epu == 0) && al16(x1) && (x2 == nullptr || al16(x2));
  a.vec_dy = (cdy % epu == 0) && al16(dy);
  a.opt = 1;
  dim3 grid((npad / 64) * (kpad / 64), ksplit);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lim = (size_t)1 << 31;
  // fast paths: channel tails are zero-filled through out-of-range offsets and input-channel blocks are cut per source
  const bool chan_ok = a.vec_x && a.vec_dy;
  dim3 fgrid((npad / 64) * (ceil_div(c1, 64) + ceil_div(c2, 64)), ksplit);
  const bool fast = dtype == MIA_BF16 && chan_ok && (size_t)hx * wx * (c1 > c2 ? c1 : c2) * 2 < lim &&
                    (size_t)hy * wy * cdy * 2 < lim;
  if (fast && o.wgrad_xcd && ksplit % 8 == 0) {  // bf16 fast kernels: 1-D grid in XCD-aware order (a split count below 8 would leave XCDs idle)
    a.opt |= 16;
    fgrid = dim3(fgrid.x * (unsigned)(ceil_div(ksplit, 8) * 8), 1);
  }
  const bool fits32 = (size_t)hx * wx * (c1 > c2 ? c1 : c2) * 4 < lim && (size_t)hy * wy * cdy * 4 < lim;
  const int fam = wgrad_select(o, mode, dtype, c1, c2, cdy, npad, chan_ok, fast, fits32, nl_scale != nullptr);
  const int th = wgrad_tile_h(o, mode, dtype, fast);
  a.tiles_y = ceil_div(hy, th);
  a.tiles_x = ceil_div(wy, 16);
  switch (fam) {
    case MIA_WGRAD_FAM_2WG_NL:  // normalise-on-load: the register-staged two-workgroup kernel is the one that transforms
      a.tiles_y = ceil_div(hy, 8);
      wgrad_ring_launch(WG_RING_2WG_NL, a, fgrid, st);
      break;
    case MIA_WGRAD_FAM_DMA96: {  // 96-wide ring blocks: one block per pixel tile where 64-wide ones need 2 x 2
      const unsigned ncol = (unsigned)(ceil_div(cdy, 96) * (ceil_div(c1, 96) + ceil_div(c2, 96)));
      const dim3 wgrid = (a.opt & 16) ? dim3(ncol * (unsigned)(ceil_div(ksplit, 8) * 8), 1) : dim3(ncol, ksplit);
      a.tiles_y = ceil_div(hy, 4);
      wgrad_ring_launch(WG_RING_DMA96, a, wgrid, st);
      break;
    }
    case MIA_WGRAD_FAM_BT: wgrad_bt_launch(mode, a, dim3(fgrid.x / 2, fgrid.y), st); break;  // half as many column blocks
    case MIA_WGRAD_FAM_DMA: wgrad_ring_launch(WG_RING_DMA, a, fgrid, st); break;
    case MIA_WGRAD_FAM_2WG: wgrad_ring_launch(WG_RING_2WG, a, fgrid, st); break;
    case MIA_WGRAD_FAM_TILE_FAST: wgrad_tile_launch(mode, dtype, true, false, false, a, fgrid, st); break;
    case MIA_WGRAD_FAM_F32_NARROW:  // 32-channel layers: half-width blocks, all four waves busy
      if (mode == MODE_W3S1) a.tiles_y = ceil_div(hy, 8);  // (8-row tiles: wgrad_f32_fast_kernel N8)
      wgrad_tile_launch(mode, dtype, true, true, split, a, fgrid, st);
      break;
    case MIA_WGRAD_FAM_F32_FAST: wgrad_tile_launch(mode, dtype, true, false, split, a, fgrid, st); break;
    case MIA_WGRAD_FAM_GENERIC: wgrad_tile_launch(mode, dtype, false, false, false, a, grid, st); break;
    default:
      mia_set_error("mia_conv_wgrad_nl: shape outside the normalise-on-load kernel's contract (ask mia_wgrad_nl_supported first)");
      return fam;
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_conv_wgrad(int mode, int dtype, const void* x1, int c1, const void* x2, int c2, const void* dy,
                              int cdy, float* slabs, int ksplit, int npad, int kpad, int n, int hx, int wx, int hy,
                              int wy, const void* amax_x1, const void* amax_x2, const void* amax_dy, void* stream) {
  return conv_wgrad_run(mode, dtype, x1, c1, x2, c2, dy, cdy, slabs, ksplit, npad, kpad, n, hx, wx, hy, wy, stream, nullptr, nullptr, 0.f,
                        amax_x1, amax_x2, amax_dy);
}

// Weight gradient with normalise-on-load of x (the backward half of the fused PlainBlock): see include/mia_hip.h.
extern "C" int mia_wgrad_nl_supported(int mode, int dtype, int c1, int cdy) {
  if (mode != MODE_W3S1) return 0;
  return (dtype == MIA_BF16 && c1 % 8 == 0 && cdy % 8 == 0) ? 1 : 0;
}

extern "C" int mia_conv_wgrad_nl(int mode, int dtype, const void* y_in, int c1, const float* in_scale, const float* in_shift,
                                 float slope, const void* dy, int cdy, float* slabs, int ksplit, int npad, int kpad, int n,
                                 int hx, int wx, int hy, int wy, void* stream) {
  MIA_CHECK_ARG(in_scale != nullptr && in_shift != nullptr, "mia_conv_wgrad_nl: null coefficient arrays");
  MIA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "mia_conv_wgrad_nl: slope %g outside [0, 1]", (double)slope);
  MIA_CHECK_ARG(mia_wgrad_nl_supported(mode, dtype, c1, cdy), "mia_conv_wgrad_nl: unsupported shape (mode %d dtype %d %d x %d)", mode,
                dtype, c1, cdy);
  return conv_wgrad_run(mode, dtype, y_in, c1, nullptr, 0, dy, cdy, slabs, ksplit, npad, kpad, n, hx, wx, hy, wy, stream, in_scale,
                        in_shift, slope);
}

extern "C" int mia_wgrad_reduce(const float* slabs, int ksplit, int taps, int npad, int kpad, float* grad, int nn,
                                int kk, int accumulate, void* stream) {
  MIA_CHECK_ARG(slabs && grad && ksplit >= 1 && taps >= 1 && nn >= 1 && kk >= 1 && nn <= npad && kk <= kpad,
                "mia_wgrad_reduce: bad arguments");
  MIA_CHECK_ARG(taps <= 9 && (int64_t)nn * kk < ((int64_t)1 << 31), "mia_wgrad_reduce: taps > 9 or gradient too large");
  const int64_t total = (int64_t)nn * kk;
  // many slabs: split them over 8 lanes per element (the per-(n,k) kernel below walks all `ksplit` slabs serially, which is
  // latency bound -- 57 us for 75 MB at 512 slabs); few slabs: one thread per (n,k), all taps
  if ((total < 32768 || ksplit >= 8) && total * taps < ((int64_t)1 << 31)) {
    if (kk % 4 == 0 && kpad % 4 == 0 && (reinterpret_cast<uintptr_t>(slabs) & 15) == 0) {
      const int blocks = (int)((total / 4 * taps + 31) / 32);
      hipLaunchKernelGGL(wgrad_reduce_small4_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), slabs, ksplit,
                         taps, npad, kpad, grad, nn, kk, accumulate);
    } else {
      const int blocks = (int)((total * taps + 31) / 32);
      hipLaunchKernelGGL(wgrad_reduce_small_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), slabs, ksplit,
                         taps, npad, kpad, grad, nn, kk, accumulate);
    }
  } else {
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), slabs, ksplit,
                       taps, npad, kpad, grad, nn, kk, accumulate);
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
