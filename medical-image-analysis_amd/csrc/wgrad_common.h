// Shared pieces of the weight-gradient kernels: arguments, geometry, the swizzled LDS image and its transposing reads, the block
// decode, and one host launcher per kernel family (kernels are launched from their own translation unit: -fno-gpu-rdc).
//   wgrad_tile.hip  register-staged tiles: wgrad_bf16_kernel, wgrad_bf16_fast_kernel, wgrad_f32_kernel, wgrad_f32_fast_kernel
//   wgrad_ring.hip  256- / 768-thread stride-1 kernels: wgrad_bf16_2wg_kernel, wgrad_bf16_dma_kernel, wgrad_bf16_dma96_kernel
//   wgrad_bt.hip    512-thread 128 n x 64 k blocks: wgrad_bf16_bt_kernel, wgrad_bf16_bt_s2_kernel, wgrad_bf16_bt_t2_kernel
//   conv_wgrad.hip  slab reduce, planner, dispatcher and the C entry points
#pragma once
#include "lds_dma.h"
#include "options.h"
#include <type_traits>

enum { MODE_W3S1 = 0, MODE_W3S2 = 1, MODE_W2S2 = 2 };
// kernel families of the dispatcher (conv_wgrad.hip wgrad_select; the values of include/mia_hip.h MIA_WGRAD_FAM_*)
enum { MIA_WGRAD_FAM_DMA96 = 0, MIA_WGRAD_FAM_BT = 1, MIA_WGRAD_FAM_DMA = 2, MIA_WGRAD_FAM_2WG = 3, MIA_WGRAD_FAM_2WG_NL = 4,
       MIA_WGRAD_FAM_TILE_FAST = 5, MIA_WGRAD_FAM_F32_FAST = 6, MIA_WGRAD_FAM_F32_NARROW = 7, MIA_WGRAD_FAM_GENERIC = 8 };

struct WgArgs {
  const void* x1; const void* x2; int c1; int c2;
  const void* dy; int cdy;
  float* slabs;
  int N, Hx, Wx, Hy, Wy;
  int npad, kpad, ksplit;
  int tiles_x, tiles_y;
  int vec_x, vec_dy;
  int opt;  // bit 0: table-driven staging of interior tiles (wgrad_bf16_2wg_kernel); bit 4: XCD-aware block order (wg_block)
  // normalise-on-load (mia_conv_wgrad_nl): x1 is the RAW conv output y of the producing PlainBlock; the kernel stages
  // lrelu(nl_scale[n][k] * y + nl_shift[n][k]) (zero outside the image); nullptr = x1 is an ordinary activation
  const float* nl_scale = nullptr; const float* nl_shift = nullptr; float nl_slope = 0.f;
  // fp32 split mode (common.h SplitF16): max |x| of x1 / x2 / dy as fp32 bit patterns in device memory
  const unsigned* amax_x1 = nullptr; const unsigned* amax_x2 = nullptr; const unsigned* amax_dy = nullptr;
};

template <int MODE> struct WGeo {
  static constexpr int KS = MODE == MODE_W2S2 ? 2 : 3;
  static constexpr int S = MODE == MODE_W3S1 ? 1 : 2;
  static constexpr int PAD = MODE == MODE_W2S2 ? 0 : 1;
  static constexpr int TAPS = KS * KS;
};

// ---------------------------------------------------------------- bf16 (tr16 reads)
__device__ __forceinline__ int swz_off(int row, int ch) {
  // byte offset of 16-byte chunk `ch` (0..7) of pixel-row `row` in a [rows][64 x bf16] tile, stored as
  // 8-row x 32-column subtiles of 512 B with the chunk index XOR-swizzled by (row>>2)&3
  return 512 * ((row >> 3) * 2 + (ch >> 2)) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ s16x4 tr_read(const unsigned char* base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off));
}

// transposing read at an absolute LDS byte address (the workgroup's LDS base folded into the lane-constant part once, instead of
// a v_add per read)
typedef __attribute__((address_space(3))) unsigned char lds_u8;
__device__ __forceinline__ s16x4 tr_read_at(unsigned addr) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_u8*)(size_t)addr);
}

// ---------------------------------------------------------------- which block of dW a workgroup owns (bf16 fast kernels)
// Input-channel blocks are cut per SOURCE (ceil(c1 / KW) + ceil(c2 / KW) of them), so a block never straddles the two tensors of a
// concatenated input whatever c1 is; a source's last block may be partial (lanes beyond cs read zeros and do not store).
struct WgBlock {
  int cs, kloc;      // channels of the block's source tensor; the block's first channel within it
  int n0, k0;        // first output channel; first input channel in dW's columns
  const void* xsrc;  // the source tensor (x1 or x2)
};
// The column blocks of one split index.  NW = a block's width in output channels: 64, 128, or 96 (with 96-wide input-channel blocks too).
// A kernel fills it once, then:   int bx = blockIdx.x, by = blockIdx.y;
//                                 if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
//                                 const WgBlock blk = cols.block(a, bx);
template <int NW> struct WgCols {
  static constexpr int KW = NW == 96 ? 96 : 64;
  int kb1, nkb;  // input-channel blocks of the first source, of both
  __device__ __forceinline__ explicit WgCols(const WgArgs& a) : kb1((a.c1 + KW - 1) / KW), nkb(kb1 + (a.c2 + KW - 1) / KW) {}
  // XCD-aware order (1-D grid of columns x 8 x ceil(ksplit / 8) workgroups): the column blocks of one split index share their tiles
  // -> one XCD, one L2.  blockIdx.x -> (column block bx, split index by); by >= a.ksplit: grid padding, nothing to do.
  __device__ __forceinline__ void xcd_order(const WgArgs& a, int& bx, int& by) const {
    const int ncol = nkb * (NW == 96 ? (a.cdy + NW - 1) / NW : a.npad / NW), slot = bx >> 3;
    by = (slot / ncol) * 8 + (bx & 7);
    bx = slot % ncol;
  }
  __device__ __forceinline__ WgBlock block(const WgArgs& a, int bx) const {
    const int kblk = bx % nkb, nblk = bx / nkb;
    const bool second = kblk >= kb1;
    WgBlock b;
    b.cs = second ? a.c2 : a.c1; b.kloc = (second ? kblk - kb1 : kblk) * KW;
    b.n0 = nblk * NW; b.k0 = (second ? a.c1 : 0) + b.kloc;
    b.xsrc = second ? a.x2 : a.x1;
    return b;
  }
};

// ---------------------------------------------------------------- host launchers, one per family file
// runtime mode -> template argument: f(std::integral_constant<int, MODE>{})
template <typename F> static inline void wgrad_with_mode(int mode, F&& f) {
  if (mode == MODE_W3S1) f(std::integral_constant<int, MODE_W3S1>{});
  else if (mode == MODE_W3S2) f(std::integral_constant<int, MODE_W3S2>{});
  else f(std::integral_constant<int, MODE_W2S2>{});
}

// wgrad_tile.hip.  fast = the branch-free raw-buffer kernels (conv_wgrad_run checks their contract); narrow / split: fp32 fast only
void wgrad_tile_launch(int mode, int dtype, bool fast, bool narrow, bool split, const WgArgs& a, dim3 grid, hipStream_t st);
// wgrad_ring.hip (stride-1 3x3 bf16)
enum { WG_RING_2WG = 0, WG_RING_2WG_NL = 1, WG_RING_DMA = 2, WG_RING_DMA96 = 3 };
void wgrad_ring_launch(int which, const WgArgs& a, dim3 grid, hipStream_t st);
// wgrad_bt.hip (bf16, cdy % 128 == 0): one kernel per mode
void wgrad_bt_launch(int mode, const WgArgs& a, dim3 grid, hipStream_t st);
#ifdef CONV64_STAMPS
// diagnostic build only: resident workgroups per CU of a family's persistent kernels, -1 = no such kernel (mia_wgrad_debug_occupancy)
int wgrad_ring_debug_occupancy(int which);
int wgrad_bt_debug_occupancy(int mode);
#endif
