// Weight gradients, bf16, 512-thread workgroups on 128 n x 64 k blocks with an LDS-DMA ring: stride-1 3x3, stride-2 3x3 and the
// transposed 2x2.  See conv_wgrad.hip for the GEMM and wgrad_common.h for the shared pieces.
#include "wgrad_common.h"

// ---------------------------------------------------------------- bf16, 512-thread big block (stride-1 3x3, cdy % 128 == 0)
// Round 3.  wgrad_bf16_dma_kernel moves 92 bytes L2 -> LDS per MFMA (an 18 KB x tile + an 8 KB dy tile per 288 MFMAs) and runs two
// 256-thread workgroups per CU.  Here ONE 512-thread workgroup per CU owns a 128 n x 64 k x 9 taps block: waves 0-3 take output
// channels n0 .. n0 + 63, waves 4-7 the next 64, both halves share the x tile (59 bytes per MFMA), wave (nh, kq) keeps the same
// 9 x 4 accumulator tiles as before.  Same swizzled LDS images, transposing reads and three-stage LDS-DMA ring; what changes with
// one workgroup per CU is that nothing hides a wave's non-matrix work any more, so (lesson of conv_bt.hip) the DMA pieces of tile
// t + 2 are issued BETWEEN the MFMA steps of tile t instead of in a block in front of them, and everything a piece needs is a lane
// constant or a scalar prepared once per tile.
__global__ __launch_bounds__(512, 2) void wgrad_bf16_bt_kernel(const WgArgs a) {
  constexpr int KS = 3, TAPS = 9, TH = 4;
  constexpr int XH = TH + 2, XROW = 3072;  // 24 pixels x 128 B per image row of the x tile
  constexpr int X_BYTES = XH * XROW, DH_BYTES = TH * 16 * 128, D_BYTES = 2 * DH_BYTES, STAGE = X_BYTES + D_BYTES, NSTAGE = 3;
  constexpr int XPIECES = XH * 3, DPIECES = TH * 2, PIECES = XPIECES + 2 * DPIECES;  // 18 + 8 + 8: piece pc lives at byte 1024 pc
  constexpr int MAXOWN = (PIECES + 7) / 8;                                            // 5 (waves 0, 1) or 4 pieces per wave and tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nh = wave >> 2, kq = wave & 3;  // 64-channel half of dy and 16-input-channel tile of this wave
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const WgCols<128> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  // DMA lane constants (as in wgrad_bf16_dma_kernel): lane L of a piece is 16-byte chunk (L&3) of half (L>>5) of pixel row
  // r = (L>>2)&7 of the 8-row block; the source chunk is un-swizzled by the block's parity
  const int dr = (lane >> 2) & 7;
  const int ch8_0 = 4 * (lane >> 5) + ((lane & 3) ^ ((dr >> 2) & 3)), ch8_1 = 4 * (lane >> 5) + ((lane & 3) ^ ((2 + (dr >> 2)) & 3));
  const unsigned xlane0 = (unsigned)((dr * cs + kloc + ch8_0 * 8) * 2), xlane1 = (unsigned)((dr * cs + kloc + ch8_1 * 8) * 2);
  const unsigned dlane0 = (unsigned)((dr * a.cdy + n0 + ch8_0 * 8) * 2), dlane1 = (unsigned)((dr * a.cdy + n0 + ch8_1 * 8) * 2);
  const bool xok0 = kloc + ch8_0 * 8 < cs, xok1 = kloc + ch8_1 * 8 < cs;
  const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

  // per-piece lane offsets of a tile whose 18 columns lie inside the image (descriptor based at the tile origin); padding /
  // channel-tail lanes already point out of range.  dy piece q = (half h = q >> 3, 8-pixel block q & 7) reads channels n0 + 64 h ..
  unsigned voffc[MAXOWN];
#pragma unroll
  for (int j = 0; j < MAXOWN; ++j) {
    const int pc = wave + 8 * j;
    if (pc < XPIECES) {
      const int iy = pc / 3, xb = pc - 3 * iy, ix = 8 * xb + dr;
      const bool ok = (ix < 18) & ((xb & 1) ? xok1 : xok0);
      voffc[j] = ok ? (unsigned)((iy * a.Wx + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0) : SENT;
    } else {
      const int q = pc - XPIECES, h = q >> 3, qq = q & 7;
      const bool ok = pc < PIECES;
      voffc[j] = ok ? (unsigned)(((qq >> 1) * a.Wy + 8 * (qq & 1)) * a.cdy * 2) + ((qq & 1) ? dlane1 : dlane0) + (unsigned)(h * 128) : SENT;
    }
  }

  // ---- issue state of the tile being fetched (prepared once per tile, pieces issued between the MFMA steps)
  i32x4 rx, rd;
  bool fastp = false;
  int i_oy0 = 0, i_ox0 = 0;
  unsigned i_stage = 0;
  auto prepare = [&](int img, int ty, int tx, unsigned stage_base) {
    i_oy0 = ty * TH; i_ox0 = tx * 16; i_stage = stage_base;
    fastp = tx > 0 && tx * 16 + 17 <= a.Wx && tx * 16 + 16 <= a.Wy;  // uniform
    if (fastp) {  // descriptor bases at the tile origin (row iy0 may be -1: its pieces are dropped, nothing is read through it)
      const long long xorg = ((long long)(img * a.Hx + i_oy0 - 1) * a.Wx + i_ox0 - 1) * cs;
      const long long dorg = ((long long)(img * a.Hy + i_oy0) * a.Wy + i_ox0) * a.cdy;
      rx = rsrc_words(xsrc + xorg, (unsigned)(XH * a.Wx * cs * 2));
      rd = rsrc_words(dy + dorg, (unsigned)(TH * a.Wy * a.cdy * 2));
    } else {
      rx = rsrc_words(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
      rd = rsrc_words(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
    }
  };
  auto issue_piece = [&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    const int pc = wave + 8 * j;  // wave-uniform piece index
    if (pc >= PIECES) return;
    const unsigned dst = i_stage + pc * 1024;
    const int iy0 = i_oy0 - 1, ix0 = i_ox0 - 1;
    if (fastp) {
      if (pc < XPIECES) {
        const bool rowok = (unsigned)(iy0 + pc / 3) < (unsigned)a.Hx;
        dma16<0>(rx, rowok ? voffc[j] : SENT, __builtin_amdgcn_readfirstlane(dst));
      } else {
        const bool rowok = i_oy0 + (((pc - XPIECES) & 7) >> 1) < a.Hy;
        dma16<0>(rd, rowok ? voffc[j] : SENT, __builtin_amdgcn_readfirstlane(dst));
      }
    } else if (pc < XPIECES) {
      const int iy = pc / 3, xb = pc - 3 * iy;
      const int gy = iy0 + iy, gx = ix0 + 8 * xb + dr;
      const bool ok = ((unsigned)gy < (unsigned)a.Hx) & ((unsigned)gx < (unsigned)a.Wx) & (8 * xb + dr < 18) & ((xb & 1) ? xok1 : xok0);
      const unsigned off = (unsigned)((gy * a.Wx + ix0 + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0);
      dma16<0>(rx, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    } else {
      const int q = pc - XPIECES, h = q >> 3, qq = q & 7;  // 8-pixel block of the dy tile: output row qq >> 1, pixels 8 (qq & 1) ..
      const int gy = i_oy0 + (qq >> 1), gx = i_ox0 + 8 * (qq & 1) + dr;
      const bool ok = (gy < a.Hy) & (gx < a.Wy);
      const unsigned off = (unsigned)((gy * a.Wy + i_ox0 + 8 * (qq & 1)) * a.cdy * 2) + ((qq & 1) ? dlane1 : dlane0) + (unsigned)(h * 128);
      dma16<0>(rd, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    }
  };
  auto issue_all = [&]() {
    issue_piece(std::integral_constant<int, 0>{}); issue_piece(std::integral_constant<int, 1>{}); issue_piece(std::integral_constant<int, 2>{});
    issue_piece(std::integral_constant<int, 3>{}); issue_piece(std::integral_constant<int, 4>{});
  };
  // this wave's pieces per tile: waves with wave < PIECES % 8 own one more
  auto wait_own_in_flight = [&]() {  // all but the newest tile's own pieces have landed
    if (wave < (PIECES & 7)) wait_vm<MAXOWN>();
    else wait_vm<MAXOWN - 1>();
  };

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant fragment bases (absolute LDS bytes of the CURRENT stage; stepped by one stage per tile)
  const int g1 = grp >> 1, xb0 = 8 * (grp & 1) + qp, sub = 8 * (pp & 1);
  unsigned dbase[2][2], xbase[KS][2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // channel tiles c and c + 2 differ by +512 bytes
    dbase[c][0] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0, 2 * c + (pp >> 1)) + sub;
    dbase[c][1] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0 + 4, 2 * c + (pp >> 1)) + sub;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {
    xbase[kw][0] = lds0 + g1 * XROW + swz_off(xb0 + kw, 2 * kq + (pp >> 1)) + sub;
    xbase[kw][1] = lds0 + g1 * XROW + swz_off(xb0 + kw + 4, 2 * kq + (pp >> 1)) + sub;
  }

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int tile = by;
  int t_tx, t_ty, t_img;  // digits of the NEXT tile to issue
  { int tt = tile; t_tx = tt % a.tiles_x; tt /= a.tiles_x; t_ty = tt % a.tiles_y; t_img = tt / a.tiles_y; }
  int d_tx, d_ty, d_img;
  { int tt = a.ksplit; d_tx = tt % a.tiles_x; tt /= a.tiles_x; d_ty = tt % a.tiles_y; d_img = tt / a.tiles_y; }
  auto advance = [&]() {
    t_tx += d_tx; if (t_tx >= a.tiles_x) { t_tx -= a.tiles_x; t_ty += 1; }
    t_ty += d_ty; if (t_ty >= a.tiles_y) { t_ty -= a.tiles_y; t_img += 1; }
    t_img += d_img;
  };
  int issue_tile = tile;       // index of the next tile to issue
  unsigned issue_stage = 0;    // ring slot it goes to
  // prologue: two tiles in flight
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    if (issue_tile < ntiles) { prepare(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); issue_all(); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;
  }
  if (tile + a.ksplit < ntiles) wait_own_in_flight(); else wait_vm<0>();
  __builtin_amdgcn_s_barrier();

  int stage = 0;
  for (; tile < ntiles; tile += a.ksplit) {
    const bool more = issue_tile < ntiles;  // uniform
    if (more) { prepare(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;

    u32x4 af[2][4], bf[3];
    auto load_a = [&](int kb, int c) -> u32x4 {
      const s16x4 lo = tr_read_at(dbase[c & 1][0] + 512 * (c >> 1) + 4096 * kb);
      const s16x4 hi = tr_read_at(dbase[c & 1][1] + 512 * (c >> 1) + 4096 * kb);
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto load_b = [&](int step) -> u32x4 {  // step = kb * 9 + tap
      const int kb = step / TAPS, t = step % TAPS, kh = t / KS, kw = t % KS;
      const s16x4 lo = tr_read_at(xbase[kw][0] + XROW * (2 * kb + kh));
      const s16x4 hi = tr_read_at(xbase[kw][1] + XROW * (2 * kb + kh));
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) af[0][c] = load_a(0, c);
    bf[0] = load_b(0);
    bf[1] = load_b(1);
#pragma unroll
    for (int step = 0; step < 2 * TAPS; ++step) {
      const int kb = step / TAPS, t = step % TAPS;
      if (step + 2 < 2 * TAPS) bf[(step + 2) % 3] = load_b(step + 2);
      if (kb == 0 && t >= 5 && t <= 8) af[1][t - 5] = load_a(1, t - 5);  // second row block's dy fragments behind the first's MFMAs
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kb][c]), __builtin_bit_cast(bf16x8, bf[step % 3]),
                                                            acc[t][c], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // the pieces of tile t + 2 behind the MFMAs of steps 1, 4, 7, 10, 13
      if (more) {
        if (step == 1) issue_piece(std::integral_constant<int, 0>{});
        if (step == 4) issue_piece(std::integral_constant<int, 1>{});
        if (step == 7) issue_piece(std::integral_constant<int, 2>{});
        if (step == 10) issue_piece(std::integral_constant<int, 3>{});
        if (step == 13) issue_piece(std::integral_constant<int, 4>{});
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // next stage's fragment bases
    const int delta = stage == NSTAGE - 1 ? -(NSTAGE - 1) * STAGE : STAGE;
    stage = stage == NSTAGE - 1 ? 0 : stage + 1;
#pragma unroll
    for (int c = 0; c < 2; ++c) { dbase[c][0] += delta; dbase[c][1] += delta; }
#pragma unroll
    for (int kw = 0; kw < KS; ++kw) { xbase[kw][0] += delta; xbase[kw][1] += delta; }
    if (more) wait_own_in_flight(); else wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 64 * nh + c * 16 + 4 * grp + r, k = k0 + kq * 16 + i16;
        if (kloc + kq * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- bf16, 512-thread big block, 3x3 STRIDE 2 (cdy % 128 == 0)
// The stride-2 weight gradient (first conv of every encoder level, unet.py:57) ran on wgrad_bf16_fast_kernel<MODE_W3S2>: 436
// registers = one wave per SIMD, register staging, two barriers per tile, 0.5 PFLOP/s.  Same block and wave roles as
// wgrad_bf16_bt_kernel (128 n x 64 k x 9 taps, waves = 2 n halves x 4 k tiles); differences:
//   * x tile of 4 output rows x 16 pixels = 9 input rows x 33 pixels, kept as [9 rows][40-pixel pitch][64 ch] (45 pieces of 8
//     pixels x 128 B, swizzled within a row like the stride-1 image): the pitch is a multiple of 8 pixels, so a tap row (kh) and a
//     row block (kb) are IMMEDIATE offsets of the transposing reads (5 KB, 20 KB): six lane-constant bases (kw x the two 4-pixel
//     halves of a fragment) serve all 36 x reads of a tile.
//     A transposing read takes its four K rows from four lane-supplied addresses, so the stride-2 pixel gather costs nothing;
//   * 61 KB per stage -> a ring of TWO stages (122 KB): tile t + 1 is issued during the first MFMA steps of tile t and waited
//     for (vmcnt(0)) at its end.
__global__ __launch_bounds__(512, 2) void wgrad_bf16_bt_s2_kernel(const WgArgs a) {
  constexpr int KS = 3, TAPS = 9, TH = 4;
  constexpr int XH = 2 * TH + 1, XBLK = 5, XROW = XBLK * 1024, XW = 33;  // 9 rows x 5 blocks of 8 pixels (33 used) x 128 B
  constexpr int X_BYTES = XH * XROW, DH_BYTES = TH * 16 * 128, D_BYTES = 2 * DH_BYTES, STAGE = X_BYTES + D_BYTES, NSTAGE = 2;
  constexpr int XPIECES = XH * XBLK, DPIECES = TH * 2, PIECES = XPIECES + 2 * DPIECES;  // 45 + 8 + 8: piece pc lives at byte 1024 pc
  constexpr int MAXOWN = (PIECES + 7) / 8;                                              // 8 (waves 0-4) or 7 pieces per wave and tile
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nh = wave >> 2, kq = wave & 3;
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const WgCols<128> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  // DMA lane constants: lane L of a piece = 16-byte chunk (L&3) of half (L>>5) of pixel row (L>>2)&7 of the 8-pixel block; the
  // source chunk is un-swizzled by the block's parity within its image row
  const int dr = (lane >> 2) & 7;
  const int ch8_0 = 4 * (lane >> 5) + ((lane & 3) ^ ((dr >> 2) & 3)), ch8_1 = 4 * (lane >> 5) + ((lane & 3) ^ ((2 + (dr >> 2)) & 3));
  const unsigned xlane0 = (unsigned)((dr * cs + kloc + ch8_0 * 8) * 2), xlane1 = (unsigned)((dr * cs + kloc + ch8_1 * 8) * 2);
  const unsigned dlane0 = (unsigned)((dr * a.cdy + n0 + ch8_0 * 8) * 2), dlane1 = (unsigned)((dr * a.cdy + n0 + ch8_1 * 8) * 2);
  const bool xok0 = kloc + ch8_0 * 8 < cs, xok1 = kloc + ch8_1 * 8 < cs;
  const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

  // ---- issue state of the tile being fetched
  i32x4 rx, rd;
  int i_oy0 = 0, i_ox0 = 0;
  unsigned i_stage = 0;
  auto prepare = [&](int img, int ty, int tx, unsigned stage_base) {
    i_oy0 = ty * TH; i_ox0 = tx * 16; i_stage = stage_base;
    rx = rsrc_words(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
    rd = rsrc_words(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
  };
  auto issue_piece = [&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    const int pc = wave + 8 * j;  // wave-uniform piece index
    if (pc >= PIECES) return;
    const unsigned dst = i_stage + pc * 1024;
    if (pc < XPIECES) {
      const int iy = pc / XBLK, xb = pc - XBLK * iy;
      const int iy0 = 2 * i_oy0 - 1, ix0 = 2 * i_ox0 - 1;
      const int gy = iy0 + iy, gx = ix0 + 8 * xb + dr;
      const bool ok = ((unsigned)gy < (unsigned)a.Hx) & ((unsigned)gx < (unsigned)a.Wx) & (8 * xb + dr < XW) & ((xb & 1) ? xok1 : xok0);
      const unsigned off = (unsigned)((gy * a.Wx + ix0 + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0);
      dma16<0>(rx, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    } else {
      const int q = pc - XPIECES, h = q >> 3, qq = q & 7;  // 8-pixel block of the dy tile: output row qq >> 1, pixels 8 (qq & 1) ..
      const int gy = i_oy0 + (qq >> 1), gx = i_ox0 + 8 * (qq & 1) + dr;
      const bool ok = (gy < a.Hy) & (gx < a.Wy);
      const unsigned off = (unsigned)((gy * a.Wy + i_ox0 + 8 * (qq & 1)) * a.cdy * 2) + ((qq & 1) ? dlane1 : dlane0) + (unsigned)(h * 128);
      dma16<0>(rd, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    }
  };
#define WG_PIECE(J) issue_piece(std::integral_constant<int, J>{})

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant fragment bases (absolute LDS bytes of stage 0; the stage offset is added per tile)
  const int g1 = grp >> 1, xb0 = 8 * (grp & 1) + qp, sub = 8 * (pp & 1);
  unsigned dbase[2][2], xbase[KS][2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // channel tiles c and c + 2 differ by +512 bytes
    dbase[c][0] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0, 2 * c + (pp >> 1)) + sub;
    dbase[c][1] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0 + 4, 2 * c + (pp >> 1)) + sub;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {  // input row 4 kb + 2 g1 + kh, input column 2 (output pixel) + kw; +4 output pixels = +8 columns
    xbase[kw][0] = lds0 + 2 * g1 * XROW + swz_off(2 * xb0 + kw, 2 * kq + (pp >> 1)) + sub;
    xbase[kw][1] = lds0 + 2 * g1 * XROW + swz_off(2 * xb0 + kw + 8, 2 * kq + (pp >> 1)) + sub;  // (+8 flips the swizzle's bit 1)
  }

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int tile = by;
  int t_tx, t_ty, t_img;  // digits of the NEXT tile to issue
  { int tt = tile; t_tx = tt % a.tiles_x; tt /= a.tiles_x; t_ty = tt % a.tiles_y; t_img = tt / a.tiles_y; }
  int d_tx, d_ty, d_img;
  { int tt = a.ksplit; d_tx = tt % a.tiles_x; tt /= a.tiles_x; d_ty = tt % a.tiles_y; d_img = tt / a.tiles_y; }
  auto advance = [&]() {
    t_tx += d_tx; if (t_tx >= a.tiles_x) { t_tx -= a.tiles_x; t_ty += 1; }
    t_ty += d_ty; if (t_ty >= a.tiles_y) { t_ty -= a.tiles_y; t_img += 1; }
    t_img += d_img;
  };
  int issue_tile = tile;
  unsigned stage = 0;  // stage the CURRENT tile is read from
  if (issue_tile < ntiles) {
    prepare(t_img, t_ty, t_tx, lds0);
    WG_PIECE(0); WG_PIECE(1); WG_PIECE(2); WG_PIECE(3); WG_PIECE(4); WG_PIECE(5); WG_PIECE(6); WG_PIECE(7);
    advance();
  }
  issue_tile += a.ksplit;
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();

  for (; tile < ntiles; tile += a.ksplit) {
    const bool more = issue_tile < ntiles;  // uniform
    if (more) { prepare(t_img, t_ty, t_tx, lds0 + (stage ^ 1) * STAGE); advance(); }
    issue_tile += a.ksplit;
    const unsigned so = stage * STAGE;

    u32x4 af[2][4], bf[3];
    auto load_a = [&](int kb, int c) -> u32x4 {
      const s16x4 lo = tr_read_at(dbase[c & 1][0] + so + 512 * (c >> 1) + 4096 * kb);
      const s16x4 hi = tr_read_at(dbase[c & 1][1] + so + 512 * (c >> 1) + 4096 * kb);
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto load_b = [&](int step) -> u32x4 {  // step = kb * 9 + tap
      const int kb = step / TAPS, t = step % TAPS, kh = t / KS, kw = t % KS;
      const s16x4 lo = tr_read_at(xbase[kw][0] + so + XROW * (4 * kb + kh));
      const s16x4 hi = tr_read_at(xbase[kw][1] + so + XROW * (4 * kb + kh));
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) af[0][c] = load_a(0, c);
    bf[0] = load_b(0);
    bf[1] = load_b(1);
#pragma unroll
    for (int step = 0; step < 2 * TAPS; ++step) {
      const int kb = step / TAPS, t = step % TAPS;
      if (step + 2 < 2 * TAPS) bf[(step + 2) % 3] = load_b(step + 2);
      if (kb == 0 && t >= 5 && t <= 8) af[1][t - 5] = load_a(1, t - 5);  // second row block's dy fragments behind the first's MFMAs
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kb][c]), __builtin_bit_cast(bf16x8, bf[step % 3]),
                                                            acc[t][c], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // tile t + 1: two pieces behind each of the first four steps, so that they have the rest of the tile to land
      if (more) {
        if (step == 0) { WG_PIECE(0); WG_PIECE(1); }
        if (step == 1) { WG_PIECE(2); WG_PIECE(3); }
        if (step == 2) { WG_PIECE(4); WG_PIECE(5); }
        if (step == 3) { WG_PIECE(6); WG_PIECE(7); }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    stage ^= 1;
    wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef WG_PIECE
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 64 * nh + c * 16 + 4 * grp + r, k = k0 + kq * 16 + i16;
        if (kloc + kq * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- bf16, 512-thread big block, ConvTranspose 2x2 / stride 2 (cdy % 128 == 0)
// The weight gradient of nn.ConvTranspose2d(c_below, c, 2, 2) (unet.py:142): "x" = the fine output gradient, "dy" = the coarse input,
// four taps without overlap.  Same block, wave roles, LDS images and transposing reads as wgrad_bf16_bt_s2_kernel with KS = 2 and no
// padding row / column: x tile = 8 fine rows x 32 pixels (32 pieces), 48 KB per stage -> a ring of THREE stages (tile t + 2 issued one
// piece per MFMA step of tile t, counted wait for tile t + 1): 32 MFMAs per wave and tile are too few to hide a DMA round trip
// inside one tile, which the two-stage ring of the 3x3 kernel relies on.
__global__ __launch_bounds__(512, 2) void wgrad_bf16_bt_t2_kernel(const WgArgs a) {
  constexpr int KS = 2, TAPS = 4, TH = 4;
  constexpr int XH = 2 * TH, XBLK = 4, XROW = XBLK * 1024, XW = 32;  // 8 fine rows x 4 blocks of 8 pixels x 128 B
  constexpr int X_BYTES = XH * XROW, DH_BYTES = TH * 16 * 128, D_BYTES = 2 * DH_BYTES, STAGE = X_BYTES + D_BYTES, NSTAGE = 3;
  constexpr int XPIECES = XH * XBLK, DPIECES = TH * 2, PIECES = XPIECES + 2 * DPIECES;  // 32 + 8 + 8: piece pc lives at byte 1024 pc
  constexpr int MAXOWN = PIECES / 8;                                                    // 6 pieces per wave and tile, every wave
  static_assert(PIECES % 8 == 0, "uniform piece count: one counted wait for all waves");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nh = wave >> 2, kq = wave & 3;
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const WgCols<128> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  // DMA lane constants: lane L of a piece = 16-byte chunk (L&3) of half (L>>5) of pixel row (L>>2)&7 of the 8-pixel block; the
  // source chunk is un-swizzled by the block's parity within its image row
  const int dr = (lane >> 2) & 7;
  const int ch8_0 = 4 * (lane >> 5) + ((lane & 3) ^ ((dr >> 2) & 3)), ch8_1 = 4 * (lane >> 5) + ((lane & 3) ^ ((2 + (dr >> 2)) & 3));
  const unsigned xlane0 = (unsigned)((dr * cs + kloc + ch8_0 * 8) * 2), xlane1 = (unsigned)((dr * cs + kloc + ch8_1 * 8) * 2);
  const unsigned dlane0 = (unsigned)((dr * a.cdy + n0 + ch8_0 * 8) * 2), dlane1 = (unsigned)((dr * a.cdy + n0 + ch8_1 * 8) * 2);
  const bool xok0 = kloc + ch8_0 * 8 < cs, xok1 = kloc + ch8_1 * 8 < cs;
  const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

  // ---- issue state of the tile being fetched
  i32x4 rx, rd;
  int i_oy0 = 0, i_ox0 = 0;
  unsigned i_stage = 0;
  auto prepare = [&](int img, int ty, int tx, unsigned stage_base) {
    i_oy0 = ty * TH; i_ox0 = tx * 16; i_stage = stage_base;
    rx = rsrc_words(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
    rd = rsrc_words(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
  };
  auto issue_piece = [&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    const int pc = wave + 8 * j;  // wave-uniform piece index
    if (pc >= PIECES) return;
    const unsigned dst = i_stage + pc * 1024;
    if (pc < XPIECES) {
      const int iy = pc / XBLK, xb = pc - XBLK * iy;
      const int iy0 = 2 * i_oy0, ix0 = 2 * i_ox0;
      const int gy = iy0 + iy, gx = ix0 + 8 * xb + dr;
      const bool ok = ((unsigned)gy < (unsigned)a.Hx) & ((unsigned)gx < (unsigned)a.Wx) & (8 * xb + dr < XW) & ((xb & 1) ? xok1 : xok0);
      const unsigned off = (unsigned)((gy * a.Wx + ix0 + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0);
      dma16<0>(rx, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    } else {
      const int q = pc - XPIECES, h = q >> 3, qq = q & 7;  // 8-pixel block of the dy tile: output row qq >> 1, pixels 8 (qq & 1) ..
      const int gy = i_oy0 + (qq >> 1), gx = i_ox0 + 8 * (qq & 1) + dr;
      const bool ok = (gy < a.Hy) & (gx < a.Wy);
      const unsigned off = (unsigned)((gy * a.Wy + i_ox0 + 8 * (qq & 1)) * a.cdy * 2) + ((qq & 1) ? dlane1 : dlane0) + (unsigned)(h * 128);
      dma16<0>(rd, ok ? off : SENT, __builtin_amdgcn_readfirstlane(dst));
    }
  };
#define WG_PIECE(J) issue_piece(std::integral_constant<int, J>{})

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant fragment bases (absolute LDS bytes of stage 0; the stage offset is added per tile)
  const int g1 = grp >> 1, xb0 = 8 * (grp & 1) + qp, sub = 8 * (pp & 1);
  unsigned dbase[2][2], xbase[KS][2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {  // channel tiles c and c + 2 differ by +512 bytes
    dbase[c][0] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0, 2 * c + (pp >> 1)) + sub;
    dbase[c][1] = lds0 + X_BYTES + nh * DH_BYTES + swz_off(g1 * 16 + xb0 + 4, 2 * c + (pp >> 1)) + sub;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {  // input row 4 kb + 2 g1 + kh, input column 2 (output pixel) + kw; +4 output pixels = +8 columns
    xbase[kw][0] = lds0 + 2 * g1 * XROW + swz_off(2 * xb0 + kw, 2 * kq + (pp >> 1)) + sub;
    xbase[kw][1] = lds0 + 2 * g1 * XROW + swz_off(2 * xb0 + kw + 8, 2 * kq + (pp >> 1)) + sub;  // (+8 flips the swizzle's bit 1)
  }

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int tile = by;
  int t_tx, t_ty, t_img;  // digits of the NEXT tile to issue
  { int tt = tile; t_tx = tt % a.tiles_x; tt /= a.tiles_x; t_ty = tt % a.tiles_y; t_img = tt / a.tiles_y; }
  int d_tx, d_ty, d_img;
  { int tt = a.ksplit; d_tx = tt % a.tiles_x; tt /= a.tiles_x; d_ty = tt % a.tiles_y; d_img = tt / a.tiles_y; }
  auto advance = [&]() {
    t_tx += d_tx; if (t_tx >= a.tiles_x) { t_tx -= a.tiles_x; t_ty += 1; }
    t_ty += d_ty; if (t_ty >= a.tiles_y) { t_ty -= a.tiles_y; t_img += 1; }
    t_img += d_img;
  };
  int issue_tile = tile;
  unsigned stage = 0, issue_stage = 0;  // ring slot the CURRENT tile is read from / the next tile goes to
  int issued = 0;
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {  // prologue: two tiles in flight
    if (issue_tile < ntiles) {
      prepare(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE);
      WG_PIECE(0); WG_PIECE(1); WG_PIECE(2); WG_PIECE(3); WG_PIECE(4); WG_PIECE(5);
      advance();
      ++issued;
    }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;
  }
  if (issued == 2) wait_vm<MAXOWN>(); else wait_vm<0>();
  __builtin_amdgcn_s_barrier();

  for (; tile < ntiles; tile += a.ksplit) {
    const bool more = issue_tile < ntiles;  // uniform
    if (more) { prepare(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;
    const unsigned so = stage * STAGE;

    u32x4 af[2][4], bf[3];
    auto load_a = [&](int kb, int c) -> u32x4 {
      const s16x4 lo = tr_read_at(dbase[c & 1][0] + so + 512 * (c >> 1) + 4096 * kb);
      const s16x4 hi = tr_read_at(dbase[c & 1][1] + so + 512 * (c >> 1) + 4096 * kb);
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
    auto load_b = [&](int step) -> u32x4 {  // step = kb * 4 + tap
      const int kb = step / TAPS, t = step % TAPS, kh = t / KS, kw = t % KS;
      const s16x4 lo = tr_read_at(xbase[kw][0] + so + XROW * (4 * kb + kh));
      const s16x4 hi = tr_read_at(xbase[kw][1] + so + XROW * (4 * kb + kh));
      return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) af[0][c] = load_a(0, c);
    bf[0] = load_b(0);
    bf[1] = load_b(1);
#pragma unroll
    for (int step = 0; step < 2 * TAPS; ++step) {
      const int kb = step / TAPS, t = step % TAPS;
      if (step + 2 < 2 * TAPS) bf[(step + 2) % 3] = load_b(step + 2);
      if (kb == 0) af[1][t] = load_a(1, t);  // second row block's dy fragments behind the first's MFMAs
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kb][c]), __builtin_bit_cast(bf16x8, bf[step % 3]),
                                                            acc[t][c], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // tile t + 2: one piece behind each of the first six steps
      if (more) {
        if (step == 0) WG_PIECE(0);
        if (step == 1) WG_PIECE(1);
        if (step == 2) WG_PIECE(2);
        if (step == 3) WG_PIECE(3);
        if (step == 4) WG_PIECE(4);
        if (step == 5) WG_PIECE(5);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    stage = stage == NSTAGE - 1 ? 0 : stage + 1;
    // own pieces of the tile after next may stay in flight; the next tile's have landed
    if (more) wait_vm<MAXOWN>(); else wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
#undef WG_PIECE
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 64 * nh + c * 16 + 4 * grp + r, k = k0 + kq * 16 + i16;
        if (kloc + kq * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- host launcher
void wgrad_bt_launch(int mode, const WgArgs& a, dim3 grid, hipStream_t st) {
  if (mode == MODE_W3S1) hipLaunchKernelGGL(wgrad_bf16_bt_kernel, grid, dim3(512), 0, st, a);
  else if (mode == MODE_W3S2) hipLaunchKernelGGL(wgrad_bf16_bt_s2_kernel, grid, dim3(512), 0, st, a);
  else hipLaunchKernelGGL(wgrad_bf16_bt_t2_kernel, grid, dim3(512), 0, st, a);
}

#ifdef CONV64_STAMPS
int wgrad_bt_debug_occupancy(int mode) {
  int n = -1;
  hipError_t e = hipErrorInvalidValue;
  if (mode == MODE_W3S1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_bf16_bt_kernel, 512, 0);
  else if (mode == MODE_W3S2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_bf16_bt_s2_kernel, 512, 0);
  return e == hipSuccess ? n : -1;
}
#endif
