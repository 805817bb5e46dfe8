// Weight gradients, stride-1 3x3 bf16 on 64 n x 64 k (256 threads) and 96 n x 96 k (768 threads) blocks: the register-staged
// two-workgroup kernel and the LDS-DMA rings.  See conv_wgrad.hip for the GEMM and wgrad_common.h for the shared pieces.
#include "wgrad_common.h"

// ---------------------------------------------------------------- bf16, two workgroups per CU
// wgrad_bf16_fast_kernel ends up at 464 registers = ONE workgroup of four waves per CU, one wave per SIMD.  Measured on the
// 64-channel launch (rocprofv3 PMC, profiles/r02_pmc_wgrad64.csv): matrix pipe 41 % busy, 3.3 us per 128-pixel tile against
// 1.2 us of MFMA issue -- with a single tile (39 KB) of loads in flight per CU the walk waits on memory latency, and nothing
// covers the staging writes and the two barriers of a tile.  This kernel keeps the same 64(n) x 64(k) x all-taps block per
// workgroup and the same swizzled LDS image, but fits in 256 registers so that TWO workgroups share a CU (two tiles in
// flight, one workgroup's staging / barriers behind the other's MFMAs):
//   * the row-block loop stays ROLLED and its fragment reads are "lane-constant base + immediate": the x image lives at a
//     pitch of 32 pixels (18 used), so a tap / row step is a multiple of 32 LDS rows = 4096 bytes and leaves the swizzle
//     bits alone (unrolled, hipcc hoists one computed address per (row block, tap) and the fragment reads of all row
//     blocks: 464 registers);
//   * staging addresses are branch free and recomputed per tile (a hoisted table is spilled and reloaded behind vmcnt(0)),
//     the tile walk carries (image, row, column) digits instead of dividing.
// Stride-1 3x3 only (the 32-pixel pitch); the stride-2 / transposed shapes stay on wgrad_bf16_fast_kernel.
// Diagnostic build only (-DCONV64_STAMPS, tools/conv64_stamps.py wgrad): per-wave cycle sums of a tile's phases.
#ifdef CONV64_STAMPS
__device__ unsigned long long wgrad_dbg[512 * 4 * 8];
#define WSTAMP(var)                                                                  \
  do {                                                                               \
    __builtin_amdgcn_sched_barrier(0);                                               \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");      \
    __builtin_amdgcn_sched_barrier(0);                                               \
  } while (0)
extern "C" int mia_wgrad_debug_read(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(wgrad_dbg), sizeof(wgrad_dbg));
}
#else
#define WSTAMP(var) do { } while (0)
#endif

// NL = normalise-on-load of the x operand (see conv64.hip: the consumer-side half of the fused PlainBlock): x1 holds the
// producer's raw conv output and commit() turns each staged 16-byte unit into bf16(lrelu(scale * y + shift)) -- bit for bit the
// activation mia_norm_act_fwd would have written -- with the coefficients of the tile's image in a 512-byte LDS table
// (threads 0..127 fetch one entry each with the tile), and halo units outside the image forced back to zero.
template <int TH, bool NL = false>
__global__ __launch_bounds__(256, 2) void wgrad_bf16_2wg_kernel(const WgArgs a) {
  constexpr int KS = 3, PAD = 1, TAPS = 9;
  constexpr int XH = TH - 1 + KS, XW = 15 + KS, XP = 32;
  constexpr int X_IT = (XH * XW + 31) / 32, D_IT = TH * 16 / 32;  // 32 pixels x 8 chunks per staging iteration
  constexpr int X_BYTES = XH * XP * 128, D_BYTES = TH * 16 * 128;
  static_assert(X_IT == 6 && D_IT == 4, "the staging table below is laid out for TH = 8");
  __shared__ __attribute__((aligned(16))) unsigned char smem[X_BYTES + D_BYTES + 4 * 256 * 16 + (NL ? 512 : 0)];
  u32x4* tab = reinterpret_cast<u32x4*>(smem + X_BYTES + D_BYTES);  // [4][256]: per-thread staging constants, see below
  float* cft = reinterpret_cast<float*>(smem + X_BYTES + D_BYTES + 4 * 256 * 16);  // NL: [0, 64) scale, [64, 128) shift (this k block, committed tile's image)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const int ch8 = tid & 7, p8 = tid >> 3;
  const WgCols<64> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;
  const bool x_chan_ok = kloc + ch8 * 8 < cs, d_chan_ok = n0 + ch8 * 8 < a.cdy;

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int tile = by;
  int t_tx, t_ty, t_img;
  { int tt = tile; t_tx = tt % a.tiles_x; tt /= a.tiles_x; t_ty = tt % a.tiles_y; t_img = tt / a.tiles_y; }
  int d_tx, d_ty, d_img;
  { int tt = a.ksplit; d_tx = tt % a.tiles_x; tt /= a.tiles_x; d_ty = tt % a.tiles_y; d_img = tt / a.tiles_y; }

  // Per-thread staging constants live in LDS, not in registers (there are none to spare) and not in VALU work per tile
  // (measured with the stamps build: ~200 address instructions per tile, issued at half rate beside the other workgroup's
  // MFMAs, made the fetch phase 1800 cycles of an 8000-cycle tile): for a tile whose halo lies inside the image the ten
  // global offsets are "tile origin (folded into the buffer descriptor) + constant", and the six LDS offsets are constant.
  //   tab[0] = x offsets 0..3, tab[1] = x offsets 4..5 | dy offsets 0..1, tab[2] = dy offsets 2..3 | LDS offsets 0..1,
  //   tab[3] = LDS offsets 2..5
  {
    unsigned xo[X_IT], xl[X_IT], dofs[D_IT];
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      const int pix = p8 + 32 * i, iy = pix / XW, ix = pix - iy * XW;
      xo[i] = (pix < XH * XW && x_chan_ok) ? (unsigned)(((iy * a.Wx + ix) * cs + kloc + ch8 * 8) * 2) : SENT;
      xl[i] = (unsigned)swz_off(iy * XP + ix, ch8);
    }
#pragma unroll
    for (int i = 0; i < D_IT; ++i) {
      const int pix = p8 + 32 * i;
      dofs[i] = d_chan_ok ? (unsigned)((((pix >> 4) * a.Wy + (pix & 15)) * a.cdy + n0 + ch8 * 8) * 2) : SENT;
    }
    tab[tid] = u32x4{xo[0], xo[1], xo[2], xo[3]};
    tab[256 + tid] = u32x4{xo[4], xo[5], dofs[0], dofs[1]};
    tab[512 + tid] = u32x4{dofs[2], dofs[3], xl[0], xl[1]};
    tab[768 + tid] = u32x4{xl[2], xl[3], xl[4], xl[5]};
  }

  u32x4 px[X_IT], pd[D_IT];
  float cpf = 0.f;  // NL: this thread's entry of the fetched tile's coefficient table
  auto fetch = [&](int img, int ty, int tx) {
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 - PAD, ix0 = ox0 - PAD;
    if constexpr (NL) {
      if (wave < 2) {  // wave 0 fetches the 64 scales, wave 1 the 64 shifts: the array pointer stays scalar
        const float* cp = wave == 0 ? a.nl_scale : a.nl_shift;
        int lv = lane;
        asm volatile("" : "+v"(lv));  // recomputed per tile: a hoisted 64-bit lane address would be spilled around the tile loop
        const int ch = kloc + lv;
        cpf = ch < cs ? cp[(unsigned)(img * cs + ch)] : 0.f;  // scalar base + 32-bit lane offset
      }
    }
    if ((a.opt & 1) && iy0 >= 0 && ix0 >= 0 && iy0 + XH <= a.Hx && ix0 + XW <= a.Wx && oy0 + TH <= a.Hy && ox0 + 16 <= a.Wy) {
      const size_t xorg = (size_t)iy0 * a.Wx + ix0, dorg = (size_t)oy0 * a.Wy + ox0;
      const rsrc_t rx = make_rsrc(xsrc + ((size_t)img * xpix + xorg) * cs, (unsigned)((xpix - xorg) * cs * 2));
      const rsrc_t rd = make_rsrc(dy + ((size_t)img * ypix + dorg) * a.cdy, (unsigned)((ypix - dorg) * a.cdy * 2));
      const u32x4 t0 = tab[tid], t1 = tab[256 + tid], t2 = tab[512 + tid];
      px[0] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t0.x, 0, 0);
      px[1] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t0.y, 0, 0);
      px[2] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t0.z, 0, 0);
      px[3] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t0.w, 0, 0);
      px[4] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t1.x, 0, 0);
      px[5] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)t1.y, 0, 0);
      pd[0] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)t1.z, 0, 0);
      pd[1] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)t1.w, 0, 0);
      pd[2] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)t2.x, 0, 0);
      pd[3] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)t2.y, 0, 0);
      return;
    }
    const rsrc_t rx = make_rsrc(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
    const rsrc_t rd = make_rsrc(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
    int p8v = p8;
    asm volatile("" : "+v"(p8v));
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      const int pix = p8v + 32 * i, iy = pix / XW, ix = pix - iy * XW;
      const int gy = iy0 + iy, gx = ix0 + ix;
      const int okm = -(int)(((unsigned)gy < (unsigned)a.Hx) & ((unsigned)gx < (unsigned)a.Wx) & (pix < XH * XW) & x_chan_ok);
      const unsigned off = (unsigned)(((gy * a.Wx + gx) * cs + kloc + ch8 * 8) * 2);
      px[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)((off & (unsigned)okm) | (SENT & ~(unsigned)okm)), 0, 0);
    }
#pragma unroll
    for (int i = 0; i < D_IT; ++i) {
      const int pix = p8v + 32 * i;
      const int gy = oy0 + (pix >> 4), gx = ox0 + (pix & 15);
      const int okm = -(int)((gy < a.Hy) & (gx < a.Wy) & d_chan_ok);
      const unsigned off = (unsigned)(((gy * a.Wy + gx) * a.cdy + n0 + ch8 * 8) * 2);
      pd[i] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)((off & (unsigned)okm) | (SENT & ~(unsigned)okm)), 0, 0);
    }
  };
  auto commit = [&](int ty, int tx) {
    int p8v = p8;
    asm volatile("" : "+v"(p8v));
    if constexpr (NL) {
      const f32x4* cf4 = reinterpret_cast<const f32x4*>(cft);
      const int iy0 = ty * TH - PAD, ix0 = tx * 16 - PAD;
      const bool interior = iy0 >= 0 && ix0 >= 0 && iy0 + XH <= a.Hx && ix0 + XW <= a.Wx;  // uniform
      typedef float nl_f32x2 __attribute__((ext_vector_type(2)));
      typedef __bf16 nl_bf16x2 __attribute__((ext_vector_type(2)));
      const nl_f32x2 sl2 = {a.nl_slope, a.nl_slope};
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {  // dwords 0,1 then 2,3 of every unit: 8 coefficient registers live at a time
        const f32x4 sc = cf4[2 * ch8 + hf], sh = cf4[16 + 2 * ch8 + hf];
#pragma unroll
        for (int i = 0; i < X_IT; ++i) {
#pragma unroll
          for (int d = 0; d < 2; ++d) {  // packed fp32 math: one issue slot per channel pair (v_pk_fma_f32, v_pk_mul_f32)
            const unsigned w = px[i][2 * hf + d];
            const nl_f32x2 x = {__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xFFFF0000u)};
            const nl_f32x2 v = __builtin_elementwise_fma(nl_f32x2{sc[2 * d], sc[2 * d + 1]}, x, nl_f32x2{sh[2 * d], sh[2 * d + 1]});
            const nl_f32x2 m = v * sl2;
            // (channels past `cs` carry scale = shift = 0 in the table: lrelu(0) = 0)
            px[i][2 * hf + d] = __builtin_bit_cast(unsigned, __builtin_convertvector(nl_f32x2{__builtin_fmaxf(v[0], m[0]), __builtin_fmaxf(v[1], m[1])}, nl_bf16x2));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (!interior) {  // border tile: halo units outside the image go back to zero
#pragma unroll
        for (int i = 0; i < X_IT; ++i) {
          const int pix = p8v + 32 * i, iy = pix / XW, ix = pix - iy * XW;
          const unsigned keep = 0u - (unsigned)(((unsigned)(iy0 + iy) < (unsigned)a.Hx) & ((unsigned)(ix0 + ix) < (unsigned)a.Wx));
#pragma unroll
          for (int d = 0; d < 4; ++d) px[i][d] &= keep;
        }
      }
    }
    const u32x4 t2 = tab[512 + tid], t3 = tab[768 + tid];
    *reinterpret_cast<u32x4*>(smem + t2.z) = px[0];
    *reinterpret_cast<u32x4*>(smem + t2.w) = px[1];
    *reinterpret_cast<u32x4*>(smem + t3.x) = px[2];
    *reinterpret_cast<u32x4*>(smem + t3.y) = px[3];
    *reinterpret_cast<u32x4*>(smem + t3.z) = px[4];
    if (p8v + 32 * 5 < XH * XW) *reinterpret_cast<u32x4*>(smem + t3.w) = px[5];
    const int d0 = swz_off(p8v, ch8);  // + 4096 per iteration (32 rows)
#pragma unroll
    for (int i = 0; i < D_IT; ++i) *reinterpret_cast<u32x4*>(smem + X_BYTES + d0 + 4096 * i) = pd[i];
  };

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant read bases (bytes).  Lane group `grp` covers pixels 8*(grp&1) .. +7 of output row 2*kb + (grp>>1); a
  // transposing read fetches 4 consecutive pixel rows, the pair (lo, hi) = rows r0 .. r0+3 and r0+4 .. r0+7.
  const int g1 = grp >> 1, xb = 8 * (grp & 1) + qp, sub = 8 * (pp & 1);
  const int lds0 = (int)(unsigned)(size_t)(lds_u8*)smem;  // absolute LDS address of the tile image
  int dbase[4][2], xbase[KS][2];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    dbase[c][0] = lds0 + X_BYTES + swz_off(g1 * 16 + xb, 2 * c + (pp >> 1)) + sub;
    dbase[c][1] = lds0 + X_BYTES + swz_off(g1 * 16 + xb + 4, 2 * c + (pp >> 1)) + sub;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {
    xbase[kw][0] = lds0 + swz_off(g1 * XP + xb + kw, 2 * wave + (pp >> 1)) + sub;
    xbase[kw][1] = lds0 + swz_off(g1 * XP + xb + kw + 4, 2 * wave + (pp >> 1)) + sub;
  }

  if (tile < ntiles) fetch(t_img, t_ty, t_tx);
#ifdef CONV64_STAMPS
  unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0, a_b1 = 0, a_c = 0, a_b2 = 0, a_f = 0, a_m = 0, a_n = 0;
#endif
  for (; tile < ntiles; tile += a.ksplit) {
    WSTAMP(w0);
    if constexpr (NL) {  // the table is read in commit() only, i.e. between the two barriers below
      if (tid < 128) cft[tid] = cpf;
    }
    __syncthreads();  // previous tile's fragment reads are done
    WSTAMP(w1);
    commit(t_ty, t_tx);
    WSTAMP(w2);
    __syncthreads();
    WSTAMP(w3);
    if (tile + a.ksplit < ntiles) {
      t_tx += d_tx; if (t_tx >= a.tiles_x) { t_tx -= a.tiles_x; t_ty += 1; }
      t_ty += d_ty; if (t_ty >= a.tiles_y) { t_ty -= a.tiles_y; t_img += 1; }
      t_img += d_img;
      fetch(t_img, t_ty, t_tx);
    }
    WSTAMP(w4);
#pragma unroll 1
    for (int kb = 0; kb < TH / 2; ++kb) {
      const int koff = 4096 * kb;  // 32 dy rows per row block; the x image advances two 32-pixel rows
      u32x4 af[4], bf[2];
      auto load_b = [&](int t) -> u32x4 {
        const int kh = t / KS, kw = t % KS;
        const s16x4 lo = tr_read_at((unsigned)(xbase[kw][0] + 2 * koff + 4096 * kh));
        const s16x4 hi = tr_read_at((unsigned)(xbase[kw][1] + 2 * koff + 4096 * kh));
        return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      };
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const s16x4 lo = tr_read_at((unsigned)(dbase[c][0] + koff));
        const s16x4 hi = tr_read_at((unsigned)(dbase[c][1] + koff));
        af[c] = __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
      bf[0] = load_b(0);
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        if (t + 1 < TAPS) bf[(t + 1) & 1] = load_b(t + 1);  // next tap's fragment ahead of this tap's MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[c]), __builtin_bit_cast(bf16x8, bf[t & 1]),
                                                              acc[t][c], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    WSTAMP(w5);
#ifdef CONV64_STAMPS
    a_b1 += w1 - w0; a_c += w2 - w1; a_b2 += w3 - w2; a_f += w4 - w3; a_m += w5 - w4; a_n += 1;
#endif
  }
#ifdef CONV64_STAMPS
  if (lane == 0 && bx == 0 && by < 512) {
    unsigned long long* d = wgrad_dbg + ((size_t)by * 4 + wave) * 8;
    d[0] = a_b1; d[1] = a_c; d[2] = a_b2; d[3] = a_f; d[4] = a_m; d[5] = a_n;
  }
#endif
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + c * 16 + 4 * grp + r, k = k0 + wave * 16 + i16;
        if (kloc + wave * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- bf16, LDS-DMA ring (stride-1 3x3)
// Same block per workgroup (64 n x 64 k x 9 taps), same swizzled LDS image and fragment reads as wgrad_bf16_2wg_kernel, but
// the tiles arrive by LDS-DMA (`buffer_load_dwordx4 ... offen lds`: no staging registers, no ds_write pass, no second
// barrier) into a ring of THREE tile images, so a tile's loads have two tile times to land:
//   * a tile is 4 output rows x 16 pixels: x image [6 rows][24 pixels (18 used)][64 ch] = 18 KB, dy image [64 px][64 ch] =
//     8 KB; 3 x 26 KB = 78 KB per workgroup, two workgroups per CU (156 of 160 KB);
//   * one DMA instruction writes 1 KB = one 8-pixel x 128-byte row block of the image, lane L at byte 16 L; the chunk
//     swizzle is applied on the SOURCE side (lane L fetches chunk (L&3) ^ swizzle(row)), out-of-image / out-of-channel lanes
//     point past the descriptor and are zero filled.  26 pieces per tile, dealt round-robin to the 4 waves;
//   * per tile: issue tile t+2 -> MFMAs of tile t -> s_waitcnt vmcnt(own pieces of t+2) [= own pieces of t+1 landed] ->
//     s_barrier [everyone's pieces of t+1 landed, everyone done reading t].  The DMA is issued and counted in inline asm
//     (hipcc would drain it with vmcnt(0) at every barrier / LDS read it can see);
//   * the 40 staging registers of the 2wg kernel pay for a second set of dy fragments and a three-deep x fragment ring, so
//     the fragment reads run two taps ahead of their MFMAs.
// (A form that skipped a narrow block's empty 16-channel tiles measured no gain and is gone: profiles/r04_ab_wgrad_narrow.txt.)
__global__ __launch_bounds__(256, 2) void wgrad_bf16_dma_kernel(const WgArgs a) {
  constexpr int KS = 3, TAPS = 9, TH = 4;
  constexpr int XH = TH + 2, XROW = 3072;  // 24 pixels x 128 B per image row of the x tile
  constexpr int X_BYTES = XH * XROW, D_BYTES = TH * 16 * 128, STAGE = X_BYTES + D_BYTES, NSTAGE = 3;
  constexpr int XPIECES = XH * 3, PIECES = XPIECES + TH * 2;  // 18 + 8
  constexpr int MAXOWN = (PIECES + 3) / 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const WgCols<64> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  // DMA lane constants: lane L of a piece is 16-byte chunk (L&3) of half (L>>5) of pixel row r = (L>>2)&7 of the 8-row block;
  // the source chunk is un-swizzled by the block's parity p (rows 8 blk + r: (row>>2)&3 = (2 p + (r>>2)) & 3)
  const int dr = (lane >> 2) & 7;
  // (plain scalars, not arrays: a wave-uniform but run-time index sends an array to scratch, whose reload waits vmcnt(0))
  const int ch8_0 = 4 * (lane >> 5) + ((lane & 3) ^ ((dr >> 2) & 3)), ch8_1 = 4 * (lane >> 5) + ((lane & 3) ^ ((2 + (dr >> 2)) & 3));
  const unsigned xlane0 = (unsigned)((dr * cs + kloc + ch8_0 * 8) * 2), xlane1 = (unsigned)((dr * cs + kloc + ch8_1 * 8) * 2);
  const unsigned dlane0 = (unsigned)((dr * a.cdy + n0 + ch8_0 * 8) * 2), dlane1 = (unsigned)((dr * a.cdy + n0 + ch8_1 * 8) * 2);
  const bool xok0 = kloc + ch8_0 * 8 < cs, xok1 = kloc + ch8_1 * 8 < cs;
  const bool dok0 = n0 + ch8_0 * 8 < a.cdy, dok1 = n0 + ch8_1 * 8 < a.cdy;
  const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

  auto issue = [&](int img, int ty, int tx, unsigned stage_base) {
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    const i32x4 rx = rsrc_words(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
    const i32x4 rd = rsrc_words(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
#pragma unroll
    for (int j = 0; j < MAXOWN; ++j) {
      const int pc = wave + 4 * j;  // wave-uniform piece index
      if (pc < XPIECES) {
        const int iy = pc / 3, xb = pc - 3 * iy;
        const int gy = iy0 + iy, gx = ix0 + 8 * xb + dr;
        const bool ok = ((unsigned)gy < (unsigned)a.Hx) & ((unsigned)gx < (unsigned)a.Wx) & (8 * xb + dr < 18) & ((xb & 1) ? xok1 : xok0);
        const unsigned off = (unsigned)((gy * a.Wx + ix0 + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0);
        dma16<0>(rx, ok ? off : SENT, __builtin_amdgcn_readfirstlane(stage_base + iy * XROW + xb * 1024));
      } else if (pc < PIECES) {
        const int q = pc - XPIECES;  // 8-pixel block of the dy tile: output row q>>1, pixels 8 (q&1) ..
        const int gy = oy0 + (q >> 1), gx = ox0 + 8 * (q & 1) + dr;
        const bool ok = (gy < a.Hy) & (gx < a.Wy) & ((q & 1) ? dok1 : dok0);
        const unsigned off = (unsigned)((gy * a.Wy + ox0 + 8 * (q & 1)) * a.cdy * 2) + ((q & 1) ? dlane1 : dlane0);
        dma16<0>(rd, ok ? off : SENT, __builtin_amdgcn_readfirstlane(stage_base + X_BYTES + q * 1024));
      }
    }
  };
  // Tiles whose 18 columns lie inside the image (all but the first / last tile of a row): the lane part of every piece's
  // offset is a constant (kept in registers, padding / channel-tail lanes already pointing out of range), the tile origin
  // goes into the descriptor base and a piece's rows are valid or not as a whole.  Measured with the stamps build: the
  // general issue() above costs ~1700 cycles per tile and wave (as long as the tile's MFMAs), this one a fraction.
  unsigned voffc[MAXOWN];
#pragma unroll
  for (int j = 0; j < MAXOWN; ++j) {
    const int pc = wave + 4 * j;
    if (pc < XPIECES) {
      const int iy = pc / 3, xb = pc - 3 * iy, ix = 8 * xb + dr;
      const bool ok = (ix < 18) & ((xb & 1) ? xok1 : xok0);
      voffc[j] = ok ? (unsigned)((iy * a.Wx + 8 * xb) * cs * 2) + ((xb & 1) ? xlane1 : xlane0) : SENT;
    } else {
      const int q = pc - XPIECES;
      const bool ok = (pc < PIECES) & ((q & 1) ? dok1 : dok0);
      voffc[j] = ok ? (unsigned)(((q >> 1) * a.Wy + 8 * (q & 1)) * a.cdy * 2) + ((q & 1) ? dlane1 : dlane0) : SENT;
    }
  }
  auto issue_fast = [&](int img, int ty, int tx, unsigned stage_base) {
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    // descriptor bases at the tile origin (row iy0 may be -1: its pieces are dropped below, nothing is read through it)
    const long long xorg = ((long long)(img * a.Hx + iy0) * a.Wx + ix0) * cs;
    const long long dorg = ((long long)(img * a.Hy + oy0) * a.Wy + ox0) * a.cdy;
    const i32x4 rx = rsrc_words(xsrc + xorg, (unsigned)(XH * a.Wx * cs * 2));
    const i32x4 rd = rsrc_words(dy + dorg, (unsigned)(TH * a.Wy * a.cdy * 2));
    const unsigned m0base = stage_base + wave * 1024;  // piece pc of the tile image lives at byte 1024 pc
#pragma unroll
    for (int j = 0; j < MAXOWN; ++j) {
      const int pc = wave + 4 * j;
      const bool is_x = 4 * j + 3 < XPIECES || (4 * j < XPIECES && pc < XPIECES);
      const bool is_d = !is_x && (4 * j + 3 < PIECES || pc < PIECES);
      if (is_x) {
        const bool rowok = (unsigned)(iy0 + pc / 3) < (unsigned)a.Hx;
        dma16<0>(rx, rowok ? voffc[j] : SENT, m0base + 4096 * j);
      } else if (is_d) {
        const bool rowok = oy0 + ((pc - XPIECES) >> 1) < a.Hy;
        dma16<0>(rd, rowok ? voffc[j] : SENT, m0base + 4096 * j);
      }
    }
  };
  auto issue_any = [&](int img, int ty, int tx, unsigned stage_base) {
    if (tx > 0 && tx * 16 + 17 <= a.Wx && tx * 16 + 16 <= a.Wy) issue_fast(img, ty, tx, stage_base);
    else issue(img, ty, tx, stage_base);
  };
  // this wave's pieces per tile: waves with wave < PIECES % 4 own one more
  auto wait_own_in_flight = [&]() {  // all but the newest tile's own pieces have landed
    if (wave < (PIECES & 3)) wait_vm<MAXOWN>();
    else wait_vm<MAXOWN - 1>();
  };

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant fragment bases (absolute LDS bytes of the CURRENT stage; stepped by one stage per tile)
  const int g1 = grp >> 1, xb0 = 8 * (grp & 1) + qp, sub = 8 * (pp & 1);
  unsigned dbase[4][2], xbase[KS][2];  // wave w owns k tile w against the block's four n tiles
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    dbase[c][0] = lds0 + X_BYTES + swz_off(g1 * 16 + xb0, 2 * c + (pp >> 1)) + sub;
    dbase[c][1] = lds0 + X_BYTES + swz_off(g1 * 16 + xb0 + 4, 2 * c + (pp >> 1)) + sub;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {
    xbase[kw][0] = lds0 + g1 * XROW + swz_off(xb0 + kw, 2 * wave + (pp >> 1)) + sub;
    xbase[kw][1] = lds0 + g1 * XROW + swz_off(xb0 + kw + 4, 2 * wave + (pp >> 1)) + sub;
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
    if (issue_tile < ntiles) { issue_any(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;
  }
  if (tile + a.ksplit < ntiles) wait_own_in_flight(); else wait_vm<0>();
  __builtin_amdgcn_s_barrier();

  int stage = 0;
#ifdef CONV64_STAMPS
  unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0, w4 = 0, a_i = 0, a_m = 0, a_w = 0, a_b = 0, a_n = 0, c_t0, c_r0, c_t1, c_r1;
  WSTAMP(c_t0);
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_r0)::"memory");
#endif
  for (; tile < ntiles; tile += a.ksplit) {
    WSTAMP(w0);
    const bool more = issue_tile < ntiles;
    if (more) { issue_any(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;

    WSTAMP(w1);
    {
      u32x4 af[2][4], bf[3];
      auto load_a = [&](int kb, int c) -> u32x4 {
        const s16x4 lo = tr_read_at(dbase[c][0] + 4096 * kb);
        const s16x4 hi = tr_read_at(dbase[c][1] + 4096 * kb);
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
      }
    }
    // next stage's fragment bases
    const int delta = stage == NSTAGE - 1 ? -(NSTAGE - 1) * STAGE : STAGE;
    stage = stage == NSTAGE - 1 ? 0 : stage + 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) { dbase[c][0] += delta; dbase[c][1] += delta; }
#pragma unroll
    for (int kw = 0; kw < KS; ++kw) { xbase[kw][0] += delta; xbase[kw][1] += delta; }
    WSTAMP(w2);
    if (more) wait_own_in_flight(); else wait_vm<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    WSTAMP(w3);
    __builtin_amdgcn_s_barrier();
    WSTAMP(w4);
#ifdef CONV64_STAMPS
    a_i += w1 - w0; a_m += w2 - w1; a_w += w3 - w2; a_b += w4 - w3; a_n += 1;
#endif
  }
#ifdef CONV64_STAMPS
  if (lane == 0 && bx == 0 && by < 512) {
    unsigned long long* d = wgrad_dbg + ((size_t)by * 4 + wave) * 8;
    WSTAMP(c_t1);
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_r1)::"memory");
    d[0] = a_i; d[1] = a_m; d[2] = a_w; d[3] = a_b; d[4] = 0; d[5] = a_n; d[6] = c_t1 - c_t0; d[7] = c_r1 - c_r0;
  }
#endif
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + c * 16 + 4 * grp + r, k = k0 + wave * 16 + i16;
        if (kloc + wave * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
  // (slab entries this block does not compute -- padded n / k tiles -- are never read: mia_wgrad_reduce sums n < nn, k < kk only)
}

// ---------------------------------------------------------------- bf16, LDS-DMA ring, 96-wide blocks (stride-1 3x3; cfg5's level 0)
// Channel counts that are multiples of 96 and not of 64 cost the 64-wide kernel 2 x 2 blocks per 96 x 96 of dW: 1.78x the MFMAs and the
// x / dy tiles fetched L2 -> LDS four times -- and that fill, not the MFMAs, is what the launch waits for (skipping the empty MFMA tiles
// measured +-0 in round 4; a register-staged 96-wide block measured slower in round 5).  This is the ring kernel on 96-wide images:
//   * a tile is 4 output rows x 16 pixels: x image [6 rows][24 pixels][96 ch] = 27 KB, dy image [64 px][96 ch] = 12 KB, as 32-channel
//     subtiles of 8 pixels x 64 B (THREE per 8-pixel group, same chunk swizzle as the 64-wide image); ring of three images = 117 KB,
//     one 768-thread workgroup per CU;
//   * a DMA piece is 1 KB = two consecutive subtiles: 27 + 12 = 39 pieces per tile dealt round-robin to the twelve waves (3 or 4 each);
//     lane L of a piece is chunk slot L & 3 of pixel (L >> 2) & 7 of subtile 2 p + (L >> 5), the source chunk un-swizzled, out-of-image /
//     out-of-channel lanes pointing past the descriptor (zero fill).  Per-lane offsets are tile-invariant (relative to the tile origin,
//     which rides in the descriptor); what changes per tile is which rows / columns exist;
//   * waves = 6 input-channel tiles x 2 halves of the six output-channel tiles: 27 accumulator tiles, 54 MFMAs per wave and tile;
//   * per tile: issue tile t + 2 -> MFMAs of tile t -> s_waitcnt vmcnt(own pieces of t + 2) -> s_barrier (the 64-wide kernel's protocol).
template <int DUMMY>
__global__ __launch_bounds__(768) void wgrad_bf16_dma96_kernel(const WgArgs a) {
  constexpr int KS = 3, TAPS = 9, TH = 4, CW = 96;
  constexpr int XH = TH + 2, XROW = 3 * 3 * 512;  // 24 pixels = 3 groups of 8, x 3 subtiles of 512 B
  constexpr int X_BYTES = XH * XROW, D_BYTES = TH * 2 * 3 * 512, STAGE = X_BYTES + D_BYTES, NSTAGE = 3;
  constexpr int XPIECES = X_BYTES / 1024, PIECES = XPIECES + D_BYTES / 1024;  // 27 + 12
  constexpr int NWAVE = 12, MAXOWN = (PIECES + NWAVE - 1) / NWAVE, NC = 3;
  static_assert(X_BYTES % 1024 == 0 && D_BYTES % 1024 == 0, "whole pieces");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NSTAGE * STAGE];
  auto swz = [](int row, int ch) { return 512 * ((row >> 3) * 3 + (ch >> 2)) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3)); };

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const int ktile = wave % 6, nh = (wave / 6) * NC;
  const WgCols<CW> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const unsigned lds0 = (unsigned)(size_t)(lds_u8*)smem;

  // tile-invariant lane constants of this wave's pieces: byte offset from the tile origin (SENT: padding pixel / channel tail) and the
  // (row, column) the lane's pixel has inside the tile, to be checked against the image per tile
  unsigned voffc[MAXOWN];
  int rcc[MAXOWN];  // row << 8 | column (one register per piece: the kernel sits at the 168 registers three waves per SIMD allow)
  const int hl = lane >> 5, r8 = (lane >> 2) & 7, slot4 = lane & 3;
#pragma unroll
  for (int j = 0; j < MAXOWN; ++j) {
    const int pc = wave + NWAVE * j;
    voffc[j] = SENT; rcc[j] = 0;
    if (pc < XPIECES) {
      const int t = 2 * pc + hl;                       // subtile of the x image
      const int iy = t / 9, gx = (t % 9) / 3, sub = t % 3;
      const int px = 8 * gx + r8, c = 4 * sub + (slot4 ^ ((px >> 2) & 3));
      rcc[j] = iy << 8 | px;
      if (px < 18 && kloc + c * 8 < cs) voffc[j] = (unsigned)(((iy * a.Wx + px) * cs + kloc + c * 8) * 2);
    } else if (pc < PIECES) {
      const int t = 2 * (pc - XPIECES) + hl;           // subtile of the dy image
      const int g8 = t / 3, sub = t % 3;
      const int P = 8 * g8 + r8, c = 4 * sub + (slot4 ^ ((P >> 2) & 3));
      rcc[j] = (P >> 4) << 8 | (P & 15);
      if (n0 + c * 8 < a.cdy) voffc[j] = (unsigned)((((P >> 4) * a.Wy + (P & 15)) * a.cdy + n0 + c * 8) * 2);
    }
  }
  auto issue = [&](int img, int ty, int tx, unsigned stage_base) {
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 - 1, ix0 = ox0 - 1;
    // descriptor bases at the tile origin (may lie one row / one pixel in front of the image: those lanes are masked, nothing is read through them)
    const long long xorg = ((long long)(img * a.Hx + iy0) * a.Wx + ix0) * cs;
    const long long dorg = ((long long)(img * a.Hy + oy0) * a.Wy + ox0) * a.cdy;
    // (ranges: the last tile row reaches 17 / 15 pixels past its first column, which is more than an image row when the image is
    // narrower than the tile -- the per-lane row / column masks, not the range, keep the loads inside the tensor)
    const i32x4 rx = rsrc_words(xsrc + xorg, (unsigned)((XH * a.Wx + 24) * cs * 2));
    const i32x4 rd = rsrc_words(dy + dorg, (unsigned)((TH * a.Wy + 16) * a.cdy * 2));
    const unsigned m0base = stage_base + wave * 1024;  // piece pc of the tile image lives at byte 1024 pc
#pragma unroll
    for (int j = 0; j < MAXOWN; ++j) {
      const int pc = wave + NWAVE * j;  // wave-uniform
      if (pc < XPIECES) {
        const bool ok = ((unsigned)(iy0 + (rcc[j] >> 8)) < (unsigned)a.Hx) & ((unsigned)(ix0 + (rcc[j] & 255)) < (unsigned)a.Wx);
        dma16<0>(rx, ok ? voffc[j] : SENT, m0base + NWAVE * 1024 * j);
      } else if (pc < PIECES) {
        const bool ok = (oy0 + (rcc[j] >> 8) < a.Hy) & (ox0 + (rcc[j] & 255) < a.Wy);
        dma16<0>(rd, ok ? voffc[j] : SENT, m0base + NWAVE * 1024 * j);
      }
    }
  };
  auto wait_own_in_flight = [&]() {  // all but the newest tile's own pieces have landed
    if (wave < (PIECES % NWAVE)) wait_vm<MAXOWN>();
    else wait_vm<MAXOWN - 1>();
  };

  f32x4 acc[TAPS][NC];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane-constant fragment bases (absolute LDS bytes of the CURRENT stage; stepped by one stage per tile)
  const int g1 = grp >> 1, xb0 = 8 * (grp & 1) + qp, sub8 = 8 * (pp & 1);
  unsigned dbase[NC][2], xbase[KS][2];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dbase[c][0] = lds0 + X_BYTES + swz(g1 * 16 + xb0, 2 * (nh + c) + (pp >> 1)) + sub8;
    dbase[c][1] = lds0 + X_BYTES + swz(g1 * 16 + xb0 + 4, 2 * (nh + c) + (pp >> 1)) + sub8;
  }
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) {
    xbase[kw][0] = lds0 + g1 * XROW + swz(xb0 + kw, 2 * ktile + (pp >> 1)) + sub8;
    xbase[kw][1] = lds0 + g1 * XROW + swz(xb0 + kw + 4, 2 * ktile + (pp >> 1)) + sub8;
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
  unsigned issue_stage = 0;
#pragma unroll 1
  for (int s_ = 0; s_ < 2; ++s_) {  // prologue: two tiles in flight
    if (issue_tile < ntiles) { issue(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;
  }
  if (tile + a.ksplit < ntiles) wait_own_in_flight(); else wait_vm<0>();
  __builtin_amdgcn_s_barrier();

  int stage = 0;
  for (; tile < ntiles; tile += a.ksplit) {
    const bool more = issue_tile < ntiles;
    if (more) { issue(t_img, t_ty, t_tx, lds0 + issue_stage * STAGE); advance(); }
    issue_tile += a.ksplit;
    issue_stage = issue_stage == NSTAGE - 1 ? 0 : issue_stage + 1;

    {
      u32x4 af[NC], bf[3];  // (ONE set of dy fragments, reloaded between the two row blocks: a second set does not fit 168 registers)
      auto load_a = [&](int kb, int c) -> u32x4 {  // 32 pixels = 4 groups of 8 x 3 subtiles = 6144 B per row block
        const s16x4 lo = tr_read_at(dbase[c][0] + 6144 * kb);
        const s16x4 hi = tr_read_at(dbase[c][1] + 6144 * kb);
        return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      };
      auto load_b = [&](int step) -> u32x4 {  // step = kb * 9 + tap
        const int kb = step / TAPS, t = step % TAPS, kh = t / KS, kw = t % KS;
        const s16x4 lo = tr_read_at(xbase[kw][0] + XROW * (2 * kb + kh));
        const s16x4 hi = tr_read_at(xbase[kw][1] + XROW * (2 * kb + kh));
        return __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      };
#pragma unroll
      for (int c = 0; c < NC; ++c) af[c] = load_a(0, c);
      bf[0] = load_b(0);
      bf[1] = load_b(1);
#pragma unroll
      for (int step = 0; step < 2 * TAPS; ++step) {
        const int kb = step / TAPS, t = step % TAPS;
        if (step + 2 < 2 * TAPS) bf[(step + 2) % 3] = load_b(step + 2);
        if (step == TAPS) {
#pragma unroll
          for (int c = 0; c < NC; ++c) af[c] = load_a(1, c);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[c]), __builtin_bit_cast(bf16x8, bf[step % 3]),
                                                              acc[t][c], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const int delta = stage == NSTAGE - 1 ? -(NSTAGE - 1) * STAGE : STAGE;
    stage = stage == NSTAGE - 1 ? 0 : stage + 1;
#pragma unroll
    for (int c = 0; c < NC; ++c) { dbase[c][0] += delta; dbase[c][1] += delta; }
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
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (nh + c) * 16 + 4 * grp + r, k = k0 + ktile * 16 + i16;
        if (kloc + ktile * 16 + i16 < cs && n < a.npad) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- host launcher
void wgrad_ring_launch(int which, const WgArgs& a, dim3 grid, hipStream_t st) {
  if (which == WG_RING_2WG_NL) hipLaunchKernelGGL((wgrad_bf16_2wg_kernel<8, true>), grid, dim3(256), 0, st, a);
  else if (which == WG_RING_2WG) hipLaunchKernelGGL(wgrad_bf16_2wg_kernel<8>, grid, dim3(256), 0, st, a);
  else if (which == WG_RING_DMA) hipLaunchKernelGGL(wgrad_bf16_dma_kernel, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(wgrad_bf16_dma96_kernel<0>, grid, dim3(768), 0, st, a);
}

#ifdef CONV64_STAMPS
int wgrad_ring_debug_occupancy(int which) {
  int n = -1;
  hipError_t e = hipErrorInvalidValue;
  if (which == WG_RING_DMA) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_bf16_dma_kernel, 256, 0);
  else if (which == WG_RING_2WG) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, wgrad_bf16_2wg_kernel<8>, 256, 0);
  return e == hipSuccess ? n : -1;
}
#endif
