// Weight gradients, register-staged tile kernels (every mode, bf16 and fp32): the generic kernels with per-element predicates and
// the branch-free "fast" kernels on raw buffer loads.  See conv_wgrad.hip for the GEMM and wgrad_common.h for the shared pieces.
#include "wgrad_common.h"

// ---------------------------------------------------------------- bf16, generic
template <int MODE>
__global__ __launch_bounds__(256) void wgrad_bf16_kernel(const WgArgs a) {
  using G = WGeo<MODE>;
  constexpr int KS = G::KS, S = G::S, PAD = G::PAD, TAPS = G::TAPS;
  constexpr int TH = (S == 1) ? 8 : 4;
  constexpr int XH = (TH - 1) * S + KS, XW = 15 * S + KS;
  constexpr int XROWS = ((XH * XW + 7) / 8) * 8;
  constexpr int X_BYTES = XROWS * 128, D_BYTES = TH * 16 * 128;
  __shared__ __attribute__((aligned(16))) unsigned char smem[X_BYTES + D_BYTES];
  unsigned char* xs = smem;
  unsigned char* ds = smem + X_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const int nkb = a.kpad / 64;
  const int kblk = blockIdx.x % nkb, nblk = blockIdx.x / nkb;
  const int n0 = nblk * 64, k0 = kblk * 64;
  const int kin = a.c1 + a.c2;
  const bf16_t* x1 = static_cast<const bf16_t*>(a.x1);
  const bf16_t* x2 = static_cast<const bf16_t*>(a.x2);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wave_active = (k0 + wave * 16) < kin;

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  for (int tile = blockIdx.y; tile < ntiles; tile += a.ksplit) {
    int tt = tile;
    const int tx = tt % a.tiles_x; tt /= a.tiles_x;
    const int ty = tt % a.tiles_y; tt /= a.tiles_y;
    const int img = tt;
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
    __syncthreads();  // previous tile's reads done
    for (int u = tid; u < XH * XW * 8; u += 256) {
      const int ch = u & 7, pix = u >> 3;
      const int iy = pix / XW, ix = pix - iy * XW;
      const int gy = iy0 + iy, gx = ix0 + ix, c = k0 + ch * 8;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < a.Hx && gx >= 0 && gx < a.Wx && c < kin) {
        const size_t p = ((size_t)img * a.Hx + gy) * a.Wx + gx;
        if (a.vec_x) {
          const bf16_t* src = (c < a.c1) ? x1 + p * a.c1 + c : x2 + p * a.c2 + (c - a.c1);
          v = *reinterpret_cast<const u32x4*>(src);
        } else {
          alignas(16) bf16_t tmp[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ce = c + e;
            tmp[e] = ce < a.c1 ? x1[p * a.c1 + ce] : (ce < kin ? x2[p * a.c2 + (ce - a.c1)] : (bf16_t)0);
          }
          v = *reinterpret_cast<const u32x4*>(tmp);
        }
      }
      *reinterpret_cast<u32x4*>(xs + swz_off(pix, ch)) = v;
    }
    for (int u = tid; u < TH * 16 * 8; u += 256) {
      const int ch = u & 7, pix = u >> 3;
      const int y = pix >> 4, xx = pix & 15;
      const int gy = oy0 + y, gx = ox0 + xx, c = n0 + ch * 8;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (gy < a.Hy && gx < a.Wy && c < a.cdy) {
        const size_t p = ((size_t)img * a.Hy + gy) * a.Wy + gx;
        if (a.vec_dy) {
          v = *reinterpret_cast<const u32x4*>(dy + p * a.cdy + c);
        } else {
          alignas(16) bf16_t tmp[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) tmp[e] = (c + e < a.cdy) ? dy[p * a.cdy + c + e] : (bf16_t)0;
          v = *reinterpret_cast<const u32x4*>(tmp);
        }
      }
      *reinterpret_cast<u32x4*>(ds + swz_off(pix, ch)) = v;
    }
    __syncthreads();
    if (wave_active) {
#pragma unroll
      for (int kb = 0; kb < TH / 2; ++kb) {
        // lane group `grp` covers k = 8*grp .. 8*grp+7 of this 32-pixel block; two 4-row tr reads each
        const int yy = 2 * kb + (grp >> 1), xb = 8 * (grp & 1) + qp;
        u32x4 af[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int ch = 2 * c + (pp >> 1);
          const int r0 = yy * 16 + xb;
          const s16x4 lo = tr_read(ds, swz_off(r0, ch) + 8 * (pp & 1));
          const s16x4 hi = tr_read(ds, swz_off(r0 + 4, ch) + 8 * (pp & 1));
          af[c] = __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int kh = 0; kh < KS; ++kh) {
#pragma unroll
          for (int kw = 0; kw < KS; ++kw) {
            const int ch = 2 * wave + (pp >> 1);
            const int r0 = (yy * S + kh) * XW + xb * S + kw;
            const s16x4 lo = tr_read(xs, swz_off(r0, ch) + 8 * (pp & 1));
            const s16x4 hi = tr_read(xs, swz_off(r0 + 4 * S, ch) + 8 * (pp & 1));
            const bf16x8 b = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int c = 0; c < 4; ++c)
              acc[kh * KS + kw][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[c]), b,
                                                                               acc[kh * KS + kw][c], 0, 0, 0);
          }
        }
      }
    }
  }
  // slab[z][tap][n][k]: C rows = n (A side), cols = k (B side)
  float* slab = a.slabs + (size_t)blockIdx.y * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + c * 16 + 4 * grp + r, k = k0 + wave * 16 + i16;
        slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- bf16 fast path
// Same tiling / LDS image / MFMA schedule as wgrad_bf16_kernel, but (a) the NEXT pixel tile is fetched
// global -> VGPR while the current tile's MFMAs run (the generic kernel idles the matrix pipe for the
// whole staging phase: rocprofv3 SQ_WAIT_ANY = 63 % of wave cycles), and (b) every access is a raw
// buffer load against a per-image descriptor, so borders are out-of-range offsets -> zeros, no branches.
// Contract: channel counts multiples of the 16-byte unit, a two-source input split on a 64-channel boundary,
// 16-byte aligned, per-image tensors < 2 GiB (channel tails are zero-filled like the image border).

// W8 (round 5): 512 threads -- eight waves = 4 input-channel tiles x 2 halves of the block's output channels, 72 accumulator registers per
// wave.  The 256-thread form compiles to 436-464 registers (accumulators parked in AGPRs): ONE wave per SIMD, staging and MFMAs never
// overlapping (0.37 PFLOP/s on cfg5's 96 -> 192 stride-2 and 192 -> 96 transposed gradients, the only launches that still use it).
template <int MODE, int TH, bool W8 = false>
__global__ __launch_bounds__(W8 ? 512 : 256) void wgrad_bf16_fast_kernel(const WgArgs a) {
  using G = WGeo<MODE>;
  constexpr int KS = G::KS, S = G::S, PAD = G::PAD, TAPS = G::TAPS;
  constexpr int XH = (TH - 1) * S + KS, XW = 15 * S + KS;
  constexpr int PPI = W8 ? 64 : 32;  // pixels x 8 chunks per staging iteration
  constexpr int X_IT = (XH * XW + PPI - 1) / PPI, D_IT = (TH * 16 + PPI - 1) / PPI;
  constexpr int X_BYTES = X_IT * PPI * 128, D_BYTES = D_IT * PPI * 128;
  constexpr int NC = W8 ? 2 : 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[X_BYTES + D_BYTES];
  unsigned char* xs = smem;
  unsigned char* ds = smem + X_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, i16 = lane & 15, qp = i16 >> 2, pp = i16 & 3;
  const int ch8 = tid & 7, p8 = tid >> 3;
  const int kq = W8 ? (wave & 3) : wave, nh = W8 ? 2 * (wave >> 2) : 0;  // input-channel tile; first output-channel tile of this wave
  const WgCols<64> cols(a);
  int bx = blockIdx.x, by = blockIdx.y;
  if (a.opt & 16) { cols.xcd_order(a, bx, by); if (by >= a.ksplit) return; }
  const WgBlock blk = cols.block(a, bx);
  const int cs = blk.cs, kloc = blk.kloc, n0 = blk.n0, k0 = blk.k0;
  const bf16_t* xsrc = static_cast<const bf16_t*>(blk.xsrc);
  const bf16_t* dy = static_cast<const bf16_t*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  // tile-invariant unit geometry
  int x_iy[X_IT], x_ix[X_IT];
#pragma unroll
  for (int i = 0; i < X_IT; ++i) {
    const int pix = p8 + PPI * i;
    x_iy[i] = pix < XH * XW ? pix / XW : -100000;
    x_ix[i] = pix - (pix / XW) * XW;
  }
  const int lds_x0 = swz_off(p8, ch8), lds_d0 = swz_off(p8, ch8);  // + 128 PPI per iteration (PPI rows)

  f32x4 acc[TAPS][NC];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 px[X_IT], pd[D_IT];
  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  auto fetch = [&](int tile) {
    int tt = tile;
    const int tx = tt % a.tiles_x; tt /= a.tiles_x;
    const int ty = tt % a.tiles_y; tt /= a.tiles_y;
    const int img = tt;
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
    const rsrc_t rx = make_rsrc(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 2));
    const rsrc_t rd = make_rsrc(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 2));
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      const int gy = iy0 + x_iy[i], gx = ix0 + x_ix[i];
      const bool ok = gy >= 0 && gy < a.Hx && gx >= 0 && gx < a.Wx;
      const unsigned voff = (ok && kloc + ch8 * 8 < cs) ? (unsigned)(((gy * a.Wx + gx) * cs + kloc + ch8 * 8) * 2) : SENT;
      px[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)voff, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < D_IT; ++i) {
      const int pix = p8 + PPI * i;
      const int gy = oy0 + (pix >> 4), gx = ox0 + (pix & 15);
      const bool ok = pix < TH * 16 && gy < a.Hy && gx < a.Wy;
      const unsigned voff = (ok && n0 + ch8 * 8 < a.cdy) ? (unsigned)(((gy * a.Wy + gx) * a.cdy + n0 + ch8 * 8) * 2) : SENT;
      pd[i] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)voff, 0, 0);
    }
  };

  int tile = by;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += a.ksplit) {
    __syncthreads();  // previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < X_IT; ++i) *reinterpret_cast<u32x4*>(xs + lds_x0 + 128 * PPI * i) = px[i];
#pragma unroll
    for (int i = 0; i < D_IT; ++i) *reinterpret_cast<u32x4*>(ds + lds_d0 + 128 * PPI * i) = pd[i];
    __syncthreads();
    if (tile + a.ksplit < ntiles) fetch(tile + a.ksplit);
#pragma unroll(TH <= 8 ? TH / 2 : 2)
    for (int kb = 0; kb < TH / 2; ++kb) {
      const int yy = 2 * kb + (grp >> 1), xb = 8 * (grp & 1) + qp;
      u32x4 af[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int ch = 2 * (nh + c) + (pp >> 1);
        const int r0 = yy * 16 + xb;
        const s16x4 lo = tr_read(ds, swz_off(r0, ch) + 8 * (pp & 1));
        const s16x4 hi = tr_read(ds, swz_off(r0 + 4, ch) + 8 * (pp & 1));
        af[c] = __builtin_bit_cast(u32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      }
#pragma unroll
      for (int kh = 0; kh < KS; ++kh) {
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const int ch = 2 * kq + (pp >> 1);
          const int r0 = (yy * S + kh) * XW + xb * S + kw;
          const s16x4 lo = tr_read(xs, swz_off(r0, ch) + 8 * (pp & 1));
          const s16x4 hi = tr_read(xs, swz_off(r0 + 4 * S, ch) + 8 * (pp & 1));
          const bf16x8 b = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
          for (int c = 0; c < NC; ++c)
            acc[kh * KS + kw][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[c]), b,
                                                                             acc[kh * KS + kw][c], 0, 0, 0);
        }
      }
    }
  }
  float* slab = a.slabs + (size_t)by * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (nh + c) * 16 + 4 * grp + r, k = k0 + kq * 16 + i16;
        if (kloc + kq * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- fp32
template <int MODE>
__global__ __launch_bounds__(256) void wgrad_f32_kernel(const WgArgs a) {
  using G = WGeo<MODE>;
  constexpr int KS = G::KS, S = G::S, PAD = G::PAD, TAPS = G::TAPS;
  constexpr int TH = (S == 1) ? 4 : 2;
  constexpr int XH = (TH - 1) * S + KS, XW = 15 * S + KS;
  constexpr int PS = 80;  // LDS pixel stride in dwords (64 channels + 16 pad)
  __shared__ __attribute__((aligned(16))) float smem[(XH * XW + TH * 16) * PS];
  float* xs = smem;
  float* ds = smem + XH * XW * PS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, i16 = lane & 15;
  const int nkb = a.kpad / 64;
  const int kblk = blockIdx.x % nkb, nblk = blockIdx.x / nkb;
  const int n0 = nblk * 64, k0 = kblk * 64;
  const int kin = a.c1 + a.c2;
  const float* x1 = static_cast<const float*>(a.x1);
  const float* x2 = static_cast<const float*>(a.x2);
  const float* dy = static_cast<const float*>(a.dy);

  f32x4 acc[TAPS][4];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool wave_active = (k0 + wave * 16) < kin;

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  for (int tile = blockIdx.y; tile < ntiles; tile += a.ksplit) {
    int tt = tile;
    const int tx = tt % a.tiles_x; tt /= a.tiles_x;
    const int ty = tt % a.tiles_y; tt /= a.tiles_y;
    const int img = tt;
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
    __syncthreads();
    for (int u = tid; u < XH * XW * 16; u += 256) {
      const int ch = u & 15, pix = u >> 4;
      const int iy = pix / XW, ix = pix - iy * XW;
      const int gy = iy0 + iy, gx = ix0 + ix, c = k0 + ch * 4;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < a.Hx && gx >= 0 && gx < a.Wx && c < kin) {
        const size_t p = ((size_t)img * a.Hx + gy) * a.Wx + gx;
        if (a.vec_x) {
          const float* src = (c < a.c1) ? x1 + p * a.c1 + c : x2 + p * a.c2 + (c - a.c1);
          v = *reinterpret_cast<const f32x4*>(src);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int ce = c + e;
            v[e] = ce < a.c1 ? x1[p * a.c1 + ce] : (ce < kin ? x2[p * a.c2 + (ce - a.c1)] : 0.f);
          }
        }
      }
      *reinterpret_cast<f32x4*>(xs + pix * PS + ch * 4) = v;
    }
    for (int u = tid; u < TH * 16 * 16; u += 256) {
      const int ch = u & 15, pix = u >> 4;
      const int y = pix >> 4, xx = pix & 15;
      const int gy = oy0 + y, gx = ox0 + xx, c = n0 + ch * 4;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (gy < a.Hy && gx < a.Wy && c < a.cdy) {
        const size_t p = ((size_t)img * a.Hy + gy) * a.Wy + gx;
        if (a.vec_dy) {
          v = *reinterpret_cast<const f32x4*>(dy + p * a.cdy + c);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (c + e < a.cdy) ? dy[p * a.cdy + c + e] : 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(ds + pix * PS + ch * 4) = v;
    }
    __syncthreads();
    if (wave_active) {
      for (int y = 0; y < TH; ++y) {
#pragma unroll
        for (int xq = 0; xq < 4; ++xq) {
          const int xx = xq * 4 + q;  // this lane's pixel (k index) within the row
          float af[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) af[c] = ds[(y * 16 + xx) * PS + c * 16 + i16];
#pragma unroll
          for (int kh = 0; kh < KS; ++kh)
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
              const float b = xs[((y * S + kh) * XW + xx * S + kw) * PS + wave * 16 + i16];
#pragma unroll
              for (int c = 0; c < 4; ++c)
                acc[kh * KS + kw][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c], b, acc[kh * KS + kw][c], 0, 0, 0);
            }
        }
      }
    }
  }
  float* slab = a.slabs + (size_t)blockIdx.y * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + c * 16 + 4 * q + r, k = k0 + wave * 16 + i16;
        slab[((size_t)t * a.npad + n) * a.kpad + k] = acc[t][c][r];
      }
}

// ---------------------------------------------------------------- fp32 fast path (same contract as the bf16 one)
// NARROW (32-channel layers: cdy <= 32 and every source <= 32 channels, e.g. al_train's first level): the 64 x 64 block would
// multiply 75 % zeros (1.22 ms vs 0.41 ms for the forward conv of the same layer).  The four waves become 2 input-channel tiles x 2
// halves of the tile's pixel rows with 2 output-channel tiles each; the two pixel halves are summed through LDS at the end.
// SPLIT (option f32_split): the products run on the f16 matrix cores from two-part split operands (SplitF16, common.h), each operand
// tensor scaled by the power of two its maximum dictates (a block's input channels lie in ONE source, so x1 and x2 keep their own scale).
// LDS holds one (h | l << 16) word per element in the exact kernel's layout; the reduction dimension of an MFMA is 16 pixels
// (one tile row) x 2 parts: lane group q takes pixels q, q + 4, q + 8, q + 12 (the exact kernel's conflict-free bank pattern),
// the dy fragment is expanded to its (H, H) and (L, L) forms once per row and meets every tap's (h, l) x fragment in two MFMAs; the
// accumulators are scaled back when the slab is written.
// Full blocks (round 5): 512 threads -- eight waves = 4 input-channel tiles x 2 halves of the block's output channels, 72 accumulator
// registers per wave instead of 144.  The 256-thread form needed 364 registers (hipcc parks accumulators in AGPRs), i.e. ONE wave per
// SIMD and one workgroup per CU: staging and MFMA phases never overlapped (PMC: 45 % matrix-pipe busy); forced to 256 registers it spilled.
template <int MODE, bool NARROW = false, bool SPLIT = false>
__global__ __launch_bounds__(NARROW ? 256 : 512, 2) void wgrad_f32_fast_kernel(const WgArgs a) {
  using G = WGeo<MODE>;
  constexpr int KS = G::KS, S = G::S, PAD = G::PAD, TAPS = G::TAPS;
  // N8 (narrow stride-1 3x3, round 5: al_train's 32-channel first level): 8-row tiles -- twice the MFMAs per barrier pair, a 10-row halo tile for
  // 8 rows instead of 6 for 4 -- on a 48-dword pixel stride (32 channels + 16 pad: the same conflict-free bank pattern as 80) and staging
  // lanes dealt 32 pixels x 8 units, so no lane idles on the 32 channels that do not exist.  61 KB of LDS: still two workgroups per CU.
  constexpr bool N8 = NARROW && MODE == MODE_W3S1;
  constexpr int TH = N8 ? 8 : ((S == 1) ? 4 : 2);
  constexpr int XH = (TH - 1) * S + KS, XW = 15 * S + KS;
  constexpr int PS = N8 ? 48 : 80;  // LDS pixel stride in dwords (64 channels + 16 pad): conflict-free b32 fragment reads
  constexpr int NTHR = NARROW ? 256 : 512;
  constexpr int UL = N8 ? 8 : 16, PPI = NTHR / UL;  // four-channel units staged per pixel; pixels per staging iteration
  constexpr int X_IT = (XH * XW + PPI - 1) / PPI, D_IT = TH * 16 / PPI;
  __shared__ __attribute__((aligned(16))) float smem[(X_IT * PPI + TH * 16) * PS];
  float* xs = smem;
  float* ds = smem + X_IT * PPI * PS;

  constexpr int NC = 2;  // output-channel tiles per wave
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = NARROW ? (wave & 1) : (wave & 3), ph = NARROW ? (wave >> 1) : 0;  // input-channel tile; half of the tile's pixel rows
  const int nh = NARROW ? 0 : 2 * (wave >> 2);  // first output-channel tile of this wave (full blocks: waves 4 .. 7 take tiles 2, 3)
  const int q = lane >> 4, i16 = lane & 15;
  const int ch4 = tid % UL, p16 = tid / UL;
  // 64-channel input blocks are cut per SOURCE (ceil(c1/64) + ceil(c2/64) of them), so a block never straddles the
  // two tensors of a concatenated input whatever c1 is; a source's last block may be partial (lanes beyond cs read
  // zeros and do not store)
  const int kb1 = (a.c1 + 63) / 64, nkb = kb1 + (a.c2 + 63) / 64;
  const int kblk = blockIdx.x % nkb, nblk = blockIdx.x / nkb;
  const bool second = kblk >= kb1;
  const int cs = second ? a.c2 : a.c1, kloc = (second ? kblk - kb1 : kblk) * 64;
  const int n0 = nblk * 64, k0 = (second ? a.c1 : 0) + kloc;
  const float* xsrc = static_cast<const float*>(second ? a.x2 : a.x1);
  const float* dy = static_cast<const float*>(a.dy);
  const size_t xpix = (size_t)a.Hx * a.Wx, ypix = (size_t)a.Hy * a.Wy;

  int x_iy[X_IT], x_ix[X_IT];
#pragma unroll
  for (int i = 0; i < X_IT; ++i) {
    const int pix = p16 + PPI * i;
    x_iy[i] = pix < XH * XW ? pix / XW : -100000;
    x_ix[i] = pix - (pix / XW) * XW;
  }
  f32x4 acc[TAPS][NC];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 px[X_IT], pd[D_IT];
  float sc_x = 1.f, sc_d = 1.f;
  int e_out = 0;
  if constexpr (SPLIT) {
    const int ex = SplitF16::exp_of(*(second ? a.amax_x2 : a.amax_x1) & 0x7FFFFFFFu), ed = SplitF16::exp_of(*a.amax_dy & 0x7FFFFFFFu);
    sc_x = SplitF16::pow2(ex); sc_d = SplitF16::pow2(ed); e_out = -(ex + ed);
  }
  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  auto fetch = [&](int tile) {
    int tt = tile;
    const int tx = tt % a.tiles_x; tt /= a.tiles_x;
    const int ty = tt % a.tiles_y; tt /= a.tiles_y;
    const int img = tt;
    const int oy0 = ty * TH, ox0 = tx * 16;
    const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
    const rsrc_t rx = make_rsrc(xsrc + (size_t)img * xpix * cs, (unsigned)(xpix * cs * 4));
    const rsrc_t rd = make_rsrc(dy + (size_t)img * ypix * a.cdy, (unsigned)(ypix * a.cdy * 4));
#pragma unroll
    for (int i = 0; i < X_IT; ++i) {
      const int gy = iy0 + x_iy[i], gx = ix0 + x_ix[i];
      const bool ok = gy >= 0 && gy < a.Hx && gx >= 0 && gx < a.Wx;
      const unsigned voff = (ok && kloc + ch4 * 4 < cs) ? (unsigned)(((gy * a.Wx + gx) * cs + kloc + ch4 * 4) * 4) : SENT;
      px[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (int)voff, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < D_IT; ++i) {
      const int pix = p16 + PPI * i;
      const int gy = oy0 + (pix >> 4), gx = ox0 + (pix & 15);
      const bool ok = gy < a.Hy && gx < a.Wy;
      const unsigned voff = (ok && n0 + ch4 * 4 < a.cdy) ? (unsigned)(((gy * a.Wy + gx) * a.cdy + n0 + ch4 * 4) * 4) : SENT;
      pd[i] = __builtin_amdgcn_raw_buffer_load_b128(rd, (int)voff, 0, 0);
    }
  };

  int tile = blockIdx.y;
  if (tile < ntiles) fetch(tile);
  for (; tile < ntiles; tile += a.ksplit) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < X_IT; ++i) *reinterpret_cast<u32x4*>(xs + (p16 + PPI * i) * PS + ch4 * 4) = SPLIT ? SplitF16::unit(px[i], sc_x) : px[i];
#pragma unroll
    for (int i = 0; i < D_IT; ++i) *reinterpret_cast<u32x4*>(ds + (p16 + PPI * i) * PS + ch4 * 4) = SPLIT ? SplitF16::unit(pd[i], sc_d) : pd[i];
    __syncthreads();
    if (tile + a.ksplit < ntiles) fetch(tile + a.ksplit);
    constexpr int YR = NARROW ? TH / 2 : TH;
    if constexpr (SPLIT) {
      const unsigned* xw = reinterpret_cast<const unsigned*>(xs);
      const unsigned* dw = reinterpret_cast<const unsigned*>(ds);
#pragma unroll
      for (int yy = 0; yy < YR; ++yy) {
        const int y = ph * YR + yy;
        u32x4 ah[NC], al[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          u32x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = dw[(y * 16 + 4 * j + q) * PS + (nh + c) * 16 + i16];
          ah[c] = w; al[c] = SplitF16::swap_hl(w);  // (H, L) and (L, H) against the (h, l) x fragment: all four products
        }
#pragma unroll
        for (int kh = 0; kh < KS; ++kh)
#pragma unroll
          for (int kw = 0; kw < KS; ++kw) {
            u32x4 b;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = xw[((y * S + kh) * XW + (4 * j + q) * S + kw) * PS + kq * 16 + i16];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[kh * KS + kw][c] = SplitF16::mma_a(ah[c], al[c], b, acc[kh * KS + kw][c]);
          }
      }
      continue;
    }
#pragma unroll
    for (int yy = 0; yy < YR; ++yy) {
      const int y = ph * YR + yy;
#pragma unroll
      for (int xq = 0; xq < 4; ++xq) {
        const int xx = xq * 4 + q;
        float af[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) af[c] = ds[(y * 16 + xx) * PS + (nh + c) * 16 + i16];
#pragma unroll
        for (int kh = 0; kh < KS; ++kh)
#pragma unroll
          for (int kw = 0; kw < KS; ++kw) {
            const float b = xs[((y * S + kh) * XW + xx * S + kw) * PS + kq * 16 + i16];
#pragma unroll
            for (int c = 0; c < NC; ++c)
              acc[kh * KS + kw][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[c], b, acc[kh * KS + kw][c], 0, 0, 0);
          }
      }
    }
  }
  if constexpr (NARROW) {  // the second pixel half hands its partial sums over through LDS
    static_assert(TAPS * NC * 4 * 128 * 4 <= (int)sizeof(smem), "exchange buffer fits the staging LDS");
    __syncthreads();
    float* ex = smem + (kq * 64 + lane) * (TAPS * NC * 4);
    if (ph == 1) {
#pragma unroll
      for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int c = 0; c < NC; ++c) *reinterpret_cast<f32x4*>(ex + (t * NC + c) * 4) = acc[t][c];
    }
    __syncthreads();
    if (ph == 1) return;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const f32x4 o = *reinterpret_cast<const f32x4*>(ex + (t * NC + c) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][c][r] += o[r];
      }
  }
  float* slab = a.slabs + (size_t)blockIdx.y * TAPS * a.npad * a.kpad;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + (nh + c) * 16 + 4 * q + r, k = k0 + kq * 16 + i16;
        if (kloc + kq * 16 + i16 < cs) slab[((size_t)t * a.npad + n) * a.kpad + k] = SPLIT ? SplitF16::unscale(acc[t][c][r], e_out) : acc[t][c][r];
      }
}

// ---------------------------------------------------------------- host launcher
void wgrad_tile_launch(int mode, int dtype, bool fast, bool narrow, bool split, const WgArgs& a, dim3 grid, hipStream_t st) {
  if (fast && dtype == MIA_BF16) {  // stride-2 / transposed shapes only: conv_wgrad_run sends every stride-1 one to wgrad_ring / wgrad_bt
    if (mode == MODE_W3S2) hipLaunchKernelGGL((wgrad_bf16_fast_kernel<MODE_W3S2, 4, true>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((wgrad_bf16_fast_kernel<MODE_W2S2, 4>), grid, dim3(256), 0, st, a);  // (four taps: 172 registers, two waves per SIMD as it is; the 512-thread form measured 10 % slower)
  } else if (fast) {  // fp32; narrow = 32-channel layers (half-width blocks, 256 threads), split = two-part split f16 products
    wgrad_with_mode(mode, [&](auto m) {
      constexpr int M = decltype(m)::value;
      if (narrow && split) hipLaunchKernelGGL((wgrad_f32_fast_kernel<M, true, true>), grid, dim3(256), 0, st, a);
      else if (split) hipLaunchKernelGGL((wgrad_f32_fast_kernel<M, false, true>), grid, dim3(512), 0, st, a);
      else if (narrow) hipLaunchKernelGGL((wgrad_f32_fast_kernel<M, true>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(wgrad_f32_fast_kernel<M>, grid, dim3(512), 0, st, a);
    });
  } else if (dtype == MIA_BF16) {
    wgrad_with_mode(mode, [&](auto m) { hipLaunchKernelGGL(wgrad_bf16_kernel<decltype(m)::value>, grid, dim3(256), 0, st, a); });
  } else {
    wgrad_with_mode(mode, [&](auto m) { hipLaunchKernelGGL(wgrad_f32_kernel<decltype(m)::value>, grid, dim3(256), 0, st, a); });
  }
}
