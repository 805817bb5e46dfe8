// Deep-supervision loss: Dice + CE of an auxiliary head's LOW-resolution logits against the FULL-resolution labels, with the
// bilinear upsampling (torch interpolate, align_corners=False, integer scale factor: the arithmetic of resize_bilinear_kernel in
// augment.hip) done in registers.  The full-resolution logits and their gradient never exist in memory.
//
//   u = Uy z Ux^T per (image, class);  forward = what mia_dice_ce_fwd computes on u (same partial layout, same finalize kernel);
//   backward: dz = Uy^T du Ux with du the per-pixel gradient dice_ce_bwd_kernel would write, recomputed from z, labels and coef.
//
// Forward: one block per (image, slab of full-resolution rows); a thread takes two neighbouring pixels per step (one 16-byte label
// load) when the labels are 16-byte aligned, one otherwise.  The four taps per class come from the low-resolution tensor, which is
// 1/4 .. 1/256 of the labels and stays in cache.
// Backward: a GATHER.  Low-resolution pixel i owns the full-resolution rows [(i - 1) f + f/2, (i + 1) f + f/2) (clipped; the clamped
// border rows fall inside that range too), and the same along x: the footprint is separable.  One block per (image, tile of TH x TW
// low-resolution pixels): (1) du of the tile's (TH + 1) f x (TW + 1) f region -- the tile plus half a cell of halo on every side --
// is computed ONCE per pixel into LDS, (2) reduced along x with the column weights, (3) reduced along y with the row weights, and
// written through dz's own strides.  Every sum runs in a fixed order and there is no atomic anywhere: out, sums and dz are
// bit-identical run to run.  Nothing synchronises with the host; every launch goes to the caller's stream.
#include "ds_common.h"

// ---------------------------------------------------------------- forward
// NK: compile-time class bound (k1 == NK for 2, 3, 4; NK = 8 with a run-time k1 otherwise).  VEC: two pixels per 16-byte label load.
template <int NK, bool VEC>
__global__ __launch_bounds__(256) void ds_loss_fwd_kernel(const float* __restrict__ z, const long long* __restrict__ labels, int h, int w,
                                                          int factor, int k1, LossGeom g, int flags, int slabs, float* __restrict__ part,
                                                          float* __restrict__ cepart, int* __restrict__ bad_label) {
  constexpr int PX = VEC ? 2 : 1;
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int H = h * factor, W = w * factor;
  const int per = (H + slabs - 1) / slabs;
  const int y0 = s * per < H ? s * per : H, y1 = y0 + per < H ? y0 + per : H;
  const float scale = 1.f / (float)factor;
  const float* zb = z + b * g.sn;
  const long long* lb = labels + (size_t)b * H * W;
  const int rowu = W / PX, units = (y1 - y0) * rowu;
  float si[NK], sp[NK], st[NK], ce = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) { si[k] = 0.f; sp[k] = 0.f; st[k] = 0.f; }
  bool bad = false;
  for (int u = threadIdx.x; u < units; u += 256) {
    const int r = u / rowu, yy = y0 + r, x = (u - r * rowu) * PX;
    const DsTap ty = ds_tap(yy, scale, h);
    unsigned lo[PX], hi[PX];
    if constexpr (VEC) {
      load_label_pair(lb + (size_t)yy * W + x, lo, hi);
    } else {
      const unsigned long long l = (unsigned long long)lb[(size_t)yy * W + x];
      lo[0] = (unsigned)(l & 0xFFFFFFFFull); hi[0] = (unsigned)(l >> 32);
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const DsTap tx = ds_tap(x + j, scale, w);
      float v[NK];
      ds_interp<NK>(zb, g, w, k1, ty, tx, v);
      const bool ok = hi[j] == 0u && lo[j] < (unsigned)k1;
      bad |= !ok;
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) mx = fmaxf(mx, v[k]);
      float pr[NK], se = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
      const float inv = ok ? 1.f / se : 0.f;  // an out-of-range label drops the pixel (and poisons the loss in finalize)
      const float lse = mx + __logf(se);
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) {
          const float pk = (flags & LF_SOFTMAX) ? pr[k] * inv : (ok ? v[k] : 0.f);
          const float t = (ok && lo[j] == (unsigned)k) ? 1.f : 0.f;
          si[k] += pk * t;
          sp[k] += (flags & LF_SQUARED) ? pk * pk : pk;
          st[k] += t;
          ce += t * (lse - v[k]);
        }
    }
  }
  if (bad) *bad_label = 1;
  auto red = loss_block_sums<3 * NK + 1, 0>();
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) {
      const float v[3] = {si[k], sp[k], st[k]};
      red.put(3 * k, v);
    }
  const float v[1] = {ce};
  red.put(3 * NK, v);
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 3 * k1) part[((size_t)b * slabs + s) * k1 * 3 + t] = red.sum_f(t);
  else if (t == 3 * NK) cepart[(size_t)b * slabs + s] = red.sum_f(t);
}

// ---------------------------------------------------------------- backward
// LDS: du [k1][RH][pitch] (pitch = RW + 1, odd: a column walk of phase 2 touches every bank once), then tx [k1][tw][RH].
template <int NK>
__global__ __launch_bounds__(256) void ds_loss_bwd_kernel(const float* __restrict__ z, const long long* __restrict__ labels,
                                                          const float* __restrict__ coef, const float* __restrict__ gout,
                                                          float* __restrict__ dz, int nb, int h, int w, int factor, int k1, LossGeom g,
                                                          LossGeom go, int flags, float dice_w, float ce_w, int th, int tw, int tiles_x,
                                                          int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) float ds_smem[];
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int ia = tyi * th, ja = txi * tw;
  const int nth = ia + th < h ? th : h - ia, ntw = ja + tw < w ? tw : w - ja;  // live tile
  const int H = h * factor, W = w * factor;
  const int Y0 = ia * factor - factor / 2, X0 = ja * factor - factor / 2;    // region origin (may lie half a cell outside)
  const int RH = (th + 1) * factor, pitch = (tw + 1) * factor + 1;             // allocated
  const int rh = (nth + 1) * factor, rw = (ntw + 1) * factor;                  // live region
  float* du = ds_smem;
  float* tx_s = ds_smem + (size_t)k1 * RH * pitch;
  const float scale = 1.f / (float)factor;
  const float go_s = gout ? gout[0] : 1.f;
  const float cew = ce_w / (float)((double)nb * (double)H * (double)W);
  float al[NK], be[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    al[k] = k < k1 ? coef[((size_t)b * k1 + k) * 2] : 0.f;
    be[k] = k < k1 ? coef[((size_t)b * k1 + k) * 2 + 1] : 0.f;
  }
  const float* zb = z + b * g.sn;
  const long long* lb = labels + (size_t)b * H * W;

  // (1) du of every full-resolution pixel of the region, once
  for (int idx = threadIdx.x; idx < rh * rw; idx += 256) {
    const int ry = idx / rw, rx = idx - ry * rw;
    const int Y = Y0 + ry, X = X0 + rx;
    float o[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) o[k] = 0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
      const DsTap ty = ds_tap(Y, scale, h), tx = ds_tap(X, scale, w);
      float v[NK], pr[NK];
      ds_interp<NK>(zb, g, w, k1, ty, tx, v);
      float mx = -INFINITY, se = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) mx = fmaxf(mx, v[k]);
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
      const float inv = 1.f / se;
      const long long lab = lb[(size_t)Y * W + X];
      // a bad label leaves t = 0 everywhere; coef is NaN after such a forward, so the pixel is poisoned like every other one
      float gk[NK], dot = 0.f;
      const float tsum = (lab >= 0 && lab < k1) ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) {
          pr[k] *= inv;
          const float pk = (flags & LF_SOFTMAX) ? pr[k] : v[k];
          const float t = (lab == (long long)k) ? 1.f : 0.f;
          gk[k] = (al[k] * t + be[k] * ((flags & LF_SQUARED) ? 2.f * pk : 1.f)) * dice_w;
          dot += gk[k] * pr[k];
        }
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (k < k1) {
          const float t = (lab == (long long)k) ? 1.f : 0.f;
          const float dd = (flags & LF_SOFTMAX) ? pr[k] * (gk[k] - dot) : gk[k];
          o[k] = go_s * (dd + cew * (tsum * pr[k] - t));
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) du[((size_t)k * RH + ry) * pitch + rx] = o[k];
  }
  __syncthreads();

  // (2) along x: tx[k][tj][ry] = sum over the 2 f columns of low-resolution column ja + tj, left to right
  for (int item = threadIdx.x; item < k1 * ntw * rh; item += 256) {
    const int ry = item % rh, rest = item / rh, tj = rest % ntw, k = rest / ntw;
    const float* row = du + ((size_t)k * RH + ry) * pitch + tj * factor;
    float acc = 0.f;
    for (int m = 0; m < 2 * factor; ++m) {
      const int X = X0 + tj * factor + m;
      if (X >= 0 && X < W) acc += ds_weight(ds_tap(X, scale, w), ja + tj) * row[m];
    }
    tx_s[((size_t)k * tw + tj) * RH + ry] = acc;
  }
  __syncthreads();

  // (3) along y, top to bottom, and out through dz's strides
  for (int item = threadIdx.x; item < k1 * nth * ntw; item += 256) {
    const int tj = item % ntw, rest = item / ntw, ti = rest % nth, k = rest / nth;
    const float* col = tx_s + ((size_t)k * tw + tj) * RH + ti * factor;
    float acc = 0.f;
    for (int m = 0; m < 2 * factor; ++m) {
      const int Y = Y0 + ti * factor + m;
      if (Y >= 0 && Y < H) acc += ds_weight(ds_tap(Y, scale, h), ia + ti) * col[m];
    }
    dz[b * go.sn + ((int64_t)(ia + ti) * w + (ja + tj)) * go.sp + k * go.sk] = acc;
  }
}

static bool ds_shape_ok(int nb, int h, int w, int factor, int k1) {
  if (nb <= 0 || h <= 0 || w <= 0 || k1 < 1 || k1 > LOSS_MAXK) return false;
  if (factor != 2 && factor != 4 && factor != 8 && factor != 16) return false;
  return (int64_t)h * factor * w * factor < ((int64_t)1 << 31);
}

// ================================================================ C ABI
extern "C" int mia_ds_loss_workspace(int nb, int k1, int slabs) {
  if (nb <= 0 || k1 <= 0 || slabs <= 0) return 0;
  return nb * slabs * (k1 * 3 + 1);
}

extern "C" int mia_ds_loss_fwd(const float* z, const long long* labels, int nb, int h, int w, int factor, int k1, int64_t sn, int64_t sk,
                               int64_t sp, int flags, float smooth, float dice_w, float ce_w, int slabs, float* workspace, float* sums,
                               float* coef, float* out, int* bad_label, void* stream) {
  MIA_CHECK_ARG(z && labels && workspace && sums && coef && out && bad_label, "mia_ds_loss_fwd: null pointer");
  MIA_CHECK_ARG(ds_shape_ok(nb, h, w, factor, k1), "mia_ds_loss_fwd: nb=%d h=%d w=%d factor=%d k1=%d (factor 2, 4, 8 or 16, k1 in [1,%d])",
                nb, h, w, factor, k1, LOSS_MAXK);
  MIA_CHECK_ARG(slabs > 0 && (int64_t)nb * slabs < ((int64_t)1 << 31), "mia_ds_loss_fwd: bad slab count");
  MIA_CHECK_ARG(!(flags & LF_DENSE), "mia_ds_loss_fwd: a dense target is not supported (index labels only)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  float* part = workspace;
  float* cepart = workspace + (size_t)nb * slabs * k1 * 3;
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  // W = w * factor is even and every image holds a multiple of four labels: an aligned base keeps every pair aligned
  const bool vec = (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
#define DS_FWD(NK)                                                                                                                       \
  if (vec) hipLaunchKernelGGL((ds_loss_fwd_kernel<NK, true>), grid, blk, 0, st, z, labels, h, w, factor, k1, g, flags, slabs, part, cepart, \
                              bad_label);                                                                                                \
  else hipLaunchKernelGGL((ds_loss_fwd_kernel<NK, false>), grid, blk, 0, st, z, labels, h, w, factor, k1, g, flags, slabs, part, cepart,   \
                          bad_label)
  if (k1 == 2) { DS_FWD(2); } else if (k1 == 3) { DS_FWD(3); } else if (k1 == 4) { DS_FWD(4); } else { DS_FWD(LOSS_MAXK); }
#undef DS_FWD
  MIA_LAUNCH_CHECK();
  return mia_dice_ce_finalize_launch(part, cepart, nb, slabs, k1, (int64_t)h * factor * w * factor, flags, smooth, dice_w, ce_w, sums, coef,
                                     out, bad_label, st);
}

extern "C" int mia_ds_loss_bwd(const float* z, const long long* labels, const float* coef, const float* grad_out, float* dz, int nb, int h,
                               int w, int factor, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp,
                               int flags, float dice_w, float ce_w, void* stream) {
  MIA_CHECK_ARG(z && labels && coef && dz, "mia_ds_loss_bwd: null pointer");
  MIA_CHECK_ARG(ds_shape_ok(nb, h, w, factor, k1), "mia_ds_loss_bwd: nb=%d h=%d w=%d factor=%d k1=%d (factor 2, 4, 8 or 16, k1 in [1,%d])",
                nb, h, w, factor, k1, LOSS_MAXK);
  MIA_CHECK_ARG(!(flags & LF_DENSE), "mia_ds_loss_bwd: a dense target is not supported (index labels only)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  int th, tw;
  ds_bwd_tile(factor, k1, &th, &tw);
  const int tiles_y = ceil_div(h, th), tiles_x = ceil_div(w, tw);
  MIA_CHECK_ARG((int64_t)nb * tiles_y * tiles_x < ((int64_t)1 << 31), "mia_ds_loss_bwd: too many tiles");
  const dim3 grid((unsigned)(nb * tiles_y * tiles_x)), blk(256);
  const size_t lds = ds_bwd_lds(factor, k1, th, tw);
#define DS_BWD(NK)                                                                                                                      \
  hipLaunchKernelGGL(ds_loss_bwd_kernel<NK>, grid, blk, lds, st, z, labels, coef, grad_out, dz, nb, h, w, factor, k1, g, go, flags, dice_w, \
                     ce_w, th, tw, tiles_x, tiles_y)
  if (k1 == 2) { DS_BWD(2); } else if (k1 == 3) { DS_BWD(3); } else if (k1 == 4) { DS_BWD(4); } else { DS_BWD(LOSS_MAXK); }
#undef DS_BWD
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
