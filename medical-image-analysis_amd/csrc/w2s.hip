// Weak-to-strong consistency on the GPU (gfx950): the confident arg-max labels of a WEAK view supervise the same network on a strongly
// augmented, CutMix-ed view (FixMatch: Sohn et al., NeurIPS 2020; UniMatch: Yang et al., CVPR 2023; CutMix-CPS: Chen et al., CVPR
// 2021).  The reference has no such code; the definition is losses/weak_strong.py.
//
// Labels: weak logits zw [nb][k1][hw] fp32 by (sn, sk, sp), per pixel
//   y = argmax_k zw_k            on the fp32 logits themselves, a tie goes to the LOWEST index (cs_argmax)
//   keep = [max_k softmax(zw)_k >= tau]      tau = dyn[1] read on the device; dyn NULL: tau = 0 (a NaN keeps nothing)
//   code [nb][hw] = y | keep << 7, one byte per pixel;  kept = sum keep as int64
//
// CutMix of a batch with itself: out[n][c][p] = mask[n or 0][p] != 0 ? x[src(n)][c][p] : x[n][c][p], src(n) = perm[n] when
// (unsigned)perm[n] < nb, else n.  A SELECTION as mia_bcp_mix: the 32 bits of the chosen operand pass through; the partner image is
// read only by the threads that have a mask byte set.  A perm entry outside the batch never becomes an address: the image is mixed
// with itself and bad_perm[1] is raised (the flags have the layout of bad_label -- [0] working, [1] sticky; with no finalize kernel
// to fold [0] into [1] the kernels here raise [1] themselves, and nothing re-arms it but the host's check).
//
// Loss: strong logits zs [nb][k1][hw] fp32 by (sn, sk, sp), the code map above, mask / perm as for the mix (both NULL: no mix).  For
// pixel (n, p): c = code[mask[n][p] ? src(n) : n][p], y = c & 7, kept = c >> 7.  The hard-label Dice + CE core (hard_loss.h) with ONE
// region, the kept pixels of the WHOLE call:
//   wd = w dice_w,  wc = w ce_w,  w = dyn[0] (dyn NULL: 1),  cden = nb * hw: always every pixel (cps.hip); no kept pixel: CE = D = 0
//   L = w (ce_w CE + dice_w D)
//   out = {L, CE, D, w};  counts = {kept pixels of the mixed view, pixels whose mask byte is set (0 without a mix)}
//   coef [2 k1 + 1]: what the backward reads; a pixel that is not kept gets exactly 0.0f
//   w2s_labels_kernel     block (image, slab of pixels): one streaming pass over zw; soft-max in double per pixel (cs_softmax); writes
//                         `code` (one 4-byte store per four pixels on the wide path) and the block's count
//   w2s_count_kernel      one block: the counts in a fixed order in int64
//   w2s_cutmix_kernel     a thread per four elements (16-byte path) or per element
//   w2s_loss_fwd_kernel   block (image, slab of pixels): ONE streaming pass over zs, the mask byte and the one or two code bytes of a
//                         pixel
//   w2s_finalize_kernel   one block: the partials in a fixed order in double / int64 (loss_totals) -> out, counts, coef
//   w2s_loss_bwd_kernel   one streaming pass, a thread per pixel group: re-reads `code` through mask / perm (so both directions agree
//                         on every pixel), writes dzs by its own strides
// A code byte whose label is not below k1 (a map made for more classes) counts as not kept.  A thread owns the SAME four consecutive
// pixels on the 16-byte path (planar / channels-last logits, hw % 4 == 0, aligned pointers and strides) and on the scalar path, and
// every sum runs in the same order on both, so the two paths give the same bits.  No float atomics: bit-identical from run to run; an
// image's code does not depend on the rest of the batch; nothing synchronises with the host.
#include "hard_loss.h"

// ---------------------------------------------------------------- labels
template <int K1>
__device__ __forceinline__ unsigned w2s_label_pixel(const float (&v)[K1], double tau, int& kept) {
  float mx;
  const int y = cs_argmax<K1>(v, mx);
  double p[K1];
  cs_softmax<K1>(v, p);
  const bool keep = cs_max<K1>(p) >= tau;  // a NaN keeps nothing
  kept += keep;
  return (unsigned)y | (unsigned)keep << 7;
}

// block (image, slab of `per` pixels; per % PX == 0); wsn [nb * slabs] = the block's count of kept pixels
template <int K1, int MODE>
__global__ __launch_bounds__(256) void w2s_labels_kernel(const float* __restrict__ z, const float* __restrict__ dyn, int64_t hw,
                                                         LossGeom g, int slabs, int64_t per, int* __restrict__ wsn,
                                                         unsigned char* __restrict__ code) {
  constexpr int PX = CS_PX(MODE);
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* img = z + b * g.sn;
  const double tau = dyn ? (double)dyn[1] : 0.0;
  int kept = 0;
  for (int64_t p = r0 + (int64_t)threadIdx.x * PX; p < r1; p += 256 * PX) {
    float v[PX][K1];
    cs_load<K1, MODE>(img, p, g, v);
    unsigned bits = w2s_label_pixel<K1>(v[0], tau, kept);
    if constexpr (PX == 4) {  // written out: every index into v is a constant before any loop is unrolled (cps.hip)
      bits |= w2s_label_pixel<K1>(v[1], tau, kept) << 8;
      bits |= w2s_label_pixel<K1>(v[2], tau, kept) << 16;
      bits |= w2s_label_pixel<K1>(v[3], tau, kept) << 24;
    }
    unsigned char* cd = code + (int64_t)b * hw + p;
    if (PX == 4)  // one 4-byte store; b * hw + p is a multiple of 4
      *reinterpret_cast<unsigned*>(cd) = bits;
    else
      cd[0] = (unsigned char)bits;
  }
  auto red = loss_block_sums<1, 1>();
  const int c = wave_sum_i(kept);
  if (red.l == 0) red.i[red.w][0] = c;
  __syncthreads();
  if (threadIdx.x == 0) wsn[blockIdx.x] = red.sum_i(0);
}

// one block of 256 threads: kept[0] = the sum of the blocks' counts
__global__ __launch_bounds__(256) void w2s_count_kernel(const int* __restrict__ wsn, int nparts, long long* __restrict__ kept) {
  const LossTotals tot = loss_totals<1, 1>(nullptr, wsn, nparts, 0);
  if (threadIdx.x == 0) kept[0] = tot.n[0];
}

// ---------------------------------------------------------------- CutMix with a permutation of the batch
// the image that `perm` pairs with image n; an entry outside the batch pairs the image with itself
__device__ __forceinline__ int w2s_partner(const int* __restrict__ perm, int n, int nb, bool& ok) {
  const int pn = perm[n];
  ok = (unsigned)pn < (unsigned)nb;
  return ok ? pn : n;
}

// WIDE: a thread owns four consecutive pixels of one (image, channel) plane: one 16-byte load, one 4-byte mask load, a second 16-byte
// load only where a mask byte is set, one 16-byte store
template <bool WIDE>
__global__ __launch_bounds__(256) void w2s_cutmix_kernel(const unsigned* __restrict__ x, const int* __restrict__ perm,
                                                         const unsigned char* __restrict__ mask, unsigned* __restrict__ out, int nb,
                                                         int64_t hw, int64_t chw, int64_t msn, int64_t osn, int64_t total,
                                                         int* __restrict__ bad_perm) {
  constexpr int PX = WIDE ? 4 : 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per = chw / PX, n = idx / per, e = (idx - n * per) * PX, p = e % hw;
  bool ok;
  const int64_t src = w2s_partner(perm, (int)n, nb, ok);
  if (!ok && e == 0) bad_perm[1] = 1;
  const unsigned char* mk = mask + n * msn + p;
  if constexpr (WIDE) {
    u32x4 o = *reinterpret_cast<const u32x4*>(x + n * chw + e);
    const unsigned m = *reinterpret_cast<const unsigned*>(mk);
    if (m) {
      const u32x4 f = *reinterpret_cast<const u32x4*>(x + src * chw + e);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = ((m >> (8 * i)) & 0xffu) ? f[i] : o[i];
    }
    *reinterpret_cast<u32x4*>(out + n * osn + e) = o;
    store_data_pad();
  } else {
    out[n * osn + e] = mk[0] ? x[src * chw + e] : x[n * chw + e];
  }
}

// ---------------------------------------------------------------- loss: what forward and backward share
// The code bytes that supervise the group's four pixels (bytes 0..3 of the result): the partner image's where the pixel's mask byte is
// set, the image's own elsewhere.  The partner's map is read only by a thread that has a mask byte set.
template <bool WIDE>
__device__ __forceinline__ unsigned w2s_codes(const unsigned char* __restrict__ own, const unsigned char* __restrict__ oth, unsigned mb,
                                              int nlive) {
  const unsigned a = px4_bytes<WIDE>(own, nlive);
  if (mb == 0u) return a;
  const unsigned b = px4_bytes<WIDE>(oth, nlive);
  unsigned c = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) c |= ((mb >> (8 * i)) & 0xffu) ? (b & (0xffu << (8 * i))) : (a & (0xffu << (8 * i)));
  return c;
}

// (label, kept) of one code byte for K1 classes
template <int K1>
__device__ __forceinline__ bool w2s_decode(unsigned c, int& y) {
  y = (int)(c & 7u);
  return (c & 0x80u) != 0u && y < K1;
}

// ---------------------------------------------------------------- forward
// block (image, slab of `per` pixels; per % 4 == 0); the workspace is laid out by hl_park, the block's third count is the pixels whose
// mask byte is set
template <int K1, int MODE>
__global__ __launch_bounds__(256) void w2s_loss_fwd_kernel(const float* __restrict__ z, const unsigned char* __restrict__ code,
                                                           const unsigned char* __restrict__ mask, const int* __restrict__ perm,
                                                           int nb, int64_t hw, int64_t msn, LossGeom g, int slabs, int64_t per,
                                                           float* __restrict__ ws, int nparts, int* __restrict__ bad_perm) {
  constexpr bool WIDE = MODE != CS_SCALAR;
  constexpr int NQ = 2 * K1 + 1, NC = K1 + 2;
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* img = z + b * g.sn;
  int src = b;
  if (mask) {  // mask and perm come together
    bool ok;
    src = w2s_partner(perm, b, nb, ok);
    if (!ok && s == 0 && threadIdx.x == 0) bad_perm[1] = 1;
  }
  const unsigned char* mk = mask ? mask + b * msn : nullptr;
  const unsigned char* cown = code + (int64_t)b * hw;
  const unsigned char* coth = code + (int64_t)src * hw;
  HlAcc<K1, 1> acc;
  acc.zero();
  int pasted = 0;
  for (int64_t p = r0 + (int64_t)threadIdx.x * 4; p < r1; p += 256 * 4) {
    const int nlive = r1 - p < 4 ? (int)(r1 - p) : 4;  // 4 on the 16-byte path (hw % 4 == 0)
    float v[4][K1];
    px4_load<K1, MODE>(img, p, nlive, g, v);
    const unsigned mb = mask ? px4_bytes<WIDE>(mk + p, nlive) : 0u;
    const unsigned cd = w2s_codes<WIDE>(cown + p, coth + p, mb, nlive);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pasted += ((mb >> (8 * i)) & 0xffu) != 0u;  // the bytes past nlive are zero
      int y;
      const bool in[1] = {w2s_decode<K1>((cd >> (8 * i)) & 0xffu, y) && i < nlive};
      hl_fwd_pixel<K1, 1>(v[i], y, in, acc);
    }
  }
  const int extra[1] = {pasted};
  hl_park<K1, 1, 1>(acc, extra, ws, nparts);
}

// one block of 256 threads: out[4], counts[2], coef[2 K1 + 1]
template <int K1>
__global__ __launch_bounds__(256) void w2s_finalize_kernel(const float* __restrict__ ws, int nparts, double n_all,
                                                           const float* __restrict__ dyn, float smooth, float ce_w, float dice_w,
                                                           float* __restrict__ out, long long* __restrict__ counts,
                                                           float* __restrict__ coef) {
  constexpr int NQ = 2 * K1 + 1, NC = K1 + 2;
  __shared__ float res[4], cf[NQ];  // results and coefficients are parked here and leave by one 4-byte store per lane
  const int* wn = reinterpret_cast<const int*>(ws + (size_t)nparts * (2 * NQ));
  const LossTotals tot = loss_totals<NQ, NC>(ws, wn, nparts, NQ);
  const int t = threadIdx.x;
  if (t == 0) {
    const float wt = dyn ? dyn[0] : 1.f;
    const double wc = (double)wt * (double)ce_w;
    double d, ce;
    hl_region<K1>(tot.f, tot.n, (double)smooth, (double)wt * (double)dice_w, wc, n_all, d, ce, cf);
    cf[2 * K1] = (float)(wc / n_all);  // the CE denominator never vanishes: this one is written with no kept pixel too
    res[0] = (float)((double)wt * ((double)ce_w * ce + (double)dice_w * d));
    res[1] = (float)ce;
    res[2] = (float)d;
    res[3] = wt;
  }
  __syncthreads();
  if (t < 4) out[t] = res[t];
  else if (t >= 64 && t < 66) counts[t - 64] = tot.n[K1 + (t - 64)];
  else if (t >= 128 && t < 128 + NQ) coef[t - 128] = cf[t - 128];
}

// ---------------------------------------------------------------- backward
// a thread per group of four pixels (`groups` per image); dz has the layout class of z on the 16-byte path
template <int K1, int MODE>
__global__ __launch_bounds__(256) void w2s_loss_bwd_kernel(const float* __restrict__ z, const unsigned char* __restrict__ code,
                                                           const unsigned char* __restrict__ mask, const int* __restrict__ perm,
                                                           const float* __restrict__ coef, const float* __restrict__ gout,
                                                           float* __restrict__ dz, int nb, int64_t hw, int64_t msn, int64_t groups,
                                                           int64_t total, LossGeom g, LossGeom gd) {
  constexpr bool WIDE = MODE != CS_SCALAR;
  constexpr int NQ = 2 * K1 + 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / groups, p = (idx - b * groups) * 4;
  const int nlive = hw - p < 4 ? (int)(hw - p) : 4;
  const double go = (double)(gout ? gout[0] : 1.f);
  float cf[NQ];  // uniform
#pragma unroll
  for (int k = 0; k < NQ; ++k) cf[k] = coef[k];
  int64_t src = b;
  if (mask) {
    bool ok;
    src = w2s_partner(perm, (int)b, nb, ok);  // the forward has raised the verdict
  }
  float v[4][K1], d[4][K1];
  px4_load<K1, MODE>(z + b * g.sn, p, nlive, g, v);
  const unsigned mb = mask ? px4_bytes<WIDE>(mask + b * msn + p, nlive) : 0u;
  const unsigned cd = w2s_codes<WIDE>(code + b * hw + p, code + src * hw + p, mb, nlive);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int y;
    const bool kept = w2s_decode<K1>((cd >> (8 * i)) & 0xffu, y);
    float t[K1];  // not d[i] itself (bcp.hip): handed the row, <4, planar> gets a store-data site at 3 wait states behind a store
    hl_bwd_pixel<K1>(v[i], y, kept, cf, go, t);
#pragma unroll
    for (int k = 0; k < K1; ++k) d[i][k] = t[k];
  }
  float* dst = dz + b * gd.sn;
  if constexpr (WIDE) {
    cs_store<K1, MODE>(dst, p, gd, d);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nlive) {
        float t[1][K1];
#pragma unroll
        for (int k = 0; k < K1; ++k) t[0][k] = d[i][k];
        cs_store<K1, CS_SCALAR>(dst, p + i, gd, t);
      }
  }
}

// ---------------------------------------------------------------- host side
template <int K1, int MODE>
static void w2s_launch_labels(hipStream_t st, const float* z, const float* dyn, int nb, int64_t hw, const LossGeom& g, int slabs,
                              int* wsn, unsigned char* code) {
  constexpr int PX = CS_PX(MODE);
  const int64_t per = ceil_div64(ceil_div64(hw, PX), slabs) * PX;
  hipLaunchKernelGGL((w2s_labels_kernel<K1, MODE>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, z, dyn, hw, g, slabs, per, wsn,
                     code);
}

template <int K1, int MODE>
static void w2s_launch_fwd(hipStream_t st, const float* z, const unsigned char* code, const unsigned char* mask, const int* perm,
                           int nb, int64_t hw, int64_t msn, const LossGeom& g, int slabs, float* ws, int* bad_perm) {
  const int64_t per = ceil_div64(ceil_div64(hw, 4), slabs) * 4;
  hipLaunchKernelGGL((w2s_loss_fwd_kernel<K1, MODE>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, z, code, mask, perm, nb, hw, msn,
                     g, slabs, per, ws, nb * slabs, bad_perm);
}

template <int K1, int MODE>  // MODE unused: the shape CS_DISPATCH1 calls
static void w2s_launch_finalize(hipStream_t st, const float* ws, int nparts, double n_all, const float* dyn, float smooth, float ce_w,
                                float dice_w, float* out, long long* counts, float* coef) {
  hipLaunchKernelGGL(w2s_finalize_kernel<K1>, dim3(1), dim3(256), 0, st, ws, nparts, n_all, dyn, smooth, ce_w, dice_w, out, counts,
                     coef);
}

template <int K1, int MODE>
static void w2s_launch_bwd(hipStream_t st, const float* z, const unsigned char* code, const unsigned char* mask, const int* perm,
                           const float* coef, const float* gout, float* dz, int nb, int64_t hw, int64_t msn, const LossGeom& g,
                           const LossGeom& gd) {
  const int64_t groups = ceil_div64(hw, 4), total = (int64_t)nb * groups;
  hipLaunchKernelGGL((w2s_loss_bwd_kernel<K1, MODE>), dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, z, code, mask, perm,
                     coef, gout, dz, nb, hw, msn, groups, total, g, gd);
}

static size_t w2s_words_per_block(int k1) { return (size_t)(2 * k1 + 1) * 2 + k1 + 2; }

extern "C" int mia_w2s_labels(const float* logits, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                              int slabs, int* workspace, unsigned char* code, long long* kept, void* stream) {
  MIA_CHECK_ARG(logits && workspace && code && kept, "mia_w2s_labels: null pointer");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_w2s_labels: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0 && hw <= 0x7fffffff && (int64_t)nb * hw <= 0x7fffffff &&
                    (int64_t)nb * slabs <= 0x7fffffff,
                "mia_w2s_labels: bad shape nb=%d hw=%lld slabs=%d", nb, (long long)hw, slabs);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0, "mia_w2s_labels: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  const int sm = px4_mode(logits, g, k1, hw, code, nullptr);  // four pixels per thread: one 4-byte word of the map
  CS_DISPATCH1(w2s_launch_labels, st, logits, dyn_dev, nb, hw, g, slabs, workspace, code);
  hipLaunchKernelGGL(w2s_count_kernel, dim3(1), dim3(256), 0, st, workspace, nb * slabs, kept);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_cutmix_perm(const float* x, const int* perm, const unsigned char* mask, float* out, int nb, int c, int64_t hw,
                               int64_t mask_sn, int64_t out_sn, int* bad_perm, void* stream) {
  MIA_CHECK_ARG(x && perm && mask && out && bad_perm, "mia_cutmix_perm: null pointer");
  const unsigned* xi = reinterpret_cast<const unsigned*>(x);
  unsigned* o = reinterpret_cast<unsigned*>(out);
  return px4_mix_launch("mia_cutmix_perm", x, x, mask, out, nb, c, hw, mask_sn, out_sn,
                        [&](bool wide, dim3 grid, int64_t chw, int64_t total) -> int {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), x1 = x0 + 4 * (uintptr_t)((int64_t)nb * chw);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + 4 * (uintptr_t)((int64_t)(nb - 1) * out_sn + chw);
    MIA_CHECK_ARG(o1 <= x0 || x1 <= o0, "mia_cutmix_perm: out overlaps x (an image is read after its partner may have been written)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(w2s_cutmix_kernel<true>, grid, dim3(256), 0, st, xi, perm, mask, o, nb, hw, chw, mask_sn, out_sn, total, bad_perm);
    else hipLaunchKernelGGL(w2s_cutmix_kernel<false>, grid, dim3(256), 0, st, xi, perm, mask, o, nb, hw, chw, mask_sn, out_sn, total, bad_perm);
    return MIA_OK;
  });
}

extern "C" int mia_w2s_loss_workspace(int nb, int k1, int slabs) {
  if (nb <= 0 || slabs <= 0 || k1 < 1 || k1 > LOSS_MAXK || (int64_t)nb * slabs * (int64_t)w2s_words_per_block(k1) > 0x7fffffff) return -1;
  return (int)((size_t)nb * slabs * w2s_words_per_block(k1));
}

extern "C" int mia_w2s_loss_fwd(const float* logits, const unsigned char* code, const unsigned char* mask, const int* perm,
                                const float* dyn_dev, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t mask_sn,
                                float smooth, float ce_weight, float dice_weight, int slabs, float* workspace, float* coef, float* out,
                                long long* counts, int* bad_perm, void* stream) {
  MIA_CHECK_ARG(logits && code && workspace && coef && out && counts && bad_perm, "mia_w2s_loss_fwd: null pointer");
  const LossGeom g{sn, sk, sp};
  if (const int e = hl_check("mia_w2s_loss_fwd", nb, hw, k1, slabs, w2s_words_per_block(k1), g, nullptr, mask_sn)) return e;
  if (!mask || !perm) mask = nullptr, perm = nullptr;  // no mix: plain FixMatch
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int sm = px4_mode(logits, g, k1, hw, code, mask);
  CS_DISPATCH1(w2s_launch_fwd, st, logits, code, mask, perm, nb, hw, mask_sn, g, slabs, workspace, bad_perm);
  CS_DISPATCH1(w2s_launch_finalize, st, workspace, nb * slabs, (double)nb * (double)hw, dyn_dev, smooth, ce_weight, dice_weight, out,
               counts, coef);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_w2s_loss_bwd(const float* logits, const unsigned char* code, const unsigned char* mask, const int* perm,
                                const float* coef, const float* grad_out, float* dlogits, int nb, int64_t hw, int k1, int64_t sn,
                                int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp, int64_t mask_sn, void* stream) {
  MIA_CHECK_ARG(logits && code && coef && dlogits, "mia_w2s_loss_bwd: null pointer");
  const LossGeom g{sn, sk, sp}, gd{gsn, gsk, gsp};
  if (const int e = hl_check("mia_w2s_loss_bwd", nb, hw, k1, 0, 0, g, &gd, mask_sn)) return e;
  if (!mask || !perm) mask = nullptr, perm = nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int sm = px4_mode(logits, g, k1, hw, code, mask);
  if (cs_mode(dlogits, gd, k1) != sm) sm = CS_SCALAR;  // the gradient in the layout class of its logits, or one pixel at a time
  CS_DISPATCH1(w2s_launch_bwd, st, logits, code, mask, perm, coef, grad_out, dlogits, nb, hw, mask_sn, g, gd);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
