// Bidirectional copy-paste on the GPU (gfx950): the mix of two image batches under a mask, and the loss of a mixed image whose pixels
// are supervised by one of TWO label maps (BCP: Bai et al., CVPR 2023).  The reference has no such code; the definition is
// losses/copy_paste.py.
//
// Mix: out[n][c][p] = mask[n or 0][p] != 0 ? fg[n][c][p] : bg[n][c][p].  A SELECTION, not fg * m + bg * (1 - m): the 32 bits of the
// chosen operand pass through as they are (NaN payloads and -0.0 included), and the operand not chosen is never looked at.
//
// Loss: logits z [nb][k1][hw] fp32 by (sn, sk, sp), label maps ya, yb [nb][hw] (int64 or uint8), mask byte m per pixel; region A is
// m != 0 and reads ya, region B is m == 0 and reads yb.  The hard-label Dice + CE core (hard_loss.h) with R = 2 regions over ALL images
// and pixels of the call, every class counting, background included:
//   wd_r = wc_r = w_r / 2,  cden_r = N_r + 1e-16            an empty region: D_r = C_r = 0
//   L = wa (D_A + C_A) / 2 + wb (D_B + C_B) / 2
//   out = {L, D_A, C_A, D_B, C_B};  counts = {N_A, N_B};  coef [2][2 k1 + 1]: what the backward reads
//   bcp_loss_fwd_kernel   block (image, slab of pixels): ONE streaming pass over logits, mask byte and the two label maps
//   bcp_finalize_kernel   one block: the partials in a fixed order in double / int64 (loss_totals, once per region) -> out, counts, coef
//   bcp_loss_bwd_kernel   one streaming pass, a thread per pixel group: picks the region's coefficients by the mask byte, writes
//                         dlogits by its own strides
// A pixel reads ONLY its own region's label: the other map may hold anything there.  A selected label outside [0, k1) follows the
// protocol of the other losses (loss_bad_label_verdict): NaN results and the sticky per-device verdict.
// A thread owns the SAME four consecutive pixels on the 16-byte path (planar / channels-last logits, hw % 4 == 0, aligned pointers
// and strides) and on the scalar path, and every sum runs in the same order on both, so the two paths give the same bits.  No float
// atomics: bit-identical from run to run.  Nothing synchronises with the host.
#include "hard_loss.h"

// ---------------------------------------------------------------- mix
// WIDE: a thread owns four consecutive pixels of one (image, channel) plane: two 16-byte loads, one 4-byte mask load, one 16-byte store
template <bool WIDE>
__global__ __launch_bounds__(256) void bcp_mix_kernel(const unsigned* __restrict__ fg, const unsigned* __restrict__ bg,
                                                      const unsigned char* __restrict__ mask, unsigned* __restrict__ out, int64_t hw,
                                                      int64_t chw, int64_t msn, int64_t osn, int64_t total) {
  constexpr int PX = WIDE ? 4 : 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per = chw / PX, n = idx / per, e = (idx - n * per) * PX, p = e % hw;
  const unsigned char* mk = mask + n * msn + p;
  if constexpr (WIDE) {
    const u32x4 f = *reinterpret_cast<const u32x4*>(fg + n * chw + e), b = *reinterpret_cast<const u32x4*>(bg + n * chw + e);
    const unsigned m = *reinterpret_cast<const unsigned*>(mk);
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = ((m >> (8 * i)) & 0xffu) ? f[i] : b[i];
    *reinterpret_cast<u32x4*>(out + n * osn + e) = o;
    store_data_pad();
  } else {
    out[n * osn + e] = mk[0] ? fg[n * chw + e] : bg[n * chw + e];
  }
}

// ---------------------------------------------------------------- loss: what forward and backward share
// class index in [0, K1), -1 = outside
template <int K1>
__device__ __forceinline__ int bcp_class(unsigned lo, unsigned hi) {
  return (hi == 0u && lo < (unsigned)K1) ? (int)lo : -1;
}

// The mask bytes of the group's pixels (px4_bytes) are kept as the bytes themselves: a pixel tests its byte != 0.
// the SELECTED label of each pixel of the group as a class index (-1: outside [0, K1), and every pixel past nlive)
template <int K1, bool WIDE>
__device__ __forceinline__ void bcp_labels(const long long* __restrict__ la, const long long* __restrict__ lb, unsigned mbytes,
                                           int nlive, int (&y)[4]) {
  if (WIDE) {
    unsigned alo[4], ahi[4], blo[4], bhi[4];
    load_label_quad(la, alo, ahi);
    load_label_quad(lb, blo, bhi);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool m = ((mbytes >> (8 * i)) & 0xffu) != 0u;
      y[i] = bcp_class<K1>(m ? alo[i] : blo[i], m ? ahi[i] : bhi[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i] = -1;
      if (i < nlive) {
        const unsigned long long v = (unsigned long long)((((mbytes >> (8 * i)) & 0xffu) != 0u) ? la[i] : lb[i]);
        y[i] = bcp_class<K1>((unsigned)(v & 0xFFFFFFFFull), (unsigned)(v >> 32));
      }
    }
  }
}
template <int K1, bool WIDE>
__device__ __forceinline__ void bcp_labels(const unsigned char* __restrict__ la, const unsigned char* __restrict__ lb, unsigned mbytes,
                                           int nlive, int (&y)[4]) {
  if (WIDE) {
    const unsigned wa = *reinterpret_cast<const unsigned*>(la), wb = *reinterpret_cast<const unsigned*>(lb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool m = ((mbytes >> (8 * i)) & 0xffu) != 0u;
      y[i] = bcp_class<K1>(((m ? wa : wb) >> (8 * i)) & 0xffu, 0u);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      y[i] = -1;
      if (i < nlive) y[i] = bcp_class<K1>((((mbytes >> (8 * i)) & 0xffu) != 0u) ? la[i] : lb[i], 0u);
    }
  }
}

// ---------------------------------------------------------------- forward
// block (image, slab of `per` pixels; per % 4 == 0); the workspace is laid out by hl_park
template <int K1, int MODE, typename LT>
__global__ __launch_bounds__(256) void bcp_loss_fwd_kernel(const float* __restrict__ z, const LT* __restrict__ la,
                                                           const LT* __restrict__ lb, const unsigned char* __restrict__ mask,
                                                           int64_t hw, int64_t msn, LossGeom g, int slabs, int64_t per,
                                                           float* __restrict__ ws, int nparts, int* __restrict__ bad_label) {
  constexpr bool WIDE = MODE != CS_SCALAR;
  constexpr int NQ = 2 * K1 + 1, NC = K1 + 1;
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* img = z + b * g.sn;
  const unsigned char* mk = mask + b * msn;
  const LT* ia = la + (int64_t)b * hw;
  const LT* ib = lb + (int64_t)b * hw;
  HlAcc<K1, 2> acc;
  acc.zero();
  bool bad = false;
  for (int64_t p = r0 + (int64_t)threadIdx.x * 4; p < r1; p += 256 * 4) {
    const int nlive = r1 - p < 4 ? (int)(r1 - p) : 4;  // 4 on the 16-byte path (hw % 4 == 0)
    float v[4][K1];
    int y[4];
    px4_load<K1, MODE>(img, p, nlive, g, v);
    const unsigned mb = px4_bytes<WIDE>(mk + p, nlive);
    bcp_labels<K1, WIDE>(ia + p, ib + p, mb, nlive, y);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool live = i < nlive, m = ((mb >> (8 * i)) & 0xffu) != 0u;
      bad |= live && y[i] < 0;
      const bool in[2] = {live && m, live && !m};
      hl_fwd_pixel<K1, 2>(v[i], y[i], in, acc);
    }
  }
  if (bad) *bad_label = 1;
  hl_park<K1, 2, 0>(acc, nullptr, ws, nparts);
}

// one block of 256 threads: out[5], counts[2], coef[2][2 K1 + 1]
template <int K1>
__global__ __launch_bounds__(256) void bcp_finalize_kernel(const float* __restrict__ ws, int nparts, float smooth, float wa, float wb,
                                                           float* __restrict__ out, long long* __restrict__ counts,
                                                           float* __restrict__ coef, int* __restrict__ bad_label) {
  constexpr int NQ = 2 * K1 + 1, NC = K1 + 1;
  __shared__ double tf[2][NQ], term[2][2];
  __shared__ long long tn[2][NC];
  __shared__ float res[5], cf[2 * NQ];  // results and coefficients are parked here and leave by one 4-byte store per lane
  const int* wn = reinterpret_cast<const int*>(ws + (size_t)2 * nparts * (2 * NQ));
  const int t = threadIdx.x;
  for (int r = 0; r < 2; ++r) {  // the same LDS serves both regions: the totals are copied out before the second pass
    const LossTotals tot = loss_totals<NQ, NC>(ws + (size_t)r * nparts * (2 * NQ), wn + (size_t)r * nparts * NC, nparts, NQ);
    if (t < NQ) tf[r][t] = tot.f[t];
    else if (t >= 64 && t < 64 + NC) tn[r][t - 64] = tot.n[t - 64];
    __syncthreads();
  }
  if (t < 2) {  // one thread per region
    const double hw_ = 0.5 * (double)(t ? wb : wa);
    hl_region<K1>(tf[t], tn[t], (double)smooth, hw_, hw_, (double)tn[t][K1] + 1e-16, term[t][0], term[t][1], cf + t * NQ);
  }
  __syncthreads();
  if (t == 0) {
    res[0] = (float)((double)wa * (term[0][0] + term[0][1]) * 0.5 + (double)wb * (term[1][0] + term[1][1]) * 0.5);
    res[1] = (float)term[0][0];
    res[2] = (float)term[0][1];
    res[3] = (float)term[1][0];
    res[4] = (float)term[1][1];
  }
  __syncthreads();
  if (t < 5) out[t] = res[t];
  else if (t >= 64 && t < 66) counts[t - 64] = tn[t - 64][K1];
  else if (t >= 128 && t < 128 + 2 * NQ) coef[t - 128] = cf[t - 128];
  const int bad = bad_label[0];  // read before the verdict re-arms it: out[3], out[4] lie past the three values it overwrites
  loss_bad_label_verdict(bad_label, out, coef, 2 * NQ);
  if (bad && t >= 3 && t < 5) out[t] = __builtin_nanf("");
}

// ---------------------------------------------------------------- backward
// a thread per group of four pixels (`groups` per image); dz has the layout class of z on the 16-byte path
template <int K1, int MODE, typename LT>
__global__ __launch_bounds__(256) void bcp_loss_bwd_kernel(const float* __restrict__ z, const LT* __restrict__ la,
                                                           const LT* __restrict__ lb, const unsigned char* __restrict__ mask,
                                                           const float* __restrict__ coef, const float* __restrict__ gout,
                                                           float* __restrict__ dz, int64_t hw, int64_t msn, int64_t groups,
                                                           int64_t total, LossGeom g, LossGeom gd) {
  constexpr bool WIDE = MODE != CS_SCALAR;
  constexpr int NQ = 2 * K1 + 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / groups, p = (idx - b * groups) * 4;
  const int nlive = hw - p < 4 ? (int)(hw - p) : 4;
  const double go = (double)(gout ? gout[0] : 1.f);
  float ca[NQ], cb[NQ];  // uniform: the two regions' coefficients
#pragma unroll
  for (int k = 0; k < NQ; ++k) { ca[k] = coef[k]; cb[k] = coef[NQ + k]; }
  float v[4][K1], d[4][K1];
  int y[4];
  px4_load<K1, MODE>(z + b * g.sn, p, nlive, g, v);
  const unsigned mb = px4_bytes<WIDE>(mask + b * msn + p, nlive);
  bcp_labels<K1, WIDE>(la + b * hw + p, lb + b * hw + p, mb, nlive, y);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool m = ((mb >> (8 * i)) & 0xffu) != 0u;
    float cf[NQ];  // the pixel's region
#pragma unroll
    for (int k = 0; k < NQ; ++k) cf[k] = m ? ca[k] : cb[k];
    float t[K1];  // not d[i] itself: handed the row, the channels-last instantiations keep up to 24 more registers (occupancy 6 -> 4)
    hl_bwd_pixel<K1>(v[i], y[i], true, cf, go, t);
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
static void bcp_launch_fwd(hipStream_t st, const float* z, const void* la, const void* lb, bool u8, const unsigned char* mask, int nb,
                           int64_t hw, int64_t msn, const LossGeom& g, int slabs, float* ws, int* bad_label) {
  const int64_t per = ceil_div64(ceil_div64(hw, 4), slabs) * 4;
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  if (u8)
    hipLaunchKernelGGL((bcp_loss_fwd_kernel<K1, MODE, unsigned char>), grid, blk, 0, st, z, static_cast<const unsigned char*>(la),
                       static_cast<const unsigned char*>(lb), mask, hw, msn, g, slabs, per, ws, nb * slabs, bad_label);
  else
    hipLaunchKernelGGL((bcp_loss_fwd_kernel<K1, MODE, long long>), grid, blk, 0, st, z, static_cast<const long long*>(la),
                       static_cast<const long long*>(lb), mask, hw, msn, g, slabs, per, ws, nb * slabs, bad_label);
}

template <int K1, int MODE>
static void bcp_launch_bwd(hipStream_t st, const float* z, const void* la, const void* lb, bool u8, const unsigned char* mask,
                           const float* coef, const float* gout, float* dz, int nb, int64_t hw, int64_t msn, const LossGeom& g,
                           const LossGeom& gd) {
  const int64_t groups = ceil_div64(hw, 4), total = (int64_t)nb * groups;
  const dim3 grid((unsigned)ceil_div64(total, 256)), blk(256);
  if (u8)
    hipLaunchKernelGGL((bcp_loss_bwd_kernel<K1, MODE, unsigned char>), grid, blk, 0, st, z, static_cast<const unsigned char*>(la),
                       static_cast<const unsigned char*>(lb), mask, coef, gout, dz, hw, msn, groups, total, g, gd);
  else
    hipLaunchKernelGGL((bcp_loss_bwd_kernel<K1, MODE, long long>), grid, blk, 0, st, z, static_cast<const long long*>(la),
                       static_cast<const long long*>(lb), mask, coef, gout, dz, hw, msn, groups, total, g, gd);
}

template <int K1, int MODE>  // MODE unused: the shape CS_DISPATCH1 calls
static void bcp_launch_finalize(hipStream_t st, const float* ws, int nparts, float smooth, float wa, float wb, float* out,
                                long long* counts, float* coef, int* bad_label) {
  hipLaunchKernelGGL(bcp_finalize_kernel<K1>, dim3(1), dim3(256), 0, st, ws, nparts, smooth, wa, wb, out, counts, coef, bad_label);
}

// the 16-byte path: px4_mode with the mask, and four labels per unit (16-byte units of int64 or 4-byte words of uint8)
static int bcp_mode(const float* z, const LossGeom& g, int k1, int64_t hw, const void* la, const void* lb, bool u8,
                    const unsigned char* mask) {
  if (u8 ? !(cs_al4(la) && cs_al4(lb)) : !(cs_al16(la) && cs_al16(lb))) return CS_SCALAR;
  return px4_mode(z, g, k1, hw, mask, nullptr);
}

static size_t bcp_words_per_block(int k1) { return (size_t)2 * ((2 * k1 + 1) * 2 + k1 + 1); }

extern "C" int mia_bcp_mix(const float* fg, const float* bg, const unsigned char* mask, float* out, int nb, int c, int64_t hw,
                           int64_t mask_sn, int64_t out_sn, void* stream) {
  MIA_CHECK_ARG(fg && bg && mask && out, "mia_bcp_mix: null pointer");
  const unsigned* f = reinterpret_cast<const unsigned*>(fg);
  const unsigned* b = reinterpret_cast<const unsigned*>(bg);
  unsigned* o = reinterpret_cast<unsigned*>(out);
  return px4_mix_launch("mia_bcp_mix", fg, bg, mask, out, nb, c, hw, mask_sn, out_sn,
                        [&](bool wide, dim3 grid, int64_t chw, int64_t total) -> int {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (wide) hipLaunchKernelGGL(bcp_mix_kernel<true>, grid, dim3(256), 0, st, f, b, mask, o, hw, chw, mask_sn, out_sn, total);
    else hipLaunchKernelGGL(bcp_mix_kernel<false>, grid, dim3(256), 0, st, f, b, mask, o, hw, chw, mask_sn, out_sn, total);
    return MIA_OK;
  });
}

extern "C" int mia_bcp_loss_workspace(int nb, int k1, int slabs) {
  if (nb <= 0 || slabs <= 0 || k1 < 1 || k1 > LOSS_MAXK || (int64_t)nb * slabs * (int64_t)bcp_words_per_block(k1) > 0x7fffffff) return -1;
  return (int)((size_t)nb * slabs * bcp_words_per_block(k1));
}

extern "C" int mia_bcp_loss_fwd(const float* logits, const void* label_a, const void* label_b, const unsigned char* mask, int nb,
                                int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t mask_sn, int labels_u8, float smooth,
                                float weight_a, float weight_b, int slabs, float* workspace, float* coef, float* out,
                                long long* counts, int* bad_label, void* stream) {
  MIA_CHECK_ARG(logits && label_a && label_b && mask && workspace && coef && out && counts && bad_label,
                "mia_bcp_loss_fwd: null pointer");
  const LossGeom g{sn, sk, sp};
  if (const int e = hl_check("mia_bcp_loss_fwd", nb, hw, k1, slabs, bcp_words_per_block(k1), g, nullptr, mask_sn)) return e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool u8 = labels_u8 != 0;
  const int sm = bcp_mode(logits, g, k1, hw, label_a, label_b, u8, mask);
  CS_DISPATCH1(bcp_launch_fwd, st, logits, label_a, label_b, u8, mask, nb, hw, mask_sn, g, slabs, workspace, bad_label);
  CS_DISPATCH1(bcp_launch_finalize, st, workspace, nb * slabs, smooth, weight_a, weight_b, out, counts, coef, bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_bcp_loss_bwd(const float* logits, const void* label_a, const void* label_b, const unsigned char* mask,
                                const float* coef, const float* grad_out, float* dlogits, int nb, int64_t hw, int k1, int64_t sn,
                                int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp, int64_t mask_sn, int labels_u8,
                                void* stream) {
  MIA_CHECK_ARG(logits && label_a && label_b && mask && coef && dlogits, "mia_bcp_loss_bwd: null pointer");
  const LossGeom g{sn, sk, sp}, gd{gsn, gsk, gsp};
  if (const int e = hl_check("mia_bcp_loss_bwd", nb, hw, k1, 0, 0, g, &gd, mask_sn)) return e;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool u8 = labels_u8 != 0;
  int sm = bcp_mode(logits, g, k1, hw, label_a, label_b, u8, mask);
  if (cs_mode(dlogits, gd, k1) != sm) sm = CS_SCALAR;  // the gradient in the layout class of its logits, or one pixel at a time
  CS_DISPATCH1(bcp_launch_bwd, st, logits, label_a, label_b, u8, mask, coef, grad_out, dlogits, nb, hw, mask_sn, g, gd);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
