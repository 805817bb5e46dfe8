// Losses of the fold trainers (reference src/losses/: DC_and_CE_loss over MemoryEfficientSoftDiceLoss + RobustCrossEntropyLoss with
// class weights / ignore label, TopKLoss, and the hard tp/fp/fn of get_tp_fp_fn_tn on the arg-max prediction).
//
//   valid = (label != ignore_label);  p = softmax(logits) (or the logits themselves);  t = onehot(label) where valid
//   I[b,k] = sum valid p_k t_k     P[b,k] = sum valid p_k     G[b,k] = #{valid, label = k}
//   CEnum  = sum valid w[label] (logsumexp - logit[label])     CEden = sum valid w[label]
//   a = argmax_k logits (lowest index on a tie):  tp = #{valid, a = k, label = k}, fp = #{valid, a = k, label != k}, fn = #{valid, a != k, label = k}
//   dc = -mean_k (2I + smooth) / max(G + P + smooth, 1e-8),  ce = CEnum / CEden (0 when nothing is valid),  loss = ce_w ce + dice_w dc
//
// No float atomics anywhere: fp32 partials per block, summed in double in a fixed order by a one-block kernel, so every result is
// bit-identical run to run.  Counts are integers end to end (G is the integer count of labelled pixels, exact at any size).
// Nothing here synchronises with the host or sizes an allocation from device data, and every launch goes to the caller's stream.
// A label that is neither a class nor the ignore label follows the protocol of the fused Dice/CE kernel (loss_bad_label_verdict in
// loss_common.h): the pixel is dropped, a working flag is raised, and the finalize kernel turns it into NaN results plus the sticky
// per-device verdict.
#include "loss_common.h"

#define SL_SOFTMAX 1
#define SL_DO_BG 2
#define SL_BATCH 4
#define SL_LABEL_U8 8
#define SL_IGNORE 16

// class index in [0, k1), -1 = ignored, -2 = neither (bad label)
__device__ __forceinline__ int sl_class64(unsigned lo, unsigned hi, int k1, const LossIgnore& g) {
  if (hi == 0u && lo < (unsigned)k1) return (int)lo;
  return (g.on && lo == g.lo && hi == g.hi) ? -1 : -2;
}
__device__ __forceinline__ int sl_class8(unsigned b, int k1, const LossIgnore& g) {
  if (b < (unsigned)k1) return (int)b;
  return ((int)b == g.byte) ? -1 : -2;
}
__device__ __forceinline__ int sl_class(const long long* labels, int64_t i, int k1, const LossIgnore& g) {
  const unsigned long long v = (unsigned long long)labels[i];
  return sl_class64((unsigned)(v & 0xFFFFFFFFull), (unsigned)(v >> 32), k1, g);
}
__device__ __forceinline__ int sl_class(const unsigned char* labels, int64_t i, int k1, const LossIgnore& g) {
  return sl_class8(labels[i], k1, g);
}

// four consecutive labels of one thread's pixel quad (quad index q of the image whose labels start at `lb`)
template <int K1>
__device__ __forceinline__ void sl_quad_classes(const long long* lb, size_t q, const LossIgnore& g, int (&c)[4]) {
  unsigned lo[4], hi[4];
  load_label_quad(lb + 4 * q, lo, hi);
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = sl_class64(lo[j], hi[j], K1, g);
}
template <int K1>
__device__ __forceinline__ void sl_quad_classes(const unsigned char* lb, size_t q, const LossIgnore& g, int (&c)[4]) {
  const unsigned w = reinterpret_cast<const unsigned*>(lb)[q];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = sl_class8((w >> (8 * j)) & 0xFFu, K1, g);
}

// Per-thread accumulators of the forward pass.  NK is a compile-time bound, k1 <= NK the live count.
template <int NK>
struct SlAcc {
  float si[NK], sp[NK], cen, ced;
  int tp[NK], cl[NK], ca[NK];
  __device__ __forceinline__ void clear() {
    cen = 0.f; ced = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) { si[k] = 0.f; sp[k] = 0.f; tp[k] = 0; cl[k] = 0; ca[k] = 0; }
  }
  // one pixel: logits v[0..k1), class c (or < 0), class weights cw
  __device__ __forceinline__ void pixel(const float (&v)[NK], int k1, int c, bool softmax, const float (&cw)[NK]) {
    float mx = v[0];
    int a = 0;
#pragma unroll
    for (int k = 1; k < NK; ++k)
      if (k < k1 && v[k] > mx) { mx = v[k]; a = k; }  // strict >: the lowest index wins a tie, like torch.argmax
    float pr[NK], se = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
    const bool valid = c >= 0;
    const float inv = 1.f / se;
    const float lse = mx + __logf(se);
    float vc = 0.f, wc = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) {
        const float pk = softmax ? pr[k] * inv : v[k];
        const bool t = c == k;
        si[k] += t ? pk : 0.f;
        sp[k] += valid ? pk : 0.f;
        cl[k] += t ? 1 : 0;
        ca[k] += (valid && a == k) ? 1 : 0;
        tp[k] += (t && a == k) ? 1 : 0;
        vc = t ? v[k] : vc;
        wc = t ? cw[k] : wc;
      }
    cen += valid ? wc * (lse - vc) : 0.f;
    ced += wc;  // 0 unless valid
  }
};

// Block sums of all accumulators behind ONE barrier, written to this block's slice of the workspace: [2 k1] floats (I, P per class), cen, ced, then [3 k1] ints (tp, labelled, predicted).
template <int NK>
__device__ __forceinline__ void sl_block_store(const SlAcc<NK>& acc, int k1, float* __restrict__ slice) {
  auto red = loss_block_sums<2 * NK + 2, 3 * NK>();
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) {
      const float fv[2] = {acc.si[k], acc.sp[k]};
      const int iv[3] = {acc.tp[k], acc.cl[k], acc.ca[k]};
      red.put(2 * k, fv, 3 * k, iv);
    }
  const float ce[2] = {acc.cen, acc.ced};
  red.put(2 * k1, ce);
  __syncthreads();
  const int nf = 2 * k1 + 2, ni = 3 * k1;
  if ((int)threadIdx.x < nf) {
    const int i = threadIdx.x;
    slice[i] = red.sum_f(i);
  } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + ni) {
    const int i = threadIdx.x - 64;
    reinterpret_cast<int*>(slice + nf)[i] = red.sum_i(i);
  }
}

template <int NK>
__device__ __forceinline__ void sl_load_weights(const float* __restrict__ cw_g, int k1, float (&cw)[NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) cw[k] = (k < k1 && cw_g) ? cw_g[k] : 1.f;
}

// ---------------------------------------------------------------- forward, any strides / k1 <= 8 / ragged size
template <typename LT>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                           const float* __restrict__ cw_g, int64_t hw, int k1, LossGeom g, int flags,
                                                           LossIgnore ign, int slabs, float* __restrict__ ws, int* __restrict__ bad_label) {
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t per = (hw + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  float cw[LOSS_MAXK];
  sl_load_weights<LOSS_MAXK>(cw_g, k1, cw);
  SlAcc<LOSS_MAXK> acc;
  acc.clear();
  const float* base = logits + b * g.sn;
  bool bad = false;
  for (int64_t p = r0 + threadIdx.x; p < r1; p += 256) {
    float v[LOSS_MAXK];
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k) v[k] = (k < k1) ? base[p * g.sp + k * g.sk] : 0.f;
    const int c = sl_class(labels, (int64_t)b * hw + p, k1, ign);
    bad |= c == -2;
    acc.pixel(v, k1, c, (flags & SL_SOFTMAX) != 0, cw);
  }
  if (bad) *bad_label = 1;
  sl_block_store<LOSS_MAXK>(acc, k1, ws + (size_t)blockIdx.x * (5 * k1 + 2));
}

// ---------------------------------------------------------------- forward, fast path
// Channels-last logits (class stride 1, pixel stride K1), K1 in {2,3,4}, hw % 4 == 0.  A thread owns FOUR consecutive pixels per
// step: K1 16-byte loads of logits and the four labels in two 16-byte loads (int64) or one 4-byte load (uint8), two steps in flight.
template <int K1, typename LT>
__global__ __launch_bounds__(256) void seg_loss_fwd_fast_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                                const float* __restrict__ cw_g, int hw, int flags, LossIgnore ign,
                                                                int slabs, float* __restrict__ ws, int* __restrict__ bad_label) {
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int quads = hw >> 2;
  const int per = (quads + slabs - 1) / slabs, q0 = s * per, q1 = q0 + per < quads ? q0 + per : quads;
  const f32x4* lg = reinterpret_cast<const f32x4*>(logits + (size_t)b * hw * K1);
  const LT* lb = labels + (size_t)b * hw;
  float cw[K1];
  sl_load_weights<K1>(cw_g, K1, cw);
  SlAcc<K1> acc;
  acc.clear();
  const bool softmax = (flags & SL_SOFTMAX) != 0;
  bool bad = false;
  auto one = [&](const f32x4* f, const int (&c)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[K1];
      quad_unpack<K1>(f, j, v);
      bad |= c[j] == -2;
      acc.pixel(v, K1, c[j], softmax, cw);
    }
  };
  int q = q0 + threadIdx.x;
  for (; q + 256 < q1; q += 512) {
    f32x4 fa[K1], fb[K1];
    int ca[4], cb[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) { fa[k] = lg[(size_t)q * K1 + k]; fb[k] = lg[(size_t)(q + 256) * K1 + k]; }
    sl_quad_classes<K1>(lb, (size_t)q, ign, ca);
    sl_quad_classes<K1>(lb, (size_t)(q + 256), ign, cb);
    one(fa, ca);
    one(fb, cb);
  }
  if (q < q1) {
    f32x4 fa[K1];
    int ca[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) fa[k] = lg[(size_t)q * K1 + k];
    sl_quad_classes<K1>(lb, (size_t)q, ign, ca);
    one(fa, ca);
  }
  if (bad) *bad_label = 1;
  sl_block_store<K1>(acc, K1, ws + (size_t)blockIdx.x * (5 * K1 + 2));
}

// ---------------------------------------------------------------- finalize (one block)
// tot[b][k][3] (double: I, P, G) lives behind the per-block slices in the workspace.
// coef[b][k][2] = dice_w * (d dc / d I[b,k], d dc / d P[b,k]);  coef[nb k1 2] = ce_w / CEden (0 when nothing is valid)
// out[0] = loss, out[1] = ce, out[2] = dc;  counts[b][k][3] = tp, fp, fn (int64)
__global__ void seg_loss_finalize_kernel(const float* __restrict__ ws, double* __restrict__ tot, int nb, int slabs, int k1, int flags,
                                         float smooth, float dice_w, float ce_w, float* __restrict__ coef, float* __restrict__ out,
                                         long long* __restrict__ counts, int* __restrict__ bad_label) {
  __shared__ double dsum[256], nsum[256], wsum[256];
  const int stride = 5 * k1 + 2;
  const int kb = (flags & SL_DO_BG) ? 0 : 1;
  const int nk = k1 - kb;
  const int total = nb * k1;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int b = i / k1, k = i % k1;
    double a0 = 0, a1 = 0;
    long long t = 0, g = 0, h = 0;
    for (int s = 0; s < slabs; ++s) {
      const float* p = ws + ((size_t)b * slabs + s) * stride;
      const int* c = reinterpret_cast<const int*>(p + 2 * k1 + 2);
      a0 += p[2 * k]; a1 += p[2 * k + 1];
      t += c[3 * k]; g += c[3 * k + 1]; h += c[3 * k + 2];
    }
    tot[i * 3] = a0; tot[i * 3 + 1] = a1; tot[i * 3 + 2] = (double)g;
    counts[i * 3] = t; counts[i * 3 + 1] = h - t; counts[i * 3 + 2] = g - t;
  }
  double myn = 0.0, myw = 0.0, mydice = 0.0;
  for (int i = threadIdx.x; i < nb * slabs; i += blockDim.x) { myn += ws[(size_t)i * stride + 2 * k1]; myw += ws[(size_t)i * stride + 2 * k1 + 1]; }
  __syncthreads();
  const double sm = (double)smooth;
  if (flags & SL_BATCH) {
    for (int k = kb + threadIdx.x; k < k1; k += blockDim.x) {
      double I = 0, P = 0, G = 0;
      for (int b = 0; b < nb; ++b) { I += tot[(b * k1 + k) * 3]; P += tot[(b * k1 + k) * 3 + 1]; G += tot[(b * k1 + k) * 3 + 2]; }
      const double num = 2 * I + sm, den = G + P + sm, dc = den < 1e-8 ? 1e-8 : den;
      mydice -= (num / dc) / nk;
      const float al = (float)(dice_w * (-2.0 / dc) / nk), be = (float)(den < 1e-8 ? 0.0 : dice_w * (num / (dc * dc)) / nk);
      for (int b = 0; b < nb; ++b) { coef[(b * k1 + k) * 2] = al; coef[(b * k1 + k) * 2 + 1] = be; }
    }
  } else {
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      if (i % k1 < kb) continue;
      const double cnt = (double)nb * nk;
      const double num = 2 * tot[i * 3] + sm, den = tot[i * 3 + 2] + tot[i * 3 + 1] + sm, dc = den < 1e-8 ? 1e-8 : den;
      mydice -= (num / dc) / cnt;
      coef[i * 2] = (float)(dice_w * (-2.0 / dc) / cnt);
      coef[i * 2 + 1] = (float)(den < 1e-8 ? 0.0 : dice_w * (num / (dc * dc)) / cnt);
    }
  }
  if (!(flags & SL_DO_BG))
    for (int b = threadIdx.x; b < nb; b += blockDim.x) { coef[(b * k1) * 2] = 0.f; coef[(b * k1) * 2 + 1] = 0.f; }
  dsum[threadIdx.x] = mydice; nsum[threadIdx.x] = myn; wsum[threadIdx.x] = myw;
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0, n = 0, w = 0;
    for (int i = 0; i < (int)blockDim.x; ++i) { d += dsum[i]; n += nsum[i]; w += wsum[i]; }
    // nothing valid (or all valid weights zero ... torch divides 0/0 there; an all-ignored batch is the case that matters): the CE
    // term is dropped on the device, where the reference tests `num_fg > 0` on the host
    const bool any = w != 0.0;
    const double c = any ? n / w : 0.0;
    out[1] = (float)c; out[2] = (float)d;
    out[0] = (float)((double)ce_w * c + (double)dice_w * d);
    coef[total * 2] = any ? (float)((double)ce_w / w) : 0.f;
  }
  loss_bad_label_verdict(bad_label, out, coef, total * 2 + 1);
}

// ---------------------------------------------------------------- backward
// d loss / d logit_k of a valid pixel = go * ( cecoef w[label] (softmax_k - t_k) + dice part ), dice part = p_k (g_k - sum_j g_j p_j) with
// g_k = al_k t_k + be_k when the Dice runs on the soft-max, g_k itself when it runs on the logits.  Ignored pixels get exactly 0.
template <int NK>
__device__ __forceinline__ void sl_pixel_bwd(const float (&v)[NK], int k1, int c, bool softmax, const float (&cw)[NK],
                                             const float (&al)[NK], const float (&be)[NK], float cecoef, float (&o)[NK]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < NK; ++k)
    if (k < k1) mx = fmaxf(mx, v[k]);
  float pr[NK], gk[NK], se = 0.f, dot = 0.f, wc = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
  const float inv = 1.f / se;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) {
      pr[k] *= inv;
      gk[k] = (c == k ? al[k] : 0.f) + be[k];
      dot += gk[k] * pr[k];
      wc = (c == k) ? cw[k] : wc;
    }
  const float cs = cecoef * wc;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) {
      const float dd = softmax ? pr[k] * (gk[k] - dot) : gk[k];
      o[k] = c >= 0 ? dd + cs * (pr[k] - (c == k ? 1.f : 0.f)) : 0.f;
    }
}

template <typename LT>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                           const float* __restrict__ cw_g, const float* __restrict__ coef,
                                                           const float* __restrict__ gout, float* __restrict__ dl, int nb, int64_t hw,
                                                           int k1, LossGeom g, LossGeom go, int flags, LossIgnore ign) {
  const int64_t total = (int64_t)nb * hw;
  const float go_s = gout ? gout[0] : 1.f;
  const float cecoef = go_s * coef[(size_t)nb * k1 * 2];
  float cw[LOSS_MAXK];
  sl_load_weights<LOSS_MAXK>(cw_g, k1, cw);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    const int64_t p = i - (int64_t)b * hw;
    const float* src = logits + b * g.sn + p * g.sp;
    float v[LOSS_MAXK], al[LOSS_MAXK], be[LOSS_MAXK], o[LOSS_MAXK];
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k) {
      v[k] = (k < k1) ? src[k * g.sk] : 0.f;
      al[k] = (k < k1) ? go_s * coef[((size_t)b * k1 + k) * 2] : 0.f;
      be[k] = (k < k1) ? go_s * coef[((size_t)b * k1 + k) * 2 + 1] : 0.f;
    }
    const int c = sl_class(labels, i, k1, ign);
    sl_pixel_bwd<LOSS_MAXK>(v, k1, c, (flags & SL_SOFTMAX) != 0, cw, al, be, cecoef, o);
    float* dst = dl + b * go.sn + p * go.sp;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) dst[k * go.sk] = o[k];
  }
}

template <int K1, typename LT>
__global__ __launch_bounds__(256) void seg_loss_bwd_fast_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                                const float* __restrict__ cw_g, const float* __restrict__ coef,
                                                                const float* __restrict__ gout, float* __restrict__ dl, int nb, int hw,
                                                                int flags, LossIgnore ign) {
  const int b = blockIdx.y;
  const int quads = hw >> 2;
  const float go_s = gout ? gout[0] : 1.f;
  const float cecoef = go_s * coef[(size_t)nb * K1 * 2];
  const bool softmax = (flags & SL_SOFTMAX) != 0;
  float cw[K1], al[K1], be[K1];
  sl_load_weights<K1>(cw_g, K1, cw);
#pragma unroll
  for (int k = 0; k < K1; ++k) { al[k] = go_s * coef[((size_t)b * K1 + k) * 2]; be[k] = go_s * coef[((size_t)b * K1 + k) * 2 + 1]; }
  const f32x4* lg = reinterpret_cast<const f32x4*>(logits + (size_t)b * hw * K1);
  const LT* lb = labels + (size_t)b * hw;
  f32x4* dst = reinterpret_cast<f32x4*>(dl + (size_t)b * hw * K1);
  for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
    f32x4 f[K1], o[K1];
    int c[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) f[k] = lg[(size_t)q * K1 + k];
    sl_quad_classes<K1>(lb, (size_t)q, ign, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[K1], r[K1];
#pragma unroll
      for (int k = 0; k < K1; ++k) v[k] = f[(j * K1 + k) >> 2][(j * K1 + k) & 3];
      sl_pixel_bwd<K1>(v, K1, c[j], softmax, cw, al, be, cecoef, r);
#pragma unroll
      for (int k = 0; k < K1; ++k) o[(j * K1 + k) >> 2][(j * K1 + k) & 3] = r[k];
    }
#pragma unroll
    for (int k = 0; k < K1; ++k) dst[(size_t)q * K1 + k] = o[k];
    store_data_pad();
  }
}

static bool sl_fast_ok(const void* logits, const void* labels, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int flags) {
  const uintptr_t lab_align = (flags & SL_LABEL_U8) ? 3 : 15;
  return k1 >= 2 && k1 <= 4 && sk == 1 && sp == k1 && sn == hw * k1 && (hw & 3) == 0 && hw < ((int64_t)1 << 30) &&
         (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(labels) & lab_align) == 0;
}

static size_t sl_slices_words(int nb, int k1, int slabs) {
  const size_t w = (size_t)nb * slabs * (5 * k1 + 2);
  return (w + 1) & ~(size_t)1;  // the doubles behind the slices stay 8-byte aligned
}

// ---------------------------------------------------------------- top-k cross-entropy
// nll[i] = valid w[label] (logsumexp - logit[label]) per pixel (>= 0, so the unsigned bit pattern orders the values); tau = the n-th
// largest, found by a radix select over the bit patterns, most significant byte first: a histogram pass over the values that share
// the prefix chosen so far (LDS integer atomics per block, integer global atomics to merge), then a one-block scan that picks the
// byte.  Integer adds commute, so the histograms -- and everything derived from them -- are the same on every run.
// state: [0] prefix (the chosen high bytes of tau), [1] rank still wanted inside the chosen bin, [2] size of the last chosen bin
#define TK_SUM_BLOCKS 256
#define TK_HIST_WORDS (4 * 256)

__device__ __forceinline__ float tk_pixel_nll(const float (&v)[LOSS_MAXK], int k1, int c, const float (&cw)[LOSS_MAXK]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < LOSS_MAXK; ++k)
    if (k < k1) mx = fmaxf(mx, v[k]);
  float se = 0.f, vc = 0.f, wc = 0.f;
#pragma unroll
  for (int k = 0; k < LOSS_MAXK; ++k)
    if (k < k1) { se += expf(v[k] - mx); vc = (c == k) ? v[k] : vc; wc = (c == k) ? cw[k] : wc; }
  const float r = wc * ((mx + logf(se)) - vc);
  return c >= 0 ? (r < 0.f ? 0.f : r) : 0.f;  // a negative zero would order above every positive value
}

template <typename LT>
__global__ __launch_bounds__(256) void topk_nll_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                       const float* __restrict__ cw_g, int nb, int64_t hw, int k1, LossGeom g,
                                                       LossIgnore ign, unsigned n_top, float* __restrict__ nll,
                                                       unsigned* __restrict__ hist, unsigned* __restrict__ state,
                                                       int* __restrict__ bad_label) {
  if (blockIdx.x == 0) {  // the select's scratch is reset here: later kernels on the stream are the only readers
    for (int i = threadIdx.x; i < TK_HIST_WORDS; i += 256) hist[i] = 0u;
    if (threadIdx.x == 0) { state[0] = 0u; state[1] = n_top; state[2] = 0u; }
  }
  const int64_t total = (int64_t)nb * hw;
  float cw[LOSS_MAXK];
  sl_load_weights<LOSS_MAXK>(cw_g, k1, cw);
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    const int64_t p = i - (int64_t)b * hw;
    const float* src = logits + b * g.sn + p * g.sp;
    float v[LOSS_MAXK];
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k) v[k] = (k < k1) ? src[k * g.sk] : 0.f;
    const int c = sl_class(labels, i, k1, ign);
    bad |= c == -2;
    nll[i] = tk_pixel_nll(v, k1, c, cw);
  }
  if (bad) *bad_label = 1;
}

__global__ __launch_bounds__(256) void topk_hist_kernel(const float* __restrict__ nll, int64_t total, int pass,
                                                        const unsigned* __restrict__ state, unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned prefix = state[0];
  const int shift = 24 - 8 * pass;
  const unsigned* bits = reinterpret_cast<const unsigned*>(nll);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const unsigned u = bits[i];
    // pass 0 looks at every value; later passes at those whose higher bytes equal the prefix (64-bit shift: 32 - 8 pass can be 32)
    if ((unsigned)(((unsigned long long)(u ^ prefix)) >> (shift + 8)) == 0u) atomicAdd(&h[(u >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  const unsigned c = h[threadIdx.x];
  if (c) atomicAdd(&hist[pass * 256 + threadIdx.x], c);
}

__global__ __launch_bounds__(256) void topk_scan_kernel(int pass, const unsigned* __restrict__ hist, unsigned* __restrict__ state) {
  __shared__ unsigned s[256];
  const int t = threadIdx.x;
  const unsigned c = hist[pass * 256 + t];
  s[t] = c;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive suffix sums: s[t] = number of values in bins >= t
    const unsigned add = (t + o < 256) ? s[t + o] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const unsigned r = state[1], prefix = state[0];
  const unsigned above = s[t] - c;
  __syncthreads();
  if (r > 0u && s[t] >= r && above < r) {  // exactly one bin holds the r-th largest
    state[0] = prefix | ((unsigned)t << (24 - 8 * pass));
    state[1] = r - above;
    state[2] = c;
  }
}

__global__ __launch_bounds__(256) void topk_sum_kernel(const float* __restrict__ nll, int64_t total, const unsigned* __restrict__ state,
                                                       float* __restrict__ part) {
  __shared__ float red[16];
  const unsigned tau = state[0];
  const unsigned* bits = reinterpret_cast<const unsigned*>(nll);
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const unsigned u = bits[i];
    acc += u > tau ? __builtin_bit_cast(float, u) : 0.f;
  }
  const float r = block_sum(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// out[0] = (sum_{nll > tau} nll + r tau) / n;  sel[0] = tau bits, sel[1] = 1/n (gradient scale of nll > tau), sel[2] = (r/m)/n (nll == tau)
__global__ void topk_finish_kernel(const float* __restrict__ part, const unsigned* __restrict__ state, unsigned n_top,
                                   float* __restrict__ out, float* __restrict__ sel, int* __restrict__ bad_label) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < TK_SUM_BLOCKS; ++i) s += part[i];
  const unsigned tau_bits = state[0], r = state[1], m = state[2];
  const float tau = __builtin_bit_cast(float, tau_bits);
  const float qn = __builtin_nanf("");
  float loss, sgt, seq;
  if (n_top == 0u) {  // the reference takes the mean of an empty tensor: NaN, and no pixel carries a gradient
    loss = qn; sgt = 0.f; seq = 0.f;
    sel[0] = __builtin_bit_cast(float, 0x7F800000u);
  } else {
    loss = (float)((s + (double)r * (double)tau) / (double)n_top);
    sgt = (float)(1.0 / (double)n_top);
    seq = (float)(((double)r / (double)(m ? m : 1u)) / (double)n_top);
    sel[0] = tau;
  }
  const int bad = bad_label[0];
  if (bad) { bad_label[1] = 1; loss = qn; sgt = qn; seq = qn; }
  bad_label[0] = 0;
  out[0] = loss; sel[1] = sgt; sel[2] = seq;
}

template <typename LT>
__global__ __launch_bounds__(256) void topk_bwd_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                       const float* __restrict__ cw_g, const float* __restrict__ nll,
                                                       const float* __restrict__ sel, const float* __restrict__ gout,
                                                       float* __restrict__ dl, int nb, int64_t hw, int k1, LossGeom g, LossGeom go,
                                                       LossIgnore ign) {
  const int64_t total = (int64_t)nb * hw;
  const float go_s = gout ? gout[0] : 1.f;
  const unsigned tau = __builtin_bit_cast(unsigned, sel[0]);
  const float sgt = go_s * sel[1], seq = go_s * sel[2];
  const unsigned* bits = reinterpret_cast<const unsigned*>(nll);
  float cw[LOSS_MAXK];
  sl_load_weights<LOSS_MAXK>(cw_g, k1, cw);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    const int64_t p = i - (int64_t)b * hw;
    const unsigned u = bits[i];
    const int c = sl_class(labels, i, k1, ign);
    const bool live = c >= 0 && u >= tau;
    float* dst = dl + b * go.sn + p * go.sp;
    float o[LOSS_MAXK];
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k) o[k] = 0.f;
    if (live) {
      const float* src = logits + b * g.sn + p * g.sp;
      float v[LOSS_MAXK], pr[LOSS_MAXK], mx, se = 0.f, wc = 0.f;
#pragma unroll
      for (int k = 0; k < LOSS_MAXK; ++k) v[k] = (k < k1) ? src[k * g.sk] : 0.f;
      mx = v[0];
#pragma unroll
      for (int k = 1; k < LOSS_MAXK; ++k)
        if (k < k1) mx = fmaxf(mx, v[k]);
#pragma unroll
      for (int k = 0; k < LOSS_MAXK; ++k)
        if (k < k1) { pr[k] = expf(v[k] - mx); se += pr[k]; wc = (c == k) ? cw[k] : wc; }
      const float sc = (u > tau ? sgt : seq) * wc, inv = 1.f / se;
#pragma unroll
      for (int k = 0; k < LOSS_MAXK; ++k)
        if (k < k1) o[k] = sc * (pr[k] * inv - (c == k ? 1.f : 0.f));
    }
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) dst[k * go.sk] = o[k];
  }
}

static int sl_blocks(int64_t total, int cap) {
  const int64_t b = (total + 255) / 256;
  return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

// ================================================================ C ABI
extern "C" int mia_seg_loss_workspace(int nb, int k1, int slabs) {
  if (nb <= 0 || k1 <= 0 || slabs <= 0) return 0;
  return (int)(sl_slices_words(nb, k1, slabs) + (size_t)nb * k1 * 6);
}

extern "C" int mia_seg_loss_fwd(const float* logits, const void* labels, const float* class_w, int nb, int64_t hw, int k1, int64_t sn,
                                int64_t sk, int64_t sp, int flags, int64_t ignore_label, float smooth, float dice_w, float ce_w,
                                int slabs, float* workspace, float* coef, float* out, int64_t* counts, int* bad_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && workspace && coef && out && counts && bad_label, "mia_seg_loss_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0, "mia_seg_loss_fwd: bad shape");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_seg_loss_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mia_seg_loss_fwd: workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  const LossIgnore ign = make_ignore((flags & SL_IGNORE) != 0, ignore_label);
  const bool u8 = (flags & SL_LABEL_U8) != 0;
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  const long long* l64 = static_cast<const long long*>(labels);
  const unsigned char* l8 = static_cast<const unsigned char*>(labels);
  if (sl_fast_ok(logits, labels, hw, k1, sn, sk, sp, flags)) {
#define SL_FWD_FAST(K)                                                                                                                        \
  if (u8) hipLaunchKernelGGL((seg_loss_fwd_fast_kernel<K, unsigned char>), grid, blk, 0, st, logits, l8, class_w, (int)hw, flags, ign, slabs, \
                             workspace, bad_label);                                                                                           \
  else hipLaunchKernelGGL((seg_loss_fwd_fast_kernel<K, long long>), grid, blk, 0, st, logits, l64, class_w, (int)hw, flags, ign, slabs,       \
                          workspace, bad_label)
    if (k1 == 2) { SL_FWD_FAST(2); } else if (k1 == 3) { SL_FWD_FAST(3); } else { SL_FWD_FAST(4); }
#undef SL_FWD_FAST
  } else if (u8) {
    hipLaunchKernelGGL(seg_loss_fwd_kernel<unsigned char>, grid, blk, 0, st, logits, l8, class_w, hw, k1, g, flags, ign, slabs, workspace, bad_label);
  } else {
    hipLaunchKernelGGL(seg_loss_fwd_kernel<long long>, grid, blk, 0, st, logits, l64, class_w, hw, k1, g, flags, ign, slabs, workspace, bad_label);
  }
  double* tot = reinterpret_cast<double*>(workspace + sl_slices_words(nb, k1, slabs));
  hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, tot, nb, slabs, k1, flags, smooth, dice_w, ce_w, coef,
                     out, reinterpret_cast<long long*>(counts), bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_seg_loss_bwd(const float* logits, const void* labels, const float* class_w, const float* coef, const float* grad_out,
                                float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk,
                                int64_t gsp, int flags, int64_t ignore_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && coef && dlogits && nb > 0 && hw > 0, "mia_seg_loss_bwd: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_seg_loss_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  const LossIgnore ign = make_ignore((flags & SL_IGNORE) != 0, ignore_label);
  const bool u8 = (flags & SL_LABEL_U8) != 0;
  const long long* l64 = static_cast<const long long*>(labels);
  const unsigned char* l8 = static_cast<const unsigned char*>(labels);
  if (sl_fast_ok(logits, labels, hw, k1, sn, sk, sp, flags) && gsn == sn && gsk == sk && gsp == sp &&
      (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0) {
    const unsigned quads = (unsigned)(hw >> 2);
    const dim3 grid((quads + 255) / 256 < 512u ? (quads + 255) / 256 : 512u, (unsigned)nb), blk(256);
#define SL_BWD_FAST(K)                                                                                                                     \
  if (u8) hipLaunchKernelGGL((seg_loss_bwd_fast_kernel<K, unsigned char>), grid, blk, 0, st, logits, l8, class_w, coef, grad_out, dlogits, \
                             nb, (int)hw, flags, ign);                                                                                     \
  else hipLaunchKernelGGL((seg_loss_bwd_fast_kernel<K, long long>), grid, blk, 0, st, logits, l64, class_w, coef, grad_out, dlogits, nb,   \
                          (int)hw, flags, ign)
    if (k1 == 2) { SL_BWD_FAST(2); } else if (k1 == 3) { SL_BWD_FAST(3); } else { SL_BWD_FAST(4); }
#undef SL_BWD_FAST
    MIA_LAUNCH_CHECK();
    return MIA_OK;
  }
  const dim3 grid((unsigned)sl_blocks((int64_t)nb * hw, 8192)), blk(256);
  if (u8) hipLaunchKernelGGL(seg_loss_bwd_kernel<unsigned char>, grid, blk, 0, st, logits, l8, class_w, coef, grad_out, dlogits, nb, hw, k1, g, go, flags, ign);
  else hipLaunchKernelGGL(seg_loss_bwd_kernel<long long>, grid, blk, 0, st, logits, l64, class_w, coef, grad_out, dlogits, nb, hw, k1, g, go, flags, ign);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// words: nll [n_pixels], sel [4], histograms [4][256], state [4], partial sums [TK_SUM_BLOCKS]
extern "C" int mia_topk_ce_workspace(int64_t n_pixels) {
  const int64_t extra = 4 + TK_HIST_WORDS + 4 + TK_SUM_BLOCKS;
  return (n_pixels <= 0 || n_pixels >= ((int64_t)1 << 31) - extra) ? 0 : (int)(n_pixels + extra);
}

extern "C" int mia_topk_ce_fwd(const float* logits, const void* labels, const float* class_w, int nb, int64_t hw, int k1, int64_t sn,
                               int64_t sk, int64_t sp, int flags, int64_t ignore_label, int64_t n_top, float* workspace, float* out,
                               int* bad_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && workspace && out && bad_label, "mia_topk_ce_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0, "mia_topk_ce_fwd: bad shape");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_topk_ce_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  const int64_t total = (int64_t)nb * hw;
  MIA_CHECK_ARG(total < ((int64_t)1 << 31), "mia_topk_ce_fwd: more than 2^31 pixels");
  MIA_CHECK_ARG(n_top >= 0 && n_top <= total, "mia_topk_ce_fwd: n_top=%lld not in [0, %lld]", (long long)n_top, (long long)total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  const LossIgnore ign = make_ignore((flags & SL_IGNORE) != 0, ignore_label);
  float* nll = workspace;
  float* sel = workspace + total;
  unsigned* hist = reinterpret_cast<unsigned*>(sel + 4);
  unsigned* state = hist + TK_HIST_WORDS;
  float* part = reinterpret_cast<float*>(state + 4);
  const dim3 blk(256), grid((unsigned)sl_blocks(total, 4096)), hgrid((unsigned)sl_blocks((total + 15) / 16, 1024));
  if (flags & SL_LABEL_U8)
    hipLaunchKernelGGL(topk_nll_kernel<unsigned char>, grid, blk, 0, st, logits, static_cast<const unsigned char*>(labels), class_w, nb, hw,
                       k1, g, ign, (unsigned)n_top, nll, hist, state, bad_label);
  else
    hipLaunchKernelGGL(topk_nll_kernel<long long>, grid, blk, 0, st, logits, static_cast<const long long*>(labels), class_w, nb, hw, k1, g,
                       ign, (unsigned)n_top, nll, hist, state, bad_label);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(topk_hist_kernel, hgrid, blk, 0, st, nll, total, pass, state, hist);
    hipLaunchKernelGGL(topk_scan_kernel, dim3(1), blk, 0, st, pass, hist, state);
  }
  hipLaunchKernelGGL(topk_sum_kernel, dim3(TK_SUM_BLOCKS), blk, 0, st, nll, total, state, part);
  hipLaunchKernelGGL(topk_finish_kernel, dim3(1), dim3(64), 0, st, part, state, (unsigned)n_top, out, sel, bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_topk_ce_bwd(const float* logits, const void* labels, const float* class_w, const float* workspace,
                               const float* grad_out, float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                               int64_t gsn, int64_t gsk, int64_t gsp, int flags, int64_t ignore_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && workspace && dlogits && nb > 0 && hw > 0, "mia_topk_ce_bwd: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_topk_ce_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  const LossIgnore ign = make_ignore((flags & SL_IGNORE) != 0, ignore_label);
  const int64_t total = (int64_t)nb * hw;
  const float* nll = workspace;
  const float* sel = workspace + total;
  const dim3 blk(256), grid((unsigned)sl_blocks(total, 8192));
  if (flags & SL_LABEL_U8)
    hipLaunchKernelGGL(topk_bwd_kernel<unsigned char>, grid, blk, 0, st, logits, static_cast<const unsigned char*>(labels), class_w, nll,
                       sel, grad_out, dlogits, nb, hw, k1, g, go, ign);
  else
    hipLaunchKernelGGL(topk_bwd_kernel<long long>, grid, blk, 0, st, logits, static_cast<const long long*>(labels), class_w, nll, sel,
                       grad_out, dlogits, nb, hw, k1, g, go, ign);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
