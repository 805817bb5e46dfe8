// Fused Dice + cross-entropy loss on the logits of the 1x1 head (K1 <= 8 classes), gfx950.
//
// Reference: DiceLoss.forward (src/losses/dice_loss.py:32-76); DiceAndCELoss.forward (src/losses/compound_losses.py:33-49) with
// torch.nn.CrossEntropyLoss (mean over all pixels).  Pure bandwidth: the loss reads K1 logits + one label per pixel ONCE (the
// reference materialises softmax, a long one-hot, a float one-hot and a product) and reduces I = sum p*t, sum p (or p^2), sum t per
// (image, class) plus the CE sum with wave shuffles, no float atomics.
#include "loss_common.h"

// forward partials: part[b][slab][k][3] (I, sum_p, sum_t) and cepart[b][slab]
__global__ void dice_ce_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int64_t hw, int k1,
                                   LossGeom g, int flags, int slabs, float* __restrict__ part, float* __restrict__ cepart,
                                   int* __restrict__ bad_label) {
  __shared__ float red[16];
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t per = (hw + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  float si[LOSS_MAXK], sp[LOSS_MAXK], st[LOSS_MAXK], ce = 0.f;
#pragma unroll
  for (int k = 0; k < LOSS_MAXK; ++k) { si[k] = 0.f; sp[k] = 0.f; st[k] = 0.f; }
  const float* base = logits + b * g.sn;
  for (int64_t p = r0 + threadIdx.x; p < r1; p += blockDim.x) {
    float v[LOSS_MAXK];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) { v[k] = base[p * g.sp + k * g.sk]; mx = fmaxf(mx, v[k]); }
    const float* dense = reinterpret_cast<const float*>(labels) + (int64_t)b * k1 * hw + p;
    const long long lab = (flags & LF_DENSE) ? 0 : labels[(int64_t)b * hw + p];
    if (lab < 0 || lab >= k1) { *bad_label = 1; continue; }  // finalize poisons the loss with NaN (see there)
    float pr[LOSS_MAXK];
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
    const float inv = 1.f / se;
    const float lse = mx + __logf(se);
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) {
        const float pk = (flags & LF_SOFTMAX) ? pr[k] * inv : v[k];
        const float t = (flags & LF_DENSE) ? dense[k * hw] : ((k == (int)lab) ? 1.f : 0.f);
        si[k] += pk * t;
        sp[k] += (flags & LF_SQUARED) ? pk * pk : pk;
        st[k] += (flags & LF_SQUARED) ? t * t : t;
        ce += t * (lse - v[k]);
      }
  }
  for (int k = 0; k < k1; ++k) {
    float* dst = part + (((size_t)b * slabs + s) * k1 + k) * 3;
    float r;
    r = block_sum(si[k], red); if (threadIdx.x == 0) dst[0] = r;
    r = block_sum(sp[k], red); if (threadIdx.x == 0) dst[1] = r;
    r = block_sum(st[k], red); if (threadIdx.x == 0) dst[2] = r;
  }
  const float r = block_sum(ce, red);
  if (threadIdx.x == 0) cepart[(size_t)b * slabs + s] = r;
}


// Fast path: channels-last logits (class stride 1, pixel stride K1), int64 index labels, K1 in {2,3,4}, hw % 4 == 0.
// A thread owns FOUR consecutive pixels per step: K1 16-byte loads of logits + two 16-byte loads of labels (the generic
// kernel issues K1 + 2 four-byte loads per pixel), two steps in flight.  One block = one slab of one image; all 3*K1+1
// block sums share ONE barrier (per-wave DPP sums -> LDS -> 3*K1+1 threads add four waves).
template <int K1>
__global__ __launch_bounds__(256) void dice_ce_fwd_fast_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                               int hw, int flags, int slabs, float* __restrict__ part,
                                                               float* __restrict__ cepart, int* __restrict__ bad_label) {
  constexpr int NV = 3 * K1 + 1;
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int quads = hw >> 2;
  const int per = (quads + slabs - 1) / slabs, q0 = s * per, q1 = q0 + per < quads ? q0 + per : quads;
  const f32x4* lg = reinterpret_cast<const f32x4*>(logits + (size_t)b * hw * K1);
  const long long* lb = labels + (size_t)b * hw;
  float si[K1], sp[K1], st[K1], ce = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) { si[k] = 0.f; sp[k] = 0.f; st[k] = 0.f; }
  bool bad = false;
  auto one = [&](const f32x4* f, const unsigned (&lo)[4], const unsigned (&hi)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[K1];
      quad_unpack<K1>(f, j, v);
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < K1; ++k) mx = fmaxf(mx, v[k]);
      const bool ok = hi[j] == 0u && lo[j] < (unsigned)K1;
      bad |= !ok;
      float pr[K1], se = 0.f;
#pragma unroll
      for (int k = 0; k < K1; ++k) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
      const float inv = ok ? 1.f / se : 0.f;   // an out-of-range label drops the pixel (and poisons the loss in finalize)
      const float lse = mx + __logf(se);
#pragma unroll
      for (int k = 0; k < K1; ++k) {
        const float pk = (flags & LF_SOFTMAX) ? pr[k] * inv : (ok ? v[k] : 0.f);
        const float t = (ok && lo[j] == (unsigned)k) ? 1.f : 0.f;
        si[k] += pk * t;
        sp[k] += (flags & LF_SQUARED) ? pk * pk : pk;
        st[k] += t;
        ce += t * (lse - v[k]);
      }
    }
  };
  int q = q0 + threadIdx.x;
  for (; q + 256 < q1; q += 512) {
    f32x4 fa[K1], fb[K1];
    unsigned loa[4], hia[4], lob[4], hib[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) { fa[k] = lg[(size_t)q * K1 + k]; fb[k] = lg[(size_t)(q + 256) * K1 + k]; }
    load_label_quad(lb + 4 * (size_t)q, loa, hia);
    load_label_quad(lb + 4 * (size_t)(q + 256), lob, hib);
    one(fa, loa, hia);
    one(fb, lob, hib);
  }
  if (q < q1) {
    f32x4 fa[K1];
    unsigned loa[4], hia[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) fa[k] = lg[(size_t)q * K1 + k];
    load_label_quad(lb + 4 * (size_t)q, loa, hia);
    one(fa, loa, hia);
  }
  if (bad) *bad_label = 1;
  auto red = loss_block_sums<NV, 0>();
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    const float v[3] = {si[k], sp[k], st[k]};
    red.put(3 * k, v);
  }
  const float v[1] = {ce};
  red.put(3 * K1, v);
  __syncthreads();
  if (threadIdx.x < NV) {
    const float r = red.sum_f(threadIdx.x);
    if (threadIdx.x < 3 * K1) part[((size_t)b * slabs + s) * K1 * 3 + threadIdx.x] = r;
    else cepart[(size_t)b * slabs + s] = r;
  }
}

template <int K1>
__global__ __launch_bounds__(256) void dice_ce_bwd_fast_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                               const float* __restrict__ coef, const float* __restrict__ gout,
                                                               float* __restrict__ dl, int nb, int hw, int flags, float dice_w,
                                                               float ce_w) {
  const int b = blockIdx.y;
  const int quads = hw >> 2;
  const float go_s = gout ? gout[0] : 1.f;
  const float cew = go_s * ce_w / (float)((double)nb * (double)hw);
  float al[K1], be[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) { al[k] = go_s * dice_w * coef[((size_t)b * K1 + k) * 2]; be[k] = go_s * dice_w * coef[((size_t)b * K1 + k) * 2 + 1]; }
  const f32x4* lg = reinterpret_cast<const f32x4*>(logits + (size_t)b * hw * K1);
  const long long* lb = labels + (size_t)b * hw;
  f32x4* dst = reinterpret_cast<f32x4*>(dl + (size_t)b * hw * K1);
  for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
    f32x4 f[K1], o[K1];
    unsigned lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < K1; ++k) f[k] = lg[(size_t)q * K1 + k];
    load_label_quad(lb + 4 * (size_t)q, lo, hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[K1], pr[K1], gk[K1];
      float mx = -INFINITY, se = 0.f, dot = 0.f;
#pragma unroll
      for (int k = 0; k < K1; ++k) { v[k] = f[(j * K1 + k) >> 2][(j * K1 + k) & 3]; mx = fmaxf(mx, v[k]); }
#pragma unroll
      for (int k = 0; k < K1; ++k) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
      const bool ok = hi[j] == 0u && lo[j] < (unsigned)K1;
      const float inv = 1.f / se;
#pragma unroll
      for (int k = 0; k < K1; ++k) {
        pr[k] *= inv;
        const float pk = (flags & LF_SOFTMAX) ? pr[k] : v[k];
        const float t = (lo[j] == (unsigned)k) ? 1.f : 0.f;
        gk[k] = al[k] * t + be[k] * ((flags & LF_SQUARED) ? 2.f * pk : 1.f);
        dot += gk[k] * pr[k];
      }
#pragma unroll
      for (int k = 0; k < K1; ++k) {
        const float t = (lo[j] == (unsigned)k) ? 1.f : 0.f;
        const float dd = (flags & LF_SOFTMAX) ? pr[k] * (gk[k] - dot) : gk[k];
        // a pixel with a bad label is poisoned like every other one (coef is NaN after such a forward), never a quiet zero
        o[(j * K1 + k) >> 2][(j * K1 + k) & 3] = ok ? dd + cew * (pr[k] - t) : __builtin_nanf("");
      }
    }
#pragma unroll
    for (int k = 0; k < K1; ++k) dst[(size_t)q * K1 + k] = o[k];
  }
}

static bool dice_ce_fast_ok(const void* logits, const void* labels, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int flags) {
  return !(flags & LF_DENSE) && k1 >= 2 && k1 <= 4 && sk == 1 && sp == k1 && sn == hw * k1 && (hw & 3) == 0 && hw < ((int64_t)1 << 30) &&
         (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0;
}

// finalize: sums[b][k][3]; coef[b][k][2] = (alpha, beta) with dDice/dp_k(pixel) = alpha*t (+2p*... if squared) + beta
// out[0] = total loss, out[1] = ce, out[2] = dice
__global__ void dice_ce_finalize_kernel(const float* __restrict__ part, const float* __restrict__ cepart, int nb, int slabs,
                                        int k1, int64_t hw, int flags, float smooth, float dice_w, float ce_w,
                                        float* __restrict__ sums, float* __restrict__ coef, float* __restrict__ out,
                                        int* __restrict__ bad_label) {
  // single block; thread -> (b,k)
  __shared__ double dsum[256];
  __shared__ double cesum[256];
  const int kb = (flags & LF_DO_BG) ? 0 : 1;
  const int nk = k1 - kb;
  const int total = nb * k1;
  double mydice = 0.0, myce = 0.0;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int b = i / k1, k = i % k1;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int s = 0; s < slabs; ++s) {
      const float* p = part + (((size_t)b * slabs + s) * k1 + k) * 3;
      a0 += p[0]; a1 += p[1]; a2 += p[2];
    }
    sums[i * 3 + 0] = (float)a0; sums[i * 3 + 1] = (float)a1; sums[i * 3 + 2] = (float)a2;
  }
  for (int i = threadIdx.x; i < nb * slabs; i += blockDim.x) myce += cepart[i];
  __syncthreads();
  // dice terms (thread per (b,k) for !batch, per k for batch)
  if (flags & LF_BATCH) {
    for (int k = kb + threadIdx.x; k < k1; k += blockDim.x) {
      double I = 0, P = 0, Tt = 0;
      for (int b = 0; b < nb; ++b) { I += sums[(b * k1 + k) * 3]; P += sums[(b * k1 + k) * 3 + 1]; Tt += sums[(b * k1 + k) * 3 + 2]; }
      I /= nb; P /= nb; Tt /= nb;
      const double num = 2 * I + smooth, den = P + Tt + smooth;
      mydice += (1.0 - num / den) / nk;
      // d(dice_k)/dI_b = -(2/den)/nb ; d/dP_b = (num/den^2)/nb ; loss = mean_k
      for (int b = 0; b < nb; ++b) {
        coef[(b * k1 + k) * 2 + 0] = (float)(-(2.0 / den) / nb / nk);
        coef[(b * k1 + k) * 2 + 1] = (float)((num / (den * den)) / nb / nk);
      }
    }
  } else {
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int k = i % k1;
      if (k < kb) continue;
      const double I = sums[i * 3], P = sums[i * 3 + 1], Tt = sums[i * 3 + 2];
      const double num = 2 * I + smooth, den = P + Tt + smooth;
      mydice += (1.0 - num / den) / ((double)nb * nk);
      coef[i * 2 + 0] = (float)(-(2.0 / den) / ((double)nb * nk));
      coef[i * 2 + 1] = (float)((num / (den * den)) / ((double)nb * nk));
    }
  }
  if (!(flags & LF_DO_BG))
    for (int b = threadIdx.x; b < nb; b += blockDim.x) { coef[(b * k1) * 2] = 0.f; coef[(b * k1) * 2 + 1] = 0.f; }
  dsum[threadIdx.x] = mydice; cesum[threadIdx.x] = myce;
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0, c = 0;
    for (int i = 0; i < blockDim.x; ++i) { d += dsum[i]; c += cesum[i]; }
    c /= ((double)nb * (double)hw);
    out[1] = (float)c; out[2] = (float)d;
    out[0] = (float)(ce_w * c + dice_w * d);
  }
  loss_bad_label_verdict(bad_label, out, coef, total * 2);
}

int mia_dice_ce_finalize_launch(const float* part, const float* cepart, int nb, int slabs, int k1, int64_t hw, int flags, float smooth,
                                float dice_w, float ce_w, float* sums, float* coef, float* out, int* bad_label, hipStream_t st) {
  hipLaunchKernelGGL(dice_ce_finalize_kernel, dim3(1), dim3(256), 0, st, part, cepart, nb, slabs, k1, hw, flags, smooth, dice_w, ce_w, sums,
                     coef, out, bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// backward: dlogits[b,p,k] = gout * ( ce_w/(B*HW) * (softmax_k - t_k) + dice_w * dDice/dlogit_k )
__global__ void dice_ce_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                   const float* __restrict__ coef, const float* __restrict__ gout, float* __restrict__ dl,
                                   int nb, int64_t hw, int k1, LossGeom g, LossGeom go, int flags, float dice_w, float ce_w) {
  const int64_t total = (int64_t)nb * hw;
  const float go_s = gout ? gout[0] : 1.f;
  const float cew = ce_w / (float)((double)nb * (double)hw);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / hw);
    const int64_t p = i - (int64_t)b * hw;
    const float* src = logits + b * g.sn + p * g.sp;
    float v[LOSS_MAXK], pr[LOSS_MAXK];
    float mx = -INFINITY, se = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) { v[k] = src[k * g.sk]; mx = fmaxf(mx, v[k]); }
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) { pr[k] = __expf(v[k] - mx); se += pr[k]; }
    const float inv = 1.f / se;
    const float* dense = reinterpret_cast<const float*>(labels) + (int64_t)b * k1 * hw + p;
    const int lab = (flags & LF_DENSE) ? 0 : (int)labels[i];
    // dL/dp_k for the dice part
    float gk[LOSS_MAXK], tk[LOSS_MAXK], dot = 0.f, tsum = 0.f;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) {
        const float sm = pr[k] * inv;
        const float pk = (flags & LF_SOFTMAX) ? sm : v[k];
        const float al = coef[((size_t)b * k1 + k) * 2], be = coef[((size_t)b * k1 + k) * 2 + 1];
        tk[k] = (flags & LF_DENSE) ? dense[k * hw] : (k == lab ? 1.f : 0.f);
        tsum += tk[k];
        float gg = al * tk[k] + be * ((flags & LF_SQUARED) ? 2.f * pk : 1.f);
        gk[k] = gg * dice_w;
        pr[k] = sm;
        dot += gk[k] * sm;
      }
    float* dst = dl + b * go.sn + p * go.sp;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) {
        const float dd = (flags & LF_SOFTMAX) ? pr[k] * (gk[k] - dot) : gk[k];
        const float dc = cew * (tsum * pr[k] - tk[k]);  // d/dv_k of sum_j t_j (lse - v_j)
        dst[k * go.sk] = go_s * (dd + dc);
      }
  }
}

extern "C" int mia_dice_ce_workspace(int nb, int k1, int slabs) { return nb * slabs * (k1 * 3 + 1); }

// sums: [B][K1][3], coef: [B][K1][2], out: [3] (loss, ce, dice), bad_label: int flag (device)
extern "C" int mia_dice_ce_fwd(const float* logits, const long long* labels, int nb, int64_t hw, int k1, int64_t sn, int64_t sk,
                               int64_t sp, int flags, float smooth, float dice_w, float ce_w, int slabs, float* workspace,
                               float* sums, float* coef, float* out, int* bad_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && workspace && sums && coef && out && bad_label, "mia_dice_ce_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0, "mia_dice_ce_fwd: bad shape");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_dice_ce_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  hipStream_t st = static_cast<hipStream_t>(stream);
  LossGeom g{sn, sk, sp};
  float* part = workspace;
  float* cepart = workspace + (size_t)nb * slabs * k1 * 3;
  if (dice_ce_fast_ok(logits, labels, hw, k1, sn, sk, sp, flags)) {
    if (k1 == 2) hipLaunchKernelGGL(dice_ce_fwd_fast_kernel<2>, dim3(nb * slabs), dim3(256), 0, st, logits, labels, (int)hw, flags, slabs, part, cepart, bad_label);
    else if (k1 == 3) hipLaunchKernelGGL(dice_ce_fwd_fast_kernel<3>, dim3(nb * slabs), dim3(256), 0, st, logits, labels, (int)hw, flags, slabs, part, cepart, bad_label);
    else hipLaunchKernelGGL(dice_ce_fwd_fast_kernel<4>, dim3(nb * slabs), dim3(256), 0, st, logits, labels, (int)hw, flags, slabs, part, cepart, bad_label);
  } else {
    hipLaunchKernelGGL(dice_ce_fwd_kernel, dim3(nb * slabs), dim3(256), 0, st, logits, labels, hw, k1, g, flags, slabs, part, cepart, bad_label);
  }
  hipLaunchKernelGGL(dice_ce_finalize_kernel, dim3(1), dim3(256), 0, st, part, cepart, nb, slabs, k1, hw, flags, smooth, dice_w, ce_w, sums, coef, out, bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_dice_ce_bwd(const float* logits, const long long* labels, const float* coef, const float* grad_out,
                               float* dlogits, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t gsn,
                               int64_t gsk, int64_t gsp, int flags, float dice_w, float ce_w, void* stream) {
  MIA_CHECK_ARG(logits && labels && coef && dlogits && nb > 0 && hw > 0, "mia_dice_ce_bwd: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_dice_ce_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  const int64_t total = (int64_t)nb * hw;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  if (dice_ce_fast_ok(logits, labels, hw, k1, sn, sk, sp, flags) && gsn == sn && gsk == sk && gsp == sp &&
      (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int quads = (int)(hw >> 2);
    const dim3 grid((unsigned)(quads + 255) / 256 < 512u ? (unsigned)(quads + 255) / 256 : 512u, (unsigned)nb);
    if (k1 == 2) hipLaunchKernelGGL(dice_ce_bwd_fast_kernel<2>, grid, dim3(256), 0, st, logits, labels, coef, grad_out, dlogits, nb, (int)hw, flags, dice_w, ce_w);
    else if (k1 == 3) hipLaunchKernelGGL(dice_ce_bwd_fast_kernel<3>, grid, dim3(256), 0, st, logits, labels, coef, grad_out, dlogits, nb, (int)hw, flags, dice_w, ce_w);
    else hipLaunchKernelGGL(dice_ce_bwd_fast_kernel<4>, grid, dim3(256), 0, st, logits, labels, coef, grad_out, dlogits, nb, (int)hw, flags, dice_w, ce_w);
    MIA_LAUNCH_CHECK();
    return MIA_OK;
  }
  hipLaunchKernelGGL(dice_ce_bwd_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), logits, labels, coef,
                     grad_out, dlogits, nb, hw, k1, g, go, flags, dice_w, ce_w);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
