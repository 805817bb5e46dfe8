// Region-based loss (nnU-Net's region mode; reference src/losses/compound_losses.py:178-233, DC_and_BCE_loss over
// MemoryEfficientSoftDiceLoss(apply_nonlin=sigmoid) + BCEWithLogitsLoss): one sigmoid output per region, regions may overlap, the
// target is a multi-label mask with an optional ignore channel.
//
//   p = sigmoid(z);  per valid pixel and channel:  I += p t,  P += p,  G += t,
//   bce += pw_c t softplus(-z) + (1 - t) softplus(z),   softplus(z) = max(z, 0) + log1p(exp(-|z|))
//   dc = -mean (2I + smooth) / max(G + P + smooth, 1e-8)   (channel 0 dropped without RL_DO_BG; I, P, G summed over the batch first
//   with RL_BATCH);  CE = bce / (B C HW) without RL_IGNORE, bce / max(#valid pixels, 1e-8) with it (the reference's mask broadcasts
//   over the channels: the sum runs over all C channels, the divisor counts pixels);  loss = ce_w CE + dice_w dc
//   counts = tp, fp, fn of (z > 0) against (t > 0.5) over the valid pixels.
//
// The target comes dense ([B][C (+1)][HW], 1-byte or fp32 elements, the extra last channel = ignore) or as a label map plus a table
// region_bits[label] (bit c = label belongs to region c).  Both forms go through the SAME kernel template, which differs only in the
// loader that fills t[] and `valid`: a thread owns the four consecutive pixels 4q .. 4q+3 of a quad whatever the loader and whatever
// the access width (16-byte accesses where layout and alignment allow, scalar ones otherwise), a block owns a contiguous range of
// quads of one image, and all sums run in a fixed order -- so the two forms of one target, and the vector and scalar paths, give
// the same bits.  Floating-point contraction is off for the whole file so that no instantiation fuses what another does not.
// No float atomics, nothing synchronises with the host, every launch goes to the caller's stream.
#include "common.h"

#pragma clang fp contract(off)  // ahead of loss_common.h: what this file instantiates from there is compiled without contraction too
#include "loss_common.h"

#define RL_DO_BG 1
#define RL_BATCH 2
#define RL_IGNORE 4
#define RL_INDEX 8
#define RL_TARGET_U8 16

enum { LM_SCALAR = 0, LM_PLANAR4 = 1, LM_CLAST4 = 2 };                      // how a quad of logits is read / written
enum { TK_DENSE_U8 = 0, TK_DENSE_F32 = 1, TK_INDEX_U8 = 2, TK_INDEX_I64 = 3 };  // target loader

struct RlTarget {
  const void* ptr;        // dense [B][ct][HW] (1-byte or fp32 elements) or labels [B][HW] (uint8 or int64)
  const unsigned* bits;   // region_bits[n_labels], index form only
  int n_labels;
  int ct;                 // channels of the dense target: C, or C + 1 with the ignore channel
  LossIgnore ign;
};

// region bits of one label, or 0 with valid = false (ignored) / bad = true (neither a label of the table nor the ignore label)
__device__ __forceinline__ unsigned rl_label_bits(const RlTarget& tg, unsigned lo, unsigned hi, bool is_ign, bool& valid, bool& bad) {
  const bool in = hi == 0u && lo < (unsigned)tg.n_labels;
  valid = in && !is_ign;
  bad |= !in && !is_ign;
  return valid ? tg.bits[lo] : 0u;
}

// t[j][k] and valid[j] of the pixels 4q + j, j < n, of image b (n = 4 on the vector path); pixels j >= n come back invalid
template <int NC, int TK, bool VEC>
__device__ __forceinline__ void rl_load_target(const RlTarget& tg, int b, int64_t hw, int64_t q, int c, int n, float (&t)[4][NC],
                                               bool (&valid)[4], bool& bad) {
  if (TK == TK_DENSE_U8) {
    const unsigned char* base = static_cast<const unsigned char*>(tg.ptr) + (int64_t)b * tg.ct * hw + 4 * q;
    unsigned ig = 0u;
    if (VEC) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const unsigned w = k < c ? *reinterpret_cast<const unsigned*>(base + k * hw) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j][k] = (float)((w >> (8 * j)) & 0xFFu);
      }
      if (tg.ign.on) ig = *reinterpret_cast<const unsigned*>(base + (int64_t)(tg.ct - 1) * hw);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < NC; ++k) t[j][k] = (j < n && k < c) ? (float)base[k * hw + j] : 0.f;
        if (tg.ign.on && j < n) ig |= (unsigned)base[(int64_t)(tg.ct - 1) * hw + j] << (8 * j);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) valid[j] = j < n && ((ig >> (8 * j)) & 0xFFu) == 0u;
  } else if (TK == TK_DENSE_F32) {
    const float* base = static_cast<const float*>(tg.ptr) + (int64_t)b * tg.ct * hw + 4 * q;
    float ig[4] = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (k < c) w = *reinterpret_cast<const f32x4*>(base + k * hw);
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j][k] = w[j];
      }
      if (tg.ign.on) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(base + (int64_t)(tg.ct - 1) * hw);
#pragma unroll
        for (int j = 0; j < 4; ++j) ig[j] = w[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = 0; k < NC; ++k) t[j][k] = (j < n && k < c) ? base[k * hw + j] : 0.f;
        if (tg.ign.on && j < n) ig[j] = base[(int64_t)(tg.ct - 1) * hw + j];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) valid[j] = j < n && ig[j] == 0.f;
  } else {
    unsigned lo[4], hi[4];
    if (TK == TK_INDEX_U8) {
      const unsigned char* base = static_cast<const unsigned char*>(tg.ptr) + (int64_t)b * hw + 4 * q;
      unsigned w = 0u;
      if (VEC) {
        w = *reinterpret_cast<const unsigned*>(base);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < n) w |= (unsigned)base[j] << (8 * j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo[j] = (w >> (8 * j)) & 0xFFu; hi[j] = 0u; }
    } else {
      const long long* base = static_cast<const long long*>(tg.ptr) + (int64_t)b * hw + 4 * q;
      if (VEC) {
        load_label_quad(base, lo, hi);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned long long v = j < n ? (unsigned long long)base[j] : 0ull;
          lo[j] = (unsigned)(v & 0xFFFFFFFFull); hi[j] = (unsigned)(v >> 32);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool is_ign = TK == TK_INDEX_U8 ? (int)lo[j] == tg.ign.byte : (tg.ign.on && lo[j] == tg.ign.lo && hi[j] == tg.ign.hi);
      bool v = false, bd = false;
      unsigned bits = 0u;
      if (j < n) bits = rl_label_bits(tg, lo[j], hi[j], is_ign, v, bd);
      valid[j] = v;
      bad |= bd;
#pragma unroll
      for (int k = 0; k < NC; ++k) t[j][k] = (k < c && ((bits >> k) & 1u)) ? 1.f : 0.f;
    }
  }
}

// z[j][k] of the pixels 4q + j, j < n, of the image whose logits start at `src`
template <int NC, int LM>
__device__ __forceinline__ void rl_load_logits(const float* __restrict__ src, const LossGeom& g, int64_t q, int c, int n, float (&z)[4][NC]) {
  if (LM == LM_PLANAR4) {
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(src + k * g.sk + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j][k] = w[j];
    }
  } else if (LM == LM_CLAST4) {  // four pixels = NC consecutive 16-byte units
    f32x4 f[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) f[u] = *reinterpret_cast<const f32x4*>(src + (4 * q) * NC + 4 * u);
#pragma unroll
    for (int j = 0; j < 4; ++j) quad_unpack<NC>(f, j, z[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NC; ++k) z[j][k] = (j < n && k < c) ? src[(4 * q + j) * g.sp + k * g.sk] : 0.f;
  }
}

// sigmoid and the two soft-plus values of one logit from ONE exponential: e = exp(-|z|) in (0, 1], so nothing overflows.
// __expf is v_exp_f32 on x * log2(e): relative error about 2 ulp for x <= 0.
struct RlSig { float p, sp_pos, sp_neg; };
__device__ __forceinline__ float rl_sigmoid(float z, float& e) {
  e = __expf(-fabsf(z));
  const float r = 1.f / (1.f + e);
  return z >= 0.f ? r : e * r;
}
__device__ __forceinline__ RlSig rl_sig(float z) {
  RlSig s;
  float e;
  s.p = rl_sigmoid(z, e);
  const float l = log1pf(e);
  s.sp_pos = fmaxf(z, 0.f) + l;
  s.sp_neg = fmaxf(-z, 0.f) + l;
  return s;
}

// Per-thread accumulators of the forward pass.  NC is a compile-time bound, c <= NC the live count.
template <int NC>
struct RlAcc {
  float si[NC], sp[NC], sg[NC], bce;
  int tp[NC], pp[NC], gp[NC], nv;
  __device__ __forceinline__ void clear() {
    bce = 0.f; nv = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) { si[k] = 0.f; sp[k] = 0.f; sg[k] = 0.f; tp[k] = 0; pp[k] = 0; gp[k] = 0; }
  }
  __device__ __forceinline__ void pixel(const float (&z)[NC], const float (&t)[NC], bool valid, int c, const float (&pw)[NC]) {
#pragma unroll
    for (int k = 0; k < NC; ++k)
      if (k < c) {
        const RlSig s = rl_sig(z[k]);
        const float tk = t[k];
        const float term = (pw[k] * tk) * s.sp_neg + (1.f - tk) * s.sp_pos;
        si[k] += valid ? s.p * tk : 0.f;
        sp[k] += valid ? s.p : 0.f;
        sg[k] += valid ? tk : 0.f;
        bce += valid ? term : 0.f;
        const bool hp = z[k] > 0.f, ht = tk > 0.5f;
        pp[k] += (valid && hp) ? 1 : 0;
        gp[k] += (valid && ht) ? 1 : 0;
        tp[k] += (valid && hp && ht) ? 1 : 0;
      }
    nv += valid ? 1 : 0;
  }
};

// Block sums behind ONE barrier, written to this block's slice of the workspace: [3 c] floats (I, P, G per channel), bce, then [3 c] ints (tp, predicted, labelled), #valid pixels.
template <int NC>
__device__ __forceinline__ void rl_block_store(const RlAcc<NC>& acc, int c, float* __restrict__ slice) {
  auto red = loss_block_sums<3 * NC + 1, 3 * NC + 1>();
#pragma unroll
  for (int k = 0; k < NC; ++k)
    if (k < c) {
      const float fv[3] = {acc.si[k], acc.sp[k], acc.sg[k]};
      const int iv[3] = {acc.tp[k], acc.pp[k], acc.gp[k]};
      red.put(3 * k, fv, 3 * k, iv);
    }
  const float fv[1] = {acc.bce};
  const int iv[1] = {acc.nv};
  red.put(3 * c, fv, 3 * c, iv);
  __syncthreads();
  const int nf = 3 * c + 1;
  if ((int)threadIdx.x < nf) {
    const int i = threadIdx.x;
    slice[i] = red.sum_f(i);
  } else if ((int)threadIdx.x >= 64 && (int)threadIdx.x < 64 + nf) {
    const int i = threadIdx.x - 64;
    reinterpret_cast<int*>(slice + nf)[i] = red.sum_i(i);
  }
}

template <int NC>
__device__ __forceinline__ void rl_load_pw(const float* __restrict__ pw_g, int c, float (&pw)[NC]) {
#pragma unroll
  for (int k = 0; k < NC; ++k) pw[k] = (k < c && pw_g) ? pw_g[k] : 1.f;
}

// ---------------------------------------------------------------- forward: block (b, s) owns the quads [s per, (s + 1) per) of image b
template <int NC, int LM, int TK>
__global__ __launch_bounds__(256) void region_loss_fwd_kernel(const float* __restrict__ logits, RlTarget tg, const float* __restrict__ pw_g,
                                                              int64_t hw, int c, LossGeom g, int slabs, float* __restrict__ ws,
                                                              int* __restrict__ bad_label) {
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t nq = (hw + 3) >> 2, per = (nq + slabs - 1) / slabs, q0 = s * per, q1 = q0 + per < nq ? q0 + per : nq;
  float pw[NC];
  rl_load_pw<NC>(pw_g, c, pw);
  RlAcc<NC> acc;
  acc.clear();
  const float* src = logits + b * g.sn;
  bool bad = false;
  for (int64_t q = q0 + threadIdx.x; q < q1; q += 256) {
    const int n = hw - 4 * q >= 4 ? 4 : (int)(hw - 4 * q);
    float z[4][NC], t[4][NC];
    bool valid[4];
    rl_load_logits<NC, LM>(src, g, q, c, n, z);
    rl_load_target<NC, TK, LM != LM_SCALAR>(tg, b, hw, q, c, n, t, valid, bad);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.pixel(z[j], t[j], valid[j], c, pw);
  }
  if (bad) *bad_label = 1;
  rl_block_store<NC>(acc, c, ws + (size_t)blockIdx.x * (6 * c + 2));
}

// ---------------------------------------------------------------- finalize (one block)
// tot[b][k][3] (double: I, P, G) lives behind the per-block slices in the workspace.
// coef[b][k][2] = dice_w * (d dc / d I[b,k], d dc / d P[b,k]), both 0 where the denominator was clipped;  coef[nb c 2] = ce_w / N
// out[0] = loss, out[1] = CE, out[2] = dc;  counts[b][k][3] = tp, fp, fn (int64)
__global__ void region_loss_finalize_kernel(const float* __restrict__ ws, double* __restrict__ tot, int nb, int slabs, int c, int flags,
                                            int64_t hw, float smooth, float dice_w, float ce_w, float* __restrict__ coef,
                                            float* __restrict__ out, long long* __restrict__ counts, int* __restrict__ bad_label) {
  __shared__ double dsum[256], esum[256], vsum[256];
  const int stride = 6 * c + 2, nf = 3 * c + 1;
  const int kb = (flags & RL_DO_BG) ? 0 : 1;
  const int nk = c - kb;
  const int total = nb * c;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int b = i / c, k = i % c;
    double a0 = 0, a1 = 0, a2 = 0;
    long long t = 0, h = 0, m = 0;
    for (int s = 0; s < slabs; ++s) {
      const float* p = ws + ((size_t)b * slabs + s) * stride;
      const int* n = reinterpret_cast<const int*>(p + nf);
      a0 += p[3 * k]; a1 += p[3 * k + 1]; a2 += p[3 * k + 2];
      t += n[3 * k]; h += n[3 * k + 1]; m += n[3 * k + 2];
    }
    const long long fp = h - t, fn = m - t;
    store_data_fence();
    tot[i * 3] = a0; tot[i * 3 + 1] = a1; tot[i * 3 + 2] = a2;
    store_data_pad();  // tools/check_store_hazard.py
    counts[i * 3] = t; counts[i * 3 + 1] = fp; counts[i * 3 + 2] = fn;
    store_data_pad();
  }
  double mye = 0.0, myv = 0.0, mydice = 0.0;
  for (int i = threadIdx.x; i < nb * slabs; i += blockDim.x) {
    mye += ws[(size_t)i * stride + 3 * c];
    myv += (double)reinterpret_cast<const int*>(ws + (size_t)i * stride + nf)[3 * c];
  }
  __syncthreads();
  const double sm = (double)smooth;
  if (flags & RL_BATCH) {
    for (int k = kb + threadIdx.x; k < c; k += blockDim.x) {
      double I = 0, P = 0, G = 0;
      for (int b = 0; b < nb; ++b) { I += tot[(b * c + k) * 3]; P += tot[(b * c + k) * 3 + 1]; G += tot[(b * c + k) * 3 + 2]; }
      const double num = 2 * I + sm, den = G + P + sm;
      const bool clip = den < 1e-8;
      const double dc = clip ? 1e-8 : den;
      mydice -= (num / dc) / nk;
      const float al = clip ? 0.f : (float)(dice_w * (-2.0 / dc) / nk), be = clip ? 0.f : (float)(dice_w * (num / (dc * dc)) / nk);
      for (int b = 0; b < nb; ++b) { coef[(b * c + k) * 2] = al; coef[(b * c + k) * 2 + 1] = be; }
    }
  } else {
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      if (i % c < kb) continue;
      const double cnt = (double)nb * nk;
      const double num = 2 * tot[i * 3] + sm, den = tot[i * 3 + 2] + tot[i * 3 + 1] + sm;
      const bool clip = den < 1e-8;
      const double dc = clip ? 1e-8 : den;
      mydice -= (num / dc) / cnt;
      coef[i * 2] = clip ? 0.f : (float)(dice_w * (-2.0 / dc) / cnt);
      coef[i * 2 + 1] = clip ? 0.f : (float)(dice_w * (num / (dc * dc)) / cnt);
    }
  }
  if (!(flags & RL_DO_BG))
    for (int b = threadIdx.x; b < nb; b += blockDim.x) { coef[(b * c) * 2] = 0.f; coef[(b * c) * 2 + 1] = 0.f; }
  dsum[threadIdx.x] = mydice; esum[threadIdx.x] = mye; vsum[threadIdx.x] = myv;
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0, e = 0, v = 0;
    for (int i = 0; i < (int)blockDim.x; ++i) { d += dsum[i]; e += esum[i]; v += vsum[i]; }
    // the reference's two normalisations: the mean over every element, or the sum over valid pixels and ALL channels divided by the
    // number of valid PIXELS (clipped at 1e-8: nothing valid gives 0 / 1e-8 = 0)
    const double n = (flags & RL_IGNORE) ? (v < 1e-8 ? 1e-8 : v) : (double)nb * (double)c * (double)hw;
    const double ce = e / n;
    const float o0 = (float)((double)ce_w * ce + (double)dice_w * d), o1 = (float)ce, o2 = (float)d, cn = (float)((double)ce_w / n);
    store_data_fence();
    out[0] = o0; out[1] = o1; out[2] = o2;
    store_data_pad();
    coef[total * 2] = cn;
  }
  loss_bad_label_verdict(bad_label, out, coef, total * 2 + 1);
}

// ---------------------------------------------------------------- backward: one pass, a thread owns a quad of one image
// dL/dz = go * valid * [ (ce_w / N) (p (1 + (pw - 1) t) - pw t) + p (1 - p) (a t + b) ]; invalid pixels get exactly 0.
template <int NC, int LM, int TK>
__global__ __launch_bounds__(256) void region_loss_bwd_kernel(const float* __restrict__ logits, RlTarget tg, const float* __restrict__ pw_g,
                                                              const float* __restrict__ coef, const float* __restrict__ gout,
                                                              float* __restrict__ dl, int nb, int64_t hw, int c, LossGeom g, LossGeom go) {
  const int b = blockIdx.y;
  const int64_t nq = (hw + 3) >> 2;
  const float go_s = gout ? gout[0] : 1.f;
  const float cecoef = go_s * coef[(size_t)nb * c * 2];
  float pw[NC], al[NC], be[NC];
  rl_load_pw<NC>(pw_g, c, pw);
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    al[k] = k < c ? go_s * coef[((size_t)b * c + k) * 2] : 0.f;
    be[k] = k < c ? go_s * coef[((size_t)b * c + k) * 2 + 1] : 0.f;
  }
  const float* src = logits + b * g.sn;
  float* dst = dl + b * go.sn;
  bool bad = false;  // the forward has given the verdict; the backward only drops such pixels
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    const int n = hw - 4 * q >= 4 ? 4 : (int)(hw - 4 * q);
    float z[4][NC], t[4][NC], o[4][NC];
    bool valid[4];
    rl_load_logits<NC, LM>(src, g, q, c, n, z);
    rl_load_target<NC, TK, LM != LM_SCALAR>(tg, b, hw, q, c, n, t, valid, bad);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        float e;
        const float p = rl_sigmoid(z[j][k], e), tk = t[j][k];
        const float ce = cecoef * (p * (1.f + (pw[k] - 1.f) * tk) - pw[k] * tk);
        const float di = (p * (1.f - p)) * (al[k] * tk + be[k]);
        o[j][k] = (valid[j] && k < c) ? ce + di : 0.f;
      }
    if (LM == LM_PLANAR4) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const f32x4 w = {o[0][k], o[1][k], o[2][k], o[3][k]};
        store_data_fence();
        *reinterpret_cast<f32x4*>(dst + k * go.sk + 4 * q) = w;
        store_data_pad();  // tools/check_store_hazard.py
      }
    } else if (LM == LM_CLAST4) {
      float flat[4 * NC];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NC; ++k) flat[j * NC + k] = o[j][k];
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const f32x4 w = {flat[4 * u], flat[4 * u + 1], flat[4 * u + 2], flat[4 * u + 3]};
        store_data_fence();
        *reinterpret_cast<f32x4*>(dst + (4 * q) * NC + 4 * u) = w;
        store_data_pad();
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (j < n && k < c) dst[(4 * q + j) * go.sp + k * go.sk] = o[j][k];
    }
  }
}

// ================================================================ host side
static RlTarget rl_make_target(const void* target, const unsigned* region_bits, int n_labels, int c, int flags, int64_t ign) {
  RlTarget t;
  t.ptr = target;
  t.bits = region_bits;
  t.n_labels = n_labels;
  t.ign = make_ignore((flags & RL_IGNORE) != 0, ign);
  t.ct = c + ((flags & RL_INDEX) ? 0 : t.ign.on);
  return t;
}

static int rl_target_kind(int flags) {
  if (flags & RL_INDEX) return (flags & RL_TARGET_U8) ? TK_INDEX_U8 : TK_INDEX_I64;
  return (flags & RL_TARGET_U8) ? TK_DENSE_U8 : TK_DENSE_F32;
}

// Four pixels per thread with 16-byte accesses: C <= 4, hw a multiple of 4, planar (sp == 1) or channels-last (sk == 1, sp == C)
// logits whose image and channel strides keep every quad 16-byte aligned, and a target whose quads are aligned units of their
// own (4 bytes of 1-byte elements, 16 bytes of fp32, 32 bytes of int64 read as two 16-byte units).
static int rl_logits_mode(const void* logits, const void* target, int64_t hw, int c, int64_t sn, int64_t sk, int64_t sp, int flags) {
  const int tk = rl_target_kind(flags);
  const uintptr_t t_align = (tk == TK_DENSE_U8 || tk == TK_INDEX_U8) ? 3 : 15;
  const bool quad = c <= 4 && (hw & 3) == 0 && (sn & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(target) & t_align) == 0;
  if (!quad) return LM_SCALAR;
  if (sp == 1 && (c == 1 || (sk & 3) == 0)) return LM_PLANAR4;
  if (sk == 1 && sp == c) return LM_CLAST4;
  return LM_SCALAR;
}

static int rl_check_common(const char* who, const void* logits, const void* target, const unsigned* region_bits, int n_labels, int nb,
                           int64_t hw, int c, int64_t sn, int64_t sk, int64_t sp, int flags) {
  MIA_CHECK_ARG(logits && target, "%s: null pointer", who);
  MIA_CHECK_ARG(nb > 0 && hw > 0 && hw < ((int64_t)1 << 31), "%s: bad shape", who);
  MIA_CHECK_ARG(c >= 1 && c <= LOSS_MAXK, "%s: c=%d not in [1,%d]", who, c, LOSS_MAXK);
  MIA_CHECK_ARG(c > 1 || (flags & RL_DO_BG), "%s: one channel without MIA_REGLOSS_DO_BG leaves no Dice term", who);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0, "%s: negative strides", who);
  MIA_CHECK_ARG((flags & ~(RL_DO_BG | RL_BATCH | RL_IGNORE | RL_INDEX | RL_TARGET_U8)) == 0, "%s: unknown flag bits in %d", who, flags);
  if (flags & RL_INDEX) MIA_CHECK_ARG(region_bits && n_labels > 0, "%s: the index form needs region_bits and n_labels > 0", who);
  return MIA_OK;
}

#define RL_LAUNCH_TK(KERNEL, NC, LM, ...)                                                                              \
  switch (tk) {                                                                                                        \
    case TK_DENSE_U8: hipLaunchKernelGGL((KERNEL<NC, LM, TK_DENSE_U8>), grid, blk, 0, st, __VA_ARGS__); break;         \
    case TK_DENSE_F32: hipLaunchKernelGGL((KERNEL<NC, LM, TK_DENSE_F32>), grid, blk, 0, st, __VA_ARGS__); break;       \
    case TK_INDEX_U8: hipLaunchKernelGGL((KERNEL<NC, LM, TK_INDEX_U8>), grid, blk, 0, st, __VA_ARGS__); break;         \
    default: hipLaunchKernelGGL((KERNEL<NC, LM, TK_INDEX_I64>), grid, blk, 0, st, __VA_ARGS__); break;                 \
  }
#define RL_LAUNCH_LM(KERNEL, NC, ...)                                                      \
  if (lm == LM_PLANAR4) { RL_LAUNCH_TK(KERNEL, NC, LM_PLANAR4, __VA_ARGS__) }              \
  else { RL_LAUNCH_TK(KERNEL, NC, LM_CLAST4, __VA_ARGS__) }
#define RL_LAUNCH(KERNEL, ...)                                                             \
  if (lm == LM_SCALAR) { RL_LAUNCH_TK(KERNEL, LOSS_MAXK, LM_SCALAR, __VA_ARGS__) }           \
  else if (c == 1) { RL_LAUNCH_LM(KERNEL, 1, __VA_ARGS__) }                                \
  else if (c == 2) { RL_LAUNCH_LM(KERNEL, 2, __VA_ARGS__) }                                \
  else if (c == 3) { RL_LAUNCH_LM(KERNEL, 3, __VA_ARGS__) }                                \
  else { RL_LAUNCH_LM(KERNEL, 4, __VA_ARGS__) }

static size_t rl_slices_words(int nb, int c, int slabs) {
  const size_t w = (size_t)nb * slabs * (6 * c + 2);
  return (w + 1) & ~(size_t)1;  // the doubles behind the slices stay 8-byte aligned
}

extern "C" int mia_region_loss_workspace(int nb, int c, int slabs) {
  if (nb <= 0 || c <= 0 || slabs <= 0) return 0;
  return (int)(rl_slices_words(nb, c, slabs) + (size_t)nb * c * 6);
}

extern "C" int mia_region_loss_fwd(const float* logits, const void* target, const unsigned* region_bits, int n_labels,
                                   const float* pos_weight, int nb, int64_t hw, int c, int64_t sn, int64_t sk, int64_t sp, int flags,
                                   int64_t ignore_label, float smooth, float dice_w, float ce_w, int slabs, float* workspace,
                                   float* coef, float* out, int64_t* counts, int* bad_label, void* stream) {
  const int rc = rl_check_common("mia_region_loss_fwd", logits, target, region_bits, n_labels, nb, hw, c, sn, sk, sp, flags);
  if (rc != MIA_OK) return rc;
  MIA_CHECK_ARG(workspace && coef && out && counts && bad_label, "mia_region_loss_fwd: null pointer");
  MIA_CHECK_ARG(slabs > 0 && (int64_t)nb * slabs <= 0x7fffffffLL, "mia_region_loss_fwd: bad slab count %d", slabs);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mia_region_loss_fwd: workspace must be 8-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  const RlTarget tg = rl_make_target(target, region_bits, n_labels, c, flags, ignore_label);
  const int tk = rl_target_kind(flags), lm = rl_logits_mode(logits, target, hw, c, sn, sk, sp, flags);
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  RL_LAUNCH(region_loss_fwd_kernel, logits, tg, pos_weight, hw, c, g, slabs, workspace, bad_label)
  double* tot = reinterpret_cast<double*>(workspace + rl_slices_words(nb, c, slabs));
  hipLaunchKernelGGL(region_loss_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, tot, nb, slabs, c, flags, hw, smooth, dice_w,
                     ce_w, coef, out, reinterpret_cast<long long*>(counts), bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_region_loss_bwd(const float* logits, const void* target, const unsigned* region_bits, int n_labels,
                                   const float* pos_weight, const float* coef, const float* grad_out, float* dlogits, int nb,
                                   int64_t hw, int c, int64_t sn, int64_t sk, int64_t sp, int64_t gsn, int64_t gsk, int64_t gsp,
                                   int flags, int64_t ignore_label, void* stream) {
  const int rc = rl_check_common("mia_region_loss_bwd", logits, target, region_bits, n_labels, nb, hw, c, sn, sk, sp, flags);
  if (rc != MIA_OK) return rc;
  MIA_CHECK_ARG(coef && dlogits, "mia_region_loss_bwd: null pointer");
  MIA_CHECK_ARG(gsn >= 0 && gsk >= 0 && gsp >= 0, "mia_region_loss_bwd: negative strides");
  MIA_CHECK_ARG(nb <= 65535, "mia_region_loss_bwd: nb=%d images are more than one launch takes", nb);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  const RlTarget tg = rl_make_target(target, region_bits, n_labels, c, flags, ignore_label);
  const int tk = rl_target_kind(flags);
  int lm = rl_logits_mode(logits, target, hw, c, sn, sk, sp, flags);
  // the gradient is written with the access width of the logits only where it has their layout and alignment
  if (lm != LM_SCALAR && !(rl_logits_mode(dlogits, target, hw, c, gsn, gsk, gsp, flags) == lm)) lm = LM_SCALAR;
  const int64_t nq = (hw + 3) >> 2, want = (nq + 255) / 256;
  const dim3 grid((unsigned)(want < 2048 ? want : 2048), (unsigned)nb), blk(256);
  RL_LAUNCH(region_loss_bwd_kernel, logits, tg, pos_weight, coef, grad_out, dlogits, nb, hw, c, g, go)
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
