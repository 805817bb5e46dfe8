// Virtual adversarial training (VAT: Miyato et al., TPAMI 2018) on the GPU (gfx950): the KL distance between two logits tensors and
// the three streaming pieces of the power iteration.
//   p = softmax(zt) (the target: no gradient), log q = z - logsumexp(z), log p likewise
//   L = coef * sum_pix sum_k p_k (log p_k - log q_k),  coef = 1 / den;  a term with p_k == 0 contributes 0 (saturated logits stay finite)
//   dL/dz_j = coef (q_j - p_j)
// The caller passes den: nb * hw for a per-pixel mean, nb for the published code's "batchmean".  The weight is read at run time from
// dyn_dev = {weight, ...} (NULL = 1), as in mia_consistency_fwd, so a captured step follows its ramp.
//   kl_fwd_kernel       block (image, slab of pixels): streams z and zt by their own (sn, sk, sp) strides; both log-soft-maxes in
//                       double per pixel; the block's sum leaves as a (hi, lo) float pair (LossBlockSums, loss_wave_pair)
//   kl_finalize_kernel  one block: the pairs in a fixed order in double; out = {weight L, L, weight}, coef[0] = 1 / den
//   kl_bwd_kernel       one streaming pass: z and zt in, dz out by its own strides
// Layout classes and their 16-byte loads / stores are pixel_stream.h's (planar, channels-last, scalar; batch slices).
//   vat_noise_kernel    u ~ U[-0.5, 0.5) from Philox4x32-10 (the generator of mia_dropout_mask, pack.hip): element i of the flat buffer
//                       is word i & 3 of the counter (i >> 2, offset) under key `seed`, so it depends on (seed, offset, i) alone
//   sumsq_kernel        per-sample sum of squares in double: block (sample, slab) partial pairs, then one block adds each sample's
//                       pairs in slab order and rounds once
//   vat_perturb_kernel  out = x + s (gscale g) / (gscale sqrt(sumsq[n]) + 1e-8) in double, rounded once; s = *scale_dev when given.
//                       g == 0 gives out = x.  16-byte accesses over the body when the three buffers are 16-byte aligned, scalar tail.
// No float atomics anywhere: bit-identical from run to run; nothing synchronises with the host.
#include "pixel_stream.h"

// log-soft-max and soft-max of one pixel in double: z - max is exact in double, exp and log are the double-precision ones.
// No contraction here or where p and q meet: with `p * inv - pt` fused into one fma for one operand and not for the other, equal
// logits would give a gradient of 1e-19 instead of exactly 0.
template <int K1>
__device__ __forceinline__ void kl_logsoftmax(const float (&v)[K1], double (&p)[K1], double (&lp)[K1]) {
#pragma clang fp contract(off)
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) mx = fmaxf(mx, v[k]);
  double se = 0.0;
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    lp[k] = (double)v[k] - (double)mx;
    p[k] = exp(lp[k]);
    se += p[k];
  }
  const double inv = 1.0 / se, lse = log(se);
#pragma unroll
  for (int k = 0; k < K1; ++k) { p[k] *= inv; lp[k] -= lse; }
}

// block (image, slab of `per` pixels; per % PX == 0).  ws [nb * slabs][2] = (hi, lo) of the block's sum
template <int K1, int SM, int TM>
__global__ __launch_bounds__(256) void kl_fwd_kernel(const float* __restrict__ z, const float* __restrict__ zt, int64_t hw, LossGeom gs,
                                                     LossGeom gt, int slabs, int64_t per, float* __restrict__ ws) {
  constexpr int PX = CS_PX(SM);
  static_assert(CS_PX(SM) == CS_PX(TM), "both tensors take the same number of pixels per thread");
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* is = z + b * gs.sn;
  const float* it = zt + b * gt.sn;
  double acc = 0.0;
  for (int64_t p = r0 + (int64_t)threadIdx.x * PX; p < r1; p += 256 * PX) {
    float a[PX][K1], t[PX][K1];
    cs_load<K1, SM>(is, p, gs, a);
    cs_load<K1, TM>(it, p, gt, t);
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      double q[K1], lq[K1], pt[K1], lpt[K1];
      kl_logsoftmax<K1>(a[i], q, lq);
      kl_logsoftmax<K1>(t[i], pt, lpt);
      double d = 0.0;
#pragma unroll
      for (int k = 0; k < K1; ++k) {
#pragma clang fp contract(off)
        d += pt[k] > 0.0 ? pt[k] * (lpt[k] - lq[k]) : 0.0;
      }
      acc += d;
    }
  }
  float part[2];
  loss_wave_pair(acc, threadIdx.x & 63, part);
  auto red = loss_block_sums<2, 0>();
  red.put(0, part);
  __syncthreads();
  if (threadIdx.x < 2) ws[(size_t)blockIdx.x * 2 + threadIdx.x] = red.sum_f(threadIdx.x);
}

__global__ void kl_finalize_kernel(const float* __restrict__ ws, int nparts, double den, const float* __restrict__ dyn,
                                   float* __restrict__ coef, float* __restrict__ out) {
  const LossTotals tot = loss_totals<1, 0>(ws, nullptr, nparts, 1);
  __shared__ float res[3];
  if (threadIdx.x == 0) {
    const float wt = dyn ? dyn[0] : 1.f;
    const double l = tot.f[0] / den;
    res[0] = (float)((double)wt * l);
    res[1] = (float)l;
    res[2] = wt;
    coef[0] = (float)(1.0 / den);
  }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = res[threadIdx.x];
}

template <int K1, int SM, int TM>
__global__ __launch_bounds__(256) void kl_bwd_kernel(const float* __restrict__ z, const float* __restrict__ zt, const float* __restrict__ coef,
                                                     const float* __restrict__ dyn, const float* __restrict__ gout, float* __restrict__ dz,
                                                     int64_t hw, int64_t total, LossGeom gs, LossGeom gt, LossGeom go) {
  constexpr int PX = CS_PX(SM);
  static_assert(CS_PX(SM) == CS_PX(TM), "both tensors take the same number of pixels per thread");
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per = hw / PX, b = idx / per, p = (idx - b * per) * PX;
  const double sc = (double)(gout ? gout[0] : 1.f) * (double)(dyn ? dyn[0] : 1.f) * (double)coef[0];
  float a[PX][K1], t[PX][K1], g[PX][K1];
  cs_load<K1, SM>(z + b * gs.sn, p, gs, a);
  cs_load<K1, TM>(zt + b * gt.sn, p, gt, t);
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    double q[K1], lq[K1], pt[K1], lpt[K1];
    kl_logsoftmax<K1>(a[i], q, lq);
    kl_logsoftmax<K1>(t[i], pt, lpt);
#pragma unroll
    for (int k = 0; k < K1; ++k) {
#pragma clang fp contract(off)
      g[i][k] = (float)(sc * (q[k] - pt[k]));
    }
  }
  cs_store<K1, SM>(dz + b * go.sn, p, go, g);
}

template <int K1, int SM, int TM>
static void kl_launch_fwd(hipStream_t st, const float* z, const float* zt, int nb, int64_t hw, const LossGeom& gs, const LossGeom& gt,
                          int slabs, float* ws) {
  constexpr int PX = CS_PX(SM);
  const int64_t per = ceil_div64(hw / PX, slabs) * PX;  // hw % PX == 0 on the four-pixel path
  hipLaunchKernelGGL((kl_fwd_kernel<K1, SM, TM>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, z, zt, hw, gs, gt, slabs, per, ws);
}

template <int K1, int SM, int TM>
static void kl_launch_bwd(hipStream_t st, const float* z, const float* zt, const float* coef, const float* dyn, const float* gout,
                          float* dz, int nb, int64_t hw, const LossGeom& gs, const LossGeom& gt, const LossGeom& go) {
  const int64_t total = (int64_t)nb * (hw / CS_PX(SM));
  hipLaunchKernelGGL((kl_bwd_kernel<K1, SM, TM>), dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, z, zt, coef, dyn, gout, dz, hw,
                     total, gs, gt, go);
}

extern "C" int mia_kl_workspace(int nb, int slabs) {
  if (nb <= 0 || slabs <= 0 || (int64_t)nb * slabs * 2 > 0x7fffffff) return -1;
  return nb * slabs * 2;
}

extern "C" int mia_kl_fwd(const float* z, const float* zt, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t sn, int64_t sk,
                          int64_t sp, int64_t tsn, int64_t tsk, int64_t tsp, double den, int slabs, float* workspace, float* coef,
                          float* out, void* stream) {
  MIA_CHECK_ARG(z && zt && workspace && coef && out, "mia_kl_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0 && (int64_t)nb * slabs * 2 <= 0x7fffffff && (int64_t)nb * hw < ((int64_t)1 << 31),
                "mia_kl_fwd: bad shape nb=%d hw=%lld slabs=%d", nb, (long long)hw, slabs);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_kl_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0 && tsn >= 0 && tsk >= 0 && tsp >= 0, "mia_kl_fwd: negative strides");
  MIA_CHECK_ARG(den > 0.0 && den < (double)__builtin_inff(), "mia_kl_fwd: den=%g must be finite and > 0", den);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom gs{sn, sk, sp}, gt{tsn, tsk, tsp};
  int sm = cs_mode(z, gs, k1), tm = cs_mode(zt, gt, k1);
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR) sm = tm = CS_SCALAR;
  CS_DISPATCH(kl_launch_fwd, st, z, zt, nb, hw, gs, gt, slabs, workspace);
  hipLaunchKernelGGL(kl_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, nb * slabs, den, dyn_dev, coef, out);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_kl_bwd(const float* z, const float* zt, const float* coef, const float* dyn_dev, const float* grad_out, float* dz,
                          int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp, int64_t tsn, int64_t tsk, int64_t tsp,
                          int64_t gsn, int64_t gsk, int64_t gsp, void* stream) {
  MIA_CHECK_ARG(z && zt && coef && dz, "mia_kl_bwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && (int64_t)nb * hw < ((int64_t)1 << 31), "mia_kl_bwd: bad shape nb=%d hw=%lld", nb, (long long)hw);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_kl_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0 && tsn >= 0 && tsk >= 0 && tsp >= 0 && gsn >= 0 && gsk >= 0 && gsp >= 0,
                "mia_kl_bwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom gs{sn, sk, sp}, gt{tsn, tsk, tsp}, go{gsn, gsk, gsp};
  int sm = cs_mode(z, gs, k1), tm = cs_mode(zt, gt, k1);
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || cs_mode(dz, go, k1) != sm) sm = tm = CS_SCALAR;  // the gradient in z's layout class
  CS_DISPATCH(kl_launch_bwd, st, z, zt, coef, dyn_dev, grad_out, dz, nb, hw, gs, gt, go);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------ noise
__device__ __forceinline__ void vat_philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
  const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
  const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
  c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

__global__ __launch_bounds__(256) void vat_noise_kernel(float* __restrict__ u, int64_t n, unsigned long long seed, unsigned long long offset) {
  const int64_t quads = (n + 3) / 4;
  for (int64_t qd = (int64_t)blockIdx.x * 256 + threadIdx.x; qd < quads; qd += (int64_t)gridDim.x * 256) {
    unsigned c0 = (unsigned)qd, c1 = (unsigned)(qd >> 32), c2 = (unsigned)offset, c3 = (unsigned)(offset >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) { vat_philox_round(c0, c1, c2, c3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const unsigned c[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t i = qd * 4 + e;
      if (i < n) u[i] = (float)(c[e] >> 8) * (1.f / 16777216.f) - 0.5f;  // 24 bits: every value is exact, in [-0.5, 0.5)
    }
  }
}

extern "C" int mia_vat_noise(float* u, int nb, int64_t per, uint64_t seed, uint64_t offset, void* stream) {
  MIA_CHECK_ARG(u && nb > 0 && per > 0, "mia_vat_noise: bad arguments (nb=%d per=%lld)", nb, (long long)per);
  MIA_CHECK_ARG(per <= ((int64_t)1 << 40) / nb, "mia_vat_noise: nb * per is too large");
  const int64_t n = (int64_t)nb * per, quads = (n + 3) / 4;
  const int blocks = (int)((quads + 255) / 256 < 4096 ? (quads + 255) / 256 : 4096);
  hipLaunchKernelGGL(vat_noise_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), u, n, (unsigned long long)seed,
                     (unsigned long long)offset);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------ per-sample sum of squares
static int sumsq_slabs(int64_t per) {
  const int64_t s = per / 4096;
  return s < 1 ? 1 : (s > 64 ? 64 : (int)s);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, int64_t per, int slabs, float* __restrict__ ws) {
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t chunk = (per + slabs - 1) / slabs, r0 = s * chunk, r1 = r0 + chunk < per ? r0 + chunk : per;
  const float* xs = x + (int64_t)b * per;
  double acc = 0.0;
  for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) { const double v = (double)xs[i]; acc += v * v; }
  float part[2];
  loss_wave_pair(acc, threadIdx.x & 63, part);
  auto red = loss_block_sums<2, 0>();
  red.put(0, part);
  __syncthreads();
  if (threadIdx.x < 2) ws[(size_t)blockIdx.x * 2 + threadIdx.x] = red.sum_f(threadIdx.x);
}

__global__ __launch_bounds__(256) void sumsq_finalize_kernel(const float* __restrict__ ws, int nb, int slabs, float* __restrict__ out) {
  for (int b = threadIdx.x; b < nb; b += 256) {
    double s = 0.0;
    for (int i = 0; i < slabs; ++i) s += (double)ws[((size_t)b * slabs + i) * 2] + (double)ws[((size_t)b * slabs + i) * 2 + 1];
    out[b] = (float)s;
  }
}

extern "C" int mia_sample_sumsq_workspace(int nb, int64_t per) {
  if (nb <= 0 || per <= 0 || (int64_t)nb * sumsq_slabs(per) * 2 > 0x7fffffff) return -1;
  return nb * sumsq_slabs(per) * 2;
}

extern "C" int mia_sample_sumsq(const float* x, int nb, int64_t per, float* workspace, float* out, void* stream) {
  MIA_CHECK_ARG(x && workspace && out, "mia_sample_sumsq: null pointer");
  MIA_CHECK_ARG(nb > 0 && per > 0 && (int64_t)nb * sumsq_slabs(per) * 2 <= 0x7fffffff, "mia_sample_sumsq: bad shape nb=%d per=%lld", nb,
                (long long)per);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = sumsq_slabs(per);
  hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)(nb * slabs)), dim3(256), 0, st, x, per, slabs, workspace);
  hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, nb, slabs, out);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------ perturbation
__device__ __forceinline__ float vat_perturb_one(float x, float g, float ss, double gs, double s) {
  return (float)((double)x + s * (gs * (double)g) / (gs * sqrt((double)ss) + 1e-8));
}

// nvec 16-byte units over the flat buffers from element 0 (nvec = 0 when a buffer is not 16-byte aligned), then the other
// `total - 4 nvec` elements one at a time
__global__ __launch_bounds__(256) void vat_perturb_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                          const float* __restrict__ sumsq, float gscale, float scale,
                                                          const float* __restrict__ scale_dev, float* __restrict__ out, int64_t per,
                                                          int64_t nvec, int64_t total) {
  const double s = (double)(scale_dev ? scale_dev[0] : scale), gs = (double)gscale;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < nvec) {
    const f32x4 xv = reinterpret_cast<const f32x4*>(x)[idx], gv = reinterpret_cast<const f32x4*>(g)[idx];
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = vat_perturb_one(xv[i], gv[i], sumsq[(idx * 4 + i) / per], gs, s);
    reinterpret_cast<f32x4*>(out)[idx] = r;
    store_data_pad();
  }
  for (int64_t j = 4 * nvec + idx; j < total; j += (int64_t)gridDim.x * 256) out[j] = vat_perturb_one(x[j], g[j], sumsq[j / per], gs, s);
}

extern "C" int mia_vat_perturb(const float* x, const float* g, const float* sumsq, float gscale, float scale, const float* scale_dev,
                               float* out, int nb, int64_t per, void* stream) {
  MIA_CHECK_ARG(x && g && sumsq && out, "mia_vat_perturb: null pointer");
  MIA_CHECK_ARG(nb > 0 && per > 0 && per <= ((int64_t)1 << 38) / nb, "mia_vat_perturb: bad shape nb=%d per=%lld", nb, (long long)per);
  MIA_CHECK_ARG(gscale > 0.f && gscale < __builtin_inff(), "mia_vat_perturb: gscale=%g must be finite and > 0", (double)gscale);
  const int64_t total = (int64_t)nb * per;
  const bool al = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t nvec = al ? total / 4 : 0, tail = total - 4 * nvec;
  const int64_t blocks = ceil_div64(nvec > tail ? nvec : tail, 256);
  hipLaunchKernelGGL(vat_perturb_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), x, g, sumsq, gscale, scale,
                     scale_dev, out, per, nvec, total);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
