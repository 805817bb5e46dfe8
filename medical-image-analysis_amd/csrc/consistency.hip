// Mean-teacher consistency on the GPU (gfx950): the softmax-MSE loss between a student's and a teacher's logits (Tarvainen & Valpola
// 2017), its uncertainty-masked form (UA-MT, Yu et al., MICCAI 2019) and the teacher's exponential moving average.
//   ps = softmax(zs), pt = softmax(zt), e_k = ps_k - pt_k, d(b,p) = sum_k e_k^2
//   plain:   L = sum_{b,p} d / (nb * k1 * hw)                                        = torch.mean((ps - pt)**2)
//   masked:  u = -sum_k pbar_k log(pbar_k + 1e-6), keep = (u < threshold), n_keep = sum keep,
//            L = sum keep d / (den_scale * n_keep + 1e-16)                           n_keep = 0: L = 0 and a zero gradient, no NaN
//   dL/dzs_j = coef keep 2 ps_j (e_j - sum_k ps_k e_k),  coef = 1 / denominator;  the teacher and pbar get no gradient
// weight and threshold are read at run time from dyn_dev = {weight, threshold} (NULL = weight 1, plain form only), so a captured step
// follows the ramps without a re-capture (the idea of mia_boundary_loss_fwd's weight_dev).
//   cons_fwd_kernel       block (image, slab of pixels): streams zs and zt by their own (sn, sk, sp) strides and pbar (planar); the
//                         entropy in fp32 (eight terms of magnitude <= 0.37: ~1e-7, the tests allow 1e-5 around the threshold), the
//                         two soft-maxes in double per pixel (boundary.hip's form: fp32 exponentials with the rounding error of
//                         `z - max` carried along); writes the byte map keep[nb][hw] and per-block partials: the sum as a (hi, lo)
//                         float pair and the kept count as an int, through LossBlockSums
//   cons_finalize_kernel  one block: the partials in a fixed order in double / int64, the denominator, out, coef, n_keep
//   cons_bwd_kernel       one streaming pass: zs, zt and the byte map in, dzs out -- both directions agree on every pixel by
//                         construction, pbar is not read again
// Planar (sp == 1) and channels-last (sk == 1, sp == k1) tensors take four pixels per thread with 16-byte accesses when hw % 4 == 0
// and pointers / strides are 16-byte aligned (the rule of mia_softmax_accum); student and teacher may differ in layout; anything else
// takes one pixel per thread.  No float atomics: bit-identical from run to run; an image's keep map does not depend on the rest of
// the batch; nothing synchronises with the host.
//   ema_kernel            teacher = alpha teacher + (1 - alpha) student over flat fp32 buffers, in double, rounded once; 16-byte
//                         accesses over the co-aligned body, scalar head and tail; alpha == 0 copies the student's bits
#include "pixel_stream.h"  // the layout classes, cs_load / cs_store, cs_softmax and the dispatch, shared with cps.hip

// u < threshold with u = -sum_k pbar_k log(pbar_k + 1e-6) in fp32 (a NaN in pbar or in the threshold keeps nothing)
template <int K1>
__device__ __forceinline__ bool cs_keep(const float (&pb)[K1], float thr) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) s = __builtin_fmaf(pb[k], logf(pb[k] + 1e-6f), s);
  return -s < thr;
}

// block (image, slab of `per` pixels; per % PX == 0).  ws [nb * slabs][2] = (hi, lo) of the block's sum of keep * d;
// wsn [nb * slabs] = its kept pixels.  pbar == NULL: the plain form, every pixel is kept.  keep may be NULL only then.
template <int K1, int SM, int TM>
__global__ __launch_bounds__(256) void cons_fwd_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                                                       const float* __restrict__ pbar, const float* __restrict__ dyn, int64_t hw,
                                                       LossGeom gs, LossGeom gt, int slabs, int64_t per, float* __restrict__ ws,
                                                       int* __restrict__ wsn, unsigned char* __restrict__ keep) {
  constexpr int PX = CS_PX(SM);
  static_assert(CS_PX(SM) == CS_PX(TM), "student and teacher take the same number of pixels per thread");
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* is = zs + b * gs.sn;
  const float* it = zt + b * gt.sn;
  const float* ip = pbar ? pbar + (int64_t)b * K1 * hw : nullptr;
  const float thr = pbar ? dyn[1] : 0.f;
  double acc = 0.0;
  int cnt = 0;
  for (int64_t p = r0 + (int64_t)threadIdx.x * PX; p < r1; p += 256 * PX) {
    float a[PX][K1], t[PX][K1];
    cs_load<K1, SM>(is, p, gs, a);
    cs_load<K1, TM>(it, p, gt, t);
    bool kp[PX];
#pragma unroll
    for (int i = 0; i < PX; ++i) kp[i] = true;
    if (ip) {
      float pb[PX][K1];
      cs_load<K1, PX == 4 ? CS_PLANAR4 : CS_SCALAR>(ip, p, LossGeom{0, hw, 1}, pb);
#pragma unroll
      for (int i = 0; i < PX; ++i) kp[i] = cs_keep<K1>(pb[i], thr);
    }
#pragma unroll
    for (int i = 0; i < PX; ++i)
      if (kp[i]) {
        double ps[K1], pt[K1];
        cs_softmax<K1>(a[i], ps);
        cs_softmax<K1>(t[i], pt);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < K1; ++k) { const double e = ps[k] - pt[k]; d += e * e; }
        acc += d;
        ++cnt;
      }
    if (keep) {
      unsigned char* kd = keep + (int64_t)b * hw + p;
      if (PX == 4)  // one 4-byte store; b * hw + p is a multiple of 4
        *reinterpret_cast<unsigned*>(kd) = (unsigned)kp[0] | (unsigned)kp[1] << 8 | (unsigned)kp[2] << 16 | (unsigned)kp[3] << 24;
      else
        kd[0] = (unsigned char)kp[0];
    }
  }
  float part[2];
  loss_split(acc, part);
  const int cpart[1] = {cnt};
  auto red = loss_block_sums<2, 1>();
  red.put(0, part, 0, cpart);
  __syncthreads();
  if (threadIdx.x < 2) ws[(size_t)blockIdx.x * 2 + threadIdx.x] = red.sum_f(threadIdx.x);
  if (threadIdx.x == 2) wsn[blockIdx.x] = red.sum_i(0);
}

// one block: out[0] = weight * L, out[1] = L, out[2] = weight; coef[0] = 1 / denominator; n_keep[0] = the kept pixels
__global__ void cons_finalize_kernel(const float* __restrict__ ws, const int* __restrict__ wsn, int nparts, int masked, double n_all,
                                     double den_scale, const float* __restrict__ dyn, float* __restrict__ coef,
                                     float* __restrict__ out, long long* __restrict__ n_keep) {
  const LossTotals tot = loss_totals<1, 1>(ws, wsn, nparts, 1);
  __shared__ float res[3];
  if (threadIdx.x == 0) {
    const double t = tot.f[0];
    const long long n = tot.n[0];
    const float wt = dyn ? dyn[0] : 1.f;
    const double den = masked ? den_scale * (double)n + 1e-16 : n_all;
    const double l = t / den;  // nothing kept: 0 / 1e-16 = 0
    res[0] = (float)((double)wt * l);
    res[1] = (float)l;
    res[2] = wt;
    coef[0] = (float)(1.0 / den);
    n_keep[0] = n;
  }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = res[threadIdx.x];  // one 4-byte store per lane
}

// a thread per group of PX pixels; the gradient has the student's layout class (its own strides) on the four-pixel path
template <int K1, int SM, int TM>
__global__ __launch_bounds__(256) void cons_bwd_kernel(const float* __restrict__ zs, const float* __restrict__ zt,
                                                       const unsigned char* __restrict__ keep, const float* __restrict__ coef,
                                                       const float* __restrict__ dyn, const float* __restrict__ gout,
                                                       float* __restrict__ dl, int64_t hw, int64_t total, LossGeom gs, LossGeom gt,
                                                       LossGeom go) {
  constexpr int PX = CS_PX(SM);
  static_assert(CS_PX(SM) == CS_PX(TM), "student and teacher take the same number of pixels per thread");
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per = hw / PX, b = idx / per, p = (idx - b * per) * PX;
  const double sc = 2.0 * (double)(gout ? gout[0] : 1.f) * (double)(dyn ? dyn[0] : 1.f) * (double)coef[0];
  float a[PX][K1], t[PX][K1], g[PX][K1];
  cs_load<K1, SM>(zs + b * gs.sn, p, gs, a);
  cs_load<K1, TM>(zt + b * gt.sn, p, gt, t);
  unsigned kbits = 0x01010101u;
  if (keep) {
    const unsigned char* kd = keep + b * hw + p;
    kbits = PX == 4 ? *reinterpret_cast<const unsigned*>(kd) : (unsigned)kd[0];
  }
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    if ((kbits >> (8 * i)) & 0xffu) {
      double ps[K1], pt[K1], e[K1];
      cs_softmax<K1>(a[i], ps);
      cs_softmax<K1>(t[i], pt);
      double dot = 0.0;
#pragma unroll
      for (int k = 0; k < K1; ++k) { e[k] = ps[k] - pt[k]; dot += ps[k] * e[k]; }
#pragma unroll
      for (int k = 0; k < K1; ++k) g[i][k] = (float)(sc * ps[k] * (e[k] - dot));
    } else {
#pragma unroll
      for (int k = 0; k < K1; ++k) g[i][k] = 0.f;  // a dropped pixel: exactly zero, whatever coef holds
    }
  }
  cs_store<K1, SM>(dl + b * go.sn, p, go, g);
}

template <int K1, int SM, int TM>
static void cs_launch_fwd(hipStream_t st, const float* zs, const float* zt, const float* pbar, const float* dyn, int nb, int64_t hw,
                          const LossGeom& gs, const LossGeom& gt, int slabs, float* ws, int* wsn, unsigned char* keep) {
  constexpr int PX = CS_PX(SM);
  const int64_t per = ceil_div64(hw / PX, slabs) * PX;  // hw % PX == 0 on the four-pixel path
  hipLaunchKernelGGL((cons_fwd_kernel<K1, SM, TM>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, zs, zt, pbar, dyn, hw, gs, gt, slabs,
                     per, ws, wsn, keep);
}

template <int K1, int SM, int TM>
static void cs_launch_bwd(hipStream_t st, const float* zs, const float* zt, const unsigned char* keep, const float* coef,
                          const float* dyn, const float* gout, float* dl, int nb, int64_t hw, const LossGeom& gs, const LossGeom& gt,
                          const LossGeom& go) {
  const int64_t total = (int64_t)nb * (hw / CS_PX(SM));
  hipLaunchKernelGGL((cons_bwd_kernel<K1, SM, TM>), dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, zs, zt, keep, coef, dyn,
                     gout, dl, hw, total, gs, gt, go);
}

extern "C" int mia_consistency_workspace(int nb, int slabs) {
  if (nb <= 0 || slabs <= 0 || (int64_t)nb * slabs * 3 > 0x7fffffff) return -1;
  return nb * slabs * 3;
}

extern "C" int mia_consistency_fwd(const float* zs, const float* zt, const float* prob_mean, const float* dyn_dev, int nb, int64_t hw,
                                   int k1, int64_t sn, int64_t sk, int64_t sp, int64_t tsn, int64_t tsk, int64_t tsp, float den_scale,
                                   int slabs, float* workspace, unsigned char* keep, float* coef, float* out, long long* n_keep,
                                   void* stream) {
  MIA_CHECK_ARG(zs && zt && workspace && coef && out && n_keep, "mia_consistency_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0 && (int64_t)nb * slabs * 3 <= 0x7fffffff && (int64_t)nb * hw <= 0x7fffffff,
                "mia_consistency_fwd: bad shape nb=%d hw=%lld slabs=%d", nb, (long long)hw, slabs);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_consistency_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0 && tsn >= 0 && tsk >= 0 && tsp >= 0, "mia_consistency_fwd: negative strides");
  MIA_CHECK_ARG(!prob_mean || dyn_dev, "mia_consistency_fwd: prob_mean needs dyn_dev (the threshold is read from dyn_dev[1])");
  MIA_CHECK_ARG(!prob_mean || keep, "mia_consistency_fwd: prob_mean needs a keep map for the backward");
  MIA_CHECK_ARG(!prob_mean || (den_scale > 0.f && den_scale < __builtin_inff()), "mia_consistency_fwd: den_scale=%g must be finite and > 0",
                (double)den_scale);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom gs{sn, sk, sp}, gt{tsn, tsk, tsp};
  int sm = cs_mode(zs, gs, k1), tm = cs_mode(zt, gt, k1);
  // four pixels per thread: 16-byte units in both logits, in prob_mean and 4-byte units in the keep map
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || (prob_mean && !cs_al16(prob_mean)) || (keep && !cs_al16(keep)))
    sm = tm = CS_SCALAR;
  int* wsn = reinterpret_cast<int*>(workspace + (size_t)nb * slabs * 2);
  CS_DISPATCH(cs_launch_fwd, st, zs, zt, prob_mean, dyn_dev, nb, hw, gs, gt, slabs, workspace, wsn, keep);
  hipLaunchKernelGGL(cons_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, wsn, nb * slabs, prob_mean ? 1 : 0,
                     (double)nb * k1 * (double)hw, (double)den_scale, dyn_dev, coef, out, n_keep);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_consistency_bwd(const float* zs, const float* zt, const unsigned char* keep, const float* coef, const float* dyn_dev,
                                   const float* grad_out, float* dzs, int nb, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp,
                                   int64_t tsn, int64_t tsk, int64_t tsp, int64_t gsn, int64_t gsk, int64_t gsp, void* stream) {
  MIA_CHECK_ARG(zs && zt && coef && dzs, "mia_consistency_bwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && (int64_t)nb * hw <= 0x7fffffff, "mia_consistency_bwd: bad shape nb=%d hw=%lld", nb, (long long)hw);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_consistency_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0 && tsn >= 0 && tsk >= 0 && tsp >= 0 && gsn >= 0 && gsk >= 0 && gsp >= 0,
                "mia_consistency_bwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom gs{sn, sk, sp}, gt{tsn, tsk, tsp}, go{gsn, gsk, gsp};
  int sm = cs_mode(zs, gs, k1), tm = cs_mode(zt, gt, k1);
  // four pixels per thread: as the forward, and the gradient in the student's layout class
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || cs_mode(dzs, go, k1) != sm || (keep && !cs_al16(keep))) sm = tm = CS_SCALAR;
  CS_DISPATCH(cs_launch_bwd, st, zs, zt, keep, coef, dyn_dev, grad_out, dzs, nb, hw, gs, gt, go);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------ exponential moving average
// body: nvec 16-byte units from element `head` on (both buffers 16-byte aligned there); the other `nsc` elements -- the head, then the
// tail from element head + 4 * nvec on -- one at a time.  In double, rounded once: |error| <= 2^-24 |result|.
__device__ __forceinline__ float ema_one(float t, float s, float a) {
  return a == 0.f ? s : (float)((double)a * (double)t + (1.0 - (double)a) * (double)s);
}

__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ teacher, const float* __restrict__ student, int64_t head,
                                                  int64_t nvec, int64_t nsc, float alpha, const float* __restrict__ alpha_dev) {
  const float a = alpha_dev ? alpha_dev[0] : alpha;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < nvec) {
    f32x4* tp = reinterpret_cast<f32x4*>(teacher + head) + idx;
    const f32x4 s = reinterpret_cast<const f32x4*>(student + head)[idx];
    const f32x4 t = *tp;
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = ema_one(t[i], s[i], a);
    *tp = r;
  }
  for (int64_t j = idx; j < nsc; j += (int64_t)gridDim.x * 256) {
    const int64_t i = j < head ? j : j + 4 * nvec;
    teacher[i] = ema_one(teacher[i], student[i], a);
  }
}

extern "C" int mia_ema_update(float* teacher, const float* student, int64_t n, float alpha, const float* alpha_dev, void* stream) {
  MIA_CHECK_ARG(teacher && student, "mia_ema_update: null pointer");
  MIA_CHECK_ARG(n > 0, "mia_ema_update: n=%lld must be positive", (long long)n);
  MIA_CHECK_ARG(alpha_dev || (alpha >= 0.f && alpha <= 1.f), "mia_ema_update: alpha=%g not in [0,1]", (double)alpha);
  const uintptr_t ta = reinterpret_cast<uintptr_t>(teacher), sa = reinterpret_cast<uintptr_t>(student);
  MIA_CHECK_ARG(ta % 4 == 0 && sa % 4 == 0, "mia_ema_update: buffers must be 4-byte aligned");
  int64_t head = 0, nvec = 0;
  if ((ta & 15) == (sa & 15)) {  // co-aligned: 16-byte units from the first aligned element on
    head = (int64_t)(((16 - (ta & 15)) & 15) / 4);
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  const int64_t nsc = n - 4 * nvec;
  int64_t blocks = ceil_div64(nvec > nsc ? nvec : nsc, 256);
  MIA_CHECK_ARG(blocks <= 0x7fffffffLL, "mia_ema_update: n=%lld is too large", (long long)n);
  hipLaunchKernelGGL(ema_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), teacher, student, head, nvec, nsc,
                     alpha, alpha_dev);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
