// Prediction path (gfx950): the ensemble reduction and the mask clean-up behind the models.
//
// * mia_softmax_accum: `P = P + seg.softmax(1)` over the fold models and the final `argmax` (reference
//   entry/fugc2025/predict.py:144-161, :55-57) as ONE streaming pass per model: prob_sum = (first ? 0 : prob_sum) + weight * softmax,
//   and the arg-max of the updated sum where `pred` is given.  Every pixel is owned by one thread, models are accumulated in call
//   order, no atomics: bit-identical from run to run.  HBM-bound (4*K1 bytes of logits + 4*K1 read + 4*K1 written per pixel), so
//   a thread takes four pixels with 16-byte accesses where layout and alignment allow (planar NCHW, or the head's channels-last
//   layout where four pixels are K1 consecutive 16-byte units); any other strides take the one-pixel scalar path.
// * mia_mask_denoise: `denoise_one_mask` (predict.py:55-90 = models/unet/unet_processor.py:72-160) for a batch of label maps in
//   one launch.  One workgroup per 64 x 64 output tile; both binary masks (`in > 0`, `in == 1`) of the tile plus a halo of
//   2 * (dilate + erode) + 3 pixels live bit-packed in LDS, one 192-bit row (three 64-bit words) per mask row, and every stage --
//   dilate, erode, erode, dilate on the zero-padded domain, crop, reflect -- is a vertical OR / AND over rows followed by a
//   log-step shift-OR inside the row.  The 8.8 fixed-point Gaussian and its threshold are integer sums over 7 x 7 bits.  The
//   result depends on 2 bits per pixel: the kernel reads 8 bytes (x ~3 for the halo, mostly from cache) and writes 8 per pixel.
// * mia_window_accum / mia_window_finalize: tiled prediction with overlap (the `patch_size` / `stride` fields of the reference's
//   trainer configs, al_trainer.py:112,167,253, which nothing there reads).  One streaming pass per (model, mirror combination,
//   window) adds importance * weight * softmax into the window's region of a full-size canvas, reading the logits mirrored where the
//   input was; one pass at the end takes the arg-max of the raw canvas and scales it by the separable 1 / coverage.  A thread owns a
//   canvas pixel for a whole pass, windows are separate launches in stream order: no atomics, bit-identical from run to run.  Per
//   window pixel 4*K1 bytes of logits and 4*K1 read + 4*K1 written of canvas, the canvas part normally from the Infinity Cache.
#include "common.h"

#define PMAXK 8

// ------------------------------------------------------------------------------------------------ ensemble reduction
enum { SA_SCALAR = 0, SA_PLANAR4 = 1, SA_CLAST4 = 2 };

// weight * softmax of K1 logits in v[], in place.  __expf is v_exp_f32 on x * log2(e): for x <= 0 the absolute error is below
// (|x| * 2^-24 + 2 ulp) * e^x < 1e-7, so every probability stays within ~2e-7 of the exact one.
template <int K1> __device__ __forceinline__ void softmax_w(float (&v)[K1], float weight) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) mx = fmaxf(mx, v[k]);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) { v[k] = __expf(v[k] - mx); sum += v[k]; }
  const float sc = weight / sum;
#pragma unroll
  for (int k = 0; k < K1; ++k) v[k] *= sc;
}

template <int K1> __device__ __forceinline__ long long argmax_first(const float (&v)[K1]) {
  float best = v[0];
  int arg = 0;
#pragma unroll
  for (int k = 1; k < K1; ++k)
    if (v[k] > best) { best = v[k]; arg = k; }  // strict: ties go to the lowest class (torch.argmax)
  return arg;
}

template <int K1, int MODE>
__global__ void __launch_bounds__(256) softmax_accum_kernel(const float* __restrict__ logits, float* __restrict__ prob_sum,
                                                            long long* __restrict__ pred, int64_t hw, int64_t total, int64_t sn,
                                                            int64_t sk, int64_t sp, float weight, int first) {
  constexpr int PX = MODE == SA_SCALAR ? 1 : 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one group of PX pixels
  if (idx >= total) return;
  const int64_t per = hw / PX, b = idx / per, p = (idx - b * per) * PX;
  const float* src = logits + b * sn;
  float v[PX][K1];
  if (MODE == SA_PLANAR4) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + k * sk + p);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i][k] = t[i];
    }
  } else if (MODE == SA_CLAST4) {  // four pixels = K1 consecutive 16-byte units
    float flat[4 * K1];
#pragma unroll
    for (int u = 0; u < K1; ++u) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + p * K1 + 4 * u);
#pragma unroll
      for (int i = 0; i < 4; ++i) flat[4 * u + i] = t[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < K1; ++k) v[i][k] = flat[i * K1 + k];
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) v[0][k] = src[p * sp + k * sk];
  }
#pragma unroll
  for (int i = 0; i < PX; ++i) softmax_w<K1>(v[i], weight);
  float* acc = prob_sum ? prob_sum + (b * K1) * hw + p : nullptr;
  if (acc && !first) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (PX == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(acc + k * hw);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i][k] += t[i];
      } else {
        v[0][k] += acc[k * hw];
      }
    }
  }
  if (acc) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (PX == 4) {
        f32x4 t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = v[i][k];
        *reinterpret_cast<f32x4*>(acc + k * hw) = t;
      } else {
        acc[k * hw] = v[0][k];
      }
    }
  }
  if (pred) {
    long long* dst = pred + b * hw + p;
    if (PX == 4) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      *reinterpret_cast<i64x2*>(dst) = i64x2{argmax_first<K1>(v[0]), argmax_first<K1>(v[1])};
      *reinterpret_cast<i64x2*>(dst + 2) = i64x2{argmax_first<K1>(v[2]), argmax_first<K1>(v[3])};
    } else {
      dst[0] = argmax_first<K1>(v[0]);
    }
  }
}

template <int K1>
static void launch_softmax_accum(int mode, int64_t groups, hipStream_t st, const float* logits, float* prob_sum, long long* pred,
                                 int64_t hw, int64_t sn, int64_t sk, int64_t sp, float weight, int first) {
  const dim3 grid((unsigned)ceil_div64(groups, 256)), block(256);
  if (mode == SA_PLANAR4)
    hipLaunchKernelGGL((softmax_accum_kernel<K1, SA_PLANAR4>), grid, block, 0, st, logits, prob_sum, pred, hw, groups, sn, sk, sp, weight, first);
  else if (mode == SA_CLAST4)
    hipLaunchKernelGGL((softmax_accum_kernel<K1, SA_CLAST4>), grid, block, 0, st, logits, prob_sum, pred, hw, groups, sn, sk, sp, weight, first);
  else
    hipLaunchKernelGGL((softmax_accum_kernel<K1, SA_SCALAR>), grid, block, 0, st, logits, prob_sum, pred, hw, groups, sn, sk, sp, weight, first);
}

extern "C" int mia_softmax_accum(const float* logits, float* prob_sum, long long* pred, int nb, int64_t hw, int k1, int64_t sn,
                                 int64_t sk, int64_t sp, float weight, int first, void* stream) {
  MIA_CHECK_ARG(logits && nb > 0 && hw > 0, "mia_softmax_accum: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= PMAXK, "mia_softmax_accum: k1=%d not in [1,%d]", k1, PMAXK);
  MIA_CHECK_ARG(prob_sum || (first && pred), "mia_softmax_accum: prob_sum may be NULL only with first set and pred given");
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0, "mia_softmax_accum: negative strides");
  const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  // four pixels per thread: 16-byte aligned units in the logits, the running sum and the label map
  const bool quad = hw % 4 == 0 && al16(logits) && sn % 4 == 0 && (!prob_sum || al16(prob_sum)) && (!pred || al16(pred));
  int mode = SA_SCALAR;
  if (quad && sp == 1 && sk % 4 == 0) mode = SA_PLANAR4;
  else if (quad && sk == 1 && sp == k1) mode = SA_CLAST4;
  const int64_t groups = (int64_t)nb * (mode == SA_SCALAR ? hw : hw / 4);
  MIA_CHECK_ARG(ceil_div64(groups, 256) <= 0x7fffffffLL, "mia_softmax_accum: nb * hw = %lld is too large", (long long)nb * hw);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k1) {
#define SA_CASE(K) case K: launch_softmax_accum<K>(mode, groups, st, logits, prob_sum, pred, hw, sn, sk, sp, weight, first); break;
    SA_CASE(1) SA_CASE(2) SA_CASE(3) SA_CASE(4) SA_CASE(5) SA_CASE(6) SA_CASE(7) SA_CASE(8)
#undef SA_CASE
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------ region ensemble
// The sigmoid counterpart for region-based models (one sigmoid output per region, regions may overlap): prob_sum = (first ? 0 :
// prob_sum) + weight * sigmoid(logits), and nnU-Net's region-to-label rule on the updated sum: pred = 0; for i in 0 .. K1-1:
// if prob_sum[i] > threshold: pred = class_order[i] -- later regions overwrite earlier ones.  Same ownership, order and access
// widths as softmax_accum_kernel.
__device__ __forceinline__ float sigmoid_w(float z, float weight) {
  const float e = __expf(-fabsf(z));  // in (0, 1]: nothing overflows
  const float r = 1.f / (1.f + e);
  return weight * (z >= 0.f ? r : e * r);
}

template <int K1, int MODE>
__global__ void __launch_bounds__(256) sigmoid_accum_kernel(const float* __restrict__ logits, float* __restrict__ prob_sum,
                                                            long long* __restrict__ pred, const long long* __restrict__ class_order,
                                                            int64_t hw, int64_t total, int64_t sn, int64_t sk, int64_t sp, float weight,
                                                            float threshold, int first) {
  constexpr int PX = MODE == SA_SCALAR ? 1 : 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one group of PX pixels
  if (idx >= total) return;
  const int64_t per = hw / PX, b = idx / per, p = (idx - b * per) * PX;
  const float* src = logits + b * sn;
  float v[PX][K1];
  if (MODE == SA_PLANAR4) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + k * sk + p);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i][k] = t[i];
    }
  } else if (MODE == SA_CLAST4) {  // four pixels = K1 consecutive 16-byte units
    float flat[4 * K1];
#pragma unroll
    for (int u = 0; u < K1; ++u) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + p * K1 + 4 * u);
#pragma unroll
      for (int i = 0; i < 4; ++i) flat[4 * u + i] = t[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < K1; ++k) v[i][k] = flat[i * K1 + k];
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) v[0][k] = src[p * sp + k * sk];
  }
#pragma unroll
  for (int i = 0; i < PX; ++i)
#pragma unroll
    for (int k = 0; k < K1; ++k) v[i][k] = sigmoid_w(v[i][k], weight);
  float* acc = prob_sum ? prob_sum + (b * K1) * hw + p : nullptr;
  if (acc && !first) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (PX == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(acc + k * hw);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i][k] += t[i];
      } else {
        v[0][k] += acc[k * hw];
      }
    }
  }
  if (acc) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (PX == 4) {
        f32x4 t;
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = v[i][k];
        store_data_fence();
        *reinterpret_cast<f32x4*>(acc + k * hw) = t;
        store_data_pad();  // tools/check_store_hazard.py
      } else {
        acc[k * hw] = v[0][k];
      }
    }
  }
  if (pred) {
    long long order[K1], lab[PX];
#pragma unroll
    for (int k = 0; k < K1; ++k) order[k] = class_order[k];
#pragma unroll
    for (int i = 0; i < PX; ++i) {
      lab[i] = 0;
#pragma unroll
      for (int k = 0; k < K1; ++k) lab[i] = v[i][k] > threshold ? order[k] : lab[i];
    }
    long long* dst = pred + b * hw + p;
    if (PX == 4) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      const i64x2 lo = i64x2{lab[0], lab[1]}, hi = i64x2{lab[2], lab[3]};
      store_data_fence();
      *reinterpret_cast<i64x2*>(dst) = lo;
      store_data_pad();
      *reinterpret_cast<i64x2*>(dst + 2) = hi;
      store_data_pad();
    } else {
      dst[0] = lab[0];
    }
  }
}

template <int K1>
static void launch_sigmoid_accum(int mode, int64_t groups, hipStream_t st, const float* logits, float* prob_sum, long long* pred,
                                 const long long* class_order, int64_t hw, int64_t sn, int64_t sk, int64_t sp, float weight,
                                 float threshold, int first) {
  const dim3 grid((unsigned)ceil_div64(groups, 256)), block(256);
#define SG_LAUNCH(M) hipLaunchKernelGGL((sigmoid_accum_kernel<K1, M>), grid, block, 0, st, logits, prob_sum, pred, class_order, hw, groups, \
                                        sn, sk, sp, weight, threshold, first)
  if (mode == SA_PLANAR4) SG_LAUNCH(SA_PLANAR4);
  else if (mode == SA_CLAST4) SG_LAUNCH(SA_CLAST4);
  else SG_LAUNCH(SA_SCALAR);
#undef SG_LAUNCH
}

extern "C" int mia_sigmoid_accum(const float* logits, float* prob_sum, long long* pred, const long long* class_order, int nb, int64_t hw,
                                 int c, int64_t sn, int64_t sk, int64_t sp, float weight, float threshold, int first, void* stream) {
  MIA_CHECK_ARG(logits && nb > 0 && hw > 0, "mia_sigmoid_accum: bad arguments");
  MIA_CHECK_ARG(c >= 1 && c <= PMAXK, "mia_sigmoid_accum: c=%d not in [1,%d]", c, PMAXK);
  MIA_CHECK_ARG(prob_sum || (first && pred), "mia_sigmoid_accum: prob_sum may be NULL only with first set and pred given");
  MIA_CHECK_ARG(!pred || class_order, "mia_sigmoid_accum: pred needs class_order");
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0, "mia_sigmoid_accum: negative strides");
  const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  // four pixels per thread: 16-byte aligned units in the logits, the running sum and the label map (the rule of mia_softmax_accum)
  const bool quad = hw % 4 == 0 && al16(logits) && sn % 4 == 0 && (!prob_sum || al16(prob_sum)) && (!pred || al16(pred));
  int mode = SA_SCALAR;
  if (quad && sp == 1 && sk % 4 == 0) mode = SA_PLANAR4;
  else if (quad && sk == 1 && sp == c) mode = SA_CLAST4;
  const int64_t groups = (int64_t)nb * (mode == SA_SCALAR ? hw : hw / 4);
  MIA_CHECK_ARG(ceil_div64(groups, 256) <= 0x7fffffffLL, "mia_sigmoid_accum: nb * hw = %lld is too large", (long long)nb * hw);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (c) {
#define SG_CASE(K) case K: launch_sigmoid_accum<K>(mode, groups, st, logits, prob_sum, pred, class_order, hw, sn, sk, sp, weight, threshold, first); break;
    SG_CASE(1) SG_CASE(2) SG_CASE(3) SG_CASE(4) SG_CASE(5) SG_CASE(6) SG_CASE(7) SG_CASE(8)
#undef SG_CASE
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------- sliding-window prediction
// canvas[n][k][y0 + i][x0 + j] = fma(gy[i] * gx[j], weight * softmax_k(logits[n][:, i', j']), canvas[...]) with (i', j') the
// pixel mirrored inside the window where flip_h / flip_w say so.  Every branch below evaluates exactly that expression per
// pixel -- one multiply for the importance, softmax_w, one explicit fma -- so which branch took a pixel cannot show in its bits.
enum { WA_SCALAR = 0, WA_PLANAR4 = 1, WA_CLAST4 = 2 };

template <int K1, int MODE>
__global__ void __launch_bounds__(256) window_accum_kernel(const float* __restrict__ logits, float* __restrict__ canvas,
                                                           const float* __restrict__ gy, const float* __restrict__ gx, int ph, int pw,
                                                           int h, int w, int y0, int x0, int64_t total, int64_t sn, int64_t sk,
                                                           int64_t sp, float weight, int flip_h, int flip_w) {
  constexpr int PX = MODE == WA_SCALAR ? 1 : 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one group of PX pixels of one window row
  if (idx >= total) return;
  const int gpr = pw / PX;  // groups per window row
  const int64_t row = idx / gpr, b = row / ph;
  const int j = (int)(idx - row * gpr) * PX, i = (int)(row - b * ph);
  const int si = flip_h ? ph - 1 - i : i;
  const int sj = flip_w ? pw - PX - j : j;                  // first source column of the group (its last canvas pixel when mirrored)
  const float* src = logits + b * sn;
  const int64_t p = (int64_t)si * pw + sj;
  float v[PX][K1];
  if (MODE == WA_PLANAR4) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + k * sk + p);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u][k] = t[u];
    }
  } else if (MODE == WA_CLAST4) {  // four pixels = K1 consecutive 16-byte units
    float flat[4 * K1];
#pragma unroll
    for (int u = 0; u < K1; ++u) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + p * K1 + 4 * u);
#pragma unroll
      for (int q = 0; q < 4; ++q) flat[4 * u + q] = t[q];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < K1; ++k) v[u][k] = flat[u * K1 + k];
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) v[0][k] = src[p * sp + k * sk];
  }
#pragma unroll
  for (int u = 0; u < PX; ++u) softmax_w<K1>(v[u], weight);
  const float wy = gy[i];
  float g[PX];  // importance of canvas pixel j + c
#pragma unroll
  for (int c = 0; c < PX; ++c) g[c] = wy * gx[j + c];
  float* acc = canvas + ((b * K1) * h + (y0 + i)) * (int64_t)w + x0 + j;
  const int64_t plane = (int64_t)h * w;
  if (PX == 4) {
    f32x4 t[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) t[k] = *reinterpret_cast<const f32x4*>(acc + k * plane);
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (flip_w) {  // canvas pixel c holds source pixel 3 - c
#pragma unroll
        for (int c = 0; c < 4; ++c) t[k][c] = __builtin_fmaf(g[c], v[3 - c][k], t[k][c]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) t[k][c] = __builtin_fmaf(g[c], v[c][k], t[k][c]);
      }
    }
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      store_data_fence();
      *reinterpret_cast<f32x4*>(acc + k * plane) = t[k];
      store_data_pad();  // tools/check_store_hazard.py
    }
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) acc[k * plane] = __builtin_fmaf(g[0], v[0][k], acc[k * plane]);
  }
}

template <int K1>
static void launch_window_accum(int mode, int64_t groups, hipStream_t st, const float* logits, float* canvas, const float* gy,
                                const float* gx, int ph, int pw, int h, int w, int y0, int x0, int64_t sn, int64_t sk, int64_t sp,
                                float weight, int flip_h, int flip_w) {
  const dim3 grid((unsigned)ceil_div64(groups, 256)), block(256);
#define WA_LAUNCH(M) hipLaunchKernelGGL((window_accum_kernel<K1, M>), grid, block, 0, st, logits, canvas, gy, gx, ph, pw, h, w, y0, x0, \
                                        groups, sn, sk, sp, weight, flip_h, flip_w)
  if (mode == WA_PLANAR4) WA_LAUNCH(WA_PLANAR4);
  else if (mode == WA_CLAST4) WA_LAUNCH(WA_CLAST4);
  else WA_LAUNCH(WA_SCALAR);
#undef WA_LAUNCH
}

extern "C" int mia_window_accum(const float* logits, float* canvas, const float* gy, const float* gx, int nb, int k1, int ph, int pw,
                                int h, int w, int y0, int x0, int64_t sn, int64_t sk, int64_t sp, float weight, int flip_h, int flip_w,
                                void* stream) {
  MIA_CHECK_ARG(logits && canvas && gy && gx && nb > 0 && ph > 0 && pw > 0 && h > 0 && w > 0, "mia_window_accum: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= PMAXK, "mia_window_accum: k1=%d not in [1,%d]", k1, PMAXK);
  MIA_CHECK_ARG(y0 >= 0 && x0 >= 0 && (int64_t)y0 + ph <= h && (int64_t)x0 + pw <= w,
                "mia_window_accum: window %dx%d at (%d,%d) does not lie inside the %dx%d canvas", ph, pw, y0, x0, h, w);
  MIA_CHECK_ARG(sn >= 0 && sk >= 0 && sp >= 0, "mia_window_accum: negative strides");
  const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  // four pixels per thread: every group is a 16-byte aligned unit of the logits (mirrored or not) and of the canvas
  const bool quad = pw % 4 == 0 && x0 % 4 == 0 && w % 4 == 0 && al16(logits) && sn % 4 == 0 && al16(canvas);
  int mode = WA_SCALAR;
  if (quad && sp == 1 && sk % 4 == 0) mode = WA_PLANAR4;
  else if (quad && sk == 1 && sp == k1) mode = WA_CLAST4;
  const int64_t groups = (int64_t)nb * ph * (mode == WA_SCALAR ? pw : pw / 4);
  MIA_CHECK_ARG(ceil_div64(groups, 256) <= 0x7fffffffLL, "mia_window_accum: nb * ph * pw = %lld is too large", (long long)nb * ph * pw);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k1) {
#define WA_CASE(K) case K: launch_window_accum<K>(mode, groups, st, logits, canvas, gy, gx, ph, pw, h, w, y0, x0, sn, sk, sp, weight, flip_h != 0, flip_w != 0); break;
    WA_CASE(1) WA_CASE(2) WA_CASE(3) WA_CASE(4) WA_CASE(5) WA_CASE(6) WA_CASE(7) WA_CASE(8)
#undef WA_CASE
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// pred = arg-max over classes of the raw canvas, then (normalise) canvas *= (scale * ry[y]) * rx[x]; PX pixels of one row per thread
template <int K1, int PX>
__global__ void __launch_bounds__(256) window_finalize_kernel(float* __restrict__ canvas, long long* __restrict__ pred,
                                                              const float* __restrict__ ry, const float* __restrict__ rx, int h, int w,
                                                              int64_t total, float scale, int normalise) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int gpr = w / PX;
  const int64_t row = idx / gpr, b = row / h;
  const int x = (int)(idx - row * gpr) * PX, y = (int)(row - b * h);
  const int64_t plane = (int64_t)h * w;
  float* acc = canvas + (b * K1) * plane + (int64_t)y * w + x;
  float v[PX][K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    if (PX == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(acc + k * plane);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c][k] = t[c];
    } else {
      v[0][k] = acc[k * plane];
    }
  }
  if (pred) {
    long long* dst = pred + b * plane + (int64_t)y * w + x;
    if (PX == 4) {
      typedef __attribute__((ext_vector_type(2))) long long i64x2;
      const i64x2 lo = i64x2{argmax_first<K1>(v[0]), argmax_first<K1>(v[1])}, hi = i64x2{argmax_first<K1>(v[2]), argmax_first<K1>(v[3])};
      store_data_fence();
      *reinterpret_cast<i64x2*>(dst) = lo;
      store_data_pad();  // tools/check_store_hazard.py
      *reinterpret_cast<i64x2*>(dst + 2) = hi;
      store_data_pad();
    } else {
      dst[0] = argmax_first<K1>(v[0]);
    }
  }
  if (normalise) {
    const float sy = scale * ry[y];
    float s[PX];
#pragma unroll
    for (int c = 0; c < PX; ++c) s[c] = sy * rx[x + c];
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      if (PX == 4) {
        f32x4 t;
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = v[c][k] * s[c];
        store_data_fence();
        *reinterpret_cast<f32x4*>(acc + k * plane) = t;
        store_data_pad();
      } else {
        acc[k * plane] = v[0][k] * s[0];
      }
    }
  }
}

extern "C" int mia_window_finalize(float* canvas, long long* pred, const float* ry, const float* rx, int nb, int k1, int h, int w,
                                   float scale, int normalise, void* stream) {
  MIA_CHECK_ARG(canvas && nb > 0 && h > 0 && w > 0, "mia_window_finalize: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= PMAXK, "mia_window_finalize: k1=%d not in [1,%d]", k1, PMAXK);
  MIA_CHECK_ARG(pred || normalise, "mia_window_finalize: nothing to do without pred and without normalise");
  MIA_CHECK_ARG(!normalise || (ry && rx), "mia_window_finalize: normalise needs ry and rx");
  const auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool quad = w % 4 == 0 && al16(canvas) && (!pred || al16(pred));
  const int64_t groups = (int64_t)nb * h * (quad ? w / 4 : w);
  MIA_CHECK_ARG(ceil_div64(groups, 256) <= 0x7fffffffLL, "mia_window_finalize: nb * h * w = %lld is too large", (long long)nb * h * w);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)ceil_div64(groups, 256)), block(256);
  switch (k1) {
#define WF_CASE(K)                                                                                                                      \
  case K:                                                                                                                               \
    if (quad) hipLaunchKernelGGL((window_finalize_kernel<K, 4>), grid, block, 0, st, canvas, pred, ry, rx, h, w, groups, scale, normalise); \
    else hipLaunchKernelGGL((window_finalize_kernel<K, 1>), grid, block, 0, st, canvas, pred, ry, rx, h, w, groups, scale, normalise);     \
    break;
    WF_CASE(1) WF_CASE(2) WF_CASE(3) WF_CASE(4) WF_CASE(5) WF_CASE(6) WF_CASE(7) WF_CASE(8)
#undef WF_CASE
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ------------------------------------------------------------------------------------------------------ mask denoise
#define DN_T 64                            // output tile edge
#define DN_MAXR 8                          // largest dilate / erode radius
#define DN_MAXHALO (4 * DN_MAXR + 3)       // 2 * (dilate + erode) + 3
#define DN_MAXROWS (DN_T + 2 * DN_MAXHALO) // 134 window rows; a row is 192 bits >= 64 + 2 * 35 columns
#define DN_THREADS 256
#define DN_ROWS_INFLIGHT 8                 // window rows (three loads each) a wave keeps in flight while it fills the window
#define DN_MAXDIM (1 << 20)

struct W3 { uint64_t a, b, c; };  // one window row: bit i of (a, b, c) = window column i, 0 <= i < 192

__device__ __forceinline__ W3 w3_or(W3 x, W3 y) { return W3{x.a | y.a, x.b | y.b, x.c | y.c}; }
__device__ __forceinline__ W3 w3_and(W3 x, W3 y) { return W3{x.a & y.a, x.b & y.b, x.c & y.c}; }
__device__ __forceinline__ W3 w3_not(W3 x) { return W3{~x.a, ~x.b, ~x.c}; }
__device__ __forceinline__ W3 w3_fill(bool one) { const uint64_t v = one ? ~0ull : 0ull; return W3{v, v, v}; }
// column i -> i + k / i - k, zeros shifted in, 0 < k < 64
__device__ __forceinline__ W3 w3_shl(W3 x, int k) { return W3{x.a << k, (x.b << k) | (x.a >> (64 - k)), (x.c << k) | (x.b >> (64 - k))}; }
__device__ __forceinline__ W3 w3_shr(W3 x, int k) { return W3{(x.a >> k) | (x.b << (64 - k)), (x.b >> k) | (x.c << (64 - k)), x.c >> k}; }
__device__ __forceinline__ uint64_t ones_below(int n) { return n <= 0 ? 0ull : (n >= 64 ? ~0ull : ((1ull << n) - 1)); }
__device__ __forceinline__ W3 w3_range(int lo, int hi) {  // columns lo <= i < hi
  return W3{ones_below(hi) & ~ones_below(lo), ones_below(hi - 64) & ~ones_below(lo - 64), ones_below(hi - 128) & ~ones_below(lo - 128)};
}
__device__ __forceinline__ uint64_t w3_bit(W3 x, int i) { return ((i < 64 ? x.a : (i < 128 ? x.b : x.c)) >> (i & 63)) & 1ull; }
__device__ __forceinline__ void w3_or_bit(W3& x, int i, uint64_t v) {
  const uint64_t m = v << (i & 63);
  if (i < 64) x.a |= m; else if (i < 128) x.b |= m; else x.c |= m;
}
// OR over columns i - r .. i + r: doubling shift-ORs up to 2r + 1 columns, then re-centre
__device__ __forceinline__ W3 w3_dilate(W3 x, int r) {
  if (r == 0) return x;
  const int n = 2 * r + 1;
  int cov = 1;
  while (2 * cov <= n) { x = w3_or(x, w3_shl(x, cov)); cov *= 2; }
  if (cov < n) x = w3_or(x, w3_shl(x, n - cov));
  return w3_shr(x, r);
}
struct DnGeom { int h, w, dil, ero, pad, halo, rows, rs, tiles_x, tiles_y, w0, w1, w2, w3; };

__device__ __forceinline__ int dn_idx(int buf, int m, int j, int row) { return ((buf * 2 + m) * 3 + j) * DN_MAXROWS + row; }
__device__ __forceinline__ W3 dn_load(const uint64_t* s, int buf, int m, int row) {
  return W3{s[dn_idx(buf, m, 0, row)], s[dn_idx(buf, m, 1, row)], s[dn_idx(buf, m, 2, row)]};
}
__device__ __forceinline__ void dn_store(uint64_t* s, int buf, int m, int row, W3 v) {
  s[dn_idx(buf, m, 0, row)] = v.a; s[dn_idx(buf, m, 1, row)] = v.b; s[dn_idx(buf, m, 2, row)] = v.c;
}

// One morphology stage on both masks, LDS buffer `from` -> `to`; a thread owns whole rows.  Clipping to the padded domain D =
// [-pad, h + pad) x [-pad, w + pad) (OpenCV ignores what lies outside the image it is given): the input of a stage holds the
// neutral value of that stage outside D (0 for a dilate, 1 for an erode), so plain window ORs / ANDs are the clipped ones, and a
// stage writes the neutral value of the NEXT stage there.  Rows / columns beyond the window edge count as neutral too; what that
// gets wrong stays within `radius` of the edge per stage, which is what the halo is for.
template <bool ERODE>
__device__ __forceinline__ void dn_stage(uint64_t* s, int from, int to, int r, bool next_neutral, bool last, const DnGeom& g, int ty0,
                                         int tx0, W3 dmask, W3 imask) {
  for (int item = threadIdx.x; item < 2 * g.rows; item += DN_THREADS) {
    const int m = item >= g.rows, wr = item - m * g.rows, y = ty0 - g.halo + wr;
    const int lo = wr - r < 0 ? 0 : wr - r, hi = wr + r > g.rows - 1 ? g.rows - 1 : wr + r;
    W3 acc = dn_load(s, from, m, lo);
    for (int q = lo + 1; q <= hi; ++q) acc = ERODE ? w3_and(acc, dn_load(s, from, m, q)) : w3_or(acc, dn_load(s, from, m, q));
    acc = ERODE ? w3_not(w3_dilate(w3_not(acc), r)) : w3_dilate(acc, r);
    W3 res;
    if (!last) {
      const bool in_rows = y >= -g.pad && y < g.h + g.pad;
      res = in_rows ? w3_or(w3_and(acc, dmask), next_neutral ? w3_not(dmask) : w3_fill(false)) : w3_fill(next_neutral);
    } else {
      // crop to the image, then BORDER_REFLECT_101 in x for the blur: column -t = column t, column w - 1 + t = column w - 1 - t
      res = (y >= 0 && y < g.h) ? w3_and(acc, imask) : w3_fill(false);
      const int c0 = g.halo - tx0;  // window column of image column 0
      for (int t = 1; t <= g.rs; ++t) {
        const int dl = c0 - t, sl = c0 + t, dr = c0 + g.w - 1 + t, sr = c0 + g.w - 1 - t;
        if (dl >= 0 && dl < 192 && sl >= 0 && sl < 192) w3_or_bit(res, dl, w3_bit(res, sl));
        if (dr >= 0 && dr < 192 && sr >= 0 && sr < 192) w3_or_bit(res, dr, w3_bit(res, sr));
      }
    }
    dn_store(s, to, m, wr, res);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(DN_THREADS) mask_denoise_kernel(const long long* __restrict__ in, long long* __restrict__ out, DnGeom g) {
  __shared__ uint64_t s[2 * 2 * 3 * DN_MAXROWS];
  const int tile = blockIdx.x % (g.tiles_x * g.tiles_y), b = blockIdx.x / (g.tiles_x * g.tiles_y);
  const int ty0 = (tile / g.tiles_x) * DN_T, tx0 = (tile % g.tiles_x) * DN_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long* src = in + (int64_t)b * g.h * g.w;
  // window: rows ty0 - halo .. ty0 + 64 + halo, columns tx0 - halo .. (bit 0 = column tx0 - halo); a wave packs 64 columns per ballot
  const int ncols = DN_T + 2 * g.halo;
  for (int r0 = wave; r0 < g.rows; r0 += DN_ROWS_INFLIGHT * (DN_THREADS / 64)) {  // independent loads first, then their ballots
    long long v[DN_ROWS_INFLIGHT][3];
#pragma unroll
    for (int u = 0; u < DN_ROWS_INFLIGHT; ++u) {
      const int wr = r0 + u * (DN_THREADS / 64), y = ty0 - g.halo + wr;
      const bool row_ok = wr < g.rows && y >= 0 && y < g.h;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int col = j * 64 + lane, x = tx0 - g.halo + col;
        v[u][j] = (row_ok && col < ncols && x >= 0 && x < g.w) ? src[(int64_t)y * g.w + x] : 0;
      }
    }
#pragma unroll
    for (int u = 0; u < DN_ROWS_INFLIGHT; ++u) {
      const int wr = r0 + u * (DN_THREADS / 64);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const uint64_t obj = __ballot(v[u][j] > 0), c1 = __ballot(v[u][j] == 1);
        if (lane == 0 && wr < g.rows) { s[dn_idx(0, 0, j, wr)] = obj; s[dn_idx(0, 1, j, wr)] = c1; }
      }
    }
  }
  __syncthreads();
  const int c0 = g.halo - tx0;
  const W3 dmask = w3_range(c0 - g.pad, c0 + g.w + g.pad), imask = w3_range(c0, c0 + g.w);
  dn_stage<false>(s, 0, 1, g.dil, true, false, g, ty0, tx0, dmask, imask);   // fill_hole: dilate,
  dn_stage<true>(s, 1, 0, g.ero, true, false, g, ty0, tx0, dmask, imask);    //            erode
  dn_stage<true>(s, 0, 1, g.ero, false, false, g, ty0, tx0, dmask, imask);   // remove_cc: erode,
  dn_stage<false>(s, 1, 0, g.dil, false, true, g, ty0, tx0, dmask, imask);   //            dilate; crop; reflect columns
  // smoothen_boundary: 8.8 fixed-point Gaussian in both axes, blur > 127 <=> weighted bit sum >= 2^15.  Lane = tile column, a wave
  // owns 16 tile rows: 22 horizontal sums per mask (rows reflected on read), then 16 vertical ones.
  const int x = tx0 + lane, yb = ty0 + wave * 16;
  // the seven bits around a lane's column sit in two consecutive 32-bit words of the row: word index and shift are per lane
  const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s);
  const int s0 = g.halo + lane - 3, k0 = s0 >> 5, k1 = k0 + 1;  // s0 <= 95: k1 <= 3
  const int o0 = 2 * (k0 >> 1) * DN_MAXROWS + (k0 & 1), o1 = 2 * (k1 >> 1) * DN_MAXROWS + (k1 & 1);
  int hs[2][22];
#pragma unroll
  for (int q = 0; q < 22; ++q) {
    const int yy = yb - 3 + q, ry = yy < 0 ? -yy : (yy >= g.h ? 2 * (g.h - 1) - yy : yy);
    int wr = ry - (ty0 - g.halo);
    wr = wr < 0 ? 0 : (wr > g.rows - 1 ? g.rows - 1 : wr);  // only rows whose weight is 0 or whose output is not stored get clamped
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int base = 2 * dn_idx(0, m, 0, wr);
      const uint32_t n7 = __builtin_amdgcn_alignbit(s32[base + o1], s32[base + o0], s0 & 31) & 0x7fu;
      hs[m][q] = g.w0 * __builtin_popcount(n7 & 0x41u) + g.w1 * __builtin_popcount(n7 & 0x22u) + g.w2 * __builtin_popcount(n7 & 0x14u) +
                 g.w3 * (int)((n7 >> 3) & 1u);
    }
  }
  long long* dst = out + (int64_t)b * g.h * g.w;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    int tot[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
      tot[m] = g.w0 * (hs[m][i] + hs[m][i + 6]) + g.w1 * (hs[m][i + 1] + hs[m][i + 5]) + g.w2 * (hs[m][i + 2] + hs[m][i + 4]) + g.w3 * hs[m][i + 3];
    const int y = yb + i;
    if (y < g.h && x < g.w) dst[(int64_t)y * g.w + x] = tot[0] >= 32768 ? (tot[1] >= 32768 ? 1 : 2) : 0;
  }
}

extern "C" int mia_mask_denoise_supported(int h, int w, int dilate, int erode, int smooth_k) {
  if (dilate < 0 || dilate > DN_MAXR || erode < 0 || erode > DN_MAXR) return 0;
  if (smooth_k != 1 && smooth_k != 3 && smooth_k != 5 && smooth_k != 7) return 0;
  if (h <= smooth_k / 2 || w <= smooth_k / 2 || h > DN_MAXDIM || w > DN_MAXDIM) return 0;
  return 1;
}

extern "C" int mia_mask_denoise(const long long* in, long long* out, int nb, int h, int w, int dilate, int erode, int smooth_k,
                                void* stream) {
  MIA_CHECK_ARG(in && out && in != out && nb > 0 && h > 0 && w > 0, "mia_mask_denoise: bad arguments");
  if (!mia_mask_denoise_supported(h, w, dilate, erode, smooth_k)) {
    mia_set_error("mia_mask_denoise: h=%d w=%d dilate=%d erode=%d smooth_k=%d is outside the kernel's range (radii 0..%d, smooth_k 1/3/5/7, "
                  "smooth_k / 2 < h, w <= %d)", h, w, dilate, erode, smooth_k, DN_MAXR, DN_MAXDIM);
    return MIA_EUNSUPPORTED;
  }
  DnGeom g;
  g.h = h; g.w = w; g.dil = dilate; g.ero = erode; g.pad = dilate > erode ? dilate : erode;
  g.halo = 2 * (dilate + erode) + 3;
  g.rows = DN_T + 2 * g.halo;
  g.rs = smooth_k / 2;
  g.tiles_x = ceil_div(w, DN_T); g.tiles_y = ceil_div(h, DN_T);
  static const int taps[4][4] = {{0, 0, 0, 256}, {0, 0, 64, 128}, {0, 16, 64, 96}, {8, 28, 56, 72}};  // _SMALL_GAUSS_256, outer to centre
  g.w0 = taps[g.rs][0]; g.w1 = taps[g.rs][1]; g.w2 = taps[g.rs][2]; g.w3 = taps[g.rs][3];
  const int64_t blocks = (int64_t)nb * g.tiles_x * g.tiles_y;
  MIA_CHECK_ARG(blocks <= 0x7fffffffLL, "mia_mask_denoise: %lld tiles are too many for one launch", (long long)blocks);
  hipLaunchKernelGGL(mask_denoise_kernel, dim3((unsigned)blocks), dim3(DN_THREADS), 0, static_cast<hipStream_t>(stream), in, out, g);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
