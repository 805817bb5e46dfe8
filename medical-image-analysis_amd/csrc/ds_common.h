// What the kernels that upsample low-resolution logits in registers share (ds_loss.hip, urpc.hip): the taps and weights of torch's
// interpolate(scale_factor=factor, mode="bilinear", align_corners=False) for an integer factor (the arithmetic of
// resize_bilinear_kernel in augment.hip), and the low-resolution tile of the gather backward.  ONE definition of each, so that the two
// files cannot drift apart.
#pragma once
#include "loss_common.h"

#define DS_LDS_BYTES (60 * 1024)  // per block: below the 64 KiB a kernel gets without asking, two or more blocks per CU

// source taps of full-resolution index `dst` on an axis of n low-resolution pixels (scale = 1 / factor, exact)
struct DsTap { int i0, i1; float l; };
__device__ __forceinline__ DsTap ds_tap(int dst, float scale, int n) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  DsTap t;
  t.i0 = (int)s;
  t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
  t.l = s - (float)t.i0;
  return t;
}
// weight of that full-resolution index on low-resolution pixel i (both taps can name i at a clamped border)
__device__ __forceinline__ float ds_weight(const DsTap& t, int i) { return (t.i0 == i ? 1.f - t.l : 0.f) + (t.i1 == i ? t.l : 0.f); }

// u[k] = bilinear(z)[k] at one full-resolution pixel; zb = the image's logits
template <int NK>
__device__ __forceinline__ void ds_interp(const float* __restrict__ zb, const LossGeom& g, int w, int k1, const DsTap& ty, const DsTap& tx,
                                          float (&v)[NK]) {
  const int64_t o00 = ((int64_t)ty.i0 * w + tx.i0) * g.sp, o01 = ((int64_t)ty.i0 * w + tx.i1) * g.sp;
  const int64_t o10 = ((int64_t)ty.i1 * w + tx.i0) * g.sp, o11 = ((int64_t)ty.i1 * w + tx.i1) * g.sp;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) {
      const int64_t ok = k * g.sk;
      const float top = (1.f - tx.l) * zb[o00 + ok] + tx.l * zb[o01 + ok];
      const float bot = (1.f - tx.l) * zb[o10 + ok] + tx.l * zb[o11 + ok];
      v[k] = (1.f - ty.l) * top + ty.l * bot;
    } else {
      v[k] = 0.f;
    }
}

// low-resolution tile of a gather backward: the largest of the factor's default that keeps the block's LDS under DS_LDS_BYTES.
// LDS: du [k1][RH][pitch] (pitch = RW + 1, odd), then tx [k1][tw][RH], with RH = (th + 1) factor and RW = (tw + 1) factor.
static inline size_t ds_bwd_lds(int factor, int k1, int th, int tw) {
  const size_t RH = (size_t)(th + 1) * factor, pitch = (size_t)(tw + 1) * factor + 1;
  return ((size_t)k1 * RH * pitch + (size_t)k1 * tw * RH) * sizeof(float);
}
static inline void ds_bwd_tile(int factor, int k1, int* th, int* tw) {
  int a = factor == 2 ? 16 : factor == 4 ? 8 : factor == 8 ? 4 : 3, c = a;
  while (ds_bwd_lds(factor, k1, a, c) > DS_LDS_BYTES && (a > 1 || c > 1)) {
    if (a >= c) --a; else --c;
  }
  *th = a; *tw = c;
}
