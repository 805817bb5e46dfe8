// 1x1 segmentation head (C0 -> K1 <= 8 logits), alone and fused with the last block's norm + LeakyReLU, gfx950.
//
// Reference: seg_output = Conv2d(c0, K1, 1) (src/models/unet/unet.py:176).  Pure bandwidth: the head reads C0
// values and writes K1 per pixel.
#include "common.h"

#define MAXK 8

// ---------------------------------------------------------------- head forward
// 8 lanes per pixel, each lane strides over the pixel's 16-byte units; K1 accumulators; xor-shuffle reduce.
template <typename T>
__global__ void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                float* __restrict__ out, int64_t npix, int c0, int k1, int64_t osp, int64_t osk,
                                int64_t osn, int64_t hw, bool vec) {  // vec: c0 % EPU == 0 and x 16-byte aligned (the host decides)
  extern __shared__ float wsh[];  // [k1][c0]
  for (int i = threadIdx.x; i < k1 * c0; i += blockDim.x) wsh[i] = w[i];
  __syncthreads();
  constexpr int EPU = Elem<T>::EPU;
  const int sub = threadIdx.x & 7;
  for (int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; p < npix; p += ((int64_t)gridDim.x * blockDim.x) >> 3) {
    float acc[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) acc[k] = 0.f;
    const T* row = x + p * c0;
    if (vec) {
      for (int u = sub; u < c0 / EPU; u += 8) {
        alignas(16) T v[EPU];
        *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(row + u * EPU);
#pragma unroll
        for (int e = 0; e < EPU; ++e) {
          const float xv = Elem<T>::ld(v + e);
#pragma unroll
          for (int k = 0; k < MAXK; ++k)
            if (k < k1) acc[k] += xv * wsh[k * c0 + u * EPU + e];
        }
      }
    } else {
      for (int ch = sub; ch < c0; ch += 8) {
        const float xv = Elem<T>::ld(row + ch);
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
          if (k < k1) acc[k] += xv * wsh[k * c0 + ch];
      }
    }
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      if (k < k1) {
        float v = acc[k];
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
        if (sub == 0) out[(osn == hw * osp ? p * osp : (p / hw) * osn + (p % hw) * osp) + k * osk] = v + b[k];
      }
    }
  }
}

// ---------------------------------------------------------------- specialised head kernels
// K1 (logits) and UPP (16-byte units per pixel = threads per pixel, 4 / 8 / 16) are compile-time: a thread owns one
// channel unit for its whole life, so its K1 x EPU weights sit in registers, there is no per-element index arithmetic
// (32-bit pixel counters, pointers advanced by a constant stride) and the cross-lane sums are DPP butterflies instead
// of LDS permutes.  Contract: c0 == UPP * EPU, pixel-linear logits (sn == hw * sp), n * hw * c0 < 2^31.
__device__ __forceinline__ float dpp_add(float v, int ctrl_sel) {
  const int iv = __builtin_bit_cast(int, v);
  int r;
  if (ctrl_sel == 0) r = __builtin_amdgcn_update_dpp(iv, iv, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]: lane ^ 1
  else if (ctrl_sel == 1) r = __builtin_amdgcn_update_dpp(iv, iv, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]: lane ^ 2
  else if (ctrl_sel == 2) r = __builtin_amdgcn_update_dpp(iv, iv, 0x141, 0xF, 0xF, false);  // row_half_mirror: other quad of 8
  else r = __builtin_amdgcn_update_dpp(iv, iv, 0x140, 0xF, 0xF, false);                     // row_mirror: other half of 16
  return v + __builtin_bit_cast(float, r);
}
template <int UPP> __device__ __forceinline__ float group_sum(float v) {  // every lane of the UPP group gets the sum
  v = dpp_add(v, 0); v = dpp_add(v, 1);
  if (UPP >= 8) v = dpp_add(v, 2);
  if (UPP >= 16) v = dpp_add(v, 3);
  return v;
}

template <typename T, int K1, int UPP>
__global__ __launch_bounds__(256) void head_fwd_fast_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ b, float* __restrict__ out, int npix,
                                                            int64_t osp, int64_t osk) {
  constexpr int EPU = Elem<T>::EPU, C0 = UPP * EPU, LANES = 256 / UPP;
  const int u = threadIdx.x % UPP, pl = threadIdx.x / UPP;
  float wr[K1][EPU];
#pragma unroll
  for (int k = 0; k < K1; ++k)
#pragma unroll
    for (int e = 0; e < EPU; ++e) wr[k][e] = w[k * C0 + u * EPU + e];
  float bu = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) bu = (u == k) ? b[k] : bu;
  const int stride = gridDim.x * LANES;
  auto body = [&](const u32x4& raw, int p) {
    alignas(16) T v[EPU];
    *reinterpret_cast<u32x4*>(v) = raw;
    float acc[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) acc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPU; ++e) {
      const float xv = Elem<T>::ld(v + e);
#pragma unroll
      for (int k = 0; k < K1; ++k) acc[k] += xv * wr[k][e];
    }
    float mine = 0.f;  // lane u < K1 of the group writes logit u: one store instruction, K1 adjacent floats per pixel
#pragma unroll
    for (int k = 0; k < K1; ++k) { const float t = group_sum<UPP>(acc[k]); mine = (u == k) ? t : mine; }
    if (u < K1) out[(int64_t)p * osp + u * osk] = mine + bu;
  };
  int p = blockIdx.x * LANES + pl;
  for (; p + stride < npix; p += 2 * stride) {  // two independent 16-byte loads in flight
    const u32x4 r0 = *reinterpret_cast<const u32x4*>(x + (size_t)p * C0 + u * EPU);
    const u32x4 r1 = *reinterpret_cast<const u32x4*>(x + (size_t)(p + stride) * C0 + u * EPU);
    body(r0, p); body(r1, p + stride);
  }
  if (p < npix) body(*reinterpret_cast<const u32x4*>(x + (size_t)p * C0 + u * EPU), p);
}

template <typename T, int K1, int UPP>
__global__ __launch_bounds__(256) void head_bwd_input_fast_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                                                  T* __restrict__ dx, int npix, int64_t gsp, int64_t gsk) {
  constexpr int EPU = Elem<T>::EPU, C0 = UPP * EPU, LANES = 256 / UPP;
  const int u = threadIdx.x % UPP, pl = threadIdx.x / UPP;
  float wr[K1][EPU];
#pragma unroll
  for (int k = 0; k < K1; ++k)
#pragma unroll
    for (int e = 0; e < EPU; ++e) wr[k][e] = w[k * C0 + u * EPU + e];
  const int stride = gridDim.x * LANES;
  for (int p = blockIdx.x * LANES + pl; p < npix; p += stride) {
    const float* g = dl + (int64_t)p * gsp;
    float gv[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) gv[k] = g[k * gsk];
    alignas(16) T o[EPU];
#pragma unroll
    for (int e = 0; e < EPU; ++e) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < K1; ++k) a += gv[k] * wr[k][e];
      o[e] = Elem<T>::cvt(a);
    }
    *reinterpret_cast<u32x4*>(dx + (size_t)p * C0 + u * EPU) = *reinterpret_cast<const u32x4*>(o);
  }
}

// part: [gridDim.x][K1][C0 + 1] (last column = bias partial), same layout as the generic kernels
template <typename T, int K1, int UPP>
__global__ __launch_bounds__(256) void head_bwd_weight_fast_kernel(const float* __restrict__ dl, const T* __restrict__ x,
                                                                   float* __restrict__ part, int npix, int64_t gsp, int64_t gsk) {
  constexpr int EPU = Elem<T>::EPU, C0 = UPP * EPU, LANES = 256 / UPP, SHS = C0 + 1;
  __shared__ float shd[LANES * SHS];
  const int u = threadIdx.x % UPP, pl = threadIdx.x / UPP;
  const int per = (npix + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = r0 + per < npix ? r0 + per : npix;
  float acc[K1][EPU], bacc[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    bacc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPU; ++e) acc[k][e] = 0.f;
  }
  auto body = [&](const u32x4& raw, const float* gv) {
    alignas(16) T v[EPU];
    *reinterpret_cast<u32x4*>(v) = raw;
#pragma unroll
    for (int e = 0; e < EPU; ++e) {
      const float xv = Elem<T>::ld(v + e);
#pragma unroll
      for (int k = 0; k < K1; ++k) acc[k][e] += gv[k] * xv;
    }
#pragma unroll
    for (int k = 0; k < K1; ++k) bacc[k] += gv[k];
  };
  int p = r0 + pl;
  for (; p + LANES < r1; p += 2 * LANES) {
    const u32x4 a0 = *reinterpret_cast<const u32x4*>(x + (size_t)p * C0 + u * EPU);
    const u32x4 a1 = *reinterpret_cast<const u32x4*>(x + (size_t)(p + LANES) * C0 + u * EPU);
    float g0[K1], g1[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) { g0[k] = dl[(int64_t)p * gsp + k * gsk]; g1[k] = dl[(int64_t)(p + LANES) * gsp + k * gsk]; }
    body(a0, g0); body(a1, g1);
  }
  if (p < r1) {
    float g0[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) g0[k] = dl[(int64_t)p * gsp + k * gsk];
    body(*reinterpret_cast<const u32x4*>(x + (size_t)p * C0 + u * EPU), g0);
  }
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPU; ++e) shd[pl * SHS + u * EPU + e] = acc[k][e];
    if (u == 0) shd[pl * SHS + C0] = bacc[k];
    __syncthreads();
    if (threadIdx.x <= C0) {
      float t = 0.f;
      for (int j = 0; j < LANES; ++j) t += shd[j * SHS + threadIdx.x];
      part[((size_t)blockIdx.x * K1 + k) * (C0 + 1) + threadIdx.x] = t;
    }
  }
}

// 0 = not eligible; otherwise UPP
static int head_fast_upp(int dtype, int c0, int k1, int64_t npix, int64_t sn, int64_t sp, int64_t hw, const void* x) {
  const int epu = dtype == MIA_BF16 ? 8 : 4;
  if (dtype != MIA_BF16 && dtype != MIA_F32) return 0;
  if (c0 % epu != 0 || (reinterpret_cast<uintptr_t>(x) & 15) != 0) return 0;
  const int upp = c0 / epu;
  if (upp != 4 && upp != 8 && upp != 16) return 0;
  if (k1 < 2 || k1 > 4) return 0;
  if (sn != hw * sp || npix * c0 >= ((int64_t)1 << 31)) return 0;
  return upp;
}
#define HEAD_DISPATCH(KERNEL, T, grid, ...)                                                                           \
  do {                                                                                                                \
    if (upp == 4) {                                                                                                   \
      if (k1 == 2) hipLaunchKernelGGL((KERNEL<T, 2, 4>), grid, dim3(256), 0, st, __VA_ARGS__);                        \
      else if (k1 == 3) hipLaunchKernelGGL((KERNEL<T, 3, 4>), grid, dim3(256), 0, st, __VA_ARGS__);                   \
      else hipLaunchKernelGGL((KERNEL<T, 4, 4>), grid, dim3(256), 0, st, __VA_ARGS__);                                \
    } else if (upp == 8) {                                                                                            \
      if (k1 == 2) hipLaunchKernelGGL((KERNEL<T, 2, 8>), grid, dim3(256), 0, st, __VA_ARGS__);                        \
      else if (k1 == 3) hipLaunchKernelGGL((KERNEL<T, 3, 8>), grid, dim3(256), 0, st, __VA_ARGS__);                   \
      else hipLaunchKernelGGL((KERNEL<T, 4, 8>), grid, dim3(256), 0, st, __VA_ARGS__);                                \
    } else {                                                                                                          \
      if (k1 == 2) hipLaunchKernelGGL((KERNEL<T, 2, 16>), grid, dim3(256), 0, st, __VA_ARGS__);                       \
      else if (k1 == 3) hipLaunchKernelGGL((KERNEL<T, 3, 16>), grid, dim3(256), 0, st, __VA_ARGS__);                  \
      else hipLaunchKernelGGL((KERNEL<T, 4, 16>), grid, dim3(256), 0, st, __VA_ARGS__);                               \
    }                                                                                                                 \
  } while (0)

// the fused norm + head kernels also take twelve units per pixel (96 bf16 / 48 fp32 channels) on groups of sixteen lanes
#define HEAD_DISPATCH_N(KERNEL, T, grid, ...)                                                                         \
  do {                                                                                                                \
    if (upp == 12) {                                                                                                  \
      if (k1 == 2) hipLaunchKernelGGL((KERNEL<T, 2, 16, 12>), grid, dim3(256), 0, st, __VA_ARGS__);                   \
      else if (k1 == 3) hipLaunchKernelGGL((KERNEL<T, 3, 16, 12>), grid, dim3(256), 0, st, __VA_ARGS__);              \
      else hipLaunchKernelGGL((KERNEL<T, 4, 16, 12>), grid, dim3(256), 0, st, __VA_ARGS__);                           \
    } else HEAD_DISPATCH(KERNEL, T, grid, __VA_ARGS__);                                                               \
  } while (0)


// ---------------------------------------------------------------- head fused with the last block's norm + LeakyReLU
// The last decoder block's activated output z = lrelu(scale*y + shift) has exactly one consumer, the 1x1 head.  These
// kernels recompute it from the raw conv output y on load (per-(image, channel) scale / shift in registers: a block
// works inside one image), so z is never written or read: the forward apply pass and one activation round trip vanish.
// CU < UPP (round 5: 96 channels in bf16 = 12 units dealt to groups of 16 lanes): lanes CU .. UPP - 1 of a pixel group load nothing and
// hold zero coefficients, so the group sums and every address (C0 = CU units) stay right; 25 % idle lanes on a memory-bound pass.
template <typename T, int K1, int UPP, int CU = UPP>
__global__ __launch_bounds__(256) void head_norm_fwd_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float slope,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            float* __restrict__ out, int hw, int slabs, int64_t osn,
                                                            int64_t osp, int64_t osk) {
  constexpr int EPU = Elem<T>::EPU, C0 = CU * EPU, LANES = 256 / UPP;
  const int u = threadIdx.x % UPP, pl = threadIdx.x / UPP;
  const bool act = CU == UPP || u < CU;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int n = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int per = (hw + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  float wr[K1][EPU], sc[EPU], sf[EPU];
#pragma unroll
  for (int e = 0; e < EPU; ++e) {
    sc[e] = act ? scale[(size_t)n * C0 + u * EPU + e] : 0.f;
    sf[e] = act ? shift[(size_t)n * C0 + u * EPU + e] : 0.f;
#pragma unroll
    for (int k = 0; k < K1; ++k) wr[k][e] = act ? w[k * C0 + u * EPU + e] : 0.f;
  }
  float bu = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) bu = (u == k) ? b[k] : bu;
  const T* yb = y + (size_t)n * hw * C0 + u * EPU;
  float* ob = out + (int64_t)n * osn + u * osk;
  auto body = [&](const u32x4& raw, int p) {
    alignas(16) T v[EPU];
    *reinterpret_cast<u32x4*>(v) = raw;
    float acc[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) acc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPU; ++e) {
      float xv = sc[e] * Elem<T>::ld(v + e) + sf[e];
      xv = xv > 0.f ? xv : xv * slope;
#pragma unroll
      for (int k = 0; k < K1; ++k) acc[k] += xv * wr[k][e];
    }
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < K1; ++k) { const float t = group_sum<UPP>(acc[k]); mine = (u == k) ? t : mine; }
    if (u < K1) ob[(int64_t)p * osp] = mine + bu;
  };
  // Bulk: a wave takes 64 consecutive pixels per round -- UPP independent 16-byte loads per lane in flight (each load
  // instruction reads 64 / UPP whole pixels = 1 KB contiguous), the K1 sums of a pixel go through a wave-private LDS
  // transpose so that the logits leave as one contiguous 256-byte run per class plane (NCHW fp32 logits: the per-pixel
  // store of K1 lanes per pixel group wrote 32-byte pieces, 1.8 TB/s on the cfg3 launch).
  constexpr int GP = 64 / UPP;  // pixels per load instruction and wave
  __shared__ float tbuf[4][K1][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gl = lane / UPP;
  float* tb = &tbuf[wave][0][0];
  const int nbulk = (r1 - r0) / 256 * 256;
  for (int q0 = r0 + wave * 64; q0 < r0 + nbulk; q0 += 256) {
    u32x4 raw[UPP];
#pragma unroll
    for (int j = 0; j < UPP; ++j) raw[j] = act ? *reinterpret_cast<const u32x4*>(yb + (size_t)(q0 + j * GP + gl) * C0) : zero4;
#pragma unroll
    for (int j = 0; j < UPP; ++j) {
      alignas(16) T v[EPU];
      *reinterpret_cast<u32x4*>(v) = raw[j];
      float acc[K1];
#pragma unroll
      for (int k = 0; k < K1; ++k) acc[k] = 0.f;
#pragma unroll
      for (int e = 0; e < EPU; ++e) {
        float xv = sc[e] * Elem<T>::ld(v + e) + sf[e];
        xv = xv > 0.f ? xv : xv * slope;
#pragma unroll
        for (int k = 0; k < K1; ++k) acc[k] += xv * wr[k][e];
      }
      float mine = 0.f;
#pragma unroll
      for (int k = 0; k < K1; ++k) { const float t = group_sum<UPP>(acc[k]); mine = (u == k) ? t : mine; }
      if (u < K1) tb[u * 64 + j * GP + gl] = mine + bu;
    }
    // wave-private transpose: other lanes read what this lane wrote.  The wave barrier (free at run time) states the
    // write -> read and, for the next round, read -> write order in the program instead of leaving it to in-order DS issue.
    __builtin_amdgcn_wave_barrier();
    float* on = out + (int64_t)n * osn + (int64_t)(q0 + lane) * osp;
#pragma unroll
    for (int k = 0; k < K1; ++k) on[k * osk] = tb[k * 64 + lane];
    __builtin_amdgcn_wave_barrier();
  }
  for (int p = r0 + nbulk + pl; p < r1; p += LANES) body(act ? *reinterpret_cast<const u32x4*>(yb + (size_t)p * C0) : zero4, p);
}

// part: [gridDim.x][K1][C0 + 1] like head_bwd_weight_fast_kernel, with x = lrelu(scale*y + shift) recomputed
template <typename T, int K1, int UPP, int CU = UPP>  // (CU < UPP: see head_norm_fwd_kernel)
__global__ __launch_bounds__(256) void head_norm_wgrad_kernel(const float* __restrict__ dl, const T* __restrict__ y,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              float slope, float* __restrict__ part, int hw, int slabs,
                                                              int64_t gsn, int64_t gsp, int64_t gsk) {
  constexpr int EPU = Elem<T>::EPU, C0 = CU * EPU, LANES = 256 / UPP, SHS = C0 + 1;
  __shared__ float shd[LANES * SHS];
  const int u = threadIdx.x % UPP, pl = threadIdx.x / UPP;
  const bool act = CU == UPP || u < CU;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const int n = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int per = (hw + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  float sc[EPU], sf[EPU], acc[K1][EPU], bacc[K1];
#pragma unroll
  for (int e = 0; e < EPU; ++e) {
    sc[e] = act ? scale[(size_t)n * C0 + u * EPU + e] : 0.f;
    sf[e] = act ? shift[(size_t)n * C0 + u * EPU + e] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    bacc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPU; ++e) acc[k][e] = 0.f;
  }
  const T* yb = y + (size_t)n * hw * C0 + u * EPU;
  const float* gb = dl + (int64_t)n * gsn;
  auto body = [&](const u32x4& raw, const float (&gv)[K1]) {
    alignas(16) T v[EPU];
    *reinterpret_cast<u32x4*>(v) = raw;
#pragma unroll
    for (int k = 0; k < K1; ++k) bacc[k] += gv[k];
#pragma unroll
    for (int e = 0; e < EPU; ++e) {
      float xv = sc[e] * Elem<T>::ld(v + e) + sf[e];
      xv = xv > 0.f ? xv : xv * slope;
#pragma unroll
      for (int k = 0; k < K1; ++k) acc[k][e] += gv[k] * xv;
    }
  };
  int p = r0 + pl;
  for (; p + 3 * LANES < r1; p += 4 * LANES) {  // four pixels' loads in flight per thread
    u32x4 raw[4];
    float gv[4][K1];
#pragma unroll
    for (int j = 0; j < 4; ++j) raw[j] = act ? *reinterpret_cast<const u32x4*>(yb + (size_t)(p + j * LANES) * C0) : zero4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < K1; ++k) gv[j][k] = gb[(int64_t)(p + j * LANES) * gsp + k * gsk];
#pragma unroll
    for (int j = 0; j < 4; ++j) body(raw[j], gv[j]);
  }
  for (; p < r1; p += LANES) {
    float gv[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) gv[k] = gb[(int64_t)p * gsp + k * gsk];
    body(act ? *reinterpret_cast<const u32x4*>(yb + (size_t)p * C0) : zero4, gv);
  }
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPU; ++e)
      if (act) shd[pl * SHS + u * EPU + e] = acc[k][e];
    if (u == 0) shd[pl * SHS + C0] = bacc[k];
    __syncthreads();
    if (threadIdx.x <= C0) {
      float t = 0.f;
      for (int j = 0; j < LANES; ++j) t += shd[j * SHS + threadIdx.x];
      part[((size_t)blockIdx.x * K1 + k) * (C0 + 1) + threadIdx.x] = t;
    }
  }
}

extern "C" int mia_head_fwd(const void* x, int dtype, const float* w, const float* b, float* logits, int n, int64_t hw,
                            int c0, int k1, int64_t osn, int64_t osk, int64_t osp, void* stream) {
  MIA_CHECK_ARG(x && w && b && logits && n > 0 && hw > 0 && c0 > 0, "mia_head_fwd: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= MAXK, "mia_head_fwd: k1=%d not in [1,%d]", k1, MAXK);
  MIA_CHECK_ARG((size_t)k1 * c0 * 4 <= 60000, "mia_head_fwd: weight tile too large for LDS");
  const int64_t npix = (int64_t)n * hw;
  const int blocks = (int)((npix * 8 + 255) / 256 < 8192 ? (npix * 8 + 255) / 256 : 8192);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (const int upp = head_fast_upp(dtype, c0, k1, npix, osn, osp, hw, x)) {
    const int lanes = 256 / upp;
    const int fblocks = (int)((npix + 2 * lanes - 1) / (2 * lanes) < 16384 ? (npix + 2 * lanes - 1) / (2 * lanes) : 16384);
    if (dtype == MIA_BF16) HEAD_DISPATCH(head_fwd_fast_kernel, bf16_t, dim3(fblocks), static_cast<const bf16_t*>(x), w, b, logits, (int)npix, osp, osk);
    else HEAD_DISPATCH(head_fwd_fast_kernel, float, dim3(fblocks), static_cast<const float*>(x), w, b, logits, (int)npix, osp, osk);
    MIA_LAUNCH_CHECK();
    return MIA_OK;
  }
  // 16-byte loads need an aligned x as well as whole units: a view into a larger buffer takes the scalar branch (as in mia_head_bwd)
  const bool vec = c0 % (dtype == MIA_BF16 ? 8 : 4) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (dtype == MIA_BF16)
    hipLaunchKernelGGL(head_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), k1 * c0 * 4, st, static_cast<const bf16_t*>(x), w, b, logits, npix, c0, k1, osp, osk, osn, hw, vec);
  else if (dtype == MIA_F32)
    hipLaunchKernelGGL(head_fwd_kernel<float>, dim3(blocks), dim3(256), k1 * c0 * 4, st, static_cast<const float*>(x), w, b, logits, npix, c0, k1, osp, osk, osn, hw, vec);
  else { mia_set_error("mia_head_fwd: bad dtype"); return MIA_EARG; }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// ---------------------------------------------------------------- head backward (input gradient)
template <typename T>
__global__ void head_bwd_input_kernel(const float* __restrict__ dl, const float* __restrict__ w, T* __restrict__ dx,
                                      int64_t npix, int c0, int k1, int64_t gsp, int64_t gsk, int64_t gsn, int64_t hw) {
  extern __shared__ float wsh[];
  for (int i = threadIdx.x; i < k1 * c0; i += blockDim.x) wsh[i] = w[i];
  __syncthreads();
  const int64_t total = npix * c0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / c0;
    const int ch = (int)(i - p * c0);
    const float* g = dl + (gsn == hw * gsp ? p * gsp : (p / hw) * gsn + (p % hw) * gsp);
    float s = 0.f;
    for (int k = 0; k < k1; ++k) s += g[k * gsk] * wsh[k * c0 + ch];
    Elem<T>::st(dx + i, s);
  }
}

// weight / bias gradient partials: block handles a pixel slab; thread -> channel, loops pixels
template <typename T>
__global__ void head_bwd_weight_kernel(const float* __restrict__ dl, const T* __restrict__ x, float* __restrict__ part,
                                       int64_t npix, int c0, int k1, int64_t gsp, int64_t gsk, int64_t gsn, int64_t hw) {
  // part: [gridDim.x][k1][c0 + 1]  (last column = bias partial)
  extern __shared__ float sh[];  // [rows_par][cw] per k
  const int cw = blockDim.x >= c0 ? c0 : blockDim.x, rows_par = blockDim.x / cw;
  const int tc = threadIdx.x % cw, tr = threadIdx.x / cw;
  const int64_t per = (npix + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = r0 + per < npix ? r0 + per : npix;
  for (int cb = 0; cb < c0; cb += cw) {
    const int ch = cb + tc;
    float acc[MAXK], bacc[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) { acc[k] = 0.f; bacc[k] = 0.f; }
    if (ch < c0 && tr < rows_par)
      for (int64_t p = r0 + tr; p < r1; p += rows_par) {
        const float xv = Elem<T>::ld(x + p * c0 + ch);
        const float* g = dl + (gsn == hw * gsp ? p * gsp : (p / hw) * gsn + (p % hw) * gsp);
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
          if (k < k1) { const float gv = g[k * gsk]; acc[k] += gv * xv; bacc[k] += gv; }
      }
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      if (k >= k1) break;
      __syncthreads();
      sh[threadIdx.x] = acc[k];
      sh[blockDim.x + threadIdx.x] = bacc[k];
      __syncthreads();
      if (tr == 0 && ch < c0) {
        float t = 0.f;
        for (int j = 0; j < rows_par; ++j) t += sh[j * cw + tc];
        part[((size_t)blockIdx.x * k1 + k) * (c0 + 1) + ch] = t;
        if (ch == 0) {
          float tb = 0.f;
          for (int j = 0; j < rows_par; ++j) tb += sh[blockDim.x + j * cw];
          part[((size_t)blockIdx.x * k1 + k) * (c0 + 1) + c0] = tb;
        }
      }
    }
    __syncthreads();
  }
}

// block = 16 outputs x 16 lanes sweeping the partial blocks
__global__ void head_bwd_final_kernel(const float* __restrict__ part, int nblk, int k1, int c0, float* __restrict__ dw,
                                      float* __restrict__ db, int accumulate) {
  __shared__ float sh[16][17];
  const int cl = threadIdx.x & 15, tl = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + cl;
  const int tot = k1 * (c0 + 1);
  float s = 0.f;
  if (i < tot)
    for (int b = tl; b < nblk; b += 16) s += part[(size_t)b * tot + i];
  sh[tl][cl] = s;
  __syncthreads();
  if (tl == 0 && i < tot) {
    float t = 0.f;
    for (int j = 0; j < 16; ++j) t += sh[j][cl];
    const int k = i / (c0 + 1), ch = i % (c0 + 1);
    if (ch < c0) dw[k * c0 + ch] = accumulate ? dw[k * c0 + ch] + t : t;
    else db[k] = accumulate ? db[k] + t : t;
  }
}

// vectorised variants (c0 % EPU == 0, 16-byte aligned): thread = (pixel lane, 16-byte unit)
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_input_vec_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                                                 T* __restrict__ dx, int64_t npix, int c0, int k1, int64_t gsp,
                                                                 int64_t gsk, int64_t gsn, int64_t hw) {
  extern __shared__ float wsh[];
  for (int i = threadIdx.x; i < k1 * c0; i += blockDim.x) wsh[i] = w[i];
  __syncthreads();
  constexpr int EPU = Elem<T>::EPU;
  const int upp = c0 / EPU;
  const int64_t total = npix * upp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = i / upp;
    const int ch = (int)(i - p * upp) * EPU;
    const float* g = dl + (gsn == hw * gsp ? p * gsp : (p / hw) * gsn + (p % hw) * gsp);
    float acc[EPU];
#pragma unroll
    for (int e = 0; e < EPU; ++e) acc[e] = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k < k1) {
        const float gv = g[k * gsk];
#pragma unroll
        for (int e = 0; e < EPU; ++e) acc[e] += gv * wsh[k * c0 + ch + e];
      }
    alignas(16) T out[EPU];
#pragma unroll
    for (int e = 0; e < EPU; ++e) out[e] = Elem<T>::cvt(acc[e]);
    *reinterpret_cast<u32x4*>(dx + i * EPU) = *reinterpret_cast<const u32x4*>(out);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void head_bwd_weight_vec_kernel(const float* __restrict__ dl, const T* __restrict__ x,
                                                                  float* __restrict__ part, int64_t npix, int c0, int k1,
                                                                  int64_t gsp, int64_t gsk, int64_t gsn, int64_t hw) {
  // part: [gridDim.x][k1][c0 + 1]; requires c0 <= 256 and c0 % EPU == 0
  constexpr int EPU = Elem<T>::EPU;
  extern __shared__ float shd[];  // [lanes][c0 + 1]
  const int shs = c0 + 1;
  const int upp = c0 / EPU, lanes = 256 / upp;
  const int u = threadIdx.x % upp, pl = threadIdx.x / upp;
  const int64_t per = (npix + gridDim.x - 1) / gridDim.x, r0 = blockIdx.x * per, r1 = r0 + per < npix ? r0 + per : npix;
  float acc[MAXK][EPU], bacc[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    bacc[k] = 0.f;
#pragma unroll
    for (int e = 0; e < EPU; ++e) acc[k][e] = 0.f;
  }
  if (pl < lanes)
    for (int64_t p = r0 + pl; p < r1; p += lanes) {
      alignas(16) T v[EPU];
      *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(x + p * c0 + u * EPU);
      const float* g = dl + (gsn == hw * gsp ? p * gsp : (p / hw) * gsn + (p % hw) * gsp);
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k < k1) {
          const float gv = g[k * gsk];
          bacc[k] += gv;
#pragma unroll
          for (int e = 0; e < EPU; ++e) acc[k][e] += gv * Elem<T>::ld(v + e);
        }
    }
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {  // static indexing: a runtime k would push acc[][] to scratch memory
    if (k < k1) {
      __syncthreads();
      if (pl < lanes) {
#pragma unroll
        for (int e = 0; e < EPU; ++e) shd[pl * shs + u * EPU + e] = acc[k][e];
        if (u == 0) shd[pl * shs + c0] = bacc[k];
      }
      __syncthreads();
      if (threadIdx.x <= c0) {
        float t = 0.f;
        for (int j = 0; j < lanes; ++j) t += shd[j * shs + threadIdx.x];
        part[((size_t)blockIdx.x * k1 + k) * (c0 + 1) + threadIdx.x] = t;
      }
    }
  }
}

#define HEAD_BWD_BLOCKS 2048
extern "C" int mia_head_bwd_workspace(int c0, int k1) { return HEAD_BWD_BLOCKS * k1 * (c0 + 1); }

extern "C" int mia_head_bwd(const float* dlogits, const void* x, int dtype, const float* w, void* dx, float* dw, float* db,
                            float* workspace, int n, int64_t hw, int c0, int k1, int64_t gsn, int64_t gsk, int64_t gsp,
                            int accumulate, void* stream) {
  // dw == db == NULL: the input gradient alone (a backward with frozen parameters); the weight kernels and the workspace are not touched
  const bool wg = dw != nullptr || db != nullptr;
  MIA_CHECK_ARG(dlogits && x && w && (wg ? (dw && db && workspace) : dx != nullptr) && n > 0 && hw > 0 && c0 > 0, "mia_head_bwd: bad arguments");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= MAXK, "mia_head_bwd: k1=%d not in [1,%d]", k1, MAXK);
  const int64_t npix = (int64_t)n * hw;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t total = npix * c0;
  const int blocks = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  const int wblocks = (int)(npix / 64 < 1 ? 1 : (npix / 64 > HEAD_BWD_BLOCKS ? HEAD_BWD_BLOCKS : npix / 64));
  const int epu = dtype == MIA_BF16 ? 8 : 4;
  const bool vec = (c0 % epu == 0) && c0 <= 255 && c0 / epu <= 128 && (256 / (c0 / epu)) <= 128 &&
                   ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
  const int upp = ((reinterpret_cast<uintptr_t>(dx) & 15) == 0) ? head_fast_upp(dtype, c0, k1, npix, gsn, gsp, hw, x) : 0;
  if (upp) {
    const int lanes = 256 / upp;
    const int iblocks = (int)((npix + lanes - 1) / lanes < 16384 ? (npix + lanes - 1) / lanes : 16384);
    if (dtype == MIA_BF16) {
      if (dx) HEAD_DISPATCH(head_bwd_input_fast_kernel, bf16_t, dim3(iblocks), dlogits, w, static_cast<bf16_t*>(dx), (int)npix, gsp, gsk);
      if (wg) { HEAD_DISPATCH(head_bwd_weight_fast_kernel, bf16_t, dim3(wblocks), dlogits, static_cast<const bf16_t*>(x), workspace, (int)npix, gsp, gsk); }
    } else {
      if (dx) HEAD_DISPATCH(head_bwd_input_fast_kernel, float, dim3(iblocks), dlogits, w, static_cast<float*>(dx), (int)npix, gsp, gsk);
      if (wg) { HEAD_DISPATCH(head_bwd_weight_fast_kernel, float, dim3(wblocks), dlogits, static_cast<const float*>(x), workspace, (int)npix, gsp, gsk); }
    }
  } else if (vec && (dtype == MIA_BF16 || dtype == MIA_F32)) {
    const int64_t units = npix * (c0 / epu);
    const int vblocks = (int)((units + 255) / 256 < 16384 ? (units + 255) / 256 : 16384);
    if (dtype == MIA_BF16) {
      if (dx) hipLaunchKernelGGL(head_bwd_input_vec_kernel<bf16_t>, dim3(vblocks), dim3(256), k1 * c0 * 4, st, dlogits, w, static_cast<bf16_t*>(dx), npix, c0, k1, gsp, gsk, gsn, hw);
      if (wg) { hipLaunchKernelGGL(head_bwd_weight_vec_kernel<bf16_t>, dim3(wblocks), dim3(256), (256 / (c0 / epu)) * (c0 + 1) * 4, st, dlogits, static_cast<const bf16_t*>(x), workspace, npix, c0, k1, gsp, gsk, gsn, hw); }
    } else {
      if (dx) hipLaunchKernelGGL(head_bwd_input_vec_kernel<float>, dim3(vblocks), dim3(256), k1 * c0 * 4, st, dlogits, w, static_cast<float*>(dx), npix, c0, k1, gsp, gsk, gsn, hw);
      if (wg) { hipLaunchKernelGGL(head_bwd_weight_vec_kernel<float>, dim3(wblocks), dim3(256), (256 / (c0 / epu)) * (c0 + 1) * 4, st, dlogits, static_cast<const float*>(x), workspace, npix, c0, k1, gsp, gsk, gsn, hw); }
    }
  } else if (dtype == MIA_BF16) {
    if (dx) hipLaunchKernelGGL(head_bwd_input_kernel<bf16_t>, dim3(blocks), dim3(256), k1 * c0 * 4, st, dlogits, w, static_cast<bf16_t*>(dx), npix, c0, k1, gsp, gsk, gsn, hw);
    if (wg) { hipLaunchKernelGGL(head_bwd_weight_kernel<bf16_t>, dim3(wblocks), dim3(256), 512 * 4, st, dlogits, static_cast<const bf16_t*>(x), workspace, npix, c0, k1, gsp, gsk, gsn, hw); }
  } else if (dtype == MIA_F32) {
    if (dx) hipLaunchKernelGGL(head_bwd_input_kernel<float>, dim3(blocks), dim3(256), k1 * c0 * 4, st, dlogits, w, static_cast<float*>(dx), npix, c0, k1, gsp, gsk, gsn, hw);
    if (wg) { hipLaunchKernelGGL(head_bwd_weight_kernel<float>, dim3(wblocks), dim3(256), 512 * 4, st, dlogits, static_cast<const float*>(x), workspace, npix, c0, k1, gsp, gsk, gsn, hw); }
  } else { mia_set_error("mia_head_bwd: bad dtype"); return MIA_EARG; }
  if (wg) { hipLaunchKernelGGL(head_bwd_final_kernel, dim3(ceil_div(k1 * (c0 + 1), 16)), dim3(256), 0, st, workspace, wblocks, k1, c0, dw, db, accumulate); }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// 0 = not eligible for the fused (norm + LeakyReLU + head) kernels, else units per pixel
extern "C" int mia_head_norm_eligible(int dtype, int n, int64_t hw, int c0, int k1) {
  const int epu = dtype == MIA_BF16 ? 8 : 4;
  if ((dtype != MIA_BF16 && dtype != MIA_F32) || c0 % epu != 0) return 0;
  const int upp = c0 / epu;
  if ((upp != 4 && upp != 8 && upp != 12 && upp != 16) || k1 < 2 || k1 > 4) return 0;
  if (hw >= ((int64_t)1 << 31) || n > HEAD_BWD_BLOCKS) return 0;
  return upp;
}
static int head_norm_slabs(int n, int64_t hw) {
  int64_t sl = HEAD_BWD_BLOCKS / n;
  const int64_t maxsl = hw / 512 > 0 ? hw / 512 : 1;
  if (sl > maxsl) sl = maxsl;
  return (int)(sl < 1 ? 1 : sl);
}

// logits = W * lrelu(scale*y + shift) + b   (y = raw conv output of the last decoder block, NHWC; scale / shift [N][C0])
extern "C" int mia_head_norm_fwd(const void* y, int dtype, const float* scale, const float* shift, float slope, const float* w,
                                 const float* b, float* logits, int n, int64_t hw, int c0, int k1, int64_t osn, int64_t osk,
                                 int64_t osp, void* stream) {
  MIA_CHECK_ARG(y && scale && shift && w && b && logits && n > 0 && hw > 0, "mia_head_norm_fwd: bad arguments");
  const int upp = mia_head_norm_eligible(dtype, n, hw, c0, k1);
  MIA_CHECK_ARG(upp > 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "mia_head_norm_fwd: shape not eligible (c0=%d k1=%d)", c0, k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = head_norm_slabs(n, hw);
  if (dtype == MIA_BF16) HEAD_DISPATCH_N(head_norm_fwd_kernel, bf16_t, dim3(n * slabs), static_cast<const bf16_t*>(y), scale, shift, slope, w, b, logits, (int)hw, slabs, osn, osp, osk);
  else HEAD_DISPATCH_N(head_norm_fwd_kernel, float, dim3(n * slabs), static_cast<const float*>(y), scale, shift, slope, w, b, logits, (int)hw, slabs, osn, osp, osk);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// dW, db of the head with its input recomputed from y (workspace: mia_head_bwd_workspace floats)
extern "C" int mia_head_norm_wgrad(const float* dlogits, const void* y, int dtype, const float* scale, const float* shift,
                                   float slope, float* dw, float* db, float* workspace, int n, int64_t hw, int c0, int k1,
                                   int64_t gsn, int64_t gsk, int64_t gsp, int accumulate, void* stream) {
  MIA_CHECK_ARG(dlogits && y && scale && shift && dw && db && workspace && n > 0 && hw > 0, "mia_head_norm_wgrad: bad arguments");
  const int upp = mia_head_norm_eligible(dtype, n, hw, c0, k1);
  MIA_CHECK_ARG(upp > 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0, "mia_head_norm_wgrad: shape not eligible (c0=%d k1=%d)", c0, k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = head_norm_slabs(n, hw);
  if (dtype == MIA_BF16) HEAD_DISPATCH_N(head_norm_wgrad_kernel, bf16_t, dim3(n * slabs), dlogits, static_cast<const bf16_t*>(y), scale, shift, slope, workspace, (int)hw, slabs, gsn, gsp, gsk);
  else HEAD_DISPATCH_N(head_norm_wgrad_kernel, float, dim3(n * slabs), dlogits, static_cast<const float*>(y), scale, shift, slope, workspace, (int)hw, slabs, gsn, gsp, gsk);
  hipLaunchKernelGGL(head_bwd_final_kernel, dim3(ceil_div(k1 * (c0 + 1), 16)), dim3(256), 0, st, workspace, n * slabs, k1, c0, dw, db, accumulate);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
