// What the streaming losses over logits-shaped tensors share.  ONE definition of each piece, so that the files cannot drift apart
// (loss_common.h, ds_common.h).
//   consistency.hip, cps.hip, bcp.hip, w2s.hip, dtc.hip   the layout classes of a logits-shaped tensor (cs_mode), the loads and stores of
//                                 one thread's pixel group in each class (cs_load, cs_store), the per-pixel soft-max in double (cs_softmax)
//   consistency.hip, cps.hip      the dispatch over (class count, layout class of the first, of the second tensor): CS_DISPATCH; dtc.hip: CS_MODES
//   cps.hip, w2s.hip, hard_loss.h the hard-label pieces: cs_argmax, cs_nll_term, cs_max
//   bcp.hip, w2s.hip, dtc.hip     a thread that owns FOUR consecutive pixels on every path (px4_*; cs_park not in dtc.hip), the dispatch over (class
//                                 count, layout class): CS_DISPATCH1, and the launch of a mix under a mask (px4_mix_launch); their
//                                 Dice + CE core is hard_loss.h
// The double-precision partial sums, which boundary.hip and urpc.hip use too, are in loss_common.h.
#pragma once
#include "loss_common.h"

enum { CS_SCALAR = 0, CS_PLANAR4 = 1, CS_CLAST4 = 2 };
#define CS_PX(MODE) ((MODE) == CS_SCALAR ? 1 : 4)

// Soft-max of one pixel in double: e_k = exp(z_k - max) in fp32, times (1 + the rounding error of the subtraction), so the only
// fp32 error left in s_k is expf's own (bl_softmax of boundary.hip with the class count as a template parameter).
template <int K1>
__device__ __forceinline__ void cs_softmax(const float (&v)[K1], double (&s)[K1]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) mx = fmaxf(mx, v[k]);
  double se = 0.0;
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    const float d = v[k] - mx;
    const float t = d - v[k];
    const float err = (v[k] - (d - t)) + (-mx - t);  // v - mx = d + err exactly
    const float e = expf(d);
    s[k] = (double)e + (double)e * (double)err;
    se += s[k];
  }
  const double inv = 1.0 / se;
#pragma unroll
  for (int k = 0; k < K1; ++k) s[k] *= inv;
}

// arg-max of the fp32 logits, the lowest index among equals; mx = the maximum.  Plain compares and selects over compile-time indices:
// no register array is indexed at run time.
template <int K1>
__device__ __forceinline__ int cs_argmax(const float (&v)[K1], float& mx) {
  int y = 0;
  mx = v[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) {
    const bool up = v[k] > mx;
    mx = up ? v[k] : mx;
    y = up ? k : y;
  }
  return y;
}

// logsumexp(v) - v[y] for a label y that need not be v's own arg-max: -log(max_k p_k) = log sum_k exp(v_k - max v) comes from the
// soft-max, max v - v[y] is exact in double.  v[y] is picked as a sum of one value and K1 - 1 zeros (exact): a chain of selects between
// the array's elements is turned into an indexed read of the array by the compiler, which then keeps the array in scratch memory.
template <int K1>
__device__ __forceinline__ double cs_nll_term(const float (&v)[K1], int y, float mx, double pmax) {
  float vy = 0.f;
#pragma unroll
  for (int k = 0; k < K1; ++k) vy += (k == y) ? v[k] : 0.f;
  return -log(pmax) + ((double)mx - (double)vy);
}

template <int K1>
__device__ __forceinline__ double cs_max(const double (&p)[K1]) {
  double r = p[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) r = p[k] > r ? p[k] : r;
  return r;
}

// the logits of PX consecutive pixels from pixel p of one image (`img` = the image's first element)
template <int K1, int MODE>
__device__ __forceinline__ void cs_load(const float* __restrict__ img, int64_t p, const LossGeom& g, float (&v)[CS_PX(MODE)][K1]) {
  if (MODE == CS_PLANAR4) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(img + k * g.sk + p);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i][k] = t[i];
    }
  } else if (MODE == CS_CLAST4) {  // four pixels = K1 consecutive 16-byte units
    f32x4 f[K1];
#pragma unroll
    for (int u = 0; u < K1; ++u) f[u] = *reinterpret_cast<const f32x4*>(img + p * K1 + 4 * u);
#pragma unroll
    for (int i = 0; i < 4; ++i) quad_unpack<K1>(f, i, v[i]);
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) v[0][k] = img[p * g.sp + k * g.sk];
  }
}

template <int K1, int MODE>
__device__ __forceinline__ void cs_store(float* __restrict__ img, int64_t p, const LossGeom& g, const float (&v)[CS_PX(MODE)][K1]) {
  if (MODE == CS_PLANAR4) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      f32x4 t;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = v[i][k];
      *reinterpret_cast<f32x4*>(img + k * g.sk + p) = t;
      store_data_pad();  // the next unit's values may recycle t's registers (common.h)
    }
  } else if (MODE == CS_CLAST4) {
#pragma unroll
    for (int u = 0; u < K1; ++u) {
      f32x4 t;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[i] = v[(4 * u + i) / K1][(4 * u + i) % K1];
      *reinterpret_cast<f32x4*>(img + p * K1 + 4 * u) = t;
      store_data_pad();
    }
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) img[p * g.sp + k * g.sk] = v[0][k];
  }
}

// ---- a thread that owns FOUR consecutive pixels on the 16-byte path and on the scalar path alike (bcp.hip, w2s.hip)
// four bytes of a per-pixel byte map (mask, code) from `mk`, byte i in bits 8 i ..: one 4-byte load, or the live ones one by one
// and zeros for the rest
template <bool WIDE>
__device__ __forceinline__ unsigned px4_bytes(const unsigned char* __restrict__ mk, int nlive) {
  if (WIDE) return *reinterpret_cast<const unsigned*>(mk);
  unsigned m = 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nlive) m |= (unsigned)mk[i] << (8 * i);
  return m;
}

// the logits of the group's four pixels from pixel p; the scalar path reads the live ones one by one and zeroes the rest
template <int K1, int MODE>
__device__ __forceinline__ void px4_load(const float* __restrict__ img, int64_t p, int nlive, const LossGeom& g, float (&v)[4][K1]) {
  if constexpr (MODE != CS_SCALAR) {
    cs_load<K1, MODE>(img, p, g, v);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t[1][K1];
#pragma unroll
      for (int k = 0; k < K1; ++k) t[0][k] = 0.f;
      if (i < nlive) cs_load<K1, CS_SCALAR>(img, p + i, g, t);
#pragma unroll
      for (int k = 0; k < K1; ++k) v[i][k] = t[0][k];
    }
  }
}

// the wave's sum of v in double, parked by lane 0 as a (hi, lo) pair in the block's slots
template <int NF, int NI>
__device__ __forceinline__ void cs_park(const LossBlockSums<NF, NI>& red, int slot, double v) {
  float pr[2];
  loss_split(wave_sum_d(v), pr);
  if (red.l == 0) { red.f[red.w][slot] = pr[0]; red.f[red.w][slot + 1] = pr[1]; }
}

static inline bool cs_al4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }
static inline bool cs_al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
// the four-pixel layout class of a logits-shaped tensor whose base and image stride are 16-byte aligned, else CS_SCALAR
static int cs_mode(const void* base, const LossGeom& g, int k1) {
  if (!cs_al16(base) || g.sn % 4 != 0) return CS_SCALAR;
  if (g.sp == 1 && g.sk % 4 == 0) return CS_PLANAR4;
  if (g.sk == 1 && g.sp == k1) return CS_CLAST4;
  return CS_SCALAR;
}
// the same for a thread that owns four pixels of the logits and of up to two byte maps (mask, code; a null one passes): the maps are
// read as 4-byte words
static int px4_mode(const void* z, const LossGeom& g, int k1, int64_t hw, const void* m0, const void* m1) {
  return hw % 4 == 0 && cs_al4(m0) && cs_al4(m1) ? cs_mode(z, g, k1) : CS_SCALAR;
}

// The body of mia_bcp_mix and mia_cutmix_perm after their pointer checks: out [nb][c][hw] fp32 (image stride out_sn) takes each
// element from a or from b by the mask byte of its pixel.  WIDE (four pixels per thread: 16-byte loads and stores, the mask as 4-byte
// words) when every operand allows it.  `launch(wide, grid, chw, total)` starts the caller's kernel and returns MIA_OK, or its own
// error.
template <typename F>
static int px4_mix_launch(const char* who, const void* a, const void* b, const unsigned char* mask, const void* out, int nb, int c,
                          int64_t hw, int64_t mask_sn, int64_t out_sn, F&& launch) {
  MIA_CHECK_ARG(nb > 0 && c > 0 && hw > 0 && hw <= 0x7fffffff && (int64_t)c * hw <= 0x7fffffff &&
                    ceil_div64((int64_t)nb * c * hw, 256) <= 0x7fffffff,
                "%s: bad shape nb=%d c=%d hw=%lld", who, nb, c, (long long)hw);
  MIA_CHECK_ARG((mask_sn == 0 || mask_sn == hw) && out_sn >= (int64_t)c * hw, "%s: bad strides mask_sn=%lld out_sn=%lld", who,
                (long long)mask_sn, (long long)out_sn);
  const int64_t chw = (int64_t)c * hw;
  const bool wide = hw % 4 == 0 && out_sn % 4 == 0 && cs_al16(a) && cs_al16(b) && cs_al16(out) && cs_al4(mask);
  const int64_t total = (int64_t)nb * (wide ? chw / 4 : chw);
  if (const int e = launch(wide, dim3((unsigned)ceil_div64(total, 256)), chw, total)) return e;
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

// FN<K1, SM, TM>(args...) for the run-time (k1, student mode, teacher mode); the modes are both CS_SCALAR or both four-pixel classes
#define CS_MODES(FN, K, ...)                                                                        \
  do {                                                                                              \
    if (sm == CS_SCALAR) FN<K, CS_SCALAR, CS_SCALAR>(__VA_ARGS__);                                  \
    else if (sm == CS_PLANAR4 && tm == CS_PLANAR4) FN<K, CS_PLANAR4, CS_PLANAR4>(__VA_ARGS__);      \
    else if (sm == CS_PLANAR4) FN<K, CS_PLANAR4, CS_CLAST4>(__VA_ARGS__);                           \
    else if (tm == CS_PLANAR4) FN<K, CS_CLAST4, CS_PLANAR4>(__VA_ARGS__);                           \
    else FN<K, CS_CLAST4, CS_CLAST4>(__VA_ARGS__);                                                  \
  } while (0)
#define CS_DISPATCH(FN, ...)                            \
  switch (k1) {                                         \
    case 1: CS_MODES(FN, 1, __VA_ARGS__); break;        \
    case 2: CS_MODES(FN, 2, __VA_ARGS__); break;        \
    case 3: CS_MODES(FN, 3, __VA_ARGS__); break;        \
    case 4: CS_MODES(FN, 4, __VA_ARGS__); break;        \
    case 5: CS_MODES(FN, 5, __VA_ARGS__); break;        \
    case 6: CS_MODES(FN, 6, __VA_ARGS__); break;        \
    case 7: CS_MODES(FN, 7, __VA_ARGS__); break;        \
    default: CS_MODES(FN, 8, __VA_ARGS__); break;       \
  }

// The same for a loss over ONE logits tensor (bcp.hip, w2s.hip): FN<K1, SM>(args...) for the run-time (k1, sm)
#define CS_MODES1(FN, K, ...)                                          \
  do {                                                                 \
    if (sm == CS_SCALAR) FN<K, CS_SCALAR>(__VA_ARGS__);                \
    else if (sm == CS_PLANAR4) FN<K, CS_PLANAR4>(__VA_ARGS__);         \
    else FN<K, CS_CLAST4>(__VA_ARGS__);                                \
  } while (0)
#define CS_DISPATCH1(FN, ...)                            \
  switch (k1) {                                          \
    case 1: CS_MODES1(FN, 1, __VA_ARGS__); break;        \
    case 2: CS_MODES1(FN, 2, __VA_ARGS__); break;        \
    case 3: CS_MODES1(FN, 3, __VA_ARGS__); break;        \
    case 4: CS_MODES1(FN, 4, __VA_ARGS__); break;        \
    case 5: CS_MODES1(FN, 5, __VA_ARGS__); break;        \
    case 6: CS_MODES1(FN, 6, __VA_ARGS__); break;        \
    case 7: CS_MODES1(FN, 7, __VA_ARGS__); break;        \
    default: CS_MODES1(FN, 8, __VA_ARGS__); break;       \
  }
