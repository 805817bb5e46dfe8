// Dual-task consistency on the GPU (gfx950): one network predicts the segmentation and, from a second 1x1 head, a level-set map -- tanh
// of a regression of the normalised signed distance to the object boundary -- and the two must agree on every image (DTC: Luo et al.,
// AAAI 2021).  The reference has no such code; the definition is losses/dual_task.py.
//
// z [nb][k1][hw] fp32 by (sn, sk, sp) are the segmentation logits, r [nb][k1 - 1][hw] fp32 by (rsn, rsk, rsp) the level-set logits,
// channel c of r belongs to class c + 1; the first lb images are labelled and have phi [lb][k1 - 1][hw] (contiguous fp32, the signed
// distance map of boundary.hip at unit spacing) and the extents ext [lb][k1 - 1][2] = {max phi, max -phi}, both >= 0.
//   s = softmax(z),  t = tanh(r),  q = sigmoid(-k t)
//   T = phi / m_out (phi > 0),  -(1 - phi) / (1 + m_in) (phi < 0),  0 (phi = 0)          never stored: computed per pixel
//   L_cons = mean over ALL (n, c, p) of (q_c - s_{c+1})^2,   L_sdf = mean over (n < lb, c, p) of (t - T)^2   (0 when lb = 0)
//   L = w0 L_cons + w1 L_sdf,  {w0, w1} = dyn[0..1] read on the device (dyn NULL: 1, 1)
//   out = {L, L_cons, L_sdf};  coef = {2 w0 / (nb C hw), 2 w1 / (lb C hw) or 0}: what the backward reads, each rounded once to fp32
//   dz_j = go coef0 s_j (e_j - sum_i s_i e_i),  e_0 = 0, e_{c+1} = -(q_c - s_{c+1})
//   dr_c = go [coef0 (q_c - s_{c+1}) (-k q_c (1 - q_c)) + (n < lb) coef1 (t - T)] (1 - t^2)
// Everything per pixel is double arithmetic on the fp32 inputs.  tanh and 1 - t^2 come from ONE expm1: with m = expm1(-2 |r|),
// |t| = -m / (2 + m) and 1 - t^2 = 4 (1 + m) / (2 + m)^2, so neither cancels for small or for large |r|.  The sigmoid is evaluated
// from e = exp(-|k t|): a = 1 / (1 + e), b = e a, q is a or b by the sign and q (1 - q) = a b -- finite for |k t| in the thousands,
// where e and with it q (1 - q) underflow to 0.
//   dtc_extent_kernel     block (plane, slab): max phi and max -phi of non-negative values, merged by INTEGER max on the bit patterns
//                         (exact and order-independent; the destination is zeroed by a memset node before)
//   dtc_fwd_kernel        block (image, slab of pixels): ONE streaming pass over z, r and (n < lb) phi
//   dtc_finalize_kernel   one block: the partials in a fixed order in double (loss_totals) -> out, coef
//   dtc_bwd_kernel        one streaming pass, a thread per pixel group: recomputes s, t, q, T; writes dz and dr by their own strides
// z and r are each planar with 16-byte units, channels-last with 16-byte units (the head's layout, batch slices included) or anything
// else by scalar strides; the 16-byte path needs BOTH in a four-pixel class, hw % 4 == 0 and a 16-byte aligned phi, and in the backward
// each gradient in the layout class of its logits.  The channels-last helper covers C = 1 (one 16-byte unit is four pixels), so r takes
// the 16-byte path for k1 = 2 as well.  A thread owns the SAME four consecutive pixels on the 16-byte path and on the scalar path, and
// every sum runs in the same order on both, so the two paths give the same bits.  No float atomics: bit-identical from run to run; an
// image's gradient depends on the rest of the batch through coef alone; nothing synchronises with the host.
#include "pixel_stream.h"

// the per-pixel double expressions are shared by the two paths; without contraction they are also the same instructions on both
#pragma clang fp contract(off)

// ---------------------------------------------------------------- what forward and backward share
// t = tanh(r) and sech2 = 1 - t^2 in double from the fp32 logit
__device__ __forceinline__ void dtc_tanh(float r, double& t, double& sech2) {
  const double a = fabs((double)r);
  const double m = expm1(-2.0 * a);  // in (-1, 0]
  const double den = 2.0 + m, inv = 1.0 / den;
  const double ta = -m * inv;
  t = r < 0.f ? -ta : ta;  // a NaN stays a NaN through m
  sech2 = 4.0 * (1.0 + m) * inv * inv;
}

// q = sigmoid(-k t) and qq = q (1 - q)
__device__ __forceinline__ void dtc_sigmoid(double k, double t, double& q, double& qq) {
  const double x = -k * t;
  const double e = exp(-fabs(x));  // in [0, 1]
  const double a = 1.0 / (1.0 + e), b = e * a;
  q = x >= 0.0 ? a : b;
  qq = a * b;
}

// the normalised target from phi and the reciprocal extents {1 / m_out (0 with no outside), 1 / (1 + m_in)}
__device__ __forceinline__ double dtc_target(float phi, double inv_out, double inv_in) {
  const double p = (double)phi;
  return p > 0.0 ? p * inv_out : (p < 0.0 ? -(1.0 - p) * inv_in : 0.0);
}

template <int C>
__device__ __forceinline__ void dtc_extents(const float* __restrict__ ext, double (&io)[C], double (&ii)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float mo = ext[2 * c], mi = ext[2 * c + 1];
    io[c] = mo > 0.f ? 1.0 / (double)mo : 0.0;
    ii[c] = 1.0 / (1.0 + (double)mi);
  }
}

// phi of the group's four pixels in C planes of `hw` elements from pixel p; the scalar path reads the live ones and zeroes the rest
template <int C, bool WIDE>
__device__ __forceinline__ void dtc_phi(const float* __restrict__ img, int64_t hw, int64_t p, int nlive, float (&ph)[4][C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if constexpr (WIDE) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(img + c * hw + p);
#pragma unroll
      for (int i = 0; i < 4; ++i) ph[i][c] = t[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) ph[i][c] = i < nlive ? img[c * hw + p + i] : 0.f;
    }
  }
}

__device__ __forceinline__ void dtc_pin(float& v) { asm volatile("" : "+v"(v)); }

// between the two gradients' stores (cps_store_gap of cps.hip): the address arithmetic of the second may recycle the data registers of
// the first one's last 16-byte store
__device__ __forceinline__ void dtc_store_gap() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 3" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------- extents
// block (plane, slab of `per` elements; per % 4 == 0); ext [planes][2] as unsigned, zero on entry
template <bool WIDE>
__global__ __launch_bounds__(256) void dtc_extent_kernel(const float* __restrict__ phi, int64_t hw, int slabs, int64_t per,
                                                         unsigned* __restrict__ ext) {
  const int pl = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* img = phi + (int64_t)pl * hw;
  float mo = 0.f, mi = 0.f;  // a compare, not fmaxf: -0.0 and a NaN never replace +0.0, so the bits stay those of a value >= +0
  for (int64_t p = r0 + (int64_t)threadIdx.x * 4; p < r1; p += 256 * 4) {
    float v[4];
    if constexpr (WIDE) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(img + p);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = t[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p + i < r1 ? img[p + i] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      mo = v[i] > mo ? v[i] : mo;
      mi = -v[i] > mi ? -v[i] : mi;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float a = __shfl_xor(mo, o, 64), b = __shfl_xor(mi, o, 64);
    mo = a > mo ? a : mo;
    mi = b > mi ? b : mi;
  }
  __shared__ float sh[4][2];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) { sh[w][0] = mo; sh[w][1] = mi; }
  __syncthreads();
  if (threadIdx.x < 2) {
    float m = sh[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < 4; ++k) m = sh[k][threadIdx.x] > m ? sh[k][threadIdx.x] : m;
    atomicMax(ext + (size_t)pl * 2 + threadIdx.x, __float_as_uint(m));  // non-negative floats order like their bit patterns
  }
}

// ---------------------------------------------------------------- forward
// block (image, slab of `per` pixels; per % 4 == 0); ws [nb * slabs][2][2] = (hi, lo) of the block's sums for L_cons and L_sdf
template <int K1, int ZM, int RM>
__global__ __launch_bounds__(256) void dtc_fwd_kernel(const float* __restrict__ z, const float* __restrict__ r,
                                                      const float* __restrict__ phi, const float* __restrict__ ext, int lb, float kf,
                                                      int64_t hw, LossGeom gz, LossGeom gr, int slabs, int64_t per,
                                                      float* __restrict__ ws) {
  constexpr int C = K1 - 1;
  constexpr bool WIDE = ZM != CS_SCALAR;
  static_assert((ZM == CS_SCALAR) == (RM == CS_SCALAR), "both tensors on the 16-byte path or both on the scalar path");
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* zi = z + b * gz.sn;
  const float* ri = r + b * gr.sn;
  const bool lab = b < lb;  // uniform in the block
  const float* pi = lab ? phi + (int64_t)b * C * hw : nullptr;
  double io[C], ii[C];
  if (lab) dtc_extents<C>(ext + (size_t)b * C * 2, io, ii);
  const double k = (double)kf;
  double acc_c = 0.0, acc_s = 0.0;
  for (int64_t p = r0 + (int64_t)threadIdx.x * 4; p < r1; p += 256 * 4) {
    const int nlive = r1 - p < 4 ? (int)(r1 - p) : 4;  // 4 on the 16-byte path (hw % 4 == 0)
    float vz[4][K1], vr[4][C], ph[4][C];
    px4_load<K1, ZM>(zi, p, nlive, gz, vz);
    px4_load<C, RM>(ri, p, nlive, gr, vr);
    if (lab) dtc_phi<C, WIDE>(pi, hw, p, nlive, ph);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < nlive) {
        double sm[K1];
        cs_softmax<K1>(vz[i], sm);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          double t, sech2, q, qq;
          dtc_tanh(vr[i][c], t, sech2);
          dtc_sigmoid(k, t, q, qq);
          const double d = q - sm[c + 1];
          acc_c += d * d;
          if (lab) {
            const double e = t - dtc_target(ph[i][c], io[c], ii[c]);
            acc_s += e * e;
          }
        }
      }
    }
  }
  // the wave's sums in double, the four waves' in double in wave order, then ONE split into (hi, lo) per quantity
  __shared__ double wsum[4][2];
  const double wc = wave_sum_d(acc_c), wsd = wave_sum_d(acc_s);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) { wsum[w][0] = wc; wsum[w][1] = wsd; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double tot = ((wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + wsum[2][threadIdx.x]) + wsum[3][threadIdx.x];
    float pr[2];
    loss_split(tot, pr);
    ws[(size_t)blockIdx.x * 4 + threadIdx.x * 2] = pr[0];
    ws[(size_t)blockIdx.x * 4 + threadIdx.x * 2 + 1] = pr[1];
  }
}

// one block of 256 threads: out[3] = {L, L_cons, L_sdf}, coef[2]
__global__ __launch_bounds__(256) void dtc_finalize_kernel(const float* __restrict__ ws, int nparts, double n_cons, double n_sdf,
                                                           const float* __restrict__ dyn, float* __restrict__ coef,
                                                           float* __restrict__ out) {
  const LossTotals tot = loss_totals<2, 0>(ws, nullptr, nparts, 2);
  __shared__ float res[3], cf[2];  // results and coefficients are parked here and leave by one 4-byte store per lane
  if (threadIdx.x == 0) {
    const double w0 = dyn ? (double)dyn[0] : 1.0, w1 = dyn ? (double)dyn[1] : 1.0;
    const double lc = tot.f[0] / n_cons;
    const double ls = n_sdf > 0.0 ? tot.f[1] / n_sdf : 0.0;  // no labelled image: 0, never 0 / 0
    res[0] = (float)(w0 * lc + w1 * ls);
    res[1] = (float)lc;
    res[2] = (float)ls;
    cf[0] = (float)(2.0 * w0 / n_cons);
    cf[1] = n_sdf > 0.0 ? (float)(2.0 * w1 / n_sdf) : 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = res[threadIdx.x];
  else if (threadIdx.x >= 64 && threadIdx.x < 66) coef[threadIdx.x - 64] = cf[threadIdx.x - 64];
}

// ---------------------------------------------------------------- backward
// a thread per group of four pixels (`groups` per image); dz and dr have the layout class of z and r on the 16-byte path
template <int K1, int ZM, int RM>
__global__ __launch_bounds__(256) void dtc_bwd_kernel(const float* __restrict__ z, const float* __restrict__ r,
                                                      const float* __restrict__ phi, const float* __restrict__ ext,
                                                      const float* __restrict__ coef, const float* __restrict__ gout,
                                                      float* __restrict__ dz, float* __restrict__ dr, int lb, float kf, int64_t hw,
                                                      int64_t groups, int64_t total, LossGeom gz, LossGeom gr, LossGeom gdz,
                                                      LossGeom gdr) {
  constexpr int C = K1 - 1;
  constexpr bool WIDE = ZM != CS_SCALAR;
  static_assert((ZM == CS_SCALAR) == (RM == CS_SCALAR), "both tensors on the 16-byte path or both on the scalar path");
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t b = idx / groups, p = (idx - b * groups) * 4;
  const int nlive = hw - p < 4 ? (int)(hw - p) : 4;
  const double go = (double)(gout ? gout[0] : 1.f);
  const double c0 = go * (double)coef[0], c1 = go * (double)coef[1], k = (double)kf;
  const bool lab = b < lb;
  float vz[4][K1], vr[4][C], ph[4][C], gz4[4][K1], gr4[4][C];
  px4_load<K1, ZM>(z + b * gz.sn, p, nlive, gz, vz);
  px4_load<C, RM>(r + b * gr.sn, p, nlive, gr, vr);
  double io[C], ii[C];
  if (lab) {
    dtc_extents<C>(ext + (size_t)b * C * 2, io, ii);
    dtc_phi<C, WIDE>(phi + b * C * hw, hw, p, nlive, ph);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sm[K1], e[K1];
    cs_softmax<K1>(vz[i], sm);
    e[0] = 0.0;
    double dot = 0.0;
    float tr[C];  // not gr4[i] / gz4[i] themselves (bcp.hip, w2s.hip)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double t, sech2, q, qq;
      dtc_tanh(vr[i][c], t, sech2);
      dtc_sigmoid(k, t, q, qq);
      const double d = q - sm[c + 1];
      e[c + 1] = -d;
      dot += sm[c + 1] * e[c + 1];
      double a = c0 * d * (-k * qq);
      if (lab) a += c1 * (t - dtc_target(ph[i][c], io[c], ii[c]));
      tr[c] = (float)(a * sech2);
    }
    float tz[K1];
#pragma unroll
    for (int j = 0; j < K1; ++j) tz[j] = (float)(c0 * sm[j] * (e[j] - dot));
#pragma unroll
    for (int c = 0; c < C; ++c) gr4[i][c] = tr[c];
#pragma unroll
    for (int j = 0; j < K1; ++j) gz4[i][j] = tz[j];
  }
  float* zd = dz + b * gdz.sn;
  float* rd = dr + b * gdr.sn;
  if constexpr (WIDE) {
    // Every gradient value exists before the first store.  Left alone, the compiler computes each value right in front of the store
    // that takes it, in the data registers of the store before (store-data hazard, common.h: a VALU write 3 wait states behind a
    // 16-byte store).  An empty statement that names the value pins it; no instruction is emitted.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < K1; ++j) dtc_pin(gz4[i][j]);
#pragma unroll
      for (int c = 0; c < C; ++c) dtc_pin(gr4[i][c]);
    }
    cs_store<K1, ZM>(zd, p, gdz, gz4);
    dtc_store_gap();
    cs_store<C, RM>(rd, p, gdr, gr4);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nlive) {
        float t[1][K1], u[1][C];
#pragma unroll
        for (int j = 0; j < K1; ++j) t[0][j] = gz4[i][j];
#pragma unroll
        for (int c = 0; c < C; ++c) u[0][c] = gr4[i][c];
        cs_store<K1, CS_SCALAR>(zd, p + i, gdz, t);
        cs_store<C, CS_SCALAR>(rd, p + i, gdr, u);
      }
  }
}

// ---------------------------------------------------------------- host side
template <int K1, int ZM, int RM>
static void dtc_launch_fwd(hipStream_t st, const float* z, const float* r, const float* phi, const float* ext, int nb, int lb, float k,
                           int64_t hw, const LossGeom& gz, const LossGeom& gr, int slabs, float* ws) {
  const int64_t per = ceil_div64(ceil_div64(hw, 4), slabs) * 4;
  hipLaunchKernelGGL((dtc_fwd_kernel<K1, ZM, RM>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, z, r, phi, ext, lb, k, hw, gz, gr,
                     slabs, per, ws);
}

template <int K1, int ZM, int RM>
static void dtc_launch_bwd(hipStream_t st, const float* z, const float* r, const float* phi, const float* ext, const float* coef,
                           const float* gout, float* dz, float* dr, int nb, int lb, float k, int64_t hw, const LossGeom& gz,
                           const LossGeom& gr, const LossGeom& gdz, const LossGeom& gdr) {
  const int64_t groups = ceil_div64(hw, 4), total = (int64_t)nb * groups;
  hipLaunchKernelGGL((dtc_bwd_kernel<K1, ZM, RM>), dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, z, r, phi, ext, coef,
                     gout, dz, dr, lb, k, hw, groups, total, gz, gr, gdz, gdr);
}

// FN<K1, ZM, RM>(args...) for the run-time (k1 in 2..8, sm, tm): CS_DISPATCH without the one-class case, which has no level-set head
#define DTC_DISPATCH(FN, ...)                           \
  switch (k1) {                                         \
    case 2: CS_MODES(FN, 2, __VA_ARGS__); break;        \
    case 3: CS_MODES(FN, 3, __VA_ARGS__); break;        \
    case 4: CS_MODES(FN, 4, __VA_ARGS__); break;        \
    case 5: CS_MODES(FN, 5, __VA_ARGS__); break;        \
    case 6: CS_MODES(FN, 6, __VA_ARGS__); break;        \
    case 7: CS_MODES(FN, 7, __VA_ARGS__); break;        \
    default: CS_MODES(FN, 8, __VA_ARGS__); break;       \
  }

static int dtc_check(const char* who, int nb, int lb, int64_t hw, int k1, bool have_phi) {
  MIA_CHECK_ARG(k1 >= 2 && k1 <= LOSS_MAXK, "%s: k1=%d not in [2,%d]", who, k1, LOSS_MAXK);
  MIA_CHECK_ARG(nb > 0 && hw > 0 && hw <= 0x7fffffff && (int64_t)nb * hw <= 0x7fffffff,
                "%s: bad shape nb=%d hw=%lld (nb * hw must stay below 2^31)", who, nb, (long long)hw);
  MIA_CHECK_ARG(lb >= 0 && lb <= nb, "%s: lb=%d not in [0, nb=%d]", who, lb, nb);
  MIA_CHECK_ARG(lb == 0 || have_phi, "%s: labelled images need phi and their extents", who);
  return MIA_OK;
}

static bool dtc_geom_ok(const LossGeom& g) { return g.sn >= 0 && g.sk >= 0 && g.sp >= 0; }

extern "C" int mia_sdm_extent(const float* phi, int planes, int64_t hw, float* extent, void* stream) {
  MIA_CHECK_ARG(phi && extent, "mia_sdm_extent: null pointer");
  MIA_CHECK_ARG(planes > 0 && hw > 0 && hw <= 0x7fffffff && (int64_t)planes * hw <= 0x7fffffff,
                "mia_sdm_extent: bad shape planes=%d hw=%lld (planes * hw must stay below 2^31)", planes, (long long)hw);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int slabs = (int)(hw / 8192 < 1 ? 1 : (hw / 8192 > 64 ? 64 : hw / 8192));
  MIA_CHECK_ARG((int64_t)planes * slabs <= 0x7fffffff, "mia_sdm_extent: too many planes (%d)", planes);
  const int64_t per = ceil_div64(ceil_div64(hw, 4), slabs) * 4;
  const hipError_t e = hipMemsetAsync(extent, 0, (size_t)planes * 2 * sizeof(float), st);
  if (e != hipSuccess) {
    mia_set_error("mia_sdm_extent: %s", hipGetErrorString(e));
    return (int)e;
  }
  unsigned* ex = reinterpret_cast<unsigned*>(extent);
  const dim3 grid((unsigned)(planes * slabs));
  if (hw % 4 == 0 && cs_al16(phi)) hipLaunchKernelGGL(dtc_extent_kernel<true>, grid, dim3(256), 0, st, phi, hw, slabs, per, ex);
  else hipLaunchKernelGGL(dtc_extent_kernel<false>, grid, dim3(256), 0, st, phi, hw, slabs, per, ex);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_dtc_fwd(const float* z, const float* r, const float* phi, const float* extent, int nb, int lb, int64_t hw, int k1,
                           float k, int64_t sn, int64_t sk, int64_t sp, int64_t rsn, int64_t rsk, int64_t rsp, int slabs,
                           float* workspace, void* stream) {
  MIA_CHECK_ARG(z && r && workspace, "mia_dtc_fwd: null pointer");
  if (const int e = dtc_check("mia_dtc_fwd", nb, lb, hw, k1, phi && extent)) return e;
  MIA_CHECK_ARG(slabs > 0 && (int64_t)nb * slabs * 4 <= 0x7fffffff, "mia_dtc_fwd: bad shape nb=%d slabs=%d", nb, slabs);
  const LossGeom gz{sn, sk, sp}, gr{rsn, rsk, rsp};
  MIA_CHECK_ARG(dtc_geom_ok(gz) && dtc_geom_ok(gr), "mia_dtc_fwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int sm = cs_mode(z, gz, k1), tm = cs_mode(r, gr, k1 - 1);
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || (lb > 0 && !cs_al16(phi))) sm = tm = CS_SCALAR;
  DTC_DISPATCH(dtc_launch_fwd, st, z, r, phi, extent, nb, lb, k, hw, gz, gr, slabs, workspace);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_dtc_finalize(const float* workspace, const float* dyn_dev, int nb, int lb, int64_t hw, int k1, int slabs,
                                float* coef, float* out, void* stream) {
  MIA_CHECK_ARG(workspace && coef && out, "mia_dtc_finalize: null pointer");
  if (const int e = dtc_check("mia_dtc_finalize", nb, lb, hw, k1, true)) return e;
  MIA_CHECK_ARG(slabs > 0 && (int64_t)nb * slabs * 4 <= 0x7fffffff, "mia_dtc_finalize: bad shape nb=%d slabs=%d", nb, slabs);
  const double per = (double)(k1 - 1) * (double)hw;
  hipLaunchKernelGGL(dtc_finalize_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), workspace, nb * slabs,
                     (double)nb * per, (double)lb * per, dyn_dev, coef, out);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_dtc_bwd(const float* z, const float* r, const float* phi, const float* extent, const float* coef,
                           const float* grad_out, float* dz, float* dr, int nb, int lb, int64_t hw, int k1, float k, int64_t sn,
                           int64_t sk, int64_t sp, int64_t rsn, int64_t rsk, int64_t rsp, int64_t gsn, int64_t gsk, int64_t gsp,
                           int64_t hsn, int64_t hsk, int64_t hsp, void* stream) {
  MIA_CHECK_ARG(z && r && coef && dz && dr, "mia_dtc_bwd: null pointer");
  if (const int e = dtc_check("mia_dtc_bwd", nb, lb, hw, k1, phi && extent)) return e;
  const LossGeom gz{sn, sk, sp}, gr{rsn, rsk, rsp}, gdz{gsn, gsk, gsp}, gdr{hsn, hsk, hsp};
  MIA_CHECK_ARG(dtc_geom_ok(gz) && dtc_geom_ok(gr) && dtc_geom_ok(gdz) && dtc_geom_ok(gdr), "mia_dtc_bwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int sm = cs_mode(z, gz, k1), tm = cs_mode(r, gr, k1 - 1);
  // four pixels per unit: as the forward, and each gradient in the layout class of its logits
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || (lb > 0 && !cs_al16(phi)) || cs_mode(dz, gdz, k1) != sm ||
      cs_mode(dr, gdr, k1 - 1) != tm)
    sm = tm = CS_SCALAR;
  DTC_DISPATCH(dtc_launch_bwd, st, z, r, phi, extent, coef, grad_out, dz, dr, nb, lb, k, hw, gz, gr, gdz, gdr);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
