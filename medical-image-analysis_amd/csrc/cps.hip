// Cross pseudo supervision on the GPU (gfx950): two networks, each trained on the hard pseudo-labels of the other (CPS: Chen et al.,
// CVPR 2021).  Logits za, zb [nb][k1][hw] fp32, N = nb * hw, per pixel:
//   ya = argmax_k za_k, yb = argmax_k zb_k       on the fp32 logits themselves, a tie goes to the LOWEST index (numpy.argmax)
//   ca = [max_k softmax(za)_k >= tau], cb likewise    the confidence of the label SOURCE; tau = dyn[1], 0 keeps every pixel
//   LA = (1/N) sum cb (logsumexp(za) - za[yb]),  LB = (1/N) sum ca (logsumexp(zb) - zb[ya])
// The denominator is always N (the FixMatch form): tau = 0 is F.cross_entropy(za, yb) + F.cross_entropy(zb, ya), an empty mask
// gives 0 and not NaN.  -log p is logsumexp(z) - z_y = -log(max_k p_k) + (max_k z_k - z_y): the first term lies in [0, ln k1], the
// second is an exact difference of two fp32 values in double, so a label whose soft-max is 0 in fp32 still has a finite term.
//   out = {w (LA + LB), LA, LB, w}, w = dyn[0];  dyn NULL: w = 1, tau = 0
//   dLA/dza_j = (w/N) cb (pa_j - [j = yb]), symmetric for zb; labels and flags carry no gradient; a pixel whose flag is clear
//   gets exactly 0.0f
//   counts = {sum ca, sum cb, sum [ya = yb]} as int64;  code [nb][hw] = ya | yb << 3 | ca << 6 | cb << 7, one byte per pixel
//   cps_fwd_kernel       block (image, slab of pixels): streams za and zb by their own (sn, sk, sp) strides; both soft-maxes in double
//                        per pixel (cs_softmax); writes `code` (one 4-byte store per four pixels on the wide path) and per-block
//                        partials through LossBlockSums: the two sums as (hi, lo) float pairs and the three counts as ints
//   cps_finalize_kernel  one block: the partials in a fixed order in double / int64 -> out[4], counts[3]
//   cps_bwd_kernel       one streaming pass, a thread per pixel group: za, zb and `code` in, dza AND dzb out -- the backward reads
//                        `code` instead of recomputing arg-max and threshold, so both directions agree on every pixel by construction
// Layouts as consistency.hip (pixel_stream.h): planar and channels-last tensors take four pixels per thread with 16-byte accesses
// when hw % 4 == 0 and pointers / strides are 16-byte aligned, anything else one pixel per thread; the two networks may differ in
// layout, and each gradient has the layout class of its logits.  No float atomics: bit-identical from run to run; an image's code
// does not depend on the rest of the batch; nothing synchronises with the host.
#include "pixel_stream.h"

#define CPS_WORDS 7  // per block: (hi, lo) of the two sums, three counts

// The arg-max (cs_argmax) and logsumexp(v) - v[y] for the label y of the OTHER network (cs_nll_term) are in pixel_stream.h.
// one pixel of the forward: its code byte; the two terms and the three counts are added to the thread's running sums
template <int K1>
__device__ __forceinline__ unsigned cps_fwd_pixel(const float (&a)[K1], const float (&t)[K1], double tau, double& acc_a, double& acc_b,
                                                  int (&cnt)[3]) {
  float ma, mb;
  const int ya = cs_argmax<K1>(a, ma), yb = cs_argmax<K1>(t, mb);
  double pa[K1], pb[K1];
  cs_softmax<K1>(a, pa);
  cs_softmax<K1>(t, pb);
  const double qa = cs_max<K1>(pa), qb = cs_max<K1>(pb);  // max_k p_k = 1 / sum_k exp(z_k - max)
  const bool ca = qa >= tau, cb = qb >= tau;                // a NaN keeps nothing
  if (cb) acc_a += cs_nll_term<K1>(a, yb, ma, qa);
  if (ca) acc_b += cs_nll_term<K1>(t, ya, mb, qb);
  cnt[0] += ca;
  cnt[1] += cb;
  cnt[2] += ya == yb;
  return (unsigned)ya | (unsigned)yb << 3 | (unsigned)ca << 6 | (unsigned)cb << 7;
}

// block (image, slab of `per` pixels; per % PX == 0).  ws [nb * slabs][4] = (hi, lo) of the block's sums of cb * termA and ca * termB;
// wsn [nb * slabs][3] = its counts of ca, cb and ya == yb.
template <int K1, int AM, int BM>
__global__ __launch_bounds__(256) void cps_fwd_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                      const float* __restrict__ dyn, int64_t hw, LossGeom ga, LossGeom gb, int slabs,
                                                      int64_t per, float* __restrict__ ws, int* __restrict__ wsn,
                                                      unsigned char* __restrict__ code) {
  constexpr int PX = CS_PX(AM);
  static_assert(CS_PX(AM) == CS_PX(BM), "both networks take the same number of pixels per thread");
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* ia = za + b * ga.sn;
  const float* ib = zb + b * gb.sn;
  const double tau = dyn ? (double)dyn[1] : 0.0;
  double acc_a = 0.0, acc_b = 0.0;
  int cnt[3] = {0, 0, 0};
  for (int64_t p = r0 + (int64_t)threadIdx.x * PX; p < r1; p += 256 * PX) {
    float a[PX][K1], t[PX][K1];
    cs_load<K1, AM>(ia, p, ga, a);
    cs_load<K1, BM>(ib, p, gb, t);
    unsigned bits = cps_fwd_pixel<K1>(a[0], t[0], tau, acc_a, acc_b, cnt);
    if constexpr (PX == 4) {  // written out: every index into a and t is a constant before any loop is unrolled
      bits |= cps_fwd_pixel<K1>(a[1], t[1], tau, acc_a, acc_b, cnt) << 8;
      bits |= cps_fwd_pixel<K1>(a[2], t[2], tau, acc_a, acc_b, cnt) << 16;
      bits |= cps_fwd_pixel<K1>(a[3], t[3], tau, acc_a, acc_b, cnt) << 24;
    }
    unsigned char* cd = code + (int64_t)b * hw + p;
    if (PX == 4)  // one 4-byte store; b * hw + p is a multiple of 4
      *reinterpret_cast<unsigned*>(cd) = bits;
    else
      cd[0] = (unsigned char)bits;
  }
  // the wave's sums in double first, so that the float pairs below are added four at a time only
  auto red = loss_block_sums<4, 3>();
  float part[4];
  loss_wave_pair(acc_a, red.l, part);
  loss_wave_pair(acc_b, red.l, part + 2);
  red.put(0, part, 0, cnt);
  __syncthreads();
  if (threadIdx.x < 4) ws[(size_t)blockIdx.x * 4 + threadIdx.x] = red.sum_f(threadIdx.x);
  else if (threadIdx.x < 7) wsn[(size_t)blockIdx.x * 3 + (threadIdx.x - 4)] = red.sum_i(threadIdx.x - 4);
}

// one block: out = {weight (LA + LB), LA, LB, weight}; counts = {sum ca, sum cb, sum [ya == yb]}
__global__ void cps_finalize_kernel(const float* __restrict__ ws, const int* __restrict__ wsn, int nparts, double n_all,
                                    const float* __restrict__ dyn, float* __restrict__ out, long long* __restrict__ counts) {
  const LossTotals tot = loss_totals<2, 3>(ws, wsn, nparts, 2);
  __shared__ float res[4];
  if (threadIdx.x == 0) {
    const double la = tot.f[0] / n_all, lb = tot.f[1] / n_all;
    const float wt = dyn ? dyn[0] : 1.f;
    res[0] = (float)((double)wt * (la + lb));
    res[1] = (float)la;
    res[2] = (float)lb;
    res[3] = wt;
  }
  __syncthreads();
  if (threadIdx.x < 4) out[threadIdx.x] = res[threadIdx.x];  // one 4-byte store per lane
  else if (threadIdx.x < 7) counts[threadIdx.x - 4] = tot.n[threadIdx.x - 4];
}

// Between the two gradients: the address arithmetic of the second one may recycle the data registers of the first one's last
// 16-byte store (store-data hazard, common.h), and store_data_pad()'s wait states are free to sink behind that arithmetic.  Nothing
// crosses a full scheduling barrier, so these wait states stay where they are written.
__device__ __forceinline__ void cps_store_gap() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 3" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// a thread per group of PX pixels; each gradient has the layout class of its logits (its own strides) on the four-pixel path
template <int K1, int AM, int BM>
__global__ __launch_bounds__(256) void cps_bwd_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                      const unsigned char* __restrict__ code, const float* __restrict__ dyn,
                                                      const float* __restrict__ gout, float* __restrict__ dza,
                                                      float* __restrict__ dzb, int64_t hw, int64_t total, double inv_n, LossGeom ga,
                                                      LossGeom gb, LossGeom gda, LossGeom gdb) {
  constexpr int PX = CS_PX(AM);
  static_assert(CS_PX(AM) == CS_PX(BM), "both networks take the same number of pixels per thread");
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int64_t per = hw / PX, b = idx / per, p = (idx - b * per) * PX;
  const double sc = (double)(gout ? gout[0] : 1.f) * (double)(dyn ? dyn[0] : 1.f) * inv_n;
  float a[PX][K1], t[PX][K1], da[PX][K1], db[PX][K1];
  cs_load<K1, AM>(za + b * ga.sn, p, ga, a);
  cs_load<K1, BM>(zb + b * gb.sn, p, gb, t);
  const unsigned char* cd = code + b * hw + p;
  const unsigned bits = PX == 4 ? *reinterpret_cast<const unsigned*>(cd) : (unsigned)cd[0];
#pragma unroll
  for (int i = 0; i < PX; ++i) {
    const unsigned c = (bits >> (8 * i)) & 0xffu;
    const int ya = (int)(c & 7u), yb = (int)((c >> 3) & 7u);
    if (c & 0x80u) {  // cb: network B's label is trusted, network A learns from it
      double pa[K1];
      cs_softmax<K1>(a[i], pa);
#pragma unroll
      for (int k = 0; k < K1; ++k) da[i][k] = (float)(sc * (pa[k] - (k == yb ? 1.0 : 0.0)));
    } else {
#pragma unroll
      for (int k = 0; k < K1; ++k) da[i][k] = 0.f;  // a dropped pixel: exactly zero
    }
    if (c & 0x40u) {  // ca
      double pb[K1];
      cs_softmax<K1>(t[i], pb);
#pragma unroll
      for (int k = 0; k < K1; ++k) db[i][k] = (float)(sc * (pb[k] - (k == ya ? 1.0 : 0.0)));
    } else {
#pragma unroll
      for (int k = 0; k < K1; ++k) db[i][k] = 0.f;
    }
  }
  cs_store<K1, AM>(dza + b * gda.sn, p, gda, da);
  cps_store_gap();
  cs_store<K1, BM>(dzb + b * gdb.sn, p, gdb, db);
}

template <int K1, int AM, int BM>
static void cps_launch_fwd(hipStream_t st, const float* za, const float* zb, const float* dyn, int nb, int64_t hw, const LossGeom& ga,
                           const LossGeom& gb, int slabs, float* ws, int* wsn, unsigned char* code) {
  constexpr int PX = CS_PX(AM);
  const int64_t per = ceil_div64(hw / PX, slabs) * PX;  // hw % PX == 0 on the four-pixel path
  hipLaunchKernelGGL((cps_fwd_kernel<K1, AM, BM>), dim3((unsigned)(nb * slabs)), dim3(256), 0, st, za, zb, dyn, hw, ga, gb, slabs, per,
                     ws, wsn, code);
}

template <int K1, int AM, int BM>
static void cps_launch_bwd(hipStream_t st, const float* za, const float* zb, const unsigned char* code, const float* dyn,
                           const float* gout, float* dza, float* dzb, int nb, int64_t hw, const LossGeom& ga, const LossGeom& gb,
                           const LossGeom& gda, const LossGeom& gdb) {
  const int64_t total = (int64_t)nb * (hw / CS_PX(AM));
  hipLaunchKernelGGL((cps_bwd_kernel<K1, AM, BM>), dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, st, za, zb, code, dyn, gout,
                     dza, dzb, hw, total, 1.0 / ((double)nb * (double)hw), ga, gb, gda, gdb);
}

extern "C" int mia_cps_workspace(int nb, int slabs) {
  if (nb <= 0 || slabs <= 0 || (int64_t)nb * slabs * CPS_WORDS > 0x7fffffff) return -1;
  return nb * slabs * CPS_WORDS;
}

extern "C" int mia_cps_fwd(const float* za, const float* zb, const float* dyn_dev, int nb, int64_t hw, int k1, int64_t asn, int64_t ask,
                           int64_t asp, int64_t bsn, int64_t bsk, int64_t bsp, int slabs, float* workspace, unsigned char* code,
                           float* out, long long* counts, void* stream) {
  MIA_CHECK_ARG(za && zb && workspace && code && out && counts, "mia_cps_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0 && (int64_t)nb * slabs * CPS_WORDS <= 0x7fffffff && hw <= 0x7fffffff &&
                    (int64_t)nb * hw <= 0x7fffffff,
                "mia_cps_fwd: bad shape nb=%d hw=%lld slabs=%d", nb, (long long)hw, slabs);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_cps_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(asn >= 0 && ask >= 0 && asp >= 0 && bsn >= 0 && bsk >= 0 && bsp >= 0, "mia_cps_fwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom ga{asn, ask, asp}, gb{bsn, bsk, bsp};
  int sm = cs_mode(za, ga, k1), tm = cs_mode(zb, gb, k1);
  // four pixels per thread: 16-byte units in both logits and 4-byte units in the code map
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || !cs_al16(code)) sm = tm = CS_SCALAR;
  int* wsn = reinterpret_cast<int*>(workspace + (size_t)nb * slabs * 4);
  CS_DISPATCH(cps_launch_fwd, st, za, zb, dyn_dev, nb, hw, ga, gb, slabs, workspace, wsn, code);
  hipLaunchKernelGGL(cps_finalize_kernel, dim3(1), dim3(256), 0, st, workspace, wsn, nb * slabs, (double)nb * (double)hw, dyn_dev, out,
                     counts);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_cps_bwd(const float* za, const float* zb, const unsigned char* code, const float* dyn_dev, const float* grad_out,
                           float* dza, float* dzb, int nb, int64_t hw, int k1, int64_t asn, int64_t ask, int64_t asp, int64_t bsn,
                           int64_t bsk, int64_t bsp, int64_t gasn, int64_t gask, int64_t gasp, int64_t gbsn, int64_t gbsk,
                           int64_t gbsp, void* stream) {
  MIA_CHECK_ARG(za && zb && code && dza && dzb, "mia_cps_bwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && hw <= 0x7fffffff && (int64_t)nb * hw <= 0x7fffffff, "mia_cps_bwd: bad shape nb=%d hw=%lld", nb,
                (long long)hw);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_cps_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(asn >= 0 && ask >= 0 && asp >= 0 && bsn >= 0 && bsk >= 0 && bsp >= 0 && gasn >= 0 && gask >= 0 && gasp >= 0 &&
                    gbsn >= 0 && gbsk >= 0 && gbsp >= 0,
                "mia_cps_bwd: negative strides");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom ga{asn, ask, asp}, gb{bsn, bsk, bsp}, gda{gasn, gask, gasp}, gdb{gbsn, gbsk, gbsp};
  int sm = cs_mode(za, ga, k1), tm = cs_mode(zb, gb, k1);
  // four pixels per thread: as the forward, and each gradient in the layout class of its logits
  if (hw % 4 != 0 || sm == CS_SCALAR || tm == CS_SCALAR || cs_mode(dza, gda, k1) != sm || cs_mode(dzb, gdb, k1) != tm || !cs_al16(code))
    sm = tm = CS_SCALAR;
  CS_DISPATCH(cps_launch_bwd, st, za, zb, code, dyn_dev, grad_out, dza, dzb, nb, hw, ga, gb, gda, gdb);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
