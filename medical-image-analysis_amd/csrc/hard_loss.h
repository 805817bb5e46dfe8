// The hard-label Dice + CE core of the streaming losses over ONE logits tensor and per-pixel byte maps (bcp.hip with R = 2 regions,
// w2s.hip with R = 1).  Every pixel has a label y, belongs to at most one of R regions, and with p = softmax(z) adds to its region's
//   I_k = sum p_k [y = k]   Z_k = sum p_k^2   Y_k = sum [y = k]   N = sum 1   CE = sum (logsumexp(z) - z[y])     (Y, N exact integers)
// in double.  A region's Dice term and the coefficients of its gradient come from the totals:
//   D = (1/K) sum_k (1 - (2 I_k + s) / (Z_k + Y_k + s)),  C = CE / cden,  den_k = Z_k + Y_k + s
//   al_k = -2 wd / (K den_k),  be_k = 2 wd (2 I_k + s) / (K den_k^2),  cec = wc / cden
//   dL/dz_j = go [ cec (p_j - [j = y]) + p_j (g_j - sum_k g_k p_k) ],  g_k = al_k [y = k] + be_k p_k
// ONE definition of the accumulator, the forward pixel, the parking of a block's sums, the region's arithmetic in the finalize
// kernel, the backward pixel and the host-side checks.  What a caller keeps: how a pixel finds its label and its region, what the
// weights and the CE denominator are, the layout of its results and its bad-input protocol.
#pragma once
#include "pixel_stream.h"

template <int K1, int R>
struct HlAcc {
  double si[R][K1], sz[R][K1], ce[R];
  int cy[R][K1], cn[R];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ce[r] = 0.0;
      cn[r] = 0;
#pragma unroll
      for (int k = 0; k < K1; ++k) { si[r][k] = 0.0; sz[r][k] = 0.0; cy[r][k] = 0; }
    }
  }
};

// one pixel: label y (-1: none, its CE term is 0), in[r]: it adds to region r (none: a pixel past the end of the image, or dropped).
// Every index into the accumulators is a constant; the region is chosen by predication, so no register array is indexed at run time
// (an indexed one would live in scratch memory).
template <int K1, int R>
__device__ __forceinline__ void hl_fwd_pixel(const float (&v)[K1], int y, const bool (&in)[R], HlAcc<K1, R>& a) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < K1; ++k) mx = fmaxf(mx, v[k]);
  double p[K1];
  cs_softmax<K1>(v, p);
  const double term = y >= 0 ? cs_nll_term<K1>(v, y, mx, cs_max<K1>(p)) : 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    a.ce[r] += in[r] ? term : 0.0;
    a.cn[r] += in[r];
  }
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    const bool t = y == k;
    const double q = p[k] * p[k];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      a.si[r][k] += (in[r] && t) ? p[k] : 0.0;
      a.sz[r][k] += in[r] ? q : 0.0;
      a.cy[r][k] += in[r] && t;
    }
  }
}

// The end of a forward block.  Per region r the block's slice of the workspace holds wf_r [2 K1 + 1][2]: the (hi, lo) pairs of I_rk,
// Z_rk, CE_r, and after the pairs of all regions wn_r [NC]: Y_rk, N_r and, in the last region, NX counts `extra` of the caller's.
// Holds the block's one barrier.
template <int K1, int R, int NX>
__device__ __forceinline__ void hl_park(const HlAcc<K1, R>& acc, const int* extra, float* __restrict__ ws, int nparts) {
  constexpr int NQ = 2 * K1 + 1, NC = K1 + 1 + NX;
  static_assert(NX == 0 || R == 1, "extra counts have a slot in every region and are written in the last only");
  auto red = loss_block_sums<2 * R * NQ, R * NC>();
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      cs_park(red, (r * NQ + k) * 2, acc.si[r][k]);
      cs_park(red, (r * NQ + K1 + k) * 2, acc.sz[r][k]);
      const int c = wave_sum_i(acc.cy[r][k]);
      if (red.l == 0) red.i[red.w][r * NC + k] = c;
    }
    cs_park(red, (r * NQ + 2 * K1) * 2, acc.ce[r]);
    const int c = wave_sum_i(acc.cn[r]);
    if (red.l == 0) red.i[red.w][r * NC + K1] = c;
  }
#pragma unroll
  for (int x = 0; x < NX; ++x) {
    const int c = wave_sum_i(extra[x]);
    if (red.l == 0) red.i[red.w][(R - 1) * NC + K1 + 1 + x] = c;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < R * 2 * NQ) {  // region t / (2 NQ), word t % (2 NQ) of this block's pairs
    const int r = R == 1 ? 0 : t / (2 * NQ), j = t - r * (2 * NQ);
    ws[((size_t)r * nparts + blockIdx.x) * (2 * NQ) + j] = red.sum_f(t);
  } else if (t >= 128 && t < 128 + R * NC) {
    const int r = R == 1 ? 0 : (t - 128) / NC, j = (t - 128) - r * NC;
    int* wn = reinterpret_cast<int*>(ws + (size_t)R * nparts * (2 * NQ));
    wn[((size_t)r * nparts + blockIdx.x) * NC + j] = red.sum_i(t - 128);
  }
}

// One region in the finalize kernel (one thread): its totals tf [2 K1 + 1], tn [K1 + 1], the weights wd, wc of its Dice and CE terms
// in the loss and the CE denominator cden -> D, C and the coefficients cf [2 K1 + 1] = {al_k}, {be_k}, cec.  An empty region has no
// term, and no pixel reads its coefficients.
template <int K1>
__device__ __forceinline__ void hl_region(const double* tf, const long long* tn, double s, double wd, double wc, double cden, double& d,
                                          double& c, float* cf) {
  d = c = 0.0;
  if (tn[K1] > 0) {
    for (int k = 0; k < K1; ++k) {
      const double num = 2.0 * tf[k] + s, den = tf[K1 + k] + (double)tn[k] + s;
      d += 1.0 - num / den;
      cf[k] = (float)(wd * (-2.0 / ((double)K1 * den)));
      cf[K1 + k] = (float)(wd * (2.0 * num / ((double)K1 * den * den)));
    }
    d /= (double)K1;
    c = tf[2 * K1] / cden;
    cf[2 * K1] = (float)(wc / cden);
  } else {
    for (int k = 0; k < 2 * K1 + 1; ++k) cf[k] = 0.f;
  }
}

// one pixel of the backward: its region's coefficients cf and go = grad_out -> d; a pixel that is not kept gets exactly 0.0f
template <int K1>
__device__ __forceinline__ void hl_bwd_pixel(const float (&v)[K1], int y, bool kept, const float (&cf)[2 * K1 + 1], double go,
                                             float (&d)[K1]) {
  if (kept) {
    double pr[K1], gk[K1], dot = 0.0;
    cs_softmax<K1>(v, pr);
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      gk[k] = (y == k ? (double)cf[k] : 0.0) + (double)cf[K1 + k] * pr[k];
      dot += gk[k] * pr[k];
    }
    const double cec = (double)cf[2 * K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) d[k] = (float)(go * (cec * (pr[k] - (y == k ? 1.0 : 0.0)) + pr[k] * (gk[k] - dot)));
  } else {
#pragma unroll
    for (int k = 0; k < K1; ++k) d[k] = 0.f;
  }
}

// ---- host side
// The checks of the loss entry points after their pointers, with the texts the callers match on.  A forward gives its workspace
// words per block (`slabs` blocks per image); a backward gives 0 and the gradient's strides.
static int hl_check(const char* who, int nb, int64_t hw, int k1, int slabs, size_t words, const LossGeom& g, const LossGeom* gd,
                    int64_t mask_sn) {
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "%s: k1=%d not in [1,%d]", who, k1, LOSS_MAXK);
  const bool shape = nb > 0 && hw > 0 && hw <= 0x7fffffff && (int64_t)nb * hw <= 0x7fffffff;
  if (words)
    MIA_CHECK_ARG(shape && slabs > 0 && (int64_t)nb * slabs * (int64_t)words <= 0x7fffffff, "%s: bad shape nb=%d hw=%lld slabs=%d", who,
                  nb, (long long)hw, slabs);
  else
    MIA_CHECK_ARG(shape, "%s: bad shape nb=%d hw=%lld", who, nb, (long long)hw);
  MIA_CHECK_ARG(g.sn >= 0 && g.sk >= 0 && g.sp >= 0 && (!gd || (gd->sn >= 0 && gd->sk >= 0 && gd->sp >= 0)) &&
                    (mask_sn == 0 || mask_sn == hw),
                "%s: bad strides", who);
  return MIA_OK;
}
