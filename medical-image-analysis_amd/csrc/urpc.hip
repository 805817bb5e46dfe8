// Uncertainty rectified pyramid consistency (URPC: Luo et al., MICCAI 2021 / MedIA 2022) between the S outputs one network makes at
// several decoder scales, on the unlabelled images.  z_s [nb][k1][H / f_s][W / f_s] fp32, f_0 = 1 (the main output), the others
// factors of the deep-supervision heads (2, 4, 8, 16), brought to full resolution by the heads' own bilinear upsampling IN REGISTERS
// (ds_common.h).  Per full-resolution pixel, with P = nb H W:
//   u_s = up(z_s), p_s = softmax(u_s), lp_s = u_s - logsumexp(u_s), m = (1/S) sum_s p_s
//   v_s = sum_k m_k (log m_k - lp_sk)   (KL(m || p_s); a class with m_k == 0 adds 0),  w_s = exp(-v_s),  D_s = sum_k (m_k - p_sk)^2
//   A_s = sum D_s w_s, B_s = sum w_s, C_s = sum v_s  over all pixels  -> sums [S][3]
//   L_s = (A_s / (P k1)) / (B_s / P + 1e-8) + C_s / P -> terms [S],   L = (1/S) sum_s L_s,   out = {weight L, L}
// Backward (plain autograd of the above, m included), per pixel for scale t, with al_s = dL_s/dA_s = 1 / (P k1 b_s),
// be_s = dL_s/dB_s = -a_s / (b_s^2 P), ga = dL_s/dC_s = 1 / P, a_s = A_s / (P k1), b_s = B_s / P + 1e-8 and q = grad_out weight / S:
//   c_s = q (ga - w_s (al_s D_s + be_s))        = q dL/dv_s            e_s = q al_s w_s         = q dL/dD_s
//   G_k = sum_s [c_s (log m_k - lp_sk) + 2 e_s (m_k - p_sk)]            (the gradient of m; its class-independent part cancels below)
//   g_k = G_k / S - 2 e_t (m_k - p_tk)                                  (the gradient of p_t: through m, and direct)
//   du_tk = p_tk (g_k - sum_j g_j p_tj) - c_t (m_k - p_tk)              (soft-max Jacobian; lp_t direct: p dv/dp = -m, no division)
// and dz_t = Uy^T du_t Ux.  log p is never the log of a rounded probability, so saturated logits stay finite in both directions.
//   urpc_fwd_kernel       block (image, slab of full-resolution rows): a thread interpolates all S x k1 logits of a pixel in
//                         registers and adds the three terms per scale in double; block partials as (hi, lo) float pairs
//   urpc_finalize_kernel  one block: the partials in a fixed order in double -> sums, terms, out; weight = dyn[0] read here
//   urpc_bwd_full_kernel  f = 1: one streaming pass, a thread per pixel, dz_0 through its own strides
//   urpc_bwd_gather_kernel f > 1: the gather of ds_loss_bwd_kernel -- one block per (image, tile of low-resolution pixels): (1) every
//                         pixel of the tile's region recomputes all S scales but stores only scale t's du in LDS, (2) / (3) the
//                         separable reductions along x and y.  One launch per scale; the scale whose gradient a launch writes sits
//                         in slot 0 of its argument block (the host swaps it there: the definition is symmetric in the scales), so
//                         no register array is indexed at run time.
// Nothing of full-resolution size is stored in either direction.  No float atomics, every sum in a fixed order: out, sums, terms and
// every dz are bit-identical run to run.  Every launch goes to the caller's stream; nothing synchronises with the host.
#include "ds_common.h"

#define URPC_MAXS 5

struct UrpcScales {
  const float* z[URPC_MAXS];
  int64_t sn[URPC_MAXS];
  int sk[URPC_MAXS], sp[URPC_MAXS];  // class and pixel strides fit 32 bits (checked on the host): half the scalar registers
  int sh[URPC_MAXS];  // log2 of the factor
  int id[URPC_MAXS];  // the scale's row in sums
};

// p_s, lp_s of every scale and m at full-resolution pixel (Y, X) of image b
template <int NK, int NS>
__device__ __forceinline__ void urpc_pixel(const UrpcScales& a, int b, int Y, int X, int H, int W, int k1, float (&p)[NS][NK],
                                           float (&lp)[NS][NK], float (&m)[NK]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) m[k] = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    int sk = a.sk[s], sp = a.sp[s], sh = a.sh[s];
    const float* zb = a.z[s] + b * a.sn[s];
    // Opaque to the optimiser: otherwise every k * sk of every scale (and h, w, 1 / f) is hoisted out of the caller's pixel loop and
    // the kernel runs out of scalar registers.  Recomputing them per pixel is a handful of scalar instructions.
    asm volatile("" : "+s"(sk), "+s"(sp), "+s"(sh));
    const LossGeom g{0, sk, sp};
    float u[NK];
    if (sh == 0) {
      const int64_t o = ((int64_t)Y * W + X) * g.sp;
#pragma unroll
      for (int k = 0; k < NK; ++k) u[k] = k < k1 ? zb[o + k * g.sk] : 0.f;
    } else {
      const int h = H >> sh, w = W >> sh;
      const float scale = __int_as_float((127 - sh) << 23);  // 1 / f, exact
      ds_interp<NK>(zb, g, w, k1, ds_tap(Y, scale, h), ds_tap(X, scale, w), u);
    }
    float mx = -INFINITY, se = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) mx = fmaxf(mx, u[k]);
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) { lp[s][k] = u[k] - mx; p[s][k] = expf(lp[s][k]); se += p[s][k]; }
    const float inv = 1.f / se, lse = logf(se);
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) { p[s][k] *= inv; lp[s][k] -= lse; m[k] += p[s][k]; } else { p[s][k] = 0.f; lp[s][k] = 0.f; }
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) m[k] = m[k] / (float)NS;  // a division: S equal probabilities average to themselves exactly
}

// lm_k = log m_k (0 where m_k == 0: every p_sk is 0 there and the class adds nothing), v_s, w_s, D_s
template <int NK, int NS>
__device__ __forceinline__ void urpc_terms(const float (&p)[NS][NK], const float (&lp)[NS][NK], const float (&m)[NK], int k1,
                                           float (&lm)[NK], float (&v)[NS], float (&wt)[NS], float (&d)[NS]) {
#pragma unroll
  for (int k = 0; k < NK; ++k) lm[k] = (k < k1 && m[k] > 0.f) ? logf(m[k]) : 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float vs = 0.f, ds = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) {
        vs += m[k] * (lm[k] - lp[s][k]);
        const float e = m[k] - p[s][k];
        ds += e * e;
      }
    v[s] = vs; wt[s] = expf(-vs); d[s] = ds;
  }
}

// ---------------------------------------------------------------- forward
// part [nb * slabs][NS][3][2]: (hi, lo) of the block's sums of D_s w_s, w_s and v_s
template <int NK, int NS>
__global__ __launch_bounds__(256) void urpc_fwd_kernel(UrpcScales a, int H, int W, int k1, int slabs, float* __restrict__ part) {
  const int b = blockIdx.x / slabs, sl = blockIdx.x % slabs;
  const int per = (H + slabs - 1) / slabs;
  const int y0 = sl * per < H ? sl * per : H, y1 = y0 + per < H ? y0 + per : H;
  double acc[NS][3];
#pragma unroll
  for (int s = 0; s < NS; ++s) { acc[s][0] = 0.0; acc[s][1] = 0.0; acc[s][2] = 0.0; }
  for (int idx = threadIdx.x; idx < (y1 - y0) * W; idx += 256) {
    const int r = idx / W, Y = y0 + r, X = idx - r * W;
    float p[NS][NK], lp[NS][NK], m[NK], lm[NK], v[NS], wt[NS], d[NS];
    urpc_pixel<NK, NS>(a, b, Y, X, H, W, k1, p, lp, m);
    urpc_terms<NK, NS>(p, lp, m, k1, lm, v, wt, d);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      acc[s][0] += (double)(d[s] * wt[s]);
      acc[s][1] += (double)wt[s];
      acc[s][2] += (double)v[s];
    }
  }
  auto red = loss_block_sums<6 * NS, 0>();
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float pr[2];
      loss_wave_pair(acc[s][j], red.l, pr);
      red.put((s * 3 + j) * 2, pr);
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 3 * NS) {
    double tot = 0.0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) tot += (double)red.f[wv][2 * t] + (double)red.f[wv][2 * t + 1];
    loss_split(tot, part + ((size_t)blockIdx.x * 3 * NS + t) * 2);
  }
}

// one block of 256 threads
__global__ __launch_bounds__(256) void urpc_finalize_kernel(const float* __restrict__ part, int nparts, int ns, int k1, double npix,
                                                            const float* __restrict__ dyn, float* __restrict__ sums,
                                                            float* __restrict__ terms, float* __restrict__ out) {
  const double* tot = loss_totals<3 * URPC_MAXS, 0>(part, nullptr, nparts, 3 * ns).f;
  if ((int)threadIdx.x < 3 * ns) sums[threadIdx.x] = (float)tot[threadIdx.x];
  if (threadIdx.x == 0) {
    double l = 0.0;
    for (int s = 0; s < ns; ++s) {
      const double as = tot[3 * s] / (npix * (double)k1), bs = tot[3 * s + 1] / npix + 1e-8;
      const double ls = as / bs + tot[3 * s + 2] / npix;
      terms[s] = (float)ls;
      l += ls;
    }
    l /= (double)ns;
    const float wt = dyn ? dyn[0] : 1.f;
    out[0] = (float)((double)wt * l);
    out[1] = (float)l;
  }
}

// ---------------------------------------------------------------- backward
// al_s, be_s (see the head of the file) of the scale in every slot, and q = grad_out * weight / S
template <int NS>
__device__ __forceinline__ void urpc_coefs(const UrpcScales& a, const float* __restrict__ sums, const float* __restrict__ dyn,
                                           const float* __restrict__ gout, double npix, int k1, float (&al)[NS], float (&be)[NS], float& ga,
                                           float& q) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float* r = sums + 3 * a.id[s];
    const double as = (double)r[0] / (npix * (double)k1), bs = (double)r[1] / npix + 1e-8;
    al[s] = (float)(1.0 / (npix * (double)k1 * bs));
    be[s] = (float)(-as / (bs * bs * npix));
  }
  ga = (float)(1.0 / npix);
  q = (gout ? gout[0] : 1.f) * (dyn ? dyn[0] : 1.f) / (float)NS;
}

// du of the scale in slot 0 at one pixel
template <int NK, int NS>
__device__ __forceinline__ void urpc_du(const float (&p)[NS][NK], const float (&lp)[NS][NK], const float (&m)[NK], int k1,
                                        const float (&al)[NS], const float (&be)[NS], float ga, float q, float (&du)[NK]) {
  float lm[NK], v[NS], wt[NS], d[NS], c[NS], e[NS];
  urpc_terms<NK, NS>(p, lp, m, k1, lm, v, wt, d);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    c[s] = q * (ga - wt[s] * (al[s] * d[s] + be[s]));
    e[s] = q * al[s] * wt[s];
  }
  float g[NK], dot = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    g[k] = 0.f;
    if (k < k1) {
      float gm = 0.f;
#pragma unroll
      for (int s = 0; s < NS; ++s) gm += c[s] * (lm[k] - lp[s][k]) + 2.f * e[s] * (m[k] - p[s][k]);
      g[k] = gm / (float)NS - 2.f * e[0] * (m[k] - p[0][k]);
      dot += g[k] * p[0][k];
    }
  }
#pragma unroll
  for (int k = 0; k < NK; ++k) du[k] = k < k1 ? p[0][k] * (g[k] - dot) - c[0] * (m[k] - p[0][k]) : 0.f;
}

// slot 0 has factor 1: a thread per full-resolution pixel
template <int NK, int NS>
__global__ __launch_bounds__(256) void urpc_bwd_full_kernel(UrpcScales a, const float* __restrict__ sums, const float* __restrict__ dyn,
                                                            const float* __restrict__ gout, float* __restrict__ dz, LossGeom go, int nb,
                                                            int H, int W, int k1) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t hw = (int64_t)H * W;
  if (idx >= (int64_t)nb * hw) return;
  const int b = (int)(idx / hw), pix = (int)(idx - (int64_t)b * hw);
  const int Y = pix / W, X = pix - Y * W;
  float al[NS], be[NS], ga, q;
  urpc_coefs<NS>(a, sums, dyn, gout, (double)nb * (double)hw, k1, al, be, ga, q);
  float p[NS][NK], lp[NS][NK], m[NK], du[NK];
  urpc_pixel<NK, NS>(a, b, Y, X, H, W, k1, p, lp, m);
  urpc_du<NK, NS>(p, lp, m, k1, al, be, ga, q, du);
  float* o = dz + b * go.sn + (int64_t)pix * go.sp;
#pragma unroll
  for (int k = 0; k < NK; ++k)
    if (k < k1) o[k * go.sk] = du[k];
}

// slot 0 has factor f > 1 and h x w pixels.  LDS as in ds_loss_bwd_kernel: du [k1][RH][pitch], then tx [k1][tw][RH].
template <int NK, int NS>
__global__ __launch_bounds__(256) void urpc_bwd_gather_kernel(UrpcScales a, const float* __restrict__ sums, const float* __restrict__ dyn,
                                                              const float* __restrict__ gout, float* __restrict__ dz, LossGeom go, int nb,
                                                              int H, int W, int k1, int th, int tw, int tiles_x, int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) float urpc_smem[];
  const int factor = 1 << a.sh[0], h = H >> a.sh[0], w = W >> a.sh[0];
  const int tiles = tiles_x * tiles_y;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  const int ia = tyi * th, ja = txi * tw;
  const int nth = ia + th < h ? th : h - ia, ntw = ja + tw < w ? tw : w - ja;  // live tile
  const int Y0 = ia * factor - factor / 2, X0 = ja * factor - factor / 2;    // region origin (may lie half a cell outside)
  const int RH = (th + 1) * factor, pitch = (tw + 1) * factor + 1;             // allocated
  const int rh = (nth + 1) * factor, rw = (ntw + 1) * factor;                  // live region
  float* dus = urpc_smem;
  float* tx_s = urpc_smem + (size_t)k1 * RH * pitch;
  const float scale = 1.f / (float)factor;
  float al[NS], be[NS], ga, q;
  urpc_coefs<NS>(a, sums, dyn, gout, (double)nb * (double)H * (double)W, k1, al, be, ga, q);

  // (1) du of every full-resolution pixel of the region, once
  for (int idx = threadIdx.x; idx < rh * rw; idx += 256) {
    const int ry = idx / rw, rx = idx - ry * rw;
    const int Y = Y0 + ry, X = X0 + rx;
    float du[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) du[k] = 0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
      float p[NS][NK], lp[NS][NK], m[NK];
      urpc_pixel<NK, NS>(a, b, Y, X, H, W, k1, p, lp, m);
      urpc_du<NK, NS>(p, lp, m, k1, al, be, ga, q, du);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (k < k1) dus[((size_t)k * RH + ry) * pitch + rx] = du[k];
  }
  __syncthreads();

  // (2) along x: tx[k][tj][ry] = sum over the 2 f columns of low-resolution column ja + tj, left to right
  for (int item = threadIdx.x; item < k1 * ntw * rh; item += 256) {
    const int ry = item % rh, rest = item / rh, tj = rest % ntw, k = rest / ntw;
    const float* row = dus + ((size_t)k * RH + ry) * pitch + tj * factor;
    float acc = 0.f;
    for (int i = 0; i < 2 * factor; ++i) {
      const int X = X0 + tj * factor + i;
      if (X >= 0 && X < W) acc += ds_weight(ds_tap(X, scale, w), ja + tj) * row[i];
    }
    tx_s[((size_t)k * tw + tj) * RH + ry] = acc;
  }
  __syncthreads();

  // (3) along y, top to bottom, and out through dz's strides
  for (int item = threadIdx.x; item < k1 * nth * ntw; item += 256) {
    const int tj = item % ntw, rest = item / ntw, ti = rest % nth, k = rest / nth;
    const float* col = tx_s + ((size_t)k * tw + tj) * RH + ti * factor;
    float acc = 0.f;
    for (int i = 0; i < 2 * factor; ++i) {
      const int Y = Y0 + ti * factor + i;
      if (Y >= 0 && Y < H) acc += ds_weight(ds_tap(Y, scale, h), ia + ti) * col[i];
    }
    dz[b * go.sn + ((int64_t)(ia + ti) * w + (ja + tj)) * go.sp + k * go.sk] = acc;
  }
}

// ---------------------------------------------------------------- host
static int urpc_log2_factor(int f) { return f == 1 ? 0 : f == 2 ? 1 : f == 4 ? 2 : f == 8 ? 3 : f == 16 ? 4 : -1; }

// every argument check the two directions share; fills `a` in the caller's order
static int urpc_scales(const char* who, const float* const* z, const int* factors, const int64_t* strides, int ns, int nb, int H, int W,
                       int k1, UrpcScales* a) {
  MIA_CHECK_ARG(z && factors && strides, "%s: null pointer", who);
  MIA_CHECK_ARG(ns >= 2 && ns <= URPC_MAXS, "%s: %d scales, not in [2,%d]", who, ns, URPC_MAXS);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "%s: k1=%d not in [1,%d]", who, k1, LOSS_MAXK);
  MIA_CHECK_ARG(nb > 0 && H > 0 && W > 0 && (int64_t)nb * H * W < ((int64_t)1 << 31), "%s: bad shape nb=%d H=%d W=%d", who, nb, H, W);
  MIA_CHECK_ARG(factors[0] == 1, "%s: the first scale is the full-resolution output, its factor is %d", who, factors[0]);
  for (int s = 0; s < ns; ++s) {
    const int sh = urpc_log2_factor(factors[s]);
    MIA_CHECK_ARG(sh >= 0 && (s == 0 || sh > 0), "%s: factor %d of scale %d (1 for the first, then 2, 4, 8 or 16)", who, factors[s], s);
    MIA_CHECK_ARG(H % factors[s] == 0 && W % factors[s] == 0, "%s: factor %d of scale %d does not divide H=%d W=%d", who, factors[s], s, H,
                  W);
    MIA_CHECK_ARG(z[s], "%s: null pointer (scale %d)", who, s);
    MIA_CHECK_ARG(strides[3 * s] >= 0 && strides[3 * s + 1] >= 0 && strides[3 * s + 2] >= 0, "%s: negative strides (scale %d)", who, s);
    MIA_CHECK_ARG(strides[3 * s + 1] <= 0x7fffffff && strides[3 * s + 2] <= 0x7fffffff, "%s: class / pixel stride of scale %d beyond 2^31",
                  who, s);
    a->z[s] = z[s];
    a->sn[s] = strides[3 * s];
    a->sk[s] = (int)strides[3 * s + 1];
    a->sp[s] = (int)strides[3 * s + 2];
    a->sh[s] = sh;
    a->id[s] = s;
  }
  for (int s = ns; s < URPC_MAXS; ++s) { a->z[s] = nullptr; a->sn[s] = 0; a->sk[s] = 0; a->sp[s] = 0; a->sh[s] = 0; a->id[s] = 0; }
  return MIA_OK;
}

// KERNEL<NK, NS> for the run-time (k1, ns): compile-time k1 for 2, 3, 4, the run-time bound under NK = 8 otherwise
#define URPC_NS(KERNEL, NK, ...)                                              \
  switch (ns) {                                                               \
    case 2: hipLaunchKernelGGL((KERNEL<NK, 2>), __VA_ARGS__); break;          \
    case 3: hipLaunchKernelGGL((KERNEL<NK, 3>), __VA_ARGS__); break;          \
    case 4: hipLaunchKernelGGL((KERNEL<NK, 4>), __VA_ARGS__); break;          \
    default: hipLaunchKernelGGL((KERNEL<NK, 5>), __VA_ARGS__); break;         \
  }
#define URPC_LAUNCH(KERNEL, ...)                                              \
  do {                                                                        \
    if (k1 == 2) { URPC_NS(KERNEL, 2, __VA_ARGS__) }                          \
    else if (k1 == 3) { URPC_NS(KERNEL, 3, __VA_ARGS__) }                     \
    else if (k1 == 4) { URPC_NS(KERNEL, 4, __VA_ARGS__) }                     \
    else { URPC_NS(KERNEL, LOSS_MAXK, __VA_ARGS__) }                          \
  } while (0)

// ================================================================ C ABI
extern "C" int mia_urpc_workspace(int nb, int ns, int slabs) {
  if (nb <= 0 || ns < 2 || ns > URPC_MAXS || slabs <= 0 || (int64_t)nb * slabs * ns * 6 > 0x7fffffff) return -1;
  return nb * slabs * ns * 6;
}

extern "C" int mia_urpc_fwd(const float* const* z, const int* factors, const int64_t* strides, int ns, int nb, int H, int W, int k1,
                            const float* dyn_dev, int slabs, float* workspace, float* sums, float* terms, float* out, void* stream) {
  UrpcScales a;
  if (int rc = urpc_scales("mia_urpc_fwd", z, factors, strides, ns, nb, H, W, k1, &a)) return rc;
  MIA_CHECK_ARG(workspace && sums && terms && out, "mia_urpc_fwd: null pointer");
  MIA_CHECK_ARG(slabs > 0 && mia_urpc_workspace(nb, ns, slabs) > 0, "mia_urpc_fwd: bad slab count %d", slabs);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  URPC_LAUNCH(urpc_fwd_kernel, grid, blk, 0, st, a, H, W, k1, slabs, workspace);
  hipLaunchKernelGGL(urpc_finalize_kernel, dim3(1), blk, 0, st, workspace, nb * slabs, ns, k1, (double)nb * (double)H * (double)W, dyn_dev,
                     sums, terms, out);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_urpc_bwd(const float* const* z, const int* factors, const int64_t* strides, float* const* dz, const int64_t* gstrides,
                            int ns, int nb, int H, int W, int k1, const float* sums, const float* dyn_dev, const float* grad_out,
                            void* stream) {
  UrpcScales a;
  if (int rc = urpc_scales("mia_urpc_bwd", z, factors, strides, ns, nb, H, W, k1, &a)) return rc;
  MIA_CHECK_ARG(dz && gstrides && sums, "mia_urpc_bwd: null pointer");
  for (int s = 0; s < ns; ++s) {
    MIA_CHECK_ARG(dz[s], "mia_urpc_bwd: null pointer (gradient of scale %d)", s);
    MIA_CHECK_ARG(gstrides[3 * s] >= 0 && gstrides[3 * s + 1] >= 0 && gstrides[3 * s + 2] >= 0,
                  "mia_urpc_bwd: negative strides (gradient of scale %d)", s);
  }
  int th[URPC_MAXS], tw[URPC_MAXS];
  for (int s = 1; s < ns; ++s) {  // every check before the first launch
    ds_bwd_tile(factors[s], k1, &th[s], &tw[s]);
    MIA_CHECK_ARG((int64_t)nb * ceil_div(H / factors[s], th[s]) * ceil_div(W / factors[s], tw[s]) < ((int64_t)1 << 31),
                  "mia_urpc_bwd: too many tiles");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 blk(256);
  {
    const LossGeom go{gstrides[0], gstrides[1], gstrides[2]};
    const dim3 grid((unsigned)ceil_div64((int64_t)nb * H * W, 256));
    URPC_LAUNCH(urpc_bwd_full_kernel, grid, blk, 0, st, a, sums, dyn_dev, grad_out, dz[0], go, nb, H, W, k1);
  }
  for (int s = 1; s < ns; ++s) {
    UrpcScales t = a;  // scale s into slot 0
    t.z[0] = a.z[s]; t.sn[0] = a.sn[s]; t.sk[0] = a.sk[s]; t.sp[0] = a.sp[s]; t.sh[0] = a.sh[s]; t.id[0] = a.id[s];
    t.z[s] = a.z[0]; t.sn[s] = a.sn[0]; t.sk[s] = a.sk[0]; t.sp[s] = a.sp[0]; t.sh[s] = a.sh[0]; t.id[s] = a.id[0];
    const LossGeom go{gstrides[3 * s], gstrides[3 * s + 1], gstrides[3 * s + 2]};
    const int tiles_y = ceil_div(H / factors[s], th[s]), tiles_x = ceil_div(W / factors[s], tw[s]);
    const dim3 grid((unsigned)(nb * tiles_y * tiles_x));
    const size_t lds = ds_bwd_lds(factors[s], k1, th[s], tw[s]);
    URPC_LAUNCH(urpc_bwd_gather_kernel, grid, blk, lds, st, t, sums, dyn_dev, grad_out, dz[s], go, nb, H, W, k1, th[s], tw[s], tiles_x,
                tiles_y);
  }
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
