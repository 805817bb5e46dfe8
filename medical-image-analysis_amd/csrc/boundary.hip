// Boundary loss of Kervadec et al. (MIDL 2019; `one_hot2dist` + `SurfaceLoss` of their public code) on the GPU (gfx950):
//   phi[b,k] = edt(~G) (~G) - (edt(G) - 1) G,  G = (labels[b] == k), for the selected classes k (a bit mask over 0 .. k1-1)
//   L = (1/N) sum_{b, k selected, p} softmax(z)[b,k,p] phi[b,k,p],  N = B * (number of selected classes) * H * W
//   dL/dz_j = g s_j (w_j - sum_k w_k s_k),  w_k = phi_k / N for a selected k, else 0
// edt is the exact Euclidean distance transform with per-axis spacing (sh, sw).  The `- 1` is literal whatever the spacing (the
// published definition).  Edge rule: pixels outside the array do not exist, an object that touches the image edge has no boundary
// there (scipy's rule; surface.hip's border test counts the outside as background).  No-boundary rule: a class that is absent from
// an image, or fills it, has phi = 0 there.  A label outside 0 .. k1-1 is a member of no class.
//
// Signed distance map, the separable transform of surface.hip (edt_common.h) with every pixel a query:
//   sdm_col_kernel   a thread per (image, class, column, segment of 64 rows), the rows' membership as bit words: ONE signed value per
//                    pixel that holds both 1-D squared fields: -(squared distance to the nearest non-member of the column) on a
//                    member, +(squared distance to the nearest member of the column) on a non-member, -inf / +inf where the
//                    column has none.  The field a pixel does not store is 0 there (spacing^2 is a normal fp32, so no stored
//                    value is 0 and the sign tells members from non-members).
//   sdm_row_kernel   a block per (image, class, slab of rows): the rows are unpacked into the two fields in LDS; a member scans the
//                    non-member field, a non-member the member field (line_min_x4: outward with early exit, exact); then the square
//                    root, sign and - 1, one 4-byte store per pixel.  A row whose field has no finite value belongs to an image
//                    whose field has none (a column's finiteness does not depend on the row): the class is absent or fills the
//                    image, phi = 0 -- the no-boundary rule without a flag, a second pass or a host sync.
// Loss: bl_fwd_kernel streams logits (any (sn, sk, sp) strides: planar and channels-last), labels (range check only) and phi,
// soft-max and products in double per pixel (the exponentials are fp32 with the rounding error of `z - max` carried along),
// per-block partials as (hi, lo) float pairs through LossBlockSums; bl_finalize_kernel adds them in a fixed order in double,
// applies the device-side weight and gives the bad-label verdict (loss_common.h).  bl_bwd_kernel is one streaming pass that
// writes dlogits.  No float atomics: bit-identical from run to run; nothing synchronises with the host.
#include "edt_common.h"
#include "loss_common.h"

#define SDM_MAX_HW 4096

__device__ __forceinline__ bool bl_is_class(long long v, int c) { return v == (long long)c; }
__device__ __forceinline__ bool bl_is_class(unsigned char v, int c) { return (int)v == c; }
__device__ __forceinline__ bool bl_in_range(long long v, int k1) { return (unsigned long long)v < (unsigned long long)k1; }
__device__ __forceinline__ bool bl_in_range(unsigned char v, int k1) { return (int)v < k1; }

static inline int bl_popcount(int m) { return __builtin_popcount((unsigned)m); }
static inline bool bl_mask_ok(int k1, int mask) { return mask > 0 && (mask >> k1) == 0; }

// block (column tile, image * nc + ci): 256 threads = segs segments of 64 rows x cw columns (segs = 1 << segs_log2 >= ceil(h / 64),
// cw = 256 / segs; thread = seg * cw + column).  A thread packs the membership of its 64 rows into two 64-bit words (members,
// non-members; rows past h in neither) and shares them through LDS; the nearest row of the other set above and below any row is
// then a count of leading / trailing zeros in its own words, or the carry found once per thread in the words of the segments
// above and below.  One read of the labels, one 4-byte store per pixel, no sweep that waits on its own stores.  f [nb][nc][h][w]
template <typename LT>
__global__ void __launch_bounds__(256) sdm_col_kernel(const LT* __restrict__ labels, int h, int w, int nc, int mask, int segs_log2,
                                                      float sh, float* __restrict__ f) {
  __shared__ unsigned long long mem[256], non[256];
  const int segs = 1 << segs_log2, cw = 256 >> segs_log2;
  const int cx = threadIdx.x & (cw - 1), sg = threadIdx.x >> (8 - segs_log2);
  const int x = blockIdx.x * cw + cx, y0 = sg * 64;
  const int b = blockIdx.y / nc, ci = blockIdx.y % nc;
  int c = 0;
  for (int k = 0, n = 0; k < LOSS_MAXK; ++k)
    if ((mask >> k) & 1) { if (n == ci) c = k; ++n; }
  const LT* lab = labels + (int64_t)b * h * w + x;
  unsigned long long m = 0ull, n = 0ull;
  if (x < w)
    for (int i = 0; i < 64 && y0 + i < h; ++i) {
      const bool is = bl_is_class(lab[(int64_t)(y0 + i) * w], c);
      m |= (unsigned long long)is << i;
      n |= (unsigned long long)!is << i;
    }
  mem[threadIdx.x] = m;
  non[threadIdx.x] = n;
  __syncthreads();
  if (x >= w) return;
  int upM = -1, upN = -1, dnM = -1, dnN = -1;  // the nearest member / non-member row above and below this segment
  for (int s = sg - 1; s >= 0 && (upM < 0 || upN < 0); --s) {
    const unsigned long long mm = mem[s * cw + cx], nn = non[s * cw + cx];
    if (upM < 0 && mm) upM = s * 64 + 63 - __builtin_clzll(mm);
    if (upN < 0 && nn) upN = s * 64 + 63 - __builtin_clzll(nn);
  }
  for (int s = sg + 1; s < segs && (dnM < 0 || dnN < 0); ++s) {
    const unsigned long long mm = mem[s * cw + cx], nn = non[s * cw + cx];
    if (dnM < 0 && mm) dnM = s * 64 + __builtin_ctzll(mm);
    if (dnN < 0 && nn) dnN = s * 64 + __builtin_ctzll(nn);
  }
  float* col = f + (int64_t)blockIdx.y * h * w + x;
  const float inf = __builtin_inff();
  for (int i = 0; i < 64 && y0 + i < h; ++i) {
    const int y = y0 + i;
    const bool is = (m >> i) & 1ull;
    const unsigned long long other = is ? n : m;  // a member looks for the nearest non-member and the other way round
    const int up = is ? upN : upM, dn = is ? dnN : dnM;
    const unsigned long long lo = other & ((1ull << i) - 1ull), hi = i < 63 ? other >> (i + 1) : 0ull;
    const int da = lo ? i - (63 - __builtin_clzll(lo)) : (up >= 0 ? y - up : -1);
    const int db = hi ? 1 + __builtin_ctzll(hi) : (dn >= 0 ? dn - y : -1);
    const int d = da < 0 ? db : (db < 0 ? da : (da < db ? da : db));
    const float v = d < 0 ? inf : sq_dist(sh, d);
    col[(int64_t)y * w] = is ? -v : v;
  }
}

// block (image * nc + ci, slab of `rows` rows), rows * w <= 2048 floats per field (one row when w is larger): the slab is staged once
__global__ void __launch_bounds__(256) sdm_row_kernel(const float* __restrict__ f, int h, int w, int rows, int slabs, float sw,
                                                      float* __restrict__ phi) {
  extern __shared__ float sdm_lds[];  // distance^2 along H to the nearest member [rows][w] | to the nearest non-member [rows][w]
  const int img = blockIdx.x / slabs, r0 = (blockIdx.x % slabs) * rows;
  const int nr = r0 + rows < h ? rows : h - r0, tot = nr * w;
  float* gin = sdm_lds;
  float* gout = sdm_lds + rows * w;
  const int64_t base = ((int64_t)img * h + r0) * w;  // the slab's rows are contiguous
  const float inf = __builtin_inff();
  int finI = 0, finO = 0;
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const float v = f[base + i];
    gin[i] = v > 0.f ? v : 0.f;
    gout[i] = v < 0.f ? -v : 0.f;
    finI |= v < inf;
    finO |= v > -inf;
  }
  finI = __syncthreads_or(finI);  // a column is finite in every row or in none, so one row of the image decides for all of them
  finO = __syncthreads_or(finO);
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const int r = i / w, x = i - r * w;
    float o;
    if (gout[i] > 0.f) {  // a member: minus (distance to the nearest non-member, minus one)
      const float d2 = finO ? line_min_x4(gout + r * w, w, x, sw) : inf;
      o = d2 < inf ? (float)(1.0 - sqrt((double)d2)) : 0.f;
    } else {
      const float d2 = finI ? line_min_x4(gin + r * w, w, x, sw) : inf;
      o = d2 < inf ? sqrtf(d2) : 0.f;
    }
    phi[base + i] = o;
  }
}

// Soft-max of one pixel in double: e_k = exp(z_k - max) in fp32, times (1 + the rounding error of the subtraction), so the only
// fp32 error left in s_k is expf's own.  phi of an unselected class is 0.
__device__ __forceinline__ void bl_softmax(const float (&v)[LOSS_MAXK], int k1, double (&s)[LOSS_MAXK]) {
  float mx = v[0];
#pragma unroll
  for (int k = 1; k < LOSS_MAXK; ++k)
    if (k < k1) mx = fmaxf(mx, v[k]);
  double se = 0.0;
#pragma unroll
  for (int k = 0; k < LOSS_MAXK; ++k) {
    s[k] = 0.0;
    if (k < k1) {
      const float d = v[k] - mx;
      const float t = d - v[k];
      const float err = (v[k] - (d - t)) + (-mx - t);  // v - mx = d + err exactly
      const float e = expf(d);
      s[k] = (double)e + (double)e * (double)err;
      se += s[k];
    }
  }
  const double inv = 1.0 / se;
#pragma unroll
  for (int k = 0; k < LOSS_MAXK; ++k) s[k] *= inv;
}

__device__ __forceinline__ void bl_load(const float* __restrict__ src, const float* __restrict__ ph, int64_t hw, int k1, int mask,
                                        const LossGeom& g, float (&v)[LOSS_MAXK], float (&d)[LOSS_MAXK]) {
  int ci = 0;
#pragma unroll
  for (int k = 0; k < LOSS_MAXK; ++k) {
    v[k] = (k < k1) ? src[k * g.sk] : 0.f;
    d[k] = 0.f;
    if (k < k1 && ((mask >> k) & 1)) { d[k] = ph[(int64_t)ci * hw]; ++ci; }
  }
}

// block (image, slab of pixels); ws [nb * slabs][2] = (hi, lo) of the block's sum of s phi
template <typename LT>
__global__ __launch_bounds__(256) void bl_fwd_kernel(const float* __restrict__ logits, const LT* __restrict__ labels,
                                                     const float* __restrict__ phi, int64_t hw, int k1, int mask, int nc, LossGeom g,
                                                     int slabs, float* __restrict__ ws, int* __restrict__ bad_label) {
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int64_t per = (hw + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* base = logits + b * g.sn;
  const float* ph = phi + (int64_t)b * nc * hw;
  double acc = 0.0;
  bool bad = false;
  for (int64_t p = r0 + threadIdx.x; p < r1; p += 256) {
    float v[LOSS_MAXK], d[LOSS_MAXK];
    double sm[LOSS_MAXK];
    bl_load(base + p * g.sp, ph + p, hw, k1, mask, g, v, d);
    bad |= !bl_in_range(labels[(int64_t)b * hw + p], k1);
    bl_softmax(v, k1, sm);
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) acc += sm[k] * (double)d[k];
  }
  if (bad) *bad_label = 1;
  float part[2];
  loss_split(acc, part);
  auto red = loss_block_sums<2, 0>();
  red.put(0, part);
  __syncthreads();
  if (threadIdx.x < 2) ws[(size_t)blockIdx.x * 2 + threadIdx.x] = red.sum_f(threadIdx.x);
}

// one block: out[0] = weight * L, out[1] = L, out[2] = weight; coef[0] = 1 (NaN after a bad label: every gradient follows)
__global__ void bl_finalize_kernel(const float* __restrict__ ws, int nparts, double n_terms, const float* __restrict__ weight_dev,
                                   float* __restrict__ coef, float* __restrict__ out, int* __restrict__ bad_label) {
  const LossTotals tot = loss_totals<1, 0>(ws, nullptr, nparts, 1);
  __shared__ float res[3];
  if (threadIdx.x == 0) {
    const float wt = weight_dev ? weight_dev[0] : 1.f;
    const double l = tot.f[0] / n_terms;
    res[0] = (float)((double)wt * l);
    res[1] = (float)l;
    res[2] = wt;
    coef[0] = 1.f;
  }
  __syncthreads();
  if (threadIdx.x < 3) out[threadIdx.x] = res[threadIdx.x];  // one 4-byte store per lane
  loss_bad_label_verdict(bad_label, out, coef, 1);
}

__global__ __launch_bounds__(256) void bl_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ phi,
                                                     const float* __restrict__ coef, const float* __restrict__ weight_dev,
                                                     const float* __restrict__ gout, float* __restrict__ dl, int nb, int64_t hw, int k1,
                                                     int mask, int nc, double inv_n, LossGeom g, LossGeom go) {
  const int64_t total = (int64_t)nb * hw;
  const double sc = (double)(gout ? gout[0] : 1.f) * (double)coef[0] * (double)(weight_dev ? weight_dev[0] : 1.f) * inv_n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / hw);
    const int64_t p = i - (int64_t)b * hw;
    float v[LOSS_MAXK], d[LOSS_MAXK];
    double sm[LOSS_MAXK];
    bl_load(logits + b * g.sn + p * g.sp, phi + (int64_t)b * nc * hw + p, hw, k1, mask, g, v, d);
    bl_softmax(v, k1, sm);
    double dot = 0.0;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) dot += sm[k] * (double)d[k];
    float* dst = dl + b * go.sn + p * go.sp;
#pragma unroll
    for (int k = 0; k < LOSS_MAXK; ++k)
      if (k < k1) dst[k * go.sk] = (float)(sc * sm[k] * ((double)d[k] - dot));
  }
}

// the checks shared by mia_sdm_workspace and mia_signed_distance_map; returns the number of selected classes, 0 outside the limits
static int sdm_classes(int nb, int h, int w, int k1, int mask) {
  if (nb < 1 || h < 1 || w < 1 || h > SDM_MAX_HW || w > SDM_MAX_HW || k1 < 1 || k1 > LOSS_MAXK || !bl_mask_ok(k1, mask)) return 0;
  const int nc = bl_popcount(mask);
  if ((int64_t)nb * nc > 65535 || (int64_t)nb * nc * h * w > 0x7fffffff) return 0;
  return nc;
}

extern "C" int mia_sdm_workspace(int nb, int h, int w, int k1, int class_mask) {
  const int nc = sdm_classes(nb, h, w, k1, class_mask);
  return nc ? (int)((int64_t)nb * nc * h * w) : -1;
}

extern "C" int mia_signed_distance_map(const void* labels, int label_u8, int nb, int h, int w, int k1, int class_mask, float sh, float sw,
                                       float* workspace, float* phi, void* stream) {
  MIA_CHECK_ARG(labels && workspace && phi, "mia_signed_distance_map: null pointer");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_signed_distance_map: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(bl_mask_ok(k1, class_mask), "mia_signed_distance_map: class_mask=0x%x selects no class or one outside [0,%d)",
                (unsigned)class_mask, k1);
  MIA_CHECK_ARG(sh > 0.f && sw > 0.f && sh < __builtin_inff() && sw < __builtin_inff(),
                "mia_signed_distance_map: spacing (%g, %g) must be finite and > 0", (double)sh, (double)sw);
  // a stored 1-D squared distance must never be 0: the sign of the packed field tells members from non-members
  MIA_CHECK_ARG(sh * sh >= 1.17549435e-38f && sw * sw >= 1.17549435e-38f,
                "mia_signed_distance_map: spacing (%g, %g) too small: its square is not a normal fp32", (double)sh, (double)sw);
  const int nc = sdm_classes(nb, h, w, k1, class_mask);
  MIA_CHECK_ARG(nc > 0,
                "mia_signed_distance_map: extents nb=%d h=%d w=%d outside the limits (1 <= h, w <= %d, nb * classes <= 65535, "
                "nb * classes * h * w < 2^31)", nb, h, w, SDM_MAX_HW);
  MIA_CHECK_ARG((double)sh * sh * h * h + (double)sw * sw * w * w < 1e30,
                "mia_signed_distance_map: spacing x extent too large for fp32 squared distances");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int segs_log2 = 0;
  while ((64 << segs_log2) < h) ++segs_log2;  // <= 6: h <= 4096
  const dim3 cgrid((unsigned)ceil_div(w, 256 >> segs_log2), (unsigned)(nb * nc));
  if (label_u8)
    hipLaunchKernelGGL(sdm_col_kernel<unsigned char>, cgrid, dim3(256), 0, st, static_cast<const unsigned char*>(labels), h, w, nc, class_mask,
                       segs_log2, sh, workspace);
  else
    hipLaunchKernelGGL(sdm_col_kernel<long long>, cgrid, dim3(256), 0, st, static_cast<const long long*>(labels), h, w, nc, class_mask,
                       segs_log2, sh, workspace);
  int rows = 2048 / w;  // rows per block: at most 2048 floats per LDS field, 1 .. 8 rows
  rows = rows < 1 ? 1 : (rows > 8 ? 8 : rows);
  const int slabs = ceil_div(h, rows);
  hipLaunchKernelGGL(sdm_row_kernel, dim3((unsigned)((int64_t)nb * nc * slabs)), dim3(256), (size_t)2 * rows * w * 4, st, workspace, h, w, rows,
                     slabs, sw, phi);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_boundary_loss_workspace(int nb, int slabs) {
  if (nb <= 0 || slabs <= 0 || (int64_t)nb * slabs * 2 > 0x7fffffff) return -1;
  return nb * slabs * 2;
}

extern "C" int mia_boundary_loss_fwd(const float* logits, const void* labels, int label_u8, const float* phi, const float* weight_dev, int nb,
                                     int64_t hw, int k1, int class_mask, int64_t sn, int64_t sk, int64_t sp, int slabs, float* workspace,
                                     float* coef, float* out, int* bad_label, void* stream) {
  MIA_CHECK_ARG(logits && labels && phi && workspace && coef && out && bad_label, "mia_boundary_loss_fwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0 && slabs > 0 && (int64_t)nb * slabs * 2 <= 0x7fffffff, "mia_boundary_loss_fwd: bad shape");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_boundary_loss_fwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(bl_mask_ok(k1, class_mask), "mia_boundary_loss_fwd: class_mask=0x%x selects no class or one outside [0,%d)",
                (unsigned)class_mask, k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp};
  const int nc = bl_popcount(class_mask);
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  if (label_u8)
    hipLaunchKernelGGL(bl_fwd_kernel<unsigned char>, grid, blk, 0, st, logits, static_cast<const unsigned char*>(labels), phi, hw, k1,
                       class_mask, nc, g, slabs, workspace, bad_label);
  else
    hipLaunchKernelGGL(bl_fwd_kernel<long long>, grid, blk, 0, st, logits, static_cast<const long long*>(labels), phi, hw, k1, class_mask,
                       nc, g, slabs, workspace, bad_label);
  hipLaunchKernelGGL(bl_finalize_kernel, dim3(1), blk, 0, st, workspace, nb * slabs, (double)nb * nc * (double)hw, weight_dev, coef, out,
                     bad_label);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_boundary_loss_bwd(const float* logits, const float* phi, const float* coef, const float* weight_dev, const float* grad_out,
                                     float* dlogits, int nb, int64_t hw, int k1, int class_mask, int64_t sn, int64_t sk, int64_t sp,
                                     int64_t gsn, int64_t gsk, int64_t gsp, void* stream) {
  MIA_CHECK_ARG(logits && phi && coef && dlogits, "mia_boundary_loss_bwd: null pointer");
  MIA_CHECK_ARG(nb > 0 && hw > 0, "mia_boundary_loss_bwd: bad shape");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= LOSS_MAXK, "mia_boundary_loss_bwd: k1=%d not in [1,%d]", k1, LOSS_MAXK);
  MIA_CHECK_ARG(bl_mask_ok(k1, class_mask), "mia_boundary_loss_bwd: class_mask=0x%x selects no class or one outside [0,%d)",
                (unsigned)class_mask, k1);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const LossGeom g{sn, sk, sp}, go{gsn, gsk, gsp};
  const int nc = bl_popcount(class_mask);
  const int64_t blocks = ceil_div64((int64_t)nb * hw, 256);
  hipLaunchKernelGGL(bl_bwd_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, logits, phi, coef, weight_dev, grad_out,
                     dlogits, nb, hw, k1, class_mask, nc, 1.0 / ((double)nb * nc * (double)hw), g, go);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
