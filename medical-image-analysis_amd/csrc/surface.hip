// Surface distances of `calculate_metric_percase` (src/training/al_trainer.py:1539-1556) on the GPU (gfx950):
//   HD  = max(max_{a in A} d(a, B), max_{b in B} d(b, A))        (metric.cal_hd -> ITK HausdorffDistanceImageFilter)
//   ASD = mean_{a in dA} d(a, dB)                                 (medpy.metric.binary.asd, connectivity 1)
// with dX = X & !erode(X) (face-connected cross: 4 neighbours for ndim 2, 6 for ndim 3; outside the array is background) and
// d the Euclidean distance with per-axis spacing (sd, sh, sw).  Mask 0 is (pred > 0, labels > 0), mask c is (pred == c, labels == c).
//
// Three exact squared-EDT fields per mask -- F_B (queried on A), F_A (queried on B), F_dB (queried on dA) -- as the separable
// transform of the 1-D passes along D, H and W, each pass the exact lower envelope min_j ((s (i - j))^2 + f(j)) of its line:
//   surf_pass1_kernel   one thread per (n, h, w) column: membership + border test (face neighbours), 1-D distance along D by a
//                       forward and a backward sweep; writes the three fields and one query byte (A | B << 1 | dA << 2)
//   surf_pass2_kernel   a block per (n, z, CW-column tile, field): the tile's columns staged in LDS, scan along H, in place
//   surf_pass3_kernel   a block per (n, slab of rows): each row staged in LDS, scan along W only at query voxels, fused with the
//                       reductions: per-block partials (max F_B over A, max F_A over B, sum sqrt(F_dB) over dA, |dA|)
//   surf_finalize_kernel  fixed-order double reduction of the partials, empty-set rules, square roots of the maxima
// The per-line minimisation is a scan outward from i with early exit once (s r)^2 >= best (every further term is >= (s r)^2);
// lines without a finite value are skipped.  Masks run one at a time through the same workspace, so it holds 3 floats + 1 byte
// per voxel plus the partials, whatever k1 is.  No float atomics: results are bit-identical from run to run.
#include "common.h"

#define SURF_MAXK 8
#define SURF_MAX_D 1024
#define SURF_MAX_HW 4096
#define SURF_P2_LDS (60 * 1024)  // bytes of LDS for one pass-2 column tile: h * CW floats (h <= 4096 -> CW >= 2)
#define SURF_MAX_PART (1 << 20)  // floats of partials
#define SURF_NPART 5             // partial arrays: max F_B | max F_A | sum hi | sum lo | |dA| (int bits)

namespace {

__device__ __forceinline__ bool in_mask(long long v, int m) { return m == 0 ? v > 0 : v == (long long)m; }

__device__ __forceinline__ float sq_dist(float s, int r) {
  const float t = s * (float)r;
  return t * t;
}

// min_j ((s (i - j))^2 + f[j * stride]) over 0 <= j < n, scanning outward from i; f has at least one finite value
__device__ __forceinline__ float line_min(const float* f, int stride, int n, int i, float s) {
  float best = f[i * stride];
  for (int r = 1;; ++r) {
    const float dr = sq_dist(s, r);
    if (dr >= best) break;
    const int lo = i - r, hi = i + r;
    if (lo < 0 && hi >= n) break;
    if (lo >= 0) best = fminf(best, dr + f[lo * stride]);
    if (hi < n) best = fminf(best, dr + f[hi * stride]);
  }
  return best;
}

struct SurfGeom {
  int nvol, d, h, w, ndim;
};

// Pass 1: one thread per (n, y, x); walks z.  A voxel is a border voxel when it is in the set and one of its face neighbours is not
// (out of the array counts as not).  Fields: squared distance along D to the nearest feature voxel of the column (0 on a feature
// voxel, +inf when the column has none).
__global__ void surf_pass1_kernel(const long long* __restrict__ pred, const long long* __restrict__ labels, SurfGeom g, int m, float sd,
                                  float* __restrict__ fb, float* __restrict__ fa, float* __restrict__ fdb, unsigned char* __restrict__ q) {
  const int64_t hw = (int64_t)g.h * g.w;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.nvol * hw) return;
  const int64_t n = i / hw, p = i % hw;
  const int y = (int)(p / g.w), x = (int)(p % g.w);
  const int64_t col = n * g.d * hw + p;  // voxel (n, 0, y, x)
  const float inf = __builtin_inff();
  bool aC = in_mask(pred[col], m), bC = in_mask(labels[col], m);
  bool aP = false, bP = false;  // plane z - 1 (outside: background)
  int lastB = -1, lastA = -1, lastD = -1;
  for (int z = 0; z < g.d; ++z) {
    const int64_t v = col + z * hw;
    bool aN = false, bN = false;
    if (z + 1 < g.d) { aN = in_mask(pred[v + hw], m); bN = in_mask(labels[v + hw], m); }
    bool dA = false, dB = false;
    if (aC || bC) {
      bool allA = x > 0 && x + 1 < g.w && y > 0 && y + 1 < g.h, allB = allA;
      if (allA) {
        const int64_t nb[4] = {v - 1, v + 1, v - g.w, v + g.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          allA = allA && in_mask(pred[nb[k]], m);
          allB = allB && in_mask(labels[nb[k]], m);
        }
      }
      if (g.ndim == 3) { allA = allA && aP && aN; allB = allB && bP && bN; }
      dA = aC && !allA;
      dB = bC && !allB;
    }
    if (bC) lastB = z;
    if (aC) lastA = z;
    if (dB) lastD = z;
    fb[v] = lastB >= 0 ? sq_dist(sd, z - lastB) : inf;
    fa[v] = lastA >= 0 ? sq_dist(sd, z - lastA) : inf;
    fdb[v] = lastD >= 0 ? sq_dist(sd, z - lastD) : inf;
    q[v] = (unsigned char)((aC ? 1 : 0) | (bC ? 2 : 0) | (dA ? 4 : 0));
    aP = aC; bP = bC; aC = aN; bC = bN;
  }
  if (g.d == 1) return;
  int nextB = -1, nextA = -1, nextD = -1;  // backward sweep: a feature voxel holds 0 (spacings are > 0)
  for (int z = g.d - 1; z >= 0; --z) {
    const int64_t v = col + z * hw;
    float vb = fb[v], va = fa[v], vd = fdb[v];
    if (vb == 0.f) nextB = z; else if (nextB >= 0) { vb = fminf(vb, sq_dist(sd, nextB - z)); fb[v] = vb; }
    if (va == 0.f) nextA = z; else if (nextA >= 0) { va = fminf(va, sq_dist(sd, nextA - z)); fa[v] = va; }
    if (vd == 0.f) nextD = z; else if (nextD >= 0) { vd = fminf(vd, sq_dist(sd, nextD - z)); fdb[v] = vd; }
  }
}

// Pass 2: block (plane n * d + z, tile of cw columns), blockIdx.y = field.  The tile's h x cw values are staged whole before any is
// written back, and no other block touches them: the pass runs in place.  Lanes sit on adjacent x (row segments of cw floats).
__global__ void __launch_bounds__(256) surf_pass2_kernel(float* __restrict__ f0, float* __restrict__ f1, float* __restrict__ f2, SurfGeom g,
                                                         int cw, int tiles, float sh) {
  extern __shared__ float lds2[];  // [h][cw]
  __shared__ int finite[64];
  float* f = blockIdx.y == 0 ? f0 : blockIdx.y == 1 ? f1 : f2;
  const int plane = blockIdx.x / tiles, x0 = (blockIdx.x % tiles) * cw;
  float* base = f + (int64_t)plane * g.h * g.w + x0;
  const int tot = g.h * cw;
  if (threadIdx.x < 64) finite[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const int y = i / cw, c = i % cw;
    const float v = x0 + c < g.w ? base[(int64_t)y * g.w + c] : __builtin_inff();
    lds2[i] = v;
    if (v < __builtin_inff()) finite[c] = 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < tot; i += blockDim.x) {
    const int y = i / cw, c = i % cw;
    if (x0 + c >= g.w || !finite[c]) continue;  // a column without a finite value stays +inf
    base[(int64_t)y * g.w + c] = line_min(lds2 + c, cw, g.h, y, sh);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Pass 3: block (n, slab of rows), 256 threads.  A row without a query voxel is skipped after reading its query bytes; otherwise its
// three fields are staged in LDS and each query voxel scans its row.  Partials are written to five separate arrays (4-byte stores).
__global__ void __launch_bounds__(256) surf_pass3_kernel(const float* __restrict__ fb, const float* __restrict__ fa,
                                                         const float* __restrict__ fdb, const unsigned char* __restrict__ q, SurfGeom g,
                                                         int slabs, int k1, int m, float sw, float* __restrict__ part, int npart) {
  extern __shared__ float lds3[];  // fb[w] | fa[w] | fdb[w] | q[w] bytes
  __shared__ float redf[2][4];
  __shared__ double redd[4];
  __shared__ int redi[4];
  float* sb = lds3;
  float* sa = lds3 + g.w;
  float* sdb = lds3 + 2 * g.w;
  unsigned char* sq = reinterpret_cast<unsigned char*>(lds3 + 3 * g.w);
  const int n = blockIdx.x / slabs, s = blockIdx.x % slabs;
  const int rows = g.d * g.h;
  const int per = (rows + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < rows ? r0 + per : rows;
  const float inf = __builtin_inff();
  float maxB = -1.f, maxA = -1.f;  // -1: no query voxel seen
  double sum = 0.0;
  int cnt = 0;
  for (int r = r0; r < r1; ++r) {
    const int64_t row = ((int64_t)n * rows + r) * g.w;
    int anyq = 0;
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) { const unsigned char v = q[row + x]; sq[x] = v; anyq |= v; }
    if (!__syncthreads_or(anyq)) continue;
    int finB = 0, finA = 0, finD = 0;
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const float vb = fb[row + x], va = fa[row + x], vd = fdb[row + x];
      sb[x] = vb; sa[x] = va; sdb[x] = vd;
      finB |= vb < inf; finA |= va < inf; finD |= vd < inf;
    }
    finB = __syncthreads_or(finB);
    finA = __syncthreads_or(finA);
    finD = __syncthreads_or(finD);
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const unsigned char v = sq[x];
      if (v & 1) maxB = fmaxf(maxB, finB ? line_min(sb, 1, g.w, x, sw) : inf);
      if (v & 2) maxA = fmaxf(maxA, finA ? line_min(sa, 1, g.w, x, sw) : inf);
      if (v & 4) { sum += sqrt((double)(finD ? line_min(sdb, 1, g.w, x, sw) : inf)); ++cnt; }
    }
    __syncthreads();  // the next row's staging overwrites the LDS rows
  }
  maxB = wave_max(maxB); maxA = wave_max(maxA); sum = wave_sum_d(sum); cnt = wave_sum_i(cnt);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (ln == 0) { redf[0][wv] = maxB; redf[1][wv] = maxA; redd[wv] = sum; redi[wv] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < nw; ++k) { maxB = fmaxf(maxB, redf[0][k]); maxA = fmaxf(maxA, redf[1][k]); sum += redd[k]; cnt += redi[k]; }
    const int64_t o = ((int64_t)n * k1 + m) * slabs + s;
    const float hi = (float)sum;
    part[o] = maxB;
    part[npart + o] = maxA;
    part[2 * npart + o] = hi;
    part[3 * npart + o] = hi < inf ? (float)(sum - (double)hi) : 0.f;  // inf - inf would be NaN
    part[4 * npart + o] = __int_as_float(cnt);
  }
}

// hd / asd [nvol][k1]: NaN where A is empty; +inf where only B is (F_B and F_dB are +inf everywhere then)
__global__ void surf_finalize_kernel(const float* __restrict__ part, int npart, int nvol, int k1, int slabs, float* __restrict__ hd,
                                     float* __restrict__ asd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvol * k1) return;
  float mb = -1.f, ma = -1.f;
  double sum = 0.0;
  long long cnt = 0;
  for (int s = 0; s < slabs; ++s) {
    const int64_t o = (int64_t)i * slabs + s;
    mb = fmaxf(mb, part[o]);
    ma = fmaxf(ma, part[npart + o]);
    sum += (double)part[2 * npart + o] + (double)part[3 * npart + o];
    cnt += __float_as_int(part[4 * npart + o]);
  }
  const float nan = __builtin_nanf("");
  hd[i] = mb < 0.f ? nan : (float)sqrt((double)fmaxf(mb, ma));
  asd[i] = cnt == 0 ? nan : (float)(sum / (double)cnt);
}

struct SurfPlan {
  int64_t vox;    // nvol * d * h * w
  int slabs;      // pass-3 blocks per volume
  int64_t npart;  // entries per partial array: nvol * k1 * slabs
  int64_t total;  // workspace floats
};

bool surf_plan(int nvol, int d, int h, int w, int k1, SurfPlan& p) {
  if (nvol < 1 || d < 1 || h < 1 || w < 1 || k1 < 1 || k1 > SURF_MAXK || d > SURF_MAX_D || h > SURF_MAX_HW || w > SURF_MAX_HW) return false;
  if ((int64_t)nvol * k1 * SURF_NPART > SURF_MAX_PART) return false;
  p.vox = (int64_t)nvol * d * h * w;
  const int64_t rows = (int64_t)d * h;
  const int64_t cap = SURF_MAX_PART / ((int64_t)nvol * k1 * SURF_NPART);  // >= 1
  int64_t slabs = (rows + 3) / 4;  // >= 4 rows per block
  if (slabs > 2048) slabs = 2048;
  if (slabs > cap) slabs = cap;
  p.slabs = (int)slabs;
  p.npart = (int64_t)nvol * k1 * slabs;
  p.total = 3 * p.vox + (p.vox + 3) / 4 + SURF_NPART * p.npart;  // fields | query bytes | partials
  return p.total <= 0x7fffffff;
}

}  // namespace

extern "C" int mia_surface_distance_workspace(int nvol, int d, int h, int w, int k1) {
  SurfPlan p;
  return surf_plan(nvol, d, h, w, k1, p) ? (int)p.total : -1;
}

extern "C" int mia_surface_distance(const long long* pred, const long long* labels, int nvol, int ndim, int d, int h, int w, int k1, float sd,
                                    float sh, float sw, float* workspace, float* hd, float* asd, void* stream) {
  MIA_CHECK_ARG(pred && labels && workspace && hd && asd, "mia_surface_distance: null pointer");
  MIA_CHECK_ARG(k1 >= 1 && k1 <= SURF_MAXK, "mia_surface_distance: k1=%d not in [1,%d]", k1, SURF_MAXK);
  MIA_CHECK_ARG(ndim == 2 || ndim == 3, "mia_surface_distance: ndim=%d not 2 or 3", ndim);
  MIA_CHECK_ARG(ndim == 3 || d == 1, "mia_surface_distance: ndim 2 needs d == 1 (got d=%d)", d);
  if (ndim == 2) sd = 1.f;  // unused: no D axis
  MIA_CHECK_ARG(sd > 0.f && sh > 0.f && sw > 0.f && sd < __builtin_inff() && sh < __builtin_inff() && sw < __builtin_inff(),
                "mia_surface_distance: spacing (%g, %g, %g) must be finite and > 0", (double)sd, (double)sh, (double)sw);
  // a non-feature voxel must never hold a squared distance of 0 (pass 1 tells feature voxels by their 0)
  MIA_CHECK_ARG(sd * sd >= 1.17549435e-38f && sh * sh >= 1.17549435e-38f && sw * sw >= 1.17549435e-38f,
                "mia_surface_distance: spacing (%g, %g, %g) too small: its square is not a normal fp32", (double)sd, (double)sh, (double)sw);
  SurfPlan p;
  MIA_CHECK_ARG(surf_plan(nvol, d, h, w, k1, p),
                "mia_surface_distance: extents nvol=%d d=%d h=%d w=%d k1=%d outside the limits (d <= %d, h, w <= %d, nvol * k1 <= %d, "
                "workspace < 2^31 floats)", nvol, d, h, w, k1, SURF_MAX_D, SURF_MAX_HW, SURF_MAX_PART / SURF_NPART);
  // squared physical extents must stay far inside fp32 (the scans add (s r)^2 terms of up to the whole diagonal)
  const double diag = (double)sd * sd * d * d + (double)sh * sh * h * h + (double)sw * sw * w * w;
  MIA_CHECK_ARG(diag < 1e30, "mia_surface_distance: spacing x extent too large for fp32 squared distances");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SurfGeom g{nvol, d, h, w, ndim};
  float* fb = workspace;
  float* fa = workspace + p.vox;
  float* fdb = workspace + 2 * p.vox;
  unsigned char* q = reinterpret_cast<unsigned char*>(workspace + 3 * p.vox);
  float* part = workspace + 3 * p.vox + (p.vox + 3) / 4;
  int cw = 64;
  while (cw > 1 && (int64_t)cw * h * 4 > SURF_P2_LDS) cw >>= 1;
  while (cw > 1 && cw / 2 >= w) cw >>= 1;  // no tile wider than the image
  const int tiles = ceil_div(w, cw);
  const int64_t cols = (int64_t)nvol * h * w;
  const size_t lds3 = (size_t)3 * w * 4 + ((w + 3) / 4) * 4;
  for (int m = 0; m < k1; ++m) {
    hipLaunchKernelGGL(surf_pass1_kernel, dim3((unsigned)ceil_div64(cols, 256)), dim3(256), 0, st, pred, labels, g, m, sd, fb, fa, fdb, q);
    hipLaunchKernelGGL(surf_pass2_kernel, dim3((unsigned)(nvol * d * tiles), 3), dim3(256), (size_t)h * cw * 4, st, fb, fa, fdb, g, cw,
                       tiles, sh);
    hipLaunchKernelGGL(surf_pass3_kernel, dim3((unsigned)(nvol * p.slabs)), dim3(256), lds3, st, fb, fa, fdb, q, g, p.slabs, k1, m, sw,
                       part, (int)p.npart);
  }
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(ceil_div(nvol * k1, 64)), dim3(64), 0, st, part, (int)p.npart, nvol, k1, p.slabs, hd, asd);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
