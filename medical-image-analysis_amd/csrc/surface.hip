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
//
// mia_surface_metrics adds the symmetric quantities over S1 = {d(a, dB) : a in dA} and S2 = {d(b, dA) : b in dB}:
//   HD_q = numpy's linear percentile of S1 u S2 (medpy hd95), ASSD = (mean S1 + mean S2) / 2 (medpy assd),
//   NSD(tau) = (|S1 <= tau| + |S2 <= tau|) / (|dA| + |dB|) (voxel-count surface Dice)
// from a fourth field F_dA (queried on dB; query bit 3 = dB):
//   surf_pass1_kernel<true>   also writes F_dA along D and the dB bit
//   surf_pass2_kernel         blockIdx.y = 3 is F_dA
//   surf_pass3_ext_kernel     pass 3 with the rows staged two fields at a time (F_B, F_A, then F_dB, F_dA): the same partials in the
//                             same order, plus sum sqrt(F_dA) over dB, |dB| and the two counts of squared distances <= tau^2; it
//                             writes each dA voxel's squared distance back into the F_dB row and each dB voxel's into the F_dA row,
//                             and all-ones bits (not a non-negative float) everywhere else: two sparse key arrays
//   surf_sel_hist / surf_sel_scan   4 x 8-bit radix select of the rank-k key per volume over both arrays (bits of a non-negative
//                             float order like its value): LDS histogram per block, one integer global atomic per non-empty bin,
//                             a one-block scan per volume that narrows the prefix; pass 0's scan derives k from its own total
//   surf_sel_next_kernel      the smallest key above v[k] by integer atomicMin (skipped where v[k] occurs again after rank k)
//   surf_finalize_ext_kernel  fp64: square roots of the two keys, the interpolation, fixed-order sums of the partials
// Integer adds and mins commute, so these results are bit-identical from run to run and independent of the grid as well.
#include "edt_common.h"  // sq_dist, line_min (shared with boundary.hip)

#define SURF_MAXK 8
#define SURF_MAX_D 1024
#define SURF_MAX_HW 4096
#define SURF_P2_LDS (60 * 1024)  // bytes of LDS for one pass-2 column tile: h * CW floats (h <= 4096 -> CW >= 2)
#define SURF_MAX_PART (1 << 20)  // floats of partials
#define SURF_NPART 5             // partial arrays: max F_B | max F_A | sum hi | sum lo | |dA| (int bits)
#define SURF_NPART_EXT 10        // ... | sum2 hi | sum2 lo | |dB| | |S1 <= tau| | |S2 <= tau| (int bits)
#define SURF_EXT_MAX_NVOL 4096   // mia_surface_metrics: one 256-bin histogram per volume
#define SURF_SEL_STATE 8         // words per (volume, mask): prefix | rank left | keys in the bin | next key | n | unused
#define SURF_NOKEY 0xFFFFFFFFu   // not the bits of a non-negative float

namespace {

__device__ __forceinline__ bool in_mask(long long v, int m) { return m == 0 ? v > 0 : v == (long long)m; }

struct SurfGeom {
  int nvol, d, h, w, ndim;
};

// Pass 1: one thread per (n, y, x); walks z.  A voxel is a border voxel when it is in the set and one of its face neighbours is not
// (out of the array counts as not).  Fields: squared distance along D to the nearest feature voxel of the column (0 on a feature
// voxel, +inf when the column has none).  EXT: also F_dA (fda) and query bit 3 = dB.
template <bool EXT>
__global__ void surf_pass1_kernel(const long long* __restrict__ pred, const long long* __restrict__ labels, SurfGeom g, int m, float sd,
                                  float* __restrict__ fb, float* __restrict__ fa, float* __restrict__ fdb, float* __restrict__ fda,
                                  unsigned char* __restrict__ q) {
  const int64_t hw = (int64_t)g.h * g.w;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.nvol * hw) return;
  const int64_t n = i / hw, p = i % hw;
  const int y = (int)(p / g.w), x = (int)(p % g.w);
  const int64_t col = n * g.d * hw + p;  // voxel (n, 0, y, x)
  const float inf = __builtin_inff();
  bool aC = in_mask(pred[col], m), bC = in_mask(labels[col], m);
  bool aP = false, bP = false;  // plane z - 1 (outside: background)
  int lastB = -1, lastA = -1, lastD = -1, lastE = -1;
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
    if constexpr (EXT) {
      if (dA) lastE = z;
      fda[v] = lastE >= 0 ? sq_dist(sd, z - lastE) : inf;
    }
    q[v] = (unsigned char)((aC ? 1 : 0) | (bC ? 2 : 0) | (dA ? 4 : 0) | (EXT && dB ? 8 : 0));
    aP = aC; bP = bC; aC = aN; bC = bN;
  }
  if (g.d == 1) return;
  int nextB = -1, nextA = -1, nextD = -1, nextE = -1;  // backward sweep: a feature voxel holds 0 (spacings are > 0)
  for (int z = g.d - 1; z >= 0; --z) {
    const int64_t v = col + z * hw;
    float vb = fb[v], va = fa[v], vd = fdb[v];
    if (vb == 0.f) nextB = z; else if (nextB >= 0) { vb = fminf(vb, sq_dist(sd, nextB - z)); fb[v] = vb; }
    if (va == 0.f) nextA = z; else if (nextA >= 0) { va = fminf(va, sq_dist(sd, nextA - z)); fa[v] = va; }
    if (vd == 0.f) nextD = z; else if (nextD >= 0) { vd = fminf(vd, sq_dist(sd, nextD - z)); fdb[v] = vd; }
    if constexpr (EXT) {
      float ve = fda[v];
      if (ve == 0.f) nextE = z; else if (nextE >= 0) { ve = fminf(ve, sq_dist(sd, nextE - z)); fda[v] = ve; }
    }
  }
}

// Pass 2: block (plane n * d + z, tile of cw columns), blockIdx.y = field.  The tile's h x cw values are staged whole before any is
// written back, and no other block touches them: the pass runs in place.  Lanes sit on adjacent x (row segments of cw floats).
__global__ void __launch_bounds__(256) surf_pass2_kernel(float* __restrict__ f0, float* __restrict__ f1, float* __restrict__ f2,
                                                         float* __restrict__ f3, SurfGeom g, int cw, int tiles, float sh) {
  extern __shared__ float lds2[];  // [h][cw]
  __shared__ int finite[64];
  float* f = blockIdx.y == 0 ? f0 : blockIdx.y == 1 ? f1 : blockIdx.y == 2 ? f2 : f3;
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

// ---------------------------------------------------------------------------------------------- mia_surface_metrics

__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)v, o, 64); v = t < v ? t : v; }
  return v;
}

// Pass 3 of mia_surface_metrics: surf_pass3_kernel's block shape, rows, per-thread accumulation order and reduction, so the first
// five partials hold the same bits.  The row's fields go through two LDS rows in two stages (F_B | F_A, then F_dB | F_dA), which
// keeps the block under surf_pass3_kernel's LDS at every w.  Stage 2 writes the keys back: each row of F_dB / F_dA is fully
// staged before its first key is written, and no other block touches it.  The two fields come in as words (kdb, kda), so the
// all-ones word, a NaN as a float, is only ever moved as an integer.  The slab-0 block of a volume also resets the volume's
// histogram and this mask's select state (the select kernels are the only readers, later on the stream).
__global__ void __launch_bounds__(256) surf_pass3_ext_kernel(const float* __restrict__ fb, const float* __restrict__ fa,
                                                             unsigned* __restrict__ kdb, unsigned* __restrict__ kda,
                                                             const unsigned char* __restrict__ q, SurfGeom g,
                                                             int slabs, int k1, int m, float sw, float tau2, float* __restrict__ part,
                                                             int npart, unsigned* __restrict__ hist, unsigned* __restrict__ state) {
  extern __shared__ float lds3[];  // s0[w] | s1[w] | q[w] bytes
  __shared__ float redf[2][4];
  __shared__ double redd[2][4];
  __shared__ int redi[4][4];
  float* s0 = lds3;
  float* s1 = lds3 + g.w;
  unsigned char* sq = reinterpret_cast<unsigned char*>(lds3 + 2 * g.w);
  const int n = blockIdx.x / slabs, s = blockIdx.x % slabs;
  if (s == 0) {
    hist[(int64_t)n * 256 + threadIdx.x] = 0u;
    if (threadIdx.x < SURF_SEL_STATE) state[((int64_t)n * k1 + m) * SURF_SEL_STATE + threadIdx.x] = threadIdx.x == 3 ? SURF_NOKEY : 0u;
  }
  const int rows = g.d * g.h;
  const int per = (rows + slabs - 1) / slabs, r0 = s * per, r1 = r0 + per < rows ? r0 + per : rows;
  const float inf = __builtin_inff();
  float maxB = -1.f, maxA = -1.f;  // -1: no query voxel seen
  double sum = 0.0, sum2 = 0.0;
  int cnt = 0, cnt2 = 0, le1 = 0, le2 = 0;
  for (int r = r0; r < r1; ++r) {
    const int64_t row = ((int64_t)n * rows + r) * g.w;
    int anyq = 0;
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) { const unsigned char v = q[row + x]; sq[x] = v; anyq |= v; }
    const int anyb = __syncthreads_or(anyq & 12);  // a border voxel is a mask voxel: no query voxel means no border voxel either
    if (!__syncthreads_or(anyq)) {
      for (int x = threadIdx.x; x < g.w; x += blockDim.x) { kdb[row + x] = SURF_NOKEY; kda[row + x] = SURF_NOKEY; }
      continue;
    }
    int fin0 = 0, fin1 = 0;
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const float vb = fb[row + x], va = fa[row + x];
      s0[x] = vb; s1[x] = va;
      fin0 |= vb < inf; fin1 |= va < inf;
    }
    fin0 = __syncthreads_or(fin0);
    fin1 = __syncthreads_or(fin1);
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const unsigned char v = sq[x];
      if (v & 1) maxB = fmaxf(maxB, fin0 ? line_min(s0, 1, g.w, x, sw) : inf);
      if (v & 2) maxA = fmaxf(maxA, fin1 ? line_min(s1, 1, g.w, x, sw) : inf);
    }
    if (!anyb) {  // block-uniform
      for (int x = threadIdx.x; x < g.w; x += blockDim.x) { kdb[row + x] = SURF_NOKEY; kda[row + x] = SURF_NOKEY; }
      __syncthreads();
      continue;
    }
    __syncthreads();  // every scan of F_B / F_A is done before stage 2 overwrites the LDS rows
    fin0 = 0; fin1 = 0;
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const float vd = __uint_as_float(kdb[row + x]), ve = __uint_as_float(kda[row + x]);
      s0[x] = vd; s1[x] = ve;
      fin0 |= vd < inf; fin1 |= ve < inf;
    }
    fin0 = __syncthreads_or(fin0);
    fin1 = __syncthreads_or(fin1);
    for (int x = threadIdx.x; x < g.w; x += blockDim.x) {
      const unsigned char v = sq[x];
      unsigned key0 = SURF_NOKEY, key1 = SURF_NOKEY;
      if (v & 4) {
        const float f = fin0 ? line_min(s0, 1, g.w, x, sw) : inf;
        sum += sqrt((double)f); ++cnt; le1 += f <= tau2;
        key0 = __float_as_uint(f);
      }
      if (v & 8) {
        const float f = fin1 ? line_min(s1, 1, g.w, x, sw) : inf;
        sum2 += sqrt((double)f); ++cnt2; le2 += f <= tau2;
        key1 = __float_as_uint(f);
      }
      kdb[row + x] = key0;
      kda[row + x] = key1;
    }
    __syncthreads();  // the next row's staging overwrites the LDS rows
  }
  maxB = wave_max(maxB); maxA = wave_max(maxA); sum = wave_sum_d(sum); cnt = wave_sum_i(cnt);
  sum2 = wave_sum_d(sum2); cnt2 = wave_sum_i(cnt2); le1 = wave_sum_i(le1); le2 = wave_sum_i(le2);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (ln == 0) {
    redf[0][wv] = maxB; redf[1][wv] = maxA; redd[0][wv] = sum; redd[1][wv] = sum2;
    redi[0][wv] = cnt; redi[1][wv] = cnt2; redi[2][wv] = le1; redi[3][wv] = le2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < nw; ++k) {
      maxB = fmaxf(maxB, redf[0][k]); maxA = fmaxf(maxA, redf[1][k]); sum += redd[0][k]; cnt += redi[0][k];
      sum2 += redd[1][k]; cnt2 += redi[1][k]; le1 += redi[2][k]; le2 += redi[3][k];
    }
    const int64_t o = ((int64_t)n * k1 + m) * slabs + s;
    const float hi = (float)sum, hi2 = (float)sum2;
    part[o] = maxB;
    part[npart + o] = maxA;
    part[2 * (int64_t)npart + o] = hi;
    part[3 * (int64_t)npart + o] = hi < inf ? (float)(sum - (double)hi) : 0.f;  // inf - inf would be NaN
    part[4 * (int64_t)npart + o] = __int_as_float(cnt);
    part[5 * (int64_t)npart + o] = hi2;
    part[6 * (int64_t)npart + o] = hi2 < inf ? (float)(sum2 - (double)hi2) : 0.f;
    part[7 * (int64_t)npart + o] = __int_as_float(cnt2);
    part[8 * (int64_t)npart + o] = __int_as_float(le1);
    part[9 * (int64_t)npart + o] = __int_as_float(le2);
  }
}

// Select, pass p of 4 (byte 3 - p of the key): block (chunk, volume).  Keys are the valid words (top bit clear) of the volume's two
// key arrays whose higher bytes equal the prefix found so far.  LDS atomics per block, one global atomic per non-empty bin.
__global__ void __launch_bounds__(256) surf_sel_hist_kernel(const unsigned* __restrict__ ka, const unsigned* __restrict__ kb, int64_t voxv,
                                                            int k1, int m, int pass, const unsigned* __restrict__ state,
                                                            unsigned* __restrict__ hist) {
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int n = blockIdx.y;
  const unsigned prefix = state[((int64_t)n * k1 + m) * SURF_SEL_STATE];
  const int shift = 24 - 8 * pass;
  ka += (int64_t)n * voxv;
  kb += (int64_t)n * voxv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < voxv; i += (int64_t)gridDim.x * 256) {
    const unsigned u[2] = {ka[i], kb[i]};
#pragma unroll
    for (int a = 0; a < 2; ++a)  // 64-bit shift: 32 - 8 pass can be 32 (pass 0 looks at every valid key)
      if ((int)u[a] >= 0 && (unsigned)(((unsigned long long)(u[a] ^ prefix)) >> (shift + 8)) == 0u) atomicAdd(&h[(u[a] >> shift) & 0xFFu], 1u);
  }
  __syncthreads();
  const unsigned c = h[threadIdx.x];
  if (c) atomicAdd(&hist[(int64_t)n * 256 + threadIdx.x], c);
}

// One block per volume: the bin that holds the key of ascending rank r (1-based among the keys under the prefix) extends the prefix.
// Pass 0 derives r = floor((n - 1) * qf) + 1 from its own total n = |dA| + |dB| (qf = percentile / 100, numpy's linear method).
// The histogram is cleared for the next pass.  After pass 3: state = bits of v[k] | rank of position k among the keys equal to
// v[k] | number of those keys, so v[k + 1] = v[k] exactly when the rank is below the number.
__global__ void __launch_bounds__(256) surf_sel_scan_kernel(int pass, int k1, int m, double qf, unsigned* __restrict__ hist,
                                                            unsigned* __restrict__ state) {
  __shared__ unsigned s[256];
  const int t = threadIdx.x;
  unsigned* hv = hist + (int64_t)blockIdx.x * 256;
  unsigned* st = state + ((int64_t)blockIdx.x * k1 + m) * SURF_SEL_STATE;
  const unsigned c = hv[t];
  hv[t] = 0u;
  s[t] = c;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {  // inclusive prefix sums: s[t] = number of keys in bins <= t
    const unsigned add = t >= o ? s[t - o] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const unsigned total = s[255], prefix = st[0];
  const unsigned r = pass == 0 ? (total ? (unsigned)floor((double)(total - 1u) * qf) + 1u : 0u) : st[1];
  const unsigned below = s[t] - c;
  __syncthreads();  // every thread has read the state before the one writer below
  if (r > 0u && s[t] >= r && below < r) {  // exactly one bin
    st[0] = prefix | ((unsigned)t << (24 - 8 * pass));
    st[1] = r - below;
    st[2] = c;
  }
  if (pass == 0 && t == 0) st[4] = total;
}

// state[3] = the smallest key above v[k]; needed only where position k is the last of the keys equal to v[k]
__global__ void __launch_bounds__(256) surf_sel_next_kernel(const unsigned* __restrict__ ka, const unsigned* __restrict__ kb, int64_t voxv,
                                                            int k1, int m, unsigned* __restrict__ state) {
  __shared__ unsigned red[4];
  const int n = blockIdx.y;
  unsigned* st = state + ((int64_t)n * k1 + m) * SURF_SEL_STATE;
  const unsigned vk = st[0];
  if (st[1] < st[2]) return;  // block-uniform; no block writes st[0..2]
  unsigned mn = SURF_NOKEY;
  ka += (int64_t)n * voxv;
  kb += (int64_t)n * voxv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < voxv; i += (int64_t)gridDim.x * 256) {
    const unsigned u[2] = {ka[i], kb[i]};
#pragma unroll
    for (int a = 0; a < 2; ++a)
      if ((int)u[a] >= 0 && u[a] > vk && u[a] < mn) mn = u[a];
  }
  mn = wave_min_u(mn);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) mn = red[k] < mn ? red[k] : mn;
    if (mn != SURF_NOKEY) atomicMin(&st[3], mn);
  }
}

// hd_pct / assd / nsd [nvol][k1]: NaN, NaN, 0 where A is empty; +inf, +inf, 0 where only B is
__global__ void surf_finalize_ext_kernel(const float* __restrict__ part, int npart, int nvol, int k1, int slabs, double qf,
                                         const unsigned* __restrict__ state, float* __restrict__ hd_pct, float* __restrict__ assd,
                                         float* __restrict__ nsd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nvol * k1) return;
  double sum = 0.0, sum2 = 0.0;
  long long cnt = 0, cnt2 = 0, le = 0;
  for (int s = 0; s < slabs; ++s) {
    const int64_t o = (int64_t)i * slabs + s;
    sum += (double)part[2 * (int64_t)npart + o] + (double)part[3 * (int64_t)npart + o];
    cnt += __float_as_int(part[4 * (int64_t)npart + o]);
    sum2 += (double)part[5 * (int64_t)npart + o] + (double)part[6 * (int64_t)npart + o];
    cnt2 += __float_as_int(part[7 * (int64_t)npart + o]);
    le += (long long)__float_as_int(part[8 * (int64_t)npart + o]) + __float_as_int(part[9 * (int64_t)npart + o]);
  }
  if (cnt == 0 || cnt2 == 0) {
    const float e = cnt == 0 ? __builtin_nanf("") : __builtin_inff();
    hd_pct[i] = e; assd[i] = e; nsd[i] = 0.f;
    return;
  }
  const unsigned* st = state + (int64_t)i * SURF_SEL_STATE;
  const long long n = cnt + cnt2;  // == st[4], the select's own total
  const double pos = (double)(n - 1) * qf, kf = floor(pos), t = pos - kf;
  const double vk = sqrt((double)__uint_as_float(st[0]));
  const bool same = (long long)kf + 1 >= n || st[1] < st[2];  // v[min(k + 1, n - 1)] == v[k]
  const double vn = same ? vk : sqrt((double)__uint_as_float(st[3]));
  hd_pct[i] = (float)(vk + (vn - vk) * t);
  assd[i] = (float)((sum / (double)cnt + sum2 / (double)cnt2) * 0.5);
  nsd[i] = (float)((double)le / (double)n);
}

struct SurfExtPlan {
  SurfPlan base;  // the same slabs as mia_surface_distance: hd / asd sum the same partials in the same order
  int64_t part, hist, state, total;  // offsets in floats; total workspace floats
};

bool surf_plan_ext(int nvol, int d, int h, int w, int k1, SurfExtPlan& p) {
  if (!surf_plan(nvol, d, h, w, k1, p.base) || nvol > SURF_EXT_MAX_NVOL) return false;
  p.part = 4 * p.base.vox + (p.base.vox + 3) / 4;  // four fields | query bytes
  p.hist = p.part + SURF_NPART_EXT * p.base.npart;
  p.state = p.hist + (int64_t)nvol * 256;
  p.total = p.state + (int64_t)nvol * k1 * SURF_SEL_STATE;
  return p.total <= 0x7fffffff;
}

// the argument checks shared by both entry points; fills the plan of mia_surface_distance
int surf_check_args(const char* fn, bool ptrs, int nvol, int ndim, int d, int h, int w, int k1, float& sd, float sh, float sw, SurfPlan& p) {
  MIA_CHECK_ARG(ptrs, "%s: null pointer", fn);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= SURF_MAXK, "%s: k1=%d not in [1,%d]", fn, k1, SURF_MAXK);
  MIA_CHECK_ARG(ndim == 2 || ndim == 3, "%s: ndim=%d not 2 or 3", fn, ndim);
  MIA_CHECK_ARG(ndim == 3 || d == 1, "%s: ndim 2 needs d == 1 (got d=%d)", fn, d);
  if (ndim == 2) sd = 1.f;  // unused: no D axis
  MIA_CHECK_ARG(sd > 0.f && sh > 0.f && sw > 0.f && sd < __builtin_inff() && sh < __builtin_inff() && sw < __builtin_inff(),
                "%s: spacing (%g, %g, %g) must be finite and > 0", fn, (double)sd, (double)sh, (double)sw);
  // a non-feature voxel must never hold a squared distance of 0 (pass 1 tells feature voxels by their 0)
  MIA_CHECK_ARG(sd * sd >= 1.17549435e-38f && sh * sh >= 1.17549435e-38f && sw * sw >= 1.17549435e-38f,
                "%s: spacing (%g, %g, %g) too small: its square is not a normal fp32", fn, (double)sd, (double)sh, (double)sw);
  MIA_CHECK_ARG(surf_plan(nvol, d, h, w, k1, p),
                "%s: extents nvol=%d d=%d h=%d w=%d k1=%d outside the limits (d <= %d, h, w <= %d, nvol * k1 <= %d, "
                "workspace < 2^31 floats)", fn, nvol, d, h, w, k1, SURF_MAX_D, SURF_MAX_HW, SURF_MAX_PART / SURF_NPART);
  // squared physical extents must stay far inside fp32 (the scans add (s r)^2 terms of up to the whole diagonal)
  const double diag = (double)sd * sd * d * d + (double)sh * sh * h * h + (double)sw * sw * w * w;
  MIA_CHECK_ARG(diag < 1e30, "%s: spacing x extent too large for fp32 squared distances", fn);
  return MIA_OK;
}

int surf_pass2_cw(int h, int w) {
  int cw = 64;
  while (cw > 1 && (int64_t)cw * h * 4 > SURF_P2_LDS) cw >>= 1;
  while (cw > 1 && cw / 2 >= w) cw >>= 1;  // no tile wider than the image
  return cw;
}

}  // namespace

extern "C" int mia_surface_distance_workspace(int nvol, int d, int h, int w, int k1) {
  SurfPlan p;
  return surf_plan(nvol, d, h, w, k1, p) ? (int)p.total : -1;
}

extern "C" int mia_surface_distance(const long long* pred, const long long* labels, int nvol, int ndim, int d, int h, int w, int k1, float sd,
                                    float sh, float sw, float* workspace, float* hd, float* asd, void* stream) {
  SurfPlan p;
  if (const int rc = surf_check_args("mia_surface_distance", pred && labels && workspace && hd && asd, nvol, ndim, d, h, w, k1, sd, sh, sw, p))
    return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SurfGeom g{nvol, d, h, w, ndim};
  float* fb = workspace;
  float* fa = workspace + p.vox;
  float* fdb = workspace + 2 * p.vox;
  unsigned char* q = reinterpret_cast<unsigned char*>(workspace + 3 * p.vox);
  float* part = workspace + 3 * p.vox + (p.vox + 3) / 4;
  const int cw = surf_pass2_cw(h, w);
  const int tiles = ceil_div(w, cw);
  const int64_t cols = (int64_t)nvol * h * w;
  const size_t lds3 = (size_t)3 * w * 4 + ((w + 3) / 4) * 4;
  for (int m = 0; m < k1; ++m) {
    hipLaunchKernelGGL(surf_pass1_kernel<false>, dim3((unsigned)ceil_div64(cols, 256)), dim3(256), 0, st, pred, labels, g, m, sd, fb, fa,
                       fdb, (float*)nullptr, q);
    hipLaunchKernelGGL(surf_pass2_kernel, dim3((unsigned)(nvol * d * tiles), 3), dim3(256), (size_t)h * cw * 4, st, fb, fa, fdb,
                       (float*)nullptr, g, cw, tiles, sh);
    hipLaunchKernelGGL(surf_pass3_kernel, dim3((unsigned)(nvol * p.slabs)), dim3(256), lds3, st, fb, fa, fdb, q, g, p.slabs, k1, m, sw,
                       part, (int)p.npart);
  }
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(ceil_div(nvol * k1, 64)), dim3(64), 0, st, part, (int)p.npart, nvol, k1, p.slabs, hd, asd);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_surface_metrics_workspace(int nvol, int d, int h, int w, int k1) {
  SurfExtPlan p;
  return surf_plan_ext(nvol, d, h, w, k1, p) ? (int)p.total : -1;
}

extern "C" int mia_surface_metrics(const long long* pred, const long long* labels, int nvol, int ndim, int d, int h, int w, int k1, float sd,
                                   float sh, float sw, double percentile, const float* tolerance, float* workspace, float* hd, float* asd,
                                   float* hd_pct, float* assd, float* nsd, void* stream) {
  SurfExtPlan p;
  if (const int rc = surf_check_args("mia_surface_metrics", pred && labels && tolerance && workspace && hd && asd && hd_pct && assd && nsd,
                                     nvol, ndim, d, h, w, k1, sd, sh, sw, p.base))
    return rc;
  MIA_CHECK_ARG(surf_plan_ext(nvol, d, h, w, k1, p),
                "mia_surface_metrics: extents nvol=%d d=%d h=%d w=%d k1=%d outside the limits (nvol <= %d, workspace < 2^31 floats)", nvol, d,
                h, w, k1, SURF_EXT_MAX_NVOL);
  MIA_CHECK_ARG(percentile > 0.0 && percentile <= 100.0, "mia_surface_metrics: percentile=%g not in (0, 100]", percentile);
  float tau2[SURF_MAXK];
  for (int m = 0; m < k1; ++m) {
    MIA_CHECK_ARG(tolerance[m] >= 0.f && tolerance[m] < __builtin_inff(), "mia_surface_metrics: tolerance[%d]=%g must be finite and >= 0", m,
                  (double)tolerance[m]);
    tau2[m] = tolerance[m] * tolerance[m];  // the kernels compare squared distances in fp32
  }
  const double qf = percentile / 100.0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const SurfGeom g{nvol, d, h, w, ndim};
  const int64_t vox = p.base.vox, voxv = (int64_t)d * h * w;
  const int slabs = p.base.slabs, npart = (int)p.base.npart;
  float* fb = workspace;
  float* fa = workspace + vox;
  float* fdb = workspace + 2 * vox;
  float* fda = workspace + 3 * vox;
  unsigned char* q = reinterpret_cast<unsigned char*>(workspace + 4 * vox);
  float* part = workspace + p.part;
  unsigned* hist = reinterpret_cast<unsigned*>(workspace + p.hist);
  unsigned* state = reinterpret_cast<unsigned*>(workspace + p.state);
  unsigned* ka = reinterpret_cast<unsigned*>(fdb);  // F_dB / F_dA as words: pass 3 turns them into the key arrays
  unsigned* kb = reinterpret_cast<unsigned*>(fda);
  const int cw = surf_pass2_cw(h, w);
  const int tiles = ceil_div(w, cw);
  const int64_t cols = (int64_t)nvol * h * w;
  const size_t lds3 = (size_t)2 * w * 4 + ((w + 3) / 4) * 4;
  int64_t chunks = ceil_div64(voxv, 256 * 8);  // select blocks per volume: at least 8 keys of each array per thread, and about
  if (chunks > ceil_div(2048, nvol)) chunks = ceil_div(2048, nvol);  // 2048 blocks in all (integer atomics: any grid gives the same counts)
  const dim3 sel((unsigned)chunks, (unsigned)nvol);
  for (int m = 0; m < k1; ++m) {
    hipLaunchKernelGGL(surf_pass1_kernel<true>, dim3((unsigned)ceil_div64(cols, 256)), dim3(256), 0, st, pred, labels, g, m, sd, fb, fa,
                       fdb, fda, q);
    hipLaunchKernelGGL(surf_pass2_kernel, dim3((unsigned)(nvol * d * tiles), 4), dim3(256), (size_t)h * cw * 4, st, fb, fa, fdb, fda, g, cw,
                       tiles, sh);
    hipLaunchKernelGGL(surf_pass3_ext_kernel, dim3((unsigned)(nvol * slabs)), dim3(256), lds3, st, fb, fa, ka, kb, q, g, slabs, k1, m, sw,
                       tau2[m], part, npart, hist, state);
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(surf_sel_hist_kernel, sel, dim3(256), 0, st, ka, kb, voxv, k1, m, pass, state, hist);
      hipLaunchKernelGGL(surf_sel_scan_kernel, dim3((unsigned)nvol), dim3(256), 0, st, pass, k1, m, qf, hist, state);
    }
    hipLaunchKernelGGL(surf_sel_next_kernel, sel, dim3(256), 0, st, ka, kb, voxv, k1, m, state);
  }
  hipLaunchKernelGGL(surf_finalize_kernel, dim3(ceil_div(nvol * k1, 64)), dim3(64), 0, st, part, npart, nvol, k1, slabs, hd, asd);
  hipLaunchKernelGGL(surf_finalize_ext_kernel, dim3(ceil_div(nvol * k1, 64)), dim3(64), 0, st, part, npart, nvol, k1, slabs, qf, state, hd_pct,
                     assd, nsd);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
