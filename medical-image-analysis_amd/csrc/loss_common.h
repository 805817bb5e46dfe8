// What the loss kernels share (dice_ce.hip, seg_loss.hip, region_loss.hip, ds_loss.hip, and the streaming losses boundary.hip,
// consistency.hip, cps.hip, urpc.hip): ONE definition of each piece, so that the files cannot drift apart.  Arithmetic that differs
// between the losses stays in their own files.
#pragma once
#include "common.h"

#define LOSS_MAXK 8
// MIA_LOSS_* flags of the fused Dice + CE (dice_ce.hip) and of the deep-supervision loss (ds_loss.hip)
#define LF_SOFTMAX 1
#define LF_DO_BG 2
#define LF_BATCH 4
#define LF_SQUARED 8
#define LF_DENSE 16  // `labels` points at a contiguous fp32 [B][K1][HW] target (already one-hot / soft; dice_loss.py:40-41 skips the encoder)

struct LossGeom { int64_t sn, sk, sp; };  // element strides of a logits-shaped tensor: image, class, pixel

// Which label values are "ignore": one 64-bit value for int64 labels, one byte (or none) for uint8 labels.
struct LossIgnore {
  int on;           // an ignore label is set
  unsigned lo, hi;  // the ignore label as two words (int64 labels)
  int byte;         // its value when it fits a byte, else -1 (uint8 labels can then never be ignored)
};
static inline LossIgnore make_ignore(bool on, int64_t ign) {
  LossIgnore g;
  g.on = on ? 1 : 0;
  g.lo = (unsigned)((uint64_t)ign & 0xFFFFFFFFull);
  g.hi = (unsigned)((uint64_t)ign >> 32);
  g.byte = (on && ign >= 0 && ign < 256) ? (int)ign : -1;
  return g;
}

// Four consecutive int64 labels at a 16-byte aligned `p`, read as two 16-byte units and split into low / high words.
__device__ __forceinline__ void load_label_quad(const long long* p, unsigned (&lo)[4], unsigned (&hi)[4]) {
  const u32x4 l0 = reinterpret_cast<const u32x4*>(p)[0], l1 = reinterpret_cast<const u32x4*>(p)[1];
  lo[0] = l0[0]; hi[0] = l0[1]; lo[1] = l0[2]; hi[1] = l0[3];
  lo[2] = l1[0]; hi[2] = l1[1]; lo[3] = l1[2]; hi[3] = l1[3];
}
// the two-label form: one 16-byte unit
__device__ __forceinline__ void load_label_pair(const long long* p, unsigned (&lo)[2], unsigned (&hi)[2]) {
  const u32x4 l = *reinterpret_cast<const u32x4*>(p);
  lo[0] = l[0]; hi[0] = l[1]; lo[1] = l[2]; hi[1] = l[3];
}

// Channels-last logits of four consecutive pixels = K1 consecutive 16-byte units f[0..K1): pixel j's K1 values out of them.  Used by
// the forward kernels; dice_ce_bwd_fast_kernel and seg_loss_bwd_fast_kernel keep the indexing inline, because with a helper the
// compiler fuses their multiply-adds differently for K1 = 3 and the gradient's bits change.
template <int K1>
__device__ __forceinline__ void quad_unpack(const f32x4* f, int j, float (&v)[K1]) {
#pragma unroll
  for (int k = 0; k < K1; ++k) v[k] = f[(j * K1 + k) >> 2][(j * K1 + k) & 3];
}

// Block sums of up to NF float and NI int values of a 256-thread block behind ONE barrier: put() sums a group of values over the
// wave and parks them in consecutive slots of the LDS; after the caller's __syncthreads() one thread per slot adds the four waves
// with sum_f() / sum_i(), always in the same order -- no atomics, so every result is bit-identical run to run.
template <int NF, int NI>
struct LossBlockSums {
  float (*f)[NF];
  int (*i)[NI ? NI : 1];
  int w, l;  // this thread's wave and lane
  template <int MF, int MI>
  __device__ __forceinline__ void put(int fslot, const float (&fv)[MF], int islot, const int (&iv)[MI]) {
    float a[MF];
    int c[MI];
#pragma unroll
    for (int m = 0; m < MF; ++m) a[m] = wave_sum(fv[m]);
#pragma unroll
    for (int m = 0; m < MI; ++m) c[m] = wave_sum_i(iv[m]);
    if (l == 0) {
#pragma unroll
      for (int m = 0; m < MF; ++m) f[w][fslot + m] = a[m];
#pragma unroll
      for (int m = 0; m < MI; ++m) i[w][islot + m] = c[m];
    }
  }
  template <int MF>
  __device__ __forceinline__ void put(int fslot, const float (&fv)[MF]) {
    float a[MF];
#pragma unroll
    for (int m = 0; m < MF; ++m) a[m] = wave_sum(fv[m]);
    if (l == 0) {
#pragma unroll
      for (int m = 0; m < MF; ++m) f[w][fslot + m] = a[m];
    }
  }
  __device__ __forceinline__ float sum_f(int slot) const { return f[0][slot] + f[1][slot] + f[2][slot] + f[3][slot]; }
  __device__ __forceinline__ int sum_i(int slot) const { return i[0][slot] + i[1][slot] + i[2][slot] + i[3][slot]; }
};
template <int NF, int NI>
__device__ __forceinline__ LossBlockSums<NF, NI> loss_block_sums() {
  __shared__ float f[4][NF];
  __shared__ int i[4][NI ? NI : 1];
  return {f, i, (int)(threadIdx.x >> 6), (int)(threadIdx.x & 63)};
}

// ---- double-precision sums that travel as float pairs (boundary.hip, consistency.hip, cps.hip, urpc.hip)
// A block's sum is kept in double, parked as hi = (float)v, lo = (float)(v - hi), and read back as (double)hi + (double)lo.
__device__ __forceinline__ void loss_split(double v, float* p) {
  p[0] = (float)v;
  p[1] = (float)(v - (double)p[0]);
}

// The wave's sum of v in double as a pair in lane 0, zeros in the other lanes: LossBlockSums::put() then adds one pair and 63 zeros
// in fp32, which is exact (a pair summed in fp32 across the wave would round at every level).  boundary.hip and consistency.hip park
// a pair per THREAD instead and let put() add them in fp32; the two forms round differently and each kernel keeps its own.
__device__ __forceinline__ void loss_wave_pair(double v, int lane, float* p) {
  loss_split(wave_sum_d(v), p);
  p[0] = lane == 0 ? p[0] : 0.f;
  p[1] = lane == 0 ? p[1] : 0.f;
}

// The head of a finalize kernel (one block of 256 threads): the totals of nq <= MAXQ quantities whose per-block pairs lie in
// part [nparts][nq][2], and of NC counts in cnt [nparts][NC].  A thread adds hi + lo of parts t, t + 256, ... in double (counts in
// int64) into its entry of a 256-entry LDS array per quantity; then one thread per quantity adds the 256 entries in index order.  The
// sequence of additions of every quantity is fixed, so the totals are bit-identical run to run.  f[q] and n[c] are LDS and valid in
// every thread on return.
struct LossTotals {
  const double* f;
  const long long* n;
};
template <int MAXQ, int NC>
__device__ __forceinline__ LossTotals loss_totals(const float* __restrict__ part, const int* __restrict__ cnt, int nparts, int nq) {
  static_assert(MAXQ <= 64, "one thread of the first wave per quantity");
  __shared__ double fsh[MAXQ][256], ftot[MAXQ];
  __shared__ long long nsh[NC ? NC : 1][256], ntot[NC ? NC : 1];
  for (int q = 0; q < nq; ++q) {
    double my = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
      const float* o = part + ((size_t)i * nq + q) * 2;
      my += (double)o[0] + (double)o[1];
    }
    fsh[q][threadIdx.x] = my;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    long long my = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) my += cnt[(size_t)i * NC + c];
    nsh[c][threadIdx.x] = my;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < nq) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += fsh[t][i];
    ftot[t] = s;
  } else if (t >= 64 && t < 64 + NC) {  // the counts in the second wave, beside the sums
    long long s = 0;
    for (int i = 0; i < 256; ++i) s += nsh[t - 64][i];
    ntot[t - 64] = s;
  }
  __syncthreads();
  return {ftot, ntot};
}

// The tail of every finalize kernel (one block), after out[0..3) and coef[0..ncoef) are written.
// A label outside the classes (and not the ignore label): the reference raises (scatter index error in DiceLoss, dice_loss.py:25-30;
// target bound check in CrossEntropyLoss).  A device kernel cannot raise, so the result is made unusable instead of silently
// training on such masks: loss values and the backward coefficients (hence every gradient) become NaN; ops.check_labels() turns the
// flag into an exception at the caller's next host sync.
// bad_label[0] is the working flag the pixel kernels raise; it is OR-ed into bad_label[1] -- the STICKY verdict that check_labels
// reads and clears, so a clean forward (validation, a second loss term, a deep-supervision head) between the offending call and the
// check cannot erase it -- and re-armed here, so the caller never has to clear it between calls.
__device__ __forceinline__ void loss_bad_label_verdict(int* bad_label, float* out, float* coef, int ncoef) {
  __syncthreads();
  const int bad = bad_label[0];
  __syncthreads();
  if (threadIdx.x == 0) { if (bad) bad_label[1] = 1; bad_label[0] = 0; }
  if (bad) {
    const float qn = __builtin_nanf("");
    if (threadIdx.x < 3) out[threadIdx.x] = qn;
    for (int i = threadIdx.x; i < ncoef; i += blockDim.x) coef[i] = qn;
  }
}

// dice_ce.hip: launches dice_ce_finalize_kernel on `part` [B][slabs][K1][3] / `cepart` [B][slabs], for the other files that produce
// this layout (ds_loss.hip)
int mia_dice_ce_finalize_launch(const float* part, const float* cepart, int nb, int slabs, int k1, int64_t hw, int flags, float smooth,
                                float dice_w, float ce_w, float* sums, float* coef, float* out, int* bad_label, hipStream_t st);
