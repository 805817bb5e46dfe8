// BADGE gradient embeddings for a whole batch of pool images in one fused pass (reference src/activelearning/badge_selector.py:19-35
// `image_wise_grad` and :80-96, the per-image loss it differentiates): the gradient of  CE(logits, a) + DiceLoss(logits, a)  on the
// model's own arg-max labels a, with respect to the weight of the 1x1 head  logits = W feat + bias,  has a closed form per image:
//
//   p = softmax_k(logits);  a = argmax_k logits (lowest index on a tie);  y = onehot(a);  P = H W
//   I_c = sum p_c y_c      Z_c = sum p_c  (sum p_c^2 when squared)      Y_c = sum y_c
//   D_c = Z_c + Y_c + smooth          N_c = 2 I_c + smooth
//   S   = classes counted by Dice: all K1 when do_bg, else 1..K1-1;   n = |S|
//   loss = (1/P) sum_pixels (logsumexp - logit_a)  +  (1/n) sum_{c in S} (1 - N_c / D_c)
//   g_c(pixel)  = (1/n) ( -2 y_c / D_c + (N_c / D_c^2) (2 p_c when squared, else 1) )  for c in S, else 0
//   dz_c(pixel) = p_c ( g_c - sum_j p_j g_j )  +  (p_c - y_c) / P
//   G[c, k]     = sum_pixels dz_c(pixel) feat_k(pixel)
//
// Pass one reduces I, Z, Y and the CE sum per (image, slab); a one-block-per-image kernel sums the slabs in double and writes the
// loss and the two Dice coefficients per class; pass two recomputes p per pixel, forms dz in registers / LDS (never in memory) and
// accumulates G per (image, slab); the last kernel sums the slabs in double.  No float atomics: fp32 partials per block, summed in a
// fixed order, so results are bit-identical run to run.  The slab geometry depends on H W alone, and every image is reduced by its
// own blocks, so an image gets the same bits alone or inside any batch.  Nothing synchronises with the host; every launch goes to
// the caller's stream.
//
// Cancellation: with mx = logit_a the arg-max class has exp(0) = 1 exactly, so  1 - p_a = so / (1 + so)  with so = sum_{k != a} e_k  and
// logsumexp - logit_a = log1p(so)  carry no rounding from a subtraction of nearly equal numbers;  g_c - sum_j p_j g_j  is formed as
// sum_j p_j (g_c - g_j)  for the same reason (the j = c term vanishes, and for c = a only the small p_j remain).
#include "common.h"

#define BE_MAXK 8
#define BE_MAXC 128
#define BE_TILE 1024      // pixels per tile: 256 threads x 4 consecutive pixels
#define BE_SLAB_TILES 4   // tiles per slab while the image has at most BE_MAX_SLABS such slabs
#define BE_MAX_SLABS 256
#define BE_LD_GENERIC 0   // scalar loads through (sk, sp)
#define BE_LD_CLAST 1     // channels-last logits (sk = 1, sp = K1): the quad's 4 K1 values in K1 16-byte loads
#define BE_LD_PLANAR 2    // planar logits (sp = 1): one 16-byte load per class

struct BeGeom { int64_t sn, sk, sp; };

// The K1 logits of the four consecutive pixels p0 .. p0 + 3 of one image (`base` = its first logit).  Every mode hands the same
// pixels to the same thread, so the arithmetic -- and the bits -- do not depend on the layout.
template <int K1>
__device__ __forceinline__ void be_load_quad(const float* __restrict__ base, int64_t p0, int64_t r1, const BeGeom& g, int mode,
                                             float (&v)[4][K1]) {
  if (mode == BE_LD_CLAST) {
    const f32x4* s = reinterpret_cast<const f32x4*>(base + p0 * K1);
    f32x4 f[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) f[k] = s[k];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < K1; ++k) v[j][k] = f[(j * K1 + k) >> 2][(j * K1 + k) & 3];
  } else if (mode == BE_LD_PLANAR) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      const f32x4 f = *reinterpret_cast<const f32x4*>(base + k * g.sk + p0);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j][k] = f[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < K1; ++k) v[j][k] = (p0 + j < r1) ? base[(p0 + j) * g.sp + k * g.sk] : 0.f;
  }
}

// p = softmax(v), a = argmax (strict >: the lowest index wins a tie, like torch.argmax), q = 1 - p_a, so = sum_{k != a} exp(v_k - v_a)
template <int K1>
struct BePix {
  float p[K1], q, so;
  int a;
  __device__ __forceinline__ void softmax(const float (&v)[K1]) {
    float mx = v[0];
    a = 0;
#pragma unroll
    for (int k = 1; k < K1; ++k)
      if (v[k] > mx) { mx = v[k]; a = k; }
    float e[K1];
    so = 0.f;
#pragma unroll
    for (int k = 0; k < K1; ++k) {
      e[k] = (k == a) ? 1.f : expf(v[k] - mx);
      so += (k == a) ? 0.f : e[k];
    }
    const float inv = 1.f / (1.f + so);
#pragma unroll
    for (int k = 0; k < K1; ++k) p[k] = e[k] * inv;
    q = so * inv;
  }
};

// ---------------------------------------------------------------- pass one: I, Z, CE sum (fp32) and Y (int) per (image, slab)
// slice of block (b, s): [K1] I, [K1] Z, CE, then [K1] ints Y
template <int K1>
__global__ __launch_bounds__(256) void badge_sums_kernel(const float* __restrict__ logits, int64_t hw, BeGeom g, int mode, int squared,
                                                         int64_t per, int slabs, float* __restrict__ part) {
  __shared__ float redf[4][2 * K1 + 1];
  __shared__ int redi[4][K1];
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs, tid = threadIdx.x;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const float* base = logits + b * g.sn;
  float si[K1], sz[K1], ce = 0.f;
  int cy[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) { si[k] = 0.f; sz[k] = 0.f; cy[k] = 0; }
  for (int64_t t0 = r0; t0 < r1; t0 += BE_TILE) {
    const int64_t p0 = t0 + 4 * tid;
    if (p0 >= r1) continue;
    float v[4][K1];
    be_load_quad<K1>(base, p0, r1, g, mode, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (p0 + j >= r1) continue;
      BePix<K1> px;
      px.softmax(v[j]);
#pragma unroll
      for (int k = 0; k < K1; ++k) {
        si[k] += (px.a == k) ? px.p[k] : 0.f;
        sz[k] += squared ? px.p[k] * px.p[k] : px.p[k];
        cy[k] += (px.a == k) ? 1 : 0;
      }
      ce += log1pf(px.so);
    }
  }
  const int w = tid >> 6, l = tid & 63;
#pragma unroll
  for (int k = 0; k < K1; ++k) {
    const float a = wave_sum(si[k]), z = wave_sum(sz[k]);
    int y = cy[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) y += __shfl_xor(y, o, 64);
    if (l == 0) { redf[w][k] = a; redf[w][K1 + k] = z; redi[w][k] = y; }
  }
  const float c = wave_sum(ce);
  if (l == 0) redf[w][2 * K1] = c;
  __syncthreads();
  float* slice = part + (size_t)blockIdx.x * (3 * K1 + 1);
  if (tid < 2 * K1 + 1) {
    slice[tid] = redf[0][tid] + redf[1][tid] + redf[2][tid] + redf[3][tid];
  } else if (tid >= 64 && tid < 64 + K1) {
    const int i = tid - 64;
    reinterpret_cast<int*>(slice + 2 * K1 + 1)[i] = redi[0][i] + redi[1][i] + redi[2][i] + redi[3][i];
  }
}

// ---------------------------------------------------------------- per image: slabs summed in double, loss and Dice coefficients
// coef[b][c][2] = (-2 / (n D_c), N_c / (n D_c^2)) for c in S, (0, 0) otherwise
__global__ __launch_bounds__(64) void badge_finalize_kernel(const float* __restrict__ part, int slabs, int k1, int64_t hw, float smooth,
                                                            int do_bg, float* __restrict__ coef, float* __restrict__ loss) {
  __shared__ double tot[3 * BE_MAXK + 1];
  const int b = blockIdx.x, i = threadIdx.x, nv = 3 * k1 + 1;
  if (i < nv) {
    double a = 0.0;
    for (int s = 0; s < slabs; ++s) {
      const float* slice = part + ((size_t)b * slabs + s) * nv;
      a += (i <= 2 * k1) ? (double)slice[i] : (double)reinterpret_cast<const int*>(slice)[i];
    }
    tot[i] = a;
  }
  __syncthreads();
  const int kb = do_bg ? 0 : 1;
  const double n = (double)(k1 - kb), sm = (double)smooth;
  if (i < k1) {
    const double num = 2.0 * tot[i] + sm, den = tot[k1 + i] + tot[2 * k1 + 1 + i] + sm;
    const bool in = i >= kb;
    coef[((size_t)b * k1 + i) * 2] = in ? (float)(-2.0 / (n * den)) : 0.f;
    coef[((size_t)b * k1 + i) * 2 + 1] = in ? (float)(num / (n * den * den)) : 0.f;
  }
  if (i == 0) {
    double d = 0.0;
    for (int c = kb; c < k1; ++c) d += 1.0 - (2.0 * tot[c] + sm) / (tot[k1 + c] + tot[2 * k1 + 1 + c] + sm);
    loss[b] = (float)(tot[2 * k1] / (double)hw + d / n);
  }
}

// ---------------------------------------------------------------- pass two: G partial per (image, slab)
// Four channels of one pixel per lane and step: 16-byte (fp32) / 8-byte (bf16) loads, consecutive lanes on consecutive addresses.
__device__ __forceinline__ f32x4 be_load_feat(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 be_load_feat(const bf16_t* p) {
  const u32x2 w = *reinterpret_cast<const u32x2*>(p);
  f32x4 f;
  f[0] = __builtin_bit_cast(float, w[0] << 16); f[1] = __builtin_bit_cast(float, w[0] & 0xFFFF0000u);
  f[2] = __builtin_bit_cast(float, w[1] << 16); f[3] = __builtin_bit_cast(float, w[1] & 0xFFFF0000u);
  return f;
}

// With U = C0 / 4 channel groups, thread t < (256 / U) U owns group t % U and the pixels t / U, t / U + 256 / U, .. of every tile, so its
// K1 x 4 accumulators belong to fixed channels while the block's loads stay contiguous.  Per tile: every thread forms dz of its four
// pixels once (phase A, into LDS), then the owners stream the features against it (phase B).
template <int K1, typename FT>
__global__ __launch_bounds__(256) void badge_embed_kernel(const float* __restrict__ logits, const FT* __restrict__ feat, int64_t hw, int c0,
                                                          BeGeom g, int mode, int squared, int64_t per, int slabs,
                                                          const float* __restrict__ coef, float* __restrict__ part) {
  constexpr int KP = K1 <= 4 ? 4 : 8;  // dz row in LDS, padded to whole 16-byte units
  constexpr int NV = KP / 4;
  __shared__ __attribute__((aligned(16))) float sm[BE_TILE * KP];  // dz of one tile; reused for the block reduction (256 K1 4 <= BE_TILE KP)
  const int b = blockIdx.x / slabs, s = blockIdx.x % slabs, tid = threadIdx.x;
  const int64_t r0 = s * per, r1 = r0 + per < hw ? r0 + per : hw;
  const int nu = c0 >> 2, ppi = 256 / nu, unit = tid % nu, slot = tid / nu;
  const bool owner = slot < ppi;
  const float* base = logits + b * g.sn;
  const FT* fb = feat + (size_t)b * hw * c0 + unit * 4;
  const float inv_p = (float)(1.0 / (double)hw);
  float al[K1], be[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) { al[k] = coef[((size_t)b * K1 + k) * 2]; be[k] = coef[((size_t)b * K1 + k) * 2 + 1]; }
  f32x4 acc[K1];
#pragma unroll
  for (int k = 0; k < K1; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4* smv = reinterpret_cast<f32x4*>(sm);

  for (int64_t t0 = r0; t0 < r1; t0 += BE_TILE) {
    const int64_t p0 = t0 + 4 * tid;
    if (p0 < r1) {
      float v[4][K1];
      be_load_quad<K1>(base, p0, r1, g, mode, v);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        BePix<K1> px;
        px.softmax(v[j]);
        float gk[K1], dz[KP];
#pragma unroll
        for (int k = 0; k < K1; ++k) gk[k] = (px.a == k ? al[k] : 0.f) + be[k] * (squared ? 2.f * px.p[k] : 1.f);
#pragma unroll
        for (int c = 0; c < K1; ++c) {
          float t = 0.f;
#pragma unroll
          for (int k = 0; k < K1; ++k)
            if (k != c) t += px.p[k] * (gk[c] - gk[k]);
          dz[c] = px.p[c] * t + (px.a == c ? -px.q : px.p[c]) * inv_p;
        }
#pragma unroll
        for (int c = K1; c < KP; ++c) dz[c] = 0.f;
#pragma unroll
        for (int u = 0; u < NV; ++u) smv[(4 * tid + j) * NV + u] = f32x4{dz[4 * u], dz[4 * u + 1], dz[4 * u + 2], dz[4 * u + 3]};
      }
    }
    __syncthreads();
    const int tp = (int)(r1 - t0 < BE_TILE ? r1 - t0 : BE_TILE);
    if (owner) {
      const FT* ft = fb + (size_t)t0 * c0;
      for (int q = slot; q < tp; q += 4 * ppi) {
        f32x4 f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int qq = q + j * ppi;
          f[j] = qq < tp ? be_load_feat(ft + (size_t)qq * c0) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int qq = q + j * ppi;
          if (qq < tp) {
            float dz[KP];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
              const f32x4 d = smv[qq * NV + u];
              dz[4 * u] = d[0]; dz[4 * u + 1] = d[1]; dz[4 * u + 2] = d[2]; dz[4 * u + 3] = d[3];
            }
#pragma unroll
            for (int k = 0; k < K1; ++k) acc[k] += dz[k] * f[j];
          }
        }
      }
    }
    __syncthreads();
  }

  if (owner) {
#pragma unroll
    for (int k = 0; k < K1; ++k) smv[tid * K1 + k] = acc[k];
  }
  __syncthreads();
  const int n = K1 * c0;
  float* dst = part + (size_t)blockIdx.x * n;
  for (int o = tid; o < n; o += 256) {
    const int c = o / c0, ch = o - c * c0, u = ch >> 2, i = ch & 3;
    float r = 0.f;
    for (int sl = 0; sl < ppi; ++sl) r += sm[((sl * nu + u) * K1 + c) * 4 + i];
    dst[o] = r;
  }
}

// embed[b][o] = sum over the slabs, in slab order, in double
__global__ __launch_bounds__(256) void badge_reduce_kernel(const float* __restrict__ part, int slabs, int n, int bpi, float* __restrict__ embed) {
  const int b = blockIdx.x / bpi, o = (blockIdx.x % bpi) * 256 + threadIdx.x;
  if (o >= n) return;
  double a = 0.0;
  for (int s = 0; s < slabs; ++s) a += (double)part[((size_t)b * slabs + s) * n + o];
  embed[(size_t)b * n + o] = (float)a;
}

// ---------------------------------------------------------------- launcher
// Slab rule: BE_SLAB_TILES tiles per slab; an image with more than BE_MAX_SLABS such slabs gets BE_MAX_SLABS slabs of whole tiles.
static int be_slabs(int64_t hw, int64_t* per_out) {
  int64_t per = (int64_t)BE_TILE * BE_SLAB_TILES;
  if (ceil_div64(hw, per) > BE_MAX_SLABS) per = ceil_div64(ceil_div64(hw, BE_MAX_SLABS), BE_TILE) * BE_TILE;
  if (per_out) *per_out = per;
  return (int)ceil_div64(hw, per);
}

static int be_mode(const float* logits, int64_t hw, int k1, int64_t sn, int64_t sk, int64_t sp) {
  if ((hw & 3) != 0 || (sn & 3) != 0 || (reinterpret_cast<uintptr_t>(logits) & 15) != 0) return BE_LD_GENERIC;
  if (sk == 1 && sp == k1) return BE_LD_CLAST;
  if (sp == 1 && (sk & 3) == 0) return BE_LD_PLANAR;
  return BE_LD_GENERIC;
}

// floats: pass-one slices [nb][slabs][3 k1 + 1], coefficients [nb][k1][2], pass-two slices [nb][slabs][k1 c0]
static int64_t be_words(int nb, int slabs, int k1, int c0) {
  return (int64_t)nb * slabs * (3 * k1 + 1) + (int64_t)nb * k1 * 2 + (int64_t)nb * slabs * k1 * c0;
}

static bool be_shape_ok(int nb, int64_t hw, int k1, int c0, int dtype) {
  return nb >= 1 && hw >= 1 && hw < ((int64_t)1 << 31) && k1 >= 1 && k1 <= BE_MAXK && c0 >= 4 && c0 <= BE_MAXC && (c0 & 3) == 0 &&
         (dtype == MIA_F32 || dtype == MIA_BF16);
}

extern "C" int mia_badge_embed_workspace(int nb, int64_t hw, int k1, int c0, int dtype, int* slabs_out) {
  if (slabs_out) *slabs_out = 0;
  if (!be_shape_ok(nb, hw, k1, c0, dtype)) return 0;
  const int slabs = be_slabs(hw, nullptr);
  const int64_t words = be_words(nb, slabs, k1, c0);
  if ((int64_t)nb * slabs >= ((int64_t)1 << 31) / 4 || words >= ((int64_t)1 << 31)) return 0;
  if (slabs_out) *slabs_out = slabs;
  return (int)words;
}

extern "C" int mia_badge_embed(const float* logits, const void* feat, int dtype, int nb, int64_t hw, int k1, int c0, int64_t sn, int64_t sk,
                               int64_t sp, float smooth, int do_bg, int squared, float* workspace, float* embed, float* loss,
                               void* stream) {
  MIA_CHECK_ARG(logits && feat && workspace && embed && loss, "mia_badge_embed: null pointer");
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "mia_badge_embed: unknown dtype %d", dtype);
  MIA_CHECK_ARG(nb >= 1 && hw >= 1 && hw < ((int64_t)1 << 31), "mia_badge_embed: bad shape nb=%d hw=%lld", nb, (long long)hw);
  MIA_CHECK_ARG(k1 >= 1 && k1 <= BE_MAXK, "mia_badge_embed: k1=%d not in [1,%d]", k1, BE_MAXK);
  MIA_CHECK_ARG(c0 >= 4 && c0 <= BE_MAXC && (c0 & 3) == 0, "mia_badge_embed: c0=%d is not a multiple of 4 in [4,%d]", c0, BE_MAXC);
  MIA_CHECK_ARG(do_bg || k1 >= 2, "mia_badge_embed: k1=1 without do_bg leaves the Dice term no class");
  MIA_CHECK_ARG(sp >= 1 && sn >= 0 && sk >= 0 && (k1 == 1 || sk >= 1) && (nb == 1 || sn >= 1),
                "mia_badge_embed: bad logit strides (%lld, %lld, %lld)", (long long)sn, (long long)sk, (long long)sp);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(feat) & (dtype == MIA_F32 ? 15 : 7)) == 0 && (reinterpret_cast<uintptr_t>(logits) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "mia_badge_embed: misaligned pointer");
  int slabs = 0;
  MIA_CHECK_ARG(mia_badge_embed_workspace(nb, hw, k1, c0, dtype, &slabs) > 0, "mia_badge_embed: the batch does not fit one call");
  int64_t per;
  be_slabs(hw, &per);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const BeGeom g{sn, sk, sp};
  const int mode = be_mode(logits, hw, k1, sn, sk, sp);
  float* part1 = workspace;
  float* coef = part1 + (size_t)nb * slabs * (3 * k1 + 1);
  float* part2 = coef + (size_t)nb * k1 * 2;
  const dim3 grid((unsigned)(nb * slabs)), blk(256);
  const int sq = squared ? 1 : 0, n = k1 * c0, bpi = ceil_div(n, 256);
  const float* f32 = static_cast<const float*>(feat);
  const bf16_t* b16 = static_cast<const bf16_t*>(feat);
#define BE_CASE(K)                                                                                                                       \
  case K:                                                                                                                                \
    hipLaunchKernelGGL(badge_sums_kernel<K>, grid, blk, 0, st, logits, hw, g, mode, sq, per, slabs, part1);                              \
    hipLaunchKernelGGL(badge_finalize_kernel, dim3((unsigned)nb), dim3(64), 0, st, part1, slabs, k1, hw, smooth, do_bg ? 1 : 0, coef, loss); \
    if (dtype == MIA_F32)                                                                                                                \
      hipLaunchKernelGGL((badge_embed_kernel<K, float>), grid, blk, 0, st, logits, f32, hw, c0, g, mode, sq, per, slabs, coef, part2);   \
    else                                                                                                                                 \
      hipLaunchKernelGGL((badge_embed_kernel<K, bf16_t>), grid, blk, 0, st, logits, b16, hw, c0, g, mode, sq, per, slabs, coef, part2);  \
    break
  switch (k1) {
    BE_CASE(1); BE_CASE(2); BE_CASE(3); BE_CASE(4); BE_CASE(5); BE_CASE(6); BE_CASE(7); BE_CASE(8);
  }
#undef BE_CASE
  hipLaunchKernelGGL(badge_reduce_kernel, dim3((unsigned)(nb * bpi)), blk, 0, st, part2, slabs, n, bpi, embed);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
