// UniMatch's feature-perturbation stream (Yang et al., CVPR 2023) on an encoder output x [n][hw][c] (NHWC, fp32 or bf16): the decoder
// reads cat(x, Dropout2d(x[row0 : row0 + nu])) along the batch axis.  ONE streaming pass each way (definition: include/mia_hip.h):
//   forward   out[i] = x[i];  out[n + u] = m[u][ch] == 0 ? +0 : rnd(x[row0 + u] * m[u][ch])        reads n rows, writes n + nu
//   backward  dx[i] = dy[i], or rnd(dy[i] + rnd(dy[n + u] * m[u][ch])) where i = row0 + u and m != 0  reads n + nu rows, writes n
// A block owns TILES of whole pixels of one image (FD_TILE accesses, or one pixel when a pixel has more): inside a tile an access index
// is a 32-bit number, its channel unit is `index % units-per-pixel` (a mask when that is a power of two), and nothing per access needs
// a 64-bit division.  The grid is capped at FD_MAX_BLOCKS; a block strides over the tiles and carries (image, tile of the image)
// along by the grid's quotient and remainder, so the loop has no division either.  An access is 16 bytes (4 fp32 / 8 bf16 channels
// of one pixel; mask values as aligned float4 loads of a table that stays in L2) or, on the fallback, one element.
#include "common.h"

namespace {

constexpr int FD_THREADS = 256;
constexpr int FD_TILE = 512;         // accesses per tile: two per thread
constexpr int FD_MAX_BLOCKS = 2048;  // 256 CUs x 8 blocks of 256 threads

struct FdGeom {
  int64_t hw, tpi, tiles;        // pixels per image, tiles per image, tiles in all
  int n, row0, nu, c;
  int upp, ppt, pow2;            // accesses per pixel, pixels per tile, upp is a power of two
  int gq, gr;                    // gridDim.x / tpi, gridDim.x % tpi
};

// rounding to the storage type and back: the identity for fp32, round-to-nearest-even for bf16
template <typename T> __device__ __forceinline__ float fd_rnd(float v) {
  if constexpr (sizeof(T) == 4) return v; else return bf2f(f2bf(v));
}

// One perturbed value.  A dropped channel is a selection: whatever x holds, the result is +0.
template <typename T> __device__ __forceinline__ T fd_fwd(T x, float m) {
  const float p = Elem<T>::ld(&x) * m;
  return m == 0.f ? Elem<T>::cvt(0.f) : Elem<T>::cvt(p);
}

// One gradient value of a perturbed row: the bits of the tensor-op form under autograd, which multiplies in one kernel (and, for bf16,
// rounds the product to bf16 when the gradient of the cast leaves fp32) and adds in another.  The product and the sum are rounded
// separately: without the pragma both `a + b * m` and __fadd_rn(a, __fmul_rn(b, m)) compile to one v_fmac_f32.
template <typename T> __device__ __forceinline__ T fd_bwd(T a, T b, float m) {
#pragma clang fp contract(off)
  const float t = fd_rnd<T>(Elem<T>::ld(&b) * m);
  const float r = Elem<T>::ld(&a) + t;
  return m == 0.f ? a : Elem<T>::cvt(r);
}

template <typename T, int W> __device__ __forceinline__ void fd_fold(unsigned& am, const T (&v)[W], const unsigned* amax) {
  if constexpr (sizeof(T) == 4) {
    if (amax == nullptr) return;
#pragma unroll
    for (int e = 0; e < W; ++e) { const unsigned b = __builtin_bit_cast(unsigned, v[e]) & 0x7FFFFFFFu; am = b > am ? b : am; }
  }
}

// lanes -> wave -> block (LDS) -> one conditional atomic per block (amax_publish of norm.hip).  Integer maximum of the bit patterns
// of |v|: exact, independent of the order, and a NaN counts as mia_amax counts it (above every finite value and inf).
__device__ __forceinline__ void fd_publish(unsigned m, unsigned* __restrict__ slot) {
  __shared__ unsigned blk;
  if (threadIdx.x == 0) blk = 0u;
  __syncthreads();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = (unsigned)__shfl_xor((int)m, o, 64); m = t > m ? t : m; }
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(&blk, m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned b = blk;
    if (b > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, b);
  }
}

// W = elements per access: Elem<T>::EPU (16 bytes) or 1.  BWD = false: src = x, dst = out; true: src = dy, dst = dx.
template <typename T, int W, bool BWD>
__global__ __launch_bounds__(FD_THREADS) void feat_drop_cat_kernel(const T* __restrict__ src, const float* __restrict__ mask,
                                                                    T* __restrict__ dst, const FdGeom g, unsigned* __restrict__ amax) {
  struct alignas(sizeof(T) * W) Unit { T v[W]; };
  auto ld = [](const T* p) -> Unit { return *reinterpret_cast<const Unit*>(p); };
  auto st = [](T* p, const Unit& u) {
    if (W > 1) store_data_fence();
    *reinterpret_cast<Unit*>(p) = u;
    if (W > 1) store_data_pad();
  };
  int64_t t = blockIdx.x;
  int64_t img = t / g.tpi, ti = t - img * g.tpi;  // the block's only 64-bit division
  unsigned am = 0u;
  for (; t < g.tiles; t += gridDim.x) {
    const int64_t p0 = ti * g.ppt;
    const int np = (int)(g.hw - p0 < g.ppt ? g.hw - p0 : g.ppt);
    const int nv = np * g.upp;  // <= max(FD_TILE, upp)
    const int u = (int)img - g.row0;
    const bool pert = (unsigned)u < (unsigned)g.nu;  // the whole tile belongs to one image
    const int64_t base = (img * g.hw + p0) * g.c;
    const int64_t twin = (((int64_t)g.n + (pert ? u : 0)) * g.hw + p0) * g.c;
    const float* __restrict__ mrow = mask + (int64_t)(pert ? u : 0) * g.c;
    auto mvals = [&](int l, float (&m)[W]) {
      const int cu = g.pow2 ? (l & (g.upp - 1)) : (l % g.upp);
      if constexpr (W == 1) {
        m[0] = mrow[cu];
      } else {
#pragma unroll
        for (int q = 0; q < W / 4; ++q) {
          const f32x4 f = *reinterpret_cast<const f32x4*>(mrow + (int64_t)cu * W + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) m[4 * q + e] = f[e];
        }
      }
    };
    auto body = [&](int l, const Unit& a, const Unit& b) {
      const int64_t off = (int64_t)l * W;
      if constexpr (!BWD) {
        fd_fold<T, W>(am, a.v, amax);
        st(dst + base + off, a);
        if (pert) {
          float m[W];
          mvals(l, m);
          Unit o;
#pragma unroll
          for (int e = 0; e < W; ++e) o.v[e] = fd_fwd<T>(a.v[e], m[e]);
          fd_fold<T, W>(am, o.v, amax);
          st(dst + twin + off, o);
        }
      } else {
        Unit o = a;
        if (pert) {
          float m[W];
          mvals(l, m);
#pragma unroll
          for (int e = 0; e < W; ++e) o.v[e] = fd_bwd<T>(a.v[e], b.v[e], m[e]);
        }
        fd_fold<T, W>(am, o.v, amax);
        st(dst + base + off, o);
      }
    };
    const bool two = BWD && pert;  // the backward of a perturbed row reads its twin's gradient as well
    int l = threadIdx.x;
    for (; l + FD_THREADS < nv; l += 2 * FD_THREADS) {  // two independent accesses (four in the backward of a perturbed row) in flight
      const int l1 = l + FD_THREADS;
      const Unit a0 = ld(src + base + (int64_t)l * W), a1 = ld(src + base + (int64_t)l1 * W);
      const Unit b0 = two ? ld(src + twin + (int64_t)l * W) : a0, b1 = two ? ld(src + twin + (int64_t)l1 * W) : a1;
      body(l, a0, b0);
      body(l1, a1, b1);
    }
    for (; l < nv; l += FD_THREADS) {
      const Unit a0 = ld(src + base + (int64_t)l * W);
      const Unit b0 = two ? ld(src + twin + (int64_t)l * W) : a0;
      body(l, a0, b0);
    }
    img += g.gq;
    ti += g.gr;
    if (ti >= g.tpi) { ti -= g.tpi; ++img; }
  }
  if constexpr (sizeof(T) == 4) { if (amax != nullptr) fd_publish(am, amax); }  // (every thread of the block arrives here)
}

bool fd_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T, bool BWD>
void fd_launch(const void* src, const float* mask, void* dst, int n, int64_t hw, int c, int row0, int nu, void* amax, bool wide,
               hipStream_t st) {
  constexpr int EPU = Elem<T>::EPU;
  FdGeom g;
  g.hw = hw; g.n = n; g.row0 = row0; g.nu = nu; g.c = c;
  g.upp = wide ? c / EPU : c;
  g.ppt = g.upp >= FD_TILE ? 1 : FD_TILE / g.upp;
  g.pow2 = (g.upp & (g.upp - 1)) == 0;
  g.tpi = ceil_div64(hw, g.ppt);
  g.tiles = g.tpi * n;
  const int grid = (int)(g.tiles < FD_MAX_BLOCKS ? g.tiles : FD_MAX_BLOCKS);
  g.gq = (int)(grid / g.tpi);
  g.gr = (int)(grid % g.tpi);
  unsigned* am = sizeof(T) == 4 ? static_cast<unsigned*>(amax) : nullptr;  // the maximum serves fp32 consumers only
  if (wide)
    hipLaunchKernelGGL((feat_drop_cat_kernel<T, EPU, BWD>), dim3(grid), dim3(FD_THREADS), 0, st, static_cast<const T*>(src), mask,
                       static_cast<T*>(dst), g, am);
  else
    hipLaunchKernelGGL((feat_drop_cat_kernel<T, 1, BWD>), dim3(grid), dim3(FD_THREADS), 0, st, static_cast<const T*>(src), mask,
                       static_cast<T*>(dst), g, am);
}

// src / dst: (x [n], out [n + nu]) of the forward, (dy [n + nu], dx [n]) of the backward
template <bool BWD>
int fd_run(const char* who, int dtype, const void* src, const float* mask, void* dst, int n, int64_t hw, int c, int row0, int nu,
           void* amax_out, void* stream) {
  MIA_CHECK_ARG(src && mask && dst, "%s: null pointer", who);
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "%s: bad dtype %d", who, dtype);
  MIA_CHECK_ARG(nu >= 1 && row0 >= 0 && (int64_t)row0 + nu <= n, "%s: rows [%d, %d + %d) outside the %d images", who, row0, row0, nu, n);
  MIA_CHECK_ARG(c >= 1 && hw >= 1, "%s: bad shape hw=%lld c=%d", who, (long long)hw, c);
  const int es = dtype == MIA_F32 ? 4 : 2;
  MIA_CHECK_ARG(hw <= INT64_MAX / es / c / ((int64_t)n + nu), "%s: n=%d nu=%d hw=%lld c=%d overflows 64-bit byte offsets", who, n, nu,
                (long long)hw, c);
  const int64_t row = hw * c * es;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t s1 = s0 + (uintptr_t)(row * (BWD ? (int64_t)n + nu : n)), d1 = d0 + (uintptr_t)(row * (BWD ? n : (int64_t)n + nu));
  MIA_CHECK_ARG(d1 <= s0 || s1 <= d0, "%s: %s overlaps %s", who, BWD ? "dx" : "out", BWD ? "dy" : "x");
  MIA_CHECK_ARG((s0 | d0) % es == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0 && (reinterpret_cast<uintptr_t>(amax_out) & 3) == 0,
                "%s: misaligned pointer", who);
  const bool wide = (int64_t)c * es % 16 == 0 && fd_al16(src) && fd_al16(dst) && fd_al16(mask);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MIA_F32) fd_launch<float, BWD>(src, mask, dst, n, hw, c, row0, nu, amax_out, wide, st);
  else fd_launch<bf16_t, BWD>(src, mask, dst, n, hw, c, row0, nu, nullptr, wide, st);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

}  // namespace

extern "C" int mia_feat_drop_cat_fwd(int dtype, const void* x, const float* mask, void* out, int n, int64_t hw, int c, int row0, int nu,
                                     void* amax_out, void* stream) {
  return fd_run<false>("mia_feat_drop_cat_fwd", dtype, x, mask, out, n, hw, c, row0, nu, amax_out, stream);
}

extern "C" int mia_feat_drop_cat_bwd(int dtype, const void* dy, const float* mask, void* dx, int n, int64_t hw, int c, int row0, int nu,
                                     void* amax_out, void* stream) {
  return fd_run<true>("mia_feat_drop_cat_bwd", dtype, dy, mask, dx, n, hw, c, row0, nu, amax_out, stream);
}

// The tile count one sweep of the capped grid covers (tests size their grid-stride cases from it).
extern "C" int mia_feat_drop_cat_sweep(int dtype, int c, int wide, int* tile_pixels) {
  MIA_CHECK_ARG((dtype == MIA_F32 || dtype == MIA_BF16) && c >= 1 && tile_pixels, "mia_feat_drop_cat_sweep: bad arguments");
  const int upp = wide ? c / (dtype == MIA_F32 ? 4 : 8) : c;
  MIA_CHECK_ARG(upp >= 1, "mia_feat_drop_cat_sweep: c=%d has no 16-byte unit", c);
  *tile_pixels = upp >= FD_TILE ? 1 : FD_TILE / upp;
  return FD_MAX_BLOCKS;
}
