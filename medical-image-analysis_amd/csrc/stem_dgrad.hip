// Input gradient of the stem convolution (Cin = 1): d loss / d image of Conv2d(1, C0, 3, padding=1), gfx950.
//
//   dx[n][y][x] = sum_co sum_(a,b) w[co][3a+b] * dy[n][y+1-a][x+1-b][co]          (dy outside the image = 0; fp32 sums, fp32 dx)
//
// The weight gradient and the forward of this layer are in stem.hip; nothing there needed this tensor until somebody asked for the
// gradient of a loss with respect to the IMAGE (virtual adversarial training, saliency maps).  The kernel is a stream: it reads dy
// once (N*H*W*C0 elements, plus the halo below) and writes N*H*W floats.
//   stage 1  per pixel the nine tap sums g[p][t] = sum_co w[co][t] * dy[p][co]: a [pixels x C0] . [C0 x 9 -> 16] product on the matrix
//            cores.  NHWC dy IS the A operand's layout: lane l loads the 16-byte channel unit q = l >> 4 of pixel l & 15 of a 16-pixel
//            strip, per K chunk (bf16: 32 channels on v_mfma_f32_16x16x32_bf16; fp32: 16 channels = four v_mfma_f32_16x16x4_f32,
//            exact fp32 as in stem_fwd_mfma_kernel).  K is zero-padded where C0 is no multiple of the chunk.  The B fragments (the
//            weights, tap = column) are built once per workgroup in LDS; bf16 weights go in as w = hi + lo (two bf16 parts, two MFMAs),
//            so the fp32 parameter keeps 16 significand bits instead of 8.
//   stage 2  dx[q] = sum_t g[q - off_t][t] gathered from an LDS tile of g.  A workgroup owns SD_TR x SD_TC output pixels and recomputes
//            the one-pixel halo of g around them (16 x 64 / (14 x 62) = 1.18 x the reads of dy, most of them L2 hits).
// Every sum has a fixed order and there are no float atomics: bit-identical from run to run.  dx leaves in 4-byte stores.
// Out of scope: forming dy on load from (dz, y, coefficients) as mia_stem_wgrad_fused does.  When the image needs a gradient the
// stem's norm backward takes the unfused route and materialises dy (ops.PlainBlockFn.backward).
#include "common.h"

#define SD_TR 14  // output rows / columns of a tile; the g tile is (SD_TR + 2) x (SD_TC + 2) = 16 rows x four 16-pixel strips
#define SD_TC 62
#define SD_GR (SD_TR + 2)
#define SD_GC (SD_TC + 2)

template <typename T>
__global__ __launch_bounds__(256) void stem_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w /*[C0][9]*/,
                                                         float* __restrict__ dx, int h, int wd, int c0, int tiles_x, int tiles_y) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int KC = BF ? 32 : 16;          // channels per K chunk
  constexpr int EPU = BF ? 8 : 4;           // channels per 16-byte unit
  __shared__ float g[SD_GR * SD_GC * 9];    // g[row][col][tap]
  __shared__ u32x4 wf[16 * 64];             // B fragments: bf16 [chunk][hi | lo][lane], fp32 [chunk][lane]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q = lane >> 4, c16 = lane & 15;
  const int chunks = (c0 + KC - 1) / KC;
  int b = blockIdx.x;
  const int tx = b % tiles_x; b /= tiles_x;
  const int ty = b % tiles_y;
  const int n = b / tiles_y;
  // ---- B fragments: lane (tap = l & 15, q = l >> 4) of chunk kk holds w[KC kk + EPU q + j][tap], zero for taps >= 9 and channels >= C0
  for (int i = tid; i < chunks * 64; i += 256) {
    const int kk = i >> 6, l = i & 63, tap = l & 15, ch0 = KC * kk + EPU * (l >> 4);
    float v[EPU];
#pragma unroll
    for (int j = 0; j < EPU; ++j) v[j] = (tap < 9 && ch0 + j < c0) ? w[(ch0 + j) * 9 + tap] : 0.f;
    if constexpr (BF) {
      u32x4 hi, lo;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bf16_t h0 = f2bf(v[2 * p]), h1 = f2bf(v[2 * p + 1]);
        hi[p] = (unsigned)h0 | (unsigned)h1 << 16;
        lo[p] = pack_bf16x2(v[2 * p] - bf2f(h0), v[2 * p + 1] - bf2f(h1));  // the residual is exact in fp32
      }
      wf[(2 * kk) * 64 + l] = hi;
      wf[(2 * kk + 1) * 64 + l] = lo;
    } else {
      wf[kk * 64 + l] = __builtin_bit_cast(u32x4, f32x4{v[0], v[1], v[2], v[3]});
    }
  }
  __syncthreads();
  const int y0 = ty * SD_TR, x0 = tx * SD_TC;
  const int rows_out = h - y0 < SD_TR ? h - y0 : SD_TR, cols_out = wd - x0 < SD_TC ? wd - x0 : SD_TC;
  // ---- stage 1: an item = one 16-pixel strip of one row of the g tile; rows / strips that stage 2 never reads are skipped
  for (int item = wave; item < SD_GR * 4; item += 4) {
    const int row = item >> 2, strip = item & 3;
    if (row > rows_out + 1 || 16 * strip > cols_out + 1) continue;
    const int yy = y0 - 1 + row, xs = x0 - 1 + 16 * strip, px = xs + c16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)yy < (unsigned)h && xs + 15 >= 0 && xs < wd) {  // (wave-uniform) the strip meets the image
      const bool pok = (unsigned)px < (unsigned)wd;
      const T* src = dy + (((size_t)n * h + yy) * wd + (pok ? px : 0)) * c0 + EPU * q;
      const u32x4 zero = {0u, 0u, 0u, 0u};
      u32x4 nxt = (pok && EPU * q < c0) ? *reinterpret_cast<const u32x4*>(src) : zero;
      for (int kk = 0; kk < chunks; ++kk) {
        const u32x4 a = nxt;
        const int chn = KC * (kk + 1) + EPU * q;  // the next chunk's unit travels behind this chunk's MFMAs
        nxt = (pok && kk + 1 < chunks && chn < c0) ? *reinterpret_cast<const u32x4*>(src + KC * (kk + 1)) : zero;
        if constexpr (BF) {
          const bf16x8 av = __builtin_bit_cast(bf16x8, a);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(bf16x8, wf[(2 * kk) * 64 + lane]), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, __builtin_bit_cast(bf16x8, wf[(2 * kk + 1) * 64 + lane]), acc, 0, 0, 0);
        } else {
          const f32x4 av = __builtin_bit_cast(f32x4, a), wv = __builtin_bit_cast(f32x4, wf[kk * 64 + lane]);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], wv[j], acc, 0, 0, 0);
        }
      }
    }
    // D: this lane holds taps c16 of the strip's pixels 4q .. 4q + 3
    if (c16 < 9) {
#pragma unroll
      for (int r = 0; r < 4; ++r) g[(row * SD_GC + 16 * strip + 4 * q + r) * 9 + c16] = acc[r];
    }
  }
  __syncthreads();
  // ---- stage 2: output (oy, ox) sits at g-tile (oy + 1, ox + 1); tap (a, b) comes from the pixel at (+1 - a, +1 - b)
  float* out = dx + ((size_t)n * h + y0) * wd + x0;
  for (int o = tid; o < rows_out * cols_out; o += 256) {
    const int oy = o / cols_out, ox = o - oy * cols_out;
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bb = 0; bb < 3; ++bb) s += g[((oy + 2 - a) * SD_GC + ox + 2 - bb) * 9 + 3 * a + bb];
    out[(size_t)oy * wd + ox] = s;
  }
}

extern "C" int mia_stem_dgrad(const void* dy, int dtype, const float* w, float* dx, int n, int h, int wd, int c0, void* stream) {
  MIA_CHECK_ARG(dy && w && dx && n > 0 && h > 0 && wd > 0 && c0 > 0, "mia_stem_dgrad: bad arguments (n=%d h=%d w=%d c0=%d)", n, h, wd, c0);
  MIA_CHECK_ARG(dtype == MIA_BF16 || dtype == MIA_F32, "mia_stem_dgrad: bad dtype");
  MIA_CHECK_ARG(c0 % (dtype == MIA_BF16 ? 8 : 4) == 0 && c0 <= 256, "mia_stem_dgrad: c0=%d must be a multiple of the 16-byte unit and <= 256", c0);
  MIA_CHECK_ARG((int64_t)h * wd < ((int64_t)1 << 31), "mia_stem_dgrad: image too large");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(dy) & 15) == 0 && (reinterpret_cast<uintptr_t>(dx) & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 3) == 0,
                "mia_stem_dgrad: dy must be 16-byte aligned, w and dx 4-byte aligned");
  const int tiles_x = ceil_div(wd, SD_TC), tiles_y = ceil_div(h, SD_TR);
  const int64_t blocks = (int64_t)n * tiles_x * tiles_y;
  MIA_CHECK_ARG(blocks <= 0x7fffffffLL, "mia_stem_dgrad: %lld tiles are more than one launch holds", (long long)blocks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == MIA_BF16)
    hipLaunchKernelGGL(stem_dgrad_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const bf16_t*>(dy), w, dx, h, wd, c0,
                       tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(stem_dgrad_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, static_cast<const float*>(dy), w, dx, h, wd, c0,
                       tiles_x, tiles_y);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
