// The exact 1-D lower-envelope step of the separable squared Euclidean distance transform, shared by surface.hip (surface
// metrics) and boundary.hip (signed distance maps): ONE definition, so the two files evaluate the same fp32 expressions.
#pragma once
#include "common.h"

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

// The same minimum for a dense line (stride 1), four steps of the outward scan per early-exit test: eight independent reads in
// flight instead of two behind every test.  Every term a step adds beyond line_min's is >= (s r)^2 >= best, and
// dr + min(a, b) = min(dr + a, dr + b) in fp32 (rounding is monotone), so the result has line_min's bits.
__device__ __forceinline__ float line_min_x4(const float* f, int n, int i, float s) {
  const float inf = __builtin_inff();
  float best = f[i];
  for (int r = 1;; r += 4) {
    if (sq_dist(s, r) >= best) break;
    if (i - r < 0 && i + r >= n) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int lo = i - r - k, hi = i + r + k;
      const float a = lo >= 0 ? f[lo] : inf, b = hi < n ? f[hi] : inf;
      best = fminf(best, sq_dist(s, r + k) + fminf(a, b));
    }
  }
  return best;
}
