// Connected components of int64 label maps on the GPU (gfx950), 2-D and 3-D, and the clean-up built on them: "remove all but the
// largest component" / "remove components below a size", per class or for the whole foreground.  The reference only approximates
// this step: `UnetProcessor.remove_cc` (models/unet/unet_processor.py:121-125) is a morphological opening inside `denoise_one_mask`
// (:72-113), which cannot remove a blob larger than its structuring element.
//
// Definition.  Two voxels are joined when they are neighbours (connectivity 1: faces; connectivity ndim: faces, edges and corners)
// and hold the same label in [1, n_classes) -- with `foreground`, when both hold some label in that range.  A component's root is the
// smallest linear index, within its image, of its voxels; the labelling is root + 1 on component voxels and 0 elsewhere.  That map
// is a function of the input alone, so whatever order the atomics land in, the bits are the same.
//
// Launches (every launch boundary is a visibility point; inside the merge launch `parent` is only touched by agent-scope atomics):
//   cc_init_kernel     zeroes the status word and the winners (no memset node)
//   cc_tile_kernel     a workgroup labels one in-slice CC_TH x CC_TW tile in LDS by union-find (atomicMin on LDS) and writes every
//                      voxel's tile-local root as (linear index in the image) + 1 into `parent`; 0 = no component.  Zeroes `size`.
//   cc_merge_kernel    one thread per voxel: unites it with those of its raster-order predecessors that lie in another tile or in the
//                      previous slice -- union(find(a), find(b)) by fetch_min on `parent`
//   cc_flatten_kernel  parent[x] = find(x) + 1 (now the labelling itself); with `size`, exact counts by fetch_add at the root's slot,
//                      folded per wave and per block first
//   cc_winner_kernel   roots only: 64-bit fetch_max of (size << 32) | ~root per (image, class) -- largest size, ties to the lowest root
//   cc_filter_kernel   out = fill where the component is below min_size or (keep_largest and) not the winner, else the input
//
// parent[x] <= x + 1 always and every hop of a find strictly decreases, so every loop ends by construction.  After cc_tile_kernel a
// voxel points at a tile root and only tile roots are ever re-linked, so the longest legal chain is one hop plus one per tile root
// of the image: at most (voxels of the image) + 1 hops, the cap every loop carries.  A hop that does not decrease, or a loop that
// reaches the cap, can only come from a wrong kernel: the thread sets the status word and leaves at once.
#include "common.h"

#define CC_TH 16
#define CC_TW 64
#define CC_TILE (CC_TH * CC_TW)
#define CC_THREADS 256
#define CC_FLAT_PASSES 8  // voxels per thread of the flatten pass
#define CC_MAX_CLASSES 256

#define CC_STATUS_CAP 1       // a find / union loop reached its iteration cap
#define CC_STATUS_ORDER 2     // a hop did not decrease (parent[x] > x + 1)

namespace {

struct CcGeom {
  int nimg, d, h, w;   // images (ndim 2: every slice), slices per image, rows, columns
  int vox;             // d * h * w
  int full;            // connectivity: 0 = faces, 1 = faces + edges + corners
  int n_classes, foreground;
  int ty, tx;          // tiles per slice
};

// 0 = belongs to no component; else the value two joined neighbours share
__device__ __forceinline__ int cc_key(long long v, int n_classes, int foreground) {
  if (v < 1 || v >= (long long)n_classes) return 0;
  return foreground ? 1 : (int)v;
}

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ void cc_flag(int* status, int bit) { __hip_atomic_fetch_or(status, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x (linear index; parent holds index + 1) or -1 after flagging `status`.
__device__ __forceinline__ int cc_find(const int* parent, int x, unsigned cap, int* status) {
  for (unsigned it = 0; it <= cap; ++it) {
    const int p = ld_agent(parent + x) - 1;
    if (p == x) return x;
    if (p > x || p < 0) { cc_flag(status, CC_STATUS_ORDER); return -1; }
    x = p;
  }
  cc_flag(status, CC_STATUS_CAP);
  return -1;
}

// Unite the sets of a and b: the larger root is linked under the smaller one.  fetch_min returns what the slot held: if that is
// still the root itself the link is made, otherwise somebody lowered it meanwhile and the walk goes on from there (strictly lower).
__device__ __forceinline__ void cc_union(int* parent, int a, int b, unsigned cap, int* status) {
  for (unsigned it = 0; it <= cap; ++it) {
    a = cc_find(parent, a, cap, status);
    b = cc_find(parent, b, cap, status);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(parent + a, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (old == a) return;
    a = old;
  }
  cc_flag(status, CC_STATUS_CAP);
}

__global__ void cc_init_kernel(int* status, unsigned long long* winner, int nwin) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *status = 0;
  if (i < nwin) winner[i] = 0ull;
}

// ---- (a) one tile in LDS
__device__ __forceinline__ int lds_find(int* par, int x, int* status) {
  for (int it = 0; it <= CC_TILE; ++it) {
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == x) return x;
    if (p > x || p < 0) { cc_flag(status, CC_STATUS_ORDER); return -1; }
    x = p;
  }
  cc_flag(status, CC_STATUS_CAP);
  return -1;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b, int* status) {
  for (int it = 0; it <= CC_TILE; ++it) {
    a = lds_find(par, a, status);
    b = lds_find(par, b, status);
    if (a < 0 || b < 0 || a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == a) return;
    a = old;
  }
  cc_flag(status, CC_STATUS_CAP);
}

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const long long* __restrict__ labels, int* __restrict__ parent,
                                                             int* __restrict__ size, CcGeom g, int* status) {
  __shared__ int skey[CC_TILE];
  __shared__ int spar[CC_TILE];
  int b = blockIdx.x;
  const int bx = b % g.tx; b /= g.tx;
  const int by = b % g.ty; b /= g.ty;
  const int z = b % g.d;
  const int img = b / g.d;
  const int y0 = by * CC_TH, x0 = bx * CC_TW;
  const int64_t base = (int64_t)img * g.vox;
  const int zoff = z * (g.h * g.w);  // < vox < 2^31
  const int lx = threadIdx.x & (CC_TW - 1), ly0 = threadIdx.x / CC_TW;
  constexpr int ROWS_PER_PASS = CC_THREADS / CC_TW, PASSES = CC_TH / ROWS_PER_PASS;
  const bool xin = x0 + lx < g.w;
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ly = ly0 + k * ROWS_PER_PASS, i = ly * CC_TW + lx;
    int key = 0;
    if (xin && y0 + ly < g.h) key = cc_key(labels[base + zoff + (y0 + ly) * g.w + x0 + lx], g.n_classes, g.foreground);
    skey[i] = key;
    spar[i] = i;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ly = ly0 + k * ROWS_PER_PASS, i = ly * CC_TW + lx;
    const int key = skey[i];
    if (!key) continue;
    if (lx > 0 && skey[i - 1] == key) lds_union(spar, i, i - 1, status);
    if (ly > 0) {
      if (skey[i - CC_TW] == key) {
        lds_union(spar, i, i - CC_TW, status);  // its row neighbours of the same key are joined to it by their own left test
      } else if (g.full) {
        if (lx > 0 && skey[i - CC_TW - 1] == key) lds_union(spar, i, i - CC_TW - 1, status);
        if (lx < CC_TW - 1 && skey[i - CC_TW + 1] == key) lds_union(spar, i, i - CC_TW + 1, status);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PASSES; ++k) {
    const int ly = ly0 + k * ROWS_PER_PASS, i = ly * CC_TW + lx;
    if (!(xin && y0 + ly < g.h)) continue;
    int out = 0;
    if (skey[i]) {
      const int r = lds_find(spar, i, status);
      // the local order (row, column) is the image's raster order, so the smallest local index is the smallest linear index
      out = r < 0 ? 0 : zoff + (y0 + r / CC_TW) * g.w + x0 + (r & (CC_TW - 1)) + 1;
    }
    const int64_t o = base + zoff + (y0 + ly) * g.w + x0 + lx;
    parent[o] = out;
    if (size) size[o] = 0;
  }
}

// ---- (b) unions across tile borders and slices
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const long long* __restrict__ labels, int* parent, CcGeom g, unsigned cap,
                                                              int* status) {
  const int64_t gi = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (gi >= (int64_t)g.nimg * g.vox) return;
  const int i = (int)(gi % g.vox);
  const int64_t base = gi - i;
  const int hw = g.h * g.w;
  const int z = i / hw, r = i - z * hw, y = r / g.w, x = r - y * g.w;
  const bool top = (y % CC_TH) == 0 && y > 0, left = (x % CC_TW) == 0 && x > 0, right = (x % CC_TW) == CC_TW - 1 && x + 1 < g.w;
  if (z == 0 && !top && !left && !(g.full && right && y > 0)) return;  // every predecessor lies in this voxel's own tile
  const long long* lab = labels + base;
  int* par = parent + base;
  const int key = cc_key(lab[i], g.n_classes, g.foreground);
  if (!key) return;
  auto same = [&](int j) { return cc_key(lab[j], g.n_classes, g.foreground) == key; };
  // in the slice: left, up-left, up, up-right -- those that the tile pass could not see
  if (left && same(i - 1)) cc_union(par, i, i - 1, cap, status);
  if (y > 0) {
    if (top && same(i - g.w)) cc_union(par, i, i - g.w, cap, status);
    if (g.full) {
      if (x > 0 && (top || left) && same(i - g.w - 1)) cc_union(par, i, i - g.w - 1, cap, status);
      if (x + 1 < g.w && (top || right) && same(i - g.w + 1)) cc_union(par, i, i - g.w + 1, cap, status);
    }
  }
  // the previous slice: 1 or 9 neighbours.  Where the one straight below matches, the others that match are its own in-slice
  // neighbours of the same key and get joined to it there, so the one union is enough.
  if (z > 0) {
    const int c = i - hw;
    if (same(c)) {
      cc_union(par, i, c, cap, status);
    } else if (g.full) {
      for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= g.h) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dy == 0 && dx == 0) || x + dx < 0 || x + dx >= g.w) continue;
          const int j = c + dy * g.w + dx;
          if (same(j)) cc_union(par, i, j, cap, status);
        }
      }
    }
  }
}

// ---- (c) + (d) final roots, and exact sizes at the root's slot
// A block walks CC_FLAT_PASSES x CC_THREADS consecutive voxels.  Sizes: lanes are consecutive voxels, so a wave first folds every
// run of lanes with the same (image, root) into one add; the first such slot a block meets becomes the block's own, counted in LDS
// and added once at the end -- a component that fills whole blocks costs one global atomic per block, not one per wave and pass.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* parent, int* size, CcGeom g, unsigned cap, int* status) {
  __shared__ unsigned long long s_slot;  // ~0 = none yet
  __shared__ int s_cnt;
  const int64_t total = (int64_t)g.nimg * g.vox;
  const int lane = threadIdx.x & 63;
  if (size) {  // uniform over the launch
    if (threadIdx.x == 0) { s_slot = ~0ull; s_cnt = 0; }
    __syncthreads();
  }
  for (int k = 0; k < CC_FLAT_PASSES; ++k) {
    const int64_t gi = ((int64_t)blockIdx.x * CC_FLAT_PASSES + k) * CC_THREADS + threadIdx.x;
    int root = -1;
    int64_t base = 0;
    if (gi < total) {
      const int i = (int)(gi % g.vox);
      base = gi - i;
      if (ld_agent(parent + gi) != 0) {
        root = cc_find(parent + base, i, cap, status);
        // other threads may still walk through this slot: the new value is an ancestor too, and smaller
        __hip_atomic_store(parent + gi, root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // a flagged find leaves 0
      }
    }
    if (!size) continue;
    const int64_t slot = root < 0 ? -1 : base + root;
    const int64_t prev = __shfl_up(slot, 1, 64);
    const bool head = lane == 0 || prev != slot;
    const unsigned long long heads = __ballot(head);
    if (head && slot >= 0) {
      const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
      const int run = after ? __builtin_ctzll(after) + 1 : 64 - lane;
      unsigned long long own = __hip_atomic_load(&s_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (own == ~0ull) {
        own = atomicCAS(&s_slot, ~0ull, (unsigned long long)slot);
        if (own == ~0ull) own = (unsigned long long)slot;
      }
      if (own == (unsigned long long)slot) atomicAdd(&s_cnt, run);
      else __hip_atomic_fetch_add(size + slot, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!size) return;
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt > 0) __hip_atomic_fetch_add(size + s_slot, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- (e) the largest component per (image, class), ties to the lowest root
__global__ __launch_bounds__(CC_THREADS) void cc_winner_kernel(const long long* __restrict__ labels, const int* __restrict__ parent,
                                                               const int* __restrict__ size, CcGeom g, unsigned long long* winner) {
  const int64_t gi = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (gi >= (int64_t)g.nimg * g.vox) return;
  const int i = (int)(gi % g.vox);
  if (parent[gi] != i + 1) return;  // roots only
  const int cls = g.foreground ? 0 : (int)labels[gi];
  const unsigned long long v = ((unsigned long long)(unsigned)size[gi] << 32) | (unsigned)~(unsigned)i;
  unsigned long long* slot = winner + (gi / g.vox) * g.n_classes + cls;
  // the slot only grows, so a value already above v makes the atomic pointless: the many small components of one volume then do not
  // queue up at a single address behind the large one
  if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)
    __hip_atomic_fetch_max(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct CcClassMask {
  unsigned bits[CC_MAX_CLASSES / 32];
};

// ---- (f)
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const long long* __restrict__ labels, long long* __restrict__ out,
                                                               const int* __restrict__ parent, const int* __restrict__ size,
                                                               const unsigned long long* __restrict__ winner, CcGeom g, CcClassMask cm,
                                                               int keep_largest, int min_size, long long fill) {
  const int64_t gi = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (gi >= (int64_t)g.nimg * g.vox) return;
  const long long v = labels[gi];
  long long o = v;
  const int p = parent[gi];
  if (p != 0 && (g.foreground || ((cm.bits[(int)v >> 5] >> ((int)v & 31)) & 1u))) {  // p != 0: v is in [1, n_classes)
    const int64_t img = gi / g.vox;
    const int root = p - 1;
    const int sz = size[img * g.vox + root];
    const unsigned long long win = winner[img * g.n_classes + (g.foreground ? 0 : (int)v)];
    if (sz < min_size || (keep_largest && root != (int)~(unsigned)win)) o = fill;
  }
  out[gi] = o;
}

struct CcPlan {
  CcGeom g;
  int64_t total;     // voxels of all images
  int64_t tiles;     // workgroups of the tile pass
  int64_t nwin;      // winners
  int64_t words;     // workspace of mia_cc_filter in 4-byte words: parent | size | winners (8-byte aligned)
};

bool cc_plan(int nvol, int ndim, int d, int h, int w, int n_classes, CcPlan& p) {
  if (nvol < 1 || d < 1 || h < 1 || w < 1 || (ndim != 2 && ndim != 3)) return false;
  if (n_classes < 1 || n_classes > CC_MAX_CLASSES) return false;
  const int64_t nimg = ndim == 2 ? (int64_t)nvol * d : nvol;
  const int dd = ndim == 2 ? 1 : d;
  const int64_t vox = (int64_t)dd * h * w;
  if (vox > 0x7ffffffeLL || nimg > 0x7fffffffLL) return false;
  CcGeom& g = p.g;
  g.nimg = (int)nimg; g.d = dd; g.h = h; g.w = w; g.vox = (int)vox;
  g.full = 0; g.n_classes = n_classes; g.foreground = 0;
  g.ty = ceil_div(h, CC_TH); g.tx = ceil_div(w, CC_TW);
  p.total = nimg * vox;
  p.tiles = nimg * dd * g.ty * g.tx;
  p.nwin = nimg * n_classes;
  p.words = 2 * ((p.total + 1) / 2 * 2) + 2 * p.nwin;
  return p.tiles <= 0x7fffffffLL && ceil_div64(p.total, CC_THREADS) <= 0x7fffffffLL;
}

int cc_check(const char* who, int ndim, int connectivity, int foreground, CcPlan& p, bool planned, int nvol, int d, int h, int w, int n_classes) {
  MIA_CHECK_ARG(ndim == 2 || ndim == 3, "%s: ndim=%d not 2 or 3", who, ndim);
  MIA_CHECK_ARG(connectivity == 1 || connectivity == ndim, "%s: connectivity=%d not 1 or ndim (%d)", who, connectivity, ndim);
  MIA_CHECK_ARG(planned, "%s: extents nvol=%d d=%d h=%d w=%d n_classes=%d outside the limits (all >= 1, voxels per image < 2^31 - 1, "
                "n_classes <= %d)", who, nvol, d, h, w, n_classes, CC_MAX_CLASSES);
  p.g.full = connectivity > 1;
  p.g.foreground = foreground != 0;
  return MIA_OK;
}

// (init,) tile, merge, flatten
void cc_label_launches(const long long* labels, int* parent, int* size, unsigned long long* winner, const CcPlan& p, int* status,
                       hipStream_t st) {
  const CcGeom& g = p.g;
  const int nwin = winner ? (int)p.nwin : 0;
  const unsigned cap = (unsigned)g.vox + 1u;
  const unsigned blocks = (unsigned)ceil_div64(p.total, CC_THREADS);
  hipLaunchKernelGGL(cc_init_kernel, dim3((unsigned)ceil_div(nwin + 1, 256)), dim3(256), 0, st, status, winner, nwin);
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)p.tiles), dim3(CC_THREADS), 0, st, labels, parent, size, g, status);
  if (p.tiles > g.nimg) hipLaunchKernelGGL(cc_merge_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, labels, parent, g, cap, status);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)ceil_div64(p.total, CC_THREADS * CC_FLAT_PASSES)), dim3(CC_THREADS), 0, st, parent, size,
                     g, cap, status);
}

}  // namespace

extern "C" int mia_cc_workspace(int nvol, int ndim, int d, int h, int w, int n_classes) {
  CcPlan p;
  if (!cc_plan(nvol, ndim, d, h, w, n_classes, p) || p.words > 0x7fffffffLL) return -1;
  return (int)p.words;
}

extern "C" int mia_cc_label(const long long* labels, int* roots, int nvol, int ndim, int d, int h, int w, int connectivity, int n_classes,
                            int foreground, int* status, void* stream) {
  MIA_CHECK_ARG(labels && roots && status, "mia_cc_label: null pointer");
  CcPlan p;
  const bool ok = cc_plan(nvol, ndim, d, h, w, n_classes, p);
  const int rc = cc_check("mia_cc_label", ndim, connectivity, foreground, p, ok, nvol, d, h, w, n_classes);
  if (rc != MIA_OK) return rc;
  cc_label_launches(labels, roots, nullptr, nullptr, p, status, static_cast<hipStream_t>(stream));
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}

extern "C" int mia_cc_filter(const long long* labels, long long* out, int nvol, int ndim, int d, int h, int w, int connectivity,
                             int n_classes, int foreground, int keep_largest, int min_size, const unsigned char* class_mask,
                             int64_t fill, float* workspace, int* status, void* stream) {
  MIA_CHECK_ARG(labels && out && workspace && status, "mia_cc_filter: null pointer");
  MIA_CHECK_ARG(labels != out, "mia_cc_filter: in place is not supported");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mia_cc_filter: the workspace must be 8-byte aligned");
  MIA_CHECK_ARG(min_size >= 0, "mia_cc_filter: min_size=%d is negative", min_size);
  CcPlan p;
  const bool ok = cc_plan(nvol, ndim, d, h, w, n_classes, p) && p.words <= 0x7fffffffLL;
  const int rc = cc_check("mia_cc_filter", ndim, connectivity, foreground, p, ok, nvol, d, h, w, n_classes);
  if (rc != MIA_OK) return rc;
  CcClassMask cm;
  for (unsigned& b : cm.bits) b = 0;
  for (int c = 1; c < n_classes; ++c)
    if (!class_mask || class_mask[c]) cm.bits[c >> 5] |= 1u << (c & 31);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t n2 = (p.total + 1) / 2 * 2;
  int* parent = reinterpret_cast<int*>(workspace);
  int* size = parent + n2;
  unsigned long long* winner = reinterpret_cast<unsigned long long*>(size + n2);
  cc_label_launches(labels, parent, size, winner, p, status, st);
  const unsigned blocks = (unsigned)ceil_div64(p.total, CC_THREADS);
  if (keep_largest) hipLaunchKernelGGL(cc_winner_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, labels, parent, size, p.g, winner);
  hipLaunchKernelGGL(cc_filter_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, labels, out, parent, size, winner, p.g, cm,
                     keep_largest != 0, min_size, fill);
  MIA_LAUNCH_CHECK();
  return MIA_OK;
}
