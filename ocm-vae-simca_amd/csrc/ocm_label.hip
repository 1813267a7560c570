// Images into objects (include/ocm.h, "images into objects"): the foreground
// mask of an (H, W, p) cube, the connected components of a mask, and the gather
// of pixel rows, i.e. nut_data.py:64-70 (band mean, threshold, ndimage.label)
// and :131-144 (hsi_image[labeled_array == obj]) without the host.
//
// ocm_label_u8 is a union–find over a parent array P (one int32 per pixel, −1
// for background) in which a parent is always a smaller linear pixel index of
// the same component, so the root of a tree is its smallest index.  Six
// launches, whatever the image holds:
//   1 k_label_tile     one workgroup per LB_TH × LB_TW tile: a wave takes a row,
//                      a ballot gives the row's runs, the runs of adjacent rows
//                      are united in LDS, and every pixel stores the global
//                      index of its tile-local root.  No inter-workgroup traffic.
//   2 k_label_border   one thread per pixel on the first row / column of a tile
//                      (not of the image): it unites the pixel with its
//                      neighbours across the border, the diagonal ones at a
//                      tile corner included, by agent-scope atomicMin on P.
//   3 k_label_flatten  every pixel follows P to its root (the launch boundary
//                      orders it after every union), stores root + 1 in the
//                      label image and counts the roots of its 1024 pixels.
//   4 k_label_scan     one workgroup: exclusive prefix sum of those counts, n.
//   5 k_label_rank     a root's rank among all roots, 1-based, stored in P[root].
//   6 k_label_write    label = P[root].
// Roots are numbered in index order, which is the order in which a raster scan
// meets the components: scipy.ndimage.label's numbering.  No workgroup waits
// for another anywhere: no spin, no flag, no arrival counter.
//
// Bytes at H·W = 1M: the mask 1 MB read twice, P 4 MB written once and read
// three times, the labels 4 MB written twice and read once: ≈ 30 MB, against
// the 1 GB one pass over a p = 256 float32 cube reads.
#include "ocm_internal.h"

namespace {

constexpr int LB_TW = 64;       // tile width: one lane per column, one ballot per row
constexpr int LB_TH = 32;       // tile height
constexpr int LB_NT = 256;      // threads per workgroup
constexpr int LB_CHUNK = 1024;  // pixels per workgroup of the flatten / rank launches (4 per thread)

// ---- union–find -----------------------------------------------------------
// Unite the trees of a and b in `par` (LDS or global).  Correctness rests only
// on the value an atomicMin RETURNS: a parent only ever decreases and every
// value a cell has held lies in the cell's component, so a stale plain load in
// `find` can stop short of the root or walk an older path, which costs an extra
// turn of the loop and can never unite two components that do not touch.  When
// the min returns old ≠ a, cell a was no root: it now points at min(old, b), and
// what remains is to unite old and b.  max(a, b) strictly decreases, so the loop
// ends without a timeout.
template <typename Find>
__device__ __forceinline__ void unite(int* par, int a, int b, Find find) {
  a = find(a);
  b = find(b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) break;  // a was a root and now hangs under b
    a = find(old);
  }
}

__device__ __forceinline__ bool bit(unsigned long long w, int c) { return c >= 0 && c < 64 && ((w >> c) & 1ull); }

__global__ __launch_bounds__(LB_NT) void k_label_tile(const uint8_t* __restrict__ mask, int H, int W, int conn,
                                                      int ntx, int* __restrict__ P) {
  __shared__ int lp[LB_TH * LB_TW];
  __shared__ unsigned long long rowbits[LB_TH];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ty = blockIdx.x / ntx, tx = blockIdx.x % ntx;
  const int y0 = ty * LB_TH, x0 = tx * LB_TW;
  const int gx = x0 + lane;
  // runs of a row: every pixel starts at the first pixel of its run
  for (int r = wave; r < LB_TH; r += LB_NT / 64) {
    const int gy = y0 + r;
    const bool fg = gy < H && gx < W && mask[(int64_t)gy * W + gx] != 0;
    const unsigned long long bits = __ballot(fg);
    const unsigned long long gaps = ~bits & ((1ull << lane) - 1ull);  // background left of this lane
    const int start = gaps ? 64 - __clzll(gaps) : 0;
    lp[r * LB_TW + lane] = fg ? r * LB_TW + start : -1;
    if (lane == 0) rowbits[r] = bits;
  }
  __syncthreads();
  volatile int* vlp = lp;
  auto find = [vlp](int a) {
    int q;
    while ((q = vlp[a]) != a) a = q;
    return a;
  };
  // a row's runs against the row above; of a stretch of pixels that share both runs only the first unites
  for (int r = wave < 1 ? LB_NT / 64 : wave; r < LB_TH; r += LB_NT / 64) {
    const unsigned long long cur = rowbits[r], up = rowbits[r - 1];
    if (!bit(cur, lane)) continue;
    const int me = r * LB_TW + lane, above = me - LB_TW;
    if (bit(up, lane)) {
      if (!(bit(cur, lane - 1) && bit(up, lane - 1))) unite(lp, me, above, find);
    } else if (conn == 8) {
      if (bit(up, lane - 1) && !bit(cur, lane - 1)) unite(lp, me, above - 1, find);
      if (bit(up, lane + 1) && !bit(cur, lane + 1)) unite(lp, me, above + 1, find);
    }
  }
  __syncthreads();
  for (int r = wave; r < LB_TH; r += LB_NT / 64) {
    const int gy = y0 + r;
    if (gy >= H || gx >= W) continue;
    int v = -1;
    if (bit(rowbits[r], lane)) {
      const int root = find(r * LB_TW + lane);
      v = (int)((int64_t)(y0 + root / LB_TW) * W + x0 + root % LB_TW);
    }
    P[(int64_t)gy * W + gx] = v;
  }
}

// threads [0, nhb·W): pixel x of row k·LB_TH against the row above; the rest:
// pixel y of column j·LB_TW against the column to the left
__global__ __launch_bounds__(LB_NT) void k_label_border(const uint8_t* __restrict__ mask, int H, int W, int conn,
                                                        int64_t nh, int64_t total, int* P) {
  const int64_t t = (int64_t)blockIdx.x * LB_NT + threadIdx.x;
  if (t >= total) return;
  auto fg = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W && mask[(int64_t)y * W + x] != 0; };
  auto at = [&](int y, int x) { return (int)((int64_t)y * W + x); };
  // agent-scope loads (served past this CU's L1) only keep the walks short; see unite()
  auto find = [P](int a) {
    int q;
    while ((q = __hip_atomic_load(P + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != a) a = q;
    return a;
  };
  if (t < nh) {
    const int y = (int)(t / W + 1) * LB_TH, x = (int)(t % W);
    if (!fg(y, x)) return;
    if (fg(y - 1, x)) {
      if (!(fg(y, x - 1) && fg(y - 1, x - 1))) unite(P, at(y, x), at(y - 1, x), find);
    } else if (conn == 8) {
      if (fg(y - 1, x - 1) && !fg(y, x - 1)) unite(P, at(y, x), at(y - 1, x - 1), find);
      if (fg(y - 1, x + 1) && !fg(y, x + 1)) unite(P, at(y, x), at(y - 1, x + 1), find);
    }
  } else {
    const int64_t u = t - nh;
    const int x = (int)(u / H + 1) * LB_TW, y = (int)(u % H);
    if (!fg(y, x)) return;
    if (fg(y, x - 1)) {  // the diagonal neighbours of that column touch (y, x − 1) themselves
      unite(P, at(y, x), at(y, x - 1), find);
    } else if (conn == 8) {
      if (fg(y - 1, x - 1)) unite(P, at(y, x), at(y - 1, x - 1), find);
      if (fg(y + 1, x - 1)) unite(P, at(y, x), at(y + 1, x - 1), find);
    }
  }
}

// exclusive prefix sum of v over the LB_NT threads of a workgroup, in thread order; *total = the sum
__device__ __forceinline__ int block_excl_scan(int v, int* total) {
  __shared__ int wsum[LB_NT / 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < LB_NT / 64; ++w) {
    if (w < wave) before += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(LB_NT) void k_label_flatten(const int* __restrict__ P, int64_t HW,
                                                         int* __restrict__ L, int* __restrict__ bsum) {
  const int64_t base = (int64_t)blockIdx.x * LB_CHUNK + threadIdx.x * 4;
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + e;
    if (i >= HW) break;
    int q = P[i];
    if (q < 0) {
      L[i] = 0;
      continue;
    }
    cnt += q == (int)i;
    int n;
    while ((n = P[q]) != q) q = n;
    L[i] = q + 1;
  }
  int total;
  block_excl_scan(cnt, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(LB_NT) void k_label_scan(int* __restrict__ bsum, int64_t nb, int* __restrict__ n_out) {
  const int64_t per = (nb + LB_NT - 1) / LB_NT;
  const int64_t b = threadIdx.x * per, e = b + per < nb ? b + per : nb;
  int s = 0;
  for (int64_t i = b; i < e; ++i) s += bsum[i];
  int total;
  int run = block_excl_scan(s, &total);
  for (int64_t i = b; i < e; ++i) {
    const int v = bsum[i];
    bsum[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) *n_out = total;
}

__global__ __launch_bounds__(LB_NT) void k_label_rank(int* __restrict__ P, int64_t HW, const int* __restrict__ bsum) {
  const int64_t base = (int64_t)blockIdx.x * LB_CHUNK + threadIdx.x * 4;
  bool root[4];
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = base + e;
    root[e] = i < HW && P[i] == (int)i;
    cnt += root[e];
  }
  int total;
  int rank = block_excl_scan(cnt, &total) + bsum[blockIdx.x];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (root[e]) P[base + e] = ++rank;  // read again by no thread of this launch
}

__global__ __launch_bounds__(LB_NT) void k_label_write(const int* __restrict__ P, int64_t HW, int* __restrict__ L) {
  const int64_t i = (int64_t)blockIdx.x * LB_NT + threadIdx.x;
  if (i >= HW) return;
  const int l = L[i];
  if (l) L[i] = P[l - 1];
}

// ---- the mask pass and the row gather -------------------------------------
template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

constexpr int FG_UNROLL = 8;  // loads in flight per lane

// One wave per row, four rows per workgroup (as k_prep_rowstats).  Lane l adds
// the VEC-wide pieces at columns VEC·(l + 64k) in order of k, then the wave's
// 64 partial sums meet in a butterfly: a fixed order for a given (p, VEC).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_fgmask(const T* __restrict__ X, int64_t ldx, int64_t m, int p,
                                                double thr, uint8_t* __restrict__ mask,
                                                double* __restrict__ mean_out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= m) return;
  const T* xr = X + r * ldx;
  const int pv = p - p % VEC;
  double s = 0.0;
  for (int c0 = lane * VEC; c0 < pv; c0 += 64 * VEC * FG_UNROLL) {
    Pack<T, VEC> y[FG_UNROLL];
#pragma unroll
    for (int u = 0; u < FG_UNROLL; ++u) {
      const int c = c0 + u * 64 * VEC;
      if (c < pv) {
        y[u] = *reinterpret_cast<const Pack<T, VEC>*>(xr + c);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) y[u].v[e] = T(0);
      }
    }
#pragma unroll
    for (int u = 0; u < FG_UNROLL; ++u)
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += (double)y[u].v[e];
  }
  if (pv + lane < p) s += (double)xr[pv + lane];  // the p % VEC columns that fill no piece
  const double mean = wave_sum_f64(s) / p;
  if (lane == 0) {
    mask[r] = !(mean < thr);  // ~(mean < thr): NaN is foreground
    if (mean_out) mean_out[r] = mean;
  }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int GR_UNROLL = 8;

// One wave per output row; V is the copy unit (16 bytes, or one element as an
// unsigned integer: the bits travel unchanged), ldx / ldo / pu in units of V.
template <typename V>
__global__ __launch_bounds__(256) void k_gather_rows(const V* __restrict__ X, int64_t ldx,
                                                     const int64_t* __restrict__ rows, int64_t n, int pu,
                                                     V* __restrict__ out, int64_t ldo) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + wave;
  if (i >= n) return;
  const V* src = X + rows[i] * ldx;
  V* dst = out + i * ldo;
  for (int c0 = lane; c0 < pu; c0 += 64 * GR_UNROLL) {
    V y[GR_UNROLL];
#pragma unroll
    for (int u = 0; u < GR_UNROLL; ++u) {
      const int c = c0 + 64 * u;
      if (c < pu) y[u] = src[c];
    }
#pragma unroll
    for (int u = 0; u < GR_UNROLL; ++u) {
      const int c = c0 + 64 * u;
      if (c < pu) dst[c] = y[u];
    }
  }
}

inline bool aligned_to(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

template <typename T>
int fgmask(const T* X, int64_t ldx, int64_t m, int32_t p, double thr, uint8_t* mask, double* mean_out,
           hipStream_t st) {
  if (m == 0) return OCM_OK;
  constexpr int V = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)((m + 3) / 4));
  if (ldx % V == 0 && aligned_to(X, 16))
    hipLaunchKernelGGL((k_fgmask<T, V>), grid, dim3(256), 0, st, X, ldx, m, p, thr, mask, mean_out);
  else
    hipLaunchKernelGGL((k_fgmask<T, 1>), grid, dim3(256), 0, st, X, ldx, m, p, thr, mask, mean_out);
  OCM_CHECK_LAUNCH("k_fgmask");
  return OCM_OK;
}

template <typename T, typename U>
int gather_rows(const T* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p, T* out, int64_t ldo,
                hipStream_t st) {
  if (n == 0) return OCM_OK;
  constexpr int V = 16 / (int)sizeof(T);
  const dim3 grid((unsigned)((n + 3) / 4));
  if (p % V == 0 && ldx % V == 0 && ldo % V == 0 && aligned_to(X, 16) && aligned_to(out, 16))
    hipLaunchKernelGGL(k_gather_rows<u32x4>, grid, dim3(256), 0, st, reinterpret_cast<const u32x4*>(X), ldx / V,
                       rows, n, p / V, reinterpret_cast<u32x4*>(out), ldo / V);
  else
    hipLaunchKernelGGL(k_gather_rows<U>, grid, dim3(256), 0, st, reinterpret_cast<const U*>(X), ldx, rows, n, p,
                       reinterpret_cast<U*>(out), ldo);
  OCM_CHECK_LAUNCH("k_gather_rows");
  return OCM_OK;
}

}  // namespace

extern "C" {

#define OCM_FGMASK_CHECKS(name)                                                            \
  OCM_REQUIRE(ctx && mask_out, name ": NULL argument");                                    \
  OCM_REQUIRE(X || m == 0, name ": X is NULL");                                            \
  OCM_REQUIRE(m >= 0 && m < (1LL << 33), name ": bad shape (0 <= m < 2^33)");              \
  OCM_REQUIRE(p >= 1 && ldx >= p, name ": bad shape (p >= 1, ldx >= p)")

int ocm_fgmask_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, double threshold,
                   uint8_t* mask_out, double* mean_out, void* stream) {
  OCM_FGMASK_CHECKS("ocm_fgmask_f32");
  return fgmask<float>(X, ldx, m, p, threshold, mask_out, mean_out, (hipStream_t)stream);
}

int ocm_fgmask_f64(ocm_ctx* ctx, const double* X, int64_t ldx, int64_t m, int32_t p, double threshold,
                   uint8_t* mask_out, double* mean_out, void* stream) {
  OCM_FGMASK_CHECKS("ocm_fgmask_f64");
  return fgmask<double>(X, ldx, m, p, threshold, mask_out, mean_out, (hipStream_t)stream);
}

#undef OCM_FGMASK_CHECKS

int ocm_label_u8(ocm_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t connectivity, int32_t* labels_out,
                 int32_t* n_out, void* stream) {
  OCM_REQUIRE(connectivity == 4 || connectivity == 8, "ocm_label_u8: connectivity must be 4 or 8");
  OCM_REQUIRE(H >= 1 && W >= 1, "ocm_label_u8: H and W must be at least 1");
  const int64_t HW = (int64_t)H * W;
  OCM_REQUIRE(HW <= 0x7fffffffLL, "ocm_label_u8: H * W exceeds 2^31 - 1");
  OCM_REQUIRE(ctx && mask && labels_out && n_out, "ocm_label_u8: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int ntx = (W + LB_TW - 1) / LB_TW, nty = (H + LB_TH - 1) / LB_TH;
  const int64_t nb = (HW + LB_CHUNK - 1) / LB_CHUNK;
  ocm::Carve cv{static_cast<char*>(ocm::workspace(ctx, (size_t)(HW + nb) * sizeof(int) + 512, st))};
  if (!cv.base) return OCM_ERR_NOMEM;
  int* P = cv.take<int>((size_t)HW);
  int* bsum = cv.take<int>((size_t)nb);
  hipLaunchKernelGGL(k_label_tile, dim3((unsigned)((int64_t)ntx * nty)), dim3(LB_NT), 0, st, mask, H, W, connectivity,
                     ntx, P);
  OCM_CHECK_LAUNCH("k_label_tile");
  const int64_t nh = (int64_t)(nty - 1) * W, total = nh + (int64_t)(ntx - 1) * H;
  if (total > 0) {
    hipLaunchKernelGGL(k_label_border, dim3((unsigned)((total + LB_NT - 1) / LB_NT)), dim3(LB_NT), 0, st, mask, H, W,
                       connectivity, nh, total, P);
    OCM_CHECK_LAUNCH("k_label_border");
  }
  hipLaunchKernelGGL(k_label_flatten, dim3((unsigned)nb), dim3(LB_NT), 0, st, P, HW, labels_out, bsum);
  OCM_CHECK_LAUNCH("k_label_flatten");
  hipLaunchKernelGGL(k_label_scan, dim3(1), dim3(LB_NT), 0, st, bsum, nb, n_out);
  OCM_CHECK_LAUNCH("k_label_scan");
  hipLaunchKernelGGL(k_label_rank, dim3((unsigned)nb), dim3(LB_NT), 0, st, P, HW, bsum);
  OCM_CHECK_LAUNCH("k_label_rank");
  hipLaunchKernelGGL(k_label_write, dim3((unsigned)((HW + LB_NT - 1) / LB_NT)), dim3(LB_NT), 0, st, P, HW, labels_out);
  OCM_CHECK_LAUNCH("k_label_write");
  return OCM_OK;
}

#define OCM_GATHER_CHECKS(name)                                                                   \
  OCM_REQUIRE(ctx, name ": NULL context");                                                        \
  OCM_REQUIRE(n >= 0 && n < (1LL << 33), name ": bad shape (0 <= n < 2^33)");                     \
  OCM_REQUIRE((X && rows && out) || n == 0, name ": NULL argument");                              \
  OCM_REQUIRE(p >= 1 && ldx >= p && ldo >= p, name ": bad shape (p >= 1, ldx >= p, ldo >= p)")

int ocm_gather_rows_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        float* out, int64_t ldo, void* stream) {
  OCM_GATHER_CHECKS("ocm_gather_rows_f32");
  return gather_rows<float, uint32_t>(X, ldx, rows, n, p, out, ldo, (hipStream_t)stream);
}

int ocm_gather_rows_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        double* out, int64_t ldo, void* stream) {
  OCM_GATHER_CHECKS("ocm_gather_rows_f64");
  return gather_rows<double, unsigned long long>(X, ldx, rows, n, p, out, ldo, (hipStream_t)stream);
}

#undef OCM_GATHER_CHECKS

}  // extern "C"
