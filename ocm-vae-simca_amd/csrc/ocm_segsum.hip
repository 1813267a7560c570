// Segment sums: per-object column sums of an m × p matrix whose objects are runs
// of adjacent rows (include/ocm.h, "object-level sums"),
//   sum_out[g, j] = Σ_{r = off[g]}^{off[g+1]−1} (double)X[r·ldx + j],
// in one read of X, fp64 accumulation, a fixed summation order and no atomics.
//
// Decomposition.  The rows are cut into chunks of SS_ROWS rows at multiples of
// SS_ROWS, wherever the segments fall, so one segment of all rows and m segments
// of one row spread over the same grid.  k_segsum_part runs one workgroup per
// (chunk, column tile); a lane owns SS_VEC adjacent columns (one 16-byte load
// where ldx and the base allow, 8- or 4-byte loads otherwise) and walks the rows
// of its chunk in order, SS_UNROLL loads in flight, adding in row order.  At
// every segment boundary inside the chunk it stores the sum and starts over:
//   a segment that lies inside the chunk goes straight to sum_out (an empty one
//     too, as the exact 0.0 of a sum over no rows, written by the chunk that
//     holds its offset);
//   the part of a segment that began in an earlier chunk goes to head[chunk];
//   the part of a segment that goes on into the next chunk goes to tail[chunk].
// A chunk has at most one of each, so the partials take 2·p doubles per chunk
// and are written only where a segment crosses a chunk boundary.
// k_segsum_final then runs one workgroup per (chunk, 256 columns): the chunk
// that holds the first row of a segment of more than one chunk adds, in chunk
// order, tail[first], head[first + 1], …, head[last].  For a long segment that
// chain is shortened by k_segsum_super, which runs between the two: it adds the
// heads of each aligned group of SS_FANIN chunks that one segment covers, in
// chunk order, and the final pass takes the group's sum in place of its heads
// (the heads up to the first aligned group, the groups, the heads after the
// last).  The order is therefore a function of the offsets alone.
//
// Bytes at 1M × 2048 float32: 8.39 GB read; one segment of all rows adds 64 MB
// of heads written and read once (0.8 %); 2000 objects of 500 rows add 2·p·8 B
// per crossed boundary (3906 boundaries: 128 MB written and read); 15 625
// objects of 64 rows cross none and write their 256 MB of output once.
#include "ocm_internal.h"

namespace {

constexpr int SS_ROWS = 256;   // rows per chunk
constexpr int SS_UNROLL = 8;   // row loads in flight per lane
constexpr int SS_FANIN = 64;   // chunks per group of the second level
constexpr int SS_NT = 256;     // threads per workgroup (64 when the columns fit one wave)

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

// acc = Σ rows [r0, r1) of the lane's VEC columns at xc, in row order
template <typename T, int VEC>
__device__ __forceinline__ void sum_rows(const T* __restrict__ xc, int64_t ldx, int64_t r0, int64_t r1,
                                         double (&acc)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
  const T* q = xc + r0 * ldx;
  int64_t r = r0;
  for (; r + SS_UNROLL <= r1; r += SS_UNROLL, q += SS_UNROLL * ldx) {
    Pack<T, VEC> y[SS_UNROLL];
#pragma unroll
    for (int u = 0; u < SS_UNROLL; ++u) y[u] = *reinterpret_cast<const Pack<T, VEC>*>(q + u * ldx);
#pragma unroll
    for (int u = 0; u < SS_UNROLL; ++u)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[e] += (double)y[u].v[e];
  }
  for (; r < r1; ++r, q += ldx) {
    const Pack<T, VEC> y = *reinterpret_cast<const Pack<T, VEC>*>(q);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += (double)y.v[e];
  }
}

template <int VEC>
__device__ __forceinline__ void store_sums(double* __restrict__ dst, const double (&acc)[VEC]) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) dst[e] = acc[e];
}

// first i in [0, n) with off[i] >= v (n when there is none)
__device__ __forceinline__ int64_t lower_bound(const int64_t* __restrict__ off, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// Row reads stay inside [chunk start, min(chunk end, m)) and segment indices
// inside [0, G) whatever the offsets hold, so unchecked offsets that break the
// contract give wrong sums, never an access outside X, sum_out or the workspace.
template <typename T, int VEC>
__global__ __launch_bounds__(SS_NT) void k_segsum_part(const T* __restrict__ X, int64_t ldx, int64_t m, int p,
                                                       const int64_t* __restrict__ off, int64_t G, int ncolt,
                                                       double* __restrict__ out, int64_t ldo,
                                                       double* __restrict__ head, double* __restrict__ tail) {
  const int64_t c = blockIdx.x / ncolt;
  const int col = ((int)(blockIdx.x % ncolt) * (int)blockDim.x + (int)threadIdx.x) * VEC;
  if (col >= p) return;
  const int64_t c0 = c * SS_ROWS, cend = c0 + SS_ROWS;
  const int64_t rend = cend < m ? cend : m;
  const int64_t gf = lower_bound(off, G + 1, c0);  // the first segment that starts in this chunk or later
  if (gf > G) return;
  const T* xc = X + col;
  double acc[VEC];
  if (gf >= 1) {  // segment gf − 1 began before the chunk: its rows here, if any, are a head
    const int64_t b = off[gf];
    const int64_t e = b < rend ? b : rend;
    if (e > c0) {
      sum_rows<T, VEC>(xc, ldx, c0, e, acc);
      store_sums<VEC>(head + c * p + col, acc);
    }
  }
  for (int64_t g = gf; g < G; ++g) {
    int64_t a = off[g];
    if (a >= cend) break;
    if (a < c0) a = c0;
    const int64_t b = off[g + 1];
    if (b <= cend) {
      sum_rows<T, VEC>(xc, ldx, a, b < rend ? b : rend, acc);
      store_sums<VEC>(out + g * ldo + col, acc);
    } else {
      sum_rows<T, VEC>(xc, ldx, a, rend, acc);
      store_sums<VEC>(tail + c * p + col, acc);
      break;
    }
  }
}

// v + Σ_{i < count} src[i·stride] in index order, eight loads in flight
__device__ __forceinline__ double add_strided(double v, const double* __restrict__ src, int64_t stride,
                                              int64_t count) {
  int64_t i = 0;
  for (; i + 8 <= count; i += 8) {
    double y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) y[u] = src[(i + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += y[u];
  }
  for (; i < count; ++i) v += src[i * stride];
  return v;
}

// sup[s] = Σ head[s·SS_FANIN .. s·SS_FANIN + SS_FANIN − 1] where one segment has a head in each of them
__global__ __launch_bounds__(SS_NT) void k_segsum_super(const int64_t* __restrict__ off, int64_t G, int p,
                                                        int64_t nchunks, int ncolt,
                                                        const double* __restrict__ head, double* __restrict__ sup) {
  const int64_t s = blockIdx.x / ncolt;
  const int col = (int)(blockIdx.x % ncolt) * (int)blockDim.x + (int)threadIdx.x;
  if (col >= p) return;
  const int64_t cfirst = s * SS_FANIN, clast = cfirst + SS_FANIN - 1;
  if (clast >= nchunks) return;
  const int64_t r0 = cfirst * SS_ROWS;
  const int64_t i = lower_bound(off, G + 1, r0 + 1);  // first offset past r0: segment i − 1 holds row r0
  if (i < 1 || i > G) return;
  if (off[i - 1] >= r0 || off[i] <= clast * SS_ROWS) return;
  sup[s * p + col] = add_strided(0.0, head + cfirst * p + col, p, SS_FANIN);
}

__global__ __launch_bounds__(SS_NT) void k_segsum_final(const int64_t* __restrict__ off, int64_t G, int p,
                                                        int64_t nchunks, int ncolt,
                                                        const double* __restrict__ head,
                                                        const double* __restrict__ tail,
                                                        const double* __restrict__ sup, double* __restrict__ out,
                                                        int64_t ldo) {
  const int64_t c = blockIdx.x / ncolt;
  const int col = (int)(blockIdx.x % ncolt) * (int)blockDim.x + (int)threadIdx.x;
  if (col >= p) return;
  const int64_t c0 = c * SS_ROWS, cend = c0 + SS_ROWS;
  const int64_t i = lower_bound(off, G + 1, cend);  // segment i − 1 is the last that starts in this chunk
  if (i < 1 || i > G) return;
  const int64_t g = i - 1, b = off[i];
  if (off[g] < c0 || b <= cend) return;  // it began earlier (another chunk's job), or ends in this chunk
  int64_t clast = (b - 1) / SS_ROWS;
  if (clast > nchunks - 1) clast = nchunks - 1;
  double v = tail[c * p + col];
  const int64_t cc = c + 1;
  int64_t ca = (cc + SS_FANIN - 1) / SS_FANIN * SS_FANIN;  // the first aligned group
  if (ca > clast + 1) ca = clast + 1;
  v = add_strided(v, head + cc * p + col, p, ca - cc);
  const int64_t ns = (clast + 1 - ca) / SS_FANIN;  // whole groups (ca is aligned whenever ca ≤ clast)
  v = add_strided(v, sup + (ca / SS_FANIN) * p + col, p, ns);
  const int64_t cb = ca + ns * SS_FANIN;
  v = add_strided(v, head + cb * p + col, p, clast + 1 - cb);
  out[g * ldo + col] = v;
}

inline bool aligned_to(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

template <typename T>
int segsum(ocm_ctx* ctx, const T* X, int64_t ldx, int64_t m, int32_t p, const int64_t* off, int64_t G, double* out,
           int64_t ldo, hipStream_t st) {
  if (G == 0) return OCM_OK;
  // the widest load the row pitch, the width and the base allow, 16 bytes at the most
  int vec = 16 / (int)sizeof(T);
  while (vec > 1 && !(p % vec == 0 && ldx % vec == 0 && aligned_to(X, sizeof(T) * vec))) vec >>= 1;
  const int colthreads = p / vec;
  const int nt = colthreads <= 64 ? 64 : SS_NT;
  const int ncolt = (colthreads + nt - 1) / nt;
  const int ncolt1 = (p + SS_NT - 1) / SS_NT;  // the second pass: one column per lane
  // row m has a chunk too: an empty segment at off = m is written by the chunk that holds its offset
  const int64_t nchunks = m / SS_ROWS + 1;
  const int64_t nsuper = nchunks / SS_FANIN;
  OCM_REQUIRE(nchunks * std::max(ncolt, ncolt1) < (1LL << 31), "ocm_segsum: m × p too large for one call");
  auto* w = static_cast<double*>(ocm::workspace(ctx, (size_t)(2 * nchunks + nsuper) * p * sizeof(double), st));
  if (!w) return OCM_ERR_NOMEM;
  double* head = w;
  double* tail = head + nchunks * p;
  double* sup = tail + nchunks * p;
  const dim3 grid((unsigned)(nchunks * ncolt));
#define OCM_SS(V_) \
  hipLaunchKernelGGL((k_segsum_part<T, V_>), grid, dim3(nt), 0, st, X, ldx, m, p, off, G, ncolt, out, ldo, head, tail)
  if (vec == 4) {
    if constexpr (sizeof(T) == 4) OCM_SS(4);
  } else if (vec == 2) {
    OCM_SS(2);
  } else {
    OCM_SS(1);
  }
#undef OCM_SS
  OCM_CHECK_LAUNCH("k_segsum_part");
  if (nchunks < 2) return OCM_OK;  // one chunk: no segment crosses a boundary
  if (nsuper >= 2) {               // group 0 is never used: a head chain starts at chunk ≥ 1
    hipLaunchKernelGGL(k_segsum_super, dim3((unsigned)(nsuper * ncolt1)), dim3(SS_NT), 0, st, off, G, p, nchunks,
                       ncolt1, head, sup);
    OCM_CHECK_LAUNCH("k_segsum_super");
  }
  hipLaunchKernelGGL(k_segsum_final, dim3((unsigned)(nchunks * ncolt1)), dim3(SS_NT), 0, st, off, G, p, nchunks,
                     ncolt1, head, tail, sup, out, ldo);
  OCM_CHECK_LAUNCH("k_segsum_final");
  return OCM_OK;
}

}  // namespace

extern "C" {

#define OCM_SEGSUM_CHECKS(name)                                                                       \
  OCM_REQUIRE(ctx && offsets && sum_out, name ": NULL argument");                                     \
  OCM_REQUIRE(X || m == 0, name ": X is NULL");                                                       \
  OCM_REQUIRE(m >= 0 && m < (1LL << 31) && nseg >= 0, name ": bad shape (0 <= m < 2^31, nseg >= 0)"); \
  OCM_REQUIRE(p > 0 && ldx >= p && ld_out >= p, name ": bad shape (p > 0, ldx >= p, ld_out >= p)")

int ocm_segsum_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const int64_t* offsets,
                   int64_t nseg, double* sum_out, int64_t ld_out, void* stream) {
  OCM_SEGSUM_CHECKS("ocm_segsum_f32");
  return segsum<float>(ctx, X, ldx, m, p, offsets, nseg, sum_out, ld_out, (hipStream_t)stream);
}

int ocm_segsum_f64(ocm_ctx* ctx, const double* X, int64_t ldx, int64_t m, int32_t p, const int64_t* offsets,
                   int64_t nseg, double* sum_out, int64_t ld_out, void* stream) {
  OCM_SEGSUM_CHECKS("ocm_segsum_f64");
  return segsum<double>(ctx, X, ldx, m, p, offsets, nseg, sum_out, ld_out, (hipStream_t)stream);
}

#undef OCM_SEGSUM_CHECKS

}  // extern "C"
