// Robust calibration (include/ocm.h, "robust calibration"): the spatial (L1)
// median of n rows by Weiszfeld's iteration with the Vardi–Zhang correction,
// and the rows sphered about a centre, u_i = (x_i − m)/‖x_i − m‖.
//
// Decomposition of one Weiszfeld step.  The rows are cut into chunks of L1_ROWS
// rows at multiples of L1_ROWS.  k_l1_part runs one workgroup of eight waves per
// chunk and walks it in tiles of L1_TILE rows.  A row is needed twice: for its
// distance d_i (a sum over the whole row) and then, weighted by 1/d_i, for the p
// column sums.  Phase 1 gives each wave the tile rows w, w + 8: its lanes stride
// over the row with up to eight 16-byte loads in flight, store what they loaded
// into the LDS tile and add the squared differences in fp64; a butterfly gives
// d_i.  Phase 2 turns the tile: a thread owns up to L1_KC vector columns and adds
// x_ij/d_i over the tile's rows in row order, out of LDS.  So X leaves HBM once
// per step.  Where 16 rows do not fit in 128 KiB (p > 2048 float32, 1024
// float64) phase 2 reads the rows again from global memory, 16 rows · p values
// after they came in, and keeps the running sums in the chunk's partial row
// (the same thread reads and writes a column, no other does).  The chunk writes
// p + 3 partials: S, W = Σ1/d, Σd, η.  k_l1_group (more than L1_FANIN chunks)
// adds each aligned group of L1_FANIN chunks in chunk order; k_l1_update, one
// workgroup, adds the groups (or the chunks) in order, forms R = S − W·m, γ and
// m⁺, writes the centre, the step length and the done flag.  Every launch of a
// later step reads the flag first and returns.  After the last step one more
// pass (k_l1_part in its distance-only form) measures d_i, Σd and η at the
// returned centre.  Kernel boundaries are the only hand-offs: no atomics, no
// fences, and the order of every sum is a function of (n, p, ldx, base) alone.
//
// Bytes at 1M × 2048 float32: 8.39 GB read per step; the partials are 3907
// chunks · 2051 doubles = 64 MB written and read once (0.8 %), the groups 1 MB.
#include "ocm_internal.h"

namespace {

constexpr int L1_ROWS = 256;   // rows per chunk
constexpr int L1_TILE = 16;    // rows per tile
constexpr int L1_NT = 512;     // threads per workgroup of k_l1_part
constexpr int L1_NW = L1_NT / 64;
constexpr int L1_UNROLL = 8;   // row loads in flight per lane
constexpr int L1_KC = 4;       // vector columns a thread owns in the LDS-resident form
constexpr int L1_FANIN = 64;   // chunks per group
constexpr int L1_UNT = 1024;   // threads of k_l1_update
constexpr size_t L1_TILE_BYTES = 128 * 1024;

enum { L1_RESIDENT = 0, L1_TWICE = 1, L1_DIST = 2 };
enum { INFO_ITERS = 0, INFO_DONE = 1, INFO_STEP = 2, INFO_OBJ = 3, INFO_COINC = 4 };

template <typename T, int VEC>
struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

// LDS of k_l1_part: wave partials, 1/d and the source row of each tile row,
// then (resident form) the centre and the tile; every offset a multiple of 16
constexpr int L1_RED = 4 * L1_NW;  // doubles
__host__ __device__ inline size_t l1_lds_head() { return (L1_RED + L1_TILE) * sizeof(double) + L1_TILE * sizeof(int64_t); }
template <typename T>
inline size_t l1_lds_bytes(int p, int mode) {
  size_t b = l1_lds_head();
  if (mode == L1_RESIDENT) b += (size_t)((p + 1) & ~1) * sizeof(double) + (size_t)L1_TILE * p * sizeof(T);
  return b;
}

template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(L1_NT) void k_l1_part(const T* __restrict__ X, int64_t ldx,
                                                   const int64_t* __restrict__ rows, int64_t n, int p,
                                                   const double* center, const double* info,
                                                   double* part_all, double* __restrict__ dist_out) {
  if (MODE != L1_DIST && info[INFO_DONE] != 0.0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char l1_lds[];
  double* red = reinterpret_cast<double*>(l1_lds);
  double* invd = red + L1_RED;
  int64_t* rix = reinterpret_cast<int64_t*>(invd + L1_TILE);
  double* mc = reinterpret_cast<double*>(rix + L1_TILE);
  T* tile = reinterpret_cast<T*>(mc + ((p + 1) & ~1));
  using P = Pack<T, VEC>;

  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int pv = p / VEC;
  const int64_t r0 = (int64_t)blockIdx.x * L1_ROWS;
  const int64_t rend = r0 + L1_ROWS < n ? r0 + L1_ROWS : n;
  double* part = part_all + (int64_t)blockIdx.x * (p + 3);
  const double* mm = center;
  if constexpr (MODE == L1_RESIDENT) {
    for (int j = tid; j < p; j += L1_NT) mc[j] = center[j];
    mm = mc;
    __syncthreads();
  }

  double acc[L1_KC][VEC];
#pragma unroll
  for (int k = 0; k < L1_KC; ++k)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[k][e] = 0.0;
  double wW = 0.0, wD = 0.0, wE = 0.0;  // this wave's Σ1/d, Σd, η (equal in every lane)

  for (int64_t t0 = r0; t0 < rend; t0 += L1_TILE) {
    const int nrows = rend - t0 < L1_TILE ? (int)(rend - t0) : L1_TILE;
    // ---- phase 1: the distances of the tile's rows, wave w takes rows w, w + 8
    for (int rr = wave; rr < L1_TILE; rr += L1_NW) {
      const int64_t row = t0 + (rr < nrows ? rr : nrows - 1);  // the tail of a short tile repeats its last row
      const int64_t src = rows ? rows[row] : row;
      if (rr >= nrows) {
        if (lane == 0) {
          invd[rr] = 0.0;
          rix[rr] = src;
        }
        continue;
      }
      const T* xr = X + src * ldx;
      double s = 0.0;
      for (int c0 = lane; c0 < pv; c0 += 64 * L1_UNROLL) {
        P y[L1_UNROLL];
#pragma unroll
        for (int u = 0; u < L1_UNROLL; ++u) {
          const int c = c0 + 64 * u;
          if (c < pv) y[u] = *reinterpret_cast<const P*>(xr + (int64_t)c * VEC);
        }
#pragma unroll
        for (int u = 0; u < L1_UNROLL; ++u) {
          const int c = c0 + 64 * u;
          if (c < pv) {
            if constexpr (MODE == L1_RESIDENT) *reinterpret_cast<P*>(tile + (size_t)rr * p + (size_t)c * VEC) = y[u];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
              const double df = (double)y[u].v[e] - mm[c * VEC + e];
              s += df * df;
            }
          }
        }
      }
      s = wave_sum_f64(s);
      const double d = sqrt(s);
      const double w = d > 0.0 ? 1.0 / d : 0.0;  // a coincident row (d == 0 exactly) adds nothing
      wW += w;
      wD += d;
      wE += d == 0.0 ? 1.0 : 0.0;
      if (lane == 0) {
        invd[rr] = w;
        rix[rr] = src;
        if (dist_out) dist_out[row] = d;
      }
    }
    if constexpr (MODE == L1_DIST) continue;
    __syncthreads();
    // ---- phase 2: S_j += x_ij/d_i over the tile's rows, in row order
    if constexpr (MODE == L1_RESIDENT) {
#pragma unroll
      for (int k = 0; k < L1_KC; ++k) {
        const int c = tid + k * L1_NT;
        if (c < pv) {
          for (int rr = 0; rr < nrows; ++rr) {
            const P y = *reinterpret_cast<const P*>(tile + (size_t)rr * p + (size_t)c * VEC);
            const double w = invd[rr];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[k][e] += (double)y.v[e] * w;
          }
        }
      }
    } else {
      for (int c = tid; c < pv; c += L1_NT) {
        double a[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = t0 == r0 ? 0.0 : part[c * VEC + e];
        P y[L1_TILE];
#pragma unroll
        for (int rr = 0; rr < L1_TILE; ++rr) y[rr] = *reinterpret_cast<const P*>(X + rix[rr] * ldx + (int64_t)c * VEC);
#pragma unroll
        for (int rr = 0; rr < L1_TILE; ++rr) {
          const double w = invd[rr];  // 0 past the end of a short tile
          if (rr < nrows) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) a[e] += (double)y[rr].v[e] * w;
          }
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) part[c * VEC + e] = a[e];
      }
    }
    __syncthreads();  // the tile, invd and rix are free again
  }

  if constexpr (MODE == L1_RESIDENT) {
#pragma unroll
    for (int k = 0; k < L1_KC; ++k) {
      const int c = tid + k * L1_NT;
      if (c < pv) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) part[c * VEC + e] = acc[k][e];
      }
    }
  }
  if (lane == 0) {
    red[wave * 4 + 0] = wW;
    red[wave * 4 + 1] = wD;
    red[wave * 4 + 2] = wE;
  }
  __syncthreads();
  if (tid < 3) {
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < L1_NW; ++w) v += red[w * 4 + tid];  // in wave order
    part[p + tid] = v;
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

// grp[g, col] = Σ part[g·L1_FANIN + i, col], i < L1_FANIN (fewer in the last group), col in [col0, stride)
__global__ __launch_bounds__(256) void k_l1_group(const double* __restrict__ part, int64_t nchunks, int stride,
                                                  int col0, int ncolt, const double* info, int check_done,
                                                  double* __restrict__ grp) {
  if (check_done && info[INFO_DONE] != 0.0) return;
  const int64_t g = blockIdx.x / ncolt;
  const int col = col0 + (int)(blockIdx.x % ncolt) * 256 + (int)threadIdx.x;
  if (col >= stride) return;
  const int64_t c0 = g * L1_FANIN;
  const int64_t cnt = nchunks - c0 < L1_FANIN ? nchunks - c0 : L1_FANIN;
  grp[g * stride + col] = add_strided(0.0, part + c0 * stride + col, stride, cnt);
}

// Σ over the workgroup in a fixed order: a butterfly in each wave, then the waves in order
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* sh) {
  v = wave_sum_f64(v);
  __syncthreads();  // sh is free
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) t += sh[w];
  return t;
}

// one workgroup: S, W, η from the partials in order, then the Vardi–Zhang update of the centre
__global__ __launch_bounds__(L1_UNT) void k_l1_update(const double* __restrict__ src, int64_t count, int p,
                                                      double* center, double* sfin, double* info, double tol,
                                                      int it) {
  if (info[INFO_DONE] != 0.0) return;
  __shared__ double sh[L1_UNT / 64];
  __shared__ double tot[3];
  const int tid = (int)threadIdx.x, stride = p + 3;
  for (int j = tid; j < stride; j += L1_UNT) {
    const double v = add_strided(0.0, src + j, stride, count);
    if (j < p)
      sfin[j] = v;
    else
      tot[j - p] = v;
  }
  __syncthreads();
  const double W = tot[0], eta = tot[2];
  double r2 = 0.0;
  for (int j = tid; j < p; j += L1_UNT) {
    const double R = sfin[j] - W * center[j];
    r2 += R * R;
  }
  const double r = sqrt(block_sum<L1_UNT / 64>(r2, sh));
  const double gamma = eta == 0.0 ? 0.0 : (r == 0.0 ? 1.0 : fmin(1.0, eta / r));
  const bool stay = gamma == 1.0 || W == 0.0;  // the centre is the median, or every row lies on it
  double ds = 0.0, ns = 0.0;
  for (int j = tid; j < p; j += L1_UNT) {
    const double m = center[j];
    const double mp = stay ? m : (1.0 - gamma) * (sfin[j] / W) + gamma * m;
    center[j] = mp;
    ds += (mp - m) * (mp - m);
    ns += mp * mp;
  }
  const double step = sqrt(block_sum<L1_UNT / 64>(ds, sh));
  const double norm = sqrt(block_sum<L1_UNT / 64>(ns, sh));
  if (tid == 0) {
    info[INFO_ITERS] = (double)(it + 1);
    info[INFO_STEP] = step;
    info[INFO_DONE] = step <= tol * norm ? 1.0 : 0.0;
  }
}

// the objective Σd and η at the returned centre, from the distance pass's partials in order
__global__ __launch_bounds__(64) void k_l1_final(const double* __restrict__ src, int64_t count, int p,
                                                 double* info) {
  const int tid = (int)threadIdx.x, stride = p + 3;
  if (tid == 0) info[INFO_OBJ] = add_strided(0.0, src + p + 1, stride, count);
  if (tid == 1) info[INFO_COINC] = add_strided(0.0, src + p + 2, stride, count);
}

// one wave per row: d = ‖x − m‖, then u = (x − m)/d rounded to T (zeros where d == 0)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_sphere_rows(const T* __restrict__ X, int64_t ldx,
                                                     const int64_t* __restrict__ rows, int64_t n, int p,
                                                     const double* __restrict__ center, T* __restrict__ U,
                                                     int64_t ldu, double* __restrict__ dist_out) {
  using P = Pack<T, VEC>;
  const int lane = (int)threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= n) return;
  const int pv = p / VEC;
  const T* xr = X + (rows ? rows[row] : row) * ldx;
  T* ur = U + row * ldu;
  double s = 0.0;
  for (int c0 = lane; c0 < pv; c0 += 64 * L1_UNROLL) {
    P y[L1_UNROLL];
#pragma unroll
    for (int u = 0; u < L1_UNROLL; ++u) {
      const int c = c0 + 64 * u;
      if (c < pv) y[u] = *reinterpret_cast<const P*>(xr + (int64_t)c * VEC);
    }
#pragma unroll
    for (int u = 0; u < L1_UNROLL; ++u) {
      const int c = c0 + 64 * u;
      if (c < pv) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const double df = (double)y[u].v[e] - center[c * VEC + e];
          s += df * df;
        }
      }
    }
  }
  s = wave_sum_f64(s);
  const double d = sqrt(s);
  const double w = d > 0.0 ? 1.0 / d : 0.0;
  if (lane == 0 && dist_out) dist_out[row] = d;
  for (int c = lane; c < pv; c += 64) {
    const P y = *reinterpret_cast<const P*>(xr + (int64_t)c * VEC);
    P o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.v[e] = (T)(((double)y.v[e] - center[c * VEC + e]) * w);
    *reinterpret_cast<P*>(ur + (int64_t)c * VEC) = o;
  }
}

inline bool aligned_to(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

template <typename T, int VEC, int MODE>
int launch_part(ocm_ctx* ctx, size_t lds, int64_t nchunks, hipStream_t st, const T* X, int64_t ldx,
                const int64_t* rows, int64_t n, int p, const double* center, const double* info, double* part,
                double* dist_out, bool set_attr) {
  auto kern = k_l1_part<T, VEC, MODE>;
  if (set_attr && lds > 48 * 1024)
    OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)nchunks), dim3(L1_NT), lds, st, X, ldx, rows, n, p, center, info, part,
                     dist_out);
  OCM_CHECK_LAUNCH("k_l1_part");
  return OCM_OK;
}

template <typename T, int VEC>
int l1median_v(ocm_ctx* ctx, const T* X, int64_t ldx, const int64_t* rows, int64_t n, int p, double* center,
               double tol, int max_iter, double* dist_out, double* info, hipStream_t st) {
#ifdef OCM_L1_FORCE_TWICE  // `make exp` A/B builds only: time the read-twice form where the tile would fit
  const int mode = L1_TWICE;
#else
  const int mode = (size_t)L1_TILE * p * sizeof(T) <= L1_TILE_BYTES ? L1_RESIDENT : L1_TWICE;
#endif
  const int64_t nchunks = (n + L1_ROWS - 1) / L1_ROWS;
  const int64_t ngroups = nchunks > L1_FANIN ? (nchunks + L1_FANIN - 1) / L1_FANIN : 0;
  const int stride = p + 3;
  const int ncolt = (stride + 255) / 256;
  OCM_REQUIRE(ngroups * ncolt < (1LL << 31), "ocm_l1median: n × p too large for one call");
  auto* w = static_cast<double*>(
      ocm::workspace(ctx, (size_t)((nchunks + ngroups + 1) * stride + 8) * sizeof(double), st));
  if (!w) return OCM_ERR_NOMEM;
  double* part = w;
  double* grp = part + nchunks * stride;
  double* sfin = grp + ngroups * stride;
  const double* src = ngroups ? grp : part;
  const int64_t count = ngroups ? ngroups : nchunks;
  OCM_HIP(hipMemsetAsync(info, 0, OCM_L1_INFO * sizeof(double), st));
  const size_t lds = l1_lds_bytes<T>(p, mode);
  for (int it = 0; it < max_iter; ++it) {
    int rc;
    if (mode == L1_RESIDENT)
      rc = launch_part<T, VEC, L1_RESIDENT>(ctx, lds, nchunks, st, X, ldx, rows, n, p, center, info, part, nullptr,
                                            it == 0);
    else
      rc = launch_part<T, VEC, L1_TWICE>(ctx, lds, nchunks, st, X, ldx, rows, n, p, center, info, part, nullptr,
                                         it == 0);
    if (rc != OCM_OK) return rc;
    if (ngroups) {
      hipLaunchKernelGGL(k_l1_group, dim3((unsigned)(ngroups * ncolt)), dim3(256), 0, st, part, nchunks, stride, 0,
                         ncolt, info, 1, grp);
      OCM_CHECK_LAUNCH("k_l1_group");
    }
    hipLaunchKernelGGL(k_l1_update, dim3(1), dim3(L1_UNT), 0, st, src, count, p, center, sfin, info, tol, it);
    OCM_CHECK_LAUNCH("k_l1_update");
  }
  // the distances, the objective and η at the returned centre
  const int rc = launch_part<T, VEC, L1_DIST>(ctx, l1_lds_bytes<T>(p, L1_DIST), nchunks, st, X, ldx, rows, n, p,
                                              center, info, part, dist_out, false);
  if (rc != OCM_OK) return rc;
  if (ngroups) {
    hipLaunchKernelGGL(k_l1_group, dim3((unsigned)ngroups), dim3(256), 0, st, part, nchunks, stride, p, 1, info, 0,
                       grp);
    OCM_CHECK_LAUNCH("k_l1_group");
  }
  hipLaunchKernelGGL(k_l1_final, dim3(1), dim3(64), 0, st, src, count, p, info);
  OCM_CHECK_LAUNCH("k_l1_final");
  return OCM_OK;
}

// the widest load p, the row pitches and the bases allow, 16 bytes at the most
template <typename T>
int pick_vec(int p, int64_t ldx, const void* X, int64_t ldu = 0, const void* U = nullptr) {
  int vec = 16 / (int)sizeof(T);
  while (vec > 1 && !(p % vec == 0 && ldx % vec == 0 && aligned_to(X, sizeof(T) * vec) && ldu % vec == 0 &&
                      aligned_to(U, sizeof(T) * vec)))
    vec >>= 1;
  return vec;
}

template <typename T>
int l1median(ocm_ctx* ctx, const T* X, int64_t ldx, const int64_t* rows, int64_t n, int p, double* center,
             double tol, int max_iter, double* dist_out, double* info, hipStream_t st) {
  const int vec = pick_vec<T>(p, ldx, X);
  if (vec == 4) {
    if constexpr (sizeof(T) == 4)
      return l1median_v<T, 4>(ctx, X, ldx, rows, n, p, center, tol, max_iter, dist_out, info, st);
  }
  if (vec == 2) return l1median_v<T, 2>(ctx, X, ldx, rows, n, p, center, tol, max_iter, dist_out, info, st);
  return l1median_v<T, 1>(ctx, X, ldx, rows, n, p, center, tol, max_iter, dist_out, info, st);
}

template <typename T>
int sphere_rows(ocm_ctx* ctx, const T* X, int64_t ldx, const int64_t* rows, int64_t n, int p, const double* center,
                T* U, int64_t ldu, double* dist_out, hipStream_t st) {
  const int vec = pick_vec<T>(p, ldx, X, ldu, U);
  const dim3 grid((unsigned)((n + 3) / 4));
#define OCM_SPH(V_) \
  hipLaunchKernelGGL((k_sphere_rows<T, V_>), grid, dim3(256), 0, st, X, ldx, rows, n, p, center, U, ldu, dist_out)
  if (vec == 4) {
    if constexpr (sizeof(T) == 4) OCM_SPH(4);
  } else if (vec == 2) {
    OCM_SPH(2);
  } else {
    OCM_SPH(1);
  }
#undef OCM_SPH
  OCM_CHECK_LAUNCH("k_sphere_rows");
  return OCM_OK;
}

}  // namespace

extern "C" {

#define OCM_L1_CHECKS(name)                                                                      \
  OCM_REQUIRE(ctx && X && center && info_out, name ": NULL argument");                           \
  OCM_REQUIRE(n >= 1 && n < (1LL << 31), name ": bad shape (1 <= n < 2^31)");                    \
  OCM_REQUIRE(p > 0 && ldx >= p, name ": bad shape (p > 0, ldx >= p)");                          \
  OCM_REQUIRE(tol >= 0.0, name ": tol must be >= 0");                                            \
  OCM_REQUIRE(max_iter >= 0 && max_iter <= 100000, name ": max_iter must lie in [0, 100000]")

int ocm_l1median_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                     double* center, double tol, int32_t max_iter, double* dist_out, double* info_out,
                     void* stream) {
  OCM_L1_CHECKS("ocm_l1median_f32");
  return l1median<float>(ctx, X, ldx, rows, n, p, center, tol, max_iter, dist_out, info_out, (hipStream_t)stream);
}

int ocm_l1median_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                     double* center, double tol, int32_t max_iter, double* dist_out, double* info_out,
                     void* stream) {
  OCM_L1_CHECKS("ocm_l1median_f64");
  return l1median<double>(ctx, X, ldx, rows, n, p, center, tol, max_iter, dist_out, info_out,
                          (hipStream_t)stream);
}

#undef OCM_L1_CHECKS

#define OCM_SPHERE_CHECKS(name)                                                                  \
  OCM_REQUIRE(ctx && X && center && U, name ": NULL argument");                                  \
  OCM_REQUIRE(n >= 1 && n < (1LL << 31), name ": bad shape (1 <= n < 2^31)");                    \
  OCM_REQUIRE(p > 0 && ldx >= p && ldu >= p, name ": bad shape (p > 0, ldx >= p, ldu >= p)")

int ocm_sphere_rows_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        const double* center, float* U, int64_t ldu, double* dist_out, void* stream) {
  OCM_SPHERE_CHECKS("ocm_sphere_rows_f32");
  return sphere_rows<float>(ctx, X, ldx, rows, n, p, center, U, ldu, dist_out, (hipStream_t)stream);
}

int ocm_sphere_rows_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        const double* center, double* U, int64_t ldu, double* dist_out, void* stream) {
  OCM_SPHERE_CHECKS("ocm_sphere_rows_f64");
  return sphere_rows<double>(ctx, X, ldx, rows, n, p, center, U, ldu, dist_out, (hipStream_t)stream);
}

#undef OCM_SPHERE_CHECKS

}  // extern "C"
