// Kennard–Stone and Duplex sample selection (include/ocm.h, "sample selection").
//   d2(i, j) = Σ_c w_c (z_ic − z_jc)²   in fp64, the difference form, c ascending:
//              t = z_ic − z_jc;  acc = fma(w_c·t, t, acc)
// Every kernel of this file forms d2 by that one recurrence, so a distance has the
// same bits whichever kernel or path computes it, and d2(i, j) == d2(j, i).  Plain
// fp64 VALU: the work is a chain of small dependent reductions, bound by launches
// and cache latency, not by FLOPs (no MFMA).
//
// A candidate is (value, i, j) under one total order: value descending, then i
// ascending, then j ascending.  Lanes, waves, workgroups and the reduction launches
// all compare with it, so a result does not depend on tile shape or grid size.
//
// Farthest pair: the upper triangle of the n × n pair space in 128 × 128 tiles, one
// workgroup per tile pair (block b ↔ (ti ≤ tj)), both row panels staged through LDS
// in 16-column chunks as doubles, an 8 × 8 register block per thread; one partial
// per workgroup, reduced by small follow-up launches (4096 partials per workgroup).
// d2(i, i) of a diagonal tile is 0 unless row i holds a non-finite value: that is
// the count of bad rows.
//
// Selection, small path: one workgroup, the min-distance arrays (and Z, transposed,
// when it fits) resident in LDS, every step in one launch, one __syncthreads per
// step (a thread owns its rows for the whole run).
// Selection, wide path: one launch per pick.  A launch first reduces the previous
// launch's per-workgroup partials (every workgroup for itself: the kernel boundary
// gives the visibility), applies that pick to its rows' min distances and writes its
// own partial for the next pick into the other half of a ping-pong buffer.  No
// fences, no atomics but the bad-row count, no workgroup waits for another.
// Nothing is written to order / d2 when a row is non-finite or a start index is out
// of range (the launches after the first return at once).
#include "ocm_internal.h"

namespace {

constexpr int64_t KS_NONE = INT64_MAX;
constexpr int KS_BAD_START = 1 << 30;  // added to the bad-row count for a start index outside [0, n)
constexpr int KP_TS = 128;             // pair kernel: rows per tile side
constexpr int KP_QC = 16;              // ... columns per LDS chunk
constexpr int KS_ROWS = 256;           // wide path: threads per workgroup
constexpr int KS_MAX_WG = 1024;        // ... workgroups at most (= partials every workgroup reduces)
constexpr int64_t KS_RED_CHUNK = 4096; // partials one workgroup of a reduction launch takes
constexpr size_t KS_LDS_DYN = 160 * 1024 - 2048;  // dynamic LDS the small path may take
// Auto rule (measured, DESIGN.md "Kennard–Stone and Duplex selection"): the small path exactly while Z
// fits LDS beside the min distances.  There a pick took 2.6–6.6 µs against the wide path's 6.4–8.2 µs;
// with Z read from L2 the one workgroup was slower than a launch per pick at every size measured.

struct Cand {
  double v;
  int64_t i, j;
};

__device__ __forceinline__ double ks_ninf() { return -__builtin_huge_val(); }

__device__ __forceinline__ bool better(double v, int64_t i, int64_t j, const Cand& b) {
  return v > b.v || (v == b.v && (i < b.i || (i == b.i && j < b.j)));
}

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Cand d;
    d.v = __shfl_xor(c.v, o, 64);
    d.i = (int64_t)__shfl_xor((long long)c.i, o, 64);
    d.j = (int64_t)__shfl_xor((long long)c.j, o, 64);
    if (better(d.v, d.i, d.j, c)) c = d;
  }
  return c;
}

// The workgroup's best candidate, in every thread.  scratch: 16 Cands of LDS that no
// thread touches again before the workgroup's next barrier.  blockDim.x % 64 == 0.
__device__ __forceinline__ Cand block_best(Cand c, Cand* scratch) {
  c = wave_best(c);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  if (lane == 0) scratch[wave] = c;
  __syncthreads();
  Cand d{ks_ninf(), KS_NONE, KS_NONE};
  if (lane < nw) d = scratch[lane];
  return wave_best(d);
}

template <typename T>
__device__ __forceinline__ bool finite_v(T v) {
  return fabs((double)v) < __builtin_huge_val();
}

// d2 of two rows in memory
template <typename T>
__device__ __forceinline__ double d2_rows(const T* __restrict__ a, const T* __restrict__ b,
                                          const double* __restrict__ w, int q) {
  double acc = 0.0;
  for (int c = 0; c < q; ++c) {
    const double t = (double)a[c] - (double)b[c];
    const double wc = w ? w[c] : 1.0;
    acc = fma(wc * t, t, acc);
  }
  return acc;
}

// ------------------------------------------------------------------ farthest pair

template <typename T>
__global__ __launch_bounds__(256) void k_ks_pair(const T* __restrict__ Z, int64_t ldz, int64_t n, int q,
                                                 const double* __restrict__ w, const uint8_t* __restrict__ skip,
                                                 Cand* __restrict__ part, int* __restrict__ nbad) {
  __shared__ double sA[KP_QC][KP_TS];
  __shared__ double sB[KP_QC][KP_TS];
  __shared__ double sW[KP_QC];
  __shared__ Cand sred[16];
  const int64_t b = blockIdx.x;
  int64_t tj = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while (tj > 0 && tj * (tj + 1) / 2 > b) --tj;
  while ((tj + 1) * (tj + 2) / 2 <= b) ++tj;
  const int64_t ti = b - tj * (tj + 1) / 2;
  const int64_t i0 = ti * KP_TS, j0 = tj * KP_TS;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[8][8];
#pragma unroll
  for (int ra = 0; ra < 8; ++ra)
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) acc[ra][rb] = 0.0;
  for (int c0 = 0; c0 < q; c0 += KP_QC) {
    const int nc = min(KP_QC, q - c0);
    __syncthreads();  // the previous chunk has been read
    for (int e = threadIdx.x; e < KP_TS * KP_QC; e += 256) {
      const int r = e / KP_QC, c = e % KP_QC;
      const int64_t ia = i0 + r, jb = j0 + r;
      sA[c][r] = (c < nc && ia < n) ? (double)Z[ia * ldz + c0 + c] : 0.0;
      sB[c][r] = (c < nc && jb < n) ? (double)Z[jb * ldz + c0 + c] : 0.0;
    }
    if (threadIdx.x < KP_QC) sW[threadIdx.x] = (int)threadIdx.x < nc ? (w ? w[c0 + threadIdx.x] : 1.0) : 0.0;
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      double a[8], bb[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        a[r] = sA[c][ty + 16 * r];
        bb[r] = sB[c][tx + 16 * r];
      }
      const double wc = sW[c];
#pragma unroll
      for (int ra = 0; ra < 8; ++ra)
#pragma unroll
        for (int rb = 0; rb < 8; ++rb) {
          const double t = a[ra] - bb[rb];
          acc[ra][rb] = fma(wc * t, t, acc[ra][rb]);
        }
    }
  }
  Cand best{ks_ninf(), KS_NONE, KS_NONE};
  int badc = 0;
  bool vj[8];
#pragma unroll
  for (int rb = 0; rb < 8; ++rb) {
    const int64_t j = j0 + tx + 16 * rb;
    vj[rb] = j < n && !(skip && skip[j]);
  }
#pragma unroll
  for (int ra = 0; ra < 8; ++ra) {
    const int64_t i = i0 + ty + 16 * ra;
    const bool vi = i < n && !(skip && skip[i]);
#pragma unroll
    for (int rb = 0; rb < 8; ++rb) {
      const int64_t j = j0 + tx + 16 * rb;
      if (!(vi && vj[rb])) continue;
      if (i < j) {
        if (better(acc[ra][rb], i, j, best)) best = Cand{acc[ra][rb], i, j};
      } else if (i == j && !(acc[ra][rb] == 0.0)) {
        ++badc;  // z − z is 0 for every finite z, NaN otherwise
      }
    }
  }
  if (badc) atomicAdd(nbad, badc);
  best = block_best(best, sred);
  if (threadIdx.x == 0) part[b] = best;
}

// argmin_i d2(z_i, center): the candidate value is −d2 (the order's value runs descending)
template <typename T>
__global__ __launch_bounds__(KS_ROWS) void k_ks_nearest(const T* __restrict__ Z, int64_t ldz, int64_t n, int q,
                                                        const double* __restrict__ w,
                                                        const double* __restrict__ center, Cand* __restrict__ part,
                                                        int* __restrict__ nbad) {
  __shared__ Cand sred[16];
  Cand best{ks_ninf(), KS_NONE, 0};
  int badc = 0;
  for (int64_t i = (int64_t)blockIdx.x * KS_ROWS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KS_ROWS) {
    const T* zi = Z + i * ldz;
    double acc = 0.0;
    bool fin = true;
    for (int c = 0; c < q; ++c) {
      const T z = zi[c];
      fin = fin && finite_v(z);
      const double t = (double)z - center[c];
      const double wc = w ? w[c] : 1.0;
      acc = fma(wc * t, t, acc);
    }
    badc += !fin;
    if (better(-acc, i, 0, best)) best = Cand{-acc, i, 0};
  }
  if (badc) atomicAdd(nbad, badc);
  best = block_best(best, sred);
  if (threadIdx.x == 0) part[blockIdx.x] = best;
}

// Workgroup b reduces in[b·chunk, min(count, (b + 1)·chunk)).  mode 0: → out[b]; 1: the pair search's
// last launch (idx_out = {i, j}, d2_out = value); 2: the nearest row's (idx_out = {i}, d2_out = −value).
__global__ __launch_bounds__(256) void k_ks_reduce(const Cand* __restrict__ in, int64_t count, int64_t chunk,
                                                   Cand* __restrict__ out, int64_t* __restrict__ idx_out,
                                                   double* __restrict__ d2_out, int mode) {
  __shared__ Cand sred[16];
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = lo + chunk < count ? lo + chunk : count;
  Cand best{ks_ninf(), KS_NONE, KS_NONE};
  for (int64_t k = lo + threadIdx.x; k < hi; k += 256) {
    const Cand c = in[k];
    if (better(c.v, c.i, c.j, best)) best = c;
  }
  best = block_best(best, sred);
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    out[blockIdx.x] = best;
    return;
  }
  const bool none = best.i == KS_NONE;
  idx_out[0] = none ? -1 : best.i;
  if (mode == 1) idx_out[1] = none ? -1 : best.j;
  d2_out[0] = none ? __builtin_nan("") : (mode == 1 ? best.v : -best.v);
}

// partials → result: launches of KS_RED_CHUNK partials per workgroup until one workgroup is left
int reduce_partials(Cand* part, Cand* part2, int64_t count, int64_t* idx_out, double* d2_out, int mode,
                    hipStream_t st) {
  Cand *cur = part, *other = part2;
  while (count > KS_RED_CHUNK) {
    const int64_t nb = (count + KS_RED_CHUNK - 1) / KS_RED_CHUNK;
    hipLaunchKernelGGL(k_ks_reduce, dim3((unsigned)nb), dim3(256), 0, st, cur, count, KS_RED_CHUNK, other,
                       (int64_t*)nullptr, (double*)nullptr, 0);
    OCM_CHECK_LAUNCH("k_ks_reduce");
    std::swap(cur, other);
    count = nb;
  }
  hipLaunchKernelGGL(k_ks_reduce, dim3(1), dim3(256), 0, st, cur, count, count, (Cand*)nullptr, idx_out, d2_out,
                     mode);
  OCM_CHECK_LAUNCH("k_ks_reduce");
  return OCM_OK;
}

template <typename T>
int run_pair(ocm_ctx* ctx, const T* Z, int64_t ldz, int64_t n, int q, const double* w, const uint8_t* skip,
             int64_t* pair_out, double* d2_out, int* nbad_out, hipStream_t st, const char* who) {
  OCM_REQUIRE(ctx && Z && pair_out && d2_out && nbad_out, std::string(who) + ": NULL argument");
  OCM_REQUIRE(n >= 2 && q >= 1 && ldz >= q, std::string(who) + ": bad shape (n >= 2, q >= 1, ldz >= q)");
  OCM_REQUIRE(n < (1LL << 31), std::string(who) + ": n must be below 2^31");
  const int64_t tiles = (n + KP_TS - 1) / KP_TS;
  const int64_t npair = tiles * (tiles + 1) / 2;  // tiles ≤ 2^24: no overflow
  OCM_REQUIRE(npair <= 2147483647LL, std::string(who) + ": too many rows for one launch (tile pairs exceed the grid limit)");
  const int64_t n2 = (npair + KS_RED_CHUNK - 1) / KS_RED_CHUNK;
  char* ws = static_cast<char*>(ocm::workspace(ctx, ocm::align_up((size_t)npair * sizeof(Cand), 256) +
                                                        (size_t)n2 * sizeof(Cand), st));
  if (!ws) return OCM_ERR_NOMEM;
  Cand* part = reinterpret_cast<Cand*>(ws);
  Cand* part2 = reinterpret_cast<Cand*>(ws + ocm::align_up((size_t)npair * sizeof(Cand), 256));
  OCM_HIP(hipMemsetAsync(nbad_out, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_ks_pair<T>, dim3((unsigned)npair), dim3(256), 0, st, Z, ldz, n, q, w, skip, part, nbad_out);
  OCM_CHECK_LAUNCH("k_ks_pair");
  return reduce_partials(part, part2, npair, pair_out, d2_out, 1, st);
}

template <typename T>
int run_nearest(ocm_ctx* ctx, const T* Z, int64_t ldz, int64_t n, int q, const double* w, const double* center,
                int64_t* idx_out, double* d2_out, int* nbad_out, hipStream_t st, const char* who) {
  OCM_REQUIRE(ctx && Z && center && idx_out && d2_out && nbad_out, std::string(who) + ": NULL argument");
  OCM_REQUIRE(n >= 1 && q >= 1 && ldz >= q, std::string(who) + ": bad shape (n >= 1, q >= 1, ldz >= q)");
  OCM_REQUIRE(n < (1LL << 31), std::string(who) + ": n must be below 2^31");
  const int64_t need = (n + KS_ROWS - 1) / KS_ROWS;
  const int grid = (int)(need < KS_MAX_WG ? need : KS_MAX_WG);
  Cand* part = static_cast<Cand*>(ocm::workspace(ctx, (size_t)grid * sizeof(Cand), st));
  if (!part) return OCM_ERR_NOMEM;
  OCM_HIP(hipMemsetAsync(nbad_out, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_ks_nearest<T>, dim3(grid), dim3(KS_ROWS), 0, st, Z, ldz, n, q, w, center, part, nbad_out);
  OCM_CHECK_LAUNCH("k_ks_nearest");
  return reduce_partials(part, nullptr, grid, idx_out, d2_out, 2, st);
}

// ------------------------------------------------------------------ selection

struct KsArgs {
  const void* Z;
  int64_t ldz, n;
  int q;
  const double* w;
  const int64_t* start[2];
  int64_t ns[2];    // start indices per set
  int64_t nsel[2];  // set sizes; nsel[1] == 0: Kennard–Stone, one set
  int64_t* order[2];
  double* d2[2];
  int* nbad;
};

// Step t of the run picks for `set` its element ns[set] + pos: the sets take turns, A first, a full set
// is skipped.  ra, rb: picks the sets still take after their starts.
__host__ __device__ __forceinline__ void step_slot(int64_t t, int64_t ra, int64_t rb, int& set, int64_t& pos) {
  const int64_t mn = ra < rb ? ra : rb;
  if (t < 2 * mn) {
    set = (int)(t & 1);
    pos = t >> 1;
  } else {
    set = ra > rb ? 0 : 1;
    pos = t - mn;
  }
}

// the starts of both sets go to order, their d2 is NaN
__device__ __forceinline__ void write_starts(const KsArgs& a) {
  for (int s = 0; s < 2; ++s)
    for (int64_t k = threadIdx.x; k < a.ns[s]; k += blockDim.x) {
      a.order[s][k] = a.start[s][k];
      a.d2[s][k] = __builtin_nan("");
    }
}

template <typename T, bool ZLDS>
__global__ __launch_bounds__(1024) void k_ks_small(const KsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ks_dyn[];
  __shared__ Cand sred[2][16];
  __shared__ int sbad;
  const int n = (int)a.n, q = a.q, tid = threadIdx.x, nt = blockDim.x;
  const bool two = a.nsel[1] > 0;
  double* m0 = reinterpret_cast<double*>(ks_dyn);
  double* m1 = two ? m0 + n : m0;
  T* Zs = reinterpret_cast<T*>(m0 + (two ? 2 : 1) * (size_t)n);
  const T* __restrict__ Zg = static_cast<const T*>(a.Z);
  const double* __restrict__ w = a.w;
  const int64_t ldz = a.ldz;
  if (tid == 0) sbad = 0;
  if constexpr (ZLDS) {
    for (int64_t e = tid; e < (int64_t)n * q; e += nt) {
      const int i = (int)(e / q), c = (int)(e % q);
      Zs[(size_t)c * n + i] = Zg[i * ldz + c];
    }
  }
  __syncthreads();
  auto zat = [&](int i, int c) -> double {
    if constexpr (ZLDS)
      return (double)Zs[(size_t)c * n + i];
    else
      return (double)Zg[i * ldz + c];
  };
  auto dist = [&](int i, int p) -> double {
    double acc = 0.0;
    for (int c = 0; c < q; ++c) {
      const double t = zat(i, c) - zat(p, c);
      const double wc = w ? w[c] : 1.0;
      acc = fma(wc * t, t, acc);
    }
    return acc;
  };
  // min distances to the starts; non-finite rows and start indices out of range are counted
  int bad = 0;
  for (int i = tid; i < n; i += nt) {
    bool fin = true;
    for (int c = 0; c < q; ++c) fin = fin && finite_v(zat(i, c));
    bad += !fin;
    bool marked = false;
    for (int s = 0; s < (two ? 2 : 1); ++s) {
      double mm = __builtin_huge_val();
      for (int64_t k = 0; k < a.ns[s]; ++k) {
        const int64_t p = a.start[s][k];
        if (p < 0 || p >= n) continue;
        marked = marked || p == i;
        const double d = dist(i, (int)p);
        if (d < mm) mm = d;
      }
      (s ? m1 : m0)[i] = mm;
    }
    if (marked) {
      m0[i] = -1.0;
      m1[i] = -1.0;
    }
  }
  if (tid == 0) {
    for (int s = 0; s < 2; ++s)
      for (int64_t k = 0; k < a.ns[s]; ++k)
        if (a.start[s][k] < 0 || a.start[s][k] >= n) bad += KS_BAD_START;
  }
  if (bad) atomicAdd(&sbad, bad);
  __syncthreads();
  const int nb = sbad;
  if (tid == 0) *a.nbad = nb;
  if (nb) return;
  write_starts(a);
  const int64_t ra = a.nsel[0] - a.ns[0], rb = two ? a.nsel[1] - a.ns[1] : 0, steps = ra + rb;
  for (int64_t t = 0; t < steps; ++t) {
    int set;
    int64_t pos;
    step_slot(t, ra, rb, set, pos);
    double* ms = set ? m1 : m0;
    Cand best{ks_ninf(), KS_NONE, 0};
    for (int i = tid; i < n; i += nt) {
      const double v = ms[i];
      if (v >= 0.0 && better(v, i, 0, best)) best = Cand{v, i, 0};
    }
    best = block_best(best, sred[t & 1]);
    if (best.i == KS_NONE) return;  // no unassigned row is left (the host checks the sizes)
    const int p = (int)best.i;
    if (tid == 0) {
      a.order[set][a.ns[set] + pos] = p;
      a.d2[set][a.ns[set] + pos] = best.v;
    }
    for (int i = tid; i < n; i += nt) {
      if (i == p) {
        m0[i] = -1.0;
        m1[i] = -1.0;
      } else {
        const double v = ms[i];
        if (v >= 0.0) {
          const double d = dist(i, p);
          if (d < v) ms[i] = d;
        }
      }
    }
  }
}

// wide path, first launch: the min distances to the starts, the bad-row count, the partial of step 0
template <typename T>
__global__ __launch_bounds__(KS_ROWS) void k_ks_init(const KsArgs a, double* __restrict__ m0, double* __restrict__ m1,
                                                     Cand* __restrict__ part_out, int set0) {
  __shared__ Cand sred[16];
  const T* __restrict__ Z = static_cast<const T*>(a.Z);
  const int64_t n = a.n, ldz = a.ldz;
  const int q = a.q;
  const bool two = a.nsel[1] > 0;
  Cand best{ks_ninf(), KS_NONE, 0};
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * KS_ROWS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KS_ROWS) {
    const T* zi = Z + i * ldz;
    bool fin = true;
    for (int c = 0; c < q; ++c) fin = fin && finite_v(zi[c]);
    bad += !fin;
    bool marked = false;
    double mv[2] = {0.0, 0.0};
    for (int s = 0; s < (two ? 2 : 1); ++s) {
      double mm = __builtin_huge_val();
      for (int64_t k = 0; k < a.ns[s]; ++k) {
        const int64_t p = a.start[s][k];
        if (p < 0 || p >= n) continue;
        marked = marked || p == i;
        const double d = d2_rows(zi, Z + p * ldz, a.w, q);
        if (d < mm) mm = d;
      }
      mv[s] = mm;
    }
    if (marked) mv[0] = mv[1] = -1.0;
    m0[i] = mv[0];
    if (two) m1[i] = mv[1];
    const double cand = mv[two ? set0 : 0];
    if (cand >= 0.0 && better(cand, i, 0, best)) best = Cand{cand, i, 0};
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int s = 0; s < 2; ++s)
      for (int64_t k = 0; k < a.ns[s]; ++k)
        if (a.start[s][k] < 0 || a.start[s][k] >= n) bad += KS_BAD_START;
  }
  if (bad) atomicAdd(a.nbad, bad);
  best = block_best(best, sred);
  if (threadIdx.x == 0) part_out[blockIdx.x] = best;
}

// wide path, one launch per pick: find the previous step's pick from its npart partials, record it
// (workgroup 0), apply it to this workgroup's rows and write the partial of the current step.
// prev / cur: the sets of the two steps (m of set s: s ? m1 : m0; m1 NULL with one set).
template <typename T>
__global__ __launch_bounds__(KS_ROWS) void k_ks_step(const T* __restrict__ Z, int64_t ldz, int64_t n, int q,
                                                     const double* __restrict__ w, double* m0, double* m1,
                                                     int prev, int cur,
                                                     const Cand* __restrict__ part_in, int npart,
                                                     Cand* __restrict__ part_out, int64_t* __restrict__ order_slot,
                                                     double* __restrict__ d2_slot, const int* __restrict__ nbad) {
  __shared__ Cand sred[2][16];
  if (*nbad) return;
  Cand pk{ks_ninf(), KS_NONE, 0};
  for (int k = threadIdx.x; k < npart; k += KS_ROWS) {
    const Cand c = part_in[k];
    if (better(c.v, c.i, c.j, pk)) pk = c;
  }
  pk = block_best(pk, sred[0]);
  const int64_t p = pk.i;
  if (p < 0 || p >= n) return;  // no unassigned row was left (the host checks the sizes)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *order_slot = p;
    *d2_slot = pk.v;
  }
  double* mp = prev ? m1 : m0;
  const double* mc = cur ? m1 : m0;
  const T* zp = Z + p * ldz;
  Cand best{ks_ninf(), KS_NONE, 0};
  for (int64_t i = (int64_t)blockIdx.x * KS_ROWS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KS_ROWS) {
    double cand;
    if (i == p) {
      m0[i] = -1.0;
      if (m1) m1[i] = -1.0;
      cand = -1.0;
    } else {
      double v = mp[i];
      if (v >= 0.0) {
        const double d = d2_rows(Z + i * ldz, zp, w, q);
        if (d < v) {
          v = d;
          mp[i] = d;
        }
      }
      cand = cur == prev ? v : mc[i];
    }
    if (cand >= 0.0 && better(cand, i, 0, best)) best = Cand{cand, i, 0};
  }
  best = block_best(best, sred[1]);
  if (threadIdx.x == 0) part_out[blockIdx.x] = best;
}

// wide path, last launch: the last pick (has_pick) and the starts
__global__ __launch_bounds__(KS_ROWS) void k_ks_final(const KsArgs a, const Cand* __restrict__ part_in, int npart,
                                                      int has_pick, int64_t* __restrict__ order_slot,
                                                      double* __restrict__ d2_slot) {
  __shared__ Cand sred[16];
  if (*a.nbad) return;
  write_starts(a);
  if (!has_pick) return;
  Cand pk{ks_ninf(), KS_NONE, 0};
  for (int k = threadIdx.x; k < npart; k += KS_ROWS) {
    const Cand c = part_in[k];
    if (better(c.v, c.i, c.j, pk)) pk = c;
  }
  pk = block_best(pk, sred);
  if (threadIdx.x == 0 && pk.i != KS_NONE) {
    *order_slot = pk.i;
    *d2_slot = pk.v;
  }
}

template <typename T, bool ZLDS>
int launch_small(ocm_ctx* ctx, const KsArgs& a, size_t dyn, hipStream_t st) {
  auto kern = k_ks_small<T, ZLDS>;
  static int lds_ok[64] = {0};  // per device: the attribute is set once per kernel, for the whole LDS
  if (!lds_ok[ctx->device & 63]) {
    OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)KS_LDS_DYN));
    lds_ok[ctx->device & 63] = 1;
  }
  const int64_t nt = (a.n + 63) / 64 * 64;
  hipLaunchKernelGGL(kern, dim3(1), dim3((unsigned)(nt < 1024 ? nt : 1024)), dyn, st, a);
  OCM_CHECK_LAUNCH("k_ks_small");
  return OCM_OK;
}

template <typename T>
int run_select(ocm_ctx* ctx, const T* Z, int64_t ldz, int64_t n, int q, const double* w, const int64_t* start_a,
               int64_t ns_a, int64_t n_a, const int64_t* start_b, int64_t ns_b, int64_t n_b, int64_t* order_a,
               double* d2_a, int64_t* order_b, double* d2_b, int* nbad_out, int path, hipStream_t st,
               const char* who) {
  const std::string me(who);
  OCM_REQUIRE(ctx && Z && start_a && order_a && d2_a && nbad_out, me + ": NULL argument");
  OCM_REQUIRE(n >= 1 && q >= 1 && ldz >= q && n < (1LL << 31), me + ": bad shape (1 <= n < 2^31, q >= 1, ldz >= q)");
  OCM_REQUIRE(ns_a >= 1 && ns_a <= n_a, me + ": set A needs 1 <= n_start <= n_select");
  OCM_REQUIRE(n_b >= 0, me + ": n_b must be >= 0");
  if (n_b > 0) {
    OCM_REQUIRE(start_b && order_b && d2_b, me + ": NULL argument (set B)");
    OCM_REQUIRE(ns_b >= 1 && ns_b <= n_b, me + ": set B needs 1 <= n_start <= n_select");
  }
  OCM_REQUIRE(n_a + n_b <= n, me + ": the sets take more rows than there are");
  OCM_REQUIRE(path >= 0 && path <= 2, me + ": path must be 0 (auto), 1 (small) or 2 (wide)");
  const int nsets = n_b > 0 ? 2 : 1;
  KsArgs a{};
  a.Z = Z, a.ldz = ldz, a.n = n, a.q = q, a.w = w, a.nbad = nbad_out;
  a.start[0] = start_a, a.ns[0] = ns_a, a.nsel[0] = n_a, a.order[0] = order_a, a.d2[0] = d2_a;
  a.start[1] = start_b, a.ns[1] = n_b > 0 ? ns_b : 0, a.nsel[1] = n_b, a.order[1] = order_b, a.d2[1] = d2_b;
  const size_t m_bytes = (size_t)nsets * (size_t)n * sizeof(double);
  const size_t z_bytes = (size_t)n * (size_t)q * sizeof(T);
  const bool small_ok = m_bytes <= KS_LDS_DYN;
  const bool z_fits = small_ok && (size_t)q <= (KS_LDS_DYN - m_bytes) / sizeof(T) / (size_t)n;
  OCM_REQUIRE(path != 1 || small_ok, me + ": the small path needs the min-distance arrays to fit LDS");
  const bool small = path == 1 || (path == 0 && z_fits);
  if (small) {
    if (z_fits) return launch_small<T, true>(ctx, a, m_bytes + z_bytes, st);
    return launch_small<T, false>(ctx, a, m_bytes, st);
  }
  const int64_t need = (n + KS_ROWS - 1) / KS_ROWS;
  const int grid = (int)(need < KS_MAX_WG ? need : KS_MAX_WG);
  const size_t mb = ocm::align_up((size_t)n * sizeof(double), 256);
  char* ws = static_cast<char*>(ocm::workspace(ctx, nsets * mb + 2 * ocm::align_up(grid * sizeof(Cand), 256), st));
  if (!ws) return OCM_ERR_NOMEM;
  double* m0 = reinterpret_cast<double*>(ws);
  double* m1 = nsets == 2 ? reinterpret_cast<double*>(ws + mb) : nullptr;
  Cand* part[2];
  part[0] = reinterpret_cast<Cand*>(ws + nsets * mb);
  part[1] = reinterpret_cast<Cand*>(ws + nsets * mb + ocm::align_up(grid * sizeof(Cand), 256));
  const int64_t ra = n_a - ns_a, rb = n_b > 0 ? n_b - ns_b : 0, steps = ra + rb;
  OCM_HIP(hipMemsetAsync(nbad_out, 0, sizeof(int), st));
  int set = 0, prev = 0;
  int64_t pos = 0;
  if (steps > 0) step_slot(0, ra, rb, set, pos);
  hipLaunchKernelGGL(k_ks_init<T>, dim3(grid), dim3(KS_ROWS), 0, st, a, m0, m1, part[0], set);
  OCM_CHECK_LAUNCH("k_ks_init");
  for (int64_t t = 1; t <= steps; ++t) {
    prev = set;
    int64_t* oslot = a.order[prev] + a.ns[prev] + pos;
    double* dslot = a.d2[prev] + a.ns[prev] + pos;
    if (t == steps) {
      hipLaunchKernelGGL(k_ks_final, dim3(1), dim3(KS_ROWS), 0, st, a, part[(t - 1) & 1], grid, 1, oslot, dslot);
      OCM_CHECK_LAUNCH("k_ks_final");
      break;
    }
    step_slot(t, ra, rb, set, pos);
    hipLaunchKernelGGL(k_ks_step<T>, dim3(grid), dim3(KS_ROWS), 0, st, Z, ldz, n, q, w, m0, m1, prev, set,
                       part[(t - 1) & 1], grid, part[t & 1], oslot, dslot, nbad_out);
    OCM_CHECK_LAUNCH("k_ks_step");
  }
  if (steps == 0) {
    hipLaunchKernelGGL(k_ks_final, dim3(1), dim3(KS_ROWS), 0, st, a, part[0], grid, 0, (int64_t*)nullptr,
                       (double*)nullptr);
    OCM_CHECK_LAUNCH("k_ks_final");
  }
  return OCM_OK;
}

}  // namespace

extern "C" {

int ocm_ks_pair_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                    const uint8_t* skip, int64_t* pair_out, double* d2_out, int32_t* nbad_out, void* stream) {
  return run_pair<float>(ctx, Z, ldz, n, q, w, skip, pair_out, d2_out, nbad_out, (hipStream_t)stream,
                         "ocm_ks_pair_f32");
}

int ocm_ks_pair_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                    const uint8_t* skip, int64_t* pair_out, double* d2_out, int32_t* nbad_out, void* stream) {
  return run_pair<double>(ctx, Z, ldz, n, q, w, skip, pair_out, d2_out, nbad_out, (hipStream_t)stream,
                          "ocm_ks_pair_f64");
}

int ocm_ks_nearest_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                       const double* center, int64_t* idx_out, double* d2_out, int32_t* nbad_out, void* stream) {
  return run_nearest<float>(ctx, Z, ldz, n, q, w, center, idx_out, d2_out, nbad_out, (hipStream_t)stream,
                            "ocm_ks_nearest_f32");
}

int ocm_ks_nearest_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                       const double* center, int64_t* idx_out, double* d2_out, int32_t* nbad_out, void* stream) {
  return run_nearest<double>(ctx, Z, ldz, n, q, w, center, idx_out, d2_out, nbad_out, (hipStream_t)stream,
                             "ocm_ks_nearest_f64");
}

int ocm_ks_select_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                      const int64_t* start_a, int64_t n_start_a, int64_t n_a, const int64_t* start_b,
                      int64_t n_start_b, int64_t n_b, int64_t* order_a, double* d2_a, int64_t* order_b, double* d2_b,
                      int32_t* nbad_out, int32_t path, void* stream) {
  return run_select<float>(ctx, Z, ldz, n, q, w, start_a, n_start_a, n_a, start_b, n_start_b, n_b, order_a, d2_a,
                           order_b, d2_b, nbad_out, path, (hipStream_t)stream, "ocm_ks_select_f32");
}

int ocm_ks_select_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                      const int64_t* start_a, int64_t n_start_a, int64_t n_a, const int64_t* start_b,
                      int64_t n_start_b, int64_t n_b, int64_t* order_a, double* d2_a, int64_t* order_b, double* d2_b,
                      int32_t* nbad_out, int32_t path, void* stream) {
  return run_select<double>(ctx, Z, ldz, n, q, w, start_a, n_start_a, n_a, start_b, n_start_b, n_b, order_a, d2_a,
                            order_b, d2_b, nbad_out, path, (hipStream_t)stream, "ocm_ks_select_f64");
}

}  // extern "C"
