// Fold engine kernels for class-wise SIMCA cross-validation
// (utils/CVSIMCA.py:103-269, SURVEY.md §8e "CVSIMCA").
//
// The reference refits a full SIMCA per (param combo, LV, fold) and predicts
// the held-out rows (utils/CVSIMCA.py:179-199).  Here the fold models come
// from ONE Gram pass (per-fold segments, train Gram = total − fold, fp64) and
// ONE eigensolve per fold at LV_max; every LV ≤ LV_max reuses that basis:
//   T²_LV = Σ_{j<LV} t_j² / λ_j,        Q_LV = Q_{LVmax} + Σ_{LV≤j<LVmax} t_j²
// (the leading-LV PCA of the same class matrix is the leading LV of the same
// decomposition, utils/SIMCA.py:64-70).  These kernels turn the LV_max scores
// of a row set into per-LV T²/Q (training rows: limit statistics) and into
// confusion counts for every (LV, limit set) decision at once (test rows).
#include <algorithm>
#include <vector>

#include "ocm_internal.h"

namespace {

constexpr int MAXTERM_C = 8;
constexpr int CV_MAXK = 64;

struct CombineTerms {
  const double* G[MAXTERM_C];
  const double* cs[MAXTERM_C];
  double coef[MAXTERM_C];
  int nterm;
  int accumulate;  // 1: out += Σ coef·G (out is also read), 0: out = Σ coef·G
};

__global__ __launch_bounds__(256) void k_combine(CombineTerms tm, int64_t count, double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double v = tm.accumulate ? out[e] : 0.0;
  for (int t = 0; t < tm.nterm; ++t) v += tm.coef[t] * tm.G[t][e];
  out[e] = v;
}

__global__ __launch_bounds__(256) void k_combine_cs(CombineTerms tm, int p, double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= p) return;
  double v = tm.accumulate ? out[e] : 0.0;
  for (int t = 0; t < tm.nterm; ++t) v += tm.coef[t] * tm.cs[t][e];
  out[e] = v;
}

// Row r: t (k floats, row-major m×k), q.  Per LV: T² (f64) and Q (f32), plus
// per-block moment partials {ΣT², ΣT²², ΣQ, ΣQ²} (deterministic reduction).
template <int KB>
__global__ __launch_bounds__(256) void k_cv_prefix(const float* __restrict__ T, int64_t m, int k,
                                                   const float* __restrict__ Q, const double* __restrict__ inv,
                                                   const int* __restrict__ lvs, int nlv, double* __restrict__ T2_out,
                                                   float* __restrict__ Q_out, double* __restrict__ part) {
  __shared__ double sinv[CV_MAXK];
  __shared__ int slv[CV_MAXK];
  __shared__ double sred[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < CV_MAXK) sinv[tid] = tid < k ? inv[tid] : 0.0;
  if (tid < nlv) slv[tid] = lvs[tid];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  const bool own = r < m;
  double t2sq[KB];  // t_j² (registers: every index below is compile-time)
  double qres = 0.0;
  const float* tr = T + (own ? r : 0) * k;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const double t = (own && j < k) ? (double)tr[j] : 0.0;
    t2sq[j] = t * t;
  }
  if (own) qres = (double)Q[r];
  for (int l = 0; l < nlv; ++l) {
    const int lv = slv[l];
    double t2 = 0.0, q = qres;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      if (j < lv) t2 += t2sq[j] * sinv[j];
      else q += t2sq[j];  // zero beyond k
    }
    const float qf = (float)q;
    if (own) {
      if (T2_out) T2_out[(int64_t)l * m + r] = t2;
      if (Q_out) Q_out[(int64_t)l * m + r] = qf;
    }
    if (part) {
      const double qd = own ? (double)qf : 0.0;
      double s0 = own ? t2 : 0.0, s1 = own ? t2 * t2 : 0.0, s2 = qd, s3 = qd * qd;
      s0 = wave_sum_f64(s0);
      s1 = wave_sum_f64(s1);
      s2 = wave_sum_f64(s2);
      s3 = wave_sum_f64(s3);
      if (lane == 0) {
        sred[wave][0] = s0;
        sred[wave][1] = s1;
        sred[wave][2] = s2;
        sred[wave][3] = s3;
      }
      __syncthreads();
      if (tid < 4)
        part[((int64_t)blockIdx.x * nlv + l) * 4 + tid] =
            (sred[0][tid] + sred[1][tid]) + (sred[2][tid] + sred[3][tid]);
      __syncthreads();
    }
  }
}

// stats[l][c] = Σ_blocks part[b][l][c] in a fixed order
__global__ __launch_bounds__(256) void k_cv_prefix_reduce(const double* __restrict__ part, int64_t nblk, int nlv,
                                                          double* __restrict__ stats) {
  const int l = blockIdx.x, c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double v = 0.0;
  for (int64_t b = lane; b < nblk; b += 64) v += part[(b * nlv + l) * 4 + c];
  v = wave_sum_f64(v);
  if (lane == 0) stats[l * 4 + c] = v;
}

// The decision arithmetic of the sweep, shared by every kernel that decides rows
// from LV_max scores (k_cv_counts, k_cv_objects): one row's squared scores, then
// per configuration the reduced distance d_red of its LV prefix.  A row is
// accepted when cv_dred(...) < cfg.dlim.
template <int KB>
__device__ __forceinline__ void cv_load_row(const float* __restrict__ tr, int k, bool own, double (&t2sq)[KB]) {
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const double t = (own && j < k) ? (double)tr[j] : 0.0;
    t2sq[j] = t * t;
  }
}

template <int KB>
__device__ __forceinline__ double cv_dred(const double (&t2sq)[KB], double qres, const double* sinv,
                                          const ocm_cv_config& cf) {
  double t2 = 0.0, q = qres;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j < cf.lv) t2 += t2sq[j] * sinv[j];
    else q += t2sq[j];  // zero beyond k
  }
  const double qf = (double)(float)q;
  return ocm::dred_of(cf.type, t2 * cf.t2_scale, qf * cf.q_scale);
}

// Confusion counts of every configuration over m rows; rows < m_split are
// part 0 (held-out target fold), the rest part 1 (other-class rows).
// counts[cfg][part][{TP, TN, FP, FN}] as in utils/SIMCA.py:240-245.
template <int KB>
__global__ __launch_bounds__(256) void k_cv_counts(const float* __restrict__ T, int64_t m, int k,
                                                   const float* __restrict__ Q, const double* __restrict__ inv,
                                                   const uint8_t* __restrict__ positive, int64_t m_split,
                                                   const ocm_cv_config* __restrict__ cfg, int ncfg,
                                                   unsigned long long* __restrict__ counts,
                                                   double* __restrict__ accept_out) {
  extern __shared__ unsigned int scount[];  // ncfg × 8
  __shared__ double sinv[CV_MAXK];
  const int tid = threadIdx.x;
  for (int i = tid; i < ncfg * 8; i += 256) scount[i] = 0u;
  if (tid < CV_MAXK) sinv[tid] = tid < k ? inv[tid] : 0.0;
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < m; r += (int64_t)gridDim.x * 256) {
    double t2sq[KB];
    cv_load_row<KB>(T + r * k, k, true, t2sq);
    const double qres = (double)Q[r];
    const int part = r < m_split ? 0 : 4;
    const bool pos = positive[r] != 0;
    for (int c = 0; c < ncfg; ++c) {
      const ocm_cv_config cf = cfg[c];
      const bool acc = cv_dred<KB>(t2sq, qres, sinv, cf) < cf.dlim;
      // TP: accepted positive, TN: rejected negative, FP: accepted negative, FN: rejected positive
      const int slot = acc ? (pos ? 0 : 2) : (pos ? 3 : 1);
      atomicAdd(&scount[c * 8 + part + slot], 1u);
      if (accept_out) accept_out[(int64_t)c * m + r] = acc ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  for (int i = tid; i < ncfg * 8; i += 256)
    if (scount[i]) atomicAdd(&counts[i], (unsigned long long)scount[i]);
}

// ---- per-object votes and decision sums of every configuration ------------
// (include/ocm.h, ocm_cv_objects).  Objects are runs of adjacent rows given by
// G + 1 offsets.  The rows are cut into chunks of CO_ROWS rows at multiples of
// CO_ROWS wherever the objects fall (as ocm_segsum does), one workgroup per
// chunk, one row per lane, so one object of all rows and m objects of one row
// spread over the same grid.  Per configuration a lane decides its row
// (cv_dred, the arithmetic of k_cv_counts); the rows of an object are adjacent
// lanes, a "piece" per wave:
//   votes  popcount of the accept ballot under the piece's lane mask;
//   dsum   Σ (dlim − d_red) by a segmented shuffle reduction (offsets 1, 2, 4,
//          …, 32, each step adding the lane `offset` above while it is in the
//          piece), so the piece's first lane holds the sum in a fixed tree;
// then the waves' leading pieces go through LDS and the lane that begins an
// object (or the chunk) adds the following waves' leading pieces of the same
// object in wave order.  That lane stores
//   an object inside the chunk straight to the output;
//   the part of an object that began in an earlier chunk to head[chunk];
//   the part of an object that goes on into the next chunk to tail[chunk]
// (a chunk has at most one of each), and the chunk's last lane records in
// tailg[chunk] which object, if any, has a tail there.  k_cv_objects_final
// completes those objects: tail[first] + (P_0 + … + P_15), P_j the sum of
// head[first + 1 + j], head[first + 1 + j + 16], … in chunk order.  The order of
// every sum is a function of m, the offsets and ncfg alone; no atomics.
constexpr int CO_ROWS = 256;    // rows per chunk = lanes per workgroup
constexpr int CO_WAVES = CO_ROWS / 64;
constexpr int CO_FPARTS = 16;   // waves of the final pass: interleaved head chains per object
constexpr int CO_FCFG = 64;     // configurations per workgroup of the final pass (one per lane)

// first i in [0, n) with off[i] > v (n when there is none)
__device__ __forceinline__ int64_t co_upper_bound(const int64_t* __restrict__ off, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

struct CoPartials {
  unsigned int* head_v;  // nchunks × ncfg
  unsigned int* tail_v;
  double* head_d;        // nchunks × ncfg (dsum requested)
  double* tail_d;
  int64_t* tailg;        // nchunks: the object whose tail the chunk holds, or −1
};

// Object indices are kept inside [0, G) and rows inside [0, m) whatever the
// offsets hold, so unchecked offsets that break the contract give wrong
// results, never an access outside T, Q, the outputs or the workspace.
template <int KB, bool DSUM>
__global__ __launch_bounds__(CO_ROWS) void k_cv_objects(const float* __restrict__ T, int64_t m, int k,
                                                        const float* __restrict__ Q, const double* __restrict__ inv,
                                                        const int64_t* __restrict__ off, int64_t G,
                                                        const ocm_cv_config* __restrict__ cfg, int ncfg,
                                                        unsigned int* __restrict__ votes, double* __restrict__ dsum,
                                                        CoPartials pt) {
  __shared__ double sinv[CV_MAXK];
  __shared__ long long sg_first[CO_WAVES], sg_last[CO_WAVES];
  __shared__ int s_whole[CO_WAVES];  // the wave's leading piece is the whole wave
  __shared__ unsigned int slead_v[2][CO_WAVES];
  __shared__ double slead_d[2][CO_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < CV_MAXK) sinv[tid] = tid < k ? inv[tid] : 0.0;
  const int64_t c = blockIdx.x, c0 = c * CO_ROWS, cend = c0 + CO_ROWS;
  const int64_t r = c0 + tid;
  const bool own = r < m;
  double t2sq[KB];
  cv_load_row<KB>(T + (own ? r : 0) * k, k, own, t2sq);
  const double qres = own ? (double)Q[r] : 0.0;
  // the row's object: the last g with off[g] <= r; rows past m and rows no object holds take G
  long long g = G;
  if (own) {
    const int64_t i = co_upper_bound(off, G + 1, r);
    if (i >= 1 && i <= G) g = i - 1;
  }
  // the lane's piece: lanes [start, end] of the wave hold the same object
  const long long gprev = __shfl_up(g, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || g != gprev);
  const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
  const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
  const int end = above ? __ffsll(above) - 2 : 63;
  const unsigned long long pmask = (~0ull >> (63 - end)) & (~0ull << start);
  if (lane == 0) {
    sg_first[wave] = g;
    s_whole[wave] = end == 63;
  }
  if (lane == 63) sg_last[wave] = g;
  __syncthreads();
  // the lane that stores a sum: first of its piece, of a real object, and not
  // the continuation of the previous wave's last piece
  const bool lead = lane == start && g < G && !(lane == 0 && wave > 0 && sg_last[wave - 1] == g);
  int nfollow = 0;  // following waves whose leading piece belongs to the same object
  int dest = 0;     // 0: output, 1: head[chunk], 2: tail[chunk]
  if (lead) {
    if (end == 63)
      for (int w = wave + 1; w < CO_WAVES && sg_first[w] == g; ++w) {
        ++nfollow;
        if (!s_whole[w]) break;
      }
    if (off[g] < c0) dest = 1;
    else if (off[g + 1] > cend) dest = 2;
  }
  if (tid == CO_ROWS - 1) pt.tailg[c] = (g < G && off[g] >= c0 && off[g + 1] > cend) ? g : -1;
  for (int ci = 0; ci < ncfg; ++ci) {
    const ocm_cv_config cf = cfg[ci];
    const double dred = cv_dred<KB>(t2sq, qres, sinv, cf);
    const bool acc = own && dred < cf.dlim;
    unsigned int v = (unsigned int)__popcll(__ballot(acc) & pmask);
    double d = 0.0;
    if (DSUM) {
      d = own ? cf.dlim - dred : 0.0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_down(d, o, 64);
        if (lane + o <= end) d += up;
      }
    }
    const int buf = ci & 1;  // two buffers: one barrier per configuration
    if (lane == 0) {
      slead_v[buf][wave] = v;
      if (DSUM) slead_d[buf][wave] = d;
    }
    __syncthreads();
    if (lead) {
      for (int j = 1; j <= nfollow; ++j) {
        v += slead_v[buf][wave + j];
        if (DSUM) d += slead_d[buf][wave + j];
      }
      if (dest == 0) {
        if (votes) votes[(int64_t)ci * G + g] = v;
        if (DSUM) dsum[(int64_t)ci * G + g] = d;
      } else {
        (dest == 1 ? pt.head_v : pt.tail_v)[c * ncfg + ci] = v;
        if (DSUM) (dest == 1 ? pt.head_d : pt.tail_d)[c * ncfg + ci] = d;
      }
    }
  }
}

// One workgroup per (chunk, CO_FCFG configurations): a lane owns a
// configuration, wave j the heads of chunks first + 1 + j, + 16, … of the
// object whose tail the chunk holds.
__global__ __launch_bounds__(CO_FPARTS * 64) void k_cv_objects_final(const int64_t* __restrict__ off, int64_t G,
                                                                     int ncfg, int64_t nchunks, CoPartials pt,
                                                                     unsigned int* __restrict__ votes,
                                                                     double* __restrict__ dsum) {
  __shared__ unsigned int sv[CO_FPARTS][CO_FCFG];
  __shared__ double sd[CO_FPARTS][CO_FCFG];
  const int64_t c = blockIdx.x;
  const int64_t g = pt.tailg[c];
  if (g < 0 || g >= G) return;  // the same for the whole workgroup
  const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
  const int ci = blockIdx.y * CO_FCFG + lane;
  int64_t clast = (off[g + 1] - 1) / CO_ROWS;
  if (clast > nchunks - 1) clast = nchunks - 1;
  unsigned int v = 0u;
  double d = 0.0;
  if (ci < ncfg) {
#pragma unroll 4
    for (int64_t cc = c + 1 + part; cc <= clast; cc += CO_FPARTS) {
      v += pt.head_v[cc * ncfg + ci];
      if (dsum) d += pt.head_d[cc * ncfg + ci];
    }
  }
  sv[part][lane] = v;
  sd[part][lane] = d;
  __syncthreads();
  if (part != 0 || ci >= ncfg) return;
  unsigned int hv = 0u;
  double hd = 0.0;
#pragma unroll
  for (int j = 0; j < CO_FPARTS; ++j) {
    hv += sv[j][lane];
    hd += sd[j][lane];
  }
  if (votes) votes[(int64_t)ci * G + g] = pt.tail_v[c * ncfg + ci] + hv;
  if (dsum) dsum[(int64_t)ci * G + g] = pt.tail_d[c * ncfg + ci] + hd;
}

// {TP, TN, FP, FN} of one class column of the prediction matrix
// (utils/SIMCA.py:238-245): accept[r·stride] ∈ {0, 1}, positive[r] = (y_true == class)
__global__ __launch_bounds__(256) void k_confusion(const double* __restrict__ accept, int64_t m, int64_t stride,
                                                   const uint8_t* __restrict__ positive,
                                                   unsigned long long* __restrict__ counts) {
  __shared__ unsigned int sc[4];
  if (threadIdx.x < 4) sc[threadIdx.x] = 0u;
  __syncthreads();
  unsigned int c[4] = {0u, 0u, 0u, 0u};
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += (int64_t)gridDim.x * 256) {
    const double a = accept[r * stride];
    const bool pos = positive[r] != 0;
    if (a == 1.0) ++c[pos ? 0 : 2];       // TP / FP
    else if (a == 0.0) ++c[pos ? 3 : 1];  // FN / TN
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned int v = c[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sc[i], v);
  }
  __syncthreads();
  if (threadIdx.x < 4 && sc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)sc[threadIdx.x]);
}

int combine_impl(const double* const* G_list, const double* const* colsum_list, const double* coef, int32_t nterm,
                 int32_t p, double* G_out, double* colsum_out, hipStream_t st) {
  const int64_t pp = (int64_t)p * p;
  for (int t0 = 0; t0 < nterm; t0 += MAXTERM_C) {
    CombineTerms tm{};
    tm.nterm = std::min(MAXTERM_C, nterm - t0);
    tm.accumulate = t0 > 0;
    for (int t = 0; t < tm.nterm; ++t) {
      tm.G[t] = G_list[t0 + t];
      tm.cs[t] = colsum_list ? colsum_list[t0 + t] : nullptr;
      tm.coef[t] = coef[t0 + t];
    }
    if (G_out) {
      hipLaunchKernelGGL(k_combine, dim3((unsigned)((pp + 255) / 256)), dim3(256), 0, st, tm, pp, G_out);
      OCM_CHECK_LAUNCH("k_combine");
    }
    if (colsum_out && colsum_list) {
      hipLaunchKernelGGL(k_combine_cs, dim3((p + 255) / 256), dim3(256), 0, st, tm, p, colsum_out);
      OCM_CHECK_LAUNCH("k_combine_cs");
    }
  }
  return OCM_OK;
}

}  // namespace

extern "C" {

int ocm_gram_combine(ocm_ctx* ctx, const double* const* G_list, const double* const* colsum_list,
                     const double* coef, int32_t nterm, int32_t p, double* G_out, double* colsum_out, void* stream) {
  OCM_REQUIRE(ctx && G_list && coef && nterm >= 1 && p >= 1, "ocm_gram_combine: bad argument");
  OCM_REQUIRE(G_out || colsum_out, "ocm_gram_combine: no output");
  for (int t = 0; t < nterm; ++t) {
    OCM_REQUIRE(G_list[t], "ocm_gram_combine: NULL Gram");
    OCM_REQUIRE(G_list[t] != G_out || t == 0, "ocm_gram_combine: G_out may alias only the first term");
  }
  return combine_impl(G_list, colsum_list, coef, nterm, p, G_out, colsum_out, (hipStream_t)stream);
}

int ocm_cv_prefix(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                  const int32_t* lvs, int32_t nlv, double* T2_out, float* Q_out, double* stats_out, void* stream) {
  OCM_REQUIRE(ctx && T && Q && inv_evals && lvs, "ocm_cv_prefix: NULL argument");
  OCM_REQUIRE(k >= 1 && k <= CV_MAXK && nlv >= 1 && nlv <= CV_MAXK, "ocm_cv_prefix: 1 <= k, nlv <= 64");
  for (int l = 0; l < nlv; ++l) OCM_REQUIRE(lvs[l] >= 1 && lvs[l] <= k, "ocm_cv_prefix: LV outside [1, k]");
  hipStream_t st = (hipStream_t)stream;
  if (m <= 0) {
    if (stats_out) OCM_HIP(hipMemsetAsync(stats_out, 0, (size_t)nlv * 4 * sizeof(double), st));
    return OCM_OK;
  }
  const int64_t nblk = (m + 255) / 256;
  const size_t part_n = stats_out ? (size_t)nblk * nlv * 4 : 0;
  void* w = ocm::workspace(ctx, part_n * sizeof(double) + 512 + nlv * sizeof(int), st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  double* part = stats_out ? cv.take<double>(part_n) : nullptr;
  int* dlv = cv.take<int>(nlv);
  OCM_HIP(hipMemcpyAsync(dlv, lvs, nlv * sizeof(int), hipMemcpyHostToDevice, st));
#define OCM_CV_PREFIX(KB)                                                                                        \
  hipLaunchKernelGGL(k_cv_prefix<KB>, dim3((unsigned)nblk), dim3(256), 0, st, T, m, k, Q, inv_evals, dlv, nlv, T2_out, \
                     Q_out, part)
  if (k <= 16) OCM_CV_PREFIX(16); else if (k <= 32) OCM_CV_PREFIX(32); else OCM_CV_PREFIX(64);
#undef OCM_CV_PREFIX
  OCM_CHECK_LAUNCH("k_cv_prefix");
  if (stats_out) {
    hipLaunchKernelGGL(k_cv_prefix_reduce, dim3(nlv), dim3(256), 0, st, part, nblk, nlv, stats_out);
    OCM_CHECK_LAUNCH("k_cv_prefix_reduce");
  }
  return OCM_OK;
}

int ocm_cv_counts(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                  const uint8_t* positive, int64_t m_split, const ocm_cv_config* cfg, int32_t ncfg,
                  uint64_t* counts_out, double* accept_out, void* stream) {
  OCM_REQUIRE(ctx && Q && inv_evals && positive && cfg && counts_out, "ocm_cv_counts: NULL argument");
  OCM_REQUIRE(k >= 1 && k <= CV_MAXK, "ocm_cv_counts: 1 <= k <= 64");
  OCM_REQUIRE(ncfg >= 1 && ncfg <= OCM_CV_MAXCFG, "ocm_cv_counts: 1 <= ncfg <= OCM_CV_MAXCFG");
  for (int c = 0; c < ncfg; ++c) {
    OCM_REQUIRE(cfg[c].lv >= 1 && cfg[c].lv <= k, "ocm_cv_counts: LV outside [1, k]");
    OCM_REQUIRE(cfg[c].type >= OCM_TYPE_SIM && cfg[c].type <= OCM_TYPE_DD, "ocm_cv_counts: bad decision type");
  }
  hipStream_t st = (hipStream_t)stream;
  OCM_HIP(hipMemsetAsync(counts_out, 0, (size_t)ncfg * 8 * sizeof(uint64_t), st));
  if (m <= 0) return OCM_OK;
  OCM_REQUIRE(T, "ocm_cv_counts: NULL T");
  void* w = ocm::workspace(ctx, (size_t)ncfg * sizeof(ocm_cv_config) + 256, st);
  if (!w) return OCM_ERR_NOMEM;
  auto* dcfg = static_cast<ocm_cv_config*>(w);
  // pageable source: the copy is staged before hipMemcpyAsync returns
  OCM_HIP(hipMemcpyAsync(dcfg, cfg, (size_t)ncfg * sizeof(ocm_cv_config), hipMemcpyHostToDevice, st));
  const int64_t want = (m + 255) / 256;
  const unsigned grid = (unsigned)std::min<int64_t>(want, (int64_t)ctx->num_cus * 8);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts_out);
  const size_t lds = (size_t)ncfg * 8 * sizeof(unsigned);
#define OCM_CV_COUNTS(KB)                                                                                        \
  hipLaunchKernelGGL(k_cv_counts<KB>, dim3(grid), dim3(256), lds, st, T, m, k, Q, inv_evals, positive, m_split, dcfg, \
                     ncfg, cnt, accept_out)
  if (k <= 16) OCM_CV_COUNTS(16); else if (k <= 32) OCM_CV_COUNTS(32); else OCM_CV_COUNTS(64);
#undef OCM_CV_COUNTS
  OCM_CHECK_LAUNCH("k_cv_counts");
  return OCM_OK;
}

int ocm_cv_objects(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                   const int64_t* offsets, int64_t G, const ocm_cv_config* cfg, int32_t ncfg, uint32_t* votes_out,
                   double* dsum_out, void* stream) {
  OCM_REQUIRE(ctx && cfg, "ocm_cv_objects: NULL argument");
  OCM_REQUIRE(k >= 1 && k <= CV_MAXK, "ocm_cv_objects: 1 <= k <= 64");
  OCM_REQUIRE(ncfg >= 1 && ncfg <= OCM_CV_MAXCFG, "ocm_cv_objects: 1 <= ncfg <= OCM_CV_MAXCFG");
  OCM_REQUIRE(m >= 0 && G >= 0, "ocm_cv_objects: bad shape (m >= 0, G >= 0)");
  for (int c = 0; c < ncfg; ++c) {
    OCM_REQUIRE(cfg[c].lv >= 1 && cfg[c].lv <= k, "ocm_cv_objects: LV outside [1, k]");
    OCM_REQUIRE(cfg[c].type >= OCM_TYPE_SIM && cfg[c].type <= OCM_TYPE_DD, "ocm_cv_objects: bad decision type");
  }
  if (m == 0 || G == 0) return OCM_OK;
  OCM_REQUIRE(votes_out || dsum_out, "ocm_cv_objects: no output");
  OCM_REQUIRE(T && Q && inv_evals && offsets, "ocm_cv_objects: NULL argument");
  const int64_t nchunks = (m + CO_ROWS - 1) / CO_ROWS;
  OCM_REQUIRE(nchunks < (1LL << 31), "ocm_cv_objects: m too large for one call");
  hipStream_t st = (hipStream_t)stream;
  // an object without rows belongs to no chunk: its entries are the zeros written here
  if (votes_out) OCM_HIP(hipMemsetAsync(votes_out, 0, (size_t)ncfg * G * sizeof(uint32_t), st));
  if (dsum_out) OCM_HIP(hipMemsetAsync(dsum_out, 0, (size_t)ncfg * G * sizeof(double), st));
  const size_t npart = (size_t)nchunks * ncfg;
  const size_t bytes = (size_t)ncfg * sizeof(ocm_cv_config) + (size_t)nchunks * sizeof(int64_t) +
                       2 * npart * sizeof(unsigned int) + (dsum_out ? 2 * npart * sizeof(double) : 0) + 6 * 256;
  void* w = ocm::workspace(ctx, bytes, st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  auto* dcfg = cv.take<ocm_cv_config>(ncfg);
  CoPartials pt{};
  pt.tailg = cv.take<int64_t>(nchunks);
  pt.head_v = cv.take<unsigned int>(npart);
  pt.tail_v = cv.take<unsigned int>(npart);
  if (dsum_out) {
    pt.head_d = cv.take<double>(npart);
    pt.tail_d = cv.take<double>(npart);
  }
  // pageable source: the copy is staged before hipMemcpyAsync returns
  OCM_HIP(hipMemcpyAsync(dcfg, cfg, (size_t)ncfg * sizeof(ocm_cv_config), hipMemcpyHostToDevice, st));
#define OCM_CV_OBJECTS(KB)                                                                                          \
  do {                                                                                                              \
    if (dsum_out)                                                                                                   \
      hipLaunchKernelGGL((k_cv_objects<KB, true>), dim3((unsigned)nchunks), dim3(CO_ROWS), 0, st, T, m, k, Q,       \
                         inv_evals, offsets, G, dcfg, ncfg, votes_out, dsum_out, pt);                               \
    else                                                                                                            \
      hipLaunchKernelGGL((k_cv_objects<KB, false>), dim3((unsigned)nchunks), dim3(CO_ROWS), 0, st, T, m, k, Q,      \
                         inv_evals, offsets, G, dcfg, ncfg, votes_out, dsum_out, pt);                               \
  } while (0)
  if (k <= 16) OCM_CV_OBJECTS(16); else if (k <= 32) OCM_CV_OBJECTS(32); else OCM_CV_OBJECTS(64);
#undef OCM_CV_OBJECTS
  OCM_CHECK_LAUNCH("k_cv_objects");
  if (nchunks < 2) return OCM_OK;  // one chunk: no object crosses a boundary
  hipLaunchKernelGGL(k_cv_objects_final, dim3((unsigned)nchunks, (unsigned)((ncfg + CO_FCFG - 1) / CO_FCFG)),
                     dim3(CO_FPARTS * 64), 0, st, offsets, G, ncfg, nchunks, pt, votes_out, dsum_out);
  OCM_CHECK_LAUNCH("k_cv_objects_final");
  return OCM_OK;
}

int ocm_confusion_counts(ocm_ctx* ctx, const double* accept, int64_t m, int64_t accept_stride,
                         const uint8_t* positive, uint64_t* counts_out, void* stream) {
  OCM_REQUIRE(ctx && counts_out, "ocm_confusion_counts: NULL argument");
  OCM_REQUIRE(m == 0 || (accept && positive), "ocm_confusion_counts: NULL argument");
  OCM_REQUIRE(m >= 0 && accept_stride >= 1, "ocm_confusion_counts: bad shape");
  hipStream_t st = (hipStream_t)stream;
  OCM_HIP(hipMemsetAsync(counts_out, 0, 4 * sizeof(uint64_t), st));
  if (m == 0) return OCM_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((m + 255) / 256, (int64_t)ctx->num_cus * 4);
  hipLaunchKernelGGL(k_confusion, dim3(grid), dim3(256), 0, st, accept, m, accept_stride, positive,
                     reinterpret_cast<unsigned long long*>(counts_out));
  OCM_CHECK_LAUNCH("k_confusion");
  return OCM_OK;
}

}  // extern "C"
