// Multi-class SIMCA scoring (include/ocm.h, "multi-class SIMCA"): T², Q, the
// reduced distance and the decision of every processed row against C class
// models, and the class assignment, in one launch.
//
// Reference math: utils/SIMCA.py:120-145 (predict loops over the classes and
// scores X once per class); per class c, with y = x − μ_c, t = P_c·y and
// a = diag(1/λ) (utils/SIMCA.py:67-71):  Q_c = ‖y − P_cᵀt‖²,  T²_c = Σ t²·a,
// dred_c as k_decide forms it (ocm_score.hip), accept_c = dred_c < dlim_c,
// ratio_c = dred_c / dlim_c.
//
// k_score_multi: k_contrib's tiling (ocm_contrib.hip) with a loop over the
// classes inside the tile.  One workgroup of four waves per 16-row tile,
// persistent over the tiles, two workgroups per CU.  The first sweep of the
// first class reads the tile's rows from HBM and, where 16 × p floats fit
// beside the static arrays in half a CU's LDS (p ≤ ≈ 1100), leaves the raw
// rows there: every later sweep of every class reads them from LDS, so X
// leaves HBM once for all classes.  For wider rows the later sweeps read the
// tile's rows again through the cache hierarchy (64 – 128 KiB after they were
// first read), as k_contrib's sweep 2 does.  The waves split the columns in
// blocks of MS_CHAIN.  Per class:
//   sweep 1  Tᵀ (comps × rows) += P_chunk · Y_chunkᵀ on 16x16x4 f32 MFMA, f32
//            partials over MS_CHAIN columns, flushed to f64; the four waves'
//            partial t meet in LDS (f64, fixed order);
//   sweep 2  the explicit f32 residual e = y − t·P per 64-column block (rows ×
//            cols: A = t of row l&15, B = the loadings of the lane's column),
//            e² summed over the lane's four columns in f32, then in f64 over
//            the blocks, the 16 column lanes and the waves (fixed order);
//            the first wave forms T² = Σ t²·a (f64, from the t in LDS) meanwhile.
// The classes' partial Q and T² wait in LDS for the end of the tile:
//   decide   thread (class c, row r): Q, dred, accept, ratio and their stores;
//   assign   thread r < 16 owns row r: nearest, index, n_accept, the counters.
// The mean is kept as a float pair (hi + lo): y = (x − hi) − lo carries two
// roundings of y whatever the size of the mean.
// Counts: LDS counters per workgroup over all its tiles, one 64-bit integer
// atomic per non-zero counter at the end (integers: the order is free).  No
// floating-point atomics, no workgroup waits for another: a launch's outputs
// depend on its arguments only.
#include "ocm_internal.h"

#include <algorithm>

namespace {

constexpr int MS_W = 4;        // waves per workgroup
constexpr int MS_R = 16;       // rows per tile
constexpr int MS_CHAIN = 64;   // columns of one f32 accumulation chain (a wave's block), then fp64
constexpr int MS_MAXC = 8;     // classes
constexpr int MS_MAXK = 64;    // stacked components
constexpr int MS_WPC = 2;      // workgroups per CU
constexpr int MS_LDS_BYTES = 160 * 1024;
constexpr int MS_NCNT = (MS_MAXC + 1) * (3 * MS_MAXC + 2);  // counters of the largest C

struct MsDec {
  int type;
  double t2_scale, q_scale, dlim;
};
struct MsArgs {
  int koff[MS_MAXC + 1];
  MsDec dec[MS_MAXC];
};

// static LDS of k_score_multi<KT, *> (the rest is the row tile)
constexpr int multi_static_lds(int kt) { return MS_W * kt * 16 * MS_R * 8 + MS_MAXC * 32 + MS_NCNT * 4 + 64; }
// dynamic LDS behind the row tile: per class the waves' partial Q ([MS_W][MS_R] f64) and T² ([MS_R] f64)
constexpr int multi_class_lds(int C) { return C * (MS_W + 1) * MS_R * 8; }

__global__ void k_multi_cast(const double* __restrict__ P, int64_t nP, float* __restrict__ P32,
                             const double* __restrict__ mu, int64_t nmu, float* __restrict__ mu_hi,
                             float* __restrict__ mu_lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nP) P32[i] = (float)P[i];
  if (i < nmu) {
    const float hi = (float)mu[i];
    mu_hi[i] = hi;
    mu_lo[i] = (float)(mu[i] - (double)hi);
  }
}

// KT: component tiles of 16 of the largest class (k_c ≤ 16·KT).  VEC: 16-B
// loads of X, μ and P rows (p % 4 == 0, ldx % 4 == 0, 16-B aligned X).  ps: LDS
// row stride of the tile in floats (0: no tile, later sweeps read X again).
template <int KT, bool VEC>
__global__ __launch_bounds__(64 * MS_W, MS_WPC) void k_score_multi(
    const float* __restrict__ X, int64_t ldx, const int64_t* __restrict__ rows, int64_t m, int p,
    const float* __restrict__ P, const float* __restrict__ mu_hi, const float* __restrict__ mu_lo,
    const double* __restrict__ a_diag, int C, MsArgs args, double* __restrict__ T2_out, float* __restrict__ Q_out,
    double* __restrict__ ratio_out, double* __restrict__ accept_out, int64_t accept_stride,
    int8_t* __restrict__ index_out, uint8_t* __restrict__ nearest_out, uint8_t* __restrict__ naccept_out,
    const uint8_t* __restrict__ y_true, unsigned long long* __restrict__ counts, int64_t ntiles, int ps) {
  constexpr int KP = KT * 16;
  constexpr int PCS = KT <= 2 ? 4 : 1;  // 16-column pieces of a block loaded ahead of their MFMAs (registers)
  extern __shared__ __attribute__((aligned(32))) unsigned char dyn_lds[];
  float* xt = reinterpret_cast<float*>(dyn_lds);  // [MS_R][ps] raw rows
  __shared__ double tred[MS_W][KP][MS_R];          // partial t per wave; [0] holds the sum
  __shared__ MsDec decs[MS_MAXC];
  __shared__ unsigned cnt[MS_NCNT];
  double* qpart = reinterpret_cast<double*>(dyn_lds + (size_t)MS_R * ps * sizeof(float));  // [C][MS_W][MS_R]
  double* t2s = qpart + C * MS_W * MS_R;                                                    // [C][MS_R]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int ncnt = (C + 1) * (3 * C + 2);
  if (counts)
    for (int e = tid; e < ncnt; e += 64 * MS_W) cnt[e] = 0u;
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < MS_MAXC; ++c) decs[c] = args.dec[c];
  }

  auto ld4 = [&](const float* base, int col) -> f32x4 {
    f32x4 v;
    if (VEC) {
      v = *reinterpret_cast<const f32x4*>(base + (col < p ? col : 0));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = base[min(col + e, p - 1)];
    }
    return v;
  };

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * MS_R;
    // sweep 1: lane (row j, quarter q); sweep 2: lane (column j, quarter q), rows 4q + i
    const int64_t ga = row0 + j;
    const int64_t gac = ga < m ? ga : m - 1;  // rows past m read row m − 1; their results are dropped
    const float* xrow = X + (rows ? rows[gac] : gac) * ldx;
    const float* xr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t g = row0 + 4 * q + i;
      const int64_t gc = g < m ? g : m - 1;
      xr[i] = X + (rows ? rows[gc] : gc) * ldx;
    }
    for (int c = 0; c < C; ++c) {
      const int k0 = args.koff[c], kc = args.koff[c + 1] - k0;
      const int ktc = (kc + 15) >> 4;  // component tiles of this class (uniform)
      const int ns = (kc + 3) >> 2;    // sweep-2 steps of four components
      const float* Pc = P + (int64_t)k0 * p;
      const float* mh = mu_hi + (int64_t)c * p;
      const float* ml = mu_lo + (int64_t)c * p;
      const bool from_lds = ps && c > 0;

      // ---- sweep 1 ---------------------------------------------------------------
      f32x4 acc[KT];
      double acc64[KT][4];
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[t][i] = 0.f;
          acc64[t][i] = 0.0;
        }
      for (int b0 = wave * MS_CHAIN; b0 < p; b0 += MS_W * MS_CHAIN) {
#pragma unroll
        for (int g0 = 0; g0 < MS_CHAIN / 16; g0 += PCS) {
          if (b0 + 16 * g0 >= p) break;
          // PCS 16-B pieces of this lane's row, of the mean and of the loadings (from L2) ahead of their MFMAs
          f32x4 xv[PCS], uh[PCS], ul[PCS], w[PCS][KT];
#pragma unroll
          for (int cb = 0; cb < PCS; ++cb) {
            const int col = b0 + 16 * (g0 + cb) + 4 * q;  // loads past p are clamped, their values masked
            if (from_lds)  // this wave wrote it in the first class's sweep 1 (columns past p: masked below)
              xv[cb] = *reinterpret_cast<const f32x4*>(&xt[j * ps + col]);
            else
              xv[cb] = ld4(xrow, col);
            uh[cb] = ld4(mh, col);
            ul[cb] = ld4(ml, col);
#pragma unroll
            for (int t = 0; t < KT; ++t) {
              if (t < ktc) {
                const int comp = 16 * t + j;
                w[cb][t] = ld4(Pc + (int64_t)min(comp, kc - 1) * p, col);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (comp >= kc || col + e >= p) w[cb][t][e] = 0.f;
              }
            }
          }
#pragma unroll
          for (int cb = 0; cb < PCS; ++cb) {
            const int c0 = b0 + 16 * (g0 + cb);
            if (c0 >= p) break;
            const int col = c0 + 4 * q;
            if (ps && c == 0) *reinterpret_cast<f32x4*>(&xt[j * ps + col]) = xv[cb];
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              y[e] = ga < m && col + e < p ? __fsub_rn(__fsub_rn(xv[cb][e], uh[cb][e]), ul[cb][e]) : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int t = 0; t < KT; ++t)
                if (t < ktc) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[cb][t][e], y[e], acc[t], 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < KT; ++t)  // f32 chains of ≤ MS_CHAIN columns, flushed to f64
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc64[t][i] += (double)acc[t][i];
            acc[t][i] = 0.f;
          }
      }
      __syncthreads();  // the previous class's (or tile's) t is consumed (its sweep 2 operands, its T²)
#pragma unroll
      for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) tred[wave][16 * t + 4 * q + i][j] = acc64[t][i];  // D[M = comp][N = row j]
      __syncthreads();
      for (int e = tid; e < KP * MS_R; e += 64 * MS_W) {
        double* s = &tred[0][0][0] + e;
        *s = ((s[0] + s[KP * MS_R]) + s[2 * KP * MS_R]) + s[3 * KP * MS_R];
      }
      __syncthreads();

      if (wave == 0) {  // T² = Σ t²·a of row j: a quarter of the components per lane, fixed order
        double s2 = 0.0;
        for (int a = q; a < kc; a += 4) {
          const double tv = tred[0][a][j];
          s2 += tv * tv * a_diag[k0 + a];
        }
        s2 += __shfl_xor(s2, 16, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (q == 0) t2s[c * MS_R + j] = s2;
      }
      // ---- sweep 2 ---------------------------------------------------------------
      float tA[KT * 4];  // A operands: t of row j, component 4s + q (0 past k_c: its loadings were masked)
#pragma unroll
      for (int s = 0; s < KT * 4; ++s) tA[s] = (float)tred[0][4 * s + q][j];
      double rq[4] = {0.0, 0.0, 0.0, 0.0};
      for (int b0 = wave * MS_CHAIN; b0 < p; b0 += MS_W * MS_CHAIN) {
        const int col4 = b0 + 4 * j;  // the lane's four columns of the block
        f32x4 w2[KT * 4];
#pragma unroll
        for (int s = 0; s < KT * 4; ++s) {
          if (s < ns) {  // uniform: the trailing steps hold only zero operands
            const int comp = 4 * s + q;
            w2[s] = ld4(Pc + (int64_t)min(comp, kc - 1) * p, col4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (comp >= kc || col4 + e >= p) w2[s][e] = 0.f;
          }
        }
        const f32x4 uh = ld4(mh, col4), ul = ld4(ml, col4);
        f32x4 y[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          f32x4 xv;
          if (ps)  // written by this wave in the first class's sweep 1 (columns past p: never written)
            xv = *reinterpret_cast<const f32x4*>(&xt[(4 * q + i) * ps + col4]);
          else
            xv = ld4(xr[i], col4);
          const bool rok = row0 + 4 * q + i < m;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            y[i][e] = rok && col4 + e < p ? __fsub_rn(__fsub_rn(xv[e], uh[e]), ul[e]) : 0.f;
        }
        f32x4 e2[4];  // [row i][column e]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f32x4 aE = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KT * 4; ++s)
            if (s < ns) aE = __builtin_amdgcn_mfma_f32_16x16x4f32(tA[s], w2[s][e], aE, 0, 0, 0);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float ev = y[i][e] - aE[i];
            e2[i][e] = ev * ev;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)  // the lane's four columns in f32, then fp64
          rq[i] += (double)((e2[i][0] + e2[i][1]) + (e2[i][2] + e2[i][3]));
      }
      // row sums: over the 16 column lanes, then over the waves (fixed order)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) rq[i] += __shfl_xor(rq[i], o, 64);
        if (j == 0) qpart[(c * MS_W + wave) * MS_R + 4 * q + i] = rq[i];
      }
    }
    __syncthreads();  // every class's partial Q and T² of the tile are in LDS

    // ---- decide: thread (class c, row r) -------------------------------------------
    if (tid < MS_R * C) {
      const int c = tid >> 4, r = tid & 15;
      const int64_t g = row0 + r;
      const double* qp = qpart + c * MS_W * MS_R + r;
      const float Qf = (float)(((qp[0] + qp[MS_R]) + qp[2 * MS_R]) + qp[3 * MS_R]);
      const double T2 = t2s[c * MS_R + r];
      const MsDec d = decs[c];
      const double dr = ocm::dred_of(d.type, T2 * d.t2_scale, (double)Qf * d.q_scale);
      const bool ok = dr < d.dlim;
      const double ratio = dr / d.dlim;
      t2s[c * MS_R + r] = ratio;              // for the assignment below (this thread has read its T²)
      qpart[c * MS_W * MS_R + r] = ok ? 1.0 : 0.0;  // ... and its partial Q
      if (g < m) {
        if (T2_out) T2_out[g * C + c] = T2;
        if (Q_out) Q_out[g * C + c] = Qf;
        if (ratio_out) ratio_out[g * C + c] = ratio;
        if (accept_out) accept_out[g * accept_stride + c] = ok ? 1.0 : 0.0;
      }
    }
    __syncthreads();
    // ---- assign: thread r owns row r ---------------------------------------------------
    if (tid < MS_R && row0 + tid < m) {
      const int64_t g = row0 + tid;
      double best_all = __builtin_inf(), best_acc = __builtin_inf();
      int near = 0, idx = -1, nacc = 0;
      unsigned accmask = 0u;
      for (int c = 0; c < C; ++c) {
        const double ratio = t2s[c * MS_R + tid];
        const double rr = ratio != ratio ? __builtin_inf() : ratio;  // a NaN ratio counts as +inf
        if (rr < best_all) {
          best_all = rr;
          near = c;
        }
        if (qpart[c * MS_W * MS_R + tid] != 0.0) {
          if (idx < 0 || rr < best_acc) {
            best_acc = rr;
            idx = c;
          }
          ++nacc;
          accmask |= 1u << c;
        }
      }
      if (index_out) index_out[g] = (int8_t)idx;
      if (nearest_out) nearest_out[g] = (uint8_t)near;
      if (naccept_out) naccept_out[g] = (uint8_t)nacc;
      if (counts) {
        const int yt = min((int)y_true[g], C);  // a value ≥ C is the row "other"
        const int C1 = C + 1;
        atomicAdd(&cnt[yt * C1 + (idx < 0 ? C : idx)], 1u);
        for (int c = 0; c < C; ++c)
          if (accmask >> c & 1u) atomicAdd(&cnt[C1 * C1 + yt * C + c], 1u);
        atomicAdd(&cnt[C1 * C1 + C1 * C + yt * C1 + nacc], 1u);
      }
    }
  }
  if (counts) {
    __syncthreads();
    for (int e = tid; e < ncnt; e += 64 * MS_W) {
      const unsigned n = cnt[e];
      if (n) atomicAdd(&counts[e], (unsigned long long)n);
    }
  }
}

}  // namespace

extern "C" {

int ocm_score_multi_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                        const double* P, const double* mu, const double* a_diag, const int32_t* koff, int32_t C,
                        const ocm_decision* dec, double* T2_out, float* Q_out, double* ratio_out,
                        double* accept_out, int64_t accept_stride, int8_t* index_out, uint8_t* nearest_out,
                        uint8_t* naccept_out, const uint8_t* y_true, int64_t* counts_out, void* stream) {
  OCM_REQUIRE(ctx && P && mu && a_diag && koff && dec, "ocm_score_multi_f32: NULL argument");
  OCM_REQUIRE(X || m == 0, "ocm_score_multi_f32: X is NULL");
  OCM_REQUIRE(m >= 0 && p >= 1 && ldx >= p, "ocm_score_multi_f32: bad shape (m >= 0, p >= 1, ldx >= p)");
  OCM_REQUIRE(C >= 1 && C <= MS_MAXC, "ocm_score_multi_f32: 1 <= C <= 8");
  OCM_REQUIRE(koff[0] == 0, "ocm_score_multi_f32: koff[0] must be 0");
  MsArgs args{};
  int kmax = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t kc = (int64_t)koff[c + 1] - koff[c];
    OCM_REQUIRE(kc >= 1 && kc <= p, "ocm_score_multi_f32: every class needs 1 <= k_c <= p components");
    OCM_REQUIRE(koff[c + 1] <= MS_MAXK, "ocm_score_multi_f32: at most 64 stacked components");
    kmax = std::max<int>(kmax, (int)kc);
    args.koff[c] = koff[c];
    args.dec[c] = MsDec{dec[c].type, dec[c].t2_scale, dec[c].q_scale, dec[c].dlim};
  }
  args.koff[C] = koff[C];
  const int K = koff[C];
  OCM_REQUIRE(!accept_out || accept_stride >= C, "ocm_score_multi_f32: accept_stride >= C");
  OCM_REQUIRE(!counts_out || y_true || m == 0, "ocm_score_multi_f32: counts_out needs y_true");
  hipStream_t st = (hipStream_t)stream;
  if (counts_out) OCM_HIP(hipMemsetAsync(counts_out, 0, (size_t)(C + 1) * (3 * C + 2) * sizeof(int64_t), st));
  if (m == 0) return OCM_OK;
  const int64_t ntiles = (m + MS_R - 1) / MS_R;
  OCM_REQUIRE(ntiles < (1LL << 31), "ocm_score_multi_f32: too many rows");
  const int grid = (int)std::min<int64_t>((int64_t)MS_WPC * ctx->num_cus, ntiles);
  const size_t nP = (size_t)K * p, nmu = (size_t)C * p;
  void* w = ocm::workspace(ctx, (nP + 2 * nmu) * sizeof(float) + 1024, st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  float* P32 = cv.take<float>(nP);
  float* mu_hi = cv.take<float>(nmu);
  float* mu_lo = cv.take<float>(nmu);
  hipLaunchKernelGGL(k_multi_cast, dim3((unsigned)((std::max(nP, nmu) + 255) / 256)), dim3(256), 0, st, P,
                     (int64_t)nP, P32, mu, (int64_t)nmu, mu_hi, mu_lo);
  OCM_CHECK_LAUNCH("k_multi_cast");
  const int kt = (kmax + 15) / 16;
  // the row tile in LDS when it leaves room for every workgroup a CU runs at once
  int ps = (p + MS_CHAIN - 1) / MS_CHAIN * MS_CHAIN + 4;
  if ((size_t)MS_R * ps * sizeof(float) + multi_class_lds(C) + multi_static_lds(kt) > (size_t)MS_LDS_BYTES / MS_WPC)
    ps = 0;
  const size_t dyn = (size_t)MS_R * ps * sizeof(float) + multi_class_lds(C);
  const bool vec = (ldx % 4 == 0) && (p % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts_out);
  {
    ocm::TimedRegion tr(ctx, OCM_KERNEL_SCORE, st);
#define OCM_MULTI_LAUNCH(KT_, V_)                                                                                 \
  do {                                                                                                            \
    auto kern = k_score_multi<KT_, V_>;                                                                           \
    static int lds_ok[64] = {0}; /* per device: the attribute is set once per kernel, for the whole LDS */        \
    if (dyn > 0 && !lds_ok[ctx->device & 63]) {                                                                   \
      OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  MS_LDS_BYTES / MS_WPC - multi_static_lds(KT_)));                                \
      lds_ok[ctx->device & 63] = 1;                                                                               \
    }                                                                                                             \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * MS_W), dyn, st, X, ldx, rows, m, p, P32, mu_hi, mu_lo, a_diag, \
                       C, args, T2_out, Q_out, ratio_out, accept_out, accept_stride, index_out, nearest_out,     \
                       naccept_out, y_true, cnt, ntiles, ps);                                                     \
  } while (0)
#define OCM_MULTI_KT(KT_)         \
  if (vec)                        \
    OCM_MULTI_LAUNCH(KT_, true);  \
  else                            \
    OCM_MULTI_LAUNCH(KT_, false)
    if (kt == 1) {
      OCM_MULTI_KT(1);
    } else if (kt == 2) {
      OCM_MULTI_KT(2);
    } else if (kt == 3) {
      OCM_MULTI_KT(3);
    } else {
      OCM_MULTI_KT(4);
    }
#undef OCM_MULTI_KT
#undef OCM_MULTI_LAUNCH
  }
  OCM_CHECK_LAUNCH("k_score_multi");
  return OCM_OK;
}

}  // extern "C"
