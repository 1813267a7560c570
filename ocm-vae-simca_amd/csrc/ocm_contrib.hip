// Contribution plots of a SIMCA decision: per-variable residual e (Q) and
// T² share c of every processed row, their row sums, and the per-group
// column profiles Σ_rows e², Σ_rows c.
//
// With y = x − μ, t = P·y and a = diag(1/λ) (utils/SIMCA.py:67-71, 104-107):
//   e_j = y_j − Σ_c t_c·P_cj          Σ_j e_j² = Q
//   c_j = y_j · Σ_c (t_c·a_c)·P_cj    Σ_j c_j  = T²   (c_j may be negative)
//
// k_contrib: one workgroup of four waves per 16-row tile, persistent over the
// tiles, two workgroups per CU (two waves per SIMD, 256 registers each): one
// workgroup's loads and barriers overlap the other's MFMAs.  Measured at
// 1M × 2048, k = 20: one workgroup per CU with the whole tile in LDS 15.3 ms,
// two per CU 10.3 ms.  Where a tile of centred rows y fits twice
// into a CU's LDS (16 × p values ≤ ≈ 70 KiB: p ≤ ≈ 1000 f32, ≈ 500 f64) it
// stays in LDS between the two sweeps; for wider rows sweep 2 reads the tile's
// rows again through the cache hierarchy, 128 KiB after they were first read.
// The waves split the columns in blocks of 64.
//   sweep 1  Tᵀ (comps × rows) += P_chunk · Y_chunkᵀ on 16x16x4 MFMA: lane
//            (row = l&15, q = l>>4) feeds column 4q + e of a 16-column chunk
//            (one 16-B piece of its row) as B and the same columns of the
//            loadings as A; f32
//            partials over 64 columns, flushed to f64;
//   reduce   the four waves' partial t meet in LDS (f64, fixed order); t stays
//            there, as [comp][row], until the tile is done;
//   sweep 2  per 64-column block, lane (j = l&15, q) owns columns 4j .. 4j+3
//            (one 16-B piece of the loadings, of y and of E / C); for each of
//            its columns two chains over the components, (T·P) and (T·a·P)
//            (rows × cols: A = t or t·a of row l&15, B = the loadings of the
//            lane's column), so a lane holds four rows of its columns: e and
//            c and their squares / sums per row (f64).  The column sums over
//            the tile's rows per group are one more product, on the fp64
//            matrix core: a 0/1 group indicator (groups × rows) times e² or c
//            (rows × cols) — no transpose, no lane exchange.
// (An OCM_CONTRIB_WPS = 1 build loads the operands of a block one block ahead on
// the aligned float32, k ≤ 32 variants; two waves per SIMD hide more.)
// Profiles: every workgroup owns one ngroups × 2 × p fp64 slice of the context
// workspace: its first tile stores the column sums there, the later ones add (the same lane owns the
// same address for the whole launch: plain loads and stores); k_contrib_reduce
// sums the slices in workgroup order.  No floating-point atomics: a launch's
// result depends on its arguments only.
#include "ocm_internal.h"

#include <algorithm>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int CW = 4;    // waves per workgroup
constexpr int CR = 16;   // rows per tile
constexpr int CB = 64;   // columns per wave block (the f32 chain length)
constexpr int LDS_BYTES = 160 * 1024;
// A/B knobs of `make exp` builds (the product library is built with the defaults)
#ifndef OCM_CONTRIB_LDS
#define OCM_CONTRIB_LDS 1  // 0: never keep the row tile in LDS (sweep 2 reads X again)
#endif
#ifndef OCM_CONTRIB_WPS
#define OCM_CONTRIB_WPS 2  // waves per SIMD = workgroups per CU (1: 512 registers each, 2: 256)
#endif

template <typename T>
struct Mf;
template <>
struct Mf<float> {
  using acc = f32x4;
  using vec4 = f32x4;
  static __device__ __forceinline__ acc mfma(float a, float b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  // accumulator register i of lane quarter q holds row ...
  static __device__ __forceinline__ int row(int q, int i) { return 4 * q + i; }
};
template <>
struct Mf<double> {
  using acc = f64x4;
  using vec4 = f64x4;
  static __device__ __forceinline__ acc mfma(double a, double b, acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int i) { return q + 4 * i; }
};

// static LDS of k_contrib<T, KT, *> (the rest is the row tile)
constexpr int contrib_static_lds(int kt) { return CW * kt * 16 * CR * 8 + CW * 2 * CR * 8 + CR * 4 + 64; }

// KT: component tiles of 16 (k ≤ 16·KT).  VEC: 16-B loads of X, μ and P rows
// (p % 4 == 0, ldx % 4 == 0, 16-B aligned bases).  ps: LDS row stride of the
// tile in elements (0: no tile, sweep 2 reads X again).  vst: E_out / C_out
// take 16-B stores (f32, p, lde, ldc multiples of 4, 16-B aligned bases).
template <typename T, int KT, bool VEC>
__global__ __launch_bounds__(64 * CW, OCM_CONTRIB_WPS) void k_contrib(const T* __restrict__ X, int64_t ldx,
                                                        const int64_t* __restrict__ rows, int64_t m, int p,
                                                        const T* __restrict__ P, const T* __restrict__ mu,
                                                        const double* __restrict__ a_diag, int k,
                                                        const uint8_t* __restrict__ group, int ngroups,
                                                        T* __restrict__ E_out, int64_t lde, T* __restrict__ C_out,
                                                        int64_t ldc, double* __restrict__ T2_out,
                                                        T* __restrict__ Q_out, double* __restrict__ part,
                                                        int64_t ntiles, int ps, int vst) {
  using M = Mf<T>;
  using acc_t = typename M::acc;
  using vec4 = typename M::vec4;
  constexpr int KP = KT * 16;
  // operands one 64-column block ahead of the MFMAs where the registers allow it
  // (one wave per SIMD, aligned float32, k ≤ 32); the other variants load in place
  constexpr bool PF = OCM_CONTRIB_WPS == 1 && sizeof(T) == 4 && KT <= 2 && VEC;
  extern __shared__ __attribute__((aligned(32))) unsigned char dyn_lds[];
  T* yt = reinterpret_cast<T*>(dyn_lds);  // [CR][ps]
  __shared__ double tred[CW][KP][CR];      // partial t per wave; [0] holds the sum
  __shared__ double rowred[CW][2][CR];
  __shared__ int grp_s[CR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int ns = (k + 3) / 4;  // sweep-2 steps of four components
  double* mypart = part ? part + (int64_t)blockIdx.x * ngroups * 2 * p : nullptr;

  auto ld4 = [&](const T* base, int col) -> vec4 {
    vec4 v;
    if (VEC) {
      v = *reinterpret_cast<const vec4*>(base + (col < p ? col : 0));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = base[min(col + e, p - 1)];
    }
    return v;
  };

  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * CR;
    __syncthreads();  // the previous tile's tred / rowred / grp_s are consumed
    if (tid < CR) {
      const int64_t g = row0 + tid;
      int gi = 255;
      if (g < m) {
        gi = group ? (int)group[g] : 0;
        if (gi >= ngroups) gi = 255;
      }
      grp_s[tid] = gi;
    }
    // ---- sweep 1: lane (row j, quarter q) -------------------------------------
    const int64_t ga = row0 + j;
    const int64_t gac = ga < m ? ga : m - 1;
    const T* xrow = X + (rows ? rows[gac] : gac) * ldx;
    const bool aok = ga < m;
    acc_t acc[KT];
    double acc64[KT][4];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[t][i] = T(0);
        acc64[t][i] = 0.0;
      }
    // the block's four 16-B pieces of this lane's row
    // (with the same pieces of the mean and of the loadings, which come from L2)
    struct S1 {
      vec4 x[CB / 16], u[CB / 16], w[CB / 16][KT];
    };
    auto load1 = [&](S1& S, int b0) {
#pragma unroll
      for (int cb = 0; cb < CB / 16; ++cb) {
        const int col = b0 + 16 * cb + 4 * q;  // loads past p are clamped, their values masked
        S.x[cb] = ld4(xrow, col);
        S.u[cb] = ld4(mu, col);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
          const int comp = 16 * t + j;
          S.w[cb][t] = ld4(P + (int64_t)min(comp, k - 1) * p, col);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (comp >= k || col + e >= p) S.w[cb][t][e] = T(0);
        }
      }
    };
    S1 SA, SB;
    SB = S1{};
    if (PF && wave * CB < p) load1(SA, wave * CB);
    for (int b0 = wave * CB; b0 < p; b0 += CW * CB) {
      if (!PF)
        load1(SA, b0);
      else if (b0 + CW * CB < p)
        load1(SB, b0 + CW * CB);
#pragma unroll
      for (int cb = 0; cb < CB / 16; ++cb) {
        const int c0 = b0 + 16 * cb;
        if (c0 >= p) break;
        const int col = c0 + 4 * q;
        const vec4 xv = SA.x[cb];
        const vec4 uv = SA.u[cb];
        vec4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = aok && col + e < p ? xv[e] - uv[e] : T(0);
        if (ps) *reinterpret_cast<vec4*>(&yt[j * ps + col]) = y;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < KT; ++t) acc[t] = M::mfma(SA.w[cb][t][e], y[e], acc[t]);
      }
      if constexpr (sizeof(T) == 4) {  // f32 chains of ≤ 64 columns, flushed to f64
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc64[t][i] += (double)acc[t][i];
            acc[t][i] = T(0);
          }
      }
      if (PF) SA = SB;
    }
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double v = sizeof(T) == 4 ? acc64[t][i] : (double)acc[t][i];
        tred[wave][16 * t + M::row(q, i)][j] = v;  // D[M = comp][N = row j]
      }
    __syncthreads();
    for (int e = tid; e < KP * CR; e += 64 * CW) {
      double* s = &tred[0][0][0] + e;
      *s = ((s[0] + s[KP * CR]) + s[2 * KP * CR]) + s[3 * KP * CR];
    }
    __syncthreads();

    // ---- sweep 2: lane (column j, quarter q), rows M::row(q, i) ---------------
    T tA[KT * 4], tS[KT * 4];  // A operands: t and t·a of row j, component 4s + q
#pragma unroll
    for (int s = 0; s < KT * 4; ++s) {
      const int comp = 4 * s + q;
      const double tv = tred[0][comp][j];
      const double av = a_diag[min(comp, k - 1)];
      tA[s] = (T)tv;
      tS[s] = comp < k ? (T)(tv * av) : T(0);
    }
    int64_t grow[4];
    const T* xr[4];
    bool rok[4];
    double ind[4];  // A operand of the group sums: row M::row(q, i) is in group j
    double rq[4], rt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = M::row(q, i);
      grow[i] = row0 + r;
      const int64_t gc = grow[i] < m ? grow[i] : m - 1;
      xr[i] = X + (rows ? rows[gc] : gc) * ldx;
      rok[i] = grow[i] < m;
      ind[i] = grp_s[r] == j ? 1.0 : 0.0;
      rq[i] = 0.0;
      rt[i] = 0.0;
    }
    // a lane owns four neighbouring columns of the block (one 16-B piece of the
    // loadings, of y and of the outputs); MFMA group e takes column 4j + e of each lane
    // the loadings of a block are loaded one block ahead
    struct S2 {
      vec4 w[KT * 4];
    };
    auto load2 = [&](S2& S, int b0) {
      const int c4 = b0 + 4 * j;
#pragma unroll
      for (int s = 0; s < KT * 4; ++s) {
        if (s < ns) {  // uniform: the trailing steps hold only zero operands
          const int comp = 4 * s + q;
          S.w[s] = ld4(P + (int64_t)min(comp, k - 1) * p, c4);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (comp >= k || c4 + e >= p) S.w[s][e] = T(0);
        }
      }
    };
    S2 PA, PB;
    PA = S2{};
    PB = S2{};
    if (PF && wave * CB < p) load2(PA, wave * CB);
    for (int b0 = wave * CB; b0 < p; b0 += CW * CB) {
      const int col4 = b0 + 4 * j;
      if (!PF)
        load2(PA, b0);
      else if (b0 + CW * CB < p)
        load2(PB, b0 + CW * CB);
      // this lane's slice of the workgroup's profile partials (quarter q keeps group q)
      // (its first tile stores, the later ones add: the slice needs no zero fill)
      const bool own = mypart && q < ngroups;
      double* pe = own ? mypart + ((int64_t)q * 2 + 0) * p + col4 : nullptr;
      double* pc = own ? mypart + ((int64_t)q * 2 + 1) * p + col4 : nullptr;
      const bool add = own && tile != (int64_t)blockIdx.x;
      double oe[4], oc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        oe[e] = add && col4 + e < p ? pe[e] : 0.0;
        oc[e] = add && col4 + e < p ? pc[e] : 0.0;
      }
      vec4 y[4];
      if (ps) {
#pragma unroll
        for (int i = 0; i < 4; ++i)  // this wave wrote it in sweep 1 (columns past p: never written)
          y[i] = *reinterpret_cast<const vec4*>(&yt[M::row(q, i) * ps + col4]);
      } else {
        const vec4 uv = ld4(mu, col4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const vec4 xv = ld4(xr[i], col4);
#pragma unroll
          for (int e = 0; e < 4; ++e) y[i][e] = rok[i] ? xv[e] - uv[e] : T(0);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col4 + e >= p) y[i][e] = T(0);
      vec4 ev[4], cv[4], e2[4];  // [row i][column e]
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc_t aE, aS;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          aE[i] = T(0);
          aS[i] = T(0);
        }
#pragma unroll
        for (int s = 0; s < KT * 4; ++s) {
          if (s < ns) {
            aE = M::mfma(tA[s], PA.w[s][e], aE);
            aS = M::mfma(tS[s], PA.w[s][e], aS);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ev[i][e] = y[i][e] - aE[i];
          cv[i][e] = y[i][e] * aS[i];
          e2[i][e] = ev[i][e] * ev[i][e];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // the lane's four columns in the input precision, then fp64
        rq[i] += (double)((e2[i][0] + e2[i][1]) + (e2[i][2] + e2[i][3]));
        rt[i] += (double)((cv[i][0] + cv[i][1]) + (cv[i][2] + cv[i][3]));
      }
      if (col4 < p) {
        const bool whole = vst && col4 + 3 < p;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (grow[i] >= m) continue;
          if (E_out) {
            T* eo = E_out + grow[i] * lde + col4;
            if (whole) {
              *reinterpret_cast<vec4*>(eo) = ev[i];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (col4 + e < p) eo[e] = ev[i][e];
            }
          }
          if (C_out) {
            T* co = C_out + grow[i] * ldc + col4;
            if (whole) {
              *reinterpret_cast<vec4*>(co) = cv[i];
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (col4 + e < p) co[e] = cv[i][e];
            }
          }
        }
      }
      if (mypart) {
        // column sums over the tile's 16 rows per group on the fp64 matrix core:
        // D[group][column] = Σ_rows ind[group][row] · v[row][column] (exact products,
        // one fixed summation order); lane quarter g, register 0 holds group g
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f64x4 gE = {0.0, 0.0, 0.0, 0.0}, gC = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            gE = __builtin_amdgcn_mfma_f64_16x16x4f64(ind[i], (double)e2[i][e], gE, 0, 0, 0);
            gC = __builtin_amdgcn_mfma_f64_16x16x4f64(ind[i], (double)cv[i][e], gC, 0, 0, 0);
          }
          if (own && col4 + e < p) {
            pe[e] = oe[e] + gE[0];
            pc[e] = oc[e] + gC[0];
          }
        }
      }
      if (PF) PA = PB;
    }
    // row sums: over the 16 column lanes, then over the waves (fixed order)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        rq[i] += __shfl_xor(rq[i], o, 64);
        rt[i] += __shfl_xor(rt[i], o, 64);
      }
      if (j == 0) {
        rowred[wave][0][M::row(q, i)] = rq[i];
        rowred[wave][1][M::row(q, i)] = rt[i];
      }
    }
    __syncthreads();
    if (tid < 2 * CR) {
      const int w = tid / CR, r = tid % CR;
      const double v = ((rowred[0][w][r] + rowred[1][w][r]) + rowred[2][w][r]) + rowred[3][w][r];
      const int64_t g = row0 + r;
      if (g < m) {
        if (w == 0 && Q_out) Q_out[g] = (T)v;
        if (w == 1 && T2_out) T2_out[g] = v;
      }
    }
  }
}

// prof[i] = Σ_w part[w][i] in workgroup order, i < n (= ngroups·2·p)
__global__ __launch_bounds__(256) void k_contrib_reduce(const double* __restrict__ part, int nwg, int64_t n,
                                                        double* __restrict__ prof) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  for (int w = 0; w < nwg; ++w) v += part[(int64_t)w * n + i];
  prof[i] = v;
}

template <typename T>
int check_args(const char* who, ocm_ctx* ctx, const T* X, int64_t ldx, int64_t m, int32_t p, const double* P,
               const double* mu, const double* a_diag, int32_t k, int32_t ngroups, const T* E_out, int64_t lde,
               const T* C_out, int64_t ldc) {
  const std::string w(who);
  OCM_REQUIRE(ctx && X && P && mu && a_diag, w + ": NULL argument");
  OCM_REQUIRE(m >= 1 && p >= 1, w + ": m >= 1 and p >= 1");
  OCM_REQUIRE(ldx >= p, w + ": ldx >= p");
  OCM_REQUIRE(k >= 1, w + ": k >= 1");
  if (k > 64 || k > p)
    return ocm::fail(OCM_ERR_UNSUPPORTED, w + ": k <= min(p, 64) (got k = " + std::to_string(k) + ")");
  OCM_REQUIRE(ngroups >= 1 && ngroups <= 4, w + ": 1 <= ngroups <= 4");
  OCM_REQUIRE(!E_out || lde >= p, w + ": lde >= p");
  OCM_REQUIRE(!C_out || ldc >= p, w + ": ldc >= p");
  OCM_REQUIRE((m + CR - 1) / CR < (1LL << 31), w + ": too many rows");
  return OCM_OK;
}

template <typename T>
int contrib_impl(ocm_ctx* ctx, const T* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p, const double* P,
                 const double* mu, const double* a_diag, int32_t k, const uint8_t* group, int32_t ngroups, T* E_out,
                 int64_t lde, T* C_out, int64_t ldc, double* T2_out, T* Q_out, double* prof_out, hipStream_t st) {
  constexpr bool F32 = sizeof(T) == 4;
  const int64_t ntiles = (m + CR - 1) / CR;
  const int grid = (int)std::min<int64_t>((int64_t)OCM_CONTRIB_WPS * ctx->num_cus, ntiles);
  const int64_t nprof = (int64_t)ngroups * 2 * p;
  // workspace: O(p) per workgroup of a grid that does not grow with m
  const size_t part_n = prof_out ? (size_t)grid * nprof : 0;
  const size_t cast_n = F32 ? (size_t)k * p + (size_t)p : 0;
  void* w = ocm::workspace(ctx, part_n * sizeof(double) + cast_n * sizeof(float) + 1024, st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  double* part = prof_out ? cv.take<double>(part_n) : nullptr;
  const T* Pk;
  const T* muk;
  if constexpr (F32) {  // the f32 kernel takes f32 loadings / mean, as the scoring kernels do
    float* P32 = cv.take<float>((size_t)k * p);
    float* mu32 = cv.take<float>(p);
    if (int rc = ocm_cast_f64_f32(ctx, P, (int64_t)k * p, P32, st)) return rc;
    if (int rc = ocm_cast_f64_f32(ctx, mu, (int64_t)p, mu32, st)) return rc;
    Pk = P32;
    muk = mu32;
  } else {
    Pk = P;
    muk = mu;
  }
  const int kt = (k + 15) / 16;
  // the row tile in LDS when it leaves room for every workgroup a CU runs at once
  int ps = (p + CB - 1) / CB * CB + 4;
  if (!OCM_CONTRIB_LDS ||
      (size_t)CR * ps * sizeof(T) + contrib_static_lds(kt) > (size_t)LDS_BYTES / OCM_CONTRIB_WPS)
    ps = 0;
  const size_t dyn = (size_t)CR * ps * sizeof(T);
  const auto al16 = [](const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; };
  const int vst = F32 && p % 4 == 0 && (!E_out || (lde % 4 == 0 && al16(E_out))) &&
                  (!C_out || (ldc % 4 == 0 && al16(C_out)));
  const bool vec = F32 && (ldx % 4 == 0) && (p % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
#define OCM_CONTRIB_LAUNCH(KT_, V_)                                                                              \
  do {                                                                                                            \
    auto kern = k_contrib<T, KT_, V_>;                                                                            \
    static int lds_ok[64] = {0}; /* per device: the attribute is set once per kernel, for the whole LDS */        \
    if (dyn > 48 * 1024 && !lds_ok[ctx->device & 63]) {                                                           \
      OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  LDS_BYTES - contrib_static_lds(KT_)));                                          \
      lds_ok[ctx->device & 63] = 1;                                                                               \
    }                                                                                                             \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * CW), dyn, st, X, ldx, rows, m, p, Pk, muk, a_diag, k, group,   \
                       ngroups, E_out, lde, C_out, ldc, T2_out, Q_out, part, ntiles, ps, vst);                    \
  } while (0)
#define OCM_CONTRIB_KT(KT_)           \
  if (vec)                            \
    OCM_CONTRIB_LAUNCH(KT_, true);    \
  else                                \
    OCM_CONTRIB_LAUNCH(KT_, false)
  if (kt == 1) {
    OCM_CONTRIB_KT(1);
  } else if (kt == 2) {
    OCM_CONTRIB_KT(2);
  } else if (kt == 3) {
    OCM_CONTRIB_KT(3);
  } else {
    OCM_CONTRIB_KT(4);
  }
#undef OCM_CONTRIB_KT
#undef OCM_CONTRIB_LAUNCH
  OCM_CHECK_LAUNCH("k_contrib");
  if (prof_out) {
    hipLaunchKernelGGL(k_contrib_reduce, dim3((unsigned)((nprof + 255) / 256)), dim3(256), 0, st, part, grid, nprof,
                       prof_out);
    OCM_CHECK_LAUNCH("k_contrib_reduce");
  }
  return OCM_OK;
}

}  // namespace

extern "C" {

int ocm_contrib_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                    const double* P, const double* mu, const double* a_diag, int32_t k, const uint8_t* group,
                    int32_t ngroups, float* E_out, int64_t lde, float* C_out, int64_t ldc, double* T2_out,
                    float* Q_out, double* prof_out, void* stream) {
  if (int rc = check_args("ocm_contrib_f32", ctx, X, ldx, m, p, P, mu, a_diag, k, ngroups, E_out, lde, C_out, ldc))
    return rc;
  return contrib_impl<float>(ctx, X, ldx, rows, m, p, P, mu, a_diag, k, group, ngroups, E_out, lde, C_out, ldc,
                             T2_out, Q_out, prof_out, (hipStream_t)stream);
}

int ocm_contrib_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                    const double* P, const double* mu, const double* a_diag, int32_t k, const uint8_t* group,
                    int32_t ngroups, double* E_out, int64_t lde, double* C_out, int64_t ldc, double* T2_out,
                    double* Q_out, double* prof_out, void* stream) {
  if (int rc = check_args("ocm_contrib_f64", ctx, X, ldx, m, p, P, mu, a_diag, k, ngroups, E_out, lde, C_out, ldc))
    return rc;
  return contrib_impl<double>(ctx, X, ldx, rows, m, p, P, mu, a_diag, k, group, ngroups, E_out, lde, C_out, ldc,
                              T2_out, Q_out, prof_out, (hipStream_t)stream);
}

}  // extern "C"
