// PLS-DA (include/ocm.h, "PLS-DA"): the PLS recursion on the moments of the
// training rows, and the one-pass projection + LDA sweep over the rows scored.
//
// Reference math: data_cheese.py:193-328 (PLSRegression(a) then
// LinearDiscriminantAnalysis on its scores, for every a and every fold);
// sklearn/cross_decomposition/_pls.py (NIPALS, _svd_flip_1d, "y residual is
// constant"); Dayal & MacGregor 1997, the improved kernel algorithm.
//
// ocm_pls_fit_f64.  Kernel PLS needs only S = XcᵀXc and s = XcᵀYc.  For
// component a:  w = dominant left singular vector of s (s itself for one
// column), r = w − Σ_{j<a} (p_jᵀw) r_j, v = S r, tt = rᵀv, p = v / tt,
// q = sᵀr / tt, s −= tt p qᵀ.  Two launches per component for all problems:
//   k_pls_step    one workgroup per problem: finishes component a − 1 from its
//                 v (tt, p, q, the deflation of s) and prepares w, r of
//                 component a — the O(p·a) work;
//   k_pls_matvec  v = S r, PLS_MV_ROWS rows of one problem's S per workgroup,
//                 a wave per row pair: S is read once per component.
// A launch boundary is the only synchronisation.  Every sum is taken in a fixed
// order (a lane's elements in index order, the wave butterfly, the waves in
// order), so two calls give the same bits.  The workspace holds w, r, v and
// the deflated s of each problem: it does not grow with A (p_j and r_j are
// read back from the outputs).
//
// ocm_plsda_predict_f32.  k_score_direct's sweep 1 (ocm_score.hip) without
// its sweep 2: every wave streams its 32 rows from HBM straight into f32 MFMA
// operands (v_mfma_f32_32x32x2_f32), the projection matrix and the mean staged
// per workgroup in LDS blocks of PD_CHAIN columns; an f32 accumulation chain
// runs over one block and is then added to the fp64 scores.  The mean is kept
// as a float pair (hi + lo), so y = (x − hi) − lo carries two roundings of y
// whatever the size of the mean.  The epilogue gathers a wave's scores in LDS
// (fp64) and applies the LDA of every prefix length: D, the first class at the
// maximum, and the confusion counts (LDS counters per workgroup, one 64-bit
// atomic per non-zero counter at the end; integers, so the order is free).
#include "ocm_internal.h"

#include <algorithm>

namespace {

// ---------------------------------------------------------------------------
// PLS recursion
// ---------------------------------------------------------------------------
constexpr int PLS_NT = 256;      // threads per workgroup
constexpr int PLS_NW = PLS_NT / 64;
constexpr int PLS_MV_ROWS = 8;   // rows of S per matvec workgroup (two per wave)
constexpr int PLS_MAXM = 8;      // target columns
constexpr int PLS_MAXA = 64;     // components

// Σ over the workgroup, the same bits in every thread: red holds PLS_NW doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < PLS_NW; ++w) s += red[w];
  return s;
}

// Σ_i a[i·sa]·b[i·sb] over one wave
__device__ __forceinline__ double wave_dot(const double* a, int sa, const double* b, int sb, int p, int lane) {
  double acc = 0.0;
  for (int i = lane; i < p; i += 64) acc += a[(int64_t)i * sa] * b[(int64_t)i * sb];
  return wave_sum_f64(acc);
}

// dominant eigenvector of the symmetric M × M matrix G (destroyed): cyclic
// Jacobi until the off-diagonal mass is below eps² of the diagonal's
__device__ void jacobi_dominant(double* G, double* V, int M, double* c_out) {
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) V[i * M + j] = i == j ? 1.0 : 0.0;
  const double eps2 = 0x1p-104;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int i = 0; i < M; ++i) {
      dg += G[i * M + i] * G[i * M + i];
      for (int j = i + 1; j < M; ++j) off += G[i * M + j] * G[i * M + j];
    }
    if (!(off > eps2 * dg)) break;
    for (int i = 0; i < M - 1; ++i)
      for (int j = i + 1; j < M; ++j) {
        const double gij = G[i * M + j];
        if (gij == 0.0) continue;
        const double theta = (G[j * M + j] - G[i * M + i]) / (2.0 * gij);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
        for (int l = 0; l < M; ++l) {  // columns i, j
          const double a = G[l * M + i], b = G[l * M + j];
          G[l * M + i] = c * a - sn * b;
          G[l * M + j] = sn * a + c * b;
        }
        for (int l = 0; l < M; ++l) {  // rows i, j
          const double a = G[i * M + l], b = G[j * M + l];
          G[i * M + l] = c * a - sn * b;
          G[j * M + l] = sn * a + c * b;
        }
        G[i * M + j] = 0.0;
        G[j * M + i] = 0.0;
        for (int l = 0; l < M; ++l) {
          const double a = V[l * M + i], b = V[l * M + j];
          V[l * M + i] = c * a - sn * b;
          V[l * M + j] = sn * a + c * b;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < M; ++i)
    if (G[i * M + i] > G[best * M + best]) best = i;
  for (int l = 0; l < M; ++l) c_out[l] = V[l * M + best];
}

// per-problem workspace: w, r, v (p each), the deflated s (p·M), ‖s₀‖²
__host__ __device__ inline int64_t pls_ws_doubles(int p, int M) { return (int64_t)p * (3 + M) + 8; }

__global__ __launch_bounds__(PLS_NT) void k_pls_step(int a, int A, int p, int M, const double* __restrict__ s_in,
                                                    double* __restrict__ ws, int* __restrict__ done,
                                                    double* W_out, double* R_out, double* P_out,
                                                    double* __restrict__ q_out, double* __restrict__ tt_out,
                                                    int* __restrict__ ncomp_out) {
  __shared__ double red[PLS_NW];
  __shared__ double gsh[PLS_MAXA];
  __shared__ double Gm[PLS_MAXM * PLS_MAXM], Vm[PLS_MAXM * PLS_MAXM], cv[PLS_MAXM], qv[PLS_MAXM];
  __shared__ double amax_v[PLS_NW];
  __shared__ int amax_i[PLS_NW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (done[b]) return;  // the same for the whole workgroup (written by an earlier launch)
  double* w = ws + (int64_t)b * pls_ws_doubles(p, M);
  double* r = w + p;
  double* v = r + p;
  double* s = v + p;
  double* scal = s + (int64_t)p * M;
  double* Wb = W_out + (int64_t)b * A * p;
  double* Rb = R_out + (int64_t)b * A * p;
  double* Pb = P_out + (int64_t)b * A * p;
  const int pm = p * M;

  if (a == 0) {
    const double* s0 = s_in + (int64_t)b * pm;
    for (int i = tid; i < pm; i += PLS_NT) s[i] = s0[i];
    __syncthreads();
  } else {
    // ---- finish component a − 1: tt = rᵀv, p = v / tt, q = sᵀr / tt, s −= tt p qᵀ
    const int j = a - 1;
    double acc = 0.0;
    for (int i = tid; i < p; i += PLS_NT) acc += r[i] * v[i];
    const double tt = block_sum(acc, red);
    if (!(tt > 0.0)) {
      if (tid == 0) done[b] = 1;
      return;
    }
    for (int mm = wave; mm < M; mm += PLS_NW) {
      const double d = wave_dot(s + mm, M, r, 1, p, lane);
      if (lane == 0) qv[mm] = d / tt;
    }
    __syncthreads();
    for (int i = tid; i < p; i += PLS_NT) {
      const double pi = v[i] / tt;
      Pb[(int64_t)j * p + i] = pi;
      Wb[(int64_t)j * p + i] = w[i];
      Rb[(int64_t)j * p + i] = r[i];
      const double tp = tt * pi;
      for (int mm = 0; mm < M; ++mm) s[(int64_t)i * M + mm] -= tp * qv[mm];
    }
    if (tid < M) q_out[((int64_t)b * A + j) * M + tid] = qv[tid];
    if (tid == 0) {
      tt_out[(int64_t)b * A + j] = tt;
      ncomp_out[b] = a;
    }
    __syncthreads();
  }
  if (a >= A) return;

  // ---- prepare component a: the stop test, w, r
  double acc = 0.0;
  for (int i = tid; i < pm; i += PLS_NT) acc += s[i] * s[i];
  const double ss = block_sum(acc, red);
  if (a == 0 && tid == 0) scal[0] = ss;
  const double ss0 = a == 0 ? ss : scal[0];
  if (ss <= 0x1p-100 * ss0) {  // "y residual is constant"
    if (tid == 0) done[b] = 1;
    return;
  }
  if (M > 1) {
    const int npair = M * (M + 1) / 2;
    for (int e = wave; e < npair; e += PLS_NW) {
      int m0 = 0, rem = e;
      while (rem >= M - m0) {
        rem -= M - m0;
        ++m0;
      }
      const int m1 = m0 + rem;
      const double d = wave_dot(s + m0, M, s + m1, M, p, lane);
      if (lane == 0) {
        Gm[m0 * M + m1] = d;
        Gm[m1 * M + m0] = d;
      }
    }
    __syncthreads();
    if (tid == 0) jacobi_dominant(Gm, Vm, M, cv);
    __syncthreads();
  }
  // w (not yet scaled), its norm and its largest entry (the first of equals)
  double n2 = 0.0, bv = -1.0;
  int bi = 0;
  for (int i = tid; i < p; i += PLS_NT) {
    double wi;
    if (M == 1) {
      wi = s[i];
    } else {
      wi = 0.0;
      for (int mm = 0; mm < M; ++mm) wi += s[(int64_t)i * M + mm] * cv[mm];
    }
    w[i] = wi;
    n2 += wi * wi;
    if (fabs(wi) > bv) {
      bv = fabs(wi);
      bi = i;
    }
  }
  const double nrm2 = block_sum(n2, red);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    amax_v[wave] = bv;
    amax_i[wave] = bi;
  }
  __syncthreads();  // also orders the w stores before the reads below
  bv = amax_v[0];
  bi = amax_i[0];
  for (int ww = 1; ww < PLS_NW; ++ww)
    if (amax_v[ww] > bv || (amax_v[ww] == bv && amax_i[ww] < bi)) {
      bv = amax_v[ww];
      bi = amax_i[ww];
    }
  const double scale = (w[bi] < 0.0 ? -1.0 : 1.0) / sqrt(nrm2);
  __syncthreads();  // every thread has read w[bi]
  for (int i = tid; i < p; i += PLS_NT) w[i] *= scale;
  __syncthreads();
  for (int j = wave; j < a; j += PLS_NW) {
    const double d = wave_dot(Pb + (int64_t)j * p, 1, w, 1, p, lane);
    if (lane == 0) gsh[j] = d;
  }
  __syncthreads();
  for (int i = tid; i < p; i += PLS_NT) {
    double ri = w[i];
    for (int j = 0; j < a; ++j) ri -= gsh[j] * Rb[(int64_t)j * p + i];
    r[i] = ri;
  }
}

// v = S r for every live problem; grid = nprob · ⌈p / PLS_MV_ROWS⌉
__global__ __launch_bounds__(PLS_NT) void k_pls_matvec(int p, int M, int nrt, const double* __restrict__ S,
                                                      double* __restrict__ ws, const int* __restrict__ done) {
  const int b = blockIdx.x / nrt, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (done[b]) return;
  double* wsb = ws + (int64_t)b * pls_ws_doubles(p, M);
  const double* r = wsb + p;
  double* v = wsb + 2 * (int64_t)p;
  const int row0 = (blockIdx.x % nrt) * PLS_MV_ROWS + wave * 2;
  if (row0 >= p) return;
  const int row1 = row0 + 1 < p ? row0 + 1 : row0;
  const double* S0 = S + ((int64_t)b * p + row0) * p;
  const double* S1 = S + ((int64_t)b * p + row1) * p;
  double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
  for (int j = lane; j < p; j += 64) {
    const double rj = r[j];
    a0 += S0[j] * rj;
    a1 += S1[j] * rj;
  }
  a0 = wave_sum_f64(a0);
  a1 = wave_sum_f64(a1);
  if (lane == 0) {
    v[row0] = a0;
    if (row0 + 1 < p) v[row0 + 1] = a1;
  }
}

// ---------------------------------------------------------------------------
// projection + LDA sweep
// ---------------------------------------------------------------------------
constexpr int PD_CHAIN = 256;  // columns of one f32 accumulation chain (an LDS block), then fp64
constexpr int PD_W = 4;        // waves per workgroup
constexpr int PD_R = 32;       // rows per wave
constexpr int PD_ROWS = PD_W * PD_R;
constexpr int PD_AHEAD = 4;    // 32-column chunks of a wave's rows in flight ahead of the MFMAs
constexpr int PD_CNT_LDS = 512;  // confusion counters kept in LDS (more: global atomics)
constexpr int PD_MAXK = 64, PD_MAXLV = 64, PD_MAXC = 8;

struct PdLvs {
  uint8_t lv[PD_MAXLV];
};

__global__ void k_pd_cast(const double* __restrict__ P, int64_t n, float* __restrict__ P32, const double* __restrict__ mu,
                          int p, float* __restrict__ mu_hi, float* __restrict__ mu_lo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) P32[i] = (float)P[i];
  if (i < p) {
    const float hi = (float)mu[i];
    mu_hi[i] = hi;
    mu_lo[i] = (float)(mu[i] - (double)hi);
  }
}

template <int KT, bool VEC>
__global__ __launch_bounds__(256, 2) void k_plsda_predict(
    const float* __restrict__ X, int64_t ldx, const int64_t* __restrict__ rows, int64_t m, int p,
    const float* __restrict__ P, const float* __restrict__ mu_hi, const float* __restrict__ mu_lo, int k, int nlv,
    PdLvs lvs, int C, const double* __restrict__ table, float* __restrict__ T_out, float* __restrict__ D_out,
    uint8_t* __restrict__ pred_out, const uint8_t* __restrict__ y_true, unsigned long long* __restrict__ counts) {
  constexpr int PB = PD_CHAIN;
  constexpr int KP = KT * 32;
  constexpr int PS = PB + 4;  // padded LDS row: conflict-free ds_read_b128 across comps
  constexpr int MAIN_F = KP * PS + 2 * PB;
  constexpr int TAB_D = KT == 1 ? 2048 : 256;  // doubles of LDA table that fit beside the gathered scores
  constexpr int EPI_F = PD_W * PD_R * (KP + 1) * 2 + TAB_D * 2;
  __shared__ __attribute__((aligned(16))) float smem[MAIN_F > EPI_F ? MAIN_F : EPI_F];
  __shared__ unsigned cnt[PD_CNT_LDS];
  __shared__ int lvl[PD_MAXLV];
  float* Pl = smem;            // [KP][PS]
  float* Mh = smem + KP * PS;  // [PB]
  float* Ml = Mh + PB;         // [PB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * PD_ROWS + wave * PD_R;
  const int64_t grow = row0 + l31;
  const int64_t gcl = grow < m ? grow : m - 1;  // rows past m read row m − 1; their results are dropped
  const float* xrow = X + (rows ? rows[gcl] : gcl) * ldx;

  auto ld4 = [&](const float* base, int col) -> f32x4 {
    if (VEC) return *reinterpret_cast<const f32x4*>(base + (col < p ? col : 0));
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = base[min(col + e, p - 1)];
    return v;
  };
  // stage projection / mean columns [b0, b0 + PB) into LDS (zero outside k, p)
  auto stage = [&](int b0) {
    __syncthreads();  // previous block fully consumed
    for (int e = tid; e < KP * (PB / 4); e += 256) {
      const int comp = e / (PB / 4), c4 = (e % (PB / 4)) * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (comp < k) v = ld4(P + (int64_t)comp * p, b0 + c4);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (b0 + c4 + q >= p) v[q] = 0.f;
      *reinterpret_cast<f32x4*>(&Pl[comp * PS + c4]) = v;
    }
    for (int c = tid; c < PB; c += 256) {
      Mh[c] = b0 + c < p ? mu_hi[b0 + c] : 0.f;
      Ml[c] = b0 + c < p ? mu_lo[b0 + c] : 0.f;
    }
    __syncthreads();
  };

  f32x16 accT[KT];
  double accT64[KT][16];
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      accT[t][r] = 0.f;
      accT64[t][r] = 0.0;
    }

  // Tᵀ = P · Yᵀ in 32-column chunks; the data of one chunk: d[i] = x[8i + 4h .. +3]
  // (MFMA step 4i + e uses column 8i + 4h + e for the data (B) and the projection (A) alike)
  struct S1 {
    f32x4 d[4];
  };
  auto load1 = [&](S1& S, int c0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) S.d[i] = ld4(xrow, c0 + 8 * i + 4 * h);
  };
  auto comp1 = [&](const S1& S, int c0, int b0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lc = c0 - b0 + 8 * i + 4 * h;  // column within the LDS block
      const f32x4 uh = *reinterpret_cast<const f32x4*>(&Mh[lc]);
      const f32x4 ul = *reinterpret_cast<const f32x4*>(&Ml[lc]);
      f32x4 w[KT];
#pragma unroll
      for (int t = 0; t < KT; ++t) w[t] = *reinterpret_cast<const f32x4*>(&Pl[(t * 32 + l31) * PS + lc]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // padded columns have w = 0 (and a finite, clamped x)
        const float y = __fsub_rn(__fsub_rn(S.d[i][e], uh[e]), ul[e]);
#pragma unroll
        for (int t = 0; t < KT; ++t) accT[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[t][e], y, accT[t], 0, 0, 0);
      }
    }
  };
  // PD_AHEAD chunks (4 KiB per wave each) are in flight ahead of the MFMAs, across the LDS
  // blocks: the X loads do not depend on the staging.  Loads past p are clamped and unused.
  static_assert(PD_AHEAD == 4 && PB % (32 * PD_AHEAD) == 0, "the ring below is written out for four buffers");
  S1 B0, B1, B2, B3;
  load1(B0, 0);
  load1(B1, 32);
  load1(B2, 64);
  load1(B3, 96);
  for (int b0 = 0; b0 < p; b0 += PB) {
    stage(b0);
    const int bend = min(b0 + PB, p);
    for (int c0 = b0; c0 < bend; c0 += 32 * PD_AHEAD) {
      comp1(B0, c0, b0);
      if (c0 + 128 < p) load1(B0, c0 + 128);
      if (c0 + 32 < bend) comp1(B1, c0 + 32, b0);
      if (c0 + 160 < p) load1(B1, c0 + 160);
      if (c0 + 64 < bend) comp1(B2, c0 + 64, b0);
      if (c0 + 192 < p) load1(B2, c0 + 192);
      if (c0 + 96 < bend) comp1(B3, c0 + 96, b0);
      if (c0 + 224 < p) load1(B3, c0 + 224);
    }
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accT64[t][r] += (double)accT[t][r];
        accT[t][r] = 0.f;
      }
  }

  // ---- epilogue: the wave's scores in LDS (fp64), accumulator layout
  // comp = 32t + (r&3) + 8(r>>2) + 4h, row = lane & 31
  double* tls = reinterpret_cast<double*>(smem);
  double* tab = tls + PD_W * PD_R * (KP + 1);
  const int ntab = nlv * C * (k + 1);
  const bool tab_lds = ntab <= TAB_D;
  const int ncnt = nlv * C * C;
  const bool cnt_lds = ncnt <= PD_CNT_LDS;
  __syncthreads();
  double* Tt = tls + wave * PD_R * (KP + 1);
#pragma unroll
  for (int t = 0; t < KT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int comp = t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      Tt[l31 * (KP + 1) + comp] = accT64[t][r];
    }
  if (tab_lds)
    for (int e = tid; e < ntab; e += 256) tab[e] = table[e];
  if (counts && cnt_lds)
    for (int e = tid; e < ncnt; e += 256) cnt[e] = 0u;
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < PD_MAXLV; ++e) lvl[e] = lvs.lv[e];
  }
  __syncthreads();
  const bool valid = grow < m;
  const double* trow = Tt + l31 * (KP + 1);
  if (T_out && valid && h == 0)
    for (int a = 0; a < k; ++a) T_out[grow * k + a] = (float)trow[a];
  const int yt = (counts && valid) ? (int)y_true[grow] : 255;

  auto sweep = [&](const double* coef, const double* icpt) {
    for (int l0 = 0; l0 < nlv; l0 += 2) {
      const int l = l0 + h;
      const bool act = valid && l < nlv;
      int key = -1;
      if (act) {
        const int lv = lvl[l];
        double best = 0.0;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
          const double* cf = coef + ((int64_t)l * C + c) * k;
          double d = 0.0;
          for (int a = 0; a < lv; ++a) d += cf[a] * trow[a];
          d += icpt[l * C + c];
          if (D_out) D_out[(grow * nlv + l) * C + c] = (float)d;
          if (c == 0 || d > best) {
            best = d;
            bi = c;
          }
        }
        if (pred_out) pred_out[grow * nlv + l] = (uint8_t)bi;
        if (yt < C) key = (l * C + yt) * C + bi;
      }
      if (counts) {  // one add per distinct (prefix, truth, prediction) of the wave
        unsigned long long live = __ballot(key >= 0);
        while (live) {
          const int leader = __ffsll((long long)live) - 1;
          const int kk = __shfl(key, leader, 64);
          const unsigned long long same = __ballot(key == kk);
          if (lane == leader) {
            const unsigned n = (unsigned)__popcll(same);
            if (cnt_lds)
              atomicAdd(&cnt[kk], n);
            else
              atomicAdd(&counts[kk], (unsigned long long)n);
          }
          live &= ~same;
        }
      }
    }
  };
  if (nlv > 0) {
    if (tab_lds)
      sweep(tab, tab + nlv * C * k);
    else
      sweep(table, table + (int64_t)nlv * C * k);
  }
  if (counts && cnt_lds) {
    __syncthreads();
    for (int e = tid; e < ncnt; e += 256) {
      const unsigned n = cnt[e];
      if (n) atomicAdd(&counts[e], (unsigned long long)n);
    }
  }
}

}  // namespace

extern "C" {

int ocm_pls_fit_f64(ocm_ctx* ctx, const double* S, const double* s, int32_t nprob, int32_t p, int32_t M, int32_t A,
                    double* W_out, double* R_out, double* P_out, double* q_out, double* tt_out, int32_t* ncomp_out,
                    void* stream) {
  OCM_REQUIRE(ctx && S && s && W_out && R_out && P_out && q_out && tt_out && ncomp_out,
              "ocm_pls_fit_f64: NULL argument");
  OCM_REQUIRE(nprob >= 1 && p >= 1 && M >= 1 && M <= PLS_MAXM, "ocm_pls_fit_f64: bad shape (nprob, p >= 1, 1 <= M <= 8)");
  OCM_REQUIRE(A >= 1 && A <= PLS_MAXA && A <= p, "ocm_pls_fit_f64: 1 <= A <= min(p, 64)");
  const int nrt = (p + PLS_MV_ROWS - 1) / PLS_MV_ROWS;
  OCM_REQUIRE((int64_t)nprob * nrt < (1LL << 31) && (int64_t)p * M < (1LL << 31),
              "ocm_pls_fit_f64: too many problems or columns for one call");
  hipStream_t st = (hipStream_t)stream;
  const size_t ws_bytes = (size_t)nprob * pls_ws_doubles(p, M) * sizeof(double);
  void* wsp = ocm::workspace(ctx, ws_bytes + (size_t)nprob * sizeof(int) + 512, st);
  if (!wsp) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(wsp)};
  double* ws = cv.take<double>((size_t)nprob * pls_ws_doubles(p, M));
  int* done = cv.take<int>(nprob);
  const size_t ap = (size_t)nprob * A * p * sizeof(double);
  OCM_HIP(hipMemsetAsync(done, 0, (size_t)nprob * sizeof(int), st));
  OCM_HIP(hipMemsetAsync(W_out, 0, ap, st));
  OCM_HIP(hipMemsetAsync(R_out, 0, ap, st));
  OCM_HIP(hipMemsetAsync(P_out, 0, ap, st));
  OCM_HIP(hipMemsetAsync(q_out, 0, (size_t)nprob * A * M * sizeof(double), st));
  OCM_HIP(hipMemsetAsync(tt_out, 0, (size_t)nprob * A * sizeof(double), st));
  OCM_HIP(hipMemsetAsync(ncomp_out, 0, (size_t)nprob * sizeof(int32_t), st));
  for (int a = 0; a <= A; ++a) {
    hipLaunchKernelGGL(k_pls_step, dim3(nprob), dim3(PLS_NT), 0, st, a, A, p, M, s, ws, done, W_out, R_out, P_out,
                       q_out, tt_out, ncomp_out);
    OCM_CHECK_LAUNCH("k_pls_step");
    if (a == A) break;
    hipLaunchKernelGGL(k_pls_matvec, dim3((unsigned)(nprob * nrt)), dim3(PLS_NT), 0, st, p, M, nrt, S, ws, done);
    OCM_CHECK_LAUNCH("k_pls_matvec");
  }
  return OCM_OK;
}

int ocm_plsda_predict_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                          const double* P, const double* mu, int32_t k, const int32_t* lvs, int32_t nlv, int32_t C,
                          const double* table, float* T_out, float* D_out, uint8_t* pred_out, const uint8_t* y_true,
                          int64_t* counts_out, void* stream) {
  OCM_REQUIRE(ctx && P && mu, "ocm_plsda_predict_f32: NULL argument");
  OCM_REQUIRE(X || m == 0, "ocm_plsda_predict_f32: X is NULL");
  OCM_REQUIRE(m >= 0 && p >= 1 && ldx >= p, "ocm_plsda_predict_f32: bad shape (m >= 0, p >= 1, ldx >= p)");
  OCM_REQUIRE(k >= 1 && k <= PD_MAXK, "ocm_plsda_predict_f32: 1 <= k <= 64");
  OCM_REQUIRE(nlv >= 0 && nlv <= PD_MAXLV, "ocm_plsda_predict_f32: 0 <= nlv <= 64");
  PdLvs lv{};
  if (nlv > 0) {
    OCM_REQUIRE(lvs && table, "ocm_plsda_predict_f32: lvs and table are needed when nlv > 0");
    OCM_REQUIRE(C >= 2 && C <= PD_MAXC, "ocm_plsda_predict_f32: 2 <= C <= 8");
    for (int l = 0; l < nlv; ++l) {
      OCM_REQUIRE(lvs[l] >= 1 && lvs[l] <= k && (l == 0 || lvs[l] >= lvs[l - 1]),
                  "ocm_plsda_predict_f32: lvs must be ascending in [1, k]");
      lv.lv[l] = (uint8_t)lvs[l];
    }
  } else {
    OCM_REQUIRE(!D_out && !pred_out && !counts_out, "ocm_plsda_predict_f32: D, pred and counts need nlv > 0");
  }
  OCM_REQUIRE(!counts_out || y_true || m == 0, "ocm_plsda_predict_f32: counts_out needs y_true");
  hipStream_t st = (hipStream_t)stream;
  if (counts_out) OCM_HIP(hipMemsetAsync(counts_out, 0, (size_t)nlv * C * C * sizeof(int64_t), st));
  if (m == 0) return OCM_OK;
  const int64_t nblk = (m + PD_ROWS - 1) / PD_ROWS;
  OCM_REQUIRE(nblk < (1LL << 31), "ocm_plsda_predict_f32: too many rows");
  void* w = ocm::workspace(ctx, ((size_t)k * p + 2 * (size_t)p) * sizeof(float) + 1024, st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  float* P32 = cv.take<float>((size_t)k * p);
  float* mu_hi = cv.take<float>(p);
  float* mu_lo = cv.take<float>(p);
  const int64_t nkp = (int64_t)k * p;
  hipLaunchKernelGGL(k_pd_cast, dim3((unsigned)((nkp + 255) / 256)), dim3(256), 0, st, P, nkp, P32, mu, p, mu_hi,
                     mu_lo);
  OCM_CHECK_LAUNCH("k_pd_cast");
  const bool vec = (ldx % 4 == 0) && (p % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts_out);
  {
    ocm::TimedRegion tr(ctx, OCM_KERNEL_SCORE, st);
#define OCM_PD_LAUNCH(KT_, V_)                                                                                    \
  hipLaunchKernelGGL((k_plsda_predict<KT_, V_>), dim3((unsigned)nblk), dim3(256), 0, st, X, ldx, rows, m, p, P32, \
                     mu_hi, mu_lo, k, nlv, lv, C, table, T_out, D_out, pred_out, y_true, cnt)
    if (k <= 32) {
      if (vec) OCM_PD_LAUNCH(1, true); else OCM_PD_LAUNCH(1, false);
    } else {
      if (vec) OCM_PD_LAUNCH(2, true); else OCM_PD_LAUNCH(2, false);
    }
#undef OCM_PD_LAUNCH
  }
  OCM_CHECK_LAUNCH("k_plsda_predict");
  return OCM_OK;
}

}  // extern "C"
