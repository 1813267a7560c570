// K2 — top-k eigenpairs of the class covariance and the tail moments θ1..θ3.
//
// The reference gets every eigenvalue from a full float32 SVD of the centred
// class matrix (utils/SIMCA.py:64-66, explained_variance_ = S²/(n-1),
// sklearn/decomposition/_pca.py:584) and then uses only the leading k
// loadings (:66) plus Σ_{i>k} λ^m (m=1..3) for the Jackson–Mudholkar /
// Box / ci limits (:189-191, 203-204, 226-227).  Here:
//   * subspace iteration with Rayleigh–Ritz on C (p×p fp64, HBM-resident):
//     one C·V product per step (fp64 MFMA), the b×b projected problem by
//     one-workgroup cyclic Jacobi in LDS, re-orthonormalisation by CholQR2;
//   * θ_m from the deflated matrix C⊥ = (I-VVᵀ)C(I-VVᵀ): θ1 = tr C⊥,
//     θ2 = ‖C⊥‖²_F, θ3 = tr(C⊥³) (one fp64-MFMA p³ product with a fused
//     trace epilogue) — no full spectrum, no catastrophic cancellation
//     against the leading eigenvalues;
//   * p ≤ 64 (VAE latents, tiny spectra): Jacobi on C directly.
#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <limits>
#include <vector>

#include "ocm_hostla.h"
#include "ocm_internal.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

// ---------------------------------------------------------------------------
// fp64 MFMA GEMM  D = A·B  (row-major, NN), 64×64 tile, BK = 16.
// MODE 0: store (split-K: z-slice writes its own partial plane)
// MODE 1: trace epilogue  part[wg] = w · Σ_{tile} (A·B)_{ij} · E_{ij}; A·B
//         and E symmetric: the grid is the upper triangle of tiles
//         (blockIdx.x linear), off-diagonal tiles weighted 2
// MODE 2: rank update  D = E − A·B, part[2wg..] = {Σ diag D, Σ D²}
// TA: A is given transposed (A(r, kk) = A[kk·lda + r]) — the b×b projections
// VᵀW of tall p×b blocks when b > 64 (MODE 0 only).
// tile0 (MODE 1): first upper-triangle tile of this launch (a rank's slice of
// the trace GEMM when the θ3 work is split over GPUs).
// ---------------------------------------------------------------------------
using ocm_eig::CQ_G;  // the eigensolver's constants that its workspace plan shares (ocm_eig_plan.h)
using ocm_eig::CVQ_G1;
using ocm_eig::DT;
using ocm_eig::JMAX;
using ocm_eig::QB;
constexpr int DBK = 16, DPAD = 16;
#ifndef OCM_JACOBI_TOL2
#define OCM_JACOBI_TOL2 1e-26  // Jacobi stop: off-diagonal ‖·‖² ≤ this × diagonal ‖·‖²
#endif

// MODE 3: as MODE 2 without storing D in fp64: the off-diagonal part goes to
//         O32 (float32, zero diagonal, row-major p×p), the diagonal to D[row],
//         each row's Σ_{col≠row} D² over this tile's 64 columns to
//         rowpart[blockIdx.y·M + row] (the θ3 expansion's Δ terms), plus the
//         {Σ diag, Σ D²} pair partials of MODE 2.
template <int MODE, bool TA = false>
__global__ __launch_bounds__(256) void k_dgemm(const double* __restrict__ A, int64_t lda, const double* __restrict__ B,
                                               int64_t ldb, double* __restrict__ D, int64_t ldd, int M, int N, int K,
                                               int kper, const double* __restrict__ E, int64_t lde,
                                               double* __restrict__ part, int tile0 = 0,
                                               float* __restrict__ O32 = nullptr,
                                               double* __restrict__ rowpart = nullptr) {
  __shared__ double As[DBK][DT + DPAD];
  __shared__ double Bs[DBK][DT + DPAD];
  __shared__ double red[8];
  __shared__ double rsum[2][2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int bx = blockIdx.x, by = blockIdx.y;
  double wtile = 1.0;
  if (MODE == 1) {  // linear upper-triangle index -> (bx <= by)
    const int nt = (N + DT - 1) / DT;
    int rem = blockIdx.x + tile0;
    bx = 0;
    while (rem >= nt - bx) {
      rem -= nt - bx;
      ++bx;
    }
    by = bx + rem;
    wtile = bx == by ? 1.0 : 2.0;
  }
  const int m0 = bx * DT, n0 = by * DT;
  const int kb = blockIdx.z * kper, ke = min(K, kb + kper);
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

  const int arow = tid >> 2, akc = (tid & 3) * 4;   // A: 64 rows × 16 k
  const int bk = tid >> 4, bcol = (tid & 15) * 4;   // B: 16 k × 64 cols
  // register prefetch: the next K-step's operands are loaded before this
  // step's MFMAs, so global latency hides behind them
  double ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = m0 + arow, kk = k0 + akc + e;
      if (TA) {  // 64 rows × 16 k from Aᵀ: lanes walk r (contiguous in A)
        const int r2 = m0 + (tid & 63), kk2 = k0 + (tid >> 6) * 4 + e;
        ra[e] = (r2 < M && kk2 < ke) ? A[(int64_t)kk2 * lda + r2] : 0.0;
      } else {
        ra[e] = (r < M && kk < ke) ? A[(int64_t)r * lda + kk] : 0.0;
      }
      const int kr = k0 + bk, c = n0 + bcol + e;
      rb[e] = (kr < ke && c < N) ? B[(int64_t)kr * ldb + c] : 0.0;
    }
  };
  if (kb < ke) gload(kb);
  for (int k0 = kb; k0 < ke; k0 += DBK) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (TA)
        As[(tid >> 6) * 4 + e][tid & 63] = ra[e];
      else
        As[akc + e][arow] = ra[e];
      Bs[bk][bcol + e] = rb[e];
    }
    __syncthreads();
    if (k0 + DBK < ke) gload(k0 + DBK);
#pragma unroll
    for (int kq = 0; kq < DBK / 4; ++kq) {
      const int kr = kq * 4 + (lane >> 4);
      const double a0 = As[kr][wm * 32 + (lane & 15)];
      const double a1 = As[kr][wm * 32 + 16 + (lane & 15)];
      const double b0 = Bs[kr][wn * 32 + (lane & 15)];
      const double b1 = Bs[kr][wn * 32 + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
  double tr = 0.0, fro = 0.0;
  double rs[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // f64 16x16x4 C/D map: col = lane&15, row = (lane>>4) + 4*reg
        const int row = m0 + wm * 32 + a * 16 + (lane >> 4) + 4 * r;
        const int col = n0 + wn * 32 + b * 16 + (lane & 15);
        if (row < M && col < N) {
          if (MODE == 0) {
            D[(int64_t)blockIdx.z * M * ldd + (int64_t)row * ldd + col] = acc[a][b][r];
          } else if (MODE == 1) {
            tr += acc[a][b][r] * E[(int64_t)row * lde + col];
          } else if (MODE == 3) {
            const double v = E[(int64_t)row * lde + col] - acc[a][b][r];
            fro += v * v;
            if (row == col) {
              tr += v;
              D[row] = v;
              O32[(int64_t)row * N + col] = 0.f;
            } else {
              O32[(int64_t)row * N + col] = (float)v;
              rs[a][r] += v * v;
            }
          } else {
            const double v = E[(int64_t)row * lde + col] - acc[a][b][r];
            D[(int64_t)row * ldd + col] = v;
            fro += v * v;
            if (row == col) tr += v;
          }
        }
      }
  if (MODE == 3) {
    // row sums over the 16 column lanes of each row, then the two column waves
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double v = rs[a][r];
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        if ((lane & 15) == 0) rsum[wm][wn][a * 16 + (lane >> 4) + 4 * r] = v;
      }
    __syncthreads();
    if (tid < 64) {
      const int row = m0 + tid;
      if (row < M) rowpart[(int64_t)by * M + row] = rsum[tid >> 5][0][tid & 31] + rsum[tid >> 5][1][tid & 31];
    }
  }
  if (MODE >= 1) {
    tr = wave_sum_f64(tr);
    if (MODE >= 2) fro = wave_sum_f64(fro);
    if (lane == 0) {
      red[wave] = tr;
      red[4 + wave] = fro;
    }
    __syncthreads();
    if (tid == 0) {
      if (MODE == 1) {
        part[blockIdx.z * gridDim.x + blockIdx.x] = wtile * ((red[0] + red[1]) + (red[2] + red[3]));
      } else {
        const int wg = blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * wg] = (red[0] + red[1]) + (red[2] + red[3]);
        part[2 * wg + 1] = (red[4] + red[5]) + (red[6] + red[7]);
      }
    }
  }
}

// k_dgemm<3> for K ≤ 64 (the fused path's rank-2b deflation, b = 32): every
// global load is issued up front — the four K-steps' A / B pieces and this
// thread's 16 elements of E (C) for the epilogue — so one memory latency
// covers the workgroup instead of one per K-step plus one for E; the K-steps
// then run from registers through LDS.  Same outputs as k_dgemm<3>.
__global__ __launch_bounds__(256, 4) void k_deflate64(const double* __restrict__ A, int64_t lda,
                                                   const double* __restrict__ B, int64_t ldb,
                                                   double* __restrict__ D, int M, int N, int K,
                                                   const double* __restrict__ E, int64_t lde,
                                                   double* __restrict__ part, float* __restrict__ O32,
                                                   double* __restrict__ rowpart) {
  constexpr int NS = 64 / DBK;  // K-steps
  __shared__ double As[DBK][DT + DPAD];
  __shared__ double Bs[DBK][DT + DPAD];
  __shared__ double red[8];
  __shared__ double rsum[2][2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * DT, n0 = blockIdx.y * DT;
  const int arow = tid >> 2, akc = (tid & 3) * 4;
  const int bk = tid >> 4, bcol = (tid & 15) * 4;
  // E's 16 elements are loaded after the K-steps: preloaded, they held the
  // kernel at 2 workgroups per CU (216 registers), two rounds of workgroups
  // for the 1024 tiles at p = 2048 and no room for the Jacobi workgroup that
  // runs beside it (r05s5); at ≤ 128 it is 4 per CU, one round
  double ev[2][2][4];
  double ra[NS][4], rb[NS][4];
#pragma unroll
  for (int st = 0; st < NS; ++st)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = m0 + arow, kk = st * DBK + akc + e;
      ra[st][e] = (r < M && kk < K) ? A[(int64_t)r * lda + kk] : 0.0;
      const int kr = st * DBK + bk, c = n0 + bcol + e;
      rb[st][e] = (kr < K && c < N) ? B[(int64_t)kr * ldb + c] : 0.0;
    }
  f64x4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int st = 0; st < NS; ++st) {
    if (st * DBK >= K) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      As[akc + e][arow] = ra[st][e];
      Bs[bk][bcol + e] = rb[st][e];
    }
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < DBK / 4; ++kq) {
      const int kr = kq * 4 + (lane >> 4);
      const double a0 = As[kr][wm * 32 + (lane & 15)];
      const double a1 = As[kr][wm * 32 + 16 + (lane & 15)];
      const double b0 = Bs[kr][wn * 32 + (lane & 15)];
      const double b1 = Bs[kr][wn * 32 + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 32 + a * 16 + (lane >> 4) + 4 * r;
        const int col = n0 + wn * 32 + b * 16 + (lane & 15);
        ev[a][b][r] = (row < M && col < N) ? E[(int64_t)row * lde + col] : 0.0;
      }
  double tr = 0.0, fro = 0.0;
  double rs[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 32 + a * 16 + (lane >> 4) + 4 * r;
        const int col = n0 + wn * 32 + b * 16 + (lane & 15);
        if (row < M && col < N) {
          const double v = ev[a][b][r] - acc[a][b][r];
          fro += v * v;
          if (row == col) {
            tr += v;
            D[row] = v;
            O32[(int64_t)row * N + col] = 0.f;
          } else {
            O32[(int64_t)row * N + col] = (float)v;
            rs[a][r] += v * v;
          }
        }
      }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double v = rs[a][r];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if ((lane & 15) == 0) rsum[wm][wn][a * 16 + (lane >> 4) + 4 * r] = v;
    }
  __syncthreads();
  if (tid < 64) {
    const int row = m0 + tid;
    if (row < M) rowpart[(int64_t)blockIdx.y * M + row] = rsum[tid >> 5][0][tid & 31] + rsum[tid >> 5][1][tid & 31];
  }
  tr = wave_sum_f64(tr);
  fro = wave_sum_f64(fro);
  if (lane == 0) {
    red[wave] = tr;
    red[4 + wave] = fro;
  }
  __syncthreads();
  if (tid == 0) {
    const int wg = blockIdx.y * gridDim.x + blockIdx.x;
    part[2 * wg] = (red[0] + red[1]) + (red[2] + red[3]);
    part[2 * wg + 1] = (red[4] + red[5]) + (red[6] + red[7]);
  }
}

// ---------------------------------------------------------------------------
// W = C·V for a 32-column block (the subspace iteration's product, b = 32):
// two workgroups of eight waves per 16 rows of C, each a half of K, each wave
// a sixteenth of K in 32-column groups.  Lane (i, g) holds C[r0 + i][k0 + 8g
// .. k0 + 8g + 7] (64 contiguous bytes) and V rows k0 + 8g + s, columns i and
// 16 + i; MFMA s of a group pairs K-slot g with column k0 + 8g + s for both
// operands (v_mfma_f64_16x16x4f64).  The eight wave partials meet in LDS in a
// fixed order; the second workgroup of a row block to finish (a parity
// ticket per row block) adds the first one's partial: half 0 + half 1 in
// either case, so the result does not depend on which finishes first.  One
// launch instead of the generic 64×64-tile GEMM (half its columns idle at
// b = 32) plus a split-K plane sum: 16 µs against 19 + 6 µs (r03y).  The
// publish is one agent-scope release by one lane (a __threadfence() in every
// thread measured 77 µs per launch).
// ---------------------------------------------------------------------------
constexpr int CV_W = 8;  // waves per workgroup
// AX (a Chebyshev filter step, below): W = a·(C·V) + bb·V + gc·Vg instead of C·V
template <bool AX>
__device__ __forceinline__ void cv32_body(const double* __restrict__ C, int p, const double* __restrict__ V,
                                          double* __restrict__ W, double* __restrict__ part,
                                          unsigned* __restrict__ ticket, double a, double bb,
                                          const double* __restrict__ Vg, double gc) {
  __shared__ double red[CV_W][16 * 33];
  __shared__ int last;
  const int rb = blockIdx.x >> 1, half = blockIdx.x & 1;
  const int r0 = rb * 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, g = lane >> 4;
  const int kslice = (p + 2 * CV_W * 32 - 1) / (2 * CV_W * 32) * 32;
  const int kb = (half * CV_W + wave) * kslice;
  const int ke = min(p, kb + kslice);
  const double* crow = C + (int64_t)min(r0 + i, p - 1) * p;
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
  // (loading the next group before this group's MFMAs measured 18.1 vs 16.1 µs)
  for (int k0 = kb; k0 < ke; k0 += 32) {
    double a[8], b0[8], b1[8];
    const int kk0 = k0 + 8 * g;
    if (k0 + 32 <= ke) {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        a[s] = crow[kk0 + s];
        b0[s] = V[(int64_t)(kk0 + s) * 32 + i];
        b1[s] = V[(int64_t)(kk0 + s) * 32 + 16 + i];
      }
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int kk = kk0 + s;
        const bool ok = kk < ke;
        a[s] = ok ? crow[kk] : 0.0;
        b0[s] = ok ? V[(int64_t)kk * 32 + i] : 0.0;
        b1[s] = ok ? V[(int64_t)kk * 32 + 16 + i] : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b1[s], acc1, 0, 0, 0);
    }
  }
  // f64 16x16x4 C/D map: col = lane&15, row = (lane>>4) + 4*reg
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wave][(g + 4 * r) * 33 + i] = acc0[r];
    red[wave][(g + 4 * r) * 33 + 16 + i] = acc1[r];
  }
  __syncthreads();
  const int orow = tid >> 5, ocol = tid & 31;
  double v = 0.0;
#pragma unroll
  for (int w = 0; w < CV_W; ++w) v += red[w][orow * 33 + ocol];
  part[(int64_t)blockIdx.x * 512 + tid] = v;
  // publish: every wave drains its stores, then one agent-scope release and
  // the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = (__hip_atomic_fetch_add(&ticket[rb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) == 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  const double o = part[(int64_t)(blockIdx.x ^ 1) * 512 + tid];
  if (r0 + orow < p) {
    const int64_t e = (int64_t)(r0 + orow) * 32 + ocol;
    const double cv = half == 0 ? v + o : o + v;
    if constexpr (AX)
      W[e] = fma(a, cv, fma(bb, V[e], Vg ? gc * Vg[e] : 0.0));
    else
      W[e] = cv;
  }
}
__global__ __launch_bounds__(512) void k_cv32(const double* __restrict__ C, int p, const double* __restrict__ V,
                                            double* __restrict__ W, double* __restrict__ part,
                                            unsigned* __restrict__ ticket) {
  cv32_body<false>(C, p, V, W, part, ticket, 1.0, 0.0, nullptr, 0.0);
}
// one step of the three-term Chebyshev recurrence on the block (eig_topk's
// filtered iterations): W = a·(C·V) + bb·V + g·Vg (Vg nullable), the product as
// k_cv32's
__global__ __launch_bounds__(512) void k_cv32x(const double* __restrict__ C, int p, const double* __restrict__ V,
                                             double* __restrict__ W, double* __restrict__ part,
                                             unsigned* __restrict__ ticket, double a, double bb,
                                             const double* __restrict__ Vg, double g) {
  cv32_body<true>(C, p, V, W, part, ticket, a, bb, Vg, g);
}

// sum of split-K planes: D[i] = Σ_z P[z][i]
__global__ void k_sum_planes(const double* __restrict__ P, int nz, int64_t plane, double* __restrict__ D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  double v = 0.0;
  for (int z = 0; z < nz; ++z) v += P[(int64_t)z * plane + i];
  D[i] = v;
}

// partial  S = Aᵀ B  for tall row-major A, B (p×b, ld = b): block = 64 rows
__global__ __launch_bounds__(256) void k_atb_part(const double* __restrict__ A, const double* __restrict__ B, int p,
                                                  int b, double* __restrict__ part) {
  __shared__ double sa[64][65];
  __shared__ double sb[64][65];
  const int r0 = blockIdx.x * 64;
  for (int e = threadIdx.x; e < 64 * b; e += 256) {
    const int r = e / b, c = e % b;
    const bool ok = r0 + r < p;
    sa[r][c] = ok ? A[(int64_t)(r0 + r) * b + c] : 0.0;
    sb[r][c] = ok ? B[(int64_t)(r0 + r) * b + c] : 0.0;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < b * b; o += 256) {
    const int i = o / b, j = o % b;
    double v = 0.0;
#pragma unroll 8
    for (int r = 0; r < 64; ++r) v += sa[r][i] * sb[r][j];
    part[(int64_t)blockIdx.x * b * b + o] = v;
  }
}

// ---------------------------------------------------------------------------
// One-workgroup cyclic Jacobi for a symmetric n×n fp64 matrix, n ≤ 64 (even;
// an odd input is padded with a zero row/column).  Round-robin ordering: in
// each of the n-1 rounds every index is in exactly one rotation pair.
// Outputs eigenvalues (descending) and Z (n_in×n_in, column j = eigenvector j).
// ---------------------------------------------------------------------------

// NF > 0: compile-time padded size (index arithmetic folds); NT threads
// (64 = one wave: the per-round barriers reduce to LDS waits).
template <int NF, int NT>
__global__ __launch_bounds__(NT) void k_jacobi(const double* __restrict__ Ain, int n_in, int max_sweeps,
                                               double* __restrict__ evals, double* __restrict__ Zout,
                                               int* __restrict__ sweeps_out) {
  constexpr int NW = NT / 64;
  __shared__ double A[JMAX][JMAX + 1];
  __shared__ double Z[JMAX][JMAX + 1];
  __shared__ double rc[JMAX], rs[JMAX];
  __shared__ int pp[JMAX / 2], qq[JMAX / 2];
  __shared__ double wsum[2 * NW];
  __shared__ int done;
  const int n = NF > 0 ? NF : (n_in + 1) & ~1;
  const int tid = threadIdx.x;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e % n;
    A[i][j] = (i < n_in && j < n_in) ? 0.5 * (Ain[i * n_in + j] + Ain[j * n_in + i]) : 0.0;
    Z[i][j] = (i == j) ? 1.0 : 0.0;
  }
  __syncthreads();
  const int half = n / 2;
  int sweep = 0;
  for (; sweep < max_sweeps; ++sweep) {
    // convergence test: off(A)² ≤ (1e-15)² · Σ diag²  (relative to the scale of A)
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < n * n; e += NT) {
      const int i = e / n, j = e % n;
      const double v = A[i][j] * A[i][j];
      if (i == j) dg += v; else off += v;
    }
    off = wave_sum_f64(off);
    dg = wave_sum_f64(dg);
    if ((tid & 63) == 0) {
      wsum[tid >> 6] = off;
      wsum[NW + (tid >> 6)] = dg;
    }
    __syncthreads();
    if (tid == 0) {
      double o = 0.0, d = 0.0;
      for (int w = 0; w < NW; ++w) {
        o += wsum[w];
        d += wsum[NW + w];
      }
      // off-diagonal norm ≤ 1e-13 of the diagonal's: eigenvalue error ~ off²/gap
      done = (o <= OCM_JACOBI_TOL2 * d) || (o == 0.0);
    }
    __syncthreads();
    if (done) break;
    for (int round = 0; round < n - 1; ++round) {
      if (tid < half) {
        // positions: idx[0] = 0, idx[t] = 1 + (t - 1 + round) mod (n - 1)
        auto idx = [&](int t) { return t == 0 ? 0 : 1 + (t - 1 + round) % (n - 1); };
        int p = idx(tid), q = idx(n - 1 - tid);
        if (p > q) { const int t = p; p = q; q = t; }
        pp[tid] = p;
        qq[tid] = q;
        const double apq = A[p][q];
        double c = 1.0, s = 0.0;
        if (apq != 0.0) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          c = 1.0 / sqrt(t * t + 1.0);
          s = t * c;
        }
        rc[tid] = c;
        rs[tid] = s;
      }
      __syncthreads();
      // rows:  A ← Jᵀ A
      for (int e = tid; e < half * n; e += NT) {
        const int k = e / n, j = e % n;
        const int p = pp[k], q = qq[k];
        const double c = rc[k], s = rs[k];
        const double ap = A[p][j], aq = A[q][j];
        A[p][j] = c * ap - s * aq;
        A[q][j] = s * ap + c * aq;
      }
      __syncthreads();
      // columns: A ← A J, Z ← Z J
      for (int e = tid; e < half * n; e += NT) {
        const int i = e / half, k = e % half;
        const int p = pp[k], q = qq[k];
        const double c = rc[k], s = rs[k];
        const double ap = A[i][p], aq = A[i][q];
        A[i][p] = c * ap - s * aq;
        A[i][q] = s * ap + c * aq;
        const double zp = Z[i][p], zq = Z[i][q];
        Z[i][p] = c * zp - s * zq;
        Z[i][q] = s * zp + c * zq;
      }
      __syncthreads();
    }
  }
  // sort descending (stable): rank by value then index
  for (int i = tid; i < n_in; i += NT) {
    const double li = A[i][i];
    int rank = 0;
    for (int j = 0; j < n_in; ++j) {
      const double lj = A[j][j];
      rank += (lj > li) || (lj == li && j < i);
    }
    evals[rank] = li;
    for (int r = 0; r < n_in; ++r) Zout[r * n_in + rank] = Z[r][i];
  }
  if (tid == 0 && sweeps_out) *sweeps_out = sweep;
}

// ---------------------------------------------------------------------------
// Block-parallel Jacobi (NF = 32/48/64, compile-time).  Parallel ordering in
// storage: rotation pair k always occupies slots (2k, 2k+1); after each round
// the contents move to the round-robin tournament's next slots (a fixed
// permutation `jdest`), written into a ping-pong buffer.  One thread updates a
// whole 2×2 block with both the row and the column rotation (and writes the
// mirrored block), so a round is: rotations → barrier → block update →
// barrier.  Slot order is irrelevant for the output (sorted at the end).
// ---------------------------------------------------------------------------
template <int NF>
__device__ __forceinline__ int jdest(int s) {
  // slot -> tournament position; position t shifts to t-1 (1 -> NF-1, 0 fixed)
  const int t = (s & 1) ? NF - 1 - (s >> 1) : (s >> 1);
  const int t2 = t == 0 ? 0 : (t == 1 ? NF - 1 : t - 1);
  return t2 < NF / 2 ? 2 * t2 : 2 * (NF - 1 - t2) + 1;
}

template <int NF>
__global__ __launch_bounds__(256) void k_jacobi_blk(const double* __restrict__ Ain, int max_sweeps,
                                                    double* __restrict__ evals, double* __restrict__ Zout,
                                                    int* __restrict__ sweeps_out) {
  constexpr int H = NF / 2, NB = H * (H + 1) / 2, LD = NF + 1;
  __shared__ double A[2][NF][LD];
  __shared__ double Z[2][NF][LD];
  __shared__ double rc[H], rs[H];
  __shared__ unsigned char bk[NB], bl[NB];
  __shared__ double wsum[8];
  __shared__ int done;
  const int tid = threadIdx.x;
  for (int e = tid; e < NF * NF; e += 256) {
    const int i = e / NF, j = e % NF;
    A[0][i][j] = 0.5 * (Ain[i * NF + j] + Ain[j * NF + i]);
    Z[0][i][j] = (i == j) ? 1.0 : 0.0;
  }
  if (tid == 0) {
    int b = 0;
    for (int k = 0; k < H; ++k)
      for (int l = k; l < H; ++l) {
        bk[b] = (unsigned char)k;
        bl[b] = (unsigned char)l;
        ++b;
      }
  }
  __syncthreads();
  int cur = 0, sweep = 0;
  for (; sweep < max_sweeps; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < NF * NF; e += 256) {
      const int i = e / NF, j = e % NF;
      const double v = A[cur][i][j] * A[cur][i][j];
      if (i == j) dg += v; else off += v;
    }
    off = wave_sum_f64(off);
    dg = wave_sum_f64(dg);
    if ((tid & 63) == 0) {
      wsum[tid >> 6] = off;
      wsum[4 + (tid >> 6)] = dg;
    }
    __syncthreads();
    if (tid == 0) {
      const double o = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
      const double d = (wsum[4] + wsum[5]) + (wsum[6] + wsum[7]);
      // off-diagonal norm ≤ 1e-13 of the diagonal's: eigenvalue error ~ off²/gap
      done = (o <= OCM_JACOBI_TOL2 * d) || (o == 0.0);
    }
    __syncthreads();
    if (done) break;
    for (int round = 0; round < NF - 1; ++round) {
      if (tid < H) {
        const double app = A[cur][2 * tid][2 * tid], aqq = A[cur][2 * tid + 1][2 * tid + 1];
        const double apq = A[cur][2 * tid][2 * tid + 1];
        double c = 1.0, sn = 0.0;
        if (apq != 0.0) {
          // t = sgn(θ)/(|θ| + √(θ² + 1)), θ = d/e (d = aqq − app, e = 2apq), c = 1/√(1 + t²),
          // s = t·c, rewritten with u = |d| + √(d² + e²): c = u/√(u² + e²), s = ±e/√(u² + e²)
          // — one square root and one reciprocal square root on the round's serial
          // path instead of three divisions and two square roots
          const double d = aqq - app, e = 2.0 * apq;
          // (the unrefined v_sqrt_f64 / v_rsq_f64 save ≈ 10 µs per solve but
          // leave the rotations 1e-6 from orthogonal: eigenvalues off by
          // 2.4e-6, round 5 — the refined forms stay)
          const double u = fabs(d) + sqrt(fma(d, d, e * e));
          const double w = rsqrt(fma(u, u, e * e));
          c = u * w;
          sn = (d >= 0.0 ? e : -e) * w;
        }
        rc[tid] = c;
        rs[tid] = sn;
      }
      __syncthreads();
      const int nx = cur ^ 1;
      for (int b = tid; b < NB; b += 256) {
        const int k = bk[b], l = bl[b];
        const double ck = rc[k], sk = rs[k], cl = rc[l], sl = rs[l];
        const int p = 2 * k, q = 2 * k + 1, u = 2 * l, v = 2 * l + 1;
        const double a00 = A[cur][p][u], a01 = A[cur][p][v], a10 = A[cur][q][u], a11 = A[cur][q][v];
        // rows (pair k): B = Jkᵀ A
        const double b00 = ck * a00 - sk * a10, b01 = ck * a01 - sk * a11;
        const double b10 = sk * a00 + ck * a10, b11 = sk * a01 + ck * a11;
        // columns (pair l): B Jl
        double o00 = cl * b00 - sl * b01, o01 = sl * b00 + cl * b01;
        double o10 = cl * b10 - sl * b11, o11 = sl * b10 + cl * b11;
        if (k == l) {  // the rotated pair: exact zero off-diagonal
          o01 = 0.0;
          o10 = 0.0;
        }
        const int dp = jdest<NF>(p), dq = jdest<NF>(q), du = jdest<NF>(u), dv = jdest<NF>(v);
        A[nx][dp][du] = o00;
        A[nx][dp][dv] = o01;
        A[nx][dq][du] = o10;
        A[nx][dq][dv] = o11;
        if (k != l) {
          A[nx][du][dp] = o00;
          A[nx][dv][dp] = o01;
          A[nx][du][dq] = o10;
          A[nx][dv][dq] = o11;
        }
      }
      // Z ← Z J (columns = slots; rows = coordinates, not permuted)
      for (int e = tid; e < NF * H; e += 256) {
        const int r = e / H, l = e % H;
        const double cl = rc[l], sl = rs[l];
        const double zp = Z[cur][r][2 * l], zq = Z[cur][r][2 * l + 1];
        Z[nx][r][jdest<NF>(2 * l)] = cl * zp - sl * zq;
        Z[nx][r][jdest<NF>(2 * l + 1)] = sl * zp + cl * zq;
      }
      __syncthreads();
      cur = nx;
    }
  }
  for (int i = tid; i < NF; i += 256) {
    const double li = A[cur][i][i];
    int rank = 0;
    for (int j = 0; j < NF; ++j) {
      const double lj = A[cur][j][j];
      rank += (lj > li) || (lj == li && j < i);
    }
    evals[rank] = li;
    for (int r = 0; r < NF; ++r) Zout[r * NF + rank] = Z[cur][r][i];
  }
  if (tid == 0 && sweeps_out) *sweeps_out = sweep;
}

// ---------------------------------------------------------------------------
// The 32×32 block Jacobi with ONE barrier per round (the RR eigensolve's
// serial step).  k_jacobi_blk's round was: 16 threads compute the rotations →
// LDS → barrier → block update → barrier.  Here every updating thread computes
// the (one or two) rotations it applies itself, from the round's 2×2 diagonal
// blocks (broadcast LDS reads), so the rotations' LDS hand-off and its barrier
// go; the ping-pong buffers make the remaining barrier the only one.  Threads
// 0..135: the 136 2×2 blocks (k ≤ l) of A; threads 192..319: Z ← Z J, pair
// l = t & 15 on rows t/16 + 8i.  The rotation: t = tan φ from the fast
// (unrefined) v_rsq / v_rcp — t only decides how well a_pq is annihilated —
// and c = 1/√(1 + t²) refined, s = t·c, so c² + s² = 1 to rounding: every
// rotation stays orthogonal and A's spectrum is untouched.  The rotated
// pair's off-diagonal is therefore computed, not set to zero (its remainder,
// ~1e-7·a_pq, is taken by the later rounds).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void jrot_fast(double app, double aqq, double apq, double& c, double& s) {
  const double d = aqq - app, e = 2.0 * apq;
  const double h = fma(d, d, e * e);
  c = 1.0;
  s = 0.0;
  if (apq != 0.0 && h > 0.0) {
    const double u = fabs(d) + h * __builtin_amdgcn_rsq(h);     // |d| + √(d² + e²), approximately
    const double t = (d >= 0.0 ? e : -e) * __builtin_amdgcn_rcp(u);  // |t| ≤ 1
    c = rsqrt(fma(t, t, 1.0));
    s = t * c;
  }
}

// S (optional): the Rayleigh–Ritz test fused at the end — the former k_rr_test32's
// res[i] = √max(z_iᵀ S z_i, 0) for the first k Ritz pairs, the same sums in
// the same order — with S taken in flight from k_rr_resid32 on another
// stream once *sflag reaches epoch.  The wait is bounded (≈ 1 s): on a
// timeout the residuals are written as −1 (valid ones are ≥ 0), and the host
// runs the Jacobi and its test again behind the producer's event instead of
// hanging or mistaking the timeout for bad data
#define OCM_JACOBI_SPINS_1S (1u << 22)  // ≈ 1 s of s_sleep(8) polls
#ifndef OCM_JACOBI_WAIT_SPINS           // (make exp: 0 gives up at once, to exercise the re-run)
#define OCM_JACOBI_WAIT_SPINS OCM_JACOBI_SPINS_1S
#endif
#ifdef OCM_JACOBI_STAMPS  // make exp diagnostic: wall-clock stamps of k_jacobi_1b's phases (100 MHz)
__device__ unsigned long long g_jac_st[16][64];
// wave 0 stores the stamp at 64 lane addresses (a vector store)
#define JAC_STAMP(slot_)                                              \
  do {                                                                \
    if (tid < 64) g_jac_st[(slot_)][tid] = wall_clock64();           \
  } while (0)
#else
#define JAC_STAMP(slot_)
#endif
template <int NF>
__global__ __launch_bounds__(320) void k_jacobi_1b(const double* __restrict__ Ain, int max_sweeps,
                                                   double* __restrict__ evals, double* __restrict__ Zout,
                                                   int* __restrict__ sweeps_out, const double* __restrict__ S,
                                                   const unsigned* __restrict__ sflag, unsigned epoch, int ktest,
                                                   double* __restrict__ res, unsigned max_spins) {
  static_assert(NF == 32, "thread map for 32×32");
  constexpr int H = NF / 2, NB = H * (H + 1) / 2, LD = NF + 1, NT = 320, ZT0 = 192;
  __shared__ double A[2][NF][LD];
  __shared__ double Z[2][NF][LD];
  __shared__ double wsum[10];
  __shared__ int done;
  const int tid = threadIdx.x;
  // the top issue priority: this one workgroup shares its CU with the θ3
  // chain's (deflation, quantiser, Gram) waves, which took ≈ 20 % of its issue
  // slots (128 against 107 µs alone, r05s4)
  __builtin_amdgcn_s_setprio(3);
  JAC_STAMP(0);
  for (int e = tid; e < NF * NF; e += NT) {
    const int i = e / NF, j = e % NF;
    A[0][i][j] = 0.5 * (Ain[i * NF + j] + Ain[j * NF + i]);
    Z[0][i][j] = (i == j) ? 1.0 : 0.0;
  }
  // this thread's block (k, l), k ≤ l (row-major over the upper triangle), or Z pair
  int k = 0, l = 0;
  if (tid < NB) {
    int b = tid;
    while (b >= H - k) {
      b -= H - k;
      ++k;
    }
    l = k + b;
  } else if (tid >= ZT0) {
    l = (tid - ZT0) & (H - 1);
  }
  const int p = 2 * k, q = p + 1, u = 2 * l, v = u + 1;
  const int dp = jdest<NF>(p), dq = jdest<NF>(q), du = jdest<NF>(u), dv = jdest<NF>(v);
  const int zr = (tid - ZT0) >> 4;  // Z rows zr + 8i
  __syncthreads();
  int cur = 0, sweep = 0;
  for (; sweep < max_sweeps; ++sweep) {
    if (sweep < 12) JAC_STAMP(1 + sweep);
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < NF * NF; e += NT) {
      const int i = e / NF, j = e % NF;
      const double x = A[cur][i][j] * A[cur][i][j];
      if (i == j) dg += x; else off += x;
    }
    off = wave_sum_f64(off);
    dg = wave_sum_f64(dg);
    if ((tid & 63) == 0) {
      wsum[tid >> 6] = off;
      wsum[5 + (tid >> 6)] = dg;
    }
    __syncthreads();
    if (tid == 0) {
      const double o = ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3])) + wsum[4];
      const double d = ((wsum[5] + wsum[6]) + (wsum[7] + wsum[8])) + wsum[9];
      done = (o <= OCM_JACOBI_TOL2 * d) || (o == 0.0);
    }
    __syncthreads();
    if (done) break;
    for (int round = 0; round < NF - 1; ++round) {
      const int nx = cur ^ 1;
      if (tid < NB) {
        double ck, sk, cl, sl;
        jrot_fast(A[cur][p][p], A[cur][q][q], A[cur][p][q], ck, sk);
        jrot_fast(A[cur][u][u], A[cur][v][v], A[cur][u][v], cl, sl);
        const double a00 = A[cur][p][u], a01 = A[cur][p][v], a10 = A[cur][q][u], a11 = A[cur][q][v];
        const double b00 = ck * a00 - sk * a10, b01 = ck * a01 - sk * a11;
        const double b10 = sk * a00 + ck * a10, b11 = sk * a01 + ck * a11;
        const double o00 = cl * b00 - sl * b01, o01 = sl * b00 + cl * b01;
        const double o10 = cl * b10 - sl * b11, o11 = sl * b10 + cl * b11;
        A[nx][dp][du] = o00;
        A[nx][dp][dv] = o01;
        A[nx][dq][du] = o10;
        A[nx][dq][dv] = o11;
        if (k != l) {
          A[nx][du][dp] = o00;
          A[nx][dv][dp] = o01;
          A[nx][du][dq] = o10;
          A[nx][dv][dq] = o11;
        }
      } else if (tid >= ZT0) {
        double cl, sl;
        jrot_fast(A[cur][u][u], A[cur][v][v], A[cur][u][v], cl, sl);
#pragma unroll
        for (int i = 0; i < NF / 8; ++i) {
          const int r = zr + 8 * i;
          const double zp = Z[cur][r][u], zq = Z[cur][r][v];
          Z[nx][r][du] = cl * zp - sl * zq;
          Z[nx][r][dv] = sl * zp + cl * zq;
        }
      }
      __syncthreads();
      cur = nx;
    }
  }
  JAC_STAMP(13);
  int myrank = NF;
  for (int i = tid; i < NF; i += NT) {
    const double li = A[cur][i][i];
    int rank = 0;
    for (int j = 0; j < NF; ++j) {
      const double lj = A[cur][j][j];
      rank += (lj > li) || (lj == li && j < i);
    }
    evals[rank] = li;
    for (int r = 0; r < NF; ++r) Zout[r * NF + rank] = Z[cur][r][i];
    myrank = rank;
  }
  if (tid == 0 && sweeps_out) *sweeps_out = sweep;
  JAC_STAMP(14);
  if (!S) return;
  const int nx = cur ^ 1;  // free buffers: S into A[nx], S·Z into Z[nx]
  if (tid == 0) {
    unsigned n = 0;
    while ((int)(__hip_atomic_load(const_cast<unsigned*>(sflag), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - epoch) < 0 &&
           ++n < max_spins)
      __builtin_amdgcn_s_sleep(8);
    done = n < max_spins;
  }
  __syncthreads();
  for (int e = tid; e < NF * NF; e += NT) A[nx][e / NF][e % NF] = ld_agent(S + e);
  __syncthreads();
  for (int e = tid; e < NF * NF; e += NT) {
    const int r = e / NF, i = e % NF;
    double acc = 0.0;
#pragma unroll 8
    for (int j = 0; j < NF; ++j) acc = fma(A[nx][r][j], Z[cur][j][i], acc);
    Z[nx][r][i] = acc;
  }
  __syncthreads();
  if (tid < NF && myrank < ktest) {
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < NF; ++r) acc = fma(Z[cur][r][tid], Z[nx][r][tid], acc);
    res[myrank] = done ? sqrt(fmax(acc, 0.0)) : -1.0;
  }
  JAC_STAMP(15);
}

// ---------------------------------------------------------------------------
// One-workgroup Cholesky S = L Lᵀ (b ≤ 64).  A pivot below 1e-14·max diag is
// clamped (the CholQR2 second pass restores orthogonality).
// ---------------------------------------------------------------------------
// Right-looking Cholesky, one barrier per column: column j is read unscaled
// by every thread (its L column goes to a separate array), so the trailing
// update and the scaling need no barrier between them; threads form a 16×16
// grid over the trailing block (no integer division in the loop).
__global__ __launch_bounds__(256) void k_chol(const double* __restrict__ S, int b, double* __restrict__ L) {
  __shared__ double a[JMAX][JMAX + 1];
  __shared__ double lc[JMAX][JMAX + 1];
  const int tid = threadIdx.x, ti = tid >> 4, tl = tid & 15;
  for (int e = tid; e < b * b; e += 256) {
    a[e / b][e % b] = S[e];
    lc[e / b][e % b] = 0.0;
  }
  __syncthreads();
  double dmax = 0.0;
  for (int i = 0; i < b; ++i) dmax = fmax(dmax, a[i][i]);
  if (!(dmax > 0.0)) dmax = 1.0;
  for (int j = 0; j < b; ++j) {
    const double djj = sqrt(fmax(a[j][j], 1e-14 * dmax));
    const double inv = 1.0 / djj;
    for (int i = j + 1 + ti; i < b; i += 16) {
      const double aij = a[i][j] * inv;
      for (int l = j + 1 + tl; l <= i; l += 16) a[i][l] -= aij * (a[l][j] * inv);
    }
    if (tid < b - j) lc[j + tid][j] = tid == 0 ? djj : a[j + tid][j] * inv;
    __syncthreads();
  }
  for (int e = tid; e < b * b; e += 256) L[e] = lc[e / b][e % b];
}

// V = W · L⁻ᵀ row by row (forward substitution), b = compile-time block.
template <int BB>
__global__ __launch_bounds__(64) void k_trsm_rows(const double* __restrict__ W, const double* __restrict__ L, int p,
                                                   double* __restrict__ V) {
  __shared__ double sl[BB][BB + 1];
  __shared__ double rd[BB];  // reciprocal diagonal: no division on the dependency chain
  for (int e = threadIdx.x; e < BB * BB; e += blockDim.x) sl[e / BB][e % BB] = L[e];
  for (int j = threadIdx.x; j < BB; j += blockDim.x) rd[j] = 1.0 / L[j * BB + j];
  __syncthreads();
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= p) return;
  double v[BB];
#pragma unroll
  for (int j = 0; j < BB; ++j) {
    double s = W[(int64_t)r * BB + j];
#pragma unroll
    for (int l = 0; l < j; ++l) s -= v[l] * sl[j][l];
    v[j] = s * rd[j];
  }
#pragma unroll
  for (int j = 0; j < BB; ++j) V[(int64_t)r * BB + j] = v[j];
}

// b = 32: the fused path's block width (its CholQR kernels are below)
// lane l's double, wave-uniform l (two v_readlane_b32 into SGPRs: no LDS round trip)
__device__ __forceinline__ double readlane_f64(double v, int l) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, l);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), l);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double hash_normal(uint64_t a);

// ---------------------------------------------------------------------------
// CholQR of a tall p×32 fp64 block in two kinds of launch over CQ_G
// workgroups (four waves each, 16-row blocks split evenly), instead of
// k_colnormalize + k_atb_part + k_chol + k_trsm_rows per pass (what the
// 48- and 64-wide blocks still run):
//
//   k_cq_gram32   S = srcᵀsrc on fp64 MFMA (v_mfma_f64_16x16x4f64), wave
//                 partials summed in LDS, one 32×32 partial per workgroup; the
//                 LAST workgroup to finish (a ticket on a counter) sums the
//                 partials in workgroup order, scales the columns (r_i =
//                 1/√S_ii: the old k_colnormalize), factors S' = D S D = L Lᵀ in
//                 registers (lane i holds row i, v_readlane broadcasts, pivot
//                 clamp 1e-14 as k_chol), inverts L (lane c: row c of X = L⁻¹
//                 by back substitution) and writes M = D·Xᵀ (upper triangular),
//                 so that src·M has orthonormal columns.  With APPLY the
//                 launch first forms T = src·M_prev, stores it and takes the
//                 Gram of T straight from the MFMA result registers (the C
//                 layout is the row-contraction operand layout): the second
//                 CholQR pass costs no extra read of T;
//   k_cq_apply32  dst = src·M on fp64 MFMA.
//
// One pass: gram(W) → apply.  CholQR2: gram(W) → gram+apply(W → T) → apply(T).
// span(src·M) = span(src) whatever the pivots (M is invertible), so a single
// pass keeps the subspace exactly; only orthonormality depends on cond(src).
// Operand layouts (16×16 blocks, lane l: g = l>>4, c = l&15): the Gram reads
// src[16rb + g + 4j][16cb + c] (K-step j, both operands); the product reads
// A = src[16rb + c][4ks + g], B = M[4ks + g][16cb + c] and yields
// dst[16rb + g + 4r][16cb + c] in accumulator r.
// ---------------------------------------------------------------------------

__device__ __forceinline__ void cq_blocks(int p, int& lo, int& hi) {
  const int nrb = (p + 15) / 16;
  lo = (int)((int64_t)blockIdx.x * nrb / CQ_G);
  hi = (int)((int64_t)(blockIdx.x + 1) * nrb / CQ_G);
}

// this wave's 16-row block: dst = src · M (M rows from LDS), into o0 / o1
__device__ __forceinline__ void cq_apply_block(const double* src, int p, int rb, const double (*sm)[33], int g, int c,
                                               f64x4& o0, f64x4& o1) {
  const int ra = 16 * rb + c;
  double av[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) av[ks] = ra < p ? src[(int64_t)ra * 32 + 4 * ks + g] : 0.0;
  o0 = f64x4{0.0, 0.0, 0.0, 0.0};
  o1 = o0;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    o0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], sm[4 * ks + g][c], o0, 0, 0, 0);
    o1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], sm[4 * ks + g][16 + c], o1, 0, 0, 0);
  }
}

// The CholQR factor of a 32×32 Gram S (in sS): column scaling r_i = 1/√S_ii,
// S' = D S D = L Lᵀ by wave 0 in registers (lane i holds row i, v_readlane
// broadcasts, pivot clamp 1e-14 as k_chol), X = L⁻¹ by back substitution and
// M = D·Xᵀ (upper triangular), so that W·M has orthonormal columns.  A
// (numerically) zero column of W (rank-deficient C, fix_zero) is replaced by
// a pseudo-random one and S formed again from all of W by this workgroup.
// Called by every thread of ONE workgroup (any blockDim ≥ 64).
__device__ __forceinline__ void cq_finalize(double (*sS)[33], double* rsc, int* degen_flag, double* W, int p, int fix_zero,
                            uint64_t seed, double* __restrict__ Mout) {
  const int tid = threadIdx.x, lane = tid & 63, nt = blockDim.x;
  int& degen = *degen_flag;
  __shared__ double sm[32][33];
  if (tid == 0) degen = 0;
  __syncthreads();
  if (tid < 32) {
    const double nrm = sqrt(sS[tid][tid]);
    const bool zero = !(nrm > 1e-280);
    if (zero && fix_zero) atomicOr(&degen, 1);
    rsc[tid] = zero ? 0.0 : 1.0 / nrm;
  }
  __syncthreads();
  if (degen) {
    // rank-deficient C: a (numerically) zero column of W is replaced by the
    // pseudo-random column k_colnormalize uses, and S is formed again here
    // from all of W by this one workgroup (rare; the first pass only)
    for (int cc = 0; cc < 32; ++cc) {
      if (rsc[cc] != 0.0) continue;
      for (int r = tid; r < p; r += nt) W[(int64_t)r * 32 + cc] = hash_normal(seed * 0x9E3779B1ull + (uint64_t)r * 131 + cc);
    }
    __threadfence();
    __syncthreads();
    for (int e = tid; e < 32 * 32; e += nt) {
      const int i = e >> 5, j = e & 31;
      double v = 0.0;
      for (int r = 0; r < p; ++r) v += ld_agent(&W[(int64_t)r * 32 + i]) * ld_agent(&W[(int64_t)r * 32 + j]);
      sS[i][j] = v;
    }
    __syncthreads();
    if (tid < 32) rsc[tid] = 1.0 / sqrt(fmax(sS[tid][tid], 1e-300));
    __syncthreads();
  }
  if (tid < 64) {
    // Cholesky of S' = D S D in registers (lanes 32..63 mirror 0..31)
    const int i = lane & 31;
    const double ri = rsc[i];
    double a[32];
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) a[cc] = sS[i][cc] * ri * rsc[cc];
    double lrow[32], invd[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const double ajj = fmax(readlane_f64(a[j], j), 1e-14);  // diag(S') = 1: clamp 1e-14 · max diag
      const double inv = rsqrt(ajj);
      const double djj = ajj * inv;
      invd[j] = inv;
      const double lij = i > j ? a[j] * inv : (i == j ? djj : 0.0);
      lrow[j] = lij;
#pragma unroll
      for (int l = j + 1; l < 32; ++l) {
        const double llj = readlane_f64(lij, l);
        if (l <= i) a[l] -= lij * llj;
      }
    }
    if (lane < 32) {
#pragma unroll
      for (int cc = 0; cc < 32; ++cc) sm[i][cc] = lrow[cc];
    }
    __builtin_amdgcn_wave_barrier();
    // lane i: row i of X = L⁻¹ by X·L = I, columns j = 31 … 0, right-looking:
    // once X[i][j] is known its products with row j of L go into the pending
    // sums of columns < j (independent FMAs; the serial chain is one FMA and
    // one multiply per column)
    double xr[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) xr[j] = 0.0;
#pragma unroll
    for (int j = 31; j >= 0; --j) {
      xr[j] = j > i ? 0.0 : ((j == i ? 1.0 : 0.0) - xr[j]) * invd[j];
#pragma unroll
      for (int jj = 0; jj < j; ++jj) xr[jj] = fma(xr[j], sm[j][jj], xr[jj]);
    }
    // M[k][i] = r_k · X[i][k]
    if (lane < 32) {
#pragma unroll
      for (int k = 0; k < 32; ++k) Mout[k * 32 + i] = rsc[k] * xr[k];
    }
  }
}

// The CholQR factor of a non-degenerate Gram (sS) computed by ONE wave, into
// LDS: msm[k][i] = M[k][i], M = D·L⁻ᵀ as cq_finalize defines it (same pivot
// clamp), but without cross-lane register broadcasts: the rows of L go
// through LDS (Ls, rows 16-B aligned) and every lane reads row j of L with
// 16-B broadcast loads (left-looking Cholesky, lane i builds row i; then lane
// c solves L x = e_c for column c of L⁻¹).  k_cvq32<true>'s eighth wave runs
// it beside the other seven's product: cq_finalize's readlane form took
// ≈ 40 µs there (SGPR pressure next to the product waves) against 14 µs alone.
// Not bit-identical to cq_finalize (the sums run in another order).
__device__ __forceinline__ void cq_factor_wave(const double (*sS)[33], double (*Ls)[34], double* rsc, double* dinv,
                                               double (*msm)[33], int lane) {
  const int i = lane & 31;
  if (lane < 32) rsc[i] = 1.0 / sqrt(sS[i][i]);
  __builtin_amdgcn_wave_barrier();
  const double ri = rsc[i];
  double a[32], l[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) a[c] = sS[i][c] * ri * rsc[c];
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    double s0 = a[j], s1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < j; k += 2) {
      const double2 r2 = *reinterpret_cast<const double2*>(&Ls[j][k]);
      s0 = fma(-l[k], r2.x, s0);
      s1 = fma(-l[k + 1], r2.y, s1);
    }
    if (j & 1) s0 = fma(-l[j - 1], Ls[j][j - 1], s0);
    const double sj = s0 + s1;
    if (lane == j) {
      const double ajj = fmax(sj, 1e-14);
      const double inv = rsqrt(ajj);
      Ls[j][j] = ajj * inv;
      dinv[j] = inv;
    }
    __builtin_amdgcn_wave_barrier();
    const double inv = dinv[j];
    l[j] = i > j ? sj * inv : (i == j ? Ls[j][j] : 0.0);
    if (lane < 32 && i > j) Ls[i][j] = l[j];
    __builtin_amdgcn_wave_barrier();
  }
  // column c = i of X = L⁻¹: x_r = (δ_rc − Σ_{k<r} L[r][k] x_k) / L[r][r], r ≥ c
  double x[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    double s0 = r == i ? 1.0 : 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < r; k += 2) {
      const double2 r2 = *reinterpret_cast<const double2*>(&Ls[r][k]);
      s0 = fma(-r2.x, x[k], s0);
      s1 = fma(-r2.y, x[k + 1], s1);
    }
    if (r & 1) s0 = fma(-Ls[r][r - 1], x[r - 1], s0);
    x[r] = r < i ? 0.0 : (s0 + s1) * dinv[r];
  }
  // M[c][r] = r_c · X[r][c]
  if (lane < 32) {
#pragma unroll
    for (int r = 0; r < 32; ++r) msm[i][r] = rsc[i] * x[r];
  }
  __builtin_amdgcn_wave_barrier();
}

template <bool APPLY>
__global__ __launch_bounds__(256) void k_cq_gram32(double* W, int p, const double* __restrict__ Mprev, double* T,
                                                   double* __restrict__ part, unsigned* __restrict__ ticket,
                                                   int fix_zero, uint64_t seed, double* __restrict__ Mout) {
  __shared__ double wpart[4][3][4][64];
  __shared__ double sS[32][33];
  __shared__ double sm[32][33];
  __shared__ double rsc[32];
  __shared__ int last, degen;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  int lo, hi;
  cq_blocks(p, lo, hi);
  if (APPLY) {
    for (int e = tid; e < 32 * 32; e += 256) sm[e >> 5][e & 31] = Mprev[e];
    __syncthreads();
  }
  f64x4 s00 = {0.0, 0.0, 0.0, 0.0}, s01 = s00, s11 = s00;
  for (int rb = lo + wave; rb < hi; rb += 4) {
    double x[2][4];
    if (APPLY) {
      f64x4 o0, o1;
      cq_apply_block(W, p, rb, sm, g, c, o0, o1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rb + g + 4 * r;
        x[0][r] = row < p ? o0[r] : 0.0;
        x[1][r] = row < p ? o1[r] : 0.0;
        if (row < p) {
          T[(int64_t)row * 32 + c] = o0[r];
          T[(int64_t)row * 32 + 16 + c] = o1[r];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 16 * rb + g + 4 * j;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) x[cb][j] = r < p ? W[(int64_t)r * 32 + 16 * cb + c] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0][j], x[0][j], s00, 0, 0, 0);
      s01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0][j], x[1][j], s01, 0, 0, 0);
      s11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[1][j], x[1][j], s11, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    wpart[wave][0][r][lane] = s00[r];
    wpart[wave][1][r][lane] = s01[r];
    wpart[wave][2][r][lane] = s11[r];
  }
  __syncthreads();
  // hand-off without fences (ocm_internal.h: write-through stores, drained,
  // then the ticket; the last workgroup reads them back write-through, all
  // CQ_G of an element in flight together — a loop of loads waited out one
  // memory round trip per partial)
  for (int e = tid; e < 768; e += 256) {
    const double* w0 = &wpart[0][0][0][0];
    st_agent(&part[(int64_t)blockIdx.x * 768 + e], (w0[e] + w0[768 + e]) + (w0[1536 + e] + w0[2304 + e]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % CQ_G) == CQ_G - 1;
  __syncthreads();
  if (!last) return;
  for (int e = tid; e < 768; e += 256) {
    double pv[CQ_G];
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) pv[wg] = ld_agent(&part[(int64_t)wg * 768 + e]);
    double v = 0.0;
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) v += pv[wg];
    const int blk = e >> 8, r = (e >> 6) & 3, l = e & 63;
    const int row = 16 * (blk == 2) + (l >> 4) + 4 * r, col = 16 * (blk != 0) + (l & 15);
    sS[row][col] = v;
    if (blk == 1) sS[col][row] = v;
  }
  cq_finalize(sS, rsc, &degen, W, p, fix_zero, seed, Mout);
}

__global__ __launch_bounds__(256) void k_cq_apply32(const double* __restrict__ src, int p, const double* __restrict__ M,
                                                    double* __restrict__ dst) {
  __shared__ double sm[32][33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  for (int e = tid; e < 32 * 32; e += 256) sm[e >> 5][e & 31] = M[e];
  __syncthreads();
  int lo, hi;
  cq_blocks(p, lo, hi);
  for (int rb = lo + wave; rb < hi; rb += 4) {
    f64x4 o0, o1;
    cq_apply_block(src, p, rb, sm, g, c, o0, o1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rb + g + 4 * r;
      if (row < p) {
        dst[(int64_t)row * 32 + c] = o0[r];
        dst[(int64_t)row * 32 + 16 + c] = o1[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// One plain subspace iteration for b = 32 in ONE launch (the product, the
// basis change and the next CholQR factor):
//   Wout = (C · Win) · Min     (Min = the CholQR factor of Win: Win·Min is the
//                               orthonormal basis; nullptr = identity)
//   Mout = CholQR factor of Wout (cq_finalize)
// so V = Win·Min is never stored: span(C·V) = span(Wout), and only the
// Rayleigh–Ritz step materialises an orthonormal basis.  The product is
// k_cv32's (two half-K workgroups per 16 rows, parity ticket); the second of a
// pair to finish applies Min to its 16 rows in LDS, stores them and their
// 32×32 Gram partial (write-through); the last of each CVQ_G1 row blocks sums
// its group's partials in row-block order, the last group sums the group
// partials in order (two-level last arrival: deterministic, ≤ 16 + ⌈rb/16⌉
// counter adds in a row) and factors the Gram.  Replaces k_cv32 +
// k_cq_gram32 + k_cq_apply32 (three launches, ≈ 49 µs per iteration, r04zf).
// gpart: cv_rb·1024 row-block partials, then ⌈cv_rb/16⌉·1024 group partials;
// gtick: 1 + ⌈cv_rb/16⌉ counters TICKET_STRIDE words apart (zeroed once).
// ---------------------------------------------------------------------------
// Deferred factor (DEFER, round 5): Min is not given — the previous launch
// left the Gram of Win (Sin[0..1023], Sin[1024] = 0) instead of factoring it,
// and the eighth wave of every workgroup factors it (cq_factor_wave, the same
// values as cq_finalize would have produced) while the other seven form the
// product, so the ≈ 14 µs one-wave factorisation leaves the critical path.
// Sin[1024] = 1: the previous launch met a zero column and factored (and
// repaired W) itself; Min holds its factor.  defer_next: this launch leaves
// its Gram in Sout (non-degenerate) instead of factoring it.
template <bool DEFER>
__global__ __launch_bounds__(512) void k_cvq32(const double* __restrict__ C, int p, const double* __restrict__ Win,
                                             const double* __restrict__ Min, double* __restrict__ Wout,
                                             double* __restrict__ part, unsigned* __restrict__ ticket,
                                             double* __restrict__ gpart, unsigned* __restrict__ gtick,
                                             uint64_t seed, double* __restrict__ Mout, const double* __restrict__ Sin,
                                             double* __restrict__ Sout, int defer_next) {
  // DEFER: the factor wave (7) shares a SIMD with wave 3 (waves w and w + 4
  // share SIMD w), so the product runs on the six waves of the other SIMDs
  constexpr int PW = DEFER ? CV_W - 2 : CV_W;  // product waves
  __shared__ double red[CV_W][16 * 33];
  __shared__ __attribute__((aligned(16))) double lsc[DEFER ? 32 : 1][34];  // the factor wave's L
  __shared__ double dinv[DEFER ? 32 : 1];
  __shared__ double sm[32][33];
  __shared__ double sv[16][33];
  __shared__ double sS[32][33];
  __shared__ double rsc[32];
  __shared__ int last, degen;
  const int rb = blockIdx.x >> 1, half = blockIdx.x & 1;
  const int nrb = (p + 15) / 16;
  const int r0 = rb * 16;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = lane & 15, g = lane >> 4;
  const int pwave = DEFER ? (wave < 3 ? wave : wave - 1) : wave;  // product slot (DEFER: waves 0-2, 4-6)
  const bool prod = DEFER ? (wave != 3 && wave != 7) : true;
  const int kslice = (p + 2 * PW * 32 - 1) / (2 * PW * 32) * 32;
  const int kb = (half * PW + pwave) * kslice;
  const int ke = prod ? min(p, kb + kslice) : kb;  // waves 3 and 7 form no product
  const double* crow = C + (int64_t)min(r0 + i, p - 1) * p;
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
  for (int k0 = kb; k0 < ke; k0 += 32) {
    double a[8], b0[8], b1[8];
    const int kk0 = k0 + 8 * g;
    if (k0 + 32 <= ke) {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        a[s] = crow[kk0 + s];
        b0[s] = Win[(int64_t)(kk0 + s) * 32 + i];
        b1[s] = Win[(int64_t)(kk0 + s) * 32 + 16 + i];
      }
    } else {
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int kk = kk0 + s;
        const bool ok = kk < ke;
        a[s] = ok ? crow[kk] : 0.0;
        b0[s] = ok ? Win[(int64_t)kk * 32 + i] : 0.0;
        b1[s] = ok ? Win[(int64_t)kk * 32 + 16 + i] : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b0[s], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b1[s], acc1, 0, 0, 0);
    }
  }
  if (prod) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[pwave][(g + 4 * r) * 33 + i] = acc0[r];
      red[pwave][(g + 4 * r) * 33 + 16 + i] = acc1[r];
    }
  }
  if (DEFER) {
    if (wave == 7) {  // the factor of Win: from the previous launch's Gram (or its own factor)
      // all sixteen loads of a lane in flight at once: the product waves keep
      // the memory system busy, and one load at a time cost ≈ 2 µs apiece
      const bool ready = Sin[1024] != 0.0;
      const double* src = ready ? Min : Sin;
      double t[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) t[q] = src[lane + 64 * q];
      if (ready) {
#pragma unroll
        for (int q = 0; q < 16; ++q) sm[(lane + 64 * q) >> 5][(lane + 64 * q) & 31] = t[q];
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) sS[(lane + 64 * q) >> 5][(lane + 64 * q) & 31] = t[q];
        __builtin_amdgcn_wave_barrier();
        cq_factor_wave(sS, lsc, rsc, dinv, sm, lane);
      }
    }
  } else if (Min) {
    for (int e = tid; e < 32 * 32; e += 512) sm[e >> 5][e & 31] = Min[e];
  }
  __syncthreads();
  const int orow = tid >> 5, ocol = tid & 31;
  double v = 0.0;
#pragma unroll
  for (int w = 0; w < PW; ++w) v += red[w][orow * 33 + ocol];
  part[(int64_t)blockIdx.x * 512 + tid] = v;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = (__hip_atomic_fetch_add(&ticket[rb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) == 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!last) return;
  const double o = part[(int64_t)(blockIdx.x ^ 1) * 512 + tid];
  double y = half == 0 ? v + o : o + v;  // (C·Win)[r0 + orow][ocol]
  const bool rok = r0 + orow < p;
  if (DEFER || Min) {  // basis change on the output rows: (C·Win)·Min
    sv[orow][ocol] = y;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 32; ++j) t = fma(sv[orow][j], sm[j][ocol], t);
    y = t;
    __syncthreads();
  }
  // write-through: the finishing workgroup may re-read Wout (rank-deficient C)
  if (rok) st_agent(&Wout[(int64_t)(r0 + orow) * 32 + ocol], y);
  sv[orow][ocol] = rok ? y : 0.0;
  __syncthreads();
  // this row block's Gram partial (entries tid and tid + 512 of the 32×32)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = tid + 512 * h, a = e >> 5, b = e & 31;
    double gs = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) gs = fma(sv[r][a], sv[r][b], gs);
    st_agent(&gpart[(int64_t)rb * 1024 + e], gs);
  }
  const int ngrp = (nrb + CVQ_G1 - 1) / CVQ_G1;
  const int grp = rb / CVQ_G1, g0 = grp * CVQ_G1, gsize = min(CVQ_G1, nrb - g0);
  if (!last_arrival(gtick + (1 + grp) * TICKET_STRIDE, (unsigned)gsize)) return;
  double* gsum = gpart + (int64_t)nrb * 1024;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = tid + 512 * h;
    double pv[CVQ_G1];
#pragma unroll
    for (int q = 0; q < CVQ_G1; ++q) pv[q] = q < gsize ? ld_agent(&gpart[(int64_t)(g0 + q) * 1024 + e]) : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < CVQ_G1; ++q) acc += pv[q];
    st_agent(&gsum[(int64_t)grp * 1024 + e], acc);
  }
  if (!last_arrival(gtick, (unsigned)ngrp)) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = tid + 512 * h;
    double acc = 0.0;
    for (int q0 = 0; q0 < ngrp; q0 += 16) {
      double pv[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) pv[q] = q0 + q < ngrp ? ld_agent(&gsum[(int64_t)(q0 + q) * 1024 + e]) : 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) acc += pv[q];
    }
    sS[e >> 5][e & 31] = acc;
  }
  __syncthreads();
  if (defer_next) {  // hand the Gram on (the next launch factors it) unless a column is zero
    if (tid == 0) degen = 0;
    __syncthreads();
    if (tid < 32 && !(sqrt(sS[tid][tid]) > 1e-280)) atomicOr(&degen, 1);
    __syncthreads();
    if (!degen) {
      for (int e = tid; e < 32 * 32; e += 512) Sout[e] = sS[e >> 5][e & 31];
      if (tid == 0) Sout[1024] = 0.0 + (double)(tid & 1);
      return;
    }
    if (tid == 0) Sout[1024] = 1.0 + (double)(tid & 1);  // factored here (Mout), W repaired
  }
  cq_finalize(sS, rsc, &degen, Wout, p, 1, seed, Mout);
  __syncthreads();
}

__device__ __forceinline__ double hash_normal(uint64_t a) {
  // splitmix64 -> two uniforms -> Box-Muller
  auto mix = [](uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  const uint64_t h1 = mix(a), h2 = mix(a ^ 0xD1B54A32D192ED03ull);
  const double u1 = ((h1 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  const double u2 = ((h2 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// (+ zeroes nz words at z: the eigensolver's ticket counters, one launch
// instead of two memsets ahead of it)
// out = a·x + b·y over n values (the first step of a Chebyshev filter that
// starts from the Rayleigh–Ritz basis: Y1 = (2/β)·(C·V) − V from W = C·V)
__global__ void k_axpby(const double* __restrict__ x, const double* __restrict__ y, int64_t n, double a, double b,
                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fma(a, x[i], b * y[i]);
}

__global__ void k_randn(double* __restrict__ V, int64_t count, uint64_t seed, unsigned* __restrict__ z0 = nullptr,
                        int nz0 = 0, unsigned* __restrict__ z1 = nullptr, int nz1 = 0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) V[i] = hash_normal(seed * 0x100000001B3ull + (uint64_t)i);
  if (i < nz0) z0[i] = 0u;
  if (i < nz1) z1[i] = 0u;
}

// Normalise each column of a tall p×b matrix; an (almost) zero column is
// replaced by a pseudo-random one (rank-deficient C).
__global__ __launch_bounds__(256) void k_colnormalize(double* __restrict__ W, int p, int b, uint64_t seed) {
  __shared__ double red[4];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < p; r += 256) {
    const double v = W[(int64_t)r * b + c];
    s += v * v;
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  const double nrm = sqrt(red[0] + red[1] + red[2] + red[3]);
  __syncthreads();
  if (!(nrm > 1e-280)) {
    double s2 = 0.0;
    for (int r = threadIdx.x; r < p; r += 256) {
      const double v = hash_normal(seed * 0x9E3779B1ull + (uint64_t)r * 131 + c);
      W[(int64_t)r * b + c] = v;
      s2 += v * v;
    }
    s2 = wave_sum_f64(s2);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s2;
    __syncthreads();
    const double n2 = sqrt(red[0] + red[1] + red[2] + red[3]);
    for (int r = threadIdx.x; r < p; r += 256) W[(int64_t)r * b + c] /= n2;
    return;
  }
  const double inv = 1.0 / nrm;
  for (int r = threadIdx.x; r < p; r += 256) W[(int64_t)r * b + c] *= inv;
}

// ---------------------------------------------------------------------------
// Rayleigh–Ritz for b = 32 without rotating the block (round 5):
//   k_atb32        out = AᵀB (32×32) of tall p×32 blocks on fp64 MFMA, CQ_G
//                  workgroups, the last to finish sums the partials in order
//                  (H = VᵀW, and G2 = Rᵀ(C·R) for θ3);
//   k_rr_resid32   R = W − V·H (the projection residual, stored) and
//                  S = RᵀR (same hand-off; S stored write-through and a
//                  counter raised after it);
//   k_jacobi_1b    the Jacobi on H and, at its end, the Ritz residuals
//                  ‖C v_i − θ_i v_i‖ = ‖R z_i‖ = √(z_iᵀ S z_i) of the top-k
//                  pairs (S taken in flight once the counter is up) — no
//                  rotated block is formed for the convergence test;
//   k_theta_combine θ1..θ3 of the deflated matrix (I − P_k)C(I − P_k) from the
//                  b-block deflation Ct_b = (I − P_b)C(I − P_b) (traces,
//                  computed beside the Jacobi on side streams) plus the
//                  Ritz block's exact corrections, block form with
//                  E = (P_b − P_k)C(I − P_b):
//                    θ1 = Σ_t θ_i + tr Ct_b
//                    θ2 = Σ_t θ_i² + 2 Σ_t z_iᵀSz_i + ‖Ct_b‖²
//                    θ3 = Σ_t θ_i³ + 3 Σ_t θ_i z_iᵀSz_i + 3 Σ_t z_iᵀ G2 z_i + tr Ct_b³
//                  (t: Ritz pairs k..b−1; every term ≥ 0 for PSD C: no
//                  cancellation against the leading eigenvalues).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_atb32(const double* __restrict__ A, const double* __restrict__ B, int p,
                                               double* __restrict__ part, unsigned* __restrict__ ticket,
                                               double* __restrict__ out) {
  __shared__ double wpart[4][4][4][64];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  int lo, hi;
  cq_blocks(p, lo, hi);
  f64x4 s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int rb = lo + wave; rb < hi; rb += 4) {
    double a[2][4], bq[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 16 * rb + g + 4 * j;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        a[cb][j] = r < p ? A[(int64_t)r * 32 + 16 * cb + c] : 0.0;
        bq[cb][j] = r < p ? B[(int64_t)r * 32 + 16 * cb + c] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        s[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q >> 1][j], bq[q & 1][j], s[q], 0, 0, 0);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) wpart[wave][q][r][lane] = s[q][r];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const double* w0 = &wpart[0][0][0][0];
    st_agent(&part[(int64_t)blockIdx.x * 1024 + e], (w0[e] + w0[1024 + e]) + (w0[2048 + e] + w0[3072 + e]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % CQ_G) == CQ_G - 1;
  __syncthreads();
  if (!last) return;
  for (int e = tid; e < 1024; e += 256) {
    double pv[CQ_G];
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) pv[wg] = ld_agent(&part[(int64_t)wg * 1024 + e]);
    double v = 0.0;
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) v += pv[wg];
    const int q = e >> 8, r = (e >> 6) & 3, l = e & 63;
    out[(16 * (q >> 1) + (l >> 4) + 4 * r) * 32 + 16 * (q & 1) + (l & 15)] = v;
  }
}

// The Rayleigh–Ritz basis, W and H in one launch (round 5): with T = Wc·Mc
// (k_cq_gram32<true>, its CholQR factor M2 in M2) and CW = C·Wc (k_cv32 on a
// side stream, beside it), V = T·M2 and W = C·V = CW·(Mc·M2) need no second
// product with C; each workgroup forms Mc·M2 in LDS, applies both to its row
// blocks, stores V and W and its partial of H = VᵀW (k_atb32's MFMA layout and
// hand-off).  Replaces k_cq_apply32 + k_cv32 + k_atb32 on the critical path.
__global__ __launch_bounds__(256) void k_rr_basis32(const double* __restrict__ T, const double* __restrict__ CW,
                                                    int p, const double* __restrict__ Mc,
                                                    const double* __restrict__ M2, double* __restrict__ V,
                                                    double* __restrict__ W, double* __restrict__ part,
                                                    unsigned* __restrict__ ticket, double* __restrict__ H) {
  __shared__ double sm2[32][33];
  __shared__ double smc[32][33];
  __shared__ double smp[32][33];
  __shared__ double wpart[4][4][4][64];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  for (int e = tid; e < 32 * 32; e += 256) {
    sm2[e >> 5][e & 31] = M2[e];
    smc[e >> 5][e & 31] = Mc[e];
  }
  __syncthreads();
  for (int e = tid; e < 32 * 32; e += 256) {  // Mc·M2
    const int i = e >> 5, j = e & 31;
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) acc = fma(smc[i][k], sm2[k][j], acc);
    smp[i][j] = acc;
  }
  __syncthreads();
  int lo, hi;
  cq_blocks(p, lo, hi);
  f64x4 s[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int rb = lo + wave; rb < hi; rb += 4) {
    f64x4 v0, v1, w0, w1;
    cq_apply_block(T, p, rb, sm2, g, c, v0, v1);
    cq_apply_block(CW, p, rb, smp, g, c, w0, w1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rb + g + 4 * r;
      if (row < p) {
        V[(int64_t)row * 32 + c] = v0[r];
        V[(int64_t)row * 32 + 16 + c] = v1[r];
        W[(int64_t)row * 32 + c] = w0[r];
        W[(int64_t)row * 32 + 16 + c] = w1[r];
      }
    }
    // H partial: rows past p are zero in both (cq_apply_block reads them as 0)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(v0[r], w0[r], s[0], 0, 0, 0);
      s[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(v0[r], w1[r], s[1], 0, 0, 0);
      s[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[r], w0[r], s[2], 0, 0, 0);
      s[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(v1[r], w1[r], s[3], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 4; ++r) wpart[wave][q][r][lane] = s[q][r];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const double* w0p = &wpart[0][0][0][0];
    st_agent(&part[(int64_t)blockIdx.x * 1024 + e], (w0p[e] + w0p[1024 + e]) + (w0p[2048 + e] + w0p[3072 + e]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % CQ_G) == CQ_G - 1;
  __syncthreads();
  if (!last) return;
  for (int e = tid; e < 1024; e += 256) {
    double pv[CQ_G];
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) pv[wg] = ld_agent(&part[(int64_t)wg * 1024 + e]);
    double v = 0.0;
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) v += pv[wg];
    const int q = e >> 8, r = (e >> 6) & 3, l = e & 63;
    H[(16 * (q >> 1) + (l >> 4) + 4 * r) * 32 + 16 * (q & 1) + (l & 15)] = v;
  }
}

// sflag (optional): S is stored write-through and the counter raised to
// epoch (release) after it — k_jacobi_1b's test reads S in flight
__global__ __launch_bounds__(256) void k_rr_resid32(const double* __restrict__ V, const double* __restrict__ W, int p,
                                                    const double* __restrict__ H, double* __restrict__ R,
                                                    double* __restrict__ part, unsigned* __restrict__ ticket,
                                                    double* __restrict__ S, unsigned* __restrict__ sflag = nullptr,
                                                    unsigned epoch = 0) {
  __shared__ double wpart[4][3][4][64];
  __shared__ double sm[32][33];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  int lo, hi;
  cq_blocks(p, lo, hi);
  for (int e = tid; e < 32 * 32; e += 256) sm[e >> 5][e & 31] = H[e];
  __syncthreads();
  f64x4 s00 = {0.0, 0.0, 0.0, 0.0}, s01 = s00, s11 = s00;
  for (int rb = lo + wave; rb < hi; rb += 4) {
    f64x4 o0, o1;
    cq_apply_block(V, p, rb, sm, g, c, o0, o1);  // (V·H)[16rb + g + 4r][16cb + c]
    double x[2][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * rb + g + 4 * r;
      const bool ok = row < p;
      const double r0 = ok ? W[(int64_t)row * 32 + c] - o0[r] : 0.0;
      const double r1 = ok ? W[(int64_t)row * 32 + 16 + c] - o1[r] : 0.0;
      x[0][r] = r0;
      x[1][r] = r1;
      if (ok) {
        R[(int64_t)row * 32 + c] = r0;
        R[(int64_t)row * 32 + 16 + c] = r1;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0][j], x[0][j], s00, 0, 0, 0);
      s01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[0][j], x[1][j], s01, 0, 0, 0);
      s11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x[1][j], x[1][j], s11, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    wpart[wave][0][r][lane] = s00[r];
    wpart[wave][1][r][lane] = s01[r];
    wpart[wave][2][r][lane] = s11[r];
  }
  __syncthreads();
  for (int e = tid; e < 768; e += 256) {
    const double* w0 = &wpart[0][0][0][0];
    st_agent(&part[(int64_t)blockIdx.x * 768 + e], (w0[e] + w0[768 + e]) + (w0[1536 + e] + w0[2304 + e]));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0)
    last = (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % CQ_G) == CQ_G - 1;
  __syncthreads();
  if (!last) return;
  for (int e = tid; e < 768; e += 256) {
    double pv[CQ_G];
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) pv[wg] = ld_agent(&part[(int64_t)wg * 768 + e]);
    double v = 0.0;
#pragma unroll
    for (int wg = 0; wg < CQ_G; ++wg) v += pv[wg];
    const int blk = e >> 8, r = (e >> 6) & 3, l = e & 63;
    const int row = 16 * (blk == 2) + (l >> 4) + 4 * r, col = 16 * (blk != 0) + (l & 15);
    st_agent(&S[row * 32 + col], v);
    if (blk == 1) st_agent(&S[col * 32 + row], v);
  }
  if (!sflag) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) __hip_atomic_store(sflag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// q[i] = z_iᵀ M z_i for the 32 columns z_i of Z (32×32, column i = vector i):
// M and Z staged in LDS, Y = M·Z by the workgroup (four entries per thread),
// then the column dots Σ_r Z[r][i]·Y[r][i] — one workgroup of 256 threads.
__device__ __forceinline__ void quad_forms32(const double* __restrict__ M, double (*sz)[33], double (*sy)[33],
                                             double (*smm)[33], double* q) {
  const int tid = threadIdx.x;
  for (int e = tid; e < 1024; e += 256) smm[e >> 5][e & 31] = M[e];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256) {
    const int r = e >> 5, i = e & 31;
    double acc = 0.0;
#pragma unroll 8
    for (int j = 0; j < 32; ++j) acc = fma(smm[r][j], sz[j][i], acc);
    sy[r][i] = acc;
  }
  __syncthreads();
  if (tid < 32) {
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < 32; ++r) acc = fma(sz[r][tid], sy[r][tid], acc);
    q[tid] = acc;
  }
  __syncthreads();
}

// tr3[0..2] = tr Ct_b, ‖Ct_b‖², tr Ct_b³ (this slice's part); θ3 corrections
// only on slice 0 (the slices' θ3 partials are summed over ranks)
__global__ __launch_bounds__(256) void k_theta_combine(const double* __restrict__ th, const double* __restrict__ Z,
                                                       const double* __restrict__ S, const double* __restrict__ G2,
                                                       const double* __restrict__ tr3, int b, int k, int slice0,
                                                       int want3, double* __restrict__ theta_out) {
  __shared__ double sz[32][33], sy[32][33], smm[32][33];
  __shared__ double qs[32], qg[32];
  for (int e = threadIdx.x; e < 1024; e += 256) sz[e >> 5][e & 31] = Z[e];
  quad_forms32(S, sz, sy, smm, qs);
  if (want3) quad_forms32(G2, sz, sy, smm, qg);
  __syncthreads();
  if (threadIdx.x == 0) {
    double t1 = 0.0, t2 = 0.0, t3 = 0.0, e2 = 0.0, e3 = 0.0, g3 = 0.0;
    for (int i = k; i < b; ++i) {
      const double l = th[i];
      t1 += l;
      t2 += l * l;
      t3 += l * l * l;
      e2 += qs[i];
      e3 += l * qs[i];
      g3 += want3 ? qg[i] : 0.0;
    }
    theta_out[0] = t1 + tr3[0];
    theta_out[1] = (t2 + 2.0 * e2) + tr3[1];
    theta_out[2] = want3 ? (slice0 ? (t3 + 3.0 * e3 + 3.0 * g3) : 0.0) + tr3[2] : 0.0;
  }
}

// res[i] = ‖W_i − θ_i V_i‖ for i < kk
__global__ __launch_bounds__(256) void k_ritz_residual(const double* __restrict__ W, const double* __restrict__ V,
                                                       const double* __restrict__ theta, int p, int b,
                                                       double* __restrict__ res) {
  __shared__ double red[4];
  const int c = blockIdx.x;
  const double th = theta[c];
  double s = 0.0;
  for (int r = threadIdx.x; r < p; r += 256) {
    const double d = W[(int64_t)r * b + c] - th * V[(int64_t)r * b + c];
    s += d * d;
  }
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) res[c] = sqrt(red[0] + red[1] + red[2] + red[3]);
}

// evecs[i][j] = s_i · V[j][i] with s_i making the max-|entry| of row i positive
// (sklearn svd_flip(u_based_decision=False), first index on ties like argmax).
// inv_out (optional, with theta): workgroup 0 also writes k_inv_evals' 1/λ
// of the k values (the same cutoff and values; one launch less on the
// Rayleigh–Ritz tail)
__global__ __launch_bounds__(256) void k_extract_signfix(const double* __restrict__ V, int p, int b, int k,
                                                         double* __restrict__ evecs,
                                                         const double* __restrict__ theta = nullptr,
                                                         double* __restrict__ evals = nullptr, double rcond = 0.0,
                                                         double* __restrict__ inv_out = nullptr) {
  if (evals && threadIdx.x == 0) evals[blockIdx.x] = theta[blockIdx.x];  // λ_i (no separate copy)
  __shared__ double bv[256];
  __shared__ int bi[256];
  if (inv_out && blockIdx.x == 0) {
    double mx = 0.0;
    for (int i = threadIdx.x; i < k; i += 256) mx = fmax(mx, fabs(theta[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if ((threadIdx.x & 63) == 0) bv[threadIdx.x >> 6] = mx;
    __syncthreads();
    const double cut = rcond * fmax(fmax(bv[0], bv[1]), fmax(bv[2], bv[3]));
    for (int i = threadIdx.x; i < k; i += 256) {
      const double l = theta[i];
      inv_out[i] = fabs(l) > cut ? 1.0 / l : 0.0;
    }
    __syncthreads();  // bv is reused below
  }
  const int i = blockIdx.x;
  double best = -1.0;
  int bidx = 0x7fffffff;
  for (int j = threadIdx.x; j < p; j += 256) {
    const double a = fabs(V[(int64_t)j * b + i]);
    if (a > best || (a == best && j < bidx)) {
      best = a;
      bidx = j;
    }
  }
  bv[threadIdx.x] = best;
  bi[threadIdx.x] = bidx;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const double a = bv[threadIdx.x + o];
      const int ai = bi[threadIdx.x + o];
      if (a > bv[threadIdx.x] || (a == bv[threadIdx.x] && ai < bi[threadIdx.x])) {
        bv[threadIdx.x] = a;
        bi[threadIdx.x] = ai;
      }
    }
    __syncthreads();
  }
  const double sg = V[(int64_t)bi[0] * b + i] < 0.0 ? -1.0 : 1.0;
  for (int j = threadIdx.x; j < p; j += 256) evecs[(int64_t)i * p + j] = sg * V[(int64_t)j * b + i];
}

// Operands of the deflation update C⊥ = C − U·Wt (one fp64-MFMA GEMM):
//   C⊥ = C − V_k M_kᵀ − M_k V_kᵀ + N_k V_kᵀ = C − [V_k | M_k − N_k]·[M_k | V_k]ᵀ
// with V the Ritz basis, M = C V, N = V_k H_k (H = VᵀM; first k columns of p×b
// blocks).  U p×2k row-major, Wt 2k×p row-major.  Thread (i, l) forms its N
// entry itself (H_k in LDS for k ≤ 64): one launch, no separate GEMM for N.
__global__ __launch_bounds__(256) void k_deflate_operands_h(const double* __restrict__ V, const double* __restrict__ M,
                                                            const double* __restrict__ H, int p, int b, int k,
                                                            double* __restrict__ U, double* __restrict__ Wt) {
  __shared__ double Hs[64 * 64];
  const bool lds = k <= 64;
  if (lds)
    for (int e = threadIdx.x; e < k * k; e += 256) Hs[e] = H[(e / k) * b + e % k];
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)p * k) return;
  const int i = (int)(e / k), l = (int)(e % k);
  const double* vr = V + (int64_t)i * b;
  double nn = 0.0;
  for (int t = 0; t < k; ++t) nn = fma(vr[t], lds ? Hs[t * k + l] : H[(int64_t)t * b + l], nn);
  const double v = vr[l], m = M[(int64_t)i * b + l];
  U[(int64_t)i * 2 * k + l] = v;
  U[(int64_t)i * 2 * k + k + l] = m - nn;
  Wt[(int64_t)l * p + i] = m;
  Wt[(int64_t)(k + l) * p + i] = v;
}

// θ's sums in one launch (fixed order): out3[0..1] = the deflation GEMM's
// {tr, ‖·‖²} tile pairs (which & 1), out3[2] = Σ of the Δ-term partials + Σ
// of the trace partials (which & 2; either count may be 0)
__global__ __launch_bounds__(256) void k_theta_final(const double* __restrict__ pairs, int npairs,
                                                     const double* __restrict__ d3, int nd3,
                                                     const double* __restrict__ tr, int ntr,
                                                     double* __restrict__ out3, int which) {
  __shared__ double red[3][4];
  double a = 0.0, b = 0.0, c = 0.0, t = 0.0;
  for (int i = threadIdx.x; i < npairs; i += 256) {
    a += pairs[2 * i];
    b += pairs[2 * i + 1];
  }
  for (int i = threadIdx.x; i < nd3; i += 256) c += d3[i];
  for (int i = threadIdx.x; i < ntr; i += 256) t += tr[i];
  c += t;
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  c = wave_sum_f64(c);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
    red[2][threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x < 3 && (which & (threadIdx.x < 2 ? 1 : 2)))
    out3[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// p ≤ 64 path: evecs (k×p) from Z (p×p columns), θ from the tail eigenvalues
__global__ void k_small_finish(const double* __restrict__ ev, const double* __restrict__ Z, int p, int k,
                               double* __restrict__ evals, double* __restrict__ evecs, double* __restrict__ theta) {
  const int i = threadIdx.x;
  if (i < k) {
    evals[i] = ev[i];
    // sign: max |entry| positive (first index on ties)
    double best = -1.0;
    int bj = 0;
    for (int j = 0; j < p; ++j) {
      const double a = fabs(Z[j * p + i]);
      if (a > best) {
        best = a;
        bj = j;
      }
    }
    const double sg = Z[bj * p + i] < 0.0 ? -1.0 : 1.0;
    for (int j = 0; j < p; ++j) evecs[i * p + j] = sg * Z[j * p + i];
  }
  if (i == 0 && theta) {
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int j = k; j < p; ++j) {
      const double l = ev[j];
      t1 += l;
      t2 += l * l;
      t3 += l * l * l;
    }
    theta[0] = t1;
    theta[1] = t2;
    theta[2] = t3;
  }
}

__global__ void k_pinv_from_eig(const double* __restrict__ ev, const double* __restrict__ Z, int d, double rcond,
                                double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= d * d) return;
  const int i = e / d, j = e % d;
  double lmax = 0.0;
  for (int l = 0; l < d; ++l) lmax = fmax(lmax, fabs(ev[l]));
  const double cut = rcond * lmax;
  double v = 0.0;
  for (int l = 0; l < d; ++l)
    if (fabs(ev[l]) > cut) v += Z[i * d + l] * Z[j * d + l] / ev[l];
  out[e] = v;
}

// ---------------------------------------------------------------------------
// host-side drivers
// ---------------------------------------------------------------------------

int dgemm(const double* A, int64_t lda, const double* B, int64_t ldb, double* D, int64_t ldd, int M, int N, int K,
          int ksplit, double* planes, hipStream_t st) {
  if (ksplit <= 1) {
    dim3 g((M + DT - 1) / DT, (N + DT - 1) / DT, 1);
    hipLaunchKernelGGL(k_dgemm<0>, g, dim3(256), 0, st, A, lda, B, ldb, D, ldd, M, N, K, K, nullptr, 0, nullptr);
    OCM_CHECK_LAUNCH("k_dgemm");
    return OCM_OK;
  }
  int kper = (K + ksplit - 1) / ksplit;
  kper = (kper + DBK - 1) / DBK * DBK;
  const int nz = (K + kper - 1) / kper;
  dim3 g((M + DT - 1) / DT, (N + DT - 1) / DT, nz);
  hipLaunchKernelGGL(k_dgemm<0>, g, dim3(256), 0, st, A, lda, B, ldb, planes, (int64_t)N, M, N, K, kper, nullptr, 0,
                     nullptr);
  OCM_CHECK_LAUNCH("k_dgemm split");
  const int64_t plane = (int64_t)M * N;
  hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, planes, nz, plane, D);
  OCM_CHECK_LAUNCH("k_sum_planes");
  (void)ldd;  // planes path writes D densely with ldd == N
  return OCM_OK;
}

#ifdef OCM_JACOBI_STAMPS  // make exp diagnostic (scripts/jacobi_micro.py, profiles/r06w_jacobi_round_probes.txt)
// the phase times of the k_jacobi_1b launch last queued on st, printed once it is done; clears the stamps
void jacobi_print_stamps(hipStream_t st, bool tested) {
  static unsigned long long h[16][64];
  (void)hipStreamSynchronize(st);
  (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_jac_st), sizeof(h));
  fprintf(stderr, "jacobi32 us: load %.2f", (h[1][0] - h[0][0]) / 100.0);
  for (int i = 1; i < 13 && h[i + 1][0] > h[i][0] && h[i][0] >= h[1][0]; ++i)
    fprintf(stderr, " sweep%d %.2f", i - 1, (h[i + 1][0] - h[i][0]) / 100.0);
  fprintf(stderr, " | rounds %.2f sort+write %.2f", (h[13][0] - h[1][0]) / 100.0, (h[14][0] - h[13][0]) / 100.0);
  if (tested) fprintf(stderr, " test %.2f", (h[15][0] - h[14][0]) / 100.0);
  fprintf(stderr, "\n");
  static unsigned long long z[16][64];
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_jac_st), z, sizeof(z));
}
#else
inline void jacobi_print_stamps(hipStream_t, bool) {}
#endif

int jacobi(const double* A, int n, int max_sweeps, double* ev, double* Z, hipStream_t st, const double* S = nullptr,
           const unsigned* sflag = nullptr, unsigned epoch = 0, int k = 0, double* res = nullptr,
           unsigned spins = OCM_JACOBI_WAIT_SPINS) {
  // n = 32: the one-barrier block kernel k_jacobi_1b (107 µs alone against 139 for the two-barrier
  // k_jacobi_blk, r05s3_jacobi_ab.txt; the block rounds in one wave without barriers measured 204 µs,
  // r05s_eig_timeline.txt); S: the Rayleigh–Ritz test at its end (S from k_rr_resid32 in flight)
  if (n == 32)
    hipLaunchKernelGGL(k_jacobi_1b<32>, dim3(1), dim3(320), 0, st, A, max_sweeps, ev, Z, nullptr, S, sflag, epoch, k,
                       res, spins);
  else if (n == 48)
    hipLaunchKernelGGL(k_jacobi_blk<48>, dim3(1), dim3(256), 0, st, A, max_sweeps, ev, Z, nullptr);
  else if (n == 64)
    hipLaunchKernelGGL(k_jacobi_blk<64>, dim3(1), dim3(256), 0, st, A, max_sweeps, ev, Z, nullptr);
  else if (n <= 32)
    hipLaunchKernelGGL((k_jacobi<0, 64>), dim3(1), dim3(64), 0, st, A, n, max_sweeps, ev, Z, nullptr);
  else
    hipLaunchKernelGGL((k_jacobi<0, 256>), dim3(1), dim3(256), 0, st, A, n, max_sweeps, ev, Z, nullptr);
  OCM_CHECK_LAUNCH("k_jacobi");
  if (n == 32) jacobi_print_stamps(st, S != nullptr);
  return OCM_OK;
}

int atb(const double* A, const double* B, int p, int b, double* out, double* part, hipStream_t st) {
  const int nblk = (p + 63) / 64;
  hipLaunchKernelGGL(k_atb_part, dim3(nblk), dim3(256), 0, st, A, B, p, b, part);
  OCM_CHECK_LAUNCH("k_atb_part");
  const int64_t plane = (int64_t)b * b;
  hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, part, nblk, plane, out);
  OCM_CHECK_LAUNCH("k_sum_planes");
  return OCM_OK;
}

int trsm_rows(const double* W, const double* L, int p, int b, double* V, hipStream_t st) {
  // 64-thread workgroups: the p rows spread over p/64 CUs (the per-row chain is serial)
  dim3 g((p + 63) / 64);
  switch (b) {
    case 48: hipLaunchKernelGGL(k_trsm_rows<48>, g, dim3(64), 0, st, W, L, p, V); break;
    case 64: hipLaunchKernelGGL(k_trsm_rows<64>, g, dim3(64), 0, st, W, L, p, V); break;
    default: return ocm::fail(OCM_ERR_UNSUPPORTED, "trsm block must be 48 or 64");
  }
  OCM_CHECK_LAUNCH("k_trsm_rows");
  return OCM_OK;
}

// ---- wide blocks (b > 64: n_components beyond one 64-wide block) ----------
// The b×b steps of the iteration run on the host in fp64 (b ≤ p; the p×b
// products stay on the GPU): Cholesky of the CholQR Gram, and the projected
// eigenproblem of Rayleigh–Ritz by Householder tridiagonalisation + implicit
// QL with Wilkinson shifts.

// S = Aᵀ B (b×b) for tall p×b row-major A, B on the fp64-MFMA GEMM (split-K planes)
int dgemm_ta(const double* A, const double* B, int p, int b, double* S, double* planes, size_t plane_cap,
             hipStream_t st) {
  const int tiles = ((b + DT - 1) / DT) * ((b + DT - 1) / DT);
  int ksplit = std::max(1, std::min(16, 256 / tiles));
  while (ksplit > 1 && (size_t)ksplit * b * b > plane_cap) --ksplit;
  int kper = (p + ksplit - 1) / ksplit;
  kper = (kper + DBK - 1) / DBK * DBK;
  const int nz = (p + kper - 1) / kper;
  dim3 g((b + DT - 1) / DT, (b + DT - 1) / DT, nz);
  hipLaunchKernelGGL((k_dgemm<0, true>), g, dim3(256), 0, st, A, (int64_t)b, B, (int64_t)b, planes, (int64_t)b, b, b, p,
                     kper, nullptr, 0, nullptr, 0);
  OCM_CHECK_LAUNCH("k_dgemm TA");
  const int64_t plane = (int64_t)b * b;
  hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, planes, nz, plane, S);
  OCM_CHECK_LAUNCH("k_sum_planes");
  return OCM_OK;
}

// θ3 = trace(D³) of the deflated covariance D = Δ + O (Δ its diagonal, O the
// off-diagonal part), expanded so that only O goes through a Gram:
//   trace(D³) = Σ_i Δ_i³ + 3 Σ_i Δ_i Σ_j O_ij² + Σ_ij O_ij (O²)_ij
// (the terms with one O vanish: O_ii = 0).  The first two are exact fp64 sums
// over rows [r0, r1) (this slice's rows) of k_dgemm<3>'s diagonal and row
// sums; O² is the i8×3 Gram of O's rows [r0, r1) (a Gram over a row subset is
// a partial of O², and the trace is linear in it), and the last term pairs it
// with all of O.  O has no dominant diagonal, so the Gram's outlier guard
// stays quiet.
// rows [r0, r1) of the Δ terms of θ3 from k_dgemm<3>'s outputs: per
// workgroup Σ_i (Δ_i³ + 3 Δ_i Σ_t rowpart[t][i]) over its 256 rows
__global__ __launch_bounds__(256) void k_theta3_rows(const double* __restrict__ diag,
                                                     const double* __restrict__ rowpart, int ntc, int p, int r0,
                                                     int r1, double* __restrict__ part) {
  __shared__ double red[4];
  const int i = r0 + blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (i < r1) {
    double s2 = 0.0;
    for (int t = 0; t < ntc; ++t) s2 += rowpart[(int64_t)t * p + i];
    const double di = diag[i];
    acc = di * di * di + 3.0 * di * s2;
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// 1/λ with np.linalg.pinv's cutoff (|λ| ≤ rcond·max|λ| → 0); one workgroup,
// every thread reads all k values (k is the component count: ≤ p, small)
__global__ __launch_bounds__(256) void k_inv_evals(const double* __restrict__ ev, int k, double rcond,
                                                   double* __restrict__ out) {
  __shared__ double red[4];
  double mx = 0.0;
  for (int i = threadIdx.x; i < k; i += 256) mx = fmax(mx, fabs(ev[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  const double cut = rcond * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();  // out may alias ev: every read of ev is done
  for (int i = threadIdx.x; i < k; i += 256) {
    const double l = ev[i];
    out[i] = fabs(l) > cut ? 1.0 / l : 0.0;
  }
}

// the eigensolver's side stream, its events and the θ3 Gram's sub-context
int eig_side_init(ocm_ctx* ctx) {
  if (ctx->eig_sub) return OCM_OK;
  for (auto& s : ctx->eig_side) OCM_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  for (auto& e : ctx->eig_ev) OCM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  OCM_HIP(hipMalloc(reinterpret_cast<void**>(&ctx->eig_flag), sizeof(unsigned)));
  OCM_HIP(hipMemset(ctx->eig_flag, 0, sizeof(unsigned)));
  ctx->eig_epoch = 0;
  auto* sub = new ocm_ctx();
  sub->device = ctx->device;
  sub->num_cus = ctx->num_cus;
  ctx->eig_sub = sub;
  return OCM_OK;
}

// ---- ocm_eig_topk -----------------------------------------------------------
// eig_topk_impl plans (ocm_eig_plan.h: the path, the block width b, the
// workspace layout) and hands over to one driver per path: eig_small,
// eig_fused32 (b = 32), eig_block (b = 48 / 64 on the device, wider blocks
// with their b×b steps on the host).
//
// Iterations are plain orthogonal iterations V ← orth(C V) except at the
// Rayleigh–Ritz steps, which are the only ones that can test convergence:
// the subspace after iteration i is span(Cⁱ V₀) whatever rotations happen in
// between, so Rayleigh–Ritz only has to run where the test can pass
// (ocm_eig::Schedule predicts where).  The first test comes at iteration
// PLAIN + 1: the spectra of the bench data (p = 2048, k = 20) converge at
// iteration 5, the derivative spectra of the nuts preprocessing
// (simca_nuts.py:47-52) at ~33.
using ocm_eig::PLAIN;

// what the drivers share: the call's arguments, the plan and the carved workspace
struct EigState {
  ocm_ctx* ctx;
  hipStream_t st;
  const double* C;
  int p, k;
  double tol;
  int max_iter, theta_mode, slice, nslices;
  double *evals_out, *evecs_out, *theta_out, *inv_out;
  double rcond;
  ocm_eig::Plan pl;
  ocm_eig::Layout w;
  double* hres;  // pinned: θ (b) then the residuals (b) of a test; wide: + b×b staging, a b×b result, b values
  double* hmat() const { return hres + 2 * pl.b; }
};

int eig_small(const EigState& s) {
  double *ev = s.w.theta, *Z = s.w.Z;
  int rc = jacobi(s.C, s.p, 60, ev, Z, s.st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_small_finish, dim3(1), dim3(64), 0, s.st, ev, Z, s.p, s.k, s.evals_out, s.evecs_out,
                     s.theta_mode ? s.theta_out : nullptr);
  OCM_CHECK_LAUNCH("k_small_finish");
  if (s.inv_out) hipLaunchKernelGGL(k_inv_evals, dim3(1), dim3(256), 0, s.st, s.evals_out, s.k, s.rcond, s.inv_out);
  if (s.theta_mode && s.slice != 0) OCM_HIP(hipMemsetAsync(s.theta_out + 2, 0, sizeof(double), s.st));
  return OCM_OK;
}

// θ1..θ3 of (I − P)C(I − P), P the projector on the first kd columns of the
// orthonormal block Vb (Wb_ = C·Vb, Hb = Vbᵀ Wb_): the rank-2kd deflation
// GEMM with its trace and Frobenius epilogue → out3[0..1], and this slice's
// θ3 rows → out3[2], all on stream sa; the θ3 Gram runs on gctx's workspaces.
// s2 (≠ sa: the fused path's second side stream) takes the Δ terms beside the
// θ3 Gram; eig_ev[4] / [5] order them.
int theta_deflated(const EigState& s, const double* Vb, const double* Wb_, const double* Hb, int kd, hipStream_t sa,
                   hipStream_t s2, ocm_ctx* gctx, double* out3) {
  const int p = s.p, b = s.pl.b;
  double *Ud = s.w.Ud, *Wd = s.w.Wd, *dpart = s.w.dpart;
  hipLaunchKernelGGL(k_deflate_operands_h, dim3((unsigned)(((size_t)p * kd + 255) / 256)), dim3(256), 0, sa, Vb, Wb_,
                     Hb, p, b, kd, Ud, Wd);
  OCM_CHECK_LAUNCH("k_deflate_operands_h");
  // the deflated matrix D = C − U·Wdᵀ is never stored in fp64: k_dgemm<3>
  // writes its off-diagonal part O (float32, the θ3 Gram's input), its
  // diagonal Δ, per-tile row sums of O² and the {tr D, ‖D‖²} partials.  O
  // and the partials live in gctx's second arena (the Gram takes gctx's
  // workspace).
  const size_t pp = (size_t)p * p;
  const int ntc = (p + DT - 1) / DT;
  const int ntq = (p + 127) / 128;
  const int ntr_cap = ntq * (ntq + 1) / 2 * 16;  // k_gram_trace partials
  const size_t o32_bytes = (pp * sizeof(float) + 255) / 256 * 256;
  char* aux = static_cast<char*>(ocm::workspace_aux(
      gctx, o32_bytes + (2 * (size_t)p + (size_t)ntc * p + ntr_cap + 64) * sizeof(double), sa));
  if (!aux) return OCM_ERR_NOMEM;
  float* O32 = reinterpret_cast<float*>(aux);
  double* diag = reinterpret_cast<double*>(aux + o32_bytes);
  double* rowpart = diag + p;
  double* dpart3 = rowpart + (size_t)ntc * p;  // ≤ p/256 + 1 workgroup partials
  double* trpart = dpart3 + p;
  const dim3 gd(ntc, ntc, 1);
  if (2 * kd <= 64)
    hipLaunchKernelGGL(k_deflate64, gd, dim3(256), 0, sa, Ud, (int64_t)(2 * kd), Wd, (int64_t)p, diag, p, p, 2 * kd,
                       s.C, (int64_t)p, dpart, O32, rowpart);
  else
    hipLaunchKernelGGL(k_dgemm<3>, gd, dim3(256), 0, sa, Ud, (int64_t)(2 * kd), Wd, (int64_t)p, diag, (int64_t)p, p, p,
                       2 * kd, 2 * kd, s.C, (int64_t)p, dpart, 0, O32, rowpart);
  OCM_CHECK_LAUNCH("k_dgemm deflate");
  // the tile pairs sit in this context's workspace, which the θ3 Gram takes
  // over when gctx is this context (the unfused paths): sum them first there
  const bool own_ws = gctx == s.ctx;
  if (own_ws) {
    hipLaunchKernelGGL(k_theta_final, dim3(1), dim3(256), 0, sa, dpart, (int)(gd.x * gd.y), nullptr, 0, nullptr, 0,
                       out3, 1);
    OCM_CHECK_LAUNCH("k_theta_final pairs");
  }
  // θ3 = Σ Δ³ + 3 Σ Δ_i Σ_j O_ij² + Σ O∘(O²): this slice's rows of the Δ
  // terms (on s2), and the i8×3 Gram of its rows of O paired with all of O
  // in the Gram's epilogue (k_gram_trace, on sa)
  const int r0 = (int)((int64_t)p * s.slice / s.nslices), r1 = (int)((int64_t)p * (s.slice + 1) / s.nslices);
  int nb3 = 0, ntr = 0;
  if (s.theta_mode >= 2 && r1 > r0) {
    const int nr = r1 - r0;
    nb3 = (nr + 255) / 256;
    if (s2 != sa) {
      OCM_HIP(hipEventRecord(s.ctx->eig_ev[4], sa));
      OCM_HIP(hipStreamWaitEvent(s2, s.ctx->eig_ev[4], 0));
    }
    hipLaunchKernelGGL(k_theta3_rows, dim3(nb3), dim3(256), 0, s2, diag, rowpart, ntc, p, r0, r1, dpart3);
    OCM_CHECK_LAUNCH("k_theta3_rows");
    if (s2 != sa) OCM_HIP(hipEventRecord(s.ctx->eig_ev[5], s2));
    int rc2 = ocm::trace_gram_rows_i8(gctx, O32 + (size_t)r0 * p, p, nr, p, O32, trpart, &ntr, sa);
    if (rc2) return rc2;
    if (s2 != sa) OCM_HIP(hipStreamWaitEvent(sa, s.ctx->eig_ev[5], 0));
  }
  hipLaunchKernelGGL(k_theta_final, dim3(1), dim3(256), 0, sa, dpart, own_ws ? 0 : (int)(gd.x * gd.y), dpart3, nb3,
                     trpart, ntr, out3, own_ws ? 2 : 3);
  OCM_CHECK_LAUNCH("k_theta_final");
  return OCM_OK;
}

// V₀: a Gaussian block, used as it is — the subspace after i iterations is
// span(Cⁱ V₀) whatever basis V₀ has, so only the Rayleigh–Ritz steps need an
// orthonormal basis (every iteration before one ends with CholQR2), and an
// orthonormalisation of V₀ costs a CholQR pass (≈ 36 µs) for nothing.  The
// launch also zeroes the tickets (ocm_eig::carve).  rr_first (max_iter = 1,
// Rayleigh–Ritz on the first product): a second block into T1, which the
// caller orthonormalises into V.
int eig_start_block(const EigState& s, bool rr_first) {
  const size_t pb = s.pl.pb;
  hipLaunchKernelGGL(k_randn, dim3((unsigned)((std::max<size_t>(pb, s.pl.nzero_cv) + 255) / 256)), dim3(256), 0, s.st,
                     s.w.V, (int64_t)pb, 0x5EEDull, s.w.cq_ticket, 1, s.w.cv_ticket, s.pl.nzero_cv);
  OCM_CHECK_LAUNCH("k_randn");
  if (rr_first) {
    hipLaunchKernelGGL(k_randn, dim3((unsigned)((pb + 255) / 256)), dim3(256), 0, s.st, s.w.T1, (int64_t)pb, 0x5EEDull);
    OCM_CHECK_LAUNCH("k_randn");
  }
  return OCM_OK;
}

// ---- b = 32: the fused path -------------------------------------------------
// The chain of plain iterations: the current unnormalised block Wc and its
// CholQR factor Mc (nullptr: Wc is orthonormal or the start block, used as it
// is), the block the next launch writes, the factor slot it uses, and the
// Gram the previous plain launch left unfactored (k_cvq32<true>).
//
// Chebyshev-filtered iterations, from the first failed
// Rayleigh–Ritz test on: the test's Ritz values bound the unwanted spectrum
// (λ_{b+1} … λ_p ≤ θ_b up to the test's accuracy; C is PSD, so ≥ 0), and a
// degree-d Chebyshev polynomial T_d(X), X = 2C/θ_b − I, damps [0, θ_b] to
// ≤ 1 while it amplifies λ_k by T_d(2λ_k/θ_b − 1) ≈ e^{d·acosh(2λ_k/θ_b − 1)}
// — for a slow gap (λ_k/θ_b = 1 + δ) a rate of e^{−2√δ} per product against
// (1 + δ)^{−1} for the plain iteration.  Each product is one three-term step
// Y_{j+1} = (4/θ_b)·C·Y_j − 2Y_j − Y_{j−1} (k_cv32x) with no CholQR in
// between; a segment ends with one CholQR factor once the block's condition
// would pass ≈ 1e6 (T_d(x_1) ≤ 1e6, x_1 = 2θ_1/θ_b − 1), and the next segment
// restarts the recurrence from the orthonormalised block.  Before the first
// test nothing bounds λ_{b+1} (the bench data converge at that test), so the
// plain iterations stay.
struct Chain32 {
  double* Wc;
  double* Wn;
  const double* Mc = nullptr;
  int mslot = 0;
  const double* Sprev = nullptr;
  int sslot = 0;
  bool cheb = false;       // filtered continuation active
  bool y1_from_w = false;  // the segment starts at the Rayleigh–Ritz basis V with C·V = W in hand
  double cheb_beta = 0.0;  // θ_b of the test that switched it on
  int cheb_dmax = 1;
};

// one filter segment from iteration it on: Y0 (orthonormal) → Y_d, then its
// CholQR factor; *np_out: the products it ran (iterations it … it + np − 1)
int cheb_segment(const EigState& s, Chain32& ch, int it, int next_rr, int* np_out) {
  const ocm_eig::Layout& w = s.w;
  const int p = s.p, cv_rb = s.pl.cv_rb;
  const size_t pb = s.pl.pb;
  hipStream_t st = s.st;
  const double* Y0 = ch.Wc;
  if (ch.Mc) {  // Y0 = Wc·Mc
    hipLaunchKernelGGL(k_cq_apply32, dim3(CQ_G), dim3(256), 0, st, ch.Wc, p, ch.Mc, w.T1);
    OCM_CHECK_LAUNCH("k_cq_apply32 cheb");
    Y0 = w.T1;
  }
  const double a1 = 2.0 / ch.cheb_beta, a2 = 4.0 / ch.cheb_beta;
  // products in this segment, degree d
  const int np = std::max(1, std::min(ch.cheb_dmax - (ch.y1_from_w ? 1 : 0), next_rr - it));
  const int d = np + (ch.y1_from_w ? 1 : 0);
  double* const buf[4] = {w.T2, w.T1, w.Wa, w.Wb};  // by ocm_eig::SegBuf, which picks each step's output
  int i1 = ocm_eig::SEG_V, i2 = ocm_eig::SEG_NONE;  // (Y0 is live only as Y_{j−1} or Y_{j−2})
  for (int c = 0; c < 4; ++c)
    if (buf[c] == Y0) i1 = c;
  const double *ym1 = Y0, *ym2 = nullptr;  // Y_{j−1}, Y_{j−2}
  for (int j = 1; j <= d; ++j) {
    const int io = ocm_eig::cheb_out(j, d, i1, i2);
    if (io == ocm_eig::SEG_NONE) return ocm::fail(OCM_ERR_ARG, "ocm_eig_topk: no free block for the Chebyshev filter");
    double* out = buf[io];
    if (j == 1 && ch.y1_from_w) {  // Y1 = X·V = (2/β)·W − V, W = C·V from the test's step
      hipLaunchKernelGGL(k_axpby, dim3((unsigned)((pb + 255) / 256)), dim3(256), 0, st, w.W, Y0, (int64_t)pb, a1, -1.0,
                         out);
      OCM_CHECK_LAUNCH("k_axpby cheb");
    } else if (j == 1) {  // Y1 = (2/β)·C·Y0 − Y0
      hipLaunchKernelGGL(k_cv32x, dim3(2 * cv_rb), dim3(512), 0, st, s.C, p, Y0, out, w.cv_part, w.cv_ticket, a1, -1.0,
                         nullptr, 0.0);
      OCM_CHECK_LAUNCH("k_cv32x cheb");
    } else {  // Y_j = (4/β)·C·Y_{j−1} − 2·Y_{j−1} − Y_{j−2}
      hipLaunchKernelGGL(k_cv32x, dim3(2 * cv_rb), dim3(512), 0, st, s.C, p, ym1, out, w.cv_part, w.cv_ticket, a2, -2.0,
                         ym2, -1.0);
      OCM_CHECK_LAUNCH("k_cv32x cheb");
    }
    ym2 = ym1;
    ym1 = out;
    i2 = i1;
    i1 = io;
  }
  ch.y1_from_w = false;
  double* Yd = buf[i1];
  double* Mn = w.Mf + 1024 * ch.mslot;
  hipLaunchKernelGGL(k_cq_gram32<false>, dim3(CQ_G), dim3(256), 0, st, Yd, p, nullptr, nullptr, w.cq_part, w.cq_ticket,
                     1, (uint64_t)(1500 + it), Mn);
  OCM_CHECK_LAUNCH("k_cq_gram32 cheb");
  ch.Wc = Yd;
  ch.Wn = (Yd == w.Wa) ? w.Wb : w.Wa;
  ch.Mc = Mn;
  ch.mslot ^= 1;
  ch.Sprev = nullptr;
  *np_out = np;
  return OCM_OK;
}

// one plain iteration: W ← (C·Wc)·Mc and its factor, one launch
int chain_step(const EigState& s, Chain32& ch, int it, int next_rr) {
  const ocm_eig::Layout& w = s.w;
  const int cv_rb = s.pl.cv_rb;
  double* Mn = w.Mf + 1024 * ch.mslot;
  // the next launch is a plain iteration too: it factors this one's Gram
  // in a wave of its own (k_cvq32<true>), off the critical path
  const int defer_next = it + 1 < next_rr ? 1 : 0;
  double* Sout = w.Sb + 1056 * ch.sslot;
  if (ch.Sprev)
    hipLaunchKernelGGL(k_cvq32<true>, dim3(2 * cv_rb), dim3(512), 0, s.st, s.C, s.p, ch.Wc, ch.Mc, ch.Wn, w.cv_part,
                       w.cv_ticket, w.gpart, w.gtick, (uint64_t)(500 + it), Mn, ch.Sprev, Sout, defer_next);
  else
    hipLaunchKernelGGL(k_cvq32<false>, dim3(2 * cv_rb), dim3(512), 0, s.st, s.C, s.p, ch.Wc, ch.Mc, ch.Wn, w.cv_part,
                       w.cv_ticket, w.gpart, w.gtick, (uint64_t)(500 + it), Mn, nullptr, Sout, defer_next);
  OCM_CHECK_LAUNCH("k_cvq32");
  ch.Sprev = defer_next ? Sout : nullptr;
  ch.sslot ^= 1;
  ch.Wc = ch.Wn;
  ch.Wn = (ch.Wn == w.Wa) ? w.Wb : w.Wa;
  ch.Mc = Mn;
  ch.mslot ^= 1;
  return OCM_OK;
}

// the Rayleigh–Ritz basis V = CholQR2 of the chain's block: T = Wc·Mc and
// its factor M2 (k_cq_gram32<true>) while a side stream forms C·Wc; then
// V = T·M2, W = C·V = (C·Wc)·(Mc·M2) and H = VᵀW in one launch
int rr_basis32(const EigState& s, Chain32& ch, int it) {
  const ocm_eig::Layout& w = s.w;
  ocm_ctx* ctx = s.ctx;
  hipStream_t st = s.st;
  int rc = eig_side_init(ctx);
  if (rc) return rc;
  hipStream_t sc = ctx->eig_side[1];
  OCM_HIP(hipEventRecord(ctx->eig_ev[0], st));
  OCM_HIP(hipStreamWaitEvent(sc, ctx->eig_ev[0], 0));
  hipLaunchKernelGGL(k_cv32, dim3(2 * s.pl.cv_rb), dim3(512), 0, sc, s.C, s.p, ch.Wc, w.T2, w.cv_part, w.cv_ticket);
  OCM_CHECK_LAUNCH("k_cv32 CWc");
  OCM_HIP(hipEventRecord(ctx->eig_ev[4], sc));
  hipLaunchKernelGGL(k_cq_gram32<true>, dim3(CQ_G), dim3(256), 0, st, ch.Wc, s.p, ch.Mc, w.T1, w.cq_part, w.cq_ticket,
                     0, (uint64_t)(700 + it), w.cq_M);
  OCM_CHECK_LAUNCH("k_cq_gram32 rr");
  OCM_HIP(hipStreamWaitEvent(st, ctx->eig_ev[4], 0));
  hipLaunchKernelGGL(k_rr_basis32, dim3(CQ_G), dim3(256), 0, st, w.T1, w.T2, s.p, ch.Mc, w.cq_M, w.V, w.W, w.cq_part,
                     w.cq_ticket, w.H);
  OCM_CHECK_LAUNCH("k_rr_basis32");
  ch.Mc = nullptr;
  return OCM_OK;
}

// Rayleigh–Ritz on the unrotated block, V, W = C·V and H = VᵀW given: the
// projection residual R = W − V·H and S = RᵀR, Jacobi on H; the test reads
// ‖R z_i‖ (at the Jacobi's end).  With θ wanted, R/S, C·R, G2 = Rᵀ(C·R) and
// the deflation of the whole block run on side streams beside the Jacobi
// (they need no Ritz rotation: k_theta_combine adds its terms later).  (The
// eigenproblem of H on the host — implicit QL, ocm_hostla.h — measured
// slower: ≈ 50–90 µs of QL plus two round trips against the 135 µs Jacobi,
// profiles/r05m_eig_timeline.txt.)  Leaves the test's θ and residuals in
// s.hres and, queued, every output of the call as a converged test wants it.
int rr_step32(const EigState& s) {
  const ocm_eig::Layout& w = s.w;
  ocm_ctx* ctx = s.ctx;
  hipStream_t st = s.st;
  const int p = s.p, k = s.k, b = s.pl.b, cv_rb = s.pl.cv_rb, theta_mode = s.theta_mode;
  // two side streams when θ is wanted: A deflates the block and runs θ3;
  // B forms R and S (handed to the Jacobi's test in flight), then C·R and
  // G2.  The Jacobi stays on the launch stream, queued first: it then
  // starts at once on an idle chip (107 µs; 128–145 µs when it started
  // behind the deflation's workgroups with the θ3 chain on the launch
  // stream, r05s4–r05s7)
  hipStream_t sa = st, sb = st;
  int rc = eig_side_init(ctx);  // the streams and events (the test's read-back event too)
  if (rc) return rc;
  if (theta_mode) {
    sa = ctx->eig_side[0];
    sb = ctx->eig_side[1];
    OCM_HIP(hipEventRecord(ctx->eig_ev[0], st));
    OCM_HIP(hipStreamWaitEvent(sa, ctx->eig_ev[0], 0));
    OCM_HIP(hipStreamWaitEvent(sb, ctx->eig_ev[0], 0));
  }
  double* R = w.T1;
  double* CR = w.T2;
  // S reaches the Jacobi's fused test in flight (ctx->eig_flag)
  const unsigned epoch = ++ctx->eig_epoch;
  hipLaunchKernelGGL(k_rr_resid32, dim3(CQ_G), dim3(256), 0, sb, w.V, w.W, p, w.H, R, w.cq_part, w.cq_ticket, w.S,
                     ctx->eig_flag, epoch);
  OCM_CHECK_LAUNCH("k_rr_resid32");
  if (theta_mode) {
    hipLaunchKernelGGL(k_cv32, dim3(2 * cv_rb), dim3(512), 0, sb, s.C, p, R, CR, w.cv_part, w.cv_ticket);
    OCM_CHECK_LAUNCH("k_cv32 CR");
    if (theta_mode >= 2) {
      hipLaunchKernelGGL(k_atb32, dim3(CQ_G), dim3(256), 0, sb, R, CR, p, w.cq_part, w.cq_ticket, w.L);  // G2
      OCM_CHECK_LAUNCH("k_atb32 G2");
    }
    OCM_HIP(hipEventRecord(ctx->eig_ev[3], sb));
    // after B's test inputs: theta_deflated queues its Δ terms on B too
    rc = theta_deflated(s, w.V, w.W, w.H, b, sa, sb, ctx->eig_sub, w.tr3);
    if (rc) return rc;
    OCM_HIP(hipEventRecord(ctx->eig_ev[2], sa));
  }
  // the Jacobi and the test in one launch (the former k_rr_test32's sums)
  double *theta = w.theta, *res = w.theta + b;
  rc = jacobi(w.H, b, 40, theta, w.Z, st, w.S, ctx->eig_flag, epoch, k, res);
  if (rc) return rc;
  OCM_HIP(hipMemcpyAsync(s.hres, theta, 2 * (size_t)b * sizeof(double), hipMemcpyDeviceToHost, st));
  OCM_HIP(hipEventRecord(ctx->eig_ev[6], st));
  // R (= T1) and CR are reused below: side stream B is done with them
  if (theta_mode) OCM_HIP(hipStreamWaitEvent(st, ctx->eig_ev[3], 0));
  // the outputs of a converged test are queued before the host has read
  // it (the GPU would idle through the round trip otherwise): the Ritz
  // vectors V·Z into T1, λ and the eigenvectors, then θ once side stream
  // A is done.  A test that fails leaves them to be overwritten.
  hipLaunchKernelGGL(k_cq_apply32, dim3(CQ_G), dim3(256), 0, st, w.V, p, w.Z, w.T1);  // Ritz vectors
  OCM_CHECK_LAUNCH("k_cq_apply32 ritz");
  hipLaunchKernelGGL(k_extract_signfix, dim3(k), dim3(256), 0, st, w.T1, p, b, k, s.evecs_out, theta, s.evals_out,
                     s.rcond, s.inv_out);
  OCM_CHECK_LAUNCH("k_extract_signfix");
  if (theta_mode) {  // (the deflation operands and the θ3 arena are reused by the next test too)
    OCM_HIP(hipStreamWaitEvent(st, ctx->eig_ev[2], 0));
    hipLaunchKernelGGL(k_theta_combine, dim3(1), dim3(256), 0, st, theta, w.Z, w.S, w.L, w.tr3, b, k,
                       s.slice == 0 ? 1 : 0, theta_mode >= 2 ? 1 : 0, s.theta_out);
    OCM_CHECK_LAUNCH("k_theta_combine");
  }
  OCM_HIP(hipEventSynchronize(ctx->eig_ev[6]));
  if (ocm_eig::verdict(s.hres, k, b, s.tol).waited_out) {
    // the fused test gave up waiting for S (side stream B not scheduled
    // within ≈ 1 s): the launch stream has since waited for B's event, so
    // the same Jacobi + test runs again with S complete (the same Z and λ;
    // the outputs queued above read them before this rewrites them)
    ++ctx->eig_test_reruns;
    rc = jacobi(w.H, b, 40, theta, w.Z, st, w.S, ctx->eig_flag, epoch, k, res, OCM_JACOBI_SPINS_1S);
    if (rc) return rc;
    OCM_HIP(hipMemcpyAsync(s.hres, theta, 2 * (size_t)b * sizeof(double), hipMemcpyDeviceToHost, st));
    OCM_HIP(hipStreamSynchronize(st));
    if (ocm_eig::verdict(s.hres, k, b, s.tol).waited_out)
      return ocm::fail(OCM_ERR_HIP, "ocm_eig_topk: the Rayleigh-Ritz test's operand S was not ready after its "
                                    "producer finished");
  }
  return OCM_OK;
}

int eig_fused32(const EigState& s, int32_t* iters_out) {
  const ocm_eig::Layout& w = s.w;
  hipStream_t st = s.st;
  const int p = s.p, k = s.k, b = s.pl.b, max_iter = s.max_iter;
  int next_rr = std::min(PLAIN + 1, max_iter);
  int rc = eig_start_block(s, next_rr == 1);
  if (rc) return rc;
  if (next_rr == 1) {
    // V = CholQR2 of T1: the Gram and its factor M1, then T = T1·M1 (in place:
    // every wave rewrites only rows it has read) with the Gram of T and its
    // factor M2, then V = T·M2
    hipLaunchKernelGGL(k_cq_gram32<false>, dim3(CQ_G), dim3(256), 0, st, w.T1, p, nullptr, nullptr, w.cq_part,
                       w.cq_ticket, 1, (uint64_t)1, w.cq_M);
    OCM_CHECK_LAUNCH("k_cq_gram32");
    hipLaunchKernelGGL(k_cq_gram32<true>, dim3(CQ_G), dim3(256), 0, st, w.T1, p, w.cq_M, w.T1, w.cq_part, w.cq_ticket,
                       0, (uint64_t)1, w.cq_M + 1024);
    OCM_CHECK_LAUNCH("k_cq_gram32 apply");
    hipLaunchKernelGGL(k_cq_apply32, dim3(CQ_G), dim3(256), 0, st, w.T1, p, w.cq_M + 1024, w.V);
    OCM_CHECK_LAUNCH("k_cq_apply32");
  }
  Chain32 ch{w.V, w.Wa};
  ocm_eig::Schedule sched;
  bool converged = false;
  int it;
  for (it = 1; it <= max_iter; ++it) {
    if (ch.cheb && it < next_rr) {
      int np = 0;
      rc = cheb_segment(s, ch, it, next_rr, &np);
      if (rc) return rc;
      it += np - 1;  // (the loop adds the last)
      continue;
    }
    if (it < next_rr) {
      rc = chain_step(s, ch, it, next_rr);
      if (rc) return rc;
      continue;
    }
    if (ch.Mc) {
      rc = rr_basis32(s, ch, it);
      if (rc) return rc;
    } else {  // the test on the first product (max_iter = 1), V orthonormal: W = C V, H = VᵀW
      hipLaunchKernelGGL(k_cv32, dim3(2 * s.pl.cv_rb), dim3(512), 0, st, s.C, p, w.V, w.W, w.cv_part, w.cv_ticket);
      OCM_CHECK_LAUNCH("k_cv32");
      hipLaunchKernelGGL(k_atb32, dim3(CQ_G), dim3(256), 0, st, w.V, w.W, p, w.cq_part, w.cq_ticket, w.H);
      OCM_CHECK_LAUNCH("k_atb32 H");
    }
    rc = rr_step32(s);
    if (rc) return rc;
    const double* h = s.hres;
    const ocm_eig::Verdict v = ocm_eig::verdict(h, k, b, s.tol);
    if (v.nan) return ocm::fail(OCM_ERR_ARG, "ocm_eig_topk: NaN in covariance");
    converged = v.converged;
    if (converged || it == max_iter) break;  // evals, evecs and θ are queued
    const double tb = std::fabs(h[b - 1]);
    const ocm_eig::Step nx = sched.next(it, max_iter, v.rmax, v.target, std::fabs(h[0]), std::fabs(h[k - 1]), tb, true);
    next_rr = nx.next_rr;
    ch.Sprev = nullptr;
    ch.cheb = nx.use_cheb && next_rr > it + 1;
    if (ch.cheb) {
      // the filter starts at the orthonormal basis V, whose C·V = W is in hand
      ch.cheb_beta = tb;
      ch.cheb_dmax = nx.dmax;
      ch.y1_from_w = true;
      ch.Wc = w.V;
      ch.Mc = nullptr;
      continue;
    }
    // the chain continues from W = C·V (span is all it needs) and its factor
    OCM_HIP(hipMemcpyAsync(w.Wa, w.W, s.pl.pb * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_cq_gram32<false>, dim3(CQ_G), dim3(256), 0, st, w.Wa, p, nullptr, nullptr, w.cq_part,
                       w.cq_ticket, 1, (uint64_t)(1000 + it), w.Mf);
    OCM_CHECK_LAUNCH("k_cq_gram32 chain");
    ch.Wc = w.Wa;
    ch.Wn = w.Wb;
    ch.Mc = w.Mf;
    ch.mslot = 1;
  }
  if (iters_out) *iters_out = std::min(it, max_iter);
  return converged ? OCM_OK : ocm::fail(OCM_ERR_NOCONV, "ocm_eig_topk: max_iter reached before tolerance");
}

// ---- b = 48 / 64 on the device, wider blocks with host b×b steps -------------
// wide: S = AᵀB on the device → host (s.hmat())
int proj_to_host(const EigState& s, const double* A, const double* B) {
  int rc = dgemm_ta(A, B, s.p, s.pl.b, s.w.S, s.w.planes, s.pl.plane_cap, s.st);
  if (rc) return rc;
  OCM_HIP(hipMemcpyAsync(s.hmat(), s.w.S, s.pl.bb * sizeof(double), hipMemcpyDeviceToHost, s.st));
  OCM_HIP(hipStreamSynchronize(s.st));
  return OCM_OK;
}

// CholQR2 of the column-normalised Win; result in Vout (Win is clobbered)
int orth_block(const EigState& s, double* Win, double* Vout, uint64_t seed) {
  const ocm_eig::Layout& w = s.w;
  hipStream_t st = s.st;
  const int p = s.p, b = s.pl.b;
  const size_t pb = s.pl.pb, bb = s.pl.bb;
  hipLaunchKernelGGL(k_colnormalize, dim3(b), dim3(256), 0, st, Win, p, b, seed);
  OCM_CHECK_LAUNCH("k_colnormalize");
  for (int pass = 0; pass < 2; ++pass) {
    if (s.pl.wide()) {  // pass 0: Win → Vout; pass 1: Vout → Win → Vout (the GEMM cannot run in place)
      double* src = pass == 0 ? Win : Vout;
      double* dst = pass == 0 ? Vout : Win;
      double* hmat = s.hmat();
      int rc = proj_to_host(s, src, src);
      if (rc) return rc;
      ocm::host_chol_inv_t(hmat, b, hmat + bb);
      OCM_HIP(hipMemcpyAsync(w.L, hmat + bb, bb * sizeof(double), hipMemcpyHostToDevice, st));
      rc = dgemm(src, b, w.L, b, dst, b, p, b, b, 1, nullptr, st);
      if (rc) return rc;
      if (pass == 1) OCM_HIP(hipMemcpyAsync(Vout, Win, pb * sizeof(double), hipMemcpyDeviceToDevice, st));
      OCM_HIP(hipStreamSynchronize(st));  // hmat is reused by the next pass
      continue;
    }
    double* src = pass == 0 ? Win : Vout;  // b = 48 or 64
    int rc = atb(src, src, p, b, w.S, w.apart, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_chol, dim3(1), dim3(256), 0, st, w.S, b, w.L);
    OCM_CHECK_LAUNCH("k_chol");
    rc = trsm_rows(src, w.L, p, b, Vout, st);
    if (rc) return rc;
  }
  return OCM_OK;
}

// out = Aᵀ B (b×b) on the device
int project(const EigState& s, const double* A, const double* B, double* out) {
  if (s.pl.wide()) return dgemm_ta(A, B, s.p, s.pl.b, out, s.w.planes, s.pl.plane_cap, s.st);
  return atb(A, B, s.p, s.pl.b, out, s.w.apart, s.st);
}

// Ritz values (theta, descending) and rotations Z of H = Vᵀ W
int ritz(const EigState& s, const double* V, const double* W) {
  const ocm_eig::Layout& w = s.w;
  const int b = s.pl.b;
  const size_t bb = s.pl.bb;
  if (!s.pl.wide()) {
    int rc = project(s, V, W, w.H);
    if (rc) return rc;
    return jacobi(w.H, b, 40, w.theta, w.Z, s.st);
  }
  int rc = proj_to_host(s, V, W);
  if (rc) return rc;
  double* hmat = s.hmat();
  if (!ocm::host_sym_eig(hmat, b, hmat + 2 * bb, hmat + bb)) {
    ocm::set_error("ocm_eig_topk: implicit QL of the Rayleigh-Ritz problem did not converge");
    return OCM_ERR_NOCONV;
  }
  OCM_HIP(hipMemcpyAsync(w.Z, hmat + bb, bb * sizeof(double), hipMemcpyHostToDevice, s.st));
  OCM_HIP(hipMemcpyAsync(w.theta, hmat + 2 * bb, b * sizeof(double), hipMemcpyHostToDevice, s.st));
  return OCM_OK;
}

int eig_block(const EigState& s, int32_t* iters_out) {
  const ocm_eig::Layout& w = s.w;
  hipStream_t st = s.st;
  const int p = s.p, k = s.k, b = s.pl.b, max_iter = s.max_iter;
  const size_t pb = s.pl.pb;
  double *V = w.V, *W = w.W, *T1 = w.T1, *T2 = w.T2, *theta = w.theta, *res = w.theta + b;
  int next_rr = std::min(PLAIN + 1, max_iter);
  int rc = eig_start_block(s, next_rr == 1);
  if (rc) return rc;
  if (next_rr == 1) {
    rc = orth_block(s, T1, V, 1);
    if (rc) return rc;
  }
  ocm_eig::Schedule sched;
  bool converged = false;
  int it;
  for (it = 1; it <= max_iter; ++it) {
    rc = dgemm(s.C, p, V, b, W, b, p, b, p, s.pl.ksplit, w.planes, st);  // W = C V
    if (rc) return rc;
    if (it < next_rr) {  // W is not needed again (recomputed next iteration)
      rc = orth_block(s, W, V, 500 + it);
      if (rc) return rc;
      continue;
    }
    rc = ritz(s, V, W);
    if (rc) return rc;
    rc = dgemm(V, b, w.Z, b, T1, b, p, b, b, 1, nullptr, st);  // Ritz vectors
    if (rc) return rc;
    rc = dgemm(W, b, w.Z, b, T2, b, p, b, b, 1, nullptr, st);  // C · Ritz vectors
    if (rc) return rc;
    std::swap(V, T1);
    std::swap(W, T2);
    hipLaunchKernelGGL(k_ritz_residual, dim3(k), dim3(256), 0, st, W, V, theta, p, b, res);
    OCM_CHECK_LAUNCH("k_ritz_residual");
    OCM_HIP(hipMemcpyAsync(s.hres, theta, 2 * (size_t)b * sizeof(double), hipMemcpyDeviceToHost, st));
    OCM_HIP(hipStreamSynchronize(st));
    const double* h = s.hres;
    const ocm_eig::Verdict v = ocm_eig::verdict(h, k, b, s.tol);
    if (v.nan) return ocm::fail(OCM_ERR_ARG, "ocm_eig_topk: NaN in covariance");
    converged = v.converged;
    if (converged || it == max_iter) break;  // V, W, theta are consistent for the outputs
    next_rr = sched.next(it, max_iter, v.rmax, v.target, std::fabs(h[0]), std::fabs(h[k - 1]), std::fabs(h[b - 1]),
                         false).next_rr;
    // next basis: orth(C · Ritz vectors)
    OCM_HIP(hipMemcpyAsync(T1, W, pb * sizeof(double), hipMemcpyDeviceToDevice, st));
    rc = orth_block(s, T1, V, 1000 + it);
    if (rc) return rc;
  }
  if (iters_out) *iters_out = std::min(it, max_iter);
  hipLaunchKernelGGL(k_extract_signfix, dim3(k), dim3(256), 0, st, V, p, b, k, s.evecs_out, theta, s.evals_out);
  OCM_CHECK_LAUNCH("k_extract_signfix");
  if (s.inv_out) hipLaunchKernelGGL(k_inv_evals, dim3(1), dim3(256), 0, st, s.evals_out, k, s.rcond, s.inv_out);
  if (s.theta_mode) {
    // H_k = V_kᵀ (C V_k): the projected block of the Ritz vectors; deflate
    // the leading k of them
    rc = project(s, V, W, w.H);
    if (rc) return rc;
    rc = theta_deflated(s, V, W, w.H, k, st, st, s.ctx, s.theta_out);
    if (rc) return rc;
  }
  return converged ? OCM_OK : ocm::fail(OCM_ERR_NOCONV, "ocm_eig_topk: max_iter reached before tolerance");
}

int eig_topk_impl(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                  int32_t theta_mode, int32_t slice, int32_t nslices, double* evals_out, double* evecs_out,
                  double* theta_out, int32_t* iters_out, hipStream_t st, double* inv_out = nullptr,
                  double rcond = 1e-15) {
  if (tol <= 0) tol = 1e-10;
  if (max_iter <= 0) max_iter = 2000;
  EigState s{ctx, st, C, p, k, tol, max_iter, theta_mode, slice, nslices, evals_out, evecs_out, theta_out, inv_out,
             rcond};
  s.pl = ocm_eig::make_plan(p, k, theta_mode);
  OCM_REQUIRE(s.pl.ok, "ocm_eig_topk: p too small for the block path");
  ocm::Carve measure{nullptr};
  ocm_eig::carve(s.pl, measure);
  void* ws = ocm::workspace(ctx, measure.off, st);
  if (!ws) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(ws)};
  s.w = ocm_eig::carve(s.pl, cv);
  if (s.pl.path == ocm_eig::Path::small) {
    const int rc = eig_small(s);
    if (!rc && iters_out) *iters_out = 1;
    return rc;
  }
  s.hres = static_cast<double*>(ocm::host_staging(ctx, s.pl.host_doubles * sizeof(double)));
  if (!s.hres) return OCM_ERR_NOMEM;
  return s.pl.fused() ? eig_fused32(s, iters_out) : eig_block(s, iters_out);
}


}  // namespace

extern "C" {

int ocm_eig_topk(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                 int32_t theta_mode, double* evals_out, double* evecs_out, double* theta_out, int32_t* iters_out,
                 void* stream) {
  OCM_REQUIRE(ctx && C && evals_out && evecs_out, "ocm_eig_topk: NULL argument");
  OCM_REQUIRE(p >= 1 && k >= 1 && k <= p, "ocm_eig_topk: need 1 <= k <= p");
  OCM_REQUIRE(theta_mode == 0 || theta_out, "ocm_eig_topk: theta_out is NULL");
  return eig_topk_impl(ctx, C, p, k, tol, max_iter, theta_mode, 0, 1, evals_out, evecs_out, theta_out, iters_out,
                       (hipStream_t)stream);
}

int ocm_eig_topk_ex(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                    int32_t theta_mode, int32_t theta3_slice, int32_t theta3_nslices, double* evals_out,
                    double* evecs_out, double* theta_out, int32_t* iters_out, void* stream) {
  OCM_REQUIRE(ctx && C && evals_out && evecs_out, "ocm_eig_topk_ex: NULL argument");
  OCM_REQUIRE(p >= 1 && k >= 1 && k <= p, "ocm_eig_topk_ex: need 1 <= k <= p");
  OCM_REQUIRE(theta_mode == 0 || theta_out, "ocm_eig_topk_ex: theta_out is NULL");
  OCM_REQUIRE(theta3_nslices >= 1 && theta3_slice >= 0 && theta3_slice < theta3_nslices,
              "ocm_eig_topk_ex: need 0 <= theta3_slice < theta3_nslices");
  return eig_topk_impl(ctx, C, p, k, tol, max_iter, theta_mode, theta3_slice, theta3_nslices, evals_out, evecs_out,
                       theta_out, iters_out, (hipStream_t)stream);
}

int ocm_eig_topk_ex2(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                     int32_t theta_mode, int32_t theta3_slice, int32_t theta3_nslices, double* evals_out,
                     double* evecs_out, double* theta_out, int32_t* iters_out, double rcond, double* inv_out,
                     void* stream) {
  OCM_REQUIRE(ctx && C && evals_out && evecs_out && inv_out, "ocm_eig_topk_ex2: NULL argument");
  OCM_REQUIRE(p >= 1 && k >= 1 && k <= p, "ocm_eig_topk_ex2: need 1 <= k <= p");
  OCM_REQUIRE(theta_mode == 0 || theta_out, "ocm_eig_topk_ex2: theta_out is NULL");
  OCM_REQUIRE(theta3_nslices >= 1 && theta3_slice >= 0 && theta3_slice < theta3_nslices,
              "ocm_eig_topk_ex2: need 0 <= theta3_slice < theta3_nslices");
  return eig_topk_impl(ctx, C, p, k, tol, max_iter, theta_mode, theta3_slice, theta3_nslices, evals_out, evecs_out,
                       theta_out, iters_out, (hipStream_t)stream, inv_out, rcond);
}

int ocm_inv_evals_f64(ocm_ctx* ctx, const double* evals, int32_t k, double rcond, double* out, void* stream) {
  OCM_REQUIRE(ctx && evals && out, "ocm_inv_evals_f64: NULL argument");
  OCM_REQUIRE(k >= 1, "ocm_inv_evals_f64: k >= 1");
  hipLaunchKernelGGL(k_inv_evals, dim3(1), dim3(256), 0, (hipStream_t)stream, evals, k, rcond, out);
  OCM_CHECK_LAUNCH("k_inv_evals");
  return OCM_OK;
}

int ocm_sym_pinv_f64(ocm_ctx* ctx, const double* A, int32_t d, double rcond, double* out, void* stream) {
  OCM_REQUIRE(ctx && A && out, "ocm_sym_pinv_f64: NULL argument");
  OCM_REQUIRE(d >= 1 && d <= JMAX, "ocm_sym_pinv_f64: 1 <= d <= 64");
  hipStream_t st = (hipStream_t)stream;
  void* w = ocm::workspace(ctx, (size_t)(d + d * d + 64) * sizeof(double), st);
  if (!w) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(w)};
  double* ev = cv.take<double>(d);
  double* Z = cv.take<double>((size_t)d * d);
  const int rc = jacobi(A, d, 60, ev, Z, st);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pinv_from_eig, dim3((d * d + 255) / 256), dim3(256), 0, st, ev, Z, d,
                     rcond > 0 ? rcond : 1e-15, out);
  OCM_CHECK_LAUNCH("k_pinv_from_eig");
  return OCM_OK;
}

}  // extern "C"
