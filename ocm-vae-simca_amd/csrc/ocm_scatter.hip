// Multiplicative scatter correction (MSC) and its extended form (EMSC), the
// reference-spectrum counterparts of the SNV (include/ocm.h, "scatter
// correction"):
//   c = W·x          q row coefficients of the least-squares fit of the row on
//                    the basis B (q × p: ones, the reference spectrum, baseline
//                    and interferent terms), W = pinv(Bᵀ) from the host
//   MSC  (q = 2)     y_j = (x_j − c0) / c1
//   EMSC (q ≤ 8)     y_j = (x_j − c0 − Σ_{t≥2} c_t·B_tj) / c1
// ocm_rowfit_f32 is the read-only pass (coefficients and / or the (m_r, s_r)
// pair of a lazy view); ocm_emsc_apply_f32 reads each row once, forms c and
// writes y.  One wave per row, eight rows per workgroup, the row in registers
// for p ≤ 4096 (float4 pieces at columns 256k + 4·lane, as k_prep_rowstats
// holds it); any p, leading dimension or alignment takes the scalar path,
// which reads the row again (from cache) to apply.  The q dot products run
// in fp64 ((double)x_j·W_tj, fixed order, no atomics): with a raw baseline of
// 100 on the spectra float32 products cost 1e-3 on c0.  W is q·p·8 bytes
// (32 KiB at q = 2, p = 2048), four times the row at q = 2: a workgroup stages
// it in LDS once and then walks over 16 groups of 8 rows, so W costs one L2
// read per 128 rows, not one per row (the apply pass keeps the baseline rows of
// B there too, as float32); past 80 KiB the lanes read W and B from L2.
#include "ocm_internal.h"

namespace {

constexpr int SC_QMAX = 8;
constexpr size_t SC_LDS_MAX = 80 * 1024;   // W (and the apply pass's B) staged in LDS up to here: two workgroups per CU
constexpr int SC_NT = 512;                  // threads per workgroup
constexpr int SC_ROWS = SC_NT / 64;         // one wave per row
constexpr int SC_CHUNK = 16;                // row groups per workgroup: W is staged once per 128 rows

typedef double f64x2 __attribute__((ext_vector_type(2)));

// MAXSEG > 0: the row in registers (p % 4 == 0, p ≤ 256·MAXSEG, 16-byte aligned
// rows, W and B); MAXSEG == 0: any p, scalar loads.  Q: the unrolled bound of
// the coefficient loops (q ≤ Q; Q = 2 is q = 2).  Lane sums: two partial fp64
// sums per coefficient (even / odd elements of the lane), added, then the xor
// butterfly.
//
// SC_NT threads = 8 waves share one copy of W (at q = 2, p = 2048, 32 KiB: four workgroups, so 8 waves
// per SIMD, on a CU).  The register path keeps W in LDS in the order the lanes read it: per
// coefficient and 256-column segment two 1-KiB halves, half h holding for lane l the columns
// 4l + 2h, 4l + 2h + 1 of the segment, so a lane's two reads per segment are 16 bytes at stride 16
// across the wave (ds_read_b128 without bank conflicts; in column order a lane's 32 bytes at stride
// 32 conflict four ways as 8-byte reads, and the LDS then bounds the pass: measured 3.9 TB/s).  The
// columns of the last segment past p hold 0 and the row registers there hold 0, so the sums need no
// column guard.
template <int MAXSEG, int Q, bool APPLY, bool WLDS>
__global__ __launch_bounds__(SC_NT) void k_scatter(const float* __restrict__ X, int64_t ldx, int64_t m, int p, int q,
                                                   const double* __restrict__ W, const double* __restrict__ B,
                                                   float* __restrict__ coef_out, float* __restrict__ rowstat_out,
                                                   float* __restrict__ out, int64_t ldo) {
  // WLDS: [q][p rounded up to 256] (+ float [q − 2][the same] of B), or on the scalar path [q][p]
  extern __shared__ f64x2 sW2[];
  double* sW = reinterpret_cast<double*>(sW2);
  const int pseg = (p + 255) & ~255;  // the register path's row pitch in LDS
  if constexpr (WLDS) {
    if constexpr (MAXSEG > 0) {
      for (int t = 0; t < q; ++t)
        for (int j = threadIdx.x; j < pseg; j += SC_NT) {
          const int e = j & 3, l = (j & 255) >> 2;
          sW[t * pseg + (j & ~255) + (e >> 1) * 128 + 2 * l + (e & 1)] = j < p ? W[(size_t)t * p + j] : 0.0;
        }
      if constexpr (APPLY) {  // the baseline rows of B behind W, as the float32 values the apply stage uses
        float* sB = reinterpret_cast<float*>(sW + q * pseg);
        for (int t = 2; t < q; ++t)
          for (int j = threadIdx.x; j < pseg; j += SC_NT)
            sB[(t - 2) * pseg + j] = j < p ? (float)B[(size_t)t * p + j] : 0.f;
      }
    } else {
      for (int i = threadIdx.x; i < q * p; i += SC_NT) sW[i] = W[i];
    }
    __syncthreads();
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t groups = (m + SC_ROWS - 1) / SC_ROWS;
  const int64_t g0 = (int64_t)blockIdx.x * SC_CHUNK;
  for (int64_t g = g0; g < g0 + SC_CHUNK && g < groups; ++g) {
    const int64_t r = g * SC_ROWS + wave;
    if (r >= m) continue;
    const float* xr = X + r * ldx;
    double acc[Q][2];
#pragma unroll
    for (int t = 0; t < Q; ++t) acc[t][0] = acc[t][1] = 0.0;
    double c[Q];
    if constexpr (MAXSEG > 0) {
      const int nseg = (p + 255) / 256;
      f32x4 x[MAXSEG];
#pragma unroll
      for (int k = 0; k < MAXSEG; ++k) {
        const int c0 = 256 * k + 4 * lane;
        x[k] = (k < nseg && c0 < p) ? *reinterpret_cast<const f32x4*>(xr + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int k = 0; k < MAXSEG; ++k) {
        const int c0 = 256 * k + 4 * lane;
        if (k < nseg && (WLDS || c0 < p)) {
#pragma unroll
          for (int t = 0; t < Q; ++t)
            if (Q == 2 || t < q) {
              f64x2 w0, w1;
              if constexpr (WLDS) {
                w0 = sW2[(t * pseg + 256 * k) / 2 + lane];
                w1 = sW2[(t * pseg + 256 * k) / 2 + 64 + lane];
              } else {
                w0 = *reinterpret_cast<const f64x2*>(W + (size_t)t * p + c0);
                w1 = *reinterpret_cast<const f64x2*>(W + (size_t)t * p + c0 + 2);
              }
              acc[t][0] = fma((double)x[k][0], w0[0], acc[t][0]);
              acc[t][1] = fma((double)x[k][1], w0[1], acc[t][1]);
              acc[t][0] = fma((double)x[k][2], w1[0], acc[t][0]);
              acc[t][1] = fma((double)x[k][3], w1[1], acc[t][1]);
            }
        }
      }
#pragma unroll
      for (int t = 0; t < Q; ++t) c[t] = (Q == 2 || t < q) ? wave_sum_f64(acc[t][0] + acc[t][1]) : 0.0;
      if constexpr (APPLY) {
        const float mf = (float)c[0], sf = (float)(1.0 / c[1]);
        float cf[Q];
#pragma unroll
        for (int t = 0; t < Q; ++t) cf[t] = (float)c[t];
        float* orow = out + r * ldo;
#pragma unroll
        for (int k = 0; k < MAXSEG; ++k) {
          const int c0 = 256 * k + 4 * lane;
          if (k < nseg && c0 < p) {
            f32x4 u;
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = __fsub_rn(x[k][e], mf);
#pragma unroll
            for (int t = 2; t < Q; ++t)
              if (t < q) {
                f32x4 b;
                if constexpr (WLDS) {
                  const float* sB = reinterpret_cast<const float*>(sW + q * pseg);
                  b = *reinterpret_cast<const f32x4*>(sB + (t - 2) * pseg + c0);
                } else {
                  const f64x2 b0 = *reinterpret_cast<const f64x2*>(B + (size_t)t * p + c0);
                  const f64x2 b1 = *reinterpret_cast<const f64x2*>(B + (size_t)t * p + c0 + 2);
                  b = f32x4{(float)b0[0], (float)b0[1], (float)b1[0], (float)b1[1]};
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) u[e] = fmaf(-cf[t], b[e], u[e]);
              }
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = ocm::mul_nc(u[e], sf);
            *reinterpret_cast<f32x4*>(orow + c0) = u;
          }
        }
      }
    } else {
      for (int j = lane, i = 0; j < p; j += 64, i ^= 1) {
        const double v = (double)xr[j];
#pragma unroll
        for (int t = 0; t < Q; ++t)
          if (t < q) {
            double w;
            if constexpr (WLDS)
              w = sW[(size_t)t * p + j];
            else
              w = W[(size_t)t * p + j];
            acc[t][0] = i == 0 ? fma(v, w, acc[t][0]) : acc[t][0];
            acc[t][1] = i == 1 ? fma(v, w, acc[t][1]) : acc[t][1];
          }
      }
#pragma unroll
      for (int t = 0; t < Q; ++t) c[t] = (Q == 2 || t < q) ? wave_sum_f64(acc[t][0] + acc[t][1]) : 0.0;
      if constexpr (APPLY) {
        const float mf = (float)c[0], sf = (float)(1.0 / c[1]);
        float cf[Q];
#pragma unroll
        for (int t = 0; t < Q; ++t) cf[t] = (float)c[t];
        float* orow = out + r * ldo;
        for (int j = lane; j < p; j += 64) {
          float u = __fsub_rn(xr[j], mf);
#pragma unroll
          for (int t = 2; t < Q; ++t)
            if (t < q) u = fmaf(-cf[t], (float)B[(size_t)t * p + j], u);
          orow[j] = ocm::mul_nc(u, sf);
        }
      }
    }
    if (lane == 0) {
      if (coef_out)
#pragma unroll
        for (int t = 0; t < Q; ++t)
          if (t < q) coef_out[r * q + t] = (float)c[t];
      if (rowstat_out) {
        rowstat_out[2 * r] = (float)c[0];
        rowstat_out[2 * r + 1] = (float)(1.0 / c[1]);
      }
    }
  }
}

inline bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

template <bool APPLY>
int launch_scatter(const float* X, int64_t ldx, int64_t m, int p, const double* W, const double* B,
                   int q, float* coef_out, float* rowstat_out, float* out, int64_t ldo, hipStream_t st) {
  // the register tile of p > 2048 beside more than four fp64 sums per lane does not fit the register file
  bool vec = p % 4 == 0 && (p <= 2048 || (p <= 4096 && q <= 4)) && ldx % 4 == 0 && aligned16(X) && aligned16(W);
  if (APPLY) vec = vec && ldo % 4 == 0 && aligned16(out) && aligned16(B);
  const size_t pseg = (size_t)(p + 255) / 256 * 256;
  const size_t wbytes = (size_t)q * (vec ? pseg : p) * sizeof(double) +
                        (APPLY && vec ? (q - 2) * pseg * sizeof(float) : 0);
  const bool wlds = wbytes <= SC_LDS_MAX;
  const size_t lds = wlds ? wbytes : 0;
  const int64_t groups = (m + SC_ROWS - 1) / SC_ROWS;
  // each workgroup stages W once and walks over SC_CHUNK consecutive row groups (at q = 2, p = 2048:
  // 32 KiB of W from L2 per 1 MiB of rows); the dispatcher balances the workgroups over the CUs
  const dim3 grid((unsigned)((groups + SC_CHUNK - 1) / SC_CHUNK));
#define OCM_SC(S_, Q_, L_)                                                                                         \
  hipLaunchKernelGGL((k_scatter<S_, Q_, APPLY, L_>), grid, dim3(SC_NT), lds, st, X, ldx, m, p, q, W, B, coef_out, \
                     rowstat_out, out, ldo)
#define OCM_SC_Q(S_, L_) \
  if (q <= 2)            \
    OCM_SC(S_, 2, L_);   \
  else if (q <= 4)       \
    OCM_SC(S_, 4, L_);   \
  else                   \
    OCM_SC(S_, 8, L_);
#define OCM_SC_S(L_)        \
  if (vec && p <= 2048) {   \
    OCM_SC_Q(8, L_)         \
  } else if (vec) {         \
    if (q <= 2)             \
      OCM_SC(16, 2, L_);    \
    else                    \
      OCM_SC(16, 4, L_);    \
  } else {                  \
    OCM_SC_Q(0, L_)         \
  }
  if (wlds) {
    OCM_SC_S(true)
  } else {
    OCM_SC_S(false)
  }
#undef OCM_SC_S
#undef OCM_SC_Q
#undef OCM_SC
  OCM_CHECK_LAUNCH("k_scatter");
  return OCM_OK;
}

}  // namespace

extern "C" {

int ocm_rowfit_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const double* W, int32_t q,
                   float* coef_out, float* rowstat_out, void* stream) {
  OCM_REQUIRE(ctx && X && W, "ocm_rowfit_f32: NULL argument");
  OCM_REQUIRE(coef_out || rowstat_out, "ocm_rowfit_f32: coef_out and rowstat_out are both NULL");
  OCM_REQUIRE(q >= 2 && q <= SC_QMAX, "ocm_rowfit_f32: q must be in [2, 8]");
  OCM_REQUIRE(m >= 0 && p >= q && ldx >= p, "ocm_rowfit_f32: bad shape (p >= q, ldx >= p)");
  OCM_REQUIRE(m < (1LL << 31), "ocm_rowfit_f32: too many rows per call");
  if (m == 0) return OCM_OK;
  return launch_scatter<false>(X, ldx, m, p, W, nullptr, q, coef_out, rowstat_out, nullptr, 0,
                               (hipStream_t)stream);
}

int ocm_emsc_apply_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const double* W,
                       const double* B, int32_t q, float* out, int64_t ldo, float* coef_out, void* stream) {
  OCM_REQUIRE(ctx && X && W && out, "ocm_emsc_apply_f32: NULL argument");
  OCM_REQUIRE(q >= 2 && q <= SC_QMAX, "ocm_emsc_apply_f32: q must be in [2, 8]");
  OCM_REQUIRE(B || q == 2, "ocm_emsc_apply_f32: the basis B is required for q > 2");
  OCM_REQUIRE(m >= 0 && p >= q && ldx >= p && ldo >= p, "ocm_emsc_apply_f32: bad shape (p >= q, ldx, ldo >= p)");
  OCM_REQUIRE(m < (1LL << 31), "ocm_emsc_apply_f32: too many rows per call");
  if (m == 0) return OCM_OK;
  return launch_scatter<true>(X, ldx, m, p, W, B, q, coef_out, nullptr, out, ldo, (hipStream_t)stream);
}

}  // extern "C"
