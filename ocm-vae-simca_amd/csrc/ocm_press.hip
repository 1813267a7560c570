// Element-wise cross-validation of a PCA model (ekf: Bro, Kjeldahl, Smilde,
// Kiers 2008): the predicted residual sum of squares of held-out rows for
// every number of components 0..K in one read of the rows.
//
// With y = x − μ, t = P·y (P: K × p, orthonormal rows), the residual after k
// components r⁽ᵏ⁾ = y − Σ_{a≤k} t_a·P_a and the leverage of variable j
// h_j⁽ᵏ⁾ = Σ_{a≤k} P_aj², the error of predicting variable j from the other
// p − 1 through the loadings is e_j⁽ᵏ⁾ = r_j⁽ᵏ⁾ / (1 − h_j⁽ᵏ⁾) (Sherman–Morrison
// on P₋ⱼᵀP₋ⱼ = I − p_j·p_jᵀ), so
//   PRESS_k = Σ_rows Σ_j w_k[j]·(r_j⁽ᵏ⁾)²,   w_k[j] = 1 / (1 − h_j⁽ᵏ⁾)²
//   naive_k = Σ_rows Σ_j (r_j⁽ᵏ⁾)²           (the row-wise curve: Σ Q at k)
//
// k_press_weights: workgroup k forms w_k[·] in fp64 (rounded once to the
//   element type of the main kernel); 1 − h ≤ 1e-8 gives weight 0 and counts in
//   ndegen[k].
// k_press: four waves per 16-row tile, as k_contrib.  A workgroup owns whole
//   chunks of 256 rows (16 tiles) at multiples of 256.
//   sweep 1  Tᵀ (comps × rows) += P_chunk · Y_chunkᵀ on 16x16x4 MFMA, f32
//            partials over 64 columns flushed to f64; the centred tile y stays
//            in LDS where 16 × p values fit once per resident workgroup, wider
//            rows are read a second time (out of L2);
//   reduce   the waves' partial t meet in LDS (f64, fixed order) and stay there
//            rounded to the element type, as [comp][row];
//   sweep 2  per 64-column block a lane holds 4 rows × 4 columns of the
//            residual in registers and walks k = 1..K: r ← r − t_k·P_k, then
//            Σ w_k·r² and Σ r² into per-lane accumulators (element type);
//   sums     a lane keeps its sums over the tiles of a chunk (float32, K ≤ 32: at
//            most 128 block sums; otherwise one tile), then lanes → wave (fp64
//            butterflies) → workgroup (waves in order, LDS), added to the
//            chunk's sum in tile order; per chunk one slot of 2·(K + 1) doubles.
// k_press_reduce: output o adds its chunk partials in chunk order: thread t
//   the consecutive chunks [t·L, (t + 1)·L), thread 0 the 256 subtotals in order.
// No atomics, no fences, no workgroup waits for another: the result depends on
// the arguments only, not on the grid.
#include "ocm_internal.h"

#include <algorithm>
#include <type_traits>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int CW = 4;      // waves per workgroup
constexpr int CR = 16;     // rows per tile
constexpr int CB = 64;     // columns per wave block (the f32 chain length)
constexpr int CHUNK = 256; // rows per chunk of partial sums
constexpr int LDS_BYTES = 160 * 1024;
constexpr double DEGEN = 1e-8;  // 1 − h at or below this: the variable is left out

template <typename T>
struct Mf;
template <>
struct Mf<float> {
  using acc = f32x4;
  using vec4 = f32x4;
  static constexpr int WPS = 2;  // workgroups per CU (waves per SIMD)
  static __device__ __forceinline__ acc mfma(float a, float b, acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int i) { return 4 * q + i; }
};
template <>
struct Mf<double> {
  using acc = f64x4;
  using vec4 = f64x4;
  static constexpr int WPS = 1;
  static __device__ __forceinline__ acc mfma(double a, double b, acc c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int row(int q, int i) { return q + 4 * i; }
};

// static LDS of k_press<T, KT, *> (the rest is the row tile)
constexpr int press_static_lds(int kt, int esz) {
  return CW * kt * 16 * CR * 8 + kt * 16 * CR * esz + CW * 2 * (kt * 16 + 1) * 8 + 64;
}

// w[k·p + j] = 1/(1 − h_j⁽ᵏ⁾)², 0 where 1 − h ≤ DEGEN; ndegen[k] = number of zeros
template <typename T>
__global__ __launch_bounds__(256) void k_press_weights(const double* __restrict__ P, int p, T* __restrict__ w,
                                                       int32_t* __restrict__ ndegen) {
  __shared__ int cnt_s[256];
  const int k = blockIdx.x;
  int cnt = 0;
  for (int j = threadIdx.x; j < p; j += 256) {
    double h = 0.0;
    for (int a = 0; a < k; ++a) {
      const double v = P[(int64_t)a * p + j];
      h += v * v;
    }
    const double d = 1.0 - h;
    const bool bad = !(d > DEGEN);
    w[(int64_t)k * p + j] = bad ? T(0) : (T)(1.0 / (d * d));
    cnt += bad ? 1 : 0;
  }
  cnt_s[threadIdx.x] = cnt;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) cnt_s[threadIdx.x] += cnt_s[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0 && ndegen) ndegen[k] = cnt_s[0];
}

// KT: component tiles of 16 (K ≤ 16·KT).  VEC: 16-B loads of X, μ, P and w rows
// (p % 4 == 0, ldx % 4 == 0, 16-B aligned bases).  ps: LDS row stride of the
// tile in elements (0: no tile, sweep 2 reads X again).
template <typename T, int KT, bool VEC>
__global__ __launch_bounds__(64 * CW, Mf<T>::WPS) void k_press(const T* __restrict__ X, int64_t ldx,
                                                               const int64_t* __restrict__ rows, int64_t m, int p,
                                                               const T* __restrict__ P, const T* __restrict__ mu,
                                                               const T* __restrict__ W, int K,
                                                               double* __restrict__ part, int64_t nchunks, int ps) {
  using M = Mf<T>;
  using acc_t = typename M::acc;
  using vec4 = typename M::vec4;
  constexpr int KP = KT * 16;
  constexpr int NO = 2 * (KP + 1);  // sums per tile: press then naive, k = 0..KP
  extern __shared__ __attribute__((aligned(32))) unsigned char dyn_lds[];
  T* yt = reinterpret_cast<T*>(dyn_lds);  // [CR][ps]
  __shared__ double tred[CW][KP][CR];      // partial t per wave
  __shared__ __attribute__((aligned(32))) T tT[KP][CR];  // t in the element type, [comp][row]
  __shared__ double wred[CW][NO];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int no = 2 * (K + 1);
  // a lane keeps its sums over up to LANE_TILES tiles of a chunk before they are
  // reduced, as long as that is at most 128 block sums in the element type
  // (float32: a rounding error of 128·2⁻²⁴ at the very worst); where the
  // accumulators would not fit beside sweep 1's (K > 32) every tile flushes
  constexpr int LANE_TILES = (sizeof(T) == 4 && KT <= 2) ? CHUNK / CR : 1;
  const int nblk = (p + CW * CB - 1) / (CW * CB);
  const int flush = LANE_TILES == 1 ? 1 : (128 / nblk < 1 ? 1 : (128 / nblk > LANE_TILES ? LANE_TILES : 128 / nblk));

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

  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    double csum = 0.0;  // thread tid < no: the chunk's sum of output tid
    T pacc[KP + 1], nacc[KP + 1];  // this lane's Σ w·r² and Σ r² since the last flush
    int since = 0;                 // tiles since the last flush
    const int64_t tile0 = chunk * (CHUNK / CR);
    const int64_t ntiles = (m + CR - 1) / CR;
    const int64_t tile1 = tile0 + CHUNK / CR < ntiles ? tile0 + CHUNK / CR : ntiles;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
      const int64_t row0 = tile * CR;
      __syncthreads();  // the previous tile's tT / wred are consumed
      // ---- sweep 1: lane (row j, quarter q) -----------------------------------
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
      for (int b0 = wave * CB; b0 < p; b0 += CW * CB) {
#pragma unroll
        for (int cb = 0; cb < CB / 16; ++cb) {
          const int c0 = b0 + 16 * cb;
          if (c0 >= p) break;
          const int col = c0 + 4 * q;  // loads past p are clamped, their values masked
          const vec4 xv = ld4(xrow, col);
          const vec4 uv = ld4(mu, col);
          vec4 y;
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = aok && col + e < p ? xv[e] - uv[e] : T(0);
          if (ps) *reinterpret_cast<vec4*>(&yt[j * ps + col]) = y;
#pragma unroll
          for (int t = 0; t < KT; ++t) {
            const int comp = 16 * t + j;
            vec4 wv = ld4(P + (int64_t)min(comp, K - 1) * p, col);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (comp >= K || col + e >= p) wv[e] = T(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t] = M::mfma(wv[e], y[e], acc[t]);
          }
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
        const double* s = &tred[0][0][0] + e;
        (&tT[0][0])[e] = (T)(((s[0] + s[KP * CR]) + s[2 * KP * CR]) + s[3 * KP * CR]);
      }
      __syncthreads();

      // ---- sweep 2: lane (columns 4j..4j+3 of the block, rows 4q..4q+3) --------
      if (LANE_TILES == 1 || since == 0) {
#pragma unroll
        for (int k = 0; k <= KP; ++k) {
          pacc[k] = T(0);
          nacc[k] = T(0);
        }
      }
      const T* xr[4];
      bool rok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t g = row0 + 4 * q + i;
        const int64_t gc = g < m ? g : m - 1;
        xr[i] = X + (rows ? rows[gc] : gc) * ldx;
        rok[i] = g < m;
      }
      // one 64-column block; TAIL: the block may reach past p (only a row's last block can)
      auto block = [&](auto tail_c, int b0) {
        constexpr bool TAIL = decltype(tail_c)::value;
        const int col4 = b0 + 4 * j;
        vec4 r[4];  // [row i][column e]
        if (ps) {
#pragma unroll
          for (int i = 0; i < 4; ++i)  // this wave wrote it in sweep 1 (columns past p: never written)
            r[i] = *reinterpret_cast<const vec4*>(&yt[(4 * q + i) * ps + col4]);
        } else {
          const vec4 uv = ld4(mu, col4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const vec4 xv = ld4(xr[i], col4);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[i][e] = rok[i] ? xv[e] - uv[e] : T(0);
          }
        }
        if constexpr (TAIL) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col4 + e >= p) r[i][e] = T(0);
        }
#pragma unroll
        for (int k = 0; k <= KP; ++k) {
          if (k > K) continue;  // uniform
          if (k > 0) {
            vec4 pk = ld4(P + (int64_t)(k - 1) * p, col4);
            if constexpr (TAIL) {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (col4 + e >= p) pk[e] = T(0);
            }
            const vec4 tk = *reinterpret_cast<const vec4*>(&tT[k - 1][4 * q]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int e = 0; e < 4; ++e) r[i][e] -= tk[i] * pk[e];
          }
          const vec4 wk = ld4(W + (int64_t)k * p, col4);  // finite past p, where r = 0
          // the lane's four rows of each column first, then the columns: Σ r² and Σ w·r²
          vec4 c2;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            c2[e] = (r[0][e] * r[0][e] + r[1][e] * r[1][e]) + (r[2][e] * r[2][e] + r[3][e] * r[3][e]);
          nacc[k] += (c2[0] + c2[1]) + (c2[2] + c2[3]);
          pacc[k] += (wk[0] * c2[0] + wk[1] * c2[1]) + (wk[2] * c2[2] + wk[3] * c2[3]);
        }
      };
      for (int b0 = wave * CB; b0 < p; b0 += CW * CB) {
        if (b0 + CB <= p)
          block(std::false_type{}, b0);
        else
          block(std::true_type{}, b0);
      }
      // flush: lanes → wave (fp64), waves → workgroup (fixed order), flushes in tile order
      if (++since < flush && tile + 1 < tile1) continue;  // uniform
      since = 0;
#pragma unroll
      for (int k = 0; k <= KP; ++k) {
        if (k > K) continue;
        const double a = wave_sum_f64((double)pacc[k]);
        const double b = wave_sum_f64((double)nacc[k]);
        if (lane == 0) {
          wred[wave][k] = a;
          wred[wave][K + 1 + k] = b;
        }
      }
      __syncthreads();
      if (tid < no) csum += ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    }
    if (tid < no) part[chunk * no + tid] = csum;
  }
}

// out[o] = Σ_chunks part[c·no + o] in chunk order: thread t adds the consecutive
// chunks [t·L, (t + 1)·L), thread 0 the 256 subtotals in order
__global__ __launch_bounds__(256) void k_press_reduce(const double* __restrict__ part, int64_t nchunks, int K,
                                                      double* __restrict__ press_out,
                                                      double* __restrict__ naive_out) {
  __shared__ double sub[256];
  const int o = blockIdx.x, no = 2 * (K + 1);
  const int64_t L = (nchunks + 255) / 256;
  const int64_t c0 = (int64_t)threadIdx.x * L, c1 = c0 + L < nchunks ? c0 + L : nchunks;
  double v = 0.0;
  for (int64_t c = c0; c < c1; ++c) v += part[c * no + o];
  sub[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int t = 0; t < 256; ++t) s += sub[t];
    if (o <= K)
      press_out[o] = s;
    else if (naive_out)
      naive_out[o - (K + 1)] = s;
  }
}

template <typename T>
int press_impl(const char* who, ocm_ctx* ctx, const T* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
               const double* P, const double* mu, int32_t K, double* press_out, double* naive_out,
               int32_t* ndegen_out, hipStream_t st) {
  using M = Mf<T>;
  constexpr bool F32 = sizeof(T) == 4;
  const std::string w(who);
  OCM_REQUIRE(ctx && P && mu && press_out, w + ": NULL argument");
  OCM_REQUIRE(m >= 0 && p >= 2, w + ": m >= 0 and p >= 2");
  OCM_REQUIRE(X || m == 0, w + ": NULL argument");
  OCM_REQUIRE(ldx >= p, w + ": ldx >= p");
  OCM_REQUIRE(K >= 1 && K <= 64 && K <= p, w + ": 1 <= K <= min(p, 64) (got K = " + std::to_string(K) + ")");
  const int64_t nchunks = (m + CHUNK - 1) / CHUNK;
  OCM_REQUIRE(nchunks < (1LL << 31), w + ": too many rows");
  const int no = 2 * (K + 1);
  // workspace: the weight table, the element-type copies of P and μ, one slot per chunk
  const size_t cast_n = F32 ? (size_t)K * p + (size_t)p : 0;
  void* ws = ocm::workspace(ctx, (size_t)(K + 1) * p * sizeof(T) + cast_n * sizeof(float) +
                                     (size_t)nchunks * no * sizeof(double) + 2048, st);
  if (!ws) return OCM_ERR_NOMEM;
  ocm::Carve cv{static_cast<char*>(ws)};
  T* W = cv.take<T>((size_t)(K + 1) * p);
  double* part = cv.take<double>((size_t)nchunks * no);
  hipLaunchKernelGGL(k_press_weights<T>, dim3(K + 1), dim3(256), 0, st, P, p, W, ndegen_out);
  OCM_CHECK_LAUNCH("k_press_weights");
  if (m == 0) {
    OCM_HIP(hipMemsetAsync(press_out, 0, (size_t)(K + 1) * sizeof(double), st));
    if (naive_out) OCM_HIP(hipMemsetAsync(naive_out, 0, (size_t)(K + 1) * sizeof(double), st));
    return OCM_OK;
  }
  const T* Pk;
  const T* muk;
  if constexpr (F32) {  // the f32 kernel takes f32 loadings / mean, as the scoring kernels do
    float* P32 = cv.take<float>((size_t)K * p);
    float* mu32 = cv.take<float>(p);
    if (int rc = ocm_cast_f64_f32(ctx, P, (int64_t)K * p, P32, st)) return rc;
    if (int rc = ocm_cast_f64_f32(ctx, mu, (int64_t)p, mu32, st)) return rc;
    Pk = P32;
    muk = mu32;
  } else {
    Pk = P;
    muk = mu;
  }
  const int kt = (K + 15) / 16;
  const int grid = (int)std::min<int64_t>((int64_t)M::WPS * ctx->num_cus, nchunks);
  // the row tile in LDS when it leaves room for every workgroup a CU runs at once
  int ps = (p + CB - 1) / CB * CB + 4;
  if ((size_t)CR * ps * sizeof(T) + press_static_lds(kt, (int)sizeof(T)) > (size_t)LDS_BYTES / M::WPS) ps = 0;
  const size_t dyn = (size_t)CR * ps * sizeof(T);
  const bool vec = F32 && (ldx % 4 == 0) && (p % 4 == 0) && ((reinterpret_cast<uintptr_t>(X) & 15) == 0);
#define OCM_PRESS_LAUNCH(KT_, V_)                                                                                 \
  do {                                                                                                            \
    auto kern = k_press<T, KT_, V_>;                                                                              \
    static int lds_ok[64] = {0}; /* per device: the attribute is set once per kernel, for the whole LDS */        \
    if (dyn > 48 * 1024 && !lds_ok[ctx->device & 63]) {                                                           \
      OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  LDS_BYTES - press_static_lds(KT_, (int)sizeof(T))));                            \
      lds_ok[ctx->device & 63] = 1;                                                                               \
    }                                                                                                             \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * CW), dyn, st, X, ldx, rows, m, p, Pk, muk, W, K, part,         \
                       nchunks, ps);                                                                              \
  } while (0)
#define OCM_PRESS_KT(KT_)         \
  if (vec)                        \
    OCM_PRESS_LAUNCH(KT_, true);  \
  else                            \
    OCM_PRESS_LAUNCH(KT_, false)
  if (kt == 1) {
    OCM_PRESS_KT(1);
  } else if (kt == 2) {
    OCM_PRESS_KT(2);
  } else if (kt == 3) {
    OCM_PRESS_KT(3);
  } else {
    OCM_PRESS_KT(4);
  }
#undef OCM_PRESS_KT
#undef OCM_PRESS_LAUNCH
  OCM_CHECK_LAUNCH("k_press");
  hipLaunchKernelGGL(k_press_reduce, dim3(no), dim3(256), 0, st, part, nchunks, K, press_out, naive_out);
  OCM_CHECK_LAUNCH("k_press_reduce");
  return OCM_OK;
}

}  // namespace

extern "C" {

int ocm_press_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                  const double* P, const double* mu, int32_t K, double* press_out, double* naive_out,
                  int32_t* ndegen_out, void* stream) {
  return press_impl<float>("ocm_press_f32", ctx, X, ldx, rows, m, p, P, mu, K, press_out, naive_out, ndegen_out,
                           (hipStream_t)stream);
}

int ocm_press_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                  const double* P, const double* mu, int32_t K, double* press_out, double* naive_out,
                  int32_t* ndegen_out, void* stream) {
  return press_impl<double>("ocm_press_f64", ctx, X, ldx, rows, m, p, P, mu, K, press_out, naive_out, ndegen_out,
                            (hipStream_t)stream);
}

}  // extern "C"
