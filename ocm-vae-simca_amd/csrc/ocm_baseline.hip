// Whittaker smoothing and asymmetric-least-squares (AsLS) baselines along the
// wavelength axis (include/ocm.h, "baseline correction"):
//   (diag(w) + λ·DᵀD) z = w ∘ x      D the d-th difference matrix, d ∈ {1, 2}
// a symmetric positive definite system of half bandwidth d per row, solved by
// the LDLᵀ elimination without pivoting, all of it in fp64.
//
// Mapping: one lane owns one row and walks it; a 64-row wave is a workgroup.
//   forward   eliminate column by column, carrying the last two pivots'
//             multipliers and right-hand sides in registers; store per column
//             the multipliers l1_j, l2_j and the scaled right-hand side u_j
//   backward  z_j = u_j − l1_j·z_{j+1} − l2_j·z_{j+2}
// X, W and out are row-major, so a lane per row reads at stride ldx: they go
// through LDS as 64-row × 32-column tiles (loaded / stored along the
// wavelengths, 128 bytes per row piece; the image's rows are 33 words apart, so
// the 64 lanes reading one column hit 64 different banks).  The next tile is
// fetched into registers while the lanes work on the current one.  The
// per-column factors live in a scratch slab of the workgroup, laid out
// [column][lane]: every step is one 512-byte access per wave.
//
// Shared weights (w = 1, or one (p) vector for all rows; AsLS's first solve):
// k_baseline_factor factorises once (one lane), the forward sweep stores u
// only and both sweeps read the multipliers at wave-uniform addresses.
//
// AsLS: a workgroup runs all iterations of its 64 rows before it takes the
// next 64.  The weights are one bit per element (x_j > z_j), kept in the slab
// as [32-column word][lane].  A row whose update changes no bit is finished;
// its lane keeps solving with the same weights (the same bits come out) until
// the whole wave is finished, then one more solve writes the result: only the
// last solve of a wave writes `out`.
//
// Every row is computed by one lane in one order, whatever m, the row's
// position, ldx or ldo: results are bitwise reproducible.  The only atomic is
// the count of failed rows.
#include "ocm_internal.h"

namespace {

constexpr int BL_ROWS = 64;            // rows per workgroup: one wave, a lane per row
constexpr int BL_TC = 32;              // columns per LDS tile = bits per weight word
constexpr int BL_PITCH = BL_TC + 1;    // words between the rows of the LDS image
constexpr int BL_PER_CU = 8;           // workgroups (waves) per CU the grid is sized for
constexpr int BL_MODE_SHARED = 0, BL_MODE_ROWS = 1, BL_MODE_ASLS = 2;

// entries of λ·DᵀD in column j: diagonal, first and second sub-diagonal
template <int D>
__device__ __forceinline__ void band(int j, int p, double lam, double& g0, double& g1, double& g2) {
  if constexpr (D == 2) {
    const int a = j <= p - 3, b = j >= 1 && j <= p - 2, c = j >= 2;
    g0 = lam * (double)(a + 4 * b + c);
    g1 = lam * (double)(-2 * (a + b));
    g2 = lam * (double)a;
  } else {
    g0 = lam * (double)((j >= 1) + (j <= p - 2));
    g1 = j <= p - 2 ? -lam : 0.0;
    g2 = 0.0;
  }
}

// The elimination of one row, column by column.  With n_j = A_{j+1,j} −
// A_{j+1,j−1}·l1_{j−1} (= l1_j·d_j) and A_{j+2,j} = l2_j·d_j:
//   d_j = A_jj − l1_{j−1}·n_{j−1} − l2_{j−2}·A_{j,j−2}
struct Elim {
  double l1p = 0.0, l2p = 0.0, l2pp = 0.0;  // l1_{j−1}, l2_{j−1}, l2_{j−2}
  double n1p = 0.0, g2p = 0.0, g2pp = 0.0;  // n_{j−1}, A_{j+1,j−1}, A_{j,j−2}
  double y1 = 0.0, y2 = 0.0;                // unscaled right-hand sides of columns j − 1, j − 2
  bool bad = false;

  // the factor's step: pivot → (l1_j, l2_j, 1/d_j)
  template <int D>
  __device__ __forceinline__ void pivot(int j, int p, double lam, double w, double& l1, double& l2, double& inv) {
    double g0, g1, g2;
    band<D>(j, p, lam, g0, g1, g2);
    const double dj = (g0 + w) - l1p * n1p - l2pp * g2pp;
    if (!(dj > 0.0 && dj < __builtin_huge_val())) bad = true;
    inv = 1.0 / dj;
    const double n1 = g1 - g2p * l1p;
    l1 = j < p - 1 ? n1 * inv : 0.0;
    l2 = g2 * inv;
    n1p = n1;
    g2pp = g2p;
    g2p = g2;
  }
  // the right-hand side's step under multipliers (l1, l2, inv) of column j: → u_j
  __device__ __forceinline__ double rhs(double r, double l1, double l2, double inv) {
    const double y = r - l1p * y1 - l2pp * y2;
    y2 = y1;
    y1 = y;
    l2pp = l2p;
    l2p = l2;
    l1p = l1;
    return y * inv;
  }
};

// The shared factor: F = l1 [p] ++ l2 [p] ++ 1/d [p] ++ {1.0 if a pivot failed or a weight is bad, else 0.0}.
template <int D>
__global__ __launch_bounds__(64) void k_baseline_factor(const float* __restrict__ wv, int p, double lam,
                                                        double* __restrict__ F) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Elim e;
  int npos = 0;
  for (int j = 0; j < p; ++j) {
    const double w = wv ? (double)wv[j] : 1.0;
    if (!(w >= 0.0)) e.bad = true;
    npos += w > 0.0;
    double l1, l2, inv;
    e.pivot<D>(j, p, lam, w, l1, l2, inv);
    e.rhs(0.0, l1, l2, inv);
    F[j] = l1;
    F[p + j] = l2;
    F[2 * (size_t)p + j] = inv;
  }
  F[3 * (size_t)p] = (e.bad || npos < D) ? 1.0 : 0.0;
}

struct BlArgs {
  const float* X;
  int64_t ldx, m;
  int p;
  const float* W;  // BL_MODE_ROWS: (m, p) weights; BL_MODE_SHARED: the (p) vector or NULL
  int64_t ldw;
  const double* F;  // the shared factor (BL_MODE_SHARED, BL_MODE_ASLS)
  double lam, asym;
  int n_iter, mode, subtract;
  float* out;
  int64_t ldo;
  int* iters_out;
  int* nbad_out;
  char* slabs;
  size_t slab_bytes;
};

// a workgroup's scratch: u, l1, l2 as [column][lane] doubles, the weight bits as [word][lane]
struct Slab {
  double *u, *l1, *l2;
  uint32_t* bits;
};

// A 64 × 32 tile between the matrix and its LDS image.  M points at the tile's first element, nr × nc
// (≥ 1 × 1) of the tile lie inside the matrix.  Thread t moves tile rows 2i + t / 32, column t % 32: a
// wave-instruction moves two 128-byte row pieces.  A full block of rows (nr = 64) is fetched into
// registers ahead of its use, at wave-uniform row offsets; columns past nc repeat column nc − 1 (they
// are not walked).  The last, partial block of rows takes a plain guarded loop at the time of use; its
// rows past nr hold 0 (their lanes solve a zero row and write nothing).
__device__ __forceinline__ void tile_fetch(const float* __restrict__ M, int64_t ld, int nr, int nc,
                                           float (&v)[BL_TC]) {
  if (nr < BL_ROWS) return;
  const float* q = M + (int64_t)(threadIdx.x >> 5) * ld + min((int)threadIdx.x & 31, nc - 1);
#pragma unroll
  for (int i = 0; i < BL_TC; ++i) v[i] = q[2 * i * ld];
}
__device__ __forceinline__ void tile_put(float* s, const float* __restrict__ M, int64_t ld, int nr, int nc,
                                         const float (&v)[BL_TC]) {
  const int c = threadIdx.x & 31, rr = threadIdx.x >> 5;
  if (nr == BL_ROWS) {
#pragma unroll
    for (int i = 0; i < BL_TC; ++i) s[(2 * i + rr) * BL_PITCH + c] = v[i];
  } else {
#pragma unroll 1
    for (int r = rr; r < BL_ROWS; r += 2) s[r * BL_PITCH + c] = (r < nr && c < nc) ? M[r * ld + c] : 0.f;
  }
}
__device__ __forceinline__ void tile_write(float* __restrict__ M, int64_t ld, int nr, int nc, const float* s) {
  const int c = threadIdx.x & 31, rr = threadIdx.x >> 5;
  if (c >= nc) return;
  if (nr == BL_ROWS) {
    float* q = M + (int64_t)rr * ld + c;
#pragma unroll
    for (int i = 0; i < BL_TC; ++i) q[2 * i * ld] = s[(2 * i + rr) * BL_PITCH + c];
  } else {
#pragma unroll 1
    for (int r = rr; r < nr; r += 2) M[r * ld + c] = s[r * BL_PITCH + c];
  }
}

// SRC 0: the shared factor (weights a.W as a (p) vector, or 1); 1: the rows of a.W; 2: the weight bits
template <int D, int SRC>
__device__ __forceinline__ void sweep_forward(const BlArgs& a, const Slab& sl, int64_t row0, bool& bad, float* sX,
                                              float* sW) {
  const int lane = threadIdx.x, p = a.p;
  const int nt = (p + BL_TC - 1) / BL_TC;
  Elim e;
  int npos = 0;
  const int nr = (int)(a.m - row0 < BL_ROWS ? a.m - row0 : BL_ROWS);
  const float* Xb = a.X + row0 * a.ldx;
  const float* Wb = SRC == 1 ? a.W + row0 * a.ldw : nullptr;
  float pre[BL_TC], prew[BL_TC];
  tile_fetch(Xb, a.ldx, nr, p, pre);
  if constexpr (SRC == 1) tile_fetch(Wb, a.ldw, nr, p, prew);
  for (int t = 0; t < nt; ++t) {
    const int j0 = t * BL_TC, jn = min(BL_TC, p - j0);
    __syncthreads();  // the lanes have read the previous tile
    tile_put(sX, Xb + j0, a.ldx, nr, jn, pre);
    if constexpr (SRC == 1) tile_put(sW, Wb + j0, a.ldw, nr, jn, prew);
    __syncthreads();
    if (t + 1 < nt) {
      tile_fetch(Xb + j0 + BL_TC, a.ldx, nr, p - j0 - BL_TC, pre);
      if constexpr (SRC == 1) tile_fetch(Wb + j0 + BL_TC, a.ldw, nr, p - j0 - BL_TC, prew);
    }
    uint32_t word = 0;
    if constexpr (SRC == 2) word = sl.bits[(size_t)t * BL_ROWS + lane];
#pragma unroll 4
    for (int c = 0; c < jn; ++c) {
      const int j = j0 + c;
      const size_t at = (size_t)j * BL_ROWS + lane;
      const double x = (double)sX[lane * BL_PITCH + c];
      if constexpr (SRC == 0) {
        const double w = a.W ? (double)a.W[j] : 1.0;
        sl.u[at] = e.rhs(w * x, a.F[j], a.F[p + j], a.F[2 * (size_t)p + j]);
      } else {
        double w;
        if constexpr (SRC == 1) {
          w = (double)sW[lane * BL_PITCH + c];
          if (!(w >= 0.0)) e.bad = true;
          npos += w > 0.0;
        } else {
          w = (word >> c) & 1u ? a.asym : 1.0 - a.asym;
        }
        double l1, l2, inv;
        e.pivot<D>(j, p, a.lam, w, l1, l2, inv);
        sl.u[at] = e.rhs(w * x, l1, l2, inv);
        sl.l1[at] = l1;
        if constexpr (D == 2) sl.l2[at] = l2;
      }
    }
  }
  if (e.bad || (SRC == 1 && npos < D)) bad = true;
}

// The substitution, last column first.  ASLS: also the new weight bits (x_j > z_j; returns whether one
// differs from the stored word, `first`: there is none yet) and x − z.  `write`: the result goes to a.out
// through the tile sO; rows marked bad are written as NaN.
template <int D, bool SHARED, bool ASLS>
__device__ __forceinline__ bool sweep_backward(const BlArgs& a, const Slab& sl, int64_t row0, bool write, bool first,
                                               bool bad, float* sX, float* sO) {
  const int lane = threadIdx.x, p = a.p;
  const int nt = (p + BL_TC - 1) / BL_TC;
  double z1 = 0.0, z2 = 0.0;
  bool changed = first;
  const int nr = (int)(a.m - row0 < BL_ROWS ? a.m - row0 : BL_ROWS);
  const float* Xb = a.X + row0 * a.ldx;
  float pre[BL_TC];
  if constexpr (ASLS) tile_fetch(Xb + (nt - 1) * BL_TC, a.ldx, nr, p - (nt - 1) * BL_TC, pre);
  for (int t = nt - 1; t >= 0; --t) {
    const int j0 = t * BL_TC, jn = min(BL_TC, p - j0);
    uint32_t oldw = 0, neww = 0;
    if constexpr (ASLS) {
      __syncthreads();  // the lanes have read the previous tile
      tile_put(sX, Xb + j0, a.ldx, nr, jn, pre);
      __syncthreads();
      if (t > 0) tile_fetch(Xb + j0 - BL_TC, a.ldx, nr, BL_TC, pre);
      if (!first) oldw = sl.bits[(size_t)t * BL_ROWS + lane];
    }
#pragma unroll 4
    for (int c = jn - 1; c >= 0; --c) {
      const int j = j0 + c;
      const size_t at = (size_t)j * BL_ROWS + lane;
      const double l1 = SHARED ? a.F[j] : sl.l1[at];
      double z = sl.u[at] - l1 * z1;
      if constexpr (D == 2) z -= (SHARED ? a.F[p + j] : sl.l2[at]) * z2;
      z2 = z1;
      z1 = z;
      double val = z;
      if constexpr (ASLS) {
        const double x = (double)sX[lane * BL_PITCH + c];
        neww |= (uint32_t)(x > z) << c;
        if (a.subtract) val = x - z;
      }
      if (write) sO[lane * BL_PITCH + c] = bad ? __builtin_nanf("") : (float)val;
    }
    if constexpr (ASLS) {
      changed = changed || neww != oldw;
      sl.bits[(size_t)t * BL_ROWS + lane] = neww;
    }
    if (write) {
      __syncthreads();
      tile_write(a.out + row0 * a.ldo + j0, a.ldo, nr, jn, sO);
      __syncthreads();  // before the lanes fill sO again
    }
  }
  return changed;
}

template <int D, int MODE>
__global__ __launch_bounds__(BL_ROWS) void k_baseline(const BlArgs a) {
  __shared__ float sX[BL_ROWS * BL_PITCH];
  __shared__ float sW[BL_ROWS * BL_PITCH];  // the weights' tile going forward, the result's going backward
  const int lane = threadIdx.x;
  const size_t cols = (size_t)a.p * BL_ROWS;
  char* base = a.slabs + (size_t)blockIdx.x * a.slab_bytes;
  Slab sl;
  sl.u = reinterpret_cast<double*>(base);
  sl.l1 = sl.u + cols;
  sl.l2 = sl.l1 + cols;
  sl.bits = reinterpret_cast<uint32_t*>(sl.u + (MODE == BL_MODE_ASLS ? (D + 1) * cols : 0));
  const bool fbad = MODE != BL_MODE_ROWS && a.F[3 * (size_t)a.p] != 0.0;
  const int64_t nblk = (a.m + BL_ROWS - 1) / BL_ROWS;
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t row0 = blk * BL_ROWS, row = row0 + lane;
    bool bad = fbad;
    if constexpr (MODE == BL_MODE_SHARED) {
      sweep_forward<D, 0>(a, sl, row0, bad, sX, sW);
      sweep_backward<D, true, false>(a, sl, row0, true, true, bad, sX, sW);
    } else if constexpr (MODE == BL_MODE_ROWS) {
      sweep_forward<D, 1>(a, sl, row0, bad, sX, sW);
      sweep_backward<D, false, false>(a, sl, row0, true, true, bad, sX, sW);
    } else {
      int iters = 0;
      bool done = false, all_done = false;
      for (int it = 1; it <= a.n_iter; ++it) {
        const bool last = it == a.n_iter || all_done;
        bool changed;
        if (it == 1) {
          sweep_forward<D, 0>(a, sl, row0, bad, sX, sW);
          changed = sweep_backward<D, true, true>(a, sl, row0, last, true, bad, sX, sW);
        } else {
          sweep_forward<D, 2>(a, sl, row0, bad, sX, sW);
          changed = sweep_backward<D, false, true>(a, sl, row0, last, false, bad, sX, sW);
        }
        if (!done) {
          iters = it;
          done = !changed;
        }
        if (last) break;
        all_done = __all(done);
      }
      if (a.iters_out && row < a.m) a.iters_out[row] = iters;
    }
    if (a.nbad_out && bad && row < a.m) atomicAdd(a.nbad_out, 1);
  }
}

int run_baseline(ocm_ctx* ctx, BlArgs a, int d, hipStream_t st) {
  const int64_t nblk = (a.m + BL_ROWS - 1) / BL_ROWS;
  const int64_t grid = nblk < (int64_t)ctx->num_cus * BL_PER_CU ? nblk : (int64_t)ctx->num_cus * BL_PER_CU;
  const size_t cols = (size_t)a.p * BL_ROWS;
  const size_t words = (size_t)(a.p + BL_TC - 1) / BL_TC * BL_ROWS;
  // u alone under a shared factor; u, l1 (, l2) per row; AsLS adds the weight bits
  const size_t ndbl = a.mode == BL_MODE_SHARED ? 1 : d + 1;
  a.slab_bytes = ocm::align_up(ndbl * cols * sizeof(double) + (a.mode == BL_MODE_ASLS ? words * 4 : 0), 256);
  const size_t fbytes = ocm::align_up((3 * (size_t)a.p + 1) * sizeof(double), 256);
  char* ws = static_cast<char*>(ocm::workspace(ctx, fbytes + (size_t)grid * a.slab_bytes, st));
  if (!ws) return OCM_ERR_NOMEM;
  a.F = reinterpret_cast<double*>(ws);
  a.slabs = ws + fbytes;
  if (a.mode != BL_MODE_ROWS) {
    const float* wv = a.mode == BL_MODE_SHARED ? a.W : nullptr;
    double* F = reinterpret_cast<double*>(ws);
    if (d == 2)
      hipLaunchKernelGGL(k_baseline_factor<2>, dim3(1), dim3(64), 0, st, wv, a.p, a.lam, F);
    else
      hipLaunchKernelGGL(k_baseline_factor<1>, dim3(1), dim3(64), 0, st, wv, a.p, a.lam, F);
    OCM_CHECK_LAUNCH("k_baseline_factor");
  }
#define OCM_BL(D_, M_) hipLaunchKernelGGL((k_baseline<D_, M_>), dim3((unsigned)grid), dim3(BL_ROWS), 0, st, a)
#define OCM_BL_D(M_) \
  if (d == 2)        \
    OCM_BL(2, M_);   \
  else               \
    OCM_BL(1, M_);
  if (a.mode == BL_MODE_SHARED) {
    OCM_BL_D(BL_MODE_SHARED)
  } else if (a.mode == BL_MODE_ROWS) {
    OCM_BL_D(BL_MODE_ROWS)
  } else {
    OCM_BL_D(BL_MODE_ASLS)
  }
#undef OCM_BL_D
#undef OCM_BL
  OCM_CHECK_LAUNCH("k_baseline");
  return OCM_OK;
}

inline bool finite_pos(double v) { return v > 0.0 && v < __builtin_huge_val(); }

}  // namespace

extern "C" {

int ocm_whittaker_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const float* W, int64_t ldw,
                      double lam, int32_t d, float* out, int64_t ldo, int32_t* nbad_out, void* stream) {
  OCM_REQUIRE(ctx && X && out, "ocm_whittaker_f32: NULL argument");
  OCM_REQUIRE(d == 1 || d == 2, "ocm_whittaker_f32: d must be 1 or 2");
  OCM_REQUIRE(finite_pos(lam), "ocm_whittaker_f32: lam must be positive and finite");
  OCM_REQUIRE(m >= 0 && p >= d + 1 && ldx >= p && ldo >= p, "ocm_whittaker_f32: bad shape (p >= d + 1, ldx, ldo >= p)");
  OCM_REQUIRE(!W || ldw == 0 || ldw >= p, "ocm_whittaker_f32: ldw must be 0 (one vector for all rows) or >= p");
  OCM_REQUIRE(m < (1LL << 31), "ocm_whittaker_f32: too many rows per call");
  if (nbad_out) OCM_HIP(hipMemsetAsync(nbad_out, 0, sizeof(int32_t), (hipStream_t)stream));
  if (m == 0) return OCM_OK;
  BlArgs a{};
  a.X = X, a.ldx = ldx, a.m = m, a.p = p, a.W = W, a.ldw = ldw, a.lam = lam, a.asym = 0.0, a.n_iter = 1;
  a.mode = (W && ldw > 0) ? BL_MODE_ROWS : BL_MODE_SHARED;
  a.subtract = 0, a.out = out, a.ldo = ldo, a.iters_out = nullptr, a.nbad_out = nbad_out;
  return run_baseline(ctx, a, d, (hipStream_t)stream);
}

int ocm_asls_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, double lam, double asym, int32_t d,
                 int32_t n_iter, int32_t subtract, float* out, int64_t ldo, int32_t* iters_out, void* stream) {
  OCM_REQUIRE(ctx && X && out, "ocm_asls_f32: NULL argument");
  OCM_REQUIRE(d == 1 || d == 2, "ocm_asls_f32: d must be 1 or 2");
  OCM_REQUIRE(finite_pos(lam), "ocm_asls_f32: lam must be positive and finite");
  OCM_REQUIRE(asym > 0.0 && asym < 1.0, "ocm_asls_f32: asym must lie in (0, 1)");
  OCM_REQUIRE(n_iter >= 1, "ocm_asls_f32: n_iter must be >= 1");
  OCM_REQUIRE(m >= 0 && p >= d + 1 && ldx >= p && ldo >= p, "ocm_asls_f32: bad shape (p >= d + 1, ldx, ldo >= p)");
  OCM_REQUIRE(m < (1LL << 31), "ocm_asls_f32: too many rows per call");
  if (m == 0) return OCM_OK;
  BlArgs a{};
  a.X = X, a.ldx = ldx, a.m = m, a.p = p, a.W = nullptr, a.ldw = 0, a.lam = lam, a.asym = asym, a.n_iter = n_iter;
  a.mode = BL_MODE_ASLS, a.subtract = subtract != 0, a.out = out, a.ldo = ldo, a.iters_out = iters_out;
  a.nbad_out = nullptr;
  return run_baseline(ctx, a, d, (hipStream_t)stream);
}

}  // extern "C"
