/*
 * ocm.h — C ABI of libocm.so, the MI355X (gfx950) SIMCA / VAE-SIMCA engine.
 *
 * The reference (TEAM-AIOLY/OCM-VAE-SIMCA) is pure Python and has no native
 * boundary; the boundary its drivers use is the estimator API of
 * utils/SIMCA.py and utils/CVSIMCA.py.  This header is the
 * native layer UNDER that API: every entry point replaces one piece of
 * arithmetic the reference runs through NumPy/SciPy/scikit-learn, cited
 * per function.  The Python mirror (ocm-vae-simca_amd/utils/SIMCA.py,
 * .../ocm/_lib.py) binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Arrays marked [dev] are device pointers
 *    (HBM, e.g. torch tensor data_ptr()); [host] are host pointers.
 *  - Row-major.  X is n×p float32 with leading dimension ldx (elements).
 *  - `rows` [dev, nullable]: optional int64 row-index list; when non-NULL
 *    the r-th processed row is X[rows[r]] (class subsets / CV test sets
 *    without a gather copy).
 *  - `stream` is a hipStream_t (NULL = default stream).  Every call is
 *    stream-ordered; calls that return host values synchronise that stream.
 *  - Return 0 on success, a negative OCM_ERR_* code on failure;
 *    ocm_last_error() gives the message (thread-local).
 */
#ifndef OCM_H_
#define OCM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCM_ABI_VERSION 12

#define OCM_OK 0
#define OCM_ERR_ARG (-1)         /* invalid argument (maps to ValueError) */
#define OCM_ERR_HIP (-2)         /* HIP runtime error */
#define OCM_ERR_NOMEM (-3)       /* device allocation failed */
#define OCM_ERR_NOCONV (-4)      /* eigensolver hit max_iter (results still written) */
#define OCM_ERR_UNSUPPORTED (-5) /* shape outside the supported envelope */

/* decision types (utils/SIMCA.py:131-144) */
#define OCM_TYPE_SIM 0 /* dred = max(t, q)       */
#define OCM_TYPE_ALT 1 /* dred = sqrt(t² + q²)   */
#define OCM_TYPE_CI 2  /* dred = t + q           */
#define OCM_TYPE_DD 3  /* dred = t + q (dof-scaled t, q) */

typedef struct ocm_ctx ocm_ctx;

/* t = T2 * t2_scale, q = Q * q_scale; accept = dred(t, q) < dlim.
 * Non-dd types: t2_scale = 1/T2_limit, q_scale = 1/Q_limit.
 * dd: t2_scale = t2dof/t2scfact, q_scale = qdof/qscfact (utils/SIMCA.py:76-81,141-144). */
typedef struct ocm_decision {
  int32_t type;
  int32_t pad_;
  double t2_scale;
  double q_scale;
  double dlim;
} ocm_decision;

int ocm_abi_version(void);
/* 16 hex digits: the first 64 bits of the SHA-256 of the library's build
 * inputs (the csrc .hip sources, its headers and Makefile, in the Makefile's
 * ID_INPUTS order).  The Python binding refuses a library whose id differs from the
 * hash of the sources beside it (a stale prebuilt libocm.so). */
const char* ocm_build_id(void);
const char* ocm_last_error(void);
int ocm_ctx_create(int device, ocm_ctx** out);
int ocm_ctx_destroy(ocm_ctx* ctx);
/* Pre-size the context workspace (bytes) so later calls never allocate
 * (lets a caller capture the launch sequence in a hipGraph). */
int ocm_ctx_reserve(ocm_ctx* ctx, size_t bytes);

/* Live kernel timing for benchmarks: while enabled, every launch of a timed
 * kernel is bracketed by a hipEvent pair on its stream (no synchronisation).
 * ocm_ctx_read_timing waits for the recorded events, returns the summed
 * duration (ms) and launch count of kernel `kernel_id`, and clears them. */
#define OCM_TIMED_KERNELS 3
#define OCM_KERNEL_GRAM 0  /* the Gram main kernel (k_gram8e / k_gram8d / k_gram3 / k_gram) */
#define OCM_KERNEL_SCORE 1 /* k_score: fused projection / Q / T² kernel */
#define OCM_KERNEL_QUANT 2 /* k_q8_quant: int8 digit split feeding k_gram8d */
int ocm_ctx_set_timing(ocm_ctx* ctx, int enable);
int ocm_ctx_read_timing(ocm_ctx* ctx, int kernel_id, double* total_ms, int64_t* count);

/* Column mean of the first n processed rows, fp64 accumulation.
 * Replaces sklearn PCA mean_ (sklearn/decomposition/_pca.py:560; called
 * from utils/SIMCA.py:64-66).  Used with n = a small sample as the Gram
 * shift, and as the exact mean when needed.  mean_out [dev] p doubles. */
int ocm_colmean_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                    double* mean_out, void* stream);

/* Per-segment shifted Gram (default mode OCM_GRAM_I8X3): y = x − shift is
 * split into three int8 digits per value (power-of-two scale per 1536-row
 * block and column) and the six digit products of weight ≥ 254⁻² are summed
 * exactly in int32 on integer MFMA (fp32-grade Gram: max relative error
 * ≈ 5e-8 on the bench data).  Outlier guard: values above 16× their column's
 * robust sample scale (2^e ≥ median|y| over the first ≤ 4096 rows) are
 * screened out of the digits of their 32-column group and
 * added back exactly (fp64 fix-up), so one extreme row does not coarsen the
 * other rows of its block; when more than n/8 rows are screened the call
 * recomputes the Gram on the bf16×3 split.  Workspace: ≈ 3 B per value for the digit
 * planes plus the chunk partials (≈ 8.4 GB at 1M × 2048).
 * Replaces the SVD of the centred class matrix (utils/SIMCA.py:64-66 ->
 * sklearn _pca.py:569-584 scipy.linalg.svd gesdd): the covariance
 * eigen-decomposition needs only Σ yᵀy and Σ y with y = x - shift.
 * Segment s covers processed rows [seg_offsets[s], seg_offsets[s+1]).
 * G_out [dev] nseg·p·p doubles (full symmetric), colsum_out [dev] nseg·p.
 * seg_offsets [host] nseg+1 ascending, seg_offsets[0] = 0, last = n.
 * shift [dev] p floats.  p ≤ 64 always takes an fp64-accumulated VALU Gram. */
int ocm_gram_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                 const float* shift, const int64_t* seg_offsets, int32_t nseg, double* G_out, double* colsum_out,
                 void* stream);

/* Same with an explicit arithmetic mode and row-chunk length (0 = automatic):
 *   OCM_GRAM_I8X3   the default above;
 *   OCM_GRAM_F32    FP32 MFMA (v_mfma_f32_32x32x2_f32), f32 chunk partials summed in f64;
 *   OCM_GRAM_BF16X3 exact three-level bf16 split on bf16 MFMA;
 *   OCM_GRAM_I8X3_K32 the i8×3 Gram on v_mfma_i32_32x32x32_i8 (round 2's
 *                   kernel) instead of the default's 16x16x64: bit-identical
 *                   result, kept for kernel A/B.
 * chunk_rows, i8×3 modes (rows are cut into chunks; each chunk's f32 partial
 * Gram is summed with the others in f64, in chunk order):
 *   > 0  uniform chunks of that many rows, rounded up to whole 1536-row scale
 *        blocks;
 *   < 0  −chunk_rows balanced chunks: the B = ⌈n/1536⌉ scale blocks in that
 *        many chunks (at most B) of ⌊B/N⌋ or ⌈B/N⌉ blocks, the longer ones
 *        first.  One segment of contiguous rows only; with several segments
 *        or a row list it is the automatic choice;
 *   = 0  automatic: for one segment of contiguous rows a cost model picks a
 *        balanced count with at most 12 blocks per chunk (csrc/ocm_gram_map.h
 *        plan_chunks), otherwise — and whenever the model finds nothing
 *        cheaper — uniform chunks of ≤ 4608 rows that fill the chip.
 * G does not depend on the chunking beyond its f32 rounding; a given
 * chunk_rows gives the same bits in both i8×3 modes. */
#define OCM_GRAM_I8X3 0
#define OCM_GRAM_F32 1
#define OCM_GRAM_BF16X3 2
#define OCM_GRAM_I8X3_K32 3
int ocm_gram_f32_ex(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                    const float* shift, const int64_t* seg_offsets, int32_t nseg, int32_t mode, int64_t chunk_rows,
                    double* G_out, double* colsum_out, void* stream);

/* Outlier-guard marks ((row, 32-column group) pairs screened out) of the
 * context's last i8×3 Gram that synchronised (diagnostics / tests). */
int ocm_gram_last_marks(ocm_ctx* ctx, int64_t* marks_out);

/* Covariance from a signed combination of segment Grams (CV downdating):
 *   Gc = Σ_t coef[t]·G[t], sc = Σ_t coef[t]·colsum[t], d = sc/n,
 *   C = (Gc - n·d·dᵀ)/(n-1), mean = shift + d.
 * Replaces np.cov / explained_variance_ = S²/(n-1) (_pca.py:584).
 * G_list/colsum_list/coef [host] arrays of nterm pointers/values; C_out [dev]
 * p·p doubles; mean_out [dev] p doubles. */
int ocm_cov_from_gram(ocm_ctx* ctx, const double* const* G_list, const double* const* colsum_list,
                      const double* coef, int32_t nterm, const float* shift, int64_t n, int32_t p, double* C_out,
                      double* mean_out, void* stream);

/* Top-k eigenpairs of symmetric C (fp64 subspace iteration + Rayleigh-Ritz,
 * Jacobi on the projected block) and the tail moments
 *   theta[m-1] = Σ_{i>k} λ_i^m  (m = 1..3, utils/SIMCA.py:189-191, 203-204, 226-227)
 * computed from the deflated matrix (I-VVᵀ)C(I-VVᵀ) (traces, no full spectrum).
 * theta_mode: 0 none, 1 θ1..θ2, 2 θ1..θ3.
 * evals_out [dev] k (descending), evecs_out [dev] k×p rows = loadings with the
 * sklearn svd_flip sign (max-|entry| positive, extmath.py:895-953),
 * theta_out [dev] 3, iters_out [host, nullable].  Returns OCM_ERR_NOCONV if
 * the residual tolerance was not met within max_iter (outputs still valid).
 * Any 1 ≤ k ≤ p: the block is k plus oversampling; beyond 64 columns the
 * block's b×b Cholesky and Rayleigh–Ritz problems are solved on the host in
 * fp64 (the p×b products stay on the GPU). */
int ocm_eig_topk(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                 int32_t theta_mode, double* evals_out, double* evecs_out, double* theta_out, int32_t* iters_out,
                 void* stream);

/* Same, with the θ3 trace work split into `theta3_nslices` slices of which
 * this call computes slice `theta3_slice` only: theta_out[2] is then that
 * slice's partial sum and the caller sums the partials of every slice (the
 * ranks of a row-sharded fit each take one slice and all-reduce θ3;
 * SURVEY.md §8e).  theta_out[0..1] and all other outputs are complete on every
 * slice.  ocm_eig_topk is the call with (0, 1). */
int ocm_eig_topk_ex(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                    int32_t theta_mode, int32_t theta3_slice, int32_t theta3_nslices, double* evals_out,
                    double* evecs_out, double* theta_out, int32_t* iters_out, void* stream);
/* ocm_eig_topk_ex plus inv_out [dev] k = 1/λ with np.linalg.pinv's cutoff (|λ| ≤ rcond·max|λ| → 0), the
 * diagonal of pinv(cov(T)) that ocm_inv_evals_f64 forms (utils/SIMCA.py:69), queued inside the call so the
 * fit-set scoring can follow the eigensolve without another launch from the host. */
int ocm_eig_topk_ex2(ocm_ctx* ctx, const double* C, int32_t p, int32_t k, double tol, int32_t max_iter,
                     int32_t theta_mode, int32_t theta3_slice, int32_t theta3_nslices, double* evals_out,
                     double* evecs_out, double* theta_out, int32_t* iters_out, double rcond, double* inv_out,
                     void* stream);

/* ---- row-sharded fit: one all-reduce of packed moments ----
 * ocm_gram_pack turns a rank's shifted Gram (G, colsum about `shift`, n rows,
 * as ocm_gram_f32 returns them) into its moments about zero, packed
 *   packed_out[0 .. p(p+1)/2)      upper triangle (row-major) of
 *                                  G + s·csᵀ + cs·sᵀ + n·s·sᵀ  (Σ x xᵀ)
 *   packed_out[p(p+1)/2 .. +p)     cs + n·s                    (Σ x)
 *   packed_out[p(p+1)/2 + p]       n
 * so that a plain sum over ranks (one RCCL all-reduce of p(p+1)/2 + p + 1
 * doubles) gives the moments of all rows whatever shift each rank used.
 * ocm_cov_from_packed then forms μ = Σx/n and C = (Σ x xᵀ − n·μμᵀ)/(n−1)
 * (np.cov / sklearn explained_variance_, utils/SIMCA.py:64-66 →
 * _pca.py:584) with n read from the buffer on the device.  [dev] all. */
int ocm_gram_pack(ocm_ctx* ctx, const double* G, const double* colsum, const float* shift, int64_t n, int32_t p,
                  double* packed_out, void* stream);
int ocm_cov_from_packed(ocm_ctx* ctx, const double* packed, int32_t p, double* C_out, double* mean_out,
                        void* stream);

/* Symmetric pseudo-inverse (eigenvalue cutoff rcond·λmax) of a small d×d
 * fp64 matrix, d ≤ 64 (np.linalg.pinv(np.cov(...)) at utils/SIMCA.py:69,
 * VAE_SIMCA.py:247-248, utils/final_vaesimca.py:430-434).  [dev] in/out. */
int ocm_sym_pinv_f64(ocm_ctx* ctx, const double* A, int32_t d, double rcond, double* out, void* stream);

/* diag(pinv(cov(T))) on the eigenbasis, cov(T) = diag(λ): out_i = 1/λ_i
 * where |λ_i| > rcond·max|λ|, else 0 (np.linalg.pinv's cutoff, rcond 1e-15,
 * utils/SIMCA.py:69).  One launch in place of the host-issued elementwise
 * ops of the fit.  [dev] evals / out (k doubles, may alias).  ABI 9. */
int ocm_inv_evals_f64(ocm_ctx* ctx, const double* evals, int32_t k, double rcond, double* out, void* stream);

/* Fused scoring of float32 spectra (utils/SIMCA.py:65-71 fit, 104-107
 * transform, 127-130 predict):  y = x - mu; t = P·y (k); Q = ‖y − Pᵀt‖²;
 * T2 = tᵀ·A·t.  FP32 MFMA projection + explicit residual (first-order
 * insensitive to rounding in t).  P [dev] k×p float64 row-major with orthonormal rows
 * (ldp = p), mu [dev] p doubles, A [dev] k×k doubles.
 * Outputs (all nullable, [dev]): T_out m×k float32,
 * T2_out m doubles, Q_out m floats.  If dec != NULL [host] the decision is
 * fused: accept_out[r·accept_stride] = 1.0/0.0 (float64, the reference's
 * predictions[:, i] column).  stats_out [dev, nullable] 4 doubles
 * = {ΣT2, ΣT2², ΣQ, ΣQ²} (chi2pom moments).  k ≤ 64. */
int ocm_score_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                  const double* P, const double* mu, const double* A, int32_t k, float* T_out, double* T2_out,
                  float* Q_out, const ocm_decision* dec, double* accept_out, int64_t accept_stride,
                  double* stats_out, void* stream);

/* Same with A = diag(a_diag) (a_diag [dev] k doubles) — the SIMCA case: the
 * scores are on the eigenbasis, so invcovT = pinv(cov(T)) = diag(1/λ)
 * (utils/SIMCA.py:69).  For p ∈ {256, 512, 1024, 2048}, k ≤ 20 and 16-B
 * aligned X / ldx this runs k_score_1p, which reads every row of X from HBM
 * once (the row tile stays in registers between the projection and the
 * residual); other shapes take the two-sweep kernel of ocm_score_f32.
 * Arguments and outputs as ocm_score_f32. */
int ocm_score_f32_diag(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                       const double* P, const double* mu, const double* a_diag, int32_t k, float* T_out,
                       double* T2_out, float* Q_out, const ocm_decision* dec, double* accept_out,
                       int64_t accept_stride, double* stats_out, void* stream);

/* Reduced distances and decision from stored T2/Q (utils/SIMCA.py:76-81,
 * 109-114, 131-145).  Outputs nullable [dev]: t2red, qred, dred (m doubles),
 * accept (m doubles 0/1 at stride accept_stride). */
int ocm_decide(ocm_ctx* ctx, const double* T2, const float* Q, int64_t m, const ocm_decision* dec,
               double* t2red_out, double* qred_out, double* dred_out, double* accept_out, int64_t accept_stride,
               void* stream);

/* q_i = Σ_j (x_ij - xhat_ij)² (fp64 accumulation) for a VAE reconstruction
 * (vae_model.py:164, utils/final_vaesimca.py:425,492), the latent round-trip Q
 * (VAE_SIMCA.py:256-259, 365-366) and the Euclidean latent distance h about a
 * stored mean (utils/final_vaesimca.py:510-512: ldxh = 0 broadcasts one xhat
 * row).  x [dev] m×p float32 (ldx), xhat [dev] (ldxh), q_out [dev] m floats. */
int ocm_rowsq_residual_f32(ocm_ctx* ctx, const float* x, int64_t ldx, const float* xhat, int64_t ldxh, int64_t m,
                           int32_t p, float* q_out, void* stream);

/* q_i = Σ_j (s(x_ij) − s(xhat_ij))², s(v) = clamp((v − min_j x_ij)/(max_j x_ij − min_j x_ij + eps), 0, 1):
 * the per-sample min–max scaled reconstruction residual that
 * utils/final_vaesimca.py:417-423 (calibration Q threshold) and :484-490
 * (test Q) use for BCE-trained networks (eps = 1e-8 there).  Scaling in
 * float32 in the reference's order, f64 sum.  x, xhat [dev] m×p float32
 * (ldx, ldxh ≥ p), q_out [dev] m floats. */
int ocm_rowsq_minmax_f32(ocm_ctx* ctx, const float* x, int64_t ldx, const float* xhat, int64_t ldxh, int64_t m,
                         int32_t p, float eps, float* q_out, void* stream);

/* b[i] = (float)a[i] — loadings / mean handed to the float32 scoring kernel. */
int ocm_cast_f64_f32(ocm_ctx* ctx, const double* a, int64_t n, float* b, void* stream);

/* np.percentile(v, pct) with linear interpolation (utils/SIMCA.py:160,187;
 * VAE_SIMCA.py:285,305; utils/final_vaesimca.py:436-437) by radix select.
 * dtype: 0 = float64, 1 = float32.  v [dev] n values (no NaN);
 * out [host] 1 double. */
int ocm_percentile(ocm_ctx* ctx, const void* v, int32_t dtype, int64_t n, double pct, double* out, void* stream);

/* One radix-select pass (for multi-rank percentiles: callers all-reduce the
 * histogram between passes).  Counts values whose order key matches
 * `prefix` on the bits above `shift + 8`, binned by the 8 bits at `shift`.
 * hist_out [dev] 256 uint64 (overwritten). */
int ocm_radix_hist(ocm_ctx* ctx, const void* v, int32_t dtype, int64_t n, uint64_t prefix, int32_t shift,
                   uint64_t* hist_out, void* stream);

/* ---- class-wise cross-validation fold engine (utils/CVSIMCA.py:103-269) ----
 * One Gram pass gives every fold's Gram (segments), train Gram = total − fold;
 * one eigensolve per fold at LV_max; each LV ≤ LV_max reuses it through
 *   T²_LV = Σ_{j<LV} t_j²/λ_j,   Q_LV = Q_{LVmax} + Σ_{LV≤j<LVmax} t_j².   */

/* G_out = Σ_t coef[t]·G_list[t] (p×p), colsum_out = Σ_t coef[t]·colsum_list[t]
 * (either output nullable; colsum_list nullable).  G_out may alias G_list[0]
 * only.  G_list/colsum_list/coef [host] arrays of nterm device pointers/values. */
int ocm_gram_combine(ocm_ctx* ctx, const double* const* G_list, const double* const* colsum_list,
                     const double* coef, int32_t nterm, int32_t p, double* G_out, double* colsum_out, void* stream);

/* Per-LV T² and Q of m rows from their LV_max scores (training rows of a fold:
 * the perc / chi2pom limit statistics, utils/SIMCA.py:157-159, 172-181, 186-187,
 * 211-216).  T [dev] m×k float32 (from ocm_score_f32, k = LV_max), Q [dev] m
 * float32, inv_evals [dev] k doubles (diag of invcovT), lvs [host] nlv values
 * in [1, k].  Outputs nullable [dev]: T2_out nlv×m doubles, Q_out nlv×m floats,
 * stats_out nlv×4 doubles {ΣT², ΣT²², ΣQ, ΣQ²}.  k, nlv ≤ 64. */
int ocm_cv_prefix(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                  const int32_t* lvs, int32_t nlv, double* T2_out, float* Q_out, double* stats_out, void* stream);

/* One decision configuration of the CV sweep: LV components, a decision
 * type and its scales / critical distance (as ocm_decision). */
typedef struct ocm_cv_config {
  int32_t lv;
  int32_t type;
  double t2_scale;
  double q_scale;
  double dlim;
} ocm_cv_config;
#define OCM_CV_MAXCFG 1024

/* Confusion counts of every configuration over the test rows of a fold
 * (utils/CVSIMCA.py:186-199 → utils/SIMCA.py:238-266): rows < m_split are the
 * held-out target rows, the rest the other-class rows.  positive [dev] m
 * bytes (y_true == class_index).  counts_out [dev] ncfg×2×4 uint64
 * {TP, TN, FP, FN} per (config, part).  accept_out [dev, nullable] ncfg×m
 * doubles 0/1 (pooled predictions).  cfg [host]. */
int ocm_cv_counts(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                  const uint8_t* positive, int64_t m_split, const ocm_cv_config* cfg, int32_t ncfg,
                  uint64_t* counts_out, double* accept_out, void* stream);

/* Per-object votes and decision sums of every configuration over rows scored
 * at LV_max (object-wise cross-validation; the object rules of
 * SIMCA.predict_objects, utils/SIMCA.py:560-564).  T, Q, inv_evals and cfg
 * [host] as for ocm_cv_counts.  Objects are runs of adjacent rows: offsets
 * [dev] G + 1 non-decreasing int64 with offsets[0] = 0 and offsets[G] = m (not
 * checked here: offsets that break this give wrong results, never an access
 * out of bounds).  Outputs [dev], either nullable but not both:
 *   votes_out ncfg×G uint32: the rows of object g that configuration c
 *     accepts, the accept being that of ocm_cv_counts bit for bit;
 *   dsum_out  ncfg×G doubles: Σ over the rows of object g of dlim_c − d_red,c(row)
 *     (decision_function), summed in an order fixed by m, the offsets and ncfg
 *     alone, without atomics: the same bits on every call, with or without
 *     votes_out.
 * An object without rows gets 0.  k ≤ 64, ncfg ≤ OCM_CV_MAXCFG; m = 0 or G = 0
 * is a successful no-op.  Per-chunk partial sums use the context workspace
 * (24 bytes per 256 rows and configuration). */
int ocm_cv_objects(ocm_ctx* ctx, const float* T, int64_t m, int32_t k, const float* Q, const double* inv_evals,
                   const int64_t* offsets, int64_t G, const ocm_cv_config* cfg, int32_t ncfg,
                   uint32_t* votes_out, double* dsum_out, void* stream);

/* Confusion counts of one class column of a prediction matrix
 * (utils/SIMCA.py:238-245, called from predict(X, y_true) at :146-152):
 * accept [dev] m doubles 0/1 at stride accept_stride (the column written by
 * ocm_score_f32*'s fused decision), positive [dev] m bytes (y_true == class).
 * counts_out [dev] 4 uint64 {TP, TN, FP, FN}. */
int ocm_confusion_counts(ocm_ctx* ctx, const double* accept, int64_t m, int64_t accept_stride,
                         const uint8_t* positive, uint64_t* counts_out, void* stream);

/* ---- spectral preprocessing ----
 * SNV x ← (x − mean_row)/(std_row + 1e-8) (np.std ddof 0; simca_nuts.py:47-49,
 * utils/data_utils.py:57) when snv != 0, then, when window > 0, the
 * Savitzky–Golay filter scipy.signal.savgol_filter(x, window, polyorder,
 * deriv, delta, axis=1, mode='interp') (simca_nuts.py:51,
 * simca_new_cheese.py:37-38) given as taps [host] (window + 2·(window/2)·window
 * doubles: interior correlation taps, then the left and right edge rows; see
 * ocm/preprocess.py savgol_taps).  One HBM pass per row.  X, out [dev] m×p
 * float32 (ldx, ldo; out may not alias X).  window odd ≤ 63, p ≤ 12288. */
int ocm_snv_savgol_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, int32_t snv,
                       int32_t window, const double* taps, float* out, int64_t ldo, void* stream);

/* ---- dense symmetric eigensolver (fp64) ----
 * evals_out [dev] all p eigenvalues of C (p×p fp64, symmetric) in descending order; when k > 0,
 * evecs_out [dev] k×p the leading k eigenvectors as rows (svd_flip sign: largest |entry| positive).
 * Householder tridiagonalisation on the GPU, QL eigenvalues and inverse-iteration vectors of the
 * tridiagonal on the host, back-transformation on the GPU.  Replaces the full spectrum of the
 * reference's SVD (utils/SIMCA.py:64-66,88 `eigs_all`; sklearn _pca.py:584-598) and is the fallback of
 * ocm_eig_topk when its subspace iteration does not converge.  Synchronises the stream.
 * Limits: 1 ≤ p ≤ 16384 for eigenvalues only (k = 0); p ≤ 12288 when k > 0 (checked before any
 * work).  OCM_ERR_NOCONV if the implicit QL of the tridiagonal does not converge. */
int ocm_eigh_f64(ocm_ctx* ctx, const double* C, int32_t p, double* evals_out, int32_t k, double* evecs_out,
                 void* stream);

/* ---- preprocessing in the load path (lazy view) ----
 * The drivers run SNV then Savitzky–Golay right before SIMCA
 * (simca_nuts.py:47-52, simca_new_cheese.py:37-38, utils/data_utils.py:57-61).
 * An ocm_prep describes that transform and the *_prep kernels apply it to each
 * row as they load it, so the preprocessed matrix X′ never exists in HBM.
 * Row r, column j, float32 arithmetic identical in every kernel (the Gram,
 * the scores and ocm_prep_apply_f32 see bit-identical values):
 *   u_c = x_c − m_r when snv and deriv == 0, else u_c = x_c
 *   window == 0:                 a = u_j
 *   interior, odd deriv:         a = Σ_{t=1..H} c_{H+t}·(u_{j+t} − u_{j−t})   (c antisymmetric)
 *   interior, deriv 0:           a = c_H·u_j + Σ_{t=1..H} c_{H+t}·(u_{j+t} + u_{j−t})
 *   interior, even deriv ≥ 2:    a = Σ_{t=1..H} c_{H+t}·((u_{j+t} − u_j) + (u_{j−t} − u_j))
 *   edges (j < H or j ≥ p − H):  a = Σ_t e_{j,t}·(u_{s+t} − [deriv ≥ 1]·u_j), s = 0 or p − window
 *   y_j = a·s_r when snv, else a
 * (fmaf chains in t order from 0; H = window/2; (m_r, s_r) = (mean_r,
 * 1/(std_r + 1e-8)) from ocm_prep_rowstats_f32).  Savitzky–Golay maps a
 * constant to 0 for deriv ≥ 1 and to itself for deriv 0, so y = SG(SNV(x))
 * up to float32 rounding, with the row mean cancelling exactly in the
 * drivers' deriv-1 filters; differences of neighbouring samples keep a large
 * baseline from costing precision. */
typedef struct ocm_prep {
  int32_t window;        /* 0 (SNV only) or odd 3..31 */
  int32_t deriv;         /* Savitzky–Golay derivative order (0 when window == 0) */
  int32_t snv;           /* 1: apply the SNV row statistics */
  int32_t pad_;
  const float* taps;     /* [dev] window + 2·H·window floats: interior c, left-edge rows, right-edge rows
                            (ocm/preprocess.py savgol_taps); NULL when window == 0 */
  const float* rowstat;  /* [dev] (m_r, s_r) per row of X, indexed like X (gather lists index it too);
                            NULL when snv == 0 */
} ocm_prep;

/* rowstat_out [dev] m×2 floats: m_r = mean (fp64, rounded), s_r = 1/(std_r + 1e-8) (np.std ddof 0)
 * of each row of X — the one read-only pre-pass the SNV needs. */
int ocm_prep_rowstats_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, float* rowstat_out,
                          void* stream);
/* out [dev] m×p (ldo) = the preprocessed rows X[rows[i]] (rows nullable): the materialised view, for
 * shapes and modes the fused kernels do not cover and for tests. */
int ocm_prep_apply_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                       const ocm_prep* prep, float* out, int64_t ldo, void* stream);
/* ---- scatter correction against a reference spectrum (MSC, EMSC) ----
 * Basis B: q × p fp64, 2 ≤ q ≤ 8 and p ≥ q: row 0 all ones, row 1 the reference spectrum, rows 2.. the
 * baseline (polynomials in λ ∈ [−1, 1]) and interferent terms.  Weights W = pinv(Bᵀ), q × p fp64, from
 * the host (ocm/preprocess.py scatter_weights).  Row coefficients c = W·x: c0 the offset, c1 the scale,
 * c2.. the baseline amplitudes — the least-squares fit x ≈ Σ_t c_t·B_t.
 *   MSC  (q = 2, = np.polyfit(ref, x, 1)):  y_j = (x_j − c0) / c1
 *   EMSC:                                   y_j = (x_j − c0 − Σ_{t≥2} c_t·B_tj) / c1
 * No epsilon is added to c1: a row orthogonal to the reference gives inf / nan, as NumPy does.
 * Numerics: the q dot products are fp64 sums of (double)x_j·W_tj in a fixed order (no atomics: the same
 * bits on every launch); coefficients are the fp64 results rounded to float32.  The row-affine pair of a
 * lazy view (ocm_prep.rowstat with snv = 1) is m_r = (float)c0, s_r = (float)(1.0 / c1), so the view's
 * y_j = (x_j − m_r)·s_r is MSC.  ocm_emsc_apply_f32 then works in float32, in this order:
 *   u = x_j − m_r;  for t = 2, 3, .., q − 1:  u = fmaf(−(float)c_t, (float)B_tj, u);  y_j = u·s_r
 * (the product never fused into a later operation), which for q = 2 is what ocm_prep_apply_f32 writes for
 * the MSC view of the same rows, bit for bit.
 * X [dev] m × p float32, any ldx ≥ p and any 4-byte alignment (16-byte aligned rows, W and B with
 * p % 4 == 0 and p ≤ 4096 (p ≤ 2048 when q > 4) take the vector path: the row stays in registers); W, B
 * [dev] q × p fp64,
 * dense (B may be NULL when q = 2).  OCM_ERR_ARG for q < 2, q > 8 or p < q. */
/* One read-only pass over X.  coef_out [dev] m × q floats (nullable), rowstat_out [dev] m × 2 floats
 * (m_r, s_r) (nullable); at least one of them. */
int ocm_rowfit_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const double* W, int32_t q,
                   float* coef_out, float* rowstat_out, void* stream);
/* One read and one write of X: out [dev] m × p (ldo ≥ p) = the corrected rows; coef_out as above (nullable). */
int ocm_emsc_apply_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const double* W,
                       const double* B, int32_t q, float* out, int64_t ldo, float* coef_out, void* stream);
/* ---- baseline correction: Whittaker smoother and asymmetric least squares (Eilers & Boelens 2005) ----
 * D is the d-th order difference matrix, np.diff(np.eye(p), d, axis=0), d ∈ {1, 2}; λ > 0.
 *   Whittaker: for a row x (float32, read as fp64) and weights w ≥ 0, z solves
 *       (diag(w) + λ·DᵀD) z = w ∘ x
 *     a symmetric system of half bandwidth d, positive definite when at least d weights are positive.
 *   AsLS(λ, asym, n_iter): w⁽¹⁾ = 1; for it = 1..n_iter, z⁽ⁱᵗ⁾ is the Whittaker solve of x under w⁽ⁱᵗ⁾ and
 *       w⁽ⁱᵗ⁺¹⁾_j = asym if x_j > z⁽ⁱᵗ⁾_j else 1 − asym
 *     (compared in fp64 on the unrounded z; an exact tie takes 1 − asym, where Eilers' code gives 0: the
 *     matrix stays positive definite).  A row stops once an update leaves all its weights unchanged
 *     (further solves would repeat bit for bit); iters is the number of solves the row ran.  The result
 *     is the baseline z of the last solve, or x − z formed in fp64, rounded once to float32.
 * Numerics: LDLᵀ without pivoting, every recurrence in fp64 (the systems reach condition numbers of 1e8
 * and more at ordinary settings), one lane per row in one fixed order: the same bits on every launch,
 * for any m, any position of the row in the matrix and any ldx / ldo.  No atomics but the nbad count.
 * A row whose pivot is not a positive finite number, or with a negative or NaN weight, or with fewer
 * than d positive weights, is written as NaN and counted in nbad_out; no other row is affected.
 * Workspace: a workgroup's 64 rows keep (d + 1)·8 bytes per element (8 under shared weights) for the
 * back substitution, AsLS one bit more.  The grid is at most 8 workgroups per CU and walks over the
 * 64-row blocks, so the workspace depends on the device and on p (at most CUs·8·64·p·(8·(d + 1) + 1/8)
 * bytes), not on m: 2M rows need no more than 1M.
 * X [dev] m × p float32 (ldx ≥ p, any 4-byte alignment), out [dev] m × p float32 (ldo ≥ p), not
 * overlapping X.  OCM_ERR_ARG for d ∉ {1, 2}, p < d + 1, λ not positive and finite, ldx or ldo < p,
 * m ≥ 2³¹. */
/* W [dev]: NULL: w = 1; ldw = 0: one (p) vector for all rows; ldw ≥ p: (m, p) per row.  With shared weights
 * the matrix is factorised once and a row costs one read, one write and 16 bytes of workspace traffic per
 * element.  nbad_out [dev] one int32 (nullable). */
int ocm_whittaker_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const float* W, int64_t ldw,
                      double lam, int32_t d, float* out, int64_t ldo, int32_t* nbad_out, void* stream);
/* subtract 0: out = the baseline z, 1: out = x − z.  iters_out [dev] m int32 (nullable).  Also
 * OCM_ERR_ARG for asym ∉ (0, 1) or n_iter < 1. */
int ocm_asls_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, double lam, double asym, int32_t d,
                 int32_t n_iter, int32_t subtract, float* out, int64_t ldo, int32_t* iters_out, void* stream);
/* ocm_colmean_f32 / ocm_gram_f32_ex / ocm_score_f32_diag on the preprocessed rows, read raw from X.
 * The default i8×3 Gram applies the transform in its quantiser (halo columns staged through LDS) and
 * k_score_1p applies it to each row tile in registers as the tile arrives (p ∈ {256, 512, 1024, 2048},
 * window ∈ {0, 5, 15}, p % 4 == 0); other shapes, windows and Gram modes materialise the preprocessed
 * rows in a temporary device buffer first. */
int ocm_colmean_f32_prep(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                         const ocm_prep* prep, double* mean_out, void* stream);
int ocm_gram_f32_prep(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                      const float* shift, const int64_t* seg_offsets, int32_t nseg, int32_t mode,
                      int64_t chunk_rows, const ocm_prep* prep, double* G_out, double* colsum_out, void* stream);
/* Write-through (round 5): ocm_gram_f32_prep (i8×3, all n rows of X, no gather list) whose quantiser
 * also writes the preprocessed rows to xout [dev] n×p (ldo % 4 == 0, 16-B aligned) as it forms them:
 * the stencil runs once, in the Gram's read of X, and the consumers after the Gram (scoring of the fit
 * and predict sets) read X′ with the plain kernels.  The values are those of ocm_prep_apply_f32 bit for
 * bit.  Shapes and transforms the fused quantiser does not cover run the eager pass into xout, then the
 * Gram on it. */
int ocm_gram_f32_prep_write(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t n, int32_t p, const float* shift,
                            const int64_t* seg_offsets, int32_t nseg, int64_t chunk_rows, const ocm_prep* prep,
                            double* G_out, double* colsum_out, float* xout, int64_t ldo, void* stream);
/* Number of times this context materialised a lazy view (the fallback paths above), for tests and
 * diagnostics: 0 after any call on the fused paths. */
int ocm_prep_materialised(ocm_ctx* ctx, int64_t* count_out);
/* How many Rayleigh–Ritz tests of ocm_eig_topk* this context ran twice: the
 * test fused into the Jacobi takes S from a side stream in flight and gives up
 * after ≈ 1 s (kernels serialised, or the side stream not scheduled); the host
 * then runs the Jacobi + test again behind S's event (a diagnostic counter). */
int ocm_eig_test_reruns(ocm_ctx* ctx, int64_t* count_out);
int ocm_score_f32_diag_prep(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                            const ocm_prep* prep, const double* P, const double* mu, const double* a_diag, int32_t k,
                            float* T_out, double* T2_out, float* Q_out, const ocm_decision* dec,
                            double* accept_out, int64_t accept_stride, double* stats_out, void* stream);

/* ---- float64 spectra: the PCA precision follows the input dtype ----
 * The reference's PCA runs in the input dtype (utils/SIMCA.py:64-66 →
 * sklearn _pca.py:544-584 on float64 X), and its scores, residuals and Q are
 * then float64 (utils/SIMCA.py:65-71, 104-107, 127-130).  X [dev] n×p float64
 * (ldx elements); rows as above.
 *
 * ocm_colmean_f64: column mean of the first n processed rows (fp64).
 * ocm_gram_f64: per-segment shifted Gram Σ (x − s)(x − s)ᵀ and Σ (x − s) on
 *   fp64 MFMA (v_mfma_f64_16x16x4f64), no digit split; arguments and outputs as
 *   ocm_gram_f32 (the float shift is exact in fp64), so ocm_cov_from_gram /
 *   ocm_gram_pack apply unchanged.
 * ocm_score_f64_diag: t = P·(x − μ), T² = Σ t²·a_diag, and Q = ‖(x − μ) − Pᵀt‖²
 *   as the explicit residual of the reconstruction X̂ = T·P + μ
 *   (utils/SIMCA.py:67-68, 71), fused decision and the moments, as
 *   ocm_score_f32_diag; T_out m×k float64 (nullable), Q_out m float64; any
 *   1 ≤ k ≤ p (component blocks of 64 beyond that).
 * ocm_decide_f64: ocm_decide with float64 Q. */
int ocm_colmean_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                    double* mean_out, void* stream);
int ocm_gram_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                 const float* shift, const int64_t* seg_offsets, int32_t nseg, double* G_out, double* colsum_out,
                 void* stream);
int ocm_score_f64_diag(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                       const double* P, const double* mu, const double* a_diag, int32_t k, double* T_out,
                       double* T2_out, double* Q_out, const ocm_decision* dec, double* accept_out,
                       int64_t accept_stride, double* stats_out, void* stream);
int ocm_decide_f64(ocm_ctx* ctx, const double* T2, const double* Q, int64_t m, const ocm_decision* dec,
                   double* t2red_out, double* qred_out, double* dred_out, double* accept_out, int64_t accept_stride,
                   void* stream);

/* ---- contribution plots (which variables put a sample outside the class) ----
 * For every processed row (all rows, or X[rows[r]]), with y = x − μ, t = P·y
 * and a = diag(1/λ) (the model of ocm_score_f32_diag, utils/SIMCA.py:67-71):
 *   e_j = y_j − Σ_c t_c·P_cj          the residual;        Σ_j e_j² = Q
 *   c_j = y_j · Σ_c (t_c·a_c)·P_cj    the T² contribution; Σ_j c_j  = T² (c_j may be negative)
 * group [dev, nullable] m bytes: the profile group of each processed row, in
 *   [0, ngroups), ngroups 1..4 (NULL: every row in group 0; rows with a larger
 *   id contribute to no profile).
 * E_out, C_out [dev, nullable] m×p (lde, ldc ≥ p): e and c.
 * T2_out, Q_out [dev, nullable] m: the row sums Σ_j c_j and Σ_j e_j².
 * prof_out [dev, nullable] ngroups×2×p: Σ_rows e_j² then Σ_rows c_j per group,
 *   summed in a fixed order (two launches on one input give the same bits).
 * Any p ≥ 1, 1 ≤ k ≤ min(p, 64), m ≥ 1, no alignment requirement.  With E_out
 * and C_out NULL a launch writes O(m + p) values and its workspace does not
 * grow with m.  f32: f32 MFMA products, t in f32 over ≤ 64 columns per chain
 * flushed to f64, the residual formed in f32 (as the reference forms
 * X − (T·P + μ) in float32); f64: fp64 MFMA throughout. */
int ocm_contrib_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                    const double* P, const double* mu, const double* a_diag, int32_t k, const uint8_t* group,
                    int32_t ngroups, float* E_out, int64_t lde, float* C_out, int64_t ldc, double* T2_out,
                    float* Q_out, double* prof_out, void* stream);
int ocm_contrib_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                    const double* P, const double* mu, const double* a_diag, int32_t k, const uint8_t* group,
                    int32_t ngroups, double* E_out, int64_t lde, double* C_out, int64_t ldc, double* T2_out,
                    double* Q_out, double* prof_out, void* stream);

/* ---- object-level sums (an object = a run of adjacent rows) ----
 * The data sets are objects of many pixel spectra each (nut_data.py:131-185 stores every connected
 * component as an (n_pixels, p) block); the per-object sums the host loops over `obj_ids == idx`
 * (utils/data_utils.py:79-82) form, in one read of X:
 *   sum_out[g, j] = Σ_{r = offsets[g]}^{offsets[g+1]−1} (double)X[r·ldx + j]      g < nseg, j < p
 * offsets [dev] nseg + 1 int64, non-decreasing, 0 ≤ offsets[0], offsets[nseg] ≤ m ((nseg + 1)·8 bytes,
 *   read by every workgroup from L2).  They are NOT checked here, as `rows` is not: the caller
 *   validates them (ocm/objects.py check_offsets).  Offsets that break the contract give wrong sums but
 *   no access outside X, sum_out or the workspace: row reads are bounded by m and segment indices by
 *   nseg in the kernels.
 * X [dev] m × p float32 / float64, any ldx ≥ p; rows outside [offsets[0], offsets[nseg]) and columns
 *   ≥ p of a strided X are never read.  Loads are 16 bytes per lane when p, ldx and the base allow
 *   (p % 4 == 0, ldx % 4 == 0, 16-byte aligned; float64: % 2), else 8 or 4 (float64: 8).
 * sum_out [dev] nseg × ld_out doubles (ld_out ≥ p; nseg·p·8 bytes written, columns ≥ p untouched); an
 *   empty segment gives exactly 0.0.
 * Numerics: fp64 accumulation; the summation order is a function of the offsets alone (rows in order
 *   inside each 256-row chunk at multiples of 256, then a segment's chunk partials in chunk order,
 *   aligned groups of 64 chunks summed first), no floating-point atomics: two calls give the same bits.
 * Workspace: (2 + 1/64)·(m/256 + 1)·p doubles (134 MB at 1M × 2048), written only where a segment
 *   crosses a chunk boundary.  nseg = 0 is a no-op; m = 0 writes zeros.  OCM_ERR_ARG for m ≥ 2^31. */
int ocm_segsum_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, const int64_t* offsets,
                   int64_t nseg, double* sum_out, int64_t ld_out, void* stream);
int ocm_segsum_f64(ocm_ctx* ctx, const double* X, int64_t ldx, int64_t m, int32_t p, const int64_t* offsets,
                   int64_t nseg, double* sum_out, int64_t ld_out, void* stream);

/* ---- VAE network support (vae_model.py:37-81, BatchNorm1d in train mode) ----
 * Training-mode batch norm over (N, C, L) contiguous activations, bf16 or f32,
 * statistics per channel over N·L < 2³¹ (torch.nn.functional.batch_norm semantics:
 * biased variance normalises, unbiased variance feeds running_var with
 * `momentum`).  Replaces the MIOpen spatial BN the reference's nn.BatchNorm1d
 * lowers to (vae_model.py:45-47, 75-77).  running_mean / running_var may both
 * be NULL (no update); gamma / beta may be NULL (affine=False); num_batches_tracked
 * [nullable] is incremented by one (nn.BatchNorm1d's counter).  scratch [dev]
 * ocm_bn_scratch_bytes(C) bytes of caller-owned memory that stays put while a
 * captured hipGraph replays the launches, ZERO-FILLED BEFORE ITS FIRST USE and
 * then reused by every call of that layer (forward and backward): it ends in
 * per-channel completion counters — the last of a channel's reduction
 * workgroups forms the statistics, one launch per direction fewer — which
 * every call leaves zero.  Calls sharing one scratch must be stream-ordered.
 * All work is stream-ordered (graph-capturable).
 * Accuracy of the statistics: the variance is Σx²/M − mean² with Σx and Σx² held in float32 per
 * thread (t terms each, t = 32 at N·L = 136000, C = 2; f64 across threads), so under a common
 * offset its relative error grows as (μ/σ)²·2⁻²⁴·t: at most (t + 2)·2⁻²⁴·(1 + (μ/σ)²), measured
 * 3.5e-5 at |μ|/σ = 100 and that shape (y is then off by up to 1.2e-4 absolute).  The backward's
 * sums Σdz and Σdz·x̂ are accumulated in f64 per thread. */
#define OCM_DTYPE_F32 0
#define OCM_DTYPE_BF16 1
/* act: OCM_ACT_ELU fuses the ELU (α = 1) that follows every batch norm of the
 * VAE (vae_model.py:45-49, 75-79): y = ELU(BN(x)) forward; the backward takes
 * the gradient of the ELU output and that output y (dz = dy·(y > 0 ? 1 : y + 1)). */
#define OCM_ACT_NONE 0
#define OCM_ACT_ELU 1
size_t ocm_bn_scratch_bytes(int32_t C);
int ocm_bn_fwd_train(ocm_ctx* ctx, int32_t dtype, const void* x, int32_t N, int32_t C, int32_t L,
                     const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                     float* running_var, int64_t* num_batches_tracked, int32_t act, void* y, float* save_mean,
                     float* save_invstd, void* scratch, void* stream);
/* Eval-mode BatchNorm1d (running statistics, vae_model.py:45-47 in model.eval(), the
 * latent encoding of utils/final_vaesimca.py:406-442): y = (x − rm)·γ/√(rv + ε) + β,
 * then the fused ELU with act = OCM_ACT_ELU; gamma / beta nullable.  No scratch,
 * any N (one flat grid).  ABI 9. */
int ocm_bn_fwd_eval(ocm_ctx* ctx, int32_t dtype, const void* x, int32_t N, int32_t C, int32_t L,
                    const float* running_mean, const float* running_var, float eps, const float* gamma,
                    const float* beta, int32_t act, void* y, void* stream);
/* dx = γ·invstd·(dz − mean(dz) − x̂·mean(dz·x̂)), dz = dy (act NONE) or the ELU's input gradient;
 * dgamma = Σ dz·x̂, dbeta = Σ dz (either may be NULL); y [act ELU] the forward's output. */
int ocm_bn_bwd(ocm_ctx* ctx, int32_t dtype, const void* x, const void* dy, int32_t N, int32_t C, int32_t L,
               const float* gamma, const float* save_mean, const float* save_invstd, int32_t act, const void* y,
               void* dx, float* dgamma, float* dbeta, void* scratch, void* stream);
/* ocm_bn_fused_timeouts (ABI 12): with OCM_BN_FUSED=1 in the environment (an experiment, off by default:
 * slower on the C4 step), training-mode ocm_bn_fwd_train / ocm_bn_bwd run as ONE launch where the
 * layout allows (L % 8 = 0, 16-byte aligned tensors, the grid co-resident on the device): each workgroup
 * keeps its share of the channel in registers while the channel's last workgroup forms the statistics,
 * the others waiting on an epoch word in the scratch.  A wait that exceeds ≈ 1 s gives up rather than
 * hang (its outputs are then wrong) and is counted (count_out: the process total). */
int ocm_bn_fused_timeouts(int64_t* count_out);

/* ---- VAE narrow convolutions (vae_model.py:37-81: Conv1d / ConvTranspose1d,
 * 1-12 channels, kernel 7, stride 1 or 2; the layers nn.Conv1d /
 * nn.ConvTranspose1d lower to MIOpen in the reference) ----
 * Activations (B, C, L) contiguous, float32 or bfloat16 (dtype_*: OCM_DTYPE_*);
 * weights, bias, gradients float32; float32 accumulation.  Stream-ordered,
 * graph-capturable (scratch is caller-owned).
 *
 * ocm_conv1d, mode OCM_CONV_DOWN:  y[b][o][l] = bias[o] + Σ_i Σ_t w[o][i][t]·x[b][i][l·s + t − pad]
 *   (Conv1d forward, w [O][I][K]; ConvTranspose1d input gradient with w its [I][O][K] weight, x = dy);
 * mode OCM_CONV_UP:  y[b][o][j] = bias[o] + Σ_i Σ_t w[i][o][t]·x[b][i][(j + pad − t)/s] over the
 *   terms where s divides j + pad − t (ConvTranspose1d forward, w [I][O][K]; Conv1d input gradient with
 *   w its [O][I][K] weight read as [I][O][K] of dy's channels).  bias nullable; I ≤ 64, K ≤ 15.
 * ocm_conv1d_wgrad: G[o][i][t] = Σ_b Σ_l P[b][o][l]·Q[b][i][l·s + t − pad], written [O][I][K]
 *   (Conv1d: P = dy, Q = x → its [O][I][K] weight gradient; ConvTranspose1d: P = x, Q = dy → its
 *   [I][O][K] weight gradient); psum_out [nullable] = Σ_b Σ_l P[b][o][l] (Conv1d's bias gradient).
 *   scratch ≥ ocm_conv1d_scratch_bytes(O, I, K), zero-filled before its first use and reused (it
 *   starts with completion counters that every call leaves zero: the last partial workgroup of
 *   an output group sums the partials — one launch); fixed-order two-stage sums (deterministic).
 * ocm_conv1d_wgrad_qsum (ABI 12): the same G, and qsum_out[i] = Σ_b Σ_j Q[b][i][j] (ConvTranspose1d's bias
 *   gradient, Q = dy) in the same launch when Lq = s·Lp and pad + s ≤ K (bf16 operands, the matrix-core
 *   path: a row of ones in P), else by ocm_chan_sum after it.  scratch as ocm_conv1d_wgrad's.
 * ocm_chan_sum: out[c] = Σ_b Σ_l v[b][c][l] (the bias gradient), C ≤ 284; scratch as above with
 *   O·I·K ≥ C (the same zero-filled, reused memory as the layer's wgrad may serve both). */
#define OCM_CONV_DOWN 0
#define OCM_CONV_UP 1
size_t ocm_conv1d_scratch_bytes(int32_t O, int32_t I, int32_t K);
int ocm_conv1d(ocm_ctx* ctx, int32_t mode, int32_t dtype_in, const void* x, int32_t B, int32_t I, int32_t Lin,
               const float* w, const float* bias, int32_t O, int32_t Lout, int32_t K, int32_t stride, int32_t pad,
               int32_t dtype_out, void* y, void* stream);
int ocm_conv1d_wgrad(ocm_ctx* ctx, int32_t dtype_p, const void* P, int32_t O, int32_t Lp, int32_t dtype_q,
                     const void* Q, int32_t I, int32_t Lq, int32_t B, int32_t K, int32_t stride, int32_t pad,
                     float* G_out, float* psum_out, void* scratch, void* stream);
int ocm_conv1d_wgrad_qsum(ocm_ctx* ctx, int32_t dtype_p, const void* P, int32_t O, int32_t Lp, int32_t dtype_q,
                          const void* Q, int32_t I, int32_t Lq, int32_t B, int32_t K, int32_t stride, int32_t pad,
                          float* G_out, float* qsum_out, void* scratch, void* stream);
int ocm_chan_sum(ocm_ctx* ctx, int32_t dtype, const void* v, int32_t B, int32_t C, int32_t L, float* out,
                 void* scratch, void* stream);

/* ---- the VAE training step's small tensors, fused (vae_model.py:136-158, vae_bce_nut.py:178-203,
 * utils/final_vaesimca.py:198-224): the graphed step is bound by its kernel count, so the
 * reparameterisation + KL, the de-standardisation + reconstruction term + total, their backward
 * passes and Adam each take one launch.  Activations in dtype (OCM_DTYPE_*), sums fp64 with
 * fixed-order partials, losses float32; graph-capturable (scratch caller-owned,
 * ocm_vae_scratch_bytes(B) bytes, zeroed once before first use).
 *
 * ocm_vae_bottleneck_fwd: z = μ + ε·exp(½·logσ²); kl_out = −½·mean_B Σ_d (1 + logσ² − μ² − exp(logσ²))
 *   (vae_model.py:150-152, reparameterize :124-126).  μ, logσ², ε, z [dev] B×d, B·d ≤ 2²⁰; scratch
 *   [dev] ocm_vae_bottleneck_scratch_bytes(), zero-filled once before first use (its counters are
 *   left zero).
 * ocm_vae_bottleneck_bwd: dμ = dz + dkl·μ/B, dlogσ² = dz·ε·½exp(½logσ²) − ½·dkl·(1 − exp(logσ²))/B
 *   (dz or dkl may be NULL: no gradient from that output).
 * ocm_vae_recon_fwd: x̂ = xs·std + mean (forward's de-standardisation, vae_model.py:130-134); kind
 *   OCM_VAE_LOSS_BCE: mean BCE-with-logits(x̂, clamp((x − min_x)/(max_x − min_x + eps), 0, 1)) per
 *   sample min / max (vae_model.py:153-156); OCM_VAE_LOSS_MSE: mean (x̂ − x)² (final_vaesimca.py:208);
 *   out2 [dev] {recon + β·kl, recon} (kl [dev] nullable: 0); gxs_out [dev] B×L f32 = d recon / d xs.
 * ocm_vae_recon_bwd: dxs = dtotal·gxs (n values, written in dtype), dkl_out = β·dtotal (nullable).
 * ocm_adam_step: torch.optim.Adam (L2 weight_decay, no amsgrad) over `ntensors` tensors of
 *   `table` [dev] (offsets: prefix of numel, total = Σ numel); step [dev] f32 counter, advanced by
 *   one per call (bias corrections 1 − βᵗ); scratch [dev] ocm_vae_scratch_bytes(4096) bytes,
 *   zero-filled once (completion counters, left zero). */
#define OCM_VAE_LOSS_BCE 0
#define OCM_VAE_LOSS_MSE 1
typedef struct ocm_adam_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t offset;
  int64_t numel;
} ocm_adam_tensor;
size_t ocm_vae_scratch_bytes(int32_t B);
size_t ocm_vae_bottleneck_scratch_bytes(void);
int ocm_vae_bottleneck_fwd(ocm_ctx* ctx, int32_t dtype, const void* mu, const void* logvar, const void* eps, int32_t B,
                           int32_t d, void* z_out, float* kl_out, void* scratch, void* stream);
int ocm_vae_bottleneck_bwd(ocm_ctx* ctx, int32_t dtype, const void* dz, const float* dkl, const void* mu,
                           const void* logvar, const void* eps, int32_t B, int32_t d, void* dmu_out, void* dlogvar_out,
                           void* stream);
/* ocm_vae_bottleneck_fwd_ld / _bwd_ld (ABI 12): the same with μ, logσ² (and dμ, dlogσ²) as rows of stride
 * ld ≥ d — ld = 2d, logvar = mu + d: the packed B×2d output of one [fc_mu; fc_logvar] product
 * (vae_model.py:81-82), read and written in place; ε, z, dz stay B×d. */
int ocm_vae_bottleneck_fwd_ld(ocm_ctx* ctx, int32_t dtype, const void* mu, const void* logvar, int32_t ld,
                              const void* eps, int32_t B, int32_t d, void* z_out, float* kl_out, void* scratch,
                              void* stream);
int ocm_vae_bottleneck_bwd_ld(ocm_ctx* ctx, int32_t dtype, const void* dz, const float* dkl, const void* mu,
                              const void* logvar, int32_t ld, const void* eps, int32_t B, int32_t d, void* dmu_out,
                              void* dlogvar_out, void* stream);
int ocm_vae_recon_fwd(ocm_ctx* ctx, int32_t kind, const float* x, int32_t dtype, const void* xs, int32_t B, int32_t L,
                      const float* mean, const float* std, float eps, const float* kl, float beta, float* gxs_out,
                      float* out2, void* scratch, void* stream);
int ocm_vae_recon_bwd(ocm_ctx* ctx, const float* dtotal, const float* gxs, int64_t n, int32_t dtype, void* dxs_out,
                      float beta, float* dkl_out, void* stream);
int ocm_adam_step(ocm_ctx* ctx, const ocm_adam_tensor* table, int32_t ntensors, int64_t total, float* step, float lr,
                  float beta1, float beta2, float eps, float weight_decay, void* scratch, void* stream);
/* ocm_cast_multi: dst[k] = src[k] converted (float32 ↔ bfloat16, round to nearest even) for n ≤ 32
 *   tensors of numel[k] elements in one launch (src / dst / numel: HOST arrays of device pointers;
 *   the pointers travel as kernel arguments, so a captured graph replays them).  The VAE step casts
 *   its Linear weights to bf16 once per step, and their bf16 gradients back, in one launch each.
 * ocm_vae_standardise: out = (x − mean) / std per column of a B×L float32 batch, in dtype
 *   (vae_model.py:128-129 standardises the spectra before the encoder). */
int ocm_cast_multi(ocm_ctx* ctx, int32_t n, const void* const* src, int32_t src_dtype, void* const* dst,
                   int32_t dst_dtype, const int64_t* numel, void* stream);
int ocm_vae_standardise(ocm_ctx* ctx, const float* x, int32_t B, int32_t L, const float* mean, const float* std_,
                        int32_t dtype, void* out, void* stream);
/* ocm_vae_act_bias_bwd (ABI 11): the backward tail of a bf16 Linear layer (vae_model.py:80-84):
 *   act 1 (Linear → ELU): gy_out = g · elu'(y), y the pre-activation (torch's elu_backward, float32
 *   arithmetic rounded to bf16), and gbias_out[c] = Σ_r gy[r, c] (float32 over the rounded values,
 *   rounded to bf16); act 0 (Linear alone): gbias_out = Σ_r g[r, c], y / gy_out unused.
 *   g, y, gy_out [dev] B×N bf16 row-major, N a multiple of 8, 16-byte aligned; gbias_out [dev] N bf16.
 *   One launch instead of torch's elu_backward and sum-reduction kernels. */
int ocm_vae_act_bias_bwd(ocm_ctx* ctx, int32_t act, const void* g, const void* y, int32_t B, int32_t N, void* gy_out,
                         void* gbias_out, void* stream);
/* ocm_vae_linear_act (ABI 12): y = x·Wᵀ + b (bf16, float32 accumulation, rounded to bf16) and a = ELU(y) of
 * the rounded y (torch's expm1 form) in one launch, for the bottleneck's short-K Linear + ELU layers
 * (vae_model.py:83-84).  x M×K, W N×K, bias N (nullable), y_out / a_out M×N, all bf16 and row-major;
 * M, N multiples of 64, K ∈ {32, 64, 128, 256}; x and W 16-byte aligned. */
int ocm_vae_linear_act(ocm_ctx* ctx, const void* x, const void* W, const void* bias, int32_t M, int32_t N, int32_t K,
                       void* y_out, void* a_out, void* stream);
/* ocm_gemm_bf16_sk (ABI 11): C = A·B (+ bias) in bf16 with float32 accumulation, for the VAE bottleneck's
 *   long-K products (vae_model.py:80-84: fc[0]'s forward, fc_dec[3]'s input gradient), split over K in
 *   256-deep chunks: A [dev] M×K row-major; B [dev] N×K row-major when b_nk (a Linear weight, C = A·Bᵀ),
 *   else K×N row-major; bias [dev] N bf16 or NULL; C [dev] M×N row-major.  M, N multiples of 64, K of 256,
 *   16-byte aligned.  scratch [dev] ocm_gemm_bf16_sk_scratch_bytes(M, N, K) bytes (caller-owned, so a
 *   captured graph keeps it): float32 partial tiles, summed in chunk order by the second launch. */
size_t ocm_gemm_bf16_sk_scratch_bytes(int32_t M, int32_t N, int32_t K);
int ocm_gemm_bf16_sk(ocm_ctx* ctx, int32_t b_nk, const void* A, const void* B, const void* bias, int32_t M, int32_t N,
                     int32_t K, void* C, void* scratch, void* stream);

/* ---- images into objects (appended; the ABI version stays 12) ----
 * The objects of the data sets come out of an (H, W, p) image (nut_data.py:64-70, 131-144): the band
 * mean thresholded into a foreground mask, its connected components, and each component's pixel rows.
 *
 * ocm_fgmask_f32 / _f64: one read-only pass over the m = H·W pixel rows of X [dev] (any ldx ≥ p, any
 *   element alignment; 16-byte loads per lane where the base and ldx allow, a scalar tail for p % 4):
 *   mean_r = (fp64 sum of row r in a fixed order) / p, mask_out[r] = !(mean_r < threshold), the
 *   reference's ~(mean < thr): a NaN pixel is foreground.  mask_out [dev] m bytes (0 / 1); mean_out
 *   [dev] m doubles or NULL.  m = 0 is a no-op; OCM_ERR_ARG for m ≥ 2^33.
 *
 * ocm_label_u8: connected components of mask [dev] (H × W bytes, non-zero = foreground) with
 *   connectivity 4 or 8.  labels_out [dev] H × W int32: 0 background, 1..n the components numbered by
 *   their first pixel in raster order (scipy.ndimage.label's numbering, bit for bit); n_out [dev] one
 *   int32 = n.  A component's representative is its smallest linear pixel index and its label 1 + the
 *   rank of that index among the representatives, so the result does not depend on scheduling.
 *   Union–find in six launches whatever the image holds: tiles labelled in LDS, tile borders united
 *   with device-scope atomicMin alone (no workgroup waits for another), flatten, and a three-launch
 *   prefix sum of the representative flags.  No host synchronisation.  Workspace: (H·W + H·W/1024 + 1)
 *   int32.  OCM_ERR_ARG, before any pointer is looked at, for connectivity other than 4 or 8, H or
 *   W < 1, or H·W > 2^31 − 1.
 *
 * ocm_gather_rows_f32 / _f64: out[i·ldo + j] = X[rows[i]·ldx + j] for i < n, j < p, bit for bit
 *   (NaN payloads included).  rows [dev] n int64, NOT checked here (as in every entry that takes
 *   `rows`).  16-byte copies per lane where X, out, ldx, ldo and p allow, element copies otherwise.
 *   n = 0 is a no-op; OCM_ERR_ARG for n ≥ 2^33. */
int ocm_fgmask_f32(ocm_ctx* ctx, const float* X, int64_t ldx, int64_t m, int32_t p, double threshold,
                   uint8_t* mask_out, double* mean_out, void* stream);
int ocm_fgmask_f64(ocm_ctx* ctx, const double* X, int64_t ldx, int64_t m, int32_t p, double threshold,
                   uint8_t* mask_out, double* mean_out, void* stream);
int ocm_label_u8(ocm_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t connectivity, int32_t* labels_out,
                 int32_t* n_out, void* stream);
int ocm_gather_rows_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        float* out, int64_t ldo, void* stream);
int ocm_gather_rows_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        double* out, int64_t ldo, void* stream);

/* ---- PLS-DA (appended; the ABI version stays 12) ----
 * The discriminant baseline of data_cheese.py:193-328: PLSRegression(a) on the class target, then
 * LinearDiscriminantAnalysis on the PLS scores, for every a and every cross-validation fold.
 *
 * ocm_pls_fit_f64: the PLS recursion of `nprob` independent problems (the full fit and every fold) on
 *   their moments.  S [dev] nprob × p × p = XcᵀXc and s [dev] nprob × p × M = XcᵀYc of the centred,
 *   scaled training rows (neither is changed); 1 ≤ M ≤ 8, 1 ≤ A ≤ min(p, 64).  For a = 0..A−1:
 *   w = s (M = 1) or s·c with c the dominant eigenvector of sᵀs (cyclic Jacobi, fp64), scaled to unit
 *   norm with its largest-magnitude entry positive (sklearn's _svd_flip_1d);
 *   r = w − Σ_{j<a} (p_jᵀw) r_j;  v = S r;  tt = rᵀv;  p_a = v / tt;  q_a = sᵀr / tt;  s −= tt p_a q_aᵀ.
 *   W_out, R_out, P_out [dev] nprob × A × p; q_out [dev] nprob × A × M; tt_out [dev] nprob × A;
 *   ncomp_out [dev] nprob int32, the components completed: a problem stops at the first step where
 *   ‖s‖² ≤ 2⁻¹⁰⁰ ‖s₀‖² or tt ≤ 0 (sklearn's "y residual is constant") and its later rows are zeros.
 *   Two launches per component whatever nprob is, no workgroup waits for another, every sum in a fixed
 *   order (two calls give the same bits).  Workspace: nprob · (p · (3 + M) + 8) doubles, whatever A is.
 *
 * ocm_plsda_predict_f32: t = P (x − mu) for the m processed rows in one read of X (any p ≥ 1, any
 *   ldx ≥ p, optional `rows`), P [dev] k × p doubles, mu [dev] p doubles, 1 ≤ k ≤ 64: f32 MFMA
 *   products, f32 chains over 256 columns added up in fp64.  Then, for each of the nlv prefixes lvs[l]
 *   ([host] int32, ascending, 1 ≤ lvs[l] ≤ k, 0 ≤ nlv ≤ 64) and each class c < C (2 ≤ C ≤ 8),
 *   D[l][c] = Σ_{a<lvs[l]} coef[l][c][a] t_a + b[l][c] in fp64 and pred[l] = the lowest c at the maximum
 *   (np.argmax).  table [dev]: nlv × C × k coefficients, then nlv × C intercepts.  Outputs, each
 *   nullable: T_out [dev] m × k float32; D_out [dev] m × nlv × C float32; pred_out [dev] m × nlv
 *   uint8; counts_out [dev] nlv × C × C int64, counts[l][true][pred] over the rows whose y_true
 *   ([dev] m uint8 class indices) is < C (other rows count nowhere); counts_out needs y_true.
 *   nlv = 0 gives the scores alone.  m = 0 writes zero counts. */
int ocm_pls_fit_f64(ocm_ctx* ctx, const double* S, const double* s, int32_t nprob, int32_t p, int32_t M, int32_t A,
                    double* W_out, double* R_out, double* P_out, double* q_out, double* tt_out, int32_t* ncomp_out,
                    void* stream);
int ocm_plsda_predict_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                          const double* P, const double* mu, int32_t k, const int32_t* lvs, int32_t nlv, int32_t C,
                          const double* table, float* T_out, float* D_out, uint8_t* pred_out, const uint8_t* y_true,
                          int64_t* counts_out, void* stream);

/* ---- multi-class SIMCA (appended; the ABI version stays 12) ----
 * The reference's SIMCA is a multi-class estimator (model_class=None fits every class,
 * utils/SIMCA.py:27-59) whose predict loops over the classes and reads X once per class
 * (utils/SIMCA.py:120-145); data_cheese.py:193-328 reads its one-class results against PLS-DA on the
 * same rows.  ocm_score_multi_f32 scores the m processed rows (all rows, or X[rows[r]]) against C class
 * models in one launch and ends in the class assignment.
 *   koff [host] C + 1 ascending offsets, koff[0] = 0: class c owns the stacked components
 *     koff[c] .. koff[c+1] − 1; K = koff[C].  1 ≤ C ≤ 8, every k_c in [1, p], K ≤ 64 (else OCM_ERR_ARG).
 *   P [dev] K × p float64, each class's rows orthonormal; mu [dev] C × p float64; a_diag [dev] K float64
 *     (1/λ); dec [host] C ocm_decision, one per class.  Any p ≥ 1, any ldx ≥ p, no alignment requirement.
 * Per processed row and class c, with y = x − μ_c and t = P_c·y:
 *   Q_c = ‖y − P_cᵀt‖² (the explicit residual, f32), T²_c = Σ t²·a (fp64), dred_c as ocm_decide forms it
 *   from T²_c and the float32 Q_c, accept_c = dred_c < dlim_c, ratio_c = dred_c / dlim_c (fp64).
 *   naccept = the number of accepting classes; nearest = the lowest c at the smallest ratio_c over all
 *   classes (a NaN ratio counts as +inf; all NaN: 0); index = the lowest accepting c at the smallest
 *   ratio_c among the accepting classes, −1 when none accepts.
 * Outputs [dev], every one nullable: T2_out m × C float64, Q_out m × C float32, ratio_out m × C float64,
 *   accept_out[r·accept_stride + c] = 1.0 / 0.0 (accept_stride ≥ C: predict's matrix), index_out m int8,
 *   nearest_out and naccept_out m uint8, counts_out (C + 1)·(3C + 2) int64, which needs y_true [dev]
 *   (m uint8 class indices; a value ≥ C is the row "other" = C) and holds three blocks in this order:
 *   table[C+1][C+1] ([true][index, column C = none]), acc[C+1][C] ([true][class] accepted) and
 *   hist[C+1][C+1] ([true][naccept]).  m = 0 writes zero counts.
 * Numerics: f32 MFMA products; t in f32 chains over 64 columns flushed to fp64; the mean as a float pair
 *   (hi + lo); the residual in f32; T², dred and ratio in fp64.  The counts are integer sums (64-bit
 *   integer atomics, no floating-point atomics): two launches on one input give the same bytes in every
 *   output.  X is read from HBM once for all classes where a 16-row tile fits half a CU's LDS beside the
 *   kernel's static arrays (p ≤ ≈ 1100); for wider rows the later sweeps read the tile again through the
 *   cache hierarchy.  Workspace: (K + 2C)·p floats. */
int ocm_score_multi_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                        const double* P, const double* mu, const double* a_diag, const int32_t* koff, int32_t C,
                        const ocm_decision* dec, double* T2_out, float* Q_out, double* ratio_out,
                        double* accept_out, int64_t accept_stride, int8_t* index_out, uint8_t* nearest_out,
                        uint8_t* naccept_out, const uint8_t* y_true, int64_t* counts_out, void* stream);

/* ---- ROC AUC, ROC points and a keys-only sort (appended; the ABI version stays 12) ----
 * The reference scores a trial without a threshold: roc_auc_score(labels_true, f_all)
 * (optim_bce_nuts.py:241,279).  These entries turn scores that are already on the device into the exact
 * AUC, into points of the ROC curve, or into their sorted copy.
 *
 * Every value input takes dtype 0 = float64 or 1 = float32 and is addressed in elements as
 *   S[c·col_stride + r·row_stride]   (c < ncol, r < m; strides ≥ 0),
 * so an (m, C) matrix and a (ncfg, m) table are both read in place.  m, n < 2^31.
 *
 * ocm_roc_tile_keys: the keys one workgroup ranks per sort tile.
 *
 * ocm_sort_f: out [dev] ncol × n contiguous, same dtype: the ascending sorted copy of each column, keys
 *   only.  The order is that of the okey64 / okey32 keys of ocm_percentile (−0.0 before +0.0); NaNs go
 *   last, as in np.sort, and come out as one canonical NaN.  n = 0 is a no-op.
 *
 * ocm_auc: positive [dev] m bytes (non-zero = positive), shared by the columns.  u2_out [dev] ncol
 *   uint64: u2 = Σ over (positive i, negative j) of 2·[s_i > s_j] + [s_i == s_j], compared by value
 *   (−0.0 == +0.0, ±inf in order, a float32 score as its exact double), so AUC = u2 / (2·P·N), the
 *   trapezoid AUC with scikit-learn's tie rule.  np_out [dev] 2 int64 {P, N} (every row counts, NaN or
 *   not).  nnan_out [dev, nullable] ncol int64: the NaN scores of each column; those rows are left out of
 *   that column's u2.  m = 0, P = 0 or N = 0 give u2 = 0 and success.
 *
 * ocm_roc_counts: thr [dev] ncol × K float64, ascending per column, 1 ≤ K ≤ 4096 (else OCM_ERR_ARG);
 *   cnt_out [dev] ncol × K × 2 uint64: {positives with s ≥ thr, negatives with s ≥ thr}, the same value
 *   comparison; a NaN score counts nowhere.  ncol ≤ 65535.  Workspace: ncol · 2 · (K + 1) uint64.
 *
 * ocm_roc_last_passes: the radix passes the calling thread's last ocm_sort_f / ocm_auc executed (the most
 *   over its column groups), out of 8 (float64) or 4 (float32).
 *
 * How: ocm_auc sorts the keys of the smaller class only (no payload), folding −0.0 into +0.0; each row of
 *   the other class is read from S through the mask and finds lt = #keys < s and le = #keys ≤ s in the
 *   sorted side by binary searches with no branch on the data (bucket splitters in LDS, then inside one
 *   bucket; le by two probes behind lt, by a second search only in a wave that meets a longer run of equal
 *   keys): with the negatives sorted it adds 2·lt + (le − lt), with the positives sorted
 *   2·(P − le) + (le − lt).  64-bit integer sums, one integer atomic per workgroup.  The sort is an LSD
 *   radix sort on 8-bit digits: one read histograms every digit position of every column, a position
 *   whose digit is the same for all keys of a column is skipped for that column, and an executed pass is
 *   three launches (tile histograms, a scan over (digit, tile), a stable scatter ranked by 64-bit
 *   __ballot masks); the first executed pass gathers the sorted class out of S.  No workgroup waits for
 *   another, no floating-point atomics: every output is an integer or a permutation of its input, and
 *   two calls on one input give the same bytes.  Columns are a grid dimension.  Both entries wait for
 *   the stream (ocm_auc twice, ocm_sort_f once per column group) to read the class sizes and the passes
 *   to run.
 * Workspace of ocm_sort_f and ocm_auc, per column of a group, with n_s the keys sorted (n, or the smaller
 *   class) and b the key bytes (8 or 4): 2·n_s·b + (⌈m/2048⌉ + b)·1 KiB + 24 bytes, and 32 KiB more for
 *   ocm_auc (the last key of each of ≤ 32 KiB / b buckets of the sorted side, which its search keeps in
 *   LDS so that only the steps inside one bucket go to memory).  Columns are processed
 *   in groups of ⌊2^26 / max(n_s, m/8)⌋ (at least one, at most 65535), which keeps a group's workspace
 *   near 1 GiB. */
int ocm_roc_tile_keys(void);
int ocm_roc_last_passes(void);
int ocm_sort_f(ocm_ctx* ctx, const void* v, int32_t dtype, int64_t n, int64_t ncol, int64_t col_stride,
               int64_t row_stride, void* out, void* stream);
int ocm_auc(ocm_ctx* ctx, const void* S, int32_t dtype, int64_t m, int64_t ncol, int64_t col_stride,
            int64_t row_stride, const uint8_t* positive, uint64_t* u2_out, int64_t* np_out, int64_t* nnan_out,
            void* stream);
int ocm_roc_counts(ocm_ctx* ctx, const void* S, int32_t dtype, int64_t m, int64_t ncol, int64_t col_stride,
                   int64_t row_stride, const uint8_t* positive, const double* thr, int32_t K, uint64_t* cnt_out,
                   void* stream);

/* ---- sample selection: Kennard–Stone and Duplex (appended; the ABI version stays 12) ----
 * Choosing the calibration rows in place of a random train_test_split (simca_nuts.py:73-74,
 * utils/data_utils.py): Kennard & Stone's max–min selection and Snee's Duplex, on a coordinate matrix
 * Z [dev] n × q (float32 or float64, ldz ≥ q, read in place, every value taken as its exact double).
 *   d2(i, j) = Σ_c w_c (z_ic − z_jc)²  in fp64, in the difference form (never |a|² + |b|² − 2a·b),
 *   c ascending: t = z_ic − z_jc, acc = fma(w_c·t, t, acc).  w [dev] q doubles ≥ 0, NULL: all 1
 *   (pass 1/λ for a Mahalanobis distance on PCA scores).  Every kernel forms d2 this one way, so a
 *   distance has the same bits in every entry and on both selection paths; plain fp64 VALU (the work
 *   is bound by launches and cache latency, not FLOPs).
 * Candidates compare under one total order (value descending, then i ascending, then j ascending) at
 * every level, so no result depends on tile shape or grid size, and two calls give the same bytes.
 * A row with a non-finite coordinate is an argument error of the caller: the kernels count such rows
 * into nbad_out [dev] one int32 (required) and the other outputs are then unspecified (ocm_ks_select:
 * left untouched).  Everything is ordered on `stream`; no entry waits for the device (but a workspace
 * that has to grow drains the stream first: ocm_ctx_reserve pre-sizes it).  No workgroup waits for
 * another, no cooperative launch, no fences; the only atomic is the bad-row count.
 *
 * ocm_ks_pair_f32 / _f64: the farthest pair.  (i*, j*) = argmax of d2 over i < j among the rows with
 *   skip[i] == 0 (skip [dev] n bytes, NULL: none), ties to the smallest i, then the smallest j;
 *   pair_out [dev] 2 int64, d2_out [dev] one double ({−1, −1} and NaN when fewer than two rows are
 *   left).  One workgroup per pair of 128-row tiles of the upper triangle, both panels staged through
 *   LDS in 16-column chunks (any q), one partial per workgroup, then reduction launches of 4096
 *   partials per workgroup.  n ≥ 2.  OCM_ERR_ARG when the tile pairs exceed the grid limit (n above
 *   ≈ 8.3M).  Workspace: 24 bytes per tile pair.
 *
 * ocm_ks_nearest_f32 / _f64: idx_out [dev] one int64 = argmin_i Σ_c w_c (z_ic − center_c)², ties to the
 *   smallest i, and d2_out that value (center [dev] q doubles: the column mean for the "mean" start).
 *
 * ocm_ks_select_f32 / _f64: all steps of Kennard–Stone (n_b = 0) or Duplex (n_b > 0) after the starts.
 *   start_a [dev] n_start_a ≥ 1 distinct rows (and start_b, n_start_b for Duplex; the two lists
 *   disjoint): order_a [dev] n_a int64 begins with them and their d2_a [dev] n_a doubles is NaN.
 *   Step: m_i = min over the set's members s of d2(i, s); the next member is the argmax of m_i over the
 *   rows in no set, ties to the smallest i (m = 0 is a valid maximum: selection runs on through
 *   duplicates), and its d2 entry is that m.  Duplex: the sets take turns, A first, each by the
 *   distance to its own members; a full set is skipped.  n_a + n_b ≤ n.  A start index outside [0, n)
 *   adds 2^30 to nbad_out and nothing is written.
 *   path 0 auto, 1 small, 2 wide (tests force each).  small: one workgroup, the min distances (and Z,
 *   when it fits beside them) in LDS, all steps in one launch, one barrier per step; OCM_ERR_ARG when
 *   the min distances alone exceed the LDS.  wide: one launch per pick; each workgroup reduces the
 *   previous launch's ≤ 1024 partials itself, applies that pick to its rows and writes its partial to
 *   the other half of a ping-pong buffer; a last small launch records the final pick and the starts.
 *   Workspace (wide): 8 bytes per row and set, and 48 KiB. */
int ocm_ks_pair_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                    const uint8_t* skip, int64_t* pair_out, double* d2_out, int32_t* nbad_out, void* stream);
int ocm_ks_pair_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                    const uint8_t* skip, int64_t* pair_out, double* d2_out, int32_t* nbad_out, void* stream);
int ocm_ks_nearest_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                       const double* center, int64_t* idx_out, double* d2_out, int32_t* nbad_out, void* stream);
int ocm_ks_nearest_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                       const double* center, int64_t* idx_out, double* d2_out, int32_t* nbad_out, void* stream);
int ocm_ks_select_f32(ocm_ctx* ctx, const float* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                      const int64_t* start_a, int64_t n_start_a, int64_t n_a, const int64_t* start_b,
                      int64_t n_start_b, int64_t n_b, int64_t* order_a, double* d2_a, int64_t* order_b, double* d2_b,
                      int32_t* nbad_out, int32_t path, void* stream);
int ocm_ks_select_f64(ocm_ctx* ctx, const double* Z, int64_t ldz, int64_t n, int32_t q, const double* w,
                      const int64_t* start_a, int64_t n_start_a, int64_t n_a, const int64_t* start_b,
                      int64_t n_start_b, int64_t n_b, int64_t* order_a, double* d2_a, int64_t* order_b, double* d2_b,
                      int32_t* nbad_out, int32_t path, void* stream);

/* ---- mask morphology (appended; the ABI version stays 12) ----
 * Eroding, dilating and measuring the object masks of "images into objects" before their spectra are
 * read: the outer pixels of an object mix it with the belt, a specular hole inside it is lost.  One
 * primitive gives all of it, the exact Euclidean distance transform of the mask:
 *   d2(y, x) = min over the background pixels (y', x') of (y − y')² + (x − x')²,  0 on background.
 * Erosion by the disc {dx² + dy² ≤ r2} is d2 > r2 (scipy.ndimage.binary_erosion, bit for bit), dilation
 * the same on the complement, opening and closing two such calls, the depth of a pixel √d2.
 *
 * ocm_edt_u8: mask [dev] H × W bytes, non-zero = foreground.  d2_out [dev] H × W int32 or NULL;
 *   mask_out [dev] H × W bytes (0 / 1) or NULL, mask_out = d2 > r2; at least one of the two.  mask_out
 *   may alias nothing.  flags:
 *     OCM_EDT_BORDER_BG   the pixels just outside the image are background (binary_erosion's
 *                         border_value = 0); without it only the image's own pixels count;
 *     OCM_EDT_INVERT_IN   zero bytes are the foreground: distances to the nearest non-zero pixel;
 *     OCM_EDT_INVERT_OUT  mask_out = !(d2 > r2).
 *   Without any background (and without BORDER_BG) every d2 is OCM_EDT_NONE, which mask_out takes as
 *   greater than any r2.  Integer arithmetic alone: two calls give the same bytes.  Three launches,
 *   whatever the image holds: (1) the background bits of every column packed 64 rows to a word, 4 mask
 *   bytes per lane where W and the pointer allow, single bytes otherwise; (2) g(y, x), the vertical
 *   distance to the nearest background pixel of column x, from those words by count-leading / -trailing-
 *   zeros (no sweep along H: one thread per column and 64-row band), uint16 with 65535 for "none in this
 *   column"; (3) one workgroup per row: the row's g staged in LDS (2 bytes per pixel and the minimum of
 *   every 64-column segment), d2 = min over x' of (x − x')² + g(y, x')² by a scan outwards from x that
 *   stops once (x − x')² ≥ the best so far and skips a segment whose minimum cannot improve it.  Exact;
 *   O(H·W·min(R, W)) for objects of radius R.  No atomics, no host synchronisation, no workgroup waits
 *   for another.  Workspace: 2 bytes per pixel and 8 bytes per column and 64 rows.  OCM_ERR_ARG, before
 *   any pointer is looked at, for H or W < 1, H or W > 32767 (H² + W² stays below 2^31), unknown flag
 *   bits, r2 < 0 or both outputs NULL. */
#define OCM_EDT_BORDER_BG 1
#define OCM_EDT_INVERT_IN 2
#define OCM_EDT_INVERT_OUT 4
#define OCM_EDT_NONE 0x7fffffff
int ocm_edt_u8(ocm_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t flags, int64_t r2, int32_t* d2_out,
               uint8_t* mask_out, void* stream);

/* ---- robust calibration: the spatial median and sphered rows ----------------------------------------
 * The L1 (spatial) median of the n rows x_i = X[rows ? rows[i] : i] minimises Σ_i ‖x_i − m‖.  It is found
 * by Weiszfeld's iteration with the Vardi–Zhang correction for rows that coincide with the centre.  One
 * step from the centre m, every difference, product and sum in fp64:
 *   d_i = ‖x_i − m‖;  the η rows with d_i == 0 (exactly) take no part in the sums;
 *   W = Σ 1/d_i,  S = Σ x_i/d_i  (p column sums),  T̃ = S/W,  R = S − W·m,  r = ‖R‖;
 *   γ = 0 when η = 0, otherwise min(1, η/r) (1 when r = 0);
 *   m⁺ = (1 − γ)·T̃ + γ·m  (m itself, bit for bit, when γ = 1);
 *   stop when ‖m⁺ − m‖ ≤ tol·‖m⁺‖ or after max_iter steps.
 *
 * ocm_l1median_f32 / _f64: X [dev] with row pitch ldx ≥ p; rows [dev] n int64 row indices or NULL (rows
 *   0..n − 1); center [dev] p doubles, in: the start, out: the result; dist_out [dev] n doubles or NULL:
 *   the distances to the returned centre; info_out [dev] OCM_L1_INFO doubles: steps done, converged
 *   (0 / 1), the last step's length ‖m⁺ − m‖, the objective Σ d_i and the number of coincident rows,
 *   the last two at the returned centre.  max_iter = 0 evaluates the start.  Nothing is read back:
 *   every step is queued at once and a step that finds the done flag raised returns at its first
 *   instruction.  A step is k_l1_part, one workgroup per chunk of 256 rows at multiples of 256, which
 *   writes the chunk's p + 3 partials (S, W, Σd, η) with the rows added in row order, then (more than
 *   64 chunks) k_l1_group, which adds each aligned group of 64 chunks in chunk order, then k_l1_update,
 *   one workgroup, which adds the groups in order and forms the update.  A row is used twice in a step,
 *   for its distance and for the weighted sums: 16 rows at a time wait in LDS in between where
 *   16·p·sizeof(element) ≤ 128 KiB (p ≤ 2048 float32, 1024 float64), and are read a second time, out of
 *   L2, where p is wider.  One more pass measures the distances to the returned centre.  No atomics, no
 *   fences, no workgroup waits for another: the result is a function of (X, rows, start, tol, max_iter)
 *   alone, bit for bit.  16-byte loads where p, ldx and the base allow them, 8-byte or single-element
 *   loads otherwise.  Workspace: (chunks + groups + 1)·(p + 3) + 8 doubles.  OCM_ERR_ARG for n < 1, n ≥ 2^31,
 *   p < 1, ldx < p, tol < 0 (or NaN), max_iter < 0 or > 100000.  The row indices are not checked.
 *
 * ocm_sphere_rows_f32 / _f64: U[i·ldu + j] = (x_ij − center_j)/‖x_i − center‖ computed in fp64 and
 *   rounded once to the element type; a row at distance 0 gives zeros.  dist_out [dev] n doubles or
 *   NULL.  One wave per row; the row's second read comes out of the cache the first one filled.  U may
 *   not overlap X. */
#define OCM_L1_INFO 5
int ocm_l1median_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                     double* center, double tol, int32_t max_iter, double* dist_out, double* info_out, void* stream);
int ocm_l1median_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                     double* center, double tol, int32_t max_iter, double* dist_out, double* info_out, void* stream);
int ocm_sphere_rows_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        const double* center, float* U, int64_t ldu, double* dist_out, void* stream);
int ocm_sphere_rows_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t n, int32_t p,
                        const double* center, double* U, int64_t ldu, double* dist_out, void* stream);

/* ---- cross-validation of the PCA itself: PRESS of every number of components ----
 * Element-wise k-fold cross-validation (Bro, Kjeldahl, Smilde, Kiers 2008): for a model (μ, P) fitted
 * without the rows given here, with y = x − μ, t = P·y, the residual r⁽ᵏ⁾ = y − Σ_{a≤k} t_a·P_a and the
 * leverage h_j⁽ᵏ⁾ = Σ_{a≤k} P_aj² (r⁽⁰⁾ = y, h⁽⁰⁾ = 0), variable j predicted from the other p − 1
 * variables through the loadings misses by exactly r_j⁽ᵏ⁾/(1 − h_j⁽ᵏ⁾), so
 *   press_out[k] = Σ_rows Σ_j (r_j⁽ᵏ⁾/(1 − h_j⁽ᵏ⁾))²      k = 0..K
 *   naive_out[k] = Σ_rows Σ_j (r_j⁽ᵏ⁾)²                   the row-wise curve (Σ Q at k components)
 * Degenerate rule: where 1 − h_j⁽ᵏ⁾ ≤ 1e-8 the model reproduces variable j by itself and its leave-out
 *   prediction is undefined: the variable is left out of press_out[k] (weight 0; naive_out keeps it)
 *   and counted in ndegen_out[k].
 * X [dev] with row pitch ldx ≥ p; rows [dev, nullable] m int64 row indices (NULL: rows 0..m − 1, not
 *   checked); P [dev] K×p doubles with orthonormal rows, mu [dev] p doubles; press_out [dev] K + 1
 *   doubles; naive_out [dev, nullable] K + 1 doubles; ndegen_out [dev, nullable] K + 1 int32.
 * 1 ≤ K ≤ min(p, 64), p ≥ 2, m ≥ 0 (m = 0 writes zeros; ndegen_out is still filled), OCM_ERR_ARG
 *   otherwise.  No alignment requirement (16-byte loads where p, ldx and the base allow them).
 * One read of the rows: a tile of 16 centred rows waits in LDS between the projection and the residual
 *   updates where 16·p elements fit once per resident workgroup (float32, two workgroups per CU:
 *   p ≤ 1088 / 896 / 768 / 576 at K ≤ 16 / 32 / 48 / 64; float64, one per CU: p ≤ 1152 / 1088 / 960 /
 *   896); wider rows are read a second time, out of L2.  f32: t on f32 MFMA over ≤ 64 columns per chain
 *   flushed to f64, the residual explicit in f32 (r ← r − t_k·P_k); f64: fp64 MFMA and fp64 residual.
 *   The weights 1/(1 − h)² are formed in fp64.  In float32 a variable with h_j close to 1 is
 *   ill-conditioned short of the degenerate rule: the relative error of its term grows like
 *   2⁻²⁴·|y_j|/|r_j|; give such data as float64.
 * Sums: a lane adds its 64-column block sums in the element type, over one tile or (float32, K ≤ 32)
 *   over the tiles of its chunk up to 128 block sums; then fp64: wave, workgroup, the tiles of a chunk
 *   of 256 rows (at multiples of 256) in tile order, then the chunks in chunk order.  No atomics, no
 *   workgroup waits for another: two launches on one input give the same bits.  Workspace:
 *   (K + 1)·p weights, (f32) K·p + p floats, chunks·2·(K + 1) doubles. */
int ocm_press_f32(ocm_ctx* ctx, const float* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                  const double* P, const double* mu, int32_t K, double* press_out, double* naive_out,
                  int32_t* ndegen_out, void* stream);
int ocm_press_f64(ocm_ctx* ctx, const double* X, int64_t ldx, const int64_t* rows, int64_t m, int32_t p,
                  const double* P, const double* mu, int32_t K, double* press_out, double* naive_out,
                  int32_t* ndegen_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* OCM_H_ */
