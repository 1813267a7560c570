// The host-side planning of ocm_eig_topk (ocm_linalg.hip): which of the four
// solver paths a (p, k) takes and every count derived from it, the layout of
// the workspace, the schedule of the Rayleigh–Ritz tests and the buffer
// rotation of a Chebyshev filter segment.  Plain C++17 with no HIP headers:
// tests/test_eig_plan.py compiles it into a stand-alone g++ program.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>

namespace ocm_eig {

constexpr int JMAX = 64;           // widest one-workgroup Jacobi: p ≤ JMAX is solved directly, b ≤ JMAX on the device
constexpr int QB = 32;             // block width of the fused kernels (k_cq_*32, k_cv32, k_cvq32, k_rr_*32)
constexpr int DT = 64;             // k_dgemm's tile
constexpr int CQ_G = 16;           // workgroups per CholQR launch (a power of two: the ticket wraps)
constexpr int CVQ_G1 = 16;         // k_cvq32: row blocks per Gram group
constexpr int TICKET_STRIDE = 32;  // words between two arrival counters: one per 128-B line
constexpr int PLAIN = 4;           // plain iterations before the first Rayleigh–Ritz test

// ---------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------
enum class Path {
  small,    // p ≤ JMAX: one Jacobi on C itself
  fused32,  // b = 32: the k_cvq32 chain, Chebyshev segments, three-stream Rayleigh–Ritz
  block,    // b = 48 / 64: split-K dgemm, k_atb_part, k_chol, k_trsm_rows, k_jacobi_blk
  wide,     // b > 64: the b×b steps on the host
};

struct Plan {
  Path path;
  int p, k, theta_mode;
  int b;               // block width: k plus oversampling (0 on the small path)
  bool ok;             // b ≥ k and b ≥ 16 (always, for 1 ≤ k ≤ p; the driver refuses otherwise)
  size_t pb, bb;       // p·b, b·b
  int ksplit;          // split-K planes of C·V (block, wide)
  int nblk;            // k_atb_part's 64-row blocks
  int cv_rb;           // k_cv32 / k_cvq32 row blocks (16 rows)
  int cvq_ng;          // k_cvq32's Gram groups
  int gt_words;        // k_cvq32's two-level counters, in words
  int nzero_cv;        // words from cv_ticket on that the first k_randn launch zeroes
  size_t def_blocks;   // tiles of the deflation GEMM
  size_t plane_cap;    // split-K planes, in doubles
  size_t host_doubles;  // pinned staging: θ and residuals (2b), wide: + two b×b matrices and b values
  bool fused() const { return path == Path::fused32; }
  bool wide() const { return path == Path::wide; }
};

inline Plan make_plan(int p, int k, int theta_mode) {
  Plan pl{};
  pl.p = p;
  pl.k = k;
  pl.theta_mode = theta_mode;
  if (p <= JMAX) {
    pl.path = Path::small;
    pl.ok = true;
    return pl;
  }
  // block size: k plus oversampling, a multiple of 16, ≤ p
  int b = ((k + std::max(8, k / 2)) + 15) / 16 * 16;
  b = std::max(b, 32);
  if (k <= JMAX && b > JMAX) b = JMAX;
  if (b > p) b = std::max(k, (p / 16) * 16);
  pl.b = b;
  pl.ok = b >= k && b >= 16;
  pl.path = b > JMAX ? Path::wide : b == QB ? Path::fused32 : Path::block;
  pl.pb = (size_t)p * b;
  pl.bb = (size_t)b * b;
  pl.ksplit = std::max(1, std::min(16, (int)(256 / std::max(1, ((p + 63) / 64) * ((b + 63) / 64)))));
  pl.nblk = (p + 63) / 64;
  pl.cv_rb = (p + 15) / 16;
  pl.cvq_ng = (pl.cv_rb + CVQ_G1 - 1) / CVQ_G1;
  pl.gt_words = (1 + pl.cvq_ng) * TICKET_STRIDE;
  // fused: k_cv32's parity tickets, the gap to the next TICKET_STRIDE boundary, k_cvq32's counters
  pl.nzero_cv = pl.fused() ? (pl.cv_rb + TICKET_STRIDE - 1) / TICKET_STRIDE * TICKET_STRIDE + pl.gt_words : pl.cv_rb;
  pl.def_blocks = (size_t)((p + DT - 1) / DT) * ((p + DT - 1) / DT);
  pl.plane_cap = std::max((size_t)pl.ksplit * pl.pb, pl.wide() ? 16 * pl.bb : (size_t)0);
  pl.host_doubles = pl.wide() ? 3 * pl.bb + b : 2 * (size_t)b;
  return pl;
}

// ---------------------------------------------------------------------------
// the workspace
// ---------------------------------------------------------------------------
// A buffer a path does not use is null.
struct Layout {
  double *V, *W, *T1, *T2;   // p×b blocks
  double *H, *Z, *S, *L;     // b×b (small: Z is p×p)
  double* theta;             // θ (b), then the residuals (b): one read-back (small: the p eigenvalues)
  double* planes;            // split-K planes (block, wide)
  double* apart;             // k_atb_part's partials (block)
  double *cq_part, *cq_M;    // fused: CholQR / k_atb32 partials, the factors M1 / M2
  unsigned* cq_ticket;       // k_cq_gram32's ticket (counts from a multiple of CQ_G)
  double* cv_part;           // fused: k_cv32's partials
  unsigned *cv_ticket, *gtick;  // k_cv32's parity tickets (start even); fused: k_cvq32's counters
  double *Wa, *Wb, *Mf, *gpart, *Sb;  // fused: the chain's blocks and factors, Gram partials, two deferred Grams
  double *dpart, *Ud, *Wd;   // θ: the deflation GEMM's tile partials and its rank-2kd operands
  double* tr3;               // θ on the fused path: the block's three traces
};

// Carves every buffer out of cv (ocm::Carve: each starts on a 256-byte
// boundary).  The driver runs it twice: on a null base, after which cv.off
// is the size to ask ocm::workspace for, and on the workspace itself.
// The bytes of a buffer that a path does not use stay reserved (`unless`):
// every buffer then sits at the offset it has had since the paths shared one
// layout.  Without the fused path's 4 MB of planes, at p = 2048, the solve
// measured 0.3 to 1.7 % slower in two A/B runs (profiles/eig_driver_split_ab.json);
// closing the gaps wants that measurement repeated first.
template <class Carver>
Layout carve(const Plan& pl, Carver& cv) {
  Layout w{};
  if (pl.path == Path::small) {
    w.theta = cv.template take<double>((size_t)pl.p);
    w.Z = cv.template take<double>((size_t)pl.p * pl.p);
    return w;
  }
  const bool fused = pl.fused(), block = pl.path == Path::block, theta = pl.theta_mode != 0;
  auto unless = [](bool unused, double* q) { return unused ? nullptr : q; };
  const size_t pb = pl.pb, bb = pl.bb;
  w.V = cv.template take<double>(pb);
  w.W = cv.template take<double>(pb);
  w.T1 = cv.template take<double>(pb);
  w.T2 = cv.template take<double>(pb);
  w.H = cv.template take<double>(bb);
  w.Z = cv.template take<double>(bb);
  w.S = cv.template take<double>(bb);
  w.L = cv.template take<double>(bb);
  w.theta = cv.template take<double>(2 * (size_t)pl.b);
  w.planes = unless(fused, cv.template take<double>(pl.plane_cap));
  if (!pl.wide()) w.apart = unless(!block, cv.template take<double>((size_t)pl.nblk * bb));
  w.cq_part = unless(!fused, cv.template take<double>((size_t)CQ_G * 1024));
  w.cq_M = unless(!fused, cv.template take<double>(2048));
  // the first k_randn launch zeroes the ticket's first word
  w.cq_ticket = cv.template take<unsigned>(64);
  w.cv_part = unless(!fused, cv.template take<double>((size_t)pl.cv_rb * 2 * 512));
  // cv_ticket … gtick + gt_words is one range of nzero_cv words, zeroed by
  // that same launch: cv_ticket starts on a 256-byte boundary, so gtick, the
  // next multiple of TICKET_STRIDE words after the cv_rb tickets, is on a
  // TICKET_STRIDE boundary (one counter per 128-B line)
  w.cv_ticket = cv.template take<unsigned>((size_t)pl.nzero_cv + (fused ? TICKET_STRIDE : 0));  // (+ a reserved line)
  if (fused && w.cv_ticket) w.gtick = w.cv_ticket + (pl.nzero_cv - pl.gt_words);
  if (fused) {
    w.Wa = cv.template take<double>(pb);
    w.Wb = cv.template take<double>(pb);
    w.Mf = cv.template take<double>(2048);
    w.gpart = cv.template take<double>((size_t)(pl.cv_rb + pl.cvq_ng) * 1024);
    w.Sb = cv.template take<double>(2 * 1056);  // (+ their flags)
  }
  // θ work buffers, carved up front: the fused path fills them during its
  // Rayleigh–Ritz step, on a side stream
  if (theta) {
    w.dpart = cv.template take<double>(2 * pl.def_blocks);
    w.Ud = cv.template take<double>((size_t)2 * pl.b * pl.p);
    w.Wd = cv.template take<double>((size_t)2 * pl.b * pl.p);
    if (fused) w.tr3 = cv.template take<double>(8);
  }
  return w;
}

// ---------------------------------------------------------------------------
// the Rayleigh–Ritz schedule
// ---------------------------------------------------------------------------
// A Rayleigh–Ritz step costs ~5 plain iterations, so the next one is
// scheduled where the residual is predicted to reach the tolerance: the max
// residual (that of Ritz pair k) shrinks by λ_{b+1}/λ_k per iteration,
// estimated by θ_b/θ_k (θ_b ≤ λ_b) and, from the second test on, by the
// measured decay since the last one, whichever is slower.  A short prediction
// costs one more test, a long one a few plain iterations past convergence;
// the stopping rule itself does not depend on it.

// largest Chebyshev degree whose amplification of λ_1, T_d(x1), stays ≤ 1e6
// (the block's condition before the segment's CholQR), at most 8
inline int cheb_degree_cap(double x1) {
  int d = 1;
  while (d < 8 && std::cosh((d + 1) * std::acosh(x1)) <= 1e6) ++d;
  return d;
}

struct Verdict {
  bool waited_out;  // a negative residual: the fused test gave up waiting for its operand S
  bool nan;
  bool converged;
  double rmax, target;
};

// h: the values read back from a test, θ (b, descending) then the residuals of the first k Ritz pairs
inline Verdict verdict(const double* h, int k, int b, double tol) {
  Verdict v{};
  for (int i = 0; i < k; ++i) v.waited_out |= h[b + i] < 0.0;
  for (int i = 0; i < k; ++i) v.rmax = std::max(v.rmax, h[b + i]);
  const double scale = std::fabs(h[0]);
  v.nan = !(v.rmax == v.rmax);
  v.target = tol * (scale > 0 ? scale : 1.0);
  v.converged = v.rmax <= v.target;
  return v;
}

struct Step {
  int next_rr;    // iteration of the next test: 1 … 64 ahead, ≤ max_iter
  bool use_cheb;  // Chebyshev-filtered iterations pay from here on
  int dmax;       // their degree cap
};

struct Schedule {
  int prev_it = 0;          // the last failed test …
  double prev_rmax = 0.0;   // … and its max residual
  bool cheb_prev = false;   // the interval before it was filtered

  // after a failed test at iteration it < max_iter: t1, tk, tb = |θ_1|, |θ_k|,
  // |θ_b| of that test.  may_filter: the caller can run filtered iterations
  // (the fused path); θ_b then bounds the unwanted spectrum, [0, θ_b] maps to
  // [−1, 1] and λ_1, λ_k to x1, xk.
  Step next(int it, int max_iter, double rmax, double target, double t1, double tk, double tb, bool may_filter) {
#ifdef OCM_EIG_NO_CHEB  // make exp A/B: the plain iterations throughout
    may_filter = false;
#endif
    double rate = tk > 0 ? tb / tk : 1.0;
    Step s{it + 1, false, 1};
    if (may_filter) {
      const double x1 = tb > 0 ? 2.0 * t1 / tb - 1.0 : 0.0, xk = tb > 0 ? 2.0 * tk / tb - 1.0 : 0.0;
      s.dmax = tb > 0 && x1 > 1.0 && std::isfinite(x1) ? cheb_degree_cap(x1) : 1;
      // (dmax = 1, T_2(x_1) > 1e6: a filter of degree 2 would already pass the
      // condition budget — the plain iteration stays)
      s.use_cheb = s.dmax >= 2 && tk > tb * (1.0 + 1e-12);
      // per product: the segments restart the recurrence, so a segment of
      // degree d gains T_d(x_k) (1.2 at d = 2, x_k = 1.05: 0.913 per product
      // against θ_b/θ_k = 0.976 for the plain iteration, measured on the nuts
      // spectrum, profiles/r06h_eig_schedule_nuts.txt)
      if (s.use_cheb) rate = std::pow(std::cosh(s.dmax * std::acosh(xk)), -1.0 / s.dmax);
    }
    const bool measured_same = !s.use_cheb || cheb_prev;  // the last interval ran the same iteration
    if (prev_it > 0 && prev_rmax > 0 && measured_same)
      rate = std::max(rate, std::pow(rmax / prev_rmax, 1.0 / (it - prev_it)));
    int ahead = 1;
    if (rate < 0.999) ahead = (int)std::ceil(std::log(target / rmax) / std::log(std::max(rate, 1e-3)));
    ahead = std::max(1, std::min(ahead, 64));
    s.next_rr = std::min(it + ahead, max_iter);
#ifdef OCM_EIG_TRACE  // make exp diagnostic: the Rayleigh–Ritz schedule
    std::fprintf(stderr, "eig test it %d rmax %.3e target %.3e rate %.4f ahead %d cheb %d dmax %d th1/thb %.3e "
                 "thk/thb %.6f\n", it, rmax, target, rate, ahead, (int)s.use_cheb, s.dmax, t1 / tb, tk / tb);
#endif
    prev_it = it;
    prev_rmax = rmax;
    cheb_prev = s.use_cheb;
    return s;
  }
};

// ---------------------------------------------------------------------------
// a Chebyshev filter segment's buffers
// ---------------------------------------------------------------------------
// Step j of a degree-d segment writes Y_j while Y_{j−1} and Y_{j−2} are live.
// Intermediates prefer T2, T1, Wa; the last degree lands in a chain buffer,
// Wa or Wb (Wb is never an intermediate, so one of the two is always free).
// Y_0 is T1 or the Rayleigh–Ritz basis V (SEG_V: no candidate).
enum SegBuf { SEG_T2 = 0, SEG_T1 = 1, SEG_WA = 2, SEG_WB = 3, SEG_V = 4, SEG_NONE = -1 };

// the buffer step j of d writes, given those holding Y_{j−1} and Y_{j−2}; SEG_NONE if none is free
inline int cheb_out(int j, int d, int ym1, int ym2) {
  for (int c = j == d ? SEG_WA : SEG_T2; c <= SEG_WB; ++c)
    if (c != ym1 && c != ym2) return c;
  return SEG_NONE;
}

}  // namespace ocm_eig
