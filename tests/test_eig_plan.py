"""The host-side planning of ocm_eig_topk (csrc/ocm_eig_plan.h): the path and
block width of every (p, k), the workspace layout, the Rayleigh–Ritz schedule
and the buffer rotation of a Chebyshev filter segment.

Method of test_gram_plan.py: the header is plain C++, so a stand-alone g++
program (its own main, AddressSanitizer + UBSan, host only) includes it.  The
carver it carves with is ocm::Carve itself, its text taken from
csrc/ocm_internal.h.

  * plan: every p in 1 … 400 with every k in 1 … p, and (2048, 20 / 21 / 64 /
    65): path and b equal ``_block`` (the restatement test_gpu_eig_blocks.py
    keeps; the copy here is asserted equal to it), a non-wide b is 32, 48 or
    64, b ≥ k, fused ⇔ b = 32;
  * layout: p ∈ {65, 66, 70, 100, 128, 300, 1000, 2048} × k ∈ {1, 6, 20, 21,
    22, 32, 33, 64, 65, p} × theta_mode 0 / 1 / 2: every buffer on a 256-byte
    boundary, no two overlapping, each as large as its kernels index it
    (sizes restated in the program), all inside the size the null-base pass
    reports, the buffers a path does not use null, the ticket range contiguous
    and gtick on a TICKET_STRIDE boundary;
  * schedule: verdict and next step against a restatement, in Python, of the
    formulas eig_topk_impl had in two copies; next_rr, use_cheb and dmax are
    equal exactly.  Every value that reaches ceil lies more than 1e-9 from an
    integer and every T_d(x1) more than 1e-9 (relative) from the 1e6 budget
    (asserted of the cases), so that libm differences cannot flip a result;
  * segments: for every degree 1 … 8 and every start buffer no step writes a
    buffer that is live as Y_{j−1} or Y_{j−2}, and the last lands in Wa or Wb.
CPU only.
"""
import ast
import inspect
import math
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ocm-vae-simca_amd", "csrc")


def _block(p, k):
    """The path ocm_eig_topk takes for (p, k): "small", the device block
    width 32 (fused) / 48 / 64, or ("wide", b)."""
    if p <= 64:
        return "small"
    b = -(-(k + max(8, k // 2)) // 16) * 16
    b = max(b, 32)
    if k <= 64 and b > 64:
        b = 64
    if b > p:
        b = max(k, (p // 16) * 16)
    assert b >= k and b >= 16
    return ("wide", b) if b > 64 else b


DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ocm_eig_plan.h"

namespace ocm {
@CARVE@
}
using namespace ocm_eig;

static const char* path_name(Path q) {
  return q == Path::small ? "small" : q == Path::fused32 ? "fused32" : q == Path::block ? "block" : "wide";
}

static int plan_grid() {
  for (int p = 1; p <= 400; ++p)
    for (int k = 1; k <= p; ++k) {
      const Plan pl = make_plan(p, k, 2);
      std::printf("%d %d %s %d %d\n", p, k, path_name(pl.path), pl.b, (int)pl.ok);
    }
  for (int k : {20, 21, 64, 65}) {
    const Plan pl = make_plan(2048, k, 2);
    std::printf("%d %d %s %d %d\n", 2048, k, path_name(pl.path), pl.b, (int)pl.ok);
  }
  return 0;
}

struct Buf { const char* name; const void* ptr; size_t bytes; bool used; };

#define FAIL(...) do { std::printf("p=%d k=%d mode=%d: ", p, k, mode); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static int layout_case(int p, int k, int mode) {
  const Plan pl = make_plan(p, k, mode);
  if (!pl.ok || pl.path == Path::small) FAIL("unexpected plan");
  // the counts, restated from what the kernels index
  const size_t b = pl.b, pb = (size_t)p * b, bb = b * b, D = sizeof(double);
  const bool fused = b == 32, wide = b > 64, block = !fused && !wide;
  const int cv_rb = (p + 15) / 16, cvq_ng = (cv_rb + 15) / 16, gt_words = (1 + cvq_ng) * 32, nblk = (p + 63) / 64;
  const int gt_at = (cv_rb + 31) / 32 * 32;  // gtick's word offset from cv_ticket
  const int nzero = fused ? gt_at + gt_words : cv_rb;
  const int tiles = ((p + 63) / 64) * (((int)b + 63) / 64);
  const int ksplit = std::max(1, std::min(16, 256 / tiles));
  const size_t ntile = (size_t)((p + 63) / 64), plane_cap = std::max((size_t)ksplit * pb, wide ? 16 * bb : (size_t)0);
  if (pl.fused() != fused || pl.wide() != wide || pl.cv_rb != cv_rb || pl.cvq_ng != cvq_ng || pl.gt_words != gt_words ||
      pl.nblk != nblk || pl.nzero_cv != nzero || pl.ksplit != ksplit || pl.plane_cap != plane_cap || pl.pb != pb ||
      pl.bb != bb || pl.def_blocks != ntile * ntile || pl.host_doubles != (wide ? 3 * bb + b : 2 * b))
    FAIL("a derived count differs from its restatement");
  ocm::Carve measure{nullptr};
  const Layout m = carve(pl, measure);
  const size_t size = measure.off;
  if (m.V || m.theta || m.cv_ticket || m.gtick || m.Wd) FAIL("the null-base pass returned a pointer");
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 40);
  ocm::Carve cv{base};
  const Layout w = carve(pl, cv);
  if (cv.off != size) FAIL("the two passes end at %zu and %zu", size, cv.off);
  const bool th = mode != 0;
  const std::vector<Buf> bufs = {
      {"V", w.V, pb * D, true}, {"W", w.W, pb * D, true}, {"T1", w.T1, pb * D, true}, {"T2", w.T2, pb * D, true},
      {"H", w.H, bb * D, true}, {"Z", w.Z, bb * D, true}, {"S", w.S, bb * D, true}, {"L", w.L, bb * D, true},
      {"theta", w.theta, 2 * b * D, true},
      {"planes", w.planes, plane_cap * D, !fused}, {"apart", w.apart, (size_t)nblk * bb * D, block},
      {"cq_part", w.cq_part, (size_t)16 * 1024 * D, fused}, {"cq_M", w.cq_M, 2048 * D, fused},
      {"cq_ticket", w.cq_ticket, 4, true},
      {"cv_part", w.cv_part, (size_t)cv_rb * 2 * 512 * D, fused},
      {"cv_ticket", w.cv_ticket, (size_t)nzero * 4, true},
      {"Wa", w.Wa, pb * D, fused}, {"Wb", w.Wb, pb * D, fused}, {"Mf", w.Mf, 2048 * D, fused},
      {"gpart", w.gpart, (size_t)(cv_rb + cvq_ng) * 1024 * D, fused}, {"Sb", w.Sb, 2 * 1056 * D, fused},
      {"dpart", w.dpart, 2 * ntile * ntile * D, th}, {"Ud", w.Ud, 2 * pb * D, th}, {"Wd", w.Wd, 2 * pb * D, th},
      {"tr3", w.tr3, 8 * D, th && fused}};
  for (const Buf& x : bufs) {
    if (!x.used) {
      if (x.ptr) FAIL("%s is carved, this path does not use it", x.name);
      continue;
    }
    if (!x.ptr) FAIL("%s is null", x.name);
    const size_t at = (const char*)x.ptr - base;
    if (at % 256) FAIL("%s at offset %zu, no multiple of 256", x.name, at);
    if (at + x.bytes > size) FAIL("%s ends at %zu, the workspace at %zu", x.name, at + x.bytes, size);
    for (const Buf& y : bufs) {
      if (&y == &x || !y.used || !y.ptr) continue;
      const size_t ay = (const char*)y.ptr - base;
      if (at < ay + y.bytes && ay < at + x.bytes) FAIL("%s and %s overlap", x.name, y.name);
    }
  }
  if (!fused) {
    if (w.gtick) FAIL("gtick is carved, this path does not use it");
  } else {
    // k_cv32's parity tickets, then k_cvq32's counters: one range of nzero_cv words
    if (w.gtick != w.cv_ticket + gt_at) FAIL("gtick is not the next TICKET_STRIDE multiple after the cv tickets");
    if (((const char*)w.gtick - base) % (TICKET_STRIDE * 4)) FAIL("gtick is not on a TICKET_STRIDE boundary");
    if (w.gtick + gt_words != w.cv_ticket + pl.nzero_cv) FAIL("the ticket range does not end with k_cvq32's counters");
    if (w.gtick < w.cv_ticket + cv_rb) FAIL("gtick starts inside the cv tickets");
  }
  return 0;
}

static int layouts() {
  int n = 0, bad = 0;
  for (int p : {65, 66, 70, 100, 128, 300, 1000, 2048})
    for (int k : {1, 6, 20, 21, 22, 32, 33, 64, 65, p}) {
      if (k > p) continue;
      for (int mode = 0; mode <= 2; ++mode) {
        bad += layout_case(p, k, mode);
        ++n;
      }
    }
  {  // the small path: the eigenvalues and the p×p rotations
    const int p = 50, k = 5, mode = 2;
    ocm::Carve measure{nullptr};
    const Plan pl = make_plan(p, k, mode);
    carve(pl, measure);
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 40);
    ocm::Carve cv{base};
    const Layout w = carve(pl, cv);
    if (pl.path != Path::small || (char*)w.theta != base || (char*)w.Z - base < (long)(p * sizeof(double)) ||
        ((char*)w.Z - base) % 256 || (char*)w.Z - base + (size_t)p * p * sizeof(double) > measure.off || w.V || w.cv_ticket)
      FAIL("small layout");
  }
  std::printf("%d layouts, %d failed\n", n, bad);
  return bad ? 1 : 0;
}

static int segments() {
  int n = 0;
  for (int d = 1; d <= 8; ++d)
    for (int y1_from_w = 0; y1_from_w <= 1; ++y1_from_w)  // (step 1 then reads W and Y0 instead of C·Y0: the same liveness)
      for (int start : {(int)SEG_V, (int)SEG_T1, (int)SEG_T2, (int)SEG_WA, (int)SEG_WB}) {
        int i1 = start, i2 = SEG_NONE;
        for (int j = 1; j <= d; ++j) {
          const int o = cheb_out(j, d, i1, i2);
          if (o < SEG_T2 || o > SEG_WB || o == i1 || o == i2 || (j == d && o != SEG_WA && o != SEG_WB)) {
            std::printf("d=%d start=%d step %d writes %d (live %d, %d)\n", d, start, j, o, i1, i2);
            return 1;
          }
          i2 = i1;
          i1 = o;
        }
        ++n;
      }
  std::printf("%d segments, 0 failed\n", n);
  return 0;
}

// replays the calls on stdin: H / C (first / next call of a history) it max_iter rmax target t1 tk tb may_filter;
// V k b tol h[0 … 2b); D x1
static int schedule() {
  char line[1 << 16];
  Schedule sch;
  while (std::fgets(line, sizeof(line), stdin)) {
    char* q = line + 2;
    if (line[0] == 'H' || line[0] == 'C') {
      if (line[0] == 'H') sch = Schedule();
      const int it = (int)std::strtol(q, &q, 10), max_iter = (int)std::strtol(q, &q, 10);
      double v[5];
      for (double& x : v) x = std::strtod(q, &q);
      const int may = (int)std::strtol(q, &q, 10);
      const Step s = sch.next(it, max_iter, v[0], v[1], v[2], v[3], v[4], may != 0);
      std::printf("%d %d %d\n", s.next_rr, (int)s.use_cheb, s.dmax);
    } else if (line[0] == 'V') {
      const int k = (int)std::strtol(q, &q, 10), b = (int)std::strtol(q, &q, 10);
      const double tol = std::strtod(q, &q);
      std::vector<double> h(2 * b);
      for (double& x : h) x = std::strtod(q, &q);
      const Verdict v = verdict(h.data(), k, b, tol);
      std::printf("%d %d %d %a %a\n", (int)v.waited_out, (int)v.nan, (int)v.converged, v.rmax, v.target);
    } else if (line[0] == 'D') {
      std::printf("%d\n", cheb_degree_cap(std::strtod(q, &q)));
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  const char* what = argc > 1 ? argv[1] : "";
  if (!std::strcmp(what, "plan")) return plan_grid();
  if (!std::strcmp(what, "layout")) return layouts();
  if (!std::strcmp(what, "segments")) return segments();
  if (!std::strcmp(what, "schedule")) return schedule();
  return 2;
}
"""


def _carve_text():
    """align_up and struct Carve as csrc/ocm_internal.h defines them."""
    with open(os.path.join(CSRC, "ocm_internal.h")) as f:
        src = f.read()
    m = re.search(r"^inline size_t align_up\(.*?^struct Carve \{.*?^\};\n", src, re.S | re.M)
    assert m, "ocm::Carve not found in ocm_internal.h"
    assert "hip" not in m.group(0).lower()
    return m.group(0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("eig_plan")
    src = d / "drv.cpp"
    src.write_text(DRIVER.replace("@CARVE@", _carve_text()))
    exe = d / "drv"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def _run(driver, what, stdin=None):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(driver), what], env=env, input=stdin, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_block_restatement_is_the_gpu_tests():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_eig_blocks.py")) as f:
        src = f.read()
    theirs = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "_block"]
    assert len(theirs) == 1
    assert ast.get_source_segment(src, theirs[0]).strip() == inspect.getsource(_block).strip()


def test_plan_paths_and_widths(driver):
    rows = [ln.split() for ln in _run(driver, "plan").splitlines()]
    want = [(p, k) for p in range(1, 401) for k in range(1, p + 1)] + [(2048, k) for k in (20, 21, 64, 65)]
    assert [(int(r[0]), int(r[1])) for r in rows] == want
    for p, k, path, b, ok in rows:
        p, k, b = int(p), int(k), int(b)
        assert ok == "1", (p, k)
        blk = _block(p, k)
        got = "small" if path == "small" else ("wide", b) if path == "wide" else b
        assert got == blk, (p, k, path, b, blk)
        if path == "small":
            continue
        assert b >= k, (p, k, b)
        assert (path == "fused32") == (b == 32), (p, k, path, b)
        if path != "wide":
            assert b in (32, 48, 64) and path == ("fused32" if b == 32 else "block"), (p, k, path, b)
        else:
            assert b > 64
    by = {(int(r[0]), int(r[1])): (r[2], int(r[3])) for r in rows}
    assert by[(2048, 20)] == ("fused32", 32) and by[(2048, 21)] == ("fused32", 32)
    assert by[(2048, 64)] == ("block", 64) and by[(2048, 65)] == ("wide", 112)


def test_workspace_layout(driver):
    out = _run(driver, "layout")
    n = sum(1 for p in (65, 66, 70, 100, 128, 300, 1000, 2048) for k in (1, 6, 20, 21, 22, 32, 33, 64, 65, p)
            if k <= p) * 3
    assert f"{n} layouts, 0 failed" in out, out[-4000:]


def test_chebyshev_segment_buffers(driver):
    assert "80 segments, 0 failed" in _run(driver, "segments")


# ---- the schedule: today's formulas, restated --------------------------------
_margins = {"ceil": 1.0, "budget": 1.0}


def _cheb_degree_cap(x1):
    d = 1
    while d < 8:
        t = math.cosh((d + 1) * math.acosh(x1))
        _margins["budget"] = min(_margins["budget"], abs(t / 1e6 - 1.0))
        if not t <= 1e6:
            break
        d += 1
    return d


def _verdict(h, k, b, tol):
    waited = any(h[b + i] < 0.0 for i in range(k))
    rmax = 0.0
    for i in range(k):
        rmax = h[b + i] if rmax < h[b + i] else rmax  # std::max(rmax, h)
    scale = abs(h[0])
    target = tol * (scale if scale > 0 else 1.0)
    return waited, rmax != rmax, rmax <= target, rmax, target


class _Schedule:
    def __init__(self):
        self.prev_it, self.prev_rmax, self.cheb_prev = 0, 0.0, False

    def next(self, it, max_iter, rmax, target, t1, tk, tb, may_filter):
        rate = tb / tk if tk > 0 else 1.0
        use_cheb, dmax = False, 1
        if may_filter:  # the fused copy; with use_cheb False it is the unfused one
            x1 = 2.0 * t1 / tb - 1.0 if tb > 0 else 0.0
            xk = 2.0 * tk / tb - 1.0 if tb > 0 else 0.0
            dmax = _cheb_degree_cap(x1) if tb > 0 and x1 > 1.0 and math.isfinite(x1) else 1
            use_cheb = dmax >= 2 and tk > tb * (1.0 + 1e-12)
            if use_cheb:
                rate = math.cosh(dmax * math.acosh(xk)) ** (-1.0 / dmax)
        measured_same = (not use_cheb) or self.cheb_prev
        if self.prev_it > 0 and self.prev_rmax > 0 and measured_same:
            rate = max(rate, (rmax / self.prev_rmax) ** (1.0 / (it - self.prev_it)))
        ahead = 1
        if rate < 0.999:
            arg = math.log(target / rmax) / math.log(max(rate, 1e-3))
            _margins["ceil"] = min(_margins["ceil"], abs(arg - round(arg)))
            ahead = math.ceil(arg)
        ahead = max(1, min(ahead, 64))
        self.prev_it, self.prev_rmax, self.cheb_prev = it, rmax, use_cheb
        return min(it + ahead, max_iter), use_cheb, dmax


def _hx(x):
    return "inf" if x == math.inf else "nan" if x != x else float(x).hex()


def test_rayleigh_ritz_schedule(driver):
    lines, want = [], []
    # the degree cap: x1 = 1 and ∞ are its edges (acosh 0: every degree passes; T_2 = ∞: none does)
    for x1 in (1.0, 1.0001, 1.05, 3.0, 300.0, 1e6, math.inf):
        lines.append(f"D {_hx(x1)}")
        want.append(str(_cheb_degree_cap(x1)))
    assert want == ["8", "8", "8", "8", "2", "1", "1"]
    # verdicts: converged at the first test, not converged, the residual of pair k + 1 ignored, θ_1 = 0 (scale 1),
    # a negative residual (waited out), NaN residuals (std::max keeps the running maximum: see _verdict)
    k, b = 3, 4
    for tol, h in [(1e-10, [5.0, 4, 3, 2, 1e-11, 3e-10, 2e-10, 7.0]), (1e-10, [5.0, 4, 3, 2, 1e-11, 6e-10, 2e-10, 0.0]),
                   (1e-3, [0.0, 0, 0, 0, 5e-4, 1e-4, 0.0, 9.0]), (1e-10, [5.0, 4, 3, 2, 1e-3, -1.0, -1.0, -1.0]),
                   (1e-10, [5.0, 4, 3, 2, math.nan, 1e-3, 1e-4, 0.0]), (1e-10, [5.0, 4, 3, 2, 1e-3, math.nan, 1e-4, 0.0]),
                   (1e-10, [math.nan, 4, 3, 2, 1e-12, 1e-12, 1e-12, 0.0])]:
        lines.append(f"V {k} {b} {_hx(tol)} " + " ".join(_hx(float(x)) for x in h))
        wo, nan, conv, rmax, target = _verdict([float(x) for x in h], k, b, tol)
        want.append(f"{int(wo)} {int(nan)} {int(conv)} {rmax.hex() if rmax == rmax else 'nan'} "
                    f"{target.hex() if target == target else 'nan'}")
    assert [w.split()[:3] for w in want[7:11]] == [["0", "0", "1"], ["0", "0", "0"], ["0", "0", "1"], ["1", "0", "0"]]
    # histories: the residual of a test at iteration it is r0·f^it
    nhist = 0
    spectra = [(50.0, 10.0, 9.7), (50.0, 10.0, 1.0), (50.0, 10.0, 0.0), (50.0, 0.0, 0.0), (1.00005, 1.00001, 1.0),
               (1.025, 1.02, 1.0), (2.0, 1.3, 1.0), (150.5, 3.0, 1.0), (500000.5, 7.0, 1.0), (math.inf, 2.0, 1.0),
               (10.0, 1.0, 1.0)]
    for f in (0.5, 0.9, 0.976, 0.9995, 1.03):
        for t1, tk, tb in spectra:
            for may_filter in (False, True):
                for max_iter in (3000, 40):
                    sch, it, first = _Schedule(), 5, True
                    scale = t1 if math.isfinite(t1) else 1.0
                    target = 1e-10 * scale
                    for _ in range(12):
                        rmax = 0.37 * scale * f ** it
                        if rmax <= target or it >= max_iter:
                            break
                        lines.append(f"{'H' if first else 'C'} {it} {max_iter} {_hx(rmax)} {_hx(target)} {_hx(t1)} "
                                     f"{_hx(tk)} {_hx(tb)} {int(may_filter)}")
                        nxt, use_cheb, dmax = sch.next(it, max_iter, rmax, target, t1, tk, tb, may_filter)
                        want.append(f"{nxt} {int(use_cheb)} {dmax}")
                        assert it < nxt <= min(it + 64, max_iter)
                        it, first = nxt, False
                    nhist += not first
    # rmax ≤ target at a test that still asks (the drivers stop before): one iteration ahead
    lines.append(f"H 5 3000 {_hx(1e-11)} {_hx(3e-10)} {_hx(3.0)} {_hx(2.0)} {_hx(1.0)} 1")
    want.append("%d %d %d" % _Schedule().next(5, 3000, 1e-11, 3e-10, 3.0, 2.0, 1.0, True))
    assert want[-1].split()[0] == "6"
    got = _run(driver, "schedule", "\n".join(lines) + "\n").splitlines()
    assert nhist == 5 * len(spectra) * 4 and len(got) == len(want)  # every history asked at least once
    for ln, g, w in zip(lines, got, want):
        assert g == w, (ln, g, w)
    kinds = {tuple(w.split()[1:]) for ln, w in zip(lines, want) if ln[0] in "HC"}
    assert {d for c, d in kinds if c == "1"} >= {"2", "8"} and ("0", "1") in kinds  # filtered and plain steps
    aheads = {int(w.split()[0]) - int(ln.split()[1]) for ln, w in zip(lines, want) if ln[0] in "HC"}
    assert 64 in aheads and 1 in aheads and len(aheads) > 10  # the cap, the floor and predictions in between
    assert _margins["ceil"] > 1e-9 and _margins["budget"] > 1e-9, _margins
