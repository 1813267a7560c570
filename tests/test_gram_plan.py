"""The chunk planner of the i8×3 Gram (csrc/ocm_gram_map.h: bal_first,
bal_count, plan_cost, plan_chunks, PlanMemo): one segment's B scale blocks in
N balanced chunks, N chosen by a cost model of the persistent launch's round
sweep.

Method of test_gram_roundmap.py: the header is plain C++, so a stand-alone g++
program (its own main, AddressSanitizer + UBSan, host only) includes it and
enumerates

    B ∈ {1, 2, 3, 7, 8, 82, 652, 653} × nt ∈ {1, 2, 16} × CUs ∈ {8, 256, 304}

checking that
  * for every N ≤ B the chunks partition [0, B) exactly, in order, their sizes
    differ by at most 1 and the longer ones come first;
  * the planner's choice never has more than 12 blocks per chunk (nor more
    than plan_max_blocks, the cache condition, itself in 1 … 12) and never
    more chunks than blocks;
  * it is the uniform plan (0) when B ≤ 3, and whenever it is not 0 its
    modelled cost is strictly below the uniform plan's;
  * plan_cost agrees with a makespan computed item by item from round_slot;
  * at B = 652, nwg = 132, 256 CUs the choice's modelled cost is ≤ the
    218-chunk uniform plan's;
  * the memo returns the planner's answer, answers a repeated question from
    its table, and keeps different grids (CU counts) apart.
CPU only.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ocm-vae-simca_amd", "csrc")

DRIVER = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "ocm_gram_map.h"

using namespace ocm_g8;

#define FAIL(...) do { std::printf("B=%d nt=%d cus=%d: ", B, nt, cus); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

// the makespan item by item: every workgroup's items from round_slot, each priced by its own chunk
static double slow_cost(const std::vector<int>& blocks, int nwg, int ntiles, int cus) {
  const int total = (int)blocks.size() * nwg, grid = launch_grid(total, cus);
  double span = 0.0;
  for (int b = 0; b < grid; ++b) {
    const Slot sl = round_slot(total, grid, b);
    double t = 0.0;
    for (int k = 0; k < sl.count; ++k) t += PLAN_T_FIX_US + PLAN_T_BLK_US * blocks[(sl.first + k * sl.step) / nwg];
    span = std::max(span, t);
  }
  return span + (double)blocks.size() * ntiles * 65536.0 / PLAN_REDUCE_BYTES_PER_US;
}

// the automatic uniform choice, in blocks: ≥ 4 workgroups per CU, ≤ 4096 rows → whole 1536-row blocks
static int uniform_blocks(int B, int ntiles, int cus) {
  const long long n = (long long)B * 1536;
  const long long want = std::max<long long>(1, (4LL * cus + ntiles - 1) / ntiles);
  const long long rows = std::min<long long>(4096, (n + want - 1) / want);
  return (int)std::max<long long>(1, (rows + 1535) / 1536);
}

static int check(int B, int nt, int cus) {
  const int ntiles = nt * (nt + 1) / 2, nblocks = 4 * ntiles - nt, nwg = (nblocks + 3) / 4;
  for (int N = 1; N <= B; ++N) {
    const int q = B / N, r = B % N;
    int at = 0, prev = 1 << 30;
    std::vector<int> blocks;
    for (int c = 0; c < N; ++c) {
      const int f = bal_first(q, r, c), k = bal_count(q, r, c);
      if (f != at) FAIL("N=%d chunk %d starts at %d, the chunks before it end at %d", N, c, f, at);
      if (k < 1 || (k != q && k != q + 1)) FAIL("N=%d chunk %d has %d blocks, q = %d", N, c, k, q);
      if (k > prev) FAIL("N=%d chunk %d (%d blocks) is longer than the one before it (%d)", N, c, k, prev);
      prev = k;
      at += k;
      blocks.push_back(k);
    }
    if (at != B) FAIL("N=%d covers %d blocks", N, at);
    if (B <= 82 || N == 64 || N == 218 || N == B) {
      const double a = plan_cost_balanced(B, N, nwg, ntiles, cus), s = slow_cost(blocks, nwg, ntiles, cus);
      if (std::fabs(a - s) > 1e-9 * s) FAIL("N=%d: plan_cost %.6f, item by item %.6f", N, a, s);
    }
  }
  const int cb = uniform_blocks(B, ntiles, cus);
  {
    std::vector<int> blocks;
    for (int left = B; left > 0; left -= cb) blocks.push_back(std::min(cb, left));
    const double a = plan_cost_uniform(B, cb, nwg, ntiles, cus), s = slow_cost(blocks, nwg, ntiles, cus);
    if (std::fabs(a - s) > 1e-9 * s) FAIL("uniform %d blocks: plan_cost %.6f, item by item %.6f", cb, a, s);
  }
  const int N = plan_chunks(B, cb, nwg, ntiles, cus);
  if (N < 0 || N > B) FAIL("planner: %d chunks", N);
  if (B <= 3 && N != 0) FAIL("planner: %d chunks for %d blocks, the uniform plan expected", N, B);
  if (N > 0) {
    if ((B + N - 1) / N > PLAN_MAX_BLOCKS) FAIL("planner: %d chunks, %d blocks in the longest", N, (B + N - 1) / N);
    if ((B + N - 1) / N > plan_max_blocks(nwg, ntiles, cus)) FAIL("planner: %d chunks overfill the cache", N);
    if (!(plan_cost_balanced(B, N, nwg, ntiles, cus) < plan_cost_uniform(B, cb, nwg, ntiles, cus)))
      FAIL("planner: %d chunks modelled no cheaper than the uniform plan", N);
  }
  if (PLAN_MAX_BLOCKS != 12) FAIL("cap %d", PLAN_MAX_BLOCKS);
  const int maxb = plan_max_blocks(nwg, ntiles, cus);
  if (maxb < 1 || maxb > PLAN_MAX_BLOCKS) FAIL("longest chunk allowed: %d blocks", maxb);
  // the memo: the planner's answer, once
  PlanMemo m;
  if (m.lookup(B, cb, nwg, ntiles, cus) != N || m.used != 1) FAIL("memo: first lookup");
  if (m.lookup(B, cb, nwg, ntiles, cus) != N || m.used != 1) FAIL("memo: repeated lookup added an entry");
  const int cus2 = cus + 48, N2 = plan_chunks(B, cb, nwg, ntiles, cus2);
  if (m.lookup(B, cb, nwg, ntiles, cus2) != N2 || m.used != 2) FAIL("memo: another grid must be another entry");
  if (m.lookup(B, cb, nwg, ntiles, cus) != N || m.used != 2) FAIL("memo: first grid after the second");
  for (int i = 0; i < 40; ++i)  // more questions than the table holds
    if (m.lookup(B + 1 + i, cb, nwg, ntiles, cus) != plan_chunks(B + 1 + i, cb, nwg, ntiles, cus)) FAIL("memo: wrap");
  if (m.used != PlanMemo::CAP) FAIL("memo: %d entries", m.used);
  std::printf("B=%d nt=%d cus=%d: uniform %d blocks, planner %d\n", B, nt, cus, cb, N);
  return 0;
}

int main() {
  const int Bs[] = {1, 2, 3, 7, 8, 82, 652, 653}, nts[] = {1, 2, 16}, cuss[] = {8, 256, 304};
  int bad = 0, n = 0;
  for (int B : Bs)
    for (int nt : nts)
      for (int cus : cuss) {
        bad += check(B, nt, cus);
        ++n;
      }
  {  // the headline shape: 1M × 2048 on 256 CUs
    const int B = 652, nt = 16, cus = 256, ntiles = 136, nwg = 132;
    const int N = plan_chunks(B, 3, nwg, ntiles, cus);
    const double today = plan_cost_uniform(B, 3, nwg, ntiles, cus);
    const double c = N > 0 ? plan_cost_balanced(B, N, nwg, ntiles, cus) : today;
    std::printf("headline: %d chunks modelled %.1f us, 218 uniform chunks %.1f us\n", N, c, today);
    if ((B + 2) / 3 != 218) FAIL("218 chunks expected");
    if (!(c <= today)) FAIL("headline: modelled cost above the uniform plan's");
  }
  std::printf("%d combinations, %d failed\n", n, bad);
  return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("gram_plan")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def test_balanced_chunks_and_planner(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(driver)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "72 combinations, 0 failed" in r.stdout
