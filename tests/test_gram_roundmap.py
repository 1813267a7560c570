"""The round-sweep work map of the persistent i8×3 Gram launch
(csrc/ocm_gram_map.h: round_slot, map_slot): the launch runs in rounds of
`grid` consecutive logical items; inside a round XCD x takes a contiguous
range of them, one item per workgroup, so all eight XCDs advance through the
chunk list together.

Method of test_gram_workmap.py: the header is plain C++, so a stand-alone g++
program (its own main, AddressSanitizer + UBSan, host only) includes it and
enumerates every combination of

    nt ∈ {1, 2, 3, 4, 16} × chunks ∈ {1, 2, 7, 8, 9, 218} × CUs ∈ {8, 24, 256, 304} × chunk0 ∈ {0, 5}

checking that
  * the union over (workgroup, round, wave) covers every (chunk, block)
    exactly once, `dead` being set only for waves past `nblocks` (and always
    there);
  * in every round each XCD's items, by slot, are consecutive logical ids
    (the band sharing inside an XCD's L2 is the range map's);
  * all workgroups' items of round r lie in [r·grid, (r + 1)·grid), every id
    of that window below `total` taken once: at most ⌈grid / nwg⌉ + 1 chunks
    are live in a round;
  * for total ≤ grid the slots give the items slot_of gives, workgroup by
    workgroup;
  * each wave's (tile, block, dead) is block_tile's of the item's index in its
    chunk, equal to the one-item launch's formulas written out independently;
  * map_slot dispatches to slot_of (MAP_RANGE) and round_slot (MAP_ROUND).
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
#include <cstdio>
#include <set>
#include <vector>
#include "ocm_gram_map.h"

// the one-item-per-workgroup block formulas, written out independently of the header
struct OldBlock { int ti, tj, wm, wn, bi; bool dead; };
static OldBlock old_block(int nt, int ntiles, int nblocks, int local, int wave) {
  constexpr int R = 4, C = 8;
  OldBlock o{-1, 0, 0, 0, local * 4 + wave, false};
  o.dead = o.bi >= nblocks;
  if (o.dead) o.bi = nblocks - 1;
  const int bi = o.bi, noff = 4 * (ntiles - nt);
  if (bi < noff) {
    int rem = bi >> 2;
    o.wm = (bi >> 1) & 1;
    o.wn = bi & 1;
    for (int u = 0; u < nt && o.ti < 0; u += R)
      for (int v = u; v < nt && o.ti < 0; v += C)
        for (int a = u; a < std::min(nt, u + R) && o.ti < 0; ++a)
          for (int c = std::max(v, a + 1); c < std::min(nt, v + C); ++c) {
            if (rem == 0) { o.ti = a; o.tj = c; break; }
            --rem;
          }
  } else {
    const int d = (bi - noff) / 3, r = (bi - noff) - 3 * d;
    o.ti = o.tj = d;
    o.wm = (r == 2);
    o.wn = (r >= 1);
  }
  return o;
}

#define FAIL(...) do { std::printf("nt=%d chunks=%d cus=%d chunk0=%d: ", nt, nch, cus, chunk0); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

static int check(int nt, int nch, int cus, int chunk0) {
  const int ntiles = nt * (nt + 1) / 2, nblocks = 4 * ntiles - nt, nwg = (nblocks + 3) / 4;
  const int total = nch * nwg, grid = std::min(total, std::max(cus, ocm_g8::NXCD));
  const int nrounds = (total + grid - 1) / grid;
  std::vector<int> cover((size_t)nch * nblocks, 0);
  // item[r][b]: the logical id workgroup b takes in round r, or −1
  std::vector<std::vector<int>> item(nrounds, std::vector<int>(grid, -1));
  for (int b = 0; b < grid; ++b) {
    const ocm_g8::Slot sl = ocm_g8::round_slot(total, grid, b);
    const ocm_g8::Slot sm = ocm_g8::map_slot(ocm_g8::MAP_ROUND, total, grid, b);
    const ocm_g8::Slot so = ocm_g8::slot_of(total, grid, b), sr = ocm_g8::map_slot(ocm_g8::MAP_RANGE, total, grid, b);
    if (sm.first != sl.first || sm.step != sl.step || sm.count != sl.count) FAIL("workgroup %d: map_slot(MAP_ROUND)", b);
    if (sr.first != so.first || sr.step != so.step || sr.count != so.count) FAIL("workgroup %d: map_slot(MAP_RANGE)", b);
    if (sl.step != grid) FAIL("workgroup %d: step %d", b, sl.step);
    if (sl.count < 0 || sl.count > nrounds) FAIL("workgroup %d: %d items in %d rounds", b, sl.count, nrounds);
    if (total <= grid) {
      // one item or none per workgroup: the range map's
      if (sl.count != so.count) FAIL("workgroup %d: %d items, slot_of gives %d", b, sl.count, so.count);
      if (sl.count > 1) FAIL("workgroup %d: %d items of %d on %d workgroups", b, sl.count, total, grid);
      if (sl.count == 1 && sl.first != so.first) FAIL("workgroup %d: item %d, slot_of gives %d", b, sl.first, so.first);
      if (sl.count == 1 && sl.first != ocm_g8::logical_item(total, b)) FAIL("workgroup %d: logical_item", b);
    }
    for (int n = 0; n < sl.count; ++n) {
      const int wg = sl.first + n * sl.step;
      if (wg < 0 || wg >= total) FAIL("workgroup %d round %d: item %d out of range", b, n, wg);
      item[n][b] = wg;
      const int cl = wg / nwg, local = wg - cl * nwg, chunk = chunk0 + cl;
      if (chunk < chunk0 || chunk >= chunk0 + nch) FAIL("item %d: chunk %d", wg, chunk);
      for (int w = 0; w < 4; ++w) {
        const ocm_g8::Block k = ocm_g8::block_tile(nt, ntiles, nblocks, local, w);
        const OldBlock o = old_block(nt, ntiles, nblocks, local, w);
        if (k.ti != o.ti || k.tj != o.tj || k.wm != o.wm || k.wn != o.wn || k.dead != o.dead || k.bi != o.bi)
          FAIL("item %d wave %d: (%d,%d,%d,%d,%d) against the one-item formula's (%d,%d,%d,%d,%d)", wg, w, k.ti, k.tj,
               k.wm, k.wn, (int)k.dead, o.ti, o.tj, o.wm, o.wn, (int)o.dead);
        if (k.dead != (local * 4 + w >= nblocks)) FAIL("item %d wave %d: dead = %d", wg, w, (int)k.dead);
        if (k.ti < 0 || k.ti > k.tj || k.tj >= nt) FAIL("item %d wave %d: tile (%d, %d)", wg, w, k.ti, k.tj);
        const int tile = ocm_g8::tile_index(nt, k.ti, k.tj);
        if (tile < 0 || tile >= ntiles) FAIL("item %d wave %d: tile index %d", wg, w, tile);
        if (!k.dead) ++cover[(size_t)cl * nblocks + k.bi];
      }
    }
    // a workgroup's rounds are its first `count` ones: the kernel's item loop has no holes
    for (int n = sl.count; n < nrounds; ++n)
      if ((long long)sl.first + (long long)n * sl.step < total) FAIL("workgroup %d: round %d not taken", b, n);
  }
  for (size_t i = 0; i < cover.size(); ++i)
    if (cover[i] != 1) FAIL("chunk %d block %d covered %d times", (int)(i / nblocks), (int)(i % nblocks), cover[i]);
  const int live_max = (grid + nwg - 1) / nwg + 1;
  for (int r = 0; r < nrounds; ++r) {
    const int lo = r * grid, hi = std::min(total, lo + grid);
    std::vector<int> seen(hi - lo, 0);
    std::set<int> chunks;
    for (int b = 0; b < grid; ++b) {
      const int wg = item[r][b];
      if (wg < 0) continue;
      if (wg < lo || wg >= hi) FAIL("round %d workgroup %d: item %d outside [%d, %d)", r, b, wg, lo, hi);
      ++seen[wg - lo];
      chunks.insert(wg / nwg);
    }
    for (int i = 0; i < hi - lo; ++i)
      if (seen[i] != 1) FAIL("round %d: item %d taken %d times", r, lo + i, seen[i]);
    if ((int)chunks.size() > live_max) FAIL("round %d: %d chunks live, at most %d", r, (int)chunks.size(), live_max);
    // each XCD's items, by slot, are consecutive logical ids
    for (int x = 0; x < 8; ++x) {
      int prev = -1;
      bool ended = false;
      for (int b = x; b < grid; b += 8) {
        const int wg = item[r][b];
        if (wg < 0) { ended = true; continue; }
        if (ended) FAIL("round %d XCD %d: slot %d works after an idle slot", r, x, b / 8);
        if (prev >= 0 && wg != prev + 1) FAIL("round %d XCD %d slot %d: item %d after %d", r, x, b / 8, wg, prev);
        prev = wg;
      }
    }
  }
  return 0;
}

int main() {
  const int nts[] = {1, 2, 3, 4, 16}, chunks[] = {1, 2, 7, 8, 9, 218}, cuss[] = {8, 24, 256, 304}, c0s[] = {0, 5};
  int bad = 0, n = 0;
  for (int nt : nts)
    for (int nch : chunks)
      for (int cus : cuss)
        for (int chunk0 : c0s) {
          bad += check(nt, nch, cus, chunk0);
          ++n;
        }
  std::printf("%d combinations, %d failed\n", n, bad);
  return bad ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("gram_roundmap")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def test_round_sweep_map_covers_every_block_once_round_by_round(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(driver)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "240 combinations, 0 failed" in r.stdout
