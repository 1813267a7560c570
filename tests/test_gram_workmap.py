"""The i8×3 Gram's work map (csrc/ocm_gram_map.h): which (chunk, tile, block)
each wave of each workgroup of the persistent launch computes, and in which
order.

The header is plain C++ shared by the kernels and the host, so this test
compiles it alone with g++ under AddressSanitizer + UBSan (host sanitizers
only) next to an independent copy of the one-item-per-workgroup formulas (the
XCD remap and the nested band walk as the first one-item kernel had them
inline) and enumerates
every combination of

    nt ∈ {1, 2, 3, 4, 16} × chunks ∈ {1, 2, 7, 8, 9, 218} × CUs ∈ {8, 24, 256, 304} × chunk0 ∈ {0, 5}

checking that
  * the union over (workgroup, iteration, wave) covers every (chunk, block)
    exactly once;
  * `dead` is set only for waves past `nblocks` (and always there);
  * the four waves of a workgroup take the same items (same chunk, same item
    count), and the same tile whenever the item is an off-diagonal tile — the
    order packs the diagonal tiles' three blocks, so the four waves of a
    diagonal item are on neighbouring diagonal tiles, as they always were;
  * XCD x's items, in the order its workgroups take them (iteration-major), are
    the sequence the old formula gives for workgroups b = x + 8j, j = 0, 1, …,
    with the same (tile, block, dead) per wave.
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
#include <vector>
#include "ocm_gram_map.h"

// the one-item-per-workgroup formulas, written out independently of the header
static int old_logical(int total_wg, int b) {
  const int q8 = total_wg / 8, r8 = total_wg % 8, x8 = b % 8;
  return (x8 < r8 ? x8 * (q8 + 1) : r8 * (q8 + 1) + (x8 - r8) * q8) + b / 8;
}
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
  std::vector<int> cover((size_t)nch * nblocks, 0);
  std::vector<std::vector<std::pair<int, int>>> seq(8);  // per XCD: (iteration·S + slot, item)
  for (int b = 0; b < grid; ++b) {
    const ocm_g8::Slot sl = ocm_g8::slot_of(total, grid, b);
    if (sl.step != ocm_g8::xcd_count(grid, b % 8)) FAIL("workgroup %d: stride %d", b, sl.step);
    for (int n = 0; n < sl.count; ++n) {
      const int wg = sl.first + n * sl.step;
      if (wg < 0 || wg >= total) FAIL("workgroup %d iteration %d: item %d out of range", b, n, wg);
      seq[b % 8].push_back({n * sl.step + b / 8, wg});
      const int cl = wg / nwg, local = wg - cl * nwg, chunk = chunk0 + cl;
      if (chunk < chunk0 || chunk >= chunk0 + nch) FAIL("item %d: chunk %d", wg, chunk);
      ocm_g8::Block k0{};
      for (int w = 0; w < 4; ++w) {
        const ocm_g8::Block k = ocm_g8::block_tile(nt, ntiles, nblocks, local, w);
        const OldBlock o = old_block(nt, ntiles, nblocks, local, w);
        if (k.ti != o.ti || k.tj != o.tj || k.wm != o.wm || k.wn != o.wn || k.dead != o.dead || k.bi != o.bi)
          FAIL("item %d wave %d: (%d,%d,%d,%d,%d) against the old formula's (%d,%d,%d,%d,%d)", wg, w, k.ti, k.tj,
               k.wm, k.wn, (int)k.dead, o.ti, o.tj, o.wm, o.wn, (int)o.dead);
        if (k.dead != (local * 4 + w >= nblocks)) FAIL("item %d wave %d: dead = %d", wg, w, (int)k.dead);
        if (k.ti < 0 || k.ti > k.tj || k.tj >= nt) FAIL("item %d wave %d: tile (%d, %d)", wg, w, k.ti, k.tj);
        const int tile = ocm_g8::tile_index(nt, k.ti, k.tj);
        if (tile < 0 || tile >= ntiles) FAIL("item %d wave %d: tile index %d", wg, w, tile);
        if (w == 0) k0 = k;
        if (k0.offrank >= 0 && !k.dead && (k.ti != k0.ti || k.tj != k0.tj || k.wm != (w >> 1) || k.wn != (w & 1)))
          FAIL("item %d: wave %d of an off-diagonal item on tile (%d, %d), wave 0 on (%d, %d)", wg, w, k.ti, k.tj,
               k0.ti, k0.tj);
        if (!k.dead) ++cover[(size_t)cl * nblocks + k.bi];
        // the off-diagonal table entry a kernel would build
        if (k.offrank >= 0) {
          int a, c;
          ocm_g8::offdiag_tile(nt, k.offrank, a, c);
          if (a != k.ti || c != k.tj || a >= 256 || c >= 256) FAIL("rank %d: table entry (%d, %d)", k.offrank, a, c);
        }
      }
    }
  }
  for (size_t i = 0; i < cover.size(); ++i)
    if (cover[i] != 1) FAIL("chunk %d block %d covered %d times", (int)(i / nblocks), (int)(i % nblocks), cover[i]);
  for (int x = 0; x < 8; ++x) {
    std::sort(seq[x].begin(), seq[x].end());
    const int cnt = total / 8 + (x < total % 8 ? 1 : 0);
    if ((int)seq[x].size() != cnt) FAIL("XCD %d: %d items, the old launch gave it %d", x, (int)seq[x].size(), cnt);
    for (int j = 0; j < cnt; ++j) {
      if (seq[x][j].first != j) FAIL("XCD %d: position %d taken %s", x, j, seq[x][j].first < j ? "twice" : "never");
      if (seq[x][j].second != old_logical(total, x + 8 * j))
        FAIL("XCD %d position %d: item %d, the old formula gives %d", x, j, seq[x][j].second,
             old_logical(total, x + 8 * j));
      if (ocm_g8::logical_item(total, x + 8 * j) != old_logical(total, x + 8 * j)) FAIL("logical_item(%d)", x + 8 * j);
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
    d = tmp_path_factory.mktemp("gram_workmap")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def test_persistent_work_map_matches_one_item_launch(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(driver)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "240 combinations, 0 failed" in r.stdout
