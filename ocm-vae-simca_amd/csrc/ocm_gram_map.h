// The work map of the i8×3 Gram kernels (k_gram8d, k_gram8e), shared by host
// and device: which (chunk, tile, 64×64 block) a wave of a workgroup computes.
// Plain C++ (no HIP types), so a host program can enumerate it
// (tests/test_gram_workmap.py).
//
// A launch covers `nchunks` chunks × `nwg` workgroup items; item `local` of a
// chunk is the four blocks 4·local .. 4·local + 3 of that chunk's block list:
// first the off-diagonal 128×128 tiles in band order, four blocks each, then
// the nt diagonal tiles, three blocks each (the strictly-lower block of a
// diagonal tile is its mirror), packed.  Logical item ids run chunk-major;
// XCD x (workgroups b with b % 8 == x) owns a contiguous range of them
// (slot_of), or of every round of `grid` consecutive ones (round_slot).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_MAP_HD __host__ __device__ inline
#else
#define OCM_MAP_HD inline
#endif

#ifndef OCM_G8_BAND_R
#define OCM_G8_BAND_R 4
#endif
#ifndef OCM_G8_BAND_C
#define OCM_G8_BAND_C 8
#endif

namespace ocm_g8 {

constexpr int BAND_R = OCM_G8_BAND_R, BAND_C = OCM_G8_BAND_C;
constexpr int NXCD = 8;

OCM_MAP_HD int imin(int a, int b) { return a < b ? a : b; }
OCM_MAP_HD int imax(int a, int b) { return a > b ? a : b; }

// first logical item and item count of XCD x's contiguous range of `total` items
OCM_MAP_HD int xcd_first(int total, int x) {
  const int q8 = total / NXCD, r8 = total % NXCD;
  return x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8;
}
OCM_MAP_HD int xcd_count(int total, int x) { return total / NXCD + (x < total % NXCD ? 1 : 0); }

// one item per workgroup (grid = total): the logical item of workgroup b
OCM_MAP_HD int logical_item(int total, int b) { return xcd_first(total, b % NXCD) + b / NXCD; }

// persistent launch (grid ≤ total): workgroup b is slot b / 8 of XCD b % 8 and
// takes items slot, slot + S, slot + 2S, … of that XCD's range, S = the XCD's
// number of workgroups.  All derived from blockIdx alone: nothing to reset.
struct Slot {
  int first;  // logical id of the workgroup's first item
  int step;   // S
  int count;  // items of this workgroup
};
OCM_MAP_HD Slot slot_of(int total, int grid, int b) {
  const int x = b % NXCD, s = b / NXCD;
  const int S = xcd_count(grid, x), n = xcd_count(total, x);
  Slot r;
  r.first = xcd_first(total, x) + s;
  r.step = S;
  r.count = s < n ? (n - s + S - 1) / S : 0;
  return r;
}

// round sweep (grid ≤ total): the launch runs in rounds, round r being the
// logical items [r·grid, (r + 1)·grid) ∩ [0, total); inside a round XCD x
// takes the contiguous range xcd_first(grid, x) … of it, slot by slot, so an
// XCD's workgroups are on band-consecutive items as under slot_of, but all
// eight XCDs advance through the chunk list together: a round spans at most
// ⌈grid / nwg⌉ + 1 chunks.  For total ≤ grid (one item or none per
// workgroup) it is slot_of's map.  From blockIdx alone, like slot_of.
OCM_MAP_HD Slot round_slot(int total, int grid, int b) {
  Slot r;
  r.first = xcd_first(grid, b % NXCD) + b / NXCD;
  r.step = grid;
  r.count = r.first < total ? (total - r.first - 1) / grid + 1 : 0;
  return r;
}

// the two maps of the persistent launch, as k_gram8e's launch argument
enum Map { MAP_RANGE = 0, MAP_ROUND = 1 };
OCM_MAP_HD Slot map_slot(int map, int total, int grid, int b) {
  return map == MAP_ROUND ? round_slot(total, grid, b) : slot_of(total, grid, b);
}

// off-diagonal tile of band-order rank `rank` (0 .. nt(nt−1)/2 − 1)
OCM_MAP_HD void offdiag_tile(int nt, int rank, int& ti, int& tj) {
  ti = -1;
  tj = 0;
  int rem = rank;
  for (int u = 0; u < nt && ti < 0; u += BAND_R)
    for (int v = u; v < nt && ti < 0; v += BAND_C)
      for (int a = u; a < imin(nt, u + BAND_R) && ti < 0; ++a)
        for (int c = imax(v, a + 1); c < imin(nt, v + BAND_C); ++c) {
          if (rem == 0) {
            ti = a;
            tj = c;
            break;
          }
          --rem;
        }
}

// packed walk (k_gram8d has the same loops inline): every tile in band order, diagonal ones three blocks
OCM_MAP_HD void packed_block(int nt, int bi, int& ti, int& tj, int& wm, int& wn) {
  ti = -1;
  tj = wm = wn = 0;
  int rem = bi;
  for (int u = 0; u < nt && ti < 0; u += BAND_R)
    for (int v = u; v < nt && ti < 0; v += BAND_C)
      for (int a = u; a < imin(nt, u + BAND_R) && ti < 0; ++a)
        for (int c = imax(v, a); c < imin(nt, v + BAND_C); ++c) {
          const int nbk = (a == c) ? 3 : 4;
          if (rem < nbk) {
            ti = a;
            tj = c;
            wm = (a == c) ? (rem == 2) : (rem >> 1);
            wn = (a == c) ? (rem >= 1) : (rem & 1);
            break;
          }
          rem -= nbk;
        }
}

struct Block {
  int bi;      // block index within the chunk (clamped to the last one when dead)
  int offrank; // band-order rank of its off-diagonal tile, or −1: a diagonal tile's block
  int ti, tj;  // tile (set by block_tile / by the caller's table for offrank ≥ 0)
  int wm, wn;  // 64×64 block of the tile
  bool dead;   // a wave past the chunk's last block: computes a copy of it, stores nothing
};

// wave `wave` of item `local` (tile-aligned order), everything but an off-diagonal tile's (ti, tj)
OCM_MAP_HD Block block_of(int nt, int ntiles, int nblocks, int local, int wave) {
  Block k;
  k.bi = local * 4 + wave;
  k.dead = k.bi >= nblocks;
  if (k.dead) k.bi = nblocks - 1;
  const int noff = 4 * (ntiles - nt);
  if (k.bi < noff) {
    k.offrank = k.bi >> 2;
    k.wm = (k.bi >> 1) & 1;
    k.wn = k.bi & 1;
    k.ti = -1;
    k.tj = 0;
  } else {
    const int d = (k.bi - noff) / 3, r = (k.bi - noff) - 3 * d;
    k.offrank = -1;
    k.ti = k.tj = d;
    k.wm = (r == 2);
    k.wn = (r >= 1);
  }
  return k;
}
OCM_MAP_HD Block block_tile(int nt, int ntiles, int nblocks, int local, int wave) {
  Block k = block_of(nt, ntiles, nblocks, local, wave);
  if (k.offrank >= 0) offdiag_tile(nt, k.offrank, k.ti, k.tj);
  return k;
}

// index of tile (ti ≤ tj) in the partials' tile list
OCM_MAP_HD int tile_index(int nt, int ti, int tj) { return ti * nt - ti * (ti - 1) / 2 + (tj - ti); }

}  // namespace ocm_g8
