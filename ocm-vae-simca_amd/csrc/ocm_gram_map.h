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

// ---------------------------------------------------------------------------
// Balanced chunks.  One segment's B scale blocks split into N ≤ B chunks of
// q + 1 (the first r chunks) or q blocks, q = B / N, r = B mod N: the longer
// chunks are one run at the front, so only one round of the sweep mixes item
// lengths.  The kernels derive a chunk's blocks from (q, r) alone.
// ---------------------------------------------------------------------------
OCM_MAP_HD int bal_first(int q, int r, int c) { return c * q + imin(c, r); }
OCM_MAP_HD int bal_count(int q, int r, int c) { return q + (c < r ? 1 : 0); }

// The planner (host).  A chunk's f32 running sum takes one flush per scale
// block, so its rounding grows with the chunk's length: 12 blocks per chunk is
// the cap the accuracy test is written for (4× the 3 blocks of the uniform
// default) — a condition, not a tuning result.
constexpr int PLAN_MAX_BLOCKS = 12;
// The model's constants, all measured at 1M × 2048 on MI355X:
//   PLAN_T_FIX_US  per item, entry → first MFMA (0.8 µs) plus last MFMA → end
//                  (2.0 µs): k_gram8e's wall-clock stamps ("The
//                  persistent Gram launch");
//   PLAN_T_BLK_US  per item and scale block: the 3-block items' ≈ 80 µs less
//                  the fixed part, over three (same stamps);
//   PLAN_REDUCE_BYTES_PER_US  k_gram_reduce reading the f32 partials: 1.9 GB
//                  in 0.30–0.38 ms (DESIGN kernel table).
constexpr double PLAN_T_FIX_US = 2.8, PLAN_T_BLK_US = 25.7, PLAN_REDUCE_BYTES_PER_US = 5.9e6;
// The model holds only while the digit panels a round has live stay in the
// Infinity Cache (256 MiB): a round spans ⌈grid / nwg⌉ + 1 chunks, and an
// item's panels are read again by the chunk's other items, partly a round
// later.  Measured per-block time (profiles/r09a_gram_plan_ab.txt, three
// chunks live of 9.4 MB per block): 25.5–25.7 µs for 3 … 7 blocks per chunk
// (≤ 198 MB live), +0.6 % at 9 (255 MB), +3.7 % at 11 (311 MB), with the
// bytes fetched beyond L2 up by a quarter; at 8 (226 MB) the kernel ran 0.5 %
// under the 5 … 7-block plans and the whole call lost to them in the same
// process.  Chunks whose round would fill more than PLAN_CACHE_FILL of the
// cache are no candidates: three quarters admits 7 blocks at that shape.
constexpr double PLAN_CACHE_BYTES = 256.0 * 1024 * 1024, PLAN_CACHE_FILL = 0.75;
constexpr int PLAN_BLOCK_ROWS = 1536, PLAN_TILE_COLS = 128;  // the quantiser's scale block, the Gram's tile

// the persistent launch's grid for `total` items on `cus` compute units
OCM_MAP_HD int launch_grid(int total, int cus) { return imin(total, imax(cus, NXCD)); }

// Modelled µs of Gram + reduce for `nl` chunks of `bl` blocks followed by `ns`
// chunks of `bs` blocks (both the balanced split and the uniform one with its
// short last chunk have this form): the makespan over the workgroups of
// Σ (t_fix + blocks · t_blk) over the items round_slot hands each, plus the
// reduce's pass over the partials (64 KiB per chunk and tile).
inline double plan_cost(int nl, int bl, int ns, int bs, int nwg, int ntiles, int cus) {
  const long long total_ll = (long long)(nl + ns) * nwg;
  if (total_ll <= 0 || total_ll >= (1LL << 31)) return 1e300;
  const int total = (int)total_ll, grid = launch_grid(total, cus);
  const long long nlong_items = (long long)nl * nwg;
  double span = 0.0;
  for (int b = 0; b < grid; ++b) {
    const Slot sl = round_slot(total, grid, b);
    long long cl = sl.first < nlong_items ? (nlong_items - sl.first - 1) / grid + 1 : 0;
    if (cl > sl.count) cl = sl.count;
    const double t = sl.count * PLAN_T_FIX_US + PLAN_T_BLK_US * ((double)cl * bl + (double)(sl.count - cl) * bs);
    if (t > span) span = t;
  }
  return span + (double)(nl + ns) * ntiles * 65536.0 / PLAN_REDUCE_BYTES_PER_US;
}
inline double plan_cost_balanced(int B, int N, int nwg, int ntiles, int cus) {
  return plan_cost(B % N, B / N + 1, N - B % N, B / N, nwg, ntiles, cus);
}
// uniform chunks of cb blocks, the last one holding what is left
inline double plan_cost_uniform(int B, int cb, int nwg, int ntiles, int cus) {
  const int C = (B + cb - 1) / cb;
  return plan_cost(C - 1, cb, 1, B - (C - 1) * cb, nwg, ntiles, cus);
}

// the longest chunk, in blocks, the planner may choose: the accuracy cap and
// the cache condition (three digit planes of 1 B per value)
inline int plan_max_blocks(int nwg, int ntiles, int cus) {
  int nt = 1;
  while (nt * (nt + 1) / 2 < ntiles) ++nt;
  const double block_bytes = 3.0 * PLAN_BLOCK_ROWS * PLAN_TILE_COLS * nt;
  const int live = (imax(cus, NXCD) + nwg - 1) / nwg + 1;
  const double fit = PLAN_CACHE_BYTES * PLAN_CACHE_FILL / (live * block_bytes);
  return fit >= PLAN_MAX_BLOCKS ? PLAN_MAX_BLOCKS : imax(1, (int)fit);
}

// The balanced chunk count for B scale blocks, or 0: keep the uniform plan of
// `cb_uniform` blocks per chunk (the automatic choice before the planner),
// which stands whenever no candidate is modelled strictly cheaper.  Candidates
// are the N with ⌈B / N⌉ ≤ plan_max_blocks.
inline int plan_chunks(int B, int cb_uniform, int nwg, int ntiles, int cus) {
  if (B <= 3) return 0;  // at most one uniform chunk's worth: nothing to plan
  double best = plan_cost_uniform(B, cb_uniform, nwg, ntiles, cus);
  int bestN = 0;
  const int maxb = plan_max_blocks(nwg, ntiles, cus);
  for (int N = (B + maxb - 1) / maxb; N <= B; ++N) {
    const double c = plan_cost_balanced(B, N, nwg, ntiles, cus);
    if (c < best) {
      best = c;
      bestN = N;
    }
  }
  return bestN;
}

// The planner's answers of one context, by (B, nwg, grid cap, uniform blocks):
// a fit asks the same question every step and pays the model once.
struct PlanMemo {
  static constexpr int CAP = 16;
  struct Entry {
    int B, nwg, grid, cb, N;
  };
  Entry e[CAP];
  int used = 0, next = 0;
  int lookup(int B, int cb_uniform, int nwg, int ntiles, int cus) {
    const int grid = imax(cus, NXCD);
    for (int i = 0; i < used; ++i)
      if (e[i].B == B && e[i].nwg == nwg && e[i].grid == grid && e[i].cb == cb_uniform) return e[i].N;
    const int N = plan_chunks(B, cb_uniform, nwg, ntiles, cus);
    e[next] = Entry{B, nwg, grid, cb_uniform, N};
    next = (next + 1) % CAP;
    if (used < CAP) ++used;
    return N;
  }
};

}  // namespace ocm_g8
