// K20 — threshold-free evaluation: exact ROC AUC, ROC points and a keys-only
// device sort.  Reference site: optim_bce_nuts.py:241,279
// (roc_auc_score(labels_true, f_all)).
//
// AUC = u2 / (2 P N) with u2 = Σ_{pos i, neg j} 2·[s_i > s_j] + [s_i == s_j], an
// exact integer.  Only the smaller class is sorted (keys only, no payload); the
// rows of the other class are read straight from S through the mask and each
// finds lt = #keys < s and le = #keys ≤ s in the sorted side by binary searches
// without a branch on the data (k_auc_search: two levels, bucket splitters in
// LDS; le from two probes behind lt unless a wave meets a longer run of equal
// keys, which costs it the second search).  Lanes add up in 64-bit integers,
// waves reduce by shuffles, and one integer atomic per workgroup lands in
// u2_out: no floating-point sum anywhere, so two calls give the same bytes.
//
// The sort is a least-significant-digit radix sort on the 8-bit digits of the
// order-preserving key of ocm_select.hip (okey64 / okey32; a NaN maps to the
// all-ones key and so goes last).  One read up front histograms every digit
// position of every column (k_prehist); a position at which all keys of a
// column share one digit is skipped for that column (decision values usually
// share their sign and exponent bytes), and a column whose keys are all equal
// is never sorted at all (its one key is known from the histogram).  An
// executed pass is three launches, and no workgroup waits for another:
//   k_tile_hist  digit histogram of each tile of TILE keys      → cnt[col][tile][256]
//   k_scan       exclusive scan over (digit, tile), in place, one workgroup per column
//   k_scatter    stable scatter: a key's rank inside its wave comes from eight
//                __ballot masks (64-bit) and popcounts, the waves' and the
//                tile's bases from the scanned table
// The first executed pass of a column loads its keys from S through the mask
// (its tiles span the m rows), so the sorted class is gathered by that pass
// and never by a launch of its own; later passes ping-pong between two key
// buffers.  Columns are grid dimension y: ncol columns cost one set of launches.
//
// Bytes moved per executed pass and column, n keys of b bytes: tile histogram
// reads n·b, scatter reads n·b and writes n·b, the table adds ⌈n/TILE⌉·1 KiB
// written, scanned (read twice, written once) and read back: ≈ 3·n·b + n·2.5.
#include <algorithm>
#include <cstring>

#include "ocm_internal.h"

namespace {

constexpr int TILE_THREADS = 256;
constexpr int KPT = 8;  // keys per thread of a sort tile
constexpr int TILE = TILE_THREADS * KPT;
constexpr int WAVES = TILE_THREADS / 64;
constexpr int SCAN_THREADS = 1024;
// keys of one column group: the two key buffers of a group stay below 1 GiB
constexpr int64_t GROUP_KEYS = (int64_t)1 << 26;
constexpr int MAX_THR = 4096;

__device__ __forceinline__ uint64_t okey64(uint64_t u) {
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ uint32_t okey32(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }

// where the keys of a column come from before its first executed pass
struct Src {
  const void* S;  // already advanced to the group's first column
  int64_t cs, rs, m;
  const uint8_t* mask;  // NULL: every row
  int want;             // the class taken (mask != 0) == want; ignored without a mask
  int fold;             // −0.0 → +0.0 before the key is formed
};

struct ColPlan {
  uint32_t exec;   // bit d: digit position d is sorted for this column
  uint32_t nan_s;  // NaN rows of the taken class
  uint32_t nan_o;  // NaN rows of the other class
  uint32_t pad_;
  uint64_t ckey;  // the digits of the skipped positions (the whole key when exec == 0)
};

template <typename K>
struct Key;
template <>
struct Key<uint64_t> {
  static constexpr int ND = 8;
  __device__ static uint64_t load(const Src& s, int c, int64_t r, bool& nan) {
    uint64_t u = static_cast<const uint64_t*>(s.S)[(int64_t)c * s.cs + r * s.rs];
    if (s.fold && (u << 1) == 0) u = 0;
    nan = (u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
    return nan ? ~0ull : okey64(u);
  }
  __device__ static uint64_t bits(uint64_t key) { return (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key; }
};
template <>
struct Key<uint32_t> {
  static constexpr int ND = 4;
  __device__ static uint32_t load(const Src& s, int c, int64_t r, bool& nan) {
    uint32_t u = static_cast<const uint32_t*>(s.S)[(int64_t)c * s.cs + r * s.rs];
    if (s.fold && (u << 1) == 0) u = 0;
    nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
    return nan ? ~0u : okey32(u);
  }
  __device__ static uint32_t bits(uint32_t key) { return (key >> 31) ? (key & 0x7FFFFFFFu) : ~key; }
};

__device__ __forceinline__ bool in_class(const Src& s, int64_t r) {
  return !s.mask || (int)(s.mask[r] != 0) == s.want;
}

// lh[d] += 1 for the lanes with `take`; one atomic per wave when they all share
// the digit (same-address LDS atomics of a wave are served one after another)
__device__ __forceinline__ void hist_add(unsigned* lh, unsigned d, bool take) {
  const uint64_t act = __ballot(take);
  if (!act) return;
  const int fl = __ffsll((unsigned long long)act) - 1;
  const unsigned d0 = __shfl(d, fl, 64);
  if (__ballot(take && d != d0) == 0) {
    if ((int)(threadIdx.x & 63) == fl) atomicAdd(&lh[d0], (unsigned)__popcll(act));
  } else if (take) {
    atomicAdd(&lh[d], 1u);
  }
}

__global__ __launch_bounds__(256) void k_count_mask(const uint8_t* __restrict__ mask, int64_t m,
                                                    unsigned long long* __restrict__ np) {
  __shared__ unsigned long long part[4];
  unsigned long long p = 0, rows = 0;
  // eight flags per load between the first and the last 8-byte boundary, single bytes outside
  const int64_t head = std::min<int64_t>(m, (int64_t)((8 - (reinterpret_cast<uintptr_t>(mask) & 7)) & 7));
  const int64_t nw = (m - head) / 8, tail0 = head + nw * 8;
  const uint64_t* w = reinterpret_cast<const uint64_t*>(mask + head);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nw; i += stride) {
    const uint64_t x = w[i];  // bit 7 of every byte of y: that byte of x is not zero
    const uint64_t y = (((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull;
    p += (unsigned)__popcll(y);
    rows += 8;
  }
  if (blockIdx.x == 0) {
    const int64_t t = threadIdx.x;
    if (t < head) {
      p += mask[t] != 0;
      ++rows;
    }
    if (t >= 8 && tail0 + (t - 8) < m) {
      p += mask[tail0 + (t - 8)] != 0;
      ++rows;
    }
  }
  p |= rows << 32;  // a thread sees far fewer than 2^31 rows: both counts in one word
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long tot = part[0] + part[1] + part[2] + part[3];
    const unsigned long long pos = tot & 0xFFFFFFFFull, all = tot >> 32;
    if (pos) atomicAdd(&np[0], pos);
    if (all - pos) atomicAdd(&np[1], all - pos);
  }
}

// every digit position of every column in one read; NaN rows counted per class
template <typename K>
__global__ __launch_bounds__(256) void k_prehist(Src src, unsigned* __restrict__ h0, ColPlan* __restrict__ plan) {
  constexpr int ND = Key<K>::ND;
  __shared__ unsigned lh[ND * 256];
  __shared__ unsigned lnan[2];
  const int c = blockIdx.y;
  for (int i = threadIdx.x; i < ND * 256; i += 256) lh[i] = 0;
  if (threadIdx.x < 2) lnan[threadIdx.x] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < src.m; base += stride) {
    const int64_t r = base + threadIdx.x;
    const bool in = r < src.m;
    bool nan = false;
    K key = 0;
    if (in) key = Key<K>::load(src, c, r, nan);
    const bool take = in && in_class(src, r);
    const uint64_t ns = __ballot(take && nan), no = __ballot(in && !take && nan);
    if ((threadIdx.x & 63) == 0) {
      if (ns) atomicAdd(&lnan[0], (unsigned)__popcll(ns));
      if (no) atomicAdd(&lnan[1], (unsigned)__popcll(no));
    }
#pragma unroll
    for (int pos = 0; pos < ND; ++pos) hist_add(lh + pos * 256, (unsigned)(key >> (8 * pos)) & 255u, take);
  }
  __syncthreads();
#pragma unroll
  for (int pos = 0; pos < ND; ++pos) {
    const unsigned v = lh[pos * 256 + threadIdx.x];
    if (v) atomicAdd(&h0[((int64_t)c * ND + pos) * 256 + threadIdx.x], v);
  }
  if (threadIdx.x == 0) {
    if (lnan[0]) atomicAdd(&plan[c].nan_s, lnan[0]);
    if (lnan[1]) atomicAdd(&plan[c].nan_o, lnan[1]);
  }
}

// which positions a column sorts, and the digits of those it skips
template <int ND>
__global__ __launch_bounds__(256) void k_plan(const unsigned* __restrict__ h0, ColPlan* __restrict__ plan,
                                              long long* __restrict__ nnan_out) {
  __shared__ unsigned sd[ND];
  const int c = blockIdx.x;
  if (threadIdx.x < ND) sd[threadIdx.x] = 0;
  __syncthreads();
  unsigned exec = 0;
  for (int pos = 0; pos < ND; ++pos) {
    const unsigned v = h0[((int64_t)c * ND + pos) * 256 + threadIdx.x];
    const int nz = __syncthreads_count(v != 0);
    if (nz > 1)
      exec |= 1u << pos;
    else if (v != 0)
      sd[pos] = threadIdx.x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t ck = 0;
    for (int pos = 0; pos < ND; ++pos) ck |= (uint64_t)sd[pos] << (8 * pos);
    plan[c].exec = exec;
    plan[c].ckey = ck;
    if (nnan_out) nnan_out[c] = (long long)plan[c].nan_s + (long long)plan[c].nan_o;
  }
}

// the state of column c at digit position pos
struct PassState {
  bool run, first, last;
  int nprev;
};
__device__ __forceinline__ PassState pass_state(const ColPlan* plan, int c, int pos) {
  const unsigned exec = plan[c].exec;
  PassState s;
  s.run = (exec >> pos) & 1u;
  s.nprev = __popc(exec & ((1u << pos) - 1u));
  s.first = s.nprev == 0;
  s.last = (exec >> (pos + 1)) == 0;
  return s;
}

template <typename K>
__global__ __launch_bounds__(TILE_THREADS) void k_tile_hist(Src src, const ColPlan* __restrict__ plan,
                                                            const K* __restrict__ bufA, const K* __restrict__ bufB,
                                                            int64_t ns, int pos, unsigned* __restrict__ cnt,
                                                            int64_t ntstride) {
  __shared__ unsigned lh[256];
  const int c = blockIdx.y;
  const PassState ps = pass_state(plan, c, pos);
  if (!ps.run) return;
  const int64_t n = ps.first ? src.m : ns;
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  if (t0 >= n) return;
  const K* in = (((ps.nprev - 1) & 1) ? bufB : bufA) + (int64_t)c * ns;
  lh[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int64_t i = t0 + j * TILE_THREADS + threadIdx.x;
    bool a = i < n;
    K key = 0;
    if (a) {
      if (ps.first) {
        bool nan;
        a = in_class(src, i);
        if (a) key = Key<K>::load(src, c, i, nan);
      } else {
        key = in[i];
      }
    }
    hist_add(lh, (unsigned)(key >> (8 * pos)) & 255u, a);
  }
  __syncthreads();
  cnt[((int64_t)c * ntstride + blockIdx.x) * 256 + threadIdx.x] = lh[threadIdx.x];
}

// cnt[col][tile][digit] → its exclusive prefix in (digit, tile) order.  Four
// thread groups take a quarter of the tiles each, so a sweep is a quarter as
// many dependent steps; the loads of a sweep do not depend on its sums.
__global__ __launch_bounds__(SCAN_THREADS) void k_scan(const ColPlan* __restrict__ plan, unsigned* __restrict__ cnt,
                                                       int64_t ntstride, int64_t m, int64_t ns, int pos) {
  constexpr int G = SCAN_THREADS / 256;
  __shared__ unsigned part[G][256];
  __shared__ unsigned sc[256];
  const int c = blockIdx.x;
  const PassState ps = pass_state(plan, c, pos);
  if (!ps.run) return;
  const int64_t n = ps.first ? m : ns;
  const int64_t nt = (n + TILE - 1) / TILE;
  const int g = threadIdx.x >> 8, t = threadIdx.x & 255;
  const int64_t per = (nt + G - 1) / G;
  const int64_t lo = std::min<int64_t>(nt, g * per), hi = std::min<int64_t>(nt, lo + per);
  unsigned* col = cnt + (int64_t)c * ntstride * 256;
  unsigned s = 0;
#pragma unroll 8
  for (int64_t k = lo; k < hi; ++k) s += col[k * 256 + t];
  part[g][t] = s;
  __syncthreads();
  unsigned tot = 0, before = 0;
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const unsigned v = part[q][t];
    if (q < g) before += v;
    tot += v;
  }
  if (g == 0) sc[t] = tot;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned v = (g == 0 && t >= off) ? sc[t - off] : 0u;
    __syncthreads();
    if (g == 0) sc[t] += v;
    __syncthreads();
  }
  unsigned run = sc[t] - tot + before;
#pragma unroll 8
  for (int64_t k = lo; k < hi; ++k) {
    const unsigned v = col[k * 256 + t];
    col[k * 256 + t] = run;
    run += v;
  }
}

template <typename K>
__global__ __launch_bounds__(TILE_THREADS) void k_scatter(Src src, const ColPlan* __restrict__ plan,
                                                          K* __restrict__ bufA, K* __restrict__ bufB, int64_t ns,
                                                          int pos, const unsigned* __restrict__ cnt, int64_t ntstride,
                                                          K* __restrict__ out) {
  __shared__ unsigned wc[WAVES][256];
  const int c = blockIdx.y;
  const PassState ps = pass_state(plan, c, pos);
  if (!ps.run) return;
  const int64_t n = ps.first ? src.m : ns;
  const int64_t t0 = (int64_t)blockIdx.x * TILE;
  if (t0 >= n) return;
  const K* in = (((ps.nprev - 1) & 1) ? bufB : bufA) + (int64_t)c * ns;
  const bool to_out = ps.last && out != nullptr;
  K* dst = (to_out ? out : ((ps.nprev & 1) ? bufB : bufA)) + (int64_t)c * ns;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t lt_mask = ((uint64_t)1 << lane) - 1;
#pragma unroll
  for (int q = 0; q < WAVES; ++q) wc[q][threadIdx.x] = 0;
  __syncthreads();
  K key[KPT];
  unsigned rk[KPT];
  unsigned active = 0;
  // element order inside a tile: wave, round, lane — the order of the input
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int64_t i = t0 + (int64_t)w * (64 * KPT) + j * 64 + lane;
    bool a = i < n;
    K kk = 0;
    if (a) {
      if (ps.first) {
        bool nan;
        a = in_class(src, i);
        if (a) kk = Key<K>::load(src, c, i, nan);
      } else {
        kk = in[i];
      }
    }
    key[j] = kk;
    const unsigned d = (unsigned)(kk >> (8 * pos)) & 255u;
    uint64_t same = __ballot(a);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bb = __ballot(bit);
      same &= bit ? bb : ~bb;
    }
    const unsigned rank = (unsigned)__popcll(same & lt_mask);
    unsigned base = 0;
    if (a) base = wc[w][d];
    __builtin_amdgcn_wave_barrier();
    if (a && rank == 0) wc[w][d] = base + (unsigned)__popcll(same);
    __builtin_amdgcn_wave_barrier();
    rk[j] = base + rank;
    active |= (unsigned)a << j;
  }
  __syncthreads();
  {  // thread = digit: the tile's base from the scanned table, then the waves in order
    unsigned g = cnt[((int64_t)c * ntstride + blockIdx.x) * 256 + threadIdx.x];
#pragma unroll
    for (int q = 0; q < WAVES; ++q) {
      const unsigned v = wc[q][threadIdx.x];
      wc[q][threadIdx.x] = g;
      g += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (!((active >> j) & 1u)) continue;
    const unsigned d = (unsigned)(key[j] >> (8 * pos)) & 255u;
    const int64_t o = (int64_t)wc[w][d] + rk[j];
    if (o < ns) dst[o] = to_out ? Key<K>::bits(key[j]) : key[j];
  }
}

// ocm_sort_f for a column that is never sorted: all its keys are one key
template <typename K>
__global__ __launch_bounds__(256) void k_fill_equal(const ColPlan* __restrict__ plan, int64_t n, K* __restrict__ out) {
  const int c = blockIdx.y;
  if (plan[c].exec != 0) return;
  const K v = Key<K>::bits((K)plan[c].ckey);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[(int64_t)c * n + i] = v;
}

// #{i < n : f(i) < k} (or ≤ k with `incl`) for an ascending f, n ≥ 1: a binary search with no branch on the
// data (n is the same for every lane)
template <typename K, typename F>
__device__ __forceinline__ int64_t count_below(F f, int64_t n, K k, bool incl) {
  int64_t b = 0, len = n;
  while (len > 1) {
    const int64_t half = len >> 1;
    const K v = f(b + half - 1);
    b = (incl ? v <= k : v < k) ? b + half : b;
    len -= half;
  }
  const K v = f(b);
  return b + ((incl ? v <= k : v < k) ? 1 : 0);
}

// The rows of the class that is not sorted against the sorted side.  The rows
// come in no order, so every step of a search in the whole array is a cache line
// of its own per lane (inferred from timings, not from counters: the rate at which
// the cache hierarchy serves one line per lane, not latency, sets this kernel's
// time).  Hence two levels: the last key of each of ≤ SPLIT buckets of
// `bs` keys (k_splitters) sits in LDS and is searched there, and only the
// ⌈log2 bs⌉ steps inside one bucket (a few adjacent lines) go to memory.
template <typename K>
constexpr int SPLIT = 32768 / sizeof(K);
__host__ __device__ constexpr int64_t bucket_keys(int64_t ns, int split) { return (ns + split - 1) / split; }

// the last key of every bucket, contiguous per column, so that a workgroup fills its LDS with one coalesced read
template <typename K>
__global__ __launch_bounds__(256) void k_splitters(const ColPlan* __restrict__ plan, const K* __restrict__ bufA,
                                                   const K* __restrict__ bufB, int64_t ns, K* __restrict__ spl) {
  const int c = blockIdx.y;
  const int nexec = __popc(plan[c].exec);
  if (nexec == 0) return;
  const K* a = (((nexec - 1) & 1) ? bufB : bufA) + (int64_t)c * ns;
  const int64_t bs = bucket_keys(ns, SPLIT<K>), nb = (ns + bs - 1) / bs;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j < nb) spl[(int64_t)c * SPLIT<K> + j] = a[std::min<int64_t>(ns, (j + 1) * bs) - 1];
}

template <typename K>
__global__ __launch_bounds__(256) void k_auc_search(Src src, const ColPlan* __restrict__ plan,
                                                    const K* __restrict__ bufA, const K* __restrict__ bufB,
                                                    const K* __restrict__ splitters, int64_t ns, int sorted_is_pos,
                                                    unsigned long long* __restrict__ u2) {
  __shared__ K spl[SPLIT<K>];
  __shared__ unsigned long long part[4];
  const int c = blockIdx.y;
  const ColPlan pl = plan[c];
  const int nexec = __popc(pl.exec);
  const K* a = (((nexec - 1) & 1) ? bufB : bufA) + (int64_t)c * ns;
  const K ck = (K)pl.ckey;
  const int64_t pv = ns - (int64_t)pl.nan_s;  // the sorted class without its NaN rows
  const int64_t bs = bucket_keys(ns, SPLIT<K>);  // keys per bucket
  const int64_t nb = (ns + bs - 1) / bs;          // buckets, ≤ SPLIT
  if (nexec != 0) {
    for (int64_t j = threadIdx.x; j < nb; j += 256) spl[j] = splitters[(int64_t)c * SPLIT<K> + j];
    __syncthreads();
  }
  unsigned long long acc = 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < src.m; base += stride) {
    const int64_t r = base + threadIdx.x;
    bool on = r < src.m && !in_class(src, r);
    bool nan = false;
    K k = 0;
    if (on) k = Key<K>::load(src, c, r, nan);
    on = on && !nan;
    int64_t lt, le;
    if (nexec == 0) {
      lt = ck < k ? ns : 0;
      le = ck <= k ? ns : 0;
    } else {
      // two levels: the buckets wholly below k (LDS), then the count inside the next one (memory)
      auto top = [&](int64_t i) { return spl[i]; };
      auto two_level = [&](bool incl) {
        const int64_t o = count_below(top, nb, k, incl) * bs;
        auto in = [&](int64_t i) { return o + i < ns ? a[o + i] : (K) ~(K)0; };
        return std::min<int64_t>(o + count_below(in, bs, k, incl), ns);
      };
      lt = two_level(false);
      // le = lt + the keys equal to k, which follow a[lt]: scores without ties have none or one, and two
      // probes show it; the second search runs only for a wave that holds a row with a longer run
      const K e0 = lt < ns ? a[lt] : (K) ~(K)0, e1 = lt + 1 < ns ? a[lt + 1] : (K) ~(K)0;
      le = lt + (e0 == k ? 1 : 0);
      if (__any(e0 == k && e1 == k)) le = two_level(true);
    }
    if (on) acc += sorted_is_pos ? 2ull * (unsigned long long)(pv - le) + (unsigned long long)(le - lt)
                                 : 2ull * (unsigned long long)lt + (unsigned long long)(le - lt);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long tot = part[0] + part[1] + part[2] + part[3];
    if (tot) atomicAdd(&u2[c], tot);
  }
}

// rows binned by the number of thresholds ≤ s, per class
__global__ __launch_bounds__(256) void k_roc_bins(const void* __restrict__ S, int dtype, int64_t m, int64_t cs,
                                                  int64_t rs, const uint8_t* __restrict__ positive,
                                                  const double* __restrict__ thr, int K,
                                                  unsigned long long* __restrict__ bins) {
  __shared__ unsigned lh[2 * (MAX_THR + 1)];
  const int c = blockIdx.y;
  const double* th = thr + (int64_t)c * K;
  for (int i = threadIdx.x; i < 2 * (K + 1); i += 256) lh[i] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < m; r += stride) {
    const int64_t at = (int64_t)c * cs + r * rs;
    const double v = dtype == 0 ? static_cast<const double*>(S)[at] : (double)static_cast<const float*>(S)[at];
    if (v != v) continue;
    int lo = 0, len = K;  // #thresholds ≤ v
    while (len > 0) {
      const int half = len >> 1;
      if (th[lo + half] <= v) {
        lo += half + 1;
        len -= half + 1;
      } else {
        len = half;
      }
    }
    atomicAdd(&lh[(positive[r] != 0 ? 0 : K + 1) + lo], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * (K + 1); i += 256) {
    const unsigned v = lh[i];
    if (v) atomicAdd(&bins[(int64_t)c * 2 * (K + 1) + i], (unsigned long long)v);
  }
}

// cnt[c][k][cls] = Σ_{j > k} bins[c][cls][j]
__global__ __launch_bounds__(256) void k_roc_suffix(const unsigned long long* __restrict__ bins, int K,
                                                    unsigned long long* __restrict__ cnt) {
  __shared__ unsigned long long tot[256];
  const int c = blockIdx.x, cls = blockIdx.y;
  const unsigned long long* b = bins + ((int64_t)c * 2 + cls) * (K + 1);
  const int per = (K + 256) / 256;  // ⌈(K + 1) / 256⌉ bins j = 1..K per thread, from the top
  const int hi = K - (int)threadIdx.x * per, lo = std::max(hi - per, 0);
  unsigned long long s = 0;
  for (int j = hi; j > lo; --j) s += b[j];
  tot[threadIdx.x] = s;
  __syncthreads();
  unsigned long long run = 0;
  for (int q = 0; q < (int)threadIdx.x; ++q) run += tot[q];
  for (int j = hi; j > lo; --j) {
    run += b[j];
    cnt[((int64_t)c * K + (j - 1)) * 2 + cls] = run;
  }
}

int grid_for(ocm_ctx* ctx, int64_t n, int64_t ncol) {
  int64_t want = std::max<int64_t>(1, (int64_t)ctx->num_cus * 8 / std::max<int64_t>(ncol, 1));
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, want));
}

// Sort the keys of the rows of `src` (its class `want`, n_s of them) of ncg
// columns.  out != NULL: the last executed pass writes values there (ocm_sort_f).
// Leaves the plan and the two key buffers in the workspace for the caller.
struct SortBufs {
  ColPlan* plan = nullptr;
  void* bufA = nullptr;
  void* bufB = nullptr;
  void* spl = nullptr;  // ocm_auc: the bucket splitters, SPLIT keys per column
};

template <typename K>
int sort_group(ocm_ctx* ctx, const Src& src, int ncg, int64_t ns, K* out, long long* nnan_out, SortBufs* sb,
               int* passes_out, hipStream_t st) {
  constexpr int ND = Key<K>::ND;
  const int64_t ntm = (src.m + TILE - 1) / TILE;
  ocm::Carve cv{nullptr};
  auto layout = [&](char* base) {
    cv = ocm::Carve{base};
    sb->plan = cv.take<ColPlan>(ncg);
    unsigned* h0 = cv.take<unsigned>((size_t)ncg * ND * 256);
    unsigned* cnt = cv.take<unsigned>((size_t)ncg * ntm * 256);
    sb->bufA = cv.take<K>((size_t)ncg * ns);
    sb->bufB = cv.take<K>((size_t)ncg * ns);
    sb->spl = out ? nullptr : cv.take<K>((size_t)ncg * SPLIT<K>);
    return std::make_pair(h0, cnt);
  };
  layout(nullptr);
  char* base = static_cast<char*>(ocm::workspace(ctx, cv.off + 256, st));
  auto* hp = static_cast<ColPlan*>(ocm::host_staging(ctx, (size_t)ncg * sizeof(ColPlan)));
  if (!base || !hp) return OCM_ERR_NOMEM;
  auto [h0, cnt] = layout(base);
  K* bufA = static_cast<K*>(sb->bufA);
  K* bufB = static_cast<K*>(sb->bufB);
  // plan and h0 are adjacent carve-outs: one memset
  OCM_HIP(hipMemsetAsync(sb->plan, 0, (size_t)(reinterpret_cast<char*>(cnt) - reinterpret_cast<char*>(sb->plan)), st));
  hipLaunchKernelGGL(k_prehist<K>, dim3(grid_for(ctx, src.m, ncg), ncg), dim3(256), 0, st, src, h0, sb->plan);
  OCM_CHECK_LAUNCH("k_prehist");
  hipLaunchKernelGGL(k_plan<ND>, dim3(ncg), dim3(256), 0, st, h0, sb->plan, nnan_out);
  OCM_CHECK_LAUNCH("k_plan");
  OCM_HIP(hipMemcpyAsync(hp, sb->plan, (size_t)ncg * sizeof(ColPlan), hipMemcpyDeviceToHost, st));
  OCM_HIP(hipStreamSynchronize(st));
  int npass = 0;
  if (ns > 0) {
    const int64_t nts = (ns + TILE - 1) / TILE;
    for (int pos = 0; pos < ND; ++pos) {
      bool any = false, any_first = false;
      for (int c = 0; c < ncg; ++c) {
        if (!((hp[c].exec >> pos) & 1u)) continue;
        any = true;
        if ((hp[c].exec & ((1u << pos) - 1u)) == 0) any_first = true;
      }
      if (!any) continue;
      ++npass;
      const dim3 grid((unsigned)(any_first ? ntm : nts), ncg);
      hipLaunchKernelGGL(k_tile_hist<K>, grid, dim3(TILE_THREADS), 0, st, src, sb->plan, bufA, bufB, ns, pos, cnt, ntm);
      OCM_CHECK_LAUNCH("k_tile_hist");
      hipLaunchKernelGGL(k_scan, dim3(ncg), dim3(SCAN_THREADS), 0, st, sb->plan, cnt, ntm, src.m, ns, pos);
      OCM_CHECK_LAUNCH("k_scan");
      hipLaunchKernelGGL(k_scatter<K>, grid, dim3(TILE_THREADS), 0, st, src, sb->plan, bufA, bufB, ns, pos, cnt, ntm,
                         out);
      OCM_CHECK_LAUNCH("k_scatter");
    }
    if (out) {
      bool any_equal = false;
      for (int c = 0; c < ncg; ++c) any_equal |= hp[c].exec == 0;
      if (any_equal) {
        hipLaunchKernelGGL(k_fill_equal<K>, dim3(grid_for(ctx, ns, ncg), ncg), dim3(256), 0, st, sb->plan, ns, out);
        OCM_CHECK_LAUNCH("k_fill_equal");
      }
    }
  }
  if (passes_out) *passes_out = std::max(*passes_out, npass);
  return OCM_OK;
}

int group_cols(int64_t keys_per_col, int64_t ncol) {
  const int64_t g = std::max<int64_t>(1, GROUP_KEYS / std::max<int64_t>(keys_per_col, 1));
  return (int)std::min<int64_t>(std::min<int64_t>(g, ncol), 65535);
}

thread_local int g_last_passes = 0;

template <typename K>
int sort_f(ocm_ctx* ctx, const char* v, int64_t n, int64_t ncol, int64_t cs, int64_t rs, K* out, hipStream_t st) {
  const int gc = group_cols(n, ncol);
  g_last_passes = 0;
  for (int64_t c0 = 0; c0 < ncol; c0 += gc) {
    const int ncg = (int)std::min<int64_t>(gc, ncol - c0);
    Src src{v + c0 * cs * (int64_t)sizeof(K), cs, rs, n, nullptr, 1, 0};
    SortBufs sb;
    int rc = sort_group<K>(ctx, src, ncg, n, out + c0 * n, nullptr, &sb, &g_last_passes, st);
    if (rc) return rc;
  }
  return OCM_OK;
}

template <typename K>
int auc(ocm_ctx* ctx, const char* S, int64_t m, int64_t ncol, int64_t cs, int64_t rs, const uint8_t* positive,
        int64_t P, int64_t N, unsigned long long* u2, long long* nnan, hipStream_t st) {
  const int sorted_is_pos = P <= N ? 1 : 0;
  const bool degenerate = P == 0 || N == 0;  // nothing to rank: the NaN rows are still counted
  const int64_t ns = degenerate ? 0 : (sorted_is_pos ? P : N);
  const int gc = group_cols(std::max(ns, m / 8), ncol);
  g_last_passes = 0;
  for (int64_t c0 = 0; c0 < ncol; c0 += gc) {
    const int ncg = (int)std::min<int64_t>(gc, ncol - c0);
    Src src{S + c0 * cs * (int64_t)sizeof(K), cs, rs, m, positive, sorted_is_pos, 1};
    SortBufs sb;
    int rc = sort_group<K>(ctx, src, ncg, ns, (K*)nullptr, nnan ? nnan + c0 : nullptr, &sb, &g_last_passes, st);
    if (rc) return rc;
    if (degenerate) continue;
    const K *bufA = static_cast<const K*>(sb.bufA), *bufB = static_cast<const K*>(sb.bufB);
    hipLaunchKernelGGL(k_splitters<K>, dim3(SPLIT<K> / 256, ncg), dim3(256), 0, st, sb.plan, bufA, bufB, ns,
                       static_cast<K*>(sb.spl));
    OCM_CHECK_LAUNCH("k_splitters");
    hipLaunchKernelGGL(k_auc_search<K>, dim3(grid_for(ctx, m, ncg), ncg), dim3(256), 0, st, src, sb.plan, bufA, bufB,
                       static_cast<const K*>(sb.spl), ns, sorted_is_pos, u2 + c0);
    OCM_CHECK_LAUNCH("k_auc_search");
  }
  return OCM_OK;
}

bool strides_ok(int64_t m, int64_t ncol, int64_t cs, int64_t rs) { return cs >= 0 && rs >= 0 && m >= 0 && ncol >= 0; }

}  // namespace

extern "C" {

int ocm_roc_tile_keys(void) { return TILE; }

int ocm_roc_last_passes(void) { return g_last_passes; }

int ocm_sort_f(ocm_ctx* ctx, const void* v, int32_t dtype, int64_t n, int64_t ncol, int64_t col_stride,
               int64_t row_stride, void* out, void* stream) {
  OCM_REQUIRE(ctx != nullptr, "ocm_sort_f: NULL ctx");
  OCM_REQUIRE(dtype == 0 || dtype == 1, "ocm_sort_f: dtype 0 (f64) or 1 (f32)");
  OCM_REQUIRE(strides_ok(n, ncol, col_stride, row_stride), "ocm_sort_f: negative size or stride");
  OCM_REQUIRE(n < ((int64_t)1 << 31), "ocm_sort_f: n < 2^31");
  if (n == 0 || ncol == 0) return OCM_OK;
  OCM_REQUIRE(v && out, "ocm_sort_f: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 0)
    return sort_f<uint64_t>(ctx, static_cast<const char*>(v), n, ncol, col_stride, row_stride,
                            static_cast<uint64_t*>(out), st);
  return sort_f<uint32_t>(ctx, static_cast<const char*>(v), n, ncol, col_stride, row_stride,
                          static_cast<uint32_t*>(out), st);
}

int ocm_auc(ocm_ctx* ctx, const void* S, int32_t dtype, int64_t m, int64_t ncol, int64_t col_stride,
            int64_t row_stride, const uint8_t* positive, uint64_t* u2_out, int64_t* np_out, int64_t* nnan_out,
            void* stream) {
  OCM_REQUIRE(ctx != nullptr, "ocm_auc: NULL ctx");
  OCM_REQUIRE(dtype == 0 || dtype == 1, "ocm_auc: dtype 0 (f64) or 1 (f32)");
  OCM_REQUIRE(strides_ok(m, ncol, col_stride, row_stride), "ocm_auc: negative size or stride");
  OCM_REQUIRE(m < ((int64_t)1 << 31), "ocm_auc: m < 2^31");
  OCM_REQUIRE(np_out && (ncol == 0 || u2_out), "ocm_auc: NULL output");
  hipStream_t st = (hipStream_t)stream;
  OCM_HIP(hipMemsetAsync(np_out, 0, 2 * sizeof(int64_t), st));
  if (ncol) OCM_HIP(hipMemsetAsync(u2_out, 0, (size_t)ncol * sizeof(uint64_t), st));
  if (ncol && nnan_out) OCM_HIP(hipMemsetAsync(nnan_out, 0, (size_t)ncol * sizeof(int64_t), st));
  if (m == 0) return OCM_OK;
  OCM_REQUIRE(positive && (ncol == 0 || S), "ocm_auc: NULL argument");
  auto* hn = static_cast<int64_t*>(ocm::host_staging(ctx, 2 * sizeof(int64_t)));
  if (!hn) return OCM_ERR_NOMEM;
  hipLaunchKernelGGL(k_count_mask, dim3(grid_for(ctx, (m + 7) / 8, 1)), dim3(256), 0, st, positive, m,
                     reinterpret_cast<unsigned long long*>(np_out));
  OCM_CHECK_LAUNCH("k_count_mask");
  OCM_HIP(hipMemcpyAsync(hn, np_out, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  OCM_HIP(hipStreamSynchronize(st));
  const int64_t P = hn[0], N = hn[1];
  if (ncol == 0) return OCM_OK;
  auto* u2 = reinterpret_cast<unsigned long long*>(u2_out);
  auto* nn = reinterpret_cast<long long*>(nnan_out);
  if (dtype == 0)
    return auc<uint64_t>(ctx, static_cast<const char*>(S), m, ncol, col_stride, row_stride, positive, P, N, u2, nn,
                         st);
  return auc<uint32_t>(ctx, static_cast<const char*>(S), m, ncol, col_stride, row_stride, positive, P, N, u2, nn, st);
}

int ocm_roc_counts(ocm_ctx* ctx, const void* S, int32_t dtype, int64_t m, int64_t ncol, int64_t col_stride,
                   int64_t row_stride, const uint8_t* positive, const double* thr, int32_t K, uint64_t* cnt_out,
                   void* stream) {
  OCM_REQUIRE(ctx != nullptr, "ocm_roc_counts: NULL ctx");
  OCM_REQUIRE(dtype == 0 || dtype == 1, "ocm_roc_counts: dtype 0 (f64) or 1 (f32)");
  OCM_REQUIRE(K >= 1 && K <= MAX_THR, "ocm_roc_counts: 1 <= K <= 4096");
  OCM_REQUIRE(strides_ok(m, ncol, col_stride, row_stride), "ocm_roc_counts: negative size or stride");
  OCM_REQUIRE(ncol <= 65535, "ocm_roc_counts: ncol <= 65535");
  if (ncol == 0) return OCM_OK;
  OCM_REQUIRE(thr && cnt_out && (m == 0 || (S && positive)), "ocm_roc_counts: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const size_t nb = (size_t)ncol * 2 * (K + 1) * sizeof(uint64_t);
  auto* bins = static_cast<unsigned long long*>(ocm::workspace(ctx, nb, st));
  if (!bins) return OCM_ERR_NOMEM;
  OCM_HIP(hipMemsetAsync(bins, 0, nb, st));
  if (m > 0) {
    hipLaunchKernelGGL(k_roc_bins, dim3(grid_for(ctx, m, ncol), (unsigned)ncol), dim3(256), 0, st, S, (int)dtype, m,
                       col_stride, row_stride, positive, thr, (int)K, bins);
    OCM_CHECK_LAUNCH("k_roc_bins");
  }
  hipLaunchKernelGGL(k_roc_suffix, dim3((unsigned)ncol, 2), dim3(256), 0, st, bins, (int)K,
                     reinterpret_cast<unsigned long long*>(cnt_out));
  OCM_CHECK_LAUNCH("k_roc_suffix");
  return OCM_OK;
}

}  // extern "C"
