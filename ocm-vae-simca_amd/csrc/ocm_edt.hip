// Mask morphology (include/ocm.h, "mask morphology"): the exact squared
// Euclidean distance transform of an H × W byte mask, from which erosion and
// dilation by a disc, opening, closing and the depth of a pixel inside its
// object all follow (ocm/image.py).
//
//   d2(y, x) = min over x' of (x − x')² + g(y, x')²,
//   g(y, x)  = the vertical distance from (y, x) to the nearest background
//              pixel of column x (0 on background, "none" without one).
//
// Three launches, whatever the image holds:
//   1 k_edt_pack  the background bits of a column, EDT_BH = 64 rows to a word:
//                 a thread takes VEC adjacent columns of one band, so the 64
//                 loads of a lane are independent and a wave's are coalesced
//                 (4 mask bytes per lane when W and the pointer allow, single
//                 bytes otherwise).
//   2 k_edt_cols  g from those words: the nearest set bit below and above a row
//                 is a count of leading / trailing zeros, and a band without
//                 one looks through the words of the bands above / below until
//                 it meets one.  No sweep along H: H/64 · W threads, each with
//                 O(1) work per pixel, so a narrow image still fills the chip.
//                 g is uint16, EDT_NONE16 for "none in this column".
//   3 k_edt_rows  one workgroup per row.  The row's g and the minimum of every
//                 EDT_SEG = 64 columns are staged in LDS; every pixel scans
//                 outwards from x, first left, then right, and stops once
//                 (x − x')² reaches the best so far.  At a segment's near edge
//                 it skips the segment whole when (distance to the edge)² +
//                 (segment minimum)² cannot improve the best: columns without
//                 any background cost one test per 64.
// Exact (every candidate that is passed over is bounded below by the best), in
// integers (H, W ≤ 32767 keep every sum below 2³¹), and O(H·W·min(R, W)) for
// objects of radius R: the outward scan visits about R columns per side.  No
// atomics, no host synchronisation, no workgroup waits for another.
#include "ocm_internal.h"

namespace {

constexpr int EDT_BH = 64;    // rows per band: one bit each in a 64-bit word
constexpr int EDT_SEG = 64;   // columns per segment of the row pass: one wave stages it and takes its minimum
constexpr int EDT_NT = 256;   // threads per workgroup
constexpr int EDT_MAX = 32767;           // largest H or W
constexpr unsigned EDT_NONE16 = 0xffffu;  // g: no background in this column
constexpr int EDT_FAR = 1 << 20;          // a row further than any image is high
// dynamic LDS of the row pass at the widest row: g and the segment minima, 2 bytes each
constexpr int EDT_LDS_MAX = ((EDT_MAX + EDT_SEG) / EDT_SEG * EDT_SEG + (EDT_MAX + EDT_SEG) / EDT_SEG) * 2;

typedef unsigned long long u64;
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// grid (column groups, bands); thread: VEC adjacent columns of one band
template <int VEC>
__global__ __launch_bounds__(EDT_NT) void k_edt_pack(const uint8_t* __restrict__ mask, int H, int W, int invert,
                                                     u64* __restrict__ bits) {
  const int x = (blockIdx.x * EDT_NT + threadIdx.x) * VEC;
  if (x >= W) return;
  const int b = blockIdx.y, y0 = b * EDT_BH;
  const int rows = H - y0 < EDT_BH ? H - y0 : EDT_BH;
  const uint8_t* src = mask + (int64_t)y0 * W + x;
  u64 w[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) w[e] = 0;
#pragma unroll 16
  for (int r = 0; r < EDT_BH; ++r) {
    // rows past the image read the band's last row again (the load stays unconditional) and set no bit
    const uint8_t* p = src + (int64_t)(r < rows ? r : rows - 1) * W;
    const u64 in = r < rows;
    if constexpr (VEC == 4) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] |= (in & (u64)((((v >> (8 * e)) & 0xffu) != 0) == (invert != 0))) << r;
    } else {
      w[0] |= (in & (u64)((*p != 0) == (invert != 0))) << r;
    }
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) bits[(int64_t)b * W + x + e] = w[e];
}

template <int VEC>
__global__ __launch_bounds__(EDT_NT) void k_edt_cols(const u64* __restrict__ bits, int H, int W, int nb, int border,
                                                     uint16_t* __restrict__ g) {
  const int x = (blockIdx.x * EDT_NT + threadIdx.x) * VEC;
  if (x >= W) return;
  const int b = blockIdx.y, y0 = b * EDT_BH;
  const int rows = H - y0 < EDT_BH ? H - y0 : EDT_BH;
  u64 w[VEC];
  int up[VEC], down[VEC];  // the nearest background rows outside the band
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    w[e] = bits[(int64_t)b * W + x + e];
    up[e] = border ? -1 : -EDT_FAR;
    down[e] = border ? H : EDT_FAR;
    if (!(w[e] & 1ull)) {  // the band's first row looks above the band
      for (int bb = b - 1; bb >= 0; --bb) {
        const u64 v = bits[(int64_t)bb * W + x + e];
        if (v) {
          up[e] = bb * EDT_BH + 63 - __clzll((long long)v);
          break;
        }
      }
    }
    if (!((w[e] >> (rows - 1)) & 1ull)) {  // and its last row below
      for (int bb = b + 1; bb < nb; ++bb) {
        const u64 v = bits[(int64_t)bb * W + x + e];
        if (v) {
          down[e] = bb * EDT_BH + __ffsll((long long)v) - 1;
          break;
        }
      }
    }
  }
  uint16_t* dst = g + (int64_t)y0 * W + x;
  for (int r = 0; r < rows; ++r) {
    unsigned short out[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const u64 lo = w[e] & ((1ull << r) - 1ull), hi = (w[e] >> r) >> 1;
      const int da = lo ? r - (63 - __clzll((long long)lo)) : y0 + r - up[e];
      const int db = hi ? __ffsll((long long)hi) : down[e] - (y0 + r);
      int d = da < db ? da : db;
      if (d > (int)EDT_NONE16) d = (int)EDT_NONE16;
      out[e] = (unsigned short)(((w[e] >> r) & 1ull) ? 0 : d);
    }
    if constexpr (VEC == 4) {
      u16x4 v = {out[0], out[1], out[2], out[3]};
      *reinterpret_cast<u16x4*>(dst + (int64_t)r * W) = v;
    } else {
      dst[(int64_t)r * W] = out[0];
    }
  }
}

// grid H; LDS: the row's g padded to whole segments, then one minimum per segment
__global__ __launch_bounds__(EDT_NT) void k_edt_rows(const uint16_t* __restrict__ g, int W, int flags, int64_t r2,
                                                     int* __restrict__ d2_out, uint8_t* __restrict__ mask_out) {
  extern __shared__ unsigned short edt_row[];
  const int Wp = (W + EDT_SEG - 1) / EDT_SEG * EDT_SEG;
  unsigned short* segmin = edt_row + Wp;
  const int lane = threadIdx.x & 63;
  const int64_t base = (int64_t)blockIdx.x * W;
  for (int i = threadIdx.x; i < Wp; i += EDT_NT) {  // whole waves: Wp and EDT_NT are multiples of 64
    const unsigned v = i < W ? g[base + i] : EDT_NONE16;
    edt_row[i] = (unsigned short)v;
    unsigned m = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned n = __shfl_xor(m, o, 64);
      m = n < m ? n : m;
    }
    if (lane == 0) segmin[i / EDT_SEG] = (unsigned short)m;
  }
  __syncthreads();
  const bool border = flags & OCM_EDT_BORDER_BG, inv_out = flags & OCM_EDT_INVERT_OUT;
  constexpr unsigned NONE = (unsigned)OCM_EDT_NONE;
  for (int x = threadIdx.x; x < W; x += EDT_NT) {
    const unsigned g0 = edt_row[x];
    unsigned best = g0 == EDT_NONE16 ? NONE : g0 * g0;
    if (border) {
      const unsigned l = (unsigned)(x + 1) * (unsigned)(x + 1), r = (unsigned)(W - x) * (unsigned)(W - x);
      best = l < best ? l : best;
      best = r < best ? r : best;
    }
    for (int xl = x - 1; xl >= 0;) {
      const unsigned dx = (unsigned)(x - xl), dx2 = dx * dx;
      if (dx2 >= best) break;
      if ((xl & (EDT_SEG - 1)) == EDT_SEG - 1) {  // the near edge of a segment: can any of its columns improve?
        const unsigned s = segmin[xl / EDT_SEG];
        if (s == EDT_NONE16 || dx2 + s * s >= best) {
          xl -= EDT_SEG;
          continue;
        }
      }
      const unsigned v = edt_row[xl];
      if (v != EDT_NONE16) {
        const unsigned c = dx2 + v * v;
        best = c < best ? c : best;
      }
      --xl;
    }
    for (int xr = x + 1; xr < W;) {
      const unsigned dx = (unsigned)(xr - x), dx2 = dx * dx;
      if (dx2 >= best) break;
      if ((xr & (EDT_SEG - 1)) == 0) {
        const unsigned s = segmin[xr / EDT_SEG];
        if (s == EDT_NONE16 || dx2 + s * s >= best) {
          xr += EDT_SEG;
          continue;
        }
      }
      const unsigned v = edt_row[xr];
      if (v != EDT_NONE16) {
        const unsigned c = dx2 + v * v;
        best = c < best ? c : best;
      }
      ++xr;
    }
    if (d2_out) d2_out[base + x] = (int)best;
    if (mask_out) {
      const bool in = best == NONE || (int64_t)best > r2;  // no background anywhere: deeper than any radius
      mask_out[base + x] = (uint8_t)(in != inv_out);
    }
  }
}

inline bool aligned_to(const void* ptr, size_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int ocm_edt_u8(ocm_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t flags, int64_t r2, int32_t* d2_out,
               uint8_t* mask_out, void* stream) {
  OCM_REQUIRE(H >= 1 && W >= 1, "ocm_edt_u8: H and W must be at least 1");
  OCM_REQUIRE(H <= EDT_MAX && W <= EDT_MAX, "ocm_edt_u8: H and W must be at most 32767");
  OCM_REQUIRE((flags & ~(OCM_EDT_BORDER_BG | OCM_EDT_INVERT_IN | OCM_EDT_INVERT_OUT)) == 0,
              "ocm_edt_u8: unknown flag bits");
  OCM_REQUIRE(r2 >= 0, "ocm_edt_u8: r2 must not be negative");
  OCM_REQUIRE(d2_out || mask_out, "ocm_edt_u8: d2_out and mask_out are both NULL");
  OCM_REQUIRE(ctx && mask, "ocm_edt_u8: NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (H + EDT_BH - 1) / EDT_BH;
  const size_t HW = (size_t)H * W, nbits = (size_t)nb * W;
  ocm::Carve cv{static_cast<char*>(ocm::workspace(ctx, nbits * sizeof(u64) + HW * sizeof(uint16_t) + 512, st))};
  if (!cv.base) return OCM_ERR_NOMEM;
  u64* bits = cv.take<u64>(nbits);
  uint16_t* g = cv.take<uint16_t>(HW);
  const int invert = (flags & OCM_EDT_INVERT_IN) != 0, border = (flags & OCM_EDT_BORDER_BG) != 0;
  if (W % 4 == 0 && aligned_to(mask, 4)) {
    const dim3 grid((unsigned)((W / 4 + EDT_NT - 1) / EDT_NT), (unsigned)nb);
    hipLaunchKernelGGL(k_edt_pack<4>, grid, dim3(EDT_NT), 0, st, mask, H, W, invert, bits);
    OCM_CHECK_LAUNCH("k_edt_pack");
    hipLaunchKernelGGL(k_edt_cols<4>, grid, dim3(EDT_NT), 0, st, bits, H, W, nb, border, g);
  } else {
    const dim3 grid((unsigned)((W + EDT_NT - 1) / EDT_NT), (unsigned)nb);
    hipLaunchKernelGGL(k_edt_pack<1>, grid, dim3(EDT_NT), 0, st, mask, H, W, invert, bits);
    OCM_CHECK_LAUNCH("k_edt_pack");
    hipLaunchKernelGGL(k_edt_cols<1>, grid, dim3(EDT_NT), 0, st, bits, H, W, nb, border, g);
  }
  OCM_CHECK_LAUNCH("k_edt_cols");
  static int lds_ok[64] = {0};  // per device: the attribute is set once, for the widest row
  if (!lds_ok[ctx->device & 63]) {
    OCM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_edt_rows), hipFuncAttributeMaxDynamicSharedMemorySize,
                                EDT_LDS_MAX));
    lds_ok[ctx->device & 63] = 1;
  }
  const int nseg = (W + EDT_SEG - 1) / EDT_SEG;
  const size_t dyn = (size_t)(nseg * EDT_SEG + nseg) * sizeof(unsigned short);
  hipLaunchKernelGGL(k_edt_rows, dim3((unsigned)H), dim3(EDT_NT), dyn, st, g, W, flags, r2, d2_out, mask_out);
  OCM_CHECK_LAUNCH("k_edt_rows");
  return OCM_OK;
}

}  // extern "C"
