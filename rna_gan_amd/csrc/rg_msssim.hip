// rg_msssim.hip -- MS-SSIM between pairs of uint8 RGB tiles on the device (rna_gan_amd.msssim): the planner, the pyramid launch
// and the pair launch.  include/rnagan_hip.h states the definition and the contract, tests/msssim_refs.py restates it in numpy.
//
//   rg_msssim_pyramid  levels 1 .. S - 1 of every tile as EXACT block sums (uint16: at most 255 * 256 at level 4), once per tile.
//                      A workgroup owns a 32 x 32 block of bytes of one channel of one tile: a lane sums a 2 x 2 block (level 1),
//                      then 64, 16 and 4 lanes sum 2 x 2 blocks of the level before out of LDS.  A pixel of level s exists when its
//                      whole 2^s x 2^s block of bytes does, so bytes outside the tile (read as 0) only reach pixels that are not stored.
//   rg_msssim_pairs    a workgroup owns MS_BAND x MS_COLS window positions of one (pair, level, channel).
//     stage       the (MS_BAND + 10) x (MS_COLS + 10) pixels of both tiles -> LDS as fp32 (a block sum times 4^-s is exact in fp32),
//                 each read from memory once; outside the level: 0.
//     horizontal  a lane takes one staged row and FOUR adjacent output columns: 14 pixels of each tile from LDS, the three products
//                 once per pixel, 11 taps in ascending order into the five moments -> LDS (fp64).
//     vertical    a lane takes one column and TWO adjacent rows: 12 rows x 5 moments from LDS, 11 taps in ascending order, then cs and
//                 l cs of its two positions; positions outside the level's (h - 10) x (w - 10) add nothing.
//     reduction   lane (rows ascending) -> wave (shuffle tree) -> the four waves in order -> ONE partial pair per workgroup in ws;
//                 ms_finish_kernel adds the partials of a (pair, level, channel) in ascending workgroup order and writes out.
//   Everything a result depends on is the bytes of its two tiles: the summation order is fixed by the plan of the SHAPE alone.
//   LDS per workgroup: 2 x 42 x 27 fp32 + 42 x 88 fp64 = 38.6 KB, four workgroups per CU.  The moment rows are padded to 88 doubles:
//   the four row pairs a wave reads in the vertical pass then start 32 banks apart, two by two.
// No 16-bit float type is involved: both builds behave identically.
#include "rg_common.h"

namespace {

constexpr int MS_BAND = RG_MSSSIM_BAND, MS_COLS = RG_MSSSIM_COLS;
constexpr int MS_TAPS = 11, MS_HALO = MS_TAPS - 1;
constexpr int MS_IR = MS_BAND + MS_HALO, MS_IC = MS_COLS + MS_HALO;     // staged rows and columns: 42 x 26
constexpr int MS_SSTR = MS_IC + 1;                                      // row stride of the staged pixels (fp32)
constexpr int MS_HROW = 5 * MS_COLS + 8;                                // row stride of the moments (fp64): [row][moment][column]
constexpr int MS_SMAX = 5;
constexpr int MS_DIMMAX = 4096;
constexpr double MS_C1 = (0.01 * 255.0) * (0.01 * 255.0), MS_C2 = (0.03 * 255.0) * (0.03 * 255.0);
static_assert(MS_COLS % 4 == 0 && MS_BAND % 2 == 0 && MS_IR * (MS_COLS / 4) <= 256 && (MS_BAND / 2) * MS_COLS == 256,
              "the lane maps of ms_pair_kernel");

struct ms_plan {
  int S;
  int h[MS_SMAX], w[MS_SMAX];         // extents of the levels
  int nbr[MS_SMAX], nbc[MS_SMAX];     // bands and column tiles of a level
  int blk0[MS_SMAX + 1];              // the first workgroup of a level within a pair; blk0[S]: workgroups per pair
  long long off[MS_SMAX];             // where level s >= 1 starts in a tile's pyramid, in uint16 elements
  long long tile_elems;               // uint16 elements of a tile's pyramid
};
struct ms_taps { double g[MS_TAPS]; };

// shape and S -> plan; what is refused here is refused by every entry point
int ms_make_plan(const char* what, int H, int W, int S, ms_plan* pl) {
  RG_REQUIRE(H >= MS_TAPS && W >= MS_TAPS, RG_EINVAL, "%s: H %d x W %d is below %d x %d", what, H, W, MS_TAPS, MS_TAPS);
  RG_REQUIRE(S >= 1 && S <= MS_SMAX, RG_EINVAL, "%s: S %d is not in 1..%d", what, S, MS_SMAX);
  RG_REQUIRE(((H < W ? H : W) >> (S - 1)) >= MS_TAPS, RG_EINVAL, "%s: S %d is too deep for H %d x W %d (the last level needs %d pixels)",
             what, S, H, W, MS_TAPS);
  RG_REQUIRE(H <= MS_DIMMAX && W <= MS_DIMMAX, RG_EUNSUPPORTED, "%s: H %d x W %d is more than %d", what, H, W, MS_DIMMAX);
  pl->S = S;
  pl->blk0[0] = 0;
  long long off = 0;
  for (int s = 0; s < MS_SMAX; ++s) {
    const bool on = s < S;
    pl->h[s] = on ? H >> s : 0;
    pl->w[s] = on ? W >> s : 0;
    pl->nbr[s] = on ? (pl->h[s] - MS_HALO + MS_BAND - 1) / MS_BAND : 0;
    pl->nbc[s] = on ? (pl->w[s] - MS_HALO + MS_COLS - 1) / MS_COLS : 0;
    pl->blk0[s + 1] = pl->blk0[s] + 3 * pl->nbr[s] * pl->nbc[s];          // at most 3 * 128 * 256 * 4 / 3
    pl->off[s] = off;
    if (on && s >= 1) off += 3LL * pl->h[s] * pl->w[s];
  }
  pl->tile_elems = off;
  return RG_OK;
}

__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ the pyramid
// grid: N * 3 * gy * gx workgroups; workgroup b: block column b % gx, block row (b / gx) % gy, channel (b / gx / gy) % 3, tile the rest
__global__ __launch_bounds__(256) void ms_pyr_kernel(const uint8_t* __restrict__ tiles, int H, int W, int planar, int reverse, ms_plan pl,
                                                     uint16_t* __restrict__ pyr, unsigned gx, unsigned gy) {
  __shared__ unsigned s1[16][16], s2[8][8], s3[4][4];
  const int tid = threadIdx.x;
  unsigned b = blockIdx.x;
  const int bx = (int)(b % gx);
  b /= gx;
  const int by = (int)(b % gy);
  b /= gy;
  const int ch = (int)(b % 3u);
  const size_t n = b / 3u;
  const int sc = reverse ? 2 - ch : ch;
  const size_t HW = (size_t)H * (size_t)W;
  const uint8_t* src = tiles + n * HW * 3 + (planar ? (size_t)sc * HW : (size_t)sc);
  const size_t pstep = planar ? 1 : 3;
  uint16_t* dst = pyr + n * (size_t)pl.tile_elems;
  {
    const int ty = tid >> 4, tx = tid & 15, y = by * 16 + ty, x = bx * 16 + tx;
    unsigned v = 0;
    if (y < pl.h[1] && x < pl.w[1]) {
      const uint8_t* p = src + ((size_t)(2 * y) * (size_t)W + (size_t)(2 * x)) * pstep;
      v = (unsigned)p[0] + (unsigned)p[pstep] + (unsigned)p[(size_t)W * pstep] + (unsigned)p[((size_t)W + 1) * pstep];
      dst[(size_t)pl.off[1] + ((size_t)ch * pl.h[1] + y) * (size_t)pl.w[1] + x] = (uint16_t)v;
    }
    s1[ty][tx] = v;
  }
  __syncthreads();
  if (tid < 64) {
    const int ty = tid >> 3, tx = tid & 7, y = by * 8 + ty, x = bx * 8 + tx;
    const unsigned v = s1[2 * ty][2 * tx] + s1[2 * ty][2 * tx + 1] + s1[2 * ty + 1][2 * tx] + s1[2 * ty + 1][2 * tx + 1];
    s2[ty][tx] = v;
    if (pl.S > 2 && y < pl.h[2] && x < pl.w[2]) dst[(size_t)pl.off[2] + ((size_t)ch * pl.h[2] + y) * (size_t)pl.w[2] + x] = (uint16_t)v;
  }
  __syncthreads();
  if (tid < 16) {
    const int ty = tid >> 2, tx = tid & 3, y = by * 4 + ty, x = bx * 4 + tx;
    const unsigned v = s2[2 * ty][2 * tx] + s2[2 * ty][2 * tx + 1] + s2[2 * ty + 1][2 * tx] + s2[2 * ty + 1][2 * tx + 1];
    s3[ty][tx] = v;
    if (pl.S > 3 && y < pl.h[3] && x < pl.w[3]) dst[(size_t)pl.off[3] + ((size_t)ch * pl.h[3] + y) * (size_t)pl.w[3] + x] = (uint16_t)v;
  }
  __syncthreads();
  if (tid < 4) {
    const int ty = tid >> 1, tx = tid & 1, y = by * 2 + ty, x = bx * 2 + tx;
    const unsigned v = s3[2 * ty][2 * tx] + s3[2 * ty][2 * tx + 1] + s3[2 * ty + 1][2 * tx] + s3[2 * ty + 1][2 * tx + 1];
    if (pl.S > 4 && y < pl.h[4] && x < pl.w[4]) dst[(size_t)pl.off[4] + ((size_t)ch * pl.h[4] + y) * (size_t)pl.w[4] + x] = (uint16_t)v;
  }
}

// ------------------------------------------------------------------------------------------------ the pairs
// one tile's share of the staging: level s, channel ch, rows r0 .., columns c0 .. -> dst[MS_IR][MS_SSTR]
__device__ __forceinline__ void ms_stage(float (*dst)[MS_SSTR], const uint8_t* __restrict__ tiles, const uint16_t* __restrict__ pyr,
                                         size_t n, int H, int W, int planar, int reverse, const ms_plan& pl, int s, int ch, int r0,
                                         int c0, int hs, int wd) {
  const int tid = threadIdx.x;
  if (s == 0) {
    const int sc = reverse ? 2 - ch : ch;
    const size_t HW = (size_t)H * (size_t)W;
    const uint8_t* src = tiles + n * HW * 3 + (planar ? (size_t)sc * HW : (size_t)sc);
    const size_t pstep = planar ? 1 : 3;
    for (int i = tid; i < MS_IR * MS_IC; i += 256) {
      const int rr = i / MS_IC, cc = i - rr * MS_IC, y = r0 + rr, x = c0 + cc;
      float v = 0.f;
      if (y < hs && x < wd) v = (float)src[((size_t)y * (size_t)W + (size_t)x) * pstep];
      dst[rr][cc] = v;
    }
  } else {
    const uint16_t* src = pyr + n * (size_t)pl.tile_elems + (size_t)pl.off[s] + (size_t)ch * (size_t)hs * (size_t)wd;
    const float scale = ldexpf(1.f, -2 * s);
    for (int i = tid; i < MS_IR * MS_IC; i += 256) {
      const int rr = i / MS_IC, cc = i - rr * MS_IC, y = r0 + rr, x = c0 + cc;
      float v = 0.f;
      if (y < hs && x < wd) v = (float)src[(size_t)y * (size_t)wd + (size_t)x] * scale;     // exact: 16 bits times a power of two
      dst[rr][cc] = v;
    }
  }
}

// grid: P * blk0[S] workgroups; workgroup b: pair b / blk0[S]; within the pair level by level, channel, band, column tile.
// ws[2 b], ws[2 b + 1]: the workgroup's sums of cs and l cs.
__global__ __launch_bounds__(256) void ms_pair_kernel(const uint8_t* __restrict__ a, const uint16_t* __restrict__ pa, int Na,
                                                      const uint8_t* __restrict__ b, const uint16_t* __restrict__ pb, int Nb,
                                                      const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, int H, int W,
                                                      int planar, int reverse, ms_plan pl, ms_taps tp, double* __restrict__ ws) {
  __shared__ float sx[MS_IR][MS_SSTR], sy[MS_IR][MS_SSTR];
  __shared__ double hm[MS_IR][MS_HROW];
  __shared__ double red[4][2];
  const int tid = threadIdx.x;
  const unsigned per = (unsigned)pl.blk0[pl.S];
  const unsigned pair = blockIdx.x / per;
  int rem = (int)(blockIdx.x % per);
  int s = 0;
  while (s + 1 < pl.S && rem >= pl.blk0[s + 1]) ++s;
  rem -= pl.blk0[s];
  const int hs = pl.h[s], wd = pl.w[s], nbc = pl.nbc[s], nb = pl.nbr[s] * nbc;
  const int ch = rem / nb, k = rem - ch * nb;
  const int r0 = (k / nbc) * MS_BAND, c0 = (k % nbc) * MS_COLS;
  const int na = ia[pair], nbi = ib[pair];
  double* slot = ws + 2 * (size_t)blockIdx.x;
  if (na < 0 || na >= Na || nbi < 0 || nbi >= Nb) {                      // never an address: the pair's sums become NaN
    if (tid == 0) { slot[0] = __longlong_as_double(0x7ff8000000000000LL); slot[1] = slot[0]; }
    return;
  }
  ms_stage(sx, a, pa, (size_t)na, H, W, planar, reverse, pl, s, ch, r0, c0, hs, wd);
  ms_stage(sy, b, pb, (size_t)nbi, H, W, planar, reverse, pl, s, ch, r0, c0, hs, wd);
  __syncthreads();
  // horizontal: lane = (staged row r, columns 4 q .. 4 q + 3)
  if (tid < MS_IR * (MS_COLS / 4)) {
    const int r = tid / (MS_COLS / 4), q = tid - r * (MS_COLS / 4);
    double acc[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
    for (int i = 0; i < MS_TAPS + 3; ++i) {
      const double xv = (double)sx[r][4 * q + i], yv = (double)sy[r][4 * q + i];
      const double xx = xv * xv, yy = yv * yv, xy = xv * yv;             // exact: integers below 2^32 times a power of two
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int j = i - o;
        if (j >= 0 && j < MS_TAPS) {
          const double g = tp.g[j];
          acc[o][0] = fma(g, xv, acc[o][0]);
          acc[o][1] = fma(g, yv, acc[o][1]);
          acc[o][2] = fma(g, xx, acc[o][2]);
          acc[o][3] = fma(g, yy, acc[o][3]);
          acc[o][4] = fma(g, xy, acc[o][4]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int o = 0; o < 4; ++o) hm[r][m * MS_COLS + 4 * q + o] = acc[o][m];
  }
  __syncthreads();
  // vertical: lane = (column col, rows 2 rg and 2 rg + 1)
  double tcs = 0.0, tl = 0.0;
  {
    const int col = tid & (MS_COLS - 1), rg = tid / MS_COLS;
    double acc[2][5];
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
      for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
#pragma unroll
    for (int i = 0; i < MS_TAPS + 1; ++i) {
      double v[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) v[m] = hm[2 * rg + i][m * MS_COLS + col];
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        const int j = i - o;
        if (j >= 0 && j < MS_TAPS) {
          const double g = tp.g[j];
#pragma unroll
          for (int m = 0; m < 5; ++m) acc[o][m] = fma(g, v[m], acc[o][m]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const double mx = acc[o][0], my = acc[o][1];
      const double mxx = mx * mx, myy = my * my, mxy = mx * my;
      const double vx = acc[o][2] - mxx, vy = acc[o][3] - myy, cxy = acc[o][4] - mxy;
      const double cs = (2.0 * cxy + MS_C2) / (vx + vy + MS_C2);
      const double l = (2.0 * mxy + MS_C1) / (mxx + myy + MS_C1);
      const bool in = r0 + 2 * rg + o < hs - MS_HALO && c0 + col < wd - MS_HALO;
      tcs += in ? cs : 0.0;
      tl += in ? l * cs : 0.0;
    }
  }
  tcs = ms_wave_sum(tcs);
  tl = ms_wave_sum(tl);
  if ((tid & 63) == 0) { red[tid >> 6][0] = tcs; red[tid >> 6][1] = tl; }
  __syncthreads();
  if (tid == 0) {
    slot[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    slot[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
}

// one lane per (pair, level, channel): its workgroups' partials in ascending order, from 0.0 -> out[P][S][3][2]
__global__ __launch_bounds__(256) void ms_finish_kernel(const double* __restrict__ ws, ms_plan pl, long long entries,
                                                        double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  const int ch = (int)(e % 3), s = (int)((e / 3) % pl.S);
  const long long pair = e / (3LL * pl.S);
  const int nb = pl.nbr[s] * pl.nbc[s];
  const double* p = ws + 2 * ((size_t)pair * (size_t)pl.blk0[pl.S] + (size_t)pl.blk0[s] + (size_t)ch * (size_t)nb);
  double cs = 0.0, l = 0.0;
  for (int k = 0; k < nb; ++k) {
    cs = cs + p[2 * k];
    l = l + p[2 * k + 1];
  }
  out[2 * e] = cs;
  out[2 * e + 1] = l;
}

int ms_flags(const char* what, int flags) {
  RG_REQUIRE((flags & ~(RG_EXPORT_PLANAR | RG_EXPORT_REVERSE)) == 0, RG_EINVAL, "%s: unknown flag bits 0x%x", what, flags);
  return RG_OK;
}

}  // namespace

extern "C" int rg_msssim_plan(int H, int W, int S, int P, int32_t* info, size_t* pyramid_tile_bytes, size_t* pair_ws_bytes) {
  ms_plan pl;
  const int rc = ms_make_plan("msssim_plan", H, W, S, &pl);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(P >= 0, RG_EINVAL, "msssim_plan: P %d is negative", P);
  RG_REQUIRE((long long)P * pl.blk0[S] <= 0x7fffffffLL, RG_EUNSUPPORTED, "msssim_plan: P %d x %d workgroups per pair is more than 2^31 - 1",
             P, pl.blk0[S]);
  if (info) {
    info[0] = MS_BAND;
    info[1] = MS_COLS;
    for (int s = 0; s < S; ++s) { info[2 + 2 * s] = pl.h[s]; info[3 + 2 * s] = pl.w[s]; }
  }
  if (pyramid_tile_bytes) *pyramid_tile_bytes = (size_t)pl.tile_elems * sizeof(uint16_t);
  if (pair_ws_bytes) *pair_ws_bytes = (size_t)P * (size_t)pl.blk0[S] * 2 * sizeof(double);
  return RG_OK;
}

extern "C" int rg_msssim_pyramid(const uint8_t* tiles, int N, int H, int W, int flags, int S, void* pyr, size_t pyr_bytes, void* stream) {
  ms_plan pl;
  int rc = ms_make_plan("msssim_pyramid", H, W, S, &pl);
  if (rc != RG_OK || (rc = ms_flags("msssim_pyramid", flags)) != RG_OK) return rc;
  RG_REQUIRE(N >= 0, RG_EINVAL, "msssim_pyramid: N %d is negative", N);
  RG_REQUIRE(tiles && (pyr || S == 1), RG_EINVAL, "msssim_pyramid: NULL buffer");
  RG_REQUIRE(((uintptr_t)pyr & 1) == 0, RG_EINVAL, "msssim_pyramid: pyr needs 2-byte alignment");
  RG_REQUIRE(pyr_bytes / sizeof(uint16_t) / (size_t)(N > 0 ? N : 1) >= (size_t)pl.tile_elems, RG_EWORKSPACE,
             "msssim_pyramid: pyr of %zu bytes, %zu needed", pyr_bytes, (size_t)N * (size_t)pl.tile_elems * sizeof(uint16_t));
  if (N == 0 || S == 1) return RG_OK;
  const unsigned gx = (unsigned)((W + 31) / 32), gy = (unsigned)((H + 31) / 32);
  const long long blocks = (long long)N * 3 * gx * gy;
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "msssim_pyramid: N %d H %d W %d is more than 2^31 - 1 workgroups", N, H, W);
  hipLaunchKernelGGL(ms_pyr_kernel, dim3((unsigned)blocks), dim3(256), 0, rg_stream(stream), tiles, H, W,
                     (flags & RG_EXPORT_PLANAR) != 0, (flags & RG_EXPORT_REVERSE) != 0, pl, (uint16_t*)pyr, gx, gy);
  RG_LAUNCH_CHECK("msssim_pyramid");
  return RG_OK;
}

extern "C" int rg_msssim_pairs(const uint8_t* a, const void* pyr_a, int Na, const uint8_t* b, const void* pyr_b, int Nb,
                               const int32_t* ia, const int32_t* ib, int P, int H, int W, int flags, int S, const double* taps, void* ws,
                               size_t ws_bytes, double* out, void* stream) {
  ms_plan pl;
  int rc = ms_make_plan("msssim_pairs", H, W, S, &pl);
  if (rc != RG_OK || (rc = ms_flags("msssim_pairs", flags)) != RG_OK) return rc;
  RG_REQUIRE(P >= 0, RG_EINVAL, "msssim_pairs: P %d is negative", P);
  if (P == 0) return RG_OK;
  RG_REQUIRE(a && b && ia && ib && taps && out, RG_EINVAL, "msssim_pairs: NULL buffer");
  RG_REQUIRE(S == 1 || (pyr_a && pyr_b), RG_EINVAL, "msssim_pairs: NULL pyramid with S %d", S);
  RG_REQUIRE(Na >= 1 && Nb >= 1, RG_EINVAL, "msssim_pairs: Na %d or Nb %d is below 1", Na, Nb);
  RG_REQUIRE((((uintptr_t)pyr_a | (uintptr_t)pyr_b) & 1) == 0 && (((uintptr_t)ia | (uintptr_t)ib) & 3) == 0 && ((uintptr_t)out & 7) == 0,
             RG_EINVAL, "msssim_pairs: the pyramids need 2-byte, the index arrays 4-byte and out 8-byte alignment");
  const long long blocks = (long long)P * pl.blk0[S];
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "msssim_pairs: P %d x %d workgroups per pair is more than 2^31 - 1", P, pl.blk0[S]);
  const size_t need = (size_t)blocks * 2 * sizeof(double);
  RG_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= need, RG_EWORKSPACE, "msssim_pairs: workspace of %zu bytes, %zu needed (8-byte aligned)",
             ws ? ws_bytes : (size_t)0, need);
  ms_taps tp;
  for (int j = 0; j < MS_TAPS; ++j) tp.g[j] = taps[j];
  hipStream_t st = rg_stream(stream);
  hipLaunchKernelGGL(ms_pair_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, (const uint16_t*)pyr_a, Na, b, (const uint16_t*)pyr_b, Nb,
                     ia, ib, H, W, (flags & RG_EXPORT_PLANAR) != 0, (flags & RG_EXPORT_REVERSE) != 0, pl, tp, (double*)ws);
  RG_LAUNCH_CHECK("msssim_pairs");
  const long long entries = (long long)P * S * 3;
  hipLaunchKernelGGL(ms_finish_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, (const double*)ws, pl, entries, out);
  RG_LAUNCH_CHECK("msssim_pairs");
  return RG_OK;
}
