// rg_tiler.hip -- the tiler's device half (rna_gan_amd.tiler): windows of a slide raster resized as Pillow's 8-bit Image.resize does
// (rg_window_resize_u8), the erosion that closes the thumbnail's tissue mask (rg_mask_erode), and a box thumbnail for a raster that
// brings no pyramid level (rg_box_reduce_u8).  Integer arithmetic only: include/rnagan_hip.h states the contracts, tests/tiler_refs.py
// restates them, and every byte is demanded equal.  No 16-bit type is involved.
//
// rg_window_resize_u8, one launch: a workgroup (4 waves) owns a WR_BH x WR_BW block of output pixels of ONE window.
//   bounds   (xmin, count) of the block's 32 output columns and 32 output rows go to LDS, clamped (a table that is not Pillow's can
//            give wrong bytes, never an access outside LDS, the tables or the raster); from them the source columns
//            [c_lo, c_lo + ncols) and source rows [r_lo, r_lo + nrows) the block needs, cut to the LDS the launch brought.
//   strips   WR_SR source rows at a time.  Load: a wave takes a row, a lane its bytes, each byte read from the raster once (a pixel
//            outside the raster reads as 0; byte offsets into the raster are 64-bit).  HORIZONTAL pass: a wave takes an output
//            column, so the table row it walks is wave-uniform (the coefficients come through scalar loads, the loop bound is
//            scalar); its lanes are the strip's 21 rows x 3 channels.  One byte per (source row, output column, channel) goes
//            into the LDS intermediate `mid` -- rounded and clipped to a byte as the contract demands.
//   vertical a wave takes an output row (uniform table row again), its lanes the 96 bytes of the block's row; out of `mid`, the same
//            formula, straight to the output.  The intermediate never goes to memory.
// An axis whose size does not change takes the identity row (xmin = i, one coefficient 1 << 22), which the formula maps to the byte
// itself: a copy.  A block of 32 outputs spans at most 31 scale + K source rows / columns (the centres of its first and last output
// lie 31 scale apart, the taps reach support + 1/2 to either side and K >= 2 support + 1), at most 31 * 8.5 + 35 < WR_SPAN; the
// host sizes the dynamic LDS by that bound, so a 2 : 1 resize takes 12 KB per workgroup, not 48.
#include "rg_common.h"

namespace {

constexpr int WR_BH = 32, WR_BW = 32;     // the block of output pixels a workgroup owns
constexpr int WR_KMAX = 35;               // widest table row
constexpr int WR_SPAN = 300;              // source rows / columns one block can need at most
constexpr int WR_SR = 21;                 // source rows per strip: 21 rows x 3 channels = 63 lanes of the horizontal pass
constexpr int WR_ROW = WR_BW * 3;         // bytes of one row of the intermediate
constexpr int WR_PREC = 22;               // Pillow's PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int wr_clip8(unsigned acc) {
  const int t = (int)acc >> WR_PREC;      // arithmetic shift
  return t < 0 ? 0 : (t > 255 ? 255 : t);
}

// (1 << 21) + sum_j p[j STRIDE] k_j over the cnt (wave-uniform) taps of an LDS column; lane j of kv holds k_j.  Four taps at a time,
// by hand: a loop with a lane read in it is not unrolled for us, and one tap per trip waits for its LDS byte every time
template <int STRIDE>
__device__ __forceinline__ unsigned wr_taps(const uint8_t* p, int kv, int cnt) {
  unsigned acc = 1u << (WR_PREC - 1);
  int j = 0;
  for (; j + 4 <= cnt; j += 4) {
    const unsigned p0 = p[j * STRIDE], p1 = p[(j + 1) * STRIDE], p2 = p[(j + 2) * STRIDE], p3 = p[(j + 3) * STRIDE];
    acc += p0 * (unsigned)__builtin_amdgcn_readlane(kv, j) + p1 * (unsigned)__builtin_amdgcn_readlane(kv, j + 1) +
           p2 * (unsigned)__builtin_amdgcn_readlane(kv, j + 2) + p3 * (unsigned)__builtin_amdgcn_readlane(kv, j + 3);
  }
  for (; j < cnt; ++j) acc += (unsigned)p[j * STRIDE] * (unsigned)__builtin_amdgcn_readlane(kv, j);
  return acc;
}

// (xmin, count) of output index go of a table (int32 rows xmin, count, k_0 .. k_{K-1}), clamped; tab == nullptr: the identity row
__device__ __forceinline__ void wr_bounds(const int32_t* __restrict__ tab, int K, int n_in, int n_out, int go, int* mn, int* cn) {
  int m = 0, c = 0;
  if (go < n_out) {
    if (!tab) { m = go; c = 1; }
    else { m = tab[(size_t)go * (2 + K)]; c = tab[(size_t)go * (2 + K) + 1]; }
    m = min(max(m, 0), n_in);
    c = min(min(max(c, 0), tab ? K : 1), n_in - m);
  }
  *mn = m;
  *cn = c;
}

// the smallest bound and the largest end of the rows that have taps; none: 0, 0
__device__ __forceinline__ void wr_span(const int* mn, const int* cn, int B, int* lo_hi) {
  int lo = 0x7fffffff, hi = 0;
  for (int o = 0; o < B; ++o)
    if (cn[o] > 0) { lo = min(lo, mn[o]); hi = max(hi, mn[o] + cn[o]); }
  if (hi == 0) lo = 0;
  lo_hi[0] = lo;
  lo_hi[1] = hi;
}

// grid: N * by * bx workgroups of 256 lanes; workgroup b: window b / (bx by), block row (b % (bx by)) / bx, block column b % bx.
// dynamic LDS: mid [rcap][WR_ROW], then src [WR_SR][sstride], sstride = ccap * 3 rounded up to 4
__global__ __launch_bounds__(256) void wr_kernel(const uint8_t* __restrict__ raster, int RH, int RW, const int32_t* __restrict__ origins,
                                                 int h, int w, int oh, int ow, const int32_t* __restrict__ xtab, int kx,
                                                 const int32_t* __restrict__ ytab, int ky, uint8_t* __restrict__ out, int bx, int by,
                                                 int reverse, int rcap, int ccap) {
  extern __shared__ uint8_t wr_dyn[];
  __shared__ int sxmin[WR_BW], sxcnt[WR_BW], symin[WR_BH], sycnt[WR_BH];
  __shared__ int lim[4];                                                         // c_lo, c_hi, r_lo, r_hi
  const int sstride = (ccap * 3 + 3) & ~3;
  uint8_t* mid = wr_dyn;
  uint8_t* src = wr_dyn + rcap * WR_ROW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned per = (unsigned)bx * (unsigned)by;
  const size_t n = blockIdx.x / per;
  const unsigned rem = blockIdx.x % per;
  const int oy0 = (int)(rem / (unsigned)bx) * WR_BH, ox0 = (int)(rem % (unsigned)bx) * WR_BW;
  if (tid < WR_BW) wr_bounds(xtab, kx, w, ow, ox0 + tid, &sxmin[tid], &sxcnt[tid]);
  else if (tid >= 64 && tid < 64 + WR_BH) wr_bounds(ytab, ky, h, oh, oy0 + tid - 64, &symin[tid - 64], &sycnt[tid - 64]);
  __syncthreads();
  if (tid == 0) wr_span(sxmin, sxcnt, WR_BW, &lim[0]);
  if (tid == 64) wr_span(symin, sycnt, WR_BH, &lim[2]);
  __syncthreads();
  const int c_lo = lim[0], r_lo = lim[2];
  const int ncols = min(lim[1] - c_lo, ccap), nrows = min(lim[3] - r_lo, rcap);
  const long long wx = (long long)origins[2 * n] + c_lo, wy = (long long)origins[2 * n + 1] + r_lo;   // raster position of (r_lo, c_lo)
  const int nb = ncols * 3;                                                                             // bytes of a strip row
  // the lane's place in the horizontal pass: row hr of the strip, channel hc; lane 63 idles
  const int hr = lane / 3, hc = lane - 3 * hr;
  for (int s0 = 0; s0 < nrows && nb > 0; s0 += WR_SR) {
    const int sr = min(WR_SR, nrows - s0);
    // the strip's raster bytes -> LDS, each once; outside the raster: 0
    // (a wave takes rows wv, wv + 4, ..; a lane issues the loads of up to four of its rows before it uses the first)
    for (int rr0 = wv; rr0 < sr; rr0 += 16) {
#pragma unroll 2
      for (int b = lane; b < nb; b += 64) {
        const int px = (b * 43691) >> 17;                                         // b / 3 for b < 2^15
        const long long gx = wx + px;
        const bool colok = gx >= 0 && gx < RW;
        const size_t cb = (size_t)gx * 3 + (size_t)(b - 3 * px);
        uint8_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rr = rr0 + 4 * u;
          const long long gy = wy + s0 + rr;
          v[u] = 0;
          if (rr < sr && gy >= 0 && gy < RH && colok) v[u] = raster[(size_t)gy * (size_t)RW * 3 + cb];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int rr = rr0 + 4 * u;
          if (rr < sr) src[rr * sstride + b] = v[u];
        }
      }
    }
    __syncthreads();
    // the horizontal pass of the strip: a wave per output column.  Lane j fetches coefficient j of the wave's table row once;
    // the tap loop takes it from there with a lane read, so nothing in the loop waits for memory but the LDS bytes
    {
      const bool active = lane < 63 && hr < sr;
      const uint8_t* sp = src + (active ? hr : 0) * sstride + hc;
      for (int ox = wv; ox < WR_BW; ox += 4) {
        const int m = __builtin_amdgcn_readfirstlane(sxmin[ox]) - c_lo;
        const int cnt = min(__builtin_amdgcn_readfirstlane(sxcnt[ox]), ncols - m);           // cnt == 0 beyond the last column
        int kv = 1 << WR_PREC;
        if (xtab && lane < cnt) kv = xtab[(size_t)(ox0 + ox) * (2 + kx) + 2 + lane];
        const uint8_t* tp = sp + m * 3;
        const unsigned acc = wr_taps<3>(tp, kv, cnt);
        if (active) mid[(s0 + hr) * WR_ROW + ox * 3 + hc] = (uint8_t)wr_clip8(acc);
      }
    }
    __syncthreads();
  }
  // the vertical pass out of LDS: a wave per output row
  uint8_t* o = out + n * (size_t)oh * (size_t)ow * 3;
  for (int oy = wv; oy < WR_BH; oy += 4) {
    const int goy = oy0 + oy;
    if (goy >= oh) break;
    const int m = __builtin_amdgcn_readfirstlane(symin[oy]) - r_lo;
    const int cnt = nb > 0 ? min(__builtin_amdgcn_readfirstlane(sycnt[oy]), nrows - m) : 0;
    int kv = 1 << WR_PREC;
    if (ytab && lane < cnt) kv = ytab[(size_t)goy * (2 + ky) + 2 + lane];
    for (int cb = 0; cb < WR_ROW; cb += 64) {
      const int col = cb + lane, ox = col / 3, c = col - 3 * ox;
      const bool ok = col < WR_ROW && ox0 + ox < ow;
      const uint8_t* mp = mid + m * WR_ROW + (ok ? col : 0);
      const unsigned acc = wr_taps<WR_ROW>(mp, kv, cnt);
      if (ok) o[((size_t)goy * (size_t)ow + (size_t)(ox0 + ox)) * 3 + (size_t)(reverse ? 2 - c : c)] = (uint8_t)wr_clip8(acc);
    }
  }
}

// ------------------------------------------------------------------ rg_mask_erode
constexpr int ER_TH = 32, ER_TW = 128;    // the block of pixels a workgroup owns
constexpr int ER_RMAX = 8;

// Erosion by the L1 ball = the complement of the dilation of the complement, with everything outside the rectangle in the
// complement.  The dilation is the two LDS passes of tq_mask_kernel (rg_tissue.hip).
// grid: N * bx * by workgroups; workgroup b: mask b / (bx by), block row (b % (bx by)) / bx, block column b % bx
__global__ __launch_bounds__(256) void er_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W, int bx, int by,
                                                 int d) {
  __shared__ uint8_t m[ER_TH + 2 * ER_RMAX][ER_TW + 2 * ER_RMAX];
  __shared__ uint8_t hd[ER_TH + 2 * ER_RMAX][ER_TW];
  const int tid = threadIdx.x;
  const unsigned per = (unsigned)bx * (unsigned)by;
  const size_t n = blockIdx.x / per;
  const unsigned rem = blockIdx.x % per;
  const int r0 = (int)(rem / (unsigned)bx) * ER_TH, c0 = (int)(rem % (unsigned)bx) * ER_TW;
  const size_t HW = (size_t)H * W;
  const uint8_t* src = in + n * HW;
  const int RH = ER_TH + 2 * d, RW = ER_TW + 2 * d;
  // i / RW as (i rwinv) >> 20, rwinv = ceil(2^20 / RW): exact for i < RH RW <= 6912 (the excess is < RW <= 144 and 6912 * 144 < 2^20)
  const unsigned rwinv = ((1u << 20) + (unsigned)RW - 1u) / (unsigned)RW;
  for (int i = tid; i < RH * RW; i += 256) {
    const int rr = (int)(((unsigned)i * rwinv) >> 20), cc = i - rr * RW;
    const int gr = r0 - d + rr, gc = c0 - d + cc;
    uint8_t v = 1;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = src[(size_t)gr * W + gc] ? 0 : 1;
    m[rr][cc] = v;
  }
  __syncthreads();
  // per row of the region, the distance to the nearest unset pixel within d columns (d + 1: none)
  for (int i = tid; i < RH * ER_TW; i += 256) {
    const int rr = i / ER_TW, c = i - rr * ER_TW;
    int best = d + 1;
    for (int dc = -d; dc <= d; ++dc)
      if (m[rr][c + d + dc]) best = min(best, dc < 0 ? -dc : dc);
    hd[rr][c] = (uint8_t)best;
  }
  __syncthreads();
  uint8_t* dst = out + n * HW;
  for (int i = tid; i < ER_TH * ER_TW; i += 256) {
    const int r = i / ER_TW, c = i - r * ER_TW;
    const int gr = r0 + r, gc = c0 + c;
    if (gr >= H || gc >= W) continue;
    int hit = 0;                                                                 // some unset pixel within L1 distance d
    for (int dr = -d; dr <= d; ++dr) hit |= (int)hd[r + d + dr][c] <= d - (dr < 0 ? -dr : dr);
    dst[(size_t)gr * W + gc] = (uint8_t)(hit ? 0 : 1);
  }
}

// ------------------------------------------------------------------ rg_box_reduce_u8
// one lane per output byte, grid-stride (the caller launches at most 2^20 workgroups)
__global__ __launch_bounds__(256) void box_kernel(const uint8_t* __restrict__ raster, uint8_t* __restrict__ out, int RH, int RW, int TH,
                                                  int TW, int f) {
  const size_t total = (size_t)TH * (size_t)TW * 3;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t p = i / 3;
    const int c = (int)(i - 3 * p);
    const int ty = (int)(p / (size_t)TW), tx = (int)(p - (size_t)ty * TW);
    const int y0 = ty * f, x0 = tx * f;                                          // ty f < RH <= 2^31 - 1
    const int y1 = (int)min((long long)y0 + f, (long long)RH), x1 = (int)min((long long)x0 + f, (long long)RW);
    unsigned sum = 0;
    for (int y = y0; y < y1; ++y) {
      const uint8_t* row = raster + ((size_t)y * (size_t)RW) * 3 + c;
      for (int x = x0; x < x1; ++x) sum += row[(size_t)x * 3];
    }
    const unsigned cnt = (unsigned)(y1 - y0) * (unsigned)(x1 - x0);
    out[i] = (uint8_t)((sum + cnt / 2) / cnt);
  }
}

// Pillow's ksize of one axis: (int)ceil(support) * 2 + 1, support = 2 max(in / out, 1)
int wr_ksize(int n_in, int n_out) {
  const double scale = (double)n_in / (double)n_out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  long long c = (long long)support;
  if ((double)c < support) ++c;
  return (int)(c * 2 + 1);
}

// the source rows / columns a block of 32 outputs can span on an axis n_in -> n_out: 31 scale + K, at most WR_SPAN
int wr_span_cap(int n_in, int n_out) {
  if (n_in == n_out) return WR_BH;
  const long long cap = (long long)(31.0 * (double)n_in / (double)n_out) + 1 + wr_ksize(n_in, n_out);
  return (int)(cap < WR_SPAN ? cap : WR_SPAN);
}

// ------------------------------------------------------------------ the two-launch form (measurement only)
// The same arithmetic with the byte intermediate in memory: mid [N][h][ow][3].  One lane per intermediate / output byte, the raster and
// the tables read straight from memory.  tools/ab_tiler.py measures the one-launch kernel against it.
__global__ __launch_bounds__(256) void wr2_h_kernel(const uint8_t* __restrict__ raster, int RH, int RW, const int32_t* __restrict__ origins,
                                                    int h, int w, int ow, const int32_t* __restrict__ xtab, int kx,
                                                    uint8_t* __restrict__ mid, int bpr) {
  const size_t row = blockIdx.x / (unsigned)bpr;                                 // n * h + y
  const int col = (int)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
  if (col >= ow * 3) return;
  const size_t n = row / (unsigned)h;
  const int y = (int)(row - n * (unsigned)h), ox = col / 3, c = col - 3 * ox;
  int m = ox, cnt = 1;
  if (xtab) {
    m = xtab[(size_t)ox * (2 + kx)];
    cnt = xtab[(size_t)ox * (2 + kx) + 1];
    m = min(max(m, 0), w);
    cnt = min(min(max(cnt, 0), kx), w - m);
  }
  const long long gy = (long long)origins[2 * n + 1] + y, gx0 = (long long)origins[2 * n] + m;
  unsigned acc = 1u << (WR_PREC - 1);
  if (gy >= 0 && gy < RH)
    for (int j = 0; j < cnt; ++j) {
      const long long gx = gx0 + j;
      if (gx >= 0 && gx < RW)
        acc += (unsigned)raster[((size_t)gy * (size_t)RW + (size_t)gx) * 3 + c] * (unsigned)(xtab ? xtab[(size_t)ox * (2 + kx) + 2 + j] : (1 << WR_PREC));
    }
  mid[row * (size_t)ow * 3 + col] = (uint8_t)wr_clip8(acc);
}

__global__ __launch_bounds__(256) void wr2_v_kernel(const uint8_t* __restrict__ mid, int h, int oh, int ow, const int32_t* __restrict__ ytab,
                                                    int ky, uint8_t* __restrict__ out, int bpr, int reverse) {
  const size_t row = blockIdx.x / (unsigned)bpr;                                 // n * oh + oy
  const int col = (int)(blockIdx.x % (unsigned)bpr) * 256 + threadIdx.x;
  if (col >= ow * 3) return;
  const size_t n = row / (unsigned)oh;
  const int oy = (int)(row - n * (unsigned)oh), ox = col / 3, c = col - 3 * ox;
  int m = oy, cnt = 1;
  if (ytab) {
    m = ytab[(size_t)oy * (2 + ky)];
    cnt = ytab[(size_t)oy * (2 + ky) + 1];
    m = min(max(m, 0), h);
    cnt = min(min(max(cnt, 0), ky), h - m);
  }
  unsigned acc = 1u << (WR_PREC - 1);
  for (int j = 0; j < cnt; ++j)
    acc += (unsigned)mid[(n * (size_t)h + (size_t)(m + j)) * (size_t)ow * 3 + col] * (unsigned)(ytab ? ytab[(size_t)oy * (2 + ky) + 2 + j] : (1 << WR_PREC));
  out[row * (size_t)ow * 3 + (size_t)(3 * ox + (reverse ? 2 - c : c))] = (uint8_t)wr_clip8(acc);
}

// what both forms refuse; `blocks`: workgroups per window of the form that asks
int wr_validate(const uint8_t* raster, int RH, int RW, const int32_t* origins, int N, int h, int w, int oh, int ow, const int32_t* xtab,
                int kx, const int32_t* ytab, int ky, const uint8_t* out, int flags, long long blocks) {
  RG_REQUIRE(raster && origins && out, RG_EINVAL, "window_resize_u8: NULL buffer");
  RG_REQUIRE(N >= 0 && RH > 0 && RW > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, RG_EINVAL,
             "window_resize_u8: bad shape N %d raster %d x %d read %d x %d out %d x %d", N, RH, RW, h, w, oh, ow);
  RG_REQUIRE((flags & ~RG_EXPORT_REVERSE) == 0, RG_EINVAL, "window_resize_u8: unknown flag bits 0x%x", flags);
  RG_REQUIRE(((uintptr_t)origins & 3) == 0 && ((uintptr_t)xtab & 3) == 0 && ((uintptr_t)ytab & 3) == 0, RG_EINVAL,
             "window_resize_u8: origins and tables need 4-byte alignment");
  RG_REQUIRE(oh <= 1024 && ow <= 1024, RG_EUNSUPPORTED, "window_resize_u8: out %d x %d is more than 1024", oh, ow);
  RG_REQUIRE(h <= 8192 && w <= 8192, RG_EUNSUPPORTED, "window_resize_u8: read size %d x %d is more than 8192", h, w);
  if (w != ow) {
    const int need = wr_ksize(w, ow);
    RG_REQUIRE(need <= WR_KMAX, RG_EUNSUPPORTED, "window_resize_u8: %d -> %d columns needs %d coefficients, more than %d", w, ow, need, WR_KMAX);
    RG_REQUIRE(xtab && kx >= need && kx <= WR_KMAX, RG_EINVAL, "window_resize_u8: %d -> %d columns needs a table of width %d..%d, got %d%s",
               w, ow, need, WR_KMAX, kx, xtab ? "" : " (NULL)");
  }
  if (h != oh) {
    const int need = wr_ksize(h, oh);
    RG_REQUIRE(need <= WR_KMAX, RG_EUNSUPPORTED, "window_resize_u8: %d -> %d rows needs %d coefficients, more than %d", h, oh, need, WR_KMAX);
    RG_REQUIRE(ytab && ky >= need && ky <= WR_KMAX, RG_EINVAL, "window_resize_u8: %d -> %d rows needs a table of width %d..%d, got %d%s",
               h, oh, need, WR_KMAX, ky, ytab ? "" : " (NULL)");
  }
  RG_REQUIRE((long long)N * blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "window_resize_u8: N %d read %d x %d out %d x %d is more than 2^31 - 1 workgroups",
             N, h, w, oh, ow);
  const uintptr_t a0 = (uintptr_t)raster, a1 = a0 + (size_t)RH * (size_t)RW * 3;
  const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (size_t)N * (size_t)oh * (size_t)ow * 3;
  RG_REQUIRE(N == 0 || b1 <= a0 || a1 <= b0, RG_EINVAL, "window_resize_u8: out overlaps the raster");
  return RG_OK;
}

}  // namespace

extern "C" int rg_window_resize_u8(const uint8_t* raster, int RH, int RW, const int32_t* origins, int N, int h, int w, int oh, int ow,
                                   const int32_t* xtab, int kx, const int32_t* ytab, int ky, uint8_t* out, int flags, void* stream) {
  const int bx = ow > 0 ? (ow + WR_BW - 1) / WR_BW : 1, by = oh > 0 ? (oh + WR_BH - 1) / WR_BH : 1;
  const int rc = wr_validate(raster, RH, RW, origins, N, h, w, oh, ow, xtab, kx, ytab, ky, out, flags, (long long)bx * by);
  if (rc != RG_OK || N == 0) return rc;
  const int rcap = wr_span_cap(h, oh), ccap = wr_span_cap(w, ow);
  const size_t lds = (size_t)rcap * WR_ROW + (size_t)WR_SR * (size_t)((ccap * 3 + 3) & ~3);
  hipLaunchKernelGGL(wr_kernel, dim3((unsigned)(N * bx * by)), dim3(256), lds, rg_stream(stream), raster, RH, RW, origins, h, w, oh, ow,
                     w == ow ? (const int32_t*)nullptr : xtab, kx, h == oh ? (const int32_t*)nullptr : ytab, ky, out, bx, by,
                     (flags & RG_EXPORT_REVERSE) != 0, rcap, ccap);
  RG_LAUNCH_CHECK("window_resize_u8");
  return RG_OK;
}

extern "C" int rg_probe_window_resize_2pass(const uint8_t* raster, int RH, int RW, const int32_t* origins, int N, int h, int w, int oh, int ow,
                                            const int32_t* xtab, int kx, const int32_t* ytab, int ky, uint8_t* out, int flags,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const int bpr = ow > 0 ? (ow * 3 + 255) / 256 : 1;
  const long long rows = h > oh ? h : oh;
  const int rc = wr_validate(raster, RH, RW, origins, N, h, w, oh, ow, xtab, kx, ytab, ky, out, flags, rows * bpr);
  if (rc != RG_OK || N == 0) return rc;
  const size_t need = (size_t)N * (size_t)h * (size_t)ow * 3;
  RG_REQUIRE(workspace && workspace_bytes >= need, RG_EINVAL, "probe_window_resize_2pass: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  uint8_t* mid = (uint8_t*)workspace;
  hipLaunchKernelGGL(wr2_h_kernel, dim3((unsigned)((size_t)N * h * bpr)), dim3(256), 0, rg_stream(stream), raster, RH, RW, origins, h, w, ow,
                     w == ow ? (const int32_t*)nullptr : xtab, kx, mid, bpr);
  hipLaunchKernelGGL(wr2_v_kernel, dim3((unsigned)((size_t)N * oh * bpr)), dim3(256), 0, rg_stream(stream), (const uint8_t*)mid, h, oh, ow,
                     h == oh ? (const int32_t*)nullptr : ytab, ky, out, bpr, (flags & RG_EXPORT_REVERSE) != 0);
  RG_LAUNCH_CHECK("probe_window_resize_2pass");
  return RG_OK;
}

extern "C" int rg_mask_erode(const uint8_t* mask, uint8_t* out, int N, int H, int W, int radius, void* stream) {
  RG_REQUIRE(mask && out, RG_EINVAL, "mask_erode: NULL buffer");
  RG_REQUIRE(N >= 0 && H > 0 && W > 0, RG_EINVAL, "mask_erode: bad shape N %d H %d W %d", N, H, W);
  RG_REQUIRE(radius >= 0 && radius <= ER_RMAX, RG_EINVAL, "mask_erode: radius %d is not in 0..%d", radius, ER_RMAX);
  {
    const size_t bytes = (size_t)N * (size_t)H * (size_t)W;
    const uintptr_t a0 = (uintptr_t)mask, b0 = (uintptr_t)out;
    RG_REQUIRE(N == 0 || b0 + bytes <= a0 || a0 + bytes <= b0, RG_EINVAL, "mask_erode: out overlaps the input");
  }
  if (N == 0) return RG_OK;
  const int bx = (W + ER_TW - 1) / ER_TW, by = (H + ER_TH - 1) / ER_TH;
  RG_REQUIRE((long long)N * bx * by <= 0x7fffffffLL, RG_EUNSUPPORTED, "mask_erode: N %d H %d W %d is more than 2^31 - 1 workgroups", N, H, W);
  hipLaunchKernelGGL(er_kernel, dim3((unsigned)(N * bx * by)), dim3(256), 0, rg_stream(stream), mask, out, H, W, bx, by, radius);
  RG_LAUNCH_CHECK("mask_erode");
  return RG_OK;
}

extern "C" int rg_box_reduce_u8(const uint8_t* raster, int RH, int RW, int factor, uint8_t* out, void* stream) {
  RG_REQUIRE(raster && out, RG_EINVAL, "box_reduce_u8: NULL buffer");
  RG_REQUIRE(RH > 0 && RW > 0, RG_EINVAL, "box_reduce_u8: bad raster %d x %d", RH, RW);
  RG_REQUIRE(factor >= 1 && factor <= 64, RG_EINVAL, "box_reduce_u8: factor %d is not in 1..64", factor);
  const int TH = (int)(((long long)RH + factor - 1) / factor), TW = (int)(((long long)RW + factor - 1) / factor);
  const size_t total = (size_t)TH * (size_t)TW * 3;
  {
    const uintptr_t a0 = (uintptr_t)raster, a1 = a0 + (size_t)RH * (size_t)RW * 3, b0 = (uintptr_t)out;
    RG_REQUIRE(b0 + total <= a0 || a1 <= b0, RG_EINVAL, "box_reduce_u8: out overlaps the raster");
  }
  const size_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(box_kernel, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, rg_stream(stream), raster, out,
                     RH, RW, TH, TW, factor);
  RG_LAUNCH_CHECK("box_reduce_u8");
  return RG_OK;
}
