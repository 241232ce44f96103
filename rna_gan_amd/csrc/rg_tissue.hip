// rg_tissue.hip -- tile quality control on the device (rg_tile_qc): per uint8 RGB tile the four Otsu thresholds (R, G, B and the
// 8-bit saturation), the raw and the dilated tissue-mask counts and four exact order statistics of the integer luma.  Everything
// returned is an integer (include/rnagan_hip.h states the contract, tests/tissue_refs.py restates it); the float decisions --
// fractions, percentile interpolation, low contrast -- are the caller's (rna_gan_amd/tissue.py).
//
// Five launches on the caller's stream; the tile bytes are read from memory TWICE (plus the dilation halo):
//   u8px_zero     the per-tile workspace (TQ_WORDS counters per tile)
//   tq_hist       read 1: a workgroup owns TQ_CHUNK consecutive pixels of one tile, read through the pixel stream of rg_u8px.h.
//                 Five LDS histograms (R, G, B, s8: 256 bins each;
//                 the luma's coarse level L >> 10: 2491 of TQ_COARSE bins) filled with LDS atomics, merged into the tile's counters
//                 with one global 32-bit integer atomic per OCCUPIED bin.
//   tq_scan       one workgroup per tile, wave c = channel c: Otsu on the merged histogram (integer prefix sums in LDS, the 255
//                 candidates evaluated in fp64 exactly as the contract orders the operations, first largest wins); then the coarse
//                 luma bin and the residual rank of each of the four ranks.
//   tq_mask       read 2: a workgroup owns a TQ_TH x TQ_TW block of pixels and reads it with a `dilate`-wide halo (a lane issues the
//                 byte loads of TQ_BATCH pixels before it uses the first).  The raw mask goes
//                 to LDS as bytes; the dilation by the L1 ball of radius d is two LDS passes (per row the distance to the nearest
//                 set pixel within d columns; per pixel, whether some row r + dr has such a distance <= d - |dr|) -- equal to d
//                 iterations of the 4-connected cross inside a rectangle.  The pixels of the block proper also fill the fine luma
//                 histograms (L & 1023 of the pixels whose coarse bin a rank selected) and the raw count.
//   tq_final      one workgroup per tile: the fine bin of each rank; writes the tile's 12 stats words with plain stores.
// s8 takes no division: a 256-entry table of ceil(2^24 / mx) in LDS and one 32 x 32 -> 64-bit multiply (tq_s8).
// Integer atomics commute, so no result depends on the launch plan, on N or on a neighbouring tile; no 16-bit type is involved.
#include "rg_u8px.h"

#pragma clang fp contract(off)

namespace {

constexpr int TQ_CHUNK = 16384;         // pixels per tq_hist workgroup
constexpr int TQ_COARSE = 2560;         // coarse luma bins allocated; (2550000 >> 10) + 1 = 2491 are reachable
constexpr int TQ_FINE = 1024;           // fine luma bins: L & 1023
constexpr int TQ_TH = 32, TQ_TW = 128;  // the block of pixels a tq_mask workgroup owns
constexpr int TQ_DMAX = 8;
constexpr int TQ_BATCH = 4;              // region pixels a tq_mask lane loads before it uses the first
constexpr int TQ_RW = TQ_TW + 2 * TQ_DMAX, TQ_RH = TQ_TH + 2 * TQ_DMAX;
// the per-tile workspace, in 32-bit words
constexpr int TQ_OFF_HIST = 0;                                // [4][256]  R, G, B, s8
constexpr int TQ_OFF_COARSE = 1024;                           // [TQ_COARSE]
constexpr int TQ_OFF_FINE = TQ_OFF_COARSE + TQ_COARSE;        // [4][TQ_FINE]
constexpr int TQ_OFF_THR = TQ_OFF_FINE + 4 * TQ_FINE;         // [4] thresholds
constexpr int TQ_OFF_SEL = TQ_OFF_THR + 4;                    // [4][2] coarse bin, residual rank
constexpr int TQ_OFF_COUNT = TQ_OFF_SEL + 8;                  // [2] raw, dilated
constexpr int TQ_WORDS = TQ_OFF_COUNT + 4;                    // 7696 words = 30784 bytes

struct tq_ranks { int r[4]; };

// s8 = (255 (mx - mn)) / mx without a division: inv[mx] = ceil(2^24 / mx) (inv[0] = 0), s8 = (num inv[mx]) >> 24.  Exact: the
// multiplier's excess e = inv[mx] mx - 2^24 < mx <= 255 and num <= 255 * 255, so num e < 2^24 (every (mx, mn) pair was also
// enumerated on the host).  inv lives in LDS, filled by tq_fill_inv once per workgroup.
__device__ __forceinline__ void tq_fill_inv(unsigned* inv, int tid) {
  if (tid < 256) inv[tid] = tid ? ((1u << 24) + (unsigned)tid - 1u) / (unsigned)tid : 0u;
}
__device__ __forceinline__ int tq_s8(const unsigned* inv, int R, int G, int B) {
  const int mx = max(R, max(G, B)), mn = min(R, min(G, B));
  return (int)(((unsigned long long)(unsigned)(255 * (mx - mn)) * inv[mx]) >> 24);
}
__device__ __forceinline__ int tq_luma(int R, int G, int B) { return 2125 * R + 7154 * G + 721 * B; }

struct tq_hist_lds {
  unsigned h[4][256];
  unsigned coarse[TQ_COARSE];
  unsigned inv[256];
};

struct tq_count_f {
  tq_hist_lds& s;
  __device__ __forceinline__ void px(int R, int G, int B) {
    atomicAdd(&s.h[0][R], 1u);
    atomicAdd(&s.h[1][G], 1u);
    atomicAdd(&s.h[2][B], 1u);
    atomicAdd(&s.h[3][tq_s8(s.inv, R, G, B)], 1u);
    atomicAdd(&s.coarse[tq_luma(R, G, B) >> 10], 1u);
  }
  __device__ __forceinline__ void flush() {}
};

// grid: N * geom.chunks workgroups, every tile chunked on its own (u8px_plan's per_tile): workgroup b counts into tile b / chunks
__global__ __launch_bounds__(256) void tq_hist_kernel(const uint8_t* __restrict__ tiles, unsigned* __restrict__ ws, u8px_geom geom) {
  __shared__ tq_hist_lds s;
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x / geom.chunks;
  for (int i = tid; i < 4 * 256 + TQ_COARSE; i += 256) (&s.h[0][0])[i] = 0u;      // h and coarse are contiguous
  tq_fill_inv(s.inv, tid);
  __syncthreads();
  tq_count_f f = {s};
  u8px_each(tiles, geom, f);
  __syncthreads();
  unsigned* g = ws + n * TQ_WORDS;                // TQ_OFF_HIST = 0 and TQ_OFF_COARSE = 1024: the same contiguous order as in LDS
  for (int i = tid; i < 4 * 256 + TQ_COARSE; i += 256) {
    const unsigned v = (&s.h[0][0])[i];
    if (v) atomicAdd(&g[i], v);
  }
}

// grid: N workgroups of 256 lanes (4 waves)
__global__ __launch_bounds__(256) void tq_scan_kernel(unsigned* __restrict__ ws, tq_ranks ranks) {
  __shared__ unsigned h[4][256];
  __shared__ unsigned w1s[4][256];
  __shared__ unsigned long long s1s[4][256];
  __shared__ double bestv[4][64];
  __shared__ int bestk[4][64];
  __shared__ int lohi[4][2];
  __shared__ unsigned coarse[TQ_COARSE];
  __shared__ unsigned part[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned* g = ws + (size_t)blockIdx.x * TQ_WORDS;
  for (int i = tid; i < 1024; i += 256) (&h[0][0])[i] = g[TQ_OFF_HIST + i];
  for (int i = tid; i < TQ_COARSE; i += 256) coarse[i] = g[TQ_OFF_COARSE + i];
  __syncthreads();
  // ---- Otsu: wave = channel
  if (lane == 0) {
    unsigned w1 = 0;
    unsigned long long s1 = 0;
    int lo = -1, hi = -1;
    for (int i = 0; i < 256; ++i) {
      const unsigned v = h[wave][i];
      w1 += v;
      s1 += (unsigned long long)i * v;
      w1s[wave][i] = w1;
      s1s[wave][i] = s1;
      if (v) {
        if (lo < 0) lo = i;
        hi = i;
      }
    }
    lohi[wave][0] = lo;
    lohi[wave][1] = hi;
  }
  __syncthreads();
  {
    const int lo = lohi[wave][0], hi = lohi[wave][1];
    const unsigned nn = w1s[wave][255];
    const unsigned long long S = s1s[wave][255];
    double bv = -1.0;
    int bk = 256;
    for (int k = lane; k < 255; k += 64) {          // ascending k per lane: a strict > keeps the first
      if (k < lo || k >= hi) continue;
      const unsigned w1 = w1s[wave][k], w2 = nn - w1;
      const unsigned long long s1 = s1s[wave][k], s2 = S - s1;
      const double m1 = (double)s1 / (double)w1;
      const double m2 = (double)s2 / (double)w2;
      const double d = m1 - m2;
      const double v = (((double)w1 * (double)w2) * d) * d;
      if (v > bv) { bv = v; bk = k; }
    }
    bestv[wave][lane] = bv;
    bestk[wave][lane] = bk;
  }
  __syncthreads();
  if (lane == 0) {
    const int lo = lohi[wave][0], hi = lohi[wave][1];
    int thr = lo < 0 ? 0 : lo;                      // lo == hi: the constant channel (lo < 0 cannot happen: H W >= 1)
    if (lo != hi) {
      double bv = -1.0;
      int bk = 256;
      for (int l = 0; l < 64; ++l) {
        const double v = bestv[wave][l];
        const int k = bestk[wave][l];
        if (v > bv || (v == bv && k < bk)) { bv = v; bk = k; }
      }
      thr = bk;
    }
    g[TQ_OFF_THR + wave] = (unsigned)thr;
  }
  // ---- the coarse luma bin of each rank: the smallest bin whose inclusive prefix count exceeds the rank
  {
    unsigned a = 0;
    for (int i = 0; i < TQ_COARSE / 256; ++i) a += coarse[tid * (TQ_COARSE / 256) + i];
    part[tid] = a;
  }
  __syncthreads();
  if (tid < 4) {
    const unsigned r = (unsigned)ranks.r[tid];
    unsigned cum = 0;
    int seg = 0;
    while (seg < 255 && cum + part[seg] <= r) { cum += part[seg]; ++seg; }
    int b = seg * (TQ_COARSE / 256);
    const int bend = b + TQ_COARSE / 256 - 1;
    while (b < bend && cum + coarse[b] <= r) { cum += coarse[b]; ++b; }
    g[TQ_OFF_SEL + 2 * tid] = (unsigned)b;
    g[TQ_OFF_SEL + 2 * tid + 1] = r - cum;
  }
}

// grid: N * bx * by workgroups; workgroup b: tile b / (bx by), block row (b % (bx by)) / bx, block column b % bx
__global__ __launch_bounds__(256) void tq_mask_kernel(const uint8_t* __restrict__ tiles, unsigned* __restrict__ ws,
                                                      uint8_t* __restrict__ mask, int H, int W, int bx, int by, int planar,
                                                      int reverse, int rgb_min, int d) {
  __shared__ uint8_t m[TQ_RH][TQ_RW];
  __shared__ uint8_t hd[TQ_RH][TQ_TW];
  __shared__ unsigned fine[4][TQ_FINE];
  __shared__ unsigned counts[2];
  __shared__ int thr[4];
  __shared__ int sel[4];
  __shared__ unsigned inv[256];
  const int tid = threadIdx.x;
  const unsigned per = (unsigned)bx * (unsigned)by;
  const size_t n = blockIdx.x / per;
  const unsigned rem = blockIdx.x % per;
  const int r0 = (int)(rem / (unsigned)bx) * TQ_TH, c0g = (int)(rem % (unsigned)bx) * TQ_TW;
  unsigned* g = ws + n * TQ_WORDS;
  for (int i = tid; i < 4 * TQ_FINE; i += 256) (&fine[0][0])[i] = 0u;
  tq_fill_inv(inv, tid);
  if (tid < 2) counts[tid] = 0u;
  if (tid < 4) {
    thr[tid] = (int)g[TQ_OFF_THR + tid];
    sel[tid] = (int)g[TQ_OFF_SEL + 2 * tid];
  }
  __syncthreads();
  const size_t HW = (size_t)H * W;
  const uint8_t* t = tiles + n * 3 * HW;
  const int RH = TQ_TH + 2 * d, RW = TQ_TW + 2 * d;
  const int tR = thr[0], tG = thr[1], tB = thr[2], tS = thr[3];
  // i / RW as (i rwinv) >> 20, rwinv = ceil(2^20 / RW): exact for i < RH RW <= 6912 (the excess is < RW <= 144 and 6912 * 144 < 2^20)
  const unsigned rwinv = ((1u << 20) + (unsigned)RW - 1u) / (unsigned)RW;
  const int total = RH * RW;
  unsigned raw = 0;
  // pass A: the raw mask of the block and its halo; outside the tile it is background.  A lane takes TQ_BATCH region pixels per
  // step and issues all their byte loads before it uses the first (one exposed memory latency per step, not per pixel)
  for (int i0 = tid; i0 < total; i0 += 256 * TQ_BATCH) {
    int c0[TQ_BATCH], c1[TQ_BATCH], c2[TQ_BATCH];
#pragma unroll
    for (int j = 0; j < TQ_BATCH; ++j) {
      const int i = i0 + 256 * j;
      const int rr = (int)(((unsigned)i * rwinv) >> 20), cc = i - rr * RW;
      const int gr = r0 - d + rr, gc = c0g - d + cc;
      c0[j] = -1;
      if (i < total && gr >= 0 && gr < H && gc >= 0 && gc < W) u8px_load(t, HW, (size_t)gr * W + gc, planar, 0, c0[j], c1[j], c2[j]);
    }
#pragma unroll
    for (int j = 0; j < TQ_BATCH; ++j) {
      const int i = i0 + 256 * j;
      if (i >= total) break;
      const int rr = (int)(((unsigned)i * rwinv) >> 20), cc = i - rr * RW;
      uint8_t v = 0;
      if (c0[j] >= 0) {
        const int R = reverse ? c2[j] : c0[j], G = c1[j], B = reverse ? c0[j] : c2[j];
        const bool on = tq_s8(inv, R, G, B) > tS && !(R > tR && G > tG && B > tB) && R > rgb_min && G > rgb_min && B > rgb_min;
        v = on ? 1 : 0;
        if (rr >= d && rr < d + TQ_TH && cc >= d && cc < d + TQ_TW) {      // the block proper: counted once over the grid
          raw += v;
          const int L = tq_luma(R, G, B);
          const int cb = L >> 10, fb = L & (TQ_FINE - 1);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (cb == sel[q]) atomicAdd(&fine[q][fb], 1u);
        }
      }
      m[rr][cc] = v;
    }
  }
  __syncthreads();
  // pass B: per row of the region, the distance to the nearest set pixel within d columns (d + 1: none)
  for (int i = tid; i < RH * TQ_TW; i += 256) {
    const int rr = i / TQ_TW, c = i - rr * TQ_TW;
    int best = d + 1;
    for (int dc = -d; dc <= d; ++dc)
      if (m[rr][c + d + dc]) best = min(best, dc < 0 ? -dc : dc);
    hd[rr][c] = (uint8_t)best;
  }
  __syncthreads();
  // pass C: some raw pixel within L1 distance d
  unsigned dil = 0;
  uint8_t* mk = mask ? mask + n * HW : nullptr;
  for (int i = tid; i < TQ_TH * TQ_TW; i += 256) {
    const int r = i / TQ_TW, c = i - r * TQ_TW;
    const int gr = r0 + r, gc = c0g + c;
    if (gr >= H || gc >= W) continue;
    int on = 0;
    for (int dr = -d; dr <= d; ++dr) on |= (int)hd[r + d + dr][c] <= d - (dr < 0 ? -dr : dr);
    dil += (unsigned)on;
    if (mk) mk[(size_t)gr * W + gc] = (uint8_t)on;
  }
  if (raw) atomicAdd(&counts[0], raw);
  if (dil) atomicAdd(&counts[1], dil);
  __syncthreads();
  for (int i = tid; i < 4 * TQ_FINE; i += 256) {
    const unsigned v = (&fine[0][0])[i];
    if (v) atomicAdd(&g[TQ_OFF_FINE + i], v);
  }
  if (tid < 2 && counts[tid]) atomicAdd(&g[TQ_OFF_COUNT + tid], counts[tid]);
}

// grid: N workgroups of 256 lanes; wave j = rank j
__global__ __launch_bounds__(256) void tq_final_kernel(const unsigned* __restrict__ ws, int32_t* __restrict__ stats) {
  __shared__ unsigned part[4][64];
  __shared__ int lum[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned* g = ws + (size_t)blockIdx.x * TQ_WORDS;
  const unsigned* f = g + TQ_OFF_FINE + wave * TQ_FINE;
  constexpr int PER = TQ_FINE / 64;
  unsigned a = 0;
  for (int i = 0; i < PER; ++i) a += f[lane * PER + i];
  part[wave][lane] = a;
  __syncthreads();
  if (lane == 0) {
    const unsigned r = g[TQ_OFF_SEL + 2 * wave + 1];
    unsigned cum = 0;
    int seg = 0;
    while (seg < 63 && cum + part[wave][seg] <= r) { cum += part[wave][seg]; ++seg; }
    int b = seg * PER;
    const int bend = b + PER - 1;
    while (b < bend && cum + f[b] <= r) { cum += f[b]; ++b; }
    lum[wave] = (int)((g[TQ_OFF_SEL + 2 * wave] << 10) | (unsigned)b);
  }
  __syncthreads();
  if (tid < 12) {
    int v = 0;
    if (tid < 4) v = (int)g[TQ_OFF_THR + tid];
    else if (tid < 6) v = (int)g[TQ_OFF_COUNT + tid - 4];
    else if (tid < 10) v = lum[tid - 6];
    stats[(size_t)blockIdx.x * 12 + tid] = v;
  }
}

}  // namespace

extern "C" size_t rg_tile_qc_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)N * TQ_WORDS * sizeof(unsigned);
}

extern "C" int rg_tile_qc(const uint8_t* tiles, int N, int H, int W, int flags, int rgb_min, int dilate, const int* ranks4,
                          int32_t* stats, uint8_t* mask_or_null, void* workspace, size_t workspace_bytes, void* stream) {
  RG_REQUIRE(tiles && stats && ranks4 && workspace, RG_EINVAL, "tile_qc: NULL buffer");
  // (a bad shape is u8px_plan's to refuse)
  RG_REQUIRE(N < 0 || H <= 0 || W <= 0 || (long long)H * W <= (1LL << 26), RG_EUNSUPPORTED, "tile_qc: H %d W %d is more than 2^26 pixels per tile", H, W);
  u8px_geom geom;
  unsigned hist_blocks;
  int rc = u8px_plan("tile_qc", N, H, W, flags, TQ_CHUNK, ((uintptr_t)tiles & 3) == 0, true, &geom, &hist_blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(rgb_min >= 0 && rgb_min <= 255, RG_EINVAL, "tile_qc: rgb_min %d is not in 0..255", rgb_min);
  RG_REQUIRE(dilate >= 0 && dilate <= TQ_DMAX, RG_EINVAL, "tile_qc: dilate %d is not in 0..%d", dilate, TQ_DMAX);
  const int HW = H * W;
  tq_ranks ranks;
  for (int j = 0; j < 4; ++j) {
    RG_REQUIRE(ranks4[j] >= 0 && ranks4[j] < HW, RG_EINVAL, "tile_qc: rank %d = %d is not in [0, H W = %d)", j, ranks4[j], HW);
    ranks.r[j] = ranks4[j];
  }
  RG_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)stats & 3) == 0, RG_EINVAL, "tile_qc: stats and workspace need 4-byte alignment");
  if (N == 0) return RG_OK;
  const size_t need = (size_t)N * TQ_WORDS * sizeof(unsigned);
  RG_REQUIRE(workspace_bytes >= need, RG_EINVAL, "tile_qc: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const int bx = (W + TQ_TW - 1) / TQ_TW, by = (H + TQ_TH - 1) / TQ_TH;
  RG_REQUIRE((long long)N * bx * by <= 0x7fffffffLL, RG_EUNSUPPORTED, "tile_qc: N %d H %d W %d is more than 2^31 - 1 workgroups", N, H, W);
  hipStream_t st = rg_stream(stream);
  unsigned* ws = (unsigned*)workspace;
  if ((rc = u8px_zero("tile_qc", ws, (size_t)N * TQ_WORDS, st)) != RG_OK) return rc;
  hipLaunchKernelGGL(tq_hist_kernel, dim3(hist_blocks), dim3(256), 0, st, tiles, ws, geom);
  hipLaunchKernelGGL(tq_scan_kernel, dim3((unsigned)N), dim3(256), 0, st, ws, ranks);
  hipLaunchKernelGGL(tq_mask_kernel, dim3((unsigned)(N * bx * by)), dim3(256), 0, st, tiles, ws, mask_or_null, H, W, bx, by, geom.planar,
                     geom.reverse, rgb_min, dilate);
  hipLaunchKernelGGL(tq_final_kernel, dim3((unsigned)N), dim3(256), 0, st, (const unsigned*)ws, stats);
  RG_LAUNCH_CHECK("tile_qc");
  return RG_OK;
}
