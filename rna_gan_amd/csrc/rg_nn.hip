// rg_nn.hip -- the memorisation audit's all-pairs search (rna_gan_amd.nearest): int8 tile descriptors and their exact nearest
// neighbours on the integer matrix cores.  Everything is an INTEGER (include/rnagan_hip.h states the contract, tests/nn_audit_refs.py
// restates it); no floating-point instruction is involved and no 16-bit type: both builds behave identically.
//
//   rg_tile_descriptor_i8   uint8 [N][C][S][S] -> int8 [N][ldd] block means minus 128, and their squared norms.  One workgroup per
//                           tile, so norm2 is one block reduction and needs neither a second pass nor an atomic.
//   rg_nn_topk_i8           per query the k smallest keys (d2 << 32 | reference row), d2 = |a|^2 + |b|^2 - 2 <a, b> with the dot
//                           product from v_mfma_i32_16x16x64_i8.
//
// Search kernel.  A workgroup of 4 waves owns NN_QB = 128 queries and walks a contiguous SHARE of the NN_RB = 128-row tiles of b.
// Per 64-byte k step both operand tiles (128 rows x 64 bytes each) go global -> registers -> LDS (the next step's global loads are in
// flight while this step's MFMAs run); LDS rows are 80 bytes apart, so the 16 rows of a fragment read (16 bytes per lane) fall on 16
// different groups of four banks.  A and B are loaded through the SAME byte-to-lane rule -- lane l holds bytes [16 (l >> 4), + 16)
// of row l & 15 of the step -- so whatever order the instruction gives k inside a step, both operands share it and the dot
// product is the dot product; only the C/D map matters: col = lane & 15, row = (lane >> 4) * 4 + reg.  A (rows) is the queries, B
// (columns) the references.  Each wave holds a 64 x 64 corner as 4 x 4 accumulators of 16 x 16, all k steps into the same ones.
// After the k loop the d2 values go to an LDS image [128][128] uint32 (the column index XORed with the row, so that a thread
// walking its row and its neighbours walking theirs hit different banks) that reuses the staging bytes, and thread t folds the 64
// references of half t >> 7 for query t & 127 into 8 sorted registers; the two halves are merged once, after the last tile.  The
// kept list always has 8 entries whatever k is: one code path, and k <= 8 of them are stored.  Keys are distinct (the row is in the
// low word), so the k smallest are one set whatever the order of insertion: the result does not depend on the tiling or the shares.
// Per-share lists go to the workspace as [share][8][Q]; nn_merge_kernel, one thread per query, folds them.  Rows of a tile beyond
// N (and queries beyond Q) are loaded from the last valid row, never from outside the operand, and are dropped when folding.
#include "rg_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int nn_i32x4;

constexpr int NN_QB = 128;            // queries per workgroup
constexpr int NN_RB = 128;            // reference rows per tile
constexpr int NN_LROW = 80;           // bytes between LDS rows of a 64-byte k step
constexpr int NN_KEEP = 8;            // entries of every kept list (k <= 8)
constexpr int NN_TARGET_WGS = 1024;   // shares are cut so that about this many workgroups exist (4 per CU)
constexpr int NN_DMAX = 32768;
constexpr unsigned long long NN_NONE = ~0ull;        // no real key: d2 < 2^31

// the k smallest of a stream: top[] ascending, all NN_NONE at the start
__device__ __forceinline__ void nn_insert(unsigned long long (&top)[NN_KEEP], unsigned long long key) {
#pragma unroll
  for (int i = NN_KEEP - 1; i > 0; --i) top[i] = key < top[i - 1] ? top[i - 1] : (key < top[i] ? key : top[i]);
  top[0] = key < top[0] ? key : top[0];
}

struct nn_plan {
  long long q_blocks, tiles, tiles_per_share, shares;
};

// THE SHARING RULE (include/rnagan_hip.h): with tiles = ceil(N / 128) and q_blocks = ceil(Q / 128), a query block's tiles are cut
// into shares of tiles_per_share = ceil(tiles / max(1, 1024 / q_blocks)) consecutive tiles
nn_plan nn_make_plan(long long Q, long long N) {
  nn_plan p;
  p.q_blocks = (Q + NN_QB - 1) / NN_QB;
  p.tiles = (N + NN_RB - 1) / NN_RB;
  long long want = p.q_blocks > 0 ? NN_TARGET_WGS / p.q_blocks : 1;
  want = want < 1 ? 1 : want;
  p.tiles_per_share = p.tiles > 0 ? (p.tiles + want - 1) / want : 1;
  p.shares = p.tiles > 0 ? (p.tiles + p.tiles_per_share - 1) / p.tiles_per_share : 0;
  return p;
}

__global__ __launch_bounds__(256) void nn_search_kernel(const int8_t* __restrict__ a, const int32_t* __restrict__ na2, int Q,
                                                        const int8_t* __restrict__ b, const int32_t* __restrict__ nb2, int N, int D,
                                                        long long ldd, const int32_t* __restrict__ exclude, int tiles,
                                                        int tiles_per_share, int shares, unsigned long long* __restrict__ ws) {
  // staging: rows 0..127 the queries, 128..255 the references, 80 bytes apart (20 480 bytes); the d2 image takes 65 536
  __shared__ __attribute__((aligned(16))) unsigned char smem[NN_QB * NN_RB * 4];
  uint32_t* img = reinterpret_cast<uint32_t*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int share = (int)(blockIdx.x % (unsigned)shares);
  const long long q0 = (long long)(blockIdx.x / (unsigned)shares) * NN_QB;
  const int wq = w >> 1, wr = w & 1;                   // this wave's 64 x 64 corner of the 128 x 128 tile
  const int lrow = lane & 15, lkg = lane >> 4;

  // global -> LDS: thread t moves 16 bytes of rows (t >> 2) + 64 i, i = 0..3 (i < 2: queries)
  const int srow = tid >> 2, sseg = (tid & 3) * 16;
  const int8_t* ga[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    long long q = q0 + srow + 64 * i;
    q = q < Q ? q : (long long)Q - 1;
    ga[i] = a + q * ldd + sseg;
  }
  // the query this thread folds for
  const long long qf = q0 + (tid & 127);
  const int half = tid >> 7;
  const bool qlive = qf < Q;
  const int excl = (exclude && qlive) ? exclude[qf] : -1;
  unsigned long long top[NN_KEEP];
#pragma unroll
  for (int i = 0; i < NN_KEEP; ++i) top[i] = NN_NONE;
  // the norms of the 16 query rows whose results this lane holds: row = wq 64 + m 16 + lkg 4 + r
  uint32_t qn[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long q = q0 + wq * 64 + m * 16 + lkg * 4 + r;
      qn[m][r] = (uint32_t)na2[q < Q ? q : (long long)Q - 1];
    }

  const int t_begin = share * tiles_per_share;
  const int t_end = min(tiles, t_begin + tiles_per_share);
  const int ksteps = D >> 6;
  for (int t = t_begin; t < t_end; ++t) {
    const long long r0 = (long long)t * NN_RB;
    const int8_t* gb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      long long r = r0 + srow + 64 * i;
      r = r < N ? r : (long long)N - 1;
      gb[i] = b + r * ldd + sseg;
    }
    nn_i32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) acc[m][n] = nn_i32x4{0, 0, 0, 0};
    nn_i32x4 st[4];
    st[0] = *reinterpret_cast<const nn_i32x4*>(ga[0]);
    st[1] = *reinterpret_cast<const nn_i32x4*>(ga[1]);
    st[2] = *reinterpret_cast<const nn_i32x4*>(gb[0]);
    st[3] = *reinterpret_cast<const nn_i32x4*>(gb[1]);
    for (int ks = 0; ks < ksteps; ++ks) {
      __syncthreads();                                 // the previous step's fragment reads, or the previous tile's fold, are done
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<nn_i32x4*>(smem + (srow + 64 * i) * NN_LROW + sseg) = st[i];
      __syncthreads();
      if (ks + 1 < ksteps) {
        const int k1 = (ks + 1) << 6;
        st[0] = *reinterpret_cast<const nn_i32x4*>(ga[0] + k1);
        st[1] = *reinterpret_cast<const nn_i32x4*>(ga[1] + k1);
        st[2] = *reinterpret_cast<const nn_i32x4*>(gb[0] + k1);
        st[3] = *reinterpret_cast<const nn_i32x4*>(gb[1] + k1);
      }
      nn_i32x4 fa[4], fb[4];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        fa[m] = *reinterpret_cast<const nn_i32x4*>(smem + (wq * 64 + m * 16 + lrow) * NN_LROW + lkg * 16);
#pragma unroll
      for (int n = 0; n < 4; ++n)
        fb[n] = *reinterpret_cast<const nn_i32x4*>(smem + (NN_QB + wr * 64 + n * 16 + lrow) * NN_LROW + lkg * 16);
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb[n], acc[m][n], 0, 0, 0);
    }
    __syncthreads();                                   // every wave has read its last fragments: the image may take the bytes
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int col = wr * 64 + n * 16 + lrow;
      const long long r = r0 + col;
      const uint32_t rn = (uint32_t)nb2[r < N ? r : (long long)N - 1];
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = wq * 64 + m * 16 + lkg * 4 + rr;
          // modulo 2^32; with true norms the value is the distance itself, below 2^31
          img[row * NN_RB + (col ^ row)] = qn[m][rr] + rn - 2u * (uint32_t)acc[m][n][rr];
        }
    }
    __syncthreads();
    if (qlive) {
      const int row = tid & 127;
      for (int j = 0; j < 64; ++j) {
        const int col = half * 64 + j;
        const long long r = r0 + col;
        if (r < N && r != (long long)excl) {
          const unsigned long long key = ((unsigned long long)img[row * NN_RB + (col ^ row)] << 32) | (unsigned long long)r;
          if (key < top[NN_KEEP - 1]) nn_insert(top, key);
        }
      }
    }
  }
  // merge the two halves: the upper half hands its list over through LDS
  __syncthreads();
  unsigned long long* hand = reinterpret_cast<unsigned long long*>(smem);
  if (half == 1) {
#pragma unroll
    for (int i = 0; i < NN_KEEP; ++i) hand[i * NN_QB + (tid & 127)] = top[i];
  }
  __syncthreads();
  if (half == 0 && qlive) {
#pragma unroll
    for (int i = 0; i < NN_KEEP; ++i) {
      const unsigned long long key = hand[i * NN_QB + tid];
      if (key < top[NN_KEEP - 1]) nn_insert(top, key);
    }
#pragma unroll
    for (int i = 0; i < NN_KEEP; ++i) ws[((size_t)share * NN_KEEP + i) * (size_t)Q + (size_t)qf] = top[i];
  }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(const unsigned long long* __restrict__ ws, int Q, int shares, int k,
                                                       unsigned long long* __restrict__ keys) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= Q) return;
  unsigned long long top[NN_KEEP];
#pragma unroll
  for (int i = 0; i < NN_KEEP; ++i) top[i] = NN_NONE;
  for (int s = 0; s < shares; ++s)
    for (int i = 0; i < NN_KEEP; ++i) {
      const unsigned long long key = ws[((size_t)s * NN_KEEP + i) * (size_t)Q + (size_t)q];
      if (key >= top[NN_KEEP - 1]) break;              // a share's list ascends: nothing further in it can enter
      nn_insert(top, key);
    }
#pragma unroll
  for (int i = 0; i < NN_KEEP; ++i)
    if (i < k) keys[(size_t)q * k + i] = top[i];
}

// ------------------------------------------------------------------------------------------------ descriptors
// One workgroup per tile.  VEC: an item is 16 consecutive bytes of the f rows of one block row (S % 16 == 0, f <= 16, aligned
// buffers): f 16-byte loads, 16 / f descriptor bytes in one store.  Otherwise a thread forms one value from f x f single bytes.
template <bool VEC>
__global__ __launch_bounds__(256) void nn_desc_kernel(const uint8_t* __restrict__ tiles, int C, int S, int f, int fshift,
                                                      int8_t* __restrict__ desc, long long ldd, int32_t* __restrict__ norm2) {
  __shared__ int red[4];
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x;
  const int P = S >> fshift, D = C * P * P;
  const uint8_t* t = tiles + n * (size_t)C * S * S;
  int8_t* d = desc + n * (size_t)ldd;
  const int rnd = (f * f) >> 1, sh = 2 * fshift;
  int sq = 0;
  if (VEC) {
    const int chunks = S >> 4, per = 16 >> fshift;               // 16-byte chunks per row, values per item
    const int items = C * P * chunks;
    for (int it = tid; it < items; it += 256) {
      const int br = it / chunks, ch = it - br * chunks;        // block row c P + y
      const int c = br / P, y = br - c * P;
      const uint8_t* src = t + ((size_t)c * S + (size_t)y * f) * S + (size_t)ch * 16;
      int colsum[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) colsum[i] = 0;
      for (int dy = 0; dy < f; ++dy) {
        const rg_u32x4 v = *reinterpret_cast<const rg_u32x4*>(src + (size_t)dy * S);
#pragma unroll
        for (int i = 0; i < 16; ++i) colsum[i] += (int)((v[i >> 2] >> (8 * (i & 3))) & 255u);
      }
      // the f columns of a block are neighbours: fshift rounds of pairwise sums leave block o's sum in colsum[o]
#pragma unroll
      for (int lv = 0; lv < 4; ++lv)
        if (lv < fshift) {
#pragma unroll
          for (int i = 0; i < (8 >> lv); ++i) colsum[i] = colsum[2 * i] + colsum[2 * i + 1];
        }
      uint32_t out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        if (o < per) {
          const int s = colsum[o];
          const int v = ((s + rnd) >> sh) - 128;
          sq += v * v;
          out[o >> 2] |= ((uint32_t)v & 255u) << (8 * (o & 3));
        }
      }
      int8_t* dst = d + (size_t)br * P + (size_t)ch * per;
      if (per == 16) *reinterpret_cast<rg_u32x4*>(dst) = rg_u32x4{out[0], out[1], out[2], out[3]};
      else if (per == 8) *reinterpret_cast<rg_u32x2*>(dst) = rg_u32x2{out[0], out[1]};
      else if (per == 4) *reinterpret_cast<uint32_t*>(dst) = out[0];
      else if (per == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)out[0];
      else *dst = (int8_t)out[0];
    }
  } else {
    for (int e = tid; e < D; e += 256) {
      const int x = e % P, cy = e / P;                            // cy = c P + y
      const int c = cy / P, y = cy - c * P;
      const uint8_t* src = t + ((size_t)c * S + (size_t)y * f) * S + (size_t)x * f;
      int s = 0;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) s += (int)src[(size_t)dy * S + dx];
      const int v = ((s + rnd) >> sh) - 128;
      sq += v * v;
      d[e] = (int8_t)v;
    }
  }
  for (long long e = D + tid; e < ldd; e += 256) d[e] = 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) norm2[n] = red[0] + red[1] + red[2] + red[3];
}

bool nn_overlap(const void* p, size_t pb, const void* q, size_t qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qb && b < a + pb;
}

}  // namespace

extern "C" int rg_tile_descriptor_i8(const uint8_t* tiles, int N, int C, int S, int f, int8_t* desc, long long ldd, int32_t* norm2,
                                     void* stream) {
  RG_REQUIRE(tiles && desc && norm2, RG_EINVAL, "tile_descriptor_i8: NULL buffer");
  RG_REQUIRE(N >= 0 && C > 0 && S > 0, RG_EINVAL, "tile_descriptor_i8: bad shape N %d C %d S %d", N, C, S);
  RG_REQUIRE(f == 1 || f == 2 || f == 4 || f == 8 || f == 16 || f == 32, RG_EINVAL, "tile_descriptor_i8: f %d is not 1, 2, 4, 8, 16 or 32", f);
  RG_REQUIRE(S % f == 0, RG_EINVAL, "tile_descriptor_i8: S %d is not a multiple of f %d", S, f);
  const long long P = S / f, D = (long long)C * P * P;
  RG_REQUIRE(ldd > 0 && ldd % 64 == 0 && ldd >= D, RG_EINVAL, "tile_descriptor_i8: ldd %lld is not a multiple of 64 that holds D = %lld", ldd, D);
  RG_REQUIRE(((uintptr_t)norm2 & 3) == 0, RG_EINVAL, "tile_descriptor_i8: norm2 needs 4-byte alignment");
  RG_REQUIRE(D <= NN_DMAX, RG_EUNSUPPORTED, "tile_descriptor_i8: D = %lld is more than %d (squared distances would leave int32)", D, NN_DMAX);
  const size_t tb = (size_t)N * C * S * S, db = (size_t)N * (size_t)ldd, nb = (size_t)N * 4;
  RG_REQUIRE(!nn_overlap(desc, db, tiles, tb) && !nn_overlap(norm2, nb, tiles, tb) && !nn_overlap(norm2, nb, desc, db), RG_EINVAL,
             "tile_descriptor_i8: desc or norm2 overlaps another buffer");
  if (N == 0) return RG_OK;
  hipStream_t st = rg_stream(stream);
  const int fshift = rg_ilog2(f);
  const bool vec = S % 16 == 0 && f <= 16 && ((uintptr_t)tiles & 15) == 0 && ((uintptr_t)desc & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(nn_desc_kernel<true>, dim3((unsigned)N), dim3(256), 0, st, tiles, C, S, f, fshift, desc, ldd, norm2);
  else
    hipLaunchKernelGGL(nn_desc_kernel<false>, dim3((unsigned)N), dim3(256), 0, st, tiles, C, S, f, fshift, desc, ldd, norm2);
  RG_LAUNCH_CHECK("tile_descriptor_i8");
  return RG_OK;
}

extern "C" size_t rg_nn_topk_ws_bytes(int Q, long long N, int k) {
  (void)k;                                                        // every kept list has 8 entries
  if (Q <= 0 || N <= 0) return 0;
  const nn_plan p = nn_make_plan(Q, N);
  return (size_t)p.shares * NN_KEEP * (size_t)Q * sizeof(unsigned long long);
}

extern "C" int rg_nn_topk_i8(const int8_t* a, const int32_t* na2, int Q, const int8_t* b, const int32_t* nb2, long long N, int D,
                             long long ldd, int k, const int32_t* exclude, uint64_t* keys, void* ws, size_t ws_bytes, void* stream) {
  RG_REQUIRE(Q >= 0 && N >= 0 && N <= 0x7fffffffLL, RG_EINVAL, "nn_topk_i8: bad Q %d or N %lld", Q, N);
  RG_REQUIRE(k >= 1 && k <= NN_KEEP, RG_EINVAL, "nn_topk_i8: k %d is not in 1..%d", k, NN_KEEP);
  RG_REQUIRE(D > 0 && D % 64 == 0, RG_EINVAL, "nn_topk_i8: D %d is not a positive multiple of 64", D);
  RG_REQUIRE(ldd >= D && ldd % 16 == 0, RG_EINVAL, "nn_topk_i8: ldd %lld is not a multiple of 16 that holds D = %d", ldd, D);
  RG_REQUIRE(D <= NN_DMAX, RG_EUNSUPPORTED, "nn_topk_i8: D = %d is more than %d (squared distances would leave int32)", D, NN_DMAX);
  if (Q == 0) return RG_OK;
  RG_REQUIRE(a && na2 && b && nb2 && keys, RG_EINVAL, "nn_topk_i8: NULL buffer");
  RG_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 15) == 0 && (((uintptr_t)na2 | (uintptr_t)nb2 | (uintptr_t)exclude) & 3) == 0, RG_EINVAL,
             "nn_topk_i8: a and b need 16-byte, the int32 operands 4-byte alignment");
  RG_REQUIRE(((uintptr_t)keys & 7) == 0 && ((uintptr_t)ws & 7) == 0, RG_EINVAL, "nn_topk_i8: keys and ws need 8-byte alignment");
  // fewer than k candidates: N itself decides unless an exclusion is given (then one row may leave: the device values are not read
  // here, so N - 1 must do)
  RG_REQUIRE(N - (exclude ? 1 : 0) >= k, RG_EINVAL, "nn_topk_i8: %lld reference rows%s are fewer than k = %d candidates", N,
             exclude ? " less one that may be excluded" : "", k);
  const nn_plan p = nn_make_plan(Q, N);
  RG_REQUIRE(p.q_blocks * p.shares <= 0x7fffffffLL, RG_EUNSUPPORTED, "nn_topk_i8: Q %d N %lld is more than 2^31 - 1 workgroups", Q, N);
  const size_t need = rg_nn_topk_ws_bytes(Q, N, k);
  RG_REQUIRE(ws && ws_bytes >= need, RG_EWORKSPACE, "nn_topk_i8: workspace of %zu bytes, %zu needed", ws_bytes, need);
  hipStream_t st = rg_stream(stream);
  hipLaunchKernelGGL(nn_search_kernel, dim3((unsigned)(p.q_blocks * p.shares)), dim3(256), 0, st, a, na2, Q, b, nb2, (int)N, D, ldd,
                     exclude, (int)p.tiles, (int)p.tiles_per_share, (int)p.shares, (unsigned long long*)ws);
  RG_LAUNCH_CHECK("nn_topk_i8");
  hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)ws, Q,
                     (int)p.shares, k, (unsigned long long*)keys);
  RG_LAUNCH_CHECK("nn_topk_i8 (merge)");
  return RG_OK;
}
