// rg_augment.hip -- the device-side input transform: uint8 / fp32 tiles -> normalised fp32 NCHW, with one of the eight
// symmetries of the square (D4) per sample, in ONE launch that touches every pixel once (rg_tile_transform).
//
// Bandwidth-bound: 1 B (uint8) or 4 B (fp32) read and 4 B written per pixel.  Every code goes through the same path: a workgroup
// owns one 64 x 64 tile of one OUTPUT plane, fetches the source tile that maps onto it with coalesced row reads, converts at the
// LDS store (LDS holds final fp32 values for both source types) and reads the tile back along the output's rows.  The code is
// uniform per workgroup; the eight index maps differ only in WHICH source tile is fetched and in the sign of the two in-tile
// steps, so the transposing codes (1, 3, 5, 7) never read global memory with a stride of S.  The LDS pitch is 65 dwords: a
// column walk (address step 65) visits bank (l + c) % 32 for lane l, conflict-free like a row walk.  No 16-bit type is
// involved: both builds of the library behave identically.
// rg_tile_gather_transform is the same kernel with a per-sample SOURCE tile: the batches of a training set that lives on the
// device as uint8 (rna_gan_amd.resident) are gathered by index, normalised and transformed in that one launch.
#include "rg_common.h"

namespace {

constexpr int TT_TILE = 64;            // tile edge
constexpr int TT_PITCH = 65;           // LDS row pitch in dwords (odd: rows and columns are both conflict-free walks)

template <typename SrcT> struct TileSrc;
template <> struct TileSrc<uint8_t> {
  // the same three fp32 operations, in the same order, as u8_to_norm_kernel (rg_misc.hip) and the host transform
  __device__ static __forceinline__ float cvt(uint8_t b, float mean, float stdv) { return ((float)b / 255.0f - mean) / stdv; }
  __device__ static __forceinline__ void ld4(const uint8_t* p, float* o, float mean, float stdv) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
    o[0] = cvt((uint8_t)(w & 0xffu), mean, stdv);
    o[1] = cvt((uint8_t)((w >> 8) & 0xffu), mean, stdv);
    o[2] = cvt((uint8_t)((w >> 16) & 0xffu), mean, stdv);
    o[3] = cvt((uint8_t)(w >> 24), mean, stdv);
  }
};
template <> struct TileSrc<float> {
  __device__ static __forceinline__ float cvt(float v, float, float) { return v; }
  __device__ static __forceinline__ void ld4(const float* p, float* o, float, float) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  }
};

// code = r + 4 f: flip left-right if f, then rotate counter-clockwise by r quarter turns.  With T = S - 1 the source of output
// pixel (i, j) is src[row(u)][col(v)], where (u, v) = (i, j) for the even codes and (j, i) for the odd (transposing) ones,
// row(u) = rflip ? T - u : u and col(v) = cflip ? T - v : v:
//   code   0       1        2          3        4        5       6        7
//   src  [i][j] [j][T-i] [T-i][T-j] [T-j][i] [i][T-j] [j][i]  [T-i][j] [T-j][T-i]
// VEC: S % 4 == 0 and both buffers aligned to four elements -- every tile origin, tile width and plane offset is then a multiple
// of 4, and the tile is fetched and stored four elements per lane.
// GATHER (rg_tile_gather_transform): sample n reads tile index[n] (NULL: n) of a store of M tiles instead of tile n of the batch.
// The index is read once per workgroup, next to the code, clamped into [0, M) and widened before the multiplication; nothing
// else differs, and without GATHER the two extra arguments are never looked at.
template <typename SrcT, bool VEC, bool GATHER>
__global__ __launch_bounds__(256) void tile_transform_kernel(const SrcT* __restrict__ src, float* __restrict__ dst, int C, int S,
                                                             int tiles, const int* __restrict__ codes, float mean, float stdv,
                                                             const int* __restrict__ index, long long M) {
  __shared__ float lds[TT_TILE * TT_PITCH];
  const int tid = threadIdx.x;
  const int per_plane = tiles * tiles;
  const int plane = blockIdx.x / per_plane, tile = blockIdx.x % per_plane;
  const int code = codes ? (codes[plane / C] & 7) : 0;           // uniform: one sample, one code
  const bool tr = (code & 1) != 0;
  const bool rflip = code == 2 || code == 3 || code == 6 || code == 7;
  const bool cflip = code == 1 || code == 2 || code == 4 || code == 7;
  const int i0 = (tile / tiles) * TT_TILE, j0 = (tile % tiles) * TT_TILE;       // the output tile
  const int hi = min(TT_TILE, S - i0), wj = min(TT_TILE, S - j0);
  // the source tile: nu rows from r0, nv columns from c0 (inside the plane by construction: 0 <= r0, r0 + nu <= S, the same for c)
  const int u0 = tr ? j0 : i0, nu = tr ? wj : hi;
  const int v0 = tr ? i0 : j0, nv = tr ? hi : wj;
  const int r0 = rflip ? S - u0 - nu : u0;
  const int c0 = cflip ? S - v0 - nv : v0;
  const size_t base = (size_t)plane * S * S;
  size_t sbase = base;
  if (GATHER) {
    const int n = plane / C;
    long long t = index ? (long long)index[n] : (long long)n;    // uniform: one sample, one source tile
    t = t < 0 ? 0 : (t >= M ? M - 1 : t);                        // a bad index reads a valid tile, never outside the store
    sbase = ((size_t)t * C + (size_t)(plane - n * C)) * S * S;   // 64-bit throughout: t C S S passes 2^32 in a resident set
  }
  const SrcT* sp = src + sbase;
  float* dp = dst + base;

  // ---- fetch: coalesced rows of the source tile, converted at the LDS store
  if (VEC) {
    const int q = (tid & 15) * 4, r = tid >> 4;                  // 16 lanes x 4 elements per row, 16 rows per pass
    if (q < nv) {
#pragma unroll
      for (int p = 0; p < TT_TILE / 16; ++p) {
        const int lr = r + 16 * p;
        if (lr < nu) {
          float v[4];
          TileSrc<SrcT>::ld4(sp + (size_t)(r0 + lr) * S + (c0 + q), v, mean, stdv);
          float* l = lds + lr * TT_PITCH + q;
          l[0] = v[0]; l[1] = v[1]; l[2] = v[2]; l[3] = v[3];
        }
      }
    }
  } else {
    const int lc = tid & 63, r = tid >> 6;                       // one wave per row, 4 rows per pass
    if (lc < nv) {
#pragma unroll 4
      for (int p = 0; p < TT_TILE / 4; ++p) {
        const int lr = r + 4 * p;
        if (lr < nu) lds[lr * TT_PITCH + lc] = TileSrc<SrcT>::cvt(sp[(size_t)(r0 + lr) * S + (c0 + lc)], mean, stdv);
      }
    }
  }
  __syncthreads();

  // ---- store: output pixel (li, lj) of the tile reads lds[lr(lu)][lc(lv)], (lu, lv) = (li, lj) or (lj, li);
  // lr(lu) = rflip ? nu - 1 - lu : lu, lc(lv) = cflip ? nv - 1 - lv : lv.  Along an output row the LDS address moves by `step`.
  const int step = tr ? (rflip ? -TT_PITCH : TT_PITCH) : (cflip ? -1 : 1);
  if (VEC) {
    // a wave stores 8 rows x 32 columns (8 lanes x float4 = one 128-byte line per row): the 32 lanes of a half wave are 4 rows x
    // 8 quads, whose dwords sit on banks (li + 4 q + k) % 32 for either walk -- all different
    const int lane = tid & 63, w = tid >> 6;
    const int q = (lane & 7) * 4, rr = lane >> 3;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int idx = p * 4 + w;
      const int li = (idx >> 1) * 8 + rr, lj = (idx & 1) * 32 + q;
      if (li < hi && lj < wj) {
        const int lu = tr ? lj : li, lv = tr ? li : lj;
        const int a = (rflip ? nu - 1 - lu : lu) * TT_PITCH + (cflip ? nv - 1 - lv : lv);
        float4 o;
        o.x = lds[a]; o.y = lds[a + step]; o.z = lds[a + 2 * step]; o.w = lds[a + 3 * step];
        *reinterpret_cast<float4*>(dp + (size_t)(i0 + li) * S + (j0 + lj)) = o;
      }
    }
  } else {
    const int lj = tid & 63, r = tid >> 6;
    if (lj < wj) {
#pragma unroll 4
      for (int p = 0; p < TT_TILE / 4; ++p) {
        const int li = r + 4 * p;
        if (li < hi) {
          const int lu = tr ? lj : li, lv = tr ? li : lj;
          dp[(size_t)(i0 + li) * S + (j0 + lj)] = lds[(rflip ? nu - 1 - lu : lu) * TT_PITCH + (cflip ? nv - 1 - lv : lv)];
        }
      }
    }
  }
}

template <typename SrcT>
void launch_tile_transform(const void* src, float* dst, int C, int S, int tiles, unsigned blocks, const int* codes, float mean,
                           float stdv, hipStream_t st) {
  // four elements of either buffer per access: S % 4 == 0 keeps every row, tile and plane a multiple of 4 from the base
  const bool vec = S % 4 == 0 && ((uintptr_t)src & (4 * sizeof(SrcT) - 1)) == 0 && ((uintptr_t)dst & 15) == 0;
  if (vec)
    hipLaunchKernelGGL((tile_transform_kernel<SrcT, true, false>), dim3(blocks), dim3(256), 0, st, (const SrcT*)src, dst, C, S,
                       tiles, codes, mean, stdv, (const int*)nullptr, 0LL);
  else
    hipLaunchKernelGGL((tile_transform_kernel<SrcT, false, false>), dim3(blocks), dim3(256), 0, st, (const SrcT*)src, dst, C, S,
                       tiles, codes, mean, stdv, (const int*)nullptr, 0LL);
}

}  // namespace

extern "C" int rg_tile_transform(const void* src, int src_dtype, float* dst, int N, int C, int S, const int* codes, float mean,
                                 float stdv, void* stream) {
  RG_REQUIRE(src && dst, RG_EINVAL, "tile_transform: NULL buffer");
  RG_REQUIRE(N >= 0 && C > 0 && S > 0, RG_EINVAL, "tile_transform: bad shape N %d C %d S %d", N, C, S);
  RG_REQUIRE(src_dtype == RG_U8 || src_dtype == RG_F32, RG_EINVAL, "tile_transform: src_dtype %d is neither RG_U8 nor RG_F32",
             src_dtype);
  RG_REQUIRE(src_dtype != RG_U8 || stdv != 0.f, RG_EINVAL, "tile_transform: std must not be 0");
  if (N == 0) return RG_OK;
  const int tiles = (S + TT_TILE - 1) / TT_TILE;
  const long long blocks = (long long)N * C * tiles * tiles;
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "tile_transform: more than 2^31 - 1 tiles");
  if (src_dtype == RG_U8)
    launch_tile_transform<uint8_t>(src, dst, C, S, tiles, (unsigned)blocks, codes, mean, stdv, rg_stream(stream));
  else
    launch_tile_transform<float>(src, dst, C, S, tiles, (unsigned)blocks, codes, mean, stdv, rg_stream(stream));
  RG_LAUNCH_CHECK("tile_transform");
  return RG_OK;
}

// The resident training set (rna_gan_amd.resident): the same launch plan with a per-sample source tile.  S % 4 == 0 makes C S S
// a multiple of 4, so every gathered tile is as aligned as the store's base and one test chooses the path for all of them.
extern "C" int rg_tile_gather_transform(const uint8_t* store, long long M, const int* index, float* dst, int N, int C, int S,
                                        const int* codes, float mean, float stdv, void* stream) {
  RG_REQUIRE(store && dst, RG_EINVAL, "tile_gather_transform: NULL buffer");
  RG_REQUIRE(N >= 0 && C > 0 && S > 0, RG_EINVAL, "tile_gather_transform: bad shape N %d C %d S %d", N, C, S);
  RG_REQUIRE(M > 0 || N == 0, RG_EINVAL, "tile_gather_transform: a store of %lld tiles cannot fill %d samples", M, N);
  RG_REQUIRE(stdv != 0.f, RG_EINVAL, "tile_gather_transform: std must not be 0");
  RG_REQUIRE(index || (long long)N <= M, RG_EINVAL, "tile_gather_transform: no index and N %d > M %lld", N, M);
  if (N == 0) return RG_OK;
  const int tiles = (S + TT_TILE - 1) / TT_TILE;
  const long long blocks = (long long)N * C * tiles * tiles;
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "tile_gather_transform: more than 2^31 - 1 tiles");
  const bool vec = S % 4 == 0 && ((uintptr_t)store & 3) == 0 && ((uintptr_t)dst & 15) == 0;
  hipStream_t st = rg_stream(stream);
  if (vec)
    hipLaunchKernelGGL((tile_transform_kernel<uint8_t, true, true>), dim3((unsigned)blocks), dim3(256), 0, st, store, dst, C, S,
                       tiles, codes, mean, stdv, index, M);
  else
    hipLaunchKernelGGL((tile_transform_kernel<uint8_t, false, true>), dim3((unsigned)blocks), dim3(256), 0, st, store, dst, C, S,
                       tiles, codes, mean, stdv, index, M);
  RG_LAUNCH_CHECK("tile_gather_transform");
  return RG_OK;
}
