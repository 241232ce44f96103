// rg_u8px.h -- the pixel stream of uint8 RGB tiles shared by the stain kernels (rg_stain.hip) and the tile-QC histogram pass
// (rg_tissue.hip): a workgroup of 256 lanes owns `chunk` consecutive pixels and hands every one of them to a functor as (R, G, B).
//
// Layouts.  A set is N tiles of H x W pixels, interleaved ([N][H][W][3]) or planar (RG_EXPORT_PLANAR: [N][3][H][W]), the three
// stored channels R, G, B or (RG_EXPORT_REVERSE) B, G, R.  A planar set is chunked tile by tile.  An interleaved set is ONE stream
// of N H W pixels (per_tile = false: the caller's result is over the set, tiles do not matter) or is chunked tile by tile as well
// (per_tile = true: the caller's counters are per tile).  Workgroup b owns pixels [(b % chunks) chunk, + chunk) of stream
// b / chunks, cut at the stream's end; stream n starts at byte n 3 HW.
//
// vec.  A lane takes 4 pixels from three dword loads where every stream, plane and chunk starts on a dword: the base is 4-byte
// aligned (the caller says so: `aligned`), chunk % 4 == 0, and, where the set is chunked per tile, H W % 4 == 0 -- tile n starts at
// byte n 3 H W and a plane at a multiple of H W.  Otherwise single bytes.  The up to 3 pixels a stream's last chunk leaves after
// its quads go through the byte loop too.  Both paths hand the functor the same integers.
//
// The functor.  f.px(R, G, B) once per pixel, the channels as int in 0..255 and in R, G, B order whatever the stored order;
// f.flush() after at most four of them (a lane may sum a quad in narrow registers and widen once).  No order of pixels is
// promised, within a lane or between lanes: a functor accumulates with operations that commute.
//
// Storing (u8px_map).  px takes the three channels by reference and leaves the bytes to store in them, again in R, G, B order; the
// stream puts them back where and in the order it read them.  dst == src is legal: a lane reads all the bytes of its pixels before
// it writes any of them, and no other lane touches those bytes.  Any other overlap of dst and src is the caller's to refuse.
#pragma once
#include "rg_common.h"

namespace {

struct u8px_geom {
  long long HW;      // pixels per stream: of a tile, or of the whole set
  unsigned chunks;   // workgroups per stream
  int chunk, planar, reverse, vec;
};

// Shape and flags -> the geometry and the number of workgroups (0 for N == 0), under the caller's error prefix.  The caller's own
// limit on the pixels of a call (N H W <= 2^33 at the most, wherever the shape is valid) is checked in front of this.
inline int u8px_plan(const char* what, int N, int H, int W, int flags, int chunk, bool aligned, bool per_tile, u8px_geom* g,
                     unsigned* blocks) {
  RG_REQUIRE(N >= 0 && H > 0 && W > 0, RG_EINVAL, "%s: bad shape N %d H %d W %d", what, N, H, W);
  RG_REQUIRE((flags & ~(RG_EXPORT_PLANAR | RG_EXPORT_REVERSE)) == 0, RG_EINVAL, "%s: unknown flag bits 0x%x", what, flags);
  const long long HW = (long long)H * W;
  g->planar = (flags & RG_EXPORT_PLANAR) != 0;
  g->reverse = (flags & RG_EXPORT_REVERSE) != 0;
  g->chunk = chunk;
  const bool tiled = g->planar || per_tile;
  g->HW = tiled ? HW : HW * N;                               // not tiled: one stream of pixels
  const long long per = (g->HW + chunk - 1) / chunk;
  const long long total = tiled ? per * N : per;             // < 2^33 / chunk + 2^31
  RG_REQUIRE(total <= 0x7fffffffLL, RG_EUNSUPPORTED, "%s: N %d H %d W %d is more than 2^31 - 1 workgroups", what, N, H, W);
  g->chunks = (unsigned)(per > 0 ? per : 1);
  g->vec = aligned && chunk % 4 == 0 && (!tiled || HW % 4 == 0);
  *blocks = (unsigned)total;
  return RG_OK;
}

__device__ __forceinline__ int u8px_byte(const uint32_t* w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }

// pixel p of the tile at t (HW pixels)
__device__ __forceinline__ void u8px_load(const uint8_t* __restrict__ t, size_t HW, size_t p, int planar, int reverse, int& R, int& G,
                                          int& B) {
  int c0, c2;
  if (planar) {
    c0 = t[p]; G = t[HW + p]; c2 = t[2 * HW + p];
  } else {
    c0 = t[3 * p]; G = t[3 * p + 1]; c2 = t[3 * p + 2];
  }
  R = reverse ? c2 : c0;
  B = reverse ? c0 : c2;
}

// One pixel through the functor: (c0, c1, c2) as stored; STORE: o takes the functor's bytes, as stored.  The reading form hands the
// functor VALUES: through references the statistics kernels of rg_stain.hip compile to more registers.
template <bool STORE, typename F>
__device__ __forceinline__ void u8px_px(F& f, int reverse, int c0, int c1, int c2, int (&o)[3]) {
  if constexpr (STORE) {
    int R = reverse ? c2 : c0, G = c1, B = reverse ? c0 : c2;
    f.px(R, G, B);
    o[0] = reverse ? B : R;
    o[1] = G;
    o[2] = reverse ? R : B;
  } else {
    f.px(reverse ? c2 : c0, c1, reverse ? c0 : c2);
  }
}

// the pixel whose channels are bytes k0, k1, k2 of the quad's three words w; STORE: its new bytes go to the same places of r
template <bool STORE, typename F>
__device__ __forceinline__ void u8px_quad_px(F& f, int reverse, const uint32_t* w, uint32_t* r, int k0, int k1, int k2) {
  int o[3];
  u8px_px<STORE>(f, reverse, u8px_byte(w, k0), u8px_byte(w, k1), u8px_byte(w, k2), o);
  if constexpr (STORE) {
    r[k0 >> 2] |= (uint32_t)o[0] << (8 * (k0 & 3));
    r[k1 >> 2] |= (uint32_t)o[1] << (8 * (k1 & 3));
    r[k2 >> 2] |= (uint32_t)o[2] << (8 * (k2 & 3));
  }
}

// src and dst are NOT restrict: dst == src is the in-place call (the rule at the top).  dst is not used unless STORE.
template <bool STORE, typename F>
__device__ __forceinline__ void u8px_stream(const uint8_t* src, uint8_t* dst, const u8px_geom& g, F& f) {
  const int tid = threadIdx.x;
  const size_t n = blockIdx.x / g.chunks;
  const long long p0 = (long long)(blockIdx.x % g.chunks) * g.chunk;
  const long long left = g.HW - p0;
  const int cnt = left < (long long)g.chunk ? (int)left : g.chunk;
  const size_t HW = (size_t)g.HW;
  const uint8_t* t = src + n * 3 * HW;
  uint8_t* u = STORE ? dst + n * 3 * HW : nullptr;
  int done = 0;
  if (g.vec) {
    const int quads = cnt >> 2;
    for (int q = tid; q < quads; q += 256) {
      const size_t p = (size_t)p0 + 4 * (size_t)q;
      uint32_t w[3], r[3] = {0u, 0u, 0u};
      if (g.planar) {
        w[0] = *reinterpret_cast<const uint32_t*>(t + p);
        w[1] = *reinterpret_cast<const uint32_t*>(t + HW + p);
        w[2] = *reinterpret_cast<const uint32_t*>(t + 2 * HW + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) u8px_quad_px<STORE>(f, g.reverse, w, r, j, 4 + j, 8 + j);
        if constexpr (STORE) {
          *reinterpret_cast<uint32_t*>(u + p) = r[0];
          *reinterpret_cast<uint32_t*>(u + HW + p) = r[1];
          *reinterpret_cast<uint32_t*>(u + 2 * HW + p) = r[2];
        }
      } else {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(t + 3 * p);
        w[0] = s4[0]; w[1] = s4[1]; w[2] = s4[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) u8px_quad_px<STORE>(f, g.reverse, w, r, 3 * j, 3 * j + 1, 3 * j + 2);
        if constexpr (STORE) {
          uint32_t* d4 = reinterpret_cast<uint32_t*>(u + 3 * p);
          d4[0] = r[0]; d4[1] = r[1]; d4[2] = r[2];
        }
      }
      f.flush();
    }
    done = quads << 2;                               // chunked per tile: cnt % 4 == 0 here; one stream: its last chunk may leave up to 3
  }
  for (int i = done + tid; i < cnt; i += 256) {
    const size_t p = (size_t)p0 + (size_t)i;
    int c0, c1, c2, o[3];
    if (g.planar) {                                  // (not u8px_load: see u8px_px)
      c0 = t[p]; c1 = t[HW + p]; c2 = t[2 * HW + p];
    } else {
      c0 = t[3 * p]; c1 = t[3 * p + 1]; c2 = t[3 * p + 2];
    }
    u8px_px<STORE>(f, g.reverse, c0, c1, c2, o);
    f.flush();
    if constexpr (STORE) {
      if (g.planar) {
        u[p] = (uint8_t)o[0]; u[HW + p] = (uint8_t)o[1]; u[2 * HW + p] = (uint8_t)o[2];
      } else {
        u[3 * p] = (uint8_t)o[0]; u[3 * p + 1] = (uint8_t)o[1]; u[3 * p + 2] = (uint8_t)o[2];
      }
    }
  }
}

// every pixel of this workgroup's chunk: f.px(R, G, B) per pixel, f.flush() after at most four of them
template <typename F>
__device__ __forceinline__ void u8px_each(const uint8_t* __restrict__ tiles, const u8px_geom& g, F& f) {
  u8px_stream<false>(tiles, nullptr, g, f);
}

// the same with f.px(int& R, int& G, int& B) and its bytes stored at the pixel's place in dst
template <typename F>
__device__ __forceinline__ void u8px_map(const uint8_t* src, uint8_t* dst, const u8px_geom& g, F& f) {
  u8px_stream<true>(src, dst, g, f);
}

// Zeroes `words` dwords (4-byte aligned) on the stream with a kernel in front of the counting one, not a memset node: the launches
// of a captured call then form one plain chain of kernel nodes.  A grid-stride fill: at most 2^20 workgroups whatever `words` is.
__global__ __launch_bounds__(256) void u8px_zero_kernel(unsigned* __restrict__ p, size_t words) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) p[i] = 0u;
}

inline int u8px_zero(const char* what, void* p, size_t words, hipStream_t st) {
  const size_t blocks = (words + 2 * 256 - 1) / (2 * 256);   // two dwords per lane: the grid the stain outputs (64-bit words) always had
  hipLaunchKernelGGL(u8px_zero_kernel, dim3((unsigned)(blocks < (1u << 20) ? blocks : (1u << 20))), dim3(256), 0, st, (unsigned*)p, words);
  RG_LAUNCH_CHECK(what);
  return RG_OK;
}

}  // namespace
