// rg_export.hip -- the device-side tile export: generated fp32 NCHW images -> uint8 tiles in ONE launch (rg_tile_export_u8),
// interleaved [N][H][W][C] (what a PNG or a tile record takes) or planar [N][C][H][W] (what the datasets hand to
// rg_tile_transform / rg_resize_bilinear01), optionally with the channels reversed (BGR, the order of the reference's records).
//
// A pure stream: 4 C bytes read and C bytes written per pixel, nothing reused, so no pass through LDS -- the interleave happens in
// registers.  Three kernels, the same bytes from each:
//   * interleaved, C == 3, W % 4 == 0, src 16-byte and dst 4-byte aligned: a lane owns 4 consecutive pixels of a row.  It issues
//     three independent 16-byte loads, one per plane and each coalesced along the row (a wave reads 1 KiB per plane), packs the 12
//     bytes into three dwords and stores them as one contiguous 12-byte piece: a wave writes 768 contiguous bytes.
//   * planar (and C == 1, where the two layouts coincide), H W % 4 == 0, the same alignments: a lane owns 4 consecutive pixels
//     of one plane, one 16-byte load and one dword store (a wave writes 256 contiguous bytes, the shape that stores at the full rate); a workgroup walks four such rows of
//     quads, so every lane has four independent loads in flight.  (16 pixels per lane and one 16-byte store would put the lanes of
//     a load 64 bytes apart: four instructions per cache line instead of one.)
//   * everything else (other C, ragged W, odd alignment): one bounds-checked lane per output byte.  Its speed is no criterion.
// Every arithmetic step is a separately rounded fp32 operation (contraction off, a true division); no 16-bit type is involved, so
// both builds of the library behave identically.
#include "rg_common.h"

#pragma clang fp contract(off)

namespace {

// the contract's byte: v = (x - sub) / div; t = v * 255 (+ 0.5 under the rounding rule); 0 if !(t >= 0) (NaN and -0.0 included),
// 255 if t >= 255, otherwise t truncated toward zero
template <bool TRUNC>
__device__ __forceinline__ uint32_t export_byte(float x, float sub, float div) {
  const float v = (x - sub) / div;
  float t = v * 255.0f;
  if (!TRUNC) t = t + 0.5f;
  if (!(t >= 0.0f)) return 0u;
  if (t >= 255.0f) return 255u;
  return (uint32_t)t;
}

template <bool TRUNC>
__device__ __forceinline__ uint32_t export_pack4(float a, float b, float c, float d, float sub, float div) {
  return export_byte<TRUNC>(a, sub, div) | (export_byte<TRUNC>(b, sub, div) << 8) | (export_byte<TRUNC>(c, sub, div) << 16) |
         (export_byte<TRUNC>(d, sub, div) << 24);
}

struct __attribute__((aligned(4))) bytes12 { uint32_t a, b, c; };

// quads = N * HW / 4 quads of pixels; quad q = (n, p): pixels 4 p .. 4 p + 3 of sample n
template <bool TRUNC>
__global__ __launch_bounds__(256) void export_rgb4_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t quads,
                                                          int HW4, int reverse, float sub, float div) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const size_t n = q / (size_t)HW4, p = q % (size_t)HW4;
  const size_t plane = (size_t)HW4 * 4;
  const float* s = src + n * 3 * plane + p * 4;
  const float4 c0 = *reinterpret_cast<const float4*>(s + (reverse ? 2 * plane : 0));
  const float4 c1 = *reinterpret_cast<const float4*>(s + plane);
  const float4 c2 = *reinterpret_cast<const float4*>(s + (reverse ? 0 : 2 * plane));
  bytes12 o;
  o.a = export_pack4<TRUNC>(c0.x, c1.x, c2.x, c0.y, sub, div);
  o.b = export_pack4<TRUNC>(c1.y, c2.y, c0.z, c1.z, sub, div);
  o.c = export_pack4<TRUNC>(c2.z, c0.w, c1.w, c2.w, sub, div);
  *reinterpret_cast<bytes12*>(dst + q * 12) = o;
}

// quads = N * C * HW / 4; a workgroup owns 1024 consecutive quads, lane t the quads t, t + 256, t + 512, t + 768 of them
template <bool TRUNC>
__global__ __launch_bounds__(256) void export_planar4_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t quads,
                                                             int HW4, int C, int reverse, float sub, float div) {
  const size_t q0 = (size_t)blockIdx.x * 1024 + threadIdx.x;
  float4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t q = q0 + 256 * k;
    if (q < quads) {
      size_t sq = q;
      if (reverse) {
        const size_t pl = q / (size_t)HW4, p = q % (size_t)HW4;
        const size_t n = pl / (size_t)C, c = pl % (size_t)C;
        sq = (n * C + (C - 1 - c)) * (size_t)HW4 + p;
      }
      v[k] = *reinterpret_cast<const float4*>(src + sq * 4);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t q = q0 + 256 * k;
    if (q < quads) *reinterpret_cast<uint32_t*>(dst + q * 4) = export_pack4<TRUNC>(v[k].x, v[k].y, v[k].z, v[k].w, sub, div);
  }
}

// one lane per output byte i < total
template <bool TRUNC>
__global__ __launch_bounds__(256) void export_scalar_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t total,
                                                            int C, size_t HW, int planar, int reverse, float sub, float div) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  size_t n, c, p;
  if (planar) {
    p = i % HW;
    const size_t pl = i / HW;
    c = pl % (size_t)C; n = pl / (size_t)C;
  } else {
    c = i % (size_t)C;
    const size_t t = i / (size_t)C;
    p = t % HW; n = t / HW;
  }
  const size_t sc = reverse ? (size_t)C - 1 - c : c;
  dst[i] = (uint8_t)export_byte<TRUNC>(src[(n * C + sc) * HW + p], sub, div);
}

}  // namespace

extern "C" int rg_tile_export_u8(const float* src, uint8_t* dst, int N, int C, int H, int W, float sub, float div, int flags,
                                 void* stream) {
  RG_REQUIRE(src && dst, RG_EINVAL, "tile_export_u8: NULL buffer");
  RG_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0, RG_EINVAL, "tile_export_u8: bad shape N %d C %d H %d W %d", N, C, H, W);
  RG_REQUIRE(div == div && div != 0.f, RG_EINVAL, "tile_export_u8: div must be neither 0 nor NaN");
  RG_REQUIRE((flags & ~(RG_EXPORT_PLANAR | RG_EXPORT_REVERSE | RG_EXPORT_TRUNC)) == 0, RG_EINVAL,
             "tile_export_u8: unknown flag bits 0x%x", flags);
  if (N == 0) return RG_OK;
  // no path covers more than 4096 elements per workgroup: beyond this the grid overflows whatever the path (and below it every
  // product of the four extents fits a size_t)
  RG_REQUIRE((unsigned __int128)N * C * H * W <= (unsigned __int128)0x7fffffffULL * 4096, RG_EUNSUPPORTED,
             "tile_export_u8: N %d C %d H %d W %d is more than 2^31 - 1 workgroups", N, C, H, W);
  const bool planar = (flags & RG_EXPORT_PLANAR) != 0, trunc = (flags & RG_EXPORT_TRUNC) != 0;
  const int reverse = (flags & RG_EXPORT_REVERSE) != 0 && C > 1;
  const size_t HW = (size_t)H * W;
  const size_t total = (size_t)N * C * HW;
  const bool aligned = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0;
  hipStream_t st = rg_stream(stream);
  const size_t limit = 0x7fffffffULL;
  if (!planar && C == 3 && W % 4 == 0 && aligned && HW / 4 <= limit) {
    const size_t quads = (size_t)N * (HW / 4);
    const size_t blocks = (quads + 255) / 256;
    RG_REQUIRE(blocks <= limit, RG_EUNSUPPORTED, "tile_export_u8: more than 2^31 - 1 workgroups");
    if (trunc)
      hipLaunchKernelGGL((export_rgb4_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, quads, (int)(HW / 4),
                         reverse, sub, div);
    else
      hipLaunchKernelGGL((export_rgb4_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, quads, (int)(HW / 4),
                         reverse, sub, div);
  } else if ((planar || C == 1) && HW % 4 == 0 && aligned && HW / 4 <= limit) {
    const size_t quads = total / 4;
    const size_t blocks = (quads + 1023) / 1024;
    RG_REQUIRE(blocks <= limit, RG_EUNSUPPORTED, "tile_export_u8: more than 2^31 - 1 workgroups");
    if (trunc)
      hipLaunchKernelGGL((export_planar4_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, quads, (int)(HW / 4),
                         C, reverse, sub, div);
    else
      hipLaunchKernelGGL((export_planar4_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, quads, (int)(HW / 4),
                         C, reverse, sub, div);
  } else {
    const size_t blocks = (total + 255) / 256;
    RG_REQUIRE(blocks <= limit, RG_EUNSUPPORTED, "tile_export_u8: more than 2^31 - 1 workgroups");
    if (trunc)
      hipLaunchKernelGGL((export_scalar_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, total, C, HW,
                         (int)planar, reverse, sub, div);
    else
      hipLaunchKernelGGL((export_scalar_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, src, dst, total, C, HW,
                         (int)planar, reverse, sub, div);
  }
  RG_LAUNCH_CHECK("tile_export_u8");
  return RG_OK;
}
