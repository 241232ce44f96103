// rg_plainact.hip -- what a BatchNorm-free critic layer needs behind its conv (DCGANDiscriminator(batchnorm=False),
// rna_gan_amd.engine.PlainDiscNet):
//   * the two kernels that FINISH a split-K conv launch's slabs (rg_conv_down_partial / rg_conv_up_partial) -- without
//     BatchNorm nothing else consumes them:
//       rg_slab_bias_act   a[m][c]   = lrelu(sum_s slab[s][m][c] + bias[c])                      (forward)
//       rg_slab_mask       out[m][c] = (sum_s slab[s][m][c]) * lrelu'(mask[m][c])                (tangent forward, data gradient)
//                          + per-workgroup column sums of `out` [rows][C] (the consumer layer's bias gradient), finished in a
//                          fixed order by rg_parts_col_sum;
//   * the unsplit MFMA stride-2 conv with the bias + LeakyReLU (affine epilogue, scale = 1) or the mask in its epilogue
//     (rg_conv_down_epi);
//   * the elementwise bias + LeakyReLU pass of the paths without a fused form (fp32 storage, generic kernels): rg_bias_act;
//   * rg_vec_sum: the head's bias gradient sum_n gh[n].
// The finishing kernels are streaming kernels: every slab element is read once with 16-byte loads, the result written once with
// 16-byte stores, sums in the fixed order s = 0, 1, ...; no LDS staging of data (LDS only carries the 8 column sums per thread
// across the rows of a workgroup), a grid sized by the row count, no hand-off between workgroups.
#include "rg_common.h"
#include "rg_internal.h"

namespace {

constexpr int PA_ROWS_PT = 8;      // rows per thread of a finishing kernel

__device__ __forceinline__ float pa_lmask(uint32_t abits, float slope) {
  return (abits & 0x8000u) || !(abits & 0x7fffu) ? slope : 1.f;      // a <= 0 (incl. -0): slope
}

// 8 consecutive elements of slab s (fp32 or the build's 16-bit type) added to v
template <bool S16>
__device__ __forceinline__ void pa_add8(const void* slab, size_t idx, float* v) {
  float t[8];
  if (S16) Vec<h16_t, 8>::ld(reinterpret_cast<const h16_t*>(slab) + idx, t);
  else Vec<float, 8>::ld(reinterpret_cast<const float*>(slab) + idx, t);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] += t[e];
}

// Thread layout of both finishing kernels: CGB = min(C / 8, 256) column groups of 8 per workgroup (blockIdx.y covers C / 8 > 256),
// RB = 256 / CGB rows per pass, PA_ROWS_PT passes: a workgroup owns RB * PA_ROWS_PT consecutive rows.
// MASK = false: bias + LeakyReLU.  MASK = true: the LeakyReLU mask, and (parts != nullptr) the column sums of the STORED values.
template <bool S16, bool MASK>
__global__ __launch_bounds__(256) void slab_finish_kernel(const void* __restrict__ slab, int nsplit, size_t stride,
                                                          const float* __restrict__ bias, const uint16_t* __restrict__ mask,
                                                          float slope, uint16_t* __restrict__ out, float* __restrict__ parts,
                                                          long long M, int C, int cgb) {
  __shared__ float red[256 * 8];
  const int t = threadIdx.x;
  const int cg = t % cgb, rl = t / cgb, rb = 256 / cgb;
  const int col = (blockIdx.y * cgb + cg) * 8;
  const long long row0 = (long long)blockIdx.x * rb * PA_ROWS_PT;
  float b[8], cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { b[e] = 0.f; cs[e] = 0.f; }
  if (!MASK) {                          // (scalar loads: a bias is a slice of the flat parameter buffer, 4-byte aligned only)
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = bias[col + e];
  }
#pragma unroll 2
  for (int p = 0; p < PA_ROWS_PT; ++p) {
    const long long m = row0 + (long long)p * rb + rl;
    if (m >= M) break;
    const size_t idx = (size_t)m * C + col;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    for (int s = 0; s < nsplit; ++s) pa_add8<S16>(slab, (size_t)s * stride + idx, v);
    if (MASK) {
      const uint4 a = *reinterpret_cast<const uint4*>(mask + idx);
      const uint32_t ab[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[2 * e] *= pa_lmask(ab[e], slope); v[2 * e + 1] *= pa_lmask(ab[e] >> 16, slope); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = lrelu_f(v[e] + b[e], slope);
    }
    Vec<h16_t, 8>::st(reinterpret_cast<h16_t*>(out) + idx, v);
    if (MASK) {
#pragma unroll
      for (int e = 0; e < 8; ++e) cs[e] += Elem<h16_t>::round(v[e]);
    }
  }
  if (MASK && parts != nullptr) {       // (wave-uniform: a kernel argument)
#pragma unroll
    for (int e = 0; e < 8; ++e) red[t * 8 + e] = cs[e];
    __syncthreads();
    if (rl == 0) {
      float s[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] = 0.f;
      for (int r = 0; r < rb; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += red[(r * cgb + cg) * 8 + e];
      float* po = parts + (size_t)blockIdx.x * C + col;
      Vec<float, 4>::st(po, s);
      Vec<float, 4>::st(po + 4, s + 4);
    }
  }
}

// out[c] (+)= sum_r parts[r][c], r = 0, 1, ... (fixed order)
__global__ __launch_bounds__(256) void parts_col_sum_kernel(const float* __restrict__ parts, int rows, int C, float* out,
                                                            int accumulate) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += parts[(size_t)r * C + c];
  out[c] = accumulate ? out[c] + s : s;
}

// y[m][c] = lrelu(z[m][c] + bias[c]) (y may be z), 8 elements per thread
template <typename T>
__global__ __launch_bounds__(256) void bias_act_kernel(const T* __restrict__ z, const float* __restrict__ bias, T* __restrict__ y,
                                                       size_t n8, int C, float slope) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
    const int col = (int)((i * 8) % (size_t)C);
    float v[8], b[8];
    Vec<T, 8>::ld(z + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = bias[col + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = lrelu_f(v[e] + b[e], slope);
    Vec<T, 8>::st(y + i * 8, v);
  }
}

// out[0] (+)= sum_i x[i] in a fixed order (one workgroup: n is a batch size)
__global__ __launch_bounds__(256) void vec_sum_kernel(const float* __restrict__ x, int n, float* out, int accumulate) {
  __shared__ float sm[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += x[i];
  const float t = block_sum_256(s, sm);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + t : t;
}

bool pa_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// column groups per workgroup, or 0 when the finishing kernels' thread layout does not cover this width
int pa_cgb(int C) {
  if (C <= 0 || C % 8) return 0;
  const int g = C / 8;
  if (g >= 256) return g % 256 == 0 ? 256 : 0;
  return 256 % g == 0 ? g : 0;
}

}  // namespace

extern "C" int rg_slab_finish_rows(long long M, int C) {
  const int cgb = pa_cgb(C);
  if (M <= 0 || !cgb) return 0;
  const long long rpb = (long long)(256 / cgb) * PA_ROWS_PT;
  const long long rows = (M + rpb - 1) / rpb;
  return rows > 0x7fffffffll ? 0 : (int)rows;
}

static int slab_finish(const char* name, bool mask_mode, const void* slab, int nsplit, size_t stride, int slab_dtype,
                       const float* bias, const void* mask, float slope, void* out, float* parts, long long M, int C,
                       hipStream_t st) {
  RG_REQUIRE(slab && out && nsplit >= 1 && M > 0 && (slab_dtype == RG_F32 || slab_dtype == RG_H16), RG_EINVAL, "%s: bad args", name);
  const int rows = rg_slab_finish_rows(M, C);
  RG_REQUIRE(rows > 0, RG_EUNSUPPORTED, "%s: channel count %d not covered (rg_slab_finish_rows)", name, C);
  RG_REQUIRE(stride >= (size_t)M * C && stride % 8 == 0, RG_EINVAL, "%s: slab stride smaller than a slab / not a multiple of 8", name);
  RG_REQUIRE(pa_aligned16(slab) && pa_aligned16(out) && pa_aligned16(mask) && pa_aligned16(parts), RG_EINVAL,
             "%s: 16-byte aligned buffers required", name);
  const int cgb = pa_cgb(C);
  const dim3 grid((unsigned)rows, (unsigned)(C / 8 / cgb));
  const uint16_t* mk = (const uint16_t*)mask;
  uint16_t* o = (uint16_t*)out;
  if (mask_mode) {
    if (slab_dtype == RG_F32)
      hipLaunchKernelGGL((slab_finish_kernel<false, true>), grid, dim3(256), 0, st, slab, nsplit, stride, bias, mk, slope, o, parts, M, C, cgb);
    else
      hipLaunchKernelGGL((slab_finish_kernel<true, true>), grid, dim3(256), 0, st, slab, nsplit, stride, bias, mk, slope, o, parts, M, C, cgb);
  } else {
    if (slab_dtype == RG_F32)
      hipLaunchKernelGGL((slab_finish_kernel<false, false>), grid, dim3(256), 0, st, slab, nsplit, stride, bias, mk, slope, o, parts, M, C, cgb);
    else
      hipLaunchKernelGGL((slab_finish_kernel<true, false>), grid, dim3(256), 0, st, slab, nsplit, stride, bias, mk, slope, o, parts, M, C, cgb);
  }
  RG_LAUNCH_CHECK(name);
  return RG_OK;
}

extern "C" int rg_slab_bias_act(const void* slab, int nsplit, size_t stride, int slab_dtype, const float* bias, void* y,
                                long long M, int C, float slope, void* stream) {
  RG_REQUIRE(bias, RG_EINVAL, "slab_bias_act: bias is NULL");
  return slab_finish("slab_bias_act", false, slab, nsplit, stride, slab_dtype, bias, nullptr, slope, y, nullptr, M, C,
                     rg_stream(stream));
}

extern "C" int rg_slab_mask(const void* slab, int nsplit, size_t stride, int slab_dtype, const void* mask_act, float mask_slope,
                            void* y, float* col_parts, long long M, int C, void* stream) {
  RG_REQUIRE(mask_act, RG_EINVAL, "slab_mask: mask is NULL");
  return slab_finish("slab_mask", true, slab, nsplit, stride, slab_dtype, nullptr, mask_act, mask_slope, y, col_parts, M, C,
                     rg_stream(stream));
}

extern "C" int rg_parts_col_sum(const float* parts, int rows, int C, float* out, int accumulate, void* stream) {
  RG_REQUIRE(parts && out && rows > 0 && C > 0, RG_EINVAL, "parts_col_sum: bad args");
  hipLaunchKernelGGL(parts_col_sum_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, rg_stream(stream), parts, rows, C, out,
                     accumulate);
  RG_LAUNCH_CHECK("parts_col_sum");
  return RG_OK;
}

extern "C" int rg_bias_act(const void* z, const float* bias, void* y, long long M, int C, float slope, int dtype, void* stream) {
  RG_REQUIRE(z && bias && y && M > 0 && C > 0 && C % 8 == 0 && (dtype == RG_F32 || dtype == RG_H16), RG_EINVAL,
             "bias_act: bad args (C must be a multiple of 8)");
  RG_REQUIRE(pa_aligned16(z) && pa_aligned16(y), RG_EINVAL, "bias_act: 16-byte aligned buffers required");
  const size_t n8 = (size_t)M * C / 8;
  size_t blocks = (n8 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (dtype == RG_F32)
    hipLaunchKernelGGL((bias_act_kernel<float>), dim3((unsigned)blocks), dim3(256), 0, rg_stream(stream), (const float*)z, bias,
                       (float*)y, n8, C, slope);
  else
    hipLaunchKernelGGL((bias_act_kernel<h16_t>), dim3((unsigned)blocks), dim3(256), 0, rg_stream(stream), (const h16_t*)z, bias,
                       (h16_t*)y, n8, C, slope);
  RG_LAUNCH_CHECK("bias_act");
  return RG_OK;
}

extern "C" int rg_vec_sum(const float* x, int n, float* out, int accumulate, void* stream) {
  RG_REQUIRE(x && out && n > 0, RG_EINVAL, "vec_sum: bad args");
  hipLaunchKernelGGL(vec_sum_kernel, dim3(1), dim3(256), 0, rg_stream(stream), x, n, out, accumulate);
  RG_LAUNCH_CHECK("vec_sum");
  return RG_OK;
}

// The unsplit matrix-core stride-2 conv with an epilogue on the fp32 accumulator, rounded once:
//   shift != NULL: y = lrelu(conv(x) + shift[c], slope)       (the affine epilogue with a NULL scale = 1)
//   mask  != NULL: y = conv(x) * lrelu'(mask[m][c])           (mask: an activation of y's shape)
// Either forces the launch not to split K, so callers use it where rg_conv_split says the plain launch does not split either.
extern "C" int rg_conv_down_epi_supported(int N, int Hi, int Wi, int I, int O, int dtype, int algo) {
  if (N <= 0 || Hi <= 0 || Wi <= 0 || I <= 0 || O <= 0 || Hi % 2 || Wi % 2 || O % 8) return 0;
  if (algo == RG_ALGO_GENERIC || dtype != RG_H16) return 0;
  return rg_mfma_conv_supported(N, Hi / 2, Wi / 2, I, O) ? 1 : 0;
}

extern "C" int rg_conv_down_epi(const void* x, const void* wdn, void* y, int N, int Hi, int Wi, int I, int O, const float* shift,
                                float slope, const void* mask_act, float mask_slope, int dtype, int algo, void* ws, size_t ws_bytes,
                                void* stream) {
  RG_REQUIRE(x && wdn && y && ((shift != nullptr) != (mask_act != nullptr)), RG_EINVAL,
             "conv_down_epi: bad args (exactly one of shift / mask)");
  RG_REQUIRE(rg_conv_down_epi_supported(N, Hi, Wi, I, O, dtype, algo), RG_EUNSUPPORTED,
             "conv_down_epi: shape / dtype not supported by the MFMA kernel");
  RG_REQUIRE(pa_aligned16(shift) && pa_aligned16(mask_act) && pa_aligned16(y), RG_EINVAL, "conv_down_epi: 16-byte aligned buffers required");
  return rg_mfma_conv_down(x, wdn, y, N, Hi, Wi, I, O, nullptr, ws, ws_bytes, rg_stream(stream), 0, shift, slope,
                           mask_act, mask_slope);
}
