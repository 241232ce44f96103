// rg_fidstat.hip -- the two kernels a Frechet-distance evaluation needs besides the feature extractor (rna_gan_amd.fid,
// rna_gan_amd.metrics): the bilinear resize of an image batch to the extractor's input size and the fp64 accumulation of the
// features' first and second raw moments.  With them an evaluation moves F + F^2 doubles to the host and nothing else.
// And the one kernel of the kernel distance (rna_gan_amd.kid): fp64 sums of a polynomial kernel over 64 x 64 tiles of row pairs.
// Nothing here depends on the build's 16-bit storage type: both builds compile the same code.
#include "rg_pairtile.h"

namespace {

// ---- bilinear resize, half-pixel centres, no anti-aliasing (cv2.resize / F.interpolate(align_corners=False)) -----------------
// Source coordinates in fp64 (fp32 coordinates move results by 1.4e-5 at 256 -> 299), the weights rounded to fp32, the four-tap
// value in fp32 (the build has contraction off: every operation below is rounded on its own).
struct AxisTap { int i0, i1; float lam; };
__device__ __forceinline__ AxisTap axis_tap(int d, int in, int out) {
  double s = ((double)d + 0.5) * (double)in / (double)out - 0.5;
  s = s > 0.0 ? s : 0.0;
  int i0 = (int)floor(s);
  if (i0 > in - 1) i0 = in - 1;
  AxisTap t;
  t.i0 = i0;
  t.i1 = i0 + 1 < in ? i0 + 1 : in - 1;
  t.lam = (float)(s - (double)i0);
  return t;
}

template <typename S> __device__ __forceinline__ float tap_value(const S* p, float mul, float add);
template <> __device__ __forceinline__ float tap_value<uint8_t>(const uint8_t* p, float, float) { return (float)p[0] / 255.0f; }
template <> __device__ __forceinline__ float tap_value<float>(const float* p, float mul, float add) { return p[0] * mul + add; }

// one thread per output pixel (n, oy, ox), ox fastest: the coordinates are shared by the C channels; the writes of a wave are
// contiguous in each output plane.  The clamp lets a NaN through (comparisons, not fmaxf): a tap read outside the image shows.
template <typename S>
__global__ __launch_bounds__(256) void resize_bilinear01_kernel(const S* __restrict__ src, long long sn, long long sc, long long sh,
                                                                long long sw, float mul, float add, float* __restrict__ dst,
                                                                int N, int C, int H, int W, int Ho, int Wo) {
  const size_t total = (size_t)N * Ho * Wo;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t plane = (size_t)Ho * Wo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int ox = (int)(i % Wo);
    const size_t r = i / Wo;
    const int oy = (int)(r % Ho);
    const size_t n = r / Ho;
    const AxisTap ty = axis_tap(oy, H, Ho), tx = axis_tap(ox, W, Wo);
    const float omx = 1.f - tx.lam, omy = 1.f - ty.lam;
    const S* base = src + (long long)n * sn;
    const long long o00 = ty.i0 * sh + tx.i0 * sw, o01 = ty.i0 * sh + tx.i1 * sw;
    const long long o10 = ty.i1 * sh + tx.i0 * sw, o11 = ty.i1 * sh + tx.i1 * sw;
    float* d = dst + n * C * plane + (size_t)oy * Wo + ox;
    for (int c = 0; c < C; ++c) {
      const S* p = base + c * sc;
      const float t00 = tap_value<S>(p + o00, mul, add), t01 = tap_value<S>(p + o01, mul, add);
      const float t10 = tap_value<S>(p + o10, mul, add), t11 = tap_value<S>(p + o11, mul, add);
      const float top = omx * t00 + tx.lam * t01, bot = omx * t10 + tx.lam * t11;
      float v = omy * top + ty.lam * bot;
      v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
      d[c * plane] = v;
    }
  }
}

// ---- first and second raw moments of feature rows, fp64 ----------------------------------------------------------------------
// s2 is cut into MT x MT tiles; a workgroup owns one tile (ti <= tj) for the whole call: it sums x[r][i] * x[r][j] over ALL n
// rows in row order (no split over rows, no atomics: the same bits on every run), adds the sum to the tile and writes the result
// to s2[i][j] and, off the diagonal, to s2[j][i] as well.  The product of two fp32 values is exact in fp64, so an element's
// chain of additions depends on its row order alone: s2[i][j] and s2[j][i] inside a diagonal tile get the same bits although
// two threads compute them.  The diagonal workgroups also own their MT entries of s1.
//
// Plain v_fma_f64, not v_mfma_f64_16x16x4_f64: the part's fp64 matrix and vector peaks are equal (78.6 TFLOPS), so the matrix
// instruction buys no rate, and a 4 x 4 register tile per thread (16 FMAs for two 16-byte LDS reads and 8 conversions) keeps
// the vector pipe fed without its non-standard C/D lane map.
constexpr int MT = 64;            // tile edge: 16 x 16 threads, 4 x 4 results each
static_assert(MT == PAIR_ROWS, "rg_moments_update counts its column tiles with pair_tiles");
constexpr int MK = 32;            // rows of x staged per pass

__global__ __launch_bounds__(256) void moments_kernel(const float* __restrict__ x, int ldx, int n, int F, double* __restrict__ s1,
                                                      double* __restrict__ s2, int T) {
  __shared__ __attribute__((aligned(16))) float xi[MK][MT];
  __shared__ __attribute__((aligned(16))) float xj[MK][MT];
  int ti, tj;
  upper_triangle_tile((int)blockIdx.x, T, ti, tj);
  const bool diag = ti == tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = ti * MT, j0 = tj * MT;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  double sum1[4] = {0.0, 0.0, 0.0, 0.0};
  const float (*bj)[MT] = diag ? xi : xj;
  for (int r0 = 0; r0 < n; r0 += MK) {
    // stage MK rows of the two column tiles, zero past row n and past column F (adding an exact zero changes nothing); scalar
    // loads, a wave reads 64 consecutive floats of a row: any ldx >= F, no alignment needed
    for (int e = tid; e < MK * MT; e += 256) {
      const int rr = e / MT, cc = e % MT;
      const int r = r0 + rr;
      const size_t row = (size_t)r * (size_t)ldx;
      xi[rr][cc] = (r < n && i0 + cc < F) ? x[row + i0 + cc] : 0.f;
      if (!diag) xj[rr][cc] = (r < n && j0 + cc < F) ? x[row + j0 + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < MK; ++k) {
      const float4 av = *reinterpret_cast<const float4*>(&xi[k][ty * 4]);
      const float4 bv = *reinterpret_cast<const float4*>(&bj[k][tx * 4]);
      const double a[4] = {(double)av.x, (double)av.y, (double)av.z, (double)av.w};
      const double b[4] = {(double)bv.x, (double)bv.y, (double)bv.z, (double)bv.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
      if (diag && ty == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) sum1[q] += b[q];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + ty * 4 + p;
    if (i >= F) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx * 4 + q;
      if (j >= F) continue;
      const size_t at = (size_t)i * F + j;
      const double v = s2[at] + acc[p][q];
      s2[at] = v;
      if (!diag) s2[(size_t)j * F + i] = v;
    }
  }
  if (diag && ty == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx * 4 + q;
      if (j < F) s1[j] = s1[j] + sum1[q];
    }
  }
}

// ---- polynomial-kernel sums over tiles of row pairs, fp64 (the Gram sums of the kernel distance) -----------------------------
// k(a_r, b_s) = (gamma <a_r, b_s> + coef0)^degree for 64 rows of a against 64 rows of b; a workgroup owns one tile pair for the
// whole call and writes ONE double, the sum of its up to 4096 values.  The dots are rg_pairtile.h's tile (fp32 rows, PairDot):
// its staging, its LDS layout and its arithmetic contract are stated there.
//
// On top of the dots: t = gamma * dot + coef0 as two rounded operations (the build has contraction off; __dmul_rn / __dadd_rn
// say so in the code); v = t, t t, (t t) t.  A zero-padded row has dot 0 but k(0, y) = coef0^degree is not zero, so the VALUES
// of rows past na / nb are masked out of the sum.
//
// Order of the tile's sum: fixed, and invariant under transposing the tile -- a thread adds v[p][p] in order and then the pairs
// (v[p][q] + v[q][p]), p < q; thread (ty, tx) then pairs its partial with thread (tx, ty)'s; the 136 pair sums are added by a
// fixed tree.  Addition commutes bit for bit, so the tile (tj, ti) of a two-operand call on (a, a) gives the bits of tile
// (ti, tj): the symmetric form (each off-diagonal pair computed once, stored twice) returns exactly what the general form does.
__device__ __forceinline__ double polyk(double dot, double gamma, double coef0, int degree) {
  const double t = __dadd_rn(__dmul_rn(gamma, dot), coef0);
  if (degree == 1) return t;
  const double t2 = __dmul_rn(t, t);
  return degree == 2 ? t2 : __dmul_rn(t2, t);
}

__global__ __launch_bounds__(256) void polykernel_tile_sums_kernel(const float* __restrict__ a, int lda, int na,
                                                                   const float* __restrict__ b, int ldb, int nb, int F, double gamma,
                                                                   double coef0, int degree, double* __restrict__ sums,
                                                                   double* __restrict__ diag, int Ta, int Tb, int symmetric) {
  __shared__ __attribute__((aligned(16))) float sa[PAIR_ROWS * PairStage<float>::PITCH];
  __shared__ __attribute__((aligned(16))) float sb[PAIR_ROWS * PairStage<float>::PITCH];
  __shared__ double part[16][17];
  __shared__ double red[256];
  int ti, tj;
  if (symmetric) {
    upper_triangle_tile((int)blockIdx.x, Ta, ti, tj);
  } else {
    ti = (int)(blockIdx.x / (unsigned)Tb);
    tj = (int)(blockIdx.x % (unsigned)Tb);
  }
  const bool same = symmetric && ti == tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long long i0 = (long long)ti * PAIR_ROWS, j0 = (long long)tj * PAIR_ROWS;
  double acc[4][4];
  pair_tile_accumulate<float, PairDot>(a, lda, PairRowsFrom{i0, na}, b, ldb, PairRowsFrom{j0, nb}, F, same, sa, sb, acc);
  // the kernel values, rows past the end masked to an exact zero
  double v[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = i0 + ty + 16 * p < na && j0 + tx + 16 * q < nb;
      v[p][q] = in ? polyk(acc[p][q], gamma, coef0, degree) : 0.0;
    }
  double s = ((v[0][0] + v[1][1]) + v[2][2]) + v[3][3];
  const double dsum = s;                                    // thread (t, t) of a diagonal tile: k(a_r, a_r) of its 4 rows
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = p + 1; q < 4; ++q) s += v[p][q] + v[q][p];
  part[ty][tx] = s;
  __syncthreads();
  red[tid] = ty == tx ? part[ty][ty] : (ty < tx ? part[ty][tx] + part[tx][ty] : 0.0);
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double total = red[0];
    sums[(size_t)ti * (size_t)Tb + (size_t)tj] = total;
    if (symmetric && !same) sums[(size_t)tj * (size_t)Tb + (size_t)ti] = total;
  }
  if (same) {                                               // block-uniform
    if (ty == tx) part[0][tx] = dsum;
    __syncthreads();
    if (tid == 0) {
      double d = 0.0;
      for (int t = 0; t < 16; ++t) d += part[0][t];
      diag[ti] = d;
    }
  }
}

}  // namespace

extern "C" int rg_resize_bilinear01(const void* src, int src_dtype, int64_t sn, int64_t sc, int64_t sh, int64_t sw, float mul,
                                    float add, float* dst_nchw, int N, int C, int H, int W, int Ho, int Wo, void* stream) {
  RG_REQUIRE(src_dtype == RG_F32 || src_dtype == RG_U8, RG_EINVAL, "resize_bilinear01: src_dtype %d is neither RG_F32 nor RG_U8",
             src_dtype);
  RG_REQUIRE(N >= 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, RG_EINVAL,
             "resize_bilinear01: bad sizes N %d C %d H %d W %d -> %d x %d", N, C, H, W, Ho, Wo);
  if (N == 0) return RG_OK;
  RG_REQUIRE(src && dst_nchw, RG_EINVAL, "resize_bilinear01: null buffer");
  const size_t total = (size_t)N * Ho * Wo;
  size_t blocks = (total + 255) / 256;
  if (blocks > 65535u * 16u) blocks = 65535u * 16u;        // the rest is the grid-stride loop
  const dim3 grid((unsigned)blocks), block(256);
  if (src_dtype == RG_U8)
    hipLaunchKernelGGL(resize_bilinear01_kernel<uint8_t>, grid, block, 0, rg_stream(stream), (const uint8_t*)src, (long long)sn,
                       (long long)sc, (long long)sh, (long long)sw, mul, add, dst_nchw, N, C, H, W, Ho, Wo);
  else
    hipLaunchKernelGGL(resize_bilinear01_kernel<float>, grid, block, 0, rg_stream(stream), (const float*)src, (long long)sn,
                       (long long)sc, (long long)sh, (long long)sw, mul, add, dst_nchw, N, C, H, W, Ho, Wo);
  RG_LAUNCH_CHECK("resize_bilinear01");
  return RG_OK;
}

extern "C" int rg_moments_update(const float* x, int ldx, int n, int F, double* s1, double* s2, void* stream) {
  RG_REQUIRE(F >= 1 && n >= 0 && ldx >= F, RG_EINVAL, "moments_update: bad sizes n %d F %d ldx %d", n, F, ldx);
  if (n == 0) return RG_OK;
  RG_REQUIRE(x && s1 && s2, RG_EINVAL, "moments_update: null buffer");
  const long long T = pair_tiles(F);
  const long long tiles = T * (T + 1) / 2;
  RG_REQUIRE(tiles <= 0x7fffffffLL, RG_EUNSUPPORTED, "moments_update: F %d needs %lld tiles", F, tiles);
  hipLaunchKernelGGL(moments_kernel, dim3((unsigned)tiles), dim3(256), 0, rg_stream(stream), x, ldx, n, F, s1, s2, (int)T);
  RG_LAUNCH_CHECK("moments_update");
  return RG_OK;
}

extern "C" int rg_polykernel_tile_sums(const float* a, int lda, int na, const float* b, int ldb, int nb, int F, double gamma,
                                       double coef0, int degree, double* sums, double* diag, void* stream) {
  const bool symmetric = b == nullptr;
  if (symmetric) { ldb = lda; nb = na; }
  RG_REQUIRE(F >= 1 && na >= 0 && nb >= 0 && lda >= F && ldb >= F, RG_EINVAL,
             "polykernel_tile_sums: bad sizes na %d nb %d F %d lda %d ldb %d", na, nb, F, lda, ldb);
  RG_REQUIRE(degree >= 1 && degree <= 3, RG_EINVAL, "polykernel_tile_sums: degree %d is not 1, 2 or 3", degree);
  RG_REQUIRE(symmetric ? diag != nullptr : diag == nullptr, RG_EINVAL,
             "polykernel_tile_sums: diag is required in the symmetric form (b == NULL) and must be NULL with two operands");
  if (na == 0 || nb == 0) return RG_OK;
  RG_REQUIRE(a && sums, RG_EINVAL, "polykernel_tile_sums: null buffer");
  const long long Ta = pair_tiles(na), Tb = pair_tiles(nb);
  const long long tiles = symmetric ? Ta * (Ta + 1) / 2 : Ta * Tb;
  RG_REQUIRE(tiles <= 0x7fffffffLL, RG_EUNSUPPORTED, "polykernel_tile_sums: %d x %d rows need %lld tiles", na, nb, tiles);
  hipLaunchKernelGGL(polykernel_tile_sums_kernel, dim3((unsigned)tiles), dim3(256), 0, rg_stream(stream), a, lda, na,
                     symmetric ? a : b, ldb, nb, F, gamma, coef0, degree, sums, diag, (int)Ta, (int)Tb, symmetric ? 1 : 0);
  RG_LAUNCH_CHECK("polykernel_tile_sums");
  return RG_OK;
}
