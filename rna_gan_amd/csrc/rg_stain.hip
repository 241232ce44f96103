// rg_stain.hip -- Macenko stain normalisation of uint8 RGB tiles on the device (rna_gan_amd.stain): the three statistics passes of the
// fit and the one pass that applies it.  Everything the device computes is an INTEGER on fixed-point tables that the host builds in
// fp64 (include/rnagan_hip.h states the contract, tests/stain_refs.py restates it); eigenvectors, percentiles and the
// pseudo-inverse are the host's, between the passes.
//
//   rg_stain_moments     count, sum od_c, sum od_c od_d over the stained pixels: 10 int64
//   rg_stain_angle_hist  the bin of each stained pixel's angle in the plane of the two leading eigenvectors, by binary search over
//                        the quantised bin directions: K + 1 uint64 (the last counts the pixels with p1 <= 0)
//   rg_stain_conc_hist   the two stain concentrations of EVERY pixel: 2 x bins uint64
//   rg_stain_apply       src -> dst bytes, one pass, in place when dst == src
//
// Launch plan: every kernel reads its pixels through the stream of rg_u8px.h (layouts, the dword path, the in-place rule are stated
// there), SN_CHUNK pixels per workgroup in the statistics kernels and SN_APPLY_CHUNK in apply; an interleaved set is one stream
// (the fit is over the set, tiles do not matter).  Tables are staged in LDS; counting is 32-bit integer LDS atomics (a chunk is far
// below 2^32 pixels), then ONE 64-bit global integer atomic per occupied bin per workgroup.  Integer adds commute: no result
// depends on the launch plan, on the batching or on the order of accumulating calls.
//
// Narrowed arithmetic (the contract's sums are exact in int64; these keep the same bits):
//   moments   |od| <= 23170, so a product fits int32 and the sum of FOUR products stays below 2^31: a lane sums a quad in int32 and
//             widens once per quad.
//   angle     |od| <= 23170 and |basis| <= 30000: p1, p2 are int32 (3 * 23170 * 30000 < 2^31); the predicate is two 32 x 32 -> 64
//             multiply-adds.
//   conc, apply  the host checks the ranges of its operands: when every factor fits int32 the kernels are instantiated on int
//             (32 x 32 -> 64 multiply-adds), else on long long.
// No 16-bit type is involved: both builds behave identically.
#include "rg_u8px.h"

namespace {

constexpr int SN_CHUNK = 32768;        // pixels per workgroup of the statistics kernels (rna_gan_amd.stain.STAT_CHUNK)
constexpr int SN_APPLY_CHUNK = 8192;   // pixels per workgroup of the apply kernel (rna_gan_amd.stain.APPLY_CHUNK)
constexpr int SN_KMAX = 2048;          // angle bins
constexpr int SN_BINSMAX = 4096;       // concentration bins per stain
constexpr int SN_LMAX = 8192;          // entries of the output table
constexpr long long SN_MAXPIX = 1LL << 33;

__device__ __forceinline__ long long sn_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ pass 1: moments
struct sn_moments_f {
  const int* lut;
  int beta;
  int q[10];
  long long acc[10];
  __device__ __forceinline__ void px(int R, int G, int B) {
    const int a = lut[R], b = lut[G], c = lut[B];
    if (a >= beta && b >= beta && c >= beta) {
      q[0] += 1; q[1] += a; q[2] += b; q[3] += c;
      q[4] += a * a; q[5] += a * b; q[6] += a * c; q[7] += b * b; q[8] += b * c; q[9] += c * c;
    }
  }
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int i = 0; i < 10; ++i) { acc[i] += (long long)q[i]; q[i] = 0; }
  }
};

__global__ __launch_bounds__(256) void sn_moments_kernel(const uint8_t* __restrict__ tiles, const int32_t* __restrict__ od_lut,
                                                         int beta_q, unsigned long long* __restrict__ out, u8px_geom g) {
  __shared__ int lut[256];
  __shared__ long long red[4][10];
  const int tid = threadIdx.x;
  lut[tid] = od_lut[tid];
  __syncthreads();
  sn_moments_f f;
  f.lut = lut; f.beta = beta_q;
#pragma unroll
  for (int i = 0; i < 10; ++i) { f.q[i] = 0; f.acc[i] = 0; }
  u8px_each(tiles, g, f);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const long long v = sn_wave_sum(f.acc[i]);
    if ((tid & 63) == 0) red[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < 10) {
    const long long v = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (v) atomicAdd(&out[tid], (unsigned long long)v);           // two's complement: the sums of od_c may be negative
  }
}

// ------------------------------------------------------------------------------------------------ pass 2: angle histogram
struct sn_basis { int e[6]; };

struct sn_angle_f {
  const int* lut;
  const int2* dirs;     // dirs[k], k = 1 .. K - 1
  unsigned* h;
  sn_basis b;
  int beta, K;
  __device__ __forceinline__ void px(int R, int G, int B) {
    const int a = lut[R], bb = lut[G], c = lut[B];
    if (!(a >= beta && bb >= beta && c >= beta)) return;
    const int p1 = a * b.e[0] + bb * b.e[1] + c * b.e[2];
    const int p2 = a * b.e[3] + bb * b.e[4] + c * b.e[5];
    if (p1 <= 0) {
      atomicAdd(&h[K], 1u);
      return;
    }
    int lo = 0, hi = K - 1;                     // the largest k in 0 .. K - 1 whose predicate holds (k = 0: always)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      const int2 d = dirs[mid];
      const bool on = (long long)d.x * p2 - (long long)d.y * p1 >= 0;
      lo = on ? mid : lo;
      hi = on ? hi : mid - 1;
    }
    atomicAdd(&h[lo], 1u);
  }
  __device__ __forceinline__ void flush() {}
};

__global__ __launch_bounds__(256) void sn_angle_kernel(const uint8_t* __restrict__ tiles, const int32_t* __restrict__ od_lut, int beta_q,
                                                       sn_basis basis, const int32_t* __restrict__ dirs, int K,
                                                       unsigned long long* __restrict__ hist, u8px_geom g) {
  __shared__ int lut[256];
  __shared__ int2 d[SN_KMAX];
  __shared__ unsigned h[SN_KMAX + 1];
  const int tid = threadIdx.x;
  lut[tid] = od_lut[tid];
  for (int k = 1 + tid; k < K; k += 256) d[k] = make_int2(dirs[2 * (k - 1)], dirs[2 * (k - 1) + 1]);
  for (int i = tid; i <= K; i += 256) h[i] = 0u;
  __syncthreads();
  sn_angle_f f;
  f.lut = lut; f.dirs = d; f.h = h; f.b = basis; f.beta = beta_q; f.K = K;
  u8px_each(tiles, g, f);
  __syncthreads();
  for (int i = tid; i <= K; i += 256) {
    const unsigned v = h[i];
    if (v) atomicAdd(&hist[i], (unsigned long long)v);
  }
}

// ------------------------------------------------------------------------------------------------ pass 3: concentration histogram
template <typename T> struct sn_pinv { T p[6]; };            // [stain][channel]

template <typename T>
__device__ __forceinline__ long long sn_conc(const sn_pinv<T>& P, int s, int a, int b, int c, int qp) {
  return ((long long)P.p[3 * s] * a + (long long)P.p[3 * s + 1] * b + (long long)P.p[3 * s + 2] * c) >> qp;
}

template <typename T>
struct sn_conc_f {
  const int* lut;
  unsigned* h;
  sn_pinv<T> P;
  int qp, csh, bins;
  __device__ __forceinline__ void px(int R, int G, int B) {
    const int a = lut[R], b = lut[G], c = lut[B];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      long long v = sn_conc(P, s, a, b, c, qp) >> csh;
      v = v < 0 ? 0 : (v > (long long)(bins - 1) ? (long long)(bins - 1) : v);
      atomicAdd(&h[s * bins + (int)v], 1u);
    }
  }
  __device__ __forceinline__ void flush() {}
};

template <typename T>
__global__ __launch_bounds__(256) void sn_conc_kernel(const uint8_t* __restrict__ tiles, const int32_t* __restrict__ od_lut,
                                                      sn_pinv<T> P, int qp, int csh, int bins, unsigned long long* __restrict__ hist,
                                                      u8px_geom g) {
  __shared__ int lut[256];
  __shared__ unsigned h[2 * SN_BINSMAX];
  const int tid = threadIdx.x;
  lut[tid] = od_lut[tid];
  for (int i = tid; i < 2 * bins; i += 256) h[i] = 0u;
  __syncthreads();
  sn_conc_f<T> f;
  f.lut = lut; f.h = h; f.P = P; f.qp = qp; f.csh = csh; f.bins = bins;
  u8px_each(tiles, g, f);
  __syncthreads();
  for (int i = tid; i < 2 * bins; i += 256) {
    const unsigned v = h[i];
    if (v) atomicAdd(&hist[i], (unsigned long long)v);
  }
}

// ------------------------------------------------------------------------------------------------ pass 4: apply
template <typename T>
struct sn_apply_par {
  sn_pinv<T> P;
  T scale[2];
  T href[6];           // [channel][stain]
  long long rnd;
  int qp, qs, shift, L, off;
};

// px: the normalised bytes of one pixel, in place of its R, G, B
template <typename T>
struct sn_apply_f {
  const int* lut;
  const uint8_t* olut;
  const sn_apply_par<T>& a;
  __device__ __forceinline__ void px(int& R, int& G, int& B) {
    const int oR = lut[R], oG = lut[G], oB = lut[B];
    long long k[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const long long conc = sn_conc(a.P, s, oR, oG, oB, a.qp);
      // T = int: the host has checked that conc and conc2 fit int32, so the casts below drop nothing
      k[s] = ((long long)(T)conc * (long long)a.scale[s]) >> a.qs;
    }
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      long long v = ((long long)a.href[2 * c] * (long long)(T)k[0] + (long long)a.href[2 * c + 1] * (long long)(T)k[1] + a.rnd) >> a.shift;
      v += a.off;
      v = v < 0 ? 0 : (v > (long long)(a.L - 1) ? (long long)(a.L - 1) : v);
      o[c] = olut[(int)v];
    }
    R = o[0]; G = o[1]; B = o[2];
  }
  __device__ __forceinline__ void flush() {}
};

// src and dst are NOT restrict: dst == src is the in-place call.  A lane reads all the bytes of its pixels before it writes any of
// them, and no other lane touches those bytes (u8px_map, rg_u8px.h).
template <typename T>
__global__ __launch_bounds__(256) void sn_apply_kernel(const uint8_t* src, uint8_t* dst, const int32_t* __restrict__ od_lut,
                                                       const uint8_t* __restrict__ out_lut, sn_apply_par<T> a, u8px_geom g) {
  __shared__ int lut[256];
  __shared__ uint8_t olut[SN_LMAX];
  const int tid = threadIdx.x;
  lut[tid] = od_lut[tid];
  for (int i = tid; i < a.L; i += 256) olut[i] = out_lut[i];
  __syncthreads();
  sn_apply_f<T> f = {lut, olut, a};
  u8px_map(src, dst, g, f);
}

// ------------------------------------------------------------------------------------------------ host side
// what the four entry points share: the two buffers every pass reads, the launch geometry, the limit of a call.  *blocks = 0 for
// N == 0.  accumulate == 0: the output is zeroed by u8px_zero in front of the counting kernel.
int sn_plan(const char* what, const void* tiles, int N, int H, int W, int flags, const void* od_lut, int chunk, bool aligned,
            u8px_geom* g, unsigned* blocks) {
  RG_REQUIRE(tiles && od_lut, RG_EINVAL, "%s: NULL buffer", what);
  const long long HW = (long long)H * W;                     // a bad shape is u8px_plan's to refuse
  RG_REQUIRE(N < 0 || H <= 0 || W <= 0 || (HW <= SN_MAXPIX && (N == 0 || (long long)N <= SN_MAXPIX / HW)), RG_EUNSUPPORTED,
             "%s: N %d H %d W %d is more than 2^33 pixels per call", what, N, H, W);
  const int rc = u8px_plan(what, N, H, W, flags, chunk, aligned, false, g, blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(((uintptr_t)od_lut & 3) == 0, RG_EINVAL, "%s: od_lut needs 4-byte alignment", what);
  return RG_OK;
}

bool sn_fits_int(long long v) { return v >= -0x7fffffffLL && v <= 0x7fffffffLL; }

constexpr long long SN_ODMAX = 23170;                        // the contract's bound on |od_lut[v]|
constexpr long long SN_PMAX = 1LL << 40;                      // on |pinv6[i]|: 3 * 2^40 * 23170 < 2^57

}  // namespace

extern "C" int rg_stain_moments(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, int beta_q, int64_t* out,
                                int accumulate, void* stream) {
  u8px_geom g;
  unsigned blocks;
  RG_REQUIRE(out, RG_EINVAL, "stain_moments: NULL buffer");
  int rc = sn_plan("stain_moments", tiles, N, H, W, flags, od_lut, SN_CHUNK, ((uintptr_t)tiles & 3) == 0, &g, &blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(((uintptr_t)out & 7) == 0, RG_EINVAL, "stain_moments: out needs 8-byte alignment");
  if (N == 0) return RG_OK;
  hipStream_t st = rg_stream(stream);
  if (!accumulate && (rc = u8px_zero("stain_moments", out, 2 * 10, st)) != RG_OK) return rc;
  hipLaunchKernelGGL(sn_moments_kernel, dim3(blocks), dim3(256), 0, st, tiles, od_lut, beta_q, (unsigned long long*)out, g);
  RG_LAUNCH_CHECK("stain_moments");
  return RG_OK;
}

extern "C" int rg_stain_angle_hist(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, int beta_q,
                                   const int* basis6, const int32_t* dirs, int K, uint64_t* hist, int accumulate, void* stream) {
  u8px_geom g;
  unsigned blocks;
  RG_REQUIRE(basis6 && dirs && hist, RG_EINVAL, "stain_angle_hist: NULL buffer");
  int rc = sn_plan("stain_angle_hist", tiles, N, H, W, flags, od_lut, SN_CHUNK, ((uintptr_t)tiles & 3) == 0, &g, &blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(K >= 2 && K <= SN_KMAX, RG_EINVAL, "stain_angle_hist: K %d is not in 2..%d", K, SN_KMAX);
  RG_REQUIRE(((uintptr_t)dirs & 3) == 0 && ((uintptr_t)hist & 7) == 0, RG_EINVAL,
             "stain_angle_hist: dirs needs 4-byte and hist 8-byte alignment");
  sn_basis b;
  for (int i = 0; i < 6; ++i) {
    RG_REQUIRE(basis6[i] >= -30000 && basis6[i] <= 30000, RG_EINVAL, "stain_angle_hist: basis6[%d] = %d is outside +-30000", i, basis6[i]);
    b.e[i] = basis6[i];
  }
  if (N == 0) return RG_OK;
  hipStream_t st = rg_stream(stream);
  if (!accumulate && (rc = u8px_zero("stain_angle_hist", hist, 2 * (size_t)(K + 1), st)) != RG_OK) return rc;
  hipLaunchKernelGGL(sn_angle_kernel, dim3(blocks), dim3(256), 0, st, tiles, od_lut, beta_q, b, dirs, K, (unsigned long long*)hist, g);
  RG_LAUNCH_CHECK("stain_angle_hist");
  return RG_OK;
}

extern "C" int rg_stain_conc_hist(const uint8_t* tiles, int N, int H, int W, int flags, const int32_t* od_lut, const long long* pinv6,
                                  int qp, int csh, int bins, uint64_t* hist, int accumulate, void* stream) {
  u8px_geom g;
  unsigned blocks;
  RG_REQUIRE(pinv6 && hist, RG_EINVAL, "stain_conc_hist: NULL buffer");
  int rc = sn_plan("stain_conc_hist", tiles, N, H, W, flags, od_lut, SN_CHUNK, ((uintptr_t)tiles & 3) == 0, &g, &blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(bins >= 1 && bins <= SN_BINSMAX, RG_EINVAL, "stain_conc_hist: bins %d is not in 1..%d", bins, SN_BINSMAX);
  RG_REQUIRE(qp >= 0 && qp <= 40 && csh >= 0 && csh <= 31, RG_EINVAL, "stain_conc_hist: qp %d is not in 0..40 or csh %d not in 0..31", qp, csh);
  RG_REQUIRE(((uintptr_t)hist & 7) == 0, RG_EINVAL, "stain_conc_hist: hist needs 8-byte alignment");
  bool narrow = true;
  for (int i = 0; i < 6; ++i) {
    RG_REQUIRE(pinv6[i] >= -SN_PMAX && pinv6[i] <= SN_PMAX, RG_EINVAL, "stain_conc_hist: pinv6[%d] = %lld is outside +-2^40", i, pinv6[i]);
    narrow = narrow && sn_fits_int(pinv6[i]);
  }
  if (N == 0) return RG_OK;
  hipStream_t st = rg_stream(stream);
  if (!accumulate && (rc = u8px_zero("stain_conc_hist", hist, 2 * (size_t)(2 * bins), st)) != RG_OK) return rc;
  if (narrow) {
    sn_pinv<int> P;
    for (int i = 0; i < 6; ++i) P.p[i] = (int)pinv6[i];
    hipLaunchKernelGGL(sn_conc_kernel<int>, dim3(blocks), dim3(256), 0, st, tiles, od_lut, P, qp, csh, bins, (unsigned long long*)hist, g);
  } else {
    sn_pinv<long long> P;
    for (int i = 0; i < 6; ++i) P.p[i] = pinv6[i];
    hipLaunchKernelGGL(sn_conc_kernel<long long>, dim3(blocks), dim3(256), 0, st, tiles, od_lut, P, qp, csh, bins,
                       (unsigned long long*)hist, g);
  }
  RG_LAUNCH_CHECK("stain_conc_hist");
  return RG_OK;
}

extern "C" int rg_stain_apply(const uint8_t* src, uint8_t* dst, int N, int H, int W, int flags, const int32_t* od_lut,
                              const long long* pinv6, int qp, const long long* scale2, int qs, const int* href6, int shift,
                              const uint8_t* out_lut, int L, int off, void* stream) {
  u8px_geom g;
  unsigned blocks;
  RG_REQUIRE(dst && pinv6 && scale2 && href6 && out_lut, RG_EINVAL, "stain_apply: NULL buffer");
  int rc = sn_plan("stain_apply", src, N, H, W, flags, od_lut, SN_APPLY_CHUNK, (((uintptr_t)src | (uintptr_t)dst) & 3) == 0, &g, &blocks);
  if (rc != RG_OK) return rc;
  RG_REQUIRE(L >= 1 && L <= SN_LMAX, RG_EINVAL, "stain_apply: L %d is not in 1..%d", L, SN_LMAX);
  RG_REQUIRE(off >= 0 && off < L, RG_EINVAL, "stain_apply: off %d is not in [0, L = %d)", off, L);
  RG_REQUIRE(qp >= 0 && qp <= 40 && qs >= 0 && qs <= 40 && shift >= 0 && shift <= 40, RG_EINVAL,
             "stain_apply: qp %d, qs %d or shift %d is not in 0..40", qp, qs, shift);
  // the ranges in which every sum of the contract is exact in int64, and those in which every factor fits int32
  long long pmax = 0, hmax = 0, smax = 0;
  for (int i = 0; i < 6; ++i) {
    RG_REQUIRE(pinv6[i] >= -SN_PMAX && pinv6[i] <= SN_PMAX, RG_EINVAL, "stain_apply: pinv6[%d] = %lld is outside +-2^40", i, pinv6[i]);
    const long long p = pinv6[i] < 0 ? -pinv6[i] : pinv6[i], h = href6[i] < 0 ? -(long long)href6[i] : (long long)href6[i];
    pmax = p > pmax ? p : pmax;
    hmax = h > hmax ? h : hmax;
  }
  for (int s = 0; s < 2; ++s) {
    RG_REQUIRE(scale2[s] >= 0, RG_EINVAL, "stain_apply: scale2[%d] = %lld is negative", s, scale2[s]);
    smax = scale2[s] > smax ? scale2[s] : smax;
  }
  const long long cmax = ((3 * pmax * SN_ODMAX) >> qp) + 1;                       // |conc|
  RG_REQUIRE(smax == 0 || cmax <= (1LL << 61) / smax, RG_EINVAL, "stain_apply: pinv6 and scale2 leave int64 (|conc| up to %lld)", cmax);
  const long long kmax = ((cmax * smax) >> qs) + 1;                                // |conc2|
  RG_REQUIRE(hmax == 0 || kmax <= (1LL << 60) / hmax, RG_EINVAL, "stain_apply: scale2 and href6 leave int64 (|conc2| up to %lld)", kmax);
  const size_t bytes = (size_t)3 * (size_t)H * (size_t)W * (size_t)N;
  RG_REQUIRE(dst == src || (uintptr_t)dst >= (uintptr_t)src + bytes || (uintptr_t)src >= (uintptr_t)dst + bytes, RG_EINVAL,
             "stain_apply: dst overlaps src without being src");
  if (N == 0) return RG_OK;
  const bool narrow = sn_fits_int(pmax) && sn_fits_int(cmax) && sn_fits_int(smax) && sn_fits_int(kmax);
  const long long rnd = shift > 0 ? 1LL << (shift - 1) : 0;
  hipStream_t st = rg_stream(stream);
  if (narrow) {
    sn_apply_par<int> a;
    for (int i = 0; i < 6; ++i) { a.P.p[i] = (int)pinv6[i]; a.href[i] = href6[i]; }
    a.scale[0] = (int)scale2[0]; a.scale[1] = (int)scale2[1];
    a.rnd = rnd; a.qp = qp; a.qs = qs; a.shift = shift; a.L = L; a.off = off;
    hipLaunchKernelGGL(sn_apply_kernel<int>, dim3(blocks), dim3(256), 0, st, src, dst, od_lut, out_lut, a, g);
  } else {
    sn_apply_par<long long> a;
    for (int i = 0; i < 6; ++i) { a.P.p[i] = pinv6[i]; a.href[i] = href6[i]; }
    a.scale[0] = scale2[0]; a.scale[1] = scale2[1];
    a.rnd = rnd; a.qp = qp; a.qs = qs; a.shift = shift; a.L = L; a.off = off;
    hipLaunchKernelGGL(sn_apply_kernel<long long>, dim3(blocks), dim3(256), 0, st, src, dst, od_lut, out_lut, a, g);
  }
  RG_LAUNCH_CHECK("stain_apply");
  return RG_OK;
}
