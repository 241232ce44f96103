// rg_knn.hip -- the two primitives of the precision / recall / density / coverage metrics (rna_gan_amd.prdc,
// rna_gan_amd.metrics.PrecisionRecall): k-th nearest-neighbour radii of a set of feature rows and membership of the rows of one
// set in the balls of another.  Both are all-pairs SQUARED distances in fp64 over 64 x 64 tiles of row pairs with a selection or
// a comparison per pair; the n x n matrix never exists in memory.
// Nothing here depends on the build's 16-bit storage type: both builds compile the same code.
#include "rg_pairtile.h"

#include <cmath>

namespace {

// ---- squared distances of a 64 x 64 tile of row pairs, fp64 -------------------------------------------------------------------
// rg_pairtile.h's tile for fp32 rows and PairDist2 -- the same staging, LDS layout and d2 contract (symmetric bit for bit,
// independent of the tiling, the pairs of rows past the end skipped by INDEX), stated there -- written out here and NOT taken from
// the template: through it the loops compile to the same instructions, but the code around them does not (the d2 stores pair up
// into ds_write2_b64, 102 VGPRs for 108), and rg_radius_hits measured 0.3 to 0.5 % slower at 2048 x 2048 x 2048
// (profiles/pair_tile_core.json).  tests/test_repr_ops_gpu.py holds this copy and the template's fp64 form to the same bits.
//
// The tile's 4096 values then go to LDS (pitch 65 doubles, over the staging buffers, which are dead by then) and one thread per
// row walks its 64 values in column order.  Everything after d2 (k smallest, count, minimum) is independent of order: the same
// bits on every run, no atomics.
constexpr int DT = PAIR_ROWS;     // rows per tile
constexpr int DK = PairStage<float>::K;          // features staged per pass
constexpr int DPITCH = PairStage<float>::PITCH;  // floats per staged row
constexpr int D2PITCH = DT + 1;   // doubles per row of the tile's d2 matrix in LDS
constexpr int KMAX = 16;          // largest k of rg_knn_radii2
constexpr size_t STAGE_BYTES = 2 * DT * DPITCH * sizeof(float);
constexpr size_t D2_BYTES = DT * D2PITCH * sizeof(double);
constexpr size_t TILE_LDS = D2_BYTES > STAGE_BYTES ? D2_BYTES : STAGE_BYTES;

// the tile's d2 values into d2[row of a][row of b]; a and b may be the same tile of one set (same != 0: staged once)
__device__ __forceinline__ void tile_dist2(const float* __restrict__ a, int lda, int na, long long i0, const float* __restrict__ b,
                                           int ldb, int nb, long long j0, int F, bool same, unsigned char* smem) {
  float (*sa)[DPITCH] = reinterpret_cast<float (*)[DPITCH]>(smem);
  float (*sb)[DPITCH] = sa + DT;
  const float (*bs)[DPITCH] = same ? sa : sb;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int k0 = 0; k0 < F; k0 += DK) {
    // scalar loads, half a wave reads 32 consecutive floats of a row (any ld >= F, no alignment needed); nothing past row
    // na / nb or feature F is read
    for (int e = tid; e < DT * DK; e += 256) {
      const int rr = e / DK, kk = e % DK;
      const bool kin = k0 + kk < F;
      const long long ra = i0 + rr, rb = j0 + rr;
      sa[rr][kk] = (kin && ra < na) ? a[(size_t)ra * (size_t)lda + (size_t)(k0 + kk)] : 0.f;
      if (!same) sb[rr][kk] = (kin && rb < nb) ? b[(size_t)rb * (size_t)ldb + (size_t)(k0 + kk)] : 0.f;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < DK; k += 4) {
      float4 av[4], bv[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) av[p] = *reinterpret_cast<const float4*>(&sa[ty + 16 * p][k]);
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[q] = *reinterpret_cast<const float4*>(&bs[tx + 16 * q][k]);
      // four features, in ascending order for every accumulator
#define RG_D2_STEP(c)                                                    \
  _Pragma("unroll") for (int p = 0; p < 4; ++p) {                        \
    const double ap = (double)av[p].c;                                   \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                      \
      const double diff = __dsub_rn(ap, (double)bv[q].c);                \
      acc[p][q] = fma(diff, diff, acc[p][q]);                            \
    }                                                                    \
  }
      RG_D2_STEP(x)
      RG_D2_STEP(y)
      RG_D2_STEP(z)
      RG_D2_STEP(w)
#undef RG_D2_STEP
    }
    __syncthreads();                                        // also: the staging buffers are dead after the last pass
  }
  double (*d2)[D2PITCH] = reinterpret_cast<double (*)[D2PITCH]>(smem);
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) d2[ty + 16 * p][tx + 16 * q] = acc[p][q];
  __syncthreads();
}

// keep the KMAX smallest values seen, ascending (best starts at +inf); a NaN never enters (the caller maps it to +inf)
__device__ __forceinline__ void keep_smallest(double (&best)[KMAX], double v) {
  if (v < best[KMAX - 1]) {
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
      const bool lt = v < best[s];
      const double lo = lt ? v : best[s], hi = lt ? best[s] : v;
      best[s] = lo;
      v = hi;
    }
  }
}

__device__ __forceinline__ double nan_to_inf(double v) { return v != v ? (double)INFINITY : v; }

// ---- k nearest neighbours: per tile pair, the k smallest d2 of every row ------------------------------------------------------
// Workgroups run over the upper triangle of tile pairs (ti <= tj).  Wave 0 handles the rows of tile ti against the columns of
// tile tj and writes part[tj][.][i]; on an off-diagonal pair wave 1 handles the rows of tile tj against the columns of tile ti
// (the transposed tile: the same bits, d2 is symmetric) and writes part[ti][.][j].  So part[t][s][i], t < T, s < k, holds the
// s-th smallest d2 of row i against the rows of tile t other than i itself (own index skipped, NOT zero distances), +inf where
// the tile has fewer.
__global__ __launch_bounds__(256) void knn_tile_kernel(const float* __restrict__ a, int lda, int n, int F, int k,
                                                       double* __restrict__ part, int T) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_LDS];
  int ti, tj;
  upper_triangle_tile((int)blockIdx.x, T, ti, tj);
  const bool same = ti == tj;
  const long long i0 = (long long)ti * DT, j0 = (long long)tj * DT;
  tile_dist2(a, lda, n, i0, a, lda, n, j0, F, same, smem);
  const double (*d2)[D2PITCH] = reinterpret_cast<const double (*)[D2PITCH]>(smem);
  const int tid = threadIdx.x;
  if (tid >= 128 || (tid >= 64 && same)) return;
  const bool transposed = tid >= 64;
  const int r = tid & 63;
  const long long row = (transposed ? j0 : i0) + r, c0 = transposed ? i0 : j0;
  if (row >= n) return;
  double best[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) best[s] = (double)INFINITY;
  for (int c = 0; c < DT; ++c) {
    const long long col = c0 + c;
    if (col >= n || col == row) continue;
    keep_smallest(best, nan_to_inf(transposed ? d2[c][r] : d2[r][c]));
  }
  double* out = part + (size_t)(transposed ? ti : tj) * (size_t)k * (size_t)n + (size_t)row;
#pragma unroll
  for (int s = 0; s < KMAX; ++s)
    if (s < k) out[(size_t)s * (size_t)n] = best[s];
}

// one thread per row: the k-th smallest of its T * k partial values part[q][i], q = t * k + s.  They are loaded MERGE_BATCH at a
// time before any is inserted: the loads of a batch are in flight together (one at a time, the chain of T * k dependent
// load-then-insert steps took 94 us at n = 2048, k = 5 -- an eighth of the tile kernel)
constexpr int MERGE_BATCH = 16;
__global__ __launch_bounds__(64) void knn_merge_kernel(const double* __restrict__ part, int n, int k, int T, double* __restrict__ r2) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double best[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) best[s] = (double)INFINITY;
  const long long total = (long long)T * k;
  for (long long q0 = 0; q0 < total; q0 += MERGE_BATCH) {
    double v[MERGE_BATCH];
#pragma unroll
    for (int u = 0; u < MERGE_BATCH; ++u) v[u] = q0 + u < total ? part[(size_t)(q0 + u) * (size_t)n + (size_t)i] : (double)INFINITY;
#pragma unroll
    for (int u = 0; u < MERGE_BATCH; ++u) keep_smallest(best, v[u]);
  }
  double kth = (double)INFINITY;
#pragma unroll
  for (int s = 0; s < KMAX; ++s)
    if (s == k - 1) kth = best[s];
  r2[i] = kth;
}

// ---- hits: per tile pair and row of a, the number of b_s with d2 <= rb2[s] and the minimum d2 ---------------------------------
// pmin[tj][i], pcnt[tj][i] over the columns of tile tj; a NaN d2 never hits (the comparison is made on the value itself, so not
// even against an infinite radius) and counts as +inf in the minimum.
__global__ __launch_bounds__(256) void hits_tile_kernel(const float* __restrict__ a, int lda, int na, const float* __restrict__ b,
                                                        int ldb, int nb, int F, const double* __restrict__ rb2,
                                                        double* __restrict__ pmin, int* __restrict__ pcnt, int Tb) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_LDS];
  const int ti = (int)(blockIdx.x / (unsigned)Tb), tj = (int)(blockIdx.x % (unsigned)Tb);
  const long long i0 = (long long)ti * DT, j0 = (long long)tj * DT;
  tile_dist2(a, lda, na, i0, b, ldb, nb, j0, F, false, smem);
  const double (*d2)[D2PITCH] = reinterpret_cast<const double (*)[D2PITCH]>(smem);
  const int r = threadIdx.x;
  if (r >= DT || i0 + r >= na) return;
  double lo = (double)INFINITY;
  int count = 0;
  for (int c = 0; c < DT; ++c) {
    const long long col = j0 + c;
    if (col >= nb) break;
    const double v = d2[r][c];
    if (rb2 != nullptr && v <= rb2[col]) ++count;
    const double w = nan_to_inf(v);
    lo = w < lo ? w : lo;
  }
  const size_t at = (size_t)tj * (size_t)na + (size_t)(i0 + r);
  pmin[at] = lo;
  if (rb2 != nullptr) pcnt[at] = count;
}

__global__ __launch_bounds__(256) void hits_merge_kernel(const double* __restrict__ pmin, const int* __restrict__ pcnt, int na, int Tb,
                                                         int* __restrict__ count, double* __restrict__ mind2) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  double lo = (double)INFINITY;
  int total = 0;
  for (int t = 0; t < Tb; ++t) {
    const size_t at = (size_t)t * (size_t)na + (size_t)i;
    const double w = pmin[at];
    lo = w < lo ? w : lo;
    if (count != nullptr) total += pcnt[at];
  }
  mind2[i] = lo;
  if (count != nullptr) count[i] = total;
}

}  // namespace

extern "C" size_t rg_pairdist_ws_bytes(int na, int nb, int k) {
  if (na < 0 || nb < 0 || k < 0 || k > KMAX) return 0;
  const size_t per_row = k > 0 ? (size_t)k * sizeof(double) : sizeof(double) + sizeof(int);
  return (size_t)pair_tiles(nb) * (size_t)na * per_row;
}

extern "C" int rg_knn_radii2(const float* a, int lda, int n, int F, int k, void* ws, size_t ws_bytes, double* r2, void* stream) {
  RG_REQUIRE(F >= 1 && n >= 0 && lda >= F, RG_EINVAL, "knn_radii2: bad sizes n %d F %d lda %d", n, F, lda);
  RG_REQUIRE(k >= 1 && k <= KMAX, RG_EINVAL, "knn_radii2: k %d is outside 1..%d", k, KMAX);
  RG_REQUIRE(n >= k + 1, RG_EINVAL, "knn_radii2: k %d needs at least %d rows, got %d", k, k + 1, n);
  RG_REQUIRE(a && ws && r2, RG_EINVAL, "knn_radii2: null buffer");
  RG_REQUIRE(((uintptr_t)ws & 7u) == 0, RG_EINVAL, "knn_radii2: the workspace must be 8-byte aligned");
  const long long T = pair_tiles(n);
  const long long tiles = T * (T + 1) / 2;
  RG_REQUIRE(tiles <= 0x7fffffffLL, RG_EUNSUPPORTED, "knn_radii2: %d rows need %lld tiles", n, tiles);
  const size_t need = rg_pairdist_ws_bytes(n, n, k);
  RG_REQUIRE(ws_bytes >= need, RG_EWORKSPACE, "knn_radii2: workspace of %zu bytes, %zu needed", ws_bytes, need);
  double* part = static_cast<double*>(ws);
  hipLaunchKernelGGL(knn_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, rg_stream(stream), a, lda, n, F, k, part, (int)T);
  RG_LAUNCH_CHECK("knn_radii2 (tiles)");
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)(((long long)n + 63) / 64)), dim3(64), 0, rg_stream(stream), part, n, k, (int)T, r2);
  RG_LAUNCH_CHECK("knn_radii2 (merge)");
  return RG_OK;
}

extern "C" int rg_radius_hits(const float* a, int lda, int na, const float* b, int ldb, int nb, int F, const double* rb2, void* ws,
                              size_t ws_bytes, int32_t* count, double* mind2, void* stream) {
  RG_REQUIRE(F >= 1 && na >= 0 && nb >= 0 && lda >= F && ldb >= F, RG_EINVAL,
             "radius_hits: bad sizes na %d nb %d F %d lda %d ldb %d", na, nb, F, lda, ldb);
  RG_REQUIRE((rb2 != nullptr) == (count != nullptr), RG_EINVAL,
             "radius_hits: count and rb2 go together (both given, or both NULL for the minimum alone)");
  if (na == 0 || nb == 0) return RG_OK;
  RG_REQUIRE(a && b && ws && mind2, RG_EINVAL, "radius_hits: null buffer");
  RG_REQUIRE(((uintptr_t)ws & 7u) == 0, RG_EINVAL, "radius_hits: the workspace must be 8-byte aligned");
  const long long Ta = pair_tiles(na), Tb = pair_tiles(nb);
  const long long tiles = Ta * Tb;
  RG_REQUIRE(tiles <= 0x7fffffffLL, RG_EUNSUPPORTED, "radius_hits: %d x %d rows need %lld tiles", na, nb, tiles);
  const size_t need = rg_pairdist_ws_bytes(na, nb, 0);
  RG_REQUIRE(ws_bytes >= need, RG_EWORKSPACE, "radius_hits: workspace of %zu bytes, %zu needed", ws_bytes, need);
  double* pmin = static_cast<double*>(ws);
  int* pcnt = reinterpret_cast<int*>(pmin + (size_t)Tb * (size_t)na);
  hipLaunchKernelGGL(hits_tile_kernel, dim3((unsigned)tiles), dim3(256), 0, rg_stream(stream), a, lda, na, b, ldb, nb, F, rb2, pmin,
                     pcnt, (int)Tb);
  RG_LAUNCH_CHECK("radius_hits (tiles)");
  hipLaunchKernelGGL(hits_merge_kernel, dim3((unsigned)(((long long)na + 255) / 256)), dim3(256), 0, rg_stream(stream), pmin, pcnt, na, (int)Tb,
                     count, mind2);
  RG_LAUNCH_CHECK("radius_hits (merge)");
  return RG_OK;
}
