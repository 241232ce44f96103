// rg_pairtile.h -- the 64 x 64 fp64 tile of row pairs shared by the kernel-distance Gram sums (rg_fidstat.hip), the k-NN radii
// and ball memberships (rg_knn.hip) and the partner ranks (rg_groupstat.hip): acc[p][q] = sum over the features f of
// step(a_row[f], b_row[f]) for 64 rows of a against 64 rows of b, one 256-thread workgroup per tile.
//
// Structure.  moments_kernel's (rg_fidstat.hip: 256 threads, a 4 x 4 register block each, plain v_fma_f64 for the reason stated
// there) with the operands the other way round: there the summed index is the row and a staged slice is [row][64 columns]; here
// it is the feature, and a slice is 64 rows x PairStage<T>::K features, kept as the rows lie in memory ([row][feature]) so that
// a 16-byte LDS read brings consecutive features of one row: 4 floats, or 2 doubles.  Thread (ty, tx) = (tid >> 4, tid & 15)
// owns the rows ty + 16 p of a and tx + 16 q of b.
//
// LDS layout.  ds_read_b128 is served in groups of 16 lanes and banks by (byte address / 4) mod 64, i.e. a group is conflict-free
// when its distinct addresses fall into distinct 16-byte slots of the 256-byte bank row.  The lanes of a group read the same
// feature offset of different rows, so the slot is decided by row * pitch.  The pitch must be a whole number of slots (16-byte
// reads).  With the rows of a thread adjacent (row = 4 t + p, as in moments_kernel) neighbouring lanes are 4 pitches apart, a
// multiple of 4 slots: at most 4 distinct slots of the 16 whatever the padding, 4-way or worse.  So a thread's rows are
// INTERLEAVED (row = t + 16 p) and the pitch is 128 bytes of features + 16 = 144 bytes = 9 slots -- 36 floats, or 18 doubles:
// lanes t = 0..15 land on slots 9 t mod 16, all 16 distinct (9 is odd).  The b side of a 16-lane group holds all 16 values of tx;
// the a side holds two values of ty (adjacent rows, 9 slots apart: distinct), the rest broadcast.  Staging writes (a run of
// lanes on consecutive elements of a row) are conflict-free as well.  The byte geometry is the same for both element types, so
// the analysis is.
//
// Arithmetic (the contract of include/rnagan_hip.h).  Every operand is converted to fp64; every accumulator starts from 0.0 and
// takes ONE step per feature in ascending feature order, whatever the tiling:
//   PairDot    acc = fma(a_f, b_f, acc).  The product of two fp32 values is exact in fp64, so fma == mul + add bit for bit.
//   PairDist2  diff = a_f - b_f is ONE rounded subtraction (__dsub_rn says so in the code; the build has contraction off),
//              acc = fma(diff, diff, acc).  So d2 >= 0, d2(a, a) = 0, and d2(a, b) and d2(b, a) hold the same bits (diff only
//              changes sign).  The Gram form |a|^2 + |b|^2 - 2 <a, b> is not used: it cancels, can go negative and is not
//              symmetric bit for bit.
// Features past F and missing rows (past the end of a set, index -1 of a gathered side) are staged as zeros and never read from
// memory: fma(0, 0, acc) = acc bit for bit, so padding changes no accumulator of a real pair.  The accumulators of pairs with a
// missing row are NOT meaningful (a dot is 0, a distance |a|^2): the caller skips or masks them by INDEX.  fp32 rows widened to
// fp64 and handed to the double instantiation therefore give the bits of the float instantiation.
#pragma once
#include "rg_internal.h"

namespace {

constexpr int PAIR_ROWS = 64;     // rows per tile side: 16 x 16 threads, 4 x 4 results each (rows t, t + 16, t + 32, t + 48)

// tiles of PAIR_ROWS that cover n rows (or, in moments_kernel, n columns)
__host__ __device__ constexpr long long pair_tiles(long long n) { return (n + PAIR_ROWS - 1) / PAIR_ROWS; }

// linear index -> (ti, tj), ti <= tj < T, of the upper triangle of T x T tiles, row by row
__device__ __forceinline__ void upper_triangle_tile(int linear, int T, int& ti, int& tj) {
  int rem = linear;
  ti = 0;
  while (rem >= T - ti) { rem -= T - ti; ++ti; }
  tj = ti + rem;
}

// staged element type -> features per pass, elements per staged row (144 bytes either way) and the 16-byte LDS read
template <typename T> struct PairStage;
template <> struct PairStage<float> {
  typedef float4 Vec;
  static constexpr int K = 32, PITCH = K + 4, VEC = 4;
  static __device__ __forceinline__ double at(const float4& v, int c) { return (double)(c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w); }
};
template <> struct PairStage<double> {
  typedef double2 Vec;
  static constexpr int K = 16, PITCH = K + 2, VEC = 2;
  static __device__ __forceinline__ double at(const double2& v, int c) { return c == 0 ? v.x : v.y; }
};
// bytes of the staging buffer of one side
template <typename T> constexpr size_t pair_stage_bytes() { return (size_t)PAIR_ROWS * PairStage<T>::PITCH * sizeof(T); }

struct PairDot {
  static __device__ __forceinline__ double step(double a, double b, double acc) { return fma(a, b, acc); }
};
struct PairDist2 {
  static __device__ __forceinline__ double step(double a, double b, double acc) {
    const double diff = __dsub_rn(a, b);
    return fma(diff, diff, acc);
  }
};

// where the 64 rows of a side come from: row(rr) is the row of the set staged as row rr of the tile, where has(rr) says it exists
struct PairRowsFrom {             // the consecutive rows first + rr of a set of n rows
  long long first;
  int n;
  __device__ __forceinline__ long long row(int rr) const { return first + rr; }
  __device__ __forceinline__ bool has(int rr) const { return first + rr < n; }
};
struct PairRowsAt {               // the rows index[rr]: 64 indices in LDS (-1: no row), written and synchronised by the caller
  const int* index;
  __device__ __forceinline__ int row(int rr) const { return index[rr]; }
  __device__ __forceinline__ bool has(int rr) const { return index[rr] >= 0; }
};

// acc[p][q] = sum_f Step(a[ra.row(ty + 16 p)][f], b[rb.row(tx + 16 q)][f]), f < F ascending, from 0.0.  sa, sb: the caller's
// staging buffers (PAIR_ROWS x PairStage<T>::PITCH each, 16-byte aligned); same: the b side IS the a side (one tile of one set
// against itself) -- it is staged once and read twice, b, ldb and sb are not used (rb is still evaluated).  Block-uniform; every thread
// of the workgroup calls.  The buffers are dead on return (the last pass ends with a barrier): the caller may lay results over
// them.  Scalar loads, a run of lanes reads consecutive elements of a row: any ld >= F, no alignment needed.
template <typename T, typename Step, typename RowsA, typename RowsB>
__device__ __forceinline__ void pair_tile_accumulate(const T* __restrict__ a, int lda, const RowsA ra, const T* __restrict__ b,
                                                     int ldb, const RowsB rb, int F, bool same, T* sa, T* sb,
                                                     double (&acc)[4][4]) {
  typedef PairStage<T> S;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  const T* bs = same ? sa : sb;
  for (int k0 = 0; k0 < F; k0 += S::K) {
    for (int e = tid; e < PAIR_ROWS * S::K; e += 256) {
      const int rr = e / S::K, kk = e % S::K;
      const bool kin = k0 + kk < F;
      // both rows and both conditions before the first store: one branch per load, and a gathered index is read once
      const bool ina = kin & ra.has(rr), inb = kin & rb.has(rr);
      const size_t ia = (size_t)ra.row(rr), ib = (size_t)rb.row(rr);
      sa[rr * S::PITCH + kk] = ina ? a[ia * (size_t)lda + (size_t)(k0 + kk)] : (T)0;
      if (!same) sb[rr * S::PITCH + kk] = inb ? b[ib * (size_t)ldb + (size_t)(k0 + kk)] : (T)0;
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < S::K; k += S::VEC) {
      typename S::Vec av[4], bv[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) av[p] = *reinterpret_cast<const typename S::Vec*>(&sa[(ty + 16 * p) * S::PITCH + k]);
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[q] = *reinterpret_cast<const typename S::Vec*>(&bs[(tx + 16 * q) * S::PITCH + k]);
      // S::VEC features, in ascending order for every accumulator; an operand is widened where it is used (widening all
      // eight vectors first serialises the LDS reads behind the conversions: 10 % slower)
#pragma unroll
      for (int c = 0; c < S::VEC; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[p][q] = Step::step(S::at(av[p], c), S::at(bv[q], c), acc[p][q]);
    }
    __syncthreads();
  }
}

}  // namespace
