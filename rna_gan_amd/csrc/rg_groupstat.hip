// rg_groupstat.hip -- the two primitives of the per-patient representations and the RNA-conditioning metric
// (rna_gan_amd.representation, rna_gan_amd.metrics.ConditioningFidelity): fp64 sums of feature rows PER GROUP (a patient's tiles)
// and, between two sets of fp64 centroids, the rank of every row's designated partner among all rows of the other set.
// Nothing here depends on the build's 16-bit storage type: both builds compile the same code.
#include "rg_pairtile.h"

namespace {

// ---- per-group sums of feature rows, fp64 -------------------------------------------------------------------------------------
// A workgroup owns GS_COLS consecutive columns of ONE group g for the whole call; thread j owns the entry (g, j).  It starts from
// the value already in sums[g][j] and adds (double)x[r][j] for the rows r of its group in ascending r: one chain of additions per
// entry, nobody else touches the entry -- no atomics, the bits of a sequential loop in row order, and the same bits whether the
// rows arrive in one call or split over several (the chain simply goes on from the stored value).
//
// The group ids are staged through LDS GS_IDS at a time (one coalesced load per thread, shared by the four waves).  A wave then
// reads 64 staged ids with ONE ds_read_b32 (lane l takes id l: 64 consecutive dwords, conflict-free), turns "id == g" into a
// 64-bit ballot and walks the set bits in ascending order: the walk is uniform over the wave, costs nothing for the rows of other
// groups (at G = 512 one row in 512 is the owner's) and only the owner's rows are ever loaded -- a wave reads 64 consecutive
// floats of such a row.  A row whose id is outside [0, G) matches no workgroup: it is never read.
constexpr int GS_COLS = 256;      // threads per workgroup = columns per workgroup
constexpr int GS_IDS = 1024;      // group ids staged per pass

__global__ __launch_bounds__(GS_COLS) void group_sums_kernel(const float* __restrict__ x, int ldx, int n, int F,
                                                             const int* __restrict__ group, double* __restrict__ sums,
                                                             long long* __restrict__ counts, unsigned colblocks) {
  __shared__ int ids[GS_IDS];
  const int g = (int)(blockIdx.x / colblocks);
  const unsigned cb = blockIdx.x % colblocks;
  const int tid = threadIdx.x, lane = tid & 63;
  const long long j = (long long)cb * GS_COLS + tid;
  const bool own = j < F;
  const size_t at = (size_t)g * (size_t)F + (size_t)j;
  double acc = own ? sums[at] : 0.0;
  long long count = 0;
  for (long long r0 = 0; r0 < n; r0 += GS_IDS) {
    for (int e = tid; e < GS_IDS; e += GS_COLS) ids[e] = r0 + e < n ? group[r0 + e] : -1;
    __syncthreads();
    const int staged = (int)(n - r0 < GS_IDS ? n - r0 : GS_IDS);
    for (int c = 0; c < staged; c += 64) {
      unsigned long long mine = __ballot(ids[c + lane] == g);          // past the end: -1, never a group
      count += __popcll(mine);
      while (mine) {                                                   // uniform over the wave, ascending rows
        const int bit = __ffsll((long long)mine) - 1;
        mine &= mine - 1;
        const long long r = r0 + c + bit;
        if (own) acc = acc + (double)x[(size_t)r * (size_t)ldx + (size_t)j];
      }
    }
    __syncthreads();
  }
  if (own) sums[at] = acc;
  if (cb == 0 && tid == 0) counts[g] = counts[g] + count;
}

// ---- ranks of the designated partners, fp64 -----------------------------------------------------------------------------------
// d2 is rg_pairtile.h's tile (PairDist2) on fp64 rows: one rounded subtraction per feature, fma(diff, diff, acc) in ascending f
// from 0 -- its staging, its LDS layout and its contract are stated there; pairs of rows past the end are skipped by INDEX.
//
// A workgroup owns 64 query rows and every `split`-th tile of 64 rows of b.  It first computes the tile of its query rows against
// THEIR OWN TARGET ROWS, gathered by index (the rows of b at target[r]): the diagonal of that tile is d*(r), with the bits that
// the same pair has in any other tile -- the value does not depend on the tiling.  Then, per tile of b, every thread compares its
// 16 values with d* and counts in registers; the counts of a row are integers, so they are added with integer atomics (LDS, then
// one atomicAdd per row onto rank, which the entry point zeroes in the same call when split > 1): the same bits on every run.
constexpr int MT = PAIR_ROWS;     // rows per tile

__global__ __launch_bounds__(256) void match_ranks_kernel(const double* __restrict__ a, int lda, int na, const double* __restrict__ b,
                                                          int ldb, int nb, int F, const int* __restrict__ target,
                                                          int* __restrict__ rank, double* __restrict__ dtarget, int Tb, int split) {
  __shared__ __attribute__((aligned(16))) double sa[MT * PairStage<double>::PITCH];
  __shared__ __attribute__((aligned(16))) double sb[MT * PairStage<double>::PITCH];
  __shared__ double dstar[MT];
  __shared__ int tgt[MT], brow[MT], rowcnt[MT];
  const int ti = (int)(blockIdx.x / (unsigned)split), part = (int)(blockIdx.x % (unsigned)split);
  const long long i0 = (long long)ti * MT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  if (tid < MT) {
    const long long r = i0 + tid;
    long long t = -1;
    if (r < na) {
      t = target ? (long long)target[r] : r;
      t = t < 0 ? 0 : (t >= nb ? nb - 1 : t);              // a bad target reads a valid row, never outside b
    }
    tgt[tid] = brow[tid] = (int)t;
    rowcnt[tid] = 0;
  }
  __syncthreads();
  // acc[p][q] = d2(a[i0 + ty + 16 p], b[brow[tx + 16 q]]); brow: 64 row indices of b, -1 = no row
  const PairRowsFrom arows{i0, na};
  const PairRowsAt brows{brow};
  double acc[4][4];
  pair_tile_accumulate<double, PairDist2>(a, lda, arows, b, ldb, brows, F, false, sa, sb, acc);
  if (ty == tx) {
#pragma unroll
    for (int p = 0; p < 4; ++p) dstar[ty + 16 * p] = acc[p][p];
  }
  __syncthreads();
  double ds[4];
  int t[4], cnt[4] = {0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    ds[p] = dstar[ty + 16 * p];
    t[p] = tgt[ty + 16 * p];
  }
  for (int tj = part; tj < Tb; tj += split) {
    const long long j0 = (long long)tj * MT;
    __syncthreads();                                       // brow is free: everybody is past the previous tile's staging
    if (tid < MT) brow[tid] = j0 + tid < nb ? (int)(j0 + tid) : -1;
    __syncthreads();
    pair_tile_accumulate<double, PairDist2>(a, lda, arows, b, ldb, brows, F, false, sa, sb, acc);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long s = j0 + tx + 16 * q;
      if (s >= nb) continue;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const double v = acc[p][q];                        // a NaN v or a NaN d*: both comparisons are false
        if (s != t[p] && (v < ds[p] || (v == ds[p] && s < t[p]))) ++cnt[p];
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (cnt[p]) atomicAdd(&rowcnt[ty + 16 * p], cnt[p]);
  __syncthreads();
  if (tid < MT && i0 + tid < na) {
    const long long r = i0 + tid;
    const double d = dstar[tid];
    int total = rowcnt[tid];
    if (part == 0) {
      dtarget[r] = d;
      if (d != d) total = nb - 1;                          // no count anywhere for a NaN d*: this part supplies the whole rank
    }
    if (split == 1) rank[r] = total;
    else if (total) atomicAdd(&rank[r], total);
  }
}

}  // namespace

extern "C" int rg_group_sums_update(const float* x, int ldx, int n, int F, const int32_t* group, int G, double* sums,
                                    long long* counts, void* stream) {
  RG_REQUIRE(F >= 1 && G >= 1 && n >= 0 && ldx >= F, RG_EINVAL, "group_sums_update: bad sizes n %d F %d G %d ldx %d", n, F, G, ldx);
  RG_REQUIRE(x && group && sums && counts, RG_EINVAL, "group_sums_update: null buffer");
  if (n == 0) return RG_OK;
  const long long colblocks = ((long long)F + GS_COLS - 1) / GS_COLS;
  const long long blocks = (long long)G * colblocks;
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "group_sums_update: G %d x F %d need %lld workgroups", G, F, blocks);
  hipLaunchKernelGGL(group_sums_kernel, dim3((unsigned)blocks), dim3(GS_COLS), 0, rg_stream(stream), x, ldx, n, F, group, sums, counts,
                     (unsigned)colblocks);
  RG_LAUNCH_CHECK("group_sums_update");
  return RG_OK;
}

extern "C" int rg_match_ranks(const double* a, int lda, int na, const double* b, int ldb, int nb, int F, const int32_t* target,
                              int32_t* rank, double* dtarget, void* stream) {
  RG_REQUIRE(F >= 1 && nb >= 1 && na >= 0 && lda >= F && ldb >= F, RG_EINVAL,
             "match_ranks: bad sizes na %d nb %d F %d lda %d ldb %d", na, nb, F, lda, ldb);
  RG_REQUIRE(target || na <= nb, RG_EINVAL, "match_ranks: no target and na %d > nb %d", na, nb);
  RG_REQUIRE(a && b && rank && dtarget, RG_EINVAL, "match_ranks: null buffer");
  if (na == 0) return RG_OK;
  const long long Ta = pair_tiles(na), Tb = pair_tiles(nb);
  // the tiles of b are dealt to `split` workgroups per 64 query rows while the query tiles alone leave compute units idle (each
  // part pays the d* tile again, so no more parts than that)
  long long split = 256 / Ta;
  split = split < 1 ? 1 : (split > Tb ? Tb : split);
  if (split > 1) {
    hipError_t e = hipMemsetAsync(rank, 0, (size_t)na * sizeof(int32_t), rg_stream(stream));
    RG_REQUIRE(e == hipSuccess, RG_EHIP, "match_ranks: clearing rank failed: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(match_ranks_kernel, dim3((unsigned)(Ta * split)), dim3(256), 0, rg_stream(stream), a, lda, na, b, ldb, nb, F,
                     target, rank, dtarget, (int)Tb, (int)split);
  RG_LAUNCH_CHECK("match_ranks");
  return RG_OK;
}
