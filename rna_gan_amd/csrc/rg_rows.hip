// rg_rows.hip -- the batch of a RESIDENT expression table (rna_gan_amd.rna_tables): rows gathered by index into a dense, zero
// padded fp32 batch in ONE launch (rg_rows_gather_f32).
//
// A row copy: bound by memory and by the launch, no LDS, no matrix core.  A betaVAE row is 19 198 floats = 76 792 bytes, which is
// 8 mod 16: consecutive rows of the table AND of the batch alternate between 16-byte and 8-byte alignment, so a (source row,
// destination row) pair has one of three relative alignments, and which one is known only once the index has been read.  The
// kernel therefore chooses per row, from the two actual addresses (both uniform over the workgroup):
//   * the destination row is cut into 16-byte-aligned chunks of four floats; every chunk that lies inside [0, ld_dst) is written
//     with ONE 16-byte store, whatever the source looks like (a row that starts off a 16-byte boundary has a head chunk, and may
//     have a tail chunk, that is written float by float);
//   * the four floats of a chunk inside [0, F) are read with the widest access the source address of that chunk allows: one
//     16-byte load, two 8-byte loads, or four 4-byte loads -- the plain path, taken when the two rows differ by an odd number of
//     floats;  a chunk that straddles 0, F or ld_dst is assembled float by float, zeros behind F.
// A workgroup owns RW_CHUNKS chunks of one row (several workgroups share a long row) and reads its index once, through a
// workgroup-uniform (scalar) load.  The index is clamped into [0, M) and widened BEFORE the multiplication by ld_table.  No
// 16-bit type is involved: both builds of the library behave identically.
#include "rg_common.h"

namespace {

constexpr int RW_THREADS = 256;
constexpr int RW_PER_THREAD = 4;                                   // chunks per thread: four independent 16-byte loads in flight
constexpr int RW_CHUNKS = RW_THREADS * RW_PER_THREAD;              // chunks per workgroup

template <int LW> __device__ __forceinline__ float4 rw_load4(const float* p);
template <> __device__ __forceinline__ float4 rw_load4<4>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 rw_load4<2>(const float* p) {
  const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
  return make_float4(a.x, a.y, b.x, b.y);
}
template <> __device__ __forceinline__ float4 rw_load4<1>(const float* p) { return make_float4(p[0], p[1], p[2], p[3]); }

// One chunk that is not wholly inside [0, F): columns c0 .. c0 + 3, of which those inside [0, ld) are written -- the source value
// below F, zero from F on.  c0 may be negative (the head of a row that starts off a 16-byte boundary).
__device__ __forceinline__ void rw_edge_chunk(const float* __restrict__ s, float* __restrict__ d, long long c0, int F, long long ld) {
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long c = c0 + e;
    v[e] = (c >= 0 && c < F) ? s[c] : 0.f;
  }
  if (c0 >= 0 && c0 + 4 <= ld) {
    *reinterpret_cast<float4*>(d + c0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long c = c0 + e;
      if (c >= 0 && c < ld) d[c] = v[e];
    }
  }
}

// s / d: the source and destination ROW; lead: floats by which d is past a 16-byte boundary (chunk k covers columns
// 4 k - lead .. 4 k - lead + 3, and d + 4 k - lead is 16-byte aligned); k0: this thread's first chunk, the others follow at a
// stride of RW_THREADS.  LW: what the source address of a chunk allows.
template <int LW>
__device__ __forceinline__ void rw_copy(const float* __restrict__ s, float* __restrict__ d, int lead, long long k0, long long nchunks,
                                        int F, long long ld) {
  const long long first = 4 * k0 - lead, last = first + 4LL * RW_THREADS * (RW_PER_THREAD - 1);
  if (first >= 0 && last + 4 <= F) {                               // all four inside [0, F): loads first, then the stores
    float4 v[RW_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RW_PER_THREAD; ++j) v[j] = rw_load4<LW>(s + first + 4LL * RW_THREADS * j);
#pragma unroll
    for (int j = 0; j < RW_PER_THREAD; ++j) *reinterpret_cast<float4*>(d + first + 4LL * RW_THREADS * j) = v[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < RW_PER_THREAD; ++j) {
    const long long k = k0 + (long long)RW_THREADS * j;
    if (k >= nchunks) break;
    const long long c0 = 4 * k - lead;
    if (c0 >= 0 && c0 + 4 <= F)
      *reinterpret_cast<float4*>(d + c0) = rw_load4<LW>(s + c0);
    else
      rw_edge_chunk(s, d, c0, F, ld);
  }
}

__global__ __launch_bounds__(RW_THREADS) void rows_gather_kernel(const float* __restrict__ table, long long M, int F,
                                                                 long long ld_table, const int* __restrict__ index,
                                                                 float* __restrict__ dst, long long ld_dst, unsigned parts) {
  const unsigned n = blockIdx.x / parts, part = blockIdx.x % parts;            // uniform: one row, one part of it
  long long t = index ? (long long)index[n] : (long long)n;                    // read once per workgroup (a uniform load)
  t = t < 0 ? 0 : (t >= M ? M - 1 : t);                                        // a bad index reads a valid row, never outside the table
  const float* s = table + t * ld_table;                                       // 64-bit: t ld_table passes 2^31 in a real table
  float* d = dst + (long long)n * ld_dst;
  const int lead = (int)(((uintptr_t)d & 15) >> 2);
  const long long nchunks = (ld_dst + lead + 3) >> 2;
  const long long k0 = (long long)part * RW_CHUNKS + threadIdx.x;
  if (k0 >= nchunks) return;
  const unsigned sa = (unsigned)(((uintptr_t)s - 4u * (unsigned)lead) & 15);   // the source address of every chunk, mod 16
  if (sa == 0) rw_copy<4>(s, d, lead, k0, nchunks, F, ld_dst);
  else if (sa == 8) rw_copy<2>(s, d, lead, k0, nchunks, F, ld_dst);
  else rw_copy<1>(s, d, lead, k0, nchunks, F, ld_dst);
}

}  // namespace

extern "C" int rg_rows_gather_f32(const float* table, long long M, int F, long long ld_table, const int* index, float* dst, int N,
                                  long long ld_dst, void* stream) {
  RG_REQUIRE(table && dst, RG_EINVAL, "rows_gather_f32: NULL buffer");
  RG_REQUIRE(N >= 0 && F > 0, RG_EINVAL, "rows_gather_f32: bad shape N %d F %d", N, F);
  RG_REQUIRE(M > 0 || N == 0, RG_EINVAL, "rows_gather_f32: a table of %lld rows cannot fill %d rows", M, N);
  RG_REQUIRE(ld_table >= F && ld_dst >= F, RG_EINVAL, "rows_gather_f32: ld_table %lld / ld_dst %lld below F %d", ld_table, ld_dst, F);
  RG_REQUIRE(index || (long long)N <= M, RG_EINVAL, "rows_gather_f32: no index and N %d > M %lld", N, M);
  if (N == 0) return RG_OK;
  // chunks of a row: at most three floats of lead in front of ld_dst
  const long long parts = ((ld_dst + 3 + 3) / 4 + RW_CHUNKS - 1) / RW_CHUNKS;
  const long long blocks = (long long)N * parts;
  RG_REQUIRE(blocks <= 0x7fffffffLL, RG_EUNSUPPORTED, "rows_gather_f32: more than 2^31 - 1 workgroups");
  hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)blocks), dim3(RW_THREADS), 0, rg_stream(stream), table, M, F, ld_table,
                     index, dst, ld_dst, (unsigned)parts);
  RG_LAUNCH_CHECK("rows_gather_f32");
  return RG_OK;
}
