// rg_linprobe.hip -- the three primitives of the linear-probe scores (rna_gan_amd.linprobe: the classifier two-sample test and
// train-on-synthetic; tissue_probe.py): multinomial logistic regression on fp32 feature rows that stay on the device.  One
// objective evaluation is  z = x W^T + b  (rg_linear_scores_f64), the softmax residual and loss of every row
// (rg_softmax_residual_f64) and  R^T x  (rg_rows_weighted_colsums_f64); the same column sums, with a 0/1 column for R, give the
// moments the standardisation needs.  Everything is fp64 with a fixed summation order and no atomics.
// Nothing here depends on the build's 16-bit storage type: both builds compile the same code.
#include "rg_internal.h"

namespace {

// ---- scores: z[r][c] = sum_f x[r][f] w[c][f] (+ bias[c]) ----------------------------------------------------------------------
// rg_pairtile.h's PairDot tile has this shape, but it stages both sides as ONE element type; here one side is fp32 rows and the
// other fp64 weights, and C is 2..8 in practice against the tile's 64 -- so this is a small kernel of its own and that header is
// untouched.
//
// A workgroup owns LS_ROWS rows and LS_CLS classes.  Thread (row, cg) = (tid & 31, tid >> 5) owns ONE accumulator, row `row` of
// the block against class c0 + cg: one chain acc = fma((double)x, w, acc) in ascending f from 0.0, so the value is the same for
// every tiling and launch plan (a workgroup never splits F).  A pass stages LS_K features: the x slice as the rows lie in memory
// ([row][feature], a run of 64 lanes loads 256 consecutive bytes of one row), the w slice likewise as doubles.  Only the
// features below F are walked, so nothing is padded and no padding enters a chain; rows past n and classes past C are staged
// as zeros, never loaded, and their accumulators are not stored.
//
// LDS banking.  ds_read_b32 banks by (byte address / 4) mod 64.  The lanes of a wave hold rows 0..31 twice (two values of cg):
// the pitch of LS_K + 1 floats (1 mod 64) puts rows 0..31 of one feature on 32 distinct banks, and the second half of the wave
// reads the same 32 addresses (a broadcast, no conflict).  The w operand is two addresses per wave (one per cg).  Staging stores walk consecutive
// features of a row: consecutive banks.  A pass is 256 features (LDS: 32 x 257 x 4 + 8 x 256 x 8 = 48.1 KB): between two passes
// the chains wait for the next slice's global loads behind a barrier, and there are too few chains (n C) to hide that behind
// other waves, so the passes are made long; 32 + 8 independent loads per thread are in flight per pass.
constexpr int LS_ROWS = 32;       // rows per workgroup
constexpr int LS_CLS = 8;         // classes per workgroup
constexpr int LS_K = 256;         // features per staging pass
constexpr int LS_XP = LS_K + 1;   // pitch of a staged x row, floats

__global__ __launch_bounds__(256) void linear_scores_kernel(const float* __restrict__ x, int ldx, int n, int F,
                                                            const double* __restrict__ w, int ldw, int C,
                                                            const double* __restrict__ bias, double* __restrict__ z, int ldz,
                                                            unsigned cchunks) {
  __shared__ float sx[LS_ROWS * LS_XP];
  __shared__ double sw[LS_CLS * LS_K];
  const long long r0 = (long long)(blockIdx.x / cchunks) * LS_ROWS;
  const int c0 = (int)(blockIdx.x % cchunks) * LS_CLS;
  const int tid = threadIdx.x, row = tid & 31, cg = tid >> 5;
  double acc = 0.0;
  for (int k0 = 0; k0 < F; k0 += LS_K) {
    const int kn = F - k0 < LS_K ? F - k0 : LS_K;
    for (int e = tid; e < LS_ROWS * LS_K; e += 256) {
      const int rr = e / LS_K, kk = e % LS_K;
      const bool in = kk < kn && r0 + rr < n;
      sx[rr * LS_XP + kk] = in ? x[(size_t)(r0 + rr) * (size_t)ldx + (size_t)(k0 + kk)] : 0.f;
    }
    for (int e = tid; e < LS_CLS * LS_K; e += 256) {
      const int cc = e / LS_K, kk = e % LS_K;
      const bool in = kk < kn && c0 + cc < C;
      sw[e] = in ? w[(size_t)(c0 + cc) * (size_t)ldw + (size_t)(k0 + kk)] : 0.0;
    }
    __syncthreads();
    const float* xr = &sx[row * LS_XP];
    const double* wr = &sw[cg * LS_K];
#pragma unroll 4
    for (int k = 0; k < kn; ++k) acc = fma((double)xr[k], wr[k], acc);
    __syncthreads();
  }
  const long long r = r0 + row;
  const int c = c0 + cg;
  if (r < n && c < C) z[(size_t)r * (size_t)ldz + (size_t)c] = bias ? acc + bias[c] : acc;
}

// ---- softmax residual and loss, one thread per row ----------------------------------------------------------------------------
// Three passes over the C logits of the row (C is small; the row is re-read, not kept): the maximum, s = sum exp(z_c - m) in
// ascending c from 0.0, then p_c = exp(z_c - m) / s -- the same exp of the same argument as in the second pass, so p sums to what
// s was built from.  The maximum takes a NaN explicitly (a comparison would skip it): a NaN logit makes m, every e_c, s and so the
// whole row NaN, and no other row.  |z| of 1e3 and more is harmless: z_c - m <= 0, exp underflows to 0, s >= 1.
// A masked row (label outside [0, C)) is written as exact zeros without looking at its logits.
__global__ __launch_bounds__(256) void softmax_residual_kernel(const double* __restrict__ z, int ldz, int n, int C,
                                                               const int* __restrict__ label, const double* __restrict__ weight,
                                                               double* __restrict__ resid, int ldr, double* __restrict__ row_loss) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const double* zr = z + (size_t)r * (size_t)ldz;
  double* out = resid + (size_t)r * (size_t)ldr;
  const int y = label[r];
  if (y < 0 || y >= C) {
    for (int c = 0; c < C; ++c) out[c] = 0.0;
    row_loss[r] = 0.0;
    return;
  }
  const double wt = weight ? weight[r] : 1.0;
  double m = zr[0];
  for (int c = 1; c < C; ++c) {
    const double v = zr[c];
    if (v != v || v > m) m = (m != m) ? m : v;
  }
  double s = 0.0;
  for (int c = 0; c < C; ++c) s = s + exp(zr[c] - m);
  for (int c = 0; c < C; ++c) {
    const double p = exp(zr[c] - m) / s;
    out[c] = wt * (p - (c == y ? 1.0 : 0.0));
  }
  row_loss[r] = wt * (log(s) - (zr[y] - m));
}

// ---- weighted column sums: out[c][f] = sum_rows r[row][c] t(x[row][f]) ---------------------------------------------------------
// Partials.  A workgroup owns one block of RG_COLSUM_ROWS rows, CS_COLS consecutive columns and CS_CLS consecutive classes.
// Thread (col, cg) = (tid & 63, tid >> 6) owns the entries (c0 + cg, f) and (c0 + cg + 4, f): per entry ONE chain
// acc = fma(r[row][c], t(x[row][f]), acc) over the rows of the block in ascending order from 0.0, stored to ws[block][c][f].
// The r block is staged in LDS once ([row][class], 16 KB) and read as a broadcast (one address per wave and class); a wave loads
// 64 consecutive floats of a row of x.  The loads do not depend on the chains, so the compiler keeps several rows in flight;
// what is left is the chain's own latency -- 256 dependent v_fma_f64 -- and with C of 2 only two of the four waves hold a class:
// the pass is latency-bound at small C, which is why the rows are cut into blocks (n / 256 x F / 64 workgroups) rather than one
// chain per entry over all rows.
// Finisher.  One thread per entry adds the block partials in ascending block order from 0.0 and WRITES out.
constexpr int CS_COLS = 64;       // columns per workgroup
constexpr int CS_CLS = 8;         // classes per workgroup: two per thread

template <int POWER>
__global__ __launch_bounds__(256) void colsum_partials_kernel(const float* __restrict__ x, int ldx, int n, int F,
                                                              const double* __restrict__ r, int ldr, int C,
                                                              double* __restrict__ ws, unsigned colblocks, unsigned cchunks) {
  __shared__ double sr[RG_COLSUM_ROWS * CS_CLS];
  unsigned b = blockIdx.x;
  const int c0 = (int)(b % cchunks) * CS_CLS;
  b /= cchunks;
  const long long f = (long long)(b % colblocks) * CS_COLS + (threadIdx.x & 63);
  const long long block = b / colblocks;
  const long long row0 = block * RG_COLSUM_ROWS;
  const int rows = (int)(n - row0 < RG_COLSUM_ROWS ? n - row0 : RG_COLSUM_ROWS);
  const int tid = threadIdx.x, cg = tid >> 6;
  for (int e = tid; e < RG_COLSUM_ROWS * CS_CLS; e += 256) {
    const int rr = e / CS_CLS, cc = e % CS_CLS;
    const bool in = rr < rows && c0 + cc < C;
    sr[e] = in ? r[(size_t)(row0 + rr) * (size_t)ldr + (size_t)(c0 + cc)] : 0.0;
  }
  __syncthreads();
  if (f >= F || c0 + cg >= C) return;
  const float* xc = x + (size_t)row0 * (size_t)ldx + (size_t)f;
  double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 4
  for (int rr = 0; rr < rows; ++rr) {
    const double v = (double)xc[(size_t)rr * (size_t)ldx];
    const double t = POWER == 2 ? v * v : v;
    acc0 = fma(sr[rr * CS_CLS + cg], t, acc0);
    acc1 = fma(sr[rr * CS_CLS + cg + 4], t, acc1);
  }
  const size_t at = ((size_t)block * (size_t)C + (size_t)(c0 + cg)) * (size_t)F + (size_t)f;
  ws[at] = acc0;
  if (c0 + cg + 4 < C) ws[at + 4 * (size_t)F] = acc1;
}

__global__ __launch_bounds__(256) void colsum_finish_kernel(const double* __restrict__ ws, long long blocks, long long entries,
                                                            double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  double acc = 0.0;
  for (long long b = 0; b < blocks; ++b) acc = acc + ws[(size_t)b * (size_t)entries + (size_t)e];
  out[e] = acc;
}

}  // namespace

extern "C" int rg_linear_scores_f64(const float* x, int ldx, int n, int F, const double* w, int ldw, int C, const double* bias,
                                    double* z, int ldz, void* stream) {
  RG_REQUIRE(F >= 1 && C >= 1 && n >= 0 && ldx >= F && ldw >= F && ldz >= C, RG_EINVAL,
             "linear_scores_f64: bad sizes n %d F %d C %d ldx %d ldw %d ldz %d", n, F, C, ldx, ldw, ldz);
  RG_REQUIRE(x && w && z, RG_EINVAL, "linear_scores_f64: null buffer");
  if (n == 0) return RG_OK;
  const long long rowblocks = ((long long)n + LS_ROWS - 1) / LS_ROWS, cchunks = ((long long)C + LS_CLS - 1) / LS_CLS;
  RG_REQUIRE(rowblocks * cchunks <= 0x7fffffffLL, RG_EUNSUPPORTED, "linear_scores_f64: n %d x C %d need %lld workgroups", n, C,
             rowblocks * cchunks);
  hipLaunchKernelGGL(linear_scores_kernel, dim3((unsigned)(rowblocks * cchunks)), dim3(256), 0, rg_stream(stream), x, ldx, n, F, w,
                     ldw, C, bias, z, ldz, (unsigned)cchunks);
  RG_LAUNCH_CHECK("linear_scores_f64");
  return RG_OK;
}

extern "C" int rg_softmax_residual_f64(const double* z, int ldz, int n, int C, const int32_t* label, const double* weight,
                                       double* resid, int ldr, double* row_loss, void* stream) {
  RG_REQUIRE(C >= 1 && n >= 0 && ldz >= C && ldr >= C, RG_EINVAL, "softmax_residual_f64: bad sizes n %d C %d ldz %d ldr %d", n, C,
             ldz, ldr);
  RG_REQUIRE(z && label && resid && row_loss, RG_EINVAL, "softmax_residual_f64: null buffer");
  if (n == 0) return RG_OK;
  hipLaunchKernelGGL(softmax_residual_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, rg_stream(stream), z, ldz,
                     n, C, label, weight, resid, ldr, row_loss);
  RG_LAUNCH_CHECK("softmax_residual_f64");
  return RG_OK;
}

extern "C" size_t rg_colsums_ws_bytes(int n, int F, int C) {
  if (n < 0 || F < 1 || C < 1) return 0;
  const size_t blocks = ((size_t)n + RG_COLSUM_ROWS - 1) / RG_COLSUM_ROWS;
  return blocks * (size_t)C * (size_t)F * sizeof(double);
}

extern "C" int rg_rows_weighted_colsums_f64(const float* x, int ldx, int n, int F, const double* r, int ldr, int C, int power,
                                            void* ws, size_t ws_bytes, double* out, void* stream) {
  RG_REQUIRE(F >= 1 && C >= 1 && n >= 0 && ldx >= F && ldr >= C, RG_EINVAL,
             "rows_weighted_colsums_f64: bad sizes n %d F %d C %d ldx %d ldr %d", n, F, C, ldx, ldr);
  RG_REQUIRE(power == 1 || power == 2, RG_EINVAL, "rows_weighted_colsums_f64: power %d is neither 1 nor 2", power);
  // no rows: nothing is read, so only out is needed; the finisher alone runs and WRITES the empty sums (+0.0)
  RG_REQUIRE(out && (n == 0 || (x && r && ws)), RG_EINVAL, "rows_weighted_colsums_f64: null buffer");
  const long long blocks = ((long long)n + RG_COLSUM_ROWS - 1) / RG_COLSUM_ROWS;
  const long long colblocks = ((long long)F + CS_COLS - 1) / CS_COLS, cchunks = ((long long)C + CS_CLS - 1) / CS_CLS;
  const long long entries = (long long)C * (long long)F;
  // (blocks * colblocks is below 2^48; the product with cchunks, below 2^28, is taken only once that is below 2^31)
  const long long tiles = blocks * colblocks <= 0x7fffffffLL ? blocks * colblocks * cchunks : 0x7fffffffLL + 1;
  RG_REQUIRE(tiles <= 0x7fffffffLL && (entries + 255) / 256 <= 0x7fffffffLL, RG_EUNSUPPORTED,
             "rows_weighted_colsums_f64: n %d x F %d x C %d need more than 2^31 - 1 workgroups", n, F, C);
  if (n > 0) {
    RG_REQUIRE(((uintptr_t)ws & 7u) == 0, RG_EWORKSPACE, "rows_weighted_colsums_f64: the workspace must be 8-byte aligned");
    const size_t need = rg_colsums_ws_bytes(n, F, C);
    RG_REQUIRE(ws_bytes >= need, RG_EWORKSPACE, "rows_weighted_colsums_f64: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const dim3 grid((unsigned)tiles);
    if (power == 2)
      hipLaunchKernelGGL(colsum_partials_kernel<2>, grid, dim3(256), 0, rg_stream(stream), x, ldx, n, F, r, ldr, C, (double*)ws,
                         (unsigned)colblocks, (unsigned)cchunks);
    else
      hipLaunchKernelGGL(colsum_partials_kernel<1>, grid, dim3(256), 0, rg_stream(stream), x, ldx, n, F, r, ldr, C, (double*)ws,
                         (unsigned)colblocks, (unsigned)cchunks);
    RG_LAUNCH_CHECK("rows_weighted_colsums_f64");
  }
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, rg_stream(stream),
                     (const double*)ws, blocks, entries, out);
  RG_LAUNCH_CHECK("rows_weighted_colsums_f64");
  return RG_OK;
}
