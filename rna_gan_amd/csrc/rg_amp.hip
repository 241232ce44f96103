// rg_amp.hip -- dynamic loss scaling on the device (opt-in: rna_gan_amd.amp.DynamicLossScaler).
//
// The state is a small int32 buffer (layout RG_AMP_* in include/rnagan_hip.h): the exponent k of the scale S = 2^k, the growth
// tracker, the skipped-step counter, and per stepped network ("slot") the exponent latched at its train_op's first seed and a
// non-finite flag.  One optimizer step of a scaled train_op is
//     rg_nonfinite_probe (every gradient value the step's Adam launches read, and the loss)  -> flag[slot]
//     rg_adam_hyper_dev3   hyper[8] = 2^-latch[slot], hyper[9] = flag[slot]; the step counter advances only when the flag is clear
//     Adam launches        return at once when hyper[9] != 0 (rg_common.h)
//     rg_amp_update        the GradScaler rule on k / tracker / skipped, flag[slot] = 0
// so the decision, the skip and the update stay on the device and inside captured step graphs.
#include "rg_common.h"
#include "rg_internal.h"

namespace {

constexpr int PROBE_MAX_SEGS = 32;
struct ProbeSeg { const void* p; unsigned long long n; int h16; int pad; };
struct ProbeSegs { int nseg; int pad; ProbeSeg s[PROBE_MAX_SEGS]; };

// exponent field all ones = infinity or NaN, tested on the raw bits (no floating-point compare that -ffast-math could fold away)
#ifdef RG_HALF_F16
constexpr uint32_t H16_EXP = 0x7c00u;     // IEEE fp16
#else
constexpr uint32_t H16_EXP = 0x7f80u;     // bf16
#endif
__device__ __forceinline__ int nf32(uint32_t w) { return (w & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ int nf16(uint32_t b) { return (b & H16_EXP) == H16_EXP; }
__device__ __forceinline__ int nf16x2(uint32_t w) { return nf16(w & 0xffffu) | nf16(w >> 16); }
__device__ __forceinline__ int nf_word(uint32_t w, int h16) { return h16 ? nf16x2(w) : nf32(w); }

__global__ __launch_bounds__(256) void nonfinite_probe_kernel(ProbeSegs t, int* __restrict__ flag) {
  int bad = 0;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (int si = 0; si < t.nseg; ++si) {
    const ProbeSeg sg = t.s[si];
    const size_t esz = sg.h16 ? 2 : 4;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(sg.p);
    // elements before the first 16-byte boundary, the 16-byte body, the elements after it
    size_t head = ((16 - ((uintptr_t)b & 15)) & 15) / esz;
    if (head > sg.n) head = sg.n;
    const size_t nv = (sg.n - head) * esz / 16;
    const uint4* body = reinterpret_cast<const uint4*>(b + head * esz);
    for (size_t q = tid; q < nv; q += stride) {
      const uint4 w = body[q];
      bad |= nf_word(w.x, sg.h16) | nf_word(w.y, sg.h16) | nf_word(w.z, sg.h16) | nf_word(w.w, sg.h16);
    }
    const size_t done = head + nv * 16 / esz;      // first element after the body
    const size_t odd = head + (sg.n - done);       // < 16 elements
    if (tid < odd) {
      const size_t i = tid < head ? tid : done + (tid - head);
      bad |= sg.h16 ? nf16(reinterpret_cast<const uint16_t*>(b)[i]) : nf32(reinterpret_cast<const uint32_t*>(b)[i]);
    }
  }
  // wave-wide OR; one atomic per wave, and only when the wave found something
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

__global__ void amp_update_kernel(int* st, int slot, int interval, int kmin, int kmax) {
  int* flag = st + RG_AMP_FLAG + slot;
  if (*flag != 0) {
    st[RG_AMP_EXP] = max(st[RG_AMP_EXP] - 1, kmin);      // backoff 0.5
    st[RG_AMP_TRACKER] = 0;
    st[RG_AMP_SKIPPED] += 1;
  } else if (st[RG_AMP_TRACKER] + 1 >= interval) {
    st[RG_AMP_EXP] = min(st[RG_AMP_EXP] + 1, kmax);      // growth 2
    st[RG_AMP_TRACKER] = 0;
  } else {
    st[RG_AMP_TRACKER] += 1;
  }
  *flag = 0;
}

__global__ void amp_latch_kernel(int* st, int slot) { st[RG_AMP_LATCH + slot] = st[RG_AMP_EXP]; }

// rg_head_grad with the seed coefficient coef * 2^part(k): the product is formed first, as the host forms coef * S for the static
// scale (a power of two: exact either way)
__global__ void head_grad_dev_kernel(const float* h, float* gh, int N, float coef, const int* st, int slot, int part,
                                     float slope) {
  const int k = st[RG_AMP_LATCH + slot];
  const int e = part == 0 ? k : (part == 1 ? (k >> 1) : k - (k >> 1));
  const float c = coef * ldexpf(1.f, e);
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) gh[n] = c * lrelu_mask(h[n], slope);
}

inline bool slot_ok(int slot) { return slot >= 0 && slot < RG_AMP_SLOTS; }

}  // namespace

extern "C" int rg_nonfinite_probe(int nseg, const void* const* seg_ptr, const unsigned long long* seg_n, const int* seg_dtype,
                                  int* flag, void* stream) {
  RG_REQUIRE(seg_ptr && seg_n && seg_dtype && flag && nseg >= 1 && nseg <= PROBE_MAX_SEGS, RG_EINVAL,
             "nonfinite_probe: 1 .. %d segments", PROBE_MAX_SEGS);
  ProbeSegs t{};
  t.nseg = nseg;
  unsigned long long vecs = 0;
  for (int i = 0; i < nseg; ++i) {
    RG_REQUIRE(seg_dtype[i] == RG_F32 || seg_dtype[i] == RG_H16, RG_EINVAL, "nonfinite_probe: segment %d: dtype %d", i,
               seg_dtype[i]);
    const int h16 = seg_dtype[i] == RG_H16;
    RG_REQUIRE(seg_n[i] == 0 || (seg_ptr[i] && ((uintptr_t)seg_ptr[i] & (h16 ? 1 : 3)) == 0), RG_EINVAL,
               "nonfinite_probe: segment %d: null or misaligned", i);
    t.s[i] = ProbeSeg{seg_ptr[i], seg_n[i], h16, 0};
    vecs += seg_n[i] * (h16 ? 2 : 4) / 16;
  }
  unsigned long long blocks = (vecs + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;        // grid-stride: 8 workgroups per CU
  hipLaunchKernelGGL(nonfinite_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, rg_stream(stream), t, flag);
  RG_LAUNCH_CHECK("nonfinite_probe");
  return RG_OK;
}

extern "C" int rg_amp_update(int* state, int slot, int growth_interval, int min_exp, int max_exp, void* stream) {
  RG_REQUIRE(state && slot_ok(slot) && growth_interval >= 1 && min_exp <= max_exp && min_exp > -127 && max_exp < 127,
             RG_EINVAL, "amp_update: bad args");
  hipLaunchKernelGGL(amp_update_kernel, dim3(1), dim3(1), 0, rg_stream(stream), state, slot, growth_interval, min_exp, max_exp);
  RG_LAUNCH_CHECK("amp_update");
  return RG_OK;
}

extern "C" int rg_amp_latch(int* state, int slot, void* stream) {
  RG_REQUIRE(state && slot_ok(slot), RG_EINVAL, "amp_latch: bad args");
  hipLaunchKernelGGL(amp_latch_kernel, dim3(1), dim3(1), 0, rg_stream(stream), state, slot);
  RG_LAUNCH_CHECK("amp_latch");
  return RG_OK;
}

extern "C" int rg_head_grad_dev(const float* h, float* gh, int N, float coef, const int* state, int slot, int part, float slope,
                                void* stream) {
  RG_REQUIRE(h && gh && N > 0 && state && slot_ok(slot) && part >= 0 && part <= 2, RG_EINVAL, "head_grad_dev: bad args");
  hipLaunchKernelGGL(head_grad_dev_kernel, dim3((N + 255) / 256), dim3(256), 0, rg_stream(stream), h, gh, N, coef, state, slot,
                     part, slope);
  RG_LAUNCH_CHECK("head_grad_dev");
  return RG_OK;
}

extern "C" int rg_gp_coef_parts_scaled_dev(const float* part, int nblocks, float* sq, float* loss, float* coef, float lambd,
                                           const int* state, int slot, void* stream) {
  RG_REQUIRE(part && loss && coef && nblocks > 0 && state && slot_ok(slot), RG_EINVAL, "gp_coef_parts_dev: bad args");
  return rg_skinny_lu_part_final(part, nblocks, sq, 0, 1, loss, coef, lambd, rg_stream(stream), 1.f, 1.f,
                                 state + RG_AMP_LATCH + slot);
}
