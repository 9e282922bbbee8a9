// Device-side helpers shared by the kernel families of libtsm_hip.so (one translation unit per family: an edit to one
// family recompiles one object) and the internal launch functions they call across files.  gfx950 only.
//
//   tsm_conv_rules.h   (HIP-free) parameter blocks, tile geometries, every family's validity / grid rule, conv_route
//   tsm_igemm.hip      conv_igemm (every precision, every tile), launch_conv (conv_route -> one launch), the split-K reduction
//   tsm_bf16_256.hip   conv_bf16_256[p]_kernel: the 256 x 256 LDS-DMA tile, one-shot and persistent
//   tsm_ws.hip         weight-stationary bf16 kernels: conv3x3_ws[128], conv1x1_ws[n]
//   tsm_bneck.hip      bneck_ws_kernel: a whole layer1 Bottleneck per launch (bf16)
//   tsm_conv31.hip     conv31_fused_kernel: conv3 + residual of block b and shift + conv1 of block b + 1 per launch (bf16)
//   tsm_front.hip      front_s2_kernel: shift + conv1 + stride-2 conv2 of layer2.0 per launch (bf16)
//   tsm_fused23.hip    conv23_fused_kernel: conv2 + conv3 + residual per launch (fp32 / split-bf16)
//   tsm_stem.hip       stem_direct / stem_pool[_f32]: the 7x7 stem with the max-pool fused behind it
//   tsm_ops.hip        pack / convert / preprocess / gather_clips / preprocess_clips / preprocess_indexed / maxpool / shift / head / pool_feat / scores_to_states / top1_tally, device_info()
//   tsm_similarity.hip cosine_dist_kernel: the cosine-distance matrix of unit rows on the exact-fp32 MFMA
//   tsm_nonlocal.hip   maxpool2x2_kernel, nonlocal_attn_kernel: the non-local block's pool and its fused online-softmax attention (fp32)
//   tsm_convnext.hip   dwconv7_ln_kernel, ln_kernel, stem_pack4_kernel, gelu_kernel: the non-GEMM part of a ConvNeXt-Base image model (fp32)
//   tsm_tdn.hip        tdn_front_kernel, tdn_fuse_kernel, mse_*_kernel: the difference front end, the blends and the long-term (mSE + temporal conv) module of a TDN-ResNet50 (fp32)
#pragma once
#include "tsm_kernels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>

namespace tsm {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS row stride in floats: 32 data + 4 pad.  With ds_read_b128 (16-lane groups, 64 banks) the 16
// rows of a group land on 16 distinct 4-bank slots (row*36 mod 64 is a permutation of multiples
// of 4), so fragment reads are conflict-free; ds_write_b128 of 8 consecutive lanes covers one row.
constexpr int kLds = 36;

constexpr unsigned kInvalid = 0x80000000u;  // >= num_records of every descriptor below

// XCD-chunked tile order.  Workgroup b of a launch runs on XCD b & 7 (round-robin dispatch), and each XCD has an L2 of its
// own: virtual index v = b + k * gridDim.x (gridDim.x a multiple of 8, or a single pass) is mapped to a tile such that every
// XCD walks ONE contiguous eighth of the n tiles -- tiles that share halo lines, weights or neighbouring frames are then
// fetched once per XCD instead of once per workgroup.  A bijection on [0, n) for any grid.
__device__ __forceinline__ long xcd_chunked(long v, long n) {
  const long q8 = n >> 3, r8 = n & 7, x = v & 7;
  return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + (v >> 3);
}
__device__ __forceinline__ int xcd_chunked32(int v, int n) {   // the same in 32 bits (tile counts fit; half the scalar work)
  const int q8 = n >> 3, r8 = n & 7, x = v & 7;
  return (x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8) + (v >> 3);
}

// Buffer descriptors: a raw (untyped, unswizzled) window of `bytes` bytes at `base`; offsets at or past num_records load
// zeros and store nothing.  buffer_window: a window that may exceed what 32-bit offsets reach (a tensor's tail from a
// tile's first row on) -- clamped, the kernel addresses only its tile's neighbourhood; buffer_fixed: a size that is an int.
// (Kernels that keep a window in a struct store base + window_bytes() and build the descriptor where it is used: hipcc's
//  host pass cannot hold __amdgpu_buffer_rsrc_t in a struct.)
__device__ __forceinline__ int window_bytes(size_t bytes) { return (int)(bytes > 0x7FFFFFF0u ? 0x7FFFFFF0u : bytes); }
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_fixed(const void *base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_window(const void *base, size_t bytes) {
  return buffer_fixed(base, window_bytes(bytes));
}

// Cache policy of the activation stores of the bf16 kernel families (the aux operand of raw_buffer_store: 0 = plain,
// 2 = nt, 16 = sc1 = write-through that drops the line from the XCD's L2, MI355X_MICROARCH.md "stores of each flavour").
#ifndef TSM_OUT_AUX
#define TSM_OUT_AUX 0
#endif
#ifndef TSM_AUX_256
#define TSM_AUX_256 TSM_OUT_AUX
#endif
#ifndef TSM_AUX_C31
#define TSM_AUX_C31 TSM_OUT_AUX
#endif
#ifndef TSM_AUX_WS
#define TSM_AUX_WS TSM_OUT_AUX
#endif
#ifndef TSM_AUX_BNECK
#define TSM_AUX_BNECK TSM_OUT_AUX
#endif

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// split-bf16 helpers.  A 32-byte group is [hi x8 | lo x8]; word w of a half holds elements 2w (low 16
// bits) and 2w+1 (high 16 bits).
__device__ __forceinline__ float split_elem(u32x4 half8, int e) {
  const unsigned w = half8[e >> 1];
  return __builtin_bit_cast(float, (e & 1) ? (w & 0xFFFF0000u) : (w << 16));
}
__device__ __forceinline__ unsigned pack_bf16(float x0, float x1) {  // element 0 in the low half
  const bf16x2 h = {(__bf16)x0, (__bf16)x1};
  return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned *hi, unsigned *lo) {
  const bf16x2 h = {(__bf16)x0, (__bf16)x1};  // v_cvt_pk_bf16_f32, round to nearest even
  const unsigned hw = __builtin_bit_cast(unsigned, h);
  const float r0 = x0 - __builtin_bit_cast(float, hw << 16);
  const float r1 = x1 - __builtin_bit_cast(float, hw & 0xFFFF0000u);
  const bf16x2 l = {(__bf16)r0, (__bf16)r1};
  *hi = hw;
  *lo = __builtin_bit_cast(unsigned, l);
}

__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, (int)soff, 0));
}
// Compile-time loop: f(std::integral_constant<int, 0>{}) ... f(<N - 1>) -- unrolled in the AST, for bodies too large for
// `#pragma unroll` to honour (its size threshold silently leaves a loop, and the register arrays go to scratch).
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, f);
}

// Counted vector-memory waits (the instruction takes an immediate).  wait_vmcnt<N>(): `s_waitcnt vmcnt(N)` for a constant
// expression; wait_vmcnt_lgkm0<N>(): with lgkmcnt(0) in the same instruction; wait_vmcnt(n): for an n that is a constant only
// after inlining and unrolling (the switch folds to its one case).
template <int N> __device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int N> __device__ __forceinline__ void wait_vmcnt_lgkm0() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_vmcnt(int n) {
#define TSM_VMCNT_CASE(k) case k: wait_vmcnt<k>(); break;
  switch (n) {
    TSM_VMCNT_CASE(0) TSM_VMCNT_CASE(1) TSM_VMCNT_CASE(2) TSM_VMCNT_CASE(3) TSM_VMCNT_CASE(4) TSM_VMCNT_CASE(5) TSM_VMCNT_CASE(6) TSM_VMCNT_CASE(7)
    TSM_VMCNT_CASE(8) TSM_VMCNT_CASE(9) TSM_VMCNT_CASE(10) TSM_VMCNT_CASE(11) TSM_VMCNT_CASE(12) TSM_VMCNT_CASE(13) TSM_VMCNT_CASE(14) TSM_VMCNT_CASE(15)
    TSM_VMCNT_CASE(16) TSM_VMCNT_CASE(17) TSM_VMCNT_CASE(18) TSM_VMCNT_CASE(19) TSM_VMCNT_CASE(20) TSM_VMCNT_CASE(21) TSM_VMCNT_CASE(22) TSM_VMCNT_CASE(23)
    TSM_VMCNT_CASE(24) TSM_VMCNT_CASE(25) TSM_VMCNT_CASE(26) TSM_VMCNT_CASE(27) TSM_VMCNT_CASE(28) TSM_VMCNT_CASE(29) TSM_VMCNT_CASE(30) TSM_VMCNT_CASE(31)
    TSM_VMCNT_CASE(32) TSM_VMCNT_CASE(33) TSM_VMCNT_CASE(34) TSM_VMCNT_CASE(35) TSM_VMCNT_CASE(36) TSM_VMCNT_CASE(37) TSM_VMCNT_CASE(38) TSM_VMCNT_CASE(39)
    TSM_VMCNT_CASE(40) TSM_VMCNT_CASE(41) TSM_VMCNT_CASE(42) TSM_VMCNT_CASE(43) TSM_VMCNT_CASE(44) TSM_VMCNT_CASE(45) TSM_VMCNT_CASE(46) TSM_VMCNT_CASE(47)
    TSM_VMCNT_CASE(48) TSM_VMCNT_CASE(49) TSM_VMCNT_CASE(50) TSM_VMCNT_CASE(51) TSM_VMCNT_CASE(52) TSM_VMCNT_CASE(53) TSM_VMCNT_CASE(54) TSM_VMCNT_CASE(55)
    TSM_VMCNT_CASE(56) TSM_VMCNT_CASE(57) TSM_VMCNT_CASE(58) TSM_VMCNT_CASE(59) TSM_VMCNT_CASE(60) TSM_VMCNT_CASE(61) TSM_VMCNT_CASE(62) TSM_VMCNT_CASE(63)
    default: wait_vmcnt<0>(); break;
  }
#undef TSM_VMCNT_CASE
}
// Phase stamps of a diagnostic build (-DTSM_<FAMILY>_STAMP=1, the switch each family file declares; tools/probes/*_stamp.py):
// TSM_STAMP_DECL(on, n) declares n cycle sums `stamp_acc` and the clock reading they are measured from, TSM_STAMP(on, i) adds
// the s_memtime cycles since the previous stamp to sum i; the kernel prints the sums at its end.  `on` is the family's switch:
// with 0, the product, both are constant-folded away and leave the code object as it is without them.
#define TSM_STAMP_DECL(on, n) \
  [[maybe_unused]] unsigned long long stamp_acc[(on) ? (n) : 1] = {}, stamp_last = (on) ? __builtin_amdgcn_s_memtime() : 0
#define TSM_STAMP(on, i)                                          \
  do {                                                            \
    if (on) {                                                     \
      const unsigned long long _t = __builtin_amdgcn_s_memtime(); \
      stamp_acc[(on) ? (i) : 0] += _t - stamp_last;               \
      stamp_last = _t;                                            \
    }                                                             \
  } while (0)

// Every kernel launch of the library goes through this macro: the launch itself, plus one line in the calling thread's
// launch trace when a test has switched it on (tsm_trace_launches; note_launch is a thread-local pointer test otherwise).
// The trace names the kernel as the launch site spells it and, for a launch inside a template, the enclosing
// function's template arguments -- so a parity test can assert that the kernel under test is the one that ran.
#define TSM_KLAUNCH(kern, ...)                          \
  do {                                                  \
    ::tsm::note_launch(#kern, __PRETTY_FUNCTION__);     \
    hipLaunchKernelGGL(kern, __VA_ARGS__);              \
  } while (0)
// The same for a kernel that walks its output tiles / frames in either direction (`rev`: its params' reverse field): a
// reverse walk appends " [reverse]" to the trace line, so a test can tell that the direction it asked for reached the kernel
// (a bracket of its own: the line still ends in ']', and whatever prefix of it a test matches still matches).
#define TSM_KLAUNCH_WALK(rev, kern, ...)                             \
  do {                                                               \
    ::tsm::note_launch(#kern, __PRETTY_FUNCTION__, (rev) ? 1 : 0);   \
    hipLaunchKernelGGL(kern, __VA_ARGS__);                           \
  } while (0)

// ... and with a bracket about its grid in the trace line (note_launch's `mark`; NULL: none)
#define TSM_KLAUNCH_WALK_MARK(rev, mark, kern, ...)                          \
  do {                                                                       \
    ::tsm::note_launch(#kern, __PRETTY_FUNCTION__, (rev) ? 1 : 0, (mark));   \
    hipLaunchKernelGGL(kern, __VA_ARGS__);                                   \
  } while (0)

inline unsigned grid_for(int64_t total, int cap) {
  const int64_t blocks = (total + 255) / 256;
  return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

// Per DEVICE, once: the CU count that sizes the persistent grids and the > 64 KB dynamic-LDS opt-in of every kernel
// that needs one.  tsm_hip.h lets engines on several devices live in one process, so neither may be cached from
// whichever device happened to launch first.  device_info() (tsm_ops.hip) runs every family's opt-in function once per
// device: each returns the first error of its hipFuncSetAttribute calls.
struct DeviceInfo {
  int n_cu = 256;
  hipError_t status = hipSuccess;
};
const DeviceInfo &device_info();
hipError_t lds_opt_in(const void *kernel, size_t bytes);   // hipFuncSetAttribute(MaxDynamicSharedMemorySize)
struct OptIn {   // a family's opt-ins: the first error of its lds_opt_in calls
  hipError_t first = hipSuccess;
  void operator()(const void *fn, size_t bytes) {
    const hipError_t st = lds_opt_in(fn, bytes);
    if (st != hipSuccess && first == hipSuccess) first = st;
  }
};
hipError_t opt_in_bf16_256();
hipError_t opt_in_ws();
hipError_t opt_in_bneck();
hipError_t opt_in_conv31();
hipError_t opt_in_front();

// launch functions one family's dispatch calls in another family's file
// (of a route conv_route accepted for one of the file's families, after launch_conv's device_info() status check; p.ntm / p.ntn set)
hipError_t launch_conv_bf16_256(const ConvParams &p, const ConvRoute &r, hipStream_t s);
hipError_t launch_conv_ws(const ConvParams &p, const ConvRoute &r, hipStream_t s);
hipError_t launch_conv23_ws(const Fused23Params &p, hipStream_t s);

}  // namespace tsm
