// conv23_fused_kernel / conv23_fused2_kernel: Bottleneck.conv2 + conv3 + residual in one launch (fp32 / split-bf16).
#include "tsm_device.h"

namespace tsm {

// Cout3 = 4 * CMID (layer1.1-2 and layer2.1-3 of ResNet-50: CMID 64 / 128)
#define TSM_F23_KERNEL conv23_fused_kernel
#define TSM_F23_NCHUNK 4
#include "tsm_fused23_kernel.h"
#undef TSM_F23_KERNEL
#undef TSM_F23_NCHUNK

// Cout3 = 2 * CMID (layer1.1-2 of wide_resnet50_2: CMID 128, 256 outputs); instantiated for CMID = 128 only
#define TSM_F23_KERNEL conv23_fused2_kernel
#define TSM_F23_NCHUNK 2
#include "tsm_fused23_kernel.h"
#undef TSM_F23_KERNEL
#undef TSM_F23_NCHUNK

hipError_t launch_conv23_fused(const Fused23Params &p_in, int cmid, int cout3, int prec, hipStream_t s) {
  Fused23Params p = p_in;
  if (prec == kPrecBf16) {   // weight-stationary form (conv3x3_ws_kernel<true>): layer1's geometry only
    if (cmid != 64 || cout3 != 256 || !p.x || !p.w2 || !p.bias2 || !p.w3f || !p.bias3 || !p.res || !p.y || p.M != p.N * p.H * p.W)
      return hipErrorInvalidValue;
    return launch_conv23_ws(p, s);
  }
  if (prec != kPrecF32 && prec != kPrecBf16x3) return hipErrorInvalidValue;
  if (prec == kPrecBf16x3 && p.kseg_len != 0) return hipErrorInvalidValue;   // (only fp32 layers are segmented)
  if (!p.x || !p.w2 || !p.bias2 || !p.w3f || !p.bias3 || !p.res || !p.y) return hipErrorInvalidValue;
  if ((cmid != 64 && cmid != 128) || p.N <= 0 || p.H <= 0 || p.W <= 0 || p.M != p.N * p.H * p.W) return hipErrorInvalidValue;
  if (cout3 != 4 * cmid && !(cout3 == 2 * cmid && cmid == 128)) return hipErrorInvalidValue;
  if (p.kseg_len < 0 || 6.0 * p.H * p.W * cmid * 4.0 > 2.0e9) return hipErrorInvalidValue;   // 32-bit offsets per window
  const unsigned grid = (unsigned)((p.M + 63) / 64);
  if (cout3 == 2 * cmid) {
    if (prec == kPrecBf16x3) TSM_KLAUNCH_WALK(p.reverse, (conv23_fused2_kernel<128, true>), dim3(grid), dim3(512), 0, s, p);
    else TSM_KLAUNCH_WALK(p.reverse, (conv23_fused2_kernel<128, false>), dim3(grid), dim3(512), 0, s, p);
    return hipGetLastError();
  }
  if (prec == kPrecBf16x3) {
    if (cmid == 64) TSM_KLAUNCH_WALK(p.reverse, (conv23_fused_kernel<64, true>), dim3(grid), dim3(256), 0, s, p);
    else TSM_KLAUNCH_WALK(p.reverse, (conv23_fused_kernel<128, true>), dim3(grid), dim3(512), 0, s, p);
  } else {
    if (cmid == 64) TSM_KLAUNCH_WALK(p.reverse, (conv23_fused_kernel<64, false>), dim3(grid), dim3(256), 0, s, p);
    else TSM_KLAUNCH_WALK(p.reverse, (conv23_fused_kernel<128, false>), dim3(grid), dim3(512), 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace tsm
