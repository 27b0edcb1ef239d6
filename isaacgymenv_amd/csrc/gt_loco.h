// gt_loco.h -- what the locomotion tails (gt_ant.hip, gt_humanoid.hip) share: torch_jit_utils' quaternion product and
// torch.remainder in the reference's operation order, so each tail tracks its torch statements to float rounding.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace gt_loco {

constexpr float kTwoPi = 6.2831854820251465f;  // float(2*np.pi) as torch casts it for a float32 tensor

// torch.remainder(x, m) for float32 (sign of the divisor)
__device__ __forceinline__ float py_mod(float x, float m) {
  const float r = fmodf(x, m);
  return (r != 0.f && ((r < 0.f) != (m < 0.f))) ? r + m : r;
}

// torch_jit_utils.quat_mul (xyzw), same operation order
__device__ __forceinline__ void quat_mul(const float* a, const float* b, float* o) {
  const float x1 = a[0], y1 = a[1], z1 = a[2], w1 = a[3];
  const float x2 = b[0], y2 = b[1], z2 = b[2], w2 = b[3];
  const float ww = (z1 + x1) * (x2 + y2);
  const float yy = (w1 - y1) * (w2 + z2);
  const float zz = (w1 + y1) * (w2 - z2);
  const float xx = ww + yy + zz;
  const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
  o[3] = qq - ww + (z1 - y1) * (y2 - z2);
  o[0] = qq - xx + (x1 + w1) * (x2 + w2);
  o[1] = qq - yy + (w1 - x1) * (y2 + z2);
  o[2] = qq - zz + (z1 + y1) * (w2 - x2);
}

}  // namespace gt_loco
