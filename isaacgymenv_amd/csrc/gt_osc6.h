// gt_osc6.h -- the 6-DoF arm's operational-space controller in float64, one env per lane, all in registers: what
// gt_hound.hip (UsefulHound's arm on the trunk) and gt_arm.hip (Houndarm's bare arm) share.
//   u = J^T M_eef (kp dpose - kd v_eef) + (1 - J^T M_eef J M^-1) M u_null,  M_eef = (J M^-1 J^T)^-1,
//   u_null = -kd_null qd + kp_null ((default - q + pi) mod 2 pi - pi)
// (useful_hound.py:660-691, hound_arm.py:462-493).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace gt_osc6 {

// In-place inverse of a 6x6 row-major matrix, Gauss-Jordan with partial pivoting (as LU-based
// torch.inverse, no error on singular input: a zero pivot yields inf/nan like torch's result would).
__device__ __forceinline__ void inv6(double* A) {
  double B[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) B[i] = (i % 7 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double best = fabs(A[c * 6 + c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double v = fabs(A[r * 6 + c]);
      if (v > best) { best = v; piv = r; }
    }
    // row swap by predicated selects (registers stay statically indexed)
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      if (r == piv) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double ta = A[c * 6 + k], tb = B[c * 6 + k];
          A[c * 6 + k] = A[r * 6 + k]; B[c * 6 + k] = B[r * 6 + k];
          A[r * 6 + k] = ta; B[r * 6 + k] = tb;
        }
      }
    }
    const double inv = 1.0 / A[c * 6 + c];
#pragma unroll
    for (int k = 0; k < 6; ++k) { A[c * 6 + k] *= inv; B[c * 6 + k] *= inv; }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      if (r == c) continue;
      const double f = A[r * 6 + c];
#pragma unroll
      for (int k = 0; k < 6; ++k) { A[r * 6 + k] -= f * A[c * 6 + k]; B[r * 6 + k] -= f * B[c * 6 + k]; }
    }
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) A[i] = B[i];
}

// C = A B (6x6)
__device__ __forceinline__ void mul6(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += A[i * 6 + k] * B[k * 6 + j];
      C[i * 6 + j] = s;
    }
}

// The controller's body.  M, J: the arm's 6x6 mass-matrix and Jacobian blocks (row-major); dpose: the scaled
// cartesian action; eef_vel: the end-effector's 6 velocity components; arm_dof: the arm's dof-state rows (q, qd
// interleaved); the gains and the default pose are per-dof float[6].  u receives the unclamped torques.
__device__ __forceinline__ void torques(const double* M, const double* J, const double* dpose, const float* eef_vel,
                                        const float* arm_dof, const float* kp, const float* kd, const float* kp_null,
                                        const float* kd_null, const float* dflt, double* u) {
  double Minv[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) Minv[i] = M[i];
  inv6(Minv);
  double JMi[36], Meef[36], T[36];
  mul6(J, Minv, JMi);  // J M^-1
  // M_eef^-1 = J M^-1 J^T
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s += JMi[i * 6 + k] * J[j * 6 + k];
      Meef[i * 6 + j] = s;
    }
  inv6(Meef);
  double f[6], g[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) f[k] = (double)kp[k] * dpose[k] - (double)kd[k] * (double)eef_vel[k];
  // u = J^T (M_eef f)
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += Meef[i * 6 + k] * f[k];
    g[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += J[k * 6 + i] * g[k];
    u[i] = s;
  }
  // null space: u_null = M (-kd_null qd + kp_null wrap(default - q)),  u += (1 - J^T M_eef J M^-1) u_null
  const double kTwoPi = 2.0 * M_PI;
  double un[6], mun[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double q = arm_dof[2 * k], qd = arm_dof[2 * k + 1];
    const double x = (double)dflt[k] - q + M_PI;
    const double w = x - kTwoPi * floor(x / kTwoPi) - M_PI;  // torch.remainder (floor mod)
    un[k] = (double)kd_null[k] * -qd + (double)kp_null[k] * w;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += M[i * 6 + k] * un[k];
    mun[i] = s;
  }
  mul6(Meef, JMi, T);  // j_eef_inv = M_eef J M^-1
  // (J^T T) mun
  double tm[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += T[i * 6 + k] * mun[k];
    tm[i] = s;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += J[k * 6 + i] * tm[k];
    u[i] += mun[i] - s;
  }
}

}  // namespace gt_osc6
