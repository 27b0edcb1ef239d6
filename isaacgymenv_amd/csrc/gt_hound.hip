// gt_hound.hip -- UsefulHound control, fused (include/gymtask.h gt_hound_control).
//
// Replaces the torch statements of useful_hound.py:695-726 that run before every simulate of the
// decimation loop: the leg PD and the arm's operational-space controller (_compute_osc_torques,
// useful_hound.py:660-691).  In torch the OSC is ~40 launches per decimation step including two
// batched torch.inverse calls, each of which checks its LU info on the host (a device sync); here
// it is one lane per env: the env's 6x6 arm mass-matrix block, the 6x6 Jacobian block and the
// end-effector velocity are loaded once and the whole controller runs in registers in float64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gymtask.h"
#include "gt_host.h"
#include "gt_osc6.h"

namespace {

__global__ __launch_bounds__(64) void k_hound_control(gt_hound_control_params p, const float* __restrict__ actions,
                                                     const float* __restrict__ dof, const float* __restrict__ leg_default,
                                                     const float* __restrict__ mm, const float* __restrict__ jac,
                                                     const float* __restrict__ rb, float* __restrict__ torques,
                                                     float* __restrict__ arm_control) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.num_envs) return;
  constexpr int ND = 18, NL = 12;
  const float* a = actions + (size_t)e * ND;
  const float* ds = dof + (size_t)e * ND * 2;
  float* tq = torques + (size_t)e * ND;
  // ---- legs: reference float32 expression order
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const float t = p.kp * (p.action_scale * a[j] + leg_default[j] - ds[2 * j]) - p.kd * ds[2 * j + 1];
    tq[j] = fminf(fmaxf(t, -p.torque_limit), p.torque_limit);
  }
  // ---- arm OSC (float64)
  const int nv = p.nv, o = nv - 6;
  double M[36], J[36];
  const float* mme = mm + (size_t)e * nv * nv;
  const float* je = jac + (((size_t)e * p.num_links + p.jac_row) * 6) * nv;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      M[i * 6 + j] = mme[(o + i) * nv + o + j];
      J[i * 6 + j] = je[i * nv + j];
    }
  const float* eef = rb + ((size_t)e * p.num_links + p.eef_link) * 13;
  double dpose[6], u[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) dpose[k] = (double)(a[NL + k] * p.arm_cmd_limit[k] / p.arm_action_scale);
  gt_osc6::torques(M, J, dpose, eef + 7, ds + 2 * NL, p.arm_kp, p.arm_kd, p.arm_kp_null, p.arm_kd_null, p.arm_default,
                   u);
  float* ac = arm_control + (size_t)e * p.arm_control_stride;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float lim = p.arm_effort[k];
    const float v = fminf(fmaxf((float)u[k], -lim), lim);
    tq[NL + k] = v;
    ac[k] = v;
  }
}

}  // namespace

extern "C" int gt_hound_control(const gt_hound_control_params* p, const float* actions, const float* dof_state,
                                const float* leg_default, const float* mass_matrix, const float* jacobian,
                                const float* rigid_body, float* torques, float* arm_control, void* stream) {
  if (!p || p->num_envs <= 0 || p->nv < 6 || p->num_links <= 0 || p->jac_row < 0 || p->jac_row >= p->num_links ||
      p->eef_link < 0 || p->eef_link >= p->num_links || p->arm_control_stride < 6 || !actions || !dof_state ||
      !leg_default || !mass_matrix || !jacobian || !rigid_body || !torques || !arm_control) {
    gt_set_last_error("gt_hound_control: invalid parameters or null buffers");
    return -1;
  }
  const int blocks = (p->num_envs + 63) / 64;
  hipLaunchKernelGGL(k_hound_control, dim3(blocks), dim3(64), 0, (hipStream_t)stream, *p, actions, dof_state,
                     leg_default, mass_matrix, jacobian, rigid_body, torques, arm_control);
  return gt_launched("gt_hound_control");
}
