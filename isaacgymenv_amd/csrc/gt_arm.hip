// gt_arm.hip -- Houndarm's control, post-physics tail and reset, fused (include/gymtask.h gt_arm_control,
// gt_arm_post_physics, gt_arm_reset_flagged; tasks/hound_arm.py).
//
// The torch path of the task is about sixty launches per step: the operational-space controller with its three
// batched torch.inverse calls (each checks its LU info on the host, a device sync), the observation concatenation,
// the reward's norms and tanh terms, and reset_idx with four torch.rand draws behind a nonzero().  Here each is one
// kernel, one lane per env in 64-lane workgroups:
//   - the controller is gt_hound.hip's (gt_osc6.h: one float64 implementation for both arms), on the bare arm's
//     6x6 mass matrix and the joint6 row of its fixed-base Jacobian (nv = 6, no offset);
//   - the tail is float32 in the reference's expression order (built with -ffp-contract=off) and publishes the done
//     count through gt_wave.h, so a step on which nothing is done needs no nonzero();
//   - the reset is bit-identical to torch, its draws evaluated from torch's own Philox stream (torch_philox.h).
// Bandwidth-trivial: an env's rows (36 + 36 + 13 + 12 + 6 floats in, 12 out for the controller) are read by its own
// lane; no LDS.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gymtask.h"
#include "torch_philox.h"
#include "gt_host.h"
#include "gt_osc6.h"
#include "gt_wave.h"

namespace {

constexpr int ND = 6;
constexpr int kObs = 10;

__global__ __launch_bounds__(64) void k_arm_control(gt_arm_params p, const float* __restrict__ actions,
                                                   const float* __restrict__ dof, const float* __restrict__ mm,
                                                   const float* __restrict__ jac, const float* __restrict__ rb,
                                                   float* __restrict__ torques, float* __restrict__ effort) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= p.num_envs) return;
  const float* a = actions + (size_t)e * ND;
  const float* ds = dof + (size_t)e * ND * 2;
  const float* mme = mm + (size_t)e * ND * ND;
  const float* je = jac + (((size_t)e * p.num_links + p.jac_row) * 6) * ND;
  double M[36], J[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    M[i] = mme[i];
    J[i] = je[i];
  }
  const float* eef = rb + ((size_t)e * p.num_links + p.eef_link) * 13;
  double dpose[6], u[6];
  // (hound_arm.py:506: float32, left to right)
#pragma unroll
  for (int k = 0; k < 6; ++k) dpose[k] = (double)(a[k] * p.cmd_limit[k] / p.action_scale);
  gt_osc6::torques(M, J, dpose, eef + 7, ds, p.kp, p.kd, p.kp_null, p.kd_null, p.dof_default, u);
  float* tq = torques + (size_t)e * ND;
  float* ef = effort + (size_t)e * p.effort_stride;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const float lim = p.effort_limit[k];
    const float v = fminf(fmaxf((float)u[k], -lim), lim);
    tq[k] = v;
    ef[k] = v;
  }
}

__global__ void __launch_bounds__(64) k_arm_tail(gt_arm_params p, gt_arm_buffers b) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  bool done = false;
  if (e < p.num_envs) {
    const float* eef = b.rigid_body + ((size_t)e * p.num_links + p.eef_link) * 13;
    const float* cmd = b.commands + (size_t)e * 3;
    float* ob = b.obs_buf + (size_t)e * kObs;
#pragma unroll
    for (int k = 0; k < 7; ++k) ob[k] = eef[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) ob[7 + k] = cmd[k];
    // compute_houndarm_reward (hound_arm.py:556-563)
    float d2 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = eef[k] - cmd[k];
      d2 += x * x;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) v2 += eef[7 + k] * eef[7 + k];
    const float d = sqrtf(d2), v = sqrtf(v2);
    const float dist_rew = 1.0f - tanhf(10.0f * d);
    const float vel_rew = 1.0f - tanhf(10.0f * v);
    const float in_reach = d < 0.02f ? 1.0f : 0.0f;
    const float total = dist_rew * p.r_dist + vel_rew * in_reach * p.r_vel;
    b.rew_buf[e] = fmaxf(total, 0.0f);
    const long long r = b.progress_buf[e] >= (long long)p.max_episode_length - 1 ? 1ll : b.reset_buf[e];
    b.reset_buf[e] = r;
    done = r != 0;
  }
  gt_wave::record_done(b, done, (unsigned)e >> 6, (gridDim.x * blockDim.x + 63) / 64);
}

// reset_idx of the flagged envs: one lane per env, one wave per workgroup; a flagged env's rank among all flagged
// envs is the exclusive prefix of the earlier waves' ballot popcounts (gt_wave.h flagged_rank)
__global__ void __launch_bounds__(64) k_arm_reset_flagged(gt_arm_params p, gt_arm_buffers b, gt_arm_reset_args r) {
  const int lane = threadIdx.x, w = blockIdx.x, e = w * 64 + lane;
  int base;
  const unsigned long long mine = gt_wave::flagged_rank(b.reset_masks, w, lane, base);
  if (e >= p.num_envs || !((mine >> lane) & 1ull)) return;
  const int t = base + (int)__popcll(mine & ((1ull << lane) - 1ull));
  float* cmd = r.commands + (size_t)e * 3;
  // torch_rand_float: (upper - lower) * rand + lower
#pragma unroll
  for (int c = 0; c < 3; ++c) cmd[c] = r.range[c] * torch_philox::rand_at(r.plan[c], (size_t)t) + r.lower[c];
  float* ds = r.dof_state + (size_t)e * ND * 2;
  float* pc = r.pos_control + (size_t)e * p.effort_stride;
  float* ec = r.effort_control + (size_t)e * p.effort_stride;
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    // hound_arm.py:418-422: tensor_clamp(default + noise * 2.0 * (u - 0.5), lower, upper)
    const float u = torch_philox::rand_at(r.plan[3], (size_t)t * ND + j);
    const float x = p.dof_default[j] + (u - 0.5f) * p.dof_noise2;
    const float q = fmaxf(fminf(x, p.dof_upper[j]), p.dof_lower[j]);
    ds[2 * j] = q;
    ds[2 * j + 1] = 0.0f;
    pc[j] = q;
    ec[j] = 0.0f;
  }
  r.progress_buf[e] = 0;
  b.reset_buf[e] = 0;
  r.env_ids_out[t] = e;
}

bool params_ok(const gt_arm_params* p) {
  return p && p->num_envs > 0 && p->num_links > 0 && p->jac_row >= 0 && p->jac_row < p->num_links && p->eef_link >= 0 &&
         p->eef_link < p->num_links && p->effort_stride >= ND;
}

}  // namespace

extern "C" int gt_arm_control(const gt_arm_params* p, const float* actions, const float* dof_state,
                              const float* mass_matrix, const float* jacobian, const float* rigid_body, float* torques,
                              float* effort, void* stream) {
  if (!params_ok(p) || !actions || !dof_state || !mass_matrix || !jacobian || !rigid_body || !torques || !effort) {
    gt_set_last_error("gt_arm_control: invalid parameters (link indices inside num_links, effort_stride >= 6) or null "
                      "buffers");
    return -1;
  }
  hipLaunchKernelGGL(k_arm_control, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, actions,
                     dof_state, mass_matrix, jacobian, rigid_body, torques, effort);
  return gt_launched("gt_arm_control");
}

extern "C" int gt_arm_post_physics(const gt_arm_params* p, const gt_arm_buffers* b, void* stream) {
  if (!params_ok(p) || !b || !b->rigid_body || !b->commands || !b->obs_buf || !b->rew_buf || !b->reset_buf ||
      !b->progress_buf || !b->reset_count || !b->reset_masks) {
    gt_set_last_error("gt_arm_post_physics: invalid parameters (link indices inside num_links) or null buffers");
    return -1;
  }
  hipLaunchKernelGGL(k_arm_tail, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b);
  return gt_launched("gt_arm_post_physics");
}

extern "C" int gt_arm_reset_flagged(const gt_arm_params* p, const gt_arm_buffers* b, int k, const gt_arm_reset_args* r,
                                    void* stream) {
  bool ok = params_ok(p) && b && r && b->reset_masks && b->reset_buf && r->dof_state && r->commands &&
            r->pos_control && r->effort_control && r->progress_buf && r->env_ids_out && k >= 0 && k <= p->num_envs;
  if (ok)
    for (int i = 0; i < 4; ++i) ok = ok && r->plan[i].numel == (uint32_t)k * (i < 3 ? 1u : (uint32_t)ND);
  if (!ok) {
    gt_set_last_error("gt_arm_reset_flagged: invalid parameters, null buffers or plans that do not cover k, k, k, "
                      "k x 6");
    return -1;
  }
  if (k == 0) return 0;
  hipLaunchKernelGGL(k_arm_reset_flagged, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b, *r);
  return gt_launched("gt_arm_reset_flagged");
}
