// gt_anymal_flat.hip -- the flat-ground tasks' post-physics tail and reset, fused (include/gymtask.h
// gt_flat_post_physics, gt_flat_reset_flagged; tasks/anymal.py: Anymal and Hound).
//
// Replaces the torch statements of compute_observations and compute_reward (anymal.py:241-276, 312-386) that follow the
// resets of post_physics_step -- about forty elementwise launches (two quat_rotate_inverse per function, quat_rotate,
// the 48-wide concatenation, the exp terms, the torque sum, three contact norms, the done mask) -- by one lane per env,
// and reset_idx (:278-304) with its five torch_rand_float draws by one lane per env as well.  Built with
// -ffp-contract=off and written in the reference's expression order (torch_jit_utils quat_rotate /
// quat_rotate_inverse), so the results track the torch path to float rounding (tests/test_flat_tail_gpu.py); the
// reset is bit-identical, its draws evaluated from torch's own Philox stream (torch_philox.h).  The done count goes
// {count, seq} into pinned host memory, so a step on which nothing is done needs no nonzero().
//
// Bandwidth-trivial kernels: an env's AoS rows (13 + 24 + 12 + 12 floats in, 48 out, the contact rows of five to nine
// links) are read and written by its own lane as gt_ant.hip does; no LDS, no scratch, nothing of the wave's size
// beyond the 64-bit ballot.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gymtask.h"
#include "torch_philox.h"
#include "gt_anymal_tail.h"
#include "gt_host.h"

namespace {

using gt_tail::quat_rotate;
using gt_tail::quat_rotate_inverse;

constexpr int ND = 12;
constexpr int kObs = 48;

__device__ __forceinline__ bool link_in_contact(const float* cf, int link) {
  const float* f = cf + (size_t)link * 3;
  return sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]) > 1.0f;
}

__global__ void __launch_bounds__(64) k_flat_tail(gt_flat_params p, gt_flat_buffers b) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  bool done = false;
  if (e < p.num_envs) {
    const float* rs = b.root_states + (size_t)e * 13;
    const float quat[4] = {rs[3], rs[4], rs[5], rs[6]};
    float lin[3], ang[3], grav[3];
    quat_rotate_inverse(quat, rs + 7, lin);
    quat_rotate_inverse(quat, rs + 10, ang);
    quat_rotate(quat, b.gravity_vec + (size_t)e * 3, grav);
    const float* cmd = b.commands + (size_t)e * 3;
    float* ob = b.obs_buf + (size_t)e * kObs;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ob[k] = lin[k] * p.lin_vel_scale;
      ob[3 + k] = ang[k] * p.ang_vel_scale;
      ob[6 + k] = grav[k];
    }
    ob[9] = cmd[0] * p.lin_vel_scale;
    ob[10] = cmd[1] * p.lin_vel_scale;
    ob[11] = cmd[2] * p.ang_vel_scale;
    const float* ds = b.dof_state + (size_t)e * ND * 2;
    const float* dflt = b.default_dof_pos + (size_t)e * ND;
    const float* act = b.actions + (size_t)e * ND;
    const float* tq = b.torques + (size_t)e * ND;
    float tsum = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      ob[12 + j] = (ds[2 * j] - dflt[j]) * p.dof_pos_scale;
      ob[24 + j] = ds[2 * j + 1] * p.dof_vel_scale;
      ob[36 + j] = act[j];
      tsum += tq[j] * tq[j];
    }
    // reward (anymal.py:334-344): x / 0.25 is ATen's product with the reciprocal, exactly 4
    const float ex = cmd[0] - lin[0], ey = cmd[1] - lin[1], ez = cmd[2] - ang[2];
    const float lin_err = ex * ex + ey * ey;
    const float ang_err = ez * ez;
    const float total = expf(-lin_err * 4.0f) * p.rew_lin_vel_xy + expf(-ang_err * 4.0f) * p.rew_ang_vel_z +
                        tsum * p.rew_torque;
    b.rew_buf[e] = fmaxf(total, 0.0f);
    // done mask (anymal.py:346-349)
    const float* cf = b.contact_forces + (size_t)e * p.num_bodies * 3;
    bool r = link_in_contact(cf, p.base_index);
    for (int i = 0; i < p.num_knees; ++i) r = r || link_in_contact(cf, p.knee_idx[i]);
    r = r || b.progress_buf[e] >= (long long)p.max_episode_length - 1;
    b.reset_buf[e] = r ? 1ll : 0ll;
    done = r;
  }
  gt_wave::record_done(b, done, (unsigned)e >> 6, (gridDim.x * blockDim.x + 63) / 64);
}

// reset_idx of the flagged envs: one lane per env, one wave per workgroup; a flagged env's rank among all flagged
// envs is the exclusive prefix of the earlier waves' ballot popcounts (gt_wave.h flagged_rank)
__global__ void __launch_bounds__(64) k_flat_reset_flagged(gt_flat_params p, gt_flat_buffers b, gt_flat_reset_args r) {
  const int lane = threadIdx.x, w = blockIdx.x, e = w * 64 + lane;
  int base;
  const unsigned long long mine = gt_wave::flagged_rank(b.reset_masks, w, lane, base);
  if (e >= p.num_envs || !((mine >> lane) & 1ull)) return;
  const int t = base + (int)__popcll(mine & ((1ull << lane) - 1ull));
  float* ds = r.dof_state + (size_t)e * ND * 2;
  const float* dflt = b.default_dof_pos + (size_t)e * ND;
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    const size_t q = (size_t)t * ND + j;
    // torch_rand_float: (upper - lower) * rand + lower
    ds[2 * j] = dflt[j] * (r.range[0] * torch_philox::rand_at(r.plan[0], q) + r.lower[0]);
    ds[2 * j + 1] = r.range[1] * torch_philox::rand_at(r.plan[1], q) + r.lower[1];
  }
  float* cmd = r.commands + (size_t)e * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) cmd[c] = r.range[2 + c] * torch_philox::rand_at(r.plan[2 + c], (size_t)t) + r.lower[2 + c];
  r.progress_buf[e] = 0;
  b.reset_buf[e] = 1;  // (anymal.py:304: 1, overwritten by the step's compute_reward)
  r.env_ids_out[t] = e;
}

bool params_ok(const gt_flat_params* p) {
  if (!p || p->num_envs <= 0 || p->num_dofs != ND || p->num_bodies <= 0 || p->base_index < 0 ||
      p->base_index >= p->num_bodies || p->num_knees < 0 || p->num_knees > 8)
    return false;
  for (int i = 0; i < p->num_knees; ++i)
    if (p->knee_idx[i] < 0 || p->knee_idx[i] >= p->num_bodies) return false;
  return true;
}

}  // namespace

extern "C" int gt_flat_post_physics(const gt_flat_params* p, const gt_flat_buffers* b, void* stream) {
  if (!params_ok(p) || !b || !b->root_states || !b->dof_state || !b->contact_forces || !b->torques || !b->actions ||
      !b->commands || !b->default_dof_pos || !b->gravity_vec || !b->obs_buf || !b->rew_buf || !b->reset_buf ||
      !b->progress_buf || !b->reset_count || !b->reset_masks) {
    gt_set_last_error("gt_flat_post_physics: invalid parameters (12 dofs, link indices inside num_bodies, at most 8 "
                      "knees) or null buffers");
    return -1;
  }
  hipLaunchKernelGGL(k_flat_tail, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b);
  return gt_launched("gt_flat_post_physics");
}

extern "C" int gt_flat_reset_flagged(const gt_flat_params* p, const gt_flat_buffers* b, int k, const gt_flat_reset_args* r,
                                     void* stream) {
  bool ok = params_ok(p) && b && r && b->reset_masks && b->default_dof_pos && b->reset_buf && r->dof_state &&
            r->commands && r->progress_buf && r->env_ids_out && k >= 0 && k <= p->num_envs;
  if (ok)
    for (int i = 0; i < 5; ++i) ok = ok && r->plan[i].numel == (uint32_t)k * (i < 2 ? (uint32_t)ND : 1u);
  if (!ok) {
    gt_set_last_error("gt_flat_reset_flagged: invalid parameters, null buffers or plans that do not cover k x 12, "
                      "k x 12, k, k, k");
    return -1;
  }
  if (k == 0) return 0;
  hipLaunchKernelGGL(k_flat_reset_flagged, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b, *r);
  return gt_launched("gt_flat_reset_flagged");
}
