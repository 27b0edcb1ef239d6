// gt_humanoid.hip -- Humanoid post-physics tail and reset, fused (include/gymtask.h gt_humanoid_post_physics,
// gt_humanoid_reset_flagged).
//
// Replaces the torch statements of humanoid.py:378-413 (compute_humanoid_observations) and :324-375
// (compute_humanoid_reward) that follow the resets of post_physics_step: one lane per env builds the 108-wide
// observation (it reads the DOF force tensor next to the dof state), the potentials, the up and heading vectors, the
// reward with its per-dof motor-effort ratio in the joint-limit and electricity costs, and the done mask.  Built with
// -ffp-contract=off and written in the reference's expression order (gt_loco.h, gt_anymal_tail.h), so results track
// the torch path to float rounding (tests/test_humanoid_tail_gpu.py).  The done count is published as Ant's is
// (gt_wave.h).  The per-dof loops run to the runtime num_dofs and keep nothing per dof in registers: the limits and
// efforts are read from the kernel arguments, the sums are carried in three scalars.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gymtask.h"
#include "torch_philox.h"
#include "gt_anymal_tail.h"
#include "gt_loco.h"
#include "gt_wave.h"
#include "gt_host.h"

namespace {

using gt_loco::kTwoPi;
using gt_loco::py_mod;
using gt_loco::quat_mul;
using gt_tail::quat_rotate;
using gt_tail::quat_rotate_inverse;

// torch_jit_utils.normalize_angle: atan2(sin(x), cos(x))
__device__ __forceinline__ float normalize_angle(float x) { return atan2f(sinf(x), cosf(x)); }

__global__ void __launch_bounds__(64) k_humanoid_tail(gt_humanoid_params p, gt_humanoid_buffers b) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  bool done = false;
  if (e < p.num_envs) {
    const int nd = p.num_dofs;
    const float* rs = b.root_states + (size_t)e * 13;
    const float pos[3] = {rs[0], rs[1], rs[2]};
    const float* tg = b.targets + (size_t)e * 3;
    // to_target with z zeroed, potentials (humanoid.py:390-394)
    const float tt[3] = {tg[0] - pos[0], tg[1] - pos[1], 0.0f};
    const float prev = b.potentials[e];
    const float tnorm = sqrtf(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
    const float pot = -tnorm / p.dt;
    // compute_heading_and_up (torch_jit_utils.py:248-263)
    const float tn = fmaxf(tnorm, 1e-9f);
    const float tdir[3] = {tt[0] / tn, tt[1] / tn, tt[2] / tn};
    float tq[4];
    quat_mul(rs + 3, b.inv_start_rot + (size_t)e * 4, tq);
    const float vec0[3] = {1.0f, 0.0f, 0.0f}, vec1[3] = {0.0f, 0.0f, 1.0f};
    float up[3], hd[3];
    quat_rotate(tq, vec1, up);
    quat_rotate(tq, vec0, hd);
    const float up_proj = up[2];
    const float heading_proj = hd[0] * tdir[0] + hd[1] * tdir[1] + hd[2] * tdir[2];
    // compute_rot (torch_jit_utils.py:266-277): local velocities, roll / yaw, angle to target
    float vl[3], avl[3];
    quat_rotate_inverse(tq, rs + 7, vl);
    quat_rotate_inverse(tq, rs + 10, avl);
    const float x = tq[0], y = tq[1], z = tq[2], w = tq[3];
    const float roll = py_mod(atan2f(2.0f * (w * x + y * z), w * w - x * x - y * y + z * z), kTwoPi);
    const float yaw = py_mod(atan2f(2.0f * (w * z + x * y), w * w + x * x - y * y - z * z), kTwoPi);
    const float walk = atan2f(tg[2] - pos[2], tg[0] - pos[0]);
    // observation (humanoid.py:402-411)
    float* ob = b.obs_buf + (size_t)e * (24 + 4 * nd);
    ob[0] = pos[2];
    ob[1] = vl[0]; ob[2] = vl[1]; ob[3] = vl[2];
    ob[4] = avl[0] * p.angular_velocity_scale;
    ob[5] = avl[1] * p.angular_velocity_scale;
    ob[6] = avl[2] * p.angular_velocity_scale;
    ob[7] = normalize_angle(yaw);
    ob[8] = normalize_angle(roll);
    ob[9] = normalize_angle(walk - yaw);
    ob[10] = up_proj;
    ob[11] = heading_proj;
    const float* ds = b.dof_state + (size_t)e * nd * 2;
    const float* frc = b.dof_force + (size_t)e * nd;
    const float* act = b.actions + (size_t)e * nd;
    float* ob_pos = ob + 12;
    float* ob_vel = ob_pos + nd;
    float* ob_frc = ob_vel + nd;
    float* ob_sen = ob_frc + nd;
    float* ob_act = ob_sen + GT_HUMANOID_SENSOR_VALUES;
    // the reward's three sums over the dofs (humanoid.py:352-359), carried while the columns are written
    float ac = 0.f, el = 0.f, lim = 0.f;
    // 0 while every observation column is finite, NaN otherwise (x * 0 is NaN for an infinite or NaN x)
    float chk = 0.f;
#pragma unroll
    for (int k = 0; k < 12; ++k) chk += ob[k] * 0.f;
    for (int j = 0; j < nd; ++j) {
      const float lo = p.dof_lower[j], hi = p.dof_upper[j];
      const float dpos = (2.0f * ds[2 * j] - hi - lo) / (hi - lo);  // unscale
      const float dvel = ds[2 * j + 1] * p.dof_vel_scale;
      const float a = act[j];
      ob_pos[j] = dpos;
      ob_vel[j] = dvel;
      ob_frc[j] = frc[j] * p.contact_force_scale;
      ob_act[j] = a;
      chk += (dpos + dvel + ob_frc[j] + a) * 0.f;
      const float ratio = p.motor_efforts[j] / p.max_motor_effort;
      const float scaled_cost = p.joints_at_limit_cost_scale * (fabsf(dpos) - 0.98f) / 0.02f;
      ac += a * a;
      lim += (fabsf(dpos) > 0.98f ? 1.0f : 0.0f) * scaled_cost * ratio;
      el += fabsf(a * dvel) * ratio;
    }
    const float* sn = b.sensors + (size_t)e * GT_HUMANOID_SENSOR_VALUES;
#pragma unroll
    for (int k = 0; k < GT_HUMANOID_SENSOR_VALUES; ++k) {
      ob_sen[k] = sn[k] * p.contact_force_scale;
      chk += ob_sen[k] * 0.f;
    }
    b.potentials[e] = pot;
    b.prev_potentials[e] = prev;
    float* uv = b.up_vec + (size_t)e * 3;
    float* hv = b.heading_vec + (size_t)e * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) { uv[k] = up[k]; hv[k] = hd[k]; }
    // reward and done mask (humanoid.py:344-373)
    const float heading_reward = heading_proj > 0.8f ? p.heading_weight : p.heading_weight * heading_proj / 0.8f;
    const float up_reward = up_proj > 0.93f ? 0.0f + p.up_weight : 0.0f;
    const float alive = 1.0f * 2.0f;
    const float progress = pot - prev;
    float total = progress + alive + up_reward + heading_reward - p.actions_cost_scale * ac -
                  p.energy_cost_scale * el - lim;
    bool fallen = pos[2] < p.termination_height;
    if (fallen) total = 1.0f * p.death_cost;
    // not the reference's: an env whose observation or reward is not finite (a diverged simulation) ends here as a
    // fallen one does -- a zero observation, the death cost, the done flag -- so that reset_idx restores it at the
    // next step and nothing non-finite reaches the learner (humanoid.py's height test is false for NaN)
    if (!(chk == 0.f) || !(fabsf(total) <= 3.4028235e38f)) {
      fallen = true;
      total = 1.0f * p.death_cost;
      for (int k = 0; k < 24 + 4 * nd; ++k) ob[k] = 0.f;
    }
    b.rew_buf[e] = total;
    long long r = fallen ? 1ll : b.reset_buf[e];
    if ((double)b.progress_buf[e] >= (double)p.max_episode_length - 1.0) r = 1ll;
    b.reset_buf[e] = r;
    done = r != 0;
  }
  gt_wave::record_done(b, done, (unsigned)e >> 6, (gridDim.x * blockDim.x + 63) / 64);
}

// reset_idx of the flagged envs (gymtask.h gt_humanoid_reset_flagged): one lane per env, one wave per workgroup; a
// flagged env's rank among all flagged envs is the exclusive prefix of the earlier waves' ballot popcounts
// (gt_wave.h flagged_rank), which is its row in the two [k][nd] draws
__global__ void __launch_bounds__(64) k_humanoid_reset_flagged(gt_humanoid_params p, gt_humanoid_buffers b,
                                                               gt_humanoid_reset_args r) {
  const int nd = p.num_dofs;
  const int lane = threadIdx.x, w = blockIdx.x, e = w * 64 + lane;
  int base;
  const unsigned long long mine = gt_wave::flagged_rank(b.reset_masks, w, lane, base);
  if (e >= p.num_envs || !((mine >> lane) & 1ull)) return;
  const int t = base + (int)__popcll(mine & ((1ull << lane) - 1ull));
  float* ds = r.dof_state + (size_t)e * nd * 2;
  for (int j = 0; j < nd; ++j) {
    const size_t q = (size_t)t * nd + j;
    const float up = r.u_pos ? r.u_pos[q] : torch_philox::rand_at(r.plan_pos, q);
    const float uv = r.u_vel ? r.u_vel[q] : torch_philox::rand_at(r.plan_vel, q);
    const float off = r.pos_range * up + r.pos_lower;  // torch_rand_float: (upper - lower) * rand + lower
    const float x = r.initial_dof_pos[(size_t)e * nd + j] + off;
    ds[2 * j] = fmaxf(fminf(x, p.dof_upper[j]), p.dof_lower[j]);  // tensor_clamp = max(min(t, upper), lower)
    ds[2 * j + 1] = r.vel_range * uv + r.vel_lower;
  }
  const float* tg = b.targets + (size_t)e * 3;
  const float* ir = r.initial_root_states + (size_t)e * 13;
  const float px = tg[0] - ir[0], py = tg[1] - ir[1], pz = 0.0f;
  // -torch.norm(to_target) / dt: ATen divides by a host scalar as a product with its float reciprocal
  const float prev = -sqrtf(px * px + py * py + pz * pz) * (1.0f / p.dt);
  b.prev_potentials[e] = prev;
  b.potentials[e] = prev;
  r.progress_buf[e] = 0;
  b.reset_buf[e] = 0;
  r.env_ids_out[t] = e;
}

bool dofs_ok(const gt_humanoid_params* p) { return p->num_dofs >= 1 && p->num_dofs <= GT_HUMANOID_MAXD; }

}  // namespace

extern "C" int gt_humanoid_reset_flagged(const gt_humanoid_params* p, const gt_humanoid_buffers* b, int k,
                                         const gt_humanoid_reset_args* r, void* stream) {
  if (!p || !b || !r || p->num_envs <= 0 || !dofs_ok(p) || !b->reset_masks || !b->targets || !b->potentials ||
      !b->prev_potentials || !b->reset_buf || !r->initial_dof_pos || !r->initial_root_states || !r->dof_state ||
      !r->progress_buf || !r->env_ids_out || k < 0 || k > p->num_envs ||
      (!r->u_pos && r->plan_pos.numel != (uint32_t)k * (uint32_t)p->num_dofs) ||
      (!r->u_vel && r->plan_vel.numel != (uint32_t)k * (uint32_t)p->num_dofs)) {
    gt_set_last_error("gt_humanoid_reset_flagged: invalid parameters, null buffers, num_dofs outside 1..32 or plans "
                      "that do not cover k x num_dofs");
    return -1;
  }
  if (k == 0) return 0;
  hipLaunchKernelGGL(k_humanoid_reset_flagged, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b,
                     *r);
  return gt_launched("gt_humanoid_reset_flagged");
}

extern "C" int gt_humanoid_post_physics(const gt_humanoid_params* p, const gt_humanoid_buffers* b, void* stream) {
  if (!p || !b || p->num_envs <= 0 || !dofs_ok(p) || !b->root_states || !b->dof_state || !b->dof_force ||
      !b->sensors || !b->actions || !b->targets || !b->inv_start_rot || !b->potentials || !b->prev_potentials ||
      !b->up_vec || !b->heading_vec || !b->obs_buf || !b->rew_buf || !b->reset_buf || !b->progress_buf ||
      !b->reset_count) {
    gt_set_last_error("gt_humanoid_post_physics: invalid parameters, null buffers or num_dofs outside 1..32");
    return -1;
  }
  const int blocks = (p->num_envs + 63) / 64;
  hipLaunchKernelGGL(k_humanoid_tail, dim3(blocks), dim3(64), 0, (hipStream_t)stream, *p, *b);
  return gt_launched("gt_humanoid_post_physics");
}
