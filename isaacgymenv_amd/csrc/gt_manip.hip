// gt_manip.hip -- the Manipulator task's controller and reset (include/gymtask.h gt_osc_control,
// gt_manip_reset_flagged; tasks/manipulator.py).  The tail is gt_arm_post_physics unchanged.
//
// gt_osc_control is the operational-space controller of gt_osc6.h with one env spread over a team of 8 lanes, 8 envs
// per wave, for nd = 6 or 7 dofs.  The one-env-per-lane form keeps every matrix of an env in one lane's registers:
// 392 registers at nd = 6 and about 620 at nd = 7, which no lane has.  Here lane r of a team
// owns row r of every left operand and of every result (at most 14 float64 live per matrix step), and the rows of a
// right operand are read back from the team's LDS slab, where the 8 lanes of a team read the same address (a
// broadcast) and the teams of a wave read disjoint banks (slab stride 212 dwords = 20 mod 64, reads of 8 or 16 bytes).
//
// The arithmetic is gt_osc6::torques', operation for operation (built with -ffp-contract=off): the Gauss-Jordan
// elimination updates are elementwise, every sum runs k = 0..n-1 from 0.0, the pivot is the first row of the largest
// magnitude.  At nd = 6 the kernel returns gt_arm_control's bits (tests/test_manipulator_gpu.py).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/gymtask.h"
#include "torch_philox.h"
#include "gt_host.h"
#include "gt_wave.h"

namespace {

constexpr int kTeam = 8;             // lanes per env
constexpr int kTeamsPerWave = 8;     // envs per 64-lane workgroup
constexpr int kRow = 14;             // a Gauss-Jordan row: 7 of A, 7 of B
constexpr int kVec = 7 * kRow;       // the slab's vector area (8 doubles) follows its 7 rows
constexpr int kSlab = kVec + 8;      // doubles per team: 848 B

// (one wave per workgroup: the barrier orders the team's LDS traffic and costs no wait on another wave)
__device__ __forceinline__ void team_sync() { __syncthreads(); }

// In-place inverse of the N x N matrix whose row r is lane r's A[0..N) (lanes r >= N idle), gt_osc6::inv6's
// Gauss-Jordan: every lane publishes its row, finds the pivot with the serial code's scan, rebuilds the normalised
// pivot row (the same bits on every lane), the pivot's lane takes row c, and every lane eliminates its own row.
template <int N>
__device__ __forceinline__ void team_inverse(double* A, double* sh, int r) {
  double B[N];
#pragma unroll
  for (int k = 0; k < N; ++k) B[k] = (k == r) ? 1.0 : 0.0;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    if (r < N) {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        sh[r * kRow + k] = A[k];
        sh[r * kRow + 7 + k] = B[k];
      }
    }
    team_sync();
    int piv = c;
    double best = fabs(sh[c * kRow + c]);
#pragma unroll
    for (int q = c + 1; q < N; ++q) {
      const double v = fabs(sh[q * kRow + c]);
      if (v > best) { best = v; piv = q; }
    }
    const double* prow = sh + piv * kRow;
    const double inv = 1.0 / prow[c];
    // rows c and piv change places: the pivot's lane goes on with the old row c
    const double* mine = sh + ((r == piv) ? c : (r < N ? r : 0)) * kRow;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const double pa = prow[k] * inv, pb = prow[7 + k] * inv;
      if (r == c) {
        A[k] = pa;
        B[k] = pb;
      } else {
        const double f = mine[c];
        A[k] = mine[k] - f * pa;
        B[k] = mine[7 + k] - f * pb;
      }
    }
    team_sync();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) A[k] = B[k];
}

// lane r < rows publishes its row of `cols` values as row r of the slab's matrix (row pitch 7)
template <int COLS>
__device__ __forceinline__ void team_publish(const double* row, double* sh, int r, int rows) {
  team_sync();  // the slab's previous readers are done
  if (r < rows) {
#pragma unroll
    for (int k = 0; k < COLS; ++k) sh[r * 7 + k] = row[k];
  }
  team_sync();
}

// lane r < n publishes one value as element r of the slab's vector
__device__ __forceinline__ void team_publish_vec(double v, double* sh, int r, int n) {
  team_sync();
  if (r < n) sh[kVec + r] = v;
  team_sync();
}

template <int ND>
__global__ __launch_bounds__(64) void k_osc_control(gt_manip_params p, const float* __restrict__ actions,
                                                   const float* __restrict__ dof, const float* __restrict__ mm,
                                                   const float* __restrict__ jac, const float* __restrict__ rb,
                                                   float* __restrict__ torques, float* __restrict__ effort) {
  __shared__ double slabs[kTeamsPerWave * kSlab];
  const int team = threadIdx.x / kTeam, r = threadIdx.x % kTeam;
  double* sh = slabs + team * kSlab;
  const int env = blockIdx.x * kTeamsPerWave + team;
  const bool live = env < p.num_envs;
  const int e = live ? env : p.num_envs - 1;  // a ragged wave's spare teams recompute the last env and store nothing
  const int rd = r < ND ? r : ND - 1, r6 = r < 6 ? r : 5;  // idle lanes read a valid row
  const float* a = actions + (size_t)e * 6;
  const float* ds = dof + (size_t)e * ND * 2;
  const float* mme = mm + (size_t)e * ND * ND;
  const float* je = jac + (((size_t)e * p.num_links + p.jac_row) * 6) * ND;
  const float* eef = rb + ((size_t)e * p.num_links + p.eef_link) * 13;

  // row r of M, row r of J (r < 6) and column r of J: J is an input, so nothing is transposed across lanes
  double Mrow[ND], Jrow[ND], Jcol[6];
#pragma unroll
  for (int k = 0; k < ND; ++k) {
    Mrow[k] = mme[rd * ND + k];
    Jrow[k] = je[r6 * ND + k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) Jcol[k] = je[k * ND + rd];

  double Minv[ND];
#pragma unroll
  for (int k = 0; k < ND; ++k) Minv[k] = Mrow[k];
  team_inverse<ND>(Minv, sh, r);

  // J M^-1: row r (r < 6), the rows of M^-1 in k order
  team_publish<ND>(Minv, sh, r, ND);
  double JMi[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) JMi[j] = 0.0;
#pragma unroll
  for (int k = 0; k < ND; ++k)
#pragma unroll
    for (int j = 0; j < ND; ++j) JMi[j] += Jrow[k] * sh[k * 7 + j];

  // M_eef^-1 = J M^-1 J^T, then its inverse
  team_publish<ND>(Jrow, sh, r, 6);
  double Meef[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < ND; ++k) s += JMi[k] * sh[j * 7 + k];
    Meef[j] = s;
  }
  team_sync();
  team_inverse<6>(Meef, sh, r);

  // u = J^T (M_eef f),  f = kp dpose - kd v_eef  (dpose in float32, left to right, as the task computes it)
  double g = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double dpose = (double)(a[k] * p.cmd_limit[k] / p.action_scale);
    const double f = (double)p.kp[k] * dpose - (double)p.kd[k] * (double)eef[7 + k];
    g += Meef[k] * f;
  }
  team_publish_vec(g, sh, r, 6);
  double u = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) u += Jcol[k] * sh[kVec + k];

  // null space: u_null = M (-kd_null qd + kp_null wrap(default - q)),  u += (1 - J^T M_eef J M^-1) u_null
  const double kTwoPi = 2.0 * M_PI;
  const double q = ds[2 * rd], qd = ds[2 * rd + 1];
  const double x = (double)p.dof_default[rd] - q + M_PI;
  const double w = x - kTwoPi * floor(x / kTwoPi) - M_PI;  // torch.remainder (floor mod)
  const double un = (double)p.kd_null[rd] * -qd + (double)p.kp_null[rd] * w;
  team_publish_vec(un, sh, r, ND);
  double mun = 0.0;
#pragma unroll
  for (int k = 0; k < ND; ++k) mun += Mrow[k] * sh[kVec + k];
  team_publish_vec(mun, sh, r, ND);
  // T = M_eef (J M^-1), row r (r < 6); then T mun
  team_publish<ND>(JMi, sh, r, 6);
  double T[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) T[j] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k)
#pragma unroll
    for (int j = 0; j < ND; ++j) T[j] += Meef[k] * sh[k * 7 + j];
  double tm = 0.0;
#pragma unroll
  for (int k = 0; k < ND; ++k) tm += T[k] * sh[kVec + k];
  team_publish_vec(tm, sh, r, 6);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) s += Jcol[k] * sh[kVec + k];
  u += mun - s;

  if (live && r < ND) {
    const float lim = p.effort_limit[r];
    const float v = fminf(fmaxf((float)u, -lim), lim);
    torques[(size_t)e * ND + r] = v;
    effort[(size_t)e * p.effort_stride + r] = v;
  }
}

constexpr int kManipDofs = 7;

// reset_idx of the flagged envs, gt_arm.hip's kernel for 7 dofs with the reference's last-two-joints rule
__global__ void __launch_bounds__(64) k_manip_reset_flagged(gt_manip_params p, gt_arm_buffers b,
                                                            gt_manip_reset_args r) {
  constexpr int ND = kManipDofs;
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
    // manipulator.py:407-413: tensor_clamp(default + noise * 2.0 * (u - 0.5), lower, upper), then the last two
    // joints at their defaults exactly (their draws belong to the (k, 7) block all the same)
    float q = p.dof_default[j];
    if (j < ND - 2) {
      const float u = torch_philox::rand_at(r.plan[3], (size_t)t * ND + j);
      const float x = p.dof_default[j] + (u - 0.5f) * p.dof_noise2;
      q = fmaxf(fminf(x, p.dof_upper[j]), p.dof_lower[j]);
    }
    ds[2 * j] = q;
    ds[2 * j + 1] = 0.0f;
    pc[j] = q;
    ec[j] = 0.0f;
  }
  r.progress_buf[e] = 0;
  b.reset_buf[e] = 0;
  r.env_ids_out[t] = e;
}

bool params_ok(const gt_manip_params* p) {
  return p && p->num_envs > 0 && (p->nd == 6 || p->nd == 7) && p->num_links > 0 && p->jac_row >= 0 &&
         p->jac_row < p->num_links && p->eef_link >= 0 && p->eef_link < p->num_links && p->effort_stride >= p->nd;
}

}  // namespace

extern "C" int gt_osc_control(const gt_manip_params* p, const float* actions, const float* dof_state,
                              const float* mass_matrix, const float* jacobian, const float* rigid_body, float* torques,
                              float* effort, void* stream) {
  if (!params_ok(p) || !actions || !dof_state || !mass_matrix || !jacobian || !rigid_body || !torques || !effort) {
    gt_set_last_error("gt_osc_control: invalid parameters (nd 6 or 7, link indices inside num_links, effort_stride >= "
                      "nd) or null buffers");
    return -1;
  }
  const dim3 grid((p->num_envs + kTeamsPerWave - 1) / kTeamsPerWave), block(64);
  if (p->nd == 6)
    hipLaunchKernelGGL(k_osc_control<6>, grid, block, 0, (hipStream_t)stream, *p, actions, dof_state, mass_matrix,
                       jacobian, rigid_body, torques, effort);
  else
    hipLaunchKernelGGL(k_osc_control<7>, grid, block, 0, (hipStream_t)stream, *p, actions, dof_state, mass_matrix,
                       jacobian, rigid_body, torques, effort);
  return gt_launched("gt_osc_control");
}

extern "C" int gt_manip_reset_flagged(const gt_manip_params* p, const gt_arm_buffers* b, int k,
                                      const gt_manip_reset_args* r, void* stream) {
  bool ok = params_ok(p) && p->nd == kManipDofs && b && r && b->reset_masks && b->reset_buf && r->dof_state &&
            r->commands && r->pos_control && r->effort_control && r->progress_buf && r->env_ids_out && k >= 0 &&
            k <= p->num_envs;
  if (ok)
    for (int i = 0; i < 4; ++i) ok = ok && r->plan[i].numel == (uint32_t)k * (i < 3 ? 1u : (uint32_t)kManipDofs);
  if (!ok) {
    gt_set_last_error("gt_manip_reset_flagged: invalid parameters (nd 7), null buffers or plans that do not cover k, "
                      "k, k, k x 7");
    return -1;
  }
  if (k == 0) return 0;
  hipLaunchKernelGGL(k_manip_reset_flagged, dim3((p->num_envs + 63) / 64), dim3(64), 0, (hipStream_t)stream, *p, *b,
                     *r);
  return gt_launched("gt_manip_reset_flagged");
}
