// libgymrl.so -- the policy player's two kernels (include/gymrl.h: rl_policy_infer, rl_play_post).
//
// rl_policy_infer: the whole deterministic (or sampled) policy forward of rl_games' continuous player
// (players.py PpoPlayerContinuous.get_action on ModelA2CContinuousLogStd's eval forward: input
// normalisation with frozen moments, the actor MLP of Linear + ELU layers, the mu head, the action) in ONE
// launch.  One workgroup of four waves owns 16 rows and carries them through every layer: the activations
// ping-pong between two LDS buffers (row stride = widest layer + 4 floats, so the 16-B fragment reads of 16
// rows hit disjoint banks, as k_gemm_nt_f32), the products run on v_mfma_f32_16x16x4_f32 (exact f32
// products, f32 accumulation), the weights are read in place from the nn.Linear parameters ([out][in] f32,
// 16-B loads along the reduction index where the row is 16-B aligned, guarded scalar loads elsewhere -- the
// first layer of an odd obs_dim).  Each wave owns every fourth 16-column block of a layer's output and keeps
// up to eight of them in accumulators at once, so one activation fragment read feeds eight weight fragments.
// Rows past num_envs and reduction indices past obs_dim are zero-filled in LDS, never read from memory.
// The mu head and the action statements run from the last LDS buffer, one lane per (row, action).
//
// rl_play_post: rl_games BasePlayer.run's statements after env.step, one workgroup, no host synchronisation.
// (libgymrl builds with -ffp-contract=off: each statement rounds as torch's elementwise kernels do)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "gymrl.h"

int rl_set_error(const char* msg);  // rl_gae.hip

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 16;  // rows per workgroup: one MFMA tile

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float elu_f(float z) { return z > 0.f ? z : expm1f(z); }

struct InferLayers {
  const float* w[RL_INFER_MAX_LAYERS];
  const float* b[RL_INFER_MAX_LAYERS];
  int width[RL_INFER_MAX_LAYERS];
  int vec[RL_INFER_MAX_LAYERS];  // the layer's weight rows are 16-B aligned and a multiple of 4 long
  int count;
};

// four consecutive k of weight row `row` (k .. k + 3), zero past K
template <bool VEC>
__device__ __forceinline__ f4 wload(const float* __restrict__ w, int row, int k, int K) {
  const float* p = w + (size_t)row * K + k;
  if constexpr (VEC) {
    if (k < K) return *reinterpret_cast<const f4*>(p);  // K % 4 == 0: the chunk is whole or absent
    return f4{0.f, 0.f, 0.f, 0.f};
  } else {
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = k + j < K ? p[j] : 0.f;
    return v;
  }
}

// NB 16-column output blocks (nb0, nb0 + 4, ...) of one layer for this wave: out[r][c] = ELU(sum_k in[r][k] w[c][k] +
// b[c]).  Kp = K rounded up to 32 (the LDS columns K .. Kp are zero).  The reduction runs in chunks of 32: a lane
// holds 8 consecutive k of its weight row per block (32 contiguous bytes, the four quarters of the wave one 128-B
// line of the row), the next chunk's loads in flight while this one feeds 8 MFMAs per block.  In MFMA s of chunk c,
// quarter kq of the wave carries k = 32 c + 8 kq + s for both operands: every k is summed exactly once.
template <int NB, bool VEC>
__device__ __forceinline__ void layer_blocks(const float* __restrict__ in, float* __restrict__ out, int LD,
                                             const float* __restrict__ w, const float* __restrict__ bias, int K,
                                             int Kp, int nb0, int r, int kq) {
  f4 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
  const int chunks = Kp >> 5;
  f4 fw[NB][2], nw[NB][2];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int h = 0; h < 2; ++h) fw[j][h] = wload<VEC>(w, (nb0 + 4 * j) * 16 + r, 8 * kq + 4 * h, K);
  for (int c = 0; c < chunks; ++c) {
#pragma unroll
    for (int j = 0; j < NB; ++j)  // the next chunk's fragments (past K: zeros, nothing read)
#pragma unroll
      for (int h = 0; h < 2; ++h) nw[j][h] = wload<VEC>(w, (nb0 + 4 * j) * 16 + r, (c + 1) * 32 + 8 * kq + 4 * h, K);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f4 fa = *reinterpret_cast<const f4*>(in + r * LD + c * 32 + 8 * kq + 4 * h);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fw[j][h][q], fa[q], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) fw[j][h] = nw[j][h];
  }
  // registers 0 .. 3 of block j are columns 16 nb + 4 kq + (0..3) of row r
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = (nb0 + 4 * j) * 16 + 4 * kq;
    f4 ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = elu_f(acc[j][e] + bias[c + e]);
    *reinterpret_cast<f4*>(out + r * LD + c) = ov;
  }
}

template <bool VEC>
__device__ __forceinline__ void layer(const float* __restrict__ in, float* __restrict__ out, int LD,
                                      const float* __restrict__ w, const float* __restrict__ bias, int K, int Kp,
                                      int N, int wave, int r, int kq) {
  const int nblocks = N >> 4;
  int nb = wave;  // this wave's blocks: wave, wave + 4, ...
  int rem = nblocks > wave ? (nblocks - wave + 3) >> 2 : 0;
  while (rem >= 8) {
    layer_blocks<8, VEC>(in, out, LD, w, bias, K, Kp, nb, r, kq);
    nb += 32;
    rem -= 8;
  }
  if (rem >= 4) {
    layer_blocks<4, VEC>(in, out, LD, w, bias, K, Kp, nb, r, kq);
    nb += 16;
    rem -= 4;
  }
  if (rem >= 2) {
    layer_blocks<2, VEC>(in, out, LD, w, bias, K, Kp, nb, r, kq);
    nb += 8;
    rem -= 2;
  }
  if (rem >= 1) layer_blocks<1, VEC>(in, out, LD, w, bias, K, Kp, nb, r, kq);
}

__global__ __launch_bounds__(kThreads) void k_policy_infer(const float* __restrict__ obs, int N, int O,
                                                           const double* __restrict__ mean,
                                                           const double* __restrict__ var, float eps, InferLayers L,
                                                           const float* __restrict__ w_mu,
                                                           const float* __restrict__ b_mu, int A,
                                                           const float* __restrict__ noise,
                                                           const float* __restrict__ logstd, int clip, int LD,
                                                           float* __restrict__ actions, float* __restrict__ mu_out) {
  extern __shared__ float sm[];
  float* buf0 = sm;
  float* buf1 = sm + kRows * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const int r0 = blockIdx.x * kRows;
  const int nr = min(kRows, N - r0);
  // the input tile, normalised (running_mean_std.py eval forward, f32), zero past the rows and past obs_dim
  // one column per lane (Op <= 256 lanes): its moments read once, its 16 rows' loads independent of each other
  const int Op = (O + 31) & ~31;
  if (tid < Op) {
    const int k = tid;
    const bool live = k < O;
    float m = 0.f, sd = 1.f;
    if (mean && live) {
      m = (float)mean[k];
      sd = sqrtf((float)var[k] + eps);
    }
#pragma unroll 8
    for (int row = 0; row < kRows; ++row) {
      float v = 0.f;
      if (live && row < nr) {
        v = obs[(size_t)(r0 + row) * O + k];
        if (mean) {
          v = (v - m) / sd;
          v = fminf(fmaxf(v, -5.f), 5.f);
        }
      }
      buf0[row * LD + k] = v;
    }
  }
  __syncthreads();
  float* in = buf0;
  float* out = buf1;
  int K = O, Kp = Op;
  for (int l = 0; l < L.count; ++l) {
    const int W = L.width[l];
    if (L.vec[l]) layer<true>(in, out, LD, L.w[l], L.b[l], K, Kp, W, wave, r, kq);
    else layer<false>(in, out, LD, L.w[l], L.b[l], K, Kp, W, wave, r, kq);
    __syncthreads();
    float* t = in;
    in = out;
    out = t;
    K = Kp = W;
  }
  // the mu head from the last buffer and the action (rl_policy_head's statements): lane (row, action); four f32
  // FMA chains over k mod 4, added pairwise, as rl_act_heads (columns K .. Kp of `in` are zero when there is no layer)
  for (int t = tid; t < kRows * A; t += kThreads) {
    const int row = t & (kRows - 1), a = t >> 4;
    if (row >= nr) continue;
    const float* h = in + row * LD;
    const float* w = w_mu + (size_t)a * K;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 4 <= K; k += 4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fmaf(h[k + q], w[k + q], acc[q]);
    }
    for (; k < K; ++k) acc[k & 3] = fmaf(h[k], w[k], acc[k & 3]);
    const float m = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + b_mu[a];
    const size_t o = (size_t)(r0 + row) * A + a;
    float x = m;
    if (noise) {
      const float s = expf(logstd[a]);
      const float tt = noise[o] * s;
      x = tt + m;
    }
    if (clip) x = fminf(fmaxf(x, -1.f), 1.f);
    actions[o] = x;
    if (mu_out) mu_out[o] = m;
  }
}

int launch_fail(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  char msg[256];
  snprintf(msg, sizeof(msg), "%s: launch failed: %s", what, hipGetErrorString(e));
  return rl_set_error(msg) + 1;
}

}  // namespace

extern "C" int rl_policy_infer(const float* obs, int32_t num_envs, int32_t obs_dim, const double* mean,
                               const double* var, double eps, int32_t num_layers, const int32_t* widths,
                               const float* const* weights, const float* const* biases, const float* w_mu,
                               const float* b_mu, int32_t num_actions, const float* noise, const float* logstd,
                               int32_t clip, float* actions, float* mu, void* stream) {
  if (num_envs < 1) return rl_set_error("rl_policy_infer: num_envs must be >= 1");
  if (obs_dim < 1 || obs_dim > RL_INFER_MAX_OBS) return rl_set_error("rl_policy_infer: obs_dim must be in 1 .. 256");
  if (num_layers < 0 || num_layers > RL_INFER_MAX_LAYERS)
    return rl_set_error("rl_policy_infer: at most 4 hidden layers (num_layers in 0 .. 4)");
  if (num_actions < 1 || num_actions > RL_INFER_MAX_ACTIONS)
    return rl_set_error("rl_policy_infer: num_actions must be in 1 .. 32");
  if (!obs || !w_mu || !b_mu || !actions || (num_layers > 0 && (!widths || !weights || !biases)))
    return rl_set_error("rl_policy_infer: null required pointer (obs, weights, biases, w_mu, b_mu, actions)");
  if ((!mean) != (!var)) return rl_set_error("rl_policy_infer: mean and var must both be given or both be null");
  if (noise && !logstd) return rl_set_error("rl_policy_infer: null required pointer (logstd with noise)");
  InferLayers L{};
  L.count = num_layers;
  int K = obs_dim, maxw = (obs_dim + 31) & ~31;
  for (int l = 0; l < num_layers; ++l) {
    const int W = widths[l];
    if (W < 32 || W > RL_INFER_MAX_WIDTH || W % 32)
      return rl_set_error("rl_policy_infer: hidden widths must be multiples of 32 and at most 512");
    if (!weights[l] || !biases[l])
      return rl_set_error("rl_policy_infer: null required pointer (a layer's weight or bias)");
    L.w[l] = weights[l];
    L.b[l] = biases[l];
    L.width[l] = W;
    L.vec[l] = (K % 4 == 0) && (((uintptr_t)weights[l] & 15) == 0);
    if (W > maxw) maxw = W;
    K = W;
  }
  const int LD = maxw + 4;
  const size_t lds = sizeof(float) * 2 * (size_t)kRows * LD;  // <= 2 * 16 * 516 * 4 = 66048 B: two workgroups per CU
  if (lds > 64 * 1024) {
    // the opt-in for more than 64 KB of dynamic LDS; a refusal shows as the launch's own error below
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_policy_infer),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipGetLastError();
  }
  hipLaunchKernelGGL(k_policy_infer, dim3((num_envs + kRows - 1) / kRows), dim3(kThreads), lds, (hipStream_t)stream,
                     obs, (int)num_envs, (int)obs_dim, mean, var, (float)eps, L, w_mu, b_mu, (int)num_actions, noise,
                     logstd, (int)clip, LD, actions, mu);
  return launch_fail("rl_policy_infer");
}

// ---------------------------------------------------------------- the player's bookkeeping after env.step
// rl_games players.py BasePlayer.run, the loop body after env_step: cr += r; steps += 1; the done envs' episode
// reward / length added to the run's totals and games_played; the done envs' counters reset.  One workgroup of
// 1024 lanes.  Pass 1 is elementwise (lane = env mod 1024) and leaves each wave's done mask of its 64 consecutive
// envs in LDS; pass 2, wave 0 alone, walks the masks in env order and adds the done envs' values to the float64
// totals one by one (ascending env order, whatever N is), then zeroes their counters.  Once `finished` is set only
// the counters move.
namespace {

constexpr int kPlayLanes = 1024;
constexpr int kMaskSlots = 2048;  // 64-env done masks kept in LDS (131072 envs); beyond, pass 2 re-reads the flags

__device__ __forceinline__ bool flag(const void* p, int bytes, int i) {
  return bytes == 8 ? static_cast<const int64_t*>(p)[i] != 0 : static_cast<const uint8_t*>(p)[i] != 0;
}

__global__ __launch_bounds__(kPlayLanes) void k_play_post(const float* __restrict__ rew,
                                                          const void* __restrict__ dones, int dones_bytes, int N,
                                                          float* __restrict__ cur_rew, float* __restrict__ cur_steps,
                                                          double* __restrict__ sums, int64_t* __restrict__ games,
                                                          int64_t games_num) {
  __shared__ unsigned long long masks[kMaskSlots];
  const int t = threadIdx.x;
  const bool finished = games[1] != 0;  // read by every lane before lane 0 may set it (after the barrier)
  const int batches = (N + 63) >> 6;
  for (int base = 0; base < batches * 64; base += kPlayLanes) {
    const int i = base + t;
    bool d = false;
    if (i < N) {
      d = flag(dones, dones_bytes, i);
      const float cr = cur_rew[i] + rew[i];
      const float cs = cur_steps[i] + 1.f;
      const bool zero = d && finished;  // unfinished: pass 2 reads the done envs' values, then zeroes them
      cur_rew[i] = zero ? 0.f : cr;
      cur_steps[i] = zero ? 0.f : cs;
    }
    const unsigned long long m = __ballot(d);
    const int b = i >> 6;
    if ((t & 63) == 0 && b < batches && b < kMaskSlots) masks[b] = m;
  }
  if (finished) return;
  __syncthreads();
  if (t >= 64) return;
  double srew = sums[0], ssteps = sums[1];
  int64_t played = games[0];
  for (int b = 0; b < batches; ++b) {
    const int i = b * 64 + t;
    unsigned long long m;
    if (b < kMaskSlots) m = masks[b];
    else m = __ballot(i < N && flag(dones, dones_bytes, i));
    if (m == 0ull) continue;
    const bool mine = (m >> t) & 1ull;
    const float cr = mine ? cur_rew[i] : 0.f;
    const float cs = mine ? cur_steps[i] : 0.f;
    played += __popcll(m);
    while (m) {
      const int j = __ffsll((long long)m) - 1;
      srew += (double)__shfl(cr, j);
      ssteps += (double)__shfl(cs, j);
      m &= m - 1ull;
    }
    if (mine) {
      cur_rew[i] = 0.f;
      cur_steps[i] = 0.f;
    }
  }
  if (t == 0) {
    sums[0] = srew;
    sums[1] = ssteps;
    games[0] = played;
    if (played >= games_num) games[1] = 1;
  }
}

}  // namespace

extern "C" int rl_play_post(const float* rewards, const void* dones, int32_t dones_bytes, int32_t num_envs,
                            float* cur_rewards, float* cur_steps, double* sums, int64_t* games, int64_t games_num,
                            void* stream) {
  if (num_envs <= 0) return rl_set_error("rl_play_post: num_envs must be positive");
  if (!rewards || !dones || !cur_rewards || !cur_steps || !sums || !games)
    return rl_set_error("rl_play_post: null required pointer");
  if (dones_bytes != 1 && dones_bytes != 8)
    return rl_set_error("rl_play_post: dones must be 1-byte (bool / uint8) or 8-byte (int64) elements");
  hipLaunchKernelGGL(k_play_post, dim3(1), dim3(kPlayLanes), 0, (hipStream_t)stream, rewards, dones, (int)dones_bytes,
                     (int)num_envs, cur_rewards, cur_steps, sums, games, games_num);
  return launch_fail("rl_play_post");
}
