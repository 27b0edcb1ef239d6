// gt_wave.h -- the done-count protocol of libgymtask's post-physics kernels and the rank of a flagged env in their
// fused resets, one implementation for every task ("The done count"):
//   1. a post-physics kernel ballots its done mask per wave and stores the 64-bit word in reset_masks;
//   2. one lane per wave joins the grid-wide {waves done << 32 | count} accumulator, and the wave that completes the
//      grid publishes {count, seq} as ONE 8-byte store into pinned host memory, where the host spin-waits on it;
//   3. the fused reset ranks a flagged env by the exclusive prefix of the earlier waves' popcounts, so env_ids_out is
//      in torch.nonzero order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gt_wave {

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The done count of one wave (popc envs flagged) joins the launch's total: one 64-bit atomic per wave carries
// {waves done << 32 | count} in reset_count[0:2]; the wave that completes the grid (nwaves waves) publishes the total
// (device word reset_count[2], and {count, seq} into host memory for the host's spin wait) and re-arms the
// accumulator: every other wave's add has returned, so a plain store does.  Called by one lane per wave.  b: the
// task's buffers struct (its reset_count, host_count, seq), by reference: only the publishing wave reads the last two.
template <class B>
__device__ __forceinline__ void publish_done_count(const B& b, unsigned popc, unsigned nwaves) {
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(b.reset_count);
  const unsigned long long add = (1ull << 32) | (unsigned long long)popc;
  const unsigned long long old = atomicAdd(acc, add);
  if ((unsigned)(old >> 32) == nwaves - 1) {
    const int total = (int)((old + add) & 0xffffffffull);
    *acc = 0ull;
    b.reset_count[2] = total;
    if (b.host_count) {
      // {count, seq} as ONE 8-byte store: the host reads only this word, so no release fence
      // (a system-scope release writes back the whole L2, microseconds at the end of the tail)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(b.host_count),
                         ((unsigned long long)(uint32_t)b.seq << 32) | (uint32_t)total, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// One lane per env, called by every lane of the grid (whole waves) with the task's buffers struct B (its reset_masks,
// reset_count, host_count and seq): the ballot of `done` goes to word `wave` of reset_masks (when given) and its
// popcount joins the done count of the grid's nwaves waves.  Returns the ballot.  The caller derives wave and nwaves
// from its own reads of the launch geometry: a second blockDim.x read in here is not merged with the kernel's.
template <class B>
__device__ __forceinline__ unsigned long long record_done(const B& b, bool done, unsigned wave, unsigned nwaves) {
  const unsigned long long m = __ballot(done);
  if ((threadIdx.x & 63) == 0) {
    if (b.reset_masks) b.reset_masks[wave] = m;
    publish_done_count(b, (unsigned)__popcll(m), nwaves);
  }
  return m;
}

// A fused reset's wave `wave` (64 lanes, all calling): base = the envs flagged in the earlier waves, 64 mask words
// per pass; returns this wave's mask word.  Flagged lane l has rank base + popcount(word & ((1 << l) - 1)).
__device__ __forceinline__ unsigned long long flagged_rank(const uint64_t* reset_masks, int wave, int lane,
                                                           int& base) {
  base = 0;
  for (int c = 0; c < wave; c += 64) {
    const int i = c + lane;
    base += wave_sum(i < wave ? (int)__popcll(reset_masks[i]) : 0);
  }
  return reset_masks[wave];
}

}  // namespace gt_wave
