// Per-neuron firing rows from inside the captured training step (include/s2f.h "firing log"; gfx950 only).  Every neuron kernel of
// the package adds {sum of counts, number of non-zero counts} into the 256 contention slots of its neuron's `stats`; this file is
// the path from those counters to a log the host reads once per interval.
//
//   s2f_firing_log_append  ONE launch, one wave per neuron.  The wave loads its neuron's 256 slots (each lane four slots, one
//                          16-byte load per slot: a slot IS a {sum, nonzero} pair), adds them up as 64-bit integers, stores the
//                          pair into row head[0] % window of the ring, clears the 512 counter words with 16-byte stores and moves
//                          the neuron's silent streak on.  A streak that REACHES `patience` is offered to the latch head[1], and
//                          head[0] advances once per launch, by the head protocol of s2f_ring.h.
#include "s2f_common.h"
#include "s2f_ring.h"

namespace {

constexpr int kSlotsPerLane = S2F_STAT_SLOTS / S2F_WAVE;
static_assert(kSlotsPerLane * S2F_WAVE == S2F_STAT_SLOTS, "a wave covers the slots in whole rounds");

typedef s2f_u64 u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
  // (__shfl_xor moves a 64-bit value as two 32-bit halves and hands the whole value back: the ADD below is a 64-bit one, so a
  // carry out of the low half reaches the high half)
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S2F_WAVE);
  return v;
}

__global__ __launch_bounds__(S2F_WAVE) void firing_log_append_kernel(u64* __restrict__ counters, int n, long long* __restrict__ ring,
                                                                     int window, int* __restrict__ silent, int patience, u64* head) {
  const int i = blockIdx.x;          // (the grid is n workgroups of one wave)
  const int lane = threadIdx.x;
  const u64 row = s2f_ring_row(head);
  ulonglong2* __restrict__ slots = reinterpret_cast<ulonglong2*>(counters + (size_t)i * (2 * S2F_STAT_SLOTS));
  u64 sum = 0, nonzero = 0;
#pragma unroll
  for (int k = 0; k < kSlotsPerLane; ++k) {
    const ulonglong2 s = slots[k * S2F_WAVE + lane];
    sum += s.x;
    nonzero += s.y;
  }
#pragma unroll
  for (int k = 0; k < kSlotsPerLane; ++k) slots[k * S2F_WAVE + lane] = make_ulonglong2(0, 0);
  sum = wave_sum_u64(sum);
  nonzero = wave_sum_u64(nonzero);
  if (lane == 0) {
    long long* out = ring + ((long long)(row % (u64)window) * n + i) * 2;
    out[0] = (long long)sum;
    out[1] = (long long)nonzero;
    int s = silent[i];
    if (s != -1) {          // -1: a neuron the step never runs is not watched
      s = sum == 0 ? s + 1 : 0;
      silent[i] = s;
      if (s == patience) s2f_ring_offer(head, 1, s2f_ring_event(row, i));
    }
    s2f_ring_commit(head, row, n);
  }
}

}  // namespace

extern "C" int s2f_firing_log_append(uint64_t* counters, int n, int64_t* ring, int window, int32_t* silent, int patience, int64_t* head,
                                     void* stream) {
  S2F_REQUIRE(counters && ring && silent && head, S2F_EINVAL, "s2f_firing_log_append: null pointer");
  S2F_REQUIRE(n >= 1, S2F_EINVAL, "s2f_firing_log_append: n %d below 1", n);
  S2F_REQUIRE(window >= 1, S2F_EINVAL, "s2f_firing_log_append: window %d below 1", window);
  S2F_REQUIRE(patience >= 1, S2F_EINVAL, "s2f_firing_log_append: patience %d below 1", patience);
  S2F_REQUIRE(s2f_aligned16(counters) && (reinterpret_cast<uintptr_t>(ring) & 7u) == 0 && (reinterpret_cast<uintptr_t>(head) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(silent) & 3u) == 0,
              S2F_EALIGN, "s2f_firing_log_append: counters must be 16-byte aligned, ring and head 8-byte, silent 4-byte");
  hipLaunchKernelGGL(firing_log_append_kernel, dim3((unsigned)n), dim3(S2F_WAVE), 0, (hipStream_t)stream,
                     reinterpret_cast<u64*>(counters), n, reinterpret_cast<long long*>(ring), window, silent, patience,
                     reinterpret_cast<u64*>(head));
  return s2f_check_launch("s2f_firing_log_append");
}
