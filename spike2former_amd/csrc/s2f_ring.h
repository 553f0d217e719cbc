// The head of a device ring whose row is appended by a launch of SEVERAL workgroups (firinglog.hip, gradlog.hip; the host side is
// spike2former_amd/devring.py): four 64-bit words, [0] the rows appended so far -- the launch writes row head[0] % window -- [1] and
// [3] latches, [2] the launch's ticket word (0 between launches).  head[0] advances once per launch: every workgroup reads the row
// index at entry (s2f_ring_row) -- before it takes a ticket from head[2] -- and the workgroup that draws the last ticket, when every
// other has read its row index, stores head[0] + 1 and puts the ticket word back to 0 (s2f_ring_commit).  No workgroup waits for
// another.  An event is offered to a latch by an unsigned 64-bit atomicMin of row * 2^32 + index (s2f_ring_event, s2f_ring_offer):
// the earliest row's lowest index wins in whatever order the workgroups finish, and -1 (all ones: the largest unsigned value) means
// none.  The words of `head` are touched by agent-scope atomics only: nothing of them lives in a CU's L1.
#pragma once

typedef unsigned long long s2f_u64;

__device__ __forceinline__ s2f_u64 s2f_ring_row(const s2f_u64* head) { return __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ s2f_u64 s2f_ring_event(s2f_u64 row, int i) { return (row << 32) | (s2f_u64)(unsigned)i; }
__device__ __forceinline__ void s2f_ring_offer(s2f_u64* head, int k, s2f_u64 event) { atomicMin(head + k, event); }

// one thread per workgroup, `n` workgroups, each behind its own s2f_ring_row, row stores and offers
__device__ __forceinline__ void s2f_ring_commit(s2f_u64* head, s2f_u64 row, int n) {
  // The row index was read before this add: whoever draws the last ticket knows that every workgroup holds its own.
  const s2f_u64 ticket = atomicAdd(head + 2, 1ull);
  if (ticket == (s2f_u64)(n - 1)) {
    __hip_atomic_store(head + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(head, row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
