// What a training LOOP owes the captured step besides the step itself (include/s2f.h "training loop"; gfx950 only): a record of
// every iteration's scalars that the host reads once per log interval, and a one-launch copy of the whole training state into a
// staging buffer that the next replay may overtake.  Both are plain streaming launches: no allocation, no synchronisation, no
// atomics -- capturable, and ordered by the stream they are queued on.
//
//   s2f_state_copy         chunk table -> every chunk of <= 4 096 32-bit WORDS of one tensor, tensor -> flat (to_params = 0) or
//                          flat -> tensor (to_params = 1).  The tables have the shapes of s2f_adamw_step (csrc/optim.hip): the
//                          tensors stay where their modules own them, behind a pointer table.  The kernel moves bits and knows
//                          no dtype: an fp32 weight, an fp32 running statistic and an int64 counter (two words per element) are
//                          slots of one launch.  16-byte accesses where BOTH addresses of a chunk are 16-byte aligned (a slot of
//                          `flat` is; a tensor's storage usually is, but sibling weights that ops.flatten_together keeps adjacent
//                          in one storage start at 4-byte-aligned addresses only), word accesses otherwise and on a chunk's last,
//                          partial group.  Words of `flat` outside the slots are never written.  HBM-bound: 8 B per word.
//   s2f_train_log_append   ONE wave: row head[0] % window of the ring <- the n scalars behind a device table of pointers, a
//                          non-finite value in any of them latches head[1] (once: the first such row survives the ring's wrap),
//                          head[0] += 1.  Nothing else writes `head`, and appends are ordered by their stream, so the row index
//                          needs no atomic.
#include "s2f_common.h"

namespace {

constexpr int kStateChunk = 4096;          // words per workgroup: 256 threads x 4 groups of 4 words (= s2f_adamw_chunk_elems())

// slots  int64 [nslots][3] = {tensor pointer, offset of the slot in flat (words), length (words)}
// chunks int32 [nchunks][2] = {slot, first word inside the slot}
template <bool kToParams>
__global__ __launch_bounds__(256) void state_copy_kernel(const long long* __restrict__ slots, const int* __restrict__ chunks,
                                                         uint32_t* __restrict__ flat) {
  const int slot = chunks[2 * blockIdx.x];
  const long long start = chunks[2 * blockIdx.x + 1];
  uint32_t* __restrict__ p = reinterpret_cast<uint32_t*>(slots[3 * slot]) + start;
  uint32_t* __restrict__ f = flat + slots[3 * slot + 1] + start;
  const long long len = slots[3 * slot + 2] - start;          // words of the slot from this chunk on
  const int cnt = (int)(len < kStateChunk ? len : kStateChunk);          // (<= 0: a malformed chunk copies nothing)
  const bool vec = (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(f)) & 15u) == 0);
  const uint32_t* __restrict__ src = kToParams ? f : p;
  uint32_t* __restrict__ dst = kToParams ? p : f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = (i * 256 + (int)threadIdx.x) * 4;
    if (e >= cnt) break;
    if (vec && e + 4 <= cnt) {
      *reinterpret_cast<uint4*>(dst + e) = *reinterpret_cast<const uint4*>(src + e);
    } else {
      const int m = min(4, cnt - e);
      for (int k = 0; k < m; ++k) dst[e + k] = src[e + k];
    }
  }
}

constexpr int kLogLanes = S2F_WAVE;

__global__ __launch_bounds__(kLogLanes) void train_log_append_kernel(const float* const* __restrict__ srcs, int n, float* __restrict__ ring,
                                                                      int window, int stride, long long* __restrict__ head) {
  const long long count = head[0];          // every lane reads it before lane 0 advances it (one wave, and the barrier below)
  float* __restrict__ row = ring + (count % window) * (long long)stride;
  int bad = 0;
  for (int i = threadIdx.x; i < n; i += kLogLanes) {
    const float v = *srcs[i];
    row[i] = v;
    bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;          // inf or NaN: an all-ones exponent
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    if (bad && head[1] < 0) head[1] = count;
    head[0] = count + 1;
  }
}

}  // namespace

extern "C" int s2f_state_copy(const int64_t* slots, const int32_t* chunks, int nchunks, void* flat, int to_params, void* stream) {
  S2F_REQUIRE(slots && chunks && flat, S2F_EINVAL, "s2f_state_copy: null pointer");
  S2F_REQUIRE(nchunks > 0, S2F_EINVAL, "s2f_state_copy: no chunks");
  S2F_REQUIRE(to_params == 0 || to_params == 1, S2F_EINVAL, "s2f_state_copy: to_params %d is neither 0 nor 1", to_params);
  S2F_REQUIRE(s2f_aligned16(flat), S2F_EALIGN, "s2f_state_copy: the flat buffer must be 16-byte aligned");
  static_assert(kStateChunk == 256 * 4 * 4, "a chunk is what one workgroup copies");
  const long long* sl = reinterpret_cast<const long long*>(slots);
  uint32_t* fl = static_cast<uint32_t*>(flat);
  if (to_params)
    S2F_LAUNCH(true, true, state_copy_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, sl, chunks, fl);
  else
    S2F_LAUNCH(true, true, state_copy_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, sl, chunks, fl);
  return s2f_check_launch("s2f_state_copy");
}

extern "C" int s2f_train_log_append(const float* const* srcs, int n, float* ring, int window, int stride, int64_t* head, void* stream) {
  S2F_REQUIRE(srcs && ring && head, S2F_EINVAL, "s2f_train_log_append: null pointer");
  S2F_REQUIRE(n >= 1 && n <= S2F_TRAIN_LOG_MAX_TERMS, S2F_EINVAL, "s2f_train_log_append: n %d outside 1 .. %d", n, S2F_TRAIN_LOG_MAX_TERMS);
  S2F_REQUIRE(stride >= n, S2F_EINVAL, "s2f_train_log_append: stride %d below n %d", stride, n);
  S2F_REQUIRE(window >= 1, S2F_EINVAL, "s2f_train_log_append: window %d below 1", window);
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(srcs) & 7u) == 0 && (reinterpret_cast<uintptr_t>(head) & 7u) == 0 &&
                  (reinterpret_cast<uintptr_t>(ring) & 3u) == 0,
              S2F_EALIGN, "s2f_train_log_append: srcs and head must be 8-byte aligned, ring 4-byte aligned");
  hipLaunchKernelGGL(train_log_append_kernel, dim3(1), dim3(kLogLanes), 0, (hipStream_t)stream, srcs, n, ring, window, stride,
                     reinterpret_cast<long long*>(head));
  return s2f_check_launch("s2f_train_log_append");
}
