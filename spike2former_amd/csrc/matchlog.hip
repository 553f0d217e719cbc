// What the Hungarian assignment did, from inside the captured step (include/s2f.h "match log"; gfx950 only).  With the assignment on
// the device (lsa.hip) the tables tgt_labels / row_class / num_masks never reach the host; this file reads them back on the device,
// next to the costs the assignment saw and the class scores of the decoder, and appends one row of figures per replay to a ring the
// host reads once per log line: how many pairs were matched and at what cost, whether a matched query is also the cheapest of its
// class (greedy), whether the class changed hands since the decoder layer before (moved), whether matched queries classify their
// target (DETR's class_error), how many unmatched queries still claim an object, and which queries are never used.
//
//   s2f_match_log_partials  one workgroup of four waves per (layer l, image b).  row_class is sanitised into LDS (anything outside
//                           0 .. K-1 is -1 and is never used as an index); the class -> query tables of layers l and l-1 are built in
//                           LDS by atomicMin (an assignment names a class once; were it named twice, the lowest query owns it); the
//                           first arg-min of every owned class's cost column is found with lanes striped over the classes, so a
//                           wave's reads of a cost row are contiguous; the first arg-max of every query's K+1 class logits is one
//                           wave's butterfly; the five counts are ballots and popcounts into LDS integers; the cost is ONE thread's
//                           fp64 sum over the queries in ascending order.  int64 [6] per (l, b) and the last layer's int32 flags
//                           [B][Q] are stored plainly into the log's workspace.
//   s2f_match_log_rows      ONE workgroup: a thread per (layer, field) adds the B partials in ascending b (the cost in fp64, the
//                           others as integers) into row head[0] % window, a thread per query adds the flags into the row's usage
//                           words, moves the query's idle streak on and offers the latch; thread 0 stores head[0] + 1.  No ticket:
//                           nothing else runs in the launch and nothing waits for anything.
// Both launches only read cost, cls and row_class; every loop is bounded by L, B, Q or K.
#include "s2f_common.h"
#include "s2f_ring.h"

namespace {

typedef s2f_u64 u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / S2F_WAVE;
constexpr int kMaxQ = S2F_LSA_MAX_QUERIES;
constexpr int kMaxK = S2F_LSA_MAX_CLASSES;
constexpr int kMaxL = S2F_MATCH_LOG_MAX_LAYERS;
constexpr int kFields = S2F_MATCH_LOG_FIELDS;
constexpr int kNone = 0x7fffffff;          // an unowned class of the tables; larger than any query under atomicMin
enum { MATCHED = 0, COST = 1, GREEDY = 2, MOVED = 3, CLS_HIT = 4, UNMATCHED_OBJ = 5 };
static_assert(kMaxQ <= 256 && kMaxK < 256 && kFields == 6, "the LDS tables below");

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// cost fp32 [L][B][Q][K], cls fp32 [L][B][Q][K+1], row_class int32 [B][L*Q]; partials int64 [L][B][6], usage int32 [B][Q]
__global__ __launch_bounds__(kThreads) void match_log_partials_kernel(const float* __restrict__ cost, const float* __restrict__ cls,
                                                                      const int* __restrict__ row_class, int L, int B, int Q, int K,
                                                                      long long* __restrict__ partials, int* __restrict__ usage) {
  __shared__ int owner[kMaxK];          // class -> the query it is matched to in layer l (kNone: none)
  __shared__ int before[kMaxK];         // ... in layer l - 1
  __shared__ int cheapest[kMaxK];       // class -> the first arg-min of its cost column (owned classes only)
  __shared__ int klass[kMaxQ];          // query -> its class, -1 for ANY value outside 0 .. K-1
  __shared__ int top[kMaxQ];            // query -> the first arg-max of its K+1 logits
  __shared__ float paid[kMaxQ];         // query -> cost[q][klass[q]]
  __shared__ int count[kFields];
  __shared__ double total;
  const int tid = threadIdx.x, lane = tid % S2F_WAVE, wave = tid / S2F_WAVE;
  const int b = blockIdx.x, l = blockIdx.y;
  const int* __restrict__ rows = row_class + ((size_t)b * L + l) * Q;          // (layer l - 1: Q words before)
  const float* __restrict__ cst = cost + ((size_t)l * B + b) * Q * (size_t)K;
  const float* __restrict__ logit = cls + ((size_t)l * B + b) * Q * (size_t)(K + 1);
  for (int c = tid; c < K; c += kThreads) owner[c] = before[c] = kNone;
  if (tid < kFields) count[tid] = 0;
  __syncthreads();
  for (int q0 = 0; q0 < Q; q0 += kThreads) {          // (every thread runs every trip: the ballots are whole)
    const int q = q0 + tid;
    const bool in = q < Q;
    const int c = in ? rows[q] : -1;
    const bool m = in && c >= 0 && c < K;
    if (in) {
      klass[q] = m ? c : -1;
      paid[q] = m ? cst[(size_t)q * K + c] : 0.f;
      if (l == L - 1) usage[(size_t)b * Q + q] = m ? 1 : 0;
    }
    if (m) atomicMin(&owner[c], q);
    if (in && l > 0) {
      const int p = rows[q - Q];
      if (p >= 0 && p < K) atomicMin(&before[p], q);
    }
    const int n = wave_count(m);
    if (lane == 0 && n) atomicAdd(&count[MATCHED], n);
  }
  __syncthreads();
  // column arg-mins: lane = class, the queries in ascending order, strict <
  for (int c = tid; c < K; c += kThreads) {
    int at = -1;
    if (owner[c] != kNone) {
      float best = cst[c];
      at = 0;
#pragma unroll 8
      for (int q = 1; q < Q; ++q) {
        const float v = cst[(size_t)q * K + c];
        if (v < best) {
          best = v;
          at = q;
        }
      }
    }
    cheapest[c] = at;
  }
  // row arg-maxes: a wave per query.  The serial rule -- best = x[0], then strict > -- lets a NaN at index 0 stand and skips every
  // other NaN; striped over lanes that is: NaN counts as -inf, the largest value's lowest index wins, and a NaN x[0] answers 0.
  for (int q = wave; q < Q; q += kWaves) {
    const float* __restrict__ x = logit + (size_t)q * (K + 1);
    float bv = -INFINITY;
    int bi = kNone;
    for (int k = lane; k <= K; k += S2F_WAVE) {
      float v = x[k];
      v = v != v ? -INFINITY : v;
      if (bi == kNone || v > bv) {
        bv = v;
        bi = k;
      }
    }
#pragma unroll
    for (int s = S2F_WAVE / 2; s >= 1; s >>= 1) {
      const float ov = __shfl_xor(bv, s, S2F_WAVE);
      const int oi = __shfl_xor(bi, s, S2F_WAVE);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      const float first = x[0];
      top[q] = first != first ? 0 : bi;
    }
  }
  __syncthreads();
  for (int q0 = 0; q0 < Q; q0 += kThreads) {
    const int q = q0 + tid;
    const bool in = q < Q;
    const int c = in ? klass[q] : -1;
    const int a = in ? top[q] : K;
    const bool m = c >= 0;
    const int greedy = wave_count(m && cheapest[m ? c : 0] == q);
    const int moved = wave_count(m && l > 0 && before[m ? c : 0] != q);
    const int hit = wave_count(m && a == c);
    const int claims = wave_count(in && !m && a != K);
    if (lane == 0) {
      if (greedy) atomicAdd(&count[GREEDY], greedy);
      if (moved) atomicAdd(&count[MOVED], moved);
      if (hit) atomicAdd(&count[CLS_HIT], hit);
      if (claims) atomicAdd(&count[UNMATCHED_OBJ], claims);
    }
  }
  if (tid == 0) {          // the prescribed order: one serial fp64 sum, q ascending
    double s = 0.0;
    for (int q = 0; q < Q; ++q)
      if (klass[q] >= 0) s += (double)paid[q];
    total = s;
  }
  __syncthreads();
  if (tid < kFields)
    partials[((size_t)l * B + b) * kFields + tid] = tid == COST ? __double_as_longlong(total) : (long long)count[tid];
}

// partials int64 [L][B][6], usage int32 [B][Q]; ring int64 [window][6L + ceil(Q/2)], idle int32 [Q]
__global__ __launch_bounds__(kThreads) void match_log_rows_kernel(const long long* __restrict__ partials, const int* __restrict__ usage,
                                                                  int L, int B, int Q, long long* __restrict__ ring, int window,
                                                                  int* __restrict__ idle, int patience, u64* head) {
  const int tid = threadIdx.x;
  const int pad = (Q + 1) / 2;
  const u64 row = s2f_ring_row(head);
  long long* __restrict__ out = ring + (long long)(row % (u64)window) * (kFields * L + pad);
  for (int i = tid; i < kFields * L; i += kThreads) {
    const long long* __restrict__ src = partials + (size_t)(i / kFields) * B * kFields + i % kFields;
    if (i % kFields == COST) {
      double s = 0.0;
      for (int b = 0; b < B; ++b) s += __longlong_as_double(src[(size_t)b * kFields]);          // b ascending
      out[i] = __double_as_longlong(s);
    } else {
      long long a = 0;
      for (int b = 0; b < B; ++b) a += src[(size_t)b * kFields];
      out[i] = a;
    }
  }
  int* __restrict__ used = reinterpret_cast<int*>(out + kFields * L);
  for (int q = tid; q < 2 * pad; q += kThreads) {
    int u = 0;
    if (q < Q) {
      for (int b = 0; b < B; ++b) u += usage[(size_t)b * Q + q] != 0;
      const int was = idle[q];
      const int s = u > 0 ? 0 : was + (was < kNone);
      idle[q] = s;
      if (u == 0 && s == patience && was != s) s2f_ring_offer(head, 1, s2f_ring_event(row, q));
    }
    used[q] = u;          // (the padding word of an odd Q: 0)
  }
  __syncthreads();
  if (tid == 0) __hip_atomic_store(head, row + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

inline bool shape_ok(int L, int B, int Q) { return L >= 1 && L <= kMaxL && B >= 1 && B <= 65535 && Q >= 1 && Q <= kMaxQ; }

}  // namespace

extern "C" int s2f_match_log_partials(const float* cost, const float* cls, const int32_t* row_class, int L, int B, int Q, int K,
                                      int64_t* partials, int32_t* usage, void* stream) {
  S2F_REQUIRE(cost && cls && row_class && partials && usage, S2F_EINVAL, "s2f_match_log_partials: null pointer");
  S2F_REQUIRE(shape_ok(L, B, Q), S2F_EINVAL, "s2f_match_log_partials: L %d outside 1 .. %d, B %d outside 1 .. 65535 or Q %d outside 1 .. %d",
              L, kMaxL, B, Q, kMaxQ);
  S2F_REQUIRE(K >= 1 && K <= kMaxK, S2F_EINVAL, "s2f_match_log_partials: K %d outside 1 .. %d", K, kMaxK);
  S2F_REQUIRE(aligned(cost, 4) && aligned(cls, 4) && aligned(row_class, 4) && aligned(usage, 4) && aligned(partials, 8), S2F_EALIGN,
              "s2f_match_log_partials: partials must be 8-byte aligned, cost, cls, row_class and usage 4-byte");
  hipLaunchKernelGGL(match_log_partials_kernel, dim3((unsigned)B, (unsigned)L), dim3(kThreads), 0, (hipStream_t)stream, cost, cls,
                     row_class, L, B, Q, K, reinterpret_cast<long long*>(partials), usage);
  return s2f_check_launch("s2f_match_log_partials");
}

extern "C" int s2f_match_log_rows(const int64_t* partials, const int32_t* usage, int L, int B, int Q, int64_t* ring, int window,
                                  int32_t* idle, int patience, int64_t* head, void* stream) {
  S2F_REQUIRE(partials && usage && ring && idle && head, S2F_EINVAL, "s2f_match_log_rows: null pointer");
  S2F_REQUIRE(shape_ok(L, B, Q), S2F_EINVAL, "s2f_match_log_rows: L %d outside 1 .. %d, B %d outside 1 .. 65535 or Q %d outside 1 .. %d", L,
              kMaxL, B, Q, kMaxQ);
  S2F_REQUIRE(window >= 1, S2F_EINVAL, "s2f_match_log_rows: window %d below 1", window);
  S2F_REQUIRE(patience >= 1, S2F_EINVAL, "s2f_match_log_rows: patience %d below 1", patience);
  S2F_REQUIRE(aligned(partials, 8) && aligned(ring, 8) && aligned(head, 8) && aligned(usage, 4) && aligned(idle, 4), S2F_EALIGN,
              "s2f_match_log_rows: partials, ring and head must be 8-byte aligned, usage and idle 4-byte");
  hipLaunchKernelGGL(match_log_rows_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(partials), usage, L, B, Q, reinterpret_cast<long long*>(ring), window, idle,
                     patience, reinterpret_cast<u64*>(head));
  return s2f_check_launch("s2f_match_log_rows");
}
