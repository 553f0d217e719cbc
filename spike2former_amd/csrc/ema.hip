// An exponential moving average of the weights, kept on the device behind the optimizer's update (include/s2f.h "weight averaging";
// gfx950 only) -- what mmengine's EMAHook + ExponentialMovingAverage / ExpMomentumEMA do with one lerp_ per parameter tensor and
// iteration, as ONE table-driven launch that the step's hipGraph holds:
//
//   s2f_ema_update   chunk table -> every chunk of <= 4 096 elements of one parameter: the slot of `ema` <- copy of, or lerp towards,
//                    the parameter.  Every workgroup reads the optimizer's update count state[4] and derives the same decision:
//                        c = t - max(begin, 1)      (the started updates before this one; t = state[4], this update, from 1)
//                        c <= 0                     e = p, bit for bit
//                        c % interval != 0          nothing is read or written
//                        otherwise                  m = table[min(c, ntable - 1)];  e = fl(e + fl(m * fl(p - e)))
//                    and, where `partials` is given, the chunk's fp64 sums {(p - e)^2, e^2} over the values just written.
//   s2f_ema_swap     parameter <-> its slot of `ema`, bits: validation runs on the average, and the weights come back unchanged.
//
// Pure streaming, 12 B per element for the update (read p, read e, write e; 8 B in its copy form), 16 B for the swap: one workgroup
// of 256 threads per chunk (the tables are s2f_adamw_step's), every thread's four 16-byte loads of BOTH streams are issued before the
// first use, so a wave has 8 KiB in flight; the update takes 48 VGPRs with `partials` (and 4 KiB of LDS), 44 without, the swap 76,
// none uses scratch: 8 / 8 / 6 waves per SIMD, i.e. as many workgroups per CU.  A parameter may start at a 4-byte-aligned address only
// (sibling weights that share one storage): such a chunk, and every chunk's last partial group, goes word by word.
#include "s2f_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kEmaChunk = 4096;          // elements per workgroup: 256 threads x 4 groups of 4 (= s2f_adamw_chunk_elems())
constexpr uint32_t kQuietNaN = 0x7fc00000u;

struct Chunk {
  uint32_t* p;          // the parameter, from this chunk's first element on
  uint32_t* e;          // its slot of `ema`, likewise
  int cnt;              // elements of this chunk (<= 0: a malformed chunk touches nothing)
  bool vec;             // both addresses 16-byte aligned
};

// slots  int64 [nslots][3] = {parameter pointer, offset of the slot in ema (elements, % 4 == 0), numel}
// chunks int32 [nchunks][2] = {slot, first element inside the slot}
__device__ __forceinline__ Chunk chunk_of(const long long* __restrict__ slots, const int* __restrict__ chunks, uint32_t* ema) {
  const int slot = chunks[2 * blockIdx.x];
  const long long start = chunks[2 * blockIdx.x + 1];
  Chunk c;
  c.p = reinterpret_cast<uint32_t*>(slots[3 * slot]) + start;
  c.e = ema + slots[3 * slot + 1] + start;
  const long long len = slots[3 * slot + 2] - start;
  c.cnt = (int)(len < kEmaChunk ? len : kEmaChunk);
  c.vec = (((reinterpret_cast<uintptr_t>(c.p) | reinterpret_cast<uintptr_t>(c.e)) & 15u) == 0);
  return c;
}

// one thread's share of a chunk: group i = elements [(i * 256 + tid) * 4, + 4); loads first, all of them, then `op` per element, then
// the stores.  op(p, e) -> the new bits of both (kStoreP: the parameter is written too).  `load_e` (uniform over the grid): false
// where op overwrites the average without looking at it -- the copy form then moves 8 B per element, not 12.
template <bool kStoreP, class Op>
__device__ __forceinline__ void stream_chunk(const Chunk& c, bool load_e, Op op) {
  uint32_t pv[4][4], ev[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int at = (i * 256 + (int)threadIdx.x) * 4;
    if (c.vec && at + 4 <= c.cnt) {
      const uint4 a = *reinterpret_cast<const uint4*>(c.p + at);
      const uint4 b = load_e ? *reinterpret_cast<const uint4*>(c.e + at) : make_uint4(0u, 0u, 0u, 0u);
      pv[i][0] = a.x, pv[i][1] = a.y, pv[i][2] = a.z, pv[i][3] = a.w;
      ev[i][0] = b.x, ev[i][1] = b.y, ev[i][2] = b.z, ev[i][3] = b.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = at + k < c.cnt;
        pv[i][k] = ok ? c.p[at + k] : 0u;
        ev[i][k] = ok && load_e ? c.e[at + k] : 0u;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int at = (i * 256 + (int)threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (at + k < c.cnt) op(pv[i][k], ev[i][k]);
    if (c.vec && at + 4 <= c.cnt) {
      *reinterpret_cast<uint4*>(c.e + at) = make_uint4(ev[i][0], ev[i][1], ev[i][2], ev[i][3]);
      if (kStoreP) *reinterpret_cast<uint4*>(c.p + at) = make_uint4(pv[i][0], pv[i][1], pv[i][2], pv[i][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (at + k < c.cnt) {
          c.e[at + k] = ev[i][k];
          if (kStoreP) c.p[at + k] = pv[i][k];
        }
    }
  }
}

// the workgroup's 256 pairs of fp64 sums -> part[0 .. 1], by a tree of fixed shape (bit-repeatable; a plain store)
__device__ __forceinline__ void drift_tree(double d2, double e2, double* __restrict__ part) {
  __shared__ double red[2][256];
  red[0][threadIdx.x] = d2;
  red[1][threadIdx.x] = e2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) part[0] = red[0][0], part[1] = red[1][0];
}

template <bool kPartials>
__global__ __launch_bounds__(256) void ema_update_kernel(const long long* __restrict__ slots, const int* __restrict__ chunks,
                                                         uint32_t* ema, const float* __restrict__ state,
                                                         const float* __restrict__ table, int ntable, int begin, int interval,
                                                         double* __restrict__ partials) {
  // the same three words in every workgroup: the decision is uniform over the grid
  const int c = (int)state[4] - (begin > 1 ? begin : 1);
  if (c > 0 && c % interval != 0) return;          // a started update that `interval` skips: ema and partials stay as they were
  const bool copy = c <= 0;
  const float m = copy ? 0.f : table[c < ntable ? c : ntable - 1];
  const Chunk ch = chunk_of(slots, chunks, ema);
  double d2 = 0.0, e2 = 0.0;
  stream_chunk<false>(ch, !copy, [&](uint32_t& pb, uint32_t& eb) {
    if (copy) {
      eb = pb;
    } else {
      const float p = __uint_as_float(pb), e = __uint_as_float(eb);
      // plain operators under `fp contract(off)`: v_sub_f32, v_mul_f32, v_add_f32.  (__fsub_rn / __fmul_rn / __fadd_rn are inline
      // functions of the HIP headers that carry the HEADERS' contraction setting: written with them, the product and the sum
      // came out as one v_fmac_f32.)
      const float d = p - e;
      const float q = m * d;
      const float r = e + q;
      eb = r != r ? kQuietNaN : __float_as_uint(r);          // ONE NaN, whatever the operands' payloads were (include/s2f.h)
    }
    if (kPartials) {
      const double e = (double)__uint_as_float(eb), d = (double)__uint_as_float(pb) - e;
      d2 += d * d;
      e2 += e * e;
    }
  });
  if (kPartials) drift_tree(d2, e2, partials + 2 * (long long)blockIdx.x);
}

__global__ __launch_bounds__(256) void ema_swap_kernel(const long long* __restrict__ slots, const int* __restrict__ chunks, uint32_t* ema) {
  const Chunk ch = chunk_of(slots, chunks, ema);
  stream_chunk<true>(ch, true, [](uint32_t& pb, uint32_t& eb) {
    const uint32_t t = pb;
    pb = eb;
    eb = t;
  });
}

}  // namespace

extern "C" int s2f_ema_update(const int64_t* slots, const int32_t* chunks, int nchunks, float* ema, const float* state,
                              const float* table, int ntable, int begin, int interval, double* partials, void* stream) {
  S2F_REQUIRE(slots && chunks && ema && state && table, S2F_EINVAL, "s2f_ema_update: null pointer");
  S2F_REQUIRE(nchunks > 0, S2F_EINVAL, "s2f_ema_update: no chunks");
  S2F_REQUIRE(ntable >= 1, S2F_EINVAL, "s2f_ema_update: the momentum table has no entry");
  S2F_REQUIRE(begin >= 0 && interval >= 1, S2F_EINVAL, "s2f_ema_update: begin %d below 0 or interval %d below 1", begin, interval);
  S2F_REQUIRE(s2f_aligned16(ema), S2F_EALIGN, "s2f_ema_update: the ema buffer must be 16-byte aligned");
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0, S2F_EALIGN, "s2f_ema_update: partials must be 8-byte aligned");
  S2F_REQUIRE(s2f_adamw_chunk_elems() == kEmaChunk, S2F_EINVAL, "s2f_ema_update: built for chunks of %d elements", kEmaChunk);
  const long long* sl = reinterpret_cast<const long long*>(slots);
  uint32_t* em = reinterpret_cast<uint32_t*>(ema);
  if (partials)
    hipLaunchKernelGGL(ema_update_kernel<true>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, sl, chunks, em, state, table,
                       ntable, begin, interval, partials);
  else
    hipLaunchKernelGGL(ema_update_kernel<false>, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, sl, chunks, em, state, table,
                       ntable, begin, interval, partials);
  return s2f_check_launch("s2f_ema_update");
}

extern "C" int s2f_ema_swap(const int64_t* slots, const int32_t* chunks, int nchunks, float* ema, void* stream) {
  S2F_REQUIRE(slots && chunks && ema, S2F_EINVAL, "s2f_ema_swap: null pointer");
  S2F_REQUIRE(nchunks > 0, S2F_EINVAL, "s2f_ema_swap: no chunks");
  S2F_REQUIRE(s2f_aligned16(ema), S2F_EALIGN, "s2f_ema_swap: the ema buffer must be 16-byte aligned");
  S2F_REQUIRE(s2f_adamw_chunk_elems() == kEmaChunk, S2F_EINVAL, "s2f_ema_swap: built for chunks of %d elements", kEmaChunk);
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(slots), chunks, reinterpret_cast<uint32_t*>(ema));
  return s2f_check_launch("s2f_ema_swap");
}
