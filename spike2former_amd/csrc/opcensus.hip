// Operand census (include/s2f.h "operand census"; gfx950 only): one launch reduces one activation operand of a synaptic op -- n
// contiguous fp32 or bf16 elements -- into one row of eight 64-bit integers: how many elements, the sum and the maximum of their
// integer spike levels x * D, how many are non-zero, how many lie off the level grid, how many are not finite.  The host
// (spike2former_amd/energy.py: OpCensus) derives from the rows whether an op is accumulate-only and how many synaptic operations it
// performs, and checks at the point of use that a spike map really is a map of multiples of 1 / D.
//
//   s2f_operand_census   a streaming reduction: a grid-stride loop of 16-byte loads (two in flight per thread) over the 16-byte
//                        aligned middle of the operand, the (at most 7 + 7) elements before and behind it one per lane of workgroup
//                        0; sums across the 64 lanes by __shfl_xor, across the sixteen waves through LDS, then ONE 64-bit atomic
//                        per field and workgroup.  Every field is an integer: the row does not depend on the order the atomics
//                        arrive in.  All workgroups add into the SAME eight words, and atomics on one address are served one
//                        after the other: hence few, large workgroups (at most two of 1024 threads per CU) and no atomic for a
//                        field whose contribution is zero (the off-grid and non-finite counts of a sound map).  Measured on 2^25
//                        elements (profiles/op_census.txt): fp32 36 us, 0.96 of a device-to-device copy of the same bytes; bf16
//                        37 us, 1.89 of its copy -- the time follows the element count there (the grid test and five sums per
//                        element, two elements per word), not the bytes: bf16 is what nearly every operand of a census is, and
//                        the per-element arithmetic is where a faster kernel would start.
//                        Partial sums: 32-bit over the at most 8 elements of one 16-byte group (8 * 65535 < 2^32), folded into
//                        64-bit sums per thread after every group; everything from there on is 64-bit.
#include "s2f_common.h"
#include "census_level.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / S2F_WAVE;
constexpr int kMaxBlocks = 512;           // 2 workgroups = 32 waves on each of 256 CUs; the grid-stride loop takes the rest
constexpr int kFields = 5;                // level sum, non-zero, off grid, non-finite, max level

typedef unsigned long long u64;

struct Group {          // one 16-byte group (or one element of the ends)
  unsigned level, nonzero, off, nonfinite, max_level;
};

struct Acc {
  u64 level, nonzero, off, nonfinite;
  unsigned max_level;
  __device__ __forceinline__ void add(const Group& g) {
    level += g.level;
    nonzero += g.nonzero;
    off += g.off;
    nonfinite += g.nonfinite;
    max_level = g.max_level > max_level ? g.max_level : max_level;
  }
};

// One element, given as the bits of its fp32 value (census_level.h: the level and the grid test, shared with firingmap.hip).
__device__ __forceinline__ void census_one(unsigned bits, float Df, Group& a) {
  const S2fLevel e = s2f_census_level(bits, Df);
  a.level += e.level;
  a.nonzero += e.nonzero;
  a.off += !e.on;
  a.nonfinite += !e.finite;
  a.max_level = e.level > a.max_level ? e.level : a.max_level;
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S2F_WAVE);
  return v;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) {
    const unsigned o = __shfl_xor(v, m, S2F_WAVE);
    v = o > v ? o : v;
  }
  return v;
}

// One 16-byte group of fp32 (4 elements) or bf16 (8 elements; two per word, the lower address in the low half).
template <bool kBf16>
__device__ __forceinline__ void census_group(const uint4& w, float Df, Acc& a) {
  const unsigned words[4] = {w.x, w.y, w.z, w.w};
  Group g = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!kBf16) {
      census_one(words[k], Df, g);
    } else {
      census_one(words[k] << 16, Df, g);
      census_one(words[k] & 0xffff0000u, Df, g);
    }
  }
  a.add(g);
}

__device__ __forceinline__ unsigned elem_bits(const float* p, int64_t i) { return __float_as_uint(p[i]); }
__device__ __forceinline__ unsigned elem_bits(const unsigned short* p, int64_t i) { return (unsigned)p[i] << 16; }

// x: the operand's first element; head: elements in front of the first 16-byte boundary (already clipped to n); nvec: whole
// 16-byte groups behind them; the remaining n - head - nvec * VEC elements follow the last group.
template <typename T>
__global__ __launch_bounds__(kThreads) void operand_census_kernel(const T* __restrict__ x, int64_t n, int head, int64_t nvec, float Df,
                                                                  u64* __restrict__ row) {
  constexpr int VEC = 16 / (int)sizeof(T);
  Acc a = {0, 0, 0, 0, 0u};
  const uint4* __restrict__ body = reinterpret_cast<const uint4*>(x + head);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += 2 * stride) {
    // two loads in flight; a group past the end is read as zeros, which count nothing (the elements are counted from n)
    const uint4 w0 = body[v];
    const uint4 w1 = v + stride < nvec ? body[v + stride] : make_uint4(0u, 0u, 0u, 0u);
    census_group<sizeof(T) == 2>(w0, Df, a);
    census_group<sizeof(T) == 2>(w1, Df, a);
  }
  if (blockIdx.x == 0) {
    const int tail = (int)(n - head - nvec * VEC);          // < VEC
    const int t = threadIdx.x;
    Group g = {0u, 0u, 0u, 0u, 0u};
    if (t < head)
      census_one(elem_bits(x, t), Df, g);
    else if (t < head + tail)
      census_one(elem_bits(x, (int64_t)head + nvec * VEC + (t - head)), Df, g);
    a.add(g);
  }
  a.level = wave_sum_u64(a.level);
  a.nonzero = wave_sum_u64(a.nonzero);
  a.off = wave_sum_u64(a.off);
  a.nonfinite = wave_sum_u64(a.nonfinite);
  a.max_level = wave_max_u32(a.max_level);
  __shared__ u64 part[kWaves][kFields];
  const int lane = threadIdx.x % S2F_WAVE, wave = threadIdx.x / S2F_WAVE;
  if (lane == 0) {
    part[wave][0] = a.level;
    part[wave][1] = a.nonzero;
    part[wave][2] = a.off;
    part[wave][3] = a.nonfinite;
    part[wave][4] = a.max_level;
  }
  __syncthreads();
  if (threadIdx.x < kFields) {
    const int f = threadIdx.x;
    u64 v = part[0][f];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = f == 4 ? (part[w][f] > v ? part[w][f] : v) : v + part[w][f];
    // row: 0 elements | 1 level sum | 2 non-zero | 3 off grid | 4 max level | 5 non-finite | 6 calls | 7 reserved
    if (v != 0) {          // (adding 0 and a maximum with 0 change nothing)
      if (f == 0) atomicAdd(row + 1, v);
      if (f == 1) atomicAdd(row + 2, v);
      if (f == 2) atomicAdd(row + 3, v);
      if (f == 3) atomicAdd(row + 5, v);
      if (f == 4) atomicMax(row + 4, v);
    }
  } else if (blockIdx.x == 0 && threadIdx.x == kFields) {
    atomicAdd(row + 0, (u64)n);
  } else if (blockIdx.x == 0 && threadIdx.x == kFields + 1) {
    atomicAdd(row + 6, 1ull);
  }
}

template <typename T>
void launch(const void* x, int64_t n, int D, int64_t* row, hipStream_t stream) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
  int64_t head = (int64_t)(((16u - (unsigned)(addr & 15u)) & 15u) / sizeof(T));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / VEC;
  int64_t blocks = (nvec + kThreads - 1) / kThreads;
  if (blocks < 1) blocks = 1;          // (n == 0 and operands of a few elements: workgroup 0 alone)
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  S2F_LAUNCH(true, true, operand_census_kernel<T>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, reinterpret_cast<const T*>(x), n,
             (int)head, nvec, (float)D, reinterpret_cast<u64*>(row));
}

}  // namespace

extern "C" int s2f_operand_census(const void* x, int dtype, int64_t n, int D, int64_t* row, void* stream) {
  S2F_REQUIRE(x && row, S2F_EINVAL, "s2f_operand_census: null pointer");
  S2F_REQUIRE(n >= 0, S2F_EINVAL, "s2f_operand_census: n %lld below 0", (long long)n);
  S2F_REQUIRE(D >= 1, S2F_EINVAL, "s2f_operand_census: D %d below 1", D);
  S2F_REQUIRE(dtype == S2F_CENSUS_F32 || dtype == S2F_CENSUS_BF16, S2F_EINVAL,
              "s2f_operand_census: unknown dtype %d (S2F_CENSUS_F32 = 0, S2F_CENSUS_BF16 = 1)", dtype);
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(x) & (dtype == S2F_CENSUS_F32 ? 3u : 1u)) == 0 && (reinterpret_cast<uintptr_t>(row) & 7u) == 0,
              S2F_EALIGN, "s2f_operand_census: x must be aligned to its element, row to 8 bytes");
  if (dtype == S2F_CENSUS_F32)
    launch<float>(x, n, D, row, (hipStream_t)stream);
  else
    launch<unsigned short>(x, n, D, row, (hipStream_t)stream);
  return s2f_check_launch("s2f_operand_census");
}
