// Per-parameter gradient, weight and update norms from inside the training step (include/s2f.h "gradient log"; gfx950 only).
// FlatAdamW's buffers already hold everything: the raw gradients and both moments are flat buffers of one layout, the parameters sit
// behind the slot table.  This file is the segmented reduction over them and the path into a ring the host reads once per interval.
//
//   s2f_grad_log_partials  one workgroup per SPAN (<= 16 384 consecutive elements of one parameter; span table built on the host).
//                          Reads g, m, v, p (16-byte loads where the parameter pointer allows, as adamw_step_kernel), restates the
//                          Adam step u of optim.hip in its fp32 expressions, accumulates per thread in fp64 and reduces over the
//                          block in a fixed order; 8 words per span, plain stores.  Nothing floating-point crosses workgroups here.
//   s2f_grad_log_rows      one wave per parameter: lane c < 8 combines column c of that parameter's spans IN SPAN ORDER (sums add,
//                          max of max, counts add) and stores the row at head[0] % window; lane 0 moves the two streaks on, offers
//                          the two latches head[1] and head[3] and advances head[0]: the head protocol of s2f_ring.h.
// Both kernels only READ g, m, v, p, hyper and state.
#include "s2f_common.h"
#include "s2f_ring.h"

#pragma clang fp contract(off)

namespace {

typedef s2f_u64 u64;

constexpr int kSpan = 16384;          // elements per workgroup: 256 threads x 16 float4
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / S2F_WAVE;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S2F_WAVE);          // a fixed butterfly: every lane, the same bits
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, S2F_WAVE));
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S2F_WAVE);
  return v;
}

// slots int64 [nslots][3], hyper float [nslots][2], state float [5]: the tables of adamw_step_kernel (optim.hip), AFTER its launch.
// spans int32 [nspans][2] = {slot, first element inside the slot}; partials 8 words per span, the row's columns over the span.
__global__ __launch_bounds__(kBlock) void grad_log_partials_kernel(const long long* __restrict__ slots, const float* __restrict__ hyper,
                                                                   const int* __restrict__ spans, const float* __restrict__ g,
                                                                   const float* __restrict__ m, const float* __restrict__ v,
                                                                   const float* __restrict__ state, float eps,
                                                                   long long* __restrict__ partials) {
  const int slot = spans[2 * blockIdx.x], start = spans[2 * blockIdx.x + 1];
  const float* __restrict__ p = reinterpret_cast<const float*>(slots[3 * slot]);
  const long long off = slots[3 * slot + 1];
  const int numel = (int)slots[3 * slot + 2];
  const float lr = hyper[2 * slot];
  const bool moved = !(lr < 0.f);          // lr < 0: a parameter without a gradient, u = 0 (optim.hip returns before it moves anything)
  const float bc1 = state[2], bc2s = state[3];
  const float step_size = lr / bc1;
  const int end = min(numel, start + kSpan);
  const bool vec = ((reinterpret_cast<uintptr_t>(p) & 15u) == 0);          // slot offsets are multiples of 4 elements, `start` too
  double sg = 0.0, sp = 0.0, su = 0.0;
  float gmax = 0.f;
  int zeros = 0, bad_g = 0, bad_pu = 0;
  for (int i = 0; i < kSpan / (kBlock * 4); ++i) {
    const int e = start + (i * kBlock + (int)threadIdx.x) * 4;
    if (e >= end) break;
    const int cnt = min(4, end - e);
    float pv[4], gv[4], mv[4], vv[4];
    if (vec && cnt == 4) {
      const float4 a = *reinterpret_cast<const float4*>(p + e), b = *reinterpret_cast<const float4*>(g + off + e);
      pv[0] = a.x, pv[1] = a.y, pv[2] = a.z, pv[3] = a.w;
      gv[0] = b.x, gv[1] = b.y, gv[2] = b.z, gv[3] = b.w;
      if (moved) {
        const float4 c = *reinterpret_cast<const float4*>(m + off + e), d = *reinterpret_cast<const float4*>(v + off + e);
        mv[0] = c.x, mv[1] = c.y, mv[2] = c.z, mv[3] = c.w;
        vv[0] = d.x, vv[1] = d.y, vv[2] = d.z, vv[3] = d.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = k < cnt;
        pv[k] = ok ? p[e + k] : 0.f;
        gv[k] = ok ? g[off + e + k] : 0.f;
        mv[k] = ok && moved ? m[off + e + k] : 0.f;
        vv[k] = ok && moved ? v[off + e + k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k >= cnt) break;          // the pads behind numel never count
      float u = 0.f;
      if (moved) {
        const float denom = sqrtf(vv[k]) / bc2s + eps;          // optim.hip's expressions, in its order
        u = step_size * (mv[k] / denom);
      }
      const float gk = gv[k], pk = pv[k];
      if (isfinite(gk)) {
        sg += (double)gk * (double)gk;
        gmax = fmaxf(gmax, fabsf(gk));
        zeros += gk == 0.f;
      } else {
        ++bad_g;
      }
      const bool pf = isfinite(pk), uf = isfinite(u);
      if (pf) sp += (double)pk * (double)pk;
      if (uf) su += (double)u * (double)u;
      bad_pu += !(pf && uf);
    }
  }
  // fixed order: a butterfly over each wave, then the four waves' results in wave order
  __shared__ double red_f[kWaves][4];
  __shared__ int red_i[kWaves][3];
  sg = wave_sum_f64(sg);
  sp = wave_sum_f64(sp);
  su = wave_sum_f64(su);
  const double gm = wave_max_f64((double)gmax);
  zeros = wave_sum_i32(zeros);
  bad_g = wave_sum_i32(bad_g);
  bad_pu = wave_sum_i32(bad_pu);
  const int wave = threadIdx.x / S2F_WAVE;
  if (threadIdx.x % S2F_WAVE == 0) {
    red_f[wave][0] = sg, red_f[wave][1] = sp, red_f[wave][2] = su, red_f[wave][3] = gm;
    red_i[wave][0] = zeros, red_i[wave][1] = bad_g, red_i[wave][2] = bad_pu;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int c = threadIdx.x;
    long long word;
    if (c < 3) {
      double a = red_f[0][c];
      for (int w = 1; w < kWaves; ++w) a += red_f[w][c];
      word = __double_as_longlong(a);
    } else if (c == 3) {
      double a = red_f[0][3];
      for (int w = 1; w < kWaves; ++w) a = fmax(a, red_f[w][3]);
      word = __double_as_longlong(a);
    } else if (c < 7) {
      long long a = 0;
      for (int w = 0; w < kWaves; ++w) a += red_i[w][c - 4];
      word = a;
    } else {
      word = end - start;          // the span's elements: the row's numel is their sum
    }
    partials[(size_t)blockIdx.x * 8 + c] = word;
  }
}

// streak int32 [n][2] = {rows in a row with an all-zero gradient, rows in a row with a non-finite gradient element}
__global__ __launch_bounds__(S2F_WAVE) void grad_log_rows_kernel(const int* __restrict__ spans, int nspans,
                                                                 const long long* __restrict__ partials, int n,
                                                                 long long* __restrict__ ring, int window, int* __restrict__ streak,
                                                                 int patience, u64* head) {
  const int i = blockIdx.x;          // (the grid is n workgroups of one wave)
  const int lane = threadIdx.x;
  const u64 row = s2f_ring_row(head);
  // the first span of parameter i: the table is sorted by slot (the whole wave takes the same steps)
  int lo = 0, hi = nspans;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (spans[2 * mid] < i) lo = mid + 1; else hi = mid;
  }
  const int c = lane & 7;
  double fa = 0.0;
  long long ia = 0;
  for (int k = lo; k < nspans && spans[2 * k] == i; ++k) {          // span order
    const long long w = partials[(size_t)k * 8 + c];
    if (c < 3) fa += __longlong_as_double(w);
    else if (c == 3) fa = fmax(fa, __longlong_as_double(w));
    else ia += w;
  }
  const long long word = c < 4 ? __double_as_longlong(fa) : ia;
  if (lane < 8) ring[((long long)(row % (u64)window) * n + i) * 8 + c] = word;
  const long long zeros = __shfl(word, 4, S2F_WAVE), bad = __shfl(word, 5, S2F_WAVE), numel = __shfl(word, 7, S2F_WAVE);
  if (lane == 0) {
    int s = streak[2 * i], b = streak[2 * i + 1];
    s = (numel > 0 && zeros == numel) ? s + 1 : 0;
    b = bad > 0 ? b + 1 : 0;
    streak[2 * i] = s;
    streak[2 * i + 1] = b;
    const u64 event = s2f_ring_event(row, i);
    if (s == patience) s2f_ring_offer(head, 1, event);
    if (b == 1) s2f_ring_offer(head, 3, event);
    s2f_ring_commit(head, row, n);
  }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int s2f_grad_log_span_elems(void) { return kSpan; }

extern "C" int s2f_grad_log_partials(const int64_t* slots, const float* hyper, const int32_t* spans, int nspans, const float* g,
                                     const float* m, const float* v, const float* state, float eps, int64_t* partials, void* stream) {
  S2F_REQUIRE(slots && hyper && spans && g && m && v && state && partials, S2F_EINVAL, "s2f_grad_log_partials: null pointer");
  S2F_REQUIRE(nspans >= 1, S2F_EINVAL, "s2f_grad_log_partials: n %d spans below 1", nspans);
  S2F_REQUIRE(s2f_aligned16(g) && s2f_aligned16(m) && s2f_aligned16(v) && aligned8(partials) && aligned8(slots), S2F_EALIGN,
              "s2f_grad_log_partials: flat buffers must be 16-byte aligned, slots and partials 8-byte");
  hipLaunchKernelGGL(grad_log_partials_kernel, dim3((unsigned)nspans), dim3(kBlock), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(slots), hyper, spans, g, m, v, state, eps, reinterpret_cast<long long*>(partials));
  return s2f_check_launch("s2f_grad_log_partials");
}

extern "C" int s2f_grad_log_rows(const int32_t* spans, int nspans, const int64_t* partials, int n, int64_t* ring, int window,
                                 int32_t* streak, int patience, int64_t* head, void* stream) {
  S2F_REQUIRE(spans && partials && ring && streak && head, S2F_EINVAL, "s2f_grad_log_rows: null pointer");
  S2F_REQUIRE(nspans >= 1, S2F_EINVAL, "s2f_grad_log_rows: n %d spans below 1", nspans);
  S2F_REQUIRE(n >= 1, S2F_EINVAL, "s2f_grad_log_rows: n %d below 1", n);
  S2F_REQUIRE(window >= 1, S2F_EINVAL, "s2f_grad_log_rows: window %d below 1", window);
  S2F_REQUIRE(patience >= 1, S2F_EINVAL, "s2f_grad_log_rows: patience %d below 1", patience);
  S2F_REQUIRE(aligned8(partials) && aligned8(ring) && aligned8(head) && (reinterpret_cast<uintptr_t>(streak) & 3u) == 0, S2F_EALIGN,
              "s2f_grad_log_rows: partials, ring and head must be 8-byte aligned, streak 4-byte");
  hipLaunchKernelGGL(grad_log_rows_kernel, dim3((unsigned)n), dim3(S2F_WAVE), 0, (hipStream_t)stream, spans, nspans,
                     reinterpret_cast<const long long*>(partials), n, reinterpret_cast<long long*>(ring), window, streak, patience,
                     reinterpret_cast<u64*>(head));
  return s2f_check_launch("s2f_grad_log_rows");
}
