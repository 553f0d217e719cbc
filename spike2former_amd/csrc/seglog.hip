// Whether the model segments its own training crops, from inside the captured step (include/s2f.h "segmentation log"; gfx950 only).
// The step holds the decoder's class scores and mask logits and the label map on the device; this file scores them the way
// MaskFormerHead.predict does -- softmax over the classes without the void column, sigmoid of the masks, their product summed over the
// queries, the arg-max -- at the MASK resolution, against the labels the matching costs see (seg[:, ::2, ::2]), and counts the three
// areas of IoUMetric.intersect_and_union per class into a ring the host reads once per log line.
//
//   s2f_seg_log_partials  one workgroup per tile of kTile pixels of one (scored layer, image), one pixel per thread.  The classes go
//                         in chunks of KC, the queries in chunks of 128 or 64: the softmax table of a (class chunk, query chunk) is built in
//                         LDS (a wave per query takes the row's maximum and its sum of exponentials, the sum in fp64, by a fixed
//                         butterfly), every thread adds P[q, k] * sigmoid(mask[q, p]) to its KC scores with one fma per term, q
//                         ascending, re-reading the Q mask logits of its pixel per class chunk, and keeps the running first maximum
//                         across the chunks.  A sigmoid costs about 30 instructions and is evaluated once per (query, class chunk), a
//                         class slot one fma: KC is the one of 32, 76 and 128 with the smallest chunks * (KC + 30) for the K at hand
//                         (K = 150: two chunks of 76).  The three areas are counted in an LDS histogram of 3K int32 (at most kTile
//                         per word) and stored into the workgroup's own slice of `partials`, plain stores.
//   s2f_seg_log_rows      one workgroup per scored layer: wave v adds the partials v, v + 16, ... of its layer, lane = column, and the
//                         sixteen sums of a column meet in LDS (integers: any order, the same sum); the int64 row is stored at
//                         head[0] % window (overwritten, never accumulated into); the last scored layer's workgroup moves the
//                         per-class streaks on and offers the latch head[1]; every workgroup commits by the head protocol of s2f_ring.h.
#include "s2f_common.h"
#include "s2f_ring.h"

namespace {

typedef s2f_u64 u64;

constexpr int kTile = 256;          // pixels per workgroup = threads per workgroup
constexpr int kWaves = kTile / S2F_WAVE;
constexpr int kQC = 128;            // the most queries per chunk: the LDS table is QC * KC * 4 bytes, whatever Q and K are
constexpr int chunk_queries(int KC) { return KC > 76 ? kQC / 2 : kQC; }          // 32 KB at KC = 128, 38 KB at 76, 16 KB at 32
constexpr int kAhead = 8;           // mask logits a thread loads ahead of their use: the loop waits for memory, not for arithmetic
constexpr int kSigmoid = 30;        // the instructions of one sigmoid, in fma slots: what a class chunk costs beside its KC slots
constexpr int kRowsBlock = 1024;    // s2f_seg_log_rows: sixteen waves share a layer's partials
constexpr int kMaxK = 254;          // 255 is the ignored label
constexpr int kMaxLayers = S2F_SEG_LOG_MAX_LAYERS;

struct Layers {
  int n;
  int at[kMaxLayers];
};

// the rule of resize.hip's arg-max: the first maximum; NaN counts as larger than any number (the first NaN wins)
__device__ __forceinline__ bool beats(float v, float best) { return v > best || (v != v && best == best); }
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, S2F_WAVE));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = S2F_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S2F_WAVE);          // a fixed butterfly: every lane, the same bits
  return v;
}

// mask fp32 [B][L*Q][hw] (the head's own buffer), cls fp32 [L][B][Q][K+1], seg u8 [B][2h][2w]; partials int32 [nl*B*tiles][3K],
// workgroup (tile x, image y, scored layer z) owns slice (z*B + y)*tiles + x = {intersect[K], pred[K], label[K]}
template <int KC>
__global__ __launch_bounds__(kTile) void seg_log_partials_kernel(const float* __restrict__ mask, const float* __restrict__ cls,
                                                                 const unsigned char* __restrict__ seg, Layers layers, int L, int B, int Q,
                                                                 int K, int h, int w, int* __restrict__ partials) {
  constexpr int QC = chunk_queries(KC);
  static_assert(KC % 4 == 0 && QC * KC * 4 <= 56 * 1024, "16-byte table reads; table, row figures and histogram within 64 KB");
  __shared__ __attribute__((aligned(16))) float tab[QC][KC];          // P[q][k] of the current (query chunk, class chunk)
  __shared__ float row_max[kQC];
  __shared__ float row_den[kQC];
  __shared__ int hist[3 * kMaxK];
  const int tid = threadIdx.x, lane = tid % S2F_WAVE, wave = tid / S2F_WAVE;
  const int b = blockIdx.y, l = layers.at[blockIdx.z];
  const int hw = h * w;
  const int p = blockIdx.x * kTile + tid;
  const bool active = p < hw;
  for (int i = tid; i < 3 * K; i += kTile) hist[i] = 0;
  const float* __restrict__ crow = cls + ((size_t)l * B + b) * Q * (size_t)(K + 1);
  const float* __restrict__ mpix = mask + ((size_t)b * L + l) * Q * (size_t)hw + (active ? p : 0);          // (past the map: pixel 0, not counted)
  const int nqc = (Q + QC - 1) / QC;
  float best = 0.f;
  int pred = 0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kn = min(KC, K - k0);
    float acc[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) acc[j] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += QC) {
      const int qn = min(QC, Q - q0);
      __syncthreads();          // whoever still reads the table of the chunk before
      if (k0 == 0 || nqc > 1) {          // (one query chunk: the rows' maxima and sums stay for every class chunk)
        for (int q = wave; q < qn; q += kWaves) {
          const float* __restrict__ c = crow + (size_t)(q0 + q) * (K + 1);
          float mx = -INFINITY;
          for (int k = lane; k <= K; k += S2F_WAVE) mx = fmaxf(mx, c[k]);
          mx = wave_max_f32(mx);
          double den = 0.0;
          for (int k = lane; k <= K; k += S2F_WAVE) den += (double)expf(c[k] - mx);          // a NaN score makes its row NaN
          den = wave_sum_f64(den);
          if (lane == 0) {
            row_max[q] = mx;
            row_den[q] = (float)den;
          }
        }
        __syncthreads();
      }
      for (int i = tid; i < qn * KC; i += kTile) {
        const int q = i / KC, j = i % KC;
        tab[q][j] = j < kn ? expf(crow[(size_t)(q0 + q) * (K + 1) + k0 + j] - row_max[q]) / row_den[q] : 0.f;
      }
      __syncthreads();
      const float* __restrict__ m = mpix + (size_t)q0 * hw;
      for (int q = 0; q < qn; q += kAhead) {
        float x[kAhead];          // the next kAhead mask logits of this pixel, their loads in flight together
#pragma unroll
        for (int u = 0; u < kAhead; ++u) x[u] = q + u < qn ? m[(size_t)(q + u) * hw] : 0.f;
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          if (q + u >= qn) break;
          const float s = sigmoidf_(x[u]);
          const float4* __restrict__ t4 = reinterpret_cast<const float4*>(tab[q + u]);          // one address per wave: a broadcast
#pragma unroll
          for (int j = 0; j < KC / 4; ++j) {
            const float4 t = t4[j];
            acc[4 * j + 0] = fmaf(t.x, s, acc[4 * j + 0]);
            acc[4 * j + 1] = fmaf(t.y, s, acc[4 * j + 1]);
            acc[4 * j + 2] = fmaf(t.z, s, acc[4 * j + 2]);
            acc[4 * j + 3] = fmaf(t.w, s, acc[4 * j + 3]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      if (j < kn && ((k0 == 0 && j == 0) || beats(acc[j], best))) {
        best = acc[j];
        pred = k0 + j;
      }
    }
  }
  if (active) {
    const int y = p / w, x = p - y * w;
    const int label = seg[((size_t)b * (2 * h) + 2 * y) * (size_t)(2 * w) + 2 * x];
    if (label < K) {          // 255 (ignored) and any label >= K count nowhere
      atomicAdd(&hist[2 * K + label], 1);
      atomicAdd(&hist[K + pred], 1);
      if (pred == label) atomicAdd(&hist[label], 1);
    }
  }
  __syncthreads();
  int* __restrict__ out = partials + (((size_t)blockIdx.z * B + b) * gridDim.x + blockIdx.x) * (size_t)(3 * K);
  for (int i = tid; i < 3 * K; i += kTile) out[i] = hist[i];
}

// what a pixel and query cost with class chunks of KC: every chunk its KC fma slots and one sigmoid
inline int chunk_cost(int K, int KC) { return (K + KC - 1) / KC * (KC + kSigmoid); }

// partials int32 [nl][per_layer][3K]; ring int64 [window][nl][3][K]; streak int32 [K]
__global__ __launch_bounds__(kRowsBlock) void seg_log_rows_kernel(const int* __restrict__ partials, int nl, int per_layer, int K,
                                                             long long* __restrict__ ring, int window, int* __restrict__ streak,
                                                             int patience, u64* head) {
  __shared__ u64 total[3 * kMaxK];
  const int i = blockIdx.x;          // (the grid is nl workgroups)
  const int lane = threadIdx.x % S2F_WAVE, wave = threadIdx.x / S2F_WAVE;
  const u64 row = s2f_ring_row(head);
  const int* __restrict__ src = partials + (size_t)i * per_layer * (size_t)(3 * K);
  long long* __restrict__ out = ring + ((long long)(row % (u64)window) * nl + i) * (long long)(3 * K);
  for (int c = threadIdx.x; c < 3 * K; c += kRowsBlock) total[c] = 0;
  __syncthreads();
  for (int c = lane; c < 3 * K; c += S2F_WAVE) {
    u64 a = 0;
#pragma unroll 8
    for (int k = wave; k < per_layer; k += kRowsBlock / S2F_WAVE) a += (u64)src[(size_t)k * (3 * K) + c];          // (counts: never negative)
    atomicAdd(&total[c], a);          // LDS; integers: any order, the same sum
  }
  __syncthreads();          // (and every thread of the workgroup holds its row index)
  for (int c = threadIdx.x; c < 3 * K; c += kRowsBlock) out[c] = (long long)total[c];
  if (i == nl - 1) {
    for (int c = threadIdx.x; c < K; c += kRowsBlock) {
      const u64 hit = total[c], labelled = total[2 * K + c];
      if (hit > 0) {
        streak[c] = 0;
      } else if (labelled > 0) {
        const int s = streak[c] + 1;
        streak[c] = s;
        if (s == patience) s2f_ring_offer(head, 1, s2f_ring_event(row, c));
      }          // an absent class: unchanged
    }
  }
  if (threadIdx.x == 0) s2f_ring_commit(head, row, nl);
}

inline bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

}  // namespace

extern "C" int s2f_seg_log_tile_pixels(void) { return kTile; }

extern "C" int s2f_seg_log_partials(const float* mask, const float* cls, const uint8_t* seg, const int32_t* layers, int nl, int L, int B,
                                    int Q, int K, int h, int w, int32_t* partials, void* stream) {
  S2F_REQUIRE(mask && cls && seg && layers && partials, S2F_EINVAL, "s2f_seg_log_partials: null pointer");
  S2F_REQUIRE(K >= 1 && K <= kMaxK, S2F_EINVAL, "s2f_seg_log_partials: K %d outside 1 .. %d", K, kMaxK);
  S2F_REQUIRE(Q >= 1, S2F_EINVAL, "s2f_seg_log_partials: Q %d below 1", Q);
  S2F_REQUIRE(L >= 1 && B >= 1 && B <= 65535, S2F_EINVAL, "s2f_seg_log_partials: L %d below 1 or B %d outside 1 .. 65535", L, B);
  S2F_REQUIRE(h >= 1 && w >= 2 && w % 2 == 0 && ((long long)h * w) % 4 == 0 && (long long)h * w < (1ll << 30), S2F_EINVAL,
              "s2f_seg_log_partials: a %d x %d mask map: w must be even and h * w a multiple of 4 (below 2^30)", h, w);
  S2F_REQUIRE(nl >= 1 && nl <= kMaxLayers, S2F_EINVAL, "s2f_seg_log_partials: %d scored layers outside 1 .. %d", nl, kMaxLayers);
  Layers ls;
  ls.n = nl;
  for (int i = 0; i < kMaxLayers; ++i) ls.at[i] = 0;
  for (int i = 0; i < nl; ++i) {
    S2F_REQUIRE(layers[i] >= 0 && layers[i] < L, S2F_EINVAL, "s2f_seg_log_partials: layer %d outside 0 .. %d", layers[i], L - 1);
    ls.at[i] = layers[i];
  }
  S2F_REQUIRE(aligned(mask, 4) && aligned(cls, 4) && aligned(partials, 4), S2F_EALIGN,
              "s2f_seg_log_partials: mask, cls and partials must be 4-byte aligned");
  const int tiles = (h * w + kTile - 1) / kTile;
  const dim3 grid((unsigned)tiles, (unsigned)B, (unsigned)nl);
  const int c32 = chunk_cost(K, 32), c76 = chunk_cost(K, 76), c128 = chunk_cost(K, 128);
  if (c32 <= c76 && c32 <= c128)
    hipLaunchKernelGGL(seg_log_partials_kernel<32>, grid, dim3(kTile), 0, (hipStream_t)stream, mask, cls, seg, ls, L, B, Q, K, h, w, partials);
  else if (c76 <= c128)
    hipLaunchKernelGGL(seg_log_partials_kernel<76>, grid, dim3(kTile), 0, (hipStream_t)stream, mask, cls, seg, ls, L, B, Q, K, h, w, partials);
  else
    hipLaunchKernelGGL(seg_log_partials_kernel<128>, grid, dim3(kTile), 0, (hipStream_t)stream, mask, cls, seg, ls, L, B, Q, K, h, w, partials);
  return s2f_check_launch("s2f_seg_log_partials");
}

extern "C" int s2f_seg_log_rows(const int32_t* partials, int nl, int per_layer, int K, int64_t* ring, int window, int32_t* streak,
                                int patience, int64_t* head, void* stream) {
  S2F_REQUIRE(partials && ring && streak && head, S2F_EINVAL, "s2f_seg_log_rows: null pointer");
  S2F_REQUIRE(K >= 1 && K <= kMaxK, S2F_EINVAL, "s2f_seg_log_rows: K %d outside 1 .. %d", K, kMaxK);
  S2F_REQUIRE(nl >= 1 && nl <= kMaxLayers, S2F_EINVAL, "s2f_seg_log_rows: %d scored layers outside 1 .. %d", nl, kMaxLayers);
  S2F_REQUIRE(per_layer >= 1, S2F_EINVAL, "s2f_seg_log_rows: %d partials per layer below 1", per_layer);
  S2F_REQUIRE(window >= 1, S2F_EINVAL, "s2f_seg_log_rows: window %d below 1", window);
  S2F_REQUIRE(patience >= 1, S2F_EINVAL, "s2f_seg_log_rows: patience %d below 1", patience);
  S2F_REQUIRE(aligned(partials, 4) && aligned(ring, 8) && aligned(head, 8) && aligned(streak, 4), S2F_EALIGN,
              "s2f_seg_log_rows: ring and head must be 8-byte aligned, partials and streak 4-byte");
  hipLaunchKernelGGL(seg_log_rows_kernel, dim3((unsigned)nl), dim3(kRowsBlock), 0, (hipStream_t)stream, partials, nl, per_layer, K,
                     reinterpret_cast<long long*>(ring), window, streak, patience, reinterpret_cast<u64*>(head));
  return s2f_check_launch("s2f_seg_log_rows");
}
