// Segmentation scoring (include/s2f.h "evaluation"): per image ONE launch that adds the class histograms of the participating
// pixels -- intersection, prediction, label -- into a device-resident int64 [3, K] accumulator.  gfx950 only.
//
//   * every lane takes 4 consecutive pixels per iteration: the prediction with 16-byte loads (two for int64, one for fp32), the
//     label with one 4-byte (uint8) or two 16-byte (int64) loads when it is contiguous and aligned behind the same head, otherwise
//     with four strided element loads (a transposed label is read in place);
//   * the pixels in front of the first 16-byte boundary of `pred` and behind the last whole group (at most 3 + 3) go through the
//     same counting routine on the first wave of workgroup 0;
//   * per-workgroup histograms [3][K] of 32-bit counters in LDS.  Label maps are large uniform regions: the 64 pixels a wave
//     holds in one slot usually carry one to three distinct (pred, label) pairs, and 64 LDS atomics on one address serialise.
//     So a lane whose 4 pixels agree takes part in the wave's PEELING with weight 4: the key of the lowest lane that is still
//     pending, a ballot of the lanes that hold it, one lane adds 4 x popcount, those lanes retire; peeling stops after a round that
//     retired fewer than SEG_PEEL_MIN_LANES lanes (or SEG_PEEL_MAX_ROUNDS rounds) and the lanes left -- and every lane on a region
//     boundary -- add for themselves.  Measured: a round costs about as much as 64 LDS adds on one address, so only rounds that
//     retire many lanes pay (docs/EXPERIMENTS.md "IoUMetric");
//   * flush: one 64-bit global atomic add per non-zero bin and workgroup.  Integer adds: the totals do not depend on the arrival
//     order, so they are bit-repeatable and exact.
#include "s2f_common.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_PEEL_MAX_ROUNDS = 4, SEG_PEEL_MIN_LANES = 16;
constexpr int SEG_MAX_GRID = 512;          // 2 workgroups per CU of the 256-CU part; a 512 x 683 map needs 342

struct alignas(16) I64x2 {
  int64_t v[2];
};

__device__ __forceinline__ int pred_class(int64_t p, int K) { return (p >= 0 && p < (int64_t)K) ? (int)p : -1; }
// a float map counts where it holds a class index exactly (the 0 / 1 maps of a one-class head); NaN fails every comparison
__device__ __forceinline__ int pred_class(float p, int K) { return (p >= 0.0f && p < (float)K && p == truncf(p)) ? (int)p : -1; }

// -> key = (pred class + 1) | (label class + 1) << 16, 0 in a half = "counts nowhere"; active: the pixel has something to count
template <typename PredT>
__device__ __forceinline__ uint32_t seg_key(PredT p, int64_t l, int K, int64_t ignore, int rzl, bool& active) {
  if (rzl) l = (l == 0 || l == 255) ? 255 : l - 1;          // LoadAnnotations(reduce_zero_label=True) on the raw annotation
  const int pc = pred_class(p, K);
  const int lc = (l >= 0 && l < (int64_t)K) ? (int)l : -1;
  const uint32_t key = (uint32_t)(pc + 1) | ((uint32_t)(lc + 1) << 16);
  active = active && l != ignore && key != 0;
  return key;
}

__device__ __forceinline__ void seg_add(unsigned int* hist, int K, uint32_t key, unsigned int n) {
  const int pc = (int)(key & 0xffffu) - 1, lc = (int)(key >> 16) - 1;
  if (pc >= 0) atomicAdd(&hist[K + pc], n);
  if (lc >= 0) atomicAdd(&hist[2 * K + lc], n);
  if (pc >= 0 && pc == lc) atomicAdd(&hist[pc], n);
}

// Called by all 64 lanes of a wave together (wave-uniform control flow around it); an active lane holds `weight` pixels of `key`.
__device__ __forceinline__ void seg_wave_count(unsigned int* hist, int K, uint32_t key, bool active, int lane, unsigned int weight) {
  uint64_t pend = __ballot(active);
#pragma unroll 1
  for (int r = 0; r < SEG_PEEL_MAX_ROUNDS && pend != 0; ++r) {
    // the first lane that is STILL pending (the raw register of lane 0 may belong to an ignored or already counted pixel)
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)pend) - 1);
    const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
    const bool mine = active && key == k;
    const uint64_t same = __ballot(mine);
    const int n = __popcll((unsigned long long)same);
    // (the leader's own register, not k: with a wave-uniform address the compiler wraps each add in its own lane-counting code)
    if (lane == leader) seg_add(hist, K, key, (unsigned int)n * weight);
    active = active && !mine;
    pend &= ~same;
    if (n < SEG_PEEL_MIN_LANES) break;          // a round costs more than the adds of the few lanes it would retire next
  }
  if (active) seg_add(hist, K, key, weight);
}

template <typename LabelT>
__device__ __forceinline__ int64_t seg_label_at(const LabelT* __restrict__ label, int p, int W, int64_t lrs, int64_t lps, int contig) {
  if (contig) return (int64_t)label[p];
  const int r = p / W, c = p - r * W;
  return (int64_t)label[(int64_t)r * lrs + (int64_t)c * lps];
}

__device__ __forceinline__ void seg_load4(const int64_t* __restrict__ p, int64_t (&out)[4]) {
  const I64x2 a = *reinterpret_cast<const I64x2*>(p), b = *reinterpret_cast<const I64x2*>(p + 2);
  out[0] = a.v[0], out[1] = a.v[1], out[2] = b.v[0], out[3] = b.v[1];
}
__device__ __forceinline__ void seg_load4(const float* __restrict__ p, float (&out)[4]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  out[0] = a.x, out[1] = a.y, out[2] = a.z, out[3] = a.w;
}
__device__ __forceinline__ void seg_load4_label(const int64_t* __restrict__ p, int64_t (&out)[4]) { seg_load4(p, out); }
__device__ __forceinline__ void seg_load4_label(const uint8_t* __restrict__ p, int64_t (&out)[4]) {
  const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
  out[0] = w & 0xffu, out[1] = (w >> 8) & 0xffu, out[2] = (w >> 16) & 0xffu, out[3] = w >> 24;
}

// pixels [0, head) and [head + 4 ngroups, HW) are the scalar head and tail; group g covers pixels head + 4 g .. + 3
template <typename PredT, typename LabelT>
__global__ __launch_bounds__(SEG_THREADS) void seg_hist_kernel(const PredT* __restrict__ pred, const LabelT* __restrict__ label, int64_t lrs,
                                                               int64_t lps, int W, int head, int ngroups, int HW, int K, int64_t ignore,
                                                               int rzl, int contig, int lab_vec, unsigned long long* __restrict__ totals) {
  extern __shared__ unsigned int hist[];
  const int tid = threadIdx.x, lane = tid & (S2F_WAVE - 1);
  for (int i = tid; i < 3 * K; i += SEG_THREADS) hist[i] = 0;
  __syncthreads();

  const int stride = gridDim.x * SEG_THREADS;
  // the loop runs on the wave's first group: every lane of a wave makes the same number of trips
  for (int g0 = blockIdx.x * SEG_THREADS + (tid - lane); g0 < ngroups; g0 += stride) {
    const int g = g0 + lane;
    const bool in = g < ngroups;
    PredT pv[4] = {};
    int64_t lv[4] = {};
    if (in) {
      const int p0 = head + 4 * g;
      seg_load4(pred + p0, pv);
      if (lab_vec) {
        seg_load4_label(label + p0, lv);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[j] = seg_label_at(label, p0 + j, W, lrs, lps, contig);
      }
    }
    uint32_t key[4];
    bool act[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      act[j] = in;
      key[j] = seg_key(pv[j], lv[j], K, ignore, rzl, act[j]);
    }
    // a lane whose four pixels agree (the inside of a region) enters the wave's peeling once with weight 4; a lane on a boundary
    // adds its pixels itself
    const bool uni = act[0] && act[1] && act[2] && act[3] && key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
    seg_wave_count(hist, K, key[0], uni, lane, 4u);
    if (!uni) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (act[j]) seg_add(hist, K, key[j], 1u);
    }
  }
  if (blockIdx.x == 0 && tid < S2F_WAVE) {
    const int tail0 = head + 4 * ngroups, n = head + (HW - tail0);          // n <= 6
    bool active = tid < n;
    const int p = tid < head ? tid : tail0 + (tid - head);
    PredT pvs = PredT();
    int64_t lvs = 0;
    if (active) {
      pvs = pred[p];
      lvs = seg_label_at(label, p, W, lrs, lps, contig);
    }
    const uint32_t key = seg_key(pvs, lvs, K, ignore, rzl, active);
    seg_wave_count(hist, K, key, active, lane, 1u);
  }
  __syncthreads();
  for (int i = tid; i < 3 * K; i += SEG_THREADS) {
    const unsigned int v = hist[i];
    if (v != 0) atomicAdd(&totals[i], (unsigned long long)v);
  }
}

template <typename PredT, typename LabelT>
int seg_hist_launch(const void* pred, const void* label, int64_t lrs, int64_t lps, int W, int64_t HW, int K, int ignore_index, int flags,
                    int64_t* totals, hipStream_t stream) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(pred), la = reinterpret_cast<uintptr_t>(label);
  int64_t head = (int64_t)(((16 - (pa & 15u)) & 15u) / sizeof(PredT));
  if (head > HW) head = HW;
  const int64_t ngroups = (HW - head) / 4;
  const int contig = (lps == 1 && lrs == W) ? 1 : 0;
  const uintptr_t need = sizeof(LabelT) == 1 ? 4 : 16;          // the label's address at the first group
  const int lab_vec = (contig && ((la + (uintptr_t)head * sizeof(LabelT)) & (need - 1)) == 0) ? 1 : 0;
  int64_t grid = (ngroups + SEG_THREADS - 1) / SEG_THREADS;
  if (grid < 1) grid = 1;
  if (grid > SEG_MAX_GRID) grid = SEG_MAX_GRID;
  S2F_LAUNCH(true, true, (seg_hist_kernel<PredT, LabelT>), dim3((unsigned)grid), dim3(SEG_THREADS), (size_t)3 * K * sizeof(unsigned int), stream,
             static_cast<const PredT*>(pred), static_cast<const LabelT*>(label), lrs, lps, W, (int)head, (int)ngroups, (int)HW, K,
             (int64_t)ignore_index, flags & S2F_SEG_REDUCE_ZERO_LABEL, contig, lab_vec, reinterpret_cast<unsigned long long*>(totals));
  return s2f_check_launch("s2f_seg_hist");
}

}  // namespace

extern "C" int s2f_seg_hist(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                            int64_t label_pixel_stride, int W, int64_t HW, int K, int ignore_index, int flags, int64_t* totals,
                            void* stream) {
  S2F_REQUIRE(pred && label && totals, S2F_EINVAL, "s2f_seg_hist: null pointer");
  S2F_REQUIRE(HW > 0 && HW < ((int64_t)1 << 31) - 8, S2F_EINVAL,
              "s2f_seg_hist: bad map size HW %lld (1 .. 2^31 - 9: the workgroup counters are 32-bit)", (long long)HW);
  S2F_REQUIRE(W > 0 && HW % W == 0, S2F_EINVAL, "s2f_seg_hist: HW %lld is no whole number of rows of W %d", (long long)HW, W);
  S2F_REQUIRE(K > 0 && K <= S2F_SEG_HIST_MAX_CLASSES, S2F_EINVAL, "s2f_seg_hist: K %d outside 1 .. %d (the LDS histogram)", K,
              S2F_SEG_HIST_MAX_CLASSES);
  S2F_REQUIRE(pred_dtype == S2F_SEG_PRED_I64 || pred_dtype == S2F_SEG_PRED_F32, S2F_EINVAL, "s2f_seg_hist: unknown pred dtype code %d",
              pred_dtype);
  S2F_REQUIRE(label_dtype == S2F_SEG_LABEL_U8 || label_dtype == S2F_SEG_LABEL_I64, S2F_EINVAL,
              "s2f_seg_hist: unknown label dtype code %d", label_dtype);
  S2F_REQUIRE((flags & ~S2F_SEG_REDUCE_ZERO_LABEL) == 0, S2F_EINVAL, "s2f_seg_hist: unknown flags %d", flags);
  S2F_REQUIRE(label_row_stride >= 0 && label_pixel_stride >= 0, S2F_EINVAL, "s2f_seg_hist: negative label stride");
  const uintptr_t pa = reinterpret_cast<uintptr_t>(pred), la = reinterpret_cast<uintptr_t>(label), ta = reinterpret_cast<uintptr_t>(totals);
  S2F_REQUIRE(pa % (pred_dtype == S2F_SEG_PRED_I64 ? 8 : 4) == 0 && (label_dtype == S2F_SEG_LABEL_U8 || la % 8 == 0) && ta % 8 == 0,
              S2F_EALIGN, "s2f_seg_hist: a pointer is not aligned to its element size");
  hipStream_t st = (hipStream_t)stream;
  if (pred_dtype == S2F_SEG_PRED_I64) {
    if (label_dtype == S2F_SEG_LABEL_U8)
      return seg_hist_launch<int64_t, uint8_t>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, totals, st);
    return seg_hist_launch<int64_t, int64_t>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, totals, st);
  }
  if (label_dtype == S2F_SEG_LABEL_U8)
    return seg_hist_launch<float, uint8_t>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, totals, st);
  return seg_hist_launch<float, int64_t>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, totals, st);
}
