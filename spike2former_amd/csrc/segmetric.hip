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
//
// s2f_seg_confusion (the class-pair table, [K, K] int64, row = label, column = prediction) runs the SAME front end -- seg_scan
// below: the loads, the scalar head and tail, seg_key, the peeling -- over another set of bins: the key the peeling ballots on IS
// the (prediction, label) pair, so a peeled round is one add of 4 x popcount into one bin of the table.  Two routes:
//   * LDS: a per-workgroup [K][K] table of 32-bit counters (4 K^2 bytes: 90 000 at K = 150, 116 964 at K = 171) while it fits
//     S2F_SEG_CONF_LDS_BYTES and what the device reports; 1024 threads, since at most two such workgroups -- one above 80 KiB --
//     fit a CU and the loads need waves in flight; every workgroup pays K^2 words of zeroing and K^2 of flush scan, so the grid is
//     no larger than the resident slots and no workgroup gets fewer than SEG_CONF_MIN_TRIPS trips of the pixel loop;
//   * global: 64-bit atomics straight into the matrix after the same peeling (every larger K, or S2F_SEG_CONF_GLOBAL).
#include "s2f_common.h"
#include "seg_label.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_PEEL_MAX_ROUNDS = 4, SEG_PEEL_MIN_LANES = 16;
constexpr int SEG_MAX_GRID = 512;          // 2 workgroups per CU of the 256-CU part; a 512 x 683 map needs 342
constexpr int SEG_CONF_THREADS = 1024;     // the LDS route of the class-pair table: 16 waves on the CU that holds a table
constexpr int SEG_CONF_MIN_TRIPS = 4;      // ... and at least this many trips of the pixel loop per workgroup and table

struct alignas(16) I64x2 {
  int64_t v[2];
};

// -> key = (pred class + 1) | (label class + 1) << 16, 0 in a half = "counts nowhere"; active: the pixel has something to count
template <typename PredT>
__device__ __forceinline__ uint32_t seg_key(PredT p, int64_t l, int K, int64_t ignore, int rzl, bool& active) {
  if (rzl) l = seg_reduce_zero_label(l);
  const int pc = pred_class(p, K);
  const int lc = (l >= 0 && l < (int64_t)K) ? (int)l : -1;
  const uint32_t key = (uint32_t)(pc + 1) | ((uint32_t)(lc + 1) << 16);
  active = active && l != ignore && key != 0;
  return key;
}

// The bins a counted key goes to: add(key, n) is the only thing the front end knows of them.
struct SegHistBins {          // s2f_seg_hist: [3][K] 32-bit counters in LDS {intersection, prediction, label}
  unsigned int* hist;
  int K;
  __device__ __forceinline__ void add(uint32_t key, unsigned int n) const {
    const int pc = (int)(key & 0xffffu) - 1, lc = (int)(key >> 16) - 1;
    if (pc >= 0) atomicAdd(&hist[K + pc], n);
    if (lc >= 0) atomicAdd(&hist[2 * K + lc], n);
    if (pc >= 0 && pc == lc) atomicAdd(&hist[pc], n);
  }
};
// s2f_seg_confusion: table[label][pred], a pixel counts only with BOTH halves of its key a class.  Counter = unsigned int: the
// workgroup's table in LDS; unsigned long long: the caller's matrix itself.
template <typename Counter>
struct SegPairBins {
  Counter* table;
  int K;
  __device__ __forceinline__ void add(uint32_t key, unsigned int n) const {
    const int pc = (int)(key & 0xffffu) - 1, lc = (int)(key >> 16) - 1;
    if (pc >= 0 && lc >= 0) atomicAdd(&table[lc * K + pc], (Counter)n);
  }
};

// Called by all 64 lanes of a wave together (wave-uniform control flow around it); an active lane holds `weight` pixels of `key`.
template <typename Bins>
__device__ __forceinline__ void seg_wave_count(const Bins& bins, uint32_t key, bool active, int lane, unsigned int weight) {
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
    if (lane == leader) bins.add(key, (unsigned int)n * weight);
    active = active && !mine;
    pend &= ~same;
    if (n < SEG_PEEL_MIN_LANES) break;          // a round costs more than the adds of the few lanes it would retire next
  }
  if (active) bins.add(key, weight);
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

// What the front end needs of one image; pixels [0, head) and [head + 4 ngroups, HW) are the scalar head and tail, group g covers
// pixels head + 4 g .. + 3
struct SegMap {
  int64_t lrs, lps, ignore;
  int W, head, ngroups, HW, K, rzl, contig, lab_vec;
};

template <typename PredT, typename LabelT>
SegMap seg_map(const void* pred, const void* label, int64_t lrs, int64_t lps, int W, int64_t HW, int K, int ignore_index, int flags) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(pred), la = reinterpret_cast<uintptr_t>(label);
  int64_t head = (int64_t)(((16 - (pa & 15u)) & 15u) / sizeof(PredT));
  if (head > HW) head = HW;
  const int64_t ngroups = (HW - head) / 4;
  const int contig = (lps == 1 && lrs == W) ? 1 : 0;
  const uintptr_t need = sizeof(LabelT) == 1 ? 4 : 16;          // the label's address at the first group
  const int lab_vec = (contig && ((la + (uintptr_t)head * sizeof(LabelT)) & (need - 1)) == 0) ? 1 : 0;
  return SegMap{lrs, lps, (int64_t)ignore_index, W, (int)head, (int)ngroups, (int)HW, K, flags & S2F_SEG_REDUCE_ZERO_LABEL, contig, lab_vec};
}

// The front end of both kernels: every participating pixel of the image reaches bins.add exactly once, with the pixels of a
// workgroup of THREADS lanes grid-strided over the groups and the head and tail on the first wave of workgroup 0.
template <int THREADS, typename PredT, typename LabelT, typename Bins>
__device__ __forceinline__ void seg_scan(const PredT* __restrict__ pred, const LabelT* __restrict__ label, const SegMap& m, const Bins& bins) {
  const int tid = threadIdx.x, lane = tid & (S2F_WAVE - 1);
  const int K = m.K, ngroups = m.ngroups, head = m.head;
  const int stride = gridDim.x * THREADS;
  // the loop runs on the wave's first group: every lane of a wave makes the same number of trips
  for (int g0 = blockIdx.x * THREADS + (tid - lane); g0 < ngroups; g0 += stride) {
    const int g = g0 + lane;
    const bool in = g < ngroups;
    PredT pv[4] = {};
    int64_t lv[4] = {};
    if (in) {
      const int p0 = head + 4 * g;
      seg_load4(pred + p0, pv);
      if (m.lab_vec) {
        seg_load4_label(label + p0, lv);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) lv[j] = seg_label_at(label, p0 + j, m.W, m.lrs, m.lps, m.contig);
      }
    }
    uint32_t key[4];
    bool act[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      act[j] = in;
      key[j] = seg_key(pv[j], lv[j], K, m.ignore, m.rzl, act[j]);
    }
    // a lane whose four pixels agree (the inside of a region) enters the wave's peeling once with weight 4; a lane on a boundary
    // adds its pixels itself
    const bool uni = act[0] && act[1] && act[2] && act[3] && key[0] == key[1] && key[1] == key[2] && key[2] == key[3];
    seg_wave_count(bins, key[0], uni, lane, 4u);
    if (!uni) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (act[j]) bins.add(key[j], 1u);
    }
  }
  if (blockIdx.x == 0 && tid < S2F_WAVE) {
    const int tail0 = head + 4 * ngroups, n = head + (m.HW - tail0);          // n <= 6
    bool active = tid < n;
    const int p = tid < head ? tid : tail0 + (tid - head);
    PredT pvs = PredT();
    int64_t lvs = 0;
    if (active) {
      pvs = pred[p];
      lvs = seg_label_at(label, p, m.W, m.lrs, m.lps, m.contig);
    }
    const uint32_t key = seg_key(pvs, lvs, K, m.ignore, m.rzl, active);
    seg_wave_count(bins, key, active, lane, 1u);
  }
}

// `n` 32-bit counters of the workgroup's LDS: zero -- count -- one 64-bit global atomic per non-zero counter
template <int THREADS, typename PredT, typename LabelT, typename Bins>
__device__ __forceinline__ void seg_count_in_lds(const PredT* __restrict__ pred, const LabelT* __restrict__ label, const SegMap& m, int n,
                                                 unsigned long long* __restrict__ out) {
  extern __shared__ unsigned int seg_lds[];
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += THREADS) seg_lds[i] = 0;
  __syncthreads();
  seg_scan<THREADS>(pred, label, m, Bins{seg_lds, m.K});
  __syncthreads();
  for (int i = tid; i < n; i += THREADS) {
    const unsigned int v = seg_lds[i];
    if (v != 0) atomicAdd(&out[i], (unsigned long long)v);
  }
}

template <typename PredT, typename LabelT>
__global__ __launch_bounds__(SEG_THREADS) void seg_hist_kernel(const PredT* __restrict__ pred, const LabelT* __restrict__ label, SegMap m,
                                                               unsigned long long* __restrict__ totals) {
  seg_count_in_lds<SEG_THREADS, PredT, LabelT, SegHistBins>(pred, label, m, 3 * m.K, totals);
}

template <typename PredT, typename LabelT>
__global__ __launch_bounds__(SEG_CONF_THREADS) void seg_conf_lds_kernel(const PredT* __restrict__ pred, const LabelT* __restrict__ label,
                                                                        SegMap m, unsigned long long* __restrict__ matrix) {
  seg_count_in_lds<SEG_CONF_THREADS, PredT, LabelT, SegPairBins<unsigned int>>(pred, label, m, m.K * m.K, matrix);
}

template <typename PredT, typename LabelT>
__global__ __launch_bounds__(SEG_THREADS) void seg_conf_global_kernel(const PredT* __restrict__ pred, const LabelT* __restrict__ label,
                                                                      SegMap m, unsigned long long* __restrict__ matrix) {
  seg_scan<SEG_THREADS>(pred, label, m, SegPairBins<unsigned long long>{matrix, m.K});
}

int seg_grid(int ngroups, int per_group, int cap) {
  int64_t grid = ((int64_t)ngroups + per_group - 1) / per_group;
  return (int)(grid < 1 ? 1 : grid > cap ? cap : grid);
}

template <typename PredT, typename LabelT>
int seg_hist_launch(const void* pred, const void* label, int64_t lrs, int64_t lps, int W, int64_t HW, int K, int ignore_index, int flags,
                    int64_t* totals, hipStream_t stream) {
  const SegMap m = seg_map<PredT, LabelT>(pred, label, lrs, lps, W, HW, K, ignore_index, flags);
  S2F_LAUNCH(true, true, (seg_hist_kernel<PredT, LabelT>), dim3((unsigned)seg_grid(m.ngroups, SEG_THREADS, SEG_MAX_GRID)), dim3(SEG_THREADS),
             (size_t)3 * K * sizeof(unsigned int), stream, static_cast<const PredT*>(pred), static_cast<const LabelT*>(label), m,
             reinterpret_cast<unsigned long long*>(totals));
  return s2f_check_launch("s2f_seg_hist");
}

// lds_dev / cus: what the device reports (unused on the global route)
template <typename PredT, typename LabelT>
int seg_conf_launch(const void* pred, const void* label, int64_t lrs, int64_t lps, int W, int64_t HW, int K, int ignore_index, int flags,
                    int64_t* matrix, bool in_lds, int lds_dev, int cus, hipStream_t stream) {
  const SegMap m = seg_map<PredT, LabelT>(pred, label, lrs, lps, W, HW, K, ignore_index, flags);
  const PredT* p = static_cast<const PredT*>(pred);
  const LabelT* l = static_cast<const LabelT*>(label);
  unsigned long long* out = reinterpret_cast<unsigned long long*>(matrix);
  if (!in_lds) {
    S2F_LAUNCH(true, true, (seg_conf_global_kernel<PredT, LabelT>), dim3((unsigned)seg_grid(m.ngroups, SEG_THREADS, SEG_MAX_GRID)),
               dim3(SEG_THREADS), 0, stream, p, l, m, out);
    return s2f_check_launch("s2f_seg_confusion");
  }
  const size_t table = (size_t)K * K * sizeof(unsigned int);
  static bool raised = false;          // (per kernel: the 64 KiB default limit on dynamic LDS)
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(seg_conf_lds_kernel<PredT, LabelT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       lds_dev < S2F_SEG_CONF_LDS_BYTES ? lds_dev : S2F_SEG_CONF_LDS_BYTES);
    S2F_REQUIRE(e == hipSuccess, S2F_ELAUNCH, "s2f_seg_confusion: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
    raised = true;
  }
  // resident slots: tables that fit the CU's LDS, at most the two workgroups of 1024 lanes a CU holds
  const int per_cu = (size_t)lds_dev >= 2 * table ? 2 : 1;
  S2F_LAUNCH(true, true, (seg_conf_lds_kernel<PredT, LabelT>),
             dim3((unsigned)seg_grid(m.ngroups, SEG_CONF_THREADS * SEG_CONF_MIN_TRIPS, cus * per_cu)), dim3(SEG_CONF_THREADS), table, stream,
             p, l, m, out);
  return s2f_check_launch("s2f_seg_confusion");
}

// the argument rules both entry points share; `fn` names the entry point in the message, `out` is its accumulator
int seg_check_args(const char* fn, const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                   int64_t label_pixel_stride, int W, int64_t HW, int K, int flags, int known_flags, const void* out, const char* k_why) {
  S2F_REQUIRE(pred && label && out, S2F_EINVAL, "%s: null pointer", fn);
  S2F_REQUIRE(HW > 0 && HW < ((int64_t)1 << 31) - 8, S2F_EINVAL,
              "%s: bad map size HW %lld (1 .. 2^31 - 9: the workgroup counters are 32-bit)", fn, (long long)HW);
  S2F_REQUIRE(W > 0 && HW % W == 0, S2F_EINVAL, "%s: HW %lld is no whole number of rows of W %d", fn, (long long)HW, W);
  S2F_REQUIRE(K > 0 && K <= S2F_SEG_HIST_MAX_CLASSES, S2F_EINVAL, "%s: K %d outside 1 .. %d (%s)", fn, K, S2F_SEG_HIST_MAX_CLASSES, k_why);
  S2F_REQUIRE(pred_dtype == S2F_SEG_PRED_I64 || pred_dtype == S2F_SEG_PRED_F32, S2F_EINVAL, "%s: unknown pred dtype code %d", fn,
              pred_dtype);
  S2F_REQUIRE(label_dtype == S2F_SEG_LABEL_U8 || label_dtype == S2F_SEG_LABEL_I64, S2F_EINVAL, "%s: unknown label dtype code %d", fn,
              label_dtype);
  S2F_REQUIRE((flags & ~known_flags) == 0, S2F_EINVAL, "%s: unknown flags %d", fn, flags);
  S2F_REQUIRE(label_row_stride >= 0 && label_pixel_stride >= 0, S2F_EINVAL, "%s: negative label stride", fn);
  const uintptr_t pa = reinterpret_cast<uintptr_t>(pred), la = reinterpret_cast<uintptr_t>(label), ta = reinterpret_cast<uintptr_t>(out);
  S2F_REQUIRE(pa % (pred_dtype == S2F_SEG_PRED_I64 ? 8 : 4) == 0 && (label_dtype == S2F_SEG_LABEL_U8 || la % 8 == 0) && ta % 8 == 0,
              S2F_EALIGN, "%s: a pointer is not aligned to its element size", fn);
  return S2F_OK;
}

}  // namespace

extern "C" int s2f_seg_hist(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                            int64_t label_pixel_stride, int W, int64_t HW, int K, int ignore_index, int flags, int64_t* totals,
                            void* stream) {
  const int rc = seg_check_args("s2f_seg_hist", pred, pred_dtype, label, label_dtype, label_row_stride, label_pixel_stride, W, HW, K, flags,
                                S2F_SEG_REDUCE_ZERO_LABEL, totals, "the LDS histogram");
  if (rc != S2F_OK) return rc;
  return seg_by_types(pred_dtype, label_dtype, [&](auto p, auto l) {
    return seg_hist_launch<decltype(p), decltype(l)>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, totals,
                                                     (hipStream_t)stream);
  });
}

extern "C" int s2f_seg_confusion(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                                 int64_t label_pixel_stride, int W, int64_t HW, int K, int ignore_index, int flags, int64_t* matrix,
                                 void* stream) {
  const int rc = seg_check_args("s2f_seg_confusion", pred, pred_dtype, label, label_dtype, label_row_stride, label_pixel_stride, W, HW, K,
                                flags, S2F_SEG_REDUCE_ZERO_LABEL | S2F_SEG_CONF_GLOBAL, matrix, "the 16-bit halves of the pair key");
  if (rc != S2F_OK) return rc;
  // the LDS route while the table fits the budget AND what this device offers one workgroup (asked, not assumed)
  const size_t table = (size_t)K * K * sizeof(unsigned int);
  bool in_lds = !(flags & S2F_SEG_CONF_GLOBAL) && table <= (size_t)S2F_SEG_CONF_LDS_BYTES;
  static int lds_dev = 0, cus = 0;          // asked once (one device per process, as resident_blocks of bn_lif.hip)
  if (in_lds) {
    if (cus == 0) {
      int dev = 0, lds = 0, n = 0;
      hipError_t e = hipGetDevice(&dev);
      if (e == hipSuccess) e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
      if (e == hipSuccess) e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
      S2F_REQUIRE(e == hipSuccess && n > 0, S2F_ELAUNCH, "s2f_seg_confusion: cannot query the device: %s", hipGetErrorString(e));
      lds_dev = lds, cus = n;
    }
    in_lds = table <= (size_t)lds_dev;
  }
  return seg_by_types(pred_dtype, label_dtype, [&](auto p, auto l) {
    return seg_conf_launch<decltype(p), decltype(l)>(pred, label, label_row_stride, label_pixel_stride, W, HW, K, ignore_index, flags, matrix,
                                                     in_lds, lds_dev, cus, (hipStream_t)stream);
  });
}
