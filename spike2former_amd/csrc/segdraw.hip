// Segmentation drawing (include/s2f.h "visualisation"): ONE launch blends the class colours of a ground-truth map and / or a
// prediction into a decoded picture and writes the panel(s) side by side -- SegLocalVisualizer._draw_sem_seg and add_datasample's
// np.concatenate (mmseg/visualization/local_visualizer.py:79-118, 218-219) as one streaming pass.  gfx950 only.
//
//   * the arithmetic is the reference's float64 expression, operation for operation: fl64(v * (1 - alpha)), fl64(c * alpha), their
//     fl64 sum, truncation.  THREE separately rounded operations: a fused multiply-add gives another byte at hundreds of the 65 536
//     (v, c) pairs (tests/test_visualizer.py counts them).  hipcc contracts by default, and HIP's __dmul_rn / __dadd_rn do not stop
//     it: they are inline functions compiled under that default, and their product and sum fuse once inlined (seen in this
//     kernel's assembly: v_fma_f64, no v_add_f64).  So the three operations are written out HERE, under s2f_common.h's
//     `#pragma clang fp contract(off)`, which holds for the operations this file spells;
//   * no byte stream here has an alignment: picture b of a staged batch starts at byte 3 h0 w0 b, the right panel of a row at byte
//     3 W of it, and a row of W pixels is 3 W bytes.  A workgroup takes a piece of ONE row, at most DRAW_PIXELS pixels: it loads the
//     aligned 32-bit words that cover the piece's picture bytes into LDS (a word that holds one byte of the picture lies in that
//     byte's page: nothing outside it is touched), every lane blends one pixel out of LDS into LDS, at the byte phase of the
//     panel's destination, and the lanes then store whole aligned 32-bit words; the (at most 3 + 3) bytes of a piece's first and
//     last word that belong to somebody else are peeled: those two words are stored byte by byte;
//   * the maps are read with one element load per lane (1, 4 or 8 bytes, consecutive lanes consecutive elements);
//   * the palette, K x 3 bytes, is packed into K words of LDS once per workgroup; the workgroups stride over the pieces.
//     (A picture narrower than DRAW_PIXELS leaves lanes idle: a piece never spans two rows, since with two panels the rows of the
//     output are not adjacent.)
#include "s2f_common.h"
#include "seg_label.h"

namespace {

constexpr int DRAW_PIXELS = 256;                                   // pixels per piece = lanes per workgroup
constexpr int DRAW_WORDS = (3 + 3 * DRAW_PIXELS + 3) / 4 + 1;      // the aligned words that cover 3 * DRAW_PIXELS bytes at any phase
constexpr int DRAW_MAX_GRID = 2048;                                // 8 workgroups of 256 lanes per CU of the 256-CU part

struct DrawArgs {
  const uint8_t* image;
  const void* gt;
  const void* pred;
  const uint8_t* palette;
  uint8_t* out;
  double keep, alpha;          // keep = fl64(1 - alpha), formed on the host
  int H, W, K, bgr, rzl;
};

// the three blended bytes of one pixel of one panel: kv[ch] = fl64(v[ch] * keep), colour = r | g << 8 | b << 16 (0: no class)
__device__ __forceinline__ void draw_blend(const double (&kv)[3], uint32_t colour, double alpha, uint8_t* __restrict__ dst) {
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double c = (double)((colour >> (8 * ch)) & 0xffu);
    const double ca = c * alpha;
    dst[ch] = (uint8_t)(int)(kv[ch] + ca);
  }
}

template <typename PredT, typename GtT>
__global__ __launch_bounds__(DRAW_PIXELS) void seg_draw_kernel(DrawArgs a) {
  extern __shared__ uint32_t draw_pal[];          // [K] r | g << 8 | b << 16
  __shared__ uint32_t in_w[DRAW_WORDS];
  __shared__ uint32_t out_w[2][DRAW_WORDS];
  const int tid = threadIdx.x;
  const GtT* __restrict__ gt = static_cast<const GtT*>(a.gt);
  const PredT* __restrict__ pred = static_cast<const PredT*>(a.pred);
  const int panels = (gt ? 1 : 0) + (pred ? 1 : 0);
  const int W = a.W, K = a.K;
  for (int k = tid; k < K; k += DRAW_PIXELS)
    draw_pal[k] = (uint32_t)a.palette[3 * k] | ((uint32_t)a.palette[3 * k + 1] << 8) | ((uint32_t)a.palette[3 * k + 2] << 16);

  const int per_row = (W + DRAW_PIXELS - 1) / DRAW_PIXELS;
  const int64_t pieces = (int64_t)a.H * per_row, row_bytes = (int64_t)3 * W * panels;
  const uint8_t* in_b = reinterpret_cast<const uint8_t*>(in_w);
  for (int64_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
    const int64_t r = piece / per_row;
    const int c0 = (int)(piece - r * per_row) * DRAW_PIXELS;
    const int n = min(DRAW_PIXELS, W - c0);
    const int64_t p0 = r * W + c0;          // the piece's first pixel in the picture and the maps
    {
      const uint8_t* src = a.image + 3 * p0;
      const int sh = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
      const uint32_t* src_w = reinterpret_cast<const uint32_t*>(src - sh);
      if (tid < (sh + 3 * n + 3) / 4) in_w[tid] = src_w[tid];          // word t holds picture byte 4 t - sh + {0..3}: one is inside
      __syncthreads();          // (also: the palette is in LDS)
      if (tid < n) {
        const uint8_t* px = in_b + sh + 3 * tid;
        const uint8_t v0 = px[0], v1 = px[1], v2 = px[2];
        const double kv[3] = {(double)(a.bgr ? v2 : v0) * a.keep, (double)v1 * a.keep, (double)(a.bgr ? v0 : v2) * a.keep};
        int q = 0;
        if (gt) {
          int64_t l = (int64_t)gt[p0 + tid];
          if (a.rzl) l = seg_reduce_zero_label(l);
          const int cls = pred_class(l, K);
          const int osh = (int)(reinterpret_cast<uintptr_t>(a.out + r * row_bytes + 3 * c0) & 3u);
          draw_blend(kv, cls >= 0 ? draw_pal[cls] : 0u, a.alpha, reinterpret_cast<uint8_t*>(out_w[0]) + osh + 3 * tid);
          q = 1;
        }
        if (pred) {
          const int cls = pred_class(pred[p0 + tid], K);
          const int osh = (int)(reinterpret_cast<uintptr_t>(a.out + r * row_bytes + (int64_t)3 * W * q + 3 * c0) & 3u);
          draw_blend(kv, cls >= 0 ? draw_pal[cls] : 0u, a.alpha, reinterpret_cast<uint8_t*>(out_w[q]) + osh + 3 * tid);
        }
      }
      __syncthreads();
    }
    for (int q = 0; q < panels; ++q) {
      uint8_t* dst = a.out + r * row_bytes + (int64_t)3 * W * q + 3 * c0;          // 3 n bytes from here are this piece's
      const int osh = (int)(reinterpret_cast<uintptr_t>(dst) & 3u), end = osh + 3 * n;
      uint8_t* dst_al = dst - osh;
      if (tid < (end + 3) / 4) {
        const int lo = 4 * tid;
        if (lo >= osh && lo + 4 <= end) {
          reinterpret_cast<uint32_t*>(dst_al)[tid] = out_w[q][tid];
        } else {          // the first or the last word of the piece: only the bytes inside [osh, end)
          const uint8_t* ob = reinterpret_cast<const uint8_t*>(out_w[q]);
          for (int b = lo; b < lo + 4; ++b)
            if (b >= osh && b < end) dst_al[b] = ob[b];
        }
      }
    }
    // (the next trip writes in_w behind this trip's second barrier and out_w behind its own first one: no third barrier)
  }
}

template <typename PredT, typename GtT>
int seg_draw_launch(const DrawArgs& a, hipStream_t stream) {
  const int64_t pieces = (int64_t)a.H * ((a.W + DRAW_PIXELS - 1) / DRAW_PIXELS);
  const unsigned grid = (unsigned)(pieces < DRAW_MAX_GRID ? pieces : DRAW_MAX_GRID);
  S2F_LAUNCH(true, true, (seg_draw_kernel<PredT, GtT>), dim3(grid), dim3(DRAW_PIXELS), (size_t)a.K * sizeof(uint32_t), stream, a);
  return s2f_check_launch("s2f_seg_draw");
}

}  // namespace

extern "C" int s2f_seg_draw(const uint8_t* image, const void* gt, int gt_dtype, const void* pred, int pred_dtype, const uint8_t* palette,
                            int K, double alpha, int flags, int H, int W, uint8_t* out, void* stream) {
  S2F_REQUIRE(image && palette && out, S2F_EINVAL, "s2f_seg_draw: null pointer (image, palette or out)");
  S2F_REQUIRE(gt || pred, S2F_EINVAL, "s2f_seg_draw: neither a ground-truth map nor a prediction to draw");
  S2F_REQUIRE(H > 0 && W > 0, S2F_EINVAL, "s2f_seg_draw: bad picture size %d x %d", H, W);
  S2F_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 8, S2F_EINVAL, "s2f_seg_draw: bad map size HW %lld (1 .. 2^31 - 9, as s2f_seg_hist)",
              (long long)((int64_t)H * W));
  S2F_REQUIRE(K > 0 && K <= S2F_SEG_HIST_MAX_CLASSES, S2F_EINVAL, "s2f_seg_draw: K %d outside 1 .. %d (the palette in LDS)", K,
              S2F_SEG_HIST_MAX_CLASSES);
  S2F_REQUIRE(alpha >= 0.0 && alpha <= 1.0, S2F_EINVAL, "s2f_seg_draw: alpha %g outside 0 .. 1", alpha);          // (NaN fails both)
  S2F_REQUIRE((flags & ~(S2F_SEG_REDUCE_ZERO_LABEL | S2F_SEG_DRAW_BGR)) == 0, S2F_EINVAL, "s2f_seg_draw: unknown flags %d", flags);
  S2F_REQUIRE(!gt || gt_dtype == S2F_SEG_LABEL_U8 || gt_dtype == S2F_SEG_LABEL_I64, S2F_EINVAL, "s2f_seg_draw: unknown label dtype code %d",
              gt_dtype);
  S2F_REQUIRE(!pred || pred_dtype == S2F_SEG_PRED_I64 || pred_dtype == S2F_SEG_PRED_F32, S2F_EINVAL,
              "s2f_seg_draw: unknown pred dtype code %d", pred_dtype);
  const uintptr_t ga = reinterpret_cast<uintptr_t>(gt), pa = reinterpret_cast<uintptr_t>(pred);
  S2F_REQUIRE((!gt || gt_dtype == S2F_SEG_LABEL_U8 || ga % 8 == 0) && (!pred || pa % (pred_dtype == S2F_SEG_PRED_I64 ? 8 : 4) == 0),
              S2F_EALIGN, "s2f_seg_draw: a map is not aligned to its element size");
  const DrawArgs a{image, gt, pred, palette, out, 1.0 - alpha, alpha, H, W, K, (flags & S2F_SEG_DRAW_BGR) ? 1 : 0,
                   (flags & S2F_SEG_REDUCE_ZERO_LABEL) ? 1 : 0};
  // (an absent map's dtype code is not looked at: its instantiation never reads through the null pointer)
  return seg_by_types(pred ? pred_dtype : S2F_SEG_PRED_I64, gt ? gt_dtype : S2F_SEG_LABEL_U8,
                      [&](auto p, auto l) { return seg_draw_launch<decltype(p), decltype(l)>(a, (hipStream_t)stream); });
}
