// Sliding-window inference (include/s2f.h "sliding-window inference"): s2f_slide_windows cuts a group of windows out of the input,
// s2f_slide_accumulate merges a group's logits into the full map -- EncoderDecoder.slide_inference's F.pad / preds += / count_mat += 1 /
// preds / count_mat (mmseg/models/segmentors/encoder_decoder.py:246-296) as one gather launch per group.  gfx950 only.
//
//   * the window grid is a function of six integers (SlideGrid); both kernels compute it themselves, there is no table.  Along one
//     axis window i starts at min(i * stride, size - extent): every window but the last starts at i * stride, the last one is
//     shifted back to end at the picture's edge.  The windows that cover a coordinate are therefore a contiguous index range, found
//     in closed form (slide_cover: two integer divisions per axis, whatever the number of windows);
//   * the merge is a GATHER: a lane owns one pixel, adds the covering windows of the group in increasing window index (rows of the
//     grid outside, columns inside: row-major) and divides once when the group holds the pixel's last window.  The reference's
//     scatter adds an exact zero wherever a window does not cover a pixel, so the gather gives the same bits; it starts from +0.0
//     like the reference's zero-filled map (+0.0 + -0.0 = +0.0) when the group holds the pixel's first window, and from the stored
//     value otherwise: preds needs no zero-fill and a pixel the group does not cover is neither read nor written;
//   * lanes run along x: consecutive lanes read consecutive floats of a window row (as long as they share their covering columns:
//     the range changes at a few x per row) and write consecutive floats of a preds row.  A window starts at any column, so a row of
//     it has no alignment beyond its elements': the accesses are one dword per lane, 256 contiguous bytes per wave, and there is
//     nothing to peel;
//   * the row and the row's covering range are uniform per workgroup (blockIdx.y), the column range is per lane, and both are
//     computed once and reused for all the planes (b, k) the lane walks (blockIdx.z strides over them): the stream is
//     n B K eh ew reads plus one read-modify-write of the group's region, and the index arithmetic is off its critical path;
//   * the additions are spelled one by one under s2f_common.h's `#pragma clang fp contract(off)`; the division is IEEE (hipcc's
//     default: correctly rounded fp32 division, no fast-math in FLAGS).
#include "s2f_common.h"

namespace {

constexpr int SLIDE_LANES = 256;          // lanes per workgroup = pixels of one row piece
constexpr int SLIDE_MIN_BLOCKS = 4096;    // 16 workgroups per CU of the 256-CU part before a lane walks more than one plane

struct SlideAxis {
  int size, extent, stride, count;          // picture size, window extent min(crop, size), stride, number of windows
};

struct SlideGrid {
  SlideAxis y, x;
};

__host__ __device__ __forceinline__ int slide_start(const SlideAxis& a, int i) {
  const int s = i * a.stride, last = a.size - a.extent;          // (i < count: i * stride < size + stride, no overflow)
  return s < last ? s : last;
}

// the windows of one axis that cover coordinate p: [lo, hi], empty (lo > hi) where the grid leaves p uncovered
__device__ __forceinline__ void slide_cover(const SlideAxis& a, int p, int& lo, int& hi) {
  const int before = p - a.extent + 1;          // a window starting here or later still covers p
  lo = before <= 0 ? 0 : (before + a.stride - 1) / a.stride;
  hi = p / a.stride;
  if (hi > a.count - 2) hi = a.count - 2;          // windows 0 .. count - 2 start at i * stride ...
  if (p >= a.size - a.extent) {                    // ... and the last one at size - extent
    hi = a.count - 1;
    if (lo > hi) lo = hi;
  }
}

static SlideAxis slide_axis(int size, int crop, int stride) {
  SlideAxis a;
  a.size = size;
  a.extent = crop < size ? crop : size;
  a.stride = stride;
  const int64_t over = (int64_t)size - crop + stride - 1;
  a.count = (int)((over > 0 ? over : 0) / stride) + 1;
  return a;
}

struct SlideArgs {
  SlideGrid g;
  int planes;                  // B * C (B * K)
  int w0, n;                   // the group
  int row0, col0, cols;        // the group's bounding box starts here and is `cols` wide
};

__global__ __launch_bounds__(SLIDE_LANES) void slide_windows_kernel(const float* __restrict__ x, float* __restrict__ out, SlideArgs a) {
  const int c = blockIdx.x * SLIDE_LANES + threadIdx.x, r = blockIdx.y;
  const int ew = a.g.x.extent, eh = a.g.y.extent;
  if (c >= ew) return;
  const int64_t plane_in = (int64_t)a.g.y.size * a.g.x.size, plane_out = (int64_t)eh * ew;
  const int64_t jobs = (int64_t)a.n * a.planes;
  for (int64_t job = blockIdx.z; job < jobs; job += gridDim.z) {          // job = (window of the group, plane)
    const int wi = (int)(job / a.planes), p = (int)(job - (int64_t)wi * a.planes);
    const int j = a.w0 + wi, i = j / a.g.x.count, jx = j - i * a.g.x.count;
    const int y1 = slide_start(a.g.y, i), x1 = slide_start(a.g.x, jx);
    out[job * plane_out + (int64_t)r * ew + c] = x[p * plane_in + (int64_t)(y1 + r) * a.g.x.size + x1 + c];
  }
}

__global__ __launch_bounds__(SLIDE_LANES) void slide_accumulate_kernel(const float* __restrict__ logits, float* __restrict__ preds,
                                                                       SlideArgs a) {
  const int cx = blockIdx.x * SLIDE_LANES + threadIdx.x;
  if (cx >= a.cols) return;
  const int px = a.col0 + cx, py = a.row0 + blockIdx.y;
  int ylo, yhi, xlo, xhi;
  slide_cover(a.g.y, py, ylo, yhi);
  slide_cover(a.g.x, px, xlo, xhi);
  if (ylo > yhi || xlo > xhi) return;          // the grid leaves this pixel uncovered
  const int nx = a.g.x.count, w_end = a.w0 + a.n;
  const int first = ylo * nx + xlo, last = yhi * nx + xhi;          // the first and the last of ALL windows that cover the pixel
  // the group's share: grid rows i0 .. i1 can hold one of its windows (a row-major range of windows is a range of rows)
  const int i0 = max(ylo, a.w0 / nx), i1 = min(yhi, (w_end - 1) / nx);
  bool any = false;
  for (int i = i0; i <= i1 && !any; ++i) {
    const int jl = max(i * nx + xlo, a.w0), jh = min(i * nx + xhi, w_end - 1);
    any = jl <= jh;
  }
  if (!any) return;
  const bool fresh = first >= a.w0, done = last < w_end;          // (groups arrive in increasing w0: first < w0 was merged before)
  const float total = (float)((yhi - ylo + 1) * (xhi - xlo + 1));
  const int ew = a.g.x.extent, eh = a.g.y.extent, W = a.g.x.size;
  const int64_t plane_win = (int64_t)eh * ew, plane_map = (int64_t)a.g.y.size * W, win = plane_win * a.planes;
  float* __restrict__ dst = preds + (int64_t)py * W + px;
  for (int p = blockIdx.z; p < a.planes; p += gridDim.z) {
    float acc = fresh ? 0.0f : dst[p * plane_map];
    for (int i = i0; i <= i1; ++i) {
      const int jl = max(i * nx + xlo, a.w0), jh = min(i * nx + xhi, w_end - 1);
      const int64_t row = (int64_t)(py - slide_start(a.g.y, i)) * ew;
      for (int j = jl; j <= jh; ++j) {
        const float v = logits[(int64_t)(j - a.w0) * win + p * plane_win + row + (px - slide_start(a.g.x, j - i * nx))];
        acc = acc + v;
      }
    }
    if (done) acc = acc / total;
    dst[p * plane_map] = acc;
  }
}

// the argument rules the two entry points share; fills a (grid, group, the group's bounding box)
int slide_args(const char* what, const void* src, const void* dst, int B, int C, int H, int W, int crop_h, int crop_w, int stride_h,
               int stride_w, int w0, int n, SlideArgs& a) {
  S2F_REQUIRE(src && dst, S2F_EINVAL, "%s: null pointer", what);
  S2F_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, S2F_EINVAL, "%s: bad shape (B %d, planes %d, H %d, W %d)", what, B, C, H, W);
  S2F_REQUIRE(crop_h > 0 && crop_w > 0 && stride_h > 0 && stride_w > 0, S2F_EINVAL, "%s: bad window (crop %d x %d, stride %d x %d)", what,
              crop_h, crop_w, stride_h, stride_w);
  S2F_REQUIRE((int64_t)B * C < 65536 && H < 65536, S2F_EINVAL, "%s: B * planes %lld or H %d beyond 65535", what, (long long)B * C, H);
  constexpr int LIM = 1 << 30;          // (coordinate + stride stays a 32-bit int)
  S2F_REQUIRE(W < LIM && crop_h < LIM && crop_w < LIM && stride_h < LIM && stride_w < LIM, S2F_EINVAL,
              "%s: W, crop or stride of 2^30 or more", what);
  S2F_REQUIRE((int64_t)B * C * H * W < ((int64_t)1 << 62) / 4, S2F_EINVAL, "%s: the map does not fit 64-bit byte offsets", what);
  a.g.y = slide_axis(H, crop_h, stride_h);
  a.g.x = slide_axis(W, crop_w, stride_w);
  const int64_t windows = (int64_t)a.g.y.count * a.g.x.count;
  S2F_REQUIRE(windows < ((int64_t)1 << 31), S2F_EINVAL, "%s: %lld windows", what, (long long)windows);
  S2F_REQUIRE(w0 >= 0 && n > 0 && (int64_t)w0 + n <= windows, S2F_EINVAL, "%s: windows %d .. %lld outside the grid's %lld", what, w0,
              (long long)w0 + n - 1, (long long)windows);
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0, S2F_EALIGN,
              "%s: a pointer is not aligned to its fp32 elements", what);
  a.planes = B * C;
  a.w0 = w0;
  a.n = n;
  const int nx = a.g.x.count, i_first = w0 / nx, i_last = (w0 + n - 1) / nx;
  a.row0 = slide_start(a.g.y, i_first);          // (starts do not decrease with the index)
  a.col0 = 0;
  a.cols = W;
  if (i_first == i_last) {                       // a group inside one row of the grid: its columns only
    a.col0 = slide_start(a.g.x, w0 - i_first * nx);
    a.cols = slide_start(a.g.x, w0 + n - 1 - i_first * nx) + a.g.x.extent - a.col0;
  }
  return S2F_OK;
}

unsigned slide_depth(int64_t blocks_xy, int64_t jobs) {          // workgroups along z: enough of them, then a lane walks several jobs
  int64_t z = (SLIDE_MIN_BLOCKS + blocks_xy - 1) / blocks_xy;
  if (z > jobs) z = jobs;
  if (z > 65535) z = 65535;
  return (unsigned)(z < 1 ? 1 : z);
}

}  // namespace

extern "C" int s2f_slide_windows(const float* x, float* out, int B, int C, int H, int W, int crop_h, int crop_w, int stride_h,
                                 int stride_w, int w0, int n, void* stream) {
  SlideArgs a;
  if (int rc = slide_args("s2f_slide_windows", x, out, B, C, H, W, crop_h, crop_w, stride_h, stride_w, w0, n, a)) return rc;
  const unsigned gx = (unsigned)((a.g.x.extent + SLIDE_LANES - 1) / SLIDE_LANES), gy = (unsigned)a.g.y.extent;
  const dim3 grid(gx, gy, slide_depth((int64_t)gx * gy, (int64_t)n * a.planes));
  S2F_LAUNCH(true, true, slide_windows_kernel, grid, dim3(SLIDE_LANES), 0, (hipStream_t)stream, x, out, a);
  return s2f_check_launch("s2f_slide_windows");
}

extern "C" int s2f_slide_accumulate(const float* logits, float* preds, int B, int K, int H, int W, int crop_h, int crop_w, int stride_h,
                                    int stride_w, int w0, int n, void* stream) {
  SlideArgs a;
  if (int rc = slide_args("s2f_slide_accumulate", logits, preds, B, K, H, W, crop_h, crop_w, stride_h, stride_w, w0, n, a)) return rc;
  const int rows = slide_start(a.g.y, (w0 + n - 1) / a.g.x.count) + a.g.y.extent - a.row0;
  const unsigned gx = (unsigned)((a.cols + SLIDE_LANES - 1) / SLIDE_LANES), gy = (unsigned)rows;
  const dim3 grid(gx, gy, slide_depth((int64_t)gx * gy, a.planes));
  S2F_LAUNCH(true, true, slide_accumulate_kernel, grid, dim3(SLIDE_LANES), 0, (hipStream_t)stream, logits, preds, a);
  return s2f_check_launch("s2f_slide_accumulate");
}
