// General bilinear resizing of [planes, h, w] fp32 maps to [planes, H, W] (any sizes, enlarging or shrinking, align_corners False
// or True), its deterministic adjoint, and the inference post-processing around it: arg-max / threshold of the class logits, the
// two fused into one pass that writes the label map alone (s2f_seg_label), and the test-time-augmentation accumulator (mmseg
// segmentors/seg_tta.py:14-48), for gfx950.
//
// Call sites: every bilinear F.interpolate of the predict path that is not the exact-2x even-width case of upsample.hip -- the
// pixel decoder's top-down up-samplings and MaskFormerHead.predict at image sizes that are not multiples of 32 (a 512 x 683
// ADE20K test image gives 32x43 -> 64x86 -> 128x171 -> 256x342 -> 512x683), and EncoderDecoder.postprocess_result's resize to
// `ori_shape` (mmseg segmentors/base.py:127-200).
//
// Arithmetic: ATen's upsample_bilinear2d for an explicit output size, reproduced operation for operation --
//   scale = align_corners ? (in - 1) / (out - 1) (0 for out == 1) : in / out                     (area_pixel_compute_scale)
//   src   = align_corners ? scale * o : max(scale * (o + 0.5) - 0.5, 0)                          (area_pixel_compute_source_index)
//   i0 = (int)src, i1 = i0 + (i0 < in - 1), l = src - i0,  out = (1 - ly)((1 - lx) a + lx b) + ly((1 - lx) c + lx d)
// with contraction off, as upsample.hip::taps (at scale 0.5 the two agree bit for bit).
//
// Every kernel here is a gather that writes each output element once: the write stream bounds it.
#include "s2f_common.h"

#pragma clang fp contract(off)

namespace {

struct Axis {
  float scale;
  int in, out;
  bool align;
};

inline Axis make_axis(int in, int out, bool align) {
  Axis a;
  a.in = in;
  a.out = out;
  a.align = align;
  a.scale = align ? (out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f) : (float)in / (float)out;
  return a;
}

__device__ __forceinline__ void axis_taps(const Axis& a, int o, int& i0, int& i1, float& l1) {
  float src;
  if (a.align) {
    src = a.scale * (float)o;
  } else {
    src = a.scale * ((float)o + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
  }
  i0 = (int)src;
  i1 = i0 + (i0 < a.in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// source window of a plane: logical pixel (r, c) of the (flipped) window reads base[(row0 + r') * ld + col0 + c'] with
// r' = flip_v ? h - 1 - r : r, c' = flip_h ? w - 1 - c : c
struct Window {
  int64_t plane_stride;
  int ld, row0, col0;
  bool flip_h, flip_v;
};

__device__ __forceinline__ int64_t win_row(const Window& wd, int h, int r) {
  return (int64_t)(wd.row0 + (wd.flip_v ? h - 1 - r : r)) * wd.ld;
}
__device__ __forceinline__ int win_col(const Window& wd, int w, int c) { return wd.col0 + (wd.flip_h ? w - 1 - c : c); }

// Forward.  Workgroup = 4 rows x 64 threads, a 256-column strip; a thread produces 4 output columns of a row: with VEC
// (W % 4 == 0) the consecutive columns 4q .. 4q + 3 of the strip (one 16-byte store), otherwise columns q, q + 64, q + 128,
// q + 192 (4 scalar stores, each one contiguous 256-byte run across the wavefront -- four consecutive columns per lane would put
// the lanes' scalar stores 16 bytes apart).  The strip's column taps (source columns of the window, weight) are computed once per
// workgroup into LDS and reused for every row and plane it walks.
constexpr int kStrip = 256, kRowsPerPass = 4;

template <bool VEC, bool SIGMOID>
__global__ __launch_bounds__(256) void resize_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t planes,
                                                         Window wd, int h, int w, int H, int W, Axis ax, Axis ay,
                                                         int rows_per_wg) {
  __shared__ int sc0[kStrip], sc1[kStrip];
  __shared__ float sl[kStrip];
  const int strip0 = blockIdx.x * kStrip;
  {
    const int c = strip0 + (int)threadIdx.x;
    int x0 = 0, x1 = 0;
    float lx = 0.f;
    if (c < W) {
      axis_taps(ax, c, x0, x1, lx);
      x0 = win_col(wd, w, x0);
      x1 = win_col(wd, w, x1);
    }
    sc0[threadIdx.x] = x0;
    sc1[threadIdx.x] = x1;
    sl[threadIdx.x] = lx;
  }
  __syncthreads();
  const int q = threadIdx.x & 63, rsub = threadIdx.x >> 6;
  auto slot = [&](int j) { return VEC ? 4 * q + j : 64 * j + q; };      // the strip column of the thread's j-th output
  if (strip0 + slot(0) >= W) return;
  const int r_beg = blockIdx.y * rows_per_wg, r_end = min(H, r_beg + rows_per_wg);
  for (int64_t p = blockIdx.z; p < planes; p += gridDim.z) {
    const float* base = x + p * wd.plane_stride;
    float* yp = y + p * (int64_t)H * W;
    for (int oy = r_beg + rsub; oy < r_end; oy += kRowsPerPass) {
      int y0, y1;
      float ly;
      axis_taps(ay, oy, y0, y1, ly);
      const float* r0 = base + win_row(wd, h, y0);
      const float* r1 = base + win_row(wd, h, y1);
      float out[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = strip0 + slot(j) < W ? slot(j) : slot(0);
        const int x0 = sc0[s], x1 = sc1[s];
        const float lx = sl[s];
        const float top = (1.f - lx) * r0[x0] + lx * r0[x1];
        const float bot = (1.f - lx) * r1[x0] + lx * r1[x1];
        float v = (1.f - ly) * top + ly * bot;
        out[j] = SIGMOID ? sigmoidf_(v) : v;
      }
      float* o = yp + (int64_t)oy * W + strip0;
      if (VEC) {
        *reinterpret_cast<float4*>(o + 4 * q) = make_float4(out[0], out[1], out[2], out[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (strip0 + slot(j) < W) o[slot(j)] = out[j];
      }
    }
  }
}

// [lo, hi] = the outputs whose taps reach input index i (i0 <= i <= i1; i0 and i1 are non-decreasing in o): a contiguous range
__device__ __forceinline__ void reach(const Axis& a, int i, int& lo, int& hi) {
  int l = 0, r = a.out;                        // first o with i1(o) >= i
  while (l < r) {
    const int m = (l + r) >> 1;
    int i0, i1;
    float l1;
    axis_taps(a, m, i0, i1, l1);
    if (i1 >= i) r = m; else l = m + 1;
  }
  lo = l;
  l = 0, r = a.out;                            // first o with i0(o) > i
  while (l < r) {
    const int m = (l + r) >> 1;
    int i0, i1;
    float l1;
    axis_taps(a, m, i0, i1, l1);
    if (i0 > i) r = m; else l = m + 1;
  }
  hi = l - 1;
}

__device__ __forceinline__ float weight(const Axis& a, int o, int i) {     // d out[o] / d in[i] along one axis
  int i0, i1;
  float l1;
  axis_taps(a, o, i0, i1, l1);
  float r = 0.f;
  if (i0 == i) r += 1.f - l1;
  if (i1 == i) r += l1;
  return r;
}

// Adjoint as a gather (no atomics, a fixed summation order: bit-repeatable).  grid (ceil(h * w / 256), plane groups): the
// thread's two reach ranges are found once and reused for every plane it walks.
//   gx[i][j] = sum_{oy in reach_y(i)} wy(oy, i) * (sum_{ox in reach_x(j)} wx(ox, j) * gy[oy][ox])   (+ add[i][j])
__global__ __launch_bounds__(256) void resize_bwd_kernel(const float* __restrict__ gy, float* __restrict__ gx, int64_t planes,
                                                         int h, int w, int H, int W, Axis ax, Axis ay,
                                                         const float* __restrict__ add) {
  const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
  if (cell >= (uint32_t)h * (uint32_t)w) return;
  const int iy = (int)(cell / (uint32_t)w), ix = (int)(cell - (uint32_t)iy * (uint32_t)w);
  int ylo, yhi, xlo, xhi;
  reach(ay, iy, ylo, yhi);
  reach(ax, ix, xlo, xhi);
  for (int64_t p = blockIdx.y; p < planes; p += gridDim.y) {
    const float* g = gy + p * (int64_t)H * W;
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
      const float wyv = weight(ay, oy, iy);
      const float* row = g + (int64_t)oy * W;
      float s = 0.f;
      for (int ox = xlo; ox <= xhi; ++ox) s += weight(ax, ox, ix) * row[ox];
      acc += wyv * s;
    }
    const int64_t idx = p * (int64_t)h * w + cell;
    gx[idx] = add ? acc + add[idx] : acc;
  }
}

// torch.argmax over the leading K: the first maximum; NaN counts as larger than any number (the first NaN wins)
__device__ __forceinline__ bool beats(float v, float best) { return v > best || (v != v && best == best); }

// Per pixel of a [K, HW] map: DIV > 0 first replaces x[k] by x[k] / DIV in place (the TTA mean, seg_tta.py:38); then K > 1: the
// arg-max into label (int64); K == 1: (SIGMOID ? sigmoid(x) : x) > threshold into label (int64) or label_f (float 0 / 1).
__global__ __launch_bounds__(256) void seg_argmax_kernel(float* __restrict__ x, int64_t* __restrict__ label,
                                                         float* __restrict__ label_f, int K, int64_t HW, int div, int sigmoid,
                                                         float threshold) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (int64_t)gridDim.x * blockDim.x) {
    if (K == 1) {
      float v = x[i];
      if (div > 0) {
        v = v / (float)div;
        x[i] = v;
      }
      if (sigmoid) v = sigmoidf_(v);
      const bool on = v > threshold;
      if (label) label[i] = on ? 1 : 0;
      else label_f[i] = on ? 1.f : 0.f;
      continue;
    }
    float best = 0.f;
    int bi = 0;
    for (int k = 0; k < K; ++k) {
      float v = x[(int64_t)k * HW + i];
      if (div > 0) {
        v = v / (float)div;
        x[(int64_t)k * HW + i] = v;
      }
      if (k == 0 || beats(v, best)) {
        best = v;
        bi = k;
      }
    }
    label[i] = bi;
  }
}

// TTA accumulation: one thread per output pixel of [H, W]; the view's logits x [K] x (window of the padded map) are cropped,
// un-flipped and resized in the same pass (as EncoderDecoder.postprocess_result), then
//   K > 1:  acc[k] (+)= softmax_k(v)  = exp(v_k - max) / sum_j exp(v_j - max)      (three sweeps over K: max, sum, write)
//   K == 1: acc    (+)= sigmoid(PRE ? sigmoid(v) : v)   (seg_tta.py:31-34 applies sigmoid to the post-processed, already sigmoid
//           seg_logits of a one-class model: PRE restates that)
__global__ __launch_bounds__(256) void tta_acc_kernel(const float* __restrict__ x, float* __restrict__ acc, int K, Window wd, int h,
                                                      int w, int H, int W, Axis ax, Axis ay, int first, int pre_sigmoid) {
  const int ox = blockIdx.x * 256 + (int)threadIdx.x;
  const int oy = blockIdx.y;
  if (ox >= W) return;
  int y0, y1, x0, x1;
  float ly, lx;
  axis_taps(ay, oy, y0, y1, ly);
  axis_taps(ax, ox, x0, x1, lx);
  const int64_t r0 = win_row(wd, h, y0), r1 = win_row(wd, h, y1);
  const int c0 = win_col(wd, w, x0), c1 = win_col(wd, w, x1);
  const int64_t HW = (int64_t)H * W, o = (int64_t)oy * W + ox;
  auto val = [&](int k) {
    const float* b = x + (int64_t)k * wd.plane_stride;
    const float top = (1.f - lx) * b[r0 + c0] + lx * b[r0 + c1];
    const float bot = (1.f - lx) * b[r1 + c0] + lx * b[r1 + c1];
    return (1.f - ly) * top + ly * bot;
  };
  if (K == 1) {
    float v = val(0);
    if (pre_sigmoid) v = sigmoidf_(v);
    v = sigmoidf_(v);
    acc[o] = first ? v : acc[o] + v;
    return;
  }
  float m = val(0);
  for (int k = 1; k < K; ++k) m = fmaxf(m, val(k));
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf(val(k) - m);
  for (int k = 0; k < K; ++k) {
    const float pk = expf(val(k) - m) / s;
    float* a = acc + (int64_t)k * HW + o;
    *a = first ? pk : *a + pk;
  }
}

// Label map straight from the padded logits: one thread per output pixel of [H, W], tta_acc_kernel's walk over K.  Each class is
// cropped, un-flipped and interpolated with resize_fwd_kernel's expressions (the same bits), and only the running best is kept:
//   K > 1:  label = the arg-max over K by beats() -- seg_argmax_kernel's rule on values that are never stored;
//   K == 1: sigmoid(v) > threshold into label (int64) or label_f (float 0 / 1).
// What resize_fwd + seg_argmax write and read back as [K, H, W] fp32 planes stays in registers.
__global__ __launch_bounds__(256) void seg_label_kernel(const float* __restrict__ x, int64_t* __restrict__ label,
                                                        float* __restrict__ label_f, int K, Window wd, int h, int w, int H, int W,
                                                        Axis ax, Axis ay, float threshold) {
  const int ox = blockIdx.x * 256 + (int)threadIdx.x;
  const int oy = blockIdx.y;
  if (ox >= W) return;
  int y0, y1, x0, x1;
  float ly, lx;
  axis_taps(ay, oy, y0, y1, ly);
  axis_taps(ax, ox, x0, x1, lx);
  const int64_t r0 = win_row(wd, h, y0), r1 = win_row(wd, h, y1);
  const int c0 = win_col(wd, w, x0), c1 = win_col(wd, w, x1);
  const int64_t o = (int64_t)oy * W + ox;
  auto val = [&](int k) {
    const float* b = x + (int64_t)k * wd.plane_stride;
    const float top = (1.f - lx) * b[r0 + c0] + lx * b[r0 + c1];
    const float bot = (1.f - lx) * b[r1 + c0] + lx * b[r1 + c1];
    return (1.f - ly) * top + ly * bot;
  };
  if (K == 1) {
    const bool on = sigmoidf_(val(0)) > threshold;
    if (label) label[o] = on ? 1 : 0;
    else label_f[o] = on ? 1.f : 0.f;
    return;
  }
  float best = val(0);
  int bi = 0;
#pragma unroll 4
  for (int k = 1; k < K; ++k) {
    const float v = val(k);
    if (beats(v, best)) {
      best = v;
      bi = k;
    }
  }
  label[o] = bi;
}

inline int grid_1d(int64_t total) {
  int64_t b = (total + 255) / 256;
  if (b > 256 * 16) b = 256 * 16;
  return (int)(b < 1 ? 1 : b);
}

int check_window(const char* what, int64_t plane_stride, int ld, int row0, int col0, int h, int w) {
  S2F_REQUIRE(h > 0 && w > 0 && row0 >= 0 && col0 >= 0 && ld >= col0 + w && plane_stride >= (int64_t)(row0 + h) * ld,
              S2F_EINVAL, "%s: bad source window (h %d, w %d, row0 %d, col0 %d, row stride %d, plane stride %lld)", what, h, w, row0,
              col0, ld, (long long)plane_stride);
  return S2F_OK;
}

}  // namespace

extern "C" int s2f_resize_fwd(const float* x, float* y, int64_t planes, int64_t plane_stride, int row_stride, int row0, int col0,
                              int h, int w, int H, int W, int flags, void* stream) {
  S2F_REQUIRE(x && y, S2F_EINVAL, "s2f_resize_fwd: null pointer");
  S2F_REQUIRE(planes > 0 && H > 0 && W > 0 && H < 65536 && W < 65536, S2F_EINVAL, "s2f_resize_fwd: bad shape (planes %lld, H %d, W %d)", (long long)planes,
              H, W);
  S2F_REQUIRE((flags & ~15) == 0, S2F_EINVAL, "s2f_resize_fwd: unknown flags %d", flags);
  if (check_window("s2f_resize_fwd", plane_stride, row_stride, row0, col0, h, w) != S2F_OK) return S2F_EINVAL;
  const bool align = flags & S2F_RESIZE_ALIGN_CORNERS, sig = flags & S2F_RESIZE_SIGMOID;
  Window wd{plane_stride, row_stride, row0, col0, (flags & S2F_RESIZE_FLIP_H) != 0, (flags & S2F_RESIZE_FLIP_V) != 0};
  const Axis ax = make_axis(w, W, align), ay = make_axis(h, H, align);
  const int rows_per_wg = 16;
  const int64_t gz = planes < 65535 ? planes : 65535;
  const dim3 grid((unsigned)((W + kStrip - 1) / kStrip), (unsigned)((H + rows_per_wg - 1) / rows_per_wg), (unsigned)gz);
  const bool vec = (W % 4) == 0 && s2f_aligned16(y);
  hipStream_t s = (hipStream_t)stream;
  s2f_dispatch_bool(vec, [&](auto v) {
    s2f_dispatch_bool(sig, [&](auto sg) {
      S2F_LAUNCH(true, true, (resize_fwd_kernel<v.value, sg.value>), grid, dim3(256), 0, s, x, y, planes, wd, h, w, H, W, ax, ay,
                 rows_per_wg);
    });
  });
  return s2f_check_launch("s2f_resize_fwd");
}

extern "C" int s2f_resize_bwd_add(const float* gy, const float* add, float* gx, int64_t planes, int h, int w, int H, int W, int flags,
                                  void* stream) {
  S2F_REQUIRE(gy && gx, S2F_EINVAL, "s2f_resize_bwd_add: null pointer");
  S2F_REQUIRE(planes > 0 && h > 0 && w > 0 && H > 0 && W > 0 && (int64_t)h * w < ((int64_t)1 << 31), S2F_EINVAL,
              "s2f_resize_bwd_add: bad shape (planes %lld, %d x %d -> %d x %d)", (long long)planes, h, w, H, W);
  S2F_REQUIRE((flags & ~S2F_RESIZE_ALIGN_CORNERS) == 0, S2F_EINVAL, "s2f_resize_bwd_add: only S2F_RESIZE_ALIGN_CORNERS is accepted");
  const bool align = flags & S2F_RESIZE_ALIGN_CORNERS;
  const Axis ax = make_axis(w, W, align), ay = make_axis(h, H, align);
  const int64_t cells = (int64_t)h * w;
  const int64_t gy_ = planes < 65535 ? planes : 65535;
  hipLaunchKernelGGL(resize_bwd_kernel, dim3((unsigned)((cells + 255) / 256), (unsigned)gy_), dim3(256), 0, (hipStream_t)stream, gy,
                     gx, planes, h, w, H, W, ax, ay, add);
  return s2f_check_launch("s2f_resize_bwd_add");
}

extern "C" int s2f_seg_argmax(const float* x, int64_t* label, float* label_f, int K, int64_t HW, int sigmoid, float threshold,
                              void* stream) {
  S2F_REQUIRE(x && (label || label_f), S2F_EINVAL, "s2f_seg_argmax: null pointer");
  S2F_REQUIRE(K > 0 && HW > 0, S2F_EINVAL, "s2f_seg_argmax: bad shape (K %d, HW %lld)", K, (long long)HW);
  S2F_REQUIRE(!(label && label_f) && (K == 1 || label), S2F_EINVAL,
              "s2f_seg_argmax: exactly one output; the float label map is for K == 1 only");
  S2F_LAUNCH(true, true, seg_argmax_kernel, dim3(grid_1d(HW)), dim3(256), 0, (hipStream_t)stream, const_cast<float*>(x), label,
             label_f, K, HW, 0, sigmoid, threshold);
  return s2f_check_launch("s2f_seg_argmax");
}

extern "C" int s2f_tta_accumulate(const float* x, float* acc, int K, int64_t plane_stride, int row_stride, int row0, int col0, int h,
                                  int w, int H, int W, int flags, int first, void* stream) {
  S2F_REQUIRE(x && acc, S2F_EINVAL, "s2f_tta_accumulate: null pointer");
  S2F_REQUIRE(K > 0 && H > 0 && W > 0 && H < 65536, S2F_EINVAL, "s2f_tta_accumulate: bad shape (K %d, H %d, W %d)", K, H, W);
  S2F_REQUIRE((flags & ~15) == 0, S2F_EINVAL, "s2f_tta_accumulate: unknown flags %d", flags);
  if (check_window("s2f_tta_accumulate", plane_stride, row_stride, row0, col0, h, w) != S2F_OK) return S2F_EINVAL;
  const bool align = flags & S2F_RESIZE_ALIGN_CORNERS;
  Window wd{plane_stride, row_stride, row0, col0, (flags & S2F_RESIZE_FLIP_H) != 0, (flags & S2F_RESIZE_FLIP_V) != 0};
  const Axis ax = make_axis(w, W, align), ay = make_axis(h, H, align);
  hipLaunchKernelGGL(tta_acc_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, (hipStream_t)stream, x, acc, K,
                     wd, h, w, H, W, ax, ay, first, (flags & S2F_RESIZE_SIGMOID) ? 1 : 0);
  return s2f_check_launch("s2f_tta_accumulate");
}

extern "C" int s2f_seg_label(const float* x, int64_t* label, float* label_f, int K, int64_t plane_stride, int row_stride, int row0,
                             int col0, int h, int w, int H, int W, int flags, float threshold, void* stream) {
  S2F_REQUIRE(x && (label || label_f), S2F_EINVAL, "s2f_seg_label: null pointer");
  S2F_REQUIRE(K > 0 && H > 0 && W > 0 && H < 65536, S2F_EINVAL, "s2f_seg_label: bad shape (K %d, H %d, W %d)", K, H, W);
  S2F_REQUIRE(!(label && label_f) && (K == 1 || label), S2F_EINVAL,
              "s2f_seg_label: exactly one output; the float label map is for K == 1 only");
  S2F_REQUIRE((flags & ~(S2F_RESIZE_ALIGN_CORNERS | S2F_RESIZE_FLIP_H | S2F_RESIZE_FLIP_V)) == 0, S2F_EINVAL,
              "s2f_seg_label: unknown flags %d (the one-class sigmoid is implied)", flags);
  if (check_window("s2f_seg_label", plane_stride, row_stride, row0, col0, h, w) != S2F_OK) return S2F_EINVAL;
  const bool align = flags & S2F_RESIZE_ALIGN_CORNERS;
  Window wd{plane_stride, row_stride, row0, col0, (flags & S2F_RESIZE_FLIP_H) != 0, (flags & S2F_RESIZE_FLIP_V) != 0};
  const Axis ax = make_axis(w, W, align), ay = make_axis(h, H, align);
  S2F_LAUNCH(true, true, seg_label_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, (hipStream_t)stream, x, label,
             label_f, K, wd, h, w, H, W, ax, ay, threshold);
  return s2f_check_launch("s2f_seg_label");
}

extern "C" int s2f_tta_finish(float* acc, int64_t* label, float* label_f, int K, int64_t HW, int n_views, float threshold,
                              void* stream) {
  S2F_REQUIRE(acc && (label || label_f), S2F_EINVAL, "s2f_tta_finish: null pointer");
  S2F_REQUIRE(K > 0 && HW > 0 && n_views > 0, S2F_EINVAL, "s2f_tta_finish: bad shape (K %d, HW %lld, views %d)", K, (long long)HW,
              n_views);
  S2F_REQUIRE(!(label && label_f) && (K == 1 || label), S2F_EINVAL,
              "s2f_tta_finish: exactly one output; the float label map is for K == 1 only");
  hipLaunchKernelGGL(seg_argmax_kernel, dim3(grid_1d(HW)), dim3(256), 0, (hipStream_t)stream, acc, label, label_f, K, HW, n_views, 0,
                     threshold);
  return s2f_check_launch("s2f_tta_finish");
}
