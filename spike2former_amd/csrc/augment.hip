// Training augmentation on the device (include/s2f.h "training augmentation"): the shipped configs' train_pipeline --
// RandomResize(keep_ratio) -> RandomCrop(cat_max_ratio) -> RandomFlip -> PhotoMetricDistortion (mmseg datasets/transforms/
// transforms.py:215-331, 575-737) -- and SegDataPreProcessor (channel swap, (x - mean) / std, pad to `size`) as TWO launches that read
// the batch's raw u8 pictures and annotations and write the step's static [B, 3, Hc, Wc] fp32 / [B, Hc, Wc] u8 inputs.  gfx950 only.
//
//   s2f_aug_crop_stats : one workgroup per (image, candidate crop): the 256-bin label histogram of the candidate's window of the
//                        nearest-resized annotation in LDS, then RandomCrop.crop_bbox's rule -> one pass flag.
//   s2f_aug_apply      : a gather that writes every output element once.  Per output pixel: un-flip, add the chosen origin, the
//                        bilinear sample of the source (resize.hip's axis_taps arithmetic), rintf to u8, the photometric chain with
//                        the reference's quantisation after every stage, channel swap, normalisation.  The chosen candidate comes
//                        from the flags in device memory: nothing is read back by the host between the launches.
//
// The random numbers are drawn on the host (augment.py: TrainAugment.draw) and arrive in the parameter table; the kernels are
// functions of their inputs.  Every float operation below is ONE IEEE fp32 operation (contraction off, correctly rounded divides):
// tests/aug_ref.py restates them in numpy in the same order and the image is compared bit for bit.
//
// The table lives in device memory the host wrote: both kernels treat it as untrusted.  A picture whose offsets or sizes do not fit
// the byte buffer is treated as empty (all padding, every flag 0), origins are clamped into [0, margin] and tap indices into the
// source, so no load leaves `data` whatever the table holds; stores are bounded by the grid alone.
//
// The test pipeline's counterpart (include/s2f.h "test-time views") lives here as well and CALLS what s2f_aug_apply calls -- axis_taps,
// sample_bgr (the interpolation and its rounding), normalise (channel swap, (x - mean) / std), picture_ok and, on the host, prepare
// (the argument checks and the PreConst both kernels take) -- so a picture is resized at test time by the code it was trained on:
//
//   s2f_test_views     : ONE launch for every (view, image) of a test / TTA iteration: keep-ratio Resize, horizontal flip,
//                        channel swap, normalisation and the padding of SegDataPreProcessor's test branch, into blocks of different
//                        sizes packed in one fp32 buffer.  Here the table carries the store addresses too: an entry whose block
//                        does not fit `out` is skipped, so no store leaves `out` either.
#include "s2f_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kStrip = 256, kRowsPerPass = 4, kRowsPerWg = 8;
constexpr int kStatThreads = 1024;
constexpr int kParamWords = (int)(sizeof(S2fAugParams) / 4);
static_assert(sizeof(S2fAugParams) == 160 && sizeof(S2fAugParams) % 8 == 0, "ops/misc.py PARAM_DTYPE mirrors this layout");
static_assert(sizeof(S2fViewParams) == 48 && sizeof(S2fViewParams) % 8 == 0, "ops/misc.py VIEW_PARAM_DTYPE mirrors this layout");

// resize.hip's axis_taps for align_corners = False: scale = in / out, src = max(scale * (o + 0.5) - 0.5, 0)
__device__ __forceinline__ void axis_taps(float scale, int in, int o, int& i0, int& i1, float& l1) {
  float src = scale * ((float)o + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = (int)src;
  if (i0 > in - 1) i0 = in - 1;          // (never for an o inside the resized picture; an untrusted table cannot leave the source)
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
}

// nearest source index of resized index o: floor(o * in / out), 64-bit product
__device__ __forceinline__ int nearest(int o, int in, int out) { return (int)(((int64_t)o * in) / out); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LoadAnnotations(reduce_zero_label=True) on a raw u8 label: the convention of segmetric.hip's seg_key
__device__ __forceinline__ int reduce_label(int l, int rzl) { return rzl ? ((l == 0 || l == 255) ? 255 : l - 1) : l; }

// an h0 x w0 picture resized to H x W fits `data` with 3 bytes per pixel at img_off -- and, where seg_off is given, its annotation
// with 1 byte per pixel there: -> h0 * w0 < 2^31, so every pixel index below fits an int.  (References into the table entry: a
// field is loaded when its test is reached.  docs/EXPERIMENTS.md has the timings of this form and of two others.)
__device__ __forceinline__ bool picture_ok(const int& h0, const int& w0, const int& H, const int& W, const int64_t& img_off,
                                           const int64_t* seg_off, int64_t data_bytes) {
  if (h0 <= 0 || w0 <= 0 || H <= 0 || W <= 0 || img_off < 0 || (seg_off && *seg_off < 0)) return false;
  const int64_t px = (int64_t)h0 * w0;
  return px < ((int64_t)1 << 31) && img_off <= data_bytes - 3 * px && (!seg_off || *seg_off <= data_bytes - px);
}

// the bilinear sample of one pixel of the HWC source rows r0, r1 at the columns x0, x1 (axis_taps), rounded to nearest into u8:
// per channel four products and two sums along the row, two products and a sum across the rows, rintf
__device__ __forceinline__ void sample_bgr(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int x0, int x1, float lx,
                                           float ly, int (&bgr)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = (1.f - lx) * (float)r0[3 * x0 + c] + lx * (float)r0[3 * x1 + c];
    const float bot = (1.f - lx) * (float)r1[3 * x0 + c] + lx * (float)r1[3 * x1 + c];
    bgr[c] = (int)rintf((1.f - ly) * top + ly * bot);
  }
}

// SegDataPreProcessor's constants, as both kernels take them (seg_pad and rzl are the training kernel's alone)
struct PreConst {
  float mean[3], stdv[3];
  float pad_val;
  int swap, seg_pad, rzl;
};

// channel swap and (x - mean) / std of one u8 pixel into column j of a thread's three output planes
__device__ __forceinline__ void normalise(const int (&bgr)[3], const PreConst& k, int j, float (&out)[3][4]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c][j] = ((float)bgr[k.swap ? 2 - c : c] - k.mean[c]) / k.stdv[c];
}

// PhotoMetricDistortion.convert: fp32(img) * alpha + beta, clipped to 0 .. 255, truncated
__device__ __forceinline__ int convert(int u, float alpha, float beta) {
  float f = (float)u * alpha + beta;
  f = fminf(fmaxf(f, 0.f), 255.f);
  return (int)f;
}

// 8-bit HSV: V = max, S = 255 (V - min) / V, hue in 60-degree sectors (V == R, then G, then B), halved into 0 .. 179, each rounded to
// nearest (ties to even)
__device__ __forceinline__ void bgr2hsv(int b, int g, int r, int& h, int& s, int& v) {
  v = max(b, max(g, r));
  const int mn = min(b, min(g, r));
  const float diff = (float)(v - mn);
  s = v == 0 ? 0 : (int)rintf(255.f * diff / (float)v);
  float hf;
  if (v == mn) hf = 0.f;
  else if (v == r) hf = 60.f * (float)(g - b) / diff;
  else if (v == g) hf = 120.f + 60.f * (float)(b - r) / diff;
  else hf = 240.f + 60.f * (float)(r - g) / diff;
  if (hf < 0.f) hf = hf + 360.f;
  h = (int)rintf(hf * 0.5f);
  if (h >= 180) h -= 180;
}

// the standard sector inverse on the 0 .. 255 scale
__device__ __forceinline__ void hsv2bgr(int h, int s, int v, int& b, int& g, int& r) {
  const float vf = (float)v, sf = (float)s / 255.f;
  const float hh = (float)h / 30.f;          // [0, 6)
  int i = (int)hh;
  const float f = hh - (float)i;
  if (i > 5) i = 5;
  const int p = (int)rintf(vf * (1.f - sf));
  const int q = (int)rintf(vf * (1.f - sf * f));
  const int t = (int)rintf(vf * (1.f - sf * (1.f - f)));
  switch (i) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
  }
}

// PhotoMetricDistortion.transform on one u8 BGR pixel; every branch is uniform over the image
__device__ __forceinline__ void photometric(const S2fAugParams& p, int& b, int& g, int& r) {
  if (p.bright_on) {
    b = convert(b, 1.f, p.bright_beta);
    g = convert(g, 1.f, p.bright_beta);
    r = convert(r, 1.f, p.bright_beta);
  }
  if (p.mode == 1 && p.contrast_on) {
    b = convert(b, p.contrast_alpha, 0.f);
    g = convert(g, p.contrast_alpha, 0.f);
    r = convert(r, p.contrast_alpha, 0.f);
  }
  if (p.sat_on) {
    int h, s, v;
    bgr2hsv(b, g, r, h, s, v);
    s = convert(s, p.sat_alpha, 0.f);
    hsv2bgr(h, s, v, b, g, r);
  }
  if (p.hue_on) {
    int h, s, v;
    bgr2hsv(b, g, r, h, s, v);
    h = (h + p.hue_delta) % 180;
    if (h < 0) h += 180;
    hsv2bgr(h, s, v, b, g, r);
  }
  if (p.mode != 1 && p.contrast_on) {
    b = convert(b, p.contrast_alpha, 0.f);
    g = convert(g, p.contrast_alpha, 0.f);
    r = convert(r, p.contrast_alpha, 0.f);
  }
}

__device__ __forceinline__ void load_entry(S2fAugParams* dst, const S2fAugParams* __restrict__ src) {
  if (threadIdx.x < kParamWords) reinterpret_cast<int*>(dst)[threadIdx.x] = reinterpret_cast<const int*>(src)[threadIdx.x];
}

// grid (strips of 256 columns, groups of kRowsPerWg rows, B).  Workgroup = 4 rows x 64 threads as resize_fwd_kernel: a thread
// produces 4 output columns of a row -- with VEC the consecutive columns 4q .. 4q + 3 (one 16-byte store per plane, one 4-byte
// store of the map), otherwise q, q + 64, q + 128, q + 192 (scalar stores, contiguous across the wavefront).
template <bool VEC>
__global__ __launch_bounds__(256) void aug_apply_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                        const S2fAugParams* __restrict__ params, const int* __restrict__ flags,
                                                        int Hc, int Wc, PreConst k, float* __restrict__ inputs,
                                                        uint8_t* __restrict__ seg) {
  __shared__ S2fAugParams sp;
  __shared__ int s_choice;
  __shared__ int sc0[kStrip], sc1[kStrip], ssx[kStrip];
  __shared__ float sl[kStrip];
  const int b = blockIdx.z, tid = threadIdx.x;
  load_entry(&sp, params + b);
  if (tid == 64) {          // RandomCrop.crop_bbox: the first passing candidate among 0 .. 9, else the eleventh
    int c = 0;
    if (flags) {
      c = S2F_AUG_CANDIDATES - 1;
      for (int i = S2F_AUG_CANDIDATES - 2; i >= 0; --i)
        if (flags[b * S2F_AUG_CANDIDATES + i]) c = i;
    }
    s_choice = c;
  }
  __syncthreads();
  const bool ok = picture_ok(sp.h0, sp.w0, sp.H, sp.W, sp.img_off, &sp.seg_off, data_bytes);
  const int h0 = sp.h0, w0 = sp.w0, H = sp.H, W = sp.W;
  const int hv = ok ? min(Hc, H) : 0, wv = ok ? min(Wc, W) : 0;
  const int oy0 = ok ? clampi(sp.crop_y[s_choice], 0, H - hv) : 0, ox0 = ok ? clampi(sp.crop_x[s_choice], 0, W - wv) : 0;
  const float scale_x = ok ? (float)w0 / (float)W : 1.f, scale_y = ok ? (float)h0 / (float)H : 1.f;
  const int strip0 = blockIdx.x * kStrip;
  {
    const int c = strip0 + tid;
    int x0 = 0, x1 = 0, sx = 0;
    float lx = 0.f;
    if (c < wv) {
      const int X = ox0 + (sp.flip ? wv - 1 - c : c);
      axis_taps(scale_x, w0, X, x0, x1, lx);
      sx = min(nearest(X, w0, W), w0 - 1);
    }
    sc0[tid] = x0;
    sc1[tid] = x1;
    ssx[tid] = sx;
    sl[tid] = lx;
  }
  __syncthreads();
  const int q = tid & 63, rsub = tid >> 6;
  auto slot = [&](int j) { return VEC ? 4 * q + j : 64 * j + q; };
  if (strip0 + slot(0) >= Wc) return;
  const uint8_t* img = data + (ok ? sp.img_off : 0);
  const uint8_t* ann = data + (ok ? sp.seg_off : 0);
  const int r_beg = blockIdx.y * kRowsPerWg, r_end = min(Hc, r_beg + kRowsPerWg);
  const int64_t plane = (int64_t)Hc * Wc;
  for (int oy = r_beg + rsub; oy < r_end; oy += kRowsPerPass) {
    const bool row_in = oy < hv;
    int y0 = 0, y1 = 0, sy = 0;
    float ly = 0.f;
    if (row_in) {
      axis_taps(scale_y, h0, oy0 + oy, y0, y1, ly);
      sy = min(nearest(oy0 + oy, h0, H), h0 - 1);
    }
    const uint8_t* r0 = img + (int64_t)y0 * w0 * 3;
    const uint8_t* r1 = img + (int64_t)y1 * w0 * 3;
    const uint8_t* ra = ann + (int64_t)sy * w0;
    float out[3][4];
    int lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = slot(j);
      if (!row_in || strip0 + s >= wv) {
        out[0][j] = out[1][j] = out[2][j] = k.pad_val;
        lab[j] = k.seg_pad;
        continue;
      }
      int bgr[3];
      sample_bgr(r0, r1, sc0[s], sc1[s], sl[s], ly, bgr);
      photometric(sp, bgr[0], bgr[1], bgr[2]);
      normalise(bgr, k, j, out);
      lab[j] = reduce_label(ra[ssx[s]], k.rzl);
    }
    float* o = inputs + ((int64_t)b * 3 * Hc + oy) * Wc + strip0;
    uint8_t* os = seg + ((int64_t)b * Hc + oy) * Wc + strip0;
    if (VEC) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<float4*>(o + c * plane + 4 * q) = make_float4(out[c][0], out[c][1], out[c][2], out[c][3]);
      *reinterpret_cast<uint32_t*>(os + 4 * q) =
          (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (strip0 + slot(j) < Wc) {
#pragma unroll
          for (int c = 0; c < 3; ++c) o[c * plane + slot(j)] = out[c][j];
          os[slot(j)] = (uint8_t)lab[j];
        }
    }
  }
}

// grid (candidates, B), 1024 threads.  LDS: hist[256] | row offsets [hv] | source columns [wv] (both nearest maps are computed once,
// with their 64-bit divisions).  The threads walk the window's pixels tid, tid + 1024, ... (consecutive lanes on consecutive
// columns); a thread counts RUNS of equal labels in registers and adds a run to the LDS histogram when the label changes -- label
// maps are large uniform regions, where one add per pixel would serialise 64 lanes on one address.
__global__ __launch_bounds__(kStatThreads) void aug_crop_stats_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                                     const S2fAugParams* __restrict__ params, int Hc, int Wc,
                                                                     int ignore, int rzl, double max_ratio, int* __restrict__ flags) {
  extern __shared__ int lds[];
  __shared__ S2fAugParams sp;
  __shared__ unsigned int s_sum, s_max, s_present;
  const int cand = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  load_entry(&sp, params + b);
  if (tid < 256) lds[tid] = 0;
  if (tid == 256) s_sum = s_max = s_present = 0;
  __syncthreads();
  const bool ok = picture_ok(sp.h0, sp.w0, sp.H, sp.W, sp.img_off, &sp.seg_off, data_bytes);
  if (!ok) {          // (uniform over the workgroup)
    if (tid == 0) flags[b * S2F_AUG_CANDIDATES + cand] = 0;
    return;
  }
  const int h0 = sp.h0, w0 = sp.w0, H = sp.H, W = sp.W;
  const int hv = min(Hc, H), wv = min(Wc, W);
  const int oy0 = clampi(sp.crop_y[cand], 0, H - hv), ox0 = clampi(sp.crop_x[cand], 0, W - wv);
  unsigned int* hist = reinterpret_cast<unsigned int*>(lds);
  int* rowoff = lds + 256;
  int* col = rowoff + hv;
  for (int i = tid; i < hv; i += kStatThreads) rowoff[i] = min(nearest(oy0 + i, h0, H), h0 - 1) * w0;
  for (int i = tid; i < wv; i += kStatThreads) col[i] = min(nearest(ox0 + i, w0, W), w0 - 1);
  __syncthreads();
  const uint8_t* ann = data + sp.seg_off;
  const int n = hv * wv, dy = kStatThreads / wv, dx = kStatThreads % wv;
  int y = tid / wv, x = tid % wv;
  int cur = -1;
  unsigned int run = 0;
  for (int p = tid; p < n; p += kStatThreads) {
    const int l = reduce_label(ann[rowoff[y] + col[x]], rzl);
    if (l != cur) {
      if (run) atomicAdd(&hist[cur], run);
      cur = l;
      run = 0;
    }
    ++run;
    x += dx;
    y += dy;
    if (x >= wv) {
      x -= wv;
      ++y;
    }
  }
  if (run) atomicAdd(&hist[cur], run);
  __syncthreads();
  if (tid < 256) {
    const unsigned int c = tid == ignore ? 0u : hist[tid];
    if (c) {
      atomicAdd(&s_sum, c);
      atomicMax(&s_max, c);
      atomicAdd(&s_present, 1u);
    }
  }
  __syncthreads();
  // len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < cat_max_ratio: an fp64 quotient of integers, as numpy forms it
  if (tid == 0) flags[b * S2F_AUG_CANDIDATES + cand] = (s_present > 1u && (double)s_max / (double)s_sum < max_ratio) ? 1 : 0;
}

// ---- the test pipeline's views (include/s2f.h "test-time views") ---------------------------------------------------------------
// the entry's block fits `out` and the launch's grid covers it (3 * Hp * Wp <= 3 * 2^24: no overflow)
__device__ __forceinline__ bool view_block_ok(const S2fViewParams& p, int max_hp, int max_wp, int64_t out_elems) {
  if (p.Hp <= 0 || p.Wp <= 0 || p.Hp > max_hp || p.Wp > max_wp || p.out_off < 0 || (p.out_off & 3) != 0) return false;
  return p.out_off <= out_elems - 3 * (int64_t)p.Hp * p.Wp;
}

// grid (tiles of 256 quads, V).  The padded plane of entry v is cut into QUADS of 4 consecutive columns of one row, ceil(Wp / 4) per
// row; a thread produces one quad for the three channels: the row's taps and its two source rows once, one gather of the HWC source
// per output column.  An entry with fewer quads than the grid's widest leaves its surplus workgroups at once.  BASE16: `out` is
// 16-byte aligned, so (out_off % 4 == 0) a block is, and with Wp % 4 == 0 every quad is one 16-byte store per plane.
template <bool BASE16>
__global__ __launch_bounds__(256) void test_views_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                         const S2fViewParams* __restrict__ params, int max_hp, int max_wp,
                                                         PreConst k, float* __restrict__ out, int64_t out_elems) {
  const S2fViewParams p = params[blockIdx.y];          // (uniform over the workgroup)
  if (!view_block_ok(p, max_hp, max_wp, out_elems)) return;
  const int Hp = p.Hp, Wp = p.Wp;
  const int qpr = (Wp + 3) >> 2;
  const int quad = (int)blockIdx.x * 256 + (int)threadIdx.x;          // < 2^22 + 256: max_hp, max_wp <= S2F_AUG_MAX_CROP
  if (quad >= Hp * qpr) return;
  const int oy = quad / qpr, ox = (quad - oy * qpr) * 4;
  const bool ok = p.H <= p.Hp && p.W <= p.Wp && picture_ok(p.h0, p.w0, p.H, p.W, p.img_off, nullptr, data_bytes);
  const int h0 = p.h0, w0 = p.w0, H = ok ? p.H : 0, W = ok ? p.W : 0;
  float o[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[c][j] = k.pad_val;
  if (oy < H && ox < W) {
    const float scale_x = (float)w0 / (float)W, scale_y = (float)h0 / (float)H;
    int y0, y1;
    float ly;
    axis_taps(scale_y, h0, oy, y0, y1, ly);
    const uint8_t* img = data + p.img_off;
    const uint8_t* r0 = img + (int64_t)y0 * w0 * 3;
    const uint8_t* r1 = img + (int64_t)y1 * w0 * 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ox + j >= W) continue;
      int x0, x1;
      float lx;
      axis_taps(scale_x, w0, p.flip ? W - 1 - (ox + j) : ox + j, x0, x1, lx);
      int bgr[3];
      sample_bgr(r0, r1, x0, x1, lx, ly, bgr);
      normalise(bgr, k, j, o);
    }
  }
  const int64_t plane = (int64_t)Hp * Wp;
  float* dst = out + p.out_off + (int64_t)oy * Wp + ox;
  if (BASE16 && (Wp & 3) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ox + j < Wp) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c * plane + j] = o[c][j];
      }
  }
}

// the names an entry point's error texts give its table's length and its output size
struct Names {
  const char *what, *count, *size;
};
constexpr Names kStats = {"s2f_aug_crop_stats", "batch size B", "crop size"}, kApply = {"s2f_aug_apply", "batch size B", "crop size"},
                kViews = {"s2f_test_views", "number of entries V", "largest padded size"};

// what every launcher checks of data, of its n-entry table and of the size H x W its grid is made for
int check_common(const Names& e, const void* data, int64_t data_bytes, const void* params, int n, int H, int W) {
  S2F_REQUIRE(data && params, S2F_EINVAL, "%s: null pointer", e.what);
  S2F_REQUIRE(data_bytes > 0, S2F_EINVAL, "%s: bad byte count %lld", e.what, (long long)data_bytes);
  S2F_REQUIRE(n > 0 && n <= 65535, S2F_EINVAL, "%s: bad %s %d (1 .. 65535)", e.what, e.count, n);
  S2F_REQUIRE(H > 0 && W > 0 && H <= S2F_AUG_MAX_CROP && W <= S2F_AUG_MAX_CROP, S2F_EINVAL, "%s: bad %s %d x %d (1 .. %d)", e.what,
              e.size, H, W, S2F_AUG_MAX_CROP);
  S2F_REQUIRE(reinterpret_cast<uintptr_t>(params) % 8 == 0, S2F_EALIGN, "%s: the parameter table is not 8-byte aligned", e.what);
  return S2F_OK;
}

// s2f_aug_apply's and s2f_test_views' common half: check_common, the fp32 output non-null and aligned, no std of 0 -> the PreConst
int prepare(const Names& e, const void* data, int64_t data_bytes, const void* params, int n, int H, int W, const float* out,
            const float (&mean)[3], const float (&stdv)[3], int bgr_to_rgb, float pad_val, PreConst& k) {
  if (int rc = check_common(e, data, data_bytes, params, n, H, W)) return rc;
  S2F_REQUIRE(out, S2F_EINVAL, "%s: null pointer", e.what);
  S2F_REQUIRE(stdv[0] != 0.f && stdv[1] != 0.f && stdv[2] != 0.f, S2F_EINVAL, "%s: a std of 0 (pass mean 0, std 1 for no normalisation)",
              e.what);
  S2F_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0, S2F_EALIGN, "%s: the fp32 output is not aligned to its element size", e.what);
  k = {{mean[0], mean[1], mean[2]}, {stdv[0], stdv[1], stdv[2]}, pad_val, bgr_to_rgb ? 1 : 0, 0, 0};
  return S2F_OK;
}

}  // namespace

extern "C" int s2f_aug_param_bytes(void) { return (int)sizeof(S2fAugParams); }

extern "C" int s2f_aug_crop_stats(const uint8_t* data, int64_t data_bytes, const S2fAugParams* params, int B, int Hc, int Wc,
                                  int ignore_index, int reduce_zero_label, double cat_max_ratio, int* flags, void* stream) {
  if (int rc = check_common(kStats, data, data_bytes, params, B, Hc, Wc)) return rc;
  S2F_REQUIRE(flags, S2F_EINVAL, "s2f_aug_crop_stats: null pointer");
  S2F_REQUIRE(reinterpret_cast<uintptr_t>(flags) % 4 == 0, S2F_EALIGN, "s2f_aug_crop_stats: flags is not 4-byte aligned");
  const size_t lds = (size_t)(256 + Hc + Wc) * sizeof(int);
  hipLaunchKernelGGL(aug_crop_stats_kernel, dim3(S2F_AUG_CANDIDATES, (unsigned)B), dim3(kStatThreads), lds, (hipStream_t)stream, data,
                     data_bytes, params, Hc, Wc, ignore_index, reduce_zero_label ? 1 : 0, cat_max_ratio, flags);
  return s2f_check_launch("s2f_aug_crop_stats");
}

extern "C" int s2f_aug_apply(const uint8_t* data, int64_t data_bytes, const S2fAugParams* params, const int* flags, int B, int Hc,
                             int Wc, float mean0, float mean1, float mean2, float std0, float std1, float std2, int bgr_to_rgb,
                             float pad_val, int seg_pad_val, int reduce_zero_label, float* inputs, uint8_t* seg, void* stream) {
  PreConst k;
  if (int rc = prepare(kApply, data, data_bytes, params, B, Hc, Wc, inputs, {mean0, mean1, mean2}, {std0, std1, std2}, bgr_to_rgb,
                       pad_val, k))
    return rc;
  S2F_REQUIRE(seg, S2F_EINVAL, "s2f_aug_apply: null pointer");
  S2F_REQUIRE(seg_pad_val >= 0 && seg_pad_val <= 255, S2F_EINVAL, "s2f_aug_apply: seg_pad_val %d is no uint8", seg_pad_val);
  S2F_REQUIRE(reinterpret_cast<uintptr_t>(flags) % 4 == 0, S2F_EALIGN, "s2f_aug_apply: flags is not 4-byte aligned");
  k.seg_pad = seg_pad_val;
  k.rzl = reduce_zero_label ? 1 : 0;
  const dim3 grid((unsigned)((Wc + kStrip - 1) / kStrip), (unsigned)((Hc + kRowsPerWg - 1) / kRowsPerWg), (unsigned)B);
  const bool vec = (Wc % 4) == 0 && s2f_aligned16(inputs) && reinterpret_cast<uintptr_t>(seg) % 4 == 0;
  hipStream_t s = (hipStream_t)stream;
  s2f_dispatch_bool(vec, [&](auto v) {
    hipLaunchKernelGGL((aug_apply_kernel<v.value>), grid, dim3(256), 0, s, data, data_bytes, params, flags, Hc, Wc, k, inputs, seg);
  });
  return s2f_check_launch("s2f_aug_apply");
}

extern "C" int s2f_view_param_bytes(void) { return (int)sizeof(S2fViewParams); }

extern "C" int s2f_test_views(const uint8_t* data, int64_t data_bytes, const S2fViewParams* params, int V, int max_Hp, int max_Wp,
                              float mean0, float mean1, float mean2, float std0, float std1, float std2, int bgr_to_rgb,
                              float pad_val, float* out, int64_t out_elems, void* stream) {
  PreConst k;
  if (int rc = prepare(kViews, data, data_bytes, params, V, max_Hp, max_Wp, out, {mean0, mean1, mean2}, {std0, std1, std2},
                       bgr_to_rgb, pad_val, k))
    return rc;
  S2F_REQUIRE(out_elems > 0, S2F_EINVAL, "s2f_test_views: bad element count %lld", (long long)out_elems);
  const int64_t quads = (int64_t)max_Hp * ((max_Wp + 3) / 4);
  const dim3 grid((unsigned)((quads + 255) / 256), (unsigned)V);
  hipStream_t s = (hipStream_t)stream;
  s2f_dispatch_bool(s2f_aligned16(out), [&](auto a) {
    hipLaunchKernelGGL((test_views_kernel<a.value>), grid, dim3(256), 0, s, data, data_bytes, params, max_Hp, max_Wp, k, out, out_elems);
  });
  return s2f_check_launch("s2f_test_views");
}
