// Firing maps (include/s2f.h "firing maps"; gfx950 only): where in the picture a neuron fires.
//
//   s2f_firing_map    one streaming pass over a neuron's output [TB][C][P] (row n of the leading dimension belongs to image n % B)
//                     into four int32 planes per image and pixel: the sum of the integer levels over all (n, c) of the image, the
//                     number of non-zero elements, the maximum level, the number of elements off the level grid.  The level is
//                     census_level.h's, the operand census's definition.
//                     A workgroup of 256 threads OWNS a tile of pixels of one image: it alone reads every (n, c) plane over that
//                     tile and it alone writes the tile's 4 x pixels words -- integer sums, no global atomics, the same bits in
//                     every run.  Consecutive lanes read consecutive pixels of one plane.
//                     WIDE path (P % 4 == 0 and x aligned to four elements: then every plane starts on such a boundary): a lane
//                     takes four consecutive pixels with one 16-byte (fp32) or 8-byte (bf16) load.  SCALAR path (any other P, any
//                     other element offset): one element per lane.
//                     The split rule.  The 256 threads are L pixel lanes x S = 256 / L slices; slice s takes the planes
//                     r = s, s + S, ... of the image's R = (TB / B) C planes (four loads in flight), and the S partial tiles are
//                     combined in LDS -- integer sum, maximum for plane 2 -- by the threads that then store them.  L starts at 256
//                     and is halved while   L > L_min (8 wide: 128 bytes of fp32 per plane row; 64 scalar)   and   2 S <= R
//                     (every slice keeps a plane)   and   either the half tile still covers the whole map or the launch has fewer
//                     than 1024 tiles (four workgroups on each of the 256 CUs).  So a 16 x 16 map of 640 channels runs as 8
//                     lanes x 32 slices per 32-pixel tile, each thread walking 20 planes per time step, not as 512 lanes walking
//                     2 560 each; a 256 x 256 map of 64 channels as 32 lanes x 8 slices, 1 024 tiles for two images.
//                     Per-thread sums are 32-bit: the entry point refuses R * 65535 >= 2^31.
//   s2f_firing_draw   one launch per tile of a panel: resamples one int32 plane [h][w] to the picture's H x W (half-pixel centres,
//                     weights in 1/256), looks the value up in a 256-entry colour table and blends it into the picture -- all in
//                     integer arithmetic, so the bytes have one definition.  No byte stream has an alignment (segdraw.hip's
//                     method): a workgroup takes a piece of ONE row, at most 256 pixels, loads the aligned 32-bit words that cover
//                     the piece's picture bytes into LDS, every lane blends one pixel out of LDS into LDS at the byte phase of its
//                     destination, and the lanes store whole aligned words; the first and the last word of a piece are peeled,
//                     stored byte by byte and only where the byte is the piece's.  Rows of out are out_row_bytes apart.
#include "s2f_common.h"
#include "census_level.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ s2f_firing_map
constexpr int MAP_THREADS = 256;
constexpr int MAP_TARGET_TILES = 1024;
constexpr int MAP_IN_FLIGHT = 4;          // loads a thread issues before it counts the first
constexpr int MAP_MAX_GRID = 1 << 16;          // the workgroups stride over the tiles of a larger launch

struct MapAcc {
  unsigned sum, nonzero, max_level, off;
};

__device__ __forceinline__ void map_one(unsigned bits, float Df, MapAcc& a) {
  const S2fLevel e = s2f_census_level(bits, Df);
  a.sum += e.level;
  a.nonzero += e.nonzero;
  a.max_level = e.level > a.max_level ? e.level : a.max_level;
  a.off += !e.on;
}

// VEC consecutive elements as fp32 bits; `live` false: zeros, which count nothing
template <int VEC>
__device__ __forceinline__ void map_load(const float* src, bool live, unsigned (&bits)[VEC]) {
  if constexpr (VEC == 4) {
    const uint4 w = live ? *reinterpret_cast<const uint4*>(src) : make_uint4(0u, 0u, 0u, 0u);
    bits[0] = w.x, bits[1] = w.y, bits[2] = w.z, bits[3] = w.w;
  } else {
    bits[0] = live ? __float_as_uint(*src) : 0u;
  }
}
template <int VEC>
__device__ __forceinline__ void map_load(const unsigned short* src, bool live, unsigned (&bits)[VEC]) {
  if constexpr (VEC == 4) {          // two per word, the lower address in the low half
    const uint2 w = live ? *reinterpret_cast<const uint2*>(src) : make_uint2(0u, 0u);
    bits[0] = w.x << 16, bits[1] = w.x & 0xffff0000u, bits[2] = w.y << 16,
    bits[3] = w.y & 0xffff0000u;
  } else {
    bits[0] = live ? (unsigned)*src << 16 : 0u;
  }
}

// R = (TB / B) C planes per image; L = 1 << logL pixel lanes, S = MAP_THREADS >> logL slices
template <typename T, int VEC>
__global__ __launch_bounds__(MAP_THREADS) void firing_map_kernel(const T* __restrict__ x, int B, int C, int R, int64_t P, int logL, float Df,
                                                                 int32_t* __restrict__ stats, int assign) {
  __shared__ __attribute__((aligned(16))) uint32_t part[MAP_THREADS * 4 * VEC];          // [slice][plane][pixel of the tile]
  const int tid = threadIdx.x;
  const int L = 1 << logL, S = MAP_THREADS >> logL, TPX = L * VEC;
  const int l = tid & (L - 1), s = tid >> logL;
  const int64_t tiles_per = (P + TPX - 1) / TPX, tiles = tiles_per * B;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int b = (int)(tile / tiles_per);
    const int64_t p0 = (tile - b * tiles_per) * TPX, p = p0 + (int64_t)l * VEC;
    MapAcc a[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) a[k] = MapAcc{0u, 0u, 0u, 0u};
    if (p < P) {          // (wide path: P % 4 == 0, so the four pixels are inside together)
      int t = s / C, c = s - t * C;          // plane r = t C + c of image b is row (t B + b) C + c of x
      for (int r = s; r < R; r += MAP_IN_FLIGHT * S) {
        const T* src[MAP_IN_FLIGHT];
        bool live[MAP_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < MAP_IN_FLIGHT; ++u) {
          live[u] = r + u * S < R;
          src[u] = live[u] ? x + ((int64_t)(t * B + b) * C + c) * P + p : src[0];          // (a dead slot is given a valid address)
          c += S;
          if (c >= C) {
            const int q = c / C;
            t += q, c -= q * C;
          }
        }
        unsigned bits[MAP_IN_FLIGHT][VEC];
#pragma unroll
        for (int u = 0; u < MAP_IN_FLIGHT; ++u) map_load<VEC>(src[u], live[u], bits[u]);
#pragma unroll
        for (int u = 0; u < MAP_IN_FLIGHT; ++u)
#pragma unroll
          for (int k = 0; k < VEC; ++k) map_one(bits[u][k], Df, a[k]);
      }
    }
    {
      uint32_t* mine = part + (size_t)s * 4 * TPX + l * VEC;
      if constexpr (VEC == 4) {
        *reinterpret_cast<uint4*>(mine) = make_uint4(a[0].sum, a[1].sum, a[2].sum, a[3].sum);
        *reinterpret_cast<uint4*>(mine + TPX) =
            make_uint4(a[0].nonzero, a[1].nonzero, a[2].nonzero, a[3].nonzero);
        *reinterpret_cast<uint4*>(mine + 2 * TPX) =
            make_uint4(a[0].max_level, a[1].max_level, a[2].max_level, a[3].max_level);
        *reinterpret_cast<uint4*>(mine + 3 * TPX) = make_uint4(a[0].off, a[1].off, a[2].off, a[3].off);
      } else {
        mine[0] = a[0].sum, mine[TPX] = a[0].nonzero, mine[2 * TPX] = a[0].max_level, mine[3 * TPX] = a[0].off;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < 4 * TPX; idx += MAP_THREADS) {
      const int plane = idx / TPX, px = idx - plane * TPX;          // (TPX is a power of two)
      if (p0 + px >= P) continue;
      uint32_t v = part[plane * TPX + px];
      for (int q = 1; q < S; ++q) {
        const uint32_t o = part[(q * 4 + plane) * TPX + px];
        v = plane == 2 ? (o > v ? o : v) : v + o;
      }
      int32_t* dst = stats + ((int64_t)b * 4 + plane) * P + p0 + px;
      const int32_t nv = (int32_t)v;
      if (assign) {
        *dst = nv;
      } else {
        const int32_t old = *dst;
        *dst = plane == 2 ? (nv > old ? nv : old) : old + nv;
      }
    }
    __syncthreads();          // (the next tile writes part)
  }
}

template <typename T>
int firing_map_launch(const void* x, int TB, int B, int C, int64_t P, int D, int32_t* stats, int assign, hipStream_t stream) {
  const int R = TB / B * C;
  const bool wide = P % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (4 * sizeof(T)) == 0;
  const int vec = wide ? 4 : 1, log_min = wide ? 3 : 6;
  int logL = 8;
  auto tiles = [&](int lg) { return ((P + ((int64_t)vec << lg) - 1) / ((int64_t)vec << lg)) * B; };
  while (logL > log_min && 2 * (MAP_THREADS >> logL) <= R && (((int64_t)vec << (logL - 1)) >= P || tiles(logL) < MAP_TARGET_TILES)) --logL;
  const int64_t n = tiles(logL);
  const unsigned grid = (unsigned)(n < MAP_MAX_GRID ? n : MAP_MAX_GRID);
  if (wide)
    S2F_LAUNCH(true, true, (firing_map_kernel<T, 4>), dim3(grid), dim3(MAP_THREADS), 0, stream, reinterpret_cast<const T*>(x), B, C, R, P, logL,
               (float)D, stats, assign);
  else
    S2F_LAUNCH(true, true, (firing_map_kernel<T, 1>), dim3(grid), dim3(MAP_THREADS), 0, stream, reinterpret_cast<const T*>(x), B, C, R, P, logL,
               (float)D, stats, assign);
  return s2f_check_launch("s2f_firing_map");
}

// ----------------------------------------------------------------------------------------------------------------- s2f_firing_draw
constexpr int DRAW_PIXELS = 256;                                   // pixels per piece = lanes per workgroup = entries of the table
constexpr int DRAW_WORDS = (3 + 3 * DRAW_PIXELS + 3) / 4 + 1;      // the aligned words that cover 3 * DRAW_PIXELS bytes at any phase
constexpr int DRAW_MAX_GRID = 2048;

struct FiringDrawArgs {
  const uint8_t* image;
  const int32_t* plane;
  const uint8_t* lut;
  uint8_t* out;
  int64_t full, out_row_bytes;
  int h, w, H, W, a8, bgr;
};

// output coordinate Z of an axis of `big` samples over a plane axis of `small`: the two plane samples and the weight of the second
// in 1/256 (the half-pixel centres of align_corners=False)
__device__ __forceinline__ void draw_axis(int64_t Z, int64_t small, int64_t big, int& z0, int& z1, int64_t& f) {
  int64_t nz = (2 * Z + 1) * small - big;
  nz = nz < 0 ? 0 : nz;
  const int64_t q = nz / (2 * big);
  f = ((nz - q * 2 * big) * 256) / (2 * big);
  z0 = (int)q;
  z1 = (int)(q + 1 < small ? q + 1 : small - 1);
}

__global__ __launch_bounds__(DRAW_PIXELS) void firing_draw_kernel(FiringDrawArgs a) {
  __shared__ uint32_t lut_w[256];          // r | g << 8 | b << 16
  __shared__ uint32_t in_w[DRAW_WORDS];
  __shared__ uint32_t out_w[DRAW_WORDS];
  const int tid = threadIdx.x;
  const int W = a.W;
  lut_w[tid] = (uint32_t)a.lut[3 * tid] | ((uint32_t)a.lut[3 * tid + 1] << 8) | ((uint32_t)a.lut[3 * tid + 2] << 16);
  const int per_row = (W + DRAW_PIXELS - 1) / DRAW_PIXELS;
  const int64_t pieces = (int64_t)a.H * per_row;
  const uint8_t* in_b = reinterpret_cast<const uint8_t*>(in_w);
  for (int64_t piece = blockIdx.x; piece < pieces; piece += gridDim.x) {
    const int64_t r = piece / per_row;
    const int c0 = (int)(piece - r * per_row) * DRAW_PIXELS;
    const int n = min(DRAW_PIXELS, W - c0);
    uint8_t* dst = a.out + r * a.out_row_bytes + (int64_t)3 * c0;          // 3 n bytes from here are this piece's
    const int osh = (int)(reinterpret_cast<uintptr_t>(dst) & 3u), end = osh + 3 * n;
    const uint8_t* src = a.image + 3 * (r * W + c0);
    const int sh = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
    const uint32_t* src_w = reinterpret_cast<const uint32_t*>(src - sh);
    if (tid < (sh + 3 * n + 3) / 4) in_w[tid] = src_w[tid];          // word t holds picture byte 4 t - sh + {0..3}: one is inside
    __syncthreads();          // (also: the table is in LDS)
    if (tid < n) {
      int y0, y1, x0, x1;
      int64_t fy, fx;
      draw_axis(r, a.h, a.H, y0, y1, fy);
      draw_axis(c0 + tid, a.w, W, x0, x1, fx);
      const int32_t* row0 = a.plane + (int64_t)y0 * a.w;
      const int32_t* row1 = a.plane + (int64_t)y1 * a.w;
      const int64_t s00 = max(0, row0[x0]), s01 = max(0, row0[x1]), s10 = max(0, row1[x0]), s11 = max(0, row1[x1]);
      const int64_t v = (256 - fy) * ((256 - fx) * s00 + fx * s01) + fy * ((256 - fx) * s10 + fx * s11);
      int64_t idx = (255 * v + 32768 * a.full) / (65536 * a.full);
      idx = idx > 255 ? 255 : idx;
      const uint32_t col = lut_w[idx];
      const uint8_t* px = in_b + sh + 3 * tid;
      uint8_t* ob = reinterpret_cast<uint8_t*>(out_w) + osh + 3 * tid;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const uint32_t img = px[a.bgr ? 2 - ch : ch], cc = (col >> (8 * ch)) & 0xffu;
        ob[ch] = (uint8_t)((img * (uint32_t)(256 - a.a8) + cc * (uint32_t)a.a8 + 128u) >> 8);
      }
    }
    __syncthreads();
    uint8_t* dst_al = dst - osh;
    if (tid < (end + 3) / 4) {
      const int lo = 4 * tid;
      if (lo >= osh && lo + 4 <= end) {
        reinterpret_cast<uint32_t*>(dst_al)[tid] = out_w[tid];
      } else {          // the first or the last word of the piece: only the bytes inside [osh, end)
        const uint8_t* ob = reinterpret_cast<const uint8_t*>(out_w);
        for (int bb = lo; bb < lo + 4; ++bb)
          if (bb >= osh && bb < end) dst_al[bb] = ob[bb];
      }
    }
    // (the next trip writes in_w behind this trip's second barrier and out_w behind its own first one: no third barrier)
  }
}

}  // namespace

extern "C" int s2f_firing_map(const void* x, int dtype, int TB, int B, int C, int64_t P, int D, int32_t* stats, int flags, void* stream) {
  S2F_REQUIRE(x && stats, S2F_EINVAL, "s2f_firing_map: null pointer");
  S2F_REQUIRE(TB >= 1 && B >= 1 && C >= 1, S2F_EINVAL, "s2f_firing_map: TB %d, B %d, C %d: each at least 1", TB, B, C);
  S2F_REQUIRE(TB % B == 0, S2F_EINVAL, "s2f_firing_map: TB %d is no multiple of B %d", TB, B);
  S2F_REQUIRE(P >= 0, S2F_EINVAL, "s2f_firing_map: P %lld below 0", (long long)P);
  S2F_REQUIRE(D >= 1, S2F_EINVAL, "s2f_firing_map: D %d below 1", D);
  S2F_REQUIRE(dtype == S2F_CENSUS_F32 || dtype == S2F_CENSUS_BF16, S2F_EINVAL,
              "s2f_firing_map: unknown dtype %d (S2F_CENSUS_F32 = 0, S2F_CENSUS_BF16 = 1)", dtype);
  S2F_REQUIRE((flags & ~S2F_FIRING_MAP_ASSIGN) == 0, S2F_EINVAL, "s2f_firing_map: unknown flags %d", flags);
  S2F_REQUIRE((int64_t)(TB / B) * C * 65535 < ((int64_t)1 << 31), S2F_EINVAL,
              "s2f_firing_map: (TB / B) C = %lld planes per image: their level sum may pass 2^31 (at most 32768 planes)",
              (long long)((int64_t)(TB / B) * C));
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(x) & (dtype == S2F_CENSUS_F32 ? 3u : 1u)) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0,
              S2F_EALIGN, "s2f_firing_map: x must be aligned to its element, stats to 4 bytes");
  if (P == 0) return S2F_OK;
  const int assign = (flags & S2F_FIRING_MAP_ASSIGN) ? 1 : 0;
  if (dtype == S2F_CENSUS_F32) return firing_map_launch<float>(x, TB, B, C, P, D, stats, assign, (hipStream_t)stream);
  return firing_map_launch<unsigned short>(x, TB, B, C, P, D, stats, assign, (hipStream_t)stream);
}

extern "C" int s2f_firing_draw(const uint8_t* image, const int32_t* plane, int h, int w, int64_t full, const uint8_t* lut, int a8, int flags,
                               int H, int W, uint8_t* out, int64_t out_row_bytes, void* stream) {
  S2F_REQUIRE(image && plane && lut && out, S2F_EINVAL, "s2f_firing_draw: null pointer (image, plane, lut or out)");
  S2F_REQUIRE(h > 0 && w > 0 && H > 0 && W > 0, S2F_EINVAL, "s2f_firing_draw: bad sizes: plane %d x %d, picture %d x %d", h, w, H, W);
  S2F_REQUIRE((int64_t)H * W < ((int64_t)1 << 31) - 8 && (int64_t)h * w < ((int64_t)1 << 31), S2F_EINVAL,
              "s2f_firing_draw: picture of %lld or plane of %lld elements: below 2^31 each", (long long)((int64_t)H * W),
              (long long)((int64_t)h * w));
  S2F_REQUIRE(a8 >= 0 && a8 <= 256, S2F_EINVAL, "s2f_firing_draw: a8 %d outside 0 .. 256", a8);
  S2F_REQUIRE(full >= 1 && full <= ((int64_t)1 << 40), S2F_EINVAL, "s2f_firing_draw: full %lld outside 1 .. 2^40", (long long)full);
  S2F_REQUIRE((flags & ~S2F_SEG_DRAW_BGR) == 0, S2F_EINVAL, "s2f_firing_draw: unknown flags %d", flags);
  S2F_REQUIRE(out_row_bytes >= (int64_t)3 * W, S2F_EINVAL, "s2f_firing_draw: out_row_bytes %lld below 3 W = %lld", (long long)out_row_bytes,
              (long long)((int64_t)3 * W));
  S2F_REQUIRE((reinterpret_cast<uintptr_t>(plane) & 3u) == 0, S2F_EALIGN, "s2f_firing_draw: plane is not aligned to 4 bytes");
  const FiringDrawArgs a{image, plane, lut, out, full, out_row_bytes, h, w, H, W, a8, (flags & S2F_SEG_DRAW_BGR) ? 1 : 0};
  const int64_t pieces = (int64_t)H * ((W + DRAW_PIXELS - 1) / DRAW_PIXELS);
  const unsigned grid = (unsigned)(pieces < DRAW_MAX_GRID ? pieces : DRAW_MAX_GRID);
  S2F_LAUNCH(true, true, firing_draw_kernel, dim3(grid), dim3(DRAW_PIXELS), 0, (hipStream_t)stream, a);
  return s2f_check_launch("s2f_firing_draw");
}
