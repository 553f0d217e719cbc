// Device-side Hungarian assignment of the MaskFormer loss on semantic maps (include/s2f.h "assignment"): what
// loss.MaskFormerLoss.match_tables does on the host with scipy.optimize.linear_sum_assignment, as two launches that never leave the
// stream -- the whole training step fits into one hipGraph (graph.GraphedHungarianStep(assign="device")).  gfx950 only.
//
//   * lsa_init_kernel (one wave): the classes present per image -> num_masks [L] and status bit 0; it WRITES the status word, so
//     no fill precedes a replay.
//   * lsa_solve_kernel: one workgroup of ONE wave64 per (layer, image) problem.  The solver is the shortest-augmenting-path
//     algorithm of Crouse (2016), "On implementing 2D rectangular assignment algorithms" (the Jonker-Volgenant variant scipy
//     uses): the matrix is oriented so that rows <= columns, every row is augmented once along a shortest path found by a
//     Dijkstra-like scan, the duals u / v are updated after each augmentation.  All arithmetic is fp64 on the fp32 costs, every
//     expression in the order of the textbook form ((minVal + c) - u) - v, so that on matrices without ties the assignment is the one
//     scipy returns.
//   * the scan is a serial chain of "relax every unscanned column against one row, take the minimum": columns are striped over
//     the lanes (column j = slot * 64 + lane, at most LSA_SLOTS = 4 slots = 256 columns), their state (shortest path cost, dual v,
//     scanned bit, owner row, list position) lives in registers, the minimum is a wave reduction on the DPP path.  Row state (dual
//     u, col4row) and the predecessor list are small LDS arrays; there is one wave, so the barriers are compiler fences around
//     the serial parts.
//   * ties.  Costs that are fp32 numbers tie exactly more often than one expects (100 queries whose costs differ by 1e-4 share ~400
//     fp32 values per column), and among equal minima the textbook scan takes the first column of its list of unscanned columns,
//     or the last UNASSIGNED one if there is one; the list starts as nc - 1 .. 0 and a scanned column is replaced by the list's
//     last.  Each lane keeps the list position of its columns (a scanned column's place goes to whichever lane holds the last
//     position) and the second reduction's key is that order -- a function of the algorithm's state, not of the lane layout.  With
//     it the tables are scipy's bit for bit on tied matrices too (integer costs, constant matrices: tests/test_gpu_lsa.py).
//   * the compacted, oriented cost tile is converted to fp64 ONCE into LDS (Q x n_present x 8 B: 120 000 B at Q = 100, n = 150,
//     of the CU's 160 KiB) -- problems whose tile does not fit (Q * n_present > LSA_TILE) re-read the fp32 costs from L2 through
//     the same column table (measured at Q = 100: LDS 23 / 75 / 260 / 4 226 us against L2 25 / 84 / 290 / 5 033 us for 14 problems
//     at n = 10 / 40 / 150 / 150 with every query alike, docs/EXPERIMENTS.md); s2f_lsa_tables_ex with S2F_LSA_TILE_L2 forces that form (the measurement of tools/probe_lsa.py).
//   * EVERY loop has a structural bound: a scan visits at most nc columns, a path has at most nr rows, there are nr augmentations.
//     Non-finite costs in a present column are found while the tile is loaded, before the solver runs: status bit 1, the problem's
//     rows "unmatched", num_masks[l] = NaN.  Nothing here can spin on NaN / Inf input.
#include "s2f_common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LSA_SLOTS = 4;
constexpr int LSA_MAX = LSA_SLOTS * S2F_WAVE;          // rows / columns of the oriented problem (include/s2f.h S2F_LSA_MAX_QUERIES)
constexpr int LSA_TILE = 15000;                        // fp64 elements of the LDS cost tile (100 x 150)

static_assert(S2F_LSA_MAX_QUERIES == LSA_MAX && S2F_LSA_MAX_CLASSES < LSA_MAX, "the column striping holds 256 columns");

// Minimum over the 64 lanes on the DPP path, the pattern of s2f_wave_sum_lane63 (prefix inside rows of 16, then row_bcast 15 / 31)
// with a lane's own value as the fill of lanes that have no source: min(v, v) = v.  The result is in lane 63 and read from there.
#define LSA_DPP_MIN_I32(v, ctrl, rows) v = min(v, __builtin_amdgcn_update_dpp(v, v, ctrl, rows, 0xf, false))
#define LSA_DPP_MIN_F64(v, ctrl, rows)                                                  \
  do {                                                                                  \
    const int lo_ = __double2loint(v), hi_ = __double2hiint(v);                         \
    const int lo2_ = __builtin_amdgcn_update_dpp(lo_, lo_, ctrl, rows, 0xf, false);     \
    const int hi2_ = __builtin_amdgcn_update_dpp(hi_, hi_, ctrl, rows, 0xf, false);     \
    v = fmin(v, __hiloint2double(hi2_, lo2_));                                          \
  } while (0)

__device__ __forceinline__ int lsa_wave_min(int v) {
  LSA_DPP_MIN_I32(v, 0x111, 0xf);
  LSA_DPP_MIN_I32(v, 0x112, 0xf);
  LSA_DPP_MIN_I32(v, 0x114, 0xf);
  LSA_DPP_MIN_I32(v, 0x118, 0xf);
  LSA_DPP_MIN_I32(v, 0x142, 0xa);
  LSA_DPP_MIN_I32(v, 0x143, 0xc);
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ double lsa_wave_min(double v) {
  LSA_DPP_MIN_F64(v, 0x111, 0xf);
  LSA_DPP_MIN_F64(v, 0x112, 0xf);
  LSA_DPP_MIN_F64(v, 0x114, 0xf);
  LSA_DPP_MIN_F64(v, 0x118, 0xf);
  LSA_DPP_MIN_F64(v, 0x142, 0xa);
  LSA_DPP_MIN_F64(v, 0x143, 0xc);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

__device__ __forceinline__ bool lsa_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// num_masks[l] = sum over the images of max(min(Q, n_present), 1) (the same for every l), NaN with a label in K..254 present;
// status = bit 0 of that.  The solver's workgroups OR bit 1 into the word this kernel has written.
__global__ __launch_bounds__(S2F_WAVE) void lsa_init_kernel(const float* __restrict__ count_full, float* __restrict__ num_masks,
                                                            int32_t* __restrict__ status, int L, int B, int Q, int K) {
  const int lane = threadIdx.x;
  float acc = 0.0f;
  bool bad = false;
  for (int b = 0; b < B; ++b) {
    const float* cnt = count_full + (size_t)b * 256;
    int n = 0;
#pragma unroll
    for (int s = 0; s < LSA_SLOTS; ++s) {
      const int k = s * S2F_WAVE + lane;          // < 256: inside the row
      const bool nz = cnt[k] != 0.0f;
      n += __popcll(__ballot(nz && k < K));
      bad = bad || (nz && k >= K && k < 255);
    }
    acc += (float)max(min(Q, n), 1);
  }
  const bool any_bad = __ballot(bad) != 0;
  for (int l = lane; l < L; l += S2F_WAVE) num_masks[l] = any_bad ? __int_as_float(0x7fc00000) : acc;
  if (lane == 0) status[0] = any_bad ? 1 : 0;
}

__global__ __launch_bounds__(S2F_WAVE) void lsa_solve_kernel(const float* __restrict__ cost, const float* __restrict__ count_full,
                                                             int64_t* __restrict__ tgt_labels, int32_t* __restrict__ row_class,
                                                             float* __restrict__ num_masks, int32_t* __restrict__ status, int L, int B,
                                                             int Q, int K, int force_l2) {
  __shared__ double tile[LSA_TILE];
  __shared__ double u[LSA_MAX];
  __shared__ int col4row[LSA_MAX], row4col[LSA_MAX], path[LSA_MAX], present[LSA_MAX];
  const int lane = threadIdx.x;
  const int l = blockIdx.x / B, b = blockIdx.x - l * B;
  const float* __restrict__ c0 = cost + (size_t)blockIdx.x * Q * K;          // cost[l][b]
  const float* __restrict__ cnt = count_full + (size_t)b * 256;
  const double INF = __longlong_as_double(0x7ff0000000000000ll);

  // the classes present, ascending, as the column list
  int n = 0;
#pragma unroll
  for (int s = 0; s < LSA_SLOTS; ++s) {
    const int k = s * S2F_WAVE + lane;
    const bool p = k < K && cnt[k] != 0.0f;
    const unsigned long long m = __ballot(p);
    if (p) present[n + __popcll(m & ((1ull << lane) - 1ull))] = k;
    n += __popcll(m);
  }
  __syncthreads();

  // orientation: rows <= columns (the transposed problem has the classes as rows)
  const bool tr = n < Q;
  const int nr = tr ? n : Q, nc = tr ? Q : n;
  const bool in_lds = !force_l2 && nr * nc <= LSA_TILE;
  bool fin = true;
  constexpr int LOADS = 8;          // independent loads in flight per lane: the tile is 235 dependent round trips to L2 otherwise
  for (int e0 = lane; e0 < nr * nc; e0 += LOADS * S2F_WAVE) {
    float x[LOADS];
#pragma unroll
    for (int t = 0; t < LOADS; ++t) {
      const int e = e0 + t * S2F_WAVE;
      x[t] = 0.0f;
      if (e < nr * nc) {
        const int i = e / nc, j = e - i * nc;
        x[t] = c0[(tr ? j : i) * K + present[tr ? i : j]];
      }
    }
#pragma unroll
    for (int t = 0; t < LOADS; ++t) {
      const int e = e0 + t * S2F_WAVE;
      fin = fin && lsa_finite(x[t]);
      if (in_lds && e < nr * nc) tile[e] = (double)x[t];
    }
  }
  bool ok = __ballot(!fin) == 0;

  if (ok && n > 0) {
    for (int i = lane; i < LSA_MAX; i += S2F_WAVE) {
      u[i] = 0.0;
      col4row[i] = row4col[i] = path[i] = -1;
    }
    double v[LSA_SLOTS];
    int colbase[LSA_SLOTS];          // the L2 form: element (i, j) is c0[rowoff(i) + colbase(j)]
#pragma unroll
    for (int s = 0; s < LSA_SLOTS; ++s) {
      const int j = s * S2F_WAVE + lane;
      v[s] = 0.0;
      colbase[s] = j < nc ? (tr ? j * K : present[j]) : 0;
    }
    __syncthreads();

    for (int cur = 0; cur < nr; ++cur) {          // one augmentation per row
      double spc[LSA_SLOTS];                      // shortest path cost to each of this lane's columns
      int r4c[LSA_SLOTS];                         // their owner rows (row4col changes between augmentations only)
#pragma unroll
      for (int s = 0; s < LSA_SLOTS; ++s) {
        spc[s] = INF;
        r4c[s] = row4col[s * S2F_WAVE + lane];
      }
      int pos[LSA_SLOTS];                         // position of the column in the textbook's list of unscanned columns
#pragma unroll
      for (int s = 0; s < LSA_SLOTS; ++s) pos[s] = nc - 1 - (s * S2F_WAVE + lane);
      int remaining = nc;
      unsigned scanned = 0;
      double min_val = 0.0;
      int i = cur, sink = -1;
      for (int it = 0; it < nc; ++it) {           // each trip scans one more column: at most nc
        const double ui = u[i];
        const int rowoff = in_lds ? i * nc : (tr ? present[i] : i * K);
        double best = INF;
#pragma unroll
        for (int s = 0; s < LSA_SLOTS; ++s) {
          const int j = s * S2F_WAVE + lane;
          if (j < nc && !((scanned >> s) & 1u)) {
            const double cij = in_lds ? tile[rowoff + j] : (double)c0[rowoff + colbase[s]];
            double r = min_val + cij;
            r = r - ui;
            r = r - v[s];
            if (r < spc[s]) {
              spc[s] = r;
              path[j] = i;
            }
            best = fmin(best, spc[s]);
          }
        }
        const double lowest = lsa_wave_min(best);
        if (!(lowest < INF)) break;               // (finite costs cannot get here)
        // among the columns at the minimum: the LAST unassigned one of the list, else the FIRST one of the list (see the header)
        int key = INT_MAX;
#pragma unroll
        for (int s = 0; s < LSA_SLOTS; ++s) {
          const int j = s * S2F_WAVE + lane;
          if (j < nc && !((scanned >> s) & 1u) && spc[s] == lowest)
            key = min(key, ((r4c[s] < 0 ? nc - 1 - pos[s] : LSA_MAX + pos[s]) << 8) | j);
        }
        key = lsa_wave_min(key);
        if (key == INT_MAX) break;
        const int jstar = key & (LSA_MAX - 1), prio = key >> 8;
        min_val = lowest;
        if (lane == (jstar & (S2F_WAVE - 1))) scanned |= 1u << (jstar >> 6);
        // the list's last column moves into the place of the scanned one
        const int hole = prio < LSA_MAX ? nc - 1 - prio : prio - LSA_MAX;
        --remaining;
#pragma unroll
        for (int s = 0; s < LSA_SLOTS; ++s)
          if (!((scanned >> s) & 1u) && pos[s] == remaining) pos[s] = hole;
        if (prio < LSA_MAX) {                     // an unassigned column: the path ends here
          sink = jstar;
          break;
        }
        i = __builtin_amdgcn_readfirstlane(row4col[jstar]);
      }
      if (sink < 0) {
        ok = false;
        break;
      }
      __syncthreads();
      // duals: u[cur] += minVal; for every scanned column j but the sink, with its owner row i (col4row[i] == j):
      // u[i] += minVal - spc[j], v[j] -= minVal - spc[j]   (the sink's own difference is zero)
      if (lane == 0) u[cur] += min_val;
#pragma unroll
      for (int s = 0; s < LSA_SLOTS; ++s) {
        if (((scanned >> s) & 1u) && r4c[s] >= 0) {
          const double d = min_val - spc[s];
          u[r4c[s]] += d;
          v[s] -= d;
        }
      }
      // augment along the predecessor list: at most one step per row
      if (lane == 0) {
        int j = sink;
        for (int step = 0; step < nr; ++step) {
          if ((unsigned)j >= (unsigned)nc) break;
          const int ip = path[j];
          if ((unsigned)ip >= (unsigned)nr) break;
          row4col[j] = ip;
          const int t = col4row[ip];
          col4row[ip] = j;
          j = t;
          if (ip == cur) break;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();

  for (int q = lane; q < Q; q += S2F_WAVE) {
    int cls = -1;
    if (ok && n > 0) {
      const int c = tr ? row4col[q] : col4row[q];          // transposed: the columns are the queries
      if (c >= 0) cls = present[c];
    }
    tgt_labels[(size_t)blockIdx.x * Q + q] = cls >= 0 ? (int64_t)cls : (int64_t)K;
    row_class[((size_t)b * L + l) * Q + q] = cls;
  }
  if (!ok && lane == 0) {
    atomicOr(reinterpret_cast<int*>(status), 2);
    num_masks[l] = __int_as_float(0x7fc00000);
  }
}

}  // namespace

extern "C" int s2f_lsa_tables_ex(const float* cost, const float* count_full, int64_t* tgt_labels, int32_t* row_class, float* num_masks,
                                 int32_t* status, int L, int B, int Q, int K, int flags, void* stream) {
  S2F_REQUIRE((flags & ~S2F_LSA_TILE_L2) == 0, S2F_EINVAL, "s2f_lsa_tables: unknown flags %d", flags);
  S2F_REQUIRE(cost && count_full && tgt_labels && row_class && num_masks && status, S2F_EINVAL, "s2f_lsa_tables: null pointer");
  S2F_REQUIRE(L >= 1 && B >= 1 && Q >= 1, S2F_EINVAL, "s2f_lsa_tables: L %d, B %d, Q %d must be positive", L, B, Q);
  S2F_REQUIRE(K >= 1 && K <= S2F_LSA_MAX_CLASSES, S2F_EINVAL,
              "s2f_lsa_tables: K %d outside 1 .. %d (255 is the ignored label)", K, S2F_LSA_MAX_CLASSES);
  S2F_REQUIRE(Q <= S2F_LSA_MAX_QUERIES, S2F_EINVAL, "s2f_lsa_tables: Q %d above %d (4 columns per lane of one wave)", Q,
              S2F_LSA_MAX_QUERIES);
  S2F_REQUIRE((int64_t)L * B <= (1 << 20), S2F_EINVAL, "s2f_lsa_tables: L * B %lld above 2^20 problems", (long long)L * B);
  S2F_REQUIRE(reinterpret_cast<uintptr_t>(cost) % 4 == 0 && reinterpret_cast<uintptr_t>(count_full) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(tgt_labels) % 8 == 0 && reinterpret_cast<uintptr_t>(row_class) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(num_masks) % 4 == 0 && reinterpret_cast<uintptr_t>(status) % 4 == 0,
              S2F_EALIGN, "s2f_lsa_tables: a pointer is not aligned to its element size");
  const int force_l2 = (flags & S2F_LSA_TILE_L2) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  S2F_LAUNCH(true, false, lsa_init_kernel, dim3(1), dim3(S2F_WAVE), 0, st, count_full, num_masks, status, L, B, Q, K);
  S2F_LAUNCH(false, true, lsa_solve_kernel, dim3((unsigned)(L * B)), dim3(S2F_WAVE), 0, st, cost, count_full, tgt_labels, row_class,
             num_masks, status, L, B, Q, K, force_l2);
  return s2f_check_launch("s2f_lsa_tables");
}

extern "C" int s2f_lsa_tables(const float* cost, const float* count_full, int64_t* tgt_labels, int32_t* row_class, float* num_masks,
                              int32_t* status, int L, int B, int Q, int K, void* stream) {
  return s2f_lsa_tables_ex(cost, count_full, tgt_labels, row_class, num_masks, status, L, B, Q, K, 0, stream);
}
