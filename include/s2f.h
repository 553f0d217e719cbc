/*
 * s2f.h -- C ABI of libs2f_hip.so: the MI355X (gfx950) kernels of the Spike2Former hot path.
 *
 * Conventions (every entry point):
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross this boundary.
 *   - all pointers are DEVICE pointers owned by the caller; nothing is allocated or freed inside;
 *     `?` in a comment marks a nullable pointer.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); launches are asynchronous.
 *   - return value: S2F_OK (0) or a negative S2F_E* code; `s2f_last_error()` gives the text.
 *   - re-entrant, no global state apart from the thread-local error string and the thread-local launch-timing arm.
 *
 * The reference (BICLab/Spike2Former) has no FFI on its live path -- everything is ATen ops called from
 * Python.  The in-tree precedents this ABI follows are the (dormant) pybind pair
 * `dcnv3_forward/backward` (ops_dcnv3/src/vision.cpp:14-17, argument list src/dcnv3.h:20-59) and the cupy
 * raw-pointer launch convention (Qtrick_architecture/clock_driven/cu_kernel_opt.py:53-71).  Each function
 * below names the reference code it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 */
#ifndef S2F_H
#define S2F_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2F_OK 0
#define S2F_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unsupported geometry) */
#define S2F_EALIGN (-2)   /* pointer not aligned as required */
#define S2F_ELAUNCH (-3)  /* hipLaunch / runtime error */

#define S2F_ABI_VERSION 56
#define S2F_STAT_SLOTS 256

int s2f_version(void);
const char* s2f_last_error(void);

/* ---- measurement: kernel-timestamp timing of one call ------------------------------------------------
 * bench.py's roofline figures need the duration of individual launches.  Two hipEventRecord markers around a launch
 * add ~4 us of command-processor time to a ~10 us kernel; instead the launch itself carries the events
 * (hipExtLaunchKernelGGL start/stop events = the dispatch packet's own begin/end timestamps, what rocprofv3 reports).
 *   s2f_event_create/destroy: a hipEvent_t as void*.
 *   s2f_time_next_call(start, stop): arms THIS thread; the next s2f_lif_fwd / s2f_lif_bwd / s2f_bn_stats /
 *       s2f_bn_act_fwd / s2f_bn_act_bwd / s2f_spike_gemm_fwd / s2f_spike_gemm_dw / s2f_spike_conv3x3_* / s2f_split_gemm / s2f_seg_hist / s2f_seg_confusion / s2f_seg_draw / s2f_slide_windows / s2f_slide_accumulate / s2f_state_copy call stamps `start` with the begin of
 *       its first kernel and `stop` with the end of its last one, then disarms.  Not valid during stream capture.
 *   s2f_event_elapsed_us: stop - start in microseconds (both must have completed: synchronise first). */
void* s2f_event_create(void);
void s2f_event_destroy(void* event);
int s2f_time_next_call(void* start_event, void* stop_event);
int s2f_event_elapsed_us(void* start_event, void* stop_event, double* microseconds);

/* Number of uint64 words of the in-range bitmask for n elements: 4 words per 256-element tile.
 * Tile i covers elements [256 i, 256 i + 256); word j (0..3) bit l (0..63) belongs to element 256 i + 4 l + j
 * (lane l of a wavefront holds 4 consecutive elements; word j is the wave ballot of component j). */
int64_t s2f_lif_mask_words(int64_t n);

/* ---- a1/a2: Q_IFNode.forward + quant STE ------------------------------------------------------------
 * Replaces BaseNode.forward (Qtrick_architecture/clock_driven/neuron.py:166-197; charge :459-460, soft reset
 * :133-153) with `quant` (surrogate.py:522-538) as surrogate:
 *     h = v_in + x ; s = rint(clamp(h, 0, D)) (round-half-even) ; v_out = h - s*vth ; y = s / D
 *     mask bit = (0 <= h <= D)                          (what the STE backward needs instead of fp32 h)
 * v_in? NULL == membrane freshly reset (python float 0.).  v_out? NULL == membrane not kept.
 * mask? NULL == no backward wanted.  count_u8? NULL == integer counts not wanted.
 * stats? : uint64[S2F_STAT_SLOTS][2], atomically accumulated {sum of counts s, number of non-zero s}; the caller sums the
 *          slots (cal_firing_num.py:138-160 accumulates mean(y*D) = sum(stats[.][0])/n; firing_utils non-zero rate =
 *          sum(stats[.][1])/n).  Workgroup b adds into slot b % S2F_STAT_SLOTS: with ONE pair of counters the 2 048
 *          workgroups of a launch serialise on two L2 atomics (measured 52 us on a 5 us kernel).
 * x, y, v_* need 16-byte alignment when n >= 4.
 * y_bf16 != 0: y points to uint16 storage and the spikes are written as bf16 -- exact (a spike has <= 8 significant bits),
 *   2 bytes / element instead of the reference's 4; what the *_bf16 GEMM / attention entry points consume. */
int s2f_lif_fwd(const float* x, const float* v_in, void* y, float* v_out, uint64_t* mask, uint8_t* count_u8,
                uint64_t* stats, int64_t n, float vth, int D, int y_bf16, void* stream);

/* STE backward of one step:  gx = gv_out + (gy / D - gv_out * vth) * m   (gv_out? NULL == 0; dL/dv_in == gx). */
int s2f_lif_bwd(const float* gy, const float* gv_out, const uint64_t* mask, float* gx, int64_t n, float vth, int D,
                void* stream);
/* The same with the gradient sums of a fan-out folded in (each NULL = absent): gy2? = the gradient a SECOND consumer of the spike
 * map sends back, skip? = the gradient of a residual branch that read the neuron's INPUT (x + f(Q_IFNode(x)), sdtv2.py:203-219,
 * detr_layers.py:523-556):  gx = STE((gy + gy2) / D) + skip  -- the adds autograd's engine would launch on its own.  skip needs
 * gv_out == NULL. */
int s2f_lif_bwd_ports(const float* gy, const float* gy2, const float* gv_out, const uint64_t* mask, const float* skip, float* gx,
                      int64_t n, float vth, int D, void* stream);

/* Leaky charge in front of the same firing rule -- LIFNode.neuronal_charge (neuron.py:803-814) under the fork's BaseNode.forward
 * (:166-197: multi-level quantised firing, soft reset, y = s / D).  No Spike2Former module instantiates LIFNode; the
 * entry points exist so that the neuron file's second node type has the same kernel-backed mirror (host: neuron.LIFNode).
 *     decay_input != 0:  h = v + (x - v) / tau        (reference expression order, true fp32 division)
 *     decay_input == 0:  h = v * (1 - 1/tau) + x      (factor formed in double, rounded to fp32 once, as Python's scalar multiply)
 * then as s2f_lif_fwd.  v_in? NULL == membrane freshly reset (0.): h = x / tau resp. x.  tau > 1 (neuron.py:792).
 * Backward: g_h = gv_out + (gy / D - gv_out * vth) * m;  decay_input: gx = g_h / tau, gv_in = g_h - g_h / tau;
 * otherwise gx = g_h, gv_in = g_h * (1 - 1/tau).  gv_out? NULL == 0; gv_in? NULL == not wanted. */
int s2f_lif_leaky_fwd(const float* x, const float* v_in, void* y, float* v_out, uint64_t* mask, uint64_t* stats, int64_t n, float vth,
                      int D, float tau, int decay_input, int y_bf16, void* stream);
int s2f_lif_leaky_bwd(const float* gy, const float* gv_out, const uint64_t* mask, float* gx, float* gv_in, int64_t n, float vth, int D,
                      float tau, int decay_input, void* stream);

/* The decoder's value / key neurons on  a = x + e[c]  and  a + pos[b, c, l]  in one pass (x [TB, C, L] with tb = t*B + b,
 * e [C] = level_embed row, pos [B, C, L] = key positional encoding; mmdet/models/dense_heads/maskformer_head.py:535-540,
 * mmcv_spike/transformer.py:626-629): y_value = Q_IFNode(a), y_key = Q_IFNode(a + pos), reset stateless neurons, 1-bit
 * in-range masks as s2f_lif_fwd.  Backward: gx = STE(g_key, mask_key) + STE(g_value, mask_value); the gradient of e is the
 * per-channel sum of gx (left to the caller).  L % 4 == 0. */
int s2f_sum2_lif_fwd(const float* x, const float* e, const float* pos, void* y_key, void* y_value, uint64_t* mask_key,
                     uint64_t* mask_value, int64_t TB, int64_t B, int64_t C, int64_t L, float vth, int D, int y_bf16,
                     void* stream);
int s2f_sum2_lif_bwd(const float* g_key, const float* g_value, const uint64_t* mask_key, const uint64_t* mask_value,
                     float* gx, int64_t n, int D, void* stream);
/* The same with either incoming gradient optional (NULL = zero) and, in gx_key?, STE(g_key, mask_key) alone: summed over the T
 * time steps it is the gradient with respect to `pos` (the decoder's self- / cross-attention query neurons, whose position term is
 * the learnable query embedding: mmcv_spike/transformer.py:597-638). */
int s2f_sum2_lif_bwd_ex(const float* g_key, const float* g_value, const uint64_t* mask_key, const uint64_t* mask_value, float* gx,
                        float* gx_key, int64_t n, int D, void* stream);
/* ... and with a second consumer's gradient per spike map and a residual branch's gradient on x folded in (s2f_lif_bwd_ports):
 * the key / value spikes of one memory level are read by two decoder layers (maskformer_head.py:554-564), the decoder's
 * query + attention(query) reads the query beside its neurons (detr_layers.py:523-537). */
int s2f_sum2_lif_bwd_ports(const float* g_key, const float* g_key2, const float* g_value, const float* g_value2,
                           const uint64_t* mask_key, const uint64_t* mask_value, const float* skip, float* gx, float* gx_key, int64_t n,
                           int D, void* stream);

/* Layer scale folded into a BatchNorm's affine pair: w[c] = gamma[c] * s[c], b[c] = beta[c] * s[c]  (the pixel decoder's
 * `q + gamma_i * f(q)`, detr_layers.py:331-337, with f ending in a BatchNorm: u = s * BN(z) = BN_{gamma s, beta s}(z)).
 * Backward: dgamma = gw * s, dbeta = gb * s, ds = gw * gamma + gb * beta.  One launch each instead of 2 + 5 vector ops. */
int s2f_scale_affine_fwd(const float* gamma, const float* beta, const float* s, float* w, float* b, int C, void* stream);
int s2f_scale_affine_bwd(const float* gw, const float* gb, const float* gamma, const float* beta, const float* s,
                         float* dgamma, float* dbeta, float* ds, int C, void* stream);

/* ---- T successive stateful calls on one neuron, membrane carried in registers -----------------------
 * Same arithmetic as T calls of s2f_lif_fwd with v chained (what tools/cal_firing_num.py:203-225 does across
 * images; structural precedent: the dormant cupy kernel IFNode_fptt_softReset, neuron_kernel.py:19-119).
 * x_seq, y_seq: [T, n]; mask: [T, s2f_lif_mask_words(n)]; v0? / vT? : [n]. stats?: uint64[T][S2F_STAT_SLOTS][2]. */
int s2f_lif_seq_fwd(const float* x_seq, const float* v0, float* y_seq, float* vT, uint64_t* mask, uint64_t* stats,
                    int T, int64_t n, float vth, int D, void* stream);
/* BPTT: g_h[t] = g_h[t+1] + (gy[t]/D - g_h[t+1]*vth) * m[t], g_h[T] := gvT (NULL == 0); gx_seq[t] = g_h[t]; gv0? = g_h[0]. */
int s2f_lif_seq_bwd(const float* gy_seq, const float* gvT, const uint64_t* mask, float* gx_seq, float* gv0, int T,
                    int64_t n, float vth, int D, void* stream);

/* ---- BatchNorm fused with the conv bias, the residual add and the following Q_IFNode -------------------
 * Replaces the reference's chain  t = conv(x) + b ; u = BatchNorm(t) [+ residual] ; y = Q_IFNode(u)  (e.g. MS_ConvBlock,
 * SepConv, MS_MLP: mmseg/models/backbones/sdtv2.py:167-255; every Sequential(conv, BN) + Q_IFNode of the head), which
 * runs as ~12 ATen elementwise kernels forward and as many backward.  z: [N, C, L] channel-major, any L >= 1 (rows of
 * L % 4 != 0 elements take element-wise kernels: odd shapes only, e.g. a 10-query decoder; no map of the path at its real sizes).
 *
 * s2f_bn_stats (training only): per-channel sum / sum of squares of (z + conv_bias?) accumulated into sums_zeroed
 *   (double[2C], MUST be zero on entry -- the host hands out slices of one arena cleared once per step).
 * s2f_bn_act_fwd:  mean / rstd = 1/sqrt(var + eps) from `sums` (training) or from the running statistics (eval), written to
 *   stat_out[0:C] / stat_out[C:2C] (stat_out: float[3C]); training: running_mean?/running_var? updated in place with
 *   `momentum` and the unbiased variance, *num_batches_tracked? += 1 (torch.nn.BatchNorm semantics).
 *   stat_out[2C:3C] = beta - running_mean * gamma / sqrt(running_var + eps) with the UPDATED running statistics: the
 *   border value "BN(0)" of BNAndPadLayer (sdtv2.py:68-78), which s2f_dwconv_fwd takes as `border`.
 *   u = ((z + b) - mean) * rstd * gamma + beta [+ residual?] ; u_out? = u ;
 *   if y != NULL:  the Q_IFNode update of s2f_lif_fwd on u (v_in?, v_out?, mask?, stats? as there).
 * s2f_bn_act_bwd:  gu = g_u? + STE(g_y?, g_v?, mask) ;  training: gz = gamma*rstd*(gu - mean(gu) - xhat*mean(gu*xhat)),
 *   eval: gz = gamma*rstd*gu ;  g_residual? = gu ;  dgamma = sum(gu*xhat) ; dbeta = sum(gu).  sums_zeroed as above. */
/* 1 when, in training mode, s2f_bn_act_fwd / s2f_bn_act_bwd compute the channel statistics of this shape themselves
 * (one workgroup per channel holds the channel's N*L elements in registers: small maps with L % 256 == 0; one to sixteen wavefronts
 * per channel for rows that are not whole tiles, see s2f_bn_mask_words): the caller then skips s2f_bn_stats and may pass sums / sums_zeroed = NULL. */
int s2f_bn_single_pass(int64_t N, int64_t C, int64_t L);
/* uint64 words of the in-range mask that s2f_bn_act_fwd writes and s2f_bn_act_bwd reads for this shape in training mode: the flat
 * 256-element-tile layout of s2f_lif_mask_words, except for rows that are not whole tiles (L % 4 == 0, L % 256 != 0, C >= 32) with
 * N * L <= 20 480 -- the decoder's 100-token maps (N * L <= 2 048: one wavefront per channel, 32 words per channel) and C5's 50 x 84
 * maps (up to sixteen wavefronts per channel, 320 words per channel) -- whose single-pass kernels keep a per-channel mask layout of
 * their own (private to this forward / backward pair). */
int64_t s2f_bn_mask_words(int64_t N, int64_t C, int64_t L);
int s2f_bn_stats(const float* z, const float* conv_bias, double* sums_zeroed, int64_t N, int64_t C, int64_t L,
                 void* stream);
int s2f_bn_act_fwd(const float* z, const float* conv_bias, const double* sums, float* stat_out, float* running_mean,
                   float* running_var, int64_t* num_batches_tracked, const float* gamma, const float* beta,
                   const float* residual, float* u_out, const float* v_in, void* y, float* v_out, uint64_t* mask,
                   uint64_t* stats, int64_t N, int64_t C, int64_t L, float momentum, float eps, int training, float vth,
                   int D, int y_bf16, void* stream);
int s2f_bn_act_bwd(const float* z, const float* conv_bias, const float* stat, const float* gamma, const float* g_u,
                   const float* g_y, const float* g_v, const uint64_t* mask, double* sums_zeroed, float* gz,
                   float* g_residual, float* dgamma, float* dbeta, int64_t N, int64_t C, int64_t L, int training,
                   float vth, int D, void* stream);
/* s2f_bn_act_fwd on [N, C, H * W] whose residual is the exact-2x bilinear up-sampling (s2f_upsample2x_fwd) of residual_lo
 * [N * C, H/2, W/2] -- the top-down add of an FPN level: the apply kernel forms the up-sampled values from the low-resolution map
 * itself (same expressions, same order, no contraction: u, spikes, mask, counters and statistics are bit-identical to the two
 * launches) and the [N, C, H, W] fp32 map is neither written nor read.  Training mode with `sums` given, on the row-walking
 * kernels: s2f_bn_up_ok(N, C, H, W, training, D) = 1 <=> H * W % 256 == 0, W % 4 == 0, 256 % W == 0 or W % 256 == 0, H even, D a
 * power of two, not a single-pass shape; residual_lo 8-byte aligned.  Everything else: the two launches.  The backward is
 * s2f_bn_act_bwd with g_residual, then s2f_upsample2x_bwd_add. */
int s2f_bn_up_ok(int64_t N, int64_t C, int64_t H, int64_t W, int training, int D);
int s2f_bn_act_up_fwd(const float* z, const float* conv_bias, const double* sums, float* stat_out, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, const float* gamma, const float* beta,
                      const float* residual_lo, float* u_out, const float* v_in, void* y, float* v_out, uint64_t* mask,
                      uint64_t* stats, int64_t N, int64_t C, int64_t H, int64_t W, float momentum, float eps, int training,
                      float vth, int D, int y_bf16, void* stream);

/* Train-mode BatchNorm o BatchNorm as ONE kernel (every RepConv chain of the attention blocks ends in two: Sequential(RepConv(..,
 * BN), BN), mmseg/models/backbones/sdtv2.py:112-132, 280-296, 304-306).  With xhat = (z + b - mean) r the first BatchNorm gives
 * a = gamma xhat + beta, whose batch mean is beta and whose biased batch variance is gamma^2 var r^2: the second needs no pass of
 * its own,  BN2(BN1(z)) = gamma gamma2 r2 xhat + beta2,  r2 = 1 / sqrt(gamma^2 var r^2 + eps2);  running_mean2 / running_var2 are
 * updated with (beta, gamma^2 var r^2 n/(n-1)).  Single-pass shapes only (s2f_bn2_fused_ok; the 32x32-stage maps where these
 * chains live); stat_out: float[4C] = mean, r, BN1(0) border, r2.  The backward returns both BatchNorms' parameter gradients:
 * dbeta2 = sum gu, dgamma2 = gamma r2 sum(gu xhat), dbeta = 0, dgamma = gamma2 eps2 r2^3 sum(gu xhat). */
int s2f_bn2_fused_ok(int64_t N, int64_t C, int64_t L);
int s2f_bn2_act_fwd(const float* z, const float* conv_bias, float* stat_out, float* running_mean, float* running_var,
                    int64_t* num_batches_tracked, const float* gamma, const float* beta, float momentum, float eps,
                    const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                    int64_t* num_batches_tracked2, float momentum2, float eps2, const float* residual, float* u_out,
                    const float* v_in, void* y, float* v_out, uint64_t* mask, uint64_t* stats, int64_t N, int64_t C, int64_t L,
                    float vth, int D, int y_bf16, void* stream);
int s2f_bn2_act_bwd(const float* z, const float* conv_bias, const float* stat, const float* gamma, const float* gamma2, float eps2,
                    const float* g_u, const float* g_y, const float* g_v, const uint64_t* mask, float* gz, float* g_residual,
                    float* dgamma, float* dbeta, float* dgamma2, float* dbeta2, int64_t N, int64_t C, int64_t L, float vth, int D,
                    void* stream);

/* ---- im2col / col2im of the dense k x k convolutions that do not take the implicit 3x3 kernels: the stride-2 down-samplings and
 * the 7x7 stem (MS_DownSampling, mmseg/models/backbones/sdtv2.py:386-421).  cols [N][C kh kw][Ho Wo] (same dtype as x: fp32, or
 * bf16 spikes with x_bf16), row (c kh + ky) kw + kx, zero outside the plane, dilation 1 -- torch.nn.functional.unfold's layout.
 * s2f_col2im is its adjoint as a gather (no atomics, no zero fill): gx[n][c][y][x] = sum of the column entries that cover it. */
int s2f_im2col(const void* x, void* cols, int N, int C, int H, int W, int kh, int kw, int stride, int pad, int x_bf16, void* stream);
int s2f_col2im(const float* cols, float* gx, int N, int C, int H, int W, int kh, int kw, int stride, int pad, void* stream);

/* ---- depthwise KxK convolution (stride 1, dilation 1, K in {3,5,7}) on [N, C, H, W] -----------------------
 * Replaces nn.Conv2d(groups=C) as used by SepConv.dwconv (mmseg/models/backbones/sdtv2.py:156-163), RepConv's un-padded
 * 3x3 on the BNAndPadLayer output (sdtv2.py:48-89, 123-127), SepConv_Spike.dwconv (mmcv_spike/SNN_core.py:36-40),
 * DCNv3_pytorch.dw_conv (ops_dcnv3/modules/dcnv3.py:161-169) and the pixel decoder's output_convs (pixel_decoder.py:374-378).
 * w: [C, K, K].  Output size Ho = H + 2*pad - K + 1.  border?: per-channel value read inside the padding ring instead of
 * zero (BNAndPadLayer's constant border, sdtv2.py:68-84) -- the padded tensor is never materialised.
 * x_bf16 != 0: x is a bf16 spike map (uint16 storage) as the neuron kernels write it (SepConv.dwconv, the pixel decoder's
 * output convolutions and DCNv3's dw_conv all read a neuron output); the arithmetic stays fp32. */
int s2f_dwconv_fwd(const void* x, const float* w, const float* border, float* y, int N, int C, int H, int W, int K,
                   int pad, int x_bf16, void* stream);
/* s2f_dwconv_fwd for K = 3, pad = 1, no border (the same y, bit for bit) that also stores the BatchNorm partials of y for the
 * train-mode BatchNorm behind it: every workgroup reduces the outputs it stored to one fp32 (sum, sum of squares) pair -- wave
 * shuffles and one LDS round in a fixed order, no atomics -- at partials[(c * P + n * tiles + tile) * 2 + {0, 1}],
 * P = s2f_dwconv_stats_slots(N, H, W) = N * workgroups per plane (64 x 32 tiles for W % 4 == 0, W >= 128, H >= 32, else 32 x 32).
 * s2f_bn_partials_finalize(partials, P, ...) turns them into the sums of s2f_bn_stats.  x aligned to four elements. */
int64_t s2f_dwconv_stats_slots(int N, int H, int W);
int s2f_dwconv_fwd_stats(const void* x, const float* w, float* y, float* partials, int64_t P, int N, int C, int H, int W,
                         int x_bf16, void* stream);
/* Eval mode (row f4): the stencil with the BatchNorm (running statistics) and the Q_IFNode that follow every depthwise convolution of
 * the path in its store -- u_out? = fp32 pre-activation, y_bf16? = bf16 spikes, stats? = firing counters; the fp32 convolution
 * output is never written.  Per-element expressions of s2f_bn_act_fwd in eval mode (bit-identical spikes). */
int s2f_dwconv_bn_lif_fwd(const void* x, const float* w, const float* border, const float* running_mean, const float* running_var,
                          const float* gamma, const float* beta, float eps, float* u_out, void* y_bf16, uint64_t* stats, int N,
                          int C, int H, int W, int K, int pad, int x_bf16, float vth, int D, void* stream);
int s2f_dwconv_bwd_input(const float* gy, const float* w, float* gx, int N, int C, int H, int W, int K, int pad,
                         void* stream);
int s2f_dwconv_bwd_weight(const void* x, const float* border, const float* gy, float* gw, int N, int C, int H, int W,
                          int K, int pad, int accumulate, int x_bf16, void* stream);

/* ---- spike GEMM on the bf16 matrix cores ---------------------------------------------------------------
 * Y[b] (M x N) = W (M x K) @ X[b] (K x N) [+ bias[M]]   for b in [0, batch): the 1x1 Conv2d / Conv1d(k=1) / im2col'd kxk
 * convolution of the path on channel-major activations [batch, K, N] whose input is a Q_IFNode output (q/k/v/proj RepConv
 * 1x1, sdtv2.py:121-125, 304-306; MS_MLP / MS_ConvBlock / MS_DownSampling, sdtv2.py:197-204, 229-235, 399-405; the head's
 * Conv1d / 1x1 Conv2d, mmcv_spike/transformer.py:213-236, 758-763, pixel_decoder.py:368-404, SNN_core.py:31-45).
 * X must hold spikes -- multiples of 1/D with at most 8 significant bits (exact in bf16).  W is pre-split by
 * s2f_split_bf16x3 into hi + mid + lo bf16 terms (24 mantissa bits); products are exact, accumulation is fp32:
 * the accuracy of an fp32 GEMM on v_mfma_f32_32x32x16_bf16.  `terms` in {1,2,3} = number of weight terms used.
 * w_split: [3][Mpad][Kpad] bf16, zero padded, Mpad % 64 == 0, Kpad % 32 == 0.  N % 4 == 0. */
int s2f_split_bf16x3(const float* w, uint16_t* w_split, int M, int K, int Mpad, int Kpad, void* stream);
/* All weights of a model in ONE launch -- the re-split a training step owes after the optimiser has updated them, and the
 * node a captured step replays so that every replay multiplies by the LIVE fp32 weights.  jobs (device): int64 [njobs][8] =
 * {src fp32 pointer, dst bf16 pointer, M, K, Mpad, Kpad, mode | (C << 8), first workgroup}; job i owns workgroups
 * [first_i, first_i + ceil(Mpad Kpad / 1024)), total_workgroups = their sum.  mode 0: src = the [M][K] matrix; 1: src = a
 * conv weight [M][C][3][3] read tap-major (the w_split layout of s2f_spike_conv3x3_fwd); 2: the flipped, transposed
 * matrix of a conv weight [C][M][3][3] that s2f_conv3x3_general takes for the input gradient (C field = its out-channels). */
int s2f_split_bf16x3_multi(const int64_t* jobs, int njobs, int64_t total_workgroups, void* stream);
int s2f_spike_gemm_fwd(const uint16_t* w_split, const float* X, const float* bias, float* Y, int batch, int M, int N,
                       int K, int Mpad, int Kpad, int terms, void* stream);
/* 3x3 convolution (stride 1, padding 1) of a SPIKE activation as an implicit GEMM on the same kernels: the B operand is
 * the activation X [batch, C, H, W] itself, the kernels' loaders form the rows of the im2col matrix on the fly -- the 9x
 * inflated column matrix of F.unfold is never materialised (MS_ConvBlock.conv1 / conv2,
 * mmseg/models/backbones/sdtv2.py:197-204).  The contraction runs TAP-MAJOR, k = (3 ky + kx) C + c (C % 32 == 0: a 32-wide
 * step lies in one tap): w_split = s2f_split_bf16x3 of weight.permute(0,2,3,1) viewed [M, 9C].  Y: [batch, M, H*W].
 * s2f_spike_conv3x3_fwd needs W % 4 == 0; s2f_spike_conv3x3_dw needs W % 4 == 0 (round 5: any such width; a power of two decodes the pixel index with a shift) and writes dW in the same tap-major
 * order, [M, 3, 3, C] (dY [batch, M, H*W]); the caller permutes it back to the weight's [M, C, 3, 3]. */
int s2f_spike_conv3x3_fwd(const uint16_t* w_split, const float* X, const float* bias, float* Y, int batch, int M, int C,
                          int H, int W, int Mpad, int Kpad, int terms, void* stream);
int s2f_spike_conv3x3_dw(const float* dY, const float* X, float* dW, int batch, int M, int C, int H, int W, int accumulate,
                         void* stream);
/* 3x3 convolution (stride 1, padding 1) of a GENERAL fp32 tensor, implicit GEMM with both operands split hi+mid+lo
 * (6 passes): Y[b] (M x H*W) = Wt (M x 9C, tap-major as above, Mpad % 128 == 0) (*) X[b] ([C, H, W]).  Used for the input
 * gradient of the 3x3 convolutions as the transposed convolution dX = flip(W)^T (*) dY -- no unfold(dY), no col2im. */
int s2f_conv3x3_general(const uint16_t* w_split, const float* X, float* Y, int batch, int M, int C, int H, int W, int Mpad,
                        int Kpad, void* stream);
/* General split GEMM on the same kernel structure:  Y[b] (M x N) = out_scale * A[b] (M x K) @ X[b] (K x N).
 *   a_split: bf16 terms as written by s2f_split_bf16x3: term i of batch b starts at a_split + i*a_term_stride +
 *     b*a_batch_stride (ELEMENTS; rows Kpad apart, Mpad readable rows per batch; a_batch_stride = 0 shares one A; several
 *     batches may be row blocks of ONE split matrix); a_terms in {1, 3} = terms used (1: A exact in bf16, e.g. spikes).
 *   X: fp32; row k of batch b lies at X + b*x_batch_stride + (k / k_inner)*x_outer_stride + (k % k_inner)*N (floats): a
 *     contraction over the T slabs of a [T, B, C, HW] tensor is ONE launch with K = T*C, k_inner = C, x_outer_stride =
 *     B*C*HW.  x_terms in {1, 3}: X is split in the kernel into that many bf16 terms.
 *   (a_terms, x_terms) = (1,3) or (3,1): 3 MFMA passes, exact products; (3,3): 6 passes (terms i + j <= 2), 2^-24.
 *   Mpad % 128 == 0, Kpad % 32 == 0, N % 4 == 0.  Call sites: the mask einsum 'ltbqc,tbchw->ltbqhw' + mean over t
 *   (mmdet/models/dense_heads/maskformer_head.py:582-583) forward and its d(mask_features). */
int s2f_split_gemm(const uint16_t* a_split, int64_t a_batch_stride, int64_t a_term_stride, int a_terms, const float* X,
                   int64_t x_batch_stride,
                   int k_inner, int64_t x_outer_stride, int x_terms, float* Y, int64_t y_batch_stride, float out_scale,
                   int batch, int M, int N, int K, int Mpad, int Kpad, void* stream);
/* Weight gradient of the same convolution:  dW[m][k] = sum_b sum_l dY[b][m][l] * X[b][k][l]   (dY [batch, M, L],
 * X [batch, K, L] spikes, dW [M, K] overwritten).  X is exact in bf16; dY is split on the fly into hi + mid + lo bf16
 * terms: three MFMA passes, exact products, fp32 accumulation (split-K partial tiles are combined with fp32 atomics, so
 * the result is reproducible to fp32 round-off, not bit for bit).  L % 4 == 0.
 * accumulate != 0: dW += ... (no clearing memset; for gradients summed straight into a pre-zeroed flat buffer).
 * x_terms: 1 = X exact in bf16 (spikes), 3 passes; 3 = X a general fp32 tensor, split like dY: 6 passes (terms i + j <= 2)
 *   -- the "both operands contraction-contiguous" GEMM of two general tensors, e.g. dE = g @ MF^T of the mask einsum. */
int s2f_spike_gemm_dw(const float* dY, const float* X, float* dW, int batch, int M, int K, int L, int accumulate, int x_terms,
                      void* stream);

/* ---- the same GEMMs with the activation operand ARRIVING in bf16 ------------------------------------------------------
 * The neuron kernels can write their spikes as bf16 (`y_bf16` of s2f_lif_fwd / s2f_bn_act_fwd / s2f_sum2_lif_fwd): spikes are
 * multiples of 1/D with at most 8 significant bits, so bf16 holds them exactly, at half the bytes of the reference's fp32
 * tensors.  X: bf16 [batch, K, N] (uint16_t storage), channel-major as above.  The K loops then hold loads, LDS traffic and
 * MFMAs only: the forward kernel copies the X tile as it lies in memory and forms the k-contiguous MFMA fragments with the
 * LDS transpose read (ds_read_b64_tr_b16); the weight-gradient kernel reads the contraction-contiguous rows directly.
 * Same arithmetic, same results as the fp32-operand entry points above.  N % 4 == 0 (16-byte chunks when N % 8 == 0).
 * s2f_to_bf16_exact: fp32 -> bf16 for a tensor that is exactly representable (spikes a caller still holds in fp32); n % 4 == 0. */
int s2f_to_bf16_exact(const float* x, uint16_t* y, int64_t n, void* stream);
int s2f_spike_gemm_fwd_bf16(const uint16_t* w_split, const uint16_t* X, const float* bias, float* Y, int batch, int M, int N,
                            int K, int Mpad, int Kpad, int terms, void* stream);
int s2f_spike_conv3x3_fwd_bf16(const uint16_t* w_split, const uint16_t* X, const float* bias, float* Y, int batch, int M,
                               int C, int H, int W, int Mpad, int Kpad, int terms, void* stream);
/* General form of the forward kernel: Y[b] (M x N) = out_scale * (A[b] (M x K) @ X[b] (K x N) + bias[b][m]) with a weight per
 * batch element (a_split + b * a_batch_stride: three bf16 terms [3][Mpad][Kpad] per batch, Mpad * Kpad * 3 apart at least),
 * and the contraction running over K / k_inner slabs of a bf16 spike map that lie x_outer_stride elements apart (row k of
 * batch b at X + b * x_batch_stride + (k / k_inner) * x_outer_stride + (k % k_inner) * N; k_inner % 32 == 0).  Call site:
 * the mask contraction of the head with the mask_feature 1x1 convolution folded into it (ops.mask_einsum_folded):
 * sum_t (E_t W_mf) @ S_t over the T time slices of mask_feature_spike's output as ONE contraction of length T*C
 * (mmdet/models/dense_heads/maskformer_head.py:582-583 + mmdet/models/layers/pixel_decoder.py:467-470). */
int s2f_spike_gemm_fwd_bf16_ex(const uint16_t* a_split, int64_t a_batch_stride, const uint16_t* X, int64_t x_batch_stride,
                               int k_inner, int64_t x_outer_stride, const float* bias, int64_t bias_batch_stride,
                               float out_scale, float* Y, int batch, int M, int N, int K, int Mpad, int Kpad, void* stream);
/* The same general product on the LDS-DMA pipeline (csrc/pgemm.hip, round 5): a_pack holds one s2f_pack_bf16x3 pack of [M][K] per
 * batch element, a_batch_stride elements apart; N % 8 == 0. */
int s2f_pgemm_nn_bf16_ex(const uint16_t* a_pack, int64_t a_batch_stride, const uint16_t* X, int64_t x_batch_stride, int k_inner,
                         int64_t x_outer_stride, const float* bias, int64_t bias_batch_stride, float out_scale, float* Y, int batch,
                         int M, int N, int K, void* stream);
int s2f_spike_gemm_dw_bf16(const float* dY, const uint16_t* X, float* dW, int batch, int M, int K, int L, int accumulate,
                           void* stream);
/* Implicit 3x3 weight gradient (stride 1, padding 1).  accumulate: bit 0 = add into dW (otherwise dW is zeroed first); bit 1 = dW in
 * the WEIGHT's layout [M][C][3][3] instead of the tap-major [M][3][3][C] the kernel contracts in -- with both bits the gradient goes
 * straight into the parameter's slot of the flat gradient buffer (no zeroed staging tensor, no permuted add). */
int s2f_spike_conv3x3_dw_bf16(const float* dY, const uint16_t* X, float* dW, int batch, int M, int C, int H, int W,
                              int accumulate, void* stream);
/* MANY weight gradients in one launch.  jobs: HOST array of njobs (<= 56) records {dY, X, dW (device pointers), batch, M, K,
 * L} as int64; each is the product of s2f_spike_gemm_dw_bf16 with accumulate != 0 (dW += ...: the destinations are slices
 * of a pre-zeroed flat gradient buffer).  The short-contraction layers of the path (32x32 / 64x64 stages, the decoder's
 * 100-token layers: ~180 launches per step of 18-35 us each, every one split 32-64 ways to fill the chip) become one grid
 * over all (job, tile, split) triples with a launch-wide contraction length per workgroup; the job table travels in the
 * kernel arguments.  bkv = contraction elements per step: 64 (rows with L % 64 == 0 or L >= 512) or 32. */
int s2f_spike_gemm_dw_grouped(const int64_t* jobs, int njobs, int bkv, void* stream);
/* The same weight gradients on the LDS-DMA pipeline (csrc/dwp.hip, round 5): tile 128 (dY rows) x 256 (X rows), contraction step
 * 32, eight wavefronts in two halves that alternate a multiply segment with a staging segment (X by global_load_lds into a
 * three-slot ring, dY split hi + mid + lo through registers into two stages), one barrier per segment.  Needs L % 4 == 0,
 * L >= 32, M L < 2^30, K L < 2^31; with L % 32 != 0 the last step of a batch element is masked while dY is split and the copies
 * are range-checked against the whole tensors: batch M L < 2^30, batch K L < 2^31 (s2f_spike_gemm_dw_pipe_ok says whether a shape qualifies; the host falls back to
 * s2f_spike_gemm_dw_bf16 otherwise).  cfg: 0 = the two-halves schedule, 1 = every wavefront in the same phase (probe);
 * target_wgs <= 0: default split of the contraction.  Replaces the autograd weight gradient of the 1x1 convolutions fed by a
 * Q_IFNode (mmseg/models/backbones/sdtv2.py:222-255, 304-306; mmcv_spike/transformer.py:213-236, 758-763;
 * mmdet/models/layers/pixel_decoder.py:368-404; mmdet/models/dense_heads/maskformer_head.py:581-582 for the mask contraction's
 * embedding gradient). */
int s2f_spike_gemm_dw_pipe_ok(int batch, int M, int K, int L);
int s2f_spike_gemm_dw_pipe(const float* dY, const uint16_t* X, float* dW, int batch, int M, int K, int L, int accumulate, int cfg,
                           int target_wgs, void* stream);
int s2f_spike_gemm_dw_pipe_grouped(const int64_t* jobs, int njobs, int cfg, int target_wgs, void* stream);
/* The implicit 3x3 weight gradient (stride 1, padding 1; what s2f_spike_conv3x3_dw_bf16 computes: dW [M][3][3][C] tap-major) on the same
 * kernel, up to 16 convolutions per launch.  The shifted rows of a tap are 2-byte aligned, which an LDS-DMA cannot fetch: the kernel
 * reads the horizontal taps from Xs, a copy of the activation shifted by one element behind an 8-element front pad (s2f_shift1_bf16:
 * Xs holds n + 16 elements, Xs[8 + i] = X[i + 1] for i = -1 .. n - 2, zeros elsewhere; n % 8 == 0),
 * and zeroes in the fragments what the zero padding would have supplied.  jobs (HOST array): njobs x {dY, X, Xs, dW (pointers),
 * batch, M, C, H, W} as int64; every dW is accumulated into; cfg bit 0 = the probe schedule of s2f_spike_gemm_dw_pipe, bit 1 = dW in
 * the weight's layout [M][C][3][3] (as s2f_spike_conv3x3_dw_bf16's accumulate bit 1).  Needs C % 32 == 0, W % 8 == 0, W >= 32, H W % 32 == 0, B C H W 2 < 2^31
 * (s2f_spike_conv3x3_dw_pipe_ok).  Replaces the autograd weight gradient of MS_ConvBlock's dense 3x3 convolutions and of the stride-1
 * down-sampling (mmseg/models/backbones/sdtv2.py:183-219, 540-548). */
int s2f_spike_conv3x3_dw_pipe_ok(int batch, int M, int C, int H, int W);
int s2f_shift1_bf16(const uint16_t* X, uint16_t* Xs, int64_t n, void* stream);
int s2f_spike_conv3x3_dw_pipe(const int64_t* jobs, int njobs, int cfg, int target_wgs, void* stream);

/* ---- pipelined GEMMs fed by LDS-DMA (csrc/pgemm.hip, round 3) ------------------------------------------------------------
 * The same products as s2f_spike_gemm_fwd_bf16 and as the autograd input gradient of a 1x1 convolution
 * (mmseg/models/backbones/sdtv2.py:121-125, 164, 222-255, 304-306; mmcv_spike/transformer.py:196-361), with the operand tiles
 * copied global -> LDS asynchronously (global_load_lds_dwordx4), 2-3 LDS stages and one barrier per K step.
 * The weight operand is PRE-PACKED into the kernels' LDS image: blocks of [3 terms hi|mid|lo][64 rows][32 k] bf16, block
 * (mb, kb) at element ((mb * ceil(K/32) + kb) * 6144), the 16-byte chunk c of row r stored at chunk c ^ ((r >> 2) & 3), rows
 * and columns past M / K zero.  s2f_pack_elems(M, K) = bf16 elements of a pack.
 * s2f_pack_bf16x3_multi: every pack of a model in one launch (what a training step owes after the optimiser update; recorded
 *   in a captured step).  jobs (device): int64 [njobs][8] = {src fp32 pointer, dst bf16 pointer, M, K, mode | (C << 8), first
 *   workgroup, 0, 0}; job i owns workgroups [first_i, first_i + ceil(ceil(M/64) ceil(K/32) 2048 / 1024)).  mode 0: src is the
 *   [M][K] matrix; 1: a conv weight [M][C][3][3] read tap-major (k = tap C + c); 2: the flipped, transposed matrix of a conv
 *   weight [Mw][M][3][3] (C field = Mw): A[c][tap Mw + m] = src[(m M + c) 9 + 8 - tap]; 3: the transpose of a [K][M] matrix.
 * s2f_pack_bf16x3: one matrix (the job in the kernel arguments: usable inside a stream capture).
 * s2f_pgemm_nn_bf16:  Y[b] (M x N) = A (M x K, packed) @ X[b] (K x N bf16 spikes, n contiguous) [+ bias[m]];  N % 8 == 0;
 *   terms in {1,2,3}; cfg: 0 = pick a tile by the problem size, 1..5 = force one (probe switch).
 * s2f_pgemm_dx_f32:   DX[b] (Ki x N) = W^T (Ki x Mo) @ G[b] (Mo x N, fp32) [+ beta * DX[b]] with W (Mo x Ki) given as ITS
 *   forward pack (the same buffer the forward product reads); G is split hi + mid + lo in the kernel: 6 MFMA passes, 2^-24.
 *   N % 4 == 0; batch strides in elements (0 = dense).  With the pack of W^T (mode 3) the same kernel is the forward product
 *   Y = W @ X of a convolution whose input X is a general fp32 tensor.  Replaces the library fp32 GEMM (rocBLAS / hipBLASLt) of round 1-2. */
/* Eval-mode fusion (the reference's fold: Qtrick_architecture/clock_driven/functional.py:574-692):
 *   y = Q_IFNode( BatchNorm_running( W @ X + conv_bias ) [+ residual] )   as ONE launch -- the GEMM above with bn_apply's and
 * the neuron's arithmetic in its epilogue (same per-element expressions: bit-identical to s2f_pgemm_nn_bf16 + s2f_bn_act_fwd in
 * eval mode).  u_out? = the fp32 pre-activation, y_bf16? = the spikes (bf16), v_in? / v_out? = carried membrane, stats? = firing
 * counters as in s2f_lif_fwd.  N % 4 == 0, N >= 8; the tile follows the plain product's rule (round 4: the eight-wavefront
 * register-staged tiles too).  No backward (inference path). */
int s2f_gemm_bn_lif_fwd(const uint16_t* a_pack, const uint16_t* X, const float* conv_bias, const float* running_mean,
                        const float* running_var, const float* gamma, const float* beta, float eps, const float* residual,
                        float* u_out, const float* v_in, void* y_bf16, float* v_out, uint64_t* stats, int batch, int M, int N,
                        int K, float vth, int D, void* stream);
/* The same epilogue on the implicit 3x3 convolution (stride 1, padding 1; w_pack = the tap-major pack, s2f_pack_bf16x3 mode 1; X
 * [batch][C][H][W] bf16 spikes): eval-mode conv3x3 -> BatchNorm [+ residual] [-> Q_IFNode] as one launch (MS_ConvBlock's two
 * convolutions in inference, mmseg/models/backbones/sdtv2.py:183-219). */
int s2f_conv3x3_bn_lif_fwd(const uint16_t* w_pack, const uint16_t* X, const float* conv_bias, const float* running_mean,
                           const float* running_var, const float* gamma, const float* beta, float eps, const float* residual,
                           float* u_out, const float* v_in, void* y_bf16, float* v_out, uint64_t* stats, int batch, int M, int C,
                           int H, int W, float vth, int D, void* stream);
int64_t s2f_pack_elems(int M, int K);
int s2f_pack_bf16x3(const float* src, uint16_t* dst, int M, int K, int mode, int C, void* stream);
int s2f_pack_bf16x3_multi(const int64_t* jobs, int njobs, int64_t total_workgroups, void* stream);
int s2f_pgemm_nn_bf16(const uint16_t* a_pack, const uint16_t* X, const float* bias, float* Y, int batch, int M, int N, int K,
                      int terms, int cfg, void* stream);
int s2f_pgemm_dx_f32(const uint16_t* w_pack, const float* G, int64_t g_batch_stride, float* DX, int64_t dx_batch_stride,
                     int batch, int Mo, int Ki, int N, float beta, int cfg, void* stream);
/* Inference: 1x1 convolution of a DENSE fp32 input -> BatchNorm (running statistics) [+ residual] [-> Q_IFNode from a reset
 * membrane] as ONE launch, `groups` (1..4) independent weights on consecutive channel groups: SepConv.pwconv2 behind the depthwise
 * convolution (sdtv2.py:135-180), the second 1x1 of the RepConv chains with their composed BatchNorm pair (sdtv2.py:112-132,
 * 304-306; the fold helpers of clock_driven/functional.py:574-692), the stem's column matrix (sdtv2.py:386-421).
 * X [batch][groups K][N] fp32 (strides in elements), per-channel vectors [groups M], residual / u_out / y_bf16
 * [batch][groups M][N]; w_packs[g] = s2f_pack_bf16x3 (mode 3) of W_g [M][K].  Six bf16 passes (fp32 accuracy).  N % 4 == 0. */
int s2f_dense_gemm_bn_lif_fwd(const uint16_t* const* w_packs, int groups, const float* X, int64_t x_batch_stride, int64_t x_group_stride,
                              const float* conv_bias, const float* running_mean, const float* running_var, const float* gamma,
                              const float* beta, float eps, const float* residual, float* u_out, void* y_bf16, uint64_t* stats,
                              int batch, int K, int M, int N, float vth, int D, void* stream);
/* Up to four independent products of s2f_pgemm_dx_f32's plain-store form in ONE launch (blockIdx.z = group): w_packs is a HOST
 * array of `groups` device pointers (copied into the kernel arguments); group g reads G + g * g_group_stride and writes DX + g *
 * dx_group_stride (and bn_partials? + g * partials_group_stride: the _stats form).  The channel groups of a grouped 1x1
 * convolution -- the second 1x1 of the stacked q | k | v projection chain (sdtv2.py:304-306), forward and input gradient. */
int s2f_pgemm_dx_f32_grouped(const uint16_t* const* w_packs, int groups, const float* G, int64_t g_batch_stride,
                             int64_t g_group_stride, float* DX, int64_t dx_batch_stride, int64_t dx_group_stride, float* bn_partials,
                             int64_t partials_group_stride, int batch, int Mo, int Ki, int N, void* stream);
/* Up to four sibling products of s2f_pgemm_nn_bf16 (no bias, three weight terms) in ONE launch (blockIdx.z = group): a_packs and Xs
 * are HOST arrays of `groups` device pointers (copied into the kernel arguments) -- the packed weight [M][K] and the contiguous bf16
 * spike map [batch][K][N] of each group; two groups may read one map.  Y [groups][batch][M][N] at y_group_stride elements.  Each
 * group runs the tile s2f_pgemm_nn_bf16 picks for ONE such product: bit-identical to `groups` single calls.  Only the shapes that
 * take the register-staged activation rows there (s2f_pgemm_nn_grouped_ok = 1: every N % 8 != 0, and the short contractions);
 * anything else is S2F_EINVAL before any launch.  The q / k / v projections of the decoder's self-attention
 * (mmcv_spike/transformer.py:196-361). */
int s2f_pgemm_nn_grouped_ok(int batch, int M, int N, int K);
int s2f_pgemm_nn_bf16_grouped(const uint16_t* const* a_packs, const uint16_t* const* Xs, int groups, float* Y, int64_t y_group_stride,
                              int batch, int M, int N, int K, void* stream);
/* Implicit 3x3 convolution (stride 1, padding 1) on the same pipeline: Y[b] (M x H W) = A (M x 9 C, the TAP-MAJOR pack of the
 * weight: s2f_pack_bf16x3 mode 1) @ im2col(X[b]), the column matrix never formed.  _bf16: X [batch][C][H][W] bf16 spikes, 3 passes
 * (forward; replaces s2f_spike_conv3x3_fwd_bf16, bit-identical).  _f32: X fp32, split in the kernel, 6 passes -- the INPUT
 * gradient as the convolution of dY [batch][C = conv out_channels][H][W] with the flipped, transposed weight (pack mode 2, M =
 * conv in_channels; replaces s2f_conv3x3_general, bit-identical).  C % 32 == 0, W % 4 == 0.  cfg 0 = automatic tile. */
int s2f_pgemm_conv3x3_bf16(const uint16_t* w_pack, const uint16_t* X, const float* bias, float* Y, int batch, int M, int C, int H,
                           int W, int cfg, void* stream);
int s2f_pgemm_conv3x3_f32(const uint16_t* w_pack, const float* X, float* Y, int batch, int M, int C, int H, int W, int cfg,
                          void* stream);
/* BatchNorm statistics from the producing GEMM's epilogue, without atomics (round 4; reference chain conv -> BatchNorm ->
 * Q_IFNode: mmseg/models/backbones/sdtv2.py:222-255, 304-333).  The `_stats` forms of the three forward
 * products above (no bias, all three weight terms, automatic tile) additionally store, per output row and per workgroup tile
 * (128 columns of one batch element), the fp32 sum and sum of squares of the tile's values:
 *   bn_partials[(row * P + p) * 2 + {0, 1}],   p = b * ceil(N / 128) + column tile,   P = s2f_bn_partials_count(batch, N)
 * (channel-major: one channel's partials are contiguous; plain stores: no atomics, nothing to zero, deterministic).  A group of a
 * grouped product (s2f_pgemm_dx_f32_stats with batch strides) writes its rows into a wider table: pass bn_partials + 2 * first_row * P.
 * s2f_bn_partials_finalize adds the P partials of every channel in fp64 in a fixed order into sums_out (double[2C], need not be
 * zeroed) -- the sums s2f_bn_stats produces (of z + conv_bias?: the shift is applied to the sums), which s2f_bn_act_fwd then takes
 * as `sums`.  The statistics pass over z -- one read of the tensor per BatchNorm, 5-47 us at C2 -- becomes a 2.5-4 us launch over
 * P * C * 8 bytes, and the statistics no longer depend on the order of fp64 atomics. */
int64_t s2f_bn_partials_count(int batch, int N);
int s2f_pgemm_nn_bf16_stats(const uint16_t* a_pack, const uint16_t* X, float* Y, float* bn_partials, int batch, int M, int N, int K,
                            void* stream);
int s2f_pgemm_conv3x3_bf16_stats(const uint16_t* w_pack, const uint16_t* X, float* Y, float* bn_partials, int batch, int M, int C,
                                 int H, int W, void* stream);
int s2f_pgemm_dx_f32_stats(const uint16_t* w_pack, const float* G, int64_t g_batch_stride, float* DX, int64_t dx_batch_stride,
                           float* bn_partials, int batch, int Mo, int Ki, int N, void* stream);
int s2f_bn_partials_finalize(const float* partials, int64_t P, const float* conv_bias, double* sums_out, int64_t N, int64_t C,
                             int64_t L, void* stream);
/* Up to four sibling train-mode BatchNorms [-> Q_IFNode from rest] of one SHORT-ROW shape (s2f_bn_grouped_ok = 1: L % 4 == 0,
 * L % 256 != 0, 8 <= N L <= 2048, C >= 32 -- the one-wavefront-per-channel kernels of s2f_bn_act_fwd / _bwd) in ONE launch
 * (blockIdx.y = group).  z, u_out?, y_out?, g_u?, g_y?, gz [groups][N][C][L]; conv_bias?, running_mean?, running_var?, gamma,
 * beta, dgamma, dbeta [groups C]; stat [groups][3 C]; mask groups x s2f_bn_mask_words(N, C, L) words.  No residual, membrane,
 * firing counters or second gradient port; num_batches_tracked is the caller's to count.  Bit-identical to `groups` single calls
 * on the slices; any other shape is S2F_EINVAL. */
int s2f_bn_grouped_ok(int64_t N, int64_t C, int64_t L);
int s2f_bn_act_fwd_grouped(const float* z, const float* conv_bias, float* stat_out, float* running_mean, float* running_var,
                           const float* gamma, const float* beta, float* u_out, void* y_out, uint64_t* mask, int groups, int64_t N,
                           int64_t C, int64_t L, float momentum, float eps, float vth, int D, int y_bf16, void* stream);
int s2f_bn_act_bwd_grouped(const float* z, const float* conv_bias, const float* stat, const float* gamma, const float* g_u,
                           const float* g_y, const uint64_t* mask, float* gz, float* dgamma, float* dbeta, int groups, int64_t N,
                           int64_t C, int64_t L, float vth, int D, void* stream);
/* s2f_bn_act_bwd with a SECOND gradient of the spike map (g_y2?, NULL = absent): the neuron fused into this BatchNorm has two
 * readers (the backbone taps feed the next stage and the pixel decoder's lateral convolution, mask2former's pixel_decoder.py:316-472;
 * DCNv3's offset and mask convolutions share offset_spike, dcnv3.py:209-214), and g_y + g_y2 is formed where g_y is read instead of
 * by an add launch of the autograd engine.  Only on the kernels s2f_bn_bwd_ports_ok() names (1 = supported for this shape). */
int s2f_bn_bwd_ports_ok(int64_t N, int64_t C, int64_t L, int training, int D);
int s2f_bn_act_bwd_ports(const float* z, const float* conv_bias, const float* stat, const float* gamma, const float* g_u,
                         const float* g_y, const float* g_y2, const float* g_v, const uint64_t* mask, double* sums_zeroed, float* gz,
                         float* g_residual, float* dgamma, float* dbeta, int64_t N, int64_t C, int64_t L, int training, float vth,
                         int D, void* stream);

/* The gradient of a GEMM-produced pre-activation as THREE bf16 PLANES hi | mid | lo (gz = hi + mid + lo to 2^-24; plane p at
 * gz_split + p * N C L): s2f_bn_act_bwd_split is s2f_bn_act_bwd writing that form instead of fp32 (6 instead of 4 bytes per
 * element), s2f_pgemm_dx_split the input-gradient product reading it (plane p of batch b at G_split + p * plane_stride +
 * b * Mo * N): both operands of its K loop arrive by LDS-DMA, nothing is converted or stored to LDS by the wavefronts.
 * N % 8 == 0. */
int s2f_bn_act_bwd_split(const float* z, const float* conv_bias, const float* stat, const float* gamma, const float* g_u,
                         const float* g_y, const float* g_v, const uint64_t* mask, double* sums_zeroed, uint16_t* gz_split,
                         float* g_residual, float* dgamma, float* dbeta, int64_t N, int64_t C, int64_t L, int training,
                         float vth, int D, void* stream);
int s2f_pgemm_dx_split(const uint16_t* w_pack, const uint16_t* G_split, int64_t plane_stride, float* DX, int batch, int Mo,
                       int Ki, int N, int cfg, void* stream);
/* The weight gradients of the same layers from the planes: s2f_spike_gemm_dw_bf16 / s2f_spike_gemm_dw_grouped with dY given as
 * hi | mid | lo (plane_stride >= batch * M * L elements apart; in the grouped form every job's dY is such a triple, batch * M * L
 * apart): the tile is copied into LDS as it lies -- the loop converts nothing. */
int s2f_spike_gemm_dw_bf16_split(const uint16_t* dY_split, int64_t plane_stride, const uint16_t* X, float* dW, int batch, int M,
                                 int K, int L, int accumulate, void* stream);
int s2f_spike_gemm_dw_grouped_split(const int64_t* jobs, int njobs, int bkv, void* stream);
/* dW (+)= sum_b dY[b] (M x L) X[b]^T (L x K), both operands general fp32 (6 passes), batch strides in elements (0 = dense);
 * accumulate: bit 0 = add into dW (else it is zeroed first), bit 1 = no contraction split (one add per element: run-to-run identical):
 * the weight gradient of the 1x1 convolutions whose input is not a spike map. */
int s2f_gemm_dw_general(const float* dY, int64_t dy_batch_stride, const float* X, int64_t x_batch_stride, float* dW, int batch,
                        int M, int K, int L, int accumulate, void* stream);
/* Many of them in ONE launch (the counterpart of s2f_spike_gemm_dw_grouped for two general operands): jobs = HOST array of
 * njobs x {dY, dy_batch_stride, X, x_batch_stride, dW, batch, M, K, L} (int64 each; strides in elements, 0 = dense); every dW
 * is ACCUMULATED into.  1 <= njobs <= 56; the table travels in the kernel arguments (capturable). */
int s2f_gemm_dw_general_grouped(const int64_t* jobs, int njobs, void* stream);

/* ---- exact-2x bilinear up-sampling (align_corners = False) of [planes, h, w] -> [planes, 2h, 2w] and its adjoint ------
 * Replaces F.interpolate(y, size=2x, mode='bilinear', align_corners=False) in the pixel decoder's FPN path
 * (mmdet/models/layers/pixel_decoder.py:456-460).  w must be even (16-byte output stores). */
int s2f_upsample2x_fwd(const float* x, float* y, int64_t planes, int h, int w, void* stream);
/* y = sigmoid(up2x(x)) in one pass (w % 4 == 0, x and y 16-byte aligned): the inference post-processing's
 * F.interpolate(mask_pred, size = img_shape) followed by mask_pred.sigmoid() (mmseg/models/decode_heads/maskformer_head.py:170-176)
 * where the masks are predicted at half the image resolution (every Spike2Former config).  No adjoint: inference only. */
int s2f_upsample2x_sigmoid_fwd(const float* x, float* y, int64_t planes, int h, int w, void* stream);
int s2f_upsample2x_bwd(const float* gy, float* gx, int64_t planes, int h, int w, void* stream);
/* gx = adjoint(gy) + add  (add? [planes, h, w], NULL = absent): the pixel decoder's level map feeds the next level's up-sampling
 * AND the transformer decoder (pixel_decoder.py:437-449, 466-471); the gradient the second reader sends back is summed here instead
 * of by an add launch of the autograd engine. */
int s2f_upsample2x_bwd_add(const float* gy, const float* add, float* gx, int64_t planes, int h, int w, void* stream);

/* ---- general bilinear resizing and the inference post-processing (csrc/resize.hip) ----------------------------------------------
 * F.interpolate(x, size=(H, W), mode='bilinear', align_corners=...) of [planes, h, w] fp32 maps for any sizes (enlarging or
 * shrinking, 1-pixel maps included), with ATen's arithmetic for an explicit size; the predict path at image sizes that are not
 * multiples of 32 (the exact-2x even-width case stays on s2f_upsample2x_*).  Source window: plane p's logical pixel (r, c) is
 * x[p * plane_stride + (row0 + r) * row_stride + col0 + c] (the padding crop of postprocess_result, mmseg segmentors/base.py:
 * 160-175, without a copy), after the flips the flags ask for; y is a contiguous [planes, H, W].
 * flags: S2F_RESIZE_ALIGN_CORNERS | S2F_RESIZE_SIGMOID (y = sigmoid(resize), the head's predict) | S2F_RESIZE_FLIP_H / _V (the
 * window is flipped before resizing: a flipped test-time view undone). */
#define S2F_RESIZE_ALIGN_CORNERS 1
#define S2F_RESIZE_SIGMOID 2
#define S2F_RESIZE_FLIP_H 4
#define S2F_RESIZE_FLIP_V 8
int s2f_resize_fwd(const float* x, float* y, int64_t planes, int64_t plane_stride, int row_stride, int row0, int col0, int h, int w,
                   int H, int W, int flags, void* stream);
/* gx [planes, h, w] = adjoint of the (window-free, flip-free) resize applied to gy [planes, H, W], + add (add? NULL = absent: the
 * gradient of a second reader of the input, as s2f_upsample2x_bwd_add).  A gather with a fixed summation order: bit-repeatable.
 * flags: S2F_RESIZE_ALIGN_CORNERS only. */
int s2f_resize_bwd_add(const float* gy, const float* add, float* gx, int64_t planes, int h, int w, int H, int W, int flags,
                       void* stream);
/* Per pixel of x [K, HW]: K > 1 -> label = argmax over K (int64; torch.argmax: the first maximum, NaN wins);
 * K == 1 -> (sigmoid ? sigmoid(x) : x) > threshold, into label (int64) or label_f (float 0 / 1): exactly one of the two.
 * (EncoderDecoder.postprocess_result's arg-max / threshold, mmseg segmentors/base.py:190-198.) */
int s2f_seg_argmax(const float* x, int64_t* label, float* label_f, int K, int64_t HW, int sigmoid, float threshold, void* stream);
/* s2f_resize_fwd + s2f_seg_argmax in one launch, without the [K, H, W] planes between them (ABI 48): per pixel of the [H, W] output
 * the K classes of x's window (plane_stride .. w and the align / flip flags as s2f_resize_fwd) are interpolated with s2f_resize_fwd's
 * arithmetic and only the running best is kept.  K > 1 -> label = argmax over K (int64; the first maximum, NaN wins);
 * K == 1 -> sigmoid(value) > threshold into label (int64) or label_f (float 0 / 1): exactly one of the two.  The bits of the two-pass
 * route.  flags: S2F_RESIZE_ALIGN_CORNERS | S2F_RESIZE_FLIP_H / _V (S2F_RESIZE_SIGMOID is implied for K == 1 and not accepted). */
int s2f_seg_label(const float* x, int64_t* label, float* label_f, int K, int64_t plane_stride, int row_stride, int row0, int col0,
                  int h, int w, int H, int W, int flags, float threshold, void* stream);
/* Test-time augmentation (mmseg segmentors/seg_tta.py:14-48) for one image and one view: the view's logits x [K] x (window, flags as
 * s2f_resize_fwd) are resized to the accumulator's [H, W] and acc [K, H, W] (first ? = : +=) softmax over K (max-subtracted, expf,
 * divided by the sum); K == 1: sigmoid, after a first sigmoid if flags has S2F_RESIZE_SIGMOID (the reference's one-class merge
 * applies sigmoid to already-sigmoid seg_logits). */
int s2f_tta_accumulate(const float* x, float* acc, int K, int64_t plane_stride, int row_stride, int row0, int col0, int h, int w,
                       int H, int W, int flags, int first, void* stream);
/* acc [K, HW] /= n_views in place, then the arg-max / threshold of s2f_seg_argmax (no sigmoid) into label or label_f. */
int s2f_tta_finish(float* acc, int64_t* label, float* label_f, int K, int64_t HW, int n_views, float threshold, void* stream);

/* ---- sliding-window inference: cut the windows, merge their logits (csrc/slide.hip, ABI 46) ---------------------------------------
 * EncoderDecoder.slide_inference (mmseg/models/segmentors/encoder_decoder.py:246-296: per window a slice, an F.pad to the full map,
 * preds += , count_mat += 1, and a final preds / count_mat) as one gather launch per group of windows, with no padded temporary, no
 * zero-fill, no count map and no division pass.
 * The window grid is a function of (H, W, crop_h, crop_w, stride_h, stride_w) alone and both kernels compute it themselves:
 *     ny = max(H - crop_h + stride_h - 1, 0) / stride_h + 1            (nx alike from W, crop_w, stride_w)
 *     row i of the grid:   y2 = min(i * stride_h + crop_h, H),  y1 = max(y2 - crop_h, 0)            (columns alike)
 *     every window is eh = min(crop_h, H) by ew = min(crop_w, W); window index j = i * nx + jx, row-major: the reference's loop
 *     order.  The windows of the last row / column are shifted back inside the picture, so two windows may coincide: both count.
 * s2f_slide_windows: out [n, B, C, eh, ew] (contiguous, window-major) <- windows w0 .. w0 + n - 1 of x [B, C, H, W].  One launch;
 *     x and out need only their 4-byte element alignment (a window starts at any column).
 * s2f_slide_accumulate: merges logits [n, B, K, eh, ew], the logits of windows w0 .. w0 + n - 1, into preds [B, K, H, W].  For every
 *     pixel covered by at least one window of the group and every (b, k):
 *       acc = +0.0 if the group holds the FIRST of all windows that cover the pixel, else the stored preds value;
 *       acc += the group's covering windows, in increasing window index, each a separate fp32 addition;
 *       if the group holds the LAST window that covers the pixel: acc /= the number of ALL windows that cover it (IEEE fp32 division);
 *       preds = acc.
 *     Pixels outside the group's windows are not touched.  Submitted for all groups in INCREASING w0, this is bit for bit the
 *     reference's loop (which adds exact zeros where a window does not cover a pixel), for every grouping.  preds MAY START
 *     UNINITIALISED: no stale value is read.  A grid that leaves pixels uncovered (stride > crop on an axis where the picture is
 *     larger than the crop) leaves them unwritten: the caller checks coverage (the reference's assert) on the host.
 * Bounds (S2F_EINVAL before any launch): non-null pointers; B, C / K, H, W, crops, strides > 0; B * C (B * K) < 65536;
 *     0 <= w0, n > 0, w0 + n <= ny * nx; B * C * H * W < 2^62.  S2F_EALIGN: a pointer that is not 4-byte aligned.
 * Nothing is allocated and nothing synchronises: capturable in a hipGraph. */
int s2f_slide_windows(const float* x, float* out, int B, int C, int H, int W, int crop_h, int crop_w, int stride_h, int stride_w,
                      int w0, int n, void* stream);
int s2f_slide_accumulate(const float* logits, float* preds, int B, int K, int H, int W, int crop_h, int crop_w, int stride_h,
                         int stride_w, int w0, int n, void* stream);

/* ---- evaluation: the class histograms behind mIoU / mDice / mFscore (csrc/segmetric.hip, ABI 35) ---------------------------------
 * One image of IoUMetric.intersect_and_union (mmseg/evaluation/metrics/iou_metric.py:164-205: two boolean-mask gathers, three
 * torch.histc(bins = K, min = 0, max = K - 1) on float copies, three device -> host copies, float32 sums over the images) as ONE
 * launch that ADDS into totals, an int64 [3, K] device buffer the caller owns and zeroes: row 0 the intersection, row 1 the prediction
 * areas, row 2 the label areas (the union is row 1 + row 2 - row 0, formed on the host).  For pixel p of HW, with l the label:
 *   - the pixel takes part iff l != ignore_index;
 *   - totals[1][c] += 1 when pred == c, totals[2][c] += 1 when l == c, totals[0][c] += 1 when pred == l == c, each for 0 <= c < K
 *     only: a prediction or a label outside the classes counts nowhere (what histc does outside [min, max]) -- a pixel labelled 200 at
 *     K = 150 takes part and its prediction still counts in row 1.
 * Integer adds: independent of the arrival order, bit-repeatable, exact to 2^63 (the reference's float32 sums stop being exact at 2^24
 * pixels per class).  Nothing is allocated and nothing synchronises: capturable in a hipGraph.
 * pred: [HW] contiguous, S2F_SEG_PRED_I64 (what s2f_seg_argmax / s2f_tta_finish write for K > 1) or S2F_SEG_PRED_F32 (their one-class
 * 0 / 1 maps; a float counts in class c iff it equals c exactly, which is the reference's comparison after label.to(pred)).
 * label: S2F_SEG_LABEL_U8 (an annotation file as read) or S2F_SEG_LABEL_I64 (PackSegInputs); pixel p = (row p / W, column p % W) is
 * label[row * label_row_stride + column * label_pixel_stride] (ELEMENT strides; W, 1 = contiguous; 1, H = a label stored transposed,
 * the branch of iou_metric.py:187-190, read in place).
 * flags: S2F_SEG_REDUCE_ZERO_LABEL applies LoadAnnotations' reduce_zero_label mapping to the raw label first (0 -> 255, 255 -> 255,
 * every other value - 1), then the rules above: an un-shifted annotation scored directly.
 * Bounds: 0 < HW < 2^31 - 8 (32-bit workgroup counters), HW % W == 0, 0 < K <= S2F_SEG_HIST_MAX_CLASSES (three rows of K 32-bit
 * counters in LDS: 24 KiB at the bound). */
#define S2F_SEG_HIST_MAX_CLASSES 2048
#define S2F_SEG_PRED_I64 0
#define S2F_SEG_PRED_F32 1
#define S2F_SEG_LABEL_U8 0
#define S2F_SEG_LABEL_I64 1
#define S2F_SEG_REDUCE_ZERO_LABEL 1
int s2f_seg_hist(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                 int64_t label_pixel_stride, int W, int64_t HW, int K, int ignore_index, int flags, int64_t* totals, void* stream);
/* The class-pair table behind those histograms (ABI 40): ONE launch that ADDS one image into matrix, an int64 [K, K] device buffer the
 * caller owns and zeroes, row = label, column = prediction -- what the reference's tools/analysis_tools/confusion_matrix.py:46-65
 * takes on the host as bincount(n * gt + pred, minlength = n * n).  pred, pred_dtype, label, label_dtype, the strides, W, HW, K, the
 * bounds, the alignment rules and S2F_SEG_REDUCE_ZERO_LABEL are exactly those of s2f_seg_hist.  For pixel p, with l the label after
 * the reduce_zero_label mapping (applied to the raw label FIRST) and c the prediction:
 *   - the pixel counts iff l != ignore_index, 0 <= l < K, and c is a class: 0 <= c < K, for S2F_SEG_PRED_F32 also integral (NaN is
 *     never a class);
 *   - then matrix[l][c] += 1.  The accumulator is added to, never cleared.
 * The reference's function has no ignore_index: a 255 label takes its bincount out of the n * n range and its reshape fails.  The
 * rule here is the one IoUMetric / s2f_seg_hist apply, so diag(matrix) == totals[0] always, and the column sums == totals[1], the
 * row sums == totals[2] whenever every participating pixel has both a valid prediction and a valid label (the arg-max of a K-class
 * head always has).  Integer adds only: exact, independent of the arrival order.  Nothing is allocated and nothing synchronises:
 * capturable in a hipGraph.
 * Routes: a [K][K] table of 32-bit counters per workgroup in LDS while 4 K^2 bytes fit S2F_SEG_CONF_LDS_BYTES and what the device
 * reports for one workgroup (K <= 181; 90 000 B at K = 150, 116 964 B at K = 171: 128 KiB of the CU's 160 KiB hold the data sets'
 * 150 / 171 classes and leave the rest of the CU's LDS to whatever else is resident); otherwise, or with S2F_SEG_CONF_GLOBAL in
 * flags at any K, 64-bit global atomics straight into matrix.  Both give the same matrix.  Any other flag bit is S2F_EINVAL. */
#define S2F_SEG_CONF_LDS_BYTES 131072
#define S2F_SEG_CONF_GLOBAL 2
int s2f_seg_confusion(const void* pred, int pred_dtype, const void* label, int label_dtype, int64_t label_row_stride,
                      int64_t label_pixel_stride, int W, int64_t HW, int K, int ignore_index, int flags, int64_t* matrix, void* stream);

/* ---- visualisation: the panel SegLocalVisualizer draws (csrc/segdraw.hip, ABI 43) -------------------------------------------------
 * SegLocalVisualizer._draw_sem_seg and add_datasample's np.concatenate((gt, pred), axis=1) (mmseg/visualization/
 * local_visualizer.py:79-118, 218-219: np.unique, one full-image masked write per class present, a float64 blend, a truncation, on
 * the host) as ONE launch per image.
 * image: uint8 [H, W, 3].  gt: NULL, or a contiguous [H, W] map, S2F_SEG_LABEL_U8 or S2F_SEG_LABEL_I64.  pred: NULL, or a contiguous
 * [H, W] map, S2F_SEG_PRED_I64 or S2F_SEG_PRED_F32 (at least one of the two; the dtype code of a NULL map is ignored).  palette:
 * uint8 [K, 3] RGB in device memory.  out: uint8 [H, P W, 3] RGB, P the number of maps given: with both, the ground truth is the
 * left half of every row and the prediction the right half.
 * For map value l and source channel value v:  c = palette[l][ch] when 0 <= l < K, else 0;  the output byte is
 *     (uint8) trunc( fl64(v * (1 - alpha)) + fl64(c * alpha) )
 * with 1 - alpha formed once in double on the host -- exactly (image * (1 - alpha) + mask * alpha).astype(np.uint8).  The two
 * products and the sum are three separately rounded fp64 operations (a contracted evaluation differs at hundreds of (v, c) pairs).
 * A float pred paints class c iff it equals c exactly (-0.0 is class 0; NaN, +-inf and non-integers paint nothing), an int64 value
 * is compared as 64 bits (2^40 + 3 is not class 3).  Stated deviation: a NEGATIVE label paints nothing, where the reference would
 * index palette[-1]; no arg-max produces one.
 * flags: S2F_SEG_DRAW_BGR -- image is BGR (as mmcv decodes and TestAugment stages it) and is swapped on read; the palette and out
 * stay RGB.  S2F_SEG_REDUCE_ZERO_LABEL -- gt only: the raw annotation is mapped first (0 -> 255, 255 -> 255, else - 1), exactly as
 * in s2f_seg_hist.  Any other bit is S2F_EINVAL.
 * Bounds (S2F_EINVAL before any launch): H, W > 0, H W < 2^31 - 8, 0 < K <= S2F_SEG_HIST_MAX_CLASSES (the palette in LDS),
 * 0 <= alpha <= 1, gt or pred, non-null image, palette and out.  image, gt as uint8, palette and out may start at ANY byte (picture
 * b of a staged batch starts at byte 3 h0 w0 b, the right panel of a row at byte 3 W): the kernel moves whole aligned 32-bit words
 * and peels the bytes at the ends of its pieces; an int64 / fp32 map is aligned to its element (S2F_EALIGN).  Only the 3 H P W
 * bytes of out are written.  Nothing is allocated and nothing synchronises: capturable in a hipGraph. */
#define S2F_SEG_DRAW_BGR 4
int s2f_seg_draw(const uint8_t* image, const void* gt, int gt_dtype, const void* pred, int pred_dtype, const uint8_t* palette, int K,
                 double alpha, int flags, int H, int W, uint8_t* out, void* stream);

/* ---- training augmentation: the configs' train_pipeline + SegDataPreProcessor on the device (csrc/augment.hip, ABI 37) ------------
 * RandomResize(keep_ratio) -> RandomCrop(cat_max_ratio) -> RandomFlip -> PhotoMetricDistortion (mmseg datasets/transforms/
 * transforms.py:215-331, 575-737; the resize itself is mmcv's) and SegDataPreProcessor's training branch (channel swap,
 * (x - mean) / std, pad right / bottom to the crop size) as two launches, from the batch's raw pictures to the step's static inputs.
 * The random numbers are drawn by the caller and arrive in the table; the kernels are functions of their inputs, allocate nothing
 * and synchronise nothing: capturable in a hipGraph (a single chain).
 * data: `data_bytes` device bytes holding, per image and back to back with NO alignment, a uint8 HWC BGR picture [h0, w0, 3] and a
 * uint8 annotation [h0, w0].  params: B table entries in device memory (8-byte aligned):
 *   img_off, seg_off : byte offsets of the two into data          h0, w0 : source size          H, W : size after the resize
 *   crop_y/x[11]     : candidate crop origins in the resized picture, each in [0, max(H - Hc, 0)] x [0, max(W - Wc, 0)]
 *   flip             : horizontal flip of the cropped window
 *   bright_on/_beta, mode, contrast_on/_alpha, sat_on/_alpha, hue_on/_delta : PhotoMetricDistortion's draws
 * An entry that does not fit data (or has a non-positive size) yields an all-padding image and flags 0; origins outside their
 * range are clamped into it: no load leaves data whatever the table holds.
 *
 * s2f_aug_crop_stats: flags [B, 11] int32 <- RandomCrop.crop_bbox's test of every candidate window (rows crop_y .. + min(Hc, H),
 * columns crop_x .. + min(Wc, W)) of the NEAREST-resized annotation, source pixel ((y h0) / H, (x w0) / W) in exact integer
 * arithmetic: over the labels != ignore_index at least two are present and max / sum < cat_max_ratio (an fp64 quotient of the
 * integer counts, as numpy forms it).  reduce_zero_label maps each sample first (0 -> 255, 255 -> 255, l -> l - 1).
 *
 * s2f_aug_apply: writes EVERY element of inputs [B, 3, Hc, Wc] fp32 and seg [B, Hc, Wc] uint8 once (the outputs are never read).
 * The candidate is the first of 0 .. 9 whose flag is set, else 10 (flags? NULL: candidate 0 -- cat_max_ratio >= 1 needs no first
 * launch).  Output pixel (y, x) with y < hv = min(Hc, H), x < wv = min(Wc, W): resized pixel (crop_y + y, crop_x + (flip ? wv - 1 - x
 * : x)); bilinear sample of the picture with half-pixel centres and no antialias (the arithmetic of s2f_resize_fwd, scale = in /
 * out), rounded to nearest into uint8; PhotoMetricDistortion in the reference's order with its quantisation after every stage
 * (convert = fp32(v) * alpha + beta, clipped to 0 .. 255, TRUNCATED; brightness, contrast here if mode == 1, saturation, hue, contrast
 * here otherwise; saturation and hue each one BGR -> HSV -> BGR round trip on uint8 values); channel c of the output is channel
 * (bgr_to_rgb ? 2 - c : c) of that, (v - mean_c) / std_c with an IEEE divide (mean 0, std 1: none).  The map takes the nearest sample
 * with the label reduction.  Elsewhere: pad_val / seg_pad_val.
 * The 8-bit HSV used here (the reference calls OpenCV): V = max, S = 255 (V - min) / V, hue by 60-degree sectors (V == R, then G, then
 * B) halved into 0 .. 179 with 180 -> 0, each rounded to nearest; inverse: h / 30 -> sector i and fraction f, p = V (1 - s), q = V (1 -
 * s f), t = V (1 - s (1 - f)) with s = S / 255, rounded to nearest.  Every step is one fp32 operation (tests/aug_ref.py restates them).
 * Bounds: 0 < B <= 65535, 0 < Hc, Wc <= S2F_AUG_MAX_CROP.  16-byte stores when Wc % 4 == 0 and inputs is 16-byte (seg 4-byte)
 * aligned, scalar stores otherwise. */
#define S2F_AUG_CANDIDATES 11
#define S2F_AUG_MAX_CROP 4096
typedef struct S2fAugParams {
  int64_t img_off, seg_off;
  int32_t h0, w0, H, W;
  int32_t crop_y[S2F_AUG_CANDIDATES], crop_x[S2F_AUG_CANDIDATES];
  int32_t flip;
  int32_t bright_on, mode, contrast_on, sat_on, hue_on, hue_delta;
  float bright_beta, contrast_alpha, sat_alpha;
} S2fAugParams;
/* sizeof(S2fAugParams): what a binding checks its mirror of the layout against */
int s2f_aug_param_bytes(void);
int s2f_aug_crop_stats(const uint8_t* data, int64_t data_bytes, const S2fAugParams* params, int B, int Hc, int Wc, int ignore_index,
                       int reduce_zero_label, double cat_max_ratio, int* flags, void* stream);
int s2f_aug_apply(const uint8_t* data, int64_t data_bytes, const S2fAugParams* params, const int* flags, int B, int Hc, int Wc,
                  float mean0, float mean1, float mean2, float std0, float std1, float std2, int bgr_to_rgb, float pad_val,
                  int seg_pad_val, int reduce_zero_label, float* inputs, uint8_t* seg, void* stream);

/* ---- test-time views: the configs' test_pipeline / tta_pipeline + SegDataPreProcessor's test branch (csrc/augment.hip, ABI 39) ----
 * Resize(keep_ratio) -> RandomFlip(prob 0 | 1, horizontal) of every view of a test iteration (the data-set files under mmseg's configs/_base_/datasets:
 * test_pipeline, tta_pipeline: TestTimeAug's scales x flips; the resize itself is mmcv's) and SegDataPreProcessor.forward(training =
 * False) (channel swap, (x - mean) / std, pad right / bottom by test_cfg's size / size_divisor) as ONE launch from the decoded
 * pictures to every view, each a [3, Hp, Wp] fp32 block of its own size inside one packed buffer.  The sizes are computed by the
 * caller and arrive in the table; the kernel is a function of its inputs, allocates nothing and synchronises nothing: capturable
 * in a hipGraph.
 * data: `data_bytes` device bytes holding uint8 HWC BGR pictures [h0, w0, 3] with NO alignment.  params: V table entries in device
 * memory (8-byte aligned), one per (view, image):
 *   img_off : byte offset of the picture in data          out_off : ELEMENT offset of the entry's block in out, a multiple of 4
 *   h0, w0  : source size      H, W : size after the resize      Hp, Wp : padded size, >= H, W      flip : horizontal flip of the
 *   RESIZED picture (before the padding: the padding stays on the right)
 * Entry v, output pixel (c, y, x) of its block:
 *   y < H and x < W : resized pixel (y, flip ? W - 1 - x : x) -- the bilinear sample of the picture with half-pixel centres and no
 *     antialias, scale = in / out, rounded to nearest into uint8: s2f_aug_apply's resize step (both kernels call ONE device
 *     function, sample_bgr), so H == h0 and W == w0 reproduces the source bytes; channel (bgr_to_rgb ? 2 - c : c) of that, (v - mean_c) /
 *     std_c with an IEEE divide (mean 0, std 1: none).  Every step is one fp32 operation (tests/view_ref.py restates them).
 *   elsewhere (up to Hp, Wp) : pad_val itself, un-normalised, as stack_batch pads after the normalisation.
 * Every element of every entry's block is written once; elements of out between the blocks are not touched (the blocks are
 * disjoint: the caller's business).  The table is untrusted: an entry whose block does not fit out (out_off < 0, not a multiple
 * of 4 or out_off + 3 Hp Wp > out_elems; Hp, Wp outside 1 .. max_Hp, max_Wp) is SKIPPED; an entry whose picture does not fit data
 * (or with a non-positive size, or H > Hp, W > Wp) yields an all-pad_val block; tap indices are clamped into the source.  No load
 * leaves data and no store leaves out, whatever the table holds.
 * max_Hp, max_Wp: the largest Hp and the largest Wp of the table (what the grid is sized by: an entry beyond them is skipped).
 * Bounds: 0 < V <= 65535, 0 < max_Hp, max_Wp <= S2F_AUG_MAX_CROP.  16-byte stores for an entry with Wp % 4 == 0 when out is
 * 16-byte aligned (out_off % 4 == 0 then aligns the block), scalar stores otherwise. */
typedef struct S2fViewParams {
  int64_t img_off;
  int64_t out_off;
  int32_t h0, w0;
  int32_t H, W;
  int32_t Hp, Wp;
  int32_t flip;
  int32_t reserved;
} S2fViewParams;
/* sizeof(S2fViewParams): what a binding checks its mirror of the layout against */
int s2f_view_param_bytes(void);
int s2f_test_views(const uint8_t* data, int64_t data_bytes, const S2fViewParams* params, int V, int max_Hp, int max_Wp, float mean0,
                   float mean1, float mean2, float std0, float std1, float std2, int bgr_to_rgb, float pad_val, float* out,
                   int64_t out_elems, void* stream);

/* ---- batched transposition of the last two dimensions: x [B, R, C] -> y [B, C, R] (fp32) -----------------------------------
 * Replaces the `.permute(0, 1, 3, 4, 2)` / `.permute(0, 1, 4, 2, 3)` copies around the DCNv3 sampling core
 * (ops_dcnv3/modules/dcnv3.py:198-233; mmdet/models/layers/detr_layers.py:331-337).  x != y; B < 65536. */
int s2f_transpose_last2(const float* x, float* y, int64_t B, int R, int C, void* stream);
/* y = x^T + add  (add? of y's shape [B, C, R], NULL = absent): as the adjoint of a transposition whose SOURCE has a second reader --
 * the decoder layer's result goes to the prediction stack and, transposed, to the next layer (detr_layers.py:556, maskformer_head.py:554-566)
 * -- the second reader's gradient is summed here instead of by an add launch of the autograd engine. */
int s2f_transpose_last2_add(const float* x, const float* add, float* y, int64_t B, int R, int C, void* stream);
/* y[b][c][r] = q[b][c][r] + g[c] * x[b][r][c]  (x [B, R, C] token-major, q / y [B, C, R] channel-major, g [C]): the pixel decoder's
 * `query + gamma3 * ffn(query)` (detr_layers.py:336-337) with the FFN output's reinterpretation (mmcv_spike/transformer.py:829) as
 * one pass.  Backward: gx[b][r][c] = g[c] gy[b][c][r], gg[c] += sum gy[b][c][r] x[b][r][c] (gg zeroed by the caller; d/dq = gy).
 * R % 64 == 0, C % 64 == 0. */
int s2f_transpose_scale_add_fwd(const float* x, const float* q, const float* g, float* y, int64_t B, int R, int C, void* stream);
int s2f_transpose_scale_add_bwd(const float* gy, const float* x, const float* g, float* gx, float* gg_zeroed, int64_t B, int R, int C,
                                void* stream);

/* ---- mask losses of the Hungarian-matched loss on the 2x up-sampled logits -------------------
 * For matched prediction p: u = bilinear2x(pred[p]) (F.interpolate align_corners=False, dense_heads/maskformer_head.py:475-479),
 * s = sigmoid(u), t = tgt[gt_index[p]] (uint8 0/1, [2h, 2w]):  sums[p] = { sum s t, sum s, sum t, sum focal(u, t) } with the
 * sigmoid focal loss of losses/focal_loss.py:36-44; the naive dice loss (losses/dice_loss.py:45-50) follows from the first
 * three.  Nothing of size [P, 2h, 2w] is materialised forward; backward writes d(sum_k g_sums[p][k] sums[p][k])/du, to be
 * pulled back to the low-resolution logits by s2f_upsample2x_bwd.  w even; targets 4-byte aligned rows (2w % 4 == 0). */
int s2f_mask_loss_fwd(const float* pred, const uint8_t* tgt, const int64_t* gt_index, float* sums, int64_t P, int h, int w,
                      float alpha, float gamma, void* stream);
int s2f_mask_loss_bwd(const float* pred, const uint8_t* tgt, const int64_t* gt_index, const float* g_sums, float* gup, int64_t P,
                      int h, int w, float alpha, float gamma, void* stream);

/* ---- the same loss against SEMANTIC maps: disjoint targets "seg == class" (mmseg/models/decode_heads/maskformer_head.py:53-106) --
 * Matching costs (mmdet task_modules/assigners/match_cost.py:289-297 FocalLossCost(binary_input), :361-371 DiceCost) as segmented
 * sums by label instead of three [L*Q, hw] x [hw, n_gt] products: for image b, prediction row r, class id c < K
 *   out[b][r][c] = sum_{pixels of c} (pos - neg),  out[b][r][K + c] = sum_{pixels of c} s,
 *   out[b][r][2K] = sum_all neg,  out[b][r][2K + 1] = sum_all s        (s = sigmoid(pred), pos / neg the two focal terms)
 * pred [B, R, hw] fp32, seg_small [B, hw] uint8 label map at the predictions' resolution (ids >= K, e.g. the ignore label 255,
 * belong to no class), out [B, R, 2K + 2] fp32.  Sums are accumulated in 64-bit fixed point: run-to-run identical.  hw % 4 == 0.
 * Mask losses: row = (b, r) has the target  seg[b] == row_class[row]  (seg [B, 2h, 2w] uint8; row_class int32, < 0: unmatched row,
 * sums 0 / gradient 0): sums [B*R, 4] as s2f_mask_loss_fwd; the backward returns the gradient w.r.t. the LOW-resolution logits
 * [B, R, h, w] directly (the adjoint of the up-sampling is applied to an LDS tile; no [rows, 2h, 2w] tensor exists). */
int s2f_mask_cost_bins(const float* pred, const uint8_t* seg_small, float* out, int B, int R, int64_t hw, int K, float alpha,
                       float gamma, float eps, void* stream);
/* partials: workspace of s2f_mask_loss_seg_partials(B, R, h, w) floats (need not be zeroed): a row's pixels are cut into chunks whose
 * partial sums are stored there and added in chunk order -- the loss is bit-repeatable (rounds 2-4: fp32 atomics in arrival order). */
int64_t s2f_mask_loss_seg_partials(int B, int R, int h, int w);
int s2f_mask_loss_seg_fwd(const float* pred, const uint8_t* seg, const int32_t* row_class, float* sums, float* partials, int B, int R,
                          int h, int w, float alpha, float gamma, void* stream);
int s2f_mask_loss_seg_bwd(const float* pred, const uint8_t* seg, const int32_t* row_class, const float* g_sums, float* gpred, int B,
                          int R, int h, int w, float alpha, float gamma, void* stream);

/* ---- assignment: the Hungarian matching of that loss on the device (csrc/lsa.hip, ABI 36) ------------------------------------------
 * What loss.MaskFormerLoss.match_tables does on the host (HungarianAssigner: scipy.optimize.linear_sum_assignment per decoder layer
 * and image, mmdet task_modules/assigners/hungarian_assigner.py:126-135), without leaving the stream:
 *   cost [L, B, Q, K] fp32 and count_full [B, 256] fp32 as MaskFormerLoss.costs_all_classes returns them; per image the classes
 *   present are the k < K with count_full[b][k] != 0; per (l, b) the rectangular linear sum assignment of cost[l][b][:, present]
 *   (shortest augmenting paths, Crouse 2016, in fp64 on the fp32 costs; rows <= columns after orientation);
 *   tgt_labels [L, B, Q] int64: class id of the matched column, K = no object;  row_class [B, L*Q] int32: the same, -1 = unmatched;
 *   num_masks [L] fp32 = sum over the images of max(min(Q, n_present), 1);
 *   status [1] int32: 0, or bit 0 = a label in K..254 is present (every num_masks is NaN), bit 1 = a non-finite cost (NaN, +Inf,
 *   -Inf) in a present column (that problem's rows are unmatched, num_masks[l] is NaN).  A non-finite cost in an ABSENT column
 *   is never read.
 * EVERY element of the four outputs is written by every call (two launches, the first writes the status word): no fill precedes a
 * replay inside a hipGraph.  Every loop of the solver has a structural bound; it cannot spin on any input.  Among equal minima
 * the scan takes the column the textbook's list of unscanned columns yields (its first, or its last unassigned one): the tables are
 * those of the host route bit for bit, on matrices with exactly tied totals too.
 * Bounds: L, B, Q >= 1, L * B <= 2^20, Q <= S2F_LSA_MAX_QUERIES, 1 <= K <= S2F_LSA_MAX_CLASSES (255 is the ignored label).  One
 * wave64 per problem, columns striped 4 per lane; the fp64 cost tile sits in LDS while Q * n_present <= 15 000 (Q = 100, K = 150)
 * and is re-read as fp32 from L2 above that. */
#define S2F_LSA_MAX_QUERIES 256
#define S2F_LSA_MAX_CLASSES 254
int s2f_lsa_tables(const float* cost, const float* count_full, int64_t* tgt_labels, int32_t* row_class, float* num_masks,
                   int32_t* status, int L, int B, int Q, int K, void* stream);
/* The same with flags (measurement only, tools/probe_lsa.py): S2F_LSA_TILE_L2 re-reads the fp32 costs from L2 for every problem
 * instead of keeping the fp64 tile in LDS; the tables are the same. */
#define S2F_LSA_TILE_L2 1
int s2f_lsa_tables_ex(const float* cost, const float* count_full, int64_t* tgt_labels, int32_t* row_class, float* num_masks,
                      int32_t* status, int L, int B, int Q, int K, int flags, void* stream);

/* ---- a5 / a10: spike-driven (softmax-free) attention core --------------------------------------------
 * Replaces  kv = k^T @ v ; o = (q @ kv) * scale ; o.transpose(3,4).reshape(T,B,C,N)
 * (MS_Attention_RepConv_qkv_id, mmseg/models/backbones/sdtv2.py:308-339) and the decoder's
 * (q k^T / sqrt(C)) v  ((Cross)MultiHeadAttentionBlock, mmcv_spike/transformer.py:253-274, :334-355 -- no softmax,
 * so the same bilinear form) on spikes laid out channel-major [TB, C, N] (channel c = head*d + j), i.e. directly on
 * the *_spike outputs without the reference's permute/contiguous copies.  d = C / heads <= 64.
 * q, o: [TB, C, Nq]; k, v: [TB, C, Nk]; kv_save: [TB, heads, d, d] (kept for backward).
 * With spike inputs (multiples of 1/D) every partial sum is an exactly representable fp32 while it stays below
 * 2^24 ulps -- the result is then independent of summation order and equals the reference's bit for bit. */
int s2f_sdsa_fwd(const float* q, const float* k, const float* v, float* o, float* kv_save, int TB, int heads, int d,
                 int Nq, int Nk, float scale, void* stream);
/* gq = scale * go kv^T ; gkv = scale * q^T go ; gk = v gkv^T ; gv = k gkv.   gkv_ws: [TB, heads, d, d] scratch.
 * Launches (here and in s2f_sdsa_bwd_bf16): the outer product gkv (after its clear when the token axis is split), then the three
 * applies gq, gk, gv -- independent of one another once gkv exists -- as ONE sdsa_apply_jobs_kernel launch where they take the same
 * workgroup shape, else gk + gv as one launch and gq as another (100 queries against 4 096 or more keys). */
int s2f_sdsa_bwd(const float* q, const float* k, const float* v, const float* kv_save, const float* go, float* gq,
                 float* gk, float* gv, float* gkv_ws, int TB, int heads, int d, int Nq, int Nk, float scale,
                 void* stream);
/* The two building blocks (exported for tests and for callers that fuse differently):
 *   kv[tb,h][i][j]    = alpha * sum_n k[tb, h*d+i, n] * v[tb, h*d+j, n]
 *   y[tb, h*d+j, n]   = alpha * sum_i x[tb, h*d+i, n] * m[tb,h][i][j]      (transpose_m != 0: m[j][i]) */
int s2f_sdsa_kv(const float* k, const float* v, float* kv, int TB, int heads, int d, int N, float alpha, void* stream);
int s2f_sdsa_apply(const float* x, const float* m, float* y, int TB, int heads, int d, int N, float alpha,
                   int transpose_m, void* stream);
/* One to three INDEPENDENT applies (no job reads what another writes) of one TB, heads, d; each keeps the workgroup shape it
 * would have as a launch of its own, jobs that agree on it share one launch (grid z = job), and every output element is computed
 * as by that launch of its own, bit for bit.  `jobs`: njobs * S2F_SDSA_JOB_WORDS int64 words in HOST memory, per job
 *   [0] x, device pointer             [1] batch stride of x, in elements      [2] type of x: 0 = fp32, 1 = bf16 spikes
 *   [3] straight-through mask of x?, device pointer or 0 (layout of s2f_lif_mask_words over the contiguous [TB, C, N]: the
 *       operand is then bit ? x / D : 0, as `go_mask` of s2f_sdsa_bwd_bf16)   [4] D (1..255; read with a mask only)
 *   [5] m [TB, heads, d, d] fp32      [6] y, fp32                             [7] batch stride of y, in elements
 *   [8] N                             [9] alpha: the bits of the float in the low 32 bits      [10] transpose_m
 * bf16 operands need N and the batch stride to be multiples of 4 and an 8-byte aligned pointer (as s2f_sdsa_fwd_bf16).  Every job
 * is checked before anything is launched: a malformed job returns S2F_EINVAL / S2F_EALIGN and nothing is written. */
#define S2F_SDSA_JOB_WORDS 11
int s2f_sdsa_apply_jobs(const int64_t* jobs, int njobs, int TB, int heads, int d, void* stream);

/* The same core on bf16 spike operands (uint16_t storage; what the neuron kernels write with y_bf16): exact, half the bytes.
 * q / k / v may be channel ranges of ONE tensor (the stacked q|k|v map [TB, 3C, N] of the batched projection chain): each
 * operand comes with the distance between its batch elements, in elements (multiples of 4; C*N for a plain [TB, C, N]).
 * s2f_sdsa_bwd_bf16: `go` is the gradient of o [TB, C, Nq] -- or, with go_mask != NULL, the gradient of the SPIKES
 * y = Q_IFNode(o) of the fused forward below: the straight-through estimator (in-range bit ? g / D : 0, mask layout of
 * s2f_lif_mask_words over the contiguous [TB, C, Nq]) is applied inside the loaders, no separate neuron backward pass.
 * gq / gk / gv are fp32 with their own batch strides (three ranges of one [TB, 3C, N] gradient, or three tensors). */
int s2f_sdsa_fwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_batch_stride,
                      int64_t k_batch_stride, int64_t v_batch_stride, float* o, float* kv_save, int TB, int heads, int d,
                      int Nq, int Nk, float scale, void* stream);
int s2f_sdsa_bwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_batch_stride,
                      int64_t k_batch_stride, int64_t v_batch_stride, const float* kv_save, const float* go,
                      const uint64_t* go_mask, int D, float* gq, float* gk, float* gv, int64_t gq_batch_stride,
                      int64_t gk_batch_stride, int64_t gv_batch_stride, float* gkv_ws, int TB, int heads, int d, int Nq,
                      int Nk, float scale, void* stream);
/* Attention core AND the neuron behind it as one kernel -- north_star's "spike-masked attention + LIF as one CDNA4 kernel"
 * for the backbone's self-attention (sdtv2.py:335-342: kv = k^T v; o = scale q kv; attn_spike(o)): one workgroup per
 * (tb, head); kv on the matrix cores straight from memory (contraction-contiguous bf16 rows, exact), kept in LDS for the
 * q kv product; o never reaches HBM: the Q_IFNode update of s2f_lif_fwd (reset membrane) runs in the epilogue and writes
 * y as bf16 spikes [TB, C, N] + the 1-bit in-range mask (mask? NULL == no backward) + the firing counters (stats? as
 * s2f_lif_fwd).  kv_save [TB, heads, d, d] leaves for the backward pass.  Needs N % 256 == 0, batch strides % 8 == 0. */
int s2f_sdsa_lif_fwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_batch_stride,
                          int64_t k_batch_stride, int64_t v_batch_stride, uint16_t* y_spikes, uint64_t* mask, uint64_t* stats,
                          float* kv_save, int TB, int heads, int d, int N, float scale, float vth, int D, void* stream);
/* The same without the in-range mask -- inference, where nothing is back-propagated -- for any Nq % 4 == 0 and separate key length
 * Nk: the decoder's 100-query attention blocks (mmcv_spike/transformer.py:238-300).  kv_ws [TB, heads, d, d] is scratch. */
int s2f_sdsa_lif_fwd_bf16_nomask(const uint16_t* q, const uint16_t* k, const uint16_t* v, int64_t q_batch_stride,
                                 int64_t k_batch_stride, int64_t v_batch_stride, uint16_t* y_spikes, uint64_t* stats, float* kv_ws,
                                 int TB, int heads, int d, int Nq, int Nk, float scale, float vth, int D, void* stream);

/* ---- a9: DCNv3 core ---------------------------------------------------------------------------------
 * Replaces dcnv3_core_pytorch (ops_dcnv3/functions/dcnv3_func.py:147-189; = the dormant CUDA op
 * dcnv3_forward/backward, ops_dcnv3/src/dcnv3.h:20-59, same geometry tuple).  Layouts:
 *   input [N, H, W, G*Cg]; offset [N, Ho, Wo, G*K*K*2] ((x, y) per tap, tap k = i_w*Kh + j_h);
 *   mask [N, Ho, Wo, G*K*K]; output [N, Ho, Wo, G*Cg].   Bilinear, zero outside the zero-padded input. */
int s2f_dcnv3_fwd(const float* input, const float* offset, const float* mask, float* output, int N, int H, int W,
                  int G, int Cg, int Kh, int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w,
                  float offset_scale, void* stream);
/* All three gradients are fully overwritten (grad_input need not be zeroed).  When one (n, group) slice fits in the
 * CU's LDS (12*H*W*Cg bytes + a staging chunk <= 160 KiB) the scatter-add into grad_input runs in LDS in 64-bit fixed
 * point (order-independent, see csrc/dcnv3.hip); larger maps fall back to fp32 global atomics after a memset. */
int s2f_dcnv3_bwd(const float* input, const float* offset, const float* mask, const float* grad_output,
                  float* grad_input, float* grad_offset, float* grad_mask, int N, int H, int W, int G, int Cg, int Kh,
                  int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale,
                  void* stream);
/* The same core on CHANNEL-MAJOR maps: input / grad_input [N, G*Cg, H*W], output / grad_output [N, G*Cg, Ho*Wo]; offset, mask and
 * their gradients keep the layouts above.  One workgroup owns an (n, group) slice -- Cg contiguous planes, staged in LDS -- in the
 * forward as in the backward, so only maps whose slice fits one workgroup's LDS are taken: s2f_dcnv3_cm_ok says which (1 / 0, no
 * launch), and the two entry points return S2F_EINVAL, before any launch, for every other geometry (the caller transposes and uses
 * the [N, H, W, C] entry points there).  Results are bit-identical to those entry points on the transposed maps. */
int s2f_dcnv3_cm_ok(int N, int H, int W, int G, int Cg, int Kh, int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                    int dil_w);
int s2f_dcnv3_fwd_cm(const float* input, const float* offset, const float* mask, float* output, int N, int H, int W, int G, int Cg,
                     int Kh, int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale,
                     void* stream);
int s2f_dcnv3_bwd_cm(const float* input, const float* offset, const float* mask, const float* grad_output, float* grad_input,
                     float* grad_offset, float* grad_mask, int N, int H, int W, int G, int Cg, int Kh, int Kw, int stride_h,
                     int stride_w, int pad_h, int pad_w, int dil_h, int dil_w, float offset_scale, void* stream);
/* Which kernels the four entry points above run for a geometry (ABI 54) -- the very function they dispatch on; launches nothing,
 * needs no device.  `aligned16`: the maps read and written in 16-byte vectors (input and output in the forward, input and grad_output in the
 * backward) start at multiples of 16 bytes.  Writes S2F_DCN_ROUTE_FIELDS integers to `out`:
 *   [0] the [N, H, W, C] forward kernel                       S2F_DCN_FWD_*
 *   [1] the [N, H, W, C] backward route                       S2F_DCN_BWD_*
 *   [2] workgroups per (n, group) slice of that backward:     1 (LDS), the band count (BANDED), 0 (global atomics)
 *   [3] the channel-major entry points take the geometry      1 / 0 (= s2f_dcnv3_cm_ok); [4] .. [6] are 0 without it
 *   [4] the channel-major forward kernel                      S2F_DCN_CM_FWD_*
 *   [5] floats per staged pixel row of that kernel            Cg or Cg + 4
 *   [6] the channel-major backward kernel's form              S2F_DCN_CM_BWD_*
 * The backward route depends on the environment variable S2F_DCN_FORCE_BANDS (tests: a value b > 1 bands a map that would fit one
 * workgroup into b bands), which is read here, per call.  The route ids, every one a distinct number:
 *   FWD_K3C8     the 3x3 / Cg = 8 geometry unrolled, 16-byte accesses
 *   FWD_VEC4     the generic loops, four channels at a time;   FWD_SCALAR  one at a time (Cg % 4 != 0, or a map off the 16-byte grid)
 *   BWD_LDS      one workgroup per (n, group) slice, the scatter-add in LDS in fixed point
 *   BWD_BANDED   several workgroups per slice, each owning a band of input rows
 *   BWD_ATOMIC_VEC4 / _SCALAR   fp32 global atomics after a memset, four channels / one channel at a time
 *   CM_FWD_K3C8 / CM_FWD_GENERIC   the channel-major forward with the 3x3 / Cg = 8 sizes compiled in / with the generic loops
 *   CM_BWD_PLAIN one global round trip per 256-pixel chunk;  CM_BWD_PIPE  the next chunk prefetched into registers;
 *   CM_BWD_PIPE_K3C8  the same with the 3x3 / Cg = 8 sizes compiled in */
#define S2F_DCN_ROUTE_FIELDS 7
#define S2F_DCN_FWD_K3C8 1
#define S2F_DCN_FWD_VEC4 2
#define S2F_DCN_FWD_SCALAR 3
#define S2F_DCN_BWD_LDS 11
#define S2F_DCN_BWD_BANDED 12
#define S2F_DCN_BWD_ATOMIC_VEC4 13
#define S2F_DCN_BWD_ATOMIC_SCALAR 14
#define S2F_DCN_CM_FWD_K3C8 21
#define S2F_DCN_CM_FWD_GENERIC 22
#define S2F_DCN_CM_BWD_PLAIN 31
#define S2F_DCN_CM_BWD_PIPE 32
#define S2F_DCN_CM_BWD_PIPE_K3C8 33
int s2f_dcnv3_route(int N, int H, int W, int G, int Cg, int Kh, int Kw, int stride_h, int stride_w, int pad_h, int pad_w, int dil_h,
                    int dil_w, int aligned16, int* out);

/* ---- f2: one training iteration's parameter update (csrc/optim.hip, round 5) -------------------------------------------
 * Replaces mmengine OptimWrapper.update_params for the Spike2Former configs
 * (configs/Spike2Former/SDTv2_maskformer_DCNpixelDecoder_ade20k.py:137-155): torch.nn.utils.clip_grad_norm_(max_norm = 0.01,
 * norm_type = 2) + torch.optim.AdamW.step() with one (lr, weight_decay) pair per parameter (`custom_keys` multipliers), over
 * the flat gradient buffer of the data-parallel step (dist.FlatGradAllReduce: 16-byte-aligned slots, zero pads).
 *   s2f_grad_sqnorm_parts(n)   number of fp64 partials s2f_grad_sqnorm writes for n elements
 *   s2f_grad_sqnorm            partials[i] = sum of g^2 over the i-th run of 16 384 elements (plain stores: bit-repeatable)
 *   s2f_adamw_prepare          state[0] = clip coefficient min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: 1), [1] = norm,
 *                              [4] += 1 (the step count t), [2] = 1 - beta1^t, [3] = sqrt(1 - beta2^t); state = float[8], zeroed
 *                              by the caller before the first iteration
 *   s2f_adamw_step             slots int64 [nslots][3] = {parameter pointer, slot offset in g / m / v (elements, % 4 == 0),
 *                              numel}; hyper float [nslots][2] = {lr, weight_decay} of THIS iteration; chunks int32 [nchunks][2]
 *                              = {slot, first element} covering every slot in runs of s2f_adamw_chunk_elems();
 *                              g' = g * state[0]; p *= 1 - lr wd; m += (g' - m)(1 - beta1); v = beta2 v + (1 - beta2) g'^2;
 *                              p -= lr / state[2] * m / (sqrt(v) / state[3] + eps)      (torch/optim/adamw.py, single-tensor form)
 * All tables are DEVICE memory; nothing synchronises, so the three launches can be captured behind the step's hipGraph.
 *
 * Gradient accumulation over the same buffer (mmengine OptimWrapper(accumulative_counts = k); ABI 51):
 *   s2f_grad_accumulate        out[i] = fl(acc[i] + fl(scale * g[i])), or fl(scale * g[i]) with acc == NULL: two fp32 roundings, never
 *                              contracted into an fma; non-finite values propagate.  `out` may be `g` or `acc` (each element is read and
 *                              written by one thread); any other overlap is the caller's error.  16-byte accesses on whole groups of
 *                              four, scalar ones in the tail; one workgroup per run of 16 384 elements, as s2f_grad_sqnorm.
 *                              partials: NULL, or s2f_grad_sqnorm_parts(n) doubles: partials[i] = sum of g^2 of the INPUT g over run
 *                              i, bit-identical to what s2f_grad_sqnorm writes for that buffer (plain stores).  n == 0: S2F_OK, no
 *                              launch.  S2F_EINVAL: g or out NULL, n < 0; S2F_EALIGN: g / acc / out not 16-byte aligned, partials not
 *                              8-byte aligned.
 *   s2f_grad_accum_stats       ONE workgroup of 256 threads.  micro double [rows][nparts]; every row and accum_parts[nparts] is summed
 *                              in s2f_adamw_prepare's fixed order, the row sums are added in ascending row order.
 *                              stats[0] = (float)(sum of the row sums / rows), [1] = (float)(sum of accum_parts), [2] = rows, [3] = 0.
 *                              Bit-repeatable.  S2F_EINVAL: null pointer, rows < 1, nparts < 1.
 * Neither allocates or synchronises: both can be captured. */
int64_t s2f_grad_sqnorm_parts(int64_t n);
int s2f_grad_sqnorm(const float* g, int64_t n, double* partials, void* stream);
int s2f_adamw_prepare(const double* partials, int nparts, float max_norm, double beta1, double beta2, float* state, void* stream);
int s2f_grad_accumulate(const float* g, const float* acc, float* out, int64_t n, float scale, double* partials, void* stream);
int s2f_grad_accum_stats(const double* micro, int rows, const double* accum_parts, int nparts, float* stats, void* stream);
int s2f_adamw_chunk_elems(void);
int s2f_adamw_step(const int64_t* slots, const float* hyper, const int32_t* chunks, int nchunks, const float* g, float* m, float* v,
                   const float* state, double beta1, double beta2, float eps, void* stream);

/* ---- training loop: device-side log and one-launch state snapshot (csrc/trainstate.hip, ABI 44) ----------------------------------
 * What mmengine's IterBasedTrainLoop + LoggerHook + CheckpointHook need from a step that never waits for the GPU
 * (configs/_base_/schedules/schedule_160k.py, configs/_base_/default_runtime.py): the scalars of every iteration, and the weights.
 *   s2f_state_copy         one launch copies every tensor of a pointer table into `flat` (to_params = 0) or back (to_params = 1).
 *                          slots int64 [nslots][3] = {tensor pointer, slot offset in flat, length}, chunks int32 [nchunks][2] =
 *                          {slot, first word} covering every slot in runs of s2f_adamw_chunk_elems() -- the tables of
 *                          s2f_adamw_step, but offsets and lengths count 32-BIT WORDS: the kernel copies bits and knows no dtype
 *                          (an int64 tensor is two words per element).  A tensor pointer is 4-byte aligned at least; slot offsets
 *                          are multiples of 4 words, so that a slot of the 16-byte-aligned `flat` is 16-byte aligned.  Where a
 *                          chunk's two addresses are both 16-byte aligned it moves 16 bytes per access, else word by word.
 *                          Words of `flat` between and behind the slots are never written.  Plain vector loads and stores.
 *                          S2F_EINVAL: null pointer, nchunks <= 0, to_params not 0 / 1; S2F_EALIGN: flat not 16-byte aligned.
 *   s2f_train_log_append   srcs: DEVICE table of n device pointers to fp32 scalars; ring float [window][stride]; head int64 [2] on
 *                          the device: head[0] = rows appended so far, head[1] = the value of head[0] at the first row that held
 *                          a non-finite value, or -1 (the caller initialises {0, -1}; sticky, survives the ring's wrap).  One
 *                          workgroup writes the n values into row head[0] % window (columns n .. stride - 1 are not written),
 *                          then advances head[0].  Appends are ordered by the stream; nothing else writes head.
 *                          S2F_EINVAL: null pointer, n outside 1 .. S2F_TRAIN_LOG_MAX_TERMS, stride < n, window < 1;
 *                          S2F_EALIGN: srcs / head not 8-byte, ring not 4-byte aligned.
 * All tables are DEVICE memory; neither call allocates, synchronises or uses atomics: both can be captured into the step's hipGraph. */
#define S2F_TRAIN_LOG_MAX_TERMS 256
int s2f_state_copy(const int64_t* slots, const int32_t* chunks, int nchunks, void* flat, int to_params, void* stream);
int s2f_train_log_append(const float* const* srcs, int n, float* ring, int window, int stride, int64_t* head, void* stream);

/* ---- firing log: per-neuron firing rows from inside the captured step (csrc/firinglog.hip, ABI 45) -------------------------------
 * The neuron kernels count into `stats` (above: uint64[S2F_STAT_SLOTS][2] per neuron); this launch is the device-side path from those
 * counters to a log that the host reads once per interval (tools/cal_firing_num.py reads its hooks' sums on the host, per image).
 *   s2f_firing_log_append  counters uint64 [n][S2F_STAT_SLOTS][2], ONE allocation: neuron i's `stats` is the slice i.  ring int64
 *                          [window][n][2]; silent int32 [n]; head int64 [4], initialised by the caller to {0, -1, 0, 0}.  One launch,
 *                          one wave per neuron i:
 *                            {sum, nonzero} = the 64-bit sums of the neuron's 256 slots  ->  ring[head[0] % window][i];
 *                            the neuron's 512 counter words are cleared (the next iteration counts from zero);
 *                            silent[i] == -1 (not watched: a neuron the step never runs) stays -1; otherwise silent[i] becomes
 *                            silent[i] + 1 where sum == 0, and 0 where it is not;
 *                            where silent[i] REACHES `patience`, the event head[0] * 2^32 + i is offered to head[1], which keeps
 *                            the minimum under UNSIGNED comparison (-1: none yet) -- the lowest neuron of the earliest row,
 *                            whatever order the workgroups finish in; a later event never replaces it.
 *                          head[0], the number of rows appended, advances exactly once per launch: every workgroup uses the value
 *                          it had at entry.  head[2] is the launch's own workspace (the ticket of a last-workgroup-done scheme),
 *                          0 at entry and on exit; head[3] is reserved.  Appends are ordered by their stream.
 *                          S2F_EINVAL: null pointer, n < 1, window < 1, patience < 1; S2F_EALIGN: counters not 16-byte, ring / head
 *                          not 8-byte, silent not 4-byte aligned.
 * Plain vector loads and stores and ordinary global atomics (one add and at most one min per neuron); nothing allocates or
 * synchronises: capturable behind the step's last launch. */
int s2f_firing_log_append(uint64_t* counters, int n, int64_t* ring, int window, int32_t* silent, int patience, int64_t* head,
                          void* stream);

/* ---- gradient log: per-parameter gradient, weight and update norms from inside the step (csrc/gradlog.hip, ABI 50) ---------------
 * Where the gradient goes, per parameter tensor and iteration, without ~1 000 norm launches and a host stop: a segmented reduction
 * over the buffers s2f_adamw_step has just updated, into a ring the host reads once per interval.  Per parameter i and iteration one
 * row of eight 8-byte words -- columns 0-3 doubles stored by bit pattern, columns 4-7 int64:
 *     0  sum g^2 over the finite elements of the raw gradient (as the all-reduce left it, before clipping)
 *     1  sum p^2 over the finite elements of the parameter AFTER the update
 *     2  sum u^2 over the finite u = step_size * (m / (sqrtf(v) / bc2s + eps)), the Adam step just applied without the decay term:
 *        the fp32 expressions of s2f_adamw_step in their order, from the post-update m, v, hyper and state[2], state[3]; u = 0 for a
 *        parameter with lr < 0 (no gradient)
 *     3  max |g| over the finite elements (0 if none)        4  elements with g == 0        5  non-finite elements of g
 *     6  elements whose p or u is non-finite                  7  numel
 * Only numel elements count, never the zero pads of the 16-byte slots.
 *   s2f_grad_log_span_elems  the most elements of one span (16 384).
 *   s2f_grad_log_partials    slots, hyper, g, m, v, state: the arguments of s2f_adamw_step, after it ran.  spans int32 [nspans][2] =
 *                            {slot, first element}: every parameter in runs of s2f_grad_log_span_elems(), sorted by slot (built on
 *                            the host, once).  One workgroup per span; 16-byte loads where the parameter pointer is 16-byte aligned,
 *                            scalar loads otherwise and in the tail; fp64 accumulation per thread and a fixed-order tree over the
 *                            block; partials int64 [nspans][8] <- the row's columns over the span (column 7: the span's elements),
 *                            plain stores.  Bit-repeatable.
 *                            S2F_EINVAL: null pointer, nspans < 1; S2F_EALIGN: g / m / v not 16-byte, slots / partials not 8-byte.
 *   s2f_grad_log_rows        one wave per parameter i of n combines its spans' partials IN SPAN ORDER (sums add, max of max, counts
 *                            add; a parameter without elements gets a row of zeros) -> ring int64 [window][n][8] at row
 *                            head[0] % window.  streak int32 [n][2]: [i][0] counts the rows in a row whose gradient was all zero
 *                            (column 4 == column 7 > 0), [i][1] those with column 5 > 0.  head int64 [4], initialised by the caller
 *                            to {0, -1, 0, -1}: where streak[i][0] REACHES `patience` the event head[0] * 2^32 + i is offered to
 *                            head[1], where streak[i][1] becomes 1 to head[3]; both keep the minimum under UNSIGNED comparison
 *                            (-1: none yet) -- the lowest parameter of the earliest row, whatever order the workgroups finish in.
 *                            head[0] advances exactly once per launch by the ticket in head[2] (0 at entry and on exit), as in
 *                            s2f_firing_log_append; the words of head see agent-scope atomics only.
 *                            S2F_EINVAL: null pointer, nspans / n / window / patience < 1; S2F_EALIGN: partials / ring / head not
 *                            8-byte, streak not 4-byte aligned.
 * Both launches only READ g, m, v, the parameters, hyper and state; nothing allocates or synchronises: capturable behind
 * s2f_adamw_step.  No floating-point value passes between workgroups inside a launch. */
int s2f_grad_log_span_elems(void);
int s2f_grad_log_partials(const int64_t* slots, const float* hyper, const int32_t* spans, int nspans, const float* g, const float* m,
                          const float* v, const float* state, float eps, int64_t* partials, void* stream);
int s2f_grad_log_rows(const int32_t* spans, int nspans, const int64_t* partials, int n, int64_t* ring, int window, int32_t* streak,
                      int patience, int64_t* head, void* stream);

/* ---- weight averaging: an exponential moving average of the parameters behind the update (csrc/ema.hip, ABI 52) -------------------
 * mmengine's EMAHook with ExponentialMovingAverage / ExpMomentumEMA (custom_hooks = [dict(type='EMAHook', ...)]) is one lerp_ per
 * parameter tensor and iteration on the host's side of the step; here it is one table-driven launch behind s2f_adamw_step, one
 * workgroup per chunk.  slots int64 [nslots][3] = {parameter pointer (fp32, 4-byte aligned at least), slot offset in `ema` (elements,
 * % 4 == 0), numel}, chunks int32 [nchunks][2] = {slot, first element}: the tables of s2f_adamw_step.  `ema`: an fp32 flat buffer in
 * the layout of the moments, 16-byte aligned.  16-byte accesses where both addresses of a chunk are 16-byte aligned, word by word
 * otherwise and in a chunk's last partial group; elements of `ema` outside the slots are never written.
 *   s2f_ema_update   state: the optimizer's float[8]; behind s2f_adamw_prepare state[4] = t is the 1-based count of THIS update (an fp32
 *                    holds it exactly up to 2^24 updates; past that the count, and with it the decision below, stops moving).  Every
 *                    workgroup derives the same decision from t, begin and interval (mmengine 0.8.4: EMAHook._ema_started,
 *                    BaseAveragedModel.update_parameters):
 *                        c = t - max(begin, 1)            the started updates before this one
 *                        c <= 0                           e = p, bit for bit (not started, or the first started update)
 *                        c > 0, c % interval != 0         nothing is touched: ema and partials stay as they were
 *                        otherwise                        m = table[min(c, ntable - 1)];  e = fl(e + fl(m * fl(p - e)))
 *                    -- three fp32 operations, each rounded to nearest even on its own (never contracted), denormals kept; a NaN
 *                    result is stored as the ONE quiet NaN 0x7fc00000, whatever the operands' payloads were, so that the result's bits
 *                    are a function of the operands' VALUES alone.  table: fp32 [ntable] momenta, computed by the host in fp64 and
 *                    rounded once; the device evaluates no exp.  partials?: double [nchunks][2], row i <- {sum ((double)p - (double)e)^2,
 *                    sum (double)e^2} over chunk i's elements after the update (fp64 per thread, a tree of fixed shape, plain stores:
 *                    bit-repeatable); overwritten by every update that is not skipped.
 *                    S2F_EINVAL: null pointer, nchunks < 1, ntable < 1, begin < 0, interval < 1; S2F_EALIGN: ema not 16-byte, partials
 *                    not 8-byte aligned.
 *   s2f_ema_swap     every parameter <-> its slot of `ema`.  Bits: no arithmetic, NaN payloads survive; twice is the identity.
 *                    S2F_EINVAL: null pointer, nchunks < 1; S2F_EALIGN: ema not 16-byte aligned.
 * Loading and saving the buffer needs no entry point of its own: for fp32 parameters s2f_state_copy's word-counted tables ARE these
 * tables.  Neither call allocates, synchronises or uses atomics: both can be captured. */
int s2f_ema_update(const int64_t* slots, const int32_t* chunks, int nchunks, float* ema, const float* state, const float* table,
                   int ntable, int begin, int interval, double* partials, void* stream);
int s2f_ema_swap(const int64_t* slots, const int32_t* chunks, int nchunks, float* ema, void* stream);

/* ---- segmentation log: train-crop accuracy and mIoU from inside the captured step (csrc/seglog.hip, ABI 53) -------------------------
 * mmseg's BaseDecodeHead logs decode.acc_seg with every loss; the reference's MaskFormerHead logs losses only.  The step holds the
 * decoder's class scores, its mask logits and the label map on the device, so the score is two launches of the step and a ring the
 * host reads once per log line.  Per scored layer l, image b and pixel p = (y, x) of the h x w mask prediction
 *     P[q][k]  = softmax(cls[l][b][q][0 .. K])[k], k < K            (the void column is dropped: MaskFormerHead.predict)
 *     score[k] = sum over q, ascending, of P[q][k] * sigmoid(mask[b][l*Q + q][p])           (fp32, one fma per term)
 *     pred     = the first maximum of score (NaN larger than any number: s2f_seg_argmax's rule)
 *     label    = seg[b][2y][2x]                                     (the sub-sampling of the matching costs; 255 = ignored)
 * and a pixel with label < K adds 1 to label[label], 1 to pred[pred] and, where pred == label, 1 to intersect[label]; any other pixel
 * counts nowhere.  A row of the ring is int64 [nl][3][K] = {intersect, pred, label} per scored layer: the totals of
 * IoUMetric.intersect_and_union over the batch, at the MASK resolution (predict scores the up-sampled masks: a training diagnostic,
 * not the validation metric).
 *   s2f_seg_log_tile_pixels  the pixels one workgroup of s2f_seg_log_partials scores (256).
 *   s2f_seg_log_partials     mask fp32 [B][L*Q][h*w], the head's own buffer; cls fp32 [L][B][Q][K+1]; seg uint8 [B][2h][2w], read with
 *                            stride 2; layers: HOST memory, int32 [nl], the scored layers (read and checked during the call, passed
 *                            to the kernel by value: nl <= S2F_SEG_LOG_MAX_LAYERS).  One workgroup per tile of
 *                            s2f_seg_log_tile_pixels() pixels of one (scored layer, image); the softmax table is built in LDS in
 *                            chunks of 32, 76 or 128 classes (chosen by K) x 128 or 64 queries (at most 38 KB whatever Q and K are; a row's
 *                            sum of exponentials in fp64),
 *                            the Q mask logits of a pixel are re-read per class chunk.  partials int32 [nl * B * tiles][3][K], tiles =
 *                            ceil(h*w / s2f_seg_log_tile_pixels()): slice (i*B + b)*tiles + t <- the counts of tile t of image b in
 *                            scored layer i, plain stores (every word is written).
 *                            S2F_EINVAL: null pointer, K outside 1 .. 254, Q < 1, L < 1, B outside 1 .. 65535, w odd or h*w % 4 != 0,
 *                            nl outside 1 .. S2F_SEG_LOG_MAX_LAYERS, a layer outside 0 .. L-1; S2F_EALIGN: mask / cls / partials not
 *                            4-byte aligned.
 *   s2f_seg_log_rows         one workgroup per scored layer i of nl adds its per_layer (= B * tiles) partials (sixteen waves, each
 *                            every sixteenth partial; integers, so the order does not matter) ->
 *                            ring int64 [window][nl][3][K] at row head[0] % window: overwritten, never accumulated into.  streak int32
 *                            [K], from the LAST scored layer's totals: streak[c] = 0 where intersect[c] > 0, + 1 where label[c] > 0
 *                            and intersect[c] == 0, unchanged where the class is absent.  head int64 [4], initialised by the caller
 *                            to {0, -1, 0, 0}: where streak[c] REACHES `patience` the event head[0] * 2^32 + c is offered to head[1],
 *                            which keeps the minimum under UNSIGNED comparison (-1: none yet).  head[0] advances exactly once per
 *                            launch by the ticket in head[2] (0 at entry and on exit), as in s2f_firing_log_append.
 *                            S2F_EINVAL: null pointer, K outside 1 .. 254, nl outside 1 .. S2F_SEG_LOG_MAX_LAYERS, per_layer / window /
 *                            patience < 1; S2F_EALIGN: ring / head not 8-byte, partials / streak not 4-byte aligned.
 * Both launches only READ mask, cls and seg; no global atomics on the rows (LDS counters inside a workgroup, the head's words as
 * above); nothing allocates or synchronises: capturable behind the step's last launch. */
#define S2F_SEG_LOG_MAX_LAYERS 32
int s2f_seg_log_tile_pixels(void);
int s2f_seg_log_partials(const float* mask, const float* cls, const uint8_t* seg, const int32_t* layers, int nl, int L, int B, int Q,
                         int K, int h, int w, int32_t* partials, void* stream);
int s2f_seg_log_rows(const int32_t* partials, int nl, int per_layer, int K, int64_t* ring, int window, int32_t* streak, int patience,
                     int64_t* head, void* stream);

/* ---- match log: what the Hungarian assignment did, from inside the captured step (csrc/matchlog.hip, ABI 56) ------------------------
 * With the assignment on the device (s2f_lsa_tables) its tables never reach the host.  Two read-only launches behind it turn them,
 * the costs the assignment read and the decoder's class logits into one row of figures per replay, in a ring the host reads once per
 * log line.  None of the figures has a counterpart in the reference, whose MaskFormerHead logs losses only; `cls_hit` is the count
 * behind DETR's class_error.  cost fp32 [L][B][Q][K] and row_class int32 [B][L*Q] as s2f_lsa_tables reads and writes them, cls fp32
 * [L][B][Q][K+1] (logits, the void column last).  Query q of (layer l, image b) is MATCHED to class c = row_class[b][l*Q + q] where
 * 0 <= c < K; ANY other value (-1, or one >= K) counts as unmatched and is never used as an index.  Per layer l, summed over the B
 * images, S2F_MATCH_LOG_FIELDS = 6 int64 fields:
 *   [0] matched        the matched queries
 *   [1] cost           the bits of the fp64 sum of (double)cost[l][b][q][c] over the matched pairs: per (l, b) ONE serial sum from +0.0
 *                      with q ascending, then the images' sums added from +0.0 with b ascending.  No float atomics, no tree.
 *   [2] greedy         the matched pairs whose q is the first arg-min of cost[l][b][:][c] over all Q queries: best = the value at
 *                      q = 0, then strict < in fp32 with q ascending (a NaN at q = 0 stands, any other NaN never wins)
 *   [3] moved          for l >= 1: the matched pairs whose class c is matched to another query in layer l-1 of the same image, or to
 *                      none there; 0 for l = 0.  (Were a class named by two queries of one layer, its lowest query owns it.)
 *   [4] cls_hit        the matched pairs whose first arg-max of cls[l][b][q][0 .. K] equals c: best = the value at index 0, then
 *                      strict > with the index ascending (a NaN at index 0 stands, any other NaN never wins)
 *   [5] unmatched_obj  the unmatched queries whose first arg-max is not the void column K
 * A problem the assignment flagged (its rows all -1) so adds to [5] alone.  usage[q] = the images in which the LAST layer matched
 * query q.  A row of the ring is int64 [6L] followed by usage as int32 [Q], padded with a zero to whole 8-byte words:
 * 6L + ceil(Q/2) words.
 *   s2f_match_log_partials  one workgroup per (l, b): partials int64 [L][B][6] and flags int32 [B][Q] (1: the last layer matched q in
 *                           image b), plain stores, every word written.  S2F_EINVAL before any launch: null pointer, L outside
 *                           1 .. S2F_MATCH_LOG_MAX_LAYERS, B outside 1 .. 65535, Q outside 1 .. S2F_LSA_MAX_QUERIES, K outside
 *                           1 .. S2F_LSA_MAX_CLASSES; S2F_EALIGN: partials not 8-byte, another pointer not 4-byte aligned.
 *   s2f_match_log_rows      ONE workgroup: row head[0] % window of ring int64 [window][6L + ceil(Q/2)] <- the sums above
 *                           (overwritten, never accumulated into); idle int32 [Q]: idle[q] = 0 where usage[q] > 0, + 1 otherwise;
 *                           head int64 [4], initialised by the caller to {0, -1, 0, 0}: where idle[q] REACHES `patience` the event
 *                           head[0] * 2^32 + q is offered to head[1], which keeps the minimum under UNSIGNED comparison (-1: none
 *                           yet); then head[0] + 1 is stored.  One workgroup: head[2] (the ticket of the other rings) is not used.
 *                           S2F_EINVAL: null pointer, L / B / Q as above, window or patience < 1; S2F_EALIGN: partials / ring / head
 *                           not 8-byte, usage / idle not 4-byte aligned.
 * Both launches only READ cost, cls and row_class; every loop is bounded by L, B, Q or K; nothing allocates or synchronises:
 * capturable behind the step's last launch. */
#define S2F_MATCH_LOG_MAX_LAYERS 16
#define S2F_MATCH_LOG_FIELDS 6
int s2f_match_log_partials(const float* cost, const float* cls, const int32_t* row_class, int L, int B, int Q, int K, int64_t* partials,
                           int32_t* usage, void* stream);
int s2f_match_log_rows(const int64_t* partials, const int32_t* usage, int L, int B, int Q, int64_t* ring, int window, int32_t* idle,
                       int patience, int64_t* head, void* stream);

/* ---- operand census:what a synaptic op really reads (csrc/opcensus.hip, ABI 49) -----------------------------------------------------
 * The reference's tools/cal_firing_num.py stops at firing rates per neuron (fr_rate.csv) and leaves operations and energy to a
 * spreadsheet.  Not every synaptic layer reads a neuron's output (SepConv.pwconv2 reads the depthwise convolution's real-valued map, the
 * stem the image, the attention / DCNv3 / mask products tensors no neuron counter describes), so the census measures the OPERANDS:
 *   s2f_operand_census   x: n contiguous elements, fp32 (dtype S2F_CENSUS_F32) or bf16 (S2F_CENSUS_BF16), aligned to the element only
 *                        (any element offset into a larger buffer; nothing outside x[0 .. n) is read); D: the level grid, >= 1;
 *                        row: int64 [8] on the device, ONE launch adds one operand into it:
 *                          row[0] += n                   elements
 *                          row[1] += sum level(x)        level(x) = x * D where that is an integer in [0, 65535], else 0
 *                          row[2] += #{x != 0}           (-0.0 counts as zero)
 *                          row[3] += #{x off the grid}   x * D not an integer, or < 0, or > 65535, or x not finite
 *                          row[4]  = max(row[4], max level)
 *                          row[5] += #{x not finite}
 *                          row[6] += 1                   calls
 *                          row[7]                        reserved, stays 0
 *                        The product x * D is ONE fp32 multiply of x (a bf16 element widened exactly) by D converted to fp32, rounded
 *                        to nearest even, and the integer test is made on that rounded product.  For D a power of two (every shipped
 *                        config) the product is exact; for any other D an x whose exact product is within half an ulp of an integer
 *                        counts as on the grid (1/3 as fp32 at D = 3 is level 1).  A subnormal x is off the grid.
 *                        Integer sums and 64-bit atomics (one per field and workgroup): the row does not depend on the order of
 *                        arrival, two runs give the same bits.  n == 0 adds one call and nothing else.
 *                        S2F_EINVAL before any launch: null pointer, n < 0, D < 1, unknown dtype; S2F_EALIGN: x not aligned to its
 *                        element, row not 8-byte aligned.  Nothing allocates or synchronises.
 * Counting rules of the census built on it (spike2former_amd/energy.py: OpCensus / EnergyReport).  MACs of one call:
 *     dense k x k conv        N C_out H_out W_out (C_in / groups) kh kw
 *     depthwise conv          N C H_out W_out kh kw
 *     1x1 conv / conv1d / linear   rows C_in C_out          (rows: every position the weight is applied at)
 *     spike-driven attention  two products: k^T v = TB heads N_k d d  and  q (k^T v) = TB heads N_q d d  (csrc/sdsa.hip contracts in
 *                             this association; the softmax-free form has no N_q x N_k product)
 *     masked attention        q k^T and (q k^T) v: TB heads N_q N_k d each (csrc/sdsa_masked.hip; the mask forbids the association)
 *     DCNv3 core              5 N H_out W_out G Cg K: per sampling point and channel 4 bilinear taps and 1 modulation
 *     mask contraction        T B (L Q) C H W
 *     class_mask_product      B K Q H W
 * An operand is ON THE GRID when its row[3] == 0.  An op with at least one activation operand on the grid is accumulate-only: each
 * spike of that operand adds the other operand's value `level` times, SOPs = MACs * min(rate) over its on-grid operands with
 * rate = row[1] / row[0] (the mean integer count per element: the quantity in the reference's fr_rate.csv).  Any other op is real and
 * costs its MACs.  energy = e_mac * sum(real MACs) + e_ac * sum(SOPs).  Not counted: BatchNorm (folded at inference), the neuron
 * updates, residual adds, resizes, softmax / sigmoid. */
#define S2F_CENSUS_F32 0
#define S2F_CENSUS_BF16 1
#define S2F_CENSUS_FIELDS 8
int s2f_operand_census(const void* x, int dtype, int64_t n, int D, int64_t* row, void* stream);

/* ---- firing maps: where in the picture a neuron fires (csrc/firingmap.hip, ABI 55) ---------------------------------------------------
 * The figures above are one number per neuron; these are one per neuron AND pixel (spike2former_amd/firingmaps.py: FiringMaps).
 *   s2f_firing_map    x: TB C P contiguous elements read as [TB][C][P], fp32 (S2F_CENSUS_F32) or bf16 (S2F_CENSUS_BF16), aligned to
 *                     the element only (any element offset into a larger buffer; nothing outside x[0 .. TB C P) is read).  Row n of
 *                     the leading dimension belongs to image n % B (t-major: the memory of a [T, B, C, H, W], [T B, C, H, W],
 *                     [T, B, C, N] or [T B, C, N] tensor); TB % B == 0.  stats: int32 [B][4][P], 4-byte aligned.  For image b and
 *                     pixel p, over all (n, c) with n % B == b:
 *                       plane 0 += sum level(x)
 *                       plane 1 += #{x != 0}           (-0.0 counts as zero)
 *                       plane 2  = max(old, max level)
 *                       plane 3 += #{x off the grid}
 *                     level(x) and "off the grid" are the operand census's (below, "operand census"): ONE fp32 multiply of x (a bf16
 *                     element widened exactly) by D converted to fp32, the integer test on that rounded product, the range
 *                     0 .. 65535, a subnormal or non-finite x off the grid, level 0 where off the grid -- one device function for
 *                     both kernels (csrc/census_level.h).
 *                     flags: S2F_FIRING_MAP_ASSIGN -- the four planes are WRITTEN (plane 2 = the max level) instead of added to:
 *                     the first pass needs no clear launch.  Any other bit is S2F_EINVAL.
 *                     All sums are integers and one workgroup owns its pixels: no global atomics, two runs give the same bits,
 *                     nothing outside stats[0 .. 4 B P) is written.  Consecutive lanes read consecutive pixels of one (n, c) plane,
 *                     16 / 8 bytes per lane where P % 4 == 0 and x is aligned to four elements, one element per lane otherwise; for
 *                     a small P the planes of a pixel tile are split over the waves of the workgroup and combined in LDS (the rule:
 *                     the header of csrc/firingmap.hip).
 *                     S2F_EINVAL before any launch: null pointer; TB, B or C < 1; TB % B != 0; P < 0; D < 1; unknown dtype or flags;
 *                     (TB / B) C 65535 >= 2^31 (one pass could leave int32; the HOST keeps passes * that product inside the same
 *                     bound).  S2F_EALIGN: x not aligned to its element, stats not to 4 bytes.  P == 0 launches nothing.  Nothing
 *                     allocates or synchronises.
 *   s2f_firing_draw   ONE launch per tile of a panel: plane, int32 [h][w] (4-byte aligned), is resampled to the picture's H x W,
 *                     looked up in lut, uint8 [256][3] RGB, and blended into image, uint8 [H][W][3].  For output pixel (Y, X), all
 *                     in int64:
 *                       ny = max(0, (2 Y + 1) h - H);  y0 = ny / (2 H);  fy = ((ny - y0 2 H) 256) / (2 H);  y1 = min(y0 + 1, h - 1)
 *                       the same for x                (the half-pixel centres of align_corners=False, weights in 1/256)
 *                       s_ij = max(0, plane[y_i][x_j])
 *                       v    = (256 - fy) ((256 - fx) s00 + fx s01) + fy ((256 - fx) s10 + fx s11)
 *                       idx  = min(255, (255 v + 32768 full) / (65536 full));  col = lut[idx]
 *                       out[ch] = (img[ch] (256 - a8) + col[ch] a8 + 128) >> 8
 *                     This table and this resampling are the package's own specification (not OpenCV's applyColorMap / resize).
 *                     flags: S2F_SEG_DRAW_BGR -- the picture's channels are swapped on read, as in s2f_seg_draw; out is always RGB.
 *                     Row Y of out starts at byte Y out_row_bytes (>= 3 W): a tile is written straight into a panel of several.
 *                     image and out may start at ANY byte (aligned words through LDS, the first and last word of a piece peeled);
 *                     only the H rows of 3 W bytes are written.  S2F_EINVAL before any launch: null pointer; h, w, H or W < 1;
 *                     H W >= 2^31 - 8 or h w >= 2^31; a8 outside 0 .. 256; full outside 1 .. 2^40; unknown flags;
 *                     out_row_bytes < 3 W.  S2F_EALIGN: plane.  Nothing allocates or synchronises. */
#define S2F_FIRING_MAP_ASSIGN 1
int s2f_firing_map(const void* x, int dtype, int TB, int B, int C, int64_t P, int D, int32_t* stats, int flags, void* stream);
int s2f_firing_draw(const uint8_t* image, const int32_t* plane, int h, int w, int64_t full, const uint8_t* lut, int a8, int flags, int H,
                    int W, uint8_t* out, int64_t out_row_bytes, void* stream);

/* ---- general strided fp32 product on the vector ALUs (csrc/bmm.hip, round 6) -----------------------------------------------
 * C[b][m][n] = sum_k A[b][m][k] B[b][k][n], every operand with explicit ELEMENT strides (a transposed or broadcast operand is a
 * stride choice: *_sb = 0 shares one matrix over the batch); reduce_batch != 0: C[m][n] = sum_b sum_k ... (c_sb ignored) -- the
 * weight-gradient form.  Ascending-k (then ascending-b) fp32 multiply-adds: bit-repeatable.  Any M, N, K >= 0, any alignment.
 * Serves the shapes the matrix-core GEMM families do not take (rows that are no whole 16-byte groups, maps below one 128-column
 * tile: the plumbing configuration C1's 4 x 4 .. 16 x 16 maps and 10-query rows) -- replaces torch.bmm (rocBLAS / hipBLASLt), i.e.
 * the reference's nn.Conv2d / nn.Conv1d / nn.Linear and their autograd gradients on such shapes
 * (mmseg/models/backbones/sdtv2.py:112-255; mmdet/models/layers/transformer/mmcv_spike/transformer.py:196-361, 710-784). */
int s2f_bmm_f32(const float* a, int64_t a_sb, int64_t a_sm, int64_t a_sk, const float* b, int64_t b_sb, int64_t b_sk, int64_t b_sn,
                float* c, int64_t c_sb, int64_t c_sm, int64_t c_sn, int B, int M, int N, int K, int reduce_batch, void* stream);

/* ---- reductions and fills of the step outside the neuron / BatchNorm / GEMM kernels (csrc/glue.hip, round 6) --------------------
 * What ran as ATen reduce / fill launches inside the captured step.  Partial sums are STORED and added in index order by a second
 * small kernel: deterministic, no atomics.
 *   s2f_sum_all       out[0] = scale * sum_i x[i]; partials: float[s2f_sum_all_parts(n)] scratch.  The benchmark's headline loss
 *                     (the mean of all_cls_scores / all_mask_preds, mmdet dense_heads/maskformer_head.py:498-586 outputs).
 *   s2f_fill          p[i] = (value_ptr? ? value_ptr[0] : 1) * value -- a device scalar times a host scalar, no host round trip: the
 *                     constant gradient of a mean, written once in the layout its consumer reads.
 *   s2f_channel_sum   out[c] (+)= sum_n sum_l x[n][c][l], x [N][C][L], L % 4 == 0; workspace: float[C * s2f_channel_sum_slices(N, C, L)].
 *                     The level-embedding gradient of the decoder's fused key / value neurons (maskformer_head.py:535-540), the
 *                     mask contraction's row sums.
 *   s2f_sum_lead      out[m] = sum_t x[t][m], x [T][M], M % 4 == 0: the query position embedding's gradient, summed over the T time
 *                     steps (mmcv_spike/transformer.py:626-629). */
int64_t s2f_sum_all_parts(int64_t n);
int s2f_sum_all(const float* x, int64_t n, float scale, float* partials, float* out, void* stream);
int s2f_fill(float* p, int64_t n, const float* value_ptr, float value, void* stream);
int s2f_channel_sum_slices(int N, int C, int L);
int s2f_channel_sum(const float* x, int N, int C, int L, float* workspace, float* out, int accumulate, void* stream);
int s2f_sum_lead(const float* x, int T, int64_t M, float* out, void* stream);
/* The residual glue of a step as generic strided kernels (host: ops/glue_mode.py, a TorchDispatchMode that routes the aten calls autograd
 * and the module code still make -- gradient accumulation where two consumers meet, scalar multiples, sigmoid, layout copies, dtype
 * casts, small sums -- to these instead of ATen's kernels, and reports what it could not route).
 *   s2f_ew          out[..] = f(a[..], b?[..]) over an index space of ndim <= 6 dimensions; size / sa / sb / so: extents and ELEMENT strides
 *                   (0 = broadcast), host arrays of ndim entries.  op: 0 copy | 1 a + alpha b | 2 a b | 3 a / b | 4 sigmoid(a) |
 *                   5 (a (1 - b)) b  [sigmoid_backward(grad = a, output = b)] | 6 a alpha | 7 a alpha + beta | 8 a - alpha b |
 *                   9 a + beta alpha | 10 beta  [a fill: a is not read and may be null]  (ABI 34: ops 6, 7, 9, 10).  The
 *                   products of ops 1, 7 and 8 are fused into the add (one rounding), op 9's is rounded first: ATen's add / sub /
 *                   addcmul with a tensor and with a host scalar as `other`.
 *                   a_bf16: a is bf16 (a dtype cast); flat != 0: every operand contiguous over the same elements (16-byte accesses).
 *   s2f_reduce_sum  out[o] = scale * sum_r a[off(o) + off(r)]: kept index space (nd_o <= 6; may be 0) and reduced index space (1 <= nd_r <= 6),
 *                   the reduced space cut into pieces whose partial sums are stored and added in order (deterministic);
 *                   one wavefront per (output, piece), or one lane per output when consecutive outputs are adjacent in memory. */
int s2f_ew(int op, const void* a, const float* b, float* out, int ndim, const int64_t* size, const int64_t* sa, const int64_t* sb,
           const int64_t* so, float alpha, float beta, int a_bf16, int flat, void* stream);
/* up to eight contiguous fp32 pieces (each a multiple of 4 elements, 16-byte aligned) copied back to back into dst: torch.stack / cat along
 * the leading dimension as one launch; srcs / ns: HOST arrays of `count` entries */
int s2f_copy_segments(float* dst, const void* const* srcs, const int64_t* ns, int count, void* stream);
/* out = ((srcs[0] + srcs[1]) + srcs[2]) + ...  over n fp32 elements, 1 .. 16 addends (HOST array of device pointers), in the order given:
 * the gradient of a tensor with MANY readers (the decoder's query position embedding: twelve neurons per step,
 * mmcv_spike/transformer.py:597-638) in one launch and in the order the autograd engine would have accumulated it. */
int s2f_sum_n(const void* const* srcs, int count, float* out, int64_t n, void* stream);
int64_t s2f_reduce_sum_workspace(int64_t n_out, int64_t n_red);          /* floats of scratch for the call below */
int s2f_reduce_sum(const float* a, float* out, float* workspace, int nd_o, const int64_t* size_o, const int64_t* sa_o, const int64_t* so,
                   int nd_r, const int64_t* size_r, const int64_t* sa_r, float scale, void* stream);

/* ---- masked spike-driven attention (csrc/sdsa_masked.hip, round 6) -------------------------------------------------------------
 * The `attn_mask` branch of (Cross)MultiHeadAttentionBlock.forward (mmcv_spike/transformer.py:259-272, 343-355):
 *     scores = q k^T * scale ; scores.masked_fill(mask, 0) ; out = scores v
 * q, o, go, gq: fp32 [TB][heads * d][Nq]; k, v, gk, gv: fp32 [TB][heads * d][Nk] (channel-major, c = head * d + j, tb = t * B + b);
 * mask: uint8 [B][heads][Nq][Nk], non-zero = masked, shared by the time steps (the reference reshapes attn_mask with t where its comment
 * says bs and therefore only runs for t == b -- where it applies mask[b, h] to every t: the semantics implemented here, for any t).
 * Explicit O(Nq Nk d) evaluation on the vector ALUs (a mask forbids the q (k^T v) association of s2f_sdsa_*); d <= 64.  The head of
 * every shipped config passes no mask (dense_heads/maskformer_head.py:554-564). */
int s2f_sdsa_masked_fwd(const float* q, const float* k, const float* v, const uint8_t* mask, float* o, int TB, int B, int heads, int d,
                        int Nq, int Nk, float scale, void* stream);
int s2f_sdsa_masked_bwd(const float* q, const float* k, const float* v, const uint8_t* mask, const float* go, float* gq, float* gk,
                        float* gv, int TB, int B, int heads, int d, int Nq, int Nk, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* S2F_H */
