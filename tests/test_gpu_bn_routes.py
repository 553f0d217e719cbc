"""Every route of the fused BatchNorm (+ conv bias, + residual, + Q_IFNode) kernels of csrc/bn_lif.hip -- s2f_bn_stats,
s2f_bn_partials_finalize, s2f_bn_act_fwd / _up_fwd / _bwd_ports, s2f_bn2_act_*, s2f_bn_act_*_grouped -- against the fp64 restatement of
tests/bn_ref.py, at the smallest shapes that reach it.  One parametrised row per route, id = route name (the table: tests/bn_rows.py,
shared with tests/test_bn_ref_host.py, which holds the same caps to the reference's own fp32 evaluation).  The kernel is chosen inside
the library, so a row first proves its route from the library's own predicates:

  bn_fused_*       s2f_bn2_fused_ok                                    bn_small_*    s2f_bn_grouped_ok (and not the former)
  bn_mid_*         s2f_bn_single_pass with both of these 0; s2f_bn_mask_words = 320 C confirms it
  row-walking      s2f_bn_bwd_ports_ok(N, C, L, 0, D) and not single-pass; aligned or straddling from L % 256
  flat / ANYL      everything else, which of the two from L % 4

and by a call census over the launching s2f_bn_* symbols, s2f_bn2_*, the grouped pair and s2f_upsample2x_* that the op layer made
exactly the launches it lists (the partials rows call the ABI themselves, with partials the test forms: exact fp64 tile sums rounded
to fp32).  Variants sit on the rows where they are distinct code: every single-pass kernel and both row-walking forms run all five
forward variants and all seven incoming-gradient combinations (reached through autograd by choosing which of u, y, v_out enter the
loss); the flat and ANYL kernels {g_u}, {g_y}, {g_u, g_y, g_v}; a second reader of the spike map on every port-capable form and on one
where the op layer adds; eval mode with the bias gradient on every apply kernel; vth = 0.75 with v_in and g_v on three; D = 4, 6, 16;
want_pre=False on every forward family.

Checks per row
  neuron, exact    y, v_out and the firing counters EQUAL bn_ref.neuron applied in fp32 to h = fl32(v_in + u_kernel), u_kernel the
                   kernel's own u_out (want_pre=False: the u_out of the same call with want_pre=True), on every element: the kernel's
                   decision is a deterministic function of an fp32 value it wrote, no share of elements may differ.
  pre-activation   |u - u64| <= C_U A_u + 1e-30 per entry, A_u = |gamma| rstd (|z| + |b| + |mean|) + kappa |gamma xhat| + |beta| + |r|
                   (bn_ref.abs_sums), C_U = 2e-6 = 32 x 2^-24: the roundings of z + b, the mean, t - mean, two products and two adds
                   are each at most 2^-24 of a term of A_u, the correctly rounded 1 / sqrtf of the variance adds a relative
                   4 kappa 2^-24, and the result is doubled.  kappa = 1 + E[(t - p)^2] / (var + eps) is the conditioning of the
                   variance as the route computes it, p the route's pivot: the first element of the channel's slice (s2f_bn_stats) or
                   of the channel (single-pass kernels); for a producer's partials t - p = z, the un-shifted fp32 tile sums; eval: 1.
                   mean and rstd (stat_out, where the test calls the ABI), the running statistics, the border and
                   num_batches_tracked: the same constant against their own scale (A_mean, A_rstd = kappa rstd, A_rm, A_rv, A_border).
  gradients        the reference takes its in-range bits from the kernel's own h, so an error of the mask layout shows as a gradient
                   error and no flip allowance exists: |g - g64| <= C_G A_g + 1e-30 per entry for gz, g_residual / g_lo, dgamma,
                   dbeta, dbias; A_g the header's expression with every term absolute and every xhat replaced by |xhat| + X,
                   X = rstd (|t| + |mean|) + kappa |xhat|.  C_G = 5.2e-6 = 8 x the worst ratio |err| / A of bn_ref's own expressions
                   evaluated in fp32 on the CPU over the rows (6.5e-7, gz of fused-rest-f32-y; the factor covers FMA contraction and
                   other reduction trees; test_bn_ref_host.py re-measures it and asserts the cap 1e-5).
  bn2              dgamma of the FIRST BatchNorm against its own fp64 value (autograd through the literal composition of two
                   BatchNorms), A = |gamma2| eps2 r2^3 sum |gu xhat|; its dbeta exactly 0.
  exact rows       per channel half the elements m + a, half m - a (m, b, gamma, beta, r, v_in multiples of 1/8, a in {1/2, 1, 2},
                   eps = 0, D = 8): mean, var, rstd in {2, 1, 1/2} are exact in any order, so u, spikes, v_out, counters EQUAL the
                   fp64 values; eval mode: the whole backward too; train mode, BatchNorm only: gu = gu0 + k1 + k2 xhat gives
                   gz = gamma rstd gu0, dbeta = k1 N L, dgamma = k2 N L (bn_rows.exact_draw asserts all of it on its own draw).
  large mean       mean 50, std 1e-2 .. 1, one constant channel, on s2f_bn_stats with two slices, its ANYL form, the row-straddling
                   apply and the partials route, under the same C_U / C_G: the bounds carry kappa, so the shifted routes are held to
                   a kappa of a few units and the partials route to the 2^-24 E[z^2] its tile sums imply (numerics).
                   The gradient sums are quadratic in X (1e4 on these rows), so gz is held loosely there by construction; what binds
                   is u: with the pivot of either statistics kernel set to 0 exactly these rows fail (docs/EXPERIMENTS.md).

Measured on the MI355X, worst |err| / A over the entries, kernel | fp32 CPU (docs/EXPERIMENTS.md has every row):
  fused-bn-u                            (4,64,256)     u 7.7e-08 | 1.7e-07   gz 9.0e-08 | 2.1e-07   dgamma 3.9e-09 | 4.7e-09   dbeta 9.4e-09 | 8.6e-09
  fused-rest-f32-y                      (5,64,256)     u 6.6e-08 | 1.9e-07   gz 1.2e-07 | 6.5e-07   dgamma 2.1e-09 | 2.6e-09   dbeta 8.4e-09 | 1.2e-08
  fused-rest-bf16-uy                    (8,64,2048)    u 7.8e-08 | 1.6e-07   gz 1.2e-07 | 2.0e-07   dgamma 5.6e-10 | 1.1e-09   dbeta 2.1e-09 | 4.2e-09
  fused-v-f32-v                         (4,64,256)     u 7.2e-08 | 1.1e-07   gz 7.5e-08 | 1.0e-07   dgamma 8.1e-10 | 1.3e-09   dbeta 2.1e-09 | 3.2e-09
  fused-v-bf16-yv                       (5,64,256)     u 8.7e-08 | 1.5e-07   gz 5.6e-08 | 1.0e-07   dgamma 6.9e-10 | 1.9e-09   dbeta 2.4e-09 | 4.7e-09
  fused-rest-f32-uv                     (8,64,2048)    u 7.8e-08 | 2.4e-07   gz 6.4e-08 | 1.0e-07   dgamma 4.3e-10 | 4.5e-10   dbeta 9.3e-10 | 1.3e-09
  fused-v-bf16-uyv                      (4,64,256)     u 7.5e-08 | 1.4e-07   gz 6.8e-08 | 1.1e-07   dgamma 1.3e-09 | 1.4e-09   dbeta 4.2e-09 | 4.9e-09
  small-bn-u                            (2,32,4)       u 5.6e-08 | 5.9e-08   gz 4.2e-08 | 8.2e-08   dgamma 2.0e-08 | 3.0e-08   dbeta 6.6e-08 | 6.6e-08
  small-rest-f32-y                      (2,32,100)     u 7.1e-08 | 1.0e-07   gz 1.0e-07 | 9.4e-08   dgamma 4.5e-09 | 5.0e-09   dbeta 9.5e-09 | 3.0e-08
  small-rest-bf16-uy                    (16,32,128)    u 7.4e-08 | 1.7e-07   gz 9.6e-08 | 1.4e-07   dgamma 1.9e-09 | 3.0e-09   dbeta 6.0e-09 | 6.5e-09
  small-v-f32-v                         (2,32,4)       u 4.9e-08 | 7.4e-08   gz 1.8e-08 | 2.6e-08   dgamma 1.7e-08 | 1.9e-08   dbeta 5.1e-08 | 5.1e-08
  small-v-bf16-yv                       (2,32,100)     u 6.4e-08 | 2.0e-07   gz 3.6e-08 | 9.9e-08   dgamma 2.3e-09 | 2.8e-09   dbeta 4.8e-09 | 4.5e-09
  small-rest-f32-uv                     (16,32,128)    u 7.5e-08 | 1.3e-07   gz 6.2e-08 | 7.1e-08   dgamma 7.5e-10 | 6.7e-10   dbeta 4.2e-09 | 2.7e-09
  small-v-bf16-uyv                      (2,32,4)       u 6.1e-08 | 6.9e-08   gz 2.0e-08 | 2.0e-08   dgamma 7.8e-09 | 1.3e-08   dbeta 2.9e-08 | 2.9e-08
  mid-bn-u                              (1,32,2052)    u 8.7e-08 | 1.5e-07   gz 8.1e-08 | 2.1e-07   dgamma 1.4e-09 | 2.9e-09   dbeta 4.5e-09 | 8.6e-09
  mid-rest-f32-y                        (4,32,4200)    u 7.6e-08 | 1.5e-07   gz 1.2e-07 | 2.7e-07   dgamma 5.2e-10 | 9.1e-10   dbeta 2.6e-09 | 2.7e-09
  mid-rest-bf16-uy                      (4,32,5116)    u 7.8e-08 | 2.3e-07   gz 1.1e-07 | 1.6e-07   dgamma 6.1e-10 | 7.3e-10   dbeta 1.3e-09 | 1.7e-09
  mid-v-f32-v                           (1,32,2052)    u 7.8e-08 | 1.3e-07   gz 5.8e-08 | 9.9e-08   dgamma 7.0e-10 | 1.1e-09   dbeta 1.5e-09 | 2.2e-09
  mid-v-bf16-yv                         (4,32,4200)    u 8.2e-08 | 2.2e-07   gz 9.3e-08 | 1.2e-07   dgamma 2.8e-10 | 7.2e-10   dbeta 5.7e-10 | 1.4e-09
  mid-rest-f32-uv                       (4,32,5116)    u 7.8e-08 | 2.1e-07   gz 6.2e-08 | 9.4e-08   dgamma 2.8e-10 | 3.2e-10   dbeta 6.4e-10 | 1.9e-09
  mid-v-bf16-uyv                        (1,32,2052)    u 7.8e-08 | 1.3e-07   gz 6.8e-08 | 1.2e-07   dgamma 7.3e-10 | 1.4e-09   dbeta 2.2e-09 | 4.3e-09
  rows-aligned-bn-u                     (2,3,256)      u 6.3e-08 | 7.3e-08   gz 4.4e-08 | 8.6e-08   dgamma 8.2e-10 | 1.7e-09   dbeta 5.0e-09 | 1.9e-09
  rows-aligned-rest-f32-y               (1,2,4096)     u 4.3e-08 | 5.3e-08   gz 6.3e-08 | 6.3e-08   dgamma 5.1e-10 | 9.5e-10   dbeta 5.0e-10 | 2.7e-09
  rows-aligned-rest-bf16-uy             (2,3,256)      u 6.3e-08 | 5.6e-08   gz 5.2e-08 | 6.0e-08   dgamma 4.8e-10 | 2.4e-09   dbeta 3.3e-09 | 2.5e-09
  rows-aligned-v-f32-v                  (1,2,4096)     u 5.0e-08 | 7.3e-08   gz 1.3e-08 | 5.4e-08   dgamma 8.0e-11 | 1.4e-10   dbeta 3.5e-10 | 4.1e-10
  rows-aligned-v-bf16-yv                (2,3,256)      u 5.7e-08 | 7.9e-08   gz 2.5e-08 | 4.9e-08   dgamma 1.1e-09 | 1.5e-09   dbeta 2.0e-09 | 1.0e-09
  rows-aligned-rest-f32-uv              (1,2,4096)     u 6.5e-08 | 6.5e-08   gz 3.2e-08 | 3.2e-08   dgamma 6.9e-11 | 2.6e-10   dbeta 1.1e-09 | 5.3e-10
  rows-aligned-v-bf16-uyv               (2,3,256)      u 5.9e-08 | 7.4e-08   gz 4.7e-08 | 4.7e-08   dgamma 9.1e-10 | 9.1e-10   dbeta 1.6e-09 | 2.4e-09
  rows-straddling-bn-u                  (3,5,260)      u 5.5e-08 | 8.4e-08   gz 7.9e-08 | 6.1e-08   dgamma 9.9e-10 | 1.1e-09   dbeta 3.8e-09 | 9.6e-09
  rows-straddling-rest-f32-y            (1,2,4100)     u 6.3e-08 | 6.3e-08   gz 8.6e-08 | 8.6e-08   dgamma 8.6e-10 | 1.4e-09   dbeta 1.9e-09 | 6.8e-09
  rows-straddling-rest-bf16-uy          (3,5,260)      u 5.6e-08 | 7.2e-08   gz 5.8e-08 | 6.0e-08   dgamma 1.9e-09 | 2.7e-09   dbeta 3.4e-09 | 2.7e-09
  rows-straddling-v-f32-v               (1,2,4100)     u 5.6e-08 | 6.2e-08   gz 2.7e-08 | 3.9e-08   dgamma 2.5e-10 | 2.5e-10   dbeta 3.4e-10 | 8.6e-10
  rows-straddling-v-bf16-yv             (3,5,260)      u 6.4e-08 | 6.9e-08   gz 3.5e-08 | 4.4e-08   dgamma 1.0e-09 | 1.1e-09   dbeta 1.9e-09 | 1.3e-09
  rows-straddling-rest-f32-uv           (1,2,4100)     u 6.9e-08 | 9.2e-08   gz 3.4e-08 | 4.4e-08   dgamma 1.6e-10 | 2.8e-10   dbeta 4.8e-10 | 1.9e-09
  rows-straddling-v-bf16-uyv            (3,5,260)      u 5.9e-08 | 6.5e-08   gz 3.8e-08 | 8.0e-08   dgamma 1.3e-09 | 8.7e-10   dbeta 3.0e-09 | 2.5e-09
  flat-u                                (2,7,36)       u 4.5e-08 | 6.4e-08   gz 4.1e-08 | 4.1e-08   dgamma 4.8e-09 | 4.9e-09   dbeta 2.1e-08 | 2.0e-08
  flat-y                                (2,7,36)       u 5.5e-08 | 6.9e-08   gz 4.4e-08 | 6.0e-08   dgamma 5.5e-09 | 1.0e-08   dbeta 1.7e-08 | 2.5e-08
  flat-uyv                              (2,7,36)       u 4.6e-08 | 8.6e-08   gz 1.9e-08 | 4.0e-08   dgamma 1.4e-09 | 2.6e-09   dbeta 7.8e-09 | 7.8e-09
  anyl-uyv                              (3,5,7)        u 4.0e-08 | 6.8e-08   gz 1.2e-08 | 2.9e-08   dgamma 3.2e-09 | 1.1e-08   dbeta 2.2e-09 | 1.3e-08
  anyl-one-column-y                     (2,3,1)        u 2.3e-08 | 2.3e-08   gz 4.6e-09 | 5.3e-09   dgamma 1.3e-08 | 1.4e-08   dbeta 0.0e+00 | 0.0e+00
  anyl-slices-u                         (1,2,4099)     u 6.6e-08 | 6.6e-08   gz 9.5e-08 | 9.5e-08   dgamma 6.1e-10 | 4.1e-10   dbeta 2.2e-09 | 3.3e-09
  d6-off-the-rows-uyv                   (2,3,512)      u 4.8e-08 | 6.2e-08   gz 2.9e-08 | 2.9e-08   dgamma 2.8e-10 | 6.6e-10   dbeta 1.3e-09 | 1.9e-09
  up-image-rows                         (1,2,16,16)    u 7.2e-08 | 6.9e-08   gz 4.1e-08 | 4.1e-08   dgamma 1.4e-09 | 1.3e-09   dbeta 1.8e-09 | 4.3e-09
  up-wide-row                           (1,1,2,256)    u 5.6e-08 | 5.6e-08   gz 3.0e-08 | 3.0e-08   dgamma 7.4e-11 | 9.7e-10   dbeta 7.3e-10 | 7.3e-10
  bn2-u                                 (4,64,256)     u 5.5e-08 | 1.1e-07   gz 7.9e-08 | 1.1e-07   dgamma 2.8e-08 | 6.1e-08   dbeta 0.0e+00 | 0.0e+00   dgamma2 1.6e-09 | 1.9e-09
  bn2-bf16-uy-res                       (8,64,1024)    u 7.2e-08 | 2.0e-07   gz 9.5e-08 | 2.1e-07   dgamma 1.1e-08 | 1.2e-08   dbeta 0.0e+00 | 0.0e+00   dgamma2 6.9e-10 | 8.4e-10
  bn2-v-uyv                             (4,64,256)     u 5.6e-08 | 1.6e-07   gz 5.0e-08 | 5.4e-08   dgamma 1.5e-08 | 2.0e-08   dbeta 0.0e+00 | 0.0e+00   dgamma2 9.2e-10 | 1.0e-09
  grouped-2-bf16-uy                     (2,32,100)     u 6.7e-08 | 9.3e-08   gz 7.9e-08 | 9.1e-08   dgamma 4.0e-09 | 9.3e-09   dbeta 1.1e-08 | 1.7e-08
  grouped-4-u                           (2,32,100)     u 6.9e-08 | 1.5e-07   gz 8.0e-08 | 1.2e-07   dgamma 5.6e-09 | 1.0e-08   dbeta 1.3e-08 | 1.8e-08
  grouped-2-f32-y                       (2,32,100)     u 7.1e-08 | 2.1e-07   gz 1.1e-07 | 3.3e-07   dgamma 4.6e-09 | 1.3e-08   dbeta 2.0e-08 | 2.8e-08
  partials-per-wave                     (1,6,1040)     u 6.0e-08 | 7.2e-08   gz 6.7e-08 | 6.3e-08   dgamma 1.3e-09 | 1.4e-09   dbeta 3.2e-09 | 8.4e-09
  partials-per-channel                  (1,6,4112)     u 7.0e-08 | 6.9e-08   gz 4.8e-08 | 5.2e-08   dgamma 5.6e-10 | 5.6e-10   dbeta 6.3e-10 | 1.2e-09
  second-reader-fused                   (5,64,256)     u 7.3e-08 | 1.2e-07   gz 8.0e-08 | 1.5e-07   dgamma 1.3e-09 | 4.3e-09   dbeta 6.6e-09 | 9.1e-09
  second-reader-rows-aligned            (2,3,256)      u 4.9e-08 | 6.9e-08   gz 3.1e-08 | 3.1e-08   dgamma 4.2e-10 | 4.2e-10   dbeta 2.3e-09 | 2.3e-09
  second-reader-rows-straddling         (3,5,260)      u 6.3e-08 | 6.3e-08   gz 7.2e-08 | 7.2e-08   dgamma 1.9e-09 | 1.6e-09   dbeta 4.4e-09 | 6.8e-09
  second-reader-added-by-the-op-layer   (2,32,100)     u 6.8e-08 | 1.1e-07   gz 9.6e-08 | 1.0e-07   dgamma 2.8e-09 | 6.7e-09   dbeta 8.0e-09 | 1.5e-08
  eval-flat                             (2,7,36)       u 9.0e-08 | 9.1e-08   gz 1.6e-07 | 1.9e-07   dgamma 5.1e-09 | 1.0e-08   dbeta 5.1e-09 | 3.4e-08
  eval-anyl                             (3,5,7)        u 5.6e-08 | 5.6e-08   gz 9.6e-08 | 9.6e-08   dgamma 3.9e-09 | 5.7e-09   dbeta 7.6e-09 | 2.3e-08
  eval-rows-aligned                     (2,3,256)      u 1.0e-07 | 1.1e-07   gz 1.1e-07 | 1.1e-07   dgamma 2.1e-09 | 1.3e-09   dbeta 2.2e-09 | 3.5e-09
  eval-rows-straddling                  (3,5,260)      u 8.9e-08 | 8.9e-08   gz 1.2e-07 | 1.2e-07   dgamma 1.8e-09 | 2.6e-09   dbeta 4.1e-09 | 5.4e-09
  vth-fused                             (4,64,256)     u 7.0e-08 | 2.2e-07   gz 6.3e-08 | 9.3e-08   dgamma 1.6e-09 | 2.3e-09   dbeta 4.3e-09 | 4.6e-09
  vth-rows-aligned                      (2,3,256)      u 5.7e-08 | 5.5e-08   gz 4.1e-08 | 4.1e-08   dgamma 4.9e-10 | 1.2e-09   dbeta 1.2e-09 | 4.0e-09
  vth-flat                              (2,7,36)       u 6.3e-08 | 3.5e-07   gz 1.7e-08 | 3.9e-08   dgamma 1.6e-09 | 3.5e-09   dbeta 4.1e-09 | 4.1e-09
  d4-small                              (2,32,100)     u 6.3e-08 | 3.3e-07   gz 5.2e-08 | 1.6e-07   dgamma 4.4e-09 | 1.1e-08   dbeta 9.3e-09 | 1.9e-08
  d16-mid                               (1,32,2052)    u 6.5e-08 | 2.4e-07   gz 5.5e-08 | 1.3e-07   dgamma 6.1e-10 | 1.5e-09   dbeta 3.3e-09 | 3.1e-09
  d4-rows-aligned                       (2,3,256)      u 5.2e-08 | 6.1e-08   gz 2.0e-08 | 2.0e-08   dgamma 6.3e-10 | 4.3e-10   dbeta 8.5e-10 | 3.1e-09
  d16-rows-straddling                   (3,5,260)      u 5.4e-08 | 5.8e-08   gz 6.4e-08 | 5.2e-08   dgamma 1.6e-09 | 1.9e-09   dbeta 4.5e-09 | 1.1e-08
  d16-fused                             (4,64,256)     u 7.3e-08 | 1.9e-07   gz 9.1e-08 | 1.4e-07   dgamma 2.6e-09 | 5.2e-09   dbeta 1.1e-08 | 8.8e-09
  no-pre-fused                          (4,64,256)     u 6.6e-08 | 2.4e-07   gz 1.1e-07 | 2.9e-07   dgamma 2.6e-09 | 6.5e-09   dbeta 6.1e-09 | 1.0e-08
  no-pre-small                          (2,32,100)     u 6.3e-08 | 6.7e-08   gz 7.8e-08 | 1.0e-07   dgamma 4.0e-09 | 8.6e-09   dbeta 1.1e-08 | 3.1e-08
  no-pre-mid                            (1,32,2052)    u 7.3e-08 | 1.7e-07   gz 1.1e-07 | 2.0e-07   dgamma 1.9e-09 | 3.3e-09   dbeta 5.6e-09 | 6.7e-09
  no-pre-rows                           (3,5,260)      u 5.8e-08 | 1.0e-07   gz 3.7e-08 | 3.7e-08   dgamma 1.8e-10 | 9.3e-10   dbeta 2.4e-09 | 1.2e-09
  no-pre-flat                           (2,7,36)       u 6.5e-08 | 1.3e-07   gz 8.7e-08 | 9.1e-08   dgamma 5.4e-09 | 1.7e-08   dbeta 1.5e-08 | 4.7e-08
  large-mean-stats-two-slices           (1,2,4096)     u 7.6e-09 | 7.6e-09   gz 1.4e-13 | 1.4e-13   dgamma 1.2e-13 | 1.2e-13   dbeta 1.9e-10 | 3.3e-09
  large-mean-stats-any                  (1,2,4099)     u 1.4e-08 | 1.4e-08   gz 1.0e-13 | 1.0e-13   dgamma 2.9e-10 | 2.9e-10   dbeta 1.1e-09 | 2.7e-09
  large-mean-rows-straddling            (3,5,260)      u 1.4e-08 | 1.5e-08   gz 5.8e-12 | 5.8e-12   dgamma 6.3e-10 | 6.3e-10   dbeta 2.5e-09 | 5.3e-09
  large-mean-partials                   (1,6,1040)     u 1.4e-08 | 1.4e-08   gz 6.5e-12 | 6.5e-12   dgamma 2.3e-10 | 2.3e-10   dbeta 2.6e-09 | 6.4e-09
  i.e. every row is a factor of 20 or more inside C_U (worst 1.0e-7: u of eval-rows-aligned) and of 32 or more inside C_G (worst
  1.6e-7: gz of eval-flat); the kernels reduce in fp64 and are at or below the fp32 CPU evaluation almost everywhere.  Ten arithmetic
  mutants of csrc/bn_lif.hip (no address moves; the record is in docs/EXPERIMENTS.md) are each caught, and only by rows on the kernel
  they change; the row-walking kernels multiply by 1 / D where the others divide, hence a D other than 8 on every kernel family.
  An output that is not finite counts as an infinite ratio (bn_rows._ratio): a NaN fails every bound.

Not repeated here: the bit-for-bit pins of the existing tests -- grouped == single calls (test_gpu_decoder_siblings.py), the
up-sampling residual == two launches (test_gpu_fpn_levels.py), the bf16-plane gradient == fp32 gz, the second reader == the engine's
sum, partials ~ statistics pass (test_gpu_kernels.py, test_gpu_round6.py): they stay as they are and now rest on routes this file holds
to fp64.  s2f_bn_act_bwd_split is reached only through them."""
import copy
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_ref  # noqa: E402
import bn_rows  # noqa: E402
from bn_rows import C_G, C_U  # noqa: E402

pytestmark = pytest.mark.gpu

# every launch ops/bn.py can make for a BatchNorm
CENSUS = ("bn_stats", "bn_partials_finalize", "bn_act_fwd", "bn_act_up_fwd", "bn_act_bwd", "bn_act_bwd_ports", "bn_act_bwd_split",
          "bn2_act_fwd", "bn2_act_bwd", "bn_act_fwd_grouped", "bn_act_bwd_grouped", "upsample2x_fwd", "upsample2x_bwd",
          "upsample2x_bwd_add")


_PORT = [None]


@pytest.fixture(scope="module")
def ops():
    from spike2former_amd import ops
    return ops


@pytest.fixture
def census(ops, monkeypatch):
    """{symbol without its s2f_ prefix: number of calls} since the fixture was set up; _PORT[0]: whether the last
    s2f_bn_act_bwd_ports call was handed a second spike gradient (its g_y2 argument)"""
    calls = {}

    def wrap(name, fn):
        def counted(*a):
            calls[name] = calls.get(name, 0) + 1
            if name == "bn_act_bwd_ports":
                _PORT[0] = bool(a[6])
            return fn(*a)
        return counted
    for name in CENSUS:
        monkeypatch.setattr(ops.lib, "s2f_" + name, wrap(name, getattr(ops.lib, "s2f_" + name)))
    return calls


# -------------------------------------------------------------------------------------------------------------- routes, from the shape
def prove_route(ops, r):
    lib = ops.lib
    N, C = r.shape[:2]
    L = 1
    for s in r.shape[2:]:
        L *= s
    fused, small, single = lib.s2f_bn2_fused_ok(N, C, L), lib.s2f_bn_grouped_ok(N, C, L), lib.s2f_bn_single_pass(N, C, L)
    ports = lib.s2f_bn_bwd_ports_ok(N, C, L, 0, r.D)
    own_stats = r.training and single          # eval mode never takes the single-pass kernels
    route = "rows-straddling" if r.route == "partials" else r.route
    if route in ("fused", "bn2"):
        assert fused == 1 and r.training
        assert lib.s2f_bn_bwd_ports_ok(N, C, L, 1, r.D) == 1
    elif route in ("small", "grouped"):
        assert small == 1 and fused == 0 and r.training and lib.s2f_bn_mask_words(N, C, L) == 32 * C
        assert lib.s2f_bn_bwd_ports_ok(N, C, L, 1, r.D) == 0
    elif route == "mid":
        assert single == 1 and fused == 0 and small == 0 and r.training and lib.s2f_bn_mask_words(N, C, L) == 320 * C
        assert lib.s2f_bn_bwd_ports_ok(N, C, L, 1, r.D) == 0
    elif route in ("rows-aligned", "rows-straddling", "up"):
        assert ports == 1 and not own_stats and (L % 256 == 0) == (route != "rows-straddling")
        assert lib.s2f_bn_bwd_ports_ok(N, C, L, int(r.training), r.D) == 1
        if route == "up":
            assert lib.s2f_bn_up_ok(N, C, r.shape[2], r.shape[3], 1, r.D) == 1
    else:
        assert route in ("flat", "anyl") and ports == 0 and not own_stats and (L % 4 == 0) == (route == "flat")
    if r.kind == "partials":
        P = N * L // r.tile
        assert (P <= 256) == (r.id != "partials-per-channel")          # per wave / per channel: s2f_bn_partials_finalize's two forms
    if not single and r.training and r.kind == "act":
        S = bn_rows.stats_slice(C, L)[0]
        assert (S == 2) == (L >= 4096)          # the rows with two statistics slices
    return N, C, L


def expected_launches(r):
    if r.kind == "bn2":
        return {"bn2_act_fwd": 1, "bn2_act_bwd": 1}
    if r.kind == "grouped":
        return {"bn_act_fwd_grouped": 1, "bn_act_bwd_grouped": 1}
    e = {"bn_act_up_fwd" if r.route == "up" else "bn_act_fwd": 1, "bn_act_bwd_ports": 1}
    if r.training and not bn_rows.single_pass(r.route):
        e["bn_stats"] = 1
    if r.route == "up":
        e["upsample2x_bwd_add"] = 1
    return e


# -------------------------------------------------------------------------------------------------------------- running a row
def _leaf(t, grad=True):
    return None if t is None else t.cuda().requires_grad_(grad)


def _spikes_dtype(r, numel):
    return torch.bfloat16 if (r.bf16 and numel % 4 == 0 and r.D & (r.D - 1) == 0) else torch.float32


def run_op(ops, r, d, want_pre, backward=True):
    """the row through the op layer (bn_act / bn2_act / bn_act_siblings) and autograd -> forward outputs, gradients (CPU tensors; grouped:
    group-outermost)"""
    ds = d.groups or [d]
    cat = lambda k: None if getattr(d, k) is None else torch.cat([getattr(x, k) for x in ds])
    z = _leaf(torch.stack([x.z for x in ds]) if d.groups else d.z)
    bias, gamma, beta = _leaf(cat("bias")), _leaf(cat("gamma")), _leaf(cat("beta"))
    rm, rv = cat("rm").cuda(), cat("rv").cuda()
    res, lo, v_in = _leaf(d.residual), _leaf(d.residual_lo), _leaf(d.v_in, False)
    nbt = torch.zeros((), dtype=torch.int64, device="cuda") if r.training else None
    stats = ops.new_stats("cuda") if (r.lif and r.kind != "grouped") else None
    keep_v = r.lif and (r.v_in or "v" in r.grads)
    out = SimpleNamespace(border=None, rm2=None, rv2=None, nbt=None, nbt2=None)
    if r.kind == "bn2":
        b2 = {k: v.cuda() if torch.is_tensor(v) else v for k, v in d.bn2.items()}
        g2, be2 = b2["gamma"].requires_grad_(True), b2["beta"].requires_grad_(True)
        nbt2 = torch.zeros((), dtype=torch.int64, device="cuda")
        bn_a = SimpleNamespace(weight=gamma, bias=beta, running_mean=rm, running_var=rv, num_batches_tracked=nbt, momentum=r.momentum, eps=r.eps)
        bn_b = SimpleNamespace(weight=g2, bias=be2, running_mean=b2["rm"], running_var=b2["rv"], num_batches_tracked=nbt2,
                               momentum=b2["momentum"], eps=b2["eps"])
        u, y, v = ops.bn2_act(z, bn_a, bn_b, residual=res, lif=r.lif, want_pre=want_pre, v_in=v_in, keep_v=keep_v, D=r.D, vth=r.vth, stats=stats)
        out.rm2, out.rv2, out.nbt2 = b2["rm"].cpu(), b2["rv"].cpu(), int(nbt2)
    elif r.kind == "grouped":
        u, y = ops.bn_act_siblings(z, bias, gamma, beta, rm, rv, r.momentum, r.eps, lif=r.lif, want_pre=want_pre, D=r.D, vth=r.vth)
        v = None
    else:
        got = ops.bn_act(z, bias, gamma, beta, rm, rv, nbt, r.training, r.momentum, r.eps, residual=res, lif=r.lif, want_pre=want_pre,
                         v_in=v_in, keep_v=keep_v, D=r.D, vth=r.vth, stats=stats, want_border=True, residual_lo=lo)
        u, y, v, out.border = got[0], got[1], got[2], got[3].cpu()
    assert (u is not None) == want_pre and (y is not None) == r.lif and (v is not None) == bool(keep_v)
    if r.lif:
        assert y.data.dtype == _spikes_dtype(r, ds[0].z.numel())
    out.u = None if u is None else u.detach().cpu()
    out.y = None if y is None else y.data.detach().float().cpu()
    out.v = None if v is None else v.detach().cpu()
    out.rm, out.rv, out.nbt = rm.cpu(), rv.cpu(), None if nbt is None else int(nbt)
    out.counters = None if stats is None else ops.read_stats(stats).tolist()
    grads = {}
    if backward:
        w = {k: (torch.stack([x.w[k] for x in ds]) if d.groups else d.w[k]).cuda() for k in r.grads}
        loss = 0
        if "u" in r.grads:
            loss = loss + (u * w["u"]).sum()
        if "y" in r.grads:
            loss = loss + (y.float() * w["y"]).sum()
        if "2" in r.grads:
            # the second reader arrives on the neuron's spare handle (else second() is the map itself and the engine adds)
            assert y.tok2 is not None and y.second().tok is y.tok2 and y.tok2 is not y.tok
            loss = loss + (y.second().float() * w["2"]).sum()
        if "v" in r.grads:
            loss = loss + (v * w["v"]).sum()
        loss.backward()
        cpu = lambda t: None if (t is None or t.grad is None) else t.grad.cpu()
        grads = dict(gz=cpu(z), dgamma=cpu(gamma), dbeta=cpu(beta), g_residual=cpu(res if lo is None else lo), dbias=cpu(bias))
        if r.kind == "bn2":
            grads.update(dgamma2=cpu(g2), dbeta2=cpu(be2))
        if r.training:
            assert grads["dbias"] is None or float(grads["dbias"].abs().max()) == 0.0          # train mode removes the bias exactly
            grads["dbias"] = None
    return out, grads


def run_abi(ops, r, d):
    """a partials row on the C ABI: s2f_bn_partials_finalize on partials the test forms, s2f_bn_act_fwd with those sums, s2f_bn_act_bwd"""
    lib, P_, S_ = ops.lib, ops._ptr, ops._stream
    N, C, L = r.shape
    dev = "cuda"
    part = bn_ref.tile_partials(d.z, r.tile).cuda()
    z, bias, gamma, beta, v_in = (None if t is None else t.cuda() for t in (d.z, d.bias, d.gamma, d.beta, d.v_in))
    rm, rv, nbt = d.rm.cuda(), d.rv.cuda(), torch.zeros((), dtype=torch.int64, device=dev)
    ws = torch.full((2 * C,), float("nan"), dtype=torch.float64, device=dev)          # (plain stores: need not be zeroed)
    ops.check(lib.s2f_bn_partials_finalize(P_(part), part.shape[1], P_(bias), P_(ws), N, C, L, S_()), "s2f_bn_partials_finalize")
    want = bn_ref.partial_sums(part, d.bias, N * L)
    assert torch.allclose(ws.cpu().view(C, 2), want, rtol=1e-14, atol=0), "the sums of the partials, in fp64"
    stat = torch.empty(3 * C, device=dev)
    u = torch.empty_like(z)
    y = torch.empty_like(z) if r.lif else None
    v = torch.empty_like(z) if r.lif else None
    mask = torch.empty(int(lib.s2f_bn_mask_words(N, C, L)), dtype=torch.int64, device=dev) if r.lif else None
    stats = ops.new_stats(dev) if r.lif else None
    ops.check(lib.s2f_bn_act_fwd(P_(z), P_(bias), P_(ws), P_(stat), P_(rm), P_(rv), P_(nbt), P_(gamma), P_(beta), 0, P_(u), P_(v_in),
                                 P_(y), P_(v), P_(mask), P_(stats), N, C, L, r.momentum, r.eps, 1, r.vth, r.D, 0, S_()), "s2f_bn_act_fwd")
    g = {k: (d.w[k].cuda() if k in r.grads else None) for k in "uyv"}
    gz, dgamma, dbeta = torch.empty_like(z), torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws2 = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    ops.check(lib.s2f_bn_act_bwd(P_(z), P_(bias), P_(stat), P_(gamma), P_(g["u"]), P_(g["y"]), P_(g["v"]), P_(mask), P_(ws2), P_(gz), 0,
                                 P_(dgamma), P_(dbeta), N, C, L, 1, r.vth, r.D, S_()), "s2f_bn_act_bwd")
    cpu = lambda t: None if t is None else t.cpu()
    out = SimpleNamespace(u=cpu(u), y=cpu(y), v=cpu(v), rm=cpu(rm), rv=cpu(rv), nbt=int(nbt), border=stat[2 * C:].cpu(), mean=stat[:C].cpu(),
                          rstd=stat[C:2 * C].cpu(), counters=None if stats is None else ops.read_stats(stats).tolist(), rm2=None, rv2=None,
                          nbt2=None)
    return out, dict(gz=cpu(gz), dgamma=cpu(dgamma), dbeta=cpu(dbeta))


def check_neuron(r, d, out, u_kernel):
    """y, v_out, counters == bn_ref.neuron in fp32 on h = fl32(v_in + u_kernel), bit for bit -> the in-range map of that h"""
    h = u_kernel if d.v_in is None else d.v_in + u_kernel
    assert h.dtype == torch.float32
    y, v, s, bits = bn_ref.neuron(h, r.D, r.vth)
    assert torch.equal(out.y, y), f"{int((out.y != y).sum())} spikes differ"
    if out.v is not None:
        assert torch.equal(out.v, v), f"{int((out.v != v).sum())} membranes differ"
    if out.counters is not None:
        assert out.counters == [int(s.sum()), int((s != 0).sum())]
    return bits


def split_groups(r, d, t, per_channel):
    """group g's slice of a group-outermost result"""
    if t is None or d.groups is None:
        return [t] * len(d.groups or [d])
    if per_channel:
        return list(t.view(len(d.groups), -1))
    return list(t)


@pytest.mark.parametrize("r", bn_rows.ROWS, ids=[r.id for r in bn_rows.ROWS])
def test_route_vs_fp64(ops, spike_mode, census, r):
    N, C, L = prove_route(ops, r)
    d = bn_rows.draw(r)
    spike_mode(r.bf16)
    if r.kind == "partials":
        out, grads = run_abi(ops, r, d)
        u_kernel = out.u
    else:
        out, grads = run_op(ops, r, d, r.want_pre)
        assert dict(census) == expected_launches(r), (dict(census), expected_launches(r))
        if r.kind == "act":
            # the second reader's gradient reaches the kernel's own port where the form has one; elsewhere the op layer adds
            has_port = bool(ops.lib.s2f_bn_bwd_ports_ok(N, C, L, int(r.training), r.D))
            assert _PORT[0] == ("2" in r.grads and has_port), (_PORT[0], has_port)
            assert has_port == (r.id != "second-reader-added-by-the-op-layer") or "2" not in r.grads
        # want_pre=False: the u_out of the same call with want_pre=True (running statistics from the same start)
        u_kernel = out.u if r.want_pre else run_op(ops, r, d, True, backward=False)[0].u
        if not r.want_pre:
            assert out.u is None
    # num_batches_tracked: + 1 per train-mode call (the siblings' is the caller's to count)
    assert out.nbt == (None if not r.training else 0 if r.kind == "grouped" else 1) and out.nbt2 == (1 if r.kind == "bn2" else None)
    groups = d.groups or [d]
    fwd_k, bwd_k, fwd_c, bwd_c = {}, {}, {}, {}
    worst = bn_rows.worse          # (a NaN ratio counts as inf)
    sl = lambda t, pc: split_groups(r, d, t, pc)
    for g, dg in enumerate(groups):
        pick = lambda t, pc=False: sl(t, pc)[g]
        og = SimpleNamespace(u=pick(u_kernel), y=pick(out.y), v=pick(out.v), counters=out.counters)
        bits = check_neuron(r, dg, og, og.u) if r.lif else None
        got = dict(u=og.u, running_mean=pick(out.rm, True), running_var=pick(out.rv, True), border=pick(out.border, True))
        if r.kind == "partials":
            got.update(mean=out.mean, rstd=out.rstd)
        if r.kind == "bn2":
            got.update(running_mean2=out.rm2, running_var2=out.rv2)
        worst(fwd_k, bn_rows.forward_ratios(r, dg, got))
        per_channel = ("dgamma", "dbeta", "dbias", "dgamma2", "dbeta2")
        worst(bwd_k, bn_rows.backward_ratios(r, dg, {k: pick(v, k in per_channel) for k, v in grads.items()}, bits))
        c_fwd, c_bwd, c_bits = bn_rows.cpu32(r, dg)
        worst(fwd_c, bn_rows.forward_ratios(r, dg, c_fwd))
        worst(bwd_c, bn_rows.backward_ratios(r, dg, c_bwd, c_bits))
    line = "  ".join(f"{k} {v:.1e} | {({**fwd_c, **bwd_c}).get(k, float('nan')):.1e}" for k, v in {**fwd_k, **bwd_k}.items())
    print(f"\n{r.id:38s} {str(r.shape):18s} {line}")
    assert bn_rows.within(fwd_k, C_U), {k: v for k, v in fwd_k.items() if not v <= C_U}
    assert bn_rows.within(bwd_k, C_G), {k: v for k, v in bwd_k.items() if not v <= C_G}
    expect = {"gz", "dgamma", "dbeta"} | ({"g_residual"} if r.res else set()) | ({"dbias"} if (r.bias and not r.training) else set()) | \
        ({"dgamma2", "dbeta2"} if r.kind == "bn2" else set())
    assert set(bwd_k) == expect, (sorted(bwd_k), sorted(expect))


@pytest.mark.parametrize("route,shape", bn_rows.EXACT, ids=[e[0] for e in bn_rows.EXACT])
def test_exact_row(ops, spike_mode, census, route, shape):
    N, C, L = shape
    d = bn_rows.exact_draw(route, shape)
    eq = lambda a, b: torch.equal(a.double(), b.double())
    spike_mode(True)
    # train mode with bias, residual, membrane and neuron: u, spikes, v_out, counters, running_mean EQUAL the fp64 values
    r = bn_rows.row("exact-" + route, route, shape, lif=True, v_in=True, bf16=True, grads="", bias=True, res="res", eps=0.0, momentum=0.25)
    prove_route(ops, r)
    out, _ = run_op(ops, r, d, True, backward=False)
    fw = bn_ref.forward(*bn_rows.fwd_args(r, d), residual=d.residual)
    y, v, s, _bits = bn_ref.neuron(d.v_in.double() + fw.u, 8, 1.0)
    assert eq(out.u, fw.u) and eq(out.y, y) and eq(out.v, v) and out.counters == [int(s.sum()), int((s != 0).sum())]
    assert eq(out.rm, fw.running_mean) and out.nbt == 1
    # train mode, BatchNorm only: gu = gu0 + k1 + k2 xhat  ->  gz = gamma rstd gu0, dbeta = k1 N L, dgamma = k2 N L
    r = bn_rows.row("exact-" + route, route, shape, grads="u", bias=True, eps=0.0, momentum=0.25)
    dt = copy.copy(d)
    dt.residual, dt.v_in, dt.w = None, None, {"u": d.gu_train}
    census.clear()
    out, grads = run_op(ops, r, dt, True)
    assert dict(census) == expected_launches(r)
    assert eq(grads["gz"], (d.gamma.double() * fw.rstd).view(1, C, 1) * d.gu0.double())
    assert eq(grads["dbeta"], d.k1 * N * L) and eq(grads["dgamma"], d.k2 * N * L)
    # eval mode: forward and the whole backward, bias gradient included
    # (no single-pass kernel in eval mode: the shape lands on the apply kernel its row length selects)
    eval_route = "flat" if L < 256 else "rows-aligned" if L % 256 == 0 else "rows-straddling"
    r = bn_rows.row("exact-" + route, eval_route, shape, lif=True, v_in=True, bf16=True, grads="uyv", training=False, bias=True, res="res",
                    eps=0.0)
    prove_route(ops, r)
    out, grads = run_op(ops, r, d, True)
    fw = bn_ref.forward(*bn_rows.fwd_args(r, d), residual=d.residual)
    y, v, s, bits = bn_ref.neuron(d.v_in.double() + fw.u, 8, 1.0)
    assert eq(out.u, fw.u) and eq(out.y, y) and eq(out.v, v) and out.counters == [int(s.sum()), int((s != 0).sum())]
    bw = bn_ref.backward(d.z, d.bias, d.gamma, d.beta, d.rm, d.rv, False, 0.0, bits=bits, **bn_rows.loss_grads(r, d))
    for k in ("gz", "dgamma", "dbeta", "dbias", "g_residual"):
        assert eq(grads[k], getattr(bw, k)), k
