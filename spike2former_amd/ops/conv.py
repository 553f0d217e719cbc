"""Depthwise stencils (csrc/dwconv.hip) and dense k x k convolutions lowered to the GEMM kernels."""
import ctypes

import torch

from .config import cfg
from .core import *          # noqa: F401,F403  (the shared plumbing: _ptr, _stream, check, lib, Spikes, ...)
from .gemm import *          # noqa: F401,F403
from .wcache import pack_weight_conv3, split_weight_conv3, split_weight_tconv3


# ------------------------------------------------------------------------------------------------ depthwise conv
class _DWConv(torch.autograd.Function):
    """Depthwise KxK, stride 1 (nn.Conv2d(groups=C)); `border` = per-channel constant padding value (detached).
    x: fp32, or a bf16 spike map with its autograd handle `tok`."""

    @staticmethod
    def forward(ctx, x, tok, w, border, pad, stats=False):
        _need_cuda(w, border, spikes=x)
        x, w = x.contiguous(), w.contiguous()
        N, C, H, W = x.shape
        K = w.shape[-1]
        Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
        y = torch.empty(N, C, Ho, Wo, dtype=torch.float32, device=x.device)
        if border is not None:
            border = border.contiguous()
        xb = int(x.dtype == torch.bfloat16)
        # a train-mode BatchNorm follows (3 x 3 'same', no border): the stencil stores its per-workgroup (sum, sum of squares) next to
        # y and hands them over like the GEMMs do (cfg.BN_PARTIALS, gemm.stats_of) -- no statistics pass over y
        P = 0
        if stats and K == 3 and pad == 1 and border is None and _want_partials(True, N, C, H * W) and x.data_ptr() % 16 == 0:
            P = int(lib.s2f_dwconv_stats_slots(N, H, W))
        if P:
            part = torch.empty(C, P, 2, dtype=torch.float32, device=x.device)
            check(lib.s2f_dwconv_fwd_stats(_ptr(x), _ptr(w), _ptr(y), _ptr(part), P, N, C, H, W, xb, _stream()), "s2f_dwconv_fwd_stats")
        else:
            check(lib.s2f_dwconv_fwd(_ptr(x), _ptr(w), _ptr(border), _ptr(y), N, C, H, W, K, pad, xb, _stream()),
                  "s2f_dwconv_fwd")
        ctx.save_for_backward(x, w, border)
        ctx.pad, ctx.has_tok = pad, tok is not None
        if not P:
            part = y.new_empty(0)
        ctx.mark_non_differentiable(part)
        ctx.set_materialize_grads(False)          # (no zero-filled "gradient" of the partials)
        return y, part

    @staticmethod
    def backward(ctx, gy, _gpart=None):
        x, w, border = ctx.saved_tensors
        if gy is None:
            return _grads(ctx)
        gy = gy.contiguous()
        N, C, H, W = x.shape
        K = w.shape[-1]
        gx = gw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gx = torch.empty(N, C, H, W, dtype=torch.float32, device=gy.device)
            check(lib.s2f_dwconv_bwd_input(_ptr(gy), _ptr(w), _ptr(gx), N, C, H, W, K, ctx.pad, _stream()),
                  "s2f_dwconv_bwd_input")
        if ctx.needs_input_grad[2]:
            sink = _sink_for(w)
            gw = torch.empty_like(w) if sink is None else None
            side = _wgrad_stream(sink, gy, x, border)
            check(lib.s2f_dwconv_bwd_weight(_ptr(x), _ptr(border), _ptr(gy), _ptr(gw if sink is None else sink), N, C, H, W,
                                            K, ctx.pad, int(sink is not None), int(x.dtype == torch.bfloat16),
                                            side.cuda_stream if side is not None else _stream()), "s2f_dwconv_bwd_weight")
        return _grad_pair(ctx.has_tok, gx) + (gw, None, None, None)


def dwconv_bn_lif_eval(x, w, pad, running_mean, running_var, gamma, beta, eps, border=None, want_pre=False, lif=False, D=8, vth=1.0,
                       stats=None):
    """Eval-mode  depthwise conv -> BatchNorm(running statistics) [-> Q_IFNode (reset, no membrane kept)]  as ONE launch
    (s2f_dwconv_bn_lif_fwd; row f4).  x: fp32 tensor or Spikes [N, C, H, W]; w [C, 1, K, K] -> (u fp32 or None, Spikes or None)."""
    data, _ = _unpack(x)
    data = data.contiguous()
    N, C, H, W = data.shape
    K = w.shape[-1]
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    if _TAP[0] is not None:
        _TAP[0]("dwconv", w, conv_macs(N, C, H, W, C, K, K, 1, pad, C), (("x", x, 1),))
    dev = data.device
    with torch.no_grad():
        u = torch.empty(N, C, Ho, Wo, dtype=torch.float32, device=dev) if want_pre else None
        y = torch.empty(N, C, Ho, Wo, dtype=torch.bfloat16, device=dev) if lif else None
        check(lib.s2f_dwconv_bn_lif_fwd(_ptr(data), _ptr(w.detach().contiguous()), _ptr(None if border is None else border.contiguous()),
                                        _ptr(running_mean), _ptr(running_var), _ptr(gamma), _ptr(beta), float(eps), _ptr(u), _ptr(y),
                                        _ptr(stats), N, C, H, W, K, pad, int(data.dtype == torch.bfloat16), float(vth), int(D), _stream()),
              "s2f_dwconv_bn_lif_fwd")
    return u, (_spikes(None, y) if lif else None)


def dwconv(x, w, pad, border=None, stats=False):
    """x: fp32 tensor or Spikes.  stats: the consumer is a train-mode BatchNorm -- where the stencil can (3 x 3, pad 1, no border,
    cfg.BN_PARTIALS) it stores the BatchNorm partials with y and hands them over as y's `_s2f_part` (gemm.stats_of)"""
    data, tok = _unpack(x)
    if _TAP[0] is not None:
        N, C, H, W = data.shape
        K = w.shape[-1]
        _TAP[0]("dwconv", w, conv_macs(N, C, H, W, C, K, K, 1, pad, C), (("x", x, 1),))
    return _with_part(*_DWConv.apply(data, tok, w, border, pad, bool(stats)))




# ------------------------------------------------------------------------------------------------ dense k x k convolution
# 3x3 / stride 1 / pad 1 spike convolutions as implicit GEMMs (no im2col matrix; s2f_spike_conv3x3_fwd / _dw).  Round 1 measured
# the pair (forward + weight gradient) as a win on the >= 128x128 maps only (tools/probe_conv3.py: 64x64 maps 485 vs 420 and
# 795 vs 660 us against the saved column matrix).  With the loaders' prefetches freed of their predicates (round 2, conv3_fix)
# the implicit form wins from 32x32 up -- same-box A/B of the step: threshold 128x128 43.92, 64x64 43.39, 32x32 43.44 ms -- and
# the bf16 column matrices of the 64x64 / 32x32 stages (ATen im2col) are gone.
# Input gradient of the 3x3 convolutions: an implicit transposed convolution on the 6-pass split GEMM (no unfold / col2im).
def im2col(x, kh, kw, stride, padding):
    """torch.nn.functional.unfold(x, (kh, kw), 1, padding, stride) for fp32 maps and bf16 spike maps, as one gather kernel
    (csrc/im2col.hip): [N, C, H, W] -> [N, C kh kw, Ho Wo], the column matrix of the reference's stride-2 / 7x7 nn.Conv2d
    (mmseg/models/backbones/sdtv2.py:386-421)."""
    N, C, H, W = x.shape
    Ho = (H + 2 * padding - kh) // stride + 1
    Wo = (W + 2 * padding - kw) // stride + 1
    if not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("im2col: needs an fp32 or bf16 map in device memory (there is no host path)")
    x = x.contiguous()
    cols = torch.empty(N, C * kh * kw, Ho * Wo, dtype=x.dtype, device=x.device)
    check(lib.s2f_im2col(_ptr(x), _ptr(cols), N, C, H, W, kh, kw, stride, padding, int(x.dtype == torch.bfloat16), _stream()),
          "s2f_im2col")
    return cols


def col2im(dcols, C, H, W, kh, kw, stride, padding):
    """torch.nn.functional.fold(dcols, (H, W), (kh, kw), 1, padding, stride) as a gather: every input pixel sums the column entries
    that cover it, in a fixed order, with no zero fill (csrc/im2col.hip)."""
    N = dcols.shape[0]
    if not dcols.is_cuda or dcols.dtype != torch.float32:
        raise RuntimeError("col2im: needs fp32 columns in device memory (there is no host path)")
    dcols = dcols.contiguous()
    gx = torch.empty(N, C, H, W, dtype=torch.float32, device=dcols.device)
    check(lib.s2f_col2im(_ptr(dcols), _ptr(gx), N, C, H, W, kh, kw, stride, padding, _stream()), "s2f_col2im")
    return gx


class _ConvDense(torch.autograd.Function):
    """Dense k x k Conv2d lowered to GEMMs (MIOpen is not usable on this image, see conv.py).

    forward : cols = im2col(x) ; y = W2d @ cols                       (spike GEMM when x is a neuron output)
    dW      : dY @ cols^T                                              (bf16-MFMA batch-reduce kernel for spike inputs)
              3x3 / stride 1 / padding 1 on spikes: both as IMPLICIT GEMMs -- the kernels' loaders read x itself, `cols`
              (9x the activation: 2.4 GB for MS_ConvBlock1_1.conv2 at C2) is neither written, read nor saved
    dX      : the cheaper of two equivalent lowerings --
                M >= C : dcols = W2d^T @ dY ; dX = col2im(dcols)       (the adjoint of im2col; C*k*k rows)
                M <  C : dX = flip(W)^T (*) dY = W_t2d @ im2col(dY)     (transposed convolution; M*k*k rows)
              the second form moves k*k*M instead of k*k*C rows through HBM and needs no col2im scatter; it applies to
              stride 1 (MS_ConvBlock.conv2: 4C -> C, sdtv2.py:202-204)."""

    @staticmethod
    def forward(ctx, x, tok, weight, bias, stride, padding, spike_input, stats=False):
        _need_cuda(weight, bias, spikes=x)
        ctx.has_tok = tok is not None
        part = None
        xb = x.dtype == torch.bfloat16
        N, C, H, W = x.shape
        M, _, kh, kw = weight.shape
        Ho = (H + 2 * padding - kh) // stride + 1
        Wo = (W + 2 * padding - kw) // stride + 1
        w2d = weight.view(M, -1)
        # implicit GEMM: 3x3, stride 1, padding 1 on spikes -- the kernels' loaders read the activation itself
        implicit = (spike_input and cfg.SPIKE_GEMM_ENABLED and cfg.CONV3X3_IMPLICIT and kh == 3 and kw == 3 and stride == 1
                    and padding == 1 and C % 32 == 0 and W % 4 == 0
                    and H * W >= cfg.CONV3X3_IMPLICIT_MIN_PIXELS)
        if implicit:
            x = x.contiguous()
            if cfg.SPIKE_GEMM_CHECK:
                assert _is_spike_grid(x), "not a spike tensor"
            y = torch.empty(N, M, H * W, dtype=torch.float32, device=x.device)
            _time_next("spike_gemm_fwd", 4 * N * H * W * (C + M), 2 * N * M * H * W * C * 9,
                       moved=N * H * W * ((2 if xb else 4) * C + 4 * M))
            pg = xb and cfg.SPIKE_GEMM_TERMS == 3          # what the packed-weight pipeline takes
            P = _want_partials(stats and pg and bias is None, N, M, H * W)
            if P:
                part = torch.empty(M, P, 2, dtype=torch.float32, device=x.device)
                check(lib.s2f_pgemm_conv3x3_bf16_stats(_ptr(pack_weight_conv3(weight)), _ptr(x), _ptr(y), _ptr(part), N, M, C, H, W,
                                                       _stream()), "s2f_pgemm_conv3x3_bf16_stats")
            elif pg:
                check(lib.s2f_pgemm_conv3x3_bf16(_ptr(pack_weight_conv3(weight)), _ptr(x), _ptr(bias), _ptr(y), N, M, C, H, W, 0,
                                                 _stream()), "s2f_pgemm_conv3x3_bf16")
            else:
                ws = split_weight_conv3(weight)
                fn = lib.s2f_spike_conv3x3_fwd_bf16 if xb else lib.s2f_spike_conv3x3_fwd
                check(fn(_ptr(ws), _ptr(x), _ptr(bias), _ptr(y), N, M, C, H, W, ws.shape[1], ws.shape[2], cfg.SPIKE_GEMM_TERMS,
                         _stream()), "s2f_spike_conv3x3_fwd")
            ctx.save_for_backward(x, weight)
            ctx.geo = (N, C, H, W, M, kh, kw, Ho, Wo, stride, padding, bias is not None, True)
            ctx.implicit = True
            return y.view(N, M, Ho, Wo), _part_output(ctx, y, part)
        ctx.implicit = False
        cols = im2col(x, kh, kw, stride, padding)                                       # [N, C*kh*kw, Ho*Wo]
        use_mfma = spike_input and cfg.SPIKE_GEMM_ENABLED and cols.shape[2] % 4 == 0
        if use_mfma:
            y, part = _spike_product(cols, w2d, bias, stats)
        else:
            if xb:
                cols = cols.float()
            # general fp32 input (the stem reads the image): the product of dense_gemm with one weight, the bias added after it
            y, part = _dense_product(cols, [w2d], stats and bias is None)
            if bias is not None:
                y = y + bias.view(1, -1, 1)
        ctx.save_for_backward(cols, weight)
        ctx.geo = (N, C, H, W, M, kh, kw, Ho, Wo, stride, padding, bias is not None, use_mfma)
        return y.view(N, M, Ho, Wo), _part_output(ctx, y, part)

    @staticmethod
    def backward(ctx, gy, _gpart=None):
        cols, weight = ctx.saved_tensors
        if gy is None:
            return _grads(ctx)
        N, C, H, W, M, kh, kw, Ho, Wo, stride, padding, has_bias, use_mfma = ctx.geo
        gy = gy.contiguous().view(N, M, Ho * Wo)
        w2d = weight.view(M, -1)
        gx = gw = gb = None
        xb = cols.dtype == torch.bfloat16
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            if (cfg.CONV3X3_DX_IMPLICIT and kh == 3 and kw == 3 and stride == 1 and padding == 1 and M % 32 == 0 and W % 4 == 0
                    and gy.is_cuda):
                # transposed convolution dX = flip(W)^T (*) dY as an implicit 6-pass split GEMM: no unfold(dY), no col2im
                gx = torch.empty(N, C, H, W, dtype=torch.float32, device=gy.device)
                _time_next("dx_gemm", 4 * N * H * W * (C + M), 2 * N * M * H * W * C * 9)
                # measured (tools/probe_pgemm.py conv): the pipelined kernel wins for <= 64 output rows (narrow tiles: 442 vs 729 us
                # on [32 <- 128] at 256 x 256) and for long contractions (>= 256 channels); the round-2 kernel keeps a 5-10 % edge
                # on wide outputs over short contractions
                if C <= 64 or M >= 256:
                    check(lib.s2f_pgemm_conv3x3_f32(_ptr(pack_weight_conv3(weight, transposed=True)), _ptr(gy), _ptr(gx), N, C, M, H,
                                                    W, 0, _stream()), "s2f_pgemm_conv3x3_f32")
                else:
                    wt = split_weight_tconv3(weight)
                    check(lib.s2f_conv3x3_general(_ptr(wt), _ptr(gy), _ptr(gx), N, C, M, H, W, wt.shape[1], wt.shape[2], _stream()),
                          "s2f_conv3x3_general")
            elif M < C and stride == 1 and kh == kw and Ho == H and Wo == W:
                wt = weight.flip(2, 3).permute(1, 0, 2, 3).reshape(C, M * kh * kw)        # [C, M*k*k], tiny
                gcols = im2col(gy.view(N, M, Ho, Wo), kh, kw, 1, kh - 1 - padding)
                gx = _bmm_small(wt.unsqueeze(0).expand(N, -1, -1), gcols).view(N, C, H, W)
            else:
                dcols = dx_gemm(w2d, gy)
                gx = col2im(dcols, C, H, W, kh, kw, stride, padding)
        if ctx.needs_input_grad[2]:
            K = w2d.shape[1]
            if ctx.implicit:
                x = cols                                                  # the saved tensor is the activation itself
                # the kernels contract tap-major into a [M, 3, 3, C] staging tensor (the pipelined one adds into it, zeroed first); a
                # permuted add moves it to the sink (storing in the weight's own layout measured slower: docs/EXPERIMENTS.md)
                sink = _sink_for(weight)
                gt = torch.empty(M, 3, 3, C, dtype=torch.float32, device=gy.device)
                _time_next("spike_gemm_dw", 4 * N * H * W * (C + M), 2 * N * M * H * W * K,
                           moved=N * H * W * ((2 if xb else 4) * C + 4 * M))
                if xb and M >= 128 and C >= 64 and lib.s2f_spike_conv3x3_dw_pipe_ok(N, M, C, H, W):
                    # the LDS-DMA pipelined kernel (csrc/dwp.hip): the horizontal taps come from a copy shifted by one element.
                    # Its tile is 128 output channels x 256 (tap, input channel) rows: narrower layers stay on the round-2 kernel
                    # (measured, tools/probe_dwp_conv.py: M = 32 / 64 lose 10-70 %, C = 32 ties)
                    xs = torch.empty(x.numel() + 16, dtype=x.dtype, device=x.device)
                    check(lib.s2f_shift1_bf16(_ptr(x), _ptr(xs), x.numel(), _stream()), "s2f_shift1_bf16")
                    arr = (ctypes.c_int64 * 9)(_ptr(gy), _ptr(x), _ptr(xs), _ptr(gt), N, M, C, H, W)
                    gt.zero_()
                    check(lib.s2f_spike_conv3x3_dw_pipe(arr, 1, 0, 0, _stream()), "s2f_spike_conv3x3_dw_pipe")
                elif xb:
                    check(lib.s2f_spike_conv3x3_dw_bf16(_ptr(gy), _ptr(x), _ptr(gt), N, M, C, H, W, 0, _stream()),
                          "s2f_spike_conv3x3_dw_bf16")
                else:
                    check(lib.s2f_spike_conv3x3_dw(_ptr(gy), _ptr(x), _ptr(gt), N, M, C, H, W, 0, _stream()), "s2f_spike_conv3x3_dw")
                if sink is not None:
                    sink.view(M, C, 3, 3).add_(gt.permute(0, 3, 1, 2))
                    gw = None
                else:
                    gw = gt.permute(0, 3, 1, 2).contiguous()
            elif use_mfma and M >= 16:
                # (the stand-alone pipelined kernel: not measured for column-matrix operands, therefore off)
                gw = _spike_dw(gy, cols, weight, N, M, K, Ho * Wo, pipe=False)
            elif (Ho * Wo) % 4 == 0 and cols.dtype == torch.float32:
                # both operands general fp32 (the stem): 6-pass weight-gradient kernel, straight into the sink when there is one
                sink = _sink_for(weight)
                gw = torch.empty(M, K, dtype=torch.float32, device=gy.device) if sink is None else None
                check(lib.s2f_gemm_dw_general(_ptr(gy), 0, _ptr(cols), 0, _ptr(gw if sink is None else sink), N, M, K, Ho * Wo,
                                              int(sink is not None), _stream()), "s2f_gemm_dw_general")
            else:
                gw = _bmm_small(gy, cols.float().transpose(1, 2), reduce_batch=True)          # ragged / tiny maps (csrc/bmm.hip)
            gw = gw.view_as(weight) if gw is not None else None
        if has_bias and ctx.needs_input_grad[3]:
            gb = gy.sum((0, 2))
        return _grad_pair(ctx.has_tok, gx) + (gw, gb, None, None, None, None)


def conv_dense(x, weight, bias, stride, padding, spike_input, stats=False):
    """x: fp32 tensor, or Spikes (then `spike_input` is implied).  stats: as spike_gemm"""
    data, tok = _unpack(x)
    if _TAP[0] is not None:
        N, C, H, W = data.shape
        M, Cg, kh, kw = weight.shape
        _TAP[0]("conv", weight, conv_macs(N, C, H, W, M, kh, kw, stride, padding, C // Cg), (("x", x),))
    return _with_part(*_ConvDense.apply(data, tok, weight, bias, stride, padding, spike_input or isinstance(x, Spikes), bool(stats)))


__all__ = [n for n in dir() if not n.startswith('__')]
