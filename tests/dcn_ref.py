"""Plain fp64 restatement of the DCNv3 sampling core (spike2former_amd/ops/attention.py: dcnv3_core, dcnv3_core_cm) with its three
gradients -- a test helper, no conftest, nothing of the package imported: torch only.  Written from the formula of SURVEY.md
appendix C.5, as explicit gathers and one scatter-add, not from the kernels, not through grid_sample and not through autograd:

  maps       x [N, H, W, G*Cg], offset [N, Ho, Wo, G*P*2] ((x, y) per tap), mask [N, Ho, Wo, G*P], gy and y [N, Ho, Wo, G*Cg];
             P = Kh*Kw, tap k = i_w*Kh + j_h (kernel-w outer), Ho = (H + 2 ph - (dh (Kh - 1) + 1)) // sh + 1, Wo likewise
  position   px = wo*sw + c0w + (i_w - (Kw-1)//2) * dw * s + off_x * s      c0w = (dw*(Kw-1))//2,  s = offset_scale
             py = ho*sh + c0h + (j_h - (Kh-1)//2) * dh * s + off_y * s      in the coordinates of the map padded by (ph, pw) zeros
  corners    x0 = floor(px), lx = px - x0 (y likewise); the corner q = (ey, ex) in {0, 1}^2 reads v_q = x[n, y0 + ey - ph, x0 + ex - pw]
             -- zero outside the map -- with the weight w_q = (ey ? ly : 1 - ly) * (ex ? lx : 1 - lx)
  y[c]       = sum_k m_k sum_q w_q v_q[c]
  dmask_k    = sum_c gy[c] sum_q w_q v_q[c]
  doffset_k  = s m_k sum_c gy[c] ( (1 - ly) (v_01 - v_00) + ly (v_11 - v_10),          the x component: d/d px of the bilinear form
                                   (1 - lx) (v_10 - v_00) + lx (v_11 - v_01) )         the y component
  dx         scatter-add: every corner inside the map receives gy[c] m_k w_q at its pixel

(floor makes the derivative with respect to a position that is exactly an integer the right-hand one, as autograd through
px - floor(px) and through grid_sample does.)  `dtype`: fp64 is the reference; fp32 evaluates the same association plainly, for
measuring.  The maps may live on any device.  tests/test_dcn_ref_host.py checks the closed forms against autograd of the oracle and
of F.grid_sample in fp64, abs_sums against the same operations on absolute values, and the golden vectors of the reference."""
import torch


def out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - (dh * (Kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (Kw - 1) + 1)) // sw + 1


def positions(offset, H, W, G, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, dtype=torch.float64):
    """(px, py), each [N, Ho, Wo, G, P]: the sampling positions in padded coordinates, every operation in `dtype`, left to right"""
    Ho, Wo = out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    P = Kh * Kw
    N = offset.shape[0]
    dev = offset.device
    off = offset.to(dtype).reshape(N, Ho, Wo, G, P, 2)
    s = torch.tensor(offset_scale, dtype=dtype, device=dev)
    k = torch.arange(P, device=dev)
    iw = (k // Kh - (Kw - 1) // 2).to(dtype).view(1, 1, 1, 1, P)
    jh = (k % Kh - (Kh - 1) // 2).to(dtype).view(1, 1, 1, 1, P)
    wo = (torch.arange(Wo, device=dev) * sw).to(dtype).view(1, 1, Wo, 1, 1)
    ho = (torch.arange(Ho, device=dev) * sh).to(dtype).view(1, Ho, 1, 1, 1)
    px = wo + float((dw * (Kw - 1)) // 2) + iw * float(dw) * s + off[..., 0] * s
    py = ho + float((dh * (Kh - 1)) // 2) + jh * float(dh) * s + off[..., 1] * s
    return px, py


def _evaluate(x, offset, mask, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, dtype, absolute):
    """absolute=False: (y, dx, doffset, dmask).  absolute=True: the same sums over the ABSOLUTE values of their terms (a difference of
    two corner values counts as two terms), and the number of terms behind every entry."""
    N, H, W, C = x.shape
    assert C == G * Cg
    P = Kh * Kw
    Ho, Wo = out_hw(H, W, Kh, Kw, sh, sw, ph, pw, dh, dw)
    dev = x.device
    x, mask, gy = x.to(dtype), mask.to(dtype), gy.to(dtype)
    if absolute:
        x, mask, gy = x.abs(), mask.abs(), gy.abs()
    sgn = 1.0 if absolute else -1.0
    px, py = positions(offset, H, W, G, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, dtype)
    x0, y0 = torch.floor(px), torch.floor(py)
    lx, ly = px - x0, py - y0
    # far positions: clamp before the integer conversion (everything outside [-2, size + 2] is outside either way)
    ix = x0.clamp(-2, W + 2 * pw + 2).long() - pw
    iy = y0.clamp(-2, H + 2 * ph + 2).long() - ph
    x4 = x.reshape(N, H * W, G, Cg)
    m = mask.reshape(N, Ho, Wo, G, P)
    g5 = gy.reshape(N, Ho, Wo, G, Cg)
    nidx = torch.arange(N, device=dev).view(N, 1, 1, 1, 1).expand(N, Ho, Wo, G, P)
    gidx = torch.arange(G, device=dev).view(1, 1, 1, G, 1).expand(N, Ho, Wo, G, P)
    v, w, pix, ok = {}, {}, {}, {}
    for ey in (0, 1):
        for ex in (0, 1):
            yy, xx = iy + ey, ix + ex
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            p = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            q = (ey, ex)
            ok[q], pix[q] = inside, p
            v[q] = x4[nidx, p, gidx] * inside.to(dtype).unsqueeze(-1)          # [N, Ho, Wo, G, P, Cg]
            w[q] = (ly if ey else 1 - ly) * (lx if ex else 1 - lx)             # [N, Ho, Wo, G, P]
    sampled = sum(w[q].unsqueeze(-1) * v[q] for q in w)                        # sum_q w_q v_q
    y = (m.unsqueeze(-1) * sampled).sum(4)
    gc = g5.unsqueeze(4)                                                       # [N, Ho, Wo, G, 1, Cg]
    dmask = (gc * sampled).sum(5)
    ddx = (1 - ly).unsqueeze(-1) * (v[0, 1] + sgn * v[0, 0]) + ly.unsqueeze(-1) * (v[1, 1] + sgn * v[1, 0])
    ddy = (1 - lx).unsqueeze(-1) * (v[1, 0] + sgn * v[0, 0]) + lx.unsqueeze(-1) * (v[1, 1] + sgn * v[0, 1])
    s = torch.tensor(offset_scale, dtype=dtype, device=dev)
    doffset = torch.stack(((gc * ddx).sum(5) * m * s, (gc * ddy).sum(5) * m * s), dim=5)
    dx = torch.zeros(N * H * W * G, Cg, dtype=dtype, device=dev)
    landed = torch.zeros(N * H * W * G, dtype=dtype, device=dev)
    for q in w:
        rows = ((nidx * (H * W) + pix[q]) * G + gidx)[ok[q]]
        dx.index_add_(0, rows, (gc * (m * w[q]).unsqueeze(-1))[ok[q]])
        landed.index_add_(0, rows, torch.ones(rows.shape, dtype=dtype, device=dev))
    out = (y.reshape(N, Ho, Wo, C), dx.reshape(N, H, W, C), doffset.reshape(N, Ho, Wo, G * P * 2), dmask.reshape(N, Ho, Wo, G * P))
    if not absolute:
        return out
    terms = (torch.full_like(out[0], 4 * P), landed.view(N, H, W, G, 1).expand(N, H, W, G, Cg).reshape(N, H, W, C),
             torch.full_like(out[2], 4 * Cg), torch.full_like(out[3], 4 * Cg))
    return out, terms


def dcnv3(x, offset, mask, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, dtype=torch.float64):
    """dcnv3_core_pytorch and its gradients for the output gradient gy -> (y, dx, doffset, dmask)"""
    return _evaluate(x, offset, mask, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, dtype, False)


def abs_sums(x, offset, mask, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale):
    """((A_y, A_dx, A_doffset, A_dmask), (T_y, T_dx, T_doffset, T_dmask)) in fp64: per entry of what dcnv3 returns, the sum A of the
    ABSOLUTE values of the terms added into it -- the same expressions on |x|, |mask|, |gy| with the bilinear weights as they are
    (they are not negative) and every difference of two corner values read as two terms -- and the number T of those terms: 4 P
    for y, 4 Cg for doffset and dmask, the number of corners that landed on the pixel for dx.  While A stays below 2^24 granules --
    the granule: the product of the operands' common denominators -- every partial sum of the entry is a whole number of granules
    below 2^24, i.e. exact in fp32 in ANY order of the additions; and T + 6 roundings of 2^-24 A each bound what an fp32 evaluation
    of T terms in any order, with the few roundings inside one term, can lose."""
    return _evaluate(x, offset, mask, gy, G, Cg, Kh, Kw, sh, sw, ph, pw, dh, dw, offset_scale, torch.float64, True)
