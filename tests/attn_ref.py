"""Plain fp64 restatement of the spike-driven attention core (spike2former_amd/csrc/sdsa.hip) on channel-major maps [TB, C, N], channel
c = head * d + j -- a test helper, no conftest, nothing of the package imported: torch only.  Written from the formulas the
kernel's header quotes (sdtv2.py:335-339, transformer.py:253-274: o = scale q (k^T v), no softmax) and from the neuron convention of
oracle.s2f_oracle.lif_step / _QuantSTE, not from the kernels:

  kv [i][j]  = sum_n k[i][n] v[j][n]                 (per batch element and head; d x d)
  o  [j][n]  = scale sum_i q[i][n] kv[i][j]
  gq [i][n]  = scale sum_j go[j][n] kv[i][j]
  gkv[i][j]  = scale sum_n q[i][n] go[j][n]
  gk [i][n]  = sum_j v[j][n] gkv[i][j]
  gv [j][n]  = sum_i k[i][n] gkv[i][j]

With the neuron y = Q_IFNode(o) behind the core (reset membrane: h = o), the gradient g of y reaches o as go = g / D where
0 <= o <= D, else 0.  tests/test_attn_ref_host.py checks the closed forms against autograd of the expression, the neuron against
lif_step, and the mask packing against a per-element loop."""
import torch


def heads_view(t, heads):
    """[TB, C, N] -> [TB, heads, d, N] (a view: channel c = head * d + j)"""
    TB, C, N = t.shape
    return t.reshape(TB, heads, C // heads, N)


def kv_of(k, v, heads):
    """-> kv [TB, heads, d, d] = k v^T per head, WITHOUT the scale (what the kernels save)"""
    return heads_view(k, heads) @ heads_view(v, heads).transpose(-1, -2)


def forward(q, k, v, heads, scale, dtype=torch.float64):
    """-> (o [TB, C, Nq], kv [TB, heads, d, d]) in `dtype` (fp64: the reference; fp32: what a plain evaluation of the same association
    gives, for measuring)"""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    kv = kv_of(k, v, heads)
    o = (kv.transpose(-1, -2) @ heads_view(q, heads)) * scale
    return o.reshape(q.shape), kv


def backward(q, k, v, go, heads, scale, dtype=torch.float64):
    """The three gradients in closed form -> (gq, gk, gv, gkv); gkv [TB, heads, d, d] carries the scale, as the kernels' workspace."""
    q, k, v, go = q.to(dtype), k.to(dtype), v.to(dtype), go.to(dtype)
    kv = kv_of(k, v, heads)
    goh = heads_view(go, heads)
    gq = (kv @ goh) * scale
    gkv = (heads_view(q, heads) @ goh.transpose(-1, -2)) * scale
    gk = gkv @ heads_view(v, heads)
    gv = gkv.transpose(-1, -2) @ heads_view(k, heads)
    return gq.reshape(q.shape), gk.reshape(k.shape), gv.reshape(v.shape), gkv


def abs_sums(q, k, v, go, heads):
    """The sum of ABSOLUTE terms behind every entry of kv, o, gq, gkv, gk, gv (scale 1; the entries of kv / gkv that enter the second
    sums are themselves replaced by their sums of absolute terms: an upper bound).  While such a sum stays below 2^24 granules -- the
    granule: the product of the operands' common denominators -- every partial sum of the entry is an integer number of granules below
    2^24, i.e. exact in fp32 in ANY order of the additions."""
    q, k, v, go = q.double().abs(), k.double().abs(), v.double().abs(), go.double().abs()
    o, kv = forward(q, k, v, heads, 1.0)
    gq, gk, gv, gkv = backward(q, k, v, go, heads, 1.0)
    return {"kv": kv, "o": o, "gq": gq, "gkv": gkv, "gk": gk, "gv": gv}


def in_range(o, D=8):
    """the straight-through mask of y = Q_IFNode(o) from a reset membrane: 0 <= o <= D, both ends included (_QuantSTE.backward)"""
    return (o >= 0) & (o <= D)


def neuron(o, D=8):
    """y = Q_IFNode(o) from a reset membrane -> (y, counts): counts = rint(clamp(o, 0, D)) (torch.round: half to even), y = counts / D"""
    s = torch.round(torch.clamp(o, min=0, max=D))
    return s / D, s


def firing(counts):
    """-> (sum of spike counts, number of non-zero counts): the two firing counters of a neuron kernel"""
    return int(counts.sum().item()), int((counts != 0).sum().item())


def fused_grad(o, g, D=8):
    """the gradient of o when g is the gradient of y = Q_IFNode(o)"""
    return torch.where(in_range(o, D), g.to(o.dtype) / D, torch.zeros_like(o))


def pack_mask(bits):
    """bool tensor (any shape; element e = its index in the contiguous tensor) -> int64 words in the layout of s2f_lif_mask_words:
    four words per tile of 256 elements; element e is bit (e & 255) >> 2 of word (e & 3) of tile e >> 8; a last, partly filled tile is
    padded with zero bits."""
    flat = bits.reshape(-1).to(torch.int64)
    n = flat.numel()
    tiles = (n + 255) >> 8
    padded = torch.zeros(tiles * 256, dtype=torch.int64)
    padded[:n] = flat
    b = padded.reshape(tiles, 64, 4)                                      # [tile, bit, word]
    shifts = torch.arange(64, dtype=torch.int64).reshape(1, 64, 1)
    # the shifted bits of one word are disjoint, so the sum is their OR; bit 63 lands on the sign bit of the int64 word (wrap-around
    # of the two's complement sum is exactly that bit pattern)
    return (b << shifts).sum(1).reshape(-1)
