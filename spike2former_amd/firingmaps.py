"""Per-pixel firing-rate maps of any neuron: WHERE in the picture a layer fires (the figure the spike-driven-transformer papers print
per layer beside their mIoU tables; `FiringRecorder`, `FiringLog` and `OpCensus` give one number per neuron).

    with s2f.FiringMaps(model, layers=r"backbone\\.|pixel_decoder\\.") as maps:      # registers the hooks; __exit__ removes them
        model.test_step(batch)
        read = maps.read()                                                          # ONE read-back
        panel = vis.draw_firing(picture, read, image=0)

Every selected `Q_IFNode` / `LIFNode` carries one `nn.Module` forward hook, which sees the fp32 spikes of the reference's interface
(every fused, memoised and pre-fired route steps aside for a hooked neuron, and `GraphedPredict` runs eager); the hook makes ONE launch
over that tensor (`ops.firing_map`, s2f_firing_map) into an int32 [B, 4, h, w] of this neuron: per image and pixel, over time steps
and channels, {sum of the integer levels, non-zero elements, max level, elements off the 1 / D grid}.  Nothing in a hook reads the
device back.  An opt-in diagnostic: with no FiringMaps attached every launch, allocation and bit of the package is what it was.

Geometry (`map_geometry`): decided from the output's shape, T, and the size of the picture batch the BACKBONE was last called with
(one forward pre-hook on `model.backbone` -- on the model itself when it has none --, which also fires under SegTTAModel and
slide inference, whose passes do not go through the segmentor's `forward`).  Leading dimensions (T, B) or (T B), then C, then either
(h, w) or one N; (h, w), or the (H_in / s, W_in / s) that N stands for, must be the input's size over ONE power-of-two stride s (there
is at most one).  A neuron whose output is anything else gets no map and no exception: `maps.skipped[name]` says why -- not
contiguous, another rank, no such stride, two readings that both fit, or token-major (the decoder's [T, B, Q, C] query stream, whose
neurons are named by `token_major`: a shape alone cannot tell Q x C from C x N).

A forward with another input size or batch clears all maps first: under `SegTTAModel` the maps are those of the views of the LAST
scale.  Maps of the captured training step, token-major layouts and per-time-step maps are out of scope."""
import collections
import re
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .neuron import LIFNode, Q_IFNode

# the query stream of MaskFormerHead: [T, B, Q, C] (and its channel-major twin [T, B, C, Q]) -- no picture geometry
TOKEN_MAJOR = r"(^|\.)(transformer_decoder|mask_embed|mask_embed_spike|decoder_out_spike|shortcut_conv_spike)(\.|$)"


def _stride_of(h, w, H_in, W_in):
    """the power-of-two s with (h, w) == (H_in / s, W_in / s) exactly, or None"""
    if h < 1 or w < 1 or H_in % h or W_in % w:
        return None
    s = H_in // h
    return s if s & (s - 1) == 0 and W_in // w == s else None


def _grid_of(N, H_in, W_in):
    """N -> (h, w, s) = (H_in / s, W_in / s, s) for the power-of-two s dividing both sizes with N s^2 == H_in W_in, or None (the
    product falls strictly with s: at most one fits)"""
    s = 1
    while s <= min(H_in, W_in):
        if H_in % s == 0 and W_in % s == 0 and N * s * s == H_in * W_in:
            return H_in // s, W_in // s, s
        s *= 2
    return None


def map_geometry(shape, T, B, H_in, W_in):
    """The layout rule.  shape: a neuron output's; T: time steps; (B, H_in, W_in): the picture batch.  -> (C, h, w, s) or a string,
    the reason there is no map.  Accepted: [T, B, C, h, w], [T B, C, h, w], [T, B, C, N], [T B, C, N]."""
    shape = tuple(int(d) for d in shape)
    fits = []
    if len(shape) == 5:
        if shape[:2] == (T, B):
            s = _stride_of(shape[3], shape[4], H_in, W_in)
            if s is not None:
                fits.append((shape[2], shape[3], shape[4], s))
    elif len(shape) == 4:
        if shape[0] == T * B:
            s = _stride_of(shape[2], shape[3], H_in, W_in)
            if s is not None:
                fits.append((shape[1], shape[2], shape[3], s))
        if shape[:2] == (T, B):
            g = _grid_of(shape[3], H_in, W_in)
            if g is not None:
                fits.append((shape[2],) + g)
    elif len(shape) == 3:
        if shape[0] == T * B:
            g = _grid_of(shape[2], H_in, W_in)
            if g is not None:
                fits.append((shape[1],) + g)
    else:
        return f"rank {len(shape)}: {shape}"
    if not fits:
        return f"no power-of-two stride of the {H_in} x {W_in} input (T {T}, B {B}) fits {shape}"
    if len(set(fits)) > 1:
        return f"ambiguous: {shape} reads both as [T B, C, h, w] and as [T, B, C, N]"
    return fits[0]


class FiringMapRead(collections.namedtuple("FiringMapRead", "names planes meta")):
    """What `FiringMaps.read()` returns.  names: the neurons with a map, in `named_modules()` order; planes[name]: int32 [B, 4, h, w]
    = {level sum, non-zero elements, max level, off-grid elements} per image and pixel; meta[name]: (T, C, D, passes) -- `passes`
    the calls of the neuron the planes add up."""
    __slots__ = ()

    def rate(self, name):
        """float64 [B, h, w]: the mean integer level per element over D -- the firing rate in 0 .. 1 of each pixel"""
        T, C, D, passes = self.meta[name]
        return self.planes[name][:, 0].astype(np.float64) / (T * C * D * passes)

    def active(self, name):
        """float64 [B, h, w]: the share of (time step, channel) elements of each pixel that fired at all"""
        T, C, D, passes = self.meta[name]
        return self.planes[name][:, 1].astype(np.float64) / (T * C * passes)

    def off_grid(self, name):
        """the elements that were no multiple of 1 / D in 0 .. 65535 / D: 0 for a sound spike map"""
        return int(self.planes[name][:, 3].astype(np.int64).sum())

    def summary(self):
        """per neuron: the mean and the max rate, the share of silent pixels (no element fired), the map's size -- one line of
        vis_data/firing_maps.jsonl (FiringMapHook)"""
        out = OrderedDict()
        for n in self.names:
            r = self.rate(n)
            out[n] = dict(mean=float(r.mean()), max=float(r.max()), silent=float((self.planes[n][:, 1] == 0).mean()),
                          shape=list(r.shape[1:]))
        return out


class FiringMaps:
    """model: the segmentor (or any module with Q_IFNode / LIFNode inside; a SegTTAModel: its `module`'s neurons are found through
    it).  layers: None -- every Q_IFNode / LIFNode --, a regex searched in the module name, or a predicate of that name.
    T: the time steps of the leading dimension (default `model.backbone.T`).  token_major: regex of the neurons of a token-major
    stream (-> skipped).  `with` attaches on entry and detaches on exit; `attach()` / `detach()` by hand: between `detach()` and
    `attach()` the neurons carry no hooks, and the fast routes and GraphedPredict's replays are back.  A neuron that also has a live
    FiringRecorder / FiringLog counter is fine: hooks and counters are independent."""

    def __init__(self, model, layers=None, T=None, token_major=TOKEN_MAJOR):
        self.model = model
        if layers is None:
            chosen = lambda n, m: True  # noqa: E731
        elif callable(layers):
            chosen = lambda n, m: bool(layers(n))  # noqa: E731
        else:
            pattern = re.compile(layers)
            chosen = lambda n, m: pattern.search(n) is not None  # noqa: E731
        self.nodes = OrderedDict((n, m) for n, m in model.named_modules() if isinstance(m, (Q_IFNode, LIFNode)) and chosen(n, m))
        if not self.nodes:
            raise ValueError("FiringMaps: no Q_IFNode or LIFNode selected")
        owner = next((m for m in model.modules() if isinstance(getattr(m, "backbone", None), torch.nn.Module)), None)
        self._front = owner.backbone if owner is not None else model
        if T is None:
            if owner is None or not hasattr(owner.backbone, "T"):
                raise ValueError("FiringMaps: T= is needed: the model has no backbone.T")
            T = owner.backbone.T
        self.T = int(T)
        self._token_major = re.compile(token_major) if token_major else None
        self._handles = []
        self._input = None          # (B, H_in, W_in) of the forward under way
        self._stats = {}          # name -> int32 [B, 4, h, w]
        self.clear()

    # ------------------------------------------------------------------------------------------------ hooks
    @property
    def attached(self):
        return bool(self._handles)

    def attach(self):
        if self._handles:
            return self
        self._handles.append(self._front.register_forward_pre_hook(self._see_input))
        for name, m in self.nodes.items():
            self._handles.append(m.register_forward_hook(lambda mod, args, out, name=name: self._see_output(name, mod, args, out)))
        return self

    def detach(self):
        for h in self._handles:
            h.remove()
        self._handles = []
        self._last_input = {}
        return self

    def __enter__(self):
        return self.attach()

    def __exit__(self, *exc):
        self.detach()
        return False

    def clear(self):
        """forget every map, pass count and skip reason (the allocations of an unchanged geometry are kept and overwritten by the next
        pass: no launch here)"""
        self.passes = OrderedDict()
        self.skipped = OrderedDict()
        self._geometry = {}          # name -> (C, h, w, s)
        self._last_input = {}          # name -> the input of the neuron's last sighting (_echo)

    def _see_input(self, module, args):
        x = args[0] if args else None
        if not torch.is_tensor(x) or x.dim() != 4:
            raise RuntimeError("FiringMaps: the watched front module was not called with a [B, 3, H, W] batch")
        size = (int(x.shape[0]), int(x.shape[2]), int(x.shape[3]))
        if size != self._input:
            self.clear()          # another picture size or batch: the maps begin again
            self._stats = {}
        self._input = size
        self._last_input = {}

    def _echo(self, name, args):
        """Whether this sighting repeats the last one.  A neuron that a producer kernel has already applied (fused.py: `next_lif`,
        Q_IFNode.prefire) shows its call to the hooks TWICE: once from the producer's site and once more when the consumer's module
        call hands the pre-fired spikes out -- on the same input tensor, unchanged.  The second is no call of the neuron (its firing
        counters count one), so it adds no pass.  The input of the last sighting is held (not just its address: a freed address is
        reused) until the neuron's next sighting, the next forward, `read()`, `clear()` or `detach()`."""
        x = args[0] if args else None
        if not torch.is_tensor(x):
            return False
        last = self._last_input.pop(name, None)
        if last is not None and (last[0].data_ptr(), last[1], last[0].numel()) == (x.data_ptr(), x._version, x.numel()):
            return True
        self._last_input[name] = (x, x._version)
        return False

    def _see_output(self, name, module, args, out):
        if name in self.skipped or self._echo(name, args):
            return
        if self._input is None:
            raise RuntimeError(f"FiringMaps: neuron {name!r} ran before any input was seen")
        out = out.data if isinstance(out, ops.Spikes) else out
        B, H_in, W_in = self._input
        if self._token_major is not None and self._token_major.search(name):
            self.skipped[name] = "token-major stream"
            return
        geo = map_geometry(out.shape, self.T, B, H_in, W_in)
        if isinstance(geo, str):
            self.skipped[name] = geo
            return
        if not out.is_contiguous():
            self.skipped[name] = "not contiguous"
            return
        if out.dtype not in (torch.float32, torch.bfloat16):
            self.skipped[name] = f"dtype {out.dtype}"
            return
        C, h, w, _ = geo
        if self._geometry.get(name, geo) != geo:          # (a shared neuron called on two geometries in one pass)
            self.skipped[name] = f"called with two geometries: {self._geometry[name]} and {geo}"
            self.passes.pop(name, None)
            return
        passes = self.passes.get(name, 0)
        if not ops.firing_map_sum_ok(self.T * C, passes + 1):
            raise OverflowError(f"FiringMaps: pass {passes + 1} of neuron {name!r} ({self.T} x {C} planes per image) could take a level "
                                f"sum past 2^31: read() and clear() first")
        stats = self._stats.get(name)
        if stats is None or tuple(stats.shape) != (B, ops.FIRING_MAP_PLANES, h, w) or stats.device != out.device:
            stats = self._stats[name] = torch.empty(B, ops.FIRING_MAP_PLANES, h, w, dtype=torch.int32, device=out.device)
        self._geometry[name] = geo
        ops.firing_map(out.view(self.T * B, C, h, w), B, module.D, stats, assign=passes == 0)
        self.passes[name] = passes + 1

    # ------------------------------------------------------------------------------------------------ reading
    def read(self):
        """-> FiringMapRead.  ONE read-back: the planes of all neurons leave the device as one tensor."""
        self._last_input = {}
        names = [n for n in self.nodes if self.passes.get(n, 0) > 0]
        planes, meta = OrderedDict(), OrderedDict()
        if names:
            flat = torch.cat([self._stats[n].reshape(-1) for n in names]).cpu().numpy()
            at = 0
            for n in names:
                shape = tuple(self._stats[n].shape)
                size = int(np.prod(shape))
                planes[n] = flat[at:at + size].reshape(shape).copy()
                at += size
                meta[n] = (self.T, self._geometry[n][0], int(self.nodes[n].D), self.passes[n])
        return FiringMapRead(names, planes, meta)
