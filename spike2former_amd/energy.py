"""Operations and energy: per-layer MACs, synaptic operations and an energy estimate -- the two figures a spiking-network result
table carries beside mIoU.  The reference stops half way: tools/cal_firing_num.py writes firing rates per neuron (fr_rate.csv, what
`FiringRecorder` reproduces) and leaves the operation counts to a spreadsheet (its FLOP half is commented out).

Firing rates times a hand count of layers is not enough here: not every synaptic layer reads a neuron's output (SepConv.pwconv2 reads
the depthwise convolution's real-valued map, the stem the image; the DCNv3 core, the attention products, alpha * spikes in the SDME
block, the mask contraction and the class-mask product read tensors no neuron counter describes).  So the census measures the
OPERANDS, on the device: while an `OpCensus` is live every synaptic op of the forward reports itself once per call from its ONE home,
the ops entry point (ops/core.py `_TAP`), and each activation operand costs one `ops.operand_census` launch (csrc/opcensus.hip) into
a row of an int64 table on the device -- {elements, sum of integer levels x * D, non-zero, OFF THE LEVEL GRID, max level, non-finite,
calls}.  The table is read back once, in `report()`.  The same pass checks the invariant the design rests on and nothing else checks
at the point of use: a spike map is exact multiples of 1 / D (`EnergyReport.spikes_off_grid()` must be empty).

        with s2f.OpCensus(model, max_passes=100) as census:     # puts the model in eval mode, runs under no_grad
            s2f.evaluate(model, batches, metric)                # or model.test_step(batch) by hand
        rep = census.report(e_mac=4.6e-12, e_ac=0.9e-12)        # -> EnergyReport
        rep.rows; rep.totals; rep.to_csv(path); rep.to_json(); print(rep)

Rows.  A weighted op's row key is the state_dict key of its weight (`backbone....pwconv1.weight`: the key the reference and the
oracle use), found by the weight's ADDRESS -- a launch whose weight spans several adjacent parameters (the q | k | v twins) yields one
row per parameter.  A weightless product is keyed `<module path>:<kind>[:<index>]` (`...attn:sdsa:kv`, `...attn:sdsa:q_kv`), the module
path being the innermost module of the census's model whose call is live, the index the product's ordinal (from 1; the first has
none) among the products of that kind under that path within one forward.

Counting rules (include/s2f.h "operand census").  MACs of one call:
    dense k x k conv             N C_out H_out W_out (C_in / groups) kh kw
    depthwise conv               N C H_out W_out kh kw
    1x1 conv / conv1d / linear   rows C_in C_out
    spike-driven attention       k^T v: TB heads N_k d d;  q (k^T v): TB heads N_q d d     (the association csrc/sdsa.hip contracts in)
    masked attention             q k^T and (q k^T) v: TB heads N_q N_k d each
    DCNv3 core                   5 N H_out W_out G Cg K: 4 bilinear taps of the map (`dcnv3:sample`) + 1 modulation by the mask
                                 (`dcnv3:modulate`) per sampling point -- two rows, they read different operands
    mask contraction             T B (L Q) C H W
    class_mask_product           B K Q H W
An operand is ON THE GRID when none of its elements is off it.  An op with at least one activation operand on the grid is
accumulate-only (class `ac`): each spike of that operand adds the other operand's value `level` times,
    SOPs = MACs * min(rate) over its on-grid operands,   rate = sum of levels / elements
(the mean integer count per element: the quantity in fr_rate.csv).  Any other op is `real`: it costs its MACs, and its row gives the
share of off-grid elements.   energy = e_mac * sum(real MACs) + e_ac * sum(SOPs).   The defaults, 4.6 pJ per MAC and 0.9 pJ per
accumulate, are the 45 nm figures the spike-driven-transformer papers quote; the reference has no energy formula (DESIGN.md
section 7: the figure's parity is UNPINNED; the integers -- MACs, levels, elements -- are pinned by the tests).
NOT counted: BatchNorm (folded into the convolution at inference), the neuron updates, residual adds, resizes, softmax / sigmoid.

A census pass runs the network's layers as the reference defines them: the routes that fold two layers into one product (the
mask_feature convolution inside the mask contraction) or skip dead outputs (`PREDICT_LAST_ONLY`) or lower a convolution to another
op's column matrix step aside through their switches, and a GraphedPredict runs the pass eager.  Eval-mode conv + BatchNorm + neuron
epilogues stay fused: still one op with one input.  After `max_passes` forwards of the model the taps go quiet, the switches return
and the rest of the evaluation runs at full speed.  Rows average over the passes.  A pass is one CALL of the model (`model(...)`, which
`test_step` and `evaluate` go through): drive the model through its call, not through `predict` / `inference` / `encode_decode`
directly -- `report()` raises when ops were counted and no pass was.  The membranes are reset when the census begins and
when it goes quiet (the switches change the shapes the SDME block's neurons see): carry no membrane across either border."""
import bisect
import csv
import json
from collections import OrderedDict

import torch

from . import ops
from .neuron import LIFNode, Q_IFNode, reset_net

E_MAC, E_AC = 4.6e-12, 0.9e-12          # J per multiply-accumulate / per accumulate (45 nm)
NOT_COUNTED = "not counted: BatchNorm (folded at inference), neuron updates, residual adds, resizes, softmax / sigmoid"
_FIELDS = ("elements", "level_sum", "nonzero", "off_grid", "max_level", "nonfinite")          # table columns 0 .. 5 (6: calls)
_TABLE_ROWS = 4096


# The counting rules themselves are functions of the op layer, where the taps call them (ops/core.py): conv_macs, linear_macs,
# product_macs, sdsa_macs, sdsa_masked_macs, dcnv3_macs.


# ------------------------------------------------------------------------------------------------ report arithmetic
def _ratio(a, b):
    return a / b if b else 0.0


def classify(operands):
    """operands: records with `elements`, `level_sum`, `off_grid` -> (klass, rate or None, off-grid share): `ac` with the smallest
    rate of the on-grid operands, or `real` with the share of off-grid elements over all operands"""
    on = [o for o in operands if o["off_grid"] == 0]
    share = _ratio(sum(o["off_grid"] for o in operands), sum(o["elements"] for o in operands))
    if on:
        return "ac", min(_ratio(o["level_sum"], o["elements"]) for o in on), share
    return "real", None, share


class EnergyReport:
    """rows: records {key, kind, calls, macs, operands [{name, spikes, elements, level_sum, nonzero, off_grid, max_level, nonfinite}],
    rate, sops, klass, off_share, energy_J} in first-call order -- calls and the operands' integers are sums over the passes, macs is
    per pass; totals: {params, macs, real_macs, sops, energy_mJ, passes}."""

    def __init__(self, rows, params=0, passes=1, e_mac=E_MAC, e_ac=E_AC, D=8):
        self.e_mac, self.e_ac, self.D = float(e_mac), float(e_ac), int(D)
        self.rows = []
        for r in rows:
            r = dict(r, operands=[dict(o) for o in r["operands"]])
            r["klass"], r["rate"], r["off_share"] = classify(r["operands"])
            r["sops"] = r["macs"] * r["rate"] if r["klass"] == "ac" else 0.0
            r["energy_J"] = self.e_ac * r["sops"] if r["klass"] == "ac" else self.e_mac * r["macs"]
            self.rows.append(r)
        real = [r for r in self.rows if r["klass"] == "real"]
        self.totals = OrderedDict(
            params=int(params), macs=sum(r["macs"] for r in self.rows), real_macs=sum(r["macs"] for r in real),
            sops=sum(r["sops"] for r in self.rows), energy_mJ=1e3 * sum(r["energy_J"] for r in self.rows), passes=int(passes))

    # ---- views
    @staticmethod
    def stage_of(key):
        """the first two components of a row key's module path ("(model)": a weightless product of the model's own forward)"""
        return ".".join(key.split(":")[0].split(".")[:2]) or "(model)"

    def by_stage(self):
        """-> OrderedDict stage -> {rows, macs, real_macs, sops, energy_J}, stages in first-row order"""
        out = OrderedDict()
        for r in self.rows:
            s = out.setdefault(self.stage_of(r["key"]), dict(rows=0, macs=0, real_macs=0, sops=0.0, energy_J=0.0))
            s["rows"] += 1
            s["macs"] += r["macs"]
            s["real_macs"] += r["macs"] if r["klass"] == "real" else 0
            s["sops"] += r["sops"]
            s["energy_J"] += r["energy_J"]
        return out

    def spikes_off_grid(self):
        """the rows with an operand that was handed over as ops.Spikes and yet has elements off the level grid: the invariant check
        (a spike map is exact multiples of 1 / D); empty for a sound model"""
        return [r for r in self.rows if any(o.get("spikes") and o["off_grid"] > 0 for o in r["operands"])]

    # ---- files
    _CSV = ("key", "kind", "klass", "calls", "macs", "rate", "sops", "off_share", "energy_J", "operands")

    def to_csv(self, path):
        """a header and one line per row; the operands as one JSON cell"""
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(self._CSV)
            for r in self.rows:
                w.writerow([json.dumps(r[c]) if c == "operands" else ("" if r[c] is None else repr(r[c]) if isinstance(r[c], float) else r[c])
                            for c in self._CSV])

    @staticmethod
    def rows_from_csv(path):
        """the rows `to_csv` wrote, as records"""
        out = []
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                macs = float(r["macs"])
                out.append(dict(key=r["key"], kind=r["kind"], klass=r["klass"], calls=int(r["calls"]),
                                macs=int(macs) if macs == int(macs) else macs, rate=float(r["rate"]) if r["rate"] else None,
                                sops=float(r["sops"]), off_share=float(r["off_share"]), energy_J=float(r["energy_J"]),
                                operands=json.loads(r["operands"])))
        return out

    def to_json(self):
        return json.dumps(dict(rows=self.rows, totals=self.totals, e_mac=self.e_mac, e_ac=self.e_ac, D=self.D, note=NOT_COUNTED))

    @classmethod
    def from_json(cls, text):
        d = json.loads(text)
        return cls(d["rows"], d["totals"]["params"], d["totals"]["passes"], d["e_mac"], d["e_ac"], d.get("D", 8))

    def totals_line(self):
        t = self.totals
        return (f"total: params {t['params'] / 1e6:.3f} M | MACs {t['macs'] / 1e9:.4f} G | real MACs {t['real_macs'] / 1e9:.4f} G | "
                f"SOPs {t['sops'] / 1e9:.4f} G | energy {t['energy_mJ']:.4f} mJ | passes {t['passes']}")

    def __str__(self):
        width = max([len(r["key"]) for r in self.rows] + [3])
        lines = [f"{'key':<{width}}  {'kind':<18} {'class':<5} {'calls':>6} {'MACs':>14} {'rate':>8} {'SOPs':>14} {'off-grid':>8} {'energy uJ':>10}"]
        for r in self.rows:
            rate = "" if r["rate"] is None else f"{r['rate']:.4f}"
            lines.append(f"{r['key']:<{width}}  {r['kind']:<18} {r['klass']:<5} {r['calls']:>6} {r['macs']:>14.6g} {rate:>8} {r['sops']:>14.6g} "
                         f"{r['off_share']:>8.4f} {1e6 * r['energy_J']:>10.4f}")
        lines.append(self.totals_line())
        lines.append(f"e_mac {self.e_mac:g} J, e_ac {self.e_ac:g} J, D {self.D}; {NOT_COUNTED}")
        return "\n".join(lines)


# ------------------------------------------------------------------------------------------------ the census
def _switches():
    from . import maskformer_head
    return ((maskformer_head, "FOLD_MASK_FEATURE", False), (maskformer_head, "PREDICT_LAST_ONLY", False))


class OpCensus:
    """Context manager: while it is live (and for at most `max_passes` forwards of `model`) every synaptic op of a forward reports
    itself to it; `report()` reads the device table back, once.  `D`: the level grid the operands are measured on; None: the D of
    the model's neurons (they must agree).  One census at a time."""

    def __init__(self, model, max_passes=100, D=None):
        if max_passes < 1:
            raise ValueError(f"OpCensus: max_passes {max_passes} below 1")
        self.model, self.max_passes = model, int(max_passes)
        if D is None:
            Ds = sorted({int(m.D) for m in model.modules() if isinstance(m, (Q_IFNode, LIFNode))})
            if len(Ds) > 1:
                raise ValueError(f"OpCensus: the model's neurons quantise to different D {Ds}: name the grid to measure on (D=...)")
            D = Ds[0] if Ds else 8
        self.D = int(D)
        p = next(model.parameters(), None)
        self.device = p.device if p is not None else torch.device("cpu")
        self.passes = 0
        self.records = OrderedDict()          # key -> {kind, calls, macs, operands: OrderedDict name -> [table row, spikes]}
        self._tables, self._used = [], 0
        self._stack, self._seen, self._live, self._entered = [], {}, False, False

    # ---- life cycle
    def __enter__(self):
        if ops.core._TAP[0] is not None:
            raise RuntimeError("OpCensus: another census is live")
        self._names = {id(m): n for n, m in self.model.named_modules()}
        # the state_dict keys by address: (first byte, one past the last byte, key), fp32 tensors only, sorted
        spans = {}
        for key, t in self.model.state_dict(keep_vars=True).items():
            if t.dtype == torch.float32 and t.numel() and t.is_contiguous():
                spans.setdefault(t.data_ptr(), (t.data_ptr(), t.data_ptr() + 4 * t.numel(), key))
        self._spans = sorted(spans.values())
        self._starts = [s[0] for s in self._spans]
        self._was_training = self.model.training
        self.model.eval()
        self._no_grad = torch.no_grad()
        self._no_grad.__enter__()
        self._entered = True
        self._activate()
        return self

    def __exit__(self, *exc):
        self._quiet()
        if self._entered:
            self._no_grad.__exit__(*exc)
            self.model.train(self._was_training)
            self._entered = False
        return False

    def _activate(self):
        from torch.nn.modules import module as _m
        self._saved = [(mod, name, getattr(mod, name)) for mod, name, _ in _switches()]
        for mod, name, value in _switches():
            setattr(mod, name, value)
        self._hooks = [_m.register_module_forward_pre_hook(self._enter_module),
                       _m.register_module_forward_hook(self._leave_module, always_call=True)]
        self._stack = []
        reset_net(self.model)          # (see _quiet)
        ops.core._TAP[0] = self
        self._live = True

    def _quiet(self):
        """taps off, switches back, hooks gone; what was counted stays"""
        if not self._live:
            return
        ops.core._TAP[0] = None
        for h in self._hooks:
            h.remove()
        for mod, name, value in self._saved:
            setattr(mod, name, value)
        # The switches change the shapes some neurons see (the SDME block's run over all L + 1 decoder layers in a census pass, over
        # the last one in a plain `predict`), and a neuron reads one kept membrane value per input element: no membrane crosses the
        # border between census passes and plain ones, in either direction.
        reset_net(self.model)
        self._live = False

    # ---- the module path
    def _enter_module(self, module, args):
        name = self._names.get(id(module))
        if name is None:
            return
        if module is self.model:
            self._stack, self._seen = [], {}
            if self.passes >= self.max_passes:
                self._quiet()
                return
            self.passes += 1
        self._stack.append(name)

    def _leave_module(self, module, args, output):
        if self._stack and self._names.get(id(module)) == self._stack[-1]:
            self._stack.pop()
            if not self._stack:
                self._seen = {}

    # ---- the tap (ops/core.py _TAP)
    def _row(self):
        if not self._tables or self._used == _TABLE_ROWS:
            self._tables.append(torch.zeros(_TABLE_ROWS, ops.CENSUS_FIELDS, dtype=torch.int64, device=self.device))
            self._used = 0
        self._used += 1
        return len(self._tables) - 1, self._used - 1

    def _owners(self, w):
        """-> [(state_dict key, first row of w it owns, rows)] when parameters of the model cover the weight w exactly, else None"""
        if w is None or not torch.is_tensor(w) or w.dtype != torch.float32 or not w.is_contiguous() or not w.numel():
            return None
        lo, hi = w.data_ptr(), w.data_ptr() + 4 * w.numel()
        per_row = 4 * (w.numel() // w.shape[0])
        i = max(bisect.bisect_right(self._starts, lo) - 1, 0)
        out, at = [], lo
        while i < len(self._spans) and self._spans[i][0] < hi:
            s, e, key = self._spans[i]
            i += 1
            if e <= lo:
                continue
            a, b = max(s, lo), min(e, hi)
            if a != at or (a - lo) % per_row or (b - lo) % per_row:
                return None
            out.append((key, (a - lo) // per_row, (b - a) // per_row))
            at = b
        return out if out and at == hi else None

    def __call__(self, kind, weight, macs, operands):
        owners = self._owners(weight)
        if owners is None:
            # (a module whose layers are run through a method of theirs, not their call, is the path of all of them: the second and
            #  later products of one kind under one path within a forward carry their ordinal)
            key = f"{self._stack[-1] if self._stack else ''}:{kind}"
            nth = self._seen[key] = self._seen.get(key, -1) + 1
            self._count(key if nth == 0 else f"{key}:{nth}", kind, int(macs), operands, None)
            return
        rows = weight.shape[0]
        for key, r0, n in owners:
            self._count(key, kind, int(macs) * n // rows, operands, None if n == rows else (r0, n, rows))

    def _count(self, key, kind, macs, operands, part):
        rec = self.records.get(key)
        if rec is None:
            rec = self.records[key] = dict(kind=kind, calls=0, macs=0, operands=OrderedDict())
        rec["calls"] += 1
        rec["macs"] += macs
        for op in operands:
            name, x = op[0], op[1]
            spikes = isinstance(x, ops.Spikes)
            data = x.data if spikes else x
            if len(op) > 2 and part is not None:          # this parameter's share of an operand that splits with the weight's rows
                size = data.shape[op[2]]
                data = data.narrow(op[2], part[0] * size // part[2], part[1] * size // part[2])
            if data.dtype not in (torch.float32, torch.bfloat16):
                data = data.float()
            if data.device != self.device:
                data = data.to(self.device)
            slot = rec["operands"].get(name)
            if slot is None:
                slot = rec["operands"][name] = [self._row(), spikes]
            slot[1] = slot[1] or spikes
            t, r = slot[0]
            ops.operand_census(data, self._tables[t][r], self.D)

    # ---- the result
    def report(self, e_mac=E_MAC, e_ac=E_AC):
        """-> EnergyReport: ONE read-back of the device table; rows average over the passes counted so far"""
        table = torch.cat(self._tables).cpu().tolist() if self._tables else []          # (the copy waits for the launches before it)
        if self.records and not self.passes:
            raise RuntimeError("OpCensus.report: ops reported themselves but no forward went through the model's call (model(...), "
                               "test_step, evaluate): a pass is counted there, and max_passes and the per-pass averages rest on it")
        passes = self.passes
        rows = []
        for key, rec in self.records.items():
            operands = []
            for name, ((t, r), spikes) in rec["operands"].items():
                v = table[t * _TABLE_ROWS + r]
                operands.append(dict(name=name, spikes=bool(spikes), **{f: int(v[i]) for i, f in enumerate(_FIELDS)}))
            macs = rec["macs"] // passes if rec["macs"] % passes == 0 else rec["macs"] / passes
            rows.append(dict(key=key, kind=rec["kind"], calls=rec["calls"], macs=macs, operands=operands))
        params = sum(p.numel() for _, p in self.model.named_parameters())
        return EnergyReport(rows, params, passes, e_mac, e_ac, self.D)
