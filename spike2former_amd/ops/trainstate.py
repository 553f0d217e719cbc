"""The launches a training loop adds to the captured step: `state_copy`, every tensor of a pointer table into one flat buffer or
back, and `train_log_append`, one row of per-iteration scalars into a ring on the device (csrc/trainstate.hip); `firing_log_append`,
one row of per-neuron firing counters into a ring of its own (csrc/firinglog.hip).  CUDA tensors run the kernels on the current
stream; CPU tensors run the same semantics in torch (the package's CPU implementation of these three ops, as the numpy route of
`seg_draw`), so the classes of runner.py and firing.py can be driven without a GPU.  `grad_log_table` / `grad_log_append`: one row
of per-parameter gradient, weight and update norms behind the optimizer's update (csrc/gradlog.hip), HIP only -- the kernels read
the parameters through device pointers."""
import torch

from .core import STAT_SLOTS, _ptr, _stream, check, lib

TRAIN_LOG_MAX_TERMS = 256          # include/s2f.h S2F_TRAIN_LOG_MAX_TERMS


def _words(t):
    """a contiguous tensor of 4- or 8-byte elements as its flat int32 bit view (shares the storage)"""
    if t.element_size() % 4 != 0:
        raise TypeError(f"state_copy moves 32-bit words: a {t.dtype} tensor has {t.element_size()}-byte elements")
    if not t.is_contiguous():
        raise RuntimeError("state_copy: tensors must be contiguous")
    return t.detach().reshape(-1).view(torch.int32)


def state_table(tensors, device=None):
    """-> (slots int64 [n][3], chunks int32 [nchunks][2], words): the tables of s2f_state_copy over `tensors` (contiguous, 4- or
    8-byte elements, at least one element in all), on `device` (default: the tensors'), and the length of the flat int32 buffer they
    address.  Slot offsets are multiples of 4 words: every slot of a 16-byte-aligned flat buffer is 16-byte aligned; the words
    between two slots are pads that no copy writes.  Empty tensors get a slot and no chunk."""
    tensors = list(tensors)
    chunk = int(lib.s2f_adamw_chunk_elems())
    slots, chunks, off = [], [], 0
    for i, t in enumerate(tensors):
        n = _words(t).numel()
        slots.append((t.data_ptr(), off, n))
        chunks += [(i, s) for s in range(0, n, chunk)]
        off += (n + 3) // 4 * 4
    if not chunks:
        raise ValueError("state_table: nothing to copy")
    device = tensors[0].device if device is None else device
    return (torch.tensor(slots, dtype=torch.int64).reshape(-1, 3).to(device), torch.tensor(chunks, dtype=torch.int32).to(device), off)


def state_copy(tensors, slots, chunks, flat, to_params=False):
    """Every tensor of the table <-> its slot of `flat` (int32, contiguous, 16-byte aligned) in ONE launch: tensors -> flat, or
    (`to_params`) flat -> tensors.  Bits, not values: NaN payloads, denormals and int64 counters pass unchanged; pad words of `flat`
    are not written.  `slots`, `chunks`: `state_table(tensors)` -- the kernel reads the pointers baked into `slots` (rebuild the
    table when a tensor's storage moves); `tensors` itself is read by the CPU route only.  Nothing synchronises; capturable."""
    if flat.dtype != torch.int32 or not flat.is_contiguous():
        raise ValueError("state_copy: flat is one contiguous int32 buffer")
    if slots.dtype != torch.int64 or chunks.dtype != torch.int32 or slots.dim() != 2 or slots.shape[1] != 3 or chunks.dim() != 2 \
            or chunks.shape[1] != 2 or not (slots.is_contiguous() and chunks.is_contiguous()):
        raise ValueError("state_copy: slots is a contiguous int64 [n, 3], chunks a contiguous int32 [nchunks, 2] (state_table)")
    if slots.device != flat.device or chunks.device != flat.device:
        raise RuntimeError(f"state_copy: tables on {slots.device} / {chunks.device}, flat on {flat.device}")
    if not flat.is_cuda:
        tensors = list(tensors)
        if len(tensors) != slots.shape[0]:
            raise ValueError(f"state_copy: {len(tensors)} tensors for a table of {slots.shape[0]} slots")
        for t, (_, off, n) in zip(tensors, slots.tolist()):
            w = _words(t)
            if w.numel() != n or off + n > flat.numel():
                raise ValueError("state_copy: the table does not describe these tensors")
            if to_params:
                w.copy_(flat[off:off + n])
            else:
                flat[off:off + n].copy_(w)
        return flat
    check(lib.s2f_state_copy(_ptr(slots), _ptr(chunks), chunks.shape[0], _ptr(flat), int(bool(to_params)), _stream()), "s2f_state_copy")
    return flat


def train_log_table(srcs, device=None):
    """-> int64 [n] on `device`: the addresses of the fp32 scalars `srcs` (one-element CUDA tensors that outlive the table's use:
    static tensors of a captured step), the `table` of `train_log_append`.  One host-to-device copy: build it once, outside a capture."""
    srcs = list(srcs)
    for t in srcs:
        if t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError(f"train_log_append records fp32 scalars; got {t.dtype} {tuple(t.shape)}")
    device = srcs[0].device if device is None else device
    return torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64).to(device)


def train_log_append(srcs, ring, head, table=None, n=None):
    """Row head[0] % window of `ring` (fp32 [window, stride]) <- the scalars `srcs`; a non-finite value among them latches head[1]
    (int64 [2] = {rows appended, first row with a non-finite value or -1}); head[0] += 1.  One launch of one wave on the current
    stream, capturable: the CUDA route reads the scalars through `table` (`train_log_table(srcs)`; built here, with a host-to-device
    copy, when not given -- not under capture) and may be called with `srcs=None` and the count `n` of the table's entries in use.
    Columns n .. stride - 1 of the row are not written."""
    if ring.dtype != torch.float32 or ring.dim() != 2 or not ring.is_contiguous():
        raise ValueError("train_log_append: ring is a contiguous fp32 [window, stride]")
    if head.dtype != torch.int64 or tuple(head.shape) != (2,) or not head.is_contiguous() or head.device != ring.device:
        raise ValueError("train_log_append: head is a contiguous int64 [2] on the ring's device")
    window, stride = ring.shape
    n = len(srcs) if n is None else int(n)
    if not 1 <= n <= TRAIN_LOG_MAX_TERMS or stride < n or window < 1:
        raise ValueError(f"train_log_append: {n} terms (1 .. {TRAIN_LOG_MAX_TERMS}) into a ring of {window} rows of {stride}")
    if not ring.is_cuda:
        count = int(head[0])
        vals = torch.stack([t.detach().reshape(()).to(torch.float32) for t in srcs])
        ring[count % window, :n] = vals
        if int(head[1]) < 0 and not bool(torch.isfinite(vals).all()):
            head[1] = count
        head[0] = count + 1
        return ring
    if table is None:
        table = train_log_table(srcs, ring.device)
    if table.dtype != torch.int64 or table.dim() != 1 or table.numel() < n or table.device != ring.device or not table.is_contiguous():
        raise ValueError(f"train_log_append: table is a contiguous int64 [>= {n}] on the ring's device")
    check(lib.s2f_train_log_append(_ptr(table), n, _ptr(ring), window, stride, _ptr(head), _stream()), "s2f_train_log_append")
    return ring


def firing_log_append(counters, ring, silent, head, patience):
    """One row of firing counters (s2f_firing_log_append).  counters: int64 [n, STAT_SLOTS, 2], ONE contiguous allocation whose
    slice i is neuron i's `stats`; ring: int64 [window, n, 2]; silent: int32 [n]; head: int64 [4], the head of devring.py.  Per
    neuron: {sum of counts, non-zero counts} over the slots -> ring[head[0] % window, i]; the counters are cleared; silent[i] == -1
    (not watched) stays, otherwise it counts the rows in a row whose sum was 0; the first neuron whose streak reaches `patience` is
    latched in head[1] (the lowest index of the earliest row).  head[0] += 1.  One launch on the current stream; capturable."""
    if counters.dtype != torch.int64 or counters.dim() != 3 or tuple(counters.shape[1:]) != (STAT_SLOTS, 2) or not counters.is_contiguous():
        raise ValueError(f"firing_log_append: counters is a contiguous int64 [n, {STAT_SLOTS}, 2]")
    n = counters.shape[0]
    if ring.dtype != torch.int64 or ring.dim() != 3 or tuple(ring.shape[1:]) != (n, 2) or not ring.is_contiguous():
        raise ValueError(f"firing_log_append: ring is a contiguous int64 [window, {n}, 2]")
    if silent.dtype != torch.int32 or tuple(silent.shape) != (n,) or not silent.is_contiguous():
        raise ValueError(f"firing_log_append: silent is a contiguous int32 [{n}]")
    if head.dtype != torch.int64 or tuple(head.shape) != (4,) or not head.is_contiguous():
        raise ValueError("firing_log_append: head is a contiguous int64 [4]")
    if not (ring.device == silent.device == head.device == counters.device):
        raise RuntimeError("firing_log_append: counters, ring, silent and head live on one device")
    window, patience = ring.shape[0], int(patience)
    if n < 1 or window < 1 or patience < 1:
        raise ValueError(f"firing_log_append: {n} neurons, a ring of {window} rows, patience {patience}: each is at least 1")
    if not counters.is_cuda:
        count = int(head[0])
        sums = counters.sum(1)
        ring[count % window] = sums
        counters.zero_()
        watched = silent != -1
        streak = torch.where(sums[:, 0] == 0, silent + 1, torch.zeros_like(silent))
        silent.copy_(torch.where(watched, streak, silent))
        dead = torch.nonzero(watched & (silent == patience))
        if dead.numel():
            event, mask = (count << 32) | int(dead[0]), (1 << 64) - 1
            if event & mask < int(head[1]) & mask:          # the minimum under unsigned comparison: -1 is the largest
                head[1] = event
        head[0] = count + 1
        return ring
    check(lib.s2f_firing_log_append(_ptr(counters), n, _ptr(ring), window, _ptr(silent), patience, _ptr(head), _stream()),
          "s2f_firing_log_append")
    return ring


def grad_log_table(slots):
    """-> spans int32 [nspans, 2] = {slot, first element} on the slots' device: every parameter of `slots` (int64 [n, 3] = {parameter
    pointer, offset in the flat buffers, numel}: `FlatAdamW.slots`) in runs of at most s2f_grad_log_span_elems() elements, sorted by
    slot -- the workgroups of s2f_grad_log_partials.  A parameter without elements gets no span.  One device-to-host and one
    host-to-device copy: build it once, outside a capture, and again when the slot table is rebuilt."""
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 3 or not slots.is_contiguous():
        raise ValueError("grad_log_table: slots is a contiguous int64 [n, 3]")
    span = int(lib.s2f_grad_log_span_elems())
    spans = [(i, s) for i, (_, _, n) in enumerate(slots.tolist()) for s in range(0, n, span)]
    if not spans:
        raise ValueError("grad_log_table: no parameter has an element")
    return torch.tensor(spans, dtype=torch.int32).reshape(-1, 2).to(slots.device)


def grad_log_append(slots, spans, hyper, state, flat, exp_avg, exp_avg_sq, partials, ring, streak, head, eps, patience):
    """One row of per-parameter gradient figures (s2f_grad_log_partials -> s2f_grad_log_rows), behind s2f_adamw_step.  slots int64
    [n, 3], hyper fp32 [n, 2], state fp32 [>= 5], flat / exp_avg / exp_avg_sq fp32 flat buffers of one length: FlatAdamW's, after the
    update; spans: `grad_log_table(slots)`; partials int64 [nspans, 8] (workspace); ring int64 [window, n, 8]; streak int32 [n, 2];
    head int64 [4], the head of devring.py: head[1] latches the first stalled parameter, head[3] the first with a non-finite
    gradient element.  Row head[0] % window <- per parameter {sum g^2, sum p^2, sum u^2, max |g| as doubles'
    bits; g == 0, non-finite g, non-finite p or u, numel} (include/s2f.h "gradient log"); head[0] += 1.  Two launches on the current
    stream, no synchronisation, capturable; everything but partials, ring, streak and head is only read.  HIP only: CPU tensors
    raise."""
    if slots.dtype != torch.int64 or slots.dim() != 2 or slots.shape[1] != 3 or not slots.is_contiguous():
        raise ValueError("grad_log_append: slots is a contiguous int64 [n, 3]")
    n = slots.shape[0]
    if spans.dtype != torch.int32 or spans.dim() != 2 or spans.shape[1] != 2 or not spans.is_contiguous():
        raise ValueError("grad_log_append: spans is a contiguous int32 [nspans, 2] (grad_log_table)")
    nspans = spans.shape[0]
    if hyper.dtype != torch.float32 or tuple(hyper.shape) != (n, 2) or not hyper.is_contiguous():
        raise ValueError(f"grad_log_append: hyper is a contiguous fp32 [{n}, 2]")
    if state.dtype != torch.float32 or state.dim() != 1 or state.numel() < 5 or not state.is_contiguous():
        raise ValueError("grad_log_append: state is a contiguous fp32 [>= 5]")
    for name, t in (("flat", flat), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() != flat.numel():
            raise ValueError(f"grad_log_append: {name} is a contiguous fp32 [{flat.numel()}]")
    if partials.dtype != torch.int64 or tuple(partials.shape) != (nspans, 8) or not partials.is_contiguous():
        raise ValueError(f"grad_log_append: partials is a contiguous int64 [{nspans}, 8]")
    if ring.dtype != torch.int64 or ring.dim() != 3 or tuple(ring.shape[1:]) != (n, 8) or not ring.is_contiguous():
        raise ValueError(f"grad_log_append: ring is a contiguous int64 [window, {n}, 8]")
    if streak.dtype != torch.int32 or tuple(streak.shape) != (n, 2) or not streak.is_contiguous():
        raise ValueError(f"grad_log_append: streak is a contiguous int32 [{n}, 2]")
    if head.dtype != torch.int64 or tuple(head.shape) != (4,) or not head.is_contiguous():
        raise ValueError("grad_log_append: head is a contiguous int64 [4]")
    if any(t.device != slots.device for t in (spans, hyper, state, flat, exp_avg, exp_avg_sq, partials, ring, streak, head)):
        raise RuntimeError("grad_log_append: every tensor lives on the slot table's device")
    window, patience = ring.shape[0], int(patience)
    if n < 1 or nspans < 1 or window < 1 or patience < 1:
        raise ValueError(f"grad_log_append: {n} parameters in {nspans} spans, a ring of {window} rows, patience {patience}: each is "
                         "at least 1")
    if not slots.is_cuda:
        raise RuntimeError("grad_log_append: the gradient log is two HIP launches over device pointers; there is no CPU route")
    s = _stream()
    check(lib.s2f_grad_log_partials(_ptr(slots), _ptr(hyper), _ptr(spans), nspans, _ptr(flat), _ptr(exp_avg), _ptr(exp_avg_sq),
                                    _ptr(state), float(eps), _ptr(partials), s), "s2f_grad_log_partials")
    check(lib.s2f_grad_log_rows(_ptr(spans), nspans, _ptr(partials), n, _ptr(ring), window, _ptr(streak), patience, _ptr(head), s),
          "s2f_grad_log_rows")
    return ring


__all__ = ["TRAIN_LOG_MAX_TERMS", "state_table", "state_copy", "train_log_table", "train_log_append", "firing_log_append",
           "grad_log_table", "grad_log_append"]
