"""Memory ownership: every tensor of a call lies between two bands of a fixed byte pattern, so that a store outside a tensor changes a
band and a read outside it changes the result.  Used by tests/test_memory_ownership_{cpu,gpu}.py.

Nothing here launches a library kernel.  `Arena` places a tensor as the contiguous middle of a larger uint8 allocation of its own,
`GuardedEnv` makes the tensors of tests/binding_contract.py that way, and `guarded_allocations` redirects the allocations lsfa_amd/hip.py
makes itself (torch.empty / zeros / ones / full and the `_like` forms it uses; it uses no `Tensor.new_*`).  `run_guarded` puts the three
together around one row of the table.

Two patterns are needed.  0xFF reads as NaN (float32 / float64), -1 (int32) and 255 (uint8); 0x7F reads as 3.39e38 (float32, finite)
and 2139062143 (int32).  A reduction that ignores NaN (every fmaxf, every comparison that is false for NaN, the amax rows) takes a
stray 0xFF word in silently and a stray 0x7F word visibly.

What this cannot see: a read outside a tensor whose value the kernel then masks away, and tensors a wrapper makes by other means
(`.contiguous()` copies of views, `.to()` moves).  Every byte the harness touches lies inside its own allocations; it never builds a
pointer outside them."""
import contextlib

import pytest
import torch

import binding_contract as bc
from lsfa_amd import hip

MIN_BAND = 64 * 1024
ALIGN = 256
PATTERNS = (0xFF, 0x7F)

# the real constructors, whatever a test has put in their place by the time a tensor is placed
_FULL, _EMPTY = torch.full, torch.empty


def _round_up(n, a):
    return -(-n // a) * a


class Placed(object):
    """one tensor of the arena: bytes [start, start + nbytes) of `buf`; everything else of `buf` is band"""

    def __init__(self, role, tensor, buf, start, nbytes):
        self.role, self.tensor, self.buf, self.start, self.nbytes = role, tensor, buf, start, nbytes

    def __str__(self):
        return "%s %s %s" % (self.role, tuple(self.tensor.shape), self.tensor.dtype)


class Arena(object):
    """fake=True: on the host, and the tensors claim cuda:0 (binding_contract.FakeCuda)"""

    def __init__(self, pattern_byte, device=bc.CUDA0, fake=False):
        assert 0 <= int(pattern_byte) <= 255
        self.pattern, self.fake = int(pattern_byte), fake
        self.device = torch.device("cpu") if fake else torch.device(device)
        self.placed = []

    def place(self, shape, dtype, role, values=None, fill=None):
        """a contiguous `dtype` tensor of `shape`, starting on a 256-byte boundary, with a band of max(64 KiB, its own size) rounded up
        to 256 bytes on either side.  values: a tensor to copy in; fill: a number to fill with; neither: the middle holds the pattern."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _EMPTY((), dtype=dtype, device="meta").element_size()
        band = _round_up(max(MIN_BAND, nbytes), ALIGN)
        buf = _FULL((band + ALIGN + nbytes + band,), self.pattern, dtype=torch.uint8, device=self.device)
        start = band + (-(buf.data_ptr() + band)) % ALIGN
        t = buf[start:start + nbytes].view(dtype).view(shape)
        assert t.is_contiguous() and (numel == 0 or t.data_ptr() % ALIGN == 0) and start >= band and buf.numel() - start - nbytes >= band
        if values is not None:
            t.copy_(bc.plain(values))
        elif fill is not None:
            t.fill_(fill)
        if self.fake:
            t = t.as_subclass(bc.FakeCuda)
        self.placed.append(Placed(role, t, buf, start, nbytes))
        return t

    def record(self, t):
        """the Placed of a tensor this arena made (None for any other tensor)"""
        for p in self.placed:
            if p.tensor is t or (p.nbytes and isinstance(t, torch.Tensor) and t.data_ptr() == p.tensor.data_ptr() and t.dtype == p.tensor.dtype):
                return p
        return None

    def name(self, t, role):
        p = self.record(t)
        if p is not None:
            p.role = role

    def changed(self):
        """[(Placed, 'start' or 'end', offset in bytes of the first changed byte from there, number of changed bytes)]"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self.placed:
            return []
        sides = [(p, p.buf[:p.start], p.buf[p.start + p.nbytes:]) for p in self.placed]
        flags = torch.stack([torch.stack([(front != self.pattern).any(), (back != self.pattern).any()]) for _, front, back in sides]).cpu()
        out = []
        for (p, front, back), (f, b) in zip(sides, flags.tolist()):
            if f:
                idx = (front != self.pattern).nonzero().view(-1)
                out.append((p, "start", int(idx[0]) - p.start, int(idx.numel())))
            if b:
                idx = (back != self.pattern).nonzero().view(-1)
                out.append((p, "end", int(idx[0]), int(idx.numel())))
        return out

    def check(self):
        """every band still holds the pattern in every byte"""
        bad = self.changed()
        assert not bad, "stores outside a tensor (pattern 0x%02X): " % self.pattern + "; ".join(
            "%s: %d byte(s) changed, the first at %+d bytes from its %s" % (p, count, off, side) for p, side, off, count in bad)


class GuardedEnv(bc.Env):
    """binding_contract.Env (the same seed, so the same values) whose tensors lie in `arena`"""

    def __init__(self, arena):
        bc.Env.__init__(self, fake=arena.fake)
        self.arena = arena

    def dev(self, t):
        t = bc.plain(t).contiguous()
        return self.arena.place(t.shape, t.dtype, "table tensor #%d" % len(self.arena.placed), values=t)


def _on_cuda(d):
    return d is not None and torch.device(d).type == "cuda"


@contextlib.contextmanager
def guarded_allocations(monkeypatch, arena):
    """Inside: torch.empty / zeros / ones / full for a CUDA device, and torch.empty_like / zeros_like of a CUDA tensor, give tensors of
    `arena` (contiguous).  `empty` keeps the pattern in its middle; the others hold what was asked for.  CPU and pinned allocations, and
    everything else, pass through untouched."""
    fills = {"empty": lambda a, kw: None, "zeros": lambda a, kw: 0, "ones": lambda a, kw: 1,
             "full": lambda a, kw: kw["fill_value"] if "fill_value" in kw else a[1]}

    def by_device(name, fn):
        def alloc(*args, **kw):
            if not _on_cuda(kw.get("device")) or kw.get("pin_memory") or kw.get("out") is not None:
                return fn(*args, **kw)
            proto = fn(*args, **dict(kw, device="meta"))
            return arena.place(proto.shape, proto.dtype, "torch.%s" % name, fill=fills[name](args, kw))
        return alloc

    def like(name, fn):
        def alloc(t, *args, **kw):
            d = kw.get("device")
            if not (_on_cuda(d) if d is not None else isinstance(t, torch.Tensor) and t.is_cuda):
                return fn(t, *args, **kw)
            return arena.place(t.shape, kw.get("dtype") or t.dtype, "torch.%s" % name, fill=0 if name == "zeros_like" else None)
        return alloc

    with monkeypatch.context() as m:
        for name in fills:
            m.setattr(torch, name, by_device(name, getattr(torch, name)))
        for name in ("empty_like", "zeros_like"):
            m.setattr(torch, name, like(name, getattr(torch, name)))
        yield arena


# ---- one row of the table ---------------------------------------------------------------------------------------------------------------
def tensors(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, (tuple, list)):
        return [t for e in v for t in tensors(e)]
    if isinstance(v, dict):
        return [t for e in v.values() for t in tensors(e)]
    return []


def everything(row, kw, ret):
    """what a call returned and every tensor it was given (an input must come back as it went in), each once"""
    out = []
    for t in tensors(ret) + tensors(kw):
        if not any(t is o for o in out):
            out.append(t)
    return out


def _label(arena, v, path):
    if isinstance(v, torch.Tensor):
        arena.name(v, path)
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            _label(arena, e, "%s[%d]" % (path, i))
    elif isinstance(v, dict):
        for k, e in v.items():
            _label(arena, e, "%s.%s" % (path, k) if path else str(k))


def host(ts):
    return [bc.plain(t).detach().cpu().clone() for t in ts]


def run_plain(row, defined=everything, fake=False):
    """the row's call on ordinary tensors -> its defined results on the host"""
    fn, kw = row.make(bc.Env(fake=fake))
    ret = fn(**kw)
    if kw.get("status") is not None and not fake:
        hip.check_status(kw["status"])
    return host(defined(row, kw, ret))


def run_guarded(row, pattern, defined=everything, fake=False):
    """the row's call with every tensor in an Arena(pattern): a fresh GuardedEnv, `row.make` and the call inside guarded_allocations
    (objects that allocate in __init__ are covered), then arena.check() -> the defined results on the host"""
    arena = Arena(pattern, fake=fake)
    env = GuardedEnv(arena)
    with pytest.MonkeyPatch.context() as mp, guarded_allocations(mp, arena):
        fn, kw = row.make(env)
        _label(arena, kw, "")
        ret = fn(**kw)
        if kw.get("status") is not None and not fake:
            hip.check_status(kw["status"])
        out = host(defined(row, kw, ret))
    arena.check()
    return out


def same(a, b):
    """two lists of host tensors are equal in number, dtype, shape and every value"""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))
