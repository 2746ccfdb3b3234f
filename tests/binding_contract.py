"""The table behind tests/test_binding_contract_{gpu,cpu}.py and tests/test_binding_legal_gpu.py: one well-formed call of every
lsfa_amd/hip.py wrapper that hands a tensor to the library, at the smallest shapes it accepts, and the ways each tensor argument of it
can be wrong.

Nothing here launches a kernel by itself.  The refusal tests replace `hip.lib` by `Spy`, which forwards the exports of
test_abi.NO_KERNEL (host arithmetic, switches) to the real library and RECORDS every other export instead of calling it: a missing guard
shows as a recorded launch or a foreign exception, never as a bad access.

`Env` makes the tensors.  On a GPU they are real CUDA tensors.  On a machine without one (`Env(fake=True)`) they are host tensors of a
subclass that says `is_cuda` and `device == cuda:0`, and the allocations the wrappers make on "cuda:0" are redirected likewise, so that
a plain host tensor in ONE position meets well-formed neighbours in all others and every guard of a wrapper is reached, not only its
first."""
import contextlib
import re

import numpy as np
import torch

import test_abi
from lsfa_amd import hip

CUDA0 = torch.device("cuda", 0)
OTHER_DTYPE = {torch.float32: torch.float64, torch.float64: torch.float32, torch.int32: torch.int64, torch.uint8: torch.int64}


class FakeCuda(torch.Tensor):
    """a host tensor that claims to live on cuda:0 (see the module docstring); only attributes are faked, the memory is the host's"""
    is_cuda = True
    device = CUDA0

    def to(self, *args, **kw):
        """a move to the device it claims to be on already is no move (the two wrappers that move host tensors on purpose)"""
        target = kw.get("device", args[0] if args and isinstance(args[0], (str, torch.device)) else None)
        if target is not None and torch.device(target).type == "cuda":
            return self
        return super().to(*args, **kw)


def plain(t):
    """the host tensor behind a FakeCuda (or t)"""
    return t.as_subclass(torch.Tensor) if isinstance(t, FakeCuda) else t


# ---- the spy ----------------------------------------------------------------------------------------------------------------------------
def param_names(export):
    """the parameter names of an export as include/lsfa_hip.h spells them"""
    return [re.sub(r"[\[\]]", "", p.replace("*", " ").split()[-1]) for p in hip._PROTOTYPES[export][1]]


class Spy(object):
    """stands in for hip.lib(): NO_KERNEL exports go to the real library, everything else is recorded as (export, args) and answers 0"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in test_abi.NO_KERNEL:
            return getattr(self.real, name)
        if name not in hip._PROTOTYPES:
            raise AttributeError(name)

        def record(*args):
            assert len(args) == len(hip._PROTOTYPES[name][1]), "%s called with %d arguments" % (name, len(args))
            self.calls.append((name, args))
            return 0
        return record

    def launched(self):
        return [name for name, _ in self.calls]

    def values(self, export):
        """{parameter name: value} of the first recorded call of `export`; the fields of a lsfa_conv_desc under 'd'"""
        for name, args in self.calls:
            if name == export:
                out = dict(zip(param_names(export), args))
                if "d" in out and hasattr(out["d"], "_obj"):
                    out["d"] = {f: getattr(out["d"]._obj, f) for f, _ in hip.ConvDesc._fields_}
                return out
        raise AssertionError("%s was not reached; recorded: %s" % (export, self.launched()))


# ---- the environment --------------------------------------------------------------------------------------------------------------------
class Env(object):
    """makes the table's tensors: real CUDA tensors, or FakeCuda host tensors (fake=True)"""

    def __init__(self, fake):
        self.fake = fake
        self.rs = np.random.RandomState(1234)

    def dev(self, t):
        t = t.contiguous()
        return t.as_subclass(FakeCuda) if self.fake else t.to(CUDA0)

    def f32(self, *shape, lo=-1.0, hi=1.0):
        return self.dev(torch.from_numpy(self.rs.uniform(lo, hi, shape).astype(np.float32)))

    def i32(self, *shape, lo=0, hi=4):
        return self.dev(torch.from_numpy(self.rs.randint(lo, hi, shape).astype(np.int32)))

    def u8(self, *shape):
        return self.dev(torch.from_numpy(self.rs.randint(0, 256, shape).astype(np.uint8)))

    def rois(self, R, n_img, w, h):
        x1, y1 = self.rs.uniform(0, w / 2, R), self.rs.uniform(0, h / 2, R)
        r = np.stack([self.rs.randint(0, n_img, R), x1, y1, x1 + self.rs.uniform(4, w / 2, R), y1 + self.rs.uniform(4, h / 2, R)], 1)
        return self.dev(torch.from_numpy(r.astype(np.float32)))

    def amax(self):
        """a zeroed row of amax_slots() (made here: hip.amax_slots launches the zero fill)"""
        return self.dev(torch.zeros(hip.AMAX_SLOTS, dtype=torch.int32))

    def amax_in(self, bound=4.0):
        """amax_partial()'s float32 row for a map bounded by `bound`"""
        return self.dev(torch.full((hip.AMAX_SLOTS,), bound, dtype=torch.float32))

    def status(self):
        return self.dev(torch.zeros(4, dtype=torch.int32))

    def zeros(self, *shape, dtype=torch.float32):
        return self.dev(torch.zeros(shape, dtype=dtype))

    def host(self, t):
        """the CPU-tensor mutation of t"""
        return plain(t).detach().cpu().clone()

    def view_of_larger(self, t):
        """a non-contiguous view of t's shape and values inside a larger buffer"""
        p = plain(t)
        if p.dim() == 1:
            big = torch.zeros(2 * p.numel(), dtype=p.dtype)
            big[::2] = p
            v = self.dev(big)[::2]
        else:
            big = torch.zeros(tuple(p.shape[:-1]) + (p.shape[-1] + 1,), dtype=p.dtype)
            big[..., :-1] = p
            v = self.dev(big)[..., :-1]
            if v.is_contiguous():            # all leading dimensions 1: step over elements instead
                big = torch.zeros(tuple(p.shape[:-1]) + (2 * p.shape[-1],), dtype=p.dtype)
                big[..., ::2] = p
                v = self.dev(big)[..., ::2]
        assert tuple(v.shape) == tuple(t.shape) and not v.is_contiguous(), (tuple(t.shape), tuple(v.stride()))
        return v


@contextlib.contextmanager
def fake_cuda(monkeypatch):
    """what lets hip.py's wrappers run on a machine without a GPU up to the (recorded) launch: allocations on cuda:0 become FakeCuda host
    tensors, the current device is 0, torch.cuda.device() does nothing and the stream handle is 0"""
    def redirect(fn):
        def alloc(*args, **kw):
            d = kw.get("device")
            if d is not None and torch.device(d).type == "cuda":
                kw["device"] = "cpu"
                return fn(*args, **kw).as_subclass(FakeCuda)
            return fn(*args, **kw)
        return alloc
    with monkeypatch.context() as m:
        for name in ("empty", "zeros", "ones", "full"):
            m.setattr(torch, name, redirect(getattr(torch, name)))
        m.setattr(torch.cuda, "current_device", lambda: 0)
        m.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
        m.setattr(hip, "_stream", lambda: 0)
        yield


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
KINDS = ("cpu", "dtype", "noncontig", "short", "rank", "none")


class Arg(object):
    """One tensor argument of a row's call.  role: 'in' (read; a non-contiguous one may be copied), 'out' (written, or updated in
    place: never copied), 'vec' (read as so many consecutive values, whatever its shape).  short: the axis that loses one entry (None:
    every size is a legal call), or a function of the tensor.  rank: False where another rank of the same values is legal, "flat" where
    the transpose is (the mutation is then the flattened tensor).  optional:
    None is a legal value.  moved: a host tensor is moved to the device on purpose.  skip: {kind: reason}."""

    def __init__(self, role, short=0, rank=True, optional=False, moved=False, dtype=None, skip=None):
        self.role, self.short, self.rank, self.optional, self.moved, self.dtype, self.skip = role, short, rank, optional, moved, dtype, dict(skip or {})

    def kinds(self):
        for kind in KINDS:
            if kind in self.skip or (kind == "noncontig" and self.role != "out") or (kind == "short" and self.short is None) or \
                    (kind == "rank" and (self.role == "vec" or not self.rank)) or (kind == "none" and self.optional) or \
                    (kind == "cpu" and self.moved):
                continue
            yield kind


def I(**kw):
    return Arg("in", **kw)


def O(**kw):
    return Arg("out", **kw)


def V(**kw):
    kw.setdefault("short", "numel")
    return Arg("vec", **kw)


def get(kw, path):
    v = kw
    for k in (path if isinstance(path, tuple) else (path,)):
        v = v[k]
    return v


def put(kw, path, value):
    """kw with `value` at `path`; the tuples / lists on the way are rebuilt, the caller's stay as they are"""
    path = path if isinstance(path, tuple) else (path,)
    if len(path) == 1:
        if isinstance(kw, dict):
            out = dict(kw)
            out[path[0]] = value
            return out
        out = list(kw)
        out[path[0]] = value
        return type(kw)(out) if isinstance(kw, tuple) else out
    return put(kw, path[0], put(kw[path[0]], path[1:], value))


def mutate(env, arg, t, kind):
    p = plain(t)
    if kind == "cpu":
        return env.host(t)
    if kind == "dtype":
        return env.dev(p.to(arg.dtype or OTHER_DTYPE[p.dtype]))
    if kind == "noncontig":
        return env.view_of_larger(t)
    if kind == "short":
        if callable(arg.short):
            return env.dev(arg.short(p))
        if arg.short == "numel":
            return env.dev(p.reshape(-1)[:-1])
        return env.dev(p.narrow(arg.short, 0, p.shape[arg.short] - 1))
    if kind == "rank":
        if p.dim() == 2 and p.shape[0] != p.shape[1] and arg.rank != "flat":
            return env.dev(p.t())                       # (R, 5) as (5, R)
        return env.dev(p.reshape(1, -1) if p.dim() == 1 else p.reshape(-1))
    if kind == "none":
        return None
    raise KeyError(kind)


class Row(object):
    """name: the wrapper (Class.method for a method); make(env) -> (callable, kwargs); args: {path into kwargs: Arg}; expect: {export:
    {parameter: value}} of the well-formed call; cross: [(label, function(env, kwargs) -> kwargs)] mismatches between arguments;
    covers: private helpers of hip.py this row runs through; legal: False keeps the row out of the real-launch tests (it needs
    state the spy cannot give, or is covered by a sibling row)."""

    def __init__(self, name, make, args, expect, cross=(), covers=(), variant=None, legal=True):
        self.name, self.make, self.args, self.expect, self.cross, self.covers, self.variant, self.legal = \
            name, make, args, expect, list(cross), tuple(covers), variant, legal
        self.id = name + ("[%s]" % variant if variant else "")

    def cases(self):
        """(case id, path or None, kind or cross label)"""
        for path, arg in self.args.items():
            label = ".".join(str(k) for k in (path if isinstance(path, tuple) else (path,)))
            for kind in arg.kinds():
                yield "%s-%s-%s" % (self.id, label, kind), path, kind
        for label, _ in self.cross:
            yield "%s-cross-%s" % (self.id, label), None, label

    def mutated(self, env, kw, path, kind):
        if path is None:
            return dict(self.cross)[kind](env, kw)
        return put(kw, path, mutate(env, self.args[path], get(kw, path), kind))


def swap(path, fn):
    """a cross-argument case: kwargs with fn(env, tensor at path) at path"""
    return lambda env, kw: put(kw, path, fn(env, plain(get(kw, path))))


def grow(axis):
    """one more entry along `axis` (a repeat of the last)"""
    return lambda env, p: env.dev(torch.cat([p, p.narrow(axis, p.shape[axis] - 1, 1)], axis))


ROWS = []


def row(name, args, expect, **kw):
    def deco(make):
        ROWS.append(Row(name, make, args, expect, **kw))
        return make
    return deco


# R-FCN head ---------------------------------------------------------------------------------------------------------------------------------
@row("psroi_pool", {"data": I(short=None, skip={"short": "a map of any size is legal here; the C side checks C against output_dim * group^2"}),
                    "rois": I(short=1)},
     {"lsfa_psroi_pool_fwd": dict(N=2, C=18, H=5, W=7, R=3, output_dim=2, pooled_size=3, group_size=3)})
def _(env):
    return hip.psroi_pool, dict(data=env.f32(2, 18, 5, 7), rois=env.rois(3, 2, 7 * 16, 5 * 16), spatial_scale=0.0625, output_dim=2, pooled_size=3,
                                group_size=3)


@row("rfcn_head", {"cls_map": I(), "box_map": I(), "rois": I(short=1), ("out", 0): O(), ("out", 1): O(short=1)},
     {"lsfa_rfcn_head_fwd": dict(N=2, H=5, W=7, R=3, ncls=2, nbox=4, pooled_size=3, group_size=3)},
     cross=[("box_map-grid", swap("box_map", grow(2))), ("out-triple", lambda env, kw: put(kw, "out", tuple(kw["out"]) + (kw["out"][0],)))])
def _(env):
    return hip.rfcn_head, dict(cls_map=env.f32(2, 18, 5, 7), box_map=env.f32(2, 36, 5, 7), rois=env.rois(3, 2, 7 * 16, 5 * 16), spatial_scale=0.0625,
                               pooled_size=3, group_size=3, out=(env.zeros(3, 2), env.zeros(3, 4)))


@row("rfcn_head_ps", {"ps_map": I(short=4), "rois": I(short=1)},
     {"lsfa_rfcn_head_ps_fwd": dict(N=2, H=5, W=7, R=3, ncls=2, nbox=4)})
def _(env):
    return hip.rfcn_head_ps, dict(ps_map=env.f32(2, 5, 7, 9, 6), rois=env.rois(3, 2, 7 * 16, 5 * 16), ncls=2, nbox=4, pooled_size=3, group_size=3)


@row("rfcn_head_ps_ld", {"ps_map": I(short=3), "rois": I(short=1)},
     {"lsfa_rfcn_head_ps_ld_fwd": dict(cell_ld=56, N=2, H=5, W=7, R=3, ncls=2, nbox=4)})
def _(env):
    return hip.rfcn_head_ps_ld, dict(ps_map=env.f32(2, 5, 7, 56), cell_ld=56, rois=env.rois(3, 2, 7 * 16, 5 * 16), H=5, W=7, ncls=2, nbox=4,
                                     pooled_size=3, group_size=3)


# warp ---------------------------------------------------------------------------------------------------------------------------------------
def _warp_row(cl, bn):
    fn = hip.warp_bilinear_cl if cl else hip.warp_bilinear
    add = "add_cl" if cl else "add"
    feat = "feat_cl" if cl else "feat"
    args = {feat: I(short=3 if cl else 1), "flow": I(), add: I(optional=True), "res": I(optional=True), "res_w": V(), "res_b": V(), "out": O(optional=True)}
    if bn:
        args[("bn", 0)], args[("bn", 1)] = V(), V()
    elif not cl:
        args["mul"] = I(optional=True)
    if cl:
        args["amax_out"] = O(optional=True)
    export = "lsfa_warp_bilinear" + ("_bn" if bn else "") + ("_cl" if cl else "")

    def make(env):
        maps = (2, 5, 7, 8) if cl else (2, 8, 5, 7)
        kw = {feat: env.f32(*maps), "flow": env.f32(2, 2, 5, 7, lo=-2, hi=2), add: env.f32(*maps), "res": env.f32(2, 3, 5, 7),
              "res_w": env.f32(8, 3, 1, 1), "res_b": env.f32(8), "out": env.zeros(*maps)}
        if bn:
            kw["bn"] = (env.f32(8, lo=0.5, hi=1.5), env.f32(8))
        elif not cl:
            kw["mul"] = env.f32(*maps)
        if cl:
            kw["amax_out"], kw["amax_c0"] = env.amax(), 4
        return fn, kw
    cross = [("feat-grid", swap(feat, grow(1 if cl else 2))), ("res_w-without-res_b", lambda env, kw: put(kw, "res_b", None))]
    if bn:
        cross.append(("bn-single", lambda env, kw: put(kw, "bn", kw["bn"][0])))
    ROWS.append(Row(fn.__name__, make, args, {export: dict(feat_n=2, N=2, C=8, H=5, W=7, res_c=3)}, cross=cross, covers=("_warp",),
                    variant="bn" if bn else None))


for _cl in (False, True):
    for _bn in (False, True):
        _warp_row(_cl, _bn)


# gate ----------------------------------------------------------------------------------------------------------------------------------------
@row("channel_mean", {"x1": I(), "x2": I(optional=True), "out": O(optional=True, short=1)},
     {"lsfa_channel_mean": dict(C1=8, C2=4, N=2, HW=12)}, cross=[("x2-grid", swap("x2", grow(1)))])
def _(env):
    return hip.channel_mean, dict(x1=env.f32(2, 3, 4, 8), x2=env.f32(2, 3, 4, 4), out=env.zeros(2, 12))


@row("channel_gate", {"m": I(short=1), "w1": I(), "b1": V(), "w2": I(), "b2": V(), "out": O(optional=True, short=1)},
     {"lsfa_channel_gate": dict(N=2, K=8, M=12, O=5)})
def _(env):
    return hip.channel_gate, dict(m=env.f32(2, 8), w1=env.f32(12, 8), b1=env.f32(12), w2=env.f32(5, 12), b2=env.f32(5), out=env.zeros(2, 5))


@row("gate_apply", {"x": I(), "gate": I(short=1), "y": I(short=3), "out": O(optional=True), "amax_out": O(optional=True)},
     {"lsfa_gate_apply": dict(N=2, HW=12, C=8, amax_c0=4)})
def _(env):
    return hip.gate_apply, dict(x=env.f32(2, 3, 4, 8), gate=env.f32(2, 8, lo=0, hi=1), y=env.f32(2, 3, 4, 8), out=env.zeros(2, 3, 4, 8),
                                amax_out=env.amax(), amax_c0=4)


# aggregation ---------------------------------------------------------------------------------------------------------------------------------
def _softmax2_row(N, export, stride=None):
    args = {"a": I(short=1), "b": I(short=2), "logits": V(), "out": O(optional=True)}
    if stride:
        args["logits"] = V(skip={"short": "covered by the cross case: the buffer must hold the last row"})

    def make(env):
        kw = dict(a=env.f32(N, 8, 5, 7), b=env.f32(N, 8, 5, 7), logits=env.f32(2 * N, 1, 5, 7), out=env.zeros(N, 8, 5, 7))
        if stride:
            kw.update(logits=env.f32(2 * N, stride), logit_row_stride=stride)
        return hip.aggregate_softmax2, kw
    cross = [("b-batch", swap("b", grow(0)))]
    if stride:
        cross.append(("logits-last-row", swap("logits", lambda env, p: env.dev(p.reshape(-1)[:-(stride - 35) - 1]))))
    want = dict(C=8, H=5, W=7)
    if N > 1:
        want["N"] = N
    if stride:
        want["logit_row_stride"] = stride
    ROWS.append(Row("aggregate_softmax2", make, args, {export: want}, cross=cross, variant=export[len("lsfa_aggregate_softmax2"):] or "one"))


_softmax2_row(1, "lsfa_aggregate_softmax2")
_softmax2_row(2, "lsfa_aggregate_softmax2_batched")
_softmax2_row(2, "lsfa_aggregate_softmax2_rows", stride=40)


@row("aggregate_cosine", {"a": I(short=1), "b": I(short=2), "emb_warp": I(short=3), "emb_cur": I(short=1), "out": O(optional=True, short=1)},
     {"lsfa_aggregate_cosine": dict(C=8, E=6, H=5, W=7)},
     cross=[("batch-of-two", lambda env, kw: {k: (env.dev(torch.cat([plain(v), plain(v)], 0)) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})])
def _(env):
    return hip.aggregate_cosine, dict(a=env.f32(1, 8, 5, 7), b=env.f32(1, 8, 5, 7), emb_warp=env.f32(1, 6, 5, 7), emb_cur=env.f32(1, 6, 5, 7),
                                      out=env.zeros(1, 8, 5, 7))


# proposal, NMS, detection tail ---------------------------------------------------------------------------------------------------------------
@row("ProposalOp.__call__", {"cls_prob": I(short=1), "bbox_pred": I(short=1), "im_info": I(short=1), ("out", 0): O(), ("out", 1): O()},
     {"lsfa_proposal": dict(B=2, A=3, H=5, W=7, feature_stride=16, n_scales=1, n_ratios=3, rpn_pre_nms_top_n=50, rpn_post_nms_top_n=10)},
     cross=[("out-single", lambda env, kw: put(kw, "out", kw["out"][0]))])
def _(env):
    op = hip.ProposalOp(feature_stride=16, scales=(8,), ratios=(0.5, 1, 2), rpn_pre_nms_top_n=50, rpn_post_nms_top_n=10, rpn_min_size=4, output_score=True)
    im_info = env.dev(torch.tensor([[80.0, 112.0, 1.0], [80.0, 112.0, 1.0]]))
    return op, dict(cls_prob=env.f32(2, 6, 5, 7, lo=0, hi=1), bbox_pred=env.f32(2, 12, 5, 7, lo=-0.2, hi=0.2), im_info=im_info,
                    out=(env.zeros(20, 5), env.zeros(20, 1)))


@row("nms_sorted", {"boxes": I(short=None, rank="flat", skip={"short": "any number of boxes of any width >= 4 is legal"})}, {"lsfa_nms_sorted": dict(n=6, box_dim=5)})
def _(env):
    return hip.nms_sorted, dict(boxes=env.rois(6, 1, 64, 64), thresh=0.5)


@row("nms_sorted_f64", {"boxes": I(short=None, rank="flat", skip={"short": "any number of boxes of any width >= 4 is legal"})},
     {"lsfa_nms_sorted_f64": dict(n=6, box_dim=5)})
def _(env):
    return hip.nms_sorted_f64, dict(boxes=env.dev(plain(env.rois(6, 1, 64, 64)).double()), thresh=0.5)


@row("bbox_pred_clip", {"rois": I(short=1), "deltas": I()}, {"lsfa_bbox_pred_clip": dict(R=3, nreg=2)},
     cross=[("deltas-rows", swap("deltas", grow(0)))])
def _(env):
    return hip.bbox_pred_clip, dict(rois=env.rois(3, 1, 112, 80), deltas=env.f32(3, 8, lo=-0.2, hi=0.2), im_h=80, im_w=112, scale=1.0)


_DET_OUT = {("out", 0): O(), ("out", 1): O(), ("out", 2): O(short=1)}


@row("det_postprocess", {"rois": I(short=1), "deltas": I(), "probs": I(), **_DET_OUT},
     {"lsfa_det_postprocess": dict(R=3, ncls=4, nreg=2, class_agnostic=1, max_per_image=300)},
     cross=[("deltas-rows", swap("deltas", grow(0))), ("probs-rows", swap("probs", grow(0))), ("out-pair", lambda env, kw: put(kw, "out", tuple(kw["out"][:2])))])
def _(env):
    return hip.det_postprocess, dict(rois=env.rois(3, 1, 112, 80), deltas=env.f32(3, 8, lo=-0.2, hi=0.2), probs=env.f32(3, 4, lo=0, hi=1), im_h=80, im_w=112,
                                     scale=1.0, out=(env.zeros(4, 3, 5, dtype=torch.float64), env.zeros(4, dtype=torch.int32),
                                                     env.dev(torch.full((4, 3), -1, dtype=torch.int32))))


@row("det_postprocess_batch", {"rois": I(short=1), "deltas": I(), "probs": I(), **_DET_OUT},
     {"lsfa_det_postprocess_batch": dict(B=2, R=3, ncls=4, nreg=2, class_agnostic=1)},
     cross=[("probs-rows", swap("probs", grow(0))), ("out-none", lambda env, kw: put(kw, "out", None)), ("odd-batch", lambda env, kw: put(kw, "B", 4))])
def _(env):
    return hip.det_postprocess_batch, dict(rois=env.rois(6, 1, 112, 80), deltas=env.f32(6, 8, lo=-0.2, hi=0.2), probs=env.f32(6, 4, lo=0, hi=1), B=2,
                                           im_h=80, im_w=112, scale=1.0, out=(env.zeros(2, 4, 3, 5, dtype=torch.float64),
                                                                               env.zeros(2, 4, dtype=torch.int32),
                                                                               env.dev(torch.full((2, 4, 3), -1, dtype=torch.int32))))


@row("rpn_softmax_split", {"logits": I(short=lambda p: p[..., :17].contiguous())}, {"lsfa_rpn_softmax_split": dict(N=2, H=5, W=7, ld=64, A=3)})
def _(env):
    return hip.rpn_softmax_split, dict(logits=env.f32(2, 5, 7, 64), A=3)


# deformable im2col, affine + activation --------------------------------------------------------------------------------------------------------
@row("deform_im2col", {"data": I(), "offset": I(short=1), "out": O(optional=True, short=2)},
     {"lsfa_deform_im2col": dict(N=2, C=8, H=6, W=7, kh=3, kw=3, pad=1, stride=1, dilate=1, deform_groups=2, Ho=6, Wo=7)},
     cross=[("offset-grid", swap("offset", grow(2))), ("offset-batch", swap("offset", grow(0)))])
def _(env):
    return hip.deform_im2col, dict(data=env.f32(2, 8, 6, 7), offset=env.f32(2, 36, 6, 7, lo=-2, hi=2), kh=3, kw=3, pad=1, stride=1, dilate=1,
                                   deform_groups=2, out=env.zeros(2, 72, 42))


@row("deform_im2col_cl", {"data": I(), "offset": I(short=3), "out": O(optional=True, short=2)},
     {"lsfa_deform_im2col_cl_ld": dict(offset_ld=36, N=2, C=8, H=6, W=7, Ho=6, Wo=7)}, cross=[("offset-grid", swap("offset", grow(1)))])
def _(env):
    return hip.deform_im2col_cl, dict(data=env.f32(2, 6, 7, 8), offset=env.f32(2, 6, 7, 36, lo=-2, hi=2), kh=3, kw=3, pad=1, stride=1, dilate=1,
                                      deform_groups=2, out=env.zeros(2, 42, 72))


def _scale_shift_row(fn, export, cl, extra, want):
    def make(env):
        return fn, dict(dict(x=env.f32(*((2, 5, 7, 8) if cl else (2, 8, 5, 7))), scale=env.f32(8), shift=env.f32(8),
                             out=env.zeros(*((2, 5, 7, 8) if cl else (2, 8, 5, 7)))), **extra)
    ROWS.append(Row(fn.__name__, make, {"x": I(), "scale": V(), "shift": V(), "out": O(optional=True)}, {export: want}))


_scale_shift_row(hip.scale_shift_relu, "lsfa_scale_shift_relu", False, dict(relu=True), dict(N=2, C=8, HW=35, relu=1))
_scale_shift_row(hip.scale_shift_leaky, "lsfa_scale_shift_leaky", False, dict(slope=0.1), dict(N=2, C=8, HW=35))
_scale_shift_row(hip.scale_shift_relu_cl, "lsfa_scale_shift_relu_cl", True, dict(relu=True), dict(rows=70, C=8, relu=1))


# exact-fp32 convolution, copies, image transforms -----------------------------------------------------------------------------------------------
_CONV_OUT = dict(rank=False, skip={"rank": "the kernel writes N * Ho * Wo * Cout consecutive values: the element count is the contract"})


@row("conv_nhwc", {"x": I(short=3), "w_kc": I(short=1), "bias": V(optional=True), "out": O(optional=True, **_CONV_OUT), "residual": O(optional=True, **_CONV_OUT),
                   "out2": O(optional=True, **_CONV_OUT), "scale2": V(optional=True), "shift2": V(optional=True)},
     {"lsfa_conv_nhwc_fused_fwd": dict(N=1, H=5, W=6, Cin=32, Cout=64, kh=3, kw=3, stride=1, pad=1, dil=1, relu=1)})
def _(env):
    return hip.conv_nhwc, dict(x=env.f32(1, 5, 6, 32), w_kc=env.f32(64, 9, 32, lo=-0.1, hi=0.1), bias=env.f32(64), kh=3, kw=3, pad=1, relu=True,
                               out=env.zeros(1, 5, 6, 64), residual=env.f32(1, 5, 6, 64), out2=env.zeros(1, 5, 6, 64), scale2=env.f32(64), shift2=env.f32(64))


@row("copy_many", {("pairs", 0, 0): O(), ("pairs", 0, 1): I(optional=True), ("pairs", 1, 0): O(short=None, rank=False, skip={
        "short": "a zero fill of any size is legal", "rank": "a zero fill of any shape is legal"})},
     {"lsfa_copy_many": dict(njobs=2)})
def _(env):
    return hip.copy_many, dict(pairs=[(env.zeros(4, 8), env.f32(4, 8)), (env.i32(256, lo=1, hi=9), None)])


@row("transform_mv_res", {"motion_vector": I(short=2), "res_diff": I(short=2), ("out", 0): O(), ("out", 1): O()},
     {"lsfa_transform_mv_res": dict(H=64, W=80, h1=32, w1=40, rcnn_stride=16, out_h=2, out_w=3)},
     cross=[("res-grid", swap("res_diff", grow(0)))])
def _(env):
    return hip.transform_mv_res, dict(motion_vector=env.i32(64, 80, 2, lo=-8, hi=8), res_diff=env.i32(64, 80, 3, lo=-20, hi=20), im_scale=0.5,
                                      pixel_means=(1.0, 2.0, 3.0), rcnn_stride=16, out=(env.zeros(1, 2, 2, 3), env.zeros(1, 3, 2, 3)))


@row("image_resize_transform", {"im": I(short=3, dtype=torch.int64)}, {"lsfa_image_resize_transform": dict(is_u8=1, N=2, H=16, W=20, h1=8, w1=10)})
def _(env):
    return hip.image_resize_transform, dict(im=env.u8(2, 16, 20, 3), im_scale=0.5, pixel_means=(1.0, 2.0, 3.0))


@row("image_transform_u8", {"im": I(short=3), "out": O(optional=True)}, {"lsfa_image_transform_u8": dict(N=2, H=4, W=8)})
def _(env):
    return hip.image_transform_u8, dict(im=env.u8(2, 4, 8, 3), pixel_means=(1.0, 2.0, 3.0), out=env.zeros(2, 3, 4, 8))


def _yuv_row(fn, export, i420, out_shape, out_dtype, extra, want):
    planes = {"u": I(), "v": I()} if i420 else {"uv": I()}
    args = dict({"y": I(), "out": O(optional=True)}, **planes)
    if fn is hip.yuv420_to_bgr_u8:
        args["y_packed"] = O(optional=True)

    def make(env):
        kw = dict(y=env.u8(2, 6, 10), out=env.zeros(*out_shape, dtype=out_dtype), **extra)
        kw.update(dict(u=env.u8(2, 3, 5), v=env.u8(2, 3, 5)) if i420 else dict(uv=env.u8(2, 3, 10)))
        if fn is hip.yuv420_to_bgr_u8:
            kw["y_packed"] = env.zeros(2, 6, 10, dtype=torch.uint8)
        return fn, kw
    cross = [("both-layouts", lambda env, kw: dict(kw, uv=env.u8(2, 3, 10), u=env.u8(2, 3, 5), v=env.u8(2, 3, 5)))]
    ROWS.append(Row(fn.__name__, make, args, {export: dict(dict(N=2, H=6, W=10, y_pitch=10, y_frame_stride=60), **want)}, cross=cross,
                    variant="i420" if i420 else "nv12"))


for _i420 in (False, True):
    _yuv_row(hip.yuv420_to_bgr_u8, "lsfa_yuv420_to_bgr_u8", _i420, (2, 6, 10, 3), torch.uint8, {}, {})
    _yuv_row(hip.image_transform_yuv420, "lsfa_image_transform_yuv420", _i420, (2, 3, 6, 10), torch.float32, dict(pixel_means=(1.0, 2.0, 3.0)), {})
    _yuv_row(hip.image_resize_transform_yuv420, "lsfa_image_resize_transform_yuv420", _i420, (2, 3, 3, 5), torch.float32, dict(im_scale=0.5),
             dict(h1=3, w1=5, out_h=3, out_w=5))


# stem, pools, FlowNet's small kernels -------------------------------------------------------------------------------------------------------------
@row("ImageTable.set", {("images", 0): I(), ("images", 1): I(short=2)}, {"lsfa_ptr_table_set": dict(n=2)},
     cross=[("one-image", lambda env, kw: put(kw, "images", kw["images"][:1]))])
def _(env):
    return hip.ImageTable(2, 3, 4, 8, CUDA0).set, dict(images=[env.f32(3, 4, 8), env.f32(3, 4, 8)])


def _table(env, n, c, h, w):
    return hip.ImageTable(n, c, h, w, CUDA0).set([env.f32(c, h, w, lo=0, hi=255) for _ in range(n)])


@row("avgpool_nchw", {"x": I(), "out": O(optional=True, short=3)}, {"lsfa_avgpool_nchw": dict(N=2, C=3, H=5, W=7, k=2)})
def _(env):
    return hip.avgpool_nchw, dict(x=env.f32(2, 3, 5, 7), k=2, out=env.zeros(2, 3, 3, 4))


@row("avgpool_nchw", {"out": O(optional=True, short=3)}, {"lsfa_avgpool_nchw_tbl": dict(N=2, C=3, H=5, W=7, k=2)}, variant="table")
def _(env):
    return hip.avgpool_nchw, dict(x=_table(env, 2, 3, 5, 7), k=2, out=env.zeros(2, 3, 3, 4))


@row("stem_weight_layout", {"weight": I(short=1, dtype=torch.int64)}, {"lsfa_stem_weights": {}})
def _(env):
    return hip.stem_weight_layout, dict(weight=env.f32(64, 3, 7, 7, lo=-0.1, hi=0.1))


_STEM_ARGS = {"w_l": I(), "bias": V(optional=True), "in_scale": V(optional=True), "in_shift": V(optional=True), "out": O(optional=True),
              "accum": O(optional=True), "amax_out": O(optional=True)}


def _stem_kw(env, x):
    w_l = hip.stem_weight_layout(env.f32(64, 3, 7, 7, lo=-0.1, hi=0.1))      # (under the spy: right size, no layout)
    return dict(x=x, w_l=w_l, bias=env.f32(64), in_scale=env.f32(3, lo=0.5, hi=1.5), in_shift=env.f32(3), out=env.zeros(2, 5, 6, 64),
                accum=env.f32(2, 5, 6, 64), act=2, amax_out=env.amax())


@row("stem_conv", dict({"x": I(short=1)}, **_STEM_ARGS), {"lsfa_stem_conv7x7s2_ex": dict(N=2, H=9, W=11, act=2)})
def _(env):
    return hip.stem_conv, _stem_kw(env, env.f32(2, 3, 9, 11))


@row("stem_conv", dict(_STEM_ARGS), {"lsfa_stem_conv7x7s2_tbl": dict(N=2, H=9, W=11, act=2)}, variant="table")
def _(env):
    return hip.stem_conv, _stem_kw(env, _table(env, 2, 3, 9, 11))


def _head_row(nchw):
    def make(env):
        kw = dict(x=env.f32(2, 5, 7, 8), w=env.f32(2, 3, 3, 8), bias=env.f32(2), mul=2.5, nchw=nchw)
        kw.update(dict(out=env.zeros(2, 2, 5, 7)) if nchw else dict(out=env.zeros(2, 5, 7, 4), c0=1))
        return hip.head_conv3x3, kw
    cross = [] if nchw else [("c0-past-out", lambda env, kw: put(kw, "c0", 3))]
    ROWS.append(Row("head_conv3x3", make, {"x": I(), "w": I(), "bias": V(optional=True), "out": O(optional=True)},
                    {"lsfa_head_conv3x3": dict(lda=8, N=2, H=5, W=7, Cin=8, Cout=2, out_nchw=int(nchw), ldy=0 if nchw else 4, c0=0 if nchw else 1)},
                    cross=cross, variant="nchw" if nchw else "slice"))


_head_row(False)
_head_row(True)


@row("upsample_flow", {"x": I(short=3), "w": I(), "bias": V(optional=True), "out": O(), "amax_out": O(optional=True)},
     {"lsfa_upsample_flow": dict(N=2, Hi=3, Wi=4, C=2, Hc=6, Wc=8, ldy=4, c0=1)}, cross=[("c0-past-out", lambda env, kw: put(kw, "c0", 3))])
def _(env):
    return hip.upsample_flow, dict(x=env.f32(2, 3, 4, 2), w=env.f32(2, 2, 4, 4), bias=env.f32(2), out=env.zeros(2, 6, 8, 4), c0=1, amax_out=env.amax())


@row("nchw_to_nhwc", {"x": I(), "out": O(optional=True), "amax_out": O(optional=True)},
     {"lsfa_nchw_to_nhwc": dict(N=2, Ctot=8, HW=35, c0=4, C=4)}, cross=[("channels-past-map", lambda env, kw: put(kw, "c0", 5))])
def _(env):
    return hip.nchw_to_nhwc, dict(x=env.f32(2, 8, 5, 7), c0=4, c=4, out=env.zeros(2, 5, 7, 4), amax_out=env.amax())


@row("avgpool2_nhwc", {"x": I(short=None, skip={"short": "a map of any size is legal"})}, {"lsfa_avgpool2_nhwc": dict(N=2, H=5, W=7, C=8)})
def _(env):
    return hip.avgpool2_nhwc, dict(x=env.f32(2, 5, 7, 8))


@row("maxpool3x3s2_nhwc", {"x": I(), "out": O(optional=True), "scale2": V(optional=True), "shift2": V(optional=True), "amax_out": O(optional=True)},
     {"lsfa_maxpool3x3s2_nhwc": dict(N=2, H=5, W=7, C=8)}, cross=[("scale2-alone", lambda env, kw: put(kw, "shift2", None))])
def _(env):
    return hip.maxpool3x3s2_nhwc, dict(x=env.f32(2, 5, 7, 8), out=env.zeros(2, 3, 4, 8), scale2=env.f32(8), shift2=env.f32(8), amax_out=env.amax())


# split convolutions -----------------------------------------------------------------------------------------------------------------------------
def _sw(env, cout, cin, k, pieces):
    """a SplitWeight (its layout launch goes wherever hip.lib() points: recorded under the spy, real in the launch tests)"""
    return hip.SplitWeight(env.f32(cout, cin, k, k, lo=-0.1, hi=0.1), pieces=pieces)


def _split_weight_row(pieces, export, want):
    def make(env):
        need = int(hip.lib().lsfa_conv_weight_bytes(64, 3, 3, 32, pieces))
        return hip.SplitWeight, dict(weight=env.f32(64, 32, 3, 3, lo=-0.1, hi=0.1), into=env.zeros(need, dtype=torch.uint8), pieces=pieces)
    ROWS.append(Row("SplitWeight.__init__", make, {"weight": I(), "into": O(optional=True)}, {export: dict(dict(Cout=64, kh=3, kw=3, Cin=32), **want)},
                    variant="%d-pieces" % pieces, legal=False))


_split_weight_row(3, "lsfa_conv_weights", dict(pieces=3, w_exp=0))
_split_weight_row(2, "lsfa_conv_weights_pc", {})


@row("amax_partial", {"x": I(short=None, rank=False, skip={"short": "any size is legal", "rank": "any shape is legal"}), "out": O(optional=True)},
     {"lsfa_amax_partial": dict(n=16)})
def _(env):
    return hip.amax_partial, dict(x=env.f32(2, 8), out=env.zeros(hip.AMAX_SLOTS))


@row("check_status", {"status": O()}, {"lsfa_status_check": {}})
def _(env):
    return hip.check_status, dict(status=env.status())


_CONV_TAIL = {"bias": V(optional=True), "amax_in": O(optional=True), "amax_out": O(optional=True), "status": O(optional=True)}


@row("conv_split", dict({"x": I(short=3), "out": O(optional=True, **_CONV_OUT), "residual": O(optional=True, **_CONV_OUT),
                         "out2": O(optional=True, **_CONV_OUT), "scale2": V(optional=True), "shift2": V(optional=True)}, **_CONV_TAIL),
     {"lsfa_conv_fwd": dict(d=dict(N=1, H=5, W=6, Cin=32, Cout=64, kh=3, kw=3, pad_h=1, pad_w=1, lda=32, ldy=64, act=1, pieces=3))},
     covers=("_conv_launch",), cross=[("sw-none", lambda env, kw: put(kw, "sw", None))])
def _(env):
    return hip.conv_split, dict(x=env.f32(1, 5, 6, 32), sw=_sw(env, 64, 32, 3, 3), bias=env.f32(64), pad=1, relu=True, out=env.zeros(1, 5, 6, 64),
                                residual=env.f32(1, 5, 6, 64), out2=env.zeros(1, 5, 6, 64), scale2=env.f32(64), shift2=env.f32(64),
                                amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())


@row("conv_split", {"x": I(short=3), "in_scale": V(optional=True), "in_shift": V(optional=True), "bias": V(optional=True)},
     {"lsfa_conv_fwd": dict(d=dict(N=1, H=5, W=6, Cin=32, Cout=64, kh=1, kw=1, pieces=1))}, variant="input-activation", covers=("_conv_launch",))
def _(env):
    return hip.conv_split, dict(x=env.f32(1, 5, 6, 32), sw=_sw(env, 64, 32, 1, 1), bias=env.f32(64), in_scale=env.f32(32, lo=0.5, hi=1.5), in_shift=env.f32(32))


@row("conv_split", {"x": I(short=3), "bias": V(optional=True), "out": O(optional=True, **_CONV_OUT)},
     {"lsfa_conv_nhwc_fused_fwd": dict(N=1, H=5, W=6, Cin=32, Cout=64, kh=3, kw=3, pad=1)}, variant="exact", covers=("_conv_exact",))
def _(env):
    return hip.conv_split, dict(x=env.f32(1, 5, 6, 32), sw=_sw(env, 64, 32, 3, 0), bias=env.f32(64), pad=1, out=env.zeros(1, 5, 6, 64))


@row("conv_pair", {"x": I(short=3), "residual": O(**_CONV_OUT), "scale2": V(), "shift2": V(), "bias": V(optional=True), "out": O(optional=True, **_CONV_OUT),
                   "out_z": O(optional=True, **_CONV_OUT), "amax_in": O(optional=True), "amax_out_sum": O(optional=True), "amax_out_z": O(optional=True),
                   "status": O(optional=True)},
     {"lsfa_conv_pair_fwd": dict(ldx=64, N=1, H=3, W=4, Cm=64, pieces3=2, C=256, ldy=256, pieces1=2, Cn=64, ldz=64, stride=1, y_nchw=0)},
     cross=[("sw3-none", lambda env, kw: put(kw, "sw3", None))])
def _(env):
    return hip.conv_pair, dict(x=env.f32(1, 3, 4, 64), sw3=_sw(env, 256, 64, 1, 2), residual=env.f32(1, 3, 4, 256), scale2=env.f32(256, lo=0.5, hi=1.5),
                               shift2=env.f32(256), sw1=_sw(env, 64, 256, 1, 2), bias=env.f32(64), out=env.zeros(1, 3, 4, 256), out_z=env.zeros(1, 3, 4, 64),
                               amax_in=env.amax_in(), amax_out_sum=env.amax(), amax_out_z=env.amax(), status=env.status())


@row("conv_split_view", dict({"x": I(short=3), "out": O(short=3)}, **_CONV_TAIL),
     {"lsfa_conv_fwd": dict(d=dict(N=1, H=5, W=6, Cin=32, Cout=64, lda=64, ldy=128, Ho=5, Wo=6, act=2))}, covers=("_conv_launch",))
def _(env):
    return hip.conv_split_view, dict(x=env.f32(1, 5, 6, 64), sw=_sw(env, 64, 32, 3, 3), bias=env.f32(64), out=env.zeros(1, 5, 6, 128), pad=(1, 1), act=2,
                                     c0=64, cin0=32, amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())


@row("deconv_phase_weights", {"wt": I(short=2)}, {"lsfa_conv_weights": dict(Cout=64, kh=2, kw=2, Cin=32, pieces=3)}, legal=False)
def _(env):
    return hip.deconv_phase_weights, dict(wt=env.f32(32, 64, 4, 4, lo=-0.1, hi=0.1))


@row("deconv4x4s2_crop", dict({"x": I(short=3), "out": O(short=3)}, **_CONV_TAIL),
     {"lsfa_deconv4x4s2_crop_fwd": dict(lda=32, N=1, Hi=3, Wi=4, Cin=32, pieces=3, Cout=64, act=2, ldy=128, Hc=6, Wc=8)},
     cross=[("sw4-a-list", lambda env, kw: put(kw, "sw4", list(kw["sw4"])))])
def _(env):
    return hip.deconv4x4s2_crop, dict(x=env.f32(1, 3, 4, 32), sw4=hip.deconv_phase_weights(env.f32(32, 64, 4, 4, lo=-0.1, hi=0.1)), bias=env.f32(64),
                                      out=env.zeros(1, 6, 8, 128), c0=64, act=2, amax_in=env.amax_in(), amax_out=env.amax(), status=env.status())


# motion front end ---------------------------------------------------------------------------------------------------------------------------------
def _mvs(env, n):
    m = np.zeros((n, 7), np.int32)
    m[:, 0], m[:, 1], m[:, 2] = -1, 16, 16
    m[:, 3], m[:, 5] = 16 * (np.arange(n) % 2), 16 * (np.arange(n) % 2)
    return env.dev(torch.from_numpy(m))


@row("MotionVectorAccumulator.add_frame", {"mvs": I(short=1, moved=True)}, {"lsfa_mv_accumulate": dict(n_mvs=2, max_block_area=256, width=32, height=16)})
def _(env):
    return hip.MotionVectorAccumulator(32, 16, CUDA0).add_frame, dict(mvs=_mvs(env, 2), max_block_area=256)


@row("MotionVectorAccumulator.motion_vectors", {"out": O(optional=True)}, {"lsfa_mv_field": dict(width=32, height=16)})
def _(env):
    return hip.MotionVectorAccumulator(32, 16, CUDA0).motion_vectors, dict(out=env.zeros(16, 32, 2, dtype=torch.int32))


@row("MotionVectorAccumulator.residual", {"bgr_cur": I(moved=True), "bgr_ref": I(short=1, moved=True), "out": O(optional=True)},
     {"lsfa_mv_residual": dict(width=32, height=16)})
def _(env):
    return hip.MotionVectorAccumulator(32, 16, CUDA0).residual, dict(bgr_cur=env.u8(16, 32, 3), bgr_ref=env.u8(16, 32, 3), out=env.zeros(16, 32, 3, dtype=torch.int32))


@row("luma_u8", {"bgr": I(), "out": O(optional=True)}, {"lsfa_luma_u8": dict(width=32, height=16)})
def _(env):
    return hip.luma_u8, dict(bgr=env.u8(16, 32, 3), out=env.zeros(16, 32, dtype=torch.uint8))


@row("mv_estimate", {"luma_cur": I(), "luma_ref": I(short=1), "out": O(optional=True), "sad_out": O(optional=True, short=1)},
     {"lsfa_mv_estimate": dict(width=32, height=16, search=4)})
def _(env):
    return hip.mv_estimate, dict(luma_cur=env.u8(16, 32), luma_ref=env.u8(16, 32), search=4, return_sad=True, out=env.zeros(2, 7, dtype=torch.int32),
                                 sad_out=env.zeros(1, 2, dtype=torch.int32))


@row("mv_estimate_chain", {"luma_stack": I(short=1), "out": O(optional=True, short=2), "sad_out": O(optional=True, short=3)},
     {"lsfa_mv_estimate_chain": dict(plane_stride=512, n_chains=1, n_frames=2, width=32, height=16, search=4)})
def _(env):
    return hip.mv_estimate_chain, dict(luma_stack=env.u8(1, 3, 16, 32), search=4, return_sad=True, out=env.zeros(1, 2, 2, 7, dtype=torch.int32),
                                       sad_out=env.zeros(1, 2, 1, 2, dtype=torch.int32))


@row("luma_pyramid", {"luma": I(), ("out", 0): O(short=2)}, {"lsfa_luma_pyramid": dict(plane_stride=512, n_planes=2, width=32, height=16, levels=1, stride1=128)},
     cross=[("out-two-levels", lambda env, kw: put(kw, "out", list(kw["out"]) * 2))])
def _(env):
    return hip.luma_pyramid, dict(luma=env.u8(2, 16, 32), levels=1, out=[env.zeros(2, 8, 16, dtype=torch.uint8)])


@row("mv_refine_chain", {"luma_stack": I(short=1), "parent_rows": I(short=2), "out": O(optional=True, short=2), "sad_out": O(optional=True, short=3)},
     {"lsfa_mv_refine_chain": dict(n_chains=1, n_frames=2, width=48, height=32, refine=2)})
def _(env):
    return hip.mv_refine_chain, dict(luma_stack=env.u8(1, 3, 32, 48), parent_rows=env.dev(plain(_mvs(env, 2)).repeat(2, 1).view(1, 2, 2, 7).clone()),
                                     return_sad=True, out=env.zeros(1, 2, 6, 7, dtype=torch.int32), sad_out=env.zeros(1, 2, 2, 3, dtype=torch.int32))


@row("mv_cut_score", {"luma_stack": I(short=1), "sad": I(short=3), ("out", 0): O(short=3), ("out", 1): O(short=1)},
     {"lsfa_mv_cut_score": dict(n_chains=1, n_frames=2, width=32, height=16, bias=4)})
def _(env):
    return hip.mv_cut_score, dict(luma_stack=env.u8(1, 3, 16, 32), sad=env.i32(1, 2, 1, 2, hi=4000), out=(env.zeros(1, 2, 1, 2, dtype=torch.int32),
                                                                                                        env.zeros(1, 2, dtype=torch.int32)))


@row("mv_segment_inputs", {"rows": I(short=2), "bgr_stack": I(short=1), ("out", 0): O(), ("out", 1): O()},
     {"lsfa_mv_segment_inputs": dict(n_chains=1, n_frames=2, width=32, height=16, h1=16, w1=32, rcnn_stride=16, out_h=1, out_w=2)})
def _(env):
    return hip.mv_segment_inputs, dict(rows=env.dev(plain(_mvs(env, 2)).repeat(2, 1).view(1, 2, 2, 7).clone()), bgr_stack=env.u8(1, 3, 16, 32, 3), im_scale=1.0,
                                       out=(env.zeros(2, 1, 2, 1, 2), env.zeros(2, 1, 3, 1, 2)))


def _estimator(env, keyed=False, **kw):
    me = hip.MotionEstimator(32, 16, CUDA0, search=4, **kw)
    if keyed:
        me.key_frame(env.u8(16, 32, 3))
    return me


@row("MotionEstimator.key_frame", {"bgr": I()}, {"lsfa_luma_u8": dict(width=32, height=16), "lsfa_mv_identity": dict(width=32, height=16)})
def _(env):
    return _estimator(env).key_frame, dict(bgr=env.u8(16, 32, 3))


@row("MotionEstimator.next_frame", {"bgr": I()}, {"lsfa_mv_estimate": dict(width=32, height=16, search=4), "lsfa_mv_accumulate": dict(n_mvs=2)})
def _(env):
    return _estimator(env, keyed=True).next_frame, dict(bgr=env.u8(16, 32, 3))


@row("MotionEstimator.key_frame_yuv", {"y": I(), "uv": I()}, {"lsfa_yuv420_to_bgr_u8": dict(N=1, H=16, W=32), "lsfa_mv_identity": {}})
def _(env):
    return _estimator(env).key_frame_yuv, dict(y=env.u8(16, 32), uv=env.u8(8, 32))


@row("MotionEstimator.next_frame_yuv", {"y": I(), "uv": I()}, {"lsfa_yuv420_to_bgr_u8": dict(N=1, H=16, W=32), "lsfa_mv_estimate": dict(width=32, height=16)})
def _(env):
    return _estimator(env, keyed=True).next_frame_yuv, dict(y=env.u8(16, 32), uv=env.u8(8, 32))


@row("MotionEstimator.network_inputs", {"bgr_cur": I(), "bgr_key": I(short=1)},
     {"lsfa_mv_field": {}, "lsfa_mv_residual": {}, "lsfa_transform_mv_res": dict(H=16, W=32, out_h=1, out_w=2)})
def _(env):
    return _estimator(env, keyed=True).network_inputs, dict(bgr_cur=env.u8(16, 32, 3), bgr_key=env.u8(16, 32, 3), im_scale=1.0)


@row("SegmentMotionEstimator.segment", {"bgr_stack": I(short=2), ("out", 0): O(), ("out", 1): O()},
     {"lsfa_luma_u8": {}, "lsfa_mv_estimate_chain": dict(n_chains=1, n_frames=2, width=32, height=16), "lsfa_mv_segment_inputs": dict(n_frames=2, out_h=1, out_w=2)})
def _(env):
    return hip.SegmentMotionEstimator(32, 16, frames=2, device=CUDA0, search=4).segment, dict(
        bgr_stack=env.u8(1, 3, 16, 32, 3), im_scale=1.0, out=(env.zeros(2, 1, 2, 1, 2), env.zeros(2, 1, 3, 1, 2)))


@row("SegmentMotionEstimator.segment_yuv", {"y": I(short=1), "uv": I(), ("out", 0): O(), ("out", 1): O()},
     {"lsfa_yuv420_to_bgr_u8": dict(N=3, H=16, W=32), "lsfa_mv_estimate_chain": dict(n_frames=2), "lsfa_mv_segment_inputs": dict(n_frames=2)})
def _(env):
    return hip.SegmentMotionEstimator(32, 16, frames=2, device=CUDA0, search=4).segment_yuv, dict(
        y=env.u8(3, 16, 32), uv=env.u8(3, 8, 32), im_scale=1.0, out=(env.zeros(2, 1, 2, 1, 2), env.zeros(2, 1, 3, 1, 2)))


# ---- completeness -------------------------------------------------------------------------------------------------------------------------
# wrappers of hip.py that name a launching export and have no row.  The two acceptable reasons: it takes no tensor from the caller; it is
# a class whose own methods are in the table.  This dict may not grow to make a test pass.
EXEMPT = {
    "nms_host": "takes no tensor from the caller: host numpy arrays in, a host list out",
    "prof_read": "takes no tensor from the caller: host arrays of its own",
    "conv_by_kernel": "takes no tensor from the caller: reads the counters",
    "_count_launch": "takes no tensor from the caller: numbers",
    "_plan_kernel_name": "takes no tensor from the caller: a descriptor its callers built from checked tensors",
    "_parse_header": "takes no tensor from the caller: reads the header",
    "_zeros": "takes no tensor from the caller: allocates its own from a shape",
    "_MotionSearch": "takes no tensor from the caller: its methods take counts and write buffers of its own",
    "ImageTable": "a class whose own methods are in the table",
    "MotionEstimator": "a class whose own methods are in the table",
    "MotionVectorAccumulator": "a class whose own methods are in the table",
    "ProposalOp": "a class whose own methods are in the table",
    "SegmentMotionEstimator": "a class whose own methods are in the table",
    "SplitWeight": "a class whose own methods are in the table",
}
# the methods of those classes that take no tensor (everything else public must have a row)
TENSORLESS_METHODS = {
    "ImageTable": {"dim", "contiguous", "is_contiguous", "materialize"},
    "MotionEstimator": {"is_cut", "bgr_cur"},
    "MotionVectorAccumulator": {"reset", "accu", "network_inputs"},      # network_inputs: motion_vectors + residual + transform_mv_res, all in the table
    "ProposalOp": set(),
    "SegmentMotionEstimator": {"first_cuts"},
    "SplitWeight": set(),
}


def launching_exports():
    return sorted(set(test_abi.declared_symbols()) - set(test_abi.NO_KERNEL))


def wrappers_of_launching_exports():
    by_export, out = test_abi.wrappers_by_export(), set()
    for sym in launching_exports():
        out |= by_export.get(sym, set())
    return out


def covered():
    names = set()
    for r in ROWS:
        names.add(r.name.split(".")[0] if "." in r.name else r.name)
        names.add(r.name)
        names |= set(r.covers)
    return names


ALL_CASES = [(r, cid, path, kind) for r in ROWS for cid, path, kind in r.cases()]
CPU_CASES = [c for c in ALL_CASES if c[3] == "cpu"]


def run_well_formed(env, spy, r):
    """the row's call as it stands -> the spy's record of it (the launches of building the call's objects are not part of it)"""
    fn, kw = r.make(env)
    del spy.calls[:]
    fn(**kw)
    return kw


def check_expect(spy, r):
    for export, want in r.expect.items():
        got = spy.values(export)
        for name, value in want.items():
            if isinstance(value, dict):
                sub = {k: got[name][k] for k in value}
                assert sub == value, "%s: %s.%s = %s, expected %s" % (r.id, export, name, sub, value)
            else:
                assert got[name] == value, "%s: %s(%s = %r), expected %r" % (r.id, export, name, got[name], value)


def run_refusal(env, spy, r, path, kind):
    """-> None if the mutated call raised LsfaError with nothing launched, else a one-line description of what happened instead"""
    fn, kw = r.make(env)
    bad = r.mutated(env, kw, path, kind)
    del spy.calls[:]
    try:
        fn(**bad)
    except hip.LsfaError as e:
        if spy.calls:
            return "LsfaError (%s) only after launching %s" % (e, spy.launched())
        return None
    except Exception as e:      # noqa: BLE001 - the point: anything but LsfaError is a finding
        return "%s: %s%s" % (type(e).__name__, e, " after launching %s" % spy.launched() if spy.calls else "")
    return "no error; launched %s" % spy.launched()


# launching exports that some wrapper names and no row's well-formed call expects: named in a docstring only, or reached as one of
# several launches of a row whose `expect` lists the others
REACHED_ONLY_INDIRECTLY = {
    "lsfa_stem_conv7x7s2": "named by stem_weight_layout's docstring; hip.stem_conv calls its _ex and _tbl forms, which have rows",
}
