"""ctypes binding of liblsfa_hip.so (the C ABI in include/lsfa_hip.h) on torch tensors.

PyTorch is plumbing here: it owns device memory and streams; every op below hands
raw device pointers and torch's CURRENT stream to the C ABI.  There is no CPU or
eager fallback — if the library is missing or a call fails, LsfaError is raised
(the counterpart of MXNetError in the reference).
"""
import ctypes
import math
import os
import re

import numpy as np
import torch  # must be imported before the .so so that both share one libamdhip64

from lsfa_amd import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
# LSFA_HIP_LIBRARY: another build of the same library (tools/lab/drop_product_check.sh runs the parity suite against a deliberately
# degraded one to show that the suite notices); there is no fallback either way
LIB_PATH = os.environ.get("LSFA_HIP_LIBRARY") or os.path.join(_HERE, "liblsfa_hip.so")

# names of the LSFA_OP_* ids, in id order.  The table is the LIBRARY's (lsfa_op_name) — filled in by lib(); this copy only serves
# code that runs before the library is loaded and is checked against it there (an out-of-date copy made lsfa_prof_read write one
# element past the buffers sized by it: r3, after LSFA_OP_FLOWNET was added)
OP_NAMES = ["psroi_pool", "rfcn_head", "warp_bilinear", "aggregate", "proposal", "nms", "det_postprocess",
            "deform_im2col", "scale_shift_relu", "conv_nhwc", "stem", "flownet_small", "mv_estimate"]


class LsfaError(RuntimeError):
    pass


_lib = None
_WARP_VARIANTS = {'auto': 0, 'gather': 1, 'staged': 2}       # lsfa_warp_set_variant

# ---- the ABI, as include/lsfa_hip.h states it ---------------------------------------------------------------------------------------------
# The header is the one statement of the C ABI on this side too: `ConvDesc` is built from its struct and lib() gives every export the
# restype / argtypes of its prototype, so a call with a missing argument, a float for an int or a size_t read as an int is refused by
# ctypes instead of reaching the library.  Call sites pass plain Python values; None is NULL.
_HEADER = os.path.join(_build.INCLUDE, "lsfa_hip.h")
_C_TYPES = {"void": None, "int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
            "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}


def _ctype(decl, named=True):
    """ctypes type of one declaration of the header: a parameter or struct field (`named`) or a return type.  Pointers are c_void_p
    but for a returned const char* and a const lsfa_conv_desc*; a scalar type outside _C_TYPES is an error."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if named:
        words.pop()
    if "*" in words:
        if words == ["char", "*"] and not named:
            return ctypes.c_char_p
        return ctypes.POINTER(ConvDesc) if words == ["lsfa_conv_desc", "*"] else ctypes.c_void_p
    if " ".join(words) not in _C_TYPES or (named and words == ["void"]):
        raise LsfaError("%s: no ctypes type for %r; extend _C_TYPES in lsfa_amd/hip.py" % (_HEADER, decl))
    return _C_TYPES[" ".join(words)]


def _parse_header():
    """-> (the fields of struct lsfa_conv_desc as ctypes _fields_, {export: (return type, [parameter, ...])} as the header spells them)"""
    try:
        text = open(_HEADER).read()
    except OSError as e:
        raise LsfaError("the binding is derived from %s, which cannot be read (%s); there is no fallback" % (_HEADER, e))
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    struct = re.search(r"struct\s+lsfa_conv_desc\s*\{(.*?)\}", text, flags=re.S)
    if not struct:
        raise LsfaError("%s does not define struct lsfa_conv_desc" % _HEADER)
    fields = []
    for stmt in filter(str.strip, struct.group(1).split(";")):
        first, *more = [d.strip() for d in stmt.split(",")]          # `int N, H, W, Cin`: one type, several declarators
        if more and "*" in stmt:
            raise LsfaError("%s: pointer fields are declared one by one: %r" % (_HEADER, stmt.strip()))
        fields += [(name, _ctype(first)) for name in [first.replace("*", " ").split()[-1]] + more]
    protos = {m.group(2): (m.group(1), [] if m.group(3).strip() == "void" else m.group(3).split(","))
              for m in re.finditer(r"([\w\s*]+?)\b(lsfa_\w+|_nms)\s*\(([^()]*)\)\s*;", text)}
    return fields, protos


_CONV_DESC_FIELDS, _PROTOTYPES = _parse_header()


class ConvDesc(ctypes.Structure):
    """struct lsfa_conv_desc (include/lsfa_hip.h), field for field"""
    _fields_ = _CONV_DESC_FIELDS


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            # not a fallback: build the real library if the toolchain is here, else fail loudly
            try:
                _build.build_hip()
            except Exception as e:
                raise LsfaError("liblsfa_hip.so is not built (%s) and building it failed (%r); run "
                                "`python -m lsfa_amd.build` — there is no fallback path" % (LIB_PATH, e))
        L = ctypes.CDLL(LIB_PATH)
        for name, (ret, params) in _PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _ctype(ret, named=False), [_ctype(p) for p in params]
        names, i = [], 0
        while True:
            nm = L.lsfa_op_name(i)
            if not nm or nm == b"?" or i >= 64:          # "?" is what the library returns past the last id
                break
            names.append(nm.decode())
            i += 1
        if names != OP_NAMES:
            OP_NAMES[:] = names              # in place: importers of the list see the library's table
        wv = os.environ.get("LSFA_WARP_VARIANT")         # A/B runs of whole programs: 'gather' | 'staged' | 'auto'
        if wv:
            if wv not in _WARP_VARIANTS:
                raise LsfaError("LSFA_WARP_VARIANT=%r: expected one of %s" % (wv, sorted(_WARP_VARIANTS)))
            L.lsfa_warp_set_variant(_WARP_VARIANTS[wv])
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise LsfaError("%s failed (code %d): %s" % (what, rc, lib().lsfa_last_error().decode()))


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tensor(who, what, t, dtype, shape, device=None):
    """t, if it is a contiguous `dtype` tensor of `shape` (a string stands for an axis of any size) on `device` (None: any CUDA device);
    else an LsfaError that names what arrived"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != len(shape) or not (t.is_cuda if device is None else t.device == device) or \
            any(not isinstance(w, str) and int(v) != w for v, w in zip(t.shape, shape)) or not t.is_contiguous():
        raise LsfaError("%s: %s must be a contiguous (%s) %s tensor on %s, got %s %s on %s" %
                        (who, what, ", ".join(str(w) for w in shape), dtype, device or "a CUDA device", tuple(getattr(t, 'shape', ())),
                         getattr(t, 'dtype', type(t)), getattr(t, 'device', None)))
    return t


def _arrived(t):
    return "%s %s on %s" % (tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t).__name__), getattr(t, 'device', None))


def _input(who, what, t, shape, device=None, dtype=torch.float32):
    """An operand the wrapper only reads: `_tensor` without the contiguity condition -> t, or its contiguous copy.  Outputs and in-place
    buffers never come through here: a copy would receive the result in the caller's place."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != len(shape) or not (t.is_cuda if device is None else t.device == device) or \
            any(not isinstance(w, str) and int(v) != w for v, w in zip(t.shape, shape)):
        raise LsfaError("%s: %s must be a (%s) %s tensor on %s, got %s" %
                        (who, what, ", ".join(str(w) for w in shape), dtype, device or "a CUDA device", _arrived(t)))
    return t if t.is_contiguous() else t.contiguous()


def _vector(who, what, t, n, device, dtype=torch.float32):
    """A per-channel operand or a weight the kernel reads as `n` consecutive values (a bias, a scale, a shift; in any shape): `dtype`, on
    `device` -> t, or its contiguous copy; None stays None (the optional ones)"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != device or t.numel() != n:
        raise LsfaError("%s: %s must be a %s tensor of %d elements on %s, got %s" % (who, what, dtype, n, device, _arrived(t)))
    return t if t.is_contiguous() else t.contiguous()


def _amax_row(who, what, t, device, measured=False):
    """None, or a row of amax_slots(): AMAX_SLOTS contiguous int32 words on `device`.  measured: an `amax_in`, which may also be
    amax_partial()'s float32 row (the same bits)"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not (t.dtype == torch.int32 or (measured and t.dtype == torch.float32)) or t.device != device or \
            tuple(t.shape) != (AMAX_SLOTS,) or not t.is_contiguous():
        raise LsfaError("%s: %s must be a row of amax_slots()%s: a contiguous (%d,) int32 tensor on %s, got %s" %
                        (who, what, " or amax_partial()'s float32 row" if measured else "", AMAX_SLOTS, device, _arrived(t)))
    return t


def _status_word(who, t, device):
    """None, or a new_status() word: (4,) contiguous int32 on `device`"""
    return None if t is None else _tensor(who, "status (a new_status() word)", t, torch.int32, (4,), device)


def _given(who, what, v, n):
    """a caller's tuple / list of `n` buffers"""
    if not isinstance(v, (tuple, list)) or len(v) != n:
        raise LsfaError("%s: %s must be a tuple of %d tensors, got %s" % (who, what, n, type(v).__name__))
    return v


def _on_tensor_device(fn):
    """Run an op with the device of its first tensor argument current, so that `_stream()` (the CURRENT
    stream of the CURRENT device) and the C side's per-device state belong to the tensors' device even
    when the caller never called torch.cuda.set_device (e.g. Predictor(..., context='cuda:1'))."""
    import functools

    @functools.wraps(fn)
    def wrapped(*args, **kw):
        dev = next((a.device for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return wrapped


def _means(pixel_means):
    """config.network.PIXEL_MEANS (B, G, R) as the three host doubles the image transforms read"""
    return (ctypes.c_double * 3)(*[float(m) for m in pixel_means])


def _resized(H, W, im_scale, stride):
    """-> h1, w1 = cvRound(H * im_scale), cvRound(W * im_scale) as numpy rounds them, then the two padded up to multiples of `stride`
    (0: as they are)"""
    h1, w1 = int(np.rint(H * float(im_scale))), int(np.rint(W * float(im_scale)))
    return (h1, w1, -(-h1 // stride) * stride, -(-w1 // stride) * stride) if stride else (h1, w1, h1, w1)


def _resized_map(H, W, im_scale, rcnn_stride):
    """-> _resized's h1, w1, then the height and width of the `motion_vector` / `res_diff` maps: its padded size in steps of rcnn_stride"""
    h1, w1, ph, pw = _resized(H, W, im_scale, rcnn_stride)
    return h1, w1, ph // rcnn_stride, pw // rcnn_stride


# ------------------------------------------------------------------------------------
@_on_tensor_device
def psroi_pool(data, rois, spatial_scale, output_dim, pooled_size, group_size, with_mapping=False):
    data = _input("psroi_pool", "data", data, ("N", "C", "H", "W"))
    rois = _input("psroi_pool", "rois", rois, ("R", 5), data.device)
    N, C, H, W = data.shape
    R = rois.shape[0]
    out = torch.empty((R, output_dim, pooled_size, pooled_size), device=data.device, dtype=torch.float32)
    mc = torch.empty_like(out) if with_mapping else None
    _check(lib().lsfa_psroi_pool_fwd(_ptr(data), _ptr(rois), N, C, H, W, R, spatial_scale, output_dim, pooled_size, group_size, _ptr(out), _ptr(mc),
                                     _stream()), "lsfa_psroi_pool_fwd")
    return (out, mc) if with_mapping else out


@_on_tensor_device
def rfcn_head(cls_map, box_map, rois, spatial_scale=0.0625, pooled_size=7, group_size=7, want_score=False,
              out=None):
    cls_map = _input("rfcn_head", "cls_map", cls_map, ("N", "Cc", "H", "W"))
    N, Cc, H, W = cls_map.shape
    box_map = _input("rfcn_head", "box_map (a map like cls_map)", box_map, (N, "Cb", H, W), cls_map.device)
    rois = _input("rfcn_head", "rois", rois, ("R", 5), cls_map.device)
    gg = group_size * group_size
    ncls, nbox = Cc // gg, box_map.shape[1] // gg
    R = rois.shape[0]
    if out is None:
        cls_prob = torch.empty((R, ncls), device=rois.device, dtype=torch.float32)
        bbox_pred = torch.empty((R, nbox), device=rois.device, dtype=torch.float32)
    else:
        out = _given("rfcn_head", "out", out, 2)
        cls_prob = _tensor("rfcn_head", "output buffer out[0] (cls_prob)", out[0], torch.float32, (R, ncls), rois.device)
        bbox_pred = _tensor("rfcn_head", "output buffer out[1] (bbox_pred)", out[1], torch.float32, (R, nbox), rois.device)
    cls_score = torch.empty((R, ncls), device=rois.device, dtype=torch.float32) if want_score else None
    _check(lib().lsfa_rfcn_head_fwd(_ptr(cls_map), _ptr(box_map), _ptr(rois), N, H, W, R, ncls, nbox, spatial_scale, pooled_size, group_size,
                                    _ptr(cls_prob), _ptr(cls_score), _ptr(bbox_pred), _stream()), "lsfa_rfcn_head_fwd")
    return (cls_prob, cls_score, bbox_pred) if want_score else (cls_prob, bbox_pred)


@_on_tensor_device
def rfcn_head_ps(ps_map, rois, ncls, nbox, spatial_scale=0.0625, pooled_size=7, group_size=7, want_score=False):
    """ps_map (N, H, W, group^2, ncls+nbox) float32 — see lsfa_rfcn_head_ps_fwd."""
    ps_map = _input("rfcn_head_ps", "ps_map", ps_map, ("N", "H", "W", group_size * group_size, ncls + nbox))
    rois = _input("rfcn_head_ps", "rois", rois, ("R", 5), ps_map.device)
    N, H, W = ps_map.shape[0], ps_map.shape[1], ps_map.shape[2]
    R = rois.shape[0]
    cls_prob = torch.empty((R, ncls), device=rois.device, dtype=torch.float32)
    bbox_pred = torch.empty((R, nbox), device=rois.device, dtype=torch.float32)
    cls_score = torch.empty((R, ncls), device=rois.device, dtype=torch.float32) if want_score else None
    _check(lib().lsfa_rfcn_head_ps_fwd(_ptr(ps_map), _ptr(rois), N, H, W, R, ncls, nbox, spatial_scale, pooled_size, group_size, _ptr(cls_prob),
                                       _ptr(cls_score), _ptr(bbox_pred), _stream()), "lsfa_rfcn_head_ps_fwd")
    return (cls_prob, cls_score, bbox_pred) if want_score else (cls_prob, bbox_pred)


def _warp(name, cl, feat, flow, mul, add, res, res_w, res_b, bn, out, amax_out=None, amax_c0=0):
    """The four lsfa_warp_bilinear* entry points: `cl` picks the layout, `bn` = (scale, shift) the form with warp_conv_feat_bn."""
    flow = _input(name, "flow", flow, ("N", 2, "H", "W"))
    N, _, H, W = flow.shape
    dev = flow.device
    feat = _input(name, "feat_cl" if cl else "feat", feat, ("feat_n", H, W, "C") if cl else ("feat_n", "C", H, W), dev)
    feat_n, C = feat.shape[0], feat.shape[3 if cl else 1]
    maps = (N, H, W, C) if cl else (N, C, H, W)
    if mul is not None:
        mul = _input(name, "mul", mul, maps, dev)
    if add is not None:
        add = _input(name, "add_cl" if cl else "add", add, maps, dev)
    res_c = 0
    if res is not None:
        res = _input(name, "res", res, (N, "res_c", H, W), dev)
        res_c = res.shape[1]
        if res_w is None or res_b is None:
            raise LsfaError("%s: res needs res_w and res_b (rnet_conv0), got %s and %s" % (name, _arrived(res_w), _arrived(res_b)))
        res_w, res_b = _vector(name, "res_w", res_w, C * res_c, dev), _vector(name, "res_b", res_b, C, dev)
    if bn is not None:
        if mul is not None:
            raise LsfaError("%s: mul together with bn: the library has no such kernel" % name)
        bn = _given(name, "bn", bn, 2)
        if bn[0] is None or bn[1] is None:
            raise LsfaError("%s: bn must be (scale, shift), got %s and %s" % (name, _arrived(bn[0]), _arrived(bn[1])))
        bn_scale, bn_shift = _vector(name, "bn scale", bn[0], C, dev), _vector(name, "bn shift", bn[1], C, dev)
    amax_out = _amax_row(name, "amax_out", amax_out, dev)
    if out is None:
        out = torch.empty(maps, device=feat.device, dtype=torch.float32)
    else:
        _tensor(name, "output buffer out", out, torch.float32, maps, dev)
    sym = "lsfa_warp_bilinear" + ("_bn" if bn is not None else "") + ("_cl" if cl else "")
    args = [_ptr(feat), feat_n, _ptr(flow), N, C, H, W]
    if bn is None and not cl:                     # `mul` is an argument of lsfa_warp_bilinear alone
        args.append(_ptr(mul))
    args += [_ptr(add), _ptr(res), res_c, _ptr(res_w), _ptr(res_b)]
    if bn is not None:
        args += [_ptr(bn_scale), _ptr(bn_shift)]
    args.append(_ptr(out))
    if cl:
        args += [_ptr(amax_out), amax_c0]
    _check(getattr(lib(), sym)(*args, _stream()), sym)
    return out


@_on_tensor_device
def warp_bilinear(feat, flow, mul=None, add=None, res=None, res_w=None, res_b=None, out=None, bn=None):
    """lsfa_warp_bilinear on NCHW maps.  bn = (scale, shift): lsfa_warp_bilinear_bn, warp_conv_feat_bn between the warp (+ rnet_conv0(res))
    and `add`: r * scale[c] + shift[c], two roundings; not together with `mul`."""
    return _warp("warp_bilinear", False, feat, flow, mul, add, res, res_w, res_b, bn, out)


@_on_tensor_device
def warp_bilinear_cl(feat_cl, flow, add_cl=None, res=None, res_w=None, res_b=None, out=None, amax_out=None, amax_c0=0, bn=None):
    """lsfa_warp_bilinear_cl: the non-key path's warp on channels-last maps.  feat_cl (feat_n, H, W, C), flow (N, 2, H, W), add_cl (N, H, W, C),
    res (N, res_c, H, W) -> (N, H, W, C); the bits of warp_bilinear on the transposed maps.  amax_out: a zeroed row of amax_slots() that
    receives max|out| over channels [amax_c0, C) (the scale of the convolution that reads those).  bn = (scale, shift):
    lsfa_warp_bilinear_bn_cl, as in warp_bilinear."""
    return _warp("warp_bilinear_cl", True, feat_cl, flow, None, add_cl, res, res_w, res_b, bn, out, amax_out, amax_c0)


@_on_tensor_device
def channel_mean(x1, x2=None, out=None):
    """lsfa_channel_mean: per-image channel means of channels-last maps, (N, H, W, C1) [and (N, H, W, C2) read as the concatenation
    [x1 | x2] without storing it] -> (N, C1 + C2).  Deterministic; the order is documented in include/lsfa_hip.h."""
    x1 = _input("channel_mean", "x1", x1, ("N", "H", "W", "C1"))
    N, H, W, C1 = x1.shape
    C2 = 0
    if x2 is not None:
        x2 = _input("channel_mean", "x2 (a map like x1)", x2, (N, H, W, "C2"), x1.device)
        C2 = x2.shape[3]
    C = C1 + C2
    if out is None:
        out = torch.empty((N, C), device=x1.device, dtype=torch.float32)
    else:
        _tensor("channel_mean", "output buffer out", out, torch.float32, (N, C), x1.device)
    need = lib().lsfa_channel_mean_workspace_bytes(N, C, H * W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x1.device)
    _check(lib().lsfa_channel_mean(_ptr(x1), C1, _ptr(x2), C2, N, H * W, _ptr(out), _ptr(ws), need, _stream()), "lsfa_channel_mean")
    return out


@_on_tensor_device
def channel_gate(m, w1, b1, w2, b2, out=None):
    """lsfa_channel_gate: sigmoid(w2 relu(w1 m + b1) + b2) for the N rows of m (N, K); w1 (M, K), w2 (O, M) fp32 -> (N, O)."""
    m = _input("channel_gate", "m", m, ("N", "K"))
    N, K = m.shape
    dev = m.device
    for what, t in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)):
        if not isinstance(t, torch.Tensor) or t.dim() < 1:
            raise LsfaError("channel_gate: %s must be a float32 tensor on %s, got %s" % (what, dev, _arrived(t)))
    M, O = int(w1.shape[0]), int(w2.shape[0])
    w1, b1 = _vector("channel_gate", "w1 (M, %d)" % K, w1, M * K, dev), _vector("channel_gate", "b1 (M)", b1, M, dev)
    w2, b2 = _vector("channel_gate", "w2 (O, M = %d)" % M, w2, O * M, dev), _vector("channel_gate", "b2 (O)", b2, O, dev)
    if out is not None:
        _tensor("channel_gate", "output buffer out", out, torch.float32, (N, O), dev)
    hidden = torch.empty((N, M), device=m.device, dtype=torch.float32)
    if out is None:
        out = torch.empty((N, O), device=m.device, dtype=torch.float32)
    _check(lib().lsfa_channel_gate(_ptr(m), N, K, _ptr(w1), _ptr(b1), M, _ptr(w2), _ptr(b2), O, _ptr(hidden), _ptr(out), _stream()),
           "lsfa_channel_gate")
    return out


@_on_tensor_device
def gate_apply(x, gate, y, out=None, amax_out=None, amax_c0=0):
    """lsfa_gate_apply: x * gate[n, c] + y (two roundings) on channels-last (N, H, W, C) maps; gate (N, C).  amax_out: a zeroed row of
    amax_slots() that receives max|out| over channels [amax_c0, C)."""
    x = _input("gate_apply", "x", x, ("N", "H", "W", "C"))
    N, H, W, C = x.shape
    gate = _input("gate_apply", "gate", gate, (N, C), x.device)
    y = _input("gate_apply", "y (a map like x)", y, (N, H, W, C), x.device)
    amax_out = _amax_row("gate_apply", "amax_out", amax_out, x.device)
    if out is None:
        out = torch.empty_like(x)
    else:
        _tensor("gate_apply", "output buffer out", out, torch.float32, (N, H, W, C), x.device)
    _check(lib().lsfa_gate_apply(_ptr(x), _ptr(gate), _ptr(y), N, H * W, C, _ptr(out), _ptr(amax_out), amax_c0, _stream()), "lsfa_gate_apply")
    return out


def warp_set_variant(variant):
    """'auto' | 'gather' | 'staged': lsfa_warp_set_variant (process-wide kernel choice of warp_bilinear; same results.  'staged'
    makes shapes the LDS-staged kernel does not take an error instead of falling back)."""
    _check(lib().lsfa_warp_set_variant(_WARP_VARIANTS[variant]), "lsfa_warp_set_variant")


@_on_tensor_device
def aggregate_softmax2(a, b, logits, out=None, logit_row_stride=None):
    """a, b (N, C, H, W); logits (2N, 1, H, W): rows [0, N) weight a, rows [N, 2N) weight b.
    logit_row_stride (r5): `logits` is any float32 tensor whose 2N rows of H*W logits start that many floats apart (the Nq net's
    last convolution written NCHW with 64 padded output channels: channel 0 of each image, stride 64*H*W) - no strided copy."""
    a = _input("aggregate_softmax2", "a", a, ("N", "C", "H", "W"))
    N, C, H, W = a.shape
    b = _input("aggregate_softmax2", "b (a map like a)", b, (N, C, H, W), a.device)
    if out is None:
        out = torch.empty_like(a)
    else:
        _tensor("aggregate_softmax2", "output buffer out", out, torch.float32, (N, C, H, W), a.device)
    if logit_row_stride is not None:
        if (not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.device != a.device or logit_row_stride < H * W or
                logits.numel() < (2 * N - 1) * logit_row_stride + H * W):
            raise LsfaError("aggregate_softmax2: logits %s (%s, %s) must be contiguous float32 on %s with %d rows of %d logits >= %d floats apart, got stride %d" % (
                tuple(getattr(logits, 'shape', ())), getattr(logits, 'dtype', type(logits)), getattr(logits, 'device', None), a.device, 2 * N, H * W,
                H * W, logit_row_stride))
        _check(lib().lsfa_aggregate_softmax2_rows(_ptr(a), _ptr(b), _ptr(logits), logit_row_stride, N, C, H, W, _ptr(out), _stream()),
               "lsfa_aggregate_softmax2_rows")
        return out
    logits = _vector("aggregate_softmax2", "logits (2N = %d rows of H * W = %d)" % (2 * N, H * W), logits, 2 * N * H * W, a.device)
    if logits is None:
        raise LsfaError("aggregate_softmax2: logits must be a float32 tensor, got None")
    if N == 1:
        _check(lib().lsfa_aggregate_softmax2(_ptr(a), _ptr(b), _ptr(logits), C, H, W, _ptr(out), _stream()), "lsfa_aggregate_softmax2")
    else:
        _check(lib().lsfa_aggregate_softmax2_batched(_ptr(a), _ptr(b), _ptr(logits), N, C, H, W, _ptr(out), _stream()),
               "lsfa_aggregate_softmax2_batched")
    return out


@_on_tensor_device
def aggregate_cosine(a, b, emb_warp, emb_cur, out=None):
    a = _input("aggregate_cosine", "a", a, (1, "C", "H", "W"))
    _, C, H, W = a.shape
    b = _input("aggregate_cosine", "b (a map like a)", b, (1, C, H, W), a.device)
    emb_warp = _input("aggregate_cosine", "emb_warp", emb_warp, (1, "E", H, W), a.device)
    emb_cur = _input("aggregate_cosine", "emb_cur (a map like emb_warp)", emb_cur, (1, emb_warp.shape[1], H, W), a.device)
    if out is None:
        out = torch.empty_like(a)
    else:
        _tensor("aggregate_cosine", "output buffer out", out, torch.float32, (1, C, H, W), a.device)
    _check(lib().lsfa_aggregate_cosine(_ptr(a), _ptr(b), _ptr(emb_warp), _ptr(emb_cur), C, emb_warp.shape[1], H, W, _ptr(out), _stream()),
           "lsfa_aggregate_cosine")
    return out


class ProposalOp(object):
    """MultiProposal / Proposal (multi_proposal-inl.h:124-159 params).  The workspace comes from torch's
    caching allocator per call, so calls issued on different streams (or captured into different
    graphs) never share scratch memory."""

    def __init__(self, feature_stride=16, scales=(8, 16, 32), ratios=(0.5, 1, 2), rpn_pre_nms_top_n=6000,
                 rpn_post_nms_top_n=300, threshold=0.7, rpn_min_size=16, output_score=False):
        self.feature_stride = int(feature_stride)
        self.scales = (ctypes.c_float * len(scales))(*[float(s) for s in scales])
        self.ratios = (ctypes.c_float * len(ratios))(*[float(r) for r in ratios])
        self.pre_n, self.post_n = int(rpn_pre_nms_top_n), int(rpn_post_nms_top_n)
        self.threshold, self.min_size = float(threshold), int(rpn_min_size)
        self.output_score = output_score

    def __call__(self, cls_prob, bbox_pred, im_info, out=None):
        cls_prob = _input("Proposal", "cls_prob", cls_prob, ("B", "2A", "H", "W"))
        if cls_prob.device.index != torch.cuda.current_device():
            with torch.cuda.device(cls_prob.device):
                return self(cls_prob, bbox_pred, im_info, out)
        B, A2, H, W = cls_prob.shape
        A = A2 // 2
        # (multi_proposal-inl.h:179-187)
        bbox_pred = _input("Proposal", "bbox_pred", bbox_pred, (B, 4 * A, H, W), cls_prob.device)
        im_info = _input("Proposal", "im_info", im_info, (B, 3), cls_prob.device)
        if out is not None:
            n_out = B * min(self.post_n, min(self.pre_n if self.pre_n > 0 else A * H * W, A * H * W))
            out = _given("Proposal", "out", out, 2)
            _tensor("Proposal", "output buffer out[0] (rois)", out[0], torch.float32, (n_out, 5), cls_prob.device)
            _tensor("Proposal", "output buffer out[1] (scores)", out[1], torch.float32, (n_out, 1), cls_prob.device)
        need = lib().lsfa_proposal_workspace_bytes(B, A, H, W, self.pre_n)
        ws = torch.empty(need, dtype=torch.uint8, device=cls_prob.device)
        count = A * H * W
        pre_n = min(self.pre_n if self.pre_n > 0 else count, count)
        post_n = min(self.post_n, pre_n)
        if out is None:
            rois = torch.empty((B * post_n, 5), device=cls_prob.device, dtype=torch.float32)
            scores = torch.empty((B * post_n, 1), device=cls_prob.device, dtype=torch.float32)
        else:
            rois, scores = out
        _check(lib().lsfa_proposal(_ptr(cls_prob), _ptr(bbox_pred), _ptr(im_info), B, A, H, W, self.feature_stride, self.scales, len(self.scales),
                                   self.ratios, len(self.ratios), self.pre_n, self.post_n, self.threshold, self.min_size, _ptr(rois), _ptr(scores),
                                   _ptr(ws), ws.numel(), _stream()), "lsfa_proposal")
        return (rois, scores) if self.output_score else rois


@_on_tensor_device
def proposal_set_plan(plan):
    """'auto' | 'single' | 'chip' | 'chip-box-sweep': lsfa_proposal_set_plan (process-wide launch plan; same results)."""
    _check(lib().lsfa_proposal_set_plan({'auto': 0, 'single': 1, 'chip': 2, 'chip-box-sweep': 3, 'lab-no-nms': 99}[plan]), "lsfa_proposal_set_plan")


# Ablation switches (tools/lab/tail_ablation.sh): LSFA_LAB_SKIP=tail,copy,nhwc drops launches from every frame so that
# bench.py's frames/s with and without them says what they cost the PIPELINE (not what they take alone):
#   tail  the Proposal's suppression stage (nms_mask + nms_sweep: `nms`), the PSROI head (`head`), the detection post-processing (det_class +
#         det_cap: `det`); each part also by its own name
#   copy  lsfa_copy_many's staging copies of frames / motion vectors / residuals into a graph's static buffers (after each buffer's first fill)
#   nhwc  lsfa_nchw_to_nhwc in front of the R-FCN / Nq convolutions (after each output's first fill)
# Results are garbage then; bench.py labels the line, reports no parity and does not read the status word.  Never set in a product run.
LAB_SKIP = set(v for v in os.environ.get('LSFA_LAB_SKIP', '').split(',') if v)
LAB_SKIP_TAIL = 'tail' in LAB_SKIP
LAB_SKIP_NMS = LAB_SKIP_TAIL or 'nms' in LAB_SKIP        # ... or one part of the tail: nms | head | det
LAB_SKIP_HEAD = LAB_SKIP_TAIL or 'head' in LAB_SKIP
LAB_SKIP_DET = LAB_SKIP_TAIL or 'det' in LAB_SKIP
_lab_filled = set()


def _nms_operands(who, boxes, dtype):
    """The operands of nms_sorted and nms_sorted_f64: boxes (n, >=4) of `dtype` -> (boxes, n, d, keep, num_keep, workspace)"""
    boxes = _input(who, "boxes", boxes, ("n", "d >= 4"), dtype=dtype)
    n, d = boxes.shape
    if d < 4:
        raise LsfaError("%s: boxes of %d values" % (who, d))
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=boxes.device)
    num = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    ws = torch.empty(lib().lsfa_nms_workspace_bytes(n), dtype=torch.uint8, device=boxes.device)
    return boxes, n, d, keep, num, ws


@_on_tensor_device
def nms_sorted(boxes, thresh):
    """boxes (n, >=4) float32 CUDA, sorted by score descending -> (keep int32 (n,), num_keep int32 (1,)) on device."""
    boxes, n, d, keep, num, ws = _nms_operands("nms_sorted", boxes, torch.float32)
    _check(lib().lsfa_nms_sorted(_ptr(boxes), n, d, thresh, _ptr(keep), _ptr(num), _ptr(ws), ws.numel(), _stream()), "lsfa_nms_sorted")
    return keep, num


@_on_tensor_device
def nms_sorted_f64(boxes, thresh):
    """boxes (n, >=4) float64 CUDA, sorted by score descending -> (keep, num_keep) like nms_sorted; numpy's
    float64 arithmetic and `ovr <= thresh` keep rule (lib/nms/nms.py:47-72)."""
    boxes, n, d, keep, num, ws = _nms_operands("nms_sorted_f64", boxes, torch.float64)
    _check(lib().lsfa_nms_sorted_f64(_ptr(boxes), n, d, thresh, _ptr(keep), _ptr(num), _ptr(ws), ws.numel(), _stream()), "lsfa_nms_sorted_f64")
    return keep, num


def nms_host(boxes_np, thresh, device_id=0):
    """The reference's `_nms` C entry point (lib/nms/gpu_nms.hpp:14-15): host numpy in, host list out."""
    boxes_np = np.ascontiguousarray(boxes_np, dtype=np.float32)
    n, d = boxes_np.shape
    keep = np.zeros(max(n, 1), dtype=np.int32)
    num = ctypes.c_int()
    lib()._nms(keep.ctypes.data_as(ctypes.c_void_p), ctypes.byref(num), boxes_np.ctypes.data_as(ctypes.c_void_p), n, d, thresh, device_id)
    return keep[:num.value]


@_on_tensor_device
def bbox_pred_clip(rois, deltas, im_h, im_w, scale):
    rois = _input("bbox_pred_clip", "rois", rois, ("R", 5))
    R = rois.shape[0]
    deltas = _input("bbox_pred_clip", "deltas", deltas, (R, "4 nreg"), rois.device)
    nreg = deltas.shape[1] // 4
    out = torch.empty((R, 4 * nreg), dtype=torch.float64, device=rois.device)
    _check(lib().lsfa_bbox_pred_clip(_ptr(rois), _ptr(deltas), R, nreg, im_h, im_w, scale, _ptr(out), _stream()), "lsfa_bbox_pred_clip")
    return out


def _det_operands(who, rois, deltas, probs, out, batch, B=1):
    """The operands of det_postprocess (one image, outputs without the image axis, `out` optional) and det_postprocess_batch (`batch`):
    rois (B*R, 5), deltas (B*R, 4*nreg), probs (B*R, ncls) -> (rois, deltas, probs, R, ncls, nreg, dets, counts, keep_idx)"""
    rois = _input(who, "rois", rois, ("B R" if batch else "R", 5))
    BR, dev = int(rois.shape[0]), rois.device
    if batch and (int(B) < 1 or BR % int(B)):
        raise LsfaError("%s: %d rois do not divide into B = %r images" % (who, BR, B))
    deltas = _input(who, "deltas", deltas, (BR, "4 nreg"), dev)
    probs = _input(who, "probs", probs, (BR, "ncls"), dev)
    R, ncls = (BR // B if batch else BR), probs.shape[1]
    nreg = deltas.shape[1] // 4
    lead = (B,) if batch else ()
    if out is None and not batch:
        dets = torch.zeros((ncls, R, 5), dtype=torch.float64, device=dev)
        counts = torch.zeros(ncls, dtype=torch.int32, device=dev)
        keep_idx = torch.full((ncls, R), -1, dtype=torch.int32, device=dev)
    else:
        out = _given(who, "out", out, 3)
        dets = _tensor(who, "output buffer out[0] (dets)", out[0], torch.float64, lead + (ncls, R, 5), dev)
        counts = _tensor(who, "output buffer out[1] (counts)", out[1], torch.int32, lead + (ncls,), dev)
        keep_idx = _tensor(who, "output buffer out[2] (keep_idx)", out[2], torch.int32, lead + (ncls, R), dev)
    return rois, deltas, probs, R, ncls, nreg, dets, counts, keep_idx


@_on_tensor_device
def det_postprocess(rois, deltas, probs, im_h, im_w, scale, score_thresh=1e-4, nms_thresh=0.3, max_per_image=300,
                    class_agnostic=True, out=None):
    rois, deltas, probs, R, ncls, nreg, dets, counts, keep_idx = _det_operands("det_postprocess", rois, deltas, probs, out, False)
    if LAB_SKIP_DET:
        return dets, counts, keep_idx
    _check(lib().lsfa_det_postprocess(_ptr(rois), _ptr(deltas), _ptr(probs), R, ncls, nreg, int(class_agnostic), im_h, im_w, scale, score_thresh,
                                      nms_thresh, max_per_image, _ptr(dets), _ptr(counts), _ptr(keep_idx), None, 0, _stream()),
           "lsfa_det_postprocess")
    return dets, counts, keep_idx


@_on_tensor_device
def rpn_softmax_split(logits, A):
    """lsfa_rpn_softmax_split: logits (N, H, W, L >= 6A) channels-last [score 2A | delta 4A | padding] -> (rpn_cls_prob (N, 2A, H, W),
    rpn_bbox_pred (N, 4A, H, W)): the per-anchor two-way softmax and the split into MultiProposal's NCHW inputs."""
    logits = _input("rpn_softmax_split", "logits", logits, ("N", "H", "W", "L >= 6A"))
    N, H, W, L = logits.shape
    if A < 1 or L < 6 * A:
        raise LsfaError("rpn_softmax_split: %d channels do not hold the scores and deltas of A = %r anchors" % (L, A))
    cls_prob = torch.empty((N, 2 * A, H, W), device=logits.device, dtype=torch.float32)
    bbox = torch.empty((N, 4 * A, H, W), device=logits.device, dtype=torch.float32)
    _check(lib().lsfa_rpn_softmax_split(_ptr(logits), N, H, W, L, A, _ptr(cls_prob), _ptr(bbox), _stream()), "lsfa_rpn_softmax_split")
    return cls_prob, bbox


@_on_tensor_device
def det_postprocess_batch(rois, deltas, probs, B, im_h, im_w, scale, out, score_thresh=1e-4, nms_thresh=0.3, max_per_image=300,
                          class_agnostic=True):
    """lsfa_det_postprocess_batch: det_postprocess for the B images of a batch in one launch pair.  rois (B*R, 5), deltas (B*R, 4*nreg),
    probs (B*R, ncls), image b's rows [b*R, (b+1)*R); out = (dets (B, ncls, R, 5) f64, counts (B, ncls) i32, keep_idx (B, ncls, R) i32)."""
    rois, deltas, probs, R, ncls, nreg, dets, counts, keep_idx = _det_operands("det_postprocess_batch", rois, deltas, probs, out, True, B)
    if LAB_SKIP_DET:
        return dets, counts, keep_idx
    _check(lib().lsfa_det_postprocess_batch(_ptr(rois), _ptr(deltas), _ptr(probs), B, R, ncls, nreg, int(class_agnostic), im_h, im_w, scale,
                                            score_thresh, nms_thresh, max_per_image, _ptr(dets), _ptr(counts), _ptr(keep_idx), None, 0, _stream()),
           "lsfa_det_postprocess_batch")
    return dets, counts, keep_idx


@_on_tensor_device
def deform_im2col(data, offset, kh, kw, pad, stride, dilate, deform_groups, out=None):
    data = _input("deform_im2col", "data", data, ("N", "C", "H", "W"))
    N, C, H, W = data.shape
    Ho, Wo = conv_out_hw(H, W, kh, kw, stride, (pad, pad), dilate)
    offset = _input("deform_im2col", "offset (2 * kh * kw * deform_groups channels on the convolution's output grid)", offset,
                    (N, 2 * kh * kw * deform_groups, Ho, Wo), data.device)
    if out is None:
        out = torch.empty((N, C * kh * kw, Ho * Wo), dtype=torch.float32, device=data.device)
    else:
        _tensor("deform_im2col", "output buffer out", out, torch.float32, (N, C * kh * kw, Ho * Wo), data.device)
    _check(lib().lsfa_deform_im2col(_ptr(data), _ptr(offset), N, C, H, W, kh, kw, pad, stride, dilate, deform_groups, Ho, Wo, _ptr(out), _stream()),
           "lsfa_deform_im2col")
    return out


@_on_tensor_device
def deform_im2col_cl(data, offset, kh, kw, pad, stride, dilate, deform_groups, out=None):
    """data (N,H,W,C), offset (N,Ho,Wo,L) contiguous with L >= 2*kh*kw*dg (channels past those are padding)
    -> col (N, Ho*Wo, kh*kw*C), k = tap*C + c."""
    data = _input("deform_im2col_cl", "data", data, ("N", "H", "W", "C"))
    N, H, W, C = data.shape
    Ho, Wo = conv_out_hw(H, W, kh, kw, stride, (pad, pad), dilate)
    offset = _input("deform_im2col_cl", "offset (on the convolution's output grid)", offset, (N, Ho, Wo, "L"), data.device)
    if offset.shape[3] < 2 * kh * kw * deform_groups:
        raise LsfaError("deform_im2col_cl: offset has %d channels, expected %d" % (offset.shape[3], 2 * kh * kw * deform_groups))
    if out is None:
        out = torch.empty((N, Ho * Wo, kh * kw * C), dtype=torch.float32, device=data.device)
    else:
        _tensor("deform_im2col_cl", "output buffer out", out, torch.float32, (N, Ho * Wo, kh * kw * C), data.device)
    _check(lib().lsfa_deform_im2col_cl_ld(_ptr(data), _ptr(offset), offset.shape[3], N, C, H, W, kh, kw, pad, stride, dilate, deform_groups, Ho, Wo,
                                          _ptr(out), _stream()), "lsfa_deform_im2col_cl_ld")
    return out


def _scale_shift(who, x, scale, shift, out, axis):
    """The operands of the three lsfa_scale_shift_*: x float32 with its channels on `axis` (1: (N, C, ...), -1: (..., C)), scale and shift
    of C values, out like x -> (x, scale, shift, out, rows in front of the channel axis, C, values behind it)"""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or x.dim() < 2 or x.numel() == 0:
        raise LsfaError("%s: x must be a non-empty float32 CUDA tensor of at least 2 dimensions, got %s" % (who, _arrived(x)))
    C = int(x.shape[axis])
    if scale is None or shift is None:
        raise LsfaError("%s: scale and shift must be float32 tensors of %d elements, got %s and %s" % (who, C, _arrived(scale), _arrived(shift)))
    scale, shift = _vector(who, "scale", scale, C, x.device), _vector(who, "shift", shift, C, x.device)
    if out is not None:
        _tensor(who, "output buffer out", out, torch.float32, tuple(int(v) for v in x.shape), x.device)
    x = x if x.is_contiguous() else x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    lead = int(x.shape[0]) if axis == 1 else x.numel() // C
    return x, scale, shift, out, lead, C, x.numel() // (lead * C)


@_on_tensor_device
def scale_shift_relu(x, scale, shift, relu=True, out=None):
    x, scale, shift, out, N, C, HW = _scale_shift("scale_shift_relu", x, scale, shift, out, 1)
    _check(lib().lsfa_scale_shift_relu(_ptr(x), _ptr(scale), _ptr(shift), N, C, HW, int(relu), _ptr(out), _stream()), "lsfa_scale_shift_relu")
    return out


@_on_tensor_device
def scale_shift_leaky(x, scale, shift, slope, out=None):
    x, scale, shift, out, N, C, HW = _scale_shift("scale_shift_leaky", x, scale, shift, out, 1)
    _check(lib().lsfa_scale_shift_leaky(_ptr(x), _ptr(scale), _ptr(shift), N, C, HW, slope, _ptr(out), _stream()), "lsfa_scale_shift_leaky")
    return out


@_on_tensor_device
def scale_shift_relu_cl(x, scale, shift, relu=True, out=None):
    """Channels-last form: x (..., C) contiguous with the channel the fastest axis, C % 4 == 0."""
    x, scale, shift, out, rows, C, _ = _scale_shift("scale_shift_relu_cl", x, scale, shift, out, -1)
    _check(lib().lsfa_scale_shift_relu_cl(_ptr(x), _ptr(scale), _ptr(shift), rows, C, int(relu), _ptr(out), _stream()), "lsfa_scale_shift_relu_cl")
    return out


# algorithmic FLOPs (2*M*N*K, fp32-equivalent) of the own convolutions issued since the last reset: bench.py divides
# them by the event-timed duration of the same launches for its MFMA roofline
_conv_flops = {"count": False, "flops": 0.0, "launches": 0, "flops_three_products": 0.0, "flops_one_product": 0.0, "bytes": 0.0, "by_kernel": {}}


def conv_flops_reset(enable=True):
    _conv_flops.update(count=bool(enable), flops=0.0, launches=0, flops_three_products=0.0, flops_one_product=0.0, bytes=0.0, by_kernel={})


def conv_bytes_read():
    """r5: algorithmic bytes of the counted calls - each operand once: the input channels the call reads, its packed weights, the output,
    the residual, a stored second output (4 bytes per activation, 2 x pieces per weight)"""
    return _conv_flops["bytes"]


def conv_by_kernel():
    """r5: {kernel instantiation as rocprofv3 prints it: {"calls", "gflop", "mbytes"}} of the counted calls (lsfa_conv_plan_query)"""
    return {k: {"calls": v[0], "gflop": round(v[1] / 1e9, 3), "mbytes": round(v[2] / 1e6, 3)} for k, v in _conv_flops["by_kernel"].items()}


def _count_launch(name, flops, nbytes=0.0, pieces=3):
    """THE counting entry: every wrapper calls it once per launch, and only while _conv_flops["count"] is set (so that a launch that is not
    counted computes none of its arguments - the plan query behind a kernel's name least of all).  The launch's algorithmic FLOPs go into
    the total and its piece form's share; with the kernel's name also its bytes and its by_kernel row (None: lsfa_conv_nhwc_fused_fwd,
    which the roofline does not list)."""
    c = _conv_flops
    c["flops"] += flops
    c["launches"] += 1
    if pieces == 2:
        c["flops_three_products"] += flops
    elif pieces == 1:
        c["flops_one_product"] += flops
    if name is not None:
        c["bytes"] += nbytes
        e = c["by_kernel"].setdefault(name, [0, 0.0, 0.0])
        e[0] += 1
        e[1] += flops
        e[2] += nbytes


def _plan_kernel_name(d):
    q = (ctypes.c_int * 8)()
    if lib().lsfa_conv_plan_query(ctypes.byref(d), q) != 0:
        return "?"
    kind, nt, st, sp, wv, slices, af, pc = [int(v) for v in q]
    b = lambda v: "true" if v else "false"
    if kind == 2:
        return "conv_split_direct_kernel<%d>" % pc
    return "conv_ring_kernel<%d, %d, %d, %s, %s, %d>%s" % (nt, pc, st, b(sp), b(af), wv, "" if slices <= 1 else " +split_reduce")


def conv_flops_read():
    return _conv_flops["flops"], _conv_flops["launches"]


def conv_flops_three_products():
    """the part of conv_flops_read()'s FLOPs that ran on the fp16 two-piece form (three matrix instructions per product, not six)"""
    return _conv_flops["flops_three_products"]


def conv_flops_one_product():
    """... and the part that ran one bf16 product per fp32 product (the bf16 mode)"""
    return _conv_flops["flops_one_product"]


def round_up(c, m):
    """c rounded up to a multiple of m: channel counts to the kernels' granularities (32 input channels, 64 output channels)"""
    return -(-c // m) * m


def conv_out_hw(H, W, kh, kw, stride=1, pad=(0, 0), dil=1):
    """(Ho, Wo): the output grid of a convolution of an H x W map; pad = (pad_h, pad_w)"""
    return tuple((n + 2 * p - dil * (k - 1) - 1) // stride + 1 for n, p, k in ((H, pad[0], kh), (W, pad[1], kw)))


def _check_outputs(who, numel, device, **tensors):
    """the tensors a convolution writes into or adds (None = not given): contiguous float32 of the output's size on `device`"""
    for name, t in tensors.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.numel() != numel or not t.is_contiguous() or t.dtype != torch.float32 or
                              t.device != device):
            raise LsfaError("%s: %s must be a contiguous float32 tensor of %d elements on %s, got %s" % (who, name, numel, device, _arrived(t)))


def conv_weight_kc(weight):
    """(Cout, Cin, kh, kw) -> (Cout, kh*kw, Cin) contiguous: the layout conv_nhwc reads (K contiguous)."""
    co, ci, kh, kw = weight.shape
    return weight.permute(0, 2, 3, 1).reshape(co, kh * kw, ci).contiguous()


@_on_tensor_device
def conv_nhwc(x, w_kc, bias, kh, kw, stride=1, pad=0, dil=1, relu=False, out=None, residual=None, out2=None, scale2=None,
              shift2=None):
    """x (N, H, W, Cin) contiguous fp32; w_kc from conv_weight_kc; -> (N, Ho, Wo, Cout).
    residual (same shape as the output; may BE `out`): added before the ReLU / store.  out2 + scale2 + shift2: second
    output max(out*scale2[c] + shift2[c], 0) (the next ResNet unit's bn1 + relu1).  Returns out, or (out, out2)."""
    x = _input("conv_nhwc", "x", x, ("N", "H", "W", "Cin"))
    N, H, W, Cin = x.shape
    w_kc = _input("conv_nhwc", "w_kc (from conv_weight_kc)", w_kc, ("Cout", kh * kw, Cin), x.device)
    Cout = w_kc.shape[0]
    bias = _vector("conv_nhwc", "bias", bias, Cout, x.device)
    scale2, shift2 = _vector("conv_nhwc", "scale2", scale2, Cout, x.device), _vector("conv_nhwc", "shift2", shift2, Cout, x.device)
    Ho, Wo = conv_out_hw(H, W, kh, kw, stride, (pad, pad), dil)
    _check_outputs("conv_nhwc", N * Ho * Wo * Cout, x.device, out=out, residual=residual, out2=out2)
    if out is None:
        out = torch.empty((N, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    if _conv_flops["count"]:
        _count_launch(None, 2.0 * N * Ho * Wo * Cout * Cin * kh * kw)
    need = lib().lsfa_conv_nhwc_workspace_bytes(N, H, W, Cout, kh, kw, stride, pad, dil)
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    _check(lib().lsfa_conv_nhwc_fused_fwd(_ptr(x), N, H, W, Cin, _ptr(w_kc), _ptr(bias), Cout, kh, kw, stride, pad, dil, int(relu), _ptr(residual),
                                          _ptr(out), _ptr(out2), _ptr(scale2), _ptr(shift2), _ptr(ws), need, _stream()), "lsfa_conv_nhwc_fused_fwd")
    return out if out2 is None else (out, out2)


def copy_many(pairs):
    """[(dst, src), ...] (at most 32; same shapes, contiguous, 4-byte dtypes, one device) as ONE launch on the current stream.
    src None (r5): dst is zero-filled - the frame path's amax slots and padded maps are cleared by this kernel, not by a PyTorch fill."""
    pairs = list(pairs)
    for d, s in pairs:
        if not isinstance(d, torch.Tensor) or not (s is None or isinstance(s, torch.Tensor)):
            raise LsfaError("copy_many: (dst, src) pairs of tensors (src may be None) expected, got %s <- %s" % (_arrived(d), _arrived(s)))
    pairs = [(d, s) for d, s in pairs if d.numel()]
    if not pairs:
        return
    n = len(pairs)
    if n > 32:
        raise LsfaError("copy_many: at most 32 copies per launch")
    for d, s in pairs:
        if d.element_size() != 4 or not d.is_contiguous() or not d.is_cuda or d.device != pairs[0][0].device:
            raise LsfaError("copy_many: %s: need a 4-byte dtype, contiguous, one CUDA device; got %s" % (tuple(d.shape), _arrived(d)))
        if s is not None and (d.shape != s.shape or d.dtype != s.dtype or not s.is_contiguous() or d.device != s.device):
            raise LsfaError("copy_many: %s <- %s: need equal shapes, 4-byte dtype, contiguous, one device; got %s <- %s"
                            % (tuple(d.shape), tuple(s.shape), _arrived(d), _arrived(s)))
    if 'copy' in LAB_SKIP:      # ablation: copies of >= 1 KB into a buffer that has been filled once are dropped (zero fills stay)
        kept = []
        for d, s_ in pairs:
            if s_ is None or d.numel() < 256 or d.data_ptr() not in _lab_filled:
                kept.append((d, s_))
            _lab_filled.add(d.data_ptr())
        pairs = kept
        n = len(pairs)
        if not n:
            return
    dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    src = (ctypes.c_void_p * n)(*[(s.data_ptr() if s is not None else None) for _, s in pairs])
    cnt = (ctypes.c_long * n)(*[d.numel() for d, _ in pairs])
    with torch.cuda.device(pairs[0][0].device):
        _check(lib().lsfa_copy_many(n, dst, src, cnt, _stream()), "lsfa_copy_many")


@_on_tensor_device
def transform_mv_res(motion_vector, res_diff, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16, negate_mv=False, out=None):
    """lsfa_transform_mv_res: (H, W, 2) motion vectors + (H, W, 3) residual on the device (int32 or float32) -> `motion_vector` (1, 2, h, w),
    `res_diff` (1, 3, h, w) float32 (transform_mv_res, lib/utils/image.py:202-228), one launch.  negate_mv: get_image's
    `motion_vector = - motion_vector` (:54) applied to the source values.  out: a pair of contiguous float32 tensors of those shapes."""
    mv, res = motion_vector, res_diff
    if not isinstance(mv, torch.Tensor) or not isinstance(res, torch.Tensor) or not mv.is_cuda or res.device != mv.device:
        raise LsfaError("transform_mv_res: motion_vector and res_diff must be tensors on one CUDA device, got %s / %s" % (_arrived(mv), _arrived(res)))
    if mv.dtype != res.dtype or mv.dtype not in (torch.int32, torch.float32):
        raise LsfaError("transform_mv_res: int32 or float32 maps expected, got %s / %s" % (mv.dtype, res.dtype))
    if mv.dim() != 3 or res.dim() != 3 or mv.shape[2] != 2 or res.shape[2] != 3 or mv.shape[:2] != res.shape[:2] or not (mv.is_contiguous() and res.is_contiguous()):
        raise LsfaError("transform_mv_res: contiguous (H, W, 2) and (H, W, 3) expected, got %s / %s" % (tuple(mv.shape), tuple(res.shape)))
    H, W = int(mv.shape[0]), int(mv.shape[1])
    h1, w1, ph, pw = _resized(H, W, im_scale, rcnn_stride)
    oh, ow = ph // rcnn_stride, pw // rcnn_stride
    if out is None:
        out = (torch.empty((1, 2, oh, ow), device=mv.device, dtype=torch.float32), torch.empty((1, 3, oh, ow), device=mv.device, dtype=torch.float32))
    out = _given("transform_mv_res", "out", out, 2)
    out_mv = _tensor("transform_mv_res", "output buffer out[0]", out[0], torch.float32, (1, 2, oh, ow), mv.device)
    out_res = _tensor("transform_mv_res", "output buffer out[1]", out[1], torch.float32, (1, 3, oh, ow), mv.device)
    _check(lib().lsfa_transform_mv_res(_ptr(mv), _ptr(res), int(mv.dtype == torch.int32) | (2 if negate_mv else 0), H, W, float(im_scale), h1, w1,
                                       int(rcnn_stride), _means(pixel_means), float(pixel_scale), _ptr(out_mv), _ptr(out_res), oh, ow, _stream()),
           "lsfa_transform_mv_res")
    return out_mv, out_res


@_on_tensor_device
def image_resize_transform(im, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, stride=0, u8_fixed_point=False):
    """lsfa_image_resize_transform: decoded frames (N, H, W, 3) or (H, W, 3) BGR, uint8 or float32, on the device -> `data` (N, 3, h, w) float32:
    resize (lib/utils/image.py:266-294) + transform (:296-308) in one launch.  u8_fixed_point (uint8 frames only): interpolate on OpenCV's
    fixed-point uint8 path and subtract the means in float64 - what the reference does to the LAST frame of a video, which it reads with
    cv2.imread (:45); the default treats a uint8 frame like the decoder's (converted to float first, :52)."""
    if isinstance(im, torch.Tensor) and im.dim() == 3:
        im = im.unsqueeze(0)
    if not isinstance(im, torch.Tensor) or im.dtype not in (torch.uint8, torch.float32) or im.dim() != 4 or im.shape[3] != 3 or \
            not im.is_contiguous() or not im.is_cuda:
        raise LsfaError("image_resize_transform: (N, H, W, 3) contiguous uint8 or float32 on a CUDA device expected, got %s" % _arrived(im))
    N, H, W, _ = [int(v) for v in im.shape]
    h1, w1, ph, pw = _resized(H, W, im_scale, stride)
    out = torch.empty((N, 3, ph, pw), device=im.device, dtype=torch.float32)
    if u8_fixed_point and im.dtype != torch.uint8:
        raise LsfaError("image_resize_transform: u8_fixed_point needs uint8 frames")
    _check(lib().lsfa_image_resize_transform(_ptr(im), 2 if u8_fixed_point else int(im.dtype == torch.uint8), N, H, W, float(im_scale), h1, w1,
                                             int(stride), _means(pixel_means), float(pixel_scale), _ptr(out), ph, pw, _stream()),
           "lsfa_image_resize_transform")
    return out


@_on_tensor_device
def image_transform_u8(im, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, out=None):
    """lsfa_image_transform_u8: decoded frames (N, H, W, 3) uint8 BGR on the device -> (N, 3, H, W) float32 RGB minus means, times scale
    (transform, lib/utils/image.py:296-308).  pixel_means in B, G, R order (config.network.PIXEL_MEANS)."""
    _tensor("image_transform_u8", "im", im, torch.uint8, ("N", "H", "W", 3))
    N, H, W, _ = im.shape
    if out is None:
        out = torch.empty((N, 3, H, W), device=im.device, dtype=torch.float32)
    else:
        _tensor("image_transform_u8", "output buffer out", out, torch.float32, (N, 3, H, W), im.device)
    _check(lib().lsfa_image_transform_u8(_ptr(im), N, H, W, _means(pixel_means), pixel_scale, _ptr(out), _stream()), "lsfa_image_transform_u8")
    return out


# ---- YUV intake (lsfa_amd/csrc/yuvfmt.hip): the one plane checker and the one output block behind the wrappers here, in yuv10.py and yuvfmt.py
YUV_MATRICES = {'bt601': 0, 'bt709': 1, 'jpeg': 2}


def _yuv_planes(who, y, uv, u, v, matrix, sub=0, layout=None, words=False, width=None, fmt=None):
    """The plane arguments of every lsfa_*yuv* export, up to `matrix`, from CUDA tensors: y (H, W) or (N, H, W) and either uv (.., ch, 2 cw) -
    one interleaved chroma plane - or u, v (.., ch, cw) - two planes - with ch = ceil(H / 2^sy), cw = ceil(W / 2^sx).  sub (0: 4:2:0,
    1: 4:2:2, 2: 4:4:4), layout (0: planar, 1 / 2: interleaved U, V / V, U, 3 / 4: packed, y the one plane of four-byte groups and `width`
    the W where it is odd) and words (16-bit samples, else bytes) are the format's fields (include/lsfa_hip.h); layout None takes it from
    the planes given, as the 4:2:0 exports do; fmt is what a message calls the format.  Row views of pitched surfaces are taken as they
    are: pitch and frame stride come from .stride(), only the last dimension must be dense.  Returns (ctypes arguments with pitches in
    bytes, N, H, W, batched); the caller appends its own trailing argument: nothing, `shift` or `format`."""
    def shapes():
        return ", ".join("%s %s" % (n, (tuple(t.shape), tuple(t.stride()), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__)
                         for n, t in (("y", y), ("uv", uv), ("u", u), ("v", v)) if t is not None)
    if matrix not in YUV_MATRICES:
        raise LsfaError("%s: matrix %r is not one of %s" % (who, matrix, sorted(YUV_MATRICES)))
    if layout is None:
        if (uv is not None) == (u is not None or v is not None) or (uv is None and (u is None or v is None)):
            raise LsfaError("%s: give either uv (one interleaved plane: NV12, P010) or u and v (two planes: I420); got %s" % (who, shapes()))
        layout = 1 if uv is not None else 0
    packed, semi = layout >= 3, layout in (1, 2)
    if packed:
        if uv is not None or u is not None or v is not None:
            raise LsfaError("%s: a packed frame is the one plane y; got %s" % (who, shapes()))
        planes = [y]
    elif semi:
        if uv is None or u is not None or v is not None:
            raise LsfaError("%s: format %r has one interleaved chroma plane: give uv and neither u nor v; got %s" % (who, fmt, shapes()))
        planes = [y, uv]
    else:
        if uv is not None or u is None or v is None:
            raise LsfaError("%s: format %r has two chroma planes: give u and v and no uv; got %s" % (who, fmt, shapes()))
        planes = [y, u, v]
    dtypes = (torch.int16, torch.uint16) if words else (torch.uint8,)
    for t in planes:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or not t.is_cuda or t.dim() not in (2, 3):
            raise LsfaError("%s: 2-D or 3-D %s CUDA planes expected, got %s" % (who, " / ".join(str(d) for d in dtypes), shapes()))
    for t in planes:
        if t.dim() != y.dim() or t.device != y.device or (t.shape[-1] > 1 and t.stride(-1) != 1):
            raise LsfaError("%s: planes of one device and rank with a dense last dimension expected, got %s" % (who, shapes()))
    batched = y.dim() == 3
    N = int(y.shape[0]) if batched else 1
    H, row = int(y.shape[-2]), int(y.shape[-1])
    if H < 1 or row < 1 or N < 1:
        raise LsfaError("%s: empty planes: %s" % (who, shapes()))
    if packed:
        if row % 4:
            raise LsfaError("%s: a packed row is ceil(W / 2) groups of four bytes, got %s" % (who, shapes()))
        W = row // 2 if width is None else width
        if isinstance(W, bool) or not isinstance(W, int) or -(-W // 2) != row // 4:
            raise LsfaError("%s: width %r does not give the %d groups of %s" % (who, width, row // 4, shapes()))
    else:
        W = row
        if width is not None and width != W:
            raise LsfaError("%s: width %r is not the Y plane's: %s" % (who, width, shapes()))
    b = 2 if words else 1
    # a plane of one row (or one frame) has no meaningful stride of its own: the row's (the frame's) size serves
    y_pitch = int(y.stride(-2)) if H > 1 else max(int(y.stride(-2)), row)
    y_fs = int(y.stride(0)) if batched and N > 1 else 0
    if y_pitch < row:
        raise LsfaError("%s: a row pitch is below its row: %s" % (who, shapes()))
    if packed:
        return (_ptr(y), y_pitch, y_fs, None, None, 0, 0, N, H, W, YUV_MATRICES[matrix]), N, H, W, batched
    ch, cw = -(-H // (2 if sub == 0 else 1)), -(-W // (1 if sub == 2 else 2))
    want = (ch, 2 * cw) if semi else (ch, cw)
    for t in planes[1:]:
        if tuple(t.shape[-2:]) != want or (batched and int(t.shape[0]) != N):
            raise LsfaError("%s: a %d x %d frame%s has %s chroma planes of %s samples%s, got %s" %
                            (who, W, H, "" if fmt is None else " of format %r" % (fmt,), "an interleaved" if semi else "two", want,
                             " per frame, %d frames" % N if batched else "", shapes()))
    c = planes[1]
    if not semi and u.stride() != v.stride():
        raise LsfaError("%s: u and v must share one pitch and frame stride, got %s" % (who, shapes()))
    c_pitch = int(c.stride(-2)) if ch > 1 else max(int(c.stride(-2)), want[1])
    c_fs = int(c.stride(0)) if batched and N > 1 else 0
    if c_pitch < want[1]:
        raise LsfaError("%s: a row pitch is below its row: %s" % (who, shapes()))
    args = (_ptr(y), b * y_pitch, b * y_fs, _ptr(c), _ptr(None if semi else v), b * c_pitch, b * c_fs, N, H, W, YUV_MATRICES[matrix])
    return args, N, H, W, batched


def _yuv_out(who, out, shape, dtype, device, name="out"):
    """the output of an intake wrapper: a new tensor, or the caller's once it is the contiguous `dtype` tensor of `shape` on the planes' device"""
    return torch.empty(shape, dtype=dtype, device=device) if out is None else _tensor(who, name, out, dtype, shape, device)


def _yuv_bgr_out(who, N, H, W, batched, device, out, y_packed):
    """-> out (H, W, 3) / (N, H, W, 3) uint8; y_packed, where given, is checked as the (.., H, W) uint8 plane"""
    lead = (N,) if batched else ()
    if y_packed is not None:
        _tensor(who, "y_packed", y_packed, torch.uint8, lead + (H, W), device)
    return _yuv_out(who, out, lead + (H, W, 3), torch.uint8, device)


def _yuv_resized_out(who, N, H, W, im_scale, stride, device, out):
    """-> (stride, h1, w1, ph, pw, out (N, 3, ph, pw) float32) of a resize form: _resized's sizes once im_scale and stride are in range"""
    if not float(im_scale) > 0.0 or int(stride) < 0:
        raise LsfaError("%s: im_scale %r must be positive and stride %r non-negative" % (who, im_scale, stride))
    stride = int(stride)
    h1, w1, ph, pw = _resized(H, W, im_scale, stride)
    return stride, h1, w1, ph, pw, _yuv_out(who, out, (N, 3, ph, pw), torch.float32, device)


@_on_tensor_device
def yuv420_to_bgr_u8(y, uv=None, u=None, v=None, matrix='bt601', out=None, y_packed=None):
    """lsfa_yuv420_to_bgr_u8: a decoder's YUV 4:2:0 planes on the device - y (H, W) or (N, H, W) uint8 and either uv (NV12: interleaved U, V,
    (.., ceil(H/2), 2 ceil(W/2))) or u, v (I420: (.., ceil(H/2), ceil(W/2))), possibly row views of pitched surfaces (`y[:, :W]`) - to packed
    uint8 BGR (H, W, 3) / (N, H, W, 3), the layout lsfa_mv_residual, luma_u8 and image_transform_u8 take.  matrix: 'bt601' (limited range,
    the default), 'bt709' (limited range) or 'jpeg' (BT.601 full range); nearest-neighbour chroma, integer arithmetic (include/lsfa_hip.h,
    "YUV 4:2:0 intake" - this project's own specification, not swscale's or OpenCV's).  y_packed: an optional (.., H, W) uint8 tensor that
    receives the Y plane with the pitch removed (what mv_estimate wants).  One launch."""
    who = "yuv420_to_bgr_u8"
    args, N, H, W, batched = _yuv_planes(who, y, uv, u, v, matrix)
    out = _yuv_bgr_out(who, N, H, W, batched, y.device, out, y_packed)
    _check(lib().lsfa_yuv420_to_bgr_u8(*(args + (_ptr(out), _ptr(y_packed), _stream()))), "lsfa_yuv420_to_bgr_u8")
    return out


@_on_tensor_device
def image_transform_yuv420(y, uv=None, u=None, v=None, matrix='bt601', pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, out=None):
    """lsfa_image_transform_yuv420: the planes of yuv420_to_bgr_u8 -> `data` (N, 3, H, W) float32, channel i = (bgr[2 - i] - pixel_means[2 - i])
    * pixel_scale in float64, rounded once: bit-identical to image_transform_u8(yuv420_to_bgr_u8(...)) without storing the BGR frame, and
    without its H*W % 4 condition.  pixel_means in B, G, R order.  One launch."""
    who = "image_transform_yuv420"
    args, N, H, W, _ = _yuv_planes(who, y, uv, u, v, matrix)
    out = _yuv_out(who, out, (N, 3, H, W), torch.float32, y.device)
    _check(lib().lsfa_image_transform_yuv420(*(args + (_means(pixel_means), float(pixel_scale), _ptr(out), _stream()))),
           "lsfa_image_transform_yuv420")
    return out


@_on_tensor_device
def image_resize_transform_yuv420(y, uv=None, u=None, v=None, im_scale=1.0, matrix='bt601', pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, stride=0,
                                  out=None):
    """lsfa_image_resize_transform_yuv420: the planes of yuv420_to_bgr_u8 -> `data` (N, 3, h, w) float32: image_resize_transform of the
    converted uint8 frame (converted to float, interpolated in float, padded to `stride`), bit-identical to it, reading the taps from the
    planes.  One launch.  The fixed-point uint8 form (u8_fixed_point) is not offered for YUV."""
    who = "image_resize_transform_yuv420"
    args, N, H, W, _ = _yuv_planes(who, y, uv, u, v, matrix)
    stride, h1, w1, ph, pw, out = _yuv_resized_out(who, N, H, W, im_scale, stride, y.device, out)
    _check(lib().lsfa_image_resize_transform_yuv420(*(args + (float(im_scale), h1, w1, stride, _means(pixel_means), float(pixel_scale), _ptr(out),
                                                               ph, pw, _stream()))),
           "lsfa_image_resize_transform_yuv420")
    return out


class ImageTable(object):
    """N images (C, H, W) float32, each ANYWHERE on the device, in place of one (N, C, H, W) tensor: what lsfa_avgpool_nchw_tbl and
    lsfa_stem_conv7x7s2_tbl read.  The reference's loader hands over one array per frame (dff_rfcn/core/loader.py:131-141); a batched pass
    over F such frames used to copy them into one static buffer first (lsfa_copy_many: 2 x 65 MB per nine-frame segment, 2.4 % of frames/s,
    profiles/r6/tail_ablation.txt).  The table of N device pointers has a fixed address - a captured graph bakes THAT in - and `set`
    rewrites its entries on the current stream with one tiny launch (lsfa_ptr_table_set); the images must stay alive and unchanged until
    the pass that reads them has run (the table keeps references until the next `set`)."""

    def __init__(self, n, c, h, w, device):
        self.shape = (int(n), int(c), int(h), int(w))
        self.device = torch.device(device)
        self.ptrs = torch.zeros(int(n), dtype=torch.int64, device=self.device)
        self.dtype, self.is_cuda = torch.float32, True
        self.held = None

    def dim(self):
        return 4

    def contiguous(self):
        return self

    def is_contiguous(self):
        return True

    def set(self, images):
        """images: N tensors (C, H, W) (or (1, C, H, W)), float32, contiguous, on this device"""
        n, c, h, w = self.shape
        images = list(images)
        if len(images) != n:
            raise LsfaError("ImageTable.set: %d images for a table of %d" % (len(images), n))
        for t in images:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != self.device or not t.is_contiguous() or t.numel() != c * h * w or \
                    tuple(t.shape[-3:]) != (c, h, w) or t.data_ptr() % 4:
                raise LsfaError("ImageTable.set: every image must be a contiguous float32 (%d, %d, %d) tensor on %s, got %s %s on %s" % (
                    c, h, w, self.device, tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t)), getattr(t, 'device', None)))
        arr = (ctypes.c_void_p * n)(*[t.data_ptr() for t in images])
        with torch.cuda.device(self.device):
            _check(lib().lsfa_ptr_table_set(_ptr(self.ptrs), n, arr, _stream()), "lsfa_ptr_table_set")
        self.held = images
        return self

    def materialize(self):
        """the images as one (N, C, H, W) tensor (a copy; for code paths that need a tensor)"""
        return torch.stack([t.reshape(self.shape[1:]) for t in self.held], 0)


@_on_tensor_device
def avgpool_nchw(x, k, out=None):
    """(N, C, H, W) float32 (or an ImageTable of N images) -> (N, C, ceil(H/k), ceil(W/k)): k x k / k average, edge windows clipped
    (lsfa_avgpool_nchw / lsfa_avgpool_nchw_tbl)."""
    tbl = isinstance(x, ImageTable)
    if not tbl:
        x = _input("avgpool_nchw", "x", x, ("N", "C", "H", "W"))
    N, C, H, W = x.shape
    Ho, Wo = -(-H // k), -(-W // k)
    if out is None:
        out = torch.empty((N, C, Ho, Wo), device=x.device, dtype=torch.float32)
    else:
        _tensor("avgpool_nchw", "output buffer out", out, torch.float32, (N, C, Ho, Wo), x.device)
    if tbl:
        with torch.cuda.device(x.device):
            _check(lib().lsfa_avgpool_nchw_tbl(_ptr(x.ptrs), N, C, H, W, k, _ptr(out), _stream()), "lsfa_avgpool_nchw_tbl")
        return out
    _check(lib().lsfa_avgpool_nchw(_ptr(x), N, C, H, W, k, _ptr(out), _stream()), "lsfa_avgpool_nchw")
    return out


@_on_tensor_device
def stem_weight_layout(weight):
    """conv0's (64, 3, 7, 7) weight (bn0 folded) -> the fragments lsfa_stem_conv7x7s2 reads (lsfa_stem_weights: a uint8 tensor of
    lsfa_stem_weight_bytes())."""
    if not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (64, 3, 7, 7) or not weight.is_cuda or not weight.is_floating_point():
        raise LsfaError("stem_weight_layout: expected a (64, 3, 7, 7) floating-point weight on a CUDA device, got %s" % _arrived(weight))
    w_l = weight.float().permute(1, 2, 3, 0).contiguous()
    frag = torch.empty((int(lib().lsfa_stem_weight_bytes()),), dtype=torch.uint8, device=weight.device)
    _check(lib().lsfa_stem_weights(_ptr(w_l), _ptr(frag), _stream()), "lsfa_stem_weights")
    return frag


@_on_tensor_device
def stem_conv(x, w_l, bias, in_scale=None, in_shift=None, out=None, accum=None, act=1, amax_out=None):
    """bn_data + conv0 (7x7, stride 2, pad 3) + bias (+ accum) + activation (0 none, 1 ReLU, 2 LeakyReLU 0.1):
    x (N, 3, H, W) NCHW -> (N, Ho, Wo, 64) channels-last.  amax_out: a zeroed row of amax_slots() for max|out|."""
    tbl = isinstance(x, ImageTable)      # the N images given by a table of device pointers (lsfa_stem_conv7x7s2_tbl)
    if not tbl:
        x = _input("stem_conv", "x", x, ("N", 3, "H", "W"))
    N, C, H, W = x.shape
    dev = x.device
    if C != 3:
        raise LsfaError("stem_conv: x must have 3 channels, the table holds images of %d" % C)
    _tensor("stem_conv", "w_l (from stem_weight_layout)", w_l, torch.uint8, (int(lib().lsfa_stem_weight_bytes()),), dev)
    bias = _vector("stem_conv", "bias", bias, 64, dev)
    in_scale, in_shift = _vector("stem_conv", "in_scale", in_scale, 3, dev), _vector("stem_conv", "in_shift", in_shift, 3, dev)
    amax_out = _amax_row("stem_conv", "amax_out", amax_out, dev)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is not None:
        _tensor("stem_conv", "output buffer out", out, torch.float32, (N, Ho, Wo, 64), dev)
    if accum is not None:
        _tensor("stem_conv", "accum (a map like the output; may be `out`)", accum, torch.float32, (N, Ho, Wo, 64), dev)
    if out is None:
        out = torch.empty((N, Ho, Wo, 64), device=x.device, dtype=torch.float32)
    if tbl:
        with torch.cuda.device(x.device):
            _check(lib().lsfa_stem_conv7x7s2_tbl(_ptr(x.ptrs), N, H, W, _ptr(in_scale), _ptr(in_shift), _ptr(w_l), _ptr(bias), _ptr(accum), act,
                                                 _ptr(out), _ptr(amax_out), _stream()), "lsfa_stem_conv7x7s2_tbl")
        return out
    _check(lib().lsfa_stem_conv7x7s2_ex(_ptr(x), N, H, W, _ptr(in_scale), _ptr(in_shift), _ptr(w_l), _ptr(bias), _ptr(accum), act, _ptr(out),
                                        _ptr(amax_out), _stream()), "lsfa_stem_conv7x7s2_ex")
    return out


@_on_tensor_device
def head_conv3x3(x, w, bias, cin=None, mul=1.0, out=None, c0=0, nchw=False):
    """lsfa_head_conv3x3: 3x3 / pad 1 convolution to <= 4 channels (FlowNet's flow heads).  x (N,H,W,L) channels-last, w (Cout,3,3,Cin);
    nchw: returns (N,Cout,H,W); else writes channels [c0, c0+Cout) of `out` (N,H,W,Lout) (a fresh (N,H,W,Cout) map by default)."""
    x = _input("head_conv3x3", "x", x, ("N", "H", "W", "L"))
    N, H, W, L = x.shape
    w = _input("head_conv3x3", "w", w, ("Cout", 3, 3, "Cin"), x.device)
    Cout, cin = w.shape[0], (w.shape[3] if cin is None else cin)
    if w.shape[3] != cin or cin > L:
        raise LsfaError("head_conv3x3: weight %s does not fit %d input channels of %d" % (tuple(w.shape), cin, L))
    bias = _vector("head_conv3x3", "bias", bias, Cout, x.device)
    if out is None:
        if c0 != 0:
            raise LsfaError("head_conv3x3: c0 = %r needs the `out` whose channels [c0, c0 + %d) it names" % (c0, Cout))
        out = torch.empty((N, Cout, H, W) if nchw else (N, H, W, Cout), device=x.device, dtype=torch.float32)
    else:
        _tensor("head_conv3x3", "output buffer out", out, torch.float32, (N, Cout, H, W) if nchw else (N, H, W, "Lout"), x.device)
        if not nchw and not 0 <= c0 <= out.shape[3] - Cout:
            raise LsfaError("head_conv3x3: channels [%d, %d) do not fit out %s" % (c0, c0 + Cout, tuple(out.shape)))
    _check(lib().lsfa_head_conv3x3(_ptr(x), L, N, H, W, cin, _ptr(w), _ptr(bias), Cout, mul, _ptr(out), int(nchw), out.shape[3] if not nchw else 0,
                                   c0, _stream()), "lsfa_head_conv3x3")
    return out


@_on_tensor_device
def upsample_flow(x, w, bias, out, c0, amax_out=None):
    """lsfa_upsample_flow: Deconvolution(4x4, stride 2) + Crop(offset 1) of a (N,Hi,Wi,C) flow into channels [c0, c0+C) of out (N,Hc,Wc,L)."""
    x = _input("upsample_flow", "x", x, ("N", "Hi", "Wi", "C"))
    N, Hi, Wi, C = x.shape
    w = _input("upsample_flow", "w", w, (C, C, 4, 4), x.device)
    bias = _vector("upsample_flow", "bias", bias, C, x.device)
    amax_out = _amax_row("upsample_flow", "amax_out", amax_out, x.device)
    _tensor("upsample_flow", "out", out, torch.float32, (N, "Hc", "Wc", "L"), x.device)
    if not 0 <= c0 <= out.shape[3] - C:
        raise LsfaError("upsample_flow: channels [%d, %d) do not fit out %s" % (c0, c0 + C, tuple(out.shape)))
    _check(lib().lsfa_upsample_flow(_ptr(x), N, Hi, Wi, C, _ptr(w), _ptr(bias), out.shape[1], out.shape[2], _ptr(out), out.shape[3], c0,
                                    _ptr(amax_out), _stream()), "lsfa_upsample_flow")
    return out


@_on_tensor_device
def nchw_to_nhwc(x, c0=0, c=None, out=None, amax_out=None):
    """channels [c0, c0 + c) of an (N, C, H, W) map -> (N, H, W, c) channels-last (lsfa_nchw_to_nhwc), into `out` when given (a contiguous
    (N, H, W, c) tensor or leading slice of one); amax_out: a zeroed row of amax_slots() that receives max|.| of the copied values."""
    x = _input("nchw_to_nhwc", "x", x, ("N", "C", "H", "W"))
    N, C, H, W = x.shape
    c = C - c0 if c is None else c
    if c0 < 0 or c < 1 or c0 + c > C:
        raise LsfaError("nchw_to_nhwc: channels [%d, %d) of a map of %d" % (c0, c0 + c, C))
    amax_out = _amax_row("nchw_to_nhwc", "amax_out", amax_out, x.device)
    if out is None:
        out = torch.empty((N, H, W, c), device=x.device, dtype=torch.float32)
    else:
        _tensor("nchw_to_nhwc", "output buffer out", out, torch.float32, (N, H, W, c), x.device)
    if 'nhwc' in LAB_SKIP and out.data_ptr() in _lab_filled:
        return out
    if LAB_SKIP:
        _lab_filled.add(out.data_ptr())
    _check(lib().lsfa_nchw_to_nhwc(_ptr(x), N, C, H * W, c0, c, _ptr(out), _ptr(amax_out), _stream()), "lsfa_nchw_to_nhwc")
    return out


def rfcn_head_ps_ld(ps_map, cell_ld, rois, H, W, ncls, nbox, spatial_scale=0.0625, pooled_size=7, group_size=7):
    """rfcn_head_ps on a position-sensitive map whose cells are `cell_ld` floats apart (N, H, W, cell_ld)."""
    ps_map = _input("rfcn_head_ps_ld", "ps_map (N, H, W, cell_ld)", ps_map, ("N", H, W, cell_ld))
    rois = _input("rfcn_head_ps_ld", "rois", rois, ("R", 5), ps_map.device)
    N, R = ps_map.shape[0], rois.shape[0]
    if cell_ld < group_size * group_size * (ncls + nbox):
        raise LsfaError("rfcn_head_ps_ld: cells of %d floats do not hold %d x (%d + %d) scores" % (cell_ld, group_size * group_size, ncls, nbox))
    cls_prob = torch.empty((R, ncls), device=rois.device, dtype=torch.float32)
    bbox_pred = torch.empty((R, nbox), device=rois.device, dtype=torch.float32)
    if LAB_SKIP_HEAD:
        return cls_prob, bbox_pred
    with torch.cuda.device(ps_map.device):
        _check(lib().lsfa_rfcn_head_ps_ld_fwd(_ptr(ps_map), cell_ld, _ptr(rois), N, H, W, R, ncls, nbox, spatial_scale, pooled_size, group_size,
                                              _ptr(cls_prob), None, _ptr(bbox_pred), _stream()), "lsfa_rfcn_head_ps_ld_fwd")
    return cls_prob, bbox_pred


@_on_tensor_device
def avgpool2_nhwc(x):
    """(N,H,W,C) -> (N,ceil(H/2),ceil(W/2),C), 2x2 / 2 average with clipped edge windows (lsfa_avgpool2_nhwc)."""
    x = _input("avgpool2_nhwc", "x", x, ("N", "H", "W", "C"))
    N, H, W, C = x.shape
    y = torch.empty((N, (H + 1) // 2, (W + 1) // 2, C), device=x.device, dtype=torch.float32)
    _check(lib().lsfa_avgpool2_nhwc(_ptr(x), N, H, W, C, _ptr(y), _stream()), "lsfa_avgpool2_nhwc")
    return y


@_on_tensor_device
def maxpool3x3s2_nhwc(x, out=None, scale2=None, shift2=None, amax_out=None):
    """(N, H, W, C) float32 channels-last -> (N, (H-1)//2+1, (W-1)//2+1, C): 3x3, stride 2, pad 1 max pooling.
    With scale2 / shift2 (C): returns (pooled, max(pooled*scale2 + shift2, 0)) — the first unit's bn1 + relu1 in the same launch.
    amax_out: a zeroed row of amax_slots() that receives the maximum of the map the next convolution reads (the second output
    when there is one)."""
    x = _input("maxpool3x3s2_nhwc", "x", x, ("N", "H", "W", "C"))
    N, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if (scale2 is None) != (shift2 is None):
        raise LsfaError("maxpool3x3s2_nhwc: scale2 and shift2 come together, got %s and %s" % (_arrived(scale2), _arrived(shift2)))
    scale2, shift2 = _vector("maxpool3x3s2_nhwc", "scale2", scale2, C, x.device), _vector("maxpool3x3s2_nhwc", "shift2", shift2, C, x.device)
    amax_out = _amax_row("maxpool3x3s2_nhwc", "amax_out", amax_out, x.device)
    if out is None:
        out = torch.empty((N, Ho, Wo, C), device=x.device, dtype=torch.float32)
    else:
        _tensor("maxpool3x3s2_nhwc", "output buffer out", out, torch.float32, (N, Ho, Wo, C), x.device)
    out2 = torch.empty_like(out) if scale2 is not None else None
    _check(lib().lsfa_maxpool3x3s2_nhwc(_ptr(x), N, H, W, C, _ptr(out), _ptr(out2), _ptr(scale2), _ptr(shift2), _ptr(amax_out), _stream()),
           "lsfa_maxpool3x3s2_nhwc")
    return out if out2 is None else (out, out2)


# SplitWeight's default form: three bf16 pieces (exact cut, no scale needed).  The frame path binds its fp32 convolutions with
# pieces=2 (two fp16 pieces + a scale, three products) and its bf16 mode with pieces=1 (lsfa_amd/symbols).
DEFAULT_PIECES = 3
AMAX_SLOTS = 256


def _fp16_exponent(amax):
    """THE exponent rule of the fp16 two-piece form: amax (a float64 tensor of maxima: one per tensor or one per output channel) -> int32
    exponents e with amax * 2^e in [2^13, 2^14); 0 for a zero or non-finite maximum (an all-zero padding channel), clamped to +-100"""
    ok = torch.isfinite(amax) & (amax > 0)
    e = torch.where(ok, 13 - torch.floor(torch.log2(torch.where(ok, amax, torch.ones_like(amax)))), torch.zeros_like(amax))
    return e.clamp(-100, 100).to(torch.int32)


def _fp16_weight_exponent(fn, amax):
    """_fp16_exponent for a weight at bind time (a host synchronisation is fine here).  A maximum of 2^114 or more is refused: the clamp at
    -100 would leave the scaled maximum above [2^13, 2^14), towards fp16's overflow - better an error here than a status bit at run time."""
    if bool((torch.isfinite(amax) & (amax >= 2.0 ** 114)).any()):
        raise LsfaError("%s: the fp16 two-piece form takes weights below 2^114, the largest here is %g" % (fn, float(amax[torch.isfinite(amax)].max())))
    return _fp16_exponent(amax)


class SplitWeight(object):
    """A convolution weight cut into `pieces` pieces per value and laid out in MFMA fragment order (lsfa_conv_weights); made once per
    layer at bind time.  pieces = 2: the values are scaled by 2^w_exp so that the largest lands in [2^13, 2^14) (_fp16_exponent; a maximum of
    2^114 or more raises LsfaError).
    Every instance carries pieces, cout, cin, kh, kw, real_cout, real_cin, w_exp (0 unless one exponent scales the whole tensor), w_scale
    (None unless each output channel has its own), frag (None only for pieces == 0) and w_kc (None unless pieces == 0)."""

    def __init__(self, weight, real_cout=None, real_cin=None, into=None, pieces=None, per_channel_scale=True, w_exp=None):
        """weight: (Cout, Cin, kh, kw) float32 CUDA tensor (the framework's layout).  real_cout / real_cin: the layer's own
        channel counts when `weight` was zero-padded to the kernel's tile sizes (algorithmic FLOPs are counted on those).
        into: the fragments' storage (a slice of a shared allocation); w_exp: the two-piece form's exponent when the caller knows it (one
        shared by several weights: deconv_phase_weights) - then the tensor is not measured and carries no per-channel scale."""
        _input("SplitWeight", "weight", weight, ("Cout", "Cin", "kh", "kw"))
        w_kc = conv_weight_kc(weight)
        self.pieces = int(DEFAULT_PIECES if pieces is None else pieces)
        self.cout, self.cin, self.kh, self.kw = [int(v) for v in weight.shape]
        self.real_cout, self.real_cin = int(real_cout or self.cout), int(real_cin or self.cin)
        self.w_exp, self.w_scale, self.frag, self.w_kc = 0, None, None, None
        if self.pieces == 0:
            # r5, the exact-fp32 evaluation (a REFERENCE mode for tests and one bench line, LSFA_CONV_PIECES=0): the weight stays fp32 in the
            # (Cout, taps, Cin) layout lsfa_conv_nhwc_fused_fwd reads; conv_split / conv_split_view dispatch on pieces == 0 (_conv_exact)
            if self.cin % 32 or self.cout % 64:
                raise LsfaError("SplitWeight: Cin=%d must be a multiple of 32, Cout=%d of 64" % (self.cin, self.cout))
            self.w_kc = w_kc
            return
        need = lib().lsfa_conv_weight_bytes(self.cout, self.kh, self.kw, self.cin, self.pieces)
        if need == 0:
            raise LsfaError("SplitWeight: Cin=%d must be a multiple of 32, Cout=%d of 64, pieces=%d one of 1, 2, 3" % (self.cin, self.cout, self.pieces))
        if into is not None:
            _tensor("SplitWeight", "into (the fragments' storage)", into, torch.uint8, (need,), weight.device)
        self.frag = torch.empty(need, dtype=torch.uint8, device=weight.device) if into is None else into
        if self.pieces == 2 and per_channel_scale and w_exp is None:
            # r5: one power of two per OUTPUT channel, from the channel's own maximum (a BatchNorm folded into trained weights spreads the
            # channels over many octaves: with one scale per tensor the small channels' lo pieces go subnormal).  An all-zero (padding)
            # channel gets exponent 0.
            e = _fp16_weight_exponent("SplitWeight", weight.detach().abs().reshape(self.cout, -1).amax(1).double()).contiguous()
            self.w_scale = torch.ldexp(torch.ones(self.cout, dtype=torch.float32, device=weight.device), -e).contiguous()
            with torch.cuda.device(weight.device):
                _check(lib().lsfa_conv_weights_pc(_ptr(w_kc), self.cout, self.kh, self.kw, self.cin, _ptr(e), _ptr(self.frag), _stream()),
                       "lsfa_conv_weights_pc")
            return
        if self.pieces == 2:      # one exponent for the tensor: the caller's, or from its maximum (bind time: a host synchronisation is fine here)
            self.w_exp = int(_fp16_weight_exponent("SplitWeight", weight.detach().abs().max().double()).item() if w_exp is None else w_exp)
        with torch.cuda.device(weight.device):
            _check(lib().lsfa_conv_weights(_ptr(w_kc), self.cout, self.kh, self.kw, self.cin, self.pieces, self.w_exp, _ptr(self.frag), _stream()),
                   "lsfa_conv_weights")


@_on_tensor_device
def amax_partial(x, out=None):
    """lsfa_amax_partial: 256 partial maxima of |x| (float32, contiguous, numel % 4 == 0): an `amax_in` for a map that no convolution
    of this library produced (those leave theirs in `amax_out`)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda:
        raise LsfaError("amax_partial: x must be a float32 CUDA tensor, got %s" % _arrived(x))
    x = x if x.is_contiguous() else x.contiguous()
    if out is None:
        out = torch.empty(AMAX_SLOTS, device=x.device, dtype=torch.float32)
    else:
        _tensor("amax_partial", "output buffer out", out, torch.float32, (AMAX_SLOTS,), x.device)
    _check(lib().lsfa_amax_partial(_ptr(x), x.numel(), _ptr(out), _stream()), "lsfa_amax_partial")
    return out


def _zeros(shape, dtype, device):
    """torch.zeros cleared by lsfa_copy_many's zero-fill job on the current stream: no PyTorch kernel in a captured frame section"""
    t = torch.empty(shape, dtype=dtype, device=device)
    if t.is_cuda:
        with torch.cuda.device(t.device):
            copy_many([(t, None)])
    else:
        t.zero_()
    return t


def amax_slots(n, device):
    """n zeroed amax_out slot arrays (n, 256) - uint32 bit patterns of non-negative floats, readable as float32 through .view()"""
    return _zeros((n, AMAX_SLOTS), torch.int32, device)


def zeros_f32(shape, device):
    """torch.zeros(shape, float32) (see _zeros)"""
    return _zeros(shape, torch.float32, device)


def new_status(device):
    return torch.zeros(4, dtype=torch.int32, device=device)


@_on_tensor_device
def check_status(status):
    """lsfa_status_check: raises LsfaError if a convolution raised the status word (non-finite output: the fp16 form's scale was an
    under-estimate, or the input held inf / NaN).  Synchronises the current stream."""
    _tensor("check_status", "status (a new_status() word)", status, torch.int32, (4,))
    if LAB_SKIP:      # an ablation run's maps are garbage by construction
        return
    _check(lib().lsfa_status_check(_ptr(status), _stream()), "lsfa_status_check")


def _conv_desc(x, sw, N, H, W, y_ptr, x_offset=0, lda=0, cin=None, ldy=0, bias=None, stride=1, pad=(0, 0), dil=1, act=0, nchw=False, residual=None,
               out2=None, scale2=None, shift2=None, amax_in=None, amax_out=None, status=None, grid=(0, 0), view=(0, 0, 0, 0), prof_tag=0,
               x_nchw=False, in_scale=None, in_shift=None):
    """struct lsfa_conv_desc of one launch; what a caller leaves out keeps the header's default (0 / NULL: whole channel rows, the
    convolution's own output grid, no view)"""
    d = ConvDesc()
    d.x, d.lda, d.N, d.H, d.W, d.Cin = x.data_ptr() + x_offset, lda, N, H, W, sw.cin if cin is None else cin
    d.wfrag, d.pieces, d.w_exp, d.amax_in = _ptr(sw.frag), sw.pieces, sw.w_exp, _ptr(amax_in)
    d.bias, d.Cout, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.dil = _ptr(bias), sw.cout, sw.kh, sw.kw, stride, pad[0], pad[1], dil
    d.act, d.y_nchw, d.residual, d.y, d.ldy = int(act), int(nchw), _ptr(residual), y_ptr, ldy
    d.y2, d.scale2, d.shift2, d.amax_out, d.status = _ptr(out2), _ptr(scale2), _ptr(shift2), _ptr(amax_out), _ptr(status)
    d.Ho, d.Wo = grid
    d.out_H, d.out_W, d.out_sy, d.out_sx = view
    d.prof_tag, d.x_nchw = prof_tag, int(x_nchw)
    d.in_scale, d.in_shift, d.w_scale = _ptr(in_scale), _ptr(in_shift), _ptr(sw.w_scale)
    return d


def _conv_launch(who, x, sw, N, H, W, y_ptr, **desc):
    """lsfa_conv_fwd on the descriptor _conv_desc(x, sw, N, H, W, y_ptr, **desc) with its workspace.  Everything that goes through
    lsfa_conv_fwd is counted for bench.py's roofline HERE: FLOPs on the layer's own channel counts; bytes: every operand once, on the
    channels the launch reads and writes."""
    if sw.pieces == 2 and desc.get("amax_in") is None:
        desc["amax_in"] = amax_partial(x)      # no producer left the map's maximum: measured here (the whole map bounds the channels a view reads)
    d = _conv_desc(x, sw, N, H, W, y_ptr, **desc)
    need = lib().lsfa_conv_workspace_bytes(ctypes.byref(d))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    if _conv_flops["count"]:
        Ho, Wo = (d.Ho, d.Wo) if d.Ho > 0 else conv_out_hw(H, W, sw.kh, sw.kw, d.stride, (d.pad_h, d.pad_w), d.dil)
        outs = 1 + (1 if d.residual else 0) + (1 if d.y2 else 0)
        nbytes = 4.0 * N * H * W * d.Cin + 2.0 * sw.pieces * sw.cout * sw.kh * sw.kw * d.Cin + 4.0 * outs * N * Ho * Wo * sw.cout
        _count_launch(_plan_kernel_name(d), 2.0 * N * Ho * Wo * sw.real_cout * sw.real_cin * sw.kh * sw.kw, nbytes, sw.pieces)
    _check(lib().lsfa_conv_fwd(ctypes.byref(d), _ptr(ws), need, _stream()), who)


def _conv_exact(x, sw, bias, stride=1, pad=0, dil=1, act=0, out=None, residual=None, out2=None, scale2=None, shift2=None, nchw=False,
                x_nchw=False, in_scale=None, in_shift=None):
    """conv_split's contract on the EXACT fp32 matrix instructions (lsfa_conv_nhwc_fused_fwd: v_mfma_f32_32x32x2_f32, every product an fp32
    product, bitwise an fmaf chain) - a reference evaluation, not a fast path: ONE conv_nhwc call; what the channels-last kernel does not
    take (NCHW in / out, the input's bn + ReLU at the cut, LeakyReLU, a second output that is only measured) is done by separate
    elementwise steps around it, with the same fp32 operations in the same order as the split kernels' epilogues."""
    if x_nchw:
        x = x[:, :sw.cin].permute(0, 2, 3, 1).contiguous()
    if in_scale is not None:
        x = torch.relu(x * in_scale + in_shift)                       # max(v * scale + shift, 0): two roundings, like affine_relu4
    if nchw and residual is not None:
        residual = residual.permute(0, 2, 3, 1).contiguous()
    whole = not nchw and act != 2      # the kernel writes the caller's tensors itself, the second output included
    o2 = out2 if whole else None
    y = conv_nhwc(x, sw.w_kc, bias, sw.kh, sw.kw, stride, pad, dil, relu=(act == 1), out=out if whole else None, residual=residual,
                  out2=o2, scale2=None if o2 is None else scale2, shift2=None if o2 is None else shift2)
    if whole:
        return y
    if act == 2:
        y = torch.where(y > 0, y, y * 0.1)
    if nchw:
        y = y.permute(0, 3, 1, 2).contiguous()
    if out is not None:
        out.copy_(y)
        y = out
    if nchw and out2 is not None:
        out2.copy_(torch.relu(y * scale2.view(1, -1, 1, 1) + shift2.view(1, -1, 1, 1)))
        return y, out2
    return y


def _split_weight(who, what, sw, device=None):
    """sw, if it is a SplitWeight whose storage lies on `device`"""
    t = getattr(sw, 'w_kc', None) if getattr(sw, 'pieces', None) == 0 else getattr(sw, 'frag', None)
    if not isinstance(sw, SplitWeight) or not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device):
        raise LsfaError("%s: %s must be a SplitWeight on %s, got %s" % (who, what, device or "a CUDA device", type(sw).__name__))
    return sw


@_on_tensor_device
def conv_split(x, sw, bias=None, stride=1, pad=0, dil=1, relu=False, out=None, residual=None, out2=None, scale2=None,
               shift2=None, nchw=False, act=None, amax_in=None, amax_out=None, status=None, x_nchw=False, in_scale=None, in_shift=None):
    """lsfa_conv_fwd: convolution with fp32 in / out and split operands on the matrix pipe; sw: SplitWeight (its `pieces` picks the form).
    x (N, H, W, Cin) contiguous fp32 -> (N, Ho, Wo, Cout), or (N, Cout, Ho, Wo) with nchw=True (then residual / out2 are NCHW too).
    residual (same shape as the output; may BE `out`): added before the activation / store.  out2 + scale2 + shift2: second output
    max(out*scale2[c] + shift2[c], 0) (the next ResNet unit's bn1 + relu1).  act: 0 none, 1 ReLU, 2 LeakyReLU(0.1) (relu=True = act 1).
    amax_in: 256 partial maxima (float32 or int32 bit patterns) bounding |x| - required for two-piece weights; amax_out: 256 int32 slots that
    receive max|out2| (or max|out|); status: the int32 status word.  scale2 + shift2 WITHOUT out2: the second output is not stored, only its
    maximum published (amax_out) - for a consumer that applies the same affine + ReLU itself through in_scale / in_shift (Cin floats each:
    the input becomes max(x*in_scale[k] + in_shift[k], 0) where it is cut; 1x1, pad 0, two-piece or one-piece weights; amax_in must bound
    the ACTIVATED input).  Returns out, or (out, out2)."""
    x = _input("conv_split", "x", x, ("N", "C", "H", "W") if x_nchw else ("N", "H", "W", "Cin"))
    dev = x.device
    _split_weight("conv_split", "sw", sw, dev)
    if x_nchw:
        # the input is channels [0, sw.cin) of an NCHW map (N, Ctot, H, W): 1x1 / stride 1 / no padding, small weights (the RPN head)
        N, Ctot, H, W = x.shape
        Cin = sw.cin
        if Ctot < Cin or (sw.kh, sw.kw, stride, pad, dil) != (1, 1, 1, 0, 1):
            raise LsfaError("conv_split: x_nchw needs a 1x1 / stride 1 / pad 0 convolution on at least %d channels" % Cin)
    else:
        N, H, W, Cin = x.shape
        Ctot = Cin
    if Cin != sw.cin:
        raise LsfaError("conv_split: input has %d channels, the weight %d" % (Cin, sw.cin))
    Cout, act = sw.cout, ((1 if relu else 0) if act is None else act)      # lsfa_conv_desc::act; `act` wins over relu=
    Ho, Wo = conv_out_hw(H, W, sw.kh, sw.kw, stride, (pad, pad), dil)
    _check_outputs("conv_split", N * Ho * Wo * Cout, dev, out=out, residual=residual, out2=out2)
    bias = _vector("conv_split", "bias", bias, Cout, dev)
    scale2, shift2 = _vector("conv_split", "scale2", scale2, Cout, dev), _vector("conv_split", "shift2", shift2, Cout, dev)
    in_scale, in_shift = _vector("conv_split", "in_scale", in_scale, Cin, dev), _vector("conv_split", "in_shift", in_shift, Cin, dev)
    amax_in, amax_out = _amax_row("conv_split", "amax_in", amax_in, dev, measured=True), _amax_row("conv_split", "amax_out", amax_out, dev)
    status = _status_word("conv_split", status, dev)
    if out is None:
        out = torch.empty((N, Cout, Ho, Wo) if nchw else (N, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    if sw.pieces == 0:
        return _conv_exact(x, sw, bias, stride, pad, dil, act, out=out, residual=residual, out2=out2, scale2=scale2, shift2=shift2, nchw=nchw,
                           x_nchw=x_nchw, in_scale=in_scale, in_shift=in_shift)
    _conv_launch("lsfa_conv_fwd", x, sw, N, H, W, out.data_ptr(), lda=Ctot, ldy=Cout, bias=bias, stride=stride, pad=(pad, pad), dil=dil, act=act,
                 nchw=nchw, residual=residual, out2=out2, scale2=scale2, shift2=shift2, amax_in=amax_in, amax_out=amax_out, status=status,
                 x_nchw=x_nchw, in_scale=in_scale, in_shift=in_shift)
    return out if out2 is None else (out, out2)


@_on_tensor_device
def conv_pair(x, sw3, residual, scale2, shift2, sw1, bias=None, out=None, out_z=None, amax_in=None, amax_out_sum=None, amax_out_z=None,
              status=None, stride=1, nchw=False):
    """lsfa_conv_pair_fwd: a ResNet unit's conv3 + shortcut add and the next unit's conv1 (+ bias + ReLU) in one launch.
    x (N, H, W, Cm) contiguous fp32 (c2); sw3 (C = 4 Cm outputs) and sw1 (C -> Cn) two-piece SplitWeights with per-channel scales;
    residual (N, H, W, C), may BE `out`.  -> (y, z): y = conv3(x) + residual (bit-identical to conv_split's), z = max(conv1(max(y * scale2 +
    shift2, 0)) + bias, 0); the activated map is never stored.  amax_out_sum receives its maximum, amax_out_z that of z.  Channel counts
    outside Cm, Cn in {64, 128}, other piece counts, non-contiguous operands, NCHW or a stride raise LsfaError (LSFA_ENOTSUP)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise LsfaError("conv_pair: x must be a (N, H, W, Cm) float32 CUDA tensor, got %s" % _arrived(x))
    N, H, W, Cm = x.shape
    dev = x.device
    _split_weight("conv_pair", "sw3", sw3, dev), _split_weight("conv_pair", "sw1", sw1, dev)
    C, Cn = sw3.cout, sw1.cout
    if (sw3.kh, sw3.kw, sw1.kh, sw1.kw) != (1, 1, 1, 1) or sw3.cin != Cm or sw1.cin != C:
        raise LsfaError("conv_pair: two 1x1 convolutions Cm=%d -> C -> Cn, not %dx%d %d -> %d and %dx%d %d -> %d"
                        % (Cm, sw3.kh, sw3.kw, sw3.cin, C, sw1.kh, sw1.kw, sw1.cin, Cn))
    two = sw3.pieces == 2 and sw1.pieces == 2      # (any other piece count is refused by the library)
    if two and (sw3.w_scale is None or sw1.w_scale is None):
        raise LsfaError("conv_pair: the weights must carry per-channel scales (SplitWeight(per_channel_scale=True))")
    for name, t, c in (("out", out, C), ("residual", residual, C), ("out_z", out_z, Cn)):
        if (t is None and name == "residual") or (t is not None and (not isinstance(t, torch.Tensor) or t.numel() != N * H * W * c or
                                                                      t.dtype != torch.float32 or t.device != dev or not t.is_contiguous())):
            raise LsfaError("conv_pair: %s must be a contiguous float32 tensor of %d elements on %s, got %s" % (name, N * H * W * c, dev, _arrived(t)))
    for name, t, c in (("scale2", scale2, C), ("shift2", shift2, C), ("bias", bias, Cn)):
        if (t is None and name != "bias") or (t is not None and (not isinstance(t, torch.Tensor) or t.numel() != c or t.dtype != torch.float32 or
                                                                  t.device != dev or not t.is_contiguous())):
            raise LsfaError("conv_pair: %s must be a contiguous float32 tensor of %d elements on %s, got %s" % (name, c, dev, _arrived(t)))
    amax_in = _amax_row("conv_pair", "amax_in", amax_in, dev, measured=True)
    amax_out_sum, amax_out_z = _amax_row("conv_pair", "amax_out_sum", amax_out_sum, dev), _amax_row("conv_pair", "amax_out_z", amax_out_z, dev)
    status = _status_word("conv_pair", status, dev)
    if amax_in is None:
        amax_in = amax_partial(x)
    if out is None:
        out = torch.empty((N, H, W, C), device=x.device, dtype=torch.float32)
    if out_z is None:
        out_z = torch.empty((N, H, W, Cn), device=x.device, dtype=torch.float32)
    # a view is described to the library by its pixel pitch (which then refuses it): dense operands have pitch = channel count
    ldx = x.stride(2) if x.stride(3) == 1 else 0
    ldy = out.stride(-2) if out.stride(-1) == 1 and out.dim() == 4 else C
    ldz = out_z.stride(-2) if out_z.stride(-1) == 1 and out_z.dim() == 4 else Cn
    if not residual.is_contiguous():
        raise LsfaError("conv_pair: residual, scale2 and shift2 must be contiguous")
    if _conv_flops["count"] and two:
        P = N * H * W
        # each operand once: c2, the residual, the sum, z and both weight blocks (two fp16 pieces per weight)
        _count_launch("conv_pair_kernel<%d, %d>" % (Cm // 32, Cn // 32), 2.0 * P * (Cm * C + C * Cn),
                      4.0 * P * (Cm + 2 * C + Cn) + 4.0 * (Cm * C + C * Cn), 2)
    _check(lib().lsfa_conv_pair_fwd(x.data_ptr(), ldx, N, H, W, Cm, _ptr(amax_in), _ptr(sw3.frag), _ptr(sw3.w_scale), sw3.pieces, C,
                                    _ptr(residual), out.data_ptr(), ldy, _ptr(scale2), _ptr(shift2), _ptr(sw1.frag),
                                    _ptr(sw1.w_scale), sw1.pieces, Cn, _ptr(bias), out_z.data_ptr(), ldz, int(stride), int(nchw),
                                    _ptr(amax_out_sum), _ptr(amax_out_z), _ptr(status), _stream()), "lsfa_conv_pair_fwd")
    return out, out_z


@_on_tensor_device
def conv_split_view(x, sw, bias, out, stride=1, pad=(0, 0), dil=1, act=0, cin=None, c0=0, grid=None, place=None, amax_in=None,
                    amax_out=None, status=None, cin0=0):
    """lsfa_conv_fwd between VIEWS of wider channels-last maps.
    x    (N, H, W, L) contiguous fp32, the convolution reads channels [cin0, cin0 + cin) of it (cin = sw.cin by default, L >= cin0 + cin;
         cin0 a multiple of 4: the operand pointer stays 16-byte aligned);
    out  (N, Hout, Wout, Lout) contiguous fp32: the result goes to channels [c0, c0 + sw.cout) of it;
    grid (Ho, Wo): the output grid of this launch when smaller than the convolution's; place (y0, x0, sy, sx): output pixel
         (oy, ox) is written to out[:, y0 + oy*sy, x0 + ox*sx] (default: out[:, oy, ox]) - a phase of a transposed convolution;
    pad  (pad_h, pad_w); act 0 none / 1 ReLU / 2 LeakyReLU(0.1)."""
    x = _input("conv_split_view", "x", x, ("N", "H", "W", "L"))
    N, H, W, L = x.shape
    dev = x.device
    _split_weight("conv_split_view", "sw", sw, dev)
    _tensor("conv_split_view", "out", out, torch.float32, (N, "Hout", "Wout", "Lout"), dev)
    bias = _vector("conv_split_view", "bias", bias, sw.cout, dev)
    amax_in = _amax_row("conv_split_view", "amax_in", amax_in, dev, measured=True)
    amax_out, status = _amax_row("conv_split_view", "amax_out", amax_out, dev), _status_word("conv_split_view", status, dev)
    cin = sw.cin if cin is None else cin
    if cin != sw.cin or L < cin0 + cin or cin0 < 0 or cin0 % 4:
        raise LsfaError("conv_split_view: the weight has %d input channels, x offers [%d, %d) (of %d)" % (sw.cin, cin0, cin0 + cin, L))
    if c0 < 0 or c0 + sw.cout > out.shape[3] or out.shape[0] != N:
        raise LsfaError("conv_split_view: channels [%d, %d) do not fit out %s" % (c0, c0 + sw.cout, tuple(out.shape)))
    Ho, Wo = grid if grid is not None else conv_out_hw(H, W, sw.kh, sw.kw, stride, pad, dil)
    y0, x0, sy, sx = place if place is not None else (0, 0, 1, 1)
    Hout, Wout, Lout = out.shape[1], out.shape[2], out.shape[3]
    if y0 + (Ho - 1) * sy >= Hout or x0 + (Wo - 1) * sx >= Wout:
        raise LsfaError("conv_split_view: a %dx%d grid placed at (%d,%d) step (%d,%d) leaves out %s" % (Ho, Wo, y0, x0, sy, sx, tuple(out.shape)))
    if sw.pieces == 0:      # the exact-fp32 reference mode (_conv_exact): plain output grids only (the transposed convolutions keep three bf16 pieces)
        if grid is not None or place is not None or (Ho, Wo) != (Hout, Wout):
            raise LsfaError("conv_split_view: the exact-fp32 mode takes whole output grids only")
        if pad[0] != pad[1]:
            raise LsfaError("conv_split_view: the exact-fp32 mode needs pad_h == pad_w")
        xin = x if (L == cin and cin0 == 0) else x[..., cin0:cin0 + cin].contiguous()
        out[..., c0:c0 + sw.cout] = _conv_exact(xin, sw, bias, stride, pad[0], dil, act)
        return out
    first = out.data_ptr() + 4 * ((y0 * Wout + x0) * Lout + c0)
    view = place is not None or (Ho, Wo) != (Hout, Wout)
    _conv_launch("lsfa_conv_fwd (view)", x, sw, N, H, W, first, x_offset=4 * cin0, lda=L, ldy=Lout, bias=bias, stride=stride, pad=pad, dil=dil, act=act,
                 amax_in=amax_in, amax_out=amax_out, status=status, grid=(Ho, Wo), view=(Hout if view else 0, Wout, sy, sx), prof_tag=1)
    return out


class PhaseWeights(list):
    """The four phase weights of a Deconvolution(4x4, stride 2) as SplitWeight views of ONE allocation (`frag4`)."""


def deconv_phase_weights(wt, cin_pad=None, pieces=None):
    """wt: MXNet Deconvolution weight (Cin, Cout, 4, 4) -> PhaseWeights for lsfa_deconv4x4s2_crop_fwd (input channels zero-padded to
    cin_pad).  Output row 2m + py of the cropped map reads input rows (m - 1, m) through taps ky = (3, 1) when py = 0 and rows
    (m, m + 1) through ky = (2, 0) when py = 1; columns alike.  With two pieces all four phases share ONE weight scale (w_exp)."""
    _input("deconv_phase_weights", "wt", wt, ("Cin", "Cout", 4, 4))      # (read by torch here: only the phase weights go to the library)
    cin, cout = int(wt.shape[0]), int(wt.shape[1])
    cpad = int(cin_pad or cin)
    pieces = int(DEFAULT_PIECES if pieces is None else pieces)
    if pieces == 0:
        pieces = 3      # exact-fp32 reference mode: the four-phase launch exists on the split kernels only; three bf16 pieces cut the operands exactly
    per = lib().lsfa_conv_weight_bytes(cout, 2, 2, cpad, pieces)
    if per == 0:
        raise LsfaError("deconv_phase_weights: Cin=%d must be a multiple of 32 and Cout=%d of 64" % (cpad, cout))
    frag4 = torch.empty(4 * per, dtype=torch.uint8, device=wt.device)
    out = PhaseWeights()
    # the four phases together hold every tap of wt exactly once: its maximum is each phase's bound (one host synchronisation)
    w_exp = int(_fp16_weight_exponent("deconv_phase_weights", wt.detach().abs().max().double()).item()) if pieces == 2 else 0
    for py in (0, 1):
        for px in (0, 1):
            kys, kxs = ((3, 1) if py == 0 else (2, 0)), ((3, 1) if px == 0 else (2, 0))
            wp = torch.zeros((cout, cpad, 2, 2), device=wt.device, dtype=torch.float32)
            wp[:, :cin] = wt[:, :, kys, :][:, :, :, kxs].permute(1, 0, 2, 3)
            out.append(SplitWeight(wp, real_cin=cin, into=frag4[len(out) * per:(len(out) + 1) * per], pieces=pieces, w_exp=w_exp))
    out.frag4, out.pieces, out.w_exp = frag4, pieces, w_exp
    return out


@_on_tensor_device
def deconv4x4s2_crop(x, sw4, bias, out, c0=0, act=0, amax_in=None, amax_out=None, status=None):
    """lsfa_deconv4x4s2_crop_fwd: Deconvolution(4x4, stride 2) + Crop(offset 1) + bias + activation as one launch.
    x (N, Hi, Wi, L) channels-last (the weights' Cin channels read, L >= Cin); sw4: deconv_phase_weights(...); the result fills
    channels [c0, c0 + Cout) of out (N, Hc, Wc, Lout)."""
    x = _input("deconv4x4s2_crop", "x", x, ("N", "Hi", "Wi", "L"))
    N, Hi, Wi, L = x.shape
    dev = x.device
    frags = getattr(sw4, 'frag4', None)
    if not isinstance(sw4, PhaseWeights) or not isinstance(frags, torch.Tensor) or frags.device != dev:
        raise LsfaError("deconv4x4s2_crop: the phase weights must come from hip.deconv_phase_weights (one allocation) on %s, got %s" %
                        (dev, type(sw4).__name__))
    cin, cout = sw4[0].cin, sw4[0].cout
    if len(sw4) != 4 or any((s.cin, s.cout, s.kh, s.kw) != (cin, cout, 2, 2) for s in sw4) or cin > L:
        raise LsfaError("deconv4x4s2_crop: four (Cout, Cin, 2, 2) phase weights with Cin <= %d expected" % L)
    _tensor("deconv4x4s2_crop", "out", out, torch.float32, (N, "Hc", "Wc", "Lout"), dev)
    if c0 < 0 or c0 + cout > out.shape[3]:
        raise LsfaError("deconv4x4s2_crop: bad out %s for channels [%d, %d)" % (tuple(out.shape), c0, c0 + cout))
    Hc, Wc, Lout = out.shape[1], out.shape[2], out.shape[3]
    bias = _vector("deconv4x4s2_crop", "bias", bias, cout, dev)
    amax_in = _amax_row("deconv4x4s2_crop", "amax_in", amax_in, dev, measured=True)
    amax_out, status = _amax_row("deconv4x4s2_crop", "amax_out", amax_out, dev), _status_word("deconv4x4s2_crop", status, dev)
    if amax_in is None and sw4.pieces == 2:
        amax_in = amax_partial(x)
    need = lib().lsfa_deconv4x4s2_crop_workspace_bytes(N, Hi, Wi, cin, cout, Hc, Wc, sw4.pieces)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    if _conv_flops["count"]:         # four phases, ONE launch
        _count_launch("conv_ring_kernel (the four phases of a stride-2 transposed convolution)",
                      sum(2.0 * N * ((Hc + 1) // 2) * ((Wc + 1) // 2) * s.real_cout * s.real_cin * 4 for s in sw4),
                      4.0 * N * Hi * Wi * cin + 4 * 2.0 * sw4.pieces * cout * 4 * cin + 4.0 * N * Hc * Wc * cout, sw4.pieces)
    _check(lib().lsfa_deconv4x4s2_crop_fwd(_ptr(x), L, N, Hi, Wi, cin, _ptr(frags), sw4.pieces, sw4.w_exp, _ptr(amax_in), _ptr(bias), cout, act,
                                           out.data_ptr() + 4 * c0, Lout, Hc, Wc, _ptr(amax_out), _ptr(status), _ptr(ws), need, _stream()),
           "lsfa_deconv4x4s2_crop_fwd")
    return out


def conv_plan_override(kernel=0, nt=0, st=0, slices=0):
    """lsfa_conv_plan_override (lab): force the ring kernel (kernel=1), its tile width / ring depth / K slices; zeros = the plan decides"""
    _check(lib().lsfa_conv_plan_override(kernel, nt, st, slices), "lsfa_conv_plan_override")


def conv_order_override(tile_order=-1, k_order=-1):
    """lsfa_conv_order_override (lab / tests): workgroup -> tile numbering (0 pixel tile fastest, 1 channel tile fastest) and the ring kernel's walk
    of K (0 tap by tap, 1 channel chunk by channel chunk); -1 = the default"""
    _check(lib().lsfa_conv_order_override(tile_order, k_order), "lsfa_conv_order_override")


class MotionVectorAccumulator(object):
    """Accumulated compressed-domain motion vectors of one GOP on the device
    (coviar_data_loader.c:71-177 with accumulate = 1; see lsfa_mv_* in include/lsfa_hip.h).

        acc = MotionVectorAccumulator(width, height, device)     # identity: the GOP's I-frame
        acc.add_frame(mvs)          # one P-frame's blocks, (n,7) int32 {source,w,h,src_x,src_y,dst_x,dst_y}
        acc.motion_vectors()        # (H,W,2) int32, what load(..., representation=MV, accumulate=True) returns
        acc.residual(bgr_cur, bgr_ref)   # (H,W,3) int32

    motion_vectors and residual write into `out`, a contiguous int32 tensor of that shape on the device, where one is given."""

    def __init__(self, width, height, device='cuda:0'):
        self.width, self.height, self.device = int(width), int(height), torch.device(device)
        self._bufs = [torch.empty((height, width, 2), dtype=torch.int32, device=self.device) for _ in range(2)]
        self._ws = torch.empty(lib().lsfa_mv_workspace_bytes(width, height), dtype=torch.uint8, device=self.device)
        self._cur = 0
        self.reset()

    @property
    def accu(self):
        return self._bufs[self._cur]

    def reset(self):
        with torch.cuda.device(self.device):
            _check(lib().lsfa_mv_identity(_ptr(self._bufs[self._cur]), self.width, self.height, _stream()), "lsfa_mv_identity")

    def add_frame(self, mvs, max_block_area=None):
        """mvs (n, 7) int32.  max_block_area: an upper bound of w*h over the blocks (256 for 16x16 macroblocks);
        when omitted it is read from `mvs`, which costs a device-to-host synchronisation if mvs is on the device."""
        if not isinstance(mvs, torch.Tensor) or mvs.dtype != torch.int32 or mvs.dim() != 2 or mvs.shape[1] != 7:
            raise LsfaError("MotionVectorAccumulator.add_frame: mvs must be (n, 7) int32, got %s" % _arrived(mvs))
        n = mvs.shape[0]
        if max_block_area is not None:
            area = int(max_block_area)
        else:
            area = int((mvs[:, 1].clamp(min=0).long() * mvs[:, 2].clamp(min=0).long()).max().item()) if n else 0
        mvs = mvs.to(self.device).contiguous()
        old, new = self._bufs[self._cur], self._bufs[1 - self._cur]
        with torch.cuda.device(self.device):
            _check(lib().lsfa_mv_accumulate(_ptr(mvs), n, area, _ptr(old), _ptr(new), self.width, self.height, _ptr(self._ws), self._ws.numel(),
                                            _stream()), "lsfa_mv_accumulate")
        self._cur = 1 - self._cur

    def _map(self, who, channels, out):
        """the (H, W, channels) int32 map a method returns: the caller's `out`, checked, or a new one"""
        shape = (self.height, self.width, channels)
        if out is None:
            return torch.empty(shape, dtype=torch.int32, device=self.device)
        return _tensor(who, "output buffer out", out, torch.int32, shape, self.device)

    def motion_vectors(self, out=None):
        mv = self._map("MotionVectorAccumulator.motion_vectors", 2, out)
        with torch.cuda.device(self.device):
            _check(lib().lsfa_mv_field(_ptr(self.accu), self.width, self.height, _ptr(mv), _stream()), "lsfa_mv_field")
        return mv

    def residual(self, bgr_cur, bgr_ref, out=None):
        for t in (bgr_cur, bgr_ref):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or tuple(t.shape) != (self.height, self.width, 3):
                raise LsfaError("MotionVectorAccumulator.residual: frames must be (%d, %d, 3) uint8, got %s" % (self.height, self.width, _arrived(t)))
        bgr_cur, bgr_ref = bgr_cur.to(self.device).contiguous(), bgr_ref.to(self.device).contiguous()
        res = self._map("MotionVectorAccumulator.residual", 3, out)
        with torch.cuda.device(self.device):
            _check(lib().lsfa_mv_residual(_ptr(bgr_cur), _ptr(bgr_ref), _ptr(self.accu), self.width, self.height, _ptr(res), _stream()),
                   "lsfa_mv_residual")
        return res

    def network_inputs(self, bgr_cur, bgr_ref, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16):
        """The frame's `motion_vector` (1, 2, h, w) and `res_diff` (1, 3, h, w) as get_image builds them (lib/utils/image.py:52-63): the
        accumulated motion vectors, negated, and the residual through transform_mv_res - three launches, nothing leaves the device."""
        return transform_mv_res(self.motion_vectors(), self.residual(bgr_cur, bgr_ref), im_scale, pixel_means, pixel_scale, rcnn_stride, negate_mv=True)


# ---- motion estimation on decoded frames (lsfa_amd/csrc/me.hip) ------------------------------------------------------------------------------
# Parameters, not tuned values: a search range that covers the synthetic clips' motion, a small cost per pixel of vector length so that flat
# or noisy blocks stay at rest, no intra threshold.  Nothing was fitted to data (there is no encoder output here to fit to).
ME_SEARCH, ME_LAMBDA, ME_MAX_SAD = 16, 4, 0

# ---- pyramid search (lsfa_amd/csrc/me_pyramid.hip) --------------------------------------------------------------------------------------------
# levels = 0 is the full search alone.  refine = 2 is a parameter like ME_SEARCH, not a tuned value.
ME_LEVELS, ME_REFINE = 0, 2

# ---- scene cuts (lsfa_amd/csrc/me_cut.hip) -----------------------------------------------------------------------------------------------------
# Parameters like the searches', not tuned values: a block is unmatched beyond 4 grey levels per pixel over its intra cost (two frames of one
# flat, noisy area differ by about sqrt(2) times the noise, a block from its own mean by the noise only); a frame most of whose blocks are
# unmatched is a cut.
ME_CUT_BIAS, ME_CUT_PERCENT = 4, 50

# ---- stale key frames (lsfa_amd/csrc/me_key.hip) ------------------------------------------------------------------------------------------------
# The same rule against the KEY frame (the block's SAD against its walked-back source there), with parameters of its own - parameters, not
# tuned values, and independent of the pair rule's.
ME_STALE_BIAS, ME_STALE_PERCENT = 4, 50


def me_reach(levels, search, refine=ME_REFINE):
    """the longest vector component, in pixels, the search can return: search * 2^levels + refine * (2^levels - 1)"""
    return int(search) * 2 ** int(levels) + int(refine) * (2 ** int(levels) - 1)


def pyramid_shapes(height, width, levels):
    """[(h_0, w_0), .., (h_levels, w_levels)]: every level ceil(h / 2) x ceil(w / 2) of the one below"""
    shapes = [(int(height), int(width))]
    for _ in range(int(levels)):
        shapes.append((-(-shapes[-1][0] // 2), -(-shapes[-1][1] // 2)))
    return shapes


def _plane_stack(t, shape, stride0):
    """a flat uint8 buffer as (N, h, w) planes `stride0` bytes apart"""
    return t.as_strided(shape, (stride0, shape[2], 1))


def _search_outputs(who, lead, H, W, device, out, sad_out, return_sad):
    """the rows `lead` + (mbh * mbw, 7) and the SAD `lead` + (mbh, mbw) of a search on (H, W) planes: allocated where the caller gave none
    (the SAD only if asked for), the caller's checked -> (out, sad_out or None)"""
    mbh, mbw = -(-H // 16), -(-W // 16)
    if out is None:
        out = torch.empty(lead + (mbh * mbw, 7), dtype=torch.int32, device=device)
    if return_sad and sad_out is None:
        sad_out = torch.empty(lead + (mbh, mbw), dtype=torch.int32, device=device)
    _tensor(who, "output buffer out", out, torch.int32, lead + (mbh * mbw, 7), device)
    if sad_out is not None:
        _tensor(who, "output buffer sad_out", sad_out, torch.int32, lead + (mbh, mbw), device)
    return out, sad_out


@_on_tensor_device
def luma_u8(bgr, out=None):
    """lsfa_luma_u8: (H, W, 3) uint8 BGR frame on the device -> (H, W) uint8 luma, Y = (29 B + 150 G + 77 R + 128) >> 8."""
    _tensor("luma_u8", "bgr", bgr, torch.uint8, ("H", "W", 3))
    H, W = int(bgr.shape[0]), int(bgr.shape[1])
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=bgr.device)
    _tensor("luma_u8", "out", out, torch.uint8, (H, W), bgr.device)
    _check(lib().lsfa_luma_u8(_ptr(bgr), W, H, _ptr(out), _stream()), "lsfa_luma_u8")
    return out


@_on_tensor_device
def mv_estimate(luma_cur, luma_ref, search=ME_SEARCH, lam=ME_LAMBDA, max_sad=ME_MAX_SAD, return_sad=False, out=None, sad_out=None):
    """lsfa_mv_estimate: two (H, W) uint8 luma planes on the device -> (mbh * mbw, 7) int32 rows {-1, 16, 16, src_x, src_y, dst_x, dst_y}, one per
    16 x 16 macroblock (zero vectors included), as MotionVectorAccumulator.add_frame takes them; with return_sad also the winners' SAD
    (mbh, mbw) int32.  Full search over [-search, search]^2, cost = SAD + lam (|dx| + |dy|), ties by (|dx| + |dy|, dy, dx); max_sad > 0 zeroes
    the vector of a block whose best SAD exceeds it.  Defined by its own specification (include/lsfa_hip.h), not by an encoder's search."""
    _tensor("mv_estimate", "luma_cur", luma_cur, torch.uint8, ("H", "W"))
    H, W = int(luma_cur.shape[0]), int(luma_cur.shape[1])
    _tensor("mv_estimate", "luma_ref (a plane like luma_cur)", luma_ref, torch.uint8, (H, W), luma_cur.device)
    out, sad_out = _search_outputs("mv_estimate", (), H, W, luma_cur.device, out, sad_out, return_sad)
    _check(lib().lsfa_mv_estimate(_ptr(luma_cur), _ptr(luma_ref), W, H, int(search), int(lam), int(max_sad), _ptr(out), _ptr(sad_out), _stream()),
           "lsfa_mv_estimate")
    return (out, sad_out) if return_sad else out


def _u8_stack(who, name, t, trailing):
    """a uint8 CUDA stack (C, F + 1) + trailing (a string stands for an axis of any size) whose frames are dense and whose chains lie (F + 1)
    frames apart -> (C, F, frame stride, the frame's shape)"""
    nd = 2 + len(trailing)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda or t.dim() != nd or int(t.shape[0]) < 1 or int(t.shape[1]) < 2 or \
            any(not isinstance(w, str) and int(v) != w for v, w in zip(t.shape[2:], trailing)):
        raise LsfaError("%s: %s must be a (C, F + 1, %s) uint8 CUDA stack with C >= 1 and F >= 1, got %s %s" %
                        (who, name, ", ".join(str(v) for v in trailing), tuple(getattr(t, 'shape', ())), getattr(t, 'dtype', type(t))))
    C, F1, frame = int(t.shape[0]), int(t.shape[1]), tuple(int(v) for v in t.shape[2:])
    dense = tuple(int(np.prod(frame[i + 1:])) for i in range(len(frame)))
    fs = int(t.stride(1))
    if tuple(int(s) for s in t.stride()[2:]) != dense or fs < int(np.prod(frame)) or (C > 1 and int(t.stride(0)) != F1 * fs):
        raise LsfaError("%s: %s needs dense frames, one stride from frame to frame and chains (F + 1) frames apart; got shape %s strides %s" %
                        (who, name, tuple(t.shape), tuple(t.stride())))
    return C, F1 - 1, fs, frame


@_on_tensor_device
def mv_estimate_chain(luma_stack, search=ME_SEARCH, lam=ME_LAMBDA, max_sad=ME_MAX_SAD, return_sad=False, out=None, sad_out=None):
    """lsfa_mv_estimate_chain: a (C, F + 1, H, W) uint8 stack of luma planes on the device, plane 0 of a chain its key frame -> rows
    (C, F, mbh * mbw, 7) int32, rows[c, f - 1] = mv_estimate(plane f, plane f - 1) of chain c bit for bit; with return_sad also the winners' SAD
    (C, F, mbh, mbw).  The plane stride is taken from .stride() (a multiple of 4 that holds a plane).  One launch."""
    C, F, stride, (H, W) = _u8_stack("mv_estimate_chain", "luma_stack", luma_stack, ("H", "W"))
    out, sad_out = _search_outputs("mv_estimate_chain", (C, F), H, W, luma_stack.device, out, sad_out, return_sad)
    _check(lib().lsfa_mv_estimate_chain(_ptr(luma_stack), stride, C, F, W, H, int(search), int(lam), int(max_sad), _ptr(out), _ptr(sad_out), _stream()),
           "lsfa_mv_estimate_chain")
    return (out, sad_out) if return_sad else out


@_on_tensor_device
def luma_pyramid(luma, levels, out=None):
    """lsfa_luma_pyramid: luma (N, H, W) uint8 on the device, dense planes any stride apart -> [P_1] or [P_1, P_2], (N, h_k, w_k) uint8 with
    P_{k+1}[y][x] = (a + b + c + d + 2) >> 2 over the 2 x 2 taps of P_k, coordinates clamped; P_2 from P_1, never from P_0.  The outputs'
    planes lie a multiple of 4 bytes apart (what the searches want); out: such tensors of the caller's.  One launch."""
    who = "luma_pyramid"
    if not isinstance(luma, torch.Tensor) or luma.dtype != torch.uint8 or not luma.is_cuda or luma.dim() != 3 or int(luma.shape[0]) < 1:
        raise LsfaError("%s: a (N, H, W) uint8 CUDA stack expected, got %s %s" % (who, tuple(getattr(luma, 'shape', ())), getattr(luma, 'dtype', type(luma))))
    levels = int(levels)
    if levels not in (1, 2):
        raise LsfaError("%s: levels %d is outside 1..2" % (who, levels))
    N, H, W = (int(v) for v in luma.shape)
    if (int(luma.stride(1)), int(luma.stride(2))) != (W, 1) or (N > 1 and int(luma.stride(0)) < H * W):
        raise LsfaError("%s: the planes must be dense; got shape %s strides %s" % (who, tuple(luma.shape), tuple(luma.stride())))
    shapes = pyramid_shapes(H, W, levels)[1:]
    if out is None:
        out = []
        for h, w in shapes:
            ps = -(-h * w // 4) * 4
            out.append(_plane_stack(torch.empty(N * ps, dtype=torch.uint8, device=luma.device), (N, h, w), ps))
    out = list(out)
    if len(out) != levels:
        raise LsfaError("%s: out must hold %d tensors, one per level" % (who, levels))
    strides = []
    for t, (h, w) in zip(out, shapes):
        ok = isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) == (N, h, w) and t.device == luma.device and \
            (int(t.stride(1)), int(t.stride(2))) == (w, 1)
        s = (int(t.stride(0)) if N > 1 else -(-h * w // 4) * 4) if ok else 0
        if not ok or s < h * w or s % 4 or t.data_ptr() % 4:
            raise LsfaError("%s: an output must be a (%d, %d, %d) uint8 tensor on %s with dense, 4-byte aligned planes a multiple of 4 bytes apart" %
                            (who, N, h, w, luma.device))
        strides.append(s)
    _check(lib().lsfa_luma_pyramid(_ptr(luma), int(luma.stride(0)) if N > 1 else H * W, N, W, H, levels, _ptr(out[0]), strides[0],
                                   _ptr(out[1]) if levels == 2 else None, strides[1] if levels == 2 else 0, _stream()), "lsfa_luma_pyramid")
    return out


@_on_tensor_device
def mv_refine_chain(luma_stack, parent_rows, refine=ME_REFINE, lam=ME_LAMBDA, max_sad=ME_MAX_SAD, return_sad=False, out=None, sad_out=None):
    """lsfa_mv_refine_chain: one refinement step of the pyramid search.  luma_stack (C, F + 1, H, W) uint8, the planes of level k as
    mv_estimate_chain takes them; parent_rows (C, F, mbh1 * mbw1, 7) int32, the rows of level k + 1 (the grid of the ceil(H / 2) x ceil(W / 2)
    plane) -> rows (C, F, mbh * mbw, 7) of level k; with return_sad also the winners' SAD (C, F, mbh, mbw).  Block (bx, by) tries
    2 * (its parent (bx >> 1, by >> 1)'s vector) + [-refine, refine]^2 and (0, 0), under the full search's cost, order and validity rule.
    One launch."""
    who = "mv_refine_chain"
    C, F, stride, (H, W) = _u8_stack(who, "luma_stack", luma_stack, ("H", "W"))
    h1, w1 = pyramid_shapes(H, W, 1)[1]
    _tensor(who, "parent_rows (the rows of the %d x %d level above)" % (w1, h1), parent_rows, torch.int32, (C, F, -(-h1 // 16) * -(-w1 // 16), 7),
            luma_stack.device)
    out, sad_out = _search_outputs(who, (C, F), H, W, luma_stack.device, out, sad_out, return_sad)
    _check(lib().lsfa_mv_refine_chain(_ptr(luma_stack), stride, C, F, W, H, _ptr(parent_rows), int(refine), int(lam), int(max_sad), _ptr(out),
                                      _ptr(sad_out), _stream()), "lsfa_mv_refine_chain")
    return (out, sad_out) if return_sad else out


@_on_tensor_device
def mv_cut_score(luma_stack, sad, bias=ME_CUT_BIAS, out=None):
    """lsfa_mv_cut_score: luma_stack (C, F + 1, H, W) uint8 as mv_estimate_chain takes it and the winners' SAD (C, F, mbh, mbw) int32 a search
    wrote for it (the full search's, or the pyramid's level 0) -> (intra (C, F, mbh, mbw), unmatched (C, F)) int32: per macroblock of plane
    f = 1..F the sum of |p - mean| over its covered pixels, per pair the number of blocks with sad > intra + bias * covered pixels (bias
    0..255).  Pair (c, f) is a cut iff unmatched * 100 > percent * mbh * mbw (hip.cut_flags).  Two launches, nothing read back.  out: a pair
    of contiguous int32 tensors of those shapes.  Defined by its own specification (include/lsfa_hip.h; tests/ref_me_cut.py): the textbook
    inter-against-intra rule, not an encoder's scene detection."""
    who = "mv_cut_score"
    C, F, stride, (H, W) = _u8_stack(who, "luma_stack", luma_stack, ("H", "W"))
    mbh, mbw = -(-H // 16), -(-W // 16)
    _tensor(who, "sad (the winners' SAD of a search on this stack)", sad, torch.int32, (C, F, mbh, mbw), luma_stack.device)
    if not 0 <= int(bias) <= 255:
        raise LsfaError("%s: bias %r is outside 0..255" % (who, bias))
    if out is None:
        out = (torch.empty((C, F, mbh, mbw), dtype=torch.int32, device=luma_stack.device),
               torch.empty((C, F), dtype=torch.int32, device=luma_stack.device))
    intra = _tensor(who, "output buffer out[0]", out[0], torch.int32, (C, F, mbh, mbw), luma_stack.device)
    unmatched = _tensor(who, "output buffer out[1]", out[1], torch.int32, (C, F), luma_stack.device)
    _check(lib().lsfa_mv_cut_score(_ptr(luma_stack), stride, C, F, W, H, _ptr(sad), int(bias), _ptr(intra), _ptr(unmatched), _stream()),
           "lsfa_mv_cut_score")
    return intra, unmatched


def cut_flags(unmatched, blocks, percent=ME_CUT_PERCENT):
    """the frame decision on HOST counts (a list, an array or a CPU tensor): unmatched * 100 > percent * blocks, elementwise, in integers"""
    return np.asarray(unmatched, dtype=np.int64) * 100 > int(percent) * int(blocks)


def _cut_params(who, cut, name='cut', defaults=(ME_CUT_BIAS, ME_CUT_PERCENT)):
    """cut=None | dict(bias=..., percent=...) -> None | (bias, percent), checked (`name`: the keyword, cut or stale)"""
    if cut is None:
        return None
    if not isinstance(cut, dict):
        raise LsfaError("%s: %s takes a dict of bias (0..255) and percent (1..100), got %r" % (who, name, cut))
    extra = set(cut) - {'bias', 'percent'}
    bias, percent = int(cut.get('bias', defaults[0])), int(cut.get('percent', defaults[1]))
    if extra or not 0 <= bias <= 255 or not 1 <= percent <= 100:
        raise LsfaError("%s: %s takes bias (0..255) and percent (1..100), got %r" % (who, name, dict(cut)))
    return bias, percent


@_on_tensor_device
def mv_segment_inputs(rows, bgr_stack, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16, out=None):
    """lsfa_mv_segment_inputs: rows (C, F, mbh * mbw, 7) int32 as mv_estimate_chain returns them and the (C, F + 1, H, W, 3) uint8 BGR stack
    they were estimated on (frame 0 of a chain its key frame) -> `motion_vector` (F, C, 2, h, w) and `res_diff` (F, C, 3, h, w) float32,
    frame-major: [f - 1, c] is what MotionEstimator.network_inputs returns for frame f of chain c, bit for bit.  One launch, no
    full-resolution map.  The frame stride is taken from .stride().  out: a pair of contiguous float32 tensors of those shapes."""
    who = "mv_segment_inputs"
    C, F, stride, (H, W, _) = _u8_stack(who, "bgr_stack", bgr_stack, ("H", "W", 3))
    _tensor(who, "rows", rows, torch.int32, (C, F, -(-H // 16) * -(-W // 16), 7), bgr_stack.device)
    if not float(im_scale) > 0.0 or int(rcnn_stride) < 1:
        raise LsfaError("%s: im_scale %r must be positive and rcnn_stride %r at least 1" % (who, im_scale, rcnn_stride))
    rcnn_stride = int(rcnn_stride)
    h1, w1, oh, ow = _resized_map(H, W, im_scale, rcnn_stride)
    if out is None:
        out = (torch.empty((F, C, 2, oh, ow), device=bgr_stack.device, dtype=torch.float32),
               torch.empty((F, C, 3, oh, ow), device=bgr_stack.device, dtype=torch.float32))
    out_mv = _tensor(who, "output buffer out[0]", out[0], torch.float32, (F, C, 2, oh, ow), bgr_stack.device)
    out_res = _tensor(who, "output buffer out[1]", out[1], torch.float32, (F, C, 3, oh, ow), bgr_stack.device)
    _check(lib().lsfa_mv_segment_inputs(_ptr(rows), _ptr(bgr_stack), stride, C, F, W, H, float(im_scale), h1, w1, rcnn_stride, _means(pixel_means),
                                        float(pixel_scale), _ptr(out_mv), _ptr(out_res), oh, ow, _stream()), "lsfa_mv_segment_inputs")
    return out_mv, out_res


class _MotionSearch(object):
    """What MotionEstimator and SegmentMotionEstimator share: the checked parameters, the geometry of every level, the planes and rows of
    every level for `planes` luma planes and `pairs` pairs - flat, so that any run of planes is a stack of its own in front of the same
    memory - and the coarse-to-fine sequence on a stack of them."""

    def __init__(self, who, width, height, device, search, lam, max_sad, luma_from, matrix, levels, refine, planes, pairs, cut=None, stale=None,
                 keep_key=False):
        self.cut = _cut_params(who, cut)
        self.stale = _cut_params(who, stale, 'stale', (ME_STALE_BIAS, ME_STALE_PERCENT))
        self.levels, self.refine = int(levels), int(refine)
        if not 0 <= self.levels <= 2:
            raise LsfaError("%s: levels %d is outside 0..2" % (who, self.levels))
        if self.levels and not 1 <= self.refine <= 3:
            raise LsfaError("%s: refine %d is outside 1..3" % (who, self.refine))
        if luma_from not in ('bgr', 'y'):
            raise LsfaError("%s: luma_from %r is not 'bgr' or 'y'" % (who, luma_from))
        if matrix not in YUV_MATRICES:
            raise LsfaError("%s: matrix %r is not one of %s" % (who, matrix, sorted(YUV_MATRICES)))
        self.luma_from, self.matrix = luma_from, matrix
        self.width, self.height, self.device = int(width), int(height), torch.device(device)
        self.search, self.lam, self.max_sad = int(search), int(lam), int(max_sad)
        if not 1 <= self.search <= 32 or self.lam < 0 or self.max_sad < 0:
            raise LsfaError("%s: search %d (1..32), lam %d (>= 0), max_sad %d (>= 0)" % (who, self.search, self.lam, self.max_sad))
        self.reach = me_reach(self.levels, self.search, self.refine)
        self.mbh, self.mbw = -(-self.height // 16), -(-self.width // 16)
        # per level: the plane's shape, its size padded to the 4 bytes the searches want from plane to plane, its macroblocks
        self.shapes = pyramid_shapes(self.height, self.width, self.levels)
        self.plane = [-(-h * w // 4) * 4 for h, w in self.shapes]
        self.blocks = [-(-h // 16) * -(-w // 16) for h, w in self.shapes]
        self.flat = [torch.empty(planes * ps, dtype=torch.uint8, device=self.device) for ps in self.plane]
        self.rows = [torch.empty(pairs * b * 7, dtype=torch.int32, device=self.device) for b in self.blocks]
        self.sad = torch.empty(pairs * self.blocks[0], dtype=torch.int32, device=self.device)
        # scene cuts (cut=dict(bias, percent)): every block's intra cost and every pair's count of unmatched blocks
        self.intra = torch.empty(pairs * self.blocks[0], dtype=torch.int32, device=self.device) if self.cut else None
        # stale key frames (stale=dict(bias, percent)): every block's SAD against the key frame, its intra cost once more (lsfa_mv_cut_score
        # writes it with every call; DESIGN.md "Stale key frames") and every frame's count of blocks the key frame does not predict
        self.keysad = torch.empty(pairs * self.blocks[0], dtype=torch.int32, device=self.device) if self.stale else None
        self.key_intra = torch.empty(pairs * self.blocks[0], dtype=torch.int32, device=self.device) if self.stale else None
        # the counts of both rules lie in one buffer, the pair rule's first: read_cuts reads them back together
        modes = (1 if self.cut else 0) + (1 if self.stale else 0)
        self._counts = torch.empty(modes * pairs, dtype=torch.int32, device=self.device) if modes else None
        self.unmatched = self._counts[:pairs] if self.cut else None
        self.key_unmatched = self._counts[modes * pairs - pairs:] if self.stale else None
        # frame by frame (keep_key) the key frame's luma outlives the two ping-pong planes: a third level-0 plane
        self.key_plane = torch.empty(self.plane[0], dtype=torch.uint8, device=self.device) if self.stale and keep_key else None

    def planes(self, k, first, count):
        """planes first .. first + count - 1 of level k as (count, h_k, w_k)"""
        return _plane_stack(self.flat[k][first * self.plane[k]:], (count,) + self.shapes[k], self.plane[k])

    def pyramid(self, first, count):
        """the upper levels of planes first .. first + count - 1 (one launch; nothing with levels = 0)"""
        if self.levels:
            luma_pyramid(self.planes(0, first, count), self.levels, out=[self.planes(k, first, count) for k in range(1, self.levels + 1)])

    def run(self, chains, frames, first=0, step=1, built=0):
        """Rows and SAD of every pair of `chains` stacks of frames + 1 planes, into the front of self.rows[0] / self.sad (self.rows[k]: level
        k's).  The stack is addressed on every level as the exports address one - plane 0 at plane `first` of the flat buffer, the others
        `step` planes on, -1 for a stack stored in reverse - and the pyramid of its first `built` planes exists already.  levels + 2
        launches: the pyramid of the other planes, the full search on the top level, one refinement per level below it; with levels = 0
        the full search alone.  max_sad and the SAD belong to level 0.  With `cut` set, lsfa_mv_cut_score's two launches follow level 0:
        the front of self.intra / self.unmatched."""
        L, N = self.levels, chains * (frames + 1)
        self.pyramid(first + step * (built if step > 0 else N - 1), N - built)
        with torch.cuda.device(self.device):
            for k in range(L, -1, -1):
                luma, stride, (h, w) = _ptr(self.flat[k][first * self.plane[k]:]), step * self.plane[k], self.shapes[k]
                max_sad, sad = (0, None) if k else (self.max_sad, _ptr(self.sad))
                if k == L:
                    _check(lib().lsfa_mv_estimate_chain(luma, stride, chains, frames, w, h, self.search, self.lam, max_sad, _ptr(self.rows[k]), sad,
                                                        _stream()), "lsfa_mv_estimate_chain")
                else:
                    _check(lib().lsfa_mv_refine_chain(luma, stride, chains, frames, w, h, _ptr(self.rows[k + 1]), self.refine, self.lam, max_sad,
                                                      _ptr(self.rows[k]), sad, _stream()), "lsfa_mv_refine_chain")
        self.cut_score(chains, frames, first, step)

    def cut_score(self, chains, frames, first=0, step=1):
        """lsfa_mv_cut_score on the stack run() was given, behind its level-0 SAD (nothing without `cut`)"""
        if self.cut:
            with torch.cuda.device(self.device):
                _check(lib().lsfa_mv_cut_score(_ptr(self.flat[0][first * self.plane[0]:]), step * self.plane[0], chains, frames, self.width,
                                               self.height, _ptr(self.sad), self.cut[0], _ptr(self.intra), _ptr(self.unmatched), _stream()),
                       "lsfa_mv_cut_score")

    def keep_key_plane(self, index):
        """level-0 plane `index` holds a key frame: with `stale` and keep_key it is copied to the third plane (one launch), else nothing"""
        if self.key_plane is not None:
            ps = self.plane[0]
            copy_many([(self.key_plane.view(torch.int32), self.flat[0][index * ps:(index + 1) * ps].view(torch.int32))])

    def key_score(self, chains, frames, first=0, step=1, accu=None):
        """The key rule behind run() on the same stack (nothing without `stale`): every block's SAD against its chain's key frame -
        lsfa_mv_key_sad, the walk back through self.rows[0]; or, with accu (H, W, 2) the accumulated source map of ONE pair whose key
        frame lies in self.key_plane, lsfa_mv_key_sad_accu - into the front of self.keysad, then lsfa_mv_cut_score with it in the place
        of the search's SAD: self.key_intra, self.key_unmatched."""
        if not self.stale:
            return
        luma, stride = _ptr(self.flat[0][first * self.plane[0]:]), step * self.plane[0]
        with torch.cuda.device(self.device):
            if accu is None:
                _check(lib().lsfa_mv_key_sad(luma, stride, chains, frames, self.width, self.height, _ptr(self.rows[0]), _ptr(self.keysad), _stream()),
                       "lsfa_mv_key_sad")
            else:
                _tensor("_MotionSearch.key_score", "accu", accu, torch.int32, (self.height, self.width, 2), self.device)
                _check(lib().lsfa_mv_key_sad_accu(_ptr(self.flat[0][(first + step) * self.plane[0]:]), _ptr(self.key_plane), _ptr(accu), self.width,
                                                  self.height, _ptr(self.keysad), _stream()), "lsfa_mv_key_sad_accu")
            _check(lib().lsfa_mv_cut_score(luma, stride, chains, frames, self.width, self.height, _ptr(self.keysad), self.stale[0], _ptr(self.key_intra),
                                           _ptr(self.key_unmatched), _stream()), "lsfa_mv_cut_score")

    def read_cuts(self, count):
        """the one readback: synchronises the current stream and returns the first `count` pairs' flags - the pair rule's (`cut`) OR the key
        rule's (`stale`), whichever are on - as a numpy bool array; 4 * count bytes per rule"""
        with torch.cuda.device(self.device):
            torch.cuda.current_stream().synchronize()
        rules = [r for r in (self.cut, self.stale) if r]
        counts = self._counts.view(len(rules), -1)[:, :count].cpu().numpy()
        return np.logical_or.reduce([cut_flags(c, self.blocks[0], r[1]) for c, r in zip(counts, rules)])


class _SearchFront(object):
    """What MotionEstimator and SegmentMotionEstimator show of the _MotionSearch they stand in front of: its checked parameters and its
    geometry, under its names.  The buffers of the modes (unmatched, keysad, ...) are the subclass's: views of the search's in its own shape.
    _to_bgr is the one conversion behind the *_yuv methods of both: (y, uv, u, v, matrix, out=, y_packed=) -> out.  A subclass for planes
    of another sample format overrides it (lsfa_amd/yuv10.py).  _y_plane is the (rows, columns) of the `y` argument of the *_yuv methods: the
    frame's, unless a subclass takes a plane of another width (a packed 4:2:2 row of lsfa_amd/yuvfmt.py)."""

    _to_bgr = staticmethod(yuv420_to_bgr_u8)

    def _y_plane(self):
        return self.height, self.width

    def __init__(self, s):
        self._search = s
        self.cut, self.stale = s.cut, s.stale
        self.width, self.height, self.device = s.width, s.height, s.device
        self.search, self.lam, self.max_sad, self.levels, self.refine = s.search, s.lam, s.max_sad, s.levels, s.refine
        self.luma_from, self.matrix, self.reach, self.mbh, self.mbw = s.luma_from, s.matrix, s.reach, s.mbh, s.mbw


class MotionEstimator(_SearchFront):
    """Decoded uint8 frames in, the network's `motion_vector` / `res_diff` out: block motion estimation (lsfa_luma_u8 + lsfa_mv_estimate) in
    front of a MotionVectorAccumulator, for clips without compressed-stream side data.

        me = MotionEstimator(width, height, device)
        me.key_frame(bgr0)                   # the GOP's I-frame: identity accumulation, bgr0 becomes the reference
        me.next_frame(bgr1)                  # a P-frame: vectors against the PREVIOUS frame (an IPPP chain), accumulated
        mv, res = me.network_inputs(bgr1, bgr0, im_scale, pixel_means, pixel_scale)

    Every buffer is allocated up front (the outputs of network_inputs at its first call for a scale), nothing is read back and nothing
    synchronises, so the three calls can be captured in a graph on one stream and replayed on new frame contents written into the same
    tensors.  The tensors network_inputs returns are reused by the next call.

    Frames that arrive as a decoder's YUV 4:2:0 planes (see yuv420_to_bgr_u8) go through key_frame_yuv / next_frame_yuv, which convert into
    BGR buffers the estimator owns (self.bgr_key; self.bgr_cur, a ping-pong pair - allocated at the first such call, nothing after it) and
    return that buffer: `me.network_inputs(me.bgr_cur, me.bgr_key, ...)` works unchanged.  luma_from='bgr' (the default) searches
    lsfa_luma_u8 of the converted frame: the rows are those of feeding the converted frames to key_frame / next_frame.  luma_from='y'
    searches the decoder's own Y plane (the conversion's y_packed output, no luma launch): DIFFERENT numbers - Y is limited-range (16..235)
    and weighs the channels by the stream's matrix, lsfa_luma_u8 is full-range with its own weights - so SADs, the lambda trade-off and
    therefore some vectors differ.  `matrix` is the conversion's.

    levels = 1 or 2 switches to the pyramid search (lsfa_amd/csrc/me_pyramid.hip; DESIGN.md "Pyramid search"): `search` is then the range on the
    top level and self.reach = search * 2^levels + refine * (2^levels - 1) pixels.  The pyramids of both ping-pong planes are kept and only
    the new frame's is built: next_frame is levels + 2 launches in front of the accumulation (pyramid, top search, one refinement per
    level) instead of one.  levels = 0 (the default) runs exactly the full search's launches; `refine` is ignored there.

    The pyramid search is SegmentMotionEstimator's on one chain of one pair: the two ping-pong planes of every level lie one plane apart in
    one buffer, a stack of two that starts at the reference plane - forwards if the current plane lies behind it, else stored in reverse.

    cut=dict(bias=..., percent=...) (either may be left out; default None: every launch and every bit as without it) adds scene-cut
    detection (lsfa_mv_cut_score, two launches behind the search; DESIGN.md "Scene cuts"): after next_frame / next_frame_yuv, self.unmatched
    is the (1,) int32 device count of blocks the previous frame does not predict, and is_cut() - the one readback, a synchronisation -
    says whether the frame starts a new scene: the caller then hands the same frame to key_frame / key_frame_yuv.

    stale=dict(bias=..., percent=...) (either may be left out; default None: every launch and every bit as without it) adds the key rule
    (DESIGN.md "Stale key frames"): the same decision on every block's SAD against the KEY frame, compensated with the accumulated vectors -
    what a fade, a dissolve or a slow pan spoils although no pair of consecutive frames shows it.  key_frame / key_frame_yuv keep the key
    frame's luma in a third plane (one copy launch); next_frame / next_frame_yuv run three more launches behind the accumulation (the key
    SAD from self.acc.accu, the intra cost and the count).  self.keysad is the (mbh, mbw) SAD against the key frame, self.key_unmatched
    the (1,) int32 device count, and is_cut() is true where either rule flags the frame (one readback for both).  Every buffer is
    allocated at construction."""

    def __init__(self, width, height, device='cuda:0', search=ME_SEARCH, lam=ME_LAMBDA, max_sad=ME_MAX_SAD, luma_from='bgr', matrix='bt601',
                 levels=ME_LEVELS, refine=ME_REFINE, cut=None, stale=None):
        s = _MotionSearch("MotionEstimator", width, height, device, search, lam, max_sad, luma_from, matrix, levels, refine, planes=2, pairs=1,
                          cut=cut, stale=stale, keep_key=True)
        _SearchFront.__init__(self, s)
        self.unmatched, self.key_unmatched = s.unmatched, s.key_unmatched
        self.keysad = s.keysad.view(s.mbh, s.mbw) if s.stale else None
        self.bgr_key, self._bgr_pp, self._bgr_i = None, None, 0
        H, W = self.height, self.width
        self.acc = MotionVectorAccumulator(W, H, self.device)
        self._luma = s.planes(0, 0, 2)
        self._ref = 0                   # index of the previous frame's plane
        self.rows, self.sad = s.rows[0].view(self.mbh * self.mbw, 7), s.sad.view(self.mbh, self.mbw)
        self._mv = torch.empty((H, W, 2), dtype=torch.int32, device=self.device)
        self._res = torch.empty((H, W, 3), dtype=torch.int32, device=self.device)
        self._out = {}

    def _frame(self, bgr, who):
        return _tensor("MotionEstimator." + who, "the frame", bgr, torch.uint8, (self.height, self.width, 3), self.device)

    def _key(self):
        """the reference plane holds a key frame: its pyramid, and the accumulation starts over"""
        self._search.pyramid(self._ref, 1)
        self._search.keep_key_plane(self._ref)
        self.acc.reset()

    def _next(self, cur):
        """plane `cur` holds the next frame: its rows against the reference plane's, accumulated; it becomes the reference"""
        if self.levels == 0:
            # the pair kernel, not run(1, 1, ...): through the chain kernel the per-frame graph of nine frames was 3.3 us (1000 x 600) to
            # 12.4 us (1920 x 1080) slower, beyond the parent's run-to-run spread of 0.4 .. 2.4 us (profiles/r9/me_frontend_refactor.txt)
            mv_estimate(self._luma[cur], self._luma[self._ref], self.search, self.lam, self.max_sad, out=self.rows, sad_out=self.sad)
            self._search.cut_score(1, 1, self._ref, cur - self._ref)
        else:
            self._search.run(1, 1, self._ref, cur - self._ref, built=1)
        self.acc.add_frame(self.rows, max_block_area=256)      # the explicit area: no device-to-host read
        self._search.key_score(1, 1, self._ref, cur - self._ref, accu=self.acc.accu)
        self._ref = cur

    def key_frame(self, bgr):
        luma_u8(self._frame(bgr, 'key_frame'), out=self._luma[self._ref])
        self._key()

    def next_frame(self, bgr):
        """Estimates the frame's vectors against the previous frame and accumulates them; returns the (mbh * mbw, 7) rows (a buffer the
        next call overwrites; self.sad holds the winners' SAD)."""
        cur = 1 - self._ref
        luma_u8(self._frame(bgr, 'next_frame'), out=self._luma[cur])
        self._next(cur)
        return self.rows

    def is_cut(self):
        """Does the frame the last next_frame / next_frame_yuv took start a new scene (`cut`), or has its key frame stopped predicting it
        (`stale`)?  Synchronises the current stream and reads self.unmatched / self.key_unmatched (4 bytes each): the one readback of the
        modes."""
        if not self.cut and not self.stale:
            raise LsfaError("MotionEstimator.is_cut: the estimator was built without cut= or stale=")
        return bool(self._search.read_cuts(1)[0])

    @property
    def bgr_cur(self):
        """the BGR frame the last next_frame_yuv converted (None before the first)"""
        return None if self._bgr_pp is None else self._bgr_pp[self._bgr_i]

    def _yuv_buffers(self):
        if self.bgr_key is None:          # the first *_yuv call: the only allocation
            self.bgr_key = torch.empty((self.height, self.width, 3), dtype=torch.uint8, device=self.device)
            self._bgr_pp = [torch.empty_like(self.bgr_key) for _ in range(2)]

    def _yuv_to(self, bgr, luma, y, uv, u, v, who):
        if not isinstance(y, torch.Tensor) or tuple(y.shape) != self._y_plane() or y.device != self.device:
            raise LsfaError("MotionEstimator.%s: a (%d, %d) uint8 Y plane on %s expected, got %s on %s" %
                            (who, self._y_plane()[0], self._y_plane()[1], self.device, tuple(getattr(y, 'shape', ())), getattr(y, 'device', type(y))))
        if self.luma_from == 'y':
            self._to_bgr(y, uv, u, v, self.matrix, out=bgr, y_packed=luma)
        else:
            self._to_bgr(y, uv, u, v, self.matrix, out=bgr)
            luma_u8(bgr, out=luma)
        return bgr

    def key_frame_yuv(self, y, uv=None, u=None, v=None):
        """key_frame on a decoder's planes: converts into self.bgr_key and returns it"""
        self._yuv_buffers()
        bgr = self._yuv_to(self.bgr_key, self._luma[self._ref], y, uv, u, v, 'key_frame_yuv')
        self._key()
        return bgr

    def next_frame_yuv(self, y, uv=None, u=None, v=None):
        """next_frame on a decoder's planes: converts into the other buffer of the ping-pong pair, which becomes self.bgr_cur, and returns it
        (the rows are in self.rows, the winners' SAD in self.sad)"""
        self._yuv_buffers()
        cur, nxt = 1 - self._ref, 1 - self._bgr_i
        bgr = self._yuv_to(self._bgr_pp[nxt], self._luma[cur], y, uv, u, v, 'next_frame_yuv')
        self._next(cur)
        self._bgr_i = nxt
        return bgr

    def network_inputs(self, bgr_cur, bgr_key, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16):
        """`motion_vector` (1, 2, h, w) and `res_diff` (1, 3, h, w) of the current frame against the key frame: MotionVectorAccumulator's
        network_inputs (lsfa_mv_field, lsfa_mv_residual, lsfa_transform_mv_res) into buffers of its own."""
        bgr_cur, bgr_key = self._frame(bgr_cur, 'network_inputs'), self._frame(bgr_key, 'network_inputs')
        oh, ow = _resized_map(self.height, self.width, im_scale, rcnn_stride)[2:]
        if (oh, ow) not in self._out:
            self._out[(oh, ow)] = (torch.empty((1, 2, oh, ow), device=self.device, dtype=torch.float32),
                                   torch.empty((1, 3, oh, ow), device=self.device, dtype=torch.float32))
        return transform_mv_res(self.acc.motion_vectors(out=self._mv), self.acc.residual(bgr_cur, bgr_key, out=self._res), im_scale, pixel_means,
                                pixel_scale, rcnn_stride, negate_mv=True, out=self._out[(oh, ow)])


class SegmentMotionEstimator(_SearchFront):
    """A key frame and the non-key frames behind it in, the `motion_vector` / `res_diff` of every one of them out - what MotionEstimator builds
    frame by frame in seven launches each, for a whole segment of `clips` lock-step clips in three: luma of the stack (lsfa_luma_u8; one
    launch where W * H % 4 == 0, else one per frame), the search of every (frame, previous frame) pair (lsfa_mv_estimate_chain), the inputs
    (lsfa_mv_segment_inputs).

        sme = SegmentMotionEstimator(width, height, frames=9, clips=1, device=device)
        mv, res = sme.segment(bgr_stack, im_scale, pixel_means, pixel_scale)      # bgr_stack (C, n + 1, H, W, 3) uint8, frame 0 the key frame
        mv[f - 1], res[f - 1]                                                      # (C, 2, h, w), (C, 3, h, w): frame f of every clip

    Every buffer is allocated up front for `frames` frames (the outputs at the first call for a scale and a length), nothing is read back
    and nothing synchronises; all launches sit on the current stream, so a call can be captured in a graph without parallel branches and
    replayed on new frame contents.  n < frames (the stack's own length, or `n` frames of a longer stack) is the short segment in front of
    a clip's last frame.  The returned tensors are reused by the next call of the same shape unless `out` supplies others; self.rows
    (C, n, mbh * mbw, 7) and self.sad (C, n, mbh, mbw) hold the last call's vectors.  segment_yuv takes a decoder's planes through the
    N-frame conversion (yuv420_to_bgr_u8); luma_from and matrix are MotionEstimator's.

    levels = 1 or 2 switches to the pyramid search (DESIGN.md "Pyramid search"): `search` is the range on the top level, self.reach the longest
    vector component.  A segment is then levels + 4 launches - luma, lsfa_luma_pyramid of every plane, lsfa_mv_estimate_chain on the top
    level, one lsfa_mv_refine_chain per level below it, the inputs - with the pyramid planes and the rows of every level allocated up
    front like everything else.  levels = 0 (the default) runs exactly the three launches above; `refine` is ignored there.

    cut=dict(bias=..., percent=...) (either may be left out; default None: every launch, every tensor and every bit as without it) adds
    scene-cut detection (DESIGN.md "Scene cuts"): lsfa_mv_cut_score's two launches between the level-0 search and the inputs, on the same
    stream, into buffers allocated up front.  segment / segment_yuv return what they return without it; self.unmatched is the (C, n)
    device view of the last call's counts of unmatched blocks, self.intra (C, n, mbh, mbw) the blocks' intra costs, and first_cuts() - the
    one readback, a synchronisation - gives per clip the first frame that starts a new scene.  The inputs of the frames from a cut on
    were estimated across it: the caller discards them and makes the cut frame a key frame.

    stale=dict(bias=..., percent=...) (either may be left out; default None, as above) adds the key rule (DESIGN.md "Stale key frames"): the
    same decision on every block's SAD against the segment's KEY frame, compensated with the walk back through the rows - `res_diff` before
    its resize - which a fade, a dissolve or a slow pan spoils although no pair of consecutive frames shows it.  Three more launches
    between the search and the inputs (the key SAD, the intra cost and the count), into buffers allocated up front: self.keysad (C, n, mbh,
    mbw), self.key_unmatched (C, n).  first_cuts() then gives per clip the first frame EITHER rule flags, still with one readback."""

    def __init__(self, width, height, frames=9, clips=1, device='cuda:0', search=ME_SEARCH, lam=ME_LAMBDA, max_sad=ME_MAX_SAD, luma_from='bgr',
                 matrix='bt601', levels=ME_LEVELS, refine=ME_REFINE, cut=None, stale=None):
        who = "SegmentMotionEstimator"
        self.frames, self.clips = int(frames), int(clips)
        if self.frames < 1 or self.clips < 1 or int(width) < 1 or int(height) < 1:
            raise LsfaError("%s: frames %d, clips %d and the %d x %d frame must all be at least 1" % (who, self.frames, self.clips, int(width), int(height)))
        s = _MotionSearch(who, width, height, device, search, lam, max_sad, luma_from, matrix, levels, refine,
                          planes=self.clips * (self.frames + 1), pairs=self.clips * self.frames, cut=cut, stale=stale)
        _SearchFront.__init__(self, s)
        self.intra, self.unmatched, self.keysad, self.key_unmatched = None, None, None, None      # views of the last segment's, set by _run
        # the search wants every plane 4-byte aligned: a frame of W * H % 4 != 0 (no 4:2:0 video has one) gets its planes padded apart and
        # its luma frame by frame
        if s.plane[0] != self.height * self.width and luma_from == 'y':
            raise LsfaError("%s: luma_from='y' needs W * H %% 4 == 0, got %d x %d" % (who, self.width, self.height))
        self._luma = s.flat[0]
        self._bgr = None                # segment_yuv's converted frames, allocated at its first call
        self.rows, self.sad = None, None
        self._out = {}

    def _length(self, have, n, who):
        n = have if n is None else int(n)
        if not 1 <= n <= min(have, self.frames):
            raise LsfaError("SegmentMotionEstimator.%s: n = %d non-key frames asked for; the stack holds %d and the estimator was built for %d" %
                            (who, n, have, self.frames))
        return n

    def _outputs(self, who, n, im_scale, rcnn_stride, out):
        """the caller's `out` pair, checked BEFORE the first launch of a segment (mv_segment_inputs, the last one, checks it again)"""
        if out is None:
            return
        if not float(im_scale) > 0.0 or rcnn_stride < 1:
            raise LsfaError("%s: im_scale %r must be positive and rcnn_stride %r at least 1" % (who, im_scale, rcnn_stride))
        oh, ow = _resized_map(self.height, self.width, im_scale, rcnn_stride)[2:]
        out = _given(who, "out", out, 2)
        for i, c in enumerate((2, 3)):
            _tensor(who, "output buffer out[%d]" % i, out[i], torch.float32, (n, self.clips, c, oh, ow), self.device)

    def _run(self, bgr, n, im_scale, pixel_means, pixel_scale, rcnn_stride, out, luma_done):
        H, W, C, s = self.height, self.width, self.clips, self._search
        N, blocks = C * (n + 1), self.mbh * self.mbw
        self.rows = s.rows[0][:C * n * blocks * 7].view(C, n, blocks, 7)
        self.sad = s.sad[:C * n * blocks].view(C, n, self.mbh, self.mbw)
        if self.cut:
            self.intra, self.unmatched = s.intra[:C * n * blocks].view(C, n, self.mbh, self.mbw), s.unmatched[:C * n].view(C, n)
        if self.stale:
            self.keysad, self.key_unmatched = s.keysad[:C * n * blocks].view(C, n, self.mbh, self.mbw), s.key_unmatched[:C * n].view(C, n)
        luma = s.planes(0, 0, N)
        if not luma_done and s.plane[0] == H * W:
            luma_u8(bgr.view(N * H, W, 3), out=luma.view(N * H, W))     # pointwise: a stack is one tall frame
        elif not luma_done:
            for i, frame in enumerate(bgr.view(N, H, W, 3)):
                luma_u8(frame, out=luma[i])
        s.run(C, n)
        s.key_score(C, n)
        if out is None:
            key = (n,) + _resized_map(H, W, im_scale, rcnn_stride)[2:]
            if key not in self._out:
                self._out[key] = (torch.empty((n, C, 2) + key[1:], device=self.device, dtype=torch.float32),
                                  torch.empty((n, C, 3) + key[1:], device=self.device, dtype=torch.float32))
            out = self._out[key]
        return mv_segment_inputs(self.rows, bgr, im_scale, pixel_means, pixel_scale, rcnn_stride, out=out)

    def first_cuts(self, n=None):
        """Per clip the first frame f = 1..n (default: the last call's length) of the last segment whose pair (f, f - 1) is a cut (`cut`) or
        which its key frame has stopped predicting (`stale`), or None.  Synchronises the current stream and reads self.unmatched /
        self.key_unmatched (4 * C * n bytes each) once: the one readback of the modes."""
        if not (self.cut or self.stale) or self.rows is None:
            raise LsfaError("SegmentMotionEstimator.first_cuts: needs cut= or stale= and a segment() / segment_yuv() call before it")
        C, have = int(self.rows.shape[0]), int(self.rows.shape[1])
        n = have if n is None else int(n)
        if not 1 <= n <= have:
            raise LsfaError("SegmentMotionEstimator.first_cuts: n = %d; the last segment holds %d frames" % (n, have))
        flags = self._search.read_cuts(C * have).reshape(C, have)[:, :n]
        return [int(np.argmax(row)) + 1 if row.any() else None for row in flags]

    def segment(self, bgr_stack, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, n=None, rcnn_stride=16, out=None):
        """bgr_stack (C, n + 1, H, W, 3) uint8, contiguous, frame 0 of every clip its key frame -> (mv (n, C, 2, h, w), res (n, C, 3, h, w)).
        `n` below the stack's length takes its first n + 1 frames."""
        C = self.clips
        who = "SegmentMotionEstimator.segment"
        t = _tensor(who, "bgr_stack (a uint8 stack, frame 0 of every clip its key frame)", bgr_stack, torch.uint8, (C, "n + 1", self.height, self.width, 3),
                    self.device)
        if int(t.shape[1]) < 2:
            raise LsfaError("%s: the uint8 stack holds %d frame(s) per clip; a key frame and at least one frame behind it expected" % (who, int(t.shape[1])))
        have = int(t.shape[1]) - 1
        n = self._length(have, n, 'segment')
        if n < have:
            if C > 1:
                raise LsfaError("SegmentMotionEstimator.segment: n = %d of a stack of %d frames needs clips = 1 (with more, hand over a stack of "
                                "n + 1 frames per clip)" % (n, have))
            t = t[:, :n + 1]
        self._outputs(who, n, im_scale, int(rcnn_stride), out)
        return self._run(t, n, im_scale, pixel_means, pixel_scale, int(rcnn_stride), out, False)

    def segment_yuv(self, y, uv=None, u=None, v=None, im_scale=1.0, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16, out=None):
        """segment on a decoder's planes: y (C * (n + 1), H, W) and uv | u, v as yuv420_to_bgr_u8 takes N frames, clip by clip, a clip's key
        frame first.  One conversion launch into a BGR stack the estimator owns (self.bgr, (C, n + 1, H, W, 3)); luma_from='y' searches the
        decoder's Y plane (the conversion's y_packed, no luma launch: three launches in all), 'bgr' lsfa_luma_u8 of the converted frames."""
        H, W, C = self.height, self.width, self.clips
        if not isinstance(y, torch.Tensor) or y.dim() != 3 or tuple(y.shape[1:]) != self._y_plane() or y.device != self.device or int(y.shape[0]) % C or \
                int(y.shape[0]) < 2 * C:
            raise LsfaError("SegmentMotionEstimator.segment_yuv: a (%d * (n + 1), %d, %d) uint8 Y stack on %s expected, got %s on %s" %
                            (C, self._y_plane()[0], self._y_plane()[1], self.device, tuple(getattr(y, 'shape', ())), getattr(y, 'device', type(y))))
        n = self._length(int(y.shape[0]) // C - 1, None, 'segment_yuv')
        self._outputs("SegmentMotionEstimator.segment_yuv", n, im_scale, int(rcnn_stride), out)
        if self._bgr is None:
            self._bgr = torch.empty(C * (self.frames + 1) * H * W * 3, dtype=torch.uint8, device=self.device)
        N = C * (n + 1)
        self.bgr = self._bgr[:N * H * W * 3].view(C, n + 1, H, W, 3)
        from_y = self.luma_from == 'y'
        self._to_bgr(y, uv, u, v, self.matrix, out=self.bgr.view(N, H, W, 3), y_packed=self._luma[:N * H * W].view(N, H, W) if from_y else None)
        return self._run(self.bgr, n, im_scale, pixel_means, pixel_scale, int(rcnn_stride), out, from_y)


# ---- live timing -----------------------------------------------------------------------
def prof_enable(on=True, ops=None):
    """on=True times every op; ops=['warp_bilinear', ...] times only those; on=False stops."""
    mask = 0
    if on:
        mask = -1 if ops is None else sum(1 << OP_NAMES.index(o) for o in ops)
    _check(lib().lsfa_prof_enable(mask), "lsfa_prof_enable")


def prof_read():
    """{op_name: (total_ms, launches)} since the last read; synchronises the recorded events."""
    n = len(OP_NAMES)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int * n)()
    _check(lib().lsfa_prof_read(ms, cnt), "lsfa_prof_read")
    return {OP_NAMES[i]: (ms[i], cnt[i]) for i in range(n)}
