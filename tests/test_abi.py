"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports
every symbol include/lsfa_hip.h declares, and lsfa_amd/hip.py binds them with the header's own prototypes and struct; the product
never touches the oracle."""
import ast
import ctypes
import os
import re
import subprocess

import pytest

import torch  # noqa: F401  (loads the HIP runtime the library binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    """the header without comments and preprocessor lines (a `#define NAME (-4)` in front of a prototype read as a call and hid the
    prototype from the searches below: lsfa_last_error and lsfa_status_check)"""
    text = open(os.path.join(ROOT, "include", "lsfa_hip.h")).read()
    return re.sub(r"^[ \t]*#.*$", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.M)


def declared_symbols():
    text = header_text()
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", text)
    return sorted(set(n for n in names if n.startswith("lsfa_") or n == "_nms"))


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for want in ("lsfa_psroi_pool_fwd", "lsfa_rfcn_head_fwd", "lsfa_warp_bilinear", "lsfa_aggregate_softmax2",
                 "lsfa_aggregate_cosine", "lsfa_proposal", "lsfa_nms_sorted", "_nms", "lsfa_det_postprocess",
                 "lsfa_bbox_pred_clip", "lsfa_deform_im2col", "lsfa_deform_im2col_cl", "lsfa_deform_im2col_cl_ld", "lsfa_scale_shift_relu", "lsfa_scale_shift_relu_cl", "lsfa_scale_shift_leaky", "lsfa_prof_read"):
        assert want in syms


def test_library_builds_loads_and_exports_every_declared_symbol():
    from lsfa_amd import build
    path = build.build_hip()
    lib = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(lib, name), "liblsfa_hip.so does not export %s" % name
    lib.lsfa_abi_version.restype = ctypes.c_int
    assert lib.lsfa_abi_version() == 1
    lib.lsfa_op_name.restype = ctypes.c_char_p
    from lsfa_amd import hip
    assert [lib.lsfa_op_name(i).decode() for i in range(len(hip.OP_NAMES))] == hip.OP_NAMES
    # ... and the table is COMPLETE: lsfa_prof_read fills LSFA_OP_COUNT entries of buffers the binding sizes by this list (an
    # out-of-date copy, one short, let it write past them and hung bench.py: r3)
    assert lib.lsfa_op_name(len(hip.OP_NAMES)) == b"?"
    # workspace sizing is host-only arithmetic: float4 boxes + u32 keys for the 21,546 anchors (no NMS mask)
    lib.lsfa_proposal_workspace_bytes.restype = ctypes.c_size_t
    ws = lib.lsfa_proposal_workspace_bytes(1, 9, 38, 63, 6000)
    # boxes + keys of the decode kernel, then the chip-wide plan's histograms, candidate list, ranks and the
    # 6000 x 94 x 8-byte suppression mask (the reference cudaMallocs that mask on every call)
    assert 21546 * 20 + 6000 * 94 * 8 <= ws < 8 << 20
    assert 21546 * 20 <= lib.lsfa_proposal_workspace_bytes(1, 9, 38, 63, 12000) < 21546 * 20 + 1024   # single-workgroup plan
    lib.lsfa_nms_workspace_bytes.restype = ctypes.c_size_t
    assert lib.lsfa_nms_workspace_bytes(6000) >= 6000 * 94 * 8


def declared_arity():
    """export -> number of parameters, counted here from the header's text (commas of the parameter list; `(void)` is none)"""
    out = {}
    for name, params in re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{]*)\)\s*;", header_text()):
        if name.startswith("lsfa_") or name == "_nms":
            out[name] = 0 if params.strip() == "void" else params.count(",") + 1
    return out


def test_bound_prototypes_cover_the_header():
    from lsfa_amd import hip
    lib = hip.lib()
    assert sorted(hip._PROTOTYPES) == declared_symbols()
    arity = declared_arity()
    assert sorted(arity) == declared_symbols()
    size_t = []
    for name in declared_symbols():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == arity[name], name
        if fn.restype is ctypes.c_size_t:
            size_t.append(name)
        elif name in ("lsfa_op_name", "lsfa_last_error"):
            assert fn.restype is ctypes.c_char_p, name
        elif name == "_nms":
            assert fn.restype is None
        else:
            assert fn.restype is ctypes.c_int, name
    assert size_t == sorted(n for n in declared_symbols() if n.endswith("_bytes")) and len(size_t) == 10
    assert lib.lsfa_conv_fwd.argtypes[0] is ctypes.POINTER(hip.ConvDesc)
    assert lib.lsfa_conv_plan_query.argtypes == [ctypes.POINTER(hip.ConvDesc), ctypes.c_void_p]
    assert lib.lsfa_amax_partial.argtypes[1] is ctypes.c_longlong and lib.lsfa_aggregate_softmax2_rows.argtypes[3] is ctypes.c_long
    assert lib.lsfa_image_transform_u8.argtypes[5] is ctypes.c_double and lib.lsfa_nms_sorted.argtypes[3] is ctypes.c_float


def test_conv_desc_has_the_layout_the_compiler_gives_the_header(tmp_path):
    """sizeof / offsetof of struct lsfa_conv_desc from a C program built on the header against the ctypes structure hip.py derives from
    the same text: a field the header lacks does not compile, a field hip.py lacks changes the size or a later offset."""
    from lsfa_amd import hip
    names = [f[0] for f in hip.ConvDesc._fields_]
    assert len(names) == 39 and names[0] == "x" and names[-1] == "w_scale"
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"lsfa_hip.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(lsfa_conv_desc));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(lsfa_conv_desc, %s));\n" % (n, n) for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    cc = subprocess.run([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    assert int(got[0]) == ctypes.sizeof(hip.ConvDesc) == 224
    assert [ln for ln in got[1:] if ln] == ["%s %d" % (n, getattr(hip.ConvDesc, n).offset) for n in names]


def test_wrong_calls_are_rejected():
    """host-only exports: the prototypes refuse what a bare CDLL passed through"""
    lib = __import__("lsfa_amd.hip", fromlist=["lib"]).lib()
    ws = lib.lsfa_proposal_workspace_bytes(1, 9, 38, 63, 6000)          # plain ints, a size_t back
    assert 21546 * 20 + 6000 * 94 * 8 <= ws < 8 << 20
    assert lib.lsfa_nms_workspace_bytes(6000) >= 6000 * 94 * 8
    with pytest.raises(TypeError):
        lib.lsfa_proposal_workspace_bytes(1, 9, 38, 63)                 # a missing argument
    with pytest.raises(ctypes.ArgumentError):
        lib.lsfa_proposal_workspace_bytes(1, 9, 38.0, 63, 6000)         # a float where an int is declared
    with pytest.raises(ctypes.ArgumentError):
        lib.lsfa_conv_weight_bytes(64, 3, 3, 32, 2.0)
    with pytest.raises(ctypes.ArgumentError):
        lib.lsfa_conv_workspace_bytes(ctypes.c_int(0))                  # not a lsfa_conv_desc*
    assert lib.lsfa_op_name(0) == b"psroi_pool"
    from lsfa_amd import hip
    for decl in ("uint64_t n", "short n", "void n"):                     # a type outside the binder's table is an error, not a guess
        with pytest.raises(hip.LsfaError, match="no ctypes type"):
            hip._ctype(decl)


SCANNED = ("lsfa_amd", "tools", "tests", "bench.py", "__graft_entry__.py")
# hip.py's star-expanded calls of an lsfa_* attribute: the three lsfa_*yuv420* wrappers, which share _yuv_planes' leading arguments.  NOT seen
# by this scan: hip._warp, which picks one of the four lsfa_warp_bilinear* exports by name (getattr) and star-expands a list built for it.  ctypes
# refuses a short list there as everywhere; a surplus argument would pass, and only the gpu-marked warp tests, which run all four, stand
# between that and the library.
STAR_CALLS_IN_HIP = 3


def abi_calls():
    """(file, line, export, positional argument count or None for a star-expanded call) of every call of an lsfa_* / _nms attribute; calls
    inside a `with pytest.raises(...)` block of THIS file are wrong on purpose and left out"""
    files = []
    for entry in SCANNED:
        path = os.path.join(ROOT, entry)
        if os.path.isfile(path):
            files.append(path)
        for d, _, names in os.walk(path):
            files += [os.path.join(d, f) for f in names if f.endswith(".py")]
    for path in sorted(files):
        tree = ast.parse(open(path).read(), path)
        meant_to_fail = set(id(n) for w in ast.walk(tree) if path == os.path.abspath(__file__) and isinstance(w, ast.With) and
                            "pytest.raises" in ast.unparse(w.items[0].context_expr) for n in ast.walk(w))
        for node in ast.walk(tree):
            if id(node) in meant_to_fail:
                continue
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and (node.func.attr.startswith("lsfa_") or node.func.attr == "_nms"):
                star = any(isinstance(a, ast.Starred) for a in node.args) or any(k.arg is None for k in node.keywords)
                yield os.path.relpath(path, ROOT), node.lineno, node.func.attr, None if star else len(node.args) + len(node.keywords)


def test_every_call_site_passes_as_many_arguments_as_the_header_declares():
    arity, calls = declared_arity(), list(abi_calls())
    assert len(calls) > 100 and any(c[0] == os.path.join("lsfa_amd", "hip.py") for c in calls)
    unknown = [c for c in calls if c[2] not in arity]
    assert not unknown, "calls of exports the header does not declare: %s" % unknown
    wrong = [c + (arity[c[2]],) for c in calls if c[3] is not None and c[3] != arity[c[2]]]
    assert not wrong, "(file, line, export, passed, declared): %s" % wrong
    stars = [c for c in calls if c[3] is None and c[0] == os.path.join("lsfa_amd", "hip.py")]
    assert len(stars) <= STAR_CALLS_IN_HIP, stars


def test_the_binding_holds_no_casts_of_its_own():
    """lsfa_amd/hip.py and lsfa_amd/core/streams.py pass plain Python values: no scalar ctypes object is built from a value (c_int() /
    c_void_p() out-parameters and the ctypes ARRAYS are data, not casts), restype is set by the binder alone."""
    hip_src = open(os.path.join(ROOT, "lsfa_amd", "hip.py")).read()
    both = hip_src + open(os.path.join(ROOT, "lsfa_amd", "core", "streams.py")).read()
    assert not re.findall(r"\bc_(?:u?int|u?long|u?longlong|size_t|float|double|void_p|char_p|bool)\(\s*[^)\s]", both)
    assert not re.findall(r"\b_(?:ci|cf|cd|cll|dp|vp)\b", both)
    assert not re.search(r"^\s*(?:from ctypes import|import ctypes as)|=\s*ctypes\.c_\w+\s*$", both, flags=re.M)        # no aliases to cast through
    assert len(re.findall(r"\.restype\b", both)) == 1 and len(re.findall(r"\.argtypes\b", both)) == 1


def test_product_never_imports_the_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "lsfa_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                if re.search(r"^\s*(import|from)\s+oracle\b", txt, flags=re.M) or "lsfa_oracle" in txt or "liblsfa_oracle" in txt:
                    bad.append(os.path.join(d, f))
    assert not bad, "product code references the oracle: %s" % bad


# exports that launch nothing (host arithmetic, process-wide switches) or only manage handles: no kernel to compare with anything
NO_KERNEL = {
    "lsfa_abi_version": "a constant",
    "lsfa_last_error": "the thread's message string",
    "lsfa_op_name": "a name table, checked against hip.OP_NAMES above",
    "lsfa_stream_create": "creates a stream handle",
    "lsfa_stream_destroy": "destroys a stream handle",
    "lsfa_prof_enable": "switches the per-operator timers",
    "lsfa_conv_plan_override": "process-wide launch-plan switch for A/B runs",
    "lsfa_conv_order_override": "process-wide tile-order switch for A/B runs",
    "lsfa_warp_set_variant": "process-wide kernel-variant switch",
    "lsfa_proposal_set_plan": "process-wide plan switch",
    "lsfa_channel_mean_workspace_bytes": "host arithmetic",
    "lsfa_conv_nhwc_workspace_bytes": "host arithmetic",
    "lsfa_conv_workspace_bytes": "host arithmetic",
    "lsfa_deconv4x4s2_crop_workspace_bytes": "host arithmetic",
    "lsfa_det_workspace_bytes": "host arithmetic",
    "lsfa_mv_workspace_bytes": "host arithmetic",
    "lsfa_nms_workspace_bytes": "host arithmetic",
    "lsfa_proposal_workspace_bytes": "host arithmetic",
    "lsfa_conv_weight_bytes": "host arithmetic",
    "lsfa_stem_weight_bytes": "host arithmetic",
}


def wrappers_by_export():
    """export -> names of the top-level functions / classes of lsfa_amd/hip.py whose body names it (`lib` binds them all and calls none but
    lsfa_op_name and lsfa_warp_set_variant)"""
    src = open(os.path.join(ROOT, "lsfa_amd", "hip.py")).read()
    found = {}
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name != "lib":
            for sym in set(re.findall(r"\b(?:lsfa_[A-Za-z0-9_]+|_nms)\b", ast.get_source_segment(src, node))):
                found.setdefault(sym, set()).add(node.name)
    return found


def gpu_test_modules():
    mods = {}
    tests = os.path.join(ROOT, "tests")
    for f in sorted(os.listdir(tests)):
        if f.startswith("test_") and f.endswith(".py"):
            txt = open(os.path.join(tests, f)).read()
            if re.search(r"^pytestmark\s*=\s*pytest\.mark\.gpu\b|^@pytest\.mark\.gpu\b", txt, flags=re.M):
                mods[f] = txt
    return mods


def test_every_export_has_a_direct_gpu_test():
    """Every lsfa_* export of the header that launches something is named by a gpu-marked test module, or one of the hip.py wrappers
    that call it is (`hip.<wrapper>`).  A NAME SEARCH is a weak notion of "tested": it says nothing about what the test asserts.  Its
    job is to make the next export that no test calls show up in review, not to prove coverage."""
    syms = declared_symbols()
    stale = sorted(set(NO_KERNEL) - set(syms))
    assert not stale, "exempted exports that the header no longer declares: %s" % stale
    wrappers, mods = wrappers_by_export(), gpu_test_modules()
    assert "test_hip_ops.py" in mods and "test_hip_ops_direct.py" in mods
    missing = []
    for sym in syms:
        if sym in NO_KERNEL:
            continue
        pats = [r"\b%s\b" % re.escape(sym)] + [r"\bhip\.%s\b" % re.escape(w) for w in sorted(wrappers.get(sym, ()))]
        if not any(re.search(p, txt) for p in pats for txt in mods.values()):
            missing.append((sym, sorted(wrappers.get(sym, ()))))
    assert not missing, "exports (and their hip.py wrappers) that no gpu-marked test module names: %s" % missing

