"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports
every symbol include/lsfa_hip.h declares; the product never touches the oracle."""
import ast
import ctypes
import os
import re

import torch  # noqa: F401  (loads the HIP runtime the library binds to)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "lsfa_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
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
    """export -> names of the top-level functions / classes of lsfa_amd/hip.py whose body names it (`lib` itself only sets return types)"""
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

