"""Cut named functions and macros out of the reference's native sources, at build time.

Nothing this module writes is committed: the slices go to oracle/_ref/*.inc, which the
committed drivers #include.  A function is found by its name followed by a parameter list
and an opening brace; the slice starts at the first line of its declaration (template<>
line and qualifiers included) and ends at the brace that closes its body.  Comments,
string and character literals are skipped while braces are counted.
"""
import os
import re

# (slice file, source file relative to the reference root, macros, functions) in output order
PLAN = [
    ("psroi.inc", "{ops}/psroi_pooling.cu", ["CUDA_KERNEL_LOOP"], ["PSROIPoolForwardKernel"]),
    ("proposal.inc", "{ops}/multi_proposal.cu", ["DIVUP"],
     ["ProposalGridKernel", "BBoxPredKernel", "FilterBoxKernel", "CopyScoreKernel", "ReorderProposalsKernel",
      "devIoU", "nms_kernel", "PrepareOutput"]),
    ("anchors.inc", "{ops}/multi_proposal-inl.h", [], ["_MakeAnchor", "_Transform", "GenerateAnchors"]),
    ("coviar.inc", "external/data_loader_py2/coviar_data_loader.c", ["MV", "RESIDUAL"], ["create_and_load_mv_residual"]),
]
OPS = "dff_rfcn/operator_cxx"          # the configured network's copy
OPS_TWIN = "rfcn/operator_cxx"         # must hold the same functions, letter for letter


def _skip_noncode(text, i):
    """i at the start of a comment or literal -> index just past it; otherwise i unchanged."""
    if text.startswith("//", i):
        j = text.find("\n", i)
        return len(text) if j < 0 else j
    if text.startswith("/*", i):
        return text.index("*/", i) + 2
    if text[i] in "\"'":
        q, j = text[i], i + 1
        while text[j] != q:
            j += 2 if text[j] == "\\" else 1
        return j + 1
    return i


def _match(text, i, open_ch, close_ch):
    """text[i] == open_ch -> index of the matching close_ch."""
    depth = 0
    while i < len(text):
        j = _skip_noncode(text, i)
        if j != i:
            i = j
            continue
        if text[i] == open_ch:
            depth += 1
        elif text[i] == close_ch:
            depth -= 1
            if depth == 0:
                return i
        i += 1
    raise ValueError("unbalanced %s%s" % (open_ch, close_ch))


def slice_function(text, name):
    for m in re.finditer(r"(?<![\w.>:])%s\s*\(" % re.escape(name), text):
        close = _match(text, m.end() - 1, "(", ")")
        rest = text[close + 1:]
        if not rest.lstrip().startswith("{"):
            continue                                   # a call or a prototype, not the definition
        body_open = close + 1 + (len(rest) - len(rest.lstrip()))
        end = _match(text, body_open, "{", "}") + 1
        start = text.rfind("\n", 0, m.start()) + 1
        while start > 0:                               # walk up over the declaration's earlier lines
            prev = text.rfind("\n", 0, start - 1) + 1
            line = text[prev:start - 1].strip()
            if not line or line[-1] in ";}" or line.startswith(("//", "#")) or line.endswith("*/"):
                break
            start = prev
        return text[start:end] + "\n"
    raise KeyError("no definition of %s" % name)


def slice_macro(text, name):
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s\b" % re.escape(name), text, re.M)
    if m is None:
        raise KeyError("no #define %s" % name)
    end = m.end()
    while True:
        nl = text.find("\n", end)
        nl = len(text) if nl < 0 else nl
        if nl == 0 or text[nl - 1] != "\\":
            return text[m.start():nl] + "\n"
        end = nl + 1


def slices(ref_root, ops=OPS):
    """{slice file: text} for the whole plan."""
    out = {}
    for fname, rel, macros, funcs in PLAN:
        with open(os.path.join(ref_root, rel.format(ops=ops)), "r") as f:
            text = f.read()
        parts = [slice_macro(text, n) for n in macros] + [slice_function(text, n) for n in funcs]
        out[fname] = "\n".join(parts)
    return out


def twin_differences(ref_root):
    """Names of the slice files whose text differs between the two operator_cxx copies (empty = identical)."""
    a, b = slices(ref_root, OPS), slices(ref_root, OPS_TWIN)
    return [fname for fname, rel, _, _ in PLAN if "{ops}" in rel and a[fname] != b[fname]]


def write(ref_root, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for fname, text in slices(ref_root).items():
        with open(os.path.join(out_dir, fname), "w") as f:
            f.write(text)
