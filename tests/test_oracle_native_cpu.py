"""The CPU oracle against the reference's own native code.

tests/golden/ref_native.npz holds what the reference's PSROIPoolForwardKernel, MultiProposal kernels,
anchor utilities and create_and_load_mv_residual compute when they are cut out of the reference tree and
compiled for the host (oracle/ref_native, tests/golden/make_native_golden.py).  oracle/lsfa_oracle.c is a
hand restatement of the same code; here the two must agree bit for bit on every case of the fixture.
Where the reference tree is at hand the fixture itself is regenerated and must come out identical.
"""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import oracle
from oracle import ref_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

PSROI_SETS = ["net", "g3", "p6g3"]
PROPOSAL_CASES = [("a", "a"), ("b", "b"), ("c07", "c"), ("c03", "c")]       # outputs, inputs
MV_SIZES = ["37x23", "96x64"]


@pytest.fixture(scope="module")
def native():
    return np.load(os.path.join(GOLDEN, "ref_native.npz"))


def _generator():
    spec = importlib.util.spec_from_file_location("make_native_golden", os.path.join(GOLDEN, "make_native_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generate_anchors_is_the_references(native):
    assert native["anchors"].shape == (9, 5)
    np.testing.assert_array_equal(oracle.generate_anchors(), native["anchors"][:, :4])
    np.testing.assert_array_equal(native["anchors"][:, 4], 0)


@pytest.mark.parametrize("name", PSROI_SETS)
def test_psroi_pool_is_the_references(native, name):
    scale, D, P, G = native["psroi_%s_params" % name]
    data, rois = native["psroi_%s_data" % name].astype(np.float32), native["psroi_%s_rois" % name]
    assert len(rois) >= 90 and (rois[:, 0] == 1).any()
    got, got_mc = oracle.psroi_pool(data, rois, float(scale), int(D), int(P), int(G), with_mapping=True)
    np.testing.assert_array_equal(got, native["psroi_%s_out" % name])
    np.testing.assert_array_equal(got_mc, native["psroi_%s_map" % name].astype(np.float32))


def proposal_args(native, name, inputs):
    min_size, pre, post, threshold = native["prop_%s_params" % name]
    args = [native["prop_%s_%s" % (inputs, k)] for k in ("prob", "deltas", "im_info")]
    return args, dict(rpn_pre_nms_top_n=int(pre), rpn_post_nms_top_n=int(post), threshold=float(threshold), rpn_min_size=int(min_size))


@pytest.mark.parametrize("name,inputs", PROPOSAL_CASES)
def test_proposal_is_the_references(native, name, inputs):
    args, kw = proposal_args(native, name, inputs)
    decode = oracle.proposal_decode(*args, rpn_min_size=kw["rpn_min_size"])
    np.testing.assert_array_equal(decode, native["prop_%s_decode" % name])
    rois, scores, order, keep, nkeep = oracle.proposal(*args, return_debug=True, **kw)
    np.testing.assert_array_equal(order, native["prop_%s_order" % name])
    np.testing.assert_array_equal(nkeep, native["prop_%s_nkeep" % name])
    np.testing.assert_array_equal(keep, native["prop_%s_keep" % name])
    np.testing.assert_array_equal(rois, native["prop_%s_rois" % name])
    np.testing.assert_array_equal(scores, native["prop_%s_scores" % name])


def test_proposal_cases_reach_the_edges_they_are_for(native):
    """What each case exists for is really in it (the inputs are fixed; this guards the generator)."""
    a = native["prop_a_decode"]
    assert np.isfinite(a).all() and (a[..., 4] == -1).any()
    assert native["prop_a_decode__off"] > 0                                   # the fixture tells the contraction rule
    b_params, b_nkeep = native["prop_b_params"], native["prop_b_nkeep"]
    assert b_params[1] > native["prop_b_order"].shape[1] == 720               # pre clamps to the anchor count
    assert b_nkeep[0] < native["prop_b_rois"].shape[0]                        # the cyclic pad ran
    assert (native["prop_b_decode"][0, :, 4] == -1).mean() > 0.5
    assert native["prop_c07_order"].shape[1] == 200 and native["prop_c03_nkeep"][0] < native["prop_c07_nkeep"][0]


def mv_frames(native, size):
    rows, counts = native["mv_%s_rows" % size], native["mv_%s_counts" % size]
    ends = np.cumsum(counts)
    return [rows[e - c:e] for c, e in zip(counts, ends)]


@pytest.mark.parametrize("size", MV_SIZES)
def test_mv_accumulation_is_the_references(native, size):
    width, height = [int(v) for v in size.split("x")]
    frames = mv_frames(native, size)
    assert len(frames) == 5 and any(len(f) == 0 for f in frames)
    accu = oracle.coviar_identity(width, height)
    for f, rows in enumerate(frames):
        accu = oracle.coviar_accumulate(rows, accu)
        np.testing.assert_array_equal(accu, native["mv_%s_accu" % size][f], err_msg="frame %d" % f)
    np.testing.assert_array_equal(oracle.coviar_mv(accu), native["mv_%s_mv" % size])
    bgr = native["mv_%s_bgr" % size]
    np.testing.assert_array_equal(oracle.coviar_residual(bgr[1], bgr[0], accu), native["mv_%s_res" % size])


# ---------------------------------------------------------------- the recipe itself -------------------------
def test_no_slice_or_object_of_the_reference_is_tracked():
    if not os.path.isdir(os.path.join(ROOT, ".git")):
        pytest.skip("not a git checkout")
    listed = subprocess.run(["git", "ls-files", "oracle/_ref"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if listed.returncode != 0:
        pytest.skip("git cannot read this checkout: %s" % listed.stderr.decode().strip()[:200])
    assert listed.stdout.decode().split() == []
    ignored = subprocess.run(["git", "check-ignore", "-q", "oracle/_ref/psroi.inc"], cwd=ROOT)
    assert ignored.returncode == 0, "oracle/_ref is not in .gitignore"


def test_build_without_a_reference_tree_does_nothing(monkeypatch, tmp_path):
    monkeypatch.setenv("LSFA_REFERENCE", str(tmp_path / "nowhere"))
    assert not ref_native.available()
    assert ref_native.build(force=True) is None
    oracle.build()


needs_reference = pytest.mark.skipif(not ref_native.available(), reason="the reference tree is not on this machine")


@needs_reference
def test_both_operator_copies_hold_the_same_functions():
    """The slices come from dff_rfcn/operator_cxx; rfcn/operator_cxx must hold the same text."""
    from oracle.ref_native import slice as slicer
    assert slicer.twin_differences(ref_native.reference_root()) == []


@needs_reference
def test_fixture_is_reproducible_from_the_reference(native):
    """Rebuild oracle/_ref from the reference tree, run the generator: every array of the committed npz, the
    off / fast counts included, comes out again exactly."""
    fresh = _generator().generate()
    assert sorted(fresh) == sorted(native.files)
    for key in native.files:
        want, got = native[key], np.asarray(fresh[key])
        assert want.dtype == got.dtype and want.shape == got.shape, key
        np.testing.assert_array_equal(got, want, err_msg=key)
