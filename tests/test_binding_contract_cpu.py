"""The CPU-tensor column of tests/binding_contract.py on a machine without a GPU: every hip.py wrapper refuses a host tensor in every
tensor position with LsfaError before anything is launched.  The only exceptions are the two places that move host tensors to the
device on purpose (MotionVectorAccumulator.add_frame's mvs, .residual's frames).

hip.lib is a spy around the REAL library (it loads without a GPU): host arithmetic is forwarded, every launching export is recorded and
not called.  The tensors in the other positions are host tensors that claim cuda:0 (binding_contract.FakeCuda), so that the guard of the
position under test is reached whatever the order of the checks."""
import pytest

import binding_contract as bc
from lsfa_amd import hip


@pytest.fixture()
def spied(monkeypatch):
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    with bc.fake_cuda(monkeypatch):
        yield bc.Env(fake=True), spy


@pytest.mark.parametrize("case", bc.CPU_CASES, ids=[c[1] for c in bc.CPU_CASES])
def test_a_host_tensor_is_refused_before_anything_is_launched(spied, case):
    env, spy = spied
    r, _, path, kind = case
    assert bc.run_refusal(env, spy, r, path, kind) is None


@pytest.mark.parametrize("r", bc.ROWS, ids=[r.id for r in bc.ROWS])
def test_the_well_formed_call_reaches_its_exports_under_the_spy(spied, r):
    """the stand-in tensors do not keep a well-formed call from its launch: the refusals above are the guards', not the stand-ins'"""
    env, spy = spied
    bc.run_well_formed(env, spy, r)
    bc.check_expect(spy, r)


def test_every_tensor_position_but_the_moving_sites_is_in_the_cpu_column():
    moved = sorted("%s:%s" % (r.id, p) for r in bc.ROWS for p, a in r.args.items() if a.moved)
    assert moved == ["MotionVectorAccumulator.add_frame:mvs", "MotionVectorAccumulator.residual:bgr_cur", "MotionVectorAccumulator.residual:bgr_ref"]
    skipped = [(r.id, p) for r in bc.ROWS for p, a in r.args.items() if "cpu" in a.skip]
    assert not skipped, skipped
    assert len(bc.CPU_CASES) == sum(len(r.args) for r in bc.ROWS) - len(moved)


def test_the_table_is_complete():
    """every hip.py wrapper that names a launching export of include/lsfa_hip.h has a row, or an exemption for one of the two reasons"""
    wrappers = bc.wrappers_of_launching_exports()
    have = bc.covered()
    missing = sorted(w for w in wrappers if w not in have and w not in bc.EXEMPT)
    assert not missing, "hip.py wrappers of launching exports without a row in tests/binding_contract.py: %s" % missing
    stale = sorted(w for w in bc.EXEMPT if w not in wrappers)
    assert not stale, "exemptions for wrappers that name no launching export: %s" % stale
    for w, reason in bc.EXEMPT.items():
        assert reason.startswith("takes no tensor from the caller") or reason == "a class whose own methods are in the table", (w, reason)
    for cls, tensorless in bc.TENSORLESS_METHODS.items():
        assert bc.EXEMPT[cls] == "a class whose own methods are in the table"
        public = [n for n, v in vars(getattr(hip, cls)).items() if (not n.startswith("_") or n in ("__init__", "__call__")) and
                  (callable(v) or isinstance(v, property))]
        rows = set(r.name.split(".", 1)[1] for r in bc.ROWS if r.name.startswith(cls + "."))
        assert rows, cls
        unlisted = sorted(n for n in public if n not in rows and n not in tensorless and not (n == "__init__" and cls != "SplitWeight"))
        assert not unlisted, "%s: methods with neither a row nor a place among the tensor-less ones: %s" % (cls, unlisted)
    # every launching export is reached by some row's well-formed call, but for those behind wrappers that take no tensor
    reached = set(e for r in bc.ROWS for e in r.expect)
    by_export = bc.test_abi.wrappers_by_export()
    unreached = sorted(e for e in bc.launching_exports() if e not in reached and not by_export.get(e, set()) <= set(bc.EXEMPT))
    assert unreached == sorted(bc.REACHED_ONLY_INDIRECTLY), unreached
