"""Every way tests/binding_contract.py knows to hand a hip.py wrapper a wrong tensor - on the host, of another dtype, a view of a
larger buffer where the wrapper writes, one row or channel short, the same values in another rank or order, None where one is required,
and the mismatches BETWEEN arguments - is refused with LsfaError before anything is launched.

NOTHING HERE REACHES A KERNEL: hip.lib is a spy around the real library that forwards host arithmetic and records every launching
export instead of calling it.  A missing guard is a failed assertion (a recorded launch, or an exception that is not LsfaError), never
an access through a foreign pointer."""
import pytest

import binding_contract as bc

pytestmark = pytest.mark.gpu


@pytest.fixture()
def spied(hip, monkeypatch):
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    return bc.Env(fake=False), spy


@pytest.mark.parametrize("case", bc.ALL_CASES, ids=[c[1] for c in bc.ALL_CASES])
def test_a_wrong_tensor_is_refused_before_anything_is_launched(spied, case):
    env, spy = spied
    r, _, path, kind = case
    assert bc.run_refusal(env, spy, r, path, kind) is None


@pytest.mark.parametrize("r", bc.ROWS, ids=[r.id for r in bc.ROWS])
def test_the_well_formed_call_reaches_its_exports_with_the_sizes_of_its_tensors(spied, r):
    env, spy = spied
    bc.run_well_formed(env, spy, r)
    assert spy.calls, "%s launched nothing" % r.id
    bc.check_expect(spy, r)


def test_the_spy_forwards_host_arithmetic_and_launches_nothing(spied, hip):
    _, spy = spied
    assert hip.lib() is spy
    assert spy.lsfa_abi_version() == 1 and spy.lsfa_nms_workspace_bytes(6000) >= 6000 * 94 * 8
    assert spy.lsfa_status_check(None, None) == 0 and spy.launched() == ["lsfa_status_check"]
    with pytest.raises(AttributeError):
        spy.lsfa_no_such_export
    with pytest.raises(AssertionError):
        getattr(spy, "lsfa_status_check")(None)     # the recorder keeps the header's arity (getattr: test_abi counts the arguments of plain calls)


def test_every_row_mutates_every_tensor_it_passes(spied):
    """a tensor in a row's call that the row's `args` does not list would go unmutated: the table, checked against itself"""
    env, spy = spied
    import torch

    def paths(v, at=()):
        if isinstance(v, torch.Tensor):
            yield at
        elif isinstance(v, (tuple, list)) and not isinstance(v, bc.hip.PhaseWeights):
            for i, e in enumerate(v):
                for p in paths(e, at + (i,)):
                    yield p
    for r in bc.ROWS:
        _, kw = r.make(env)
        have = set(p if isinstance(p, tuple) else (p,) for p in r.args)
        passed = set(p for k, v in kw.items() for p in paths(v, (k,)))
        assert passed == have, "%s: tensors passed %s, tensors mutated %s" % (r.id, sorted(passed - have), sorted(have - passed))
