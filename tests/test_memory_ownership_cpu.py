"""tests/guarded_arena.py reports what it claims to, shown on a machine without a GPU.

The arena sits on the host and its tensors claim cuda:0 (binding_contract.FakeCuda), as in test_binding_contract_cpu.py.  Each planted
fault is a small Python "wrapper" written with torch ops on views of the arena's own storage: all of its accesses stay inside that
storage.  Each fault must be reported and its correct twin must pass."""
import pytest
import torch

import binding_contract as bc
import guarded_arena as ga


class PlantedRow(object):
    """a row in the table's form around a Python wrapper: make(env) -> (fn, kwargs)"""

    def __init__(self, fn, n=8, out=True):
        self.id = self.name = fn.__name__
        self.fn, self.n, self.out = fn, n, out

    def make(self, env):
        if isinstance(env, ga.GuardedEnv):
            x = env.f32(self.n)
        else:                       # the unguarded run: x is preceded and followed by values of its own allocation, small and finite
            whole = env.f32(self.n + 2)
            values = bc.Env(fake=True).f32(self.n)
            whole[0], whole[-1] = 0.125, -0.25
            whole[1:-1] = values
            x = whole[1:-1]
        kw = dict(x=x)
        if self.out:
            kw["out"] = env.zeros(self.n)
        return self.fn, kw


def around(t, before, after):
    """the elements of t with `before` more in front and `after` more behind, as a view of the storage t lies in"""
    assert t.storage_offset() >= before and t.untyped_storage().nbytes() >= (t.storage_offset() + t.numel() + after) * t.element_size()
    return torch.as_strided(bc.plain(t), (t.numel() + before + after,), (1,), t.storage_offset() - before)


def three_runs(row):
    with pytest.MonkeyPatch.context() as mp, bc.fake_cuda(mp):
        plain = ga.run_plain(row, fake=True)
    return plain, ga.run_guarded(row, 0xFF, fake=True), ga.run_guarded(row, 0x7F, fake=True)


# ---- the arena itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ga.PATTERNS)
def test_a_placed_tensor_is_aligned_banded_and_holds_its_values(pattern):
    arena = ga.Arena(pattern, fake=True)
    env = ga.GuardedEnv(arena)
    small, big, none = env.f32(3, 5), env.u8(3, 100000), env.i32(0, 4)
    assert torch.equal(bc.plain(small), bc.plain(bc.Env(fake=True).f32(3, 5))), "the guarded table's values are the table's"
    for t in (small, big, none):
        p = arena.record(t)
        assert p.tensor is t and t.is_cuda and t.is_contiguous()
        assert (p.buf.data_ptr() + p.start) % 256 == 0
        band = -(-max(64 * 1024, p.nbytes) // 256) * 256
        assert p.start >= band and p.buf.numel() - p.start - p.nbytes >= band
        assert bool((p.buf[:p.start] == pattern).all()) and bool((p.buf[p.start + p.nbytes:] == pattern).all())
    assert arena.record(big).start >= 300000
    arena.check()
    assert len(arena.placed) == 3


def test_the_two_patterns_read_as_documented():
    f = lambda b, dt: ga.Arena(b, fake=True).place((1,), dt, "x")
    assert torch.isnan(f(0xFF, torch.float32)).all() and torch.isnan(f(0xFF, torch.float64)).all()
    assert int(f(0xFF, torch.int32)) == -1 and int(f(0xFF, torch.uint8)) == 255
    assert 3.38e38 < float(f(0x7F, torch.float32)) < 3.40e38 and int(f(0x7F, torch.int32)) == 2139062143


# ---- (a) a stray store ------------------------------------------------------------------------------------------------------------------
def copy_exact(x, out):
    out.copy_(x)
    return out


def copy_one_past(x, out):
    around(out, 0, 1)[:-1].copy_(bc.plain(x))
    around(out, 0, 1)[-1] = 1.0
    return out


def copy_one_before(x, out):
    around(out, 1, 0)[1:].copy_(bc.plain(x))
    around(out, 1, 0)[0] = 1.0
    return out


@pytest.mark.parametrize("pattern", ga.PATTERNS)
def test_a_stray_store_is_reported_with_its_tensor_and_offset(pattern):
    ga.run_guarded(PlantedRow(copy_exact), pattern, fake=True)
    with pytest.raises(AssertionError) as e:
        ga.run_guarded(PlantedRow(copy_one_past), pattern, fake=True)
    assert "out (8,) torch.float32" in str(e.value) and "the first at +0 bytes from its end" in str(e.value) and "x (8,)" not in str(e.value)
    with pytest.raises(AssertionError) as e:
        ga.run_guarded(PlantedRow(copy_one_before), pattern, fake=True)
    assert "out (8,) torch.float32" in str(e.value) and "the first at -4 bytes from its start" in str(e.value)
    # 1.0f is 00 00 80 3F: all four bytes differ from either pattern
    assert "4 byte(s) changed" in str(e.value)


def test_a_stray_store_far_inside_the_band_and_in_an_allocated_tensor_is_reported():
    def far(x):
        out = torch.empty(x.numel(), dtype=torch.float32, device="cuda:0")
        out.copy_(x)
        around(out, 0, 16000)[-1] = 0.0
        return out
    with pytest.raises(AssertionError) as e:
        ga.run_guarded(PlantedRow(far, out=False), 0xFF, fake=True)
    assert "torch.empty (8,) torch.float32" in str(e.value) and "the first at +63996 bytes from its end" in str(e.value)


# ---- (b) an unwritten output ------------------------------------------------------------------------------------------------------------
def doubled(x):
    out = torch.empty(x.numel(), dtype=torch.float32, device="cuda:0")
    out.copy_(2 * bc.plain(x))
    return out


def doubled_but_for_the_last(x):
    out = torch.empty(x.numel(), dtype=torch.float32, device="cuda:0")
    out[:-1].copy_(2 * bc.plain(x)[:-1])
    return out


def test_an_unwritten_output_element_differs_between_the_patterns():
    plain, ff, sf = three_runs(PlantedRow(doubled, out=False))
    assert ga.same(plain, ff) and ga.same(plain, sf)
    plain, ff, sf = three_runs(PlantedRow(doubled_but_for_the_last, out=False))
    assert not ga.same(ff, sf) and not ga.same(plain, ff) and not ga.same(plain, sf)
    assert torch.equal(ff[0][:-1], sf[0][:-1]) and torch.isnan(ff[0][-1]) and float(sf[0][-1]) > 3e38


# ---- (c) a stray read -------------------------------------------------------------------------------------------------------------------
def total(x, out):
    out[0] = bc.plain(x).sum()
    return out


def total_from_one_before(x, out):
    out[0] = around(x, 1, 0).sum()
    return out


def test_a_stray_read_changes_the_result_against_the_unguarded_run():
    plain, ff, sf = three_runs(PlantedRow(total))
    assert ga.same(plain, ff) and ga.same(plain, sf)
    plain, ff, sf = three_runs(PlantedRow(total_from_one_before))
    assert torch.isfinite(plain[0]).all(), "unguarded, the stray value is small and finite: a value test with a tolerance can pass"
    assert not ga.same(plain, ff) and not ga.same(plain, sf)


# ---- (d) a NaN-blind reduction: why there are two patterns ------------------------------------------------------------------------------------
def nan_ignoring_max(v):
    return torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v).max()


def amax(x, out):
    out[0] = nan_ignoring_max(bc.plain(x).abs())
    return out


def amax_over_one_too_many(x, out):
    out[0] = nan_ignoring_max(around(x, 0, 1).abs())
    return out


def test_a_nan_ignoring_maximum_over_one_too_many_is_missed_by_ff_and_caught_by_7f():
    plain, ff, sf = three_runs(PlantedRow(amax))
    assert ga.same(plain, ff) and ga.same(plain, sf)
    plain, ff, sf = three_runs(PlantedRow(amax_over_one_too_many))
    assert ga.same(plain, ff), "0xFF is NaN, which the maximum ignores: this pattern alone misses the fault"
    assert not ga.same(plain, sf) and float(sf[0][0]) > 3e38


# ---- (e) what passes through --------------------------------------------------------------------------------------------------------------
def test_cpu_and_pinned_allocations_pass_through(monkeypatch):
    calls = []
    real = torch.empty

    def spy(*args, **kw):
        calls.append((args, dict(kw)))
        kw.pop("pin_memory", None)              # (pinning needs a GPU; what is checked is that the request arrives as it was made)
        return real(*args, **kw)
    monkeypatch.setattr(torch, "empty", spy)
    arena = ga.Arena(0xFF, fake=True)
    with ga.guarded_allocations(monkeypatch, arena):
        a = torch.empty(4, dtype=torch.int32)
        b = torch.empty((2, 3), pin_memory=True)
        c = torch.zeros(5, device="cpu")
        d = torch.zeros_like(c)
        e = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
        f = torch.empty_like(e)
    # (torch's own meta-device helpers may call torch.empty after these two)
    assert calls[:2] == [((4,), dict(dtype=torch.int32)), (((2, 3),), dict(pin_memory=True))]
    assert all(torch.device(kw["device"]).type == "meta" for _, kw in calls[2:])
    assert all(type(t) is torch.Tensor and arena.record(t) is None for t in (a, b, c, d))
    assert not c.any() and not d.any() and tuple(b.shape) == (2, 3)
    assert [p.role for p in arena.placed] == ["torch.full", "torch.empty_like"]
    assert e.is_cuda and e.tolist() == [7, 7] and f.is_cuda and f.tolist() == [-1, -1]
    assert torch.empty is spy, "the redirection ends with the context"
    arena.check()


def test_objects_that_allocate_in_init_are_covered(monkeypatch):
    """the table's call under the spy, as in test_binding_contract_cpu.py: the estimator's own buffers come from the arena"""
    from lsfa_amd import hip
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    arena = ga.Arena(0x7F, fake=True)
    with bc.fake_cuda(monkeypatch), ga.guarded_allocations(monkeypatch, arena):
        row = [r for r in bc.ROWS if r.id == "SegmentMotionEstimator.segment"][0]
        fn, kw = row.make(ga.GuardedEnv(arena))
        before = len(arena.placed)
        fn(**kw)
    assert before > 3 and sum(p.role.startswith("torch.") for p in arena.placed) >= 3, [str(p) for p in arena.placed]
    assert spy.launched()
    arena.check()


def test_the_ragged_convolutions_reach_the_kernels_their_ids_name(monkeypatch):
    """RAGGED's convolution rows under the spy, the plan of every recorded lsfa_conv_fwd asked of the real library (host arithmetic): a row
    called `direct` runs the direct kernel, a forced ring plan is the plan that runs, three slices bring the reduce pass, kernel 4 the
    eight-wave tiles, the cut rows the input's activation"""
    import re
    import test_memory_ownership_gpu as own
    from lsfa_amd import hip
    real, plans = hip.lib(), []

    class PlanSpy(bc.Spy):
        def __getattr__(self, name):
            if name in ("lsfa_conv_plan_query", "lsfa_conv_plan_override"):
                return getattr(self.real, name)
            if name == "lsfa_conv_fwd":
                return lambda d, *rest: plans.append(hip._plan_kernel_name(d._obj)) or 0
            return bc.Spy.__getattr__(self, name)
    spy = PlanSpy(real)
    monkeypatch.setattr(hip, "lib", lambda: spy)
    seen = 0
    with bc.fake_cuda(monkeypatch):
        for r in own.RAGGED:
            if r.name not in ("conv_split", "conv_split_view"):
                continue
            del plans[:]
            fn, kw = r.make(bc.Env(fake=True))
            fn(**kw)
            assert len(plans) == 1, (r.id, plans)
            plan, seen = plans[0], seen + 1
            if "direct" in r.id:
                assert plan.startswith("conv_split_direct_kernel"), (r.id, plan)
                continue
            if not r.id.startswith(("conv_split[ring-", "conv_split[cut-")):
                continue                            # (the views: whichever kernel the plan picks)
            nt, pc, st, sp, af, wv = re.match(r"conv_ring_kernel<(\d), (\d), (\d), (\w+), (\w+), (\d)>", plan).groups()
            m = re.match(r"conv_split\[ring-p(\d)-k(\d)-nt(\d)-s(\d)-", r.id)
            if m:
                p, k, want_nt, s = m.groups()
                assert (pc, nt) == (p, want_nt) and plan.endswith("+split_reduce") == (s == "3"), (r.id, plan)
                assert (sp, wv) == {"1": ("false", "4"), "2": ("true", "4"), "4": ("false", "8")}[k], (r.id, plan)
            if "[cut-" in r.id:
                assert af == "true" and plan.endswith("+split_reduce") == r.id.endswith("s3]"), (r.id, plan)
    assert seen > 60 and real.lsfa_conv_plan_query is not None


def test_every_allocation_site_of_hip_py_is_reached_by_a_row(monkeypatch):
    """the legal rows of the table and RAGGED under the spy: every line of lsfa_amd/hip.py that calls torch.empty / zeros / ones / full /
    empty_like / zeros_like is executed by at least one of the calls the GPU test guards"""
    import re
    import sys
    import test_memory_ownership_gpu as own
    from lsfa_amd import hip
    path = hip.__file__
    names = ("empty", "zeros", "full", "ones", "empty_like", "zeros_like")
    lines = open(path).read().split("\n")
    sites = set(i + 1 for i, l in enumerate(lines) if re.search(r"torch\.(%s)\(" % "|".join(names), l) and not l.strip().startswith('"""'))
    assert len(sites) > 80
    seen = set()

    def watch(fn):
        def alloc(*args, **kw):
            frame = sys._getframe(1)
            if frame.f_code.co_filename == path:
                seen.add(frame.f_lineno)
            return fn(*args, **kw)
        return alloc
    spy = bc.Spy(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: spy)
    with bc.fake_cuda(monkeypatch):
        for name in names:
            monkeypatch.setattr(torch, name, watch(getattr(torch, name)))
        for r in [r for r in bc.ROWS if r.legal] + own.RAGGED:
            fn, kw = r.make(bc.Env(fake=True))
            fn(**kw)
    missed = sorted(sites - seen)
    assert not missed, "allocation sites of lsfa_amd/hip.py that no guarded row reaches: %s" % ["%d: %s" % (i, lines[i - 1].strip()) for i in missed]


def test_the_exemptions_cite_header_lines_that_say_so_and_name_no_whole_output():
    import os
    import test_memory_ownership_gpu as own
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lsfa_hip.h")).read().split("\n")
    known = set(r.name for r in bc.ROWS) | set(r.name for r in own.RAGGED)
    assert own.UNDEFINED
    for wrapper, region, where, _ in own.UNDEFINED:
        m = __import__("re").match(r"include/lsfa_hip\.h:(\d+)", where)
        assert wrapper in known and m, (wrapper, where)
        assert "not written" in header[int(m.group(1)) - 1] or "undefined" in header[int(m.group(1)) - 1], (wrapper, where, header[int(m.group(1)) - 1])
        assert re_region(region), "an exemption names a part of an output, never a whole one: %r" % region


def re_region(region):
    """`name[a:b]` with at least one bound given"""
    import re
    m = re.match(r"^\w+\[(\w*):(\w*)\]$", region)
    return bool(m and (m.group(1) or m.group(2)))
