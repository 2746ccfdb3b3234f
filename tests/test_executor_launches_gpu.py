"""The executor's convolution launches, pass by pass, against tests/golden/executor_launches.json.

The file was recorded on an MI355X by tests/golden/make_executor_launches.py on the commit before the convolution binding and the
executor were refactored, and is NOT regenerated when they change: it pins which convolutions a pass launches, on which kernel
instantiation the launch plan puts each (the plan's choices on an MI355X), and the FLOPs and bytes bench.py's roofline is fed with."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_executor_launches", os.path.join(GOLDEN_DIR, "make_executor_launches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def world(hip):
    return REC.World()


@pytest.fixture(scope="module")
def recorded():
    with open(REC.GOLDEN) as f:
        return json.load(f)


def test_the_record_covers_every_group(recorded):
    assert (recorded["height"], recorded["width"]) == (REC.H, REC.W)
    assert sorted(recorded["groups"]) == sorted(REC.GROUPS)


@pytest.mark.parametrize("group", REC.GROUPS)
def test_executor_launch_census(world, recorded, group):
    """launches, kernel names and calls exactly, gflop / mbytes as conv_by_kernel() rounds them: the record holds the launch plan's
    choices on an MI355X, as the commit before the refactor made them"""
    want, got = recorded["groups"][group], world.run(group)
    assert sorted(got) == sorted(want)
    for name, w in want.items():
        g = got[name]
        print("%s / %s: %d launches, %.3f GFLOP, %.3f MB, %d kernels" % (group, name, g["launches"], g["flops"] / 1e9, g["bytes"] / 1e6, len(g["by_kernel"])))
        assert g["launches"] == w["launches"], (group, name)
        assert sorted(g["by_kernel"]) == sorted(w["by_kernel"]), (group, name)
        assert g["by_kernel"] == w["by_kernel"], (group, name)          # calls exactly; gflop / mbytes as conv_by_kernel() rounds them
        for k in ("flops", "flops_three_products", "flops_one_product", "bytes"):
            assert g[k] == w[k], (group, name, k)
