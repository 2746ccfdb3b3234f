"""The convolution launch plan is host arithmetic: lsfa_conv_plan_query, lsfa_conv_workspace_bytes and
lsfa_deconv4x4s2_crop_workspace_bytes answer without a GPU.  tests/golden/conv_plans.json holds their answers for ~9000 descriptors
and override settings, recorded (tests/golden/make_conv_plans.py, which also explains the file's layout) on the commit before the
launch code became one plan function; the library of this tree has to reproduce every one of them exactly.  Each check runs in a
fresh child process, because the library parses its environment switches once per process."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_conv_plans", os.path.join(HERE, "golden", "make_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "conv_plans.json")) as f:
        g = json.load(f)
    for group in g["groups"] + g["env"]:
        group["want"] = [g["answers"][i] for i in group["out"]]
    return g


def _assert_reproduced(rec, groups, env):
    """the groups' recorded answers against this tree's library in a fresh process with only `env`'s lab switches set; -> its answers"""
    got = rec.eval_in_child([{"kind": g.get("kind", "conv"), "factors": g["factors"]} for g in groups], env)
    for g, res in zip(groups, got):
        assert len(res) == len(g["want"])
        bad = [(r, a, b) for r, a, b in zip(rec.rows_of(g), res, g["want"]) if a != b]
        assert not bad, "%s, %s: %d of %d rows differ; the first (row, got, recorded): %s" % (env, g["what"], len(bad), len(res), bad[:3])
    return got


def test_every_recorded_plan_and_workspace_size_is_reproduced(rec, golden):
    """no switch in the environment; the rows carry every lsfa_conv_plan_override / lsfa_conv_order_override setting"""
    assert sum(len(res) for res in _assert_reproduced(rec, golden["groups"], {})) > 8000


def test_the_recorded_rows_cover_what_they_should(rec, golden):
    """the golden file is not regenerated: it holds failures, direct and ring launches, eight-wave tiles, K slices and the over-reported
    workspace of a direct launch (the RPN head: no workspace used, 2,451,456 bytes reported - kept until a change of its own shrinks it)"""
    conv = [g for g in golden["groups"] if g.get("kind") != "deconv"]
    rows = [a for g in conv for a in g["want"]]
    assert all(len(a) == 10 for a in rows) and golden["answer"] == rec.ANSWER
    assert sum(1 for a in rows if a[0] != 0) >= 8 and all(a[1:9] == [0] * 8 for a in rows if a[0] != 0)
    assert set((a[1], a[5]) for a in rows if a[0] == 0) == {(1, 4), (1, 8), (2, 4)}
    assert set(a[2] for a in rows if a[0] == 0) == {2, 4} and set(a[3] for a in rows if a[0] == 0 and a[1] == 1) == {2, 3, 4}
    assert max(a[6] for a in rows) >= 7 and any(a[7] == 1 for a in rows)
    rpn = dict(N=1, H=38, W=63, Cin=512, Cout=64, kh=1, pad_h=0, dil=1, pieces=3)
    assert [a for r, a in zip(rec.rows_of(conv[0]), conv[0]["want"]) if r == rpn] == [[0, 2, 2, 0, 0, 4, 1, 0, 3, 2451456]]
    assert sum(len(g["want"]) for g in golden["groups"] if g.get("kind") == "deconv") == 96


def test_plan_at_changes_the_hit_shape_and_nothing_else(rec, golden):
    """LSFA_CONV_PLAN_AT=chunks,cout,kernel,nt,st,slices in a fresh process: the recorded answers under each setting are reproduced; a hit
    changes exactly the rows of the shape with that K and channel count (whatever the API override says), a miss changes none"""
    base = rec.eval_in_child([rec.ENV_GROUP], {})[0]
    changed = []
    for e in golden["env"]:
        assert json.loads(json.dumps(rec.ENV_GROUP["factors"])) == e["factors"]
        got = _assert_reproduced(rec, [e], e["env"])[0]
        chunks, cout = [int(v) for v in e["env"]["LSFA_CONV_PLAN_AT"].split(",")[:2]]
        for r, a, a0 in zip(rec.rows_of(e), got, base):
            hit = r["kh"] * r["kh"] * (r["Cin"] // 32) == chunks and r["Cout"] == cout
            assert (a != a0) == hit, "LSFA_CONV_PLAN_AT=%s, row %s: %s, without it %s" % (e["env"]["LSFA_CONV_PLAN_AT"], r, a, a0)
        changed.append(sum(1 for a, a0 in zip(got, base) if a != a0))
    assert changed == [2, 2, 0]


def test_retired_lab_switches_change_nothing(rec, golden):
    """LSFA_CONV_PLAN_LAB (r5's candidate rules) and LSFA_CONV_PLAN_LONGK are gone: setting them leaves every recorded row as it is"""
    _assert_reproduced(rec, golden["groups"], {"LSFA_CONV_PLAN_LAB": "7", "LSFA_CONV_PLAN_LONGK": "1,4,2,1"})
