"""Recorder of the convolution launch plan: what lsfa_conv_plan_query, lsfa_conv_workspace_bytes and
lsfa_deconv4x4s2_crop_workspace_bytes answer for ~9000 descriptors, under every lab override.

    python tests/golden/make_conv_plans.py            # writes tests/golden/conv_plans.json from the library hip.lib() loads
    python tests/golden/make_conv_plans.py --eval     # groups (JSON) on stdin -> their answers, in this process's environment, on stdout

The plan is host arithmetic (no kernel runs, no GPU is needed): the pointers of a descriptor only have to be non-NULL and aligned.
conv_plans.json was recorded on the build of the commit BEFORE the launch code was folded into one plan function and is not
regenerated when that code changes: tests/test_conv_plan_cpu.py holds every later build to it.

A group of the file is a cross product: "factors" is a list of [field names, list of value tuples]; its rows are the products of one
tuple per factor, the last factor varying fastest; fields not named keep DEFAULTS (kw / pad_w follow kh / pad_h).  A row's answer is
[return code of the plan query, its 8 words (zeros when it failed), workspace bytes] for "conv" groups and [workspace bytes] for
"deconv" groups; "answers" holds the distinct ones and a group's "out" the index of each row's answer.
"""
import ctypes
import itertools
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "conv_plans.json")

FORCE = ["f_kernel", "f_nt", "f_st", "f_slices", "f_tile_order", "f_k_order"]
DEFAULTS = dict(N=1, H=0, W=0, Cin=0, Cout=0, kh=1, kw=0, stride=1, pad_h=0, pad_w=-1, dil=1, pieces=2, in_scale=0, x_nchw=0, y_nchw=0,
                lda=0, Ho=0, Wo=0, out_H=0, out_W=0, out_sy=0, out_sx=0, f_kernel=0, f_nt=0, f_st=0, f_slices=0, f_tile_order=-1, f_k_order=-1)
LAB_NAMES = ("LSFA_CONV_PLAN_LAB", "LSFA_CONV_PLAN_LONGK", "LSFA_CONV_PLAN_AT", "LSFA_CONV_TILE_ORDER", "LSFA_CONV_K_ORDER")
ANSWER = ["rc", "kind", "nt", "st", "sp", "wv", "slices", "af", "pieces", "workspace_bytes"]


def rows_of(group):
    """[{field: value}] of a group, in the order of its "out" """
    fields = [f for names, _ in group["factors"] for f in names]
    return [dict(zip(fields, [v for part in combo for v in part])) for combo in itertools.product(*[values for _, values in group["factors"]])]


class Evaluator(object):
    def __init__(self):
        sys.path.insert(0, ROOT)
        from lsfa_amd import hip      # ConvDesc is the binding's own mirror of struct lsfa_conv_desc
        self.lib, self.Desc = hip.lib(), hip.ConvDesc
        self.buf = ctypes.create_string_buffer(64)
        self.ptr = (ctypes.addressof(self.buf) + 15) & ~15          # never dereferenced by the queries
        self.force = None

    def set_force(self, f):
        if f != self.force:
            assert self.lib.lsfa_conv_plan_override(*[ctypes.c_int(v) for v in f[:4]]) == 0, f
            assert self.lib.lsfa_conv_order_override(ctypes.c_int(f[4]), ctypes.c_int(f[5])) == 0, f
            self.force = f

    def conv(self, c):
        d = self.Desc()
        d.x = d.wfrag = d.y = d.amax_in = self.ptr
        for k in ("N", "H", "W", "Cin", "Cout", "kh", "stride", "pad_h", "dil", "pieces", "x_nchw", "y_nchw", "lda", "Ho", "Wo", "out_H", "out_W",
                  "out_sy", "out_sx"):
            setattr(d, k, c[k])
        d.kw = c["kw"] if c["kw"] > 0 else c["kh"]
        d.pad_w = c["pad_w"] if c["pad_w"] >= 0 else c["pad_h"]
        if c["in_scale"]:
            d.in_scale = d.in_shift = self.ptr
        q = (ctypes.c_int * 8)()
        rc = self.lib.lsfa_conv_plan_query(ctypes.byref(d), q)
        return [int(rc)] + ([int(v) for v in q] if rc == 0 else [0] * 8) + [int(self.lib.lsfa_conv_workspace_bytes(ctypes.byref(d)))]

    def deconv(self, c):
        args = [c[k] for k in ("N", "H", "W", "Cin", "Cout", "out_H", "out_W", "pieces")]      # H, W: the input map; out_H, out_W: the cropped output
        return [int(self.lib.lsfa_deconv4x4s2_crop_workspace_bytes(*[ctypes.c_int(v) for v in args]))]

    def answer(self, groups):
        """-> per group, the list of its rows' answers"""
        out = []
        for g in groups:
            res = []
            for r in rows_of(g):
                c = dict(DEFAULTS)
                c.update(r)
                self.set_force([c[k] for k in FORCE])
                res.append(self.deconv(c) if g.get("kind") == "deconv" else self.conv(c))
            out.append(res)
        self.set_force([0, 0, 0, 0, -1, -1])
        return out


def each(*values):
    return [[v] for v in values]


MAPS = ["H", "W"], [(150, 250), (75, 125), (38, 63), (19, 32), (10, 16)]
# the shapes whose plan is recorded under every override
SHAPES = ["N", "H", "W", "Cin", "Cout", "kh", "pad_h", "dil", "pieces", "in_scale"], [
    (1, 38, 63, 2048, 1024, 3, 6, 6, 2, 0),      # feat_conv_3x3: 576 chunks of K
    (1, 38, 63, 512, 64, 1, 0, 1, 3, 0),         # the RPN head: direct kernel, exact cut
    (1, 150, 250, 64, 256, 1, 0, 1, 2, 0),       # res2 conv3: two chunks
    (6, 38, 63, 1024, 256, 1, 0, 1, 1, 0),       # res4 conv1, six images, bf16
    (1, 38, 63, 256, 1024, 1, 0, 1, 2, 0),       # res4 conv3: an expanding 1x1
    (1, 75, 125, 128, 128, 3, 1, 1, 2, 0),       # res3 conv2
    (9, 19, 32, 512, 2048, 1, 0, 1, 1, 0),       # res5 conv3, nine images
    (1, 38, 63, 512, 1920, 1, 0, 1, 2, 0),       # the R-FCN maps (16 chunks, 1920 channels)
    (6, 38, 63, 256, 1024, 1, 0, 1, 1, 1),       # in_scale on 128 x 128 tiles, bf16: the stage fix
    (1, 10, 16, 64, 64, 3, 1, 1, 3, 0),          # a small map: direct kernel
    (6, 38, 63, 256, 1024, 3, 1, 1, 2, 0),       # the small net's fuse convolution (72 chunks, 1024 channels)
]
# LSFA_CONV_PLAN_AT settings, each recorded in a child process over ENV_GROUP: the first two hit one shape each, the third none
AT_ENVS = ["72,1024,2,4,3,2", "16,1920,4,4,3,1", "24,1024,1,2,2,3"]
ENV_GROUP = {"what": "SHAPES with no override and under one API override", "factors": [[FORCE, [(0, 0, 0, 0, -1, -1), (1, 2, 2, 1, 0, 1)]], SHAPES]}


def groups():
    g = []
    g.append({"what": "the network's maps x channel counts x kernels x pieces",
              "factors": [[["N"], each(1, 6, 9)], MAPS, [["Cin"], each(32, 64, 256, 512, 1024, 2048)], [["Cout"], each(64, 128, 256, 512, 1024, 1920, 2048)],
                          [["kh", "pad_h", "dil"], [(1, 0, 1), (3, 1, 1), (3, 6, 6)]], [["pieces"], each(1, 2, 3)]]})
    g.append({"what": "the input's bn + ReLU at the cut (1x1, pieces 1 and 2)",
              "factors": [[["in_scale"], each(1)], [["N"], each(1, 6)], [MAPS[0], MAPS[1][:4]],
                          [["Cin", "Cout"], [(256, 64), (64, 256), (512, 128), (256, 1024), (1024, 256), (2048, 512), (1024, 2048)]], [["pieces"], each(1, 2)]]})
    g.append({"what": "NCHW input: the direct kernel's K-major form (2048 channels x 3 pieces: too many weights, an error)",
              "factors": [[["x_nchw", "H", "W"], [(1, 38, 63)]], [["N"], each(1, 9)], [["Cin", "lda"], [(512, 0), (512, 1024), (2048, 0)]], [["Cout"], each(64, 128)],
                          [["pieces"], each(1, 2, 3)]]})
    g.append({"what": "NCHW output",
              "factors": [[["y_nchw"], each(1)], [["N"], each(1, 6)], [MAPS[0], [(38, 63), (10, 16)]], [["Cin", "Cout"], [(512, 64), (1024, 1024), (2048, 256)]],
                          [["kh", "pad_h"], [(1, 0), (3, 1)]], [["pieces"], each(2, 3)]]})
    g.append({"what": "views: an output grid placed in a larger map, pad_h != pad_w, an input row pitch above Cin, a grid one past the convolution's",
              "factors": [[["N", "H", "W", "Cin", "Cout", "kh", "kw", "pad_h", "pad_w", "pieces", "lda", "Ho", "Wo", "out_H", "out_W", "out_sy", "out_sx"],
                           [(1, 19, 32, 512, 256, 2, 2, 1, 1, 2, 0, 19, 32, 38, 63, 2, 2), (6, 19, 32, 800, 128, 2, 2, 0, 1, 3, 832, 19, 32, 38, 63, 2, 2),
                            (1, 38, 63, 256, 64, 3, 3, 1, 1, 2, 416, 38, 63, 0, 0, 0, 0), (1, 38, 63, 256, 256, 3, 1, 1, 0, 2, 256, 38, 63, 0, 0, 0, 0),
                            (1, 75, 125, 128, 256, 1, 1, 0, 0, 1, 224, 75, 125, 75, 125, 1, 1), (6, 75, 125, 64, 128, 3, 3, 1, 1, 2, 64, 75, 125, 150, 250, 2, 2),
                            (1, 10, 16, 1056, 256, 2, 2, 1, 0, 3, 1056, 10, 16, 19, 32, 2, 2), (1, 10, 16, 64, 64, 3, 3, 1, 2, 3, 96, 10, 18, 10, 18, 1, 1)]]]})
    g.append({"what": "stride 2",
              "factors": [[["stride"], each(2)], [["N"], each(1, 6)], [MAPS[0], [(150, 250), (75, 125), (19, 32)]],
                          [["Cin", "Cout"], [(64, 128), (256, 512), (512, 64), (1024, 2048)]], [["kh", "pad_h"], [(1, 0), (3, 1), (5, 2)]], [["pieces"], each(1, 2, 3)]]})
    g.append({"what": "must fail: Cin no multiple of 32, in_scale on a 3x3 or with three pieces, Cout no multiple of 64, an empty output, four pieces",
              "factors": [[["N", "H", "W", "Cin", "Cout", "kh", "pad_h", "pieces", "in_scale"],
                           [(1, 38, 63, 48, 64, 1, 0, 2, 0), (1, 38, 63, 48, 64, 3, 1, 3, 0), (1, 38, 63, 256, 64, 3, 1, 2, 1), (6, 38, 63, 256, 256, 3, 0, 1, 1),
                            (1, 38, 63, 256, 64, 1, 0, 3, 1), (1, 38, 63, 64, 96, 1, 0, 2, 0), (1, 2, 2, 64, 64, 5, 0, 2, 0), (1, 38, 63, 64, 64, 1, 0, 4, 0)]]]})
    g.append({"what": "every lsfa_conv_plan_override setting on SHAPES",
              "factors": [SHAPES, [["f_kernel"], each(0, 1, 2, 4)], [["f_nt"], each(0, 2, 4)], [["f_st"], each(0, 2, 3, 4)], [["f_slices"], each(0, 1, 2, 5, 7)]]})
    g.append({"what": "every lsfa_conv_order_override setting on SHAPES",
              "factors": [SHAPES, [["f_tile_order"], each(-1, 0, 1)], [["f_k_order"], each(-1, 0, 1)]]})
    g.append({"what": "FlowNet's four transposed convolutions (H, W: input map; out_H, out_W: cropped output), lsfa_deconv4x4s2_crop_workspace_bytes",
              "kind": "deconv",
              "factors": [[["N"], each(1, 6)],
                          [["H", "W", "Cin", "Cout", "out_H", "out_W"], [(5, 8, 1024, 512, 10, 16), (10, 16, 1056, 256, 19, 32), (19, 32, 800, 128, 38, 63), (38, 63, 416, 64, 75, 125)]],
                          [["pieces"], each(2, 3)], [FORCE[:4], [(0, 0, 0, 0), (1, 2, 2, 1), (2, 4, 3, 2), (2, 2, 4, 5), (4, 4, 3, 1), (0, 0, 0, 7)]]]})
    return g


def eval_in_child(groups_, env):
    """answer `groups_` in a fresh process whose environment is os.environ without the convolution's lab switches, + env"""
    e = {k: v for k, v in os.environ.items() if k not in LAB_NAMES}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--eval"], input=json.dumps(groups_), capture_output=True, text=True, env=e)
    if r.returncode != 0:
        raise RuntimeError("make_conv_plans.py --eval failed:\n%s" % r.stderr)
    return json.loads(r.stdout)


def main():
    if "--eval" in sys.argv:
        json.dump(Evaluator().answer(json.load(sys.stdin)), sys.stdout, separators=(",", ":"))
        return
    index = {}      # distinct answer -> its number

    def recorded(group, res):
        return dict(group, out=[index.setdefault(tuple(a), len(index)) for a in res])
    gs = groups()
    rec = {"answer": ANSWER, "groups": [recorded(g, r) for g, r in zip(gs, eval_in_child(gs, {}))],
           "env": [dict(recorded(ENV_GROUP, eval_in_child([ENV_GROUP], {"LSFA_CONV_PLAN_AT": at})[0]), env={"LSFA_CONV_PLAN_AT": at}) for at in AT_ENVS]}
    rec["answers"] = [list(a) for a, _ in sorted(index.items(), key=lambda kv: kv[1])]
    dump = lambda v: json.dumps(v, separators=(",", ":"))
    wrap = lambda items, per: ",\n   ".join(",".join(items[i:i + per]) for i in range(0, len(items), per))

    def dump_group(g):
        head = ",\n   ".join('%s:%s' % (dump(k), dump(v)) for k, v in g.items() if k not in ("factors", "out"))
        return '  {%s,\n   "factors":[%s],\n   "out":[%s]}' % (head, wrap([dump(f) for f in g["factors"]], 1), wrap([str(i) for i in g["out"]], 60))
    with open(GOLDEN, "w") as f:
        f.write('{"answer":%s,\n "groups":[\n%s],\n "env":[\n%s],\n "answers":[\n   %s]}\n' % (
            dump(rec["answer"]), ",\n".join(dump_group(g) for g in rec["groups"]), ",\n".join(dump_group(g) for g in rec["env"]),
            wrap([dump(a) for a in rec["answers"]], 6)))
    print("%s: %d rows, %d distinct answers, %d bytes" % (GOLDEN, sum(len(g["out"]) for g in rec["groups"] + rec["env"]), len(rec["answers"]), os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
