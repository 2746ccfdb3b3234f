"""The drivers of the motion front end, without a device: the estimator chain behind lsfa_amd.demo's two clips on a stub estimator (what is
handed to it, in which order, what is kept, what is dumped), the option set lsfa_amd.demo and lsfa_amd.test share
(lsfa_amd/utils/motion_options.py), and the predicate "a segment may end early" TestLoader goes by."""
import ast
import os

import numpy as np
import pytest
import torch

W, H, FRAMES = 32, 16, 7
CHAIN = 'new key next next inputs next inputs key next inputs key next inputs'


class StubAccumulator(object):
    def motion_vectors(self):
        return torch.ones((H, W, 2), dtype=torch.int32)

    def residual(self, cur, key):
        assert tuple(cur.shape) == tuple(key.shape) == (H, W, 3) and cur.dtype == key.dtype == torch.uint8
        return torch.full((H, W, 3), 2, dtype=torch.int32)


def stub_estimator(log, built, cut=False):
    """stands in for hip.MotionEstimator: records new / key / next / is_cut / inputs and what it was built with"""

    class Stub(object):
        def __init__(self, width, height, device, **kw):
            log.append('new')
            built.append((width, height, device, kw))
            self.acc, self.fed = StubAccumulator(), []
            self.bgr_key, self.bgr_cur = torch.zeros((H, W, 3), dtype=torch.uint8), torch.ones((H, W, 3), dtype=torch.uint8)

        def _take(self, what, frame):
            log.append(what)
            self.fed.append(frame)

        def key_frame(self, bgr):
            self._take('key', bgr)

        def next_frame(self, bgr):
            self._take('next', bgr)

        def key_frame_yuv(self, y, uv=None, u=None, v=None):
            self._take('key', y)
            return self.bgr_key

        def next_frame_yuv(self, y, uv=None, u=None, v=None):
            self._take('next', y)
            return self.bgr_cur

        def is_cut(self):
            log.append('is_cut')
            return cut

        def network_inputs(self, bgr_cur, bgr_key, im_scale, pixel_means=(0.0, 0.0, 0.0), pixel_scale=1.0, rcnn_stride=16):
            log.append('inputs')
            return torch.full((1, 2, 1, 2), 3.0), torch.full((1, 3, 1, 2), 4.0)

    return Stub


@pytest.fixture(scope='module')
def sources(tmp_path_factory):
    """seven 32 x 16 random PNG frames in a directory and a seven-frame 32 x 16 NV12 file -> (directory, the frames as RGB, file, its bytes)"""
    from PIL import Image
    root = tmp_path_factory.mktemp('motion_drivers')
    rng = np.random.RandomState(7)
    frame_dir = root / 'frames'
    frame_dir.mkdir()
    rgb = rng.randint(0, 256, (FRAMES, H, W, 3)).astype(np.uint8)
    for i in range(FRAMES):
        Image.fromarray(rgb[i]).save(str(frame_dir / ('shot_%02d.png' % i)))
    raw = rng.randint(0, 256, (FRAMES, W * H * 3 // 2)).astype(np.uint8)
    yuv = root / 'clip.nv12'
    yuv.write_bytes(raw.tobytes())
    return str(frame_dir), rgb, str(yuv), raw


def small_cfg():
    from lsfa_amd.config.config import lsfa_test_config
    cfg = lsfa_test_config()
    cfg.SCALES = [(H, W)]
    return cfg


def build_clip(kind, sources, estimate, dump_mv=None):
    from lsfa_amd import demo
    frame_dir, _, yuv, _ = sources
    if kind == 'dir':
        return demo.FrameDirClip(frame_dir, None, small_cfg(), estimate, 'cpu', dump_mv)
    return demo.YuvFileClip(yuv, W, H, small_cfg(), 'nv12', 'bt601', estimate, 'cpu', dump_mv)


def kept(kind, clip):
    return sorted(clip._u8 if kind == 'dir' else clip._dev)


@pytest.mark.parametrize('kind', ['dir', 'yuv'])
@pytest.mark.parametrize('mode', [dict(), dict(stale=dict()), dict(cut=dict(percent=40))])
def test_one_chain_behind_both_clips(kind, mode, sources, tmp_path, monkeypatch):
    """mv_res(2, 0), (3, 0), a step back to (1, 0) and a new key frame (5, 4): the estimator is built once, with the clip's own size and
    keywords, restarts at the key frame for the step back and the new interval, is handed every frame of the chain once and in order,
    is asked is_cut() in front of every network_inputs only where a segment may end early; the clip keeps the frames of the interval
    under way and no others; the dump is named after the frame"""
    from lsfa_amd import hip
    log, built = [], []
    monkeypatch.setattr(hip, 'MotionEstimator', stub_estimator(log, built))
    estimate = dict(search=4, **mode)
    dump = str(tmp_path / 'dump')
    clip = build_clip(kind, sources, estimate, dump)
    assert (clip.num_frames, len(clip.names)) == (FRAMES, FRAMES) and os.path.isdir(dump) and not log
    for i, key_i in ((2, 0), (3, 0), (1, 0), (5, 4)):
        mv, res = clip.mv_res(i, key_i)
        assert tuple(mv.shape) == (1, 2, 1, 2) and tuple(res.shape) == (1, 3, 1, 2) and float(mv[0, 0, 0, 0]) == 3.0 and float(res[0, 0, 0, 0]) == 4.0
    want = CHAIN.replace('inputs', 'is_cut inputs') if mode else CHAIN
    assert ' '.join(log) == want
    assert built == [(W, H, 'cpu', estimate if kind == 'dir' else dict(estimate, matrix='bt601'))]
    assert kept(kind, clip) == [4, 5]
    # every frame of the chain reached the estimator as itself: 0 1 2 | 3 | 0 1 | 4 5
    fed, (_, rgb, _, raw) = clip._me.fed, sources
    assert len(fed) == 8
    for got, f in zip(fed, (0, 1, 2, 3, 0, 1, 4, 5)):
        if kind == 'dir':
            np.testing.assert_array_equal(got.numpy(), rgb[f][:, :, ::-1])
        else:
            np.testing.assert_array_equal(got.numpy(), raw[f][:W * H].reshape(H, W))
    stems = ['shot_%02d' % f for f in (1, 2, 3, 5)] if kind == 'dir' else ['%06d' % f for f in (1, 2, 3, 5)]
    assert sorted(os.listdir(dump)) == [s + '.npz' for s in stems]
    z = np.load(os.path.join(dump, stems[0] + '.npz'))
    assert z['mv'].shape == (H, W, 2) and (z['mv'] == -1).all() and z['res'].shape == (H, W, 3) and (z['res'] == 2).all()


@pytest.mark.parametrize('kind', ['dir', 'yuv'])
def test_a_flagged_frame_has_no_inputs(kind, sources, tmp_path, monkeypatch):
    """is_cut() true: mv_res returns None, and neither network_inputs nor a dump file follows"""
    from lsfa_amd import hip
    log, built = [], []
    monkeypatch.setattr(hip, 'MotionEstimator', stub_estimator(log, built, cut=True))
    dump = str(tmp_path / 'dump')
    clip = build_clip(kind, sources, dict(search=4, cut=dict()), dump)
    assert clip.mv_res(2, 0) is None and clip.mv_res(3, 0) is None
    assert ' '.join(log) == 'new key next next is_cut next is_cut'
    assert os.listdir(dump) == []


def test_what_the_clips_refuse(sources, tmp_path, monkeypatch):
    from lsfa_amd import demo, hip
    monkeypatch.setattr(hip, 'MotionEstimator', stub_estimator([], []))
    frame_dir, _, yuv, _ = sources
    with pytest.raises(ValueError, match='not both'):
        demo.FrameDirClip(frame_dir, str(tmp_path), small_cfg(), dict(search=4), 'cpu')
    for kind in ('dir', 'yuv'):
        with pytest.raises(ValueError, match='needs estimate'):
            build_clip(kind, sources, None, str(tmp_path / 'never'))
        assert not os.path.exists(str(tmp_path / 'never'))
        # without an estimate: zero motion, zero residual on the 16-pixel grid of the network's frame
        mv, res = build_clip(kind, sources, None).mv_res(1, 0)
        assert tuple(mv.shape) == (1, 2, 1, 2) and tuple(res.shape) == (1, 3, 1, 2) and not mv.any() and not res.any()
    with pytest.raises(ValueError, match='frame 4 has no motion vectors against key frame 4'):
        build_clip('yuv', sources, dict(search=4)).mv_res(4, 4)
    with pytest.raises(ValueError, match=r'holds %d bytes: not a whole number of 30 x 16 nv12 frames of 720 bytes' % (FRAMES * W * H * 3 // 2)):
        demo.YuvFileClip(yuv, 30, H, small_cfg())
    with pytest.raises(SystemExit):
        demo.parse_args(['--yuv', yuv, '--size', '30x16'])
    assert demo.parse_args(['--yuv', yuv, '--size', '32x16']).yuv_size == (W, H)


# ---- the option set ------------------------------------------------------------------------------------------------------------------
BASE = dict(search=16, lam=4, levels=0, refine=2)
OPTIONS = [
    (['--estimate-mv'], BASE),
    (['--estimate-mv', '--search', '8', '--mv-lambda', '0'], dict(BASE, search=8, lam=0)),
    (['--estimate-mv', '--scene-cut'], dict(BASE, cut=dict(bias=4, percent=50))),
    (['--estimate-mv', '--scene-cut', '35', '--cut-bias', '0'], dict(BASE, cut=dict(bias=0, percent=35))),
    (['--estimate-mv', '--stale-key', '30', '--stale-bias', '9'], dict(BASE, stale=dict(bias=9, percent=30))),
    (['--estimate-mv', '--stale-key'], dict(BASE, stale=dict(bias=4, percent=50))),
    (['--estimate-mv', '--scene-cut', '100', '--stale-key', '1', '--cut-bias', '255'],
     dict(BASE, cut=dict(bias=255, percent=100), stale=dict(bias=4, percent=1))),
    (['--estimate-mv', '--search', '8', '--mv-levels', '2', '--mv-refine', '3', '--scene-cut'],
     dict(search=8, lam=4, levels=2, refine=3, cut=dict(bias=4, percent=50))),
    ([], None),
    (['--search', '8'], None),
]
REFUSED = [['--stale-key'], ['--scene-cut'], ['--stale-key', '30', '--stale-bias', '9'],
           ['--estimate-mv', '--stale-key', '0'], ['--estimate-mv', '--stale-key', '101'], ['--estimate-mv', '--stale-key', '--stale-bias', '256'],
           ['--estimate-mv', '--stale-key', '--stale-bias', '-1'],
           ['--estimate-mv', '--scene-cut', '0'], ['--estimate-mv', '--scene-cut', '101'], ['--estimate-mv', '--scene-cut', '--cut-bias', '256'],
           ['--estimate-mv', '--scene-cut', '--cut-bias', '-1'],
           ['--estimate-mv', '--mv-levels', '3'], ['--estimate-mv', '--mv-refine', '0']]


@pytest.mark.parametrize('argv,want', OPTIONS)
def test_both_command_lines_build_the_same_estimator_dict(argv, want, tmp_path):
    from lsfa_amd import demo, test
    a, b = demo.parse_args(['--frames', str(tmp_path)] + argv), test.parse_args(argv)
    assert a.estimate == b.estimate == want
    assert want is None or list(a.estimate) == list(want)


@pytest.mark.parametrize('argv', REFUSED)
def test_both_command_lines_refuse(argv, tmp_path, capsys):
    from lsfa_amd import demo, test
    said = []
    for parse in (lambda: demo.parse_args(['--frames', str(tmp_path)] + argv), lambda: test.parse_args(argv)):
        with pytest.raises(SystemExit) as e:
            parse()
        assert e.value.code == 2
        said.append(capsys.readouterr().err.splitlines()[-1].split('error: ')[1])
    assert said[0] == said[1]


def test_the_defaults_and_help_texts_are_stated_once():
    """both parsers carry the nine options with equal defaults, metavars and help texts - but --estimate-mv's help, which is each driver's own"""
    import argparse
    from lsfa_amd import demo, test
    from lsfa_amd.utils import motion_options
    ap = argparse.ArgumentParser()
    motion_options.add_arguments(ap, 'HELP')
    mine = {a.dest: a for a in ap._actions if a.dest != 'help'}
    assert sorted(mine) == sorted(['estimate_mv', 'search', 'mv_lambda', 'mv_levels', 'mv_refine', 'scene_cut', 'cut_bias', 'stale_key', 'stale_bias'])
    assert mine['estimate_mv'].help == 'HELP'
    assert {d: a.default for d, a in mine.items()} == dict(estimate_mv=False, search=16, mv_lambda=4, mv_levels=0, mv_refine=2, scene_cut=None,
                                                           cut_bias=4, stale_key=None, stale_bias=4)
    assert (mine['scene_cut'].const, mine['stale_key'].const, mine['scene_cut'].metavar, mine['stale_key'].metavar) == (50, 50, 'PERCENT', 'PERCENT')
    for module in (demo, test):
        src = open(module.__file__).read()
        assert 'motion_options.add_arguments(' in src and not [o for o in ap._option_string_actions if "'%s'" % o in src]


def test_the_option_module_imports_nothing_of_the_gpu():
    from lsfa_amd.utils import motion_options
    tree = ast.parse(open(motion_options.__file__).read())
    imported = [n for n in ast.walk(tree) if isinstance(n, (ast.Import, ast.ImportFrom))]
    assert imported == [], [ast.dump(n) for n in imported]


# ---- "a segment may end early" --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('estimate,want', [(None, False), (dict(search=8), False), (dict(search=8, cut=None, stale=None), False),
                                           (dict(search=8, cut=dict()), True), (dict(stale=dict(percent=30)), True),
                                           (dict(search=8, cut=dict(bias=2), stale=dict()), True)])
def test_ends_early(estimate, want):
    from lsfa_amd.utils.motion_options import ends_early
    assert ends_early(estimate) is want


@pytest.mark.parametrize('modes', [(), ('cut',), ('stale',), ('cut', 'stale')])
def test_the_loader_goes_by_it(modes):
    from lsfa_amd.config.config import lsfa_test_config
    from lsfa_amd.core.loader import TestLoader
    from lsfa_amd.utils.motion_options import ends_early
    from lsfa_amd.utils.synthetic import synthetic_roidb

    class Stub(object):
        def segment(self, stack, im_scale, pixel_means, pixel_scale):
            n = int(stack.shape[1]) - 1
            return torch.zeros((n, 1, 2, 2, 3)), torch.zeros((n, 1, 3, 2, 3))

        def first_cuts(self, n=None):
            return [None]

    class Loader(TestLoader):
        def _segment_estimator(self, width, height):
            return Stub()

    estimate = dict(search=8, **{m: dict(percent=40) for m in modes})
    loader = Loader(synthetic_roidb(1, 6, 32, 48, 4), lsfa_test_config(key_frame_interval=4), device='cpu', estimate_mv=estimate)
    assert loader.cut is ends_early(estimate) is bool(modes)
    assert TestLoader(synthetic_roidb(1, 6, 32, 48, 4), lsfa_test_config(key_frame_interval=4), device='cpu').cut is False
