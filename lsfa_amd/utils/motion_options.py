"""The motion-estimation options the command lines share (lsfa_amd.demo, lsfa_amd.test) and the dict of estimator parameters they become:
hip.MotionEstimator's and hip.SegmentMotionEstimator's keywords, handed on by the demo's clips and by TestLoader.  Nothing of the GPU is imported."""


def add_arguments(ap, estimate_help):
    """--estimate-mv (with the driver's own help text) and the eight options that belong to it"""
    ap.add_argument('--estimate-mv', action='store_true', help=estimate_help)
    ap.add_argument('--search', type=int, default=16,
                    help='--estimate-mv: search range in pixels, 1..32, with --mv-levels the range on the top level (a parameter, not a tuned value)')
    ap.add_argument('--mv-lambda', type=int, default=4, help='--estimate-mv: cost per pixel of vector length (a parameter, not a tuned value)')
    ap.add_argument('--mv-levels', type=int, default=0, choices=(0, 1, 2),
                    help='--estimate-mv: extra pyramid levels; the reach is search * 2^L + refine * (2^L - 1) pixels (0: the full search alone)')
    ap.add_argument('--mv-refine', type=int, default=2, choices=(1, 2, 3), help='--mv-levels: refinement radius per level (a parameter, not a tuned value)')
    ap.add_argument('--scene-cut', type=int, nargs='?', const=50, default=None, metavar='PERCENT',
                    help='--estimate-mv: a frame more than PERCENT (1..100, default 50) of whose macroblocks the previous frame does not predict '
                         'becomes a key frame (DESIGN.md "Scene cuts"; a parameter, not a tuned value)')
    ap.add_argument('--cut-bias', type=int, default=4,
                    help='--scene-cut: grey levels per pixel a block\'s search residual may exceed its intra cost by, 0..255 (a parameter, not a tuned value)')
    ap.add_argument('--stale-key', type=int, nargs='?', const=50, default=None, metavar='PERCENT',
                    help='--estimate-mv: a frame more than PERCENT (1..100, default 50) of whose macroblocks the KEY frame, compensated with the '
                         'accumulated vectors, does not predict becomes a key frame: fades, dissolves, slow pans (DESIGN.md "Stale key frames"; a '
                         'parameter, not a tuned value).  Combines with --scene-cut')
    ap.add_argument('--stale-bias', type=int, default=4,
                    help='--stale-key: grey levels per pixel a block\'s residual against the key frame may exceed its intra cost by, 0..255 (a '
                         'parameter, not a tuned value)')


def estimate_of(ap, args):
    """The parsed options as the estimators' keywords - search, lam, levels, refine, and cut / stale where asked for - or None without
    --estimate-mv.  What is out of range ends in ap.error."""
    if args.scene_cut is not None and (not args.estimate_mv or not 1 <= args.scene_cut <= 100 or not 0 <= args.cut_bias <= 255):
        ap.error('--scene-cut PERCENT (1..100) needs --estimate-mv; --cut-bias is 0..255')
    if args.stale_key is not None and (not args.estimate_mv or not 1 <= args.stale_key <= 100 or not 0 <= args.stale_bias <= 255):
        ap.error('--stale-key PERCENT (1..100) needs --estimate-mv; --stale-bias is 0..255')
    if not args.estimate_mv:
        return None
    estimate = dict(search=args.search, lam=args.mv_lambda, levels=args.mv_levels, refine=args.mv_refine)
    if args.scene_cut is not None:
        estimate['cut'] = dict(bias=args.cut_bias, percent=args.scene_cut)
    if args.stale_key is not None:
        estimate['stale'] = dict(bias=args.stale_bias, percent=args.stale_key)
    return estimate


def ends_early(estimate):
    """Does this dict of estimator parameters (or None) let a segment end early, at its first flagged frame: is the pair rule (cut=) or the key rule (stale=) on?"""
    return estimate is not None and (estimate.get('cut') is not None or estimate.get('stale') is not None)
