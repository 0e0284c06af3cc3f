"""``frcnn_coco_match`` (csrc/coco_match.hip) and ``coco_eval.evaluate(device='cuda')`` against the package's HOST path
(``coco_eval.match_host`` / ``accumulate_loops``: plain float64 loops) - never against device output.

The comparison is EXACT: overlaps bit for bit, matches and ignore bytes equal.  The overlap uses only min, max, +, -, * and /
on float64, contraction is off, and every one of these operations is correctly rounded on both sides; so no tolerance is
measured or allowed, and a mismatch is a bug.

The seeded scene (tests/coco_scenes.py, about 40 images and 6 categories) holds pairs with no ground truth and some
detections, pairs with ground truth and no detections, an image with neither, ground-truth counts from 0 to 12 and more with
about 15 % crowd, areas in all three ranges (some exactly 1024 and 9216, some annotations whose ``area`` is not w*h),
detections that are jittered copies of ground truth (integer-valued ones mixed in, and planted overlaps of exactly .5 and
.75), duplicates, detections inside crowd boxes, unmatched detections of every size, scores quantised to 0.01 and one pair
with 130 detections.  Its conditions are asserted from the host result before anything is compared."""
import functools

import numpy as np
import pytest

import coco_scenes as S
from faster_rcnn_pytorch_multimodal_amd import _hip
from faster_rcnn_pytorch_multimodal_amd.datasets import coco_eval as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
SENTINEL = {'float64': float('nan'), 'int32': -77, 'uint8': 0xAB}
OUTPUTS = ('ious', 'dt_match', 'dt_ignore', 'gt_ignore')
WIDE = dict(iou_thrs=np.linspace(.15, .95, 17))       # 4 x 17 = 68 walks: more than one wave of lanes


@functools.lru_cache(maxsize=None)
def host(name, wide=False):
    """The host path's result on a named scene, computed once and never changed."""
    if name.startswith('scene'):
        gt, res = S.seeded_scene(int(name[5:] or 0))
    elif name == 'sized':
        gt, res = S.sized_pairs()
    else:
        gt, res = S.hand_cases()[name]
    return C.evaluate(gt, res, C.Params(**WIDE) if wide else None)


def guarded(shape, dtype):
    """(buffer, view of ``shape`` between two GUARD-element bands), everything filled with the dtype's sentinel."""
    import torch
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL[dtype], dtype=getattr(torch, dtype), device=DEV)
    return buf, buf[GUARD:GUARD + numel].view(*shape)


def untouched(t):
    import torch
    fill = SENTINEL[str(t.dtype).split('.')[-1]]
    return bool(torch.isnan(t).all()) if fill != fill else bool((t == fill).all())


def subset(p, pairs, front=0, back=0):
    """The pairs ``pairs`` of a prepared dict, in that order, as the arrays ops.coco_match takes - with ``front`` / ``back``
    rows that belong to no pair before and after.  Also the rows of ``p`` that each new row came from."""
    def rows(off):
        r = [np.arange(int(off[q]), int(off[q + 1])) for q in pairs]
        return np.concatenate(r).astype(np.int64) if r else np.zeros(0, dtype=np.int64)

    def pad(a):
        filler = np.full((1,) + a.shape[1:], 3, dtype=a.dtype)
        return np.concatenate([np.repeat(filler, front, 0), a, np.repeat(filler, back, 0)])

    d_sel, g_sel, i_sel = rows(p['det_offsets']), rows(p['gt_offsets']), rows(p['iou_offsets'])
    pairs = np.asarray(pairs, dtype=np.int64)
    d_off = front + np.concatenate([[0], np.cumsum(np.diff(p['det_offsets'])[pairs])])
    g_off = front + np.concatenate([[0], np.cumsum(np.diff(p['gt_offsets'])[pairs])])
    new = {'det': pad(p['det'][d_sel]), 'gt': pad(p['gt'][g_sel]), 'gt_crowd': pad(p['gt_crowd'][g_sel]),
           'det_offsets': d_off.astype(np.int32), 'gt_offsets': g_off.astype(np.int32)}
    return new, d_sel, g_sel, i_sel


def launch(n, params, guard=False):
    """ops.coco_match on the arrays of ``subset``.  Returns the outputs as numpy arrays and, with ``guard``, the guarded
    buffers (outputs and workspace) for the band checks."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    A, T = params.area_rng.shape[0], params.iou_thrs.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    out = ws = None
    bufs = {}
    if guard:
        n_d, n_g = np.diff(n['det_offsets']), np.diff(n['gt_offsets'])
        shapes = {'ious': (int((n_d * n_g).sum()),), 'dt_match': (n['det'].shape[0], A, T),
                  'dt_ignore': (n['det'].shape[0], A, T), 'gt_ignore': (n['gt'].shape[0], A)}
        dtypes = {'ious': 'float64', 'dt_match': 'int32', 'dt_ignore': 'uint8', 'gt_ignore': 'uint8'}
        bufs = {k: guarded(shapes[k], dtypes[k]) for k in OUTPUTS}
        out = tuple(bufs[k][1] for k in OUTPUTS)
        need = _hip.load().frcnn_coco_match_ws_bytes(n['gt'].shape[0], int(n_g.max()) if n_g.size else 0, A, T)
        if need:
            bufs['ws'] = guarded((need,), 'uint8')
            ws = bufs['ws'][1]
    ious, i_off, dt_match, dt_ignore, gt_ignore = ops.coco_match(
        up(n['det']), n['det_offsets'], up(n['gt']), up(n['gt_crowd']), torch.from_numpy(n['gt_offsets']), params.iou_thrs,
        params.area_rng, out=out, ws=ws)
    torch.cuda.synchronize()
    got = {'ious': ious.cpu().numpy(), 'iou_offsets': i_off, 'dt_match': dt_match.cpu().numpy(),
           'dt_ignore': dt_ignore.cpu().numpy(), 'gt_ignore': gt_ignore.cpu().numpy()}
    return got, bufs


def assert_equal_to_host(got, h, d_sel, g_sel, i_sel, front=0):
    nd, ng = d_sel.shape[0], g_sel.shape[0]
    assert got['ious'].tobytes() == h['ious'][i_sel].tobytes()                   # bit for bit
    assert np.array_equal(got['dt_match'][front:front + nd], h['dt_match'][d_sel])
    assert np.array_equal(got['dt_ignore'][front:front + nd], h['dt_ignore'][d_sel].astype(np.uint8))
    assert np.array_equal(got['gt_ignore'][front:front + ng], h['gt_ignore'][g_sel].astype(np.uint8))


def all_pairs(h):
    return list(range(h['det_offsets'].shape[0] - 1))


@pytest.mark.parametrize('name', ['scene', 'scene1'])
def test_scene_meets_its_conditions_on_the_host(name):
    cond = S.scene_conditions(host(name))
    assert all(cond.values()), cond


@pytest.mark.parametrize('name', sorted(S.hand_cases()))
def test_hand_cases_on_the_device(hip, name):
    """One pair per launch; the hand values themselves are asserted on the host path (test_coco_eval_host.py)."""
    h = host(name)
    gt, res = S.hand_cases()[name]
    r = C.evaluate(gt, res, device='cuda')
    assert r['ious'].tobytes() == h['ious'].tobytes()
    for k in ('dt_match', 'dt_ignore', 'gt_ignore', 'precision', 'recall', 'scores', 'stats'):
        assert np.array_equal(r[k], h[k]), k
    want = {'identical': (0, 1.0), 'iou_077': (0, .6), 'crowd': (0, .5), 'area_range': (3, 1.0), 'max_dets': (6, .5),
            'threshold': (0, .1), 'tie': (1, 51 / 101), 'boundaries': (0, 34 / 101)}[name]
    assert abs(r['stats'][want[0]] - want[1]) <= 1e-12
    if name == 'crowd':
        assert (r['dt_match'][:2] == 1).all() and r['ious'].reshape(4, 2)[:2, 1].tolist() == [1.0, 1.0]
    if name == 'tie':
        assert r['dt_match'][0, 0, 0] == 1


@pytest.mark.parametrize('name', ['scene', 'scene1'])
def test_seeded_scene(hip, name):
    h = host(name)
    assert all(S.scene_conditions(h).values())
    pairs = all_pairs(h)
    got, _ = launch(subset(h, pairs)[0], h['params'])
    assert_equal_to_host(got, h, *subset(h, pairs)[1:])
    assert np.array_equal(got['iou_offsets'], h['iou_offsets'])


def test_sizes_where_the_layout_changes(hip):
    from faster_rcnn_pytorch_multimodal_amd import ops
    h = host('sized')
    n_d, n_g = np.diff(h['det_offsets']), np.diff(h['gt_offsets'])
    assert list(zip(n_d.tolist(), n_g.tolist())) == [(100, 90), (30, 65), (30, 64), (1, 1)]
    assert 100 * 90 > ops.COCO_LDS_IOUS and 30 * 64 > ops.COCO_LDS_IOUS and ops.COCO_MASK_GT == 64
    assert (h['dt_match'] >= 0).any(axis=(1, 2)).mean() > .5                     # the walks have something to decide
    for pairs in ([0, 1, 2, 3], [0], [1], [2], [3], [2, 3]):                     # with and without the workspace
        new, d_sel, g_sel, i_sel = subset(h, pairs)
        got, _ = launch(new, h['params'])
        assert_equal_to_host(got, h, d_sel, g_sel, i_sel)


def test_part_full_last_workgroup(hip):
    from faster_rcnn_pytorch_multimodal_amd import ops
    h = host('scene')
    count = (len(all_pairs(h)) - 1) // ops.COCO_PAIRS_PER_WG * ops.COCO_PAIRS_PER_WG + 1
    assert count % ops.COCO_PAIRS_PER_WG == 1 and count > 100
    pairs = all_pairs(h)[-count:]
    new, d_sel, g_sel, i_sel = subset(h, pairs)
    got, _ = launch(new, h['params'])
    assert_equal_to_host(got, h, d_sel, g_sel, i_sel)


def test_more_walks_than_lanes_and_pair_packing(hip):
    h = host('scene', wide=True)
    params = h['params']
    assert params.area_rng.shape[0] * params.iou_thrs.shape[0] == 68
    new, d_sel, g_sel, i_sel = subset(h, all_pairs(h))
    got, _ = launch(new, params)
    assert_equal_to_host(got, h, d_sel, g_sel, i_sel)
    perm = np.random.default_rng(5).permutation(len(all_pairs(h))).tolist()       # other neighbours in every workgroup
    new, d_sel, g_sel, i_sel = subset(h, perm)
    shuffled, _ = launch(new, params)
    assert_equal_to_host(shuffled, h, d_sel, g_sel, i_sel)
    assert shuffled['ious'].tobytes() == got['ious'][i_sel].tobytes()             # permuting the pairs permutes the outputs
    assert np.array_equal(shuffled['dt_match'], got['dt_match'][d_sel])


@pytest.mark.parametrize('name', ['scene', 'sized'])
def test_guard_bands(hip, name):
    h = host(name)
    front, back = 3, 2
    new, d_sel, g_sel, i_sel = subset(h, all_pairs(h), front, back)
    got, bufs = launch(new, h['params'], guard=True)
    assert ('ws' in bufs) == (name == 'sized')
    for k, (buf, view) in bufs.items():
        assert untouched(buf[:GUARD]) and untouched(buf[GUARD + view.numel():]), k
    nd, ng = d_sel.shape[0], g_sel.shape[0]
    assert_equal_to_host(got, h, d_sel, g_sel, i_sel, front)                     # so every element of a pair was written
    assert not np.isnan(got['ious']).any() and (got['dt_match'][front:front + nd] != SENTINEL['int32']).all()
    assert (got['dt_ignore'][front:front + nd] <= 1).all() and (got['gt_ignore'][front:front + ng] <= 1).all()
    for k, n in (('dt_match', nd), ('dt_ignore', nd), ('gt_ignore', ng)):         # rows of no pair: nothing written
        view = bufs[k][1]
        assert untouched(view[:front]) and untouched(view[front + n:]), k


def test_rejections(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert hip.frcnn_version() >= 125
    h = host('crowd')
    new = subset(h, [0])[0]
    params = h['params']
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    det, gt, crowd = up(new['det']), up(new['gt']), up(new['gt_crowd'])
    for d_off, g_off in (([0, 4, 2], [0, 2, 2]), ([0, 4], [2, 0]), ([0, 5], [0, 2]), ([-1, 4], [0, 2]), ([0, 4], [0, 1, 2])):
        with pytest.raises(_hip.HipError):
            ops.coco_match(det, np.array(d_off, dtype=np.int32), gt, crowd, np.array(g_off, dtype=np.int32), params.iou_thrs,
                           params.area_rng)
    thr, rng = up(params.iou_thrs), up(params.area_rng)
    d_off, g_off = up(new['det_offsets']), up(new['gt_offsets'])
    i_off = up(np.array([0, 8], dtype=np.int64))
    outs = [torch.empty(8, dtype=torch.float64, device=DEV), torch.empty((4, 4, 10), dtype=torch.int32, device=DEV),
            torch.empty((4, 4, 10), dtype=torch.uint8, device=DEV), torch.empty((2, 4), dtype=torch.uint8, device=DEV)]
    ptr = lambda t: t.data_ptr()

    def call(det_p=ptr(det), d_off_p=ptr(d_off), thr_p=ptr(thr), match_p=ptr(outs[1]), num_pairs=1, num_det=4, num_thr=10):
        return hip.frcnn_coco_match(det_p, d_off_p, num_det, ptr(gt), ptr(crowd), ptr(g_off), 2, ptr(i_off), 8, num_pairs,
                                    thr_p, num_thr, ptr(rng), 4, 2, ptr(outs[0]), match_p, ptr(outs[2]), ptr(outs[3]), None,
                                    0, None)

    for bad in (dict(det_p=None), dict(d_off_p=None), dict(thr_p=None), dict(match_p=None),     # a null required pointer
                dict(num_pairs=-1), dict(num_det=-1), dict(num_thr=0)):                         # a negative count
        with pytest.raises(_hip.HipError):
            _hip.check(call(**bad), "frcnn_coco_match")
    _hip.check(call(), "frcnn_coco_match")
    torch.cuda.synchronize()
    assert np.array_equal(outs[1].cpu().numpy(), h['dt_match'])
    # zero pairs: no launch, so rows that exist but belong to no pair keep what they held
    bufs = [guarded((0,), 'float64'), guarded((4, 4, 10), 'int32'), guarded((4, 4, 10), 'uint8'), guarded((2, 4), 'uint8')]
    zero = np.zeros(1, dtype=np.int32)
    ops.coco_match(det, zero, gt, crowd, zero, params.iou_thrs, params.area_rng, out=tuple(b[1] for b in bufs))
    _hip.check(call(num_pairs=0, det_p=None, d_off_p=None), "frcnn_coco_match")
    torch.cuda.synchronize()
    assert all(untouched(b[0]) for b in bufs)


@pytest.mark.parametrize('seed', [0, 1])
def test_end_to_end(hip, seed):
    gt, res = S.seeded_scene(seed)
    h = host('scene%d' % seed if seed else 'scene')
    r = C.evaluate(gt, res, device='cuda')
    for k in ('precision', 'recall', 'scores', 'stats'):
        assert np.array_equal(r[k], h[k]), k
    assert r['ious'].tobytes() == h['ious'].tobytes() and np.array_equal(r['dt_match'], h['dt_match'])
    assert C.summarize(r) == C.summarize(h) and 0 < r['stats'][0] < 1
