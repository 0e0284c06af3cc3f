"""frcnn_uncertainty_columns (csrc/boxes.hip): a frame's detections followed by their uncertainty columns in one launch,
against the host statement it replaces in utils/filter_predictions.filter_device - nets/uncertainty.
stack_uncertainty_columns (one torch gather per class and box-variance kind) + torch.cat.

Valid rows are copies and must agree bit for bit.  Padding rows (det_roi == -1) keep their box columns and hold +0.0 in
every uncertainty column; the host statement computes ``v[0] * 0`` there, which is -0.0 or NaN when RoI 0 holds a negative
or non-finite value - no consumer reads those rows (they lie past det_count).
"""
import itertools

import pytest
import torch

from test_loss_stat_kernels import _bits_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 37
# what cfg.UC.EN_BBOX_ALEATORIC / EN_CLS_ALEATORIC / EN_{BBOX,CLS}_EPISTEMIC (switched together) can produce
GROUPS = dict(bbox_al=("a_bbox_var",), cls_al=("a_entropy", "a_mutual_info", "a_cls_var"),
              epi=("e_entropy", "e_mutual_info", "e_cls_var", "e_bbox_var"))
SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(sorted(GROUPS), n)]
assert len(SUBSETS) == 7


def _mods():
    from faster_rcnn_pytorch_multimodal_amd import ops
    from faster_rcnn_pytorch_multimodal_amd.nets import uncertainty as U
    return ops, U


def _sources(k, e, g):
    """Every source of UNCERTAINTY_ORDER with the shapes classify_test gives them; signs mixed, RoI 0 negative somewhere."""
    rnd = lambda *s: torch.randn(*s, generator=g)
    full = dict(a_entropy=rnd(R), a_mutual_info=rnd(R), a_cls_var=rnd(R, k), e_entropy=rnd(R), e_mutual_info=rnd(R),
                e_cls_var=rnd(R, k), a_bbox_var=rnd(R, k * e), e_bbox_var=rnd(R, k * e))
    full["a_entropy"][0] = -1.5
    full["e_bbox_var"][0] = -full["e_bbox_var"][0].abs() - 0.1
    full["a_bbox_var"][0, ::2] = -2.0
    return {n: v.to(DEV) for n, v in full.items()}


def _det_roi(kind, k, m, g):
    if kind == "all":
        roi = torch.randint(0, R, (k, m), generator=g)
    elif kind == "none":
        roi = torch.full((k, m), -1)
    else:
        roi = torch.randint(0, R, (k, m), generator=g)
        roi[torch.rand(k, m, generator=g) < 0.4] = -1
        flat = roi.view(-1)
        flat[0] = 0                                   # RoI 0 and RoI R-1 are valid rows; a padding row sits between valid ones
        flat[-1] = R - 1
        if flat.numel() > 2:
            flat[1] = -1
    return roi.to(torch.int32).to(DEV)


def _pick(full, subset, U):
    names = [n for grp in subset for n in GROUPS[grp]]
    return {n: full[n] for n in U.UNCERTAINTY_ORDER if n in names}


def _device_form(ops, U, dets, unc, det_roi, out=None):
    srcs = [(unc[n], n.endswith("bbox_var")) for n in U.UNCERTAINTY_ORDER if n in unc]
    return ops.uncertainty_columns(dets, det_roi, srcs, out=out)


def _check(got, dets, unc, det_roi, k, U):
    host = torch.cat((dets, U.stack_uncertainty_columns(unc, det_roi, k)), 2)
    d = dets.shape[2]
    valid = det_roi >= 0
    assert got.shape == host.shape
    assert _bits_equal(got[..., :d], dets)                                          # box columns: every row, as they are
    assert _bits_equal(got[valid], host[valid])
    pad = got[~valid][:, d:].contiguous()
    assert bool((pad.view(torch.int32) == 0).all())                                 # +0.0 bit patterns


@pytest.mark.parametrize("m", [1, 100, 300])
@pytest.mark.parametrize("e", [4, 7])
@pytest.mark.parametrize("k", [2, 4, 21, 81])
def test_against_the_host_statement(hip, k, e, m):
    ops, U = _mods()
    g = torch.Generator().manual_seed(1000 * k + 10 * m + e)
    full = _sources(k, e, g)
    dets = torch.randn(k, m, e + 1, generator=g).to(DEV)
    rois = {kind: _det_roi(kind, k, m, g) for kind in ("all", "none", "mixed")}
    assert int((rois["mixed"] == 0).sum()) > 0 and int((rois["mixed"] == R - 1).sum()) > 0
    for subset in SUBSETS:
        unc = _pick(full, subset, U)
        for kind, det_roi in rois.items():
            _check(_device_form(ops, U, dets, unc, det_roi), dets, unc, det_roi, k, U)
    unc = _pick(full, SUBSETS[-1], U)
    assert len(unc) == 8
    assert _bits_equal(U.append_uncertainty_columns(dets, unc, rois["mixed"]), _device_form(ops, U, dets, unc, rois["mixed"]))


@pytest.mark.parametrize("bad", [float("-inf"), float("inf"), float("nan"), -3.0])
def test_padding_is_plus_zero_whatever_roi_0_holds(hip, bad):
    ops, U = _mods()
    k, e, m = 4, 7, 100
    g = torch.Generator().manual_seed(5)
    full = _sources(k, e, g)
    for v in full.values():
        v[0] = bad
    dets = torch.randn(k, m, e + 1, generator=g).to(DEV)
    det_roi = _det_roi("mixed", k, m, g)
    unc = _pick(full, SUBSETS[-1], U)
    got = _device_form(ops, U, dets, unc, det_roi)
    host = torch.cat((dets, U.stack_uncertainty_columns(unc, det_roi, k)), 2)
    valid = det_roi >= 0
    pad = got[~valid][:, e + 1:].contiguous()
    assert pad.numel() > 0 and bool((pad.view(torch.int32) == 0).all())
    host_pad = host[~valid][:, e + 1:].contiguous()
    assert not bool((host_pad.view(torch.int32) == 0).all())                        # the host statement leaves -0.0 / NaN there
    not0 = valid & (det_roi != 0)
    assert _bits_equal(got[not0], host[not0])
    row0 = got[det_roi == 0][:, e + 1:]
    want0 = torch.full_like(row0, bad)
    assert row0.numel() > 0 and torch.equal(torch.isnan(row0), torch.isnan(want0))
    assert torch.equal(torch.nan_to_num(row0, nan=7.0), torch.nan_to_num(want0, nan=7.0))     # a copy of RoI 0's values


@pytest.mark.parametrize("k,e,m", [(2, 4, 1), (21, 7, 100), (81, 4, 300)])
def test_output_stays_inside_guard_bands(hip, k, e, m):
    from guarded_buffers import guarded, guards_intact
    ops, U = _mods()
    g = torch.Generator().manual_seed(k)
    unc = _pick(_sources(k, e, g), SUBSETS[-1], U)
    dets = torch.randn(k, m, e + 1, generator=g).to(DEV)
    det_roi = _det_roi("mixed", k, m, g)
    w = e + 1 + 2 * (2 + k) + 2 * e
    buf, view = guarded(k * m * w)
    out = _device_form(ops, U, dets, unc, det_roi, out=view.view(k, m, w))
    torch.cuda.synchronize()
    assert guards_intact(buf, k * m * w) and not bool(torch.isnan(out).any())      # nothing outside, every element written
    _check(out, dets, unc, det_roi, k, U)


def test_a_captured_call_is_one_kernel_node(hip):
    from faster_rcnn_pytorch_multimodal_amd.model.train_graph import graph_node_kinds
    ops, U = _mods()
    k, e, m = 21, 4, 100
    g = torch.Generator().manual_seed(2)
    unc = _pick(_sources(k, e, g), SUBSETS[-1], U)
    dets = torch.randn(k, m, e + 1, generator=g).to(DEV)
    det_roi = _det_roi("mixed", k, m, g)
    eager = _device_form(ops, U, dets, unc, det_roi)
    out = torch.empty_like(eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        _device_form(ops, U, dets, unc, det_roi, out=out)
    kinds, nodes, _ = graph_node_kinds(graph)
    assert kinds == {"kernel": 1} and nodes == 1, kinds
    graph.instantiate()
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(out, eager)


def test_rejections(hip):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    ops, U = _mods()
    z = lambda *s: torch.zeros(*s, device=DEV)
    roi = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    for call in (lambda: ops.uncertainty_columns(z(2, 5, 5), roi, []),
                 lambda: ops.uncertainty_columns(z(2, 5, 5), roi, [(z(9), False)] * 9),
                 lambda: ops.uncertainty_columns(z(2, 5, 5), roi.long(), [(z(9), False)]),
                 lambda: ops.uncertainty_columns(z(2, 5, 5), roi, [(z(9, 7), True)]),          # 7 columns for 2 classes
                 lambda: ops.uncertainty_columns(z(2, 5, 5), roi, [(z(9), False), (z(8), False)]),
                 lambda: ops.uncertainty_columns(z(2, 5, 5), roi, [(z(9), False)], out=z(2, 5, 7))):
        with pytest.raises(_hip.HipError, match="uncertainty_columns"):
            call()
