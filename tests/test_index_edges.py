"""The index-producing kernels - frcnn_nms (nms.hip), frcnn_sort_topk_desc (topk.hip), frcnn_filter_per_class[_lidar]
(class_filter.hip, class_filter.h) - over the whole range of sizes the library admits, on DESIGNED inputs and inside guarded
buffers.  Every comparison is equality.

A. frcnn_nms on rank-ordered boxes whose survivors are known by construction (``designed_boxes``): how many boxes of every
   64-box chunk survive and how many chunks back the box that removes a follower lies are chosen, not drawn, so every path of
   nms_scan_kernel (0 / 1-4 / 5-8 / > SCAN_DENSE survivors; carry words, the pending ring, the helper waves; the fourth word
   slot from 12 289 boxes on) is entered on purpose.  The input's own conditions are asserted on the host (the tests without
   the ``gpu`` mark); the device result is compared with the constructed answer AND with the CPU rule (O.nms).
B. The per-class filter at 960 | 961 (the LDS kernel's last size and the general kernel's first), 1024, 4096 | 4097 (bitonic
   sort of 4096 / 8192 keys) and 8192 RoIs (the limit; the second word slot of wave_nms_scan), same construction per class.
C. All three entry points through the C ABI with every output a view between byte bands, a workspace of exactly *_ws_bytes
   bytes between bands and full of 0xFF, and a second run on the workspace another input left behind.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import frcnn_oracle as O
from guarded_buffers import OUT_BYTE, POISON_BYTE, ByteGuarded, guarded_like

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _ops():
    from faster_rcnn_pytorch_multimodal_amd import ops
    return ops


# ================================================================================================
# The generator
# ================================================================================================
# survivors per 64-rank chunk.  The schedule is walked forwards and backwards in turn: read forwards only, its consecutive
# pairs never put a 1-4 chunk after a 1-4 chunk, nor a 5-8 chunk after an empty one or before a 1-4 one; the backward walk
# and the two turning points supply exactly those three (test_schedule_offers_every_transition).
SCHEDULE = (1, 0, 4, 5, 8, 9, 64, 0, 0, 3, 33, 2, 9, 8, 0, 16)
FAR = -1                                    # "as far as possible": the leader lies in one of the first 64 chunks
REACH = (0, 1, 2, 3, 4, 64, FAR)            # chunks between a follower and the box that removes it
BOX = 10.0                                  # every leader is BOX x BOX


def survivors_in_chunk(c):
    cycle, k = divmod(c, len(SCHEDULE))
    return SCHEDULE[k] if cycle % 2 == 0 else SCHEDULE[len(SCHEDULE) - 1 - k]


def survivor_class(count):
    """The scan's four regimes: nothing to fetch, one pending batch, a second waited-for batch, the helper waves."""
    return 0 if count == 0 else 1 if count <= 4 else 2 if count <= 8 else 3


class Design:
    """boxes (n, 4) float32 in rank order; kind[r]: 'A' leader on its own cell, 'B' / 'C' the second and third member of a
    three-chain, 'f' follower, 'e' follower at IoU == threshold exactly; parent[r]: the rank that removes r ('B', 'f', 'e'),
    for 'C' the rank of its B; survivors: ranks of 'A' and 'C' (ascending) - with the rule `>` at the threshold, 'e' too."""

    def __init__(self, boxes, kind, parent):
        self.boxes, self.kind, self.parent = boxes, kind, parent
        self.n = len(kind)
        self.survivors = np.flatnonzero((kind == "A") | (kind == "C"))
        self.survivors_strict = np.flatnonzero((kind == "A") | (kind == "C") | (kind == "e"))
        self.per_chunk = np.bincount(self.survivors // 64, minlength=(self.n + 63) // 64)
        removed = np.flatnonzero((kind == "B") | (kind == "f") | (kind == "e"))
        self.follower_dist = removed // 64 - parent[removed] // 64
        self.follower_rank = removed
        third = np.flatnonzero(kind == "C")
        self.chain_dist = third // 64 - parent[third] // 64


@functools.lru_cache(maxsize=None)
def designed_boxes(n, seed=0, step=1, eq_h=7.0, cols=64, tail_follower=False):
    """Leaders sit on pairwise disjoint grid cells (pitch 24 x 16); a follower is its leader moved by one pixel in y (IoU
    9/11), an 'e' follower is the leader's box cut to ``eq_h`` rows (IoU eq_h/10: 0.7 or 0.6 in fp32 exactly, at most one
    per leader); a chain is A at x, B at x + step, C at x + 2 * step: step 1 for threshold 0.7 (IoU 9/11, 9/11, 8/12), step
    2 for 0.6 (8/12, 8/12, 6/14), so C survives only because B was removed.  No other pair of a cell reaches either
    threshold with a SURVIVOR: f-C 72/128 (step 1), e-f 60/110, e-B 63/107.  ``tail_follower``: a last chunk of one box
    holds a follower of a leader in the first 64 chunks instead of a leader."""
    rng = np.random.default_rng(seed)
    nchunks = (n + 63) // 64
    boxes = np.zeros((n, 4), np.float32)
    kind = np.full(n, "?", dtype="U1")
    parent = np.full(n, -1, np.int64)
    leaders_in = [[] for _ in range(nchunks)]           # 'A' ranks per chunk
    open_b = [[] for _ in range(nchunks)]               # (rank of B, rank of A) still without a C, per chunk of B
    has_b, has_e = set(), set()
    cells = 0

    def reach_chunk(c, lists, far=False):
        d = FAR if far else REACH[rng.integers(len(REACH))]
        t = int(rng.integers(0, min(c, 63) + 1)) if d == FAR else max(c - d, 0)
        while t >= 0 and not lists[t]:
            t -= 1                                       # the nearest earlier chunk that has one
        return t

    for c in range(nchunks):
        lo = c * 64
        live = min(64, n - lo)
        want = min(survivors_in_chunk(c), live)
        lone_tail = c == nchunks - 1 and live == 1 and c > 0
        if lone_tail:
            want = 0 if tail_follower else 1
        pos = np.sort(rng.choice(live, want, replace=False)) if want else np.zeros(0, np.int64)
        if c == 0:
            pos[0] = 0                                   # rank 0 has nobody to follow
        surv = set(int(lo + p) for p in pos)
        for r in range(lo, lo + live):
            if r in surv:
                t = reach_chunk(c, open_b) if rng.random() < 0.25 else -1
                if t >= 0:
                    b, a = open_b[t].pop(int(rng.integers(len(open_b[t]))))
                    x, y = boxes[a, 0] + 2 * step, boxes[a, 1]
                    kind[r], parent[r] = "C", b
                else:
                    x, y = (cells % cols) * 24.0, (cells // cols) * 16.0
                    cells += 1
                    kind[r] = "A"
                    leaders_in[c].append(r)
                boxes[r] = (x, y, x + BOX, y + BOX)
                continue
            t = reach_chunk(c, leaders_in, far=lone_tail)
            a = leaders_in[t][int(rng.integers(len(leaders_in[t])))]
            x, y = boxes[a, 0], boxes[a, 1]
            u = rng.random()
            if u < 0.25 and a not in has_b:
                has_b.add(a)
                open_b[c].append((r, a))
                kind[r], boxes[r] = "B", (x + step, y, x + step + BOX, y + BOX)
            elif u < 0.32 and a not in has_e:
                has_e.add(a)
                kind[r], boxes[r] = "e", (x, y, x + BOX, y + eq_h)
            else:
                kind[r], boxes[r] = "f", (x, y + 1, x + BOX, y + 1 + BOX)
            parent[r] = a
    return Design(boxes, kind, parent)


def check_design(d, fourth_slot_pairs=True):
    """The conditions the input was built for, as far as its size admits them."""
    nchunks = len(d.per_chunk)
    full = d.per_chunk[:nchunks - 1] if d.n % 64 else d.per_chunk       # a partly filled last chunk may hold fewer
    assert set(SCHEDULE) <= set(full.tolist()) and {0, 1, 4, 5, 8, 9, 64} <= set(full.tolist())
    if nchunks > 2 * len(SCHEDULE):
        cls = [survivor_class(v) for v in d.per_chunk]
        assert {(a, b) for a, b in zip(cls, cls[1:])} == {(a, b) for a in range(4) for b in range(4)}
    dist = set(d.follower_dist.tolist())
    assert {0, 1, 2, 3, 4} <= dist and {0, 1, 2, 3, 4} <= set(d.chain_dist.tolist())
    if nchunks > 64:
        assert max(dist) >= 64 and int(d.chain_dist.max()) >= 64
    assert (d.kind == "e").sum() >= 1 and (d.kind == "C").sum() >= nchunks // 4
    if nchunks > 192 and fourth_slot_pairs:             # the fourth word slot: removed by, and surviving next to, rows far back
        assert max(dist) >= 192
        late = d.follower_rank >= 192 * 64
        assert (d.parent[d.follower_rank[late]] < 64 * 64).any() and (d.survivors >= 192 * 64).any()


NMS_SIZES = [(12288, False), (12289, False), (12289, True), (16321, False), (16384, False)]
NMS_IDS = ["12288", "12289-leader", "12289-follower", "16321", "16384"]


@functools.lru_cache(maxsize=None)
def _oracle_nms(key, live, at_equal, thresh=0.7):
    """O.nms on the first ``live`` boxes of designed_boxes(*key) under one rule at IoU == threshold (read-only)."""
    d = designed_boxes(*key)
    old = O.NMS_SUPPRESS_AT_EQUAL
    O.NMS_SUPPRESS_AT_EQUAL = at_equal
    try:
        b = torch.from_numpy(d.boxes[:live])
        return O.nms(b, torch.arange(live, 0, -1, dtype=torch.float32), thresh).numpy()
    finally:
        O.NMS_SUPPRESS_AT_EQUAL = old


def test_schedule_offers_every_transition():
    counts = [survivors_in_chunk(c) for c in range(4 * len(SCHEDULE))]
    assert counts[:16] == list(SCHEDULE) and counts[16:32] == list(SCHEDULE)[::-1] and counts[32:48] == list(SCHEDULE)
    forward = {(survivor_class(a), survivor_class(b)) for a, b in zip(SCHEDULE, SCHEDULE[1:] + SCHEDULE[:1])}
    assert {(0, 2), (1, 1), (2, 1)} == {(a, b) for a in range(4) for b in range(4)} - forward       # why it turns round
    cls = [survivor_class(v) for v in counts]
    assert {(a, b) for a, b in zip(cls, cls[1:])} == {(a, b) for a in range(4) for b in range(4)}


@pytest.mark.parametrize("n,tail_follower", NMS_SIZES, ids=NMS_IDS)
def test_designed_nms_inputs_meet_their_conditions(n, tail_follower):
    """Host only: the schedule, distance and fourth-slot conditions, and the CPU rule agrees with the construction under both
    readings of IoU == threshold.  12 289 boxes put ONE box into chunk 192: it is a leader in one input and a follower of a
    leader 129 or more chunks back in the other, and the two together meet the fourth-slot condition."""
    key = (n, n, 1, 7.0, 64, tail_follower)
    d = designed_boxes(*key)
    check_design(d, fourth_slot_pairs=n != 12289)
    assert (d.boxes[:, 2] > d.boxes[:, 0]).all() and (d.per_chunk[0] == 1) and d.kind[0] == "A"
    if n == 12289:
        assert d.kind[-1] in ("fBe" if tail_follower else "A")
        if tail_follower:
            assert d.parent[-1] < 64 * 64 and d.follower_dist.max() >= 129
    if n > 12289:
        dense = np.flatnonzero(d.per_chunk > 8)
        assert dense.max() >= 192                      # a chunk of the fourth slot goes through the helper waves
    assert np.array_equal(_oracle_nms(key, n, True), d.survivors)
    assert np.array_equal(_oracle_nms(key, n, False), d.survivors_strict)
    assert len(d.survivors_strict) > len(d.survivors)


# ================================================================================================
# A. frcnn_nms
# ================================================================================================
def _nms_raw(hip, boxes_dev, n_max, thresh, max_keep, n_dev=None):
    """frcnn_nms on pattern-filled outputs and a 0xFF workspace -> (rc, keep_idx, keep_mask, keep_count) on the host."""
    ops = _ops()
    cap = min(max_keep, n_max) if n_max <= 16384 else max_keep
    keep_idx = torch.full((cap,), -7, dtype=torch.int64, device=DEV)
    keep_mask = torch.full((n_max,), 0xAB, dtype=torch.uint8, device=DEV)
    keep_count = torch.full((1,), -99, dtype=torch.int32, device=DEV)
    ws_bytes = hip.frcnn_nms_ws_bytes(min(n_max, 16384))
    ws = torch.full((ws_bytes,), POISON_BYTE, dtype=torch.uint8, device=DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    rc = hip.frcnn_nms(boxes_dev.data_ptr(), None if nd is None else nd.data_ptr(), n_max, float(thresh), max_keep,
                       keep_idx.data_ptr(), keep_mask.data_ptr(), keep_count.data_ptr(), ws.data_ptr(), ws_bytes, ops._stream())
    torch.cuda.synchronize()
    return rc, keep_idx.cpu().numpy(), keep_mask.cpu().numpy(), int(keep_count.item())


def _expect_nms(survivors, n_max, max_keep):
    kept = survivors[:max_keep]
    idx = np.zeros(min(max_keep, n_max), np.int64)
    idx[:len(kept)] = kept
    mask = np.zeros(n_max, np.uint8)
    mask[kept] = 1
    return idx, mask, len(kept)


NMS_CASES = ["full", "cut_dense", "cut_boundary", "live_part", "live_zero", "live_over", "strict"]


@gpu
@pytest.mark.parametrize("case", NMS_CASES)
@pytest.mark.parametrize("n,tail_follower", NMS_SIZES, ids=NMS_IDS)
def test_nms_designed_structures(hip, n, tail_follower, case):
    """full: every survivor + keep_mask.  cut_dense: max_keep ends inside the last chunk with more than SCAN_DENSE survivors
    (a chunk of the fourth slot from 16 321 boxes on).  cut_boundary: max_keep is the survivor count of the chunks before
    the last chunk that has any, so the scan stops exactly between two chunks.  live_*: the live count read on the device -
    a prefix that ends one box into chunk 192 (sizes above 12 289; half the boxes plus one otherwise), zero, more than n_max
    (clamped).  strict: the rule `>` at IoU == threshold, under which the 'e' followers survive.  keep_idx is zero from the
    count on, keep_mask is one for the kept boxes and zero elsewhere, in every case."""
    key = (n, n, 1, 7.0, 64, tail_follower)
    d = designed_boxes(*key)
    boxes_dev = torch.from_numpy(d.boxes).to(DEV)
    live, max_keep, at_equal, n_dev = n, n, True, None
    cum = np.concatenate(([0], np.cumsum(d.per_chunk)))
    if case == "cut_dense":
        c = int(np.flatnonzero(d.per_chunk > 8).max())
        assert c >= 192 or n <= 12289
        max_keep = int(cum[c] + d.per_chunk[c] // 2)
    elif case == "cut_boundary":
        c = int(np.flatnonzero(d.per_chunk > 0).max())
        assert c >= 192 or n <= 12289
        max_keep = int(cum[c])
    elif case == "live_part":
        live = n_dev = 12289 if n > 12289 else n // 2 + 1
    elif case == "live_zero":
        live = n_dev = 0
    elif case == "live_over":
        n_dev = n + 5000
    elif case == "strict":
        at_equal = False
    want = (d.survivors if at_equal else d.survivors_strict)
    want = want[want < live]
    if live:
        assert np.array_equal(_oracle_nms(key, live, at_equal), want)
    old = _ops().set_nms_suppress_at_equal(at_equal)
    try:
        rc, idx, mask, count = _nms_raw(hip, boxes_dev, n, 0.7, max_keep, n_dev)
    finally:
        _ops().set_nms_suppress_at_equal(old)
    assert rc == 0, hip.frcnn_last_error()
    ref_idx, ref_mask, ref_count = _expect_nms(want, n, max_keep)
    if case.startswith("cut"):
        assert 0 < ref_count == max_keep < len(want)
    assert count == ref_count
    np.testing.assert_array_equal(idx, ref_idx)
    np.testing.assert_array_equal(mask, ref_mask)


@gpu
def test_nms_refuses_more_than_16384_boxes(hip):
    """n_max = 16 385: the library's error, and nothing is launched - the outputs keep their pattern."""
    boxes_dev = torch.zeros((16385, 4), dtype=torch.float32, device=DEV)
    rc, idx, mask, count = _nms_raw(hip, boxes_dev, 16385, 0.7, 16385)
    assert rc != 0 and b"16385 > 16384" in hip.frcnn_last_error()
    assert count == -99 and (idx == -7).all() and (mask == 0xAB).all()
    with pytest.raises(_ops()._hip.HipError, match="16385 > 16384"):
        _ops().nms_sorted(boxes_dev, 0.7)


# ================================================================================================
# B. the per-class filter
# ================================================================================================
# Which kernel a size reaches under variant 0 (class_filter.hip launch_filter): filter_class_small_kernel needs
# num_rois <= 1024 AND filter_small_lds(r) = r * (40 + 8 * ceil(r / 64)) <= 150 * 1024 = 153 600 bytes:
#    960: 960 * (40 + 8 * 15) = 153 600  -> the LDS kernel, its last size (variant 1 forces the general kernel)
#    961: 961 * (40 + 8 * 16) = 161 448  -> the general kernel, its first size in the automatic choice
#   1024: 1024 * (40 + 8 * 16) = 172 032 -> the general kernel
#   4096, 4097, 8192: above 1024         -> the general kernel: bitonic sort of 4096 (r = 4096) and 8192 (4097, 8192) keys;
#         at 8192 the class keeps 7022 boxes above the threshold: 110 chunks, the second word slot of wave_nms_scan
FILTER_SIZES = [(960, 0), (960, 1), (961, 0), (1024, 0), (4096, 0), (4097, 0), (8192, 0)]
FILTER_K = 3
FILTER_THRESH = 0.05
FILTER_INFO = np.array([0, 1000, 0, 600, 0, 0, 1.0], np.float32)
RUNS = (192, 1, 1, 3, 97, 1, 40, 64, 5, 33)         # lengths of the runs of equal scores, in ranks


def filter_small_lds(r):
    return r * (40 + 8 * ((r + 63) // 64))


def test_filter_sizes_reach_the_kernels_the_comment_names():
    assert filter_small_lds(960) == 150 * 1024 and filter_small_lds(961) > 150 * 1024 and filter_small_lds(1024) > 150 * 1024


def _as_rows(boxes, e, rng):
    """(m, 4) corner boxes as rows of the filter's input: the box itself, or a 7-DoF LiDAR box whose yaw-less BEV rectangle
    xc -+ l/2, yc -+ w/2 is that box (exact: integer and half-integer coordinates)."""
    if e == 4:
        return boxes
    m = len(boxes)
    out = np.zeros((m, 7), np.float32)
    out[:, 0], out[:, 1] = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    out[:, 3], out[:, 4] = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    out[:, 2], out[:, 5], out[:, 6] = rng.random(m), 1.0 + rng.random(m), rng.random(m) * 3.0 - 1.5
    return out


@functools.lru_cache(maxsize=None)
def _filter_case(r, e):
    """prob (r, K), pred (r, K * e) and per class (design, roi_of_rank).  Six in seven RoIs of a class score above the
    threshold, in runs of equal scores (RUNS); the rest sit AT the threshold or below it and carry boxes that leave the
    frame.  Read-only."""
    rng = np.random.default_rng(7000 + r + e)
    k = FILTER_K
    prob = np.zeros((r, k), np.float32)
    pred = np.zeros((r, k * e), np.float32)
    junk = np.concatenate((rng.uniform(-50, 900, (r, 2)), rng.uniform(50, 1100, (r, 2))), 1).astype(np.float32)
    prob[:, 0] = rng.random(r).astype(np.float32)
    pred[:, :e] = _as_rows(junk, e, rng)
    designs = [None]
    n_sel = r - r // 7
    run_of_rank = np.repeat(np.arange(n_sel), np.resize(RUNS, n_sel))[:n_sel]
    nruns = int(run_of_rank.max()) + 1
    score_of_rank = np.linspace(0.99, 0.06, nruns).astype(np.float32)[run_of_rank]
    assert len(np.unique(score_of_rank)) == nruns and score_of_rank.min() > FILTER_THRESH
    for j in range(1, k):
        d = designed_boxes(n_sel, 100 * j + e, 2, 6.0, 40, False)
        perm = rng.permutation(r)
        roi_of_rank = perm[:n_sel].copy()
        for run in range(nruns):                        # equal scores rank by RoI index
            m = run_of_rank == run
            roi_of_rank[m] = np.sort(roi_of_rank[m])
        rest = perm[n_sel:]
        prob[roi_of_rank, j] = score_of_rank
        prob[rest, j] = np.where(rng.random(len(rest)) < 0.5, np.float32(FILTER_THRESH),
                                 rng.random(len(rest)) * FILTER_THRESH).astype(np.float32)
        pred[:, j * e:(j + 1) * e] = _as_rows(junk[rng.permutation(r)], e, rng)
        pred[roi_of_rank, j * e:(j + 1) * e] = _as_rows(d.boxes, e, rng)
        designs.append((d, roi_of_rank))
    return torch.from_numpy(prob), torch.from_numpy(pred), designs


@functools.lru_cache(maxsize=None)
def _filter_oracle(r, e, live):
    """Per class: the CPU rule's rows on the first ``live`` RoIs, before the max_dets cut, in (score desc, RoI asc) order;
    and the clamped boxes of all r RoIs (the device clamps every row it is given).  Read-only."""
    prob, pred, _ = _filter_case(r, e)
    rois = torch.zeros(r, 5)
    if e == 4:
        _, rows, _ = O.filter_and_draw_prep(rois[:live], prob[:live], pred[:live], FILTER_INFO, FILTER_K, FILTER_THRESH)
        clamped = O.filter_and_draw_prep(rois[:1], prob[:1], pred, FILTER_INFO, FILTER_K, 2.0)[2]
    else:
        _, rows = O.filter_and_draw_prep_lidar(rois[:live], prob[:live], pred[:live], FILTER_K, FILTER_THRESH)
        clamped = pred
    return rows, clamped


def _cut_rows(rows, max_dets):
    want = O.max_dets_cut(rows, max_dets)
    return want[np.lexsort((np.arange(len(want)), -want[:, -1]))] if len(want) else want


@pytest.mark.parametrize("e", [4, 7])
@pytest.mark.parametrize("r", [960, 8192])
def test_designed_filter_inputs_meet_their_conditions(r, e):
    """Host only: per class the CPU rule keeps exactly the constructed survivors; the runs of equal scores cross the
    max_dets = 1 and = 100 cuts; RoIs sit at the threshold exactly; at 8192 RoIs the class fills the scan's second slot."""
    prob, pred, designs = _filter_case(r, e)
    rows, clamped = _filter_oracle(r, e, r)
    for j in range(1, FILTER_K):
        d, roi_of_rank = designs[j]
        assert {0, 1, 4, 5, 8, 9, 64} <= set(d.per_chunk.tolist()) and {0, 1, 2, 3, 4} <= set(d.follower_dist.tolist())
        kept_rois = roi_of_rank[d.survivors]
        np.testing.assert_array_equal(rows[j][:, :e], clamped[kept_rois, j * e:(j + 1) * e].numpy())
        np.testing.assert_array_equal(rows[j][:, e], prob[kept_rois, j].numpy())
        assert len(_cut_rows(rows[j], 1)) > 1 and len(rows[j]) > len(_cut_rows(rows[j], 100)) > 100
        assert int((prob[:, j] == np.float32(FILTER_THRESH)).sum()) > r // 40
        if r == 8192:
            assert d.n > 4096 + 64 and (d.survivors >= 4096).any() and (d.follower_rank >= 4096).any()
    if e == 4:
        assert not torch.equal(clamped, pred)


def _run_filter(r, e, max_dets, max_out, live, want_rois):
    ops = _ops()
    prob, pred, _ = _filter_case(r, e)
    prob_dev, pred_dev = prob.to(DEV), pred.clone().to(DEV)
    count_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
    if e == 4:
        out = ops.filter_per_class(pred_dev, prob_dev, 1000.0, 600.0, 1.0, FILTER_THRESH, O.TEST_NMS_THRESH, max_dets,
                                   max_out, roi_count=count_dev, want_rois=want_rois)
    else:
        out = ops.filter_per_class_lidar(pred_dev, prob_dev, FILTER_THRESH, O.TEST_NMS_THRESH, max_dets, max_out,
                                         roi_count=count_dev, want_rois=want_rois)
    return [t.cpu().numpy() for t in out], pred_dev.cpu()


def _check_filter_outputs(r, e, max_dets, max_out, live, out, pred_after):
    """dets / det_count / det_roi of one call against the CPU rule on the first min(live, r) RoIs."""
    prob, _, _ = _filter_case(r, e)
    rows, clamped = _filter_oracle(r, e, r if live is None else min(live, r))
    assert torch.equal(pred_after, clamped)
    dets, counts = out[0], out[1]
    assert dets.shape == (FILTER_K, max_out, e + 1)
    assert counts[0] == 0 and (dets[0] == 0).all()
    for j in range(1, FILTER_K):
        want = _cut_rows(rows[j], max_dets)[:max_out]
        assert counts[j] == len(want), (j, int(counts[j]), len(want))
        np.testing.assert_array_equal(dets[j, :len(want)], want)
        assert (dets[j, len(want):] == 0).all()
    if len(out) == 3:
        det_roi = out[2]
        assert (det_roi[0] == -1).all()
        for j in range(1, FILTER_K):
            m = int(counts[j])
            assert (det_roi[j, m:] == -1).all()
            rr = det_roi[j, :m]
            np.testing.assert_array_equal(dets[j, :m, :e], clamped.numpy()[rr, j * e:(j + 1) * e])
            np.testing.assert_array_equal(dets[j, :m, e], prob.numpy()[rr, j])
            assert len(set(rr.tolist())) == m


@gpu
@pytest.mark.parametrize("e", [4, 7])
@pytest.mark.parametrize("r,variant", FILTER_SIZES)
def test_filter_per_class_at_its_boundaries(hip, r, variant, e):
    """Rows, counts and det_roi equal the CPU rule's (O.filter_and_draw_prep[_lidar] + O.max_dets_cut, score order) with no
    cut, with the cut inside a run of equal scores (max_dets 1 and 100: the ties stay), with fewer output rows than kept
    boxes, with a live RoI count read on the device, with and without det_roi; with every RoI live the kept RoIs are the
    constructed survivors."""
    _, _, designs = _filter_case(r, e)
    live = r - 70
    hip.frcnn_filter_set_variant(variant)
    try:
        for max_dets, max_out, count, want_rois in ((0, r, None, True), (1, r, None, False), (100, r, None, True),
                                                    (100, 50, None, True), (0, 7, None, False), (0, r, live, True),
                                                    (100, r, live, False), (0, r, r + 9, False)):
            out, pred_after = _run_filter(r, e, max_dets, max_out, count, want_rois)
            _check_filter_outputs(r, e, max_dets, max_out, count, out, pred_after)
            if max_dets == 0 and count is None and want_rois:
                for j in range(1, FILTER_K):
                    d, roi_of_rank = designs[j]
                    np.testing.assert_array_equal(out[2][j, :out[1][j]], roi_of_rank[d.survivors])
    finally:
        hip.frcnn_filter_set_variant(0)


@gpu
@pytest.mark.parametrize("e", [4, 7])
def test_filter_refuses_more_than_8192_rois(hip, e):
    ops = _ops()
    r, k = 8193, FILTER_K
    prob = torch.zeros((r, k), dtype=torch.float32, device=DEV)
    pred = torch.full((r, k * e), -5.0, dtype=torch.float32, device=DEV)
    with pytest.raises(ops._hip.HipError, match="num_rois 8193 > 8192"):
        if e == 4:
            ops.filter_per_class(pred, prob, 1000.0, 600.0, 1.0, 0.05, 0.6, 100)
        else:
            ops.filter_per_class_lidar(pred, prob, 0.05, 0.6, 100)
    torch.cuda.synchronize()
    assert bool((pred == -5.0).all())                   # not even the clamp was launched


# ================================================================================================
# C. guard bands and poisoned workspaces
# ================================================================================================
def _guarded_nms(hip, boxes_dev, n, max_keep, ws, mask_offset=0):
    """One frcnn_nms call with every output between bands -> (keep_idx, keep_mask, keep_count) host arrays."""
    g_idx, g_mask, g_cnt = guarded_like(torch.int64, max_keep), ByteGuarded(n, OUT_BYTE, mask_offset), guarded_like(torch.int32, 1)
    assert g_mask.ptr % 16 == mask_offset and g_idx.ptr % 16 == 0
    rc = hip.frcnn_nms(boxes_dev.data_ptr(), None, n, 0.7, max_keep, g_idx.ptr, g_mask.ptr, g_cnt.ptr, ws.ptr, ws.nbytes,
                       _ops()._stream())
    assert rc == 0, hip.frcnn_last_error()
    torch.cuda.synchronize()
    assert g_idx.intact() and g_mask.intact() and g_cnt.intact() and ws.intact()
    return g_idx.typed(torch.int64).cpu().numpy(), g_mask.view.cpu().numpy(), int(g_cnt.typed(torch.int32).item())


@gpu
@pytest.mark.parametrize("n", [1, 64, 65, 12289, 16384])
def test_nms_inside_guard_bands(hip, n):
    """Bands intact, every element of keep_idx / keep_mask / keep_count written, results equal to the construction and to the
    same call through ops - on a workspace full of 0xFF, and again on the workspace a different input of the same size left."""
    ops = _ops()
    d, other = designed_boxes(n, 31, 1, 7.0, 64, False), designed_boxes(n, 32, 1, 7.0, 64, True)
    assert n < 3 or not np.array_equal(d.boxes, other.boxes)
    boxes_dev, other_dev = torch.from_numpy(d.boxes).to(DEV), torch.from_numpy(other.boxes).to(DEV)
    ws = ByteGuarded(hip.frcnn_nms_ws_bytes(n), POISON_BYTE)
    want = _expect_nms(d.survivors, n, n)
    first = _guarded_nms(hip, boxes_dev, n, n, ws)
    for got, ref in zip(first, want):
        np.testing.assert_array_equal(got, ref)
    k, c, m = ops.nms_sorted(boxes_dev, 0.7, want_mask=True)
    assert int(c.item()) == first[2]
    np.testing.assert_array_equal(k.cpu().numpy(), first[0])
    np.testing.assert_array_equal(m.cpu().numpy(), first[1])
    stale = _guarded_nms(hip, other_dev, n, n, ws)                 # leaves its own matrix behind
    for got, ref in zip(stale, _expect_nms(other.survivors, n, n)):
        np.testing.assert_array_equal(got, ref)
    again = _guarded_nms(hip, boxes_dev, n, n, ws)
    for got, ref in zip(again, first):
        np.testing.assert_array_equal(got, ref)


def fill_bytes_parts(offset, nbytes):
    """(head, 16-byte words, tail) of frcnn::fill_bytes on a destination ``offset`` bytes past a 16-byte boundary."""
    head = min((16 - offset) % 16, nbytes)
    return head, (nbytes - head) // 16, (nbytes - head) % 16


@gpu
@pytest.mark.parametrize("offset", [0, 1, 15])
@pytest.mark.parametrize("n", [70, 1000])
def test_nms_keep_mask_off_the_16_byte_grid(hip, n, offset):
    """keep_mask is zeroed by frcnn::fill_bytes: byte stores over an unaligned head and tail, 16-byte stores between.  The
    mask starts 0, 1 and 15 bytes past a 16-byte boundary, with sizes that leave a head (offsets 1, 15), a body and a tail."""
    head, body, tail = fill_bytes_parts(offset, n)
    assert body > 0 and tail > 0 and (head > 0) == (offset > 0)
    d = designed_boxes(n, 33, 1, 7.0, 64, False)
    ws = ByteGuarded(hip.frcnn_nms_ws_bytes(n), POISON_BYTE)
    got = _guarded_nms(hip, torch.from_numpy(d.boxes).to(DEV), n, n, ws, mask_offset=offset)
    for g, ref in zip(got, _expect_nms(d.survivors, n, n)):
        np.testing.assert_array_equal(g, ref)


TOPK_TIES = 80          # a run of equal scores around index 4096, of which the k-th key takes a part


@functools.lru_cache(maxsize=None)
def _topk_scores(n, top_n, seed):
    """Distinct even scores in random order, and TOPK_TIES equal odd scores at indices 4056 .. 4135 (both sides of the
    second 4096-score workgroup's first index, and of a thread's range in the one-workgroup kernel), valued so that the
    top_n-th key lies inside the run: 60 of them are taken (1 for top_n = 1, 79 when only one score is left out) - the first
    40 end at index 4095.  Returns (scores, order of the total order (score desc, index asc))."""
    rng = np.random.default_rng(seed)
    m = n - TOPK_TIES
    above = min(max(top_n - 60, 0), m)                  # scores above the run
    s = np.empty(n, np.float32)
    ties = np.arange(4096 - 40, 4096 + 40)
    rest = np.setdiff1d(np.arange(n), ties)
    s[rest] = rng.permutation(m).astype(np.float32) * 2
    s[ties] = 2.0 * (m - above) - 1.0
    assert int((s > s[ties[0]]).sum()) == above
    if n > top_n:
        assert 0 < top_n - above < TOPK_TIES and (top_n - above > 40 or top_n == 1)
    scores = torch.from_numpy(s)
    return scores, O.stable_desc_order(scores)


def _guarded_topk(hip, scores_dev, n, top_n, ws):
    take = min(n, top_n)
    g_ord, g_sc, g_cnt = guarded_like(torch.int64, take), guarded_like(torch.float32, take), guarded_like(torch.int32, 1)
    rc = hip.frcnn_sort_topk_desc(scores_dev.data_ptr(), n, top_n, g_ord.ptr, g_sc.ptr, g_cnt.ptr, ws.ptr, ws.nbytes,
                                  _ops()._stream())
    assert rc == 0, hip.frcnn_last_error()
    torch.cuda.synchronize()
    assert g_ord.intact() and g_sc.intact() and g_cnt.intact() and ws.intact()
    return g_ord.typed(torch.int64).cpu(), g_sc.typed(torch.float32).cpu(), int(g_cnt.typed(torch.int32).item())


@gpu
@pytest.mark.parametrize("n,top_n", [(16384, 16384), (16385, 16384), (20479, 6000), (20481, 6000), (20000, 1)])
def test_topk_inside_guard_bands(hip, n, top_n):
    """(16384, 16384): the one-workgroup kernel at its limit (no workspace: the view between the bands is empty);
    (16385, 16384): the multi-workgroup form with every candidate slot in use; 5 * 4096 -+ 1 scores: a last workgroup of
    4095 scores / of one; top_n = 1."""
    ops = _ops()
    take = min(n, top_n)
    scores, order = _topk_scores(n, top_n, 1)
    other, other_order = _topk_scores(n, top_n, 2)
    ws_bytes = hip.frcnn_sort_topk_desc_ws_bytes(n, top_n)
    assert (ws_bytes == 0) == (n <= 16384)
    ws = ByteGuarded(ws_bytes, POISON_BYTE)
    sd, od = scores.to(DEV), other.to(DEV)
    first = _guarded_topk(hip, sd, n, top_n, ws)
    assert first[2] == take
    assert torch.equal(first[0], order[:take])
    assert torch.equal(first[1].view(torch.int32), scores[order[:take]].view(torch.int32))
    o, s, c = ops.sort_topk_desc(sd, top_n)
    assert torch.equal(o.cpu(), first[0]) and torch.equal(s.cpu(), first[1]) and int(c.item()) == take
    stale = _guarded_topk(hip, od, n, top_n, ws)
    assert torch.equal(stale[0], other_order[:take]) and (take == 1 or not torch.equal(stale[0], first[0]))
    again = _guarded_topk(hip, sd, n, top_n, ws)
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and again[2] == first[2]


def _guarded_filter(hip, r, e, prob_dev, pred_dev, max_dets, max_out, ws):
    k = FILTER_K
    g_dets, g_cnt, g_roi = (guarded_like(torch.float32, k * max_out * (e + 1)), guarded_like(torch.int32, k),
                            guarded_like(torch.int32, k * max_out))
    if e == 4:
        rc = hip.frcnn_filter_per_class(pred_dev.data_ptr(), prob_dev.data_ptr(), None, r, k, 1000.0, 600.0, 1.0, FILTER_THRESH,
                                        O.TEST_NMS_THRESH, max_dets, max_out, g_dets.ptr, g_cnt.ptr, g_roi.ptr, ws.ptr,
                                        ws.nbytes, _ops()._stream())
    else:
        rc = hip.frcnn_filter_per_class_lidar(pred_dev.data_ptr(), prob_dev.data_ptr(), None, r, k, FILTER_THRESH,
                                              O.TEST_NMS_THRESH, max_dets, max_out, g_dets.ptr, g_cnt.ptr, g_roi.ptr, ws.ptr,
                                              ws.nbytes, _ops()._stream())
    assert rc == 0, hip.frcnn_last_error()
    torch.cuda.synchronize()
    assert g_dets.intact() and g_cnt.intact() and g_roi.intact() and ws.intact()
    return [g_dets.typed(torch.float32, (k, max_out, e + 1)).cpu().numpy(), g_cnt.typed(torch.int32).cpu().numpy(),
            g_roi.typed(torch.int32, (k, max_out)).cpu().numpy()]


@gpu
@pytest.mark.parametrize("e", [4, 7])
@pytest.mark.parametrize("r", [960, 961, 8192])
def test_filter_inside_guard_bands(hip, r, e):
    """dets / det_count / det_roi between bands and pre-filled, the workspace exactly frcnn_filter_per_class_ws_bytes long and
    full of 0xFF (the LDS kernel at 960 RoIs must leave it alone): the CPU rule's rows, the same call through ops, and the
    same bits again on the workspace a different input left behind."""
    ops = _ops()
    prob, pred, _ = _filter_case(r, e)
    max_dets, max_out = 100, r
    prob_dev = prob.to(DEV)
    flip = torch.arange(r - 1, -1, -1)
    other_prob, other_pred = prob[flip].contiguous().to(DEV), pred[flip].contiguous().to(DEV)   # another input, same size
    ws_bytes = hip.frcnn_filter_per_class_ws_bytes(r, FILTER_K)
    ws = ByteGuarded(ws_bytes, POISON_BYTE)
    pred_dev = pred.clone().to(DEV)
    first = _guarded_filter(hip, r, e, prob_dev, pred_dev, max_dets, max_out, ws)
    _check_filter_outputs(r, e, max_dets, max_out, None, first, pred_dev.cpu())
    if r == 960:
        assert bool((ws.view == POISON_BYTE).all())
    via_ops, _ = _run_filter(r, e, max_dets, max_out, None, True)
    for a, b in zip(first, via_ops):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    stale = _guarded_filter(hip, r, e, other_prob, other_pred, max_dets, max_out, ws)
    assert not np.array_equal(stale[2], first[2])
    again = _guarded_filter(hip, r, e, prob_dev, pred.clone().to(DEV), max_dets, max_out, ws)
    for a, b in zip(again, first):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
