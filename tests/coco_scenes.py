"""Scenes for the COCO evaluator's tests (test_coco_eval_host.py, test_coco_eval_device.py): the hand cases of the protocol,
a seeded scene with every situation the matching rules distinguish, pairs at the sizes where the kernel's layout changes,
and the conditions a scene must meet before a comparison on it means anything (read from the HOST path's result)."""
import numpy as np

IMAGE_IDS = [100 + 3 * i for i in range(40)]        # not contiguous, so an index is never mistaken for an id
CAT_IDS = [1, 3, 4, 7, 9, 12]
BIG_PAIR = (IMAGE_IDS[5], CAT_IDS[2])               # the pair with 130 detections
EMPTY_IMAGE = IMAGE_IDS[17]                         # neither ground truth nor detections


def annotations(image_ids, cat_ids, boxes):
    """A COCO annotation dict; ``boxes``: (image id, category id, [x, y, w, h], iscrowd[, area])."""
    anns = []
    for i, b in enumerate(boxes):
        a = {'id': i + 1, 'image_id': b[0], 'category_id': b[1], 'bbox': list(b[2]), 'iscrowd': int(b[3])}
        if len(b) > 4:
            a['area'] = b[4]
        anns.append(a)
    return {'images': [{'id': i} for i in image_ids], 'categories': [{'id': c} for c in cat_ids], 'annotations': anns}


def results(dets):
    """A results list; ``dets``: (image id, category id, [x, y, w, h], score)."""
    return [{'image_id': d[0], 'category_id': d[1], 'bbox': list(d[2]), 'score': d[3]} for d in dets]


def one_pair(gts, dets):
    """One image, one category: ``gts`` (box, iscrowd[, area]), ``dets`` (box, score)."""
    return (annotations([1], [1], [(1, 1) + tuple(g) for g in gts]), results([(1, 1) + tuple(d) for d in dets]))


def hand_cases():
    """The issue's cases 1-7 as {name: (annotation dict, results list)}; the expected values are in the host tests."""
    return {
        'identical': one_pair([([10, 10, 50, 50], 0)], [([10, 10, 50, 50], .9)]),
        'iou_077': one_pair([([0, 0, 100, 100], 0)], [([0, 0, 100, 77], .9)]),
        'crowd': one_pair([([0, 0, 10, 10], 0), ([20, 0, 40, 40], 1)],
                          [([25, 5, 10, 10], .97), ([30, 10, 10, 10], .96), ([200, 200, 10, 10], .95), ([0, 0, 10, 10], .90)]),
        'area_range': one_pair([([0, 0, 20, 20], 0)], [([0, 0, 20, 20], .9), ([100, 100, 200, 200], .95)]),
        'max_dets': one_pair([([0, 0, 10, 10], 0), ([100, 100, 10, 10], 0)], [([0, 0, 10, 10], .9), ([100, 100, 10, 10], .9)]),
        'threshold': one_pair([([0, 0, 10, 10], 0)], [([0, 0, 10, 5], .9)]),
        'tie': one_pair([([0, 0, 10, 10], 0), ([0, 0, 10, 10], 0)], [([0, 0, 10, 5], .9)]),
        'boundaries': one_pair([([0, 0, 32, 32], 0), ([100, 0, 40, 40], 0, 1024.0), ([200, 0, 10, 10], 0, 5000.0)],
                               [([0, 0, 32, 32], .9)]),
    }


def _size(rng, kind):
    lo, hi = {'small': (4, 30), 'medium': (34, 90), 'large': (100, 240)}[kind]
    return int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))


def seeded_scene(seed=0):
    """(annotation dict, results list): 40 images, 6 categories; see the module docstring of test_coco_eval_device.py for
    what it contains."""
    rng = np.random.default_rng(seed)
    boxes, dets = [], []

    def score():
        return round(float(rng.uniform(.05, 1.0)), 2)           # quantised: ties inside and across images

    for ii, img in enumerate(IMAGE_IDS):
        if img == EMPTY_IMAGE:
            continue
        for ci, cat in enumerate(CAT_IDS):
            if (img, cat) == BIG_PAIR:
                n_gt = 12
            else:
                n_gt = int(rng.choice([0, 0, 0, 1, 1, 2, 3, 4, 6, 9]))
            x = 0
            mine = []
            for j in range(n_gt):
                kind = ['small', 'medium', 'large'][int(rng.integers(0, 3))]
                w, h = _size(rng, kind)
                pick = rng.random()
                if pick < .08:
                    w, h = 32, 32                               # area exactly 1024
                elif pick < .16:
                    w, h = 96, 96                               # area exactly 9216
                elif pick < .24:
                    w, h = 20, 20                               # overlaps of exactly .5 and .75 are planted on these
                crowd = rng.random() < .15
                if crowd:
                    w, h = max(w, 60), max(h, 60)
                y = int(rng.integers(0, 300))
                box = [x, y, w, h]
                x += w + int(rng.integers(5, 40))
                entry = (img, cat, box, crowd)
                if rng.random() < .2:
                    entry = entry + (round(w * h * float(rng.uniform(.4, 1.0)), 1),)     # a segment's area, not w*h
                boxes.append(entry)
                mine.append((box, crowd))
                if not crowd and rng.random() < .12:
                    boxes.append(entry)                         # the same box listed twice: the later one wins a tie
                    mine.append((box, crowd))
            for box, crowd in mine:
                bx, by, bw, bh = box
                if crowd:
                    for _ in range(int(rng.integers(2, 4))):    # several detections inside a crowd box
                        dets.append((img, cat, [bx + int(rng.integers(0, bw // 2)), by + int(rng.integers(0, bh // 2)),
                                                int(rng.integers(5, bw // 2)), int(rng.integers(5, bh // 2))], score()))
                    if rng.random() < .7:                       # a plain box inside the crowd box, and its detection
                        inner = [bx + 5, by + 5, 24, 24]
                        boxes.append((img, cat, inner, False))
                        dets.append((img, cat, [bx + 5, by + 6, 24, 24 - int(rng.integers(0, 8))], score()))
                    continue
                if rng.random() < .15:
                    continue                                    # missed
                if (bw, bh) == (20, 20):
                    dets.append((img, cat, [bx, by, 20, [10, 15][int(rng.integers(0, 2))]], score()))
                    continue
                pick = rng.random()
                if pick < .15:
                    d = [bx, by, bw, bh]
                elif pick < .5:                                 # integer jitter
                    d = [bx + int(rng.integers(-3, 4)), by + int(rng.integers(-3, 4)),
                         max(2, bw + int(rng.integers(-6, 7))), max(2, bh + int(rng.integers(-6, 7)))]
                else:                                           # float jitter, up to a quarter of the box
                    f = rng.uniform(-.25, .25, 4)
                    d = [bx + float(f[0]) * bw, by + float(f[1]) * bh, bw * (1 + float(f[2])), bh * (1 + float(f[3]))]
                s = score()
                dets.append((img, cat, d, s))
                if rng.random() < .2:
                    dets.append((img, cat, list(d), s if rng.random() < .5 else score()))   # a duplicate
            n_far = int(rng.integers(0, 4)) if (n_gt or rng.random() < .3) else 0
            for _ in range(n_far):                              # matched by nothing, of every size
                w, h = _size(rng, ['small', 'medium', 'large'][int(rng.integers(0, 3))])
                dets.append((img, cat, [600 + float(rng.uniform(0, 300)), float(rng.uniform(0, 300)), w, h], score()))
            if (img, cat) == BIG_PAIR:
                have = sum(1 for d in dets if (d[0], d[1]) == BIG_PAIR)
                for _ in range(130 - have):
                    w, h = _size(rng, 'small')
                    dets.append((img, cat, [float(rng.uniform(0, 900)), float(rng.uniform(0, 400)), w, h], score()))
    order = rng.permutation(len(dets))                          # a results file is not grouped by pair
    return annotations(IMAGE_IDS, CAT_IDS, boxes), results([dets[i] for i in order])


def sized_pairs():
    """(annotation dict, results list) of four pairs at the sizes where the kernel's layout changes: D x G = 100 x 90
    (above the LDS budget), 30 x 65 and 30 x 64 (either side of the register mask), 1 x 1.  One image each."""
    rng = np.random.default_rng(7)
    boxes, dets = [], []
    for img, (D, G) in enumerate([(100, 90), (30, 65), (30, 64), (1, 1)], start=1):
        gts = []
        for g in range(G):
            w, h = int(rng.integers(10, 120)), int(rng.integers(10, 120))
            box = [(g % 10) * 130 + int(rng.integers(0, 10)), (g // 10) * 130 + int(rng.integers(0, 10)), w, h]
            gts.append(box)
            boxes.append((img, 1, box, rng.random() < .15))
        for d in range(D):
            bx, by, bw, bh = gts[int(rng.integers(0, G))]
            f = rng.uniform(-.2, .2, 4)
            dets.append((img, 1, [bx + float(f[0]) * bw, by + float(f[1]) * bh, bw * (1 + float(f[2])), bh * (1 + float(f[3]))],
                         round(float(rng.uniform(.05, 1.0)), 2)))
    return annotations([1, 2, 3, 4], [1], boxes), results(dets)


def scene_conditions(r):
    """The conditions of a seeded scene, from a HOST result dict: {name: bool}."""
    A, T = r['dt_match'].shape[1:]
    matched, ignored = r['dt_match'] >= 0, r['dt_ignore'].astype(bool)
    tps = (matched & ~ignored)[:, 0, :].sum(axis=0)
    cond = {'tp_counts_differ': bool((np.diff(tps) != 0).all()),
            'ignored_by_area_alone': bool((~matched & ignored).any()),
            'overlap_equals_threshold': bool(np.isin(r['ious'], r['params'].iou_thrs).any()),
            'stop_rule': False, 'crowd_rematched': False, 'tie_to_later': False}
    for q in range(r['det_offsets'].shape[0] - 1):
        d0, d1 = int(r['det_offsets'][q]), int(r['det_offsets'][q + 1])
        g0, g1 = int(r['gt_offsets'][q]), int(r['gt_offsets'][q + 1])
        D, G = d1 - d0, g1 - g0
        if not D or not G:
            continue
        ov = r['ious'][int(r['iou_offsets'][q]):int(r['iou_offsets'][q + 1])].reshape(D, G)
        crowd = r['gt_crowd'][g0:g1].astype(bool)
        for a in range(A):
            ig = r['gt_ignore'][g0:g1, a].astype(bool)
            for t in range(T):
                m = r['dt_match'][d0:d1, a, t]
                for d in range(D):
                    if m[d] < 0:
                        continue
                    earlier = set(int(v) for v in m[:d] if v >= 0)
                    if crowd[m[d]] and int(m[d]) in earlier:
                        cond['crowd_rematched'] = True
                    if not ig[m[d]] and (crowd & (ov[d] >= ov[d, m[d]])).any():
                        cond['stop_rule'] = True          # an always-available ignored box overlapped at least as much
                    for g in range(int(m[d])):
                        if ig[g] == ig[m[d]] and ov[d, g] == ov[d, m[d]] and g not in earlier:
                            cond['tie_to_later'] = True
    return cond
