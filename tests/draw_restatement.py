"""numpy float64 restatement of the drawing rules of include/frcnn_hip.h (frcnn_canvas_* / frcnn_draw_*), written from the
reference's lines (lib/datasets/waymo_imdb.py:190-253, waymo_lidb.py:229-328, kitti_lidb.py:289-378, db.py:260-303,
lib/utils/bbox.py:174-233,346-379) and Pillow's documented behaviour, not from the kernels: whole-array numpy for the
canvases, a Python loop over detections for the plan, boolean masks for the outlines and a serial painter that draws one
row after the other.  Shared by tests/test_draw_host.py (against Pillow), test_draw_kernels.py and test_draw_det.py."""
import numpy as np

ROW_INTS = 12
SKIP, RECT, FOOTPRINT = 0, 1, 2
PIN = 1 << 30


def to_byte(v):
    """astype(uint8) for in-range values (truncation toward zero); saturated outside, NaN -> 0 (the stated deviation)."""
    v = np.asarray(v, np.float64)
    v = np.where(np.isnan(v), 0.0, v)
    return np.trunc(np.clip(v, 0.0, 255.0)).astype(np.uint8)


def canvas_image(blob, stds, means, arrange):
    """waymo_imdb.py:200-204 with the arithmetic in float64."""
    img = blob[0].astype(np.float64)
    img = img * np.asarray(stds, np.float64).reshape(1, 1, 3)
    img = img + np.asarray(means, np.float64).reshape(1, 1, 3)
    img = img[:, :, list(arrange)]
    return to_byte(img)


def _scale(num, den):
    """num / den, or 0 where the range is empty or the factor would not be finite."""
    if den == 0 or not np.isfinite(den):
        return 0.0
    f = num / den
    return f if np.isfinite(f) else 0.0


def canvas_bev(blob, slices, form):
    """waymo_lidb.py:240-261 ('waymo') / kitti_lidb.py:289-297 ('kitti') in float64; the input is not modified."""
    grid = blob[0].astype(np.float64)
    h = grid[:, :, :slices].copy()
    if form == 'waymo':
        for i in range(slices):
            mask = np.abs(h[:, :, i]) > 0.00001
            h[:, :, i] = np.where(mask, h[:, :, i] + i * 0.5, h[:, :, i])
    allnan = np.isnan(h).all(axis=2)
    hmax = np.where(allnan, 0.0, np.fmax.reduce(h, axis=2))
    if form == 'waymo':
        mask = np.abs(hmax) > 0.00001
        masked = np.where(mask, hmax, 0.0)
        max_height, min_height = masked.max() * 1.5, masked.min()
        g_num, b_num = 6 * 255.0, 2 * 255.0
    else:
        mask = np.ones(hmax.shape, bool)
        max_height, min_height = hmax.max(), hmax.min()
        g_num, b_num = 255.0, 255.0
    out = np.zeros(hmax.shape + (3,), np.uint8)
    sr = _scale(255.0, max_height - min_height)
    sg = _scale(g_num, np.fmax.reduce(grid[:, :, slices], axis=None))
    sb = _scale(b_num, np.fmax.reduce(grid[:, :, slices + 1], axis=None))
    if sr != 0.0:
        out[:, :, 0] = np.where(mask, to_byte(hmax * sr), 0)
    if sg != 0.0:
        out[:, :, 1] = to_byte(grid[:, :, slices] * sg)
    if sb != 0.0:
        out[:, :, 2] = to_byte(grid[:, :, slices + 1] * sb)
    return out


def pil_int(v):
    """Pillow's (int) of a double corner: truncation toward zero; pinned to +-2^30."""
    v = float(v)
    return PIN if v >= PIN else -PIN if v <= -PIN else int(v)


def clamp255(v):
    return min(max(int(v), 0), 255)


def footprint_corners(box, width, height):
    """bbox_3d_to_bev_4pt + rotate_in_bev (float64, result as float32), draw_bev_bboxes' clip and truncation."""
    xc, yc, l, w, ry = (np.float64(box[i]) for i in (0, 1, 3, 4, 6))
    x1, x2, y1, y2 = xc - l / 2, xc + l / 2, yc - w / 2, yc + w / 2
    pts = [(x1, y1), (x1, y2), (x2, y2), (x2, y1)]
    out = []
    with np.errstate(invalid='ignore'):
        for px, py in pts:
            dx, dy = px - xc, py - yc
            rx = np.float32(dx * np.cos(ry) - dy * np.sin(ry) + xc)
            rr = np.float32(dx * np.sin(ry) + dy * np.cos(ry) + yc)
            rx = np.float32(0) if np.isnan(rx) else np.clip(rx, 0, width - 1)
            rr = np.float32(0) if np.isnan(rr) else np.clip(rr, 0, height - 1)
            out += [int(rx), int(rr)]
    return out


def class_order(cls_rows, key):
    """np.argsort(-sortable) of db.py:283-303 with this library's tie rule (ties to the lower row, NaN last)."""
    n = len(cls_rows)
    if key is None:
        return list(np.argsort(-np.arange(n), kind='stable'))
    col, cols = key
    keys = []
    for r in cls_rows:
        s = np.float32(r[col])
        for c in range(1, cols):
            s = np.float32(s + np.float32(r[col + c]))
        keys.append(np.float32(s / np.float32(cols)))
    keys = np.asarray(keys, np.float32)
    finite = [i for i in range(n) if not np.isnan(keys[i])]
    nan = [i for i in range(n) if np.isnan(keys[i])]
    finite.sort(key=lambda i: (-float(keys[i]), i))
    return finite + nan


def plan(dets, counts, canvas_hw, lidar, key=None, limiter0=15, limiter_resets=None, gt=None, gt_labels=None):
    """The draw list: (capacity, 12) int32, row i = the i-th thing the reference draws."""
    k, max_out, _ = dets.shape
    height, width = canvas_hw
    if limiter_resets is None:
        limiter_resets = not lidar
    num_gt = 0 if gt is None else len(gt)
    rows = np.zeros(((k - 1) * max_out + num_gt, ROW_INTS), np.int32)
    items = []

    def geometry(box):
        coords = [box[i] for i in ((0, 1, 3, 4, 6) if lidar else (0, 1, 2, 3))]
        if any(np.isnan(np.float64(c)) for c in coords):
            return SKIP, [0] * 8
        if lidar:
            return FOOTPRINT, footprint_corners(box, width, height)
        return RECT, [pil_int(c) for c in coords] + [0] * 4

    gt_items = []
    for g in range(num_gt):
        c = (127 if lidar else 0) if int(gt_labels[g]) == 0 else 255
        gt_items.append((geometry(gt[g]), 2 if lidar else 1, (c, c, c)))
    det_items = []
    limiter = limiter0
    for j in range(1, k):
        n = min(max(int(counts[j]), 0), max_out)
        if n == 0:
            continue
        if n < limiter:
            limiter = n
        elif limiter_resets:
            limiter = limiter0
        score_col = 7 if lidar else 4
        for i, idx in enumerate(class_order(dets[j, :n], key)):
            det = dets[j, idx]
            uc_gradient = int((limiter - i) / limiter * 255.0)
            gf = np.float32(det[score_col]) * np.float32(255.0)
            green = 0 if np.isnan(gf) else int(np.clip(gf, 0, 255))
            det_items.append((geometry(det), 2, (0, green, uc_gradient)))
    items = gt_items + det_items if lidar else det_items + gt_items
    for seq, ((kind, geo), wd, (r, g, b)) in enumerate(items):
        rows[seq, 0], rows[seq, 1], rows[seq, 2] = kind, wd, seq
        rows[seq, 3] = clamp255(r) | (clamp255(g) << 8) | (clamp255(b) << 16)
        rows[seq, 4:12] = geo
    for seq in range(len(items), len(rows)):
        rows[seq, 2] = seq
    return rows


def rect_mask(x0, y0, x1, y1, wd, height, width):
    """Pixels of [x0,x1] x [y0,y1] within wd pixels of the rectangle's border, on the canvas."""
    ys, xs = np.mgrid[0:height, 0:width]
    inside = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
    near = (xs - x0 < wd) | (x1 - xs < wd) | (ys - y0 < wd) | (y1 - ys < wd)
    return inside & near


def edge_pixels(ax, ay, bx, by):
    """Width-1 edge from (ax, ay) to (bx, by): for i = 0..dmaj the pixel major0 + s_major*i,
    minor0 + s_minor*((2*i*dmin + dmaj) // (2*dmaj)); x is the major axis iff dx > dy."""
    dx, dy = abs(bx - ax), abs(by - ay)
    sx, sy = (1 if bx >= ax else -1), (1 if by >= ay else -1)
    if dx == 0 and dy == 0:
        return [(ax, ay)], 'y'
    if dx > dy:
        return [(ax + sx * i, ay + sy * ((2 * i * dy + dx) // (2 * dx))) for i in range(dx + 1)], 'x'
    return [(ax + sx * ((2 * i * dx + dy) // (2 * dy)), ay + sy * i) for i in range(dy + 1)], 'y'


def edge_mask(ax, ay, bx, by, wd, height, width):
    mask = np.zeros((height, width), bool)
    pts, major = edge_pixels(ax, ay, bx, by)
    for x, y in pts:
        for side in range(wd):
            px, py = (x, y + side) if major == 'x' else (x + side, y)
            if 0 <= px < width and 0 <= py < height:
                mask[py, px] = True
    return mask


def row_mask(row, height, width):
    kind, wd = int(row[0]), int(row[1])
    g = [int(v) for v in row[4:12]]
    if kind == RECT:
        return rect_mask(g[0], g[1], g[2], g[3], wd, height, width)
    mask = np.zeros((height, width), bool)
    if kind == FOOTPRINT:
        for i in range(4):                                # draw_polygon: corner i -> corner i-1
            a, b = i, (i - 1) % 4
            mask |= edge_mask(g[2 * a], g[2 * a + 1], g[2 * b], g[2 * b + 1], wd, height, width)
    return mask


def paint(canvas, rows):
    """Serial painter: one row after the other, later rows over earlier ones.  Returns a new canvas."""
    out = canvas.copy()
    height, width = out.shape[:2]
    for row in rows:
        if int(row[0]) == SKIP:
            continue
        rgb = int(row[3])
        out[row_mask(row, height, width)] = (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)
    return out


def render(blob, lidar, dets, counts, gt=None, gt_labels=None, key=None, bev_form='waymo', slices=12, stds=(1, 1, 1),
           means=(0, 0, 0), arrange=(2, 1, 0), boxes=True):
    """A whole frame: canvas, plan, painter."""
    canvas = canvas_bev(blob, slices, bev_form) if lidar else canvas_image(blob, stds, means, arrange)
    if lidar and not boxes:
        return canvas
    rows = plan(dets, counts, canvas.shape[:2], lidar, key=key, limiter0=15, gt=gt, gt_labels=gt_labels)
    return paint(canvas, rows)
