"""The BEV voxeliser (csrc/voxelize.hip: vox_cell, vox_flag, scan_excl twice, vox_count, vox_fill, vox_feature, vox_meta) at
its edges, called directly through ops.bev_voxelize and compared with ``ref_voxelize``, a vectorised numpy restatement of
lib/roi_data_layer/minibatch.py:232-235,434-512 + the spconv voxel generator.

The unmarked tests validate the reference itself: against the oracle's literal loops (O.get_lidar_blob,
O.points_to_voxel), the tile arithmetic of scan_excl_kernel restated in numpy against np.cumsum, and the preconditions
without which a GPU case would test nothing (edge points on both sides of an edge, a height at which float32 and float64
slices differ).  The GPU tests (marked gpu) run the kernels.

Which case reaches which regime (ids as pytest prints them):
  first scan (num_points)     test_scan_edges[n-layout]: 21 sizes around 4, 64, 256, 1024 and the 4096-item tile; layout
                              "distinct" = one cell per point (flags all ones but for the outside rows), "late" = flags all
                              zero except at 0, n // 2, n - 1, 4095, 4096, 4097, 8191, 8192
  second scan (max_voxels)    test_voxel_cap[mv]: 1 .. 5, 63 .. 65, 4095 .. 4097, V - 1, V, V + 1; the cut falls INSIDE a
                              column (rank mv - 1 kept, rank mv cut) and revisits of cut cells follow
  selection loop              test_selection[max_points]: 9 values x segments of 1 .. 1000 points, shuffled, z maximum in and
                              outside the kept prefix
  parameters                  test_parameters[...]: stride, elongation column, num_meta, z_shift, gz < num_slices, non-square
  cell edges                  test_cell_edges_direct[vlen], test_cell_edges_through_get_lidar_blob[scale]
  degenerate clouds           test_degenerate[...]
  grid-stride second trip     test_second_grid_stride_trip: 1 048 576 + 300 points
  height-slice arithmetic     test_height_slices_are_the_float64_expression[h]: 0.4 and 0.3 (float64 product, one rounding)

Bars.  Occupancy, density, the occupied-cell count and the height slices are compared with assert_array_equal: the kernel
evaluates the slice as (float)((double)zmax - (double)cz * h) with h the caller's double, which IS the reference's numpy
expression, so equality holds at every voxel height, not only where cz * h is exact in float32 (0.5, 0.25).  The two tanh
channels: the kernel adds at most max_points float32 values in ascending point order, the reference adds them in float64;
|difference of the means| <= (keep - 1) * 2^-24 * sum(|values|) / keep (first-order bound of a sequential sum), tanh has
slope <= 1, and the store rounds by half a float32 ulp (of the larger of the two values).  That bound is computed per voxel (``meta_bound``), never one
global rtol.  Where the values are multiples of 2^-12 with an exactly representable sum the bound is zero and equality with
float32(np.tanh(float64 mean)) is required up to ONE float32 ulp (device tanh and libm tanh may differ in the last place of
the double, which can flip the float32 rounding; test_selection prints the largest difference: 0 ulp on the MI355X).
The per-voxel bar also carries two double ulps for that last place of tanh, so a near-tie cannot fail it.
"""
import ctypes
import functools
import types

import numpy as np
import pytest

from oracle import frcnn_oracle as O

DEV = "cuda:0"
TILE = 4096                                  # scan_excl_kernel: 1024 threads x 4 items
GRID_TRIP = 4096 * 256                       # blocks_for caps at 4096 blocks of 256: one trip covers 1 048 576 points

# the small grid of most cases: 32 x 32 x 12 cells of 0.25 m (all binary fractions: cz * 0.25 is exact), z shifted by -1
RANGE = [0.0, -4.0, 0.0, 8.0, 4.0, 3.0]
VOXEL = [0.25, 0.25, 0.25]
Z_SHIFT = -1.0
SLICES = 12
SCAN_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def ref_grid(pc_range, voxel_size):
    rng, vs = np.asarray(pc_range, np.float32), np.asarray(voxel_size, np.float32)
    return np.round((rng[3:] - rng[:3]) / vs).astype(np.int64)                   # spconv; lrintf in the library


def ref_cells(points, pc_range, voxel_size, z_shift, divide=True):
    """(ok (N,), integer cell coordinates (N, 3) as float32) in the kernel's expression order, all float32."""
    pts = np.asarray(points, np.float32)
    rng, vs = np.asarray(pc_range, np.float32), np.asarray(voxel_size, np.float32)
    zs = np.float32(z_shift)
    fmin, fmax = rng[:3].copy(), rng[3:].copy()
    fmin[2], fmax[2] = rng[2] + zs, rng[5] + zs                                  # filter_points on the RAW coordinates
    grid = ref_grid(pc_range, voxel_size)
    with np.errstate(invalid="ignore"):
        raw = pts[:, :3]
        ok = (raw >= fmin).all(1) & (raw < fmax).all(1)
        v = raw.copy()
        v[:, 2] = raw[:, 2] - zs                                                 # z - z_shift first
        t = np.floor((v - rng[:3]) / vs) if divide else np.floor((v - rng[:3]) * (np.float32(1) / vs))
        ok &= ((t >= 0) & (t < grid.astype(np.float32))).all(1)
    return ok, t


def ref_voxelize(points, pc_range, voxel_size, z_shift, max_points, max_voxels, num_slices, num_meta, elong_col):
    """numpy restatement without a loop over points.  Returns a namespace:
    bev (gy, gx, C) float32; count = occupied cells BEFORE the cap; cells_by_rank (count,) linear cell id of every cell in
    first-appearance order (voxel v < min(count, max_voxels) is cells_by_rank[v]); vox_of_point (N,) voxel number or -1;
    npts (V,) points per voxel before the max_points cut; keep (V,); kept (V, max_points) point rows in file order, -1 padded;
    meta64 / meta_bound (gy, gx, 2): float64 tanh(mean intensity / elongation) and the float32-sum bound of the module
    docstring (without the final half ulp)."""
    pts = np.asarray(points, np.float32)
    h = float(voxel_size[2])                                                     # the Python float of minibatch.py:467
    zs = np.float32(z_shift)
    gx, gy, gz = (int(g) for g in ref_grid(pc_range, voxel_size))
    ok, t = ref_cells(pts, pc_range, voxel_size, z_shift)
    idx = np.nonzero(ok)[0]
    c = t[idx].astype(np.int64)
    cell = (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0]
    uniq, first, inv = np.unique(cell, return_index=True, return_inverse=True)
    count = len(uniq)
    order = np.argsort(first, kind="stable")                                     # rank the first indices
    rank = np.empty(count, np.int64)
    rank[order] = np.arange(count)
    cells_by_rank = uniq[order]
    vox = rank[inv.reshape(-1)]
    V = min(count, int(max_voxels))
    alive = vox < max_voxels                                                     # the cap
    vox_of_point = np.full(len(pts), -1, np.int64)
    vox_of_point[idx[alive]] = vox[alive]
    o = np.argsort(vox[alive], kind="stable")                                    # by voxel, file order inside a run
    pv, pi = vox[alive][o], idx[alive][o]
    npts = np.bincount(pv, minlength=V)
    pos = np.arange(len(pv)) - (np.cumsum(npts) - npts)[pv]
    sel = pos < max_points
    kv, kp, kpos = pv[sel], pi[sel], pos[sel]
    keep = np.minimum(npts, max_points)
    kept = np.full((V, int(max_points)), -1, np.int64)
    kept[kv, kpos] = kp
    C = int(num_slices) + int(num_meta)
    out = types.SimpleNamespace(bev=np.zeros((gy, gx, C), np.float32), count=count, cells_by_rank=cells_by_rank,
                                vox_of_point=vox_of_point, npts=npts, keep=keep, kept=kept, grid=(gx, gy, gz),
                                meta64=np.zeros((gy, gx, 2)), meta_bound=np.zeros((gy, gx, 2)))
    if V == 0:
        return out
    starts = np.cumsum(keep) - keep                                              # every voxel keeps >= 1 point
    zmax = np.maximum.reduceat(pts[kp, 2] - zs, starts)
    zmax = np.where(keep < max_points, np.maximum(zmax, np.float32(0)), zmax)    # np.amax over the zero-padded buffer
    vc = cells_by_rank[:V]
    cx, cy, cz = vc % gx, (vc // gx) % gy, vc // (gx * gy)
    out.zmax = zmax.astype(np.float32)
    out.coords = np.stack((cx, cy, cz), 1)
    out.bev[cy, cx, cz] = (zmax.astype(np.float64) - cz * h).astype(np.float32)  # float64, rounded once on the store
    last = np.full(gy * gx, -1, np.int64)
    np.maximum.at(last, cy * gx + cx, np.arange(V))                              # the voxel created last in a column
    win = np.nonzero(last[cy * gx + cx] == np.arange(V))[0]
    meta = np.zeros((V, 3))
    bound = np.zeros((V, 3))
    meta[:, 0] = keep / max_points
    for m, col in ((1, 3), (2, elong_col)):
        if col < 0:
            continue
        vals = pts[kp, col].astype(np.float64)
        meta[:, m] = np.tanh(np.add.reduceat(vals, starts) / keep)
        bound[:, m] = (keep - 1) * 2.0 ** -24 * np.add.reduceat(np.abs(vals), starts) / keep
    for m in range(min(int(num_meta), 3)):
        out.bev[cy[win], cx[win], num_slices + m] = meta[win, m].astype(np.float32)
    out.meta64[cy[win], cx[win]] = meta[win, 1:]
    out.meta_bound[cy[win], cx[win]] = bound[win, 1:]
    return out


def scan_excl_restated(a, carry_thread=1023):
    """scan_excl_kernel in numpy: tiles of 4096 items, 4 per thread, a 64-lane inclusive scan per wave, 16 wave totals,
    and the carry that thread 1023 leaves for the next tile.  Returns (out, total)."""
    a = np.asarray(a, np.int64)
    n = len(a)
    out = np.zeros(n, np.int64)
    carry = 0
    for base in range(0, n, TILE):
        v = np.zeros(TILE, np.int64)
        m = min(TILE, n - base)
        v[:m] = a[base:base + m]
        v = v.reshape(1024, 4)
        mine = (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])
        incl = np.cumsum(mine.reshape(16, 64), axis=1)                           # shuffle scan inside each wave
        wave_sum = incl[:, 63]
        before = np.concatenate(([0], np.cumsum(wave_sum)[:-1]))                 # for (w < wave) run += wave_sum[w]
        run = carry + (incl - mine.reshape(16, 64)).reshape(-1) + np.repeat(before, 64)
        tile_out = run[:, None] + np.concatenate((np.zeros((1024, 1), np.int64), np.cumsum(v, 1)[:, :3]), 1)
        out[base:base + m] = tile_out.reshape(-1)[:m]
        carry = int(run[carry_thread] + v[carry_thread].sum())                   # if (t == 1023) carry_s = run
    return out, carry


# ---------------------------------------------------------------------------------------------------------------
# case builders (seeded, shared by the CPU and the GPU side)
# ---------------------------------------------------------------------------------------------------------------
CFG = dict(pc_range=RANGE, voxel_size=VOXEL, z_shift=Z_SHIFT, max_points=5, max_voxels=12293, num_slices=SLICES,
           num_meta=3, elong_col=4)


def _cfg(**kw):
    c = dict(CFG)
    c.update(kw)
    return c


def _cell_points(rng, cells, grid=(32, 32, 12), stride=5, rmin=(0.0, -4.0, 0.0), vsize=VOXEL, z_shift=Z_SHIFT):
    """One row per linear cell id, strictly inside its cell (jitter in [0.2, 0.8) of the voxel), raw z = z + z_shift."""
    cells = np.asarray(cells, np.int64)
    gx, gy, _ = grid
    c = np.stack((cells % gx, (cells // gx) % gy, cells // (gx * gy)), 1)
    p = np.zeros((len(cells), stride), np.float32)
    p[:, :3] = np.asarray(rmin) + (c + rng.uniform(0.2, 0.8, c.shape)) * np.asarray(vsize)
    p[:, 2] += z_shift
    p[:, 3:] = rng.uniform(0, 3, (len(cells), stride - 3))
    return p


def _outside_rows(rng, k, stride=5):
    """Rows the range test must drop, one kind after the other: beyond each face of the box, NaN, +Inf, -Inf."""
    p = _cell_points(rng, rng.integers(0, 32 * 32 * 12, k), stride=stride)
    kinds = [(0, 8.0), (0, -0.001), (1, 4.0), (1, -4.5), (2, 2.0), (2, -1.25), (0, np.nan), (1, np.inf), (2, -np.inf),
             (2, np.nan)]
    for i in range(k):
        col, val = kinds[i % len(kinds)]
        p[i, col] = val
    return p


@functools.lru_cache(maxsize=None)
def scan_case(n, layout):
    rng = np.random.default_rng(1000 + n)
    ncell = 32 * 32 * 12
    if layout == "distinct":
        cells = rng.permutation(ncell)[np.arange(n) % ncell]                     # one cell per point while the grid allows
    else:
        new_at = sorted({0, n // 2, n - 1, 4095, 4096, 4097, 8191, 8192} & set(range(n)))
        fresh = rng.permutation(ncell)[:len(new_at)]
        cells = np.empty(n, np.int64)
        seen = 0
        for a, b in zip(new_at, new_at[1:] + [n]):                               # rows a+1 .. b-1 revisit cells seen so far
            seen += 1
            cells[a] = fresh[seen - 1]
            cells[a + 1:b] = fresh[rng.integers(0, seen, b - a - 1)]
    pts = _cell_points(rng, cells)
    out_at = np.nonzero((np.arange(n) % 7 == 3) & ~np.isin(np.arange(n), [0, n // 2, n - 1, 4095, 4096, 4097, 8191, 8192]))[0]
    pts[out_at] = _outside_rows(rng, len(out_at))                                # known positions: the flags are not all ones
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def cap_case(lead):
    """About 6000 occupied cells created in PAIRS of one column (ranks lead + 2k and lead + 2k + 1), after ``lead``
    solitary voxels; every 10th row is outside; 3000 revisits of random cells (cut ones included) follow."""
    rng = np.random.default_rng(77 + lead)
    pairs = []
    for col in range(lead, 1024):                                               # columns 0 .. lead-1 hold the solitary voxels
        z = rng.permutation(12)[:6]
        pairs += [(col + 1024 * z[0], col + 1024 * z[1]), (col + 1024 * z[2], col + 1024 * z[3]),
                  (col + 1024 * z[4], col + 1024 * z[5])]
    pairs = np.asarray(pairs)[rng.permutation(len(pairs))]
    cells = np.concatenate((np.arange(lead) + 1024 * 3, pairs.reshape(-1)))
    cells = np.concatenate((cells, cells[rng.integers(0, len(cells), 3000)]))
    pts = _cell_points(rng, cells)
    rows = np.insert(np.arange(len(pts)), np.arange(9, len(pts), 9), -1)         # -1 = an outside row
    full = _outside_rows(rng, len(rows))
    full[rows >= 0] = pts
    full.setflags(write=False)
    return full, len(np.unique(cells))


SEGMENTS = [1, 63, 64, 65, 127, 128, 129, 1000]


@functools.lru_cache(maxsize=None)
def selection_case():
    """16 cells: every segment length twice, the z maximum of the cell once on its FIRST row in file order (inside every
    kept prefix) and once on its LAST (outside whenever the segment is longer than max_points).  Row order shuffled.
    intensity = (1 + row) * 2^-12, elongation = (3 + 2 * row) * 2^-12: n = 3222 rows, so values < 1.6 (tanh slope >= 0.08,
    and one wrong row moves a mean by >= 2^-12 / 100 = 2.4e-6, more than 40 float32 ulps after tanh), and every sum of up
    to 100 of them is a multiple of 2^-12 below 256: 20 bits, exact in float32 in any order."""
    rng = np.random.default_rng(5)
    cell_ids = rng.permutation(32 * 32 * 12)[:2 * len(SEGMENTS)]
    cells = np.repeat(cell_ids, SEGMENTS + SEGMENTS)
    perm = rng.permutation(len(cells))
    cells = cells[perm]
    pts = _cell_points(rng, cells)
    cz = cells // 1024
    for j, cid in enumerate(cell_ids):
        rows = np.nonzero(cells == cid)[0]
        top = rows[0] if j < len(SEGMENTS) else rows[-1]
        pts[top, 2] = np.float32((cz[top] + 0.9375) * 0.25 + Z_SHIFT)            # above the jitter's 0.8, inside the cell
    row = np.arange(len(pts))
    pts[:, 3] = (1 + row) * 2.0 ** -12
    pts[:, 4] = (3 + 2 * row) * 2.0 ** -12
    pts.setflags(write=False)
    return pts, cell_ids


def general_cloud(n, seed, stride=5, rng_box=((-0.5, 8.5), (-4.5, 4.5), (-1.3, 2.3)), dense=None):
    """Uniform rows reaching over every face of the box, a clump of > max_points rows in a few cells, boundary rows."""
    rng = np.random.default_rng(seed)
    p = np.empty((n, stride), np.float32)
    for j in range(3):
        p[:, j] = rng.uniform(*rng_box[j], n)
    p[:, 3:] = rng.uniform(0, 3, (n, stride - 3))
    dense = n // 4 if dense is None else dense
    centre = [np.mean(b) for b in rng_box]
    p[:dense, :3] = rng.normal(centre, [0.2, 0.2, 0.15], (dense, 3))
    p[dense:dense + 10, 0] = rng_box[0][1] - 0.5                                 # x exactly on the upper face: dropped
    p[dense + 10:dense + 20, 2] = rng_box[2][0] + 0.3                            # z exactly on the lower face: kept
    return p[rng.permutation(n)]


def edge_points(rmin, vlen32, g, axis, z_shift, stride=4):
    """rmin + k * vsize in float32 for k = 0 .. g, each with its two float32 neighbours, along one axis; the other two
    coordinates sit mid-cell.  Returns (rows, k of every row)."""
    k = np.repeat(np.arange(g + 1), 3)
    e = np.float32(rmin[axis]) + k.astype(np.float32) * np.float32(vlen32)
    e = e.astype(np.float32)
    e[0::3] = np.nextafter(e[0::3], np.float32(-np.inf))
    e[2::3] = np.nextafter(e[2::3], np.float32(np.inf))
    p = np.zeros((len(k), stride), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = rmin[0] + 1.03, rmin[1] + 1.03, 0.6 + z_shift
    p[:, axis] = e
    p[:, 3:] = 1.0
    return p, k


# ---------------------------------------------------------------------------------------------------------------
# CPU: the reference against the oracle's literal loops, the scan restatement, the preconditions
# ---------------------------------------------------------------------------------------------------------------
def _lidar_cloud(n, seed):
    rng = np.random.default_rng(seed)
    pts = np.stack((rng.uniform(-2, 72, n), rng.uniform(-42, 42, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0, 3, n),
                    rng.uniform(0, 2, n)), 1).astype(np.float32)
    pts[:600, :3] = rng.normal([10.05, 0.05, -1.25], [0.01, 0.01, 0.05], (600, 3))         # voxels holding > 32 points
    pts[600:620, 0] = 70.0
    pts[620:640, 2] = -3.0
    return pts[rng.permutation(n)]


def _default_cfg(scale, max_voxels, elong):
    vlen = O.LIDAR_VOXEL_LEN / scale
    return dict(pc_range=[O.LIDAR_X_RANGE[0], O.LIDAR_Y_RANGE[0], 0.0, O.LIDAR_X_RANGE[1], O.LIDAR_Y_RANGE[1],
                          O.LIDAR_Z_RANGE[1] - O.LIDAR_Z_RANGE[0]],
                voxel_size=[vlen, vlen, O.LIDAR_VOXEL_HEIGHT], z_shift=O.LIDAR_Z_RANGE[0],
                max_points=O.LIDAR_MAX_PTS_PER_VOXEL, max_voxels=max_voxels, num_slices=O.LIDAR_NUM_SLICES,
                num_meta=O.LIDAR_NUM_META_CHANNEL, elong_col=4 if elong else -1)


def _assert_meta_within_bound(got, ref, num_slices, num_meta, what=""):
    """Channels num_slices+1 .. : |got - float64 reference| <= per-voxel float32-sum bound + half a float32 ulp."""
    for m in range(1, min(num_meta, 3)):
        g = got[..., num_slices + m].astype(np.float64)
        r64, r32 = ref.meta64[..., m - 1], ref.bev[..., num_slices + m]
        half_ulp = np.maximum(np.spacing(np.abs(r32)), np.spacing(np.abs(got[..., num_slices + m]))).astype(np.float64) / 2
        err = np.abs(g - r64)
        bar = ref.meta_bound[..., m - 1] + half_ulp + 2 * np.spacing(np.abs(r64))   # + two ulps of the double tanh itself
        worst = float((err / bar).max())
        print("VOX|%s|meta%d|err=%.3e|ratio=%.4f" % (what, m, float(err.max()), worst))
        assert worst <= 1.0, "%s meta channel %d: max err %.3e is %.3f of its per-voxel bar" % (what, m, err.max(), worst)


@pytest.mark.parametrize("scale,max_voxels,elong", [(0.5, 25000, True), (1.0, 700, True), (0.25, 25000, False)])
def test_ref_matches_oracle_get_lidar_blob(scale, max_voxels, elong):
    pts = _lidar_cloud(3000, seed=int(scale * 100) + max_voxels)
    _, blob = O.get_lidar_blob(pts, scale, elongation=elong, max_voxels=max_voxels)
    ref = ref_voxelize(pts, **_default_cfg(scale, max_voxels, elong))
    want = blob[0]
    assert ref.bev.shape == want.shape
    np.testing.assert_array_equal(ref.bev != 0, want != 0)
    np.testing.assert_array_equal(ref.bev[..., :13], want[..., :13])             # height slices + density
    _assert_meta_within_bound(want, ref, 12, 3, "oracle")
    assert want[..., 12].max() == 1.0                                            # a voxel with > 32 points exists
    if max_voxels == 700:
        assert ref.count > 700 and int((want[..., :12] != 0).sum()) <= 700       # the cap bites
    if not elong:
        assert (ref.bev[..., 14] == 0).all()


@pytest.mark.parametrize("max_points,max_voxels", [(1, 70), (5, 5), (70, 1), (5, 70), (70, 3000), (1, 1)])
def test_ref_matches_oracle_points_to_voxel(max_points, max_voxels):
    """Voxel order, coordinates, counts, kept rows and the padded maximum of z (range with zmin < 0: a FULL voxel of negative
    z has a negative maximum, one with padding has 0)."""
    pc_range, vs, zs = [0.0, -4.0, -1.0, 8.0, 4.0, 2.0], [0.5, 0.5, 0.25], 0.5
    pts = general_cloud(2000, seed=max_points * 131 + max_voxels, rng_box=((-0.5, 8.5), (-4.5, 4.5), (-0.8, 2.8)), dense=900)
    shifted = pts.copy()
    shifted[:, 2] -= np.float32(zs)
    voxels, coors, num = O.points_to_voxel(shifted, vs, pc_range, max_points, max_voxels)
    ref = ref_voxelize(pts, pc_range, vs, zs, max_points, max_voxels, 12, 3, 4)
    # the oracle's points_to_voxel has no filter_points; the range test on the raw z is the same predicate here because
    # (z - 0.5) - (-1) >= 0 <=> z >= -0.5 for these binary fractions
    V = len(num)
    assert V == min(ref.count, max_voxels) and V == len(ref.keep)
    np.testing.assert_array_equal(coors[:, ::-1], ref.coords)                    # zyx -> xyz, in voxel order
    np.testing.assert_array_equal(num, ref.keep)
    rows = np.where(ref.kept[..., None] >= 0, shifted[np.maximum(ref.kept, 0)], 0)
    np.testing.assert_array_equal(voxels, rows)
    np.testing.assert_array_equal(np.amax(voxels[:, :, 2], axis=1), ref.zmax)
    if max_points == 1 and max_voxels > 1:
        assert (ref.zmax < 0).any()


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_restatement_matches_cumsum(n):
    rng = np.random.default_rng(n)
    for a in (rng.integers(0, 2, n), rng.integers(0, 40, n), np.ones(n, np.int64)):
        out, total = scan_excl_restated(a)
        np.testing.assert_array_equal(out, np.cumsum(a) - a)
        assert total == a.sum()
    if n > TILE:                                                                 # the check has teeth: a carry from thread 1022
        bad, _ = scan_excl_restated(np.ones(n, np.int64), carry_thread=1022)
        assert not np.array_equal(bad, np.arange(n))


VLENS = {"0.1": 0.1, "0.2": 0.2, "0.3": 0.3, "third": 1.0 / 3.0}


def _edge_case(vlen):
    vs = [vlen, vlen, 0.25]
    gx, gy, _ = ref_grid(RANGE, vs)
    px, kx = edge_points(RANGE, np.float32(vlen), int(gx), 0, Z_SHIFT)
    py, ky = edge_points(RANGE, np.float32(vlen), int(gy), 1, Z_SHIFT)
    return np.concatenate((px, py)), np.concatenate((kx, ky)), np.concatenate((np.zeros(len(kx), int), np.ones(len(ky), int))), vs


@pytest.mark.parametrize("name", list(VLENS))
def test_edge_points_fall_on_both_sides(name):
    """The precondition of the cell-edge cases: among the rows placed ON rmin + k * vsize (float32), the division puts at
    least one into cell k and at least one into k - 1 (no voxel length here is representable, so the rounding of k * vsize and
    of the quotient decide); down-neighbours land in k - 1 and in k, up-neighbours in k.  And a reciprocal-multiply would move at
    least one of all the placed rows (otherwise the case could not tell it from the division)."""
    pts, k, axis, vs = _edge_case(VLENS[name])
    ok, t = ref_cells(pts, RANGE, vs, Z_SHIFT)
    c = t[np.arange(len(k)), axis].astype(np.int64)
    on, down, up = c[1::3] - k[1::3], c[0::3] - k[0::3], c[2::3] - k[2::3]
    print("VOX|edges|%s|on-edge rows in k-1: %d, in k: %d|down in k-1: %d of %d|up in k: %d of %d" % (
        name, int((on == -1).sum()), int((on == 0).sum()), int((down == -1).sum()), len(down), int((up == 0).sum()), len(up)))
    assert set(np.unique(on)) <= {-1, 0} and (on == 0).any()
    assert (down == -1).any() and (up == 0).any()                                # one row on each side of an edge
    assert (on == -1).any() and (down == 0).any()                                # the rounding of k * vsize decides edges
    ok_m, t_m = ref_cells(pts, RANGE, vs, Z_SHIFT, divide=False)
    moved = int(((t_m != t).any(1) | (ok_m != ok)).sum())
    print("VOX|edges|%s|rows a reciprocal-multiply moves: %d" % (name, moved))
    assert moved > 0


@pytest.mark.parametrize("h,zmax", [(0.4, 4.8), (0.3, 3.6)])
def test_float32_height_slices_would_differ(h, zmax):
    """The precondition of test_height_slices_are_the_float64_expression: at these heights zmax - (float)cz * (float)h in
    float32 is NOT the reference's float64 expression for many voxels, so equality there proves the double path."""
    pts = general_cloud(3000, 9, rng_box=((-0.5, 8.5), (-4.5, 4.5), (-1.3, zmax - 0.7)))
    ref = ref_voxelize(pts, **_cfg(pc_range=RANGE[:5] + [zmax], voxel_size=[0.25, 0.25, h]))
    assert ref.grid[2] == 12
    f32 = ref.zmax - ref.coords[:, 2].astype(np.float32) * np.float32(h)
    f64 = (ref.zmax.astype(np.float64) - ref.coords[:, 2] * h).astype(np.float32)
    differ = float((f32 != f64).mean())
    print("VOX|height %.1f|%.0f %% of %d slices differ between float32 and float64 arithmetic" % (h, 100 * differ, len(f32)))
    assert differ > 0.2
    assert sorted(np.unique(ref.coords[:, 2])) == list(range(12))


def _raw_call(lib, entry="frcnn_bev_voxelize_h", points=4096, n=100, stride=5, pc_range=RANGE, voxel=VOXEL, height=None,
              z_shift=Z_SHIFT, max_points=5, max_voxels=64, num_slices=SLICES, num_meta=3, elong=4, bev=4096, count=None,
              ws=4096, ws_bytes=None):
    """The C entry with made-up device addresses (never dereferenced on the host: every check precedes the first launch)."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    rng_, vs = _hip.float_array(pc_range), _hip.float_array(voxel)
    if ws_bytes is None:
        ws_bytes = lib.frcnn_bev_voxelize_ws_bytes(n, rng_, vs, max_voxels)
    head = (points, n, stride, rng_, vs)
    tail = (float(z_shift), max_points, max_voxels, num_slices, num_meta, elong, bev, count, ws, ws_bytes, None)
    if entry == "frcnn_bev_voxelize":
        return lib.frcnn_bev_voxelize(*head, *tail)
    return lib.frcnn_bev_voxelize_h(*head, float(voxel[2] if height is None else height), *tail)


@pytest.mark.parametrize("entry", ["frcnn_bev_voxelize_h", "frcnn_bev_voxelize"])
def test_argument_errors_are_reported_without_a_gpu(entry):
    from faster_rcnn_pytorch_multimodal_amd import _hip
    lib = _hip.load()
    assert lib.frcnn_version() >= 113
    call = functools.partial(_raw_call, lib, entry)
    need = lib.frcnn_bev_voxelize_ws_bytes(100, _hip.float_array(RANGE), _hip.float_array(VOXEL), 64)
    assert need > 0
    for kw, word in ((dict(num_meta=4), b"bad arguments"), (dict(elong=5), b"bad arguments"), (dict(elong=7), b"bad arguments"),
                     (dict(max_points=0), b"bad arguments"), (dict(max_voxels=0, ws_bytes=need), b"bad arguments"),
                     (dict(num_slices=11), b"12 z cells but 11 height slices"), (dict(stride=3), b"bad arguments"),
                     (dict(n=0, ws_bytes=need), b"bad arguments"), (dict(points=None), b"bad arguments"),
                     (dict(pc_range=[0, 0, 0, 0, 4, 3], ws_bytes=need), b"empty or oversized grid"),
                     (dict(voxel=[0.25, 0.0, 0.25], ws_bytes=need), b"empty or oversized grid")):
        assert call(**kw) == -1 and word in lib.frcnn_last_error(), (kw, lib.frcnn_last_error())
    assert call(ws_bytes=need - 1) != 0 and b"workspace" in lib.frcnn_last_error()
    assert call(ws=None) != 0 and b"workspace" in lib.frcnn_last_error()
    if entry == "frcnn_bev_voxelize_h":                                           # the double must be the one behind vsize[2]
        assert call(voxel=[0.25, 0.25, 0.4], height=0.5, pc_range=RANGE[:5] + [4.8]) == -1
        assert b"voxel_height" in lib.frcnn_last_error()
        assert call(voxel=[0.25, 0.25, 0.4], height=float(np.float32(0.4)), pc_range=RANGE[:5] + [4.8], ws=None) != 0
        assert b"workspace" in lib.frcnn_last_error()                             # accepted: it rounds to the same float32


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _run(points, cfg):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import ops
    dev = torch.from_numpy(np.array(points, dtype=np.float32)).to(DEV)           # a copy: the cached cases are read-only
    bev, count = ops.bev_voxelize(dev, cfg["pc_range"], cfg["voxel_size"], cfg["z_shift"], cfg["max_points"],
                                  cfg["max_voxels"], cfg["num_slices"], cfg["num_meta"], cfg["elong_col"])
    torch.cuda.synchronize()
    return bev.cpu().numpy(), int(count.item())


def _assert_matches(got, count, ref, cfg, what):
    S, M = cfg["num_slices"], cfg["num_meta"]
    assert got.shape == ref.bev.shape and got.shape[2] == S + M, (what, got.shape, ref.bev.shape)
    assert count == ref.count, (what, count, ref.count)
    np.testing.assert_array_equal(got != 0, ref.bev != 0, err_msg=what)
    np.testing.assert_array_equal(got[..., :S + min(M, 1)], ref.bev[..., :S + min(M, 1)], err_msg=what)   # exact, see docstring
    _assert_meta_within_bound(got, ref, S, M, what)


def _check(points, cfg, what):
    got, count = _run(points, cfg)
    ref = ref_voxelize(points, **cfg)
    _assert_matches(got, count, ref, cfg, what)
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["distinct", "late"])
@pytest.mark.parametrize("n", SCAN_N)
def test_scan_edges(hip, n, layout):
    pts = scan_case(n, layout)
    got, ref = _check(pts, CFG, "scan n=%d %s" % (n, layout))
    inside = int((ref.vox_of_point >= 0).sum())
    if layout == "distinct":
        assert ref.count >= inside - 1 and (n < 8 or inside < n)              # n = 12289 wraps round the grid once
    else:
        firsts = np.nonzero(np.r_[True, ref.vox_of_point[1:] > np.maximum.accumulate(ref.vox_of_point)[:-1]])[0]
        assert set(firsts) == {0, n // 2, n - 1, 4095, 4096, 4097, 8191, 8192} & set(range(n))


def _cap_values():
    return [1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097, "V-1", "V", "V+1"]


@pytest.mark.gpu
@pytest.mark.parametrize("mv", _cap_values())
def test_voxel_cap(hip, mv):
    lead = 0
    if isinstance(mv, int):
        lead = (mv + 1) % 2                                                      # ranks mv - 1 and mv are one column's pair
    pts, V = cap_case(lead)
    if mv == "V-1" and lead == 0 and V % 2 == 1:
        pts, V = cap_case(1)
    assert 5900 <= V <= 6300
    max_voxels = {"V-1": V - 1, "V": V, "V+1": V + 1}.get(mv, mv)
    cfg = _cfg(max_voxels=max_voxels, max_points=3)
    got, ref = _check(pts, cfg, "cap mv=%s" % mv)
    assert ref.count == V                                                        # the device count ignores the cap
    if max_voxels < V:
        gx, gy, _ = ref.grid
        kept_cell, cut_cell = ref.cells_by_rank[max_voxels - 1], ref.cells_by_rank[max_voxels]
        if max_voxels > 1 or lead == 0:
            assert kept_cell % (gx * gy) == cut_cell % (gx * gy) and kept_cell != cut_cell   # the cut is inside a column
            cx, cy = int(kept_cell % gx), int((kept_cell // gx) % gy)
            assert got[cy, cx, cut_cell // (gx * gy)] == 0                        # the cut slice stays empty
            assert got[cy, cx, kept_cell // (gx * gy)] != 0
            v = max_voxels - 1                                                   # the meta channels are the KEPT voxel's
            assert got[cy, cx, SLICES] == np.float32(ref.keep[v] / 3)
        cut_rows = np.isin(_linear_cells(pts), ref.cells_by_rank[max_voxels:]) & (_linear_cells(pts) >= 0)
        assert cut_rows.sum() > max(1, V - max_voxels) and (ref.vox_of_point[cut_rows] == -1).all()   # revisits of cut cells exist
        assert int((got[..., :SLICES] != 0).sum()) == max_voxels


def _linear_cells(pts, cfg=CFG):
    ok, t = ref_cells(pts, cfg["pc_range"], cfg["voxel_size"], cfg["z_shift"])
    gx, gy, _ = ref_grid(cfg["pc_range"], cfg["voxel_size"])
    c = np.where(ok[:, None], t, -1).astype(np.int64)
    return np.where(ok, (c[:, 2] * gy + c[:, 1]) * gx + c[:, 0], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("max_points", [1, 2, 5, 31, 32, 33, 64, 65, 100])
def test_selection(hip, max_points):
    pts, cell_ids = selection_case()
    cfg = _cfg(max_points=max_points, max_voxels=16)
    got, ref = _check(pts, cfg, "selection mp=%d" % max_points)
    assert ref.count == 16 and sorted(ref.npts) == sorted(SEGMENTS + SEGMENTS)
    assert (ref.meta_bound == 0).all() or max_points > 1
    # the sums are exact (selection_case), so the only freedom is the last place of tanh in double: one float32 ulp
    want = ref.bev[..., SLICES + 1:]
    ulps = np.abs(got[..., SLICES + 1:].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("VOX|selection mp=%d|tanh channels differ from float32(np.tanh(float64 mean)) by at most %d ulp" % (max_points, ulps.max()))
    assert ulps.max() <= 1
    # the z maximum: in the kept prefix for the first 8 cells, outside it for the others when the segment is longer
    gx, gy, _ = ref.grid
    for j, cid in enumerate(cell_ids):
        v = int(np.nonzero(ref.cells_by_rank == cid)[0][0])
        top = np.float32((cid // (gx * gy) + 0.9375) * 0.25)
        seen = j < len(SEGMENTS) or ref.npts[v] <= max_points
        assert (ref.zmax[v] == top) == seen, (j, ref.npts[v], ref.zmax[v])


PARAM_CASES = {
    "stride4": dict(stride=4, elong_col=-1),
    "stride5-elong4": dict(stride=5, elong_col=4),
    "stride7-elong6": dict(stride=7, elong_col=6),
    "stride7-elong4": dict(stride=7, elong_col=4),
    "stride7-none": dict(stride=7, elong_col=-1),
    "meta0": dict(num_meta=0), "meta1": dict(num_meta=1), "meta2": dict(num_meta=2), "meta3": dict(num_meta=3),
    "zshift-3": dict(z_shift=-3.0), "zshift0": dict(z_shift=0.0), "zshift1.5": dict(z_shift=1.5),
    "gz4-of-12": dict(pc_range=RANGE[:5] + [1.0]),
    "nonsquare": dict(voxel_size=[0.25, 0.5, 0.25]),
    "cap-bites": dict(max_voxels=257),
    "zmin-negative": dict(pc_range=[0.0, -4.0, -1.0, 8.0, 4.0, 2.0], z_shift=0.5, max_points=2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARAM_CASES))
def test_parameters(hip, name):
    kw = dict(PARAM_CASES[name])
    stride = kw.pop("stride", 5)
    cfg = _cfg(**dict(dict(max_points=32, max_voxels=5000), **kw))
    lo = cfg["pc_range"][2] + cfg["z_shift"]
    hi = cfg["pc_range"][5] + cfg["z_shift"]
    pts = general_cloud(3000, seed=sorted(PARAM_CASES).index(name), stride=stride,
                        rng_box=((-0.5, 8.5), (-4.5, 4.5), (lo - 0.3, hi + 0.3)))
    got, ref = _check(pts, cfg, name)
    assert ref.count > 500 and ref.keep.max() == 32 if name != "zmin-negative" else (ref.zmax < 0).any()
    if name == "gz4-of-12":
        assert ref.grid[2] == 4 and (got[..., 4:SLICES] == 0).all() and (got[..., :4] != 0).any()
    if name == "nonsquare":
        assert got.shape[:2] == (16, 32)
    if name == "cap-bites":
        assert ref.count > 257
    if cfg["elong_col"] < 0 and cfg["num_meta"] == 3:
        assert (got[..., SLICES + 2] == 0).all()
    if name == "stride7-elong6":                                                 # neither intensity nor column 4 is taken
        for col in (3, 4):
            other = ref_voxelize(pts, **_cfg(max_points=32, max_voxels=5000, elong_col=col))
            assert np.abs(other.bev[..., SLICES + 2] - got[..., SLICES + 2]).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VLENS))
def test_cell_edges_direct(hip, name):
    pts, k, axis, vs = _edge_case(VLENS[name])
    _check(pts, _cfg(voxel_size=vs, elong_col=-1, max_voxels=4096), "edges " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [0.25, 0.5, 1.0])
def test_cell_edges_through_get_lidar_blob(hip, scale):
    """Default configuration, every interior edge of x and y: get_lidar_blob -> ops.bev_voxelize against the reference and
    against the oracle's literal loops."""
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.minibatch import get_lidar_blob
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar"
    cfg = _default_cfg(scale, O.LIDAR_MAX_NUM_VOXEL, False)
    gx, gy, _ = ref_grid(cfg["pc_range"], cfg["voxel_size"])
    rmin = [O.LIDAR_X_RANGE[0], O.LIDAR_Y_RANGE[0], 0.0]
    px, _ = edge_points(rmin, np.float32(cfg["voxel_size"][0]), int(gx), 0, O.LIDAR_Z_RANGE[0])
    py, _ = edge_points(rmin, np.float32(cfg["voxel_size"][1]), int(gy), 1, O.LIDAR_Z_RANGE[0])
    pts = np.concatenate((px, py))
    infos, blob = get_lidar_blob(pts, scale, device=DEV)
    got = blob[0].cpu().numpy()
    ref = ref_voxelize(pts, **cfg)
    info_ref, want = O.get_lidar_blob(pts, scale)
    assert infos[0] == info_ref.tolist() and got.shape == (int(gy), int(gx), 15)
    _assert_matches(got, ref.count, ref, cfg, "blob edges scale %s" % scale)
    np.testing.assert_array_equal(got[..., :13], want[0][..., :13])
    C.reset_cfg()


def _degenerate(name):
    rng = np.random.default_rng(3)
    cell = 5 + 32 * 7 + 1024 * 4
    if name == "all-outside":
        return _outside_rows(rng, 300)
    if name == "one-point":
        return _cell_points(rng, [cell])
    if name == "one-cell":
        return _cell_points(rng, [cell] * 5000)
    if name == "nonfinite":                                                     # NaN / +-Inf rows between good ones
        p = _cell_points(rng, rng.permutation(32 * 32 * 12)[:400])
        for i, (col, val) in enumerate([(c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf)] * 8):
            p[3 + 5 * i, col] = val
        p[1, :3] = np.nan                                                        # an augmentation's dropped row
        return p
    if name == "negative-zero":                                                 # -0.0 on the lower x face and as raw z == fmin
        p = _cell_points(rng, [cell, cell + 1, cell + 2])
        p[0, 0] = -0.0
        p[1, 2] = np.float32(-1.0)
        return p
    if name == "negative-zero-z":                                               # z_shift 0: raw z = -0.0 on the lower face
        p = _cell_points(rng, [cell, cell, cell + 2], z_shift=0.0)
        p[:2, 2] = -0.0
        return p
    if name == "duplicates":
        p = _cell_points(rng, rng.permutation(32 * 32 * 12)[:50])
        return np.concatenate((p, p[::-1], p[:7], p))
    if name == "z-faces":                                                       # z exactly fmin (kept, slice 0) and fmax (dropped)
        p = _cell_points(rng, np.arange(20) * 33)
        p[:10, 2] = np.float32(-1.0)
        p[10:, 2] = np.float32(2.0)
        return p
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["all-outside", "one-point", "one-cell", "nonfinite", "negative-zero", "negative-zero-z",
                                  "duplicates", "z-faces"])
def test_degenerate(hip, name):
    pts = _degenerate(name)
    cfg = _cfg(z_shift=0.0) if name == "negative-zero-z" else CFG
    got, ref = _check(pts, cfg, name)
    expect = {"all-outside": 0, "one-point": 1, "one-cell": 1, "negative-zero": 3, "negative-zero-z": 2, "duplicates": 50,
              "z-faces": 10}
    if name in expect:
        assert ref.count == expect[name]
    if name == "all-outside":
        assert not got.any()
    if name == "nonfinite":
        assert np.isfinite(got).all() and 300 < ref.count < 400
    if name == "negative-zero":
        assert got[7, 0, 4] != 0                                                 # x = -0.0 sits in cell 0


@pytest.mark.gpu
def test_second_grid_stride_trip(hip):
    """1 048 576 + 300 rows of 4 floats: the point kernels take a second trip of their stride loop, the first scan walks 257
    tiles.  About 1900 cells are filled by the first trip's rows; 100 cells appear only beyond row 1 048 576."""
    rng = np.random.default_rng(11)
    n = GRID_TRIP + 300
    ids = rng.permutation(32 * 32 * 12)[:2000]
    cells = np.concatenate((ids[rng.integers(0, 1900, GRID_TRIP)], ids[rng.integers(1800, 2000, 300)]))
    pts = _cell_points(rng, cells, stride=4)
    pts[::1001] = _outside_rows(rng, len(pts[::1001]), stride=4)
    got, ref = _check(pts, _cfg(max_points=32, max_voxels=3000, elong_col=-1), "second trip")
    first_row = np.full(ref.count, n)
    np.minimum.at(first_row, ref.vox_of_point[ref.vox_of_point >= 0], np.nonzero(ref.vox_of_point >= 0)[0])
    assert 1950 <= ref.count <= 2000 and int((first_row >= GRID_TRIP).sum()) >= 50


@pytest.mark.gpu
def test_determinism(hip):
    """Three runs into fresh outputs: the design claims independence from the order in which the atomics land."""
    pts = general_cloud(8193, seed=4, dense=5000)
    cfg = _cfg(max_points=32, max_voxels=700)
    runs = [_run(pts, cfg) for _ in range(3)]
    ref = ref_voxelize(pts, **cfg)
    assert ref.count > 700 and ref.keep.max() == 32
    for got, count in runs[1:]:
        assert count == runs[0][1] and got.tobytes() == runs[0][0].tobytes()
    _assert_matches(runs[0][0], runs[0][1], ref, cfg, "determinism")


@pytest.mark.gpu
@pytest.mark.parametrize("h,zmax", [(0.4, 4.8), (0.3, 3.6)])
def test_height_slices_are_the_float64_expression(hip, h, zmax):
    """Voxel heights at which cz * h is not exact: the slices still equal the reference's float64 expression bit for bit
    (test_float32_height_slices_would_differ shows a float32 evaluation could not)."""
    pts = general_cloud(3000, 9, rng_box=((-0.5, 8.5), (-4.5, 4.5), (-1.3, zmax - 0.7)))
    _check(pts, _cfg(pc_range=RANGE[:5] + [zmax], voxel_size=[0.25, 0.25, h], max_points=32), "height %.1f" % h)


@pytest.mark.gpu
def test_default_configuration_is_unchanged(hip):
    """Default configuration (height 0.5): get_lidar_blob equals the oracle's literal loops exactly in the slices and the
    density, as before the double voxel height; and the float-only entry frcnn_bev_voxelize gives the same bits."""
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.minibatch import get_lidar_blob
    C.reset_cfg()
    C.cfg.NET_TYPE = "lidar"
    pts = _lidar_cloud(3000, seed=21)
    _, want = O.get_lidar_blob(pts, 0.5, elongation=True)
    _, blob = get_lidar_blob(pts, 0.5, device=DEV, elongation=4)
    got = blob[0].cpu().numpy()
    cfg = _default_cfg(0.5, O.LIDAR_MAX_NUM_VOXEL, True)
    ref = ref_voxelize(pts, **cfg)
    np.testing.assert_array_equal(got[..., :13], want[0][..., :13])
    _assert_matches(got, ref.count, ref, cfg, "default")
    dev = torch.from_numpy(pts).to(DEV)
    rng_, vs = _hip.float_array(cfg["pc_range"]), _hip.float_array(cfg["voxel_size"])
    nbytes = hip.frcnn_bev_voxelize_ws_bytes(len(pts), rng_, vs, cfg["max_voxels"])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    old = torch.empty(got.shape, dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = _raw_call(hip, "frcnn_bev_voxelize", dev.data_ptr(), len(pts), 5, cfg["pc_range"], cfg["voxel_size"], None,
                   cfg["z_shift"], cfg["max_points"], cfg["max_voxels"], 12, 3, 4, old.data_ptr(), count.data_ptr(),
                   ws.data_ptr(), nbytes)
    assert rc == 0, hip.frcnn_last_error()
    torch.cuda.synchronize()
    assert old.cpu().numpy().tobytes() == got.tobytes() and int(count.item()) == ref.count
    C.reset_cfg()


@pytest.mark.gpu
def test_bad_arguments_raise_without_launching(hip):
    import torch
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    pts = torch.from_numpy(general_cloud(100, 1)).to(DEV)
    good = dict(pc_range=RANGE, voxel_size=VOXEL, z_shift=Z_SHIFT, max_points=5, max_voxels=64, num_slices=SLICES,
                num_meta=3, elongation_col=4)
    for kw, word in ((dict(num_meta=4), "bad arguments"), (dict(elongation_col=5), "bad arguments"),
                     (dict(max_points=0), "bad arguments"), (dict(max_voxels=0), "bad arguments"), (dict(num_slices=11), "z cells"),
                     (dict(pc_range=[0, 0, 0, 0, 4, 3]), "empty or oversized grid")):
        with pytest.raises(_hip.HipError, match=word):
            ops.bev_voxelize(pts, **dict(good, **kw))
    need = hip.frcnn_bev_voxelize_ws_bytes(100, _hip.float_array(RANGE), _hip.float_array(VOXEL), 64)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    bev = torch.full((32, 32, 15), 7.0, device=DEV)
    rc = _raw_call(hip, points=pts.data_ptr(), bev=bev.data_ptr(), ws=ws.data_ptr(), ws_bytes=need - 1)
    assert rc != 0 and b"workspace" in hip.frcnn_last_error()
    torch.cuda.synchronize()
    assert (bev == 7.0).all()                                                    # nothing ran
    got, count = ops.bev_voxelize(pts, **good)                                   # and the library still works afterwards
    assert int(count.item()) == ref_voxelize(pts.cpu().numpy(), RANGE, VOXEL, Z_SHIFT, 5, 64, SLICES, 3, 4).count
