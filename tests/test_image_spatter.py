"""Test-time Spatter corruption of camera frames (lib/roi_data_layer/minibatch.py:648-664, cfg.TEST.AUGMENT_EN): the record
and the gate on the host (``roi_data_layer/image_augment.py``, ``roi_data_layer/minibatch.py``), the pixels on the device
(``frcnn_image_spatter``) against a float64 numpy restatement kept in this file.  imgaug / imagecorruptions / scikit-image
are not available, so the operator is PARITY UNPINNED: the restatement follows the conventions listed in
``csrc/image_spatter.hip``; the draws are replayed with the oracle's ``uniform01``.

The operator holds two thresholds (``liquid > thr`` and ``m >= 0.8``), so a direct comparison of the bytes is ill-posed: a
value within rounding of a threshold may fall either way, and one flipped decision moves the mask of its neighbourhood.
The GPU comparison therefore replays the DEVICE's decisions: the field against float64 everywhere, the first decision
wherever the float64 field is clear of the threshold, the mask against the float64 blur of the device's decision, the
second decision likewise, and the bytes against floor(v) of the float64 blend under the device's two decisions.  Bands:
  * field, atol 1e-5: the draw term is tests/test_image_augment.py's T_NOISE = 1.5e-4 at scale 25.5, scaled to 0.4
    (2.4e-6), plus 18 fp32 multiply-adds on values up to about 3 (3e-6);
  * mask, atol 4e-6: 26 fp32 multiply-adds on values up to 1;
  * decisions: either answer stands within 1e-5 of the threshold;
  * bytes: exact where v is more than 1e-3 from an integer, +-1 within (255 x (1.6e-6 + three roundings) = 5e-4);
    pixels with m = 0 equal the input bit for bit.
Conditions on the cases (asserted on the CPU in ``test_restatement_cases_are_well_posed``, so that a band test which leaves
everything out cannot pass): each decision band holds at most 0.5 % of the pixels and at least 5 % of them are mud.
"""
import functools

import numpy as np
import pytest
import torch

from faster_rcnn_pytorch_multimodal_amd import _hip, ops
from faster_rcnn_pytorch_multimodal_amd.model import config as C
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import image_augment as IA
from faster_rcnn_pytorch_multimodal_amd.roi_data_layer.image_augment import (Spatter, draw_test_corruption, spatter_params,
                                                                             spatter_taps)
from oracle import frcnn_oracle as O

DEV = "cuda:0"
T_FIELD, T_MASK, T_DECISION, T_BYTE = 1e-5, 4e-6, 1e-5, 1e-3
MAX_BAND_SHARE, MIN_MUD_SHARE = 0.005, 0.05
FULL = (1280, 1920)
# (shape, severity, seed).  (7, 9): the whole frame is smaller than the combined halo of 10; (16, 64) / (17, 65): one
# 64x16 tile of the stencil stages and one pixel past it; (32, 64) / (33, 65): the same for this kernel's own 64x32 tile;
# (97, 131): odd sizes, several tiles, a width that is no multiple of 4; severity 4 once.
CASES = [((7, 9), 5, 11), ((16, 64), 5, 12), ((17, 65), 5, 13), ((32, 64), 5, 11), ((33, 65), 5, 12), ((97, 131), 5, 13),
         ((37, 53), 4, 12)]
FULL_CASE = (FULL, 5, 11)
CUT = np.float64(np.float32(IA.SPATTER_MASK_CUT))
COLOUR = np.array([np.float32(c) for c in IA.SPATTER_MUD_COLOUR], np.float64)


@pytest.fixture(autouse=True)
def _fresh_cfg():
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    IA.set_augmentation_rng(None)
    yield
    IA.set_augmentation_rng(None)
    C.reset_cfg()


# ---------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------
def _frame(shape, seed=0):
    """Noise with constant regions, a one-pixel checkerboard and saturated (0 / 255) patches, some on the border."""
    h, w = shape
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    im[: h // 4, : w // 3] = (90, 140, 30)
    im[h // 2: h // 2 + h // 5, w // 2:] = 128
    yy, xx = np.mgrid[0: h // 3, 0: w // 4]
    im[h - h // 3:, : w // 4] = (((yy + xx) % 2) * 255).astype(np.uint8)[..., None]
    im[h // 3: h // 3 + 9, w // 3: w // 3 + 11] = 255
    im[: max(h // 14, 1), w - max(w // 14, 1):] = 0
    im[h - max(h // 19, 1):, w - max(w // 21, 1):] = 255
    im[h // 4: h // 4 + 6, : max(w // 26, 1)] = (255, 0, 255)
    return np.ascontiguousarray(im)


def _blur64(a, taps):
    """Separable Gaussian in float64 with the float32 taps the device receives, border replicate."""
    t = np.asarray(taps, np.float32).astype(np.float64)
    r, (h, w) = len(t) // 2, a.shape
    p = np.pad(np.asarray(a, np.float64), ((r, r), (r, r)), mode='edge')
    acc = sum(t[k] * p[:, k:k + w] for k in range(len(t)))
    return sum(t[k] * acc[k:k + h] for k in range(len(t)))


def _field64(shape, severity, seed):
    """Step 1 in float64: loc + scale * normal01, the device's Box-Muller expression in double on the replayed uniforms."""
    h, w = shape
    loc, scale = (np.float64(np.float32(v)) for v in spatter_params(severity)[:2])
    k, idx = ops.AUG_STREAM['image_spatter'], np.arange(h * w)
    u1 = O.uniform01(seed, 2 * k, idx).astype(np.float64)
    u2 = O.uniform01(seed, 2 * k + 1, idx).astype(np.float64)
    two_pi = np.float64(np.float32(6.2831853071795864))
    return (loc + scale * (np.sqrt(-2.0 * np.log(u1)) * np.cos(two_pi * u2))).reshape(h, w)


@functools.lru_cache(maxsize=None)
def _liquid64(shape, severity, seed):
    """Steps 1-2: the field after the first blur.  Computed once per case and shared; never modified."""
    out = _blur64(_field64(shape, severity, seed), spatter_taps(spatter_params(severity)[2]))
    out.setflags(write=False)
    return out


def _thr(severity):
    return np.float64(np.float32(spatter_params(severity)[3]))


def _mask64(decision, severity):
    """Step 4 before the cut: the float64 blur of a first decision."""
    return _blur64(decision.astype(np.float64), spatter_taps(spatter_params(severity)[4]))


def _blend64(img, m):
    """Step 5 before the truncation, m already cut."""
    x = img.astype(np.float64) / 255.0
    return np.clip(x * (1.0 - m[..., None]) + COLOUR * m[..., None], 0.0, 1.0) * 255.0


def _shares(shape, severity, seed):
    """(share in the first decision band, share in the second, share of mud, share in the +-1 band among the mud) of the
    restatement under its own decisions."""
    liquid = _liquid64(shape, severity, seed)
    thr = _thr(severity)
    m = _mask64(liquid > thr, severity)
    mud = m >= CUT
    v = _blend64(_frame(shape, seed), np.where(mud, m, 0.0))
    near = (np.abs(v - np.rint(v)) <= T_BYTE) & mud[..., None]
    return (float((np.abs(liquid - thr) <= T_DECISION).mean()), float((np.abs(m - CUT) <= T_DECISION).mean()),
            float(mud.mean()), float(near.mean()))


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_restatement_cases_are_well_posed():
    """The conditions of the GPU comparison, asserted for every case it uses."""
    for shape, severity, seed in CASES + [FULL_CASE]:
        band1, band2, mud, near = _shares(shape, severity, seed)
        print("%s severity %d seed %d: decision bands %.4f %% / %.4f %%, mud %.1f %%, +-1 band %.2f %%"
              % (shape, severity, seed, 100 * band1, 100 * band2, 100 * mud, 100 * near))
        assert band1 <= MAX_BAND_SHARE and band2 <= MAX_BAND_SHARE, (shape, severity, seed, band1, band2)
        assert mud >= MIN_MUD_SHARE, (shape, severity, seed, mud)
    # the restatement itself: a constant field stays constant under both blurs, the field has the moments asked for
    flat = np.full((9, 11), 0.25)
    np.testing.assert_allclose(_blur64(flat, spatter_taps(1.5)), flat, atol=1e-7)
    field = _field64((97, 131), 5, 11)
    assert abs(field.mean() - 0.67) < 0.02 and abs(field.std() - 0.4) < 0.02
    # px / 255 * 255 truncates back to px: an untouched pixel (m = 0) leaves as it came
    px = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    np.testing.assert_array_equal(np.floor(_blend64(px, np.zeros((1, 256)))), px)
    f32 = (np.arange(256, dtype=np.float32) / np.float32(255)) * np.float32(255)
    np.testing.assert_array_equal(f32.astype(np.uint8), np.arange(256))


def test_taps_parameters_and_switches():
    for sigma, size in ((1.0, 9), (1.5, 13)):
        taps = spatter_taps(sigma)
        assert taps.dtype == np.float32 and len(taps) == size and abs(float(taps.astype(np.float64).sum()) - 1) < 1e-6
        np.testing.assert_array_equal(taps, taps[::-1])
        x = np.arange(size) - size // 2
        np.testing.assert_allclose(taps[1:] / taps[:-1], np.exp(-(x[1:] ** 2 - x[:-1] ** 2) / (2 * sigma ** 2)), rtol=1e-5)
    assert (len(spatter_taps(1.0)), len(spatter_taps(1.5))) == ops.SPATTER_MAX_TAPS
    assert spatter_params(5) == (0.67, 0.4, 1.0, 0.65, 1.5) and spatter_params(4) == (0.65, 0.3, 1.0, 0.65, 1.5)
    assert IA.SPATTER_MUD_COLOUR == (63 / 255.0, 42 / 255.0, 20 / 255.0) and IA.SPATTER_MASK_CUT == 0.8
    for severity in (1, 2, 3):
        with pytest.raises(NotImplementedError, match="severity %d" % severity):
            spatter_params(severity)
        with pytest.raises(NotImplementedError, match="severity %d" % severity):
            ops.image_spatter(torch.zeros(8, 8, 3, dtype=torch.uint8), Spatter(severity=severity))
    with pytest.raises(ValueError):
        spatter_params(6)
    assert ops.AUG_STREAM['image_spatter'] == 44
    assert len(set(ops.AUG_STREAM.values())) == len(ops.AUG_STREAM)
    uniform = {86, 72, 73}                       # the streams read as uniform01; a normal01 stream k reads 2k and 2k + 1
    normal = set(ops.AUG_STREAM.values()) - uniform
    assert not ({2 * k for k in normal} | {2 * k + 1 for k in normal}) & uniform
    cfg = C.cfg.IMAGE
    assert cfg.EN_TEST_SPATTER is False and cfg.TEST_SPATTER_SEVERITY == 5
    C.cfg_from_list(['IMAGE.EN_TEST_SPATTER', 'True', 'IMAGE.TEST_SPATTER_SEVERITY', '4'])
    assert cfg.EN_TEST_SPATTER is True and cfg.TEST_SPATTER_SEVERITY == 4


def test_draw_test_corruption():
    a = [draw_test_corruption(np.random.default_rng(4)) for _ in range(2)]
    assert a[0] == a[1] and a[0].severity == 5 and 0 <= a[0].seed < 2 ** 32
    IA.set_augmentation_rng(np.random.default_rng(4))
    first, second = draw_test_corruption(), draw_test_corruption()
    assert first == a[0] and second != first                                         # the installed generator advances
    IA.set_augmentation_rng(np.random.default_rng(4))
    assert draw_test_corruption(key="ignored/under/a/generator.png") == a[0]
    IA.set_augmentation_rng(None)
    # without a generator: the frame's name and cfg.RNG_SEED, nothing else
    b = draw_test_corruption(key="val/000017.png")
    assert b == draw_test_corruption(key="val/000017.png") and b.seed != draw_test_corruption(key="val/000018.png").seed
    C.cfg.RNG_SEED = 4
    assert draw_test_corruption(key="val/000017.png").seed != b.seed
    C.cfg.RNG_SEED = 3
    assert draw_test_corruption(key="val/000017.png") == b
    assert len({draw_test_corruption().seed for _ in range(12)}) > 1                 # no key either: fresh entropy
    C.cfg.IMAGE.TEST_SPATTER_SEVERITY = 4
    assert draw_test_corruption(key="x").severity == 4
    C.cfg.IMAGE.TEST_SPATTER_SEVERITY = 2
    with pytest.raises(NotImplementedError, match="severity 2"):
        draw_test_corruption(key="x")


def test_gate_names_the_switch_and_opens(tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.model import test as model_test
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    path = str(tmp_path / "frame.npy")
    np.save(path, _frame((32, 48)))
    with pytest.raises(NotImplementedError, match="Spatter") as err:
        minibatch._get_image_blob([path], 1.0, augment_en=True, mode='test', device='cpu')
    assert "cfg.IMAGE.EN_TEST_SPATTER" in str(err.value)
    C.cfg.TEST.AUGMENT_EN = True
    with pytest.raises(NotImplementedError, match="EN_TEST_SPATTER"):
        model_test._get_blobs([path])                                                # what test_net calls per frame
    C.cfg.IMAGE.EN_TEST_SPATTER = True
    with pytest.raises(_hip.HipError, match="no CPU path"):                          # past the gate: the device operator
        minibatch._get_image_blob([path], 1.0, augment_en=True, mode='test', device='cpu')
    # the training gate does not move with the new switch
    entry = {"filename": path, "boxes": np.zeros((1, 4), np.float32), "gt_classes": np.ones(1, np.int64),
             "ignore": np.zeros(1, np.int64), "flipped": False}
    with pytest.raises(NotImplementedError, match=r"cfg\.IMAGE\.EN_AUG"):
        minibatch._get_image_blob([entry], 1.0, augment_en=True, device='cpu')


def test_image_spatter_argument_errors_are_reported_without_a_gpu():
    lib = _hip.load()
    assert lib.frcnn_version() >= 116
    h, w = 48, 64
    img, out = 1 << 20, 2 << 20                                  # non-null device addresses: never dereferenced on the host
    good = dict(img=img, h=h, w=w, params=list(spatter_params(5)), taps1=list(spatter_taps(1.0)), taps2=list(spatter_taps(1.5)),
                out=out)

    def call(**kw):
        a = dict(good, **kw)
        arr = lambda v: None if v is None else _hip.float_array(v)
        n1 = a.get('n1', 0 if a['taps1'] is None else len(a['taps1']))
        n2 = a.get('n2', 0 if a['taps2'] is None else len(a['taps2']))
        return lib.frcnn_image_spatter(a['img'], a['h'], a['w'], arr(a['params']), arr(a['taps1']), n1, arr(a['taps2']), n2, 1,
                                       None, a['out'], None, None, None)

    for kw in (dict(img=None), dict(out=None), dict(params=None), dict(taps1=None, n1=9), dict(taps2=None, n2=13)):
        assert call(**kw) == -1 and b"null" in lib.frcnn_last_error(), kw
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(w=-1)):
        assert call(**kw) == -1 and b"frame size" in lib.frcnn_last_error(), kw
    assert call(out=img) == -1 and b"overlap" in lib.frcnn_last_error()
    assert call(out=img + 100) == -1 and b"overlap" in lib.frcnn_last_error()
    # more taps than the halo holds, an even count, a count off the radius rule
    p = list(spatter_params(5))
    assert call(taps1=list(spatter_taps(1.5)), params=p[:2] + [1.5] + p[3:]) == -1 and b"holds" in lib.frcnn_last_error()
    assert call(taps2=list(spatter_taps(2.0)), params=p[:4] + [2.0]) == -1 and b"holds" in lib.frcnn_last_error()
    assert call(taps1=[0.125] * 8) == -1 and call(taps2=[0.25] * 4) == -1
    assert call(taps1=list(spatter_taps(0.5))) == -1 and b"radius rule" in lib.frcnn_last_error()
    assert call(params=[float("nan")] + p[1:]) == -1 and b"non-finite" in lib.frcnn_last_error()
    assert call(params=[p[0], -0.1] + p[2:]) == -1
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.image_spatter(torch.zeros(8, 8, 3, dtype=torch.uint8), Spatter())


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _run(img, rec, debug=False, **kw):
    dev = torch.from_numpy(img).to(DEV)
    if debug:
        kw["debug_liquid"] = torch.full(img.shape[:2], float("nan"), dtype=torch.float32, device=DEV)
        kw["debug_mask"] = torch.full(img.shape[:2], float("nan"), dtype=torch.float32, device=DEV)
    out = ops.image_spatter(dev, rec, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), torch.from_numpy(img))                            # the input is not touched
    if debug:
        return out.cpu().numpy(), kw["debug_liquid"].cpu().numpy(), kw["debug_mask"].cpu().numpy()
    return out.cpu().numpy()


def _check_against_restatement(shape, severity, seed):
    what = "%s severity %d seed %d" % (shape, severity, seed)
    im = _frame(shape, seed)
    got, liquid_dev, mask_dev = _run(im, Spatter(severity, seed), debug=True)
    assert np.array_equal(got, _run(im, Spatter(severity, seed))), what              # the debug outputs change nothing
    # 1. the field
    liquid = _liquid64(shape, severity, seed)
    err1 = float(np.abs(liquid_dev.astype(np.float64) - liquid).max())
    # 2. the first decision
    thr = _thr(severity)
    b_dev = liquid_dev > np.float32(thr)
    clear1 = np.abs(liquid - thr) > T_DECISION
    # 3. the mask, from the device's decision
    m = _mask64(b_dev, severity)
    err3 = float(np.abs(mask_dev.astype(np.float64) - m).max())
    # 4. the second decision
    mud_dev = mask_dev >= np.float32(CUT)
    clear2 = np.abs(m - CUT) > T_DECISION
    # 5. the bytes, under the device's two decisions
    v = _blend64(im, np.where(mud_dev, m, 0.0))
    want = np.floor(v)
    diff = got.astype(np.int64) - want.astype(np.int64)
    clear5 = np.abs(v - np.rint(v)) > T_BYTE
    print("%s: field err %.3g (T %.3g), mask err %.3g (T %.3g), decision bands %.4f %% / %.4f %%, mud %.1f %%, bytes off by "
          "one inside the +-1 band %d of %d" % (what, err1, T_FIELD, err3, T_MASK, 100 * (1 - clear1.mean()),
                                                 100 * (1 - clear2.mean()), 100 * mud_dev.mean(), int((diff != 0).sum()),
                                                 int((~clear5).sum())))
    assert np.isfinite(liquid_dev).all() and np.isfinite(mask_dev).all(), what      # every in-frame position was written
    assert err1 <= T_FIELD, what
    assert 1 - clear1.mean() <= MAX_BAND_SHARE, what
    assert np.array_equal(b_dev[clear1], (liquid > thr)[clear1]), what
    assert err3 <= T_MASK, what
    assert 1 - clear2.mean() <= MAX_BAND_SHARE, what
    assert np.array_equal(mud_dev[clear2], (m >= CUT)[clear2]), what
    assert mud_dev.mean() >= MIN_MUD_SHARE, what
    assert (diff[clear5] == 0).all(), "%s: %d bytes differ outside the band" % (what, int((diff[clear5] != 0).sum()))
    assert (np.abs(diff) <= 1).all(), what
    assert np.array_equal(got[~mud_dev], im[~mud_dev]), what                         # m = 0: bit for bit the input
    assert (got[mud_dev] != im[mud_dev]).mean() > 0.5, what                          # and the mud is there
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-s%d-seed%d" % (c[0] + c[1:]))
def test_spatter_matches_the_float64_restatement(hip, case):
    _check_against_restatement(*case)


@pytest.mark.gpu
def test_spatter_full_frame(hip):
    """1280 x 1920: grid and index arithmetic at the workload's size, steps 1-5 against the restatement."""
    _check_against_restatement(*FULL_CASE)


@pytest.mark.gpu
def test_spatter_is_a_pure_function_of_pixels_severity_and_seed(hip):
    shape = (97, 131)
    im = _frame(shape, 3)
    rec = Spatter(5, 13)
    first = _run(im, rec)
    assert np.array_equal(first, _run(im, rec))                                      # the same record twice
    other = _run(im, Spatter(5, 14))
    assert (other != first).mean() > 0.05                                            # another seed: other mud
    assert (_run(im, Spatter(4, 13)) != first).any()                                 # another severity
    word = torch.tensor([40], dtype=torch.int32, device=DEV)
    assert np.array_equal(_run(im, Spatter(5, 13 - 40), seed_dev=word), first)       # seed + word
    assert np.array_equal(_run(im, Spatter(5, 2 ** 32 - 1), seed_dev=torch.tensor([14], dtype=torch.int32, device=DEV)), first)
    # caller-owned output; aliasing is rejected, as the header says
    dev = torch.from_numpy(im).to(DEV)
    out = torch.zeros_like(dev)
    assert ops.image_spatter(dev, rec, out=out) is out and np.array_equal(out.cpu().numpy(), first)
    with pytest.raises(_hip.HipError, match="overlap"):
        ops.image_spatter(dev, rec, out=dev)
    assert torch.equal(dev.cpu(), torch.from_numpy(im))
    for severity in (1, 2, 3):
        with pytest.raises(NotImplementedError, match="severity %d" % severity):
            ops.image_spatter(dev, Spatter(severity, 13))
    with pytest.raises(_hip.HipError, match="uint8"):
        ops.image_spatter(dev.float(), rec)
    with pytest.raises(_hip.HipError, match="debug_mask"):
        ops.image_spatter(dev, rec, debug_mask=torch.zeros(5, dtype=torch.float32, device=DEV))


@pytest.mark.gpu
def test_get_image_blob_corrupts_the_test_frame(hip, tmp_path):
    from faster_rcnn_pytorch_multimodal_amd.model import test as model_test
    from faster_rcnn_pytorch_multimodal_amd.roi_data_layer import minibatch
    from faster_rcnn_pytorch_multimodal_amd.utils.blob import prep_im_for_blob
    cfg = C.cfg
    im = _frame((97, 131), 6)
    path = str(tmp_path / "frame.npy")
    np.save(path, im)
    plain_infos, plain, _ = minibatch._get_image_blob([path], 1.0, augment_en=False, mode='test')
    with pytest.raises(NotImplementedError, match="Spatter"):
        minibatch._get_image_blob([path], 1.0, augment_en=True, mode='test')
    cfg.IMAGE.EN_TEST_SPATTER = True
    infos, blob, local = minibatch._get_image_blob([path], 1.0, augment_en=True, mode='test')
    frame = ops.image_spatter(torch.from_numpy(im).to(DEV), draw_test_corruption(key=path))
    want = prep_im_for_blob(frame, cfg.PIXEL_MEANS, cfg.PIXEL_STDDEVS, cfg.PIXEL_ARRANGE, 1.0, device=DEV).unsqueeze(0)
    assert torch.equal(blob, want) and blob.is_cuda and local is None
    np.testing.assert_array_equal(infos[0], plain_infos[0])
    assert blob.shape == plain.shape and not torch.equal(blob, plain)
    # two runs with the same cfg.RNG_SEED feed the same blob, through the call test_net makes per frame
    cfg.TEST.AUGMENT_EN = True
    again = model_test._get_blobs([path])
    assert torch.equal(again['data'], blob)
    np.testing.assert_array_equal(again['info'], plain_infos[0])
    cfg.RNG_SEED = 4
    assert not torch.equal(model_test._get_blobs([path])['data'], blob)
    # every other combination is unchanged: no corruption without augment_en, whatever the switch says
    cfg.TEST.AUGMENT_EN = False
    assert torch.equal(model_test._get_blobs([path])['data'], plain)
