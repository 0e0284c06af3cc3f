"""The bf16-operand and split-bf16 forward convolutions (conv_igemm_bf16 in conv_igemm.hip, entry points in conv_bf16.hip)
through ``ops``, bit for bit against float64 on the host, with every operand and the output between guard bands.

Method (that of test_conv_f32_exact.py).  Operands are integers held in fp32, chosen per REGIME so that every bf16 plane
holds its part exactly and every partial sum, in any order, stays below 2^24: the float64 convolution on the host IS the
fp32 answer, on either tile, at any depth of the staging ring.  The comparison is equality.  Each regime's precondition
- plane occupancy, the three dropped products zero, sum |x||w| < 2^24, the epilogue's result below 2^23 - is asserted on
the host by tests that need no GPU, together with an exact emulation of the six-product sum with one term left out, which
shows what each regime pins:

    regime  x                              w                              the product it pins       reduction
    R1      ints in [-3, 3]                ints in [-3, 3]                hi*hi, the one-plane form  dense
    R2      odd, 256 <= |x| < 512          ints in [-2, 2]                (mid, hi)                  dense
    R3      ints in [-2, 2]                odd, 256 <= |w| < 512          (hi, mid)                  dense
    R4      odd, 256 <= |x| < 512          odd, 256 <= |w| < 512          (mid, mid)                 window
    R5      odd, 2^17 <= |x| < 2^17+2^16   ints in {-1, 0, 1}             (lo, hi)                   window
    R6      ints in {-1, 0, 1}             odd, 2^17 <= |w| < 2^17+2^16   (hi, lo)                   window

"window": the products vanish outside 64 consecutive indices of the reduction axis in (r, s, c) order, placed across the
last two K-steps (``window_of``), so that the mid and lo planes travel through the last stages of the ring.  The filter has
that axis and is zeroed outside the window (R4, R6, and R5 on a filter larger than 1x1); a 1x1 layer's activations have it
too, and there R5 zeroes the activations instead, as its large operand.

Buffers.  y is a view between two NaN bands of BAND floats, filled with NaN before the call; x, residual, scale and shift
sit between NaN bands, the packed filter between bands of the bf16 NaN word 0x7FC0.  After the call: bands intact, no NaN
in y (an element never written, or a consumed read outside an operand), y == float64.

Kernel reached by (form, forced tile) - launch_bf16 in conv_igemm.hip; the steady loop runs while s + 2 DEPTH < nsteps:

    form        tile (set_conv_bf16_tile)   DEPTH   steady loop entered from   prologue loads   store path
    one plane   1: 64x64                    4       9 K-steps                  min(nsteps, 5)   K % 4 == 0: LDS transpose (default)
    one plane   2: 128x128                  1       3 K-steps                  min(nsteps, 2)       or MFMA layout, vector stores
    split       1: 64x64                    4       9 K-steps                  min(nsteps, 5)       (set_conv_algo flag 64);
    split       2: 128x128                  2       5 K-steps                  min(nsteps, 3)   K % 4 != 0: scalar stores

RING_STEPS runs every K-step count from 1 to 13 (and 18 and 25 over the taps of a 3x3 and a 5x5 filter) on all four.
A NEW FORM OR TILE OF THE KERNEL MUST BE ADDED TO FORMS / TILES BELOW.  profiles/conv_bf16_exact_tests.md has the rest.
"""
import contextlib
import functools
import zlib

import pytest
import torch

import test_conv_f32_exact as E
from guarded_buffers import DEV, guarded, guards_flag
from test_conv_split_bf16 import SPECIAL_BITS, conv64, split3

BAND = E.BAND                    # 4096 floats: a one-row overrun of the widest shape (2560 channels) stays inside the allocation
WORD_BAND = 4096                 # bf16 words per band of the packed filter: 8192 bytes, so the view keeps 16-byte alignment
NAN_WORD = 0x7FC0                # the bf16 NaN
UNWRITTEN_WORD = 0x7FA5          # a NaN with a payload: no conversion of a finite filter produces it
TWO23, TWO24 = 1 << 23, 1 << 24
FORMS = (1, 3)                   # planes per operand: frcnn_conv2d_fwd_bf16, frcnn_conv2d_fwd_bf16x3
TILES = (1, 2)                   # set_conv_bf16_tile: 64x64, 128x128
STORE_PATHS = (0, 64)            # set_conv_algo: LDS transpose; stores straight from the MFMA layout
EPILOGUES = E.EPILOGUES
FULLEST = "scale_shift_residual_relu"
REGIMES = ("R1", "R2", "R3", "R4", "R5", "R6")
SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))        # kSplitTerms: (x plane, w plane), 0 = hi, 1 = mid, 2 = lo
PINS = {"R1": (0, 0), "R2": (1, 0), "R3": (0, 1), "R4": (1, 1), "R5": (2, 0), "R6": (0, 2)}
PLANES = {"R1": ((0,), (0,)), "R2": ((0, 1), (0,)), "R3": ((0,), (0, 1)), "R4": ((0, 1), (0, 1)),      # non-zero planes of (x, w)
          "R5": ((0, 1, 2), (0,)), "R6": ((0,), (0, 1, 2))}
WINDOWED = ("R4", "R5", "R6")

# name -> (n, h, w, c, k, r, stride, pad), as in test_conv_f32_exact.py
RING_STEPS = tuple(range(1, 14))
RING = {"ring_%02d" % ns: (1, 5, 7, 32 * ns, 36, 1, 1, 0) for ns in RING_STEPS}        # M = 35 and K = 36: tails on both tiles
TAPS = {"taps_3x3": (1, 5, 7, 64, 36, 3, 1, 1),            # 18 K-steps, two per tap
        "taps_5x5": (1, 5, 7, 32, 36, 5, 1, 2)}            # 25 K-steps, one per tap
FROM_F32 = {name: sh for name, sh in E.SHAPES.items() if sh[3] % 32 == 0}
NEW = {"k18_scalar_stores": (1, 5, 7, 32, 18, 1, 1, 0),    # K % 4 != 0
       "k1_scalar_stores": (1, 3, 3, 32, 1, 1, 1, 0),
       "7x7s2": (1, 13, 17, 32, 64, 7, 2, 3),              # 49 K-steps
       "wide580": (1, 10, 13, 32, 580, 1, 1, 0),           # 3 x 10 tiles of 64x64: a ragged raster group, 30 workgroups for xcd_remap
       "rpn2560": (1, 38, 63, 64, 2560, 1, 1, 0)}          # the frame's RPN-sized GEMM at two K-steps; 19 x 20 tiles of 128x128
SHAPES = {**RING, **TAPS, **FROM_F32, **NEW}
BIG = ("persistent", "layer3")                             # default store path and the fullest epilogue only
SPLIT_STORE_SHAPES = ("3x3_odd_batch", "wide580")          # the split form's acc + low through both epilogues: R2 and R3 too

RING_CASES = [(name, regime) for name in list(RING) + list(TAPS) for regime in REGIMES]
EDGE_CASES = [(name, "R1") for name in list(FROM_F32) + list(NEW)] + [(name, regime) for name in SPLIT_STORE_SHAPES for regime in ("R2", "R3")]
CASES = RING_CASES + EDGE_CASES


def case_id(c):
    return "%s-%s" % c


def ksteps_of(name):
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    return r * r * c // 32


def window_of(name):
    """[begin, end) on the reduction axis (r, s, c): 64 indices from the middle of the last K-step but one, cut at the axis' end."""
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    begin = max(0, 32 * (ksteps_of(name) - 2) + 16)
    return begin, min(begin + 64, r * r * c)


# ---- operands and the float64 reference ------------------------------------------------------------------------------------------
def _ints(limit):
    return lambda shape, g: torch.randint(-limit, limit + 1, shape, generator=g).float()


def _odd(low, high):
    """Odd integers with low <= |v| < high and random signs (``_integers`` of test_conv_split_bf16.py)."""
    def make(shape, g):
        mag = torch.randint(low // 2, high // 2, shape, generator=g) * 2 + 1
        return (mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()
    return make


ODD9, ODD18 = _odd(256, 512), _odd(2 ** 17, 2 ** 17 + 2 ** 16)
GENERATORS = {"R1": (_ints(3), _ints(3)), "R2": (ODD9, _ints(2)), "R3": (_ints(2), ODD9), "R4": (ODD9, ODD9),
              "R5": (ODD18, _ints(1)), "R6": (_ints(1), ODD18)}


@functools.lru_cache(maxsize=None)
def case(name, regime):
    """Operands (fp32) and float64 results of one (shape, regime), computed once and left unchanged.  R1 on a shape of
    test_conv_f32_exact.py is that file's reference: same operands, one float64 convolution for both files."""
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    if regime == "R1" and name in E.SHAPES:
        ref = E.reference(name)
        out = {key: ref[key].float() for key in ("x", "w", "scale", "shift", "residual")}
        out["want"] = ref["fwd"]
        return out
    g = torch.Generator().manual_seed(zlib.crc32(("%s/%s" % (name, regime)).encode()))
    make_x, make_w = GENERATORS[regime]
    x, wt = make_x((n, h, w, c), g), make_w((k, r, r, c), g)
    if regime in WINDOWED:
        begin, end = window_of(name)
        inside = torch.zeros(r * r * c, dtype=torch.bool)
        inside[begin:end] = True
        if regime == "R5" and r == 1:
            x = torch.where(inside.view(1, 1, 1, c), x, torch.zeros(()))
        else:
            wt = torch.where(inside.view(1, r, r, c), wt, torch.zeros(()))
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (k,), generator=g)]
    shift, residual = _ints(3)((k,), g), _ints(3)((n, ho, wo, k), g)
    raw = conv64(x, wt, stride, pad)
    affine = raw * scale.double() + shift.double()
    return {"x": x, "w": wt, "scale": scale, "shift": shift, "residual": residual,
            "want": {"none": raw, "scale_shift_relu": torch.relu(affine), FULLEST: torch.relu(affine + residual.double())}}


def epilogues_of(name, regime):
    """The epilogues the device tests run for this case."""
    if name in RING or name in TAPS:
        return ("none",)
    return (FULLEST,) if name in BIG else EPILOGUES


def six_sum(name, xs, ws, terms=SIX):
    """The sum of the listed plane products in float64 (exact: integers far below 2^53)."""
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    return sum(conv64(xs[a], ws[b], stride, pad) for a, b in terms)


# ---- CPU: the inputs are valid, independently of the kernel ------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_regime_precondition_holds(c):
    name, regime = c
    n, h, w, ch, k, r, stride, pad = SHAPES[name]
    ops_ = case(name, regime)
    x, wt = ops_["x"], ops_["w"]
    assert ch % 32 == 0 and x.dtype == torch.float32 and wt.dtype == torch.float32
    # every partial sum, in any order
    assert float(conv64(x.abs(), wt.abs(), stride, pad).max()) < TWO24
    for epilogue in epilogues_of(name, regime):
        want = ops_["want"][epilogue]
        assert float(want.abs().max()) < TWO23 and torch.equal(want.float().double(), want)
    # plane occupancy
    xs, ws = split3(x), split3(wt)
    for planes, (used, operand) in zip((xs, ws), zip(PLANES[regime], (x, wt))):
        assert torch.equal((planes[0] + planes[1]) + planes[2], operand)
        for q in range(3):
            assert bool(planes[q].any()) == (q in used), (regime, q)
        nz = operand != 0
        if used == (0, 1):           # nine significant bits: the mid plane of EVERY non-zero element is non-zero
            assert bool((planes[1] != 0)[nz].all())
        if used == (0, 1, 2):        # eighteen: about half of the odd values need the lo plane
            assert float((planes[2] != 0)[nz].float().mean()) > 0.25 and bool((planes[1] != 0)[nz].any())
    # the three dropped products
    assert not (xs[1].any() and ws[2].any()) and not (xs[2].any() and ws[1].any()) and not (xs[2].any() and ws[2].any())
    if regime == "R1" and name not in RING:
        return          # one plane each: hi*hi is the convolution (asserted above); the emulation below adds nothing
    raw = ops_["want"]["none"]
    assert torch.equal(six_sum(name, xs, ws), raw)
    # the pinned product: without it the result is another one
    pinned = PINS[regime]
    assert not torch.equal(six_sum(name, xs, ws, [t for t in SIX if t != pinned]), raw)
    if regime in WINDOWED:
        begin, end = window_of(name)
        steps = set(range(begin // 32, (end - 1) // 32 + 1))
        assert steps == set(range(max(0, ksteps_of(name) - 2), ksteps_of(name))), "the window covers the last two K-steps"


def test_the_case_table_covers_the_ring_and_every_split_term():
    """Every K-step count 1 .. 13 for each (form, tile); the counts at which each DEPTH enters its steady loop, and one short
    of them, are among them; 18 and 25 steps cross taps; each entry of kSplitTerms is pinned by a regime."""
    assert [ksteps_of(name) for name in RING] == list(range(1, 14))
    assert ksteps_of("taps_3x3") == 18 and ksteps_of("taps_5x5") == 25
    for depth in (1, 2, 4):
        first_steady = 2 * depth + 1
        assert first_steady in RING_STEPS and first_steady - 1 in RING_STEPS
        assert {ns % depth for ns in RING_STEPS} == set(range(depth))
    assert sorted(PINS.values()) == sorted(SIX)
    for name in RING:
        assert {regime for n_, regime in RING_CASES if n_ == name} == set(REGIMES)
    n, h, w, c, k, r, stride, pad = SHAPES["wide580"]
    tiles = ((h * w + 63) // 64, (k + 63) // 64)
    assert tiles == (3, 10) and tiles[1] % 8 != 0 and (tiles[0] * tiles[1]) % 8 != 0
    n, h, w, c, k, r, stride, pad = SHAPES["rpn2560"]
    assert ((h * w + 127) // 128) * ((k + 127) // 128) == 19 * 20 >= 256          # the rule's 128x128 tile: one per CU at least
    assert SHAPES["k18_scalar_stores"][4] % 4 and SHAPES["k1_scalar_stores"][4] % 4
    for name in ("one_pixel", "m259_k132", "k260_3steps", "3x3_odd_batch", "3x3_map1", "3x3_pad0", "3x3s2_pad0", "3x3s2_even",
                 "3x3s2_odd", "1x1s2_even", "1x1s2_odd", "5x5", "linear", "persistent", "layer3"):
        assert name in FROM_F32


def mutated(name, regime, mutation):
    """The six-product sum in float64 after a one-line change of the kernel's arithmetic (emulated on the host)."""
    ops_ = case(name, regime)
    xs, ws = split3(ops_["x"]), split3(ops_["w"])
    if mutation == "terms_0_2_read_as_0_1":
        return six_sum(name, xs, ws, [(0, 1) if t == (0, 2) else t for t in SIX])
    if mutation == "acc_plus_low_dropped":
        return six_sum(name, xs, ws, [(0, 0)])
    assert mutation == "w_plane_one_row_short"
    k, ktot = ops_["w"].shape[0], ops_["w"][0].numel()
    packed = torch.cat([p.reshape(-1) for p in ws])
    short = [packed[q * (k - 1) * ktot:q * (k - 1) * ktot + k * ktot].view_as(ops_["w"]) for q in range(3)]
    return six_sum(name, xs, short)


MUTATIONS = {"terms_0_2_read_as_0_1": ("R3", "R4", "R6"),          # the regimes whose split-form cases then fail
             "acc_plus_low_dropped": ("R2", "R3", "R4", "R5", "R6"),
             "w_plane_one_row_short": REGIMES}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_one_line_arithmetic_changes_are_caught(mutation):
    """profiles/conv_bf16_exact_tests.md: which regime's ring case stops equalling float64 under each change, and in how
    many of its outputs - R3, R4 and R6 are not vacuous."""
    for name in ("ring_06", "ring_13"):
        for regime in REGIMES:
            raw = case(name, regime)["want"]["none"]
            wrong = int((mutated(name, regime, mutation) != raw).sum())
            print("%s, %s %s: %d of %d outputs differ from float64" % (mutation, name, regime, wrong, raw.numel()))
            assert (wrong > 0) == (regime in MUTATIONS[mutation]), (mutation, name, regime)


def test_flag_64_leaves_the_algorithm_mode_alone():
    """set_conv_algo(64): algorithm mode 0, only the store path moves (frcnn_conv2d_set_algo in conv_plan.hip)."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = E.lib().frcnn_settings_signature()
    try:
        ops.set_conv_algo(64)
        assert ops._CONV_ALGO_MODE == 0 and ops._CONV_ALGO_FLAGS == 64
        assert E.lib().frcnn_settings_signature() != before
    finally:
        ops.set_conv_algo(0)
    assert E.lib().frcnn_settings_signature() == before


# ---- guarded device runs ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def hooks():
    """Tile mode and algorithm flags are back at their defaults afterwards, and the settings' signature with them."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = E.lib().frcnn_settings_signature()
    try:
        yield
    finally:
        ops.set_conv_bf16_tile(0)
        ops.set_conv_algo(0)
    assert E.lib().frcnn_settings_signature() == before, "a hook was left set"


def guarded_copy(t):
    """(buffer, view) of a host fp32 tensor between NaN bands on the device."""
    buf, view = guarded(t.numel(), guard=BAND)
    view.copy_(t.reshape(-1).to(DEV))
    return buf, view.view(t.shape)


def guarded_words(words):
    """(buffer, view) of packed bf16 words (int16, on the device) between bands of the bf16 NaN, 16-byte aligned."""
    buf = torch.full((words.numel() + 2 * WORD_BAND,), NAN_WORD, dtype=torch.int16, device=DEV)
    view = buf[WORD_BAND:WORD_BAND + words.numel()]
    view.copy_(words.reshape(-1))
    assert view.data_ptr() % 16 == 0
    return buf, view.view(words.shape)


def word_bands_flag(buf, numel):
    return (buf[:WORD_BAND] == NAN_WORD).all() & (buf[WORD_BAND + numel:] == NAN_WORD).all()


def plane_bits(t):
    """The bf16 words of an fp32 tensor that bf16 holds exactly."""
    return t.to(torch.bfloat16).view(torch.int16)


@functools.lru_cache(maxsize=None)
def on_device(name, regime):
    """The case's operands in guarded buffers and its float64 results on the device, uploaded once.  The packers run on the
    plain filter; their results - checked against the host's split - are copied between the NaN-word bands."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    ops_ = case(name, regime)
    dev = {"bufs": []}
    for key in ("x", "scale", "shift", "residual"):
        buf, dev[key] = guarded_copy(ops_[key])
        dev["bufs"].append((buf, ops_[key].numel()))
    w_dev = ops_["w"].to(DEV)
    packed = {3: ops.conv2d_pack_bf16x3(w_dev)}
    assert torch.equal(packed[3].cpu(), torch.stack([plane_bits(p) for p in split3(ops_["w"])]))
    if regime == "R1":
        packed[1] = ops.conv2d_pack_bf16(w_dev)
        assert torch.equal(packed[1].cpu(), plane_bits(ops_["w"]))
    dev["wq"], dev["wbufs"] = {}, []
    for form, words in packed.items():
        buf, dev["wq"][form] = guarded_words(words)
        dev["wbufs"].append((buf, words.numel()))
    dev["want"] = {epilogue: ops_["want"][epilogue].to(DEV) for epilogue in epilogues_of(name, regime)}
    return dev


def run(name, regime, form, epilogue, label):
    """One guarded launch and its verdict (one synchronisation): bands of y and of every operand, no NaN in y, y == float64.
    Returns y."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    n, h, w, c, k, r, stride, pad = SHAPES[name]
    ho, wo = E.out_hw(h, w, r, stride, pad)
    dev = on_device(name, regime)
    obuf, out = guarded(n * ho * wo * k, guard=BAND)
    affine = epilogue != "none"
    fn = ops.conv2d_nhwc_bf16 if form == 1 else ops.conv2d_nhwc_bf16x3
    got = fn(dev["x"], dev["wq"][form], dev["scale"] if affine else None, dev["shift"] if affine else None,
             dev["residual"] if epilogue == FULLEST else None, stride=stride, pad=pad, relu=affine, out=out.view(n, ho, wo, k))
    assert got.data_ptr() == out.data_ptr()
    want = dev["want"][epilogue].reshape(-1)
    operands_ok = torch.stack([guards_flag(buf, numel, BAND) for buf, numel in dev["bufs"]]
                              + [word_bands_flag(buf, numel) for buf, numel in dev["wbufs"]]).all()
    flags = torch.stack([guards_flag(obuf, out.numel(), BAND), operands_ok, ~torch.isnan(out).any(), (out.double() == want).all()]).tolist()
    label = "%s %s, %s, %s %s" % (name, regime, "one plane" if form == 1 else "split", label, epilogue)
    assert flags[0], "%s: wrote outside y" % label
    assert flags[1], "%s: an operand's guard band changed" % label
    if not flags[2]:
        bad = torch.isnan(out).nonzero().reshape(-1)
        pytest.fail("%s: %d of %d outputs are NaN (not written, or computed from a read outside an operand), first at %d"
                    % (label, bad.numel(), out.numel(), int(bad[0])))
    if not flags[3]:
        bad = (out.double() != want).nonzero().reshape(-1)
        i = int(bad[0])
        pytest.fail("%s: %d of %d outputs differ from float64, first at %d (row %d, channel %d): got %r, want %r"
                    % (label, bad.numel(), out.numel(), i, i // k, i % k, float(out[i]), float(want[i])))
    return out


def forms_of(regime):
    return FORMS if regime == "R1" else (3,)


def sweep_ring(name):
    """Both forms where the regime allows, both tiles, every regime; returns the number of launches."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    runs = 0
    with hooks():
        for tile in TILES:
            ops.set_conv_bf16_tile(tile)
            for regime in REGIMES:
                for form in forms_of(regime):
                    run(name, regime, form, "none", "tile %d, %d K-steps," % (tile, ksteps_of(name)))
                    runs += 1
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RING))
def test_ring_every_step_count(hip, name):
    """1x1, M = 35, K = 36, C = 32 nsteps for nsteps = 1 .. 13: the prologue, the steady loop's entry and the tail round of
    each DEPTH at every residue.  One plane: R1.  Split: R1, R2, R3 dense, R4, R5, R6 across the last two K-steps."""
    assert sweep_ring(name) == len(TILES) * (len(REGIMES) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TAPS))
def test_ring_across_taps(hip, name):
    """3x3 / pad 1 at two K-steps per tap and 5x5 / pad 2 at one: the tap state advances with every load of the ring."""
    assert sweep_ring(name) == len(TILES) * (len(REGIMES) + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FROM_F32) + list(NEW))
def test_shapes_and_edges(hip, name):
    """R1, both forms, both forced tiles, both store paths, the three epilogues (persistent and layer3: the default store
    path and the fullest epilogue); rpn2560 also under the library's own tile rule, which picks 128x128 there."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    big = name in BIG
    tiles = TILES + (0,) if name == "rpn2560" else TILES
    runs = 0
    with hooks():
        for tile in tiles:
            ops.set_conv_bf16_tile(tile)
            for algo in STORE_PATHS[:1] if big else STORE_PATHS:
                ops.set_conv_algo(algo)
                for form in FORMS:
                    for epilogue in epilogues_of(name, "R1"):
                        run(name, "R1", form, epilogue, "tile %d, algo %d," % (tile, algo))
                        runs += 1
    assert runs == len(tiles) * len(FORMS) * (1 if big else len(STORE_PATHS) * len(EPILOGUES))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SPLIT_STORE_SHAPES)
def test_split_form_adds_its_small_terms_before_either_epilogue(hip, name):
    """R2 and R3 - `low` is not zero - through both store paths and the three epilogues, on both tiles."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    with hooks():
        for tile in TILES:
            ops.set_conv_bf16_tile(tile)
            for algo in STORE_PATHS:
                ops.set_conv_algo(algo)
                for regime in ("R2", "R3"):
                    for epilogue in EPILOGUES:
                        run(name, regime, 3, epilogue, "tile %d, algo %d," % (tile, algo))


@pytest.mark.gpu
def test_tiles_and_runs_are_bit_equal_where_the_lo_planes_matter(hip):
    """R5 at seven K-steps: the two tiles and two runs of each give the same bits (which equality with float64 implies)."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    ys = []
    with hooks():
        for tile in TILES:
            ops.set_conv_bf16_tile(tile)
            for again in range(2):
                ys.append(run("ring_07", "R5", 3, "none", "tile %d, run %d," % (tile, again)).clone())
    for y in ys[1:]:
        assert torch.equal(y.view(torch.int32), ys[0].view(torch.int32))


# ---- the packers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("planes", FORMS)
def test_packers_write_every_word_and_nothing_else(hip, planes):
    """frcnn_conv2d_pack_bf16 / _bf16x3 through the C entries on 3 x 3 x 3 x 37 = 999 values (not a multiple of the 256
    threads of a block), into a view between NaN-word bands pre-filled with a word no conversion gives."""
    from faster_rcnn_pytorch_multimodal_amd import _hip
    k, r, s, c = 3, 3, 3, 37
    count = k * r * s * c
    assert count % 256
    g = torch.Generator().manual_seed(planes)
    special = torch.tensor(SPECIAL_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    wt = torch.cat([special, torch.randn(count - len(SPECIAL_BITS), generator=g) * 0.05]).view(k, r, s, c)
    wbuf, w_dev = guarded_copy(wt)
    buf, out = guarded_words(torch.full((planes * count,), UNWRITTEN_WORD, dtype=torch.int16, device=DEV))
    entry = hip.frcnn_conv2d_pack_bf16 if planes == 1 else hip.frcnn_conv2d_pack_bf16x3
    _hip.check(entry(w_dev.data_ptr(), out.data_ptr(), k, r, s, c, torch.cuda.current_stream().cuda_stream), "pack")
    torch.cuda.synchronize()
    assert bool(word_bands_flag(buf, planes * count)), "wrote outside the packed filter"
    assert bool(guards_flag(wbuf, count, BAND))
    assert not bool((out == UNWRITTEN_WORD).any()), "a word was not written"
    want = plane_bits(wt).reshape(-1) if planes == 1 else torch.cat([plane_bits(p).reshape(-1) for p in split3(wt)])
    assert torch.equal(out.cpu(), want)


# ---- last: nothing is left set ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_hook_is_left_set(hip):
    """Tile mode 0 and algorithm 0: the settings' signature does not change when both are set to their defaults, and a
    hook-free call still gives float64."""
    from faster_rcnn_pytorch_multimodal_amd import ops
    before = hip.frcnn_settings_signature()
    ops.set_conv_bf16_tile(0)
    ops.set_conv_algo(0)
    assert hip.frcnn_settings_signature() == before, "a bf16 convolution hook was left set"
    for form in FORMS:
        run("3x3_odd_batch", "R1", form, FULLEST, "hook-free,")
