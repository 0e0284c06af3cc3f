"""The solver's weight update as one HIP launch (csrc/optim.hip frcnn_sgd_update, ops.sgd_update, model/train_val.FusedSGD,
cfg.TRAIN.FUSED_UPDATE): bit-equal to a numpy float32 restatement at every alignment of head, body and tail, nothing written
outside the segments, the same optimizer as torch.optim.SGD + per-element clamp to rounding, table upkeep, and the wiring
through SolverWrapper and a captured training step of the real detector."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                                     # unit roundoff of float32

CHUNK = 4096                                       # the kernel's elements per workgroup (asserted against ops.SGD_CHUNK)
# [1, 3, 4, 5, 63, 64, 65, CHUNK-1, CHUNK, CHUNK+1, 2*CHUNK+7] ordered so that the flat offsets cover the four residues
# mod 4 - and the four segments of a chunk or more start at four different ones
COUNTS = [4, 63, 64, CHUNK - 1, 65, 1, CHUNK + 1, 5, 2 * CHUNK + 7, CHUNK, 3]
OFFSETS = np.concatenate(([0], np.cumsum(COUNTS)[:-1])).astype(np.int64)
TOTAL = int(np.sum(COUNTS))
GAPS = [1, 2, 3, 5]                                # sentinel floats between and around the parameters
SENTINEL = np.uint32(0xDEADBEEF)
CLIP = np.float32(2.0)
LR_W, WD_W = np.float32(1e-3), np.float32(1e-4)    # weights (sgd_param_groups)
LR_B, WD_B = np.float32(2e-3), np.float32(0.0)     # biases: doubled rate, no decay
# which segments play "bias": both classes occur among the four long segments and among the short ones
IS_BIAS = [False, True, False, True, False, True, False, True, True, False, False]


def test_segment_order_covers_every_alignment():
    assert sorted(COUNTS) == sorted([1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7])
    assert {int(o) % 4 for o in OFFSETS} == {0, 1, 2, 3}
    assert {int(o) % 4 for o, c in zip(OFFSETS, COUNTS) if c >= CHUNK - 1} == {0, 1, 2, 3}
    from faster_rcnn_pytorch_multimodal_amd import ops
    assert ops.SGD_CHUNK == CHUNK
    long_ = [b for b, c in zip(IS_BIAS, COUNTS) if c >= CHUNK - 1]
    assert True in long_ and False in long_


def _rates():
    lr = np.array([LR_B if b else LR_W for b in IS_BIAS], np.float32)
    wd = np.array([WD_B if b else WD_W for b in IS_BIAS], np.float32)
    return lr, wd


def _gradients(seed):
    """Seeded normals; every segment of 63 elements or more also holds +-clip, values beyond +-clip, +0.0, -0.0, a
    subnormal, +-inf and a NaN - at its start (head and first groups) or at its end (last groups and tail)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(TOTAL).astype(np.float32)
    special = np.array([CLIP, -CLIP, 2 * CLIP, -3 * CLIP, 0.0, -0.0, 1e-40, np.inf, -np.inf, np.nan], np.float32)
    for i, (o, c) in enumerate(zip(OFFSETS, COUNTS)):
        if c >= 63:
            at = o if i % 2 == 0 else o + c - len(special)
            g[at:at + len(special)] = special
    assert np.signbit(g[g == 0]).any() and (np.abs(g[np.isfinite(g)]) > CLIP).sum() > 100
    assert ((g != 0) & (np.abs(g) < np.finfo(np.float32).tiny)).any()
    return g


def _np_update(p, g, b, lr, wd, momentum, clip, zero):
    """The five lines of the kernel in numpy float32, one numpy operation per arithmetic step.  Returns (p, g, b)."""
    assert p.dtype == g.dtype == b.dtype == np.float32
    lr, wd, momentum, clip = np.float32(lr), np.float32(wd), np.float32(momentum), np.float32(clip)
    with np.errstate(all="ignore"):
        if clip > 0 and np.isfinite(clip):
            g = np.minimum(np.maximum(g, -clip), clip)          # both propagate NaN, like torch.clamp_
        d = g
        if wd != 0:
            t = wd * p
            d = g + t
        t = b * momentum
        b = t + d
        t = (-lr) * b
        p = p + t
    for a in (p, g, b):
        assert a.dtype == np.float32
    return p, (np.zeros_like(g) if zero else g), b


def _np_update_all(p, g, b, lrs, wds, momentum, clip, zero):
    p, g, b = p.copy(), g.copy(), b.copy()
    for o, c, lr, wd in zip(OFFSETS, COUNTS, lrs, wds):
        s = slice(int(o), int(o) + c)
        p[s], g[s], b[s] = _np_update(p[s], g[s], b[s], lr, wd, momentum, clip, zero)
    return p, g, b


def _assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "%s: NaN positions differ (%d vs %d)" % (what, nan_g.sum(), nan_w.sum())
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~nan_w
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d words differ, first at %d: got %r (%#x), want %r (%#x)"
                             % (what, bad.sum(), bad.size, i, got[i], got.view(np.uint32)[i], want[i], want.view(np.uint32)[i]))


class _Arena:
    """Parameters as views into ONE buffer with sentinel gaps of 1, 2, 3, 5 floats between and around them (so the
    parameters start at every alignment too); the flat gradient and momentum buffers sit inside larger buffers at two
    different misalignments, sentinels before and behind."""

    def __init__(self, seed):
        from faster_rcnn_pytorch_multimodal_amd import ops
        rng = np.random.default_rng(seed)
        self.p_host = (rng.standard_normal(TOTAL) * 0.1).astype(np.float32)
        self.p_pos, at = [], 0
        for i, c in enumerate(COUNTS):
            at += GAPS[i % 4]
            self.p_pos.append(at)
            at += c
        at += GAPS[len(COUNTS) % 4]
        image = np.full(at, SENTINEL, np.uint32)
        self.p_mask = np.zeros(at, bool)
        for pos, o, c in zip(self.p_pos, OFFSETS, COUNTS):
            image[pos:pos + c] = self.p_host[o:o + c].view(np.uint32)
            self.p_mask[pos:pos + c] = True
        self.p_buf = torch.from_numpy(image.view(np.float32).copy()).to(DEV)
        self.g_lead, self.b_lead, trail = 3, 1, 5
        self.g_buf = torch.from_numpy(np.full(self.g_lead + TOTAL + trail, SENTINEL, np.uint32).view(np.float32).copy()).to(DEV)
        self.b_buf = torch.from_numpy(np.full(self.b_lead + TOTAL + trail, SENTINEL, np.uint32).view(np.float32).copy()).to(DEV)
        self.grad = self.g_buf[self.g_lead:self.g_lead + TOTAL]
        self.mom = self.b_buf[self.b_lead:self.b_lead + TOTAL]
        self.mom.zero_()
        assert self.grad.data_ptr() % 16 != self.mom.data_ptr() % 16
        lr, wd = _rates()
        ptrs = [self.p_buf.data_ptr() + 4 * pos for pos in self.p_pos]
        assert len({q % 16 for q in ptrs}) >= 3                    # ... and against the gradient at every relative offset
        assert {(q - self.grad.data_ptr() - 4 * int(o)) % 16 for q, o in zip(ptrs, OFFSETS)} == {0, 4, 8, 12}
        self.seg, chunks = ops.sgd_tables(ptrs, OFFSETS, COUNTS, lr, wd)
        assert len(chunks) == sum((c + CHUNK - 1) // CHUNK for c in COUNTS)
        self.seg_dev = torch.from_numpy(self.seg.view(np.uint8).copy()).to(DEV)
        self.chunks_dev = torch.from_numpy(chunks).to(DEV)

    def set_grad(self, g):
        self.grad.copy_(torch.from_numpy(g))

    def update(self, momentum, clip, zero):
        from faster_rcnn_pytorch_multimodal_amd import ops
        ops.sgd_update(self.grad, self.mom, self.seg, self.seg_dev, self.chunks_dev, momentum, clip=clip, zero_grads=zero)
        torch.cuda.synchronize()

    def params(self):
        image = self.p_buf.cpu().numpy()
        out = np.empty(TOTAL, np.float32)
        for pos, o, c in zip(self.p_pos, OFFSETS, COUNTS):
            out[o:o + c] = image[pos:pos + c]
        return out

    def assert_sentinels(self, what):
        image = self.p_buf.cpu().numpy().view(np.uint32)
        assert (image[~self.p_mask] == SENTINEL).all(), "%s: a word between the parameters was written" % what
        assert (~self.p_mask).sum() == sum(GAPS[i % 4] for i in range(len(COUNTS) + 1))
        for buf, lead, name in ((self.g_buf, self.g_lead, "gradient"), (self.b_buf, self.b_lead, "momentum")):
            words = buf.cpu().numpy().view(np.uint32)
            assert (words[:lead] == SENTINEL).all() and (words[lead + TOTAL:] == SENTINEL).all(), \
                "%s: a word outside the flat %s buffer was written" % (what, name)


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("momentum", [0.5, 0.9, 0.0])
def test_bit_equal_to_numpy_float32_restatement(hip, momentum, zero):
    """Three consecutive updates with fresh gradients (the momentum buffer is carried): parameters, momentum buffers and
    what is left in the gradient buffer equal the numpy restatement word for word, NaN positions included."""
    arena = _Arena(seed=11)
    lrs, wds = _rates()
    p, b = arena.p_host.copy(), np.zeros(TOTAL, np.float32)
    for step in range(3):
        g = _gradients(100 + step)
        arena.set_grad(g)
        arena.update(momentum, CLIP, zero)
        p, g_after, b = _np_update_all(p, g, b, lrs, wds, momentum, CLIP, zero)
        what = "momentum %g, zero %s, update %d" % (momentum, zero, step)
        _assert_bits(arena.params(), p, what + ", parameters")
        _assert_bits(arena.mom.cpu().numpy(), b, what + ", momentum buffers")
        left = arena.grad.cpu().numpy()
        if zero:
            assert not left.view(np.uint32).any(), what + ": a gradient word is not +0.0"
        else:
            _assert_bits(left, g_after, what + ", clipped gradients left in place")
            assert np.nanmax(np.abs(left[np.isfinite(left)])) == CLIP and np.isnan(left).sum() == np.isnan(g).sum()
        arena.assert_sentinels(what)
    assert np.isnan(p).any() and np.isfinite(p).sum() > 0.99 * TOTAL


def test_without_clip_the_gradient_is_untouched(hip):
    """clip <= 0 and clip = +inf mean no clip (FusedSGD.step): values beyond CLIP are stepped as they are."""
    lrs, wds = _rates()
    for clip in (0.0, -1.0, float("inf")):
        arena = _Arena(seed=12)
        g = _gradients(7)
        arena.set_grad(g)
        arena.update(0.9, clip, False)
        p, g_after, b = _np_update_all(arena.p_host, g, np.zeros(TOTAL, np.float32), lrs, wds, 0.9, clip, False)
        _assert_bits(arena.params(), p, "clip %r, parameters" % clip)
        _assert_bits(arena.mom.cpu().numpy(), b, "clip %r, momentum" % clip)
        _assert_bits(arena.grad.cpu().numpy(), g, "clip %r, gradients" % clip)
        assert np.array_equal(g_after.view(np.uint32), g.view(np.uint32))
        arena.assert_sentinels("clip %r" % clip)
        assert np.isinf(p).any() and np.isnan(p).any()


def test_nothing_outside_the_segments_is_written(hip):
    """Every sentinel word - gaps of 1, 2, 3 and 5 floats between and around the parameters, and the words before and behind
    the flat gradient and momentum buffers - survives updates with and without the clearing store."""
    arena = _Arena(seed=13)
    arena.assert_sentinels("before any update")
    for step, zero in enumerate((False, True, True)):
        arena.set_grad(_gradients(40 + step))
        before = arena.params()
        arena.update(0.5, CLIP, zero)
        arena.assert_sentinels("update %d (zero %s)" % (step, zero))
        assert (arena.params() != before).sum() > 0.98 * TOTAL           # ... and the segments themselves were written


def test_zero_segments_is_a_no_op_and_bad_tables_are_refused(hip):
    from faster_rcnn_pytorch_multimodal_amd import _hip, ops
    flat = torch.ones(16, device=DEV)
    mom = torch.ones(16, device=DEV)
    seg, chunks = ops.sgd_tables([], [], [], [], [])
    ops.sgd_update(flat, mom, seg, torch.empty(0, dtype=torch.uint8, device=DEV),
                   torch.empty((0, 2), dtype=torch.int32, device=DEV), 0.9, clip=1.0, zero_grads=True)
    torch.cuda.synchronize()
    assert float(flat.sum()) == 16 and float(mom.sum()) == 16
    lib = _hip.load()
    seg, chunks = ops.sgd_tables([flat.data_ptr()], [0], [8], [0.1], [0.0])
    seg_dev, chunks_dev = torch.from_numpy(seg.view(np.uint8).copy()).to(DEV), torch.from_numpy(chunks).to(DEV)
    good = [flat.data_ptr(), mom.data_ptr(), 16, seg_dev.data_ptr(), seg.ctypes.data, 1, chunks_dev.data_ptr(), 1, 0.9, 0.0, 0, None]
    for null_at in (0, 1, 3, 4, 6):                       # grad, momentum, device table, host table, chunk table
        args = list(good)
        args[null_at] = None
        assert lib.frcnn_sgd_update(*args) == -1 and b"null argument" in lib.frcnn_last_error(), null_at
    seg["param"][0] = 0
    assert lib.frcnn_sgd_update(*good) == -1 and b"parameter pointer of segment 0" in lib.frcnn_last_error()
    assert lib.frcnn_sgd_update(*(good[:5] + [-1] + good[6:])) == -1 and b"negative segment count" in lib.frcnn_last_error()
    torch.cuda.synchronize()
    assert float(flat.sum()) == 16 and float(mom.sum()) == 16
    prm = torch.ones(8, device=DEV)
    for offset, count, text in ((12, 8, "reaches past the flat buffer"), (0, -1, "negative count")):
        seg, _ = ops.sgd_tables([prm.data_ptr()], [offset], [count], [0.1], [0.0])
        with pytest.raises(_hip.HipError, match=text):
            ops.sgd_update(flat, mom, seg, torch.from_numpy(seg.view(np.uint8).copy()).to(DEV),
                           torch.zeros((1, 2), dtype=torch.int32, device=DEV), 0.9)
    seg, chunks = ops.sgd_tables([prm.data_ptr()], [0], [8], [0.1], [0.0])
    with pytest.raises(_hip.HipError, match="no CPU path"):
        ops.sgd_update(flat.cpu(), mom, seg, torch.from_numpy(seg.view(np.uint8).copy()).to(DEV), torch.from_numpy(chunks).to(DEV), 0.9)
    with pytest.raises(_hip.HipError, match="chunks given"):
        ops.sgd_update(flat, mom, seg, torch.from_numpy(seg.view(np.uint8).copy()).to(DEV),
                       torch.zeros((2, 2), dtype=torch.int32, device=DEV), 0.9)
    torch.cuda.synchronize()
    assert float(prm.sum()) == 8 and float(flat.sum()) == 16


# ----------------------------------------------------------------------------------------------------------------------
# FusedSGD
# ----------------------------------------------------------------------------------------------------------------------
class _Params(torch.nn.Module):
    """One parameter per segment, named so that sgd_param_groups makes the two learning-rate classes of IS_BIAS."""

    def __init__(self, values):
        super().__init__()
        for i, (o, c) in enumerate(zip(OFFSETS, COUNTS)):
            name = "seg%02d_%s" % (i, "bias" if IS_BIAS[i] else "weight")
            self.register_parameter(name, torch.nn.Parameter(torch.from_numpy(values[o:o + c].copy())))


@pytest.fixture
def cfg_():
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    C.reset_cfg()
    C.cfg.NET_TYPE = "image"
    yield C.cfg
    C.reset_cfg()


def _fused(cfg_, values, momentum):
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    cfg_.TRAIN.DOUBLE_BIAS = True
    cfg_.TRAIN.LEARNING_RATE = float(LR_W)
    cfg_.TRAIN.WEIGHT_DECAY = float(WD_W)
    net = _Params(values).to(DEV)
    groups = train_val.sgd_param_groups(net)
    assert [np.float32(g["lr"]) for g in groups] == list(_rates()[0])
    assert [np.float32(g["weight_decay"]) for g in groups] == list(_rates()[1])
    bucket = train_val.GradientBucket([p for g in groups for p in g["params"]])
    return net, bucket, train_val.FusedSGD(groups, bucket, momentum=momentum)


def _flat_params(net):
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in net.parameters()])


def test_same_optimizer_as_torch_sgd_with_clamp(hip, cfg_):
    """torch.optim.SGD + per-element clamp on CPU copies of the same inputs, three updates.  Torch's CPU kernels may contract
    a + alpha * b, so agreement is asked to the rounding bound of the formula: with u = 2^-24 and
    S = momentum |b| + |g_clipped| + wd |p|, momentum within 5 u S and parameter within 8 u (|p| + lr S).  Every update is
    judged on its own: the reference starts each one from the device's parameters and momentum buffers."""
    momentum = 0.9
    rng = np.random.default_rng(21)
    net, bucket, opt = _fused(cfg_, (rng.standard_normal(TOTAL) * 0.1).astype(np.float32), momentum)
    lrs, wds = _rates()
    lr_e = np.repeat(lrs.astype(np.float64), COUNTS)
    wd_e = np.repeat(wds.astype(np.float64), COUNTS)
    assert bucket.flat.numel() == TOTAL + 1
    for step in range(3):
        g = _gradients(300 + step)
        p0 = _flat_params(net)
        b0 = opt.momentum_flat[:TOTAL].cpu().numpy().copy()
        bucket.flat[:TOTAL].copy_(torch.from_numpy(g))
        opt.fused_update(clip=float(CLIP), zero=False)
        torch.cuda.synchronize()
        p_dev, b_dev = _flat_params(net), opt.momentum_flat[:TOTAL].cpu().numpy()
        # the existing path on the CPU: clamp_ every .grad, then torch.optim.SGD over the same one-group-per-parameter list
        ref = [torch.nn.Parameter(torch.from_numpy(p0[o:o + c].copy())) for o, c in zip(OFFSETS, COUNTS)]
        sgd = torch.optim.SGD([{"params": [r], "lr": float(lr), "weight_decay": float(wd)} for r, lr, wd in zip(ref, lrs, wds)],
                              momentum=momentum)
        for r, o, c in zip(ref, OFFSETS, COUNTS):
            r.grad = torch.from_numpy(g[o:o + c].copy())
            r.grad.clamp_(-float(CLIP), float(CLIP))
            if step > 0:
                sgd.state[r]["momentum_buffer"] = torch.from_numpy(b0[o:o + c].copy())
        sgd.step()
        p_ref = np.concatenate([r.detach().numpy() for r in ref])
        b_ref = np.concatenate([sgd.state[r]["momentum_buffer"].numpy() for r in ref])
        with np.errstate(all="ignore"):
            gc = np.clip(g.astype(np.float64), -float(CLIP), float(CLIP))
            S = momentum * np.abs(b0.astype(np.float64)) + np.abs(gc) + wd_e * np.abs(p0.astype(np.float64))
            tol_b = 5 * U * S
            tol_p = 8 * U * (np.abs(p0.astype(np.float64)) + lr_e * S)
            err_b = np.abs(b_dev.astype(np.float64) - b_ref)
            err_p = np.abs(p_dev.astype(np.float64) - p_ref)
        for name, ref_v, dev_v, err, tol in (("momentum", b_ref, b_dev, err_b, tol_b), ("parameter", p_ref, p_dev, err_p, tol_p)):
            skip = ~np.isfinite(ref_v)
            assert skip.mean() <= 0.01, (step, name, skip.mean())
            assert not np.isfinite(dev_v[skip]).any(), (step, name)
            assert np.isfinite(dev_v[~skip]).all(), (step, name)
            ratio = err[~skip] / np.maximum(tol[~skip], 1e-300)
            print("update %d %s: worst error / bound = %.3f" % (step, name, ratio.max()))
            assert (err[~skip] <= tol[~skip]).all(), (step, name, float(ratio.max()))


def test_table_follows_scale_lr_and_is_uploaded_only_then(hip, cfg_):
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    rng = np.random.default_rng(31)
    values = (rng.standard_normal(TOTAL) * 0.1).astype(np.float32)
    net, bucket, opt = _fused(cfg_, values, 0.5)
    lrs, wds = _rates()
    p, b = values.copy(), np.zeros(TOTAL, np.float32)
    assert opt.uploads == 1
    for step in range(4):
        if step == 2:
            train_val.scale_lr(opt, 0.1)
            lrs = np.array([np.float32(g["lr"]) for g in opt.param_groups], np.float32)     # the scaled rate as np.float32
            assert np.allclose(lrs, _rates()[0] * 0.1, rtol=1e-6)
        g = _gradients(500 + step)
        bucket.flat[:TOTAL].copy_(torch.from_numpy(g))
        versions = [prm._version for prm in net.parameters()]
        if step % 2:
            opt.step()                                         # the plain-optimizer form: no clip, gradients stay
            clip, zero = 0.0, False
        else:
            opt.fused_update(clip=float(CLIP), zero=True)
            clip, zero = CLIP, True
        torch.cuda.synchronize()
        # the kernel writes through raw pointers: step() and fused_update() both bump every parameter's version counter (the
        # caches of weight-derived filters are keyed by it, also on the eager path)
        assert all(prm._version > v for prm, v in zip(net.parameters(), versions)), step
        p, g_after, b = _np_update_all(p, g, b, lrs, wds, 0.5, clip, zero)
        _assert_bits(_flat_params(net), p, "update %d, parameters" % step)
        _assert_bits(opt.momentum_flat[:TOTAL].cpu().numpy(), b, "update %d, momentum" % step)
        _assert_bits(bucket.flat[:TOTAL].cpu().numpy(), g_after, "update %d, gradients" % step)
        assert opt.uploads == (1 if step < 2 else 2)           # re-uploaded once, by the update that followed scale_lr
    # the momentum buffers of state[] are the views the kernel wrote, and zero_grad keeps the bucket's views
    for prm, o in zip(net.parameters(), OFFSETS):
        assert opt.state[prm]["momentum_buffer"].data_ptr() == opt.momentum_flat.data_ptr() + 4 * int(o)
    opt.zero_grad()
    assert not bucket.flat.cpu().numpy().view(np.uint32).any()
    assert all(prm.grad.data_ptr() == bucket.flat.data_ptr() + 4 * int(o) for prm, o in zip(net.parameters(), OFFSETS))


def test_parameters_that_are_not_contiguous_float32_are_refused(hip, cfg_):
    """The segment table describes a parameter as numel() consecutive floats: a permuted or strided parameter would be
    stepped with the wrong gradient element or written between its elements."""
    from faster_rcnn_pytorch_multimodal_amd.model import train_val

    class Net(torch.nn.Module):
        def __init__(self, weight):
            super().__init__()
            self.weight = torch.nn.Parameter(weight)

    for weight in (torch.zeros(6, 4, device=DEV).t(), torch.zeros(4, 12, device=DEV)[:, ::2]):
        groups = train_val.sgd_param_groups(Net(weight))
        bucket = train_val.GradientBucket([p for g in groups for p in g["params"]])
        with pytest.raises(ValueError, match="must be contiguous float32"):
            train_val.FusedSGD(groups, bucket, momentum=0.5)


@pytest.mark.parametrize("what", ["grad", "storage"])
def test_replaced_grad_or_storage_raises_and_updates_nothing(hip, cfg_, what):
    rng = np.random.default_rng(41)
    values = (rng.standard_normal(TOTAL) * 0.1).astype(np.float32)
    net, bucket, opt = _fused(cfg_, values, 0.5)
    bucket.flat[:TOTAL].copy_(torch.from_numpy(rng.standard_normal(TOTAL).astype(np.float32)))
    victim = list(net.parameters())[6]
    if what == "grad":
        victim.grad = torch.ones_like(victim)
        text = "no longer the gradient bucket's view"
    else:
        victim.data = victim.data.clone()
        text = "storage of parameter 6 .* was replaced"
    before, grads = _flat_params(net), bucket.flat.clone()
    versions = [p._version for p in net.parameters()]
    for call in (opt.step, lambda: opt.fused_update(clip=1.0, zero=True)):
        with pytest.raises(RuntimeError, match=text):
            call()
    torch.cuda.synchronize()
    assert np.array_equal(_flat_params(net).view(np.uint32), before.view(np.uint32))
    assert torch.equal(bucket.flat, grads) and not opt.momentum_flat.cpu().numpy().view(np.uint32).any()
    assert versions == [p._version for p in net.parameters()]


# ----------------------------------------------------------------------------------------------------------------------
# through the solver
# ----------------------------------------------------------------------------------------------------------------------
class _DeviceStubNet(torch.nn.Module):
    """The protocol subset SolverWrapper uses, on the device.  The loss is LINEAR in the weights, so a frame's gradient does
    not depend on them: the run with the switch on and the run with it off see bit-identical gradients and differ by the
    rounding of their updates alone.  ``form``: 'apply_update' = Network.apply_update as Network.train_step calls it,
    'step' = optimizer.step(); optimizer.zero_grad()."""

    def __init__(self, form):
        from faster_rcnn_pytorch_multimodal_amd.nets.network import Network
        super().__init__()
        self._device = DEV
        self.form = form
        self.lin = torch.nn.Linear(37, 5)
        self.scale = torch.nn.Parameter(torch.ones(3))
        self.updates = []
        self._apply_update = Network.apply_update
        self._clip = Network._clip_gradients

    def _clip_gradients(self):
        return self._clip(self)

    def train_step(self, blobs, optimizer, update_weights=False):
        x, y = blobs["data"].to(DEV), blobs["y"].to(DEV)
        loss = (self.lin(x) * y).sum() + (self.scale * y[:, :3].sum(0)).sum()
        loss.backward()
        if update_weights:
            inner = optimizer.optimizer
            rec = {"lr": [g["lr"] for g in optimizer.param_groups], "wd": [g["weight_decay"] for g in optimizer.param_groups],
                   "p": [p.detach().clone() for p in self.parameters()], "g": [p.grad.clone() for p in self.parameters()],
                   "b": [inner.state[p]["momentum_buffer"].clone() if "momentum_buffer" in inner.state.get(p, {})
                         else torch.zeros_like(p) for p in self.parameters()]}
            if self.form == "apply_update":
                self._apply_update(self, optimizer)
            else:
                optimizer.step()
                optimizer.zero_grad()
            rec["after"] = [p.detach().clone() for p in self.parameters()]
            rec["grad_after"] = [p.grad.clone() for p in self.parameters()]
            self.updates.append(rec)
        return float(loss.item())

    def train_step_with_summary(self, blobs, optimizer, sum_size, update_weights=False):
        return self.train_step(blobs, optimizer, update_weights), [("total_loss", 0.0)]


class _Frames:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def next(self):
        return {"data": torch.from_numpy(self.rng.standard_normal((4, 37)).astype(np.float32)),
                "y": torch.from_numpy(self.rng.standard_normal((4, 5)).astype(np.float32))}


@pytest.mark.parametrize("form", ["apply_update", "step"])
def test_solver_with_the_switch_on_follows_the_run_with_it_off(hip, cfg_, tmp_path, form):
    """SolverWrapper.train_model over two learning-rate drops (STEPSIZE [6, 12], batch size 2: seven weight updates, the rate
    drops before the fourth and the seventh), once with torch.optim.SGD and once with FusedSGD, from the same seed.  After
    update k the parameters agree within sum over j <= k of 8 u (|p_j| + lr_j S_j), S_j from the reference run.  The carried
    error of the momentum buffer (at most lr * momentum * 5 u S_{j-1} per update) is inside that sum's slack: an update spends
    2 u |p| + 5 u lr S of its 8 u (|p| + lr S)."""
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    cfg_.TRAIN.STEPSIZE = [6, 12]
    cfg_.TRAIN.SNAPSHOT_ITERS = 1000
    cfg_.TRAIN.DOUBLE_BIAS = True
    cfg_.GRAD_MAX_CLIP = 1.5                         # so that the clip of the apply_update form acts on these gradients
    momentum = float(cfg_.TRAIN.MOMENTUM)
    runs = {}
    for fused in (False, True):
        cfg_.TRAIN.FUSED_UPDATE = fused
        torch.manual_seed(5)
        net = _DeviceStubNet(form)
        solver = train_val.SolverWrapper(net, 2, _Frames(9), output_dir=str(tmp_path / ("fused" if fused else "torch")),
                                         batch_size=2, sum_size=0, log=lambda *_: None)
        losses = solver.train_model(14)
        torch.cuda.synchronize()
        assert len(losses) == 14 and len(net.updates) == 7
        assert isinstance(solver.optimizer.optimizer, train_val.FusedSGD if fused else torch.optim.SGD)
        assert hasattr(solver.optimizer, "fused_update") == fused
        runs[fused] = (net, solver)
    (net_t, solver_t), (net_f, solver_f) = runs[False], runs[True]
    base = cfg_.TRAIN.LEARNING_RATE
    assert [round(r["lr"][0] / base, 6) for r in net_f.updates] == [1, 1, 1, 0.1, 0.1, 0.1, 0.01]
    assert solver_f.optimizer.optimizer.uploads == 3
    budget = [np.zeros(tuple(p.shape)) for p in net_t.parameters()]
    clipped = 0
    for k, (rt, rf) in enumerate(zip(net_t.updates, net_f.updates)):
        assert rt["lr"] == rf["lr"] and rt["wd"] == rf["wd"]
        for i in range(len(budget)):
            assert torch.equal(rt["g"][i], rf["g"][i]), (k, i)           # the gradients do not depend on the weights
            assert float(rf["grad_after"][i].abs().max()) == 0.0 and float(rt["grad_after"][i].abs().max()) == 0.0
            p, g, b = (rt[key][i].double().cpu().numpy() for key in ("p", "g", "b"))
            if form == "apply_update":
                clipped += int((np.abs(g) > cfg_.GRAD_MAX_CLIP).sum())
                g = np.clip(g, -cfg_.GRAD_MAX_CLIP, cfg_.GRAD_MAX_CLIP)
            S = momentum * np.abs(b) + np.abs(g) + rt["wd"][i] * np.abs(p)
            budget[i] += 8 * U * (np.abs(p) + rt["lr"][i] * S)
            err = np.abs(rt["after"][i].double().cpu().numpy() - rf["after"][i].double().cpu().numpy())
            assert np.isfinite(err).all() and (err <= budget[i]).all(), (form, k, i, float((err / budget[i]).max()))
        assert any(not torch.equal(a, b) for a, b in zip(rt["p"], rt["after"]))
    assert form != "apply_update" or clipped > 0
    # state_dict() has torch.optim.SGD's layout: fused -> a fresh torch optimizer, and torch -> the fused one
    fused_opt, torch_opt = solver_f.optimizer.optimizer, solver_t.optimizer.optimizer
    fresh = torch.optim.SGD(train_val.sgd_param_groups(net_f), momentum=momentum)
    fresh.load_state_dict(solver_f.optimizer.state_dict())
    for p in net_f.parameters():
        assert torch.equal(fresh.state[p]["momentum_buffer"], fused_opt.state[p]["momentum_buffer"])
        assert float(fresh.state[p]["momentum_buffer"].abs().max()) > 0
    assert [g["lr"] for g in fresh.param_groups] == [g["lr"] for g in fused_opt.param_groups]
    for p in net_f.parameters():                         # the loaded torch optimizer steps
        p.grad = torch.ones_like(p)
    fresh.step()
    views = [fused_opt.state[p]["momentum_buffer"].data_ptr() for p in net_f.parameters()]
    fused_opt.load_state_dict(torch_opt.state_dict())
    torch.cuda.synchronize()
    for pf, pt, ptr in zip(net_f.parameters(), net_t.parameters(), views):
        buf = fused_opt.state[pf]["momentum_buffer"]
        assert buf.data_ptr() == ptr and torch.equal(buf, torch_opt.state[pt]["momentum_buffer"])       # copied INTO the views
    assert [g["lr"] for g in fused_opt.param_groups] == [g["lr"] for g in torch_opt.param_groups]


# ----------------------------------------------------------------------------------------------------------------------
# a real network
# ----------------------------------------------------------------------------------------------------------------------
def test_captured_training_step_with_fused_update(hip):
    """ResNet-101 + FPN at the 256 x 320 frame of tests/test_train_graphs.py: one pseudo batch of two frames through a
    captured step (enable_train_graphs), then apply_update(in_place=True).  The two frames' gradients and the weights they
    were computed from are kept, and the SAME gradients are stepped from the SAME weights twice in this net - through the
    existing path (clamp per parameter, torch.optim.SGD, zero) and through FusedSGD - because two runs of the backward pass
    differ in the last bits (float atomics of roi_align_bwd), which is more than the rounding bound of the update.  Then:
    parameters within the bound of test_same_optimizer_as_torch_sgd_with_clamp, every derived filter equal to a fresh
    derivation, the bucket all zero, and a third frame replays the captured step."""
    import test_gpu_parity as T
    from faster_rcnn_pytorch_multimodal_amd.model import config as C
    from faster_rcnn_pytorch_multimodal_amd.model import train_val
    net, _ = T._build_fpn_pair(seed=23)
    try:
        data, info, gt, _, _ = T._fpn_case()
        net.train()
        groups = train_val.sgd_param_groups(net)
        params = [p for g in groups for p in g["params"]]
        bucket = train_val.GradientBucket(params)
        momentum = float(C.cfg.TRAIN.MOMENTUM)
        clip = float(C.cfg.GRAD_MAX_CLIP)
        opt_t = train_val.DataParallelOptimizer(torch.optim.SGD(train_val.sgd_param_groups(net), momentum=momentum), bucket)
        opt_f = train_val.DataParallelOptimizer(train_val.FusedSGD(groups, bucket, momentum=momentum), bucket)
        assert hasattr(opt_f, "fused_update") and not hasattr(opt_t, "fused_update")
        net.enable_train_graphs(True)
        rng = np.random.default_rng(9)
        frames = [data, (rng.standard_normal(data.shape) * 50).astype(np.float32), data * 0.5]
        for it in range(2):
            torch.manual_seed(100 + it)
            blobs = {"data": frames[it], "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
            assert np.isfinite(net.train_step(blobs, opt_f, update_weights=False))
        torch.cuda.synchronize()
        assert len(net._train_graphs) == 1
        w0 = [p.detach().clone() for p in params]
        g0 = bucket.flat.clone()
        assert float(g0.abs().max()) > 0 and all(p.grad.data_ptr() == bucket.flat.data_ptr() + 4 * o for p, o in
                                                 zip(params, np.concatenate(([0], np.cumsum([p.numel() for p in params])[:-1]))))
        net.apply_update(opt_t, in_place=True)                      # the existing path
        torch.cuda.synchronize()
        w_ref = [p.detach().clone() for p in params]
        with torch.no_grad():
            for p, w in zip(params, w0):
                p.copy_(w)
            bucket.flat.copy_(g0)
        bucket.fault.fill_(1.0)                                      # the slot behind the gradients is cleared too
        # the derived filters are made current for the restored weights, so that only the fused update's own bump of the
        # version counters (the kernel writes through raw pointers) can make after_optimizer_step re-derive them below
        from faster_rcnn_pytorch_multimodal_amd.model.train_graph import after_optimizer_step
        after_optimizer_step(net)
        torch.cuda.synchronize()
        assert T._assert_derived_weights_fresh(net, "before the fused update") > 100
        versions = [p._version for p in params]
        net.apply_update(opt_f, in_place=True)                      # the update kernel
        torch.cuda.synchronize()
        assert all(p._version > v for p, v in zip(params, versions)), "the fused update did not bump a version counter"
        assert not bucket.flat.cpu().numpy().view(np.uint32).any(), "the gradient bucket is not all +0.0"
        assert opt_f._reduced is False
        off, moved = 0, 0
        for grp, p, w, wr in zip(groups, params, w0, w_ref):
            g = g0[off:off + p.numel()].view_as(p).double().clamp(-clip, clip)
            off += p.numel()
            S = g.abs() + grp["weight_decay"] * w.double().abs()               # the momentum buffers start at zero
            tol = 8 * U * (w.double().abs() + grp["lr"] * S)
            err = (p.detach().double() - wr.double()).abs()
            assert bool(torch.isfinite(err).all()) and bool((err <= tol).all()), (tuple(p.shape), float((err / tol.clamp_min(1e-300)).max()))
            moved += int((p.detach() != w).sum())
        assert moved > 0.5 * off
        assert T._assert_derived_weights_fresh(net, "after the fused update") > 100
        torch.manual_seed(102)
        blobs = {"data": frames[2], "info": info, "gt_boxes": gt, "gt_boxes_dc": np.zeros((0, 4), np.float32)}
        assert np.isfinite(net.train_step(blobs, opt_f, update_weights=False))
        torch.cuda.synchronize()
        assert len(net._train_graphs) == 1 and float(bucket.flat.abs().max()) > 0
    finally:
        C.reset_cfg()
