"""tests/bf16_train_restatement.py against plain float64 autograd (no GPU)."""
import torch
import torch.nn.functional as F

import bf16_train_restatement as R


def test_exact_operands_equal_plain_autograd():
    """Integer operands in [-3, 3] (exact in bf16, every sum exact in float64): the function and both gradients equal plain
    float64 conv2d autograd bit for bit, for every stride / padding / rounding form used."""
    gen = torch.Generator().manual_seed(5)
    for (n, c, h, w, k, r, stride, pad) in ((1, 32, 5, 7, 32, 3, 1, 1), (2, 96, 4, 4, 32, 1, 2, 0), (1, 32, 9, 11, 64, 3, 2, 1)):
        for round_dgrad in (True, False):
            x = torch.randint(-3, 4, (n, c, h, w), generator=gen).double().requires_grad_(True)
            wt = torch.randint(-3, 4, (k, c, r, r), generator=gen).double().requires_grad_(True)
            y0 = F.conv2d(x, wt, None, stride, pad)
            g = torch.randint(-3, 4, tuple(y0.shape), generator=gen).double()
            gx0, gw0 = torch.autograd.grad((y0 * g).sum(), (x, wt))
            y1 = R.conv_bf16(x, wt, stride, pad, round_dgrad)
            gx1, gw1 = torch.autograd.grad((y1 * g).sum(), (x, wt))
            assert torch.equal(y0, y1) and torch.equal(gx0, gx1) and torch.equal(gw0, gw1)


def test_rounding_is_there():
    """On operands bf16 does not represent the function differs from the plain product by no more than two roundings."""
    gen = torch.Generator().manual_seed(6)
    x = torch.randn((1, 32, 6, 6), generator=gen).double()
    w = torch.randn((32, 32, 3, 3), generator=gen).double()
    y0, y1 = F.conv2d(x, w, None, 1, 1), R.conv_bf16(x, w, 1, 1)
    bound = 2.0 ** -7 * F.conv2d(x.abs(), w.abs(), None, 1, 1)
    assert not torch.equal(y0, y1) and bool(((y0 - y1).abs() <= bound).all())
