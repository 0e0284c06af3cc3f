"""Device buffers between NaN guard bands, shared by the convolution tests (test_conv_wgrad_bf16.py, test_conv_dgrad_bf16.py,
test_conv_f32_exact.py): a kernel's output or workspace is a view in the middle of one allocation whose first and last
``guard`` floats hold NaN.  A store outside the view lands in a band (or, past a band, in memory the test owns nothing of - so
the bands are made wide enough for the overrun one looks for); a view pre-filled with NaN shows every element that was not
written, and a NaN workspace turns a read of something never written into a NaN downstream."""

DEV = "cuda:0"
GUARD = 64


def guarded(numel, fill=float("nan"), guard=GUARD):
    """(buffer, view of ``numel`` floats between two ``guard``-float NaN bands), the view filled with ``fill``."""
    import torch
    buf = torch.full((numel + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[guard:guard + numel]
    view.fill_(fill)
    return buf, view


def guards_flag(buf, numel, guard=GUARD):
    """Are both bands still all NaN?  A 0-dim bool tensor on the device (no synchronisation)."""
    import torch
    return torch.isnan(buf[:guard]).all() & torch.isnan(buf[guard + numel:]).all()


def guards_intact(buf, numel, guard=GUARD):
    return bool(guards_flag(buf, numel, guard))
