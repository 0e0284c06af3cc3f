"""Device buffers between NaN guard bands, shared by the convolution tests (test_conv_wgrad_bf16.py, test_conv_dgrad_bf16.py,
test_conv_f32_exact.py): a kernel's output or workspace is a view in the middle of one allocation whose first and last
``guard`` floats hold NaN.  A store outside the view lands in a band (or, past a band, in memory the test owns nothing of - so
the bands are made wide enough for the overrun one looks for); a view pre-filled with NaN shows every element that was not
written, and a NaN workspace turns a read of something never written into a NaN downstream.  The byte-level form at the end
(ByteGuarded) does the same for the integer outputs and workspaces of the index-producing kernels (test_index_edges.py)."""

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


# ------------------------------------------------------------------------------------------------
# Byte-level form for the index-producing kernels (test_index_edges.py), whose outputs are int64 / int32 / uint8 / float32:
# a view of exactly ``nbytes`` bytes between two bands of BAND_BYTE.  The bands are a multiple of 256 bytes long, so a view
# at offset 0 keeps the 16-byte alignment of the allocation; ``offset`` (< 16) moves the view off it on purpose and the
# front band grows by as much.
# ------------------------------------------------------------------------------------------------
BAND = 1024
BAND_BYTE = 0xA5
OUT_BYTE = 0xC3          # pre-fill of an output: an element that still reads 0xC3C3... was never written
POISON_BYTE = 0xFF       # pre-fill of a workspace: every suppression bit set, every float a NaN


class ByteGuarded:
    """``view``: uint8 tensor of ``nbytes`` bytes filled with ``fill``, between two BAND_BYTE bands of one allocation."""

    def __init__(self, nbytes, fill=OUT_BYTE, offset=0, band=BAND):
        import torch
        assert band % 256 == 0 and 0 <= offset < 16
        self.nbytes, self.front = int(nbytes), band + offset
        self.buf = torch.full((self.front + self.nbytes + band,), BAND_BYTE, dtype=torch.uint8, device=DEV)
        self.view = self.buf[self.front:self.front + self.nbytes]
        self.view.fill_(fill)

    @property
    def ptr(self):
        """Address of the view (valid for an empty view too)."""
        return self.buf.data_ptr() + self.front

    def typed(self, dtype, shape=(-1,)):
        return self.view.view(dtype).view(*shape)

    def intact(self):
        """Do both bands still hold BAND_BYTE everywhere?"""
        end = self.front + self.nbytes
        return bool((self.buf[:self.front] == BAND_BYTE).all()) and bool((self.buf[end:] == BAND_BYTE).all())


def guarded_like(dtype, numel, fill=OUT_BYTE, offset=0):
    """A ByteGuarded holding ``numel`` elements of ``dtype``."""
    import torch
    return ByteGuarded(numel * torch.empty((), dtype=dtype).element_size(), fill, offset)
