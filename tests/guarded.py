"""Guard bands: a tensor that ends exactly where a poisoned band begins.

Every GPU test hands the kernels fresh `torch.empty` tensors, which the caching allocator rounds up to 512 bytes: a store
one element past an output, a workspace layout one unit short, or a read past an operand's end lands in slack and no
value comparison can see it.  `guarded()` places the payload inside one larger uint8 allocation the test owns, between
two bands of a known byte; `check()` proves the bands still hold it.  Nothing here provokes a fault: every byte a wrong
kernel would touch within a band's reach lies inside that one live allocation.

The poison bytes (POISON_FLOAT for floating operands and outputs, POISON_INDEX for index arrays and workspaces,
POISON_INT_OUT for integer outputs): 0xFF repeated is a NaN in fp16, bf16, fp32 and fp64, so a read past the end that
reaches a result shows up in the value check; index arrays get 0x00 because id 0 is a valid row."""
import numpy as np
import torch

POISON_FLOAT, POISON_INDEX, POISON_INT_OUT = 0xFF, 0x00, 0xA5
FLOAT_SENTINEL, INT_SENTINEL = 9.0, -7      # what the existing tests pre-fill outputs with


class Guarded:
    def __init__(self, buf, t, band, shift, poison):
        self.buf, self.t, self.band, self.shift, self.poison = buf, t, band, shift, poison
        self.nbytes = t.numel() * t.element_size()

    def _bands(self):
        lo = self.buf[: self.band + self.shift]
        hi = self.buf[self.band + self.shift + self.nbytes:]
        return (("leading", lo, -(self.band + self.shift)), ("trailing", hi, self.nbytes))

    def check(self, where=""):
        """Both bands still hold the poison byte (compared on the tensor's device)."""
        bands = self._bands()
        clean = torch.stack([(band == self.poison).all() for _, band, _ in bands]).tolist()     # (one read-back)
        for (name, band, origin), ok in zip(bands, clean):
            if ok:
                continue
            hit = torch.nonzero(band != self.poison).flatten()
            lo, hi = int(hit[0]) + origin, int(hit[-1]) + origin
            raise AssertionError(
                "%s band hit: %d byte(s) changed, payload-relative byte offsets %d .. %d (payload = [0, %d), %s %s, shift %d)"
                " -- %s" % (name, hit.numel(), lo, hi, self.nbytes, tuple(self.t.shape), self.t.dtype, self.shift, where))


def guarded(device, shape, dtype, *, fill=None, poison, shift=0, band=4096):
    """A contiguous tensor `.t` of `shape` / `dtype` that starts `band + shift` bytes into one uint8 allocation of
    band + shift + nbytes + band bytes and ends exactly where the trailing band begins.  `shift` (bytes, a multiple of
    the item size) misaligns the base; 0 keeps it 256-aligned.  `fill` (array or tensor) is copied into `.t`, otherwise
    it holds the type's sentinel."""
    shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    assert band > 0 and band % 256 == 0, "the band is a multiple of 256 bytes"
    assert 0 <= poison <= 0xFF
    if shift < 0 or shift % item:
        raise ValueError("shift (%d bytes) must be a non-negative multiple of the item size (%d)" % (shift, item))
    n = 1
    for s in shape:
        n *= s
    nbytes = n * item
    total = band + shift + nbytes + band
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    if buf.data_ptr() % 256:       # the host allocator aligns to 64 bytes only: the same bytes out of a slightly larger block
        assert buf.device.type == "cpu", "a device allocation whose base is not 256-byte aligned"
        raw = torch.empty(total + 255, dtype=torch.uint8, device=device)
        lead = -raw.data_ptr() % 256
        buf = raw[lead: lead + total]
    assert buf.data_ptr() % 256 == 0 and buf.numel() == total, "the allocation's base is not 256-byte aligned"
    buf.fill_(poison)
    t = buf[band + shift: band + shift + nbytes].view(dtype).view(shape)
    assert t.is_contiguous() and t.storage_offset() * item == buf.storage_offset() + band + shift
    if nbytes:                     # (torch reports no address for a tensor without elements)
        assert t.data_ptr() == buf.data_ptr() + band + shift and t.data_ptr() + nbytes == buf.data_ptr() + total - band
    if fill is not None:
        src = fill if isinstance(fill, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fill))
        assert src.dtype == dtype and src.numel() == n, (src.dtype, dtype, tuple(src.shape), shape)
        t.copy_(src.reshape(shape))
    elif dtype == torch.uint8:
        t.zero_()                                   # (a workspace: its own poison, nothing to claim)
    elif dtype.is_floating_point:
        t.fill_(FLOAT_SENTINEL)
    else:
        t.fill_(INT_SENTINEL)
    return Guarded(buf, t, band, shift, poison)
