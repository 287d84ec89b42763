"""Self-test of tests/guarded.py on CPU tensors: the harness fails when it should, without a GPU and without a kernel."""
import pytest
import torch

from tests.guarded import POISON_FLOAT, POISON_INDEX, POISON_INT_OUT, guarded

CPU = torch.device("cpu")
FLOATS = [torch.float16, torch.bfloat16, torch.float32, torch.float64]


def _item(dtype):
    return torch.empty((), dtype=dtype).element_size()


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32, torch.int64])
@pytest.mark.parametrize("shift_elems", [0, 1, 3])
def test_layout(dtype, shift_elems):
    item = _item(dtype)
    g = guarded(CPU, (5, 3), dtype, poison=POISON_FLOAT, shift=shift_elems * item, band=512)
    assert g.buf.dtype == torch.uint8 and g.buf.numel() == 512 + shift_elems * item + 15 * item + 512
    assert g.buf.data_ptr() % 256 == 0
    assert g.t.data_ptr() == g.buf.data_ptr() + 512 + shift_elems * item
    assert g.t.is_contiguous() and g.t.shape == (5, 3) and g.t.dtype == dtype
    # the payload ends exactly where the trailing band begins: no rounding
    assert g.t.data_ptr() + 15 * item == g.buf.data_ptr() + g.buf.numel() - 512
    assert (g.t == (9.0 if dtype.is_floating_point else -7)).all()
    g.check("untouched")


def test_default_band_and_fill():
    want = torch.arange(12, dtype=torch.int64).view(3, 4)
    g = guarded(CPU, (3, 4), torch.int64, fill=want.numpy(), poison=POISON_INDEX)
    assert g.band == 4096 and g.buf.numel() == 4096 + 96 + 4096
    assert torch.equal(g.t, want)
    assert g.t.data_ptr() == g.buf.data_ptr() + 4096
    g.t.fill_(123)                       # writing the whole payload is what a kernel is allowed to do
    g.check("payload written")
    assert (g.buf[:4096] == 0).all() and (g.buf[4096 + 96:] == 0).all()


@pytest.mark.parametrize("dtype", FLOATS + [torch.int32])
@pytest.mark.parametrize("shift_elems", [0, 1])
def test_one_element_past_the_end_is_caught(dtype, shift_elems):
    item = _item(dtype)
    shift = shift_elems * item
    g = guarded(CPU, 7, dtype, poison=POISON_INT_OUT, shift=shift, band=256)
    end = 256 + shift + 7 * item
    g.buf[end: end + item].view(dtype)[0] = 1            # the element right behind the payload
    with pytest.raises(AssertionError) as err:
        g.check("overrun by one")
    msg = str(err.value)
    assert "trailing band" in msg and "overrun by one" in msg
    assert "offsets %d .. %d " % (7 * item, 8 * item - 1) in msg     # (no byte of a 1 in any of these types is 0xA5)


@pytest.mark.parametrize("dtype", FLOATS + [torch.int64])
@pytest.mark.parametrize("shift_elems", [0, 3])
def test_one_element_before_the_start_is_caught(dtype, shift_elems):
    item = _item(dtype)
    shift = shift_elems * item
    g = guarded(CPU, (2, 3), dtype, poison=POISON_FLOAT, shift=shift, band=256)
    start = 256 + shift
    g.buf[start - item: start].view(dtype)[0] = 1        # the element right in front of the payload
    with pytest.raises(AssertionError) as err:
        g.check("underrun by one")
    msg = str(err.value)
    assert "leading band" in msg and "underrun by one" in msg
    assert "offsets %d .. -1 " % -item in msg             # (no byte of a 1 in any of these types is 0xFF)


def test_reported_offsets_are_relative_to_the_payload():
    g = guarded(CPU, 10, torch.float32, poison=POISON_FLOAT, band=256)
    g.buf[256 + 40 + 4] = 0
    g.buf[256 + 40 + 19] = 0
    with pytest.raises(AssertionError, match=r"trailing band hit: 2 byte\(s\) changed, payload-relative byte offsets 44 \.\. 59 "):
        g.check()
    g = guarded(CPU, 10, torch.float32, poison=POISON_FLOAT, shift=4, band=256)
    g.buf[256 + 4 - 1] = 0
    g.buf[0] = 0
    with pytest.raises(AssertionError, match=r"leading band hit: 2 byte\(s\) changed, payload-relative byte offsets -260 \.\. -1 "):
        g.check()


@pytest.mark.parametrize("dtype", FLOATS)
def test_the_float_poison_reads_as_nan(dtype):
    item = _item(dtype)
    for shift in (0, item):
        g = guarded(CPU, 6, dtype, poison=POISON_FLOAT, shift=shift, band=256)
        end = 256 + shift + 6 * item
        assert torch.isnan(g.buf[end: end + item].view(dtype)[0])
        assert torch.isnan(g.buf[256 + shift - item: 256 + shift].view(dtype)[0])
        assert not torch.isnan(g.t).any()


@pytest.mark.parametrize("dtype,shift", [(torch.float32, 2), (torch.float64, 4), (torch.float16, 1), (torch.int64, 12)])
def test_a_shift_that_splits_an_element_is_refused(dtype, shift):
    with pytest.raises(ValueError, match="multiple of the item size"):
        guarded(CPU, 4, dtype, poison=POISON_FLOAT, shift=shift)


def test_a_band_that_is_no_multiple_of_256_is_refused():
    with pytest.raises(AssertionError):
        guarded(CPU, 4, torch.float32, poison=POISON_FLOAT, band=100)


def test_empty_payload_and_workspace():
    g = guarded(CPU, 0, torch.float32, poison=POISON_FLOAT, band=256)
    assert g.t.numel() == 0 and g.buf.numel() == 512
    g.check()
    g.buf[256] = 0                                       # with no payload the two bands meet: any write is caught
    with pytest.raises(AssertionError, match="trailing band"):
        g.check()
    ws = guarded(CPU, 100, torch.uint8, poison=POISON_INDEX, band=256)
    assert ws.t.numel() == 100 and ws.t.data_ptr() == ws.buf.data_ptr() + 256
    ws.buf[256 + 100] = 1                                # a layout one byte short
    with pytest.raises(AssertionError, match="trailing band"):
        ws.check()
