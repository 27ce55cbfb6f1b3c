"""tests/fences.py held to its word without a GPU: a fence that does not notice a stray write, or a poison that does
not count the elements left unstored, would let every test built on it pass for nothing."""
import numpy as np
import pytest
import torch

import fences as fn

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8)
IDS = [str(t).split(".")[1] for t in DTYPES]


def outside(f, k):
    """The element of f's dtype that lies k elements before (k < 0) or k - 1 elements after the interior."""
    lo = fn.MARGIN + (k * f.item if k < 0 else f.nbytes + (k - 1) * f.item)
    return f.buf[lo:lo + f.item].view(f.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(1,), (7,), (5, 3), (0,)])
def test_a_write_next_to_the_interior_flips_intact(dtype, shape):
    for where in (-1, 1):
        f = fn.Fenced(shape, dtype, device="cpu")
        assert f.intact()
        f.t.fill_(0)                               # the whole interior, to its first and last byte
        assert f.intact(), "a write to the interior is no write outside it"
        outside(f, where).fill_(0)
        assert not f.intact(), where
    # one byte, the first of the front margin and the last of the back one
    for at in (0, -1):
        f = fn.Fenced(shape, dtype, device="cpu")
        f.buf[at] = 0xFE
        assert not f.intact()
    assert len(f.margins()[0]) == fn.MARGIN and len(f.margins()[1]) == fn.MARGIN


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unwritten_counts_exactly_the_elements_not_stored(dtype):
    f = fn.Fenced((6, 5), dtype, device="cpu")
    assert f.unwritten() == 30
    f.t[1, 2] = 0
    assert f.unwritten() == 29
    f.t[:4] = 3
    assert f.unwritten() == 10
    f.t[5, 4] = 1                                  # the last element
    f.t[4, 0] = 1
    assert f.unwritten() == 8 and f.intact()
    # an element of which only some bytes were stored counts as written
    if f.item > 1:
        g = fn.Fenced(4, dtype, device="cpu")
        g.bytes[g.item] = 0                        # one byte of element 1
        assert g.unwritten() == 3
    f.t.fill_(2)
    assert f.unwritten() == 0
    assert fn.Fenced(0, dtype, device="cpu").unwritten() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [1, 3, 17, 1000])
def test_alignment_shape_and_poison(dtype, n):
    f = fn.Fenced((n, 3), dtype, device="cpu")
    assert f.t.data_ptr() % fn.ALIGN == 0 and fn.ALIGN % 16 == 0
    assert f.t.shape == (n, 3) and f.t.dtype == dtype and f.t.is_contiguous()
    assert f.t.data_ptr() == f.buf.data_ptr() + fn.MARGIN
    lo, hi = outside(f, -1), outside(f, 1)
    if dtype.is_floating_point:
        assert bool(torch.isnan(f.t).all()) and bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    elif dtype == torch.uint8:
        assert bool((f.t == 255).all()) and int(lo) == 255 and int(hi) == 255
    else:
        assert bool((f.t == -1).all()) and int(lo) == -1 and int(hi) == -1


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_init_is_copied_in_and_leaves_the_margins(dtype):
    a = (np.arange(12).reshape(4, 3) % 7).astype(np.float64)
    f = fn.Fenced((4, 3), dtype, device="cpu", init=a)
    assert torch.equal(f.t, torch.as_tensor(a).to(dtype)) and f.intact() and f.unwritten() == 0
    g = fn.fenced(torch.as_tensor(a).to(dtype), device="cpu")
    assert torch.equal(g.t, f.t) and g.t.dtype == dtype and g.intact()
    assert fn.fenced(None) is None
    with pytest.raises(AssertionError):
        fn.Fenced((4, 4), dtype, device="cpu", init=a)


def test_snapshot_sees_every_byte():
    f = fn.Fenced(9, torch.float32, device="cpu", init=np.arange(9.0))
    s = f.snapshot()
    assert f.same_as(s)
    f.t[4] = 4.0                                   # the same value: the same bytes
    assert f.same_as(s)
    f.t[4] = 5.0
    assert not f.same_as(s)
    f.t[4] = 4.0
    f.buf[-1] = 0
    assert not f.same_as(s)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("elems", [1, 3])
def test_a_skewed_interior_starts_where_it_was_asked_to(dtype, elems):
    """skew=k: the interior starts k bytes after an ALIGN boundary, between the same two margins of poison."""
    item = torch.empty(0, dtype=dtype).element_size()
    skew = elems * item
    f = fn.Fenced((5, 3), dtype, device="cpu", skew=skew)
    assert f.t.data_ptr() % fn.ALIGN == skew and f.skew == skew
    assert f.t.shape == (5, 3) and f.t.dtype == dtype and f.t.is_contiguous()
    assert f.t.data_ptr() == f.buf.data_ptr() + fn.MARGIN
    lo, hi = f.margins()
    assert len(lo) == fn.MARGIN and len(hi) == fn.MARGIN and len(f.buf) == 2 * fn.MARGIN + f.nbytes
    assert bool((f.buf == fn.POISON).all()) and f.intact() and f.unwritten() == 15
    if item == 4:
        assert f.t.data_ptr() % 16 == (4 if elems == 1 else 12)
    # intact(), unwritten() and same_as() as on an aligned interior
    f.t.fill_(0)
    assert f.intact() and f.unwritten() == 0
    g = fn.Fenced((5, 3), dtype, device="cpu", skew=skew)
    g.t[1, 2] = 0
    g.t[4, 2] = 0                                  # the last element
    assert g.unwritten() == 13 and g.intact()
    s = g.snapshot()
    assert g.same_as(s)
    g.t[0, 0] = 1
    assert not g.same_as(s)
    # one byte just before and one byte just after the interior
    for at in (fn.MARGIN - 1, fn.MARGIN + f.nbytes):
        h = fn.Fenced((5, 3), dtype, device="cpu", skew=skew)
        h.t.fill_(0)
        assert h.intact()
        h.buf[at] = 0xFE
        assert not h.intact(), at
    for where in (-1, 1):
        h = fn.Fenced((5, 3), dtype, device="cpu", skew=skew)
        outside(h, where).fill_(0)
        assert not h.intact(), where
    # fenced() and Bufs pass it on; the default is no skew
    a = (np.arange(15).reshape(5, 3) % 7).astype(np.float64)
    k = fn.fenced(torch.as_tensor(a).to(dtype), device="cpu", skew=skew)
    assert k.t.data_ptr() % fn.ALIGN == skew and torch.equal(k.t, torch.as_tensor(a).to(dtype)) and k.intact()
    assert fn.Fenced(3, dtype, device="cpu").skew == 0


def test_a_skew_is_whole_elements_below_the_alignment():
    for dtype, skew in ((torch.float32, 2), (torch.float64, 4), (torch.float32, fn.ALIGN), (torch.float32, -4)):
        with pytest.raises(AssertionError):
            fn.Fenced(4, dtype, device="cpu", skew=skew)


def test_a_gathered_table_is_held_to_the_row_pitch():
    fn.Fenced((3, 1024), torch.float32, device="cpu", gathered=True)            # 4096 bytes
    with pytest.raises(AssertionError, match="4096"):
        fn.Fenced((3, 1025), torch.float32, device="cpu", gathered=True)
    with pytest.raises(AssertionError):
        fn.Fenced((3, 513), torch.float64, device="cpu", gathered=True)
    # row -1 of a fenced table lies wholly inside its front margin
    f = fn.Fenced((3, 1024), torch.float32, device="cpu", init=np.zeros((3, 1024)), gathered=True)
    row = f.buf[fn.MARGIN - 4096:fn.MARGIN].view(torch.float32)
    assert bool(torch.isnan(row).all())


def test_the_assertions_name_the_buffer():
    a, b = fn.Fenced(4, torch.float32, device="cpu"), fn.Fenced(4, torch.int32, device="cpu")
    bufs = dict(a=a, b=b, c=None)
    fn.assert_intact(bufs)
    fn.assert_untouched(bufs)
    a.t[:3] = 1.0
    with pytest.raises(AssertionError, match=r"'a': 1"):
        fn.assert_written(dict(a=a), "case")
    with pytest.raises(AssertionError, match=r"'a': 3"):
        fn.assert_untouched(bufs)
    b.t.fill_(0)
    fn.assert_written(dict(b=b))
    b.buf[0] = 0
    assert fn.broken(bufs) == ["b"]
    with pytest.raises(AssertionError, match="b"):
        fn.assert_intact(bufs, "case")


class _Eng:
    device = torch.device("cpu")

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype)


def test_fence_engine_swaps_the_allocator_and_puts_it_back():
    e = _Eng()
    with fn.fence_engine(e) as ef:
        x = e._new((3, 2), torch.float64)
        y = e._new(5, torch.int32)
        assert bool(torch.isnan(x).all()) and bool((y == -1).all()) and x.data_ptr() % fn.ALIGN == 0
        ef.check("fresh")
        assert ef.unwritten() == [(0, (3, 2), 6), (1, (5,), 5)]
        x.fill_(1.0)
        y[:2] = 0
        assert ef.unwritten() == [(0, (3, 2), 0), (1, (5,), 3)]
        assert ef.of(y).unwritten() == 3 and ef.of(x) is ef.bufs[0]
        with pytest.raises(KeyError):
            ef.of(torch.zeros(1))
        ef.bufs[1].buf[fn.MARGIN + 20] = 0                    # the byte behind y's last element
        with pytest.raises(AssertionError, match=r"later: written outside allocation 1, \(5,\) torch.int32"):
            ef.check("later")
    assert "_new" not in e.__dict__, "the class's own allocator is back"
    z = e._new((2,), torch.float32)
    assert z.shape == (2,) and z.data_ptr() not in [f.t.data_ptr() for f in ef.bufs]
