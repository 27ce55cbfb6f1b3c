"""Fenced and poisoned buffers for the GPU tests: what a kernel does to memory it does not own, and which elements of
its outputs it forgets.  No tests here: tests/test_fences_cpu.py holds the helper itself to its word without a GPU,
tests/test_gpu_env_fences.py, tests/test_gpu_fences.py and tests/test_gpu_il_fences.py run the kernels on it.

Fenced(shape, dtype) is a tensor `t` that is the interior of a uint8 buffer with MARGIN bytes of 0xFF on either side.
In 0xFF bytes float32 and float64 are NaN, int32 and int64 are -1 and uint8 is 255, so

  * a write outside the buffer flips intact();
  * a read outside a float buffer brings a NaN into whatever it is summed into;
  * an index read outside an int32 buffer (idx, perm, act_src) is -1, and a gather through it from a fenced table
    lands in that table's front margin and reads NaN there, not memory further away.  That holds while one row of the
    table is at most MARGIN bytes; pass gathered=True for a table that is gathered from, which asserts it;
  * with init=None the interior is poisoned with the same bytes, and unwritten() counts the elements a kernel left as
    they were: no element that was stored, whatever the value, has all its bytes 0xFF unless the kernel stored exactly
    the poison (a NaN with every mantissa bit set, or -1), which no output compared in these tests may hold.  A uint8
    element is one byte, so a stored 255 reads as unwritten: count a byte buffer of records by the record (see K23 in
    tests/test_gpu_fences.py) and use unwritten() on flag bytes only where 255 is no flag value.

The interior starts ALIGN-byte aligned, so the alignment the entry points ask of their operands (16 bytes in
oly_ppo_update_grads, 8 in the K24 entries) holds as it does for a tensor of torch's own.  With skew=k (bytes, a
multiple of the element size, below ALIGN) it starts k bytes after an ALIGN boundary instead, between the same two
MARGIN-byte margins: a skew of one float32 sends an entry point that picks its vector kernel by the pointer's alignment
down its scalar path, on fenced operands.

fence_engine(eng) does the same to every tensor the Engine allocates for its caller while the context is open.

Bufs is the {name: Fenced} of one case that the GPU tests fill and close with done().

What runs fenced: K1-K9, the expert-data entries and the two host batchers in tests/test_gpu_env_fences.py, K10-K14,
K23 and K24 in tests/test_gpu_fences.py, K15-K22 and K25 in tests/test_gpu_il_fences.py, K26 in tests/test_gpu_iq_q.py,
K27 in tests/test_gpu_iq_pi.py; tests/il_fence_ledger.py names the test of every entry point of the header, and
tests/test_il_fence_ledger_cpu.py holds that table to the header without a GPU.

New tests use this helper.  The two older ones stay as they are, and only in the tests that already have them: `_Guard`
in tests/test_gpu_parity.py (margins only, the engine's allocations of K1-K9) and `il_shapes.Guarded` (a float sentinel,
zeroed interior, around some outputs of the imitation-learning kernels' own test files)."""
import contextlib

import numpy as np
import torch

MARGIN = 4096        # bytes on each side, the size _Guard uses
ALIGN = 256          # of the interior's first byte
POISON = 0xFF


class Fenced:
    def __init__(self, shape, dtype, device="cuda", init=None, gathered=False, skew=0):
        shape = (shape,) if isinstance(shape, int) else tuple(int(s) for s in shape)
        self.shape, self.dtype = shape, dtype
        self.n = int(np.prod(shape, dtype=np.int64))
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = self.n * self.item
        if gathered:
            pitch = (self.n // shape[0] if shape and shape[0] else 0) * self.item
            assert pitch <= MARGIN, f"a row of {pitch} bytes: a gather through index -1 would pass the {MARGIN}-byte fence"
        self.skew = int(skew)
        assert 0 <= self.skew < ALIGN and self.skew % self.item == 0, f"a skew of {skew} bytes for {self.item}-byte elements"
        raw = torch.full((self.nbytes + 2 * MARGIN + 2 * ALIGN,), POISON, dtype=torch.uint8, device=device)
        start = MARGIN + (-(raw.data_ptr() + MARGIN)) % ALIGN + self.skew
        self.buf = raw[start - MARGIN:start + self.nbytes + MARGIN]       # margin | interior | margin
        self.bytes = self.buf[MARGIN:MARGIN + self.nbytes]
        self.t = self.bytes.view(dtype).view(shape)
        assert self.t.data_ptr() % ALIGN == self.skew and self.t.is_contiguous()
        if init is not None:
            src = torch.as_tensor(np.ascontiguousarray(init) if isinstance(init, np.ndarray) else init)
            assert src.numel() == self.n, (tuple(src.shape), shape)
            self.t.copy_(src.to(device=device, dtype=dtype).reshape(shape))

    def margins(self):
        return self.buf[:MARGIN], self.buf[MARGIN + self.nbytes:]

    def intact(self):
        """Both margins are still all 0xFF."""
        lo, hi = self.margins()
        return bool((lo == POISON).all()) and bool((hi == POISON).all())

    def unwritten(self):
        """The number of interior elements whose bytes are all still 0xFF."""
        if self.n == 0:
            return 0
        return int((self.bytes.view(self.n, self.item) == POISON).all(dim=1).sum())

    def snapshot(self):
        """A copy of margins and interior, for same_as()."""
        return self.buf.clone()

    def same_as(self, snap):
        return bool(torch.equal(self.buf, snap))


def fenced(a, device="cuda", dtype=None, gathered=False, skew=0):
    """A Fenced copy of the array or tensor `a` (None stays None)."""
    if a is None:
        return None
    src = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
    return Fenced(tuple(src.shape), dtype or src.dtype, device, init=src, gathered=gathered, skew=skew)


def broken(bufs):
    """bufs: {name: Fenced or None}; the names whose margins were written."""
    return [k for k, f in bufs.items() if f is not None and not f.intact()]


def assert_intact(bufs, what=""):
    bad = broken(bufs)
    assert not bad, f"{what}: written outside {bad}"


def assert_written(bufs, what=""):
    """Every buffer of {name: Fenced} is fully written."""
    left = {k: f.unwritten() for k, f in bufs.items() if f is not None and f.unwritten()}
    assert not left, f"{what}: elements never stored {left}"


def assert_untouched(bufs, what=""):
    """Every poisoned buffer of {name: Fenced} is still wholly poisoned and every margin intact."""
    assert_intact(bufs, what)
    hit = {k: f.n - f.unwritten() for k, f in bufs.items() if f is not None and f.unwritten() != f.n}
    assert not hit, f"{what}: elements stored {hit}"


class Bufs(dict):
    """{name: Fenced} of one case."""

    def inp(self, name, a, **kw):
        """A fenced copy of the array `a` (None stays None); returns the tensor."""
        if a is None:
            return None
        assert name not in self, name
        self[name] = fenced(a, **kw)
        return self[name].t

    def out(self, name, shape, dtype, skew=0):
        """A fenced, poisoned tensor."""
        assert name not in self, name
        self[name] = Fenced(shape, dtype, skew=skew)
        return self[name].t

    def host(self, name):
        return self[name].t.cpu().numpy()

    def done(self, what, written=(), finite=()):
        torch.cuda.synchronize()
        assert_intact(self, what)
        assert_written({k: self[k] for k in written}, what)
        for k in finite:
            t = self[k].t
            assert not t.dtype.is_floating_point or not bool(torch.isnan(t).any()), (what, k, "holds a NaN")


class EngineFence:
    """What fence_engine yields: the allocations made so far, in order."""

    def __init__(self):
        self.bufs = []

    def check(self, what=""):
        """Every margin of every allocation is intact; the message names the buffer."""
        for i, f in enumerate(self.bufs):
            assert f.intact(), f"{what}: written outside allocation {i}, {f.shape} {f.dtype}"

    def unwritten(self):
        """[(allocation number, shape, elements never stored)] for every allocation."""
        return [(i, f.shape, f.unwritten()) for i, f in enumerate(self.bufs)]

    def of(self, t):
        """The Fenced behind a tensor the engine returned (or a view of one that starts at its first element)."""
        for f in self.bufs:
            if f.t.data_ptr() == t.data_ptr() and f.n:
                return f
        raise KeyError("not a tensor allocated inside fence_engine")


@contextlib.contextmanager
def fence_engine(eng):
    """Inside the context every tensor `eng` allocates (Engine._new) is fenced and poisoned."""
    ef = EngineFence()

    def new(shape, dtype):
        f = Fenced(shape, dtype, eng.device)
        ef.bufs.append(f)
        return f.t

    had = "_new" in eng.__dict__
    keep = eng.__dict__.get("_new")
    eng._new = new
    try:
        yield ef
    finally:
        if had:
            eng._new = keep
        else:
            del eng._new
