"""Buffers between guard bands, for the tests of kernels that write through raw pointers (plain module: no fixture, no pytest setting).

    t = guarded(shape, dtype, device, src=None)

is a contiguous tensor that is a view into a larger uint8 arena.  The whole arena is 0xFF bytes (NaN in fp32 and in bf16, -1 in the integer
types), the tensor starts at a multiple of 512 bytes from the arena's start -- the alignment torch's allocator gives, so no kernel takes
another path than with a plain allocation -- and one band lies on each side of it: at least 64 KiB, at least the buffer's own size, at most
8 MiB (a 32-row tile block of the widest layer row in the tables, 470 x 64 channels x 4 B x 32 rows, is 3.9 MB).  The far band starts at the
buffer's last byte + 1: a store one element past the end is seen, which the allocator's own rounding to 512 bytes hides.  `src` copies
initial contents in; without it the buffer stays 0xFF, so an element no kernel writes reads back as NaN (or -1).

    t.guard.assert_intact()          every band byte is still 0xFF; the failure names the buffer, the side, the first and last touched byte
                                     (offsets from the buffer's first byte: negative in front of it, >= its size behind it) and the count
    t.guard.fill(byte)               the buffer's own bytes (not the bands) := byte

Guards collects the arenas of one test: g.new(...) a buffer a kernel may write, g.ro(tensor) a guarded copy of an operand a kernel only
reads (its bits are kept), g.check() = all bands intact and all read-only operands unchanged.

    assert_unchanged(t, snapshot)    same bits, compared through an integer view: NaN equals NaN, -0 differs from +0.

What the bands cannot see: a stray store of 0xFF bytes.  A kernel that runs past the end of its operands reads the operands' own bands, NaN,
and a result computed from NaN is as a rule the all-ones NaN again: such a store into a band leaves it as it was.  (Tried: a max-pool widened
by a row on both sides, loads and stores, passed; widened on the store side alone it is reported.)  The same read shows wherever its result
lands inside a buffer, where NaN fails the numeric check."""
import torch

ALIGN = 512
BAND_MIN = 64 << 10
BAND_MAX = 8 << 20
FILL = 0xFF
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def band_bytes(nbytes):
    b = min(max(BAND_MIN, int(nbytes)), BAND_MAX)
    return (b + ALIGN - 1) // ALIGN * ALIGN


def _bits(t):
    """t's bytes as integers of its element size (bit patterns: what == on floats would not compare)"""
    t = t.contiguous()
    if t.is_floating_point():
        return t.view(_INT_OF_SIZE[t.element_size()])
    return t


def same_bits(a, b):
    """two results are the same bits (NaN payloads and the sign of zero included)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def all_bytes(t, byte):
    """every byte of t is `byte` (0xFF: nothing was written since the fill)"""
    return bool((t.contiguous().view(torch.uint8) == byte).all())


def assert_unchanged(t, snapshot, name='operand'):
    assert t.shape == snapshot.shape and t.dtype == snapshot.dtype, '%s: %s %s against a snapshot %s %s' % (
        name, tuple(t.shape), t.dtype, tuple(snapshot.shape), snapshot.dtype)
    a, b = _bits(t).reshape(-1), _bits(snapshot).reshape(-1)
    if not torch.equal(a, b):
        diff = (a != b).nonzero().reshape(-1)
        raise AssertionError('%s: a read-only operand changed at %d of %d elements, first at flat index %d, last at %d' % (
            name, diff.numel(), a.numel(), int(diff[0]), int(diff[-1])))


class Guard:
    """one arena: [band | buffer | band], all 0xFF at first"""

    def __init__(self, shape, dtype, device, src=None, name='buffer'):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.name, self.shape, self.dtype = name, shape, dtype
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.band = band_bytes(self.nbytes)
        self.arena = torch.full((2 * self.band + self.nbytes,), FILL, dtype=torch.uint8, device=device)
        if src is not None:
            assert tuple(src.shape) == shape, '%s: src %s for a buffer %s' % (name, tuple(src.shape), shape)
            self.view().copy_(src.to(dtype))

    def view(self):
        """the buffer as a tensor (the guard keeps no reference to it: tensor -> guard -> arena, no cycle)"""
        t = self.arena[self.band:self.band + self.nbytes].view(self.dtype).view(self.shape)
        assert t.is_contiguous() and (t.data_ptr() - self.arena.data_ptr()) % ALIGN == 0
        t.guard = self
        return t

    def fill(self, byte):
        self.arena[self.band:self.band + self.nbytes] = byte

    def bands(self):
        """(side, offset of the band's first byte from the buffer's first byte, the band's bytes)"""
        return (('in front of', -self.band, self.arena[:self.band]),
                ('behind', self.nbytes, self.arena[self.band + self.nbytes:]))

    def touched(self):
        """[(side, first offset, last offset, count)] of the bands that are no longer all 0xFF"""
        out = []
        for side, base, b in self.bands():
            bad = b != FILL
            if bool(bad.any()):
                idx = bad.nonzero().reshape(-1)
                out.append((side, base + int(idx[0]), base + int(idx[-1]), int(idx.numel())))
        return out

    def assert_intact(self):
        hit = self.touched()
        assert not hit, '; '.join('%s %s %s (%d bytes): %d bytes written %s the buffer, byte offsets %d .. %d from its first byte' % (
            self.name, self.shape, self.dtype, self.nbytes, cnt, side, first, last) for side, first, last, cnt in hit)


def guarded(shape, dtype, device, src=None, name='buffer'):
    return Guard(shape, dtype, device, src, name).view()


class Guards:
    """the arenas of one test"""

    def __init__(self, device='cuda'):
        self.device, self.guards, self.readonly = device, [], []

    def new(self, shape, dtype=torch.float32, name=None, src=None):
        t = guarded(shape, dtype, self.device, src, name or 'buffer %d' % len(self.guards))
        self.guards.append(t.guard)
        return t

    def ro(self, src, name=None):
        """a guarded copy of an operand a kernel only reads (None stays None)"""
        if src is None:
            return None
        t = self.new(src.shape, src.dtype, name or 'operand %d' % len(self.guards), src)
        self.readonly.append((t, t.clone()))
        return t

    def assert_intact(self):
        for g in self.guards:
            g.assert_intact()

    def check(self):
        """after a call: nothing outside any buffer was written, no read-only operand changed"""
        self.assert_intact()
        for t, snap in self.readonly:
            assert_unchanged(t, snap, t.guard.name)
