"""CPU tests of tests/guarded.py (buffers between guard bands) and negative controls of every float comparator the conv / U-Net GPU tests use.

The comparators are called directly on CPU tensors: each must reject a result with one NaN, a result that is all NaN and +-inf against a finite
reference, and still accept the exact reference.  (A comparator that looks for elements above the bound passes a NaN: no comparison with NaN is
true.  It has to ask for err <= bound.)"""
import types

import pytest

torch = pytest.importorskip('torch')

import guarded as G                        # noqa: E402
from oracle import bf16_ref as R           # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.int16, torch.uint8, torch.int32]


# ---- guarded buffers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 7), (1,), (2, 9, 21, 32), (70001,)])
def test_views_are_contiguous_aligned_and_poisoned(dtype, shape):
    t = G.guarded(shape, dtype, 'cpu')
    g = t.guard
    assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
    assert (t.data_ptr() - g.arena.data_ptr()) % 512 == 0 and t.data_ptr() - g.arena.data_ptr() == g.band
    assert g.nbytes == t.numel() * t.element_size()
    assert g.band >= 64 << 10 and g.band >= min(g.nbytes, 8 << 20) and g.band <= 8 << 20 and g.band % 512 == 0
    assert g.arena.numel() == 2 * g.band + g.nbytes and bool((g.arena == 0xFF).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())                       # an element no kernel writes reads back as NaN
    elif dtype == torch.uint8:
        assert bool((t == 255).all())
    else:
        assert bool((t == -1).all())
    g.assert_intact()                                            # an untouched arena passes
    t.zero_()                                                    # ... and so does one whose buffer was written from its first byte to its last
    g.assert_intact()
    assert not bool(g.arena[g.band:g.band + g.nbytes].any())
    g.fill(0xFF)
    assert bool((g.arena == 0xFF).all())


def test_band_size_is_capped():
    assert G.band_bytes(1) == 64 << 10 and G.band_bytes(100000) == 100352 and G.band_bytes(1 << 30) == 8 << 20
    t = G.guarded((9 << 20,), torch.uint8, 'cpu')
    assert t.guard.band == 8 << 20


@pytest.mark.parametrize('dtype', DTYPES)
def test_src_is_copied_and_kept(dtype):
    src = (torch.arange(2 * 3 * 5).reshape(2, 3, 5) % 100).to(dtype)
    t = G.guarded(src.shape, dtype, 'cpu', src=src)
    assert torch.equal(t, src)
    t.guard.assert_intact()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('where', ['first byte behind', 'last byte in front', 'far end behind', 'far end in front'])
def test_one_byte_writes_are_reported(dtype, where):
    t = G.guarded((5, 33), dtype, 'cpu', name='out')
    g = t.guard
    pos = {'first byte behind': g.band + g.nbytes, 'last byte in front': g.band - 1, 'far end behind': g.arena.numel() - 1, 'far end in front': 0}[where]
    g.arena[pos] = 0xFE                                          # one bit of one byte
    off = pos - g.band
    assert g.touched() == [('behind' if off >= 0 else 'in front of', off, off, 1)]
    with pytest.raises(AssertionError) as e:
        g.assert_intact()
    msg = str(e.value)
    assert 'out' in msg and ('behind' if off >= 0 else 'in front of') in msg and 'byte offsets %d .. %d' % (off, off) in msg and '1 bytes written' in msg
    g.arena[pos] = 0xFF
    g.assert_intact()


def test_report_gives_first_last_and_count_on_both_sides():
    t = G.guarded((100,), torch.float32, 'cpu', name='dw')
    g = t.guard
    g.arena[g.band + 400:g.band + 404] = 0                       # one float past the end
    g.arena[g.band + 400 + 1000] = 7
    g.arena[g.band - 8:g.band] = 0
    assert g.touched() == [('in front of', -8, -1, 8), ('behind', 400, 1400, 5)]
    with pytest.raises(AssertionError):
        g.assert_intact()


def test_registry_checks_every_arena_and_the_read_only_operands():
    gs = G.Guards('cpu')
    out = gs.new((4, 8), torch.float32, 'out')
    x = gs.ro(torch.tensor([0.0, -0.0, float('nan'), 1.5]), 'x')
    assert gs.ro(None) is None
    out.fill_(1.0)
    gs.check()                                                   # NaN in a read-only operand equals itself
    x[1] = 0.0                                                   # -0 -> +0: equal as floats, other bits
    with pytest.raises(AssertionError) as e:
        gs.check()
    assert 'x' in str(e.value) and 'first at flat index 1' in str(e.value)
    x[1] = -0.0
    gs.check()
    out.guard.arena[out.guard.band + out.guard.nbytes] = 0
    with pytest.raises(AssertionError) as e:
        gs.check()
    assert 'out' in str(e.value)


def test_assert_unchanged_compares_bit_patterns():
    for dtype in DTYPES:
        a = (torch.arange(40) % 7).to(dtype)
        G.assert_unchanged(a, a.clone())
        b = a.clone()
        b[17] = 9
        with pytest.raises(AssertionError):
            G.assert_unchanged(b, a)
    nan = torch.full((8,), float('nan'))
    G.assert_unchanged(nan, nan.clone())
    other = nan.clone()
    other.view(torch.int32)[3] = 0x7FC00001                      # another NaN payload
    with pytest.raises(AssertionError):
        G.assert_unchanged(other, nan)
    with pytest.raises(AssertionError):
        G.assert_unchanged(torch.zeros(4), -torch.zeros(4))
    with pytest.raises(AssertionError):
        G.assert_unchanged(torch.zeros(4), torch.zeros(4, dtype=torch.int32))


# ---- the comparators ------------------------------------------------------------------------------------------------------------------------
def _f32_comparators():
    """name -> f(got, y, bound) that raises AssertionError where the comparator rejects"""
    import backward_cases as BC
    import test_backward_layers_gpu as TB
    import test_bf16_layers_gpu as B16
    import test_f32_layers_gpu as F32
    import test_unet_gpu as TU
    stage = types.SimpleNamespace(kind='control', name='control')

    def f32_rejects(got, y, bound):
        assert not BC.f32_rejects(got, y, bound)

    def close(got, y, bound):                                    # bound = tol * (1 + scale)
        TU.close(got, y, tol=1.0, scale=bound - 1.0)
    return {'test_f32_layers_gpu.check': lambda got, y, bound: F32.check(got, y, bound, 'control'),
            'test_unet_gpu.close': close,
            'test_backward_layers_gpu.check_f32': lambda got, y, bound: TB.check_f32('control', stage, got, y, bound),
            'test_bf16_layers_gpu.f32_check': lambda got, y, bound: B16.f32_check(got, y, bound, 'control'),
            'backward_cases.f32_rejects': f32_rejects}, (F32, TB, B16)


NAMES = ['test_f32_layers_gpu.check', 'test_unet_gpu.close', 'test_backward_layers_gpu.check_f32', 'test_bf16_layers_gpu.f32_check',
         'backward_cases.f32_rejects']


@pytest.mark.parametrize('name', NAMES)
def test_float_comparators_reject_nan_and_inf(name):
    fns, mods = _f32_comparators()
    assert sorted(fns) == sorted(NAMES)
    f = fns[name]
    saved = [dict(m.STATS) for m in mods]
    try:
        g = torch.Generator().manual_seed(1)
        y = torch.randn(3, 5, 7, generator=g, dtype=torch.float64)
        bound = torch.full_like(y, 1.0)
        f(y.float(),y.float().double(), bound)                  # the exact reference is accepted
        f(torch.zeros(3, 5, 7), torch.zeros(3, 5, 7, dtype=torch.float64), bound)
        f(y.float() + 0.5, y.float().double(), bound)            # ... and so is an error inside the bound
        bad = {}
        one = y.float().clone()
        one[1, 2, 3] = float('nan')
        bad['one NaN'] = (one, y)
        bad['all NaN'] = (torch.full((3, 5, 7), float('nan')), y)
        bad['all NaN, y = 0, bound = 1'] = (torch.full((3, 5, 7), float('nan')), torch.zeros_like(y))
        for v in (float('inf'), float('-inf')):
            t = y.float().clone()
            t[2, 4, 6] = v
            bad['one %s' % v] = (t, y)
            bad['all %s' % v] = (torch.full((3, 5, 7), v), y)
        far = y.float().clone()
        far[0, 0, 0] += 1.5
        bad['outside the bound'] = (far, y)
        for what, (got, ref) in bad.items():
            with pytest.raises(AssertionError):
                f(got, ref, bound)
                print('accepted:', what)
    finally:
        for m, s in zip(mods, saved):
            m.STATS.clear()
            m.STATS.update(s)


def test_f32_layer_check_records_a_nan_ratio_as_inf():
    """the summary a module prints at its end keeps max(STATS, r): with r = NaN the maximum stayed at its old value"""
    import test_f32_layers_gpu as F32
    saved = dict(F32.STATS)
    try:
        F32.STATS.clear()
        with pytest.raises(AssertionError):
            F32.check(torch.full((4,), float('nan')), torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), 'control')
        assert F32.STATS['control'] == float('inf')
    finally:
        F32.STATS.clear()
        F32.STATS.update(saved)


@pytest.mark.parametrize('pattern', [0xFFFF, 0x7FC0, 0x7F80, 0xFF80])
def test_bf16_accept_rejects_nan_and_inf_bit_patterns(pattern):
    g = torch.Generator().manual_seed(2)
    y = torch.randn(4, 6, 8, generator=g, dtype=torch.float64)
    y.view(-1)[::5] = 0.0
    m = torch.full_like(y, 1e-3)
    good = R.bits_of(R.rne_bf16(y))
    ok, flipped = R.bf16_accept(good, y, m)
    assert bool(ok.all()) and not bool(flipped.any())            # the exact reference is accepted
    one = good.clone()
    one[3, 5, 7] = pattern
    ok, _ = R.bf16_accept(one, y, m)
    assert not bool(ok[3, 5, 7]) and int((~ok).sum()) == 1
    ok, _ = R.bf16_accept(torch.full_like(good, pattern), y, m)
    assert not bool(ok.any())
    ok, _ = R.bf16_accept(torch.full_like(good, pattern), torch.zeros_like(y), torch.ones_like(y))      # y = 0, margin 1
    assert not bool(ok.any())
    # as the layer tests read an int16 output that no kernel wrote: every byte 0xFF
    import test_bf16_layers_gpu as B16
    raw = torch.full((4, 6, 8), -1, dtype=torch.int16)
    assert B16.rejects(B16.bits(raw), y, m)
    saved = dict(B16.STATS)
    try:
        with pytest.raises(AssertionError):
            B16.accept(raw, y, m, 'control')
    finally:
        B16.STATS.update(saved)
