"""CPU tests of the frame pool (eld_amd/framepool.py): the NumPy restatement reproduces the reference-minted fixture bit for bit in the
reference's dtypes (and the fixture tells float32 from float64), grid() is the reference's enumeration, bad arguments raise before any
device work, and the loader draws from np.random in its documented order."""
import contextlib
import io
import os

import numpy as np
import pytest

import framepool_ref as R

CASES = (('bayer_a', 'bayer'), ('bayer_b', 'bayer'), ('xtrans', 'xtrans'))


@pytest.fixture(scope='module')
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, 'framepool.npz')))


def case_args(gold, name, cfa):
    return dict(raw_pattern=gold[name + '_pattern'] if cfa == 'bayer' else None, black=gold[name + '_black'].tolist(), white=int(gold['white']))


def ref_codes(gold, name, cfa, ratio, dtype=None):
    k = int(gold['ksize'])
    recs = [(0, y, x, ratio) for y, x in gold[name + '_offsets']]
    return R.patches([gold[name + '_mosaic']], cfa, recs, k, k, dtype=dtype, **case_args(gold, name, cfa))


@pytest.mark.parametrize('name,cfa', CASES)
def test_restatement_reproduces_the_reference_codes(gold, name, cfa):
    for r in gold['ratios']:
        want = gold['%s_codes_r%d' % (name, r)]
        # the fixture's ratio-1 codes were minted WITHOUT the ratio multiply (ratios=None in create_lmdb_train)
        assert np.array_equal(ref_codes(gold, name, cfa, None if r == 1 else float(r)), want), (name, int(r))
    # ... and multiplying by 1 is the identity in IEEE arithmetic: ratio 1 gives the codes of the chain without the multiply
    assert np.array_equal(ref_codes(gold, name, cfa, 1.0), gold[name + '_codes_r1'])


def test_fixture_content_is_what_the_checks_need(gold):
    for name, cfa in CASES:
        u, b = gold[name + '_mosaic'], gold[name + '_black']
        assert u.dtype == np.uint16 and (u < b.min()).any() and (u == int(gold['white'])).any()
        c1, c300 = gold[name + '_codes_r1'], gold[name + '_codes_r300']
        assert ((c1 < 65535) & (c300 == 65535)).any() and (c300 < 65535).any()      # values that saturate only under the ratio, and some that never do
        assert (gold[name + '_offsets'] > 0).all()                                   # the centre crop is not trivial
    assert gold['xtrans_mosaic'].shape[0] % 6 and gold['xtrans_mosaic'].shape[1] % 6
    assert (gold['xtrans_offsets'] % 2 == 1).any()                                   # the reference's grid starts on an odd packed row / column
    assert not np.array_equal(gold['bayer_a_pattern'], gold['bayer_b_pattern']) and len(set(gold['bayer_a_black'].tolist())) == 4


@pytest.mark.parametrize('name,cfa', CASES)
def test_fixture_pins_the_dtypes(gold, name, cfa):
    """Negative control: the wrong dtype (X-Trans in float32, Bayer in float64) changes codes of the fixture."""
    wrong = np.float64 if cfa == 'bayer' else np.float32
    changed = 0
    for r in gold['ratios']:
        got = ref_codes(gold, name, cfa, None if r == 1 else float(r), dtype=wrong)
        changed += int(np.count_nonzero(got != gold['%s_codes_r%d' % (name, r)]))
    assert changed > 0


def pool_of(gold, names, cfa, **kw):
    from eld_amd.framepool import FramePool
    n0 = names[0]
    a = case_args(gold, n0, cfa)
    return FramePool([gold[n + '_mosaic'] for n in names], cfa=cfa, raw_pattern=a['raw_pattern'], black_level=a['black'], white_point=a['white'], **kw)


def test_grid_is_the_reference_enumeration(gold, eld_lib):
    k = int(gold['ksize'])
    for name, cfa in CASES:
        pool = pool_of(gold, [name], cfa)
        g = pool.grid((pool.C, k, k), (pool.C, k, k))
        assert (g.ph, g.pw) == (k, k) and np.all(g.records['ratio'] == 1) and np.all(g.records['frame'] == 0)
        assert np.array_equal(np.stack([g.records['y0'], g.records['x0']], axis=1), gold[name + '_offsets'])
    # several frames, a stride that differs from the patch: frame-major, then the restatement's order
    pool = pool_of(gold, ['bayer_a', 'bayer_b'], 'bayer')
    g = pool.grid((4, 16, 12), (4, 8, 10))
    want = R.grid([R.packed_extent(*gold[n + '_mosaic'].shape, 'bayer') for n in ('bayer_a', 'bayer_b')], 16, 12, 8, 10)
    assert np.array_equal(np.stack([g.records['frame'], g.records['y0'], g.records['x0']], axis=1), want) and len(want) > 6
    assert pool.check(g) is not g and len(pool.check(g, ratios=100.0)) == len(g)
    for bad in (((3, 16, 16), (4, 16, 16)), ((4, 16, 16), (4, 0, 16)), ((4, 64, 16), (4, 16, 16)), ((4, 16), (4, 16))):
        with pytest.raises(ValueError):
            pool.grid(*bad)


def test_bad_arguments_raise_before_device_work(gold, eld_lib, monkeypatch):
    from eld_amd import framepool as FP
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # any device work would fail loudly; none may be reached
    u = gold['bayer_a_mosaic']
    for kw in (dict(cfa='foveon'), dict(raw_pattern=[[0, 1], [1, 2]]), dict(black_level=[512, 512, 512]), dict(white_point=400, black_level=512),
               dict(white_point=70000), dict(black_level=-1)):
        with pytest.raises(ValueError):
            FP.FramePool([u], **kw)
    for m in ([], [u.astype(np.int32)], [u[:-1]], [u.reshape(-1)], [np.zeros((4, 4), np.uint16)]):
        with pytest.raises(ValueError):
            FP.FramePool(m, cfa='xtrans' if len(m) and m[0].shape == (4, 4) else 'bayer')
    pool = FP.FramePool([u, gold['bayer_b_mosaic']], black_level=512)
    assert pool.buffer is None and len(pool) == 2 and pool.extent.tolist() == [[35, 37], [19, 37]]
    assert pool.frames['offset'].tolist() == [0, 5184] and pool.elems % 8 == 0            # 70 * 74 = 5180 codes, padded to a 16-byte boundary
    good = [[0, 19, 21], [1, 3, 0]]
    assert len(pool.check(good, patch=16)) == 2
    for recs, kw in (([[2, 0, 0]], {}), ([[-1, 0, 0]], {}), ([[0, 20, 0]], {}), ([[0, 0, 22]], {}), ([[1, 4, 0]], {}), ([[0, -1, 0]], {}),
                     (good, dict(ratios=[1.0, 2.0, 3.0])), (good, dict(ratios=0.0)), (good, dict(ratios=float('nan'))), ([[0.5, 0, 0]], {}),
                     ([[0, 0]], {}), (np.zeros((0, 3), np.int64), {})):
        with pytest.raises(ValueError):
            pool.patches(recs, patch=kw.pop('patch', 16), **kw)
    with pytest.raises(ValueError):
        pool.patches(good)                                                  # rows without a patch size
    with pytest.raises(ValueError):
        pool.patches(good, patch=(16, 0))
    with pytest.raises(RuntimeError):
        pool.patches(good, patch=16)                                        # valid records, but this pool holds no frames on a device
    nm = types_noise_model()
    for kw in (dict(batch_size=0), dict(patch=64), dict(patch=(16, 12)), dict(num_burst=0), dict(steps_per_epoch=0), dict(ratios=[100, 100]),
               dict(inputs=FP.FramePool([u], black_level=512), ratios=[100, 100]), dict(inputs=pool, ratios=[100]), dict(inputs=pool)):
        with pytest.raises(ValueError):
            FP.FramePoolLoader(pool, nm, **dict(dict(batch_size=2, patch=16), **kw))
    with pytest.raises(ValueError):
        FP.FramePoolLoader(pool, None, 2, patch=16)
    with pytest.raises(ValueError):
        FP.FramePoolLoader(FP.FramePool([gold['xtrans_mosaic']], cfa='xtrans'), nm, 2, patch=5, augment=False)      # X-Trans: even sides


def test_library_missing(gold, tmp_path, monkeypatch):
    import eld_amd
    from eld_amd import _lib as L
    from eld_amd import framepool as FP
    monkeypatch.setattr(L, '_lib', None)
    monkeypatch.setattr(L, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(eld_amd.LibraryMissing):
        FP.FramePool([gold['bayer_a_mosaic']])


def types_noise_model(model='PGRU'):
    from eld_amd.noise import NoiseModel
    with contextlib.redirect_stdout(io.StringIO()):
        return NoiseModel(model=model, include=4)


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_loader_draw_order(gold, eld_lib, monkeypatch, cfa):
    """frame, y0, x0, _sample_params(), three augmentation bits -- per sample, replayed here by hand from the same seed."""
    from eld_amd import framepool as FP
    from eld_amd.noise import NoiseParams
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    if cfa == 'bayer':
        pool = FP.FramePool([gold['bayer_a_mosaic'], gold['bayer_b_mosaic']], black_level=512)
    else:
        pool = FP.FramePool([gold['xtrans_mosaic'], gold['xtrans_mosaic'][:44, :80]], cfa='xtrans')
    nm = types_noise_model()
    P, B = 12, 5
    loader = FP.FramePoolLoader(pool, nm, B, patch=P, steps_per_epoch=3, num_burst=2)
    assert len(loader) == 3
    np.random.seed(1234)
    drawn = [loader.draw() for _ in range(2)]
    np.random.seed(1234)
    step = 2 if cfa == 'xtrans' else 1
    for crops, params, bits in drawn:
        assert (crops.ph, crops.pw, len(crops)) == (P, P, B)
        for i in range(B):
            f = np.random.randint(len(pool))
            hp, wp = pool.extent[f]
            y0 = step * np.random.randint((hp - P) // step + 1)
            x0 = step * np.random.randint((wp - P) // step + 1)
            want = NoiseParams.coerce(nm._sample_params())
            b = sum(bit for bit in (1, 2, 4) if np.random.randint(2, size=1)[0] == 1)
            r = crops.records[i]
            assert (int(r['frame']), int(r['y0']), int(r['x0']), float(r['ratio'])) == (f, y0, x0, 1.0)
            assert r['y0'] % step == 0 and r['x0'] % step == 0
            assert tuple(params[i]) == tuple(want) and params[i].record(0).tobytes() == want.record(0).tobytes()
            assert bits[i] == b
        pool.check(crops)                                    # every drawn record lies inside its frame
    # the same seed draws the same batches; without augmentation no bit is drawn (and non-square patches are allowed)
    np.random.seed(1234)
    again = loader.draw()
    assert again[0].records.tobytes() == drawn[0][0].records.tobytes() and again[2] == drawn[0][2]
    plain = FP.FramePoolLoader(pool, nm, 3, patch=(12, 8), augment=False)
    np.random.seed(7)
    c, p, b = plain.draw()
    np.random.seed(7)
    for i in range(3):
        f = np.random.randint(len(pool))
        y0 = step * np.random.randint((pool.extent[f, 0] - 12) // step + 1)
        x0 = step * np.random.randint((pool.extent[f, 1] - 8) // step + 1)
        nm._sample_params()
        assert (int(c.records[i]['frame']), int(c.records[i]['y0']), int(c.records[i]['x0'])) == (f, y0, x0)
    assert b == [0, 0, 0] and len(plain) >= 1
    # paired mode: no parameter draw between the position and the bits
    paired = FP.FramePoolLoader(pool, None, 2, patch=P, inputs=pool, ratios=[100.0, 300.0])
    np.random.seed(9)
    c, p, b = paired.draw()
    np.random.seed(9)
    for i in range(2):
        f = np.random.randint(len(pool))
        y0 = step * np.random.randint((pool.extent[f, 0] - P) // step + 1)
        x0 = step * np.random.randint((pool.extent[f, 1] - P) // step + 1)
        bb = sum(bit for bit in (1, 2, 4) if np.random.randint(2, size=1)[0] == 1)
        assert (int(c.records[i]['frame']), int(c.records[i]['y0']), int(c.records[i]['x0']), b[i]) == (f, y0, x0, bb)
    assert p is None


def test_wide_load_predicate(gold, eld_lib, monkeypatch):
    """Which records take the 16-byte load path (csrc/framepool.hip): patch width, row pitch and the first code's alignment."""
    from eld_amd import framepool as FP
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    pool = FP.FramePool([np.zeros((64, 64), np.uint16), np.zeros((64, 68), np.uint16)], black_level=512)
    c = FP.Crops.make([0, 0, 0, 1], [0, 3, 1, 0], [0, 4, 2, 0], 16, 16)
    assert pool.wide_loads(c).tolist() == [True, True, False, False]          # x0 % 4; a row pitch of 68 codes is not a multiple of 8
    assert not pool.wide_loads(FP.Crops.make([0], [0], [0], 16, 12)).any()
    xp = FP.FramePool([np.zeros((96, 96), np.uint16)], cfa='xtrans')
    assert xp.wide_loads(FP.Crops.make([0, 0, 0], [0, 0, 1], [0, 2, 8], 16, 16)).tolist() == [True, False, True]


def test_entry_points_refuse_what_the_host_can_see(eld_lib):
    """ELD_EINVAL before any launch (so this runs without a GPU; the fake pointers are never dereferenced)."""
    import ctypes
    P, pat, blk = 0x10000, (ctypes.c_int * 4)(0, 1, 3, 2), (ctypes.c_float * 4)(512, 512, 512, 512)
    good = dict(pool=P, elems=4096, frames=P, F=1, max_h=32, max_w=32, recs=P, B=2, ph=16, pw=16, out=P)

    def bayer(pattern=pat, black=blk, white=16383.0, **kw):
        a = dict(good, **kw)
        return eld_lib.eld_crop_pack_raw_bayer_u16(a['pool'], a['elems'], a['frames'], a['F'], a['max_h'], a['max_w'], a['recs'], a['B'], a['ph'], a['pw'],
                                                   pattern, black, white, a['out'], None)

    def xtrans(black=1024.0, white=16383.0, **kw):
        a = dict(good, **kw)
        return eld_lib.eld_crop_pack_raw_xtrans_u16(a['pool'], a['elems'], a['frames'], a['F'], a['max_h'], a['max_w'], a['recs'], a['B'], a['ph'], a['pw'],
                                                    black, white, a['out'], None)
    for kw in (dict(B=0), dict(F=0), dict(ph=0), dict(pw=-1), dict(elems=0), dict(ph=33), dict(pw=40), dict(B=65536), dict(pool=P + 2), dict(pool=P + 8),
               dict(out=P + 4), dict(pool=None), dict(frames=None), dict(recs=None), dict(out=None)):
        assert bayer(**kw) == -1 and xtrans(**kw) == -1, kw
    assert bayer(pattern=(ctypes.c_int * 4)(0, 1, 1, 2)) == -1 and bayer(pattern=(ctypes.c_int * 4)(0, 1, 4, 2)) == -1 and bayer(pattern=None) == -1
    assert bayer(black=(ctypes.c_float * 4)(512, 512, 16383, 512)) == -1 and bayer(white=512.0) == -1 and bayer(white=70000.0) == -1 and bayer(black=None) == -1
    assert xtrans(white=1024.0) == -1 and xtrans(black=-1.0) == -1 and xtrans(white=65536.0) == -1
