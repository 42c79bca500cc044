"""CPU tests of the dark-frame noise term (flag DARK, model letter 'D'): the entry's argument errors (they precede device work), the flag
parse, the parameter record, the ValueErrors of NoiseModel / DarkPool / validate, and that the shapes of the GPU test draw crops on
every path (odd and even offsets, more than one frame, the 16-byte and the 4-byte loads)."""
import contextlib
import ctypes
import io

import numpy as np
import pytest

import darknoise_ref as R

RGGB = [[0, 1], [3, 2]]
FAKE = 0x10000          # a 16-byte aligned non-null "device pointer": every call below must return before anything dereferences it


def _call(lib, flags, C=4, H=8, W=12, pool=FAKE, pool_elems=4096, frames=FAKE, F=3, min_h=10, min_w=14, pattern=(0, 1, 3, 2), black=(512.0,) * 4,
          N=2):
    pat = None if pattern is None else (ctypes.c_int * 4)(*pattern)
    blk = None if black is None else (ctypes.c_float * 4)(*black)
    chw = C * H * W
    return lib.eld_noise_forward_dark(FAKE, 0, chw, FAKE, chw, FAKE, N, C, H, W, flags, 2018, None, None, pool, pool_elems, frames, F, min_h, min_w,
                                      pat, blk, None)


def test_entry_argument_errors(eld_lib):
    from eld_amd import _lib as L
    D, P, U, X = L.DARK, L.SHOT_POISSON, L.QUANT, L.CFA_XTRANS
    EINVAL = -1
    for extra in (L.READ_GAUSS, L.READ_TL, L.ROW, L.CBIAS):                        # those terms would be counted twice
        assert _call(eld_lib, P | D | U | extra) == EINVAL
    for kw in (dict(pool=None), dict(pool=FAKE + 8), dict(frames=None), dict(frames=FAKE + 4), dict(F=0), dict(F=-1), dict(pool_elems=0),
               dict(H=11), dict(W=15), dict(min_h=0), dict(pattern=(0, 1, 1, 2)), dict(pattern=(0, 1, 2, 4)), dict(pattern=None), dict(black=None),
               dict(black=(512.0, -1.0, 512.0, 512.0)), dict(C=3), dict(C=9)):
        assert _call(eld_lib, P | D | U, **kw) == EINVAL, kw
    assert _call(eld_lib, P | D | U | X, C=4) == EINVAL                            # X-Trans has 9 planes
    assert _call(eld_lib, P | D | U | X, C=9, pattern=None, black=None) == EINVAL
    assert _call(eld_lib, P | D | U | X, C=9, pattern=None, H=11) == EINVAL
    # the entries without a pool refuse the flag
    assert eld_lib.eld_noise_forward(FAKE, 0, FAKE, FAKE, 2, 4, 8, 12, P | D | U, 2018, None, None, None) == EINVAL
    assert eld_lib.eld_noise_forward_strided(FAKE, 0, 384, FAKE, 384, FAKE, 2, 4, 8, 12, D, 2018, None, None, None) == EINVAL
    assert _call(eld_lib, P | D | U, N=0) == 0 and _call(eld_lib, P | D | U, N=-1) == EINVAL


def test_flags_and_record():
    from eld_amd import _lib as L
    from eld_amd.noise import NoiseParams, make_records, model_flags
    assert L.DARK == 1024 and 'eld_noise_forward_dark' in L.SIGNATURES
    assert model_flags('PDU') == 1 | 32 | 1024
    assert model_flags('PDU', 'xtrans') == 1 | 32 | 1024 | 512 and model_flags('PGRU') == 1 | 8 | 16 | 32
    p = NoiseParams(2.0, 1.0, 15583, 100.0, dark=(3, 4))
    assert p.dark == (3, 4) and p.record(7)['reserved'].tolist() == [3, 4]
    assert NoiseParams(2.0, 1.0, 15583, 100.0).record(7)['reserved'].tolist() == [0, 0]
    assert NoiseParams.coerce({'K': 1.0, 'g_scale': 0.0, 'ratio': 1.0, 'dark': (1, 2)}).dark == (1, 2)
    recs = make_records([p, (1.0, 1.0, 15583, 100.0)], [0, 1])
    assert recs['reserved'].tolist() == [[3, 4], [0, 0]] and recs.dtype.itemsize == 64


def _sessions(n=(3, 2), shape=(12, 16)):
    return [{'iso': 100 * (i + 1), 'bias': np.full((k,) + shape, 512 + i, np.uint16)} for i, k in enumerate(n)]


@pytest.fixture
def no_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)      # any device work would fail loudly; none may be reached


def test_darkpool_geometry_and_errors(eld_lib, no_gpu):
    from eld_amd.darkpool import DarkPool
    s = _sessions()
    s[1]['bias'] = [np.zeros((10, 14), np.uint16), np.zeros((12, 16), np.uint16)]      # sizes may differ; a list of frames
    pool = DarkPool(s, raw_pattern=RGGB, black_level=[512, 520, 500, 531], white_level=16383, K=[1.5, 3.0])
    assert len(pool) == 5 and pool.sessions == 2 and pool.ranges == [(0, 3), (3, 2)] and pool.isos == [100, 200]
    assert pool.saturation == 16383 - 531 and pool.min_extent == (5, 7) and pool.C == 4
    assert all(int(o) % 8 == 0 for o in pool.pool.frames['offset'])
    pool.check_patch(5, 7)
    with pytest.raises(ValueError, match='smallest dark frame'):
        pool.check_patch(6, 7)
    with pytest.raises(RuntimeError):
        pool.launch_args()                                              # no frames on a device here
    for bad in ([], [{}], [{'bias': []}], [{'bias': np.zeros((2, 12, 16), np.int32)}], [{'bias': np.zeros((2, 11, 16), np.uint16)}], 'x'):
        with pytest.raises(ValueError):
            DarkPool(bad, black_level=512)
    for kw in (dict(cfa='foveon'), dict(raw_pattern=[[0, 1], [1, 2]]), dict(black_level=[512, 512]), dict(white_level=400, black_level=512),
               dict(K=[1.0]), dict(K=[1.0, 0.0]), dict(K=[1.0, float('nan')])):
        with pytest.raises(ValueError):
            DarkPool(_sessions(), **kw)
    xp = DarkPool(_sessions(shape=(18, 24)), cfa='xtrans', black_level=[1024] * 4, white_level=16383)
    assert xp.C == 9 and xp.min_extent == (6, 8) and xp.saturation == 16383 - 1024 and xp.K is None


def _noise_model(**kw):
    from eld_amd.noise import NoiseModel
    with contextlib.redirect_stdout(io.StringIO()):
        return NoiseModel(include=4, **kw)


def test_noise_model_errors_and_draws(eld_lib, no_gpu):
    from eld_amd.darkpool import DarkPool
    from eld_amd.noise import noise_model_flags
    pool = DarkPool(_sessions(), raw_pattern=RGGB, black_level=512, white_level=16383, K=[1.5, 3.0])
    with pytest.raises(ValueError, match='DarkPool'):
        _noise_model(model='PDU')
    for m in ('PDg', 'PGDU', 'PDRU', 'PDUB'):
        with pytest.raises(ValueError, match='excludes'):
            _noise_model(model=m, dark=pool)
    with pytest.raises(ValueError, match='holds bayer frames'):
        _noise_model(model='PDU', dark=pool, cfa='xtrans')
    nm = _noise_model(model='PDU', dark=pool)
    assert noise_model_flags(nm) == 1 | 32 | 1024
    ref = _noise_model(model='Pg')
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        p = nm._sample_params()
        after = np.random.randint(1 << 30)
        np.random.seed(seed)
        K, g, sat, ratio = ref._sample_params()                          # the reference's five draws come first, unchanged ...
        si = int(np.random.randint(pool.sessions))                       # ... then one session index
        assert np.random.randint(1 << 30) == after                       # and nothing else
        assert p.dark == pool.ranges[si] and p[0] == pool.K[si] and p[1] == g and p[2] == pool.saturation and p[3] == ratio and p.q_step == 1.0
        seen.add(si)
    assert seen == {0, 1}
    with pytest.raises(ValueError, match='gains'):
        _noise_model(model='PDU', dark=DarkPool(_sessions(), black_level=512))._sample_params()


def test_validate_and_train_frames_argument_errors(eld_lib, no_gpu):
    from eld_amd import train_frames as T
    from eld_amd import validate as V
    assert V._models('P,Pg,PD,PDU') == ['P', 'Pg', 'PD', 'PDU']
    for m in ('PDg', 'PGD', 'PDR', 'PDB'):
        with pytest.raises(ValueError, match='excludes'):
            V._models([m])
    s = [{'iso': 100, 'bias': np.full((1, 8, 8), 512, np.uint16), 'flats': np.full((1, 2, 8, 8), 900, np.uint16)},
         {'iso': 200, 'bias': np.full((2, 8, 8), 512, np.uint16), 'flats': np.full((1, 2, 8, 8), 900, np.uint16)}]
    with pytest.raises(ValueError, match='single bias frame'):
        V.validate_camera(s, RGGB, [512.0] * 4, 16383, diag={'frames': [], 'K': [1.0, 2.0]}, models=('P', 'PD'))
    with pytest.raises(ValueError, match='--dark'):
        T.dark_pool(None, 'SonyA7S2', 'PDU', 512)
    with pytest.raises(ValueError, match='letter D'):
        T.dark_pool('manifest.json', 'SonyA7S2', 'PGRU', 512)
    assert T.dark_pool(None, 'SonyA7S2', 'PGRU', 512) is None
    assert T.build_parser().parse_args(['a.npy', '-o', 'x.pt', '--noise', 'PDU', '--dark', 'm.json']).dark == 'm.json'


def test_choices_cover_every_path():
    """The crops the GPU test's sample ids 0..63 draw: both parities of x0, more than one frame, the 16-byte and the 4-byte loads, and even
    offsets only for X-Trans -- so that test cannot pass on aligned offsets alone."""
    ext = R.extents_of(R.BAYER_SHAPES, 'bayer')
    for C, H, W in R.BAYER_PATCHES[:2]:
        ch = [R.dark_choice(R.SEED, i, 0, 3, ext, H, W, 'bayer') for i in range(64)]
        assert {f for f, _, _ in ch} == {0, 1, 2}
        assert {x0 & 1 for _, _, x0 in ch} == {0, 1} and {y0 & 1 for _, y0, _ in ch} == {0, 1}
        for f, y0, x0 in ch:
            assert 0 <= y0 <= ext[f][0] - H and 0 <= x0 <= ext[f][1] - W
        w = {R.wide(R.BAYER_OFFSETS[f], R.BAYER_SHAPES[f][1], x0) for f, _, x0 in ch}
        assert w == {False, True}
    assert R.BAYER_OFFSETS[1] % 8 != 0 and R.BAYER_OFFSETS[1] % 2 == 0
    C, H, W = R.BAYER_PATCHES[2]                                        # the whole packed extent of the smallest frame: the origin is forced
    assert ext[0] == (H, W) and all(R.dark_choice(R.SEED, i, 0, 1, ext, H, W, 'bayer') == (0, 0, 0) for i in range(8))
    ext = R.extents_of(R.XTRANS_SHAPES, 'xtrans')
    assert ext == [(6, 8), (8, 12), (6, 8)]
    for C, H, W in R.XTRANS_PATCHES:
        ch = [R.dark_choice(R.SEED, i, 0, 3, ext, H, W, 'xtrans') for i in range(64)]
        assert {f for f, _, _ in ch} == {0, 1, 2} and all(y0 % 2 == 0 and x0 % 2 == 0 for _, y0, x0 in ch)
        assert len({(y0, x0) for _, y0, x0 in ch}) > 1
    # a sub-range draws from that range only
    assert {R.dark_choice(R.SEED, i, 1, 2, R.extents_of(R.BAYER_SHAPES, 'bayer'), 5, 7, 'bayer')[0] for i in range(64)} == {1, 2}


def test_restatement_gathers_the_packed_codes():
    """dark_codes is the crop of the packed mosaic: Bayer against the oracle's RGGB pack and a permuted pattern by hand, X-Trans against the
    oracle's pack of the truncated frame."""
    from oracle import noise_ref as O
    m = R.mosaics_of(R.BAYER_SHAPES)[1]
    full = O.pack_raw_bayer(m).astype(np.int64)
    assert np.array_equal(R.dark_codes(m, 'bayer', [0, 1, 3, 2], 3, 5, 8, 12), full[:, 3:11, 5:17])
    got = R.dark_codes(m, 'bayer', [2, 3, 1, 0], 1, 2, 4, 4)
    assert got[2, 0, 0] == m[2, 4] and got[3, 0, 0] == m[2, 5] and got[1, 0, 0] == m[3, 4] and got[0, 0, 0] == m[3, 5]
    x = R.mosaics_of(R.XTRANS_SHAPES)[2]
    assert np.array_equal(R.dark_codes(x, 'xtrans', None, 2, 0, 4, 6), O.pack_raw_xtrans(x)[:, 2:6, 0:6].astype(np.int64))
    assert len(np.unique(np.concatenate([v.reshape(-1) for v in R.mosaics_of(R.BAYER_SHAPES)]))) == sum(a * b for a, b in R.BAYER_SHAPES)
