"""GPU tests of the dark-frame noise term (eld_noise_forward_dark, flag DARK): the gather against the NumPy restatement bit for bit on every
load path, the full op chain by dumped-variate replay, invariance to batching and bursts, and the skip rule.  Pool codes are a running
index (all distinct), so any index error changes bits.  The crops the ids below draw are pinned by tests/test_darknoise_cpu.py."""
import contextlib
import io

import numpy as np
import pytest

import darknoise_ref as R

pytestmark = pytest.mark.gpu

IDS = list(range(16))
K, SAT, RATIO = 2.25, 15583.0, 137.0


@pytest.fixture(scope='module')
def dev(eld_lib):
    import torch
    assert torch.cuda.is_available()
    return torch.device('cuda', 0)


def _setup(cfa, dev, pattern=None):
    shapes, offs = (R.BAYER_SHAPES, R.BAYER_OFFSETS) if cfa == 'bayer' else (R.XTRANS_SHAPES, R.XTRANS_OFFSETS)
    mos = R.mosaics_of(shapes)
    black = R.BLACK if cfa == 'bayer' else (1024.0, 0.0, 0.0, 0.0)
    return R.HandPool(mos, offs, cfa, pattern, black, dev), R.extents_of(shapes, cfa), black


def _records(ids, rng, K=K, ratio=RATIO):
    from eld_amd.noise import NoiseParams, make_records
    return make_records([NoiseParams(K, 0.0, SAT, ratio, q_step=1.0, dark=rng)] * len(ids), ids)


def _oracle_params(ratio=RATIO):
    from oracle import noise_ref as O
    return O.Params(K=K, g_scale=0.0, saturation=SAT, ratio=ratio, q_step=1.0)


def _run(y, recs, flags, pool, dump=False, misalign=False):
    """-> (out ndarray, dump planes or None).  misalign: the output starts 4 bytes off a 16-byte boundary, which sends a W % 4 == 0 shape down
    the one-element-per-step kernel."""
    import torch
    from eld_amd import _lib as L
    from eld_amd.noise import sample_noise_records
    out = None
    if misalign:
        out = torch.empty(y.numel() + 4, dtype=torch.float32, device=y.device)[1:1 + y.numel()].view(y.shape)
        assert out.data_ptr() % 16 == 4
    d = torch.zeros(L.NPLANES, y.numel(), device=y.device) if dump else None
    z = sample_noise_records(y, recs, flags, R.SEED, dump=d, out=out, dark=pool)
    torch.cuda.synchronize()
    return z.cpu().numpy(), (None if d is None else d.cpu().numpy())


CASES = [('bayer', p, pat) for p in R.BAYER_PATCHES for pat in R.PATTERNS] + [('xtrans', p, None) for p in R.XTRANS_PATCHES]


@pytest.mark.parametrize('cfa,patch,pattern', CASES)
def test_gather_is_the_crop_of_the_packed_frame(dev, cfa, patch, pattern):
    """y = 0, model D: out = (code - black_c) * ratio / S at the sites dark_choice names, bit for bit; the aligned and the misaligned launch
    (vector and scalar kernels) agree."""
    import torch
    from eld_amd import _lib as L
    pool, ext, black = _setup(cfa, dev, pattern)
    C, H, W = patch
    full = (H, W) == pool.min_extent and cfa == 'bayer'
    rng = (0, 1) if full else (0, 3)             # the whole extent of the smallest frame: that frame alone, the origin forced
    flags = L.DARK | (L.CFA_XTRANS if cfa == 'xtrans' else 0)
    y = torch.zeros((len(IDS), C, H, W), dtype=torch.float32, device=dev)
    z, _ = _run(y, _records(IDS, rng), flags, pool)
    z2, _ = _run(y, _records(IDS, rng), flags, pool, misalign=True)
    p = _oracle_params()
    seen = set()
    for n, sid in enumerate(IDS):
        ch = R.dark_choice(R.SEED, sid, rng[0], rng[1], ext, H, W, cfa)
        seen.add(ch)
        want = R.dark_arith(np.zeros(patch, np.float32), p, flags, ch, pool.mosaics, pattern, black, {})
        code = R.dark_codes(pool.mosaics[ch[0]], cfa, pattern, ch[1], ch[2], H, W).astype(np.float32)
        by_hand = ((code - R.plane_black(cfa, black).reshape(C, 1, 1)).astype(np.float32) * np.float32(RATIO)).astype(np.float32) / np.float32(SAT)
        assert np.array_equal(want, by_hand.astype(np.float32))
        assert np.array_equal(z[n], want), (sid, ch)
        assert np.array_equal(z2[n], want), (sid, ch)
    assert len(seen) == 1 if full else len(seen) > 4


@pytest.mark.parametrize('cfa,patch,pattern', CASES)
@pytest.mark.parametrize('clip', [False, True])
def test_full_chain_replays_from_dumped_variates(dev, cfa, patch, pattern, clip):
    """PDU and PDU|CLIP on a synthetic image: the debug kernel's output equals dark_arith on the variates it dumped, and the production
    kernels (compile-time specialisation where W % 4 == 0, run-time flags otherwise and when misaligned) give the same bits."""
    import torch
    from eld_amd import _lib as L
    pool, ext, black = _setup(cfa, dev, pattern)
    C, H, W = patch
    rng = (0, 1) if ((H, W) == pool.min_extent and cfa == 'bayer') else (0, 3)
    flags = L.SHOT_POISSON | L.DARK | L.QUANT | (L.CLIP if clip else 0) | (L.CFA_XTRANS if cfa == 'xtrans' else 0)
    g = np.random.default_rng(7)
    yn = (np.floor(65535.0 * g.uniform(size=(len(IDS), C, H, W)) ** 2.2) / 65535.0).astype(np.float32)      # rates from 0 to ~50: both Poisson regimes
    y = torch.from_numpy(yn).to(dev)
    recs = _records(IDS, rng)
    zd, dump = _run(y, recs, flags, pool, dump=True)
    zp, _ = _run(y, recs, flags, pool)
    zs, _ = _run(y, recs, flags, pool, misalign=True)
    p = _oracle_params()
    planes = {k: dump[j].reshape(yn.shape) for k, j in L.PLANE.items()}
    assert planes['counts'].max() > 32 and planes['counts'].min() == 0 and 0 <= planes['u_q'].min() and planes['u_q'].max() < 1
    for n, sid in enumerate(IDS):
        ch = R.dark_choice(R.SEED, sid, rng[0], rng[1], ext, H, W, cfa)
        want = R.dark_arith(yn[n], p, flags, ch, pool.mosaics, pattern, black, {k: v[n] for k, v in planes.items()})
        assert np.array_equal(zd[n], want), (sid, ch)
    assert np.array_equal(zp, zd) and np.array_equal(zs, zd)
    if clip:
        assert zd.min() == 0.0 and zd.max() == 1.0            # codes below black and far above it: the clip acts at both ends


def _real_pool(dev, K=(1.5, 3.0)):
    from eld_amd.darkpool import DarkPool
    mos = R.mosaics_of(((20, 28), (24, 40), (22, 30), (20, 28), (26, 34)))
    sessions = [{'iso': 100, 'bias': mos[:3]}, {'iso': 800, 'bias': mos[3:]}]
    return DarkPool(sessions, raw_pattern=R.PATTERNS[0], black_level=R.BLACK, white_level=16383, K=K, device=dev), mos


def test_one_batch_equals_single_launches(dev):
    import torch
    from eld_amd import _lib as L
    from eld_amd.noise import NoiseParams, sample_noise
    pool, mos = _real_pool(dev)
    flags = L.SHOT_POISSON | L.DARK | L.QUANT | L.CLIP
    g = np.random.default_rng(3)
    y = torch.from_numpy(g.uniform(size=(4, 4, 8, 12)).astype(np.float32)).to(dev)
    prm = [NoiseParams(pool.K[i % 2], 0.0, pool.saturation, 120.0 + i, dark=pool.ranges[i % 2]) for i in range(4)]
    ids = [11, 5, 1 << 40, 7]
    whole = sample_noise(y, prm, flags, R.SEED, ids, dark=pool).cpu().numpy()
    for i in range(4):
        one = sample_noise(y[i:i + 1].contiguous(), prm[i:i + 1], flags, R.SEED, ids[i:i + 1], dark=pool).cpu().numpy()
        assert np.array_equal(one[0], whole[i])
    # the session's range is honoured: D alone on y = 0 reproduces codes of that session's frames only
    z = sample_noise(torch.zeros_like(y), prm, L.DARK, R.SEED, ids, dark=pool).cpu().numpy()
    ext = [R.packed_extent(*m.shape, 'bayer') for m in mos]
    for i in range(4):
        f, y0, x0 = R.dark_choice(R.SEED, ids[i], *pool.ranges[i % 2], ext, 8, 12, 'bayer')
        assert pool.ranges[i % 2][0] <= f < sum(pool.ranges[i % 2])
        code = R.dark_codes(mos[f], 'bayer', R.PATTERNS[0], y0, x0, 8, 12).astype(np.float32)
        d = (code - np.asarray(R.BLACK, np.float32).reshape(4, 1, 1)).astype(np.float32)
        want = ((d * np.float32(prm[i][3])).astype(np.float32) / np.float32(pool.saturation)).astype(np.float32)
        assert np.array_equal(z[i], want)


def test_synthesize_burst_draws_a_crop_per_frame(dev):
    """ELDModel.synthesize(burst=2): frame k of image i carries its own sample id, hence its own crop, and equals the direct call."""
    import torch
    from eld_amd import _lib as L
    from eld_amd.model import ELDModel
    from eld_amd.noise import NoiseModel, make_records, sample_noise_records
    pool, mos = _real_pool(dev)
    with contextlib.redirect_stdout(io.StringIO()):
        nm = NoiseModel(model='PDU', include=4, dark=pool)
    m = ELDModel.__new__(ELDModel)                 # synthesize() needs the sampler's state only, not a network
    m.noise_model, m._sample_counter, m.world, m.rank, m.seed = nm, 0, 1, 0, R.SEED
    g = np.random.default_rng(4)
    clean = torch.from_numpy(g.uniform(size=(3, 4, 8, 12)).astype(np.float32)).to(dev)
    np.random.seed(9)
    prm = [nm._sample_params() for _ in range(3)]
    out = m.synthesize(clean, prm, burst=2)
    assert tuple(out.shape) == (3, 8, 8, 12) and m._sample_counter == 6
    flags = L.SHOT_POISSON | L.DARK | L.QUANT | L.CLIP
    ext = [R.packed_extent(*x.shape, 'bayer') for x in mos]
    for k in range(2):
        ids = [2 * i + k for i in range(3)]
        direct = sample_noise_records(clean, make_records(prm, ids), flags, R.SEED, dark=pool)
        assert torch.equal(out[:, 4 * k:4 * k + 4], direct)
    crops = [[R.dark_choice(R.SEED, 2 * i + k, *prm[i].dark, ext, 8, 12, 'bayer') for k in range(2)] for i in range(3)]
    assert all(a != b for a, b in crops)
    assert not torch.equal(out[:, :4], out[:, 4:])
    # the plain call route: NoiseModel.__call__ reaches the same entry
    z = nm(clean, params=prm)
    assert tuple(z.shape) == tuple(clean.shape) and torch.isfinite(z).all()


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_bad_record_skips_its_image_only(dev, cfa):
    """A record whose range leaves the table (or is empty) leaves its slice of a NaN-filled output untouched; its neighbours are right."""
    import torch
    from eld_amd import _lib as L
    from eld_amd.noise import sample_noise_records
    pool, ext, black = _setup(cfa, dev, R.PATTERNS[0] if cfa == 'bayer' else None)
    C, H, W = (4, 8, 12) if cfa == 'bayer' else (9, 6, 8)
    flags = L.DARK | (L.CFA_XTRANS if cfa == 'xtrans' else 0)
    recs = _records([0, 1, 2, 3, 4], (0, 3))
    recs['reserved'][1] = (2, 2)              # 2 + 2 > F = 3
    recs['reserved'][3] = (1, 0)              # an empty range
    y = torch.zeros((5, C, H, W), dtype=torch.float32, device=dev)
    out = torch.full((5, C, H, W), float('nan'), dtype=torch.float32, device=dev)
    sample_noise_records(y, recs, flags, R.SEED, out=out, dark=pool)
    torch.cuda.synchronize()
    z = out.cpu().numpy()
    assert np.isnan(z[1]).all() and np.isnan(z[3]).all()
    p = _oracle_params()
    for n in (0, 2, 4):
        ch = R.dark_choice(R.SEED, n, 0, 3, ext, H, W, cfa)
        assert np.array_equal(z[n], R.dark_arith(np.zeros((C, H, W), np.float32), p, flags, ch, pool.mosaics, pool.raw_pattern, black, {}))


def test_sampler_call_refuses_a_missing_or_wrong_pool(dev):
    import torch
    from eld_amd import _lib as L
    from eld_amd.noise import sample_noise_records
    pool, _, _ = _setup('bayer', dev, R.PATTERNS[0])
    y = torch.zeros((1, 4, 8, 12), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match='DarkPool'):
        sample_noise_records(y, _records([0], (0, 3)), L.DARK, R.SEED)
    y9 = torch.zeros((1, 9, 4, 6), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match='holds bayer frames'):
        sample_noise_records(y9, _records([0], (0, 3)), L.DARK | L.CFA_XTRANS, R.SEED, dark=pool)


def test_manifest_pool_feeds_the_frame_pool_loader(dev, tmp_path):
    """calibrate's manifest -> DarkPool.from_manifest (gains given) -> NoiseModel('PDU') -> FramePoolLoader batch -> synthesize: the records of
    the collated batch carry the session's range, and the uint16 route equals the direct call on the decoded patch."""
    import json
    import torch
    from eld_amd import _lib as L
    from eld_amd.darkpool import DarkPool
    from eld_amd.framepool import FramePool, FramePoolLoader
    from eld_amd.model import ELDModel
    from eld_amd.noise import NoiseModel, decode_augment_u16, sample_noise_records
    from eld_amd.data import records_from_batch
    mos = R.mosaics_of(((24, 32),) * 5)
    names = []
    for i, m in enumerate(mos):
        np.save(tmp_path / ('b%d.npy' % i), m)
        names.append('b%d.npy' % i)
    man = {'raw_pattern': [[0, 1], [3, 2]], 'black_level': list(R.BLACK), 'white_level': 16383,
           'sessions': [{'iso': 100, 'bias': names[:3], 'flats': [[names[0], names[1]]]}, {'iso': 800, 'bias': names[3:], 'flats': [[names[3], names[4]]]}]}
    (tmp_path / 'manifest.json').write_text(json.dumps(man))
    pool = DarkPool.from_manifest(str(tmp_path / 'manifest.json'), K=[1.5, 3.0], device=dev)
    assert pool.ranges == [(0, 3), (3, 2)] and pool.min_extent == (12, 16) and pool.saturation == 16383 - max(R.BLACK)
    with contextlib.redirect_stdout(io.StringIO()):
        nm = NoiseModel(model='PDU', include=4, dark=pool)
    g = np.random.default_rng(5)
    clean = FramePool([g.integers(600, 9000, size=(40, 48)).astype(np.uint16)], raw_pattern=[[0, 1], [3, 2]], black_level=list(R.BLACK), device=dev)
    with pytest.raises(ValueError, match='smallest dark frame'):
        pool.check_patch(16, 16)
    loader = FramePoolLoader(clean, nm, 3, patch=8, steps_per_epoch=1, augment=False)
    np.random.seed(2)
    batch = next(iter(loader))
    recs = records_from_batch(batch['params'])
    assert all(tuple(r) in pool.ranges for r in recs['reserved'].tolist())
    m = ELDModel.__new__(ELDModel)
    m.noise_model, m._sample_counter, m.world, m.rank, m.seed = nm, 0, 1, 0, R.SEED
    out = m.synthesize(batch['target'], batch['params'])
    flags = L.SHOT_POISSON | L.DARK | L.QUANT | L.CLIP
    from eld_amd.noise import set_sample_ids
    direct = sample_noise_records(decode_augment_u16(batch['target']), set_sample_ids(recs, [0, 1, 2]), flags, R.SEED, dark=pool)
    assert torch.equal(out, direct) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
