"""GPU tests of the frame pool: the crop kernels (csrc/framepool.hip) against the NumPy restatement and the reference-minted fixture, all
codes equal; a pool batch trains bit-identically to the same patches delivered as host arrays through the deferred path; paired mode;
Engine.train over a FramePoolLoader; python -m eld_amd.train_frames end to end.  Every record a test hands to the kernel lies inside
its frame."""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import framepool_ref as R               # noqa: E402
from oracle import noise_ref as O       # noqa: E402  (checker only)

PATTERNS = ([[0, 1], [3, 2]], [[1, 0], [2, 3]], [[3, 2], [0, 1]], [[2, 3], [1, 0]])       # R at each of the four cell positions
BLACKS = (512, 1024, (512, 520, 500, 516), 0)
RATIOS = (1.0, 100.0, 250.0, 300.0)


def mosaic(rng, shape, black, white):
    """Codes below black, near it (so that ratios up to 300 do not all saturate), anywhere up to white, and at white."""
    kind = rng.integers(0, 8, size=shape)
    u = np.where(kind < 4, black + rng.integers(-40, 200, size=shape), np.where(kind < 7, rng.integers(0, white + 1, size=shape), white))
    return np.clip(u, 0, white).astype(np.uint16)


def records(rng, extents, ph, pw, n=10):
    """Patches flush with every frame edge, odd and even offsets, frames interleaved, ratios cycling -- all inside their frames."""
    rows = []
    for f, (hp, wp) in enumerate(extents):
        my, mx = hp - ph, wp - pw
        rows += [(f, 0, 0), (f, my, mx), (f, 0, mx), (f, my, 0), (f, min(1, my), min(1, mx)), (f, min(2, my), min(3, mx)), (f, min(3, my), min(4, mx))]
        rows += [(f, int(rng.integers(0, my + 1)), int(rng.integers(0, mx + 1))) for _ in range(n)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return [(f, y, x, RATIOS[i % len(RATIOS)]) for i, (f, y, x) in enumerate(rows)]


def run(pool, recs, ph, pw):
    from eld_amd.framepool import Crops
    a = np.array(recs, np.float64)
    got = pool.patches(Crops.make(a[:, 0], a[:, 1], a[:, 2], ph, pw, ratios=a[:, 3]))
    assert got.dtype == torch.int16 and got.is_cuda
    return got.cpu().numpy().view(np.uint16)


def check(pool, frames, cfa, recs, ph, pw, black, white, pattern=None, both_paths=None):
    from eld_amd.framepool import Crops
    a = np.array(recs, np.float64)
    if both_paths is not None:                               # this set of records exercises the 16-byte AND the 4-byte load path
        wide = pool.wide_loads(Crops.make(a[:, 0], a[:, 1], a[:, 2], ph, pw))
        assert wide.any() == both_paths and (not wide.all())
    got = run(pool, recs, ph, pw)
    want = R.patches(frames, cfa, recs, ph, pw, raw_pattern=pattern, black=np.reshape(black, -1).tolist() if cfa == 'xtrans' else black, white=white)
    assert got.shape == want.shape
    assert np.array_equal(got, want), '%d of %d codes differ' % (np.count_nonzero(got != want), got.size)


@pytest.mark.parametrize('white', [16383, 65535])
@pytest.mark.parametrize('pi', range(4))
def test_bayer_kernel_equals_restatement(eld_lib, pi, white):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(100 * pi + white)
    for black in BLACKS:
        b4 = list(black) if isinstance(black, tuple) else [black] * 4
        frames = [mosaic(rng, s, b4[0], white) for s in ((96, 128), (70, 108), (64, 100))]      # row pitches: 128 (16-byte path possible), 108, 100
        pool = FramePool(frames, raw_pattern=PATTERNS[pi], black_level=b4, white_point=white)
        ext = [R.packed_extent(*f.shape, 'bayer') for f in frames]
        for ph, pw, both in ((16, 16, True), (24, 40, True), (17, 13, False), (32, 8, True), (5, 50, False)):
            check(pool, frames, 'bayer', records(rng, ext, ph, pw), ph, pw, b4, white, PATTERNS[pi], both_paths=both)


def test_bayer_training_shape_and_a_whole_bench_frame(eld_lib):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(5)
    shapes = ((2848, 4256), (1040, 1100), (1030, 1088))
    frames = [mosaic(rng, s, 512, 16383) for s in shapes]
    pool = FramePool(frames, raw_pattern=PATTERNS[0], black_level=[512, 520, 500, 516])
    ext = [R.packed_extent(*s, 'bayer') for s in shapes]
    check(pool, frames, 'bayer', records(rng, ext, 512, 512, n=2), 512, 512, [512, 520, 500, 516], 16383, PATTERNS[0], both_paths=True)
    whole = [(0, 0, 0, 1.0), (0, 0, 0, 100.0)]               # 4 x 1424 x 2128 as a single patch
    check(pool, frames, 'bayer', whole, 1424, 2128, [512, 520, 500, 516], 16383, PATTERNS[0])
    g = pool.grid((4, 512, 512), (4, 512, 512))
    assert len(g) == 2 * 4 + 1 + 1 and pool.patches(g).shape == (10, 4, 512, 512)


@pytest.mark.parametrize('black,white', [(1024, 16383), (0, 65535), (512, 16383), (1024, 65535)])
def test_xtrans_kernel_equals_restatement(eld_lib, black, white):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(black + white)
    frames = [mosaic(rng, s, black, white) for s in ((100, 130), (70, 94), (64, 128))]           # sides not multiples of 6; one row pitch of 128
    pool = FramePool(frames, cfa='xtrans', black_level=black, white_point=white)
    ext = [R.packed_extent(*f.shape, 'xtrans') for f in frames]
    assert ext == [(32, 42), (22, 30), (20, 42)]
    for ph, pw, both in ((16, 16, True), (8, 24, True), (7, 5, False), (6, 10, False), (20, 8, True), (1, 30, False)):
        check(pool, frames, 'xtrans', records(rng, ext, ph, pw), ph, pw, black, white, both_paths=both)


def test_xtrans_training_shape_and_a_whole_frame(eld_lib):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(6)
    shapes = ((1566, 1600), (1570, 1610))                    # packed 522 x 532 and 522 x 536
    frames = [mosaic(rng, s, 1024, 16383) for s in shapes]
    pool = FramePool(frames, cfa='xtrans')
    ext = [R.packed_extent(*s, 'xtrans') for s in shapes]
    assert ext == [(522, 532), (522, 536)]
    check(pool, frames, 'xtrans', records(rng, ext, 512, 512, n=1), 512, 512, 1024, 16383, both_paths=True)
    check(pool, frames, 'xtrans', [(0, 0, 0, 1.0), (1, 0, 0, 300.0)], 522, 532, 1024, 16383)      # whole frame 0 as one patch (one-code-per-lane kernel)
    check(pool, frames, 'xtrans', [(1, 0, 0, 100.0)], 522, 536, 1024, 16383)                       # whole frame 1 (16-byte stores)


def test_fixture_grid_on_the_device(eld_lib, golden_dir):
    """pool.patches(pool.grid(...)) is the content of the reference's patch database, record for record."""
    from eld_amd.framepool import FramePool
    gold = np.load(os.path.join(golden_dir, 'framepool.npz'))
    k = int(gold['ksize'])
    for name, cfa in (('bayer_a', 'bayer'), ('bayer_b', 'bayer'), ('xtrans', 'xtrans')):
        pool = FramePool([gold[name + '_mosaic']], cfa=cfa, raw_pattern=gold[name + '_pattern'] if cfa == 'bayer' else None,
                         black_level=gold[name + '_black'].tolist(), white_point=int(gold['white']))
        g = pool.grid((pool.C, k, k), (pool.C, k, k))
        for r in gold['ratios']:
            got = pool.patches(g, ratios=float(r)).cpu().numpy().view(np.uint16)
            assert np.array_equal(got, gold['%s_codes_r%d' % (name, r)]), (name, int(r))
        assert np.array_equal(pool.patches(g).cpu().numpy().view(np.uint16), gold[name + '_codes_r1'])      # grid() carries ratio 1
    both = FramePool([torch.from_numpy(gold['bayer_a_mosaic'].view(np.int16)).cuda(), gold['bayer_a_mosaic'][:40, :60]],
                     raw_pattern=gold['bayer_a_pattern'], black_level=gold['bayer_a_black'].tolist())      # a CUDA tensor is taken as it is
    g = both.grid((4, k, k), (4, k, k))
    assert np.array_equal(both.patches(g[:4]).cpu().numpy().view(np.uint16), gold['bayer_a_codes_r1'])


# ---- downstream ---------------------------------------------------------------------------------------------------------------
def make_opt(tmp, **kw):
    d = dict(gpu_ids=[0], isTrain=True, checkpoints_dir=str(tmp), name='t', netG='unet', channels=4, stage_in='raw', stage_out='raw',
             lr=1e-4, beta1=0.9, wd=0.0, loss='l1', resume=False, chop=False, no_log=True, save_epoch_freq=100, model='eld_model', seed=2018)
    d.update(kw)
    return types.SimpleNamespace(**d)


def noise_model(letters='PGRU'):
    from eld_amd.noise import NoiseModel
    with contextlib.redirect_stdout(io.StringIO()):
        return NoiseModel(model=letters, include=4)


def small_pool(seed=3, **kw):
    from eld_amd.framepool import FramePool
    rng = np.random.default_rng(seed)
    frames = [mosaic(rng, s, 512, 16383) for s in ((200, 264), (180, 200), (160, 320))]
    return frames, FramePool(frames, raw_pattern=PATTERNS[0], black_level=512, **kw)


def train_losses(engine, batches):
    """Engine.train's loop with its one-batch lookahead, returning the loss of every step as the float the reference logs."""
    model, losses = engine.model, []
    it = iter(batches)
    data = next(it, None)
    while data is not None:
        model.set_input(data, mode='train')
        nxt = next(it, None)
        if nxt is not None:
            model.prefetch_input(nxt, mode='train')
        model.optimize_parameters()
        losses.append(model.get_current_errors()['Pixel'])
        data = nxt
    return losses


@pytest.mark.parametrize('precision,burst', [('fp32', 1), ('bf16', 2), ('fp32', 2), ('bf16', 1)])
def test_pool_batches_train_like_host_arrays(eld_lib, tmp_path, precision, burst):
    """Same seed, same sample ids, same parameters: a pool batch and the same patches as host uint16 arrays give the same losses, bit for bit."""
    from eld_amd.engine import Engine
    from eld_amd.framepool import FramePoolLoader
    frames, pool = small_pool()
    nm = noise_model()
    loader = FramePoolLoader(pool, nm, 2, patch=64, steps_per_epoch=4, num_burst=burst)
    np.random.seed(11)
    draws = [loader.draw() for _ in range(4)]
    runs = []
    for source in ('pool', 'host'):
        batches = []
        for crops, params, bits in draws:
            b = loader.batch(crops, params, bits)
            assert set(b) == {'target', 'params', 'aug', 'burst'} and b['target'].is_cuda and b['target'].dtype == torch.int16
            if source == 'host':                             # the restatement's codes as a host array: the existing deferred path
                recs = [(int(r['frame']), int(r['y0']), int(r['x0']), None) for r in crops.records]
                host = R.patches(frames, 'bayer', recs, 64, 64, raw_pattern=PATTERNS[0], black=[512] * 4, white=16383)
                b = dict(b, target=torch.from_numpy(host.view(np.int16)))
            batches.append(b)
        torch.manual_seed(2018)
        with contextlib.redirect_stdout(io.StringIO()):
            engine = Engine(make_opt(tmp_path, in_channels=4 * burst, precision=precision))
        engine.model.set_noise_model(nm)
        runs.append(train_losses(engine, batches))
        assert tuple(engine.model.input.shape) == (2, 4 * burst, 64, 64)
    assert len(runs[0]) == 4 and all(np.isfinite(runs[0]))
    assert [np.float64(v).tobytes() for v in runs[0]] == [np.float64(v).tobytes() for v in runs[1]], runs


def test_paired_mode(eld_lib, tmp_path):
    """'input' is clip(codes / 65535) of the ratio-scaled short frame; input and target are cut at the same place under every augmentation bit."""
    from eld_amd.engine import Engine
    from eld_amd.framepool import Crops, FramePool, FramePoolLoader
    frames, pool = small_pool()
    rng = np.random.default_rng(8)
    short = [mosaic(rng, f.shape, 512, 16383) for f in frames]
    inputs = FramePool(short, raw_pattern=PATTERNS[0], black_level=512)
    ratios = [100.0, 250.0, 300.0]
    loader = FramePoolLoader(pool, None, 8, patch=32, inputs=inputs, ratios=ratios)
    crops = Crops.make([0, 1, 2, 0, 1, 2, 0, 1], [0, 3, 48, 68, 58, 1, 7, 20], [100, 0, 5, 1, 68, 128, 33, 2], 32, 32)
    batch = loader.batch(crops, None, list(range(8)))        # every combination of the three augmentation bits
    assert set(batch) == {'input', 'target', 'aug'} and batch['input'].dtype == torch.float32
    recs = [(int(r['frame']), int(r['y0']), int(r['x0'])) for r in crops.records]
    kw = dict(raw_pattern=PATTERNS[0], black=[512] * 4, white=16383)
    want_in = O.lmdb_decode_u16(R.patches(short, 'bayer', [r + (ratios[r[0]],) for r in recs], 32, 32, **kw))
    want_tg = O.lmdb_decode_u16(R.patches(frames, 'bayer', [r + (None,) for r in recs], 32, 32, **kw))
    assert np.array_equal(batch['input'].cpu().numpy(), want_in)
    with contextlib.redirect_stdout(io.StringIO()):
        engine = Engine(make_opt(tmp_path))
    engine.model.set_input(batch, 'train')
    got_in, got_tg = engine.model.input.cpu().numpy(), engine.model.target.cpu().numpy()
    for i in range(8):
        assert np.array_equal(got_in[i], np.clip(O.augment(want_in[i], i & 1, i & 2, i & 4), 0, 1)), i
        assert np.array_equal(got_tg[i], O.augment(want_tg[i], i & 1, i & 2, i & 4)), i
    np.random.seed(4)
    losses = train_losses(engine, list(loader)[:2])          # and the drawn batches train
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_engine_trains_from_the_pool_and_a_seed_reproduces_it(eld_lib, tmp_path):
    from eld_amd.engine import Engine
    from eld_amd.framepool import FramePoolLoader
    _, pool = small_pool()
    runs = []
    for _ in range(2):
        nm = noise_model()
        loader = FramePoolLoader(pool, nm, 2, patch=64, steps_per_epoch=3)
        torch.manual_seed(2018)
        np.random.seed(77)
        with contextlib.redirect_stdout(io.StringIO()):
            engine = Engine(make_opt(tmp_path))
            assert engine.model.noise_model is nm
            losses = []
            orig = engine.model.get_current_errors
            engine.model.get_current_errors = lambda: (losses.append(orig()['Pixel']) or {'Pixel': losses[-1]})
            while engine.epoch < 2:
                engine.train(loader)
        assert engine.epoch == 2 and engine.iterations == 6 and len(losses) == 6 and all(np.isfinite(losses))
        runs.append(losses)
    assert runs[0] == runs[1]
    assert len(set(runs[0])) > 1


@pytest.mark.parametrize('cfa', ['bayer', 'xtrans'])
def test_train_frames_end_to_end(eld_lib, tmp_path, cfa):
    """frames on disk -> python -m eld_amd.train_frames -> a checkpoint load_denoiser loads and denoise_raw runs."""
    from eld_amd import train_frames
    from eld_amd.denoise import denoise_raw, load_denoiser
    rng = np.random.default_rng(1)
    shape, black = ((96, 128), 512) if cfa == 'bayer' else ((108, 120), 1024)
    for i in range(2):
        np.save(tmp_path / ('long%d.npy' % i), mosaic(rng, shape, black, 16383))
    meta = {'cfa': cfa, 'black_level_per_channel': [black] * 4 if cfa == 'bayer' else black, 'white_level': 16383}
    if cfa == 'bayer':
        meta['raw_pattern'] = PATTERNS[0]
    (tmp_path / 'sensor.json').write_text(json.dumps(meta))
    ckpt = tmp_path / 'out' / 'model.pt'
    os.makedirs(tmp_path / 'out')
    with contextlib.redirect_stdout(io.StringIO()):
        rc = train_frames.main([str(tmp_path / 'long*.npy'), '--meta', str(tmp_path / 'sensor.json'), '--camera', 'SonyA7S2', '--noise', 'PGRU',
                                '--patch', '32', '--batch', '2', '--epochs', '2', '--steps', '2', '--lr', '1e-4', '-o', str(ckpt)])
    assert rc == 0 and ckpt.exists()
    den = load_denoiser(str(ckpt), cfa=cfa)
    assert den.in_channels == den.out_channels == (4 if cfa == 'bayer' else 9)
    raw = mosaic(rng, shape, black, 16383)
    res = denoise_raw(den, raw, cfa, raw_pattern=PATTERNS[0] if cfa == 'bayer' else None, black_level=black, ratio=100.0)
    assert res['mosaic'].shape == raw.shape and res['mosaic'].dtype == np.uint16 and np.isfinite(res['packed']).all()
