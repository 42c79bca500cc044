"""eld_amd.evaluate on the device: evaluate_pairs against the same numbers composed by hand from the package's public pieces (bit for bit:
the same kernels in the same order), the level sums against tests/pairstats_ref.py on the written-back codes, the command line and
train_frames --val.  No tolerance anywhere."""
import contextlib
import io
import json
import math
import os

import numpy as np
import pytest

import pairstats_ref as R

pytestmark = pytest.mark.gpu

PAT = [[0, 1], [3, 2]]
BLK, WHITE = 512, 16383


def _pair(rng, shape, black, ratio):
    """A long exposure with structure from black to near white, and a short one `ratio` times darker with read noise."""
    Hm, Wm = shape
    ramp = (np.arange(Wm)[None, :] / Wm) ** 2.2 * (0.5 + 0.5 * np.sin(np.arange(Hm)[:, None] / 7.0) ** 2)
    clean = ramp * (WHITE - black) * 0.9
    long_ = np.clip(np.rint(black + clean + rng.normal(0, 3, shape)), 0, 65535).astype(np.uint16)
    short = np.clip(np.rint(black + clean / ratio + rng.normal(0, 4, shape)), 0, 65535).astype(np.uint16)
    return short, long_


def _net(planes, seed=7):
    import torch
    from eld_amd.denoise import load_denoiser
    from eld_amd.unet import UNetSeeInDark
    torch.manual_seed(seed)
    return load_denoiser(UNetSeeInDark(planes, planes), cfa='bayer' if planes == 4 else 'xtrans')


@pytest.fixture(scope='module')
def bayer(eld_lib):
    rng = np.random.default_rng(3)
    s0, l0 = _pair(rng, (64, 96), BLK, 100.0)
    s1, l1 = _pair(rng, (64, 96), BLK, 200.0)
    pairs = [{'short': s0, 'long': l0, 'ratio': 100.0, 'iso': 800, 'name': 'p0'},
             {'short': s1, 'long': l1, 'iso': 1600, 'exposure': 0.05, 'long_iso': 100, 'long_exposure': 160.0, 'name': 'p1'}]
    return _net(4), pairs


def _by_hand(den, pr, cfa, pat, blk, correct, crop, chop=None):
    """The reference's evaluation of one pair from the public pieces -> (psnr, ssim, psnr_in, ssim_in, input, output, target, y0, x0)"""
    import torch
    from eld_amd.denoise import pack_input, run_network
    from eld_amd.evaluate import pair_ratio
    from eld_amd.metrics import illuminance_correct, quality_assess_frames
    dev = next(den.net.parameters()).device
    up = lambda m: torch.from_numpy(m.view(np.int16)).to(dev)[None]
    x = pack_input(up(pr['short']), cfa, pat, blk, float(WHITE), [pair_ratio(pr)])
    t = pack_input(up(pr['long']), cfa, pat, blk, float(WHITE), [1.0])
    y0 = x0 = 0
    if crop:
        y0, x0 = x.shape[2] // 2 - crop // 2, x.shape[3] // 2 - crop // 2
        x, t = x[:, :, y0:y0 + crop, x0:x0 + crop].contiguous(), t[:, :, y0:y0 + crop, x0:x0 + crop].contiguous()
    out = run_network(den, x, chop)
    if correct:
        out = illuminance_correct(out, t)
    q, qi = quality_assess_frames(out, t)[0].tolist(), quality_assess_frames(x, t)[0].tolist()
    return q[0], q[1], qi[0], qi[1], x, out, t, y0, x0


@pytest.mark.parametrize('correct,crop', [(True, None), (False, None), (True, 16), (False, 16)])
def test_rows_equal_the_composition_by_hand(bayer, correct, crop):
    from eld_amd.evaluate import evaluate_pairs
    den, pairs = bayer
    rep = evaluate_pairs(den, pairs, 'bayer', PAT, BLK, WHITE, correct=correct, crop=crop, levels=False)
    assert rep['pooled'] is None and [r['name'] for r in rep['pairs']] == ['p0', 'p1']
    assert rep['pairs'][1]['ratio'] == 100 * 160.0 / (1600 * 0.05) and rep['pairs'][1]['iso'] == 1600.0
    for row, pr in zip(rep['pairs'], pairs):
        want = _by_hand(den, pr, 'bayer', [0, 1, 3, 2], [512.0] * 4, correct, crop)
        assert (row['psnr'], row['ssim'], row['psnr_in'], row['ssim_in']) == want[:4]
        assert math.isfinite(row['psnr']) and 'sums' not in row


def test_a_shape_that_goes_through_forward_chop(bayer):
    from eld_amd.evaluate import evaluate_pairs
    den, _ = bayer
    rng = np.random.default_rng(4)
    s, l = _pair(rng, (72, 104), BLK, 50.0)                     # packed 36 x 52: not multiples of 16
    pr = {'short': s, 'long': l, 'ratio': 50.0}
    row = evaluate_pairs(den, [pr], 'bayer', PAT, BLK, WHITE, levels=False)['pairs'][0]
    assert (row['psnr'], row['ssim'], row['psnr_in'], row['ssim_in']) == _by_hand(den, pr, 'bayer', [0, 1, 3, 2], [512.0] * 4, True, None, chop=True)[:4]
    assert row['iso'] is None


@pytest.mark.parametrize('crop', [None, 16])
def test_level_sums_equal_the_restatement_on_the_written_back_codes(bayer, crop):
    import torch
    from eld_amd.denoise import write_back
    from eld_amd.evaluate import evaluate_pairs, level_curves
    den, pairs = bayer
    blk4 = [512, 520, 500, 512]                                 # per-channel black levels reach the per-cell table
    rep = evaluate_pairs(den, pairs, 'bayer', PAT, blk4, WHITE, crop=crop)
    black_cells = [blk4[c] for c in (0, 1, 3, 2)]
    pooled = {'output': 0, 'input': 0}
    for row, pr in zip(rep['pairs'], pairs):
        _, _, _, _, x, out, _, y0, x0 = _by_hand(den, pr, 'bayer', [0, 1, 3, 2], [float(b) for b in blk4], True, crop)
        n, m = x.shape[2:]
        ref = pr['long'][2 * y0:2 * y0 + 2 * n, 2 * x0:2 * x0 + 2 * m][None]
        for k, t in (('output', out), ('input', x)):
            codes = torch.zeros((1, 2 * n, 2 * m), dtype=torch.int16, device=t.device)
            write_back(t, codes, 'bayer', [0, 1, 3, 2], [float(b) for b in blk4], float(WHITE), 'nearest')
            want = R.pair_level_sums(codes.cpu().numpy().view(np.uint16), ref, 2, [0, 1, 3, 2], 4, black_cells, WHITE)[0]
            assert np.array_equal(row['sums'][k], want)
            assert int(want[..., 0].sum()) == 4 * n * m
            pooled[k] = pooled[k] + want
        c = level_curves(row['sums']['output'], span=[WHITE - b for b in blk4])
        assert np.array_equal(row['psnr_codes'], c['psnr_codes']) and np.all(np.isfinite(row['psnr_codes']))
        assert np.array_equal(row['curves']['output']['bias'], c['bias'], equal_nan=True)
    for k in pooled:
        assert np.array_equal(rep['pooled'][k]['n'], pooled[k][..., 0])
        assert np.array_equal(rep['pooled'][k]['bias'], level_curves(pooled[k])['bias'], equal_nan=True)
    # no claim on quality here (the network is random): only that output and input are two different sets of sums
    assert not np.array_equal(rep['pairs'][0]['sums']['output'], rep['pairs'][0]['sums']['input'])


def test_closed_loop_on_the_statistics(eld_lib):
    from eld_amd.evaluate import level_curves, pair_level_stats
    rng = np.random.default_rng(8)
    d = {0: 3, 1: -2, 2: 0, 3: 7}                               # per group (R, G1, B, G2)
    ref = rng.integers(400, 16000, size=(2, 34, 70)).astype(np.uint16)       # no clipping reached on either side
    cell = np.array(PAT)[np.arange(34)[:, None] % 2, np.arange(70)[None, :] % 2]
    est = (ref.astype(np.int64) + np.vectorize(d.get)(cell)).astype(np.uint16)
    sums = pair_level_stats(est, ref, 'bayer', PAT, BLK, WHITE)
    assert np.array_equal(sums, R.pair_level_sums(est, ref, 2, [0, 1, 3, 2], 4, [BLK] * 4, WHITE))
    c = level_curves(sums, span=WHITE - BLK)
    for g, dg in d.items():
        has = c['n'][:, g] > 0
        assert has.sum() > 20
        assert np.all(c['bias'][:, g][has] == dg) and np.all(c['rmse'][:, g][has] == abs(dg))
    import torch                                                # CUDA tensors in, one frame without the batch axis
    one = pair_level_stats(torch.from_numpy(est[0].view(np.int16)).cuda(), torch.from_numpy(ref[0].view(np.int16)).cuda(), 'bayer', PAT, BLK, WHITE)
    assert np.array_equal(one, sums[:1])


def test_defects_and_shading_reach_the_input_stage(bayer):
    import torch
    from eld_amd.defects import DefectMap, repair_device
    from eld_amd.denoise import denoise_raw, pack_input
    from eld_amd.evaluate import evaluate_pairs
    from eld_amd.shading import DarkShading
    den, pairs = bayer
    rng = np.random.default_rng(12)
    Hm, Wm = 64, 96
    sh = DarkShading((3 * rng.standard_normal((Hm, Wm))).astype(np.float32), (rng.standard_normal((Hm, Wm)) / 800).astype(np.float32), 1500.0, 800, 3200,
                     'bayer', PAT)
    dmap = DefectMap.from_sites([(3, 5), (40, 77)], (Hm, Wm))
    pr = dict(pairs[0])
    pr['short'] = pr['short'].copy()
    pr['long'] = pr['long'].copy()
    pr['short'][3, 5] = pr['long'][40, 77] = 16000                 # hot pixels on both sides
    seen = {}
    rep = evaluate_pairs(den, [pr], 'bayer', PAT, BLK, WHITE, correct=False, defects=dmap, shading=sh, on_pair=lambda i, row, t: seen.update(t))
    dev = seen['input'].device
    up = lambda m: torch.from_numpy(m.view(np.int16)).to(dev)[None]
    want_x = pack_input(repair_device(up(pr['short']), dmap), 'bayer', [0, 1, 3, 2], [512.0] * 4, 16383.0, [100.0], sh, sh.t(800))
    assert torch.equal(seen['input'], want_x)
    assert not torch.equal(want_x, pack_input(up(pr['short']), 'bayer', [0, 1, 3, 2], [512.0] * 4, 16383.0, [100.0]))
    want_t = pack_input(repair_device(up(pr['long']), dmap), 'bayer', [0, 1, 3, 2], [512.0] * 4, 16383.0, [1.0])
    assert torch.equal(seen['target'], want_t)                      # the target: repaired, ratio 1, no shading
    res = denoise_raw(den, pr['short'], 'bayer', raw_pattern=PAT, black_level=BLK, ratio=100.0, defects=dmap, shading=sh, iso=800)
    assert np.array_equal(seen['output'].cpu().numpy(), res['packed'])      # the same input went through the same network
    # the flagged sites are not counted, and the reference codes are the repaired ones
    n_out = int(rep['pairs'][0]['sums']['output'][..., 0].sum())
    assert n_out == Hm * Wm - 2
    est = denoise_raw(den, pr['short'], 'bayer', raw_pattern=PAT, black_level=BLK, ratio=100.0, defects=dmap, shading=sh, iso=800)['mosaic']
    ref = repair_device(up(pr['long']), dmap).cpu().numpy().view(np.uint16)
    assert np.array_equal(rep['pairs'][0]['sums']['output'], R.pair_level_sums(est[None], ref, 2, [0, 1, 3, 2], 4, [BLK] * 4, WHITE, mask=dmap.mask)[0])


def test_table_and_means(bayer):
    from eld_amd.evaluate import evaluate_pairs
    den, pairs = bayer
    three = [pairs[0], pairs[1], dict(pairs[0], short=pairs[1]['short'], name='p2')]
    rep = evaluate_pairs(den, three, 'bayer', PAT, BLK, WHITE, levels=False)
    rows = rep['pairs']
    assert [(t['iso'], t['ratio'], t['count']) for t in rep['table']] == [(800.0, 100.0, 2), (1600.0, 200.0, 1)]
    for k in ('psnr', 'ssim', 'psnr_in', 'ssim_in'):
        assert rep['table'][0][k] == float(np.mean([rows[0][k], rows[2][k]])) and rep['table'][1][k] == rows[1][k]
        assert rep['mean'][k] == float(np.mean([r[k] for r in rows]))
    assert rep['groups'] == ['R', 'G1', 'B', 'G2']


def test_xtrans_pair_and_a_crop_that_starts_inside_a_cell(eld_lib):
    import torch
    from eld_amd.defects import xtrans_tables
    from eld_amd.denoise import write_back
    from eld_amd.evaluate import evaluate_pairs
    den = _net(9)
    colour = xtrans_tables()['colour']
    rng = np.random.default_rng(21)
    for shape, crop in (((48, 48), None), ((56, 58), 16)):      # packed 16 x 16 whole; packed 18 x 18 cut at (1, 1): mosaic site (3, 3)
        s, l = _pair(rng, shape, 1024, 100.0)
        pr = {'short': s, 'long': l, 'ratio': 100.0, 'iso': 400}
        rep = evaluate_pairs(den, [pr], 'xtrans', None, 1024, WHITE, crop=crop)
        row = rep['pairs'][0]
        psnr, ssim, psnr_in, ssim_in, x, out, _, y0, x0 = _by_hand(den, pr, 'xtrans', None, [1024.0], True, crop)
        assert (row['psnr'], row['ssim'], row['psnr_in'], row['ssim_in']) == (psnr, ssim, psnr_in, ssim_in)
        hp, wp = 2 * (shape[0] // 6), 2 * (shape[1] // 6)
        n = x.shape[2]
        assert (y0, x0) == ((0, 0) if crop is None else (1, 1))
        for k, t in (('output', out), ('input', x)):
            full = torch.zeros((1, 9, hp, wp), dtype=torch.float32, device=t.device)
            full[:, :, y0:y0 + n, x0:x0 + n] = t
            codes = torch.from_numpy(l.view(np.int16)).to(t.device)[None].clone()
            write_back(full, codes, 'xtrans', None, [1024.0], float(WHITE), 'nearest')
            outside = np.ones(shape, bool)
            outside[3 * y0:3 * (y0 + n), 3 * x0:3 * (x0 + n)] = False
            want = R.pair_level_sums(codes.cpu().numpy().view(np.uint16), l[None], 6, colour.reshape(-1), 3, [1024] * 36, WHITE, mask=outside)[0]
            assert np.array_equal(row['sums'][k], want)
            assert int(want[..., 0].sum()) == 9 * n * n
        assert rep['groups'] == ['R', 'G', 'B']


def test_command_line_writes_the_numbers_of_the_api(bayer, tmp_path):
    import torch
    from eld_amd import evaluate as E
    from eld_amd.validate import to_jsonable
    den, pairs = bayer
    torch.save({'netG': den.net.state_dict()}, str(tmp_path / 'net.pt'))
    man = {'cfa': 'bayer', 'raw_pattern': PAT, 'black_level_per_channel': [BLK] * 4, 'white_level': WHITE, 'pairs': []}
    for pr in pairs:
        np.save(str(tmp_path / (pr['name'] + '_s.npy')), pr['short'])
        np.save(str(tmp_path / (pr['name'] + '_l.npy')), pr['long'])
        q = {k: v for k, v in pr.items() if k not in ('short', 'long')}
        man['pairs'].append(dict(q, short=pr['name'] + '_s.npy', long=pr['name'] + '_l.npy'))
    (tmp_path / 'pairs.json').write_text(json.dumps(man))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = E.main([str(tmp_path / 'pairs.json'), '--ckpt', str(tmp_path / 'net.pt'), '--crop', '16', '--json', str(tmp_path / 'rep.json')])
    assert rc == 0
    text = buf.getvalue()
    assert 'PSNR' in text and 'bias out' in text and 'G2:' in text
    got = json.loads((tmp_path / 'rep.json').read_text())
    want = json.loads(json.dumps(to_jsonable(E.evaluate_pairs(den, pairs, 'bayer', PAT, [BLK] * 4, WHITE, crop=16))))
    assert got == want or json.dumps(got) == json.dumps(want)       # NaN != NaN: the texts then agree
    assert got['table'][0]['psnr'] == want['table'][0]['psnr'] and got['pairs'][1]['sums']['output'] == want['pairs'][1]['sums']['output']


def test_train_frames_val_prints_and_leaves_training_alone(eld_lib, tmp_path):
    import torch
    from eld_amd import train_frames
    rng = np.random.default_rng(1)
    for i in range(2):
        np.save(str(tmp_path / ('long%d.npy' % i)), _pair(rng, (96, 128), BLK, 1.0)[1])
    s, l = _pair(rng, (64, 96), BLK, 100.0)
    np.save(str(tmp_path / 'vs.npy'), s)
    np.save(str(tmp_path / 'vl.npy'), l)
    meta = {'cfa': 'bayer', 'black_level_per_channel': [BLK] * 4, 'white_level': WHITE, 'raw_pattern': PAT}
    (tmp_path / 'sensor.json').write_text(json.dumps(meta))
    (tmp_path / 'val.json').write_text(json.dumps(dict(meta, pairs=[{'short': 'vs.npy', 'long': 'vl.npy', 'ratio': 100, 'iso': 800}])))
    outs = {}
    for tag, extra in (('plain', []), ('val', ['--val', str(tmp_path / 'val.json')])):
        os.makedirs(str(tmp_path / tag))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rc = train_frames.main([str(tmp_path / 'long*.npy'), '--meta', str(tmp_path / 'sensor.json'), '--camera', 'SonyA7S2', '--noise', 'PGRU',
                                    '--patch', '32', '--batch', '2', '--epochs', '1', '--steps', '2', '-o', str(tmp_path / tag / 'm.pt')] + extra)
        assert rc == 0
        outs[tag] = (buf.getvalue(), torch.load(str(tmp_path / tag / 'm.pt'), map_location='cpu'))
    assert 'val PSNR' not in outs['plain'][0]
    line = [ln for ln in outs['val'][0].splitlines() if 'val PSNR' in ln]
    assert len(line) == 1
    assert math.isfinite(float(line[0].split('val PSNR')[1].split()[0]))
    a, b = outs['plain'][1]['netG'], outs['val'][1]['netG']
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
