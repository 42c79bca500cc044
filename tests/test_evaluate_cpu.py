"""eld_amd.evaluate without a device: the bin function's NumPy restatement (tests/pairstats_ref.py) against its definition, level_curves on
hand-made sums, the ratio of a pair, manifest parsing and precedence, every ValueError of evaluate_pairs / pair_level_stats (all raised
before any device work) and the --val wiring of eld_amd.train_frames."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import pairstats_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the bin function ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('black,white', [(512, 16383), (0, 65536), (1024, 16383), (2048, 4095), (65535, 65536)])
def test_bin_restatement_exhaustive(black, white):
    ref = np.arange(65536)
    b = R.bin_index(ref, black, white)
    assert np.array_equal(b, [R.bin_loop(int(r), black, white) for r in ref])          # floor(log2) against the counting loop
    assert b.min() >= 0 and b.max() <= R.NB - 1
    assert np.array_equal(b == R.NB - 1, ref >= white)                                  # the saturated bin: ref >= white and nothing else
    below = b[ref < white]
    assert np.all(np.diff(below) >= 0)                                                  # monotone in s
    assert np.all(below[ref[ref < white] <= black] == 0)
    if white > black + 1:
        assert below[black + 1] == 1


def test_bin_count_and_edges():
    from eld_amd import evaluate as E
    s = np.arange(1, 65536)
    b = R.bin_index(s, 0, 65536)
    assert E.NB == R.NB == 61
    assert len(np.unique(b)) == 59 and b.max() == 59                                    # bins 1..59; bin 0 holds s <= 0, bin 60 the saturated sites
    edges = E.bin_lower_edges()
    first = np.array([s[b == k].min() for k in range(1, 60)])
    assert np.array_equal(edges[1:60], first) and edges[0] == 0 and edges[60] == -1
    for o in range(3, 16):                                                              # quarter octaves: four bins per octave, equal widths
        k = 8 + 4 * (o - 3)
        assert np.array_equal(np.diff(np.append(edges[k:k + 4], 2 << o)), [1 << (o - 2)] * 4)


def test_ref_sums_by_hand():
    est = np.array([[[10, 20], [30, 40]]], np.uint16)
    ref = np.array([[[12, 20], [20, 300]]], np.uint16)
    out = R.pair_level_sums(est, ref, 2, [0, 1, 1, 0], 2, [10, 10, 10, 10], 256)
    assert out.shape == (1, 2, 61, 4)
    assert out[0, 0, 2].tolist() == [1, 2, -2, 4]                                       # (0,0): s = 2, e = -2
    assert out[0, 0, 60].tolist() == [1, 290, -260, 67600]                              # (1,1): saturated
    assert out[0, 1, R.bin_loop(20, 10, 256)].tolist() == [2, 20, 10, 100]              # (0,1) e = 0 and (1,0) e = 10, both s = 10
    assert int(out[..., 0].sum()) == 4


# ---- level_curves -------------------------------------------------------------------------------------------------------------------------
def test_level_curves_by_hand():
    import warnings
    from eld_amd.evaluate import level_curves
    s = np.zeros((2, 3, 61, 4), np.int64)
    s[0, 1, 3] = [4, 12, -8, 20]
    s[0, 1, 9] = [6, 66, 3, 30]
    s[0, 1, 60] = [2, 5, 100, 5000]                                                     # saturated: not in mse / psnr
    s[1, 2, 0] = [5, -10, 0, 0]
    with warnings.catch_warnings():
        warnings.simplefilter('error')                                                  # no division warning on the empty bins
        c = level_curves(s, span=[1000.0, 100.0, 10.0])
    assert c['n'].dtype == np.int64 and c['n'][0, 1, 3] == 4
    assert c['signal'][0, 1, 3] == 3.0 and c['bias'][0, 1, 3] == -2.0 and c['rmse'][0, 1, 3] == np.sqrt(5.0)
    assert c['bias'][0, 1, 60] == 50.0 and c['signal'][1, 2, 0] == -2.0 and c['rmse'][1, 2, 0] == 0.0
    empty = c['n'] == 0
    assert np.all(np.isnan(c['bias'][empty])) and np.all(np.isnan(c['rmse'][empty])) and np.all(np.isnan(c['signal'][empty]))
    assert not np.any(np.isnan(c['bias'][~empty]))
    assert c['mse_codes'][0, 1] == 50.0 / 10.0
    assert c['psnr_codes'][0, 1] == 10.0 * np.log10(100.0 * 100.0 / 5.0)
    assert np.isinf(c['psnr_codes'][1, 2]) and np.isnan(c['psnr_codes'][0, 0]) and np.isnan(c['mse_codes'][1, 0])
    assert np.all(np.isnan(level_curves(s)['psnr_codes']))                              # no span: no PSNR
    pooled = level_curves(s.sum(axis=0))
    assert pooled['n'].shape == (3, 61) and pooled['bias'][1, 3] == -2.0
    big = np.zeros((1, 61, 4), np.int64)
    big[0, 0] = [2 ** 31 - 1, 0, 0, (2 ** 31 - 1) * 65535 ** 2]                         # beyond 2^53: still the exact quotient
    assert level_curves(big)['mse_codes'][0] == 65535.0 ** 2
    for bad in (np.zeros((61, 4), np.int64), np.zeros((1, 60, 4), np.int64), np.zeros((1, 61, 4))):
        with pytest.raises(ValueError):
            level_curves(bad)
    with pytest.raises(ValueError):
        level_curves(s, span=0)


# ---- pairs, ratios, tables ----------------------------------------------------------------------------------------------------------------
def test_pair_ratio():
    from eld_amd.evaluate import pair_ratio
    assert pair_ratio({'ratio': 100}) == 100.0
    assert pair_ratio({'iso': 1600, 'exposure': 0.1, 'long_iso': 100, 'long_exposure': 10}) == 100 * 10 / (1600 * 0.1)
    assert pair_ratio({'ratio': 250, 'iso': 1600}) == 250.0                             # an explicit ratio wins; iso then only groups the table
    for bad in ({}, {'iso': 100, 'exposure': 1, 'long_iso': 100}, {'ratio': 0}, {'ratio': -1}, {'ratio': float('nan')}, {'ratio': float('inf')},
                {'iso': 0, 'exposure': 1, 'long_iso': 1, 'long_exposure': 1}, {'iso': 1, 'exposure': 1, 'long_iso': 0, 'long_exposure': 1}):
        with pytest.raises(ValueError):
            pair_ratio(bad)


def test_table_groups_and_averages():
    from eld_amd.evaluate import table_by_iso_ratio, table_lines
    rows = [dict(iso=800.0, ratio=100.0, psnr=40.0, ssim=0.9, psnr_in=20.0, ssim_in=0.1),
            dict(iso=800.0, ratio=100.0, psnr=42.0, ssim=0.8, psnr_in=22.0, ssim_in=0.3),
            dict(iso=None, ratio=100.0, psnr=1.0, ssim=0.5, psnr_in=2.0, ssim_in=0.25),
            dict(iso=800.0, ratio=300.0, psnr=30.0, ssim=0.7, psnr_in=10.0, ssim_in=0.05),
            dict(iso=100.0, ratio=300.0, psnr=35.0, ssim=0.6, psnr_in=15.0, ssim_in=0.15)]
    t = table_by_iso_ratio(rows)
    assert [(r['iso'], r['ratio'], r['count']) for r in t] == [(100.0, 300.0, 1), (800.0, 100.0, 2), (800.0, 300.0, 1), (None, 100.0, 1)]
    assert t[1]['psnr'] == 41.0 and t[1]['ssim'] == np.mean([0.9, 0.8]) and t[1]['psnr_in'] == 21.0 and t[1]['ssim_in'] == np.mean([0.1, 0.3])
    assert len(table_lines(t)) == 5


# ---- the manifest -------------------------------------------------------------------------------------------------------------------------
def _manifest(tmp_path, extra=None, pairs=None, name='pairs.json'):
    d = {'cfa': 'bayer', 'black_level_per_channel': [512, 512, 512, 512], 'white_level': 16383, 'raw_pattern': [[0, 1], [3, 2]]}
    d.update(extra or {})
    d['pairs'] = pairs if pairs is not None else [{'short': 'a.npy', 'long': 'sub/b.npy', 'ratio': 100, 'iso': 1600},
                                                  {'short': 'c.npy', 'long': 'sub/b.npy', 'iso': 800, 'exposure': 0.04, 'long_iso': 100, 'long_exposure': 32}]
    p = tmp_path / name
    p.write_text(json.dumps(d))
    return str(p)


def test_manifest_parsing(tmp_path):
    from eld_amd.evaluate import load_pairs, read_manifest
    opts, pairs = read_manifest(_manifest(tmp_path))
    assert opts == {'cfa': 'bayer', 'black_level': [512, 512, 512, 512], 'white_point': 16383, 'raw_pattern': [[0, 1], [3, 2]]}    # rawpy's names
    assert pairs[0]['short'] == str(tmp_path / 'a.npy') and pairs[0]['long'] == str(tmp_path / 'sub' / 'b.npy')                  # relative to it
    assert pairs[0]['name'] == 'a' and pairs[0]['ratio'] == 100 and pairs[1]['name'] == 'c' and 'ratio' not in pairs[1]
    with pytest.raises(ValueError, match='no such file'):
        load_pairs(pairs)
    (tmp_path / 'sub').mkdir()
    for n in ('a.npy', 'c.npy', 'sub/b.npy'):
        np.save(str(tmp_path / n), np.full((4, 6), 7, np.uint16))
    loaded = load_pairs(pairs)
    assert loaded[1]['long'].shape == (4, 6) and loaded[1]['iso'] == 800 and isinstance(pairs[1]['long'], str)
    for extra, prs in (({'ratio': 100}, None), ({'iso': 100}, None), ({'colour': 1}, None), ({}, []), ({}, [{'short': 'a.npy', 'ratio': 1}]),
                       ({}, [{'short': 'a.npy', 'long': 'b.npy'}]), ({}, [{'short': 'a.npy', 'long': 'b.npy', 'ratio': 0}]),
                       ({}, [{'short': 'a.npy', 'long': 'b.npy', 'ratio': 1, 'gain': 2}]), ({}, ['a.npy'])):
        with pytest.raises(ValueError):
            read_manifest(_manifest(tmp_path, extra, prs, 'bad.json'))
    (tmp_path / 'list.json').write_text('[1, 2]')
    for path in (str(tmp_path / 'list.json'), str(tmp_path / 'missing.json')):
        with pytest.raises(ValueError):
            read_manifest(path)


def test_command_line_precedence(tmp_path):
    from eld_amd.evaluate import parse_args
    man = _manifest(tmp_path, {'defects': 'm.npz', 'wb': [2, 1, 1.5], 'ccm': [[1, 0, 0], [0, 1, 0], [0, 0, 1]]})
    side = tmp_path / 'sensor.json'
    side.write_text(json.dumps({'black': 256, 'white': 4095, 'ratio': 3, 'rounding': 'nearest'}))
    a, o, pairs = parse_args([man, '--ckpt', 'net.pt'])
    assert o['black_level'] == [512, 512, 512, 512] and o['white_point'] == 16383 and o['precision'] == 'fp32' and o['cfa'] == 'bayer'
    assert o['defects'] == str(tmp_path / 'm.npz') and a.crop is None and not a.no_correct and len(pairs) == 2
    a, o, _ = parse_args([man, '--ckpt', 'net.pt', '--meta', str(side), '--bf16', '--defects', 'other.npz', '--crop', '512', '--no-correct', '--save',
                          str(tmp_path / 'png')])
    assert o['black_level'] == 256 and o['white_point'] == 4095                       # --meta over the manifest
    assert 'ratio' not in o and 'rounding' not in o                                     # a sidecar's ratio is not a pair's
    assert o['defects'] == 'other.npz' and o['precision'] == 'bf16' and a.crop == 512 and a.no_correct   # the command line over both
    with pytest.raises(ValueError, match='wb and ccm'):
        parse_args([_manifest(tmp_path, name='plain.json'), '--ckpt', 'net.pt', '--save', str(tmp_path / 'png')])
    with pytest.raises(ValueError, match='iso'):
        parse_args([_manifest(tmp_path, pairs=[{'short': 'a.npy', 'long': 'b.npy', 'ratio': 2}], name='noiso.json'), '--ckpt', 'n.pt', '--shading', 's.npz'])


# ---- argument errors, all on the host -----------------------------------------------------------------------------------------------------
class _Params:
    """A network stand-in whose parameters must never be looked at: the checks come first."""
    def parameters(self):
        raise AssertionError('device work before the argument checks')


def _denoiser(cfa='bayer', planes=4):
    return types.SimpleNamespace(cfa=cfa, in_channels=planes, out_channels=planes, net=_Params())


def test_evaluate_pairs_refuses_on_the_host():
    from eld_amd.evaluate import evaluate_pairs
    m = np.zeros((32, 32), np.uint16)
    ok = {'short': m, 'long': m, 'ratio': 100.0}
    bad = [
        (dict(pairs=[]), 'non-empty'),
        (dict(pairs=[{'short': m, 'ratio': 1}]), "'short' and 'long'"),
        (dict(pairs=[{'short': m, 'long': np.zeros((32, 34), np.uint16), 'ratio': 1}]), 'short is 32 x 32, long 32 x 34'),
        (dict(pairs=[{'short': m, 'long': m}]), "needs 'ratio'"),
        (dict(pairs=[{'short': m, 'long': m, 'ratio': 0}]), 'ratio must be finite and > 0'),
        (dict(pairs=[{'short': m, 'long': m, 'ratio': -2}]), 'ratio must be finite and > 0'),
        (dict(pairs=[{'short': m.astype(np.float32), 'long': m, 'ratio': 1}]), 'uint16'),
        (dict(pairs=[{'short': m[None], 'long': m[None], 'ratio': 1}]), 'one \\(Hm, Wm\\) mosaic'),
        (dict(pairs=[{'short': m[:31], 'long': m[:31], 'ratio': 1}]), 'even'),
        (dict(pairs=[dict(ok, iso=-1)]), 'iso must be'),
        (dict(cfa='foveon'), 'cfa must be'),
        (dict(cfa='xtrans'), 'loaded for'),
        (dict(chop='yes'), 'chop must be'),
        (dict(crop=0), 'crop must be'),
        (dict(crop=1.5), 'crop must be'),
        (dict(crop=17), 'exceeds the packed frame'),
        (dict(white_point=0), 'white_point'),
        (dict(black_level=[1, 2, 3]), 'black_level'),
        (dict(raw_pattern=[[0, 1], [1, 2]]), 'raw_pattern'),
        (dict(defects=3), 'defects'),
        (dict(defects='/nonexistent/map.npz'), 'no such'),
        (dict(shading=3), 'shading'),
    ]
    for kw, msg in bad:
        kw = dict(dict(pairs=[ok], cfa='bayer'), **kw)
        with pytest.raises(ValueError, match=msg):
            evaluate_pairs(_denoiser(), kw.pop('pairs'), kw.pop('cfa'), **kw)
    with pytest.raises(ValueError, match='planes'):
        evaluate_pairs(_denoiser(planes=9), [ok], 'bayer')
    with pytest.raises(ValueError, match='X-Trans crop must be even'):
        evaluate_pairs(_denoiser('xtrans', 9), [ok], 'xtrans', crop=3)


def test_shading_needs_iso_on_the_host():
    from eld_amd.evaluate import evaluate_pairs
    from eld_amd.shading import DarkShading
    m = np.zeros((32, 32), np.uint16)
    sh = DarkShading.__new__(DarkShading)                       # the iso check comes before the map is looked at
    with pytest.raises(ValueError, match='shading needs iso'):
        evaluate_pairs(_denoiser(), [{'short': m, 'long': m, 'ratio': 10.0}], 'bayer', shading=sh)


def test_pair_level_stats_refuses_on_the_host():
    from eld_amd.evaluate import pair_level_stats
    a = np.zeros((4, 6), np.uint16)
    for args, msg in (((a, np.zeros((4, 8), np.uint16), 'bayer', None, 512, 16383), 'shape'),
                      ((a.astype(np.int32), a, 'bayer', None, 512, 16383), 'uint16'),
                      ((a, a, 'bayer', None, 512, 70000), 'white_point'),
                      ((a, a, 'bayer', None, [512, 512], 16383), 'black_level'),
                      ((a, a, 'bayer', None, -1, 16383), 'black_level'),
                      ((a, a, 'bayer', [0, 1, 1, 2], 512, 16383), 'raw_pattern'),
                      ((a, a, 'bogus', None, 512, 16383), 'cfa'),
                      ((a, a, 'bayer', None, 512, 16383, 7), 'defects')):
        with pytest.raises(ValueError, match=msg):
            pair_level_stats(*args)


# ---- train_frames --val -------------------------------------------------------------------------------------------------------------------
def test_train_frames_val_wiring(tmp_path):
    from eld_amd import train_frames as T
    a = T.build_parser().parse_args(['x.npy', '-o', 'out.pt'])
    assert a.val is None and T.val_pairs(None) is None          # opt-in: nothing happens without the flag
    a = T.build_parser().parse_args(['x.npy', '-o', 'out.pt', '--val', 'pairs.json'])
    assert a.val == 'pairs.json'
    with pytest.raises(ValueError, match='no such manifest'):   # refused before any frame is read (x.npy does not exist either)
        T.main([str(tmp_path / 'x.npy'), '-o', str(tmp_path / 'out.pt'), '--val', str(tmp_path / 'missing.json')])
    man = _manifest(tmp_path)
    with pytest.raises(ValueError, match='no such file'):
        T.main([str(tmp_path / 'x.npy'), '-o', str(tmp_path / 'out.pt'), '--val', man])


def test_module_imports_without_the_library(tmp_path):
    code = ('import eld_amd._lib as L\nimport eld_amd.evaluate as E\nassert L._lib is None\n'
            'assert E.NB == 61 and E.level_curves is not None and E.build_parser() is not None\nprint("ok")')
    env = dict(os.environ, ELD_AMD_LIB=str(tmp_path / 'absent.so'), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr
