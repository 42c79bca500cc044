"""CPU tests of eld_amd.denoise: the write-back contract restated in NumPy and its measured truncation counts, the X-Trans binning order,
argument errors (raised before any device work), CLI / sidecar parsing and loading a reference-format checkpoint."""
import json
import types

import numpy as np
import pytest

import denoise_ref as R
from xtrans_ref import PLANE_COLOUR

PAIRS = [(512, 16383), (1024, 16383), (2048, 16383), (0, 65535)]


def roundtrip_losses(black, white, rounding):
    """codes in [black, white] that do not come back from a float32 pack + write-back; the count and the total"""
    u = np.arange(black, white + 1, dtype=np.int64).astype(np.uint16)
    x = np.clip((u.astype(np.float32) - np.float32(black)) / np.float32(white - black), np.float32(0), np.float32(1))
    return int((R.codes(x, black, white, rounding) != u).sum()), u.size


def test_write_back_restatement_is_the_reference_expression():
    """'trunc': postprocess_bayer (models/ELD_model.py:41-70) -- float32 clip, times an int64 (white - black) array (-> float64), plus
    black, assigned into a uint16 array (truncation); 'nearest': the same value rounded half to even; 'trunc_f32': postprocess_xtrans,
    whose Python-int constants leave the array float32."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.random(20000, dtype=np.float32), np.float32([-1, -0.0, 0, 1, 1.5, 3e38, -3e38])])
    black = np.array([512, 600, 1024, 2047])[:, None, None]
    img4c = np.clip(np.resize(x, (4, 5, x.size // 20)), 0, 1)
    ref = np.zeros(img4c.shape, np.uint16)
    ref[...] = img4c * (16383 - black) + black                      # the reference's two lines, as written
    for k in range(4):
        assert np.array_equal(R.codes(np.resize(x, (4, 5, x.size // 20))[k], int(black[k, 0, 0]), 16383, 'trunc'), ref[k])
    img9c = np.clip(x, 0, 1)
    ref9 = np.zeros(x.shape, np.uint16)
    ref9[...] = img9c * (16383 - 1024) + 1024
    assert (img9c * (16383 - 1024) + 1024).dtype == np.float32
    assert np.array_equal(R.codes(x, 1024, 16383, 'trunc_f32'), ref9)
    v = np.clip(x, 0, 1).astype(np.float64) * 15359 + 1024
    assert np.array_equal(R.codes(x, 1024, 16383, 'nearest'), np.rint(v).astype(np.uint16))
    assert R.codes(np.float32(0.5), 0, 3, 'nearest') == 2 and R.codes(np.float32(0.5), 0, 1, 'nearest') == 0      # ties to even


def test_float64_write_back_is_exact():
    """v = float64(x) * (w - b) + b has no rounding error: the product of a 24-bit mantissa and a <= 16-bit integer fits in 53 bits."""
    rng = np.random.default_rng(1)
    x = rng.random(100000, dtype=np.float32)
    from fractions import Fraction
    for b, w in PAIRS:
        v = x.astype(np.float64) * (w - b) + b
        for i in range(0, x.size, 9973):
            assert Fraction(float(v[i])) == Fraction(float(x[i])) * (w - b) + b


@pytest.mark.parametrize('black,white', PAIRS)
def test_truncation_counts_and_nearest_round_trip(black, white):
    """The measured fact of the docs: under truncation pack + write-back loses one DN on about half the codes; rounding to nearest
    round-trips every code in [black, white]; the reference's float32 X-Trans expression round-trips them too."""
    lost, total = roundtrip_losses(black, white, 'trunc')
    expected = {(512, 16383): (7893, 15872), (1024, 16383): (7676, 15360)}
    if (black, white) in expected:
        assert (lost, total) == expected[(black, white)]
    assert lost > total // 3
    assert roundtrip_losses(black, white, 'nearest')[0] == 0
    assert roundtrip_losses(black, white, 'trunc_f32')[0] == 0


def test_xtrans_binning_order():
    """R = (p0 + p3) / 2, G = ((((p1 + p5) + p6) + p7) + p8) / 5, B = (p2 + p4) / 2 in float32 -- the plane colours of xtrans_ref (the
    sampler's table).  The values are chosen so that another summation order gives other bits."""
    assert PLANE_COLOUR.tolist() == [0, 1, 2, 0, 2, 1, 1, 1, 1]
    f = np.float32
    x = np.zeros((1, 9, 1, 1), f)
    x[0, :, 0, 0] = [f(0.25), f(1), f(0.3), f(0.5), f(0.7), f(2 ** -24), f(2 ** -24), f(0), f(0)]      # G: 1 + 2^-24 rounds back to 1
    got = R.xtrans_binning(x)[0, :, 0, 0]
    p = x[0, :, 0, 0]
    assert got[0] == (p[0] + p[3]) / f(2)
    assert got[1] == ((((p[1] + p[5]) + p[6]) + p[7]) + p[8]) / f(5)
    assert got[2] == (p[2] + p[4]) / f(2)
    other = ((((p[8] + p[7]) + p[6]) + p[5]) + p[1]) / f(5)
    assert other != got[1]                     # the order matters for these values: the stated one is the one restated


def test_pack_and_gain_restatement():
    rng = np.random.default_rng(2)
    u = rng.integers(0, 16384, size=(2, 12, 18), dtype=np.uint16)
    p = R.pack_bayer(u, [[0, 1], [3, 2]], [512] * 4, 16383)
    assert p.shape == (2, 4, 6, 9) and p.dtype == np.float32
    assert p[0, 0, 1, 2] == np.clip((np.float32(u[0, 2, 4]) - 512) / np.float32(15871), 0, 1)
    g = R.gain(p, [1.0, 250.0])
    assert np.array_equal(g[0], p[0])
    assert np.array_equal(g[1], np.maximum(np.minimum(p[1] * np.float32(250.0), 1), 0))
    px = R.pack_xtrans(rng.integers(0, 16384, size=(1, 14, 20), dtype=np.uint16), 1024, 16383)
    assert px.shape == (1, 9, 4, 6)


# ---- arguments (no device work before the checks) --------------------------------------------------------------------------------
class FakeNet:
    def __init__(self, cin, cout):
        self.in_channels, self.out_channels = cin, cout


def fake(cfa, cin=None):
    from eld_amd.denoise import PLANES
    c = PLANES[cfa] if cin is None else cin
    return types.SimpleNamespace(cfa=cfa, in_channels=c, out_channels=c, net=FakeNet(c, c))


def frame(h=16, w=24, dtype=np.uint16):
    return np.full((h, w), 600, dtype)


@pytest.mark.parametrize('kw,msg', [
    (dict(mosaic=frame(15, 24)), 'even'),
    (dict(mosaic=frame(16, 23)), 'even'),
    (dict(mosaic=frame(4, 24), cfa='xtrans'), 'at least 6'),
    (dict(mosaic=frame(dtype=np.int32)), 'uint16'),
    (dict(mosaic=frame(dtype=np.float32)), 'uint16'),
    (dict(mosaic=[[1, 2], [3, 4]]), 'uint16'),
    (dict(mosaic=np.zeros((2, 2, 4, 4), np.uint16)), 'shape'),
    (dict(white_point=512), 'exceed'),
    (dict(white_point=500, black_level=[512, 400, 400, 400]), 'exceed'),
    (dict(white_point=70000), 'white_point'),
    (dict(ratio=0), 'ratio'),
    (dict(ratio=-3.0), 'ratio'),
    (dict(ratio=float('nan')), 'ratio'),
    (dict(ratio=[1.0, 2.0]), 'ratio'),
    (dict(net_planes=9), 'input planes'),
    (dict(cfa='xtrans', net_planes=4), 'input planes'),
    (dict(wb=[2.0, 1.0, 1.5]), 'both'),
    (dict(wb=[2.0, 1.0], ccm=np.eye(3)), 'wb'),
    (dict(wb=[2.0, 1.0, 1.5], ccm=np.eye(2)), 'ccm'),
    (dict(wb=[2.0, 1.0, 1.5], ccm=np.ones(8)), 'ccm'),
    (dict(raw_pattern=[[0, 1], [1, 2]]), 'raw_pattern'),
    (dict(black_level=[512, 512]), 'black_level'),
    (dict(cfa='xtrans', mosaic=frame(12, 12), black_level=[1024, 1000, 1024, 1024]), 'one black level'),
    (dict(rounding='floor'), 'rounding'),
    (dict(chop='yes'), 'chop'),
    (dict(cfa='quad'), 'cfa'),
])
def test_argument_errors(kw, msg):
    from eld_amd.denoise import denoise_raw
    kw = dict(kw)
    cfa = kw.pop('cfa', 'bayer')
    m = kw.pop('mosaic', frame())
    d = fake(cfa if cfa in ('bayer', 'xtrans') else 'bayer', kw.pop('net_planes', None))
    d.cfa = cfa
    with pytest.raises(ValueError, match=msg):
        denoise_raw(d, m, cfa, **kw)


def test_write_back_refuses_a_bad_pattern_before_any_launch(eld_lib):
    """eld_unpack_raw_bayer_u16 through the raw binding: a raw_pattern that is no permutation of 0..3 is ELD_EINVAL, decided on the host (the
    pointers are never dereferenced), even for an empty call; with a good pattern the empty call returns 0."""
    import ctypes
    p, blk = ctypes.c_void_p(0x10000), (ctypes.c_float * 4)(512, 512, 512, 512)
    for bad in ((ctypes.c_int * 4)(0, 1, 1, 2), (ctypes.c_int * 4)(0, 1, 4, 2), (ctypes.c_int * 4)(0, -1, 3, 2), None):
        for N in (1, 0):
            assert eld_lib.eld_unpack_raw_bayer_u16(p, p, N, 2, 4, bad, blk, 16383.0, 1, None) == -1
    assert eld_lib.eld_unpack_raw_bayer_u16(p, p, 0, 2, 4, (ctypes.c_int * 4)(0, 1, 3, 2), blk, 16383.0, 1, None) == 0


def test_wb_normalisation():
    from eld_amd.denoise import _colour
    w, m = _colour('bayer', [2000.0, 1000.0, 1500.0, 1000.0], np.eye(3), 2)        # rawpy camera_whitebalance: wb /= wb[1]
    assert w.shape == (2, 4) and w[0].tolist() == [2.0, 1.0, 1.5, 1.0] and m.shape == (2, 3, 3)
    w, _ = _colour('bayer', [2.0, 1.0, 1.5], np.eye(3).reshape(-1), 1)               # R, G, B -> R, G1, B, G2
    assert w[0].tolist() == [2.0, 1.0, 1.5, 1.0]
    w, _ = _colour('xtrans', [2000.0, 1000.0, 1500.0, 0.0], np.eye(3), 1)
    assert w[0].tolist() == [2.0, 1.0, 1.5]


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    from eld_amd.denoise import parse_args
    inputs, out, ckpt, o = parse_args(['--ckpt', 'm.pt', '--cfa', 'xtrans', '--black', '1024', '--white', '16383', '--ratio', '100',
                                       '--wb', '2', '1', '1.5', '--ccm', '1', '0', '0', '0', '1', '0', '0', '0', '1', '--bf16',
                                       'a.npy', 'b.npy', '-o', 'outdir'])
    assert inputs == ['a.npy', 'b.npy'] and out == 'outdir' and ckpt == 'm.pt'
    assert o['cfa'] == 'xtrans' and o['black_level'] == 1024.0 and o['white_point'] == 16383.0 and o['ratio'] == 100.0
    assert o['wb'] == [2.0, 1.0, 1.5] and o['ccm'] == np.eye(3).tolist() and o['precision'] == 'bf16'
    assert o['rounding'] == 'nearest' and o.get('chop') is None
    _, _, _, o = parse_args(['--ckpt', 'm.pt', 'a.npy', '-o', 'x', '--chop', 'on', '--rounding', 'reference', '--raw-pattern', '2', '3', '1', '0'])
    assert o['cfa'] == 'bayer' and o['chop'] is True and o['rounding'] == 'reference' and o['raw_pattern'] == [[2, 3], [1, 0]]
    assert o['precision'] == 'fp32' and o['ratio'] == 1.0 and o['white_point'] == 16383
    with pytest.raises(SystemExit):
        parse_args(['a.npy', '-o', 'x'])                                      # --ckpt is required
    with pytest.raises(ValueError, match='both'):
        parse_args(['--ckpt', 'm.pt', 'a.npy', '-o', 'x', '--wb', '2', '1', '1.5'])


def test_cli_sidecar(tmp_path):
    """The sidecar takes denoise_raw's keys or rawpy's names; a 4x3 / 3x4 rgb_camera_matrix is cut to [:3, :3]; the command line wins."""
    from eld_amd.denoise import parse_args
    cam = [[1.5, -0.3, -0.2, 0.0], [-0.1, 1.2, -0.1, 0.0], [0.0, -0.4, 1.4, 0.0]]
    meta = {'cfa': 'bayer', 'raw_pattern': [[2, 3], [1, 0]], 'black_level_per_channel': [512, 510, 512, 514], 'white_level': 16383,
            'camera_whitebalance': [2100.0, 1024.0, 1500.0, 1024.0], 'rgb_camera_matrix': cam, 'ratio': 50}
    p = tmp_path / 'frame.json'
    p.write_text(json.dumps(meta))
    _, _, _, o = parse_args(['--ckpt', 'm.pt', '--meta', str(p), 'f.npy', '-o', 'x'])
    assert o['raw_pattern'] == [[2, 3], [1, 0]] and o['black_level'] == [512, 510, 512, 514] and o['white_point'] == 16383
    assert o['wb'] == [2100.0, 1024.0, 1500.0, 1024.0] and o['ccm'] == np.asarray(cam)[:3, :3].tolist() and o['ratio'] == 50
    _, _, _, o = parse_args(['--ckpt', 'm.pt', '--meta', str(p), '--black', '500', '--ratio', '8', 'f.npy', '-o', 'x'])
    assert o['ratio'] == 8.0 and o['black_level'] == 500.0
    bad = tmp_path / 'bad.json'
    bad.write_text(json.dumps({'exposure': 3}))
    with pytest.raises(ValueError, match='unknown key'):
        parse_args(['--ckpt', 'm.pt', '--meta', str(bad), 'f.npy', '-o', 'x'])


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin', [4, 9])
def test_load_reference_checkpoint_dict(eld_lib, tmp_path, cin):
    """The reference's checkpoint dict (ELD_model.py:516-523: netG / opt_g / epoch / iterations), written with torch.save, loads by path, as
    a dict or as a bare state_dict -- same weights; the plane count and precision follow."""
    torch = pytest.importorskip('torch')
    from oracle import unet_ref as U
    from eld_amd.denoise import load_denoiser
    sd = U.seeded_state_dict(cin, cin, seed=7)
    ckpt = {'netG': sd, 'opt_g': {'state': {}, 'param_groups': []}, 'epoch': 3, 'iterations': 1200}
    path = tmp_path / 'model_latest.pt'
    torch.save(ckpt, str(path))
    cfa = 'bayer' if cin == 4 else 'xtrans'
    for src in (str(path), ckpt, sd):
        d = load_denoiser(src, cfa=cfa, precision='bf16', device='cpu')
        assert d.in_channels == cin and d.out_channels == cin and d.cfa == cfa and d.net.inference_precision == 'bf16'
        got = d.net.state_dict()
        assert sorted(got) == sorted(sd)
        for k in sd:
            assert torch.equal(got[k], sd[k]), k
    with pytest.raises(ValueError, match='U-Net checkpoint'):
        load_denoiser({'netG': {'w': torch.zeros(1)}}, device='cpu')
    with pytest.raises(ValueError, match='precision'):
        load_denoiser(ckpt, precision='fp16', device='cpu')
