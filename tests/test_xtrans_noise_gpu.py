"""GPU tests of the X-Trans row noise and colour bias (ELD_CFA_XTRANS) of the fused sampler: dumped variates replay bit for bit through
the oracle's arithmetic with the X-Trans plane bias, the row normal follows the mosaic's rows and Philox's (sensor row, STREAM_ROW)
words, the output is self-deterministic over batching and the vector / scalar paths, and the colour bias lands per CFA colour."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import noise_ref as O          # noqa: E402
from oracle import philox_ref as px        # noqa: E402
from xtrans_ref import plane_bias, sensor_rows  # noqa: E402

XT = 512
FULL = O.SHOT_POISSON | O.READ_TL | O.ROW | O.QUANT
CB3 = (1.5, -1.0, 0.25)


@pytest.fixture(scope='module')
def dev(eld_lib):
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def params(N, cb=CB3):
    from eld_amd.noise import NoiseParams
    return [NoiseParams(0.4 + i, 3.0 + i, 15583, 100.0 + 90 * i, tl_lambda=[-0.14285714, 0.0, 0.114285715][i % 3], tl_scale=2.5 + i,
                        row_scale=0.7 + i, color_bias=tuple(cb) + (7.0,)) for i in range(N)]      # [3] is ignored on X-Trans


def oparams(p):
    return O.Params(K=p[0], g_scale=p[1], saturation=p[2], ratio=p[3], tl_lambda=p.tl_lambda, tl_scale=p.tl_scale,
                    row_scale=p.row_scale, q_step=p.q_step, color_bias=plane_bias(p.color_bias[:3]))


def run(y, plist, flags, ids, dump=False, yt=None, seed=2018):
    from eld_amd import _lib as L
    from eld_amd.noise import sample_noise
    if yt is None:
        yt = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    numel = int(np.prod(y.shape))
    dmp = torch.full((L.NPLANES, numel), float('nan'), dtype=torch.float32, device='cuda') if dump else None
    z = sample_noise(yt, plist, flags, seed, ids, dump=dmp).cpu().numpy()
    if dump:
        d = dmp.cpu().numpy()
        return z, {k: d[i].reshape(y.shape) for k, i in L.PLANE.items()}
    return z


def synth(rng, shape):
    return (np.floor(65535 * rng.random(shape, dtype=np.float32) ** 2.2) / 65535).astype(np.float32)


SHAPES = [(2, 9, 16, 24), (1, 9, 7, 13), (2, 9, 11, 20), (1, 9, 10, 6), (1, 9, 600, 4), (1, 9, 400, 6)]
# even / odd h and w; w % 4 == 0 (16-byte path) and not; the last two overflow MAX_LDS_ROWS per block (1024 packed rows, 683 rows)


@pytest.mark.parametrize('flags', [FULL | XT, FULL | XT | O.CLIP, FULL | O.CBIAS | XT, FULL | O.CBIAS | XT | O.CLIP])
@pytest.mark.parametrize('shape', SHAPES)
def test_row_map_replay_bit_exact(dev, flags, shape):
    from eld_amd.noise import RawPacker
    N, _, h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    y = synth(rng, shape)
    plist = params(N)
    ids = [40 + 7 * i for i in range(N)]
    z, v = run(y, plist, flags, ids, dump=True)
    assert np.array_equal(z, run(y, plist, flags, ids))              # the production kernel (specialised for 'PGRU') gives the same bits
    rows = sensor_rows(h, w)
    for i in range(N):
        zi = O.noise_arith(y[i], oparams(plist[i]), flags & ~XT, **{k: a[i] for k, a in v.items()})
        assert np.array_equal(z[i], zi)
        mos = RawPacker('xtrans').unpack_raw_xtrans(torch.from_numpy(v['n_row'][i]).cuda()).cpu().numpy()
        assert mos.shape == (3 * h, 3 * w)
        assert np.array_equal(mos, np.broadcast_to(mos[:, :1], mos.shape))      # one normal per mosaic row
        wd = px.sampler_words(np.arange(3 * h, dtype=np.uint32), ids[i], px.STREAM_ROW, 2018)
        nrm = px.box_muller(wd[0], wd[1])[0]
        assert np.max(np.abs(mos[:, 0] - nrm)) < 1e-4                        # Box-Muller of Philox (s, STREAM_ROW)
        assert np.max(np.abs(v['n_row'][i] - nrm[rows])) < 1e-4


@pytest.mark.parametrize('flags', [FULL | XT, FULL | O.CBIAS | XT | O.CLIP])
def test_self_determinism_batch_and_paths(dev, flags):
    shape = (3, 9, 34, 48)
    rng = np.random.default_rng(11)
    y = synth(rng, shape)
    plist = params(3)
    ids = [5, 900, (3 << 32) | 17]
    zb = run(y, plist, flags, ids)
    for i in range(3):
        assert np.array_equal(run(y[i:i + 1], plist[i:i + 1], flags, ids[i:i + 1])[0], zb[i])
    # an offset view: the input is not 16-byte aligned, the scalar kernel runs
    buf = torch.zeros(y.size + 1, dtype=torch.float32, device='cuda')
    buf[1:] = torch.from_numpy(y.reshape(-1)).cuda()
    view = buf[1:].view(shape)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    assert np.array_equal(run(y, plist, flags, ids, yt=view), zb)


@pytest.mark.parametrize('shape', [(2, 9, 8, 12), (1, 9, 5, 7)])
def test_colour_bias_alone(dev, shape):
    N = shape[0]
    y = np.zeros(shape, np.float32)
    plist = params(N, cb=(3.25, -0.5, 1.75))
    z = run(y, plist, O.CBIAS | XT, list(range(N)))
    for i in range(N):
        zi = O.noise_arith(y[i], oparams(plist[i]), O.CBIAS)
        assert np.array_equal(z[i], zi)
        for c, k in enumerate((0, 1, 2, 0, 2, 1, 1, 1, 1)):
            assert np.all(z[i, c] == z[i, c].flat[0]) and z[i, c].flat[0] == zi[c].flat[0]
            assert (z[i, c].flat[0] > 0) == (plist[i].color_bias[k] > 0)


def test_cfa_flag_without_row_or_bias_changes_nothing(dev):
    shape = (2, 9, 12, 20)
    y = synth(np.random.default_rng(3), shape)
    plist = params(2)
    for fl in (O.SHOT_POISSON | O.READ_GAUSS, O.READ_GAUSS | O.READ_TL | O.QUANT | O.CLIP, 0):
        assert np.array_equal(run(y, plist, fl | XT, [1, 2]), run(y, plist, fl, [1, 2]))
