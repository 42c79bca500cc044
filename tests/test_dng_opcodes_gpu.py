"""GPU tests of the DNG opcode kernels (csrc/dng_opcodes.hip through eld_amd.dng_opcodes) against the NumPy restatement
tests/dng_opcodes_ref.py, bit for bit on the float32 patterns, and of the opcode path through the command lines.

Shapes, the smallest at which the kernel can go wrong: 6 x 12 (one X-Trans cell row, less than a wave; a multiple of 4 wide: the float4
path), 34 x 46 (row and column tails, no multiple of any vector width), 258 x 1030 (crosses the 32 x 256 tile in both directions), and
40 x 1032 (the float4 path across tiles with a column tail).  N = 1 and 3.

NaN: a NaN site of the input frame passes through every operation unchanged (the kernels neither reject the frame nor clip the NaN away);
test_nan_sites_pass_through pins that."""
import functools
import json
import os

import numpy as np
import pytest

import dng_opcodes_cases as C
import dng_opcodes_ref as R
import dng_ref as DR
from guarded import Guards

pytestmark = pytest.mark.gpu

SHAPES = ((6, 12), (34, 46), (258, 1030), (40, 1032))
CM = ((8000, 10000), (-2000, 10000), (-500, 10000), (-3000, 10000), (11000, 10000), (2000, 10000), (-500, 10000), (1500, 10000), (6000, 10000))
VIG = [{'id': 3, 'flags': 0, 'k': (0.3, -0.1, 0.2, 0.05, -0.02), 'cx': 0.47, 'cy': 0.55}]


@pytest.fixture(scope='module')
def O(eld_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail('these tests need a GPU')
    from eld_amd import dng_opcodes
    return dng_opcodes


@functools.lru_cache(maxsize=None)
def program(name, Hm, Wm):
    if name in ('MapTable', 'MapPolynomial', 'GainMap', 'DeltaPerRow', 'DeltaPerColumn', 'ScalePerRow', 'ScalePerColumn'):
        return C.each_alone(Hm, Wm)[name]
    return {'phone': C.phone_program, 'small_maps': C.small_maps, 'odd_areas': C.odd_areas, 'chain32': C.chain32, 'big_maps': C.big_maps}[name](Hm, Wm)


@functools.lru_cache(maxsize=None)
def reference(name, Hm, Wm):
    """(input frames (3,Hm,Wm), the restatement's result), computed once and left unchanged"""
    x = C.frame(Hm, Wm, 5, N=3)
    y = R.apply_list2(x, program(name, Hm, Wm))
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def same_bits(t, want):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


APPLY = ('MapTable', 'MapPolynomial', 'GainMap', 'DeltaPerRow', 'DeltaPerColumn', 'ScalePerRow', 'ScalePerColumn', 'phone', 'small_maps', 'odd_areas',
         'chain32', 'big_maps')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', APPLY)
def test_apply_list2_matches_the_restatement(O, name, shape):
    import torch
    Hm, Wm = shape
    x, want = reference(name, Hm, Wm)
    if name in ('DeltaPerRow', 'DeltaPerColumn', 'chain32') and Hm >= 34:                        # both clips are reached
        assert (want == 0).sum() > (x == 0).sum() and (want == 1).sum() > (x == 1).sum()
    if name in ('GainMap', 'ScalePerRow', 'ScalePerColumn', 'phone') and Hm >= 34:
        assert (want == 1).sum() > (x == 1).sum()
    prog = O.OpcodeProgram(C.to_opcodes(program(name, Hm, Wm)), Hm, Wm)
    g = Guards()
    xin = g.ro(torch.from_numpy(x.copy()).cuda(), 'frames')
    out3, out1 = g.new((3, Hm, Wm), torch.float32, 'out N=3'), g.new((Hm, Wm), torch.float32, 'out N=1')
    assert O.apply_list2(xin, prog, out=out3) is out3
    O.apply_list2(xin[1], prog, out=out1)
    torch.cuda.synchronize()
    g.check()
    assert same_bits(out3, want), name
    assert same_bits(out1, want[1])
    inplace = g.new((3, Hm, Wm), torch.float32, 'in place', src=xin)
    O.apply_list2(inplace, prog, out=inplace)
    fresh = O.apply_list2(xin, prog)
    torch.cuda.synchronize()
    g.check()
    assert same_bits(inplace, want) and same_bits(fresh, want)


GAIN = {'phone': ('phone', ()), 'small_maps': ('small_maps', ()), 'odd_areas': ('odd_areas', ()), 'big_maps': ('big_maps', ()),
        'ScalePerRow': ('ScalePerRow', ()), 'ScalePerColumn': ('ScalePerColumn', ()), 'vignette': (None, VIG), 'phone+vignette': ('phone', VIG),
        'chain32': ('chain32', VIG), 'nothing': (None, ())}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('name', sorted(GAIN))
def test_gain_plane_matches_the_restatement(O, name, shape):
    import torch
    Hm, Wm = shape
    n2, specs3 = GAIN[name]
    specs2 = program(n2, Hm, Wm) if n2 else []
    want = R.gain_plane(specs2, specs3, Hm, Wm)
    g = Guards()
    out = g.new((Hm, Wm), torch.float32, 'gain plane')
    prog = O.gain_program(C.to_opcodes(specs2), C.to_opcodes(list(specs3)), Hm, Wm)
    O.gain_plane(prog, None, Hm, Wm, out=out)
    torch.cuda.synchronize()
    g.check()
    assert same_bits(out, want), name
    assert same_bits(O.gain_plane(C.to_opcodes(specs2), C.to_opcodes(list(specs3)), Hm, Wm, 'cuda'), want)
    if name == 'nothing':
        assert float(out.min()) == 1.0 == float(out.max())
    if name == 'phone':
        assert want.max() > 2.0                                      # several-fold in the corners, unclipped


@pytest.mark.parametrize('shape', SHAPES[1:], ids=lambda s: '%dx%d' % s)
def test_maps_in_lds_and_from_the_blob_give_the_same_bits(O, shape):
    """big_maps (two 48 KiB maps against the 32 KiB the kernels give to maps) reads from the blob by itself; here the phone program, which
    fits, is forced onto the same path, and a budget that takes the first of its maps only"""
    import torch
    Hm, Wm = shape
    x, want = reference('phone', Hm, Wm)
    prog = O.OpcodeProgram(C.to_opcodes(program('phone', Hm, Wm)), Hm, Wm)
    xin = torch.from_numpy(x.copy()).cuda()
    old = O.MAP_LDS_BYTES
    try:
        for budget in (0, 13 * 17 * 4, 64 << 10):
            O.MAP_LDS_BYTES = budget
            assert same_bits(O.apply_list2(xin, prog), want), budget
            assert same_bits(O.gain_plane(C.to_opcodes(program('phone', Hm, Wm)), [], Hm, Wm, 'cuda'), R.gain_plane(program('phone', Hm, Wm), [], Hm, Wm))
    finally:
        O.MAP_LDS_BYTES = old


def test_nan_sites_pass_through(O):
    import torch
    Hm, Wm = 34, 46
    x = C.frame(Hm, Wm, 9)
    x[0, 0] = x[17, 23] = x[33, 45] = np.nan
    for name in ('chain32', 'phone', 'MapTable'):
        want = R.apply_list2(x, program(name, Hm, Wm))
        out = O.apply_list2(torch.from_numpy(x).cuda(), O.OpcodeProgram(C.to_opcodes(program(name, Hm, Wm)), Hm, Wm))
        assert same_bits(out, want) and int(torch.isnan(out).sum()) == 3


def test_a_refused_record_is_einval_and_the_next_call_is_exact(O, eld_lib):
    import ctypes
    import torch
    from eld_amd import _lib as L
    Hm, Wm = 34, 46
    x, want = reference('chain32', Hm, Wm)
    prog = O.OpcodeProgram(C.to_opcodes(program('chain32', Hm, Wm)), Hm, Wm)
    xin = torch.from_numpy(x.copy()).cuda()
    g = Guards()
    out = g.new((3, Hm, Wm), torch.float32, 'out')
    blob = prog.blob_on(xin.device)

    def call(recs, nbytes, n=None):
        return eld_lib.eld_dng_opcodes_apply_f32(L.dptr(xin), L.dptr(out), 3, Hm, Wm, ctypes.c_void_p(recs.ctypes.data), len(recs) if n is None else n,
                                                 L.dptr(blob), nbytes, -1, L.cur_stream())
    for field, value in (('data_off', prog.blob.size), ('n0', 1 << 20), ('bottom', Hm + 1), ('row_pitch', 0), ('kind', 3), ('kind', 42), ('data_off', 2)):
        recs = prog.records.copy()
        i = 2 if field in ('data_off', 'n0') else 0                  # record 2 is the GainMap
        recs[field][i] = value
        assert call(recs, prog.blob.size) == -1, field
    assert call(prog.records, prog.blob.size - 8) == -1              # the last operation's parameters now end beyond the blob
    assert call(prog.records, prog.blob.size, 33) == -1
    assert eld_lib.eld_dng_opcodes_gain_f32(L.dptr(out), Hm, Wm, ctypes.c_void_p(prog.records.ctypes.data), len(prog), L.dptr(blob), prog.blob.size, -1,
                                            L.cur_stream()) == -1    # a chain with additive opcodes is no gain program
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                              # nothing was launched: the buffer is as the guard filled it
    with pytest.raises(L.EldError):
        L.check(call(prog.records, prog.blob.size, 33), 'eld_dng_opcodes_apply_f32')
    assert call(prog.records, prog.blob.size) == 0
    torch.cuda.synchronize()
    g.check()
    assert same_bits(out, want)
    with pytest.raises(ValueError):
        O.apply_list2(xin[:, :, :40], prog)
    with pytest.raises(ValueError):
        O.apply_list2(xin.double(), prog)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
AA = (2, 4, 50, 68)                                                  # the visible mosaic is 48 x 64 of a stored 52 x 70


@pytest.fixture(scope='module')
def dng_file(O, tmp_path_factory):
    d = tmp_path_factory.mktemp('opc')
    rng = np.random.default_rng(4)
    img = np.clip(rng.normal(900, 40, (52, 70)), 512, 4095).astype(np.uint16)
    img[10, 20] = img[31, 9] = img[40, 60] = 0                       # the codes FixBadPixelsConstant looks for
    img[12, 12] = img[25:27, 40:43] = 4000                            # hot: the point and the rectangle of FixBadPixelsList
    specs1 = [{'id': 5, 'flags': 0, 'bayer_phase': 0, 'points': [(12, 12), (1, 30)], 'rects': [(25, 40, 27, 43), (48, 66, 52, 70)]},
              {'id': 4, 'flags': 0, 'constant': 0, 'bayer_phase': 0}]
    specs2 = C.phone_program(48, 64) + [R.area_op(10, 0, 0, 48, 64, 1, 1, flags=1, values=np.full(48, 0.01, np.float32))]
    info = DR.write_dng_file(str(d / 'f.dng'), img, bits=12, compression=7, tile=(16, 32), ljpeg=dict(P=12, geometry='nf2'),
                             tags={50714: (DR.SHORT, (512,)), 50717: (DR.LONG, (4095,)), 50829: (DR.LONG, AA),
                                   51008: (DR.UNDEFINED, R.pack_list(specs1)), 51009: (DR.UNDEFINED, R.pack_list(specs2))},
                             tags0={50728: (DR.RATIONAL, ((1, 2), (1, 1), (2, 3))), 50721: (DR.SRATIONAL, CM), 50778: (DR.SHORT, (21,))})
    return {'dir': d, 'path': info['path'], 'visible': img[AA[0]:AA[2], AA[1]:AA[3]].copy(), 'specs1': specs1, 'specs2': specs2}


@pytest.fixture(scope='module')
def converted(O, dng_file, tmp_path_factory):
    """python -m eld_amd.dng --opcodes apply with both maps written, once for the tests below"""
    import eld_amd.dng as D
    d = dng_file['dir']
    out = {k: str(d / k) for k in ('frame.npy', 'lens.npz', 'defects.npz', 'stage2.npy')}
    assert D.main([dng_file['path'], '-o', out['frame.npy'], '--opcodes', 'apply', '--flatfield-out', out['lens.npz'], '--defects-out', out['defects.npz'],
                   '--linear-out', out['stage2.npy']]) == 0
    return out


def test_converter_applies_the_lists(O, dng_file, converted, capsys):
    import eld_amd.dng as D
    from eld_amd.defects import DefectMap, repair
    from eld_amd.flatfield import FlatField
    vis = dng_file['visible']
    plain, meta = D.read_dng(dng_file['path'])
    assert np.array_equal(plain, vis) and meta['opcodes'] == ['OpcodeList1', 'OpcodeList2']
    ff = FlatField.load(converted['lens.npz'])
    want = R.gain_plane(dng_file['specs2'], [], 48, 64)
    assert np.array_equal(ff.lens.view(np.uint32), want.view(np.uint32)) and np.all(ff.prnu == 1.0) and ff.radius == 0 and ff.frames == 0
    assert want.max() > 2.0 and ff.shape == (48, 64)
    dmap = DefectMap.load(converted['defects.npz'])
    sites = R.list1_sites(dng_file['specs1'], vis, AA)
    assert len(sites) == 1 + 6 + 4 + 3 and np.array_equal(dmap.sites, sites)
    assert np.array_equal(np.load(converted['frame.npy']), repair(plain, dmap))
    assert not np.array_equal(np.load(converted['frame.npy']), plain)
    lin = (repair(plain, dmap).astype(np.float32) - np.float32(512)) / np.float32(4095 - 512)
    stage2 = R.apply_list2(np.clip(lin, 0, 1).astype(np.float32), dng_file['specs2'])
    assert np.array_equal(np.load(converted['stage2.npy']).view(np.uint32), stage2.view(np.uint32))
    # the default still prints and does what it did
    capsys.readouterr()
    assert D.main([dng_file['path'], '-o', str(dng_file['dir'] / 'plain.npy')]) == 0
    text = capsys.readouterr().out
    assert 'OpcodeList1, OpcodeList2 present and not applied (gain maps, defect lists and warps stay with the raw converter)' in text
    assert np.array_equal(np.load(str(dng_file['dir'] / 'plain.npy')), plain)
    assert D.main([dng_file['path'], '-o', str(dng_file['dir'] / 'again.npy'), '--opcodes', 'apply']) == 0
    text = capsys.readouterr().out
    assert 'OpcodeList1[0] FixBadPixelsList: applied' in text and 'OpcodeList2[3] GainMap: folded into the lens plane' in text
    assert 'OpcodeList2[4] DeltaPerRow: skipped' not in text and 'OpcodeList2[4] DeltaPerRow: not applied' in text
    # a .dng output: list 1 is applied and gone, list 2 is still to do and travels with the repaired mosaic
    assert D.main([dng_file['path'], '-o', str(dng_file['dir'] / 'repaired.dng'), '--opcodes', 'apply']) == 0
    back, m = D.read_dng(str(dng_file['dir'] / 'repaired.dng'))
    assert np.array_equal(back, repair(plain, dmap)) and m['opcodes'] == ['OpcodeList2']
    assert O.read_opcodes(str(dng_file['dir'] / 'repaired.dng'))[1] == C.to_opcodes(dng_file['specs2'])


def test_denoise_command_line_applies_the_lists(O, dng_file, converted):
    """classical.main (no checkpoint) with --opcodes apply on the .dng against the .npy + sidecar run with the two written maps"""
    import eld_amd.dng as D
    from eld_amd import classical
    d = dng_file['dir']
    meta = D.dng_meta(dng_file['path'])
    np.save(str(d / 'g.npy'), dng_file['visible'])
    with open(str(d / 'g.json'), 'w') as fh:
        json.dump({k: meta[k] for k in ('cfa', 'raw_pattern', 'black_level', 'white_point', 'wb', 'ccm')}, fh)
    args = ['--method', 'nlm', '--K', '2.0', '--sigma', '3.0']
    runs = {'apply': [dng_file['path'], '--opcodes', 'apply', '--dng'],
            'maps': [str(d / 'g.npy'), '--meta', str(d / 'g.json'), '--flatfield', converted['lens.npz'], '--defects', converted['defects.npz']],
            'ignore': [dng_file['path'], '--opcodes', 'ignore', '--dng'],
            'all': [dng_file['path'], '--opcodes', 'apply', '--lens', 'all', '--dng']}
    outs = {}
    for name, argv in runs.items():
        out = str(d / ('out_' + name))
        assert classical.main(argv + ['-o', out] + args) == 0
        stem = 'g' if name == 'maps' else 'f'
        outs[name] = {k: np.load(os.path.join(out, '%s_%s.npy' % (stem, k))) for k in ('denoised', 'srgb')}
    for k in ('denoised', 'srgb'):
        assert np.array_equal(outs['apply'][k], outs['maps'][k]), k
        assert not np.array_equal(outs['apply'][k], outs['ignore'][k]), k
    with pytest.raises(ValueError, match='twice'):
        classical.main([dng_file['path'], '--opcodes', 'apply', '--flatfield', converted['lens.npz'], '-o', str(d / 'out_x')] + args)
    with pytest.raises(ValueError, match='.dng inputs'):
        classical.main([str(d / 'g.npy'), '--meta', str(d / 'g.json'), '--opcodes', 'apply', '-o', str(d / 'out_y')] + args)
    # --dng carries lists 2 and 3, never list 1
    source = O.read_opcodes(dng_file['path'])
    assert source[1] == C.to_opcodes(dng_file['specs2']) and len(source[0]) == 2
    srgb = O.read_opcodes(os.path.join(str(d / 'out_apply'), 'f_denoised.dng'))
    assert srgb[1] == source[1] and srgb[0] == [] and srgb[2] == []
    assert O.read_opcodes(os.path.join(str(d / 'out_ignore'), 'f_denoised.dng'))[1] == []       # without the option nothing is carried
    full = O.read_opcodes(os.path.join(str(d / 'out_all'), 'f_denoised.dng'))
    assert full[1] == [op for op in source[1] if op.id != 9] and len(full[1]) == 1 and full[0] == []
    assert not np.array_equal(outs['all']['denoised'], outs['apply']['denoised'])               # the gains are in the written mosaic
    assert np.array_equal(outs['all']['srgb'], outs['apply']['srgb'])
    back, _ = D.read_dng(os.path.join(str(d / 'out_all'), 'f_denoised.dng'))
    assert np.array_equal(back, outs['all']['denoised'])


def test_a_mandatory_opcode_in_front_of_the_network_is_refused(O, dng_file):
    from eld_amd import classical
    d = dng_file['dir']
    specs2 = [dict(dng_file['specs2'][-1], flags=0)]
    info = DR.write_dng_file(str(d / 'm.dng'), np.full((48, 64), 900, np.uint16), bits=12,
                             tags={50714: (DR.SHORT, (512,)), 50717: (DR.LONG, (4095,)), 51009: (DR.UNDEFINED, R.pack_list(specs2))})
    with pytest.raises(ValueError, match='DeltaPerRow'):
        classical.main([info['path'], '--opcodes', 'apply', '-o', str(d / 'out_m'), '--method', 'nlm', '--K', '2.0', '--sigma', '3.0'])
