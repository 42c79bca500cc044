"""CPU tests of the DNG opcode lists (eld_amd/dng_opcodes.py, csrc/dng_opcodes_dev.h): the parser and writer, every rejection, the NumPy
restatement (tests/dng_opcodes_ref.py) against hand-computed and independent values, the per-site evaluator under AddressSanitizer
(tools/dng_opcodes_hostcheck.cpp, a plain executable) and the list-1 geometry.  No device is touched."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import dng_opcodes_cases as C
import dng_opcodes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def O():
    from eld_amd import dng_opcodes
    return dng_opcodes


def every_type():
    return [{'id': 3, 'flags': 1, 'k': (0.1, -0.2, 0.3, 0.0, 0.05), 'cx': 0.5, 'cy': 0.48},
            {'id': 4, 'flags': 0, 'constant': 0, 'bayer_phase': 1},
            {'id': 5, 'flags': 0, 'bayer_phase': 2, 'points': [(3, 4), (70000, 5)], 'rects': [(1, 2, 3, 4)]},
            {'id': 1, 'flags': 1, 'data': bytes(range(20))},
            {'id': 6, 'flags': 0, 'data': struct.pack('>4I', 0, 0, 10, 12)},
            {'id': 99, 'flags': 1, 'data': b'abc'}] + [s for v in C.each_alone(12, 18).values() for s in v] + C.phone_program(12, 18, points=(2, 3))


# ---- parser and writer -----------------------------------------------------------------------------------------------------------------
def test_round_trip_of_every_opcode_type():
    o = O()
    specs = every_type()
    data = R.pack_list(specs)
    ops = o.parse_opcode_list(data, 'list')
    assert [op.id for op in ops] == [s['id'] for s in specs]
    assert o.pack_opcode_list(ops) == data                           # the package's writer against the restatement's
    assert o.parse_opcode_list(o.pack_opcode_list(ops), 'list') == ops
    assert ops == C.to_opcodes(specs)
    assert ops[0].optional and not ops[1].optional and ops[0].name == 'FixVignetteRadial' and ops[5].name == 'opcode 99'
    g = [op for op in ops if op.id == 9][0]
    assert g.f['gains'].shape == (5, 7, 1) and g.f['gains'].dtype == np.float32 and g.f['spacing_h'] == 1.0 / 6
    assert [op for op in ops if op.id == 5][0].f['points'].tolist() == [[3, 4], [70000, 5]]


def test_empty_list():
    o = O()
    assert o.parse_opcode_list(bytes(8), 'OpcodeList2') == []        # what the converter test of the reader uses
    assert o.parse_opcode_list(bytes(4), 'x') == [] and o.pack_opcode_list([]) == bytes(4)
    assert o.parse_opcode_list(bytes(4) + b'garbage behind a count of 0', 'x') == []


def _list(id_, params, flags=0, count=1):
    return struct.pack('>I', count) + struct.pack('>4I', id_, 0x01030000, flags, len(params)) + params


AREA = struct.pack('>8I', 0, 0, 8, 8, 0, 1, 2, 1)
GM_HEAD = AREA + struct.pack('>II', 2, 3) + struct.pack('>4d', 1.0, 0.5, 0.0, 0.0) + struct.pack('>I', 1)
MALFORMED = {
    'shorter than the count': (b'\0\0', 'shorter'),
    'shorter than a header': (struct.pack('>I', 1) + bytes(10), 'opcode 0'),
    'second header cut': (_list(6, bytes(16), count=2), 'opcode 1'),
    'byte count beyond the blob': (struct.pack('>I', 1) + struct.pack('>4I', 9, 0, 0, 400) + bytes(40), 'byte count'),
    'GainMap float count': (_list(9, GM_HEAD + bytes(4 * 5)), 'gains'),
    'Count != rows': (_list(10, AREA + struct.pack('>I', 3) + bytes(12)), 'Count'),
    'Count != columns': (_list(13, AREA + struct.pack('>I', 4) + bytes(16)), 'Count'),
    'Degree 9': (_list(8, AREA + struct.pack('>I', 9) + bytes(80)), 'Degree'),
    'TableSize 0': (_list(7, AREA + struct.pack('>I', 0)), 'TableSize'),
    'TableSize 65537': (_list(7, AREA + struct.pack('>I', 65537) + bytes(2 * 65537)), 'TableSize'),
    'row pitch 0': (_list(12, struct.pack('>8I', 0, 0, 8, 8, 0, 1, 0, 1) + struct.pack('>I', 0)), 'RowPitch'),
    'column pitch 0': (_list(9, struct.pack('>8I', 0, 0, 8, 8, 0, 1, 1, 0) + GM_HEAD[32:] + bytes(24)), 'ColPitch'),
    'area cut': (_list(11, AREA[:20]), 'area'),
    'vignette size': (_list(3, bytes(48)), 'parameters'),
    'bad pixel list counts': (_list(5, struct.pack('>III', 0, 2, 1) + bytes(16)), 'BadPointCount'),
    'GainMap of no points': (_list(9, AREA + struct.pack('>II', 0, 3) + bytes(32) + struct.pack('>I', 1)), 'MapPoints'),
}


@pytest.mark.parametrize('case', sorted(MALFORMED))
def test_malformed_lists_name_the_opcode(case):
    data, word = MALFORMED[case]
    with pytest.raises(ValueError) as e:
        O().parse_opcode_list(data, 'OpcodeList2')
    assert 'OpcodeList2' in str(e.value) and word in str(e.value), str(e.value)
    if case != 'shorter than the count':
        assert 'opcode ' in str(e.value)


def test_well_formed_neighbours_of_the_malformed_cases_parse():
    o = O()
    ops = o.parse_opcode_list(_list(9, GM_HEAD + bytes(4 * 6)) , 'x')
    assert ops[0].f['gains'].shape == (2, 3, 1)
    assert len(o.parse_opcode_list(_list(10, AREA + struct.pack('>I', 4) + bytes(16)), 'x')[0].f['values']) == 4      # ceil(8 / 2) rows
    assert len(o.parse_opcode_list(_list(13, AREA + struct.pack('>I', 8) + bytes(32)), 'x')[0].f['values']) == 8
    assert len(o.parse_opcode_list(_list(8, AREA + struct.pack('>I', 8) + bytes(72)), 'x')[0].f['coefficients']) == 9


def test_unknown_ids_follow_the_optional_bit_on_apply_only():
    o = O()
    data = R.pack_list([{'id': 99, 'flags': 1, 'data': b'x' * 7}, C.each_alone(8, 8)['ScalePerRow'][0], {'id': 1, 'flags': 0, 'data': b''}])
    ops = o.parse_opcode_list(data, 'OpcodeList2')                   # parsing and reporting: no error
    prog = o.OpcodeProgram(ops, 8, 8)
    assert len(prog) == 1 and [op.id for op in prog.skipped] == [99, 1] and o.disposition(ops[2], 2) == 'never'
    bad = o.parse_opcode_list(R.pack_list([{'id': 99, 'flags': 0, 'data': b''}]), 'OpcodeList2')
    with pytest.raises(ValueError, match='99'):
        o.OpcodeProgram(bad, 8, 8)
    with pytest.raises(ValueError, match='FixBadPixelsList'):        # a list-1 opcode in list 2, mandatory
        o.OpcodeProgram(C.to_opcodes([{'id': 5, 'flags': 0, 'bayer_phase': 0, 'points': [], 'rects': []}]), 8, 8)
    with pytest.raises(ValueError, match='GainMap'):                 # a mosaic opcode in list 3, mandatory
        o.gain_program([], C.to_opcodes(C.small_maps(8, 8)[:1]), 8, 8)
    assert len(o.gain_program([], C.to_opcodes([dict(C.small_maps(8, 8)[0], flags=1)]), 8, 8)) == 0
    with pytest.raises(ValueError, match='FixBadPixelsConstant'):    # with a LinearizationTable the stored codes are gone
        o.defects_from_opcodes(C.to_opcodes([{'id': 4, 'flags': 0, 'constant': 0, 'bayer_phase': 0}]), np.zeros((8, 8), np.uint16), {}, linearization=True)


def test_program_records():
    o = O()
    specs = C.odd_areas(34, 46) + C.each_alone(34, 46)['MapPolynomial']
    prog = o.OpcodeProgram(C.to_opcodes(specs), 34, 46)
    assert [int(k) for k in prog.records['kind']] == [12, 9, 8]       # the empty area, the other plane and the area outside are dropped
    assert [int(prog.records[n][0]) for n in ('top', 'left', 'bottom', 'right')] == [17, 0, 34, 46]
    assert int(prog.records['n0'][0]) == 57 and all(int(v) % 8 == 0 for v in prog.records['data_off']) and prog.blob.size % 8 == 0
    co = prog.blob[int(prog.records['data_off'][2]):][:16].view('<f4')
    assert co.tolist() == [float(np.float32(v)) for v in (-0.05, 0.7, 1.9, -1.3)]
    with pytest.raises(ValueError, match='at most 32'):
        o.OpcodeProgram(C.to_opcodes(C.chain32(12, 18) + C.small_maps(12, 18)[:1]), 12, 18)
    with pytest.raises(ValueError, match='at most'):
        o.OpcodeProgram(C.to_opcodes([R.gm(0, 0, 8, 8, np.ones((4096, 4096), np.float32))] * 2), 8, 8)


# ---- the restatement against hand-computed and independent values ---------------------------------------------------------------------------
def test_two_by_two_map_by_hand():
    """[[1, 2], [3, 4]], origin 0, spacing 1 on 4 x 4: v = (y + 0.5) / 4, so i0 = 0 and the weights are 1/8, 3/8, 5/8, 7/8: all dyadic, every
    operation exact, gain = 1 + wx + 2 wy."""
    s = R.gm(0, 0, 4, 4, [[1, 2], [3, 4]])
    want = np.array([[1.375, 1.625, 1.875, 2.125],
                     [1.875, 2.125, 2.375, 2.625],
                     [2.375, 2.625, 2.875, 3.125],
                     [2.875, 3.125, 3.375, 3.625]], np.float32)
    assert np.array_equal(R.map_gain(s, 4, 4), want)
    assert np.array_equal(R.gain_plane([s], [], 4, 4), want)
    v = np.full((4, 4), 0.25, np.float32)
    assert np.array_equal(R.apply_list2(v, [s]), want * np.float32(0.25))


def test_constant_map_doubles_and_clips():
    s = R.gm(0, 0, 5, 7, np.full((3, 4), 2.0, np.float32), spacing=(0.5, 1.0 / 3))
    v = np.linspace(0, 1, 35, dtype=np.float32).reshape(5, 7)
    out = R.apply_list2(v, [s])
    assert np.array_equal(out, np.minimum(v * np.float32(2), np.float32(1))) and out.max() == 1.0 and (out == 1.0).sum() > 10


def test_gain_map_against_scipy():
    """13 x 17 random map over 34 x 46 against scipy's order-1 interpolation in float64 at the same coordinates.  The float32 restatement does
    at most 12 rounded operations per site on values bounded by max|map|, each off by at most 2^-24 relative: |diff| <= 12 * 2^-24 * max|map|
    < 2^-19 * max|map| (a derived cap, not a measured one)."""
    from scipy.ndimage import map_coordinates
    rng = np.random.default_rng(7)
    g = rng.uniform(0.5, 4.0, (13, 17)).astype(np.float32)
    Hm, Wm = 34, 46
    s = R.gm(0, 0, Hm, Wm, g, spacing=(1.0 / 12, 1.0 / 16))
    vy = np.clip(((np.arange(Hm) + 0.5) / Hm) * 12, 0, 12)
    vx = np.clip(((np.arange(Wm) + 0.5) / Wm) * 16, 0, 16)
    yy, xx = np.meshgrid(vy, vx, indexing='ij')
    want = map_coordinates(g.astype(np.float64), [yy, xx], order=1, mode='nearest')
    got = R.map_gain(s, Hm, Wm)
    diff = np.abs(got.astype(np.float64) - want).max()
    print('max |restatement - scipy| = %.3e, cap %.3e' % (diff, 2.0 ** -19 * float(np.abs(g).max())))
    assert diff <= 2.0 ** -19 * float(np.abs(g).max())


def test_table_polynomial_and_vectors_by_hand():
    v = np.array([[0.0, 0.5, 1.0, 0.25]], np.float32)
    tab = np.array([0, 65535, 30000], np.uint16)                     # indices beyond the table use its last entry
    out = R.apply_list2(v, [R.area_op(7, 0, 0, 1, 4, table=tab)])
    q = np.float32(30000) / np.float32(65535)                        # indices 0, 32768, 65535, 16384 -> entries 0, 2, 2, 2
    assert np.array_equal(out, np.array([[0.0, q, q, q]], np.float32))
    # rint ties to even: 0.5 * 65535 = 32767.5 -> 32768
    ramp = np.arange(65536, dtype=np.uint16)
    assert R.apply_list2(np.array([[0.5]], np.float32), [R.area_op(7, 0, 0, 1, 1, table=ramp)])[0, 0] == np.float32(32768) / np.float32(65535)
    out = R.apply_list2(v, [R.area_op(8, 0, 0, 1, 4, coefficients=[0.25, 0.5, 1.0])])             # 0.25 + 0.5 v + v^2, exact here
    assert out.tolist() == [[0.25, 0.75, 1.0, 0.4375]]
    out = R.apply_list2(np.full((4, 3), 0.5, np.float32), [R.area_op(10, 1, 0, 4, 3, 2, 1, values=[0.25, -1.0]),
                                                             R.area_op(13, 0, 1, 4, 3, 1, 1, values=[3.0, 0.5])])
    assert out.tolist() == [[0.5, 1.0, 0.25], [0.75, 1.0, 0.375], [0.5, 1.0, 0.25], [0.0, 0.0, 0.0]]
    nan = np.array([[np.nan, 0.5]], np.float32)
    out = R.apply_list2(nan, [R.area_op(12, 0, 0, 1, 2, values=[2.0])])
    assert np.isnan(out[0, 0]) and out[0, 1] == 1.0


def test_vignette_by_hand():
    """centre in the middle of 2 x 2: every pixel centre is half a pixel from it in both directions, the corner a whole one: r2 = 1/4"""
    s = {'id': 3, 'flags': 0, 'k': (1.0, 4.0, 0.0, 0.0, 0.0), 'cx': 0.5, 'cy': 0.5}
    assert np.array_equal(R.vignette(s, 2, 2), np.full((2, 2), 1.0 + 0.25 * (1.0 + 0.25 * 4.0), np.float32))
    assert np.array_equal(R.gain_plane([], [s], 2, 2), R.vignette(s, 2, 2))


# ---- the evaluator under AddressSanitizer ----------------------------------------------------------------------------------------------
def hostcheck_case(specs, Hm, Wm, gain_mode, specs3=(), seed=0):
    o = O()
    if gain_mode:
        prog = o.gain_program(C.to_opcodes(specs), C.to_opcodes(specs3), Hm, Wm)
        img = np.ones((Hm, Wm), np.float32)
        want = R.gain_plane(specs, specs3, Hm, Wm)
    else:
        prog = o.OpcodeProgram(C.to_opcodes(specs), Hm, Wm)
        img = C.frame(Hm, Wm, seed)
        img[1, 1] = np.nan
        want = R.apply_list2(img, specs)
    ys, xs = np.mgrid[0:Hm, 0:Wm]
    sites = np.zeros(Hm * Wm, np.dtype([('y', '<i4'), ('x', '<i4'), ('in', '<f4'), ('want', '<f4')]))
    sites['y'], sites['x'], sites['in'], sites['want'] = ys.reshape(-1), xs.reshape(-1), img.reshape(-1), want.reshape(-1)
    return (struct.pack('<6I', Hm, Wm, len(prog), prog.blob.size, int(gain_mode), len(sites)) + prog.records.tobytes() + prog.blob.tobytes() +
            sites.tobytes())


def test_evaluator_under_address_sanitizer(tmp_path):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path / 'dng_opcodes_hostcheck')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                           os.path.join(ROOT, 'tools', 'dng_opcodes_hostcheck.cpp')])
    Hm, Wm = 12, 18
    vig = [{'id': 3, 'flags': 0, 'k': (0.3, -0.1, 0.2, 0.05, -0.02), 'cx': 0.47, 'cy': 0.55}]
    cases = [hostcheck_case(C.chain32(Hm, Wm), Hm, Wm, False),
             hostcheck_case(C.phone_program(Hm, Wm, points=(4, 5)) + C.odd_areas(Hm, Wm), Hm, Wm, False, seed=1),
             hostcheck_case(C.small_maps(Hm, Wm) + [s for v in C.each_alone(Hm, Wm).values() for s in v], Hm, Wm, False, seed=2),
             hostcheck_case(C.phone_program(Hm, Wm, points=(4, 5)) + C.small_maps(Hm, Wm) + C.each_alone(Hm, Wm)['ScalePerColumn'] +
                            C.each_alone(Hm, Wm)['ScalePerRow'] + C.each_alone(Hm, Wm)['DeltaPerRow'], Hm, Wm, True, vig)]
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<I', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and 'hostcheck OK' in r.stdout, r.stdout
    assert '4000 single-field corruptions' in r.stdout


# ---- geometry of list 1 -------------------------------------------------------------------------------------------------------------------
def test_list1_coordinates_with_an_active_area():
    """ActiveArea (2, 4, 14, 20) of a 16 x 24 stored image: the visible mosaic is 12 x 16.  Points inside, on the border rows and outside; a
    rectangle that the active area cuts on two sides."""
    o = O()
    aa = (2, 4, 14, 20)
    spec = {'id': 5, 'flags': 0, 'bayer_phase': 0, 'points': [(2, 4), (13, 19), (1, 10), (14, 10), (7, 3), (7, 20), (8, 9)],
            'rects': [(0, 0, 4, 6), (12, 17, 16, 24), (6, 12, 7, 13)]}
    codes = np.full((12, 16), 700, np.uint16)
    codes[5, 5] = codes[10, 2] = 0
    specs = [spec, {'id': 4, 'flags': 0, 'constant': 0, 'bayer_phase': 0}]
    meta = {'active_area': list(aa), 'cfa': 'bayer', 'raw_pattern': [[0, 1], [3, 2]]}
    dmap = o.defects_from_opcodes(o.parse_opcode_list(R.pack_list(specs), 'OpcodeList1'), codes, meta)
    want = sorted([(0, 0), (11, 15), (6, 5),                          # the three points inside, moved by (-2, -4)
                   (0, 1), (1, 0), (1, 1),                            # rows 2..3, columns 4..5 of the first rectangle
                   (10, 13), (10, 14), (10, 15), (11, 13), (11, 14),  # rows 12..13, columns 17..19 of the second
                   (4, 8), (5, 5), (10, 2)])                          # the 1 x 1 rectangle and the two codes equal to Constant
    assert [tuple(s) for s in dmap.sites.tolist()] == want
    assert [tuple(s) for s in R.list1_sites(specs, codes, aa).tolist()] == want
    assert dmap.shape == (12, 16) and dmap.cfa == 'bayer'
    # DefectMap's own refusal comes through: a whole bad column strands its sites
    col = {'id': 5, 'flags': 0, 'bayer_phase': 0, 'points': [], 'rects': [(0, 8, 16, 13)]}
    with pytest.raises(ValueError, match='no unflagged neighbour'):
        o.defects_from_opcodes(C.to_opcodes([col]), codes, meta)
    assert o.defects_from_opcodes([], codes, meta).count == 0
