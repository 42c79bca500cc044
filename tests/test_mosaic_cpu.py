"""CPU tests of eld_amd/mosaic.py: CfaLayout against tables written out by hand, the tiling and whole-cell helpers, the checks the
saved maps share, and one rejected input for each rule set a layout is built under (no device work anywhere)."""
import os

import numpy as np
import pytest

from eld_amd import mosaic as M
from eld_amd import validate as V

RGGB = [[0, 1], [3, 2]]
GBRG = [[3, 2], [0, 1]]
# the cell the library packs, colours R 0 / G 1 / B 2 (row 0 = R B G B R G)
XCELL = [[0, 2, 1, 2, 0, 1],
         [1, 1, 0, 1, 1, 2],
         [1, 1, 2, 1, 1, 0],
         [2, 0, 1, 0, 2, 1],
         [1, 1, 2, 1, 1, 0],
         [1, 1, 0, 1, 1, 2]]
XT_PLANE_COLOUR = (0, 1, 2, 0, 2, 1, 1, 1, 1)


def test_bayer_layouts_by_hand():
    lay = M.CfaLayout('bayer', RGGB, [510, 512, 514, 516])
    assert (lay.cfa, lay.period, lay.G) == ('bayer', 2, 4)
    assert lay.codes.dtype == np.int64 and lay.codes.tolist() == [[0, 1], [3, 2]]
    assert lay.colour.tolist() == [[0, 1], [1, 2]]
    assert list(lay.group) == [0, 1, 3, 2]
    assert lay.black_cells.tolist() == [[510.0, 512.0], [516.0, 514.0]]
    assert lay.black_ints == [510, 512, 516, 514]
    assert lay.centres.tolist() == [[510, 512], [516, 514]]
    assert list(lay.c_group()) == [0, 1, 3, 2] and list(lay.c_black()) == [510, 512, 516, 514]
    lay = M.CfaLayout('bayer', GBRG, [510, 512, 514, 516])
    assert lay.codes.tolist() == [[3, 2], [0, 1]] and lay.colour.tolist() == [[1, 2], [0, 1]]
    assert list(lay.group) == [3, 2, 0, 1] and lay.G == 4
    assert lay.black_ints == [516, 514, 510, 512]
    assert lay.group_table.tolist() == [[3, 2], [0, 1]]


def test_xtrans_layout_is_the_cell_of_the_golden_pack(golden_dir, eld_lib):
    z = np.load(os.path.join(golden_dir, 'rawpacker_xtrans.npz'))
    mosaic, packed = z['exact_mosaic'], z['exact_packed']           # plane k of the pack holds four sites of every 6x6 cell
    cell = np.full((6, 6), -1)
    for k in range(9):
        for v in packed[k, :2, :2].reshape(-1):
            (y,), (x,) = np.nonzero(mosaic[:6, :6] == v)
            cell[y, x] = XT_PLANE_COLOUR[k]
    assert cell.tolist() == XCELL
    assert M.xtrans_tables()['colour'].tolist() == XCELL
    lay = M.CfaLayout('xtrans', XCELL, [1022, 1024, 1026, 1024])
    assert (lay.period, lay.G) == (6, 3)
    assert np.bincount(lay.colour.reshape(-1)).tolist() == [8, 20, 8]
    assert list(lay.group) == [c for row in XCELL for c in row]
    assert lay.black_ints == [(1022, 1024, 1026)[c] for row in XCELL for c in row]
    assert lay.black_cells.tolist() == [[(1022.0, 1024.0, 1026.0)[c] for c in row] for row in XCELL]
    coded = np.array(XCELL)
    coded[1, 1] = coded[4, 4] = 3                                     # two greens under rawpy's second green code
    lay3 = M.CfaLayout('xtrans', coded, [1022, 1024, 1026, 1030])
    assert lay3.colour.tolist() == XCELL and list(lay3.group) == list(lay.group)
    assert lay3.black_cells[1, 1] == 1030.0 and lay3.black_cells[1, 0] == 1024.0
    for build in (M.CfaLayout.for_codes, M.CfaLayout.for_map):      # a missing pattern is the library's cell, a missing black level 1024
        d = build('xtrans')
        assert d.codes.tolist() == XCELL and d.black.tolist() == [1024.0] * 4
    d = M.CfaLayout.for_codes('bayer')
    assert d.codes.tolist() == RGGB and d.black_ints == [512] * 4


def test_layout_is_immutable():
    lay = M.CfaLayout('bayer', RGGB, [510, 512, 514, 516])
    with pytest.raises(AttributeError):
        lay.period = 6
    with pytest.raises(ValueError):
        lay.codes[0, 0] = 2
    black = np.array([510.0, 512.0, 514.0, 516.0])
    lay = M.CfaLayout('bayer', RGGB, black)
    black[0] = 0.0                                                    # the caller's array is not the layout's
    assert lay.black[0] == 510.0


def test_tile_and_whole_cells():
    lay = M.CfaLayout('xtrans', XCELL)
    vals = np.arange(36) * 3 + 1
    got = lay.tile(vals, 7, 8)
    want = np.zeros((7, 8), vals.dtype)
    for y in range(7):
        for x in range(8):
            want[y, x] = vals[(y % 6) * 6 + x % 6]
    assert got.shape == (7, 8) and np.array_equal(got, want)
    b = M.CfaLayout('bayer', GBRG)
    got = b.tile(b.group, 7, 8)
    assert all(got[y, x] == GBRG[y % 2][x % 2] for y in range(7) for x in range(8))
    assert np.array_equal(M.tile_cells(np.array(GBRG), 7, 8), got)
    assert lay.whole_cells(13, 20) == (12, 18)
    assert b.whole_cells(13, 20) == (13, 20)


def test_public_delegates_return_the_layout():
    from eld_amd import flatfield as FF
    from eld_amd import structure as ST
    assert V.group_map_u16('bayer', GBRG) == (2, [3, 2, 0, 1], 4)
    assert V.group_map_u16('xtrans', XCELL) == (6, [c for row in XCELL for c in row], 3)
    assert ST.cell_centres('bayer', RGGB, [510.4, 512.5, 513.5, 70000]).tolist() == [[510, 512], [65535, 514]]     # rounds half to even, clips
    assert np.array_equal(FF.cell_map(np.array(RGGB), 5, 3), M.tile_cells(np.array(RGGB), 5, 3))
    assert FF.check_white(65535) == 65535 and M.check_white(65536) == 65536


def test_each_rule_set_still_rejects():
    with pytest.raises(ValueError):
        M.black_levels([1, 2, 3])                                      # calibrate: exactly 4 values
    with pytest.raises(ValueError):
        M.CfaLayout('bayer', RGGB, 512)                                # the strict constructor: no scalar black level
    with pytest.raises(ValueError):
        M.CfaLayout('bayer', RGGB, None)                               # ... and None is not "no black level"
    with pytest.raises(ValueError):
        M.CfaLayout('bayer', None)                                     # ... and no default pattern
    with pytest.raises(ValueError):
        M.CfaLayout('bayer', [[0, 1], [1, 2]])
    with pytest.raises(ValueError):
        M.CfaLayout('xtrans', np.where(np.arange(36).reshape(6, 6) == 0, 1, np.array(XCELL)))       # 7 R, 21 G, 8 B
    with pytest.raises(ValueError):
        M.CfaLayout('foveon', RGGB)
    with pytest.raises(ValueError):
        M.CfaLayout.for_codes('bayer', RGGB, [64.5] * 4)               # evaluate, burst, noiselevel: integers
    with pytest.raises(ValueError):
        M.CfaLayout.for_codes('bayer', RGGB, [1, 2, 3])
    with pytest.raises(ValueError):
        M.CfaLayout.for_codes('bayer', RGGB, 70000)
    assert M.CfaLayout.for_map('bayer', RGGB, [64.5] * 4).black.tolist() == [64.5] * 4            # shading, flatfield: finite values
    with pytest.raises(ValueError):
        M.CfaLayout.for_map('bayer', RGGB, -1)
    with pytest.raises(ValueError):
        M.CfaLayout.for_map('bayer', RGGB, [np.nan] * 4)
    with pytest.raises(ValueError):
        M.CfaLayout.for_map('xtrans', np.roll(np.array(XCELL), 1, axis=0))                          # not the cell the library packs
    assert M.CfaLayout.for_codes('xtrans', np.roll(np.array(XCELL), 1, axis=0)).period == 6        # evaluate takes any phase
    with pytest.raises(ValueError):
        V.group_black('xtrans', [1022, 1024, 1026, 1030])              # validate: one centre for both green codes
    assert V.group_black('xtrans', [1022, 1024.4, 1026, 1023.6]).tolist() == [1022, 1024, 1026]
    with pytest.raises(ValueError):
        M.levels('xtrans', None, [510, 512, 514, 512], 16383)          # the input stage: one X-Trans black level
    with pytest.raises(ValueError):
        M.levels('bayer', None, 512, 512)                              # ... and white > black
    with pytest.raises(ValueError):
        M.check_white(65536, 65535, 'white_level')
    for w in (0, 100.5, 65537):
        with pytest.raises(ValueError):
            M.check_white(w)


def test_stack_checks():
    u = np.zeros((3, 12, 12), np.uint16)
    assert M.check_stack(u, 'frames') == (3, 12, 12) and M.check_stack(u[0], 'frames', limit=True) == (1, 12, 12)
    with pytest.raises(ValueError, match='frames: '):
        M.check_stack(u.astype(np.int32), 'frames')
    with pytest.raises(ValueError):
        M.check_stack(np.zeros((2, 2, 4, 6), np.uint16), 'frames')
    assert M.check_mosaics(np.zeros((3, 12, 14), np.uint16), 3, 'frames', None) == (3, 12, 14)
    assert M.check_mosaics(np.zeros((3, 5, 14), np.uint16), 3, 'frames', None) == (3, 5, 14)      # the histogram rule: any height
    with pytest.raises(ValueError):
        M.check_mosaics(np.zeros((3, 12, 13), np.uint16), 3, 'frames', None)
    with pytest.raises(ValueError):
        M.check_mosaics(np.zeros((3, 5, 14), np.uint16), 3, 'frames', 'bayer')
    with pytest.raises(ValueError):
        M.check_mosaics(np.zeros((3, 4, 8), np.uint16), 3, 'frames', 'xtrans')
    with pytest.raises(ValueError, match='2\\^31'):
        M.check_site_count(1 << 16, 1 << 15)


def test_map_checks_name_their_map():
    class Map(M.FittedMap):
        NOUN = 'flat-field map'
        cfa, shape, raw_pattern = 'bayer', (12, 14), np.array(RGGB)

    m = Map()
    assert m.period == 2
    m.check_frames((3, 12, 14), 'bayer')
    m.check_pattern(None)
    m.check_pattern(RGGB)
    with pytest.raises(ValueError, match='w: the flat-field map is for cfa='):
        m.check_frames((12, 14), 'xtrans', 'w')
    with pytest.raises(ValueError, match='the flat-field map is for 12 x 14 mosaics, got 12 x 16'):
        m.check_frames((12, 16), 'bayer')
    with pytest.raises(ValueError, match='the flat-field map was fitted under raw_pattern'):
        m.check_pattern(GBRG)
