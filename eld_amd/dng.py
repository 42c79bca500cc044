"""Read DNG raw files: the TIFF container and the metadata on the host, the pixels on the device (libeld_amd: eld_dng_unpack_u16 for
uncompressed packed rows, eld_dng_ljpeg_u16 for lossless JPEG).  Built from the specifications (TIFF 6.0, DNG 1.x,
ITU-T T.81): there is no rawpy here.

    read_dng(path, device=None) -> (mosaic, meta)   the visible mosaic as rawpy's raw_image_visible would give it
    dng_meta(path)                                  the tags only, in the sidecar's keys (eld_amd.denoise.SIDECAR_KEYS)
    load_frame(path)                                .npy -> np.load(path); .dng -> read_dng(path)[0]
    write_dng(path, mosaic, meta=None, like=None, opcodes=None)   an uncompressed 16-bit little-endian DNG, one IFD, strips; compression=7: lossless-JPEG
                                                    tiles, encoded on the device (eld_dng_enc_*)
                                                    preview=bytes: a baseline JPEG (eld_amd.jpeg) as IFD0, the mosaic in a SubIFD
    encode_ljpeg(mosaic, tile, bits)                the JPEG streams of the tiles alone, for callers with a container of their own
    python -m eld_amd.dng in.dng [-o frame.npy | -o out.dng [--compression ljpeg] [--tile TH TW] [--bits N] [--preview FILE.jpg]] [--meta-out sensor.json]
                          [--opcodes apply [--flatfield-out lens.npz] [--defects-out defects.npz] [--linear-out stage2.npy]]

Container.  Classic TIFF in both byte orders.  The raw image is the IFD with NewSubFileType = 0 and PhotometricInterpretation = 32803
(CFA), looked for in IFD0 and in its SubIFDs (tag 330); SamplesPerPixel = 1; strips or tiles; Compression 1 (8, 10, 12, 14 or 16 bits, rows
bit-packed MSB-first) or 7 (lossless JPEG).  Everything else is a ValueError that names the tag and the value: LinearRaw (34892), lossy
JPEG, JPEG XL, deflate, BigTIFF, FillOrder = 2, floating-point samples.  Every offset and count is checked against the file size before
anything is uploaded.

Metadata mapping (tag -> key):
    CFARepeatPatternDim   (2, 2) -> cfa 'bayer'; (6, 6) -> 'xtrans'; anything else is an error
    CFAPattern            colours 0 R, 1 G, 2 B -> rawpy codes in raw_pattern.  Bayer: the first green in raster order is 1, the second 3 (RGGB ->
                          ((0, 1), (3, 2)), the project's default); X-Trans: every green is 1.  The pattern is relative to the top-left
                          corner of ActiveArea.
    ActiveArea            (top, left, bottom, right): the mosaic is full[top:bottom, left:right].  DefaultCropOrigin / DefaultCropSize and
                          Orientation do not change the mosaic (rawpy's raw_image_visible ignores them too); dng_meta reports them as
                          default_crop (y0, x0, h, w) and orientation when the file carries them, write_dng(like=) copies them, and
                          eld_amd.denoise --crop default / --orient auto frame the rendered picture by them.
    BlackLevelRepeatDim,  black_level: four values indexed by rawpy code (Bayer), one value (X-Trans; unequal values are an error).  A
    BlackLevel            non-zero BlackLevelDeltaH / BlackLevelDeltaV is an error.
    WhiteLevel            white_point
    LinearizationTable    applied in the decode: v = table[min(v, len - 1)]
    AsShotNeutral         (n_R, n_G, n_B) -> wb = (n_G / n_R, 1, n_G / n_B); absent -> no wb
    ColorMatrix1/2        ccm: the matrix whose CalibrationIlluminant is 21 (D65), else ColorMatrix1; cam_from_rgb = ColorMatrix . M with M
                          the linear-sRGB -> XYZ (D65) matrix; each row divided by its sum; ccm = the inverse, in float64 (what rawpy
                          reports as rgb_camera_matrix[:3, :3] for a DNG).  AnalogBalance and CameraCalibration1/2 are ignored.
    ISOSpeedRatings,      iso, exposure_time: from the Exif IFD (tag 34665), or from IFD0 where they sit there
    ExposureTime
    Make, Model           make, model
    OpcodeList1/2/3       not applied by read_dng; the lists present are named in meta['opcodes'].  eld_amd.dng_opcodes parses them and turns
                          them into a DefectMap and a lens FlatField (--opcodes apply here and in eld_amd.denoise / eld_amd.classical)
and bits (BitsPerSample), compression, active_area.

Nothing touches a device before the arguments and the file have been validated."""
import argparse
import json
import os
import struct
import sys
from fractions import Fraction

import numpy as np

from . import _lib as L

# ---- TIFF -----------------------------------------------------------------------------------------------------------------------
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
TYPE_FMT = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 11: 'f', 12: 'd', 13: 'I'}
BYTE, ASCII, SHORT, LONG, RATIONAL, UNDEFINED, SRATIONAL = 1, 2, 3, 4, 5, 7, 10

T_NEWSUBFILETYPE, T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_FILLORDER = 254, 256, 257, 258, 259, 262, 266
T_MAKE, T_MODEL, T_STRIPOFFSETS, T_ORIENTATION, T_SPP, T_ROWSPERSTRIP, T_STRIPBYTECOUNTS = 271, 272, 273, 274, 277, 278, 279
T_TILEWIDTH, T_TILELENGTH, T_TILEOFFSETS, T_TILEBYTECOUNTS, T_SUBIFDS, T_SAMPLEFORMAT = 322, 323, 324, 325, 330, 339
T_YCBCRSUBSAMPLING, YCBCR_PHOTOMETRIC = 530, 6
T_CFADIM, T_CFAPATTERN, T_EXPOSURETIME, T_EXIFIFD, T_ISO = 33421, 33422, 33434, 34665, 34855
T_DNGVERSION, T_DNGBACKWARD, T_UNIQUEMODEL, T_CFAPLANECOLOR, T_CFALAYOUT, T_LINTABLE = 50706, 50707, 50708, 50710, 50711, 50712
T_BLACKDIM, T_BLACK, T_BLACKDH, T_BLACKDV, T_WHITE = 50713, 50714, 50715, 50716, 50717
T_COLORMATRIX1, T_COLORMATRIX2, T_ANALOGBALANCE, T_ASSHOTNEUTRAL, T_ILLUMINANT1, T_ILLUMINANT2 = 50721, 50722, 50727, 50728, 50778, 50779
T_ACTIVEAREA, T_OPCODE1, T_OPCODE2, T_OPCODE3 = 50829, 51008, 51009, 51022
T_DEFAULTCROPORIGIN, T_DEFAULTCROPSIZE = 50719, 50720
OPCODE_TAGS = ((T_OPCODE1, 'OpcodeList1'), (T_OPCODE2, 'OpcodeList2'), (T_OPCODE3, 'OpcodeList3'))
CFA_PHOTOMETRIC, LINEARRAW_PHOTOMETRIC = 32803, 34892
COMPRESSION_NAMES = {6: 'old-style JPEG', 8: 'deflate', 32946: 'deflate', 34892: 'lossy JPEG', 52546: 'JPEG XL'}
UNPACK_BITS = (8, 10, 12, 14, 16)
D65 = 21
# linear sRGB -> XYZ (D65)
SRGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=np.float64)
PAD = 8                                  # bytes kept behind the last stream in the uploaded range


class Entry:
    """One IFD entry: tag, TIFF type, count, and the values (rationals as (numerator, denominator) pairs, ASCII as a str)."""
    __slots__ = ('tag', 'type', 'count', 'values')

    def __init__(self, tag, type_, count, values):
        self.tag, self.type, self.count, self.values = tag, type_, count, values


class Tiff:
    """The parsed container: byte order, file size, IFD0 and its SubIFDs and Exif IFD (each a dict tag -> Entry)."""
    def __init__(self, path, order, size, ifd0, subifds, exif):
        self.path, self.order, self.size, self.ifd0, self.subifds, self.exif = path, order, size, ifd0, subifds, exif


def _read_ifd(buf, off, bo, path, what):
    n_file = len(buf)
    if off < 8 or off + 2 > n_file:
        raise ValueError('%s: %s at offset %d lies outside the file (%d bytes)' % (path, what, off, n_file))
    n, = struct.unpack_from(bo + 'H', buf, off)
    if off + 2 + 12 * n + 4 > n_file:
        raise ValueError('%s: %s at offset %d with %d entries runs beyond the file (%d bytes)' % (path, what, off, n, n_file))
    ifd = {}
    for i in range(n):
        tag, typ, cnt = struct.unpack_from(bo + 'HHI', buf, off + 2 + 12 * i)
        if typ not in TYPE_SIZE:
            continue                                                # a type from a later specification: readers skip the field (TIFF 6.0, p. 16)
        nbytes = TYPE_SIZE[typ] * cnt
        pos = off + 2 + 12 * i + 8
        if nbytes > 4:
            pos, = struct.unpack_from(bo + 'I', buf, pos)
            if pos + nbytes > n_file:
                raise ValueError('%s: tag %d of %s: %d bytes at offset %d run beyond the file (%d bytes)' % (path, tag, what, nbytes, pos, n_file))
        if typ == ASCII:
            vals = bytes(buf[pos:pos + cnt]).split(b'\0')[0].decode('latin-1')
        elif typ in (RATIONAL, SRATIONAL):
            flat = struct.unpack_from(bo + ('%dI' if typ == RATIONAL else '%di') % (2 * cnt), buf, pos)
            vals = tuple((flat[2 * k], flat[2 * k + 1]) for k in range(cnt))
        elif typ in (BYTE, UNDEFINED) and cnt > 64:
            vals = bytes(buf[pos:pos + cnt])                        # opcode lists and the like: kept as bytes
        elif typ in (SHORT, LONG) and cnt > 64:
            vals = np.frombuffer(buf, dtype=bo + ('u2' if typ == SHORT else 'u4'), count=cnt, offset=pos)
        else:
            vals = struct.unpack_from(bo + '%d%s' % (cnt, TYPE_FMT[typ]), buf, pos)
        ifd[tag] = Entry(tag, typ, cnt, vals)
    nxt, = struct.unpack_from(bo + 'I', buf, off + 2 + 12 * n)
    return ifd, nxt


def parse_tiff(path):
    """-> (Tiff, the file's bytes).  Classic TIFF, II or MM; BigTIFF is refused."""
    path = os.fspath(path)
    with open(path, 'rb') as fh:
        buf = fh.read()
    if len(buf) < 8 or buf[:2] not in (b'II', b'MM'):
        raise ValueError('%s: not a TIFF file (no II / MM byte-order mark)' % path)
    bo = '<' if buf[:2] == b'II' else '>'
    magic, off0 = struct.unpack_from(bo + 'HI', buf, 2)
    if magic == 43:
        raise ValueError('%s: BigTIFF (version 43) is not supported: classic TIFF only' % path)
    if magic != 42:
        raise ValueError('%s: not a TIFF file (version %d)' % (path, magic))
    ifd0, _ = _read_ifd(buf, off0, bo, path, 'IFD0')
    subs = []
    if T_SUBIFDS in ifd0:
        for k, o in enumerate(ifd0[T_SUBIFDS].values):
            subs.append(_read_ifd(buf, int(o), bo, path, 'SubIFD %d' % k)[0])
    exif = {}
    if T_EXIFIFD in ifd0:
        exif = _read_ifd(buf, int(ifd0[T_EXIFIFD].values[0]), bo, path, 'the Exif IFD')[0]
    return Tiff(path, bo, len(buf), ifd0, subs, exif), buf


def _get(ifd, tag, default=None):
    e = ifd.get(tag)
    if e is None:
        return default
    return e.values


def _get1(ifd, tag, default=None):
    v = _get(ifd, tag)
    return default if v is None or len(v) == 0 else v[0]


def _raw_ifd(t):
    cands = [t.ifd0] + t.subifds
    for ifd in cands:
        if _get1(ifd, T_NEWSUBFILETYPE, 0) == 0 and _get1(ifd, T_PHOTOMETRIC) == CFA_PHOTOMETRIC:
            return ifd
    for ifd in cands:
        if _get1(ifd, T_PHOTOMETRIC) == LINEARRAW_PHOTOMETRIC:
            raise ValueError('%s: PhotometricInterpretation = 34892 (LinearRaw): a demosaiced image, not a CFA mosaic' % t.path)
    raise ValueError('%s: no raw image: no IFD with NewSubFileType = 0 and PhotometricInterpretation = 32803 in IFD0 or its SubIFDs' % t.path)


class Layout:
    """Where the raw IFD's pixels are: H, W, bits, compression, byte order and the streams (offset, bytes, x0, y0, tw, th)."""
    def __init__(self, H, W, bits, compression, big_endian, streams):
        self.H, self.W, self.bits, self.compression, self.big_endian, self.streams = H, W, bits, compression, big_endian, streams


def image_layout(t, ifd):
    """The strips or tiles of one IFD, every offset and count checked against the file size."""
    p = t.path
    for tag, name in ((T_WIDTH, 'ImageWidth'), (T_LENGTH, 'ImageLength')):
        if _get1(ifd, tag) is None or int(_get1(ifd, tag)) < 1:
            raise ValueError('%s: %s = %r' % (p, name, _get1(ifd, tag)))
    W, H = int(_get1(ifd, T_WIDTH)), int(_get1(ifd, T_LENGTH))
    if H * W >= 1 << 31:
        raise ValueError('%s: ImageWidth x ImageLength = %d x %d: more than 2^31 sites' % (p, W, H))
    spp = int(_get1(ifd, T_SPP, 1))
    if spp != 1:
        raise ValueError('%s: SamplesPerPixel = %d: a CFA mosaic has 1' % (p, spp))
    comp = int(_get1(ifd, T_COMPRESSION, 1))
    if comp not in (1, 7):
        raise ValueError('%s: Compression = %d%s: only 1 (uncompressed) and 7 (lossless JPEG) are read'
                         % (p, comp, ' (%s)' % COMPRESSION_NAMES[comp] if comp in COMPRESSION_NAMES else ''))
    if int(_get1(ifd, T_FILLORDER, 1)) != 1:
        raise ValueError('%s: FillOrder = %d: only 1 (MSB first) is read' % (p, int(_get1(ifd, T_FILLORDER))))
    sf = int(_get1(ifd, T_SAMPLEFORMAT, 1))
    if sf != 1:
        raise ValueError('%s: SampleFormat = %d%s: only 1 (unsigned integer) is read' % (p, sf, ' (floating point)' if sf == 3 else ''))
    bits = int(_get1(ifd, T_BITS, 1))
    if comp == 1 and bits not in UNPACK_BITS:
        raise ValueError('%s: BitsPerSample = %d with Compression = 1: one of %r is read' % (p, bits, UNPACK_BITS))
    if comp == 7 and not 2 <= bits <= 16:
        raise ValueError('%s: BitsPerSample = %d with Compression = 7: 2..16 is read' % (p, bits))
    streams = []
    if T_TILEOFFSETS in ifd or T_TILEWIDTH in ifd:
        for tag, name in ((T_TILEWIDTH, 'TileWidth'), (T_TILELENGTH, 'TileLength'), (T_TILEOFFSETS, 'TileOffsets'), (T_TILEBYTECOUNTS, 'TileByteCounts')):
            if tag not in ifd:
                raise ValueError('%s: tiles without %s' % (p, name))
        tw, th = int(_get1(ifd, T_TILEWIDTH)), int(_get1(ifd, T_TILELENGTH))
        if tw < 1 or th < 1 or tw > 65536 or th > 65536:
            raise ValueError('%s: TileWidth x TileLength = %d x %d' % (p, tw, th))
        offs, cnts, oname = _get(ifd, T_TILEOFFSETS), _get(ifd, T_TILEBYTECOUNTS), 'TileOffsets'
        nx, ny = -(-W // tw), -(-H // th)
        if len(offs) != nx * ny or len(cnts) != nx * ny:
            raise ValueError('%s: TileOffsets / TileByteCounts hold %d / %d values, %d x %d tiles need %d' % (p, len(offs), len(cnts), nx, ny, nx * ny))
        geo = [((i % nx) * tw, (i // nx) * th, tw, th) for i in range(nx * ny)]
    else:
        for tag, name in ((T_STRIPOFFSETS, 'StripOffsets'), (T_STRIPBYTECOUNTS, 'StripByteCounts')):
            if tag not in ifd:
                raise ValueError('%s: neither tiles nor %s' % (p, name))
        rps = min(int(_get1(ifd, T_ROWSPERSTRIP, H)), H)
        if rps < 1:
            raise ValueError('%s: RowsPerStrip = %d' % (p, rps))
        offs, cnts, oname = _get(ifd, T_STRIPOFFSETS), _get(ifd, T_STRIPBYTECOUNTS), 'StripOffsets'
        ns = -(-H // rps)
        if len(offs) != ns or len(cnts) != ns:
            raise ValueError('%s: StripOffsets / StripByteCounts hold %d / %d values, %d rows in strips of %d need %d' % (p, len(offs), len(cnts), H, rps, ns))
        if W > 65536:
            raise ValueError('%s: ImageWidth = %d in strips' % (p, W))
        geo = [(0, i * rps, W, min(rps, H - i * rps)) for i in range(ns)]
    for i, (o, c, g) in enumerate(zip(offs, cnts, geo)):
        o, c = int(o), int(c)
        if o < 8 or c < 1 or o + c > t.size:
            raise ValueError('%s: %s[%d] = %d with %d bytes lies outside the file (%d bytes)' % (p, oname, i, o, c, t.size))
        if comp == 1 and c < g[3] * ((g[2] * bits + 7) // 8):
            raise ValueError('%s: stream %d: %d bytes for %d rows of %d %d-bit samples (%s)' % (p, i, c, g[3], g[2], bits, oname.replace('Offsets', 'ByteCounts')))
        streams.append((o, c) + g)
    return Layout(H, W, bits, comp, t.order == '>', streams)


# ---- metadata -------------------------------------------------------------------------------------------------------------------
def _frac(pair, tag, path):
    if pair[1] == 0:
        raise ValueError('%s: %s holds a rational with denominator 0' % (path, tag))
    return Fraction(int(pair[0]), int(pair[1]))


def _numbers(e, name, path):
    """an entry's values as Fractions (BlackLevel may be SHORT, LONG or RATIONAL)"""
    if e.type in (RATIONAL, SRATIONAL):
        return [_frac(v, name, path) for v in e.values]
    return [Fraction(int(v)) for v in e.values]


def ccm_from_color_matrix(cm):
    """ColorMatrix (XYZ -> camera, 3x3) -> the camera -> linear sRGB matrix rawpy reports as rgb_camera_matrix[:3, :3], in float64."""
    cam_from_rgb = np.asarray(cm, dtype=np.float64).reshape(3, 3) @ SRGB_TO_XYZ
    cam_from_rgb = cam_from_rgb / cam_from_rgb.sum(axis=1, keepdims=True)
    return np.linalg.inv(cam_from_rgb)


def _active_area(ifd, H, W, path):
    aa = _get(ifd, T_ACTIVEAREA)
    if aa is None:
        return (0, 0, H, W)
    aa = tuple(int(v) for v in aa)
    if len(aa) != 4 or not (0 <= aa[0] < aa[2] <= H and 0 <= aa[1] < aa[3] <= W):
        raise ValueError('%s: ActiveArea = %r does not lie inside the %d x %d image' % (path, aa, H, W))
    return aa


def _meta(t, ifd):
    p = t.path
    H, W = int(_get1(ifd, T_LENGTH)), int(_get1(ifd, T_WIDTH))
    m = {}
    dim = tuple(int(v) for v in _get(ifd, T_CFADIM, ()))
    if dim == (2, 2):
        m['cfa'] = 'bayer'
    elif dim == (6, 6):
        m['cfa'] = 'xtrans'
    else:
        raise ValueError('%s: CFARepeatPatternDim = %r: (2, 2) Bayer and (6, 6) X-Trans are read' % (p, dim))
    plane = tuple(int(v) for v in _get(ifd, T_CFAPLANECOLOR, (0, 1, 2)))
    pat = [int(v) for v in _get(ifd, T_CFAPATTERN, ())]
    if len(pat) != dim[0] * dim[1] or any(v not in (0, 1, 2) for v in pat) or plane != (0, 1, 2):
        raise ValueError('%s: CFAPattern = %r (CFAPlaneColor %r): %d values of 0 (R), 1 (G), 2 (B) are read' % (p, pat, plane, dim[0] * dim[1]))
    if m['cfa'] == 'bayer':
        if sorted(pat) != [0, 1, 1, 2]:
            raise ValueError('%s: CFAPattern = %r: a Bayer cell has one red, two green and one blue site' % (p, pat))
        codes, greens = [], 0
        for v in pat:
            if v == 1:
                codes.append(1 if greens == 0 else 3)
                greens += 1
            else:
                codes.append(v)
        m['raw_pattern'] = [codes[:2], codes[2:]]
    else:
        m['raw_pattern'] = [pat[6 * r:6 * r + 6] for r in range(6)]
    # black levels
    bdim = tuple(int(v) for v in _get(ifd, T_BLACKDIM, (1, 1)))
    if len(bdim) != 2 or bdim[0] < 1 or bdim[1] < 1:
        raise ValueError('%s: BlackLevelRepeatDim = %r' % (p, bdim))
    blk = _numbers(ifd[T_BLACK], 'BlackLevel', p) if T_BLACK in ifd else [Fraction(0)] * (bdim[0] * bdim[1])
    if len(blk) != bdim[0] * bdim[1]:
        raise ValueError('%s: BlackLevel holds %d values, BlackLevelRepeatDim = %r needs %d' % (p, len(blk), bdim, bdim[0] * bdim[1]))
    for tag, name in ((T_BLACKDH, 'BlackLevelDeltaH'), (T_BLACKDV, 'BlackLevelDeltaV')):
        if tag in ifd and any(v != 0 for v in _numbers(ifd[tag], name, p)):
            raise ValueError('%s: %s is not zero: per-column / per-row black levels are not applied' % (p, name))

    def num(f):
        return int(f) if f.denominator == 1 else float(f)
    if m['cfa'] == 'bayer':
        if 2 % bdim[0] or 2 % bdim[1]:
            raise ValueError('%s: BlackLevelRepeatDim = %r does not divide the 2 x 2 cell' % (p, bdim))
        bl = [None] * 4
        for y in range(2):
            for x in range(2):
                bl[m['raw_pattern'][y][x]] = num(blk[(y % bdim[0]) * bdim[1] + x % bdim[1]])
        m['black_level'] = bl
    else:
        if any(v != blk[0] for v in blk):
            raise ValueError('%s: BlackLevel = %r: X-Trans takes one black level for all sites' % (p, [num(v) for v in blk]))
        m['black_level'] = num(blk[0])
    bits = int(_get1(ifd, T_BITS, 1))
    m['white_point'] = int(_get1(ifd, T_WHITE, (1 << bits) - 1))
    # colour: the IFD0 tags (a raw SubIFD carries none)
    src = t.ifd0
    if T_ASSHOTNEUTRAL in src:
        n = _numbers(src[T_ASSHOTNEUTRAL], 'AsShotNeutral', p)
        if len(n) != 3 or n[0] <= 0 or n[2] <= 0:
            raise ValueError('%s: AsShotNeutral = %r: three positive values are read' % (p, [float(v) for v in n]))
        m['wb'] = [float(n[1] / n[0]), 1.0, float(n[1] / n[2])]
    cm_tag = None
    if T_COLORMATRIX2 in src and int(_get1(src, T_ILLUMINANT2, 0)) == D65 and int(_get1(src, T_ILLUMINANT1, 0)) != D65:
        cm_tag = T_COLORMATRIX2
    elif T_COLORMATRIX1 in src:
        cm_tag = T_COLORMATRIX1
    if cm_tag is not None:
        cm = _numbers(src[cm_tag], 'ColorMatrix', p)
        if len(cm) != 9:
            raise ValueError('%s: ColorMatrix holds %d values: 9 (three colour planes) are read' % (p, len(cm)))
        m['ccm'] = ccm_from_color_matrix([float(v) for v in cm]).tolist()
    for ifd_ in (t.exif, t.ifd0):
        if 'iso' not in m and T_ISO in ifd_:
            m['iso'] = int(_get1(ifd_, T_ISO))
        if 'exposure_time' not in m and T_EXPOSURETIME in ifd_:
            m['exposure_time'] = float(_frac(ifd_[T_EXPOSURETIME].values[0], 'ExposureTime', p))
    if T_MAKE in src:
        m['make'] = src[T_MAKE].values.strip()
    if T_MODEL in src:
        m['model'] = src[T_MODEL].values.strip()
    m['active_area'] = list(_active_area(ifd, H, W, p))
    m['bits'] = bits
    m['compression'] = int(_get1(ifd, T_COMPRESSION, 1))
    m['opcodes'] = [name for tag, name in OPCODE_TAGS if tag in ifd or tag in t.ifd0]
    # the frame of the picture, only where the file carries it: Orientation (IFD0) and the default crop (raw IFD; SHORT, LONG or RATIONAL,
    # origin as (x, y) and size as (width, height), relative to the visible mosaic) as (y0, x0, h, w).  This is also read_dng's path, which
    # uses neither: a tag with values nobody can use (some writers store Orientation 0) gives no key and never an error, so such a file
    # reads as it always did, and --orient auto / --crop default treat it as a file without the tag.
    if T_ORIENTATION in t.ifd0 and t.ifd0[T_ORIENTATION].type in (SHORT, LONG) and 1 <= int(_get1(t.ifd0, T_ORIENTATION)) <= 8:
        m['orientation'] = int(_get1(t.ifd0, T_ORIENTATION))
    if T_DEFAULTCROPSIZE in ifd:
        try:
            size = _numbers(ifd[T_DEFAULTCROPSIZE], 'DefaultCropSize', p)
            origin = _numbers(ifd[T_DEFAULTCROPORIGIN], 'DefaultCropOrigin', p) if T_DEFAULTCROPORIGIN in ifd else [Fraction(0), Fraction(0)]
        except (ValueError, TypeError):                             # a rational with denominator 0, a type that holds no numbers
            size = origin = []
        if len(size) == 2 and len(origin) == 2 and min(size) > 0 and min(origin) >= 0:
            m['default_crop'] = [num(origin[1]), num(origin[0]), num(size[1]), num(size[0])]
    return m


def dng_meta(path):
    """The tags of a DNG in the sidecar's keys; decodes no pixels and touches no device."""
    t, _ = parse_tiff(path)
    ifd = _raw_ifd(t)
    image_layout(t, ifd)
    return _meta(t, ifd)


# ---- lossless JPEG: markers and tables (host) ---------------------------------------------------------------------------------------
def huff_record(counts, symbols, what):
    """DHT counts[1..16] and the symbols in code order -> one EldDngHuff record (a numpy void).  Refuses a symbol above 16, more than 32
    symbols and counts that are no prefix code."""
    if len(counts) != 16 or sum(counts) != len(symbols) or len(symbols) < 1 or len(symbols) > 32:
        raise ValueError('%s: a Huffman table of %d symbols with counts %r' % (what, len(symbols), list(counts)))
    if any(s > 16 for s in symbols):
        raise ValueError('%s: Huffman symbol %d: lossless JPEG has the categories 0..16' % (what, max(symbols)))
    rec = np.zeros((), dtype=L.DNG_HUFF_DTYPE)
    rec['maxcode'][:] = -1
    rec['vals'][:len(symbols)] = symbols
    rec['nvals'] = len(symbols)
    code, k = 0, 0
    for l in range(1, 17):
        n = counts[l - 1]
        if n:
            if code + n > (1 << l):
                raise ValueError('%s: the Huffman code lengths %r are no prefix code' % (what, list(counts)))
            rec['valoff'][l] = k - code
            rec['maxcode'][l] = code + n - 1
            if l <= L.DNG_FAST_BITS:
                for j in range(n):
                    lo = (code + j) << (L.DNG_FAST_BITS - l)
                    rec['fast'][lo:lo + (1 << (L.DNG_FAST_BITS - l))] = (l << 8) | symbols[k + j]
            code += n
            k += n
        code <<= 1
    return rec


def parse_ljpeg(buf, off, nbytes, what):
    """The marker segments of one lossless-JPEG stream at buf[off:off + nbytes] -> dict(P, Y, X, Nf, pred, tables: per component (counts,
    symbols), data: (offset, bytes) of the entropy-coded segment).  No scan of the entropy data."""
    end = off + nbytes
    if nbytes < 4 or buf[off] != 0xFF or buf[off + 1] != 0xD8:
        raise ValueError('%s: no JPEG SOI marker' % what)
    pos = off + 2
    dht, sof, comps = {}, None, None
    while True:
        if pos + 4 > end:
            raise ValueError('%s: the JPEG markers run beyond the stream' % what)
        if buf[pos] != 0xFF:
            raise ValueError('%s: byte %d is no JPEG marker' % (what, pos - off))
        mk = buf[pos + 1]
        if mk == 0xFF:
            pos += 1
            continue
        ln = (buf[pos + 2] << 8) | buf[pos + 3]
        seg, seg_end = pos + 4, pos + 2 + ln
        if ln < 2 or seg_end > end:
            raise ValueError('%s: JPEG marker FF%02X with length %d runs beyond the stream' % (what, mk, ln))
        if mk == 0xC3:
            if ln < 8:
                raise ValueError('%s: SOF3 of %d bytes' % (what, ln))
            P, Y, X, Nf = buf[seg], (buf[seg + 1] << 8) | buf[seg + 2], (buf[seg + 3] << 8) | buf[seg + 4], buf[seg + 5]
            if not (2 <= P <= 16 and 1 <= Nf <= 4 and X >= 1 and Y >= 1) or ln != 8 + 3 * Nf:
                raise ValueError('%s: SOF3 with precision %d, %d lines, %d samples per line, %d components' % (what, P, Y, X, Nf))
            sof = (P, Y, X, Nf)
            comps = [buf[seg + 6 + 3 * k] for k in range(Nf)]
            if any(buf[seg + 7 + 3 * k] != 0x11 for k in range(Nf)):
                raise ValueError('%s: SOF3 with a sampling factor other than 1 x 1' % what)
        elif mk in (0xC0, 0xC1, 0xC2, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError('%s: JPEG frame marker FF%02X: only SOF3 (lossless, Huffman) is read' % (what, mk))
        elif mk == 0xC4:
            q = seg
            while q < seg_end:
                if q + 17 > seg_end:
                    raise ValueError('%s: DHT runs beyond its segment' % what)
                tc_th = buf[q]
                counts = list(buf[q + 1:q + 17])
                n = sum(counts)
                if q + 17 + n > seg_end:
                    raise ValueError('%s: DHT runs beyond its segment' % what)
                if tc_th >> 4 != 0:
                    raise ValueError('%s: DHT of class %d: lossless JPEG has DC tables only' % (what, tc_th >> 4))
                dht[tc_th & 15] = (counts, list(buf[q + 17:q + 17 + n]))
                q += 17 + n
        elif mk == 0xDD:
            if ln >= 4 and ((buf[seg] << 8) | buf[seg + 1]) != 0:
                raise ValueError('%s: restart interval (DRI) = %d: restart markers are not read' % (what, (buf[seg] << 8) | buf[seg + 1]))
        elif mk == 0xDA:
            if sof is None:
                raise ValueError('%s: SOS before SOF3' % what)
            P, Y, X, Nf = sof
            Ns = buf[seg]
            if Ns != Nf:
                raise ValueError('%s: more than one scan: the first scan holds %d of %d components' % (what, Ns, Nf))
            if ln != 6 + 2 * Ns:
                raise ValueError('%s: SOS of %d bytes for %d components' % (what, ln, Ns))
            tabs = []
            for k in range(Ns):
                cs, td = buf[seg + 1 + 2 * k], buf[seg + 2 + 2 * k] >> 4
                if cs != comps[k]:
                    raise ValueError('%s: SOS names component %d where SOF3 has %d' % (what, cs, comps[k]))
                if td not in dht:
                    raise ValueError('%s: SOS selects Huffman table %d, which no DHT defines' % (what, td))
                tabs.append(dht[td])
            pred, al = buf[seg + 1 + 2 * Ns], buf[seg + 3 + 2 * Ns] & 15
            if not 1 <= pred <= 7:
                raise ValueError('%s: predictor %d: 1..7 are read' % (what, pred))
            if al != 0:
                raise ValueError('%s: point transform %d: only 0 is read' % (what, al))
            return {'P': P, 'Y': Y, 'X': X, 'Nf': Nf, 'pred': pred, 'tables': tabs, 'data': (seg_end, end - seg_end)}
        pos = seg_end


# ---- the decode -------------------------------------------------------------------------------------------------------------------
_LANES = 0                               # streams per wave of eld_dng_ljpeg_u16 (0: the library chooses); tests run both ends


def _plan(path):
    """Everything the decode needs, validated on the host: (Tiff, raw IFD, Layout, meta, blob range, stream records, Huffman records, ws
    elements, linearisation table)."""
    t, buf = parse_tiff(path)
    ifd = _raw_ifd(t)
    lay = image_layout(t, ifd)
    meta = _meta(t, ifd)
    lin = None
    if T_LINTABLE in ifd:
        lin = np.ascontiguousarray(np.asarray(_get(ifd, T_LINTABLE), dtype=np.uint16))
        if lin.size < 1 or lin.size > 65536:
            raise ValueError('%s: LinearizationTable of %d entries' % (path, lin.size))
    lo = min(s[0] for s in lay.streams)
    hi = max(s[0] + s[1] for s in lay.streams)
    if hi - lo >= 1 << 32:
        raise ValueError('%s: the streams span %d bytes' % (path, hi - lo))
    recs = np.zeros(len(lay.streams), dtype=L.DNG_STREAM_DTYPE)
    tables, index, ws = [], {}, 0
    for i, (o, c, x0, y0, tw, th) in enumerate(lay.streams):
        r = recs[i]
        r['x0'], r['y0'], r['tw'], r['th'] = x0, y0, tw, th
        if lay.compression == 1:
            r['data_off'], r['data_len'] = o - lo, c
            continue
        what = '%s: stream %d' % (path, i)
        j = parse_ljpeg(buf, o, c, what)
        if j['Y'] * j['X'] * j['Nf'] != tw * th:
            raise ValueError('%s: the JPEG holds %d x %d x %d samples, its %s %d x %d' % (what, j['Y'], j['X'], j['Nf'],
                                                                                        'tile' if T_TILEOFFSETS in ifd else 'strip', th, tw))
        r['data_off'], r['data_len'] = j['data'][0] - lo, j['data'][1]
        r['P'], r['X'], r['Y'], r['Nf'], r['pred'] = j['P'], j['X'], j['Y'], j['Nf'], j['pred']
        for k, (counts, syms) in enumerate(j['tables']):
            key = (tuple(counts), tuple(syms))
            if key not in index:
                if len(tables) >= 65535:
                    raise ValueError('%s: more than 65535 distinct Huffman tables' % path)
                index[key] = len(tables)
                tables.append(huff_record(counts, syms, what))
            r['table'][k] = index[key]
        if j['pred'] >= 2:
            r['ws_off'] = ws
            ws += j['X'] * j['Nf']
    huff = np.array(tables, dtype=L.DNG_HUFF_DTYPE) if tables else np.zeros(0, dtype=L.DNG_HUFF_DTYPE)
    return t, buf, lay, meta, (lo, hi), recs, huff, ws, lin


def read_dng(path, device=None):
    """-> (mosaic, meta).  mosaic: the visible mosaic (the ActiveArea of the raw IFD), (Hm, Wm) uint16 as rawpy's raw_image_visible;
    device None: a NumPy array (decoded on the GPU and copied back -- there is no CPU decoder in the package); else a contiguous CUDA int16-view
    tensor on `device`, decoded there, as denoise_raw and the pools accept.  meta: dng_meta(path).  A corrupt stream is a ValueError that names
    the stream and the reason."""
    path = os.fspath(path)
    t, buf, lay, meta, (lo, hi), recs, huff, ws_elems, lin = _plan(path)
    import torch
    lib = L.lib()
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != 'cuda':
        raise ValueError('read_dng decodes on a CUDA device, got %s' % dev)
    top, left, bottom, right = meta['active_area']
    Hm, Wm = bottom - top, right - left
    host = np.zeros(hi - lo + PAD, dtype=np.uint8)
    host[:hi - lo] = np.frombuffer(buf, dtype=np.uint8, count=hi - lo, offset=lo)
    with torch.cuda.device(dev):
        blob = torch.from_numpy(host).to(dev)
        d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
        d_lin = None if lin is None else torch.from_numpy(lin.view(np.int16)).to(dev)
        out = torch.zeros((Hm, Wm), dtype=torch.int16, device=dev)
        status = torch.zeros(len(recs), dtype=torch.int32, device=dev)
        n_lin = 0 if lin is None else int(lin.size)
        if lay.compression == 1:
            L.check(lib.eld_dng_unpack_u16(L.dptr(blob), hi - lo, L.dptr(d_recs), len(recs), lay.bits, int(lay.big_endian), lay.H, lay.W, top, left,
                                           Hm, Wm, L.dptr(d_lin), n_lin, L.dptr(out), L.dptr(status), L.cur_stream()), 'eld_dng_unpack_u16')
        else:
            d_huff = torch.from_numpy(huff.view(np.uint8).reshape(-1).copy()).to(dev)
            ws = torch.empty(max(ws_elems, 1), dtype=torch.int16, device=dev)
            L.check(lib.eld_dng_ljpeg_u16(L.dptr(blob), hi - lo, L.dptr(d_recs), len(recs), L.dptr(d_huff), len(huff), lay.H, lay.W, top, left, Hm, Wm,
                                          L.dptr(d_lin), n_lin, L.dptr(ws), ws_elems, int(_LANES), L.dptr(out), L.dptr(status), L.cur_stream()),
                    'eld_dng_ljpeg_u16')
        st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if bad.size:
        i = int(bad[0])
        raise ValueError('%s: stream %d: %s%s' % (path, i, L.DNG_STATUS.get(int(st[i]), 'status %d' % st[i]),
                                                  '' if bad.size == 1 else ' (and %d more streams)' % (bad.size - 1)))
    if device is None:
        return out.cpu().numpy().view(np.uint16), meta
    return out, meta


def load_frame(path):
    """One frame from a path: .npy -> np.load(path), .dng (any case) -> the visible mosaic of read_dng(path)."""
    if str(path).lower().endswith('.dng'):
        return read_dng(path)[0]
    return np.load(path)


def is_dng(path):
    return isinstance(path, (str, os.PathLike)) and str(path).lower().endswith('.dng')


SAME_SENSOR_KEYS = ('cfa', 'raw_pattern', 'black_level', 'white_point')


def common_meta(paths):
    """dng_meta of the first .dng among `paths` (None when there is none); every other .dng must agree with it on cfa, raw_pattern,
    black_level and white_point, or the ValueError names the file."""
    first, name = None, None
    for p in paths:
        if not is_dng(p):
            continue
        m = dng_meta(p)
        if first is None:
            first, name = m, p
            continue
        for k in SAME_SENSOR_KEYS:
            if m.get(k) != first.get(k):
                raise ValueError('%s: %s = %r, but %s has %r: the inputs of one run must come from one sensor setting' % (p, k, m.get(k), name, first.get(k)))
    return first


def fill_from_tags(o, paths, keys=SAME_SENSOR_KEYS):
    """Options `o` (command line over sidecar, already merged) with the `keys` it leaves open taken from the tags of the first .dng among
    `paths`: the third rank of the precedence, above the built-in defaults.  The sensor keys are only taken for the CFA `o` ends up with;
    the Bayer raw_pattern is the only pattern the options carry.  -> the tags (None without a DNG)."""
    tags = common_meta(paths)
    if tags is None:
        return None
    if o.get('cfa') is None:
        o['cfa'] = tags['cfa']
    if o['cfa'] != tags['cfa']:
        return tags
    for k in keys:
        if k == 'raw_pattern' and tags['cfa'] != 'bayer':
            continue
        if o.get(k) is None and tags.get(k) is not None:
            o[k] = tags[k]
    return tags


# ---- writer -----------------------------------------------------------------------------------------------------------------------
def _rational(v, max_den=1000000):
    """a float as the nearest (numerator, denominator) with a denominator up to max_den; a Fraction as it is"""
    f = v if isinstance(v, Fraction) else Fraction(v).limit_denominator(max_den)
    return (f.numerator, f.denominator)


def color_matrix_from_ccm(ccm):
    """The ColorMatrix1 rationals (denominator 10000) write_dng stores for a camera -> sRGB matrix `ccm`: ColorMatrix = inv(ccm) . inv(M),
    the inverse of dng_meta's mapping up to its per-row normalisation."""
    cm = np.linalg.inv(np.asarray(ccm, dtype=np.float64).reshape(3, 3)) @ np.linalg.inv(SRGB_TO_XYZ)
    return [(int(round(v * 10000)), 10000) for v in cm.reshape(-1)]


COPIED_RAW = (T_CFADIM, T_CFAPATTERN, T_CFAPLANECOLOR, T_BLACKDIM, T_BLACK, T_WHITE, T_DEFAULTCROPORIGIN, T_DEFAULTCROPSIZE)
COPIED_IFD0 = (T_MAKE, T_MODEL, T_UNIQUEMODEL, T_COLORMATRIX1, T_COLORMATRIX2, T_ILLUMINANT1, T_ILLUMINANT2, T_ANALOGBALANCE, T_ASSHOTNEUTRAL,
               T_ISO, T_EXPOSURETIME, T_ORIENTATION)
COPIED_EXIF = (T_ISO, T_EXPOSURETIME)


def _pack_entry(e):
    """-> (type, count, little-endian payload bytes)"""
    if e.type == ASCII:
        b = e.values.encode('latin-1') + b'\0'
        return ASCII, len(b), b
    if e.type in (RATIONAL, SRATIONAL):
        flat = [int(x) for pr in e.values for x in pr]
        return e.type, len(e.values), struct.pack('<%d%s' % (len(flat), 'I' if e.type == RATIONAL else 'i'), *flat)
    if isinstance(e.values, bytes):
        return e.type, len(e.values), e.values
    vals = [int(v) if e.type not in (11, 12) else float(v) for v in e.values]
    return e.type, len(vals), struct.pack('<%d%s' % (len(vals), TYPE_FMT[e.type]), *vals)


# ---- lossless-JPEG encoder: tables and markers on the host, the bits on the device (csrc/dng_enc.hip) ------------------
DEFAULT_TILE = (256, 256)
COMPRESSION_CHOICES = {'none': 1, 'ljpeg': 7}                        # the command lines' names of write_dng's compression
_EXTRA_BITS = np.array(list(range(16)) + [0], dtype=np.int64)        # SSSS extra bits behind the code; SSSS = 16 carries none


def huffman_lengths(hist, bins=17):
    """The 17-bin SSSS histogram of a stream -> (counts of the code lengths 1..16, the symbols in code order), as a DHT segment stores them:
    ITU-T T.81 Annex K.2.  Figure K.1 with an 18th symbol of frequency 1 that keeps the all-ones code point free (it ends up with the longest
    code and is dropped); the least frequency goes to V1, the next to V2, ties to the larger index; Figure K.3 limits the lengths to 16.
    bins: the size of the alphabet (eld_amd.jpeg: 12 DC sizes, 256 AC run/size bytes)."""
    freq = [int(v) for v in hist] + [1]
    if len(freq) != bins + 1 or min(freq) < 0:
        raise ValueError('a histogram of %d non-negative counts, got %r' % (bins, list(hist)))
    n = len(freq)
    size, chain = [0] * n, [-1] * n

    def least(skip):
        best = -1
        for i in range(n):
            if freq[i] > 0 and i != skip and (best < 0 or freq[i] <= freq[best]):
                best = i
        return best
    while True:
        v1 = least(-1)
        v2 = least(v1)
        if v2 < 0:
            break
        freq[v1] += freq[v2]
        freq[v2] = 0
        size[v1] += 1                                                # every symbol of both subtrees is one bit longer
        while chain[v1] >= 0:
            v1 = chain[v1]
            size[v1] += 1
        chain[v1] = v2                                               # V2's subtree hangs behind the end of V1's chain
        size[v2] += 1
        while chain[v2] >= 0:
            v2 = chain[v2]
            size[v2] += 1
    top = max(32, bins)                                              # no code is longer than the alphabet
    counts = [0] * (top + 1)
    for s in size:
        if s:
            counts[s] += 1
    for l in range(top, 16, -1):                                      # Figure K.3: a pair of the longest codes moves up under a shorter one
        while counts[l] > 0:
            j = l - 2
            while counts[j] == 0:
                j -= 1
            counts[l] -= 2
            counts[l - 1] += 1
            counts[j + 1] += 2
            counts[j] -= 1
    l = 16
    while counts[l] == 0:
        l -= 1
    counts[l] -= 1                                                   # the reserved code point
    by_length = sorted((size[s], s) for s in range(n - 1) if size[s])
    return counts[1:17], [s for _, s in by_length]


def encoder_table(counts, symbols, bins=17):
    """-> `bins` uint32, [ssss] = (code length << 16) | canonical code (Annex C), 0 for a symbol the table lacks"""
    tab = np.zeros(bins, dtype=np.uint32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            tab[symbols[k]] = (l << 16) | code
            code += 1
            k += 1
        code <<= 1
    return tab


def ljpeg_header(P, X, Y, counts, symbols):
    """SOI, SOF3 (two components, ids 1 and 2, 1 x 1 sampling), DHT (class 0, id 0), SOS (both components on table 0, predictor 1)"""
    sof = struct.pack('>BHHB', P, Y, X, 2) + bytes([1, 0x11, 0, 2, 0x11, 0])
    dht = bytes([0]) + bytes(counts) + bytes(symbols)
    sos = bytes([2, 1, 0, 2, 0, 1, 0, 0])
    return (b'\xff\xd8\xff\xc3' + struct.pack('>H', 2 + len(sof)) + sof + b'\xff\xc4' + struct.pack('>H', 2 + len(dht)) + dht +
            b'\xff\xda' + struct.pack('>H', 2 + len(sos)) + sos)


def _check_encode_args(tile, bits, segment=0, chunk=0):
    try:
        th, tw = (int(v) for v in tile)
    except (TypeError, ValueError):
        raise ValueError('tile takes (TileLength, TileWidth), got %r' % (tile,))
    if tw % 2:
        raise ValueError('tile %r: an odd TileWidth does not split into the two components of the JPEG' % (tile,))
    if th < 16 or tw < 16 or th % 16 or tw % 16:
        raise ValueError('tile %r: TileLength and TileWidth must be multiples of 16 (TIFF 6.0, section 15)' % (tile,))
    if th * tw > 1 << 24:
        raise ValueError('tile %r: more than 2^24 samples' % (tile,))
    bits = int(bits)
    if not 8 <= bits <= 16:
        raise ValueError('bits = %d: the lossless-JPEG writer takes 8..16' % bits)
    segment, chunk = int(segment), int(chunk)
    if segment and (segment % L.DNG_ENC_MIN_SEGMENT or not L.DNG_ENC_MIN_SEGMENT <= segment <= L.DNG_ENC_MAX_SEGMENT):
        raise ValueError('segment = %d samples: a multiple of %d up to %d, or 0 for the default' % (segment, L.DNG_ENC_MIN_SEGMENT, L.DNG_ENC_MAX_SEGMENT))
    if chunk and (chunk % L.DNG_ENC_MIN_CHUNK or not L.DNG_ENC_MIN_CHUNK <= chunk <= L.DNG_ENC_MAX_CHUNK):
        raise ValueError('chunk = %d bytes: a multiple of %d up to %d, or 0 for the default' % (chunk, L.DNG_ENC_MIN_CHUNK, L.DNG_ENC_MAX_CHUNK))
    return (th, tw), bits, segment or L.DNG_ENC_SEGMENT, chunk or L.DNG_ENC_CHUNK


def _mosaic_shape(mosaic, who):
    """(H, W) of a NumPy uint16 / int16 array or a torch int16 / uint16 tensor; anything else is a ValueError"""
    if isinstance(mosaic, np.ndarray):
        ok = mosaic.dtype in (np.uint16, np.int16)
    else:
        ok = str(getattr(mosaic, 'dtype', None)) in ('torch.int16', 'torch.uint16')
    if not ok or len(mosaic.shape) != 2 or mosaic.shape[0] < 1 or mosaic.shape[1] < 1:
        raise ValueError('%s takes one (H, W) uint16 mosaic, got %s %s' % (who, getattr(mosaic, 'dtype', type(mosaic)), tuple(getattr(mosaic, 'shape', ()))))
    return int(mosaic.shape[0]), int(mosaic.shape[1])


class Encoder:
    """One encode, step by step (encode_ljpeg runs the steps in order; tools/dng_enc_time.py times them one by one):
    hist() -> plan() -> pack() -> ffcount() -> sizes() -> stuff() -> streams().  The mosaic stays on its device; the host sees the
    histograms, the stuffed sizes and the compressed bytes."""
    def __init__(self, mosaic, tile=DEFAULT_TILE, bits=16, segment=0, chunk=0):
        (self.th, self.tw), self.bits, self.segment, self.chunk = _check_encode_args(tile, bits, segment, chunk)
        self.H, self.W = _mosaic_shape(mosaic, 'encode_ljpeg')
        self.ny, self.nx = -(-self.H // self.th), -(-self.W // self.tw)
        self.ns = self.ny * self.nx
        if self.ns > 65535:
            raise ValueError('%d x %d in tiles of %d x %d: %d tiles, more than 65535' % (self.H, self.W, self.th, self.tw, self.ns))
        if self.H * self.W >= 1 << 31:
            raise ValueError('a mosaic of %d x %d: more than 2^31 sites' % (self.H, self.W))
        self.nseg = -(-(self.th * self.tw) // self.segment)
        import torch
        self.torch = torch
        self.lib = L.lib()
        if isinstance(mosaic, np.ndarray):
            mosaic = torch.from_numpy(np.ascontiguousarray(mosaic).view(np.int16)).to(torch.device('cuda', torch.cuda.current_device()))
        if mosaic.device.type != 'cuda':
            raise ValueError('encode_ljpeg encodes on a CUDA device, got a tensor on %s' % mosaic.device)
        self.mosaic = mosaic.detach().contiguous()
        self.dev = self.mosaic.device

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.dev)

    def _geom(self):
        return (L.dptr(self.mosaic), self.H, self.W, self.th, self.tw, self.bits, self.segment)

    def hist(self):
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.d_hist = torch.empty(self.ns * self.nseg * 17, dtype=torch.int32, device=self.dev)
            self.d_max = torch.empty(self.ns, dtype=torch.int32, device=self.dev)
            L.check(self.lib.eld_dng_enc_hist_u16(*self._geom(), L.dptr(self.d_hist), L.dptr(self.d_max), L.cur_stream()), 'eld_dng_enc_hist_u16')

    def plan(self):
        """The histograms -> every stream's table and markers, every segment's first bit, the layout of the unstuffed bytes and its chunks."""
        h = self.d_hist.cpu().numpy().view(np.uint32).reshape(self.ns, self.nseg, 17).astype(np.int64)
        mx = self.d_max.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero(mx >= (1 << self.bits))
        if bad.size:
            s = int(bad[0])
            raise ValueError('the mosaic holds the code %d in tile %d (rows from %d, columns from %d): it does not fit bits = %d'
                             % (int(mx[s]), s, (s // self.nx) * self.th, (s % self.nx) * self.tw, self.bits))
        tot = h.sum(axis=1)
        tables, lens, self.headers, seen = np.zeros((self.ns, 17), dtype=np.uint32), np.zeros((self.ns, 17), dtype=np.int64), [], {}
        for s in range(self.ns):
            key = tot[s].tobytes()
            if key not in seen:
                counts, symbols = huffman_lengths(tot[s])
                seen[key] = (encoder_table(counts, symbols), ljpeg_header(self.bits, self.tw // 2, self.th, counts, symbols))
            tables[s], hd = seen[key]
            self.headers.append(hd)
            lens[s] = tables[s] >> 16
        seg_bit = np.zeros((self.ns, self.nseg + 1), dtype=np.int64)
        seg_bit[:, 1:] = np.cumsum((h * (lens + _EXTRA_BITS)[:, None, :]).sum(axis=2), axis=1)
        self.nraw = (seg_bit[:, -1] + 7) // 8                        # unstuffed bytes per stream; th * tw * 31 bits at most: below 2^29
        room = (self.nraw + 15) // 16 * 16                           # every stream starts on 16 bytes of the unstuffed buffer
        raw_off = np.concatenate([[0], np.cumsum(room)[:-1]])
        self.raw_bytes = int(room.sum())
        if self.raw_bytes >= 1 << 31:
            raise ValueError('the entropy-coded data takes %d bytes: more than 2^31' % self.raw_bytes)
        nch = -(-self.nraw // self.chunk)
        self.first_chunk = np.concatenate([[0], np.cumsum(nch)])
        sid = np.repeat(np.arange(self.ns), nch)
        j = np.arange(int(nch.sum())) - self.first_chunk[sid]
        ch = np.zeros(sid.size, dtype=L.DNG_ENC_CHUNK_DTYPE)
        ch['src'] = raw_off[sid] + j * self.chunk
        ch['nbytes'] = np.minimum(self.chunk, self.nraw[sid] - j * self.chunk)
        ch['dst'] = np.concatenate([[0], np.cumsum(self.nraw)[:-1]])[sid] + j * self.chunk
        self.nchunks = int(sid.size)
        self.d_tables, self.d_seg_bit = self._up(tables), self._up(seg_bit.astype(np.uint32))
        self.d_raw_dword, self.d_chunks = self._up((raw_off // 4).astype(np.uint32)), self._up(ch)
        self.d_last = self.torch.from_numpy(self.first_chunk[1:] - 1).to(self.dev)
        self.d_raw = self.torch.empty(self.raw_bytes // 4, dtype=self.torch.int32, device=self.dev)
        self.d_count = self.torch.empty(self.nchunks, dtype=self.torch.int32, device=self.dev)

    def pack(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_dng_enc_pack_u16(*self._geom(), L.dptr(self.d_tables), L.dptr(self.d_seg_bit), L.dptr(self.d_raw_dword),
                                                  L.dptr(self.d_raw), self.raw_bytes // 4, L.cur_stream()), 'eld_dng_enc_pack_u16')

    def ffcount(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_dng_enc_ffcount_u8(L.dptr(self.d_raw), self.raw_bytes, L.dptr(self.d_chunks), self.nchunks, self.chunk,
                                                    L.dptr(self.d_count), L.cur_stream()), 'eld_dng_enc_ffcount_u8')

    def sizes(self):
        """The running sum of the FF counts (device), then the one synchronisation: the stuffed size of every stream."""
        torch = self.torch
        cum = torch.cumsum(self.d_count, 0, dtype=torch.int32)
        self.d_before = (cum - self.d_count).contiguous()
        ends = cum[self.d_last].cpu().numpy().astype(np.int64)
        self.sizes_ = self.nraw + np.diff(np.concatenate([[0], ends]))
        self.out_bytes = int(self.sizes_.sum())
        if self.out_bytes >= 1 << 32:
            raise ValueError('the stuffed data takes %d bytes: more than 2^32' % self.out_bytes)
        self.d_out = torch.empty((self.out_bytes + 3) // 4 * 4, dtype=torch.uint8, device=self.dev)

    def stuff(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_dng_enc_stuff_u8(L.dptr(self.d_raw), self.raw_bytes, L.dptr(self.d_chunks), self.nchunks, self.chunk,
                                                  L.dptr(self.d_before), L.dptr(self.d_out), self.out_bytes, L.cur_stream()), 'eld_dng_enc_stuff_u8')

    def streams(self):
        """The one copy of the compressed bytes to the host -> the complete JPEG streams in TileOffsets order."""
        data = self.d_out.cpu().numpy()
        offs = np.concatenate([[0], np.cumsum(self.sizes_)])
        return [self.headers[s] + data[offs[s]:offs[s + 1]].tobytes() + b'\xff\xd9' for s in range(self.ns)]


def encode_ljpeg(mosaic, tile=DEFAULT_TILE, bits=16, segment=0, chunk=0):
    """`mosaic` ((H, W) uint16 codes: NumPy, uploaded; or a CUDA int16-view tensor, used in place) -> the complete lossless-JPEG streams of
    its tiles (list of bytes, rows of tiles, left to right): process 14, two components of TileWidth / 2 samples (Adobe's layout), precision
    `bits`, predictor 1, one Huffman table from the stream's own histogram.  Edge tiles are stored whole, padded by edge replication.
    segment (samples) and chunk (bytes) cut the work of the kernels, 0: the defaults; the bytes do not depend on them.  A code >= 2^bits is a
    ValueError that names the value and the tile."""
    e = Encoder(mosaic, tile, bits, segment, chunk)
    e.hist()
    e.plan()
    e.pack()
    e.ffcount()
    e.sizes()
    e.stuff()
    return e.streams()


def _serialise_ifd(tags, ifd_off):
    """One IFD at the even offset ifd_off, its out-of-line values behind it -> bytes of an even length"""
    order = sorted(tags)
    packed = {tag: _pack_entry(tags[tag]) for tag in order}
    data_off = ifd_off + 2 + 12 * len(order) + 4
    out, extra = bytearray(struct.pack('<H', len(order))), b''
    for tag in order:
        typ, cnt, payload = packed[tag]
        out += struct.pack('<HHI', tag, typ, cnt)
        if len(payload) <= 4:
            out += payload.ljust(4, b'\0')
        else:
            out += struct.pack('<I', data_off + len(extra))
            extra += payload + b'\0' * (len(payload) % 2)
    return bytes(out) + struct.pack('<I', 0) + extra


# with a preview these stay in IFD0; every other tag of the mosaic moves to the raw SubIFD
IFD0_LEVEL = (T_MAKE, T_MODEL, T_UNIQUEMODEL, T_COLORMATRIX1, T_COLORMATRIX2, T_ILLUMINANT1, T_ILLUMINANT2, T_ANALOGBALANCE, T_ASSHOTNEUTRAL,
              T_ISO, T_EXPOSURETIME, T_DNGVERSION, T_DNGBACKWARD, T_ORIENTATION)


def write_dng(path, mosaic, meta=None, like=None, rows_per_strip=None, compression=1, tile=None, bits=None, opcodes=None, preview=None):
    """Write `mosaic` ((H, W) uint16 codes, NumPy or a CUDA int16-view tensor) as a little-endian DNG with one IFD.  compression 1 (the
    default): uncompressed 16-bit strips.  compression 7: lossless-JPEG tiles of `tile` (TileLength, TileWidth; default 256 x 256) at `bits`
    (8..16, default 16) precision, encoded on the device (encode_ljpeg): a NumPy mosaic is uploaded, a device tensor is used where it is.
    like: a source DNG whose CFA, level, colour, neutral, make / model, ISO and exposure tags are copied with their original
    values (rationals stay the rationals they were; the mosaic is taken to be the source's visible mosaic, so no ActiveArea and no
    LinearizationTable are written).  meta: sidecar keys (cfa, raw_pattern, black_level, white_point, wb, ccm, iso, exposure_time, make, model);
    its tags are written from those values (ColorMatrix1 with CalibrationIlluminant1 = 21) and override what `like` gave.
    opcodes: {'OpcodeList1' | 'OpcodeList2' | 'OpcodeList3': bytes}, written as given (like= copies no opcode tag).
    preview: the bytes of a baseline YCbCr JPEG (eld_amd.jpeg.encode_jpeg of the render).  IFD0 then describes the preview (NewSubFileType 1,
    Compression 7, PhotometricInterpretation 6, one strip, its size and YCbCrSubSampling read from the stream's SOF0) and keeps the DNG
    version, camera and colour tags; the mosaic with its CFA, level and opcode tags moves to a SubIFD (NewSubFileType 0).  None: one IFD, the
    bytes of before."""
    if preview is not None:
        from .jpeg import jpeg_info
        try:
            pinfo = jpeg_info(preview)
        except ValueError as e:
            raise ValueError('preview: %s' % e)
        preview = bytes(preview)
    op_tags = {}
    for name, data in (opcodes or {}).items():
        tag = {n: t for t, n in OPCODE_TAGS}.get(name)
        if tag is None or not isinstance(data, (bytes, bytearray)) or len(data) < 4:
            raise ValueError('opcodes takes {tag name: bytes} with the names %s, got %r' % (', '.join(n for _, n in OPCODE_TAGS), name))
        op_tags[tag] = bytes(data)
    if compression not in (1, 7):
        raise ValueError('compression = %r: write_dng writes 1 (uncompressed) and 7 (lossless JPEG)' % (compression,))
    if compression == 7:
        if rows_per_strip:
            raise ValueError('rows_per_strip with compression = 7: lossless JPEG is written in tiles')
        tile, bits, _, _ = _check_encode_args(DEFAULT_TILE if tile is None else tile, 16 if bits is None else bits)
        _mosaic_shape(mosaic, 'write_dng')
    else:
        if tile is not None or bits is not None:
            raise ValueError('tile and bits belong to compression = 7; compression = 1 writes 16-bit strips')
        if not isinstance(mosaic, np.ndarray):
            mosaic = mosaic.detach().cpu().numpy()
        if mosaic.dtype == np.int16:
            mosaic = mosaic.view(np.uint16)
        if mosaic.dtype != np.uint16 or mosaic.ndim != 2 or mosaic.size == 0:
            raise ValueError('write_dng takes one (H, W) uint16 mosaic, got %s %s' % (mosaic.dtype, mosaic.shape))
    H, W = (int(v) for v in mosaic.shape)
    tags = {}

    def put(tag, typ, vals):
        tags[tag] = Entry(tag, typ, len(vals), vals)
    if like is not None:
        t, _ = parse_tiff(like)
        raw = _raw_ifd(t)
        for tag in COPIED_RAW:
            if tag in raw:
                tags[tag] = raw[tag]
        for tag in COPIED_IFD0:
            if tag in t.ifd0:
                tags[tag] = t.ifd0[tag]
        for tag in COPIED_EXIF:
            if tag in t.exif and tag not in tags:
                tags[tag] = t.exif[tag]
    m = dict(meta or {})
    cfa = m.get('cfa')
    if cfa is None and like is None:
        cfa = 'bayer'
    if cfa is not None or 'raw_pattern' in m:
        cfa = cfa or 'bayer'
        if cfa == 'bayer':
            pat = np.asarray(m.get('raw_pattern', ((0, 1), (3, 2)))).reshape(-1)
            if sorted(int(v) for v in pat) != [0, 1, 2, 3]:
                raise ValueError('raw_pattern must be a 2x2 permutation of the codes 0..3, got %r' % (m.get('raw_pattern'),))
            put(T_CFADIM, SHORT, (2, 2))
            put(T_CFAPATTERN, BYTE, tuple(1 if int(v) == 3 else int(v) for v in pat))
        elif cfa == 'xtrans':
            pat = np.asarray(m.get('raw_pattern', ())).reshape(-1)
            if pat.size != 36:
                raise ValueError('writing an X-Trans DNG needs the 6 x 6 raw_pattern in meta (or like= a DNG)')
            put(T_CFADIM, SHORT, (6, 6))
            put(T_CFAPATTERN, BYTE, tuple(1 if int(v) == 3 else int(v) for v in pat))
        else:
            raise ValueError("cfa must be 'bayer' or 'xtrans', got %r" % (cfa,))
        put(T_CFAPLANECOLOR, BYTE, (0, 1, 2))
    if 'black_level' in m and m['black_level'] is not None:
        b = np.asarray(m['black_level'], dtype=np.float64).reshape(-1)
        if T_CFADIM in tags and tuple(tags[T_CFADIM].values) == (2, 2) and b.size == 4:
            pat = tags[T_CFAPATTERN].values
            codes, greens = [], 0
            for v in pat:
                codes.append(v if v != 1 else (1 if greens == 0 else 3))
                greens += v == 1
            put(T_BLACKDIM, SHORT, (2, 2))
            put(T_BLACK, RATIONAL, tuple(_rational(float(b[c])) for c in codes))
        elif b.size == 1 or np.all(b == b[0]):
            put(T_BLACKDIM, SHORT, (1, 1))
            put(T_BLACK, RATIONAL, (_rational(float(b[0])),))
        else:
            raise ValueError('black_level takes 1 value, or 4 for Bayer, got %r' % (b.tolist(),))
    if m.get('white_point') is not None:
        put(T_WHITE, LONG, (int(m['white_point']),))
    if m.get('wb') is not None:
        w = [float(v) for v in np.asarray(m['wb'], dtype=np.float64).reshape(-1)[:3]]
        if len(w) != 3 or min(w) <= 0:
            raise ValueError('wb takes three positive values, got %r' % (m['wb'],))
        if max(w) / w[1] > 4000.0:
            raise ValueError('wb %r: a gain above 4000 times the green one does not fit a 32-bit rational' % (m['wb'],))
        # neutral = 1 / (gain over the green gain): the reciprocal of a rational with a denominator up to 10^6, so both halves fit 32 bits
        put(T_ASSHOTNEUTRAL, RATIONAL, tuple(_rational(1 / Fraction(v / w[1]).limit_denominator(1000000)) for v in w))
    if m.get('ccm') is not None:
        put(T_COLORMATRIX1, SRATIONAL, tuple(color_matrix_from_ccm(m['ccm'])))
        put(T_ILLUMINANT1, SHORT, (D65,))
        tags.pop(T_COLORMATRIX2, None)
        tags.pop(T_ILLUMINANT2, None)
    if m.get('iso') is not None:
        put(T_ISO, SHORT, (int(m['iso']),))
    if m.get('exposure_time') is not None:
        put(T_EXPOSURETIME, RATIONAL, (_rational(float(m['exposure_time'])),))
    for key, tag in (('make', T_MAKE), ('model', T_MODEL)):
        if m.get(key) is not None:
            tags[tag] = Entry(tag, ASCII, 0, str(m[key]))
    if T_CFADIM not in tags:
        raise ValueError('write_dng needs a CFA pattern: meta with cfa / raw_pattern, or like= a DNG')
    for tag, data in op_tags.items():
        tags[tag] = Entry(tag, UNDEFINED, len(data), data)
    put(T_NEWSUBFILETYPE, LONG, (0,))
    put(T_WIDTH, LONG, (W,))
    put(T_LENGTH, LONG, (H,))
    put(T_PHOTOMETRIC, SHORT, (CFA_PHOTOMETRIC,))
    put(T_SPP, SHORT, (1,))
    if compression == 7:                                            # every argument and tag has been checked: now the device
        streams = encode_ljpeg(mosaic, tile, bits)
        ns, T_OFFSETS = len(streams), T_TILEOFFSETS
        sizes = tuple(len(s) for s in streams)
        put(T_BITS, SHORT, (bits,))
        put(T_COMPRESSION, SHORT, (7,))
        put(T_TILEWIDTH, LONG, (tile[1],))
        put(T_TILELENGTH, LONG, (tile[0],))
        put(T_TILEBYTECOUNTS, LONG, sizes)
    else:
        rps = int(rows_per_strip) if rows_per_strip else max(1, min(H, (1 << 20) // (2 * W)))
        ns, T_OFFSETS = -(-H // rps), T_STRIPOFFSETS
        sizes = tuple(2 * W * min(rps, H - i * rps) for i in range(ns))
        put(T_BITS, SHORT, (16,))
        put(T_COMPRESSION, SHORT, (1,))
        put(T_ROWSPERSTRIP, LONG, (rps,))
        put(T_STRIPBYTECOUNTS, LONG, sizes)
    put(T_OFFSETS, LONG, (0,) * ns)                                 # patched below
    put(T_DNGVERSION, BYTE, (1, 4, 0, 0))
    put(T_DNGBACKWARD, BYTE, (1, 1, 0, 0))
    put(T_CFALAYOUT, SHORT, (1,))
    if T_UNIQUEMODEL not in tags:
        tags[T_UNIQUEMODEL] = Entry(T_UNIQUEMODEL, ASCII, 0, tags[T_MODEL].values if T_MODEL in tags else 'eld_amd')
    if preview is not None:
        top = {tag: tags.pop(tag) for tag in IFD0_LEVEL if tag in tags}
        for tag, typ, vals in ((T_NEWSUBFILETYPE, LONG, (1,)), (T_WIDTH, LONG, (pinfo['width'],)), (T_LENGTH, LONG, (pinfo['height'],)),
                               (T_BITS, SHORT, (8, 8, 8)), (T_COMPRESSION, SHORT, (7,)), (T_PHOTOMETRIC, SHORT, (YCBCR_PHOTOMETRIC,)),
                               (T_STRIPOFFSETS, LONG, (0,)), (T_SPP, SHORT, (3,)), (T_ROWSPERSTRIP, LONG, (pinfo['height'],)),
                               (T_STRIPBYTECOUNTS, LONG, (len(preview),)), (T_SUBIFDS, LONG, (0,)), (T_YCBCRSUBSAMPLING, SHORT, pinfo['subsampling'])):
            top[tag] = Entry(tag, typ, len(vals), vals)
        raw_off = 8 + len(_serialise_ifd(top, 8))                   # the offsets are LONGs: the sizes do not depend on their values
        prev_off = raw_off + len(_serialise_ifd(tags, raw_off))
        offs, pos = [], prev_off + len(preview) + len(preview) % 2
        for n in sizes:
            offs.append(pos)
            pos += n + n % 2
        if pos >= 1 << 32:
            raise ValueError('%s: %d bytes do not fit a classic TIFF' % (path, pos))
        top[T_SUBIFDS].values, top[T_STRIPOFFSETS].values, tags[T_OFFSETS].values = (raw_off,), (prev_off,), tuple(offs)
        with open(path, 'wb') as fh:
            fh.write(b'II' + struct.pack('<HI', 42, 8) + _serialise_ifd(top, 8) + _serialise_ifd(tags, raw_off) + preview + b'\0' * (len(preview) % 2))
            if compression == 7:
                for s in streams:
                    fh.write(s + b'\0' * (len(s) % 2))
            else:
                fh.write(np.ascontiguousarray(mosaic).astype('<u2', copy=False).tobytes())
        return
    order = sorted(tags)
    packed = {tag: _pack_entry(tags[tag]) for tag in order}
    ifd_off = 8
    data_off = ifd_off + 2 + 12 * len(order) + 4
    extra, where = b'', {}
    for tag in order:
        typ, cnt, payload = packed[tag]
        if len(payload) > 4:
            if len(extra) % 2:
                extra += b'\0'
            where[tag] = data_off + len(extra)
            extra += payload
    if len(extra) % 2:
        extra += b'\0'
    pix_off = data_off + len(extra)
    offs, pos = [], pix_off
    for n in sizes:                                                 # a compressed stream of odd length is followed by one byte of padding
        offs.append(pos)
        pos += n + n % 2
    if pos >= 1 << 32:
        raise ValueError('%s: %d bytes do not fit a classic TIFF' % (path, pos))
    packed[T_OFFSETS] = (LONG, ns, struct.pack('<%dI' % ns, *offs))
    if ns > 1:                                                      # the payload sits in `extra`: patch it in place
        a = where[T_OFFSETS] - data_off
        extra = extra[:a] + packed[T_OFFSETS][2] + extra[a + 4 * ns:]
    out = bytearray(b'II' + struct.pack('<HI', 42, ifd_off) + struct.pack('<H', len(order)))
    for tag in order:
        typ, cnt, payload = packed[tag]
        out += struct.pack('<HHI', tag, typ, cnt)
        out += payload.ljust(4, b'\0') if len(payload) <= 4 else struct.pack('<I', where[tag])
    out += struct.pack('<I', 0) + extra
    with open(path, 'wb') as fh:
        fh.write(out)
        if compression == 7:
            for s in streams:
                fh.write(s + b'\0' * (len(s) % 2))
        else:
            fh.write(np.ascontiguousarray(mosaic).astype('<u2', copy=False).tobytes())


# ---- command line -------------------------------------------------------------------------------------------------------------
def _apply_opcodes(a, mosaic, meta):
    """--opcodes apply: list 1's bad pixels repaired in `mosaic` (the project's own repair), the maps and the stage-2 image written where asked.
    -> (the repaired mosaic, one line per opcode, the tags of lists 2 and 3 for a .dng output: list 1 is applied, they are still to do)"""
    from . import dng_opcodes as O
    from .defects import repair
    lists = O.read_opcodes(a.input)
    Hm, Wm = (int(v) for v in mosaic.shape)
    dmap = O.defects_from_opcodes(lists[0], mosaic, meta, lists.linearization)
    if dmap.count:
        mosaic = repair(mosaic, dmap)
    lines = []
    for no, ops in enumerate(lists, 1):
        for i, op in enumerate(ops):
            d = O.disposition(op, no, lists.linearization)
            if d == 'never':
                what = 'never applied (warps and TrimBounds stay with the raw converter)'
            elif d == 'skip':
                what = 'skipped because optional (not supported in this list)'
            elif no == 1:
                what = 'applied: its sites are repaired (%d sites in all)' % dmap.count
            elif no == 3 or op.id in O.GAIN_IDS_2:
                what = 'folded into the lens plane' + ('' if a.flatfield_out else ' (--flatfield-out writes it)')
            else:
                what = 'applied in --linear-out' if a.linear_out else 'not applied: it changes the pixel values in front of the network (--linear-out applies it)'
            lines.append('%s: OpcodeList%d[%d] %s: %s' % (a.input, no, i, op.name, what))
    if a.defects_out:
        lines.append('%s -> %s (%d defective sites)' % (a.input, dmap.save(a.defects_out), dmap.count))
    if a.flatfield_out:
        ff = O.lens_from_opcodes(lists[1], lists[2], Hm, Wm, meta['cfa'], meta['raw_pattern'], min(int(meta['white_point']), 65535))
        lines.append('%s -> %s (lens gain %.4g .. %.4g)' % (a.input, ff.save(a.flatfield_out), float(ff.lens.min()), float(ff.lens.max())))
    if a.linear_out:
        lin = O.apply_list2(O.normalise(mosaic, meta), O.OpcodeProgram(lists[1], Hm, Wm))
        np.save(a.linear_out, lin.cpu().numpy())
        lines.append('%s -> %s (float32 stage 2)' % (a.input, a.linear_out))
    return mosaic, lines, {k: v for k, v in lists.raw.items() if k != 'OpcodeList1'}


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m eld_amd.dng', description='Convert a DNG to a uint16 mosaic (.npy) and a JSON sidecar.')
    ap.add_argument('input', help='a DNG file')
    ap.add_argument('-o', '--out', help='the mosaic (.npy), or a .dng: the visible mosaic re-written with the source\'s tags; default: the input '
                                        'name with .npy')
    ap.add_argument('--meta-out', help='the sidecar (.json) with the keys eld_amd.denoise --meta reads')
    ap.add_argument('--compression', choices=sorted(COMPRESSION_CHOICES), default='none', help='of a .dng output: uncompressed strips or '
                                                                                               'lossless-JPEG tiles (default: none)')
    ap.add_argument('--tile', type=int, nargs=2, metavar=('TH', 'TW'), help='TileLength TileWidth of --compression ljpeg (default 256 256)')
    ap.add_argument('--bits', type=int, help='the precision of --compression ljpeg, 8..16 (default 16)')
    ap.add_argument('--preview', metavar='FILE.jpg', help='of a .dng output: a baseline JPEG (python -m eld_amd.jpeg writes one) stored as the preview '
                                                          'in IFD0; the mosaic moves to a SubIFD')
    ap.add_argument('--opcodes', choices=('report', 'apply'), default='report',
                    help="OpcodeList1/2/3: 'report' names the lists present (the default); 'apply' repairs list 1's bad pixels in the -o output and "
                         'says what becomes of every opcode')
    ap.add_argument('--flatfield-out', metavar='FILE', help='with --opcodes apply: the gain opcodes of lists 2 and 3 as a flat-field map (.npz) whose '
                                                            'lens plane they fill, for --flatfield')
    ap.add_argument('--defects-out', metavar='FILE', help="with --opcodes apply: list 1's bad pixels as a defect map (.npz), for --defects")
    ap.add_argument('--linear-out', metavar='FILE', help='with --opcodes apply: the float32 stage-2 image (.npy): black / white normalisation, then '
                                                         'every list-2 opcode')
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if (a.flatfield_out or a.defects_out or a.linear_out) and a.opcodes != 'apply':
        ap.error('--flatfield-out, --defects-out and --linear-out belong to --opcodes apply')
    if (a.tile or a.bits) and a.compression != 'ljpeg':
        ap.error('--tile and --bits belong to --compression ljpeg')
    if a.compression == 'ljpeg' and not is_dng(a.out):
        ap.error('--compression ljpeg needs an -o that ends in .dng')
    if a.preview and not is_dng(a.out):
        ap.error('--preview needs an -o that ends in .dng')
    out = a.out or os.path.splitext(a.input)[0] + '.npy'
    lines, carried = [], None
    if is_dng(out):
        mosaic, meta = read_dng(a.input, device='cuda')
        if a.opcodes == 'apply':
            mosaic, lines, carried = _apply_opcodes(a, mosaic, meta)
        kw = dict(compression=7, tile=a.tile and tuple(a.tile), bits=a.bits) if a.compression == 'ljpeg' else {}
        if a.preview:
            with open(a.preview, 'rb') as fh:
                kw['preview'] = fh.read()
        write_dng(out, mosaic, like=a.input, opcodes=carried, **kw)
    else:
        mosaic, meta = read_dng(a.input)
        if a.opcodes == 'apply':
            mosaic, lines, _ = _apply_opcodes(a, mosaic, meta)
        np.save(out, mosaic)
    print('%s -> %s (%d x %d, %s, %d bits, compression %d)' % (a.input, out, mosaic.shape[0], mosaic.shape[1], meta['cfa'], meta['bits'], meta['compression']))
    for line in lines:
        print(line)
    if meta['opcodes'] and a.opcodes == 'report':
        print('%s: %s present and not applied (gain maps, defect lists and warps stay with the raw converter)' % (a.input, ', '.join(meta['opcodes'])))
    if a.meta_out:
        from .denoise import SIDECAR_KEYS
        side = {k: v for k, v in meta.items() if k in SIDECAR_KEYS}
        if meta['cfa'] == 'xtrans':
            side.pop('raw_pattern', None)                           # the X-Trans layout is fixed in this project; the sidecar's raw_pattern is Bayer's
        with open(a.meta_out, 'w') as fh:
            json.dump(side, fh, indent=1)
        print('%s -> %s' % (a.input, a.meta_out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
