"""The yardstick of the DNG reader (eld_amd/dng.py, csrc/dng.hip), in NumPy and plain Python, from the specifications (TIFF 6.0, DNG 1.x,
ITU-T T.81 Annexes C, F, H and K):

    write_dng_file   a TIFF / DNG writer: both byte orders, strips and tiles, the raw IFD in IFD0 or in a SubIFD behind a thumbnail, packed
                     8 / 10 / 12 / 14 / 16-bit rows, lossless-JPEG tiles; arbitrary extra tags
    ljpeg_encode     a lossless-JPEG (process 14) encoder, vectorised per stream: any precision <= 16, 1..4 components, predictors 1..7, a
                     Huffman table from the stream's own symbol histogram (Annex K.2), one table per component on request
    ljpeg_decode     a decoder that shares no code with the encoder: it walks the markers itself, reads the stream a bit at a time through
                     Annex F's DECODE / RECEIVE / EXTEND and predicts sample by sample in Python integers
    ref_read         the visible mosaic of a file written here, decoded from its streams by ljpeg_decode / unpack_rows
    ccm_formula      the float64 colour-matrix formula of the metadata mapping, restated
Nothing here imports eld_amd."""
import struct

import numpy as np

SRGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]], dtype=np.float64)
BYTE, ASCII, SHORT, LONG, RATIONAL, UNDEFINED, SRATIONAL, FLOAT = 1, 2, 3, 4, 5, 7, 10, 11
_FMT = {BYTE: 'B', SHORT: 'H', LONG: 'I', UNDEFINED: 'B', FLOAT: 'f', 8: 'h', 9: 'i', 13: 'I'}


def ccm_formula(color_matrix):
    cam = np.asarray(color_matrix, dtype=np.float64).reshape(3, 3) @ SRGB_TO_XYZ
    cam = cam / cam.sum(axis=1, keepdims=True)
    return np.linalg.inv(cam)


# ---- Huffman tables (Annex C, K.2) -------------------------------------------------------------------------------------------------
def code_lengths(hist):
    """Symbol histogram (17 counts) -> (bits[1..16] as a list of 16, huffval): Annex K.2 with the reserved all-ones code point, lengths
    limited to 16 as Figure K.3."""
    freq = [int(v) for v in hist] + [1]                            # the last entry reserves the all-ones code
    n = len(freq)
    codesize, others = [0] * n, [-1] * n
    while True:
        c1 = c2 = -1
        for i in range(n):
            if freq[i] and (c1 < 0 or freq[i] <= freq[c1]):
                c1 = i
        for i in range(n):
            if freq[i] and i != c1 and (c2 < 0 or freq[i] <= freq[c2]):
                c2 = i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 34
    for i in range(n):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                    # the reserved code point
    huffval = [s for l in range(1, 33) for s in range(n - 1) if codesize[s] == l]
    return bits[1:17], huffval


def deep_lengths(hist):
    """A valid table with three 16-bit codes whatever the histogram: all 17 symbols by falling count, lengths 1..14 and 16, 16, 16 (the Kraft sum
    is 1 - 2^-16: the all-ones code stays free)."""
    order = sorted(range(17), key=lambda s: (-int(hist[s]), s))
    bits = [1] * 14 + [0, 3]
    return bits, order


def canonical_codes(bits, huffval):
    """-> {symbol: (code, length)} (Annex C)"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[huffval[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- encoder ----------------------------------------------------------------------------------------------------------------------
def _predict(S, P, pred):
    """S: (Y, X, Nf) int64 samples -> the predictions, same shape"""
    px = np.empty_like(S)
    px[0, 0] = 1 << (P - 1)
    px[0, 1:] = S[0, :-1]
    px[1:, 0] = S[:-1, 0]
    ra, rb, rc = S[1:, :-1], S[:-1, 1:], S[:-1, :-1]
    px[1:, 1:] = {1: ra, 2: rb, 3: rc, 4: ra + rb - rc, 5: ra + ((rb - rc) >> 1), 6: rb + ((ra - rc) >> 1), 7: (ra + rb) >> 1}[pred]
    return px


def ljpeg_encode(samples, P, X, Y, Nf, pred=1, per_component=False, deep=False, point_transform=0, restart_interval=0, scans=None):
    """samples: the stream's sample sequence (any shape, X * Y * Nf values below 65536) -> (bytes, info).  info: tables (bits, huffval) per
    component, stuffed: the number of FF 00 pairs in the entropy data."""
    S = np.asarray(samples, dtype=np.int64).reshape(Y, X, Nf)
    d = (S - _predict(S, P, pred)) & 0xFFFF
    d = np.where(d >= 32768, d - 65536, d)                         # -32768 .. 32767
    a = np.abs(d)
    ssss = np.zeros(d.shape, dtype=np.int64)
    for s in range(1, 17):
        ssss[a >= (1 << (s - 1))] = s
    extra = np.where(d < 0, d + (1 << ssss) - 1, d)
    extra[ssss == 16] = 0
    nextra = np.where(ssss == 16, 0, ssss)
    groups = [[k] for k in range(Nf)] if per_component else [list(range(Nf))]
    tables, code = [None] * Nf, np.zeros(d.shape, dtype=np.int64)
    clen = np.zeros(d.shape, dtype=np.int64)
    dht = b''
    for ti, comps in enumerate(groups):
        hist = np.bincount(ssss[:, :, comps].reshape(-1), minlength=17)
        bits, vals = deep_lengths(hist) if deep else code_lengths(hist)
        cc = canonical_codes(bits, vals)
        lut_c, lut_l = np.zeros(17, dtype=np.int64), np.zeros(17, dtype=np.int64)
        for s, (c, l) in cc.items():
            lut_c[s], lut_l[s] = c, l
        for k in comps:
            tables[k] = (bits, vals)
            code[:, :, k] = lut_c[ssss[:, :, k]]
            clen[:, :, k] = lut_l[ssss[:, :, k]]
        body = bytes([ti]) + bytes(bits) + bytes(vals)
        dht += b'\xff\xc4' + struct.pack('>H', 2 + len(body)) + body
    word = ((code << nextra) | extra).reshape(-1)
    nb = (clen + nextra).reshape(-1)                                # <= 32
    word = word << (32 - nb)
    m = ((word[:, None] >> (31 - np.arange(32))) & 1).astype(np.uint8)
    flat = m[np.arange(32)[None, :] < nb[:, None]]
    flat = np.concatenate([flat, np.ones((-flat.size) % 8, dtype=np.uint8)])
    raw = np.packbits(flat)
    ff = np.flatnonzero(raw == 0xFF)
    ent = np.insert(raw, ff + 1, 0).tobytes()
    sof = struct.pack('>BHHB', P, Y, X, Nf) + b''.join(bytes([k + 1, 0x11, 0]) for k in range(Nf))
    ns = Nf if scans is None else scans
    sos = bytes([ns]) + b''.join(bytes([k + 1, ((k if per_component else 0) << 4)]) for k in range(ns)) + bytes([pred, 0, point_transform])
    out = b'\xff\xd8' + b'\xff\xc3' + struct.pack('>H', 2 + len(sof)) + sof + dht
    if restart_interval:
        out += b'\xff\xdd' + struct.pack('>HH', 4, restart_interval)
    out += b'\xff\xda' + struct.pack('>H', 2 + len(sos)) + sos
    header_len = len(out)
    out += ent + b'\xff\xd9'
    return out, {'tables': tables, 'stuffed': int(ff.size), 'header_len': header_len, 'max_code_len': max(max(l for _, l in canonical_codes(*t).values()) for t in tables)}


# ---- decoder (shares nothing with the encoder) ------------------------------------------------------------------------------------
class _BitReader:
    def __init__(self, data, pos):
        self.d, self.pos, self.cnt, self.b = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            if self.pos >= len(self.d):
                raise ValueError('truncated')
            self.b = self.d[self.pos]
            self.pos += 1
            if self.b == 0xFF:
                if self.pos >= len(self.d) or self.d[self.pos] != 0:
                    raise ValueError('truncated')                   # a marker where data was expected
                self.pos += 1
            self.cnt = 8
        self.cnt -= 1
        return (self.b >> self.cnt) & 1


def ljpeg_decode(data):
    """One lossless-JPEG stream -> (the sample sequence as a flat uint16 array of X * Y * Nf values, dict(P, X, Y, Nf, pred)).  Raises
    ValueError('truncated' | 'invalid code') on a stream that ends early or holds bits outside its table."""
    assert data[:2] == b'\xff\xd8'
    pos, dht, frame = 2, {}, None
    while True:
        assert data[pos] == 0xFF
        mk = data[pos + 1]
        ln = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + ln]
        pos += 2 + ln
        if mk == 0xC3:
            P, Y, X, Nf = struct.unpack('>BHHB', seg[:6])
            frame = (P, Y, X, Nf)
        elif mk == 0xC4:
            q = 0
            while q < len(seg):
                th = seg[q] & 15
                bits = list(seg[q + 1:q + 17])
                n = sum(bits)
                vals = list(seg[q + 17:q + 17 + n])
                q += 17 + n
                mincode, maxcode, valptr, code, k = [0] * 17, [-1] * 17, [0] * 17, 0, 0
                for l in range(1, 17):
                    if bits[l - 1]:
                        valptr[l], mincode[l] = k, code
                        code += bits[l - 1]
                        k += bits[l - 1]
                        maxcode[l] = code - 1
                    code <<= 1
                dht[th] = (mincode, maxcode, valptr, vals)
        elif mk == 0xDA:
            ns = seg[0]
            sel = [seg[2 + 2 * k] >> 4 for k in range(ns)]
            pred = seg[1 + 2 * ns]
            break
    P, Y, X, Nf = frame
    br = _BitReader(data, pos)
    out = [[[0] * Nf for _ in range(X)] for _ in range(Y)]
    for y in range(Y):
        for x in range(X):
            for k in range(Nf):
                mincode, maxcode, valptr, vals = dht[sel[k]]
                code, l = br.bit(), 1
                while code > maxcode[l]:
                    l += 1
                    if l > 16:
                        raise ValueError('invalid code')
                    code = (code << 1) | br.bit()
                t = vals[valptr[l] + code - mincode[l]]
                if t == 0:
                    diff = 0
                elif t == 16:
                    diff = 32768
                else:
                    v = 0
                    for _ in range(t):
                        v = (v << 1) | br.bit()
                    diff = v if v >= (1 << (t - 1)) else v - (1 << t) + 1
                if y == 0:
                    px = (1 << (P - 1)) if x == 0 else out[0][x - 1][k]
                elif x == 0:
                    px = out[y - 1][0][k]
                else:
                    ra, rb, rc = out[y][x - 1][k], out[y - 1][x][k], out[y - 1][x - 1][k]
                    px = (ra, rb, rc, ra + rb - rc, ra + ((rb - rc) >> 1), rb + ((ra - rc) >> 1), (ra + rb) >> 1)[pred - 1]
                out[y][x][k] = (px + diff) & 0xFFFF
    return np.array(out, dtype=np.uint16).reshape(-1), {'P': P, 'X': X, 'Y': Y, 'Nf': Nf, 'pred': pred}


# ---- packed rows ------------------------------------------------------------------------------------------------------------------
def pack_rows(tile, bits, order='<'):
    """(th, tw) uint16 -> bytes: each row MSB-first at `bits` per sample, padded to a byte; 16-bit samples in the file's byte order."""
    tile = np.asarray(tile, dtype=np.uint16)
    if bits == 16:
        return tile.astype(order + 'u2').tobytes()
    b = np.unpackbits(tile.astype('>u2').view(np.uint8).reshape(tile.shape[0], tile.shape[1], 2), axis=2)[:, :, 16 - bits:]
    b = b.reshape(tile.shape[0], -1)
    b = np.concatenate([b, np.zeros((b.shape[0], (-b.shape[1]) % 8), dtype=np.uint8)], axis=1)
    return np.packbits(b, axis=1).tobytes()


def unpack_rows(data, th, tw, bits, order='<'):
    """the inverse, through Python integers: one big integer per row"""
    rb = (tw * bits + 7) // 8
    out = np.zeros((th, tw), dtype=np.uint16)
    for r in range(th):
        row = data[r * rb:(r + 1) * rb]
        if bits == 16:
            out[r] = np.frombuffer(row, dtype=order + 'u2')
            continue
        big = int.from_bytes(row, 'big')
        for c in range(tw):
            out[r, c] = (big >> (rb * 8 - bits * (c + 1))) & ((1 << bits) - 1)
    return out


# ---- the file writer ----------------------------------------------------------------------------------------------------------------
def _payload(typ, vals, order):
    if typ == ASCII:
        b = (vals if isinstance(vals, bytes) else vals.encode('latin-1')) + b'\0'
        return len(b), b
    if typ in (RATIONAL, SRATIONAL):
        flat = [int(x) for pr in vals for x in pr]
        return len(vals), struct.pack(order + '%d%s' % (len(flat), 'I' if typ == RATIONAL else 'i'), *flat)
    if isinstance(vals, bytes):
        return len(vals), vals
    return len(vals), struct.pack(order + '%d%s' % (len(vals), _FMT[typ]), *vals)


def _emit_ifd(buf, tags, order):
    """append the IFD's out-of-line values, then the IFD itself; -> the IFD's offset"""
    entries = []
    for tag in sorted(tags):
        typ, vals = tags[tag]
        cnt, pl = _payload(typ, vals, order)
        if len(pl) > 4:
            if len(buf) % 2:
                buf += b'\0'
            off = len(buf)
            buf += pl
            pl = struct.pack(order + 'I', off)
        entries.append(struct.pack(order + 'HHI', tag, typ, cnt) + pl.ljust(4, b'\0'))
    if len(buf) % 2:
        buf += b'\0'
    off = len(buf)
    buf += struct.pack(order + 'H', len(entries)) + b''.join(entries) + struct.pack(order + 'I', 0)
    return off


def tile_sequences(tile, geometry):
    """The JPEG geometry of one stored tile (th, tw): -> (X, Y, Nf).  The sample sequence is the tile's raster order in every geometry."""
    th, tw = tile.shape
    if geometry == 'nf1':
        return tw, th, 1
    if geometry == 'nf2':                                           # Adobe's layout: two components, half the width
        assert tw % 2 == 0
        return tw // 2, th, 2
    if geometry == 'rowdouble':                                     # two tile rows per JPEG line
        assert th % 2 == 0
        return tw, th // 2, 2
    raise ValueError(geometry)


def write_dng_file(path, image, order='<', bits=16, compression=1, tile=None, rows_per_strip=None, subifd=False, tags=None, tags0=None, exif=None,
                   ljpeg=None, mutate=None, cfa=(0, 1, 1, 2), cfa_dim=(2, 2), photometric=32803, magic=42):
    """Write `image` ((H, W) uint16, the FULL image) as a DNG.  tile: (TileLength, TileWidth) or None for strips of rows_per_strip rows.
    compression 1: rows packed at `bits`; 7: lossless JPEG with ljpeg = dict(P, geometry, pred, per_component, deep, ...ljpeg_encode's
    switches).  Edge tiles are stored whole, padded by edge replication.  tags / tags0 / exif: {tag: (type, values)} added to the raw IFD /
    IFD0 / an Exif IFD.  subifd: IFD0 is an 8-bit RGB thumbnail and the raw IFD sits in SubIFDs.  mutate(streams) -> streams edits the encoded
    streams before they are written.  -> info: the streams, their geometry and the encoder's notes, for ref_read and the tests."""
    image = np.asarray(image, dtype=np.uint16)
    H, W = image.shape
    if tile is not None:
        th, tw = tile
        geo = [(x0, y0, tw, th) for y0 in range(0, H, th) for x0 in range(0, W, tw)]
    else:
        rps = rows_per_strip or H
        geo = [(0, y0, W, min(rps, H - y0)) for y0 in range(0, H, rps)]
    streams, notes = [], []
    for x0, y0, w_, h_ in geo:
        t = image[y0:y0 + h_, x0:x0 + w_]
        t = np.pad(t, ((0, h_ - t.shape[0]), (0, w_ - t.shape[1])), mode='edge')
        if compression == 7:
            lj = dict(ljpeg or {})
            P, geometry = lj.pop('P', bits), lj.pop('geometry', 'nf1')
            X, Y, Nf = tile_sequences(t, geometry)
            data, note = ljpeg_encode(t.reshape(-1), P, X, Y, Nf, **lj)
            notes.append(note)
        else:
            data = pack_rows(t, bits, order)
        streams.append(data)
    if mutate is not None:
        streams = mutate(list(streams))
    buf = bytearray(order.replace('<', 'II').replace('>', 'MM').encode() + struct.pack(order + 'HI', magic, 0))
    offs = []
    for s in streams:
        offs.append(len(buf))
        buf += s
    raw = {254: (LONG, (0,)), 256: (LONG, (W,)), 257: (LONG, (H,)), 258: (SHORT, (bits,)), 259: (SHORT, (compression,)),
           262: (SHORT, (photometric,)), 277: (SHORT, (1,)), 33421: (SHORT, tuple(cfa_dim)), 33422: (BYTE, tuple(cfa))}
    if tile is not None:
        raw.update({322: (LONG, (tw,)), 323: (LONG, (th,)), 324: (LONG, tuple(offs)), 325: (LONG, tuple(len(s) for s in streams))})
    else:
        raw.update({273: (LONG, tuple(offs)), 278: (LONG, (rps,)), 279: (LONG, tuple(len(s) for s in streams))})
    raw.update(tags or {})
    raw = {k: v for k, v in raw.items() if v is not None}
    top = dict(tags0 or {})
    top[50706] = (BYTE, (1, 4, 0, 0))
    if exif:
        top[34665] = (LONG, (_emit_ifd(buf, exif, order),))
    if subifd:
        thumb = bytes(range(48))                                    # 4 x 4 RGB
        toff = len(buf)
        buf += thumb
        sub = _emit_ifd(buf, raw, order)
        top.update({254: (LONG, (1,)), 256: (LONG, (4,)), 257: (LONG, (4,)), 258: (SHORT, (8, 8, 8)), 259: (SHORT, (1,)), 262: (SHORT, (2,)),
                    273: (LONG, (toff,)), 277: (SHORT, (3,)), 278: (LONG, (4,)), 279: (LONG, (48,)), 330: (LONG, (sub,))})
    else:
        top.update(raw)
    ifd0 = _emit_ifd(buf, top, order)
    buf[4:8] = struct.pack(order + 'I', ifd0)
    with open(path, 'wb') as fh:
        fh.write(buf)
    return {'path': str(path), 'H': H, 'W': W, 'bits': bits, 'compression': compression, 'order': order, 'geo': geo, 'streams': streams, 'offsets': offs,
            'notes': notes, 'tags': raw}


def ref_read(info, active_area=None, lin=None):
    """The visible mosaic of a file written by write_dng_file, decoded from info['streams'] by this module's decoders."""
    H, W = info['H'], info['W']
    full = np.zeros((H, W), dtype=np.uint16)
    for data, (x0, y0, w_, h_) in zip(info['streams'], info['geo']):
        if info['compression'] == 7:
            seq, _ = ljpeg_decode(data)
            t = seq.reshape(h_, w_)
        else:
            t = unpack_rows(data, h_, w_, info['bits'], info['order'])
        full[y0:y0 + h_, x0:x0 + w_] = t[:H - y0, :W - x0]
    if lin is not None:
        lin = np.asarray(lin, dtype=np.uint16)
        full = lin[np.minimum(full, lin.size - 1)]
    if active_area is not None:
        t_, l_, b_, r_ = active_area
        full = full[t_:b_, l_:r_]
    return np.ascontiguousarray(full)


# ---- content ----------------------------------------------------------------------------------------------------------------------
def noisy_ramp(H, W, P, seed=0):
    """a ramp over the code range with noise of several widths, a few extreme jumps (the long codes) and the values 0 and 2^P - 1"""
    rng = np.random.default_rng(seed)
    top = (1 << P) - 1
    y, x = np.mgrid[0:H, 0:W]
    v = (x * top // max(W - 1, 1) + y * 3).astype(np.float64) + rng.normal(0, 1 + top / 64.0, (H, W)) * (rng.random((H, W)) < 0.7)
    v = np.clip(np.rint(v), 0, top).astype(np.uint16)
    idx = rng.integers(0, H * W, size=max(4, H * W // 50))
    v.reshape(-1)[idx] = rng.choice([0, top, top // 2, 1], size=idx.size)
    return v


def alternating(H, W, a, b):
    """sample i of the raster is a for even i, b for odd i"""
    v = np.where(np.arange(H * W) % 2 == 0, a, b).astype(np.uint16)
    return v.reshape(H, W)
