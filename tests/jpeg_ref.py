"""The yardstick of the baseline-JPEG writer (eld_amd/jpeg.py, csrc/jpeg.hip), in NumPy integers, and a decoder that shares
no code with it.  Plain module: no fixture, no pytest setting.

    encode(rgb, quality, subsampling, info=None) -> bytes     the whole JFIF file; info (a dict) receives what the cases assert on
    coefficients(rgb, quality, subsampling) -> (nblocks, 64) int16, zigzag order, blocks in scan order, dummy blocks included
    decode(data) -> dict                                      marker parse, Huffman, unstuffing, down to the same (nblocks, 64) array
    cases() -> [Case]                                         the pictures of the tests; Case.check(info) asserts what the case is there for

The rules are libjpeg's (IJG release 6b; libjpeg-turbo computes the same integers): its colour conversion, its h2v2 downsampler, its "slow
integer" forward DCT, its quantiser, its dummy blocks and its optimal Huffman tables (Annex K.2).  test_jpeg_cpu.py pins this module to the
coefficients read out of Pillow-written files."""
import struct

import numpy as np

K1_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K1_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
SUBSAMPLING = {'444': 0, '420': 2}                                   # the names and Pillow's numbers


def zigzag():
    """natural index (8 * row + column) of zigzag position k, walked along the anti-diagonals"""
    out = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]     # (row, column), row ascending
        out += [8 * r + c for r, c in (cells if s % 2 else cells[::-1])]
    return out


ZZ = zigzag()


def quant_tables(quality):
    """-> (luma, chroma): 64 values each in natural order"""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((t * scale + 50) // 100, 1), 255) for t in tab] for tab in (K1_LUMA, K1_CHROMA))


def geometry(H, W, sub):
    """-> MCU height and width in pixels, MCU rows and columns, blocks per MCU"""
    mh = mw = 16 if sub == '420' else 8
    return mh, mw, -(-H // mh), -(-W // mw), 6 if sub == '420' else 3


def component_planes(rgb, sub):
    """(H, W, 3) uint8 -> [Y, Cb, Cr] as int64 planes of whole MCUs"""
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and sub in SUBSAMPLING
    H, W = rgb.shape[:2]
    mh, mw, my, mx, _ = geometry(H, W, sub)
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16

    def extend(p, h, w):
        return p[np.minimum(np.arange(h), p.shape[0] - 1)][:, np.minimum(np.arange(w), p.shape[1] - 1)]
    if sub == '444':
        return [extend(p, my * mh, mx * mw) for p in (Y, Cb, Cr)]
    out = [extend(Y, my * mh, mx * mw)]
    for p in (Cb, Cr):
        p = extend(p, 2 * (-(-H // 2)), mx * mw)                     # the rows to an even count, the columns to whole blocks of the output
        bias = np.tile([1, 2], p.shape[1] // 4)
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(extend(d, my * 8, mx * 8))
    return out


F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819, f2562=20995,
         f3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of jfdctint over the last axis of d (..., 8)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = np.empty_like(d)
    o[..., 0] = (t10 + t11) * 4 if first else _descale(t10 + t11, 2)
    o[..., 4] = (t10 - t11) * 4 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F['f0541']
    o[..., 2] = _descale(z1 + t13 * F['f0765'], n)
    o[..., 6] = _descale(z1 - t12 * F['f1847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F['f1175']
    t4, t5, t6, t7 = t4 * F['f0298'], t5 * F['f2053'], t6 * F['f3072'], t7 * F['f1501']
    z1, z2, z3, z4 = -z1 * F['f0899'], -z2 * F['f2562'], -z3 * F['f1961'] + z5, -z4 * F['f0390'] + z5
    o[..., 7] = _descale(t4 + z1 + z3, n)
    o[..., 5] = _descale(t5 + z2 + z4, n)
    o[..., 3] = _descale(t6 + z2 + z3, n)
    o[..., 1] = _descale(t7 + z1 + z4, n)
    return o


def plane_blocks(p, q):
    """a plane of whole blocks -> (rows of blocks, columns of blocks, 64) quantised coefficients in natural order"""
    h, w = p.shape
    b = (p - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)        # (by, bx, row, column)
    c = _pass(_pass(b, True).swapaxes(-1, -2), False).swapaxes(-1, -2).reshape(h // 8, w // 8, 64)
    qv = 8 * np.asarray(q, dtype=np.int64)
    return np.sign(c) * ((np.abs(c) + (qv >> 1)) // qv)


def coefficients(rgb, quality=90, subsampling='420'):
    H, W = rgb.shape[:2]
    mh, mw, my, mx, bpm = geometry(H, W, subsampling)
    ql, qc = quant_tables(quality)
    Y, Cb, Cr = (plane_blocks(p, q) for p, q in zip(component_planes(rgb, subsampling), (ql, qc, qc)))
    out = np.zeros((my * mx, bpm, 64), dtype=np.int64)
    zz = np.array(ZZ)
    n = mh // 8                                                       # Y blocks per MCU side
    realh, realw = -(-H // 8), -(-W // 8)
    for k in range(n * n):
        r, c = k // n, k % n
        out[:, k] = Y[r::n, c::n].reshape(my * mx, 64)[:, zz]
    if n == 2:                                                        # libjpeg's dummy blocks: no AC, the DC of a neighbour
        for m in range(my * mx):
            y, x = divmod(m, mx)
            right, below = 2 * x + 1 >= realw, 2 * y + 1 >= realh
            if right:
                out[m, 1] = 0
                out[m, 1, 0] = out[m, 0, 0]
            for k in (2, 3):
                if below:
                    out[m, k] = 0
                    out[m, k, 0] = out[m, 1, 0]
                elif k == 3 and right:
                    out[m, 3] = 0
                    out[m, 3, 0] = out[m, 2, 0]
    out[:, bpm - 2] = Cb.reshape(my * mx, 64)[:, zz]
    out[:, bpm - 1] = Cr.reshape(my * mx, 64)[:, zz]
    return out.reshape(-1, 64).astype(np.int16)


# ---- Annex K.2, as libjpeg's jpeg_gen_optimal_table walks it ---------------------------------------------------------------------------
def optimal_table(freq):
    """histogram -> (the 16 counts of the code lengths, the symbols in code order)"""
    freq = [int(v) for v in freq] + [1]                              # the reserved symbol keeps the all-ones code free
    n = len(freq)
    codesize, others = [0] * n, [-1] * n
    while True:
        c1, v = -1, None
        for i in range(n):
            if freq[i] and (v is None or freq[i] <= v):
                c1, v = i, freq[i]
        c2, v = -1, None
        for i in range(n):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                c2, v = i, freq[i]
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
    bits = [0] * 64
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(63, 16, -1):
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
    bits[i] -= 1
    vals = [s for l in range(1, 64) for s in range(n - 1) if codesize[s] == l]
    return bits[1:17], vals


def canonical(bits, vals):
    """-> {symbol: (code, length)}"""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _size(v):
    return int(abs(int(v))).bit_length()


def block_symbols(blk, pred):
    """one block (zigzag order) -> [(table class 0 DC / 1 AC, symbol, extra bits, how many)]"""
    out = []
    d = int(blk[0]) - pred
    s = _size(d)
    assert s <= 11
    out.append((0, s, (d if d >= 0 else d - 1) & ((1 << s) - 1), s))
    run = 0
    for k in range(1, 64):
        v = int(blk[k])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        s = _size(v)
        assert 1 <= s <= 10
        out.append((1, (run << 4) | s, (v if v >= 0 else v - 1) & ((1 << s) - 1), s))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def header(H, W, sub, ql, qc, tables):
    """SOI .. SOS; tables: [(bits, vals)] for DC0, AC0, DC1, AC1"""
    def seg(marker, body):
        return bytes([0xFF, marker]) + struct.pack('>H', 2 + len(body)) + body
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate((ql, qc)):
        out += seg(0xDB, bytes([i]) + bytes(q[ZZ[k]] for k in range(64)))
    hv = 0x22 if sub == '420' else 0x11
    out += seg(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (bits, vals), tc_th in zip(tables, (0x00, 0x10, 0x01, 0x11)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def deep_tables(hist):
    """every symbol in use gets a 16-bit code: no table an encoder would choose, the longest words it could ever meet"""
    return [([0] * 15 + [sum(1 for v in h if v)], [s for s, v in enumerate(h) if v]) for h in hist]


def encode(rgb, quality=90, subsampling='420', info=None, deep=False):
    rgb = np.ascontiguousarray(rgb)
    H, W = rgb.shape[:2]
    bpm = geometry(H, W, subsampling)[4]
    co = coefficients(rgb, quality, subsampling)
    comp = [0] * (bpm - 2) + [1, 2]
    pred, syms = [0, 0, 0], []
    hist = [[0] * 12, [0] * 256, [0] * 12, [0] * 256]               # DC0, AC0, DC1, AC1
    for b in range(co.shape[0]):
        c = comp[b % bpm]
        bs = block_symbols(co[b], pred[c])
        pred[c] = int(co[b, 0])
        t = 0 if c == 0 else 2
        for cls, sym, _, _ in bs:
            hist[t + cls][sym] += 1
        syms.append((t, bs))
    tables = deep_tables(hist) if deep else [optimal_table(h) for h in hist]
    codes = [canonical(*t) for t in tables]
    acc, nbits, starts = 0, 0, []
    for t, bs in syms:
        starts.append(nbits)
        for cls, sym, extra, ne in bs:
            code, length = codes[t + cls][sym]
            acc = (acc << (length + ne)) | (code << ne) | extra
            nbits += length + ne
    pad = -nbits % 8
    acc = (acc << pad) | ((1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, 'big')
    ql, qc = quant_tables(quality)
    if info is not None:
        info.update(coef=co, hist=hist, tables=tables, starts=starts, nbits=nbits, stuffed=raw.count(b'\xff'), blocks=co.shape[0],
                    symbols=[bs for _, bs in syms], bpm=bpm)
    return header(H, W, subsampling, ql, qc, tables) + raw.replace(b'\xff', b'\xff\x00') + b'\xff\xd9'


# ---- the decoder: marker parse, Huffman, unstuffing; bit by bit ------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data, pos):
        self.d, self.p, self.cur, self.left = data, pos, 0, 0

    def bit(self):
        if self.left == 0:
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                nxt = self.d[self.p]
                if nxt != 0:
                    raise ValueError('marker FF%02X inside the entropy-coded data at byte %d' % (nxt, self.p - 1))
                self.p += 1
            self.cur, self.left = b, 8
        self.left -= 1
        return (self.cur >> self.left) & 1

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v


def _decode_symbol(br, lookup):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.bit()
        if (length, code) in lookup:
            return lookup[(length, code)]
    raise ValueError('16 bits that are no code of the table')


def _extend(v, s):
    return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1


def decode(data):
    """a baseline JFIF file -> dict(H, W, subsampling, qtables {id: 64 natural}, coef (nblocks, 64) zigzag in scan order, markers, tables)"""
    if data[:2] != b'\xff\xd8':
        raise ValueError('no SOI')
    pos, q, huff, frame, markers = 2, {}, {}, None, ['SOI']
    while True:
        if data[pos] != 0xFF:
            raise ValueError('no marker at byte %d' % pos)
        m = data[pos + 1]
        n, = struct.unpack_from('>H', data, pos + 2)
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        markers.append({0xE0: 'APP0', 0xDB: 'DQT', 0xC0: 'SOF0', 0xC4: 'DHT', 0xDA: 'SOS'}.get(m, 'FF%02X' % m))
        if m == 0xDB:
            i = 0
            while i < len(body):
                pq, tq = body[i] >> 4, body[i] & 15
                if pq:
                    raise ValueError('a 16-bit quantisation table')
                nat = [0] * 64
                for k in range(64):
                    nat[_DEC_ZZ[k]] = body[i + 1 + k]
                q[tq] = nat
                i += 65
        elif m == 0xC0:
            P, Y, X, Nf = struct.unpack_from('>BHHB', body)
            frame = dict(P=P, H=Y, W=X, comps=[(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(Nf)])
        elif m == 0xC4:
            i = 0
            while i < len(body):
                tc_th = body[i]
                counts = list(body[i + 1:i + 17])
                vals = list(body[i + 17:i + 17 + sum(counts)])
                look, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        look[(length, code)] = vals[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[tc_th] = (look, counts, vals)
                i += 17 + len(vals)
        elif m == 0xDA:
            ns = body[0]
            scan = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            break
        elif m in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA, 0xDD):
            raise ValueError('marker FF%02X: not a baseline file without restart intervals' % m)
    if frame is None or frame['P'] != 8 or len(frame['comps']) != 3 or len(scan) != 3:
        raise ValueError('not an 8-bit three-component frame in one scan')
    hmax, vmax = max(c[1] for c in frame['comps']), max(c[2] for c in frame['comps'])
    mx, my = -(-frame['W'] // (8 * hmax)), -(-frame['H'] // (8 * vmax))
    br = _Bits(data, pos)
    pred, blocks = [0] * 3, []
    for _ in range(mx * my):
        for ci, (cid, h, v, tq) in enumerate(frame['comps']):
            _, td, ta = scan[ci]
            for _ in range(h * v):
                blk = [0] * 64
                s = _decode_symbol(br, huff[td][0])
                pred[ci] += _extend(br.take(s), s)
                blk[0] = pred[ci]
                k = 1
                while k < 64:
                    rs = _decode_symbol(br, huff[0x10 | ta][0])
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    blk[k] = _extend(br.take(s), s)
                    k += 1
                blocks.append(blk)
    pad_ok = all(br.bit() == 1 for _ in range(br.left))
    if data[br.p:br.p + 2] != b'\xff\xd9':
        raise ValueError('no EOI behind the entropy-coded data')
    markers.append('EOI')
    sub = {(2, 2): '420', (1, 1): '444'}.get((hmax, vmax))
    return dict(H=frame['H'], W=frame['W'], subsampling=sub, qtables=q, coef=np.array(blocks, dtype=np.int16), markers=markers,
                tables={k: (v[1], v[2]) for k, v in huff.items()}, comps=frame['comps'], pad_ok=pad_ok, end=br.p + 2)


_DEC_ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
           57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


# ---- the pictures -------------------------------------------------------------------------------------------------------------------------
MIN_SEGMENT = 8                                                      # blocks: ELD_JPEG_MIN_SEGMENT


def smooth(H, W, seed=0):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rng = np.random.default_rng(seed)
    img = np.stack([128 + 100 * np.sin(x / 7.0 + i) * np.cos(y / 5.0 - i) for i in range(3)], axis=-1) + rng.normal(0, 3, (H, W, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def grey(plane):
    return np.repeat(np.asarray(plane, dtype=np.uint8)[..., None], 3, axis=2)


def basis(u, v, amp):
    """an 8 x 8 grey block that is the DCT basis function (vertical frequency u, horizontal v)"""
    i = np.arange(8)
    return grey(np.rint(128 + amp * np.outer(np.cos((2 * i + 1) * u * np.pi / 16), np.cos((2 * i + 1) * v * np.pi / 16))))


class Case:
    def __init__(self, name, rgb, quality, subsampling, check=None):
        self.name, self.rgb, self.quality, self.subsampling, self._check = name, np.ascontiguousarray(rgb), quality, subsampling, check

    def encode(self):
        info = {}
        data = encode(self.rgb, self.quality, self.subsampling, info)
        return data, info

    def check(self, info):
        """what the case is there for holds (a case that loses its point fails)"""
        if self._check:
            self._check(info)

    def __repr__(self):
        return self.name


def _syms(info, cls):
    return [s for bs in info['symbols'] for c, s, _, _ in bs if c == cls]


def _dummy_count(H, W):
    mh, mw, my, mx, _ = geometry(H, W, '420')
    return 4 * my * mx - (-(-H // 8)) * (-(-W // 8))


def cases():
    out = []

    def add(name, rgb, q, sub, check=None):
        out.append(Case(name, rgb, q, sub, check))

    def one_mcu(info):
        assert info['blocks'] == info['bpm']
    add('one_mcu_444', smooth(8, 8, 1), 90, '444', one_mcu)
    add('one_mcu_420', smooth(16, 16, 2), 90, '420', one_mcu)
    add('one_pixel_444', noise(1, 1, 3), 90, '444', one_mcu)
    add('one_pixel_420', noise(1, 1, 3), 90, '420', one_mcu)
    for H, W in ((37, 53), (9, 70)):
        for sub in ('444', '420'):
            def edges(info, H=H, W=W, sub=sub):
                assert H % 8 and W % 8 and (W % 2 or H % 2)
                if sub == '420':
                    assert _dummy_count(H, W) > 0
            add('smooth_%dx%d_%s' % (H, W, sub), smooth(H, W, H), 90, sub, edges)
            add('noise_%dx%d_%s' % (H, W, sub), noise(H, W, W), 90, sub, edges)

    def flat(info):
        assert set(_syms(info, 1)) == {0x00} and set(_syms(info, 0)[3:]) == {0}
        assert all(sum(t[0]) <= 2 for t in info['tables'])
    add('flat_grey', np.full((48, 48, 3), 128, dtype=np.uint8), 90, '420', flat)

    def dc11(info):
        assert 11 in _syms(info, 0)
    add('dc_size_11', grey(np.kron((np.indices((2, 4)).sum(0) % 2) * 255, np.ones((8, 8)))), 100, '444', dc11)

    def ac10(info):
        assert any(s & 15 == 10 for s in _syms(info, 1))
    step = np.zeros((8, 16))
    step[:, 4:8] = 255
    step[:, 12:] = 255
    add('ac_size_10', grey(step), 100, '444', ac10)

    def zrl(info):
        assert 0xF0 in _syms(info, 1) and info['coef'][0, 63] == 0
    add('zrl', np.concatenate([basis(5, 6, 100), basis(0, 0, 0)], axis=1), 90, '444', zrl)

    def no_eob(info):
        assert info['coef'][0, 63] != 0 and 0x00 not in [s for c, s, _, _ in info['symbols'][0] if c == 1]
    add('no_eob', np.concatenate([basis(7, 7, 110), basis(0, 0, 0)], axis=1), 90, '444', no_eob)

    def stuffed(info):
        print('noise 64x48 quality 100: %d stuffed FF bytes, %d bits' % (info['stuffed'], info['nbits']))
        assert info['stuffed'] > 0
        assert max(l for t in info['tables'] for l in range(1, 17) if t[0][l - 1]) >= 10     # codes well beyond a byte, plus up to 10 extra bits

    def phases(info):
        stuffed(info)
        assert {s % 32 for s in info['starts']} == set(range(32))    # cut at MIN_SEGMENT, segments start at many phases too
        assert info['blocks'] >= 4 * MIN_SEGMENT and len({info['starts'][i] % 32 for i in range(0, info['blocks'], MIN_SEGMENT)}) >= 8
    add('noise_q100_444', noise(48, 64, 7), 100, '444', phases)
    add('noise_q100_420', noise(48, 64, 8), 100, '420', stuffed)
    return out
