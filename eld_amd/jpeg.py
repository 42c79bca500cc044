"""Write JPEG: the sRGB render (uint8, on the device) as a baseline JFIF file, encoded on the device (csrc/jpeg.hip).

    quant_tables(quality)                                   the two Annex K.1 tables scaled by libjpeg's rule, 64 values each in natural order
    encode_jpeg(rgb, quality=90, subsampling='420')         (3, H, W) or (H, W, 3) uint8 (NumPy: uploaded; a CUDA tensor: used in place) -> bytes;
                                                            (N, 3, H, W) -> a list of bytes
    write_jpeg(path, rgb, **kw)
    jpeg_info(data)                                         width, height and subsampling of a baseline file, read from its SOF0
    python -m eld_amd.jpeg in.npy -o out.jpg [--quality Q] [--subsampling 444|420]

The file: SOI, APP0 JFIF 1.01, two DQT, SOF0 (Y, Cb, Cr; one interleaved scan), four DHT built from the picture's own histograms (Annex K.2:
dng.huffman_lengths, the package's one implementation), SOS, the data, EOI.  The quantised coefficients are libjpeg's bit for bit (integer
colour conversion, h2v2 downsampling, the slow-integer DCT), so a decoder shows what Pillow's file at the same settings shows.  The host
sees the histograms, one size and the compressed bytes; the picture and its coefficients stay on the device."""
import argparse
import struct
import sys

import numpy as np

from . import _lib as L
from .dng import encoder_table, huffman_lengths

K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K1_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
SUBSAMPLING = {'444': L.JPEG_444, '420': L.JPEG_420}
_LDS_BYTES = -1                          # the LDS image of eld_jpeg_pack_i16 (-1: the library chooses); tests run both ends
# the extra bits behind every symbol of the four alphabets, in the histogram's layout: a DC size, the low nibble of an AC run/size byte
_EXTRA = np.concatenate([np.arange(12), np.arange(12), np.arange(256) & 15, np.arange(256) & 15]).astype(np.int64)


def quant_tables(quality):
    """-> (luma, chroma): 64 ints each, natural (row-major) order; quality 1..100"""
    try:
        q = int(quality)
    except (TypeError, ValueError):
        q = 0
    if not 1 <= q <= 100 or q != quality:
        raise ValueError('quality = %r: an integer in 1..100' % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((t * scale + 50) // 100, 1), 255) for t in tab] for tab in (K1_LUMA, K1_CHROMA))


def _check_args(quality, subsampling, segment, chunk):
    tables = quant_tables(quality)
    sub = str(subsampling)
    if sub not in SUBSAMPLING:
        raise ValueError("subsampling = %r: '444' or '420'" % (subsampling,))
    segment, chunk = int(segment), int(chunk)
    if segment and (segment % L.JPEG_MIN_SEGMENT or not L.JPEG_MIN_SEGMENT <= segment <= L.JPEG_MAX_SEGMENT):
        raise ValueError('segment = %d blocks: a multiple of %d up to %d, or 0 for the default' % (segment, L.JPEG_MIN_SEGMENT, L.JPEG_MAX_SEGMENT))
    if chunk and (chunk % L.DNG_ENC_MIN_CHUNK or not L.DNG_ENC_MIN_CHUNK <= chunk <= L.DNG_ENC_MAX_CHUNK):
        raise ValueError('chunk = %d bytes: a multiple of %d up to %d, or 0 for the default' % (chunk, L.DNG_ENC_MIN_CHUNK, L.DNG_ENC_MAX_CHUNK))
    return tables, sub, segment or L.JPEG_SEGMENT, chunk or L.DNG_ENC_CHUNK


def _layout(rgb):
    """-> ('chw' | 'hwc' | 'nchw', N, H, W) of a uint8 picture or batch; anything else is a ValueError that names what came"""
    dt = getattr(rgb, 'dtype', None)
    if not (dt == np.uint8 if isinstance(rgb, np.ndarray) else str(dt) == 'torch.uint8'):
        raise ValueError('rgb: a uint8 array or tensor, got dtype %s' % (dt if dt is not None else type(rgb).__name__,))
    shape = tuple(int(v) for v in rgb.shape)
    if len(shape) == 4 and shape[1] == 3:
        kind, (N, H, W) = 'nchw', (shape[0], shape[2], shape[3])
    elif len(shape) == 3 and shape[0] == 3:
        kind, (N, H, W) = 'chw', (1, shape[1], shape[2])
    elif len(shape) == 3 and shape[2] == 3:
        kind, (N, H, W) = 'hwc', (1, shape[0], shape[1])
    else:
        raise ValueError('rgb: (3, H, W), (H, W, 3) or (N, 3, H, W), got shape %r' % (shape,))
    if N < 1 or not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError('rgb of shape %r: H and W lie in 1..65535' % (shape,))
    if H * W >= 1 << 31:
        raise ValueError('rgb of shape %r: H * W must stay below 2^31' % (shape,))
    return kind, N, H, W


def header(H, W, sub, tables, dht):
    """SOI .. SOS.  tables: (luma, chroma) divisors; dht: [(counts, symbols)] for DC0, AC0, DC1, AC1"""
    def seg(marker, body):
        return bytes([0xFF, marker]) + struct.pack('>H', 2 + len(body)) + body
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, q in enumerate(tables):
        out += seg(0xDB, bytes([i]) + bytes(q[z] for z in ZIGZAG))
    out += seg(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x22 if sub == '420' else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for (counts, symbols), tc_th in zip(dht, (0x00, 0x10, 0x01, 0x11)):
        out += seg(0xC4, bytes([tc_th]) + bytes(counts) + bytes(symbols))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class Encoder:
    """One picture, step by step (encode_jpeg runs the steps in order; tools/jpeg_time.py times them one by one):
    coef() -> hist() -> plan() -> pack() -> ffcount() -> sizes() -> stuff() -> data().  planes: a contiguous (3, H, W) uint8 CUDA tensor."""
    def __init__(self, planes, quality=90, subsampling='420', segment=0, chunk=0):
        import torch
        self.torch = torch
        self.tables, self.sub, self.segment, self.chunk = _check_args(quality, subsampling, segment, chunk)
        self.planes = planes
        self.H, self.W = int(planes.shape[1]), int(planes.shape[2])
        self.dev = planes.device
        self.lib = L.lib()
        m = 16 if self.sub == '420' else 8
        self.nblocks = -(-self.H // m) * -(-self.W // m) * (6 if self.sub == '420' else 3)
        self.nseg = -(-self.nblocks // self.segment)
        self.qt = np.array(self.tables[0] + self.tables[1], dtype=np.uint16)

    def _geom(self):
        return (L.dptr(self.d_coef), self.nblocks * 64, self.H, self.W, SUBSAMPLING[self.sub], self.segment)

    def _up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(self.dev)

    def coef(self):
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.d_coef = torch.empty(self.nblocks * 64, dtype=torch.int16, device=self.dev)
            L.check(self.lib.eld_jpeg_coef_u8(L.dptr(self.planes), self.H, self.W, SUBSAMPLING[self.sub], self.qt.ctypes.data, L.dptr(self.d_coef),
                                              self.nblocks * 64, L.cur_stream()), 'eld_jpeg_coef_u8')

    def hist(self):
        torch = self.torch
        with torch.cuda.device(self.dev):
            self.d_hist = torch.empty(self.nseg * L.JPEG_HIST, dtype=torch.int32, device=self.dev)
            L.check(self.lib.eld_jpeg_hist_i16(*self._geom(), L.dptr(self.d_hist), self.nseg * L.JPEG_HIST, L.cur_stream()), 'eld_jpeg_hist_i16')

    def plan(self):
        """The histograms -> the four tables and the markers, every segment's first bit, the chunks of the unstuffed bytes."""
        h = self.d_hist.cpu().numpy().view(np.uint32).reshape(self.nseg, L.JPEG_HIST).astype(np.int64)
        tot = h.sum(axis=0)
        cut = (0, 12, 24, 280, 536)
        parts = [tot[cut[i]:cut[i + 1]] for i in range(4)]          # DC luma, DC chroma, AC luma, AC chroma
        dht = [huffman_lengths(p, len(p)) for p in parts]
        enc = [encoder_table(c, s, len(p)) for (c, s), p in zip(dht, parts)]
        tab = np.zeros(L.JPEG_TABLE, dtype=np.uint32)
        tab[0:12], tab[17:29], tab[34:290], tab[290:546] = enc
        lens = np.concatenate(enc).astype(np.int64) >> 16
        seg_bit = np.zeros(self.nseg + 1, dtype=np.int64)
        seg_bit[1:] = np.cumsum((h * (lens + _EXTRA)[None, :]).sum(axis=1))
        self.header = header(self.H, self.W, self.sub, self.tables, [dht[0], dht[2], dht[1], dht[3]])
        self.nraw = (int(seg_bit[-1]) + 7) // 8
        if self.nraw >= 1 << 32:
            raise ValueError('the entropy-coded data takes %d bytes: more than 2^32' % self.nraw)
        self.raw_bytes = (self.nraw + 3) // 4 * 4
        self.nchunks = -(-self.nraw // self.chunk)
        j = np.arange(self.nchunks, dtype=np.int64)
        ch = np.zeros(self.nchunks, dtype=L.DNG_ENC_CHUNK_DTYPE)
        ch['src'] = j * self.chunk
        ch['nbytes'] = np.minimum(self.chunk, self.nraw - j * self.chunk)
        ch['dst'] = j * self.chunk
        torch = self.torch
        self.d_tables, self.d_seg_bit, self.d_chunks = self._up(tab), self._up(seg_bit.astype(np.uint64)), self._up(ch)
        self.d_raw = torch.empty(self.raw_bytes // 4, dtype=torch.int32, device=self.dev)
        self.d_count = torch.empty(self.nchunks, dtype=torch.int32, device=self.dev)

    def pack(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_jpeg_pack_i16(*self._geom(), L.dptr(self.d_tables), L.dptr(self.d_seg_bit), L.dptr(self.d_raw), self.raw_bytes // 4,
                                               _LDS_BYTES, L.cur_stream()), 'eld_jpeg_pack_i16')

    def ffcount(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_dng_enc_ffcount_u8(L.dptr(self.d_raw), self.nraw, L.dptr(self.d_chunks), self.nchunks, self.chunk,
                                                    L.dptr(self.d_count), L.cur_stream()), 'eld_dng_enc_ffcount_u8')

    def sizes(self):
        """The running sum of the FF counts (device), then the one synchronisation: the stuffed size."""
        torch = self.torch
        cum = torch.cumsum(self.d_count, 0, dtype=torch.int64)
        self.d_before = (cum - self.d_count).to(torch.int32).contiguous()
        self.out_bytes = self.nraw + int(cum[-1])
        if self.out_bytes >= 1 << 32:
            raise ValueError('the stuffed data takes %d bytes: more than 2^32' % self.out_bytes)
        self.d_out = torch.empty((self.out_bytes + 3) // 4 * 4, dtype=torch.uint8, device=self.dev)

    def stuff(self):
        with self.torch.cuda.device(self.dev):
            L.check(self.lib.eld_dng_enc_stuff_u8(L.dptr(self.d_raw), self.nraw, L.dptr(self.d_chunks), self.nchunks, self.chunk,
                                                  L.dptr(self.d_before), L.dptr(self.d_out), self.out_bytes, L.cur_stream()), 'eld_dng_enc_stuff_u8')

    def data(self):
        """The one copy of the compressed bytes to the host -> the complete file."""
        return self.header + self.d_out[:self.out_bytes].cpu().numpy().tobytes() + b'\xff\xd9'

    def run(self):
        for step in (self.coef, self.hist, self.plan, self.pack, self.ffcount, self.sizes, self.stuff):
            step()
        return self.data()


def device_planes(rgb):
    """rgb as `_layout` accepts it -> (kind, a contiguous (N, 3, H, W) uint8 CUDA tensor); a NumPy array is uploaded"""
    import torch
    kind, N, H, W = _layout(rgb)
    if isinstance(rgb, np.ndarray):
        rgb = torch.from_numpy(np.ascontiguousarray(rgb)).to(torch.device('cuda', torch.cuda.current_device()))
    if rgb.device.type != 'cuda':
        raise ValueError('rgb: encode_jpeg encodes on a CUDA device, got a tensor on %s' % rgb.device)
    rgb = rgb.detach()
    if kind == 'hwc':
        rgb = rgb.permute(2, 0, 1)
    return kind, rgb.reshape(N, 3, H, W).contiguous()


def encode_jpeg(rgb, quality=90, subsampling='420', segment=0, chunk=0):
    """`rgb` ((3, H, W) or (H, W, 3) uint8: NumPy, uploaded; or a CUDA tensor, used where it lies, made planar and contiguous if it is not) ->
    the bytes of a baseline JFIF file; a batch (N, 3, H, W) -> a list of N.  quality 1..100 scales the Annex K.1 tables by libjpeg's rule;
    subsampling '444' or '420'.  segment (blocks) and chunk (bytes) cut the work of the kernels, 0: the defaults; the bytes do not depend on
    them.  Every argument is checked before any device work."""
    _check_args(quality, subsampling, segment, chunk)
    _layout(rgb)
    kind, planes = device_planes(rgb)
    out = [Encoder(planes[i], quality, subsampling, segment, chunk).run() for i in range(planes.shape[0])]
    return out if kind == 'nchw' else out[0]


def write_jpeg(path, rgb, **kw):
    data = encode_jpeg(rgb, **kw)
    if isinstance(data, list):
        raise ValueError('write_jpeg writes one picture, got a batch of %d' % len(data))
    with open(path, 'wb') as fh:
        fh.write(data)
    return len(data)


def jpeg_info(data):
    """The SOF0 of a baseline JPEG -> dict(width, height, subsampling=(horizontal, vertical) factors of Y over chroma).  ValueError for bytes
    that are not a baseline (SOF0) three-component 8-bit JPEG."""
    if not isinstance(data, (bytes, bytearray)) or len(data) < 4 or data[:2] != b'\xff\xd8':
        raise ValueError('not a JPEG: no SOI marker')
    pos = 2
    while pos + 4 <= len(data):
        if data[pos] != 0xFF:
            raise ValueError('not a JPEG: no marker at byte %d' % pos)
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n, = struct.unpack_from('>H', data, pos + 2)
        if m == 0xC0:
            if n < 17 or pos + 2 + n > len(data):
                raise ValueError('not a baseline JPEG: a short SOF0')
            P, Y, X, Nf = struct.unpack_from('>BHHB', data, pos + 4)
            comps = [(data[pos + 10 + 3 * i], data[pos + 11 + 3 * i] >> 4, data[pos + 11 + 3 * i] & 15) for i in range(min(Nf, 3))]
            if P != 8 or Nf != 3 or X < 1 or Y < 1 or comps[1][1:] != (1, 1) or comps[2][1:] != (1, 1):
                raise ValueError('not a baseline YCbCr JPEG: precision %d, %d components' % (P, Nf))
            return dict(width=X, height=Y, subsampling=(comps[0][1], comps[0][2]))
        if m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise ValueError('not a baseline JPEG: frame marker FF%02X' % m)
        if m == 0xDA:
            break
        pos += 2 + n
    raise ValueError('not a baseline JPEG: no SOF0 in front of the scan')


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m eld_amd.jpeg', description='Encode a uint8 sRGB picture (.npy, (3,H,W) or (H,W,3)) as a JPEG on the device.')
    ap.add_argument('input', help='a .npy file')
    ap.add_argument('-o', '--out', required=True, help='the .jpg to write')
    ap.add_argument('--quality', type=int, default=90, help='1..100 (default 90)')
    ap.add_argument('--subsampling', choices=sorted(SUBSAMPLING), default='420', help='chroma subsampling (default 420)')
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    rgb = np.load(a.input)
    n = write_jpeg(a.out, rgb, quality=a.quality, subsampling=a.subsampling)
    _, _, H, W = _layout(rgb)
    print('%s -> %s (%d x %d, quality %d, %s, %d bytes)' % (a.input, a.out, H, W, a.quality, a.subsampling, n))
    return 0


if __name__ == '__main__':
    sys.exit(main())
