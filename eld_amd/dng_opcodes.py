"""DNG opcode lists: parse OpcodeList1/2/3, and turn what they ask for into the two objects the pipeline already has -- a DefectMap (list 1's
bad pixels, repaired before anything else runs) and a FlatField whose lens plane multiplies the network's output (the gain opcodes of
lists 2 and 3).  The mosaic-domain opcodes are evaluated per site on the device (libeld_amd: eld_dng_opcodes_apply_f32,
eld_dng_opcodes_gain_f32; csrc/dng_opcodes.hip).

    lists = read_opcodes(path)                        (ops1, ops2, ops3), each a list of Opcode; .raw: the tags' bytes; .linearization
    parse_opcode_list(data, name) / pack_opcode_list(ops)       bytes <-> [Opcode]; they round-trip
    prog = OpcodeProgram(ops2, Hm, Wm)                list-2 opcodes 7..13 compiled: <= 32 records, one blob <= 64 MiB
    apply_list2(linear, prog, out=None)               float32 (Hm,Wm) / (N,Hm,Wm) in [0,1] on the device -> the "stage 2" image
    gain_plane(ops2, ops3, Hm, Wm, device)            float32 (Hm,Wm): the per-site product of the multiplicative opcodes
    lens_from_opcodes(ops2, ops3, Hm, Wm, ...)        -> FlatField (lens = that plane, prnu = 1)
    defects_from_opcodes(ops1, mosaic, meta)          -> DefectMap (FixBadPixelsList, FixBadPixelsConstant)
    warp_from_opcodes(ops3, Hm, Wm)                   -> Warp (list 3's WarpRectilinear) or None; warp_params / pack_warp: its bytes <-> fields

The list is big-endian whatever the file's byte order: uint32 count, then per opcode uint32 id, DNG version, flags (bit 0: optional, bit 1:
skip for preview), byte count of the parameters, and the parameters.  Parsing checks every offset and count against the bytes; a failure is a
ValueError that names the list, the opcode's index and the field.  An id this module does not apply (unknown, or in a list where it has no
meaning here) is skipped when its optional bit is set and a ValueError otherwise -- raised when the list is APPLIED, not when it is parsed
or reported.  Warps (1, 2) and TrimBounds (6) are known by name and never applied by the lists' own machinery: parse_opcode_list keeps their
bytes and disposition answers 'never'.  WarpRectilinear is decoded on request (warp_params, warp_from_opcodes) for the full-resolution render,
which resamples the demosaiced camera RGB with it (eld_amd.isp.warp_rgb, eld_warp_rgb_f32; denoise --warp).

Where a list applies: list 1 to the stored image (its coordinates are relative to the full stored image: the ActiveArea origin is subtracted
and what falls outside the visible mosaic is dropped); lists 2 and 3 to the active area, which is the mosaic read_dng returns.  A mosaic has
one plane: an area with Plane >= 1 addresses nothing, and plane 0 of a GainMap is used.

The arithmetic of every opcode is the contract of DESIGN.md sec. 29 and include/eld_amd.h; tests/dng_opcodes_ref.py restates it bit for bit."""
import struct

import numpy as np

from . import _lib as L

OPTIONAL, SKIP_PREVIEW = 1, 2
NAMES = {1: 'WarpRectilinear', 2: 'WarpFisheye', 3: 'FixVignetteRadial', 4: 'FixBadPixelsConstant', 5: 'FixBadPixelsList', 6: 'TrimBounds',
         7: 'MapTable', 8: 'MapPolynomial', 9: 'GainMap', 10: 'DeltaPerRow', 11: 'DeltaPerColumn', 12: 'ScalePerRow', 13: 'ScalePerColumn'}
NEVER_APPLIED = (1, 2, 6)
AREA_IDS = (7, 8, 9, 10, 11, 12, 13)
VECTOR_IDS = (10, 11, 12, 13)
GAIN_IDS_2 = (9, 12, 13)                  # list 2's multiplicative opcodes: what the lens plane folds in
NOT_GAIN_IDS_2 = (7, 8, 10, 11)           # list 2's others: they change the network's input
APPLIED = {1: (4, 5), 2: AREA_IDS, 3: (3,)}                          # list number -> the ids this module applies there
LIST_NAMES = ('OpcodeList1', 'OpcodeList2', 'OpcodeList3')
AREA_KEYS = ('top', 'left', 'bottom', 'right', 'plane', 'planes', 'row_pitch', 'col_pitch')
DEFAULT_VERSION = 0x01030000
MAX_POINTS = 1 << 24                      # V * H of one GainMap


class Opcode:
    """One opcode: id, version (uint32), flags, and either typed fields (`f`, a dict, for the ids with typed parameters) or the raw
    parameter bytes (`data`, for every other id).  name: the specification's name, or 'opcode <id>'."""
    __slots__ = ('id', 'version', 'flags', 'f', 'data')

    def __init__(self, id, f=None, data=b'', flags=0, version=DEFAULT_VERSION):
        self.id, self.version, self.flags, self.f, self.data = int(id), int(version), int(flags), f, bytes(data)

    @property
    def name(self):
        return NAMES.get(self.id, 'opcode %d' % self.id)

    @property
    def optional(self):
        return bool(self.flags & OPTIONAL)

    def _key(self):
        f = None if self.f is None else {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in self.f.items()}
        return (self.id, self.version, self.flags, f, self.data)

    def __eq__(self, other):
        return isinstance(other, Opcode) and self._key() == other._key()

    def __repr__(self):
        return 'Opcode(%s%s)' % (self.name, ', optional' if self.optional else '')


def lines_of(f, axis):
    """how many rows (axis 0) or columns (axis 1) an area addresses before clipping: ceil((Bottom - Top) / RowPitch)"""
    lo, hi, pitch = (f['top'], f['bottom'], f['row_pitch']) if axis == 0 else (f['left'], f['right'], f['col_pitch'])
    return -(-(hi - lo) // pitch)


# ---- parser and writer -----------------------------------------------------------------------------------------------------------------
def _typed(id_, p, fail):
    """the parameter bytes `p` of opcode `id_` -> its fields; fail(field, text) raises the ValueError"""
    def need(n, field):
        if len(p) < n:
            fail(field, 'needs %d parameter bytes, the opcode has %d' % (n, len(p)))

    def exact(n, field):
        if len(p) != n:
            fail(field, 'takes %d parameter bytes, the opcode has %d' % (n, len(p)))
    if id_ == 3:
        exact(56, 'parameters')
        v = struct.unpack('>7d', p)
        return {'k': tuple(v[:5]), 'cx': v[5], 'cy': v[6]}
    if id_ == 4:
        exact(8, 'parameters')
        c, ph = struct.unpack('>II', p)
        return {'constant': c, 'bayer_phase': ph}
    if id_ == 5:
        need(12, 'BayerPhase, BadPointCount, BadRectCount')
        ph, P, R = struct.unpack('>III', p[:12])
        exact(12 + 8 * P + 16 * R, 'BadPointCount / BadRectCount (%d, %d)' % (P, R))
        pts = np.frombuffer(p, '>u4', 2 * P, 12).astype(np.int64).reshape(P, 2)
        rects = np.frombuffer(p, '>u4', 4 * R, 12 + 8 * P).astype(np.int64).reshape(R, 4)
        return {'bayer_phase': ph, 'points': pts, 'rects': rects}
    need(32, 'the area record')
    f = dict(zip(AREA_KEYS, struct.unpack('>8I', p[:32])))
    for k in ('row_pitch', 'col_pitch'):
        if f[k] < 1:
            fail('RowPitch' if k == 'row_pitch' else 'ColPitch', 'is 0')
    if f['bottom'] < f['top'] or f['right'] < f['left']:
        fail('area', 'Top, Left, Bottom, Right = %d, %d, %d, %d' % (f['top'], f['left'], f['bottom'], f['right']))
    if id_ == 7:
        need(36, 'TableSize')
        n, = struct.unpack('>I', p[32:36])
        if not 1 <= n <= 65536:
            fail('TableSize', 'is %d: 1..65536' % n)
        exact(36 + 2 * n, 'TableSize (%d)' % n)
        f['table'] = np.frombuffer(p, '>u2', n, 36).astype(np.uint16)
    elif id_ == 8:
        need(36, 'Degree')
        n, = struct.unpack('>I', p[32:36])
        if n > 8:
            fail('Degree', 'is %d: at most 8' % n)
        exact(36 + 8 * (n + 1), 'Degree (%d)' % n)
        f['coefficients'] = np.frombuffer(p, '>f8', n + 1, 36).astype(np.float64)
    elif id_ == 9:
        need(76, 'the map header')
        V, H = struct.unpack('>II', p[32:40])
        f['spacing_v'], f['spacing_h'], f['origin_v'], f['origin_h'] = struct.unpack('>4d', p[40:72])
        planes, = struct.unpack('>I', p[72:76])
        if V < 1 or H < 1 or planes < 1 or V * H > MAX_POINTS:
            fail('MapPointsV, MapPointsH, MapPlanes', 'are %d, %d, %d' % (V, H, planes))
        if len(p) != 76 + 4 * V * H * planes:
            fail('the gains', 'hold %s float32, MapPointsV x MapPointsH x MapPlanes = %d x %d x %d needs %d'
                 % ((len(p) - 76) / 4.0 if (len(p) - 76) % 4 else (len(p) - 76) // 4, V, H, planes, V * H * planes))
        f['gains'] = np.frombuffer(p, '>f4', V * H * planes, 76).astype(np.float32).reshape(V, H, planes)
    else:
        need(36, 'Count')
        n, = struct.unpack('>I', p[32:36])
        want = lines_of(f, 0 if id_ in (10, 12) else 1)
        if n != want:
            fail('Count', 'is %d, the area addresses %d %s' % (n, want, 'rows' if id_ in (10, 12) else 'columns'))
        exact(36 + 4 * n, 'Count (%d)' % n)
        f['values'] = np.frombuffer(p, '>f4', n, 36).astype(np.float32)
    return f


def parse_opcode_list(data, name='opcode list'):
    """The bytes of an OpcodeList tag -> [Opcode].  A count of 0 is an empty list, whatever follows it."""
    data = bytes(data)
    if len(data) < 4:
        raise ValueError('%s: %d bytes: shorter than the count' % (name, len(data)))
    count, = struct.unpack('>I', data[:4])
    ops, pos = [], 4
    for i in range(count):
        def fail(field, text, i=i):
            raise ValueError('%s: opcode %d: %s %s' % (name, i, field, text))
        if pos + 16 > len(data):
            fail('header', 'at byte %d runs beyond the %d bytes of the list (%d opcodes announced)' % (pos, len(data), count))
        id_, ver, flags, n = struct.unpack('>4I', data[pos:pos + 16])
        if pos + 16 + n > len(data):
            fail('byte count', '%d at byte %d runs beyond the %d bytes of the list' % (n, pos + 12, len(data)))
        p = data[pos + 16:pos + 16 + n]
        if id_ in (3, 4, 5) or id_ in AREA_IDS:
            def fail_named(field, text, i=i, id_=id_):
                raise ValueError('%s: opcode %d (%s): %s %s' % (name, i, NAMES[id_], field, text))
            ops.append(Opcode(id_, _typed(id_, p, fail_named), b'', flags, ver))
        else:
            ops.append(Opcode(id_, None, p, flags, ver))
        pos += 16 + n
    return ops


def _params(op):
    f = op.f
    if f is None:
        return op.data
    if op.id == 3:
        return struct.pack('>7d', *(tuple(f['k']) + (f['cx'], f['cy'])))
    if op.id == 4:
        return struct.pack('>II', f['constant'], f['bayer_phase'])
    if op.id == 5:
        pts, rects = np.asarray(f['points']).reshape(-1, 2), np.asarray(f['rects']).reshape(-1, 4)
        return struct.pack('>III', f['bayer_phase'], len(pts), len(rects)) + pts.astype('>u4').tobytes() + rects.astype('>u4').tobytes()
    head = struct.pack('>8I', *(f[k] for k in AREA_KEYS))
    if op.id == 7:
        return head + struct.pack('>I', len(f['table'])) + np.asarray(f['table']).astype('>u2').tobytes()
    if op.id == 8:
        return head + struct.pack('>I', len(f['coefficients']) - 1) + np.asarray(f['coefficients']).astype('>f8').tobytes()
    if op.id == 9:
        g = np.asarray(f['gains'])
        return (head + struct.pack('>II', g.shape[0], g.shape[1]) + struct.pack('>4d', f['spacing_v'], f['spacing_h'], f['origin_v'], f['origin_h']) +
                struct.pack('>I', g.shape[2]) + g.astype('>f4').tobytes())
    return head + struct.pack('>I', len(f['values'])) + np.asarray(f['values']).astype('>f4').tobytes()


def pack_opcode_list(ops):
    """[Opcode] -> the bytes of an OpcodeList tag (big-endian); parse_opcode_list(pack_opcode_list(ops)) == ops."""
    out = [struct.pack('>I', len(ops))]
    for op in ops:
        p = _params(op)
        out.append(struct.pack('>4I', op.id, op.version, op.flags, len(p)) + p)
    return b''.join(out)


def area(top, left, bottom, right, row_pitch=1, col_pitch=1, plane=0, planes=1):
    """the common area record of opcodes 7..13 as the dict the typed fields start with"""
    return dict(zip(AREA_KEYS, (int(top), int(left), int(bottom), int(right), int(plane), int(planes), int(row_pitch), int(col_pitch))))


# ---- reading -----------------------------------------------------------------------------------------------------------------------------
class OpcodeLists(tuple):
    """(ops1, ops2, ops3) of one file.  raw: {tag name: the tag's bytes} of the lists present; linearization: the file has a
    LinearizationTable (the stored codes are then not the codes read_dng returns)."""
    def __new__(cls, lists, raw, linearization):
        self = super().__new__(cls, lists)
        self.raw, self.linearization = raw, bool(linearization)
        return self


def read_opcodes(path):
    """The three opcode lists of a DNG, parsed -> OpcodeLists (ops1, ops2, ops3); a list the file lacks is []."""
    from . import dng as D
    t, _ = D.parse_tiff(path)
    ifd = D._raw_ifd(t)
    raw, lists = {}, []
    for tag, name in D.OPCODE_TAGS:
        e = ifd.get(tag) or t.ifd0.get(tag)
        if e is None:
            lists.append([])
            continue
        b = e.values if isinstance(e.values, bytes) else bytes(bytearray(int(v) & 0xFF for v in e.values))
        raw[name] = b
        lists.append(parse_opcode_list(b, '%s: %s' % (t.path, name)))
    return OpcodeLists(lists, raw, D.T_LINTABLE in ifd)


def disposition(op, list_no, linearization=False):
    """What applying list `list_no` does with `op`: 'apply', 'never' (warps, TrimBounds) or 'skip' (not applied here, optional).  An id that
    is not applied and not optional is a ValueError."""
    if op.id in APPLIED[list_no] and not (op.id == 4 and linearization):
        return 'apply'
    if op.id in NEVER_APPLIED:
        return 'never'
    if op.optional:
        return 'skip'
    why = 'with a LinearizationTable' if op.id == 4 and op.id in APPLIED[list_no] else 'in OpcodeList%d' % list_no
    raise ValueError('%s (id %d) %s is not supported and not marked optional' % (op.name, op.id, why))


# ---- the compiled program -----------------------------------------------------------------------------------------------------------------
def _clip_area(f, Hm, Wm):
    """the area clipped to the image, None when it addresses nothing (empty, outside, or a plane other than 0)"""
    if f['plane'] >= 1 or f['planes'] < 1:
        return None
    t, l, b, r = f['top'], f['left'], min(f['bottom'], Hm), min(f['right'], Wm)
    if t >= b or l >= r:
        return None
    return t, l, b, r


class OpcodeProgram:
    """Opcodes compiled into what the kernels take.  ops: list-2 opcodes (7..13 are compiled; anything else goes by the optional / mandatory
    rule, raised here because compiling is the first step of applying); vignettes: list-3 FixVignetteRadial opcodes appended for the gain
    plane.  only: compile these ids alone and pass over the others without judging them (gain_plane).

    records   numpy DNG_OP_DTYPE, at most 32, areas clipped to (Hm, Wm), empty areas dropped
    blob      numpy uint8, at most 64 MiB: the tables, coefficients (as float32), gains (plane 0) and vectors, each 8-byte aligned
    source    for every record the Opcode it came from;  skipped: the opcodes passed over because optional"""
    def __init__(self, ops, Hm, Wm, vignettes=(), only=None):
        Hm, Wm = int(Hm), int(Wm)
        if Hm < 1 or Wm < 1 or Hm * Wm >= 1 << 31:
            raise ValueError('an image of %d x %d' % (Hm, Wm))
        self.shape = (Hm, Wm)
        recs, chunks, self.source, self.skipped, size = [], [], [], [], 0
        for op in list(ops) + list(vignettes):
            vig = any(op is v for v in vignettes)
            if not vig and (only is not None and op.id not in only):
                continue
            if not vig and disposition(op, 2) != 'apply':
                self.skipped.append(op)
                continue
            r = np.zeros((), L.DNG_OP_DTYPE)
            r['kind'], r['row_pitch'], r['col_pitch'] = op.id, 1, 1
            if vig:
                r['top'], r['left'], r['bottom'], r['right'] = 0, 0, Hm, Wm
                r['p'][:5], r['p'][5], r['p'][6] = op.f['k'], op.f['cx'], op.f['cy']
                data = b''
            else:
                f = op.f
                box = _clip_area(f, Hm, Wm)
                if box is None:
                    continue
                r['top'], r['left'], r['bottom'], r['right'] = box
                r['row_pitch'], r['col_pitch'] = min(f['row_pitch'], 1 << 30), min(f['col_pitch'], 1 << 30)
                if op.id == 7:
                    r['n0'], data = len(f['table']), np.asarray(f['table'], '<u2').tobytes()
                elif op.id == 8:
                    r['n0'], data = len(f['coefficients']) - 1, np.asarray(f['coefficients'], np.float64).astype('<f4').tobytes()
                elif op.id == 9:
                    g = np.ascontiguousarray(np.asarray(f['gains'], '<f4')[:, :, 0])
                    r['n0'], r['n1'], data = g.shape[0], g.shape[1], g.tobytes()
                    r['p'][:4] = f['spacing_v'], f['spacing_h'], f['origin_v'], f['origin_h']
                else:
                    r['n0'], data = len(f['values']), np.asarray(f['values'], '<f4').tobytes()
            r['data_off'] = size
            data += b'\0' * (-len(data) % 8)
            size += len(data)
            chunks.append(data)
            recs.append(r)
            self.source.append(op)
        if len(recs) > L.DNG_MAX_OPS:
            raise ValueError('%d operations: a program holds at most %d' % (len(recs), L.DNG_MAX_OPS))
        if size > L.DNG_MAX_BLOB:
            raise ValueError('the parameters take %d bytes: a program holds at most %d' % (size, L.DNG_MAX_BLOB))
        self.records = np.zeros(len(recs), L.DNG_OP_DTYPE)
        for i, r in enumerate(recs):
            self.records[i] = r[()]
        self.blob = np.frombuffer(b''.join(chunks), np.uint8).copy() if size else np.zeros(0, np.uint8)
        self._dev = {}

    def __len__(self):
        return len(self.records)

    def blob_on(self, device):
        """the blob on `device` (None when it is empty), uploaded once"""
        import torch
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.blob).to(device) if self.blob.size else None
        return self._dev[device]

    def c_records(self):
        import ctypes
        return ctypes.c_void_p(self.records.ctypes.data) if len(self.records) else None


MAP_LDS_BYTES = -1                       # bytes of GainMap gains the kernels may keep in LDS (< 0: the library's default); tests set 0


def _frames(t, shape, what):
    if not hasattr(t, 'is_cuda') or not t.is_cuda or str(t.dtype) != 'torch.float32' or not t.is_contiguous():
        raise ValueError('%s must be a contiguous CUDA float32 tensor' % what)
    s = tuple(int(v) for v in t.shape)
    if len(s) not in (2, 3) or s[-2:] != tuple(shape):
        raise ValueError('%s has shape %s, the program is for (Hm, Wm) = %s or (N, Hm, Wm)' % (what, s, tuple(shape)))
    return s


def apply_list2(linear, program, out=None):
    """Run a compiled list-2 program on float32 frames, (Hm,Wm) or (N,Hm,Wm) in [0,1] on the device: every operation in file order with a
    clip to [0,1] after each, one pass (eld_dng_opcodes_apply_f32).  The result is the specification's "stage 2" image.  out: None (a new
    tensor), a contiguous CUDA float32 tensor of the same shape, or `linear` itself (in place, the same bits).  A NaN site passes through."""
    import torch
    if not isinstance(program, OpcodeProgram):
        raise ValueError('program must be an OpcodeProgram, got %r' % (type(program).__name__,))
    s = _frames(linear, program.shape, 'linear')
    if out is None:
        out = torch.empty_like(linear)
    elif _frames(out, program.shape, 'out') != s or out.device != linear.device:
        raise ValueError('out must have the shape and device of linear')
    N = s[0] if len(s) == 3 else 1
    if N < 1:
        raise ValueError('empty batch')
    with torch.cuda.device(linear.device):
        L.check(L.lib().eld_dng_opcodes_apply_f32(L.dptr(linear), L.dptr(out), N, s[-2], s[-1], program.c_records(), len(program),
                                                  L.dptr(program.blob_on(linear.device)), int(program.blob.size), int(MAP_LDS_BYTES),
                                                  L.cur_stream()), 'eld_dng_opcodes_apply_f32')
    return out


def gain_program(ops2, ops3, Hm, Wm):
    """The multiplicative opcodes as one program: list 2's GainMap, ScalePerRow, ScalePerColumn in file order, then list 3's
    FixVignetteRadial.  Every other opcode of list 3 goes by the optional / mandatory rule; list 2's others are not looked at here."""
    vig = []
    for op in ops3 or ():
        if disposition(op, 3) == 'apply':
            vig.append(op)
    return OpcodeProgram(ops2 or (), Hm, Wm, vignettes=vig, only=GAIN_IDS_2)


def gain_plane(ops2, ops3, Hm, Wm, device=None, out=None):
    """-> float32 (Hm,Wm) on `device`: per site the float32 product, in file order (list 2 before list 3), of the multiplicative opcodes
    that address it -- list 2's GainMap, ScalePerRow and ScalePerColumn, list 3's FixVignetteRadial.  Unclipped; 1 where none applies.
    ops2 may also be an OpcodeProgram built by gain_program."""
    import torch
    prog = ops2 if isinstance(ops2, OpcodeProgram) else gain_program(ops2, ops3, Hm, Wm)
    if prog.shape != (int(Hm), int(Wm)):
        raise ValueError('the program is for %s, asked for (%d, %d)' % (prog.shape, Hm, Wm))
    if out is None:
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != 'cuda':
            raise ValueError('gain_plane runs on a CUDA device, got %s' % dev)
        out = torch.empty((int(Hm), int(Wm)), dtype=torch.float32, device=dev)
    else:
        _frames(out, prog.shape, 'out')
    with torch.cuda.device(out.device):
        L.check(L.lib().eld_dng_opcodes_gain_f32(L.dptr(out), int(Hm), int(Wm), prog.c_records(), len(prog), L.dptr(prog.blob_on(out.device)),
                                                 int(prog.blob.size), int(MAP_LDS_BYTES), L.cur_stream()), 'eld_dng_opcodes_gain_f32')
    return out


def lens_from_opcodes(ops2, ops3, Hm, Wm, cfa='bayer', raw_pattern=None, white_level=16383, device=None):
    """-> FlatField whose lens plane is gain_plane(ops2, ops3, Hm, Wm) and whose prnu is identically 1 (radius 0, frames 0): the file's
    lens-shading correction where the pipeline applies one, on the network's output under --lens.  FlatField refuses a gain that is not
    finite or not positive; that ValueError comes through with the opcode that produced it named."""
    from .flatfield import FlatField
    prog = gain_program(ops2, ops3, Hm, Wm)
    plane = gain_plane(prog, None, Hm, Wm, device).cpu().numpy()
    try:
        return FlatField(plane, np.ones_like(plane), cfa, raw_pattern, radius=0, frames=0, white_level=white_level)
    except ValueError as e:
        if np.all(np.isfinite(plane)) and np.all(plane > 0):
            raise
        who = 'the product of the gain opcodes'
        for op in prog.source:                                       # the first opcode whose own factor is bad
            one = OpcodeProgram([op] if op.id != 3 else [], Hm, Wm, vignettes=[op] if op.id == 3 else (), only=GAIN_IDS_2)
            g = gain_plane(one, None, Hm, Wm, device).cpu().numpy()
            if not (np.all(np.isfinite(g)) and np.all(g > 0)):
                who = '%s (opcode id %d)' % (op.name, op.id)
                break
        raise ValueError('%s gives a gain that is not finite and > 0: %s' % (who, e))


def defects_from_opcodes(ops1, mosaic, meta, linearization=False):
    """List 1's bad pixels -> DefectMap (DefectMap.from_sites).  FixBadPixelsList: its points and the sites of its rectangles, moved from the
    stored image's coordinates into the visible mosaic (meta['active_area']); what falls outside is dropped.  FixBadPixelsConstant: the sites
    of `mosaic` (the codes read_dng returned, NumPy or tensor) equal to Constant -- only for a file without a LinearizationTable
    (`linearization`: read_opcodes(path).linearization), whose codes are still the stored ones; with one the opcode counts as unsupported.
    BayerPhase is not used: the repair is this project's own (defects.repair_device: the lower median of the unflagged same-colour
    neighbours), not the interpolation the DNG specification describes.  DefectMap's own refusals (a flagged site with no unflagged
    neighbour, as a whole bad column gives) come through."""
    from .defects import DefectMap
    Hm, Wm = (int(v) for v in mosaic.shape[-2:])
    top, left = (int(v) for v in meta.get('active_area', (0, 0, Hm, Wm))[:2])
    mask = np.zeros((Hm, Wm), bool)
    for op in ops1 or ():
        if disposition(op, 1, linearization) != 'apply':
            continue
        if op.id == 4:
            c = op.f['constant']
            if c > 65535:
                continue
            if isinstance(mosaic, np.ndarray):
                mask |= mosaic.view(np.uint16) == c
            else:
                import torch
                idx = torch.nonzero(mosaic == (c if c < 32768 or str(mosaic.dtype) != 'torch.int16' else c - 65536)).cpu().numpy()
                mask[idx[:, 0], idx[:, 1]] = True
            continue
        pts = op.f['points'] - np.array([top, left])
        keep = (pts[:, 0] >= 0) & (pts[:, 0] < Hm) & (pts[:, 1] >= 0) & (pts[:, 1] < Wm)
        mask[pts[keep, 0], pts[keep, 1]] = True
        for t, l, b, r in op.f['rects']:
            t, l, b, r = max(t - top, 0), max(l - left, 0), min(b - top, Hm), min(r - left, Wm)
            if t < b and l < r:
                mask[t:b, l:r] = True
    return DefectMap((Hm, Wm), meta.get('cfa', 'bayer'), meta.get('raw_pattern'), mask)


# ---- WarpRectilinear (opcode 1, list 3) ----------------------------------------------------------------------------------------------------------
IDENTITY_SET = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def warp_params(op, where='WarpRectilinear'):
    """The parameter bytes of an opcode-1 Opcode (`.data`, as parse_opcode_list keeps them) -> {'sets': float64 (N,6) rows kr0, kr1, kr2, kr3,
    kt0, kt1, 'cx', 'cy'}.  Big-endian: uint32 N, N x six float64, two float64; exactly 4 + 48 N + 16 bytes; N is 1 (one set for the three
    planes) or 3 (R, G, B).  A wrong length, another N or a value that is not finite is a ValueError that starts with `where`."""
    if op.id != 1:
        raise ValueError('%s: opcode id %d (%s) is no WarpRectilinear' % (where, op.id, op.name))
    p = op.data
    if len(p) < 4:
        raise ValueError('%s: N needs 4 parameter bytes, the opcode has %d' % (where, len(p)))
    n, = struct.unpack('>I', p[:4])
    if n not in (1, 3):
        raise ValueError('%s: N (the number of coefficient sets) is %d: 1 or 3' % (where, n))
    if len(p) != 4 + 48 * n + 16:
        raise ValueError('%s: byte count: N = %d takes %d parameter bytes, the opcode has %d' % (where, n, 4 + 48 * n + 16, len(p)))
    v = np.frombuffer(p, '>f8', 6 * n + 2, 4).astype(np.float64)
    names = ('kr0', 'kr1', 'kr2', 'kr3', 'kt0', 'kt1')
    for i, x in enumerate(v):
        if not np.isfinite(x):
            field = 'set %d %s' % (i // 6, names[i % 6]) if i < 6 * n else ('cx', 'cy')[i - 6 * n]
            raise ValueError('%s: %s is %r: not finite' % (where, field, float(x)))
    return {'sets': v[:6 * n].reshape(n, 6).copy(), 'cx': float(v[6 * n]), 'cy': float(v[6 * n + 1])}


def pack_warp(sets, cx, cy, flags=0):
    """-> the opcode-1 Opcode of these coefficient sets ((6,), (1,6) or (3,6)) and centre; warp_params is its inverse."""
    sets = np.asarray(sets, np.float64).reshape(-1, 6)
    if len(sets) not in (1, 3):
        raise ValueError('a WarpRectilinear holds 1 or 3 coefficient sets, got %d' % len(sets))
    return Opcode(1, None, struct.pack('>I', len(sets)) + sets.astype('>f8').tobytes() + struct.pack('>2d', float(cx), float(cy)), flags)


class Warp:
    """A WarpRectilinear: sets float64 (1,6) or (3,6) rows kr0, kr1, kr2, kr3, kt0, kt1 (three rows: planes R, G, B); cx, cy the centre in
    relative coordinates.  record(Hm, Wm): the EldWarp record eld_warp_rgb_f32 takes for an image of that size; identity: every set is
    (1, 0, 0, 0, 0, 0), so the map returns every pixel's own centre whatever cx, cy are."""
    def __init__(self, sets, cx=0.5, cy=0.5):
        sets = np.array(sets, np.float64).reshape(-1, 6)
        if len(sets) not in (1, 3):
            raise ValueError('a warp holds 1 or 3 coefficient sets, got %d' % len(sets))
        self.sets, self.cx, self.cy = sets, float(cx), float(cy)
        if not (np.all(np.isfinite(sets)) and np.isfinite(self.cx) and np.isfinite(self.cy)):
            raise ValueError('a warp needs finite coefficients and a finite centre, got %r, (%r, %r)' % (sets.tolist(), self.cx, self.cy))

    @property
    def identity(self):
        return bool(np.all(self.sets == np.asarray(IDENTITY_SET)))

    def record(self, Hm, Wm):
        """numpy WARP_DTYPE scalar array: k = the sets with kr0 - 1 in place of kr0; cxp = cx Wm, cyp = cy Hm; m2 = mx mx + my my with
        mx = max(|cxp|, |Wm - cxp|), my likewise; m = sqrt(m2) -- float64, every operation rounded on its own."""
        Hm, Wm = int(Hm), int(Wm)
        if Hm < 1 or Wm < 1 or Hm * Wm >= 1 << 31:
            raise ValueError('an image of %d x %d' % (Hm, Wm))
        r = np.zeros(1, L.WARP_DTYPE)
        r['nsets'] = len(self.sets)
        k = self.sets.copy()
        k[:, 0] = k[:, 0] - 1.0
        r['k'][0, :len(k)] = k
        cxp, cyp = np.float64(self.cx) * np.float64(Wm), np.float64(self.cy) * np.float64(Hm)
        mx, my = max(abs(cxp), abs(np.float64(Wm) - cxp)), max(abs(cyp), abs(np.float64(Hm) - cyp))
        m2 = mx * mx + my * my
        r['cxp'], r['cyp'], r['m2'], r['m'] = cxp, cyp, m2, np.sqrt(m2)
        return r

    def __repr__(self):
        return 'Warp(%d set%s, centre (%g, %g)%s)' % (len(self.sets), '' if len(self.sets) == 1 else 's', self.cx, self.cy,
                                                    ', identity' if self.identity else '')


def warp_from_opcodes(ops3, Hm=None, Wm=None, name='OpcodeList3'):
    """List 3's WarpRectilinear -> Warp, or None when the list holds none.  More than one is a ValueError that says so.  A WarpFisheye (id 2)
    goes by its optional bit: skipped when optional, else a ValueError that names it (it is not implemented).  Every other opcode is not this
    function's business.  Hm, Wm: when given, the image the warp is for is checked as Warp.record checks it."""
    found = None
    for i, op in enumerate(ops3 or ()):
        if op.id == 2 and not op.optional:
            raise ValueError('%s: opcode %d (WarpFisheye) is not supported and not marked optional' % (name, i))
        if op.id != 1:
            continue
        if found is not None:
            raise ValueError('%s: opcode %d is a second WarpRectilinear (the first is opcode %d): a list holds at most one' % (name, i, found[0]))
        f = warp_params(op, '%s: opcode %d (WarpRectilinear)' % (name, i))
        found = (i, Warp(f['sets'], f['cx'], f['cy']))
    if found is None:
        return None
    if Hm is not None and Wm is not None:
        found[1].record(Hm, Wm)
    return found[1]


def merge_defects(a, b):
    """the union of two DefectMaps of one sensor (either may be None)"""
    from .defects import DefectMap
    if a is None or b is None:
        return a if b is None else b
    if a.shape != b.shape or a.cfa != b.cfa:
        raise ValueError('the defect maps are for %s %s and %s %s' % (a.cfa, a.shape, b.cfa, b.shape))
    return DefectMap(a.shape, a.cfa, a.raw_pattern, a.mask | b.mask)


def without_gains(ops, list_no):
    """the list without the opcodes the lens plane folds in (list 2: GainMap, ScalePerRow, ScalePerColumn; list 3: FixVignetteRadial)"""
    drop = GAIN_IDS_2 if list_no == 2 else (3,)
    return [op for op in ops if op.id not in drop]


def normalise(mosaic, meta, device=None):
    """uint16 codes (NumPy or CUDA int16-view tensor, (Hm,Wm)) -> float32 clip((code - black) / (white - black), 0, 1) on the device, with the
    black level of every site's CFA cell: the input of apply_list2.  Elementwise torch: this is plumbing."""
    import torch
    from .mosaic import CfaLayout
    if isinstance(mosaic, np.ndarray):
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        mosaic = torch.from_numpy(np.ascontiguousarray(mosaic).view(np.int16)).to(dev)
    Hm, Wm = (int(v) for v in mosaic.shape)
    lay = CfaLayout.for_map(meta['cfa'], meta.get('raw_pattern'), meta.get('black_level'))
    black = torch.from_numpy(lay.tile(lay.black_cells.reshape(-1), Hm, Wm).astype(np.float32)).to(mosaic.device)
    u = (mosaic.to(torch.int32) & 0xFFFF).to(torch.float32)
    white = torch.full((), float(meta['white_point']), dtype=torch.float32, device=mosaic.device)
    return ((u - black) / (white - black)).clamp_(0.0, 1.0).contiguous()
