"""NumPy restatement of the sampler's float32 op chain WITH the column term (flag COL, model letter C), and of its column variates.

oracle/noise_ref.py states the chain without the term; this file restates it op for op with `z = z + n_col * col_scale` directly after the
row term (tests/test_colnoise_cpu.py pins the restatement, COL off, to oracle.noise_ref.noise_arith bit for bit).  The column normals are
drawn through oracle/philox_ref.py at (STREAM_COL, sensor column), words 0 and 1, by the transform of the row normals."""
import numpy as np

from oracle import noise_ref as O
from oracle import philox_ref as px

COL = 2048            # ELD_COL
XT = 512              # ELD_CFA_XTRANS
STREAM_COL = 9
PLANE_NCOL = 6        # ELD_PLANE_NCOL; the debug buffers hold NPLANES_COL planes when COL is set
NPLANES_COL = 7
LDS_COLS = 512        # MAX_LDS_COLS of eld_amd/csrc/noise.hip: the staged column normals of one block

F32 = np.float32


def noise_arith_col(y, p, flags, col_scale=0.0, counts=None, n_shot=None, n_read=None, t_tl=None, n_row=None, n_col=None, u_q=None):
    """oracle.noise_ref.noise_arith with the column term: strict float32, one rounding per operation, no contraction."""
    y = np.asarray(y, dtype=F32)
    S, r, K = F32(p['saturation']), F32(p['ratio']), F32(p['K'])
    y1 = (y * S).astype(F32)
    y2 = (y1 / r).astype(F32)
    if flags & O.SHOT_POISSON:
        z = (np.asarray(counts).astype(F32) * K).astype(F32)
    elif flags & O.SHOT_GAUSS:
        sd = np.sqrt(np.maximum((K * y2).astype(F32), F32(1e-10))).astype(F32)
        z = (y2 + (np.asarray(n_shot, F32) * sd).astype(F32)).astype(F32)
    else:
        z = y2
    if flags & O.READ_GAUSS:
        g = np.maximum(F32(p['g_scale']), F32(1e-10))
        z = (z + (np.asarray(n_read, F32) * g).astype(F32)).astype(F32)
    if flags & O.READ_TL:
        z = (z + (np.asarray(t_tl, F32) * F32(p['tl_scale'])).astype(F32)).astype(F32)
    if flags & O.ROW:
        z = (z + (np.asarray(n_row, F32) * F32(p['row_scale'])).astype(F32)).astype(F32)
    if flags & COL:                                # the new term: mul, then add, directly after the row term
        z = (z + (np.asarray(n_col, F32) * F32(col_scale)).astype(F32)).astype(F32)
    if flags & O.QUANT:
        z = (z + ((np.asarray(u_q, F32) - F32(0.5)).astype(F32) * F32(p['q_step'])).astype(F32)).astype(F32)
    if flags & O.CBIAS:
        cb = np.asarray(p['color_bias'], F32).reshape(-1, 1, 1)
        z = (z + cb).astype(F32)
    z = (z * r).astype(F32)
    z = (z / S).astype(F32)
    if flags & O.CLIP:
        z = np.maximum(np.minimum(z, F32(1.0)), F32(0.0)).astype(F32)
    return z


def sensor_cols(C, H, W):
    """(C,H,W) int64: the patch-local sensor column of every packed element.  C == 4: Bayer, planes 0 and 3 on the even mosaic columns 2w,
    planes 1 and 2 on the odd ones (the pack of noise.py:16-19); C == 9: the mosaic column RawPacker.pack_raw_xtrans reads."""
    if C == 4:
        c = np.arange(4)
        par = (c ^ (c >> 1)) & 1
        return np.broadcast_to(2 * np.arange(W)[None, None, :] + par[:, None, None], (4, H, W)).astype(np.int64)
    assert C == 9
    return O.xtrans_source_index(H, W)[1]


def n_sensor_cols(C, W):
    return 2 * W if C == 4 else 3 * W


def col_normals(ncols, seed, sample_id):
    """The normal of sensor columns 0 .. ncols - 1 of one sample: Box-Muller (first output) of words 0, 1 of Philox (column, sample id, stream 9)."""
    w = px.sampler_words(np.arange(ncols, dtype=np.uint32), sample_id, STREAM_COL, seed)
    return px.box_muller(w[0], w[1])[0]


def unpack(planes):
    """Packed (C,H,W) -> the mosaic, by the oracle's index maps."""
    return O.unpack_raw_bayer(planes) if planes.shape[0] == 4 else O.unpack_raw_xtrans(planes)
