"""A classical baseline beside the U-Net: the generalised Anscombe transform, non-local means in the stabilised domain with weights shared
by the CFA planes, and the closed-form unbiased inverse -- the yardstick row the paper's tables open with (BM3D / A-BM3D there), run with
the gain K and the read noise the calibration measured.  It needs no checkpoint.

    den = ClassicalDenoiser('bayer', K=2.1, camera='SonyA7S2')          # sigma from the table's g_scale line at log K
    res = denoise_raw(den, mosaic_u16, 'bayer', black_level=512, white_point=16383, ratio=100, wb=wb, ccm=ccm)
    rep = evaluate_pairs(net, pairs, 'bayer', ..., baseline=den)        # adds psnr_nlm / ssim_nlm beside psnr / psnr_in

The sensor codes -- not the network's clipped input: the clip at 0 alone biases the mean by the size of the signal once sigma / K > 1 --
are packed by the existing input stage with black 0, white 65535 and ratio 1 (so shading and flat-field maps still apply in the same
kernels), turned into stabilised codes of Q = 16 per noise standard deviation by a per-plane table that holds the black level, filtered by
one HIP kernel in integer arithmetic (csrc/nlm.hip: eld_nlm_vst_f32, restated bit for bit by tests/nlm_ref.py) and inverted in float64.
Each plane of the result is z * ratio / (white - black): the network's output convention, so the lens gain, the write-back, the ISP and the
demosaic of denoise_raw follow unchanged.  The contract, the table builders and the measured times are DESIGN.md sec. 24.

With method='bm3d' the filter is BM3D instead (csrc/bm3d.hip: eld_bm3d_vst_f32, restated by tests/bm3d_ref.py): 8 x 8 blocks matched with
distances shared by the planes, a Walsh-Hadamard transform over [planes][group][8][8] -- across the four Bayer planes as well, where every
plane has unit noise variance -- hard thresholding, then an empirical Wiener filter guided by the first estimate; the tables and the inverse
around it are the same.  DESIGN.md sec. 25.

Without a calibration, ClassicalDenoiser.from_frames(frames, cfa, ...) and --K auto take K and the read noise from the frames themselves
(eld_amd.noiselevel).

Command line: python -m eld_amd.classical frames.npy... -o DIR --meta sensor.json --K K|auto [--sigma S | --camera TABLE] [--search 7]
[--patch 2] [--strength 0.5] [--method bm3d [--step 3] [--group 16] [--no-mix]] and every sensor option of python -m eld_amd.denoise (which
keeps its required --ckpt)."""
import ctypes
import math
import os
import sys

import numpy as np

from . import _lib as L

Q = 16                          # stabilised codes per noise standard deviation
FRAC = 4                        # fractional bits of the filtered code: 1 / 256 of a standard deviation
MAX_SEARCH, MAX_PATCH = 10, 3   # the kernel's argument ranges (include/eld_amd.h)
BM3D_MAX_SEARCH, BM3D_MAX_STEP, BM3D_GROUPS, BM3D_BLOCK = 16, 8, (1, 2, 4, 8, 16), 8
METHODS = ('nlm', 'bm3d')
# rint(16 kaiser(8, 2) x kaiser(8, 2)), written out: no Bessel routine is part of the contract
BM3D_WINDOW = ((3, 5, 6, 7, 7, 6, 5, 3), (5, 7, 10, 11, 11, 10, 7, 5), (6, 10, 12, 14, 14, 12, 10, 6), (7, 11, 14, 16, 16, 14, 11, 7),
               (7, 11, 14, 16, 16, 14, 11, 7), (6, 10, 12, 14, 14, 12, 10, 6), (5, 7, 10, 11, 11, 10, 7, 5), (3, 5, 6, 7, 7, 6, 5, 3))


# ---- tables (host, float64, fixed order) --------------------------------------------------------------------------------------------------
def _check_noise(K, sigma):
    K, sigma = float(K), float(sigma)
    if not (math.isfinite(K) and K > 0):
        raise ValueError('K (DN per electron) must be finite and > 0, got %r' % (K,))
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError('sigma (read noise in DN) must be finite and >= 0, got %r' % (sigma,))
    return K, sigma


def vst_tables(K, sigma, black_per_plane):
    """The forward transform of every plane as a table over the sensor codes, uint16 (C, 65536):
    fwd[c][i] = min(rint(Q * (2 / K) * sqrt(max(K * (i - black_c) + 3/8 K^2 + sigma^2, 0))), 32767)."""
    K, sigma = _check_noise(K, sigma)
    blk = [float(b) for b in np.asarray(black_per_plane, dtype=np.float64).reshape(-1)]
    if not blk or len(blk) > 16:
        raise ValueError('black_per_plane takes 1 to 16 values, got %d' % len(blk))
    i = np.arange(65536, dtype=np.float64)
    out = np.empty((len(blk), 65536), np.uint16)
    for c, b in enumerate(blk):
        arg = np.maximum(K * (i - b) + 0.375 * K * K + sigma * sigma, 0.0)
        out[c] = np.minimum(np.rint(Q * (2.0 / K) * np.sqrt(arg)), 32767.0).astype(np.uint16)
    return out


def nlm_weight_table(C, P, strength):
    """-> (sh, wtab uint16 (256,)).  With n = C (2P + 1)^2 terms in a patch distance, two patches of one signal differ by 2 Q^2 n on
    average: that much is subtracted, and the rest decays with strength^2 Q^2 n.  sh is the least shift for which 256 << sh reaches the
    distance whose weight falls below 1 / 510; bin k takes the weight of its middle: wtab[k] = rint(255 exp(-max((k + 1/2) 2^sh - 2 Q^2 n, 0)
    / (strength^2 Q^2 n))), wtab[0] at least 1."""
    C, P, strength = int(C), int(P), float(strength)
    if not (1 <= C <= 16) or not (0 <= P <= MAX_PATCH):
        raise ValueError('C must be in [1, 16] and P in [0, %d], got %d and %d' % (MAX_PATCH, C, P))
    if not (math.isfinite(strength) and strength > 0):
        raise ValueError('strength must be finite and > 0, got %r' % (strength,))
    n = C * (2 * P + 1) ** 2
    h2 = strength ** 2 * Q * Q * n
    bias = 2.0 * Q * Q * n
    top = bias + h2 * math.log(510.0)
    sh = 0
    while (256 << sh) < top:
        sh += 1
    if sh > 24:
        raise ValueError('strength %g puts the weight table beyond the kernel\'s largest shift' % strength)
    k = np.arange(256, dtype=np.float64)
    wt = np.rint(255.0 * np.exp(-np.maximum((k + 0.5) * float(1 << sh) - bias, 0.0) / h2)).astype(np.uint16)
    wt[0] = max(int(wt[0]), 1)
    return sh, wt


def bm3d_tables(C, mix, strength=1.0, lam=2.7):
    """-> (tau1, thr uint32 (5,), tau2, s2 uint32 (5,), win uint8 (64,)): the match thresholds of the two steps, the hard threshold and the
    Wiener noise energy per group size 2^lg, and the aggregation window.  With Q codes per noise standard deviation a block distance has
    n = 64 C terms of expectation 2 Q^2 each, and an unnormalised Walsh-Hadamard coefficient over M 2^lg blocks of 64 sites has the standard
    deviation 8 Q sqrt(M 2^lg) (M = C planes per transformed set with mix, else 1):
      tau1 = 4 Q^2 n strength^2            thr[lg] = rint(lam 8 Q strength sqrt(M 2^lg))
      tau2 = rint(0.64 Q^2 n strength^2)   s2[lg]  = rint((8 Q strength)^2 M 2^lg)"""
    C, mix, strength, lam = int(C), bool(mix), float(strength), float(lam)
    if not (1 <= C <= 16):
        raise ValueError('C must be in [1, 16], got %d' % C)
    if mix and C & (C - 1):
        raise ValueError('grouping across the planes needs a power-of-two number of them, got %d' % C)
    if not (math.isfinite(strength) and strength > 0) or not (math.isfinite(lam) and lam > 0):
        raise ValueError('strength and lam must be finite and > 0, got %r and %r' % (strength, lam))
    n = 64 * C
    M = C if mix else 1
    tau1 = int(np.rint(4.0 * Q * Q * n * strength * strength))
    tau2 = int(np.rint(0.64 * Q * Q * n * strength * strength))
    thr = [float(np.rint(lam * 8.0 * Q * strength * np.sqrt(float(M << lg)))) for lg in range(5)]
    s2 = [float(np.rint((8.0 * Q * strength) ** 2 * float(M << lg))) for lg in range(5)]
    if tau1 >= 1 << 30 or max(thr + s2) >= float(1 << 32) or min(s2) < 1.0:
        raise ValueError('strength %g puts the BM3D tables outside the kernel\'s ranges' % strength)
    return tau1, np.array(thr).astype(np.uint32), tau2, np.array(s2).astype(np.uint32), np.array(BM3D_WINDOW, np.uint8).reshape(-1)


def unbiased_inverse(out, frac, K, sigma):
    """The filtered codes (units of 2^-frac of a stabilised code) -> DN above black, float64 on the tensor's device: the closed form of
    Makitalo and Foi for the generalised Anscombe transform, with D = out / (Q 2^frac), s = sigma / K, Dm = max(D, 2 sqrt(3/8 + s^2)):
    z = K (Dm^2 / 4 + sqrt(3/2) / (4 Dm) - 11 / (8 Dm^2) + 5 sqrt(3/2) / (8 Dm^3) - 1/8 - s^2)."""
    import torch
    K, sigma = _check_noise(K, sigma)
    D = out.to(torch.float64) / float(Q * (1 << int(frac)))
    s = sigma / K
    Dm = torch.clamp(D, min=2.0 * math.sqrt(0.375 + s * s))
    r = math.sqrt(1.5)
    return K * (Dm * Dm / 4.0 + r / (4.0 * Dm) - 11.0 / (8.0 * Dm * Dm) + 5.0 * r / (8.0 * Dm * Dm * Dm) - 0.125 - s * s)


# ---- the kernel's wrapper -------------------------------------------------------------------------------------------------------------------
def nlm_vst(x, qscale, fwd, S, P, sh, wtab, frac, out=None):
    """eld_nlm_vst_f32 on CUDA tensors: x (N,C,h,w) float32 (any 4-byte aligned contiguous view), fwd (C,65536) uint16 codes as an int16 /
    uint16 tensor on x's device, wtab 256 host weights -> int32 (N,C,h,w).  The library checks the argument ranges (ELD_EINVAL -> EldError)."""
    import torch
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError('x must be a CUDA float32 tensor (N, C, h, w)')
    x = x if x.is_contiguous() else x.contiguous()
    N, C, h, w = (int(v) for v in x.shape)
    if tuple(fwd.shape) != (C, 65536) or fwd.element_size() != 2 or fwd.device != x.device or not fwd.is_contiguous():
        raise ValueError('fwd must be a contiguous 16-bit tensor (%d, 65536) on %s' % (C, x.device))
    wt = np.ascontiguousarray(np.asarray(wtab).reshape(-1), dtype=np.uint16)
    if wt.size != 256:
        raise ValueError('wtab takes 256 weights, got %d' % wt.size)
    if out is None:
        out = torch.empty((N, C, h, w), dtype=torch.int32, device=x.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (N, C, h, w) or out.device != x.device or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor of x\'s shape and device')
    with torch.cuda.device(x.device):
        L.check(L.lib().eld_nlm_vst_f32(L.dptr(x), N, C, h, w, float(qscale), L.dptr(fwd), int(S), int(P), int(sh),
                                        wt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), int(frac), L.dptr(out), L.cur_stream()), 'eld_nlm_vst_f32')
    return out


def bm3d_vst(x, qscale, fwd, guide, S, step, Gmax, mix, tau, par, win, frac, out=None):
    """eld_bm3d_vst_f32 on CUDA tensors: x and fwd as for nlm_vst; guide None (step 1: hard threshold, par the thresholds) or step 1's int32
    output (step 2: Wiener, par the noise energies); par 5 and win 64 host values -> int32 (N,C,h,w) in units of 2^-frac of a stabilised code.
    The workspace is allocated here; the library checks the argument ranges (ELD_EINVAL -> EldError)."""
    import torch
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
        raise ValueError('x must be a CUDA float32 tensor (N, C, h, w)')
    x = x if x.is_contiguous() else x.contiguous()
    N, C, h, w = (int(v) for v in x.shape)
    if tuple(fwd.shape) != (C, 65536) or fwd.element_size() != 2 or fwd.device != x.device or not fwd.is_contiguous():
        raise ValueError('fwd must be a contiguous 16-bit tensor (%d, 65536) on %s' % (C, x.device))
    if guide is not None and (guide.dtype != torch.int32 or tuple(guide.shape) != (N, C, h, w) or guide.device != x.device or not guide.is_contiguous()):
        raise ValueError('guide must be a contiguous int32 tensor of x\'s shape and device')
    pr = np.ascontiguousarray(np.asarray(par).reshape(-1), dtype=np.uint32)
    wn = np.ascontiguousarray(np.asarray(win).reshape(-1), dtype=np.uint8)
    if pr.size != 5 or wn.size != 64:
        raise ValueError('par takes 5 values and win 64, got %d and %d' % (pr.size, wn.size))
    if not (0 <= int(tau) < 1 << 32):
        raise ValueError('tau must fit 32 bits, got %r' % (tau,))
    if out is None:
        out = torch.empty((N, C, h, w), dtype=torch.int32, device=x.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (N, C, h, w) or out.device != x.device or not out.is_contiguous():
        raise ValueError('out must be a contiguous int32 tensor of x\'s shape and device')
    need = int(L.lib().eld_bm3d_vst_workspace_bytes(N, C, h, w))
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().eld_bm3d_vst_f32(L.dptr(x), N, C, h, w, float(qscale), L.dptr(fwd), None if guide is None else L.dptr(guide), int(S), int(step),
                                         int(Gmax), int(mix), int(tau), pr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                         wn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), int(frac), L.dptr(out), L.dptr(ws), need, L.cur_stream()),
                'eld_bm3d_vst_f32')
    return out


# ---- the denoiser ---------------------------------------------------------------------------------------------------------------------------
def camera_table(camera):
    """A calibrated table: the dict itself, the name of a table (camera_params/release/<name>_params.npy of the working directory, else the
    tables shipped with the package) or the path of a <name>_params.npy file."""
    if isinstance(camera, dict):
        return camera
    if isinstance(camera, (str, os.PathLike)):
        camera = os.fspath(camera)
        if camera.endswith('.npy'):
            if not os.path.exists(camera):
                raise ValueError('no such camera table: %s' % camera)
            return np.load(camera, allow_pickle=True).item()
        from .noise import load_camera_params
        try:
            return load_camera_params(camera, os.path.join('camera_params', 'release'))
        except KeyError:
            raise ValueError('no camera table named %r' % camera)
    raise ValueError('camera must be a table (dict), a table\'s name or the path of a _params.npy file, got %r' % (type(camera).__name__,))


def sigma_from_table(camera, K):
    """The read noise in DN the table's 'Profile-1' g_scale line gives at log K: exp(slope log K + bias)."""
    K = _check_noise(K, 0.0)[0]
    try:
        line = camera_table(camera)['Profile-1']['g_scale']
        slope, bias = float(line['slope']), float(line['bias'])
    except (KeyError, TypeError):
        raise ValueError("the camera table has no 'Profile-1' g_scale line")
    return math.exp(slope * math.log(K) + bias)


class ClassicalDenoiser:
    """The baseline as denoise_raw and evaluate_pairs take it in place of a Denoiser.

    cfa       'bayer' or 'xtrans': in_channels = out_channels = its plane count
    K, sigma  overall system gain and read noise (Gaussian, signal-independent) in DN; sigma None: from `camera` (sigma_from_table)
    search, patch   the radii S and P: candidates within |d| <= search, patches of (2 patch + 1)^2 sites in every plane
    strength  the filter parameter in units of the noise standard deviation per patch term
    method    'nlm' (search 7, patch 2, strength 0.5 by default) or 'bm3d' (search 12 at most 16, strength 1.0; blocks are 8 x 8, so a
              patch other than the default is refused): the filter in the stabilised domain; `label` holds the same word
    step, group, mix   BM3D only: the stride of the reference blocks (1 to 8), the largest group (1, 2, 4, 8 or 16 blocks) and whether the
              transform also runs across the planes (None: when their number is a power of two -- Bayer yes, X-Trans no)"""
    is_classical = True

    def __init__(self, cfa, K, sigma=None, camera=None, search=None, patch=2, strength=None, method='nlm', step=3, group=16, mix=None):
        from .mosaic import PLANES, check_cfa
        check_cfa(cfa)
        if method not in METHODS:
            raise ValueError('method must be one of %r, got %r' % (METHODS, method))
        bm3d = method == 'bm3d'
        if search is None:
            search = 12 if bm3d else 7
        if strength is None:
            strength = 1.0 if bm3d else 0.5
        if sigma is None:
            if camera is None:
                raise ValueError('ClassicalDenoiser needs sigma, or a camera table to read it from')
            sigma = sigma_from_table(camera, K)
            self._camera = camera                                # with_gain reads the line again at another K
        else:
            self._camera = None
        self.K, self.sigma = _check_noise(K, sigma)
        for name, v, top in (('search', search, BM3D_MAX_SEARCH if bm3d else MAX_SEARCH), ('patch', patch, MAX_PATCH)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (0 <= v <= top):
                raise ValueError('%s must be an integer in [0, %d], got %r' % (name, top, v))
        self.cfa, self.search, self.patch, self.strength = cfa, int(search), int(patch), float(strength)
        self.planes = PLANES[cfa]
        self.method = self.label = method
        if bm3d:
            if self.patch != 2:
                raise ValueError('BM3D blocks are %d x %d: patch takes no value but its default, got %r' % (BM3D_BLOCK, BM3D_BLOCK, patch))
            if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not (1 <= step <= BM3D_MAX_STEP):
                raise ValueError('step must be an integer in [1, %d], got %r' % (BM3D_MAX_STEP, step))
            if isinstance(group, bool) or group not in BM3D_GROUPS:
                raise ValueError('group must be one of %r, got %r' % (BM3D_GROUPS, group))
            pow2 = self.planes & (self.planes - 1) == 0
            if mix is None:
                mix = pow2
            if mix not in (False, True, 0, 1):
                raise ValueError('mix must be None, False or True, got %r' % (mix,))
            if mix and not pow2:
                raise ValueError('grouping across the planes needs a power-of-two number of them: %s has %d' % (cfa, self.planes))
            self.step, self.group, self.mix = int(step), int(group), bool(mix)
            self.tables = bm3d_tables(self.planes, self.mix, self.strength)
        else:
            self.sh, self.wtab = nlm_weight_table(self.planes, self.patch, self.strength)
        self._fwd = {}
        self._others = {}

    @classmethod
    def from_frames(cls, frames, cfa, raw_pattern=None, black_level=None, white_level=16383, defects=None, sigma=None, camera=None, **kw):
        """The baseline with K estimated from the frames themselves (eld_amd.noiselevel.estimate_noise: uint16 frames of one ISO, NumPy or
        CUDA), and the read noise too unless `sigma` or `camera` gives one; **kw as the constructor's.  The estimate is kept as
        `.estimate`."""
        from .noiselevel import estimate_noise
        est = estimate_noise(frames, cfa, raw_pattern, black_level, white_level, defects)
        den = cls(cfa, est.K, sigma=est.sigma if sigma is None and camera is None else sigma, camera=camera, **kw)
        den.estimate = est
        return den

    def with_gain(self, K):
        """This baseline at another gain (another ISO): the read noise again from the camera table where it came from one, else kept."""
        K = float(K)
        if K == self.K:
            return self
        if K not in self._others:
            self._others[K] = ClassicalDenoiser(self.cfa, K, sigma=None if self._camera is not None else self.sigma, camera=self._camera,
                                                search=self.search, patch=self.patch, strength=self.strength, **self._method_args())
        return self._others[K]

    def _method_args(self):
        return dict(method='bm3d', step=self.step, group=self.group, mix=self.mix) if self.method == 'bm3d' else {}

    @property
    def in_channels(self):
        return self.planes

    @property
    def out_channels(self):
        return self.planes

    def black_per_plane(self, black_level):
        """mosaic.levels' black levels (4 for Bayer, in colour-code order = plane order; one for X-Trans) -> one per packed plane"""
        b = [float(v) for v in black_level]
        return b if self.cfa == 'bayer' else [b[0]] * self.planes

    def fwd_on(self, device, black_level):
        """The forward tables for these black levels as an int16-view tensor (C, 65536) on `device`, built and uploaded once."""
        import torch
        key = (torch.device(device), tuple(self.black_per_plane(black_level)))
        if key not in self._fwd:
            self._fwd[key] = torch.from_numpy(vst_tables(self.K, self.sigma, key[1]).view(np.int16)).to(device)
        return self._fwd[key]

    def pack_codes(self, t3, raw_pattern, black_level, shading=None, tval=None, flatfield=None):
        """CUDA int16-view codes (N,Hm,Wm) -> the corrected sensor codes of every packed plane over 65535, float32 (N,C,h,w), unclipped at
        the black level: denoise.pack_input with black 0, white 65535 and ratio 1.  A flat-field gain g must multiply the signal above black
        only, so what it did to the pedestal is taken back: x - (g - 1) * black / 65535 in float32."""
        import torch
        from .denoise import pack_input
        N = int(t3.shape[0])
        zero = [0.0] * len(black_level)
        if flatfield is None:
            return pack_input(t3, self.cfa, raw_pattern, zero, 65535.0, [1.0] * N, shading, tval)
        x = pack_input(t3, self.cfa, raw_pattern, zero, 65535.0, [1.0] * N, shading, tval, flatfield)
        bq = torch.tensor(self.black_per_plane(black_level), dtype=torch.float32, device=x.device).reshape(1, -1, 1, 1) / 65535.0
        return x - (flatfield.packed(x.device, 'prnu') - 1.0) * bq

    def filter_planes(self, x, black_level, ratios, white_point):
        """The corrected codes over 65535 (pack_codes) -> float32 (N,C,h,w) in the network's output convention."""
        import torch
        fwd = self.fwd_on(x.device, black_level)
        if self.method == 'bm3d':
            h, w = int(x.shape[2]), int(x.shape[3])
            if h < BM3D_BLOCK or w < BM3D_BLOCK:
                raise ValueError('BM3D needs packed planes of at least %d x %d sites, this frame packs to %d x %d' % (BM3D_BLOCK, BM3D_BLOCK, h, w))
            tau1, thr, tau2, s2, win = self.tables
            first = bm3d_vst(x, 65535.0, fwd, None, self.search, self.step, self.group, self.mix, tau1, thr, win, FRAC)
            out = bm3d_vst(x, 65535.0, fwd, first, self.search, self.step, self.group, self.mix, tau2, s2, win, FRAC)
        else:
            out = nlm_vst(x, 65535.0, fwd, self.search, self.patch, self.sh, self.wtab, FRAC)
        z = unbiased_inverse(out, FRAC, self.K, self.sigma)
        blk = torch.tensor(self.black_per_plane(black_level), dtype=torch.float64, device=x.device).reshape(1, -1, 1, 1)
        r = torch.as_tensor(np.asarray(ratios, np.float64).reshape(-1), device=x.device).reshape(-1, 1, 1, 1)
        return (z * r / (float(white_point) - blk)).to(torch.float32)

    def denoise_codes(self, t3, raw_pattern, black_level, white_point, ratios, shading=None, tval=None, flatfield=None):
        """CUDA int16-view codes (N,Hm,Wm), as denoise.pack_input takes them -> the denoised packed planes (N,C,h,w) float32: plane c is
        z * ratio[n] / (white - black_c), z the estimate of the clean signal in DN above black."""
        return self.filter_planes(self.pack_codes(t3, raw_pattern, black_level, shading, tval, flatfield), black_level, ratios, white_point)


# ---- command line ---------------------------------------------------------------------------------------------------------------------------
def _gain_arg(text):
    """--K: a float, or the word 'auto' (anything else is the parser's error)."""
    return 'auto' if text == 'auto' else float(text)


def build_parser():
    from . import denoise as D
    p = D.build_parser()
    p.prog = 'python -m eld_amd.classical'
    p.description = 'Denoise uint16 raw mosaics (.npy) without a checkpoint: Anscombe transform + non-local means + unbiased inverse.'
    for act in p._actions:
        if act.dest == 'ckpt':
            act.required = False
            act.help = 'ignored: the classical baseline loads no checkpoint'
    p.add_argument('--K', type=_gain_arg, required=True, metavar='K|auto',
                   help="overall system gain in DN per electron (eld_amd.calibrate, eld_amd.burst), or 'auto': estimated from the input frames "
                        '(eld_amd.noiselevel), and with it the read noise unless --sigma or --camera gives one')
    p.add_argument('--sigma', type=float, help='read noise in DN (default: the g_scale line of --camera at log K)')
    p.add_argument('--camera', metavar='TABLE', help="a calibrated table: a name (camera_params/release/<name>_params.npy or a shipped one) or a .npy path")
    p.add_argument('--search', type=int, default=7, help='search radius (default 7, at most %d; with --method bm3d 12, at most %d)'
                                                          % (MAX_SEARCH, BM3D_MAX_SEARCH))
    p.add_argument('--patch', type=int, default=2, help='patch radius (default 2, at most %d; --method bm3d takes no other)' % MAX_PATCH)
    p.add_argument('--strength', type=float, default=0.5, help='filter strength in noise standard deviations (default 0.5; with --method bm3d 1.0)')
    p.add_argument('--method', choices=METHODS, default='nlm', help='the filter in the stabilised domain (default nlm)')
    p.add_argument('--step', type=int, default=3, help='bm3d: stride of the reference blocks (default 3, at most %d)' % BM3D_MAX_STEP)
    p.add_argument('--group', type=int, default=16, help='bm3d: the largest group, 1, 2, 4, 8 or 16 blocks (default 16)')
    p.add_argument('--no-mix', action='store_true', help='bm3d: transform every plane alone (default: across the planes when their number is a power of two)')
    return p


def parse_method_args(parser, argv, method_dest='method', prefix=''):
    """Parse, and where the method is bm3d parse again with that method's defaults for the search radius and the strength."""
    a = parser.parse_args(argv)
    if getattr(a, method_dest) == 'bm3d':
        parser.set_defaults(**{prefix + 'search': 12, prefix + 'strength': 1.0})
        a = parser.parse_args(argv)
    return a


def main(argv=None):
    from . import denoise as D
    a = parse_method_args(build_parser(), sys.argv[1:] if argv is None else argv)
    auto = a.K == 'auto'
    if a.sigma is None and a.camera is None and not auto:
        raise ValueError('the baseline needs --sigma or --camera (or --K auto, which estimates both)')
    if a.bf16:
        raise ValueError('--bf16 is the network\'s precision: the classical baseline runs in integers')
    inputs, outdir, _, o = D.options_from(a)
    K, sigma = a.K, a.sigma
    if auto:
        from .burst import load_burst
        from .noiselevel import estimate_from_options
        est = estimate_from_options(load_burst(inputs), o)
        K = est.K
        if a.sigma is None and a.camera is None:
            sigma = est.sigma
        print('estimated from the input frames: K %.5g DN/e-, sigma %.4g DN (%.0f %% of the tiles kept, %d points)'
              % (est.K, est.sigma, 100 * est.kept_share, len(est.points['bin'])))
    den = ClassicalDenoiser(o['cfa'], K, sigma=sigma, camera=a.camera, search=a.search, patch=a.patch, strength=a.strength, method=a.method,
                            step=a.step, group=a.group, mix=False if a.no_mix else None)
    if auto:
        print('using K %.5g DN/e-, sigma %.4g DN' % (den.K, den.sigma))
    return D.run_frames(den, inputs, outdir, o)


if __name__ == '__main__':
    sys.exit(main())
