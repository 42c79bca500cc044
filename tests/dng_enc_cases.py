"""The content the tests of the lossless-JPEG writer share (test_dng_enc_cpu.py, test_dng_enc_gpu.py): the mosaics, the tiles they are cut
into, and their category histograms from the reference's own prediction.  Nothing here imports eld_amd."""
import numpy as np

import dng_ref as R

WALK_SEED = 1


def flat(H, W, v=32768):
    """at the prediction of the first two samples (P = 16): every difference is 0, one 1-bit code"""
    return np.full((H, W), v, dtype=np.uint16)


def columns(H, W):
    """((c >> 1) & 1) * 32768: the differences along a row are +-32768 -- SSSS = 16, which carries no extra bits"""
    c = np.arange(W)
    return np.broadcast_to((((c >> 1) & 1) * 32768).astype(np.uint16), (H, W)).copy()


def ramp255(H, W):
    """(255 * ((c >> 1) + r + 1) + 32768) mod 65536: every difference is 255, eight extra bits of ones -- an FF byte wherever they align"""
    r, c = np.mgrid[0:H, 0:W]
    return ((255 * ((c >> 1) + r + 1) + 32768) & 0xFFFF).astype(np.uint16)


def walk(H, W, seed=WALK_SEED):
    """Every sample's difference is 2^s - 1 with s uniform in 1..15, accumulated modulo 65536 in the prediction order of the two-component
    JPEG at P = 16 over the whole (H, W) array taken as ONE tile: (r, c) from (r, c - 2), the first two of a row from (r - 1, c), the first
    two of all from 32768.  The extra bits are all ones: the entropy data is dense with FF bytes and with FF 00 FF 00 runs."""
    rng = np.random.default_rng(seed)
    d = ((1 << rng.integers(1, 16, size=(H, W // 2, 2))) - 1).astype(np.int64)
    first = 32768 + np.cumsum(d[:, 0, :], axis=0)                    # the first sample of each row and component
    t = first[:, None, :] + np.concatenate([np.zeros((H, 1, 2), dtype=np.int64), np.cumsum(d[:, 1:, :], axis=1)], axis=1)
    return (t & 0xFFFF).astype(np.uint16).reshape(H, W)


def tiles_of(img, tile):
    """the stored tiles of `img` in TileOffsets order, padded by edge replication as write_dng_file pads them"""
    th, tw = tile
    H, W = img.shape
    out = []
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            t = img[y0:y0 + th, x0:x0 + tw]
            out.append(np.pad(t, ((0, th - t.shape[0]), (0, tw - t.shape[1])), mode='edge'))
    return out


def ssss_hist(t, P):
    """the 17-bin category histogram of one stored tile under geometry 'nf2', predictor 1, from the reference's prediction"""
    th, tw = t.shape
    S = t.astype(np.int64).reshape(th, tw // 2, 2)
    d = (S - R._predict(S, P, 1)) & 0xFFFF
    a = np.abs(np.where(d >= 32768, d - 65536, d))
    ssss = np.zeros(d.shape, dtype=np.int64)
    for s in range(1, 17):
        ssss[a >= (1 << (s - 1))] = s
    return np.bincount(ssss.reshape(-1), minlength=17)


# name -> (mosaic, tile, bits, the least number of stuffed bytes the reference must show over all streams before a comparison counts)
def gpu_cases():
    return {
        'ramp_edges': (R.noisy_ramp(40, 56, 14, seed=3), (16, 16), 14, 0),      # 12 streams, edge padding both ways
        'ramp_large': (R.noisy_ramp(144, 272, 16, seed=4), (64, 128), 16, 16),  # 9 streams, two segments each at the default
        'flat': (flat(16, 16), (16, 16), 16, 0),
        'columns': (columns(16, 16), (16, 16), 16, 0),
        'ramp255': (ramp255(16, 16), (16, 16), 16, 16),
        'walk': (walk(32, 64), (32, 64), 16, 16),
    }
