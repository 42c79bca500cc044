"""The synthetic scene of the single-frame noise-level tests (tests/test_noiselevel_cpu.py, tests/test_noiselevel_gpu.py): a raw frame
with a known gain K and read noise sigma, smooth gradients over three decades of signal and, optionally, textured blocks."""
import numpy as np

BLACK, WHITE = 512, 16383
BAYER_FACTORS = np.array([[0.6, 1.0], [1.0, 0.45]])
XT_COLOUR = np.array([[0, 2, 1, 2, 0, 1], [1, 1, 0, 1, 1, 2], [1, 1, 2, 1, 1, 0], [2, 0, 1, 0, 2, 1], [1, 1, 2, 1, 1, 0], [1, 1, 0, 1, 1, 2]])
XT_GREEN = np.where(XT_COLOUR == 1, 1, -1).reshape(-1)           # the greens have period 3; everything else is not counted
CASES = [(2.0, 3.0, 0.2), (0.5, 1.5, 0.2), (8.0, 12.0, 0.4), (2.0, 3.0, 0.0)]     # (K, sigma, tex)


def scene_electrons(H, W, tex, rng, colour=True):
    """Electrons per site: a log ramp 4 -> 6000 across the width, times 0.6 + 0.4 sin(3.1 y / H); a share `tex` of the 64 x 64 blocks
    is multiplied by 1 + 0.5 sign(sin(x / 3) sin(y / 5)); Bayer colour factors per CFA position."""
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    e = 4.0 * (6000.0 / 4.0) ** (x / (W - 1)) * (0.6 + 0.4 * np.sin(3.1 * y / H))
    blocks = rng.random((-(-H // 64), -(-W // 64))) < tex
    on = np.repeat(np.repeat(blocks, 64, axis=0), 64, axis=1)[:H, :W]
    e = e * np.where(on, 1.0 + 0.5 * np.sign(np.sin(x / 3.0) * np.sin(y / 5.0)), 1.0)
    if colour:
        e = e * np.tile(BAYER_FACTORS, (H // 2 + 1, W // 2 + 1))[:H, :W]
    return e


def synth_frame(K, sigma, tex, seed, H=768, W=1024, colour=True):
    """u = clip(rint(K Poisson(e) + sigma N(0, 1) + black), 0, white) as uint16 (H, W)."""
    rng = np.random.default_rng(seed)
    e = scene_electrons(H, W, tex, rng, colour)
    u = K * rng.poisson(e) + sigma * rng.standard_normal((H, W)) + BLACK
    return np.clip(np.rint(u), 0, WHITE).astype(np.uint16)
