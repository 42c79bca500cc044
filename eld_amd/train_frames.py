"""Train a denoiser on your own clean frames: calibrate -> train -> denoise in three commands.

    python -m eld_amd.calibrate manifest.json --camera MyCam --out tables/
    python -m eld_amd.train_frames 'long/*.npy' --meta sensor.json --camera tables/MyCam_params.npy --noise PGRU -o mycam.pt
    python -m eld_amd.denoise --ckpt mycam.pt --meta sensor.json --ratio 100 short.npy -o out/

The frames are uint16 mosaics (.npy, rawpy's raw_image_visible of clean long exposures); they are uploaded once into a FramePool
(eld_amd.framepool) and every batch is cut, synthesised and trained on the device.  --meta is the JSON sidecar eld_amd.denoise reads (cfa,
raw_pattern, black_level, white_point, or rawpy's names).  --camera is a table eld_amd.calibrate wrote (<dir>/<name>_params.npy) or the
name of a release camera.  The checkpoint is the reference's dict ({'netG': ..., 'opt_g': ..., ...}), what eld_amd.denoise.load_denoiser
reads.

--noise PDU --dark manifest.json takes the signal-independent noise from the sensor's own dark frames instead of a fitted law: the bias
frames of calibrate's manifest are uploaded as a DarkPool (eld_amd.darkpool) and the sampler adds a random crop of one of them to every
patch.  The session gains come from a calibration of that manifest; --camera still names the table NoiseModel reads."""
import argparse
import glob
import os
import sys
import types

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(prog='python -m eld_amd.train_frames', description='Train an ELD U-Net on uint16 raw mosaics (.npy) held on the GPU.')
    p.add_argument('frames', nargs='+', help='clean uint16 mosaics (.npy): files or globs')
    p.add_argument('-o', '--out', required=True, help='checkpoint to write (.pt)')
    p.add_argument('--meta', help='JSON sidecar: cfa, raw_pattern, black_level, white_point (or rawpy names)')
    p.add_argument('--cfa', choices=('bayer', 'xtrans'))
    p.add_argument('--raw-pattern', type=int, nargs=4, metavar='CODE', help='Bayer 2x2 raw_pattern, row-major')
    p.add_argument('--black', type=float, nargs='+', help='black level(s): 1 or 4 (Bayer), 1 (X-Trans)')
    p.add_argument('--white', type=float, help='white point (default 16383)')
    p.add_argument('--defects', metavar='PATH', help='a defect map written by eld_amd.defects (.npz): the frames are repaired once, at upload')
    p.add_argument('--flatfield', metavar='FILE', help="a flat-field map written by eld_amd.flatfield (.npz): the clean frames are multiplied by its "
                                                       'PRNU plane once, at upload (the dark frames carry no signal and are left alone)')
    p.add_argument('--camera', default='SonyA7S2', help='a table written by eld_amd.calibrate (<dir>/<name>_params.npy) or a release camera name')
    p.add_argument('--noise', default='PGRU', help="noise model letters of NoiseModel(model=...) (default 'PGRU')")
    p.add_argument('--dark', metavar='MANIFEST', help="calibrate's manifest JSON: its bias frames become the dark-frame pool of noise letter D (--noise PDU)")
    p.add_argument('--dark-shading', metavar='FILE', help='a dark-shading map written by eld_amd.shading (.npz): subtracted from the --dark frames at '
                                                          "upload, at each session's ISO")
    p.add_argument('--patch', type=int, default=512, help='packed patch side (default 512)')
    p.add_argument('--batch', type=int, default=1, help='patches per step (default 1)')
    p.add_argument('--epochs', type=int, default=1)
    p.add_argument('--steps', type=int, help='steps per epoch (default: as many patches as tile the frames)')
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--bf16', action='store_true', help='train the U-Net in bf16')
    p.add_argument('--seed', type=int, default=2018, help='np.random / torch / Philox seed')
    p.add_argument('--val', metavar='PAIRS', help="held-out short/long pairs (eld_amd.evaluate's pairs.json): after every epoch print their mean PSNR / SSIM "
                                                  'under the model being trained')
    return p


def noise_model(camera, letters, cfa, dark=None):
    from .noise import NoiseModel
    if camera.endswith('.npy') or os.path.exists(camera):
        name = os.path.basename(camera)
        if not name.endswith('_params.npy') or not os.path.exists(camera):
            raise ValueError('--camera: %s is not a <name>_params.npy table written by eld_amd.calibrate' % camera)
        return NoiseModel(model=letters, cameras=[name[:-len('_params.npy')]], cfa=cfa, param_dir=os.path.dirname(camera) or '.', dark=dark)
    return NoiseModel(model=letters, cameras=[camera], cfa=cfa, dark=dark)


def dark_pool(manifest, camera, letters, patch, device=None, shading=None):
    """--dark: the manifest's bias frames as a DarkPool (None without the letter D; the letter without --dark is an error, and so is --dark
    without the letter).  A --camera that is a table file is handed on, so that a manifest which does not belong to it is refused; the patch
    must fit the smallest dark frame."""
    if shading is not None and manifest is None:
        raise ValueError('--dark-shading corrects the frames of --dark: it needs --dark manifest.json')
    if 'D' not in letters:
        if manifest is not None:
            raise ValueError('--dark needs the noise letter D (--noise PDU), got --noise %s' % letters)
        return None
    if manifest is None:
        raise ValueError("--noise %s: the letter D samples the sensor's dark frames and needs --dark manifest.json" % letters)
    from .darkpool import DarkPool
    pool = DarkPool.from_manifest(manifest, K=camera if camera.endswith('.npy') else None, device=device, shading=shading)
    pool.check_patch(patch, patch)
    return pool


def val_pairs(path):
    """--val: the manifest's pairs with their mosaics loaded, or None without the flag.  A missing file or a bad manifest is a ValueError before
    anything is uploaded."""
    if path is None:
        return None
    from .evaluate import load_pairs, read_manifest
    return load_pairs(read_manifest(path)[1])


def validate_epoch(engine, pairs, cfa, o, precision):
    """Mean PSNR / SSIM of the held-out pairs under the network as it stands: evaluate_pairs(levels=False), which draws no random number and
    runs the network's inference entry point (its own workspace: nothing of the training state is touched)."""
    from .denoise import Denoiser
    from .evaluate import evaluate_pairs
    rep = evaluate_pairs(Denoiser(engine.model.netG, cfa, precision), pairs, cfa, raw_pattern=o.get('raw_pattern'), black_level=o.get('black_level'),
                         white_point=o['white_point'], levels=False)
    print('epoch %d  val PSNR %.3f  SSIM %.4f  (input %.3f %.4f, %d pairs)' % (engine.epoch, rep['mean']['psnr'], rep['mean']['ssim'],
                                                                               rep['mean']['psnr_in'], rep['mean']['ssim_in'], len(pairs)))
    return rep['mean']


def main(argv=None):
    from .denoise import read_sidecar
    a = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    val = val_pairs(a.val)
    side = read_sidecar(a.meta) if a.meta else {}
    o = {k: v for k, v in side.items() if k in ('cfa', 'raw_pattern', 'black_level', 'white_point')}
    cli = {'cfa': a.cfa, 'raw_pattern': a.raw_pattern, 'black_level': a.black, 'white_point': a.white}
    o.update({k: v for k, v in cli.items() if v is not None})
    paths = [p for pat in a.frames for p in (sorted(glob.glob(pat)) or [pat])]
    from .dng import fill_from_tags, load_frame
    fill_from_tags(o, paths)                                         # command line, then sidecar, then the first DNG's tags, then the defaults
    cfa = o.pop('cfa', None) or 'bayer'
    o.setdefault('white_point', 16383)
    mosaics = [load_frame(p) for p in paths]

    import torch
    from .engine import Engine
    from .framepool import FramePool, FramePoolLoader
    np.random.seed(a.seed)
    torch.manual_seed(a.seed)
    if a.flatfield is not None:
        o['flatfield'] = a.flatfield
    pool = FramePool(mosaics, cfa=cfa, defects=a.defects if a.defects is not None else side.get('defects'), **o)
    if pool.buffer is None:
        raise RuntimeError('eld_amd.train_frames needs a GPU: there is no CPU fallback')
    dark = dark_pool(a.dark, a.camera, a.noise, a.patch, device=pool.device, shading=a.dark_shading)
    if dark is not None and dark.cfa != cfa:
        raise ValueError('--dark: the manifest holds %s frames, the clean frames are %s' % (dark.cfa, cfa))
    nm = noise_model(a.camera, a.noise, cfa, dark=dark)
    loader = FramePoolLoader(pool, nm, a.batch, patch=a.patch, steps_per_epoch=a.steps)
    out = os.path.abspath(a.out)
    opt = types.SimpleNamespace(gpu_ids=[pool.device.index], isTrain=True, checkpoints_dir=os.path.dirname(out), name='.',
                                netG='unet', channels=pool.C, in_channels=pool.C, stage_in='raw', stage_out='raw', lr=a.lr, beta1=0.9, wd=0.0,
                                loss='l1', resume=False, chop=False, no_log=True, save_epoch_freq=10 ** 9, model='eld_model', seed=a.seed,
                                precision='bf16' if a.bf16 else 'fp32')
    engine = Engine(opt)
    engine.model.set_noise_model(nm)
    print('%d frames (%s, %.1f MB on %s), %d steps of %d x %dx%dx%d per epoch' % (len(pool), cfa, pool.elems * 2 / 1e6, pool.device, len(loader), a.batch,
                                                                                 pool.C, a.patch, a.patch))
    while engine.epoch < a.epochs:
        engine.train(loader)
        if val is not None:
            validate_epoch(engine, val, cfa, o, 'bf16' if a.bf16 else 'fp32')
    torch.save(engine.model.state_dict(), out)
    print('wrote %s' % out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
