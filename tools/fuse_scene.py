"""Pan-sharpen one scene of any size with a trained network or with a classical method: reads PREFIX_lr.tif (MS, [h,w,C]) and PREFIX_pan.tif ([4h,4w]) with
dataset.read_tiff, fuses them tile by tile on the GPU (lgteun_amd/scene.py) and writes PREFIX_mul_hat.tif.

    python tools/fuse_scene.py PREFIX --checkpoint model.state.pth [--tile 128] [--overlap 32] [--bit-depth 11] [--norm-input]
                               [--batch B] [--float] [--out FILE]
    python tools/fuse_scene.py PREFIX --method gsa|sfim|wavelet [--bit-depth 11] [--norm-input] [--float] [--out FILE]
    python tools/fuse_scene.py PREFIX --method mtf_glp|mtf_glp_hpm|mtf_glp_cbd [--mtf-gains g [g ...]] [--bit-depth 11] ...
    python tools/fuse_scene.py PREFIX --method ihs|brovey|gs|pca [--cs-weights w [w ...]] [--bit-depth 11] ...
    python tools/fuse_scene.py PREFIX --method bdsd [--bdsd-block N] [--mtf-gains g [g ...]] [--mtf-gain-pan g] [--bit-depth 11] ...
    python tools/fuse_scene.py PREFIX --method atwt|awlp [--atrous-match pan|lowpass] [--bit-depth 11] ...
    python tools/fuse_scene.py PREFIX --method fs|hpm_r|hpm_h|bt_h [--mtf-gains g [g ...]] [--mtf-gain-pan g] [--bit-depth 11] ...

--method gsa / sfim / wavelet (lgteun_amd/classical.py) and mtf_glp / mtf_glp_hpm / mtf_glp_cbd (lgteun_amd/mtf_glp.py) need no checkpoint and no
tiles: the whole scene is fused in one call, with the same normalisation and the same conversion to digital numbers.  --mtf-gains: the sensor's MTF
gains at Nyquist, one for all bands or one per band; without them a placeholder (0.3) applies, which is no sensor's value.  --method bdsd
(lgteun_amd/bdsd.py) takes them too, with --mtf-gain-pan for PAN (placeholder 0.15), and --bdsd-block N fits its weights per block of N x N PAN pixels (a
multiple of 32 that divides both sides of PAN; without it one fit serves the whole scene).  --method ihs / brovey / gs / pca (lgteun_amd/cs.py) are the
component-substitution baselines; --cs-weights gives the intensity weights of the first three, one per band (without them 1 / C each).  --method fs / hpm_r /
hpm_h / bt_h (lgteun_amd/mtf_hr.py) are the regression-based and haze-corrected MTF rules: the first three take --mtf-gains, bt_h takes --mtf-gain-pan.

The checkpoint is a plain-tensor file ({'core_module': state_dict}, what Base_model.save writes and tools/convert_checkpoint.py makes of a
reference-era file); the band count and the stage count are read from it.  The output holds uint16 digital numbers
(rint(x * (2**bit_depth - 0.5)), clipped) unless --float asks for the normalised float32 image."""
import argparse
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lgteun_amd  # noqa: E402
from lgteun_amd.compat import Config  # noqa: E402
from lgteun_amd.dataset import read_tiff, write_tiff  # noqa: E402


def load_module(path, device='cuda:0'):
    ckpt = torch.load(path, map_location='cpu', weights_only=True)
    sd = ckpt['core_module'] if 'core_module' in ckpt else ckpt
    C = int(sd['R.weight'].shape[1])
    K = sum(1 for k in sd if k.startswith('eta.'))
    net = lgteun_amd.Pansharpening(Config(ms_chans=C), None, stage=K)
    net.load_state_dict(sd)
    return net.to(device).eval()


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('prefix')
    ap.add_argument('--method', choices=['network', 'gsa', 'sfim', 'wavelet', 'mtf_glp', 'mtf_glp_hpm', 'mtf_glp_cbd', 'bdsd', 'ihs', 'brovey', 'gs', 'pca',
                                         'atwt', 'awlp', 'fs', 'hpm_r', 'hpm_h', 'bt_h'], default='network')
    ap.add_argument('--atrous-match', choices=['pan', 'lowpass'], default='pan',
                    help="--method atwt / awlp: the deviation the detail is scaled by, std(pan) or std of the low-passed PAN (default: pan)")
    ap.add_argument('--mtf-gains', type=float, nargs='+', default=None, metavar='g',
                    help="--method mtf_glp* / bdsd / fs / hpm_r / hpm_h: the sensor's MTF gain at Nyquist, one for all bands or one per band (default: a placeholder, 0.3)")
    ap.add_argument('--mtf-gain-pan', type=float, default=None, metavar='g', help="--method bdsd / bt_h: PAN's MTF gain at Nyquist (default: a placeholder, 0.15)")
    ap.add_argument('--bdsd-block', type=int, default=None, metavar='N',
                    help='--method bdsd: fit the weights per block of N x N PAN pixels, N a multiple of 32 that divides both sides (default: one global fit)')
    ap.add_argument('--cs-weights', type=float, nargs='+', default=None, metavar='w',
                    help='--method ihs / brovey / gs: the intensity weights, one per band, used as given (default: 1 / C each)')
    ap.add_argument('--checkpoint', default=None, help='required for --method network')
    ap.add_argument('--tile', type=int, nargs='+', default=[128], help='one side, or height and width')
    ap.add_argument('--overlap', type=int, default=32)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--bit-depth', type=int, default=11)
    ap.add_argument('--norm-input', action='store_true', help="the dataset's extra division (cfg.norm_input of the training run)")
    ap.add_argument('--float', action='store_true', help='write the normalised float32 image instead of uint16 digital numbers')
    ap.add_argument('--out', default=None)
    return ap


def main():
    ap = parser()
    a = ap.parse_args()
    if len(a.tile) > 2:
        ap.error('--tile takes one or two values')
    if a.method == 'network' and not a.checkpoint:
        ap.error('--method network needs --checkpoint')
    tile = a.tile[0] if len(a.tile) == 1 else tuple(a.tile)
    ms, pan = read_tiff(f'{a.prefix}_lr.tif'), read_tiff(f'{a.prefix}_pan.tif')
    if ms.ndim != 3 or pan.ndim != 2:
        sys.exit(f'{a.prefix}: expected MS [h,w,C] and PAN [4h,4w], got {ms.shape} / {pan.shape}')
    if ms.dtype != pan.dtype or ms.dtype.name not in ('uint8', 'uint16'):
        ms, pan = ms.astype(np.float64).astype(np.float32), pan.astype(np.float64).astype(np.float32)      # like PSDataset
    ms_chw = np.ascontiguousarray(ms.transpose(2, 0, 1))
    gains = a.mtf_gains[0] if a.mtf_gains is not None and len(a.mtf_gains) == 1 else a.mtf_gains
    if a.method == 'bdsd':
        from lgteun_amd import bdsd
        fused = bdsd.fuse_scene(ms_chw, pan[np.newaxis], block=a.bdsd_block, gains_ms=gains, gain_pan=a.mtf_gain_pan, bit_depth=a.bit_depth,
                                norm_input=a.norm_input, out_dtype='float32' if a.float else 'uint16')
    elif a.method in ('ihs', 'brovey', 'gs', 'pca'):
        from lgteun_amd import cs
        fused = cs.fuse_scene(a.method, ms_chw, pan[np.newaxis], weights=a.cs_weights, bit_depth=a.bit_depth, norm_input=a.norm_input,
                              out_dtype='float32' if a.float else 'uint16')
    elif a.method in ('atwt', 'awlp'):
        from lgteun_amd import atrous
        fused = atrous.fuse_scene(atrous.SCENE_METHODS[a.method], ms_chw, pan[np.newaxis], match=a.atrous_match, bit_depth=a.bit_depth,
                                  norm_input=a.norm_input, out_dtype='float32' if a.float else 'uint16')
    elif a.method in ('fs', 'hpm_r', 'hpm_h', 'bt_h'):
        from lgteun_amd import mtf_hr
        fused = mtf_hr.fuse_scene(a.method, ms_chw, pan[np.newaxis], gains_ms=gains, gain_pan=a.mtf_gain_pan, bit_depth=a.bit_depth, norm_input=a.norm_input,
                                  out_dtype='float32' if a.float else 'uint16')
    elif a.method.startswith('mtf_glp'):
        from lgteun_amd import mtf_glp
        fused = mtf_glp.fuse_scene(mtf_glp.SCENE_METHODS[a.method], ms_chw, pan[np.newaxis], gains_ms=gains, bit_depth=a.bit_depth, norm_input=a.norm_input,
                                   out_dtype='float32' if a.float else 'uint16')
    elif a.method != 'network':
        from lgteun_amd import classical
        fused = classical.fuse_scene(a.method, ms_chw, pan[np.newaxis], bit_depth=a.bit_depth, norm_input=a.norm_input,
                                     out_dtype='float32' if a.float else 'uint16')
    else:
        fused = load_module(a.checkpoint).fuse_scene(ms_chw, pan[np.newaxis], tile=tile, overlap=a.overlap, batch=a.batch, bit_depth=a.bit_depth,
                                                      norm_input=a.norm_input, out_dtype='float32' if a.float else 'uint16')
    out = a.out or f'{a.prefix}_mul_hat.tif'
    write_tiff(out, fused.permute(1, 2, 0).contiguous().cpu().numpy())
    print(f'{out}: {tuple(fused.shape)} {fused.dtype}')


if __name__ == '__main__':
    main()
