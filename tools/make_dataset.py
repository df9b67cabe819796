"""From one raw scene to a training set, on the GPU (lgteun_amd/wald.py): Wald's protocol -- low-pass with the sensor's MTF gains, decimate
MS and PAN by 4, keep the raw MS as the target -- and, on request, the windows as the <id>_lr.tif / _pan.tif / _mul.tif triplets PSDataset reads.

    python tools/make_dataset.py --ms scene_ms.tif --pan scene_pan.tif --out train/ --patch 128 --step 32 --region 0 0 4096 8192
    python tools/make_dataset.py --ms scene_ms.tif --pan scene_pan.tif --out test/  --patch 128 --step 128 --region 4096 0 8192 8192
    python tools/make_dataset.py --ms scene_ms.tif --pan scene_pan.tif --out full/  --patch 512 --step 512 --no-degrade      # raw pairs, no target
    python tools/make_dataset.py --ms scene_ms.tif --pan scene_pan.tif --degraded-out lowres/                                # the degraded scene only

Training needs no files at all: a `SceneDataset` entry in the configuration (dataset.build_loader) cuts the same windows out of the scene
on the device.  --gains-ms / --gain-pan are the sensor's MTF gains at Nyquist, per band; without them 0.3 (MS) and 0.15 (PAN) are used,
which are defaults and no sensor's measured values.  --region y0 x0 y1 x1 and --step are in pixels of the grid the windows are cut on (the
raw MS grid after degradation, the raw PAN grid with --no-degrade), multiples of 4.  Prints one JSON line."""
import argparse
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--ms', required=True, help='the raw MS scene, a TIFF [h, w, C]')
    ap.add_argument('--pan', required=True, help='the raw PAN scene, a TIFF [4h, 4w]')
    ap.add_argument('--out', help='directory for the triplets')
    ap.add_argument('--degraded-out', help='directory for the degraded scene itself (lr.tif, pan.tif)')
    ap.add_argument('--patch', type=int, default=128)
    ap.add_argument('--step', type=int, default=32)
    ap.add_argument('--region', type=int, nargs=4, metavar=('Y0', 'X0', 'Y1', 'X1'))
    ap.add_argument('--gains-ms', type=float, nargs='+', help='one MTF gain per band, or one for all')
    ap.add_argument('--gain-pan', type=float)
    ap.add_argument('--phase', type=int, default=2, help='decimation phase, 0 .. 3')
    ap.add_argument('--taps', type=int, default=41)
    ap.add_argument('--no-degrade', action='store_true', help='cut the raw full-resolution pair (no target)')
    ap.add_argument('--device', default='cuda:0')
    a = ap.parse_args()
    if not a.out and not a.degraded_out:
        ap.error('nothing to write: give --out and / or --degraded-out')
    from lgteun_amd import wald
    from lgteun_amd.dataset import write_tiff
    ms, pan = wald.read_scene(a.ms, a.pan)
    gains = None if a.gains_ms is None else (a.gains_ms[0] if len(a.gains_ms) == 1 else a.gains_ms)
    store = wald.SceneStore.from_scene(ms, pan, a.device, degrade=not a.no_degrade, gains_ms=gains, gain_pan=a.gain_pan, phase=a.phase, n_taps=a.taps)
    out = dict(tool='make_dataset', sample_type=store.kind, bands=store.C, grid=[store.Hs, store.Ws], degraded=not a.no_degrade)
    if a.degraded_out:
        os.makedirs(a.degraded_out, exist_ok=True)
        write_tiff(os.path.join(a.degraded_out, 'lr.tif'), wald._as_numpy(store.lr, store.kind).transpose(1, 2, 0))
        write_tiff(os.path.join(a.degraded_out, 'pan.tif'), wald._as_numpy(store.pan, store.kind)[0])
        out['degraded_out'] = a.degraded_out
    if a.out:
        org = wald.window_origins(store.Hs, store.Ws, a.patch, a.step, a.region)
        ids = wald.export_triplets(store, org, a.out, a.patch)
        out.update(out=a.out, windows=len(ids), patch=a.patch, step=a.step, first=ids[0], last=ids[-1])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
