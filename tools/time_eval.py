"""Per-image cost of the runner's evaluation, host indices against device indices, in one process: the K = 2 forward plus the indices of
every image of a batch, synchronised (the host path ends with its numpy scores, the device path with the one copy of its rows).
Reduced resolution (PSNR / SSIM / Q / SAM / ERGAS): PAN 128^2 at C = 4 and 8, batch 1 (the reference's test loaders) and 32.
Full resolution (D_lambda / D_s / QNR): the 400^2 scene at C = 4 and 8, batch 1.  Every shape is warmed up before it is timed.
The extended leg (cfg.eval_indices = 'extended': + Q2n / SCC / CC, + D_lambda_K / HQNR) times forward alone / standard device / extended
device / extended host of every case in alternating rounds, so that a drift of the box falls on all four alike; the extended device figure
is to be read against the standard device figure of the same run and against the extended host figure.
Prints one JSON line.   python tools/time_eval.py [--reps N] [--rounds R]"""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gpu_helpers import make_module  # noqa: E402
from lgteun_amd import device_metrics as dmt  # noqa: E402
from lgteun_amd import metrics as mtc  # noqa: E402
from oracle import detweights as dw  # noqa: E402

PEAK = 2047.5
CASES = [('ref_128_c4_b1', True, 4, 32, 1), ('ref_128_c4_b32', True, 4, 32, 32), ('ref_128_c8_b1', True, 8, 32, 1),
         ('ref_128_c8_b32', True, 8, 32, 32), ('noref_400_c4_b1', False, 4, 100, 1), ('noref_400_c8_b1', False, 8, 100, 1)]


def host_np(t):
    return (t * PEAK).permute(0, 2, 3, 1).cpu().numpy()


def run(net, ref, ms, pan, gt, how):
    with torch.no_grad():
        out = net(ms, pan)
        if how == 'forward':
            torch.cuda.synchronize()
            return None
        if how == 'device':
            rows = dmt.ref_evaluate_batch(out, gt, PEAK) if ref else dmt.no_ref_evaluate_batch(out, pan, ms, PEAK)
            return rows.cpu().numpy()
        if how == 'device_ext':
            rows = dmt.ref_evaluate_ext_batch(out, gt, PEAK) if ref else dmt.no_ref_evaluate_ext_batch(out, pan, ms, PEAK)
            return rows.cpu().numpy()
        o = host_np(out)
        if ref:
            g = host_np(gt)
            score = mtc.ref_evaluate_ext if how == 'host_ext' else mtc.ref_evaluate
            return np.array([score(o[i], g[i]) for i in range(o.shape[0])])
        p, m = host_np(pan), host_np(ms)
        score = mtc.no_ref_evaluate_ext if how == 'host_ext' else mtc.no_ref_evaluate
        return np.array([score(o[i], p[i], m[i]) for i in range(o.shape[0])])


def per_image_ms(fn, B, reps):
    for _ in range(3):                     # warm-up of this shape (plans, workspaces, allocator)
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps / B * 1e3


def alternating_ms(legs, B, rounds):
    """legs: {name: (fn, repetitions per round)} -> {name: ms per image}, the median over `rounds` rounds that time every leg in turn"""
    for fn, _ in legs.values():
        for _ in range(3):
            fn()
    seen = {name: [] for name in legs}
    for _ in range(rounds):
        for name, (fn, n) in legs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(n):
                fn()
            seen[name].append((time.perf_counter() - t) / n / B * 1e3)
    return {name: float(np.median(v)) for name, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20, help='timed repetitions of the forward and device paths (host path: fewer)')
    ap.add_argument('--rounds', type=int, default=5, help='alternating rounds of the extended leg')
    a = ap.parse_args()
    nets, res = {}, {}
    for name, ref, C, h, B in CASES:
        net = nets.setdefault(C, make_module(C, K=2))
        ms, pan, gt = (torch.from_numpy(x).cuda() for x in dw.make_inputs(B, C, h, h, seed=7, kind='smooth'))
        host_reps = max(1, min(a.reps, 8 // B if ref else 2))
        row = {'forward_ms': per_image_ms(lambda: run(net, ref, ms, pan, gt, 'forward'), B, a.reps),
               'device_ms': per_image_ms(lambda: run(net, ref, ms, pan, gt, 'device'), B, a.reps),
               'host_ms': per_image_ms(lambda: run(net, ref, ms, pan, gt, 'host'), B, host_reps)}
        d, hst = run(net, ref, ms, pan, gt, 'device'), run(net, ref, ms, pan, gt, 'host')
        row['max_abs_diff'] = float(np.max(np.abs(d - hst)[np.isfinite(hst)]))
        row['speedup'] = row['host_ms'] / row['device_ms']
        res[name] = {k: round(v, 4) if k != 'max_abs_diff' else v for k, v in row.items()}
        leg = lambda how, n: (lambda: run(net, ref, ms, pan, gt, how), n)      # noqa: E731
        ext = alternating_ms({'forward_ms': leg('forward', a.reps), 'device_ms': leg('device', a.reps), 'device_ext_ms': leg('device_ext', a.reps),
                              'host_ext_ms': leg('host_ext', 1)}, B, a.rounds)
        d, hst = run(net, ref, ms, pan, gt, 'device_ext'), run(net, ref, ms, pan, gt, 'host_ext')
        res[name]['extended'] = {k: round(v, 4) for k, v in ext.items()}
        res[name]['extended']['max_abs_diff'] = float(np.max(np.abs(d - hst)[np.isfinite(hst)]))
    print(json.dumps({'tool': 'time_eval', 'unit': 'ms per image (forward K = 2 + indices, synchronised)',
                      'device': torch.cuda.get_device_name(0), 'cases': res}))


if __name__ == '__main__':
    main()
