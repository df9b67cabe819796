"""What the classical baselines cost on the GPU (lgteun_amd/classical.py, lgteun_amd/mtf_glp.py, lgteun_amd/bdsd.py): ms per call of `sfim`, `gsa`, `wavelet`,
of `mtf_glp` with each of its three rules (default gains: one filtered plane per sample), of `bdsd`, global and with blocks of 128, of the four
component-substitution methods `cs.ihs`, `cs.brovey`, `cs.gs`, `cs.pca` (lgteun_amd/cs.py) and of `atrous.atwt` and `atrous.awlp` with both matches
(lgteun_amd/atrous.py) and of the four regression-based and haze-corrected MTF rules `mtf_hr.fs`, `hpm_r`, `hpm_h`, `bt_h` (lgteun_amd/mtf_hr.py), in the same run, with the call synchronised, the
median of 20 runs after 5 warm-up runs, at C = 4 and C = 8 with PAN 128 x 128 (batch 1 and batch 32) and for one 4096 x 4096 scene of C = 4.
Beside each: the bytes the passes must move (SFIM and GSA: the moments pass reads ms and pan, the apply pass reads them again and writes the
output; Wavelet: ms and pan read once, the output written once; MTF-GLP: see the comment below) divided by the time, as a fraction of the HBM bandwidth (--hbm-gbs, default 8000: the MI355X's 8 TB/s), and the ms per image of the float64
numpy restatement (tests/classical_ref.py, tests/wavelet_ref.py, ...) on the same box (--no-host skips it).  Per case also `alternating`: sfim, mtf_glp_cbd,
the two forms of bdsd, gsa, gs, pca and awlp with both matches again, one call of each per round, so that what else the machine does falls on all of them alike.  Prints one JSON line.   python tools/time_classical.py"""
import argparse
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import classical_ref as cr  # noqa: E402
import wavelet_ref as wr  # noqa: E402
import mtf_glp_ref as mr  # noqa: E402
import bdsd_ref as br  # noqa: E402
import cs_ref as csr  # noqa: E402
import atrous_ref as ar  # noqa: E402
import mtf_hr_ref as hr  # noqa: E402
from lgteun_amd import atrous, bdsd, classical, cs, mtf_glp, mtf_hr  # noqa: E402

CASES = [(1, 4, 32, 32), (32, 4, 32, 32), (1, 8, 32, 32), (32, 8, 32, 32), (1, 4, 1024, 1024)]      # B, C, h, w


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def alternating_ms(fns, warmup, runs):
    """{name: median ms per call}: one synchronised call of every function per round"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[name].append((time.perf_counter() - t) * 1e3)
    return {name: round(statistics.median(v), 4) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--hbm-gbs', type=float, default=8000.0)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    res = {}
    for B, C, h, w in CASES:
        ms_np, pan_np = cr.make_scene(C, h, w, seed=1)
        ms = torch.from_numpy(ms_np).cuda()[None].repeat(B, 1, 1, 1)
        pan = torch.from_numpy(pan_np).cuda()[None, None].repeat(B, 1, 1, 1)
        row = {}
        glp = {m: (lambda ms, pan, m=m: mtf_glp.mtf_glp(ms, pan, m), lambda ms, pan, m=m: mr.mtf_glp(ms, pan, m, [mr.EQUAL_GAIN] * ms.shape[0]))
               for m in mr.MODES}
        bd = {blk: (lambda ms, pan, blk=blk: bdsd.bdsd(ms, pan, blk), lambda ms, pan, blk=blk: br.bdsd(ms, pan, [br.EQUAL_GAIN] * ms.shape[0], blk))
              for blk in (None, 128)}
        at = {(r, m): (lambda ms, pan, r=r, m=m: atrous.atrous(ms, pan, r, m), lambda ms, pan, r=r, m=m: ar.atrous(ms, pan, r, m))
              for r in ar.RULES for m in ar.MATCHES}
        mh = {r: (lambda ms, pan, r=r: mtf_hr.fuse(ms, pan, r), lambda ms, pan, r=r: hr.mtf_hr(ms, pan, r)) for r in hr.RULES}
        for name, fn, host, reads in (('sfim', classical.sfim, cr.sfim, 2), ('gsa', classical.gsa, cr.gsa, 2), ('wavelet', classical.wavelet, wr.wavelet, 1),
                                      ('mtf_glp', *glp['glp'], 2), ('mtf_glp_hpm', *glp['hpm'], 2), ('mtf_glp_cbd', *glp['cbd'], 3),
                                      ('bdsd', *bd[None], 3), ('bdsd_128', *bd[128], 3),
                                      *((m, getattr(cs, m), (lambda ms, pan, m=m: csr.fuse(ms, pan, m)), 2) for m in cs.SCENE_METHODS),
                                      *((r if m == 'pan' else f'{r}_lowpass', *at[r, m], 2 if m == 'pan' else 3) for r in ar.RULES for m in ar.MATCHES),
                                      *((r, *mh[r], 2 if r in hr.HAZE_RULES else 3) for r in hr.RULES)):
            moved = 4 * B * (reads * (C * h * w + 16 * h * w) + C * 16 * h * w)
            if name.startswith('mtf_glp'):
                # equal gains: ms is read by the moments pass, by cbd's second moments pass and by the apply pass; pan by the moments pass, the low-pass and
                # the apply pass; the one fp64 plane D is written once and read by the apply pass and by cbd's second moments pass
                moved = B * (4 * reads * C * h * w + 4 * 3 * 16 * h * w + 8 * reads * h * w + 4 * C * 16 * h * w)
            if name.startswith('bdsd'):
                # ms is read by its low-pass, by the Gram pass and by the apply pass; pan by its low-pass and by the apply pass; the fp64 planes D and A_k are
                # written once and read by the Gram pass
                moved = B * (4 * reads * C * h * w + 4 * 2 * 16 * h * w + 2 * 8 * (C + 1) * h * w + 4 * C * 16 * h * w)
            if name in cs.SCENE_METHODS:
                # pan is read by the adjoint pass and by the apply pass, ms by the Gram pass and by the apply pass; the fp64 plane q [h, w] is written once and
                # read by the Gram pass
                moved = B * (4 * 2 * C * h * w + 4 * 2 * 16 * h * w + 2 * 8 * h * w + 4 * C * 16 * h * w)
            if name.startswith(('atwt', 'awlp')):
                # ms and pan are read by the moments pass and by the apply pass, pan once more by the pass that sums (P_L - mu)^2 for match = lowpass
                moved = 4 * B * (2 * C * h * w + reads * 16 * h * w + C * 16 * h * w)
            if name in hr.RULES:
                # fs / hpm_r move what mtf_glp_cbd moves and read pan once more (the second moments pass takes the raw PAN).  hpm_h / bt_h: pan is read by the
                # low-pass and by the apply pass, ms by the Gram pass and by the apply pass; the fp64 plane D is written once and read by the Gram pass and, for
                # hpm_h, by the apply pass
                moved = B * (4 * reads * C * h * w + 4 * 4 * 16 * h * w + 8 * reads * h * w + 4 * C * 16 * h * w)
                if name in hr.HAZE_RULES:
                    moved = B * (4 * 2 * C * h * w + 4 * 2 * 16 * h * w + 8 * (3 if name == 'hpm_h' else 2) * h * w + 4 * C * 16 * h * w)
            ms_call = median_ms(lambda: fn(ms, pan), a.warmup, a.runs)
            row[name] = dict(bytes_moved=moved, ms_per_call=round(ms_call, 4), ms_per_image=round(ms_call / B, 4), gb_per_s=round(moved / ms_call / 1e6, 1),
                             hbm_fraction=round(moved / ms_call / 1e6 / a.hbm_gbs, 4))
            if not a.no_host:
                t = time.perf_counter()
                host(ms_np, pan_np)
                row[name]['numpy_ms_per_image'] = round((time.perf_counter() - t) * 1e3, 2)
        row['alternating'] = alternating_ms({'sfim': lambda: classical.sfim(ms, pan), 'mtf_glp_cbd': lambda: mtf_glp.mtf_glp(ms, pan, 'cbd'),
                                             'bdsd': lambda: bdsd.bdsd(ms, pan), 'bdsd_128': lambda: bdsd.bdsd(ms, pan, 128), 'gsa': lambda: classical.gsa(ms, pan),
                                             'gs': lambda: cs.gs(ms, pan), 'pca': lambda: cs.pca(ms, pan), 'awlp': lambda: atrous.awlp(ms, pan),
                                             'awlp_lowpass': lambda: atrous.awlp(ms, pan, 'lowpass'),
                                             **{r: (lambda r=r: mtf_hr.fuse(ms, pan, r)) for r in hr.RULES}}, a.warmup, a.runs)
        res[f'B{B}_C{C}_pan{4 * h}x{4 * w}'] = row
    print(json.dumps({'tool': 'time_classical', 'device': torch.cuda.get_device_name(0), 'runs': a.runs, 'warmup': a.warmup,
                      'hbm_gbs': a.hbm_gbs, 'unit': 'ms per call, synchronised, median', 'cases': res}))


if __name__ == '__main__':
    main()
