"""Cost of one training iteration per (loss, optimizer) configuration, fused route against the `fused=False` route, in one process:
`UnlgFormer.train_iter` at bench.py's configs[1] shape (C = 4, PAN 128^2, K = 4, 32 pairs), faithful mode, dropout on, the runner's
logging cadence (one host sync every 10 iterations on the fused route, two per iteration on the other).  The fused route is the four
library calls of Engine.train_step; the other one is the autograd bridge + nn.L1Loss / nn.MSELoss + the torch.optim class.
Both runners of a pair are warmed up, then their legs alternate; a leg is timed with device events around `--steps` iterations.
Prints one JSON line.   python tools/time_train_configs.py [--steps N] [--reps R]

With `--train-cfg JSON` (may be repeated) the tool times the train-step controls instead: the fused route of ONE configuration (`--config`,
default l1+Adam) without `train_cfg` against the same route with each given `cfg.train_cfg`, legs alternating in the same process, e.g.
    python tools/time_train_configs.py --train-cfg '{"max_grad_norm": 1.0}' --train-cfg '{"ema_decay": 0.999}' --train-cfg '{"accumulate": 2}'
The unit stays ms per train_iter call: with accumulate = A that is the cost per micro-batch, averaged over the window.

With `--noref` the tool times the no-reference loss (`loss_cfg['noref_loss']`, type 'qnr') with `--config`'s optimizer: the fused `l1` step
against `qnr` alone and `l1 + 0.1 qnr`, each on the fused route (lg_qnr_stats + lg_qnr_grad inside Engine.train_step) and on the `fused=False`
route (losses.QNRLoss through autograd: the reference's C^2 + C torch reductions), legs alternating in the same process.

With `--recloss` the tool times the spectral and the structural loss (`loss_cfg['spectral_loss']`, type 'sam'; `loss_cfg['struct_loss']`,
type 'ssim') the same way: the fused `l1` step against `l1 + 0.1 sam`, `l1 + 0.1 ssim` and `l1 + 0.1 sam + 0.1 ssim`, each on the fused
route (lg_sam_loss / lg_ssim_loss inside Engine.train_step) and on the `fused=False` route (losses.SAMLoss / SSIMLoss through autograd)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import warnings

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402

import lgteun_amd  # noqa: E402
from lgteun_amd.compat import Config  # noqa: E402

C, K, H, B = 4, 4, 128, 32
OPTIMS = {'Adam': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3), 'AdamW': dict(type='AdamW', lr=1.5e-3, weight_decay=1e-2),
          'SGD': dict(type='SGD', lr=1e-2, momentum=0.9), 'RMSprop': dict(type='RMSprop', lr=1.5e-3)}


def synth_batch(device):
    """integer DN in [0, 2047] / 2047.5, like bench.py's batch"""
    g = torch.Generator().manual_seed(19971118)

    def dn(*shape):
        return (torch.randint(0, 2048, shape, generator=g).float() / 2047.5).to(device)
    return dict(input_lr=dn(B, C, H // 4, H // 4), input_pan=dn(B, 1, H, H), target=dn(B, C, H, H), image_id=['x'] * B,
                input_pan_l=dn(B, 1, H // 4, H // 4))


class Leg:
    def __init__(self, loss, entry, fused, work_dir, train_cfg=None):
        """loss: 'l1' / 'l2' (one rec_loss entry of weight 1), or a whole loss_cfg"""
        extra = {} if train_cfg is None else dict(train_cfg=dict(train_cfg))
        loss_cfg = loss if isinstance(loss, dict) else {'rec_loss': dict(type=loss, w=1.)}
        cfg = Config(dict(ms_chans=C, work_dir=work_dir, datas='GF-2', cuda=True, max_iter=10 ** 9, bit_depth=11,
                          loss_cfg=loss_cfg, optim_cfg={'core_module': dict(entry, fused=fused)},
                          sched_cfg=dict(step_size=25900, gamma=0.85), model_cfg={'core_module': dict(stage=K)}, **extra))
        torch.manual_seed(19971118)
        self.runner = lgteun_amd.build_model('UnlgFormer', cfg, None, None, None, None)
        self.runner.set_cuda()
        self.runner.module_dict['core_module'].train()
        self.runner.set_optim()
        self.runner.set_sched()
        assert bool(getattr(self.runner.optim_dict['core_module'], 'is_fused_lgteun', False)) == fused
        self.it = 0

    def run(self, batch, n):
        for _ in range(n):
            self.it += 1
            self.runner.train_iter(self.it, batch)
            self.runner.sched_dict['core_module'].step()

    def timed_ms(self, batch, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        self.run(batch, n)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100, help='iterations per timed leg (at least 100)')
    ap.add_argument('--reps', type=int, default=3, help='timed legs per route; the two routes alternate')
    ap.add_argument('--warmup', type=int, default=15)
    ap.add_argument('--work-dir', default=None, help='where the runners create their output tree (default: a temporary directory)')
    ap.add_argument('--train-cfg', action='append', default=None, metavar='JSON',
                    help='a cfg.train_cfg as a JSON object, e.g. \'{"max_grad_norm": 1.0}\'; may be repeated.  Times the fused route of --config '
                         'without train_cfg against the fused route with each of them')
    ap.add_argument('--config', default='l1+Adam', help='LOSS+OPTIMIZER of the --train-cfg comparison (default l1+Adam); --noref takes its optimizer')
    ap.add_argument('--noref', action='store_true', help='time the no-reference loss: l1 / qnr / l1+qnr, fused and fused=False routes')
    ap.add_argument('--recloss', action='store_true', help='time the SAM and SSIM losses: l1 / l1+sam / l1+ssim / l1+sam+ssim, both routes')
    a = ap.parse_args()
    if a.steps < 100:
        ap.error('--steps must be at least 100')
    if a.train_cfg is not None:
        try:
            a.train_cfg = [json.loads(t) for t in a.train_cfg]
        except ValueError as e:
            ap.error(f'--train-cfg takes a JSON object: {e}')
        loss, _, name = a.config.partition('+')
        if loss not in ('l1', 'l2') or name not in OPTIMS or not all(isinstance(t, dict) for t in a.train_cfg):
            ap.error(f"--config is l1+ or l2+ one of {list(OPTIMS)}; every --train-cfg a JSON object")
    warnings.filterwarnings('ignore', message='Detected call of')
    if a.work_dir is None:
        a.work_dir = tempfile.mkdtemp(prefix='lgteun_time_')
    batch = synth_batch(torch.device('cuda', 0))
    if a.noref:
        return time_noref(a, batch)
    if a.recloss:
        return time_recloss(a, batch)
    if a.train_cfg is not None:
        return time_controls(a, batch)
    rows = {}
    for loss in ('l1', 'l2'):
        for name, entry in OPTIMS.items():
            legs = {'fused': Leg(loss, entry, True, a.work_dir), 'torch': Leg(loss, entry, False, a.work_dir)}
            for leg in legs.values():
                leg.run(batch, a.warmup)
            ms = {k: [] for k in legs}
            for _ in range(a.reps):
                for k, leg in legs.items():
                    ms[k].append(leg.timed_ms(batch, a.steps))
            row = {}
            for k, v in ms.items():
                row[k + '_ms'] = round(statistics.median(v), 4)
                row[k + '_spread_ms'] = round(max(v) - min(v), 4)
            row['torch_over_fused'] = round(row['torch_ms'] / row['fused_ms'], 4)
            rows[f'{loss}+{name}'] = row
            del legs
            torch.cuda.empty_cache()
    print(json.dumps({'tool': 'time_train_configs', 'unit': 'ms per train_iter (median of the legs; spread = max - min of the legs)',
                      'workload': f'C={C}, PAN {H}x{H}, K={K}, {B} pairs, faithful mode, dropout on', 'steps_per_leg': a.steps,
                      'legs_per_route': a.reps, 'device': torch.cuda.get_device_name(0), 'cases': rows}))


def time_controls(a, batch):
    """the fused route of one configuration: no train_cfg (every launch what it was before the controls existed) against each train_cfg"""
    loss, _, name = a.config.partition('+')
    legs = {'off': Leg(loss, OPTIMS[name], True, a.work_dir)}
    for t in a.train_cfg:
        legs[json.dumps(t, sort_keys=True)] = Leg(loss, OPTIMS[name], True, a.work_dir, train_cfg=t)
    for leg in legs.values():
        leg.run(batch, a.warmup)
    ms = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, leg in legs.items():
            ms[k].append(leg.timed_ms(batch, a.steps))
    rows = {}
    for k, v in ms.items():
        rows[k] = dict(ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4))
    for k, row in rows.items():
        row['over_off'] = round(row['ms'] / rows['off']['ms'], 4)
    print(json.dumps({'tool': 'time_train_configs', 'unit': 'ms per train_iter call (median of the legs; spread = max - min of the legs)',
                      'workload': f'{a.config}, fused route, C={C}, PAN {H}x{H}, K={K}, {B} pairs, faithful mode, dropout on',
                      'steps_per_leg': a.steps, 'legs_per_case': a.reps, 'device': torch.cuda.get_device_name(0), 'train_cfg': rows}))


def time_noref(a, batch):
    """l1 (the untouched path), qnr and l1 + 0.1 qnr on both routes; every leg alternates with every other"""
    name = a.config.partition('+')[2]
    if name not in OPTIMS:
        raise SystemExit(f'--config names one of {list(OPTIMS)} behind the +')
    l1, qnr = dict(type='l1', w=1.), dict(type='qnr', w=1.)
    cases = {'l1': {'rec_loss': l1}, 'qnr': {'noref_loss': qnr}, 'l1+qnr': {'rec_loss': l1, 'noref_loss': dict(qnr, w=0.1)}}
    time_loss_cases(a, batch, name, cases, 'noref')


def time_recloss(a, batch):
    """l1 (the untouched path), l1 + 0.1 sam, l1 + 0.1 ssim and all three on both routes; every leg alternates with every other"""
    name = a.config.partition('+')[2]
    if name not in OPTIMS:
        raise SystemExit(f'--config names one of {list(OPTIMS)} behind the +')
    l1, sam, ssim = dict(type='l1', w=1.), dict(type='sam', w=0.1), dict(type='ssim', w=0.1, data_range=1.0)
    cases = {'l1': {'rec_loss': l1}, 'l1+sam': {'rec_loss': l1, 'spectral_loss': sam}, 'l1+ssim': {'rec_loss': l1, 'struct_loss': ssim},
             'l1+sam+ssim': {'rec_loss': l1, 'spectral_loss': sam, 'struct_loss': ssim}}
    time_loss_cases(a, batch, name, cases, 'recloss')


def time_loss_cases(a, batch, name, cases, key):
    legs = {f'{route} {c}': Leg(cfg, OPTIMS[name], route == 'fused', a.work_dir) for c, cfg in cases.items() for route in ('fused', 'torch')}
    for leg in legs.values():
        leg.run(batch, a.warmup)
    ms = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, leg in legs.items():
            ms[k].append(leg.timed_ms(batch, a.steps))
    rows = {k: dict(ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4)) for k, v in ms.items()}
    print(json.dumps({'tool': 'time_train_configs', 'unit': 'ms per train_iter (median of the legs; spread = max - min of the legs)',
                      'workload': f'{name}, C={C}, PAN {H}x{H}, K={K}, {B} pairs, faithful mode, dropout on', 'steps_per_leg': a.steps,
                      'legs_per_case': a.reps, 'device': torch.cuda.get_device_name(0), key: rows}))


if __name__ == '__main__':
    main()
