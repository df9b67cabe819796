"""Cost of one training iteration per (loss, optimizer) configuration, fused route against the `fused=False` route, in one process:
`UnlgFormer.train_iter` at bench.py's configs[1] shape (C = 4, PAN 128^2, K = 4, 32 pairs), faithful mode, dropout on, the runner's
logging cadence (one host sync every 10 iterations on the fused route, two per iteration on the other).  The fused route is the four
library calls of Engine.train_step; the other one is the autograd bridge + nn.L1Loss / nn.MSELoss + the torch.optim class.
Both runners of a pair are warmed up, then their legs alternate; a leg is timed with device events around `--steps` iterations.
Prints one JSON line.   python tools/time_train_configs.py [--steps N] [--reps R]"""
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
    return dict(input_lr=dn(B, C, H // 4, H // 4), input_pan=dn(B, 1, H, H), target=dn(B, C, H, H), image_id=['x'] * B)


class Leg:
    def __init__(self, loss, entry, fused, work_dir):
        cfg = Config(dict(ms_chans=C, work_dir=work_dir, datas='GF-2', cuda=True, max_iter=10 ** 9, bit_depth=11,
                          loss_cfg={'rec_loss': dict(type=loss, w=1.)}, optim_cfg={'core_module': dict(entry, fused=fused)},
                          sched_cfg=dict(step_size=25900, gamma=0.85), model_cfg={'core_module': dict(stage=K)}))
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
    a = ap.parse_args()
    if a.steps < 100:
        ap.error('--steps must be at least 100')
    warnings.filterwarnings('ignore', message='Detected call of')
    if a.work_dir is None:
        a.work_dir = tempfile.mkdtemp(prefix='lgteun_time_')
    batch = synth_batch(torch.device('cuda', 0))
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


if __name__ == '__main__':
    main()
