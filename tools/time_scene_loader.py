"""What feeding the train step from ONE SCENE costs (lgteun_amd/wald.py) against the device-resident loader over the same windows
(lgteun_amd/resident.py), at bench.py's configs[1] shape: C = 4, patch 128, 32 pairs per batch, uint16, K = 4, faithful, l1 + Adam.

A synthetic 11-bit scene (PAN grid --side x --side, default 1024: 29 x 29 = 841 windows at step 32) is put on the device once; the same
windows, cut on the host, make the ResidentStore.  Both loaders run shuffled with fold_normalize=True.  Measured, with legs of the two
routes ALTERNATING on this one box (median and max - min of --reps legs each):
  * ms per batch of each loader alone (stream events around --steps batches, no train step in between);
  * ms per `UnlgFormer.train_iter` fed by each loader through Base_model._train_batches, and by one fixed device batch (the ceiling).
Prints one JSON line.   python tools/time_scene_loader.py [--side N] [--step S] [--steps S] [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import warnings

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402

C, K, P, B, BITS = 4, 4, 128, 32, 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=1024, help='PAN-grid side of the synthetic scene (a multiple of 4)')
    ap.add_argument('--step', type=int, default=32, help='window step (the reference cuts at 8 .. 52)')
    ap.add_argument('--steps', type=int, default=100, help='batches / iterations per timed leg')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=15)
    a = ap.parse_args()
    warnings.filterwarnings('ignore', message='Detected call of')
    import torch

    import lgteun_amd
    from lgteun_amd import wald
    from lgteun_amd.compat import Config
    from lgteun_amd.resident import HostPack, ResidentLoader, ResidentStore
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(19971118)
    dn = lambda *shape: rng.integers(0, 2 ** BITS, size=shape, dtype=np.int64).astype(np.uint16)      # noqa: E731
    scene = wald.SceneStore(dn(1, a.side, a.side), dn(C, a.side // 4, a.side // 4), dn(C, a.side, a.side), dev)
    org = wald.window_origins(a.side, a.side, P, a.step)
    pan, lr, mul = scene.windows(org, P)
    items = ResidentStore(HostPack(pan, lr, mul, [wald.window_id(y, x) for y, x in org]), dev)
    kw = dict(shuffle=True, fold_normalize=True, bit_depth=BITS)
    loaders = {'scene': wald.SceneLoader(scene, P, B, origins=org, **kw), 'resident': ResidentLoader(items, B, **kw)}
    work = tempfile.mkdtemp(prefix='lgteun_scene_loader_')

    def endless(loader):
        while True:
            yield from loader

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    # the loaders alone
    feeds = {k: endless(ld) for k, ld in loaders.items()}

    def drawer(it):
        def draw_n(n):
            for _ in range(n):
                next(it)
        return draw_n
    draw = {k: drawer(it) for k, it in feeds.items()}
    for fn in draw.values():
        fn(a.warmup)
    batch_ms = {k: [] for k in draw}
    for _ in range(a.reps):
        for k, fn in draw.items():
            batch_ms[k].append(timed(fn, a.steps))
    fixed = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in next(feeds['resident']).items()}

    class Leg:
        def __init__(self, loader):
            cfg = Config(dict(ms_chans=C, work_dir=work, datas='GF-2', cuda=True, max_iter=10 ** 9, bit_depth=BITS,
                              loss_cfg={'rec_loss': dict(type='l1', w=1.)}, optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                              sched_cfg=dict(step_size=25900, gamma=0.85), model_cfg={'core_module': dict(stage=K)}))
            torch.manual_seed(19971118)
            self.runner = lgteun_amd.build_model('UnlgFormer', cfg, None, loader, None, None)
            self.runner.set_cuda()
            self.runner.module_dict['core_module'].train()
            self.runner.set_optim()
            self.runner.set_sched()
            self.batches = self.runner._train_batches(dev) if loader is not None else None
            self.it = 0

        def run(self, n):
            for _ in range(n):
                if self.batches is None:
                    self.it, batch = self.it + 1, fixed
                else:
                    self.it, batch = next(self.batches)
                self.runner.train_iter(self.it, batch)
                self.runner.sched_dict['core_module'].step()

    legs = {'fixed_batch': Leg(None), 'scene': Leg(loaders['scene']), 'resident': Leg(loaders['resident'])}
    for leg in legs.values():
        leg.run(a.warmup)
    iter_ms = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, leg in legs.items():
            iter_ms[k].append(timed(leg.run, a.steps))

    def row(v):
        return dict(ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4), legs_ms=[round(x, 4) for x in v])
    out = dict(tool='time_scene_loader', device=torch.cuda.get_device_name(0),
               workload=f'C={C}, patch {P}, {BITS}-bit uint16, batches of {B}; scene {a.side} x {a.side}, step {a.step}: {len(org)} windows; '
                        f'K={K}, faithful mode, l1 + Adam, dropout on',
               scene_bytes=scene.nbytes, resident_bytes=items.nbytes, steps_per_leg=a.steps, legs_per_route=a.reps,
               ms_per_batch={k: row(v) for k, v in batch_ms.items()}, ms_per_train_iter={k: row(v) for k, v in iter_ms.items()})
    r, s = out['ms_per_train_iter']['resident']['ms'], out['ms_per_train_iter']['scene']['ms']
    out['scene_over_resident_train_iter'] = round(s / r, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
