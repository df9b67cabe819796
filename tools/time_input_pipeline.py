"""What feeding the train step from FILES costs: the host path (`DataLoader(PSDataset)`: three TIFF decodes and two scipy pyramids per item)
against the device-resident path (lgteun_amd/resident.py: the set decoded once, one gather kernel per batch).  Both modes write the same
N synthetic triplets (C = 4, PAN 128 x 128, 11-bit uint16, dataset.write_tiff) into a temporary directory first.

  --host   never loads the HIP library or touches a device.  Pairs per second of DataLoader(PSDataset) at num_workers 0, 4, 8 and 14
           (persistent workers; epochs are repeated until the workers' start-up is under 5 % of the leg), and the seconds
           resident.pack_host takes to decode the set for the store with 1 and with 16 threads.
  (default) on the GPU: `UnlgFormer.train_iter` at bench.py's configs[1] shape (C = 4, PAN 128^2, K = 4, 32 pairs, faithful, l1 + Adam) fed
           (c) one fixed device batch -- the ceiling, (b) the resident loader with fold_normalize=True, shuffled, (a) build_loader(...,
           device=...) with num_workers=0 -- the host path.  Legs of --steps iterations alternate c, b, a; median and max - min of --reps
           legs each, like tools/time_train_configs.py.  (b) and (a) run through Base_model._train_batches, as the runner's train() does.
           The assemble kernel's own duration comes from the library's event timers (lg_prof_*) in a pass of its own.
Prints one JSON line.   python tools/time_input_pipeline.py [--host] [--n N] [--steps S] [--reps R]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import warnings

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402

C, K, H, B, BITS = 4, 4, 128, 32, 11
WORKERS = (0, 4, 8, 14)


def write_set(root, n):
    from lgteun_amd.dataset import write_tiff
    rng = np.random.default_rng(19971118)

    def dn(*shape):
        return rng.integers(0, 2 ** BITS, size=shape, dtype=np.int64).astype(np.uint16)
    for i in range(n):
        write_tiff(os.path.join(root, f'im{i:05d}_pan.tif'), dn(H, H))
        write_tiff(os.path.join(root, f'im{i:05d}_lr.tif'), dn(H // 4, H // 4, C))
        write_tiff(os.path.join(root, f'im{i:05d}_mul.tif'), dn(H, H, C))
    return root


def set_cfg(root, **extra):
    return dict(dataset=dict(type='PSDataset', image_dirs=[root], bit_depth=BITS), batch_size=B, shuffle=True, **extra)


def host_mode(a, root):
    import torch.utils.data as data

    from lgteun_amd.dataset import PSDataset
    from lgteun_amd.resident import pack_host
    ds = PSDataset([root], BITS)
    rows = {}
    for nw in WORKERS:
        loader = data.DataLoader(ds, batch_size=B, shuffle=True, num_workers=nw, persistent_workers=nw > 0)
        t0 = time.perf_counter()
        it = iter(loader)
        first = next(it)
        start_up = time.perf_counter() - t0              # the workers' start and the first batch
        items = len(first['image_id']) + sum(len(b['image_id']) for b in it)
        epochs = 1
        while time.perf_counter() - t0 < 25.0 * start_up or epochs < 2:
            items += sum(len(b['image_id']) for b in loader)
            epochs += 1
        total = time.perf_counter() - t0
        rows[f'workers_{nw}'] = dict(pairs_per_s=round(items / total, 1), epochs=epochs, start_up_share=round(start_up / total, 4))
        del it, loader
    decode = {}
    for threads in (1, 16):
        t0 = time.perf_counter()
        pack = pack_host(ds, threads=threads)
        decode[f'threads_{threads}_s'] = round(time.perf_counter() - t0, 3)
    return dict(mode='host', items=len(ds), cpus=len(os.sched_getaffinity(0)), dataloader=rows, store_decode=decode, store_bytes=pack.nbytes)


def gpu_mode(a, root):
    import torch

    import lgteun_amd
    from lgteun_amd import _lib
    from lgteun_amd.compat import Config
    from lgteun_amd.dataset import build_loader
    dev = torch.device('cuda', 0)
    work = tempfile.mkdtemp(prefix='lgteun_pipe_')

    t0 = time.perf_counter()
    resident = build_loader(set_cfg(root), device=dev, resident=True, fold_normalize=True)[0]
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    host = build_loader(set_cfg(root, num_workers=0), device=dev)[0]
    fixed = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in next(iter(resident)).items()}
    resident.set_epoch(0)

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

        def timed_ms(self, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            self.run(n)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n

    legs = {'c_fixed_batch': Leg(None), 'b_resident': Leg(resident), 'a_host_loader': Leg(host)}
    for leg in legs.values():
        leg.run(a.warmup)
    ms = {k: [] for k in legs}
    wall = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, leg in legs.items():
            d, w = leg.timed_ms(a.steps)
            ms[k].append(d)
            wall[k].append(w)
    row = {}
    for k in legs:
        row[k] = dict(ms=round(statistics.median(ms[k]), 4), spread_ms=round(max(ms[k]) - min(ms[k]), 4), legs_ms=[round(x, 4) for x in ms[k]],
                      wall_ms=round(statistics.median(wall[k]), 4))
    # the assemble kernel alone: the library's event pair around each launch, batches drawn without a train step in between
    L = _lib.lib()
    n_prof = 64
    _lib.check(L.lg_prof_enable(_lib.KERNEL_IDS['batch'], n_prof), 'lg_prof_enable')
    it, got = iter(resident), 0
    while got < n_prof:
        b = next(it, None)
        if b is None:
            it = iter(resident)
            continue
        got += 1
    torch.cuda.synchronize()
    import ctypes
    tot, n_l = ctypes.c_double(0.0), ctypes.c_int64(0)
    _lib.check(L.lg_prof_read(ctypes.byref(tot), ctypes.byref(n_l)), 'lg_prof_read')
    L.lg_prof_disable()
    asm_ms = tot.value / max(1, n_l.value)
    c, b_, a_ = row['c_fixed_batch'], row['b_resident'], row['a_host_loader']
    return dict(mode='gpu', device=torch.cuda.get_device_name(0), items=len(resident.store), store_bytes=resident.store.nbytes,
                store_build_s=round(build_s, 3), steps_per_leg=a.steps, legs_per_route=a.reps, legs=row,
                assemble_kernel_ms=round(asm_ms, 5), assemble_launches_timed=int(n_l.value),
                b_minus_c_ms=round(b_['ms'] - c['ms'], 4), margin_ms=round(asm_ms + c['spread_ms'], 4),
                pairs_per_s=dict(fixed=round(B * 1e3 / c['wall_ms'], 1), resident=round(B * 1e3 / b_['wall_ms'], 1), host=round(B * 1e3 / a_['wall_ms'], 1)),
                resident_over_host=round(a_['wall_ms'] / b_['wall_ms'], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host', action='store_true', help='the host-only measurements (no library, no device)')
    ap.add_argument('--n', type=int, default=256, help='synthetic triplets (at least one batch of 32)')
    ap.add_argument('--steps', type=int, default=100, help='iterations per timed leg (at least 100)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=15)
    a = ap.parse_args()
    if a.n < B:
        ap.error(f'--n must be at least {B}')
    if a.steps < 100:
        ap.error('--steps must be at least 100')
    warnings.filterwarnings('ignore', message='Detected call of')
    with tempfile.TemporaryDirectory(prefix='lgteun_pipe_set_') as root:
        write_set(root, a.n)
        out = host_mode(a, root) if a.host else gpu_mode(a, root)
    out.update(tool='time_input_pipeline', workload=f'C={C}, PAN {H}x{H}, {BITS}-bit uint16, batches of {B}' +
               ('' if a.host else f'; K={K}, faithful mode, l1 + Adam, dropout on'))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
