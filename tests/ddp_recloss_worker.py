"""One rank of the 2-process check of the l1 + SAM + SSIM train step under data parallelism (tests/test_gpu_recloss.py starts two of these
as fresh child processes, with RANK / WORLD_SIZE / MASTER_* in the environment; both share the box's one MI355X and talk over gloo, like
tests/ddp_qnr_worker.py).

Each rank runs Pansharpening.attach_ddp() + Engine.train_step(spectral_weight=, struct_weight=) on ITS sample (B = 1 per rank), one step.
Rank 0 then repeats the step in a single process on the whole batch (B = 2).  Everything observable goes to <outdir>/rank<r>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

C, K, H, B_GLOBAL, SEED = 4, 2, 32, 2, 11
W_SAM, W_SSIM = 0.3, 0.2


def run(net, batch, lo, hi):
    import lgteun_amd
    import torch.distributed as dist
    opt = lgteun_amd.FusedSGD(net.parameters(), lr=0.1, momentum=0.9)
    opt.dropout = False
    eng = net.engine()
    res = {'first': eng.flat.detach().cpu().numpy().copy()}
    buckets, collectives = [], []
    if eng.buckets is not None:
        for bk in eng.buckets.values():
            inner = bk.all_reduce
            bk.all_reduce = lambda g, inner=inner: buckets.append(1) or inner(g)
    real = dist.all_reduce

    def counted(t, *a, **k):
        if not buckets:                      # what the step issues ahead of the gradient bucket: nothing, both losses are additive
            collectives.append((t.numel(), t.element_size()))
        return real(t, *a, **k)
    dist.all_reduce = counted
    try:
        ms, pan, gt = (t[lo:hi].contiguous() for t in batch)
        eng.train_step(ms, pan, gt, opt, loss_weight=1.0, loss_type='l1', spectral_weight=W_SAM, struct_weight=W_SSIM)
        torch.cuda.synchronize()
    finally:
        dist.all_reduce = real
    res['collectives'] = np.array(collectives).reshape(-1, 2)
    res['bucket_calls'] = np.array(len(buckets))
    res['sam'] = eng._sam.detach().cpu().numpy().copy()[0]
    res['ssim'] = eng._ssim.detach().cpu().numpy().copy()[0]
    res['dout'] = eng._recloss_last['dout'].detach().cpu().numpy().copy()
    res['gflat'] = eng.gflat.detach().cpu().numpy().copy()
    res['weights'] = eng.flat.detach().cpu().numpy().copy()
    res['ranges'] = np.array(eng.live_ranges)
    return res


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch.distributed as dist
    from gpu_helpers import make_module
    from lgteun_amd import ddp
    from oracle import detweights as dw

    torch.cuda.set_device(0)
    ddp.init_from_env('gloo')
    batch = tuple(torch.from_numpy(t).cuda() for t in dw.make_inputs(B_GLOBAL, C, H // 4, H // 4, seed=SEED, kind='smooth'))
    a, b = ddp.shard_bounds(B_GLOBAL, rank, world)
    net = make_module(C, K, salt=rank)               # different weights per rank: attach_ddp broadcasts rank 0's
    net.attach_ddp()
    res = run(net, batch, a, b)
    res['world'] = np.array(net.engine().world)
    dist.barrier()
    if rank == 0:
        single = make_module(C, K, salt=0)
        single.engine().local_only = True            # a deliberate single-process run inside the initialised group
        res.update({'single_' + k: v for k, v in run(single, batch, 0, B_GLOBAL).items()})
    np.savez(os.path.join(outdir, f'rank{rank}.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
