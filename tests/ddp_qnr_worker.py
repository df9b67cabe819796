"""One rank of the 2-process check of the no-reference (QNR) train step under data parallelism (tests/test_gpu_qnr_loss.py starts two of
these as fresh child processes, with RANK / WORLD_SIZE / MASTER_* in the environment; both share the box's one MI355X and talk over
gloo, like tests/ddp_train_controls_worker.py).

Each rank runs Pansharpening.attach_ddp() + Engine.train_step(gt=None, noref_weight=1) on ITS sample (B = 1 per rank), one step.  Rank 0
then repeats the step in a single process on the whole batch (B = 2).  Everything observable goes to <outdir>/rank<r>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

C, K, H, B_GLOBAL, SEED = 4, 2, 32, 2, 21


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
        if not buckets:                      # what the step issues ahead of the gradient bucket
            collectives.append((t.numel(), t.element_size()))
        return real(t, *a, **k)
    dist.all_reduce = counted
    try:
        out, pan, ms, pan_l = (t[lo:hi].contiguous() for t in batch)
        loss = eng.train_step(ms, pan, None, opt, pan_l=pan_l, noref_weight=1.0)
        torch.cuda.synchronize()
    finally:
        dist.all_reduce = real
    res['collectives'] = np.array(collectives).reshape(-1, 2)
    res['bucket_calls'] = np.array(len(buckets))
    res['loss'] = loss.detach().cpu().numpy().copy()[0]
    for k in ('table', 'indices', 'dout'):
        res[k] = eng._qnr_last[k].detach().cpu().numpy().copy()
    res['gflat'] = eng.gflat.detach().cpu().numpy().copy()
    res['weights'] = eng.flat.detach().cpu().numpy().copy()
    res['ranges'] = np.array(eng.live_ranges)
    return res


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch.distributed as dist
    import qnr_helpers as qh
    from gpu_helpers import make_module
    from lgteun_amd import ddp

    torch.cuda.set_device(0)
    ddp.init_from_env('gloo')
    batch = tuple(t.cuda() for t in qh.make_inputs(B_GLOBAL, C, H, H, SEED))
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
