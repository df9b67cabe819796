"""One rank of the 2-process check of the train-step controls under data parallelism (tests/test_gpu_train_controls.py starts two
of these as fresh child processes, with RANK / WORLD_SIZE / MASTER_* in the environment; both share the box's one MI355X and talk
over gloo, like tests/ddp_engine_worker.py).

Each rank runs Pansharpening.attach_ddp() + Engine.train_step on ITS sample of every micro-batch (B = 1 per rank) with
accumulate = 2, clipping and the weight average, two windows.  Rank 0 then repeats the run in a single process on the whole
micro-batches (B = 2).  Everything observable goes to <outdir>/rank<r>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

C, K, H_MS, B_GLOBAL, WINDOWS = 4, 2, 8, 2, 2       # PAN 32 x 32
MAX_NORM = 0.01                                      # far below the gradient norm of this problem: every step is clipped


def run(net, micro, lo, hi):
    import lgteun_amd
    opt = lgteun_amd.FusedSGD(net.parameters(), lr=1.0, momentum=0.9)
    opt.dropout = False
    opt.set_controls(lgteun_amd.TrainControls(accumulate=len(micro), max_grad_norm=MAX_NORM, ema_decay=0.9))
    eng = net.engine()
    out = {'first': eng.flat.detach().cpu().numpy().copy()}
    calls = []
    if eng.buckets is not None:
        for bk in eng.buckets.values():
            inner = bk.all_reduce
            bk.all_reduce = lambda g, inner=inner: calls.append(1) or inner(g)
    for w in range(WINDOWS):
        for ms, pan, gt in micro:
            loss = eng.train_step(ms[lo:hi].contiguous(), pan[lo:hi].contiguous(), gt[lo:hi].contiguous(), opt)
        out[f'clip{w}'] = eng._clip.detach().cpu().numpy().copy()
    out['collectives'] = np.array(len(calls))
    out['loss'] = loss.detach().cpu().numpy().copy()[0]
    out['gflat'] = eng.gflat.detach().cpu().numpy().copy()
    out['weights'] = eng.flat.detach().cpu().numpy().copy()
    out['ema'] = opt._state['ema'].detach().cpu().numpy().copy()
    out['steps'] = np.array(opt._step)
    out['ranges'] = np.array(eng.live_ranges)
    return out


def main():
    outdir = sys.argv[1]
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    import torch.distributed as dist
    from gpu_helpers import make_module
    from lgteun_amd import ddp
    from oracle import detweights as dw

    torch.cuda.set_device(0)
    ddp.init_from_env('gloo')
    micro = [tuple(torch.from_numpy(a).cuda() for a in dw.make_inputs(B_GLOBAL, C, H_MS, H_MS, seed=s, kind='smooth')) for s in (11, 12)]
    a, b = ddp.shard_bounds(B_GLOBAL, rank, world)
    net = make_module(C, K, salt=rank)               # different weights per rank: attach_ddp broadcasts rank 0's
    net.attach_ddp()
    res = run(net, micro, a, b)
    res['world'] = np.array(net.engine().world)
    dist.barrier()
    if rank == 0:
        single = make_module(C, K, salt=0)
        single.engine().local_only = True            # a deliberate single-process run inside the initialised group
        res.update({'single_' + k: v for k, v in run(single, micro, 0, B_GLOBAL).items()})
    np.savez(os.path.join(outdir, f'rank{rank}.npz'), **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
