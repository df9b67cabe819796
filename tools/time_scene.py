"""What a tiled scene costs on the GPU (lgteun_amd/scene.py): per scene size
  * ms per scene of fuse_scene (uint16 samples already on the device, C = 4, K = 4, tile 128, overlap 32, the default batch), synchronised;
  * the same number of tile batches through the forward alone, at the same tile and batch;
  * the share of the gather and blend launches, from the library's event timers (lg_prof_*, one kernel id per run).
Every size is warmed up before it is timed.  Prints one JSON line.   python tools/time_scene.py [--sizes 4096x4096 1040x272] [--reps N]"""
import argparse
import ctypes
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
from lgteun_amd import _lib  # noqa: E402
from lgteun_amd import scene as sc  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def kernel_ms(L, name, launches, fn):
    """event-timed total of one kernel id over one call of fn"""
    _lib.check(L.lg_prof_enable(_lib.KERNEL_IDS[name], launches + 8), 'lg_prof_enable')
    fn()
    tot, n = ctypes.c_double(), ctypes.c_int64()
    _lib.check(L.lg_prof_read(ctypes.byref(tot), ctypes.byref(n)), 'lg_prof_read')
    L.lg_prof_disable()
    return tot.value, int(n.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', nargs='+', default=['4096x4096', '1040x272'], help='PAN sizes HxW')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--tile', type=int, default=128)
    ap.add_argument('--overlap', type=int, default=32)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('-C', type=int, default=4)
    ap.add_argument('-K', type=int, default=4)
    a = ap.parse_args()
    net = make_module(a.C, a.K)
    eng, L = net.engine(), _lib.lib()
    rng = np.random.default_rng(0)
    res = {}
    for size in a.sizes:
        H, W = (int(v) for v in size.split('x'))
        ms = torch.from_numpy(rng.integers(0, 2048, (a.C, H // 4, W // 4)).astype(np.uint16).view(np.int16)).cuda()
        pan = torch.from_numpy(rng.integers(0, 2048, (1, H, W)).astype(np.uint16).view(np.int16)).cuda()
        plan = sc.ScenePlan(net, a.C, H, W, a.tile, a.overlap, a.batch)
        fuse = lambda: sc.fuse_scene(net, ms, pan, tile=a.tile, overlap=a.overlap, bit_depth=11, _plan=plan)      # noqa: E731
        cuts = [min(plan.batch, plan.n_tiles - f) for f in range(0, plan.n_tiles, plan.batch)]
        flags, P = plan.flags(net), (lambda t: ctypes.c_void_p(t.data_ptr()))

        def forward_only():
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for B in cuts:
                _lib.check(L.lgteun_forward(plan.plan, P(eng.flat), P(plan.t_ms), P(plan.t_pan), P(plan.t_out), P(plan.ws), plan.ws.numel(), B,
                                            flags, 0, stream), 'lgteun_forward')
        scene_ms = timed(fuse, a.reps)
        fwd_ms = timed(forward_only, a.reps)
        g_ms, g_n = kernel_ms(L, 'scene_gather', len(cuts), fuse)
        b_ms, b_n = kernel_ms(L, 'scene_blend', len(cuts), fuse)
        res[size] = dict(tiles=plan.n_tiles, batch=plan.batch, launches=len(cuts), scene_ms=round(scene_ms, 3), forward_only_ms=round(fwd_ms, 3),
                         megapixels_per_s=round(H * W / scene_ms / 1e3, 1), gather_ms=round(g_ms, 4), blend_ms=round(b_ms, 4),
                         gather_blend_share=round((g_ms + b_ms) / scene_ms, 4), timed_launches=[g_n, b_n])
    print(json.dumps({'tool': 'time_scene', 'device': torch.cuda.get_device_name(0), 'C': a.C, 'K': a.K, 'tile': a.tile, 'overlap': a.overlap,
                      'unit': 'ms per scene, synchronised', 'cases': res}))


if __name__ == '__main__':
    main()
