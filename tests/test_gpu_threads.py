"""-m gpu: the library under four host threads at once -- "forward / backward calls on different streams or threads do not interact"
(include/lgteun_hip.h), "Safe from several host threads" (csrc/common.h).  ctypes releases the GIL inside the library, so the four threads are
inside it together: the thread_local staging of the reduce queue, the mutex-guarded reduce-image cache, the lg_l2-style process-wide counters, the
per-device once-bits and the thread-local message of lg_last_error all see concurrent callers here for the first time.

Each thread has its own stream, module, plan, parameters, data and workspaces, is released through a barrier, and runs two train steps through the
C ABI (forward, l1 loss, backward, AdamW), one lg_gsa, one lg_iqa_ref and one call that a validator rejects.  Every result must be bitwise that
thread's work done alone, and the message it reads must be its own.  Three rounds; no loop until failure.
Measured on an MI355X: 0.4 s for the test; every round of every thread bitwise its work alone, every message its own thread's."""
import threading

import pytest
import torch

import stream_helpers as sh
from lgteun_amd import _lib
from stream_helpers import L
from test_abi_limits_cpu import ENTRIES
from test_thread_state_cpu import PER_THREAD, _reject

pytestmark = pytest.mark.gpu

N_THREADS, ROUNDS, STEPS = 4, 3, 2
C, CH, CW, B = 4, 5, 7, 2


class Worker:
    """everything one thread owns"""

    def __init__(self, i, stream):
        self.i, self.s = i, stream
        self.rig = sh.TrainRig(salt=i, seed=60 + i, steps=STEPS)
        self.ms, self.pan = sh.classical_scene(B, C, CH, CW, seed=70 + i)
        self.fused = torch.empty(B, C, 4 * CH, 4 * CW, device='cuda')
        self.stats = torch.empty(B, 2 * C + 1, dtype=torch.float64, device='cuda')
        self.gsa_ws = torch.empty(int(L().lg_classical_workspace_bytes(B, C, CH, CW, _lib.LG_CLASSICAL_GSA)) // 8 + 1, dtype=torch.float64, device='cuda')
        self.truth = sh.uniform((B, C, 4 * CH, 4 * CW), 80 + i).cuda()
        self.rows = torch.empty(B, 5, dtype=torch.float64, device='cuda')
        self.iqa_ws = torch.empty(int(L().lg_iqa_workspace_bytes(B, C, 4 * CH, 4 * CW, 0)) // 8 + 1, dtype=torch.float64, device='cuda')
        self.reject = PER_THREAD[i]

    def reset(self):
        self.rig.reset()
        for t in (self.fused, self.stats, self.gsa_ws, self.rows, self.iqa_ws):
            sh.fill(t)

    def work(self):
        """enqueue everything on the thread's stream, make the rejected call, wait for the stream -> (results, rc, message)"""
        for step in range(STEPS):
            for f in self.rig.calls(step):
                f(self.s)
        sh.gsa_call(self.ms, self.pan, self.fused, self.stats, self.gsa_ws, self.s)
        sh.iqa_ref_call(self.fused, self.truth, self.rows, self.iqa_ws, self.s)
        entry, bad, _ = self.reject
        rc = _reject(entry, bad)
        msg = L().lg_last_error().decode()
        self.s.synchronize()
        res = self.rig.results()
        res.update(gsa=sh.bits(self.fused), gsa_stats=sh.bits(self.stats), iqa=sh.bits(self.rows))
        return res, rc, msg


def test_four_threads_each_on_its_own_stream():
    workers = [Worker(i, s) for i, s in enumerate(sh.side_streams(N_THREADS))]
    alone = []
    for w in workers:                       # each thread's work done alone, from the main thread; it also warms every entry and the reduce-image cache
        w.reset()
        torch.cuda.synchronize()
        res, rc, msg = w.work()
        w.reset()
        torch.cuda.synchronize()
        again, _, _ = w.work()
        assert not sh.differing(res, again), (w.i, 'the work alone does not repeat its bits', sh.differing(res, again))
        entry, _, says = w.reject
        assert rc < 0 and msg.startswith(ENTRIES[entry][0] + ':') and says in msg, (w.i, rc, msg)
        assert bool(torch.isfinite(w.rig.losses).all()) and bool(torch.isfinite(w.rows).all())
        alone.append(res)
    assert all(sh.differing(alone[0], alone[k]) for k in range(1, N_THREADS)), 'the threads do the same work'

    for rnd in range(ROUNDS):
        for w in workers:
            w.reset()
        torch.cuda.synchronize()
        barrier = threading.Barrier(N_THREADS)
        got, errors = [None] * N_THREADS, [None] * N_THREADS

        def body(i):
            try:
                barrier.wait(60)
                got[i] = workers[i].work()
            except BaseException as e:      # noqa: BLE001 - reported below, from the main thread
                errors[i] = e
        threads = [threading.Thread(target=body, args=(i,)) for i in range(N_THREADS)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
            assert not t.is_alive(), 'a thread did not come back'
        torch.cuda.synchronize()
        for i, e in enumerate(errors):
            if e is not None:
                raise AssertionError(f'round {rnd}, thread {i}: {e!r}') from e
        for i, (res, rc, msg) in enumerate(got):
            entry, _, says = workers[i].reject
            assert rc < 0, (rnd, i, rc)
            assert msg.startswith(ENTRIES[entry][0] + ':') and says in msg, (rnd, i, "read another thread's message", msg)
            assert not sh.differing(alone[i], res), (rnd, i, 'differs from the work done alone', sh.differing(alone[i], res))
