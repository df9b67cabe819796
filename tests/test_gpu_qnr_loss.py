"""-m gpu: the fused no-reference loss 1 - QNR -- `lg_qnr_stats` / `lg_qnr_grad` per op against the fp64 restatement of
tests/qnr_helpers.py, `Engine.train_step(noref_weight=...)` against hand sequences of library calls, `loss_cfg['noref_loss']` through the
runner, and two data-parallel ranks against one process.  Every comparison first asserts the entry condition (qnr_helpers.reference):
every |d| of the inputs is at least 1e-3, so no sign is in doubt."""
import ctypes
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import qnr_helpers as qh
from train_controls_helpers import engine_of, make_runner, same_bits, start, weights_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# one workgroup per sample | ragged tails | planes that are no multiple of the per-workgroup chunk | C = 8 | the full-resolution scene size
SHAPES = [(1, 4, 16, 16, 1), (3, 4, 48, 32, 2), (2, 8, 32, 80, 3), (5, 4, 16, 48, 4), (2, 4, 400, 400, 5)]
GUARD = 64
U = 2.0 ** -23


def _lib():
    from lgteun_amd import _lib
    return _lib.lib()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n, dtype):
    """(buffer, view of n elements) with GUARD elements of NaN on each side, the view NaN too"""
    buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, what):
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all()), (what, 'written outside the output')


def _workspace(B, C, H, W):
    need = _lib().lg_qnr_workspace_bytes(B, C, H, W)
    assert need > 0 and need % 8 == 0
    return _guarded(need // 8, torch.float64) + (need,)


def qnr_stats(x, ws, need, want_q=True):
    """x = (out, pan, ms, pan_l) on the device -> (q [B,2,P] or None, table [P]) as device tensors, guards checked"""
    out, pan, ms, pan_l = x
    B, C, H, W = out.shape
    P = qh.n_pairs(C)[1]
    qb, q = _guarded(B * 2 * P, torch.float64) if want_q else (None, None)
    tb, table = _guarded(P, torch.float64)
    rc = _lib().lg_qnr_stats(_ptr(out), _ptr(pan), _ptr(ms), _ptr(pan_l), _ptr(q), _ptr(table), B, C, H, W, _ptr(ws), need, _stream())
    assert rc == 0, _lib().lg_last_error()
    torch.cuda.synchronize()
    _intact(tb, 'table')
    if want_q:
        _intact(qb, 'q')
    return (q.view(B, 2, P) if want_q else None), table


def qnr_grad(x, table, ws, need, b_global=None, scale=1.0, old=None, loss0=0.0):
    """-> dout [B,C,H,W], loss_accum (float), indices [3]; `old`: the dout to accumulate onto (accumulate = 1)"""
    out, pan = x[0], x[1]
    B, C, H, W = out.shape
    db, dout = _guarded(out.numel(), torch.float32)
    if old is not None:
        dout.copy_(old.reshape(-1))
    lb, loss = _guarded(1, torch.float32)
    loss.fill_(loss0)
    ib, idx = _guarded(3, torch.float64)
    rc = _lib().lg_qnr_grad(_ptr(out), _ptr(pan), _ptr(table), _ptr(dout), _ptr(loss), _ptr(idx), B, B if b_global is None else b_global, C, H, W,
                            float(scale), int(old is not None), _ptr(ws), need, _stream())
    assert rc == 0, _lib().lg_last_error()
    torch.cuda.synchronize()
    for b, n in ((db, 'dout'), (lb, 'loss_accum'), (ib, 'indices')):
        _intact(b, n)
    assert not bool(torch.isnan(dout).any()), 'a dout element was not written'
    return dout.view(B, C, H, W), loss.cpu().numpy()[0], idx.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, seed):
    """inputs on the device, the fp64 reference (computed once per shape) and one plain device run"""
    host = qh.make_inputs(B, C, H, W, seed)
    ref = qh.reference(*host)
    x = tuple(t.cuda() for t in host)
    wb, ws, need = _workspace(B, C, H, W)
    q, table = qnr_stats(x, ws, need)
    dout, loss, idx = qnr_grad(x, table, ws, need)
    _intact(wb, 'workspace')
    return dict(host=host, x=x, ref=ref, ws=ws, need=need, q=q, table=table, dout=dout, loss=loss, idx=idx)


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _dout_ok(dout, g):
    """one fp32 rounding of the fp64 gradient with a factor of two to spare, plus a floor for the order of the fp64 sums"""
    d = dout.double().cpu().numpy()
    bound = U * np.abs(g) + 1e-9 * np.abs(g).max()
    worst = float(np.max(np.abs(d - g) / bound))
    print(f'dout: worst |dout - g| / bound = {worst:.3f}, max |g| = {np.abs(g).max():.3e}')
    return worst <= 1.0


@pytest.mark.parametrize('B,C,H,W,seed', SHAPES)
def test_op_against_the_fp64_restatement(B, C, H, W, seed):
    c = _case(B, C, H, W, seed)
    ref = c['ref']
    rq, rt = _rel(c['q'].cpu().numpy(), ref['q']), _rel(c['table'].cpu().numpy(), ref['table'])
    ri = _rel(c['idx'], ref['indices'])
    rl = abs(float(c['loss']) - ref['indices'][2]) / ref['indices'][2]
    print(f'q rel {rq:.2e}  table rel {rt:.2e}  indices rel {ri:.2e}  loss_accum rel {rl:.2e}')
    assert rq <= 1e-11 and rt <= 1e-11 and ri <= 1e-11
    assert rl <= U
    assert _dout_ok(c['dout'], ref['grad'])


@pytest.mark.parametrize('B,C,H,W,seed', SHAPES)
def test_op_accumulate_scale_and_global_batch(B, C, H, W, seed):
    c = _case(B, C, H, W, seed)
    x, ws, need, table = c['x'], c['ws'], c['need'], c['table']
    # scale applies to dout only; loss_accum is added to
    s = 0.37
    d_s, loss_s, idx_s = qnr_grad(x, table, ws, need, scale=s, loss0=1.5)
    assert _dout_ok(d_s, float(np.float32(s)) * c['ref']['grad'])
    assert loss_s == np.float32(1.5) + c['loss'] and np.array_equal(idx_s, c['idx'])
    # accumulate = 1: old + fl32(scale g) in fp32, exactly
    old = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).cuda()
    d_a, _, _ = qnr_grad(x, table, ws, need, scale=s, old=old)
    assert same_bits(d_a, old + d_s)
    # B_global = 2 B: as if a second rank had contributed the same sums
    t2 = table * 2
    ref2 = qh.reference(*c['host'], b_global=2 * B, table=c['ref']['table'] * 2)
    d_g, loss_g, idx_g = qnr_grad(x, t2, ws, need, b_global=2 * B)
    assert _dout_ok(d_g, ref2['grad'])
    assert _rel(idx_g, ref2['indices']) <= 1e-11 and abs(float(loss_g) - ref2['indices'][2] / 2) <= U * ref2['indices'][2] / 2
    # the same calls give the same bits
    q2, table2 = qnr_stats(x, ws, need)
    d2, loss2, idx2 = qnr_grad(x, table2, ws, need)
    assert torch.equal(q2.view(torch.int64), c['q'].view(torch.int64)) and torch.equal(table2.view(torch.int64), table.view(torch.int64))
    assert same_bits(d2, c['dout']) and loss2.tobytes() == c['loss'].tobytes() and idx2.tobytes() == c['idx'].tobytes()


@pytest.mark.parametrize('B,C,H,W,seed', [s for s in SHAPES if s[0] > 1])
def test_a_samples_q_row_has_the_same_bits_alone_and_inside_a_batch(B, C, H, W, seed):
    c = _case(B, C, H, W, seed)
    n = B - 1
    x1 = tuple(t[n:n + 1].clone() for t in c["x"])
    wb, ws, need = _workspace(1, C, H, W)
    q1, _ = qnr_stats(x1, ws, need)
    _intact(wb, 'workspace')
    assert torch.equal(q1[0].view(torch.int64), c['q'][n].view(torch.int64))


# ------------------------------------------------------------------------------------------------------------------------
# the train step: C = 4, K = 2, PAN 32 x 32, B = 2, dropout off
# ------------------------------------------------------------------------------------------------------------------------
STEP_SEED = 21


def _batch(seed=STEP_SEED):
    out, pan, ms, pan_l = (t.cuda() for t in qh.make_inputs(2, 4, 32, 32, seed))
    return dict(input_lr=ms, input_pan=pan, input_pan_l=pan_l, target=out, image_id=['i0', 'i1'])


def _fresh(tmp_path, tag, train_cfg=None, entry=None):
    runner, _ = make_runner(tmp_path, 'l1', entry or dict(type='Adam', lr=1e-3), train_cfg, step_size=100, tag=tag)
    start(runner)
    return runner, engine_of(runner), runner.optim_dict['core_module']


def _forward(eng, b):
    from lgteun_amd._lib import LG_FLAG_DROPOUT, LG_FLAG_SAVE
    flags = (eng.base_flags(True) | LG_FLAG_SAVE) & ~LG_FLAG_DROPOUT
    out, saved = eng.forward_raw(b['input_lr'], b['input_pan'], flags, 0)
    return out, saved, flags


def _backward(eng, b, dout):
    """the flat gradients of a fresh forward + backward_raw fed `dout`"""
    _, saved, flags = _forward(eng, b)
    g = torch.zeros(eng.total, device='cuda')
    eng.backward_raw(saved, dout, g, flags, 0)
    torch.cuda.synchronize()
    return g


def _hand_qnr(eng, out, b, dout, scale, accumulate, loss):
    B, C, H, W = out.shape
    need = eng.lib.lg_qnr_workspace_bytes(B, C, H, W)
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    table = torch.empty(qh.n_pairs(C)[1], dtype=torch.float64, device='cuda')
    assert eng.lib.lg_qnr_stats(_ptr(out), _ptr(b['input_pan']), _ptr(b['input_lr']), _ptr(b['input_pan_l']), None, _ptr(table), B, C, H, W,
                                _ptr(ws), need, _stream()) == 0
    assert eng.lib.lg_qnr_grad(_ptr(out), _ptr(b['input_pan']), _ptr(table), _ptr(dout), _ptr(loss), None, B, B, C, H, W, scale, accumulate,
                               _ptr(ws), need, _stream()) == 0


def test_unsupervised_step_against_backward_of_three_douts(tmp_path):
    """train_step(gt=None, noref_weight=1): its gradient buffer is that of backward_raw fed (a) the step's own dout, bit for bit; and
    against (b) the fp32-rounded fp64-restatement gradient of the step's output it is, per live tensor, no further off than (c) the
    gradient QNRLoss gives in fp32 autograd -- the noise of the reference's own arithmetic, margin 1x since the fused dout is
    correctly rounded.  Measured on an MI355X: G_fused equals G_ref bit for bit on every live tensor (worst ratio 0.000; printed)."""
    from lgteun_amd.losses import QNRLoss
    b = _batch()
    _, eng, opt = _fresh(tmp_path, 'a')
    first = eng.flat.clone()
    loss_t = eng.train_step(b['input_lr'], b['input_pan'], None, opt, pan_l=b['input_pan_l'], noref_weight=1.0)
    torch.cuda.synchronize()
    assert loss_t.data_ptr() == eng._noref.data_ptr() and float(eng._loss) == 0.0 and not torch.equal(eng.flat, first)
    G_fused, dout = eng.gflat.clone(), eng._qnr_last['dout']
    _, e2, _ = _fresh(tmp_path, 'b')
    assert same_bits(e2.flat, first)
    out, _, _ = _forward(e2, b)
    host = (out.cpu(), b['input_pan'].cpu(), b['input_lr'].cpu(), b['input_pan_l'].cpu())
    ref = qh.reference(*host)                                    # the entry condition, on the step's own output
    assert abs(float(loss_t) - ref['indices'][2]) <= U * ref['indices'][2]
    assert np.abs(eng._qnr_last['indices'].cpu().numpy() - ref['indices']).max() <= 1e-11
    assert abs(eng.global_loss('noref') - ref['indices'][2]) <= U * ref['indices'][2] and eng.global_loss() == 0.0
    assert same_bits(_backward(e2, b, dout), G_fused)                                              # (a)
    G_ref = _backward(e2, b, torch.from_numpy(ref['grad']).float().cuda())                          # (b)
    x = out.clone().requires_grad_(True)
    QNRLoss()(pan=b['input_pan'], ms=b['input_lr'], out=x, pan_l=b['input_pan_l']).backward()
    G_torch = _backward(e2, b, x.grad)                                                              # (c)
    worst = 0.0
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        ef = float((G_fused[o:o + n] - G_ref[o:o + n]).abs().max())
        et = float((G_torch[o:o + n] - G_ref[o:o + n]).abs().max())
        worst = max(worst, ef / et if et else (0.0 if ef == 0.0 else float('inf')))
        assert ef <= et, (eng.names[i], ef, et)
    print(f'fused vs fp64-restatement gradient: worst ratio to the fp32 autograd error over live tensors {worst:.3f}')


def test_combined_step_equals_the_hand_sequence(tmp_path):
    """l1 + 0.1 qnr: lg_l1_loss writes dout, lg_qnr_grad adds to it, then backward and Adam -- bit for bit"""
    b = _batch()
    _, eng, opt = _fresh(tmp_path, 'a')
    loss_t = eng.train_step(b['input_lr'], b['input_pan'], b['target'], opt, loss_weight=1.0, loss_type='l1', pan_l=b['input_pan_l'],
                            noref_weight=0.1)
    assert loss_t.data_ptr() == eng._loss.data_ptr()
    _, e2, o2 = _fresh(tmp_path, 'b')
    e2._gbuf.zero_()
    out, saved, flags = _forward(e2, b)
    dout = torch.empty_like(out)
    assert e2.lib.lg_l1_loss(_ptr(out), _ptr(b['target']), _ptr(dout), _ptr(e2._loss), out.numel(), out.numel(), 1.0, _stream()) == 0
    _hand_qnr(e2, out, b, dout, 0.1, 1, e2._noref)
    e2.backward_raw(saved, dout, e2.gflat, flags, 0)
    o2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng._qnr_last['dout'], dout)
    assert same_bits(eng.gflat, e2.gflat)
    assert same_bits(eng.flat, e2.flat)
    # the QNR scalar is one lane's add; lg_l1_loss adds its workgroups' shares with atomics, in any order
    assert same_bits(eng._noref, e2._noref) and float(eng._noref) > 0
    assert float(eng._loss) > 0 and abs(float(eng._loss) - float(e2._loss)) <= 1e-6 * float(e2._loss)


def test_zero_weight_is_the_plain_step(tmp_path):
    b = _batch()
    _, e1, o1 = _fresh(tmp_path, 'a')
    _, e2, o2 = _fresh(tmp_path, 'b')
    for _ in range(2):
        e1.train_step(b['input_lr'], b['input_pan'], b['target'], o1)
        e2.train_step(b['input_lr'], b['input_pan'], b['target'], o2, pan_l=b['input_pan_l'], noref_weight=0.0)
    torch.cuda.synchronize()
    assert same_bits(e1.gflat, e2.gflat) and same_bits(e1.flat, e2.flat) and float(e2._noref) == 0.0 and e2._qnr_last is None
    assert abs(float(e1._loss) - float(e2._loss)) <= 1e-6 * float(e1._loss)      # lg_l1_loss adds its workgroups' shares with atomics
    with pytest.raises(ValueError, match='input_pan_l'):
        e2.train_step(b['input_lr'], b['input_pan'], b['target'], o2, noref_weight=0.5)
    with pytest.raises(ValueError, match='noref_weight'):
        e2.train_step(b['input_lr'], b['input_pan'], None, o2)


def test_accumulation_window_equals_the_hand_sequence(tmp_path):
    """accumulate = 2: each micro-batch's QNR is its own, its dout scaled by 1/2; one optimizer step at the window's end"""
    micro = [_batch(STEP_SEED), _batch(STEP_SEED + 1)]
    _, eng, opt = _fresh(tmp_path, 'a', train_cfg=dict(accumulate=2))
    first = eng.flat.clone()
    eng.train_step(micro[0]['input_lr'], micro[0]['input_pan'], None, opt, pan_l=micro[0]['input_pan_l'], noref_weight=1.0)
    assert same_bits(eng.flat, first) and opt._step == 0
    eng.train_step(micro[1]['input_lr'], micro[1]['input_pan'], None, opt, pan_l=micro[1]['input_pan_l'], noref_weight=1.0)
    assert opt._step == 1
    _, e2, o2 = _fresh(tmp_path, 'b')
    e2._gbuf.zero_()
    for b in micro:
        out, saved, flags = _forward(e2, b)
        dout = torch.empty_like(out)
        _hand_qnr(e2, out, b, dout, 0.5, 0, e2._noref)
        e2.backward_raw(saved, dout, e2.gflat, flags, 0)
    o2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng._gbuf, e2._gbuf)
    assert same_bits(eng.flat, e2.flat) and not same_bits(eng.flat, first)
    mean = eng.global_loss('noref')                               # the mean over the window's micro-batches
    assert abs(mean - float(e2._noref) / 2) <= 1e-7


def _noref_runner(tmp_path, tag, loss_cfg):
    import lgteun_amd
    from helpers import state_shapes
    from lgteun_amd.compat import Config
    from oracle import detweights as dw
    cfg = dict(ms_chans=4, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=8, bit_depth=11, loss_cfg=loss_cfg,
               optim_cfg={'core_module': dict(type='Adam', lr=1e-3)}, sched_cfg=dict(step_size=100, gamma=0.85),
               model_cfg={'core_module': dict(stage=2)})
    runner = lgteun_amd.build_model('UnlgFormer', Config(cfg), logging.getLogger('t'), None, None, None)
    sd = dw.fill_state_dict(state_shapes(4, 2), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return start(runner)


def test_train_iter_with_noref_loss_is_the_engine_step(tmp_path):
    b = _batch()
    a = _noref_runner(tmp_path, 'a', {'noref_loss': dict(type='qnr', w=1.0)})
    assert getattr(a.optim_dict['core_module'], 'is_fused_lgteun', False)
    logs = []
    a.print_train_log = lambda it, res, freq=10: logs.append(dict(res))
    a.train_iter(1, b, log_freq=1)
    rb, eng, opt = _fresh(tmp_path, 'b')
    eng.train_step(b['input_lr'], b['input_pan'], None, opt, pan_l=b['input_pan_l'], noref_weight=1.0)
    wa, wb = weights_of(a), weights_of(rb)
    for k in wa:
        assert same_bits(wa[k], wb[k]), k
    assert set(logs[0]) == {'noref_loss', 'full_loss'} and logs[0]['noref_loss'] == logs[0]['full_loss'] == eng.global_loss('noref') > 0
    # both terms: the log carries both and their weighted sum
    c = _noref_runner(tmp_path, 'c', {'rec_loss': dict(type='l1', w=1.0), 'noref_loss': dict(type='qnr', w=0.1)})
    c.print_train_log = lambda it, res, freq=10: logs.append(dict(res))
    c.train_iter(1, b, log_freq=1)
    assert set(logs[1]) == {'rec_loss', 'noref_loss', 'full_loss'}
    assert abs(logs[1]['full_loss'] - (logs[1]['rec_loss'] + 0.1 * logs[1]['noref_loss'])) <= 1e-12
    short = {k: v for k, v in b.items() if k != 'input_pan_l'}
    with pytest.raises(ValueError, match='input_pan_l'):
        a.train_iter(2, short, log_freq=1)


def test_two_ranks_equal_the_single_process(tmp_path):
    """two ranks of tests/ddp_qnr_worker.py on the one MI355X (gloo), B = 1 each, one unsupervised step, against a single process with
    B = 2: the table after the all-reduce, the loss and each rank's dout bit for bit (a sum of two terms has one order); gradients and
    live weights within the tolerances of test_two_ranks_with_controls_equal_the_single_process; one extra collective of P doubles."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    procs, logs = [], []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        env.pop('LG_DDP_OVERLAP', None)
        logs.append(str(tmp_path / f'rank{rank}.log'))
        procs.append(subprocess.Popen([sys.executable, '-W', 'ignore', os.path.join(ROOT, 'tests', 'ddp_qnr_worker.py'), str(tmp_path)],
                                      stdout=open(logs[-1], 'w'), stderr=subprocess.STDOUT, env=env, cwd=ROOT))
    try:
        for p in procs:
            assert p.wait(timeout=240) == 0, ''.join(open(f).read()[-3000:] for f in logs)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    r0, r1 = (np.load(tmp_path / f'rank{r}.npz') for r in (0, 1))
    assert int(r0['world']) == 2 and int(r1['world']) == 2
    assert np.abs(r0['single_table'] / 2).min() >= qh.MIN_ENTRY                 # the entry condition, on the step's own output
    for r in (r0, r1):
        assert r['collectives'].tolist() == [[10, 8]] and int(r['bucket_calls']) == 1      # ONE extra collective: P = 10 doubles
        assert r['table'].tobytes() == r0['single_table'].tobytes() and r['indices'].tobytes() == r0['single_indices'].tobytes()
    assert r0['dout'].tobytes() == r0['single_dout'][:1].tobytes() and r1['dout'].tobytes() == r0['single_dout'][1:].tobytes()
    assert np.float32(r0['loss']) + np.float32(r1['loss']) == np.float32(r0['single_loss']) and float(r0['single_loss']) > 0
    for k in ('gflat', 'weights'):
        assert r0[k].tobytes() == r1[k].tobytes(), k
    (a0, b0), (a1, b1) = r0['ranges']
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))      # noqa: E731
    assert rel(r0['gflat'], r0['single_gflat']) < 2e-5
    w, ws = r0['weights'], r0['single_weights']
    assert rel(w[a1:b1], ws[a1:b1]) < 1e-4 and rel(w[a0:b0], ws[a0:b0]) < 1e-4
    assert np.array_equal(w[b0:a1], ws[b0:a1]) and not np.array_equal(w[a1:b1], r0['first'][a1:b1])
