"""-m gpu: the fused spectral and structural training losses -- `lg_sam_loss` / `lg_ssim_loss` per op against losses.SAMLoss /
losses.SSIMLoss run in fp64 on the CPU and against the device evaluation indices, `Engine.train_step(spectral_weight=, struct_weight=)`
against hand sequences of library calls, `loss_cfg['spectral_loss']` / `['struct_loss']` through the runner on both routes, and two
data-parallel ranks against one process.

Accuracy of a dout tensor (recloss_helpers.dout_ratio): its largest error against the fp64 module over the bar
max(2 x the largest error of the same module run in fp32 by torch, 2^-23 |g| + 1e-9 max |g|) must not exceed 1."""
import ctypes
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recloss_helpers as rh
from train_controls_helpers import engine_of, same_bits, start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('sam', 'ssim')
# one window row | one tile | two tiles in a row, one window row more | ragged 16 x 16 tiles in both directions, B = 2 | many tiles, B = 2
SHAPES = [(1, H, W, 'smooth') for H, W in ((11, 12), (16, 16), (12, 28))] + [(2, 44, 76, 'smooth'), (2, 128, 128, 'smooth')]
# ... | variances far below c2 | the planted SAM pixels: identical, parallel, zero, opposite
CASES = [(B, C, H, W, k) for C in (4, 8) for B, H, W, k in SHAPES] + [(1, 4, 16, 28, 'flat'), (2, 4, 16, 16, 'planted'), (2, 8, 16, 16, 'planted')]
GUARD = 64
U = 2.0 ** -23
VALUE_TOL = 1e-6      # ten times the 1e-7 that the fp32 module shows against the fp64 one


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


def run_op(kind, out, gt, b_global=None, scale=1.0, old=None, loss0=0.0, data_range=1.0):
    """one library call on device tensors -> (dout [B,C,H,W], loss_accum as a numpy float32); `old`: the dout to accumulate onto
    (accumulate = 1).  dout, loss_accum and the workspace sit in NaN guard bands, checked behind the call; dout starts as NaN."""
    B, C, H, W = out.shape
    need = _lib().lg_recloss_workspace_bytes(B, C, H, W)
    assert need > 0 and need % 8 == 0
    wb, ws = _guarded(need // 8, torch.float64)
    db, dout = _guarded(out.numel(), torch.float32)
    if old is not None:
        dout.copy_(old.reshape(-1))
    lb, loss = _guarded(1, torch.float32)
    loss.fill_(loss0)
    bg = B if b_global is None else b_global
    if kind == 'sam':
        rc = _lib().lg_sam_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(loss), B, bg, C, H, W, float(scale), int(old is not None), _ptr(ws), need,
                                _stream())
    else:
        rc = _lib().lg_ssim_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(loss), B, bg, C, H, W, float(scale), float(data_range), int(old is not None),
                                 _ptr(ws), need, _stream())
    assert rc == 0, _lib().lg_last_error()
    torch.cuda.synchronize()
    for b, n in ((db, 'dout'), (lb, 'loss_accum'), (wb, 'workspace')):
        _intact(b, n)
    assert not bool(torch.isnan(dout).any()), 'a dout element was not written'
    return dout.view(B, C, H, W), loss.cpu().numpy()[0]


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, how):
    """inputs on the device, the CPU references of both losses (computed once per case) and one plain device run of each"""
    out, gt = rh.make_pair(B, C, H, W, seed=H * W + C, kind='flat' if how == 'flat' else 'smooth')
    cols = None
    if how == 'planted':
        out, gt, cols = rh.plant(out, gt)
    x = (out.cuda(), gt.cuda())
    c = dict(host=(out, gt), x=x, cols=cols)
    for kind in KINDS:
        c[kind] = dict(ref=rh.references(kind, out, gt), run=run_op(kind, *x))
    return c


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,C,H,W,how', CASES)
def test_op_against_the_fp64_module_and_the_device_indices(B, C, H, W, how, kind):
    """Measured on an MI355X (printed): see DESIGN section 3.0.3 for the ratios."""
    from lgteun_amd import device_metrics, metrics
    c = _case(B, C, H, W, how)
    ref, (dout, loss) = c[kind]['ref'], c[kind]['run']
    ratio = rh.dout_ratio(dout, ref)
    e32 = float(np.abs(ref['grad32'] - ref['grad']).max())
    print(f'{kind} {B}x{C}x{H}x{W} {how}: dout error / bar {ratio:.3f}  (fp32 module error {e32:.3e}, max |g| {np.abs(ref["grad"]).max():.3e})  '
          f'loss {float(loss):.7f} vs {ref["loss"]:.7f}')
    assert ratio <= 1.0
    assert abs(float(loss) - ref['loss']) <= VALUE_TOL
    if kind == 'sam':
        index = device_metrics.ref_evaluate_batch(*c['x'], scale=1.0)[:, device_metrics.REF_NAMES.index('SAM')].mean()
        assert abs(float(loss) - float(index)) <= VALUE_TOL
    else:
        index = device_metrics.ref_evaluate_batch(*c['x'], scale=metrics.PEAK)[:, device_metrics.REF_NAMES.index('SSIM')].mean()
        assert abs((1.0 - float(loss)) - float(index)) <= VALUE_TOL
    if c['cols'] is not None and kind == 'sam':
        for col in c['cols']:
            assert bool((dout[0, :, 0, col] == 0).all()), col
        assert int((dout.abs().sum(dim=1) == 0).sum()) == len(c['cols'])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,C,H,W,how', CASES)
def test_op_accumulate_scale_global_batch_and_repeat(B, C, H, W, how, kind):
    c = _case(B, C, H, W, how)
    x, ref, (dout, loss) = c['x'], c[kind]['ref'], c[kind]['run']
    # scale applies to dout only; loss_accum is added to
    s = float(np.float32(0.37))
    d_s, loss_s = run_op(kind, *x, scale=s, loss0=1.5)
    assert rh.dout_ratio(d_s, ref, scale=s) <= 1.0
    assert loss_s == np.float32(1.5) + loss
    # accumulate = 1 on a sentinel-filled dout: sentinel + the accumulate = 0 result, rounded once
    old = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(H + W)).cuda()
    d_a, _ = run_op(kind, *x, scale=s, old=old)
    assert same_bits(d_a, old + d_s)
    # B_global = 2 B: half the gradient, half the share of the loss
    d_g, loss_g = run_op(kind, *x, b_global=2 * B)
    assert rh.dout_ratio(d_g, ref, scale=0.5) <= 1.0
    assert abs(float(loss_g) - float(loss) / 2) <= U * float(loss)
    # the same call gives the same bits
    d2, loss2 = run_op(kind, *x)
    assert same_bits(d2, dout) and loss2.tobytes() == loss.tobytes()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,C,H,W,how', [c for c in CASES if c[0] > 1])
def test_a_samples_dout_has_the_same_bits_alone_and_inside_a_batch(B, C, H, W, how, kind):
    c = _case(B, C, H, W, how)
    n = B - 1
    d1, _ = run_op(kind, *(t[n:n + 1].clone() for t in c['x']), b_global=B)
    assert same_bits(d1[0], c[kind]['run'][0][n])


def test_shapes_the_calls_reject():
    lib = _lib()
    assert lib.lg_recloss_workspace_bytes(2, 4, 32, 32) > 0 and lib.lg_recloss_workspace_bytes(2, 8, 11, 12) > 0
    for B, C, H, W in ((2, 3, 32, 32), (2, 5, 32, 32), (2, 4, 32, 30), (0, 4, 32, 32)):
        assert lib.lg_recloss_workspace_bytes(B, C, H, W) == 0
    out, gt = (t.cuda() for t in rh.make_pair(1, 4, 10, 12, seed=1))
    need = lib.lg_recloss_workspace_bytes(1, 4, 10, 12)
    assert need > 0                                        # the spectral angle needs no window ...
    ws, dout, loss = torch.empty(need // 8, dtype=torch.float64, device='cuda'), torch.empty_like(out), torch.zeros(1, device='cuda')
    assert lib.lg_sam_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(loss), 1, 1, 4, 10, 12, 1.0, 0, _ptr(ws), need, _stream()) == 0
    rc = lib.lg_ssim_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(loss), 1, 1, 4, 10, 12, 1.0, 1.0, 0, _ptr(ws), need, _stream())
    assert rc != 0 and b'at least 11' in lib.lg_last_error()      # ... the structural index does
    for bad in (dict(acc=2), dict(bg=0), dict(ws_bytes=8)):
        rc = lib.lg_sam_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(loss), 1, bad.get('bg', 1), 4, 10, 12, 1.0, bad.get('acc', 0), _ptr(ws),
                             bad.get('ws_bytes', need), _stream())
        assert rc != 0, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# the train step: C = 4, K = 2, PAN 32 x 32, B = 2, dropout off
# ------------------------------------------------------------------------------------------------------------------------
W_SAM, W_SSIM = 0.3, 0.2


def _batch(seed=0):
    from oracle import detweights as dw
    ms, pan, gt = dw.make_inputs(2, 4, 8, 8, seed=11 + seed, kind='smooth')
    T = torch.from_numpy
    return dict(input_lr=T(ms).cuda(), input_pan=T(pan).cuda(), target=T(gt).cuda(), image_id=['i0', 'i1'])


def _runner(tmp_path, tag, loss_cfg, entry=None, train_cfg=None):
    import lgteun_amd
    from helpers import state_shapes
    from lgteun_amd.compat import Config
    from oracle import detweights as dw
    cfg = dict(ms_chans=4, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=8, bit_depth=11, loss_cfg=loss_cfg,
               optim_cfg={'core_module': dict(entry or dict(type='Adam', lr=1e-3))}, sched_cfg=dict(step_size=100, gamma=0.85),
               model_cfg={'core_module': dict(stage=2)})
    if train_cfg is not None:
        cfg['train_cfg'] = dict(train_cfg)
    runner = lgteun_amd.build_model('UnlgFormer', Config(cfg), logging.getLogger('t'), None, None, None)
    sd = dw.fill_state_dict(state_shapes(4, 2), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return start(runner)


ALL_THREE = {'rec_loss': dict(type='l1', w=1.0), 'spectral_loss': dict(type='sam', w=W_SAM), 'struct_loss': dict(type='ssim', w=W_SSIM)}


def _fresh(tmp_path, tag, train_cfg=None):
    runner = _runner(tmp_path, tag, {'rec_loss': dict(type='l1', w=1.0)}, train_cfg=train_cfg)
    return runner, engine_of(runner), runner.optim_dict['core_module']


def _forward(eng, b):
    from lgteun_amd._lib import LG_FLAG_DROPOUT, LG_FLAG_SAVE
    flags = (eng.base_flags(True) | LG_FLAG_SAVE) & ~LG_FLAG_DROPOUT
    out, saved = eng.forward_raw(b['input_lr'], b['input_pan'], flags, 0)
    return out, saved, flags


def _hand_terms(eng, out, gt, dout, div=1.0, rec=True, sam=True, ssim=True):
    """the three op calls in sequence on dout, the loss values into the engine's slots: reconstruction writes, SAM and SSIM add"""
    B, C, H, W = out.shape
    need = eng.lib.lg_recloss_workspace_bytes(B, C, H, W)
    ws = torch.empty(need // 8, dtype=torch.float64, device='cuda')
    acc = 0
    if rec:
        assert eng.lib.lg_l1_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(eng._loss), out.numel(), out.numel(), 1.0 / div, _stream()) == 0
        acc = 1
    if sam:
        assert eng.lib.lg_sam_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(eng._sam), B, B, C, H, W, W_SAM / div, acc, _ptr(ws), need, _stream()) == 0
        acc = 1
    if ssim:
        assert eng.lib.lg_ssim_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(eng._ssim), B, B, C, H, W, W_SSIM / div, 1.0, acc, _ptr(ws), need,
                                    _stream()) == 0


def test_combined_step_equals_the_hand_sequence(tmp_path):
    """l1 + 0.3 sam + 0.2 ssim: the step's gradient buffer is that of backward_raw fed the dout of the three op calls in sequence, bit for
    bit, and so are the weights behind Adam; global_loss of each term is the op-level value, which is the fp64 module's within 1e-6"""
    b = _batch()
    _, eng, opt = _fresh(tmp_path, 'a')
    loss_t = eng.train_step(b['input_lr'], b['input_pan'], b['target'], opt, loss_weight=1.0, loss_type='l1', spectral_weight=W_SAM,
                            struct_weight=W_SSIM)
    assert loss_t.data_ptr() == eng._loss.data_ptr()
    _, e2, o2 = _fresh(tmp_path, 'b')
    e2._gbuf.zero_()
    out, saved, flags = _forward(e2, b)
    dout = torch.empty_like(out)
    _hand_terms(e2, out, b['target'], dout)
    e2.backward_raw(saved, dout, e2.gflat, flags, 0)
    g_hand = e2.gflat.clone()
    o2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng._recloss_last['dout'], dout)
    for i in eng.live_idx:
        o, n = eng.offsets[i], eng.params[i].numel()
        assert same_bits(eng.gflat[o:o + n], g_hand[o:o + n]), eng.names[i]
    assert same_bits(eng.gflat, g_hand) and same_bits(eng.flat, e2.flat)
    assert same_bits(eng._sam, e2._sam) and same_bits(eng._ssim, e2._ssim) and float(eng._noref) == 0.0
    assert eng.global_loss('sam') == float(e2._sam) > 0 and eng.global_loss('ssim') == float(e2._ssim) > 0
    assert abs(eng.global_loss() - float(e2._loss)) <= 1e-6 * float(e2._loss)      # lg_l1_loss adds its workgroups' shares with atomics
    host = (out.cpu(), b['target'].cpu())
    for kind, v in (('sam', eng.global_loss('sam')), ('ssim', eng.global_loss('ssim'))):
        assert abs(v - rh.references(kind, *host)['loss']) <= VALUE_TOL, kind
    with pytest.raises(ValueError, match="'sam' or 'ssim'"):
        eng.global_loss('ergas')


def test_zero_weights_are_the_plain_step(tmp_path):
    b = _batch()
    _, e1, o1 = _fresh(tmp_path, 'a')
    _, e2, o2 = _fresh(tmp_path, 'b')
    for _ in range(2):
        e1.train_step(b['input_lr'], b['input_pan'], b['target'], o1)
        e2.train_step(b['input_lr'], b['input_pan'], b['target'], o2, spectral_weight=0.0, struct_weight=0.0)
    torch.cuda.synchronize()
    assert same_bits(e1.gflat, e2.gflat) and same_bits(e1.flat, e2.flat)
    assert float(e2._sam) == 0.0 and float(e2._ssim) == 0.0 and e2._recloss_last is None
    for kw in (dict(spectral_weight=0.5), dict(struct_weight=0.5)):
        with pytest.raises(ValueError, match='need gt'):
            e2.train_step(b['input_lr'], b['input_pan'], None, o2, pan_l=torch.zeros(2, 1, 8, 8, device='cuda'), noref_weight=1.0, **kw)


def test_accumulation_window_equals_the_hand_sequence(tmp_path):
    """accumulate = 2: every micro-batch's dout at scale w / 2, one optimizer step at the window's end"""
    micro = [_batch(0), _batch(1)]
    _, eng, opt = _fresh(tmp_path, 'a', train_cfg=dict(accumulate=2))
    first = eng.flat.clone()
    kw = dict(loss_weight=1.0, loss_type='l1', spectral_weight=W_SAM, struct_weight=W_SSIM)
    eng.train_step(micro[0]['input_lr'], micro[0]['input_pan'], micro[0]['target'], opt, **kw)
    assert same_bits(eng.flat, first) and opt._step == 0
    eng.train_step(micro[1]['input_lr'], micro[1]['input_pan'], micro[1]['target'], opt, **kw)
    assert opt._step == 1
    _, e2, o2 = _fresh(tmp_path, 'b')
    e2._gbuf.zero_()
    for b in micro:
        out, saved, flags = _forward(e2, b)
        dout = torch.empty_like(out)
        _hand_terms(e2, out, b['target'], dout, div=2.0)
        e2.backward_raw(saved, dout, e2.gflat, flags, 0)
    o2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng.gflat, e2.gflat) and same_bits(eng._gbuf[-2:], e2._gbuf[-2:])
    assert same_bits(eng.flat, e2.flat) and not same_bits(eng.flat, first)
    for which, slot in (('sam', e2._sam), ('ssim', e2._ssim)):      # the mean over the window's micro-batches
        assert abs(eng.global_loss(which) - float(slot) / 2) <= 1e-7


def test_sam_alone_without_a_reconstruction_term(tmp_path):
    """spectral_weight with loss_weight = 0: no reconstruction call; SAM writes dout"""
    b = _batch()
    _, eng, opt = _fresh(tmp_path, 'a')
    first = eng.flat.clone()
    loss_t = eng.train_step(b['input_lr'], b['input_pan'], b['target'], opt, loss_weight=0.0, spectral_weight=W_SAM)
    assert loss_t.data_ptr() == eng._sam.data_ptr() and float(eng._loss) == 0.0 and float(eng._sam) > 0 and not same_bits(eng.flat, first)
    _, e2, o2 = _fresh(tmp_path, 'b')
    e2._gbuf.zero_()
    out, saved, flags = _forward(e2, b)
    dout = torch.full_like(out, float('nan'))
    _hand_terms(e2, out, b['target'], dout, rec=False, ssim=False)
    e2.backward_raw(saved, dout, e2.gflat, flags, 0)
    o2.step_flat(e2)
    torch.cuda.synchronize()
    assert same_bits(eng._gbuf, e2._gbuf) and same_bits(eng.flat, e2.flat)


def test_train_iter_on_both_routes(tmp_path):
    """the runner: the fused step is the engine step and logs every unweighted term; the fused=False route (losses.SAMLoss / SSIMLoss
    through autograd) logs the same terms and leaves gradients that agree with the fused ones within the project's global gradient
    gate, 1e-3 relative L2 over the live tensors"""
    b = _batch()
    logs = []
    a = _runner(tmp_path, 'a', ALL_THREE)
    assert getattr(a.optim_dict['core_module'], 'is_fused_lgteun', False)
    a.print_train_log = lambda it, res, freq=10: logs.append(dict(res))
    a.train_iter(1, b, log_freq=1)
    ea = engine_of(a)
    _, eng, opt = _fresh(tmp_path, 'b')
    eng.train_step(b['input_lr'], b['input_pan'], b['target'], opt, spectral_weight=W_SAM, struct_weight=W_SSIM)
    assert same_bits(ea.gflat, eng.gflat) and same_bits(ea.flat, eng.flat)
    assert set(logs[0]) == {'rec_loss', 'spectral_loss', 'struct_loss', 'full_loss'}
    assert logs[0]['spectral_loss'] == eng.global_loss('sam') and logs[0]['struct_loss'] == eng.global_loss('ssim')
    assert abs(logs[0]['full_loss'] - (logs[0]['rec_loss'] + W_SAM * logs[0]['spectral_loss'] + W_SSIM * logs[0]['struct_loss'])) <= 1e-12
    t = _runner(tmp_path, 'c', ALL_THREE, entry=dict(type='Adam', lr=1e-3, fused=False))
    assert not getattr(t.optim_dict['core_module'], 'is_fused_lgteun', False)
    t.print_train_log = lambda it, res, freq=10: logs.append(dict(res))
    t.train_iter(1, b, log_freq=1)
    assert set(logs[1]) == set(logs[0])
    for k in logs[0]:
        assert abs(logs[1][k] - logs[0][k]) <= 1e-5, (k, logs[1][k], logs[0][k])
    et = engine_of(t)
    num = den = 0.0
    for i in ea.live_idx:
        o, n = ea.offsets[i], ea.params[i].numel()
        g = et.params[i].grad.reshape(-1).double()
        num += float((ea.gflat[o:o + n].double() - g).pow(2).sum())
        den += float(g.pow(2).sum())
    rel = (num / den) ** 0.5
    print(f'fused against fused=False gradients, l1 + sam + ssim: rel_l2 {rel:.3e}')
    assert rel < 1e-3
    # a term alone, and a batch without a target
    s = _runner(tmp_path, 'd', {'struct_loss': dict(type='ssim', w=1.0)})
    s.print_train_log = lambda it, res, freq=10: logs.append(dict(res))
    s.train_iter(1, b, log_freq=1)
    assert set(logs[2]) == {'struct_loss', 'full_loss'} and logs[2]['struct_loss'] == logs[2]['full_loss'] > 0
    short = {k: v for k, v in b.items() if k != 'target'}
    for r in (s, t):
        with pytest.raises(ValueError, match="'target'"):
            r.train_iter(2, short, log_freq=1)


def test_two_ranks_equal_the_single_process(tmp_path):
    """two ranks of tests/ddp_recloss_worker.py on the one MI355X (gloo), B = 1 each, one l1 + sam + ssim step, against a single process
    with B = 2: each rank's dout bit for bit; the loss values to one fp32 addition's rounding (two shares, each rounded to fp32, added in
    another order than the single process's one sum: at most 2 x 2^-23 relative); no collective besides the gradient bucket"""
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
        procs.append(subprocess.Popen([sys.executable, '-W', 'ignore', os.path.join(ROOT, 'tests', 'ddp_recloss_worker.py'), str(tmp_path)],
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
    for r in (r0, r1):
        assert r['collectives'].size == 0 and int(r['bucket_calls']) == 1
    assert r0['dout'].tobytes() == r0['single_dout'][:1].tobytes() and r1['dout'].tobytes() == r0['single_dout'][1:].tobytes()
    for k in ('sam', 'ssim'):
        both, one = float(np.float32(r0[k]) + np.float32(r1[k])), float(r0['single_' + k])
        assert one > 0 and abs(both - one) <= 2 * U * one, (k, both, one)
    for k in ('gflat', 'weights'):
        assert r0[k].tobytes() == r1[k].tobytes(), k
    (a0, b0), (a1, b1) = r0['ranges']
    rel = lambda x, y: float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)))      # noqa: E731
    assert rel(r0['gflat'], r0['single_gflat']) < 2e-5
    w, ws = r0['weights'], r0['single_weights']
    assert rel(w[a1:b1], ws[a1:b1]) < 1e-4 and rel(w[a0:b0], ws[a0:b0]) < 1e-4
    assert not np.array_equal(w[a1:b1], r0['first'][a1:b1])
