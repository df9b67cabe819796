"""-m gpu: the whole-network passes against HAND SEQUENCES of the per-op entries, bit for bit.

lgteun_forward, lgteun_dead_forward and net_backward (csrc/k_fwd.hip, csrc/k_bwd.hip) string data steps and LGTs into a network: they route Z[i] and X[i],
pick the stage_view / live_view slot, choose which stage's 119 tensors a reduction adds into, index eta[i], ping-pong dzA / dzB and set the flush
points of the reduce queue.  The per-op entries lg_op_resample, lg_op_data_step, lg_op_lgt, lg_op_lgt_bwd and lg_op_data_step_bwd launch the same
kernels on the same plan and route (include/lgteun_hip.h: "same kernels the orchestrators launch"), and every one of them is held to the fp64 oracle
element by element and tensor by tensor (test_gpu_forward_shapes.py, test_gpu_backward_shapes.py at stages 0, 1 and 2, test_gpu_fft_mixer.py,
test_gpu_ops_bwd.py).  Here a network is composed from them by hand, on the module and plan of the whole-network call:

  forward    Z0 = resample(ms, x4), X[0] = Z0
             faithful / live: Z[i+1] = data_step(i, Z[i]); output = lgt(K-1, Z[K]); dead stage i gives lgt(i, Z[i+1])
             chained:         Z[i+1] = data_step(i, X[i]), X[i+1] = lgt(i, Z[i+1]); output = X[K]
             (tests/test_composition_cpu.py: the oracle's forward IS this composition, so test_gpu_chained.py's checker is what is composed here)
  backward   for a fixed random dout, ONE gradient buffer carried through the whole sequence, started from the same non-zero fill as the
             whole-network call's (the reductions ADD):
             faithful / live: lgt_bwd(K-1, Z[K], dout) -> dz; for i = K-1 .. 0: data_step_bwd(i, Z[i], dz) -> dz
             chained:         for i = K-1 .. 0: lgt_bwd(i, Z[i+1], g) -> dz; data_step_bwd(i, X[i], dz) -> g
  A stage's lgt call carries LG_FLAG_SAVE exactly where the whole-network call saves that stage (the saving instance of the forward kernels),
  LG_FLAG_DROPOUT and the seed wherever the whole-network call has them.

Both sides run the same kernels on the same bits, so NOTHING here has a tolerance: the output, each dead stage's output read from the workspace through
lg_workspace_deadout (every stage of a plan that keeps K - 1 slots, stage K-2 alone of one that keeps one) and the whole flat gradient buffer, float by
float with the padding between the tensors, are compared as bits; in faithful and live mode the dead stages' slots and the padding must still be the
fill.  The FFT mixers' branch cut, which keeps the whole-network gates against the oracle at 1e-3 and 5e-3, cannot blur this comparison, and through it
the per-op pins are pins of the network: a wrong stage's weights or slot, a wrong destination, a missing flush or a dz buffer read after it was
overwritten changes bits.  The shared tensors D / DT / R / RT receive K contributions; the merged reduce launch chains them in push order, "bit for
bit what one launch per link gives" (csrc/bwd_kernels.h), and one launch per link is what the hand sequence issues.

Every case asserts its path first: dstep= and fft= from lg_plan_describe, the dead stages' slot count from lg_workspace_deadout (K - 1 slots = the plan
batches its dead stages: one pass, the live stage riding along), the reduce launches of the whole-network backward from lg_debug_reduce_stats
(faithful: 2, chained: 2 K, no flush forced by a full arena or table).  Shapes are the smallest at which each orchestration path exists:

  faithful family (LG_FLAG_FAITHFUL | LG_FLAG_SAVE), PAN H x W, batch B
    a   C=4 K=1 16x16 B=1   no dead stage
    b   C=4 K=2 32x32 B=2   one dead stage, one slot
    c   C=4 K=3 32x32 B=2   the smallest plan that batches its dead stages: one pass, the live stage riding, K slots
    c'  as c with LG_FLAG_STAGEWISE; LG_FLAG_LIVE_APART; LG_FLAG_DEFER_DEAD and lgteun_dead_forward AFTER the backward; live mode (no FAITHFUL); the
        backward as LG_FLAG_BWD_LGT then LG_FLAG_BWD_DATA -- all against the ONE hand sequence of c
    d   C=4 K=4 64x64 B=3   three dead stages, odd batch, the one-launch data step
    e   C=8 K=3 32x32 B=2   dead stages one by one, one slot
    f   C=4 K=3 48x32 B=2   rectangle: Bluestein mixer, tile data step, no batched pass
    g   as c with LG_FLAG_DROPOUT and a seed; as c with precision = 'bf16'
  chained family (LG_FLAG_CHAINED | LG_FLAG_SAVE, and the same forward without SAVE on the inference workspace)
    C=4 K=1 16x16 B=2; C=4 K=2 32x32 B=2; C=4 K=3 32x32 B=3; C=8 K=2 32x32 B=1; C=4 K=3 48x32 B=2; C=4 K=4 16x16 B=1; C=4 K=3 32x32 B=2 with
    dropout, and in bf16; C=4 K=9 16x16 B=1, whose backward issues 18 reduce tables against the 16 slots of k_wgrad.hip's table cache: tables are
    evicted and uploaded again inside one backward ("Results are the same either way"), asserted from the `uploads` counter
  controls (the comparison can fail): the hand sequence of c with two stages' indices swapped in the lgt calls; the hand sequence of g under another
  dropout seed; the chained gradient buffer against the faithful one in every stage-0 LGT tensor.

Observed on an MI355X: all 25 tests pass.  Every one of the 13 faithful / live cases (a, b, c, d, e, f, g with dropout, g in bf16 and the five forms of c) and
of the 9 chained cases is bit-equal to its hand sequence in the output, in every dead output and in the whole gradient buffer -- D / DT / R / RT, which
K stages add into, included: no tensor needed a bound in place of equality, and no orchestration error was found.  Reduce launches as asserted (2 per
faithful backward, one call or two; 2 K per chained one; none forced by a full arena).  The K = 9 case: launches 18, uploads 18 -- every table of that
backward missed the 16-slot cache -- jobs_max 120, and the bits of the hand sequence.  The three controls differ, as they are written to.  The slowest
case takes 0.8 s (case a, the first one: it loads the library), every other one less than 0.45 s."""
import ctypes

import pytest
import torch

from oracle import detweights as dw

pytestmark = pytest.mark.gpu
T = torch.from_numpy

FAITHFUL, SAVE, DROPOUT, BWD_LGT, BWD_DATA, CHAINED, DEFER_DEAD, STAGEWISE, LIVE_APART = 1, 2, 4, 8, 16, 32, 64, 128, 256
SEED, OTHER_SEED = 0x2F5C3A71, 0x2F5C3A72

# id -> C, K, H, W, B, the plan keeps K - 1 dead slots (it batches its dead stages), dstep=, fft=, dropout, precision
SHAPES = {
    'a': (4, 1, 16, 16, 1, False, 'tiles', 'k_fftmix_r', False, None),
    'b': (4, 2, 32, 32, 2, False, 'tiles', 'k_fftmix_r', False, None),
    'c': (4, 3, 32, 32, 2, True, 'tiles', 'k_fftmix_r', False, None),
    'd': (4, 4, 64, 64, 3, True, 'fused', 'k_fftmix_r', False, None),
    'e': (8, 3, 32, 32, 2, False, 'tiles', 'k_fftmix_r', False, None),
    'f': (4, 3, 48, 32, 2, False, 'tiles', 'bluestein', False, None),
    'g-dropout': (4, 3, 32, 32, 2, True, 'tiles', 'k_fftmix_r', True, None),
    'g-bf16': (4, 3, 32, 32, 2, True, 'tiles', 'k_fftmix_r', False, 'bf16'),
}
# the forms of case c: id -> (forward flags besides SAVE, form of the backward)
C_FORMS = {
    'c-stagewise': (FAITHFUL | STAGEWISE, 'one'),
    'c-live-apart': (FAITHFUL | LIVE_APART, 'one'),
    'c-defer-dead': (FAITHFUL | DEFER_DEAD, 'dead-after'),
    'c-live-mode': (0, 'one'),
    'c-split-backward': (FAITHFUL, 'split'),
}
CHAINED_SHAPES = {
    'K1': (4, 1, 16, 16, 2, 'tiles', 'k_fftmix_r', False, None),
    'K2': (4, 2, 32, 32, 2, 'tiles', 'k_fftmix_r', False, None),
    'K3-B3': (4, 3, 32, 32, 3, 'tiles', 'k_fftmix_r', False, None),
    'C8-K2': (8, 2, 32, 32, 1, 'tiles', 'k_fftmix_r', False, None),
    'K3-48x32': (4, 3, 48, 32, 2, 'tiles', 'bluestein', False, None),
    'K4-16x16': (4, 4, 16, 16, 1, 'tiles', 'k_fftmix_r', False, None),
    'K3-dropout': (4, 3, 32, 32, 2, 'tiles', 'k_fftmix_r', True, None),
    'K3-bf16': (4, 3, 32, 32, 2, 'tiles', 'k_fftmix_r', False, 'bf16'),
    'K9-16x16': (4, 9, 16, 16, 1, 'tiles', 'k_fftmix_r', False, None),
}

_HAND = {}      # hand sequences, computed once per configuration, shared, never written to
_NET = {}       # whole-network results by case id (the controls read them)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _module(C, K, precision):
    from gpu_helpers import make_module
    net = make_module(C, K)
    if precision is not None:
        net.precision = precision
    return net


def _inputs(C, H, W, B):
    ms, pan, _ = (T(a).cuda() for a in dw.make_inputs(B, C, H // 4, W // 4, seed=41, kind='smooth'))
    dout = torch.randn((B, C, H, W), generator=torch.Generator(device='cpu').manual_seed(8)).cuda()
    return ms, pan, dout


def _fill(eng):
    return (1e-3 * torch.randn(eng.flat.shape, generator=torch.Generator(device='cpu').manual_seed(9))).cuda()


def _deadout(eng, plan, B, train):
    off, stride = ctypes.c_size_t(), ctypes.c_size_t()
    assert eng.lib.lg_workspace_deadout(plan, B, train, ctypes.byref(off), ctypes.byref(stride)) == 0, eng.lib.lg_last_error()
    return off.value, stride.value


def _assert_route(eng, H, W, B, train, slots, dstep, fft, precision):
    """the path of the case, ahead of any launch: the net line and both levels' forward lines of lg_plan_describe, the dead slots of the workspace"""
    lines = eng.describe(H, W).splitlines()
    head, words = lines[0].split(': ')[0], lines[0].split(': ')[1].split()
    assert f'precision={1 if precision == "bf16" else 0} ' in head + ' ' and 'variant=0x0' in head, lines[0]
    assert f'dstep={dstep}' in words and 'reduce=merged' in words, lines[0]
    for level in (0, 1):
        fwd = [ln for ln in lines if ln.startswith(f'L{level} ') and ' fwd: ' in ln]
        assert len(fwd) == 1 and fwd[0].endswith(f'| fft={fft}'), (fwd, fft)
    _, stride = _deadout(eng, eng.plan(H, W), B, train)
    assert (stride != 0) == slots, (stride, slots)


def _hand(C, K, H, W, B, chained, drop, precision, seed=SEED, perm=None, backward=True):
    """the hand sequence of the module docstring on a fresh module: {'out', 'dead': {stage: output}, 'grads', and, chained, 'out_infer': the same forward
    with nothing saved}.  perm: the stage whose weights the lgt call of stage i uses (a control); backward=False: the forward alone"""
    key = (C, K, H, W, B, chained, drop, precision, seed, perm, backward)
    if key in _HAND:
        return _HAND[key]
    from gpu_helpers import Ops
    ops = Ops(_module(C, K, precision), H, W)
    ms, pan, dout = _inputs(C, H, W, B)
    fl = DROPOUT if drop else 0
    w = list(range(K)) if perm is None else list(perm)

    def forward(save):
        X, Z, lg = [ops.resample(ms, 2)], [None], []
        for i in range(K):
            Z.append(ops.data_step(i, X[i], ms, pan))
            lg.append(ops.lgt(w[i], Z[i + 1], fl | (save if (chained or i == K - 1) else 0), seed))
            X.append(lg[i] if chained else Z[i + 1])
        return X, Z, lg
    X, Z, lg = forward(SAVE)
    res = {'out': lg[K - 1], 'dead': {} if chained else {i: lg[i] for i in range(K - 1)}}
    if chained:
        res['out_infer'] = forward(0)[2][K - 1]
    if backward:
        g = _fill(ops.eng)
        if chained:
            cur = dout
            for i in reversed(range(K)):
                dz, _ = ops.lgt_bwd(i, Z[i + 1], cur, fl, seed, grads=g)
                cur, _ = ops.data_step_bwd(i, X[i], ms, pan, dz, grads=g)
        else:
            dz, _ = ops.lgt_bwd(K - 1, Z[K], dout, fl, seed, grads=g)
            for i in reversed(range(K)):
                dz, _ = ops.data_step_bwd(i, X[i], ms, pan, dz, grads=g)      # (X[i] is Z[i] here)
        res['grads'] = g
    torch.cuda.synchronize()
    _HAND[key] = res
    return res


def _network(C, K, H, W, B, flags, drop, precision, bwd='one', route=None):
    """one whole-network forward + backward on a fresh module, the gradient buffer started from the fill: {'out', 'dead', 'grads', 'stats', 'eng'}"""
    from test_gpu_reduce_merge import _stats
    from lgteun_amd.engine import _ptr, _stream_ptr
    eng = _module(C, K, precision).engine()
    chained = bool(flags & CHAINED)
    train = 2 if chained else 1
    if route is not None:
        _assert_route(eng, H, W, B, train, *route, precision)
    ms, pan, dout = _inputs(C, H, W, B)
    flags |= SAVE | (DROPOUT if drop else 0)
    plan = eng.plan(H, W)
    out, saved = eng.forward_raw(ms, pan, flags, seed=SEED)
    ws = saved[1].view(torch.uint8).reshape(-1)
    off, stride = _deadout(eng, plan, B, train)

    def dead():
        if not (flags & FAITHFUL) or chained or K == 1:
            return {}
        n = B * C * H * W * 4
        stages = range(K - 1) if stride else [K - 2]
        return {i: ws[off + (i * stride if stride else 0):][:n].clone().view(torch.float32).view(B, C, H, W) for i in stages}
    res = {'out': out, 'eng': eng}
    if bwd != 'dead-after':
        res['dead'] = dead()
    g = _fill(eng)
    _stats(eng.lib, True)
    if bwd == 'split':
        eng.backward_raw(saved, dout, g, flags | BWD_LGT, seed=SEED)
        eng.backward_raw(saved, dout, g, flags | BWD_DATA, seed=SEED)
    else:
        eng.backward_raw(saved, dout, g, flags, seed=SEED)
    torch.cuda.synchronize()
    res['stats'] = _stats(eng.lib, False)
    if bwd == 'dead-after':
        from lgteun_amd import _lib
        _lib.check(eng.lib.lgteun_dead_forward(plan, _ptr(eng.flat), _ptr(saved[1]), saved[1].numel(), B, flags, SEED, _stream_ptr()), 'lgteun_dead_forward')
        torch.cuda.synchronize()
        res['dead'] = dead()
    res['grads'] = g
    if chained:
        res['out_infer'] = eng.forward_raw(ms, pan, flags & ~SAVE, seed=SEED)[0]
        torch.cuda.synchronize()
    return res


def _dead_names(eng, K):
    return [n for n in eng.names if any(n.startswith(f'prior_module.{i}.') for i in range(K - 1))]


def _compare(tag, net, hand, K, chained, dead_expected):
    """output, dead outputs and the flat gradient buffer as bits; what the faithful / live backward must leave as it was"""
    from gpu_helpers import assert_bitwise
    eng = net['eng']
    for k in ('out', 'out_infer') if chained else ('out',):
        assert bool(torch.isfinite(net[k]).all()), (tag, k, 'not finite')
        assert _same(net[k], hand[k]), (tag, k, int((_bits(net[k]) != _bits(hand[k])).sum()), 'of', net[k].numel(), 'words differ')
    assert sorted(net['dead']) == sorted(dead_expected), (tag, sorted(net['dead']), dead_expected)
    for i, d in net['dead'].items():
        assert bool(torch.isfinite(d).all()), (tag, 'dead output', i, 'not finite')
        assert _same(d, hand['dead'][i]), (tag, 'dead output of stage', i, int((_bits(d) != _bits(hand['dead'][i])).sum()), 'words differ')
    assert bool(torch.isfinite(net['grads']).all()), (tag, 'gradients not finite')
    assert_bitwise(net['grads'], hand['grads'], eng, tag)
    assert _same(net['grads'], hand['grads']), (tag, 'the padding between the gradient tensors differs')
    # what is compared is not the fill: every live tensor received its sum; every other float -- dead stages' slots, padding -- is still the fill
    fill = _fill(eng)
    dead = set() if chained else set(_dead_names(eng, K))
    assert len(dead) == (0 if chained else 119 * (K - 1))
    untouched = torch.ones(fill.numel(), dtype=torch.bool, device=fill.device)
    for n, o, p in zip(eng.names, eng.offsets, eng.params):
        if n not in dead:
            untouched[o:o + p.numel()] = False
            assert not torch.equal(net['grads'][o:o + p.numel()], fill[o:o + p.numel()]), (tag, n, 'received nothing')
    assert torch.equal(_bits(net['grads'])[untouched], _bits(fill)[untouched]), (tag, 'a dead slot or the padding was written')


def _faithful_case(cid):
    shape = SHAPES['c' if cid in C_FORMS else cid]
    C, K, H, W, B, slots, dstep, fft, drop, precision = shape
    flags, bwd = C_FORMS.get(cid, (FAITHFUL, 'one'))
    net = _network(C, K, H, W, B, flags, drop, precision, bwd, route=(slots, dstep, fft))
    _NET[cid] = net
    return net, shape


@pytest.mark.parametrize('cid', list(SHAPES) + list(C_FORMS))
def test_faithful_and_live_network_is_the_hand_sequence(cid):
    net, (C, K, H, W, B, slots, dstep, fft, drop, precision) = _faithful_case(cid)
    st = net['stats']
    assert st['launches'] == 2 and st['self_flushes'] == 0, st          # the LGT's reductions, then the K data steps' as one chain per parameter
    hand = _hand(C, K, H, W, B, False, drop, precision)
    dead = [] if (cid == 'c-live-mode' or K == 1) else (list(range(K - 1)) if slots else [K - 2])
    _compare(cid, net, hand, K, False, dead)


@pytest.mark.parametrize('cid', list(CHAINED_SHAPES))
def test_chained_network_is_the_hand_sequence(cid):
    C, K, H, W, B, dstep, fft, drop, precision = CHAINED_SHAPES[cid]
    net = _network(C, K, H, W, B, CHAINED, drop, precision, route=(False, dstep, fft))
    _NET['chained-' + cid] = net
    st = net['stats']
    assert st['launches'] == 2 * K and st['self_flushes'] == 0, st      # a launch per LGT and per data step
    if K == 9:
        print('reduce tables uploaded inside one backward of K = 9:', st)
        assert st['uploads'] > 16, st                                   # 18 tables on 16 cache slots: evicted and uploaded again
    hand = _hand(C, K, H, W, B, True, drop, precision)
    _compare('chained ' + cid, net, hand, K, True, [])
    assert _same(net['out'], net['out_infer'])


# ---- controls: the comparison can fail
def _differs(net, hand):
    return not _same(net['out'], hand['out']) or any(not _same(d, hand['dead'][i]) for i, d in net['dead'].items())


def test_control_swapped_stage_indices_differ():
    """the hand sequence of c with stages 0 and 2 swapped in the lgt calls: another network, in the output and in a dead output"""
    net = _NET.get('c') or _faithful_case('c')[0]
    C, K, H, W, B = SHAPES['c'][:5]
    assert not _differs(net, _hand(C, K, H, W, B, False, False, None))
    assert _differs(net, _hand(C, K, H, W, B, False, False, None, perm=(2, 1, 0), backward=False))


def test_control_another_dropout_seed_differs():
    net = _NET.get('g-dropout') or _faithful_case('g-dropout')[0]
    C, K, H, W, B = SHAPES['g-dropout'][:5]
    assert not _differs(net, _hand(C, K, H, W, B, False, True, None))
    assert _differs(net, _hand(C, K, H, W, B, False, True, None, seed=OTHER_SEED, backward=False))


def test_control_chained_gradients_are_not_the_faithful_ones():
    """same shape, same fill, same seed: every stage-0 LGT tensor is the fill in faithful mode and fill + a gradient in chained mode"""
    faithful = _NET.get('g-dropout') or _faithful_case('g-dropout')[0]
    C, K, H, W, B, dstep, fft, drop, precision = CHAINED_SHAPES['K3-dropout']
    assert (C, K, H, W, B, drop) == SHAPES['g-dropout'][:5] + (SHAPES['g-dropout'][8],)
    chained = _NET.get('chained-K3-dropout') or _network(C, K, H, W, B, CHAINED, drop, precision)
    eng = chained['eng']
    names = [n for n in eng.names if n.startswith('prior_module.0.')]
    assert len(names) == 119
    for n, o, p in zip(eng.names, eng.offsets, eng.params):
        if n in names:
            assert not torch.equal(chained['grads'][o:o + p.numel()], faithful['grads'][o:o + p.numel()]), n
