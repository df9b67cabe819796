"""-m gpu: the device-resident dataset (lgteun_amd/resident.py, kernels k_batch_assemble / k_pyr_down2) against the host path it
replaces -- `build_loader(cfg)` on the same files, `num_workers=0`, same order.  Every comparison is torch.equal except input_pan_l of
float32 sets (one fp32 ulp: both sides compute the pyramid in fp64, whose error is far below half an fp32 ulp, so they can differ only
where the final rounding sits on a tie).  No test starts a process; two-rank cases build two loaders in this one."""
import logging
import os

import numpy as np
import pytest
import torch

from helpers import state_shapes
from oracle import detweights as dw
from resident_sets import write_set

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
KEYS = ('input_lr', 'input_pan', 'target', 'input_pan_l')
BIT_DEPTH = 11

# name -> write_set arguments; the integer sets cover the full range of their type
SETS = {
    'u16c4': dict(n=37, C=4, H=128, W=128, dtype='uint16'),
    'u16c8': dict(n=5, C=8, H=64, W=64, dtype='uint16', seed=1),
    'u8': dict(n=6, C=4, H=80, W=48, dtype='uint8', seed=2),
    'f32': dict(n=6, C=4, H=208, W=176, dtype='float32', seed=3),
    'full400': dict(n=3, C=4, H=400, W=400, dtype='uint16', with_mul=False, seed=4),
    'u16rect': dict(n=4, C=4, H=80, W=48, dtype='uint16', seed=5),
    'u16wide': dict(n=3, C=4, H=208, W=176, dtype='uint16', seed=6),
    'u8sq': dict(n=3, C=4, H=128, W=128, dtype='uint8', seed=7),
    'u8big': dict(n=2, C=4, H=400, W=400, dtype='uint8', with_mul=False, seed=8),
    'f32sq': dict(n=3, C=4, H=128, W=128, dtype='float32', seed=9),
}
_dirs = {}


@pytest.fixture(scope='module')
def sets(tmp_path_factory):
    root = tmp_path_factory.mktemp('resident_sets')

    def get(name):
        if name not in _dirs:
            _dirs[name] = write_set(root / name, **SETS[name])
        return _dirs[name]
    return get


def _cfg(d, batch_size, norm_input=False, shuffle=False, **extra):
    return dict(dataset=dict(type='PSDataset', image_dirs=[d], bit_depth=BIT_DEPTH, norm_input=norm_input), batch_size=batch_size,
                num_workers=0, shuffle=shuffle, **extra)


def _host(d, batch_size, norm_input=False):
    from lgteun_amd.dataset import build_loader
    return list(build_loader(_cfg(d, batch_size, norm_input))[0])


def _resident(d, batch_size, norm_input=False, **kw):
    from lgteun_amd.dataset import build_loader
    loader, sampler = build_loader(_cfg(d, batch_size, norm_input), device=DEV, resident=True, **kw)
    assert sampler is None
    return loader


def _ulps(a, b):
    """largest distance in units of the last place between two float32 tensors of one sign"""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


def _same(got, want, float_set=False, what=''):
    assert list(got) == list(want), (what, list(got), list(want))
    assert got['image_id'] == list(want['image_id']), what
    for k in got:
        if k == 'image_id':
            continue
        g, w = got[k].cpu(), want[k].cpu()
        assert g.dtype == torch.float32 and g.shape == w.shape and g.is_contiguous(), (what, k, g.shape, w.shape)
        if float_set and k == 'input_pan_l':
            d = _ulps(g, w)
            print(f'{what} {k}: {d} ulp, {int((g != w).sum())} of {g.numel()} differ')
            assert d <= 1, (what, k, d)
        else:
            assert torch.equal(g, w), (what, k, int((g != w).sum()), float((g - w).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# batches against the host path
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm_input', [False, True])
@pytest.mark.parametrize('name', ['u16c4', 'u16c8', 'u8', 'f32', 'full400'])
def test_batches_equal_the_host_path(sets, name, norm_input):
    d = sets(name)
    want = _host(d, 4, norm_input)
    loader = _resident(d, 4, norm_input)
    got = list(loader)
    assert len(got) == len(want) == len(loader) and got[-1]['input_lr'].shape[0] == (SETS[name]['n'] - 1) % 4 + 1     # a last partial batch
    assert ('target' in got[0]) == SETS[name].get('with_mul', True)
    for i, (g, w) in enumerate(zip(got, want)):
        assert type(g) is dict and all(v.device == torch.device(DEV) for k, v in g.items() if k != 'image_id')
        _same(g, w, name == 'f32', f'{name} norm={norm_input} batch {i}')
    st = loader.store
    assert len(st) == SETS[name]['n'] and st.image_ids == [f'im{i:04d}' for i in range(len(st))]
    item = {'uint8': 1, 'uint16': 2, 'float32': 4}[SETS[name]['dtype']]
    C, H, W = SETS[name]['C'], SETS[name]['H'], SETS[name]['W']
    planes = 1 + C / 16 + (C if 'target' in got[0] else 0)
    assert st.nbytes == len(st) * (int(planes * H * W) * item + H * W // 16 * 4)


@pytest.mark.parametrize('batch_size', [1, 5, 32])
def test_batch_sizes(sets, batch_size):
    d = sets('u16c4')
    want, got = _host(d, batch_size), list(_resident(d, batch_size))
    assert len(got) == len(want) == -(-37 // batch_size)
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, False, f'bs={batch_size} batch {i}')
    dropped = list(_resident_drop(d, batch_size))
    assert len(dropped) == 37 // batch_size and all(b['input_lr'].shape[0] == batch_size for b in dropped)


def _resident_drop(d, batch_size):
    from lgteun_amd.dataset import build_loader
    return build_loader(_cfg(d, batch_size, drop_last=True), device=DEV, resident=True)[0]


@pytest.mark.parametrize('norm_input', [False, True])
@pytest.mark.parametrize('name', ['u16c4', 'u8', 'f32'])
def test_fold_normalize_equals_data_normalize_on_the_device(sets, name, norm_input):
    from lgteun_amd.base_model import NormalizedBatch, data_normalize
    d = sets(name)
    want = _host(d, 4, norm_input)
    got = list(_resident(d, 4, norm_input, fold_normalize=True))
    for i, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, NormalizedBatch) and g.normalized is True
        w = data_normalize({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in w.items()}, BIT_DEPTH)
        _same(g, w, name == 'f32', f'{name} fold norm={norm_input} batch {i}')


# ------------------------------------------------------------------------------------------------------------------------
# input_pan_l
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['u16c4', 'full400', 'u16rect', 'u16wide', 'u8sq', 'u8big', 'u8', 'f32sq', 'f32'])
def test_pan_l_against_the_host_pyramid(sets, name):
    """integer sets over the full range of the type: bitwise; float32 sets: one ulp"""
    from lgteun_amd.dataset import PSDataset, pyr_down, read_tiff
    from lgteun_amd.resident import ResidentStore
    ds = PSDataset([sets(name)], BIT_DEPTH)
    store = ResidentStore.from_dataset(ds, DEV)
    H, W = SETS[name]['H'], SETS[name]['W']
    got = store.pan_l.cpu()
    assert got.shape == (len(ds), 1, H // 4, W // 4) and got.dtype == torch.float32
    top = 0
    for i, prefix in enumerate(ds.image_prefix_names):
        pan = read_tiff(f'{prefix}_pan.tif')
        top = max(top, float(pan.max()))
        want = torch.from_numpy(np.ascontiguousarray(pyr_down(pyr_down(np.asarray(pan, dtype=np.double))))).float()
        if SETS[name]['dtype'] == 'float32':
            d = _ulps(got[i, 0], want)
            print(f'{name} item {i}: {d} ulp, {int((got[i, 0] != want).sum())} of {want.numel()} differ')
            assert d <= 1, (name, i, d)
        else:
            assert torch.equal(got[i, 0], want), (name, i, int((got[i, 0] != want).sum()), float((got[i, 0] - want).abs().max()))
    if SETS[name]['dtype'] != 'float32':
        assert top == np.iinfo(SETS[name]['dtype']).max


# ------------------------------------------------------------------------------------------------------------------------
# flips
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ud,lr', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('name', ['u16c4', 'u8', 'u16rect', 'f32', 'full400'])
def test_flips_equal_data_augmentation(sets, name, ud, lr):
    from lgteun_amd.dataset import data_augmentation
    d = sets(name)
    plain = list(_resident(d, 4, True))
    loader = _resident(d, 4, True, aug_dict=dict(ud_flip=0.5, lr_flip=0.5))
    loader.aug_draws = lambda epoch: [dict(ud_flip=ud, lr_flip=lr)] * len(loader)        # the draw hook
    got = list(loader)
    for i, (g, p) in enumerate(zip(got, plain)):
        replay = iter([0.0 if ud else 0.9, 0.0 if lr else 0.9])                          # rnd() < 0.5 gives the same booleans
        probs = dict(ud_flip=0.5, lr_flip=0.5)
        want = data_augmentation(p, probs, rng=lambda: next(replay))
        assert probs == dict(ud_flip=ud, lr_flip=lr)
        _same(g, {k: want[k] for k in p}, False, f'{name} ud={ud} lr={lr} batch {i}')
    if ud and lr:                                    # the last selected transform wins: left-right only
        assert torch.equal(got[0]['input_pan'], torch.flip(plain[0]['input_pan'], dims=[3]))


def test_drawn_flips_replay(sets):
    """draws of the loader's own generator: per batch, and a new set every epoch"""
    from lgteun_amd.dataset import data_augmentation
    d = sets('u16c4')
    plain = list(_resident(d, 4))
    loader = _resident(d, 4, aug_dict=dict(ud_flip=0.5, lr_flip=0.5), seed=2)
    for epoch in (0, 1):
        draws = loader.aug_draws(epoch)
        assert len({(x['ud_flip'], x['lr_flip']) for x in draws}) > 1
        for g, p, x in zip(loader, plain, draws):
            replay = iter([0.0 if x['ud_flip'] else 0.9, 0.0 if x['lr_flip'] else 0.9])
            want = data_augmentation(p, dict(ud_flip=0.5, lr_flip=0.5), rng=lambda: next(replay))
            _same(g, {k: want[k] for k in p}, False, f'epoch {epoch}')
    assert loader.aug_draws(0) != loader.aug_draws(1) and loader.epoch == 2


# ------------------------------------------------------------------------------------------------------------------------
# shuffled epochs, ranks
# ------------------------------------------------------------------------------------------------------------------------
def test_shuffled_epochs_follow_the_sharded_sampler(sets):
    from lgteun_amd.dataset import ShardedSampler, build_loader
    from lgteun_amd.resident import ResidentLoader
    d = sets('u16c4')
    whole = list(_resident(d, 37))[0]
    loader = build_loader(_cfg(d, 5, shuffle=True), device=DEV, seed=3, resident=True)[0]
    orders = []
    for epoch in (0, 1, 2):                          # `for batch in loader` reshuffles without help
        smp = ShardedSampler(37, 0, 1, shuffle=True, seed=3)
        smp.set_epoch(epoch)
        order = list(smp)
        orders.append(order)
        assert loader.epoch == epoch and loader.epoch_order() == order
        got = list(loader)
        assert [i for b in got for i in b['image_id']] == [whole['image_id'][i] for i in order]
        for k in KEYS:
            assert torch.equal(torch.cat([b[k] for b in got]), whole[k][order]), (epoch, k)
    assert orders[0] != orders[1] != orders[2]
    loader.set_epoch(0)                              # a resume
    assert [i for b in loader for i in b['image_id']] == [whole['image_id'][i] for i in orders[0]]
    # two ranks: disjoint items, together the padded set
    ranks = [ResidentLoader(loader.store, 5, shuffle=True, rank=r, world=2, seed=3) for r in (0, 1)]
    for epoch in (0, 1):
        parts = []
        for r, ld in enumerate(ranks):
            smp = ShardedSampler(37, r, 2, shuffle=True, seed=3)
            smp.set_epoch(epoch)
            got = list(ld)
            for k in KEYS:
                assert torch.equal(torch.cat([b[k] for b in got]), whole[k][list(smp)]), (epoch, r, k)
            parts.append([i for b in got for i in b['image_id']])
        assert len(parts[0]) == len(parts[1]) == 19
        pad = set(parts[0]) & set(parts[1])          # 37 items padded to 38: exactly one wraps around
        assert len(pad) == 1 and set(parts[0]) | set(parts[1]) == set(whole['image_id'])
    ev = [ResidentLoader(loader.store, 5, rank=r, world=2, evaluation=True) for r in (0, 1)]
    ids = [[i for b in ld for i in b['image_id']] for ld in ev]
    assert not set(ids[0]) & set(ids[1]) and sorted(ids[0] + ids[1]) == whole['image_id']


def test_eight_batches_in_flight_keep_their_contents(sets):
    """references to 8 consecutive batches, no synchronisation in between: an output buffer that is recycled would show"""
    d = sets('u16c4')
    want = _host(d, 4, True)[:8]
    torch.cuda.synchronize()
    it = iter(_resident(d, 4, True))
    held = [next(it) for _ in range(8)]
    torch.cuda.synchronize()
    assert len({b[k].data_ptr() for b in held for k in KEYS}) == 32
    for i, (g, w) in enumerate(zip(held, want)):
        _same(g, w, False, f'held batch {i}')


# ------------------------------------------------------------------------------------------------------------------------
# runner
# ------------------------------------------------------------------------------------------------------------------------
T = torch.from_numpy


def _runner(tmp_path, tag, loaders, K=2, **extra):
    import lgteun_amd
    from lgteun_amd.compat import Config
    cfg = Config(dict(ms_chans=4, work_dir=str(tmp_path / tag), datas='GF-2', cuda=True, max_iter=3, bit_depth=BIT_DEPTH,
                      loss_cfg={'rec_loss': dict(type='l1', w=1.)}, optim_cfg={'core_module': dict(type='Adam', betas=(0.9, 0.999), lr=1.5e-3)},
                      sched_cfg=dict(step_size=1, gamma=0.85), model_cfg={'core_module': dict(stage=K)}, **extra))
    runner = lgteun_amd.build_model('UnlgFormer', cfg, logging.getLogger('t'), *loaders)
    sd = dw.fill_state_dict(state_shapes(4, K), salt=0)
    runner.module_dict['core_module'].load_state_dict({k: T(v) for k, v in sd.items()})
    runner.set_cuda()
    runner.module_dict['core_module'].eval()
    runner.set_optim()
    runner.optim_dict['core_module'].dropout = False
    runner.set_sched()
    return runner


def _train3(runner):
    losses = []
    runner.print_train_log = lambda it, res, freq=10: losses.append(res['full_loss'])
    for it, batch in runner._train_batches(runner._device()):
        runner.train_iter(it, batch, log_freq=1)
        runner.sched_dict['core_module'].step()
    torch.cuda.synchronize()
    assert len(losses) == 3
    return losses, {k: v.detach().cpu().clone() for k, v in runner.module_dict['core_module'].state_dict().items()}


@pytest.fixture(scope='module')
def train_dir(tmp_path_factory):
    return write_set(tmp_path_factory.mktemp('resident_train') / 'train', 6, 4, 32, 32, full_range=False, seed=11)


@pytest.fixture(scope='module')
def tiny_train_dir(tmp_path_factory):
    return write_set(tmp_path_factory.mktemp('resident_train') / 'tiny', 3, 4, 16, 16, full_range=False, seed=13)


@pytest.mark.parametrize('fold', [False, True])
def test_three_train_iterations_equal_the_host_loaders(tmp_path, train_dir, tiny_train_dir, fold):
    """One seed, a fresh module each time: three train_iter calls fed by the resident loader leave the weights and the losses of three
    fed by the host loader, bit for bit.

    What "bit for bit" can mean for the LOSS: lg_l1_loss adds one partial sum per workgroup to the loss scalar with a float atomicAdd, in
    the order the workgroups arrive, and launches ceil(n / 1024) of them (k_recloss.hip: k_l1).  With more than one workgroup two runs on the SAME
    batches may therefore differ in the last bits of the scalar (the gradients do not depend on it: tests/test_gpu_backward.py gates
    their reproducibility).  So the loss is compared bitwise where it is defined bitwise -- PAN 16 x 16, C = 4, one pair per batch:
    n = 1024, one workgroup -- and at PAN 32 x 32 with two pairs per batch (n = 8192, G = 8 workgroups) within the reordering bound: each of
    the G - 1 float additions of non-negative terms rounds by at most half an ulp of the final sum, so two orders differ by at most
    G - 1 = 7 ulp of it.  The weights are compared bitwise in both cases."""
    from lgteun_amd.dataset import build_loader
    for d, bs, loss_ulps in ((tiny_train_dir, 1, 0), (train_dir, 2, 7)):
        cfg = _cfg(d, bs)
        host = build_loader(cfg, device=DEV)[0]
        want_loss, want_sd = _train3(_runner(tmp_path, f'host{bs}', (host, None, None)))
        res = build_loader(cfg, device=DEV, resident=True, fold_normalize=fold)[0]
        got_loss, got_sd = _train3(_runner(tmp_path, f'res{bs}', (res, None, None)))
        print(f'fold={fold} batch size {bs}: losses {got_loss} (resident) {want_loss} (host)')
        assert all(np.isfinite(x) and x > 0 for x in got_loss)
        for g, w in zip(got_loss, want_loss):
            assert abs(g - w) <= loss_ulps * float(np.spacing(np.float32(w))), (bs, got_loss, want_loss)
        moved = sum(not torch.equal(want_sd[k], T(v)) for k, v in dw.fill_state_dict(state_shapes(4, 2), salt=0).items())
        assert moved > 0
        for k in want_sd:
            assert torch.equal(got_sd[k], want_sd[k]), (bs, k)


@pytest.mark.parametrize('fold', [False, True])
def test_runner_evaluation_from_resident_loaders(tmp_path, train_dir, sets, fold):
    """test(ref=True) on the reduced-resolution set and test(ref=False) on a target-less one, with save=True: the same eval_results and
    the same written files as from host loaders"""
    from lgteun_amd.dataset import build_loader
    full = write_set(tmp_path / 'full', 3, 4, 64, 64, with_mul=False, full_range=False, seed=12)
    out = {}
    for tag in ('host', 'res'):
        kw = dict(resident=True, fold_normalize=fold) if tag == 'res' else {}
        l1 = build_loader(_cfg(train_dir, 4), device=DEV, evaluation=True, **kw)[0]
        l0 = build_loader(_cfg(full, 2), device=DEV, evaluation=True, **kw)[0]
        runner = _runner(tmp_path, tag, (None, l0, l1))
        a = runner.test(iter_id=7, save=True, ref=True)
        b = runner.test(iter_id=7, save=True, ref=False)
        assert set(a) == {'PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'} and set(b) == {'D_lambda', 'D_s', 'QNR'}
        files = {}
        for sub in (runner.test_out1, runner.test_out0):
            folder = os.path.join(sub, 'iter_7')
            for f in sorted(os.listdir(folder)):
                files[(os.path.basename(sub), f)] = open(os.path.join(folder, f), 'rb').read()
        out[tag] = (a, b, dict(runner.eval_results), files)
    for i in range(3):                               # (NaN-safe equality: an index that is undefined on noise is so on both paths)
        np.testing.assert_equal(out['res'][i], out['host'][i])
    assert len(out['host'][2]) == 16
    assert sorted(out['res'][3]) == sorted(out['host'][3]) and len(out['host'][3]) == 9
    assert all(f.endswith('_mul_hat.tif') for _, f in out['host'][3])
    assert out['res'][3] == out['host'][3]
