"""CPU: the boundary of the device-resident dataset (lgteun_amd/resident.py; C ABI lg_pyr_down2 / lg_batch_assemble of
include/lgteun_hip.h, kernels in lgteun_amd/csrc/k_batch.hip): the exported names, argument validation before any HIP call, the
loader's order and draws, the rejected sets and the host-side packing.  The batches themselves are tested on the GPU
(tests/test_gpu_resident.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from lgteun_amd.dataset import PSDataset, ShardedSampler, read_tiff, write_tiff
from resident_sets import write_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('lg_pyr_down2', 'lg_batch_assemble')


def _lib():
    from lgteun_amd import _lib
    return _lib, _lib.lib()


class _Sized:
    """what a ResidentLoader needs of its store for the order and the draws: a length"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_resident_names_are_exported():
    import lgteun_amd
    from lgteun_amd import resident
    assert lgteun_amd.ResidentStore is resident.ResidentStore and lgteun_amd.ResidentLoader is resident.ResidentLoader
    lib_mod, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'lgteun_hip.h')).read()
    for name in NEW:
        assert name in lib_mod.SIGNATURES and re.search(rf'\b{name}\s*\(', hdr), name
        assert hasattr(ctypes.CDLL(lib_mod.LIB_PATH), name), name
    assert 'k_batch.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    assert lib_mod.LG_ABI_VERSION == L.lg_abi_version() == 2          # additions only
    for name, code in (('LG_DT_U8', lib_mod.LG_DT_U8), ('LG_DT_U16', lib_mod.LG_DT_U16), ('LG_DT_F32', lib_mod.LG_DT_F32)):
        assert int(re.search(rf'#define {name} (\d+)', hdr).group(1)) == code
    assert L.lg_kernel_name(lib_mod.KERNEL_IDS['batch']) == b'k_batch_assemble'


def test_argument_validation_without_a_device():
    """every call here is rejected before any HIP call: the pointers are never dereferenced and nothing is launched"""
    _, L = _lib()
    fake = ctypes.c_void_p(1 << 20)
    null = ctypes.c_void_p(0)

    def assemble(pan=fake, lr=fake, mul=fake, pan_l=fake, N=10, idx=fake, off=0, flips=null, o_pan=fake, o_lr=fake, o_mul=fake, o_pl=fake,
                 B=2, C=4, H=64, W=64, h=16, w=16, dtype=1, divisor=2047.5, n_div=1, post=1.0):
        rc = L.lg_batch_assemble(pan, lr, mul, pan_l, N, idx, off, flips, o_pan, o_lr, o_mul, o_pl, B, C, H, W, h, w, dtype, divisor, n_div, post, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(pan=null), 'null pointer'), (dict(lr=null), 'null pointer'), (dict(pan_l=null), 'null pointer'),
                    (dict(idx=null), 'null pointer'), (dict(o_pan=null), 'null pointer'), (dict(o_lr=null), 'null pointer'),
                    (dict(o_pl=null), 'null pointer'), (dict(mul=null), 'null pointer'), (dict(o_mul=null), 'null pointer'),
                    (dict(B=0), 'B must be'), (dict(B=-3), 'B must be'), (dict(B=70000), 'B must be'),
                    (dict(C=0), 'C must be'), (dict(C=17), 'C must be'),
                    (dict(H=60), '4 x the MS size'), (dict(W=68), '4 x the MS size'), (dict(h=0, H=0), '4 x the MS size'),
                    (dict(dtype=3), 'sample type'), (dict(dtype=-1), 'sample type'),
                    (dict(n_div=3), 'divide count'), (dict(n_div=-1), 'divide count'),
                    (dict(divisor=0.0), 'divisor'), (dict(divisor=float('inf')), 'divisor'), (dict(post=float('nan')), 'scale'),
                    (dict(N=0), 'N must be'), (dict(off=-1), 'N must be'),
                    (dict(pan=ctypes.c_void_p((1 << 20) + 4)), 'aligned'), (dict(o_lr=ctypes.c_void_p((1 << 20) + 8)), 'aligned')):
        rc, err = assemble(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)

    def pyr(pan=fake, out=fake, planes=3, H=64, W=64, dtype=1):
        rc = L.lg_pyr_down2(pan, out, planes, H, W, dtype, null)
        return rc, L.lg_last_error().decode()

    for kw, msg in ((dict(pan=null), 'null pointer'), (dict(out=null), 'null pointer'), (dict(planes=0), 'planes'), (dict(H=4), 'multiples of 4'),
                    (dict(W=66), 'multiples of 4'), (dict(H=0), 'multiples of 4'), (dict(dtype=5), 'sample type'),
                    (dict(planes=1 << 40), 'planes')):
        rc, err = pyr(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('evaluation', [False, True])
def test_loader_order_is_the_sharded_samplers(world, evaluation):
    from lgteun_amd.resident import ResidentLoader
    n, bs = 23, 4                                   # divisible by neither 2 nor 3
    per_epoch = []
    for epoch in range(3):
        seen = []
        for rank in range(world):
            loader = ResidentLoader(_Sized(n), bs, shuffle=True, rank=rank, world=world, seed=5, evaluation=evaluation)
            loader.set_epoch(epoch)
            want = ShardedSampler(n, rank, world, shuffle=True, seed=5, pad=not evaluation)
            want.set_epoch(epoch)
            got = loader.epoch_order()
            assert got == list(want) and got == loader.epoch_order(epoch)
            assert len(loader) == -(-len(got) // bs)
            seen.append(got)
        flat = [i for part in seen for i in part]
        if evaluation:                              # every item exactly once over the ranks
            assert sorted(flat) == list(range(n))
        else:                                       # padded by wrapping: equal counts, the whole set covered
            assert len({len(p) for p in seen}) == 1 and set(flat) == set(range(n)) and len(flat) == -(-n // world) * world
        if world > 1 and evaluation:
            assert all(not (set(a) & set(b)) for i, a in enumerate(seen) for b in seen[i + 1:])      # the ranks are disjoint
        per_epoch.append(seen)
    assert per_epoch[0] != per_epoch[1] and per_epoch[1] != per_epoch[2]          # consecutive epochs differ
    drop = ResidentLoader(_Sized(n), bs, shuffle=True, rank=0, world=world, seed=5, drop_last=True)
    assert drop.epoch_order() == list(ShardedSampler(n, 0, world, shuffle=True, seed=5, drop_last=True)) and len(drop) == (n // world) // bs
    plain = ResidentLoader(_Sized(n), bs)           # no shuffle: the files' order
    assert plain.epoch_order() == list(range(n))


def test_padded_ranks_are_disjoint_where_the_set_divides():
    from lgteun_amd.resident import ResidentLoader
    a, b = (ResidentLoader(_Sized(24), 4, shuffle=True, rank=r, world=2, seed=1).epoch_order() for r in (0, 1))
    assert not set(a) & set(b) and sorted(a + b) == list(range(24))


def test_aug_draws_are_reproducible_and_differ_between_epochs():
    from lgteun_amd.resident import ResidentLoader
    mk = lambda seed=3: ResidentLoader(_Sized(640), 4, shuffle=True, seed=seed, aug_dict=dict(ud_flip=0.5, lr_flip=0.5))  # noqa: E731
    a, b = mk(), mk()
    assert a.aug_draws(0) == b.aug_draws(0) and a.aug_draws(7) == b.aug_draws(7)
    assert len(a.aug_draws(0)) == len(a) == 160 and all(list(d) == ['ud_flip', 'lr_flip'] for d in a.aug_draws(0))
    assert a.aug_draws(0) != a.aug_draws(1) and a.aug_draws(0) != mk(4).aug_draws(0)
    outcomes = {(d['ud_flip'], d['lr_flip']) for d in a.aug_draws(0)}
    assert outcomes == {(False, False), (False, True), (True, False), (True, True)}
    # every selected transform applies to the original and the last one wins: both drawn = left-right only
    word = {(False, False): 0, (True, False): a.FLIP_UD, (False, True): a.FLIP_LR, (True, True): a.FLIP_LR}
    assert a.flip_words(0) == [word[(d['ud_flip'], d['lr_flip'])] for d in a.aug_draws(0)]
    assert mk().aug_dict == dict(ud_flip=0.5, lr_flip=0.5)                     # the caller's probabilities are not overwritten
    assert ResidentLoader(_Sized(8), 4).aug_draws(0) == []
    forced = ResidentLoader(_Sized(8), 4, aug_dict=dict(ud_flip=1.0, lr_flip=0.0))
    assert forced.aug_draws(2) == [dict(ud_flip=True, lr_flip=False)] * 2
    forced.aug_draws = lambda epoch: [dict(ud_flip=True, lr_flip=True), dict(ud_flip=False, lr_flip=False)]      # the hook
    assert forced.flip_words(0) == [forced.FLIP_LR, 0]


def test_crop_keys_and_bad_arguments_raise():
    from lgteun_amd.resident import ResidentLoader
    for key in ('r4_crop', 'r2_crop'):
        with pytest.raises(ValueError, match='data_augmentation'):
            ResidentLoader(_Sized(8), 4, aug_dict={'ud_flip': 0.5, key: 0.5})
    with pytest.raises(ValueError, match='unknown augmentation'):
        ResidentLoader(_Sized(8), 4, aug_dict={'rot90': 0.5})
    with pytest.raises(ValueError, match='bit_depth'):
        ResidentLoader(_Sized(8), 4, fold_normalize=True)
    with pytest.raises(ValueError, match='batch_size'):
        ResidentLoader(_Sized(8), 0)
    with pytest.raises(TypeError, match='ResidentStore'):
        next(iter(ResidentLoader(_Sized(8), 4)))


def test_mixed_shapes_and_max_bytes_raise(tmp_path):
    from lgteun_amd.resident import ResidentStore, pack_host
    d = write_set(tmp_path / 'mixed', 5, 4, 32, 32)
    write_tiff(os.path.join(d, 'im0003_pan.tif'), np.zeros((36, 32), np.uint16))
    write_tiff(os.path.join(d, 'im0004_lr.tif'), np.zeros((8, 8, 3), np.uint16))
    with pytest.raises(ValueError, match=r'im0003_pan\.tif.*host loader'):
        pack_host(PSDataset([d], 11))
    with pytest.raises(ValueError, match=r'im0003_pan\.tif.*host loader'):
        pack_host(PSDataset([d], 11), threads=1)
    d = write_set(tmp_path / 'types', 3, 4, 32, 32)
    write_tiff(os.path.join(d, 'im0001_lr.tif'), np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError, match=r'im0001_lr\.tif.*host loader'):
        pack_host(PSDataset([d], 11))
    d = write_set(tmp_path / 'partial', 3, 4, 32, 32)
    os.remove(os.path.join(d, 'im0002_mul.tif'))
    with pytest.raises(ValueError, match=r'im0002_mul\.tif.*host loader'):
        pack_host(PSDataset([d], 11))
    d = write_set(tmp_path / 'ratio', 2, 4, 32, 32)
    write_tiff(os.path.join(d, 'im0000_lr.tif'), np.zeros((16, 16, 4), np.uint16))
    with pytest.raises(ValueError, match=r'im0000_pan\.tif.*host loader'):
        pack_host(PSDataset([d], 11))
    d = write_set(tmp_path / 'big', 4, 4, 32, 32)
    need = pack_host(PSDataset([d], 11)).nbytes
    assert need == 4 * ((32 * 32 + 4 * 8 * 8 + 4 * 32 * 32) * 2 + 8 * 8 * 4)
    assert pack_host(PSDataset([d], 11), max_bytes=need).nbytes == need
    with pytest.raises(ValueError, match=r'above the cap.*host loader'):
        pack_host(PSDataset([d], 11), max_bytes=need - 1)
    with pytest.raises(ValueError, match=r'above the cap.*host loader'):
        ResidentStore.from_dataset(PSDataset([d], 11), 'cuda:0', max_bytes=need - 1)       # rejected before the device is touched
    with pytest.raises(ValueError, match='GPU'):
        ResidentStore.from_dataset(PSDataset([d], 11), 'cpu')
    os.makedirs(tmp_path / 'empty')
    with pytest.raises(ValueError, match='empty'):
        pack_host(PSDataset([str(tmp_path / 'empty')], 11))


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'float32', 'int16'])
@pytest.mark.parametrize('with_mul', [True, False])
def test_host_packing_equals_the_files(tmp_path, dtype, with_mul):
    from lgteun_amd.resident import pack_host
    if dtype == 'int16':                       # a sample type the store does not keep: converted like PSDataset does (float64, then float32)
        d = str(tmp_path / 'set')
        os.makedirs(d)
        rng = np.random.default_rng(1)
        for i in range(3):
            write_tiff(os.path.join(d, f'im{i}_pan.tif'), rng.integers(-2000, 2000, (16, 24)).astype(np.int16))
            write_tiff(os.path.join(d, f'im{i}_lr.tif'), rng.integers(-2000, 2000, (4, 6, 4)).astype(np.int16))
            if with_mul:
                write_tiff(os.path.join(d, f'im{i}_mul.tif'), rng.integers(-2000, 2000, (16, 24, 4)).astype(np.int16))
        want_kind, n, C, H, W = 'float32', 3, 4, 16, 24
    else:
        n, C, H, W = 7, 4, 16, 24
        d = write_set(tmp_path / 'set', n, C, H, W, dtype=dtype, with_mul=with_mul, seed=2)
        want_kind = dtype
    ds = PSDataset([d], 11)
    for threads in (1, 16):
        pack = pack_host(ds, threads=threads)
        assert len(pack) == n and pack.image_ids == ds.image_ids
        assert pack.pan.shape == (n, 1, H, W) and pack.lr.shape == (n, C, H // 4, W // 4) and pack.pan.dtype.name == pack.lr.dtype.name == want_kind
        assert (pack.mul is not None) == with_mul and all(a.flags['C_CONTIGUOUS'] for a in (pack.pan, pack.lr))
        for i, prefix in enumerate(ds.image_prefix_names):
            item = ds[i]                          # the host path's item: float32 of the same numbers
            assert np.array_equal(pack.pan[i, 0], read_tiff(f'{prefix}_pan.tif'))
            assert np.array_equal(pack.lr[i], read_tiff(f'{prefix}_lr.tif').transpose(2, 0, 1))
            assert np.array_equal(pack.pan[i].astype(np.float32), item['input_pan'].numpy())
            assert np.array_equal(pack.lr[i].astype(np.float32), item['input_lr'].numpy())
            assert ('target' in item) == with_mul
            if with_mul:
                assert pack.mul.shape == (n, C, H, W) and pack.mul.dtype.name == want_kind
                assert np.array_equal(pack.mul[i].astype(np.float32), item['target'].numpy())


def test_two_directories_have_no_target(tmp_path):
    """PSDataset yields `target` for a single directory only; the store follows"""
    from lgteun_amd.resident import pack_host
    a = write_set(tmp_path / 'a', 2, 4, 16, 16)
    b = write_set(tmp_path / 'b', 3, 4, 16, 16, seed=1)
    pack = pack_host(PSDataset([a, b], 11))
    assert pack.mul is None and len(pack) == 5


def test_build_loader_without_the_flag_is_unchanged(tmp_path):
    import torch.utils.data as data
    from lgteun_amd.dataset import build_loader
    d = write_set(tmp_path / 'set', 3, 4, 16, 16)
    cfg = dict(dataset=dict(type='PSDataset', image_dirs=[d], bit_depth=11), batch_size=2, num_workers=0, shuffle=False)
    loader, sampler = build_loader(cfg)
    assert isinstance(loader, data.DataLoader) and sampler is None
    loader, sampler = build_loader(dict(cfg, resident=False))
    assert isinstance(loader, data.DataLoader) and sampler is None
    with pytest.raises(ValueError, match='device'):
        build_loader(cfg, resident=True)
    with pytest.raises(ValueError, match='device'):
        build_loader(dict(cfg, resident=True))


def test_runner_skips_data_normalize_for_marked_batches_only(tmp_path):
    import torch
    from lgteun_amd.base_model import Base_model, NormalizedBatch
    from lgteun_amd.compat import Config
    cfg = Config(dict(work_dir=str(tmp_path), datas='GF-2', bit_depth=11, max_iter=2, loss_cfg={'rec_loss': dict(type='l1', w=1.)}))
    x = torch.full((1, 1, 2, 2), 2047.5)
    plain, marked = dict(input_pan=x, image_id=['a']), NormalizedBatch(input_pan=x, image_id=['a'])
    assert marked.normalized is True and isinstance(marked, dict)
    runner = Base_model(cfg, None, [plain, marked], None, None)
    got = [b['input_pan'] for _, b in runner._train_batches(torch.device('cpu'))]
    assert torch.equal(got[0], torch.ones(1, 1, 2, 2)) and torch.equal(got[1], x)
