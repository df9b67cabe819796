"""Device-resident dataset: the whole `PSDataset` decoded once and kept on the GPU in the files' sample type, and a loader whose
training batch is ONE gather kernel (lgteun_amd/csrc/k_batch.hip; C ABI lg_pyr_down2 / lg_batch_assemble in include/lgteun_hip.h).

The host path (`DataLoader(PSDataset)`, dataset.py) decodes three TIFFs and runs two scipy pyramids per item: about 2 ms of one core,
a few hundred items per second and core, against the thousands of pairs per second one GPU trains at.  The data sets of this task are
small (168 KB per pair as uint16 at C = 4, PAN 128 x 128), so they fit the card many times over:

    store = ResidentStore.from_dataset(PSDataset([...], bit_depth=11), 'cuda:0')
    loader = ResidentLoader(store, batch_size=32, shuffle=True, fold_normalize=True, bit_depth=11)
    for batch in loader: ...           # dicts with the DataLoader(PSDataset) keys and shapes, tensors on the device

Batches are bit-identical to the host path's: the integers are converted to fp32 and divided with correctly rounded fp32 divisions where
`PSDataset(norm_input=True)` divides on the host, and `input_pan_l` -- two levels of the 5 x 5 binomial pyramid -- is exact for integer
images (every intermediate is a multiple of 2^-16 below 2^16), so the device's integer arithmetic and the host's float64 give the same
fp32 value.  There is no fallback: without the built library (or without a GPU) the store cannot be built."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .base_model import NormalizedBatch
from .dataset import ShardedSampler, read_tiff
from .engine import _stream_ptr

MAX_THREADS = 16
FREE_MEMORY_SHARE = 0.8        # default cap of a store: this share of the device memory that is free when it is built
_HOST = 'use the host loader (dataset.build_loader without resident=True) for such a set'
_KINDS = {'uint8': _lib.LG_DT_U8, 'uint16': _lib.LG_DT_U16, 'float32': _lib.LG_DT_F32}


def _ptr(t):
    """device pointer of a tensor; NULL for an array the store does not hold (`mul`)"""
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _storage(a, kind):
    """a decoded file in the store's sample type: uint8 / uint16 as they are, everything else through float64 to float32 like PSDataset"""
    if a.dtype.name == kind:
        return a
    if kind == 'float32':
        return np.asarray(a, dtype=np.double).astype(np.float32)
    return None


def _chw(a):
    return (a[np.newaxis] if a.ndim == 2 else a.transpose(2, 0, 1))


class HostPack:
    """the packed set on the host: pan [N,1,H,W], lr [N,C,h,w], mul [N,C,H,W] or None (contiguous numpy arrays of one sample type)"""

    def __init__(self, pan, lr, mul, image_ids):
        self.pan, self.lr, self.mul, self.image_ids = pan, lr, mul, list(image_ids)

    def __len__(self):
        return len(self.image_ids)

    @property
    def nbytes(self):
        """bytes of the store this becomes: the arrays plus the fp32 pan_l [N,1,h,w]"""
        n, _, h, w = self.lr.shape
        return self.pan.nbytes + self.lr.nbytes + (self.mul.nbytes if self.mul is not None else 0) + 4 * n * h * w


def pack_host(ps_dataset, max_bytes=None, threads=MAX_THREADS):
    """Decode every triplet of `ps_dataset` once (dataset.read_tiff, a pool of at most 16 THREADS -- no worker processes, so this is safe
    in a process that has initialised the GPU) into contiguous arrays.  uint8 and uint16 sets keep their sample type; every other type is
    converted like PSDataset converts it (float64, then float32).  `mul` is packed when the dataset would yield `target`.
    ValueError: an empty set, items that differ in shape or sample type (names the first offending file), a set above `max_bytes`."""
    prefixes = list(ps_dataset.image_prefix_names)
    n = len(prefixes)
    if n == 0:
        raise ValueError('the dataset is empty: nothing to keep resident')
    with_mul = len(ps_dataset.image_dirs) == 1 and os.path.exists(f'{prefixes[0]}_mul.tif')
    names = ('pan', 'lr') + (('mul',) if with_mul else ())

    def decode(i):
        return {k: read_tiff(f'{prefixes[i]}_{k}.tif') for k in names}
    first = decode(0)
    kinds = {a.dtype.name for a in first.values()}
    kind = kinds.pop() if len(kinds) == 1 and kinds <= {'uint8', 'uint16'} else 'float32'
    shapes = {k: _chw(a).shape for k, a in first.items()}
    (_, H, W), (C, h, w) = shapes['pan'], shapes['lr']
    if shapes['pan'][0] != 1 or (H, W) != (4 * h, 4 * w) or (with_mul and shapes['mul'] != (C, H, W)):
        raise ValueError(f'{prefixes[0]}_pan.tif: PAN {shapes["pan"]}, LR MS {shapes["lr"]}' + (f', MS {shapes["mul"]}' if with_mul else '') +
                         f' are not [1,4h,4w] / [C,h,w] / [C,4h,4w]; {_HOST}')
    item = np.dtype(kind).itemsize
    need = n * ((H * W + C * h * w + (C * H * W if with_mul else 0)) * item + 4 * h * w)
    if max_bytes is not None and need > max_bytes:
        raise ValueError(f'{prefixes[0]}_pan.tif: {n} items of this shape need {need} bytes resident, above the cap of {int(max_bytes)}; {_HOST}')
    out = {k: np.empty((n,) + shapes[k], dtype=kind) for k in names}

    def work(i):
        """-> None, or the file that does not fit the set"""
        if with_mul is not (len(ps_dataset.image_dirs) == 1 and os.path.exists(f'{prefixes[i]}_mul.tif')):
            return f'{prefixes[i]}_mul.tif (present for some items only)'
        got = first if i == 0 else decode(i)
        for k in names:
            a = _storage(_chw(got[k]), kind)
            if a is None or a.shape != shapes[k]:
                return f'{prefixes[i]}_{k}.tif ({got[k].dtype} {_chw(got[k]).shape}, the set holds {kind} {shapes[k]})'
            out[k][i] = a
        return None
    pool = ThreadPoolExecutor(max_workers=max(1, min(MAX_THREADS, int(threads))))
    try:
        for bad in pool.map(work, range(n)):          # in item order: the FIRST offending file is reported
            if bad is not None:
                raise ValueError(f'{bad}: the items of a resident set must agree in shape and sample type; {_HOST}')
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    return HostPack(out['pan'], out['lr'], out.get('mul'), ps_dataset.image_ids)


class ResidentStore:
    """The set on one device: `pan`, `lr`, `mul` (or None) in the files' sample type and `pan_l` [N,1,H/4,W/4] fp32, computed once on
    the device by k_pyr_down2 over all N planes.  uint16 arrays are held as int16 tensors (the same bits; only the kernels read them).
    `len(store)`, `store.nbytes` and `store.image_ids` live on the host."""

    def __init__(self, pack, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError(f'a resident store lives on a GPU (got device {device})')
        self.device = device
        self.image_ids = list(pack.image_ids)
        self.kind = pack.pan.dtype.name
        self.dtype_code = _KINDS[self.kind]
        self.n, self.C, self.h, self.w = pack.lr.shape
        self.H, self.W = pack.pan.shape[2:]

        def up(a):
            return None if a is None else torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)
        self.pan, self.lr, self.mul = up(pack.pan), up(pack.lr), up(pack.mul)
        self.pan_l = torch.empty(self.n, 1, self.h, self.w, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            _lib.check(_lib.lib().lg_pyr_down2(_ptr(self.pan), _ptr(self.pan_l), self.n, self.H, self.W, self.dtype_code, _stream_ptr()),
                       'lg_pyr_down2')
        self.nbytes = sum(t.numel() * t.element_size() for t in (self.pan, self.lr, self.mul, self.pan_l) if t is not None)

    @classmethod
    def from_dataset(cls, ps_dataset, device, max_bytes=None, threads=MAX_THREADS):
        """Decode `ps_dataset` (pack_host) and put it on `device`.  max_bytes: the largest store accepted; the default is 80 % of the
        device memory that is free at the time of the call (FREE_MEMORY_SHARE).  A larger set, or one whose items differ in shape, is
        a ValueError that points to the host loader."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise ValueError(f'a resident store lives on a GPU (got device {device})')
        _lib.lib()                              # a missing library is an error before anything is decoded
        if max_bytes is None:
            max_bytes = int(FREE_MEMORY_SHARE * torch.cuda.mem_get_info(device)[0])
        return cls(pack_host(ps_dataset, max_bytes=max_bytes, threads=threads), device)

    def __len__(self):
        return self.n


class ResidentLoader:
    """Iterates a ResidentStore in batches: dicts with the keys and shapes `DataLoader(PSDataset)` collates (`input_lr`, `input_pan`,
    `target` when stored, `input_pan_l`, and `image_id` as a list of str), fresh fp32 tensors on the store's device, one kernel launch and
    no host synchronisation per batch -- the epoch's index list and flip words are uploaded once, when the epoch starts.

    Order: every epoch's order is `ShardedSampler(len(store), rank, world, shuffle, seed, drop_last, pad=not evaluation)`'s at that epoch
    (`loader.sampler`), also for world == 1 -- where the host path's DataLoader shuffles with torch's global generator instead.  Every
    rank keeps the whole set resident: the permutation is global.  `__iter__` starts a new epoch by itself: the epoch counter advances
    after each complete pass, so `for batch in loader` reshuffles without help; `set_epoch(e)` overrides it (a resume).
    Contents: raw digital numbers as fp32, divided by 2**bit_depth - 0.5 if `norm_input` (what PSDataset(norm_input=True) yields).
    fold_normalize=True also applies the runner's unconditional `data_normalize` in the kernel -- as a second operation with the device's
    own arithmetic, so the bits equal the two-step path -- and marks the batch (base_model.NormalizedBatch), which makes
    `Base_model._train_batches` / `test` skip theirs.
    aug_dict: {'ud_flip': p, 'lr_flip': p} only (the keys the reference's configs use; the crops need dataset.data_augmentation on the
    host path).  One draw per key and BATCH, in the dict's order, from a host generator seeded by (seed, epoch); the effect is
    data_augmentation's, including "the last selected transform wins": both drawn means left-right only.  `aug_draws(epoch)` returns the
    epoch's draws; it is also the hook: an instance attribute of that name replaces the generator."""
    FLIP_UD, FLIP_LR = 1, 2

    def __init__(self, store, batch_size, shuffle=False, rank=0, world=1, seed=0, drop_last=False, evaluation=False, aug_dict=None,
                 fold_normalize=False, bit_depth=None, norm_input=False):
        if int(batch_size) < 1:
            raise ValueError(f'batch_size must be positive (got {batch_size})')
        if aug_dict is not None:
            crops = [k for k in aug_dict if k in ('r4_crop', 'r2_crop')]
            if crops:
                raise ValueError(f'{crops}: crop-resize augmentation does not run on the device; use dataset.data_augmentation on the host path')
            unknown = [k for k in aug_dict if k not in ('ud_flip', 'lr_flip')]
            if unknown:
                raise ValueError(f'unknown augmentation keys {unknown} (ud_flip and lr_flip are supported)')
        if (norm_input or fold_normalize) and bit_depth is None:
            raise ValueError('norm_input / fold_normalize need bit_depth')
        self.store, self.batch_size, self.drop_last = store, int(batch_size), bool(drop_last)
        self.sampler = ShardedSampler(len(store), rank, world, shuffle=bool(shuffle), seed=seed, drop_last=bool(drop_last), pad=not evaluation)
        self.seed, self.epoch = int(seed), 0
        self.aug_dict = dict(aug_dict) if aug_dict is not None else None
        self.fold_normalize, self.norm_input, self.bit_depth = bool(fold_normalize), bool(norm_input), bit_depth
        self.divisor = float(2 ** bit_depth - .5) if bit_depth is not None else 1.0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self.sampler.set_epoch(self.epoch)

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def epoch_order(self, epoch=None):
        """this rank's store indices of `epoch` (default: the one the next pass runs), in the order they are consumed"""
        keep = self.sampler.epoch
        self.sampler.set_epoch(self.epoch if epoch is None else int(epoch))
        order = [int(i) for i in self.sampler]
        self.sampler.set_epoch(keep)
        return order

    def aug_draws(self, epoch):
        """the booleans of `epoch`: one {key: bool} per batch, keys in aug_dict's order ([] without aug_dict)"""
        if self.aug_dict is None:
            return []
        rng = np.random.default_rng([self.seed, int(epoch)])
        return [{k: bool(rng.random() < p) for k, p in self.aug_dict.items()} for _ in range(len(self))]

    def flip_words(self, epoch):
        """per batch: what the drawn transforms amount to (every one applies to the original, the last one wins)"""
        return [(self.FLIP_LR if d.get('lr_flip') else (self.FLIP_UD if d.get('ud_flip') else 0)) for d in self.aug_draws(epoch)]

    def _scaling(self):
        """(n_div, post_scale) of lg_batch_assemble.  PSDataset(norm_input=True) divides on the HOST: a correctly rounded fp32 division.
        The runner's data_normalize divides a DEVICE tensor by a Python scalar, which torch computes as a multiplication by the fp32
        reciprocal: folding it in has to do the same to give the same bits."""
        post = float(np.float32(1.0) / np.float32(self.divisor)) if self.fold_normalize else 1.0
        return (1 if self.norm_input else 0), post

    def __iter__(self):
        if not isinstance(self.store, ResidentStore):
            raise TypeError(f'batches come from a ResidentStore on a GPU (got {type(self.store).__name__}: order and draws only)')
        st, L = self.store, _lib.lib()
        epoch = self.epoch
        self.sampler.set_epoch(epoch)
        order = [int(i) for i in self.sampler]
        nb = len(self)
        words = self.flip_words(epoch) if self.aug_dict is not None else None
        if words is not None and len(words) != nb:
            raise ValueError(f'aug_draws({epoch}) returned {len(words)} draws for {nb} batches')
        dev = st.device
        idx = torch.tensor(order, dtype=torch.int32).to(dev)                       # the epoch's ONE upload (two with flips)
        flips = torch.tensor(words, dtype=torch.int32).to(dev) if words else None
        n_div, post = self._scaling()
        cls = NormalizedBatch if self.fold_normalize else dict
        B0, C, H, W, h, w = self.batch_size, st.C, st.H, st.W, st.h, st.w
        for bi in range(nb):
            ids = order[bi * B0:(bi + 1) * B0]
            B = len(ids)
            with torch.cuda.device(dev):
                o_lr = torch.empty(B, C, h, w, dtype=torch.float32, device=dev)
                o_pan = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
                o_mul = torch.empty(B, C, H, W, dtype=torch.float32, device=dev) if st.mul is not None else None
                o_pl = torch.empty(B, 1, h, w, dtype=torch.float32, device=dev)
                fp = ctypes.c_void_p(flips.data_ptr() + 4 * bi) if flips is not None else ctypes.c_void_p(0)
                _lib.check(L.lg_batch_assemble(_ptr(st.pan), _ptr(st.lr), _ptr(st.mul), _ptr(st.pan_l), st.n, _ptr(idx), bi * B0, fp,
                                               _ptr(o_pan), _ptr(o_lr), _ptr(o_mul), _ptr(o_pl), B, C, H, W, h, w, st.dtype_code,
                                               self.divisor, n_div, post, _stream_ptr()), 'lg_batch_assemble')
            batch = cls(input_lr=o_lr, input_pan=o_pan)
            if o_mul is not None:
                batch['target'] = o_mul
            batch['input_pan_l'] = o_pl
            batch['image_id'] = [st.image_ids[i] for i in ids]
            yield batch
        if self.epoch == epoch:                 # a complete pass, and nobody called set_epoch meanwhile: the next pass is the next epoch
            self.set_epoch(epoch + 1)
