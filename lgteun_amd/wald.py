"""Training from a raw scene: Wald's protocol and window batches on the GPU, with nothing on disk.

The reference's data sets were cut from one raw scene per sensor "following Wald's protocol" with the tools of another project: low-pass
and decimate MS and PAN by 4, keep the raw MS as the target, cut overlapping patches, write three TIFFs per patch.  Here the scene stays
on the device as ONE image in its sample type, and a batch is cut out of it by an origin list:

    store = SceneStore.from_scene(ms_u16, pan_u16, 'cuda:0', gains_ms=(0.3, 0.25, 0.2, 0.35), gain_pan=0.15)     # lg_fir_decimate4
    loader = SceneLoader(store, patch=128, step=32, batch_size=32, shuffle=True, fold_normalize=True, bit_depth=11)
    for batch in loader: ...            # the ResidentLoader's dicts; two launches per batch (lg_window_assemble)

Batches are bit for bit what ResidentLoader yields for a store that holds the same windows as items.  mode='random' draws fresh windows
every epoch, which a fixed patch set cannot do.  `export_triplets` writes the windows as the files PSDataset reads.

MTF gains.  The low-pass is a Gaussian whose response at the decimated grid's Nyquist frequency equals the sensor's MTF gain there.  Gains
are per band and per sensor and are the CALLER's: without them the defaults DEFAULT_GAIN_MS = 0.3 and DEFAULT_GAIN_PAN = 0.15 apply, which
are common placeholders and NOT a sensor's measured values.

The geometry (mtf_taps, window_origins, random_origins, the loader's order and draws) is pure Python: it imports and runs without a GPU and
without the built library.  Kernels: lgteun_amd/csrc/k_wald.hip, k_batch.hip; contracts: include/lgteun_hip.h."""
import ctypes
import os

import numpy as np

from .resident import ResidentLoader

DEFAULT_GAIN_MS, DEFAULT_GAIN_PAN = 0.3, 0.15
DEFAULT_TAPS = 41
_KINDS = ('uint8', 'uint16', 'float32')


# ------------------------------------------------------------------------------------------------
# geometry (no GPU)
# ------------------------------------------------------------------------------------------------
def mtf_taps(gain, n_taps=DEFAULT_TAPS, ratio=4):
    """fp64 Gaussian taps [n_taps], normalised to sum 1, with sigma = ratio * sqrt(-2 ln gain) / pi: the response at the decimated grid's
    Nyquist frequency, 1 / (2 ratio) cycles per pixel, is `gain`.  gain in (0, 1); n_taps odd in 1 .. 63 (the kernel's limit)."""
    gain = float(gain)
    if not 0.0 < gain < 1.0:
        raise ValueError(f'gain {gain}: an MTF gain at Nyquist lies strictly between 0 and 1')
    if int(n_taps) != n_taps or n_taps < 1 or n_taps > 63 or n_taps % 2 == 0:
        raise ValueError(f'n_taps {n_taps}: the tap count must be odd, in 1 .. 63')
    if int(ratio) != ratio or ratio < 1:
        raise ValueError(f'ratio {ratio}: must be a positive integer')
    sigma = ratio * np.sqrt(-2.0 * np.log(gain)) / np.pi
    x = np.arange(int(n_taps), dtype=np.float64) - int(n_taps) // 2
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return t / t.sum()


def _check_phase(phase):
    if int(phase) != phase or not 0 <= phase <= 3:
        raise ValueError(f'phase {phase}: the decimation phase must be 0, 1, 2 or 3')
    return int(phase)


def _check_region(Hs, Ws, patch, region):
    """-> (y0, x0, y1, x1, P, Q); ValueError says what to change"""
    P, Q = (patch, patch) if np.isscalar(patch) else tuple(patch)
    for name, L in (('height', Hs), ('width', Ws)):
        if int(L) != L or L < 8 or L % 4:
            raise ValueError(f'scene {name} {L}: PAN sides must be multiples of 4 (4 x the MS side) and at least 8; crop the scene')
    y0, x0, y1, x1 = (0, 0, Hs, Ws) if region is None else tuple(region)
    for name, v in (('y0', y0), ('x0', x0), ('y1', y1), ('x1', x1)):
        if int(v) != v or v % 4:
            raise ValueError(f'region {name} = {v}: region bounds are PAN pixels on the 4-pixel grid (an MS pixel is 4 PAN pixels); '
                             f'use {int(v) // 4 * 4} or {int(v) // 4 * 4 + 4}')
    if not (0 <= y0 < y1 <= Hs and 0 <= x0 < x1 <= Ws):
        raise ValueError(f'region {(y0, x0, y1, x1)} does not lie inside the scene of {Hs} x {Ws} as (y0, x0, y1, x1)')
    for name, t, L in (('height', P, y1 - y0), ('width', Q, x1 - x0)):
        if int(t) != t or t < 8 or t % 4:
            raise ValueError(f'patch {name} {t}: must be a multiple of 4, at least 8')
        if t > L:
            raise ValueError(f'patch {name} {t} exceeds the region {name} {L}: choose a smaller patch or a larger region')
    return int(y0), int(x0), int(y1), int(x1), int(P), int(Q)


def window_origins(Hs, Ws, patch, step, region=None):
    """The grid of windows: int32 [n, 2] of (oy, ox) in PAN pixels, row-major; per axis the origins 0, step, 2 step, ... (from the region's
    corner) whose window still fits.  patch: int or (P, Q); step and region = (y0, x0, y1, x1) on the 4-pixel grid.  The reference keeps
    the training and the testing part of one scene apart with two regions."""
    y0, x0, y1, x1, P, Q = _check_region(Hs, Ws, patch, region)
    if int(step) != step or step < 4 or step % 4:
        raise ValueError(f'step {step}: must be a positive multiple of 4 (an MS pixel is 4 PAN pixels); use {max(4, int(step) // 4 * 4)}')
    ys, xs = np.arange(y0, y1 - P + 1, int(step)), np.arange(x0, x1 - Q + 1, int(step))
    return np.stack(np.meshgrid(ys, xs, indexing='ij'), axis=-1).reshape(-1, 2).astype(np.int32)


def random_origins(Hs, Ws, patch, n, seed, epoch, region=None):
    """n origins of `epoch`: int32 [n, 2], uniform on the 4-pixel grid inside the region, from np.random.default_rng([seed, epoch])"""
    y0, x0, y1, x1, P, Q = _check_region(Hs, Ws, patch, region)
    if int(n) != n or n < 1:
        raise ValueError(f'windows_per_epoch {n}: must be a positive integer')
    rng = np.random.default_rng([int(seed), int(epoch)])
    oy = y0 + 4 * rng.integers(0, (y1 - y0 - P) // 4 + 1, size=int(n))
    ox = x0 + 4 * rng.integers(0, (x1 - x0 - Q) // 4 + 1, size=int(n))
    return np.stack([oy, ox], axis=-1).astype(np.int32)


def window_id(oy, ox):
    """the image_id of a window: sorts like the row-major grid, and holds no '_' (PSDataset cuts ids there)"""
    return f'y{int(oy):05d}x{int(ox):05d}'


class SceneShape:
    """the PAN-grid size of a scene a loader cuts windows from; all a SceneLoader needs for its order, origins and draws (no GPU)"""

    def __init__(self, Hs, Ws):
        self.Hs, self.Ws = int(Hs), int(Ws)


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def _scene_arrays(ms, pan):
    """-> (ms [C,h,w], pan [1,4h,4w]) as contiguous numpy arrays of one supported sample type"""
    ms, pan = np.ascontiguousarray(ms), np.ascontiguousarray(pan)
    if pan.ndim == 2:
        pan = pan[np.newaxis]
    if ms.dtype != pan.dtype or ms.dtype.name not in _KINDS:
        raise ValueError(f'ms ({ms.dtype}) and pan ({pan.dtype}) must share one sample type out of uint8, uint16, float32 '
                         '(convert float64 with .astype(np.float32))')
    if ms.ndim != 3 or pan.ndim != 3 or pan.shape[0] != 1 or pan.shape[1:] != (4 * ms.shape[1], 4 * ms.shape[2]):
        raise ValueError(f'expected MS [C,h,w] and PAN [1,4h,4w], got {ms.shape} / {pan.shape}')
    return ms, pan


def _up(a, device):
    """uint16 is held as its int16 view (the same bits; only the kernels read it), like the resident store"""
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _as_numpy(t, kind):
    a = t.cpu().numpy()
    return a.view(np.uint16) if kind == 'uint16' else a


def _cuda(device):
    import torch
    device = torch.device(device)
    if device.type != 'cuda':
        raise ValueError(f'a scene store lives on a GPU (got device {device})')
    return device


def _fir(x, taps, phase, kind):
    """lg_fir_decimate4 of the device planes x [n,H,W] with the fp64 taps [n,n_taps] -> [n,H/4,W/4] in x's sample type"""
    import torch

    from . import _lib
    from .engine import _stream_ptr
    n, H, W = x.shape
    out = torch.empty(n, H // 4, W // 4, dtype=x.dtype, device=x.device)
    t = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float64)).to(x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().lg_fir_decimate4(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(t.data_ptr()), n, H, W,
                                               t.shape[1], phase, _lib_code(kind), 1 if kind == 'float32' else 0, _stream_ptr()), 'lg_fir_decimate4')
    return out


def _lib_code(kind):
    from . import _lib
    return {'uint8': _lib.LG_DT_U8, 'uint16': _lib.LG_DT_U16, 'float32': _lib.LG_DT_F32}[kind]


def _gain_rows(gains, C, default, what):
    gains = [default] * C if gains is None else ([float(gains)] * C if np.isscalar(gains) else [float(g) for g in gains])
    if len(gains) != C:
        raise ValueError(f'{what}: {len(gains)} gains for {C} bands')
    return gains


def _degrade_device(ms_t, pan_t, kind, gains_ms, gain_pan, phase, n_taps):
    C = ms_t.shape[0]
    phase = _check_phase(phase)
    t_ms = np.stack([mtf_taps(g, n_taps) for g in _gain_rows(gains_ms, C, DEFAULT_GAIN_MS, 'gains_ms')])
    t_pan = mtf_taps(DEFAULT_GAIN_PAN if gain_pan is None else gain_pan, n_taps)[np.newaxis]
    return _fir(ms_t, t_ms, phase, kind), _fir(pan_t, t_pan, phase, kind)


def degrade_scene(ms, pan, gains_ms=None, gain_pan=None, phase=2, device='cuda:0', n_taps=DEFAULT_TAPS):
    """Wald's protocol on the device: raw MS [C,hs,ws] and raw PAN [1,4hs,4ws] (numpy; uint8, uint16 or float32; hs, ws multiples of 4) ->
    (lr [C,hs/4,ws/4], pan_lr [1,hs,ws]) as numpy arrays of the input's sample type.  The raw MS is the target of the degraded pair.
    Each plane is filtered with mtf_taps of its gain (gains_ms: one per band or one for all; defaults DEFAULT_GAIN_MS / DEFAULT_GAIN_PAN,
    which are no sensor's measured values) and sampled at (4 i + phase, 4 j + phase); integer types round half to even and saturate."""
    ms, pan = _scene_arrays(ms, pan)
    device = _cuda(device)
    lr, pan_lr = _degrade_device(_up(ms, device), _up(pan, device), ms.dtype.name, gains_ms, gain_pan, phase, n_taps)
    return _as_numpy(lr, ms.dtype.name), _as_numpy(pan_lr, ms.dtype.name)


class SceneStore(SceneShape):
    """One scene on one device in its sample type: pan [1,Hs,Ws], lr [C,Hs/4,Ws/4] and mul [C,Hs,Ws] or None -- what windows are cut
    from.  uint16 arrays are held as int16 tensors.  `SceneStore(pan, lr, mul, device)` takes a finished (already degraded) scene as numpy
    arrays; `from_scene` starts from the raw pair."""

    def __init__(self, pan, lr, mul, device, _tensors=None):
        device = _cuda(device)
        if _tensors is None:
            lr, pan = _scene_arrays(lr, pan)
            if mul is not None:
                mul = np.ascontiguousarray(mul)
                if mul.dtype != pan.dtype or mul.shape != (lr.shape[0],) + pan.shape[1:]:
                    raise ValueError(f'mul {mul.dtype} {mul.shape}: expected {pan.dtype} {(lr.shape[0],) + pan.shape[1:]}')
            self.kind = pan.dtype.name
            self.pan, self.lr, self.mul = _up(pan, device), _up(lr, device), (None if mul is None else _up(mul, device))
        else:
            self.kind, self.pan, self.lr, self.mul = _tensors
        self.device = device
        self.dtype_code = _lib_code(self.kind)
        self.C = int(self.lr.shape[0])
        super().__init__(self.pan.shape[1], self.pan.shape[2])
        if self.Hs % 4 or self.Ws % 4 or self.Hs < 8 or self.Ws < 8:
            raise ValueError(f'scene of {self.Hs} x {self.Ws} PAN pixels: sides must be multiples of 4, at least 8; crop the scene')
        self.nbytes = sum(t.numel() * t.element_size() for t in (self.pan, self.lr, self.mul) if t is not None)

    @classmethod
    def from_scene(cls, ms, pan, device, degrade=True, gains_ms=None, gain_pan=None, phase=2, n_taps=DEFAULT_TAPS):
        """degrade=True: Wald's protocol (degrade_scene's arithmetic, everything stays on the device): the store is the degraded pair with
        the raw MS as `mul`, on the raw MS grid.  degrade=False: the raw full-resolution pair with no target, for no-reference evaluation."""
        from . import _lib
        ms, pan = _scene_arrays(ms, pan)
        device = _cuda(device)
        _lib.lib()                              # a missing library is an error before anything is uploaded
        kind = ms.dtype.name
        ms_t, pan_t = _up(ms, device), _up(pan, device)
        if not degrade:
            return cls(None, None, None, device, _tensors=(kind, pan_t, ms_t, None))
        if ms.shape[1] % 4 or ms.shape[2] % 4 or min(ms.shape[1:]) < 8:
            raise ValueError(f'raw MS of {ms.shape[1]} x {ms.shape[2]}: sides must be multiples of 4, at least 8, to be decimated by 4; crop the scene')
        lr, pan_lr = _degrade_device(ms_t, pan_t, kind, gains_ms, gain_pan, phase, n_taps)
        return cls(None, None, None, device, _tensors=(kind, pan_lr, lr, ms_t))

    def windows(self, origins, patch):
        """the windows at `origins` cut on the host: (pan [n,1,P,Q], lr [n,C,P/4,Q/4], mul [n,C,P,Q] or None) as numpy arrays"""
        P, Q = (patch, patch) if np.isscalar(patch) else tuple(patch)
        pan, lr = _as_numpy(self.pan, self.kind), _as_numpy(self.lr, self.kind)
        mul = None if self.mul is None else _as_numpy(self.mul, self.kind)
        org = np.asarray(origins).reshape(-1, 2)
        cut = lambda a, s: np.stack([a[:, y // s:(y + P) // s, x // s:(x + Q) // s] for y, x in org])      # noqa: E731
        return cut(pan, 1), cut(lr, 4), (None if mul is None else cut(mul, 1))


class SceneLoader(ResidentLoader):
    """Iterates windows of a SceneStore in batches with the ResidentLoader's surface: the same dict keys and shapes, `image_id`
    (window_id of the origin), `fold_normalize`, `norm_input`, `aug_dict` flips, `set_epoch`, and a ShardedSampler over the window list.
    Per batch: two launches (gather, window pyramid), no host synchronisation; the epoch's origin list and flip words are uploaded once.

    mode='grid': the fixed windows window_origins(Hs, Ws, patch, step, region) (or `origins`, an [n, 2] list of your own).
    mode='random': `windows_per_epoch` fresh windows every epoch, random_origins(..., seed, epoch): every rank draws the same list and
    takes its sampler's share of it.
    The batches are bit for bit those of ResidentLoader over a ResidentStore that holds the same windows as items; `input_pan_l` is the
    pyramid of the WINDOW (it reflects at the window's border, not the scene's)."""

    def __init__(self, store, patch, batch_size, step=None, mode='grid', windows_per_epoch=None, region=None, origins=None, shuffle=False, rank=0,
                 world=1, seed=0, drop_last=False, evaluation=False, aug_dict=None, fold_normalize=False, bit_depth=None, norm_input=False):
        if mode not in ('grid', 'random'):
            raise ValueError(f"mode must be 'grid' or 'random' (got {mode!r})")
        self.mode, self.region = mode, region
        _, _, _, _, self.P, self.Q = _check_region(store.Hs, store.Ws, patch, region)
        if mode == 'grid':
            if origins is None:
                if step is None:
                    raise ValueError("mode='grid' needs step (or origins)")
                origins = window_origins(store.Hs, store.Ws, patch, step, region)
            self.origins = np.ascontiguousarray(np.asarray(origins).reshape(-1, 2), dtype=np.int32)
            n = len(self.origins)
            if n == 0:
                raise ValueError('no window: the origin list is empty')
        else:
            if windows_per_epoch is None:
                raise ValueError("mode='random' needs windows_per_epoch")
            random_origins(store.Hs, store.Ws, patch, windows_per_epoch, seed, 0, region)         # the checks, before the first epoch
            self.origins, n = None, int(windows_per_epoch)
        super().__init__(range(n), batch_size, shuffle=shuffle, rank=rank, world=world, seed=seed, drop_last=drop_last, evaluation=evaluation,
                         aug_dict=aug_dict, fold_normalize=fold_normalize, bit_depth=bit_depth, norm_input=norm_input)      # range(n): the window list
        self.store = store

    def epoch_origins(self, epoch=None):
        """the window list of `epoch` (default: the one the next pass runs) as int32 [n, 2]; the sampler's indices point into it"""
        if self.mode == 'grid':
            return self.origins
        return random_origins(self.store.Hs, self.store.Ws, (self.P, self.Q), self.sampler.n, self.seed, self.epoch if epoch is None else epoch,
                              self.region)

    def __iter__(self):
        import torch

        from . import _lib
        from .base_model import NormalizedBatch
        from .engine import _stream_ptr
        if not isinstance(self.store, SceneStore):
            raise TypeError(f'batches come from a SceneStore on a GPU (got {type(self.store).__name__}: order, origins and draws only)')
        st, L = self.store, _lib.lib()
        epoch = self.epoch
        order = self.epoch_order(epoch)
        org = np.ascontiguousarray(self.epoch_origins(epoch)[order])                  # in the order they are consumed
        nb = len(self)
        words = self.flip_words(epoch) if self.aug_dict is not None else None
        if words is not None and len(words) != nb:
            raise ValueError(f'aug_draws({epoch}) returned {len(words)} draws for {nb} batches')
        dev = st.device
        d_org = torch.from_numpy(org).to(dev)                                          # the epoch's ONE upload (two with flips)
        flips = torch.tensor(words, dtype=torch.int32).to(dev) if words else None
        n_div, post = self._scaling()
        cls = NormalizedBatch if self.fold_normalize else dict
        B0, C, P, Q = self.batch_size, st.C, self.P, self.Q
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)          # noqa: E731
        for bi in range(nb):
            rows = org[bi * B0:(bi + 1) * B0]
            B = len(rows)
            with torch.cuda.device(dev):
                o_lr = torch.empty(B, C, P // 4, Q // 4, dtype=torch.float32, device=dev)
                o_pan = torch.empty(B, 1, P, Q, dtype=torch.float32, device=dev)
                o_mul = torch.empty(B, C, P, Q, dtype=torch.float32, device=dev) if st.mul is not None else None
                o_pl = torch.empty(B, 1, P // 4, Q // 4, dtype=torch.float32, device=dev)
                fp = ctypes.c_void_p(flips.data_ptr() + 4 * bi) if flips is not None else ctypes.c_void_p(0)
                _lib.check(L.lg_window_assemble(ptr(st.pan), ptr(st.lr), ptr(st.mul), ptr(d_org), len(org), bi * B0, fp, ptr(o_pan), ptr(o_lr),
                                                ptr(o_mul), ptr(o_pl), B, C, st.Hs, st.Ws, P, Q, st.dtype_code, self.divisor, n_div, post,
                                                _stream_ptr()), 'lg_window_assemble')
            batch = cls(input_lr=o_lr, input_pan=o_pan)
            if o_mul is not None:
                batch['target'] = o_mul
            batch['input_pan_l'] = o_pl
            batch['image_id'] = [window_id(y, x) for y, x in rows]
            yield batch
        if self.epoch == epoch:                 # a complete pass, and nobody called set_epoch meanwhile: the next pass is the next epoch
            self.set_epoch(epoch + 1)


def export_triplets(store, origins, out_dir, patch):
    """Writes the windows at `origins` as the triplets PSDataset reads -- {id}_pan.tif [P,Q], {id}_lr.tif [P/4,Q/4,C] and, with a target,
    {id}_mul.tif [P,Q,C], id = window_id(origin) -- through dataset.write_tiff.  -> the ids, in the order of `origins` (PSDataset sorts
    file names: for a row-major grid that is the same order)."""
    from .dataset import write_tiff
    os.makedirs(out_dir, exist_ok=True)
    org = np.asarray(origins).reshape(-1, 2)
    pan, lr, mul = store.windows(org, patch)
    ids = [window_id(y, x) for y, x in org]
    for i, name in enumerate(ids):
        write_tiff(os.path.join(out_dir, f'{name}_pan.tif'), pan[i, 0])
        write_tiff(os.path.join(out_dir, f'{name}_lr.tif'), lr[i].transpose(1, 2, 0))
        if mul is not None:
            write_tiff(os.path.join(out_dir, f'{name}_mul.tif'), mul[i].transpose(1, 2, 0))
    return ids


def read_scene(ms_path, pan_path):
    """the two TIFFs of a raw scene -> (ms [C,h,w], pan [1,4h,4w]) in the files' sample type"""
    from .dataset import read_tiff
    ms, pan = read_tiff(ms_path), read_tiff(pan_path)
    if ms.ndim != 3 or pan.ndim != 2:
        raise ValueError(f'{ms_path}: expected an MS image [h,w,C]; {pan_path}: a one-band PAN image (got {ms.shape} / {pan.shape})')
    return np.ascontiguousarray(ms.transpose(2, 0, 1)), np.ascontiguousarray(pan[np.newaxis])


def loader_from_config(ds, batch_size, device, **loader_kw):
    """dataset.build_loader's branch for a dataset.SceneDataset: read the scene, build the store, -> SceneLoader"""
    ms, pan = read_scene(ds.ms_path, ds.pan_path)
    store = SceneStore.from_scene(ms, pan, device, degrade=ds.degrade, gains_ms=ds.gains_ms, gain_pan=ds.gain_pan, phase=ds.phase, n_taps=ds.n_taps)
    return SceneLoader(store, ds.patch, batch_size, step=ds.step, mode='random' if ds.windows_per_epoch is not None else 'grid',
                       windows_per_epoch=ds.windows_per_epoch, region=ds.region, bit_depth=ds.bit_depth, norm_input=ds.norm_input, **loader_kw)
