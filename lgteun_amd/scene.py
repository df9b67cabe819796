"""Tiled scene fusion: pan-sharpen an image larger than one plan (PAN above 1024 x 1024, or sides off the 16-pixel grid) on the GPU.

The scene stays on the device in its sample type.  `fuse_scene` cuts it into overlapping tiles of the training size (lg_scene_gather: one
launch per tile batch, the arithmetic of the resident loader's gather), sends the batches through the eval forward and blends the outputs
back with a separable window (lg_scene_blend), optionally leaving digital numbers (lg_scene_to_u16).  Kernels: lgteun_amd/csrc/k_scene.hip;
contracts: include/lgteun_hip.h.  The geometry below is pure Python: it imports without a GPU and without the built library.

    fused = net.fuse_scene(ms_u16, pan_u16, tile=128, overlap=32, bit_depth=11)          # [C,H,W] fp32 on the device

Geometry, per axis of length L with tile t (effective tile min(t, L)) and stride s = t - overlap: n = 1 tiles if L == t, else
ceil((L - t) / s) + 1, at origins min(i * s, L - t) -- the last tile sits flush with the border, nothing is padded.  With
overlap <= t / 2 at most 3 tiles cover a pixel per axis.  The window of local coordinate u in [0, t) is
w(u) = min(1, (min(u, t - 1 - u) + 1) / (overlap + 1)); a tile's weight is w(y) w(x); two tiles at nominal overlap sum to 1, and the
blend divides by the weight sum where a flush last tile overlaps more."""
import numpy as np

MAX_TILE = 1024          # lg_plan_create's limit
MAX_AUTO_BATCH = 64
_KINDS = ('uint8', 'uint16', 'float32')


def _axis(L, t, overlap):
    s = t - overlap
    n = 1 if L == t else -(-(L - t) // s) + 1
    return [min(i * s, L - t) for i in range(n)]


def effective_tile(H, W, tile):
    """(th, tw): the tile cut down to the scene where the scene is smaller"""
    th, tw = (tile, tile) if np.isscalar(tile) else tuple(tile)
    if int(th) != th or int(tw) != tw:
        raise ValueError(f'tile must be an int or a pair of ints (got {tile!r})')
    return min(int(th), int(H)), min(int(tw), int(W))


def check_geometry(H, W, tile, overlap):
    """-> (th, tw), the effective tile; ValueError says what to change"""
    for name, L in (('height', H), ('width', W)):
        if int(L) != L or L < 16 or L % 4:
            raise ValueError(f'scene {name} {L}: PAN sides must be multiples of 4 (4 x the MS side) and at least 16; crop or pad the scene')
    th, tw = effective_tile(H, W, tile)
    for name, t, L in (('height', th, H), ('width', tw, W)):
        if t < 16 or t % 16 or t > MAX_TILE:
            hint = (f'the scene {name} {L} is below the tile, so it is the tile: crop the scene to a multiple of 16 or choose a smaller tile'
                    if t == L and t >= 16 and t <= MAX_TILE else f'choose a multiple of 16 in 16 .. {MAX_TILE}')
            raise ValueError(f'tile {name} {t}: {hint}')
    if int(overlap) != overlap or overlap < 0 or overlap % 4 or 2 * overlap > min(th, tw):
        raise ValueError(f'overlap {overlap}: must be a non-negative multiple of 4 (MS pixels are 4 PAN pixels), at most half the smaller '
                         f'tile side ({min(th, tw) // 2} for tiles of {th} x {tw})')
    return th, tw


def tile_grid(H, W, tile, overlap):
    """-> (ys, xs): the PAN-pixel origins of the tiles per axis (tiles are numbered row-major: index = iy * len(xs) + ix)"""
    th, tw = check_geometry(H, W, tile, overlap)
    return _axis(int(H), th, int(overlap)), _axis(int(W), tw, int(overlap))


def window(t, overlap):
    """the blending window of a tile side t as float64 [t]"""
    u = np.arange(t)
    return np.minimum(1.0, (np.minimum(u, t - 1 - u) + 1) / (overlap + 1.0))


def default_overlap(H, W, tile):
    """a quarter of the smaller effective tile side, on the 4-pixel grid"""
    return min(effective_tile(H, W, tile)) // 16 * 4


def check_shapes(ms_shape, pan_shape):
    """-> (C, H, W) of MS [C,h,w] / PAN [1,4h,4w] (a leading batch axis of 1 is accepted)"""
    ms_shape, pan_shape = tuple(ms_shape), tuple(pan_shape)
    m = ms_shape[1:] if len(ms_shape) == 4 and ms_shape[0] == 1 else ms_shape
    p = pan_shape[1:] if len(pan_shape) == 4 and pan_shape[0] == 1 else pan_shape
    if len(m) != 3 or len(p) != 3 or p[0] != 1 or p[1] != 4 * m[1] or p[2] != 4 * m[2]:
        raise ValueError(f'expected MS [C,h,w] and PAN [1,4h,4w] (one scene; a leading batch axis of 1 is accepted), got {ms_shape} / {pan_shape}')
    return int(m[0]), int(p[1]), int(p[2])


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def _to_device(a, device, what):
    """-> (tensor on the device, kind); uint16 is held as an int16 view (the same bits; only the kernels read it)"""
    import torch
    if isinstance(a, np.ndarray):
        if a.dtype.name not in _KINDS:
            raise ValueError(f'{what}: sample type {a.dtype} is not supported (uint8, uint16 and float32 are; convert float64 with .astype(np.float32))')
        kind = a.dtype.name
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int16) if kind == 'uint16' else a).to(device)
    elif torch.is_tensor(a):
        names = {torch.uint8: 'uint8', torch.uint16: 'uint16', torch.int16: 'uint16', torch.float32: 'float32'}
        if a.dtype not in names:
            raise ValueError(f'{what}: sample type {a.dtype} is not supported (uint8, uint16 -- or its int16 view -- and float32 are)')
        kind = names[a.dtype]
        t = a.detach()
        if t.dtype == torch.uint16:
            t = t.view(torch.int16)
        t = t.to(device).contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
    else:
        raise ValueError(f'{what}: expected a numpy array or a torch tensor, got {type(a).__name__}')
    return t, kind


def auto_batch(engine, plan, C, th, tw, n_tiles, free_bytes):
    """the largest B <= min(64, n_tiles) that the plan accepts -- lg_workspace_bytes is 0 for a batch above the plan's bound (include/lgteun_hip.h:
    31 tiles of 1024 x 1024 at C = 4, 15 at C = 8) -- and whose inference workspace plus tile tensors fit into half of `free_bytes` (at least 1)"""
    per_tile = 4 * (th * tw + C * (th // 4) * (tw // 4) + C * th * tw)
    B = max(1, min(MAX_AUTO_BATCH, int(n_tiles)))
    while B > 1:
        need = int(engine.lib.lg_workspace_bytes(plan, B, 0))
        if need > 0 and need + B * per_tile <= free_bytes // 2:
            break
        B -= 1
    return B


class ScenePlan:
    """everything of one scene geometry that lives on the device across batches: the origin list (uploaded once), the tile tensors
    and the forward's workspace"""

    def __init__(self, module, C, H, W, tile, overlap, batch=None):
        import torch
        self.th, self.tw = check_geometry(H, W, tile, overlap)
        self.ys, self.xs = tile_grid(H, W, tile, overlap)
        self.C, self.H, self.W, self.overlap = C, H, W, int(overlap)
        self.n_tiles = len(self.ys) * len(self.xs)
        eng = module.engine()
        if C != eng.C:
            raise ValueError(f'the module was built for {eng.C} MS bands, the scene has {C}')
        self.engine, self.device = eng, eng.device
        self.plan = eng.plan(self.th, self.tw)
        if batch is None:
            batch = auto_batch(eng, self.plan, C, self.th, self.tw, self.n_tiles, torch.cuda.mem_get_info(self.device)[0])
        if int(batch) < 1:
            raise ValueError(f'batch must be positive (got {batch})')
        self.batch = B = min(int(batch), self.n_tiles, 65535)
        org = np.array([(y, x) for y in self.ys for x in self.xs], dtype=np.int32)
        self.origins = torch.from_numpy(org).to(self.device)                         # the scene's ONE upload besides the samples
        f32 = dict(dtype=torch.float32, device=self.device)
        self.t_pan = torch.empty(B, 1, self.th, self.tw, **f32)
        self.t_ms = torch.empty(B, C, self.th // 4, self.tw // 4, **f32)
        self.t_out = torch.empty(B, C, self.th, self.tw, **f32)
        self.ws = eng.workspace(self.plan, B, 0)

    def flags(self, module):
        f = self.engine.base_flags(False)
        if not getattr(module, 'faithful_eval', False):
            f &= ~_lib().LG_FLAG_FAITHFUL           # the dead stages change nothing in the output: forward_autograd's no-grad path
        return f


def _lib():
    from . import _lib as lib_mod
    return lib_mod


def fuse_scene(module, ms, pan, tile=128, overlap=32, batch=None, bit_depth=None, norm_input=False, out_dtype='float32', _plan=None):
    """Pan-sharpen one scene of any size with `module` (a Pansharpening on a GPU): MS [C,h,w], PAN [1,4h,4w] -> [C,4h,4w] on the device.

    ms / pan: numpy arrays (uint8, uint16, float32) or torch tensors, on the host or on the module's device (uint16 also as its int16 view).
    bit_depth: the runner's data_normalize (samples times the fp32 reciprocal of 2**bit_depth - 0.5); norm_input: the dataset's division by
    the same number before it.  The tile inputs are the bits ResidentLoader(fold_normalize=True) produces for the same samples.  Without
    bit_depth the samples go in as they are (already normalised float32).
    tile: int or (th, tw), multiples of 16 up to 1024 (cut down to the scene where the scene is smaller); overlap: PAN pixels, a multiple of
    4, at most half the smaller tile side.  batch: tiles per forward (None: the largest B <= 64 that fits into half of the free memory).
    The forwards run in eval mode under no_grad on the current stream; the dead stages run only with module.faithful_eval.
    out_dtype: 'float32' (normalised, like the forward's output) or 'uint16' (digital numbers clip(rint(x * (2**bit_depth - 0.5)), 0, 65535);
    needs bit_depth).  No host synchronisation beyond the uploads."""
    import ctypes

    import torch
    L = _lib()
    if out_dtype not in ('float32', 'uint16'):
        raise ValueError(f"out_dtype must be 'float32' or 'uint16' (got {out_dtype!r})")
    if (norm_input or out_dtype == 'uint16') and bit_depth is None:
        raise ValueError("norm_input and out_dtype='uint16' need bit_depth")
    C, H, W = check_shapes(ms.shape, pan.shape)
    check_geometry(H, W, tile, overlap)                       # before anything is uploaded
    eng = module.engine()
    ms_t, kind = _to_device(ms, eng.device, 'ms')
    pan_t, kind_p = _to_device(pan, eng.device, 'pan')
    if kind != kind_p:
        raise ValueError(f'ms ({kind}) and pan ({kind_p}) must have the same sample type')
    sp = _plan if _plan is not None else ScenePlan(module, C, H, W, tile, overlap, batch)
    divisor = float(2 ** bit_depth - .5) if bit_depth is not None else 1.0
    post = float(np.float32(1.0) / np.float32(divisor)) if bit_depth is not None else 1.0       # torch's tensor / scalar: resident.py _scaling
    n_div = 1 if norm_input else 0
    code = {'uint8': L.LG_DT_U8, 'uint16': L.LG_DT_U16, 'float32': L.LG_DT_F32}[kind]
    lib, flags = eng.lib, sp.flags(module)
    P = lambda t: ctypes.c_void_p(t.data_ptr())                                                  # noqa: E731
    with torch.no_grad(), torch.cuda.device(eng.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        scene = torch.empty(C, H, W, dtype=torch.float32, device=eng.device)
        for first in range(0, sp.n_tiles, sp.batch):
            B = min(sp.batch, sp.n_tiles - first)
            L.check(lib.lg_scene_gather(P(pan_t), P(ms_t), P(sp.origins), sp.n_tiles, first, P(sp.t_pan), P(sp.t_ms), B, C, H, W, sp.th, sp.tw,
                                        code, divisor, n_div, post, stream), 'lg_scene_gather')
            L.check(lib.lgteun_forward(sp.plan, P(eng.flat), P(sp.t_ms), P(sp.t_pan), P(sp.t_out), P(sp.ws), sp.ws.numel(), B, flags, 0, stream),
                    'lgteun_forward')
            L.check(lib.lg_scene_blend(P(sp.t_out), P(scene), first, B, C, H, W, sp.th, sp.tw, sp.overlap, stream), 'lg_scene_blend')
        if out_dtype == 'float32':
            return scene
        out = torch.empty(C, H, W, dtype=torch.uint16, device=eng.device)
        L.check(lib.lg_scene_to_u16(P(scene), P(out), scene.numel(), divisor, stream), 'lg_scene_to_u16')
        return out
