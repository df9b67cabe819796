"""Drop-in mirror of the reference's `models/unlg_former.py` surface for the MI355X-native path.

`Pansharpening` keeps the reference's constructor (cfg, logger, stage), call signature
`core_module(ms, pan)` (MS first, PAN second; unlg_former.py:84,94), NCHW fp32 I/O and -- key for
checkpoints (base_model.py:102-114,354-369) -- the identical `state_dict()` keys and shapes
(492 tensors at K=4).  The module tree below is built from stock torch layers used
ONLY as parameter containers (same default initialisation as the reference gets from PyTorch;
pos_emb ~ trunc_normal(0,1,[-2,2]) LGT.py:127-128, eta = 0.1 unlg_former.py:40).  No layer's
forward is ever called: compute goes through the HIP library (engine.py).  There is no CPU path.

`UnlgFormer` mirrors the runner wrapper (unlg_former.py:70-113): registered in MODELS under the
same name, same 5-argument constructor, `get_model_output` / `train_iter` with the same batch keys.
"""
import torch
import torch.nn as nn

from .base_model import Base_model
from .builder import MODELS
from .engine import Engine, canonical_names


def _point_conv(cin, cout):          # bmu.point_conv   basic_module_unformer_v2.py:13
    return nn.Conv2d(cin, cout, 1, 1, 0, groups=1)


def _dep_conv(c, k):                 # bmu.dep_conv     basic_module_unformer_v2.py:17
    return nn.Conv2d(c, c, k, 1, k // 2, groups=c)


class _Slot(nn.Identity):
    """Parameter-less placeholder keeping the reference's Sequential indices (sampling_unit_)."""


class _Box(nn.Module):
    """Named container (children are assigned as attributes)."""

    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            setattr(self, k, v)


class _LocalMixerParams(nn.Module):  # LGT.py:112-128
    def __init__(self, channels, win, heads):
        super().__init__()
        self.to_qkv = _point_conv(channels, channels * 3)
        self.pos_emb = nn.Parameter(torch.empty(1, heads, win * win, win * win))
        nn.init.trunc_normal_(self.pos_emb, mean=0.0, std=1.0, a=-2.0, b=2.0)


def _lgb(channels, nblocks, win, heads):     # LGT.py:222-248
    blocks = nn.ModuleList()
    for _ in range(nblocks):
        half = channels // 2
        mixer = _Box(
            local_mixer=_LocalMixerParams(half, win, heads),
            global_mixer=_Box(conv_amp=nn.Sequential(_dep_conv(half, 1)), conv_pha=nn.Sequential(_dep_conv(half, 1))),
            proj=_point_conv(channels, channels))
        ffn = _Box(net=nn.Sequential(
            _point_conv(channels, channels * 4), _Slot(),
            _Box(point_conv=_point_conv(channels * 4, channels * 4), depth_conv=_dep_conv(channels * 4, 3)),
            _Slot(), _point_conv(channels * 4, channels)))
        blocks.append(nn.ModuleList([
            _Box(fn=_Box(fn=mixer, norm=nn.LayerNorm(channels))),
            _Box(fn=_Box(fn=ffn, norm=nn.LayerNorm(channels)))]))
    return _Box(blocks=blocks)


def _lgt(in_channels, embed, win=8, num_block=(2, 1), heads=2):   # LGT.py:251-303
    m = _Box()
    m.patch_embed = _Box(proj=nn.Sequential(_dep_conv(in_channels, 1), _point_conv(in_channels, embed)),
                         norm=nn.LayerNorm(embed))
    m.encoder_layers = nn.ModuleList([nn.ModuleList([
        _lgb(embed, num_block[0], win, heads), nn.Sequential(_Slot(), _point_conv(embed, embed * 2))])])
    m.bottleneck = _lgb(embed * 2, num_block[1], win, heads)
    m.decoder_layers = nn.ModuleList([nn.ModuleList([
        nn.Sequential(_Slot(), _point_conv(embed * 2, embed)), _point_conv(embed * 2, embed),
        _lgb(embed, num_block[0], win, heads)])])
    m.tail = nn.Sequential(_Slot(), _point_conv(embed, in_channels))
    return m


class Pansharpening(nn.Module):
    """MI355X-native counterpart of reference `Pansharpening` (models/unlg_former.py:21-67)."""

    def __init__(self, cfg, logger, stage=5):
        super().__init__()
        self.in_channels = cfg.ms_chans
        self.stage = stage
        self.up_factor = 4
        C = self.in_channels
        self.D = nn.Sequential(_Slot(), _dep_conv(C, 3), _Slot(), _dep_conv(C, 3))
        self.DT = nn.Sequential(_Slot(), _dep_conv(C, 3), _Slot(), _dep_conv(C, 3))
        self.R = _point_conv(C, 1)
        self.RT = _point_conv(1, C)
        self.eta = nn.ParameterList([nn.Parameter(torch.tensor(0.1)) for _ in range(stage)])
        self.prior_module = nn.ModuleList([_lgt(C, C * 4) for _ in range(stage)])
        # execution options (not part of the reference surface)
        # 'faithful': run all K LGTs like the reference; 'live': skip the dead ones (identical results);
        # 'chained': the intended unfolding (stage i+1 consumes LGT_i's output; every parameter trains) -- NOT the reference's
        # results, opt-in only
        self.mode = 'faithful'
        self.faithful_eval = False  # True: also run the dead-stage LGTs in eval / no-grad forwards (timing the reference's work)
        self.precision = 'fp32'    # 'fp32': parity mode; 'bf16': saved / hidden FFN activations of the backward stored as bf16
        self._engine = None
        self._ddp = None           # (group,) once attach_ddp() was called: survives .to() / a rebuilt engine

    # ---- engine plumbing ----------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._engine = None            # parameters were re-created (.cuda()/.to()): flat storage is stale
        return r

    def __getstate__(self):
        st = self.__dict__.copy()
        st['_engine'] = None           # raw device handles never get pickled (torch.save of whole modules)
        st['_ddp'] = None              # ... nor process groups
        return st

    def engine(self):
        if self._engine is None or not self._engine.valid():
            self._engine = Engine(self)
            if self._ddp is not None:  # the data-parallel attachment belongs to the module, not to one Engine object
                # no broadcast here: a rebuild may happen on one rank only (a collective would hang) and must not overwrite what
                # the ranks loaded; call attach_ddp() again on EVERY rank to re-synchronise the weights
                self._engine.attach_ddp(self._ddp[0], broadcast=False, force=len(self._ddp) > 1 and self._ddp[1])
        return self._engine

    def attach_ddp(self, group=None, force=False):
        """join a torch.distributed process group (one process per GPU; backend nccl = RCCL over xGMI): rank-0 weights are
        broadcast and every train step / autograd backward all-reduces the flat gradient buffer.  A COLLECTIVE call: every rank
        of the group makes it (again after loading weights on one rank only).  Replaces the reference's nn.DataParallel wrap
        (models/base/base_model.py:91-100)."""
        self._ddp = None
        eng = self.engine()            # (re)built without an attachment
        self._ddp = (group, bool(force))
        return eng.attach_ddp(group, broadcast=True, force=force)

    def canonical_names(self):
        return canonical_names(self.in_channels, self.stage)

    def forward(self, ms, pan):
        if not ms.is_cuda:
            raise RuntimeError('lgteun_amd.Pansharpening runs on MI355X (HIP) only; there is no CPU path. '
                               'Move the module and inputs to cuda.')
        return self.engine().forward_autograd(ms, pan, training=self.training)

    def ema_state_dict(self, optim=None):
        """`state_dict()` with the exponentially averaged weights of `optim` (a fused optimizer whose controls have ema_decay; default: the
        one that last stepped this module) in place of the raw ones: detached copies, for export.  Before the first optimizer step the
        average is the weights themselves."""
        with self.engine().ema_weights(optim):
            return {k: v.detach().clone() for k, v in self.state_dict().items()}

    def fuse_scene(self, ms, pan, **kw):
        """one scene of any size, MS [C,h,w] / PAN [1,4h,4w], through overlapping tiles of the training size (lgteun_amd/scene.py)"""
        from .scene import fuse_scene
        return fuse_scene(self, ms, pan, **kw)


@MODELS.register_module()
class UnlgFormer(Base_model):
    """Runner wrapper with the reference's constructor and hooks (models/unlg_former.py:70-113)."""

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        super().__init__(cfg, logger, train_data_loader, test_data_loader0, test_data_loader1)
        model_cfg = cfg.get('model_cfg', dict())
        G_cfg = model_cfg.get('core_module', dict())
        self.add_module('core_module', Pansharpening(cfg=cfg, logger=logger, **G_cfg))

    def get_model_output(self, input_batch):
        input_pan = input_batch['input_pan']
        input_lr = input_batch['input_lr']
        tile = self.cfg.get('scene_tile', None)
        if tile is not None:
            # opt-in: every item as a tiled scene (eval mode, no_grad) -- how a full-resolution set above 1024 or off the 16-pixel grid is
            # evaluated.  The batch is already normalised: the tiles take the samples as they are.
            from .scene import default_overlap, fuse_scene
            G = self.module_dict['core_module']
            core = G.module if hasattr(G, 'module') else G
            overlap = self.cfg.get('scene_overlap', None)
            if overlap is None:
                overlap = default_overlap(input_pan.shape[2], input_pan.shape[3], tile)
            return torch.stack([fuse_scene(core, input_lr[i], input_pan[i], tile=tile, overlap=overlap) for i in range(input_pan.shape[0])])
        return self.module_dict['core_module'](input_lr, input_pan)

    def train_iter(self, iter_id, input_batch, log_freq=10):
        """Same contract as the reference train_iter.  With a fused optimizer (`set_optim` default on this
        build) and a rec_loss of type l1 or l2, forward + loss + backward + optimizer step run as four library calls with no
        per-iteration host sync (the reference's two `.item()` syncs, unlg_former.py:105,107, happen only every `log_freq`).
        A `noref_loss` entry (type 'qnr': losses.QNRLoss on the output, the PAN, the MS input and the batch's `input_pan_l`) rides in the
        same fused step, beside the rec_loss or -- for full-resolution data, which has no target -- on its own.  So do a `spectral_loss`
        entry (type 'sam': losses.SAMLoss) and a `struct_loss` entry (type 'ssim': losses.SSIMLoss), which compare the output with the
        batch's `target`.  The fused step is taken when every configured term has a fused form; the log carries each unweighted term and
        `full_loss`, their weighted sum."""
        G = self.module_dict['core_module']
        G_optim = self.optim_dict['core_module']
        loss_cfg = self.cfg.get('loss_cfg', {})
        w = float(loss_cfg['rec_loss'].w) if 'rec_loss' in self.loss_module else 0.0
        wn = float(loss_cfg['noref_loss'].w) if 'noref_loss' in self.loss_module else 0.0
        ws = float(loss_cfg['spectral_loss'].w) if 'spectral_loss' in self.loss_module else 0.0
        wt = float(loss_cfg['struct_loss'].w) if 'struct_loss' in self.loss_module else 0.0
        core = G.module if hasattr(G, 'module') else G
        fused_rec = 'rec_loss' in self.loss_module and self.loss_module['rec_loss'].get_type() in ('l1', 'l2')
        if (ws or wt) and input_batch.get('target') is None:
            raise ValueError("loss_cfg['spectral_loss'] / loss_cfg['struct_loss'] need the batch's 'target': SAM and SSIM compare the output "
                             'with a ground truth (full-resolution data has none; train it with noref_loss)')
        if getattr(G_optim, 'is_fused_lgteun', False) and fused_rec and not (wn or ws or wt):
            loss_t = core.engine().train_step(input_batch['input_lr'], input_batch['input_pan'], input_batch['target'],
                                              G_optim, loss_weight=w, loss_type=self.loss_module['rec_loss'].get_type())
            if iter_id % log_freq == 0:
                v = core.engine().global_loss()        # all ranks: under DDP `loss_t` is this rank's share of the global mean
                self.print_train_log(iter_id, dict(rec_loss=v / w if w else 0.0, full_loss=v), log_freq)
            return
        if getattr(G_optim, 'is_fused_lgteun', False) and (wn or ws or wt) and (fused_rec or 'rec_loss' not in self.loss_module):
            if wn and 'input_pan_l' not in input_batch:
                raise ValueError("loss_cfg['noref_loss'] needs the batch's 'input_pan_l' (the PAN at MS resolution; every loader of this build "
                                 'computes it)')
            eng = core.engine()
            eng.train_step(input_batch['input_lr'], input_batch['input_pan'], input_batch['target'] if fused_rec or ws or wt else None, G_optim,
                           loss_weight=w, loss_type=self.loss_module['rec_loss'].get_type() if fused_rec else 'l1',
                           pan_l=input_batch['input_pan_l'] if wn else None, noref_weight=wn, spectral_weight=ws, struct_weight=wt,
                           data_range=self.loss_module['struct_loss'].data_range if wt else 1.0)
            if iter_id % log_freq == 0:
                res = dict()                                           # the unweighted terms, and their weighted sum
                if wn:
                    res['noref_loss'] = eng.global_loss('noref')
                if fused_rec:
                    res['rec_loss'] = eng.global_loss()
                if ws:
                    res['spectral_loss'] = eng.global_loss('sam')
                if wt:
                    res['struct_loss'] = eng.global_loss('ssim')
                res['full_loss'] = wn * res.get('noref_loss', 0.0) + w * res.get('rec_loss', 0.0)
                if ws or wt:
                    res['full_loss'] += ws * res.get('spectral_loss', 0.0) + wt * res.get('struct_loss', 0.0)
                self.print_train_log(iter_id, res, log_freq)
            return
        output = G(input_batch['input_lr'], input_batch['input_pan'])
        loss_g = 0
        loss_res = dict()
        if 'rec_loss' in self.loss_module:
            rec_loss = self.loss_module['rec_loss'](out=output, gt=input_batch['target'])
            loss_g = loss_g + rec_loss * w
            loss_res['rec_loss'] = rec_loss.item()
        for name, wk in (('spectral_loss', ws), ('struct_loss', wt)):
            if name in self.loss_module:
                term = self.loss_module[name](out=output, gt=input_batch['target'])
                loss_g = loss_g + term * wk
                loss_res[name] = term.item()
        if 'noref_loss' in self.loss_module:
            noref_loss = self.loss_module['noref_loss'](pan=input_batch['input_pan'], ms=input_batch['input_lr'], out=output,
                                                        pan_l=input_batch.get('input_pan_l'))
            loss_g = loss_g + noref_loss * wn
            loss_res['noref_loss'] = noref_loss.item()
        loss_res['full_loss'] = loss_g.item()
        ctl = getattr(G_optim, 'lgteun_controls', None)      # cfg.train_cfg on torch's own optimizer: the window with torch's functions
        acc = ctl.accumulate if ctl is not None else 1
        pos = G_optim.lgteun_window_pos if acc > 1 else 0
        if pos == 0:
            G_optim.zero_grad()
        (loss_g / acc if acc > 1 else loss_g).backward()
        if pos + 1 >= acc:
            if ctl is not None and ctl.max_grad_norm is not None:
                self._torch_grad_norm = torch.nn.utils.clip_grad_norm_([p for p in core.parameters() if p.grad is not None], ctl.max_grad_norm)
            G_optim.step()
            pos = -1
        if acc > 1:
            G_optim.lgteun_window_pos = pos + 1
        self.print_train_log(iter_id, loss_res, log_freq)

    def last_grad_norm(self):
        """the global gradient norm of the last clipped optimizer step, before clipping (cfg.train_cfg with max_grad_norm), as a Python
        float: a host sync, for logging"""
        G = self.module_dict['core_module']
        if getattr(self.optim_dict['core_module'], 'is_fused_lgteun', False):
            return (G.module if hasattr(G, 'module') else G).engine().last_grad_norm()
        if getattr(self, '_torch_grad_norm', None) is None:
            raise RuntimeError('no gradient norm yet: cfg.train_cfg needs max_grad_norm, and one optimizer step')
        return float(self._torch_grad_norm)
