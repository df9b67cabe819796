"""Runner counterpart of reference models/base/base_model.py restricted to the hot path's callers:
add_module :56, set_cuda :91 (one process per GPU + RCCL instead of nn.DataParallel), load_checkpoint :102,
set_optim :116 (Adam / AdamW / SGD / RMSprop -> their fused HIP steps), set_sched :137 (StepLR stepped EVERY iteration :197-199),
train :164, test :267 (reference-based indices PSNR / SSIM / Q / SAM / ERGAS on the reduced-resolution set, the no-reference
D_lambda / D_s / QNR on the full-resolution set), save :354 (same `train_out/` location; optimizer state added)."""
import contextlib
import os.path as osp

import numpy as np
import torch
import torch.nn as nn
from torch.optim import SGD, Adam, AdamW, RMSprop, lr_scheduler

from . import device_metrics as dmt
from . import metrics as mtc
from .compat import Timer, mkdir_or_exist
from .losses import get_loss_module


def data_normalize(img_dict, bit_depth):
    """reference dataset/utils.py:232-249"""
    max_value = 2 ** bit_depth - .5
    return {k: (v if k == 'image_id' else v / max_value) for k, v in img_dict.items()}


class NormalizedBatch(dict):
    """a batch whose tensors are ALREADY normalised the way `data_normalize` would (resident.ResidentLoader(fold_normalize=True) does it inside
    its gather kernel): `_train_batches` and `test` skip their own data_normalize for such a batch, and for nothing else"""
    normalized = True


def data_denormalize(img, bit_depth):
    """reference dataset/utils.py:252-263"""
    return img * (2 ** bit_depth - .5)


def smart_time(second):
    second = int(second)
    return f'{second // 3600}h {second % 3600 // 60}m {second % 60}s'


class Base_model:
    """The attribute names are the reference's (subclasses and configs rely on them: base_model.py:26-54); how they are filled is this
    build's."""
    OUT_DIRS = ('train_out', 'test_out0', 'test_out1')            # under <work_dir>/<datas>/ (base_model.py:44-46)
    FREQ_DEFAULTS = dict(save_freq=10000, test_freq=10000, eval_freq=10000, max_iter=100000)

    def __init__(self, cfg, logger, train_data_loader, test_data_loader0, test_data_loader1):
        self.cfg, self.logger = cfg, logger
        self.work_dir, self.datas = cfg.work_dir, cfg.datas
        self.train_data_loader, self.test_data_loader0, self.test_data_loader1 = train_data_loader, test_data_loader0, test_data_loader1
        mkdir_or_exist(self.work_dir)
        for d in self.OUT_DIRS:
            setattr(self, d, f'{self.work_dir}/{self.datas}/{d}')
        self.module_dict, self.optim_dict, self.sched_dict, self.switch_dict, self.eval_results = {}, {}, {}, {}, {}
        self.loss_module = get_loss_module(full_cfg=cfg, logger=logger)
        self.last_iter = 0
        self.rank, self.world = 0, 1      # one process per GPU: set_cuda() reads them from torch.distributed
        self.timer = Timer()

    def _barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()

    def add_module(self, module_name, module, switch=True):
        assert isinstance(module, nn.Module)
        self.module_dict[module_name] = module
        self.switch_dict[module_name] = switch

    def print_total_params(self):
        count = sum(sum(p.numel() for p in m.parameters()) for m in self.module_dict.values())
        self.logger.info(f'total params: {count},{round(count / (1000 ** 2), 4)} M')
        return count

    def init(self):
        pass

    def set_cuda(self):
        """one process per GPU (torch.distributed/RCCL set up by the launcher) -- replaces nn.DataParallel."""
        dev = torch.device('cuda', torch.cuda.current_device())
        import torch.distributed as dist
        ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.rank, self.world = (dist.get_rank(), dist.get_world_size()) if ddp else (0, 1)
        for name in self.module_dict:
            self.module_dict[name] = self.module_dict[name].to(dev)
            if ddp and hasattr(self.module_dict[name], 'attach_ddp'):
                self.module_dict[name].attach_ddp()       # rank-0 weights broadcast; gradients all-reduced every step
        for name in self.loss_module:
            self.loss_module[name] = self.loss_module[name].to(dev)

    def _load_modules(self, checkpoint):
        for module_name, module in self.module_dict.items():
            src = checkpoint[module_name]
            module.load_state_dict(src.state_dict() if hasattr(src, 'state_dict') else src)

    def _read_checkpoint(self, path, allow_pickle):
        """plain-tensor checkpoints (what save() writes; what tools/convert_checkpoint.py makes of a reference-era file) load with
        `weights_only=True`: nothing in the file is executed.  The reference's own format -- whole pickled module objects,
        base_model.py:362-368 -- runs code from the file while loading, so it is read only when the caller says the file is
        trusted: `allow_pickle=True` or `cfg.allow_pickled_checkpoint = True`."""
        if allow_pickle is None:
            allow_pickle = bool(self.cfg.get('allow_pickled_checkpoint', False))
        import pickle
        try:
            return torch.load(path, map_location='cpu', weights_only=True)
        except (pickle.UnpicklingError, RuntimeError) as e:   # what torch raises for anything beyond tensors / containers; a missing or
            if isinstance(e, RuntimeError) and 'weights_only' not in str(e).lower() and 'unsupported' not in str(e).lower() \
                    and 'global' not in str(e).lower():        # unreadable file (OSError, EOFError, a corrupt archive) is NOT a reason to unpickle
                raise
            if not allow_pickle:
                raise RuntimeError(
                    f'{path} is not a plain-tensor checkpoint (the reference pickles whole module objects). Convert it once with '
                    'tools/convert_checkpoint.py, or pass allow_pickle=True / set cfg.allow_pickled_checkpoint for a file you '
                    f'trust.  ({type(e).__name__}: {str(e)[:200]})') from e
        if self.logger is not None:
            self.logger.warning(f'{path}: not a plain-tensor checkpoint, unpickling it as allowed by allow_pickle / cfg.allow_pickled_checkpoint')
        return torch.load(path, map_location='cpu', weights_only=False)

    def load_checkpoint(self, path, allow_pickle=None):
        checkpoint = self._read_checkpoint(path, allow_pickle)
        self.last_iter = checkpoint['iter_num']
        self._load_modules(checkpoint)
        self._resume_optim = checkpoint.get('optim')     # checkpoints of this build carry it; restored by set_optim()
        for name, st in (self._resume_optim or {}).items():
            if name in self.optim_dict:
                self.optim_dict[name].load_state_dict(st)

    def load_pretrained(self, path, allow_pickle=None):
        self._load_modules(self._read_checkpoint(path, allow_pickle))

    def _train_controls(self):
        """cfg.train_cfg = dict(accumulate=, max_grad_norm=, ema_decay=, eval_ema=) as a TrainControls; None when the key is absent"""
        from .engine import TrainControls
        train_cfg = self.cfg.get('train_cfg', None)
        if train_cfg is None:
            return None
        known = ('accumulate', 'max_grad_norm', 'ema_decay', 'eval_ema')
        unknown = sorted(set(train_cfg) - set(known))
        if unknown:
            raise ValueError(f'cfg.train_cfg has unknown key(s) {unknown}: it takes {list(known)}')
        return TrainControls(**dict(train_cfg))

    def set_optim(self):
        from .engine import FUSED_OPTIMIZERS
        optim_cfg = self.cfg.get('optim_cfg', {})
        controls = self._train_controls()
        for module_name, module in self.module_dict.items():
            if module_name in optim_cfg:
                cfg = dict(optim_cfg[module_name])
                typ = cfg.pop('type')
                fused = cfg.pop('fused', True)
                # every type the reference accepts has a fused class with torch's arithmetic; `fused=False` in the entry selects torch's own
                torch_cls = {'Adam': Adam, 'RMSprop': RMSprop, 'SGD': SGD, 'AdamW': AdamW}
                if typ not in torch_cls:
                    raise SystemExit(f'No such type optim:{typ}')
                self.optim_dict[module_name] = (FUSED_OPTIMIZERS[typ] if fused else torch_cls[typ])(module.parameters(), **cfg)
            else:
                self.optim_dict[module_name] = Adam(module.parameters(), betas=(0.9, 0.999), lr=1e-4)
            if controls is not None:                      # before the state is restored: a checkpoint may sit inside an accumulation window
                optim = self.optim_dict[module_name]
                if getattr(optim, 'is_fused_lgteun', False):
                    optim.set_controls(controls)
                elif controls.ema_decay is not None:
                    raise ValueError("cfg.train_cfg: ema_decay needs the fused optimizer (the average is updated inside its launch); take "
                                     f"fused=False out of optim_cfg['{module_name}'] or ema_decay out of train_cfg")
                else:                                     # torch's own optimizer: train_iter accumulates and clips with torch's functions
                    optim.lgteun_controls, optim.lgteun_window_pos = controls, 0
            resume = getattr(self, '_resume_optim', None) or {}
            if module_name in resume:                     # load_checkpoint ran first (main.py order): continue the optimizer state
                self.optim_dict[module_name].load_state_dict(resume[module_name])

    def set_sched(self):
        sched_cfg = dict(self.cfg.get('sched_cfg', dict(step_size=10000, gamma=0.99)))
        for name, optim in self.optim_dict.items():
            self.sched_dict[name] = lr_scheduler.StepLR(optimizer=optim, **sched_cfg)

    def _device(self):
        return next(next(iter(self.module_dict.values())).parameters()).device

    def _due(self, freq, iter_id):
        """a periodic action of the training loop is due at this iteration (never at the last one, -1 switches it off: base_model.py:187-195)"""
        return freq != -1 and iter_id % freq == 0 and iter_id != self.cfg.max_iter

    def _train_batches(self, dev):
        """(iteration number, normalised device batch) from last_iter + 1 up to cfg.max_iter, cycling through the training loader"""
        it = self.last_iter
        while it < self.cfg.max_iter:
            for batch in self.train_data_loader:
                it += 1
                done = isinstance(batch, NormalizedBatch)
                batch = {k: (v.to(dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in batch.items()}
                yield it, (batch if done else data_normalize(batch, self.cfg.bit_depth))   # normalised unconditionally (base_model.py:181)
                if it >= self.cfg.max_iter:
                    return

    def train(self):
        """the training cadence of the reference (base_model.py:164-204): train_iter on every batch, then save / evaluate when due (the
        evaluation on the full-resolution set first, then the reduced-resolution one; fused images are written when test_freq is due too),
        then one StepLR tick per ITERATION for every switched-on module"""
        for key, default in self.FREQ_DEFAULTS.items():
            self.cfg.setdefault(key, default)
        self.timer = Timer()
        for iter_id, input_batch in self._train_batches(self._device()):
            for module in self.module_dict.values():
                module.train()
            self.train_iter(iter_id=iter_id, input_batch=input_batch)
            if self._due(self.cfg.save_freq, iter_id):
                self.save(iter_id=iter_id)
            if self._due(self.cfg.eval_freq, iter_id):
                write = self._due(self.cfg.test_freq, iter_id)
                for ref in (False, True):
                    self.test(iter_id=iter_id, save=write, ref=ref)
            for name, sched in self.sched_dict.items():
                if self.switch_dict[name]:
                    sched.step()

    def print_train_log(self, iter_id, loss_res, log_freq=10):
        if iter_id % log_freq == 0 and self.logger is not None and self.rank == 0:
            avg_iter_time = self.timer.since_last_check() / log_freq
            remain_time = avg_iter_time * (self.cfg.max_iter - iter_id)
            lr = self.optim_dict['core_module'].param_groups[0]['lr']
            self.logger.info(f'iteration {iter_id} of {self.cfg.max_iter} | lr {lr:.6f} | full loss {loss_res["full_loss"]:.6f} | '
                             f'time left {smart_time(remain_time)}')

    def get_model_output(self, input_batch):
        raise NotImplementedError

    def train_iter(self, iter_id, input_batch, log_freq=10):
        raise NotImplementedError

    @contextlib.contextmanager
    def _eval_weights(self):
        """cfg.train_cfg with ema_decay and eval_ema: the averaged weights sit in every fused module for the length of the block"""
        with contextlib.ExitStack() as stack:
            for name, module in self.module_dict.items():
                ctl = getattr(self.optim_dict.get(name), 'controls', None)
                core = module.module if hasattr(module, 'module') else module
                if ctl is not None and ctl.ema_decay is not None and ctl.eval_ema and hasattr(core, 'engine'):
                    stack.enter_context(core.engine().ema_weights(self.optim_dict[name]))
            yield

    @torch.no_grad()
    def test(self, iter_id, save=False, ref=True):
        """`_test` below, with the weights `cfg.train_cfg` asks for: the exponential moving average when it has ema_decay and eval_ema
        (the raw weights are back when the call returns or raises), the raw weights otherwise"""
        with self._eval_weights():
            return self._test(iter_id, save=save, ref=ref)

    @torch.no_grad()
    def _test(self, iter_id, save=False, ref=True):
        """evaluation (base_model.py:267-352).  ref=True: reduced-resolution set, PSNR / SSIM / Q / SAM / ERGAS against the target,
        `<metric>_mean` / `<metric>_std` lists in self.eval_results like the reference.  ref=False: the full-resolution set, no target:
        D_lambda / D_s / QNR from the fused image, the PAN and the MS input (lgteun_amd/metrics.py: pinned to the reference's values).  Inputs are always normalised; arrays are brought back
        to digital numbers before the metrics / the TIFF writer only with cfg.norm_input (base_model.py:296,311-316).
        cfg.eval_metrics: 'host' (default) scores every image with the float64 numpy functions of metrics.py; 'device' scores every batch
        on the GPU (device_metrics.py: the same definitions in fp64 HIP kernels), keeps the rows there and copies them to the host once,
        at the end -- the fused images leave the device only for the TIFF writer (save=True).
        cfg.eval_indices: 'standard' (default) or 'extended', which adds the literature's columns on either route: Q2n / SCC / CC behind the
        five, D_lambda_K / HQNR behind the three (MTF gains: cfg.mtf_gains_ms, else wald.DEFAULT_GAIN_MS).  The extended set needs 2 .. 8
        bands and images of at least 32 x 32 (ref=True) or 128 x 128 (ref=False): Q2n works on 32 x 32 blocks."""
        from .dataset import save_image
        metrics_on = self.cfg.get('eval_metrics', 'host')
        if metrics_on not in ('host', 'device'):
            raise ValueError(f"cfg.eval_metrics must be 'host' or 'device' (got {metrics_on!r})")
        indices = self.cfg.get('eval_indices', 'standard')
        if indices not in ('standard', 'extended'):
            raise ValueError(f"cfg.eval_indices must be 'standard' or 'extended' (got {indices!r})")
        ext, gains_ms = indices == 'extended', self.cfg.get('mtf_gains_ms')
        loader = self.test_data_loader1 if ref else self.test_data_loader0
        for module in self.module_dict.values():
            module.eval()
        dev = self._device()
        names = ['PSNR', 'SSIM', 'Q', 'SAM', 'ERGAS'] if ref else ['D_lambda', 'D_s', 'QNR']
        if ext:
            names = list(dmt.REF_EXT_NAMES if ref else dmt.NO_REF_EXT_NAMES)
        denorm = bool(self.cfg.get('norm_input', False))
        out_dir = osp.join(self.test_out1 if ref else self.test_out0, f'iter_{iter_id}')
        # one process per GPU: the evaluation set is SPLIT over the ranks (the reference is one process).  A loader built with this rank's
        # ShardedSampler (dataset.build_loader(rank, world)) or declared so with cfg.eval_sharded already yields this rank's share; of any
        # other loader (the same on every rank) rank r takes batches r, r + world, ...  Every rank writes the fused images of ITS share,
        # the per-image metric rows of all ranks are gathered in rank order before the mean / std.
        if save:
            mkdir_or_exist(out_dir)
        from .dataset import ShardedSampler
        inner = getattr(loader, 'loader', loader)
        sharded = self.world > 1 and (bool(self.cfg.get('eval_sharded', False)) or isinstance(getattr(inner, 'sampler', None), ShardedSampler))

        def to_np(t):   # [b c h w] -> [b h w c]
            t = data_denormalize(t, self.cfg.bit_depth) if denorm else t
            return t.permute(0, 2, 3, 1).cpu().numpy()
        # what identifies an image ACROSS ranks (`image_id` is a file-name prefix -- two directories may hold equal ones -- and may be
        # absent): the dataset index this rank's ShardedSampler hands out, in the order the loader consumes it; for a loader every rank iterates
        # in full (batches dealt out round-robin) the position in that common sequence; for a foreign pre-sharded loader nothing is known,
        # its rows are kept as they come (rank-tagged keys never collide)
        smp = getattr(inner, 'sampler', None)
        own_idx = [int(i) for i in smp] if (sharded and isinstance(smp, ShardedSampler)) else None
        res, ids, seen_here = [], [], 0
        dev_rows = []                     # eval_metrics = 'device': one [nb, k] float64 device tensor per batch
        scale = float(2 ** self.cfg.bit_depth - .5) if denorm else 1.0
        for bi, input_batch in enumerate(loader or []):
            if self.world > 1 and not sharded and bi % self.world != self.rank:
                continue
            done = isinstance(input_batch, NormalizedBatch)
            input_batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in input_batch.items()}
            if not done:
                input_batch = data_normalize(input_batch, self.cfg.bit_depth)
            fused = self.get_model_output(input_batch)
            nb = fused.shape[0]
            if ext:
                side = mtc.Q2N_BLOCK if ref else 4 * mtc.Q2N_BLOCK
                if not 2 <= fused.shape[1] <= mtc.Q2N_MAX_BANDS or min(fused.shape[2:]) < side:
                    raise ValueError(f"cfg.eval_indices = 'extended' needs 2 .. {mtc.Q2N_MAX_BANDS} bands and {'reduced' if ref else 'full'}-resolution "
                                     f'images of at least {side} x {side} (Q2n works on {mtc.Q2N_BLOCK} x {mtc.Q2N_BLOCK} blocks'
                                     f"{'' if ref else ' of the MS image'}); got {tuple(fused.shape[1:])}")
            if metrics_on == 'device':
                if ref:
                    score = dmt.ref_evaluate_ext_batch if ext else dmt.ref_evaluate_batch
                    dev_rows.append(score(fused.contiguous(), input_batch['target'].contiguous(), scale))
                elif ext:
                    dev_rows.append(dmt.no_ref_evaluate_ext_batch(fused.contiguous(), input_batch['input_pan'].contiguous(),
                                                                  input_batch['input_lr'].contiguous(), scale, gains_ms=gains_ms))
                else:
                    dev_rows.append(dmt.no_ref_evaluate_batch(fused.contiguous(), input_batch['input_pan'].contiguous(),
                                                              input_batch['input_lr'].contiguous(), scale))
                out = to_np(fused) if save else None
            else:
                out = to_np(fused)
                if ref:
                    gt = to_np(input_batch['target'])
                    score = mtc.ref_evaluate_ext if ext else mtc.ref_evaluate
                    res.extend(score(out[i], gt[i]) for i in range(nb))
                else:                                            # full-resolution set: no target (base_model.py:330-334)
                    pan_np, lr_np = to_np(input_batch['input_pan']), to_np(input_batch['input_lr'])
                    if ext:
                        res.extend(mtc.no_ref_evaluate_ext(out[i], pan_np[i], lr_np[i], gains_ms) for i in range(nb))
                    else:
                        res.extend(mtc.no_ref_evaluate(out[i], pan_np[i], lr_np[i]) for i in range(nb))
            if own_idx is not None:
                ids.extend(('idx', own_idx[seen_here + i]) for i in range(nb))
            elif not sharded:
                ids.extend(('pos', bi, i) for i in range(nb))
            else:
                ids.extend(('rank', self.rank, seen_here + i) for i in range(nb))
            seen_here += nb
            if save:
                for i, image_id in enumerate(input_batch['image_id']):
                    # [C, H, W] for the writer (the reference hands its HWC array to a CHW writer, base_model.py:336: a
                    # transposed file; not reproduced)
                    save_image(osp.join(out_dir, f'{image_id}_mul_hat.tif'), np.moveaxis(out[i], -1, 0))
        if dev_rows:
            res = torch.cat(dev_rows).cpu().tolist()          # the one device-to-host copy of the pass
        latest = {}
        if self.world > 1:
            import torch.distributed as dist
            rows = [None] * self.world
            dist.all_gather_object(rows, [(tuple(i), list(map(float, r))) for i, r in zip(ids, res)])
            # an image that reached two ranks (a PADDED sharded sampler wraps around when world does not divide the set: build the
            # evaluation loaders with build_loader(..., evaluation=True)) is scored once, like the reference's one-process loop:
            # told by its dataset index, never by its name
            seen, res = set(), []
            for part in rows:
                for i, r in part:
                    if i not in seen:
                        seen.add(i)
                        res.append(r)
        if res:
            res = np.array(res)
            for k, name in enumerate(names):
                self.eval_results.setdefault(f'{name}_mean', []).append(round(float(res[:, k].mean()), 4))
                self.eval_results.setdefault(f'{name}_std', []).append(round(float(res[:, k].std()), 4))
                latest[name] = (float(res[:, k].mean()), float(res[:, k].std()))
            if self.logger is not None and self.rank == 0:
                self.logger.info(f"iter {iter_id} {'low' if ref else 'full'}-resolution eval: {latest}")
        self._barrier()                    # no rank runs ahead of files another rank is still writing
        return latest

    def save(self, iter_id):
        """`train_out/model_iter_N.pth` like the reference (base_model.py:354-369), written by rank 0 only, holding plain tensors:
        {module name: state_dict, 'iter_num', 'optim': optimizer state (absent in the reference)} -- loadable with
        `weights_only=True`.  With cfg.train_cfg the modules' entries are still the RAW weights, so that a resumed run continues the same
        trajectory; the averaged weights (ema_decay) and the position inside an accumulation window travel in 'optim'.  `cfg.pickle_modules = True` writes the reference's own format instead (whole pickled module
        objects), for tools that expect it; such a file needs `allow_pickle` to be read back."""
        path = osp.join(self.train_out, f'model_iter_{iter_id}.pth')
        if self.rank == 0:
            mkdir_or_exist(self.train_out)
            ckpt = {'iter_num': iter_id}
            pickled = bool(self.cfg.get('pickle_modules', False))
            for name, module in self.module_dict.items():
                core = module.module if hasattr(module, 'module') else module
                ckpt[name] = core if pickled else {k: v.detach().cpu() for k, v in core.state_dict().items()}
            ckpt['optim'] = {k: v.state_dict() for k, v in self.optim_dict.items()}
            tmp = path + '.tmp'
            torch.save(ckpt, tmp)
            import os
            os.replace(tmp, path)          # readers never see a half-written file
        self._barrier()
        return path
