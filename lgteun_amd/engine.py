"""Host-side engine: flat parameter storage, plans, workspaces and the calls into the HIP library.

Layout decisions (MI355X-first):
  * all parameters of the net live in ONE flat fp32 device buffer in canonical state_dict order
    (each tensor 16-byte aligned); the nn.Parameters are views into it, so `state_dict()` /
    `load_state_dict()` / `.parameters()` keep working while kernels get base pointer + offsets,
    Adam is a single launch over two contiguous live ranges and the DDP bucket is the same two ranges.
  * gradients use an identical flat buffer; only live tensors (shared data module, eta, last stage's LGT)
    are ever written -- dead-stage parameters keep `grad is None` exactly like the reference.
  * one workspace tensor per (B, train) holds every activation; the library allocates nothing.
"""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import (LG_FLAG_BWD_DATA, LG_FLAG_BWD_LGT, LG_FLAG_CHAINED, LG_FLAG_DEFER_DEAD, LG_FLAG_DROPOUT, LG_FLAG_FAITHFUL, LG_FLAG_SAVE, LG_FLAG_STAGEWISE,
                   LgConfig, check, variant_from_env)


def _block_names(pre):
    m = pre + '0.fn.'
    f = pre + '1.fn.'
    return [m + 'fn.local_mixer.pos_emb', m + 'fn.local_mixer.to_qkv.weight', m + 'fn.local_mixer.to_qkv.bias',
            m + 'fn.global_mixer.conv_amp.0.weight', m + 'fn.global_mixer.conv_amp.0.bias',
            m + 'fn.global_mixer.conv_pha.0.weight', m + 'fn.global_mixer.conv_pha.0.bias',
            m + 'fn.proj.weight', m + 'fn.proj.bias', m + 'norm.weight', m + 'norm.bias',
            f + 'fn.net.0.weight', f + 'fn.net.0.bias', f + 'fn.net.2.point_conv.weight', f + 'fn.net.2.point_conv.bias',
            f + 'fn.net.2.depth_conv.weight', f + 'fn.net.2.depth_conv.bias', f + 'fn.net.4.weight', f + 'fn.net.4.bias',
            f + 'norm.weight', f + 'norm.bias']


def canonical_names(C, K):
    """Pansharpening.state_dict() key order of the reference (models/unlg_former.py:22-48): 12 shared tensors,
    K eta, then 119 per stage.  This order defines the offsets table handed to lg_plan_create."""
    names = []
    for n in ('D.1', 'D.3', 'DT.1', 'DT.3'):
        names += [n + '.weight', n + '.bias']
    names += ['R.weight', 'R.bias', 'RT.weight', 'RT.bias']
    names += [f'eta.{i}' for i in range(K)]
    for i in range(K):
        p = f'prior_module.{i}.'
        names += [p + 'patch_embed.proj.0.weight', p + 'patch_embed.proj.0.bias', p + 'patch_embed.proj.1.weight',
                  p + 'patch_embed.proj.1.bias', p + 'patch_embed.norm.weight', p + 'patch_embed.norm.bias']
        names += _block_names(p + 'encoder_layers.0.0.blocks.0.')
        names += _block_names(p + 'encoder_layers.0.0.blocks.1.')
        names += [p + 'encoder_layers.0.1.1.weight', p + 'encoder_layers.0.1.1.bias']
        names += _block_names(p + 'bottleneck.blocks.0.')
        names += [p + 'decoder_layers.0.0.1.weight', p + 'decoder_layers.0.0.1.bias',
                  p + 'decoder_layers.0.1.weight', p + 'decoder_layers.0.1.bias']
        names += _block_names(p + 'decoder_layers.0.2.blocks.0.')
        names += _block_names(p + 'decoder_layers.0.2.blocks.1.')
        names += [p + 'tail.1.weight', p + 'tail.1.bias']
    return names


def flat_layout(names, numels, K):
    """offsets (floats, each tensor 16-byte aligned) of the canonical tensors in the flat buffers, total size, indices of
    the live tensors and the two contiguous live ranges [(shared + eta), (last stage's LGT)]  (SURVEY D3)."""
    offs, total = [], 0
    for n in numels:
        offs.append(total)
        total += (max(n, 1) + 3) // 4 * 4
    n_head = 12 + K
    first_last = 12 + K + 119 * (K - 1)
    live_idx = list(range(n_head)) + list(range(first_last, len(names)))
    live_ranges = [(0, offs[n_head] if n_head < len(offs) else total), (offs[first_last], total)]
    return offs, total, live_idx, live_ranges


def _stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _aligned(t):
    """`t` as the library takes a float tensor: contiguous and 16-byte aligned (the kernels read float4).  A contiguous view that starts inside a
    storage -- base[1:] of a flat buffer -- is copied to a tensor of its own, like scene.py's inputs; the caller's storage is only read"""
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


class TrainControls:
    """What a training run asks for around the optimizer of the fused step; attached with `optimizer.set_controls(...)`, or by the runner
    from `cfg.train_cfg`.  Everything is off by default, and an optimizer without controls steps exactly as it always did.
      accumulate     A >= 1: a step is a WINDOW of A train_step calls.  Each call adds its gradients, at loss scale loss_weight / A; only
                     the last one reduces across ranks, clips and steps the optimizer.  A scheduler keeps ticking per call, and the
                     learning rate a window applies is the one at its LAST call.
      max_grad_norm  clip the global L2 norm of the gradients to this value (torch.nn.utils.clip_grad_norm_): the norm and the coefficient
                     are taken on the device, behind the all-reduce, and the optimizer launch reads the coefficient there
      ema_decay      keep an exponential moving average of the weights, updated inside the optimizer launch: optimizer state 'ema'
      eval_ema       the runner evaluates (Base_model.test) with the averaged weights"""

    def __init__(self, accumulate=1, max_grad_norm=None, ema_decay=None, eval_ema=True):
        if isinstance(accumulate, bool) or not isinstance(accumulate, (int, np.integer)) or accumulate < 1:
            raise ValueError(f'accumulate must be an integer >= 1 (got {accumulate!r}): the number of train_step calls per optimizer step')
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float, np.integer, np.floating)) \
                    or not math.isfinite(max_grad_norm) or max_grad_norm <= 0:
                raise ValueError(f'max_grad_norm must be None (no clipping) or a finite number > 0 (got {max_grad_norm!r})')
        if ema_decay is not None:
            if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float, np.integer, np.floating)) or not 0.5 < ema_decay < 1:
                raise ValueError(f'ema_decay must be None (no average) or lie in 0.5 < decay < 1 (got {ema_decay!r}): the average moves by '
                                 '1 - decay per step, e.g. 0.999')
        self.accumulate = int(accumulate)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.eval_ema = bool(eval_ema)

    def is_window_end(self, call):
        """call: 0-based count of train_step calls; True where that call ends a window, i.e. steps the optimizer"""
        return (call + 1) % self.accumulate == 0

    def as_dict(self):
        return dict(accumulate=self.accumulate, max_grad_norm=self.max_grad_norm, ema_decay=self.ema_decay, eval_ema=self.eval_ema)

    def __repr__(self):
        return 'TrainControls(' + ', '.join(f'{k}={v!r}' for k, v in self.as_dict().items()) + ')'


class Engine:
    def __init__(self, module):
        self.lib = _lib.lib()          # raises if the HIP library is not built -- no fallback
        self.C = int(module.in_channels)
        self.K = int(module.stage)
        self.module_mode = lambda: module.mode
        self.module_faithful_eval = lambda: getattr(module, 'faithful_eval', False)
        self.module_precision = lambda: getattr(module, 'precision', 'fp32')
        names = canonical_names(self.C, self.K)
        params = dict(module.named_parameters())
        if set(names) != set(params):
            raise RuntimeError('parameter surface does not match the canonical LGTEUN state_dict')
        dev = params[names[0]].device
        if dev.type != 'cuda':
            raise RuntimeError('lgteun_amd: parameters must live on an MI355X (cuda) device')
        for n in names:
            if params[n].device != dev or params[n].dtype != torch.float32:
                raise RuntimeError(f'parameter {n}: expected float32 on {dev}')
        self.device = dev
        self.names = names
        offs, total, d3_idx, d3_ranges = flat_layout(names, [params[n].numel() for n in names], self.K)
        self.offsets = offs
        self.total = total
        # which tensors get a gradient: the reference's graph (shared + eta + last LGT) or, in 'chained' mode, all
        self._live = {False: (d3_idx, d3_ranges), True: (list(range(len(names))), [(0, total)])}
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.params = [params[n] for n in names]
        for n, o in zip(names, offs):
            p = params[n]
            view = self.flat[o:o + p.numel()].view(p.shape)
            view.copy_(p.data)
            p.data = view
        # gradients + (one 16-byte slot behind them) the loss scalar of the fused step: ONE buffer, so that train_step clears both with one fill launch
        self._gbuf = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.gflat = self._gbuf[:total]
        self._ranges_dev = {ch: torch.tensor([v for r in rg for v in r], dtype=torch.int64, device=dev)
                            for ch, (_, rg) in self._live.items()}
        self._plans = {}
        self._ws = {}
        self._ws_pool = {}             # autograd path: released training workspaces by (plan, B, train), see _WsLease
        self._loss = self._gbuf[total:total + 1]
        # the second float of that slot (the fill launch clears all four; nothing else reads them): the no-reference (QNR) loss of the
        # fused step, kept apart from the reconstruction loss so that a combined step can log both terms
        self._noref = self._gbuf[total + 1:total + 2]
        # ... and the third and fourth: the spectral (SAM) and the structural (1 - SSIM) loss of a step with spectral_weight / struct_weight
        self._sam = self._gbuf[total + 2:total + 3]
        self._ssim = self._gbuf[total + 3:total + 4]
        self._seed_ctr = 0
        # opt-in (LG_OVERLAP_DEAD=1 / engine.overlap_dead = True): 'faithful' training enqueues the K-1 dead-stage LGT forwards on a
        # second stream behind the LGT backward, beside the K data-step backwards + Adam (a chain of small latency-bound launches).
        # Bitwise the same step (tested).  Measured +0.9 % pairs/s only -- the persistent forward kernels fill every CU's LDS, so the
        # small launches get in at kernel boundaries -- while the co-running launches stretch the fused FFN's measured duration by
        # 6 %, so the default keeps one stream and per-kernel numbers that mean what they say.
        self.overlap_dead = os.environ.get('LG_OVERLAP_DEAD', '0') == '1'
        # 'faithful' mode with two or more dead stages: the library runs their LGT forwards as ONE pass over (K-1) B samples where the plan's
        # kernels can (include/lgteun_hip.h: LG_FLAG_STAGEWISE).  dead_stagewise = True (LG_DEAD_STAGEWISE=1) sets the bit: one stage at a
        # time, bitwise the same step -- the reference of the tests and the other leg of an A/B.
        self.dead_stagewise = os.environ.get('LG_DEAD_STAGEWISE', '0') == '1'
        self.variant = None            # lg_config.variant of the plans: None = from the diagnostic LG_* environment variables (normally 0)
        self._side_stream = None
        self.world = 1
        self.rank = 0
        self.process_group = None
        self.buckets = None
        self.force_collectives = False   # attach_ddp(force=True): collectives also in a group of one rank
        self.local_only = False        # True: the caller runs independent replicas inside an initialised process group on purpose
        self._clip = None              # TrainControls.max_grad_norm: [norm, clip coefficient] of the last optimizer step, on the device
        self._norm_ws = None
        self._qnr_bufs = {}            # train_step with noref_weight: (workspace, table, indices) of lg_qnr_stats / lg_qnr_grad by (B, H, W)
        self._qnr_last = None          # ... and what the last such call used: dict(table, indices, dout), on the device
        self._recloss_ws = {}          # train_step with spectral_weight / struct_weight: the workspace of lg_sam_loss / lg_ssim_loss by (B, H, W)
        self._recloss_last = None      # ... and what the last such call used: dict(dout), on the device
        self._window_seen = 1          # train_step calls of the current accumulation window so far (global_loss divides by it)
        self._optim = None             # the fused optimizer of the last train_step: whose 'ema' state ema_weights() swaps in

    def chained(self):
        return self.module_mode() == 'chained'

    @property
    def live_idx(self):
        return self._live[self.chained()][0]

    @property
    def live_ranges(self):
        return self._live[self.chained()][1]

    @property
    def ranges_dev(self):
        return self._ranges_dev[self.chained()]

    @property
    def max_range(self):
        return max(b - a for a, b in self.live_ranges)

    def attach_ddp(self, group=None, broadcast=True, force=False):
        """join a torch.distributed group: reduce the flat gradient buffer every step.  broadcast=True (an explicit
        `module.attach_ddp()`): rank-0 weights go to every rank -- a COLLECTIVE, so every rank of the group must make the call.
        broadcast=False (an engine rebuilt under an attached module, e.g. after `.to()`): no communication; the ranks' weights
        were made equal by the first attachment and identical updates keep them equal.
        force=True: issue the collectives in a group of ONE rank too (the broadcast here, the all-reduce(s) of every train step) --
        how a single-GPU box exercises the RCCL communicator and the bucket code an 8-GPU run takes (tests, `LGTEUN_FORCE_PG`)."""
        import torch.distributed as dist
        from .ddp import GradBuckets, broadcast_flat
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.process_group = group
        self.force_collectives = bool(force and dist.is_initialized())
        if self.world > 1 or self.force_collectives:
            if broadcast:
                broadcast_flat(self.flat, 0, group, force=self.force_collectives)
            self.buckets = {ch: GradBuckets(rg, group) for ch, (_, rg) in self._live.items()}
        return self

    def global_loss(self, which='rec'):
        """the GLOBAL-mean loss of the last train_step as a Python float (host sync; under DDP one scalar all-reduce: `_loss`
        holds this rank's share of the global mean).  For the logging cadence only.  Inside an accumulation window
        (TrainControls.accumulate) `_loss` is the sum over the window's calls so far: the mean over those micro-batches is returned.
        which='rec': the reconstruction term (l1 / l2); which='noref': the no-reference term (1 - QNR) of a step with noref_weight;
        which='sam' / 'ssim': the spectral angle / 1 - SSIM of a step with spectral_weight / struct_weight.  All are the unweighted
        loss values."""
        slots = dict(rec=self._loss, noref=self._noref, sam=self._sam, ssim=self._ssim)
        if which not in slots:
            raise ValueError(f"which must be 'rec', 'noref', 'sam' or 'ssim' (got {which!r})")
        t = slots[which].clone()
        if self._window_seen > 1:
            t /= self._window_seen
        if self.world > 1:
            import torch.distributed as dist
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.process_group)
        return float(t.item())

    def _check_attached(self):
        """a process group with more than one rank exists but this engine never joined it: every rank would train on its own
        shard without the gradient all-reduce and silently diverge (reference: nn.DataParallel reduces implicitly,
        base_model.py:91-100)"""
        if self.world > 1 or self.local_only:
            return
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise RuntimeError('torch.distributed is initialised with world size > 1 but this engine is not attached: call '
                               'module.attach_ddp() (or set engine.local_only = True for independent replicas)')

    # ------------------------------------------------------------------------------------------
    def valid(self):
        """every parameter is still the view into the flat buffer it was given (a caller that re-assigns one tensor's `.data`,
        `.to()`, a re-created parameter: the kernels would read stale weights) -- 492 pointer compares at K = 4, ~50 us"""
        flat_ptr = self.flat.data_ptr()
        return all(p.data_ptr() == flat_ptr + 4 * o for p, o in zip(self.params, self.offsets))

    def __del__(self):
        try:
            for pl in self._plans.values():
                self.lib.lg_plan_destroy(pl)
        except Exception:  # noqa: BLE001
            pass

    def plan(self, H, W):
        prec = {'fp32': 0, 'bf16': 1}[self.module_precision()]
        var = variant_from_env() if self.variant is None else int(self.variant)
        key = (H, W, prec, var)
        if key not in self._plans:
            cfg = LgConfig(self.C, self.K, H, W, prec, var)
            arr = (ctypes.c_int64 * len(self.offsets))(*self.offsets)
            out = ctypes.c_void_p()
            check(self.lib.lg_plan_create(ctypes.byref(cfg), arr, len(self.offsets), ctypes.byref(out)), 'lg_plan_create')
            self._plans[key] = out
        return self._plans[key]

    def describe(self, H, W):
        """which kernels the plan of an H x W PAN runs, what its saving forward keeps and its backward reads (lg_plan_describe)"""
        buf = ctypes.create_string_buffer(2048)
        check(self.lib.lg_plan_describe(self.plan(H, W), buf, len(buf)), 'lg_plan_describe')
        return buf.value.decode()

    def workspace(self, plan, B, train):
        """train: 0 inference, 1 training, 2 chained training (K saved activation sets)"""
        need = self.lib.lg_workspace_bytes(plan, B, int(train))
        key = (plan.value, B, int(train))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    def lease_workspace(self, plan, B, train):
        """a training workspace of its own for one autograd graph: the saved activations of a forward must survive until ITS
        backward, whatever other forwards (a second graph with the same B, Engine.train_step) run in between.  The lease
        returns the buffer to a pool when the autograd context that holds it is freed."""
        need = self.lib.lg_workspace_bytes(plan, B, int(train))
        key = (plan.value, B, int(train))
        pool = self._ws_pool.setdefault(key, [])
        ws = pool.pop() if pool else None
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return _WsLease(ws, pool)

    def next_seed(self):
        """dropout counter seed: torch's seed, a per-step counter and the DDP rank (ranks seeded alike must not draw the same
        masks for their shards)"""
        self._seed_ctr += 1
        return (torch.initial_seed() * 0x9E3779B1 + self._seed_ctr + self.rank * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF

    def _check_inputs(self, ms, pan):
        if ms.dim() != 4 or pan.dim() != 4 or ms.shape[1] != self.C or pan.shape[1] != 1:
            raise ValueError(f'expected ms [B,{self.C},h,w] and pan [B,1,4h,4w], got {tuple(ms.shape)} / {tuple(pan.shape)}')
        B, _, h, w = ms.shape
        if pan.shape[0] != B or pan.shape[2] != 4 * h or pan.shape[3] != 4 * w:
            raise ValueError('pan must be 4x the MS size')
        if ms.dtype != torch.float32 or pan.dtype != torch.float32:
            raise ValueError('inputs must be float32 (NCHW), like the reference')
        if ms.device != self.device or pan.device != self.device:
            raise ValueError(f'inputs must be on {self.device}')
        return B, 4 * h, 4 * w

    # ------------------------------------------------------------------------------------------
    def forward_raw(self, ms, pan, flags, seed=0, lease=False):
        B, H, W = self._check_inputs(ms, pan)
        ms = _aligned(ms)
        pan = _aligned(pan)
        plan = self.plan(H, W)
        train = (2 if flags & LG_FLAG_CHAINED else 1) if flags & LG_FLAG_SAVE else 0
        if lease:
            holder = self.lease_workspace(plan, B, train)
            ws = holder.ws
        else:
            holder = None
            ws = self.workspace(plan, B, train)
        out = torch.empty(B, self.C, H, W, dtype=torch.float32, device=self.device)
        check(self.lib.lgteun_forward(plan, _ptr(self.flat), _ptr(ms), _ptr(pan), _ptr(out), _ptr(ws), ws.numel(), B, flags,
                                      seed, _stream_ptr()), 'lgteun_forward')
        return out, (plan, ws, ms, pan, B, holder)

    def backward_raw(self, saved, dout, gflat, flags, seed=0):
        plan, ws, ms, pan, B = saved[:5]
        dout = _aligned(dout)
        check(self.lib.lgteun_backward(plan, _ptr(self.flat), _ptr(gflat), _ptr(ms), _ptr(pan), _ptr(dout), _ptr(ws),
                                       ws.numel(), B, flags, seed, _stream_ptr()), 'lgteun_backward')

    def base_flags(self, training):
        mode = self.module_mode()
        if mode not in ('faithful', 'live', 'chained'):
            raise ValueError(f"mode must be 'faithful', 'live' or 'chained' (got {mode!r})")
        f = {'faithful': LG_FLAG_FAITHFUL, 'live': 0, 'chained': LG_FLAG_CHAINED}[mode]
        if self.dead_stagewise:
            f |= LG_FLAG_STAGEWISE
        if training:
            f |= LG_FLAG_DROPOUT
        return f

    def forward_autograd(self, ms, pan, training):
        flags = self.base_flags(training)
        need_grad = torch.is_grad_enabled() and any(self.params[i].requires_grad for i in self.live_idx)
        if not need_grad:
            if not training and not self.module_faithful_eval():
                # inference: the K-1 dead-stage LGTs change nothing in the output (bitwise, tested) -- they run only
                # where the reference's WORK is being reproduced (training in 'faithful' mode, or module.faithful_eval = True)
                flags &= ~LG_FLAG_FAITHFUL
            out, _ = self.forward_raw(ms, pan, flags, self.next_seed() if training else 0)
            return out
        live = [self.params[i] for i in self.live_idx]
        return _LgteunFn.apply(self, ms, pan, flags, *live)

    # ------------------------------------------------------------------------------------------
    def train_step(self, ms, pan, gt, optim, loss_weight=1.0, loss_type='l1', *, pan_l=None, noref_weight=0.0, spectral_weight=0.0,
                   struct_weight=0.0, data_range=1.0):
        """forward + L1 / L2 (mean) + backward + the fused optimizer's step as library calls; returns the device loss scalar (this
        rank's share).  With `optim.controls` (TrainControls) a call is one micro-batch of a window of `accumulate` calls: the first
        clears gradients and loss, every call adds its gradients at loss scale loss_weight / accumulate and its loss to the scalar, and
        only the last issues the all-reduce, the norm (max_grad_norm) and the optimizer launch.  The learning rate applied is the one
        `optim.param_groups[0]['lr']` holds at that last call.
        noref_weight != 0 adds noref_weight * (1 - QNR) of (output, pan, ms, pan_l) (losses.QNRLoss; lg_qnr_stats + lg_qnr_grad): it
        needs `pan_l`, the batch's `input_pan_l`, and not a ground truth -- with gt=None the reconstruction call is skipped, the step is
        purely unsupervised and the scalar returned is the QNR one (`_noref`, which global_loss('noref') reads).  The QNR of a
        micro-batch is its own (the loss is not additive over samples); under data parallelism it is the QNR of the GLOBAL micro-batch,
        through one SUM all-reduce of the P-double table between the two library calls.
        spectral_weight != 0 adds spectral_weight * SAM(output, gt) (losses.SAMLoss; lg_sam_loss), struct_weight != 0 adds
        struct_weight * (1 - SSIM(output, gt)) with `data_range` (losses.SSIMLoss; lg_ssim_loss); both need `gt`.  The terms meet on dout
        in the order reconstruction, SAM, SSIM, QNR: the first one present writes it, the later ones add to it.  With one of the two, a
        loss_weight of 0 skips the reconstruction call, so SAM / SSIM can train alone.  Both are means over the global batch: every rank
        adds its share to `_sam` / `_ssim` (global_loss('sam' / 'ssim')) and no collective is needed.  The scalar returned is that of the
        first term present."""
        if loss_type not in ('l1', 'l2'):
            raise ValueError(f"loss_type must be 'l1' or 'l2' (got {loss_type!r})")
        noref = float(noref_weight) != 0.0
        sam, ssim = float(spectral_weight) != 0.0, float(struct_weight) != 0.0
        if (sam or ssim) and gt is None:
            raise ValueError('spectral_weight / struct_weight != 0 need gt, the target: SAM and SSIM compare the output with a ground truth')
        rec = gt is not None and (float(loss_weight) != 0.0 or not (sam or ssim))
        if noref and pan_l is None:
            raise ValueError("noref_weight != 0 needs pan_l, the PAN at MS resolution: the batch's 'input_pan_l' (every loader computes it)")
        if gt is None and not noref:
            raise ValueError('gt=None needs noref_weight != 0: without a ground truth only the no-reference loss can train')
        self._check_attached()
        ctl = getattr(optim, 'controls', None)
        acc = ctl.accumulate if ctl is not None else 1
        pos = optim._window_pos if acc > 1 else 0
        last = pos + 1 >= acc
        flags = self.base_flags(True) | LG_FLAG_SAVE
        if not getattr(optim, 'dropout', True):
            flags &= ~LG_FLAG_DROPOUT
        seed = self.next_seed()
        if pos == 0:
            self._gbuf.zero_()             # gradients and the loss scalar
        elif optim._window_gbuf is not None and optim._window_gbuf is not self._gbuf:
            self._gbuf.copy_(optim._window_gbuf)     # a window cut by a checkpoint: what its earlier calls had accumulated
        if acc > 1:
            optim._window_gbuf = None
        defer = bool(self.overlap_dead and (flags & LG_FLAG_FAITHFUL) and not (flags & LG_FLAG_CHAINED) and self.K > 1)
        if defer:
            flags |= LG_FLAG_DEFER_DEAD
        out, saved = self.forward_raw(ms, pan, flags, seed)
        dout = torch.empty_like(out)
        if gt is not None:
            gt = _aligned(gt)
        if rec:
            n_local = out.numel()
            loss_fn = self.lib.lg_l1_loss if loss_type == 'l1' else self.lib.lg_l2_loss
            scale = float(loss_weight) if acc == 1 else float(loss_weight) / acc
            check(loss_fn(_ptr(out), _ptr(gt), _ptr(dout), _ptr(self._loss), n_local, n_local * self.world, scale,
                          _stream_ptr()), f'lg_{loss_type}_loss')
        if sam or ssim:
            self._spectral_struct_loss(out, gt, dout, float(spectral_weight) / acc, float(struct_weight) / acc, float(data_range), accumulate=rec)
        if noref:
            self._qnr_loss(out, saved[3], saved[2], pan_l, dout, float(noref_weight) / acc, accumulate=rec or sam or ssim)
        bk = self.buckets[bool(flags & LG_FLAG_CHAINED)] if (last and (self.world > 1 or self.force_collectives)) else None
        overlap = bool(bk is not None and bk.overlap and not (flags & LG_FLAG_CHAINED))
        if defer or overlap:
            # two backward calls: the dead-stage forwards (side stream) and / or the opt-in asynchronous bucket of the last stage's
            # LGT start behind the LGT backward and run beside the K data-step backwards
            self.backward_raw(saved, dout, self.gflat, flags | LG_FLAG_BWD_LGT, seed)
            if defer:
                self._dead_forward(saved, flags, seed)
            if overlap:
                bk.start(self.gflat, 1)
            self.backward_raw(saved, dout, self.gflat, flags | LG_FLAG_BWD_DATA, seed)
            if overlap:
                if bk.serial:
                    bk.finish()            # the LGT bucket's result is in before the shared bucket starts
                bk.start(self.gflat, 0)
                bk.finish()
        else:
            self.backward_raw(saved, dout, self.gflat, flags, seed)
        if bk is not None and not overlap:
            bk.all_reduce(self.gflat)      # default: ONE stream-ordered collective behind the whole backward (ddp.py)
        self._window_seen = pos + 1
        self._optim = optim
        if last:
            if ctl is not None and ctl.max_grad_norm is not None:
                self.grad_norm(ctl.max_grad_norm)      # behind the all-reduce: the global gradient, the same coefficient on every rank
            optim.step_flat(self)
            if acc > 1:
                optim._window_pos = 0
        else:
            optim._window_pos = pos + 1
            optim._window_gbuf = self._gbuf            # a checkpoint written inside the window carries the gradients so far
        if defer:
            torch.cuda.current_stream().wait_stream(self._side_stream)   # the step ends when its dead-stage work has ended
        return self._loss if rec else (self._sam if sam else (self._ssim if ssim else self._noref))

    def _spectral_struct_loss(self, out, gt, dout, w_sam, w_ssim, data_range, accumulate):
        """dout (+)= w_sam * d SAM / d out + w_ssim * d(1 - SSIM) / d out, `_sam` / `_ssim` += this rank's share of the global means:
        lg_sam_loss, then lg_ssim_loss, one workspace for both.  accumulate: an earlier term wrote dout.  No host synchronisation."""
        B, C, H, W = out.shape
        if tuple(gt.shape) != (B, C, H, W) or gt.dtype != torch.float32 or gt.device != self.device:
            raise ValueError(f'gt must be float32 {(B, C, H, W)} on {self.device}, got {gt.dtype} {tuple(gt.shape)} on {gt.device}')
        ws = self._recloss_ws.get((B, H, W))
        if ws is None:
            need = int(self.lib.lg_recloss_workspace_bytes(B, C, H, W))
            if need == 0:
                raise ValueError(f'the SAM / SSIM losses take C = 4 or 8 and W a multiple of 4 (got C = {C}, {H} x {W})')
            ws = self._recloss_ws[(B, H, W)] = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        if w_sam != 0.0:
            check(self.lib.lg_sam_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(self._sam), B, B * self.world, C, H, W, w_sam, int(bool(accumulate)),
                                       _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_sam_loss')
            accumulate = True
        if w_ssim != 0.0:
            check(self.lib.lg_ssim_loss(_ptr(out), _ptr(gt), _ptr(dout), _ptr(self._ssim), B, B * self.world, C, H, W, w_ssim, data_range,
                                        int(bool(accumulate)), _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_ssim_loss')
        self._recloss_last = dict(dout=dout)

    def _qnr_loss(self, out, pan, ms, pan_l, dout, scale, accumulate):
        """dout (+)= scale * d(1 - QNR)/d out and `_noref` += this rank's share of the loss: lg_qnr_stats, the SUM all-reduce of the
        table on the engine's process group (issued here, not through GradBuckets: it is no gradient bucket), lg_qnr_grad.  The signs in
        the gradient are those of the GLOBAL batch means, which is why the table travels and not the gradient.  No host synchronisation."""
        B, C, H, W = out.shape
        if pan_l.dim() != 4 or tuple(pan_l.shape) != (B, 1, H // 4, W // 4) or pan_l.dtype != torch.float32 or pan_l.device != self.device:
            raise ValueError(f"pan_l (the batch's 'input_pan_l') must be float32 [B,1,h,w] = {(B, 1, H // 4, W // 4)} on {self.device}, got "
                             f'{pan_l.dtype} {tuple(pan_l.shape)} on {pan_l.device}')
        pan_l = _aligned(pan_l)
        bufs = self._qnr_bufs.get((B, H, W))
        if bufs is None:
            need = int(self.lib.lg_qnr_workspace_bytes(B, C, H, W))
            if need == 0:
                raise ValueError(f'the QNR loss takes C = 4 or 8 and H, W multiples of 4, at least 8 (got C = {C}, {H} x {W})')
            P = C * (C - 1) // 2 + C
            bufs = (torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device),
                    torch.empty(P, dtype=torch.float64, device=self.device), torch.empty(3, dtype=torch.float64, device=self.device))
            self._qnr_bufs[(B, H, W)] = bufs
        ws, table, indices = bufs
        check(self.lib.lg_qnr_stats(_ptr(out), _ptr(pan), _ptr(ms), _ptr(pan_l), None, _ptr(table), B, C, H, W, _ptr(ws), ws.numel() * 8,
                                    _stream_ptr()), 'lg_qnr_stats')
        if self.world > 1 or self.force_collectives:
            import torch.distributed as dist
            dist.all_reduce(table, op=dist.ReduceOp.SUM, group=self.process_group)
        check(self.lib.lg_qnr_grad(_ptr(out), _ptr(pan), _ptr(table), _ptr(dout), _ptr(self._noref), _ptr(indices), B, B * self.world, C, H, W,
                                   float(scale), int(bool(accumulate)), _ptr(ws), ws.numel() * 8, _stream_ptr()), 'lg_qnr_grad')
        self._qnr_last = dict(table=table, indices=indices, dout=dout)

    def grad_norm(self, max_norm):
        """lg_grad_norm over the live ranges of the gradient buffer into the engine's [norm, clip coefficient] pair on the device (no host
        sync); returns that pair"""
        if self._clip is None:
            self._clip = torch.zeros(2, dtype=torch.float32, device=self.device)
        n = len(self.live_ranges)
        need = int(self.lib.lg_grad_norm_workspace_bytes(n, self.max_range))
        if self._norm_ws is None or self._norm_ws.numel() * 8 < need:
            self._norm_ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        check(self.lib.lg_grad_norm(_ptr(self.gflat), _ptr(self.ranges_dev), n, self.max_range, float(max_norm), _ptr(self._clip),
                                    _ptr(self._norm_ws), self._norm_ws.numel() * 8, _stream_ptr()), 'lg_grad_norm')
        return self._clip

    def last_grad_norm(self):
        """the global gradient norm the last clipped optimizer step saw, before clipping, as a Python float (host sync: for logging only)"""
        if self._clip is None:
            raise RuntimeError('no gradient norm yet: it is taken by train_step when the optimizer has controls with max_grad_norm '
                               '(optimizer.set_controls(TrainControls(max_grad_norm=...)) or cfg.train_cfg)')
        return float(self._clip[0].item())

    def _ema_of(self, optim):
        optim = self._optim if optim is None else optim
        ctl = getattr(optim, 'controls', None)
        if ctl is None or ctl.ema_decay is None:
            raise RuntimeError('no averaged weights: the optimizer has no controls with ema_decay (optimizer.set_controls(TrainControls('
                               'ema_decay=...)) or cfg.train_cfg); pass the optimizer if it has not stepped this engine yet')
        ema = (optim._state or {}).get('ema')
        if ema is None:
            return None                    # no optimizer step yet: the average IS the weights
        if ema.numel() != self.total:
            raise RuntimeError(f"the optimizer's 'ema' state holds {ema.numel()} floats, this engine {self.total}")
        return ema

    @contextlib.contextmanager
    def ema_weights(self, optim=None):
        """inside the block the flat parameter storage (and so every nn.Parameter, state_dict() and forward) holds the averaged weights of
        `optim` (default: the optimizer of the last train_step); the raw weights are put back on exit, also after an exception"""
        ema = self._ema_of(optim)
        if ema is None:
            yield self
            return
        raw = self.flat.clone()
        self.flat.copy_(ema)               # a restored (host) state is copied up here
        try:
            yield self
        finally:
            self.flat.copy_(raw)

    def _dead_forward(self, saved, flags, seed):
        """the dead-stage LGT forwards of a LG_FLAG_DEFER_DEAD forward, on the side stream: ordered behind everything enqueued so far
        (the LGT backward has read the saved activations they overwrite), concurrent with what the caller enqueues next"""
        plan, ws, _, _, B = saved[:5]
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
        side = self._side_stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            check(self.lib.lgteun_dead_forward(plan, _ptr(self.flat), _ptr(ws), ws.numel(), B, flags, seed, _stream_ptr()),
                  'lgteun_dead_forward')

    def adam(self, state, step, lr, betas, eps, grad_scale=1.0):
        check(self.lib.lg_adam_step(_ptr(self.flat), _ptr(self.gflat), _ptr(state['exp_avg']), _ptr(state['exp_avg_sq']),
                                    _ptr(self.ranges_dev), len(self.live_ranges), self.max_range, step, float(lr),
                                    float(betas[0]), float(betas[1]), float(eps), float(grad_scale), _stream_ptr()),
              'lg_adam_step')

    def optim_step(self, states, step, algo, flags, lr, h0, h1, eps, weight_decay, grad_scale=1.0):
        """lg_optim_step over the live ranges.  states: the three state slots of include/lgteun_hip.h (None: not used by the option set)"""
        s0, s1, s2 = (None if t is None else _ptr(t) for t in states)
        check(self.lib.lg_optim_step(_ptr(self.flat), _ptr(self.gflat), s0, s1, s2, _ptr(self.ranges_dev), len(self.live_ranges),
                                     self.max_range, step, int(algo), int(flags), float(lr), float(h0), float(h1), float(eps),
                                     float(weight_decay), float(grad_scale), _stream_ptr()), 'lg_optim_step')

    def optim_step_ex(self, states, step, algo, flags, lr, h0, h1, eps, weight_decay, clip=False, ema=None, ema_decay=0.0, plain_adam=False,
                      grad_scale=1.0):
        """lg_optim_step_ex over the live ranges.  clip: read the coefficient the last grad_norm() left on the device; ema: the average to
        update in the same launch; plain_adam: lg_adam_step's arithmetic"""
        s0, s1, s2 = (None if t is None else _ptr(t) for t in states)
        check(self.lib.lg_optim_step_ex(_ptr(self.flat), _ptr(self.gflat), s0, s1, s2, _ptr(self.ranges_dev), len(self.live_ranges),
                                        self.max_range, step, int(algo), int(flags), float(lr), float(h0), float(h1), float(eps),
                                        float(weight_decay), float(grad_scale),
                                        ctypes.c_void_p(self._clip.data_ptr() + 4) if clip else None, None if ema is None else _ptr(ema),
                                        float(ema_decay), int(plain_adam), _stream_ptr()), 'lg_optim_step_ex')


class _WsLease:
    """holds one training workspace for the lifetime of an autograd graph; gives it back to the engine's pool afterwards"""

    def __init__(self, ws, pool):
        self.ws, self._pool = ws, pool

    def __del__(self):
        try:
            if not self._pool:             # one spare buffer per (plan, B, train); extras go back to the allocator
                self._pool.append(self.ws)
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class _LgteunFn(torch.autograd.Function):
    """autograd bridge for callers that use torch optimizers / losses on the module output."""

    @staticmethod
    def forward(ctx, engine, ms, pan, flags, *live):
        engine._check_attached()
        seed = engine.next_seed() if (flags & LG_FLAG_DROPOUT) else 0
        out, saved = engine.forward_raw(ms, pan, flags | LG_FLAG_SAVE, seed, lease=True)   # this graph's own activations
        ctx.engine, ctx.saved, ctx.flags, ctx.seed = engine, saved, flags | LG_FLAG_SAVE, seed
        ctx.live_idx = list(engine.live_idx)    # the mode may change before backward runs
        return out

    @staticmethod
    def backward(ctx, dout):
        eng = ctx.engine
        g = torch.zeros(eng.total, dtype=torch.float32, device=eng.device)
        eng.backward_raw(ctx.saved, dout, g, ctx.flags, ctx.seed)
        if eng.world > 1:
            # the caller's loss is this rank's local mean: average over ranks like torch DDP does
            eng.buckets[bool(ctx.flags & LG_FLAG_CHAINED)].all_reduce(g)
            g.div_(eng.world)
        grads = []
        for i in ctx.live_idx:
            p = eng.params[i]
            o = eng.offsets[i]
            grads.append(g[o:o + p.numel()].view(p.shape))
        return (None, None, None, None, *grads)


class _FusedOptimizer(torch.optim.Optimizer):
    """what the fused optimizers share: a torch.optim.Optimizer (so lr_scheduler.StepLR, base_model.py:137-147, drives
    `param_groups[0]['lr']`, and the options sit in `param_groups[0]` under torch's names) whose step is ONE HIP launch over the flat
    live ranges.  Dead-stage parameters have no gradient in the reference, and torch skips those: no weight decay, no state -- the
    launch covers `engine.live_ranges` only.  State: flat fp32 buffers of `engine.total` floats, only those the option set needs."""
    is_fused_lgteun = True
    TORCH_NAME = None                  # the torch.optim class whose arithmetic this is, and which `fused=False` selects

    def __init__(self, params, defaults, unknown):
        if unknown:
            raise TypeError(f'{type(self).__name__} got unexpected keyword argument(s) {sorted(unknown)}: the fused step takes '
                            f'{sorted(defaults)} only; put fused=False into the optim_cfg entry to use torch.optim.{self.TORCH_NAME}, '
                            'which takes them')
        super().__init__(list(params), defaults)
        self._step = 0
        self._state = None
        self.dropout = True
        self.controls = None           # TrainControls (set_controls); None: the step every earlier build took
        self._window_pos = 0           # train_step calls of the current accumulation window already made
        self._window_gbuf = None       # ... and the engine's gradient + loss buffer they filled (what a checkpoint inside a window saves)

    def set_controls(self, controls):
        """attach a TrainControls (or None: none).  Not a constructor option: the constructors take torch's keywords only."""
        if controls is not None and not isinstance(controls, TrainControls):
            raise ValueError(f'set_controls takes a TrainControls or None (got {type(controls).__name__}); build one with '
                             'TrainControls(**cfg.train_cfg)')
        self.controls = controls
        self._window_pos, self._window_gbuf = 0, None
        return self

    def _ema_on(self):
        return self.controls is not None and self.controls.ema_decay is not None

    def _ex_on(self):
        """the step goes through lg_optim_step_ex: a control that the optimizer LAUNCH carries is on (accumulate alone is not one)"""
        return self.controls is not None and (self.controls.max_grad_norm is not None or self.controls.ema_decay is not None)

    def state_names(self):
        """the state buffers of this option set, in the order of lg_optim_step's state0 / state1 / state2 slots (None: unused)"""
        raise NotImplementedError

    def _launch(self, engine, group, state):
        raise NotImplementedError

    def step_flat(self, engine):
        names = [n for n in self.state_names() if n is not None]
        st = self._state
        ema = None
        if st is not None and 'ema' in st:     # the average is kept beside the algorithm's buffers, not one of them
            st = dict(st)
            ema = st.pop('ema')
        if st is None or set(st) != set(names) or any(v.numel() != engine.total for v in st.values()):
            st = {n: torch.zeros_like(engine.flat) for n in names}
        elif any(v.device != engine.flat.device or not v.is_contiguous() for v in st.values()):
            # state restored from a checkpoint (loaded to the host): the kernel takes device pointers
            st = {k: v.to(engine.flat.device).contiguous() for k, v in st.items()}
        if self._ema_on():
            if ema is None or ema.numel() != engine.total:
                ema = engine.flat.detach().clone()     # a full copy: dead-stage slots equal the weights, and stay so
            elif ema.device != engine.flat.device or not ema.is_contiguous():
                ema = ema.to(engine.flat.device).contiguous()
            st['ema'] = ema
        self._state = st
        self._step += 1
        self._launch(engine, self.param_groups[0], st)

    def step(self, closure=None):   # pragma: no cover - the fused path goes through Engine.train_step
        raise RuntimeError(f'{type(self).__name__} is stepped by Engine.train_step(); use torch.optim.{self.TORCH_NAME} '
                           '(fused=False in the optim_cfg entry) for the autograd path')

    def state_dict(self):
        sd = super().state_dict()
        sd['lgteun'] = dict(step=self._step, state=self._state)
        if self.controls is not None:          # without controls: exactly the keys of every earlier checkpoint
            sd['lgteun']['window'] = dict(pos=self._window_pos, accumulate=self.controls.accumulate,
                                          gbuf=None if self._window_pos == 0 or self._window_gbuf is None else self._window_gbuf.detach().clone())
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)                   # the caller's dict stays as it was
        extra = sd.pop('lgteun', None)
        super().load_state_dict(sd)
        for group in self.param_groups:     # a checkpoint written before an option existed (torch's classes do this in __setstate__)
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        if extra is not None:
            self._step, self._state = extra['step'], extra['state']
            win = extra.get('window')          # absent: a checkpoint written without controls -- it ended on a window boundary
            acc = self.controls.accumulate if self.controls is not None else 1
            if win is not None and win['pos'] > 0 and (win['accumulate'] != acc or win['gbuf'] is None):
                raise ValueError(f"the checkpoint was written {win['pos']} call(s) into an accumulation window of {win['accumulate']}; "
                                 f'this optimizer accumulates {acc}: resume with train_cfg accumulate={win["accumulate"]}, or from a '
                                 'checkpoint written at a window boundary')
            self._window_pos = win['pos'] if win is not None else 0
            self._window_gbuf = win['gbuf'] if self._window_pos else None

    def _optim_step(self, engine, state, algo, flags, lr, h0, h1, eps, weight_decay, plain_adam=False):
        states = [state.get(n) if n is not None else None for n in self.state_names()]
        if not self._ex_on():
            engine.optim_step(states, self._step, algo, flags, lr, h0, h1, eps, weight_decay)
            return
        c = self.controls
        engine.optim_step_ex(states, self._step, algo, flags, lr, h0, h1, eps, weight_decay, clip=c.max_grad_norm is not None,
                             ema=state.get('ema'), ema_decay=c.ema_decay or 0.0, plain_adam=plain_adam)


def _check_adam_args(lr, betas, eps, weight_decay):
    """torch/optim/adam.py's argument checks"""
    if not 0.0 <= lr:
        raise ValueError(f'Invalid learning rate: {lr}')
    if not 0.0 <= eps:
        raise ValueError(f'Invalid epsilon value: {eps}')
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f'Invalid beta parameter at index 0: {betas[0]}')
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f'Invalid beta parameter at index 1: {betas[1]}')
    if not 0.0 <= weight_decay:
        raise ValueError(f'Invalid weight_decay value: {weight_decay}')


class FusedAdam(_FusedOptimizer):
    """torch.optim.Adam semantics (reference models/base/base_model.py:123-124) as one HIP launch over the flat live ranges;
    `weight_decay` is torch's L2 term (added to the gradient), `amsgrad` keeps the running maximum of exp_avg_sq in a third buffer.
    The plain option set (no weight decay, no amsgrad) is `lg_adam_step`, every other one an instance of `lg_optim_step`."""
    TORCH_NAME = 'Adam'
    ALGO = _lib.LG_OPT_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **unknown):
        _check_adam_args(lr, betas, eps, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad), unknown)

    def state_names(self):
        return ['exp_avg', 'exp_avg_sq', 'max_exp_avg_sq' if self.param_groups[0]['amsgrad'] else None]

    def _launch(self, engine, g, state):
        if self.ALGO == _lib.LG_OPT_ADAM and not g['weight_decay'] and not g['amsgrad']:
            if self._ex_on():              # lg_adam_step's arithmetic with the controls in the launch: the run stays on its bits
                self._optim_step(engine, state, self.ALGO, 0, g['lr'], g['betas'][0], g['betas'][1], g['eps'], 0.0, plain_adam=True)
            else:
                engine.adam(state, self._step, g['lr'], g['betas'], g['eps'])
        else:
            self._optim_step(engine, state, self.ALGO, _lib.LG_OPT_AMSGRAD if g['amsgrad'] else 0, g['lr'], g['betas'][0], g['betas'][1],
                             g['eps'], g['weight_decay'])


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW (base_model.py:129-130): the decay is decoupled, p <- p (1 - lr weight_decay) ahead of the Adam update"""
    TORCH_NAME = 'AdamW'
    ALGO = _lib.LG_OPT_ADAMW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, **unknown):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **unknown)


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD (base_model.py:127-128) with momentum, dampening, nesterov and weight_decay (L2).  Like torch's, the momentum
    buffer of the first step is the gradient itself."""
    TORCH_NAME = 'SGD'

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **unknown):
        if lr < 0.0:
            raise ValueError(f'Invalid learning rate: {lr}')
        if momentum < 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if weight_decay < 0.0:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov),
                         unknown)

    def state_names(self):
        return ['momentum_buffer' if self.param_groups[0]['momentum'] != 0 else None, None, None]

    def _launch(self, engine, g, state):
        self._optim_step(engine, state, _lib.LG_OPT_SGD, _lib.LG_OPT_NESTEROV if g['nesterov'] else 0, g['lr'], g['momentum'],
                         g['dampening'], 0.0, g['weight_decay'])


class FusedRMSprop(_FusedOptimizer):
    """torch.optim.RMSprop (base_model.py:125-126) with alpha, eps (added after the square root), weight_decay (L2), momentum and
    centered"""
    TORCH_NAME = 'RMSprop'

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0, momentum=0, centered=False, **unknown):
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= momentum:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if not 0.0 <= alpha:
            raise ValueError(f'Invalid alpha value: {alpha}')
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=weight_decay, momentum=momentum, centered=centered),
                         unknown)

    def state_names(self):
        g = self.param_groups[0]
        return ['square_avg', 'momentum_buffer' if g['momentum'] > 0 else None, 'grad_avg' if g['centered'] else None]

    def _launch(self, engine, g, state):
        self._optim_step(engine, state, _lib.LG_OPT_RMSPROP, _lib.LG_OPT_CENTERED if g['centered'] else 0, g['lr'], g['alpha'],
                         g['momentum'], g['eps'], g['weight_decay'])


FUSED_OPTIMIZERS = {'Adam': FusedAdam, 'AdamW': FusedAdamW, 'SGD': FusedSGD, 'RMSprop': FusedRMSprop}
