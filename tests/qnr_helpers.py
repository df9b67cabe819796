"""Shared by tests/test_qnr_loss_cpu.py, tests/test_gpu_qnr_loss.py and tests/ddp_qnr_worker.py: the fp64 restatement of the
no-reference loss 1 - QNR and of its gradient, written from the definitions (Wang-Bovik Q over the whole image of a sample, Alparone's
D_lambda / D_s with p = q = 1, batch means of Q taken before the absolute value), the input recipe, and the entry condition.

Per sample n and pair (a, b), with E the mean over the sample's pixels:
    Q_n(a, b) = 4 cov E[a] E[b] / ((var_a + var_b) (E[a]^2 + E[b]^2) + 1e-8)
    d_ij = mean_n Q_n(x_i, x_j) - mean_n Q_n(ms_i, ms_j)   (i < j, row-major), then   d_iP = mean_n Q_n(x_i, pan) - mean_n Q_n(ms_i, pan_l)
    D_lambda = mean |d_ij|,  D_s = mean |d_iP|,  loss = 1 - (1 - D_lambda)(1 - D_s)
The gradient is alpha_ni + sum_j beta_nij x[n, j, p] + gamma_ni pan[n, p]: every moment is linear in the pixels."""
import numpy as np
import torch

MIN_ENTRY = 1e-3      # every |d| of a test's inputs is at least this: the sign is never in doubt (a condition on the inputs, not a tolerance)


def n_pairs(C):
    return C * (C - 1) // 2, C * (C - 1) // 2 + C


def pair_list(C):
    """(i, j) of the table's entries; j = -1: the PAN"""
    return [(i, j) for i in range(C) for j in range(i + 1, C)] + [(i, -1) for i in range(C)]


def make_inputs(B, C, H, W, seed):
    """the recipe of the tests: MS bands as gains of a common base plane plus noise, pan_l their mean plus noise, pan and out bilinear x4 of
    pan_l and ms plus noise; float32 tensors out [B,C,H,W], pan [B,1,H,W], ms [B,C,H/4,W/4], pan_l [B,1,H/4,W/4]"""
    g = torch.Generator().manual_seed(seed)
    h, w = H // 4, W // 4
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)            # noqa: E731
    nrm = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)           # noqa: E731
    base = rnd(B, 1, h, w)
    gain = torch.linspace(0.6, 1.4, C, dtype=torch.float64).view(1, C, 1, 1)
    ms = 0.25 + 0.5 * gain * base + 0.15 * nrm(B, C, h, w)
    pan_l = ms.mean(dim=1, keepdim=True) + 0.05 * nrm(B, 1, h, w)
    up = lambda t: torch.nn.functional.interpolate(t, scale_factor=4, mode='bilinear', align_corners=False)      # noqa: E731
    pan = up(pan_l) + 0.1 * nrm(B, 1, H, W)
    hc = torch.linspace(1.5, 0.5, C, dtype=torch.float64).view(1, C, 1, 1)
    out = up(ms) + 0.08 * hc * nrm(B, C, H, W)
    return tuple(t.float().contiguous() for t in (out, pan, ms, pan_l))


def _moments(a, b):
    """a, b [N, H, W] fp64 -> E[a], E[b], E[aa], E[bb], E[ab], each [N]"""
    ax = (1, 2)
    return a.mean(axis=ax), b.mean(axis=ax), (a * a).mean(axis=ax), (b * b).mean(axis=ax), (a * b).mean(axis=ax)


def q_and_derivs(a, b, eps=1e-8):
    """Q_n [N] and dQ_n / d(E[a], E[b], E[aa], E[bb], E[ab]) [5, N]"""
    ea, eb, eaa, ebb, eab = _moments(a, b)
    cov, V, E2 = eab - ea * eb, (eaa - ea * ea) + (ebb - eb * eb), ea * ea + eb * eb
    den = V * E2 + eps
    Q = 4 * cov * ea * eb / den
    dq = np.stack([(4 * eb * (cov - ea * eb) - Q * 2 * ea * (V - E2)) / den, (4 * ea * (cov - ea * eb) - Q * 2 * eb * (V - E2)) / den,
                   -Q * E2 / den, -Q * E2 / den, 4 * ea * eb / den])
    return Q, dq


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def stats_ref(out, pan, ms, pan_l):
    """fp64: q [N, 2, P] (fused side, MS side), table [P] = sum_n (Q_n,fused - Q_n,ms), dq [N, P, 5] of the fused side"""
    x, p, m, pl = _f64(out), _f64(pan)[:, 0], _f64(ms), _f64(pan_l)[:, 0]
    C = x.shape[1]
    q = np.zeros((x.shape[0], 2, n_pairs(C)[1]))
    dq = np.zeros((x.shape[0], n_pairs(C)[1], 5))
    for k, (i, j) in enumerate(pair_list(C)):
        Q, d = q_and_derivs(x[:, i], x[:, j] if j >= 0 else p)
        q[:, 0, k], dq[:, k] = Q, d.T
        q[:, 1, k] = q_and_derivs(m[:, i], m[:, j] if j >= 0 else pl)[0]
    table = np.zeros(q.shape[2])
    for n in range(q.shape[0]):            # n ascending, as the library sums
        table = table + (q[n, 0] - q[n, 1])
    return q, table, dq


def indices_ref(table, b_global, C):
    """D_lambda, D_s, loss from the (global) table"""
    npl = n_pairs(C)[0]
    d = np.abs(table / b_global)
    dl, ds = d[:npl].mean(), d[npl:].mean()
    return dl, ds, 1 - (1 - dl) * (1 - ds)


def grad_ref(out, pan, table, b_global, dq):
    """fp64 gradient of the loss wrt `out` [N, C, H, W] in the analytic form alpha + beta x + gamma pan, with sign(0) = 0; `table` is the
    global one, `dq` that of these samples (stats_ref)"""
    x, p = _f64(out), _f64(pan)[:, 0]
    N, C, H, W = x.shape
    npl = n_pairs(C)[0]
    dl, ds, _ = indices_ref(table, b_global, C)
    sg = np.sign(table / b_global)
    wt = np.where(np.arange(len(table)) < npl, sg * (1 - ds) / (npl * b_global), sg * (1 - dl) / (C * b_global))
    g = np.zeros_like(x)
    hw = H * W
    for k, (i, j) in enumerate(pair_list(C)):
        for n in range(N):
            da, db, daa, dbb, dab = dq[n, k]
            b = x[n, j] if j >= 0 else p[n]
            g[n, i] += wt[k] * (da + 2 * daa * x[n, i] + dab * b) / hw
            if j >= 0:
                g[n, j] += wt[k] * (db + 2 * dbb * x[n, j] + dab * x[n, i]) / hw
    return g


def reference(out, pan, ms, pan_l, b_global=None, table=None):
    """everything the tests compare against, for one rank's samples: dict(q, table, d, indices, grad).  `table` / `b_global`: the global
    ones under data parallelism (default: these samples are the batch).  Asserts the entry condition on d."""
    q, own, dq = stats_ref(out, pan, ms, pan_l)
    table = own if table is None else table
    b_global = out.shape[0] if b_global is None else b_global
    d = table / b_global
    assert np.abs(d).min() >= MIN_ENTRY, f'inputs do not meet the entry condition: min |d| = {np.abs(d).min():.3e}; pick another seed'
    return dict(q=q, own_table=own, table=table, d=d, indices=np.array(indices_ref(table, b_global, out.shape[1])),
                grad=grad_ref(out, pan, table, b_global, dq))
