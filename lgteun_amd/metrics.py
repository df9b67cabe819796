"""Reference-based image-quality indices of the evaluation loop, written from their published definitions.

    PSNR   10 log10(peak^2 / MSE)
    SAM    mean spectral angle between the pixel vectors of the two images            (Yuhas et al., 1992)
    ERGAS  100/ratio * sqrt(mean_band(MSE_band / mean_band^2))                         (Wald, 2000)
    SSIM   mean over windows of  l(x,y) * cs(x,y)  with Gaussian-weighted local moments   (Wang et al., 2004)
    Q      universal image quality index: SSIM with C1 = C2 = 0 on box windows          (Wang & Bovik, 2002)

Conventions the evaluation of reference `models/base/metrics.py` fixes, so that numbers are comparable with its tables
(`ref_evaluate`, metrics.py:409-417): arrays are (H, W) or (H, W, bands) in digital numbers, arithmetic in float64, peak
value 2047.5 (11-bit data); a multi-band SSIM / Q is the plain mean of the per-band values; SSIM uses an 11-tap Gaussian
(sigma 1.5) and Q an 8 x 8 box, and both average only over windows that lie fully inside the image; SAM is in radians with
the cosine clipped to [0, 1]; ERGAS uses ratio 4.

Parity status: every index of `ref_evaluate` and `no_ref_evaluate`, and `cc`, is pinned by values the reference itself produced
(tests/golden/net_*.npz `metrics` for PSNR / SAM / ERGAS; tests/golden/parity_metrics_*.npz for all of them, tests/test_reference_parity_cpu.py).
SSIM / Q call cv2.filter2D in the reference and cv2 is not installed, so the reference ran over three stand-ins for the OpenCV calls it
makes (tools/_ref_import.py).  Restricting the average to fully covered windows makes the result independent of any border
rule, and the generator proves that the reference never reads one.  Host against reference: PSNR, SAM, ERGAS, CC equal; SSIM 4e-15, Q 2e-14,
D_lambda 1.4e-13 relative.
The no-reference family of the full-resolution pass (`no_ref_evaluate`: D_lambda, D_s, QNR; Alparone et al., 2008): Q on 32 x 32 windows,
the PAN image brought to MS resolution by the reference's MTF low-pass (`mtf_window_filter`: the window method with the QuickBird PAN gain
0.15), replicated edges, then every fourth sample.  The low-pass is applied as its separable factor (`mtf_taps`, the row sums of the 2-D
filter); the rank-1 residual that drops is all that separates D_s and QNR from the reference's values: at most 8.9e-7 and 1.1e-8 relative
(gates 3.6e-6 and 4.5e-8).
Device versions for whole batches (fp64 HIP kernels, tested against these functions): lgteun_amd/device_metrics.py.
The extended set (`ref_evaluate_ext`, `no_ref_evaluate_ext`) adds the columns of the pan-sharpening literature: Q2n (Garzelli & Nencini, 2009:
Q4 for four bands, Q8 for eight), SCC (Zhou et al., 1998, on Sobel magnitudes), CC (the reference's `scc`, metrics.py:58: Pearson's r per band)
and D_lambda_K / HQNR (Khan et al., 2009; Aiazzi et al., 2014).  They are written from DESIGN.md 3.8.1, which is their definition here where it
differs from the MATLAB toolbox (two deviations, recorded there).
"""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

PEAK = 2047.5
_TINY = np.finfo(np.float64).eps
SSIM_TAPS, SSIM_SIGMA, Q_BLOCK, ERGAS_RATIO = 11, 1.5, 8, 4
QNR_BLOCK, MTF_TAPS, MTF_GAIN_PAN = 32, 41, 0.15


def _as_pair(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError(f'images differ in shape: {a.shape} vs {b.shape}')
    if a.ndim not in (2, 3):
        raise ValueError(f'expected an (H, W) or (H, W, bands) array, got {a.ndim} dimensions')
    return a.astype(np.float64), b.astype(np.float64)


def _band_mean(index, a, b, *args):
    """a per-band index averaged over the bands of (H, W, bands) inputs"""
    a, b = _as_pair(a, b)
    if a.ndim == 2:
        return float(index(a, b, *args))
    return float(np.mean([index(a[..., k], b[..., k], *args) for k in range(a.shape[2])]))


def gaussian_taps(n=SSIM_TAPS, sigma=SSIM_SIGMA):
    """n samples of a centred Gaussian, normalised to sum 1"""
    t = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
    g = np.exp(-0.5 * (t / sigma) ** 2)
    return g / g.sum()


def _inside_windows(img, taps):
    """separable weighted sum over every window position that lies fully inside `img`: (H, W) -> (H-n+1, W-n+1)"""
    rows = sliding_window_view(img, taps.size, axis=0) @ taps
    return sliding_window_view(rows, taps.size, axis=1) @ taps


def _local_moments(x, y, taps):
    """local means, variances and covariance under the window `taps` x `taps`"""
    mx, my = _inside_windows(x, taps), _inside_windows(y, taps)
    vx = _inside_windows(x * x, taps) - mx * mx
    vy = _inside_windows(y * y, taps) - my * my
    cxy = _inside_windows(x * y, taps) - mx * my
    return mx, my, vx, vy, cxy


def _ssim_band(x, y, peak):
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    mx, my, vx, vy, cxy = _local_moments(x, y, gaussian_taps())
    luminance = (2.0 * mx * my + c1) / (mx * mx + my * my + c1)
    structure = (2.0 * cxy + c2) / (vx + vy + c2)
    return (luminance * structure).mean()


def _q_band(x, y, block):
    if block < 2:
        raise ValueError('the Q index needs windows of at least 2 x 2 pixels')
    mx, my, vx, vy, cxy = _local_moments(x, y, np.full(block, 1.0 / block))
    energy, spread = mx * mx + my * my, vx + vy
    # a factor whose denominator vanishes (flat window / zero-mean window) is taken as 1, the value of identical inputs
    luminance = np.divide(2.0 * mx * my, energy, out=np.ones_like(energy), where=energy > 1e-8)
    structure = np.divide(2.0 * cxy, spread, out=np.ones_like(spread), where=spread > 1e-8)
    return (luminance * structure).mean()


def psnr(img1, img2, dynamic_range=PEAK):
    a, b = _as_pair(img1, img2)
    mse = np.mean(np.square(a - b))
    if mse <= 1e-10:                      # identical up to rounding: reported as infinite, like the reference's table code
        return np.inf
    return float(20.0 * np.log10(dynamic_range / (np.sqrt(mse) + _TINY)))


def sam(img1, img2):
    a, b = _as_pair(img1, img2)
    if a.ndim != 3 or a.shape[2] < 2:
        raise ValueError('the spectral angle needs at least two bands: (H, W, bands)')
    dot = np.einsum('hwc,hwc->hw', a, b)
    norms = np.linalg.norm(a, axis=2) * np.linalg.norm(b, axis=2)
    return float(np.arccos(np.clip(dot / (norms + _TINY), 0.0, 1.0)).mean())


def ergas(img_fake, img_real, scale=ERGAS_RATIO):
    fake, real = _as_pair(img_fake, img_real)
    if fake.ndim == 2:
        fake, real = fake[..., None], real[..., None]
    band_mse = np.square(fake - real).mean(axis=(0, 1))
    band_mean = real.mean(axis=(0, 1))
    return float(100.0 / scale * np.sqrt(np.mean(band_mse / (np.square(band_mean) + _TINY))))


def ssim(img1, img2, dynamic_range=PEAK):
    return _band_mean(_ssim_band, img1, img2, dynamic_range)


def qindex(img1, img2, block_size=Q_BLOCK):
    return _band_mean(_q_band, img1, img2, block_size)


def ref_evaluate(pred, gt):
    """the five reference-based indices in the order of the reference's result tables: PSNR, SSIM, Q, SAM, ERGAS"""
    return [psnr(pred, gt), ssim(pred, gt), qindex(pred, gt), sam(pred, gt), ergas(pred, gt)]


# ---------------------------------------------------------------------------------------------------------------------
# no-reference indices of the full-resolution pass (reference models/base/metrics.py:290-408, `no_ref_evaluate`)
# ---------------------------------------------------------------------------------------------------------------------
KAISER_BETA = 0.5


def _bessel_i0(x):
    """the modified Bessel function I0 by its power series sum_k ((x/2)^k / k!)^2: for the x <= 0.5 of the window 12 terms reach the last bit"""
    term, total = 1.0, 1.0
    for k in range(1, 25):
        term = term * (0.5 * x / k) * (0.5 * x / k)
        total = total + term
    return total


def mtf_window_filter(gain_at_nyquist, ratio=ERGAS_RATIO, n=MTF_TAPS):
    """the n x n MTF-matched low-pass of the reference's no-reference indices (its `GNyq2win`, models/base/metrics.py:223-235), designed
    by the window method:
      1. the wanted frequency response is a Gaussian sampled on the n x n DFT grid, G(k) = exp(-k^2 / (2 a^2)) for k = -(n-1)/2 .. (n-1)/2 in
         each direction, with a chosen so that a continuous Gaussian would have the value `gain_at_nyquist` at the coarse grid's Nyquist
         frequency, k = (n - 1) / (2 ratio);
      2. its inverse DFT, centred: separable, g(m) = 1/n sum_k G(k) cos(2 pi k m / n) per direction;
      3. times a radial Kaiser window (beta 0.5): the 1-D window of n samples over [-1/2, 1/2], read at the radius sqrt(i^2 + j^2) / (n - 1)
         by linear interpolation between its samples, zero beyond the radius 1/2;
      4. normalised to sum 1.
    The radial window is what keeps the filter from being exactly separable (second singular value 5.3e-6 of the first at gain 0.15)."""
    if not 0.0 < gain_at_nyquist < 1.0:
        raise ValueError('the MTF gain at Nyquist lies in (0, 1)')
    if n < 3 or n % 2 == 0:
        raise ValueError('the window method is written for an odd number of taps >= 3')
    half = n // 2
    k = np.arange(-half, half + 1, dtype=np.float64)
    alpha = np.sqrt(((n - 1) * (0.5 / ratio)) ** 2 / (-2.0 * np.log(gain_at_nyquist)))
    resp = np.exp(-0.5 * (k / alpha) ** 2)
    g = np.array([np.sum(resp * np.cos(2.0 * np.pi * k * m / n)) for m in k]) / n
    i0_beta = _bessel_i0(KAISER_BETA)
    kaiser = np.array([_bessel_i0(KAISER_BETA * np.sqrt(1.0 - (j / half) ** 2)) / i0_beta for j in range(half + 1)])   # by distance from the centre
    t = k / (n - 1.0)
    radius = np.sqrt(t[:, None] * t[:, None] + t[None, :] * t[None, :])
    x = radius * (n - 1.0)
    lo = np.minimum(x.astype(np.int64), half - 1)
    window = kaiser[lo] + (x - lo) * (kaiser[lo + 1] - kaiser[lo])
    window[radius > t[-1]] = 0.0
    h = np.outer(g, g) * window
    return h / h.sum()


def mtf_taps(gain_at_nyquist, ratio=ERGAS_RATIO, n=MTF_TAPS):
    """the separable factor of `mtf_window_filter`: the row sums of the 2-D filter, n taps that sum to 1.  outer(taps, taps) is the 2-D
    filter up to its rank-1 residual (DESIGN.md 3.8 has the measured figures).  The design puts `gain_at_nyquist` on DFT bin
    (n - 1) / (2 ratio) of an n-point grid, that is at (n - 1) / (2 ratio n) cycles per fine pixel, not at the coarse grid's Nyquist frequency
    1 / (2 ratio) itself: for 0.15, ratio 4 and 41 taps the gain is 0.1506 at 5/41 and 0.1368 at 1/8.  That is the reference's filter, kept as it is"""
    return mtf_window_filter(gain_at_nyquist, ratio, n).sum(axis=1)


def mtf_degrade(img, gain_at_nyquist=MTF_GAIN_PAN, ratio=ERGAS_RATIO):
    """(H, W[, bands]) -> (H / ratio, W / ratio[, bands]): separable MTF-matched low-pass (edges replicated), then every ratio-th sample"""
    x = np.asarray(img, dtype=np.float64)
    taps = mtf_taps(gain_at_nyquist, ratio)
    half = taps.size // 2
    pad = [(half, half), (half, half)] + [(0, 0)] * (x.ndim - 2)
    xp = np.pad(x, pad, mode='edge')
    rows = np.tensordot(sliding_window_view(xp, taps.size, axis=0), taps, axes=([-1], [0]))
    full = np.tensordot(sliding_window_view(rows, taps.size, axis=1), taps, axes=([-1], [0]))
    return full[::ratio, ::ratio]


def d_lambda(fused, ms, block_size=QNR_BLOCK, p=1):
    """spectral distortion: how much the inter-band Q indices of the fused image differ from those of the MS image,
    ( mean over band pairs l < r of |Q(F_l, F_r) - Q(M_l, M_r)|^p )^(1/p)"""
    f, m = np.asarray(fused, np.float64), np.asarray(ms, np.float64)
    if f.ndim != 3 or m.ndim != 3 or f.shape[2] != m.shape[2] or f.shape[2] < 2:
        raise ValueError('fused and MS images are (H, W, bands) with the same number (>= 2) of bands')
    nb = f.shape[2]
    bs_m = min(block_size, min(m.shape[:2]))
    diffs = [abs(_q_band(f[..., l], f[..., r], block_size) - _q_band(m[..., l], m[..., r], bs_m)) ** p
             for l in range(nb) for r in range(l + 1, nb)]
    return float(np.mean(diffs) ** (1.0 / p))


def d_s(fused, ms, pan, pan_lr=None, block_size=QNR_BLOCK, q=1, ratio=ERGAS_RATIO, gain_at_nyquist=MTF_GAIN_PAN):
    """spatial distortion: ( mean over bands of |Q(F_l, P) - Q(M_l, P_lr)|^q )^(1/q); P_lr = the PAN image at MS resolution
    (MTF-matched low-pass + decimation unless given)"""
    f, m, pn = np.asarray(fused, np.float64), np.asarray(ms, np.float64), np.asarray(pan, np.float64).squeeze()
    if pn.ndim != 2 or f.shape[:2] != pn.shape:
        raise ValueError('PAN is (H, W) at the fused image\'s resolution')
    plr = mtf_degrade(pn, gain_at_nyquist, ratio) if pan_lr is None else np.asarray(pan_lr, np.float64).squeeze()
    if plr.shape != m.shape[:2]:
        raise ValueError(f'low-resolution PAN {plr.shape} does not match the MS image {m.shape[:2]}')
    bs_lr = min(block_size, min(plr.shape))        # the reference's tables use the SAME window at both resolutions (metrics.py:325,329)
    diffs = [abs(_q_band(f[..., l], pn, block_size) - _q_band(m[..., l], plr, bs_lr)) ** q for l in range(f.shape[2])]
    return float(np.mean(diffs) ** (1.0 / q))


def qnr(fused, ms, pan, pan_lr=None, alpha=1, beta=1, **kw):
    """quality with no reference: (1 - D_lambda)^alpha (1 - D_s)^beta, 1 for a fusion without spectral or spatial distortion"""
    return float((1.0 - d_lambda(fused, ms, kw.get('block_size', QNR_BLOCK))) ** alpha * (1.0 - d_s(fused, ms, pan, pan_lr, **kw)) ** beta)


def no_ref_evaluate(pred, pan, ms):
    """the three no-reference indices in the order of the reference's result tables: D_lambda, D_s, QNR"""
    dl, ds = d_lambda(pred, ms), d_s(pred, ms, pan)
    return [dl, ds, (1.0 - dl) * (1.0 - ds)]


# ---------------------------------------------------------------------------------------------------------------------
# the extended set: Q2n, SCC, CC at reduced resolution, D_lambda_K and HQNR at full resolution (definitions: DESIGN.md 3.8.1)
# ---------------------------------------------------------------------------------------------------------------------
Q2N_BLOCK, Q2N_MAX_BANDS = 32, 8


def hconj(a):
    """the hypercomplex conjugate: every component but the first negated (components on the last axis)"""
    a = np.asarray(a, np.float64)
    return np.concatenate([a[..., :1], -a[..., 1:]], axis=-1)


def hmul(x, y):
    """the hypercomplex product of vectors of length N = 2^m on the last axis (N = 1: the plain product); with halves x = (a, b) and
    y = (c, d):  x * y = ( a*c - conj(d)*b , conj(a)*conj(d) + c*conj(b) )"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[-1]
    if n != y.shape[-1] or n < 1 or n & (n - 1):
        raise ValueError(f'the hypercomplex product takes two vectors of one power-of-two length (got {x.shape[-1]} and {y.shape[-1]})')
    if n == 1:
        return x * y
    a, b, c, d = x[..., :n // 2], x[..., n // 2:], y[..., :n // 2], y[..., n // 2:]
    return np.concatenate([hmul(a, c) - hmul(hconj(d), b), hmul(hconj(a), hconj(d)) + hmul(c, hconj(b))], axis=-1)


def _block_sum(v):
    """the sum over the 1024 pixels of a block (first axis, row-major) as ONE fixed tree of pairwise additions -- the tree of the device
    kernel (k_iqa_q2n: pixel p belongs to thread p % 256, which adds its four; lanes halve inside a wave; the four waves meet pairwise).
    A tree of halvings adds 1024 equal values exactly, whatever their bits: a block that is flat in both images has P2 = M2 to the
    last bit and reaches the t3 == 0 branch.  np.sum, which runs eight sequential accumulators, forms 3 v and may round."""
    v = v.reshape((4, 4, 64) + v.shape[1:])
    v = (v[0] + v[1]) + (v[2] + v[3])
    for half in (32, 16, 8, 4, 2, 1):
        v = v[:, :half] + v[:, half:2 * half]
    return ((v[0] + v[1]) + (v[2] + v[3]))[0]


def _q2n_block(x, y):
    """one block: x (ground truth), y (fused) as [1024, N] float64, bands past the image's own are zero"""
    n, N = x.shape
    k = n / (n - 1.0)
    a = _block_sum(x) / n
    d = x - a
    c = np.sqrt(_block_sum(d * d) / (n - 1.0))
    c = np.where(c == 0.0, 1.0, c)            # a flat block keeps its scale (the toolbox divides by eps here: DESIGN.md 3.8.1)
    xn = d / c + 1.0
    z = (y - a) / c + 1.0                     # the ground truth's map on both images
    z[:, 1:] = -z[:, 1:]
    m1, m2 = _block_sum(xn) / n, _block_sum(z) / n
    sq1, sq2 = np.zeros(n), np.zeros(n)
    M1 = M2 = 0.0
    for i in range(N):                        # ascending band order, as the kernel adds them
        sq1, sq2 = sq1 + xn[:, i] * xn[:, i], sq2 + z[:, i] * z[:, i]
        M1, M2 = M1 + m1[i] * m1[i], M2 + m2[i] * m2[i]
    P1, P2 = _block_sum(sq1) / n, _block_sum(sq2) / n
    t3 = k * P1 + k * P2 - k * (M1 + M2)
    bias = 2.0 * np.sqrt(M1) * np.sqrt(M2) / (M1 + M2)
    if t3 == 0.0:
        return abs(bias)
    u = _block_sum(hmul(xn, z)) / n
    q = (k * u - k * hmul(m1, m2)) * bias * (2.0 / t3)
    s = 0.0
    for i in range(N):
        s = s + q[i] * q[i]
    return float(np.sqrt(s))


def _q2n_planes(gt, fused):
    """-> the two images as float64 [H', W', N]: bands padded with zero planes to N = 2^m, sides mirrored (edge included) to multiples of 32"""
    g, f = _as_pair(gt, fused)
    if g.ndim != 3 or not 2 <= g.shape[2] <= Q2N_MAX_BANDS:
        raise ValueError(f'Q2n takes (H, W, bands) images of 2 .. {Q2N_MAX_BANDS} bands (got shape {g.shape})')
    if min(g.shape[:2]) < Q2N_BLOCK:
        raise ValueError(f'Q2n needs H and W >= {Q2N_BLOCK}, one block (got {g.shape[0]} x {g.shape[1]})')
    N = 1 << (g.shape[2] - 1).bit_length()
    out = []
    for v in (g, f):
        v = np.concatenate([v, np.zeros(v.shape[:2] + (N - v.shape[2],))], axis=2)
        e = -v.shape[0] % Q2N_BLOCK
        if e:
            v = np.concatenate([v, v[:-e - 1:-1]], axis=0)          # lines L-1, L-2, ..., L-e: rows first
        e = -v.shape[1] % Q2N_BLOCK
        if e:
            v = np.concatenate([v, v[:, :-e - 1:-1]], axis=1)
        out.append(v)
    return out


def q2n_blocks(gt, fused):
    """the Q2n value of every 32 x 32 block of the extended image, row-major"""
    g, f = _q2n_planes(gt, fused)
    bs, N = Q2N_BLOCK, g.shape[2]
    return np.array([_q2n_block(g[r:r + bs, c:c + bs].reshape(-1, N), f[r:r + bs, c:c + bs].reshape(-1, N))
                     for r in range(0, g.shape[0], bs) for c in range(0, g.shape[1], bs)])


def q2n(gt, fused, block=Q2N_BLOCK):
    """Q2n, the hypercomplex extension of Q to 2 .. 8 bands (Q4, Q8): the mean over non-overlapping 32 x 32 blocks"""
    if block != Q2N_BLOCK:
        raise ValueError(f'Q2n is defined here on {Q2N_BLOCK} x {Q2N_BLOCK} blocks (got block = {block})')
    return float(np.mean(q2n_blocks(gt, fused)))


def _sobel_magnitude(x):
    """(H, W, bands) -> (H-2, W-2, bands): sqrt(gx^2 + gy^2) of the Sobel pair at the interior pixels, no padding"""
    gx = (x[:-2, 2:] - x[:-2, :-2]) + 2.0 * (x[1:-1, 2:] - x[1:-1, :-2]) + (x[2:, 2:] - x[2:, :-2])
    gy = (x[2:, :-2] - x[:-2, :-2]) + 2.0 * (x[2:, 1:-1] - x[:-2, 1:-1]) + (x[2:, 2:] - x[:-2, 2:])
    return np.sqrt(gx * gx + gy * gy)


def scc(gt, fused):
    """spatial correlation: sum FG / sqrt(sum F^2 sum G^2) of the Sobel magnitudes F (fused) and G (ground truth) over all bands; 1 when
    neither image has an edge, 0 when exactly one has none"""
    g, f = _as_pair(gt, fused)
    if g.ndim == 2:
        g, f = g[..., None], f[..., None]
    if min(g.shape[:2]) < 3:
        raise ValueError('SCC needs H and W >= 3 (one interior pixel)')
    F, G = _sobel_magnitude(f), _sobel_magnitude(g)
    ff, gg = float(np.sum(F * F)), float(np.sum(G * G))
    if ff == 0.0 or gg == 0.0:
        return 1.0 if ff == gg else 0.0
    return float(np.sum(F * G) / np.sqrt(ff * gg))


def cc(gt, fused):
    """the reference's `scc` (models/base/metrics.py:58): the mean over bands of Pearson's r; NaN if a band of either image is constant"""
    g, f = _as_pair(gt, fused)
    if g.ndim == 2:
        g, f = g[..., None], f[..., None]
    rs = []
    for k in range(g.shape[2]):
        x, y = g[..., k].ravel(), f[..., k].ravel()
        rs.append(np.nan if x.min() == x.max() or y.min() == y.max() else np.corrcoef(x, y)[0, 1])
    return float(np.mean(rs))


def fir_decimate4(x, taps, phase=2):
    """the arithmetic lg_fir_decimate4 documents (include/lgteun_hip.h), on the host: (H, W) float32 samples -> float32 (H/4, W/4).  fp64; the
    pass along the rows, then the pass along the columns, replicate borders, each sum in ascending k from 0.0, one rounding to fp32"""
    x, taps = np.asarray(x), np.asarray(taps, np.float64)
    H, W = x.shape
    if H % 4 or W % 4:
        raise ValueError(f'decimation by 4 needs sides that are multiples of 4 (got {H} x {W})')
    r = taps.size // 2
    xp = np.pad(x.astype(np.float64), r, mode='edge')
    rows = np.zeros((H + 2 * r, W // 4))
    for k in range(taps.size):
        rows = rows + taps[k] * xp[:, phase + k::4][:, :W // 4]
    out = np.zeros((H // 4, W // 4))
    for k in range(taps.size):
        out = out + taps[k] * rows[phase + k::4][:H // 4]
    return out.astype(np.float32)


def mtf_degrade_ms(fused, gains_ms=None, n_taps=MTF_TAPS, phase=2):
    """every band of the fused image (H, W, bands; float32 samples) through its MTF-matched Gaussian (wald.mtf_taps of the band's gain;
    default gains: wald.DEFAULT_GAIN_MS, as mtf_glp) and decimated by 4 -> float32 (H/4, W/4, bands)"""
    from . import wald
    f = np.asarray(fused)
    if f.ndim != 3:
        raise ValueError('the fused image is (H, W, bands)')
    gains = wald._gain_rows(gains_ms, f.shape[2], wald.DEFAULT_GAIN_MS, 'gains_ms')
    return np.stack([fir_decimate4(f[..., k].astype(np.float32), wald.mtf_taps(g, n_taps), phase) for k, g in enumerate(gains)], axis=-1)


def d_lambda_k(fused, ms, gains_ms=None, n_taps=MTF_TAPS, phase=2):
    """Khan's spectral distortion: 1 - Q2n(MS, the fused image brought to MS resolution through the sensor's MTF)"""
    f, m = np.asarray(fused), np.asarray(ms)
    if f.ndim != 3 or m.ndim != 3 or f.shape[2] != m.shape[2]:
        raise ValueError('fused and MS images are (H, W, bands) with the same number of bands')
    if f.shape[0] % 4 or f.shape[1] % 4 or min(f.shape[:2]) < 4 * Q2N_BLOCK or m.shape[:2] != (f.shape[0] // 4, f.shape[1] // 4):
        raise ValueError(f'D_lambda_K needs H and W >= {4 * Q2N_BLOCK} (MS sides >= {Q2N_BLOCK}) and multiples of 4, and MS at a quarter of '
                         f'them (got fused {f.shape[:2]}, MS {m.shape[:2]})')
    return 1.0 - q2n(m, mtf_degrade_ms(f, gains_ms, n_taps, phase))


def hqnr(fused, ms, pan, gains_ms=None, n_taps=MTF_TAPS, phase=2):
    """hybrid QNR: (1 - D_lambda_K)(1 - D_s), D_s as in `qnr`"""
    return float((1.0 - d_lambda_k(fused, ms, gains_ms, n_taps, phase)) * (1.0 - d_s(fused, ms, pan)))


def ref_evaluate_ext(pred, gt):
    """ref_evaluate's five, then Q2n, SCC, CC"""
    return ref_evaluate(pred, gt) + [q2n(gt, pred), scc(gt, pred), cc(gt, pred)]


def no_ref_evaluate_ext(pred, pan, ms, gains_ms=None):
    """no_ref_evaluate's three, then D_lambda_K, HQNR"""
    dl, ds = d_lambda(pred, ms), d_s(pred, ms, pan)
    dk = d_lambda_k(pred, ms, gains_ms)
    return [dl, ds, (1.0 - dl) * (1.0 - ds), dk, (1.0 - dk) * (1.0 - ds)]
