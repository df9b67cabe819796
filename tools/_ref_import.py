"""Import the reference hot path (/root/reference) on CPU in THIS container only.

Used by tools/gen_goldens.py to (i) validate the oracle restatement and (ii) generate
the golden fixtures committed under tests/golden/.  Nothing of the reference travels:
this module only *imports* it from where it lies.  Recipe follows SURVEY.md §8(c).
"""
import sys
import types

REF = '/root/reference'


def _stub_modules():
    sys.dont_write_bytecode = True

    class Registry:
        def __init__(self, name):
            self.name = name
            self._d = {}

        def register_module(self, name=None, force=False, module=None):
            def deco(cls):
                self._d[name or cls.__name__] = cls
                return cls
            return deco

        def get(self, key):
            return self._d.get(key)

        def __contains__(self, key):
            return key in self._d

    class Config(dict):
        def __getattr__(self, k):
            try:
                return self[k]
            except KeyError:
                raise AttributeError(k)

        def __setattr__(self, k, v):
            self[k] = v

        def __getitem__(self, k):
            v = dict.__getitem__(self, k)
            return Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v

        def get(self, k, d=None):
            v = dict.get(self, k, d)
            return Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v

        def copy(self):
            return Config(dict.copy(self))

    class Timer:
        def __init__(self):
            import time
            self.t = time.time()

        def since_last_check(self):
            import time
            now = time.time()
            d = now - self.t
            self.t = now
            return d

    def mkdir_or_exist(path, mode=0o777):
        import os
        os.makedirs(path, exist_ok=True)

    mmcv = types.ModuleType('mmcv')
    mmcv_utils = types.ModuleType('mmcv.utils')
    mmcv_utils.Registry = Registry
    mmcv.utils = mmcv_utils
    mmcv.Config = Config
    mmcv.Timer = Timer
    mmcv.mkdir_or_exist = mkdir_or_exist
    sys.modules['mmcv'] = mmcv
    sys.modules['mmcv.utils'] = mmcv_utils
    if 'cv2' not in sys.modules:
        sys.modules['cv2'] = cv2_standin()
    for name in ('gdal', 'osr', 'tifffile'):
        sys.modules.setdefault(name, types.ModuleType(name))
    numba = types.ModuleType('numba')
    numba.jit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
    sys.modules.setdefault('numba', numba)
    models = types.ModuleType('models')
    models.__path__ = [REF + '/models']
    sys.modules['models'] = models
    return Config


# ---------------------------------------------------------------------------------------------------------------------
# The three OpenCV functions the reference calls, as stand-ins written from OpenCV's documentation, each only in the regime the
# reference uses it in.  Anything else raises, so a fixture can never be the product of a stand-in's guess.
# ---------------------------------------------------------------------------------------------------------------------
STANDINS = {
    'cv2.filter2D': 'scipy.ndimage.correlate, default origin (anchor at ksize // 2), ddepth -1 only; the border rule is a switch '
                    '(cv2_standin().border) because every caller crops the border rows away: the generator proves that by running both',
    'cv2.getGaussianKernel': 'exp(-(i - (n - 1) / 2)^2 / (2 s^2)) normalised to sum 1, as an (n, 1) column; s > 0 only',
    'cv2.resize': 'to exactly a quarter of both sides only: INTER_NEAREST = src[::4, ::4], INTER_LINEAR = the mean of the 2 x 2 centre of '
                  'each 4 x 4 block; the third positional argument is dst (ignored), as in OpenCV; any other size or flag raises',
}
BORDERS = {'mirror': dict(mode='mirror'), 'huge': dict(mode='constant', cval=1e30)}


def cv2_standin():
    import numpy as np
    from scipy import ndimage
    cv2 = types.ModuleType('cv2')
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC = 0, 1, 2
    cv2.border = 'mirror'
    cv2.calls = {'filter2D': 0, 'getGaussianKernel': 0, 'resize': 0}

    def filter2D(src, ddepth, kernel):
        if ddepth != -1 or src.ndim != 2 or kernel.ndim != 2 or src.dtype != np.float64:
            raise NotImplementedError('filter2D stand-in: float64 (H, W) source, ddepth -1, 2-D kernel')
        cv2.calls['filter2D'] += 1
        return ndimage.correlate(src, np.asarray(kernel, np.float64), **BORDERS[cv2.border])

    def getGaussianKernel(ksize, sigma):
        if ksize < 1 or ksize % 2 == 0 or not sigma > 0:
            raise NotImplementedError('getGaussianKernel stand-in: odd ksize, sigma > 0')
        cv2.calls['getGaussianKernel'] += 1
        i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2.0
        k = np.exp(-(i * i) / (2.0 * sigma * sigma))
        return (k / k.sum()).reshape(ksize, 1)

    def resize(src, dsize, dst=None, fx=0, fy=0, interpolation=1):
        a = np.asarray(src)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[..., 0]                       # OpenCV returns a single-channel image as (H, W)
        wd, hd = dsize                          # OpenCV's order: (width, height)
        if a.ndim != 2 or fx or fy or a.shape != (4 * hd, 4 * wd):
            raise NotImplementedError(f'resize stand-in: to exactly a quarter of both sides (source {a.shape}, dsize {dsize})')
        cv2.calls['resize'] += 1
        if interpolation == cv2.INTER_NEAREST:
            return a[::4, ::4].copy()
        if interpolation == cv2.INTER_LINEAR:
            return 0.25 * (a[1::4, 1::4] + a[1::4, 2::4] + a[2::4, 1::4] + a[2::4, 2::4])
        raise NotImplementedError(f'resize stand-in: interpolation flag {interpolation}')

    cv2.filter2D, cv2.getGaussianKernel, cv2.resize = filter2D, getGaussianKernel, resize
    return cv2


SHIMS = {'numpy.int': 'np.int = int (removed in numpy 1.24; upsample_interp23 calls it)'}


def import_reference_parity():
    """what tools/gen_goldens.py --only-parity runs: the reference's metrics module, its SFIM_ / GSA_ / upsample_interp23 and its QNRLoss,
    over the cv2 stand-in above"""
    import numpy as np
    _stub_modules()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    if not hasattr(np, 'int'):
        np.int = int
    import models.base.metrics as mtc  # noqa
    from models.SFIM import SFIM_  # noqa
    from models.GSA import GSA_  # noqa
    from models.common.model_based_utils import upsample_interp23  # noqa
    from models.base.losses import QNRLoss  # noqa
    cv2 = sys.modules['cv2']
    assert mtc.cv2 is cv2 and hasattr(cv2, 'border'), 'the reference was imported over another cv2'
    return types.SimpleNamespace(mtc=mtc, SFIM_=SFIM_, GSA_=GSA_, upsample_interp23=upsample_interp23, QNRLoss=QNRLoss, cv2=cv2)


def import_reference():
    Config = _stub_modules()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from models.unlg_former import Pansharpening, UnlgFormer  # noqa
    import models.common.LGT as LGT  # noqa
    import models.common.basic_module_unformer_v2 as bmu  # noqa
    return types.SimpleNamespace(Pansharpening=Pansharpening, UnlgFormer=UnlgFormer, LGT=LGT, bmu=bmu,
                                 Config=Config)


def import_reference_dataset_utils():
    """dataset/utils.py of the reference (data_normalize / data_denormalize / data_augmentation, :155-263): pure torch / numpy
    functions behind imports of gdal / osr / tifffile / numba (stubbed as above; none of the three functions touches them).  The
    package's __init__ (which pulls in the TIFF dataset class and its registry) is bypassed the same way `models` is."""
    _stub_modules()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    pkg = types.ModuleType('dataset')
    pkg.__path__ = [REF + '/dataset']
    sys.modules['dataset'] = pkg
    import dataset.utils as du  # noqa
    return du
