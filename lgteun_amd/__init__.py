"""lgteun_amd -- MI355X-native (gfx950) implementation of the LGTEUN unfolding hot path behind the
reference's MODELS-registry / nn.Module surface.  Compute = hand-written HIP kernels behind a C ABI
(include/lgteun_hip.h); this package is the host-side mirror of the reference interface."""
from .builder import MODELS, build_model  # noqa: F401
from .unlg_former import Pansharpening, UnlgFormer  # noqa: F401
from .engine import Engine, FusedAdam, FusedAdamW, FusedRMSprop, FusedSGD, TrainControls, canonical_names  # noqa: F401
from .dataset import DATASETS, PSDataset, PrefetchLoader, SceneDataset, ShardedSampler, build_dataset, build_loader  # noqa: F401
from .classical import GSA, SFIM, Wavelet, gsa, interp23, sfim, wavelet  # noqa: F401
from .mtf_glp import MTF_GLP, MTF_GLP_CBD, MTF_GLP_HPM  # noqa: F401  (the function is mtf_glp.mtf_glp: its name is the module's)
from .bdsd import BDSD  # noqa: F401  (the function is bdsd.bdsd: its name is the module's)
from .cs import GS, IHS, PCA, Brovey  # noqa: F401  (the functions are cs.fuse, cs.ihs, cs.brovey, cs.gs, cs.pca)
from .atrous import ATWT, AWLP, atwt, awlp  # noqa: F401  (the general function is atrous.atrous: its name is the module's)
from . import mtf_hr  # noqa: F401  (the functions are mtf_hr.fuse, mtf_hr.fs, mtf_hr.hpm_r, mtf_hr.hpm_h, mtf_hr.bt_h)
from .mtf_hr import BT_H, MTF_GLP_FS, MTF_GLP_HPM_H, MTF_GLP_HPM_R  # noqa: F401
from .device_metrics import no_ref_evaluate_batch, no_ref_evaluate_ext_batch, ref_evaluate_batch, ref_evaluate_ext_batch  # noqa: F401
from .resident import ResidentLoader, ResidentStore  # noqa: F401
from .scene import fuse_scene, tile_grid  # noqa: F401
from .wald import SceneLoader, SceneStore, degrade_scene, export_triplets, mtf_taps, window_origins  # noqa: F401
