"""MI355X-native ExtDM sampling path (gfx950 HIP kernels behind a C ABI).

Import with importlib (the directory name is not a Python identifier):
    pkg = importlib.import_module('140-extdm-distribution-extrapolation-diffusion-model-for-video-prediction_amd')
"""
from . import spec, weights, configs, dist, metrics, _lib  # noqa: F401
from .models import (Unet3D, Unet3DAda, Unet3DAdaU22, Unet3DWoRef, UNET3D_BY_MODULE, GaussianDiffusion,  # noqa: F401
                     schedule_buffers, ddim_time_pairs, dpmpp_times)
from .metrics import (InceptionI3d, load_i3d_pretrained, get_feats, get_fvd_feats, calculate_fvd,  # noqa: F401
                      calculate_fvd1, calculate_fvd2, LPIPS, load_lpips_pretrained, calculate_lpips,
                      calculate_lpips1, calculate_lpips2, calculate_lpips3, best_of_n_lpips)
from .lfae import (Generator, RegionPredictor, BGMotionPredictor, FlowDiffusion,  # noqa: F401
                   FlowDiffusionMultiWRef, FlowDiffusionMultiWRefU22, FlowDiffusionMulti1248,
                   FLOW_DIFFUSION_BY_MODULE, autoregressive_sample)
