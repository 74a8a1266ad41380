"""Generate tests/golden/long_forward.npz by running the REFERENCE itself on CPU in the build
container (like make_golden.py: the reference is imported through the shims at generation time
only, and only data leaves this script): clips of more than 32 model frames.

  eps          the reference u12 Unet3D forward at dim 16, tc = 2, tp = 38 (40 model frames),
               latent 16, on the seeded weights / inputs of tests/golden_inputs.py: clip 0 of a
               B = 2 forward, [1][3][38][16][16] (at B = 1 the reference's STW trips a view at the
               levels whose window collapses to 2x2, golden_inputs.ddpm1000_case; clips are
               independent, so the stored clip is the B = 1 result)
  time_bias50  time_rel_pos_bias(50) [heads][50][50] of the same weights: the T5 buckets at
               |i - j| >= 32, which no shorter clip reaches

Usage (build container only):  python tests/golden/make_golden_long.py
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
from tests.golden_inputs import PKG, make_sd, unet_inputs  # noqa: E402
from make_golden import build_ref_unet, import_reference  # noqa: E402

spec = importlib.import_module(PKG + '.spec')
LONG_CFG = dict(dim=16, tc=2, tp=38, latent=16, fea_size=8)
BIAS_T = 50


def main():
    torch.set_num_threads(8)
    Unet3D, _, _ = import_reference()
    cfg = spec.UnetConfig(**LONG_CFG)
    net = build_ref_unet(Unet3D, cfg)
    net.load_state_dict(make_sd(cfg), strict=True)
    x, t, cond, fea = unet_inputs(cfg, B=2)
    with torch.no_grad():
        eps = net(x, t, cond, cond_fea=fea)
        bias = net.time_rel_pos_bias(BIAS_T, device=x.device)
    np.savez_compressed(os.path.join(HERE, 'long_forward.npz'), eps=eps[:1].numpy(), time_bias50=bias.numpy())
    print('eps', tuple(eps.shape), float(eps.abs().mean()), 'time_bias50', tuple(bias.shape))


if __name__ == '__main__':
    main()
