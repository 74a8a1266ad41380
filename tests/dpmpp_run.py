"""Helper of tests/test_gpu_dpmpp.py (not a test module): the shared inputs of the DPM-Solver++(2M)
tests on the `small` denoiser (n = 3 * 6 * 16 * 16 = 4608 per sample: one full 4096-element chunk
and one partial chunk, the smallest shape that reaches the multi-workgroup form's chunk sum), and a
main() that runs three single steps and one captured-graph sampling call and saves them to --out.
Run in its own process so that the sampler form can be chosen by EXTDM_SAMPLER_1WG, which the
library reads once per process."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

T = 1000
# (t_prev, t, t_next) of a first, a middle and a final step: entries of the 10-step logsnr grid
STEP_CASES = {'first': (-1, 909, 821), 'middle': (665, 449, 252), 'final': (10, 3, -1)}
STEP_B = 3
# per-sample scales of x and eps: sample 0 thresholds (s > 1), sample 1 does not (s = 1)
STEP_SCALES = (1.0, 0.02, 0.3)
LOOP_S, LOOP_B = 6, 2


def small_handle(max_batch=4):
    import importlib
    from tests.golden_inputs import CONFIGS, PKG, make_sd
    pkg = importlib.import_module(PKG)
    h = pkg._lib.Handle(CONFIGS['small'], T, max_batch, 0)
    sd = make_sd(CONFIGS['small'])
    sd.update(pkg.schedule_buffers(T))
    h.load_state(sd)
    h.finalize()
    return h


def step_inputs():
    """Seeded x, eps and a non-zero x0_prev, [STEP_B, 3, 6, 16, 16] each (CPU fp32)."""
    import torch
    from tests.golden_inputs import CONFIGS
    cfg = CONFIGS['small']
    g = torch.Generator().manual_seed(4608)
    shape = (STEP_B, 3, cfg.tp, cfg.latent, cfg.latent)
    sc = torch.tensor(STEP_SCALES).view(STEP_B, 1, 1, 1, 1)
    x = torch.randn(shape, generator=g) * sc
    eps = torch.randn(shape, generator=g) * sc
    prev = (torch.rand(shape, generator=g) * 2 - 1)
    return x, eps, prev


def run_step(h, case, dev):
    """extdm_sampler_step_hist on step_inputs() -> (x, x0_prev, thresholds) on the CPU."""
    import torch
    x, eps, prev = [v.to(dev).contiguous() for v in step_inputs()]
    th = torch.full((STEP_B,), -1., device=dev)
    h.sampler_step_hist(*STEP_CASES[case], x, eps, prev, th)
    torch.cuda.synchronize()
    return x.cpu(), prev.cpu(), th.cpu()


def loop_inputs():
    import torch
    from tests.golden_inputs import CONFIGS, unet_inputs
    cfg = CONFIGS['small']
    _, _, cond, fea = unet_inputs(cfg, B=LOOP_B, seed=61)
    xT = torch.randn((LOOP_B, 3, cfg.tp, cfg.latent, cfg.latent), generator=torch.Generator().manual_seed(62))
    return cond, fea, xT


def run_loop(h, times, dev, use_graph=True):
    """One extdm_sample call with EXTDM_SAMPLER_DPMPP and an injected x_T -> (out, thresholds [S][B])."""
    import importlib
    import torch
    from tests.golden_inputs import PKG
    pkg = importlib.import_module(PKG)
    cond, fea, xT = loop_inputs()
    S = len(times)
    rec = torch.full((S * LOOP_B,), -1., device=dev)
    h.record_thresholds(rec)
    out = torch.empty(xT.shape, device=dev)
    try:
        h.sample(pkg._lib.SAMPLER_DPMPP, times, None, 0., cond.to(dev), fea.to(dev), out, x_T=xT.to(dev),
                 use_graph=use_graph)
        torch.cuda.synchronize()
    finally:
        h.record_thresholds(None)
    return out.cpu(), rec.cpu().view(S, LOOP_B)


def loop_times(spacing):
    import importlib
    from tests.golden_inputs import PKG
    pkg = importlib.import_module(PKG)
    return pkg.dpmpp_times(T, LOOP_S, spacing, pkg.schedule_buffers(T)['alphas_cumprod'])


def run_all(h, dev):
    res = {}
    for case in STEP_CASES:
        res[f'{case}_x'], res[f'{case}_prev'], res[f'{case}_thresh'] = run_step(h, case, dev)
    res['loop_out'], res['loop_thresh'] = run_loop(h, loop_times('logsnr'), dev)
    return res


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    torch.save(run_all(small_handle(), torch.device('cuda:0')), a.out)


if __name__ == '__main__':
    main()
