"""One KTH-size generation (bench.py's kth workload: ada denoiser, 10 -> 20 frames, its bench batch,
synthetic weights) under three samplers, timed on the device:

  DDIM, 100 steps (the kth.yaml default)          extdm_sample(EXTDM_SAMPLER_DDIM)
  DPM-Solver++(2M), 20 steps, 'ddim' grid         extdm_sample(EXTDM_SAMPLER_DPMPP)
  DPM-Solver++(2M), 20 steps, 'logsnr' grid

Each timed window is one whole extdm_sample call on the captured-graph path between two device
events; the variants alternate inside every round (REPEATS rounds after WARMUP untimed ones) and the
median, minimum and maximum over the rounds are reported. Information only: what 20 second-order
steps do to sample quality on trained checkpoints is not measured here.

    python scripts_gpu/dpmpp_kth.py --out profiles/dpmpp_kth.json"""
import argparse
import json
import statistics
import sys

import torch

import cfg_handle as C

WARMUP, REPEATS = 2, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--config', default='kth')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('no GPU: this script only measures on the device')
    pkg = C.pkg
    h, B, prec = C.make(a.config)
    cfg = h.cfg
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(11)
    cond = (torch.rand((B, 3, cfg.tc, cfg.latent, cfg.latent), generator=g) * 2 - 1).to(dev)
    fea = torch.randn((B, cfg.fea_ch, cfg.frames, cfg.fea_size, cfg.fea_size), generator=g).to(dev)
    out = torch.empty((B, 3, cfg.tp, cfg.latent, cfg.latent), device=dev)
    acp = pkg.schedule_buffers(1000)['alphas_cumprod']
    pairs = pkg.ddim_time_pairs(1000, 100)
    L = pkg._lib
    variants = {
        'ddim_100': (L.SAMPLER_DDIM, [p[0] for p in pairs], [p[1] for p in pairs], 1.0),
        'dpmpp_2m_20_ddim': (L.SAMPLER_DPMPP, pkg.dpmpp_times(1000, 20, 'ddim', acp), None, 0.0),
        'dpmpp_2m_20_logsnr': (L.SAMPLER_DPMPP, pkg.dpmpp_times(1000, 20, 'logsnr', acp), None, 0.0),
    }
    ms = {k: [] for k in variants}
    finite = {}
    for r in range(WARMUP + REPEATS):
        for name, (sampler, times, nexts, eta) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h.sample(sampler, times, nexts, eta, cond, fea, out, seed=5, use_graph=True)
            e1.record()
            e1.synchronize()
            if r >= WARMUP:
                ms[name].append(e0.elapsed_time(e1))
            finite[name] = bool(torch.isfinite(out).all())
    res = {'config': a.config, 'batch': B, 'precision': prec, 'pred_frames': cfg.tp, 'warmup': WARMUP,
           'repeats': REPEATS, 'timing': 'device events around one extdm_sample call (graph path), variants '
                                         'alternating per round', 'variants': {}}
    for name, v in ms.items():
        S = len(variants[name][1])
        med = statistics.median(v)
        res['variants'][name] = {'steps': S, 'median_ms': round(med, 3), 'min_ms': round(min(v), 3),
                                 'max_ms': round(max(v), 3), 'ms_per_step': round(med / S, 3),
                                 'pred_frames_per_s': round(B * cfg.tp / (med * 1e-3), 1), 'finite': finite[name]}
    base = res['variants']['ddim_100']['median_ms']
    for name, v in res['variants'].items():
        v['speedup_vs_ddim_100'] = round(base / v['median_ms'], 3)
    res['note'] = ('time per generation only; sample quality of the 20-step solver on trained checkpoints is '
                   'not measured (synthetic weights)')
    print(json.dumps(res))
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
