"""Outputs of the paths the bench step does not reach, for a byte comparison of two builds of
the library (EXTDM_LIB selects the one a process loads), and the wall time of extdm_finalize.

  python scripts_gpu/pack_identity.py dump DIR       # one process per library
  python scripts_gpu/pack_identity.py compare DIR_A DIR_B OUT.json

dump writes, on the seeded weights and inputs of the tests:
  i3d_*       InceptionI3d logits / pooled features (tests/i3d_inputs.py 't10') and every endpoint tap
  lfae_*      region parameters, background, bottleneck and the generator's outputs (flow, decode)
              of tests/test_gpu_lfae.py's inputs
  unet_*      one Unet forward per precision mode of the reduced u12 and ada_u22 configurations
  timing.json extdm_finalize wall time of the BAIR configuration (max_batch 4)
"""
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def dump(out):
    import torch
    from tests import i3d_inputs as I
    from tests.golden_inputs import CONFIGS, PKG, make_sd, unet_inputs, video_inputs
    pkg = importlib.import_module(PKG)
    dev = torch.device('cuda:0')
    os.makedirs(out, exist_ok=True)

    def save(name, t):
        np.save(os.path.join(out, name + '.npy'), t.detach().cpu().numpy())

    # extdm_finalize of BAIR: packing and upload of every weight, tables, workspace plan
    cfg = CONFIGS['bair']
    h = pkg._lib.Handle(cfg, 1000, 4, 0)
    sd = make_sd(cfg)
    sd.update(pkg.schedule_buffers(1000))
    h.load_state(sd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h.finalize()
    torch.cuda.synchronize()
    fin = time.perf_counter() - t0
    del h
    with open(os.path.join(out, 'timing.json'), 'w') as f:
        json.dump({'bair_finalize_s': fin, 'lib': os.environ.get('EXTDM_LIB', 'in-tree')}, f)
    print(f'bair finalize {fin:.3f} s', flush=True)

    for name in ('small', 'u22_small'):
        cfg = CONFIGS[name]
        x, t, cond, fea = (v.to(dev) for v in unet_inputs(cfg, B=2))
        for prec in ('f16x3', 'fp32', 'bf16_attn'):
            h = pkg._lib.Handle(cfg, 1000, 2, 0, precision=prec)
            sd = make_sd(cfg)
            sd.update(pkg.schedule_buffers(1000))
            h.load_state(sd)
            h.finalize()
            eps = torch.empty_like(x)
            h.unet_forward(x, t, cond, fea, eps)
            torch.cuda.synchronize()
            save(f'unet_{name}_{prec}', eps)
            del h
    print('unet done', flush=True)

    from tests.test_gpu_lfae import fdiff
    fd = fdiff(True)
    vid = video_inputs().to(dev)
    ref, drv_img = vid[:, :, 1].contiguous(), vid[:, :, 0].contiguous()
    src, drv = fd.region_predictor(ref), fd.region_predictor(drv_img)
    for tag, p in (('src', src), ('drv', drv)):
        for k, v in p.items():
            save(f'lfae_region_{tag}_{k}', v)
    bg = fd.bg_predictor(ref, drv_img)
    save('lfae_bg', bg)
    save('lfae_bottleneck', fd.generator.forward_bottle(drv_img))
    for k, v in fd.generator(ref, source_region_params=src, driving_region_params=drv, bg_params=bg).items():
        save(f'lfae_generator_{k}', v)
    print('lfae done', flush=True)

    net = pkg.metrics.InceptionI3d()
    net.load_state_dict(I.make_i3d_sd())
    net = net.to(dev)
    net._h(dev, 2, 10)
    x = I.full_input('t10').to(dev)
    save('i3d_logits', net(x))
    save('i3d_pooled', net.extract_features(x))
    xt = I.tap_input().to(dev)
    for ep in I.TAPS:
        save(f'i3d_tap_{ep}', net.endpoint(xt, ep))
    print('i3d done', flush=True)


def compare(a, b, out):
    names = sorted(n for n in os.listdir(a) if n.endswith('.npy'))
    assert names and names == sorted(n for n in os.listdir(b) if n.endswith('.npy')), 'different item sets'
    items, differing = {}, 0
    for n in names:
        da, db = open(os.path.join(a, n), 'rb').read(), open(os.path.join(b, n), 'rb').read()
        arr = np.load(os.path.join(a, n))
        same = da == db
        differing += not same
        items[n[:-4]] = {'identical': same, 'sha256': hashlib.sha256(da).hexdigest()[:16], 'elements': int(arr.size),
                         'finite': bool(np.isfinite(arr).all())}
        if not same:
            items[n[:-4]]['max_abs_diff'] = float(np.abs(arr.astype(np.float64) - np.load(os.path.join(b, n))).max())
    res = {'items': items, 'compared': len(names), 'differing': differing,
           'finalize': {os.path.basename(d): json.load(open(os.path.join(d, 'timing.json'))) for d in (a, b)}}
    with open(out, 'w') as f:
        json.dump(res, f, indent=1)
    print(f'{len(names)} items compared, {differing} differ')
    return 1 if differing else 0


if __name__ == '__main__':
    if sys.argv[1] == 'dump':
        dump(sys.argv[2])
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4]))
