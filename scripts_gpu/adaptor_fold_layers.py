"""The first MotionAdaptor's last extrapolator conv and fuser conv (bench layers 20 / 21) with the
normalisation folded into the conv and on the separate passes (EXTDM_NO_ADAPTOR_FOLD=1 /
EXTDM_NO_LN_FOLD=1, read per handle: one BAIR handle per route, one after the other). The timed launch
is the conv alone on both routes; the passes the fold removes show in the kernel traces."""
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_handle  # noqa: E402

SW = ('EXTDM_NO_ADAPTOR_FOLD', 'EXTDM_NO_LN_FOLD')
res, kern = {}, {}
for arm in ('fold', 'separate'):
    for k in SW:
        os.environ.pop(k, None)
        if arm == 'separate':
            os.environ[k] = '1'
    h, B, prec = cfg_handle.make('bair')
    for k in SW:
        os.environ.pop(k, None)
    for rep in range(3):
        for layer in (20, 21):
            ms, fl = h.bench_layer(B, layer, 20)
            kern[f'{layer}_{arm}'] = h.bench_layer_kernel(layer)
            res.setdefault(f'{layer}_{arm}', []).append(round(ms * 1e3, 1))
            print(f'rep {rep} layer {layer} {arm}: {ms * 1e3:.1f} us  {fl / ms / 1e9:.1f} TF/s  [{kern[f"{layer}_{arm}"]}]', flush=True)
    del h
    gc.collect()
out_dir = os.environ.get('OUT', 'bench_out')
os.makedirs(out_dir, exist_ok=True)
print(json.dumps({'batch': B, 'us': res}))
open(os.path.join(out_dir, 'adaptor_fold_layers.json'), 'w').write(json.dumps({'batch': B, 'us': res, 'kernel': kern}))
