"""Level-0 Upsample / Downsample launches (bench layers 18 / 19) on the direct two-tap kernel and on
the implicit GEMM (EXTDM_NO_X3_UPDOWN=1, read per launch), one BAIR handle, alternating."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_handle  # noqa: E402

h, B, prec = cfg_handle.make('bair')
res = {}
for rep in range(3):
    for arm in ('direct', 'gemm'):
        if arm == 'gemm':
            os.environ['EXTDM_NO_X3_UPDOWN'] = '1'
        else:
            os.environ.pop('EXTDM_NO_X3_UPDOWN', None)
        for layer in (18, 19):
            ms, fl = h.bench_layer(B, layer, 20)
            k = h.bench_layer_kernel(layer)
            res.setdefault(f'{layer}_{arm}', []).append(round(ms * 1e3, 1))
            print(f'rep {rep} layer {layer} {arm}: {ms * 1e3:.1f} us  {fl / ms / 1e9:.1f} TF/s  [{k}]', flush=True)
os.environ.pop('EXTDM_NO_X3_UPDOWN', None)
out_dir = os.environ.get('OUT', 'bench_out')
os.makedirs(out_dir, exist_ok=True)
print(json.dumps({'batch': B, 'us': res}))
open(os.path.join(out_dir, 'layer_ab.json'), 'w').write(json.dumps({'batch': B, 'us': res}))
