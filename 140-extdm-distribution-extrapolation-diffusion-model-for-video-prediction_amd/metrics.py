"""Evaluation metrics of the reference's eval driver (scripts/DM/valid.py:199-243):
per-frame PSNR / SSIM on the device (metrics.hip through extdm_frame_metrics), the
reference's per-video reductions, best-of-n selection, frechet_distance and the
mean / std / 95 % interval summary.

Videos follow the reference's metric layout [n, t, c, h, w] (valid.py:194-195 rearranges
`(b n) c t h w -> b n t c h w`); `frame_metrics` also takes the sampler's channel-first
[n, c, t, h, w] through `layout='ncthw'`, so generated clips need no transpose. Values
are in [0, 1] as the reference's (calculate_psnr.py:6-7). The I3D features of FVD come
from `InceptionI3d` (metrics/pytorch_i3d.py, on the native library's 3-D convolution) with
the mirrored front end of metrics/calculate_fvd.py and fvd.py (`trans`, `preprocess_single`,
`get_fvd_feats`, `get_feats`, `calculate_fvd*`); the weights are the user's own
i3d_pretrained_400.pt state_dict (`load_i3d_pretrained`), which the reference does not ship
either. LPIPS (metrics/calculate_lpips.py) is `LPIPS`, the published package's AlexNet metric
restated on the native library's 2-D convolution and distance head, with the user's own weight
files (`load_lpips_pretrained`); all frame pairs of a call run as one batch.
"""
import warnings

import numpy as np
import torch
import torch.nn as nn

from . import _lib


def frame_metrics(videos1, videos2, layout='ntchw'):
    """Per-frame (PSNR, SSIM) of two fp32 ROCm tensors [n, t, c, h, w] (or [n, c, t, h, w]
    with layout='ncthw'), c in {1, 3}: two float64 tensors [n, t] on the same device.
    PSNR: metrics/calculate_psnr.py:6-15; SSIM: metrics/calculate_ssim.py:6-41."""
    import torch
    if videos1.shape != videos2.shape:
        raise AssertionError('videos must have the same shape')  # calculate_psnr.py:24
    if videos1.dim() != 5:
        raise ValueError('expected 5-D videos')
    _lib._require_device(videos1, videos2)
    if layout == 'ntchw':
        n, t, c, h, w = videos1.shape
        sn, st, sc = t * c * h * w, c * h * w, h * w
    elif layout == 'ncthw':
        n, c, t, h, w = videos1.shape
        sn, st, sc = c * t * h * w, h * w, t * h * w
    else:
        raise ValueError(f'unknown layout {layout!r}')
    if c not in (1, 3):
        raise ValueError('Wrong input image dimensions.')  # calculate_ssim.py:40-41
    L = _lib.load()
    psnr = torch.empty(n, t, dtype=torch.float64, device=videos1.device)
    ssim = torch.empty(n, t, dtype=torch.float64, device=videos1.device)
    work = torch.empty(max(1, L.extdm_frame_metrics_workspace(n, t, c, h, w)), dtype=torch.uint8,
                       device=videos1.device)
    with torch.cuda.device(videos1.device):
        _lib.check(L.extdm_frame_metrics(_lib._ptr(videos1), _lib._ptr(videos2), n, t, c, h, w, sn, st, sc,
                                         _lib._ptr(psnr), _lib._ptr(ssim), _lib._ptr(work), _lib._stream()))
    return psnr, ssim


def _as_chw(img):
    # the reference also takes a 2-D [h, w] image (calculate_ssim.py:31-32)
    return img[None] if img.dim() == 2 else img


def img_psnr(img1, img2):
    """metrics/calculate_psnr.py:6-15 for one [c, h, w] (or [h, w]) image."""
    return float(frame_metrics(_as_chw(img1)[None, None], _as_chw(img2)[None, None])[0][0, 0])


def calculate_ssim_function(img1, img2):
    """metrics/calculate_ssim.py:26-41 for one [c, h, w] (c in {1, 3}) or [h, w] image."""
    if img1.shape != img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    if img1.dim() not in (2, 3):
        raise ValueError('Wrong input image dimensions.')
    return float(frame_metrics(_as_chw(img1)[None, None], _as_chw(img2)[None, None])[1][0, 0])


def _per_frame_summary(vals, name, shape):
    v = vals.cpu().numpy()
    return {name: {f'avg[{i}]': np.mean(v[:, i]) for i in range(v.shape[1])},
            f'{name}_std': {f'std[{i}]': np.std(v[:, i]) for i in range(v.shape[1])},
            f'{name}_video_setting': shape, f'{name}_video_setting_name': 'time, channel, heigth, width'}


def calculate_psnr(videos1, videos2):
    """metrics/calculate_psnr.py:19-69: mean / std over videos per frame index."""
    return _per_frame_summary(frame_metrics(videos1, videos2)[0], 'psnr', videos1.shape[1:])


def calculate_ssim(videos1, videos2):
    """metrics/calculate_ssim.py:46-101."""
    return _per_frame_summary(frame_metrics(videos1, videos2)[1], 'ssim', videos1.shape[1:])


def calculate_psnr1(videos1, videos2):
    """metrics/calculate_psnr.py:71-87: (mean, std) over every frame."""
    v = frame_metrics(videos1, videos2)[0].cpu().numpy()
    return np.mean(v), np.std(v)


def calculate_ssim1(videos1, videos2):
    """metrics/calculate_ssim.py:103-117."""
    v = frame_metrics(videos1, videos2)[1].cpu().numpy()
    return np.mean(v), np.std(v)


def calculate_psnr2(videos1, videos2):
    """metrics/calculate_psnr.py:89-106: the best of the n samples, max over n of the
    per-sample mean over frames (valid.py:232 passes one clip's n samples)."""
    v = frame_metrics(videos1, videos2)[0].cpu().numpy()
    return np.max(np.mean(v, axis=-1))


def calculate_ssim2(videos1, videos2):
    """metrics/calculate_ssim.py:119-134."""
    v = frame_metrics(videos1, videos2)[1].cpu().numpy()
    return np.max(np.mean(v, axis=-1))


def best_of_n(origin_videos, result_videos, cond_frames):
    """valid.py:226-233: PSNR / SSIM of each clip's best sample over the predicted frames.
    origin_videos, result_videos: [b, n, t, c, h, w]. Returns (psnr_list, ssim_list), one
    value per clip; all b*n*t frames go through one device launch."""
    b, n = result_videos.shape[:2]
    a = origin_videos[:, :, cond_frames:].contiguous().flatten(0, 1)
    r = result_videos[:, :, cond_frames:].contiguous().flatten(0, 1)
    psnr, ssim = frame_metrics(a, r)
    pm = psnr.mean(dim=-1).view(b, n).max(dim=1).values.cpu().numpy()
    sm = ssim.mean(dim=-1).view(b, n).max(dim=1).values.cpu().numpy()
    return list(pm), list(sm)


def select_best(origin_feats, result_feats, num_sample_video):
    """valid.py:234-240: per clip, the sample whose features are nearest (L1) to the
    ground truth's: origin_feats [b, d], result_feats [b * n, d] -> indices [b]."""
    o = np.asarray(origin_feats)
    r = np.asarray(result_feats).reshape(o.shape[0], num_sample_video, -1)
    scores = np.abs(o[:, None, :] - r).sum(axis=-1)
    return np.argmin(scores, axis=-1)


def frechet_distance(feats_fake, feats_real):
    """metrics/fvd.py:276-293: squared distance of the feature means plus
    tr(S_fake) + tr(S_real) - 2 tr(sqrtm(S_fake S_real)) of the (unbiased) covariances;
    the mean term alone when there is a single fake feature. Host fp64 (scipy sqrtm),
    as the reference computes it."""
    from scipy.linalg import sqrtm
    fake, real = np.asarray(feats_fake), np.asarray(feats_real)
    dmu = fake.mean(axis=0) - real.mean(axis=0)
    mean_term = np.square(dmu).sum()
    if fake.shape[0] <= 1:
        return float(np.real(mean_term))
    cov_f, cov_r = np.cov(fake, rowvar=False), np.cov(real, rowvar=False)
    root = sqrtm(cov_f @ cov_r, disp=False)[0]
    return float(np.real(mean_term + np.trace(cov_f + cov_r - 2 * root)))


def metric_stuff(metric):
    """valid.py:24-27: mean, std and the half-width of the normal 95 % interval."""
    import scipy.stats as st
    avg_metric, std_metric = metric.mean().item(), metric.std().item()
    conf95_metric = avg_metric - float(st.norm.interval(confidence=0.95, loc=avg_metric, scale=st.sem(metric))[0])
    return avg_metric, std_metric, conf95_metric


def eval_metrics(origin_videos, result_videos, cond_frames, origin_feats=None, result_feats=None, i3d=None,
                 mini_bs=16, lpips=None):
    """The metric half of valid.py:199-257 on [b, n, t, c, h, w] videos: per clip the best of
    its n samples for PSNR and SSIM over the predicted frames (calculate_psnr2 /
    calculate_ssim2), summarised by metric_stuff. With video features (origin [b, d], result
    [b * n, d]) the best sample per clip by feature L1 (valid.py:234-240) and its
    frechet_distance to the originals ('fvd_best'), and one frechet_distance per sample
    trajectory summarised by metric_stuff ('fvd_traj_mean' / '_std' / '_conf95',
    valid.py:207-213). The features are either given, or computed here by the detector `i3d`
    (an InceptionI3d with the user's weights, load_i3d_pretrained): origin_feats from
    origin_videos[:, 0] and result_feats from the `(b n)` flattening (valid.py:203-204), in
    mini-batches of mini_bs. The reference runs the detector again on the selected videos
    (valid.py:235); here their rows of result_feats are taken, which is the same thing because
    a video's features do not depend on its batch. With `lpips` (an LPIPS with the user's
    weights, load_lpips_pretrained) the best sample per clip by LPIPS over the predicted frames
    (calculate_lpips2, valid.py:228) summarised by metric_stuff as 'lpips' / '_std' / '_conf95'
    (valid.py:243); without it the dict has no LPIPS entries."""
    if i3d is not None and origin_feats is None and result_feats is None:
        origin_feats = get_feats(origin_videos[:, 0], origin_videos.device, mini_bs=mini_bs, i3d=i3d)
        result_feats = get_feats(result_videos.flatten(0, 1), result_videos.device, mini_bs=mini_bs, i3d=i3d)
    psnr_list, ssim_list = best_of_n(origin_videos, result_videos, cond_frames)
    avg_psnr, std_psnr, conf95_psnr = metric_stuff(np.array(psnr_list))
    avg_ssim, std_ssim, conf95_ssim = metric_stuff(np.array(ssim_list))
    out = {'psnr': avg_psnr, 'psnr_std': std_psnr, 'psnr_conf95': conf95_psnr,
           'ssim': avg_ssim, 'ssim_std': std_ssim, 'ssim_conf95': conf95_ssim}
    if origin_feats is not None and result_feats is not None:
        n = result_videos.shape[1]
        idx = select_best(origin_feats, result_feats, n)
        rf = np.asarray(result_feats).reshape(len(idx), n, -1)
        best = rf[np.arange(len(idx)), idx]
        out['fvd_best'] = frechet_distance(np.asarray(origin_feats), best)
        out['selected_index'] = idx
        # per trajectory: the features of every clip's traj-th sample (valid.py:207-209)
        fvd_list = [frechet_distance(np.asarray(origin_feats), rf[:, traj]) for traj in range(n)]
        out['fvd_traj_mean'], out['fvd_traj_std'], out['fvd_traj_conf95'] = metric_stuff(np.array(fvd_list))
    if lpips is not None:
        lpips_list = best_of_n_lpips(origin_videos, result_videos, cond_frames, lpips)
        out['lpips'], out['lpips_std'], out['lpips_conf95'] = metric_stuff(np.array(lpips_list))
    return out


# ---------------------------------------------------------------- FVD features (I3D)
class _Unit3D(nn.Module):
    """Parameter holder of a Unit3D (pytorch_i3d.py:37-69): `conv3d` and, with batch norm, `bn`
    carry the reference's state_dict entries; the arithmetic runs in the native library."""

    def __init__(self, in_channels, output_channels, kernel_shape=(1, 1, 1), stride=(1, 1, 1), use_batch_norm=True,
                 use_bias=False):
        super().__init__()
        self.conv3d = nn.Conv3d(in_channels, output_channels, tuple(kernel_shape), stride=stride, padding=0,
                                bias=use_bias)
        if use_batch_norm:
            self.bn = nn.BatchNorm3d(output_channels, eps=1e-5, momentum=0.001)


class _InceptionModule(nn.Module):
    """pytorch_i3d.py:107-125 (b3a, the max pool, has no state)."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.b0 = _Unit3D(in_channels, out_channels[0])
        self.b1a = _Unit3D(in_channels, out_channels[1])
        self.b1b = _Unit3D(out_channels[1], out_channels[2], (3, 3, 3))
        self.b2a = _Unit3D(in_channels, out_channels[3])
        self.b2b = _Unit3D(out_channels[3], out_channels[4], (3, 3, 3))
        self.b3b = _Unit3D(in_channels, out_channels[5])


def _need_rocm(x):
    if not x.is_cuda:
        raise RuntimeError('ExtDM HIP path needs tensors on a ROCm device (no CPU fallback)')


class _MetricPrecision:
    """The `precision` attribute of InceptionI3d and LPIPS: 'f16x3' (the default), 'fp32' (the
    exact-fp32 convolutions on v_mfma_f32_32x32x2_f32, no fp16 range limit) or 'auto': f16x3 until
    the library reports an activation at the fp16 range, then one RuntimeWarning, the call re-run
    on fp32 (InceptionI3d: on a handle rebuilt for it; LPIPS: on the same handle, the route is a
    flag of the call), and fp32 from then on (GaussianDiffusion._run_sampler's scheme)."""

    PRECISIONS = ('f16x3', 'fp32', 'auto')
    _RANGE_MSG = 'out of fp16 range (|v| >= 65504)'

    @property
    def precision(self):
        return self.__dict__.get('_precision', 'f16x3')

    @precision.setter
    def precision(self, value):
        if value not in self.PRECISIONS:
            raise ValueError(f'precision must be one of {self.PRECISIONS}, got {value!r}')
        self.__dict__['_precision'] = value
        self.__dict__['_fp32_fallback'] = False

    def _route(self):
        """The handle precision of the next call."""
        p = self.precision
        return 'fp32' if p == 'fp32' or (p == 'auto' and self.__dict__.get('_fp32_fallback', False)) else 'f16x3'

    def _on_route(self, run):
        """run() on the current route; under 'auto', once more on fp32 after the range error."""
        try:
            return run()
        except RuntimeError as e:
            if self.precision != 'auto' or self._route() == 'fp32' or self._RANGE_MSG not in str(e):
                raise
            warnings.warn(f'{type(self).__name__}: f16x3 activations reached the fp16 range (|v| >= 65504); '
                          're-running the call and continuing on the FP32 kernels', RuntimeWarning)
            self.__dict__['_fp32_fallback'] = True
            return run()


class InceptionI3d(_MetricPrecision, nn.Module):
    """Inception-v1 I3D (metrics/pytorch_i3d.py:135-322), the detector of FVD, on the native
    library: the reference's constructor signature, state_dict keys and shapes (344 entries at
    the defaults, the public i3d_pretrained_400.pt layout), forward -> [N, num_classes]
    pre-softmax logits averaged over the time slots, extract_features -> the avg-pooled
    [N, 1024, T'' - 1, 1, 1], replace_logits. Inference only (dropout is the identity); inputs
    are [N, in_channels, T >= 9, 224, 224] device tensors. A video's outputs are bitwise
    independent of the batch it sits in. `precision` (an attribute, _MetricPrecision) selects the
    arithmetic of the convolutions."""

    VALID_ENDPOINTS = ('Conv3d_1a_7x7', 'MaxPool3d_2a_3x3', 'Conv3d_2b_1x1', 'Conv3d_2c_3x3', 'MaxPool3d_3a_3x3',
                       'Mixed_3b', 'Mixed_3c', 'MaxPool3d_4a_3x3', 'Mixed_4b', 'Mixed_4c', 'Mixed_4d', 'Mixed_4e',
                       'Mixed_4f', 'MaxPool3d_5a_2x2', 'Mixed_5b', 'Mixed_5c', 'Logits', 'Predictions')
    _MIXED = (('Mixed_3b', 192, (64, 96, 128, 16, 32, 32)), ('Mixed_3c', 256, (128, 128, 192, 32, 96, 64)),
              ('Mixed_4b', 480, (192, 96, 208, 16, 48, 64)), ('Mixed_4c', 512, (160, 112, 224, 24, 64, 64)),
              ('Mixed_4d', 512, (128, 128, 256, 24, 64, 64)), ('Mixed_4e', 512, (112, 144, 288, 32, 64, 64)),
              ('Mixed_4f', 528, (256, 160, 320, 32, 128, 128)), ('Mixed_5b', 832, (256, 160, 320, 32, 128, 128)),
              ('Mixed_5c', 832, (384, 192, 384, 48, 128, 128)))

    def __init__(self, num_classes=400, spatial_squeeze=True, final_endpoint='Logits', name='inception_i3d',
                 in_channels=3, dropout_keep_prob=0.5):
        if final_endpoint not in self.VALID_ENDPOINTS:
            raise ValueError('Unknown final endpoint %s' % final_endpoint)
        if final_endpoint != 'Logits':
            # the reference returns from __init__ before registering anything (pytorch_i3d.py:207)
            raise NotImplementedError("only final_endpoint='Logits' is built; InceptionI3d.endpoint() taps the others")
        super().__init__()
        self._num_classes = num_classes
        self._spatial_squeeze = spatial_squeeze
        self._final_endpoint = final_endpoint
        self._in_channels = in_channels
        self.name = name
        # the reference registers `logits` before the endpoints (pytorch_i3d.py:279-287)
        self.logits = _Unit3D(1024, num_classes, use_batch_norm=False, use_bias=True)
        self.add_module('Conv3d_1a_7x7', _Unit3D(in_channels, 64, (7, 7, 7), stride=(2, 2, 2)))
        self.add_module('Conv3d_2b_1x1', _Unit3D(64, 64))
        self.add_module('Conv3d_2c_3x3', _Unit3D(64, 192, (3, 3, 3)))
        for mname, cin, cout in self._MIXED:
            self.add_module(mname, _InceptionModule(cin, cout))
        self.eval()
        self._handle = None

    def replace_logits(self, num_classes):
        self._num_classes = num_classes
        dev = self.logits.conv3d.weight.device
        self.logits = _Unit3D(1024, num_classes, use_batch_norm=False, use_bias=True).to(dev)
        self._handle = None

    def _state_version(self):
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def _h(self, device, N, T):
        """Native handle sized for N videos of T frames, rebuilt when the state changes (the
        mechanism of lfae._NativeModule)."""
        dev = device.index or 0
        h = self._handle
        ver = self._state_version()
        route = self._route()
        if h is None or h[0] != dev or h[1] < N or h[2] < T or h[3] != ver or h[5] != route:
            same = h is not None and h[0] == dev
            N2, T2 = max(N, h[1] if same else 0), max(T, 9, h[2] if same else 0)
            if h is not None and h[5] != route:
                self._handle = h = None  # a change of route frees the other route's workspace first
            nh = _lib.FvdHandle(self._num_classes, self._in_channels, N2, T2, dev, route)
            nh.load_state(self.state_dict())
            nh.finalize()
            self._handle = h = (dev, N2, T2, ver, nh, route)
        return h[4]

    def _check(self, x, full):
        _need_rocm(x)
        if x.dim() != 5 or x.shape[1] != self._in_channels:
            raise ValueError(f'InceptionI3d: [N, {self._in_channels}, T, H, W] expected, got {tuple(x.shape)}')
        if full:
            if x.shape[2] < 9:
                # AvgPool3d([2, 7, 7]) needs two time slots after three temporal halvings
                raise ValueError(f'InceptionI3d needs at least 9 frames, got {x.shape[2]}')
            if tuple(x.shape[3:]) != (224, 224):
                raise ValueError(f'InceptionI3d: 224 x 224 frames expected, got {tuple(x.shape[3:])}')
        return x.float().contiguous()

    def _run(self, x, want_logits):
        x = self._check(x, True)
        N, T = x.shape[0], x.shape[2]

        def run():
            h = self._h(x.device, N, T)
            with torch.cuda.device(x.device):
                if want_logits:
                    out = torch.empty(N, self._num_classes, device=x.device)
                    h.features(x, logits=out)
                    return out
                S = h.endpoint_shape(T, 224, 224, 'Mixed_5c')[1] - 1
                out = torch.empty(N, 1024, S, 1, 1, device=x.device)
                h.features(x, pooled=out)
                return out
        return self._on_route(run)

    @torch.no_grad()
    def forward(self, x):
        return self._run(x, True)

    @torch.no_grad()
    def extract_features(self, x):
        return self._run(x, False)

    @torch.no_grad()
    def endpoint(self, x, name):
        """The activation after endpoint `name` (VALID_ENDPOINTS up to Mixed_5c) for an input of
        any size: the parity hook."""
        x = self._check(x, False)
        N, _, T, H, W = x.shape
        # a handle planned for 224^2 frames holds any smaller input of the same frame count
        def run():
            h = self._h(x.device, N, T)
            with torch.cuda.device(x.device):
                out = torch.empty(N, *h.endpoint_shape(T, H, W, name), device=x.device)
                h.endpoint(x, name, out)
            return out
        return self._on_route(run)


def trans(x):
    """calculate_fvd.py:6-14: grey -> 3 channels, BTCHW -> BCTHW (a view)."""
    if x.shape[-3] == 1:
        x = x.repeat(1, 1, 3, 1, 1)
    return x.permute(0, 2, 1, 3, 4)


def preprocess_single(video, resolution=224, sequence_length=None):
    """fvd.py:161-187 for one device video [C, T, H, W] in [0, 1] -> [3, T', resolution,
    resolution] in [-1, 1] (extdm_fvd_preprocess)."""
    return _lib.fvd_preprocess(video.permute(1, 0, 2, 3)[None], sequence_length, resolution)[0]


def _preprocess_bcthw(videos):
    """preprocess_single of every video of a BCTHW batch in one launch."""
    v = videos.permute(0, 2, 1, 3, 4)
    if v.dtype != torch.float32 or v.stride(-1) != 1 or v.stride(-2) != v.shape[-1]:
        v = v.float().contiguous()
    return _lib.fvd_preprocess(v)


def get_fvd_feats(videos, i3d, device, bs=10):
    """fvd.py:43-57: videos BCTHW in [0, 1] -> float64 numpy [n, num_classes], the detector's
    pre-softmax logits, in mini-batches of bs."""
    feats = np.empty((0, i3d._num_classes))
    videos = videos.to(device)
    for i in range((len(videos) - 1) // bs + 1):
        x = _preprocess_bcthw(videos[i * bs:(i + 1) * bs])
        feats = np.vstack([feats, i3d(x).detach().cpu().numpy()])
    return feats


_I3D_FILE = 'i3d_pretrained_400.pt'


def load_i3d_pretrained(device, path=None):
    """The detector with the user's weights: a state_dict file in the public
    i3d_pretrained_400.pt layout (the loader of fvd.py:16-27). `path` defaults to that file
    name next to this module. Nothing is ever fetched."""
    import os
    path = path or os.path.join(os.path.dirname(os.path.abspath(__file__)), _I3D_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f'I3D weights not found: {path} (expected the InceptionI3d state_dict '
                                f'{_I3D_FILE}, 400 classes; pass path=... or an i3d=... detector)')
    i3d = InceptionI3d(400, in_channels=3)
    i3d.load_state_dict(torch.load(path, map_location='cpu'))
    return i3d.to(device).eval()


def get_feats(videos, device, mini_bs=10, i3d=None):
    """calculate_fvd.py:61-65: videos BTCHW in [0, 1]."""
    i3d = i3d if i3d is not None else load_i3d_pretrained(device=device)
    return get_fvd_feats(trans(videos), i3d=i3d, device=device, bs=mini_bs)


def calculate_fvd(videos1, videos2, device, i3d=None):
    """calculate_fvd.py:16-59: one FVD per clip length from 10 frames upwards."""
    assert videos1.shape == videos2.shape
    i3d = i3d if i3d is not None else load_i3d_pretrained(device=device)
    videos1, videos2 = trans(videos1), trans(videos2)
    fvd_results = {}
    for clip_timestamp in range(videos1.shape[-3]):
        if clip_timestamp < 10:
            continue
        feats1 = get_fvd_feats(videos1[:, :, :clip_timestamp], i3d=i3d, device=device)
        feats2 = get_fvd_feats(videos2[:, :, :clip_timestamp], i3d=i3d, device=device)
        fvd_results[f'[{clip_timestamp}]'] = frechet_distance(feats1, feats2)
    return {'fvd': fvd_results, 'fvd_video_setting': videos1.shape,
            'fvd_video_setting_name': 'batch_size, channel, time, heigth, width'}


def calculate_fvd1(videos1, videos2, device, mini_bs=10, i3d=None):
    """calculate_fvd.py:67-74."""
    i3d = i3d if i3d is not None else load_i3d_pretrained(device=device)
    feats1 = get_fvd_feats(trans(videos1), i3d=i3d, device=device, bs=mini_bs)
    feats2 = get_fvd_feats(trans(videos2), i3d=i3d, device=device, bs=mini_bs)
    return frechet_distance(feats1, feats2)


def calculate_fvd2(feats1, feats2):
    """calculate_fvd.py:76-77."""
    return frechet_distance(feats1, feats2)


# ---------------------------------------------------------------- LPIPS (AlexNet, version 0.1)
_LPIPS_CONVS = (('slice1', 0, 3, 64, 11, 4, 2), ('slice2', 3, 64, 192, 5, 1, 2), ('slice3', 6, 192, 384, 3, 1, 1),
                ('slice4', 8, 384, 256, 3, 1, 1), ('slice5', 10, 256, 256, 3, 1, 1))


class _ScalingLayer(nn.Module):
    """lpips.ScalingLayer: the two buffers of (inp - shift) / scale."""

    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer('scale', torch.Tensor([.458, .448, .450])[None, :, None, None])


class _AlexSlices(nn.Module):
    """Parameter holder of lpips.pretrained_networks.alexnet: the five convs under torchvision's
    `features` indices (the ReLUs and pools between them have no state)."""

    def __init__(self):
        super().__init__()
        for name, idx, cin, cout, k, s, p in _LPIPS_CONVS:
            seq = nn.Sequential()
            seq.add_module(str(idx), nn.Conv2d(cin, cout, k, stride=s, padding=p))
            self.add_module(name, seq)


class _NetLinLayer(nn.Module):
    """lpips.NetLinLayer: Dropout (identity at inference) + Conv2d(chn_in, 1, 1, bias=False)."""

    def __init__(self, chn_in):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class LPIPS(_MetricPrecision, nn.Module):
    """lpips.LPIPS(net='alex', version='0.1', lpips=True), the metric of
    metrics/calculate_lpips.py:12, on the native library. The `lpips` package is not part of the
    reference, so the network is restated from the published package: the package's
    constructor signature, its 22 state_dict entries (`scaling_layer.*`, `net.sliceK.N.*`,
    `linK.model.1.weight` and the `lins.K` aliases sharing storage), forward(in0, in1,
    retPerLayer=False, normalize=False) -> [N, 1, H, W] with spatial=True, [N, 1, 1, 1] without.
    `pretrained=True` loads nothing (there is no file to load): weights come from load_state_dict
    or load_lpips_pretrained. Inference only; inputs are [N, 1 or 3, H >= 31, W >= 31] device
    tensors in [-1, 1] ([0, 1] with normalize=True). A pair's value is bitwise independent of the
    batch it sits in. `precision` (an attribute, _MetricPrecision; not a constructor parameter and
    not in the state_dict) selects the arithmetic of the five convolutions per call through
    EXTDM_LPIPS_FP32; both routes share one native handle."""

    def __init__(self, pretrained=True, net='alex', version='0.1', lpips=True, spatial=False, pnet_rand=False,
                 pnet_tune=False, use_dropout=True, model_path=None, eval_mode=True, verbose=True):
        if net not in ('alex', 'alexnet'):
            raise NotImplementedError(f"LPIPS: only net='alex' is built, got {net!r}")
        if not lpips:
            raise NotImplementedError('LPIPS: lpips=False (unweighted feature distance) is not built')
        if version != '0.1':
            raise NotImplementedError(f"LPIPS: only version='0.1' (with the scaling layer) is built, got {version!r}")
        if not use_dropout:
            raise NotImplementedError('LPIPS: use_dropout=False changes the lin keys and is not built')
        super().__init__()
        self.pnet_type, self.pnet_tune, self.pnet_rand = 'alex', pnet_tune, pnet_rand
        self.spatial, self.lpips, self.version = spatial, lpips, version
        self.chns = [c[3] for c in _LPIPS_CONVS]
        self.L = len(self.chns)
        self.scaling_layer = _ScalingLayer()
        self.net = _AlexSlices()
        for k, c in enumerate(self.chns):
            setattr(self, f'lin{k}', _NetLinLayer(c))
        self.lins = nn.ModuleList([getattr(self, f'lin{k}') for k in range(self.L)])
        if model_path is not None:
            self.load_state_dict(torch.load(model_path, map_location='cpu'), strict=False)
        self.eval()
        self.chunk = 1024  # pairs per native launch sequence
        self._handle = None

    def _state_version(self):
        return tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def _h(self, device, N, H, W):
        """Native handle holding N pairs of H x W, rebuilt when the state changes or it is too small."""
        dev = device.index or 0
        h = self._handle
        ver = self._state_version()
        if h is None or h[0] != dev or h[1] < N or h[2] < H or h[3] < W or h[4] != ver:
            same = h is not None and h[0] == dev
            N2, H2, W2 = max(N, h[1] if same else 0), max(H, h[2] if same else 0), max(W, h[3] if same else 0)
            self._handle = None  # frees the old workspace first
            nh = _lib.LpipsHandle(N2, H2, W2, dev)
            nh.load_state(self.state_dict())
            nh.finalize()
            self._handle = h = (dev, N2, H2, W2, ver, nh)
        return h[5]

    @staticmethod
    def _images(x):
        _need_rocm(x)
        if x.dim() != 4:
            raise ValueError(f'LPIPS: [N, C, H, W] expected, got {tuple(x.shape)}')
        if x.dtype != torch.float32 or x.stride(-1) != 1 or x.stride(-2) != x.shape[-1] or x.stride(0) < 0 or \
                x.stride(1) < 0:
            x = x.float().contiguous()
        return x

    @torch.no_grad()
    def distance(self, in0, in1, flags=0, want_map=False, want_mean=True):
        """(mean [N] or None, map [N, H, W] or None) of N pairs, in chunks of self.chunk pairs."""
        in0, in1 = self._images(in0), self._images(in1)
        if in0.shape != in1.shape:
            raise ValueError('LPIPS: the two image sets must have the same shape')
        N, _, H, W = in0.shape
        _lib._lpips_images(in0, in1)
        mean = torch.empty(N, device=in0.device) if want_mean else None
        smap = torch.empty(N, H, W, device=in0.device) if want_map else None
        step = max(1, int(self.chunk))
        h = self._h(in0.device, min(N, step), H, W)

        def run():
            f = flags | (_lib.LPIPS_FP32 if self._route() == 'fp32' else 0)
            with torch.cuda.device(in0.device):
                for i in range(0, N, step):
                    j = min(N, i + step)
                    h.distance(in0[i:j], in1[i:j], f, mean[i:j] if want_mean else None,
                               smap[i:j] if want_map else None)
        self._on_route(run)
        return mean, smap

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        if retPerLayer:
            raise NotImplementedError('LPIPS: retPerLayer=True is not built')
        flags = _lib.LPIPS_NORMALIZE if normalize else 0
        if self.spatial:
            return self.distance(in0, in1, flags, want_map=True, want_mean=False)[1][:, None]
        return self.distance(in0, in1, flags | _lib.LPIPS_PLAIN_MEAN)[0][:, None, None, None]

    @torch.no_grad()
    def features(self, x, tap, normalize=False):
        """Tap 'relu1' .. 'relu5' (or 0 .. 4) of one image set, post-ReLU and un-normalised: the
        parity hook."""
        x = self._images(x)
        _lib._lpips_images(x)
        k = _lib.LPIPS_TAPS.index(tap) if isinstance(tap, str) else int(tap)
        N, _, H, W = x.shape
        h = self._h(x.device, (N + 1) // 2, H, W)

        def run():
            f = (_lib.LPIPS_NORMALIZE if normalize else 0) | (_lib.LPIPS_FP32 if self._route() == 'fp32' else 0)
            with torch.cuda.device(x.device):
                return h.features(x, k, f)
        return self._on_route(run)


def load_lpips_pretrained(device, alexnet_path, lin_path):
    """LPIPS with the two files users have: torchvision's AlexNet state_dict (`features.N.weight`
    -> `net.sliceK.N.weight`) and the package's alex.pth (`linK.model.1.weight`). Nothing is ever
    fetched."""
    import os
    for path, what in ((alexnet_path, "torchvision's AlexNet state_dict"), (lin_path, "the lpips package's alex.pth")):
        if not os.path.exists(path):
            raise FileNotFoundError(f'LPIPS weights not found: {path} ({what})')
    net = LPIPS(pretrained=False)
    alex = torch.load(alexnet_path, map_location='cpu')
    sd = {}
    for name, idx, *_ in _LPIPS_CONVS:
        for s in ('weight', 'bias'):
            key = f'features.{idx}.{s}'
            if key not in alex:
                raise KeyError(f'{alexnet_path}: missing {key}')
            sd[f'net.{name}.{idx}.{s}'] = alex[key]
    lin = torch.load(lin_path, map_location='cpu')
    for k in range(5):
        key = f'lin{k}.model.1.weight'
        if key not in lin:
            raise KeyError(f'{lin_path}: missing {key}')
        sd[key] = lin[key]
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.startswith(('lins.', 'scaling_layer.')) for m in missing), (missing, unexpected)
    return net.to(device).eval()


def lpips_trans(x):
    """calculate_lpips.py:15-23: grey -> 3 channels, [0, 1] -> [-1, 1]. The calculate_lpips*
    functions below do this inside the native stem (EXTDM_LPIPS_TRANS) instead."""
    if x.shape[-3] == 1:
        x = x.repeat(1, 1, 3, 1, 1)
    return x * 2 - 1


def _need_lpips(loss_fn):
    if loss_fn is None:
        raise ValueError('LPIPS needs a network with weights: pass loss_fn=LPIPS(...) (load_lpips_pretrained)')
    return loss_fn


def lpips_frames(videos1, videos2, device, loss_fn=None):
    """`loss_fn.forward(img1, img2).mean()` of every frame pair of two [b, t, c, h, w] videos in
    [0, 1] (the loops of calculate_lpips.py:40-60): float64 numpy [b, t]. All b * t pairs run
    through the native handle as one batch, in chunks."""
    loss_fn = _need_lpips(loss_fn)
    assert videos1.shape == videos2.shape  # calculate_lpips.py:29
    if videos1.dim() != 5:
        raise ValueError('expected [b, t, c, h, w] videos')
    b, t = videos1.shape[:2]
    v1, v2 = videos1.to(device).flatten(0, 1), videos2.to(device).flatten(0, 1)
    flags = _lib.LPIPS_TRANS | (0 if loss_fn.spatial else _lib.LPIPS_PLAIN_MEAN)
    mean = loss_fn.distance(v1, v2, flags)[0]
    return mean.double().cpu().numpy().reshape(b, t)


def calculate_lpips(videos1, videos2, device, loss_fn=None):
    """metrics/calculate_lpips.py:25-76: mean / std over videos per frame index. The reference
    indexes its list of lists with [:, t] (line 66) and raises TypeError; this is the evident
    np.array form (DESIGN, reference defects)."""
    v = lpips_frames(videos1, videos2, device, loss_fn)
    shape = list(videos1.shape[2:])
    if shape[0] == 1:
        shape[0] = 3  # the reference reports the shape after trans
    return {'lpips': {f'avg[{i}]': np.mean(v[:, i]) for i in range(v.shape[1])},
            'lpips_std': {f'std[{i}]': np.std(v[:, i]) for i in range(v.shape[1])},
            'lpips_video_setting': torch.Size([videos1.shape[1]] + shape),
            'lpips_video_setting_name': 'time, channel, heigth, width'}


def calculate_lpips1(videos1, videos2, device, loss_fn=None):
    """metrics/calculate_lpips.py:78-95: (mean, std) over every frame."""
    v = lpips_frames(videos1, videos2, device, loss_fn)
    return np.mean(v), np.std(v)


def calculate_lpips2(videos1, videos2, device, loss_fn=None):
    """metrics/calculate_lpips.py:97-115: the best of the n samples, min over n of the per-sample
    mean over frames."""
    v = lpips_frames(videos1, videos2, device, loss_fn)
    return np.min(np.mean(v, axis=-1))


def calculate_lpips3(videos1, videos2, device, loss_fn=None):
    """metrics/calculate_lpips.py:117-135: the per-video mean over frames."""
    v = lpips_frames(videos1, videos2, device, loss_fn)
    return np.mean(v, axis=-1)


def best_of_n_lpips(origin_videos, result_videos, cond_frames, loss_fn):
    """valid.py:222-228: calculate_lpips2 of each clip's n samples over the predicted frames.
    origin_videos, result_videos: [b, n, t, c, h, w]. One value per clip; all b * n * t pairs go
    through the handle as one batch (a pair's value does not depend on its batch)."""
    b, n = result_videos.shape[:2]
    a = origin_videos[:, :, cond_frames:].flatten(0, 1)
    r = result_videos[:, :, cond_frames:].flatten(0, 1)
    v = lpips_frames(a, r, result_videos.device, loss_fn).reshape(b, n, -1)
    return [np.min(np.mean(v[i], axis=-1)) for i in range(b)]
