"""ctypes binding of libextdm_hip.so (include/extdm.h). The library is the
product path: if it is missing or no HIP device is visible, every entry point
raises — there is no CPU or eager-PyTorch fallback."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('EXTDM_LIB') or os.path.join(HERE, 'libextdm_hip.so')

# every symbol include/extdm.h declares
EXPORTS = ['extdm_create', 'extdm_destroy', 'extdm_last_error', 'extdm_load_weight', 'extdm_finalize',
           'extdm_workspace_bytes', 'extdm_unet_forward', 'extdm_sample', 'extdm_sampler_step', 'extdm_record_thresholds', 'extdm_bench_layer', 'extdm_bench_layer_kernel',
           'extdm_decode', 'extdm_set_lfae', 'extdm_region_params', 'extdm_region_hw', 'extdm_bg_params',
           'extdm_flow_predict', 'extdm_flow_hw', 'extdm_bottleneck', 'extdm_range_flag',
           'extdm_attn_layer', 'extdm_frame_metrics_workspace', 'extdm_frame_metrics', 'extdm_bilinear_frames',
           'extdm_sampler_step_t', 'extdm_sampler_step_hist', 'extdm_q_sample', 'extdm_p_losses', 'extdm_abs_diff_chunks', 'extdm_abs_diff_sum',
           'extdm_fvd_create', 'extdm_fvd_destroy', 'extdm_fvd_load_weight', 'extdm_fvd_finalize',
           'extdm_fvd_preprocess', 'extdm_fvd_features', 'extdm_fvd_endpoint', 'extdm_fvd_endpoint_shape',
           'extdm_fvd_range_flag', 'extdm_fvd_same_pad', 'extdm_fvd_maxpool', 'extdm_fvd_set_precision',
           'extdm_lpips_create', 'extdm_lpips_destroy', 'extdm_lpips_load_weight', 'extdm_lpips_finalize',
           'extdm_lpips_distance', 'extdm_lpips_features', 'extdm_lpips_feature_shape', 'extdm_lpips_maxpool',
           'extdm_lpips_mean_weights', 'extdm_lpips_range_flag']
# ... and the declared symbols whose names hold a digit: tests/test_abi.py scans the header for
# lower-case names only, so they are listed apart (tests/test_teacher_cpu.py checks them)
EXPORTS_DIGIT = ['extdm_x0_loss']

BG_TYPES = {'zero': 0, 'shift': 1, 'affine': 2, 'perspective': 3}

SAMPLER_DDPM = 0
SAMPLER_DDIM = 1
SAMPLER_DPMPP = 2  # DPM-Solver++(2M)
LOSS_TYPES = {'l1': 0, 'l2': 1}  # include/extdm.h EXTDM_LOSS_*

# include/extdm.h EXTDM_PRECISION_*: arithmetic of the direct convolutions ('f16_conv' / 'f16': one
# fp16 MFMA term per product in the denoiser forward's convs, 'f16' with the bf16 attention too)
PRECISIONS = {'fp32': 0, 'f16x3': 1, 'bf16_attn': 2, 'f16_conv': 3, 'f16': 4}
DEFAULT_PRECISION = os.environ.get('EXTDM_PRECISION', 'f16x3')

class ExtdmConfig(ctypes.Structure):
    _fields_ = [('arch', ctypes.c_int), ('dim', ctypes.c_int), ('channels', ctypes.c_int),
                ('dim_mults', ctypes.c_int * 4), ('n_levels', ctypes.c_int), ('window', ctypes.c_int * 3),
                ('heads', ctypes.c_int), ('dim_head', ctypes.c_int), ('tc', ctypes.c_int), ('tp', ctypes.c_int),
                ('latent', ctypes.c_int), ('fea_size', ctypes.c_int), ('fea_ch', ctypes.c_int),
                ('timesteps', ctypes.c_int), ('max_batch', ctypes.c_int), ('device', ctypes.c_int),
                ('image', ctypes.c_int), ('num_channels', ctypes.c_int), ('gen_block_expansion', ctypes.c_int),
                ('gen_max_features', ctypes.c_int), ('gen_num_down_blocks', ctypes.c_int),
                ('gen_num_bottleneck_blocks', ctypes.c_int), ('precision', ctypes.c_int)]


class ExtdmLfaeConfig(ctypes.Structure):
    _fields_ = [('num_regions', ctypes.c_int), ('num_channels', ctypes.c_int), ('image', ctypes.c_int),
                ('revert_axis_swap', ctypes.c_int), ('rp_temperature', ctypes.c_float),
                ('rp_scale_factor', ctypes.c_float), ('rp_pad', ctypes.c_int), ('rp_num_blocks', ctypes.c_int),
                ('rp_pca_based', ctypes.c_int), ('bg_type', ctypes.c_int), ('bg_num_blocks', ctypes.c_int),
                ('pf_scale_factor', ctypes.c_float), ('pf_region_var', ctypes.c_float),
                ('pf_num_blocks', ctypes.c_int), ('pf_use_covar_heatmap', ctypes.c_int),
                ('pf_use_deformed_source', ctypes.c_int)]


_lib = None


def load():
    """Load the shared library and declare the signatures."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'ExtDM HIP library not built: {LIB_PATH} (run __graft_entry__.build())')
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    L.extdm_create.argtypes = [ctypes.POINTER(ExtdmConfig), ctypes.POINTER(vp)]
    L.extdm_create.restype = i32
    L.extdm_destroy.argtypes = [vp]
    L.extdm_destroy.restype = None
    L.extdm_last_error.argtypes = []
    L.extdm_last_error.restype = ctypes.c_char_p
    L.extdm_load_weight.argtypes = [vp, ctypes.c_char_p, vp, i32, ctypes.POINTER(i64), i32]
    L.extdm_load_weight.restype = i32
    L.extdm_finalize.argtypes = [vp]
    L.extdm_finalize.restype = i32
    L.extdm_workspace_bytes.argtypes = [vp]
    L.extdm_workspace_bytes.restype = i64
    L.extdm_unet_forward.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.extdm_unet_forward.restype = i32
    L.extdm_sample.argtypes = [vp, i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), f32, vp, vp, vp, vp,
                               u64, i32, i32, vp, i32, vp]
    L.extdm_sample.restype = i32
    L.extdm_sampler_step.argtypes = [vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp]
    L.extdm_sampler_step.restype = i32
    L.extdm_record_thresholds.argtypes = [vp, vp, i64]
    L.extdm_record_thresholds.restype = i32
    L.extdm_bench_layer.argtypes = [vp, i32, i32, i32, ctypes.POINTER(f32), ctypes.POINTER(ctypes.c_double)]
    L.extdm_bench_layer.restype = i32
    L.extdm_bench_layer_kernel.argtypes = [vp, i32, ctypes.c_char_p, i32]
    L.extdm_bench_layer_kernel.restype = i32
    L.extdm_decode.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.extdm_decode.restype = i32
    L.extdm_set_lfae.argtypes = [vp, ctypes.POINTER(ExtdmLfaeConfig)]
    L.extdm_set_lfae.restype = i32
    L.extdm_region_params.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.extdm_region_params.restype = i32
    L.extdm_region_hw.argtypes = [vp]
    L.extdm_region_hw.restype = i32
    L.extdm_bg_params.argtypes = [vp, i32, vp, vp, vp, vp]
    L.extdm_bg_params.restype = i32
    L.extdm_flow_predict.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.extdm_flow_predict.restype = i32
    L.extdm_flow_hw.argtypes = [vp]
    L.extdm_flow_hw.restype = i32
    L.extdm_bottleneck.argtypes = [vp, i32, vp, vp, vp]
    L.extdm_bottleneck.restype = i32
    L.extdm_attn_layer.argtypes = [vp, ctypes.c_char_p, i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.extdm_attn_layer.restype = i32
    L.extdm_range_flag.argtypes = [vp, i32, vp]
    L.extdm_range_flag.restype = i32
    L.extdm_frame_metrics_workspace.argtypes = [i32, i32, i32, i32, i32]
    L.extdm_frame_metrics_workspace.restype = ctypes.c_size_t
    L.extdm_frame_metrics.argtypes = [vp, vp, i32, i32, i32, i32, i32, ctypes.c_long, ctypes.c_long, ctypes.c_long,
                                      vp, vp, vp, vp]
    L.extdm_frame_metrics.restype = i32
    lg = ctypes.c_long
    L.extdm_bilinear_frames.argtypes = [vp, i32, i32, i32, i32, i32, vp, lg, lg, lg, vp, lg, lg, lg, i32, i32, i32, vp]
    L.extdm_bilinear_frames.restype = i32
    L.extdm_sampler_step_t.argtypes = [vp, i32, i32, vp, vp, f32, vp, vp, vp, vp, vp]
    L.extdm_sampler_step_t.restype = i32
    L.extdm_sampler_step_hist.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.extdm_sampler_step_hist.restype = i32
    L.extdm_q_sample.argtypes = [vp, i32, vp, vp, vp, u64, i32, i32, vp, vp, vp]
    L.extdm_q_sample.restype = i32
    L.extdm_x0_loss.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    L.extdm_x0_loss.restype = i32
    L.extdm_p_losses.argtypes = [vp, i32, vp, vp, vp, vp, vp, u64, i32, i32, i32, i32, vp, vp, vp]
    L.extdm_p_losses.restype = i32
    L.extdm_abs_diff_chunks.argtypes = [i32]
    L.extdm_abs_diff_chunks.restype = i32
    L.extdm_abs_diff_sum.argtypes = [vp, vp, i32, i32, vp, vp, vp]
    L.extdm_abs_diff_sum.restype = i32
    L.extdm_fvd_create.argtypes = [i32, i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.extdm_fvd_create.restype = i32
    L.extdm_fvd_destroy.argtypes = [vp]
    L.extdm_fvd_destroy.restype = None
    L.extdm_fvd_load_weight.argtypes = [vp, ctypes.c_char_p, vp, i32, ctypes.POINTER(i64), i32]
    L.extdm_fvd_load_weight.restype = i32
    L.extdm_fvd_set_precision.argtypes = [vp, i32]
    L.extdm_fvd_set_precision.restype = i32
    L.extdm_fvd_finalize.argtypes = [vp]
    L.extdm_fvd_finalize.restype = i32
    L.extdm_fvd_preprocess.argtypes = [vp, i32, i32, i32, i32, i32, lg, lg, lg, i32, i32, vp, vp]
    L.extdm_fvd_preprocess.restype = i32
    L.extdm_fvd_features.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    L.extdm_fvd_features.restype = i32
    L.extdm_fvd_endpoint.argtypes = [vp, i32, i32, i32, i32, vp, ctypes.c_char_p, vp, vp]
    L.extdm_fvd_endpoint.restype = i32
    L.extdm_fvd_endpoint_shape.argtypes = [vp, i32, i32, i32, ctypes.c_char_p, ctypes.POINTER(i32)]
    L.extdm_fvd_endpoint_shape.restype = i32
    L.extdm_fvd_range_flag.argtypes = [vp, i32, vp]
    L.extdm_fvd_range_flag.restype = i32
    L.extdm_fvd_same_pad.argtypes = [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.extdm_fvd_same_pad.restype = i32
    L.extdm_fvd_maxpool.argtypes = [vp] + [i32] * 11 + [vp, vp]
    L.extdm_fvd_maxpool.restype = i32
    L.extdm_lpips_create.argtypes = [i32, i32, i32, i32, ctypes.POINTER(vp)]
    L.extdm_lpips_create.restype = i32
    L.extdm_lpips_destroy.argtypes = [vp]
    L.extdm_lpips_destroy.restype = None
    L.extdm_lpips_load_weight.argtypes = [vp, ctypes.c_char_p, vp, i32, ctypes.POINTER(i64), i32]
    L.extdm_lpips_load_weight.restype = i32
    L.extdm_lpips_finalize.argtypes = [vp]
    L.extdm_lpips_finalize.restype = i32
    L.extdm_lpips_distance.argtypes = [vp, i32, i32, i32, i32, vp, lg, lg, vp, lg, lg, i32, vp, vp, vp]
    L.extdm_lpips_distance.restype = i32
    L.extdm_lpips_features.argtypes = [vp, i32, i32, i32, i32, vp, lg, lg, i32, i32, vp, vp]
    L.extdm_lpips_features.restype = i32
    L.extdm_lpips_feature_shape.argtypes = [i32, i32, i32, ctypes.POINTER(i32)]
    L.extdm_lpips_feature_shape.restype = i32
    L.extdm_lpips_maxpool.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    L.extdm_lpips_maxpool.restype = i32
    L.extdm_lpips_mean_weights.argtypes = [i32, i32, ctypes.POINTER(ctypes.c_double)]
    L.extdm_lpips_mean_weights.restype = i32
    L.extdm_lpips_range_flag.argtypes = [vp, i32, vp]
    L.extdm_lpips_range_flag.restype = i32
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError('extdm: ' + load().extdm_last_error().decode())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bilinear_frames(a, b, t_split, T, size):
    """Bilinear resize (align_corners=False) into a new contiguous [B, C, T, size, size] tensor:
    frames t < t_split from a[:, :, t], the rest from b[:, :, t - t_split] (b may have a frame
    stride of 0, e.g. an expand()ed single frame). a / b: CUDA fp32 [B, C, t, H, W] with
    contiguous H*W planes (extdm_bilinear_frames)."""
    import torch
    src = a if a is not None else b
    Bn, C, _, H, W = src.shape
    out = torch.empty(Bn, C, T, size[0], size[1], device=src.device, dtype=torch.float32)
    for x in (a, b):
        if x is not None:
            if not x.is_cuda:
                raise RuntimeError('ExtDM HIP path needs tensors on a ROCm device (no CPU fallback)')
            if x.dtype != torch.float32 or x.stride(-1) != 1 or x.stride(-2) != x.shape[-1] or x.shape[-2:] != (H, W):
                raise ValueError('bilinear_frames: fp32 [B, C, t, H, W] with contiguous planes expected')
    sa = a.stride()[:3] if a is not None else (0, 0, 0)
    sb = b.stride()[:3] if b is not None else (0, 0, 0)
    with torch.cuda.device(src.device):
        check(load().extdm_bilinear_frames(_ptr(out), Bn, C, T, size[0], size[1], _ptr(a), *sa, _ptr(b), *sb, t_split,
                                           H, W, _stream()))
    return out


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_device(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError('ExtDM HIP path needs tensors on a ROCm device (no CPU fallback)')
        if not t.is_contiguous() or t.dtype.is_floating_point and t.dtype != __import__('torch').float32:
            raise RuntimeError('ExtDM HIP path needs contiguous float32 tensors')


def _require_i64(*ts):
    """The t vectors of the teacher-forced entry points: the library reads B int64 values."""
    import torch
    for t in ts:
        if t is not None and t.dtype != torch.int64:
            raise RuntimeError(f'ExtDM HIP path needs int64 timestep tensors, got {t.dtype}')


def _require_f64(t, numel):
    import torch
    if not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < numel:
        raise RuntimeError(f'ExtDM HIP path needs a contiguous float64 device tensor of at least {numel} elements')


def abs_diff_sum(a, b):
    """Per-sample sums of |a - b| over everything but dim 0 -> device float64 [B], fixed summation
    order (extdm_abs_diff_sum)."""
    import torch
    _require_device(a, b)
    if a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError('abs_diff_sum: two float32 tensors of one shape expected')
    B = a.shape[0]
    n = a.numel() // B
    if n >= 2 ** 31:
        raise ValueError('abs_diff_sum: at most 2^31 - 1 elements per sample')
    L = load()
    sums = torch.empty(B, device=a.device, dtype=torch.float64)
    work = torch.empty(B * L.extdm_abs_diff_chunks(n), device=a.device, dtype=torch.float64)
    with torch.cuda.device(a.device):
        check(L.extdm_abs_diff_sum(_ptr(a), _ptr(b), B, n, _ptr(sums), _ptr(work), _stream()))
    return sums


class Handle:
    """One native model instance (Unet3D weights + diffusion buffers [+ decoder])."""

    def __init__(self, ucfg, timesteps, max_batch, device=0, gcfg=None, precision=None):
        L = load()
        c = ExtdmConfig()
        from .spec import ARCH_IDS
        c.arch = ARCH_IDS[ucfg.arch]
        c.dim = ucfg.dim
        c.channels = ucfg.channels
        mults = list(ucfg.dim_mults)
        for i, m in enumerate(mults):
            c.dim_mults[i] = m
        c.n_levels = len(mults)
        for i, w in enumerate(ucfg.window):
            c.window[i] = w
        c.heads = ucfg.heads
        c.dim_head = ucfg.dim_head
        c.tc, c.tp = ucfg.tc, ucfg.tp
        c.latent = ucfg.latent
        c.fea_size = ucfg.fea_size
        c.fea_ch = ucfg.fea_ch
        c.timesteps = timesteps
        c.max_batch = max_batch
        c.device = device
        if gcfg is None:
            from .spec import GeneratorConfig
            gcfg = GeneratorConfig(image=2 * ucfg.latent)
        c.image = gcfg.image
        c.num_channels = gcfg.num_channels
        c.gen_block_expansion = gcfg.block_expansion
        c.gen_max_features = gcfg.max_features
        c.gen_num_down_blocks = gcfg.num_down_blocks
        c.gen_num_bottleneck_blocks = gcfg.num_bottleneck_blocks
        self.precision = precision or DEFAULT_PRECISION
        if self.precision not in PRECISIONS:
            raise ValueError(f'precision must be one of {sorted(PRECISIONS)}, got {self.precision!r}')
        c.precision = PRECISIONS[self.precision]
        self.cfg = ucfg
        self.max_batch = max_batch
        self.timesteps = timesteps
        h = ctypes.c_void_p()
        check(L.extdm_create(ctypes.byref(c), ctypes.byref(h)))
        self.h = h
        self.n = 3 * ucfg.tp * ucfg.latent * ucfg.latent

    def __del__(self):
        if getattr(self, 'h', None) and _lib is not None:
            _lib.extdm_destroy(self.h)
            self.h = None

    def load_state(self, sd):
        """sd: name -> CPU tensor (float32 or int64)."""
        import torch
        L = load()
        for name, t in sd.items():
            t = t.detach().to('cpu').contiguous()
            if t.dtype == torch.int64:
                dt = 1
            else:
                t = t.to(torch.float32)
                dt = 0
            shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
            check(L.extdm_load_weight(self.h, name.encode(), ctypes.c_void_p(t.data_ptr()), dt, shape, t.dim()))

    def finalize(self):
        check(load().extdm_finalize(self.h))

    def workspace_bytes(self):
        return int(load().extdm_workspace_bytes(self.h))

    def unet_forward(self, x, t, cond, fea, out):
        _require_device(x, cond, fea, out)
        check(load().extdm_unet_forward(self.h, x.shape[0], _ptr(x), _ptr(t), _ptr(cond), _ptr(fea), _ptr(out),
                                        _stream()))

    def sample(self, sampler, times, times_next, eta, x_cond, cond_fea, out, x_T=None, noise=None, seed=0,
               sample_base=0, round_idx=0, use_graph=True):
        _require_device(x_cond, cond_fea, out, x_T, noise)
        S = len(times)
        ta = (ctypes.c_int * S)(*times)
        tn = (ctypes.c_int * S)(*(times_next if times_next is not None else [0] * S))
        check(load().extdm_sample(self.h, out.shape[0], sampler, S, ta, tn, float(eta), _ptr(x_cond),
                                  _ptr(cond_fea), _ptr(x_T), _ptr(noise), ctypes.c_uint64(seed), sample_base,
                                  round_idx, _ptr(out), 1 if use_graph else 0, _stream()))

    def sampler_step(self, sampler, t, t_next, eta, x, eps, noise=None, thresh_out=None):
        _require_device(x, eps, noise, thresh_out)
        check(load().extdm_sampler_step(self.h, x.shape[0], sampler, int(t), int(t_next), float(eta), _ptr(x),
                                        _ptr(eps), _ptr(noise), _ptr(thresh_out), _stream()))

    def sampler_step_hist(self, t_prev, t, t_next, x, eps, x0_prev, thresh_out=None):
        """One DPM-Solver++(2M) update in place on x and x0_prev (t_prev < 0: first step, t_next < 0:
        final step)."""
        _require_device(x, eps, x0_prev, thresh_out)
        check(load().extdm_sampler_step_hist(self.h, x.shape[0], int(t_prev), int(t), int(t_next), _ptr(x), _ptr(eps),
                                             _ptr(x0_prev), _ptr(thresh_out), _stream()))

    # ---- teacher-forced evaluation step (include/extdm.h); every t is a device int64 [B] ----
    def sampler_step_t(self, sampler, t, t_next, eta, x, eps, noise=None, thresh_out=None):
        _require_device(x, eps, noise, thresh_out, t, t_next)
        _require_i64(t, t_next)
        check(load().extdm_sampler_step_t(self.h, x.shape[0], sampler, _ptr(t), _ptr(t_next), float(eta), _ptr(x),
                                          _ptr(eps), _ptr(noise), _ptr(thresh_out), _stream()))

    def q_sample(self, t, x0, x_t, noise=None, seed=0, sample_base=0, round_idx=0, noise_out=None):
        _require_device(t, x0, x_t, noise, noise_out)
        _require_i64(t)
        check(load().extdm_q_sample(self.h, x0.shape[0], _ptr(t), _ptr(x0), _ptr(noise), ctypes.c_uint64(seed),
                                    sample_base, round_idx, _ptr(noise_out), _ptr(x_t), _stream()))

    def x0_loss(self, t, x_t, eps, noise, loss_type, clip_denoised, pred_x0, loss_sum, thresh_out=None):
        """loss_sum: device float64 [B]."""
        _require_device(t, x_t, eps, noise, pred_x0, thresh_out)
        _require_i64(t)
        _require_f64(loss_sum, x_t.shape[0])
        check(load().extdm_x0_loss(self.h, x_t.shape[0], _ptr(t), _ptr(x_t), _ptr(eps), _ptr(noise),
                                   LOSS_TYPES[loss_type], 1 if clip_denoised else 0, _ptr(pred_x0), _ptr(loss_sum),
                                   _ptr(thresh_out), _stream()))

    def p_losses(self, t, x_cond, x_start, cond_fea, loss_type, clip_denoised, pred_x0, loss_sum, noise=None, seed=0,
                 sample_base=0, round_idx=0):
        _require_device(t, x_cond, x_start, cond_fea, pred_x0, noise)
        _require_i64(t)
        _require_f64(loss_sum, x_start.shape[0])
        check(load().extdm_p_losses(self.h, x_start.shape[0], _ptr(t), _ptr(x_cond), _ptr(x_start), _ptr(cond_fea),
                                    _ptr(noise), ctypes.c_uint64(seed), sample_base, round_idx,
                                    LOSS_TYPES[loss_type], 1 if clip_denoised else 0, _ptr(pred_x0), _ptr(loss_sum),
                                    _stream()))

    def record_thresholds(self, buf):
        """Record every later sample() call's per-step thresholds into buf[k * B + b] (device
        fp32; None stops). The tensor must stay alive while recording is on."""
        _require_device(buf)
        self._thresh_buf = buf
        check(load().extdm_record_thresholds(self.h, _ptr(buf), 0 if buf is None else buf.numel()))

    def range_flag(self, reset=True):
        """1 if an f16x3 conv input reached |v| >= 65504 since the last reset."""
        rc = load().extdm_range_flag(self.h, 1 if reset else 0, _stream())
        if rc < 0:
            check(rc)
        return rc

    def attn_layer(self, prefix, x, out, shifted=False):
        """One attention layer (STW or temporal) of the forward: x, out (B,C,T,H,W)."""
        _require_device(x, out)
        B, C, T, H, W = x.shape
        check(load().extdm_attn_layer(self.h, prefix.encode(), B, C, T, H, W, int(shifted), _ptr(x), _ptr(out),
                                      _stream()))

    def bench_layer(self, B, layer=0, iters=20):
        ms, fl = ctypes.c_float(), ctypes.c_double()
        check(load().extdm_bench_layer(self.h, B, layer, iters, ctypes.byref(ms), ctypes.byref(fl)))
        return float(ms.value), float(fl.value)

    def bench_layer_kernel(self, layer):
        """The kernel template the last bench_layer(layer) launched ('' if not recorded)."""
        buf = ctypes.create_string_buffer(256)
        check(load().extdm_bench_layer_kernel(self.h, layer, buf, 256))
        return buf.value.decode()

    # ---- LFAE encoder (include/extdm.h) ----
    def set_lfae(self, lc):
        c = ExtdmLfaeConfig()
        c.num_regions, c.num_channels, c.image = lc.num_regions, lc.num_channels, lc.image
        c.revert_axis_swap = int(lc.revert_axis_swap)
        c.rp_temperature, c.rp_scale_factor = lc.rp_temperature, lc.rp_scale_factor
        c.rp_pad, c.rp_num_blocks, c.rp_pca_based = lc.rp_pad, lc.rp_num_blocks, int(lc.rp_pca_based)
        c.bg_type, c.bg_num_blocks = BG_TYPES[lc.bg_type], lc.bg_num_blocks
        c.pf_scale_factor, c.pf_region_var = lc.pf_scale_factor, lc.pf_region_var
        c.pf_num_blocks = lc.pf_num_blocks
        c.pf_use_covar_heatmap, c.pf_use_deformed_source = int(lc.pf_use_covar_heatmap), int(lc.pf_use_deformed_source)
        check(load().extdm_set_lfae(self.h, ctypes.byref(c)))

    def region_hw(self):
        return int(load().extdm_region_hw(self.h))

    def flow_hw(self):
        return int(load().extdm_flow_hw(self.h))

    def region_params(self, img, shift, covar, affine, u=None, sv=None, heat=None):
        _require_device(img, shift, covar, affine, u, sv, heat)
        check(load().extdm_region_params(self.h, img.shape[0], _ptr(img), _ptr(shift), _ptr(covar), _ptr(affine),
                                         _ptr(u), _ptr(sv), _ptr(heat), _stream()))

    def bg_params(self, src, drv, out):
        _require_device(src, drv, out)
        check(load().extdm_bg_params(self.h, out.shape[0], _ptr(src), _ptr(drv), _ptr(out), _stream()))

    def flow_predict(self, src, drv, srcp, bg, flow, occ=None):
        """drv / srcp: dicts with contiguous 'shift', 'covar', 'affine' device tensors."""
        _require_device(src, bg, flow, occ, *[d[k] for d in (drv, srcp) for k in ('shift', 'covar', 'affine')])
        check(load().extdm_flow_predict(self.h, src.shape[0], _ptr(src), _ptr(drv['shift']), _ptr(drv['covar']),
                                        _ptr(drv['affine']), _ptr(srcp['shift']), _ptr(srcp['covar']),
                                        _ptr(srcp['affine']), _ptr(bg), _ptr(flow), _ptr(occ), _stream()))

    def bottleneck(self, img, out):
        _require_device(img, out)
        check(load().extdm_bottleneck(self.h, img.shape[0], _ptr(img), _ptr(out), _stream()))

    def decode(self, ref, flow, out, occ=None, warped=None):
        """ref (B,C,S,S), flow (B,2,T,fh,fw), occ (B,1,T,fh,fw) or None -> out (B,C,T,S,S)."""
        _require_device(ref, flow, out, occ, warped)
        B, C, S, _ = ref.shape
        T, fh, fw = flow.shape[2], flow.shape[3], flow.shape[4]
        check(load().extdm_decode(self.h, B, C, T, S, fh, fw, _ptr(ref), _ptr(flow), _ptr(occ), _ptr(out),
                                  _ptr(warped), _stream()))


def fvd_preprocess(videos, sequence_length=None, resolution=224):
    """trans + preprocess_single of every video in one launch (extdm_fvd_preprocess): fp32 device
    [B, T, C, H, W] in [0, 1] with contiguous planes, C in {1, 3} -> [B, 3, T', resolution,
    resolution] in [-1, 1]."""
    import torch
    if not videos.is_cuda:
        raise RuntimeError('ExtDM HIP path needs tensors on a ROCm device (no CPU fallback)')
    if videos.dim() != 5 or videos.dtype != torch.float32 or videos.stride(-1) != 1 or \
            videos.stride(-2) != videos.shape[-1]:
        raise ValueError('fvd_preprocess: fp32 [B, T, C, H, W] with contiguous planes expected')
    B, T, C, H, W = videos.shape
    if C not in (1, 3):
        raise ValueError('fvd_preprocess: 1 or 3 channels expected')
    if sequence_length is not None and sequence_length > T:
        raise AssertionError('sequence_length exceeds the clip')  # fvd.py:167
    To = T if sequence_length is None else int(sequence_length)
    out = torch.empty(B, 3, To, resolution, resolution, device=videos.device, dtype=torch.float32)
    with torch.cuda.device(videos.device):
        check(load().extdm_fvd_preprocess(_ptr(videos), B, T, C, H, W, *videos.stride()[:3], To, resolution,
                                          _ptr(out), _stream()))
    return out


# InceptionI3d's convolutions: the f16x3 route or the exact-fp32 one (extdm_fvd_set_precision)
FVD_PRECISIONS = ('f16x3', 'fp32')


def _fvd_precision(precision):
    if precision not in FVD_PRECISIONS:
        raise ValueError(f'precision must be one of {FVD_PRECISIONS}, got {precision!r}')
    return PRECISIONS[precision]


class FvdHandle:
    """One native InceptionI3d instance (include/extdm.h, extdm_fvd_*)."""

    def __init__(self, num_classes, in_channels, max_batch, max_frames, device=0, precision='f16x3'):
        mode = _fvd_precision(precision)
        h = ctypes.c_void_p()
        check(load().extdm_fvd_create(num_classes, in_channels, max_batch, max_frames, device, ctypes.byref(h)))
        self.h = h
        self.precision = precision
        check(load().extdm_fvd_set_precision(h, mode))
        self.num_classes, self.in_channels = num_classes, in_channels
        self.max_batch, self.max_frames = max_batch, max_frames

    def __del__(self):
        if getattr(self, 'h', None) and _lib is not None:
            _lib.extdm_fvd_destroy(self.h)
            self.h = None

    def load_state(self, sd):
        """sd: reference state_dict key -> tensor."""
        import torch
        L = load()
        for name, t in sd.items():
            t = t.detach().to('cpu').contiguous()
            if t.dtype == torch.int64:
                dt = 1
            else:
                t = t.to(torch.float32)
                dt = 0
            shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
            check(L.extdm_fvd_load_weight(self.h, name.encode(), ctypes.c_void_p(t.data_ptr()), dt, shape, t.dim()))

    def finalize(self):
        check(load().extdm_fvd_finalize(self.h))

    def features(self, x, logits=None, pooled=None):
        _require_device(x, logits, pooled)
        check(load().extdm_fvd_features(self.h, x.shape[0], x.shape[2], _ptr(x), _ptr(logits), _ptr(pooled),
                                        _stream()))

    def endpoint_shape(self, T, H, W, name):
        d = (ctypes.c_int * 4)()
        check(load().extdm_fvd_endpoint_shape(self.h, T, H, W, name.encode(), d))
        return tuple(d)

    def endpoint(self, x, name, out):
        _require_device(x, out)
        N, _, T, H, W = x.shape
        check(load().extdm_fvd_endpoint(self.h, N, T, H, W, _ptr(x), name.encode(), _ptr(out), _stream()))

    def range_flag(self, reset=True):
        rc = load().extdm_fvd_range_flag(self.h, 1 if reset else 0, _stream())
        if rc < 0:
            check(rc)
        return rc


LPIPS_NORMALIZE, LPIPS_TRANS, LPIPS_PLAIN_MEAN = 1, 2, 4  # include/extdm.h EXTDM_LPIPS_*
LPIPS_FP32 = 8  # EXTDM_LPIPS_FP32: this call's convolutions on the exact-fp32 kernel (csrc/lpips_f32.hip)
LPIPS_TAPS = ('relu1', 'relu2', 'relu3', 'relu4', 'relu5')


def lpips_mean_weights(n_in, n_out):
    """extdm_lpips_mean_weights: float64 numpy [n_in], the column means of the bilinear
    (align_corners=False) interpolation matrix from n_in to n_out samples. No device needed."""
    import numpy as np
    w = (ctypes.c_double * n_in)()
    if load().extdm_lpips_mean_weights(n_in, n_out, w) != 0:
        raise ValueError('lpips_mean_weights: positive sizes expected')
    return np.array(w[:], dtype=np.float64)


def lpips_feature_shape(H, W, tap):
    """(C, h, w) of tap 0 .. 4 = relu1 .. relu5 for an H x W input (extdm_lpips_feature_shape)."""
    d = (ctypes.c_int * 3)()
    check(load().extdm_lpips_feature_shape(H, W, tap, d))
    return tuple(d)


def lpips_maxpool(x):
    """nn.MaxPool2d(3, 2) of a contiguous fp32 device [B, C, H, W] (extdm_lpips_maxpool)."""
    import torch
    _require_device(x)
    B, C, H, W = x.shape
    out = torch.empty(B, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        check(load().extdm_lpips_maxpool(_ptr(x), B, C, H, W, _ptr(out), _stream()))
    return out


def _lpips_images(*ts):
    """fp32 device [N, C, H, W] image sets with contiguous planes (batch / channel strides free)."""
    import torch
    for x in ts:
        if not x.is_cuda:
            raise RuntimeError('ExtDM HIP path needs tensors on a ROCm device (no CPU fallback)')
        if x.dim() != 4 or x.dtype != torch.float32 or x.stride(-1) != 1 or x.stride(-2) != x.shape[-1] or \
                x.stride(0) < 0 or x.stride(1) < 0:
            raise ValueError('lpips: fp32 [N, C, H, W] with contiguous planes expected')
        if x.shape[1] not in (1, 3):
            raise ValueError('lpips: 1 or 3 channels expected')
        if x.shape[2] < 31 or x.shape[3] < 31:
            raise ValueError(f'lpips: H and W must be at least 31, got {x.shape[2]} x {x.shape[3]}')


class LpipsHandle:
    """One native LPIPS (AlexNet, version 0.1) instance (include/extdm.h, extdm_lpips_*)."""

    def __init__(self, max_pairs, max_h, max_w, device=0):
        h = ctypes.c_void_p()
        check(load().extdm_lpips_create(max_pairs, max_h, max_w, device, ctypes.byref(h)))
        self.h = h
        self.max_pairs, self.max_h, self.max_w = max_pairs, max_h, max_w

    def __del__(self):
        if getattr(self, 'h', None) and _lib is not None:
            _lib.extdm_lpips_destroy(self.h)
            self.h = None

    def load_state(self, sd):
        """sd: the package's state_dict key -> tensor."""
        import torch
        L = load()
        for name, t in sd.items():
            t = t.detach().to('cpu').contiguous().to(torch.float32)
            shape = (ctypes.c_int64 * max(1, t.dim()))(*t.shape)
            check(L.extdm_lpips_load_weight(self.h, name.encode(), ctypes.c_void_p(t.data_ptr()), 0, shape, t.dim()))

    def finalize(self):
        check(load().extdm_lpips_finalize(self.h))

    def distance(self, in0, in1, flags=0, mean=None, map=None):
        """in0, in1 [N, C, H, W]; mean [N] and / or map [N, H, W], contiguous fp32 device tensors."""
        _lpips_images(in0, in1)
        _require_device(mean, map)
        if in0.shape != in1.shape:
            raise ValueError('lpips: the two image sets must have the same shape')
        N, C, H, W = in0.shape
        check(load().extdm_lpips_distance(self.h, N, C, H, W, _ptr(in0), in0.stride(0), in0.stride(1), _ptr(in1),
                                          in1.stride(0), in1.stride(1), flags, _ptr(mean), _ptr(map), _stream()))

    def features(self, x, tap, flags=0):
        """Tap 0 .. 4 = relu1 .. relu5 of x [N, C, H, W] -> a new [N, C', h, w] tensor."""
        import torch
        _lpips_images(x)
        N, C, H, W = x.shape
        out = torch.empty(N, *lpips_feature_shape(H, W, tap), device=x.device, dtype=torch.float32)
        check(load().extdm_lpips_features(self.h, N, C, H, W, _ptr(x), x.stride(0), x.stride(1), flags, tap,
                                          _ptr(out), _stream()))
        return out

    def range_flag(self, reset=True):
        rc = load().extdm_lpips_range_flag(self.h, 1 if reset else 0, _stream())
        if rc < 0:
            check(rc)
        return rc
