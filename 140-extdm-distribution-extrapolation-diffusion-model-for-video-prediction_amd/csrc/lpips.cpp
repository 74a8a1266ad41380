// The LPIPS runtime: lpips.LPIPS(net='alex', version='0.1') restated from the published package
// (class LPIPS, ScalingLayer, NetLinLayer, pretrained_networks.alexnet) on a handle of its own --
// weight registry under the package's state_dict keys, the f16x3 layout of pack_conv2d uploaded per
// conv, a workspace planned at max_pairs x max_h x max_w, the forward as a sequence of lpips.hip
// launches -- and the extdm_lpips_* part of the C ABI (include/extdm.h). A call with
// EXTDM_LPIPS_FP32 runs the five convs on the exact-fp32 kernel of lpips_f32.hip instead (fp32
// tiles of pack_conv2d_f32, packed and uploaded on the handle's first such call); everything
// around the convs is shared.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "extdm.h"
#include "host_util.h"
#include "lpips.h"
#include "pack.h"

using namespace extdm;

namespace {

struct HostW {
  std::vector<float> f;
  std::vector<int64_t> shape;
};

// torchvision alexnet().features indices of the five convs, and the package's slices
struct ConvCfg { const char* key; int M, Cin, KS, stride, pad; };
const ConvCfg kConvs[5] = {{"net.slice1.0", 64, 3, 11, 4, 2},
                           {"net.slice2.3", 192, 64, 5, 1, 2},
                           {"net.slice3.6", 384, 192, 3, 1, 1},
                           {"net.slice4.8", 256, 384, 3, 1, 1},
                           {"net.slice5.10", 256, 256, 3, 1, 1}};

// Feature-map extents of the five taps for an H x W input (0 where a stage has no output)
void tap_dims(int H, int W, int h[5], int w[5]) {
  h[0] = conv2d_out(H, 11, 4, 2); w[0] = conv2d_out(W, 11, 4, 2);
  h[1] = pool32_out(h[0]); w[1] = pool32_out(w[0]);
  h[2] = pool32_out(h[1]); w[2] = pool32_out(w[1]);
  for (int k = 3; k < 5; ++k) { h[k] = h[2]; w[k] = w[2]; }
}

// Column means of the 1-D bilinear interpolation matrix (align_corners=False) from `in` to `out`
// samples, in fp64: mean_o up(m)[o] = sum_i w[i] m[i]
void mean_weights(int in, int out, double* w) {
  for (int i = 0; i < in; ++i) w[i] = 0.0;
  const double scale = (double)in / (double)out;
  for (int o = 0; o < out; ++o) {
    double src = scale * ((double)o + 0.5) - 0.5;
    if (src < 0.0) src = 0.0;
    const int i0 = (int)src, i1 = i0 + (i0 < in - 1 ? 1 : 0);
    const double l1 = src - (double)i0;
    w[i0] += (1.0 - l1) / (double)out;
    w[i1] += l1 / (double)out;
  }
}

}  // namespace

struct ExtdmLpipsHandle {
  int max_pairs = 1, max_h = 64, max_w = 64, device = 0;
  std::unordered_map<std::string, HostW> host;
  std::vector<void*> allocations;
  bool finalized = false;
  Conv2dW conv[5];
  // the exact-fp32 route: the conv weights as finalize packed them (the stem's with 1 / scale
  // folded in), kept on the host until the first EXTDM_LPIPS_FP32 call uploads their fp32 tiles
  std::vector<float> w32[5];
  Conv2dW conv32[5];
  bool have32 = false;
  const float* lin[5] = {};
  LpipsFront front;
  int* range = nullptr;
  // workspace at 2 * max_pairs images: the five taps, the two pooled maps, the lin maps and the
  // mean weights
  float* feat[5] = {};
  float* pooled[2] = {};
  float* linmap[5] = {};
  double* wy[5] = {};
  double* wx[5] = {};
  int mh[5] = {}, mw[5] = {};  // tap extents at max_h x max_w
  int wH = 0, wW = 0, wplain = -1;  // the geometry the uploaded mean weights belong to
  hipStream_t s = nullptr;

  void* dmalloc(size_t bytes) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 256)));
    allocations.push_back(p);
    return p;
  }
  template <class T>
  T* upload(const std::vector<T>& v) {
    T* d = reinterpret_cast<T*>(dmalloc(v.size() * sizeof(T)));
    HIPCHK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  const HostW& H(const std::string& n, const std::vector<int64_t>& shape) const {
    auto it = host.find(n);
    if (it == host.end()) throw Error("missing weight: " + n);
    const HostW& t = it->second;
    if (t.shape != shape) {
      std::string got, want;
      for (auto d : t.shape) got += std::to_string(d) + " ";
      for (auto d : shape) want += std::to_string(d) + " ";
      throw Error("weight " + n + ": shape [ " + got + "], expected [ " + want + "]");
    }
    return t;
  }

  // `lins.K.model.1.weight` (the ModuleList registration of the same modules) is an alias of
  // `linK.model.1.weight`: either alone is enough, both must agree
  void reconcile_lin_aliases() {
    for (int k = 0; k < 5; ++k) {
      const std::string a = "lin" + std::to_string(k) + ".model.1.weight", b = "lins." + std::to_string(k) + ".model.1.weight";
      auto ib = host.find(b);
      if (ib == host.end()) continue;
      auto ia = host.find(a);
      if (ia == host.end()) host[a] = ib->second;
      else REQUIRE(ia->second.shape == ib->second.shape && ia->second.f == ib->second.f,
                   "lpips: " + a + " and " + b + " name the same layer but differ");
    }
  }

  void finalize() {
    REQUIRE(!finalized, "already finalized");
    HIPCHK(hipSetDevice(device));
    reconcile_lin_aliases();
    // ScalingLayer.forward: (inp - shift) / scale. The subtraction runs in the stem's gather; the
    // division is folded into the stem's weights here (w / scale[ci] in fp64, rounded once).
    const HostW& sh = H("scaling_layer.shift", {1, 3, 1, 1});
    const HostW& sc = H("scaling_layer.scale", {1, 3, 1, 1});
    for (int c = 0; c < 3; ++c) {
      REQUIRE(sc.f[c] != 0.f && std::isfinite(sc.f[c]), "lpips: scaling_layer.scale must be finite and non-zero");
      front.shift[c] = sh.f[c];
    }
    for (int k = 0; k < 5; ++k) {
      const ConvCfg& c = kConvs[k];
      const std::string key = c.key;
      std::vector<float> wt = H(key + ".weight", {c.M, c.Cin, c.KS, c.KS}).f;
      const HostW& b = H(key + ".bias", {c.M});
      const bool stem = k == 0;
      if (stem)
        for (int m = 0; m < c.M; ++m)
          for (int ci = 0; ci < 3; ++ci)
            for (int t = 0; t < 121; ++t) {
              float& v = wt[((size_t)m * 3 + ci) * 121 + t];
              v = (float)((double)v / (double)sc.f[ci]);
            }
      const int bm = conv2d_bm(c.M), Cpad = (c.Cin + 7) / 8 * 8;
      const Frags p = pack_conv2d(wt, c.M, c.Cin, Cpad, c.KS, bm, stem ? kLpipsStemRow : 0);
      Conv2dW& w = conv[k];
      w.w = upload(p.g);
      w.wscale = upload(p.rs);
      w.bias = upload(b.f);
      w.M = c.M; w.Cin = c.Cin; w.Cpad = Cpad; w.KS = c.KS; w.stride = c.stride; w.pad = c.pad;
      w.bm = bm; w.nkt = p.n; w.stem = stem;
      w32[k] = std::move(wt);
      // NetLinLayer: Conv2d(C_k, 1, 1, bias=False) behind an inference-time identity dropout
      lin[k] = upload(H("lin" + std::to_string(k) + ".model.1.weight", {1, c.M, 1, 1}).f);
    }
    range = reinterpret_cast<int*>(dmalloc(sizeof(int)));
    HIPCHK(hipMemset(range, 0, sizeof(int)));
    tap_dims(max_h, max_w, mh, mw);
    const size_t NI = (size_t)2 * max_pairs;
    const int ph[2] = {mh[1], mh[2]}, pw[2] = {mw[1], mw[2]};
    for (int k = 0; k < 5; ++k) {
      // tap 1 / 2 are computed at the pooled extents of the map before them
      feat[k] = reinterpret_cast<float*>(dmalloc(NI * kConvs[k].M * mh[k] * mw[k] * sizeof(float)));
      linmap[k] = reinterpret_cast<float*>(dmalloc((size_t)max_pairs * mh[k] * mw[k] * sizeof(float)));
      wy[k] = reinterpret_cast<double*>(dmalloc((size_t)mh[k] * sizeof(double)));
      wx[k] = reinterpret_cast<double*>(dmalloc((size_t)mw[k] * sizeof(double)));
    }
    for (int k = 0; k < 2; ++k)
      pooled[k] = reinterpret_cast<float*>(dmalloc(NI * kConvs[k].M * ph[k] * pw[k] * sizeof(float)));
    host.clear();
    finalized = true;
  }

  void upload_f32() {
    if (have32) return;
    for (int k = 0; k < 5; ++k) {
      const Conv2dW& c = conv[k];
      const TilesF32 t = c.stem ? pack_conv2d_f32_stem(w32[k], c.M, c.Cin, c.KS, kLpipsF32Bm, kLpipsStemRow)
                                : pack_conv2d_f32(w32[k], c.M, c.Cin, c.Cpad, c.KS, kLpipsF32Bm);
      Conv2dW& w = conv32[k];
      w = c;
      w.bm = kLpipsF32Bm;
      w.w = upload(t.a);
      w.wscale = nullptr;
      w.nkt = t.nkt;
      std::vector<float>().swap(w32[k]);
    }
    have32 = true;
  }

  void check_geometry(int N, int C, int Hh, int W) const {
    REQUIRE(N >= 1 && (C == 1 || C == 3), "lpips: [N][C][H][W] with C = 1 or 3 expected");
    // below 31 the second MaxPool2d(3, 2) has no output
    REQUIRE(Hh >= 31 && W >= 31, "lpips: H and W must be at least 31, got " + std::to_string(Hh) + " x " + std::to_string(W));
    REQUIRE(Hh <= max_h && W <= max_w, "lpips: image larger than the planned max_h x max_w");
  }

  // relu1 .. relu(last + 1) of NI = N (in1 null) or 2 N images: set 0 in slots [0, N), set 1 in
  // [N, 2 N). The stem runs once per set (a set is one buffer); the other convs once over all.
  void run(int N, int C, int Hh, int W, const float* in0, long sn0, long sc0, const float* in1, long sn1, long sc1,
           int pre, int last, bool fp32, int h[5], int w[5]) {
    tap_dims(Hh, W, h, w);
    const int NI = in1 ? 2 * N : N;
    LpipsFront f = front;
    f.pre = pre;
    if (fp32) upload_f32();
    auto conv_ = [&](int k, const float* in, long ib, long ic, int B, int hi, int wi, float* out) {
      const LpipsFront* fr = k == 0 ? &f : nullptr;
      REQUIRE(fp32 ? conv2d_f32_forward(s, in, ib, ic, B, hi, wi, conv32[k], fr, out)
                   : conv2d_x3_forward(s, in, ib, ic, B, hi, wi, conv[k], fr, out, range),
              std::string("lpips: convolution ") + kConvs[k].key + " not covered (input larger than 4 GiB?)");
    };
    conv_(0, in0, sn0, C == 1 ? 0 : sc0, N, Hh, W, feat[0]);
    if (in1) conv_(0, in1, sn1, C == 1 ? 0 : sc1, N, Hh, W, feat[0] + (size_t)N * 64 * h[0] * w[0]);
    if (last < 1) return;
    maxpool2d_32(s, feat[0], pooled[0], (long)NI * 64, h[0], w[0]);
    conv_(1, pooled[0], (long)64 * h[1] * w[1], (long)h[1] * w[1], NI, h[1], w[1], feat[1]);
    if (last < 2) return;
    maxpool2d_32(s, feat[1], pooled[1], (long)NI * 192, h[1], w[1]);
    const long hw = (long)h[2] * w[2];
    conv_(2, pooled[1], 192 * hw, hw, NI, h[2], w[2], feat[2]);
    if (last < 3) return;
    conv_(3, feat[2], 384 * hw, hw, NI, h[2], w[2], feat[3]);
    if (last < 4) return;
    conv_(4, feat[3], 256 * hw, hw, NI, h[2], w[2], feat[4]);
  }

  // the separable mean weights of the current geometry: bilinear column means (spatial map), or
  // the plain 1 / h, 1 / w of spatial_average. Uploaded when the geometry changes; every entry
  // point ends with a stream synchronisation, so no launch is reading the old ones.
  void set_weights(int Hh, int W, const int h[5], const int w[5], bool plain) {
    if (wH == Hh && wW == W && wplain == (int)plain) return;
    std::vector<double> v;
    for (int k = 0; k < 5; ++k) {
      v.assign((size_t)h[k], 1.0 / (double)h[k]);
      if (!plain) mean_weights(h[k], Hh, v.data());
      HIPCHK(hipMemcpy(wy[k], v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
      v.assign((size_t)w[k], 1.0 / (double)w[k]);
      if (!plain) mean_weights(w[k], W, v.data());
      HIPCHK(hipMemcpy(wx[k], v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    wH = Hh; wW = W; wplain = (int)plain;
  }

  // every entry point ends here: the stream is synchronised; on the f16x3 route the range flag is
  // read and raised, on the fp32 route (no fp16 anywhere) it is neither written nor consulted
  void finish(bool fp32) {
    if (fp32) {
      HIPCHK(hipStreamSynchronize(s));
      return;
    }
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, range, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    REQUIRE(flag == 0, "lpips: activation out of fp16 range (|v| >= 65504) in an f16x3 convolution");
  }
};

extern "C" {

int extdm_lpips_create(int max_pairs, int max_h, int max_w, int device, ExtdmLpipsHandle** out) {
  return guarded([&] {
    REQUIRE(out, "null argument");
    REQUIRE(max_pairs >= 1, "lpips: bad configuration");
    REQUIRE(max_h >= 31 && max_w >= 31, "lpips: H and W must be at least 31");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    REQUIRE(ndev > 0, "no HIP device visible");
    REQUIRE(device >= 0 && device < ndev, "lpips: no such device");
    auto h = std::make_unique<ExtdmLpipsHandle>();
    h->max_pairs = max_pairs; h->max_h = max_h; h->max_w = max_w; h->device = device;
    *out = h.release();
  });
}

void extdm_lpips_destroy(ExtdmLpipsHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  for (void* p : h->allocations) (void)hipFree(p);
  delete h;
}

int extdm_lpips_load_weight(ExtdmLpipsHandle* h, const char* name, const void* ptr, int dtype, const int64_t* shape,
                            int ndim) {
  return guarded([&] {
    REQUIRE(h && name && ptr, "null argument");
    REQUIRE(!h->finalized, "weights are frozen after extdm_lpips_finalize");
    REQUIRE(dtype == 0, "lpips: float32 weights expected: " + std::string(name));
    HostW t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.f.assign(reinterpret_cast<const float*>(ptr), reinterpret_cast<const float*>(ptr) + n);
    h->host[name] = std::move(t);  // the linK / lins.K aliases are reconciled at finalize
  });
}

int extdm_lpips_finalize(ExtdmLpipsHandle* h) {
  return guarded([&] {
    REQUIRE(h, "null handle");
    h->finalize();
  });
}

int extdm_lpips_distance(ExtdmLpipsHandle* h, int N, int C, int H, int W, const float* in0, long sn0, long sc0,
                         const float* in1, long sn1, long sc1, int flags, float* mean_out, float* map_out,
                         void* stream) {
  return guarded([&] {
    REQUIRE(h && h->finalized, "lpips: handle not finalized");
    REQUIRE(in0 && in1 && (mean_out || map_out), "null argument");
    h->check_geometry(N, C, H, W);
    REQUIRE(N <= h->max_pairs, "lpips: " + std::to_string(N) + " pairs exceed max_pairs " + std::to_string(h->max_pairs));
    HIPCHK(hipSetDevice(h->device));
    h->s = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(h->range, 0, sizeof(int), h->s));
    int th[5], tw[5];
    tap_dims(H, W, th, tw);
    h->set_weights(H, W, th, tw, (flags & EXTDM_LPIPS_PLAIN_MEAN) != 0);
    const int pre = ((flags & EXTDM_LPIPS_NORMALIZE) ? 1 : 0) + ((flags & EXTDM_LPIPS_TRANS) ? 1 : 0);
    const bool fp32 = (flags & EXTDM_LPIPS_FP32) != 0;
    h->run(N, C, H, W, in0, sn0, sc0, in1, sn1, sc1, pre, 4, fp32, th, tw);
    LpipsTaps t{};
    for (int k = 0; k < 5; ++k) {
      const int hw = th[k] * tw[k];
      lpips_head(h->s, h->feat[k], (long)N * kConvs[k].M * hw, h->lin[k], h->linmap[k], N, kConvs[k].M, hw);
      t.lin[k] = h->linmap[k]; t.h[k] = th[k]; t.w[k] = tw[k]; t.wy[k] = h->wy[k]; t.wx[k] = h->wx[k];
    }
    if (mean_out) lpips_mean(h->s, t, mean_out, N);
    if (map_out) lpips_map(h->s, t, map_out, N, H, W);
    HIPCHK(hipGetLastError());
    h->finish(fp32);
  });
}

int extdm_lpips_feature_shape(int H, int W, int tap, int* dims) {
  return guarded([&] {
    REQUIRE(dims, "null argument");
    REQUIRE(tap >= 0 && tap < 5, "lpips: taps are 0 (relu1) .. 4 (relu5)");
    REQUIRE(H >= 1 && W >= 1, "lpips: bad geometry");
    int th[5], tw[5];
    tap_dims(H, W, th, tw);
    dims[0] = kConvs[tap].M; dims[1] = std::max(th[tap], 0); dims[2] = std::max(tw[tap], 0);
  });
}

int extdm_lpips_features(ExtdmLpipsHandle* h, int N, int C, int H, int W, const float* x, long sn, long sc, int flags,
                         int tap, float* out, void* stream) {
  return guarded([&] {
    REQUIRE(h && h->finalized, "lpips: handle not finalized");
    REQUIRE(x && out, "null argument");
    REQUIRE(tap >= 0 && tap < 5, "lpips: taps are 0 (relu1) .. 4 (relu5)");
    h->check_geometry(N, C, H, W);
    REQUIRE(N <= 2 * h->max_pairs, "lpips: " + std::to_string(N) + " images exceed 2 x max_pairs");
    HIPCHK(hipSetDevice(h->device));
    h->s = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemsetAsync(h->range, 0, sizeof(int), h->s));
    const int pre = ((flags & EXTDM_LPIPS_NORMALIZE) ? 1 : 0) + ((flags & EXTDM_LPIPS_TRANS) ? 1 : 0);
    int th[5], tw[5];
    const bool fp32 = (flags & EXTDM_LPIPS_FP32) != 0;
    h->run(N, C, H, W, x, sn, sc, nullptr, 0, 0, pre, tap, fp32, th, tw);
    HIPCHK(hipMemcpyAsync(out, h->feat[tap], (size_t)N * kConvs[tap].M * th[tap] * tw[tap] * sizeof(float),
                          hipMemcpyDeviceToDevice, h->s));
    HIPCHK(hipGetLastError());
    h->finish(fp32);
  });
}

int extdm_lpips_maxpool(const float* x, int B, int C, int H, int W, float* out, void* stream) {
  return guarded([&] {
    REQUIRE(x && out, "lpips_maxpool: null pointer");
    REQUIRE(B > 0 && C > 0 && H >= 3 && W >= 3, "lpips_maxpool: bad geometry (H, W at least 3)");
    maxpool2d_32(reinterpret_cast<hipStream_t>(stream), x, out, (long)B * C, H, W);
    HIPCHK(hipGetLastError());
  });
}

int extdm_lpips_mean_weights(int in, int out, double* w) {
  if (in < 1 || out < 1 || !w) return -1;
  mean_weights(in, out, w);
  return 0;
}

int extdm_lpips_range_flag(ExtdmLpipsHandle* h, int reset, void* stream) {
  int flag = 0;
  const int rc = guarded([&] {
    REQUIRE(h && h->finalized, "lpips: handle not finalized");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipMemcpyAsync(&flag, h->range, sizeof(int), hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(h->range, 0, sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));
  });
  return rc != 0 ? rc : flag;
}

}  // extern "C"
