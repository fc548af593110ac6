// LPIPS of held-out views (binocular3dgs_amd/lpips.py): launch assembly of b3gs_lpips_batch / b3gs_lpips_features -- the VGG16
// taps of lpipsPyTorch (networks.py:88-96, lpips.py:30-36) from packed weights the caller brings.  No autograd: evaluation runs
// under no_grad.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU = "LPIPS runs on the HIP device only (tests/lpips_ref.py holds the PyTorch statement)";

static const int64_t CIN[B3GS_LPIPS_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int64_t COUT[B3GS_LPIPS_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int64_t TAP_C[B3GS_LPIPS_TAPS] = {64, 128, 256, 512, 512};

// the [n,3,H,W] images of one side: float32, contiguous, on the device
static Tensor images(const Tensor& t, const char* name) {
  if (!t.defined() || !t.is_cuda()) raise(std::string(name) + " is on " + (t.defined() ? t.device().str() : "no device") + ": " + NO_CPU);
  if (t.dim() != 4 || t.size(1) != 3) throw py::value_error(std::string("lpips: ") + name + " must be [n,3,H,W]");
  return dev_f32(t, name, NO_CPU);
}

// packed weights (lpips.LpipsWeights.to): conv_w 13 x [K', Cout], conv_b 13 x [Cout], lin 5 x [C_l] (may be empty for features)
static B3gsLpipsWeights weight_table(const std::vector<Tensor>& conv_w, const std::vector<Tensor>& conv_b, const std::vector<Tensor>& lin,
                                     const std::vector<double>& shift, const std::vector<double>& scale, const at::Device& dev,
                                     bool want_lin) {
  if (conv_w.size() != B3GS_LPIPS_CONVS || conv_b.size() != B3GS_LPIPS_CONVS || shift.size() != 3 || scale.size() != 3 ||
      (want_lin && lin.size() != B3GS_LPIPS_TAPS))
    throw py::value_error("lpips: 13 packed weights, 13 biases, 5 lin vectors, 3 shifts and 3 scales");
  B3gsLpipsWeights w = {};
  auto ok = [&](const Tensor& t, std::initializer_list<int64_t> shape, const char* name) {
    dev_input(t, at::kFloat, name, NO_CPU, &dev);
    if (!t.is_contiguous() || t.sizes() != at::IntArrayRef(shape)) throw py::value_error(std::string("lpips: ") + name + " has the wrong shape");
    return t.data_ptr<float>();
  };
  for (int i = 0; i < B3GS_LPIPS_CONVS; i++) {
    const int64_t k = i == 0 ? 28 : 9 * CIN[i];
    w.conv_w[i] = ok(conv_w[i], {k, COUT[i]}, "a packed convolution weight");
    w.conv_b[i] = ok(conv_b[i], {COUT[i]}, "a convolution bias");
  }
  if (want_lin)
    for (int l = 0; l < B3GS_LPIPS_TAPS; l++) w.lin[l] = ok(lin[l], {TAP_C[l]}, "a lin vector");
  for (int c = 0; c < 3; c++) {
    w.shift[c] = (float)shift[c];
    w.scale[c] = (float)scale[c];
  }
  return w;
}

static int64_t lpips_workspace_bytes(int64_t npairs, int64_t H, int64_t W) {
  return (int64_t)b3gs_lpips_workspace_bytes((int32_t)npairs, (int32_t)H, (int32_t)W);
}

static void check_shape(int64_t n, int64_t H, int64_t W) {
  if (n < 1 || n > B3GS_LPIPS_MAX_PAIRS) throw py::value_error("lpips: 1..8 pairs (or images) per call");
  if (H < B3GS_LPIPS_MIN_SIDE || W < B3GS_LPIPS_MIN_SIDE || H * W > ((int64_t)1 << 24))
    throw py::value_error("lpips: H and W must be at least 16 (the fifth layer would be empty), H W at most 2^24");
}

// x, y: [n,3,H,W], n <= 8 -> float64 [n,5] on the device: the per-layer means
static Tensor lpips_layers(const Tensor& x, const Tensor& y, const std::vector<Tensor>& conv_w, const std::vector<Tensor>& conv_b,
                           const std::vector<Tensor>& lin, const std::vector<double>& shift, const std::vector<double>& scale,
                           bool normalize) {
  Tensor xs = images(x, "x"), ys = images(y, "y");
  if (xs.sizes() != ys.sizes() || xs.device() != ys.device()) throw py::value_error("lpips: x and y have one shape and one device");
  const int64_t n = xs.size(0), H = xs.size(2), W = xs.size(3);
  check_shape(n, H, W);
  const at::Device dev = xs.device();
  const B3gsLpipsWeights w = weight_table(conv_w, conv_b, lin, shift, scale, dev, true);
  Tensor out = at::empty({n, B3GS_LPIPS_TAPS}, at::TensorOptions().dtype(at::kDouble).device(dev));
  Tensor ws = byte_workspace(b3gs_lpips_workspace_bytes((int32_t)n, (int32_t)H, (int32_t)W), dev);
  {
    DeviceGuard g(dev);
    check(b3gs_lpips_batch((int32_t)n, xs.data_ptr<float>(), ys.data_ptr<float>(), (int32_t)H, (int32_t)W, &w, normalize ? 1 : 0,
                           out.data_ptr<double>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_lpips_batch");
  }
  return out;
}

// x: [n,3,H,W], n <= 8 -> the five tap feature maps [n,C_l,H_l,W_l] before normalisation
static std::vector<Tensor> lpips_features(const Tensor& x, const std::vector<Tensor>& conv_w, const std::vector<Tensor>& conv_b,
                                          const std::vector<double>& shift, const std::vector<double>& scale, bool normalize) {
  Tensor xs = images(x, "x");
  const int64_t n = xs.size(0), H = xs.size(2), W = xs.size(3);
  check_shape(n, H, W);
  const at::Device dev = xs.device();
  const B3gsLpipsWeights w = weight_table(conv_w, conv_b, {}, shift, scale, dev, false);
  std::vector<Tensor> feats;
  float* ptrs[B3GS_LPIPS_TAPS];
  for (int l = 0; l < B3GS_LPIPS_TAPS; l++) {
    feats.push_back(at::empty({n, TAP_C[l], H >> l, W >> l}, at::TensorOptions().dtype(at::kFloat).device(dev)));
    ptrs[l] = feats.back().data_ptr<float>();
  }
  Tensor ws = byte_workspace(b3gs_lpips_workspace_bytes((int32_t)n, (int32_t)H, (int32_t)W), dev);
  {
    DeviceGuard g(dev);
    check(b3gs_lpips_features((int32_t)n, xs.data_ptr<float>(), (int32_t)H, (int32_t)W, &w, normalize ? 1 : 0, ptrs, ws.data_ptr(),
                              cur_stream(dev)),
          "b3gs_lpips_features");
  }
  return feats;
}

void bind_lpips(py::module_& m) {
  m.def("lpips_workspace_bytes", &lpips_workspace_bytes, py::arg("npairs"), py::arg("H"), py::arg("W"));
  m.def("lpips_layers", &lpips_layers, py::arg("x"), py::arg("y"), py::arg("conv_w"), py::arg("conv_b"), py::arg("lin"),
        py::arg("shift"), py::arg("scale"), py::arg("normalize") = false);
  m.def("lpips_features", &lpips_features, py::arg("x"), py::arg("conv_w"), py::arg("conv_b"), py::arg("shift"), py::arg("scale"),
        py::arg("normalize") = false);
  m.attr("LPIPS_MAX_PAIRS") = B3GS_LPIPS_MAX_PAIRS;
}

}  // namespace b3
