// Feature fields (binocular3dgs_amd/features.py): launch assembly of b3gs_feature_render_batch and b3gs_feature_lift_batch over
// the state buffers a FusedRasterizer forward left in its slots.  No autograd node here: features.FeatureRender pairs the two
// calls in python (the lift of the incoming gradient is the backward of the render).
#include "walk_state.h"

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_F = "the feature render and lift run on the HIP device only (there is no host statement of the tile walk)";

static int64_t check_c(int64_t C, const char* fn) {
  if (C < 1 || C > B3GS_MAX_FEATURE_CHANNELS) throw py::value_error(std::string(fn) + ": 1..256 channels");
  return C;
}

// views: 1..8 tuples (geometry, binning, image, W, H, out) -- out a float32 [C,H,W] tensor, contiguous, written;
// gaussian_features: float32 [P, C].
static void feature_render(const py::list& views, Tensor gaussian_features) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("feature_render: 1..8 views");
  dev_input(gaussian_features, at::kFloat, "gaussian_features", NO_CPU_F);
  at::Device dev = gaussian_features.device();
  if (gaussian_features.dim() != 2) throw py::value_error("feature_render: gaussian_features is [P, C]");
  const int64_t P = gaussian_features.size(0);
  if (P > INT32_MAX) throw py::value_error("feature_render: P is the number of Gaussians");
  if (P == 0) return;
  const int64_t C = check_c(gaussian_features.size(1), "feature_render");
  gaussian_features = gaussian_features.contiguous();
  std::vector<Tensor> keep;
  keep.reserve(4 * n);
  B3gsScene sc[8];
  B3gsFeatureRenderView rv[8];
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 6) throw py::value_error("feature_render: a view is (geometry, binning, image, W, H, out)");
    const ViewState s = view_state(t, 3, P, &dev, keep, sc[k], "feature_render", NO_CPU_F);
    Tensor out = dev_input(t[5].cast<Tensor>(), at::kFloat, "out", NO_CPU_F, &dev);
    if (out.dim() != 3 || out.size(0) != C || out.size(1) != s.H || out.size(2) != s.W) throw py::value_error("feature_render: out is [C, H, W]");
    if (!out.is_contiguous()) throw py::value_error("feature_render: the planes are written in place and must be contiguous");
    keep.push_back(out);
    rv[k] = B3gsFeatureRenderView{&sc[k], s.geometry, s.binning, s.image, out.data_ptr<float>()};
  }
  DeviceGuard g(dev);
  check(b3gs_feature_render_batch((int32_t)n, rv, (int32_t)C, gaussian_features.data_ptr<float>(), cur_stream(dev)),
        "b3gs_feature_render_batch");
}

// views: 1..8 tuples (geometry, binning, image, W, H, maps, mask | None) -- maps float32 [C,H,W], mask uint8 / bool [H,W]
// (nonzero = count the pixel); scale: float32 [C], any device (the library takes it from host memory), every entry > 0;
// sums_q32: int64 [P, C], weight_q32: int64 [P] or None -- contiguous, accumulated into (weight's bits are uint64 words).
static void feature_lift(const py::list& views, Tensor scale, Tensor sums_q32, const c10::optional<Tensor>& weight_q32) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("feature_lift: 1..8 views");
  dev_input(sums_q32, at::kLong, "sums_q32", NO_CPU_F);
  at::Device dev = sums_q32.device();
  if (sums_q32.dim() != 2) throw py::value_error("feature_lift: sums_q32 is [P, C]");
  if (!sums_q32.is_contiguous()) throw py::value_error("feature_lift: sums_q32 is written in place and must be contiguous");
  const int64_t P = sums_q32.size(0);
  if (P > INT32_MAX) throw py::value_error("feature_lift: P is the number of Gaussians");
  if (P == 0) return;
  const int64_t C = check_c(sums_q32.size(1), "feature_lift");
  uint64_t* wq = nullptr;
  if (weight_q32.has_value() && weight_q32->defined()) {
    dev_input(*weight_q32, at::kLong, "weight_q32", NO_CPU_F, &dev);
    if (weight_q32->numel() != P) throw py::value_error("feature_lift: weight_q32 holds one element per Gaussian");
    if (!weight_q32->is_contiguous()) throw py::value_error("feature_lift: weight_q32 is written in place and must be contiguous");
    wq = (uint64_t*)weight_q32->data_ptr<int64_t>();
  }
  if (!scale.defined() || scale.scalar_type() != at::kFloat || scale.numel() != C) throw py::value_error("feature_lift: scale is float32 [C]");
  const Tensor host_scale = scale.reshape({C}).cpu().contiguous();
  std::vector<Tensor> keep;
  keep.reserve(5 * n);
  B3gsScene sc[8];
  B3gsFeatureLiftView lv[8];
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 7) throw py::value_error("feature_lift: a view is (geometry, binning, image, W, H, maps, mask | None)");
    const ViewState s = view_state(t, 3, P, &dev, keep, sc[k], "feature_lift", NO_CPU_F);
    Tensor maps = dev_input(t[5].cast<Tensor>(), at::kFloat, "maps", NO_CPU_F, &dev);
    if (maps.dim() != 3 || maps.size(0) != C || maps.size(1) != s.H || maps.size(2) != s.W) throw py::value_error("feature_lift: maps is [C, H, W]");
    maps = maps.contiguous();
    keep.push_back(maps);
    lv[k] = B3gsFeatureLiftView{&sc[k], s.geometry, s.binning, s.image, maps.data_ptr<float>(), nullptr};
    if (!t[6].is_none()) {
      Tensor m = t[6].cast<Tensor>();
      if (!m.defined() || !m.is_cuda()) raise(std::string("mask is on ") + (m.defined() ? m.device().str() : "no device") + ": " + NO_CPU_F);
      if (m.scalar_type() != at::kByte && m.scalar_type() != at::kBool) throw py::value_error("feature_lift: a mask is uint8 or bool");
      if (m.numel() != s.W * s.H) throw py::value_error("feature_lift: a mask holds H * W elements");
      m = m.contiguous();
      keep.push_back(m);
      lv[k].pixel_mask = (const uint8_t*)m.data_ptr();
    }
  }
  DeviceGuard g(dev);
  check(b3gs_feature_lift_batch((int32_t)n, lv, (int32_t)C, host_scale.data_ptr<float>(), sums_q32.data_ptr<int64_t>(), wq, cur_stream(dev)),
        "b3gs_feature_lift_batch");
}

void bind_features(py::module_& m) {
  m.def("feature_render", &feature_render, py::arg("views"), py::arg("gaussian_features"));
  m.def("feature_lift", &feature_lift, py::arg("views"), py::arg("scale"), py::arg("sums_q32"), py::arg("weight_q32") = py::none());
}

}  // namespace b3
