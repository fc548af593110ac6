// Image metrics of held-out views (binocular3dgs_amd/evaluate.py): launch assembly of b3gs_image_metrics_batch -- the
// per-view sums behind the reference's training_report (train.py:226-261) and metrics.py:37-124, every view of a batch in
// one launch.  No autograd: evaluation runs under no_grad.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU = "the image metrics run on the HIP device only (binocular3dgs_amd.loss holds the PyTorch statement)";

// images / gts: n tensors [C,H,W]; masks: None or n entries (None, [1,H,W] or [C,H,W]); out: float64 [n, 2C + 2] on the
// device, written; prepared_image / prepared_gt: None or float32 [n,C,H,W] (contiguous), written with the composited pair
static Tensor image_metrics(const std::vector<Tensor>& images, const std::vector<Tensor>& gts, const py::object& masks,
                            int64_t mode, Tensor out, const c10::optional<Tensor>& prepared_image,
                            const c10::optional<Tensor>& prepared_gt) {
  const int64_t n = (int64_t)images.size();
  if (n == 0 || (int64_t)gts.size() != n) throw py::value_error("image_metrics: as many gts as images, at least one");
  std::vector<c10::optional<Tensor>> mk(n);
  if (!masks.is_none()) {
    auto seq = masks.cast<py::sequence>();
    if ((int64_t)seq.size() != n) throw py::value_error("image_metrics: one mask (or None) per image");
    for (int64_t i = 0; i < n; i++)
      if (!seq[i].is_none()) mk[i] = seq[i].cast<Tensor>();
  }
  const Tensor& i0 = images[0];
  if (i0.dim() != 3) throw py::value_error("image_metrics expects [C,H,W] images");
  const int64_t C = i0.size(0), H = i0.size(1), W = i0.size(2);
  if (C < 1 || C > 4) throw py::value_error("image_metrics: 1..4 channels");
  const at::Device dev = i0.device();
  if (!out.is_cuda()) raise(std::string("out is on ") + out.device().str() + ": " + NO_CPU);
  if (out.scalar_type() != at::kDouble || !out.is_contiguous() || out.dim() != 2 || out.size(0) != n || out.size(1) != 2 * C + 2)
    throw py::value_error("image_metrics: out must be a contiguous float64 [n, 2C + 2] tensor");
  const bool prep = prepared_image.has_value() && prepared_image->defined();
  if (prep != (prepared_gt.has_value() && prepared_gt->defined()))
    throw py::value_error("image_metrics: prepared_image and prepared_gt go together");
  if (prep) {
    for (const Tensor* p : {&*prepared_image, &*prepared_gt})
      if (!p->is_cuda() || p->scalar_type() != at::kFloat || !p->is_contiguous() || p->sizes() != at::IntArrayRef({n, C, H, W}))
        throw py::value_error("image_metrics: prepared tensors must be contiguous float32 [n,C,H,W] on the device");
  }
  std::vector<Tensor> keep;          // contiguous / fp32 copies live until the launch is enqueued
  keep.reserve(3 * n);
  std::vector<B3gsMetricView> tab(n);
  for (int64_t i = 0; i < n; i++) {
    if (images[i].sizes() != i0.sizes() || gts[i].sizes() != i0.sizes())
      throw py::value_error("image_metrics: every image and gt of one call has the same [C,H,W]");
    keep.push_back(dev_f32(images[i], "image", NO_CPU));
    keep.push_back(dev_f32(gts[i], "gt", NO_CPU));
    B3gsMetricView& v = tab[i];
    v.image = keep[keep.size() - 2].data_ptr<float>();
    v.gt = keep.back().data_ptr<float>();
    v.mask = nullptr;
    v.mask_channels = 1;
    if (mk[i].has_value()) {
      const Tensor& m = *mk[i];
      if (m.dim() != 3 || (m.size(0) != 1 && m.size(0) != C) || m.size(1) != H || m.size(2) != W)
        throw py::value_error("image_metrics: a mask is [1,H,W] or [C,H,W]");
      keep.push_back(dev_f32(m, "mask", NO_CPU));
      v.mask = keep.back().data_ptr<float>();
      v.mask_channels = (int32_t)m.size(0);
    }
    v.prepared_image = prep ? prepared_image->data_ptr<float>() + i * C * H * W : nullptr;
    v.prepared_gt = prep ? prepared_gt->data_ptr<float>() + i * C * H * W : nullptr;
  }
  const size_t ws_bytes = b3gs_image_metrics_workspace_bytes((int32_t)n, (int32_t)C, (int32_t)H, (int32_t)W);
  Tensor ws = at::empty({(int64_t)((ws_bytes + 7) / 8)}, at::TensorOptions().dtype(at::kDouble).device(dev));
  {
    DeviceGuard g(dev);
    check(b3gs_image_metrics_batch((int32_t)n, tab.data(), (int32_t)C, (int32_t)H, (int32_t)W, (int32_t)mode,
                                   out.data_ptr<double>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_image_metrics_batch");
  }
  return out;
}

void bind_metrics(py::module_& m) {
  m.def("image_metrics", &image_metrics, py::arg("images"), py::arg("gts"), py::arg("masks"), py::arg("mode"), py::arg("out"),
        py::arg("prepared_image") = py::none(), py::arg("prepared_gt") = py::none());
  m.attr("METRIC_CLAMP") = B3GS_METRIC_CLAMP;
  m.attr("METRIC_QUANTIZE") = B3GS_METRIC_QUANTIZE;
}

}  // namespace b3
