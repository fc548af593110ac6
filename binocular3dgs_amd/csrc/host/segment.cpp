// Segmentation from 2D label planes (binocular3dgs_amd/segment.py): launch assembly of b3gs_label_votes_batch and
// b3gs_label_render_batch over the state buffers a FusedRasterizer forward left in its slots.  No autograd: votes and label
// maps are not differentiable.
#include "walk_state.h"

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_S = "the label votes and label renders run on the HIP device only (there is no host statement of the tile walk)";

// views: 1..8 tuples (geometry, binning, image, W, H, labels) -- labels a uint8 [H,W] tensor; votes_q32: int64 [P, nlabels],
// contiguous, accumulated into (its bits are the library's uint64 words).
static void label_votes(const py::list& views, int64_t nlabels, Tensor votes_q32) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("label_votes: 1..8 views");
  if (nlabels < 1 || nlabels > B3GS_MAX_LABELS) throw py::value_error("label_votes: 1..16 labels");
  dev_input(votes_q32, at::kLong, "votes_q32", NO_CPU_S);
  at::Device dev = votes_q32.device();
  if (votes_q32.dim() != 2 || votes_q32.size(1) != nlabels) throw py::value_error("label_votes: votes_q32 is [P, nlabels]");
  if (!votes_q32.is_contiguous()) throw py::value_error("label_votes: votes_q32 is written in place and must be contiguous");
  const int64_t P = votes_q32.size(0);
  if (P > INT32_MAX) throw py::value_error("label_votes: P is the number of Gaussians");
  if (P == 0) return;
  std::vector<Tensor> keep;
  keep.reserve(4 * n);
  B3gsScene sc[8];
  B3gsLabelVoteView lv[8];
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 6) throw py::value_error("label_votes: a view is (geometry, binning, image, W, H, labels)");
    const ViewState s = view_state(t, 3, P, &dev, keep, sc[k], "label_votes", NO_CPU_S);
    Tensor lab = dev_input(t[5].cast<Tensor>(), at::kByte, "labels", NO_CPU_S, &dev);
    if (lab.numel() != s.W * s.H) throw py::value_error("label_votes: a label plane holds H * W bytes");
    lab = lab.contiguous();
    keep.push_back(lab);
    lv[k] = B3gsLabelVoteView{&sc[k], s.geometry, s.binning, s.image, (const uint8_t*)lab.data_ptr()};
  }
  DeviceGuard g(dev);
  check(b3gs_label_votes_batch((int32_t)n, lv, (int32_t)nlabels, (uint64_t*)votes_q32.data_ptr<int64_t>(), cur_stream(dev)),
        "b3gs_label_votes_batch");
}

// views: 1..8 tuples (geometry, binning, image, W, H, label, weight) -- label uint8 [H,W] and weight float32 [H,W], contiguous,
// written; gaussian_label: uint8 [P].
static void label_render(const py::list& views, int64_t nlabels, Tensor gaussian_label) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("label_render: 1..8 views");
  if (nlabels < 1 || nlabels > B3GS_MAX_LABELS) throw py::value_error("label_render: 1..16 labels");
  dev_input(gaussian_label, at::kByte, "gaussian_label", NO_CPU_S);
  at::Device dev = gaussian_label.device();
  if (gaussian_label.dim() != 1) throw py::value_error("label_render: gaussian_label is [P]");
  gaussian_label = gaussian_label.contiguous();
  const int64_t P = gaussian_label.size(0);
  if (P > INT32_MAX) throw py::value_error("label_render: P is the number of Gaussians");
  if (P == 0) return;
  std::vector<Tensor> keep;
  keep.reserve(5 * n);
  B3gsScene sc[8];
  B3gsLabelRenderView rv[8];
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 7) throw py::value_error("label_render: a view is (geometry, binning, image, W, H, label, weight)");
    const ViewState s = view_state(t, 3, P, &dev, keep, sc[k], "label_render", NO_CPU_S);
    Tensor label = dev_input(t[5].cast<Tensor>(), at::kByte, "label", NO_CPU_S, &dev);
    Tensor weight = dev_input(t[6].cast<Tensor>(), at::kFloat, "weight", NO_CPU_S, &dev);
    for (const Tensor* x : {&label, &weight}) {
      if (x->dim() != 2 || x->size(0) != s.H || x->size(1) != s.W) throw py::value_error("label_render: label and weight are [H, W]");
      if (!x->is_contiguous()) throw py::value_error("label_render: the planes are written in place and must be contiguous");
      keep.push_back(*x);
    }
    rv[k] = B3gsLabelRenderView{&sc[k], s.geometry, s.binning, s.image, (uint8_t*)label.data_ptr(), weight.data_ptr<float>()};
  }
  DeviceGuard g(dev);
  check(b3gs_label_render_batch((int32_t)n, rv, (int32_t)nlabels, (const uint8_t*)gaussian_label.data_ptr(), cur_stream(dev)),
        "b3gs_label_render_batch");
}

void bind_segment(py::module_& m) {
  m.def("label_votes", &label_votes, py::arg("views"), py::arg("nlabels"), py::arg("votes_q32"));
  m.def("label_render", &label_render, py::arg("views"), py::arg("nlabels"), py::arg("gaussian_label"));
}

}  // namespace b3
