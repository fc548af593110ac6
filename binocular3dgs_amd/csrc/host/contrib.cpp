// Per-Gaussian render contribution (binocular3dgs_amd/importance.py): launch assembly of b3gs_blend_contribution_batch over
// the state buffers a FusedRasterizer forward left in its slots.  No autograd: the statistics are not differentiable.
#include "walk_state.h"

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_C = "the render contribution runs on the HIP device only (there is no host statement of the tile walk)";

// views: 1..8 tuples (geometry, binning, image, W, H, mask | None) -- the three uint8 state buffers of one view's forward,
// its size, and an optional uint8 / bool [H,W] mask (nonzero = count the pixel); weight_q32 int64 [P], hits / wmax_bits /
// dominant int32 [P]: accumulated into (their bits are the library's uint64 / uint32 words).
static void blend_contribution(const py::list& views, Tensor weight_q32, Tensor hits, Tensor wmax_bits, Tensor dominant) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("blend_contribution: 1..8 views");
  dev_input(weight_q32, at::kLong, "weight_q32", NO_CPU_C);
  const at::Device dev = weight_q32.device();
  const int64_t P = weight_q32.numel();
  for (const auto& t : {std::make_pair(&hits, "hits"), std::make_pair(&wmax_bits, "wmax_bits"), std::make_pair(&dominant, "dominant")}) {
    dev_input(*t.first, at::kInt, t.second, NO_CPU_C, &dev);
    if (t.first->numel() != P) throw py::value_error("blend_contribution: the four outputs hold one element per Gaussian");
  }
  for (const Tensor* t : {&weight_q32, &hits, &wmax_bits, &dominant})
    if (!t->is_contiguous()) throw py::value_error("blend_contribution: the outputs are written in place and must be contiguous");
  if (P == 0) return;
  std::vector<Tensor> keep;
  keep.reserve(4 * n);
  B3gsScene sc[8];
  B3gsContribView cv[8];
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 6) throw py::value_error("blend_contribution: a view is (geometry, binning, image, W, H, mask | None)");
    const ViewState s = view_state(t, 3, P, &dev, keep, sc[k], "blend_contribution", NO_CPU_C);
    cv[k] = B3gsContribView{&sc[k], s.geometry, s.binning, s.image, nullptr};
    if (!t[5].is_none()) {
      Tensor m = t[5].cast<Tensor>();
      if (!m.defined() || !m.is_cuda()) raise(std::string("mask is on ") + (m.defined() ? m.device().str() : "no device") + ": " + NO_CPU_C);
      if (m.scalar_type() != at::kByte && m.scalar_type() != at::kBool) throw py::value_error("blend_contribution: a mask is uint8 or bool");
      if (m.numel() != s.W * s.H) throw py::value_error("blend_contribution: a mask holds H * W elements");
      m = m.contiguous();
      keep.push_back(m);
      cv[k].pixel_mask = (const uint8_t*)m.data_ptr();
    }
  }
  B3gsContribOut out;
  out.weight_q32 = (uint64_t*)weight_q32.data_ptr<int64_t>();
  out.hits = (uint32_t*)hits.data_ptr<int32_t>();
  out.wmax_bits = (uint32_t*)wmax_bits.data_ptr<int32_t>();
  out.dominant = (uint32_t*)dominant.data_ptr<int32_t>();
  DeviceGuard g(dev);
  check(b3gs_blend_contribution_batch((int32_t)n, cv, &out, cur_stream(dev)), "b3gs_blend_contribution_batch");
}

void bind_contrib(py::module_& m) {
  m.def("blend_contribution", &blend_contribution, py::arg("views"), py::arg("weight_q32"), py::arg("hits"), py::arg("wmax_bits"),
        py::arg("dominant"));
}

}  // namespace b3
