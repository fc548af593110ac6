// Frames of a rendered path (binocular3dgs_amd/frames.py): launch assembly of b3gs_encode_frames_batch -- the rgb, gray depth
// and colour-mapped depth images of spiral.py:101-131 for up to 8 views of one W x H per call.  No autograd, no host read.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU = "frames are encoded on the HIP device only";

static void check_out(const c10::optional<Tensor>& t, int64_t n, int64_t H, int64_t W, const char* name) {
  if (!t.has_value() || !t->defined()) return;
  if (!t->is_cuda() || t->scalar_type() != at::kByte || !t->is_contiguous() || t->sizes() != at::IntArrayRef({n, H, W, 3}))
    throw py::value_error(std::string("encode_frames: ") + name + " must be a contiguous uint8 [n,H,W,3] tensor on the device");
}

static uint8_t* out_ptr(const c10::optional<Tensor>& t, int64_t i, int64_t H, int64_t W) {
  return (t.has_value() && t->defined()) ? t->data_ptr<uint8_t>() + i * H * W * 3 : nullptr;
}

// renders: n tensors [3,H,W]; depths / alphas: None (rgb only) or n tensors [1,H,W] (or [H,W]); rgb_out / gray_out / cmap_out: None or uint8
// [n,H,W,3], written; lut: uint8 [256,3] on the device; bounds: None or float64 [n,2] on the device, written
static void encode_frames(const std::vector<Tensor>& renders, const py::object& depths_obj, const py::object& alphas_obj,
                          const c10::optional<Tensor>& rgb_out, const c10::optional<Tensor>& gray_out,
                          const c10::optional<Tensor>& cmap_out, double percentile, const Tensor& lut,
                          const c10::optional<Tensor>& bounds) {
  const int64_t n = (int64_t)renders.size();
  if (n < 1 || n > B3GS_MAX_FRAME_VIEWS) throw py::value_error("encode_frames: 1..8 views per call");
  const bool have_depth = !depths_obj.is_none();
  if (have_depth == alphas_obj.is_none()) throw py::value_error("encode_frames: depths and alphas go together");
  std::vector<Tensor> depths, alphas;
  if (have_depth) {
    depths = depths_obj.cast<std::vector<Tensor>>();
    alphas = alphas_obj.cast<std::vector<Tensor>>();
    if ((int64_t)depths.size() != n || (int64_t)alphas.size() != n)
      throw py::value_error("encode_frames: one depth and one alpha per render");
  }
  const Tensor& r0 = renders[0];
  if (r0.dim() != 3 || r0.size(0) != 3) throw py::value_error("encode_frames expects [3,H,W] renders");
  const int64_t H = r0.size(1), W = r0.size(2);
  const at::Device dev = r0.device();
  check_out(rgb_out, n, H, W, "rgb_out");
  check_out(gray_out, n, H, W, "gray_out");
  check_out(cmap_out, n, H, W, "cmap_out");
  if (!lut.is_cuda() || lut.scalar_type() != at::kByte || !lut.is_contiguous() || lut.numel() != 256 * 3)
    throw py::value_error("encode_frames: lut must be a contiguous uint8 [256,3] tensor on the device");
  const bool want_bounds = bounds.has_value() && bounds->defined();
  if (!have_depth && (want_bounds || (gray_out.has_value() && gray_out->defined()) || (cmap_out.has_value() && cmap_out->defined())))
    throw py::value_error("encode_frames: gray, colour map and bounds need depths and alphas");
  if (want_bounds && (!bounds->is_cuda() || bounds->scalar_type() != at::kDouble || !bounds->is_contiguous() ||
                      bounds->numel() != 2 * n))
    throw py::value_error("encode_frames: bounds must be a contiguous float64 [n,2] tensor on the device");
  std::vector<Tensor> keep;          // contiguous / fp32 copies live until the launch is enqueued
  keep.reserve(3 * n);
  std::vector<B3gsFrameView> tab(n);
  for (int64_t i = 0; i < n; i++) {
    if (renders[i].sizes() != r0.sizes()) throw py::value_error("encode_frames: every render of one call has the same [3,H,W]");
    B3gsFrameView& v = tab[i];
    keep.push_back(dev_f32(renders[i], "render", NO_CPU));
    v.rgb = keep.back().data_ptr<float>();
    v.depth = v.alpha = nullptr;
    if (have_depth) {
      if (depths[i].numel() != H * W || alphas[i].numel() != H * W)
        throw py::value_error("encode_frames: depth and alpha hold H*W values per view");
      keep.push_back(dev_f32(depths[i], "depth", NO_CPU));
      v.depth = keep.back().data_ptr<float>();
      keep.push_back(dev_f32(alphas[i], "alpha", NO_CPU));
      v.alpha = keep.back().data_ptr<float>();
    }
    v.rgb_out = out_ptr(rgb_out, i, H, W);
    v.gray_out = out_ptr(gray_out, i, H, W);
    v.cmap_out = out_ptr(cmap_out, i, H, W);
  }
  const size_t ws_bytes = b3gs_frames_workspace_bytes((int32_t)n, (int32_t)H, (int32_t)W);
  Tensor ws = byte_workspace(ws_bytes, dev);
  {
    DeviceGuard g(dev);
    check(b3gs_encode_frames_batch((int32_t)n, tab.data(), (int32_t)H, (int32_t)W, percentile, lut.data_ptr<uint8_t>(),
                                   ws.data_ptr(), want_bounds ? bounds->data_ptr<double>() : nullptr, cur_stream(dev)),
          "b3gs_encode_frames_batch");
  }
}

void bind_frames(py::module_& m) {
  m.def("encode_frames", &encode_frames, py::arg("renders"), py::arg("depths"), py::arg("alphas"), py::arg("rgb_out"),
        py::arg("gray_out"), py::arg("cmap_out"), py::arg("percentile"), py::arg("lut"), py::arg("bounds") = py::none());
  m.attr("MAX_FRAME_VIEWS") = B3GS_MAX_FRAME_VIEWS;
}

}  // namespace b3
