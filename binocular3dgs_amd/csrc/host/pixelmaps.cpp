// Per-pixel geometry maps (binocular3dgs_amd/pixel_maps.py): launch assembly of b3gs_blend_pixel_maps_batch over the state
// buffers a FusedRasterizer forward left in its slots.  No autograd: there is no backward through the maps.
#include "walk_state.h"

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_P = "the pixel maps run on the HIP device only (there is no host statement of the tile walk)";
static const char* const PLANES[5] = {"median_depth", "depth_m1", "depth_m2", "dominant", "count"};

// views: 1..8 tuples (geometry, binning, image, P, W, H) -- the three uint8 state buffers of one view's forward, the Gaussian
// count of the model and the view's size; outs: per view a tuple (median_depth, depth_m1, depth_m2, dominant, count) of
// contiguous [H,W] tensors, float32 the first three, int32 the last two, any of them None (that plane is not written).
static void blend_pixel_maps(const py::list& views, const py::list& outs) {
  const size_t n = views.size();
  if (n == 0 || n > 8) throw py::value_error("blend_pixel_maps: 1..8 views");
  if (outs.size() != n) throw py::value_error("blend_pixel_maps: one tuple of output planes per view");
  std::vector<Tensor> keep;
  keep.reserve(8 * n);
  B3gsScene sc[8];
  B3gsPixelMapView pv[8];
  at::Device dev(at::kCPU);
  int64_t P0 = -1;
  for (size_t k = 0; k < n; ++k) {
    py::tuple t = views[k].cast<py::tuple>();
    if (t.size() != 6) throw py::value_error("blend_pixel_maps: a view is (geometry, binning, image, P, W, H)");
    const int64_t P = t[3].cast<int64_t>();
    if (P < 0 || P > INT32_MAX) throw py::value_error("blend_pixel_maps: P is the number of Gaussians");
    if (k == 0) P0 = P;
    if (P != P0) throw py::value_error("blend_pixel_maps: the views of one call share P");
    const ViewState s = view_state(t, 4, P, k ? &dev : nullptr, keep, sc[k], "blend_pixel_maps", NO_CPU_P);
    dev = s.dev;
    pv[k] = B3gsPixelMapView{};
    pv[k].view = &sc[k], pv[k].geometry = s.geometry, pv[k].binning = s.binning, pv[k].image = s.image;
    py::tuple o = outs[k].cast<py::tuple>();
    if (o.size() != 5) throw py::value_error("blend_pixel_maps: the planes of a view are (median_depth, depth_m1, depth_m2, dominant, count)");
    void* ptr[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int j = 0; j < 5; ++j) {
      if (o[j].is_none()) continue;
      Tensor x = dev_input(o[j].cast<Tensor>(), j < 3 ? at::kFloat : at::kInt, PLANES[j], NO_CPU_P, &dev);
      if (x.dim() != 2 || x.size(0) != s.H || x.size(1) != s.W) throw py::value_error(std::string("blend_pixel_maps: ") + PLANES[j] + " is [H, W]");
      if (!x.is_contiguous()) throw py::value_error("blend_pixel_maps: the planes are written in place and must be contiguous");
      keep.push_back(x);
      ptr[j] = x.data_ptr();
    }
    pv[k].median_depth = (float*)ptr[0], pv[k].depth_m1 = (float*)ptr[1], pv[k].depth_m2 = (float*)ptr[2];
    pv[k].dominant = (int32_t*)ptr[3], pv[k].count = (int32_t*)ptr[4];
  }
  DeviceGuard g(dev);
  check(b3gs_blend_pixel_maps_batch((int32_t)n, pv, cur_stream(dev)), "b3gs_blend_pixel_maps_batch");
}

void bind_pixelmaps(py::module_& m) {
  m.def("blend_pixel_maps", &blend_pixel_maps, py::arg("views"), py::arg("outs"));
}

}  // namespace b3
