// Undistorting a COLMAP dataset (binocular3dgs_amd/undistort.py): launch assembly of b3gs_camera_points, b3gs_undistort_map and
// b3gs_remap_batch.  No autograd, no host read, no synchronisation.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_U = "images are undistorted on the HIP device only (tests/undistort_ref.py holds the numpy statement)";

static B3gsCameraModel camera_of(int64_t model, int64_t width, int64_t height, const std::vector<double>& params) {
  if (params.size() > 12) throw py::value_error("undistort: a camera model has at most 12 parameters");
  B3gsCameraModel c = {};
  c.model = (int32_t)model;
  c.width = (int32_t)width;
  c.height = (int32_t)height;
  c.n_params = (int32_t)params.size();
  for (size_t i = 0; i < params.size(); i++) c.params[i] = params[i];
  return c;
}

// xy float64 [n,2] on the device -> (out float64 [n,2], converged uint8 [n]); converged is all 1 in the distort direction
static std::tuple<Tensor, Tensor> camera_points(int64_t model, int64_t width, int64_t height, const std::vector<double>& params,
                                                const Tensor& xy, bool inverse) {
  const B3gsCameraModel cam = camera_of(model, width, height, params);
  if (xy.defined() && (xy.dim() != 2 || xy.size(1) != 2)) throw py::value_error("camera_points: xy is [n,2]");
  Tensor p = dev_input(xy, at::kDouble, "xy", NO_CPU_U).contiguous();
  const at::Device dev = p.device();
  const int64_t n = p.size(0);
  Tensor out = at::empty_like(p);
  Tensor conv = at::ones({n}, at::TensorOptions().dtype(at::kByte).device(dev));
  DeviceGuard g(dev);
  check(b3gs_camera_points(&cam, inverse ? 1 : 0, n, p.data_ptr<double>(), out.data_ptr<double>(), conv.data_ptr<uint8_t>(),
                           cur_stream(dev)),
        "b3gs_camera_points");
  return std::make_tuple(out, conv);
}

// -> map int32 [H,W,2] on `device`
static Tensor undistort_map(int64_t model, int64_t width, int64_t height, const std::vector<double>& params, int64_t W, int64_t H,
                            double fx, double fy, const at::Device& device) {
  const B3gsCameraModel cam = camera_of(model, width, height, params);
  if (W < 1 || H < 1 || W > INT32_MAX || H > INT32_MAX) throw py::value_error("undistort_map: the output size is at least 1 x 1");
  if (!device.is_cuda()) raise(std::string("the map is asked for on ") + device.str() + ": " + NO_CPU_U);
  Tensor map = at::empty({H, W, 2}, at::TensorOptions().dtype(at::kInt).device(device));
  const at::Device dev = map.device();
  DeviceGuard g(dev);
  check(b3gs_undistort_map(&cam, (int32_t)W, (int32_t)H, fx, fy, map.data_ptr<int32_t>(), cur_stream(dev)), "b3gs_undistort_map");
  return map;
}

// sources: 1..8 uint8 [Hs,Ws,C] (or [Hs,Ws]) tensors of one shape on the device, map int32 [H,W,2] -> (out uint8 [n,H,W,C],
// valid uint8 [H,W])
static std::tuple<Tensor, Tensor> remap(const std::vector<Tensor>& sources, const Tensor& map) {
  const int64_t n = (int64_t)sources.size();
  if (n < 1 || n > B3GS_MAX_REMAP_VIEWS) throw py::value_error("remap: 1..8 images per call");
  if (!map.defined() || map.dim() != 3 || map.size(2) != 2 || map.size(0) < 1 || map.size(1) < 1)
    throw py::value_error("remap: the map is int32 [H,W,2]");
  const Tensor& s0 = sources[0];
  if (!s0.defined() || (s0.dim() != 2 && s0.dim() != 3)) throw py::value_error("remap: a source is a uint8 [Hs,Ws,C] or [Hs,Ws] tensor");
  const int64_t C = s0.dim() == 2 ? 1 : s0.size(2);
  if (C != 1 && C != 3 && C != 4) throw py::value_error("remap: 1, 3 or 4 channels");
  for (const Tensor& s : sources)
    if (!s.defined() || s.sizes() != s0.sizes()) throw py::value_error("remap: the images of one call have one size");
  Tensor m = dev_input(map, at::kInt, "map", NO_CPU_U).contiguous();
  const at::Device dev = m.device();
  std::vector<Tensor> keep;
  keep.reserve(n);
  const uint8_t* src[B3GS_MAX_REMAP_VIEWS];
  uint8_t* dst[B3GS_MAX_REMAP_VIEWS];
  const int64_t H = m.size(0), W = m.size(1);
  Tensor out = at::empty({n, H, W, C}, at::TensorOptions().dtype(at::kByte).device(dev));
  Tensor valid = at::empty({H, W}, at::TensorOptions().dtype(at::kByte).device(dev));
  for (int64_t i = 0; i < n; i++) {
    Tensor c = dev_input(sources[i], at::kByte, "source", NO_CPU_U, &dev).contiguous();
    if ((uintptr_t)c.data_ptr() & 3) c = c.clone();
    keep.push_back(c);
    src[i] = c.data_ptr<uint8_t>();
    dst[i] = out.data_ptr<uint8_t>() + i * H * W * C;
  }
  DeviceGuard g(dev);
  check(b3gs_remap_batch((int32_t)n, src, (int32_t)s0.size(0), (int32_t)s0.size(1), (int32_t)C, m.data_ptr<int32_t>(), (int32_t)H, (int32_t)W,
                         dst, valid.data_ptr<uint8_t>(), cur_stream(dev)),
        "b3gs_remap_batch");
  return std::make_tuple(out, valid);
}

void bind_undistort(py::module_& m) {
  m.def("camera_points", &camera_points, py::arg("model"), py::arg("width"), py::arg("height"), py::arg("params"), py::arg("xy"),
        py::arg("inverse"));
  m.def("undistort_map", &undistort_map, py::arg("model"), py::arg("width"), py::arg("height"), py::arg("params"), py::arg("W"),
        py::arg("H"), py::arg("fx"), py::arg("fy"), py::arg("device"));
  m.def("remap", &remap, py::arg("sources"), py::arg("map"));
  m.attr("MAX_REMAP_VIEWS") = B3GS_MAX_REMAP_VIEWS;
}

}  // namespace b3
