// The plane-sweep stereo matcher (binocular3dgs_amd/sweep_matcher.py): launch assembly of b3gs_sweep_match_pair.  No host
// read, no synchronisation: the two counts stay device words, so the call can be captured in a graph.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kSweepDeviceOnly = "the sweep matcher runs on the HIP device only";

// -> (kp_source [2,nodes,2], kp_target [2,nodes,2], score [2,nodes], count int32 [2], node_invd [2,nodes], node_score [2,nodes],
//     node_k int32 [2,nodes]); rows [0, count[d]) of direction d (0: a -> b, 1: b -> a) are the kept matches in node order
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> sweep_match_pair(
    const Tensor& image_a, const Tensor& image_b, const Tensor& homographies, const Tensor& proj, double near, double far, double inv_far,
    double step, int64_t stride, int64_t radius, double min_score, double margin, double min_var, double cyc_steps) {
  Tensor ia = dev_input(image_a, at::kByte, "sweep_match_pair: image_a", kSweepDeviceOnly).contiguous();
  const at::Device dev = ia.device();
  Tensor ib = dev_input(image_b, at::kByte, "sweep_match_pair: image_b", kSweepDeviceOnly, &dev).contiguous();
  if (ia.dim() != 3 || ia.size(2) != 3 || ib.dim() != 3 || ib.sizes() != ia.sizes())
    throw py::value_error("sweep_match_pair: image_a and image_b are uint8 [H, W, 3] images of one size");
  Tensor hs = dev_input(homographies, at::kFloat, "homographies", kSweepDeviceOnly, &dev).contiguous();
  Tensor pj = dev_input(proj, at::kFloat, "proj", kSweepDeviceOnly, &dev).contiguous();
  if (hs.dim() != 4 || hs.size(0) != 2 || hs.size(2) != 3 || hs.size(3) != 3) throw py::value_error("sweep_match_pair: homographies is float32 [2, D, 3, 3]");
  if (pj.dim() != 2 || pj.size(0) != 2 || pj.size(1) != 12) throw py::value_error("sweep_match_pair: proj is float32 [2, 12]");
  const int64_t H = ia.size(0), W = ia.size(1), D = hs.size(1);
  if (radius != 3) raise("sweep_match_pair: radius=3 (a 7x7 patch) is the only supported patch");
  const size_t bytes = (W <= INT32_MAX && H <= INT32_MAX && D <= INT32_MAX && stride >= 1 && stride <= INT32_MAX)
                           ? b3gs_sweep_workspace_bytes((int32_t)W, (int32_t)H, (int32_t)D, (int32_t)stride) : 0;
  if (bytes == 0) throw py::value_error("sweep_match_pair: images of at least 7 x 7 pixels, D >= 2 hypotheses and a stride >= 1 are needed");
  const int64_t nodes = ((W - 7) / stride + 1) * ((H - 7) / stride + 1);
  auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  auto i32 = f32.dtype(at::kInt);
  Tensor kp_source = at::empty({2, nodes, 2}, f32), kp_target = at::empty({2, nodes, 2}, f32), score = at::empty({2, nodes}, f32);
  Tensor count = at::empty({2}, i32);
  Tensor node_invd = at::empty({2, nodes}, f32), node_score = at::empty({2, nodes}, f32), node_k = at::empty({2, nodes}, i32);
  Tensor ws = byte_workspace(bytes, dev);
  B3gsSweepPair io = {};
  io.W = (int32_t)W;
  io.H = (int32_t)H;
  io.D = (int32_t)D;
  io.stride = (int32_t)stride;
  io.radius = (int32_t)radius;
  io.near = (float)near;
  io.far = (float)far;
  io.inv_far = (float)inv_far;
  io.step = (float)step;
  io.min_score = (float)min_score;
  io.margin = (float)margin;
  io.min_var = (float)min_var;
  io.cyc_steps = (float)cyc_steps;
  io.image_a = ia.data_ptr<uint8_t>();
  io.image_b = ib.data_ptr<uint8_t>();
  io.homographies = fptr(hs);
  io.proj = fptr(pj);
  io.kp_source = kp_source.data_ptr<float>();
  io.kp_target = kp_target.data_ptr<float>();
  io.score = score.data_ptr<float>();
  io.count = count.data_ptr<int32_t>();
  io.node_invd = node_invd.data_ptr<float>();
  io.node_score = node_score.data_ptr<float>();
  io.node_k = node_k.data_ptr<int32_t>();
  io.workspace = ws.data_ptr();
  {
    DeviceGuard g(dev);
    check(b3gs_sweep_match_pair(&io, cur_stream(dev)), "b3gs_sweep_match_pair");
  }
  return {kp_source, kp_target, score, count, node_invd, node_score, node_k};
}

void bind_sweep(py::module_& m) {
  m.def("sweep_match_pair", &sweep_match_pair, py::arg("image_a"), py::arg("image_b"), py::arg("homographies"), py::arg("proj"),
        py::arg("near"), py::arg("far"), py::arg("inv_far"), py::arg("step"), py::arg("stride") = 2, py::arg("radius") = 3,
        py::arg("min_score") = 0.8, py::arg("margin") = 0.05, py::arg("min_var") = 4.0, py::arg("cyc_steps") = 1.5);
  m.def("sweep_workspace_bytes", [](int64_t W, int64_t H, int64_t D, int64_t stride) {
    return b3gs_sweep_workspace_bytes((int32_t)W, (int32_t)H, (int32_t)D, (int32_t)stride);
  });
}

}  // namespace b3
