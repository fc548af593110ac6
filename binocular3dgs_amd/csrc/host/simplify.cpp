// Simplifying an extracted mesh (binocular3dgs_amd/mesh_tools.py simplify / simplify_to): launch assembly of the calls
// of csrc/simplify.hip.  Nothing here reads the device or synchronises: the totals of the count call stay device words, which
// the caller reads once, between count and emit.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kSimplifyDeviceOnly = "the mesh tools run on the HIP device only";
constexpr int kSimplifyWords = 9;     // the int64 words count leaves at the head of the workspace

static Tensor simp_rows3(const Tensor& t, at::ScalarType type, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, type, name, kSimplifyDeviceOnly, dev).contiguous();
  if (r.dim() != 2 || r.size(1) != 3) throw py::value_error(std::string(name) + " is [n, 3]");
  if (r.size(0) > INT32_MAX / 3) throw py::value_error(std::string(name) + ": more than (2^31 - 1) / 3 rows");
  return r;
}
static void check_cell(double cell) {
  if (!((float)cell > 0.f) || !std::isfinite((float)cell)) throw py::value_error("simplify: the cell is positive and finite");
}

// -> (workspace, totals): int64 [9] on the device (include/b3gs_raster.h lists the words)
static std::tuple<Tensor, Tensor> mesh_simplify_count(const Tensor& vertices, const Tensor& faces, double cell) {
  Tensor v = simp_rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = simp_rows3(faces, at::kInt, "faces", &dev);
  check_cell(cell);
  Tensor ws = byte_workspace(b3gs_mesh_simplify_workspace_bytes(v.size(0), f.size(0)), dev);
  DeviceGuard guard(dev);
  check(b3gs_mesh_simplify_count((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<int32_t>(f), (float)cell, ws.data_ptr(),
                                 cur_stream(dev)), "b3gs_mesh_simplify_count");
  return {ws, head_words(ws, kSimplifyWords)};
}

static std::tuple<Tensor, Tensor, Tensor> mesh_simplify_emit(const Tensor& vertices, const Tensor& colours, const Tensor& faces, double cell,
                                                             int64_t placement, const Tensor& ws, int64_t nverts, int64_t ntris) {
  Tensor v = simp_rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor col = simp_rows3(colours, at::kByte, "colours", &dev), f = simp_rows3(faces, at::kInt, "faces", &dev);
  Tensor w = dev_input(ws, at::kByte, "workspace", kSimplifyDeviceOnly, &dev).contiguous();
  check_cell(cell);
  if (col.size(0) != v.size(0)) throw py::value_error("simplify: one colour per vertex");
  if ((size_t)w.numel() < b3gs_mesh_simplify_workspace_bytes(v.size(0), f.size(0))) throw py::value_error("simplify: the workspace is too small");
  if (nverts < 0 || ntris < 0 || nverts > v.size(0) || ntris > f.size(0)) throw py::value_error("simplify: bad counts");
  auto opt = at::TensorOptions().device(dev);
  Tensor ov = at::empty({nverts, 3}, opt.dtype(at::kFloat)), oc = at::empty({nverts, 3}, opt.dtype(at::kByte));
  Tensor of = at::empty({ntris, 3}, opt.dtype(at::kInt));
  DeviceGuard guard(dev);
  check(b3gs_mesh_simplify_emit((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<uint8_t>(col), ptr_or_null<int32_t>(f),
                                (float)cell, (int32_t)placement, w.data_ptr(), nverts, ntris, ptr_or_null<float>(ov), ptr_or_null<uint8_t>(oc),
                                ptr_or_null<int32_t>(of), cur_stream(dev)), "b3gs_mesh_simplify_emit");
  return {ov, oc, of};
}

void bind_simplify(py::module_& m) {
  m.def("mesh_simplify_count", &mesh_simplify_count, py::arg("vertices"), py::arg("faces"), py::arg("cell"));
  m.def("mesh_simplify_emit", &mesh_simplify_emit, py::arg("vertices"), py::arg("colours"), py::arg("faces"), py::arg("cell"),
        py::arg("placement"), py::arg("workspace"), py::arg("nverts"), py::arg("ntris"));
  m.attr("SIMPLIFY_QUADRIC") = B3GS_SIMPLIFY_QUADRIC;
  m.attr("SIMPLIFY_MEAN") = B3GS_SIMPLIFY_MEAN;
}

}  // namespace b3
