// Smoothing an extracted mesh (binocular3dgs_amd/mesh_tools.py adjacency / smooth / vertex_normals / topology,
// mesh_render.py render_mesh_shaded): launch assembly of the calls of csrc/meshsmooth.hip.  Nothing here reads the device or
// synchronises: the totals of the build stay device words, which the caller reads when it asks for them.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kSmoothDeviceOnly = "the mesh tools run on the HIP device only";
constexpr int kAdjacencyWords = 8;    // the int64 words build leaves at the head of the workspace

static Tensor smooth_rows3(const Tensor& t, at::ScalarType type, const char* name, int64_t max_rows, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, type, name, kSmoothDeviceOnly, dev).contiguous();
  if (r.dim() != 2 || r.size(1) != 3) throw py::value_error(std::string(name) + " is [n, 3]");
  if (r.size(0) > max_rows) throw py::value_error(std::string(name) + ": too many rows (V <= 2^31 - 1, 6 F <= 2^31 - 1)");
  return r;
}
static Tensor adjacency_ws(const Tensor& ws, int64_t V, int64_t F, const at::Device& dev) {
  Tensor w = dev_input(ws, at::kByte, "workspace", kSmoothDeviceOnly, &dev);
  const size_t bytes = b3gs_mesh_adjacency_workspace_bytes(V, F);
  if (!bytes || (size_t)w.numel() < bytes || !w.is_contiguous()) throw py::value_error("adjacency: the workspace is not the one of this mesh");
  return w;
}

// -> the workspace, built
static Tensor mesh_adjacency_build(const Tensor& vertices, const Tensor& faces) {
  Tensor v = smooth_rows3(vertices, at::kFloat, "vertices", INT32_MAX);
  const at::Device dev = v.device();
  Tensor f = smooth_rows3(faces, at::kInt, "faces", INT32_MAX / 6, &dev);
  Tensor ws = byte_workspace(b3gs_mesh_adjacency_workspace_bytes(v.size(0), f.size(0)), dev);
  DeviceGuard guard(dev);
  check(b3gs_mesh_adjacency_build((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<int32_t>(f), ws.data_ptr(), cur_stream(dev)),
        "b3gs_mesh_adjacency_build");
  return ws;
}

// views into a built workspace, no copies: (totals int64 [8], neighbour offsets int32 [V + 1], neighbour indices int32 [6 F],
// incidence ranges int32 [V, 2], incident faces int32 [3 F], pinned-eligible mask uint8 [V])
static std::vector<Tensor> mesh_adjacency_views(const Tensor& ws, int64_t V, int64_t F) {
  if (!ws.defined() || !ws.is_cuda()) raise(std::string("workspace is on ") + (ws.defined() ? ws.device().str() : "no device") + ": " + kSmoothDeviceOnly);
  Tensor w = adjacency_ws(ws, V, F, ws.device());
  size_t off[5];
  check(b3gs_mesh_adjacency_layout(V, F, off), "b3gs_mesh_adjacency_layout");
  auto part = [&](size_t at, int64_t bytes, at::ScalarType type) { return w.slice(0, (int64_t)at, (int64_t)at + bytes).view(type); };
  return {head_words(w, kAdjacencyWords), part(off[0], 4 * (V + 1), at::kInt), part(off[1], 4 * 6 * F, at::kInt),
          part(off[2], 8 * V, at::kInt).reshape({V, 2}), part(off[3], 4 * 3 * F, at::kInt), part(off[4], V, at::kByte)};
}

static Tensor mesh_smooth(const Tensor& vertices, int64_t F, const Tensor& ws, int64_t iterations, double lam, double mu, bool pin_boundary) {
  Tensor v = smooth_rows3(vertices, at::kFloat, "vertices", INT32_MAX);
  const at::Device dev = v.device();
  if (F < 0 || F > INT32_MAX / 6) throw py::value_error("smooth: 0 <= 6 F <= 2^31 - 1");
  if (iterations < 0 || iterations > (1 << 20)) throw py::value_error("smooth: 0 <= iterations <= 2^20");
  Tensor w = adjacency_ws(ws, v.size(0), F, dev);
  Tensor out = at::empty_like(v);
  DeviceGuard guard(dev);
  check(b3gs_mesh_smooth((int32_t)v.size(0), F, ptr_or_null<float>(v), w.data_ptr(), (int32_t)iterations, lam, mu, pin_boundary ? 1 : 0,
                         ptr_or_null<float>(out), cur_stream(dev)), "b3gs_mesh_smooth");
  return out;
}

static Tensor mesh_vertex_normals(const Tensor& vertices, const Tensor& faces, const Tensor& ws) {
  Tensor v = smooth_rows3(vertices, at::kFloat, "vertices", INT32_MAX);
  const at::Device dev = v.device();
  Tensor f = smooth_rows3(faces, at::kInt, "faces", INT32_MAX / 6, &dev);
  Tensor w = adjacency_ws(ws, v.size(0), f.size(0), dev);
  Tensor out = at::empty_like(v);
  DeviceGuard guard(dev);
  check(b3gs_mesh_vertex_normals((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<int32_t>(f), w.data_ptr(),
                                 ptr_or_null<float>(out), cur_stream(dev)), "b3gs_mesh_vertex_normals");
  return out;
}

// mesh_resolve of meshraster.cpp with the colour taken from the vertex normals
static std::tuple<Tensor, Tensor, Tensor, Tensor> mesh_resolve_shaded(const Tensor& normals, const Tensor& faces, const Tensor& cameras, int64_t W,
                                                                      int64_t H, const Tensor& workspace, c10::optional<Tensor> bg, int64_t mode,
                                                                      c10::optional<Tensor> face_pixels) {
  static const char* what = "mesh_resolve_shaded";
  if (!cameras.defined() || cameras.is_cuda() || cameras.scalar_type() != at::kFloat || cameras.dim() != 2 || cameras.size(1) != 14)
    throw py::value_error(std::string(what) + ": cameras is a host float32 [views, 14] table");
  if (cameras.size(0) < 1 || cameras.size(0) > B3GS_MAX_MESH_VIEWS) throw py::value_error(std::string(what) + ": 1 .. 8 views per call");
  if (W < 1 || H < 1 || W > B3GS_MAX_MESH_IMAGE || H > B3GS_MAX_MESH_IMAGE) throw py::value_error(std::string(what) + ": 1 <= W, H <= 16384");
  if (mode != B3GS_MESH_SHADE_SMOOTH && mode != B3GS_MESH_SHADE_LIT) throw py::value_error(std::string(what) + ": unknown mode");
  Tensor cam = cameras.contiguous();
  Tensor nrm = smooth_rows3(normals, at::kFloat, "normals", INT32_MAX);
  const at::Device dev = nrm.device();
  Tensor f = smooth_rows3(faces, at::kInt, "faces", INT32_MAX, &dev);
  const int32_t n = (int32_t)cam.size(0);
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kSmoothDeviceOnly, &dev);
  if ((size_t)ws.numel() < b3gs_mesh_raster_workspace_bytes(n, nrm.size(0), f.size(0), (int32_t)W, (int32_t)H) || !ws.is_contiguous())
    throw py::value_error(std::string(what) + ": the workspace is too small");
  Tensor back, fp;
  if (bg.has_value()) {
    back = dev_input(*bg, at::kFloat, "bg", kSmoothDeviceOnly, &dev).contiguous();
    if (back.numel() != 3) throw py::value_error(std::string(what) + ": bg holds 3 values");
  }
  if (face_pixels.has_value()) {
    fp = dev_input(*face_pixels, at::kInt, "face_pixels", kSmoothDeviceOnly, &dev);
    if (fp.dim() != 1 || fp.size(0) != f.size(0) || !fp.is_contiguous()) throw py::value_error(std::string(what) + ": face_pixels is a contiguous int32 [F]");
  }
  auto opt = at::TensorOptions().device(dev);
  Tensor id = at::empty({n, H, W}, opt.dtype(at::kInt)), depth = at::empty({n, 1, H, W}, opt.dtype(at::kFloat));
  Tensor alpha = at::empty({n, 1, H, W}, opt.dtype(at::kFloat)), colour = at::empty({n, 3, H, W}, opt.dtype(at::kFloat));
  DeviceGuard guard(dev);
  check(b3gs_mesh_resolve_shaded_batch(n, cam.data_ptr<float>(), (int32_t)W, (int32_t)H, (int32_t)nrm.size(0), f.size(0), ptr_or_null<float>(nrm),
                                       ptr_or_null<int32_t>(f), ws.data_ptr(), back.defined() ? back.data_ptr<float>() : nullptr, (int32_t)mode,
                                       id.data_ptr<int32_t>(), depth.data_ptr<float>(), alpha.data_ptr<float>(), colour.data_ptr<float>(),
                                       fp.defined() ? ptr_or_null<int32_t>(fp) : nullptr, cur_stream(dev)),
        "b3gs_mesh_resolve_shaded_batch");
  return {id, depth, alpha, colour};
}

void bind_meshsmooth(py::module_& m) {
  m.def("mesh_adjacency_build", &mesh_adjacency_build, py::arg("vertices"), py::arg("faces"));
  m.def("mesh_adjacency_views", &mesh_adjacency_views, py::arg("workspace"), py::arg("V"), py::arg("F"));
  m.def("mesh_smooth", &mesh_smooth, py::arg("vertices"), py::arg("F"), py::arg("workspace"), py::arg("iterations"), py::arg("lam"), py::arg("mu"),
        py::arg("pin_boundary"));
  m.def("mesh_vertex_normals", &mesh_vertex_normals, py::arg("vertices"), py::arg("faces"), py::arg("workspace"));
  m.def("mesh_resolve_shaded", &mesh_resolve_shaded, py::arg("normals"), py::arg("faces"), py::arg("cameras"), py::arg("W"), py::arg("H"),
        py::arg("workspace"), py::arg("bg"), py::arg("mode"), py::arg("face_pixels") = py::none());
  m.def("mesh_adjacency_workspace_bytes", [](int64_t V, int64_t F) { return b3gs_mesh_adjacency_workspace_bytes(V, F); });
  m.attr("MESH_SHADE_SMOOTH") = B3GS_MESH_SHADE_SMOOTH;
  m.attr("MESH_SHADE_LIT") = B3GS_MESH_SHADE_LIT;
}

}  // namespace b3
