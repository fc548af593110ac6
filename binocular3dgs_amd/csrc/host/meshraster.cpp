// Rendering an extracted mesh (binocular3dgs_amd/mesh_render.py): launch assembly of b3gs_mesh_raster_batch and
// b3gs_mesh_resolve_batch.  Nothing here reads the device or synchronises: the rejected counts stay device words.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kRasterDeviceOnly = "the mesh renderer runs on the HIP device only";

struct MeshIn {
  Tensor v, f, cam;
  at::Device dev;
  int32_t n, W, H;
};

static Tensor rows3(const Tensor& t, at::ScalarType type, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, type, name, kRasterDeviceOnly, dev).contiguous();
  if (r.dim() != 2 || r.size(1) != 3) throw py::value_error(std::string(name) + " is [n, 3]");
  if (r.size(0) > INT32_MAX) throw py::value_error(std::string(name) + ": more than 2^31 - 1 rows");
  return r;
}

static MeshIn mesh_in(const Tensor& vertices, const Tensor& faces, const Tensor& cameras, int64_t W, int64_t H) {
  if (!cameras.defined() || cameras.is_cuda() || cameras.scalar_type() != at::kFloat || cameras.dim() != 2 || cameras.size(1) != 14)
    throw py::value_error("mesh_raster: cameras is a host float32 [views, 14] table");
  if (cameras.size(0) < 1 || cameras.size(0) > B3GS_MAX_MESH_VIEWS) throw py::value_error("mesh_raster: 1 .. 8 views per call");
  if (W < 1 || H < 1 || W > B3GS_MAX_MESH_IMAGE || H > B3GS_MAX_MESH_IMAGE) throw py::value_error("mesh_raster: 1 <= W, H <= 16384");
  Tensor v = rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = rows3(faces, at::kInt, "faces", &dev);
  return MeshIn{v, f, cameras.contiguous(), dev, (int32_t)cameras.size(0), (int32_t)W, (int32_t)H};
}

// -> (workspace, counts): counts is int32 [9] on the device (include/b3gs_raster.h lists the words)
static std::tuple<Tensor, Tensor> mesh_raster(const Tensor& vertices, const Tensor& faces, const Tensor& cameras, int64_t W, int64_t H,
                                              bool cull_backface, int64_t small_box, int64_t wave_box, c10::optional<Tensor> workspace) {
  MeshIn in = mesh_in(vertices, faces, cameras, W, H);
  if (small_box > INT32_MAX || wave_box > INT32_MAX) throw py::value_error("mesh_raster: the thresholds fit int32");
  const size_t bytes = b3gs_mesh_raster_workspace_bytes(in.n, in.v.size(0), in.f.size(0), in.W, in.H);
  Tensor ws = workspace.has_value() ? dev_input(*workspace, at::kByte, "workspace", kRasterDeviceOnly, &in.dev) : byte_workspace(bytes, in.dev);
  if ((size_t)ws.numel() < bytes || !ws.is_contiguous()) throw py::value_error("mesh_raster: the workspace is too small");
  Tensor counts = at::empty({B3GS_MAX_MESH_VIEWS + 1}, at::TensorOptions().device(in.dev).dtype(at::kInt));
  DeviceGuard guard(in.dev);
  check(b3gs_mesh_raster_batch(in.n, in.cam.data_ptr<float>(), in.W, in.H, (int32_t)in.v.size(0), in.f.size(0), ptr_or_null<float>(in.v),
                               ptr_or_null<int32_t>(in.f), cull_backface ? 1 : 0, (int32_t)(small_box < 0 ? -1 : small_box),
                               (int32_t)(wave_box < 0 ? -1 : wave_box), ws.data_ptr(), counts.data_ptr<int32_t>(), cur_stream(in.dev)),
        "b3gs_mesh_raster_batch");
  return {ws, counts};
}

// -> (triangle_id int32 [n, H, W], depth [n, 1, H, W], alpha [n, 1, H, W], colour [n, 3, H, W]); with images = false only
// face_pixels is written and the four are undefined tensors
static std::tuple<Tensor, Tensor, Tensor, Tensor> mesh_resolve(const Tensor& vertices, c10::optional<Tensor> colours, const Tensor& faces,
                                                               const Tensor& cameras, int64_t W, int64_t H, const Tensor& workspace,
                                                               c10::optional<Tensor> bg, int64_t shading, c10::optional<Tensor> face_pixels,
                                                               bool images) {
  MeshIn in = mesh_in(vertices, faces, cameras, W, H);
  if (shading != B3GS_MESH_SHADE_COLOUR && shading != B3GS_MESH_SHADE_NORMAL) throw py::value_error("mesh_resolve: unknown shading");
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kRasterDeviceOnly, &in.dev);
  if ((size_t)ws.numel() < b3gs_mesh_raster_workspace_bytes(in.n, in.v.size(0), in.f.size(0), in.W, in.H) || !ws.is_contiguous())
    throw py::value_error("mesh_resolve: the workspace is too small");
  Tensor col, back, fp;
  if (colours.has_value()) {
    col = rows3(*colours, at::kByte, "colours", &in.dev);
    if (col.size(0) != in.v.size(0)) throw py::value_error("mesh_resolve: one colour per vertex");
  } else if (images && shading == B3GS_MESH_SHADE_COLOUR) {
    throw py::value_error("mesh_resolve: colour shading needs the vertex colours");
  }
  if (bg.has_value()) {
    back = dev_input(*bg, at::kFloat, "bg", kRasterDeviceOnly, &in.dev).contiguous();
    if (back.numel() != 3) throw py::value_error("mesh_resolve: bg holds 3 values");
  }
  if (face_pixels.has_value()) {
    fp = dev_input(*face_pixels, at::kInt, "face_pixels", kRasterDeviceOnly, &in.dev);
    if (fp.dim() != 1 || fp.size(0) != in.f.size(0) || !fp.is_contiguous()) throw py::value_error("mesh_resolve: face_pixels is a contiguous int32 [F]");
  }
  Tensor id, depth, alpha, colour;
  if (images) {
    auto opt = at::TensorOptions().device(in.dev);
    id = at::empty({in.n, in.H, in.W}, opt.dtype(at::kInt));
    depth = at::empty({in.n, 1, in.H, in.W}, opt.dtype(at::kFloat));
    alpha = at::empty({in.n, 1, in.H, in.W}, opt.dtype(at::kFloat));
    colour = at::empty({in.n, 3, in.H, in.W}, opt.dtype(at::kFloat));
  }
  DeviceGuard guard(in.dev);
  check(b3gs_mesh_resolve_batch(in.n, in.cam.data_ptr<float>(), in.W, in.H, (int32_t)in.v.size(0), in.f.size(0), ptr_or_null<float>(in.v),
                                col.defined() ? ptr_or_null<uint8_t>(col) : nullptr, ptr_or_null<int32_t>(in.f), ws.data_ptr(),
                                back.defined() ? back.data_ptr<float>() : nullptr, (int32_t)shading,
                                images ? id.data_ptr<int32_t>() : nullptr, images ? depth.data_ptr<float>() : nullptr,
                                images ? alpha.data_ptr<float>() : nullptr, images ? colour.data_ptr<float>() : nullptr,
                                fp.defined() ? ptr_or_null<int32_t>(fp) : nullptr, cur_stream(in.dev)),
        "b3gs_mesh_resolve_batch");
  return {id, depth, alpha, colour};
}

void bind_meshraster(py::module_& m) {
  m.def("mesh_raster", &mesh_raster, py::arg("vertices"), py::arg("faces"), py::arg("cameras"), py::arg("W"), py::arg("H"),
        py::arg("cull_backface") = false, py::arg("small_box") = -1, py::arg("wave_box") = -1, py::arg("workspace") = py::none());
  m.def("mesh_resolve", &mesh_resolve, py::arg("vertices"), py::arg("colours"), py::arg("faces"), py::arg("cameras"), py::arg("W"),
        py::arg("H"), py::arg("workspace"), py::arg("bg") = py::none(), py::arg("shading") = 0, py::arg("face_pixels") = py::none(),
        py::arg("images") = true);
  m.def("mesh_raster_workspace_bytes", [](int64_t n, int64_t V, int64_t F, int64_t W, int64_t H) {
    return (n < 0 || n > INT32_MAX || W < 0 || W > INT32_MAX || H < 0 || H > INT32_MAX) ? (size_t)0
                                                                                        : b3gs_mesh_raster_workspace_bytes((int32_t)n, V, F, (int32_t)W, (int32_t)H);
  });
  m.attr("MESH_SMALL_BOX") = B3GS_MESH_SMALL_BOX;
  m.attr("MESH_WAVE_BOX") = B3GS_MESH_WAVE_BOX;
  m.attr("MESH_SHADE_COLOUR") = B3GS_MESH_SHADE_COLOUR;
  m.attr("MESH_SHADE_NORMAL") = B3GS_MESH_SHADE_NORMAL;
}

}  // namespace b3
