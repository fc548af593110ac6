// Texturing an extracted mesh (binocular3dgs_amd/mesh_texture.py): launch assembly of b3gs_mesh_texture_accumulate_batch,
// b3gs_mesh_texture_finalize and b3gs_mesh_resolve_textured_batch.  Nothing here reads the device or synchronises: the bad-face
// count and the coverage stay device words.
#include "common.h"

#include <cmath>
#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kTextureDeviceOnly = "the mesh texture calls run on the HIP device only";

static Tensor rows3(const Tensor& t, at::ScalarType type, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, type, name, kTextureDeviceOnly, dev).contiguous();
  if (r.dim() != 2 || r.size(1) != 3) throw py::value_error(std::string(name) + " is [n, 3]");
  if (r.size(0) > INT32_MAX) throw py::value_error(std::string(name) + ": more than 2^31 - 1 rows");
  return r;
}

struct Atlas {
  int32_t cell, Wt, Ht;
};
static Atlas atlas_in(int64_t F, int64_t cell, int64_t Wt, const char* what) {
  const int32_t Ht = (cell < 0 || cell > INT32_MAX || Wt < 0 || Wt > INT32_MAX) ? 0 : b3gs_mesh_texture_atlas_height(F, (int32_t)cell, (int32_t)Wt);
  if (!Ht) throw py::value_error(std::string(what) + ": no atlas of cell " + std::to_string(cell) + " and width " + std::to_string(Wt) + " for " +
                                 std::to_string(F) + " triangles (4 <= cell <= 256, cell + 1 <= width, width and height <= 16384)");
  return Atlas{(int32_t)cell, (int32_t)Wt, Ht};
}

static Tensor cameras_in(const Tensor& cameras, int64_t W, int64_t H, const char* what) {
  if (!cameras.defined() || cameras.is_cuda() || cameras.scalar_type() != at::kFloat || cameras.dim() != 2 || cameras.size(1) != 14)
    throw py::value_error(std::string(what) + ": cameras is a host float32 [views, 14] table");
  if (cameras.size(0) < 1 || cameras.size(0) > B3GS_MAX_MESH_VIEWS) throw py::value_error(std::string(what) + ": 1 .. 8 views per call");
  if (W < 1 || H < 1 || W > B3GS_MAX_MESH_IMAGE || H > B3GS_MAX_MESH_IMAGE) throw py::value_error(std::string(what) + ": 1 <= W, H <= 16384");
  return cameras.contiguous();
}

static Tensor accum_in(const Tensor& accum, const Atlas& a, const at::Device& dev, const char* what) {
  Tensor acc = dev_input(accum, at::kFloat, "accum", kTextureDeviceOnly, &dev);
  if (acc.dim() != 3 || acc.size(0) != a.Ht || acc.size(1) != a.Wt || acc.size(2) != 4 || !acc.is_contiguous())
    throw py::value_error(std::string(what) + ": accum is a contiguous float32 [Ht, Wt, 4]");
  return acc;
}

// accum float32 [Ht, Wt, 4] is added to in place -> bad_faces int32 [1] on the device
static Tensor mesh_texture_accumulate(const Tensor& vertices, const Tensor& faces, const Tensor& cameras, int64_t W, int64_t H, int64_t cell,
                                      int64_t Wt, const Tensor& triangle_id, const Tensor& depth, const Tensor& images, double slack,
                                      bool two_sided, Tensor accum) {
  static const char* what = "mesh_texture_accumulate";
  Tensor cam = cameras_in(cameras, W, H, what);
  Tensor v = rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = rows3(faces, at::kInt, "faces", &dev);
  const Atlas a = atlas_in(f.size(0), cell, Wt, what);
  if (!((float)slack >= 0.f) || !std::isfinite((float)slack)) throw py::value_error(std::string(what) + ": slack is at least 0 and finite");
  const int64_t n = cam.size(0);
  Tensor id = dev_input(triangle_id, at::kInt, "triangle_id", kTextureDeviceOnly, &dev).contiguous();
  Tensor z = dev_input(depth, at::kFloat, "depth", kTextureDeviceOnly, &dev).contiguous();
  Tensor img = dev_input(images, at::kFloat, "images", kTextureDeviceOnly, &dev).contiguous();
  if (id.sizes() != at::IntArrayRef({n, H, W}) || z.sizes() != at::IntArrayRef({n, 1, H, W}) || img.sizes() != at::IntArrayRef({n, 3, H, W}))
    throw py::value_error(std::string(what) + ": triangle_id is [n, H, W], depth [n, 1, H, W] and images [n, 3, H, W] for the n cameras");
  Tensor acc = accum_in(accum, a, dev, what);
  Tensor bad = at::empty({1}, at::TensorOptions().device(dev).dtype(at::kInt));
  DeviceGuard guard(dev);
  check(b3gs_mesh_texture_accumulate_batch((int32_t)n, cam.data_ptr<float>(), (int32_t)W, (int32_t)H, (int32_t)v.size(0), f.size(0), ptr_or_null<float>(v),
                                           f.data_ptr<int32_t>(), a.cell, a.Wt, a.Ht, id.data_ptr<int32_t>(), z.data_ptr<float>(),
                                           img.data_ptr<float>(), (float)slack, two_sided ? 1 : 0, acc.data_ptr<float>(), bad.data_ptr<int32_t>(),
                                           cur_stream(dev)),
        "b3gs_mesh_texture_accumulate_batch");
  return bad;
}

// -> (texture uint8 [Ht, Wt, 3], coverage int32 [2]) on the device
static std::tuple<Tensor, Tensor> mesh_texture_finalize(int64_t V, c10::optional<Tensor> colours, const Tensor& faces, int64_t cell, int64_t Wt,
                                                        const Tensor& accum) {
  static const char* what = "mesh_texture_finalize";
  Tensor f = rows3(faces, at::kInt, "faces");
  const at::Device dev = f.device();
  if (V < 0 || V > INT32_MAX) throw py::value_error(std::string(what) + ": 0 <= V <= 2^31 - 1");
  const Atlas a = atlas_in(f.size(0), cell, Wt, what);
  Tensor col;
  if (colours.has_value()) {
    col = rows3(*colours, at::kByte, "colours", &dev);
    if (col.size(0) != V) throw py::value_error(std::string(what) + ": one colour per vertex");
  }
  Tensor acc = accum_in(accum, a, dev, what);
  auto opt = at::TensorOptions().device(dev);
  Tensor texture = at::empty({a.Ht, a.Wt, 3}, opt.dtype(at::kByte)), coverage = at::empty({2}, opt.dtype(at::kInt));
  DeviceGuard guard(dev);
  check(b3gs_mesh_texture_finalize((int32_t)V, f.size(0), col.defined() ? ptr_or_null<uint8_t>(col) : nullptr, f.data_ptr<int32_t>(), a.cell, a.Wt,
                                   a.Ht, acc.data_ptr<float>(), texture.data_ptr<uint8_t>(), coverage.data_ptr<int32_t>(), cur_stream(dev)),
        "b3gs_mesh_texture_finalize");
  return {texture, coverage};
}

// mesh_resolve of meshraster.cpp with the colour fetched from the atlas
static std::tuple<Tensor, Tensor, Tensor, Tensor> mesh_resolve_textured(const Tensor& vertices, const Tensor& faces, const Tensor& cameras, int64_t W,
                                                                        int64_t H, const Tensor& workspace, c10::optional<Tensor> bg,
                                                                        const Tensor& texture, int64_t cell, c10::optional<Tensor> face_pixels) {
  static const char* what = "mesh_resolve_textured";
  Tensor cam = cameras_in(cameras, W, H, what);
  Tensor v = rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = rows3(faces, at::kInt, "faces", &dev);
  Tensor tex = dev_input(texture, at::kByte, "texture", kTextureDeviceOnly, &dev).contiguous();
  if (tex.dim() != 3 || tex.size(2) != 3) throw py::value_error(std::string(what) + ": texture is uint8 [Ht, Wt, 3]");
  const Atlas a = atlas_in(f.size(0), cell, tex.size(1), what);
  if (tex.size(0) != a.Ht) throw py::value_error(std::string(what) + ": the texture is not the atlas of this mesh and cell: " + std::to_string(a.Ht) + " rows expected");
  const int32_t n = (int32_t)cam.size(0);
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kTextureDeviceOnly, &dev);
  if ((size_t)ws.numel() < b3gs_mesh_raster_workspace_bytes(n, v.size(0), f.size(0), (int32_t)W, (int32_t)H) || !ws.is_contiguous())
    throw py::value_error(std::string(what) + ": the workspace is too small");
  Tensor back, fp;
  if (bg.has_value()) {
    back = dev_input(*bg, at::kFloat, "bg", kTextureDeviceOnly, &dev).contiguous();
    if (back.numel() != 3) throw py::value_error(std::string(what) + ": bg holds 3 values");
  }
  if (face_pixels.has_value()) {
    fp = dev_input(*face_pixels, at::kInt, "face_pixels", kTextureDeviceOnly, &dev);
    if (fp.dim() != 1 || fp.size(0) != f.size(0) || !fp.is_contiguous()) throw py::value_error(std::string(what) + ": face_pixels is a contiguous int32 [F]");
  }
  auto opt = at::TensorOptions().device(dev);
  Tensor id = at::empty({n, H, W}, opt.dtype(at::kInt)), depth = at::empty({n, 1, H, W}, opt.dtype(at::kFloat));
  Tensor alpha = at::empty({n, 1, H, W}, opt.dtype(at::kFloat)), colour = at::empty({n, 3, H, W}, opt.dtype(at::kFloat));
  DeviceGuard guard(dev);
  check(b3gs_mesh_resolve_textured_batch(n, cam.data_ptr<float>(), (int32_t)W, (int32_t)H, (int32_t)v.size(0), f.size(0), ptr_or_null<float>(v),
                                         f.data_ptr<int32_t>(), ws.data_ptr(), back.defined() ? back.data_ptr<float>() : nullptr,
                                         tex.data_ptr<uint8_t>(), a.cell, a.Wt, a.Ht, id.data_ptr<int32_t>(), depth.data_ptr<float>(),
                                         alpha.data_ptr<float>(), colour.data_ptr<float>(), fp.defined() ? ptr_or_null<int32_t>(fp) : nullptr,
                                         cur_stream(dev)),
        "b3gs_mesh_resolve_textured_batch");
  return {id, depth, alpha, colour};
}

void bind_texture(py::module_& m) {
  m.def("mesh_texture_accumulate", &mesh_texture_accumulate, py::arg("vertices"), py::arg("faces"), py::arg("cameras"), py::arg("W"), py::arg("H"),
        py::arg("cell"), py::arg("Wt"), py::arg("triangle_id"), py::arg("depth"), py::arg("images"), py::arg("slack"), py::arg("two_sided"),
        py::arg("accum"));
  m.def("mesh_texture_finalize", &mesh_texture_finalize, py::arg("V"), py::arg("colours"), py::arg("faces"), py::arg("cell"), py::arg("Wt"),
        py::arg("accum"));
  m.def("mesh_resolve_textured", &mesh_resolve_textured, py::arg("vertices"), py::arg("faces"), py::arg("cameras"), py::arg("W"), py::arg("H"),
        py::arg("workspace"), py::arg("bg"), py::arg("texture"), py::arg("cell"), py::arg("face_pixels") = py::none());
  m.def("mesh_texture_atlas_height", [](int64_t F, int64_t cell, int64_t Wt) {
    return (cell < 0 || cell > INT32_MAX || Wt < 0 || Wt > INT32_MAX) ? 0 : b3gs_mesh_texture_atlas_height(F, (int32_t)cell, (int32_t)Wt);
  });
  m.attr("TEXTURE_MIN_CELL") = B3GS_TEXTURE_MIN_CELL;
  m.attr("TEXTURE_MAX_CELL") = B3GS_TEXTURE_MAX_CELL;
  m.attr("MAX_ATLAS_SIDE") = B3GS_MAX_ATLAS_SIDE;
}

}  // namespace b3
