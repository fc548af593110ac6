// A triangle mesh of a trained scene (binocular3dgs_amd/mesh.py): launch assembly of b3gs_tsdf_integrate_batch, b3gs_mesh_count
// and b3gs_mesh_emit.  Nothing here reads the device or synchronises: the two totals of mesh_count stay device words (the
// caller reads them once, between count and emit), so integrate and count can be captured in a graph.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kMeshDeviceOnly = "the mesh extraction runs on the HIP device only";

// the volume tensors are written in place: they must be contiguous as they are
static B3gsTsdfVolume volume_of(Tensor& tsdf, Tensor& weight, Tensor& rgb, const std::vector<double>& origin, double voxel, const char* what) {
  dev_input(tsdf, at::kFloat, "tsdf", kMeshDeviceOnly);
  const at::Device dev = tsdf.device();
  dev_input(weight, at::kFloat, "weight", kMeshDeviceOnly, &dev);
  dev_input(rgb, at::kFloat, "rgb", kMeshDeviceOnly, &dev);
  if (tsdf.dim() != 3 || weight.sizes() != tsdf.sizes() || rgb.dim() != 4 || rgb.size(3) != 3 || rgb.sizes().slice(0, 3) != tsdf.sizes())
    throw py::value_error(std::string(what) + ": tsdf and weight are float32 [nz, ny, nx], rgb is float32 [nz, ny, nx, 3]");
  if (!tsdf.is_contiguous() || !weight.is_contiguous() || !rgb.is_contiguous())
    throw py::value_error(std::string(what) + ": the volume tensors are contiguous");
  if (origin.size() != 3) throw py::value_error(std::string(what) + ": origin holds 3 numbers");
  for (int d = 0; d < 3; d++)
    if (tsdf.size(d) < 1 || tsdf.size(d) > B3GS_MAX_TSDF_DIM) throw py::value_error(std::string(what) + ": every dimension of the volume is 1 .. 1024");
  B3gsTsdfVolume g = {};
  g.nz = (int32_t)tsdf.size(0), g.ny = (int32_t)tsdf.size(1), g.nx = (int32_t)tsdf.size(2);
  for (int d = 0; d < 3; d++) g.origin[d] = (float)origin[d];
  g.voxel = (float)voxel;
  g.tsdf = tsdf.data_ptr<float>();
  g.weight = weight.data_ptr<float>();
  g.rgb = rgb.data_ptr<float>();
  return g;
}

// cameras: HOST float32 [n, 14] rows of (rotation 9 row-major, translation 3, fx, fy), world -> camera
static void tsdf_integrate(Tensor tsdf, Tensor weight, Tensor rgb, std::vector<double> origin, double voxel, const std::vector<Tensor>& depths,
                           const std::vector<Tensor>& alphas, const std::vector<Tensor>& colours, const Tensor& cameras, double truncation,
                           double near, double alpha_min) {
  static const char* what = "tsdf_integrate";
  B3gsTsdfVolume g = volume_of(tsdf, weight, rgb, origin, voxel, what);
  const at::Device dev = tsdf.device();
  const size_t n = depths.size();
  if (n < 1 || n > B3GS_MAX_TSDF_VIEWS) throw py::value_error("tsdf_integrate: 1 .. 8 views per call");
  if (alphas.size() != n || colours.size() != n) throw py::value_error("tsdf_integrate: one depth, alpha and colour image per view");
  if (!cameras.defined() || cameras.is_cuda() || cameras.scalar_type() != at::kFloat || cameras.dim() != 2 || cameras.size(0) != (int64_t)n ||
      cameras.size(1) != 14)
    throw py::value_error("tsdf_integrate: cameras is a host float32 [views, 14] table");
  Tensor cam = cameras.contiguous();
  std::vector<Tensor> keep;
  B3gsTsdfView views[B3GS_MAX_TSDF_VIEWS] = {};
  int64_t H = 0, W = 0;
  for (size_t v = 0; v < n; v++) {
    Tensor d = dev_input(depths[v], at::kFloat, "depth", kMeshDeviceOnly, &dev), a = dev_input(alphas[v], at::kFloat, "alpha", kMeshDeviceOnly, &dev);
    Tensor c = dev_input(colours[v], at::kFloat, "colour", kMeshDeviceOnly, &dev);
    if (c.dim() != 3 || c.size(0) != 3) throw py::value_error("tsdf_integrate: a colour image is float32 [3, H, W]");
    if (v == 0) H = c.size(1), W = c.size(2);
    if (c.size(1) != H || c.size(2) != W || d.numel() != H * W || a.numel() != H * W || H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX)
      throw py::value_error("tsdf_integrate: the views of a call share one H x W; depth and alpha hold H * W values");
    d = d.contiguous(), a = a.contiguous(), c = c.contiguous();
    keep.push_back(d), keep.push_back(a), keep.push_back(c);
    views[v].depth = d.data_ptr<float>();
    views[v].alpha = a.data_ptr<float>();
    views[v].colour = c.data_ptr<float>();
    const float* row = cam.data_ptr<float>() + 14 * v;
    for (int q = 0; q < 9; q++) views[v].rot[q] = row[q];
    for (int q = 0; q < 3; q++) views[v].trans[q] = row[9 + q];
    views[v].fx = row[12], views[v].fy = row[13];
  }
  DeviceGuard guard(dev);
  check(b3gs_tsdf_integrate_batch(&g, (int32_t)n, views, (int32_t)W, (int32_t)H, (float)truncation, (float)near, (float)alpha_min,
                                  cur_stream(dev)), "b3gs_tsdf_integrate_batch");
}

// -> (workspace, totals): totals is the int64 [2] view {vertices, triangles} of the head of the workspace, on the device
static std::tuple<Tensor, Tensor> mesh_count(Tensor tsdf, Tensor weight, Tensor rgb, std::vector<double> origin, double voxel, double min_weight,
                                             c10::optional<Tensor> workspace) {
  static const char* what = "mesh_count";
  B3gsTsdfVolume g = volume_of(tsdf, weight, rgb, origin, voxel, what);
  const at::Device dev = tsdf.device();
  Tensor ws = workspace.has_value() ? dev_input(*workspace, at::kByte, "workspace", kMeshDeviceOnly, &dev)
                                    : byte_workspace(b3gs_mesh_workspace_bytes(g.nx, g.ny, g.nz), dev);
  if ((size_t)ws.numel() < b3gs_mesh_workspace_bytes(g.nx, g.ny, g.nz) || !ws.is_contiguous()) throw py::value_error("mesh_count: the workspace is too small");
  {
    DeviceGuard guard(dev);
    check(b3gs_mesh_count(&g, (float)min_weight, ws.data_ptr(), cur_stream(dev)), "b3gs_mesh_count");
  }
  return {ws, head_words(ws, 2)};
}

// -> (vertices float32 [V, 3], colours uint8 [V, 3], faces int32 [F, 3])
static std::tuple<Tensor, Tensor, Tensor> mesh_emit(Tensor tsdf, Tensor weight, Tensor rgb, std::vector<double> origin, double voxel, Tensor workspace,
                                                    int64_t nverts, int64_t ntris) {
  static const char* what = "mesh_emit";
  B3gsTsdfVolume g = volume_of(tsdf, weight, rgb, origin, voxel, what);
  const at::Device dev = tsdf.device();
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kMeshDeviceOnly, &dev);
  if ((size_t)ws.numel() < b3gs_mesh_workspace_bytes(g.nx, g.ny, g.nz) || !ws.is_contiguous()) throw py::value_error("mesh_emit: the workspace is too small");
  if (nverts < 0 || ntris < 0) throw py::value_error("mesh_emit: negative count");
  if (nverts > INT32_MAX || ntris > INT32_MAX) raise("mesh_emit: the mesh has more than 2^31 - 1 vertices or triangles: use a coarser volume");
  auto opt = at::TensorOptions().device(dev);
  Tensor vertices = at::empty({nverts, 3}, opt.dtype(at::kFloat)), colours = at::empty({nverts, 3}, opt.dtype(at::kByte));
  Tensor faces = at::empty({ntris, 3}, opt.dtype(at::kInt));
  {
    DeviceGuard guard(dev);
    check(b3gs_mesh_emit(&g, ws.data_ptr(), nverts, ntris, ptr_or_null<float>(vertices), ptr_or_null<uint8_t>(colours),
                         ptr_or_null<int32_t>(faces), cur_stream(dev)),
          "b3gs_mesh_emit");
  }
  return {vertices, colours, faces};
}

void bind_mesh(py::module_& m) {
  m.def("tsdf_integrate", &tsdf_integrate, py::arg("tsdf"), py::arg("weight"), py::arg("rgb"), py::arg("origin"), py::arg("voxel"),
        py::arg("depths"), py::arg("alphas"), py::arg("colours"), py::arg("cameras"), py::arg("truncation"), py::arg("near") = 0.2,
        py::arg("alpha_min") = 0.5);
  m.def("mesh_count", &mesh_count, py::arg("tsdf"), py::arg("weight"), py::arg("rgb"), py::arg("origin"), py::arg("voxel"),
        py::arg("min_weight") = 1.0, py::arg("workspace") = py::none());
  m.def("mesh_emit", &mesh_emit, py::arg("tsdf"), py::arg("weight"), py::arg("rgb"), py::arg("origin"), py::arg("voxel"), py::arg("workspace"),
        py::arg("nverts"), py::arg("ntris"));
  m.def("mesh_workspace_bytes", [](int64_t nx, int64_t ny, int64_t nz) {
    return (nx > INT32_MAX || ny > INT32_MAX || nz > INT32_MAX || nx < 0 || ny < 0 || nz < 0) ? (size_t)0 : b3gs_mesh_workspace_bytes((int32_t)nx, (int32_t)ny, (int32_t)nz);
  });
}

}  // namespace b3
