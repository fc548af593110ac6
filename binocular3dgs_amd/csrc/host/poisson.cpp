// Screened Poisson surface reconstruction (binocular3dgs_amd/poisson.py): argument checks and launch assembly of
// b3gs_oriented_points_batch / _emit and b3gs_poisson_splat / _apply / _solve / _volume.  Nothing here reads the device or
// synchronises: the sample count and the solver's status words stay device words at the head of a workspace, which the caller
// reads once each.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kPoissonDeviceOnly = "the Poisson reconstruction runs on the HIP device only";

struct ViewSet {
  std::vector<Tensor> keep;
  B3gsTsdfView views[B3GS_MAX_TSDF_VIEWS] = {};
  int32_t n = 0, W = 0, H = 0;
  at::Device dev = at::Device(at::kCPU);
};

// cameras: HOST float32 [n, 14] rows of (rotation 9 row-major, translation 3, fx, fy), world -> camera (mesh.camera_table)
static void view_set(const std::vector<Tensor>& depths, const std::vector<Tensor>& alphas, const std::vector<Tensor>& colours,
                     const Tensor& cameras, ViewSet* out) {
  const size_t n = depths.size();
  if (n < 1 || n > B3GS_MAX_TSDF_VIEWS) throw py::value_error("oriented_points: 1 .. 8 views per call");
  if (alphas.size() != n || colours.size() != n) throw py::value_error("oriented_points: one depth, alpha and colour image per view");
  if (!cameras.defined() || cameras.is_cuda() || cameras.scalar_type() != at::kFloat || cameras.dim() != 2 || cameras.size(0) != (int64_t)n ||
      cameras.size(1) != 14)
    throw py::value_error("oriented_points: cameras is a host float32 [views, 14] table");
  Tensor cam = cameras.contiguous();
  dev_input(depths[0], at::kFloat, "depth", kPoissonDeviceOnly);
  out->dev = depths[0].device();
  int64_t H = 0, W = 0;
  for (size_t v = 0; v < n; v++) {
    Tensor d = dev_input(depths[v], at::kFloat, "depth", kPoissonDeviceOnly, &out->dev), a = dev_input(alphas[v], at::kFloat, "alpha", kPoissonDeviceOnly, &out->dev);
    Tensor c = dev_input(colours[v], at::kFloat, "colour", kPoissonDeviceOnly, &out->dev);
    if (c.dim() != 3 || c.size(0) != 3) throw py::value_error("oriented_points: a colour image is float32 [3, H, W]");
    if (v == 0) H = c.size(1), W = c.size(2);
    if (c.size(1) != H || c.size(2) != W || d.numel() != H * W || a.numel() != H * W || H < 1 || W < 1 || H > INT32_MAX || W > INT32_MAX)
      throw py::value_error("oriented_points: the views of a call share one H x W; depth and alpha hold H * W values");
    d = d.contiguous(), a = a.contiguous(), c = c.contiguous();
    out->keep.push_back(d), out->keep.push_back(a), out->keep.push_back(c);
    out->views[v].depth = d.data_ptr<float>();
    out->views[v].alpha = a.data_ptr<float>();
    out->views[v].colour = c.data_ptr<float>();
    const float* row = cam.data_ptr<float>() + 14 * v;
    for (int q = 0; q < 9; q++) out->views[v].rot[q] = row[q];
    for (int q = 0; q < 3; q++) out->views[v].trans[q] = row[9 + q];
    out->views[v].fx = row[12], out->views[v].fy = row[13];
  }
  out->n = (int32_t)n, out->W = (int32_t)W, out->H = (int32_t)H;
}

// -> (workspace, count): count is the int64 [1] view of the head of the workspace, on the device
static std::tuple<Tensor, Tensor> oriented_points_count(const std::vector<Tensor>& depths, const std::vector<Tensor>& alphas,
                                                        const std::vector<Tensor>& colours, const Tensor& cameras, int64_t stride,
                                                        double alpha_min, double rel_jump, double min_cos, bool median) {
  ViewSet vs;
  view_set(depths, alphas, colours, cameras, &vs);
  if (stride < 1 || stride > INT32_MAX) throw py::value_error("oriented_points: the stride is at least 1");
  const size_t bytes = b3gs_oriented_points_workspace_bytes(vs.n, vs.W, vs.H);
  if (!bytes) throw py::value_error("oriented_points: the images hold 1 .. 2^27 pixels");
  Tensor ws = byte_workspace(bytes, vs.dev);
  {
    DeviceGuard guard(vs.dev);
    check(b3gs_oriented_points_batch(vs.n, vs.views, vs.W, vs.H, (int32_t)stride, (float)alpha_min, (float)rel_jump, (float)min_cos, median ? 1 : 0,
                                     ws.data_ptr(), cur_stream(vs.dev)),
          "b3gs_oriented_points_batch");
  }
  return {ws, head_words(ws, 1)};
}

// -> (points [n, 3], normals [n, 3], weights [n], colours [n, 3]) float32
static std::tuple<Tensor, Tensor, Tensor, Tensor> oriented_points_emit(const std::vector<Tensor>& depths, const std::vector<Tensor>& alphas,
                                                                       const std::vector<Tensor>& colours, const Tensor& cameras, int64_t stride,
                                                                       double alpha_min, double rel_jump, double min_cos, bool median,
                                                                       Tensor workspace, int64_t npoints) {
  ViewSet vs;
  view_set(depths, alphas, colours, cameras, &vs);
  if (stride < 1 || stride > INT32_MAX) throw py::value_error("oriented_points: the stride is at least 1");
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kPoissonDeviceOnly, &vs.dev);
  const size_t bytes = b3gs_oriented_points_workspace_bytes(vs.n, vs.W, vs.H);
  if (!bytes || (size_t)ws.numel() < bytes || !ws.is_contiguous()) throw py::value_error("oriented_points: the workspace is too small");
  if (npoints < 0) throw py::value_error("oriented_points: negative count");
  auto opt = at::TensorOptions().device(vs.dev).dtype(at::kFloat);
  Tensor points = at::empty({npoints, 3}, opt), normals = at::empty({npoints, 3}, opt), weights = at::empty({npoints}, opt);
  Tensor cols = at::empty({npoints, 3}, opt);
  {
    DeviceGuard guard(vs.dev);
    check(b3gs_oriented_points_emit(vs.n, vs.views, vs.W, vs.H, (int32_t)stride, (float)alpha_min, (float)rel_jump, (float)min_cos, median ? 1 : 0,
                                    ws.data_ptr(), npoints, ptr_or_null<float>(points), ptr_or_null<float>(normals), ptr_or_null<float>(weights),
                                    ptr_or_null<float>(cols), cur_stream(vs.dev)),
          "b3gs_oriented_points_emit");
  }
  return {points, normals, weights, cols};
}

static B3gsTsdfVolume grid_of(const std::vector<int64_t>& dims, const std::vector<double>& origin, double voxel, const char* what) {
  if (dims.size() != 3 || origin.size() != 3) throw py::value_error(std::string(what) + ": dims and origin hold 3 numbers");
  for (int d = 0; d < 3; d++)
    if (dims[d] < 1 || dims[d] > B3GS_MAX_TSDF_DIM) throw py::value_error(std::string(what) + ": every dimension of the grid is 1 .. 1024");
  B3gsTsdfVolume g = {};
  g.nx = (int32_t)dims[0], g.ny = (int32_t)dims[1], g.nz = (int32_t)dims[2];
  for (int d = 0; d < 3; d++) g.origin[d] = (float)origin[d];
  g.voxel = (float)voxel;
  return g;
}

// a float32 device array of exactly `count` words, contiguous as it is (written in place or read through a raw pointer)
static Tensor node_array(const Tensor& t, int64_t count, const char* name, const at::Device* dev, const char* what) {
  dev_input(t, at::kFloat, name, kPoissonDeviceOnly, dev);
  if (t.numel() != count || !t.is_contiguous()) throw py::value_error(std::string(what) + ": " + name + " is contiguous and holds one float32 per node");
  return t;
}

static Tensor poisson_ws(const Tensor& workspace, const B3gsTsdfVolume& g, int64_t ns, const at::Device& dev, const char* what) {
  Tensor ws = dev_input(workspace, at::kByte, "workspace", kPoissonDeviceOnly, &dev);
  const size_t bytes = b3gs_poisson_workspace_bytes(g.nx, g.ny, g.nz, ns);
  if (!bytes || (size_t)ws.numel() < bytes || !ws.is_contiguous()) throw py::value_error(std::string(what) + ": the workspace is too small");
  return ws;
}

// -> (density [nz, ny, nx], vector [3, nz, ny, nx], workspace)
static std::tuple<Tensor, Tensor, Tensor> poisson_splat(const Tensor& points, const Tensor& normals, const Tensor& weights, std::vector<int64_t> dims,
                                                        std::vector<double> origin, double voxel, c10::optional<Tensor> workspace) {
  static const char* what = "poisson_splat";
  B3gsTsdfVolume g = grid_of(dims, origin, voxel, what);
  dev_input(points, at::kFloat, "points", kPoissonDeviceOnly);
  const at::Device dev = points.device();
  dev_input(normals, at::kFloat, "normals", kPoissonDeviceOnly, &dev);
  dev_input(weights, at::kFloat, "weights", kPoissonDeviceOnly, &dev);
  if (points.dim() != 2 || points.size(1) != 3 || normals.sizes() != points.sizes() || weights.numel() != points.size(0))
    throw py::value_error("poisson_splat: points and normals are float32 [n, 3], weights is float32 [n]");
  const int64_t ns = points.size(0);
  if (ns >= ((int64_t)1 << 31)) throw py::value_error("poisson_splat: at most 2^31 - 1 samples");
  Tensor p = points.contiguous(), nr = normals.contiguous(), w = weights.contiguous();
  Tensor ws = workspace.has_value() ? poisson_ws(*workspace, g, ns, dev, what) : byte_workspace(b3gs_poisson_workspace_bytes(g.nx, g.ny, g.nz, ns), dev);
  auto opt = at::TensorOptions().device(dev).dtype(at::kFloat);
  Tensor density = at::empty({g.nz, g.ny, g.nx}, opt), vec = at::empty({3, g.nz, g.ny, g.nx}, opt);
  {
    DeviceGuard guard(dev);
    check(b3gs_poisson_splat(&g, ns, ptr_or_null<float>(p), ptr_or_null<float>(nr), ptr_or_null<float>(w), density.data_ptr<float>(),
                             vec.data_ptr<float>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_poisson_splat");
  }
  return {density, vec, ws};
}

static Tensor poisson_apply(const Tensor& density, double screen, const Tensor& x) {
  static const char* what = "poisson_apply";
  dev_input(density, at::kFloat, "density", kPoissonDeviceOnly);
  const at::Device dev = density.device();
  if (density.dim() != 3) throw py::value_error("poisson_apply: density is float32 [nz, ny, nx]");
  B3gsTsdfVolume g = grid_of({density.size(2), density.size(1), density.size(0)}, {0.0, 0.0, 0.0}, 1.0, what);
  node_array(density, density.numel(), "density", &dev, what);
  node_array(x, density.numel(), "x", &dev, what);
  if (!(screen > 0.0)) throw py::value_error("poisson_apply: the screening weight is positive");
  Tensor out = at::empty_like(density);
  DeviceGuard guard(dev);
  check(b3gs_poisson_apply(&g, density.data_ptr<float>(), (float)screen, x.data_ptr<float>(), out.data_ptr<float>(), cur_stream(dev)),
        "b3gs_poisson_apply");
  return out;
}

// -> (x [nz, ny, nx], rhs [nz, ny, nx], state): state is the int64 [8] view of the head of the workspace, on the device --
// {dropped samples, samples, status, iterations, done, bits of r.r, bits of b.b, ..}
static std::tuple<Tensor, Tensor, Tensor> poisson_solve(const Tensor& density, const Tensor& vec, double screen, int64_t iters, double tol,
                                                        Tensor workspace, int64_t max_blocks) {
  static const char* what = "poisson_solve";
  dev_input(density, at::kFloat, "density", kPoissonDeviceOnly);
  const at::Device dev = density.device();
  if (density.dim() != 3) throw py::value_error("poisson_solve: density is float32 [nz, ny, nx]");
  B3gsTsdfVolume g = grid_of({density.size(2), density.size(1), density.size(0)}, {0.0, 0.0, 0.0}, 1.0, what);
  node_array(density, density.numel(), "density", &dev, what);
  dev_input(vec, at::kFloat, "vector", kPoissonDeviceOnly, &dev);
  if (vec.numel() != 3 * density.numel() || !vec.is_contiguous()) throw py::value_error("poisson_solve: vector is contiguous float32 [3, nz, ny, nx]");
  if (!(screen > 0.0)) throw py::value_error("poisson_solve: the screening weight is positive");
  if (iters < 0 || iters > INT32_MAX) throw py::value_error("poisson_solve: the iteration count is not negative");
  if (!(tol >= 0.0)) throw py::value_error("poisson_solve: the tolerance is not negative");
  if (max_blocks < 0 || max_blocks > INT32_MAX) throw py::value_error("poisson_solve: max_blocks is not negative");
  Tensor ws = poisson_ws(workspace, g, 0, dev, what);
  Tensor x = at::empty_like(density), rhs = at::empty_like(density);
  {
    DeviceGuard guard(dev);
    check(b3gs_poisson_solve(&g, density.data_ptr<float>(), vec.data_ptr<float>(), (float)screen, (int32_t)iters, (float)tol, (int32_t)max_blocks,
                             rhs.data_ptr<float>(), x.data_ptr<float>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_poisson_solve");
  }
  return {x, rhs, head_words(ws, 8)};
}

// fills tsdf, weight and rgb of a volume (mesh.TsdfVolume's tensors) in place
static void poisson_volume(Tensor tsdf, Tensor weight, Tensor rgb, const Tensor& density, const Tensor& x, int64_t spread, Tensor workspace) {
  static const char* what = "poisson_volume";
  dev_input(tsdf, at::kFloat, "tsdf", kPoissonDeviceOnly);
  const at::Device dev = tsdf.device();
  if (tsdf.dim() != 3) throw py::value_error("poisson_volume: tsdf is float32 [nz, ny, nx]");
  B3gsTsdfVolume g = grid_of({tsdf.size(2), tsdf.size(1), tsdf.size(0)}, {0.0, 0.0, 0.0}, 1.0, what);
  const int64_t n = tsdf.numel();
  node_array(tsdf, n, "tsdf", &dev, what);
  node_array(weight, n, "weight", &dev, what);
  node_array(density, n, "density", &dev, what);
  node_array(x, n, "x", &dev, what);
  dev_input(rgb, at::kFloat, "rgb", kPoissonDeviceOnly, &dev);
  if (rgb.numel() != 3 * n || !rgb.is_contiguous()) throw py::value_error("poisson_volume: rgb is contiguous float32 [nz, ny, nx, 3]");
  if (spread < 0 || spread > B3GS_MAX_TSDF_DIM) throw py::value_error("poisson_volume: the spread is 0 .. 1024");
  Tensor ws = poisson_ws(workspace, g, 0, dev, what);
  g.tsdf = tsdf.data_ptr<float>(), g.weight = weight.data_ptr<float>(), g.rgb = rgb.data_ptr<float>();
  DeviceGuard guard(dev);
  check(b3gs_poisson_volume(&g, density.data_ptr<float>(), x.data_ptr<float>(), (int32_t)spread, ws.data_ptr(), cur_stream(dev)),
        "b3gs_poisson_volume");
}

void bind_poisson(py::module_& m) {
  m.def("oriented_points_count", &oriented_points_count, py::arg("depths"), py::arg("alphas"), py::arg("colours"), py::arg("cameras"),
        py::arg("stride"), py::arg("alpha_min"), py::arg("rel_jump"), py::arg("min_cos"), py::arg("median") = false);
  m.def("oriented_points_emit", &oriented_points_emit, py::arg("depths"), py::arg("alphas"), py::arg("colours"), py::arg("cameras"),
        py::arg("stride"), py::arg("alpha_min"), py::arg("rel_jump"), py::arg("min_cos"), py::arg("median"), py::arg("workspace"),
        py::arg("npoints"));
  m.def("poisson_splat", &poisson_splat, py::arg("points"), py::arg("normals"), py::arg("weights"), py::arg("dims"), py::arg("origin"),
        py::arg("voxel"), py::arg("workspace") = py::none());
  m.def("poisson_apply", &poisson_apply, py::arg("density"), py::arg("screen"), py::arg("x"));
  m.def("poisson_solve", &poisson_solve, py::arg("density"), py::arg("vector"), py::arg("screen"), py::arg("iters"), py::arg("tol"),
        py::arg("workspace"), py::arg("max_blocks") = 0);
  m.def("poisson_volume", &poisson_volume, py::arg("tsdf"), py::arg("weight"), py::arg("rgb"), py::arg("density"), py::arg("x"),
        py::arg("spread"), py::arg("workspace"));
  m.def("poisson_workspace_bytes", [](int64_t nx, int64_t ny, int64_t nz, int64_t ns) {
    return (nx > INT32_MAX || ny > INT32_MAX || nz > INT32_MAX || nx < 0 || ny < 0 || nz < 0) ? (size_t)0
                                                                                                : b3gs_poisson_workspace_bytes((int32_t)nx, (int32_t)ny, (int32_t)nz, ns);
  });
}

}  // namespace b3
