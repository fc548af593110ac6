// Cleaning and scoring an extracted mesh (binocular3dgs_amd/mesh_tools.py): launch assembly of the ABI 18 calls of
// csrc/meshtools.hip.  Nothing here reads the device or synchronises: the totals of the two count calls stay device words
// (the caller reads them once, between count and emit), and components, the grid, the query and the score can be captured.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kToolsDeviceOnly = "the mesh tools run on the HIP device only";

static Tensor rows3(const Tensor& t, at::ScalarType type, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, type, name, kToolsDeviceOnly, dev).contiguous();
  if (r.dim() != 2 || r.size(1) != 3) throw py::value_error(std::string(name) + " is [n, 3]");
  if (r.size(0) > INT32_MAX) throw py::value_error(std::string(name) + ": more than 2^31 - 1 rows");
  return r;
}

// faces int32 [F, 3] over V vertices -> (labels int32 [V], tri_count int32 [V])
static std::tuple<Tensor, Tensor> mesh_components(int64_t V, const Tensor& faces) {
  Tensor f = rows3(faces, at::kInt, "faces");
  if (V < 0 || V > INT32_MAX) throw py::value_error("mesh_components: 0 <= V <= 2^31 - 1");
  const at::Device dev = f.device();
  auto opt = at::TensorOptions().dtype(at::kInt).device(dev);
  Tensor labels = at::empty({V}, opt), count = at::empty({V}, opt);
  DeviceGuard guard(dev);
  check(b3gs_mesh_components((int32_t)V, f.size(0), ptr_or_null<int32_t>(f), ptr_or_null<int32_t>(labels), ptr_or_null<int32_t>(count),
                             cur_stream(dev)), "b3gs_mesh_components");
  return {labels, count};
}

struct CleanIn {
  Tensor faces, labels, count, threshold;
  int64_t V, F;
};
static CleanIn clean_in(const Tensor& faces, const Tensor& labels, const Tensor& tri_count, const Tensor& threshold) {
  CleanIn c;
  c.faces = rows3(faces, at::kInt, "faces");
  const at::Device dev = c.faces.device();
  c.labels = dev_input(labels, at::kInt, "labels", kToolsDeviceOnly, &dev).contiguous();
  c.count = dev_input(tri_count, at::kInt, "tri_count", kToolsDeviceOnly, &dev).contiguous();
  c.threshold = dev_input(threshold, at::kInt, "threshold", kToolsDeviceOnly, &dev).contiguous();
  if (c.labels.dim() != 1 || c.count.sizes() != c.labels.sizes() || c.threshold.numel() != 1)
    throw py::value_error("mesh_clean: labels and tri_count are int32 [V], threshold is one int32");
  c.V = c.labels.size(0), c.F = c.faces.size(0);
  return c;
}

// -> (workspace, totals): int64 [3] {vertices kept, triangles kept, triangles naming no vertex}, on the device
static std::tuple<Tensor, Tensor> mesh_clean_count(const Tensor& faces, const Tensor& labels, const Tensor& tri_count, const Tensor& threshold) {
  CleanIn c = clean_in(faces, labels, tri_count, threshold);
  const at::Device dev = c.faces.device();
  Tensor ws = byte_workspace(b3gs_mesh_clean_workspace_bytes(c.V, c.F), dev);
  DeviceGuard guard(dev);
  check(b3gs_mesh_clean_count((int32_t)c.V, c.F, ptr_or_null<int32_t>(c.faces), ptr_or_null<int32_t>(c.labels), ptr_or_null<int32_t>(c.count),
                              c.threshold.data_ptr<int32_t>(), ws.data_ptr(), cur_stream(dev)), "b3gs_mesh_clean_count");
  return {ws, head_words(ws, 3)};
}

static std::tuple<Tensor, Tensor, Tensor> mesh_clean_emit(const Tensor& vertices, const Tensor& colours, const Tensor& faces, const Tensor& labels,
                                                          const Tensor& tri_count, const Tensor& threshold, const Tensor& ws, int64_t nverts,
                                                          int64_t ntris) {
  CleanIn c = clean_in(faces, labels, tri_count, threshold);
  const at::Device dev = c.faces.device();
  Tensor v = rows3(vertices, at::kFloat, "vertices", &dev), col = rows3(colours, at::kByte, "colours", &dev);
  Tensor w = dev_input(ws, at::kByte, "workspace", kToolsDeviceOnly, &dev).contiguous();
  if (v.size(0) != c.V || col.size(0) != c.V) throw py::value_error("mesh_clean_emit: one vertex and one colour per label");
  if ((size_t)w.numel() < b3gs_mesh_clean_workspace_bytes(c.V, c.F)) throw py::value_error("mesh_clean_emit: the workspace is too small");
  if (nverts < 0 || ntris < 0 || nverts > c.V || ntris > c.F) throw py::value_error("mesh_clean_emit: bad counts");
  auto opt = at::TensorOptions().device(dev);
  Tensor ov = at::empty({nverts, 3}, opt.dtype(at::kFloat)), oc = at::empty({nverts, 3}, opt.dtype(at::kByte));
  Tensor of = at::empty({ntris, 3}, opt.dtype(at::kInt));
  DeviceGuard guard(dev);
  check(b3gs_mesh_clean_emit((int32_t)c.V, c.F, ptr_or_null<float>(v), ptr_or_null<uint8_t>(col), ptr_or_null<int32_t>(c.faces),
                             ptr_or_null<int32_t>(c.labels), ptr_or_null<int32_t>(c.count), c.threshold.data_ptr<int32_t>(), w.data_ptr(), nverts,
                             ntris, ptr_or_null<float>(ov), ptr_or_null<uint8_t>(oc), ptr_or_null<int32_t>(of), cur_stream(dev)),
        "b3gs_mesh_clean_emit");
  return {ov, oc, of};
}

// -> (workspace, totals): int64 [3] {lattice points, triangles past the 2^15 limit, triangles naming no vertex}
static std::tuple<Tensor, Tensor> mesh_sample_count(const Tensor& vertices, const Tensor& faces, double spacing) {
  Tensor v = rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = rows3(faces, at::kInt, "faces", &dev);
  if (!((float)spacing > 0.f) || !std::isfinite((float)spacing)) throw py::value_error("sample_surface: the spacing is positive and finite");
  Tensor ws = byte_workspace(b3gs_mesh_sample_workspace_bytes(f.size(0)), dev);
  DeviceGuard guard(dev);
  check(b3gs_mesh_sample_count((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<int32_t>(f), (float)spacing, ws.data_ptr(),
                               cur_stream(dev)), "b3gs_mesh_sample_count");
  return {ws, head_words(ws, 3)};
}

static Tensor mesh_sample_emit(const Tensor& vertices, const Tensor& faces, double spacing, const Tensor& ws, int64_t npoints) {
  Tensor v = rows3(vertices, at::kFloat, "vertices");
  const at::Device dev = v.device();
  Tensor f = rows3(faces, at::kInt, "faces", &dev);
  Tensor w = dev_input(ws, at::kByte, "workspace", kToolsDeviceOnly, &dev).contiguous();
  if ((size_t)w.numel() < b3gs_mesh_sample_workspace_bytes(f.size(0))) throw py::value_error("sample_surface: the workspace is too small");
  if (npoints < 0 || v.size(0) + npoints > INT32_MAX) throw py::value_error("sample_surface: more than 2^31 - 1 points: use a larger spacing");
  Tensor out = at::empty({v.size(0) + npoints, 3}, at::TensorOptions().dtype(at::kFloat).device(dev));
  DeviceGuard guard(dev);
  check(b3gs_mesh_sample_emit((int32_t)v.size(0), f.size(0), ptr_or_null<float>(v), ptr_or_null<int32_t>(f), (float)spacing, w.data_ptr(), npoints,
                              ptr_or_null<float>(out), cur_stream(dev)), "b3gs_mesh_sample_emit");
  return out;
}

static void check_max_dist(double max_dist) {
  if (!((float)max_dist > 0.f) || !std::isfinite((float)max_dist)) throw py::value_error("nearest_distances: max_dist is positive and finite");
}

// b float32 [Nb, 3], Nb >= 1 -> the workspace that holds its grid (the grid's parameters are its first 32 bytes)
static Tensor nearest_grid(const Tensor& b, double max_dist) {
  Tensor pts = rows3(b, at::kFloat, "b");
  check_max_dist(max_dist);
  if (pts.size(0) < 1) throw py::value_error("nearest_distances: the cloud searched is empty");
  const at::Device dev = pts.device();
  Tensor ws = byte_workspace(b3gs_nearest_workspace_bytes(pts.size(0)), dev);
  DeviceGuard guard(dev);
  check(b3gs_nearest_grid(pts.size(0), pts.data_ptr<float>(), (float)max_dist, ws.data_ptr(), cur_stream(dev)), "b3gs_nearest_grid");
  return ws;
}

static Tensor nearest_query(const Tensor& a, const Tensor& ws, int64_t nb, double max_dist) {
  Tensor q = rows3(a, at::kFloat, "a");
  check_max_dist(max_dist);
  const at::Device dev = q.device();
  Tensor w = dev_input(ws, at::kByte, "workspace", kToolsDeviceOnly, &dev).contiguous();
  if (nb < 1 || nb > INT32_MAX || (size_t)w.numel() < b3gs_nearest_workspace_bytes(nb)) throw py::value_error("nearest_distances: the workspace is too small");
  Tensor out = at::empty({q.size(0)}, at::TensorOptions().dtype(at::kFloat).device(dev));
  DeviceGuard guard(dev);
  check(b3gs_nearest_query(q.size(0), ptr_or_null<float>(q), nb, (float)max_dist, w.data_ptr(), ptr_or_null<float>(out), cur_stream(dev)),
        "b3gs_nearest_query");
  return out;
}

// -> (dist float32 [Na], index int32 [Na]): the nearest point of b as well, -1 when none lies within max_dist
static std::tuple<Tensor, Tensor> nearest_query_index(const Tensor& a, const Tensor& ws, int64_t nb, double max_dist) {
  Tensor q = rows3(a, at::kFloat, "a");
  check_max_dist(max_dist);
  const at::Device dev = q.device();
  Tensor w = dev_input(ws, at::kByte, "workspace", kToolsDeviceOnly, &dev).contiguous();
  if (nb < 1 || nb > INT32_MAX || (size_t)w.numel() < b3gs_nearest_workspace_bytes(nb)) throw py::value_error("nearest_distances: the workspace is too small");
  Tensor out = at::empty({q.size(0)}, at::TensorOptions().dtype(at::kFloat).device(dev));
  Tensor index = at::empty({q.size(0)}, at::TensorOptions().dtype(at::kInt).device(dev));
  DeviceGuard guard(dev);
  check(b3gs_nearest_query_index(q.size(0), ptr_or_null<float>(q), nb, (float)max_dist, w.data_ptr(), ptr_or_null<float>(out),
                                 ptr_or_null<int32_t>(index), cur_stream(dev)),
        "b3gs_nearest_query_index");
  return {out, index};
}

// dist float32 [N], mask bool [N] or None -> out (float64 [3] on the device, written): sum, count, count below tau
static void cloud_score(const Tensor& dist, const c10::optional<Tensor>& mask, double tau, Tensor out) {
  Tensor d = dev_input(dist, at::kFloat, "dist", kToolsDeviceOnly).contiguous();
  const at::Device dev = d.device();
  if (d.dim() != 1 || d.size(0) < 1 || d.size(0) > INT32_MAX) throw py::value_error("cloud_score: dist is float32 [N], 1 <= N <= 2^31 - 1");
  Tensor m;
  if (mask.has_value()) {
    m = dev_input(*mask, at::kBool, "mask", kToolsDeviceOnly, &dev).contiguous();
    if (m.dim() != 1 || m.size(0) != d.size(0)) throw py::value_error("cloud_score: one mask value per point");
  }
  if (!out.defined() || !out.is_cuda() || out.device() != dev || out.scalar_type() != at::kDouble || out.numel() != 3 || !out.is_contiguous())
    throw py::value_error("cloud_score: out is a contiguous float64 [3] on the device of dist");
  Tensor ws = byte_workspace(b3gs_cloud_score_workspace_bytes(d.size(0)), dev);
  DeviceGuard guard(dev);
  check(b3gs_cloud_score(d.size(0), d.data_ptr<float>(), m.defined() ? reinterpret_cast<const uint8_t*>(m.data_ptr<bool>()) : nullptr, (float)tau,
                         out.data_ptr<double>(), ws.data_ptr(), cur_stream(dev)), "b3gs_cloud_score");
}

void bind_meshtools(py::module_& m) {
  m.def("mesh_components", &mesh_components, py::arg("V"), py::arg("faces"));
  m.def("mesh_clean_count", &mesh_clean_count, py::arg("faces"), py::arg("labels"), py::arg("tri_count"), py::arg("threshold"));
  m.def("mesh_clean_emit", &mesh_clean_emit, py::arg("vertices"), py::arg("colours"), py::arg("faces"), py::arg("labels"), py::arg("tri_count"),
        py::arg("threshold"), py::arg("workspace"), py::arg("nverts"), py::arg("ntris"));
  m.def("mesh_sample_count", &mesh_sample_count, py::arg("vertices"), py::arg("faces"), py::arg("spacing"));
  m.def("mesh_sample_emit", &mesh_sample_emit, py::arg("vertices"), py::arg("faces"), py::arg("spacing"), py::arg("workspace"), py::arg("npoints"));
  m.def("nearest_grid", &nearest_grid, py::arg("b"), py::arg("max_dist"));
  m.def("nearest_query", &nearest_query, py::arg("a"), py::arg("workspace"), py::arg("nb"), py::arg("max_dist"));
  m.def("nearest_query_index", &nearest_query_index, py::arg("a"), py::arg("workspace"), py::arg("nb"), py::arg("max_dist"));
  m.def("cloud_score", &cloud_score, py::arg("dist"), py::arg("mask"), py::arg("tau"), py::arg("out"));
}

}  // namespace b3
