// Editing a trained model (binocular3dgs_amd/edit.py): launch assembly of b3gs_transform_points, b3gs_transform_gaussians,
// b3gs_select_gaussians and b3gs_similarity_sums (b3gs_nearest_query_index sits with its grid in meshtools.cpp).  No autograd,
// no host read, no synchronisation.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_E = "a model is edited on the HIP device only (tests/edit_ref.py holds the numpy statement)";

// xf: 101 doubles in the order of B3gsSimilarity (R 9, t 3, s, ln_s, q 4, D1 9, D2 25, D3 49)
static B3gsSimilarity similarity_of(const std::vector<double>& xf) {
  static_assert(sizeof(B3gsSimilarity) == 101 * sizeof(double), "B3gsSimilarity is 101 doubles");
  if (xf.size() != 101) throw py::value_error("edit: a similarity is 101 doubles (R, t, s, ln s, q, D1, D2, D3)");
  B3gsSimilarity T;
  std::copy(xf.begin(), xf.end(), reinterpret_cast<double*>(&T));
  return T;
}

static Tensor rows_of(const Tensor& t, int64_t cols, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, at::kFloat, name, NO_CPU_E, dev);
  if (r.dim() < 1 || r.numel() != r.size(0) * cols) throw py::value_error(std::string(name) + ": wrong shape");
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

// points float32 [N,3] -> out float32 [N,3] (out may be points itself)
static void transform_points(const Tensor& points, const std::vector<double>& xf, Tensor out) {
  const B3gsSimilarity T = similarity_of(xf);
  Tensor p = rows_of(points, 3, "points");
  const at::Device dev = p.device();
  Tensor o = rows_of(out, 3, "out", &dev);
  if (o.size(0) != p.size(0)) throw py::value_error("transform_points: one output row per point");
  DeviceGuard g(dev);
  check(b3gs_transform_points(p.size(0), ptr_or_null<float>(p), &T, ptr_or_null<float>(o), cur_stream(dev)), "b3gs_transform_points");
}

// the four raw parameter tensors and their outputs (each output may be its input)
static void transform_gaussians(int64_t sh_degree, const Tensor& xyz, const Tensor& rotation, const Tensor& scaling, const Tensor& rest,
                                const std::vector<double>& xf, Tensor out_xyz, Tensor out_rotation, Tensor out_scaling, Tensor out_rest) {
  const B3gsSimilarity T = similarity_of(xf);
  if (sh_degree < 0 || sh_degree > 3) throw py::value_error("transform_gaussians: sh_degree is 0 .. 3");
  const int64_t K = 3 * ((sh_degree + 1) * (sh_degree + 1) - 1);
  Tensor x = rows_of(xyz, 3, "xyz");
  const at::Device dev = x.device();
  const int64_t P = x.size(0);
  if (P > INT32_MAX) throw py::value_error("transform_gaussians: more than 2^31 - 1 Gaussians");
  Tensor r = rows_of(rotation, 4, "rotation", &dev), s = rows_of(scaling, 3, "scaling", &dev);
  Tensor ox = rows_of(out_xyz, 3, "out_xyz", &dev), orr = rows_of(out_rotation, 4, "out_rotation", &dev), os = rows_of(out_scaling, 3, "out_scaling", &dev);
  Tensor f, of;
  if (K > 0) {
    f = rows_of(rest, K, "features_rest", &dev), of = rows_of(out_rest, K, "out_features_rest", &dev);
    if (f.size(0) != P || of.size(0) != P) throw py::value_error("transform_gaussians: one row per Gaussian");
  }
  if (r.size(0) != P || s.size(0) != P || ox.size(0) != P || orr.size(0) != P || os.size(0) != P)
    throw py::value_error("transform_gaussians: one row per Gaussian");
  DeviceGuard g(dev);
  check(b3gs_transform_gaussians((int32_t)P, (int32_t)sh_degree, ptr_or_null<float>(x), ptr_or_null<float>(r), ptr_or_null<float>(s),
                                 K > 0 ? ptr_or_null<float>(f) : nullptr, &T, ptr_or_null<float>(ox), ptr_or_null<float>(orr),
                                 ptr_or_null<float>(os), K > 0 ? ptr_or_null<float>(of) : nullptr, cur_stream(dev)),
        "b3gs_transform_gaussians");
}

// -> (keep uint8 [P], seen int32 [P]).  box: None or 15 doubles (M 3x4 row-major, half 3); sphere: None or (cx, cy, cz, r2);
// cameras: None or float64 [V,19] on the device; masks: None or uint8 [V,H,W] on the device
static std::tuple<Tensor, Tensor> select_gaussians(const Tensor& xyz, const Tensor& opacity, const Tensor& scaling,
                                                   const c10::optional<std::vector<double>>& box, const c10::optional<std::vector<double>>& sphere,
                                                   const c10::optional<double>& logit_min, const c10::optional<double>& log_max_scale,
                                                   const c10::optional<Tensor>& cameras, const c10::optional<Tensor>& masks, int64_t min_views) {
  Tensor x = rows_of(xyz, 3, "xyz");
  const at::Device dev = x.device();
  const int64_t P = x.size(0);
  if (P > INT32_MAX) throw py::value_error("select: more than 2^31 - 1 Gaussians");
  B3gsSelect sel = {};
  Tensor o, s, cams, m;
  if (box.has_value()) {
    if (box->size() != 15) throw py::value_error("select: a box is 15 doubles (M 3x4, half 3)");
    sel.flags |= B3GS_SELECT_BOX;
    for (int k = 0; k < 12; k++) sel.box[k] = (*box)[k];
    for (int k = 0; k < 3; k++) sel.half[k] = (*box)[12 + k];
  }
  if (sphere.has_value()) {
    if (sphere->size() != 4) throw py::value_error("select: a sphere is 4 doubles (centre, r^2)");
    sel.flags |= B3GS_SELECT_SPHERE;
    for (int k = 0; k < 3; k++) sel.centre[k] = (*sphere)[k];
    sel.r2 = (*sphere)[3];
  }
  if (logit_min.has_value()) {
    o = rows_of(opacity, 1, "opacity", &dev);
    if (o.size(0) != P) throw py::value_error("select: one opacity per Gaussian");
    sel.flags |= B3GS_SELECT_OPACITY;
    sel.logit_min = (float)*logit_min;
  }
  if (log_max_scale.has_value()) {
    s = rows_of(scaling, 3, "scaling", &dev);
    if (s.size(0) != P) throw py::value_error("select: one scaling row per Gaussian");
    sel.flags |= B3GS_SELECT_SCALE;
    sel.log_max_scale = (float)*log_max_scale;
  }
  if (cameras.has_value()) {
    cams = dev_input(*cameras, at::kDouble, "cameras", NO_CPU_E, &dev).contiguous();
    if (cams.dim() != 2 || cams.size(1) != 19 || cams.size(0) < 1 || cams.size(0) > B3GS_MAX_SELECT_VIEWS)
      throw py::value_error("select: cameras are float64 [V,19], 1 <= V <= 64");
    sel.flags |= B3GS_SELECT_VIEWS;
    sel.nviews = (int32_t)cams.size(0);
    if (min_views < 0 || min_views > INT32_MAX) throw py::value_error("select: min_views is not negative");
    sel.min_views = (int32_t)min_views;
    sel.cameras = cams.data_ptr<double>();
    if (masks.has_value()) {
      m = dev_input(*masks, at::kByte, "masks", NO_CPU_E, &dev).contiguous();
      if (m.dim() != 3 || m.size(0) != cams.size(0) || m.size(1) < 1 || m.size(2) < 1 || m.size(1) > INT32_MAX || m.size(2) > INT32_MAX)
        throw py::value_error("select: masks are uint8 [V,H,W], one plane per camera");
      sel.mask_h = (int32_t)m.size(1), sel.mask_w = (int32_t)m.size(2);
      sel.masks = m.data_ptr<uint8_t>();
    }
  } else if (masks.has_value()) {
    throw py::value_error("select: masks need cameras");
  }
  Tensor keep = at::empty({P}, at::TensorOptions().dtype(at::kByte).device(dev));
  Tensor seen = at::empty({P}, at::TensorOptions().dtype(at::kInt).device(dev));
  DeviceGuard g(dev);
  check(b3gs_select_gaussians((int32_t)P, ptr_or_null<float>(x), o.defined() ? ptr_or_null<float>(o) : nullptr,
                              s.defined() ? ptr_or_null<float>(s) : nullptr, &sel, ptr_or_null<uint8_t>(keep), ptr_or_null<int32_t>(seen),
                              cur_stream(dev)),
        "b3gs_select_gaussians");
  return std::make_tuple(keep, seen);
}

// a float32 [N,3], b float32 [Nb,3], index int32 [N], dist float32 [N], mask bool [N] or None -> out (float64 [18] on the device, written)
static void similarity_sums(const Tensor& a, const Tensor& b, const Tensor& index, const Tensor& dist, double gate, const c10::optional<Tensor>& mask,
                            const std::vector<double>& origin_a, const std::vector<double>& origin_b, Tensor out) {
  Tensor pa = rows_of(a, 3, "a");
  const at::Device dev = pa.device();
  Tensor pb = rows_of(b, 3, "b", &dev);
  const int64_t N = pa.size(0);
  Tensor idx = dev_input(index, at::kInt, "index", NO_CPU_E, &dev).contiguous(), d = dev_input(dist, at::kFloat, "dist", NO_CPU_E, &dev).contiguous();
  if (N < 1 || N > INT32_MAX || pb.size(0) < 1 || pb.size(0) > INT32_MAX) throw py::value_error("similarity_sums: 1 .. 2^31 - 1 points in each cloud");
  if (idx.dim() != 1 || idx.size(0) != N || d.dim() != 1 || d.size(0) != N) throw py::value_error("similarity_sums: one index and one distance per point of a");
  Tensor m;
  if (mask.has_value()) {
    m = dev_input(*mask, at::kBool, "mask", NO_CPU_E, &dev).contiguous();
    if (m.dim() != 1 || m.size(0) != N) throw py::value_error("similarity_sums: one mask value per point of a");
  }
  if (origin_a.size() != 3 || origin_b.size() != 3) throw py::value_error("similarity_sums: an origin is 3 doubles");
  if (!out.defined() || !out.is_cuda() || out.device() != dev || out.scalar_type() != at::kDouble || out.numel() != 18 || !out.is_contiguous())
    throw py::value_error("similarity_sums: out is a contiguous float64 [18] on the device of a");
  Tensor ws = byte_workspace(b3gs_similarity_sums_workspace_bytes(N), dev);
  DeviceGuard g(dev);
  check(b3gs_similarity_sums(N, pa.data_ptr<float>(), pb.size(0), pb.data_ptr<float>(), idx.data_ptr<int32_t>(), d.data_ptr<float>(), (float)gate,
                             m.defined() ? reinterpret_cast<const uint8_t*>(m.data_ptr<bool>()) : nullptr, origin_a.data(), origin_b.data(),
                             out.data_ptr<double>(), ws.data_ptr(), cur_stream(dev)),
        "b3gs_similarity_sums");
}

void bind_edit(py::module_& m) {
  m.def("transform_points", &transform_points, py::arg("points"), py::arg("xf"), py::arg("out"));
  m.def("transform_gaussians", &transform_gaussians, py::arg("sh_degree"), py::arg("xyz"), py::arg("rotation"), py::arg("scaling"),
        py::arg("features_rest"), py::arg("xf"), py::arg("out_xyz"), py::arg("out_rotation"), py::arg("out_scaling"), py::arg("out_features_rest"));
  m.def("select_gaussians", &select_gaussians, py::arg("xyz"), py::arg("opacity"), py::arg("scaling"), py::arg("box"), py::arg("sphere"),
        py::arg("logit_min"), py::arg("log_max_scale"), py::arg("cameras"), py::arg("masks"), py::arg("min_views"));
  m.def("similarity_sums", &similarity_sums, py::arg("a"), py::arg("b"), py::arg("index"), py::arg("dist"), py::arg("gate"), py::arg("mask"),
        py::arg("origin_a"), py::arg("origin_b"), py::arg("out"));
  m.attr("MAX_SELECT_VIEWS") = B3GS_MAX_SELECT_VIEWS;
}

}  // namespace b3
