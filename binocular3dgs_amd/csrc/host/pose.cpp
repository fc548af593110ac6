// The camera pose gradient (binocular3dgs_amd/pose.py): launch assembly of b3gs_pose_gradient.  No autograd, no host read, no
// synchronisation.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_P = "the pose gradient is reduced on the HIP device only (tests/pose_ref.py holds the numpy statement)";

static Tensor pose_rows(const Tensor& t, int64_t P, int64_t cols, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, at::kFloat, name, NO_CPU_P, dev);
  if (r.dim() < 1 || r.size(0) != P || r.numel() != P * cols) throw py::value_error(std::string(name) + ": wrong shape");
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

// xyz [P,3], rotation [P,4], features_rest [P,K,3] (ignored at sh_degree 0); per view one gradient of each and, optionally, a
// uint8 / bool [P] of rows to leave out; pivot: 3 doubles; out: float64 [V,6] on the device, written (the SCENE twist gradient)
static void pose_gradient(int64_t sh_degree, const Tensor& xyz, const Tensor& rotation, const Tensor& rest, const std::vector<Tensor>& grad_xyz,
                          const std::vector<Tensor>& grad_rotation, const std::vector<Tensor>& grad_rest,
                          const c10::optional<std::vector<c10::optional<Tensor>>>& skip, const std::vector<double>& pivot, Tensor out) {
  if (sh_degree < 0 || sh_degree > 3) throw py::value_error("pose_gradient: sh_degree is 0 .. 3");
  const int64_t K = 3 * ((sh_degree + 1) * (sh_degree + 1) - 1);
  const int64_t V = (int64_t)grad_xyz.size();
  if (V < 1 || V > B3GS_MAX_POSE_VIEWS) throw py::value_error("pose_gradient: 1 .. 8 views per call");
  if ((int64_t)grad_rotation.size() != V || (K > 0 && (int64_t)grad_rest.size() != V) || (skip.has_value() && (int64_t)skip->size() != V))
    throw py::value_error("pose_gradient: one gradient of each parameter (and one skip entry) per view");
  if (pivot.size() != 3) throw py::value_error("pose_gradient: the pivot is 3 doubles");
  if (xyz.dim() != 2 || xyz.size(1) != 3) throw py::value_error("xyz: wrong shape");
  const int64_t P = xyz.size(0);
  if (P > INT32_MAX) throw py::value_error("pose_gradient: more than 2^31 - 1 Gaussians");
  Tensor x = pose_rows(xyz, P, 3, "xyz");
  const at::Device dev = x.device();
  Tensor r = pose_rows(rotation, P, 4, "rotation", &dev), f;
  if (K > 0) f = pose_rows(rest, P, K, "features_rest", &dev);
  std::vector<Tensor> keep;                      // (owners of what the pointer arrays below name)
  std::vector<const float*> gx(V), gr(V), gf(V, nullptr);
  std::vector<const uint8_t*> sk(V, nullptr);
  for (int64_t v = 0; v < V; v++) {
    keep.push_back(pose_rows(grad_xyz[v], P, 3, "grad_xyz", &dev));
    gx[v] = ptr_or_null<float>(keep.back());
    keep.push_back(pose_rows(grad_rotation[v], P, 4, "grad_rotation", &dev));
    gr[v] = ptr_or_null<float>(keep.back());
    if (K > 0) {
      keep.push_back(pose_rows(grad_rest[v], P, K, "grad_features_rest", &dev));
      gf[v] = ptr_or_null<float>(keep.back());
    }
    if (skip.has_value() && (*skip)[v].has_value()) {
      const Tensor& s = *(*skip)[v];
      if (!s.defined() || !s.is_cuda()) raise(std::string("skip is on ") + (s.defined() ? s.device().str() : "no device") + ": " + NO_CPU_P);
      if (s.device() != dev) raise("skip is on " + s.device().str() + ", not on " + dev.str());
      if (s.scalar_type() != at::kByte && s.scalar_type() != at::kBool) throw py::value_error("skip: uint8 or bool");
      if (s.dim() != 1 || s.size(0) != P || !s.is_contiguous()) throw py::value_error("skip: a contiguous [P]");
      keep.push_back(s);
      sk[v] = P ? static_cast<const uint8_t*>(s.data_ptr()) : nullptr;
    }
  }
  if (!out.defined() || !out.is_cuda() || out.device() != dev || out.scalar_type() != at::kDouble || out.dim() != 2 || out.size(0) != V ||
      out.size(1) != 6 || !out.is_contiguous())
    throw py::value_error("pose_gradient: out is a contiguous float64 [V,6] on the device of xyz");
  Tensor ws = byte_workspace(b3gs_pose_gradient_workspace_bytes((int32_t)P, (int32_t)V), dev);
  DeviceGuard g(dev);
  check(b3gs_pose_gradient((int32_t)P, (int32_t)sh_degree, (int32_t)V, ptr_or_null<float>(x), ptr_or_null<float>(r),
                           K > 0 ? ptr_or_null<float>(f) : nullptr, gx.data(), gr.data(), gf.data(), sk.data(), pivot.data(),
                           out.data_ptr<double>(), P ? ws.data_ptr() : nullptr, cur_stream(dev)),
        "b3gs_pose_gradient");
}

void bind_pose(py::module_& m) {
  m.def("pose_gradient", &pose_gradient, py::arg("sh_degree"), py::arg("xyz"), py::arg("rotation"), py::arg("features_rest"), py::arg("grad_xyz"),
        py::arg("grad_rotation"), py::arg("grad_features_rest"), py::arg("skip"), py::arg("pivot"), py::arg("out"));
  m.attr("MAX_POSE_VIEWS") = B3GS_MAX_POSE_VIEWS;
}

}  // namespace b3
