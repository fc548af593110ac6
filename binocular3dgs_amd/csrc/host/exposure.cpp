// Exposure compensation (binocular3dgs_amd/exposure.py): launch assembly of b3gs_exposure_apply / _backward / _fit / _adam.
// No autograd here (exposure.py owns the Function), no host read, no synchronisation, no allocation.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_E = "exposure compensation runs on the HIP device only (tests/exposure_ref.py holds the numpy statement)";

static Tensor image3(const Tensor& t, int64_t H, int64_t W, const char* name, const at::Device* dev) {
  Tensor r = dev_input(t, at::kFloat, name, NO_CPU_E, dev);
  if (r.dim() != 3 || r.size(0) != 3 || r.size(1) != H || r.size(2) != W) throw py::value_error(std::string(name) + ": a [3, H, W] image is expected");
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

static size_t exposure_workspace_bytes(int64_t W, int64_t H) {
  if (W > INT32_MAX || H > INT32_MAX || W < 0 || H < 0) return 0;
  return b3gs_exposure_workspace_bytes((int32_t)W, (int32_t)H);
}

static void size_of(const py::handle& h, int64_t* H, int64_t* W) {
  Tensor t = h.cast<Tensor>();
  if (t.dim() != 3) throw py::value_error("exposure: a [3, H, W] image is expected");
  *H = t.size(1), *W = t.size(2);
  if (!exposure_workspace_bytes(*W, *H)) throw py::value_error("exposure: 1 <= W, H, W H <= 2^24");
}

// the matrix of a plane: float32 [3, 4] (row None) or a table [V, 3, 4] with an int32 word on the device
static void matrix(B3gsExposurePlane& s, const py::handle& A, const py::handle& row, const at::Device& dev, std::vector<Tensor>& keep) {
  Tensor a = dev_input(A.cast<Tensor>(), at::kFloat, "A", NO_CPU_E, &dev);
  if (!a.is_contiguous()) throw py::value_error("A is contiguous");
  s.row_dev = nullptr, s.V = 0;
  if (row.is_none()) {
    if (a.numel() != 12) throw py::value_error("A: a float32 [3, 4] matrix is expected");
  } else {
    Tensor r = dev_input(row.cast<Tensor>(), at::kInt, "row", NO_CPU_E, &dev);
    if (r.numel() != 1) throw py::value_error("row: one int32 word on the device");
    if (a.numel() < 12 || a.numel() % 12 || a.numel() / 12 > INT32_MAX) throw py::value_error("A: a float32 [V, 3, 4] table is expected");
    s.row_dev = r.data_ptr<int32_t>(), s.V = (int32_t)(a.numel() / 12);
    keep.push_back(r);
  }
  s.A = a.data_ptr<float>();
  keep.push_back(a);
}

// planes: (in, out, A, row | None)
static void exposure_apply(const std::vector<py::tuple>& planes) {
  const int n = (int)planes.size();
  if (n < 1 || n > B3GS_EXPOSURE_MAX_PLANES) throw py::value_error("exposure_apply: 1 .. 8 planes per call");
  std::vector<B3gsExposurePlane> io(n);
  std::vector<Tensor> keep;
  at::Device dev(at::kCPU);
  for (int k = 0; k < n; k++) {
    const py::tuple& p = planes[k];
    if (p.size() != 4) throw py::value_error("exposure_apply: a plane is (in, out, A, row)");
    int64_t H, W;
    size_of(p[0], &H, &W);
    Tensor in = image3(p[0].cast<Tensor>(), H, W, "in", k ? &dev : nullptr);
    if (k == 0) dev = in.device();
    Tensor out = image3(p[1].cast<Tensor>(), H, W, "out", &dev);
    B3gsExposurePlane& s = io[k];
    s = B3gsExposurePlane{};
    s.W = (int32_t)W, s.H = (int32_t)H, s.in = in.data_ptr<float>(), s.out = out.data_ptr<float>();
    matrix(s, p[2], p[3], dev, keep);
    keep.insert(keep.end(), {in, out});
  }
  DeviceGuard g(dev);
  check(b3gs_exposure_apply(n, io.data(), cur_stream(dev)), "b3gs_exposure_apply");
}

// planes: (in, g_out, g_in, A, row | None, G float64 [18], workspace uint8)
static void exposure_backward(const std::vector<py::tuple>& planes) {
  const int n = (int)planes.size();
  if (n < 1 || n > B3GS_EXPOSURE_MAX_PLANES) throw py::value_error("exposure_backward: 1 .. 8 planes per call");
  std::vector<B3gsExposurePlane> io(n);
  std::vector<Tensor> keep;
  at::Device dev(at::kCPU);
  for (int k = 0; k < n; k++) {
    const py::tuple& p = planes[k];
    if (p.size() != 7) throw py::value_error("exposure_backward: a plane is (in, g_out, g_in, A, row, G, workspace)");
    int64_t H, W;
    size_of(p[0], &H, &W);
    Tensor in = image3(p[0].cast<Tensor>(), H, W, "in", k ? &dev : nullptr);
    if (k == 0) dev = in.device();
    Tensor go = image3(p[1].cast<Tensor>(), H, W, "g_out", &dev), gi = image3(p[2].cast<Tensor>(), H, W, "g_in", &dev);
    Tensor G = dev_input(p[5].cast<Tensor>(), at::kDouble, "G", NO_CPU_E, &dev), ws = dev_input(p[6].cast<Tensor>(), at::kByte, "workspace", NO_CPU_E, &dev);
    if (G.numel() != 18 || !G.is_contiguous()) throw py::value_error("G is a contiguous float64 [18]: 12 doubles and their 12 float32 roundings");
    if (!ws.is_contiguous() || (size_t)ws.numel() < exposure_workspace_bytes(W, H)) throw py::value_error("workspace: fewer bytes than exposure_workspace_bytes(W, H)");
    B3gsExposurePlane& s = io[k];
    s = B3gsExposurePlane{};
    s.W = (int32_t)W, s.H = (int32_t)H, s.in = in.data_ptr<float>(), s.g_out = go.data_ptr<float>(), s.out = gi.data_ptr<float>();
    s.G = G.data_ptr<double>(), s.workspace = ws.data_ptr();
    matrix(s, p[3], p[4], dev, keep);
    keep.insert(keep.end(), {in, go, gi, G, ws});
  }
  DeviceGuard g(dev);
  check(b3gs_exposure_backward(n, io.data(), cur_stream(dev)), "b3gs_exposure_backward");
}

// planes: (render, gt, mask uint8 [.., H, W] | None, A float32 [3, 4], sums float64 [23], flag int32 [1], workspace uint8)
static void exposure_fit(const std::vector<py::tuple>& planes) {
  const int n = (int)planes.size();
  if (n < 1 || n > B3GS_EXPOSURE_MAX_PLANES) throw py::value_error("exposure_fit: 1 .. 8 planes per call");
  std::vector<B3gsExposureFitIO> io(n);
  std::vector<Tensor> keep;
  at::Device dev(at::kCPU);
  for (int k = 0; k < n; k++) {
    const py::tuple& p = planes[k];
    if (p.size() != 7) throw py::value_error("exposure_fit: a plane is (render, gt, mask, A, sums, flag, workspace)");
    int64_t H, W;
    size_of(p[0], &H, &W);
    Tensor r = image3(p[0].cast<Tensor>(), H, W, "render", k ? &dev : nullptr);
    if (k == 0) dev = r.device();
    Tensor gt = image3(p[1].cast<Tensor>(), H, W, "gt", &dev);
    Tensor A = dev_input(p[3].cast<Tensor>(), at::kFloat, "A", NO_CPU_E, &dev), sums = dev_input(p[4].cast<Tensor>(), at::kDouble, "sums", NO_CPU_E, &dev);
    Tensor flag = dev_input(p[5].cast<Tensor>(), at::kInt, "flag", NO_CPU_E, &dev), ws = dev_input(p[6].cast<Tensor>(), at::kByte, "workspace", NO_CPU_E, &dev);
    if (A.numel() != 12 || !A.is_contiguous() || sums.numel() != 23 || !sums.is_contiguous() || flag.numel() != 1)
      throw py::value_error("exposure_fit: A is float32 [3, 4], sums float64 [23], flag int32 [1], all contiguous");
    if (!ws.is_contiguous() || (size_t)ws.numel() < exposure_workspace_bytes(W, H)) throw py::value_error("workspace: fewer bytes than exposure_workspace_bytes(W, H)");
    B3gsExposureFitIO& s = io[k];
    s = B3gsExposureFitIO{};
    s.W = (int32_t)W, s.H = (int32_t)H, s.render = r.data_ptr<float>(), s.gt = gt.data_ptr<float>();
    if (!p[2].is_none()) {
      Tensor m = dev_input(p[2].cast<Tensor>(), at::kByte, "mask", NO_CPU_E, &dev);
      if (m.numel() != H * W || !m.is_contiguous()) throw py::value_error("mask: a contiguous uint8 [H, W] plane is expected");
      s.mask = m.data_ptr<uint8_t>();
      keep.push_back(m);
    }
    s.A = A.data_ptr<float>(), s.sums = sums.data_ptr<double>(), s.flag = flag.data_ptr<int32_t>(), s.workspace = ws.data_ptr();
    keep.insert(keep.end(), {r, gt, A, sums, flag, ws});
  }
  DeviceGuard g(dev);
  check(b3gs_exposure_fit(n, io.data(), cur_stream(dev)), "b3gs_exposure_fit");
}

static void exposure_adam(Tensor table, Tensor exp_avg, Tensor exp_avg_sq, Tensor steps, Tensor prods, Tensor row, Tensor grad, Tensor lr,
                          double beta1, double beta2, double eps, const c10::optional<Tensor>& skip) {
  table = dev_input(table, at::kFloat, "table", NO_CPU_E);
  const at::Device dev = table.device();
  exp_avg = dev_input(exp_avg, at::kFloat, "exp_avg", NO_CPU_E, &dev), exp_avg_sq = dev_input(exp_avg_sq, at::kFloat, "exp_avg_sq", NO_CPU_E, &dev);
  steps = dev_input(steps, at::kInt, "steps", NO_CPU_E, &dev), prods = dev_input(prods, at::kDouble, "prods", NO_CPU_E, &dev);
  row = dev_input(row, at::kInt, "row", NO_CPU_E, &dev), grad = dev_input(grad, at::kDouble, "grad", NO_CPU_E, &dev);
  lr = dev_input(lr, at::kFloat, "lr", NO_CPU_E, &dev);
  const int64_t V = table.numel() / 12;
  if (V < 1 || V > INT32_MAX || table.numel() != 12 * V || exp_avg.numel() != 12 * V || exp_avg_sq.numel() != 12 * V || steps.numel() != V ||
      prods.numel() != 2 * V || row.numel() != 1 || grad.numel() < 12 || lr.numel() != 1)
    throw py::value_error("exposure_adam: table / exp_avg / exp_avg_sq [V, 3, 4], steps [V], prods [V, 2], row [1], grad [>= 12], lr [1]");
  for (const Tensor* t : {&table, &exp_avg, &exp_avg_sq, &steps, &prods, &grad})
    if (!t->is_contiguous()) throw py::value_error("exposure_adam: every tensor is contiguous");
  const int32_t* skip_ptr = nullptr;
  if (skip.has_value() && skip->defined()) {
    Tensor s = dev_input(*skip, at::kInt, "skip_if_nonzero", NO_CPU_E, &dev);
    if (s.numel() < 1) throw py::value_error("skip_if_nonzero: one int32 word on the device");
    skip_ptr = s.data_ptr<int32_t>();
  }
  DeviceGuard g(dev);
  check(b3gs_exposure_adam((int32_t)V, table.data_ptr<float>(), exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), steps.data_ptr<int32_t>(),
                           prods.data_ptr<double>(), row.data_ptr<int32_t>(), grad.data_ptr<double>(), lr.data_ptr<float>(), beta1, beta2, eps,
                           skip_ptr, cur_stream(dev)),
        "b3gs_exposure_adam");
}

void bind_exposure(py::module_& m) {
  m.def("exposure_workspace_bytes", &exposure_workspace_bytes, py::arg("W"), py::arg("H"));
  m.def("exposure_apply", &exposure_apply, py::arg("planes"));
  m.def("exposure_backward", &exposure_backward, py::arg("planes"));
  m.def("exposure_fit", &exposure_fit, py::arg("planes"));
  m.def("exposure_adam", &exposure_adam, py::arg("table"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("steps"), py::arg("prods"),
        py::arg("row"), py::arg("grad"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("skip_if_nonzero") = py::none());
}

}  // namespace b3
