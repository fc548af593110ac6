// Normal priors (binocular3dgs_amd/normal_prior.py): launch assembly of b3gs_normal_prior_loss_batch, b3gs_depth_normals_batch
// and b3gs_resize_normals_batch.  No autograd here (normal_prior.py owns the Function), no host read, no synchronisation, no
// allocation in the loss call.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_N = "the normal-prior loss runs on the HIP device only (tests/normal_prior_ref.py holds the numpy statement)";

static Tensor planes(const Tensor& t, at::ScalarType type, int64_t C, int64_t H, int64_t W, const char* name, const at::Device* dev) {
  Tensor r = dev_input(t, type, name, NO_CPU_N, dev);
  if (r.numel() != C * H * W || r.dim() < 2 || r.size(-1) != W || r.size(-2) != H) throw py::value_error(std::string(name) + ": wrong shape");
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

static size_t normal_prior_workspace_bytes(int64_t W, int64_t H) {
  if (W > INT32_MAX || H > INT32_MAX || W < 0 || H < 0) return 0;
  return b3gs_normal_prior_workspace_bytes((int32_t)W, (int32_t)H);
}

// views: per view (depth, alpha, target, mask | None, tanfovx, tanfovy, dL_ddepth, dL_dalpha, normals | None, valid | None, parts,
// workspace); every tensor is contiguous, on one device, and written / read in place.
static void normal_prior_loss(const std::vector<py::tuple>& views, double w_cos, double w_l1, double alpha_min) {
  const int n = (int)views.size();
  if (n < 1 || n > B3GS_NORMAL_PRIOR_MAX_VIEWS) throw py::value_error("normal_prior_loss: 1 .. 8 views per call");
  std::vector<B3gsNormalPriorIO> io(n);
  std::vector<Tensor> keep;
  at::Device dev(at::kCPU);
  for (int k = 0; k < n; k++) {
    const py::tuple& v = views[k];
    if (v.size() != 12)
      throw py::value_error("normal_prior_loss: a view is (depth, alpha, target, mask, tanfovx, tanfovy, dL_ddepth, dL_dalpha, normals, valid, parts, workspace)");
    Tensor depth = v[0].cast<Tensor>();
    if (depth.dim() < 2) throw py::value_error("depth: wrong shape");
    const int64_t H = depth.size(-2), W = depth.size(-1);
    depth = dev_input(depth, at::kFloat, "depth", NO_CPU_N, k ? &dev : nullptr);
    if (k == 0) dev = depth.device();
    depth = planes(depth, at::kFloat, 1, H, W, "depth", &dev);
    Tensor alpha = planes(v[1].cast<Tensor>(), at::kFloat, 1, H, W, "alpha", &dev), target = planes(v[2].cast<Tensor>(), at::kFloat, 3, H, W, "target", &dev);
    Tensor gd = planes(v[6].cast<Tensor>(), at::kFloat, 1, H, W, "dL_ddepth", &dev), ga = planes(v[7].cast<Tensor>(), at::kFloat, 1, H, W, "dL_dalpha", &dev);
    Tensor parts = dev_input(v[10].cast<Tensor>(), at::kDouble, "parts", NO_CPU_N, &dev), ws = dev_input(v[11].cast<Tensor>(), at::kByte, "workspace", NO_CPU_N, &dev);
    if (parts.numel() != 6 || !parts.is_contiguous()) throw py::value_error("parts is a contiguous float64 [6]");
    const size_t need = normal_prior_workspace_bytes(W, H);
    if (!need) throw py::value_error("normal_prior_loss: 1 <= W, H, W H <= 2^24");
    if (!ws.is_contiguous() || (size_t)ws.numel() < need) throw py::value_error("workspace: fewer bytes than normal_prior_workspace_bytes(W, H)");
    B3gsNormalPriorIO& s = io[k];
    s.W = (int32_t)W, s.H = (int32_t)H;
    s.depth = depth.data_ptr<float>(), s.alpha = alpha.data_ptr<float>(), s.target = target.data_ptr<float>();
    s.mask = nullptr, s.normals = nullptr, s.valid = nullptr;
    if (!v[3].is_none()) {
      Tensor m = planes(v[3].cast<Tensor>(), at::kByte, 1, H, W, "mask", &dev);
      s.mask = m.data_ptr<uint8_t>();
      keep.push_back(m);
    }
    if (!v[8].is_none()) {
      Tensor m = planes(v[8].cast<Tensor>(), at::kFloat, 3, H, W, "normals", &dev);
      s.normals = m.data_ptr<float>();
      keep.push_back(m);
    }
    if (!v[9].is_none()) {
      Tensor m = planes(v[9].cast<Tensor>(), at::kByte, 1, H, W, "valid", &dev);
      s.valid = m.data_ptr<uint8_t>();
      keep.push_back(m);
    }
    s.alpha_min = (float)alpha_min, s.tanfovx = v[4].cast<double>(), s.tanfovy = v[5].cast<double>();
    s.w_cos = w_cos, s.w_l1 = w_l1;
    s.dL_ddepth = gd.data_ptr<float>(), s.dL_dalpha = ga.data_ptr<float>(), s.parts = parts.data_ptr<double>(), s.workspace = ws.data_ptr();
    keep.insert(keep.end(), {depth, alpha, target, gd, ga, parts, ws});
  }
  DeviceGuard g(dev);
  check(b3gs_normal_prior_loss_batch(n, io.data(), cur_stream(dev)), "b3gs_normal_prior_loss_batch");
}

// views: per view (depth, alpha, mask | None, tanfovx, tanfovy) -> per view (normals float32 [3, H, W], valid uint8 [1, H, W])
static std::vector<std::tuple<Tensor, Tensor>> depth_normals(const std::vector<py::tuple>& views, double alpha_min) {
  std::vector<std::tuple<Tensor, Tensor>> out;
  at::Device dev(at::kCPU);
  std::vector<Tensor> keep;
  for (size_t k0 = 0; k0 < views.size(); k0 += B3GS_NORMAL_PRIOR_MAX_VIEWS) {
    const int n = (int)std::min<size_t>(B3GS_NORMAL_PRIOR_MAX_VIEWS, views.size() - k0);
    std::vector<B3gsDepthNormalsIO> io(n);
    for (int k = 0; k < n; k++) {
      const py::tuple& v = views[k0 + k];
      if (v.size() != 5) throw py::value_error("depth_normals: a view is (depth, alpha, mask, tanfovx, tanfovy)");
      Tensor depth = v[0].cast<Tensor>();
      if (depth.dim() < 2) throw py::value_error("depth: wrong shape");
      const int64_t H = depth.size(-2), W = depth.size(-1);
      depth = dev_input(depth, at::kFloat, "depth", NO_CPU_N, (k0 + k) ? &dev : nullptr);
      if (k0 + k == 0) dev = depth.device();
      depth = planes(depth, at::kFloat, 1, H, W, "depth", &dev);
      if (!normal_prior_workspace_bytes(W, H)) throw py::value_error("depth_normals: 1 <= W, H, W H <= 2^24");
      Tensor alpha = planes(v[1].cast<Tensor>(), at::kFloat, 1, H, W, "alpha", &dev);
      B3gsDepthNormalsIO& s = io[k];
      s.W = (int32_t)W, s.H = (int32_t)H, s.depth = depth.data_ptr<float>(), s.alpha = alpha.data_ptr<float>(), s.mask = nullptr;
      if (!v[2].is_none()) {
        Tensor m = planes(v[2].cast<Tensor>(), at::kByte, 1, H, W, "mask", &dev);
        s.mask = m.data_ptr<uint8_t>();
        keep.push_back(m);
      }
      s.alpha_min = (float)alpha_min, s.tanfovx = v[3].cast<double>(), s.tanfovy = v[4].cast<double>();
      Tensor nn = at::empty({3, H, W}, depth.options()), vv = at::empty({1, H, W}, depth.options().dtype(at::kByte));
      s.normals = nn.data_ptr<float>(), s.valid = vv.data_ptr<uint8_t>();
      keep.insert(keep.end(), {depth, alpha});
      out.emplace_back(nn, vv);
    }
    DeviceGuard g(dev);
    check(b3gs_depth_normals_batch(n, io.data(), cur_stream(dev)), "b3gs_depth_normals_batch");
  }
  return out;
}

// srcs: float32 [3, Hsrc, Wsrc] each; masks: per view None or uint8 [Hsrc, Wsrc] -> per view (normals [3, H, W], mask uint8 [1, H, W])
static std::vector<std::tuple<Tensor, Tensor>> resize_normals(const std::vector<Tensor>& srcs, const std::vector<c10::optional<Tensor>>& masks,
                                                              int64_t W, int64_t H) {
  if (masks.size() != srcs.size()) throw py::value_error("resize_normals: one mask (or None) per source");
  if (W < 1 || H < 1 || W * H > (1 << 24)) throw py::value_error("resize_normals: 1 <= W, H, W H <= 2^24");
  std::vector<std::tuple<Tensor, Tensor>> out;
  at::Device dev(at::kCPU);
  std::vector<Tensor> keep;
  for (size_t k0 = 0; k0 < srcs.size(); k0 += B3GS_NORMAL_PRIOR_MAX_VIEWS) {
    const int n = (int)std::min<size_t>(B3GS_NORMAL_PRIOR_MAX_VIEWS, srcs.size() - k0);
    std::vector<B3gsNormalResizeIO> io(n);
    for (int k = 0; k < n; k++) {
      Tensor s = dev_input(srcs[k0 + k], at::kFloat, "prior", NO_CPU_N, (k0 + k) ? &dev : nullptr);
      if (k0 + k == 0) dev = s.device();
      if (s.dim() != 3 || s.size(0) != 3 || s.numel() < 3 || s.numel() > 3 * (1 << 24))
        throw py::value_error("resize_normals: a prior is [3, Hsrc, Wsrc] with 1 <= Hsrc Wsrc <= 2^24");
      s = s.contiguous();
      B3gsNormalResizeIO& r = io[k];
      r.Hsrc = (int32_t)s.size(1), r.Wsrc = (int32_t)s.size(2), r.W = (int32_t)W, r.H = (int32_t)H;
      r.src = s.data_ptr<float>();
      r.src_mask = nullptr;
      if (masks[k0 + k].has_value()) {
        Tensor m = dev_input(*masks[k0 + k], at::kByte, "mask", NO_CPU_N, &dev).contiguous();
        if (m.dim() != 2 || m.size(0) != s.size(1) || m.size(1) != s.size(2)) throw py::value_error("resize_normals: a mask has the shape of its prior");
        r.src_mask = m.data_ptr<uint8_t>();
        keep.push_back(m);
      }
      Tensor p = at::empty({3, H, W}, s.options()), m = at::empty({1, H, W}, s.options().dtype(at::kByte));
      r.normals = p.data_ptr<float>(), r.mask = m.data_ptr<uint8_t>();
      keep.push_back(s);
      out.emplace_back(p, m);
    }
    DeviceGuard g(dev);
    check(b3gs_resize_normals_batch(n, io.data(), cur_stream(dev)), "b3gs_resize_normals_batch");
  }
  return out;
}

void bind_normalprior(py::module_& m) {
  m.def("normal_prior_workspace_bytes", &normal_prior_workspace_bytes, py::arg("W"), py::arg("H"));
  m.def("normal_prior_loss", &normal_prior_loss, py::arg("views"), py::arg("w_cos"), py::arg("w_l1"), py::arg("alpha_min"));
  m.def("depth_normals", &depth_normals, py::arg("views"), py::arg("alpha_min"));
  m.def("resize_normals", &resize_normals, py::arg("srcs"), py::arg("masks"), py::arg("W"), py::arg("H"));
}

}  // namespace b3
