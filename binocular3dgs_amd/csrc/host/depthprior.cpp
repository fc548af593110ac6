// Depth priors (binocular3dgs_amd/depth_prior.py): launch assembly of b3gs_depth_prior_loss_batch and b3gs_resize_depth_batch.
// No autograd here (depth_prior.py owns the Function), no host read, no synchronisation, no allocation in the loss call.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_D = "the depth-prior loss runs on the HIP device only (tests/depth_prior_ref.py holds the numpy statement)";

static Tensor plane(const Tensor& t, at::ScalarType type, int64_t H, int64_t W, const char* name, const at::Device* dev) {
  Tensor r = dev_input(t, type, name, NO_CPU_D, dev);
  if (r.numel() != H * W || r.dim() < 2 || r.size(-1) != W || r.size(-2) != H) throw py::value_error(std::string(name) + ": wrong shape");
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

static size_t depth_prior_workspace_bytes(int64_t W, int64_t H, int64_t patch) {
  if (W > INT32_MAX || H > INT32_MAX || patch > INT32_MAX || W < 0 || H < 0 || patch < 0) return 0;
  return b3gs_depth_prior_workspace_bytes((int32_t)W, (int32_t)H, (int32_t)patch);
}

// views: per view (depth, alpha, prior, mask, offset_dev | None, dL_ddepth, parts, workspace); every tensor is contiguous, on
// one device, and written / read in place.  dL_ddepth float32 [.., H, W], parts float64 [8], workspace uint8 (zeroed once).
static void depth_prior_loss(const std::vector<py::tuple>& views, int64_t mode, double w_global, double w_local, int64_t patch,
                             int64_t min_valid, double alpha_min) {
  const int n = (int)views.size();
  if (n < 1 || n > B3GS_DEPTH_PRIOR_MAX_VIEWS) throw py::value_error("depth_prior_loss: 1 .. 8 views per call");
  if (min_valid < 2 || min_valid > INT32_MAX) throw py::value_error("depth_prior_loss: min_valid >= 2");
  std::vector<B3gsDepthPriorIO> io(n);
  std::vector<Tensor> keep;
  at::Device dev(at::kCPU);
  for (int k = 0; k < n; k++) {
    const py::tuple& v = views[k];
    if (v.size() != 8) throw py::value_error("depth_prior_loss: a view is (depth, alpha, prior, mask, offset_dev, dL_ddepth, parts, workspace)");
    Tensor depth = v[0].cast<Tensor>();
    if (depth.dim() < 2) throw py::value_error("depth: wrong shape");
    const int64_t H = depth.size(-2), W = depth.size(-1);
    depth = dev_input(depth, at::kFloat, "depth", NO_CPU_D, k ? &dev : nullptr);
    if (k == 0) dev = depth.device();
    depth = plane(depth, at::kFloat, H, W, "depth", &dev);
    Tensor alpha = plane(v[1].cast<Tensor>(), at::kFloat, H, W, "alpha", &dev), prior = plane(v[2].cast<Tensor>(), at::kFloat, H, W, "prior", &dev);
    Tensor mask = plane(v[3].cast<Tensor>(), at::kByte, H, W, "mask", &dev), grad = plane(v[5].cast<Tensor>(), at::kFloat, H, W, "dL_ddepth", &dev);
    Tensor parts = dev_input(v[6].cast<Tensor>(), at::kDouble, "parts", NO_CPU_D, &dev), ws = dev_input(v[7].cast<Tensor>(), at::kByte, "workspace", NO_CPU_D, &dev);
    if (parts.numel() != 8 || !parts.is_contiguous()) throw py::value_error("parts is a contiguous float64 [8]");
    const size_t need = depth_prior_workspace_bytes(W, H, patch);
    if (!need) throw py::value_error("depth_prior_loss: 1 <= W, H, W H <= 2^24; patch is 0 or 8 .. 256");
    if (!ws.is_contiguous() || (size_t)ws.numel() < need) throw py::value_error("workspace: fewer bytes than depth_prior_workspace_bytes(W, H, patch)");
    B3gsDepthPriorIO& s = io[k];
    s.W = (int32_t)W, s.H = (int32_t)H;
    s.depth = depth.data_ptr<float>(), s.alpha = alpha.data_ptr<float>(), s.prior = prior.data_ptr<float>(), s.mask = mask.data_ptr<uint8_t>();
    s.mode = (int32_t)mode, s.patch = (int32_t)patch, s.min_valid = (int32_t)min_valid, s.alpha_min = (float)alpha_min;
    s.w_global = w_global, s.w_local = w_local;
    s.offset_dev = nullptr;
    if (!v[4].is_none()) {
      Tensor off = dev_input(v[4].cast<Tensor>(), at::kInt, "offset_dev", NO_CPU_D, &dev);
      if (off.numel() != 2 || !off.is_contiguous()) throw py::value_error("offset_dev is a contiguous int32 [2]");
      s.offset_dev = off.data_ptr<int32_t>();
      keep.push_back(off);
    }
    s.dL_ddepth = grad.data_ptr<float>(), s.parts = parts.data_ptr<double>(), s.workspace = ws.data_ptr();
    keep.insert(keep.end(), {depth, alpha, prior, mask, grad, parts, ws});
  }
  DeviceGuard g(dev);
  check(b3gs_depth_prior_loss_batch(n, io.data(), cur_stream(dev)), "b3gs_depth_prior_loss_batch");
}

// srcs: float32 [Hsrc, Wsrc] each; masks: per view None or uint8 [Hsrc, Wsrc] -> per view (prior float32 [1, H, W], mask uint8 [1, H, W])
static std::vector<std::tuple<Tensor, Tensor>> resize_depth(const std::vector<Tensor>& srcs, const std::vector<c10::optional<Tensor>>& masks,
                                                            int64_t W, int64_t H) {
  if (masks.size() != srcs.size()) throw py::value_error("resize_depth: one mask (or None) per source");
  if (W < 1 || H < 1 || W * H > (1 << 24)) throw py::value_error("resize_depth: 1 <= W, H, W H <= 2^24");
  std::vector<std::tuple<Tensor, Tensor>> out;
  if (srcs.empty()) return out;
  at::Device dev(at::kCPU);
  std::vector<Tensor> keep;
  for (size_t k0 = 0; k0 < srcs.size(); k0 += B3GS_DEPTH_PRIOR_MAX_VIEWS) {
    const int n = (int)std::min<size_t>(B3GS_DEPTH_PRIOR_MAX_VIEWS, srcs.size() - k0);
    std::vector<B3gsDepthResizeIO> io(n);
    for (int k = 0; k < n; k++) {
      Tensor s = dev_input(srcs[k0 + k], at::kFloat, "prior", NO_CPU_D, (k0 + k) ? &dev : nullptr);
      if (k0 + k == 0) dev = s.device();
      if (s.dim() != 2 || s.numel() < 1 || s.numel() > (1 << 24)) throw py::value_error("resize_depth: a prior is [Hsrc, Wsrc] with 1 <= Hsrc Wsrc <= 2^24");
      s = s.contiguous();
      B3gsDepthResizeIO& r = io[k];
      r.Hsrc = (int32_t)s.size(0), r.Wsrc = (int32_t)s.size(1), r.W = (int32_t)W, r.H = (int32_t)H;
      r.src = s.data_ptr<float>();
      r.src_mask = nullptr;
      if (masks[k0 + k].has_value()) {
        Tensor m = dev_input(*masks[k0 + k], at::kByte, "mask", NO_CPU_D, &dev).contiguous();
        if (m.dim() != 2 || m.size(0) != s.size(0) || m.size(1) != s.size(1)) throw py::value_error("resize_depth: a mask has the shape of its prior");
        r.src_mask = m.data_ptr<uint8_t>();
        keep.push_back(m);
      }
      Tensor p = at::empty({1, H, W}, s.options()), m = at::empty({1, H, W}, s.options().dtype(at::kByte));
      r.prior = p.data_ptr<float>(), r.mask = m.data_ptr<uint8_t>();
      keep.push_back(s);
      out.emplace_back(p, m);
    }
    DeviceGuard g(dev);
    check(b3gs_resize_depth_batch(n, io.data(), cur_stream(dev)), "b3gs_resize_depth_batch");
  }
  return out;
}

void bind_depthprior(py::module_& m) {
  m.def("depth_prior_workspace_bytes", &depth_prior_workspace_bytes, py::arg("W"), py::arg("H"), py::arg("patch"));
  m.def("depth_prior_loss", &depth_prior_loss, py::arg("views"), py::arg("mode"), py::arg("w_global"), py::arg("w_local"), py::arg("patch"),
        py::arg("min_valid"), py::arg("alpha_min"));
  m.def("resize_depth", &resize_depth, py::arg("srcs"), py::arg("masks"), py::arg("W"), py::arg("H"));
  m.attr("DEPTH_PRIOR_DEPTH") = B3GS_DEPTH_PRIOR_DEPTH;
  m.attr("DEPTH_PRIOR_DISPARITY") = B3GS_DEPTH_PRIOR_DISPARITY;
}

}  // namespace b3
