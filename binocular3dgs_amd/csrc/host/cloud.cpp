// The matcher cloud (binocular3dgs_amd/matcher_cloud.py): launch assembly of b3gs_triangulate_matches, b3gs_background_sheet
// and b3gs_cloud_grow_round.  No autograd, no host read, no synchronisation: counts stay device words.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kDeviceOnly = "the matcher cloud is built on the HIP device only";

static Tensor matrix(const Tensor& t, int64_t r, int64_t c, const char* name, const at::Device& dev) {
  Tensor m = dev_input(t, at::kFloat, name, kDeviceOnly, &dev).contiguous();
  if (m.dim() != 2 || m.size(0) != r || m.size(1) != c)
    throw py::value_error(std::string(name) + " is a float32 [" + std::to_string(r) + ", " + std::to_string(c) + "] matrix");
  return m;
}

static Tensor image_hwc3(const Tensor& t, const char* name, const at::Device* dev = nullptr) {
  Tensor im = dev_input(t, at::kByte, name, kDeviceOnly, dev).contiguous();
  if (im.dim() != 3 || im.size(2) != 3 || im.size(0) < 2 || im.size(1) < 2)
    throw py::value_error(std::string(name) + " is a uint8 [H, W, 3] image of at least 2 x 2 pixels");
  return im;
}

// -> (points [N,3] float32, colors [N,3] uint8, count int32 [1]); rows [0, count) are the kept matches in input order
static std::tuple<Tensor, Tensor, Tensor> triangulate_matches(const Tensor& proj_ref, const Tensor& proj_src, const Tensor& intrinsic,
                                                              const Tensor& w2c_ref, const Tensor& w2c_src, const Tensor& kp_ref,
                                                              const Tensor& kp_src, const Tensor& image, double reproj_threshold) {
  Tensor im = image_hwc3(image, "triangulate_matches: image");
  const at::Device dev = im.device();
  Tensor pr = matrix(proj_ref, 3, 4, "proj_ref", dev), ps = matrix(proj_src, 3, 4, "proj_src", dev);
  Tensor k = matrix(intrinsic, 3, 3, "intrinsic", dev);
  Tensor wr = matrix(w2c_ref, 4, 4, "w2c_ref", dev), wsrc = matrix(w2c_src, 4, 4, "w2c_src", dev);
  Tensor a = dev_input(kp_ref, at::kFloat, "kp_ref", kDeviceOnly, &dev).contiguous();
  Tensor b = dev_input(kp_src, at::kFloat, "kp_src", kDeviceOnly, &dev).contiguous();
  if (a.dim() != 2 || a.size(1) != 2 || b.dim() != 2 || b.size(1) != 2 || a.size(0) != b.size(0))
    throw py::value_error("triangulate_matches: kp_ref and kp_src are float32 [N, 2] with the same N");
  const int64_t N = a.size(0);
  Tensor points = at::empty({N, 3}, a.options());
  Tensor colors = at::empty({N, 3}, im.options());
  Tensor count = at::empty({1}, a.options().dtype(at::kInt));
  Tensor ws = byte_workspace(b3gs_cloud_workspace_bytes(N), dev);
  {
    DeviceGuard g(dev);
    check(b3gs_triangulate_matches((int32_t)N, fptr(pr), fptr(ps), fptr(k), fptr(wr), fptr(wsrc), fptr(a), fptr(b),
                                   im.data_ptr<uint8_t>(), (int32_t)im.size(1), (int32_t)im.size(0), (float)reproj_threshold,
                                   ptr_or_null<float>(points), ptr_or_null<uint8_t>(colors),
                                   count.data_ptr<int32_t>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_triangulate_matches");
  }
  return {points, colors, count};
}

static std::tuple<Tensor, Tensor, Tensor> background_sheet(const Tensor& image, const Tensor& inv_intrinsic_t, const Tensor& c2w,
                                                           double depth) {
  Tensor im = image_hwc3(image, "background_sheet: image");
  const at::Device dev = im.device();
  Tensor ik = matrix(inv_intrinsic_t, 3, 3, "inv_intrinsic_t", dev), e = matrix(c2w, 4, 4, "c2w", dev);
  const int64_t n = im.size(0) * im.size(1);
  Tensor points = at::empty({n, 3}, ik.options());
  Tensor colors = at::empty({n, 3}, im.options());
  Tensor count = at::empty({1}, ik.options().dtype(at::kInt));
  Tensor ws = byte_workspace(b3gs_cloud_workspace_bytes(n), dev);
  {
    DeviceGuard g(dev);
    check(b3gs_background_sheet(im.data_ptr<uint8_t>(), (int32_t)im.size(1), (int32_t)im.size(0), fptr(ik), fptr(e), (float)depth,
                                points.data_ptr<float>(), colors.data_ptr<uint8_t>(), count.data_ptr<int32_t>(), ws.data_ptr(),
                                cur_stream(dev)),
          "b3gs_background_sheet");
  }
  return {points, colors, count};
}

// One round, in place: points / colors [capacity, 3] float32, length / overflow int32 [1], grids int32 [n_views, H + 2, W + 2].
static void cloud_grow_round(const Tensor& images, const Tensor& w2c, const Tensor& window, const Tensor& seed_idx, const Tensor& noise,
                             Tensor points, Tensor colors, Tensor length, Tensor overflow, Tensor grids, int64_t ref, int64_t src,
                             int64_t n_start, int64_t h_patch_size, bool init, double fx, double fy, double cx, double cy,
                             double alpha, double ssim_threshold, const c10::optional<Tensor>& debug_ssim,
                             const c10::optional<Tensor>& debug_mask) {
  Tensor im = dev_input(images, at::kByte, "cloud_grow_round: images", kDeviceOnly).contiguous();
  const at::Device dev = im.device();
  if (im.dim() != 4 || im.size(3) != 3) throw py::value_error("cloud_grow_round: images is uint8 [n_views, H, W, 3]");
  const int64_t V = im.size(0), H = im.size(1), W = im.size(2);
  Tensor m = dev_input(w2c, at::kFloat, "w2c", kDeviceOnly, &dev).contiguous(), win = dev_input(window, at::kFloat, "window", kDeviceOnly, &dev).contiguous();
  Tensor si = dev_input(seed_idx, at::kInt, "seed_idx", kDeviceOnly, &dev).contiguous();
  Tensor nz = dev_input(noise, at::kFloat, "noise", kDeviceOnly, &dev).contiguous();
  if (m.dim() != 3 || m.size(0) != V || m.size(1) != 4 || m.size(2) != 4) throw py::value_error("cloud_grow_round: w2c is float32 [n_views, 4, 4]");
  if (h_patch_size != 5) raise("cloud_grow_round: h_patch_size=5 (an 11x11 window) is the only supported patch");
  if (win.numel() != 121) throw py::value_error("cloud_grow_round: window holds 121 weights");
  if (nz.dim() != 3 || nz.size(2) != 3 || si.dim() != 1 || si.size(0) != nz.size(0))
    throw py::value_error("cloud_grow_round: noise is float32 [n_seeds, n_samples, 3] and seed_idx int32 [n_seeds]");
  for (const Tensor* t : {&points, &colors})
    if (!t->is_cuda() || t->device() != dev || t->scalar_type() != at::kFloat || !t->is_contiguous() || t->dim() != 2 || t->size(1) != 3 ||
        t->size(0) != points.size(0))
      raise(std::string("cloud_grow_round: points and colors are contiguous float32 [capacity, 3] tensors; ") + kDeviceOnly);
  for (const Tensor* t : {&length, &overflow})
    if (!t->is_cuda() || t->device() != dev || t->scalar_type() != at::kInt || t->numel() != 1)
      raise(std::string("cloud_grow_round: length and overflow are int32 words; ") + kDeviceOnly);
  if (!grids.is_cuda() || grids.device() != dev || grids.scalar_type() != at::kInt || !grids.is_contiguous() ||
      grids.numel() != V * (H + 2) * (W + 2))
    raise(std::string("cloud_grow_round: grids is a contiguous int32 [n_views, H + 2, W + 2] tensor; ") + kDeviceOnly);
  const int64_t ncand = nz.size(0) * nz.size(1);
  Tensor dbg_s, dbg_m;
  if (debug_ssim.has_value() && debug_ssim->defined()) {
    dbg_s = *debug_ssim;
    if (!dbg_s.is_cuda() || dbg_s.scalar_type() != at::kFloat || !dbg_s.is_contiguous() || dbg_s.numel() != ncand)
      throw py::value_error("cloud_grow_round: debug_ssim is a contiguous float32 [candidates] tensor on the device");
  }
  if (debug_mask.has_value() && debug_mask->defined()) {
    dbg_m = *debug_mask;
    if (!dbg_m.is_cuda() || dbg_m.scalar_type() != at::kByte || !dbg_m.is_contiguous() || dbg_m.numel() != ncand)
      throw py::value_error("cloud_grow_round: debug_mask is a contiguous uint8 [candidates] tensor on the device");
  }
  Tensor ws = byte_workspace(b3gs_cloud_workspace_bytes(ncand), dev);
  B3gsCloudGrow io = {};
  io.W = (int32_t)W;
  io.H = (int32_t)H;
  io.n_views = (int32_t)V;
  io.ref = (int32_t)ref;
  io.src = (int32_t)src;
  io.n_seeds = (int32_t)nz.size(0);
  io.n_samples = (int32_t)nz.size(1);
  io.n_start = (int32_t)n_start;
  io.h_patch_size = (int32_t)h_patch_size;
  io.init = init ? 1 : 0;
  io.fx = (float)fx;
  io.fy = (float)fy;
  io.cx = (float)cx;
  io.cy = (float)cy;
  io.alpha = (float)alpha;
  io.ssim_threshold = (float)ssim_threshold;
  io.images = im.data_ptr<uint8_t>();
  io.w2c = fptr(m);
  io.window = fptr(win);
  io.seed_idx = si.data_ptr<int32_t>();
  io.noise = fptr(nz);
  io.points = points.data_ptr<float>();
  io.colors = colors.data_ptr<float>();
  io.capacity = (int32_t)points.size(0);
  io.length = length.data_ptr<int32_t>();
  io.overflow = overflow.data_ptr<int32_t>();
  io.grids = grids.data_ptr<int32_t>();
  io.workspace = ws.data_ptr();
  io.debug_ssim = dbg_s.defined() ? dbg_s.data_ptr<float>() : nullptr;
  io.debug_mask = dbg_m.defined() ? dbg_m.data_ptr<uint8_t>() : nullptr;
  {
    DeviceGuard g(dev);
    check(b3gs_cloud_grow_round(&io, cur_stream(dev)), "b3gs_cloud_grow_round");
  }
}

void bind_cloud(py::module_& m) {
  m.def("triangulate_matches", &triangulate_matches, py::arg("proj_ref"), py::arg("proj_src"), py::arg("intrinsic"), py::arg("w2c_ref"),
        py::arg("w2c_src"), py::arg("kp_ref"), py::arg("kp_src"), py::arg("image"), py::arg("reproj_threshold") = 2.0);
  m.def("background_sheet", &background_sheet, py::arg("image"), py::arg("inv_intrinsic_t"), py::arg("c2w"), py::arg("depth") = 10.0);
  m.def("cloud_grow_round", &cloud_grow_round, py::arg("images"), py::arg("w2c"), py::arg("window"), py::arg("seed_idx"), py::arg("noise"),
        py::arg("points"), py::arg("colors"), py::arg("length"), py::arg("overflow"), py::arg("grids"), py::arg("ref"), py::arg("src"),
        py::arg("n_start"), py::arg("h_patch_size") = 5, py::arg("init") = false, py::arg("fx"), py::arg("fy"), py::arg("cx"),
        py::arg("cy"), py::arg("alpha") = 10.0, py::arg("ssim_threshold") = 0.95, py::arg("debug_ssim") = py::none(),
        py::arg("debug_mask") = py::none());
  m.def("cloud_workspace_bytes", [](int64_t n) { return b3gs_cloud_workspace_bytes(n); });
  m.attr("CLOUD_MAX_VIEWS") = B3GS_CLOUD_MAX_VIEWS;
}

}  // namespace b3
