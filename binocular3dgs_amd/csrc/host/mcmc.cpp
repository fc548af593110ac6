// Fixed-budget training (binocular3dgs_amd/mcmc.py): launch assembly of b3gs_mcmc_random, b3gs_mcmc_noise and
// b3gs_mcmc_relocate.  No autograd, no host read, no synchronisation.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_M = "the MCMC strategy runs on the HIP device only (tests/mcmc_ref.py holds the numpy statement)";

static Tensor rows_in_place(const Tensor& t, int64_t P, int64_t cols, const char* name, const at::Device* dev = nullptr) {
  Tensor r = dev_input(t, at::kFloat, name, NO_CPU_M, dev);
  if (r.dim() < 1 || r.numel() != P * cols) throw py::value_error(std::string(name) + ": wrong shape");   // (flat moment views pass)
  if (!r.is_contiguous()) throw py::value_error(std::string(name) + " is contiguous");
  return r;
}

// -> uint32 words as int32 [n] (kind 0) or float32 [n] (kind 1)
static Tensor mcmc_random(int64_t n, uint64_t seed, int64_t stream_id, int64_t offset, int64_t kind, const at::Device& dev) {
  if (!dev.is_cuda()) raise(std::string("mcmc_random: ") + NO_CPU_M);
  if (n < 0 || n > ((int64_t)1 << 32)) throw py::value_error("mcmc_random: 0 <= n <= 2^32");
  if (stream_id < 0 || stream_id > UINT32_MAX || offset < 0 || offset > UINT32_MAX) throw py::value_error("mcmc_random: stream_id and offset are 32-bit words");
  if (kind != B3GS_RANDOM_U32 && kind != B3GS_RANDOM_NORMAL) throw py::value_error("mcmc_random: kind is 0 (uint32) or 1 (normal)");
  Tensor out = at::empty({n}, at::TensorOptions().dtype(kind == B3GS_RANDOM_NORMAL ? at::kFloat : at::kInt).device(dev));
  DeviceGuard g(dev);
  check(b3gs_mcmc_random(n, seed, (uint32_t)stream_id, (uint32_t)offset, (int32_t)kind, n ? out.data_ptr() : nullptr, cur_stream(dev)), "b3gs_mcmc_random");
  return out;
}

// xyz [P,3] is written in place.  normals: None or float32 [P,3]; lr_dev: None or one float32 on the device
static void mcmc_noise(Tensor xyz, const Tensor& scaling, const Tensor& rotation, const Tensor& opacity, const c10::optional<Tensor>& normals,
                       uint64_t seed, int64_t iteration, double noise_lr, double lr_xyz, const c10::optional<Tensor>& lr_dev) {
  Tensor x = dev_input(xyz, at::kFloat, "xyz", NO_CPU_M);
  const at::Device dev = x.device();
  const int64_t P = x.dim() ? x.size(0) : 0;
  if (P > INT32_MAX) throw py::value_error("mcmc_noise: more than 2^31 - 1 Gaussians");
  x = rows_in_place(x, P, 3, "xyz");
  Tensor s = rows_in_place(scaling, P, 3, "scaling", &dev), r = rows_in_place(rotation, P, 4, "rotation", &dev);
  Tensor o = rows_in_place(opacity, P, 1, "opacity", &dev);
  if (iteration < 0 || iteration > UINT32_MAX) throw py::value_error("mcmc_noise: the iteration is a 32-bit word");
  Tensor n, l;
  if (normals.has_value()) n = rows_in_place(*normals, P, 3, "normals", &dev);
  if (lr_dev.has_value()) {
    l = dev_input(*lr_dev, at::kFloat, "lr_xyz", NO_CPU_M, &dev);
    if (l.numel() != 1) throw py::value_error("mcmc_noise: lr_xyz on the device is ONE float32");
  }
  DeviceGuard g(dev);
  check(b3gs_mcmc_noise((int32_t)P, ptr_or_null<float>(s), ptr_or_null<float>(r), ptr_or_null<float>(o), ptr_or_null<float>(x),
                        n.defined() ? ptr_or_null<float>(n) : nullptr, seed, (uint32_t)iteration, (float)noise_lr, (float)lr_xyz,
                        l.defined() ? l.data_ptr<float>() : nullptr, cur_stream(dev)),
        "b3gs_mcmc_noise");
}

// params: the six raw tensors in model order (xyz, features_dc, features_rest, scaling, rotation, opacity), written in place;
// exp_avg / exp_avg_sq: six tensors each, or empty lists.  draws: None or int64 [P] (the bits of uint64 draws, by dead rank).
// -> None, or with debug (src int32 [P], count int32 [P], rank int32 [P], weight scan int64 [P], head int64 [3]) as COPIES.
static py::object mcmc_relocate(std::vector<Tensor> params, std::vector<Tensor> exp_avg, std::vector<Tensor> exp_avg_sq, int64_t P_old,
                                double min_opacity, int64_t n_max, uint64_t seed, int64_t offset, const c10::optional<Tensor>& draws, bool debug) {
  if (params.size() != 6) throw py::value_error("mcmc_relocate: six parameter tensors");
  if (!(exp_avg.empty() && exp_avg_sq.empty()) && !(exp_avg.size() == 6 && exp_avg_sq.size() == 6))
    throw py::value_error("mcmc_relocate: six tensors of each Adam moment, or none");
  Tensor x = dev_input(params[0], at::kFloat, "xyz", NO_CPU_M);
  const at::Device dev = x.device();
  const int64_t P = x.dim() ? x.size(0) : 0;
  if (P > INT32_MAX) throw py::value_error("mcmc_relocate: more than 2^31 - 1 Gaussians");
  const int64_t K = P ? params[2].numel() / P : 0;
  const int64_t cols[6] = {3, 3, K, 3, 4, 1};
  static const char* names[6] = {"xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"};
  if (offset < 0 || offset > UINT32_MAX) throw py::value_error("mcmc_relocate: the offset is a 32-bit word");
  B3gsMcmcIO io = {};
  io.P = (int32_t)P, io.P_old = (int32_t)P_old, io.K = (int32_t)K, io.n_max = (int32_t)n_max, io.min_opacity = (float)min_opacity;
  io.offset = (uint32_t)offset, io.seed = seed;
  if (P_old < 0 || P_old > P) throw py::value_error("mcmc_relocate: 0 <= P_old <= P");
  for (int t = 0; t < 6; t++) {
    Tensor p = rows_in_place(params[t], P, cols[t], names[t], &dev);
    io.param[t] = ptr_or_null<float>(p);
    if (!exp_avg.empty()) {
      Tensor m = rows_in_place(exp_avg[t], P, cols[t], "exp_avg", &dev), v = rows_in_place(exp_avg_sq[t], P, cols[t], "exp_avg_sq", &dev);
      io.exp_avg[t] = ptr_or_null<float>(m), io.exp_avg_sq[t] = ptr_or_null<float>(v);
    }
  }
  Tensor d;
  if (draws.has_value()) {
    d = dev_input(*draws, at::kLong, "draws", NO_CPU_M, &dev);
    if (d.dim() != 1 || d.size(0) != P || !d.is_contiguous()) throw py::value_error("mcmc_relocate: draws are a contiguous int64 [P]");
    io.draws = P ? reinterpret_cast<const uint64_t*>(d.data_ptr<int64_t>()) : nullptr;
  }
  if (P == 0) return py::none();
  Tensor ws = byte_workspace(b3gs_mcmc_workspace_bytes((int32_t)P), dev);
  DeviceGuard g(dev);
  check(b3gs_mcmc_relocate(&io, ws.data_ptr(), cur_stream(dev)), "b3gs_mcmc_relocate");
  if (!debug) return py::none();
  B3gsMcmcViews v = {};
  check(b3gs_mcmc_views((int32_t)P, ws.data_ptr(), &v), "b3gs_mcmc_views");
  const char* base = static_cast<const char*>(ws.data_ptr());
  auto view = [&](const void* p, int64_t bytes, at::ScalarType type) {
    const int64_t at0 = static_cast<const char*>(p) - base;
    return ws.slice(0, at0, at0 + bytes).view(type).clone();
  };
  return py::make_tuple(view(v.src, 4 * P, at::kInt), view(v.count, 4 * P, at::kInt), view(v.rank, 4 * P, at::kInt),
                        view(v.weight_scan, 8 * P, at::kLong), view(v.head, 24, at::kLong));
}

void bind_mcmc(py::module_& m) {
  m.def("mcmc_random", &mcmc_random, py::arg("n"), py::arg("seed"), py::arg("stream_id"), py::arg("offset"), py::arg("kind"), py::arg("device"));
  m.def("mcmc_noise", &mcmc_noise, py::arg("xyz"), py::arg("scaling"), py::arg("rotation"), py::arg("opacity"), py::arg("normals"),
        py::arg("seed"), py::arg("iteration"), py::arg("noise_lr"), py::arg("lr_xyz"), py::arg("lr_dev"));
  m.def("mcmc_relocate", &mcmc_relocate, py::arg("params"), py::arg("exp_avg"), py::arg("exp_avg_sq"), py::arg("P_old"), py::arg("min_opacity"),
        py::arg("n_max"), py::arg("seed"), py::arg("offset"), py::arg("draws"), py::arg("debug"));
  m.attr("MCMC_MAX_N") = B3GS_MCMC_MAX_N;
}

}  // namespace b3
