// Weighted k-means codebooks (binocular3dgs_amd/compress.py): launch assembly of b3gs_kmeans_assign / b3gs_kmeans.  No autograd:
// clustering is not differentiable.
#include "common.h"

#include <tuple>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* NO_CPU_K = "k-means runs on the HIP device only (tests/kmeans_ref.py holds the numpy statement)";

// x [N,D] and a codebook [K,D]: float32, contiguous, on one device, inside the library's limits
static void check_pair(const Tensor& x, const Tensor& cb) {
  if (x.dim() != 2 || cb.dim() != 2 || x.size(1) != cb.size(1)) throw py::value_error("kmeans: x is [N,D] and the codebook [K,D]");
  if (x.device() != cb.device()) raise("the codebook is on " + cb.device().str() + ", not on " + x.device().str());
  if (x.size(1) < 1 || x.size(1) > 64) throw py::value_error("kmeans: 1 <= D <= 64");
  if (cb.size(0) < 1 || cb.size(0) > 65536) throw py::value_error("kmeans: 1 <= K <= 65536");
  if (x.size(0) > INT32_MAX) throw py::value_error("kmeans: at most 2^31 - 1 rows");
}

static int64_t kmeans_workspace_bytes(int64_t N, int64_t D, int64_t K) {
  return (int64_t)b3gs_kmeans_workspace_bytes((int32_t)N, (int32_t)D, (int32_t)K);
}

// -> codes int32 [N]
static Tensor kmeans_assign(const Tensor& x, const Tensor& codebook) {
  if (!x.defined() || !x.is_cuda()) raise(std::string("x is on ") + (x.defined() ? x.device().str() : "no device") + ": " + NO_CPU_K);
  if (!codebook.defined() || !codebook.is_cuda()) raise(std::string("the codebook is on ") + (codebook.defined() ? codebook.device().str() : "no device") + ": " + NO_CPU_K);
  Tensor xs = dev_f32(x, "x", NO_CPU_K), cb = dev_f32(codebook, "codebook", NO_CPU_K);
  check_pair(xs, cb);
  const int64_t N = xs.size(0), D = xs.size(1), K = cb.size(0);
  const at::Device dev = xs.device();
  Tensor codes = at::empty({N}, at::TensorOptions().dtype(at::kInt).device(dev));
  if (N == 0) return codes;
  Tensor ws = byte_workspace(b3gs_kmeans_workspace_bytes((int32_t)N, (int32_t)D, (int32_t)K), dev);
  DeviceGuard g(dev);
  check(b3gs_kmeans_assign((int32_t)N, (int32_t)D, (int32_t)K, xs.data_ptr<float>(), cb.data_ptr<float>(), codes.data_ptr<int32_t>(),
                           ws.data_ptr(), cur_stream(dev)),
        "b3gs_kmeans_assign");
  return codes;
}

// x [N,D], weights [N] or None, init [K,D], iters -> (codebook float32 [K,D], codes int32 [N], counts int32 [K],
// distortion float64 [iters + 1]); `init` is not changed
static std::tuple<Tensor, Tensor, Tensor, Tensor> kmeans(const Tensor& x, const c10::optional<Tensor>& weights, const Tensor& init,
                                                         int64_t iters) {
  if (!x.defined() || !x.is_cuda()) raise(std::string("x is on ") + (x.defined() ? x.device().str() : "no device") + ": " + NO_CPU_K);
  if (!init.defined() || !init.is_cuda()) raise(std::string("init is on ") + (init.defined() ? init.device().str() : "no device") + ": " + NO_CPU_K);
  if (iters < 0 || iters > (1 << 20)) throw py::value_error("kmeans: iters must not be negative");
  Tensor xs = dev_f32(x, "x", NO_CPU_K);
  Tensor cb = dev_f32(init, "init", NO_CPU_K).clone();
  check_pair(xs, cb);
  const int64_t N = xs.size(0), D = xs.size(1), K = cb.size(0);
  if (N == 0) throw py::value_error("kmeans: no rows");
  const at::Device dev = xs.device();
  Tensor w;
  if (weights.has_value() && weights->defined()) {
    if (!weights->is_cuda() || weights->device() != dev) raise("weights is on " + weights->device().str() + ", not on " + dev.str());
    if (weights->numel() != N) throw py::value_error("kmeans: one weight per row");
    w = dev_f32(weights->reshape({N}), "weights", NO_CPU_K);
  }
  Tensor codes = at::empty({N}, at::TensorOptions().dtype(at::kInt).device(dev));
  Tensor counts = at::empty({K}, at::TensorOptions().dtype(at::kInt).device(dev));
  Tensor dist = at::empty({iters + 1}, at::TensorOptions().dtype(at::kDouble).device(dev));
  Tensor ws = byte_workspace(b3gs_kmeans_workspace_bytes((int32_t)N, (int32_t)D, (int32_t)K), dev);
  DeviceGuard g(dev);
  check(b3gs_kmeans((int32_t)N, (int32_t)D, (int32_t)K, (int32_t)iters, xs.data_ptr<float>(), w.defined() ? w.data_ptr<float>() : nullptr,
                    cb.data_ptr<float>(), codes.data_ptr<int32_t>(), counts.data_ptr<int32_t>(), dist.data_ptr<double>(), ws.data_ptr(),
                    cur_stream(dev)),
        "b3gs_kmeans");
  return std::make_tuple(cb, codes, counts, dist);
}

void bind_kmeans(py::module_& m) {
  m.def("kmeans_workspace_bytes", &kmeans_workspace_bytes, py::arg("N"), py::arg("D"), py::arg("K"));
  m.def("kmeans_assign", &kmeans_assign, py::arg("x"), py::arg("codebook"));
  m.def("kmeans", &kmeans, py::arg("x"), py::arg("weights"), py::arg("init"), py::arg("iters"));
}

}  // namespace b3
