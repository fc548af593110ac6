// Merging Gaussians into levels of detail (binocular3dgs_amd/lod.py): launch assembly of the calls of csrc/lod.hip.  Nothing
// here reads the device or synchronises: the totals of the count call stay device words, which the caller reads once, between
// count and emit, and hands back to emit.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const char* kLodDeviceOnly = "Gaussians are merged on the HIP device only (tests/lod_ref.py holds the numpy statement)";
constexpr int kMergeWords = 7;        // the int64 words count leaves at the head of the workspace

struct MergeInputs {
  Tensor pos, scale, quat, alpha, dc, rest, weight;
  at::Device dev = at::Device(at::kCPU);
  int64_t P = 0, K = 0;
  const double* wptr = nullptr;
};

static Tensor merge_rows(const Tensor& t, int64_t P, int64_t cols, const char* name, const at::Device* dev) {
  Tensor r = dev_input(t, at::kFloat, name, kLodDeviceOnly, dev);
  if (r.dim() < 1 || r.size(0) != P || r.numel() != P * cols) throw py::value_error(std::string(name) + ": wrong shape");
  return r.contiguous();
}

static MergeInputs merge_inputs(const Tensor& positions, const Tensor& scales, const Tensor& quaternions, const Tensor& opacities,
                                const Tensor& features_dc, const Tensor& features_rest, const c10::optional<Tensor>& weights, double cell) {
  MergeInputs in;
  Tensor p = dev_input(positions, at::kFloat, "positions", kLodDeviceOnly);
  if (p.dim() != 2 || p.size(1) != 3) throw py::value_error("positions is [P, 3]");
  in.dev = p.device();
  in.P = p.size(0);
  if (in.P >= (1 << 24)) throw py::value_error("gaussian_merge: P < 2^24");
  if (!((float)cell > 0.f) || !std::isfinite((float)cell)) throw py::value_error("gaussian_merge: the cell is positive and finite");
  in.pos = p.contiguous();
  in.scale = merge_rows(scales, in.P, 3, "scales", &in.dev);
  in.quat = merge_rows(quaternions, in.P, 4, "quaternions", &in.dev);
  in.alpha = merge_rows(opacities, in.P, 1, "opacities", &in.dev);
  in.dc = merge_rows(features_dc, in.P, 3, "features_dc", &in.dev);
  Tensor fr = dev_input(features_rest, at::kFloat, "features_rest", kLodDeviceOnly, &in.dev);
  if (fr.dim() != 3 || fr.size(0) != in.P || fr.size(2) != 3) throw py::value_error("features_rest is [P, K, 3]");
  in.K = fr.size(1);
  if (in.K != 0 && in.K != 3 && in.K != 8 && in.K != 15) throw py::value_error("features_rest: K is 0, 3, 8 or 15");
  in.rest = fr.contiguous();
  if (weights.has_value()) {
    Tensor w = dev_input(*weights, at::kDouble, "weights", kLodDeviceOnly, &in.dev);
    if (w.dim() != 1 || w.size(0) != in.P) throw py::value_error("weights is float64 [P]");
    in.weight = w.contiguous();
    in.wptr = in.P ? in.weight.data_ptr<double>() : nullptr;
  }
  return in;
}

// -> (workspace, totals): int64 [7] on the device (include/b3gs_raster.h lists the words)
static std::tuple<Tensor, Tensor> gaussian_merge_count(const Tensor& positions, const Tensor& scales, const Tensor& quaternions,
                                                       const Tensor& opacities, const Tensor& features_dc, const Tensor& features_rest,
                                                       const c10::optional<Tensor>& weights, double cell) {
  MergeInputs in = merge_inputs(positions, scales, quaternions, opacities, features_dc, features_rest, weights, cell);
  Tensor ws = byte_workspace(b3gs_gaussian_merge_workspace_bytes(in.P, (int32_t)in.K), in.dev);
  DeviceGuard guard(in.dev);
  check(b3gs_gaussian_merge_count((int32_t)in.P, (int32_t)in.K, ptr_or_null<float>(in.pos), ptr_or_null<float>(in.scale),
                                  ptr_or_null<float>(in.quat), ptr_or_null<float>(in.alpha), ptr_or_null<float>(in.dc),
                                  ptr_or_null<float>(in.rest), in.wptr, (float)cell, ws.data_ptr(), cur_stream(in.dev)),
        "b3gs_gaussian_merge_count");
  return {ws, head_words(ws, kMergeWords)};
}

// totals: the first five words the caller read -> (positions, scales, quaternions, opacities, features_dc, features_rest,
// cluster_of int32 [P], members int32 [rows])
static std::vector<Tensor> gaussian_merge_emit(const Tensor& positions, const Tensor& scales, const Tensor& quaternions, const Tensor& opacities,
                                               const Tensor& features_dc, const Tensor& features_rest, const c10::optional<Tensor>& weights,
                                               double cell, const Tensor& ws, const std::vector<int64_t>& totals) {
  MergeInputs in = merge_inputs(positions, scales, quaternions, opacities, features_dc, features_rest, weights, cell);
  Tensor w = dev_input(ws, at::kByte, "workspace", kLodDeviceOnly, &in.dev).contiguous();
  if ((size_t)w.numel() < b3gs_gaussian_merge_workspace_bytes(in.P, (int32_t)in.K)) throw py::value_error("gaussian_merge: the workspace is too small");
  if (totals.size() != 5) throw py::value_error("gaussian_merge: totals are the first five words of the count call");
  const bool failed = totals[3] != 0 || totals[4] != 0;
  int64_t rows = failed ? 0 : totals[0] + totals[1];
  if (rows < 0 || rows > in.P) throw py::value_error("gaussian_merge: bad totals");
  auto f32 = at::TensorOptions().device(in.dev).dtype(at::kFloat), i32 = at::TensorOptions().device(in.dev).dtype(at::kInt);
  Tensor op = at::empty({rows, 3}, f32), os = at::empty({rows, 3}, f32), oq = at::empty({rows, 4}, f32), oa = at::empty({rows}, f32);
  Tensor od = at::empty({rows, 1, 3}, f32), orr = at::empty({rows, in.K, 3}, f32);
  Tensor cluster_of = at::empty({failed ? 0 : in.P}, i32), members = at::empty({rows}, i32);
  DeviceGuard guard(in.dev);
  check(b3gs_gaussian_merge_emit((int32_t)in.P, (int32_t)in.K, ptr_or_null<float>(in.pos), ptr_or_null<float>(in.scale),
                                 ptr_or_null<float>(in.quat), ptr_or_null<float>(in.alpha), ptr_or_null<float>(in.dc),
                                 ptr_or_null<float>(in.rest), in.wptr, (float)cell, w.data_ptr(), totals.data(), ptr_or_null<float>(op),
                                 ptr_or_null<float>(os), ptr_or_null<float>(oq), ptr_or_null<float>(oa), ptr_or_null<float>(od),
                                 ptr_or_null<float>(orr), ptr_or_null<int32_t>(cluster_of), ptr_or_null<int32_t>(members), cur_stream(in.dev)),
        "b3gs_gaussian_merge_emit");
  return {op, os, oq, oa, od, orr, cluster_of, members};
}

void bind_lod(py::module_& m) {
  m.def("gaussian_merge_count", &gaussian_merge_count, py::arg("positions"), py::arg("scales"), py::arg("quaternions"), py::arg("opacities"),
        py::arg("features_dc"), py::arg("features_rest"), py::arg("weights"), py::arg("cell"));
  m.def("gaussian_merge_emit", &gaussian_merge_emit, py::arg("positions"), py::arg("scales"), py::arg("quaternions"), py::arg("opacities"),
        py::arg("features_dc"), py::arg("features_rest"), py::arg("weights"), py::arg("cell"), py::arg("workspace"), py::arg("totals"));
  m.attr("MERGE_JACOBI_SWEEPS") = B3GS_MERGE_JACOBI_SWEEPS;
}

}  // namespace b3
