// Ground truth of dataset images (binocular3dgs_amd/ground_truth.py): launch assembly of b3gs_prepare_gt_batch -- resize as
// PIL does, / 255, alpha split, white-background composite, clamp, alpha multiply and the DTU background mask for up to 8
// uint8 sources per call.  No autograd, no host read, no synchronisation.
#include "common.h"

#include <tuple>
#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

static const Tensor* table_of(const std::vector<c10::optional<Tensor>>& tabs, int64_t i, int64_t out, bool needed, const char* axis) {
  const bool have = tabs[i].has_value() && tabs[i]->defined();
  if (have != needed)
    throw py::value_error(std::string("prepare_gt: a ") + axis + " table goes with every source whose size along it changes, and with no other");
  if (!have) return nullptr;
  const Tensor& t = *tabs[i];
  if (!t.is_cuda() || t.scalar_type() != at::kInt || !t.is_contiguous() || t.dim() != 2 || t.size(0) < 3 || t.size(1) != out)
    throw py::value_error(std::string("prepare_gt: the ") + axis + " table must be a contiguous int32 [2 + ksize, out] tensor on the device");
  return &t;
}

// sources: n uint8 tensors [Hs, Ws, C] (or [Hs, Ws]), C in {1, 3, 4}, on the device; tabs_x / tabs_y: per source None or the
// int32 table of that axis (ground_truth.resize_table); -> per source (original_image, gt_alpha_mask | None, bg_mask | None)
static std::vector<std::tuple<Tensor, c10::optional<Tensor>, c10::optional<Tensor>>> prepare_gt(
    const std::vector<Tensor>& sources, const std::vector<c10::optional<Tensor>>& tabs_x,
    const std::vector<c10::optional<Tensor>>& tabs_y, int64_t W, int64_t H, bool white_background, double dtu_threshold) {
  const int64_t n = (int64_t)sources.size();
  if (n < 1 || n > B3GS_MAX_GT_VIEWS) throw py::value_error("prepare_gt: 1..8 views per call");
  if ((int64_t)tabs_x.size() != n || (int64_t)tabs_y.size() != n) throw py::value_error("prepare_gt: one table entry per source and axis");
  if (W < 1 || H < 1) throw py::value_error("prepare_gt: the output size is at least 1 x 1");
  if (!(dtu_threshold >= 0.0)) throw py::value_error("prepare_gt: the DTU threshold is >= 0 (0: no mask)");
  const at::Device dev = sources[0].device();
  const auto f32 = at::TensorOptions().dtype(at::kFloat).device(dev);
  std::vector<Tensor> keep;
  keep.reserve(n);
  std::vector<B3gsGtView> tab(n);
  std::vector<std::tuple<Tensor, c10::optional<Tensor>, c10::optional<Tensor>>> out;
  out.reserve(n);
  for (int64_t i = 0; i < n; i++) {
    const Tensor& s = sources[i];
    if (!s.is_cuda() || s.device() != dev) raise("prepare_gt: source " + std::to_string(i) + " is on " + s.device().str() + ": ground truth is prepared on the HIP device only");
    if (s.scalar_type() != at::kByte || (s.dim() != 2 && s.dim() != 3))
      throw py::value_error("prepare_gt: a source is a uint8 [Hs, Ws, C] or [Hs, Ws] tensor");
    const int64_t C = s.dim() == 2 ? 1 : s.size(2);
    if (C != 1 && C != 3 && C != 4) throw py::value_error("prepare_gt: 1, 3 or 4 channels");
    Tensor c = s.is_contiguous() ? s : s.contiguous();
    if ((uintptr_t)c.data_ptr() & 15) c = c.clone();
    keep.push_back(c);
    B3gsGtView& g = tab[i];
    g.src = c.data_ptr<uint8_t>();
    g.Hs = (int32_t)s.size(0);
    g.Ws = (int32_t)s.size(1);
    g.C = (int32_t)C;
    const Tensor* tx = table_of(tabs_x, i, W, s.size(1) != W, "horizontal");
    const Tensor* ty = table_of(tabs_y, i, H, s.size(0) != H, "vertical");
    g.tab_x = tx ? tx->data_ptr<int32_t>() : nullptr;
    g.tab_y = ty ? ty->data_ptr<int32_t>() : nullptr;
    g.ks_x = tx ? (int32_t)tx->size(0) - 2 : 0;
    g.ks_y = ty ? (int32_t)ty->size(0) - 2 : 0;
    Tensor image = at::empty({C == 1 ? 1 : 3, H, W}, f32);
    c10::optional<Tensor> alpha, bg;
    if (C == 4) alpha = at::empty({1, H, W}, f32);
    if (dtu_threshold > 0.0) bg = at::empty({1, H, W}, f32);
    g.image = image.data_ptr<float>();
    g.alpha = alpha.has_value() ? alpha->data_ptr<float>() : nullptr;
    g.bg_mask = bg.has_value() ? bg->data_ptr<float>() : nullptr;
    out.emplace_back(image, alpha, bg);
  }
  const size_t ws_bytes = b3gs_gt_workspace_bytes((int32_t)n, tab.data(), (int32_t)H, (int32_t)W);
  Tensor ws = byte_workspace(ws_bytes, dev);
  {
    DeviceGuard g(dev);
    check(b3gs_prepare_gt_batch((int32_t)n, tab.data(), (int32_t)H, (int32_t)W, white_background ? 1 : 0, (float)dtu_threshold,
                                ws.data_ptr(), cur_stream(dev)),
          "b3gs_prepare_gt_batch");
  }
  return out;
}

void bind_gt_prep(py::module_& m) {
  m.def("prepare_gt", &prepare_gt, py::arg("sources"), py::arg("tabs_x"), py::arg("tabs_y"), py::arg("W"), py::arg("H"),
        py::arg("white_background") = false, py::arg("dtu_threshold") = 0.0);
  m.attr("MAX_GT_VIEWS") = B3GS_MAX_GT_VIEWS;
}

}  // namespace b3
