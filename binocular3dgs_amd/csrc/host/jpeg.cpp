// Baseline JPEG of rendered frames (binocular3dgs_amd/frames.py): launch assembly of b3gs_jpeg_encode_batch -- the
// entropy-coded scans of up to 8 uint8 [H,W,3] device images of one W x H per call.  No autograd, no host read.
#include "common.h"

#include <vector>

namespace py = pybind11;
using at::Tensor;

namespace b3 {

// images: n uint8 [H,W,3] tensors on the device; qtables: int16 [2,64] on the device (luminance, chrominance; row-major);
// out: uint8, at least n * capacity elements, frame i written at i * capacity; lengths: int64, at least n elements
static void jpeg_encode(const std::vector<Tensor>& images, const Tensor& qtables, Tensor out, int64_t capacity, Tensor lengths) {
  const int64_t n = (int64_t)images.size();
  if (n < 1 || n > B3GS_MAX_FRAME_VIEWS) throw py::value_error("jpeg_encode: 1..8 images per call");
  const Tensor& i0 = images[0];
  if (i0.dim() != 3 || i0.size(2) != 3) throw py::value_error("jpeg_encode expects uint8 [H,W,3] images");
  const int64_t H = i0.size(0), W = i0.size(1);
  if (H < 1 || H > 65535 || W < 1 || W > 65535) throw py::value_error("jpeg_encode: 1..65535 pixels per side");
  if (capacity < 1) throw py::value_error("jpeg_encode: capacity must be at least 1");
  const at::Device dev = i0.device();
  std::vector<Tensor> keep;
  std::vector<const uint8_t*> ptrs(n);
  keep.reserve(n);
  for (int64_t i = 0; i < n; i++) {
    const Tensor& t = images[i];
    if (!t.is_cuda()) raise("image is on " + t.device().str() + ": JPEG frames are encoded on the HIP device only");
    if (t.scalar_type() != at::kByte || t.sizes() != i0.sizes() || t.device() != dev)
      throw py::value_error("jpeg_encode: every image of one call is uint8 [H,W,3] of the same size on one device");
    keep.push_back(t.is_contiguous() ? t : t.contiguous());
    ptrs[i] = keep.back().data_ptr<uint8_t>();
  }
  if (!qtables.is_cuda() || qtables.scalar_type() != at::kShort || !qtables.is_contiguous() || qtables.numel() != 128)
    throw py::value_error("jpeg_encode: qtables must be a contiguous int16 [2,64] tensor on the device");
  if (!out.is_cuda() || out.scalar_type() != at::kByte || !out.is_contiguous() || out.numel() < n * capacity)
    throw py::value_error("jpeg_encode: out must be a contiguous uint8 tensor of n * capacity bytes on the device");
  if (!lengths.is_cuda() || lengths.scalar_type() != at::kLong || !lengths.is_contiguous() || lengths.numel() < n)
    throw py::value_error("jpeg_encode: lengths must be a contiguous int64 tensor of n elements on the device");
  const size_t ws_bytes = b3gs_jpeg_workspace_bytes((int32_t)n, (int32_t)H, (int32_t)W);
  Tensor ws = byte_workspace(ws_bytes, dev);
  {
    DeviceGuard g(dev);
    check(b3gs_jpeg_encode_batch((int32_t)n, ptrs.data(), (int32_t)H, (int32_t)W,
                                 reinterpret_cast<const uint16_t*>(qtables.data_ptr<int16_t>()), out.data_ptr<uint8_t>(), capacity,
                                 lengths.data_ptr<int64_t>(), ws.data_ptr(), cur_stream(dev)),
          "b3gs_jpeg_encode_batch");
  }
}

void bind_jpeg(py::module_& m) {
  m.def("jpeg_encode", &jpeg_encode, py::arg("images"), py::arg("qtables"), py::arg("out"), py::arg("capacity"), py::arg("lengths"));
  m.def("jpeg_workspace_bytes", [](int n, int H, int W) { return b3gs_jpeg_workspace_bytes(n, H, W); });
}

}  // namespace b3
