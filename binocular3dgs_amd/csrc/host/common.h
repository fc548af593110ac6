// Host-only C++ side of binocular3dgs_amd._C (g++ against the torch headers; no device code in this directory).
// Everything here calls libb3gs_raster.so through the C ABI of include/b3gs_raster.h -- the same boundary the reference's
// own binding would be given -- and keeps torch types OUT of that boundary.
#pragma once
#include <torch/extension.h>
#include <torch/csrc/Exceptions.h>
#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>

#include <string>

#include "../../../include/b3gs_raster.h"

namespace b3 {

// Raises binocular3dgs_amd._lib.B3gsError (a RuntimeError) -- from a pybind call or from inside an autograd node running on
// the engine's thread (python_error travels through the engine with its Python type intact).
[[noreturn]] void raise(const std::string& msg);
void check(int rc, const char* what);

inline b3gs_stream_t cur_stream(const at::Device& d) {
  return (b3gs_stream_t)c10::hip::getCurrentHIPStream(d.index()).stream();
}

// Switches the current device only when it is not `d` already (a launch through the C ABI uses the current device).
struct DeviceGuard {
  c10::DeviceIndex prev = -1;
  explicit DeviceGuard(const at::Device& d) {
    c10::DeviceIndex cur = c10::hip::current_device();
    if (d.has_index() && d.index() != cur) {
      prev = cur;
      c10::hip::set_device(d.index());
    }
  }
  ~DeviceGuard() {
    if (prev >= 0) c10::hip::set_device(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// A float32, contiguous tensor on the HIP device, or B3gsError (there is no CPU path).
inline at::Tensor dev_f32(const at::Tensor& t, const char* name, const char* what) {
  if (!t.is_cuda()) raise(std::string(name) + " is on " + t.device().str() + ": " + what);
  at::Tensor r = t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
  return r.is_contiguous() ? r : r.contiguous();
}
// A defined tensor of dtype `type` on the HIP device (and on `*dev`), as passed: NOT made contiguous -- a caller that reads
// it through a raw pointer says .contiguous(), one that writes it in place checks is_contiguous().  Device errors are
// B3gsError ("<name> is on cpu: <device_only_msg>"), a wrong dtype is a ValueError.
inline at::Tensor dev_input(const at::Tensor& t, at::ScalarType type, const char* name, const char* device_only_msg,
                            const at::Device* dev = nullptr) {
  if (!t.defined() || !t.is_cuda()) raise(std::string(name) + " is on " + (t.defined() ? t.device().str() : "no device") + ": " + device_only_msg);
  if (dev && t.device() != *dev) raise(std::string(name) + " is on " + t.device().str() + ", not on " + dev->str());
  if (t.scalar_type() != type) throw pybind11::value_error(std::string(name) + ": wrong dtype");
  return t;
}
// an uninitialised workspace of `bytes` bytes on `dev`
inline at::Tensor byte_workspace(size_t bytes, const at::Device& dev) {
  return at::empty({(int64_t)bytes}, at::TensorOptions().dtype(at::kByte).device(dev));
}
// the first n 64-bit words of a byte workspace as an int64 [n] view (the device-side totals of a count call)
inline at::Tensor head_words(const at::Tensor& ws, int n) { return ws.slice(0, 0, 8 * n).view(at::kLong); }
template <typename T>
inline T* ptr_or_null(const at::Tensor& t) { return t.numel() ? t.data_ptr<T>() : nullptr; }
inline const float* fptr(const at::Tensor& t) { return (t.defined() && t.numel()) ? t.data_ptr<float>() : nullptr; }
inline float* fptr_mut(at::Tensor& t) { return (t.defined() && t.numel()) ? t.data_ptr<float>() : nullptr; }

void bind_loss(pybind11::module_& m);
void bind_optim(pybind11::module_& m);
void bind_raster(pybind11::module_& m);
void bind_metrics(pybind11::module_& m);
void bind_frames(pybind11::module_& m);
void bind_gt_prep(pybind11::module_& m);
void bind_cloud(pybind11::module_& m);
void bind_sweep(pybind11::module_& m);
void bind_jpeg(pybind11::module_& m);
void bind_mesh(pybind11::module_& m);
void bind_meshtools(pybind11::module_& m);
void bind_simplify(pybind11::module_& m);
void bind_meshraster(pybind11::module_& m);
void bind_texture(pybind11::module_& m);
void bind_meshsmooth(pybind11::module_& m);
void bind_lpips(pybind11::module_& m);
void bind_contrib(pybind11::module_& m);
void bind_pixelmaps(pybind11::module_& m);
void bind_segment(pybind11::module_& m);
void bind_features(pybind11::module_& m);
void bind_kmeans(pybind11::module_& m);
void bind_undistort(pybind11::module_& m);
void bind_edit(pybind11::module_& m);
void bind_pose(pybind11::module_& m);
void bind_lod(pybind11::module_& m);
void bind_poisson(pybind11::module_& m);
void bind_mcmc(pybind11::module_& m);
void bind_depthprior(pybind11::module_& m);
void bind_exposure(pybind11::module_& m);
void bind_normalprior(pybind11::module_& m);

}  // namespace b3
