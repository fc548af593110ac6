// The head of a view tuple of the calls that walk a finished forward's tile lists a second time (contrib.cpp, pixelmaps.cpp,
// segment.cpp, features.cpp): (geometry, binning, image, ... W, H) -- the three uint8 state buffers a FusedRasterizer forward left in a slot
// and the view's size.
#pragma once
#include "common.h"

#include <vector>

namespace b3 {

struct ViewState {
  const char *geometry, *binning, *image;
  int64_t W, H;
  at::Device dev;
};
// t[0..2]: the buffers, t[iw], t[iw + 1]: W and H; P: the model's Gaussian count (0 <= P <= INT32_MAX); dev: the device of the
// call, or NULL to take the geometry buffer's (-> ViewState::dev).  The tensors are pushed to `keep`, the scene is filled.
// fn names the call in a ValueError, no_cpu ends the B3gsError of a buffer that is not on the device.
inline ViewState view_state(const pybind11::tuple& t, size_t iw, int64_t P, const at::Device* dev, std::vector<at::Tensor>& keep,
                            B3gsScene& sc, const char* fn, const char* no_cpu) {
  at::Tensor geom = dev_input(t[0].cast<at::Tensor>(), at::kByte, "geometry", no_cpu, dev);
  const at::Device d = geom.device();
  at::Tensor binning = dev_input(t[1].cast<at::Tensor>(), at::kByte, "binning", no_cpu, &d);
  at::Tensor img = dev_input(t[2].cast<at::Tensor>(), at::kByte, "image", no_cpu, &d);
  const int64_t W = t[iw].cast<int64_t>(), H = t[iw + 1].cast<int64_t>();
  if (W <= 0 || H <= 0 || W > INT32_MAX || H > INT32_MAX) throw pybind11::value_error(std::string(fn) + ": W and H must be positive");
  if (geom.numel() < (int64_t)b3gs_geometry_bytes((int32_t)P) || img.numel() < (int64_t)b3gs_image_bytes((int32_t)W, (int32_t)H))
    throw pybind11::value_error(std::string(fn) + ": a state buffer is smaller than its P / W x H ask for");
  for (const at::Tensor& x : {geom, binning, img}) keep.push_back(x);
  sc = B3gsScene{};
  sc.P = (int32_t)P, sc.W = (int32_t)W, sc.H = (int32_t)H;
  return ViewState{(const char*)geom.data_ptr(), (const char*)binning.data_ptr(), (const char*)img.data_ptr(), W, H, d};
}

}  // namespace b3
