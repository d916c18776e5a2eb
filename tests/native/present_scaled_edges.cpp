// present_scaled_edges — rt_resample_rgba8 (rt_host.cpp) at the sizes where its clamped taps touch
// the image's first and last texels, for a build with the host sanitizers
// (tests/test_present_scaled_cpu.py compiles this file together with rt_host.cpp and runs it as a
// child process; it is never loaded into Python and never touches the GPU).
//
// Image and output are heap buffers of exactly width * rows * 4 floats and out_width * out_rows * 4
// bytes, so a tap or a store one element outside either is reported.  Float k of an image is
// ((37 k + 11) % 257 - 1) / 255, +inf where k % 13 == 5 and NaN where k % 17 == 3 (the floats whose
// cast to an integer type would be undefined).  Prints, per case and row order, one line
//   W R out_w out_h top_down: <the output bytes in hex>
// Exit 0 = ran clean.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>

#include "rt/abi.h"

int main() {
  const int cases[4][4] = {{1, 1, 5, 3}, {7, 5, 1, 1}, {3, 2, 16, 16}, {5, 1, 1, 7}};  // W, R, out_w, out_h
  for (const auto& c : cases) {
    const int W = c[0], R = c[1], ow = c[2], oh = c[3];
    const size_t nf = (size_t)W * R * 4, nb = (size_t)ow * oh * 4;
    std::unique_ptr<float[]> img(new float[nf]);
    for (size_t k = 0; k < nf; ++k) {
      img[k] = (float)((int)((37 * k + 11) % 257) - 1) / 255.0f;
      if (k % 13 == 5) img[k] = std::numeric_limits<float>::infinity();
      if (k % 17 == 3) img[k] = std::numeric_limits<float>::quiet_NaN();
    }
    for (int top_down = 0; top_down < 2; ++top_down) {
      std::unique_ptr<uint8_t[]> out(new uint8_t[nb]);
      if (rt_resample_rgba8(img.get(), W, R, ow, oh, top_down, out.get()) != RT_OK) return 3;
      std::printf("%d %d %d %d %d:", W, R, ow, oh, top_down);
      for (size_t k = 0; k < nb; ++k) std::printf(" %02x", out[k]);
      std::printf("\n");
    }
  }
  float one[4] = {0.5f, 0.5f, 0.5f, 1.0f};
  uint8_t px[4];
  if (rt_resample_rgba8(nullptr, 1, 1, 1, 1, 0, px) != RT_E_INVAL) return 4;
  if (rt_resample_rgba8(one, 1, 1, 1, 1, 0, nullptr) != RT_E_INVAL) return 5;
  if (rt_resample_rgba8(one, 0, 1, 1, 1, 0, px) != RT_E_INVAL) return 6;
  if (rt_resample_rgba8(one, 1, 1, 1, RT_PRESENT_SCALED_MAX + 1, 0, px) != RT_E_INVAL) return 7;
  if (rt_resample_rgba8(one, 1, 1, 1, 1, 0, px) != RT_OK || px[0] != 128 || px[3] != 255) return 8;
  return 0;
}
