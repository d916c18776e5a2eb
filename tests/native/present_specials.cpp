// present_specials — rt_quantize_rgba8 (rt_host.cpp) on floats given as bit patterns, for a build
// with the host sanitizers (tests/test_present_cpu.py compiles this file together with rt_host.cpp
// and runs it as a child process; it is never loaded into Python and never touches the GPU).
//
//   present_specials BITS...     each a 32-bit pattern, e.g. 0x7fc00000
//
// The values go, three to a pixel, into one row and then into one column (alpha = the value
// itself, so NaN and inf alpha are read too), both row orders; every call must agree with the
// first.  Prints one converted byte per value, in hex, on one line.  Exit 0 = ran clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt/abi.h"

int main(int argc, char** argv) {
  std::vector<float> vals;
  for (int i = 1; i < argc; ++i) {
    const uint32_t bits = (uint32_t)std::strtoul(argv[i], nullptr, 0);
    float v;
    std::memcpy(&v, &bits, 4);
    vals.push_back(v);
  }
  if (vals.empty()) return 2;
  const int n = (int)vals.size(), px = (n + 2) / 3;
  std::vector<float> img((size_t)px * 4, 0.0f);
  for (int i = 0; i < n; ++i) {
    img[(size_t)(i / 3) * 4 + i % 3] = vals[i];
    img[(size_t)(i / 3) * 4 + 3] = vals[i];
  }
  std::vector<uint8_t> row((size_t)px * 4), col((size_t)px * 4), flipped((size_t)px * 4);
  if (rt_quantize_rgba8(img.data(), px, 1, 0, row.data()) != RT_OK) return 3;
  if (rt_quantize_rgba8(img.data(), px, 1, 1, flipped.data()) != RT_OK || flipped != row) return 4;
  if (rt_quantize_rgba8(img.data(), 1, px, 0, col.data()) != RT_OK || col != row) return 5;
  if (rt_quantize_rgba8(img.data(), 1, px, 1, flipped.data()) != RT_OK) return 6;
  for (int p = 0; p < px; ++p)
    if (std::memcmp(&flipped[(size_t)(px - 1 - p) * 4], &row[(size_t)p * 4], 4) != 0) return 7;
  for (int p = 0; p < px; ++p)
    if (row[(size_t)p * 4 + 3] != 255) return 8;
  if (rt_quantize_rgba8(nullptr, px, 1, 0, row.data()) != RT_E_INVAL) return 9;
  if (rt_quantize_rgba8(img.data(), px, 1, 0, nullptr) != RT_E_INVAL) return 10;
  for (int i = 0; i < n; ++i) std::printf("%02x%s", row[(size_t)(i / 3) * 4 + i % 3], i + 1 < n ? " " : "\n");
  return 0;
}
