// rt_gbuf.hip — the g-buffer ring (rt_gbuf.h).
#include "rt_gbuf.h"

namespace rt {

hipError_t GbufRing::create(int F, int depth, size_t slot_bytes, hipStream_t st) {
  const int NB = F + depth;
  hipError_t e = hipSuccess;
  for (auto& r : ring) {
    r.buf.assign(NB, nullptr);
    for (int k = 0; k < NB && e == hipSuccess; ++k) e = hipMalloc(&r.buf[k], slot_bytes);
  }
  for (auto& r : ring)
    for (int k = 0; k < NB && e == hipSuccess; ++k) e = hipMemsetAsync(r.buf[k], 0, slot_bytes, st);
  for (auto& r : ring) {
    r.slot.resize(F);
    for (int k = 0; k < F; ++k) r.slot[k] = k;
  }
  spare = F;
  for (int q = 0; q < depth; ++q) {
    raw_buf[q] = F + q;  // raw buffer 0 is whichever buffer is the sequential spare
    nrm_free[q] = dep_free[q] = F + q;
  }
  return e;
}

void GbufRing::release() {
  for (auto& r : ring) {
    for (auto p : r.buf)
      if (p) (void)hipFree(p);
    r = SlotRing{};
  }
}

void GbufRing::fill(FrameParams& p, int F, int frame) const {
  for (int s = 0; s < F; ++s) {
    p.hist_pix[s] = ring[kPixels].at(s);
    p.hist_nrm[s] = ring[kNormals].at(s);
    p.hist_dep[s] = ring[kDepth].at(s);
  }
  p.nrm = ring[kNormals].at(frame);
  p.dep = ring[kDepth].at(frame);
  p.nrm_prev = p.nrm;
  p.dep_prev = p.dep;
}

void GbufRing::fresh(FrameParams& p) const {
  p.nrm = ring[kNormals].buf[nrm_free[0]];
  p.dep = ring[kDepth].buf[dep_free[0]];
}

void GbufRing::rotate(int frame, int D) {
  const int xn = nrm_free[0], xd = dep_free[0];
  for (int q = 0; q + 1 < D; ++q) {
    nrm_free[q] = nrm_free[q + 1];
    dep_free[q] = dep_free[q + 1];
  }
  nrm_free[D - 1] = ring[kNormals].slot[frame];
  dep_free[D - 1] = ring[kDepth].slot[frame];
  ring[kNormals].slot[frame] = xn;
  ring[kDepth].slot[frame] = xd;
}

}  // namespace rt
