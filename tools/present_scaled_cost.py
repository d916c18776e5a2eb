#!/usr/bin/env python
"""What the 8-bit display output at window size (rt_present_scaled, the blit of src/main.cpp:783-797
with its GL_LINEAR scaling, 381-388) costs, by the method of tools/present_cost.py
(profiles/r12_present_scaled.txt):

  kernel    present_scaled_kernel alone on a random image in [-0.1, 1.1): bursts of back-to-back
            launches between two events after a warm-up, ms per launch, for each SRC->OUT case; in
            the same process present_kernel (the 1:1 conversion) of an image of the OUTPUT's size
            and a device-to-device hipMemcpyAsync of that image as yardsticks.  Byte model of the
            scaled kernel: the output's 4 B per pixel plus 16 B for every source texel some tap
            touches, counted once (the taps' distinct rows x distinct columns); of present_kernel
            16 B read + 4 B written per pixel; of the copy 16 B read + 16 B written per pixel.
  download  rt_download_rgba8_scaled to OUT against rt_download_rgba8 of the source, wall ms,
            median of 10 each.

    python tools/present_scaled_cost.py [--case 440x330:1920x1080 ...] [--only kernel|download]
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from present_cost import burst_ms, fmt, hip_ok, hip_runtime  # noqa: E402
from real_time_ray_tracer_amd import Renderer  # noqa: E402

CASES = ["440x330:1920x1080", "3840x2160:1920x1080", "3840x2160:3840x2160"]


def touched(n_out, n_src):
    """Distinct source indices one axis's taps touch (the rule of include/rt/abi.h)."""
    i = np.arange(n_out, dtype=np.int64)
    x0 = ((2 * i + 1) * n_src - n_out) // (2 * n_out)
    return np.unique(np.clip(np.concatenate([x0, x0 + 1]), 0, n_src - 1)).size


def random_image(W, H, seed):
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.rand((H, W, 4), generator=g, device="cuda", dtype=torch.float32) * 1.2 - 0.1
    torch.cuda.synchronize()
    return img


def measure_kernel(case, reps, bursts):
    (W, H), (ow, oh) = case
    src = random_image(W, H, 1)
    same = random_image(ow, oh, 2)  # the 1:1 yardsticks' image, of the output's size
    hip = hip_runtime()  # (loaded by now: torch's)
    with Renderer(W, H, 1, 1) as r, Renderer(ow, oh, 1, 1) as y:
        r.bind_image(src.data_ptr())
        y.bind_image(same.data_ptr())
        stream = C.c_void_p(r._lib.rt_image_stream(r.ctx))
        ms = burst_ms(hip, stream, lambda: r.present_scaled(ow, oh, True), reps, bursts)
        m = statistics.median(ms)
        model = ow * oh * 4 + touched(ow, W) * touched(oh, H) * 16
        print(f"present_scaled_kernel {W}x{H} -> {ow}x{oh}: {bursts} bursts of {reps}: {fmt(ms)} ms per launch; median "
              f"{m:.4f} ms = {model / m / 1e6:.1f} GB/s of {model / 1e6:.1f} MB (4 B written per output pixel + 16 B "
              f"per source texel touched, once)")
        ystream = C.c_void_p(y._lib.rt_image_stream(y.ctx))
        ms = burst_ms(hip, ystream, lambda: y.present(True), reps, bursts)
        p = statistics.median(ms)
        px = ow * oh
        print(f"present_kernel {ow}x{oh} (1:1): {fmt(ms)} ms per launch; median {p:.4f} ms = {px * 20 / p / 1e6:.1f} GB/s "
              f"of {px * 20 / 1e6:.1f} MB; scaled / 1:1 time = {m / p:.2f}")
        dst = C.c_void_p()
        hip_ok(hip.hipMalloc(C.byref(dst), px * 16), "hipMalloc")
        ms = burst_ms(hip, ystream, lambda: hip_ok(hip.hipMemcpyAsync(dst, C.c_void_p(same.data_ptr()), px * 16, 3,
                                                                      ystream), "hipMemcpyAsync"), reps, bursts)
        c = statistics.median(ms)
        print(f"hipMemcpyAsync device-to-device of a {ow}x{oh} float image: {fmt(ms)} ms per copy; median {c:.4f} ms = "
              f"{px * 32 / c / 1e6:.1f} GB/s of {px * 32 / 1e6:.1f} MB; byte rate of present_scaled_kernel / byte rate "
              f"of the copy = {(model / m) / (px * 32 / c):.3f}")
        r.synchronize()
        y.synchronize()
        hip.hipFree(dst)


def measure_download(case, n=10):
    (W, H), (ow, oh) = case
    src = random_image(W, H, 3)
    out = np.empty((H, W, 4), np.uint8)
    small = np.empty((oh, ow, 4), np.uint8)

    def timed(call):
        call()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    with Renderer(W, H, 1, 1) as r:
        r.bind_image(src.data_ptr())
        a = timed(lambda: r._c(r._lib.rt_download_rgba8(r.ctx, 1, out.ctypes.data_as(C.c_void_p)), "rt_download_rgba8"))
        b = timed(lambda: r._c(r._lib.rt_download_rgba8_scaled(r.ctx, ow, oh, 1, small.ctypes.data_as(C.c_void_p)),
                               "rt_download_rgba8_scaled"))
    print(f"rt_download_rgba8 {W}x{H} (present + wait + copy), {out.nbytes / 1e6:.1f} MB to pageable host memory: "
          f"median of {n} {statistics.median(a):.3f} ms (min {min(a):.3f}, max {max(a):.3f})")
    print(f"rt_download_rgba8_scaled {W}x{H} -> {ow}x{oh}, {small.nbytes / 1e6:.1f} MB: median of {n} "
          f"{statistics.median(b):.3f} ms (min {min(b):.3f}, max {max(b):.3f})")


def parse(case):
    a, b = case.split(":")
    return tuple(int(v) for v in a.split("x")), tuple(int(v) for v in b.split("x"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", help="SRCWxSRCH:OUTWxOUTH (default: the three of the module docstring)")
    ap.add_argument("--only", choices=["kernel", "download"])
    ap.add_argument("--reps", type=int, default=50, help="launches per burst")
    ap.add_argument("--bursts", type=int, default=5)
    a = ap.parse_args()
    cases = [parse(c) for c in (a.case or CASES)]
    if a.only in (None, "kernel"):
        for c in cases:
            measure_kernel(c, a.reps, a.bursts)
    if a.only in (None, "download"):
        measure_download(parse("3840x2160:1920x1080") if not a.case else cases[0])


if __name__ == "__main__":
    main()
