#!/usr/bin/env python
"""What the 8-bit display output (rt_present, the blit of src/main.cpp:783-797) costs at a bench
config's size, in three measurements (profiles/r11_present.txt):

  kernel    present_kernel alone: bursts of back-to-back launches between two events after a
            warm-up (the method of bench.py's roofline.kernel_ms), ms per launch and its bytes
            (16 B read + 4 B written per pixel) over that time; in the same process a device-to-
            device hipMemcpyAsync of the float image (16 B read + 16 B written per pixel), timed
            the same way, as the yardstick for a pure streaming pass; the ratio of the byte rates.
  frame     the pipelined frame with a present after every dispatch against the frame without,
            alternating, RUNS runs each: wall ms per frame over FRAMES frames (FrameDriver).
  download  rt_download(image) against rt_download_rgba8, wall ms, median of 10 each.

    python tools/present_cost.py [--config d] [--only kernel|frame|download]
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
from bench import CONFIGS, config_header  # noqa: E402
from real_time_ray_tracer_amd import FrameDriver, Renderer  # noqa: E402


def hip_runtime():
    """The HIP runtime this process already uses (the one torch or librtrt.so loaded)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            lib.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
            lib.hipEventSynchronize.argtypes = [C.c_void_p]
            lib.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            lib.hipFree.argtypes = [C.c_void_p]
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def hip_ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hipError {rc}")


def burst_ms(hip, stream, launch, reps, bursts):
    """ms per launch of `bursts` bursts of `reps` back-to-back launches, after 3 warm-up launches."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    hip_ok(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    for _ in range(3):
        launch()
    out = []
    for _ in range(bursts):
        hip_ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
        for _ in range(reps):
            launch()
        hip_ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
        hip_ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        ms = C.c_float()
        hip_ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        out.append(ms.value / reps)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return out


def rendered(config, pipelined, frames=12):
    W, H, S, spp, mode, _ = CONFIGS[config]
    r = Renderer(W, H, S, spp)
    if pipelined:
        r.enable_pipelining(True)
    drv = FrameDriver(r, config_header(config), mode)
    for _ in range(frames):
        drv.compute()
    r.synchronize()
    return r, drv


def fmt(xs):
    return " ".join(f"{x:.4f}" for x in xs)


def measure_kernel(config, reps, bursts):
    W, H = CONFIGS[config][:2]
    r, _ = rendered(config, False, 3)
    hip = hip_runtime()
    stream = C.c_void_p(r._lib.rt_image_stream(r.ctx))
    px = W * H
    for top_down in (0, 1):
        ms = burst_ms(hip, stream, lambda: r.present(bool(top_down)), reps, bursts)
        m = statistics.median(ms)  # (the ratio below takes the display order's, top_down = 1)
        print(f"present_kernel {W}x{H} top_down={top_down}: {bursts} bursts of {reps}: {fmt(ms)} ms per launch; "
              f"median {m:.4f} ms = {px * 20 / m / 1e6:.1f} GB/s of {px * 20 / 1e6:.1f} MB (16 B read + 4 B written per pixel)")
    present_ms = m
    dst = C.c_void_p()
    hip_ok(hip.hipMalloc(C.byref(dst), px * 16), "hipMalloc")
    src = C.c_void_p(r.image_device_ptr())
    ms = burst_ms(hip, stream, lambda: hip_ok(hip.hipMemcpyAsync(dst, src, px * 16, 3, stream), "hipMemcpyAsync"),
                  reps, bursts)
    c = statistics.median(ms)
    print(f"hipMemcpyAsync device-to-device of the float image: {fmt(ms)} ms per copy; median {c:.4f} ms = "
          f"{px * 32 / c / 1e6:.1f} GB/s of {px * 32 / 1e6:.1f} MB (16 B read + 16 B written per pixel)")
    print(f"byte rate of present_kernel / byte rate of the copy = {(px * 20 / present_ms) / (px * 32 / c):.3f}")
    r.synchronize()
    hip.hipFree(dst)
    r.close()


def measure_frame(config, frames, runs):
    r, drv = rendered(config, True, 24)
    r.present(True)  # the 8-bit buffer exists before anything is timed
    r.synchronize()

    def leg(with_present):
        t0 = time.perf_counter()
        for _ in range(frames):
            drv.compute()
            if with_present:
                r.present(True)
        r.synchronize()
        return (time.perf_counter() - t0) / frames * 1e3

    leg(False), leg(True)  # one discarded round
    without, with_ = [], []
    for _ in range(runs):
        without.append(leg(False))
        with_.append(leg(True))
    a, b = statistics.median(without), statistics.median(with_)
    print(f"pipelined ({config}) frame, {frames} frames per run, {runs} runs each, alternating (wall ms per frame):")
    print(f"  without present: {fmt(without)}  median {a:.4f}  spread {max(without) - min(without):.4f}")
    print(f"  with present:    {fmt(with_)}  median {b:.4f}  spread {max(with_) - min(with_):.4f}")
    print(f"  difference of the medians {b - a:+.4f} ms per frame")
    r.close()


def measure_download(config, n=10):
    W, H = CONFIGS[config][:2]
    r, _ = rendered(config, False, 3)
    im = np.empty((H, W, 4), np.float32)
    out = np.empty((H, W, 4), np.uint8)
    fp = im.ctypes.data_as(C.POINTER(C.c_float))
    op = out.ctypes.data_as(C.c_void_p)

    def timed(call):
        call()
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    a = timed(lambda: r._c(r._lib.rt_download(r.ctx, None, None, None, fp), "rt_download"))
    b = timed(lambda: r._c(r._lib.rt_download_rgba8(r.ctx, 1, op), "rt_download_rgba8"))
    print(f"rt_download(image) {W}x{H}, {im.nbytes / 1e6:.1f} MB to pageable host memory: median of {n} "
          f"{statistics.median(a):.3f} ms (min {min(a):.3f}, max {max(a):.3f})")
    print(f"rt_download_rgba8 (present + wait + copy), {out.nbytes / 1e6:.1f} MB: median of {n} "
          f"{statistics.median(b):.3f} ms (min {min(b):.3f}, max {max(b):.3f})")
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="d", choices=sorted(CONFIGS))
    ap.add_argument("--only", choices=["kernel", "frame", "download"])
    ap.add_argument("--reps", type=int, default=50, help="launches per burst")
    ap.add_argument("--bursts", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40, help="frames per timed run")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.only in (None, "kernel"):
        measure_kernel(a.config, a.reps, a.bursts)
    if a.only in (None, "frame"):
        measure_frame(a.config, a.frames, a.runs)
    if a.only in (None, "download"):
        measure_download(a.config)


if __name__ == "__main__":
    main()
