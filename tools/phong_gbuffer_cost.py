#!/usr/bin/env python
"""What rt_set_phong_gbuffer costs per launch of modes 3 and 4 (profiles/r14_phong_gbuffer_cost.txt).

Per case (a bench config's scene and size), one context, one process:

  launches  the switch off and on alternating, ROUNDS rounds: after a warm-up (mode 4: long enough
            for the tile schedule to have taken up an order; its state is printed) BURSTS
            bursts of REPS back-to-back single-frame launches between two events, ms per launch
            (the method of tools/present_cost.py and bench.py's roofline.kernel_ms); where the host
            cannot enqueue as fast as the kernel runs (config (a)) a burst times the host, so each
            round also brackets REPS launches one by one (rt_enable_timing): "kernel" ms per launch;
  copy      in the same process and on the same stream, a device-to-device hipMemcpyAsync of 32 B
            per pixel, timed the same way: the switch adds exactly those bytes of stores (16 B of
            normals and 16 B of depth per pixel), so the copy (which also reads them) is the
            yardstick for what moving them costs.

Reported: the medians, the added time per launch (on - off) and that over the copy's time.

    python tools/phong_gbuffer_cost.py [--cases a:3,a:4,b:3,b:4,d:3,d:4] [--reps 50] [--bursts 3] [--rounds 5]
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench import CONFIGS, config_header  # noqa: E402
from present_cost import burst_ms, fmt, hip_ok, hip_runtime  # noqa: E402
from real_time_ray_tracer_amd import H_COMPUTE, P_COMPUTE, Renderer  # noqa: E402


def measure(config, mode, reps, bursts, rounds):
    W, H, S, spp = CONFIGS[config][:4]
    h = config_header(config)
    r = Renderer(W, H, S, spp)
    h.set_mode(0, h.num_objects)
    r.upload_header(h)
    hip = hip_runtime()
    stream = C.c_void_p(r._lib.rt_get_stream(r.ctx))
    px = W * H
    state = {"f": 0}

    def launch():
        state["f"] = r.dispatch(mode, state["f"])

    times, kern = {0: [], 1: []}, {0: [], 1: []}
    prog = {3: P_COMPUTE, 4: H_COMPUTE}[mode]
    for _ in range(rounds):
        for on in (0, 1):
            r.set_phong_gbuffer(bool(on))
            for _ in range(3 if mode == 3 else 48):  # mode 4: costs are read back every 16 launches
                launch()
                if mode == 4:
                    r.synchronize()
            ms = burst_ms(hip, stream, launch, reps, bursts)
            times[on].append(statistics.median(ms))
            r.enable_timing(True)
            r.reset_stats()
            for _ in range(reps):
                launch()
            n, total = r.kernel_stats(prog)
            r.enable_timing(False)
            kern[on].append(total / n)
            sched = r.tile_schedule_state() if mode == 4 else "-"
            print(f"  ({config}) {W}x{H} {S} spheres mode {mode} switch {'on ' if on else 'off'}: {fmt(ms)} ms per launch; "
                  f"kernel {total / n:.4f} (tile schedule state {sched})")
    src, dst = C.c_void_p(), C.c_void_p()
    hip_ok(hip.hipMalloc(C.byref(src), px * 32), "hipMalloc")
    hip_ok(hip.hipMalloc(C.byref(dst), px * 32), "hipMalloc")
    cp = burst_ms(hip, stream, lambda: hip_ok(hip.hipMemcpyAsync(dst, src, px * 32, 3, stream), "hipMemcpyAsync"),
                  reps, bursts * rounds)
    r.synchronize()
    hip.hipFree(src)
    hip.hipFree(dst)
    r.close()
    off, on, c = statistics.median(times[0]), statistics.median(times[1]), statistics.median(cp)
    print(f"({config}) {W}x{H} mode {mode}: off {fmt(times[0])} median {off:.4f}; on {fmt(times[1])} median {on:.4f} ms per launch")
    koff, kon = statistics.median(kern[0]), statistics.median(kern[1])
    print(f"({config}) {W}x{H} mode {mode}: kernel alone (one event pair per launch): off {fmt(kern[0])} median {koff:.4f}; "
          f"on {fmt(kern[1])} median {kon:.4f}; added {kon - koff:+.4f} ms = {(kon - koff) / c:.2f} x the copy")
    print(f"({config}) {W}x{H} mode {mode}: device-to-device copy of {px * 32 / 1e6:.1f} MB (32 B per pixel): {fmt(cp)} "
          f"median {c:.4f} ms = {px * 64 / c / 1e6:.1f} GB/s read + written")
    print(f"({config}) {W}x{H} mode {mode}: added {on - off:+.4f} ms per launch = {(on - off) / c:.2f} x the copy; "
          f"{px * 32 / max(on - off, 1e-9) / 1e6:.1f} GB/s of added stores")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a:3,a:4,b:3,b:4,d:3,d:4", help="config:mode pairs (the scene and size of a bench config)")
    ap.add_argument("--reps", type=int, default=50, help="launches per burst")
    ap.add_argument("--bursts", type=int, default=3, help="bursts per round")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    for case in a.cases.split(","):
        config, mode = case.split(":")
        measure(config, int(mode), a.reps, a.bursts, a.rounds)


if __name__ == "__main__":
    main()
