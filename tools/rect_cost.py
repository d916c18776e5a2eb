#!/usr/bin/env python
"""What a rectangle costs against the plane it replaces (profiles/r17_rectangles.txt).

The scene is bench config (p)'s: config (d)'s 64 spheres over a ground plane y = -2.5, at 3840x2160,
16 spp.  Its twin has the ground as a rectangle that covers everything a ray can reach (the same
hits, the same images: tests/test_gpu_rectangles.py test_cover_equals_the_plane), so the two
launches do the same work but for the bounds test.  One context per scene, rt_set_rectangles on in
both, one process:

  frames    modes 1-4, plane and rectangle alternating, ROUNDS rounds: after a warm-up (mode 4: long
            enough for the tile schedule to have taken up an order) BURSTS bursts of REPS
            back-to-back single-frame launches between two events, ms per launch (the method of
            tools/present_cost.py and bench.py's roofline.kernel_ms);
  queries   rt_trace_pixels_device over every pixel's ray at threshold 0.0001 and rt_occluded_device
            from the hit points to the light, timed the same way;
  counters  with --counters, in a run of its own: one counted launch per mode and scene,
            rt_read_counters' slots (the work counters are properties of the algorithm: equal for
            the twins; executed_lane_tests counts the table entries a wave's loops visited).

Reported: the medians and the plane / rectangle ratio.

    python tools/rect_cost.py [--modes 1,2,3,4] [--reps 20] [--bursts 3] [--rounds 5] [--counters]
"""
import argparse
import ctypes as C
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench import CONFIGS, config_header  # noqa: E402
from present_cost import burst_ms, fmt, hip_runtime  # noqa: E402
from real_time_ray_tracer_amd import Renderer  # noqa: E402


def scenes():
    """(plane scene, rectangle scene) of config (p)."""
    hp = config_header("p")
    hr = hp.copy()
    S = CONFIGS["p"][2]
    hr.pack_rectangle(S - 1, (8192.0, -2.5, 8192.0), (0.0, 0.0, -16384.0), (-16384.0, 0.0, 0.0), (0.45, 0.4, 0.35),
                      reflectivity=1.0)
    assert tuple(hr.shapes[S - 1, 0, :3]) == (0.0, 1.0, 0.0)
    return {"plane": hp, "rectangle": hr}


def contexts():
    W, H, S, spp = CONFIGS["p"][:4]
    out = {}
    for name, h in scenes().items():
        r = Renderer(W, H, S, spp)
        r.set_rectangles(True)
        h.set_mode(0, h.num_objects)
        r.upload_header(h)
        out[name] = (r, h)
    return out


def frames(ctx, modes, reps, bursts, rounds):
    W, H, S, spp = CONFIGS["p"][:4]
    hip = hip_runtime()
    for mode in modes:
        times = {k: [] for k in ctx}
        state = {k: 0 for k in ctx}
        for _ in range(rounds):
            for name, (r, _) in ctx.items():
                stream = C.c_void_p(r._lib.rt_get_stream(r.ctx))

                def launch():
                    state[name] = r.dispatch(mode, state[name])

                for _ in range(48 if mode == 4 else 2):  # mode 4: costs are read back every 16 launches
                    launch()
                    if mode == 4:
                        r.synchronize()
                ms = burst_ms(hip, stream, launch, reps, bursts)
                times[name].append(statistics.median(ms))
                print(f"  mode {mode} {name:9s}: {fmt(ms)} ms per launch")
        p, q = statistics.median(times["plane"]), statistics.median(times["rectangle"])
        print(f"(p) {W}x{H} {spp} spp mode {mode}: plane {fmt(times['plane'])} median {p:.4f}; rectangle "
              f"{fmt(times['rectangle'])} median {q:.4f} ms per launch; plane / rectangle = {p / q:.4f}")


def queries(ctx, reps, bursts, rounds):
    import torch

    W, H = CONFIGS["p"][:2]
    n = W * H
    hip = hip_runtime()
    dev = torch.device("cuda", 0)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    xy = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)).to(dev)
    t = torch.empty(n, dtype=torch.float32, device=dev)
    ind = torch.empty(n, dtype=torch.int32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    dirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pts = {}
    for name, (r, h) in ctx.items():
        r.trace_pixels_device(xy.data_ptr(), n, 0.0001, t.data_ptr(), ind.data_ptr(), nrm.data_ptr(), dirs.data_ptr())
        r.synchronize()
        cam = torch.from_numpy(h.data[16:19].copy()).to(dev)
        light = torch.from_numpy(h.data[20:23].copy()).to(dev)
        a = (cam[None, :] + t.clamp(min=0.0)[:, None] * dirs).contiguous()
        pts[name] = (a, light[None, :].expand(n, 3).contiguous(), float((ind >= 0).float().mean().item()))
    torch.cuda.synchronize()
    tq, oq = {k: [] for k in ctx}, {k: [] for k in ctx}
    for _ in range(rounds):
        for name, (r, _) in ctx.items():
            stream = C.c_void_p(r._lib.rt_get_stream(r.ctx))
            a, b, _ = pts[name]
            ms = burst_ms(hip, stream, lambda: r.trace_pixels_device(xy.data_ptr(), n, 0.0001, t.data_ptr(), ind.data_ptr(),
                                                                      nrm.data_ptr(), dirs.data_ptr()), reps, bursts)
            tq[name].append(statistics.median(ms))
            ms = burst_ms(hip, stream, lambda: r.occluded_device(a.data_ptr(), b.data_ptr(), n, occ.data_ptr()), reps, bursts)
            oq[name].append(statistics.median(ms))
            r.synchronize()
    for what, d in (("trace_pixels thr 0.0001", tq), ("occluded to the light", oq)):
        p, q = statistics.median(d["plane"]), statistics.median(d["rectangle"])
        print(f"(p) {n} rays {what}: plane {fmt(d['plane'])} median {p:.4f}; rectangle {fmt(d['rectangle'])} median "
              f"{q:.4f} ms per launch; plane / rectangle = {p / q:.4f}  ({pts['plane'][2]:.1%} of the rays hit)")


def counters(ctx, modes):
    for mode in modes:
        for name, (r, _) in ctx.items():
            r.enable_counters(True)
            r.read_counters()
            r.dispatch(mode, 0)
            print(f"(p) mode {mode} {name:9s} counters: {r.read_counters()}")
            r.enable_counters(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="1,2,3,4")
    ap.add_argument("--reps", type=int, default=20, help="launches per burst")
    ap.add_argument("--bursts", type=int, default=3, help="bursts per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--counters", action="store_true", help="the work counters only (a run of its own)")
    a = ap.parse_args()
    modes = [int(m) for m in a.modes.split(",")]
    ctx = contexts()
    if a.counters:
        counters(ctx, modes)
    else:
        frames(ctx, modes, a.reps, a.bursts, a.rounds)
        queries(ctx, a.reps, a.bursts, a.rounds)
    for r, _ in ctx.values():
        r.close()


if __name__ == "__main__":
    main()
