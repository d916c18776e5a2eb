#!/usr/bin/env python
"""What the ray queries cost (profiles/r16_ray_query.txt): rt_trace_pixels_device over every pixel
of a 3840x2160 frame and rt_occluded_device from the hit points to the light, on config (d)'s
64-sphere scene and config (e)'s 256 spheres, each event-timed for 20 launches after 3 warm-ups on a
torch stream the context is ordered on.  Reported per kernel: ms per launch (median, min), rays/s,
and ray-shape tests/s x 20 FLOP as a share of the 78.6 TFLOP/s non-packed FP32 peak, the compute
bound of a scan of every shape per ray (about 20 FLOP per test against 44 B per ray).  Alongside,
from the same session, phong_gbuf_kernel's time per launch on the (d) scene: the frame kernel
that traces the same primary rays with its cone cull, plus the shadow rays and the shading, as a
yardstick to set the ratio against, not a target.

    python tools/query_bench.py [--out profiles/r16_ray_query.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from bench import CONFIGS, config_header  # noqa: E402
from real_time_ray_tracer_amd import P_COMPUTE, Renderer  # noqa: E402

W, H = 3840, 2160
PEAK_FP32 = 78.6e12  # non-packed FP32 FLOP/s
FLOP_PER_TEST = 20
WARMUP, LAUNCHES = 3, 20


def timed(torch, stream, launch):
    """ms of each of LAUNCHES launches (an event pair around each) after WARMUP launches."""
    for _ in range(WARMUP):
        launch()
    pairs = []
    for _ in range(LAUNCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        pairs.append((e0, e1))
    stream.synchronize()
    ms = [a.elapsed_time(b) for a, b in pairs]
    # cross-check on the host clock: the same launches back to back, one wait at the end
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        launch()
    stream.synchronize()
    return ms, (time.perf_counter() - t0) * 1e3 / LAUNCHES


def line(what, timing, rays, nobj):
    ms, wall = timing
    med, lo = statistics.median(ms), min(ms)
    tests = rays * nobj / (med * 1e-3)
    return (f"{what:34s} {med:8.3f} ms median {lo:8.3f} ms min ({wall:.3f} ms per launch by the host clock)  "
            f"{rays / (med * 1e-3) / 1e9:7.3f} Grays/s  "
            f"{tests / 1e12:6.3f} Ttests/s  {100.0 * tests * FLOP_PER_TEST / PEAK_FP32:5.1f}% of the FP32 peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = W * H
    out = [f"ray queries at {W}x{H} = {n} rays, {LAUNCHES} launches after {WARMUP} warm-ups, "
           f"{torch.cuda.get_device_name(0)}"]
    phong_ms = None
    with torch.cuda.stream(stream):
        xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
        xy = torch.from_numpy(np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)).to(dev)  # row-major pixels
        t = torch.empty(n, dtype=torch.float32, device=dev)
        ind = torch.empty(n, dtype=torch.int32, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        for cfg in ("d", "e"):
            _, _, S, spp, _, _ = CONFIGS[cfg]
            h = config_header(cfg)
            with Renderer(W, H, S, spp) as r:
                r.set_stream(stream)
                r.upload_header(h)
                for thr in (0.0, 0.0001):
                    ms = timed(torch, stream, lambda: r.trace_pixels_device(
                        xy.data_ptr(), n, thr, t.data_ptr(), ind.data_ptr(), nrm.data_ptr(), dirs.data_ptr()))
                    out.append(line(f"({cfg}) {S} spheres trace_pixels thr {thr:g}", ms, n, h.num_objects))
                hits = float((ind >= 0).float().mean().item())
                cam = torch.from_numpy(h.data[16:19].copy()).to(dev)
                light = torch.from_numpy(h.data[20:23].copy()).to(dev)
                a_pts = (cam[None, :] + t.clamp(min=0.0)[:, None] * dirs).contiguous()  # misses: the camera
                b_pts = light[None, :].expand(n, 3).contiguous()
                ms = timed(torch, stream,
                           lambda: r.occluded_device(a_pts.data_ptr(), b_pts.data_ptr(), n, occ.data_ptr()))
                out.append(line(f"({cfg}) {S} spheres occluded to the light", ms, n, h.num_objects) +
                           f"  (upper bound: a segment stops at its first occluder; {hits:.1%} of the rays hit, "
                           f"{float(occ.float().mean().item()):.1%} occluded)")
                if cfg == "d":
                    r.set_phong_gbuffer(True)
                    f = 0
                    for _ in range(WARMUP):
                        f = r.dispatch(3, f)
                    r.enable_timing(True)
                    for _ in range(LAUNCHES):
                        f = r.dispatch(3, f)
                    r.synchronize()
                    k, total = r.kernel_stats(P_COMPUTE)
                    phong_ms = total / k
                    out.append(f"(d) phong_gbuf_kernel, same session       {phong_ms:8.3f} ms mean of {k} launches "
                               f"(cone-culled primary rays + shadow rays + shading)")
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
