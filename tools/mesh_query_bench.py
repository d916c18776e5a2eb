#!/usr/bin/env python3
"""Times the mesh queries (include/rt/mesh.h) next to the scene's own ray query, in one session.

Workload: the 3840 x 2160 pixel rays of bench.py's config (d) camera (8.3 M rays, formed on the device
by rt_trace_pixels_device), against generated icospheres of 1 280, 20 480 and 327 680 triangles placed
in view: closest hit (mesh_trace_kernel) and occlusion from the hit points to the light
(mesh_occluded_kernel).  The yardstick is ray_query_kernel on config (d)'s 64 spheres with the same
rays.  Method: every launch goes to one torch stream; after a warm-up, bursts of --burst launches are
timed between two device events; --repeats rounds alternate over all the kernels, and the figures
are the median ms per launch with the least and the greatest round.

    python tools/mesh_query_bench.py [--out FILE] [--burst 10] [--repeats 5] [--levels 3,5,7]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--levels", default="3,5,7")
    args = ap.parse_args()

    import torch

    import bench
    from mesh_cases import icosphere
    from real_time_ray_tracer_amd import Mesh, Renderer

    W, H, S, spp, _, _ = bench.CONFIGS["d"]
    h = bench.config_header("d")
    n = W * H
    stream = torch.cuda.Stream()
    f32 = torch.float32
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with torch.cuda.stream(stream):
        xs = torch.arange(W, dtype=torch.int32, device="cuda").repeat_interleave(H)
        ys = torch.arange(H, dtype=torch.int32, device="cuda").repeat(W)
        d_xy = torch.stack([xs, ys], dim=1).contiguous()
        dirs = torch.zeros(n, 3, dtype=f32, device="cuda")
        t = torch.zeros(n, dtype=f32, device="cuda")
        prim = torch.zeros(n, dtype=torch.int32, device="cuda")
        nrm = torch.zeros(n, 3, dtype=f32, device="cuda")
        occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
    stream.synchronize()
    cam = np.asarray(h.vec4(4)[:3], np.float32)
    light = np.asarray(h.vec4(5)[:3], np.float32)
    d_cam = torch.from_numpy(cam.copy()).cuda()
    origins = torch.from_numpy(np.repeat(cam[None], n, axis=0).copy()).cuda()
    d_light = torch.from_numpy(np.repeat(light[None], n, axis=0).copy()).cuda()
    torch.cuda.synchronize()

    r = Renderer(W, H, S, spp)
    r.set_stream(stream)
    r.upload_header(h)
    r.trace_pixels_device(d_xy.data_ptr(), n, 0.0, d_dirs=dirs.data_ptr())
    r.synchronize()
    centre_dir = dirs[(W // 2) * H + H // 2].cpu().numpy()

    meshes, kernels = [], {}

    def scene_query():
        r.trace_rays_device(origins.data_ptr(), dirs.data_ptr(), n, 0.0, t.data_ptr(), prim.data_ptr(), nrm.data_ptr())

    kernels["ray_query_kernel, 64 spheres"] = scene_query
    for level in map(int, args.levels.split(",")):
        t0 = time.perf_counter()
        verts, tris = icosphere(level, centre=tuple(cam + centre_dir * 12.0), radius=4.0)
        t1 = time.perf_counter()
        m = Mesh(verts, tris)
        t2 = time.perf_counter()
        st = m.stats()
        meshes.append(m)
        # the segments: from each ray's hit point on this mesh (or a point 12 along a missing ray) to the light
        m.trace_rays_device(d_cam.data_ptr(), dirs.data_ptr(), n, 0.0, one_origin=True, d_t=t.data_ptr(),
                            stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            tt = torch.where(t > 0, t, torch.full_like(t, 12.0))
            a = (d_cam[None] + dirs * tt[:, None]).contiguous()
            hits = int((t > 0).sum().item())
        stream.synchronize()
        say(f"mesh {len(tris)} triangles: {st['nodes']} nodes, {st['leaves']} leaves, {st['bytes']} device bytes; "
            f"generated in {t1 - t0:.2f} s, rt_mesh_create {t2 - t1:.2f} s; {hits} of {n} pixel rays hit it")

        def trace(m=m):
            m.trace_rays_device(d_cam.data_ptr(), dirs.data_ptr(), n, 0.0, one_origin=True, d_t=t.data_ptr(),
                                d_prim=prim.data_ptr(), d_normals=nrm.data_ptr(), stream=stream.cuda_stream)

        def occluded(m=m, a=a):
            m.occluded_device(a.data_ptr(), d_light.data_ptr(), n, d_out=occ.data_ptr(), stream=stream.cuda_stream)

        kernels[f"mesh_trace_kernel, {len(tris)} triangles"] = trace
        kernels[f"mesh_occluded_kernel, {len(tris)} triangles"] = occluded

    def burst(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(k):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / k

    for fn in kernels.values():   # warm-up
        burst(fn, 3)
    ms = {name: [] for name in kernels}
    for _ in range(args.repeats):  # the rounds alternate over the kernels
        for name, fn in kernels.items():
            ms[name].append(burst(fn, args.burst))
    say(f"{n} rays per launch, bursts of {args.burst}, {args.repeats} alternating rounds: median ms per launch [least, greatest], Grays/s")
    for name, v in ms.items():
        med = float(np.median(v))
        say(f"  {name:44s} {med:9.4f} ms  [{min(v):.4f}, {max(v):.4f}]  {n / med / 1e6:8.3f} Grays/s")
    for m in meshes:
        m.close()
    r.close()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
