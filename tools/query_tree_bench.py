#!/usr/bin/env python
"""The query tree against the linear scan (profiles/r18_query_tree.txt): rt_trace_pixels_device at
threshold 0 over every pixel of a 3840x2160 frame and rt_occluded_device from the hit points to the
light, on rt_scenegen scenes of 64, 256, 1024 and 2048 spheres, with the rays in pixel order
(coherent) and in one fixed random permutation (incoherent).  Linear and tree run on one context in
one session, alternating, ROUNDS times each; every round is 20 event-timed launches after 3
warm-ups.  Per case: the median and minimum over all launches of each side, the spread of the
linear side's round medians (its own run-to-run spread, the bar a win has to clear), and the ratio.
The answers of both sides are compared byte for byte at the full size before anything is timed.

    python tools/query_tree_bench.py [--sizes 64,256,1024,2048] [--label TEXT] [--out FILE] [--append]

RTRT_LIB names another build of the library (the kTreeLeaf variants); --label goes into the heading.
"""
import argparse
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from real_time_ray_tracer_amd import Header, Renderer, aspect_for  # noqa: E402

W, H = 3840, 2160
WARMUP, LAUNCHES, ROUNDS = 3, 20, 3


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
    return [a.elapsed_time(b) for a, b in pairs]


def alternate(torch, stream, r, launch):
    """{False: rounds, True: rounds} of `launch` with the tree off and on, alternating."""
    ms = {False: [], True: []}
    for _ in range(ROUNDS):
        for on in (False, True):
            r.set_query_tree(on)
            ms[on].append(timed(torch, stream, launch))
    return ms


def line(what, ms):
    lin, tree = ms[False], ms[True]
    flat = lambda rounds: [v for rd in rounds for v in rd]  # noqa: E731
    lm, tm = statistics.median(flat(lin)), statistics.median(flat(tree))
    meds = [statistics.median(rd) for rd in lin]
    tmeds = [statistics.median(rd) for rd in tree]
    return (f"{what:44s} linear {lm:8.3f} ms median {min(flat(lin)):8.3f} min, round medians {min(meds):.3f}..{max(meds):.3f} "
            f"(spread {100.0 * (max(meds) - min(meds)) / lm:4.1f}%) | tree {tm:8.3f} ms median {min(flat(tree)):8.3f} min, "
            f"round medians {min(tmeds):.3f}..{max(tmeds):.3f} | linear / tree {lm / tm:6.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,1024,2048")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n = W * H
    out = [f"query tree against the linear scan{' [' + a.label + ']' if a.label else ''}: {W}x{H} = {n} rays, per side "
           f"{ROUNDS} alternating rounds of {LAUNCHES} launches after {WARMUP} warm-ups, {torch.cuda.get_device_name(0)}"]
    with torch.cuda.stream(stream):
        xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
        xy_np = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)  # row-major pixels
        perm_np = np.random.default_rng(18).permutation(n)
        xy = {"coherent": torch.from_numpy(xy_np).to(dev), "incoherent": torch.from_numpy(xy_np[perm_np]).to(dev)}
        perm = torch.from_numpy(perm_np).to(dev)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        ind = torch.empty(n, dtype=torch.int32, device=dev)
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
        dirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        for S in [int(s) for s in a.sizes.split(",")]:
            h = Header.synthetic(S, 1, 1234, aspect_for(W, H))
            with Renderer(W, H, S, 1, num_frames=1) as r:
                r.set_stream(stream)
                r.upload_header(h)
                cam = torch.from_numpy(h.data[16:19].copy()).to(dev)
                light = torch.from_numpy(h.data[20:23].copy()).to(dev)
                trace = lambda p: r.trace_pixels_device(p.data_ptr(), n, 0.0, t.data_ptr(), ind.data_ptr(),  # noqa: E731
                                                        nrm.data_ptr(), dirs.data_ptr())
                # the same answers first: every output of both sides, byte for byte, at the size timed
                got = {}
                for on in (False, True):
                    r.set_query_tree(on)
                    trace(xy["coherent"])
                    stream.synchronize()
                    a_pts = (cam[None, :] + t.clamp(min=0.0)[:, None] * dirs).contiguous()  # misses: the camera
                    b_pts = light[None, :].expand(n, 3).contiguous()
                    r.occluded_device(a_pts.data_ptr(), b_pts.data_ptr(), n, occ.data_ptr())
                    stream.synchronize()
                    got[on] = [x.clone() for x in (t, ind, nrm.view(torch.int32), dirs.view(torch.int32), occ)]
                    st = r.query_tree_stats()
                same = all(bool(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                            y.view(torch.int32) if y.dtype == torch.float32 else y))
                           for x, y in zip(got[False], got[True]))
                hits = float((ind >= 0).float().mean().item())
                out.append(f"{S} spheres: tree of {st['nodes']} nodes, {st['leaves']} leaves, {st['always']} always, buffer "
                           f"{st['bytes']} bytes; {hits:.1%} of the pixel rays hit, {float(occ.float().mean().item()):.1%} of the "
                           f"segments occluded; linear and tree outputs {'equal byte for byte' if same else 'DIFFER'}")
                if not same:
                    raise SystemExit("\n".join(out))
                pts = {"coherent": a_pts, "incoherent": a_pts[perm].contiguous()}
                for order in ("coherent", "incoherent"):
                    out.append(line(f"{S} spheres {order} closest hit thr 0", alternate(torch, stream, r, lambda: trace(xy[order]))))
                    out.append(line(f"{S} spheres {order} occluded to the light", alternate(
                        torch, stream, r, lambda: r.occluded_device(pts[order].data_ptr(), b_pts.data_ptr(), n, occ.data_ptr()))))
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
