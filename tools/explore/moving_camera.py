#!/usr/bin/env python
"""The cull cache (rt_set_cull_cache) when the camera moves: a config rendered pipelined (mode 1)
as bench.py does, wall time per frame of
  still    the camera never moves (every frame after the second loads its pools' masks),
  moving   the camera nudged every frame (no table is ever built: the parent's code path),
  moves    one nudge every --period frames (each move: two frames of in-kernel cull and one fill),
each --rounds times, alternating.  Prints one JSON line; `move_cost_ms` is what one move costs over
the still rate, `still_saving_ms` what a still frame saves over a moving one.

    python tools/explore/moving_camera.py --config d
    RTRT_LIB=build/v_parent/librtrt.so python tools/explore/moving_camera.py --config d   # a build without the cache
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from bench import CONFIGS, config_header  # noqa: E402
from real_time_ray_tracer_amd import Renderer  # noqa: E402

CAM = 4  # RT_HDR_CAMERA_LOCATION


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="d")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--period", type=int, default=24, help="`moves`: frames between two nudges")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-cache", action="store_true", help="rt_set_cull_cache(0)")
    args = ap.parse_args()
    W, H, S, spp, mode, desc = CONFIGS[args.config]
    assert mode == 1, "a mode-1 config (pipelined frames)"
    h = config_header(args.config)
    r = Renderer(W, H, S, spp)
    has_cache = hasattr(r._lib, "rt_set_cull_cache") and hasattr(r._lib, "rt_cull_cache_stats")
    if args.no_cache and has_cache:
        r.set_cull_cache(False)
    r.enable_pipelining(True)
    state = {"f": 0, "k": 0}

    def run(n, every):
        """n frames, the camera nudged before every `every`-th (0: never); wall seconds."""
        r.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            if every and i % every == 0:
                h.vec4(CAM)[0] += np.float32(1e-4)
            h.fill_rand_buffer(7000 + state["k"])
            h.set_mode(state["f"], h.num_objects)
            r.upload_header(h)
            state["f"] = r.dispatch(1, state["f"])
            state["k"] += 1
        r.synchronize()
        return time.perf_counter() - t0

    def cached():
        return r.cull_cache_stats() if has_cache else {"fills": None, "cached_launches": None, "table_bytes": None}

    run(48, 0)  # ring fill, clocks
    res = {"still": [], "moving": [], "moves": []}
    stats = {}
    for _ in range(args.rounds):
        for name, every in (("still", 0), ("moving", 1), ("moves", args.period)):
            run(4, 0)  # every pass starts from a still camera with the table filled
            s0 = cached()
            res[name].append(run(args.frames, every) / args.frames * 1e3)
            s1 = cached()
            if has_cache:
                stats[name] = {k: s1[k] - s0[k] for k in ("fills", "cached_launches")}
    med = {k: float(np.median(v)) for k, v in res.items()}
    nmoves = (args.frames + args.period - 1) // args.period
    out = {"config": desc, "frames": args.frames, "period": args.period, "cull_cache": has_cache and not args.no_cache,
           "ms_per_frame": {k: [round(x, 4) for x in v] for k, v in res.items()},
           "ms_per_frame_median": {k: round(v, 4) for k, v in med.items()},
           "still_saving_ms": round(med["moving"] - med["still"], 4),
           "move_cost_ms": round((med["moves"] - med["still"]) * args.frames / nmoves, 4),
           "per_pass_cache_stats": stats, "table_bytes": cached()["table_bytes"]}
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
