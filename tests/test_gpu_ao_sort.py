"""RT_B1_SORT: ao_batch_kernel deals a pool's samples to its 64-lane batches by bounce direction
(a counting sort of the pool's items on hemi's octant, hemi parked in the samples' result slots).
The order cannot change a result, so everything here is the library against the CPU oracle as in
test_gpu_parity.py (normals and depth bit-identical, colours within the 1e-4 bar, modes 1 and 2), at
the smallest shapes where the new indexing could go wrong, plus the sorted build against the
RT_B1_SORT=0 build (make b1sort0) through tools/ab.py.  Scenes without planes of at least 48
spheres (kB1SortMinObj) take the sorted instantiations."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from conftest import assert_bitwise, assert_close
from real_time_ray_tracer_amd import SSBO, FrameDriver, Header, Renderer, aspect_for
from test_gpu_parity import make_header, run_both

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SORT_MIN = 48  # kB1SortMinObj (rt_kernels_impl.h)


def check(h, W, H, frames=2, modes=(1, 2), what=""):
    out = None
    for mode in modes:
        g, s, img = run_both(h, W, H, mode, frames)
        assert_close(g.image, img, f"{what} mode {mode} image")
        assert_close(g.pixels, s.pixels, f"{what} mode {mode} pixels")
        assert_bitwise(g.normals, s.normals, f"{what} mode {mode} normals")
        assert_bitwise(g.depth, s.depth, f"{what} mode {mode} depth")
        out = (g, s, img)
    return out


@pytest.mark.parametrize("W,H", [(40, 5), (17, 5)])
def test_partial_pools(W, H):
    """spp 16: pools of 16 pixels; W is no multiple of 16, so pools straddle row ends and the last
    pool holds 8 / 5 pixels (total = 128 / 80 < 256: one chunk of the sort is partial, two are empty)."""
    check(make_header(f"syn{SORT_MIN + 8}", W, H, 16), W, H, what=f"{W}x{H}")


@pytest.mark.parametrize("spp,W,H", [(1, 40, 13), (3, 40, 7), (4, 40, 6), (16, 24, 5), (64, 9, 3), (256, 3, 2)])
def test_samples_per_pixel(spp, W, H):
    """spp 1: 256 pixels per pool; 3: NS = 255, no multiple of 64; 4, 16, 64: the constant-spp
    instantiations; 256: one pixel per pool, item 255 in a byte.  Frame sizes with a partial last pool."""
    check(make_header(f"syn{SORT_MIN + 8}", W, H, spp), W, H, what=f"spp {spp}")


@pytest.mark.parametrize("scene", [f"syn{SORT_MIN - 1}", f"syn{SORT_MIN}", "syn64", "syn65", "syn129", "syn200", f"syn{SORT_MIN + 8}p"])
def test_scene_sizes(scene):
    """Just below and at the sort's sphere-count threshold; 64 and 65 spheres (one and two words);
    129 and 200 (the word-by-word pre-test instantiations); one scene with a plane (unsorted)."""
    check(make_header(scene, 40, 9, 16), 40, 9, what=scene)


def test_emissive_first_hits():
    """A large emissive sphere in front: first hits that write no normal / depth (the stale branch),
    3 frames so the slots are reused."""
    W, H = 40, 9
    h = make_header(f"syn{SORT_MIN + 8}", W, H, 16)
    h.pack_sphere(1, (0.0, 1.0, 4.0), 3.0, (3.0, 3.0, 2.5), emissive=True)
    h.set_mode(0, SORT_MIN + 8)
    check(h, W, H, frames=3, what="emissive")


def test_mirror_surfaces():
    """reflectivity < 0.999: the bounce direction is reflect(dir) + r * hemi, not hemi + n, so the
    octants are a poor guide to the directions; the result must not care."""
    W, H = 40, 9
    h = make_header(f"syn{SORT_MIN + 8}", W, H, 16)
    h.pack_sphere(0, (0.0, -35.0, 0.0), 33.0, (0.8, 0.6, 0.2), reflectivity=0.5)
    for i, (c, r) in enumerate([((-4.0, 0.5, 2.0), 2.0), ((3.0, 1.0, 0.0), 2.5), ((0.0, 4.0, -3.0), 3.0)]):
        h.pack_sphere(1 + i, c, r, (0.9, 0.9, 0.9), reflectivity=0.1 + 0.2 * i)
    h.set_mode(0, SORT_MIN + 8)
    check(h, W, H, what="mirror")


def far_header(spp, W, H):
    """SORT_MIN spheres, all far outside the view."""
    h = Header.synthetic(SORT_MIN, spp, 1234, aspect_for(W, H))
    for i in range(SORT_MIN):
        h.pack_sphere(i, (1000.0 + 3.0 * i, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5))
    h.set_mode(0, SORT_MIN)
    return h


def test_every_pool_culled():
    W, H = 40, 5
    g, s, img = check(far_header(16, W, H), W, H, what="culled")
    assert not s.normals.any()  # no primary hit anywhere


def test_silhouette_pool():
    """A small sphere between pixel centres: every unjittered ray of its pool misses, a jittered
    sample hits (the pool has live paths, none of them at a pixel centre)."""
    W, H = 16, 4
    h = far_header(16, W, H)
    bg = run_both(h, W, H, 2, 1)[2]
    h.pack_sphere(0, (0.3, -0.3, 0.0), 0.2, (0.7, 0.3, 0.2))
    h.set_mode(0, SORT_MIN)
    g, s, img = check(h, W, H, frames=1, modes=(2,), what="silhouette")
    assert not s.normals.any() and (img != bg).any()


def test_pool_with_one_live_path():
    """spp 1, 16 x 16 = one pool of 256 pixels; one small sphere on the view axis is hit by the
    centre pixel alone."""
    W = H = 16
    h = far_header(1, W, H)
    h.pack_sphere(0, (0.0, 0.0, 0.0), 0.2, (0.7, 0.3, 0.2))
    h.set_mode(0, SORT_MIN)
    g, s, img = check(h, W, H, frames=1, what="one path")
    assert int((np.abs(s.normals[0][..., :3]).sum(-1) > 0).sum()) == 1


def test_multi_frame_launch_and_ring_wrap():
    """Mode 2 with 3 frames per launch (each frame of the launch has its own blocks and result
    slots), and mode 1 over 10 frames, so the 8-slot ring wraps."""
    W, H = 40, 9
    h = make_header(f"syn{SORT_MIN + 8}", W, H, 16)
    r = Renderer(W, H, h.S, h.AA)
    r.set_frame_batch(3)
    hg, ho = h.copy(), h.copy()
    drv = FrameDriver(r, hg, 2, light_movement=True)
    drv.compute_many(3)
    s = SSBO(ho, W, H)
    d = oracle.dims(W, H, h.S, h.AA)
    img = np.zeros((H, W, 4), np.float32)
    fo = 0
    for k in range(3):
        ho.fill_rand_buffer(7000 + k)
        ho.set_mode(fo, ho.num_objects)
        s.set_header(ho)
        fo = oracle.dispatch(s.data, d, 2, fo, img)
    g = r.download()
    r.close()
    assert drv.frame_num == fo
    assert_close(g.image, img, "multi-frame image")
    assert_bitwise(g.normals, s.normals, "multi-frame normals")
    assert_bitwise(g.depth, s.depth, "multi-frame depth")
    check(h, W, H, frames=10, modes=(1,), what="ring")


def test_sort_on_off_identity():
    """The default build against the RT_B1_SORT=0 build in one process (tools/ab.py --libs), config
    (d) cropped to a strip of 64 rows across the middle of the frame: image, normals and depth
    bit-identical, the same samples and segments, fewer executed lane tests with the sort."""
    off, on = "build/v_b1sort0/librtrt.so", "real_time_ray_tracer_amd/librtrt.so"
    assert (ROOT / off).exists(), "make b1sort0 (build() does) builds the RT_B1_SORT=0 library"
    p = subprocess.run([sys.executable, "tools/ab.py", "--config", "d", "--rows", "1048:1112", "--all-counters", "--rounds", "1",
                        "--frames", "3", "--libs", f"{off},{on}"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count("identical=True") == 2 and "identical=False" not in p.stdout, p.stdout
    c = json.loads(p.stdout.strip().splitlines()[-1])["counters_by_variant"]
    print({k: (v["samples"], v["segments"], v["executed_lane_tests"]) for k, v in c.items()})
    assert c[on]["samples"] == c[off]["samples"] > 0
    assert c[on]["segments"] == c[off]["segments"] > 0
    assert c[on]["executed_lane_tests"] < c[off]["executed_lane_tests"]
