"""The cached AO kernels deal a pool's samples by sectors around the pool's cached surface normal
(the sort frames that cull_fill_kernel keeps in front of the cull masks) and leave a sky pool before
anything is copied to LDS.  Neither can change a result: a sample's path depends on its item only.
Every case renders the same frames with rt_set_cull_cache on and off; image, pixels, normals and
depth must be equal bit for bit, and the stats must show cached launches (six still frames: frames
0 and 1 run the in-kernel cull, frames 2..5 load the table).  Shapes are the smallest at which the
frame table's index, the centre ray or the early exit can go wrong, never the workload's."""
import numpy as np
import pytest

from real_time_ray_tracer_amd import Header, Renderer, aspect_for
from test_gpu_cull_cache import render, same
from test_gpu_parity import make_header

pytestmark = pytest.mark.gpu

CAM = 4  # RT_HDR_CAMERA_LOCATION (include/rt/layout.h)
N = 48   # kB1SortMinObj: the least spheres of a sorted scene


def pools_of(W, rows, spp):
    tp = max(1, 256 // spp)
    return (W * rows + tp - 1) // tp


def both(h, W, H, frames=6, cached=4, framed=True, trace_rows=None, **kw):
    """On against off; returns the cached run.  framed: the table holds the pools' sort frames."""
    fb = []
    on = render(h, W, H, frames, True, after=lambda k, r: fb.append(r.cull_cache_frame_bytes()), **kw)
    off = render(h, W, H, frames, False, **kw)
    same(on, off, f"{W}x{H}")
    assert off[1]["cached_launches"] == 0 and off[1]["fills"] == 0
    assert on[1]["cached_launches"] == cached, on[1]
    want = 32 * pools_of(W, trace_rows or H, h.AA) if framed else 0
    assert fb[-1] == want, (fb, want)
    return on


def far_header(spp, W, H, n=N):
    """n spheres, all far outside the view."""
    h = Header.synthetic(n, spp, 1234, aspect_for(W, H))
    for i in range(n):
        h.pack_sphere(i, (1000.0 + 3.0 * i, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5))
    h.set_mode(0, n)
    return h


def world_xy(h, W, H, px, py):
    """Where the centre ray of pixel (px, py) meets the plane z = 0 (the synthetic camera looks down -z)."""
    hor, ver, llc, cam = (h.vec4(i) for i in (1, 2, 3, CAM))
    d = llc[:3] + np.float32(px / W) * hor[:3] + np.float32(py / H) * ver[:3]
    t = -cam[2] / d[2]
    return float(cam[0] + t * d[0]), float(cam[1] + t * d[1])


@pytest.mark.parametrize("spp", [1, 4, 16, 64, 256])
@pytest.mark.parametrize("scene", ["syn48", "syn64", "syn129", "syn200"])
@pytest.mark.parametrize("W,H", [(40, 6), (64, 16)])
def test_scenes_and_sample_counts(W, H, scene, spp):
    """One to four mask words, the LDS-table and word-by-word forms, every constant-spp form and
    the run-time ones (spp 1, 256); 40 x 6: pools straddle row ends and the last pool is partial."""
    both(make_header(scene, W, H, spp), W, H)


@pytest.mark.parametrize("mode", [1, 2])
def test_strip(mode):
    """rows (5, 11) of a 64 x 16 frame: trace_row0 = 4, 8 traced rows; the centre ray's y is the frame's."""
    both(make_header("syn64", 64, 16, 16), 64, 16, rows=(5, 11), mode=mode, trace_rows=8)


@pytest.mark.parametrize("W,H,spp", [(17, 5, 16), (40, 5, 16), (9, 3, 64), (40, 13, 1)])
def test_row_ends_and_partial_last_pool(W, H, spp):
    """17 x 5: every pool straddles a row end, the last holds 5 pixels (its middle pixel is pixel 2);
    40 x 5: 8 pixels; 9 x 3 at spp 64: pools of 4 pixels, the last of 3; 40 x 13 at spp 1: pools of
    256 pixels over 6.4 rows, the middle pixel several rows above the pool's first."""
    both(make_header("syn56", W, H, spp), W, H)


def test_centre_ray_misses_in_every_pool_with_a_hit():
    """One small sphere on the centre ray of pixel (32, 2) of a 64 x 4 frame, the first pixel of its
    pool: no pool's middle pixel (pixel 8 of 16) sees it, so every frame is built on the reversed ray."""
    W, H = 64, 4
    h = far_header(16, W, H)
    x, y = world_xy(h, W, H, 32, 2)
    h.pack_sphere(0, (x, y, 0.0), 0.3, (0.7, 0.3, 0.2))
    h.set_mode(0, N)
    on = both(h, W, H, mode=2)
    hit = np.argwhere(np.abs(on[0].normals[..., :3]).sum(-1).max(0) > 0)  # [W][R] over the slots
    assert hit.size and all(int(px) % 16 != 8 for px, _ in hit), hit


@pytest.mark.parametrize("mode", [1, 2])
def test_all_sky(mode):
    """Every pool leaves at the early exit, in every cached frame."""
    on = both(far_header(16, 40, 6), 40, 6, mode=mode)
    assert not on[0].normals.any()


@pytest.mark.parametrize("mode", [1, 2])
def test_sky_pool_between_two_hit_pools(mode):
    """48 x 3, pools of 16 pixels: spheres in front of pixels 6 and 41 of row 1, six pixels and more
    from the middle pool, whose cone keeps neither."""
    W, H = 48, 3
    h = far_header(16, W, H)
    for i, px in enumerate((6, 41)):
        x, y = world_xy(h, W, H, px, 1)
        h.pack_sphere(i, (x, y, 0.0), 0.6, (0.7, 0.3 + 0.3 * i, 0.2))
    h.set_mode(0, N)
    on = both(h, W, H, mode=mode)
    n = np.abs(on[0].normals[..., :3]).sum(-1).max(0)  # [W][R]
    assert n[:16].any() and n[32:].any() and not n[16:32].any()


def test_emissive_first_hits():
    W, H = 40, 9
    h = make_header("syn56", W, H, 16)
    h.pack_sphere(1, (0.0, 1.0, 4.0), 3.0, (3.0, 3.0, 2.5), emissive=True)
    h.set_mode(0, 56)
    both(h, W, H)


def test_mirror_surfaces():
    """reflectivity < 0.999: the bounce direction is reflect(dir) + r * hemi, the sectors guide little."""
    W, H = 40, 9
    h = make_header("syn56", W, H, 16)
    h.pack_sphere(0, (0.0, -35.0, 0.0), 33.0, (0.8, 0.6, 0.2), reflectivity=0.5)
    for i, (c, r) in enumerate([((-4.0, 0.5, 2.0), 2.0), ((3.0, 1.0, 0.0), 2.5), ((0.0, 4.0, -3.0), 3.0)]):
        h.pack_sphere(1 + i, c, r, (0.9, 0.9, 0.9), reflectivity=0.1 + 0.2 * i)
    h.set_mode(0, 56)
    both(h, W, H)


def test_nan_rows_in_the_sphere_table():
    """A rectangle among the spheres: its sphere-table row is NaN (it is no plane, so the scene is
    cached): never hit, by the kernels or by the fill's centre ray, whichever mask bit it has."""
    W, H = 40, 6
    h = make_header("syn64", W, H, 16)
    h.pack_rectangle(3, (4, 6, 4), (0, 0, -8), (-8, 0, 0), (1.5, 1.5, 1.5), emissive=True)
    h.set_mode(0, 64)
    both(h, W, H)


def test_multi_frame_launches_across_the_ring_wrap():
    """Mode 2, 8 frames per launch, four launches: 32 frames through the 8-slot ring; launches 2 and
    3 read the table, every frame of a launch the same rows."""
    W, H = 40, 12
    h0 = make_header("syn64", W, H, 16)
    out = []
    for cache in (True, False):
        r = Renderer(W, H, h0.S, h0.AA)
        r.set_frame_batch(8)
        if not cache:
            r.set_cull_cache(False)
        h = h0.copy()
        f = 0
        for k in range(4):
            f = r.compute_frames(h, 2, f, 8, rand_seed=7000 + 8 * k)
        out.append((r.download(), r.cull_cache_stats(), None))
        fb = r.cull_cache_frame_bytes()
        r.close()
        assert fb == (32 * pools_of(W, H, 16) if cache else 0)
    same(out[0], out[1], "multi-frame")
    assert out[0][1]["fills"] == 1 and out[0][1]["cached_launches"] == 2


def test_camera_nudge_refills_the_frames():
    """Eight frames, the camera moves between frames 3 and 4: frames 2, 3 cached, 4 and 5 in-kernel,
    frame 6 refills masks and frames (after the last readers' events), 6 and 7 cached."""
    def mutate(k, h):
        if k == 4:
            h.vec4(CAM)[0] += np.float32(0.75)
    on = both(make_header("syn64", 40, 12, 16), 40, 12, frames=8, cached=4, mutate=mutate)
    assert on[1]["fills"] == 2


@pytest.mark.parametrize("cap,cached,table", [(1024, 4, 512), (2048 + 511, 4, 512), (2048 + 512, 4, 512), (511, 0, 0)])
def test_cap_keeps_masks_only(cap, cached, table):
    """64 x 16 at spp 16: 64 pools, 512 bytes of masks and 2048 of frames.  A cap between the two
    sums keeps the masks and the octant key; a cap of exactly the sum keeps both; under the masks'
    size nothing is cached."""
    W, H = 64, 16
    framed = cap >= 2048 + 512
    on = both(make_header("syn64", W, H, 16), W, H, cached=cached, framed=framed,
              toggle=lambda k, r: r.debug_cull_cache_cap(cap) if k == 0 else None)
    assert on[1]["table_bytes"] == table
