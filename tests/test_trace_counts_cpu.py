"""The counting references on their own (tests/trace_counts.py): the C oracle's per-pixel work planes
against the numpy restatement's, and against outputs and host functions that do not count.

numpy's emulated fmaf can differ from the C oracle's on a double-rounding tie, so every comparison of
the two first asserts that their g-buffers agree bit for bit on this input, and compares the planes of
every pixel only then.  Frames are at most 40 x 6 and scenes at most 64 shapes: numpy scans one shape
at a time."""
import numpy as np
import pytest

import oracle
import trace_counts as tc
from conftest import assert_close
from real_time_ray_tracer_amd import SSBO, Header, aspect_for, pixel_rays_host, trace_rays_host
from test_gpu_parity import make_header  # (a GPU test module; importing it needs no GPU)


def scene(name, W, H, spp):
    if name == "mirrors":
        return tc.facing_mirrors(W, H, spp)
    if name == "sky_between":
        return tc.sky_between(W, H, spp)
    if name == "syn64e":  # seed 99: every 16th sphere is an emitter
        return Header.synthetic(64, spp, 99, aspect_for(W, H))
    return make_header(name, W, H, spp)


def both(h, W, H, mode, D=20, frames=2):
    """`frames` frames of `mode` by both references on identical inputs: the g-buffers must agree
    bit for bit; returns each frame's (C planes, numpy planes)."""
    sc, sn = SSBO(h, W, H), SSBO(h, W, H)
    d = oracle.dims(W, H, h.S, h.AA, D=D)
    ic, inn = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    f, out = 0, []
    for k in range(frames):
        hk = h.copy()
        hk.fill_rand_buffer(7000 + k) if mode in (1, 2) else hk.moving_light(True)
        hk.set_mode(f, hk.num_objects)
        sc.set_header(hk)
        sn.set_header(hk)
        pn = tc.numpy_trace(sn, mode, f, inn, D=D)
        f, pc = tc.oracle_dispatch(sc, d, mode, f, ic)
        out.append((pc, pn))
    # the inputs qualify: no double-rounding tie steered the two restatements apart
    assert np.array_equal(sn.depth.view(np.uint32), sc.depth.view(np.uint32)), "pick another input"
    assert np.array_equal(sn.normals.view(np.uint32), sc.normals.view(np.uint32)), "pick another input"
    if mode != 1:  # (mode 1's C pixels are post-processed; numpy_trace ran the trace pass only)
        assert_close(sn.pixels, sc.pixels, "pixels")
    return out


CASES = [(s, m, 40, 6, 4, 20) for s in ("s1", "syn16", "syn16p", "planes", "empty", "mirrors") for m in (1, 2, 3, 4)]
CASES += [("syn64", 2, 40, 6, 16, 20), ("syn64", 2, 17, 5, 16, 20), ("syn64", 1, 40, 6, 16, 10), ("syn16", 2, 40, 7, 3, 20),
          ("syn64e", 2, 9, 3, 64, 20), ("sky_between", 2, 64, 6, 4, 20)]
CASES += [("mirrors", 4, 17, 5, 4, D) for D in (1, 3)] + [("mirrors", 4, 33, 17, 4, 20), ("s1", 3, 1, 1, 4, 20)]


@pytest.mark.parametrize("name,mode,W,H,spp,D", CASES)
def test_c_planes_equal_numpy_planes(name, mode, W, H, spp, D):
    h = scene(name, W, H, spp)
    frames = both(h, W, H, mode, D)
    per = tc.samples_per_pixel(mode, spp)
    for k, (pc, pn) in enumerate(frames):
        for key in ("segs", "shadows", "single"):
            c, n = getattr(pc, key), getattr(pn, key)
            assert c.shape == (H, W) and np.array_equal(c, n), f"frame {k} {key}: {np.argwhere(c != n)[:4]}"
        # what any count of this algorithm satisfies
        assert (pc.segs >= per).all() and (pc.segs <= per * D).all() and (pc.single <= per).all()
        assert (pc.shadows <= pc.segs).all() if mode in (3, 4) else not pc.shadows.any()
    if name == "mirrors" and mode == 4:
        assert pc.segs.max() == D and pc.segs.min() == 1, "some paths run all D segments, some stop at once"
    if name == "sky_between":
        q = W // 4
        assert (pc.segs[:, q:3 * q] == spp).all() and pc.segs[:, :q].max() > spp and pc.segs[:, 3 * q:].max() > spp


@pytest.mark.parametrize("name,D", [("mirrors", 20), ("syn64e", 3), ("syn64e", 20), ("s1", 1)])
def test_ao_segments_are_the_stop_depth_plus_one(name, D):
    """spp 1: depth.y, which the oracle has always produced, records at which segment the pixel's one
    path stopped (D - depth, ao_compute.glsl:163-258): on a miss or an emitter.  There segs is
    depth.y + 1; a path that never stopped ran all D.  A path stops at its first segment on a miss
    (zeros stored, normals.w = 0) or on an emitter (nothing but depth.y stored: normals.w keeps what
    was there); after a first hit (normals.w = 1, depth.y = 0) a later stop stores depth.y >= 1."""
    W, H = 40, 6
    h = scene(name, W, H, 1)
    h.fill_rand_buffer(7001)
    s = SSBO(h, W, H)
    s.normals[0][..., 3] = -7.0
    d = oracle.dims(W, H, h.S, 1, D=D)
    _, p = tc.oracle_dispatch(s, d, 2, 0, np.zeros((H, W, 4), np.float32))
    nw, dy = s.normals[0][..., 3].T, s.depth[0][..., 1].T  # [H][W]
    assert np.isin(nw, (-7.0, 0.0, 1.0)).all()
    stopped = (nw != 1.0) | (dy >= 1.0)
    assert np.array_equal(p.segs[stopped], dy[stopped].astype(np.int64) + 1)
    assert (p.segs[~stopped] == D).all()
    assert np.array_equal(p.single, (p.segs == 1).astype(np.int64)) and not p.shadows.any()
    if D == 20:
        assert stopped.any() and (nw == 1.0).any()
    if name == "syn64e":
        assert (nw == -7.0).any(), "no primary ray ends on an emitter: pick another scene"
    if name == "mirrors":
        assert (~stopped).any(), "no path runs all D segments: pick another scene"


@pytest.mark.parametrize("name", ["s1", "syn16", "syn16p", "manyplanes", "empty"])
@pytest.mark.parametrize("W,H", [(40, 6), (17, 5)])
def test_mode_3_casts_one_shadow_ray_per_primary_hit(name, W, H):
    """rt_pixel_rays_host and rt_trace_rays_host (the ray queries' host specification, which counts
    nothing) at mode 3's threshold 0: a pixel has a shadow ray iff its ray has a hit."""
    h = scene(name, W, H, 4)
    s = SSBO(h, W, H)
    _, p = tc.oracle_dispatch(s, oracle.dims(W, H, h.S, h.AA), 3, 0)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    o, dirs = pixel_rays_host(h, W, H, np.stack([xs.ravel(), ys.ravel()], 1))
    hit = trace_rays_host(h, o, dirs, thr=0.0).ind.reshape(H, W) >= 0
    assert np.array_equal(p.shadows, hit.astype(np.int64))
    assert (p.segs == 1).all() and (p.single == 1).all()
    assert hit.any() != (name == "empty")


@pytest.mark.parametrize("name", ["s1", "syn16", "mirrors"])
def test_mode_4_at_depth_1_counts_as_mode_3(name):
    """One hybrid segment is Phong's: the same loop and shadow ray (the thresholds, 0.001 and 0,
    differ, which no primary ray of these scenes can tell: they start outside every shape)."""
    W, H = 40, 6
    h = scene(name, W, H, 4)
    d1 = oracle.dims(W, H, h.S, h.AA, D=1)
    _, p4 = tc.oracle_dispatch(SSBO(h, W, H), d1, 4, 0)
    _, p3 = tc.oracle_dispatch(SSBO(h, W, H), d1, 3, 0)
    assert p4.same(p3) and p3.shadows.any()


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_no_objects(mode):
    """set_mode(0, 0): every sample is one empty scene loop, and no shadow ray."""
    W, H, spp = 17, 5, 3
    h = make_header("s1", W, H, spp)
    h.fill_rand_buffer(7000)
    h.set_mode(0, 0)
    _, p = tc.oracle_dispatch(SSBO(h, W, H), oracle.dims(W, H, h.S, h.AA), mode, 0)
    per = tc.samples_per_pixel(mode, spp)
    assert (p.segs == per).all() and (p.single == per).all() and not p.shadows.any()
    assert tc.totals(p, 0, per) == {"samples": W * H * per, "segments": W * H * per, "shadow_rays": 0, "tests": 0}


def test_a_band_and_a_window_write_their_own_entries():
    """gy0 / gh bands (row 0 of the planes = gy0) and column windows: the whole frame's entries, and
    nothing outside the window."""
    W, H = 40, 16
    h = make_header("syn16", W, H, 4)
    h.fill_rand_buffer(7000)
    for mode in (2, 4):
        _, whole = tc.oracle_dispatch(SSBO(h, W, H), oracle.dims(W, H, h.S, h.AA), mode, 0)
        band = oracle.dims(W, H, h.S, h.AA, gy0=4, gh=8)
        sb = np.zeros(h.data.size + 3 * 8 * W * 8 * 4, np.float32)
        sb[:h.data.size] = h.data
        planes = [np.full((8, W), 77, np.uint32) for _ in range(3)]
        oracle.run_program(sb, band, tc.OPROG[mode], 0, None, 5, 11, x0=3, x1=30, segs=planes[0], shadows=planes[1],
                           single=planes[2])
        for got, want in zip(planes, (whole.segs, whole.shadows, whole.single)):
            assert np.array_equal(got[1:7, 3:30], want[5:11, 3:30])
            got[1:7, 3:30] = 77
            assert (got == 77).all()


def test_the_helpers_arithmetic():
    """executed_lane_tests and ao_row_bounds on planes small enough to do by hand."""
    w = np.zeros((9, 10), np.int64)
    w[0, 0], w[7, 7], w[0, 8], w[8, 9] = 3, 5, 2, 4  # tiles: (rows 0-7, cols 0-7) max 5; (0-7, 8-9) 2; (8, 0-7) 0; (8, 8-9) 4
    p = tc.Planes(w, np.zeros_like(w), np.zeros_like(w))
    assert tc.executed_lane_tests(p, 7) == 64 * 7 * (5 + 2 + 0 + 4)
    assert tc.executed_lane_tests(tc.Planes(w, w, w), 7) == 2 * 64 * 7 * (5 + 2 + 0 + 4)
    # one row, two pixels, spp 3: samples of (1, 1, 4) and (2, 3, 1) loops
    p = tc.Planes(np.array([[6, 6]]), np.zeros((1, 2), np.int64), np.array([[2, 1]]))
    lo, hi = tc.ao_row_bounds(p, 10, 3)
    assert lo[0] == (1 + 1 + 24 + 2 * 10) + (24 + 24 + 10 + 1) and hi[0] == 6 * 24 + 12 * 10
    assert list(tc.row_work(tc.Planes(w, w, w))[[0, 7, 8]]) == [10, 10, 8]
