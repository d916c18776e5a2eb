"""C-ABI library checks that need no GPU: it loads, exports every symbol include/rt/abi.h
declares, and its host-only helpers (loadShapeBuffer packing, camera basis, rand buffer,
moving light, scenes) produce the reference's SSBO layout."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from real_time_ray_tracer_amd import Header, _lib, aspect_for, header_floats, ssbo_floats


def declared_functions():
    text = (ROOT / "include" / "rt" / "abi.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"librtrt.so does not export {n}"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert lib.rt_version() == 1


def test_layout_matches_reference_instance():
    # reference ssbo_data: S=10, AA=4, 440x330, F=8 -> 1,040 B header, 55,757,840 B total
    assert header_floats(10, 4) * 4 == 1040
    assert ssbo_floats(10, 4, 440, 330, 8) * 4 == 55_757_840


def test_pack_sphere_plane_rectangle_layout():
    h = Header(10, 4)
    h.pack_sphere(0, (1, 2, 3), 4.0, (0.1, 0.2, 0.3), reflectivity=0.5, emissive=True)
    s = h.shapes[0]
    np.testing.assert_array_equal(s[0], [1, 2, 3, 4])
    assert s[1, 3] == 1.0 and s[3, 3] == 0.5
    np.testing.assert_array_equal(s[4], np.float32([0.1, 0.2, 0.3, 1]))
    h.pack_plane(1, (0, 2, 0), -4.0, (0.3, 0.0, 0.5))
    p = h.shapes[1]
    np.testing.assert_array_equal(p[0], [0, 1, 0, -4])          # normalize(normal), dist
    np.testing.assert_array_equal(p[3], [0, -8, 0, 1])          # p0 = dist * (unnormalised) normal
    assert p[4, 3] == 5.0
    h.pack_rectangle(2, (4, 6, 4), (0, 0, -8), (-8, 0, 0), (1.5, 1.5, 1.5), emissive=True)
    r = h.shapes[2]
    assert r[4, 3] == 3.0 and r[1, 3] == 1.0
    np.testing.assert_allclose(r[0, :3], [0, 1, 0], atol=1e-7)  # normalize(cross(right, up))
    with pytest.raises(_lib.RtError):
        h.pack_sphere(10, (0, 0, 0), 1, (1, 1, 1))


def test_camera_basis_default_pose():
    h = Header(1, 1)
    h.camera_basis((0, 0, 14), (0, 1, 0), (0, 0, 1), 1.333333)
    np.testing.assert_array_equal(h.vec4(1), np.float32([1.333333, 0, 0, 0]))
    np.testing.assert_array_equal(h.vec4(2), [0, 1, 0, 0])
    np.testing.assert_allclose(h.vec4(3), [-0.6666665, -0.5, -1, 0], rtol=1e-7)
    np.testing.assert_array_equal(h.vec4(4), [0, 0, 14, 0])


def test_rand_buffer_seeded_and_in_unit_interval():
    a, b = Header(4, 16), Header(4, 16)
    a.fill_rand_buffer(7000)
    b.fill_rand_buffer(7000)
    np.testing.assert_array_equal(a.rand_buffer, b.rand_buffer)
    assert a.rand_buffer.shape == (32, 4)
    assert (a.rand_buffer >= 0).all() and (a.rand_buffer < 1).all()
    b.fill_rand_buffer(7001)
    assert not np.array_equal(a.rand_buffer, b.rand_buffer)


def test_moving_light():
    h = Header(1, 1)
    h.moving_light(False)
    np.testing.assert_array_equal(h.vec4(5), [-12, 8, 7, 0])
    h.moving_light(True)
    np.testing.assert_array_equal(h.vec4(5), np.float32([-12, 8, 7, 0]) + np.float32(0.1))
    h.data[20] = 50.05
    h.moving_light(True)
    np.testing.assert_array_equal(h.vec4(5), [-50, 20, -50, 0])


def test_synthetic_scene_matches_survey_recipe():
    h = Header.synthetic(64, 16, 1234 + 3, aspect_for(3840, 2160))
    assert h.num_objects == 64
    s = h.shapes
    np.testing.assert_array_equal(s[0, 0], [0, -35, 0, 33])
    c = s[1:, 0]
    assert (c[:, 0] >= -12).all() and (c[:, 0] <= 12).all()
    assert (c[:, 1] >= -2).all() and (c[:, 1] <= 6).all()
    assert (c[:, 2] >= -20).all() and (c[:, 2] <= 4).all()
    assert (c[:, 3] >= 0.3).all() and (c[:, 3] <= 1.5).all()
    assert (s[:, 4, 3] == 1).all()
    refl = s[1:, 3, 3]
    assert ((refl == 1.0) | (refl <= 0.6)).all()
    np.testing.assert_array_equal(h.vec4(6), np.float32([13 / 255.0, 153 / 255.0, 219 / 255.0, 0]))
    h2 = Header.synthetic(64, 16, 1234 + 3, aspect_for(3840, 2160))
    np.testing.assert_array_equal(h.data, h2.data)


def test_builtin_scenes():
    for which, n in ((1, 5), (5, 3), (6, 6)):
        h = Header.builtin(which, 4)
        assert h.num_objects == n
    h1 = Header.builtin(1, 4)
    assert h1.shapes[4, 4, 3] == 5.0  # scene1's plane


def test_create_without_gpu_reports_nodev(gpu_available):
    if gpu_available:
        pytest.skip("a GPU is present")
    lib = _lib.load()
    cfg = _lib.rt_config(64, 48, 10, 4, 8, 20, 0, 0)
    ctx = C.c_void_p()
    assert lib.rt_create(0, C.byref(cfg), C.byref(ctx)) == _lib.RT_E_NODEV
    assert lib.rt_strerror(_lib.RT_E_NODEV) == b"no HIP device"


def _headless():
    import subprocess

    exe = ROOT / "build" / "rt_headless"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT), "headless"], check=True, capture_output=True)
    return exe


def test_c_driver_links_against_the_abi(gpu_available):
    """build/rt_headless is plain C++ over include/rt/abi.h + librtrt.so (the reference's own
    render loop without GL): it links and runs; without a GPU rt_create reports NODEV."""
    import subprocess

    if gpu_available:
        pytest.skip("covered by the GPU run")
    p = subprocess.run([str(_headless()), "--width", "64", "--height", "48", "--frames", "2"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "no HIP device" in p.stderr, (p.returncode, p.stderr)


def test_c_driver_strips_need_visible_devices(gpu_available):
    """rt_headless --strips without a visible device stops with a message (rt_device_count), and
    rt_group_create reports NODEV instead of building a group."""
    import subprocess

    if gpu_available:
        pytest.skip("covered by the GPU run (test_gpu_group.py::test_headless_refuses_missing_devices)")
    assert _lib.load().rt_device_count() == 0
    p = subprocess.run([str(_headless()), "--width", "64", "--height", "48", "--strips", "2", "--devices", "0,1"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "no HIP device is visible" in p.stderr, (p.returncode, p.stderr)
    cfg = _lib.rt_config(64, 48, 10, 4, 8, 20, 0, 0)
    g = C.c_void_p()
    devs = (C.c_int * 2)(0, 1)
    assert _lib.load().rt_group_create(2, devs, C.byref(cfg), None, C.byref(g)) == _lib.RT_E_NODEV


def pool_of_block(b: int, n: int, Q: int) -> int:
    """ao_batch_kernel's workgroup -> pool map (rt_kernels.hip, XCD-balanced pool order): row r's
    Q pools rotated by r; a trailing partial group keeps its order."""
    r = b // Q
    if (r + 1) * Q > n:
        return b
    c = b - r * Q + r % Q
    return r * Q + (c - Q if c >= Q else c)


@pytest.mark.parametrize("n,Q", [(518400, 240), (64800, 240), (8, 8), (100, 8), (1200, 16), (33, 8), (4000, 120)])
def test_pool_rotation_is_a_bijection(n, Q):
    m = [pool_of_block(b, n, Q) for b in range(n)]
    assert sorted(m) == list(range(n))


def test_pool_rotation_spreads_columns_over_xcds():
    """Blocks are dealt round-robin to 8 XCDs (b mod 8): with 240 pools per row, every XCD takes
    every pool-column residue mod 8 once per 8 rows (in plain row order it would always take the
    same residue)."""
    Q = 240
    for xcd in range(8):
        res = {pool_of_block(b, 8 * Q, Q) % Q % 8 for b in range(8 * Q) if b % 8 == xcd}
        assert res == set(range(8))


def post_tile_of_block(L: int, gx: int, gy: int, R: int) -> int:
    """post_kernel's workgroup -> tile map (rt_kernels_impl.h xcd_tile): runs of R tiles dealt
    round-robin to the 8 XCDs; a trailing partial round keeps its order."""
    n = gx * gy
    M = n // (8 * R) * (8 * R) if R else 0
    if L >= M:
        return L
    j = L >> 3
    return ((j // R) * 8 + (L & 7)) * R + j % R


def post_tile_run(W: int) -> int:
    """launch_params' choice of R for the post-process (the least R in [4, gx/16] dividing gx/8)."""
    gx = (W + 15) // 16
    if gx % 8 == 0:
        for r in range(4, gx // 16 + 1):
            if (gx // 8) % r == 0:
                return r
    return 4 if gx >= 32 else 0


@pytest.mark.parametrize("W,H", [(3840, 2160), (1920, 1080), (7680, 4320), (440, 330), (640, 480), (200, 150)])
def test_post_tile_order_is_a_bijection_with_xcd_local_neighbours(W, H):
    """The run map of xcd_tile as a function over arbitrary grids (here the grids 16 x 16 tiles
    would give), not the production geometry: a tile is 64 x 4 pixels now and launch_params prefers
    super-tiles, both restated and checked in tests/test_post_synthetic_cpu.py."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    R = post_tile_run(W)
    m = [post_tile_of_block(L, gx, gy, R) for L in range(gx * gy)]
    assert sorted(m) == list(range(gx * gy))
    if R and gx % 8 == 0 and (gx // R) % 8 == 0:
        xcd = {t: L % 8 for L, t in enumerate(m)}
        full = gx * gy // (8 * R) * (8 * R)
        # the tile below each tile of a full round is on the same XCD (vertical neighbour lines)
        same = [xcd[t] == xcd[t - gx] for t in range(gx, full)]
        assert all(same)
        # and every XCD takes the same number of tiles from every tile row
        for row in range(min(gy, full // gx)):
            counts = [sum(1 for c in range(gx) if xcd[row * gx + c] == k) for k in range(8)]
            assert len(set(counts)) == 1
