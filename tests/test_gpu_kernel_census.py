"""The kernel census on the GPU: every scenario of tests/kernel_forms.py with the launch log on
(rt_debug_launch_log).  A scenario passes when

  (1) the logged forms equal the table's sequence: the launch took the kernel the row claims, in the
      order it claims (two uncached launches, the fill, the cached form), not a fallback;
  (2) the outputs equal the reference as everywhere in this suite: normals and depth bit for bit,
      pixels and image within the north-star tolerance, against the C oracle (oracle.dispatch), or
      against the numpy restatement with the rectangle rule installed where a rectangle is in effect
      (as tests/test_gpu_rectangles.py); the Phong g-buffer against phong_gbuffer_cases.expectation,
      with a rectangle against the host closest-hit form;
  (3) a multi-frame scenario also equals, bit for bit, the same frames launched one per call;
  (4) the queries, presents, layout conversion and math self-test equal their host specifications.

The last test holds the union of every scenario's log against the library's symbols (nm).
"""
import numpy as np
import pytest

import kernel_forms as kf
import oracle
import phong_gbuffer_cases as pg
import present_values as pv
import ray_query_cases as rq
import rect_cases as rc
from conftest import assert_bitwise, assert_close
from oracle import numpy_ref
from real_time_ray_tracer_amd import (SSBO, Renderer, RtError, _lib, occluded_host, pixel_rays_host, quantize_rgba8,
                                      resample_rgba8, trace_rays_host)

pytestmark = pytest.mark.gpu

SEEN: set = set()   # every form any scenario of this module logged
RAN: list = []      # the scenarios that ran


@pytest.fixture(scope="module", autouse=True)
def rule_installed():
    """numpy_ref intersects shape id 3 by the rule for this module's tests, and only for them."""
    mp = pytest.MonkeyPatch()
    rc.install(mp)
    yield
    mp.undo()


def renderer(sc, h, **kw) -> Renderer:
    r = Renderer(sc.W, sc.H, h.S, h.AA, max_depth=sc.D, **kw)
    if sc.rects:
        r.set_rectangles(True)
    if sc.gbuf:
        r.set_phong_gbuffer(True)
    if sc.cap:
        r.debug_cull_cache_cap(sc.cap)
    if sc.counters:
        r.enable_counters(True, rows=True)
    return r


def take_log(sc, r: Renderer):
    """(1), and the log off again so that the downloads that follow record nothing."""
    log = r.launch_log(reset=True)
    r.set_launch_log(False)
    SEEN.update(log)
    RAN.append(sc.id)
    assert log == list(sc.forms), f"{sc.id}: launched {log}, the table says {list(sc.forms)}"


class Reference:
    """The oracle (or, with a rectangle in effect, the numpy restatement) over the same headers."""

    def __init__(self, sc, h):
        self.sc, self.h = sc, h.copy()
        self.s = SSBO(self.h, sc.W, sc.H)
        self.img = np.zeros((sc.H, sc.W, 4), np.float32)
        self.f = 0

    def frame(self, k):
        sc, h = self.sc, self.h
        if sc.mode in (1, 2):
            h.fill_rand_buffer(7000 + k)
        else:
            h.moving_light(True)
        h.set_mode(self.f, h.num_objects)
        self.s.set_header(h)
        if sc.rects:
            self.f = numpy_ref.dispatch(self.s.data, sc.W, sc.H, h.S, h.AA, sc.mode, self.f, self.img, D=sc.D)
        else:
            self.f = oracle.dispatch(self.s.data, oracle.dims(sc.W, sc.H, h.S, h.AA, D=sc.D), sc.mode, self.f, self.img)


def render(sc, h, r: Renderer, batch: int) -> int:
    """The scenario's frames on r: frame by frame (upload, dispatch), or rt_compute_frames with the
    frame batch `batch`, sc.calls calls of sc.frames frames.  Returns the next frame slot."""
    hh = h.copy()
    f = 0
    if not batch:
        for k in range(sc.frames):
            if sc.mode in (1, 2):
                hh.fill_rand_buffer(7000 + k)
            else:
                hh.moving_light(True)
            hh.set_mode(f, hh.num_objects)
            r.upload_header(hh)
            f = r.dispatch(sc.mode, f)
        return f
    r.set_frame_batch(batch)
    for k in range(sc.calls):
        f = r.compute_frames(hh, sc.mode, f, sc.frames, rand_seed=7000 + sc.frames * k, light_movement=True)
    return f


def gbuffer_expectation(sc, h):
    """(normals, depth) [W][H][4] of a Phong g-buffer slot (2)."""
    if not sc.rects:
        return pg.expectation(h, sc.W, sc.H)
    xy = rq.all_pixels(sc.W, sc.H)  # x-major, as the g-buffer
    o, d = pixel_rays_host(h, sc.W, sc.H, xy)
    want = trace_rays_host(h, o, d, 0.0 if sc.mode == 3 else 0.001, rectangles=True)
    hit, n = want.ind >= 0, len(xy)
    assert (want.ind == h.num_objects - 1).sum() > 20, "the rectangle is in view"
    nrm = np.where(hit[:, None], np.concatenate([want.normals, np.ones((n, 1), np.float32)], 1), np.float32(0))
    dep = np.where(hit[:, None], np.stack([want.t, np.zeros(n), np.zeros(n), np.ones(n)], 1), np.float32(0))
    return nrm.astype(np.float32).reshape(sc.W, sc.H, 4), dep.astype(np.float32).reshape(sc.W, sc.H, 4)


def run_frames(sc):
    """The ao and shade scenarios."""
    h = kf.make_scene(sc.scene, sc.W, sc.H, sc.spp)
    if sc.rects:
        rc.assert_no_grazing_root(h, sc.W, sc.H)
    ref = Reference(sc, h)
    total = sc.frames * (sc.calls if sc.batch else 1)
    for k in range(total):
        ref.frame(k)
    with renderer(sc, h) as r:
        r.set_launch_log(True)
        f = render(sc, h, r, sc.batch)
        take_log(sc, r)
        g = r.download()
    assert f == ref.f
    what = sc.id
    assert_close(g.image, ref.img, f"{what}: image")
    assert_close(g.pixels, ref.s.pixels, f"{what}: pixels")
    if sc.kind == "ao":
        assert g.normals.any() and g.depth.any(), f"{what}: nothing was hit"
        assert_bitwise(g.normals, ref.s.normals, f"{what}: normals")
        assert_bitwise(g.depth, ref.s.depth, f"{what}: depth")
    else:
        assert (g.image[..., :3] != g.image[0, 0, :3]).any(), f"{what}: a flat image"
        wn, wd = gbuffer_expectation(sc, h) if sc.gbuf else (0, 0)
        for slot in range(8):  # modes 3 and 4 write normals and depth only with the g-buffer on
            on = sc.gbuf and slot < total
            assert_bitwise(g.normals[slot], wn if on else np.zeros_like(g.normals[slot]), f"{what}: slot {slot} normals")
            assert_bitwise(g.depth[slot], wd if on else np.zeros_like(g.depth[slot]), f"{what}: slot {slot} depth")
    if sc.batch:  # (3)
        with renderer(sc, h) as one:
            assert render(sc, h, one, 1) == f
            g1 = one.download()
        for name in ("image", "pixels", "normals", "depth"):
            assert_bitwise(getattr(g, name), getattr(g1, name), f"{what}: {name}, one launch against one per frame")


def run_query(sc):
    h = kf.make_scene(sc.scene, sc.W, sc.H, sc.spp)
    with renderer(sc, h) as r:
        r.upload_header(h)
        if sc.tree:
            r.set_query_tree(True)
            assert r.query_tree_stats()["nodes"] > 0, f"{sc.id}: the scene has no tree"
        r.set_launch_log(True)
        if sc.kind == "occluded":
            a, b = rq.segment_set(h, 600)
            got = r.occluded(a, b)
            take_log(sc, r)
            want = occluded_host(h, a, b, rectangles=sc.rects)
            assert np.array_equal(got, want), f"{sc.id}: {int((got != want).sum())} of {len(a)} segments differ from the host"
            assert got.any() and not got.all()
            return
        if sc.kind == "rays":
            o, d = rq.aimed_set(h, 600)
            got = r.trace_rays(o, d, 1e-4)
            want = trace_rays_host(h, o, d, 1e-4, rectangles=sc.rects)
        else:
            xy = np.concatenate([rq.all_pixels(sc.W, sc.H), np.array([[-3, 5], [sc.W, sc.H], [1000, -77]], np.int32)])
            got = r.trace_pixels(xy, 0.0)
            o, d = pixel_rays_host(h, sc.W, sc.H, xy)
            want = trace_rays_host(h, o, d, 0.0, rectangles=sc.rects)
            assert_bitwise(got.dirs, d, f"{sc.id}: pixel rays")
        take_log(sc, r)
    assert np.array_equal(got.ind, want.ind), f"{sc.id}: ind differs at {np.flatnonzero(got.ind != want.ind)[:5]}"
    assert_bitwise(got.t, want.t, f"{sc.id}: t")
    assert_bitwise(got.normals, want.normals, f"{sc.id}: normals")
    assert (got.ind >= 0).any() and (got.ind < 0).any()
    if sc.rects:
        assert (got.ind == h.num_objects - 1).any(), f"{sc.id}: no ray hits the rectangle"


def run_present(sc):
    """One mode-1 frame, then the 8-bit blit of the image the context holds against the host rule."""
    h = kf.make_scene(sc.scene, sc.W, sc.H, sc.spp)
    ref = Reference(sc, h)
    ref.frame(0)
    with renderer(sc, h) as r:
        r.set_launch_log(True)
        render(sc, h, r, 0)
        if sc.kind == "present":
            got = r.image8(True)
        else:
            ow, oh = 67, 5
            got = r.image8_scaled(ow, oh, True)
        take_log(sc, r)
        held = r.image()
    assert_close(held, ref.img, f"{sc.id}: image")
    if sc.kind == "present":
        want = pv.quantize_ref(held, True)
        assert np.array_equal(want, quantize_rgba8(held, True))
    else:
        want = resample_rgba8(held, ow, oh, True)
    assert np.array_equal(got, want), f"{sc.id}: {int((got != want).sum())} bytes differ"
    assert (got[..., :3] != got[0, 0, :3]).any(), f"{sc.id}: a flat image"


def run_convert(sc):
    """rt_upload_gbuffer then rt_download: the three arrays go through the slots' plane layouts and
    come back bit for bit, NaN payloads and infinities included."""
    rng = np.random.default_rng(5)
    with Renderer(sc.W, sc.H, 1, 1) as r:
        shp = (r.F, sc.W, sc.H, 4)
        arrs = [rng.integers(0, 2 ** 32, shp, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(3)]
        r.set_launch_log(True)
        r.upload_gbuffer(*arrs)
        g = r.download(image=False)
        take_log(sc, r)
    for a, b, name in zip(arrs, (g.pixels, g.normals, g.depth), ("pixels", "normals", "depth")):
        assert a.tobytes() == b.tobytes(), f"{sc.id}: {name} changed on the way through the slots"


def run_selftest(sc):
    rng = np.random.default_rng(0)
    x = rng.uniform(-5e5, 5e5, 1000).astype(np.float32)
    v = np.concatenate([rng.uniform(0, 1e6, 1000), [0.0, 1e-45, np.inf, 3.4e38]]).astype(np.float32)
    ab = rng.uniform(-1e3, 1e3, (1000, 2)).astype(np.float32)
    with Renderer(8, 8, 1, 1) as r:
        r.set_launch_log(True)
        sin = r.selftest_math(_lib.RT_MATH_SIN, x, x.size)
        sq = r.selftest_math(_lib.RT_MATH_SQRT, v, v.size)
        dv = r.selftest_math(_lib.RT_MATH_DIV, ab, len(ab))
        take_log(sc, r)
    assert_bitwise(sin, oracle.det_sin(x), "det_sin")
    assert_bitwise(sq, np.sqrt(v), "sqrt")
    assert_bitwise(dv, ab[:, 0] / ab[:, 1], "div")


RUN = {"ao": run_frames, "shade": run_frames, "rays": run_query, "pixels": run_query, "occluded": run_query,
       "present": run_present, "present_scaled": run_present, "convert": run_convert, "selftest": run_selftest}


@pytest.mark.parametrize("sc", kf.SCENARIOS, ids=[s.id for s in kf.SCENARIOS])
def test_scenario(sc):
    try:
        RUN[sc.kind](sc)
    except RtError as e:
        if e.status == _lib.RT_E_HIP:  # a device error: the rest of the file would launch onto a dead context
            pytest.exit(f"{sc.id}: {e}; nothing more is launched in this process", returncode=3)
        raise


def test_every_kernel_of_the_library_ran():
    """The union of the logs of the scenarios above against the library's kernels (nm).  Meaningful only
    when the whole file ran: a selection of scenarios leaves kernels out by construction."""
    have = kf.library_kernels()
    assert len(RAN) == len(kf.SCENARIOS), (f"only {len(RAN)} of {len(kf.SCENARIOS)} scenarios ran: this test is "
                                           f"meaningful only when the whole file runs")
    assert SEEN == have, (f"kernels no scenario launched: {sorted(have - SEEN)}; launched forms that are no kernel "
                          f"of the library: {sorted(SEEN - have)}")
