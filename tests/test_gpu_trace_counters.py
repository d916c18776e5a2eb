"""The trace work counters (rt_read_counters slots 0-4, rt_read_row_counters) against an independent
count: the C oracle's per-pixel planes for the same header sequence (tests/trace_counts.py, kept honest
on its own by tests/test_trace_counts_cpu.py).  Every case asserts

  (a) the counted launch's image, pixels, normals and depth equal the uncounted launch's bit for bit
      (a second context, counters off, fed the same headers);
  (b) normals and depth equal the oracle's bit for bit where the mode writes them, colours within the
      suite's tolerance;
  (c) samples, segments, shadow_rays and tests equal the planes' totals;
  (d) modes 3 and 4: the row counters equal the rows' segs + shadows, and executed_lane_tests equals
      the helper's restatement of count_work;
  (e) modes 1 and 2: executed_lane_tests is a multiple of 64, non-zero iff segments is, and the same
      when the same frames are rendered again;
  (f) modes 1 and 2: every own row's counter lies between the row sums of the documented estimate's
      per-sample bounds (trace_counts.ao_row_bounds);
  (g) a second read after a reset returns zeros, and with the counters off a launch adds nothing.
"""
import numpy as np
import pytest

import oracle
import phong_gbuffer_cases as pg
import trace_counts as tc
from conftest import assert_bitwise, assert_close
from real_time_ray_tracer_amd import SSBO, Renderer
from test_gpu_parity import make_header

pytestmark = pytest.mark.gpu

TRACE_KEYS = ("samples", "segments", "shadow_rays", "tests")


def scene(name, W, H, spp):
    if name == "mirrors":
        return tc.facing_mirrors(W, H, spp)
    if name == "all_sky":
        return tc.all_sky(W, H, spp)
    if name == "sky_between":
        return tc.sky_between(W, H, spp)
    return make_header(name, W, H, spp)


def band(rows, H):
    """The rows a strip context holds: its own and one halo row on each side that exists."""
    return (0, H) if rows is None else (max(0, rows[0] - 1), min(H, rows[1] + 1))


def same_outputs(a: Renderer, b: Renderer, gbuf: bool, what: str):
    """(a): a and b hold the same image and ring, bit for bit.  Returns a's download."""
    ga, gb = a.download(), b.download()
    for name in ("image", "pixels") + (("normals", "depth") if gbuf else ()):
        assert_bitwise(getattr(ga, name), getattr(gb, name), f"{what}: counted vs uncounted {name}")
    return ga


def zeros_after(r: Renderer, mode: int, frame: int):
    """(g): the reads so far reset the counters, and a launch with the counters off adds nothing."""
    zero = dict.fromkeys(r.read_counters(), 0)
    assert r.read_counters() == zero and not r.read_row_counters().any()
    r.enable_counters(False, rows=False)
    r.dispatch(mode, frame)
    assert r.read_counters() == zero and not r.read_row_counters().any()


# ---- modes 3 and 4 ---------------------------------------------------------------------------
def check_phong(name, W, H, mode, gb, D=20, rows=None, batch=0):
    """Two frames with the moving light, one read per frame; batch > 0: three frames by one
    rt_compute_frames call with that frame batch, one read."""
    h = scene(name, W, H, 4)
    nobj = h.num_objects
    r0, r1 = rows if rows else (0, H)
    t0, t1 = band(rows, H) if gb else (r0, r1)  # the rows traced: a strip's halo rows only for the g-buffer
    s = SSBO(h, W, H)
    d = oracle.dims(W, H, h.S, h.AA, D=D)
    img = np.zeros((H, W, 4), np.float32)
    ctx = [Renderer(W, H, h.S, h.AA, max_depth=D, rows=rows) for _ in range(2)]
    counted, plain = ctx
    counted.enable_counters(True, rows=True)
    for r in ctx:
        r.set_phong_gbuffer(gb)
        if batch:
            r.set_frame_batch(batch)
    ho, hg = h.copy(), [h.copy(), h.copy()]
    fo, planes = 0, []
    frames = 3 if batch else 2
    for k in range(frames):
        ho.moving_light(True)
        ho.set_mode(fo, nobj)
        s.set_header(ho)
        fo, p = tc.oracle_dispatch(s, d, mode, fo, img)
        planes.append(p.rows(t0, t1))
    got = []
    if batch:
        for r, hh in zip(ctx, hg):
            assert r.compute_frames(hh, mode, 0, frames, light_movement=True) == fo
        got.append((counted.read_counters(), counted.read_row_counters()))
        want = [planes[0] + planes[1] + planes[2]]
        lane = sum(tc.executed_lane_tests(p, nobj) for p in planes)
    else:
        f = 0
        for k in range(frames):
            for r, hh in zip(ctx, hg):
                hh.moving_light(True)
                hh.set_mode(f, nobj)
                r.upload_header(hh)
                nf = r.dispatch(mode, f)
            f = nf
            got.append((counted.read_counters(), counted.read_row_counters()))
        want = planes
        lane = None
    what = f"{name} {W}x{H} mode {mode} gb {gb} D {D} rows {rows}"
    for k, ((c, rc), p) in enumerate(zip(got, want)):
        exp = tc.totals(p, nobj, frames if batch else 1)  # (a batch's planes are its frames' sums)
        print(what, "frame", k, c, "expected", exp)
        assert {key: c[key] for key in TRACE_KEYS} == exp, f"{what} frame {k} (c)"
        assert np.array_equal(rc, tc.row_work(p.rows(r0, r1))), f"{what} frame {k} (d) rows: {rc}"
        assert c["executed_lane_tests"] == (lane if batch else tc.executed_lane_tests(p, nobj)), f"{what} frame {k} (d)"
        assert c["filtered_pixels"] == c["history_read"] == c["history_accepted"] == 0
    g = same_outputs(counted, plain, gb, what)
    assert_close(g.pixels, s.pixels[:, :, r0:r1], f"{what}: pixels")
    assert_close(g.image, img[r0:r1], f"{what}: image")
    if gb:
        exp_n, exp_d = pg.expectation(h, W, H)
        for slot in range(8):
            wn, wd = (exp_n, exp_d) if slot < frames else (np.zeros_like(exp_n), np.zeros_like(exp_d))
            assert_bitwise(g.normals[slot], wn[:, r0:r1], f"{what}: slot {slot} normals")
            assert_bitwise(g.depth[slot], wd[:, r0:r1], f"{what}: slot {slot} depth")
    zeros_after(counted, mode, 0)
    for r in ctx:
        r.close()
    return planes


@pytest.mark.parametrize("gb", [False, True], ids=["plain", "gbuf"])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("name", ["s1", "syn16", "manyplanes", "empty"])
@pytest.mark.parametrize("W,H", [(17, 5), (33, 17), (1, 1)])
def test_phong_and_hybrid_scenes(name, W, H, mode, gb):
    """17 x 5: partial tiles both ways, inactive lanes in every wave; 33 x 17: several blocks and a
    one-pixel last tile column and row; 1 x 1: one active lane."""
    check_phong(name, W, H, mode, gb)


@pytest.mark.parametrize("gb", [False, True], ids=["plain", "gbuf"])
@pytest.mark.parametrize("D", [1, 3, 20])
@pytest.mark.parametrize("W,H", [(17, 5), (33, 17)])
def test_hybrid_paths_of_every_length(W, H, D, gb):
    """Facing mirrors: lanes of one wave run 1, 2 and D segments."""
    planes = check_phong("mirrors", W, H, 4, gb, D=D)
    assert planes[0].segs.max() == D and planes[0].segs.min() == 1


@pytest.mark.parametrize("gb", [False, True], ids=["plain", "gbuf"])
@pytest.mark.parametrize("mode", [3, 4])
def test_phong_and_hybrid_strip(mode, gb):
    """Rows (5, 11) of 64 x 16: tiles start at row 5, or at the halo row 4 with the g-buffer on, when
    the totals include the two halo rows; the row counters are the own rows' either way."""
    check_phong("syn16", 64, 16, mode, gb, rows=(5, 11))
    check_phong("mirrors", 64, 16, mode, gb, rows=(5, 11))


@pytest.mark.parametrize("gb", [False, True], ids=["plain", "gbuf"])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("name,W,H", [("syn16", 33, 17), ("mirrors", 17, 5)])
def test_phong_and_hybrid_multi_frame_launch(name, W, H, mode, gb):
    """rt_compute_frames, three frames with the moving light in one launch (frame batch 8): the launch
    counts every frame, so totals, rows and lane-tests are the three frames' sums."""
    check_phong(name, W, H, mode, gb, batch=8)


# ---- modes 1 and 2 ---------------------------------------------------------------------------
def check_ao(name, W, H, mode, spp, D=20, rows=None, cached=(0, 0, 1, 2), pipelined=False, frames=4, more=None):
    """`frames` still frames, each with its own rand_buffer, on three contexts: counted, counted again,
    and uncounted.  A read after every frame (pipelined: one read at the end).  cached: the count of
    cached launches (rt_cull_cache_stats) after each frame, which says which form each frame ran.
    more(got, want): a case's own assertions on the counters read and the planes."""
    h = scene(name, W, H, spp)
    nobj = h.num_objects
    r0, r1 = rows if rows else (0, H)
    t0, t1 = band(rows, H)  # the AO programs trace a strip's halo rows
    s = SSBO(h, W, H)
    d = oracle.dims(W, H, h.S, h.AA, D=D)
    img = np.zeros((H, W, 4), np.float32)
    ctx = [Renderer(W, H, h.S, h.AA, max_depth=D, rows=rows) for _ in range(3)]
    counted, again, plain = ctx
    for r in ctx:
        if pipelined:
            r.enable_pipelining(True)
    for r in (counted, again):
        r.enable_counters(True, rows=True)
    hh = h.copy()
    f, got, want, seen = 0, [], [], []
    for k in range(frames):
        hh.fill_rand_buffer(7000 + k)
        hh.set_mode(f, nobj)
        s.set_header(hh)
        for r in ctx:
            r.upload_header(hh)
            nf = r.dispatch(mode, f)
        fo, p = tc.oracle_dispatch(s, d, mode, f, img)
        assert nf == fo
        f = nf
        want.append(p)
        seen.append(counted.cull_cache_stats()["cached_launches"])
        if not pipelined:
            got.append([(r.read_counters(), r.read_row_counters()) for r in (counted, again)])
    if pipelined:
        got.append([(r.read_counters(), r.read_row_counters()) for r in (counted, again)])
        total = want[0]
        for p in want[1:]:
            total = total + p
        want = [total]
    what = f"{name} {W}x{H} mode {mode} spp {spp} D {D} rows {rows}"
    assert seen == list(cached), f"{what}: cached launches after each frame {seen}"
    per = spp * (frames if pipelined else 1)
    lanes = []
    for k, (((c, rc), (c2, rc2)), p) in enumerate(zip(got, want)):
        traced = p.rows(t0, t1)
        exp = tc.totals(traced, nobj, per)
        lo, hi = tc.ao_row_bounds(p.rows(r0, r1), nobj, per)
        print(what, "frame", k, c, "expected", exp, "rows", rc, "in", lo, hi)
        assert {key: c[key] for key in TRACE_KEYS} == exp, f"{what} frame {k} (c)"
        assert c["executed_lane_tests"] % 64 == 0, f"{what} frame {k} (e)"
        assert c == c2 and np.array_equal(rc, rc2), f"{what} frame {k} (e): rendered again {c2} {rc2}"
        assert rc.shape == (r1 - r0,) and (lo <= rc).all() and (rc <= hi).all(), f"{what} frame {k} (f)"
        if mode == 2:
            assert c["filtered_pixels"] == c["history_read"] == c["history_accepted"] == 0
        lanes.append((c["executed_lane_tests"], c["segments"]))
    g = same_outputs(counted, plain, True, what)
    assert_bitwise(g.normals, s.normals[:, :, r0:r1], f"{what}: normals")
    assert_bitwise(g.depth, s.depth[:, :, r0:r1], f"{what}: depth")
    assert_close(g.pixels, s.pixels[:, :, r0:r1], f"{what}: pixels")
    assert_close(g.image, img[r0:r1], f"{what}: image")
    zeros_after(counted, mode, 0)
    for r in ctx:
        r.close()
    if more:
        more(got, want)
    for k, (lane, segments) in enumerate(lanes):
        assert (lane != 0) == (segments != 0), f"{what} frame {k} (e): {lane} executed lane-tests, {segments} segments"
    return got, want


# the rows of ao_select that a counted launch reaches: (scene, spp, W, H, D, cached launches per frame)
AO_FORMS = [
    ("syn16", 4, 40, 6, 20, (0, 0, 1, 2)),     # sppc 4, plain
    ("syn16", 16, 40, 6, 20, (0, 0, 1, 2)),    # CLON, unsorted
    ("syn16", 3, 40, 7, 20, (0, 0, 1, 2)),     # run-time spp
    ("syn64", 16, 40, 6, 20, (0, 0, 1, 2)),    # CLON | SORT: pools straddle row ends, the last is partial
    ("syn64", 16, 17, 5, 20, (0, 0, 1, 2)),
    ("syn64", 16, 40, 6, 10, (0, 0, 1, 2)),    # SORT, no CLON
    ("syn64", 8, 40, 6, 20, (0, 0, 1, 2)),     # run-time spp, SORT
    ("syn130", 64, 9, 3, 20, (0, 0, 1, 2)),    # CLON | SORT | WIDE
    ("syn130", 8, 40, 6, 20, (0, 0, 1, 2)),    # run-time spp, WIDE
    ("syn16p", 16, 40, 6, 20, (0, 0, 0, 0)),   # the three PL forms: a scene with planes is never cached
    ("syn16p", 4, 40, 6, 20, (0, 0, 0, 0)),
    ("syn16p", 3, 40, 6, 20, (0, 0, 0, 0)),
    ("syn150p", 16, 40, 6, 20, (0, 0, 0, 0)),  # PL | WIDE
]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name,spp,W,H,D,cached", AO_FORMS, ids=[f"{a[0]}-spp{a[1]}-{a[2]}x{a[3]}-D{a[4]}" for a in AO_FORMS])
def test_ao_forms(name, spp, W, H, D, cached, mode):
    """Frames 0 and 1 run the uncached form and frames 2 and 3 the AO_CULLC form of each row."""
    check_ao(name, W, H, mode, spp, D=D, cached=cached)


@pytest.mark.parametrize("mode", [1, 2])
def test_ao_all_sky(mode):
    """Every pool takes the empty-frustum shortcut: one segment per sample, and exactly spp per pixel
    in the rows (the lower bound of (f)).  The shortcut's own accounting of slot 4 is the cull that
    decided the pool's segments, 64 x its rounds of the wave (one round for 48 spheres) per pool: this
    test found it counting nothing, 0 executed lane-tests beside 3840 segments."""
    W, H, spp = 40, 6, 16

    def more(got, want):
        for ((c, rc), _), p in zip(got, want):
            assert (p.segs == spp).all() and c["segments"] == c["samples"] == W * H * spp
            assert (rc == W * spp).all(), rc
            assert c["executed_lane_tests"] == 64 * ((W * H + 15) // 16), c  # 15 pools of 16 pixels, one round each

    check_ao("all_sky", W, H, mode, spp, more=more)


@pytest.mark.parametrize("mode", [1, 2])
def test_ao_sky_pools_between_hit_pools(mode):
    """64 x 6 at spp 16: four pools of 16 pixels per row, spheres in the first and the last only.  The
    pixels of the two pools between them have segments == samples, and their pools take the shortcut
    in the same launch in which the others take the general path: a shortcut sample adds 1 to its row
    and a sample of the general path at least kSetupCost, so a row above W * spp and below
    W * spp * kSetupCost holds both."""
    W, H, spp = 64, 6, 16

    def more(got, want):
        for ((c, rc), _), p in zip(got, want):
            assert (p.segs[:, 16:48] == spp).all() and p.segs[:, :16].max() > spp and p.segs[:, 48:].max() > spp
            assert W * spp < rc[H // 2] < W * spp * tc.K_SETUP_COST, rc  # the spheres' row: both kinds of pool
            assert c["executed_lane_tests"] > 0

    check_ao("sky_between", W, H, mode, spp, more=more)


@pytest.mark.parametrize("mode", [1, 2])
def test_ao_strip(mode):
    """Rows (5, 11) of 64 x 16: the totals include the two halo rows that were traced (rows 4 and 11),
    read_row_counters returns the six own rows."""
    check_ao("syn64", 64, 16, mode, 16, rows=(5, 11))


def test_ao_pipelined():
    """Mode 1 pipelined, three frames and one read at the end: the trace totals are the three frames'
    sums, and the post-process launches on the output stream counted too."""
    got, _ = check_ao("syn64", 40, 6, 1, 16, cached=(0, 0, 1), pipelined=True, frames=3)
    c = got[0][0][0]
    assert c["filtered_pixels"] > 0 and c["history_read"] > 0 and c["history_accepted"] > 0, c
