"""The cull cache's pool list (rt_set_pool_list, rt_cull.h CullCache): once a table's list and its two
counts have landed, the single-frame launches of the sorted, cached AO forms run one workgroup per
non-sky pool, which reads (pb, xf, yf, np) from its row, and one per 64 sky pools.  The list orders
and sizes the launch and nothing else, so every case renders the same frames with the list on and
off and asks for equal bits; the whole-frame cases are held against the CPU oracle as well.

Frames of 64 x 8, 40 x 6 and 48 x 5 pixels (40 is no multiple of 16: pools straddle row ends, and
the last pool of 40 x 6 at spp 4 is partial), scenes of 48 spheres so that the sorted forms are
selected.  A still sequence runs frames 0 and 1 uncached, frame 2 behind the fill and the list's
build over every pool, and, since every frame here is followed by a synchronize, frame 3 and later
over the list."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import assert_bitwise, assert_close
from real_time_ray_tracer_amd import SSBO, Header, Renderer, StripGroup, _lib, aspect_for
from test_gpu_ao_normal_sort import CAM, N, far_header, pools_of, world_xy
from test_gpu_parity import make_header

pytestmark = pytest.mark.gpu

SIZES = [(64, 8), (40, 6), (48, 5)]


def scene(kind, spp, W, H):
    """sky: every sphere far outside the view.  nosky: a sphere that fills the view as well.
    mixed: two small spheres in front of row 1 instead, every other pool sky."""
    h = far_header(spp, W, H)
    if kind == "nosky":
        h.pack_sphere(0, (0.0, 0.0, 0.0), 200.0, (0.6, 0.5, 0.4))
    elif kind == "mixed":
        for i, px in enumerate((6, W - 7)):
            x, y = world_xy(h, W, H, px, 1)
            h.pack_sphere(i, (x, y, 0.0), 0.6, (0.7, 0.3 + 0.3 * i, 0.2))
    else:
        assert kind == "sky"
    h.set_mode(0, N)
    return h


def render(h0, W, H, frames, use_list, rows=None, mode=1, mutate=None, before=None, after=None, counters=False,
           want_list=False):
    """`frames` frames as the render loop makes them, a synchronize behind each.  Returns the g-buffer,
    the two stats, the launch log and (want_list) the downloaded list."""
    r = Renderer(W, H, h0.S, h0.AA, rows=rows)
    r.set_pool_list(use_list)
    r.set_launch_log(True)
    if counters:
        r.enable_counters(True, rows=True)
    h = h0.copy()
    f = 0
    for k in range(frames):
        if mutate:
            mutate(k, h)
        if before:
            before(k, r)
        h.fill_rand_buffer(7000 + k)
        h.set_mode(f, h.num_objects)
        r.upload_header(h)
        f = r.dispatch(mode, f)
        r.synchronize()
        if after:
            after(k, r)
    out = {"g": r.download(), "cull": r.cull_cache_stats(), "list": r.pool_list_stats(), "log": r.launch_log(),
           "pools": r.debug_pool_list() if want_list else None}
    r.close()
    return out


def same(a, b, what):
    for name in ("image", "pixels", "normals", "depth"):  # (pixels, normals, depth: every ring slot)
        assert_bitwise(getattr(a["g"], name), getattr(b["g"], name), f"{what} {name}")


def oracle_frames(h0, W, H, frames):
    h = h0.copy()
    s = SSBO(h, W, H)
    d = oracle.dims(W, H, h.S, h.AA)
    img = np.zeros((H, W, 4), np.float32)
    f = 0
    for k in range(frames):
        h.fill_rand_buffer(7000 + k)
        h.set_mode(f, h.num_objects)
        s.set_header(h)
        f = oracle.dispatch(s.data, d, 1, f, img)
    return s, img


def expected_list(masks, W, trace_row0, trace_rows, spp):
    """The list from the masks: ao_batch_kernel's pool start (p0 = pb TP; np, yf, xf)."""
    tp = max(1, 256 // spp)
    npix = trace_rows * W
    nonsky = masks.reshape(masks.shape[0], -1).any(axis=1)
    pb = np.flatnonzero(nonsky)
    p0 = pb * tp
    rows = np.stack([pb, p0 % W, trace_row0 + p0 // W, np.minimum(npix - p0, tp)], axis=1).astype(np.int32)
    return rows, np.flatnonzero(~nonsky).astype(np.uint32)


def check_list(out, W, trace_row0, trace_rows, spp):
    pools = pools_of(W, trace_rows, spp)
    got = out["pools"]
    masks = got["masks"].reshape(pools, -1)
    rows, sky = expected_list(masks, W, trace_row0, trace_rows, spp)
    assert np.array_equal(got["rows"], rows), (got["rows"], rows)
    assert np.array_equal(got["sky"], sky), (got["sky"], sky)
    assert (np.diff(got["rows"][:, 0]) > 0).all() and (np.diff(got["sky"].astype(np.int64)) > 0).all()
    st = out["list"]
    assert (st["n_nonsky"], st["n_sky"]) == (len(rows), len(sky)) and len(rows) + len(sky) == pools, st
    assert st["bytes"] == 16 * pools + 16 + 16  # rows and sky entries, one chunk count padded, the counts
    return len(rows), len(sky)


@pytest.mark.parametrize("kind", ["sky", "nosky", "mixed"])
@pytest.mark.parametrize("spp", [16, 4])
@pytest.mark.parametrize("W,H", SIZES)
def test_identity_and_contents(W, H, spp, kind):
    """11 frames (the 8-slot ring wraps), a fresh rand_buffer each: frames 3..10 over the list."""
    frames = 11
    h = scene(kind, spp, W, H)
    on = render(h, W, H, frames, True, want_list=True)
    off = render(h, W, H, frames, False)
    same(on, off, f"{kind} {W}x{H} spp {spp}")
    assert on["log"] == off["log"]
    assert on["cull"] == off["cull"] and on["cull"]["fills"] == 1 and on["cull"]["cached_launches"] == frames - 2
    assert on["list"]["builds"] == 1 and on["list"]["list_launches"] == frames - 3, on["list"]
    assert off["list"]["builds"] == 0 and off["list"]["list_launches"] == 0 and off["list"]["n_nonsky"] == -1
    nn, ns = check_list(on, W, 0, H, spp)
    # (the 4 pools of 240 pixels at spp 4 are 1.6 rows each: the two spheres' cones reach them all)
    mixed = nn > 0 and (ns > 0 or nn + ns <= 4)
    assert {"sky": nn == 0, "nosky": ns == 0, "mixed": mixed}[kind], (nn, ns)
    s, img = oracle_frames(h, W, H, frames)
    assert_bitwise(on["g"].normals, s.normals, "normals against the oracle")
    assert_bitwise(on["g"].depth, s.depth, "depth against the oracle")
    assert_close(on["g"].pixels, s.pixels, "pixels against the oracle")
    assert_close(on["g"].image, img, "image against the oracle")


def test_more_than_64_sky_pools_and_a_partial_sky_block():
    """64 x 40 at spp 16: 160 pools, 150 and more of them sky: three sky blocks, the last partial."""
    W, H = 64, 40
    h = scene("mixed", 16, W, H)
    on = render(h, W, H, 5, True, want_list=True)
    same(on, render(h, W, H, 5, False), "64x40")
    nn, ns = check_list(on, W, 0, H, 16)
    assert ns > 128 and ns % 64 != 0 and nn > 0
    assert on["list"]["builds"] == 1 and on["list"]["list_launches"] == 2
    assert on["cull"] == {"fills": 1, "cached_launches": 3, "table_bytes": 160 * 8}


def test_two_builds_of_one_key_are_the_same_bytes():
    """Off and on again drops the table; the same key then builds the same list."""
    W, H = 40, 6
    h = scene("mixed", 16, W, H)
    lists = []

    def before(k, r):
        if k == 4:
            lists.append(r.debug_pool_list())
            r.set_pool_list(False)
            r.set_pool_list(True)
    out = render(h, W, H, 8, True, before=before, want_list=True)
    lists.append(out["pools"])
    assert out["list"]["builds"] == 2 and out["cull"]["fills"] == 2
    for name in ("rows", "sky", "masks"):
        assert lists[0][name].tobytes() == lists[1][name].tobytes(), name
    assert len(lists[0]["rows"]) > 0 and len(lists[0]["sky"]) > 0


def test_camera_nudge_drops_the_list_and_still_frames_rebuild_it():
    """Ten frames, the camera moves before frame 5.  Frame 2 fills and builds (over every pool), 3 and
    4 run over the list; 5 and 6 in-kernel, without a list; 7 rebuilds; 8 and 9 over the new list."""
    W, H = 40, 6
    seen = []

    def mutate(k, h):
        if k == 5:
            h.vec4(CAM)[0] += np.float32(0.75)
    h = scene("mixed", 16, W, H)
    kw = dict(mutate=mutate, after=lambda k, r: seen.append((r.pool_list_stats(), r.cull_cache_stats())))
    on = render(h, W, H, 10, True, **kw)
    same(on, render(h, W, H, 10, False, mutate=mutate), "nudge")
    assert [s["builds"] for s, _ in seen] == [0, 0, 1, 1, 1, 1, 1, 2, 2, 2]
    assert [s["list_launches"] for s, _ in seen] == [0, 0, 0, 1, 2, 2, 2, 2, 3, 4]
    assert [c["cached_launches"] for _, c in seen] == [0, 0, 1, 2, 3, 3, 3, 4, 5, 6]
    # (the counts are taken up by the first launch that finds the build's event fired)
    assert [s["n_nonsky"] >= 0 for s, _ in seen] == [False, False, False, True, True, False, False, False, True, True]
    assert on["cull"]["fills"] == 2


def test_moving_camera_never_builds():
    def mutate(k, h):
        h.vec4(CAM)[0] += np.float32(0.01)
    W, H = 40, 6
    on = render(scene("mixed", 16, W, H), W, H, 6, True, mutate=mutate)
    assert on["list"] == {"builds": 0, "list_launches": 0, "n_nonsky": -1, "n_sky": -1, "bytes": 0}
    assert on["cull"]["fills"] == 0


def test_cap_below_the_sum_keeps_masks_and_frames():
    """40 x 6 at spp 16: 15 pools, 120 bytes of masks, 480 of frames, 272 of list.  A cap one byte short
    of the three: masks and frames as before, no list; the cap of the three: the list."""
    W, H = 40, 6
    h = scene("mixed", 16, W, H)
    off = render(h, W, H, 5, False)
    for cap, listed in ((120 + 480 + 271, False), (120 + 480 + 272, True)):
        fb = []
        on = render(h, W, H, 5, True, before=lambda k, r: r.debug_cull_cache_cap(cap) if k == 0 else None,
                    after=lambda k, r: fb.append(r.cull_cache_frame_bytes()))
        same(on, off, f"cap {cap}")
        assert fb[-1] == 480 and on["cull"] == {"fills": 1, "cached_launches": 3, "table_bytes": 120}
        want = {"builds": 1, "list_launches": 2, "bytes": 272} if listed else {"builds": 0, "list_launches": 0, "bytes": 0}
        assert {k: on["list"][k] for k in want} == want, on["list"]


@pytest.mark.parametrize("mode", [1, 2])
def test_strip_context(mode):
    """rows (5, 11) of a 64 x 16 frame: trace_row0 = 4 (the halo row), 8 traced rows; the rows' yf are
    the frame's.  Against the list off, and the strip's image against the whole frame's rows."""
    W, H = 64, 16
    h = scene("mixed", 16, W, H)
    for i, px in enumerate((20, 50)):  # two more spheres, inside the strip
        x, y = world_xy(h, W, H, px, 8)
        h.pack_sphere(2 + i, (x, y, 0.0), 0.6, (0.3, 0.6, 0.8))
    h.set_mode(0, N)
    on = render(h, W, H, 6, True, rows=(5, 11), mode=mode, want_list=True)
    off = render(h, W, H, 6, False, rows=(5, 11), mode=mode)
    same(on, off, "strip")
    nn, ns = check_list(on, W, 4, 8, 16)
    assert nn > 0 and ns > 0 and on["list"]["builds"] == 1 and on["list"]["list_launches"] == 3
    assert on["cull"] == off["cull"] == {"fills": 1, "cached_launches": 4, "table_bytes": 32 * 8}
    whole = render(h, W, H, 6, False, mode=mode)
    assert_bitwise(on["g"].image, whole["g"].image[5:11], "the strip's rows of the whole frame")


@pytest.mark.parametrize("pipelined", [False, True])
def test_two_strip_group_equals_the_whole_frame(pipelined):
    """Strips of rows 0..2 and 3..7 of 64 x 8 (with their halo rows 16 and 24 pools), a synchronize behind
    every frame: each strip fills and builds once and runs frames 3..9 over its own list."""
    W, H, frames = 64, 8, 10
    h0 = scene("mixed", 16, W, H)

    def drive(r):
        h, f = h0.copy(), 0
        for k in range(frames):
            h.fill_rand_buffer(7000 + k)
            h.set_mode(f, h.num_objects)
            r.upload_header(h)
            f = r.dispatch(1, f)
            r.synchronize()
        return f

    r = Renderer(W, H, h0.S, h0.AA)
    r.set_pool_list(False)
    f0 = drive(r)
    want = r.image()
    r.close()
    lib = _lib.load()
    for use_list in (True, False):
        with StripGroup(W, H, h0.S, h0.AA, [0, 0], bounds=[0, 3, 8]) as g:
            g.set_pool_list(use_list)
            if pipelined:
                g.enable_pipelining(True)
            assert drive(g) == f0
            assert_bitwise(g.image(), want, f"group, list {use_list}")
            for i, pools in enumerate((16, 24)):
                b, n, nn, ns, by = C.c_longlong(), C.c_longlong(), C.c_int(), C.c_int(), C.c_size_t()
                assert lib.rt_pool_list_stats(g.strip_ctx(i), C.byref(b), C.byref(n), C.byref(nn), C.byref(ns), C.byref(by)) == 0
                fl, ca, tb = C.c_longlong(), C.c_longlong(), C.c_size_t()
                assert lib.rt_cull_cache_stats(g.strip_ctx(i), C.byref(fl), C.byref(ca), C.byref(tb)) == 0
                assert (fl.value, ca.value, tb.value) == (1, frames - 2, 8 * pools), (i, fl.value, ca.value, tb.value)
                # (one mask word per pool; the strips' traced rows are their own and one halo row each)
                if use_list:
                    assert (b.value, n.value, nn.value + ns.value) == (1, frames - 3, pools), (i, b.value, n.value)
                    assert by.value == 16 * pools + 32
                else:
                    assert (b.value, n.value, nn.value) == (0, 0, -1)


def test_pipelined_with_streams_toggled_mid_run():
    """Pipelined mode 1 on torch streams, 16 frames; pipelining off at frame 6 and on again at 9, the
    context's own stream from frame 11, the camera moves at frame 12.  Against the sequential order
    with the list off."""
    import torch

    W, H = 40, 6
    h0 = scene("mixed", 16, W, H)
    dev = torch.device("cuda", 0)
    main, out = torch.cuda.Stream(dev), torch.cuda.Stream(dev)

    def frames(r, h, toggles):
        f = 0
        for k in range(16):
            if k == 12:
                h.vec4(CAM)[0] += np.float32(0.25)
            if toggles:
                if k == 6:
                    r.enable_pipelining(False)
                if k == 9:
                    r.enable_pipelining(True, out)
                if k == 11:
                    r.set_stream(None)
            h.fill_rand_buffer(7000 + k)
            h.set_mode(f, h.num_objects)
            r.upload_header(h)
            f = r.dispatch(1, f)
            if k in (3, 10, 15):
                r.synchronize()

    a = Renderer(W, H, h0.S, h0.AA)
    a.set_pool_list(False)
    frames(a, h0.copy(), False)
    b = Renderer(W, H, h0.S, h0.AA)
    b.set_stream(main)
    b.enable_pipelining(True, out)
    frames(b, h0.copy(), True)
    ga, gb = a.download(), b.download()
    for name in ("image", "pixels", "normals", "depth"):
        assert_bitwise(getattr(gb, name), getattr(ga, name), name)
    sa, sb = a.pool_list_stats(), b.pool_list_stats()
    assert sa["builds"] == 0 and sb["builds"] == 2 and sb["list_launches"] >= 6, (sa, sb)
    # the keys hold over frames 0..11 and 12..15: a fill at the third frame of each run
    assert a.cull_cache_stats() == {"fills": 2, "cached_launches": 10 + 2, "table_bytes": 15 * 8}
    cb = b.cull_cache_stats()  # (a change of streams may cost a refill, never a result)
    assert cb["fills"] >= 2 and cb["cached_launches"] >= sb["list_launches"] and cb["table_bytes"] == 15 * 8, cb
    a.close()
    b.close()


def test_counter_multi_frame_and_plane_forms_launch_as_before():
    """Counters on: the counter forms, over every pool.  Mode 2 in launches of 4 frames: the multi-frame
    forms.  A ground plane: never cached.  The launch logs are those of the list off."""
    W, H = 40, 6
    h = scene("mixed", 16, W, H)
    on = render(h, W, H, 6, True, counters=True)
    off = render(h, W, H, 6, False, counters=True)
    same(on, off, "counters")
    assert on["log"] == off["log"] and "ao_batch_kernel<AoProd<16, 20, 86u>>" in on["log"]
    assert on["list"]["builds"] == 1 and on["list"]["list_launches"] == 0 and on["cull"]["cached_launches"] == 4
    logs = []
    for use_list in (True, False):
        r = Renderer(W, H, h.S, h.AA)
        r.set_pool_list(use_list)
        r.set_launch_log(True)
        r.set_frame_batch(4)
        hh, f = h.copy(), 0
        for k in range(5):
            f = r.compute_frames(hh, 2, f, 4, rand_seed=7000 + 4 * k)
            r.synchronize()
        assert r.cull_cache_stats() == {"fills": 1, "cached_launches": 3, "table_bytes": 15 * 8}
        logs.append((r.download(), r.launch_log(), r.pool_list_stats()))
        r.close()
    for name in ("pixels", "normals", "depth"):
        assert_bitwise(getattr(logs[0][0], name), getattr(logs[1][0], name), f"multi-frame {name}")
    assert logs[0][1] == logs[1][1] and "ao_batch_kernel<AoProd<16, 20, 102u>>" in logs[0][1]
    assert logs[0][2]["list_launches"] == 0
    hp = make_header("syn56p", W, H, 16)
    on = render(hp, W, H, 5, True)
    assert on["list"]["builds"] == 0 and on["cull"]["fills"] == 0
