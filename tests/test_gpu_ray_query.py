"""Ray queries on the device (rt_trace_rays, rt_trace_pixels, rt_occluded and their _device forms;
include/rt/abi.h "Ray queries"): bit for bit the host specification's answers and, directly, the
expectations built from the oracle's primitives (tests/ray_query_cases.py); the pixel rays' answers
equal the Phong g-buffer's; the queries are ordered on the context's stream and leave frames alone."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import phong_gbuffer_cases as pg
import ray_query_cases as rq
from conftest import ROOT, assert_bitwise
from real_time_ray_tracer_amd import (Header, Renderer, RtError, _lib, aspect_for, occluded_host, pixel_rays_host,
                                      trace_rays_host)

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = rq.W, rq.H
STRIP = (1, 17)  # rows of H = 30


def renderer(h: Header, **kw) -> Renderer:
    r = Renderer(W, H, h.S, h.AA, **kw)
    r.upload_header(h)
    return r


def same_hits(g, t, ind, nrm, what):
    assert np.array_equal(g.ind, ind), f"{what}: ind differs at {np.flatnonzero(g.ind != ind)[:5]}"
    assert_bitwise(g.t, t, f"{what}: t")
    assert_bitwise(g.normals, nrm, f"{what}: normals")


def check_rays(r, h, o, d, what):
    """The device's answers equal the host specification's and the oracle-built expectation."""
    for thr in rq.THRESHOLDS:
        g = r.trace_rays(o, d, thr)
        s = trace_rays_host(h, o, d, thr)
        same_hits(g, s.t, s.ind, s.normals, f"{what} thr {thr} against the host specification")
        same_hits(g, *rq.expected_hits(h, o, d, thr), f"{what} thr {thr} against the oracle")


def headers():
    return [(s, rq.scene(s)) for s in rq.SCENES] + [(f"{n} spheres", rq.sized_scene(n)) for n in rq.SIZES]


@pytest.mark.parametrize("name,h", headers(), ids=[n for n, _ in headers()])
def test_closest_hit_on_every_ray_set(name, h):
    with renderer(h) as r:
        o, d = rq.primary_set(h)
        check_rays(r, h, o, d, f"{name} primary rays")
        for thr in rq.THRESHOLDS:  # the same rays formed on the device
            g = r.trace_pixels(rq.all_pixels(), thr)
            assert_bitwise(g.dirs, d, f"{name}: the pixel rays")
            same_hits(g, *rq.expected_hits(h, o, d, thr), f"{name} pixel rays thr {thr}")
        o, d = rq.aimed_set(h)
        check_rays(r, h, o, d, f"{name} aimed rays")
        if name not in rq.UNBALANCED:
            assert rq.aimed_ok(r.trace_rays(o, d, 0.0).ind), name
        o, d = rq.surface_set(h)
        check_rays(r, h, o, d, f"{name} surface rays")


@pytest.mark.parametrize("case", rq.specials(), ids=[c[0] for c in rq.specials()])
def test_specials(case):
    name, h, o, d, want = case
    with renderer(h) as r:
        check_rays(r, h, o, d, name)
        g = r.trace_rays(o, d, 0.0)
        for k, (wi, wt) in want.items():
            assert g.ind[k] == wi and (wt is None or g.t[k] == F32(wt)), f"{name} ray {k}: {g.ind[k]}, {g.t[k]!r}"


def test_thresholds_part_on_the_near_scene():
    h = rq.scene("near")
    with renderer(h) as r:
        xy = rq.all_pixels()
        i0, i1, i4 = (r.trace_pixels(xy, thr).ind for thr in (0.0, 0.0001, 0.001))
        assert (i0 == 16).all() and (i1 == 16).all() and (i4 != 16).all() and (i4 >= 0).any()


@pytest.mark.parametrize("name,h", headers(), ids=[n for n, _ in headers()])
def test_occlusion(name, h):
    a, b = rq.segment_set(h)
    occ, known, (left, cases) = rq.expected_occluded(h, a, b)
    assert left <= 0.001 * cases
    with renderer(h) as r:
        got = r.occluded(a, b)
    assert np.array_equal(got, occluded_host(h, a, b)), f"{name}: against the host specification"
    assert np.array_equal(got[known], occ[known]), f"{name}: against the oracle"
    assert not got[-1]
    assert name == "empty" or (got.any() and not got.all())


def test_occlusion_by_planes():
    h = Header.synthetic(0, 4, 1234, aspect_for(W, H), num_shapes=3)
    h.pack_plane(0, (0, 1, 0), -4.0, (1, 1, 1))
    h.pack_plane(1, (1, 0, 0.2), -9.0, (1, 1, 1))
    h.pack_plane(2, (-0.3, 0.2, 1), -6.0, (1, 1, 1))
    h.set_mode(0, 3)
    rng = np.random.default_rng(8)
    a = rng.uniform(-15, 15, (20000, 3)).astype(F32)
    b = rng.uniform(-15, 15, (20000, 3)).astype(F32)
    pocc, punsure = rq.plane_occlusion(h, a, b)
    assert punsure.sum() <= 0.001 * punsure.size, f"{int(punsure.sum())} of {punsure.size} cases left out"
    for k in range(3):
        hk = h.copy()
        hk.shapes[[i for i in range(3) if i != k], 4, 3] = 0.0
        with renderer(hk) as r:
            got = r.occluded(a, b)
        ok = ~punsure[k]
        assert np.array_equal(got[ok], pocc[k][ok]), f"plane {k}: {int((got != pocc[k])[ok].sum())} cases differ"
        assert got[ok].any() and not got[ok].all()
        assert np.array_equal(got, occluded_host(hk, a, b)), f"plane {k}: against the host specification"


# ---- the _device forms on torch tensors --------------------------------------------------------
PAD = 64
SENT_F, SENT_I, SENT_B = -12345.5, -77777, 0xAB


def padded(torch, n, width, dtype, fill):
    """A tensor of n * width elements with PAD sentinel elements behind it."""
    return torch.full((n * width + PAD,), fill, dtype=dtype, device="cuda")


def tail_intact(t, n, width, fill):
    return bool((t[n * width:] == fill).all().item())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_device_forms_and_their_bounds(n):
    import torch

    h = rq.scene("syn30p")
    o, d = rq.aimed_set(h, max(n, 1), seed=n + 1)
    o, d = o[:n], d[:n]
    xy = np.stack([np.arange(n) % W, (np.arange(n) // W) % H], axis=1).astype(np.int32).reshape(-1, 2)
    d_o, d_d = torch.from_numpy(o.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    d_xy = torch.from_numpy(xy.copy()).cuda()
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    with renderer(h) as r:
        for nulls in ((), ("t",), ("ind", "normals"), ("t", "ind", "normals")):
            t, ind = padded(torch, n, 1, f32, SENT_F), padded(torch, n, 1, i32, SENT_I)
            nrm, dirs = padded(torch, n, 3, f32, SENT_F), padded(torch, n, 3, f32, SENT_F)
            out = padded(torch, n, 1, u8, SENT_B)
            torch.cuda.synchronize()  # the tensors are filled on torch's stream, the context has its own
            ptr = lambda name, x: None if name in nulls else x.data_ptr()  # noqa: E731
            r.trace_rays_device(d_o.data_ptr(), d_d.data_ptr(), n, 0.0001, ptr("t", t), ptr("ind", ind),
                                ptr("normals", nrm))
            r.synchronize()
            s = trace_rays_host(h, o, d, 0.0001)
            for name, ten, width, fill, want in (("t", t, 1, SENT_F, s.t), ("ind", ind, 1, SENT_I, s.ind),
                                                 ("normals", nrm, 3, SENT_F, s.normals)):
                assert tail_intact(ten, n, width, fill), f"n {n}: wrote behind {name}"
                got = ten[:n * width].cpu().numpy()
                if name in nulls:
                    assert (got == fill).all(), f"n {n}: {name} was not passed and changed"
                else:
                    assert got.tobytes() == want.tobytes(), f"n {n}: {name}"
            if nulls:
                continue
            # pixel rays and occlusion, every output
            t.fill_(SENT_F), ind.fill_(SENT_I), nrm.fill_(SENT_F)
            torch.cuda.synchronize()
            r.trace_pixels_device(d_xy.data_ptr(), n, 0.0, t.data_ptr(), ind.data_ptr(), nrm.data_ptr(),
                                  dirs.data_ptr())
            r.occluded_device(d_o.data_ptr(), d_d.data_ptr(), n, out.data_ptr())
            r.synchronize()
            po, pd = pixel_rays_host(h, W, H, xy)
            s = trace_rays_host(h, po, pd, 0.0)
            assert dirs[:3 * n].cpu().numpy().tobytes() == pd.tobytes() and tail_intact(dirs, n, 3, SENT_F)
            assert t[:n].cpu().numpy().tobytes() == s.t.tobytes() and tail_intact(t, n, 1, SENT_F)
            assert ind[:n].cpu().numpy().tobytes() == s.ind.tobytes() and tail_intact(ind, n, 1, SENT_I)
            assert nrm[:3 * n].cpu().numpy().tobytes() == s.normals.tobytes() and tail_intact(nrm, n, 3, SENT_F)
            assert out[:n].cpu().numpy().tobytes() == occluded_host(h, o, d).astype(np.uint8).tobytes()
            assert tail_intact(out, n, 1, SENT_B)
            # only the directions, then nothing at all
            dirs.fill_(SENT_F), t.fill_(SENT_F)
            torch.cuda.synchronize()
            r.trace_pixels_device(d_xy.data_ptr(), n, 0.0, d_dirs=dirs.data_ptr())
            r.occluded_device(d_o.data_ptr(), d_d.data_ptr(), n, None)
            r.synchronize()
            assert dirs[:3 * n].cpu().numpy().tobytes() == pd.tobytes() and (t == SENT_F).all().item()
        assert r.query_workspace_bytes() == 0  # the _device forms allocate nothing


def test_host_pointer_forms_keep_one_workspace():
    h = rq.scene("syn16")
    o, d = rq.aimed_set(h, 4097)
    with renderer(h) as r:
        assert r.query_workspace_bytes() == 0
        r.trace_rays(o[:100], d[:100])
        small = r.query_workspace_bytes()
        assert small > 0
        for _ in range(3):
            r.trace_rays(o[:100], d[:100])
            r.trace_pixels(rq.all_pixels()[:50])
            r.occluded(o[:64], d[:64])
        assert r.query_workspace_bytes() == small  # nothing allocated per call
        g = r.trace_rays(o, d)
        big = r.query_workspace_bytes()
        assert big > small
        r.trace_rays(o[:1], d[:1])
        assert r.query_workspace_bytes() == big
        s = trace_rays_host(h, o, d)
        same_hits(g, s.t, s.ind, s.normals, "4097 rays after the workspace grew")
        e = r.trace_rays(o[:0], d[:0])
        assert e.t.shape == (0,) and e.normals.shape == (0, 3) and r.occluded(o[:0], d[:0]).shape == (0,)


# ---- pixel rays against the Phong g-buffer -----------------------------------------------------
@pytest.mark.parametrize("scene", ["syn16", "syn30p", "planetie", "near", "cam_inside", "manyplanes"])
def test_pixel_rays_equal_the_phong_gbuffer(scene):
    h = rq.scene(scene)
    xy = rq.all_pixels()
    res, _ = pg.scan(h, W, H)
    with renderer(h) as r, renderer(h, rows=STRIP) as strip:
        r.set_phong_gbuffer(True)
        for mode, thr in ((3, 0.0), (4, 0.001)):
            r.dispatch(mode, 0)
            g = r.download(pixels=False, image=False)
            nrm, dep = g.normals[0].reshape(-1, 4), g.depth[0].reshape(-1, 4)  # [W][H]: x-major, as xy
            q = r.trace_pixels(xy, thr)
            hit = q.ind >= 0
            assert np.array_equal(hit, dep[:, 3] == 1), f"{scene} mode {mode}: hit flags"
            assert_bitwise(q.t[hit], dep[hit, 0], f"{scene} mode {mode}: depth.x")
            assert not dep[~hit].any() and (q.t[~hit] == -1).all()
            assert_bitwise(q.normals, nrm[:, :3], f"{scene} mode {mode}: normals.xyz")
            st, sind = pg.closest(res, thr)
            assert np.array_equal(q.ind, sind.reshape(-1)), f"{scene} mode {mode}: ind against the scan"
            # a strip context answers for every pixel of the frame, as the whole-frame context does
            qs = strip.trace_pixels(xy, thr)
            same_hits(qs, q.t, q.ind, q.normals, f"{scene} mode {mode}: strip context")
            assert_bitwise(qs.dirs, q.dirs, "strip context: rays")
        outside = np.array([[-1, -1], [W, H], [-7, 100], [100000, -100000], [2**31 - 1, -2**31], [3, 2**24 + 1]],
                           np.int32)
        q = r.trace_pixels(outside, 0.0)
        po, pd = pixel_rays_host(h, W, H, outside)
        assert_bitwise(q.dirs, pd, "pixels outside the frame: rays")
        s = trace_rays_host(h, po, pd, 0.0)
        same_hits(q, s.t, s.ind, s.normals, "pixels outside the frame")


# ---- ordering ----------------------------------------------------------------------------------
def test_a_query_reads_the_scene_before_a_later_upload():
    """Pipelining on, frames in flight, a _device query, then at once another scene's upload and a
    dispatch: the query answers for the first scene."""
    import torch

    h0, h1, h2 = rq.scene("syn16"), rq.scene("syn16"), rq.scene("syn16")
    h0.shapes[:, 0, :3] -= F32(0.5)   # every sphere elsewhere
    h2.shapes[:, 0, :3] += F32(0.75)
    o, d = rq.aimed_set(h1, 4097)
    d_o, d_d = torch.from_numpy(o.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    t = torch.zeros(len(o), dtype=torch.float32, device="cuda")
    ind = torch.zeros(len(o), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with Renderer(W, H, h1.S, h1.AA) as r:
        r.enable_pipelining(True)
        # two frames of a third scene, then one of the first: three pipelined frames, so the header
        # copy the next upload will fill still holds the third scene, not the one in effect
        f = r.compute_frames(h0.copy(), 1, 0, 2)
        f = r.compute_frames(h1.copy(), 1, f, 1)
        r.trace_rays_device(d_o.data_ptr(), d_d.data_ptr(), len(o), 0.0001, t.data_ptr(), ind.data_ptr())
        r.upload_header(h2)
        f = r.dispatch(1, f)
        r.synchronize()
        s0, s1, s2 = (trace_rays_host(h, o, d) for h in (h0, h1, h2))
        assert not np.array_equal(s1.ind, s2.ind) and not np.array_equal(s1.ind, s0.ind)
        assert np.array_equal(ind.cpu().numpy(), s1.ind) and t.cpu().numpy().tobytes() == s1.t.tobytes()
        # and the scene in effect is now the second one (one frame in: the other copy holds the third)
        assert np.array_equal(r.trace_rays(o, d).ind, s2.ind)
        # turning pipelining on again keeps the scene in effect, wherever its table sits
        f = r.dispatch(1, f)
        r.enable_pipelining(True)
        assert np.array_equal(r.trace_rays(o, d).ind, s2.ind)
        f = r.dispatch(1, f)
        r.upload_header(h1)  # into the second header copy this time
        f = r.dispatch(1, f)
        r.enable_pipelining(True)
        assert np.array_equal(r.trace_rays(o, d).ind, s1.ind)


def test_a_query_on_a_torch_stream_sees_the_upload_before_it():
    import torch

    h1, h2 = rq.scene("syn16"), rq.scene("syn16")
    h2.shapes[:, 0, :3] += F32(0.75)
    o, d = rq.aimed_set(h1, 4097)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s), Renderer(W, H, h1.S, h1.AA) as r:
        r.set_stream(s)
        d_o, d_d = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev)
        for h in (h1, h2, h1):
            ind = torch.full((len(o),), -5, dtype=torch.int32, device=dev)
            r.upload_header(h)
            r.trace_rays_device(d_o.data_ptr(), d_d.data_ptr(), len(o), 0.0001, d_ind=ind.data_ptr())
            got = ind.cpu().numpy()  # ordered after the query on the same stream
            assert np.array_equal(got, trace_rays_host(h, o, d).ind)


# ---- errors ------------------------------------------------------------------------------------
def test_errors():
    lib = _lib.load()
    h = rq.scene("syn16")
    o, d = rq.aimed_set(h, 8)
    xy = rq.all_pixels()[:8]
    with Renderer(W, H, h.S, h.AA) as r:
        for call in (lambda: r.trace_rays(o, d), lambda: r.trace_pixels(xy), lambda: r.occluded(o, d),
                     lambda: r.trace_rays(o[:0], d[:0])):
            with pytest.raises(RtError) as e:
                call()
            assert e.value.status == _lib.RT_E_STATE  # no header yet
        r.upload_header(h)
        fp = _lib.fptr
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        t = np.zeros(8, F32)
        E = _lib.RT_E_INVAL
        assert lib.rt_trace_rays(r.ctx, fp(o), fp(d), 8, 0.0, fp(t), None, None) == 0
        assert lib.rt_trace_rays(None, fp(o), fp(d), 8, 0.0, fp(t), None, None) == E
        assert lib.rt_trace_rays(r.ctx, None, fp(d), 8, 0.0, fp(t), None, None) == E
        assert lib.rt_trace_rays(r.ctx, fp(o), None, 8, 0.0, fp(t), None, None) == E
        assert lib.rt_trace_rays(r.ctx, fp(o), fp(d), (1 << 28) + 1, 0.0, fp(t), None, None) == E
        for bad in (-1e-9, float("nan"), float("inf")):
            assert lib.rt_trace_rays(r.ctx, fp(o), fp(d), 8, bad, fp(t), None, None) == E
            assert lib.rt_trace_pixels(r.ctx, ip(xy), 8, bad, fp(t), None, None, None) == E
            assert lib.rt_trace_rays_device(r.ctx, None, None, 0, bad, None, None, None) == E
            assert lib.rt_trace_pixels_device(r.ctx, None, 0, bad, None, None, None, None) == E
        assert lib.rt_trace_pixels(r.ctx, None, 8, 0.0, fp(t), None, None, None) == E
        assert lib.rt_trace_pixels(None, ip(xy), 8, 0.0, fp(t), None, None, None) == E
        assert lib.rt_occluded(r.ctx, None, fp(d), 8, None) == E and lib.rt_occluded(None, fp(o), fp(d), 8, None) == E
        assert lib.rt_occluded(r.ctx, fp(o), fp(d), (1 << 28) + 1, None) == E
        # the _device forms check before they launch: no pointer here is ever read
        assert lib.rt_trace_rays_device(r.ctx, None, None, 8, 0.0, None, None, None) == E
        assert lib.rt_trace_rays_device(None, None, None, 0, 0.0, None, None, None) == E
        assert lib.rt_trace_pixels_device(r.ctx, None, 8, 0.0, None, None, None, None) == E
        assert lib.rt_occluded_device(r.ctx, None, None, 8, None) == E
        assert lib.rt_occluded_device(r.ctx, None, None, (1 << 28) + 1, None) == E
        assert lib.rt_trace_rays_device(r.ctx, None, None, 0, 0.0, None, None, None) == 0  # n == 0
        assert lib.rt_occluded_device(r.ctx, None, None, 0, None) == 0
        assert lib.rt_query_workspace_bytes(None) == 0


# ---- queries leave the frames alone ------------------------------------------------------------
def test_frames_do_not_depend_on_interleaved_queries():
    """A 3-frame mode-1 run: cull cache statistics, image and g-buffers are bitwise the same with
    queries between the frames as without."""
    h = rq.scene("syn16")
    o, d = rq.aimed_set(h, 2000)
    out = {}
    for queries in (False, True):
        with Renderer(W, H, h.S, h.AA) as r:
            hh = h.copy()
            f = 0
            for k in range(3):
                hh.fill_rand_buffer(7000 + k)
                hh.set_mode(f, hh.num_objects)
                r.upload_header(hh)
                f = r.dispatch(1, f)
                if queries:
                    r.trace_rays(o, d, 0.0)
                    r.trace_pixels(rq.all_pixels(), 0.001)
                    r.occluded(o, d)
            out[queries] = (r.cull_cache_stats(), r.download())
    (s0, g0), (s1, g1) = out[False], out[True]
    assert s0 == s1 and s0["fills"] + s0["cached_launches"] <= 3
    for name in ("pixels", "normals", "depth", "image"):
        assert_bitwise(getattr(g1, name), getattr(g0, name), f"{name} with queries interleaved")


# ---- the headless driver -----------------------------------------------------------------------
@pytest.mark.parametrize("xy", [(20, 15), (3, 28), (39, 0), (-4, 50)])
def test_headless_pick_prints_what_trace_pixels_predicts(xy):
    exe = ROOT / "build" / "rt_headless"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT), "headless"], check=True, capture_output=True)
    p = subprocess.run([str(exe), "--width", str(W), "--height", str(H), "--scene", "synthetic", "--objects", "16",
                        "--mode", "3", "--frames", "2", "--pick", f"{xy[0]},{xy[1]}"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    h = Header.synthetic(16, 4, 1234, aspect_for(W, H))  # rt_headless's scene
    with renderer(h) as r:
        q = r.trace_pixels([list(xy)], 0.0)
    want = "pick %d %d %d " % (xy[0], xy[1], q.ind[0]) + " ".join("%.9g" % float(v) for v in (q.t[0], *q.normals[0]))
    assert p.stdout.splitlines()[-1] == want
