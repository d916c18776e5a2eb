"""The query tree on the device (rt_set_query_tree; include/rt/abi.h "Query tree"): the three ray
queries with the switch on answer with the bytes they answer with when it is off, on one context, for
every ray of every set below, and both equal the host specification on a 512-ray subset.  Zero
mismatches allowed, no case left out.  Then the _device forms, header changes, strips, and the tree
kernels' gate, node decision and member test alone (RT_MATH_CULL_TREE)."""
import ctypes as C

import numpy as np
import pytest

import cull_cases as cc
import oracle
from conftest import assert_bitwise
from real_time_ray_tracer_amd import (Header, Hits, Renderer, RtError, StripGroup, _lib, aspect_for, occluded_host,
                                      query_tree_host, trace_rays_host)

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 64, 48
ASPECT = aspect_for(W, H)
LO, HI = np.array([-10.0, -6.0, -24.0]), np.array([10.0, 6.0, -4.0])  # the scenes' box, in front of the camera


# ---- scenes ------------------------------------------------------------------------------------
def box_scene(n, seed=5, S=None):
    """n random spheres in the box (rt_scenegen's camera, light and materials; no ground sphere)."""
    h = Header.synthetic(n, 4, 1234, ASPECT, num_shapes=S if S is not None else max(n, 1))
    rng = np.random.default_rng(seed)
    h.shapes[:n, 0, :3] = rng.uniform(LO, HI, (n, 3)).astype(F32)
    h.shapes[:n, 0, 3] = rng.uniform(0.1, 0.45, n).astype(F32)
    return h


def scene(name):
    if name == "box2048":
        return box_scene(2048)
    if name == "ground300":
        h = box_scene(301)
        h.pack_sphere(150, (0.0, -1006.5, -14.0), 1000.0, (0.5, 0.5, 0.5))  # on the always list
        return h
    if name == "mixed":
        h = box_scene(200)
        for k, i in enumerate((5, 77, 150)):
            h.pack_plane(i, ((0, 1, 0), (0, 0, 1), (1, 0, 0.2))[k], (-6.5, -25.0, -11.0)[k], (0.4, 0.4, 0.4))
        for k, i in enumerate((0, 101, 199)):
            h.pack_rectangle(i, (-6.0 + 3 * k, -3.0, -7.0 - 5 * k), (5, 0, 0), (0, 4, 0), (1, 1, 1))
        return h
    if name == "duplicates":
        h = box_scene(64)
        h.shapes[32:64] = h.shapes[0:32]
        return h
    if name == "one-centre":
        h = box_scene(48)
        h.shapes[:48, 0, :3] = (1.5, -0.25, -12.0)
        return h
    if name == "odd-rows":
        h = box_scene(64)
        h.shapes[3, 0, 3] = 0.0
        h.shapes[4, 0, 3] = -h.shapes[4, 0, 3]
        h.shapes[5, 0, 0] = np.inf
        h.shapes[6, 0, 1] = -np.inf
        h.shapes[7, 0, 3] = np.nan
        h.shapes[8, 0, 0] = np.nan
        h.shapes[9, 0, 3] = np.inf
        return h
    if name == "small":
        return box_scene(7)
    if name == "nobj0":
        return box_scene(0, S=16)
    raise KeyError(name)


SCENES = [("box2048", False), ("ground300", False), ("mixed", False), ("mixed", True), ("duplicates", False),
          ("one-centre", False), ("odd-rows", False), ("small", False), ("nobj0", False)]


# ---- rays --------------------------------------------------------------------------------------
def unit(rng, n):
    return oracle.normalize3_n(rng.normal(size=(n, 3)).astype(F32))


def finite_spheres(h):
    n = h.num_objects
    g = h.shapes[:n, 0]
    ok = (h.shapes[:n, 4, 3] == 1) & np.isfinite(g).all(axis=1) & (np.abs(g[:, 3]) < 20)
    return g[ok].astype(np.float64) if ok.any() else np.array([[0.0, 0.0, -14.0, 0.3]])


def ray_sets(h, seed=9):
    """(origins, dirs) [n][3], n <= 8192: the sets of the module's docstring, concatenated."""
    rng = np.random.default_rng(seed)
    g = finite_spheres(h)
    pick = lambda n: g[rng.integers(0, len(g), n)]  # noqa: E731
    o, d = [], []
    # random unit rays: origins around the box (outside and inside the balls), and inside spheres
    o.append(rng.uniform(LO - 4, HI + 4, (1500, 3)))
    d.append(unit(rng, 1500))
    s = pick(700)
    o.append(s[:, :3] + 0.6 * np.abs(s[:, 3:4]) * unit(rng, 700))
    d.append(unit(rng, 700))
    # bounce rays: from a sphere's surface, leaving at random angles
    s, u = pick(1500), unit(rng, 1500)
    o.append((s[:, :3].astype(F32) + (np.abs(s[:, 3:4]).astype(F32) * u)))
    d.append(unit(rng, 1500))
    # grazing rays: aimed at c + r (1 +- k 2^-23) u, perpendicular to u, from near and from 1e4 r away
    for dist in (3.0, 1e4):
        s, u = pick(900), unit(rng, 900).astype(np.float64)
        w = np.cross(u, unit(rng, 900).astype(np.float64))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        k = rng.integers(-4, 5, (900, 1))
        r = np.abs(s[:, 3:4])
        p = s[:, :3] + r * (1.0 + k * 2.0 ** -23) * u
        o.append(p - dist * r * w)
        d.append(oracle.normalize3_n(w.astype(F32)))
    # directions that are not unit vectors, and odd ones: the gate's fall-back
    s = pick(1200)
    oo = rng.uniform(LO - 4, HI + 4, (1200, 3))
    dd = oracle.normalize3_n((s[:, :3] + 0.7 * np.abs(s[:, 3:4]) * unit(rng, 1200) - oo).astype(F32))
    kind = np.arange(1200) % 6
    dd[kind == 0] *= F32(0.5)
    dd[kind == 1] *= F32(2.0)
    dd[kind == 2] *= F32(1.0 + 1e-6)
    dd[kind == 3] = 0.0
    dd[kind == 4, 1] = np.nan
    dd[kind == 5, 2] = np.inf
    o.append(oo)
    d.append(dd)
    o = np.ascontiguousarray(np.concatenate(o), F32)
    d = np.ascontiguousarray(np.concatenate(d), F32)
    assert len(o) == len(d) <= 8192
    return o, d


def segments(h, seed=10):
    """(a, b): random point pairs, surface points to the light, a == b, segments that end inside a sphere."""
    rng = np.random.default_rng(seed)
    g = finite_spheres(h)
    pick = lambda n: g[rng.integers(0, len(g), n)]  # noqa: E731
    a = [rng.uniform(LO - 4, HI + 4, (2500, 3))]
    b = [rng.uniform(LO - 4, HI + 4, (2500, 3))]
    s = pick(2500)
    a.append(s[:, :3].astype(F32) + np.abs(s[:, 3:4]).astype(F32) * unit(rng, 2500))
    b.append(np.broadcast_to(h.data[20:23], (2500, 3)))
    p = rng.uniform(LO, HI, (100, 3))
    a.append(p)
    b.append(p)
    a.append(rng.uniform(LO - 4, HI + 4, (1500, 3)))
    b.append(pick(1500)[:, :3])
    a = np.ascontiguousarray(np.concatenate(a), F32)
    b = np.ascontiguousarray(np.concatenate(b), F32)
    assert len(a) <= 8192
    return a, b


def all_pixels():
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.int32)


def raw_equal(on, off, what):
    for name in ("t", "ind", "normals", "dirs"):
        x, y = getattr(on, name, None), getattr(off, name, None)
        if x is None and y is None:
            continue
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero((x.reshape(len(x), -1).view(np.uint32) != y.reshape(len(y), -1).view(np.uint32)).any(axis=1))
            raise AssertionError(f"{what}: {name} differs on {len(bad)} of {len(x)} rays, first {bad[:5]}")


def against_host(g, s, what):
    assert np.array_equal(g.ind, s.ind), f"{what}: ind differs at {np.flatnonzero(g.ind != s.ind)[:5]}"
    assert_bitwise(g.t, s.t, f"{what}: t")
    assert_bitwise(g.normals, s.normals, f"{what}: normals")


def subset(g, sel):
    return Hits(g.t[sel], g.ind[sel], g.normals[sel])


def off_on(r, fn):
    r.set_query_tree(False)
    off = fn()
    r.set_query_tree(True)
    assert r.query_tree
    return off, fn()


# ---- equality on one context -------------------------------------------------------------------
@pytest.mark.parametrize("name,rects", SCENES, ids=[f"{n}{'-rect' if r else ''}" for n, r in SCENES])
def test_tree_answers_are_the_linear_answers(name, rects):
    h = scene(name)
    o, d = ray_sets(h)
    a, b = segments(h)
    sub = np.random.default_rng(3).choice(len(o), 512, replace=False)
    xy = all_pixels()
    with Renderer(W, H, h.S, h.AA) as r:
        r.set_rectangles(rects)
        r.upload_header(h)
        r.set_query_tree(True)
        st = r.query_tree_stats()
        want = query_tree_host(h, rectangles=rects)
        assert st["nodes"] == len(want["balls"]) and st["always"] == len(want["always"])
        assert st["leaves"] == int((want["links"][:, 2] > 0).sum()) and st["bytes"] > 0
        if name in ("small", "nobj0"):
            assert st["nodes"] == 0                       # below the threshold: the linear kernels run
        else:
            assert st["nodes"] > 0
        if name == "ground300":
            assert want["always"].tolist() == [150]
        for thr in (0.0, 0.001, 0.0001):                  # every pixel of the frame
            off, on = off_on(r, lambda: r.trace_pixels(xy, thr))
            raw_equal(on, off, f"{name} pixels thr {thr}")
        for thr in (0.0, 0.0001):
            off, on = off_on(r, lambda: r.trace_rays(o, d, thr))
            raw_equal(on, off, f"{name} rays thr {thr}")
            s = trace_rays_host(h, o[sub], d[sub], thr, rectangles=rects)
            for got, what in ((on, "on"), (off, "off")):
                against_host(subset(got, sub), s, f"{name} thr {thr}, the switch {what}")
        if name == "duplicates":                          # the lowest index of a duplicated sphere
            assert (on.ind < 32).all()
        if name not in ("nobj0",):
            assert (on.ind >= 0).any() and (on.ind < 0).any()
        off, on = off_on(r, lambda: r.occluded(a, b))
        assert on.tobytes() == off.tobytes(), f"{name}: occlusion differs on {int((on != off).sum())} segments"
        if name != "nobj0":
            assert on.any() and not on.all()
        assert r.query_tree_stats() == st


@pytest.mark.parametrize("name,rects", SCENES, ids=[f"{n}{'-rect' if r else ''}" for n, r in SCENES])
def test_occlusion_equals_the_host_specification(name, rects):
    """rt_occluded with the switch off and on against rt_occluded_host_ex on a 512-segment subset.

    [odd-rows] is the case that found a fault: the scene's sphere 7 has a NaN radius and a finite
    centre, so its discriminant is NaN and eval_ray gives NaN, which occludes nothing; the device's
    shadow-ray sphere test (rt_device.h sphere_eval_shadow) clamps the discriminant with a v_max_f32,
    which returns the other operand for a NaN, and went on with a root of 2^-50, so the sphere
    occluded whatever lay behind its centre: 176 of the 512 segments differed from the host, with the
    switch off exactly as with it on.  pack_header now packs a sphere whose radius is NaN as the NaN
    row of a shape that is never hit, which is what the rule says of it."""
    h = scene(name)
    a, b = segments(h)
    subs = np.random.default_rng(4).choice(len(a), 512, replace=False)
    want = occluded_host(h, a[subs], b[subs], rectangles=rects)
    with Renderer(W, H, h.S, h.AA) as r:
        r.set_rectangles(rects)
        r.upload_header(h)
        off, on = off_on(r, lambda: r.occluded(a[subs], b[subs]))
    print(f"{name}: of 512 segments, {int((off != want).sum())} differ from the host with the switch off, "
          f"{int((on != want).sum())} with it on")
    assert np.array_equal(off, want), f"{name}, the switch off: {int((off != want).sum())} of 512 segments differ from the host"
    assert np.array_equal(on, want), f"{name}, the switch on: {int((on != want).sum())} of 512 segments differ from the host"


# ---- the _device forms -------------------------------------------------------------------------
def test_device_forms_with_the_tree():
    import torch

    h = scene("ground300")
    o, d = ray_sets(h)
    a, b = segments(h)
    xy = all_pixels()
    n, m, p = len(o), len(a), len(xy)
    with Renderer(W, H, h.S, h.AA) as r:
        r.upload_header(h)
        r.set_query_tree(True)
        want, wpix, wocc = r.trace_rays(o, d, 0.0), r.trace_pixels(xy, 0.0), r.occluded(a, b)
        ws, ts = r.query_workspace_bytes(), r.query_tree_stats()
        assert ts["nodes"] > 0
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
        d_o, d_d, d_a, d_b, d_xy = dev(o), dev(d), dev(a), dev(b), dev(xy)
        t, ind = torch.zeros(max(n, p), dtype=torch.float32, device="cuda"), torch.zeros(max(n, p), dtype=torch.int32, device="cuda")
        nrm, dirs = torch.zeros(3 * max(n, p), dtype=torch.float32, device="cuda"), torch.zeros(3 * p, dtype=torch.float32, device="cuda")
        out = torch.zeros(m, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            r.trace_rays_device(d_o.data_ptr(), d_d.data_ptr(), n, 0.0, t.data_ptr(), ind.data_ptr(), nrm.data_ptr())
            r.synchronize()
            assert t[:n].cpu().numpy().tobytes() == want.t.tobytes() and ind[:n].cpu().numpy().tobytes() == want.ind.tobytes()
            assert nrm[:3 * n].cpu().numpy().tobytes() == want.normals.tobytes()
            r.trace_pixels_device(d_xy.data_ptr(), p, 0.0, t.data_ptr(), ind.data_ptr(), nrm.data_ptr(), dirs.data_ptr())
            r.occluded_device(d_a.data_ptr(), d_b.data_ptr(), m, out.data_ptr())
            r.synchronize()
            assert t[:p].cpu().numpy().tobytes() == wpix.t.tobytes() and ind[:p].cpu().numpy().tobytes() == wpix.ind.tobytes()
            assert nrm[:3 * p].cpu().numpy().tobytes() == wpix.normals.tobytes()
            assert dirs.cpu().numpy().tobytes() == wpix.dirs.tobytes()
            assert out.cpu().numpy().astype(bool).tobytes() == wocc.tobytes()
            assert r.query_workspace_bytes() == ws and r.query_tree_stats() == ts  # nothing allocated, nothing rebuilt


# ---- header changes ----------------------------------------------------------------------------
def test_header_changes_rebuild_the_tree():
    h1, h2 = box_scene(300, seed=5), box_scene(300, seed=6)
    o, d = ray_sets(h1)
    with Renderer(W, H, h1.S, h1.AA) as r:
        r.set_query_tree(True)
        assert r.query_tree and r.query_tree_stats()["nodes"] == 0 and r.query_tree_stats()["bytes"] > 0
        with pytest.raises(RtError) as e:                 # no header yet
            r.trace_rays(o, d)
        assert e.value.status == _lib.RT_E_STATE
        for h in (h1, h2, h1):
            r.upload_header(h)
            against_host(r.trace_rays(o[:512], d[:512], 0.0), trace_rays_host(h, o[:512], d[:512], 0.0), "after an upload")
        s1, s2 = trace_rays_host(h1, o[:512], d[:512], 0.0), trace_rays_host(h2, o[:512], d[:512], 0.0)
        assert not np.array_equal(s1.ind, s2.ind)
        # a render loop that moves the light: one structure, frame after frame
        hh = h2.copy()
        f = r.compute_frames(hh, 3, 0, 1, 7000, True)
        st = r.query_tree_stats()
        for _ in range(3):
            f = r.compute_frames(hh, 3, f, 1, 7000, True)
            assert r.query_tree_stats() == st
        f = r.compute_frames(hh, 3, f, 4, 7000, True)
        assert r.query_tree_stats() == st and st["nodes"] > 0
        g = r.trace_rays(o, d, 0.0)
        r.set_query_tree(False)
        assert r.query_tree_stats() == {"nodes": 0, "leaves": 0, "always": 0, "bytes": 0}
        raw_equal(g, r.trace_rays(o, d, 0.0), "after 8 mode-3 frames")
        against_host(subset(g, slice(0, 512)), s2, "after 8 mode-3 frames")
        # the rectangles switch packs the header again: the tree follows
        r.set_query_tree(True)
        r.set_rectangles(True)
        assert r.query_tree_stats()["nodes"] == st["nodes"]
        against_host(r.trace_rays(o[:512], d[:512], 0.0), s2, "after the rectangles switch")


# ---- strips ------------------------------------------------------------------------------------
def test_strips_answer_as_the_whole_frame():
    import torch

    h = scene("mixed")
    o, d = ray_sets(h)
    xy = all_pixels()
    ndev = max(1, torch.cuda.device_count())
    with Renderer(W, H, h.S, h.AA) as r, Renderer(W, H, h.S, h.AA, rows=(5, 23)) as strip, \
            StripGroup(W, H, h.S, h.AA, [i % ndev for i in range(3)]) as g:
        for c in (r, strip):
            c.upload_header(h)
            c.set_query_tree(True)
        want, wpix = r.trace_rays(o, d, 0.0), r.trace_pixels(xy, 0.0)
        raw_equal(strip.trace_rays(o, d, 0.0), want, "a strip context")
        raw_equal(strip.trace_pixels(xy, 0.0), wpix, "a strip context, pixels")
        assert strip.query_tree_stats() == r.query_tree_stats()
        g.set_query_tree(True)
        g.upload_header(h)
        lib = _lib.load()
        t, ind = np.zeros(len(o), F32), np.zeros(len(o), np.int32)

        def check(where):
            for i in range(3):
                ctx = g.strip_ctx(i)
                assert lib.rt_query_tree(ctx) == 1, where
                assert lib.rt_upload_header(ctx, h.data.ctypes.data_as(C.c_void_p), h.data.nbytes) == 0
                assert lib.rt_trace_rays(ctx, _lib.fptr(o), _lib.fptr(d), len(o), 0.0, _lib.fptr(t),
                                         ind.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
                assert t.tobytes() == want.t.tobytes() and ind.tobytes() == want.ind.tobytes(), f"{where}: strip {i}"
                n = C.c_int()
                assert lib.rt_query_tree_stats(ctx, C.byref(n), None, None, None) == 0 and n.value == r.query_tree_stats()["nodes"]

        check("a new group")
        g.set_bounds([0, 10, 30, H])
        check("after rt_group_set_bounds")


# ---- the tree kernels' decisions alone ---------------------------------------------------------
def selftest(fn, inp, n):
    with Renderer(16, 16, 4, 1) as r:
        return r.selftest_math(fn, inp, n)


def test_cull_tree_on_the_cluster_cases():
    inp = cc.cluster()["inp"]
    n = len(inp)
    assert n % 64 == 0
    tree = selftest(_lib.RT_MATH_CULL_TREE, inp, n).reshape(n, 3)
    cluster = selftest(_lib.RT_MATH_CULL_CLUSTER, inp, n).reshape(n, 3)
    gate, may, t = tree[:, 0], tree[:, 1], tree[:, 2]
    assert set(np.unique(gate)) <= {0.0, 1.0} and set(np.unique(may)) <= {0.0, 1.0}
    culled = may == 0
    print(f"RT_MATH_CULL_TREE: {n} cases, gate passes {int(gate.sum())}, culled {int(culled.sum())}, "
          f"accepted at threshold 0 {int((t != -1).sum())}")
    bad = culled & (t != -1)                              # a culled ball's member is never accepted, at threshold 0
    assert not bad.any(), f"{int(bad.sum())} culled cases accept their member; first: case {int(np.flatnonzero(bad)[0])}"
    g = gate == 1
    assert np.array_equal(may[g], cluster[g, 0])          # behind the gate: cluster_may_hit itself
    assert (may[~g] == 1).all()                           # a direction that fails the gate keeps the ball
    assert culled.any() and (t != -1).any() and g.any()   # no vacuity


def test_the_unit_gate():
    rng = np.random.default_rng(12)
    n = 65536
    v = unit(rng, n).astype(np.float64) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    d = selftest(_lib.RT_MATH_NORMALIZE, v.astype(F32), n).reshape(n, 3)
    inp = np.zeros((n, 14), F32)
    inp[:, 3:6] = d
    inp[:, 6:10] = (0, 0, -5, 1)
    inp[:, 10:14] = (0, 0, -5, 0.5)
    gate = selftest(_lib.RT_MATH_CULL_TREE, inp, n).reshape(n, 3)[:, 0]
    assert (gate == 1).all(), f"{int((gate != 1).sum())} of {n} normalised directions fail the unit gate"
    for scale in (1.0 + 1e-6, 1.0 - 1e-6):
        inp[:, 3:6] = d * F32(scale)
        gate = selftest(_lib.RT_MATH_CULL_TREE, inp, n).reshape(n, 3)[:, 0]
        assert (gate == 0).all(), f"scale {scale}: {int((gate != 0).sum())} directions pass the unit gate"
    inp[:64, 3:6] = [[np.nan, 0, 1], [0, 0, 0], [np.inf, 0, 0], [0.5, 0, 0]] * 16
    out = selftest(_lib.RT_MATH_CULL_TREE, inp[:64], 64).reshape(64, 3)
    assert (out[:, 0] == 0).all() and (out[:, 1] == 1).all()
    with Renderer(16, 16, 4, 1) as r:                     # its cases come in whole waves, as RT_MATH_CULL_CLUSTER's
        with pytest.raises(RtError) as e:
            r.selftest_math(_lib.RT_MATH_CULL_TREE, inp[:63], 63)
        assert e.value.status == _lib.RT_E_INVAL


# ---- the headless driver -----------------------------------------------------------------------
def test_headless_pick_through_the_tree():
    import subprocess

    from conftest import ROOT

    exe = ROOT / "build" / "rt_headless"
    if not exe.exists():
        subprocess.run(["make", "-C", str(ROOT), "headless"], check=True, capture_output=True)
    h = Header.synthetic(64, 4, 1234, ASPECT)  # rt_headless's scene
    with Renderer(W, H, h.S, h.AA) as r:
        r.upload_header(h)
        q = r.trace_pixels([[20, 15], [40, 30]], 0.0)
        r.set_query_tree(True)
        assert r.query_tree_stats()["nodes"] > 0
    assert (q.ind >= 0).any()
    for k, xy in enumerate(((20, 15), (40, 30))):
        want = "pick %d %d %d " % (xy[0], xy[1], q.ind[k]) + " ".join("%.9g" % float(v) for v in (q.t[k], *q.normals[k]))
        for on in (0, 1):
            p = subprocess.run([str(exe), "--width", str(W), "--height", str(H), "--scene", "synthetic", "--objects", "64",
                                "--mode", "3", "--frames", "1", "--pick", f"{xy[0]},{xy[1]}", "--query-tree", str(on)],
                               capture_output=True, text=True, timeout=120)
            assert p.returncode == 0, p.stderr
            assert p.stdout.splitlines()[-1] == want, f"--query-tree {on}"
