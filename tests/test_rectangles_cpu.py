"""Rectangles on the CPU (include/rt/abi.h "Rectangles"): the single primitive's known answers, the
flag-taking host functions against the numpy statement of the rule (tests/rect_cases.py) bit for
bit, and the packing into the device table.  No GPU.  The host rule and the packing also build under
the host sanitizers next to a stand-alone program (tests/native/rect_cases.cpp) that runs as a child
process; nothing sanitised is loaded into Python."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ray_query_cases as rq
import rect_cases as rc
from conftest import ROOT, assert_bitwise
from oracle import numpy_ref
from real_time_ray_tracer_amd import (Header, _lib, aspect_for, occluded_host, rectangle_eval_host, trace_rays_host)
from test_present_cpu import SAN_FLAGS

F32 = np.float32
CSRC = ROOT / "real_time_ray_tracer_amd" / "csrc"


def rect_row(llc, right, up):
    h = Header(1, 4)
    h.pack_rectangle(0, llc, right, up, (1, 1, 1))
    return h.shapes[0].copy()


def up1(x):
    return np.nextafter(F32(x), F32(np.inf))


def down1(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ---- the single primitive -----------------------------------------------------------------------
def test_known_answers():
    # axis-aligned in the plane z = -2, llc at x = y = 0 so that q = p - llc is p exactly:
    # right (4, 0, 0), up (0, 2, 0), n = (0, 0, 1); dot(right, right) = 16, dot(up, up) = 4
    sh = rect_row((0, 0, -2), (4, 0, 0), (0, 2, 0))
    assert tuple(sh[0, :3]) == (0.0, 0.0, 1.0)
    ev = lambda p, d: rectangle_eval_host(sh, p, d)  # noqa: E731
    down = (0, 0, -1)
    assert ev((2, 1, 3), down) == 5.0                                   # the centre, exact t
    assert ev((0, 1, 3), down) == 5.0 and ev((4, 1, 3), down) == 5.0    # a == 0, a == dot(right, right): inside
    assert ev((2, 0, 3), down) == 5.0 and ev((2, 2, 3), down) == 5.0    # b == 0, b == dot(up, up)
    assert ev((0, 0, 3), down) == 5.0 and ev((4, 2, 3), down) == 5.0    # corners
    assert ev((down1(0), 1, 3), down) == -1.0 and ev((up1(4), 1, 3), down) == -1.0  # one ulp outside
    assert ev((2, down1(0), 3), down) == -1.0 and ev((2, up1(2), 3), down) == -1.0
    assert ev((up1(0), 1, 3), down) == 5.0 and ev((down1(4), 1, 3), down) == 5.0    # one ulp inside
    # |den| < 0.001: parallel enough to miss, on either side of zero; at 0.001 it is tested
    for dz in (0.0, 0.0009, -0.0009):
        assert ev((2, 1, 3), (1, 0, dz)) == -1.0
    assert ev((2, 1, 3), (0, 0, -0.001)) == F32(-5.0) / F32(-0.001)
    # behind the origin: the negative t comes back (the thresholds reject it)
    assert ev((2, 1, 3), (0, 0, 1)) == -5.0
    # both faces
    assert ev((2, 1, -7), (0, 0, 1)) == 5.0 and ev((2, 1, -7), down) == -5.0
    # NaN and inf operands: a miss
    nan, inf = float("nan"), float("inf")
    assert ev((nan, 1, 3), down) == -1.0 and ev((2, 1, 3), (0, nan, -1)) == -1.0
    assert ev((inf, 1, 3), down) == -1.0 and ev((2, 1, inf), down) == -1.0
    assert ev((2, 1, 3), (inf, 0, -1)) == -1.0
    for k in ((3, 0), (2, 1), (1, 2), (0, 0)):  # llc, right, up, n
        bad = sh.copy()
        bad[k] = nan
        assert rectangle_eval_host(bad, (2, 1, 3), down) == -1.0, k
    bad = sh.copy()
    bad[2, 0] = inf  # an infinite right: whatever the arithmetic gives, as the numpy rule
    assert_bitwise(F32(rectangle_eval_host(bad, (2, 1, 3), down)), rc.rect_eval(bad, [[2, 1, 3]], [down])[0], "inf right")


def test_primitive_equals_the_numpy_rule():
    rng = np.random.default_rng(3)
    for name, llc, right, up in (("tilted", rc.OCC_RECT["llc"], rc.OCC_RECT["right"], rc.OCC_RECT["up"]),
                                 ("skew", (-2, 1, 3), (4, 0, 0), (1.5, 3, 0)), ("tiny", (0, 0, 0), (1e-3, 0, 0), (0, 2e-3, 0))):
        sh = rect_row(llc, right, up)
        h = Header(1, 4)
        h.shapes[0] = sh
        pts = rc.rect_points(h, 400, seed=9)
        o = rng.uniform(-12, 12, (len(pts), 3)).astype(F32)
        d = rc.oracle.normalize3_n((pts - o).astype(F32))
        want = rc.rect_eval(sh, o, d)
        got = np.array([rectangle_eval_host(sh, o[k], d[k]) for k in range(len(o))], F32)
        assert_bitwise(got, want, name)
        assert (want > 0).mean() > 0.3 and (want == -1).mean() > 0.05, name


# ---- the flag-taking host functions -------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.QUERY_SCENES))
def test_trace_and_occlusion_against_the_numpy_rule(name):
    h = rc.QUERY_SCENES[name]()
    o, d = rc.query_rays(h)
    assert len(o) >= 2500
    hit_rect = 0
    for thr in rc.THRESHOLDS:
        t, ind, nrm = rc.expected_hits(h, o, d, thr)
        g = trace_rays_host(h, o, d, thr, rectangles=True)
        assert np.array_equal(g.ind, ind), f"{name} thr {thr}: ind differs at {np.flatnonzero(g.ind != ind)[:5]}"
        assert_bitwise(g.t, t, f"{name} thr {thr}: t")
        assert_bitwise(g.normals, nrm, f"{name} thr {thr}: normals")
        hit_rect += int((rq.ids(h)[np.maximum(ind, 0)][ind >= 0] == 3).sum())
        # flags = 0: today's function, and today's rule (a rectangle is never hit)
        g0, p0 = trace_rays_host(h, o, d, thr, rectangles=False), rc.expected_hits(h, o, d, thr, rectangles=False)
        assert np.array_equal(g0.ind, p0[1]) and not (rq.ids(h)[np.maximum(g0.ind, 0)][g0.ind >= 0] == 3).any()
        assert_bitwise(g0.t, p0[0], f"{name} thr {thr}: t, flags 0")
    if name in ("beyond", "nan-llc", "tie-plane-first"):  # (the coplanar plane's lower index wins every tie)
        assert hit_rect == 0, f"{name}: the rectangle must never be hit"
    else:
        assert hit_rect > 0, f"{name}: no ray hit a rectangle"
    a, b = rc.segments(h)
    occ, known = rc.expected_occluded(h, a, b)
    assert known.mean() > 0.999
    got = occluded_host(h, a, b, rectangles=True)
    assert np.array_equal(got[known], occ[known]), f"{name}: {int((got != occ)[known].sum())} segments differ"
    e0, k0, _ = rq.expected_occluded(h, a, b)
    got0 = occluded_host(h, a, b)
    assert np.array_equal(got0[k0], e0[k0])
    if name in ("occluder", "skew", "light5", "wide"):
        assert (got & ~got0).any(), f"{name}: no segment is occluded by a rectangle alone"
    if name in ("beyond", "nan-llc"):
        assert np.array_equal(got, got0)


def test_flags_zero_is_the_plain_function():
    lib = _lib.load()
    h = rc.occluder()
    o, d = rc.query_rays(h, 300)
    n = len(o)
    cfg = _lib.rt_config(1, 1, h.S, h.AA, 1, 1, 0, 0)
    hp, nb = h.data.ctypes.data_as(C.c_void_p), h.data.nbytes
    fp, ip = _lib.fptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    outs = []
    for ex in (False, True):
        t, ind, nrm, occ = np.zeros(n, F32), np.zeros(n, np.int32), np.zeros((n, 3), F32), np.zeros(n, np.uint8)
        if ex:
            assert lib.rt_trace_rays_host_ex(C.byref(cfg), hp, nb, fp(o), fp(d), n, 0.001, 0, fp(t), ip(ind), fp(nrm)) == 0
            assert lib.rt_occluded_host_ex(C.byref(cfg), hp, nb, fp(o), fp(d), n, 0, vp(occ)) == 0
        else:
            assert lib.rt_trace_rays_host(C.byref(cfg), hp, nb, fp(o), fp(d), n, 0.001, fp(t), ip(ind), fp(nrm)) == 0
            assert lib.rt_occluded_host(C.byref(cfg), hp, nb, fp(o), fp(d), n, vp(occ)) == 0
        outs.append((t, ind, nrm, occ))
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes()
    E = _lib.RT_E_INVAL
    t, ind, nrm, occ = outs[0]
    for bad in (2, 3, -1, 1 << 30):
        assert lib.rt_trace_rays_host_ex(C.byref(cfg), hp, nb, fp(o), fp(d), n, 0.0, bad, fp(t), ip(ind), fp(nrm)) == E
        assert lib.rt_occluded_host_ex(C.byref(cfg), hp, nb, fp(o), fp(d), n, bad, vp(occ)) == E
    assert lib.rt_trace_rays_host_ex(C.byref(cfg), hp, nb, None, fp(d), n, 0.0, 1, fp(t), ip(ind), fp(nrm)) == E
    assert lib.rt_trace_rays_host_ex(C.byref(cfg), hp, nb, fp(o), fp(d), n, -1.0, 1, fp(t), ip(ind), fp(nrm)) == E
    assert lib.rt_occluded_host_ex(C.byref(cfg), hp, nb - 4, fp(o), fp(d), n, 1, vp(occ)) == E


def test_cover_equals_its_plane_twin():
    hp, hr = rc.cover_pair()
    o, d = rc.query_rays(hp)
    for thr in rc.THRESHOLDS:
        gp, gr = trace_rays_host(hp, o, d, thr), trace_rays_host(hr, o, d, thr, rectangles=True)
        assert np.array_equal(gp.ind, gr.ind) and (gp.ind == 4).any()
        assert_bitwise(gr.t, gp.t, f"cover thr {thr}: t")
        assert_bitwise(gr.normals, gp.normals, f"cover thr {thr}: normals")
    a, b = rc.segments(hp)
    assert np.array_equal(occluded_host(hp, a, b), occluded_host(hr, a, b, rectangles=True))


@pytest.mark.parametrize("rect_first", [True, False])
def test_tie_the_lowest_index_wins(rect_first):
    h = rc.tie(rect_first)
    # rays from above into the rectangle's footprint on the plane: both are hit at the same t
    rng = np.random.default_rng(4)
    p = np.stack([rng.uniform(-5.5, 5.5, 300), np.full(300, -4.0), rng.uniform(-5.5, 5.5, 300)], 1).astype(F32)
    o = (p + np.array([0, 6, 0], F32) + rng.uniform(-2, 2, (300, 3)).astype(F32) * np.array([1, 0, 1], F32)).astype(F32)
    d = rc.oracle.normalize3_n((p - o).astype(F32))
    res = rc.eval_all(h, o, d)
    both = (res[4] == res[5]) & (res[4] > 0)
    assert both.mean() > 0.9
    g = trace_rays_host(h, o, d, 0.0001, rectangles=True)
    # (a sphere may be nearer; of the two coplanar shapes the lower index wins every exact tie)
    assert (g.ind != 5).all() and (g.ind[both] == 4).sum() > 50
    assert rq.ids(h)[4] == (3 if rect_first else 5)


def test_python_surface():
    assert _lib.RT_SCENE_RECTANGLES == 1
    h7, h5 = Header.builtin(7, 4), Header.builtin(5, 4)
    assert h7.num_objects == 3 and rq.ids(h7)[:3].tolist() == [3, 1, 1]
    assert np.array_equal(h7.shapes[1:3], h5.shapes[1:3]) and np.array_equal(h7.data[:28], h5.data[:28])
    r = h7.shapes[0]
    assert tuple(r[3, :3]) == (4, 6, 4) and tuple(r[2, :3]) == (0, 0, -8) and tuple(r[1, :3]) == (-8, 0, 0)
    assert tuple(r[4, :3]) == (1.5, 1.5, 1.5) and r[1, 3] == 1.0 and tuple(r[0, :3]) == (0.0, 1.0, 0.0)
    lib = _lib.load()
    assert lib.rt_set_rectangles(None, 1) == _lib.RT_E_INVAL and lib.rt_rectangles(None) == _lib.RT_E_INVAL
    assert lib.rt_group_set_rectangles(None, 1) == _lib.RT_E_INVAL
    assert lib.rt_init_scene(_lib.fptr(h7.data), 2, 4, 7, C.c_float(1.0)) == _lib.RT_E_INVAL


# ---- packing, and the stand-alone program under the host sanitizers ------------------------------
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rect")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp / "rect_cases"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "rect_cases.cpp"), str(CSRC / "rt_query_host.cpp"),
                        str(CSRC / "rt_plan.cpp"), str(CSRC / "rt_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(h, a, b, thr, tag):
        hdr, rays = tmp / f"{tag}.hdr", tmp / f"{tag}.rays"
        h.data.tofile(hdr)
        np.concatenate([a, b], axis=1).astype(F32).tofile(rays)
        p = subprocess.run([str(exe), str(hdr), str(h.S), str(h.AA), str(rays), str(len(a)), repr(thr)],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr}"
        assert p.stderr == ""
        lines = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines()}
        assert list(lines) == ["trace", "occ", "eval", "pack0", "pack0x", "pack1", "nulls"] and lines["nulls"] == ["ok"]
        return lines

    return run


def unhex(s):
    return b"" if s == "-" else bytes.fromhex(s)


def table_layout(S, spp):
    """Offsets in rows (rt_table.h): plane table, rand_buffer's end = the rectangle region, the end."""
    Sc = max(S, 1) + 1
    camrel = 7 * Sc + 64 + (1 + 64) * 4 // 2
    rect = camrel + Sc + 2 * spp
    return Sc, 5 * Sc, rect, rect + 2 * Sc


@pytest.mark.parametrize("scene,n", [("occluder", 257), ("manyrects", 64), ("nan-llc", 1), ("cover", 0)])
def test_under_the_host_sanitizers_and_packing(sanitized, scene, n):
    """Every buffer an exact-size heap block: the program runs clean; its answers are the library
    build's byte for byte; without the flag the packed table is the plain call's; with it the plane
    table holds planes and rectangles in ascending index and the appended rows the stated values."""
    h = rc.QUERY_SCENES[scene]()
    a, b = rc.query_rays(h, max(n, 1), seed=5)
    a, b = a[-n:] if n else a[:0], b[-n:] if n else b[:0]  # the tail: the rays aimed at edges and corners
    thr = 0.0001
    out = sanitized(h, a, b, thr, f"{scene}_{n}")
    g = trace_rays_host(h, a, b, thr, rectangles=True)
    assert unhex(out["trace"][0]) == g.t.tobytes() and unhex(out["trace"][1]) == g.ind.tobytes()
    assert unhex(out["trace"][2]) == g.normals.tobytes()
    assert unhex(out["occ"][0]) == occluded_host(h, a, b, rectangles=True).astype(np.uint8).tobytes()
    sid = rq.ids(h)
    row = int(out["eval"][0])
    assert row == int(np.flatnonzero(sid == 3)[0])
    assert_bitwise(np.frombuffer(unhex(out["eval"][1]), F32), rc.rect_eval(h.shapes[row], a, b), "eval")
    # packing
    Sc, plane0, rect0, end = table_layout(h.S, h.AA)
    t0 = np.frombuffer(unhex(out["pack0"][1]), F32).reshape(-1, 4)
    t0x = np.frombuffer(unhex(out["pack0x"][2]), F32).reshape(-1, 4)
    t1 = np.frombuffer(unhex(out["pack1"][2]), F32).reshape(-1, 4)
    assert len(t0) == len(t0x) == rect0 and len(t1) == end
    assert t0.tobytes() == t0x.tobytes(), "flags = 0 packs the plain call's table"
    nobj = h.num_objects
    planes = [i for i in range(nobj) if sid[i] == 5]
    both = [i for i in range(nobj) if sid[i] in (3, 5)]
    assert int(out["pack0"][0]) == int(out["pack0x"][0]) == len(planes) and int(out["pack0x"][1]) == 0
    assert int(out["pack1"][0]) == len(both) and int(out["pack1"][1]) == len(both) - len(planes)

    def entries(tab, idx, with_rects):
        rows, rr, k = [], [], 0
        for i in idx:
            s = h.shapes[i]
            off = 0
            if sid[i] == 3 and with_rects:
                off = rect0 - plane0 + 2 * k
                k += 1
                right, up = s[2, :3], s[1, :3]
                with np.errstate(all="ignore"):
                    rr.append(np.append(right, numpy_ref.dot3(right[None], right[None])[0]))
                    rr.append(np.append(up, numpy_ref.dot3(up[None], up[None])[0]))
            rows.append(np.append(s[0, :3], np.array([i], np.int32).view(F32)))
            rows.append(np.append(s[3, :3], np.array([off], np.int32).view(F32)))
        return np.array(rows, F32).reshape(-1, 4), np.array(rr, F32).reshape(-1, 4)

    e0, _ = entries(t0, planes, False)
    assert_bitwise(t0[plane0:plane0 + len(e0)], e0, "plane table, switch off")
    e1, r1 = entries(t1, both, True)
    assert_bitwise(t1[plane0:plane0 + len(e1)], e1, "plane table, switch on: ascending index")
    assert_bitwise(t1[rect0:rect0 + len(r1)], r1, "rectangle rows")
    assert not t1[rect0 + len(r1):].view(np.uint32).any(), "the region's unused rows are zero"
    # everything else of the table is the same with and without the switch
    keep = np.ones(rect0, bool)
    keep[plane0:plane0 + 2 * Sc] = False
    assert t1[:rect0][keep].tobytes() == t0[keep].tobytes()
