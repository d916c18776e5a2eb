"""The mesh layer on the host (include/rt/mesh.h; real_time_ray_tracer_amd/csrc/rt_mesh_host.cpp), no GPU.

The host-only unit is built without HIP under the host sanitizers next to a stand-alone program
(tests/native/mesh_cases.cpp) and run as a child process; nothing sanitized is loaded into Python.

 - the hierarchy's invariants on every mesh of tests/mesh_cases.py, from the arrays the program prints;
 - the program's own walk over the skip links = the brute-force host functions, bit for bit;
 - box_pass is monotone under containment on 1 M seeded nested boxes: 0 violations;
 - the box gate rejects no hit the ungated binary32 Moeller-Trumbore accepts with t > 1e-4;
 - the rule against an independent binary64 numpy Moeller-Trumbore without a gate;
 - merge and one-origin semantics, argument checks;
 - the companion library's census: its kernels, its exports, their ctypes signatures."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_cases
from conftest import ROOT
from kernel_forms import normalise
from real_time_ray_tracer_amd import (Header, aspect_for, mesh, mesh_box_pass_host, mesh_bvh_host, mesh_occluded_host,
                                      mesh_trace_rays_host, mesh_tri_eval_host, trace_rays_host)
from test_present_cpu import SAN_FLAGS

CSRC = ROOT / "real_time_ray_tracer_amd" / "csrc"
NAMES = ("ico", "grid", "both", "tri1", "tri7", "tri8", "tri9", "odd", "empty")
MONO = 1 << 20
KERNELS = {"mesh_trace_kernel", "mesh_occluded_kernel"}
ARGS_EXPECTED = "args 0 -1 -1 -1 -1 -1 0 -1 -1 -1 -1 0 -1 -1 -1 0 -1 1 -1 -1 -1 0 0 0 -1"


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """One run of the sanitized program over every case: {name: parsed line}, "mono", "args"."""
    tmp = tmp_path_factory.mktemp("mesh")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp / "mesh_cases"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "mesh_cases.cpp"), str(CSRC / "rt_mesh_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    lines = []
    for name in NAMES:
        v, t = mesh_cases.meshes()[name]
        o, d, a, b, kind = mesh_cases.rays(name)
        v.tofile(tmp / f"{name}.v"), t.tofile(tmp / f"{name}.t"), kind.tofile(tmp / f"{name}.k")
        np.concatenate([o, d, a, b]).tofile(tmp / f"{name}.r")
        lines.append(f"mesh {len(v)} {len(t)} " + " ".join(str(tmp / f"{name}.{x}") for x in "vtrk") + f" {len(o)}")
    lines += [f"mono 7 {MONO}", "args"]
    (tmp / "cases.txt").write_text("".join(ln + "\n" for ln in lines))
    p = subprocess.run([str(exe), str(tmp / "cases.txt")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr}"
    assert p.stderr == ""
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)  # noqa: E731
    res = {}
    for name, ln in zip(NAMES, out):
        w = ln.split()
        assert w[0] == "mesh" and len(w) == 21, ln[:200]
        keys = ("same", "bad_trace", "bad_occ", "hits", "occluded", "pairs")
        res[name] = {"nodes": int(w[1]), "live": int(w[2]), "dead": int(w[3]),
                     "boxes": np.frombuffer(unhex(w[4]), np.float32).reshape(-1, 6),
                     "links": np.frombuffer(unhex(w[5]), np.int32).reshape(-1, 3),
                     "order": np.frombuffer(unhex(w[6]), np.int32), **{k: int(x) for k, x in zip(keys, w[7:13])},
                     "gate": {k: tuple(map(int, x.split(":"))) for k, x in zip(mesh_cases.KINDS, w[13:])}}
    res["mono"], res["args"] = out[-2], out[-1]
    return res


def tri_boxes(verts, tris):
    p = verts[tris]
    return p.min(axis=1), p.max(axis=1)


def subtree_check(c, lo, hi, k, name):
    """Checks node k's subtree in preorder; returns (next node, the leaf slots below k)."""
    skip, first, count = c["links"][k].tolist()
    assert k < skip <= c["nodes"], name
    if count > 0:
        assert skip == k + 1 and first >= 0 and first + count <= c["live"], name
        assert count <= mesh.RT_MESH_LEAF or (c["nodes"] == 1 and count < mesh.RT_MESH_SINGLE_LEAF), (name, k, count)
        slots = list(range(first, first + count))
        members = c["order"][slots]
        assert members.tolist() == sorted(members.tolist()), name
    else:
        left_end, a = subtree_check(c, lo, hi, k + 1, name)
        assert left_end < skip, name
        right_end, b = subtree_check(c, lo, hi, left_end, name)
        assert right_end == skip, name
        slots = a + b
        assert abs(len(a) - len(b)) <= 1 and len(a) <= len(b), (name, k)   # the median cut, the lower half first
        # the node's box is bitwise the min / max of its two children's
        kids = c["boxes"][[k + 1, left_end]]
        assert np.array_equal(c["boxes"][k, :3].view(np.uint32), kids[:, :3].min(axis=0).view(np.uint32)), (name, k)
        assert np.array_equal(c["boxes"][k, 3:].view(np.uint32), kids[:, 3:].max(axis=0).view(np.uint32)), (name, k)
    members = c["order"][slots]   # and of the triangle boxes below it
    assert np.array_equal(c["boxes"][k, :3].view(np.uint32), lo[members].min(axis=0).view(np.uint32)), (name, k)
    assert np.array_equal(c["boxes"][k, 3:].view(np.uint32), hi[members].max(axis=0).view(np.uint32)), (name, k)
    return skip, slots


def test_hierarchy_invariants(cases):
    for name in NAMES:
        c = cases[name]
        verts, tris = mesh_cases.meshes()[name]
        live = mesh_cases.live_triangles(verts, tris)
        assert c["live"] == len(live) and c["dead"] == len(tris) - len(live), name
        assert sorted(c["order"].tolist()) == live.tolist(), name          # each live triangle once, dead ones nowhere
        if len(live) == 0:
            assert c["nodes"] == 0, name
            continue
        lo, hi = tri_boxes(verts, tris)
        end, slots = subtree_check(c, lo, hi, 0, name)
        assert end == c["nodes"] and slots == list(range(c["live"])), name  # the leaves tile the leaf table in order
        assert (c["links"][:, 0] > np.arange(c["nodes"])).all(), name
        assert np.isfinite(c["boxes"]).all(), name
        assert (c["nodes"] == 1) == (len(live) < mesh.RT_MESH_SINGLE_LEAF), name
    assert cases["tri7"]["nodes"] == 1 and cases["tri7"]["links"][0].tolist() == [1, 0, 7]
    assert cases["tri8"]["nodes"] == 3                                      # an inner node and two leaves of 4
    assert cases["tri9"]["nodes"] == 5                                      # 4 | 5, the 5 cut again into 2 | 3
    assert cases["odd"]["dead"] == 2 and cases["empty"]["nodes"] == 0
    assert cases["both"]["nodes"] > 200


def test_the_build_is_deterministic_and_equals_the_library(cases):
    for name in NAMES:
        c = cases[name]
        assert c["same"] == 1, name
        got = mesh_bvh_host(*mesh_cases.meshes()[name])
        assert got["boxes"].tobytes() == c["boxes"].tobytes(), name
        assert got["links"].tobytes() == c["links"].tobytes(), name
        assert got["leaf_index"].tobytes() == c["order"].tobytes(), name


def test_the_walk_reproduces_brute_force(cases):
    for name in NAMES:
        c = cases[name]
        assert c["bad_trace"] == 0, f"{name}: {c['bad_trace']} rays differ"
        assert c["bad_occ"] == 0, f"{name}: {c['bad_occ']} segments differ"
        if name != "empty":   # both outcomes occur
            assert 0 < c["hits"] < mesh_cases.N_RAYS and 0 < c["occluded"] < mesh_cases.N_RAYS, (name, c["hits"], c["occluded"])
    assert cases["empty"]["hits"] == 0 and cases["empty"]["occluded"] == 0


def test_box_pass_is_monotone_under_containment(cases):
    print(cases["mono"])
    what, count, violations, inner_pass, outer_fail = cases["mono"].split()
    assert what == "mono" and int(count) == MONO >= 1_000_000
    assert int(violations) == 0
    # the cases decide something: many inner boxes pass, many outer boxes fail
    assert int(inner_pass) > MONO // 10 and int(outer_fail) > MONO // 10, cases["mono"]


def test_the_gate_rejects_no_accepted_hit(cases):
    """On the vertex-aimed and edge-aimed rays (and the interior ones) every hit the ungated binary32
    Moeller-Trumbore accepts with t > 1e-4, on any live triangle, passes the gate.  The other kinds'
    figures are printed: see the note on near-parallel rays in DESIGN.md, Round 20."""
    total = 0
    for name in NAMES:
        gate = cases[name]["gate"]
        print(name, gate)
        for kind in ("vertex", "edge", "interior"):
            hits, rejected = gate[kind]
            assert rejected == 0, f"{name}, {kind}: the gate rejects {rejected} of {hits} hits"
            total += hits
    assert total > 10_000 and cases["both"]["pairs"] > 1_500_000


def test_argument_checks(cases):
    assert cases["args"] == ARGS_EXPECTED
    lib = mesh.load()
    m = C.c_void_p()
    assert lib.rt_mesh_create(0, None, 0, None, 0, None) == mesh.RT_E_INVAL
    v, t = mesh_cases.meshes()["tri1"]
    bad = np.int32([[0, 1, len(v)]])
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert lib.rt_mesh_create(0, fp(v), len(v), ip(bad), 1, C.byref(m)) == mesh.RT_E_INVAL and not m.value
    assert lib.rt_mesh_create(0, fp(v), len(v), ip(t), mesh.RT_MESH_MAX_TRIANGLES + 1, C.byref(m)) == mesh.RT_E_INVAL
    assert lib.rt_mesh_create(0, fp(v), len(v), ip(t), -1, C.byref(m)) == mesh.RT_E_INVAL
    assert lib.rt_mesh_destroy(None) == mesh.RT_E_INVAL and lib.rt_mesh_stats(None, None, None, None, None) == mesh.RT_E_INVAL
    assert lib.rt_mesh_workspace_bytes(None) == 0 and lib.rt_mesh_synchronize(None) == mesh.RT_E_INVAL
    assert lib.rt_mesh_trace_rays(None, None, None, 0, 0, 0.0, None, None, None, None) == mesh.RT_E_INVAL
    assert lib.rt_mesh_occluded_device(None, None, None, None, 0, 0, None) == mesh.RT_E_INVAL
    with pytest.raises(ValueError):
        mesh_bvh_host(v, bad)


def mt64(verts, tris, o, d):
    """Binary64 Moeller-Trumbore, no gate: t [n][nt], inf for a miss."""
    p = verts[tris].astype(np.float64)
    v0, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    o, d = o.astype(np.float64)[:, None], d.astype(np.float64)[:, None]
    pv = np.cross(d, e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0[None]
        u = (s * pv).sum(-1) * inv
        q = np.cross(s, e1[None])
        v = (d * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
    ok = (det != 0) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1)
    return np.where(ok, t, np.inf)


def test_the_rule_against_binary64_numpy():
    """Rays aimed at points whose barycentrics all lie in [0.05, 0.9] (the "interior" and "scaled"
    kinds, from origins in front of the target): hit or miss and prim agree on every ray, t within
    rel 1e-4."""
    thr, seen = 1e-4, 0
    for name in ("ico", "grid", "tri1", "tri9"):
        verts, tris = mesh_cases.meshes()[name]
        o, d, _, _, kind = mesh_cases.rays(name)
        sel = np.isin(kind, [mesh_cases.KINDS.index("interior"), mesh_cases.KINDS.index("scaled")])
        o, d = o[sel], d[sel]
        h = mesh_trace_rays_host(verts, tris, o, d, thr)
        t = mt64(verts, tris, o, d)
        t = np.where(t > thr, t, np.inf)
        prim = np.where(np.isinf(t.min(axis=1)), -1, t.argmin(axis=1))
        assert (prim >= 0).all(), name   # every such ray hits what it aims at
        assert np.array_equal(h.prim, prim), (name, int((h.prim != prim).sum()))
        tref = t.min(axis=1)
        assert (np.abs(h.t - tref) <= 1e-4 * np.abs(tref)).all(), name
        seen += len(o)
    assert seen > 4000


def test_single_functions_follow_the_header():
    assert mesh_box_pass_host((0, 0, 0), (0, 0, 1), (-1, -1, 2), (1, 1, 3))
    assert not mesh_box_pass_host((0, 0, 4), (0, 0, 1), (-1, -1, 2), (1, 1, 3))          # behind: tf < 0
    assert mesh_box_pass_host((1, 0, 0), (0, 1e-40, 1), (-1, 0, 2), (1, 0, 3))            # zero axes on the planes
    assert not mesh_box_pass_host((1.0000001, 0, 0), (0, 0, 1), (-1, -1, 2), (1, 1, 3))   # a zero axis outside
    assert mesh_box_pass_host((0, 0, 0), (0, 0, 0), (-1, -1, -1), (1, 1, 1))              # no axis contributes
    v0, v1, v2 = (0, 0, 0), (1, 0, 0), (0, 1, 0)
    assert mesh_tri_eval_host((0.25, 0.5, 2), (0, 0, -1), v0, v1, v2) == (2.0, 0.25, 0.5)
    assert mesh_tri_eval_host((0.25, 0.5, -2), (0, 0, 4), v0, v1, v2) == (0.5, 0.25, 0.5)  # both faces, d as given
    assert mesh_tri_eval_host((0.75, 0.75, 2), (0, 0, -1), v0, v1, v2)[0] == -1.0
    assert mesh_tri_eval_host((0.25, 0.25, 0), (1, 0, 0), v0, v1, v2)[0] == -1.0           # in the plane: det = 0
    assert mesh_tri_eval_host((0.25, 0.25, 1), (0, 0, -1), v0, v1, (np.nan, 1, 0))[0] == -1.0


def test_merge_and_one_origin_semantics():
    verts, tris = mesh_cases.meshes()["both"]
    o, d, a, b, _ = mesh_cases.rays("both")
    plain = mesh_trace_rays_host(verts, tris, o, d, 1e-4)
    # an earlier answer from a scene of spheres, with NaN, equal and missing entries put in
    h = Header.synthetic(16, 4, 1234, aspect_for(64, 48))
    scene = trace_rays_host(h, o, d, 1e-4)
    old_t, old_n = scene.t.copy(), scene.normals.copy()
    hit = np.flatnonzero(plain.prim >= 0)
    old_t[hit[:50]] = plain.t[hit[:50]]          # ties: the earlier answer stands
    old_t[hit[50:60]] = np.nan                   # NaN: stands
    old_t[hit[60:200]] = -1.0                    # a miss: the mesh takes it
    old_t[hit[200:300]] = plain.t[hit[200:300]] * np.float32(1.5)
    got = mesh_trace_rays_host(verts, tris, o, d, 1e-4, merge=(old_t, old_n))
    with np.errstate(invalid="ignore"):
        takes = (plain.prim >= 0) & ((old_t < 0) | (plain.t < old_t))
    assert takes[hit[60:300]].all() and not takes[hit[:60]].any() and takes.sum() > 300 and (~takes).sum() > 300
    assert np.array_equal(got.t.view(np.uint32), np.where(takes, plain.t, old_t).view(np.uint32))
    assert np.array_equal(got.prim, np.where(takes, plain.prim, -1))
    assert np.array_equal(got.normals.view(np.uint32), np.where(takes[:, None], plain.normals, old_n).view(np.uint32))
    assert np.array_equal(got.uv.view(np.uint32), np.where(takes[:, None], plain.uv, 0).astype(np.float32).view(np.uint32))
    # one origin = that origin repeated
    one = mesh_trace_rays_host(verts, tris, o[:1], d, 1e-4, one_origin=True)
    rep = mesh_trace_rays_host(verts, tris, np.repeat(o[:1], len(d), axis=0), d, 1e-4)
    for x, y in ((one.t, rep.t), (one.normals, rep.normals), (one.uv, rep.uv)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(one.prim, rep.prim) and (one.prim >= 0).any()
    # occlusion: the earlier bytes are OR-ed
    occ = mesh_occluded_host(verts, tris, a, b)
    earlier = np.arange(len(a)) % 3 == 0
    assert np.array_equal(mesh_occluded_host(verts, tris, a, b, merge=earlier), occ | earlier)
    assert occ.any() and not occ.all()
    # n = 1 and n = 0
    assert mesh_trace_rays_host(verts, tris, o[:1], d[:1]).prim[0] == plain.prim[0]
    assert len(mesh_trace_rays_host(verts, tris, o[:0], d[:0]).t) == 0 and len(mesh_occluded_host(verts, tris, a[:0], b[:0])) == 0


def test_ties_go_to_the_lowest_index_and_dead_triangles_are_never_hit():
    verts, tris = mesh_cases.meshes()["odd"]
    o, d, _, _, _ = mesh_cases.rays("odd")
    h = mesh_trace_rays_host(verts, tris, o, d)
    lowest, *others = mesh_cases.ODD_DUPLICATES
    on_dup = np.flatnonzero(h.prim == lowest)
    assert len(on_dup) > 10 and not np.isin(h.prim, others).any()
    k = on_dup[0]
    for i in others:   # the copies give the same t on that ray
        assert mesh_tri_eval_host(o[k], d[k], *verts[tris[i]])[0] == h.t[k]
    dead = set(range(len(tris))) - set(mesh_cases.live_triangles(verts, tris).tolist())
    assert len(dead) == 2 and not dead & set(h.prim.tolist())
    assert not {25, 30} & set(h.prim.tolist())   # the zero-area triangles


def declared_functions():
    text = (ROOT / "include" / "rt" / "mesh.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rt_[a-z0-9_]+)\s*\(", text)))


def test_companion_census():
    """librtrt_mesh.so holds exactly the two mesh kernels, visible in nm, and exports every function
    include/rt/mesh.h declares, each with a ctypes signature."""
    lib = mesh.load()
    path = os.environ.get("RTRT_MESH_LIB", mesh.LIB_PATH)
    out = subprocess.run(["nm", "-C", str(path)], check=True, capture_output=True, text=True).stdout
    stubs = {normalise(ln.split(None, 2)[2]) for ln in out.splitlines() if "__device_stub__" in ln}
    assert stubs == KERNELS
    names = declared_functions()
    assert len(names) == 16 and all(n.startswith(("rt_mesh_", "rt_obj_")) for n in names), names
    for n in names:
        assert hasattr(lib, n), f"librtrt_mesh.so does not export {n}"
        assert n in mesh.SIGNATURES, f"{n} has no ctypes signature"
    assert sorted(mesh.SIGNATURES) == names
