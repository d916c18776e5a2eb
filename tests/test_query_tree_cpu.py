"""The ray queries' bounding-ball tree on the host (include/rt/abi.h "Query tree";
real_time_ray_tracer_amd/csrc/rt_plan.cpp build_query_tree behind rt_query_tree_host), built without
HIP under the host sanitizers next to a stand-alone program (tests/native/tree_cases.cpp) and run as
a child process.  No GPU, and nothing sanitized is loaded into Python.

 - invariants: from the arrays the program prints, on every scene: each finite sphere once across
   the leaves and the always list, NaN rows nowhere; preorder and skip links; leaf sizes; every sphere
   below a node inside the node's stored ball, in binary64; two builds equal; no tree below
   2 * kTreeLeaf members; and the same bytes from the built library's rt_query_tree_host;
 - traversal: the program's plain C traversal (skip links, a binary64 ball test without margins, the
   (t, index) merge) reproduces rt_trace_rays_host_ex on 4096 random unit rays per scene;
 - the argument checks of rt_query_tree_host and rt_set_query_tree."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from real_time_ray_tracer_amd import Header, _lib, aspect_for, query_tree_host
from test_present_cpu import SAN_FLAGS

SPP = 4
LEAF = 4  # kTreeLeaf
CSRC = ROOT / "real_time_ray_tracer_amd" / "csrc"
ASPECT = aspect_for(64, 48)


def synthetic(n, S=None, seed=1234):
    return Header.synthetic(n, SPP, seed, ASPECT, num_shapes=S if S is not None else n)


def scenes():
    # (rt_scenegen's first sphere is the ground, far above 8x the median radius: n objects give
    # n - 1 members, so 8 objects are one short of a tree and 9 have the fewest that build one)
    out = {f"gen{n}": synthetic(n) for n in (8, 9, 64, 257, 2048)}
    out["scene7"] = Header.builtin(7, SPP, ASPECT)
    h = synthetic(40)
    h.shapes[:40, 0, :3] = (1.5, -0.25, -3.0)       # every sphere at one centre
    out["one-centre"] = h
    h = synthetic(48)
    h.shapes[24:48] = h.shapes[0:24]                # duplicated rows at different indices
    out["duplicates"] = h
    h = synthetic(64)
    h.shapes[3, 0, 3] = 0.0                         # radius 0
    h.shapes[4, 0, 3] = -h.shapes[4, 0, 3]          # negative radius
    h.shapes[5, 0, 0] = np.inf                      # infinite centre
    h.shapes[6, 0, 1] = -np.inf
    h.shapes[7, 0, 3] = np.nan                      # NaN radius: never hit by the rule, packed as a NaN row, left out
    h.shapes[8, 0, 0] = np.nan                      # NaN row: left out
    h.shapes[10, 0, 3] = np.inf                     # infinite radius: a sphere whose geometry is not finite
    h.shapes[9, 0, 3] = 1000.0                      # a ground sphere: above 8x the median radius
    out["odd-rows"] = h
    h = synthetic(64)
    for i in (0, 13, 40):                           # planes and rectangles among the spheres
        h.pack_plane(i, (0, 1, 0), -2.5 - i, (0.4, 0.4, 0.4))
    for i in (1, 30, 63):
        h.pack_rectangle(i, (-4, -1, -6 - i / 8), (8, 0, 0), (0, 6, 0), (1, 1, 1))
    out["mixed"] = h
    out["nobj=0"] = synthetic(0, S=16)
    out["nobj<S"] = synthetic(20, S=64)
    h = synthetic(64)
    h.set_mode(0, 30)                               # rows beyond nobj are not the scene's
    out["nobj<rows"] = h
    out["S=0"] = Header(0, SPP)
    return out


@pytest.fixture(scope="module")
def tree_cases(tmp_path_factory):
    """Runs the sanitized program on a list of case lines; returns its output lines."""
    tmp = tmp_path_factory.mktemp("tree")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp / "tree_cases"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "tree_cases.cpp"), str(CSRC / "rt_plan.cpp"),
                        str(CSRC / "rt_host.cpp"), str(CSRC / "rt_query_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr

    def run(lines):
        f = tmp / "cases.txt"
        f.write_text("".join(ln + "\n" for ln in lines))
        p = subprocess.run([str(exe), str(f)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr}"
        assert p.stderr == ""
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out

    run.tmp = tmp
    return run


@pytest.fixture(scope="module")
def built(tree_cases):
    """{(scene, flags): parsed output} of the program, one run for every test."""
    hs = scenes()
    keys, lines = [], []
    for name, h in hs.items():
        path = tree_cases.tmp / f"{name}.bin"
        h.data.tofile(path)
        for flags in ((0, 1) if name == "mixed" else (0,)):
            keys.append((name, flags))
            lines.append(f"tree {h.S} {h.AA} {flags} {path}")
    out = {}
    for key, ln in zip(keys, tree_cases(lines)):
        what, n, e, a, balls, links, rows, index, always, same, bad, rays = ln.split()
        unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)  # noqa: E731
        assert what == "tree"
        out[key] = {"n": int(n), "e": int(e), "a": int(a), "same": int(same), "bad": int(bad), "rays": int(rays),
                    "balls": np.frombuffer(unhex(balls), np.float32).reshape(-1, 4),
                    "links": np.frombuffer(unhex(links), np.int32).reshape(-1, 4),
                    "rows": np.frombuffer(unhex(rows), np.float32).reshape(-1, 4),
                    "index": np.frombuffer(unhex(index), np.int32), "always": np.frombuffer(unhex(always), np.int32),
                    "header": hs[key[0]]}
    return out


def sphere_rows(h):
    """The packed sphere table of [0, nobj): (centre, r), NaN for every other shape and for a sphere
    whose radius is NaN (sphere_eval_ray gives NaN for it on every ray: nothing ever takes it)."""
    rows = h.shapes[:h.num_objects, 0].copy()
    rows[h.shapes[:h.num_objects, 4, 3].astype(np.int64) != 1] = np.nan
    rows[np.isnan(rows[:, 3])] = np.nan
    return rows


def members_of(rows):
    """(members, always) by the rule: NaN rows out; finite with |r| <= 8x the median |r| of the finite."""
    is_sphere = ~np.isnan(rows[:, 0])
    fin = is_sphere & np.isfinite(rows).all(axis=1)
    if fin.sum() == 0:
        return np.zeros(0, np.int64), np.flatnonzero(is_sphere)
    radii = np.sort(np.abs(rows[fin, 3]))
    big = 8.0 * float(radii[len(radii) // 2])
    mem = fin & (np.abs(rows[:, 3]) <= big)
    return np.flatnonzero(mem), np.flatnonzero(is_sphere & ~mem)


def test_every_sphere_once_and_nan_rows_nowhere(built):
    trees = 0
    for key, t in built.items():
        rows = sphere_rows(t["header"])
        mem, alw = members_of(rows)
        if t["n"] == 0:  # no tree: fewer than 2 * kTreeLeaf members, and nothing is listed
            assert len(mem) < 2 * LEAF and t["e"] == 0 and t["a"] == 0, key
            continue
        trees += 1
        assert len(mem) >= 2 * LEAF, key
        assert sorted(t["index"].tolist()) == mem.tolist(), key
        assert t["always"].tolist() == alw.tolist(), key
        assert not np.isnan(rows[t["index"], 0]).any() and not np.isnan(rows[t["always"], 0]).any(), key
        # the leaf table's rows are the spheres' rows, bit for bit
        assert np.array_equal(t["rows"].view(np.uint32), rows[t["index"]].view(np.uint32)), key
    assert trees >= 11
    g8, g9 = built[("gen8", 0)], built[("gen9", 0)]                          # the threshold, both sides
    assert g8["n"] == 0 and len(members_of(sphere_rows(g8["header"]))[0]) == 2 * LEAF - 1
    assert g9["n"] > 0 and g9["e"] == 2 * LEAF and g9["always"].tolist() == [0]
    assert built[("nobj=0", 0)]["n"] == 0 and built[("S=0", 0)]["n"] == 0
    odd = built[("odd-rows", 0)]
    assert odd["always"].tolist() == [0, 5, 6, 9, 10]   # the generator's ground, infinite centres, huge and infinite radii
    assert not {7, 8} & (set(odd["always"].tolist()) | set(odd["index"].tolist()))  # NaN radius, NaN centre: nowhere
    assert {3, 4} <= set(odd["index"].tolist())         # radius 0 and a negative radius are members
    assert built[("nobj<rows", 0)]["index"].max() < 30
    m0, m1 = built[("mixed", 0)], built[("mixed", 1)]                        # the flag changes no sphere row
    assert m0["n"] == m1["n"] and m0["balls"].tobytes() == m1["balls"].tobytes() and m0["index"].tolist() == m1["index"].tolist()


def subtree_check(t, k, key):
    """Checks node k's subtree in preorder; returns (next node, the entries below k)."""
    skip, first, count, pad = t["links"][k].tolist()
    assert pad == 0 and k < skip <= t["n"], key
    if count > 0:  # a leaf
        assert skip == k + 1 and 1 <= count <= LEAF and 0 <= first and first + count <= t["e"], key
        entries = list(range(first, first + count))
    else:          # an inner node: its two children follow in preorder and end at its skip link
        left_end, a = subtree_check(t, k + 1, key)
        assert left_end < skip, key
        right_end, b = subtree_check(t, left_end, key)
        assert right_end == skip, key
        entries = a + b
        cx, cy, cz, R = t["balls"][k].astype(np.float64)
        for child in (k + 1, left_end):  # |centre_child - centre| + R_child <= R
            c = t["balls"][child].astype(np.float64)
            assert np.sqrt((c[0] - cx) ** 2 + (c[1] - cy) ** 2 + (c[2] - cz) ** 2) + c[3] <= R, (key, k, child)
    # every sphere below the node lies inside its stored ball, in binary64
    cb = t["balls"][k].astype(np.float64)
    g = t["rows"][entries].astype(np.float64)
    reach = np.sqrt(((g[:, :3] - cb[:3]) ** 2).sum(axis=1)) + np.abs(g[:, 3])
    assert (reach <= cb[3]).all(), (key, k)
    return skip, entries


def test_preorder_skip_links_leaf_sizes_and_containment(built):
    for key, t in built.items():
        if t["n"] == 0:
            continue
        end, entries = subtree_check(t, 0, key)
        assert end == t["n"], key                             # the links partition the array
        assert entries == list(range(t["e"])), key            # the leaves' ranges tile the leaf table in order
        assert (t["links"][:, 0] > np.arange(t["n"])).all(), key
        assert np.isfinite(t["balls"][:, :3]).all() and (t["balls"][:, 3] >= 0).all(), key
    big = built[("gen2048", 0)]
    assert big["e"] == 2048 - big["a"] and big["n"] * 32 + (big["e"] + big["a"]) * 20 < 100 * 1024


def test_the_build_is_deterministic_and_equals_the_library(built):
    for key, t in built.items():
        assert t["same"] == 1, key
        got = query_tree_host(t["header"], rectangles=bool(key[1]))
        for name, mine in (("balls", "balls"), ("links", "links"), ("leaf_rows", "rows"), ("leaf_index", "index"),
                           ("always", "always")):
            assert got[name].tobytes() == t[mine].tobytes(), (key, name)


def test_plain_traversal_reproduces_the_linear_scan(built):
    hit_something = 0
    for key, t in built.items():
        assert t["rays"] == 4096 and t["bad"] == 0, f"{key}: {t['bad']} of {t['rays']} rays differ"
        hit_something += t["n"] > 0
    assert hit_something >= 11


def test_argument_checks(tree_cases):
    assert tree_cases(["args"]) == ["args -1 -1 -1 -1"]
    lib = _lib.load()
    assert lib.rt_set_query_tree(None, 1) == _lib.RT_E_INVAL
    assert lib.rt_query_tree(None) == _lib.RT_E_INVAL
    assert lib.rt_query_tree_stats(None, None, None, None, None) == _lib.RT_E_INVAL
    assert lib.rt_group_set_query_tree(None, 1) == _lib.RT_E_INVAL
    h = synthetic(64)
    cfg = _lib.rt_config(1, 1, h.S, h.AA, 1, 1, 0, 0)
    balls, links = np.zeros((128, 4), np.float32), np.zeros((128, 4), np.int32)
    rows, index, always = np.zeros((64, 4), np.float32), np.zeros(64, np.int32), np.zeros(64, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731

    e, a = C.c_int(-1), C.c_int(-1)

    def call(nbytes, flags, node_cap=128, leaf_cap=64, always_cap=64):
        return lib.rt_query_tree_host(C.byref(cfg), h.data.ctypes.data_as(C.c_void_p), nbytes, flags, _lib.fptr(balls),
                                      ip(links), node_cap, _lib.fptr(rows), ip(index), leaf_cap, ip(always), always_cap,
                                      C.byref(e), C.byref(a))

    n = call(h.data.nbytes, 0)
    assert n > 0 and e.value == 63 and a.value == 1   # (the generator's ground sphere is on the always list)
    assert call(h.data.nbytes, _lib.RT_SCENE_RECTANGLES) == n
    assert call(h.data.nbytes - 4, 0) == -1            # a short header
    assert call(h.data.nbytes, 2) == -1                # a stray flag bit
    assert call(h.data.nbytes, 0, node_cap=n - 1) == -1
    assert call(h.data.nbytes, 0, node_cap=n, leaf_cap=63, always_cap=1) == n
    assert call(h.data.nbytes, 0, leaf_cap=62) == -1
    assert call(h.data.nbytes, 0, always_cap=0) == -1
