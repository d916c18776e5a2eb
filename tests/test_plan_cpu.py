"""The shim's planning code (real_time_ray_tracer_amd/csrc/rt_plan.cpp: header packing, the cull
cache's key, the tile schedule's ordering step, rt_compute_frames' table slots) built without HIP
under the host sanitizers next to a stand-alone program (tests/native/plan_cases.cpp) and run as a
child process.  No GPU, and nothing here is loaded into Python.

 - packing: cull_key's bytes and pack_header's cluster table and masks equal what the built library
   returns from rt_cull_key / rt_cluster_table for the same header;
 - order step: against a numpy restatement, argsort(-max over slots, kind="stable") packed x | y << 16;
 - slot step: the properties rt_compute_frames relies on."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from real_time_ray_tracer_amd import Header, _lib, aspect_for
from test_present_cpu import SAN_FLAGS

W, H, SPP = 40, 12, 16
CSRC = ROOT / "real_time_ray_tracer_amd" / "csrc"


@pytest.fixture(scope="module")
def plan_cases(tmp_path_factory):
    """Runs the sanitized program on a list of case lines; returns its output lines."""
    tmp = tmp_path_factory.mktemp("plan")
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run([cxx, *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if p.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip(f"{cxx} cannot link a sanitizer runtime that starts here")
    exe = tmp / "plan_cases"
    p = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *SAN_FLAGS, f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "plan_cases.cpp"), str(CSRC / "rt_plan.cpp"),
                        str(CSRC / "rt_host.cpp"), "-o", str(exe)], capture_output=True, text=True)
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


# ---- packing ------------------------------------------------------------------------------------
def scene(nobj, S=None, seed=1234):
    return Header.synthetic(nobj, SPP, seed, aspect_for(W, H), num_shapes=S if S is not None else nobj)


def headers():
    out = {"S=0": Header(0, SPP), "nobj=0": scene(0, S=8)}
    out["S=0"].fill_rand_buffer(3)
    for n in (15, 16, 256, 257):  # kClusterMinObj - 1 / kClusterMinObj; 64 * kClusterWords / one more
        out[f"nobj={n}"] = scene(n)
    h = scene(64)
    h.pack_plane(9, (0, 1, 0), -2.5, (0.4, 0.4, 0.4))
    out["plane"] = h
    h = scene(64)
    h.shapes[3, 0, 0] = np.nan
    out["nan-row"] = h
    h = scene(64)
    h.shapes[5, 0, 3] = np.inf
    h.shapes[6, 0, 1] = -np.inf
    out["inf-row"] = h
    h = scene(64)
    h.shapes[:, 0, 3] = 0.5
    out["equal-radii"] = h
    out["strip"] = scene(32)
    return out


def from_library(h, rows):
    lib = _lib.load()
    cfg = _lib.rt_config(W, H, h.S, h.AA, 8, 20, rows[0], rows[1])
    p = h.data.ctypes.data_as(C.c_void_p)
    n = lib.rt_cull_key(C.byref(cfg), p, h.data.nbytes, None, 0)
    buf = (C.c_ubyte * max(n, 1))()
    assert lib.rt_cull_key(C.byref(cfg), p, h.data.nbytes, buf, n) == n
    clusters, always, members = h.cluster_table()
    masks = np.concatenate([always[None, :], members.reshape(-1, 4)]).astype(np.uint64)
    return bytes(buf[:n]), clusters, masks


def test_packing_equals_the_library(plan_cases):
    hs = headers()
    lines, rows = [], {}
    for name, h in hs.items():
        rows[name] = (3, 9) if name == "strip" else (0, H)
        path = plan_cases.tmp / f"{name}.bin"
        h.data.tofile(path)
        lines.append(f"pack {W} {H} {h.S} {h.AA} {rows[name][0]} {rows[name][1]} {path}")
    seen_clusters = set()
    for (name, h), ln in zip(hs.items(), plan_cases(lines)):
        what, key, ncl, clusters, masks = ln.split()
        unhex = lambda s: b"" if s == "-" else bytes.fromhex(s)  # noqa: E731
        want_key, want_clusters, want_masks = from_library(h, rows[name])
        assert what == "pack"
        assert unhex(key) == want_key and len(want_key) == 6 * 4 + 8 + 2 * 4 + 4 * 12 + h.num_objects * 20, name
        assert int(ncl) == len(want_clusters), name
        assert unhex(clusters) == want_clusters.tobytes(), name
        assert unhex(masks) == want_masks.tobytes(), name
        seen_clusters.add((name, int(ncl) > 0))
    # the shapes are on both sides of the thresholds
    assert ("nobj=15", False) in seen_clusters and ("nobj=16", True) in seen_clusters
    assert ("nobj=256", True) in seen_clusters and ("nobj=257", False) in seen_clusters
    assert ("S=0", False) in seen_clusters and ("nobj=0", False) in seen_clusters


# ---- the order step -----------------------------------------------------------------------------
GX, GY, PER = 3, 2, 4


def order_ref(cost, cur):
    unit = np.asarray(cost, np.uint32).reshape(GX * GY, PER).max(axis=1)
    idx = np.argsort(-unit.astype(np.int64), kind="stable")
    packed = ((idx % GX) | ((idx // GX) << 16)).astype(np.uint32).tolist()
    return None if (unit == unit[0]).all() or packed == list(cur) else packed


def order_cases():
    rng = np.random.default_rng(5)
    distinct = rng.permutation(GX * GY * PER).astype(np.uint32) + 1
    ties = np.repeat(np.uint32([3, 7, 3, 7, 1, 7]), PER)
    ties[0::PER] = 0  # a unit's cost is its slowest slot's, not its first
    equal = np.full(GX * GY * PER, 9, np.uint32)
    plain = [x | (y << 16) for y in range(GY) for x in range(GX)]
    cases = [(distinct, []), (distinct, plain), (ties, []), (ties, plain), (equal, []), (equal, plain)]
    for cost in (distinct, ties):  # an order equal to the current one
        cases.append((cost, order_ref(cost, [])))
    return cases


def test_order_step_equals_the_numpy_restatement(plan_cases):
    cases = order_cases()
    lines = [f"order {GX} {GY} {PER} {len(cur)} " + " ".join(str(int(v)) for v in [*cur, *cost]) for cost, cur in cases]
    got = plan_cases(lines)
    nones = 0
    for (cost, cur), ln in zip(cases, got):
        want = order_ref(cost, cur)
        assert ln == ("order none" if want is None else "order " + " ".join(map(str, want)))
        nones += want is None
    assert nones == 4 and order_ref(cases[2][0], []) is not None  # equal costs x 2, unchanged orders x 2
    # ties keep the plain order: units 1, 3, 5 (cost 7), then 0, 2 (3), then 4 (1)
    assert got[2] == "order " + " ".join(str((t % GX) | ((t // GX) << 16)) for t in (1, 3, 5, 0, 2, 4))


# ---- the slot step ------------------------------------------------------------------------------
NSLOTS = 64


def slot_cases():
    rng = np.random.default_rng(11)
    pats = {1: ["0", "1"], 2: ["00", "01", "10", "11"], 4: ["".join(p) for p in itertools.product("01", repeat=4)],
            32: ["0" * 32, "1" * 32, "01" * 16, "10" * 16, "0" + "1" * 31, "1" + "0" * 31,
                 "".join(rng.choice(["0", "1"], 32)), "".join(rng.choice(["0", "1"], 32))]}
    return [(m, prev, p) for m in (1, 2, 4, 32) for prev in (-1, 0, 31, 63) for p in pats[m]]


def test_slot_step(plan_cases):
    cases = slot_cases()
    got = plan_cases([f"slots {m} {prev} {NSLOTS} {p}" for m, prev, p in cases])
    for (m, prev, p), ln in zip(cases, got):
        what, base, *slot = ln.split()
        base, slot = int(base), [int(s) for s in slot]
        assert what == "slots" and len(slot) == m
        same = [c == "1" and (j > 0 or prev >= 0) for j, c in enumerate(p)]
        assert all(0 <= s < NSLOTS for s in slot), ln
        new = [slot[j] for j in range(m) if not same[j]]
        assert new == list(range(base, base + len(new))), ln  # new tables are consecutive from base
        for j in range(m):
            if same[j]:
                assert slot[j] == (slot[j - 1] if j > 0 else prev), ln  # equal neighbours share a slot
        if same[0]:
            assert prev not in new, ln  # frame 0 reads `prev`: no new table lands on it
