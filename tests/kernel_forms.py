"""The kernel census as data (test infrastructure): one scenario per compiled kernel form, each with
the forms its launches must take, in launch order, written out by hand.

A form's name is what the launch log records (include/rt/abi.h "Launch log"): the kernel template and
its arguments as the library's demangled symbol spells them.  An AO form is
ao_batch_kernel<AoProd<sppc, dc, flags>>, flags the sum of

    PL 1   CLON 2   SORT 4   WIDE 8   CNT 16   MF 32   CULLC 64   RC 128

(rt_kernels_impl.h AO_*).  The numbers below are literals: nothing here calls the selector.
tests/test_kernel_census_cpu.py holds every AO row against the selector and the table's union
against the library's symbols before any GPU time is spent; tests/test_gpu_kernel_census.py runs
every row with the log on and compares the outputs with the oracle.

Scenes: make_header's spellings (synN: N spheres; synNp: N spheres and a ground plane), and synNr:
N spheres and a ground rectangle, rendered with rt_set_rectangles on.  Sphere counts: 8 (no
clusters, unsorted), 16 (clusters, unsorted), 48 (sorted), 130 (wide), 300 (wide, no clusters).
Frame sizes, the existing form tests': 40x6 and 17x5 at spp 16, 9x3 at spp 64, 40x6 at spp 4 and 8,
40x7 at spp 3: pools straddle row ends and the last pool is partial.
"""
from __future__ import annotations

from dataclasses import dataclass, field

from real_time_ray_tracer_amd import Header

POST = "post_kernel"
FILL = "cull_fill_kernel<true>"          # masks and sort frames
FILL_MASKS = "cull_fill_kernel<false>"   # the table capped: masks only


def A(sppc: int, dc: int, flags: int) -> str:
    return f"ao_batch_kernel<AoProd<{sppc}, {dc}, {flags}u>>"


@dataclass(frozen=True)
class Scenario:
    id: str
    kind: str                  # ao | shade | rays | pixels | occluded | present | present_scaled | convert | selftest
    forms: tuple               # the launches' forms, in order
    scene: str = "syn16"
    spp: int = 4
    W: int = 33
    H: int = 17
    D: int = 20
    mode: int = 1
    counters: bool = False
    batch: int = 0             # rt_set_frame_batch; > 0: the frames go through rt_compute_frames
    gbuf: bool = False         # rt_set_phong_gbuffer
    tree: bool = False         # rt_set_query_tree
    cap: int = 0               # rt_debug_cull_cache_cap, bytes
    frames: int = 2            # frames rendered (batch > 0: per rt_compute_frames call, `calls` calls)
    calls: int = 1
    ao: tuple = field(default=())  # an AO row's (uncached flags, cached flags or None, sppc, dc), for the CPU check

    @property
    def rects(self) -> bool:
        return self.scene.endswith("r")


def make_scene(name: str, W: int, H: int, spp: int) -> Header:
    """make_header's scenes, and synNr: N synthetic spheres on a ground rectangle (rect_cases.wide's floor)."""
    from test_gpu_parity import make_header  # (a GPU test module; importing it needs no GPU)
    if name.startswith("syn") and name.endswith("r"):
        from real_time_ray_tracer_amd import aspect_for
        n = int(name[3:-1])
        h = Header.synthetic(n, spp, 1234, aspect_for(W, H), num_shapes=n + 1)
        h.pack_rectangle(n, (-12, -2.5, 6), (24, 0, 0), (0, 0, -24), (0.4, 0.4, 0.45), reflectivity=1.0)
        h.set_mode(0, n + 1)
        return h
    return make_header(name, W, H, spp)


# ---- the AO forms ----------------------------------------------------------------------------------
# (scene, spp, W, H, D, variant, sppc, dc, uncached flags, cached flags)
# variant "": four still frames of mode 1: two uncached launches, the fill, two cached launches, the
#             post-process after each; "cnt": the same with the work counters on; "mf": mode 2, three
#             rt_compute_frames calls of four frames with frame batch 4: two uncached multi-frame
#             launches, the fill, one cached launch.
# A scene with planes or rectangles is never cached (None): two frames, or two multi-frame launches
# of two frames.
AO_ROWS = [
    # all-sphere, clusters on, unsorted (16 spheres): CLON
    ("syn16", 16, 40, 6, 20, "", 16, 20, 2, 66),
    ("syn16", 16, 17, 5, 20, "cnt", 16, 20, 18, 82),
    ("syn16", 16, 40, 6, 20, "mf", 16, 20, 34, 98),
    ("syn16", 64, 9, 3, 20, "", 64, 20, 2, 66),
    ("syn16", 64, 9, 3, 20, "cnt", 64, 20, 18, 82),
    ("syn16", 64, 9, 3, 20, "mf", 64, 20, 34, 98),
    # clusters on, sorted (48 spheres): CLON | SORT
    ("syn48", 16, 40, 6, 20, "", 16, 20, 6, 70),
    ("syn48", 16, 17, 5, 20, "cnt", 16, 20, 22, 86),
    ("syn48", 16, 40, 6, 20, "mf", 16, 20, 38, 102),
    ("syn48", 64, 9, 3, 20, "", 64, 20, 6, 70),
    ("syn48", 64, 9, 3, 20, "cnt", 64, 20, 22, 86),
    ("syn48", 64, 9, 3, 20, "mf", 64, 20, 38, 102),
    # clusters on, sorted, wide (130 spheres): CLON | SORT | WIDE
    ("syn130", 16, 40, 6, 20, "", 16, 20, 14, 78),
    ("syn130", 16, 17, 5, 20, "cnt", 16, 20, 30, 94),
    ("syn130", 16, 40, 6, 20, "mf", 16, 20, 46, 110),
    ("syn130", 64, 9, 3, 20, "", 64, 20, 14, 78),
    ("syn130", 64, 9, 3, 20, "cnt", 64, 20, 30, 94),
    ("syn130", 64, 9, 3, 20, "mf", 64, 20, 46, 110),
    # no CLON (no clusters below 16 spheres, or another depth than 20), unsorted
    ("syn8", 16, 40, 6, 20, "", 16, 0, 0, 64),
    ("syn8", 16, 17, 5, 20, "cnt", 16, 0, 16, 80),
    ("syn16", 16, 40, 6, 10, "mf", 16, 0, 32, 96),
    ("syn16", 64, 9, 3, 10, "", 64, 0, 0, 64),
    ("syn8", 64, 9, 3, 20, "cnt", 64, 0, 16, 80),
    ("syn16", 64, 9, 3, 10, "mf", 64, 0, 32, 96),
    ("syn8", 4, 40, 6, 20, "", 4, 0, 0, 64),
    ("syn16", 4, 40, 6, 20, "cnt", 4, 0, 16, 80),
    ("syn16", 4, 40, 6, 20, "mf", 4, 0, 32, 96),
    ("syn16", 3, 40, 7, 20, "", 0, 0, 0, 64),
    ("syn8", 8, 40, 6, 20, "cnt", 0, 0, 16, 80),
    ("syn16", 3, 40, 7, 20, "mf", 0, 0, 32, 96),
    # no CLON, sorted (48 spheres): SORT
    ("syn48", 16, 40, 6, 10, "", 16, 0, 4, 68),
    ("syn48", 16, 17, 5, 10, "cnt", 16, 0, 20, 84),
    ("syn48", 16, 40, 6, 10, "mf", 16, 0, 36, 100),
    ("syn48", 64, 9, 3, 10, "", 64, 0, 4, 68),
    ("syn48", 64, 9, 3, 10, "cnt", 64, 0, 20, 84),
    ("syn48", 64, 9, 3, 10, "mf", 64, 0, 36, 100),
    ("syn48", 4, 40, 6, 20, "", 4, 0, 4, 68),
    ("syn48", 4, 40, 6, 20, "cnt", 4, 0, 20, 84),
    ("syn48", 4, 40, 6, 20, "mf", 4, 0, 36, 100),
    ("syn48", 8, 40, 6, 20, "", 0, 0, 4, 68),
    ("syn48", 3, 40, 7, 20, "cnt", 0, 0, 20, 84),
    ("syn48", 8, 40, 6, 20, "mf", 0, 0, 36, 100),
    # no CLON, sorted, wide (130 spheres at depth 10; 300 spheres: no clusters): SORT | WIDE
    ("syn130", 16, 40, 6, 10, "", 16, 0, 12, 76),
    ("syn300", 16, 17, 5, 20, "cnt", 16, 0, 28, 92),
    ("syn130", 16, 40, 6, 10, "mf", 16, 0, 44, 108),
    ("syn300", 64, 9, 3, 20, "", 64, 0, 12, 76),
    ("syn130", 64, 9, 3, 10, "cnt", 64, 0, 28, 92),
    ("syn300", 64, 9, 3, 20, "mf", 64, 0, 44, 108),
    ("syn130", 4, 40, 6, 20, "", 4, 0, 12, 76),
    ("syn300", 4, 40, 6, 20, "cnt", 4, 0, 28, 92),
    ("syn130", 4, 40, 6, 20, "mf", 4, 0, 44, 108),
    ("syn130", 8, 40, 6, 20, "", 0, 0, 12, 76),
    ("syn300", 3, 40, 7, 20, "cnt", 0, 0, 28, 92),
    ("syn130", 8, 40, 6, 20, "mf", 0, 0, 44, 108),
    # a ground plane: PL; spp 64 has no form of its own with planes
    ("syn16p", 16, 40, 6, 20, "", 16, 0, 1, None),
    ("syn48p", 16, 17, 5, 20, "cnt", 16, 0, 17, None),
    ("syn16p", 16, 40, 6, 20, "mf", 16, 0, 33, None),
    ("syn16p", 4, 40, 6, 20, "", 4, 0, 1, None),
    ("syn8p", 4, 40, 6, 20, "cnt", 4, 0, 17, None),
    ("syn48p", 4, 40, 6, 20, "mf", 4, 0, 33, None),
    ("syn16p", 3, 40, 7, 20, "", 0, 0, 1, None),
    ("syn16p", 64, 9, 3, 20, "cnt", 0, 0, 17, None),
    ("syn16p", 8, 40, 6, 20, "mf", 0, 0, 33, None),
    # a ground plane, wide: PL | WIDE
    ("syn130p", 16, 40, 6, 20, "", 16, 0, 9, None),
    ("syn130p", 16, 17, 5, 20, "cnt", 16, 0, 25, None),
    ("syn300p", 16, 40, 6, 20, "mf", 16, 0, 41, None),
    ("syn130p", 4, 40, 6, 20, "", 4, 0, 9, None),
    ("syn300p", 4, 40, 6, 20, "cnt", 4, 0, 25, None),
    ("syn130p", 4, 40, 6, 20, "mf", 4, 0, 41, None),
    ("syn130p", 64, 9, 3, 20, "", 0, 0, 9, None),
    ("syn130p", 3, 40, 7, 20, "cnt", 0, 0, 25, None),
    ("syn130p", 8, 40, 6, 20, "mf", 0, 0, 41, None),
    # a ground rectangle in effect: PL | RC (depth 5: the depth is a launch parameter of these forms,
    # and the numpy reference's cost grows with it)
    ("syn16r", 16, 40, 6, 5, "", 16, 0, 129, None),
    ("syn48r", 16, 17, 5, 5, "cnt", 16, 0, 145, None),
    ("syn16r", 16, 40, 6, 5, "mf", 16, 0, 161, None),
    ("syn16r", 4, 40, 6, 5, "", 4, 0, 129, None),
    ("syn8r", 4, 40, 6, 5, "cnt", 4, 0, 145, None),
    ("syn48r", 4, 40, 6, 5, "mf", 4, 0, 161, None),
    ("syn16r", 3, 40, 7, 5, "", 0, 0, 129, None),
    ("syn16r", 64, 9, 3, 5, "cnt", 0, 0, 145, None),
    ("syn16r", 8, 40, 6, 5, "mf", 0, 0, 161, None),
    # a ground rectangle, wide: PL | RC | WIDE
    ("syn130r", 16, 40, 6, 5, "", 16, 0, 137, None),
    ("syn130r", 16, 17, 5, 5, "cnt", 16, 0, 153, None),
    ("syn130r", 16, 40, 6, 5, "mf", 16, 0, 169, None),
    ("syn130r", 4, 40, 6, 5, "", 4, 0, 137, None),
    ("syn130r", 4, 40, 6, 5, "cnt", 4, 0, 153, None),
    ("syn130r", 4, 40, 6, 5, "mf", 4, 0, 169, None),
    ("syn130r", 64, 9, 3, 5, "", 0, 0, 137, None),
    ("syn130r", 3, 40, 7, 5, "cnt", 0, 0, 153, None),
    ("syn130r", 8, 40, 6, 5, "mf", 0, 0, 169, None),
]


def _ao_scenario(row) -> Scenario:
    scene, spp, W, H, D, variant, sppc, dc, fu, fc = row
    u = A(sppc, dc, fu)
    c = A(sppc, dc, fc) if fc is not None else None
    sid = f"ao-{scene}-spp{spp}-{W}x{H}-D{D}{'-' + variant if variant else ''}"
    common = dict(scene=scene, spp=spp, W=W, H=H, D=D, ao=(fu, fc, sppc, dc))
    if variant == "mf":
        if c is None:  # two multi-frame launches of two frames
            return Scenario(sid, "ao", (u, u), mode=2, batch=4, frames=2, calls=2, **common)
        return Scenario(sid, "ao", (u, u, FILL, c), mode=2, batch=4, frames=4, calls=3, **common)
    cnt = variant == "cnt"
    if c is None:
        return Scenario(sid, "ao", (u, POST, u, POST), mode=1, counters=cnt, frames=2, **common)
    return Scenario(sid, "ao", (u, POST, u, POST, FILL, c, POST, c, POST), mode=1, counters=cnt, frames=4, **common)


AO_SCENARIOS = [_ao_scenario(r) for r in AO_ROWS]

# ---- the other kernels -----------------------------------------------------------------------------
# Modes 3 and 4 (33x17: several blocks, a one-pixel last tile column and row).  A single-frame row
# renders two frames with the moving light, one launch each; a multi-frame row three frames in one
# rt_compute_frames launch (frame batch 8).
_HY = "2, 2"  # kHyBW, kHyBW


def _shade(mode, scene, mf, gb, form) -> Scenario:
    sid = f"mode{mode}-{scene}{'-mf' if mf else ''}{'-gbuf' if gb else ''}"
    if mf:
        return Scenario(sid, "shade", (form,), scene=scene, mode=mode, gbuf=gb, batch=8, frames=3)
    return Scenario(sid, "shade", (form, form), scene=scene, mode=mode, gbuf=gb, frames=2)


SHADE_SCENARIOS = [
    _shade(3, "syn16", False, False, "phong_kernel<true, false, false, false>"),
    _shade(3, "syn16", True, False, "phong_kernel<true, false, false, true>"),
    _shade(3, "syn16p", False, False, "phong_kernel<true, true, false, false>"),
    _shade(3, "syn16p", True, False, "phong_kernel<true, true, false, true>"),
    _shade(4, "syn16", False, False, f"hybrid_kernel<true, false, false, 0, {_HY}, false>"),
    _shade(4, "syn16", True, False, f"hybrid_kernel<true, false, false, 0, {_HY}, true>"),
    _shade(4, "syn16p", False, False, f"hybrid_kernel<true, true, false, 0, {_HY}, false>"),
    _shade(4, "syn16p", True, False, f"hybrid_kernel<true, true, false, 0, {_HY}, true>"),
    _shade(3, "syn16", False, True, "phong_gbuf_kernel<false, false>"),
    _shade(3, "syn16", True, True, "phong_gbuf_kernel<false, true>"),
    _shade(3, "syn16p", False, True, "phong_gbuf_kernel<true, false>"),
    _shade(3, "syn16p", True, True, "phong_gbuf_kernel<true, true>"),
    _shade(4, "syn16", False, True, f"hybrid_gbuf_kernel<false, {_HY}, false>"),
    _shade(4, "syn16", True, True, f"hybrid_gbuf_kernel<false, {_HY}, true>"),
    _shade(4, "syn16p", False, True, f"hybrid_gbuf_kernel<true, {_HY}, false>"),
    _shade(4, "syn16p", True, True, f"hybrid_gbuf_kernel<true, {_HY}, true>"),
    _shade(3, "syn16r", False, False, "phong_rc_kernel<false, false>"),
    _shade(3, "syn16r", False, True, "phong_rc_kernel<false, true>"),
    _shade(3, "syn16r", True, False, "phong_rc_kernel<true, false>"),
    _shade(3, "syn16r", True, True, "phong_rc_kernel<true, true>"),
    _shade(4, "syn16r", False, False, f"hybrid_rc_kernel<{_HY}, false, false>"),
    _shade(4, "syn16r", False, True, f"hybrid_rc_kernel<{_HY}, false, true>"),
    _shade(4, "syn16r", True, False, f"hybrid_rc_kernel<{_HY}, true, false>"),
    _shade(4, "syn16r", True, True, f"hybrid_rc_kernel<{_HY}, true, true>"),
]

# The ray queries: one host-pointer call each, on a 33x17 frame's scene; syn64 with the tree on.
QUERY_SCENARIOS = [
    Scenario("rays-syn16", "rays", ("ray_query_kernel<false, false>",), scene="syn16"),
    Scenario("pixels-syn16", "pixels", ("ray_query_kernel<false, true>",), scene="syn16"),
    Scenario("rays-syn16p", "rays", ("ray_query_kernel<true, false>",), scene="syn16p"),
    Scenario("pixels-syn16p", "pixels", ("ray_query_kernel<true, true>",), scene="syn16p"),
    Scenario("rays-syn16r", "rays", ("ray_query_rc_kernel<false>",), scene="syn16r"),
    Scenario("pixels-syn16r", "pixels", ("ray_query_rc_kernel<true>",), scene="syn16r"),
    Scenario("rays-syn64-tree", "rays", ("ray_query_tree_kernel<false>",), scene="syn64", tree=True),
    Scenario("pixels-syn64-tree", "pixels", ("ray_query_tree_kernel<true>",), scene="syn64", tree=True),
    Scenario("occluded-syn16", "occluded", ("occluded_kernel<false>",), scene="syn16"),
    Scenario("occluded-syn16p", "occluded", ("occluded_kernel<true>",), scene="syn16p"),
    Scenario("occluded-syn16r", "occluded", ("occluded_rc_kernel",), scene="syn16r"),
    Scenario("occluded-syn64-tree", "occluded", ("occluded_tree_kernel",), scene="syn64", tree=True),
]

# The masks-only fill (the cap admits the 15 pools' masks, 120 bytes, not their 480 bytes of sort
# frames as well, as test_gpu_ao_normal_sort's test_cap_keeps_masks_only); the 8-bit presents after one
# mode-1 frame; the g-buffer layout conversion of a download and an upload; the math self-test.
OTHER_SCENARIOS = [
    Scenario("ao-syn48-masks-only", "ao", (A(16, 20, 6), POST, A(16, 20, 6), POST, FILL_MASKS, A(16, 20, 70), POST,
                                           A(16, 20, 70), POST),
             scene="syn48", spp=16, W=40, H=6, frames=4, cap=15 * 8 + 8, ao=(6, 70, 16, 20)),
    Scenario("present", "present", (A(4, 0, 0), POST, "present_kernel"), scene="syn16", spp=4, W=40, H=6, frames=1),
    Scenario("present-scaled", "present_scaled", (A(4, 0, 0), POST, "present_scaled_kernel"), scene="syn16", spp=4, W=40,
             H=6, frames=1),
    # (an upload and a download of the three arrays' eight slots: one conversion per array and slot)
    Scenario("gbuf-convert", "convert", ("gbuf_convert_kernel",) * 48, W=17, H=5),
    Scenario("selftest", "selftest", ("selftest_kernel",) * 3),  # sin, sqrt, division
]

SCENARIOS = AO_SCENARIOS + SHADE_SCENARIOS + QUERY_SCENARIOS + OTHER_SCENARIOS
assert len({s.id for s in SCENARIOS}) == len(SCENARIOS), "scenario ids are unique"


def claimed_forms() -> set:
    return {f for s in SCENARIOS for f in s.forms}


# ---- the library's kernels ---------------------------------------------------------------------------
def normalise(symbol: str) -> str:
    """A demangled host-stub symbol as a form name, the one stated normalisation: the return type, the
    namespaces, the stub prefix and the parameter list stripped, "> >" written ">>"."""
    import re
    s = symbol.strip()
    s = re.sub(r"^void ", "", s)
    s = s.replace("rt::(anonymous namespace)::", "").replace("rt::", "").replace("__device_stub__", "")
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):  # the parameter list: the first '(' outside the template arguments
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut]
    while "> >" in s:
        s = s.replace("> >", ">>")
    return s


def library_path():
    """The library the package loads (RTRT_LIB, else the in-tree build), built with `make lib` when
    absent; a library that is still missing is an error."""
    import os
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    lib = Path(os.environ.get("RTRT_LIB") or root / "real_time_ray_tracer_amd" / "librtrt.so")
    if not lib.exists():
        subprocess.run(["make", "-j", str(min(16, os.cpu_count() or 1)), "lib"], cwd=root, check=True)
    assert lib.exists(), f"{lib} is missing"
    return lib


def library_kernels() -> set:
    """The form names of the kernels the library holds, from its host stubs in `nm -C` (a missing nm
    is an error)."""
    import subprocess

    lib = library_path()
    out = subprocess.run(["nm", "-C", str(lib)], check=True, capture_output=True, text=True).stdout
    names = set()
    for line in out.splitlines():
        if "__device_stub__" in line:
            names.add(normalise(line.split(None, 2)[2]))
    assert names, f"no kernel stubs in {lib}"
    return names
