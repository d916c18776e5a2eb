"""The kernel census without a GPU (tests/kernel_forms.py is the table):

  - the AO kernels the library holds are exactly the forms the launcher's selector (rt_ao_form_host,
    ao_select itself) can return for a scene the host can upload: a kernel no launch can reach is
    compiled, linked and never tested, so it fails here by name;
  - every AO row of the table names what the selector returns for the row's own scene and switches;
  - every kernel of the library is claimed by a scenario, and no scenario claims a kernel that does
    not exist;
  - the names the launchers record are the library's own symbols.
"""
import itertools
from pathlib import Path

import pytest

import kernel_forms as kf
from real_time_ray_tracer_amd import _lib
from real_time_ray_tracer_amd.host import ao_form_host

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def compiled():
    return kf.library_kernels()


def is_ao(name: str) -> bool:
    return name.startswith("ao_batch_kernel<")


# The sweep: every boundary of the selector and of the launcher's ladder.
SPP = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256)   # around 3, 4, 8, 16, 64, 256
DEPTH = (1, 10, 19, 20)
NOBJ = (0, 1, 15, 16, 17, 47, 48, 49, 64, 65, 128, 129, 256, 257, 300)
PLANES = (0, 1, 65)
RECTS = (0, 1)
CLUSTER_RANGE = (16, 256)  # objects for which rt_cluster_table can return more than 0


def test_cluster_range():
    """ncl > 0 enters the sweep only for scenes that can have clusters: all-sphere synN headers have
    some at both ends of [16, 256] and none just outside."""
    got = {n: len(kf.make_scene(f"syn{n}", 40, 6, 16).cluster_table()[0]) for n in (8, 15, 16, 256, 257, 300)}
    assert got[16] > 0 and got[256] > 0, got
    assert got[8] == got[15] == got[257] == got[300] == 0, got


def reachable_ao_forms() -> set:
    forms = set()
    for spp, D, nobj, npl, nrc in itertools.product(SPP, DEPTH, NOBJ, PLANES, RECTS):
        if npl > nobj or nrc > npl:
            continue
        ncls = (0, 8) if CLUSTER_RANGE[0] <= nobj <= CLUSTER_RANGE[1] else (0,)
        for ncl, cnt, mf, cull in itertools.product(ncls, (False, True), (False, True), (False, True)):
            forms.add(ao_form_host(spp, D, ncl, nobj, npl, nrc, cnt, mf, cull))
    return forms


def test_compiled_ao_kernels_are_the_reachable_ones(compiled):
    have = {k for k in compiled if is_ao(k)}
    reach = reachable_ao_forms()
    unreachable, missing = sorted(have - reach), sorted(reach - have)
    print(f"{len(have)} AO kernels compiled, {len(reach)} forms reachable")
    assert not unreachable and not missing, (
        f"{len(unreachable)} compiled AO kernels that no launch can select: {unreachable}; "
        f"{len(missing)} selectable forms with no kernel: {missing}")


def scene_counts(sc):
    """(ncl, nobj, nplanes, nrects) as an upload of the scenario's header gives the launcher."""
    h = kf.make_scene(sc.scene, sc.W, sc.H, sc.spp)
    nobj = h.num_objects
    ids = h.shapes[:nobj, 4, 3].astype(int)
    nrc = int((ids == _lib.RT_SHAPE_RECTANGLE).sum()) if sc.rects else 0
    npl = int((ids == _lib.RT_SHAPE_PLANE).sum()) + nrc
    return len(h.cluster_table()[0]), nobj, npl, nrc


AO_ROWS = [s for s in kf.SCENARIOS if s.ao]


@pytest.mark.parametrize("sc", AO_ROWS, ids=[s.id for s in AO_ROWS])
def test_ao_rows_name_what_the_selector_returns(sc):
    fu, fc, sppc, dc = sc.ao
    ncl, nobj, npl, nrc = scene_counts(sc)
    mf = sc.batch > 0
    uncached = ao_form_host(sc.spp, sc.D, ncl, nobj, npl, nrc, sc.counters, mf, False)
    cached = ao_form_host(sc.spp, sc.D, ncl, nobj, npl, nrc, sc.counters, mf, True)
    assert uncached == kf.A(sppc, dc, fu), f"{sc.id}: ncl {ncl} nobj {nobj} planes {npl} rects {nrc}"
    if fc is None:  # planes: a cull table changes nothing (and the cache never hands them one)
        assert cached == uncached and npl > 0
        want = [uncached] * 2
    else:
        assert cached == kf.A(sppc, dc, fc) and npl == 0
        want = [uncached] * 2 + [cached] * (1 if mf else 2)
    assert [f for f in sc.forms if is_ao(f)] == want, sc.forms


def test_every_kernel_has_a_scenario(compiled):
    claimed = kf.claimed_forms()
    assert claimed == compiled, (f"kernels no scenario claims: {sorted(compiled - claimed)}; "
                                 f"claimed forms that are not in the library: {sorted(claimed - compiled)}")


def test_logged_names_are_the_symbols(compiled):
    """The launchers write each kernel's name beside its launch: every name of a kernel outside the
    AO family is a string of the library, and the AO family's is its format."""
    data = kf.library_path().read_bytes()
    absent = sorted(k for k in compiled if not is_ao(k) and k.encode() + b"\0" not in data)
    assert not absent, f"kernels whose name no launcher records: {absent}"
    assert b"ao_batch_kernel<AoProd<%d, %d, %uu>>\0" in data


def test_normalise():
    sym = ("void rt::(anonymous namespace)::__device_stub__ao_batch_kernel<rt::(anonymous namespace)::AoProd<16, 20, 70u> >"
           "(rt::FrameParams, HIP_vector_type<float, 4u> const*, unsigned long long const*)")
    assert kf.normalise(sym) == "ao_batch_kernel<AoProd<16, 20, 70u>>" == kf.A(16, 20, 70)
    assert kf.normalise("rt::__device_stub__present_kernel(HIP_vector_type<float, 4u> const*, unsigned int*, int)") == "present_kernel"
    assert kf.normalise("void rt::__device_stub__ray_query_kernel<false, true>(rt::RayQuery)") == "ray_query_kernel<false, true>"
