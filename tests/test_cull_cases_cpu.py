"""The cull cases (tests/cull_cases.py) against the oracle alone, and the cluster table of the host.

tests/test_gpu_culls.py shows that no proof rejects a shape the exact test accepts.  That says
something only if the cases reach the proofs' boundaries from both sides and if the proofs do
reject: here the oracle shows that a good share of each family's grazing cases is hit and a good
share missed, and that the far-outside stratum is large and missed by every ray.
"""
import ctypes as C

import numpy as np
import pytest

import cull_cases as cc
from real_time_ray_tracer_amd import Header, _lib, aspect_for


def case_accepted(name):
    """Per case: the exact test accepts on the case's ray (wave families: on the tangent lane), and on
    any of its rays."""
    fam, ex = cc.FAMILIES[name](), cc.exact(name)
    acc = ex["acc"]
    if acc.ndim == 1:
        return acc, acc
    return acc[np.arange(len(acc)), fam["lane"]], acc.any(1)


@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_grazing_cases_fall_on_both_sides(name):
    fam = cc.FAMILIES[name]()
    acc, _ = case_accepted(name)
    g = fam["stratum"] == cc.GRAZING
    share = acc[g].mean()
    print(f"{name}: {g.sum()} grazing cases, {acc[g].sum()} accepted by the oracle ({share:.3f})")
    assert g.sum() >= len(g) * 0.4
    assert share >= 0.2, f"{name}: only {share:.3f} of the grazing cases are accepted"
    assert 1 - share >= 0.2, f"{name}: only {1 - share:.3f} of the grazing cases are rejected"


@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_far_outside_cases_are_many_and_all_rejected(name):
    fam = cc.FAMILIES[name]()
    _, any_acc = case_accepted(name)
    f = fam["stratum"] == cc.FAR
    print(f"{name}: {f.sum()} far-outside cases of {len(f)}, {any_acc[f].sum()} accepted by the oracle")
    assert f.mean() >= 0.1
    assert not any_acc[f].any(), f"{name}: case {np.flatnonzero(f & any_acc)[0]} is far outside and accepted"


@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_sizes_and_degenerate_rows(name):
    fam = cc.FAMILIES[name]()
    inp = fam["inp"]
    assert len(inp) == (cc.N_WAVE if name in ("bounce", "shadow") else cc.N_LANE)
    d = inp[fam["stratum"] == cc.DEGEN]
    assert np.isnan(d).any() and np.isinf(d).any()
    if name == "bounce":
        live = cc.bounce_parts(inp)[3]
        assert live.any(1).all(), "a case without a live lane is never sent"
        assert (live.sum(1) == 1).any() and (live.sum(1) == 64).any()
    if name == "shadow":
        need = cc.shadow_parts(inp)[3]
        assert need.any(1).all()
        assert (need.sum(1) == 1).any() and (need.sum(1) == 64).any()
    if name in ("shadow", "bounce"):  # ray origins on the tested sphere, and on a neighbour that touches it at one
        parts = cc.shadow_parts(inp) if name == "shadow" else cc.bounce_parts(inp)
        sph, org, on_ = (parts[1], parts[2], parts[3]) if name == "shadow" else (parts[0], parts[1], parts[3])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            gap = np.abs(np.linalg.norm(org.astype(np.float64) - sph[:, None, :3], axis=2) - sph[:, None, 3]) / sph[:, None, 3]
            touch = (gap < 1e-4) & on_
        deg = fam["stratum"] == cc.DEGEN
        assert (touch.sum(1)[deg] >= 32).sum() >= 20, "origins on the tested sphere"
        assert ((touch.sum(1)[deg] >= 1) & (touch.sum(1)[deg] <= 4)).sum() >= 20, "a neighbour touching at an origin"
    if name == "cluster":
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            gap = np.abs(np.linalg.norm(inp[:, 0:3].astype(np.float64) - inp[:, 10:13], axis=1) - inp[:, 13]) / inp[:, 13]
        deg = fam["stratum"] == cc.DEGEN
        assert (gap[deg] < 1e-4).sum() >= 2000, "origins on the member, and on a sphere the member touches there"
    if name in ("camera", "plane"):
        frames = {(int(w), int(h)) for w, h in np.unique(inp[:, 12:14], axis=0)}
        assert {(1, 1), (9, 1), (3840, 2160)} <= frames
        wh = np.unique(np.stack([inp[:, 15] - inp[:, 14] + 1, inp[:, 17] - inp[:, 16] + 1], 1), axis=0)
        assert {(1, 1), (1, 4), (64, 1)} <= {(int(a), int(b)) for a, b in wh}
    if name == "plane":
        a = inp[:, 20:23].astype(np.float64)
        with np.errstate(invalid="ignore"):
            num = (a * (inp[:, 24:27].astype(np.float64) - inp[:, 0:3])).sum(1)
        assert (num == 0).any() and (a == 0).all(1).any()
        assert (np.abs(np.linalg.norm(a, axis=1) - 2) < 1e-6).any()
        g = fam["stratum"] == cc.GRAZING
        den = np.abs((a[g] * cc.exact("plane")["dir"][g]).sum(1))
        assert (np.abs(den - 0.001) < 1e-5).mean() > 0.9


def test_table_cases_hit_and_miss():
    inp, ex = cc.cluster_tables()["inp"], cc.exact("tables")
    assert len(inp) == cc.TABLE_PAIRS and len(inp) % 64 == 0
    print(f"tables: {ex['acc'].sum()} of {len(inp)} ray-member pairs accepted by the oracle")
    assert 0.001 < ex["acc"].mean() < 0.5


# ---- rt_cluster_table against float64 arithmetic ---------------------------------------------
def bits(words):
    return {64 * w + b for w in range(len(words)) for b in range(64) if int(words[w]) >> b & 1}


@pytest.mark.parametrize("name", cc.TABLE_SCENES + ["planes32"])
def test_cluster_table_partitions_the_spheres(name):
    if name == "planes32":  # NaN rows: planes among the spheres
        h = Header.synthetic(32, 4, 99, aspect_for(64, 48))
        for i in (3, 17, 30):
            h.pack_plane(i, (0.0, 1.0, 0.0), -3.0 - i, (0.5, 0.5, 0.5))
        h.pack_sphere(5, (np.inf, 0.0, 0.0), 1.0, (0.5, 0.5, 0.5))
    else:
        h = cc.table_header(name)
    clus, always, masks = h.cluster_table()
    assert len(clus) > 0
    nobj = h.num_objects
    geo = h.shapes[:, 0].astype(np.float64)
    ids = h.shapes[:, 4, 3].astype(int)
    member_of = [bits(m) for m in masks]
    alw = bits(always)
    for i in range(h.S):
        n_in = sum(i in m for m in member_of) + (i in alw)
        if i < nobj and ids[i] == _lib.RT_SHAPE_SPHERE:
            assert n_in == 1, f"sphere {i} is in {n_in} sets"
            if not np.isfinite(geo[i]).all():
                assert i in alw
        else:
            assert n_in == 0, f"row {i} (shape id {ids[i]}) is in a set"
    for k, m in enumerate(member_of):
        assert m
        c, R = clus[k, :3].astype(np.float64), float(clus[k, 3])
        for i in m:
            assert np.linalg.norm(geo[i, :3] - c) + abs(geo[i, 3]) <= R, f"cluster {k}: member {i} sticks out"


@pytest.mark.parametrize("nobj", [15, 257])
def test_cluster_table_is_off_for_small_and_large_scenes(nobj):
    h = Header.synthetic(nobj, 4, 1234, aspect_for(64, 48))
    clus, always, masks = h.cluster_table()
    assert len(clus) == 0 and len(masks) == 0 and not always.any()
    assert len(Header.synthetic(16, 4, 1234, aspect_for(64, 48)).cluster_table()[0]) > 0
    assert len(Header.synthetic(256, 4, 1234, aspect_for(64, 48)).cluster_table()[0]) > 0


def test_cluster_table_rejects_bad_arguments():
    lib = _lib.load()
    h = Header.synthetic(64, 4, 1234, aspect_for(64, 48))
    cfg = _lib.rt_config(64, 48, h.S, h.AA, 8, 20, 0, 0)
    cl = np.zeros((64, 4), np.float32)
    mk = np.zeros((65, 4), np.uint64)
    p, mp = h.data.ctypes.data_as(C.c_void_p), mk.ctypes.data_as(C.POINTER(C.c_uint64))
    n = lib.rt_cluster_table(C.byref(cfg), p, h.data.nbytes, _lib.fptr(cl), mp, 64)
    assert n > 1
    assert lib.rt_cluster_table(C.byref(cfg), p, h.data.nbytes, _lib.fptr(cl), mp, n - 1) == -1
    assert lib.rt_cluster_table(C.byref(cfg), p, h.data.nbytes - 16, _lib.fptr(cl), mp, 64) == -1
    assert lib.rt_cluster_table(None, p, h.data.nbytes, _lib.fptr(cl), mp, 64) == -1
    assert lib.rt_cluster_table(C.byref(cfg), p, h.data.nbytes, None, mp, 64) == -1
