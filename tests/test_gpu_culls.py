"""Each conservative cull of the kernels alone, beside the exact test it lets them skip.

The production kernels skip most ray-shape tests on six hand-argued proofs: the
camera cone against spheres and planes, the first-bounce cone and its per-ray pre-test, the cluster
balls, the shadow cone.  A wrong margin there makes no noise: the kernel drops a shape that the
reference's scan accepts, for the few rays that graze it.  rt_selftest_math runs the production
device functions on the cases of tests/cull_cases.py (RT_MATH_CULL_*), which put a ray on each
proof's boundary and the shape tangent to it from both sides; tests/test_cull_cases_cpu.py shows
from the oracle alone that they do.

  soundness      a shape the proof rejects is accepted by no exact test, on the device's own exact
                 tests and on the oracle's; no violation allowed.  (Found by it: the shadow cone, whose
                 margins followed the sphere's distance from the light alone, rejected 75 spheres
                 that the reference's rounding makes occluders of far points; shadow_cone_keeps now
                 takes the longest line into the radius.  With a proof's margins at zero the test of
                 its family fails: DESIGN.md §5, round 13.)
  no vacuity     every far-outside case is rejected by the proof
  forms          the kernels' forms of the exact sphere test, the primary direction and the
                 shadow decision equal the oracle's bit for bit
"""
import functools

import numpy as np
import pytest

import adversarial_scenes
import cull_cases as cc
import oracle
from conftest import assert_bitwise
from real_time_ray_tracer_amd import Renderer, _lib

pytestmark = pytest.mark.gpu

FN = {"camera": _lib.RT_MATH_CULL_CAMERA, "plane": _lib.RT_MATH_CULL_PLANE, "bounce": _lib.RT_MATH_CULL_BOUNCE,
      "cluster": _lib.RT_MATH_CULL_CLUSTER, "tables": _lib.RT_MATH_CULL_CLUSTER, "shadow": _lib.RT_MATH_CULL_SHADOW}
OUT_W = {"camera": 7, "plane": 2, "bounce": 320, "cluster": 3, "tables": 3, "shadow": 128}


def selftest(fn, inp, n):
    with Renderer(16, 16, 4, 1) as r:
        return r.selftest_math(fn, inp, n)


def inputs(name):
    return cc.cluster_tables()["inp"] if name == "tables" else cc.FAMILIES[name]()["inp"]


@functools.lru_cache(maxsize=None)
def device(name):
    """The device's outputs for family `name`, one launch, kept for every test of the family."""
    inp = inputs(name)
    out = selftest(FN[name], inp, len(inp)).reshape(len(inp), OUT_W[name])
    if name == "bounce":
        out = out.reshape(len(inp), 64, 5)
    if name == "shadow":
        out = out.reshape(len(inp), 64, 2)
    return out


def hexrow(row):
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(row, np.float32).view(np.uint32))


def no_violation(name, bad, what):
    """bad: per case, the proof rejected and an exact test accepted."""
    n = int(bad.sum())
    print(f"{name}: {what}: {n} violations in {len(bad)} cases")
    if n:
        i = int(np.flatnonzero(bad)[0])
        strata = np.bincount(cc.FAMILIES[name]()["stratum"][bad], minlength=3) if name != "tables" else "-"
        raise AssertionError(f"{name}: {what}: {n} of {len(bad)} cases (grazing, far, degenerate: {strata}); first: case {i}, "
                             f"inputs {hexrow(inputs(name)[i])}")


def rejected_and_accepted(name):
    """Per case: (the proof rejects, some exact test of the device accepts, some of the oracle's does)."""
    o, ex = device(name), cc.exact(name)
    if name == "camera":
        return o[:, 3] == 1, (o[:, 5] != -1) | (o[:, 6] != -1), ex["acc"]
    if name == "plane":
        return o[:, 0] == 1, o[:, 1] > 0, ex["acc"]
    if name in ("cluster", "tables"):
        return o[:, 0] == 0, o[:, 2] != -1, ex["acc"]
    if name == "bounce":
        live = cc.bounce_parts(inputs(name))[3]
        return (o[:, 0, 0] == 1) | (o[:, 0, 1] == 0), ((o[..., 3] != -1) & live).any(1), ex["acc"].any(1)
    need = cc.shadow_parts(inputs(name))[3]
    return o[:, 0, 0] == 0, ((o[..., 1] == 1) & need).any(1), ex["acc"].any(1)


# ---- soundness --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FN))
def test_a_rejected_shape_is_accepted_by_no_exact_test(name):
    rej, dev_acc, ref_acc = rejected_and_accepted(name)
    print(f"{name}: the proof rejects {int(rej.sum())} of {len(rej)} cases; the exact test accepts "
          f"{int(dev_acc.sum())} (device), {int(ref_acc.sum())} (oracle)")
    assert set(np.unique(device(name)[..., 0 if name != "camera" else 3])) <= {0.0, 1.0}
    no_violation(name, rej & dev_acc, "rejected by the proof, accepted by the device's exact test")
    no_violation(name, rej & ref_acc, "rejected by the proof, accepted by the oracle's exact test")


def test_a_lane_that_fails_its_pre_test_accepts_nothing():
    o = device("bounce")
    live = cc.bounce_parts(inputs("bounce"))[3]
    keep, passed, t = o[..., 1] == 1, o[..., 2] == 1, o[..., 3]
    assert not (passed & ~live).any(), "a lane that is not live passes no pre-test"
    print(f"bounce: {int((keep & live).sum())} kept live lanes, {int((keep & live & passed).sum())} pass the pre-test, "
          f"{int((live & (t != -1)).sum())} accept")
    no_violation("bounce", (keep & ~passed & live & (t != -1)).any(1), "kept, pre-test failed, accepted on the device")
    no_violation("bounce", (keep & ~passed & cc.exact("bounce")["acc"]).any(1), "kept, pre-test failed, accepted by the oracle")


# ---- no vacuity -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_every_far_outside_case_is_rejected_by_the_proof(name):
    rej, _, _ = rejected_and_accepted(name)
    far = cc.FAMILIES[name]()["stratum"] == cc.FAR
    if name == "bounce":  # both forms of the cone test
        o = device(name)
        rej = (o[:, 0, 0] == 1) & (o[:, 0, 1] == 0)
    kept = far & ~rej
    print(f"{name}: {int(far.sum())} far-outside cases, {int(kept.sum())} kept by the proof; "
          f"{int(rej.sum())} of all {len(rej)} cases rejected")
    assert far.sum() >= 0.1 * len(far)
    assert not kept.any(), (f"{name}: {int(kept.sum())} far-outside cases kept; first: case {int(np.flatnonzero(kept)[0])}, "
                            f"inputs {hexrow(inputs(name)[np.flatnonzero(kept)[0]])}")


# ---- forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cluster", "tables"])
def test_cluster_test_equals_its_wave_mask_form(name):
    o = device(name)
    assert_bitwise(o[:, 1], o[:, 0], f"{name}: cluster_may_hit_mask's bit against cluster_may_hit")
    assert 0 < (o[:, 0] == 0).sum() < len(o)


def accepted(t, thr):
    """What a scan that starts at t = -1 holds after one sphere whose exact test gives t."""
    with np.errstate(invalid="ignore"):
        return np.where(t > np.float32(thr), t, np.float32(-1.0)).astype(np.float32)


FORMS = ["primary_dir", "sphere_eval", "camera_row_at_0.0001", "camera_row_at_0", "plane_eval", "bounce", "bounce_if",
         "cluster", "tables", "shadow"]


@pytest.mark.parametrize("form", FORMS)
def test_exact_forms_equal_the_oracle_bit_for_bit(form):
    """Every form of an exact test on its family's rays.  An accepted t is the oracle's sphere_eval
    where that exceeds the threshold, -1 elsewhere.

    The degenerate rows with r = +inf have a discriminant of +inf: sphere_eval_ray returns t = +inf there,
    which the reference's scan accepts, and so must every candidate form (their square root,
    sqrt_rn_tail_inf in rt_device.h, is exact at +inf for that; before it the two forms at threshold
    0.0001 returned -1 on exactly those rows: 2160 camera cases, 56 bounce cases)."""
    if form in ("primary_dir", "sphere_eval", "camera_row_at_0.0001", "camera_row_at_0"):
        o, inp = device("camera"), inputs("camera")
        if form == "primary_dir":
            return assert_bitwise(o[:, 0:3], cc.exact("camera")["dir"], form)
        t_ref = oracle.sphere_eval_n(inp[:, 0:3], o[:, 0:3], inp[:, 20:24])  # at the direction the device returned
        assert (t_ref > 0).sum() > 10000 and np.isnan(t_ref).any() and np.isinf(t_ref).any()
        if form == "sphere_eval":
            return assert_bitwise(o[:, 4], t_ref, form)
        thr = 0.0001 if form == "camera_row_at_0.0001" else 0.0
        return assert_bitwise(o[:, 5 if thr else 6], accepted(t_ref, thr), f"sphere_candidate_rel at {thr}")
    if form == "plane_eval":
        return assert_bitwise(device("plane")[:, 1], cc.exact("plane")["t"], form)
    if form == "shadow":
        occ, ref = device("shadow")[..., 1] == 1, cc.exact("shadow")["occ"]
        assert 0 < ref.sum() < ref.size
        assert (occ == ref).all(), f"shadow: {int((occ != ref).sum())} occluder decisions differ from the oracle"
        return
    if form == "bounce_if":  # sphere_candidate_if, the batched first bounce's form: the lanes whose pre-test passed
        o = device("bounce")
        want = np.where(o[..., 2] == 1, accepted(cc.exact("bounce")["t"], 0.0001), np.float32(-1.0)).astype(np.float32)
        assert (o[..., 2] == 1).sum() > 10000 and np.isinf(want).any()
        return assert_bitwise(o[..., 4], want, "sphere_candidate_if at 0.0001 on the lanes that pass")
    t = device(form)[..., 3 if form == "bounce" else 2]
    assert_bitwise(t, accepted(cc.exact(form)["t"], 0.0001), f"{form}: sphere_candidate at 0.0001")


def test_sphere_and_normalize_self_tests():
    """RT_MATH_SPHERE and RT_MATH_NORMALIZE on 2^16 inputs, bit for bit: tangent rays (del == 0), origins
    in and on spheres, zero and denormal vectors, 3e38."""
    rng = np.random.default_rng(0xC6)
    n = 1 << 16
    pos = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    d = oracle.normalize3_n(rng.normal(size=(n, 3)))
    c = (pos + d * rng.uniform(-5, 50, (n, 1)) + rng.normal(size=(n, 3)) * 2).astype(np.float32)
    r = (10.0 ** rng.uniform(-3, 1.5, n)).astype(np.float32)
    k = n // 8
    c[:k] = pos[:k] + (rng.normal(size=(k, 3)) * 0.3).astype(np.float32)         # origins inside
    r[:k] = 1.0
    nn = oracle.normalize3_n(rng.normal(size=(k, 3)))
    c[k:2 * k] = pos[k:2 * k] - nn * r[k:2 * k, None]                            # origins on the surface
    for j in range(6):                                                           # del == 0
        rad = [1.5, 0.75, 1.25, 1.0, 0.5, 2.0][j]
        c[2 * k + j] = adversarial_scenes.tangent_center(d[2 * k + j], 6.0 + j, rad, seed=200 + j, origin=pos[2 * k + j])
        r[2 * k + j] = rad
        assert oracle.sphere_del(pos[2 * k + j], d[2 * k + j], c[2 * k + j], rad) == 0.0
    r[3 * k:3 * k + 64] = [0.0, -1.0, 1e4, 3e38] * 16
    c[3 * k + 64:3 * k + 96] = np.float32(3e38)
    d[3 * k + 96:3 * k + 128] = 0.0
    pos[3 * k + 128:3 * k + 160] = np.nan
    inp = np.concatenate([pos, d, c, r[:, None]], axis=1).astype(np.float32)
    got = selftest(_lib.RT_MATH_SPHERE, inp, n)
    ref = oracle.sphere_eval_n(pos, d, np.concatenate([c, r[:, None]], axis=1))
    assert_bitwise(got, ref, "RT_MATH_SPHERE")
    assert (ref > 0).sum() > n // 8 and (ref == -1).sum() > n // 8

    v = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-30, 18, (n, 1))).astype(np.float32)
    v[:64] = 0.0
    v[64:128] = (rng.normal(size=(64, 3)) * 1e-42).astype(np.float32)            # denormal
    v[128:192] = np.float32(3e38) * rng.choice([-1.0, 1.0], (64, 3)).astype(np.float32)
    v[192:256, 1:] = 0.0                                                         # one component
    v[256:320] = (rng.normal(size=(64, 3)) * 1e-20).astype(np.float32)           # dot underflows
    v[320:324] = [[np.inf, 0, 0], [np.nan, 1, 1], [1, -np.inf, 1], [-0.0, 0.0, -0.0]]
    got = selftest(_lib.RT_MATH_NORMALIZE, v, n).reshape(n, 3)
    assert_bitwise(got, oracle.normalize3_n(v), "RT_MATH_NORMALIZE")


def test_self_test_rejects_a_partial_wave_of_cluster_cases():
    with Renderer(16, 16, 4, 1) as r:
        with pytest.raises(_lib.RtError) as e:
            r.selftest_math(_lib.RT_MATH_CULL_CLUSTER, np.zeros((63, 14), np.float32), 63)
        assert e.value.status == _lib.RT_E_INVAL
        with pytest.raises(_lib.RtError) as e:
            r.selftest_math(_lib.RT_MATH_CULL_SHADOW + 1, np.zeros(64, np.float32), 1)
        assert e.value.status == _lib.RT_E_INVAL
        assert r.selftest_math(_lib.RT_MATH_CULL_CLUSTER, np.zeros((64, 14), np.float32), 64).shape == (192,)
