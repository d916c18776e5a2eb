"""The Phong g-buffer's expectation, checked where the oracle runs (no GPU).

tests/test_gpu_phong_gbuffer.py holds the kernels to phong_gbuffer_cases.expectation(): the
unchanged oracle's ao_compute at spp 1, depth 1, without emissive flags.  That is the rule of
include/rt/abi.h only if the AO threshold (0.0001) picks the hits that mode 3 (0) and mode 4 (0.001)
pick, and if what ao_compute stores there is (n, 1) / (t, 0, 0, 1) / zeros.  Both are checked here
against an independent scan of every shape along every primary ray, on all 17 scenes of the rule,
and on the `near` scene, built so that the thresholds disagree."""
import numpy as np
import pytest

import phong_gbuffer_cases as pg

W, H = 64, 48


@pytest.mark.parametrize("scene", pg.SCENES)
def test_expectation_is_the_rule(scene):
    h = pg.make_scene(scene, W, H)
    nrm, dep = pg.expectation(h, W, H)
    res, _ = pg.scan(h, W, H)
    assert pg.roots(res) == 0, "a primary ray has a root in (0, 0.001]: the thresholds may disagree"
    t0, i0 = pg.closest(res, 0.0)
    for thr in (1e-4, 1e-3):
        t, i = pg.closest(res, thr)
        assert np.array_equal(i, i0) and np.array_equal(t.view(np.uint32), t0.view(np.uint32)), f"threshold {thr}"
    t, ind = pg.check_against_scan(h, W, H, nrm, dep, 0.0, what=scene)
    assert h.num_objects == 0 or scene == "empty" or (ind >= 0).any()


def test_scenes_are_all_17():
    assert len(pg.SCENES) == len(set(pg.SCENES)) == 17


def test_near_scene_separates_the_thresholds():
    """Sphere 16's only positive root lies in (0, 0.001) on every pixel: mode 3's expectation is
    the oracle's on the 17 objects (sphere 16 everywhere), mode 4's the oracle's on the first 16."""
    h = pg.near_scene(W, H)
    assert h.num_objects == 17
    res, _ = pg.scan(h, W, H)
    r16 = res[16]
    assert (r16 >= np.float32(4.997e-4)).all() and (r16 <= np.float32(6.51e-4)).all()
    # mode 3: t > 0
    n3, d3 = pg.expectation(h, W, H)
    t, ind = pg.check_against_scan(h, W, H, n3, d3, 0.0, what="near, mode 3")
    assert (ind == 16).all() and ind.size == 3072
    # mode 4: t > 0.001 on the same 17 objects = the oracle on the first 16
    n4, d4 = pg.expectation(h, W, H, nobj=16)
    t, ind = pg.check_against_scan(h, W, H, n4, d4, 0.001, what="near, mode 4")
    assert (ind != 16).all()
    assert int((ind >= 0).sum()) == 1305 and int((ind < 0).sum()) == 1767
    assert int((d4[..., 3] == 1).sum()) == 1305


def test_expectation_ignores_emissive_flags_and_light():
    """Modes 3 and 4 ignore the emissive flag and the hit does not depend on the light; the cached
    expectation is read-only."""
    h = pg.make_scene("planes", W, H)  # has emissive shapes
    assert h.shapes[:, 1, 3].any()
    nrm, dep = pg.expectation(h, W, H)
    assert (dep[..., 3] == nrm[..., 3]).all()
    h2 = h.copy()
    h2.moving_light(True)
    n2, d2 = pg.expectation(h2, W, H)
    assert np.array_equal(n2, nrm) and np.array_equal(d2, dep)
    with pytest.raises(ValueError):
        nrm[0, 0, 0] = 1.0
