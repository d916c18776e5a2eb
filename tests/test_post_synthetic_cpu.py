"""The post-process on synthetic g-buffers, CPU side (tests/post_gbuffers.py):

  - the generator's coverage, measured from the reference alone (numpy_ref's stats), so the GPU
    comparison of tests/test_gpu_post_synthetic.py cannot pass vacuously;
  - the C oracle against the independent numpy restatement on these buffers, bit for bit;
  - the hand-built threshold frame: every case sits on its edge in the reference;
  - the post-process launch geometry as the kernel has it now (64 x 4 tiles, super-tiles and
    runs): a bijection onto the tiles at the benchmark sizes, their strips and the GPU sweep's
    shapes, and the branch each shape of that sweep takes.
"""
import numpy as np
import pytest

import oracle
import post_gbuffers as pg
from conftest import assert_bitwise
from oracle import numpy_ref

POST = oracle.AOP_POSTPROCESSING


def both(s, f, rows=None):
    """The numpy restatement and the C oracle on copies of s: (numpy ssbo, numpy image, stats,
    oracle ssbo, oracle image)."""
    W, R, F = s.W, s.H, s.F
    a, b = s.data.copy(), s.data.copy()
    ia, ib = np.full((R, W, 4), -7.0, np.float32), np.full((R, W, 4), -7.0, np.float32)
    st = {}
    with np.errstate(all="ignore"):
        numpy_ref.run_program(a, W, R, s.S, s.AA, POST, f, ia, F_=F, stats=st)
    oracle.run_program(b, oracle.dims(W, R, s.S, s.AA, F=F), POST, f, ib)
    return a, ia, st, b, ib


# (W, R, F, f): frames of the GPU tests large enough for shares to mean something
COVERAGE = [(130, 6, 8, 3), (70, 9, 8, 0), (576, 8, 8, 5), (64, 48, 8, 7), (130, 6, 16, 15), (130, 6, 2, 0)]


@pytest.mark.parametrize("W,R,F,f", COVERAGE)
def test_generator_covers_every_path_of_the_filter(W, R, F, f):
    s = pg.make(W, R, F, f)
    a, ia, st, _, _ = both(s, f)
    filt = st["filtered"]
    n = int(filt.sum())
    share = n / filt.size
    print(f"filtered {share:.3f}")
    assert 0.40 <= share <= 0.90
    # exits of the temporal loop: `accepted` = k means the loop broke at index k + 1 (k < F - 1) or ran out
    exits = np.bincount(st["accepted"][filt], minlength=F) / n
    print("exit shares", np.round(exits, 3))
    assert exits.size == F and (exits >= 0.05).all()
    neg = (st["weights"][filt] < 0).any(1).mean()
    print(f"negative neighbour weight {neg:.3f}, den < 0: {int((st['den'][filt] < 0).sum())}")
    assert neg >= 0.05
    assert (st["den"][filt] < 0).any()
    out = ia.reshape(-1, 4)[filt]  # (stats and the image are both row by row, x fastest)
    assert (st["y"] * W + st["x"] == np.arange(W * R)).all()
    print(f"finite outputs {np.isfinite(out).mean():.3f}")
    assert np.isfinite(out).mean() >= 0.80
    # visited = slots tested: the accepted ones and the one that failed
    assert (st["visited"][filt] == np.minimum(st["accepted"][filt] + 1, F - 1)).all()


def test_generator_holds_every_flag_and_weight_class():
    W, R, F, f = 130, 6, 8, 3
    s = pg.make(W, R, F, f)
    _, _, st, _, _ = both(s, f)
    w = s.normals[f, :, :, 3]
    for v in pg.FLAGS:
        assert (np.isnan(w).any() if np.isnan(v) else (w == v).any()), v
    wt = st["weights"][st["filtered"]]
    assert (wt == np.float32(1.2)).any()        # unit normals that agree, equal depth and bounces
    assert (wt == np.float32(0.2)).any()        # orthogonal, or a difference at / above its bound
    assert (wt == np.float32(-0.8)).any()       # opposed
    assert ((wt > 1.2) | (wt < -0.8)).any()     # non-unit normals
    assert ((wt > 0.2) & (wt < 1.2)).any()      # a difference below its bound
    assert (wt == 1.0).any() and np.isnan(wt).any()
    d = s.depth[f]
    col = s.pixels
    tiny = np.finfo(np.float32).tiny
    for a in (d[..., 0], col):
        assert ((np.abs(a) < tiny) & (a != 0)).any() and (np.abs(a) > 1e38).any() and (a < 0).any()
        assert (a == 0).any() and np.isinf(a).any() and np.isnan(a).any()
    # depth and bounce differences between horizontal neighbours below, at and above their bounds
    dd = np.abs(d[1:, :, 0] - d[:-1, :, 0])
    assert ((dd > 0) & (dd < 1)).any() and (dd == 1).any() and (dd > 1).any()
    bd = np.abs(d[1:, :, 1] - d[:-1, :, 1]) / np.float32(1.7)
    assert ((bd > 0) & (bd < 1)).any() and (bd == 1).any() and (bd > 1).any()


def test_generator_is_seeded():
    assert_bitwise(pg.make(70, 9, 8, 2).data, pg.make(70, 9, 8, 2).data, "same seed")
    a, b = pg.make(70, 9, 8, 2).data, pg.make(70, 9, 8, 2, seed=1).data
    assert (a.view(np.uint32) != b.view(np.uint32)).mean() > 0.5


@pytest.mark.parametrize("W,R", [(1, 1), (5, 3), (70, 9), (130, 6), (2, 2), (65, 5)])
@pytest.mark.parametrize("F,fs", [(8, (0, 3, 7)), (1, (0,)), (2, (0, 1)), (16, (0, 9, 15))])
def test_oracle_equals_numpy_restatement_bitwise(W, R, F, fs):
    for f in fs:
        a, ia, _, b, ib = both(pg.make(W, R, F, f), f)
        assert_bitwise(b, a, f"ssbo {W}x{R} F={F} f={f}")
        assert_bitwise(ib, ia, f"image {W}x{R} F={F} f={f}")
        assert not (ia == -7.0).any()


def test_oracle_equals_numpy_restatement_on_a_strip():
    """A band of rows 4..14 of a 20-row frame, rows 5..13 filtered: the halo rows are read only."""
    W, H, F, f, gy0, gh = 130, 20, 8, 2, 4, 11
    s = pg.make(W, gh, F, f)
    a, b = s.data.copy(), s.data.copy()
    ia, ib = np.zeros((gh, W, 4), np.float32), np.zeros((gh, W, 4), np.float32)
    with np.errstate(all="ignore"):
        numpy_ref.run_program(a, W, H, s.S, s.AA, POST, f, ia, F_=F, gy0=gy0, gh=gh, y0=5, y1=14)
    oracle.run_program(b, oracle.dims(W, H, s.S, s.AA, F=F, gy0=gy0, gh=gh), POST, f, ib, y0=5, y1=14)
    assert_bitwise(b, a, "strip ssbo")
    assert_bitwise(ib, ia, "strip image")


def test_threshold_frame_sits_on_every_edge():
    s, names = pg.thresholds()
    a, _, st, b, _ = both(s, 1)
    assert_bitwise(b, a, "threshold frame")
    after = pg.SSBO(pg.header(1), s.W, s.H, s.F)
    after.data[:] = b
    pg.check_thresholds(st, s, after, names)


# ---- the launch geometry ------------------------------------------------------------------
BENCH_SIZES = [(3840, 2160), (1920, 1080), (7680, 4320)]


def strip_heights(H):
    """The row counts of N = 1, 2, 3, 4 and 8 equal strips (dist.py / rt_group's even split)."""
    out = {H}
    for n in (2, 3, 4, 8):
        b = [round(i * H / n) for i in range(n + 1)]
        out |= {b[i + 1] - b[i] for i in range(n)}
    return sorted(out)


def assert_bijection(W, rows):
    gx, gy, R, sx, sy = pg.post_launch(W, rows)
    assert gx == -(-W // 64) and gy == -(-rows // 4)
    tiles = np.array([pg.post_tile(L, gx, gy, R, sx, sy) for L in range(gx * gy)])
    assert (tiles >= 0).all() and (tiles[:, 0] < gx).all() and (tiles[:, 1] < gy).all()
    assert np.unique(tiles[:, 1] * gx + tiles[:, 0]).size == gx * gy


@pytest.mark.parametrize("W,H", BENCH_SIZES)
def test_post_tile_map_is_a_bijection_at_the_benchmark_sizes_and_strips(W, H):
    for rows in strip_heights(H):
        assert_bijection(W, rows)
    # whole frames take the super-tile branch (gx = 60, 30, 120: multiples of 2 or 4, at least 8 super-tiles wide)
    assert pg.post_branch(W, H)[0] == "super"


@pytest.mark.parametrize("shape,branch", pg.GRID_SHAPES)
def test_post_tile_map_branch_of_every_sweep_shape(shape, branch):
    W, H = shape
    assert W * H < 80000
    assert pg.post_branch(W, H) == branch
    assert_bijection(W, H)


def test_sweep_reaches_every_branch_of_the_map():
    kinds = {b[:3] if b[0] == "super" else b[:1] for _, b in pg.GRID_SHAPES}
    assert {("row",), ("run",)} <= kinds
    assert {("super", sx, sy) for sx, sy in [(1, 2), (1, 4), (2, 2), (2, 4), (4, 1), (4, 4)]} <= kinds
    supers = [b for _, b in pg.GRID_SHAPES if b[0] == "super"]
    assert any(b[3] == 0 for b in supers) and any(b[3] > 0 for b in supers)  # with and without a tail


def test_run_branch_never_sees_a_searched_run_length():
    """launch_params searches the least R in [4, gx / 16] dividing gx / 8 only for gx a multiple of 8;
    xcd_tile reads R only when post_sx * post_sy == 1, which a gx that is a multiple of 8 reaches
    only below 32 tiles, where the search's range is empty: the run branch always has R = 4 (gx >= 32,
    gx and gy odd) or 0."""
    for gx in range(1, 400):
        for gy in (1, 2, 3, 4, 5, 8):
            _, _, R, sx, sy = pg.post_launch(gx * 64, gy * 4)
            if sx * sy == 1:
                assert R == (4 if gx >= 32 else 0)
                assert R == 0 or (gx % 2 == 1 and gy % 2 == 1)
