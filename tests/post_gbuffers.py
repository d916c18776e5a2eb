"""Synthetic g-buffers for the mode-1 post-process alone (test infrastructure).

A rendered frame gives post_kernel only what the AO pass writes: normal w exactly 0 or 1, unit
normals, finite depths and colours, hardly ever opposed normals at equal depth, and with a still
camera a history that is accepted in every slot.  The buffers built here put a value in every
part of the filter's input domain instead (aop_postprocessing.glsl:57-208), by classes, so each
path is taken by design:

  temporal loop   every pixel draws an agreement length L: slots f-1 .. f-L carry slot f's keys
                  (coeff = |n|^2 > 0.85), slot f-L-1 is perturbed to fail (the cause cycles over
                  normal, depth, bounces, a NaN key), and the slots after it mostly agree again,
                  with colours of their own, so a loop that went on past the exit would show
  neighbours      normals from a small palette (agreeing, orthogonal, opposed, non-unit), depths
                  and bounces from a few levels whose differences are below, at and above 1 and
                  1.7, sky neighbours (w < 0.001); checkerboards of opposed normals (den < 0)
  flags           w in {0, 1, 0.99f, nextafter(0.99f, 2), 0.001f, nextafter(0.001f, 0), 2, NaN}
  values          colours in [0, 4], depths in [0, 30], with small fixed shares of subnormal,
                  near-FLT_MAX, negative, +-0, inf and NaN values

make(W, R, F, f, seed) -> SSBO of an R-row band (the header is a valid little scene, which the
post-process does not read beyond W, H, F and the frame slot).  thresholds() -> a hand-built frame
with the filter's three decisions and its divisions at their exact edges, and the names of its
pixels.  The post-process launch geometry (launch_params / xcd_tile of rt_kernels_impl.h) is
restated here too: post_launch, post_tile, post_branch, GRID_SHAPES.
"""
from __future__ import annotations

import numpy as np

from oracle import numpy_ref
from real_time_ray_tracer_amd import SSBO, Header, aspect_for

F32 = np.float32
W099, W0001 = F32(0.99), F32(0.001)
FLAGS = np.array([0.0, 1.0, W099, np.nextafter(W099, F32(2)), W0001, np.nextafter(W0001, F32(0)), 2.0, np.nan], F32)
FLAG_P = [0.10, 0.50, 0.06, 0.12, 0.05, 0.05, 0.07, 0.05]  # filtered (w > 0.99): 1, the float above 0.99f, 2

# shares of special values, per value: subnormal, near FLT_MAX, negative, +-0, inf, NaN
COLOUR_SHARES = (0.004, 0.001, 0.012, 0.008, 0.0007, 0.0007)
DEPTH_SHARES = (0.004, 0.002, 0.010, 0.010, 0.002, 0.002)


def header(f: int = 0) -> Header:
    h = Header.synthetic(4, 1, 1234, aspect_for(4, 3))
    h.set_mode(f, h.num_objects)
    return h


def _sprinkle(rng, a: np.ndarray, shares) -> np.ndarray:
    """A copy of a with fixed shares of its values replaced by special ones."""
    flat = np.array(a, F32).reshape(-1)
    u = rng.random(flat.size)
    sign = np.where(rng.random(flat.size) < 0.5, F32(-1), F32(1))
    edges = np.cumsum(shares)
    sub = rng.integers(1, 0x00800000, flat.size).astype(np.uint32).view(F32)
    special = [sub * sign, rng.uniform(1e38, 3.4e38, flat.size).astype(F32) * sign,
               -rng.uniform(0.0, 4.0, flat.size).astype(F32), F32(0) * sign, F32(np.inf) * sign,
               np.full(flat.size, np.nan, F32)]
    lo = 0.0
    for hi, v in zip(edges, special):
        m = (u >= lo) & (u < hi)
        flat[m] = v[m]
        lo = hi
    return flat.reshape(np.shape(a))


def _normals(rng, n: int) -> np.ndarray:
    k = rng.choice(8, n, p=[0.34, 0.20, 0.10, 0.05, 0.06, 0.05, 0.10, 0.10])
    palette = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 1), (1.5, 0, 0), (-1.2, 0, 0)], F32)
    out = np.zeros((n, 3), F32)
    fixed = k < 6
    out[fixed] = palette[k[fixed]]
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    v[k == 7] *= rng.uniform(0.5, 1.6, (int((k == 7).sum()), 1))  # non-unit, some with |n|^2 < 0.85
    out[~fixed] = v[~fixed].astype(F32)
    u = rng.random(n)
    out[u < 0.008, 0] = np.nan
    out[(u >= 0.008) & (u < 0.012), 1] = np.inf
    return out


def _levels(rng, n: int, levels, p, lo: float, hi: float) -> np.ndarray:
    """Values from a few levels (the last share: uniform in [lo, hi])."""
    k = rng.choice(len(levels) + 1, n, p=p)
    out = rng.uniform(lo, hi, n).astype(F32)
    for i, v in enumerate(levels):
        out[k == i] = F32(v)
    return out


def _keys(rng, n: int):
    """Slot f's keys of n pixels: normals [n][4], depth [n][4] (depth, bounces, two free channels)."""
    nrm = np.concatenate([_normals(rng, n), rng.choice(FLAGS, n, p=FLAG_P)[:, None]], 1).astype(F32)
    dep = np.empty((n, 4), F32)
    # depth levels 7.25 + {0, 0.5, 1, 1.5}: differences below, at and above 1
    dep[:, 0] = _levels(rng, n, [7.25, 7.75, 8.25, 8.75], [0.62, 0.10, 0.10, 0.06, 0.12], 0.0, 30.0)
    # bounce levels 0, 1, 1.7f, 2, 3: |0 - 1.7f| / 1.7f is exactly 1
    dep[:, 1] = _levels(rng, n, [0.0, 1.0, F32(1.7), 2.0, 3.0], [0.58, 0.12, 0.08, 0.08, 0.04, 0.10], 0.0, 4.0)
    dep[:, 2:] = rng.uniform(0.0, 30.0, (n, 2)).astype(F32)
    return nrm, _sprinkle(rng, dep, DEPTH_SHARES)


def _colours(rng, shape) -> np.ndarray:
    return _sprinkle(rng, rng.uniform(0.0, 4.0, shape).astype(F32), COLOUR_SHARES)


def _checkerboards(rng, nrm, dep, W: int, R: int):
    """3 x 3 patches of opposed normals at one depth and bounce count: the centre's four
    neighbours weigh -0.8 each (den = -2.2), every other pixel of the patch has negative weights."""
    if W < 3 or R < 3:
        return
    n4, d4 = nrm.reshape(W, R, 4), dep.reshape(W, R, 4)
    for _ in range(W * R // 300 + 1):
        x0, y0 = int(rng.integers(0, W - 2)), int(rng.integers(0, R - 2))
        for dx in range(3):
            for dy in range(3):
                s = 1.0 if (dx + dy) % 2 == 0 else -1.0
                n4[x0 + dx, y0 + dy] = (s, 0.0, 0.0, 1.0)
                d4[x0 + dx, y0 + dy, :2] = (7.25, 0.0)


def make(W: int, R: int, F: int = 8, f: int = 0, seed: int = 0) -> SSBO:
    """A seeded synthetic g-buffer ring of R rows by W columns, F slots, built around slot f."""
    rng = np.random.default_rng([seed, W, R, F, f])
    s = SSBO(header(f), W, R, F)
    n = W * R
    nrm, dep = _keys(rng, n)
    _checkerboards(rng, nrm, dep, W, R)
    pix, nrms, deps = s.pixels.reshape(F, n, 4), s.normals.reshape(F, n, 4), s.depth.reshape(F, n, 4)
    pix[:] = _colours(rng, (F, n, 4))
    nrms[f], deps[f] = nrm, dep
    # agreement lengths: dealt evenly over the filtered pixels (and over the others, whose history
    # is never read), shuffled
    L = np.empty(n, np.int64)
    filt = nrm[:, 3] > W099
    for m in (filt, ~filt):
        k = int(m.sum())
        L[m] = rng.permutation(k) % F
    cause = rng.permutation(n) % 4
    big = ~(np.abs(dep[:, :2]) < F32(1e30))  # a depth (bounce count) that adding 1.5 (2) does not move
    for i in range(1, F):
        cf = (f - i) % F
        kn, kd = nrm.copy(), dep.copy()
        kn[:, 3] = rng.choice(FLAGS, n, p=FLAG_P)          # (history flags are not read)
        kd[:, 2:] = rng.uniform(0.0, 30.0, (n, 2)).astype(F32)
        fail = i == L + 1
        c = cause
        m = fail & (c == 0)
        kn[m, :3] = np.where((np.arange(n)[m] % 2 == 0)[:, None], -nrm[m, :3], nrm[m][:, [1, 2, 0]] * F32(0.25))
        m = fail & (c == 1)
        kd[m, 0] = np.where(big[m, 0], F32(0), dep[m, 0] + F32(1.5))
        m = fail & (c == 2)
        kd[m, 1] = np.where(big[m, 1], F32(0), dep[m, 1] + F32(2.0))
        m = fail & (c == 3)
        which = np.arange(n) % 3
        kn[m & (which == 0), 0] = np.nan
        kd[m & (which == 1), 0] = np.nan
        kd[m & (which == 2), 1] = np.nan
        # past the failing slot: mostly agreeing keys again, else keys of their own
        other = (i > L + 1) & (rng.random(n) < 0.3)
        on, od = _keys(rng, n)
        kn[other], kd[other] = on[other], od[other]
        nrms[cf], deps[cf] = kn, kd
    return s


# ---- the hand-built threshold frame ----------------------------------------------------
def _dot_search(rng, target: np.float32):
    """A unit normal n and a history normal hn with dot3(n, hn) == target exactly, by walking
    hn.x's bits (one step moves the dot by less than its ulp, so every float near is met)."""
    v = rng.normal(size=3)
    v = np.abs(v / np.linalg.norm(v)).astype(F32) + F32(0.05)
    v = numpy_ref.normalize3(v[None])[0]
    hn = (v * F32(target)).astype(F32)
    for _ in range(4000):
        d = numpy_ref.dot3(v[None], hn[None])[0]
        if d == target:
            return v, hn
        hn[0] = np.nextafter(hn[0], F32(2) if d < target else F32(-2))
    raise RuntimeError("no normal pair found")


def thresholds():
    """(SSBO, names): a 52 x 2 frame, F = 4, built around slot 1 (so slot f-2 wraps to 3).  With
    two rows, row 1's pixels have left and right neighbours only (up iff y + 1 < H, down iff
    y >= 2), and the end pixels a single one.  names[case] = x of the case's pixel in row 1."""
    W, H, F, f = 52, 2, 4, 1
    s = SSBO(header(f), W, H, F)
    P, N, D = s.pixels, s.normals, s.depth
    rng = np.random.default_rng(99)
    c085 = F32(0.85)
    above = np.nextafter(c085, F32(1))
    names = {}
    own = (1.0, 0.0, 0.0, 1.0)

    def put(x, slot, pix=None, nrm=None, dep=None):
        if pix is not None:
            P[slot, x, 1] = pix
        if nrm is not None:
            N[slot, x, 1] = nrm
        if dep is not None:
            D[slot, x, 1, :len(dep)] = dep

    # one present neighbour with weight -1.2f + 0.2f = -1: den is exactly 0
    names["den_zero"] = 0
    put(0, f, (1.0, -1.0, 0.5, 2.0), own, (3.0, 1.0))
    put(1, f, (0.5, -0.5, 0.5, 1.0), (F32(-1.2), 0.0, 0.0, 1.0), (3.0, 1.0))
    # one present neighbour with weight -2 + 0.2: den = -0.8
    names["den_neg"] = W - 1
    put(W - 1, f, (1.0, 2.0, 3.0, 4.0), own, (3.0, 1.0))
    put(W - 2, f, (0.5, 0.25, 4.0, 1.0), (-2.0, 0.0, 0.0, 1.0), (3.0, 1.0))
    x = 4

    def case(name):
        nonlocal x
        names[name] = x
        x += 4
        return names[name]

    # history coefficient exactly 0.85f (the loop breaks) and the float above (accepted), three ways
    for tag, co in (("eq", c085), ("above", above)):
        xx = case(f"coeff_{tag}_axis")          # dot = 1 * co
        put(xx, f, (1.0, 2.0, 3.0, 4.0), own, (3.0, 1.0))
        put(xx, 0, (4.0, 3.0, 2.0, 1.0), (co, 0.0, 0.0, 0.0), (3.0, 1.0))
        xx = case(f"coeff_{tag}_depth")         # 1 - |0 - hd| = co
        hd = F32(1) - c085                       # exact; 1 - hd == 0.85f
        if tag == "above":
            while not F32(1) - hd > c085:
                hd = np.nextafter(hd, F32(0))
        put(xx, f, (1.0, 2.0, 3.0, 4.0), own, (0.0, 1.0))
        put(xx, 0, (4.0, 3.0, 2.0, 1.0), own, (hd, 1.0))
        xx = case(f"coeff_{tag}_general")       # a searched pair of general normals
        v, hn = _dot_search(rng, co)
        put(xx, f, (1.0, 2.0, 3.0, 4.0), (*v, 1.0), (3.0, 1.0))
        put(xx, 0, (4.0, 3.0, 2.0, 1.0), (*hn, 0.0), (3.0, 1.0))
    # own w: 0.99f passes through, the float above is filtered (neighbours would change it)
    for tag, w in (("eq", W099), ("above", np.nextafter(W099, F32(2)))):
        xx = case(f"own_w_{tag}")
        put(xx, f, (1.0, 2.0, 3.0, 4.0), (1.0, 0.0, 0.0, w), (3.0, 1.0))
        put(xx - 1, f, (9.0, 9.0, 9.0, 9.0), own, (3.0, 1.0))
        put(xx + 1, f, (7.0, 7.0, 7.0, 7.0), own, (3.0, 1.0))
    # neighbour w: 0.001f is weighted by wf (orthogonal: 0.2f), the float below weighs 1
    for tag, w in (("eq", W0001), ("below", np.nextafter(W0001, F32(0)))):
        xx = case(f"nbr_w_{tag}")
        put(xx, f, (1.0, 2.0, 3.0, 4.0), own, (3.0, 1.0))
        put(xx - 1, f, (8.0, 8.0, 8.0, 8.0), (0.0, 1.0, 0.0, w), (3.0, 1.0))
    # subnormal quotients in both sets of divisions: tiny colours, sky neighbours (den = 3), one
    # agreeing history slot with a tiny colour
    xx = case("subnormal")
    tiny = (F32(1.2e-38), F32(2e-39), F32(1.5e-38), F32(5e-39))
    put(xx, f, tiny, own, (3.0, 1.0))
    put(xx, 0, (F32(3e-39), F32(1.3e-38), F32(7e-40), F32(1.18e-38)), own, (3.0, 1.0))
    assert x <= W - 3
    return s, names


def check_thresholds(stats: dict, before: SSBO, after: SSBO, names: dict) -> None:
    """The reference's own figures (numpy_ref stats) and output on the threshold frame: every case
    really sits on its edge."""
    W, H, F, f = before.W, before.H, before.F, 1
    i = {k: int(np.nonzero((stats["x"] == x) & (stats["y"] == 1))[0][0]) for k, x in names.items()}
    st = lambda key, k: stats[key][i[k]]  # noqa: E731
    c085 = F32(0.85)
    for way in ("axis", "depth", "general"):
        k = f"coeff_eq_{way}"
        assert st("filtered", k) and st("coeff", k)[0] == c085 and st("accepted", k) == 0 and st("visited", k) == 1, k
        k = f"coeff_above_{way}"
        assert st("filtered", k) and st("coeff", k)[0] == np.nextafter(c085, F32(1)), k
        assert st("accepted", k) == 1 and st("visited", k) == 2, k  # slot f-2 holds zeros: coeff 0
    raw, out = before.pixels[f, :, 1], after.pixels[f, :, 1]
    assert not st("filtered", "own_w_eq") and (out[names["own_w_eq"]] == raw[names["own_w_eq"]]).all()
    assert st("filtered", "own_w_above") and (out[names["own_w_above"]] != raw[names["own_w_above"]]).all()
    assert st("weights", "nbr_w_eq")[2] == F32(0.2) and st("weights", "nbr_w_below")[2] == F32(1.0)
    assert st("den", "den_zero") == 0 and list(st("weights", "den_zero")) == [0, 0, 0, -1]
    assert not np.isfinite(out[names["den_zero"]]).any()
    assert st("den", "den_neg") < 0 and np.isfinite(out[names["den_neg"]]).all()
    tiny = float(np.finfo(F32).tiny)
    o = out[names["subnormal"]]
    assert st("accepted", "subnormal") == 1 and ((o > 0) & (o < tiny)).all()
    first = (raw[names["subnormal"]] / st("den", "subnormal")).astype(F32)  # (sky neighbours add 0)
    assert st("den", "subnormal") == 3 and ((first > 0) & (first < tiny)).all()


# ---- the post-process launch geometry, restated ----------------------------------------
TILE_W, TILE_H = 64, 4  # kPostTileW, kPostTileH


def post_launch(W: int, rows: int):
    """launch_params: (gx, gy, tile_run, post_sx, post_sy) of a post-process launch over `rows` rows."""
    gx, gy = -(-W // TILE_W), -(-rows // TILE_H)
    R = 0
    if gx % 8 == 0:
        for r in range(4, gx // 16 + 1):
            if (gx // 8) % r == 0:
                R = r
                break
    R = R if R else (4 if gx >= 32 else 0)
    sx = 4 if gx % 4 == 0 else (2 if gx % 2 == 0 else 1)
    sy = 4 if gy % 4 == 0 else (2 if gy % 2 == 0 else 1)
    if gx < 8 * sx:
        sx = sy = 1
    return gx, gy, R, sx, sy


def post_tile(L: int, gx: int, gy: int, R: int, sx: int, sy: int):
    """xcd_tile: linear workgroup id L -> tile (bx, by), both branches."""
    if sx * sy > 1:
        ss, gsx = sx * sy, gx // sx
        Q = gsx * (gy // sy)
        M = Q // 8 * 8
        if L < M * ss:
            j = L >> 3
            q, o = (j // ss) * 8 + (L & 7), j % ss
        else:
            q, o = M + (L - M * ss) // ss, (L - M * ss) % ss
        return (q % gsx) * sx + o % sx, (q // gsx) * sy + o // sx
    n = gx * gy
    M = n // (8 * R) * (8 * R) if R else 0
    t = L
    if L < M:
        j = L >> 3
        t = ((j // R) * 8 + (L & 7)) * R + j % R
    return t % gx, t // gx


def post_branch(W: int, rows: int):
    """("row",) | ("run", R, whole rounds of 8 runs, tiles left over) | ("super", sx, sy, super-tiles
    left over after the whole rounds of 8)."""
    gx, gy, R, sx, sy = post_launch(W, rows)
    if sx * sy > 1:
        return ("super", sx, sy, (gx // sx) * (gy // sy) % 8)
    if R:
        return ("run", R, gx * gy // (8 * R), gx * gy % (8 * R))
    return ("row",)


# the smallest frames that reach each branch of the map (all under 80 K pixels)
GRID_SHAPES = [
    ((64, 48), ("row",)),               # gx = 1
    ((130, 6), ("row",)),               # partial tiles both ways
    ((576, 12), ("row",)),              # gx = 9, gy = 3
    ((576, 8), ("super", 1, 2, 1)),
    ((576, 16), ("super", 1, 4, 1)),
    ((1152, 16), ("super", 2, 4, 1)),
    ((1100, 40), ("super", 2, 2, 5)),
    ((2048, 16), ("super", 4, 4, 0)),
    ((2304, 16), ("super", 4, 4, 1)),
    ((2048, 12), ("super", 4, 1, 0)),
    ((2300, 20), ("super", 4, 1, 5)),
    ((2100, 12), ("run", 4, 3, 3)),
    ((2100, 36), ("run", 4, 9, 9)),
    ((2100, 16), ("super", 1, 4, 1)),
]
