"""Generated meshes and ray sets for the mesh tests (include/rt/mesh.h).  Everything is made by code
from fixed seeds; nothing is read from a file.

meshes(): name -> (verts [nv][3] float32, tris [nt][3] int32)
  ico       an icosphere at subdivision 2, 320 triangles
  grid      an 8 x 8 ground grid, 128 triangles, every triangle's box flat and axis-aligned
  both      the two together, 448 triangles
  tri1, tri7, tri8, tri9   the single-leaf boundary (7 | 8) and the first tree with an inner node
  odd       a 4 x 4 grid with a NaN vertex, an infinite vertex, a zero-area triangle and three exact
            duplicates of one triangle at different indices (ODD_DUPLICATES, the lowest first)
  empty     nt = 0
rays(name): origins, dirs, a, b ([N_RAYS][3] float32 each; a -> b are the occlusion segments of the
  same rays, ending before or beyond what they aim at), kind [N_RAYS] (KINDS), aimed at interior
  points, points on shared edges, vertices exactly, past the silhouette; with zero and subnormal
  direction components, origins on triangle-box planes, unnormalised directions, NaN and infinite rays.
"""
import functools

import numpy as np

N_RAYS = 4099  # not a multiple of 64: the tail wave is exercised
KINDS = ("interior", "edge", "vertex", "miss", "axis", "plane", "scaled", "bad")
ODD_DUPLICATES = (5, 20, 37)


def icosphere(level=2, centre=(0.3, 1.4, -0.4), radius=1.0):
    g = (1 + 5 ** 0.5) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.array(v) * radius + np.array(centre)).astype(np.float32) + np.float32(0.0)
    return verts, np.array(f, np.int32)


def grid(n=8, size=8.0, y=0.0):
    xs = np.linspace(-size / 2, size / 2, n + 1)
    verts = np.array([(x, y, z) for z in xs for x in xs], np.float32) + np.float32(0.0)
    tris = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            tris += [(a, a + n + 2, a + 1), (a, a + n + 1, a + n + 2)]  # normals up
    return verts, np.array(tris, np.int32)


def cube():
    """The unit cube as 12 triangles, the mesh of CUBE_OBJ's six quads fanned."""
    verts = np.array([(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    quads = [(1, 2, 4, 3), (5, 6, 8, 7), (1, 2, 6, 5), (3, 4, 8, 7), (1, 3, 7, 5), (2, 4, 8, 6)]
    tris = [(q[0] - 1, q[k] - 1, q[k + 1] - 1) for q in quads for k in (1, 2)]
    return verts, np.array(tris, np.int32)


CUBE_OBJ = "# unit cube\n" + "".join(f"v {x} {y} {z}\n" for z in (0, 1) for y in (0, 1) for x in (0, 1)) + \
    "f 1 2 4 3\nf 5 6 8 7\nf 1 2 6 5\nf 3 4 8 7\nf 1 3 7 5\nf 2 4 8 6\n"


@functools.lru_cache(maxsize=None)
def meshes():
    out = {}
    iv, it = icosphere()
    gv, gt = grid()
    out["ico"] = (iv, it)
    out["grid"] = (gv, gt)
    out["both"] = (np.concatenate([iv, gv]), np.concatenate([it, gt + len(iv)]).astype(np.int32))
    for k in (1, 7, 8, 9):
        out[f"tri{k}"] = (gv, gt[:k].copy())
    ov, ot = grid(4, 4.0)
    ov = np.concatenate([ov, np.float32([[np.nan, 0.5, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, -np.inf]])])
    nan_v, inf_v = len(ov) - 3, len(ov) - 2
    ot = ot.tolist()
    dup = ot[ODD_DUPLICATES[0]]
    ot.insert(10, [0, 1, nan_v])                 # dead: a NaN vertex
    ot.insert(15, [2, inf_v, 3])                 # dead: an infinite vertex
    ot.insert(ODD_DUPLICATES[1], list(dup))      # an exact duplicate
    ot.insert(25, [6, 6, 7])                     # zero area: alive, never hit
    ot.insert(30, [0, 12, 24])                   # zero area: three points in a line
    ot.append(list(dup))                         # the third copy, last
    ot = np.array(ot, np.int32)
    assert all((ot[i] == ot[ODD_DUPLICATES[0]]).all() for i in ODD_DUPLICATES) and len(ot) == ODD_DUPLICATES[2] + 1
    out["odd"] = (ov, ot)
    out["empty"] = (gv, np.zeros((0, 3), np.int32))
    for v, t in out.values():
        v.setflags(write=False)
        t.setflags(write=False)
    return out


def live_triangles(verts, tris):
    return np.flatnonzero(np.isfinite(verts[tris].reshape(len(tris), 9)).all(axis=1)) if len(tris) else np.zeros(0, np.int64)


def _bary(rng, n, lo, hi):
    """n barycentric triples with every coordinate in [lo, hi]."""
    out = np.zeros((n, 3))
    k = 0
    while k < n:
        w = rng.dirichlet((1, 1, 1), 4 * n)
        w = w[((w >= lo) & (w <= hi)).all(axis=1)][:n - k]
        out[k:k + len(w)] = w
        k += len(w)
    return out


def _origins(rng, verts, tris, tri_ids):
    """An origin in front of each triangle (off its plane by 2 to 5 along the normal, jittered): on the
    outer side of the icosphere and above the grid."""
    p = verts[tris[tri_ids]].astype(np.float64)
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1), (0, 1, 0))
    return p.mean(axis=1) + nrm * rng.uniform(2, 5, (len(p), 1)) + rng.uniform(-0.3, 0.3, (len(p), 3))


@functools.lru_cache(maxsize=None)
def rays(name, seed=20):
    verts, tris = meshes()[name]
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    live = live_triangles(verts, tris)
    if len(live) == 0:  # nothing to aim at: aim at the grid's place
        verts, tris = meshes()["grid"]
        live = live_triangles(verts, tris)
    fin = verts[np.isfinite(verts).all(axis=1)]
    lo, hi = fin.min(axis=0).astype(np.float64), fin.max(axis=0).astype(np.float64)
    counts = dict(interior=1200, edge=700, vertex=700, miss=400, axis=400, plane=300, scaled=383, bad=16)
    assert sum(counts.values()) == N_RAYS and tuple(counts) == KINDS
    O, D, kind = [], [], []

    def put(o, d, k):
        O.append(o), D.append(d), kind.extend([KINDS.index(k)] * len(o))

    def aimed(n, target_of):
        ids = live[rng.integers(0, len(live), n)]
        o = _origins(rng, verts, tris, ids)
        return o, target_of(ids, verts[tris[ids]].astype(np.float64)) - o

    def interior(ids, p):
        return (_bary(rng, len(ids), 0.05, 0.9)[:, :, None] * p).sum(axis=1)

    def edge(ids, p):
        e, s = rng.integers(0, 3, len(ids)), rng.uniform(0.05, 0.95, (len(ids), 1))
        a, b = p[np.arange(len(ids)), e], p[np.arange(len(ids)), (e + 1) % 3]
        return a + s * (b - a)

    def vertex(ids, p):
        return p[np.arange(len(ids)), rng.integers(0, 3, len(ids))]

    for k, fn in (("interior", interior), ("edge", edge), ("vertex", vertex), ("scaled", interior)):
        o, d = aimed(counts[k], fn)
        if k == "scaled":  # unnormalised directions, short and long
            d = d * 10.0 ** rng.uniform(-3, 3, (len(d), 1))
        put(o, d, k)
    # past the silhouette: aimed at points well outside the bounds
    n = counts["miss"]
    o = (lo + hi) / 2 + (0, 6, 0) + rng.uniform(-1, 1, (n, 3))
    ring = rng.normal(size=(n, 3))
    ring[:, 1] = 0
    tgt = (lo + hi) / 2 + ring / np.linalg.norm(ring, axis=1, keepdims=True) * (np.linalg.norm(hi - lo) + 2)
    put(o, tgt - o, "miss")
    # directions with two zero components, one zero component and a subnormal component, from origins
    # above vertices, above edges and above interior points
    n = counts["axis"]
    ids = live[rng.integers(0, len(live), n)]
    p = verts[tris[ids]].astype(np.float64)
    tgt = np.where(rng.random((n, 1)) < 0.4, vertex(ids, p), np.where(rng.random((n, 1)) < 0.5, edge(ids, p), interior(ids, p)))
    axis = rng.integers(0, 3, n)
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = -rng.uniform(0.5, 2, n)
    form = rng.integers(0, 4, n)
    other = (axis + 1) % 3
    d[np.arange(n), other] = np.select([form == 1, form == 2, form == 3], [rng.uniform(-0.3, 0.3, n), 1e-40, -3e-42], 0.0)
    o = tgt - d * 3.0   # (a subnormal component leaves the origin's coordinate the target's)
    put(o, d, "axis")
    # origins exactly on triangle-box planes: one or two coordinates are a vertex's own
    n = counts["plane"]
    o, d = aimed(n, interior)
    tgt = o + d
    vv = fin[rng.integers(0, len(fin), n)].astype(np.float64)
    on = rng.random((n, 3)) < 0.5
    on[np.arange(n), rng.integers(0, 3, n)] = True
    on[np.arange(n), np.argmax(np.abs(d), axis=1)] = False   # keep the distance along the main axis
    o = np.where(on, vv, o)
    put(o, tgt - o, "plane")
    # NaN and infinite rays
    n = counts["bad"]
    o, d = aimed(n, interior)
    o, d = o.astype(np.float32), d.astype(np.float32)
    for j, val in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        o[4 * j:4 * j + 2, j % 3] = val
        d[4 * j + 2:4 * j + 4, (j + 1) % 3] = val
    put(o, d, "bad")
    origins = np.ascontiguousarray(np.concatenate(O), np.float32)
    dirs = np.ascontiguousarray(np.concatenate(D), np.float32)
    # the segments: to a point before (0.5) or beyond (1.5) what the ray aims at
    s = np.where(rng.random((N_RAYS, 1)) < 0.5, 0.5, 1.5)
    with np.errstate(invalid="ignore", over="ignore"):
        b = (origins.astype(np.float64) + dirs.astype(np.float64) * s).astype(np.float32)
    out = (origins, dirs, origins.copy(), np.ascontiguousarray(b), np.array(kind, np.int32))
    assert all(len(x) == N_RAYS for x in out)
    for x in out:
        x.setflags(write=False)
    return out
