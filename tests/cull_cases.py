"""Cases for the kernels' conservative culls, one family per proof (test infrastructure).

The production kernels skip most ray-shape tests on conservative proofs: the camera
cone against spheres and against planes, the first-bounce cone with its per-ray pre-test, the
cluster balls of the later bounce rounds, the shadow cone at the light.  rt_selftest_math runs each
proof beside the exact test it replaces (RT_MATH_CULL_*); these generators build its inputs, in
float64 from fixed seeds, rounded to float32 at the end.  Every family has three strata:

  GRAZING   a ray on (or just inside) the proof's boundary, and the shape tangent to that ray within
            a relative offset of +-10^U(-8, -2): about half of them are hit, half missed, and all of
            them are where a too small margin drops a shape the exact test accepts
  FAR       shapes so far outside that the proof must reject them (otherwise a test could pass
            because the proof never rejects anything); the bound of each family is derived in its
            generator's docstring from the margins in the kernels' comments, 100 times each radius
            inflation and 1e-3 on each cosine
  DEGEN     origins on / in spheres (that sphere and a touching neighbour tested), spheres behind or around the apex, r = 0, r < 0, r = 1e4, r =
            1e-3 at distance 1e3, NaN and inf rows, one live lane, opposite lanes, identical lanes,
            tiny and huge frames, planes with a zero numerator or normal

A family is a dict: "inp" the float32 rows for rt_selftest_math, "stratum" one of GRAZING / FAR /
DEGEN per case, and what the checks need to find the case's ray again ("lane": the tangent lane of
a wave family's grazing case).  tests/test_cull_cases_cpu.py checks the strata against the oracle
alone; tests/test_gpu_culls.py runs them on the device.
"""
from __future__ import annotations

import functools

import numpy as np

GRAZING, FAR, DEGEN = 0, 1, 2
N_LANE = 1 << 17   # cases of a one-lane-per-case family
N_WAVE = 4096      # cases of a one-wave-per-case family
F32 = np.float32
NAN, INF = float("nan"), float("inf")


def unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def perp(rng, d):
    """A random unit vector orthogonal to each row of d."""
    return unit(np.cross(d, unit(rng.normal(size=d.shape))))


def outward(d, a, rng):
    """The unit vector orthogonal to d that points away from the axis a (a random one where d = a)."""
    q = d - (d * a).sum(-1, keepdims=True) * a
    q = q - (q * d).sum(-1, keepdims=True) * d
    n = np.linalg.norm(q, axis=-1, keepdims=True)
    return np.where(n > 1e-9, q / np.maximum(n, 1e-300), perp(rng, d))


def eps_of(rng, n):
    """Relative tangency offsets +-10^U(-8, -2), both signs."""
    return 10.0 ** rng.uniform(-8, -2, n) * rng.choice([-1.0, 1.0], n)


def f32(a):
    return np.asarray(a, np.float64).astype(F32)


def r64(a):
    """Rounded to float32, as float64 (the value the device sees)."""
    return f32(a).astype(np.float64)


def angle(a, b):
    return np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0))


# the odd sphere rows every sphere family tests (centre relative to an anchor point, radius):
# r = 0, r < 0, huge, tiny and far, around the anchor, NaN (how a plane appears in the sphere
# table), +-inf
def odd_spheres(rng, anchor, ahead, k):
    """Row k's odd sphere for an apex / origin `anchor` whose rays go roughly along `ahead`."""
    kinds = 12
    j = k % kinds
    d = unit(ahead + 0.2 * rng.normal(size=3))
    dist = 10.0 ** rng.uniform(-0.5, 1.5)
    c, r = anchor + dist * d, 0.3 * dist
    if j == 0:
        r = 0.0
    elif j == 1:
        r = -r
    elif j == 2:
        c, r = anchor + d * (1e4 + dist), 1e4
    elif j == 3:
        c, r = anchor + 1e3 * d, 1e-3
    elif j == 4:
        c = anchor - dist * d                  # behind
    elif j == 5:
        c, r = anchor + 0.3 * dist * d, dist   # contains the apex
    elif j == 6:
        c, r = anchor + 1e4 * 0.5 * d, 1e4     # huge, contains the apex
    elif j == 7:
        c, r = anchor + r * d, r               # the apex on its surface
    elif j == 8:
        c, r = np.full(3, NAN), NAN
    elif j == 9:
        c, r = anchor + np.array([INF, 0.0, 0.0]), 1.0
    elif j == 10:
        c, r = anchor + dist * d, INF
    elif j == 11:
        c, r = anchor + np.array([0.0, -INF, 0.0]), -1.0
    return np.concatenate([c, [r]])


# ---------------------------------------------------------------------------------------------
# the camera's view: frames, rectangles and rays
# ---------------------------------------------------------------------------------------------
FRAMES = [(64, 48), (1920, 1080), (3840, 2160), (9, 1), (1, 1), (256, 64)]
RECTS = [(8, 8), (1, 1), (1, 4), (64, 1), (0, 1), (0, 3)]  # width 0: the frame's whole rows (an AO pool)
JITTER = np.array([-0.08333, 0.0, 0.0834])


def views(rng, n, frames=None, rects=None):
    """n views: a camera, its basis (float32 values), a frame and a pixel rectangle inside it."""
    fr = np.array(FRAMES)[rng.integers(0, len(FRAMES), n) if frames is None else frames]
    rc = np.array(RECTS)[rng.integers(0, len(RECTS), n) if rects is None else rects]
    W, H = fr[:, 0], fr[:, 1]
    rw = np.where(rc[:, 0] == 0, W, np.minimum(rc[:, 0], W))
    rh = np.minimum(rc[:, 1], H)
    xmin = (rng.random(n) * (W - rw + 1)).astype(np.int64)
    ymin = (rng.random(n) * (H - rh + 1)).astype(np.int64)
    edge = rng.random(n) < 0.3  # edge tiles: the widest cones of a frame
    xmin = np.where(edge, np.where(rng.random(n) < 0.5, 0, W - rw), xmin)
    ymin = np.where(edge, np.where(rng.random(n) < 0.5, 0, H - rh), ymin)
    f = unit(rng.normal(size=(n, 3)))
    u = perp(rng, f)
    w = np.cross(u, f)
    hh = rng.uniform(0.2, 0.8, n)                       # tan of half the vertical field of view
    asp = np.where(W == 256, 4.0, np.where(H == 1, 1.0, W / np.maximum(H, 1)))
    hw = hh * asp
    cam = r64(rng.uniform(-20, 20, (n, 3)))
    llc = r64(f - hw[:, None] * u - hh[:, None] * w)
    hor = r64(2 * hw[:, None] * u)
    ver = r64(2 * hh[:, None] * w)
    return dict(cam=cam, llc=llc, hor=hor, ver=ver, W=W, H=H, xmin=xmin, xmax=xmin + rw - 1, ymin=ymin,
                ymax=ymin + rh - 1)


def screen(px, j, size):
    """hp or vp of pixel px with jitter j as the kernels form it: float32 (px + j) / size."""
    return (px.astype(F32) + j.astype(F32)) / size.astype(F32)


def view_dir(v, hp, vp):
    """float64 direction of the ray at the float32 screen position (hp, vp)."""
    return unit(v["llc"] + hp.astype(np.float64)[:, None] * v["hor"] + vp.astype(np.float64)[:, None] * v["ver"])


def view_cone(v):
    """(axis, theta) of the rectangle's cone as pool_cone_f builds it (corners 0.1 px outside)."""
    W, H = v["W"].astype(np.float64), v["H"].astype(np.float64)
    hps = [(v["xmin"] - 0.1) / W, (v["xmax"] + 0.1) / W]
    vps = [(v["ymin"] - 0.1) / H, (v["ymax"] + 0.1) / H]
    ds = [unit(v["llc"] + hps[k & 1][:, None] * v["hor"] + vps[k >> 1][:, None] * v["ver"]) for k in range(4)]
    a = unit(sum(ds))
    return a, np.max([angle(a, d) for d in ds], axis=0)


def view_rows(v, hp, vp):
    """The 20 VIEW floats of RT_MATH_CULL_CAMERA / _PLANE."""
    col = lambda a: np.asarray(a, np.float64)[:, None]
    return np.concatenate([v["cam"], v["llc"], v["hor"], v["ver"], col(v["W"]), col(v["H"]), col(v["xmin"]),
                           col(v["xmax"]), col(v["ymin"]), col(v["ymax"]), col(hp), col(vp)], axis=1)


def corner_rays(rng, v):
    """Rays through the rectangle's corner pixels at the jitter's extremes and 0."""
    n = len(v["W"])
    px = np.where(rng.random(n) < 0.5, v["xmin"], v["xmax"])
    py = np.where(rng.random(n) < 0.5, v["ymin"], v["ymax"])
    return screen(px, JITTER[rng.integers(0, 3, n)], v["W"]), screen(py, JITTER[rng.integers(0, 3, n)], v["H"])


def inner_rays(rng, v):
    n = len(v["W"])
    px = v["xmin"] + (rng.random(n) * (v["xmax"] - v["xmin"] + 1)).astype(np.int64)
    py = v["ymin"] + (rng.random(n) * (v["ymax"] - v["ymin"] + 1)).astype(np.int64)
    return screen(px, rng.uniform(-0.0833, 0.0833, n), v["W"]), screen(py, rng.uniform(-0.0833, 0.0833, n), v["H"])


def far_sphere(rng, apex, a, theta, infl=0.0, forward_only=False, rho=0.0):
    """Spheres far outside the cone (apex, axis a, half-angle theta), with a mask of the rows where one
    exists.  With D = |c - apex|, r' = |r| + infl and rho the origins' spread:
        r_far = 1.01 sqrt(r'^2 + 1e-3 (D^2 + r'^2)) + rho,   r_far < 0.9 D,
        theta + alpha_far < 80 deg,  sin alpha_far = r_far / D,
        |cos phi| < cos(theta + alpha_far) - 1e-3           (forward_only: cos phi < ...)
    phi the angle between the axis and c - apex.  Returns (rows [n][4], ok [n])."""
    n = len(apex)
    D = 10.0 ** rng.uniform(-1, 3, n)
    r = D * 10.0 ** rng.uniform(-4, -0.5, n)
    rp = r + infl
    r_far = 1.01 * np.sqrt(rp * rp + 1e-3 * (D * D + rp * rp)) + rho
    with np.errstate(invalid="ignore"):
        alpha = np.arcsin(np.minimum(r_far / D, 1.0))
    K = np.cos(np.minimum(theta + alpha, np.pi)) - 1e-3
    ok = (r_far < 0.9 * D) & (theta + alpha < np.radians(80)) & (K > 2e-3)
    Ks = np.where(ok, K, 0.5) - 1e-3  # room for the rounding of the centre to float32
    cphi = rng.uniform(-1.0 if forward_only else -Ks, Ks)
    c = apex + D[:, None] * (cphi[:, None] * a + np.sqrt(1 - cphi * cphi)[:, None] * perp(rng, a))
    return np.concatenate([c, r[:, None]], axis=1), ok


def is_far_sphere(apex, a, theta, sph, infl=0.0, forward_only=False, rho=0.0):
    """far_sphere's definition evaluated on float32-rounded rows (float64 arithmetic)."""
    L = sph[:, :3] - apex
    D = np.linalg.norm(L, axis=1)
    rp = np.abs(sph[:, 3]) + infl
    r_far = 1.01 * np.sqrt(rp * rp + 1e-3 * (D * D + rp * rp)) + rho
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = np.arcsin(np.minimum(r_far / D, 1.0))
        cphi = (L * a).sum(1) / D
        K = np.cos(np.minimum(theta + alpha, np.pi)) - 1e-3
        inside = (cphi < K) if forward_only else (np.abs(cphi) < K)
        return (r_far < 0.9 * D) & (theta + alpha < np.radians(80)) & inside


def tangent_sphere(rng, o, d, a, dist_exp=(-1, 3.5), rmax=-0.1):
    """A sphere tangent, within eps_of, to the ray (o, d) on its side away from the axis a."""
    n = len(o)
    dist = 10.0 ** rng.uniform(*dist_exp, n)
    r = dist * 10.0 ** rng.uniform(-4, rmax, n)
    c = o + dist[:, None] * d + (r * (1 + eps_of(rng, n)))[:, None] * outward(d, a, rng)
    return np.concatenate([c, r[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------
# family 1: camera-ray cone vs sphere (pool_cone_f, cone_misses_f)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def camera():
    """FAR: r_far = 1.01 sqrt(r^2 + 1e-3 (D^2 + r^2)) (the code inflates r^2 by 1e-5 (D^2 + r^2)),
    r_far < 0.9 D (the code keeps spheres with D^2 <= 1.01 r_eff^2 + 1e-6), theta + alpha_far < 80 deg,
    |cos phi| < cos(theta + alpha_far) - 1e-3 (the code's slack on that cosine is 2e-5, twice)."""
    rng = np.random.default_rng(0xC0)
    n = N_LANE
    ng, nf = n // 2, n * 3 // 10
    nd = n - ng - nf
    # grazing: corner rays, the sphere tangent to them on the outside
    v = views(rng, ng)
    hp, vp = corner_rays(rng, v)
    a, _ = view_cone(v)
    rows = [np.concatenate([view_rows(v, hp, vp), tangent_sphere(rng, v["cam"], view_dir(v, hp, vp), a)], axis=1)]
    # far outside: any ray of the rectangle (full-row rectangles of wide frames leave no room: few rects there)
    v = views(rng, nf, rects=rng.choice([0, 1, 2, 3, 4], nf, p=[0.4, 0.25, 0.15, 0.15, 0.05]))
    hp, vp = inner_rays(rng, v)
    a, th = view_cone(v)
    sph, ok = far_sphere(rng, v["cam"], a, th)
    far_rows = np.concatenate([view_rows(v, hp, vp), sph], axis=1)
    rows.append(far_rows)
    # degenerate: every frame and rectangle with the odd spheres, and spheres on the rays of tiny frames
    v = views(rng, nd, frames=np.arange(nd) % len(FRAMES), rects=(np.arange(nd) // len(FRAMES)) % len(RECTS))
    hp, vp = corner_rays(rng, v)
    d = view_dir(v, hp, vp)
    sph = np.array([odd_spheres(rng, v["cam"][k], d[k], k // (len(FRAMES) * len(RECTS))) for k in range(nd)])
    rows.append(np.concatenate([view_rows(v, hp, vp), sph], axis=1))
    inp = f32(np.concatenate(rows))
    stratum = np.concatenate([np.full(ng, GRAZING), np.full(nf, FAR), np.full(nd, DEGEN)]).astype(np.uint8)
    # the far definition holds on the rounded rows (the others join the degenerate stratum)
    fr = inp[ng:ng + nf].astype(np.float64)
    still = ok & is_far_sphere(fr[:, 0:3], a, th, fr[:, 20:24])
    stratum[ng:ng + nf][~still] = DEGEN
    return dict(inp=inp, stratum=stratum)


# ---------------------------------------------------------------------------------------------
# family 2: camera-ray cone vs plane (plane_cone_misses)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane():
    """A plane is accepted only when denom = dot(n, d) has the sign of num = dot(n, p0 - cam) and
    |denom| >= 0.001.  GRAZING: n tilted outward from a corner ray d so that d has the cone's extreme
    denominator, dot(n, d) = +-0.001 (1 + eps) (within +-1e-5 of +-0.001).  FAR (the code's slack
    on the cone's extreme cosine is 1e-4; here 1e-3): with phi = angle(n, axis),
        num > 0:  cos(phi - theta') < 0.001 / |n| - 1e-3, and phi > theta'
        num < 0:  cos(phi + theta') > -0.001 / |n| + 1e-3, and phi + theta' < pi
    with cos theta' = cos theta - 2e-3.  theta' and not theta: pool_cone_f widens its cone by 2e-5 on
    the cosine of the half-angle, which for a narrow cone (one pixel of a 1920 x 1080 frame: theta =
    6e-5) is 6.3e-3 in the angle, and that much in the extreme denominator; with theta itself the
    device kept 45 of 38435 such planes, all at theta < 1e-3 (a finding about tightness, not a
    wrong cull).  100 times the widening, as for the other margins, is the 2e-3."""
    rng = np.random.default_rng(0xC1)
    n = N_LANE
    ng, nf = n // 2, n * 3 // 10
    nd = n - ng - nf
    # grazing
    v = views(rng, ng)
    hp, vp = corner_rays(rng, v)
    a, _ = view_cone(v)
    d = view_dir(v, hp, vp)
    nl = rng.choice([0.5, 1.0, 2.0, 0.01, 30.0], ng)
    sgn = rng.choice([-1.0, 1.0], ng)
    cb = np.minimum(0.001 * (1 + eps_of(rng, ng)) / nl, 1.0)
    nrm = sgn[:, None] * nl[:, None] * (cb[:, None] * d + np.sqrt(1 - cb * cb)[:, None] * outward(d, a, rng))
    p0 = v["cam"] + (10.0 ** rng.uniform(-1, 2, ng))[:, None] * unit(nrm) * sgn[:, None]
    z = np.zeros((ng, 1))
    rows = [np.concatenate([view_rows(v, hp, vp), nrm, z, p0, z], axis=1)]
    # far outside
    v = views(rng, nf, rects=rng.choice([0, 1, 2, 3, 4], nf, p=[0.4, 0.25, 0.15, 0.15, 0.05]))
    hp, vp = inner_rays(rng, v)
    a, th = view_cone(v)
    th = wider(th)
    nl = rng.choice([0.5, 1.0, 2.0, 0.01], nf)
    sgn = rng.choice([-1.0, 1.0], nf)
    bound = np.minimum(0.001 / nl - 1e-3, 1.0) - 1e-4      # cos(phi - theta) below this (num > 0)
    cpt = rng.uniform(-1.0, bound)
    phi = np.minimum(np.arccos(cpt) + th, np.pi)            # angle(n, axis) for num > 0
    okf = np.arccos(cpt) + th < np.pi
    nh = np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * perp(rng, a)
    nrm = sgn[:, None] * nl[:, None] * nh                   # (num < 0: the mirrored plane)
    p0 = v["cam"] + (10.0 ** rng.uniform(-1, 2, nf))[:, None] * nh
    z = np.zeros((nf, 1))
    rows.append(np.concatenate([view_rows(v, hp, vp), nrm, z, p0, z], axis=1))
    # degenerate
    v = views(rng, nd, frames=np.arange(nd) % len(FRAMES), rects=(np.arange(nd) // len(FRAMES)) % len(RECTS))
    hp, vp = corner_rays(rng, v)
    d = view_dir(v, hp, vp)
    kind = (np.arange(nd) // (len(FRAMES) * len(RECTS))) % 8
    nrm = unit(rng.normal(size=(nd, 3))) * rng.choice([0.5, 1.0, 2.0], nd)[:, None]
    p0 = v["cam"] + rng.normal(size=(nd, 3)) * 5
    p0[kind == 0] = v["cam"][kind == 0]                          # num == 0
    nrm[kind == 1] = 0.0                                         # n == 0
    nrm[kind == 2] = 2.0 * unit(nrm[kind == 2])                  # |n| = 2
    nrm[kind == 3] = NAN
    p0[kind == 4] = INF
    nrm[kind == 5] = np.array([INF, 0.0, 0.0])
    nrm[kind == 6] = d[kind == 6]                                # facing the ray
    nrm[kind == 7] = perp(rng, d[kind == 7]) * 1e-3              # tiny normal, parallel to the ray
    z = np.zeros((nd, 1))
    rows.append(np.concatenate([view_rows(v, hp, vp), nrm, z, p0, z], axis=1))
    inp = f32(np.concatenate(rows))
    stratum = np.concatenate([np.full(ng, GRAZING), np.full(nf, FAR), np.full(nd, DEGEN)]).astype(np.uint8)
    fr = inp[ng:ng + nf].astype(np.float64)
    stratum[ng:ng + nf][~(okf & is_far_plane(fr[:, 0:3], a, th, fr[:, 20:23], fr[:, 24:27]))] = DEGEN
    return dict(inp=inp, stratum=stratum)


def wider(theta):
    """theta' of plane()'s FAR definition: cos theta' = cos theta - 2e-3."""
    return np.arccos(np.clip(np.cos(theta) - 2e-3, -1.0, 1.0))


def is_far_plane(cam, a, theta, nrm, p0):
    """plane()'s FAR definition; theta is theta' there."""
    nl = np.linalg.norm(nrm, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        num = (nrm * (p0 - cam)).sum(1)
        phi = np.arccos(np.clip((nrm * a).sum(1) / nl, -1, 1))
        pos = (num > 0) & (phi > theta) & (np.cos(phi - theta) < 0.001 / nl - 1e-3)
        neg = (num < 0) & (phi + theta < np.pi) & (np.cos(phi + theta) > -0.001 / nl + 1e-3)
    return pos | neg


# ---------------------------------------------------------------------------------------------
# wave families: 64 rays per case
# ---------------------------------------------------------------------------------------------
def cone_dirs(rng, a, theta, m=64):
    """m unit directions per row inside the cone (a, theta), in opposite pairs about a so that their
    sum is along a; pair 0 (lanes 0 and 1) lies on the cone's surface."""
    n = len(a)
    th = theta[:, None] * np.sqrt(rng.random((n, m // 2)))
    th[:, 0] = theta
    q = unit(np.cross(a[:, None, :], unit(rng.normal(size=(n, m // 2, 3)))))
    c, s = np.cos(th)[..., None], np.sin(th)[..., None]
    return np.stack([c * a[:, None, :] + s * q, c * a[:, None, :] - s * q], axis=2).reshape(n, m, 3)


def live_masks(rng, n, m=64):
    """Live lanes: lanes 0 and 1 (the pair on the cone's surface) always, the others at random in
    whole pairs (so the live directions still sum along the axis)."""
    p = rng.choice([1.0, 0.9, 0.5, 0.1, 0.0], n)[:, None]
    live = np.repeat(rng.random((n, m // 2)) < p, 2, axis=1)
    live[:, :2] = True
    return live


def wave_cone(d, live):
    """(axis, theta) of the live directions as the kernels build it: the normalised sum, the largest angle."""
    a = unit((d * live[..., None]).sum(1))
    ang = np.where(live, angle(a[:, None, :], d), 0.0)
    return a, ang.max(1)


# ---------------------------------------------------------------------------------------------
# family 3: first-bounce cone and per-ray pre-test (bounce_cone, bounce_cone_misses, _keep_pt)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bounce():
    """The live rays start within rho of lane 0's origin o and go into the cone (axis, theta) of their
    directions.  GRAZING: the sphere is tangent to a live ray on the side away from the axis: to a
    ray on the cone's surface (lanes 0 / 1, half of the cases; the pre-test's boundary for that lane
    too), or to any live ray (the pre-test alone).  FAR, with L = |c - o|, rho' = 1.01 rho + 1e-4 (|o.x|
    + |o.y| + |o.z|) (the code: 1.0001 rho + 1e-6 |o|_1) and Lmax = L + rho':
        r_far = 1.01 sqrt(r^2 + 1e-3 (Lmax^2 + r^2)) + rho'   (the code: 1e-5, times 1.00001, + rho)
        r_far < 0.9 L   (the code's (1): L - rho - r > 1e-2 Lmax; 100 times that margin cannot hold)
        theta + alpha_far < 80 deg, cos phi < cos(theta + alpha_far) - 1e-3   (the code: 2e-5)
    with the forward cone only (phi up to 180 deg: the sphere may lie behind)."""
    rng = np.random.default_rng(0xC2)
    n = N_WAVE
    ng, nf = n // 2, n * 3 // 10
    nd = n - ng - nf
    a = unit(rng.normal(size=(n, 3)))
    theta = 10.0 ** rng.uniform(-3, np.log10(1.5), n)
    theta[ng:ng + nf] = 10.0 ** rng.uniform(-3, np.log10(1.0), nf)
    d = cone_dirs(rng, a, theta)
    live = live_masks(rng, n)
    o = rng.uniform(-20, 20, (n, 3)) * rng.choice([0.0, 1.0, 1.0, 50.0], n)[:, None]
    rho = 10.0 ** rng.uniform(-5, -0.5, n) * rng.choice([0.0, 1.0, 1.0], n)
    p = o[:, None, :] + rho[:, None, None] * unit(rng.normal(size=(n, 64, 3))) * rng.random((n, 64, 1))
    p[:, 0] = o
    lane = np.zeros(n, np.int64)
    sph = np.zeros((n, 4))
    # grazing
    k = np.arange(ng)
    anyl = np.array([rng.choice(np.flatnonzero(live[i])) for i in k])
    lane[:ng] = np.where(rng.random(ng) < 0.5, rng.integers(0, 2, ng), anyl)
    ax, _ = wave_cone(d[:ng], live[:ng])
    sph[:ng] = tangent_sphere(rng, p[k, lane[:ng]], d[k, lane[:ng]], ax, dist_exp=(-2, 3), rmax=-0.2)
    # far outside
    s = slice(ng, ng + nf)
    ax, th = wave_cone(d[s], live[s])
    rhop = 1.01 * np.linalg.norm(r64(p[s]) - r64(o[s])[:, None, :], axis=2).max(1) + 1e-4 * np.abs(o[s]).sum(1)
    sph[s], ok = far_sphere(rng, o[s], ax, th, forward_only=True, rho=rhop)
    # degenerate
    for i in range(ng + nf, n):
        j = i - ng - nf
        kind = j % 8
        if kind == 0:      # one live lane
            live[i] = False
            live[i, rng.integers(0, 64)] = True
        elif kind == 1:    # two live lanes with opposite directions: the sum cancels
            live[i] = False
            live[i, :2] = True
            d[i, 1] = -d[i, 0]
        elif kind == 2:    # 64 identical lanes
            p[i], d[i], live[i] = p[i, 0], d[i, 0], True
        elif kind == 3:    # origins on a sphere's surface, outward: that sphere, then a touching neighbour
            r0 = 10.0 ** rng.uniform(-1, 1)
            c0 = o[i] - r0 * a[i]
            nn = unit(a[i] + 0.05 * rng.normal(size=(64, 3)))
            p[i] = c0 + r0 * nn
            d[i] = unit(nn + 0.7 * unit(rng.normal(size=(64, 3))))
            o[i] = p[i, 0]
            if j % 16 < 8:
                sph[i] = np.concatenate([c0, [r0]])
            else:
                r1 = r0 * 10.0 ** rng.uniform(-1, 1)
                sph[i] = np.concatenate([c0 + (r0 + r1) * nn[rng.integers(0, 64)], [r1]])
            continue
        first = int(np.flatnonzero(live[i])[0])
        sph[i] = odd_spheres(rng, p[i, first], d[i, first], j // 8)
    lane[ng + nf:] = [int(np.flatnonzero(live[i])[0]) for i in range(ng + nf, n)]
    rows = np.concatenate([p, d, live[..., None].astype(np.float64)], axis=2).reshape(n, 64 * 7)
    inp = f32(np.concatenate([sph, rows], axis=1))
    stratum = np.concatenate([np.full(ng, GRAZING), np.full(nf, FAR), np.full(nd, DEGEN)]).astype(np.uint8)
    # the far definition on the rounded rows
    fr = inp[s].astype(np.float64)
    pr = fr[:, 4:].reshape(nf, 64, 7)
    lv = pr[..., 6] != 0
    first = lv.argmax(1)
    of = pr[np.arange(nf), first, 0:3]
    ax, th = wave_cone(pr[..., 3:6], lv)
    rhop = 1.01 * (np.linalg.norm(pr[..., 0:3] - of[:, None, :], axis=2) * lv).max(1) + 1e-4 * np.abs(of).sum(1)
    still = ok & is_far_sphere(of, ax, th, fr[:, 0:4], forward_only=True, rho=rhop)
    stratum[s][~still] = DEGEN
    return dict(inp=inp, stratum=stratum, lane=lane)


def bounce_parts(inp):
    """(sphere [n][4], origin [n][64][3], direction [n][64][3], live [n][64]) of bounce()'s rows."""
    r = inp[:, 4:].reshape(len(inp), 64, 7)
    return inp[:, :4], r[..., 0:3], r[..., 3:6], r[..., 6] != 0


# ---------------------------------------------------------------------------------------------
# family 5: shadow cone at the light (shadow_cone, cone_misses_f on r + 1e-4)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shadow():
    """The shadow lines of the lanes in need run from the light into the cone (axis, theta) of their
    directions.  GRAZING: the sphere is tangent to a needing lane's line between the light and the
    shaded point, away from the axis (lanes 0 / 1 lie on the cone's surface).  FAR: the camera
    family's bound with the apex at the light and r' = r + 1e-2 (the code tests r + 1e-4):
        r_far = 1.01 sqrt(r'^2 + 1e-3 (D^2 + r'^2)), r_far < 0.9 D, theta + alpha_far < 80 deg,
        |cos phi| < cos(theta + alpha_far) - 1e-3
    (80 deg also keeps the cone from being 'wide', cos theta <= 0.05, where nothing is culled), and
    every shaded point within 9 D of the light.  The last bound is the exact test's, not the proof's: a
    shadow ray starts at the shaded point, so its computed discriminant errs by up to ~7e-7 Lmax^2
    (DESIGN.md §5), Lmax = |point - c| <= len + D, while the far sphere's exact discriminant is only
    <= -1e-3 D^2 below zero; with Lmax < 10 D that is 14 times the error, and the reference misses.
    Beyond it the reference itself can report a hit on a sphere hundreds of radii off the line (seen
    in the oracle at len = 250 D), so such cases say nothing about 'far outside'.  They are cases of
    their own in the degenerate stratum (kinds 5 and 6, 204 cases: a small sphere at D from the light,
    0.01 to 1 rad outside the cone, lines up to 3000 D long; the oracle reports an occluder in 82):
    a cone whose margins follow D alone culls what the reference's rounding accepts there, and the
    kernel's did in 75 of them until shadow_cone_keeps took the longest line into the radius.  The
    grazing stratum also puts its tangent sphere down to len / 3000 from the light."""
    rng = np.random.default_rng(0xC4)
    n = N_WAVE
    ng, nf = n // 2, n * 3 // 10
    nd = n - ng - nf
    a = unit(rng.normal(size=(n, 3)))
    theta = 10.0 ** rng.uniform(-3, np.log10(1.4), n)
    theta[ng:ng + nf] = 10.0 ** rng.uniform(-3, np.log10(1.0), nf)
    d = cone_dirs(rng, a, theta)
    need = live_masks(rng, n)
    light = rng.uniform(-20, 20, (n, 3)) * rng.choice([0.0, 1.0, 1.0, 50.0], n)[:, None]
    ln = 10.0 ** rng.uniform(-0.5, 2.5, (n, 64))
    lane = np.zeros(n, np.int64)
    sph = np.zeros((n, 4))
    # grazing: tangent to the line of a lane in need, between the light and the point
    k = np.arange(ng)
    anyl = np.array([rng.choice(np.flatnonzero(need[i])) for i in k])
    lane[:ng] = np.where(rng.random(ng) < 0.6, rng.integers(0, 2, ng), anyl)
    ax, _ = wave_cone(d[:ng], need[:ng])
    dl, ll = d[k, lane[:ng]], ln[k, lane[:ng]]
    s_ = ll * np.where(rng.random(ng) < 0.5, rng.uniform(0.2, 0.8, ng), 10.0 ** rng.uniform(-3.5, -0.1, ng))
    r = np.minimum(s_, ll - s_) * 10.0 ** rng.uniform(-4, -0.3, ng)
    c = light[:ng] + s_[:, None] * dl + (r * (1 + eps_of(rng, ng)))[:, None] * outward(dl, ax, rng)
    sph[:ng] = np.concatenate([c, r[:, None]], axis=1)
    # far outside
    s = slice(ng, ng + nf)
    ax, th = wave_cone(d[s], need[s])
    sph[s], ok = far_sphere(rng, light[s], ax, th, infl=1e-2)
    Dl = np.linalg.norm(sph[s, :3] - light[s], axis=1)
    # (a quarter keep their long lines, up to 3000 D: far outside for the cone, not for the exact test,
    # so they end in the degenerate stratum; see the docstring)
    ln[s] = np.where(rng.random((nf, 1)) < 0.75, Dl[:, None] * 10.0 ** rng.uniform(-2, 0.9, (nf, 64)), ln[s])
    pos = light[:, None, :] + ln[..., None] * d
    # degenerate
    for i in range(ng + nf, n):
        j = i - ng - nf
        kind = j % 8
        if kind == 0:      # one lane in need
            need[i] = False
            need[i, rng.integers(0, 64)] = True
        elif kind == 1:    # two lanes in need, on opposite sides of the light
            need[i] = False
            need[i, :2] = True
            pos[i, 1] = light[i] - ln[i, 1] * d[i, 0]
        elif kind == 2:    # 64 identical lanes
            pos[i], need[i] = pos[i, 0], True
        elif kind == 3:    # the light inside the sphere
            r0 = 10.0 ** rng.uniform(-1, 1.5)
            sph[i] = np.concatenate([light[i] + 0.5 * r0 * unit(rng.normal(size=3)), [r0]])
            continue
        elif kind == 4:    # the light at less than 0.01 from the shaded points
            pos[i] = light[i] + 10.0 ** rng.uniform(-5, -2, (64, 1)) * d[i]
        elif kind in (5, 6):  # long lines past a small sphere next to the light, psi outside the cone: the
            # cone's margins scale with the sphere's distance D from the light, the exact test's error
            # with the line's length (up to 3000 D here)
            L0 = 10.0 ** rng.uniform(0, 2.5)
            pos[i] = light[i] + L0 * rng.uniform(0.7, 1.3, (64, 1)) * d[i]
            D = 0.7 * L0 * 10.0 ** rng.uniform(-3.5, -1.3)
            r0 = D * 10.0 ** rng.uniform(-3, -1)
            ax, th = wave_cone(d[i:i + 1], need[i:i + 1])
            phi = th[0] + 10.0 ** rng.uniform(-2, 0) + 2 * np.arcsin(min(1.0, r0 / D + 0.004 + 1e-4 / D))
            phi = min(phi, np.pi - 0.02)
            sph[i] = np.concatenate([light[i] + D * (np.cos(phi) * ax[0] + np.sin(phi) * perp(rng, ax)[0]), [r0]])
            continue
        elif kind == 7:    # the shaded points on a sphere S, as every Phong / hybrid shadow ray's are: its lit
            # cap up to the terminator (lanes 0-7 on it: the lines that graze S and set the cone's
            # half-angle); tested: S itself, then a neighbour touching S at one of the points
            Dd = 10.0 ** rng.uniform(-0.5, 2)
            r0 = Dd * 10.0 ** rng.uniform(-2, -0.05)
            u = unit(rng.normal(size=3))                       # from S's centre towards the light
            c0 = light[i] - Dd * u
            gt = np.arccos(r0 / Dd)                            # the terminator's angle from u
            g = gt * np.sqrt(rng.random(64))
            g[:8] = gt
            nn = np.cos(g)[:, None] * u + np.sin(g)[:, None] * perp(rng, np.tile(u, (64, 1)))
            pos[i] = c0 + r0 * nn
            need[i] = rng.random(64) < rng.choice([1.0, 0.7])
            need[i, :2] = True
            if j % 16 < 8:
                sph[i] = np.concatenate([c0, [r0]])
            else:
                r1 = r0 * 10.0 ** rng.uniform(-1, 1)
                sph[i] = np.concatenate([c0 + (r0 + r1) * nn[rng.integers(0, 64)], [r1]])
            continue
        first = int(np.flatnonzero(need[i])[0])
        sph[i] = odd_spheres(rng, light[i], unit(pos[i, first] - light[i]), j // 8)
    lane[ng + nf:] = [int(np.flatnonzero(need[i])[0]) for i in range(ng + nf, n)]
    rows = np.concatenate([pos, need[..., None].astype(np.float64)], axis=2).reshape(n, 64 * 4)
    inp = f32(np.concatenate([light, sph, rows], axis=1))
    stratum = np.concatenate([np.full(ng, GRAZING), np.full(nf, FAR), np.full(nd, DEGEN)]).astype(np.uint8)
    fr = inp[s].astype(np.float64)
    pr = fr[:, 7:].reshape(nf, 64, 4)
    nd_ = pr[..., 3] != 0
    ax, th = wave_cone(unit(pr[..., 0:3] - fr[:, None, 0:3]), nd_)
    near = (np.linalg.norm(pr[..., 0:3] - fr[:, None, 0:3], axis=2) * nd_).max(1) < 9 * np.linalg.norm(fr[:, 3:6] - fr[:, 0:3], axis=1)
    stratum[s][~(ok & near & is_far_sphere(fr[:, 0:3], ax, th, fr[:, 3:7], infl=1e-2))] = DEGEN
    return dict(inp=inp, stratum=stratum, lane=lane)


def shadow_parts(inp):
    """(light [n][3], sphere [n][4], point [n][64][3], need [n][64]) of shadow()'s rows."""
    r = inp[:, 7:].reshape(len(inp), 64, 4)
    return inp[:, 0:3], inp[:, 3:7], r[..., 0:3], r[..., 3] != 0


# ---------------------------------------------------------------------------------------------
# family 4: cluster ball vs ray (cluster_may_hit, cluster_may_hit_mask; build_clusters on the host)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cluster():
    """A cluster (centre, R) holds members with |c_i - centre| + |r_i| <= R.  GRAZING: a member that
    touches the ball's surface from inside at T = centre + R u, and a ray orthogonal to u that passes
    the member's centre at r_i (1 + eps) on T's side (tangent to member and ball at once: the line
    test's boundary), from origins up to 1e4 R away; or the origin at R (1 + |eps|) on that side with
    the ray pointing away within 90 deg (the behind test's boundary).  FAR, u = |p - centre|, Lmax = u + R:
        (A) R_far = R + 0.32 (Lmax + R)        (the code: 0.0032), and the line passes the centre at
            h with h^2 > R_far^2 + 4e-4 u^2     (the code: 4e-6 u^2);
        (B) or d . (centre - p) < -R_far - 0.1 (u + R_far) with u - R_far > 0.1 (u + R_far) (the code:
            1e-3 and 1e-2; 100 times the latter cannot hold, so 10 times)."""
    rng = np.random.default_rng(0xC3)
    n = N_LANE
    ng, nf = n // 2, n * 3 // 10
    nd = n - ng - nf
    ctr = rng.uniform(-20, 20, (n, 3)) * rng.choice([0.0, 1.0, 1.0, 50.0], n)[:, None]
    R = 10.0 ** rng.uniform(-2, 4, n)
    u = unit(rng.normal(size=(n, 3)))
    ri = R * 10.0 ** rng.uniform(-3, 0, n)                     # the member's radius, up to R (a cluster of one)
    ci = ctr + (R - ri)[:, None] * u                           # touches the ball at T = ctr + R u
    p, d = np.zeros((n, 3)), np.zeros((n, 3))
    # grazing, the line test
    k = slice(0, ng * 3 // 4)
    m = ng * 3 // 4
    d[k] = perp(rng, u[k])
    back = R[k] * 10.0 ** rng.uniform(-2, 4, m)
    p[k] = ci[k] + (ri[k] * (1 + eps_of(rng, m)))[:, None] * u[k] - back[:, None] * d[k]
    # grazing, the behind test: just outside the ball at T, pointing away
    k = slice(m, ng)
    m2 = ng - m
    p[k] = ctr[k] + (R[k] * (1 + np.abs(eps_of(rng, m2))))[:, None] * u[k]
    tilt = rng.uniform(0, np.pi / 2, m2)
    d[k] = np.cos(tilt)[:, None] * u[k] + np.sin(tilt)[:, None] * perp(rng, u[k])
    # far outside: any member inside the ball
    k = slice(ng, ng + nf)
    ri[k] = R[k] * 10.0 ** rng.uniform(-3, -0.1, nf)
    ci[k] = ctr[k] + ((R[k] - ri[k]) * rng.random(nf))[:, None] * u[k]
    uu = R[k] * 10.0 ** rng.uniform(0.5, 3, nf)                # |p - centre|
    w = unit(rng.normal(size=(nf, 3)))
    p[k] = ctr[k] + uu[:, None] * w
    Rf = R[k] + 0.32 * (uu + 2 * R[k])
    kindA = rng.random(nf) < 0.6
    # (A): sin of the angle between d and centre - p above sqrt(R_far^2 + 4e-4 u^2) / u; (B): d within
    # acos((R_far + 0.1 (u + R_far)) / u) of w
    sA = np.sqrt(Rf * Rf + 4e-4 * uu * uu) / uu
    cB = (Rf + 0.1 * (uu + Rf)) / uu
    okf = np.where(kindA, sA < 0.98, (cB < 0.98) & (uu - Rf > 0.1 * (uu + Rf)))
    angA = np.arcsin(np.minimum(sA, 1.0)) + 0.01 + rng.random(nf) * (np.pi - 2 * np.arcsin(np.minimum(sA, 1.0)) - 0.02)
    angB = np.arccos(np.minimum(cB, 1.0)) * rng.random(nf) * 0.98
    ang = np.where(kindA, angA, angB)                          # measured from w (pointing away from the centre)
    d[k] = np.cos(ang)[:, None] * w + np.sin(ang)[:, None] * perp(rng, w)
    # degenerate: origins on and in the member, odd members and balls
    k = np.arange(ng + nf, n)
    kind = (k - ng - nf) % 8
    d[k] = unit(rng.normal(size=(nd, 3)))
    p[k] = ctr[k] + (R[k] * 10.0 ** rng.uniform(-1, 1, nd))[:, None] * unit(rng.normal(size=(nd, 3)))
    on = k[kind == 0]                                          # on the member's surface, going outward
    nn = unit(rng.normal(size=(len(on), 3)))
    p[on] = ci[on] + ri[on][:, None] * nn
    d[on] = unit(nn + 0.9 * unit(rng.normal(size=(len(on), 3))))
    # every other one tests a neighbour that touches that sphere at (or near) the origin instead: the
    # member is the neighbour, and the ball is drawn around it
    nb = on[1::2]
    r1 = ri[nb] * 10.0 ** rng.uniform(-1, 1, len(nb))
    off = unit(nn[1::2] + 0.3 * rng.normal(size=(len(nb), 3)) * rng.choice([0.0, 1.0], (len(nb), 1)))
    ci[nb] = ci[nb] + (ri[nb] + r1)[:, None] * off
    ri[nb] = r1
    R[nb] = (np.linalg.norm(ci[nb] - ctr[nb], axis=1) + r1) * (1 + 1e-6)
    ins = k[kind == 1]                                         # inside the member
    p[ins] = ci[ins] + (0.5 * ri[ins])[:, None] * unit(rng.normal(size=(len(ins), 3)))
    sph = np.concatenate([ci, ri[:, None]], axis=1)
    for i in k[kind == 2]:
        sph[i] = odd_spheres(rng, p[i], d[i], int(rng.integers(0, 12)))
    # an odd member's ball is drawn around it (infinite rows are never a cluster's members: the host
    # tests them in every round; a NaN row stays, as what no test accepts), and the ball of radius 0
    # holds a point at its centre
    odd = k[kind == 2]
    sph[odd] = np.where(np.isinf(sph[odd]).any(1, keepdims=True), np.concatenate([ci, ri[:, None]], axis=1)[odd], sph[odd])
    fin = odd[np.isfinite(sph[odd]).all(1)]
    R[fin] = (np.linalg.norm(sph[fin, :3] - ctr[fin], axis=1) + np.abs(sph[fin, 3])) * (1 + 1e-6)
    R[k[kind == 3]] = 0.0
    sph[k[kind == 3]] = np.concatenate([ctr, np.zeros((n, 1))], axis=1)[k[kind == 3]]
    R[k[kind == 4]] = NAN
    R[k[kind == 5]] = INF
    ctr[k[kind == 6]] = NAN
    d[k[kind == 7]] = 0.0
    d = np.where(np.isfinite(d).all(1, keepdims=True) & (np.abs(d).sum(1, keepdims=True) > 0), unit(np.where(d == 0, 1e-300, d)), d)
    inp = f32(np.concatenate([p, d, ctr, R[:, None], sph], axis=1))
    stratum = np.concatenate([np.full(ng, GRAZING), np.full(nf, FAR), np.full(nd, DEGEN)]).astype(np.uint8)
    fr = inp[ng:ng + nf].astype(np.float64)
    stratum[ng:ng + nf][~(okf & is_far_cluster(fr))] = DEGEN
    return dict(inp=inp, stratum=stratum)


def is_far_cluster(rows):
    """cluster()'s FAR definition on float32-rounded rows, and the member inside the ball."""
    p, d, ctr, R, ci, ri = rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9], rows[:, 10:13], rows[:, 13]
    v = ctr - p
    uu = np.linalg.norm(v, axis=1)
    b = (d * v).sum(1)
    Rf = R + 0.32 * (uu + 2 * R)
    A = uu * uu - b * b > Rf * Rf + 4e-4 * uu * uu
    B = (b < -Rf - 0.1 * (uu + Rf)) & (uu - Rf > 0.1 * (uu + Rf))
    member = np.linalg.norm(ci - ctr, axis=1) + np.abs(ri) <= R * (1 + 1e-6)
    return (A | B) & member


TABLE_SCENES = ["syn64", "syn200", "adv256"]
TABLE_PAIRS = 1 << 18


def table_header(name):
    from real_time_ray_tracer_amd import Header, aspect_for

    if name == "adv256":
        import adversarial_scenes

        return adversarial_scenes.scene("adv256", 64, 48, 4)[0]
    return Header.synthetic(int(name[3:]), 4, 1234, aspect_for(64, 48))


@functools.lru_cache(maxsize=None)
def cluster_tables():
    """The cluster tables the library builds for TABLE_SCENES, with rays as the bounce rounds meet them:
    from random points of random sphere surfaces into the outward hemisphere, against every cluster and
    each of its members; TABLE_PAIRS ray-member pairs in all (a multiple of 64)."""
    rng = np.random.default_rng(0xC5)
    out = []
    for name in TABLE_SCENES:
        h = table_header(name)
        clus, _always, masks = h.cluster_table()
        geo = h.shapes[:h.num_objects, 0].astype(np.float64)
        pairs = [(c, i) for c in range(len(clus)) for i in range(h.num_objects) if int(masks[c, i >> 6]) >> (i & 63) & 1]
        pairs = np.array(pairs)
        per = TABLE_PAIRS // len(TABLE_SCENES) // 64 * 64 if name != TABLE_SCENES[-1] else None
        out.append((clus, geo, pairs, per))
    rows, used = [], 0
    for clus, geo, pairs, per in out:
        m = per if per is not None else TABLE_PAIRS - used
        used += m
        nrays = -(-m // len(pairs))
        src = geo[rng.integers(0, len(geo), nrays)]
        src = src[np.isfinite(src).all(1)]
        src = src[rng.integers(0, len(src), nrays)]
        nn = unit(rng.normal(size=(nrays, 3)))
        p = src[:, :3] + np.abs(src[:, 3:4]) * nn
        d = unit(nn + 0.99 * unit(rng.normal(size=(nrays, 3))))
        ray = np.repeat(np.arange(nrays), len(pairs))[:m]
        pr = np.tile(pairs, (nrays, 1))[:m]
        rows.append(np.concatenate([p[ray], d[ray], clus[pr[:, 0]].astype(np.float64), geo[pr[:, 1]]], axis=1))
    inp = f32(np.concatenate(rows))
    assert len(inp) == TABLE_PAIRS
    return dict(inp=inp)


FAMILIES = {"camera": camera, "plane": plane, "bounce": bounce, "cluster": cluster, "shadow": shadow}


# ---------------------------------------------------------------------------------------------
# the oracle's exact tests on a family's rows (computed once per process)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact(name):
    """The oracle's value of the exact test on every ray of family `name` (or "tables"):
    camera   dict(dir [n][3], t [n])          sphere_eval at the oracle's primary direction
    plane    dict(dir, t)                     plane_eval there
    bounce   dict(t [n][64])                  sphere_eval per lane
    cluster  dict(t [n])                      sphere_eval of the member
    shadow   dict(occ [n][64])                shadow_ray's decision per lane
    and "acc": the cases (lanes) that the scan accepts at the family's most permissive threshold."""
    import oracle

    inp = cluster_tables()["inp"] if name == "tables" else FAMILIES[name]()["inp"]
    if name in ("camera", "plane"):
        d = oracle.primary_dir_n(inp[:, 3:12], inp[:, 18], inp[:, 19])
        if name == "camera":
            t = oracle.sphere_eval_n(inp[:, 0:3], d, inp[:, 20:24])
        else:
            t = oracle.plane_eval_n(inp[:, 0:3], d, inp[:, 20:23], inp[:, 24:27])
        return dict(dir=d, t=t, acc=t > 0)
    if name == "bounce":
        sph, p, d, live = bounce_parts(inp)
        t = oracle.sphere_eval_n(p, d, np.repeat(sph, 64, axis=0)).reshape(-1, 64)
        return dict(t=t, acc=(t > F32(0.0001)) & live)
    if name in ("cluster", "tables"):
        t = oracle.sphere_eval_n(inp[:, 0:3], inp[:, 3:6], inp[:, 10:14])
        return dict(t=t, acc=t > F32(0.0001))
    light, sph, pos, need = shadow_parts(inp)
    occ = oracle.shadow_occludes_n(np.repeat(light, 64, axis=0), pos, np.repeat(sph, 64, axis=0)).reshape(-1, 64)
    return dict(occ=occ, acc=occ & need)
