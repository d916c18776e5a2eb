#!/usr/bin/env python
"""What does the batched first bounce of ao_batch_kernel test per prepared batch if a pool's 256
samples are dealt to its four 64-lane batches by bounce direction instead of in item order
(RT_B1_SORT)?  The pool's samples are reordered by a stable sort on a key and cut into batches of
64; each batch then goes through the float64 model of the kernel's bounce cone, per-sphere cull,
pre-test and merged exact passes of tools/explore/b1_pairs_sim.py (batch_masks, count).  Figures
are per batch with at least one live path, on sampled rows of a config's first frame; counts only,
no parity claim (results cannot depend on the order: every sample's path is a function of its item).

Keys (hemi = get_pt_within_unit_sphere(aa, pixel), known before any primary ray):
  item      today's order
  oct8      hemi's octant, the 8 bins in Gray-code order (neighbours differ in one sign); no axis
  az8/az16  the cached kernels' key: hemi's 45 / 22.5 degree sector around n0, counted from e1 towards
            e2 (e1 = normalize(n0 x ref), e2 = n0 x e1); n0 = the normal where the unjittered ray of
            the pool's middle pixel hits (emissive or not), the reversed ray when it misses
            (cull_fill_kernel's frame)
  faz8/faz16  the round-7 model: sectors counted from -pi, n0 = the normal at the pool's first live
            unjittered sample (first live sample when no pixel centre hits; oct8 when none is live)
  azdir     bound: the true bounce direction's azimuth around that n0, continuous

    python tools/explore/b1_sort_sim.py --config d --rows 12
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from b1_pairs_sim import batch_masks, count  # noqa: E402
from bench import CONFIGS, config_header  # noqa: E402
from oracle import numpy_ref as nr  # noqa: E402
from real_time_ray_tracer_amd import SSBO  # noqa: E402

F = np.float32
POOL = 256


def row_states(fr: nr.Frame, y: int):
    """b1_pairs_sim.first_bounce_states plus, per sample, hemi and the primary hit's normal, and per
    pixel the axis of its unjittered ray (the hit's normal, or the reversed ray)."""
    W, AA = fr.W, fr.AA
    x = np.arange(W)
    px, py = x.astype(F), np.full(W, y, F)
    cam = fr.hdr[4, :3]
    P = np.zeros((W, AA, 3)); Dn = np.zeros((W, AA, 3)); L = np.zeros((W, AA), bool)
    Hm = np.zeros((W, AA, 3)); N = np.zeros((W, AA, 3)); Nax = np.zeros((W, 3))
    for aa in range(AA):
        fst, snd = fr.rb[2 * aa], fr.rb[2 * aa + 1]
        if aa == 0:
            dirs = fr.primary(x, np.full(W, y))
        else:
            s1, s2, s3, s4 = (snd[0], fst[1]), (fst[2], snd[3]), (fst[0], snd[1]), (snd[2], fst[3])
            u = nr.grandom(((s1[0] + px * s2[0]) - px) + s3[0], ((s1[1] + py * s2[1]) - py) + s3[1])
            w = nr.grandom(s4[0] * px - (s3[0] * px) * s2[0], s4[1] * py - (s3[1] * py) * s2[1])
            il = F(1.0) / np.sqrt(nr.fma(w, w, u * u))
            dirs = fr.primary(x, np.full(W, y), (u * il) / F(6.0) - F(0.08333), (w * il) / F(6.0) - F(0.08333))
        a = nr.grandom(fst[0] + px * snd[2], fst[1] + py * snd[3])
        b = nr.grandom(fst[2] - px * snd[2], fst[3] - py * snd[3])
        e = nr.grandom(snd[0] * px + snd[2], snd[1] * py + snd[3])
        hemi = nr.normalize3(np.stack([a * F(2) - F(1), b * F(2) - F(1), e * F(2) - F(1)], 1))
        Hm[:, aa] = hemi
        pos = np.broadcast_to(cam, (W, 3)).astype(F)
        t, ind = fr.closest(pos, dirs, 0.0001)
        hit = ind >= 0
        if aa == 0:
            Nax[:] = -dirs
            hi = np.nonzero(hit)[0]
            if hi.size:
                Nax[hi] = fr.normal(ind[hi], cam + t[hi, None] * dirs[hi])
        emis = np.zeros(W, bool)
        emis[hit] = fr.shapes[ind[hit], 1, 3] > F(0.9)
        ci = np.nonzero(hit & ~emis)[0]
        if ci.size:
            curr = cam + t[ci, None] * dirs[ci]
            nn = fr.normal(ind[ci], curr)
            refl = fr.shapes[ind[ci], 3, 3]
            diffuse = refl > F(0.999)
            nd = np.empty_like(nn)
            nd[diffuse] = nr.normalize3(hemi[ci[diffuse]] + nn[diffuse])
            gl = ~diffuse
            if gl.any():
                dg = dirs[ci[gl]]
                dn = nr.dot3(dg, nn[gl])
                R = nr.normalize3(dg - F(2.0) * (dn[:, None] * nn[gl]))
                nd[gl] = nr.normalize3(R + refl[gl, None] * hemi[ci[gl]])
            P[ci, aa] = curr
            Dn[ci, aa] = nd
            L[ci, aa] = True
            N[ci, aa] = nn
    return P.reshape(-1, 3), Dn.reshape(-1, 3), L.reshape(-1), Hm.reshape(-1, 3), N.reshape(-1, 3), Nax


def oct8(h):
    """Bin of hemi's octant in Gray-code order: bin b holds octant b ^ (b >> 1), bit k = sign of axis k."""
    o = (h[..., 0] < 0).astype(np.int64) | (h[..., 1] < 0).astype(np.int64) << 1 | (h[..., 2] < 0).astype(np.int64) << 2
    return o ^ (o >> 1) ^ (o >> 2)


def pool_axis(L, N, AA):
    """[pools, 3] n0 and [pools] whether the pool has one: first live unjittered sample, else first live."""
    npool = L.shape[0]
    idx = np.arange(POOL)
    first0 = np.where(L & (idx % AA == 0), idx, POOL).min(1)
    first = np.where(L, idx, POOL).min(1)
    pick = np.where(first0 < POOL, first0, first)
    ok = pick < POOL
    n0 = N[np.arange(npool), np.minimum(pick, POOL - 1)]
    return n0, ok


def azimuth(v, n0):
    ref = np.where(np.abs(n0[:, :1]) < 0.9, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    e1 = np.cross(n0, ref)
    e1 /= np.maximum(np.linalg.norm(e1, axis=1, keepdims=True), 1e-30)
    e2 = np.cross(n0, e1)
    return np.arctan2((v * e2[:, None]).sum(2), (v * e1[:, None]).sum(2))  # [-pi, pi]


def keys(name, Hm, Dn, L, N, AA, Nax):
    npool = Hm.shape[0]
    if name == "item":
        return np.zeros((npool, POOL))
    if name == "oct8":
        return oct8(Hm).astype(np.float64)
    if name in ("az8", "az16"):  # the kernel's: the frame of the pool's middle pixel, sector 0 starts at e1
        tp = POOL // AA
        n0 = Nax[np.arange(npool) * tp + tp // 2]
        nb = int(name[2:])
        ang = np.mod(azimuth(Hm, n0), 2 * np.pi)
        return np.minimum(np.floor(ang / (2 * np.pi) * nb), nb - 1)
    if name in ("faz8", "faz16"):
        name = name[1:]
    if name == "octz":  # the Gray code's fastest bit on z (the view axis of the bench configs)
        return oct8(Hm[..., [2, 0, 1]]).astype(np.float64)
    n0, ok = pool_axis(L, N, AA)
    if name[0] in "xyz":  # e.g. y16: 16 sectors around a fixed world axis
        n0 = np.broadcast_to(np.eye(3)["xyz".index(name[0])], n0.shape)
        ok = np.ones_like(ok)
        name = "az" + name[1:]
    if name == "azdir":
        k = azimuth(Dn, n0)
    else:
        nb = int(name[2:])
        k = np.minimum(np.floor((azimuth(Hm, n0) + np.pi) / (2 * np.pi) * nb), nb - 1)
    return np.where(ok[:, None], k, oct8(Hm))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="d")
    ap.add_argument("--rows", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--keys", default="item,oct8,az8,az16,faz8,azdir")
    a = ap.parse_args()
    W, H, S, spp, mode, _ = CONFIGS[a.config]
    h = config_header(a.config)
    h.fill_rand_buffer(7000)
    h.set_mode(0, h.num_objects)
    s = SSBO(h, 4, 4, num_frames=1)
    fr = nr.Frame(s.data, 4, 4, h.S, h.AA, F_=1)  # (no g-buffer: the primary rays use W, H only)
    fr.W, fr.H = W, H
    geo = fr.shapes[:fr.nobj, 0]
    rows = np.random.default_rng(a.seed).choice(H, a.rows, replace=False)
    names = a.keys.split(",")
    tot = {n: dict(b1=0, kept=0, passing=0, defer=0, live=0, pairs=0) for n in names}
    for y in rows:
        P, Dn, L, Hm, N, Nax = row_states(fr, int(y))
        npool = P.shape[0] // POOL
        cut = lambda v: v[:npool * POOL].reshape(npool, POOL, *v.shape[1:])  # noqa: E731
        P, Dn, L, Hm, N = cut(P), cut(Dn), cut(L), cut(Hm), cut(N)
        for n in names:
            order = np.argsort(keys(n, Hm, Dn, L, N, fr.AA, Nax), axis=1, kind="stable")
            g = lambda v: np.take_along_axis(v, order[..., None] if v.ndim == 3 else order, 1)  # noqa: E731
            masks, keepb, nl, nk, _ = batch_masks(g(P).reshape(-1, 3), g(Dn).reshape(-1, 3), g(L).reshape(-1), geo)
            d, _, q, ps = count(masks[keepb])
            t = tot[n]
            t["b1"] += int(keepb.sum()); t["kept"] += int(nk.sum()); t["passing"] += int(ps.sum())
            t["defer"] += int(d.sum()); t["live"] += int(nl.sum()); t["pairs"] += int(q.sum())
    print(f"config {a.config}, {a.rows} rows (seed {a.seed}), {geo.shape[0]} spheres, {spp} spp; per batch with a live path:")
    print(f"{'key':6s} {'batches':>8s} {'live lanes':>10s} {'cone survivors':>14s} {'some lane passes':>16s} "
          f"{'merged exact passes':>19s} {'(ray, sphere) pairs':>19s}")
    for n in names:
        t = tot[n]
        b = max(t["b1"], 1)
        print(f"{n:6s} {t['b1']:8d} {t['live'] / b:10.1f} {t['kept'] / b:14.2f} {t['passing'] / b:16.2f} "
              f"{t['defer'] / b:19.2f} {t['pairs'] / b:19.1f}")


if __name__ == "__main__":
    main()
