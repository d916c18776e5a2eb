"""ctypes binding of librtrt_mesh.so (include/rt/mesh.h): triangle meshes, their ray queries on the
GPU, the host-only specification and the OBJ reader.

The companion library is required like librtrt.so: a missing build is an error, never a fall-back.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from ._lib import RT_E_INVAL, RT_OK, RtError, fptr

LIB_NAME = "librtrt_mesh.so"
LIB_PATH = Path(__file__).resolve().with_name(LIB_NAME)

RT_MESH_MAX_TRIANGLES = 1 << 24
RT_MESH_LEAF = 4
RT_MESH_SINGLE_LEAF = 8
RT_MESH_ONE_ORIGIN = 1
RT_MESH_MERGE = 2

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p
_mesh = C.c_void_p
_pi = C.POINTER(C.c_int)

# name -> (restype, argtypes); every function declared in include/rt/mesh.h
SIGNATURES = {
    "rt_mesh_create": (C.c_int, [C.c_int, _fp, C.c_int, _ip, C.c_int, C.POINTER(_mesh)]),
    "rt_mesh_destroy": (C.c_int, [_mesh]),
    "rt_mesh_stats": (C.c_int, [_mesh, _pi, _pi, _pi, C.POINTER(C.c_size_t)]),
    "rt_mesh_last_hip_error": (C.c_int, [_mesh]),
    "rt_mesh_workspace_bytes": (C.c_size_t, [_mesh]),
    "rt_mesh_synchronize": (C.c_int, [_mesh]),
    "rt_mesh_trace_rays": (C.c_int, [_mesh, _fp, _fp, C.c_size_t, C.c_int, C.c_float, _fp, _ip, _fp, _fp]),
    "rt_mesh_occluded": (C.c_int, [_mesh, _fp, _fp, C.c_size_t, C.c_int, _vp]),
    "rt_mesh_trace_rays_device": (C.c_int, [_mesh, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_float, _vp, _vp, _vp, _vp]),
    "rt_mesh_occluded_device": (C.c_int, [_mesh, _vp, _vp, _vp, C.c_size_t, C.c_int, _vp]),
    "rt_mesh_tri_eval_host": (C.c_float, [_fp, _fp, _fp, _fp, _fp, _fp]),
    "rt_mesh_box_pass_host": (C.c_int, [_fp, _fp, _fp, _fp]),
    "rt_mesh_trace_rays_host": (C.c_int, [_fp, C.c_int, _ip, C.c_int, _fp, _fp, C.c_size_t, C.c_int, C.c_float, _fp, _ip,
                                          _fp, _fp]),
    "rt_mesh_occluded_host": (C.c_int, [_fp, C.c_int, _ip, C.c_int, _fp, _fp, C.c_size_t, C.c_int, _vp]),
    "rt_mesh_bvh_host": (C.c_int, [_fp, C.c_int, _ip, C.c_int, _fp, _ip, C.c_int, _ip, C.c_int, _pi]),
    "rt_obj_parse": (C.c_int, [C.c_char_p, C.c_size_t, _fp, C.c_int, _ip, C.c_int, _pi, _pi, _pi]),
}

_LIB = None


def load() -> C.CDLL:
    """Load librtrt_mesh.so (in-tree, or RTRT_MESH_LIB).  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = Path(os.environ.get("RTRT_MESH_LIB", LIB_PATH))
    if not path.exists():
        raise RuntimeError(f"{path} not found: the mesh library is required (build it with `make lib` "
                           f"or __graft_entry__.build()); there is no CPU fallback")
    # one HIP runtime per process, the one librtrt.so uses (see _lib.load): torch's first when installed
    if os.environ.get("RTRT_NO_TORCH_FIRST") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(str(path))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def _check(rc: int, what: str, mesh=None) -> int:
    if rc < 0:
        raise RtError(rc, what, load().rt_mesh_last_hip_error(mesh) if mesh else 0)
    return rc


def _iptr(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _bptr(a):
    return a.ctypes.data_as(_vp) if a is not None else None


def _dptr(p):
    return C.c_void_p(int(p)) if p else None


def _rows(a, w: int, dtype) -> np.ndarray:
    a = np.asarray(a)
    if dtype == np.int32 and a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError("triangle indices must be integers")
    if a.size % w:
        raise ValueError(f"need rows of {w} values, got shape {a.shape}")
    return np.ascontiguousarray(a.reshape(-1, w), dtype)


def _f3(v):
    return fptr(np.ascontiguousarray(v, np.float32).reshape(3))


@dataclass
class MeshHits:
    """Closest hits of n rays on a mesh: t [n] float32 (-1: a miss), prim [n] int32 (the triangle; -1:
    a miss, or with merge: the earlier answer stands), normals [n][3] (the triangle's stored
    orientation), uv [n][2] (the barycentrics of v1 and v2)."""
    t: np.ndarray
    prim: np.ndarray
    normals: np.ndarray
    uv: np.ndarray


def _hits(n: int, merge) -> MeshHits:
    """Empty outputs, or copies of the earlier answer merge = (t, normals) / an object with .t and .normals."""
    if merge is None:
        return MeshHits(np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32),
                        np.zeros((n, 2), np.float32))
    t, nrm = (merge.t, merge.normals) if hasattr(merge, "t") else merge
    t = np.array(t, np.float32).reshape(-1)
    nrm = np.array(nrm, np.float32).reshape(-1, 3)
    if len(t) != n or len(nrm) != n:
        raise ValueError(f"merge: {len(t)} t and {len(nrm)} normals for {n} rays")
    return MeshHits(t, np.zeros(n, np.int32), nrm, np.zeros((n, 2), np.float32))


def _rays(origins, dirs, one_origin: bool, what: str):
    o, d = _rows(origins, 3, np.float32), _rows(dirs, 3, np.float32)
    if len(o) != (1 if one_origin else len(d)):
        raise ValueError(f"{what}: {len(o)} origins, {len(d)} directions")
    return o, d


def _flags(one_origin: bool, merge) -> int:
    return (RT_MESH_ONE_ORIGIN if one_origin else 0) | (RT_MESH_MERGE if merge is not None else 0)


def _segments(a, b, merge, what: str):
    a, b = _rows(a, 3, np.float32), _rows(b, 3, np.float32)
    if len(a) != len(b):
        raise ValueError(f"{what}: {len(a)} start points, {len(b)} end points")
    out = np.zeros(len(a), np.uint8) if merge is None else np.array(merge).astype(bool).astype(np.uint8).reshape(-1)
    if len(out) != len(a):
        raise ValueError(f"{what}: merge has {len(out)} answers for {len(a)} segments")
    return a, b, out


class Mesh:
    """One rt_mesh: a triangle mesh uploaded to a device with its box hierarchy (rt_mesh_create)."""

    def __init__(self, verts, tris, device: int = 0):
        self._lib = load()
        self.verts, self.tris = _rows(verts, 3, np.float32), _rows(tris, 3, np.int32)
        m = C.c_void_p()
        _check(self._lib.rt_mesh_create(device, fptr(self.verts), len(self.verts), _iptr(self.tris), len(self.tris),
                                        C.byref(m)), "rt_mesh_create")
        self.mesh = m

    @classmethod
    def from_obj(cls, path_or_text, device: int = 0) -> "Mesh":
        """A mesh from an OBJ file (a path) or an OBJ text (a str with a line break, or bytes)."""
        return cls(*parse_obj(_obj_text(path_or_text)), device=device)

    def close(self):
        if self.mesh:
            self._lib.rt_mesh_destroy(self.mesh)
            self.mesh = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _c(self, rc, what):
        return _check(rc, what, self.mesh)

    def stats(self) -> dict:
        n, lv, dead, nbytes = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        self._c(self._lib.rt_mesh_stats(self.mesh, C.byref(n), C.byref(lv), C.byref(dead), C.byref(nbytes)), "rt_mesh_stats")
        return {"nodes": n.value, "leaves": lv.value, "dead": dead.value, "bytes": nbytes.value}

    def workspace_bytes(self) -> int:
        return int(self._lib.rt_mesh_workspace_bytes(self.mesh))

    def synchronize(self):
        self._c(self._lib.rt_mesh_synchronize(self.mesh), "rt_mesh_synchronize")

    def trace_rays(self, origins, dirs, thr: float = 1e-4, one_origin: bool = False, merge=None) -> MeshHits:
        """Closest hits of the rays (origins[i], dirs[i]) accepted for t > thr (rt_mesh_trace_rays).
        one_origin: origins is one point.  merge: an earlier answer, (t, normals) or an object with
        those attributes (a Hits of Renderer.trace_rays): replaced only where the mesh is strictly closer."""
        o, d = _rays(origins, dirs, one_origin, "trace_rays")
        h = _hits(len(d), merge)
        self._c(self._lib.rt_mesh_trace_rays(self.mesh, fptr(o), fptr(d), len(d), _flags(one_origin, merge), thr,
                                             fptr(h.t), _iptr(h.prim), fptr(h.normals), fptr(h.uv)), "rt_mesh_trace_rays")
        return h

    def occluded(self, a, b, merge=None) -> np.ndarray:
        """Whether a triangle lies between a[i] and b[i] by rt_occluded's rule (rt_mesh_occluded): bool
        [n].  merge: an earlier answer (bool [n]), OR-ed."""
        a, b, out = _segments(a, b, merge, "occluded")
        self._c(self._lib.rt_mesh_occluded(self.mesh, fptr(a), fptr(b), len(a), RT_MESH_MERGE if merge is not None else 0,
                                           _bptr(out)), "rt_mesh_occluded")
        return out.astype(bool)

    # the same on device memory: integer device pointers (a torch tensor's data_ptr()); stream: an int
    # hipStream_t (Renderer's rt_get_stream, a torch stream's cuda_stream), None = the mesh's own
    def trace_rays_device(self, d_origins: int, d_dirs: int, n: int, thr: float = 1e-4, one_origin: bool = False,
                          merge: bool = False, d_t=None, d_prim=None, d_normals=None, d_uv=None, stream=None):
        flags = _flags(one_origin, True if merge else None)
        self._c(self._lib.rt_mesh_trace_rays_device(self.mesh, _dptr(stream), _dptr(d_origins), _dptr(d_dirs), int(n), flags,
                                                    thr, _dptr(d_t), _dptr(d_prim), _dptr(d_normals), _dptr(d_uv)),
                "rt_mesh_trace_rays_device")

    def occluded_device(self, d_from: int, d_to: int, n: int, merge: bool = False, d_out=None, stream=None):
        self._c(self._lib.rt_mesh_occluded_device(self.mesh, _dptr(stream), _dptr(d_from), _dptr(d_to), int(n),
                                                  RT_MESH_MERGE if merge else 0, _dptr(d_out)), "rt_mesh_occluded_device")


def _mesh_arrays(verts, tris):
    return _rows(verts, 3, np.float32), _rows(tris, 3, np.int32)


def mesh_tri_eval_host(o, d, v0, v1, v2):
    """rt_mesh_tri_eval_host: (t, u, v) of the rule for one ray and one triangle; t = -1: a miss."""
    uv = np.zeros(2, np.float32)
    t = load().rt_mesh_tri_eval_host(_f3(o), _f3(d), _f3(v0), _f3(v1), _f3(v2), fptr(uv))
    return float(t), float(uv[0]), float(uv[1])


def mesh_box_pass_host(o, d, lo, hi) -> bool:
    """rt_mesh_box_pass_host: the rule's box test."""
    return bool(load().rt_mesh_box_pass_host(_f3(o), _f3(d), _f3(lo), _f3(hi)))


def mesh_trace_rays_host(verts, tris, origins, dirs, thr: float = 1e-4, one_origin: bool = False, merge=None) -> MeshHits:
    """rt_mesh_trace_rays_host (host only): Mesh.trace_rays' rule by brute force, its specification."""
    v, f = _mesh_arrays(verts, tris)
    o, d = _rays(origins, dirs, one_origin, "mesh_trace_rays_host")
    h = _hits(len(d), merge)
    _check(load().rt_mesh_trace_rays_host(fptr(v), len(v), _iptr(f), len(f), fptr(o), fptr(d), len(d),
                                          _flags(one_origin, merge), thr, fptr(h.t), _iptr(h.prim), fptr(h.normals),
                                          fptr(h.uv)), "rt_mesh_trace_rays_host")
    return h


def mesh_occluded_host(verts, tris, a, b, merge=None) -> np.ndarray:
    """rt_mesh_occluded_host (host only): Mesh.occluded's rule by brute force, its specification."""
    v, f = _mesh_arrays(verts, tris)
    a, b, out = _segments(a, b, merge, "mesh_occluded_host")
    _check(load().rt_mesh_occluded_host(fptr(v), len(v), _iptr(f), len(f), fptr(a), fptr(b), len(a),
                                        RT_MESH_MERGE if merge is not None else 0, _bptr(out)), "rt_mesh_occluded_host")
    return out.astype(bool)


def mesh_bvh_host(verts, tris) -> dict:
    """rt_mesh_bvh_host (host only): the hierarchy Mesh builds: {"boxes" [n][6] float32 (lo, hi), "links"
    [n][3] int32 (skip, first, count), "leaf_index" [live] int32}."""
    v, f = _mesh_arrays(verts, tris)
    cap = max(2 * len(f), 1)
    boxes, links, index = np.zeros((cap, 6), np.float32), np.zeros((cap, 3), np.int32), np.zeros(max(len(f), 1), np.int32)
    live = C.c_int()
    n = load().rt_mesh_bvh_host(fptr(v), len(v), _iptr(f), len(f), fptr(boxes), _iptr(links), cap, _iptr(index), len(index),
                                C.byref(live))
    if n < 0:
        raise ValueError("rt_mesh_bvh_host rejected the mesh")
    return {"boxes": boxes[:n].copy(), "links": links[:n].copy(), "leaf_index": index[:live.value].copy()}


def _obj_text(path_or_text) -> bytes:
    if isinstance(path_or_text, bytes):
        return path_or_text
    if isinstance(path_or_text, str) and ("\n" in path_or_text or "\r" in path_or_text):
        return path_or_text.encode()
    return Path(path_or_text).read_bytes()


def parse_obj(text):
    """rt_obj_parse: (verts [nv][3] float32, tris [nt][3] int32) of an OBJ text (str or bytes).  A
    malformed line raises ValueError naming it."""
    data = text.encode() if isinstance(text, str) else bytes(text)
    lib = load()
    nv, nt, err = C.c_int(), C.c_int(), C.c_int()
    rc = lib.rt_obj_parse(data, len(data), None, 0, None, 0, C.byref(nv), C.byref(nt), C.byref(err))
    if rc != RT_OK:
        raise ValueError(f"OBJ: line {err.value} is malformed" if rc == RT_E_INVAL and err.value else f"rt_obj_parse: {rc}")
    verts, tris = np.zeros((nv.value, 3), np.float32), np.zeros((nt.value, 3), np.int32)
    _check(lib.rt_obj_parse(data, len(data), fptr(verts), nv.value, _iptr(tris), nt.value, C.byref(nv), C.byref(nt),
                            C.byref(err)), "rt_obj_parse")
    return verts, tris
