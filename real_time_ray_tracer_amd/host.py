"""Host-side mirror of the reference's compute interface, over the C ABI (librtrt.so).

Reference (src/main.cpp):
  class ssbo_data (49-85)            -> SSBO / header_size / ssbo_size
  loadShapeBuffer (395-469)          -> Header.pack_sphere / pack_plane / pack_rectangle
  fill_rand_buffer (535-539)         -> Header.fill_rand_buffer (seeded)
  moving_light (541-551)             -> Header.moving_light
  camera basis in render (772-779)   -> Header.camera_basis
  compute (553-578)                  -> Renderer.compute / Renderer.dispatch
  compute_one_shader (580-620)       -> Renderer.compute_one_shader
  compute_two_shaders (622-671)      -> Renderer.compute_two_shaders
Programs keep the reference's names: AOP_COMPUTE, AOP_POSTPROCESSING, AO_COMPUTE,
P_COMPUTE, H_COMPUTE.  Errors raise RtError (the reference exits on shader compile errors
and has no dispatch errors; here every bad argument is reported).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import RtError, fptr

AOP_COMPUTE = _lib.RT_PROG_AOP_COMPUTE
AOP_POSTPROCESSING = _lib.RT_PROG_AOP_POSTPROCESSING
AO_COMPUTE = _lib.RT_PROG_AO_COMPUTE
P_COMPUTE = _lib.RT_PROG_P_COMPUTE
H_COMPUTE = _lib.RT_PROG_H_COMPUTE
PROGRAM_NAMES = {AOP_COMPUTE: "aop_compute", AOP_POSTPROCESSING: "aop_postprocessing",
                 AO_COMPUTE: "ao_compute", P_COMPUTE: "p_compute", H_COMPUTE: "h_compute"}

ASPECT_RATIO = 1.333333            # src/main.cpp:39
FULLSCREEN_ASPECT_RATIO = 1.777777  # src/main.cpp:40


def header_floats(S: int, AA: int) -> int:
    """floats in the SSBO prefix: 7 vec4 + S*5 vec4 + 2*AA vec4 (include/rt/layout.h)."""
    return 4 * (7 + 5 * S + 2 * AA)


def ssbo_floats(S: int, AA: int, W: int, H: int, F: int = 8) -> int:
    return header_floats(S, AA) + 3 * 4 * F * W * H


def aspect_for(width: int, height: int) -> float:
    return ASPECT_RATIO if width * 3 == height * 4 else FULLSCREEN_ASPECT_RATIO


def _check(rc: int, what: str, ctx=None) -> int:
    if rc < 0:
        hip = _lib.load().rt_last_hip_error(ctx) if ctx else 0
        raise RtError(rc, what, hip)
    return rc


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


class Header:
    """The SSBO prefix (header + shapes + rand_buffer) as a float32 array; host-only helpers."""

    def __init__(self, num_shapes: int, spp: int, data: np.ndarray | None = None):
        self.S, self.AA = int(num_shapes), int(spp)
        n = header_floats(self.S, self.AA)
        self.data = np.zeros(n, np.float32) if data is None else np.ascontiguousarray(data, np.float32)
        assert self.data.size == n
        self._lib = _lib.load()

    # views
    def vec4(self, i: int) -> np.ndarray:
        return self.data[4 * i:4 * i + 4]

    @property
    def shapes(self) -> np.ndarray:
        return self.data[28:28 + 20 * self.S].reshape(self.S, 5, 4)

    @property
    def rand_buffer(self) -> np.ndarray:
        o = 28 + 20 * self.S
        return self.data[o:o + 8 * self.AA].reshape(2 * self.AA, 4)

    @property
    def num_objects(self) -> int:
        return int(self.data[2])

    def _p(self):
        return fptr(self.data)

    # loadShapeBuffer entries
    def pack_sphere(self, i, center, radius, color, reflectivity=1.0, emissive=False):
        _check(self._lib.rt_pack_sphere(self._p(), self.S, i, _f3(center), radius, _f3(color),
                                        reflectivity, int(emissive)), "rt_pack_sphere")

    def pack_plane(self, i, normal, dist, color, reflectivity=1.0, emissive=False):
        _check(self._lib.rt_pack_plane(self._p(), self.S, i, _f3(normal), dist, _f3(color),
                                       reflectivity, int(emissive)), "rt_pack_plane")

    def pack_rectangle(self, i, llc, right, up, color, reflectivity=1.0, emissive=False):
        _check(self._lib.rt_pack_rectangle(self._p(), self.S, i, _f3(llc), _f3(right), _f3(up), _f3(color),
                                           reflectivity, int(emissive)), "rt_pack_rectangle")

    def camera_basis(self, location, up, look_towards, aspect):
        _check(self._lib.rt_camera_basis(self._p(), _f3(location), _f3(up), _f3(look_towards), aspect),
               "rt_camera_basis")

    def set_mode(self, frame: int, num_objects: int):
        _check(self._lib.rt_set_mode(self._p(), frame, num_objects), "rt_set_mode")

    def fill_rand_buffer(self, seed: int):
        _check(self._lib.rt_fill_rand_buffer(self._p(), self.S, self.AA, seed), "rt_fill_rand_buffer")

    def moving_light(self, light_movement: bool = False):
        _check(self._lib.rt_moving_light(self._p(), int(light_movement)), "rt_moving_light")

    @classmethod
    def synthetic(cls, num_objects: int, spp: int, seed: int, aspect: float, num_shapes: int | None = None):
        h = cls(num_shapes if num_shapes is not None else num_objects, spp)
        _check(h._lib.rt_scenegen(h._p(), h.S, num_objects, spp, seed, aspect), "rt_scenegen")
        return h

    @classmethod
    def builtin(cls, which: int, spp: int, aspect: float = ASPECT_RATIO, num_shapes: int = 10):
        h = cls(num_shapes, spp)
        _check(h._lib.rt_init_scene(h._p(), h.S, spp, which, aspect), "rt_init_scene")
        return h

    def copy(self) -> "Header":
        return Header(self.S, self.AA, self.data.copy())

    def cluster_table(self, cap: int = 64):
        """The bounce-ray clusters an upload of this header builds (rt_cluster_table, host only):
        (clusters [n][4] float32 (centre, R), always-tested mask [4] uint64, member masks [n][4] uint64)."""
        cfg = _lib.rt_config(1, 1, self.S, self.AA, 1, 1, 0, 0)
        clusters = np.zeros((cap, 4), np.float32)
        masks = np.zeros((1 + cap, 4), np.uint64)
        n = self._lib.rt_cluster_table(C.byref(cfg), self.data.ctypes.data_as(C.c_void_p), self.data.nbytes,
                                       fptr(clusters), masks.ctypes.data_as(C.POINTER(C.c_uint64)), cap)
        if n < 0:
            raise ValueError("rt_cluster_table rejected the header or the capacity")
        return clusters[:n].copy(), masks[0].copy(), masks[1:1 + n].copy()


class SSBO:
    """A whole ssbo_data-layout host buffer (src/main.cpp:49-85) for the host-buffer path."""

    def __init__(self, header: Header, width: int, height: int, num_frames: int = 8):
        self.S, self.AA, self.W, self.H, self.F = header.S, header.AA, width, height, num_frames
        self.data = np.zeros(ssbo_floats(self.S, self.AA, width, height, num_frames), np.float32)
        self.data[:header.data.size] = header.data
        self.hn = header.data.size

    @property
    def header(self) -> Header:
        return Header(self.S, self.AA, self.data[:self.hn].copy())

    def set_header(self, header: Header):
        self.data[:self.hn] = header.data

    def _g(self, k):
        n = self.F * self.W * self.H * 4
        o = self.hn + k * n
        return self.data[o:o + n].reshape(self.F, self.W, self.H, 4)

    pixels = property(lambda self: self._g(0))
    normals = property(lambda self: self._g(1))
    depth = property(lambda self: self._g(2))


@dataclass
class GBuffer:
    pixels: np.ndarray   # [F][W][R][4]  reference layout
    normals: np.ndarray
    depth: np.ndarray
    image: np.ndarray    # [R][W][4]


@dataclass
class Hits:
    """Closest hits of n rays: t [n] float32 (-1: a miss), ind [n] int32 (-1: a miss), normals [n][3]
    float32 (zeros for a miss); dirs [n][3]: the rays used, for pixel rays (else None)."""
    t: np.ndarray
    ind: np.ndarray
    normals: np.ndarray
    dirs: np.ndarray | None = None

    @classmethod
    def empty(cls, n: int, dirs: bool = False) -> "Hits":
        return cls(np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros((n, 3), np.float32),
                   np.zeros((n, 3), np.float32) if dirs else None)


def _rows(a, w: int, dtype) -> np.ndarray:
    """a as a C-contiguous [n][w] array of dtype (integers are neither truncated from floats nor
    wrapped from beyond int32)."""
    a = np.asarray(a)
    if dtype == np.int32 and a.size:
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("pixel coordinates must be integers")
        if a.min() < -2**31 or a.max() > 2**31 - 1:
            raise ValueError("pixel coordinates must fit in int32")
    if a.size % w:
        raise ValueError(f"need rows of {w} values, got shape {a.shape}")
    return np.ascontiguousarray(a.reshape(-1, w), dtype)


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _dptr(p):
    return C.c_void_p(int(p)) if p else None


class Renderer:
    """One rt_ctx: a device, a frame (or a row strip of it), a resident g-buffer ring."""

    def __init__(self, width: int, height: int, num_shapes: int, spp: int, num_frames: int = 8,
                 max_depth: int = 20, device: int = 0, rows: tuple[int, int] | None = None):
        self._lib = _lib.load()
        r0, r1 = rows if rows is not None else (0, height)
        self.cfg = _lib.rt_config(width, height, num_shapes, spp, num_frames, max_depth, r0, r1)
        self.W, self.H, self.S, self.AA, self.F, self.D = width, height, num_shapes, spp, num_frames, max_depth
        self.row_begin, self.row_end = r0, r1
        self.R = r1 - r0
        ctx = C.c_void_p()
        _check(self._lib.rt_create(device, C.byref(self.cfg), C.byref(ctx)), "rt_create")
        self.ctx = ctx

    # lifetime
    def close(self):
        if self.ctx:
            self._lib.rt_destroy(self.ctx)
            self.ctx = None

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
        return _check(rc, what, self.ctx)

    # streams
    def set_stream(self, stream):
        """Order the context's work on `stream`: a torch.cuda.Stream or an int hipStream_t
        (0 = the NULL stream, which is torch's default stream); None = the context's own stream."""
        if stream is None:
            self._c(self._lib.rt_use_own_stream(self.ctx), "rt_use_own_stream")
            return
        ptr = int(getattr(stream, "cuda_stream", stream))
        self._c(self._lib.rt_set_stream(self.ctx, C.c_void_p(ptr)), "rt_set_stream")

    def enable_pipelining(self, on: bool = True, output_stream=None):
        """Pipelined mode 1: frame k's post-process runs on `output_stream` (a torch.cuda.Stream
        or an int hipStream_t; None = a stream of the context's own) while frame k+1's AO pass
        runs on the main stream.  Bit-identical results; consumers of the image order their
        work on the output stream (or synchronize)."""
        ptr = None if output_stream is None else int(getattr(output_stream, "cuda_stream", output_stream))
        self._c(self._lib.rt_enable_pipelining(self.ctx, int(bool(on)), C.c_void_p(ptr) if ptr is not None else None),
                "rt_enable_pipelining")

    def synchronize(self):
        self._c(self._lib.rt_synchronize(self.ctx), "rt_synchronize")

    # device-resident path
    def upload_header(self, header: Header):
        assert header.S == self.S and header.AA == self.AA
        self._c(self._lib.rt_upload_header(self.ctx, header.data.ctypes.data_as(C.c_void_p),
                                           header.data.nbytes), "rt_upload_header")

    def upload_rand_buffer(self, rb: np.ndarray):
        rb = np.ascontiguousarray(rb, np.float32).reshape(-1)
        self._c(self._lib.rt_upload_rand_buffer(self.ctx, fptr(rb), rb.size // 4), "rt_upload_rand_buffer")

    def run_program(self, program: int, frame: int):
        self._c(self._lib.rt_run_program(self.ctx, program, frame), f"rt_run_program({program})")

    def dispatch(self, mode: int, frame: int) -> int:
        return self._c(self._lib.rt_dispatch(self.ctx, mode, frame), f"rt_dispatch(mode {mode})")

    def compute_frames(self, header: Header, mode: int, frame: int, n: int, rand_seed: int = 7000,
                       light_movement: bool = False) -> int:
        """n compute() rounds with the per-frame host updates done in C++ (rt_compute_frames):
        fill_rand_buffer(rand_seed + k) or moving_light, set_mode, upload, dispatch.  `header`
        is updated in place as the frame loop leaves it.  Returns the next frame slot."""
        return self._c(self._lib.rt_compute_frames(self.ctx, header._p(), mode, frame, n, rand_seed,
                                                   int(bool(light_movement))), "rt_compute_frames")

    def set_frame_batch(self, max_frames: int):
        """compute_frames' most frames per launch (modes 2-4); 1 (the default) = one launch and one
        image write per frame, the reference's dispatch shape; > 1 = multi-frame launches, the image
        by each launch's last frame (rt_set_frame_batch)."""
        self._c(self._lib.rt_set_frame_batch(self.ctx, int(max_frames)), "rt_set_frame_batch")

    def set_tile_schedule(self, on: bool):
        """Mode 4's longest-first tile order (rt_set_tile_schedule; on by default)."""
        self._c(self._lib.rt_set_tile_schedule(self.ctx, int(bool(on))), "rt_set_tile_schedule")

    def set_phong_gbuffer(self, on: bool):
        """Modes 3 and 4 also store the primary hit's normal and depth in the frame's ring slot, as
        the AO modes do, and trace a strip's halo rows for them (rt_set_phong_gbuffer; off by
        default, as in the reference).  The colours do not depend on it."""
        self._c(self._lib.rt_set_phong_gbuffer(self.ctx, int(bool(on))), "rt_set_phong_gbuffer")

    def set_rectangles(self, on: bool):
        """Intersect rectangles (shape id 3) in every mode and in the ray queries, by the rule of
        include/rt/abi.h "Rectangles" (rt_set_rectangles; off by default, as the reference never hits
        them).  Takes effect at the next launch or query."""
        self._c(self._lib.rt_set_rectangles(self.ctx, int(bool(on))), "rt_set_rectangles")

    @property
    def rectangles(self) -> bool:
        """Whether rectangles are intersected (rt_rectangles)."""
        return bool(self._c(self._lib.rt_rectangles(self.ctx), "rt_rectangles"))

    def set_query_tree(self, on: bool):
        """The ray queries over a tree of bounding balls around the spheres (rt_set_query_tree,
        include/rt/abi.h "Query tree"; off by default).  The answers are the linear scan's, bit for bit."""
        self._c(self._lib.rt_set_query_tree(self.ctx, int(bool(on))), "rt_set_query_tree")

    @property
    def query_tree(self) -> bool:
        """Whether the ray queries walk the tree (rt_query_tree)."""
        return bool(self._c(self._lib.rt_query_tree(self.ctx), "rt_query_tree"))

    def query_tree_stats(self) -> dict:
        """{"nodes", "leaves", "always", "bytes"} of the tree of the scene in effect and its device
        buffer (rt_query_tree_stats); nodes 0: the scene has no tree, the queries scan."""
        n, lv, a, b = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
        self._c(self._lib.rt_query_tree_stats(self.ctx, C.byref(n), C.byref(lv), C.byref(a), C.byref(b)),
                "rt_query_tree_stats")
        return {"nodes": n.value, "leaves": lv.value, "always": a.value, "bytes": b.value}

    @property
    def phong_gbuffer(self) -> bool:
        """Whether modes 3 and 4 write normals and depth (rt_phong_gbuffer)."""
        return bool(self._c(self._lib.rt_phong_gbuffer(self.ctx), "rt_phong_gbuffer"))

    def tile_schedule_state(self) -> int:
        """0 off, 1 on (row order so far), 2 a longest-first order in use (rt_tile_schedule_state)."""
        return self._c(self._lib.rt_tile_schedule_state(self.ctx), "rt_tile_schedule_state")

    def tile_schedule_orders(self) -> int:
        """Orders taken up so far (rt_tile_schedule_orders)."""
        return self._c(self._lib.rt_tile_schedule_orders(self.ctx), "rt_tile_schedule_orders")

    def set_cull_cache(self, on: bool):
        """The AO pools' primary-ray cull masks kept while camera and scene hold (rt_set_cull_cache;
        on by default).  Off: every launch culls in the kernel; results are bit-identical."""
        self._c(self._lib.rt_set_cull_cache(self.ctx, int(bool(on))), "rt_set_cull_cache")

    def cull_cache_stats(self) -> dict:
        """{"fills", "cached_launches", "table_bytes"} since the context was created (rt_cull_cache_stats)."""
        f, n, b = C.c_longlong(), C.c_longlong(), C.c_size_t()
        self._c(self._lib.rt_cull_cache_stats(self.ctx, C.byref(f), C.byref(n), C.byref(b)), "rt_cull_cache_stats")
        return {"fills": f.value, "cached_launches": n.value, "table_bytes": b.value}

    def cull_cache_frame_bytes(self) -> int:
        """Bytes of the pools' sort frames kept with the masks (rt_cull_cache_frame_bytes); 0: masks only."""
        return int(self._lib.rt_cull_cache_frame_bytes(self.ctx))

    def debug_cull_cache_cap(self, nbytes: int):
        """Test hook (rt_debug_cull_cache_cap): this context's cap on the cull cache, before its first fill."""
        self._c(self._lib.rt_debug_cull_cache_cap(self.ctx, int(nbytes)), "rt_debug_cull_cache_cap")

    def set_pool_list(self, on: bool):
        """The cull cache's pool list (rt_set_pool_list; on by default): cached AO launches run one workgroup
        per non-sky pool and one per 64 sky pools.  Off: one per pool; results are bit-identical."""
        self._c(self._lib.rt_set_pool_list(self.ctx, int(bool(on))), "rt_set_pool_list")

    def pool_list_stats(self) -> dict:
        """{"builds", "list_launches", "n_nonsky", "n_sky", "bytes"} (rt_pool_list_stats); the counts are -1
        while no list's counts have landed."""
        b, n, ns, sk, by = C.c_longlong(), C.c_longlong(), C.c_int(), C.c_int(), C.c_size_t()
        self._c(self._lib.rt_pool_list_stats(self.ctx, C.byref(b), C.byref(n), C.byref(ns), C.byref(sk), C.byref(by)),
                "rt_pool_list_stats")
        return {"builds": b.value, "list_launches": n.value, "n_nonsky": ns.value, "n_sky": sk.value, "bytes": by.value}

    def debug_pool_list(self) -> dict:
        """Test hook (rt_debug_pool_list_read), after waiting for the device: {"rows": int32 [n_nonsky][4] of
        (pb, xf, yf, np), "sky": uint32 [n_sky] in list order, "masks": uint64 [pools][words]} of the current key."""
        out = {}
        for what, name, dt in ((0, "rows", np.int32), (1, "sky", np.uint32), (2, "masks", np.uint64)):
            need = int(self._lib.rt_debug_pool_list_read(self.ctx, what, None, 0))
            if need < 0:
                self._c(need, "rt_debug_pool_list_read")
            a = np.zeros(need // np.dtype(dt).itemsize, dt)
            if need:
                self._c(min(0, int(self._lib.rt_debug_pool_list_read(self.ctx, what, a.ctypes.data_as(C.c_void_p), need))),
                        "rt_debug_pool_list_read")
            out[name] = a
        out["rows"] = out["rows"].reshape(-1, 4)
        out["sky"] = out["sky"][::-1].copy()  # stored downwards from the rows' end
        return out

    def set_launch_log(self, on: bool):
        """Test hook (rt_debug_launch_log): record the form of every kernel this context launches; off empties the log."""
        self._c(self._lib.rt_debug_launch_log(self.ctx, int(bool(on))), "rt_debug_launch_log")

    def launch_log(self, reset: bool = False) -> list:
        """The forms launched since the log was switched on or last reset, in launch order
        (rt_debug_launch_log_read), e.g. "ao_batch_kernel<AoProd<16, 20, 70u>>"."""
        need = self._lib.rt_debug_launch_log_read(self.ctx, None, 0, 0)
        if need < 0:
            self._c(int(need), "rt_debug_launch_log_read")
        buf = C.create_string_buffer(int(need))
        self._c(min(0, int(self._lib.rt_debug_launch_log_read(self.ctx, buf, int(need), int(bool(reset))))),
                "rt_debug_launch_log_read")
        return buf.value.decode().splitlines()

    def download(self, pixels=True, normals=True, depth=True, image=True) -> GBuffer:
        shp = (self.F, self.W, self.R, 4)
        p = np.empty(shp, np.float32) if pixels else None
        n = np.empty(shp, np.float32) if normals else None
        d = np.empty(shp, np.float32) if depth else None
        im = np.empty((self.R, self.W, 4), np.float32) if image else None
        self._c(self._lib.rt_download(self.ctx, fptr(p), fptr(n), fptr(d), fptr(im)), "rt_download")
        return GBuffer(p, n, d, im)

    def download_rect(self, x0: int, x1: int, y0: int, y1: int, pixels=True, normals=True, depth=True,
                      image=True) -> GBuffer:
        """The window [x0, x1) x frame rows [y0, y1): g-buffer [F][w][h][4], image [h][w][4]."""
        shp = (self.F, x1 - x0, y1 - y0, 4)
        p = np.empty(shp, np.float32) if pixels else None
        n = np.empty(shp, np.float32) if normals else None
        d = np.empty(shp, np.float32) if depth else None
        im = np.empty((y1 - y0, x1 - x0, 4), np.float32) if image else None
        self._c(self._lib.rt_download_rect(self.ctx, x0, x1, y0, y1, fptr(p), fptr(n), fptr(d), fptr(im)),
                "rt_download_rect")
        return GBuffer(p, n, d, im)

    def image(self) -> np.ndarray:
        return self.download(False, False, False, True).image

    def upload_gbuffer(self, pixels=None, normals=None, depth=None):
        conv = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (pixels, normals, depth)]
        self._c(self._lib.rt_upload_gbuffer(self.ctx, *[fptr(a) for a in conv]), "rt_upload_gbuffer")

    def image_device_ptr(self) -> int:
        return self._lib.rt_image_device_ptr(self.ctx) or 0

    def bind_image(self, device_ptr: int | None):
        self._c(self._lib.rt_bind_image(self.ctx, C.c_void_p(device_ptr) if device_ptr else None),
                "rt_bind_image")

    # ray queries on the scene in effect (include/rt/abi.h "Ray queries")
    def trace_rays(self, origins, dirs, thr: float = 1e-4) -> "Hits":
        """Closest hits of the rays (origins[i], dirs[i]) ([n][3] each; dirs used as given, not
        normalised) accepted for t > thr (rt_trace_rays): Hits(t, ind, normals), -1 / -1 / zeros for a miss."""
        o, d = _rows(origins, 3, np.float32), _rows(dirs, 3, np.float32)
        if len(o) != len(d):
            raise ValueError(f"trace_rays: {len(o)} origins, {len(d)} directions")
        h = Hits.empty(len(o))
        self._c(self._lib.rt_trace_rays(self.ctx, fptr(o), fptr(d), len(o), thr, fptr(h.t), _iptr(h.ind),
                                        fptr(h.normals)), "rt_trace_rays")
        return h

    def trace_pixels(self, xy, thr: float = 0.0) -> "Hits":
        """Closest hits of the camera's rays through the pixels xy ([n][2] ints, frame coordinates,
        row 0 = the bottom row; rt_trace_pixels): Hits(t, ind, normals, dirs), dirs the rays used.
        thr 0: what a mode-3 frame shows at the pixel; 0.001: mode 4; 0.0001: the AO modes."""
        p = _rows(xy, 2, np.int32)
        h = Hits.empty(len(p), dirs=True)
        self._c(self._lib.rt_trace_pixels(self.ctx, _iptr(p), len(p), thr, fptr(h.t), _iptr(h.ind), fptr(h.normals),
                                          fptr(h.dirs)), "rt_trace_pixels")
        return h

    def occluded(self, a, b) -> np.ndarray:
        """Whether something lies between a[i] and b[i] as a shadow ray from a[i] to a light at b[i]
        sees it (rt_occluded): bool [n]."""
        a, b = _rows(a, 3, np.float32), _rows(b, 3, np.float32)
        if len(a) != len(b):
            raise ValueError(f"occluded: {len(a)} start points, {len(b)} end points")
        out = np.zeros(len(a), np.uint8)
        self._c(self._lib.rt_occluded(self.ctx, fptr(a), fptr(b), len(a), out.ctypes.data_as(C.c_void_p)),
                "rt_occluded")
        return out.astype(bool)

    # the same on device memory: integer device pointers (a torch tensor's data_ptr()), 0 / None =
    # that output is not wanted; enqueued on the context's stream, no wait (rt_*_device)
    def trace_rays_device(self, d_origins: int, d_dirs: int, n: int, thr: float = 1e-4, d_t=None, d_ind=None,
                          d_normals=None):
        self._c(self._lib.rt_trace_rays_device(self.ctx, _dptr(d_origins), _dptr(d_dirs), int(n), thr, _dptr(d_t),
                                               _dptr(d_ind), _dptr(d_normals)), "rt_trace_rays_device")

    def trace_pixels_device(self, d_xy: int, n: int, thr: float = 0.0, d_t=None, d_ind=None, d_normals=None,
                            d_dirs=None):
        self._c(self._lib.rt_trace_pixels_device(self.ctx, _dptr(d_xy), int(n), thr, _dptr(d_t), _dptr(d_ind),
                                                 _dptr(d_normals), _dptr(d_dirs)), "rt_trace_pixels_device")

    def occluded_device(self, d_from: int, d_to: int, n: int, d_out=None):
        self._c(self._lib.rt_occluded_device(self.ctx, _dptr(d_from), _dptr(d_to), int(n), _dptr(d_out)),
                "rt_occluded_device")

    def query_workspace_bytes(self) -> int:
        """Bytes of the host-pointer queries' device workspace (0 until the first such query)."""
        return int(self._lib.rt_query_workspace_bytes(self.ctx))

    # 8-bit display output (the blit, src/main.cpp:783-797)
    def present(self, top_down: bool = True):
        """Enqueue the conversion of the current image to RGBA8 (rt_present) behind the launch that
        wrote it; returns without waiting.  top_down: output row 0 is the image's top row."""
        self._c(self._lib.rt_present(self.ctx, int(bool(top_down))), "rt_present")

    def image8(self, top_down: bool = True) -> np.ndarray:
        """present + wait + copy (rt_download_rgba8): uint8 [R][W][4], equal to
        quantize_rgba8(self.image(), top_down)."""
        out = np.empty((self.R, self.W, 4), np.uint8)
        self._c(self._lib.rt_download_rgba8(self.ctx, int(bool(top_down)), out.ctypes.data_as(C.c_void_p)),
                "rt_download_rgba8")
        return out

    def present_device_ptr(self) -> int:
        """Where the last present wrote ([R][W] RGBA8 on the device); 0 before the first present."""
        return self._lib.rt_present_device_ptr(self.ctx) or 0

    def bind_present(self, device_ptr: int | None):
        """Later presents write into a caller-owned device buffer of R*W*4 bytes (None: the context's own)."""
        self._c(self._lib.rt_bind_present(self.ctx, C.c_void_p(device_ptr) if device_ptr else None),
                "rt_bind_present")

    # 8-bit display output at window size (the blit's GL_LINEAR scaling, src/main.cpp:381-388, 783-797)
    def present_scaled(self, out_w: int, out_h: int, top_down: bool = True):
        """Enqueue the bilinear blit of the current image into an [out_h][out_w] RGBA8 buffer
        (rt_present_scaled) behind the launch that wrote it; returns without waiting.  Whole-frame
        contexts only."""
        self._c(self._lib.rt_present_scaled(self.ctx, int(out_w), int(out_h), int(bool(top_down))),
                "rt_present_scaled")

    def image8_scaled(self, out_w: int, out_h: int, top_down: bool = True) -> np.ndarray:
        """present_scaled + wait + copy (rt_download_rgba8_scaled): uint8 [out_h][out_w][4], equal to
        resample_rgba8(self.image(), out_w, out_h, top_down)."""
        out = np.empty((max(0, int(out_h)), max(0, int(out_w)), 4), np.uint8)
        self._c(self._lib.rt_download_rgba8_scaled(self.ctx, int(out_w), int(out_h), int(bool(top_down)),
                                                   out.ctypes.data_as(C.c_void_p)), "rt_download_rgba8_scaled")
        return out

    def present_scaled_device_ptr(self) -> int:
        """Where the last scaled present wrote (RGBA8 on the device); 0 before the first."""
        return self._lib.rt_present_scaled_device_ptr(self.ctx) or 0

    def present_scaled_size(self) -> tuple[int, int]:
        """(out_w, out_h) of the last scaled present (rt_present_scaled_size)."""
        w, h = C.c_int(), C.c_int()
        self._c(self._lib.rt_present_scaled_size(self.ctx, C.byref(w), C.byref(h)), "rt_present_scaled_size")
        return w.value, h.value

    def bind_present_scaled(self, device_ptr: int | None):
        """Later scaled presents write into a caller-owned device buffer of out_w*out_h*4 bytes for
        every size presented (None: the context's own)."""
        self._c(self._lib.rt_bind_present_scaled(self.ctx, C.c_void_p(device_ptr) if device_ptr else None),
                "rt_bind_present_scaled")

    # host-buffer parity path (the reference's call shape)
    def compute_one_shader(self, ssbo: SSBO, frame_num: int, program: int, image: np.ndarray | None = None) -> int:
        return self._c(self._lib.rt_compute_one_shader(self.ctx, ssbo.data.ctypes.data_as(C.c_void_p), frame_num,
                                                       program, fptr(image)), "rt_compute_one_shader")

    def compute_two_shaders(self, ssbo: SSBO, frame_num: int, program1: int, program2: int,
                            image: np.ndarray | None = None) -> int:
        return self._c(self._lib.rt_compute_two_shaders(self.ctx, ssbo.data.ctypes.data_as(C.c_void_p), frame_num,
                                                        program1, program2, fptr(image)),
                       "rt_compute_two_shaders")

    # instrumentation
    def enable_timing(self, on: bool = True):
        self._c(self._lib.rt_enable_timing(self.ctx, int(on)), "rt_enable_timing")

    def kernel_stats(self, program: int) -> tuple[int, float]:
        n, ms = C.c_int(), C.c_double()
        self._c(self._lib.rt_kernel_stats(self.ctx, program, C.byref(n), C.byref(ms)), "rt_kernel_stats")
        return n.value, ms.value

    def reset_stats(self):
        self._c(self._lib.rt_reset_stats(self.ctx), "rt_reset_stats")

    def debug_fail_next_event_query(self, hip_error: int):
        """Test hook (rt_debug_fail_next_event_query): the next staging-buffer query reports hip_error."""
        self._c(self._lib.rt_debug_fail_next_event_query(self.ctx, int(hip_error)), "rt_debug_fail_next_event_query")

    def host_stats(self) -> tuple[float, int]:
        """(ms, count) of host waits for a free staging buffer since reset_stats (back-pressure)."""
        ms, n = C.c_double(), C.c_longlong()
        self._c(self._lib.rt_host_stats(self.ctx, C.byref(ms), C.byref(n)), "rt_host_stats")
        return ms.value, n.value

    def enable_counters(self, totals: bool = True, rows: bool = False):
        self._c(self._lib.rt_enable_counters(self.ctx, int(totals) | (2 if rows else 0)), "rt_enable_counters")

    def read_counters(self, reset: bool = True) -> dict:
        out = (C.c_uint64 * 8)()
        self._c(self._lib.rt_read_counters(self.ctx, out, int(reset)), "rt_read_counters")
        return {"samples": out[0], "segments": out[1], "shadow_rays": out[2], "tests": out[3],
                "executed_lane_tests": out[4], "filtered_pixels": out[5], "history_read": out[6],
                "history_accepted": out[7]}

    def read_row_counters(self, reset: bool = True) -> np.ndarray:
        out = np.zeros(self.R, np.uint64)
        self._c(self._lib.rt_read_row_counters(self.ctx, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(reset)),
                "rt_read_row_counters")
        return out

    def selftest_math(self, fn: int, inputs: np.ndarray, n: int) -> np.ndarray:
        out_w = {_lib.RT_MATH_NORMALIZE: 3, _lib.RT_MATH_SHADOW: 5, _lib.RT_MATH_SIN_TABLE: 2,
                 _lib.RT_MATH_CULL_CAMERA: 7, _lib.RT_MATH_CULL_PLANE: 2, _lib.RT_MATH_CULL_BOUNCE: 320,
                 _lib.RT_MATH_CULL_CLUSTER: 3, _lib.RT_MATH_CULL_SHADOW: 128, _lib.RT_MATH_CULL_TREE: 3}.get(fn, 1)
        in_w = {_lib.RT_MATH_RANDOM: 2, _lib.RT_MATH_DIV: 2, _lib.RT_MATH_NORMALIZE: 3, _lib.RT_MATH_SPHERE: 10,
                _lib.RT_MATH_SHADOW: 4, _lib.RT_MATH_CULL_CAMERA: 24, _lib.RT_MATH_CULL_PLANE: 28,
                _lib.RT_MATH_CULL_BOUNCE: 452, _lib.RT_MATH_CULL_CLUSTER: 14, _lib.RT_MATH_CULL_SHADOW: 263,
                _lib.RT_MATH_CULL_TREE: 14}.get(fn, 1)
        inp = np.ascontiguousarray(inputs, np.float32).reshape(-1)
        sweep = fn in (_lib.RT_MATH_SQRT_SWEEP, _lib.RT_MATH_RCP_SWEEP, _lib.RT_MATH_SQRT_TAIL_SWEEP,
                       _lib.RT_MATH_SIN_RANGE, _lib.RT_MATH_SIN_TABLE)
        if inp.size < (1 if sweep else n * in_w):
            raise ValueError(f"selftest_math: {inp.size} input floats for n = {n} (need {1 if sweep else n * in_w})")
        out = np.empty(n * out_w, np.float32)
        self._c(self._lib.rt_selftest_math(self.ctx, fn, fptr(inp), fptr(out), n), "rt_selftest_math")
        return out


class StripGroup:
    """Row strips of one frame on several devices in one process (rt_group_*, the C-ABI
    counterpart of dist.py's one-process-per-GPU path): strip i = rows [bounds[i], bounds[i+1])
    on devices[i]; the image strips are assembled into one [H][W] frame on devices[0]."""

    def __init__(self, width: int, height: int, num_shapes: int, spp: int, devices, bounds=None,
                 num_frames: int = 8, max_depth: int = 20):
        self._lib = _lib.load()
        self.W, self.H, self.S, self.AA, self.F = width, height, num_shapes, spp, num_frames
        devs = [int(d) for d in devices]
        self.n = len(devs)
        cfg = _lib.rt_config(width, height, num_shapes, spp, num_frames, max_depth, 0, 0)
        dv = (C.c_int * self.n)(*devs)
        bd = None if bounds is None else (C.c_int * (self.n + 1))(*[int(b) for b in bounds])
        g = C.c_void_p()
        _check(self._lib.rt_group_create(self.n, dv, C.byref(cfg), bd, C.byref(g)), "rt_group_create")
        self.g = g

    def close(self):
        if self.g:
            self._lib.rt_group_destroy(self.g)
            self.g = None

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
        if rc < 0:
            raise RtError(rc, what, self._lib.rt_group_last_hip_error(self.g) if self.g else 0)
        return rc

    @property
    def bounds(self) -> list[int]:
        b = (C.c_int * (self.n + 1))()
        self._c(self._lib.rt_group_bounds(self.g, b), "rt_group_bounds")
        return list(b)

    def set_bounds(self, bounds):
        self._c(self._lib.rt_group_set_bounds(self.g, (C.c_int * (self.n + 1))(*[int(b) for b in bounds])),
                "rt_group_set_bounds")

    def strip_copies(self, i: int) -> bool:
        """Whether strip i's image is copied into the frame (another device, or forced)."""
        return bool(self._c(self._lib.rt_group_strip_copies(self.g, i), "rt_group_strip_copies"))

    def set_plan(self, bounds, root_strip: int):
        """rt_group_set_plan: new bounds and root strip (the strip rendered on devices[0])."""
        b = (C.c_int * (self.n + 1))(*[int(x) for x in bounds])
        self._c(self._lib.rt_group_set_plan(self.g, b, int(root_strip)), "rt_group_set_plan")

    def root_strip(self) -> int:
        return self._c(self._lib.rt_group_root_strip(self.g), "rt_group_root_strip")

    def strip_device(self, i: int) -> int:
        return self._c(self._lib.rt_group_strip_device(self.g, i), "rt_group_strip_device")

    def set_link_model(self, link_gbps: float, ingest_gbps: float):
        self._c(self._lib.rt_group_set_link_model(self.g, float(link_gbps), float(ingest_gbps)),
                "rt_group_set_link_model")

    def link_model(self) -> tuple[float, float]:
        a, b = C.c_double(), C.c_double()
        self._c(self._lib.rt_group_link_model(self.g, C.byref(a), C.byref(b)), "rt_group_link_model")
        return a.value, b.value

    def force_copies(self, on: bool = True):
        """Test hook: every strip but strip 0 renders into its own image and copies it into the
        frame, as strips on other devices do (the copy path, exercised on one GPU)."""
        self._c(self._lib.rt_group_force_copies(self.g, int(bool(on))), "rt_group_force_copies")

    def strip_ctx(self, i: int):
        return self._lib.rt_group_strip(self.g, i)

    def strip_kernel_stats(self, i: int, program: int) -> tuple[int, float]:
        n, ms = C.c_int(), C.c_double()
        _check(self._lib.rt_kernel_stats(self.strip_ctx(i), program, C.byref(n), C.byref(ms)), "rt_kernel_stats")
        return n.value, ms.value

    def enable_pipelining(self, on: bool = True):
        self._c(self._lib.rt_group_enable_pipelining(self.g, int(bool(on))), "rt_group_enable_pipelining")

    def set_phong_gbuffer(self, on: bool):
        """Renderer.set_phong_gbuffer on every strip (rt_group_set_phong_gbuffer); kept when the
        strips are re-created by set_bounds, set_plan or balance."""
        self._c(self._lib.rt_group_set_phong_gbuffer(self.g, int(bool(on))), "rt_group_set_phong_gbuffer")

    def set_rectangles(self, on: bool):
        """Renderer.set_rectangles on every strip (rt_group_set_rectangles); kept when the strips are
        re-created."""
        self._c(self._lib.rt_group_set_rectangles(self.g, int(bool(on))), "rt_group_set_rectangles")

    def set_query_tree(self, on: bool):
        """Renderer.set_query_tree on every strip (rt_group_set_query_tree); kept when the strips are
        re-created."""
        self._c(self._lib.rt_group_set_query_tree(self.g, int(bool(on))), "rt_group_set_query_tree")

    def set_pool_list(self, on: bool):
        """Renderer.set_pool_list on every strip (rt_group_set_pool_list); kept when the strips are re-created."""
        self._c(self._lib.rt_group_set_pool_list(self.g, int(bool(on))), "rt_group_set_pool_list")

    def bind_frame(self, device_ptr: int | None):
        self._c(self._lib.rt_group_bind_frame(self.g, C.c_void_p(device_ptr) if device_ptr else None),
                "rt_group_bind_frame")

    def frame_device_ptr(self) -> int:
        return self._lib.rt_group_frame_device_ptr(self.g) or 0

    def upload_header(self, header: Header):
        assert header.S == self.S and header.AA == self.AA
        self._c(self._lib.rt_group_upload_header(self.g, header.data.ctypes.data_as(C.c_void_p), header.data.nbytes),
                "rt_group_upload_header")

    def dispatch(self, mode: int, frame: int) -> int:
        return self._c(self._lib.rt_group_dispatch(self.g, mode, frame), f"rt_group_dispatch(mode {mode})")

    def compute_frames(self, header: Header, mode: int, frame: int, n: int, rand_seed: int = 7000,
                       light_movement: bool = False) -> int:
        return self._c(self._lib.rt_group_compute_frames(self.g, header._p(), mode, frame, n, rand_seed,
                                                         int(bool(light_movement))), "rt_group_compute_frames")

    def synchronize(self):
        self._c(self._lib.rt_group_synchronize(self.g), "rt_group_synchronize")

    def image(self) -> np.ndarray:
        im = np.empty((self.H, self.W, 4), np.float32)
        self._c(self._lib.rt_group_download_image(self.g, fptr(im)), "rt_group_download_image")
        return im

    def enable_rgba8(self, on: bool = True, top_down: bool = True):
        """8-bit output (rt_group_enable_rgba8): every strip's frame is followed by its present and the
        strips are assembled as an [H][W] RGBA8 frame, a quarter of the float strips' bytes; image()
        raises while it is on."""
        self._c(self._lib.rt_group_enable_rgba8(self.g, int(bool(on)), int(bool(top_down))), "rt_group_enable_rgba8")

    def image8(self) -> np.ndarray:
        """The assembled 8-bit frame, uint8 [H][W][4], in the row order given to enable_rgba8."""
        out = np.empty((self.H, self.W, 4), np.uint8)
        self._c(self._lib.rt_group_download_rgba8(self.g, out.ctypes.data_as(C.c_void_p)), "rt_group_download_rgba8")
        return out

    def rgba8_device_ptr(self) -> int:
        return self._lib.rt_group_rgba8_device_ptr(self.g) or 0

    def image8_scaled(self, out_w: int, out_h: int, top_down: bool = True) -> np.ndarray:
        """The assembled float frame through the bilinear blit (rt_group_download_rgba8_scaled): uint8
        [out_h][out_w][4], equal to resample_rgba8(self.image(), out_w, out_h, top_down); raises
        while enable_rgba8 is on."""
        out = np.empty((max(0, int(out_h)), max(0, int(out_w)), 4), np.uint8)
        self._c(self._lib.rt_group_download_rgba8_scaled(self.g, int(out_w), int(out_h), int(bool(top_down)),
                                                         out.ctypes.data_as(C.c_void_p)),
                "rt_group_download_rgba8_scaled")
        return out

    def balance(self, header: Header, mode: int, rounds: int = 3) -> list[float]:
        """Cost-balance the strips (probe frame + `rounds` timed plans); returns the kept plan's
        per-strip ms per frame.  The strips restart with fresh rings."""
        ms = (C.c_double * self.n)()
        self._c(self._lib.rt_group_balance(self.g, header._p(), mode, rounds, ms), "rt_group_balance")
        return list(ms)


def quantize_rgba8(image, top_down: bool = True) -> np.ndarray:
    """rt_quantize_rgba8 (host only): float32 [R][W][4] -> uint8 [R][W][4] by the blit's rule (NaN and
    v <= 0 -> 0, v >= 1 -> 255, else float32 v * 255 + 0.5 truncated; alpha 255), the specification
    of Renderer.present.  top_down: output row j is image row R - 1 - j."""
    im = np.ascontiguousarray(image, np.float32)
    if im.ndim != 3 or im.shape[2] != 4:
        raise ValueError(f"quantize_rgba8: need an [R][W][4] image, got shape {im.shape}")
    out = np.empty(im.shape, np.uint8)
    _check(_lib.load().rt_quantize_rgba8(fptr(im), im.shape[1], im.shape[0], int(bool(top_down)),
                                         out.ctypes.data_as(C.c_void_p)), "rt_quantize_rgba8")
    return out


def resample_rgba8(image, out_w: int, out_h: int, top_down: bool = True) -> np.ndarray:
    """rt_resample_rgba8 (host only): float32 [R][W][4] -> uint8 [out_h][out_w][4], the image sampled
    bilinearly with clamped edges as the reference's blit samples its texture, then quantize_rgba8's
    conversion; the specification of Renderer.present_scaled (the rule: include/rt/abi.h).  top_down:
    output row 0 is the top row."""
    im = np.ascontiguousarray(image, np.float32)
    if im.ndim != 3 or im.shape[2] != 4:
        raise ValueError(f"resample_rgba8: need an [R][W][4] image, got shape {im.shape}")
    out = np.empty((max(0, int(out_h)), max(0, int(out_w)), 4), np.uint8)
    _check(_lib.load().rt_resample_rgba8(fptr(im), im.shape[1], im.shape[0], int(out_w), int(out_h),
                                         int(bool(top_down)), out.ctypes.data_as(C.c_void_p)), "rt_resample_rgba8")
    return out


def _query_cfg(header: Header, width: int = 1, height: int = 1):
    return _lib.rt_config(int(width), int(height), header.S, header.AA, 1, 1, 0, 0)


def rectangle_eval_host(shape, pos, dir) -> float:
    """rt_rectangle_eval_host (host only): the rectangle rule (include/rt/abi.h "Rectangles") for one
    packed shape row (20 floats) and one ray; t, or -1 for a miss."""
    s = np.ascontiguousarray(shape, np.float32).reshape(20)
    return float(_lib.load().rt_rectangle_eval_host(fptr(s), _f3(pos), _f3(dir)))


def trace_rays_host(header: Header, origins, dirs, thr: float = 1e-4, rectangles: bool = False) -> Hits:
    """rt_trace_rays_host_ex (host only): Renderer.trace_rays' rule in C on `header`, its specification;
    rectangles: as with Renderer.set_rectangles on (RT_SCENE_RECTANGLES)."""
    o, d = _rows(origins, 3, np.float32), _rows(dirs, 3, np.float32)
    if len(o) != len(d):
        raise ValueError(f"trace_rays_host: {len(o)} origins, {len(d)} directions")
    h = Hits.empty(len(o))
    _check(_lib.load().rt_trace_rays_host_ex(C.byref(_query_cfg(header)), header.data.ctypes.data_as(C.c_void_p),
                                             header.data.nbytes, fptr(o), fptr(d), len(o), thr,
                                             _lib.RT_SCENE_RECTANGLES if rectangles else 0, fptr(h.t), _iptr(h.ind),
                                             fptr(h.normals)), "rt_trace_rays_host_ex")
    return h


def pixel_rays_host(header: Header, width: int, height: int, xy):
    """rt_pixel_rays_host (host only): (origins, dirs) [n][3] of the camera's rays through the pixels
    xy ([n][2] ints) of a width x height frame, the rays Renderer.trace_pixels traces."""
    p = _rows(xy, 2, np.int32)
    o, d = np.zeros((len(p), 3), np.float32), np.zeros((len(p), 3), np.float32)
    _check(_lib.load().rt_pixel_rays_host(C.byref(_query_cfg(header, width, height)),
                                          header.data.ctypes.data_as(C.c_void_p), header.data.nbytes, _iptr(p), len(p),
                                          fptr(o), fptr(d)), "rt_pixel_rays_host")
    return o, d


def occluded_host(header: Header, a, b, rectangles: bool = False) -> np.ndarray:
    """rt_occluded_host_ex (host only): Renderer.occluded's rule in C on `header`, its specification;
    rectangles: as with Renderer.set_rectangles on."""
    a, b = _rows(a, 3, np.float32), _rows(b, 3, np.float32)
    if len(a) != len(b):
        raise ValueError(f"occluded_host: {len(a)} start points, {len(b)} end points")
    out = np.zeros(len(a), np.uint8)
    _check(_lib.load().rt_occluded_host_ex(C.byref(_query_cfg(header)), header.data.ctypes.data_as(C.c_void_p),
                                           header.data.nbytes, fptr(a), fptr(b), len(a),
                                           _lib.RT_SCENE_RECTANGLES if rectangles else 0,
                                           out.ctypes.data_as(C.c_void_p)), "rt_occluded_host_ex")
    return out.astype(bool)


def query_tree_host(header: Header, rectangles: bool = False) -> dict:
    """rt_query_tree_host (host only): the tree Renderer.set_query_tree builds for `header`:
    {"balls" [n][4] float32 (centre, R), "links" [n][4] int32 (skip, first, count, 0), "leaf_rows"
    [e][4] float32, "leaf_index" [e] int32, "always" [a] int32}; n = 0: no tree for this scene."""
    S = max(header.S, 1)
    balls, links = np.zeros((2 * S, 4), np.float32), np.zeros((2 * S, 4), np.int32)
    rows, index, always = np.zeros((S, 4), np.float32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    e, a = C.c_int(), C.c_int()
    n = _lib.load().rt_query_tree_host(C.byref(_query_cfg(header)), header.data.ctypes.data_as(C.c_void_p),
                                       header.data.nbytes, _lib.RT_SCENE_RECTANGLES if rectangles else 0, fptr(balls),
                                       _iptr(links), 2 * S, fptr(rows), _iptr(index), S, _iptr(always), S, C.byref(e),
                                       C.byref(a))
    if n < 0:
        raise ValueError("rt_query_tree_host rejected the header")
    return {"balls": balls[:n].copy(), "links": links[:n].copy(), "leaf_rows": rows[:e.value].copy(),
            "leaf_index": index[:e.value].copy(), "always": always[:a.value].copy()}


def ao_form_host(spp: int, depth: int, ncl: int, nobj: int, nplanes: int = 0, nrects: int = 0, counters: bool = False,
                 multi_frame: bool = False, cull_table: bool = False) -> str:
    """rt_ao_form_host (host only): the form the AO launcher's selector picks for such a launch, by
    the name the launch log gives it ("ao_batch_kernel<AoProd<sppc, dc, flagsu>>")."""
    out = (C.c_int * 3)()
    _check(_lib.load().rt_ao_form_host(int(spp), int(depth), int(ncl), int(nobj), int(nplanes), int(nrects),
                                       int(bool(counters)), int(bool(multi_frame)), int(bool(cull_table)), out),
           "rt_ao_form_host")
    return f"ao_batch_kernel<AoProd<{out[0]}, {out[1]}, {out[2]}u>>"


def plan_strips(row_cost, n: int) -> list[int]:
    """rt_plan_strips: contiguous strips of nearly equal total cost (host only)."""
    c = np.ascontiguousarray(row_cost, np.float64)
    b = (C.c_int * (n + 1))()
    _check(_lib.load().rt_plan_strips(c.ctypes.data_as(C.POINTER(C.c_double)), c.size, n, b), "rt_plan_strips")
    return list(b)


def plan_strips_gather(row_ms, n: int, width: int, link_gbps: float, ingest_gbps: float):
    """rt_plan_strips_gather (host only): strips AND root strip minimising
    max(render, per-link copy, root ingest); returns (bounds, root_strip, {T, render, link, ingest} ms)."""
    c = np.ascontiguousarray(row_ms, np.float64)
    b = (C.c_int * (n + 1))()
    root = C.c_int()
    out = (C.c_double * 4)()
    _check(_lib.load().rt_plan_strips_gather(c.ctypes.data_as(C.POINTER(C.c_double)), c.size, n, width,
                                             float(link_gbps), float(ingest_gbps), b, C.byref(root), out),
           "rt_plan_strips_gather")
    return list(b), root.value, dict(zip(("bound_ms", "render_ms", "link_ms", "ingest_ms"), list(out)))


def strip_gather_bound(row_ms, bounds, root_strip: int, width: int, link_gbps: float, ingest_gbps: float) -> dict:
    """rt_strip_gather_bound: the frame bound of a given plan {T, render, link, ingest} (ms)."""
    c = np.ascontiguousarray(row_ms, np.float64)
    n = len(bounds) - 1
    b = (C.c_int * (n + 1))(*[int(x) for x in bounds])
    out = (C.c_double * 4)()
    _check(_lib.load().rt_strip_gather_bound(c.ctypes.data_as(C.POINTER(C.c_double)), c.size, b, n, int(root_strip),
                                             width, float(link_gbps), float(ingest_gbps), out),
           "rt_strip_gather_bound")
    return dict(zip(("bound_ms", "render_ms", "link_ms", "ingest_ms"), list(out)))


def calibrate_row_cost(bounds, row_cost, strip_ms) -> np.ndarray:
    """rt_calibrate_row_cost: rescale the profile so each strip's total is its measured time."""
    c = np.array(row_cost, np.float64)
    n = len(bounds) - 1
    b = (C.c_int * (n + 1))(*[int(x) for x in bounds])
    t = np.ascontiguousarray(strip_ms, np.float64)
    _check(_lib.load().rt_calibrate_row_cost(c.ctypes.data_as(C.POINTER(C.c_double)), c.size, b, n,
                                             t.ctypes.data_as(C.POINTER(C.c_double))), "rt_calibrate_row_cost")
    return c


class FrameDriver:
    """compute() of src/main.cpp:553-578 with its per-frame host updates: the frame ring
    (static frame_num, 555/619), fill_rand_buffer for AO modes (seeded: 7000 + frame count),
    moving_light for Phong modes."""

    def __init__(self, renderer: Renderer, header: Header, lighting: int, light_movement: bool = False,
                 rand_seed0: int = 7000):
        self.r, self.h, self.lighting = renderer, header, lighting
        self.light_movement = light_movement
        self.frame_num = 0
        self.frames_done = 0
        self.rand_seed0 = rand_seed0

    def compute_many(self, n: int) -> int:
        """n compute() calls in one C++ loop (rt_compute_frames): same frames, less host time."""
        self.frame_num = self.r.compute_frames(self.h, self.lighting, self.frame_num, n,
                                               self.rand_seed0 + self.frames_done, self.light_movement)
        self.frames_done += n
        return self.frame_num

    def compute(self) -> int:
        if self.lighting in (1, 2):
            self.h.fill_rand_buffer(self.rand_seed0 + self.frames_done)
        else:
            self.h.moving_light(self.light_movement)
        self.h.set_mode(self.frame_num, self.h.num_objects)
        self.r.upload_header(self.h)
        self.frame_num = self.r.dispatch(self.lighting, self.frame_num)
        self.frames_done += 1
        return self.frame_num
