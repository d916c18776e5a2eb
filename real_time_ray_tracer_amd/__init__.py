"""MI355X-native per-pixel ray-scene intersection + shading hot path of
JustinPrivitera/Real_Time_Ray_Tracer (resources/{p,h,ao,aop}_compute.glsl,
aop_postprocessing.glsl) behind a C ABI (include/rt/abi.h, librtrt.so)."""
from ._lib import RtError, load  # noqa: F401
from .host import (AO_COMPUTE, AOP_COMPUTE, AOP_POSTPROCESSING, ASPECT_RATIO,  # noqa: F401
                   FULLSCREEN_ASPECT_RATIO, H_COMPUTE, P_COMPUTE, FrameDriver, GBuffer, Header, Hits,
                   Renderer, SSBO, StripGroup, aspect_for, header_floats, occluded_host, pixel_rays_host,
                   quantize_rgba8, query_tree_host, resample_rgba8, ssbo_floats, trace_rays_host,
                   rectangle_eval_host)
from .mesh import (Mesh, MeshHits, mesh_bvh_host, mesh_box_pass_host, mesh_occluded_host,  # noqa: F401
                   mesh_trace_rays_host, mesh_tri_eval_host, parse_obj)

__all__ = ["RtError", "load", "Renderer", "StripGroup", "Header", "SSBO", "GBuffer", "FrameDriver",
           "AOP_COMPUTE", "AOP_POSTPROCESSING", "AO_COMPUTE", "P_COMPUTE", "H_COMPUTE",
           "ASPECT_RATIO", "FULLSCREEN_ASPECT_RATIO", "aspect_for", "header_floats", "ssbo_floats",
           "quantize_rgba8", "resample_rgba8", "Hits", "trace_rays_host", "pixel_rays_host", "occluded_host",
           "rectangle_eval_host", "query_tree_host", "Mesh", "MeshHits", "mesh_trace_rays_host", "mesh_occluded_host",
           "mesh_bvh_host", "mesh_tri_eval_host", "mesh_box_pass_host", "parse_obj"]
