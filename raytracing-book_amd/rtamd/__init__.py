"""rtamd — MI355X-native path-tracing hot path of Bowen951209/raytracing-book.

Layers:
  * rtamd.scene   — host scene builder bindings (Scene.java + RaytraceModel.java mirror)
  * rtamd.render  — rt.h context + RaytraceExecutor mirror
  * rtamd.dist    — one-process-per-GPU stripe partition + RCCL gather
The compute path is the HIP kernel in lib/librtamd.so; nothing here computes pixels.
"""
from ._lib import RTError, amd, amd_ab, scene_lib  # noqa: F401
from .render import (OPTIONS, TILE_SUM_DTYPE, TILE_REACH_DTYPE, TILE_NOISE_DTYPE, RaytraceExecutor, RenderContext, comm_unique_id,  # noqa: F401
                     deinterleave, frame_rand_factors,
                     local_rows, noise_from_tile_sums, noise_from_tile_sums_frames, adaptive_select, denoise_host, denoise_guided_host, history_from_image, reproject_host, history_variance_host, reproject_variance_host, denoise_reprojected_host, present_host, tile_reach_host, refine_select, tile_noise_host, refine_noise_select, pack_albedo_id, padded_local_rows, plan_scene, sah_bvh, stripe_rows_of)
from .scene import SCENE_NAMES, Scene, SceneBuilder, decode_image, save_png, spp_uniforms, tonemap_rgb8  # noqa: F401
