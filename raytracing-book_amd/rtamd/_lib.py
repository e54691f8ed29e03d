"""ctypes loaders for the in-tree native libraries.

* ``librtamd.so``    — the HIP kernel behind the C ABI of include/rt/rt.h (release:
  one kernel structure, no environment knobs).
* ``librtamd_ab.so`` — the same ABI built with -DRT_AB_KNOBS: the A/B kernel
  structures, stats kernels and RT_* environment knobs (variant tests, tools/).
* ``librtscene.so``  — the host scene builder of include/rt/rt_scene.h.

All are built in-tree by ``make -C raytracing-book_amd`` (see
__graft_entry__.build()).  There is no Python or CPU fallback for the render
path: if the library is missing, loading raises.  ``amd()`` is the release
library unless the harness sets RTAMD_LIB=ab (tools/ab_variants.py).
"""
import ctypes
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO_DIR = os.path.dirname(PKG_DIR)
LIB_DIR = os.path.join(PKG_DIR, "lib")
ASSET_DIR = os.path.join(REPO_DIR, "assets")

c_float_p = ctypes.POINTER(ctypes.c_float)
c_int_p = ctypes.POINTER(ctypes.c_int)

_amd = None
_amd_ab = None
_scene = None


class RTError(RuntimeError):
    """A negative status from the C ABI, with rt_last_error()'s message."""

    def __init__(self, code, msg):
        super().__init__(f"rt error {code}: {msg}")
        self.code = code


def _load(name):
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make -C {PKG_DIR}` "
            "(or __graft_entry__.build()); there is no fallback path")
    return ctypes.CDLL(path)


def _proto(lib, name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


class RtsInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "scene_id", "width", "height", "n_spheres", "n_quads", "n_boxes", "n_media",
        "n_lights", "n_bvh_nodes", "n_bvh_prims", "bvh_depth", "max_stack", "n_textures")] + [
        ("background", ctypes.c_float * 3)]


class RtsCamera(ctypes.Structure):
    _fields_ = [("look_from", ctypes.c_float * 3), ("look_at", ctypes.c_float * 3), ("vup", ctypes.c_float * 3),
                ("vfov", ctypes.c_float), ("defocus_angle", ctypes.c_float), ("focus_dist", ctypes.c_float),
                ("background", ctypes.c_float * 3)]


class RtTileSum(ctypes.Structure):
    """rt.h rt_tile_sum (numpy: TILE_SUM_DTYPE)."""
    _fields_ = [("m2y", ctypes.c_float), ("y", ctypes.c_float), ("bad", ctypes.c_uint32), ("pixels", ctypes.c_uint32)]


class RtNoiseStats(ctypes.Structure):
    """rt.h rt_noise_stats."""
    _fields_ = [("sum_m2y", ctypes.c_double), ("sum_y", ctypes.c_double), ("pixels", ctypes.c_uint64),
                ("bad", ctypes.c_uint64), ("frames", ctypes.c_int), ("converged", ctypes.c_int),
                ("noise", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtDenoiseParams(ctypes.Structure):
    """rt.h rt_denoise_params."""
    _fields_ = [("levels", ctypes.c_int), ("k", ctypes.c_float), ("reserved", ctypes.c_int * 6)]


class RtGuideParams(ctypes.Structure):
    """rt.h rt_guide_params."""
    _fields_ = [("kn", ctypes.c_float), ("kz", ctypes.c_float), ("ka", ctypes.c_float), ("reserved", ctypes.c_int * 5)]


class RtReprojectParams(ctypes.Structure):
    """rt.h rt_reproject_params."""
    _fields_ = [("cos_min", ctypes.c_float), ("kz", ctypes.c_float), ("max_history", ctypes.c_float),
                ("reserved", ctypes.c_int * 5)]


class RtPresentParams(ctypes.Structure):
    """rt.h rt_present_params."""
    _fields_ = [("source", ctypes.c_int), ("exposure", ctypes.c_float), ("keep_float", ctypes.c_int),
                ("reserved", ctypes.c_int * 5)]


class RtTileReach(ctypes.Structure):
    """rt.h rt_tile_reach (numpy: TILE_REACH_DTYPE)."""
    _fields_ = [("n_min", ctypes.c_float), ("n_sum", ctypes.c_float), ("short_px", ctypes.c_uint32),
                ("pixels", ctypes.c_uint32)]


class RtRefineParams(ctypes.Structure):
    """rt.h rt_refine_params."""
    _fields_ = [("min_count", ctypes.c_float), ("extra_frames", ctypes.c_int), ("min_pixels", ctypes.c_int),
                ("max_tiles", ctypes.c_int), ("reserved", ctypes.c_int * 4)]


class RtTileNoise(ctypes.Structure):
    """rt.h rt_tile_noise (numpy: TILE_NOISE_DTYPE)."""
    _fields_ = [("v_sum", ctypes.c_float), ("y_sum", ctypes.c_float), ("known_px", ctypes.c_uint16),
                ("thin_px", ctypes.c_uint16), ("bad_px", ctypes.c_uint16), ("pixels", ctypes.c_uint16)]


class RtMovedNoiseStats(ctypes.Structure):
    """rt.h rt_moved_noise_stats."""
    _fields_ = [("sum_v", ctypes.c_double), ("sum_y", ctypes.c_double), ("known", ctypes.c_uint64),
                ("thin", ctypes.c_uint64), ("bad", ctypes.c_uint64), ("pixels", ctypes.c_uint64),
                ("rounds", ctypes.c_int), ("converged", ctypes.c_int), ("noise", ctypes.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RtNoiseRefineParams(ctypes.Structure):
    """rt.h rt_noise_refine_params."""
    _fields_ = [("target_noise", ctypes.c_float), ("min_count", ctypes.c_float), ("batch_frames", ctypes.c_int),
                ("max_rounds", ctypes.c_int), ("reserved", ctypes.c_int * 4)]


RT_FEATURE_MISS = 0xFFFFFFFF   # rt.h

RT_PK_N = 33   # rt_debug.h RT_PK_N


class RtDebugSceneIn(ctypes.Structure):
    """rt_debug.h rt_debug_scene_in."""
    _fields_ = [("buf", ctypes.c_void_p * 6), ("buf_bytes", ctypes.c_size_t * 6),
                ("tex_format", ctypes.c_int * 8), ("tex_w", ctypes.c_int * 8), ("tex_h", ctypes.c_int * 8),
                ("tex", ctypes.c_void_p * 8), ("camera", c_float_p), ("max_depth", ctypes.c_int),
                ("background", ctypes.c_float * 3), ("sqrt_spp", ctypes.c_float), ("recip_sqrt_spp", ctypes.c_float),
                ("width", ctypes.c_int), ("height", ctypes.c_int), ("rank", ctypes.c_int), ("world", ctypes.c_int),
                ("stripe_rows", ctypes.c_int), ("options", c_int_p), ("n_options", ctypes.c_int), ("ab", ctypes.c_int),
                ("bvh_mode", ctypes.c_int), ("moments", ctypes.c_int), ("mask", c_int_p), ("n_mask", ctypes.c_int),
                ("prev_frames", ctypes.c_int), ("prev_tile_frames", c_int_p), ("first_frame", ctypes.c_int),
                ("n_frames", ctypes.c_int), ("waves", ctypes.c_longlong), ("free_bytes", ctypes.c_size_t)]


class RtDebugSceneOut(ctypes.Structure):
    """rt_debug.h rt_debug_scene_out."""
    _fields_ = [("pk", ctypes.c_int * RT_PK_N), ("launched", ctypes.c_int), ("bvh_mode", ctypes.c_int),
                ("vnodes", ctypes.c_int), ("collapsed", ctypes.c_int), ("rebuilt", ctypes.c_int),
                ("first_leaf", ctypes.c_int * 4), ("first_leaf_args", ctypes.c_uint * 3), ("spine_start", ctypes.c_uint),
                ("per_launch", ctypes.c_int), ("chunks_wanted", ctypes.c_int), ("staged", ctypes.c_int),
                ("n_chunks", ctypes.c_int), ("chunk_frames", ctypes.c_int), ("tail_chunks", ctypes.c_int),
                ("stage", ctypes.c_int), ("frames_all", ctypes.c_int), ("n_tile_frames", ctypes.c_int),
                ("tile_frames", c_int_p), ("tile_cap", ctypes.c_int), ("links", ctypes.c_void_p),
                ("links_cap", ctypes.c_size_t), ("links_f4", ctypes.c_int), ("args", ctypes.c_void_p),
                ("args_cap", ctypes.c_size_t), ("args_bytes", ctypes.c_size_t)]


def _amd_protos(L, old_rev=False):
    vp, sz, i, f, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint64
    ts_p, ns_p = ctypes.POINTER(RtTileSum), ctypes.POINTER(RtNoiseStats)
    if not old_rev or hasattr(L, "rt_set_moments"):   # amd_at: a revision from before the sample moments
        _proto(L, "rt_set_moments", i, vp, i)
        _proto(L, "rt_read_moments", i, vp, c_float_p)
        _proto(L, "rt_write_moments", i, vp, c_float_p, i)
        _proto(L, "rt_read_tile_sums", i, vp, ts_p, i, c_int_p)
        _proto(L, "rt_noise_from_tile_sums", i, ts_p, i, i, ns_p)
        _proto(L, "rt_noise", i, vp, ns_p)
        _proto(L, "rt_render_until", i, vp, i, i, i, u64, f, c_int_p, ns_p)
        _proto(L, "rt_debug_read_samples", i, vp, c_float_p, sz, c_int_p)
    if not old_rev or hasattr(L, "rt_set_active_tiles"):   # ... or from before the tile masks
        u8_p, i32_p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_set_active_tiles", i, vp, u8_p, i)
        _proto(L, "rt_read_tile_frames", i, vp, i32_p, i, c_int_p)
        _proto(L, "rt_write_tile_frames", i, vp, i32_p, i)
        _proto(L, "rt_noise_from_tile_sums_frames", i, ts_p, i32_p, i, ns_p)
        _proto(L, "rt_adaptive_select", i, ts_p, u8_p, i, i, i, f, u8_p, c_int_p)
        _proto(L, "rt_render_adaptive", i, vp, i, i, i, i, u64, f, c_int_p, ns_p)
    if not old_rev or hasattr(L, "rt_denoise"):   # ... or from before the preview filter
        dp_p, i32_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_denoise", i, vp, dp_p)
        _proto(L, "rt_read_denoised", i, vp, c_float_p)
        _proto(L, "rt_denoise_host", i, c_float_p, c_float_p, i32_p, i, i, i, dp_p, c_float_p)
    if not old_rev or hasattr(L, "rt_render_features"):   # ... or from before the first-hit feature buffers
        dp_p, gp_p, i32_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtGuideParams), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_render_features", i, vp)
        _proto(L, "rt_read_features", i, vp, c_float_p, c_float_p)
        _proto(L, "rt_denoise_guided", i, vp, dp_p, gp_p)
        _proto(L, "rt_denoise_guided_host", i, c_float_p, c_float_p, i32_p, i, c_float_p, c_float_p, i, i, dp_p, gp_p,
               c_float_p)
    if not old_rev or hasattr(L, "rt_reproject"):   # ... or from before the temporal reprojection
        rp_p, i32_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_history_capture", i, vp, i)
        _proto(L, "rt_reproject", i, vp, rp_p)
        _proto(L, "rt_read_reprojected", i, vp, c_float_p)
        _proto(L, "rt_reproject_host", i, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, i32_p, i, c_float_p,
               c_float_p, c_float_p, i, i, rp_p, c_float_p)
    if not old_rev or hasattr(L, "rt_set_history_variance"):   # ... or from before the variance carried through reprojection
        dp_p, gp_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtGuideParams)
        rp_p, i32_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_set_history_variance", i, vp, i)
        _proto(L, "rt_read_reprojected_variance", i, vp, c_float_p)
        _proto(L, "rt_denoise_reprojected", i, vp, dp_p, gp_p)
        _proto(L, "rt_history_variance_host", i, c_float_p, c_float_p, i32_p, i, i, i, c_float_p)
        _proto(L, "rt_reproject_variance_host", i, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
               i32_p, i, c_float_p, c_float_p, c_float_p, i, i, rp_p, c_float_p, c_float_p)
        _proto(L, "rt_denoise_reprojected_host", i, c_float_p, c_float_p, c_float_p, c_float_p, i, i, dp_p, gp_p, c_float_p)
    if not old_rev or hasattr(L, "rt_present"):   # ... or from before the presented frame
        dp_p, gp_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtGuideParams)
        rp_p, i32_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(ctypes.c_int32)
        pp_p, u8_p = ctypes.POINTER(RtPresentParams), ctypes.POINTER(ctypes.c_uint8)
        _proto(L, "rt_present", i, vp, pp_p)
        _proto(L, "rt_read_presented", i, vp, u8_p)
        _proto(L, "rt_read_presented_float", i, vp, c_float_p)
        _proto(L, "rt_bind_device_present", i, vp, vp, sz)
        _proto(L, "rt_present_host", i, c_float_p, c_float_p, c_float_p, i32_p, i, i, i, pp_p, u8_p, c_float_p)
        _proto(L, "rt_render_moved", i, vp, c_float_p, i, c_float_p, rp_p, dp_p, gp_p, pp_p)
    if not old_rev or hasattr(L, "rt_reach_tiles"):   # ... or from before the reach records
        dp_p, gp_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtGuideParams)
        rp_p, pp_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(RtPresentParams)
        tr_p, rf_p, u8_p = ctypes.POINTER(RtTileReach), ctypes.POINTER(RtRefineParams), ctypes.POINTER(ctypes.c_uint8)
        _proto(L, "rt_reach_tiles", i, vp, f)
        _proto(L, "rt_read_tile_reach", i, vp, tr_p, i, c_int_p)
        _proto(L, "rt_tile_reach_host", i, c_float_p, i, i, f, tr_p, i)
        _proto(L, "rt_refine_select", i, tr_p, i, i, i, u8_p, c_int_p)
        _proto(L, "rt_render_moved_refined", i, vp, c_float_p, i, c_float_p, rf_p, rp_p, dp_p, gp_p, pp_p, c_int_p)
    if not old_rev or hasattr(L, "rt_set_reproject_misses"):   # ... or from before the misses reprojected by direction
        rp_p, i32_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(ctypes.c_int32)
        _proto(L, "rt_set_reproject_misses", i, vp, i)
        _proto(L, "rt_reproject_misses_host", i, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p,
               i32_p, i, c_float_p, c_float_p, c_float_p, i, i, rp_p, c_float_p, c_float_p)
    if not old_rev or hasattr(L, "rt_noise_tiles"):   # ... or from before the noise records
        dp_p, gp_p = ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtGuideParams)
        rp_p, pp_p = ctypes.POINTER(RtReprojectParams), ctypes.POINTER(RtPresentParams)
        tn_p, nr_p, u8_p = ctypes.POINTER(RtTileNoise), ctypes.POINTER(RtNoiseRefineParams), ctypes.POINTER(ctypes.c_uint8)
        ms_p = ctypes.POINTER(RtMovedNoiseStats)
        _proto(L, "rt_noise_tiles", i, vp, f)
        _proto(L, "rt_read_tile_noise", i, vp, tn_p, i, c_int_p)
        _proto(L, "rt_tile_noise_host", i, c_float_p, c_float_p, i, i, f, tn_p, i)
        _proto(L, "rt_refine_noise_select", i, tn_p, u8_p, i, f, u8_p, c_int_p, ms_p)
        _proto(L, "rt_render_moved_to_noise", i, vp, c_float_p, i, c_float_p, nr_p, rp_p, dp_p, gp_p, pp_p, c_int_p, c_int_p,
               ctypes.POINTER(ctypes.c_int64), ms_p)
    _proto(L, "rt_abi_version", i)
    _proto(L, "rt_create", i, i, c_int_p, ctypes.POINTER(vp))
    _proto(L, "rt_destroy", i, vp)
    _proto(L, "rt_last_error", ctypes.c_char_p, vp)
    _proto(L, "rt_upload_buffer", i, vp, i, vp, sz)
    _proto(L, "rt_upload_texture", i, vp, i, i, i, i, vp)
    _proto(L, "rt_set_camera", i, vp, c_float_p)
    _proto(L, "rt_set_params", i, vp, i, c_float_p, f, f)
    _proto(L, "rt_resize", i, vp, i, i)
    _proto(L, "rt_render", i, vp, i, i, c_float_p)
    _proto(L, "rt_sync", i, vp)
    _proto(L, "rt_read_image", i, vp, c_float_p)
    _proto(L, "rt_write_image", i, vp, c_float_p)
    _proto(L, "rt_last_render_ns", i, vp, ctypes.POINTER(u64))
    _proto(L, "rt_render_done", i, vp, ctypes.POINTER(u64))
    _proto(L, "rt_set_partition", i, vp, i, i, i)
    _proto(L, "rt_local_rows", i, i, i, i, i)
    _proto(L, "rt_padded_local_rows", i, i, i, i)
    _proto(L, "rt_bind_device_image", i, vp, vp, sz)
    _proto(L, "rt_set_stream", i, vp, vp)
    _proto(L, "rt_deinterleave_rows", i, c_float_p, i, i, i, i, c_float_p)
    _proto(L, "rt_frame_rand_factor", f, u64, u64)
    _proto(L, "rt_comm_unique_id", i, vp)
    _proto(L, "rt_comm_init", i, vp, vp, i, i)
    _proto(L, "rt_gather_image", i, vp, c_float_p)
    _proto(L, "rt_gather_path", i, vp)
    _proto(L, "rt_comm_set_timeout", i, vp, i)
    _proto(L, "rt_comm_abort", i, vp)
    _proto(L, "rt_debug_eval_builtin", i, i, i, c_float_p, c_float_p, c_float_p, i)
    _proto(L, "rt_debug_threaded_bvh", i, vp, sz, vp, sz, c_int_p)
    _proto(L, "rt_debug_fast_tables", i, vp, sz, vp, sz, vp, sz, i, vp, sz, c_int_p,
           ctypes.POINTER(ctypes.c_uint32), sz, c_int_p, c_int_p)
    _proto(L, "rt_debug_link_nodes", i, vp, sz, vp, sz, c_int_p)
    _proto(L, "rt_debug_collapse_links", i, vp, sz, vp, i, i, i, vp, sz, c_int_p, vp, sz, c_int_p)
    _proto(L, "rt_debug_link_nodes_vbox", i, vp, sz, c_float_p, i, vp, sz, c_int_p, c_int_p)
    _proto(L, "rt_debug_box_records", i, vp, sz, vp, sz, c_int_p)
    _proto(L, "rt_debug_perlin_pack", i, c_float_p, i, i, vp, sz)
    _proto(L, "rt_debug_sphere_pair_leaves", i, vp, sz, c_int_p)
    _proto(L, "rt_debug_deinterleave", i, c_float_p, i, i, i, i, c_float_p)
    _proto(L, "rt_debug_device_count", i)
    _proto(L, "rt_debug_enable_stats", i, vp, i)
    _proto(L, "rt_debug_read_stats", i, vp, ctypes.POINTER(ctypes.c_ulonglong), i)
    _proto(L, "rt_debug_read_census", i, vp, ctypes.POINTER(ctypes.c_uint), ctypes.c_size_t,
           ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int))
    _proto(L, "rt_debug_count_node_hits", i, vp, i)
    _proto(L, "rt_debug_read_node_hits", i, vp, ctypes.POINTER(ctypes.c_uint), ctypes.c_size_t,
           ctypes.POINTER(ctypes.c_size_t))
    _proto(L, "rt_debug_set_collapse_hits", i, vp, ctypes.POINTER(ctypes.c_uint), ctypes.c_size_t,
           ctypes.c_ulonglong)
    _proto(L, "rt_debug_ab_build", i)
    _proto(L, "rt_debug_set_option", i, vp, i, i)
    _proto(L, "rt_debug_get_option", i, vp, i, c_int_p)
    _proto(L, "rt_debug_last_launch", i, vp, c_int_p, i)
    if not old_rev or hasattr(L, "rt_debug_plan_kernel"):   # ... or from before the host-side launch plan
        _proto(L, "rt_debug_plan_kernel", i, c_int_p, i, i, c_int_p, i, c_int_p, c_int_p, i, c_int_p)
    if not old_rev or hasattr(L, "rt_debug_plan_scene"):   # ... or from before the host-side argument assembly
        _proto(L, "rt_debug_plan_scene", i, ctypes.POINTER(RtDebugSceneIn), ctypes.POINTER(RtDebugSceneOut))
    if not old_rev or hasattr(L, "rt_debug_first_leaf"):   # ... or from before the first-leaf prologue
        _proto(L, "rt_debug_first_leaf", i, vp, c_int_p)
    if not old_rev or hasattr(L, "rt_debug_eval_op"):   # ... or from before the per-operation evaluator
        _proto(L, "rt_debug_eval_op", i, i, i, i, vp, sz, c_float_p, i, i, i, i, vp, ctypes.POINTER(ctypes.c_uint32),
               c_int_p)
    if not old_rev or hasattr(L, "rt_debug_eval_shade_op"):   # ... or from before the shading-operation evaluator
        _proto(L, "rt_debug_eval_shade_op", i, vp, i, i, i, c_float_p, i, ctypes.POINTER(ctypes.c_uint32))
    _proto(L, "rt_set_bvh_mode", i, vp, i)
    _proto(L, "rt_debug_walk_bvh", i, vp, vp, sz, ctypes.POINTER(sz))
    _proto(L, "rt_debug_build_sah_bvh", i, vp, sz, vp, sz, vp, sz, vp, sz, vp, sz, i, c_float_p, f, vp, sz,
           ctypes.POINTER(sz))
    return L


def _import_torch_first():
    # One HIP runtime per process.  torch ships its own libamdhip64 (SONAME
    # libamdhip64.so.7, the name librtamd needs): loaded first, it is the one
    # librtamd binds to, so torch tensors/streams handed to rt_bind_device_image /
    # rt_set_stream belong to the same runtime.  Loaded after /opt/rocm's copy,
    # torch would bring a second runtime that sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def amd():
    """The product library (HIP), or the A/B build when RTAMD_LIB=ab.  Raises
    ImportError when it was not built."""
    global _amd
    if os.environ.get("RTAMD_LIB") == "ab":
        return amd_ab()
    if _amd is None:
        _import_torch_first()
        _amd = _amd_protos(_load("librtamd.so"))
    return _amd


def amd_ab():
    """The A/B build of the same ABI (kernel variants, stats kernels, RT_* knobs)."""
    global _amd_ab
    if _amd_ab is None:
        _import_torch_first()
        _amd_ab = _amd_protos(_load("librtamd_ab.so"))
    return _amd_ab


_amd_at = {}


def amd_at(path):
    """Another build of the same ABI loaded from `path` (tools/lib_ab.py: a previous
    revision's kernel timed beside the current one in one process)."""
    path = os.path.abspath(path)
    if path not in _amd_at:
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing")
        _import_torch_first()
        _amd_at[path] = _amd_protos(ctypes.CDLL(path), old_rev=True)
    return _amd_at[path]


def scene_lib():
    """The host scene builder (no GPU needed)."""
    global _scene
    if _scene is None:
        L = _load("librtscene.so")
        vp, sz, i, f = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
        _proto(L, "rts_build", i, i, i, i, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(vp))
        _proto(L, "rts_free", None, vp)
        _proto(L, "rts_last_error", ctypes.c_char_p)
        _proto(L, "rts_decode_image", i, ctypes.c_char_p, c_int_p, c_int_p, c_int_p,
               ctypes.POINTER(ctypes.c_uint8), sz)
        _proto(L, "rts_decode_last_error", ctypes.c_char_p)
        _proto(L, "rts_get_info", i, vp, ctypes.POINTER(RtsInfo))
        _proto(L, "rts_get_buffer", i, vp, i, ctypes.POINTER(vp), ctypes.POINTER(sz))
        _proto(L, "rts_get_texture", i, vp, i, c_int_p, c_int_p, c_int_p, ctypes.POINTER(vp), ctypes.POINTER(sz))
        _proto(L, "rts_get_camera", i, vp, c_float_p)
        _proto(L, "rts_set_image_size", i, vp, i, i)
        _proto(L, "rts_spp_uniforms", None, i, c_float_p, c_float_p)
        _proto(L, "rts_tonemap_rgb8", i, c_float_p, i, i, ctypes.POINTER(ctypes.c_uint8))
        _proto(L, "rts_save_png", i, c_float_p, i, i, ctypes.c_char_p)
        _proto(L, "rts_java_random_next_int", ctypes.c_int32, ctypes.c_int64, i)
        _proto(L, "rts_java_random_next_double", ctypes.c_double, ctypes.c_int64, i)
        _proto(L, "rts_java_random_next_float", f, ctypes.c_int64, i)
        _proto(L, "rts_java_random_next_int_bound", ctypes.c_int32, ctypes.c_int64, i)
        f3 = ctypes.POINTER(ctypes.c_float)
        _proto(L, "rts_new", i, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(vp))
        _proto(L, "rts_solid_texture", i, vp, f, f, f, c_int_p)
        _proto(L, "rts_checker_texture", i, vp, f3, f3, f, c_int_p)
        _proto(L, "rts_perlin_texture", i, vp, f, c_int_p)
        _proto(L, "rts_image_texture", i, vp, ctypes.c_char_p, i, i, c_int_p)
        _proto(L, "rts_material", i, vp, i, i, f, f3, c_int_p)
        _proto(L, "rts_sphere", i, vp, f3, f3, f, i, c_int_p)
        _proto(L, "rts_quad", i, vp, f3, f3, f3, i, c_int_p)
        _proto(L, "rts_box", i, vp, f3, f3, f3, f3, i, c_int_p)
        _proto(L, "rts_constant_medium", i, vp, i, f, i, c_int_p)
        _proto(L, "rts_add_model", i, vp, i)
        _proto(L, "rts_add_light", i, vp, i)
        _proto(L, "rts_camera", i, vp, ctypes.POINTER(RtsCamera))
        _proto(L, "rts_finish", i, vp, i, i)
        _scene = L
    return _scene


def debug_eval_op(op, form, rows, recs=None, tex=None, device=0, lib=None):
    """rt_debug_eval_op (rt_debug.h): the render kernels' own operation `op` in device form `form` over
    rows ([n, 12] float32), one lane per row.  recs: the rows' records as the uploads carry them (any
    array of n records' bytes); tex: (format, w, h, texel array) for the Perlin and texture ops.
    Returns (words [n, 8] uint32, flags [4] ints); device < 0 runs the host half alone (flags)."""
    import numpy as np
    L = lib or amd()
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    if rows.shape != (n, 12):
        raise ValueError("rows must be [n, 12] float32")
    rb = None if recs is None else np.ascontiguousarray(recs).view(np.uint8).reshape(-1)
    fmt, w, h, texels = tex if tex is not None else (0, 0, 0, None)
    tb = None if texels is None else np.ascontiguousarray(texels)
    out = np.zeros((n, 8), np.uint32)
    flags = (ctypes.c_int * 4)()
    rc = L.rt_debug_eval_op(device, op, form, None if rb is None else rb.ctypes.data, 0 if rb is None else rb.size,
                            rows.ctypes.data_as(c_float_p), n, fmt, w, h, None if tb is None else tb.ctypes.data,
                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), flags)
    if rc != 0:
        raise RTError(rc, f"rt_debug_eval_op(op {op}, form {form})")
    return out, list(flags)


def debug_eval_shade_op(ctx, op, form, rows, device=0, lib=None):
    """rt_debug_eval_shade_op (rt_debug.h): the render kernels' sampling, light, camera or shading
    operation `op` (RT_SOP_*) in device form `form` over rows ([n, 20] float32), one lane per row, on the
    scene a RenderContext uploaded.  Returns the words [n, 12] uint32; device < 0 runs the input guard
    alone (ctx may be None) and returns None."""
    import numpy as np
    L = lib or (ctx._L if ctx is not None else amd())
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    if rows.shape != (n, 20):
        raise ValueError("rows must be [n, 20] float32")
    out = np.zeros((n, 12), np.uint32)
    h = ctx._h if ctx is not None else None
    rc = L.rt_debug_eval_shade_op(h, device, op, form, rows.ctypes.data_as(c_float_p), n,
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    if rc != 0:
        raise RTError(rc, L.rt_last_error(h).decode() if h is not None else f"rt_debug_eval_shade_op(op {op}, form {form})")
    return out if device >= 0 else None
