"""Render context and the RaytraceExecutor mirror over the rt.h C ABI.

``RenderContext`` owns an ``rt_ctx`` (one or more MI355X devices, or one
stripe-partition of a multi-process render) and uploads a ``Scene`` the way the
reference's Java side fills its SSBOs/UBO/textures.  ``RaytraceExecutor``
restates J/system/RaytraceExecutor.java (setSamplePerPixel, raytrace,
sampleComplete, resetCompleteState, completion listeners) with frames batched
per kernel launch instead of one dispatch per vsync.
"""
import ctypes
import time

import numpy as np

from . import _lib
from ._lib import RTError, c_float_p
from .scene import Scene, spp_uniforms

MASK64 = (1 << 64) - 1


def frame_rand_factors(seed, start, n):
    """u_rand_factor for frames [start, start+n): top 24 bits of
    splitmix64(seed, frame)/2^24 (rt.h rt_frame_rand_factor; stands in for the
    reference's per-frame (float)Math.random(), RaytraceExecutor.java:124)."""
    out = np.empty(n, dtype=np.float32)
    for k in range(n):
        z = (seed + (start + k + 1) * 0x9E3779B97F4A7C15) & MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        z ^= z >> 31
        out[k] = np.float32(z >> 40) / np.float32(16777216.0)
    return out


def comm_unique_id(lib=None):
    """rt_comm_unique_id: a fresh 128-byte RCCL communicator id (rank 0 makes it, the host
    hands it to every rank)."""
    L = lib or _lib.amd()
    buf = ctypes.create_string_buffer(128)
    rc = L.rt_comm_unique_id(buf)
    if rc != 0:
        raise RTError(rc, "rt_comm_unique_id failed (RCCL unavailable)")
    return buf.raw


def sah_bvh(scene, order=2, eye=None, prim_cost=1.0, lib=None):
    """rt_debug_build_sah_bvh (no device needed): the RT_BVH_SAH tree of a Scene's prims, as the
    reference's BVH bytes (binding 1).  order 2 with the camera position (the default) is
    rt_set_bvh_mode's tree."""
    L = lib or _lib.amd()
    b = scene.buffers
    keep = [ctypes.create_string_buffer(b[k], len(b[k])) if b[k] else None for k in range(6)]
    e = (ctypes.c_float * 3)(*(eye if eye is not None else scene.camera[4:7]))
    n = ctypes.c_size_t()
    args = (keep[0], len(b[0]), keep[2], len(b[2]), keep[3], len(b[3]), keep[4], len(b[4]), keep[1], len(b[1]),
            int(order), e, float(prim_cost))
    rc = L.rt_debug_build_sah_bvh(*args, None, 0, ctypes.byref(n))
    if rc != 0:
        raise RTError(rc, "rt_debug_build_sah_bvh failed")
    out = ctypes.create_string_buffer(max(1, n.value))
    rc = L.rt_debug_build_sah_bvh(*args, out, n.value, ctypes.byref(n))
    if rc != 0:
        raise RTError(rc, "rt_debug_build_sah_bvh failed")
    return out.raw[:n.value]


def plan_scene(scene, frames, first_frame=1, width=None, height=None, options=None, ab=False, bvh_mode=0,
               moments=False, mask=None, prev_frames=0, prev_tile_frames=None, rank=0, world=1, stripe_rows=16,
               max_depth=5, spp=None, waves=4096, free_bytes=1 << 38, want_links=False, want_args=False, lib=None):
    """rt_debug_plan_scene (no device needed): what rt_render would assemble and launch first for a Scene,
    as a dict -- "pk" (int32 array: rt_debug_plan_kernel's input), "launched", the scene's last_launch
    fields ("bvh_mode", "box_vnodes", "collapsed", "rebuilt"), "first_leaf" (rt_debug_first_leaf's four
    words), the split and chunks, "tile_frames" (the counts after the call, one per tile of the stripe),
    and on request "links" (float32 array) and "args" (the argument block's bytes).  mask: ascending tile
    indices; options: dict name -> int as for RenderContext."""
    L = lib or _lib.amd()
    i = _lib.RtDebugSceneIn()
    keep = []
    for k in range(6):
        data = scene.buffers[k]
        b = ctypes.create_string_buffer(data, len(data)) if data else None
        keep.append(b)
        i.buf[k] = ctypes.addressof(b) if b is not None else None
        i.buf_bytes[k] = len(data)
    for t in scene.textures:
        b = ctypes.create_string_buffer(t.data, len(t.data))
        keep.append(b)
        i.tex[t.slot] = ctypes.addressof(b)
        i.tex_format[t.slot], i.tex_w[t.slot], i.tex_h[t.slot] = t.format, t.width, t.height
    cam = np.ascontiguousarray(scene.camera, dtype=np.float32)
    i.camera = cam.ctypes.data_as(c_float_p)
    i.max_depth = int(max_depth)
    i.background[:] = [float(x) for x in scene.background]
    i.sqrt_spp, i.recip_sqrt_spp = spp_uniforms(spp or frames)
    i.width, i.height = int(width or scene.width), int(height or scene.height)
    i.rank, i.world, i.stripe_rows = int(rank), int(world), int(stripe_rows)
    pairs = np.array([[OPTIONS[k], int(v)] for k, v in (options or {}).items()], np.int32).reshape(-1, 2)
    i.options, i.n_options = pairs.ctypes.data_as(_lib.c_int_p), len(pairs)
    i.ab, i.moments = int(bool(ab)), int(bool(moments))
    i.bvh_mode = BVH_MODES[bvh_mode] if isinstance(bvh_mode, str) else int(bvh_mode)
    m = None if mask is None else np.ascontiguousarray(mask, np.int32)
    i.mask, i.n_mask = (None, -1) if m is None else (m.ctypes.data_as(_lib.c_int_p), int(m.size))
    nt = ((i.width + 7) // 8) * ((local_rows(i.height, i.rank, i.world, i.stripe_rows) + 7) // 8)
    i.prev_frames = int(prev_frames)
    prev = None
    if prev_tile_frames is not None:
        prev = np.ascontiguousarray(prev_tile_frames, np.int32)
        if prev.size != nt:
            raise ValueError("one previous count per tile")
        i.prev_tile_frames = prev.ctypes.data_as(_lib.c_int_p)
    i.first_frame, i.n_frames = int(first_frame), int(frames)
    i.waves, i.free_bytes = int(waves), int(free_bytes)
    o = _lib.RtDebugSceneOut()
    tiles = np.zeros(max(nt, 1), np.int32)
    o.tile_frames, o.tile_cap = tiles.ctypes.data_as(_lib.c_int_p), nt
    rc = L.rt_debug_plan_scene(ctypes.byref(i), ctypes.byref(o))
    links = args = None
    if rc == 0 and (want_links or want_args):   # the sizes are known now
        links = np.zeros(4 * o.links_f4, np.float32)
        args = np.zeros(o.args_bytes, np.uint8)
        if want_links:
            o.links, o.links_cap = links.ctypes.data, links.nbytes
        if want_args:
            o.args, o.args_cap = args.ctypes.data, args.nbytes
        rc = L.rt_debug_plan_scene(ctypes.byref(i), ctypes.byref(o))
    if rc != 0:
        raise RTError(rc, "rt_debug_plan_scene failed")
    out = {k: getattr(o, k) for k in ("launched", "bvh_mode", "collapsed", "rebuilt", "spine_start", "per_launch",
                                     "chunks_wanted", "staged", "n_chunks", "chunk_frames", "tail_chunks", "stage")}
    out["box_vnodes"] = o.vnodes
    out["pk"] = np.array(o.pk[:], np.int32)
    out["first_leaf"] = list(o.first_leaf)
    out["first_leaf_args"] = list(o.first_leaf_args)
    out["tile_frames"] = tiles[:nt].copy() if o.n_tile_frames else np.full(nt, o.frames_all, np.int32)
    if want_links:
        out["links"] = links
    if want_args:
        out["args"] = args
    return out


def local_rows(height, rank, world, stripe_rows):
    n_stripes = (height + stripe_rows - 1) // stripe_rows
    return sum(min(stripe_rows, height - s * stripe_rows) for s in range(rank, n_stripes, world))


def padded_local_rows(height, world, stripe_rows):
    n_stripes = (height + stripe_rows - 1) // stripe_rows
    return ((n_stripes + world - 1) // world) * stripe_rows


def stripe_rows_of(height, rank, world, stripe_rows):
    """Global row indices owned by `rank`, in local (compact) order."""
    n_stripes = (height + stripe_rows - 1) // stripe_rows
    rows = []
    for s in range(rank, n_stripes, world):
        rows.extend(range(s * stripe_rows, min(height, (s + 1) * stripe_rows)))
    return np.array(rows, dtype=np.int64)


def deinterleave(gathered, height, world, stripe_rows):
    """[world, padded_rows, W, 4] gathered stripe blocks -> [H, W, 4] image."""
    W = gathered.shape[2]
    out = np.zeros((height, W, 4), dtype=gathered.dtype)
    for k in range(world):
        rows = stripe_rows_of(height, k, world, stripe_rows)
        out[rows] = gathered[k, :len(rows)]
    return out


# rt_debug.h RT_OPTION_*: per-context options set by explicit calls (the release library
# reads no environment).  Below 100 they never change a bit of the image; 100+ exist in
# the A/B build only.
OPTIONS = {"box_pretest": 1, "fastdiv": 2, "sph_lds": 3, "big_wg": 4, "chunk_target": 5,
           "staged_chunk_target": 6, "stage_tiles": 7, "sm_batch": 8, "sm_frac": 9, "walk_frac": 10,
           "watchdog_ms": 11, "chunk_wait_ms": 12, "lds_node_cap": 13, "compact_boxes": 14, "spine": 15,
           "tl_leaf_lds": 16, "perlin_packed": 17, "sparse_stage": 18, "sphere_pairs": 19, "leaf_prefetch": 20, "tl_small_lds": 21, "shade_lds": 22, "box_vnodes": 23, "zero_dir_end": 24, "collapse": 25, "rebuild": 26, "tail_chunks": 27, "box_interior": 28, "first_leaf": 29, "kernel_variant": 100, "debug_flags": 101}
# rt_debug_last_launch fields
LAUNCH_FIELDS = ("shape", "block", "fastdiv", "pretest", "lds_bytes", "lds_nodes", "box_records", "staged",
                 "chunks", "spine", "sparse", "sphere_pairs", "leaf_prefetch", "shade_lds", "walk_frac", "bvh_mode",
                 "box_vnodes", "collapsed", "rebuilt", "box_interior", "tiles_active")
BVH_MODES = {"reference": 0, "sah": 1}   # rt.h RT_BVH_*
TILE_SUM_DTYPE = np.dtype([("m2y", "<f4"), ("y", "<f4"), ("bad", "<u4"), ("pixels", "<u4")])   # rt.h rt_tile_sum


def noise_from_tile_sums(tiles, frames, lib=None):
    """rt_noise_from_tile_sums (host only) over TILE_SUM_DTYPE records -> dict."""
    L = lib or _lib.amd()
    t = np.ascontiguousarray(tiles, dtype=TILE_SUM_DTYPE)
    s = _lib.RtNoiseStats()
    rc = L.rt_noise_from_tile_sums(t.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum)), int(t.size), int(frames),
                                   ctypes.byref(s))
    if rc != 0:
        raise RTError(rc, "rt_noise_from_tile_sums: frames >= 2 required")
    return s.as_dict()


def noise_from_tile_sums_frames(tiles, frames, lib=None):
    """rt_noise_from_tile_sums_frames (host only): TILE_SUM_DTYPE records, one frame count per tile -> dict."""
    L = lib or _lib.amd()
    t = np.ascontiguousarray(tiles, dtype=TILE_SUM_DTYPE)
    n = np.ascontiguousarray(frames, dtype=np.int32)
    if n.size != t.size:
        raise ValueError("one frame count per tile")
    s = _lib.RtNoiseStats()
    rc = L.rt_noise_from_tile_sums_frames(t.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum)),
                                          n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(t.size), ctypes.byref(s))
    if rc != 0:
        raise RTError(rc, "rt_noise_from_tile_sums_frames: every count >= 2 required")
    return s.as_dict()


def adaptive_select(tiles, active, frames, min_frames, target, lib=None):
    """rt_adaptive_select (host only): which active tiles keep sampling after `frames` frames ->
    uint8 array, one per tile (active None: all tiles active)."""
    L = lib or _lib.amd()
    t = np.ascontiguousarray(tiles, dtype=TILE_SUM_DTYPE)
    u8_p = ctypes.POINTER(ctypes.c_uint8)
    a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    if a is not None and a.size != t.size:
        raise ValueError("one active byte per tile")
    out = np.zeros(t.size, np.uint8)
    n = ctypes.c_int()
    rc = L.rt_adaptive_select(t.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum)),
                              None if a is None else a.ctypes.data_as(u8_p), int(t.size), int(frames), int(min_frames),
                              float(target), out.ctypes.data_as(u8_p), ctypes.byref(n))
    if rc != 0:
        raise RTError(rc, "rt_adaptive_select: frames >= 1 and min_frames >= 2 required")
    return out


DENOISE_DEFAULTS = (3, 3.0)   # rt.h rt_denoise: levels, k


def _denoise_params(levels, k):
    """rt_denoise_params for (levels, k); None for both = NULL (the library's defaults)."""
    if levels is None and k is None:
        return None
    p = _lib.RtDenoiseParams()
    p.levels = DENOISE_DEFAULTS[0] if levels is None else int(levels)
    p.k = DENOISE_DEFAULTS[1] if k is None else float(k)
    return ctypes.byref(p)


def denoise_host(image, m2, tile_frames, levels=None, k=None, lib=None):
    """rt_denoise_host (host only, no device): the preview filter over an [H, W, 4] image, its M2 and one
    frame count per 8x8 tile (row-major; a scalar stands for every tile) -> [H, W, 4] float32."""
    L = lib or _lib.amd()
    img = np.ascontiguousarray(image, dtype=np.float32)
    mom = np.ascontiguousarray(m2, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or mom.shape != img.shape:
        raise ValueError("image and m2 are [H, W, 4]")
    H, W = img.shape[:2]
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
    if tf.size == 1:
        tf = np.full(nt, tf[0], np.int32)
    out = np.empty_like(img)
    rc = L.rt_denoise_host(img.ctypes.data_as(c_float_p), mom.ctypes.data_as(c_float_p),
                           tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size), W, H,
                           _denoise_params(levels, k), out.ctypes.data_as(c_float_p))
    if rc != 0:
        raise RTError(rc, "rt_denoise_host: levels 1..5, k > 0, one count >= 2 per 8x8 tile required")
    return out


def _guide_params(guides):
    """rt_guide_params for (kn, kz, ka); True = NULL (the library's defaults)."""
    if guides is True:
        return None
    kn, kz, ka = guides
    p = _lib.RtGuideParams()
    p.kn, p.kz, p.ka = float(kn), float(kz), float(ka)
    return ctypes.byref(p)


def denoise_guided_host(image, m2, tile_frames, normal_depth, albedo_id, levels=None, k=None, guides=True, lib=None):
    """rt_denoise_guided_host (host only): denoise_host with the first-hit guides.  normal_depth and
    albedo_id are [H, W, 4] float32 (albedo_id's w holds the id's bits); guides is (kn, kz, ka), or True
    for the library's defaults."""
    L = lib or _lib.amd()
    img = np.ascontiguousarray(image, dtype=np.float32)
    mom = np.ascontiguousarray(m2, dtype=np.float32)
    nd = np.ascontiguousarray(normal_depth, dtype=np.float32)
    ai = np.ascontiguousarray(albedo_id, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or mom.shape != img.shape or nd.shape != img.shape or ai.shape != img.shape:
        raise ValueError("image, m2, normal_depth and albedo_id are [H, W, 4]")
    H, W = img.shape[:2]
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
    if tf.size == 1:
        tf = np.full(nt, tf[0], np.int32)
    out = np.empty_like(img)
    rc = L.rt_denoise_guided_host(img.ctypes.data_as(c_float_p), mom.ctypes.data_as(c_float_p),
                                  tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size),
                                  nd.ctypes.data_as(c_float_p), ai.ctypes.data_as(c_float_p), W, H,
                                  _denoise_params(levels, k), _guide_params(guides), out.ctypes.data_as(c_float_p))
    if rc != 0:
        raise RTError(rc, "rt_denoise_guided_host: levels 1..5, k > 0, kn, kz, ka >= 0, one count >= 2 per 8x8 tile required")
    return out


def pack_albedo_id(albedo, ids):
    """(albedo [H, W, 3] float32, id [H, W] uint32) -> albedo_id [H, W, 4] float32, the id's bits in w."""
    a = np.ascontiguousarray(albedo, dtype=np.float32)
    out = np.empty(a.shape[:2] + (4,), np.float32)
    out[..., :3] = a
    out.view(np.uint32)[..., 3] = np.ascontiguousarray(ids, dtype=np.uint32)
    return out


REPROJECT_DEFAULTS = (0.9, 0.1, 64.0)   # rt.h RT_REPROJECT_DEFAULT_*: cos_min, kz, max_history
HISTORY_SOURCES = {"image": 0, "reprojected": 1}   # rt.h RT_HISTORY_FROM_*


def _reproject_params(cos_min, kz, max_history):
    """rt_reproject_params for (cos_min, kz, max_history); None for all three = NULL (the library's defaults)."""
    if cos_min is None and kz is None and max_history is None:
        return None
    p = _lib.RtReprojectParams()
    p.cos_min = REPROJECT_DEFAULTS[0] if cos_min is None else float(cos_min)
    p.kz = REPROJECT_DEFAULTS[1] if kz is None else float(kz)
    p.max_history = REPROJECT_DEFAULTS[2] if max_history is None else float(max_history)
    return ctypes.byref(p)


def history_from_image(image, tile_frames):
    """What rt_history_capture keeps of an [H, W, 4] image and one frame count per 8x8 tile (row-major; a
    scalar stands for every tile): [H, W, 4] float32 (r, g, b, n), n = 0 where a component of rgb is not finite."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    H, W = img.shape[:2]
    tx, ty = (W + 7) // 8, (H + 7) // 8
    tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
    if tf.size == 1:
        tf = np.full(tx * ty, tf[0], np.int32)
    n = np.repeat(np.repeat(tf.reshape(ty, tx), 8, axis=0), 8, axis=1)[:H, :W].astype(np.float32)
    out = img.copy()
    out[..., 3] = np.where(np.isfinite(img[..., :3]).all(axis=-1), n, np.float32(0.0))
    return out


def reproject_host(history, history_nd, history_ai, history_camera, image, tile_frames, normal_depth, albedo_id, camera,
                   cos_min=None, kz=None, max_history=None, lib=None, misses=False):
    """rt_reproject_host (host only, no device): the history (r, g, b, n), its first-hit buffers and 28-float
    camera block; the current image, one frame count per 8x8 tile (row-major; a scalar stands for every tile),
    first-hit buffers and camera block -> [H, W, 4] float32 (r, g, b, n_out).  All buffers are [H, W, 4].
    misses: rt_reproject_misses_host's no-variance form, the misses reprojected by direction."""
    L = lib or _lib.amd()
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (history, history_nd, history_ai, image, normal_depth, albedo_id)]
    img = arrs[3]
    if img.ndim != 3 or img.shape[2] != 4 or any(a.shape != img.shape for a in arrs):
        raise ValueError("history, image and the first-hit buffers are [H, W, 4]")
    cams = [np.ascontiguousarray(c, dtype=np.float32).ravel() for c in (history_camera, camera)]
    if any(c.size != 28 for c in cams):
        raise ValueError("a camera block is 28 floats")
    H, W = img.shape[:2]
    nt = ((W + 7) // 8) * ((H + 7) // 8)
    tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
    if tf.size == 1:
        tf = np.full(nt, tf[0], np.int32)
    out = np.empty_like(img)
    fp = lambda a: a.ctypes.data_as(c_float_p)  # noqa: E731
    if misses:
        rc = L.rt_reproject_misses_host(fp(arrs[0]), fp(arrs[1]), fp(arrs[2]), None, fp(cams[0]), fp(img), None,
                                        tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size), fp(arrs[4]),
                                        fp(arrs[5]), fp(cams[1]), W, H, _reproject_params(cos_min, kz, max_history), fp(out),
                                        None)
    else:
        rc = L.rt_reproject_host(fp(arrs[0]), fp(arrs[1]), fp(arrs[2]), fp(cams[0]), fp(img),
                                 tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size), fp(arrs[4]), fp(arrs[5]),
                                 fp(cams[1]), W, H, _reproject_params(cos_min, kz, max_history), fp(out))
    if rc != 0:
        raise RTError(rc, "rt_reproject_host: cos_min in [-1, 1], kz >= 0, max_history > 0, one count >= 0 per 8x8 tile "
                          "and a history camera with independent pixel deltas and view corner required")
    return out


def _tile_frames_of(tile_frames, W, H):
    tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
    if tf.size == 1:
        tf = np.full(((W + 7) // 8) * ((H + 7) // 8), tf[0], np.int32)
    return tf


def history_variance_host(image, m2, tile_frames, lib=None):
    """rt_history_variance_host (host only): what rt_history_capture keeps as s2 under set_history_variance():
    [H, W] float32 from an [H, W, 4] image, its M2 and one frame count per 8x8 tile (a scalar stands for every
    tile); -1 where unknown."""
    L = lib or _lib.amd()
    img = np.ascontiguousarray(image, dtype=np.float32)
    mom = np.ascontiguousarray(m2, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4 or mom.shape != img.shape:
        raise ValueError("image and m2 are [H, W, 4]")
    H, W = img.shape[:2]
    tf = _tile_frames_of(tile_frames, W, H)
    out = np.empty((H, W), np.float32)
    rc = L.rt_history_variance_host(img.ctypes.data_as(c_float_p), mom.ctypes.data_as(c_float_p),
                                    tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size), W, H,
                                    out.ctypes.data_as(c_float_p))
    if rc != 0:
        raise RTError(rc, "rt_history_variance_host: one count >= 0 per 8x8 tile required")
    return out


def reproject_variance_host(history, history_nd, history_ai, history_s2, history_camera, image, m2, tile_frames, normal_depth,
                            albedo_id, camera, cos_min=None, kz=None, max_history=None, lib=None, misses=False):
    """rt_reproject_variance_host (host only): reproject_host with the history's s2 [H, W] and the current
    view's M2 [H, W, 4] -> ([H, W, 4] float32 (r, g, b, n_out), [H, W] float32 s2).
    misses: rt_reproject_misses_host's variance form, the misses reprojected by direction."""
    L = lib or _lib.amd()
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (history, history_nd, history_ai, image, m2, normal_depth, albedo_id)]
    img = arrs[3]
    if img.ndim != 3 or img.shape[2] != 4 or any(a.shape != img.shape for a in arrs):
        raise ValueError("history, image, m2 and the first-hit buffers are [H, W, 4]")
    hs2 = np.ascontiguousarray(history_s2, dtype=np.float32)
    if hs2.shape != img.shape[:2]:
        raise ValueError("history_s2 is [H, W]")
    cams = [np.ascontiguousarray(c, dtype=np.float32).ravel() for c in (history_camera, camera)]
    if any(c.size != 28 for c in cams):
        raise ValueError("a camera block is 28 floats")
    H, W = img.shape[:2]
    tf = _tile_frames_of(tile_frames, W, H)
    out, s2 = np.empty_like(img), np.empty((H, W), np.float32)
    fp = lambda a: a.ctypes.data_as(c_float_p)  # noqa: E731
    entry = L.rt_reproject_misses_host if misses else L.rt_reproject_variance_host
    rc = entry(fp(arrs[0]), fp(arrs[1]), fp(arrs[2]), fp(hs2), fp(cams[0]), fp(img), fp(arrs[4]),
               tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(tf.size), fp(arrs[5]), fp(arrs[6]),
               fp(cams[1]), W, H, _reproject_params(cos_min, kz, max_history), fp(out), fp(s2))
    if rc != 0:
        raise RTError(rc, "rt_reproject_variance_host: cos_min in [-1, 1], kz >= 0, max_history > 0, one count >= 0 per 8x8 "
                          "tile and a history camera with independent pixel deltas and view corner required")
    return out, s2


def denoise_reprojected_host(rgbn, s2, normal_depth, albedo_id, levels=None, k=None, guides=True, lib=None):
    """rt_denoise_reprojected_host (host only): the preview filter over a reprojected view [H, W, 4] (r, g, b, n)
    and its s2 [H, W] -> [H, W, 4] float32 (w = 1).  guides: (kn, kz, ka), True for the library's defaults,
    None / False for the unguided filter."""
    L = lib or _lib.amd()
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (rgbn, normal_depth, albedo_id)]
    img = arrs[0]
    if img.ndim != 3 or img.shape[2] != 4 or any(a.shape != img.shape for a in arrs):
        raise ValueError("rgbn, normal_depth and albedo_id are [H, W, 4]")
    v = np.ascontiguousarray(s2, dtype=np.float32)
    if v.shape != img.shape[:2]:
        raise ValueError("s2 is [H, W]")
    H, W = img.shape[:2]
    g = (0.0, 0.0, 0.0) if guides is None or guides is False else guides
    out = np.empty_like(img)
    fp = lambda a: a.ctypes.data_as(c_float_p)  # noqa: E731
    rc = L.rt_denoise_reprojected_host(fp(img), fp(v), fp(arrs[1]), fp(arrs[2]), W, H, _denoise_params(levels, k),
                                       _guide_params(g), fp(out))
    if rc != 0:
        raise RTError(rc, "rt_denoise_reprojected_host: levels 1..5, k > 0, kn, kz, ka >= 0 required")
    return out


PRESENT_SOURCES = {"image": 0, "denoised": 1, "reprojected": 2, "moved": 3}   # rt.h RT_PRESENT_*


def _present_params(source, exposure, keep_float):
    """rt_present_params for (source, exposure, keep_float)."""
    p = _lib.RtPresentParams()
    p.source = PRESENT_SOURCES[source] if isinstance(source, str) else int(source)
    p.exposure = float(exposure)
    p.keep_float = 1 if keep_float else 0
    return ctypes.byref(p)


def present_host(source="image", image=None, denoised=None, reprojected=None, tile_frames=None, exposure=1.0,
                 keep_float=False, lib=None):
    """rt_present_host (host only, no device): the presented frame of the [H, W, 4] float32 buffers the source
    reads ("moved": reprojected, denoised and one frame count per 8x8 tile, row-major; a scalar stands for
    every tile) -> [H, W, 4] uint8 (r, g, b, 255), with keep_float (that, the float copy [H, W, 4] float32)."""
    L = lib or _lib.amd()
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (image, denoised, reprojected)]
    given = [a for a in arrs if a is not None]
    if not given or any(a.ndim != 3 or a.shape[2] != 4 or a.shape != given[0].shape for a in given):
        raise ValueError("image, denoised and reprojected are [H, W, 4]")
    H, W = given[0].shape[:2]
    tf = None
    if tile_frames is not None:
        tf = np.ascontiguousarray(tile_frames, dtype=np.int32).ravel()
        if tf.size == 1:
            tf = np.full(((W + 7) // 8) * ((H + 7) // 8), tf[0], np.int32)
    out = np.empty((H, W, 4), np.uint8)
    flt = np.empty((H, W, 4), np.float32) if keep_float else None
    fp = lambda a: None if a is None else a.ctypes.data_as(c_float_p)  # noqa: E731
    rc = L.rt_present_host(fp(arrs[0]), fp(arrs[1]), fp(arrs[2]),
                           None if tf is None else tf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                           0 if tf is None else int(tf.size), W, H, _present_params(source, exposure, keep_float),
                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), fp(flt))
    if rc != 0:
        raise RTError(rc, "rt_present_host: a source of RT_PRESENT_* with the buffers it reads, exposure > 0 and finite, "
                          "one count >= 0 per 8x8 tile required")
    return (out, flt) if keep_float else out


TILE_REACH_DTYPE = np.dtype([("n_min", "<f4"), ("n_sum", "<f4"), ("short_px", "<u4"), ("pixels", "<u4")])   # rt.h rt_tile_reach


def tile_reach_host(rgbn, min_count, lib=None):
    """rt_tile_reach_host (host only, no device): one TILE_REACH_DTYPE record per 8x8 tile (row-major) of a
    reprojected result [H, W, 4] float32 (r, g, b, n_out): the smallest and the summed good count, the pixels
    whose count is short of min_count, the pixels in the image."""
    L = lib or _lib.amd()
    r = np.ascontiguousarray(rgbn, dtype=np.float32)
    if r.ndim != 3 or r.shape[2] != 4:
        raise ValueError("rgbn is [H, W, 4]")
    H, W = r.shape[:2]
    out = np.zeros(((W + 7) // 8) * ((H + 7) // 8), dtype=TILE_REACH_DTYPE)
    rc = L.rt_tile_reach_host(r.ctypes.data_as(c_float_p), W, H, float(min_count),
                              out.ctypes.data_as(ctypes.POINTER(_lib.RtTileReach)), int(out.size))
    if rc != 0:
        raise RTError(rc, "rt_tile_reach_host: min_count > 0 and finite required")
    return out


def refine_select(reach, min_pixels=1, max_tiles=0, lib=None):
    """rt_refine_select (host only, pure): the tiles with short_px >= min_pixels -> uint8 array, one per tile.
    max_tiles > 0: the threshold rises until at most that many remain; equal counts stay or go together, so
    fewer may be chosen, and none when every tile is entirely fresh."""
    L = lib or _lib.amd()
    t = np.ascontiguousarray(reach, dtype=TILE_REACH_DTYPE)
    out = np.zeros(t.size, np.uint8)
    n = ctypes.c_int()
    rc = L.rt_refine_select(t.ctypes.data_as(ctypes.POINTER(_lib.RtTileReach)), int(t.size), int(min_pixels),
                            int(max_tiles), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(n))
    if rc != 0:
        raise RTError(rc, "rt_refine_select: min_pixels in 1 .. 64, max_tiles >= 0, every short_px <= 64 required")
    return out


def _refine_params(refine):
    """rt_refine_params for a dict of extra_frames, min_count, min_pixels, max_tiles (missing keys: 0)."""
    unknown = set(refine) - {"extra_frames", "min_count", "min_pixels", "max_tiles"}
    if unknown:
        raise ValueError(f"refine: unknown keys {sorted(unknown)}")
    p = _lib.RtRefineParams()
    p.min_count = float(refine.get("min_count") or 0.0)
    p.extra_frames = int(refine.get("extra_frames") or 0)
    p.min_pixels = int(refine.get("min_pixels") or 0)
    p.max_tiles = int(refine.get("max_tiles") or 0)
    return p


TILE_NOISE_DTYPE = np.dtype([("v_sum", "<f4"), ("y_sum", "<f4"), ("known_px", "<u2"), ("thin_px", "<u2"),
                             ("bad_px", "<u2"), ("pixels", "<u2")])   # rt.h rt_tile_noise


def tile_noise_host(rgbn, s2, min_count, lib=None):
    """rt_tile_noise_host (host only, no device): one TILE_NOISE_DTYPE record per 8x8 tile (row-major) of a
    reprojected result [H, W, 4] float32 (r, g, b, n) and its s2 [H, W]: the summed variance of the pixels' means
    and the summed y, the pixels whose variance is known, the thin ones (no variance, or a count below min_count),
    the bad ones, the pixels in the image."""
    L = lib or _lib.amd()
    r = np.ascontiguousarray(rgbn, dtype=np.float32)
    if r.ndim != 3 or r.shape[2] != 4:
        raise ValueError("rgbn is [H, W, 4]")
    v = np.ascontiguousarray(s2, dtype=np.float32)
    if v.shape != r.shape[:2]:
        raise ValueError("s2 is [H, W]")
    H, W = r.shape[:2]
    out = np.zeros(((W + 7) // 8) * ((H + 7) // 8), dtype=TILE_NOISE_DTYPE)
    rc = L.rt_tile_noise_host(r.ctypes.data_as(c_float_p), v.ctypes.data_as(c_float_p), W, H, float(min_count),
                              out.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise)), int(out.size))
    if rc != 0:
        raise RTError(rc, "rt_tile_noise_host: min_count > 0 and finite required")
    return out


def refine_noise_select(tiles, target, active=None, lib=None):
    """rt_refine_noise_select (host only, pure): the tiles still active at the noise target -> (uint8 array, one per
    tile; the stats as a dict).  A tile stays active while it has a thin pixel or its mean variance of the mean
    exceeds (target * ybar)^2; active: the tiles active so far (None: all), an inactive tile stays inactive."""
    L = lib or _lib.amd()
    t = np.ascontiguousarray(tiles, dtype=TILE_NOISE_DTYPE)
    a = None
    if active is not None:
        a = np.ascontiguousarray(active, dtype=np.uint8).ravel()
        if a.size != t.size:
            raise ValueError("active holds one byte per tile")
    out = np.zeros(t.size, np.uint8)
    n = ctypes.c_int()
    stats = _lib.RtMovedNoiseStats()
    u8_p = ctypes.POINTER(ctypes.c_uint8)
    rc = L.rt_refine_noise_select(t.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise)), None if a is None else a.ctypes.data_as(u8_p),
                                  int(t.size), float(target), out.ctypes.data_as(u8_p), ctypes.byref(n), ctypes.byref(stats))
    if rc != 0:
        raise RTError(rc, "rt_refine_noise_select: target >= 0 and finite, every count <= 64, known_px + bad_px <= pixels required")
    return out, stats.as_dict()


def _noise_refine_params(noise_refine):
    """rt_noise_refine_params for a dict of target_noise and optionally batch_frames (1), max_rounds (4), min_count (0)."""
    unknown = set(noise_refine) - {"target_noise", "batch_frames", "max_rounds", "min_count"}
    if unknown:
        raise ValueError(f"noise_refine: unknown keys {sorted(unknown)}")
    if "target_noise" not in noise_refine:
        raise ValueError("noise_refine: target_noise is required")
    p = _lib.RtNoiseRefineParams()
    p.target_noise = float(noise_refine["target_noise"])
    p.min_count = float(noise_refine.get("min_count") or 0.0)
    p.batch_frames = int(noise_refine.get("batch_frames", 1))
    p.max_rounds = int(noise_refine.get("max_rounds", 4))
    return p


SHAPES = {0: "fast-lds", 1: "fast-global", 2: "link-lds", 3: "meta-lds", 4: "meta-global", 5: "link-two-level"}


class RenderContext:
    """An rt_ctx: device buffers, accumulation image and launch state.

    ``options`` (dict name -> int, see OPTIONS) are applied right after creation;
    ``ab=True`` uses the A/B build (librtamd_ab.so) for kernel-variant options; ``lib`` a
    library at that path (tools/lib_ab.py)."""

    def __init__(self, devices=(0,), rank=0, world=1, stripe_rows=16, options=None, ab=False, lib=None):
        L = _lib.amd_at(lib) if lib else (_lib.amd_ab() if ab else _lib.amd())
        self._L = L
        devs = (ctypes.c_int * len(devices))(*devices)
        h = ctypes.c_void_p()
        rc = L.rt_create(len(devices), devs, ctypes.byref(h))
        if rc != 0:
            raise RTError(rc, L.rt_last_error(None).decode())
        self._h = h
        self.devices = tuple(devices)
        self.rank, self.world, self.stripe_rows = rank, world, stripe_rows
        if world > 1 or stripe_rows != 16:
            self._check(L.rt_set_partition(h, rank, world, stripe_rows))
        self.width = self.height = 0
        self.max_depth = 5
        self.background = np.zeros(3, np.float32)
        self.sqrt_spp, self.recip_sqrt_spp = 1.0, 1.0
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_bvh_mode(self, mode):
        """rt_set_bvh_mode: "reference" (default, bit-exact) or "sah" (non-parity fast mode)."""
        self._check(self._L.rt_set_bvh_mode(self._h, BVH_MODES[mode] if isinstance(mode, str) else int(mode)))

    def walk_bvh(self):
        """rt_debug_walk_bvh: the BVH bytes (reference node format) the link walk runs on."""
        n = ctypes.c_size_t()
        self._check(self._L.rt_debug_walk_bvh(self._h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(1, n.value))
        self._check(self._L.rt_debug_walk_bvh(self._h, buf, n.value, ctypes.byref(n)))
        return buf.raw[:n.value]

    def set_option(self, name, value):
        """rt_debug_set_option (rt_debug.h RT_OPTION_*)."""
        self._check(self._L.rt_debug_set_option(self._h, OPTIONS[name], int(value)))

    def get_option(self, name):
        v = ctypes.c_int()
        self._check(self._L.rt_debug_get_option(self._h, OPTIONS[name], ctypes.byref(v)))
        return v.value

    def count_node_hits(self, on=True):
        """rt_debug_count_node_hits: arm (and zero) the stats twin's per-node hit count."""
        self._check(self._L.rt_debug_count_node_hits(self._h, 1 if on else 0))

    def read_node_hits(self):
        """rt_debug_read_node_hits -> (hits per link node as uint32 array, walks begun at the root)."""
        n = ctypes.c_size_t()
        self._check(self._L.rt_debug_read_node_hits(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.uint32)
        self._check(self._L.rt_debug_read_node_hits(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                                     out.size, ctypes.byref(n)))
        return out[:-1].copy(), int(out[-1])

    def set_collapse_hits(self, hits, walks):
        """rt_debug_set_collapse_hits: plan the collapse from measured hits (empty: the camera grid)."""
        h = np.ascontiguousarray(hits, np.uint32)
        self._check(self._L.rt_debug_set_collapse_hits(self._h, h.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                                        h.size, int(walks)))

    def last_launch(self):
        """rt_debug_last_launch as a dict (the launch shape the last rt_render took)."""
        out = (ctypes.c_int * len(LAUNCH_FIELDS))()
        if self._L.rt_debug_last_launch(self._h, out, len(LAUNCH_FIELDS)) != 0:
            # a library from before tiles_active (tools/lib_ab.py): its 20 fields
            self._check(self._L.rt_debug_last_launch(self._h, out, 20))
        d = dict(zip(LAUNCH_FIELDS, out[:len(LAUNCH_FIELDS)]))
        d["shape_name"] = SHAPES.get(d["shape"], "?")
        return d

    def first_leaf(self):
        """rt_debug_first_leaf as a dict: whether the last rt_render armed the first-leaf prologue, and
        that leaf's link, type byte and prim word."""
        out = (ctypes.c_int * 4)()
        self._check(self._L.rt_debug_first_leaf(self._h, out))
        return {"armed": out[0], "link": out[1] & 0xFFFFFFFF, "types": out[2], "prims": out[3] & 0xFFFFFFFF}

    def _check(self, rc):
        if rc != 0:
            raise RTError(rc, self._L.rt_last_error(self._h).decode())
        return rc

    # -- scene upload (RaytraceModel.putModelsToProgram, Texture.putData, Camera.init)
    def upload_scene(self, scene: Scene):
        for b in range(6):
            data = scene.buffers[b]
            buf = ctypes.create_string_buffer(data, len(data)) if data else None
            self._check(self._L.rt_upload_buffer(self._h, b, buf, len(data)))
        for t in scene.textures:
            buf = ctypes.create_string_buffer(t.data, len(t.data))
            self._check(self._L.rt_upload_texture(self._h, t.slot, t.format, t.width, t.height, buf))
        self.set_camera(scene.camera)
        self.background = scene.background.copy()

    def set_camera(self, ubo):
        ubo = np.ascontiguousarray(ubo, dtype=np.float32)
        assert ubo.size == 28
        self._check(self._L.rt_set_camera(self._h, ubo.ctypes.data_as(c_float_p)))

    def set_params(self, max_depth=None, background=None, spp=None, uniforms=None):
        """uniforms = (sqrt_spp, recip_sqrt_spp) as raw floats, instead of spp's."""
        if max_depth is not None:
            self.max_depth = int(max_depth)
        if background is not None:
            self.background = np.asarray(background, np.float32)
        if spp is not None:
            self.sqrt_spp, self.recip_sqrt_spp = spp_uniforms(spp)
        if uniforms is not None:
            self.sqrt_spp, self.recip_sqrt_spp = float(np.float32(uniforms[0])), float(np.float32(uniforms[1]))
        bg = np.ascontiguousarray(self.background, dtype=np.float32)
        self._check(self._L.rt_set_params(self._h, self.max_depth, bg.ctypes.data_as(c_float_p),
                                          self.sqrt_spp, self.recip_sqrt_spp))

    def resize(self, width, height):
        self._check(self._L.rt_resize(self._h, int(width), int(height)))
        self.width, self.height = int(width), int(height)

    @property
    def local_rows(self):
        if len(self.devices) > 1:
            return self.height
        return local_rows(self.height, self.rank, self.world, self.stripe_rows)

    @property
    def padded_rows(self):
        return padded_local_rows(self.height, self.world, self.stripe_rows)

    def render(self, first_frame, rand_factors):
        rf = np.ascontiguousarray(rand_factors, dtype=np.float32)
        self._check(self._L.rt_render(self._h, int(first_frame), int(rf.size), rf.ctypes.data_as(c_float_p)))

    def sync(self):
        self._check(self._L.rt_sync(self._h))

    def last_render_ns(self):
        v = ctypes.c_uint64()
        self._check(self._L.rt_last_render_ns(self._h, ctypes.byref(v)))
        return v.value

    def render_done(self):
        """rt_render_done: the last render's device ns once it finished, else None (no wait)."""
        v = ctypes.c_uint64()
        rc = self._L.rt_render_done(self._h, ctypes.byref(v))
        if rc < 0:
            self._check(rc)
        return v.value if rc == 1 else None

    def read_image(self):
        """[local_rows, W, 4] float32 (the full image for an unpartitioned context)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_image(self._h, out.ctypes.data_as(c_float_p)))
        return out

    def write_image(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        self._check(self._L.rt_write_image(self._h, rgba.ctypes.data_as(c_float_p)))

    # -- per-pixel sample moments and the noise-target loop (rt.h rt_set_moments ...)
    def set_moments(self, on=True):
        """rt_set_moments: keep the per-pixel second moments beside the running mean (every launch
        staged; the image's bits do not change).  Single-device contexts."""
        self._check(self._L.rt_set_moments(self._h, 1 if on else 0))

    def read_moments(self):
        """rt_read_moments: M2 as [local_rows, W, 4] float32 (x, y, z and the channel sum)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_moments(self._h, out.ctypes.data_as(c_float_p)))
        return out

    def write_moments(self, m2, n_frames):
        """rt_write_moments: resume from a checkpoint (after write_image)."""
        m2 = np.ascontiguousarray(m2, dtype=np.float32)
        assert m2.size == self.local_rows * self.width * 4
        self._check(self._L.rt_write_moments(self._h, m2.ctypes.data_as(c_float_p), int(n_frames)))

    def tile_sums(self):
        """rt_read_tile_sums: one TILE_SUM_DTYPE record per 8x8 tile, row-major."""
        n = ctypes.c_int()
        self._check(self._L.rt_read_tile_sums(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=TILE_SUM_DTYPE)
        self._check(self._L.rt_read_tile_sums(self._h, out.ctypes.data_as(ctypes.POINTER(_lib.RtTileSum)), n.value,
                                              ctypes.byref(n)))
        return out

    def noise(self):
        """rt_noise as a dict (sum_m2y, sum_y, pixels, bad, frames, converged, noise)."""
        s = _lib.RtNoiseStats()
        self._check(self._L.rt_noise(self._h, ctypes.byref(s)))
        return s.as_dict()

    def render_until(self, target_noise, max_frames, batch_frames, seed=1, first_frame=1):
        """rt_render_until -> (frames rendered, the last batch's noise dict)."""
        s = _lib.RtNoiseStats()
        done = ctypes.c_int()
        self._check(self._L.rt_render_until(self._h, int(first_frame), int(max_frames), int(batch_frames),
                                            ctypes.c_uint64(seed), float(target_noise), ctypes.byref(done),
                                            ctypes.byref(s)))
        return done.value, s.as_dict()

    # -- tile masks, per-tile frame counts and the adaptive loop (rt.h rt_set_active_tiles ...)
    def set_active_tiles(self, active):
        """rt_set_active_tiles: one byte per 8x8 tile (row-major); render() then samples only the
        tiles whose byte is non-zero.  None: every tile again."""
        if active is None:
            self._check(self._L.rt_set_active_tiles(self._h, None, 0))
            return
        a = np.ascontiguousarray(active, dtype=np.uint8).ravel()
        self._check(self._L.rt_set_active_tiles(self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), int(a.size)))

    def read_tile_frames(self):
        """rt_read_tile_frames: the frames 1 .. n each tile holds (0 = invalid), int32 per tile."""
        n = ctypes.c_int()
        self._check(self._L.rt_read_tile_frames(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._check(self._L.rt_read_tile_frames(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value,
                                                ctypes.byref(n)))
        return out

    def write_tile_frames(self, frames):
        """rt_write_tile_frames: resume a checkpoint's per-tile counts (after write_image / write_moments)."""
        f = np.ascontiguousarray(frames, dtype=np.int32).ravel()
        self._check(self._L.rt_write_tile_frames(self._h, f.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(f.size)))

    def render_adaptive(self, target_noise, max_frames, batch_frames, min_frames=16, seed=1, first_frame=1):
        """rt_render_adaptive -> (frames of the longest-sampled tiles, the final noise dict)."""
        s = _lib.RtNoiseStats()
        done = ctypes.c_int()
        self._check(self._L.rt_render_adaptive(self._h, int(first_frame), int(max_frames), int(batch_frames),
                                               int(min_frames), ctypes.c_uint64(seed), float(target_noise),
                                               ctypes.byref(done), ctypes.byref(s)))
        return done.value, s.as_dict()

    # -- the variance-guided preview filter (rt.h rt_denoise)
    def denoise(self, levels=None, k=None, guides=None):
        """rt_denoise + rt_read_denoised: the filtered image as [H, W, 4] float32 (w = 1).  Image and
        moments are left as they are.  Needs set_moments() and at least two frames in every tile.
        guides: None = unguided; (kn, kz, ka), or True for the library's defaults = rt_denoise_guided
        over the first-hit buffers (render_features() first)."""
        if guides is None or guides is False:
            self._check(self._L.rt_denoise(self._h, _denoise_params(levels, k)))
        else:
            self._check(self._L.rt_denoise_guided(self._h, _denoise_params(levels, k), _guide_params(guides)))
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_denoised(self._h, out.ctypes.data_as(c_float_p)))
        return out

    # -- the first-hit feature buffers (rt.h rt_render_features)
    def render_features(self):
        """rt_render_features: queue the first-hit pass (one centre ray per pixel, media left out)."""
        self._check(self._L.rt_render_features(self._h))

    def read_features_raw(self):
        """rt_read_features as stored: (normal_depth, albedo_id), [H, W, 4] float32 each."""
        nd = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        ai = np.empty_like(nd)
        self._check(self._L.rt_read_features(self._h, nd.ctypes.data_as(c_float_p), ai.ctypes.data_as(c_float_p)))
        return nd, ai

    def read_features(self):
        """rt_read_features: (normal_depth [H, W, 4] f32, albedo [H, W, 3] f32, id [H, W] u32); a miss has
        N = 0, t = -1, the background colour and id RT_FEATURE_MISS."""
        nd, ai = self.read_features_raw()
        return nd, np.ascontiguousarray(ai[..., :3]), np.ascontiguousarray(ai.view(np.uint32)[..., 3])

    # -- temporal reprojection (rt.h rt_history_capture / rt_reproject)
    def history_capture(self, source="image"):
        """rt_history_capture: keep (r, g, b, n), the first-hit buffers and the camera as the history, from the
        image ("image": needs set_moments() and render_features()) or from the last reproject() result
        ("reprojected")."""
        self._check(self._L.rt_history_capture(self._h, HISTORY_SOURCES[source] if isinstance(source, str) else int(source)))

    def reproject(self, cos_min=None, kz=None, max_history=None):
        """rt_reproject: queue the gather of the history into the current view (after the camera move, the new
        view's render and render_features()).  Image, moments, counts and features are left as they are."""
        self._check(self._L.rt_reproject(self._h, _reproject_params(cos_min, kz, max_history)))

    def read_reprojected(self):
        """rt_read_reprojected: the result as [H, W, 4] float32 (r, g, b, n_out)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_reprojected(self._h, out.ctypes.data_as(c_float_p)))
        return out

    def set_history_variance(self, on=True):
        """rt_set_history_variance: carry the per-sample variance of y with the history and the reprojected
        result (off by default; a change drops both)."""
        self._check(self._L.rt_set_history_variance(self._h, 1 if on else 0))
        self._history_variance = bool(on)

    def set_reproject_misses(self, on=True):
        """rt_set_reproject_misses: reproject() carries a miss (the background, seen through the scene's fog) over
        by its ray's direction too.  Off by default; changing it drops the reprojected result and keeps the history."""
        self._check(self._L.rt_set_reproject_misses(self._h, 1 if on else 0))

    def read_reprojected_variance(self):
        """rt_read_reprojected_variance: the result's s2 as [H, W] float32 (negative: unknown)."""
        out = np.empty((self.local_rows, self.width), dtype=np.float32)
        self._check(self._L.rt_read_reprojected_variance(self._h, out.ctypes.data_as(c_float_p)))
        return out

    def denoise_reprojected(self, levels=None, k=None, guides=True):
        """rt_denoise_reprojected + rt_read_denoised: the preview filter over the reprojected view, [H, W, 4]
        float32 (w = 1).  Needs set_history_variance() and reproject().  guides: (kn, kz, ka), True for the
        library's defaults, None / False for the unguided filter (all-zero strengths)."""
        g = (0.0, 0.0, 0.0) if guides is None or guides is False else guides
        self._check(self._L.rt_denoise_reprojected(self._h, _denoise_params(levels, k), _guide_params(g)))
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_denoised(self._h, out.ctypes.data_as(c_float_p)))
        return out

    # -- the presented frame (rt.h rt_present / rt_render_moved)
    def read_presented(self):
        """rt_read_presented: the frame held as [H, W, 4] uint8 (r, g, b, 255)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.uint8)
        self._check(self._L.rt_read_presented(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def present(self, source="image", exposure=1.0, keep_float=False):
        """rt_present + rt_read_presented: compose ("moved"), expose and tonemap on the device -> [H, W, 4] uint8.
        source: "image", "denoised", "reprojected" or "moved" (the filtered buffer where the reprojected view's
        count did not grow, the reprojected view elsewhere).  keep_float: read_presented_float() has the
        exposed floats."""
        self._check(self._L.rt_present(self._h, _present_params(source, exposure, keep_float)))
        return self.read_presented()

    def read_presented_float(self):
        """rt_read_presented_float: the frame's float copy [H, W, 4] float32 (e.r, e.g, e.b, w); w is 1 but
        where "moved" shows the reprojected view.  Needs a present(keep_float=True)."""
        out = np.empty((self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_read_presented_float(self._h, out.ctypes.data_as(c_float_p)))
        return out

    def bind_device_present(self, ptr, nbytes=0):
        """rt_bind_device_present: later frames go to caller-owned device memory (a torch uint8 tensor's
        data_ptr() of at least H * W * 4 bytes), on the context's stream; None / 0 returns to the internal buffer."""
        self._check(self._L.rt_bind_device_present(self._h, ctypes.c_void_p(ptr or None), ctypes.c_size_t(nbytes)))

    # -- extra frames where the history does not reach (rt.h rt_reach_tiles / rt_render_moved_refined)
    def reach_tiles(self, min_count):
        """rt_reach_tiles: queue the reduction of the held reproject() result's counts to one record per 8x8
        tile; a pixel is short when its count is below min_count."""
        self._check(self._L.rt_reach_tiles(self._h, float(min_count)))

    def read_tile_reach(self):
        """rt_read_tile_reach: one TILE_REACH_DTYPE record per 8x8 tile, row-major."""
        n = ctypes.c_int()
        self._check(self._L.rt_read_tile_reach(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=TILE_REACH_DTYPE)
        self._check(self._L.rt_read_tile_reach(self._h, out.ctypes.data_as(ctypes.POINTER(_lib.RtTileReach)), n.value,
                                               ctypes.byref(n)))
        return out

    # -- the moved view rendered to a noise target (rt.h rt_noise_tiles / rt_render_moved_to_noise)
    def noise_tiles(self, min_count=2.0):
        """rt_noise_tiles: queue the reduction of the held reproject() result and its s2 to one noise record per
        8x8 tile; a good pixel is thin when its variance is unknown or its count is below min_count."""
        self._check(self._L.rt_noise_tiles(self._h, float(min_count)))

    def read_tile_noise(self):
        """rt_read_tile_noise: one TILE_NOISE_DTYPE record per 8x8 tile, row-major."""
        n = ctypes.c_int()
        self._check(self._L.rt_read_tile_noise(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, dtype=TILE_NOISE_DTYPE)
        self._check(self._L.rt_read_tile_noise(self._h, out.ctypes.data_as(ctypes.POINTER(_lib.RtTileNoise)), n.value,
                                               ctypes.byref(n)))
        return out

    def render_moved(self, camera, rand_factors, source=None, exposure=1.0, keep_float=False, cos_min=None, kz=None,
                     max_history=None, levels=None, k=None, guides=True, refine=None, noise_refine=None):
        """rt_render_moved + rt_read_presented: one pose of a moving camera -> [H, W, 4] uint8.  Captures the
        history, moves to `camera` (28 floats), renders len(rand_factors) frames from frame 1 and the features,
        reprojects, filters (under set_history_variance()) and presents.  source None: the library's choice
        ("moved" under set_history_variance(), else "reprojected") unless exposure or keep_float ask for
        parameters, then the same choice made here.  The other arguments are reproject()'s and denoise_reprojected()'s.
        refine: a dict of extra_frames and optionally min_count, min_pixels, max_tiles = rt_render_moved_refined ->
        (frame, tiles refined): the last extra_frames of rand_factors go to the tiles the history does not reach.
        noise_refine: a dict of target_noise and optionally batch_frames (1), max_rounds (4), min_count (0: automatic)
        = rt_render_moved_to_noise -> (frame, info): the last batch_frames * max_rounds of rand_factors go, round by
        round, to the tiles that have not met the target; info holds rounds_done, tiles_refined, tile_frames_spent
        and the final stats (sum_v, sum_y, known, thin, bad, pixels, rounds, converged, noise)."""
        if refine is not None and noise_refine is not None:
            raise ValueError("refine and noise_refine do not combine")
        cam = np.ascontiguousarray(camera, dtype=np.float32).ravel()
        assert cam.size == 28
        rf = np.ascontiguousarray(rand_factors, dtype=np.float32)
        if source is None and float(exposure) == 1.0 and not keep_float:
            pp = None
        else:
            src = source if source is not None else ("moved" if getattr(self, "_history_variance", False) else "reprojected")
            pp = _present_params(src, exposure, keep_float)
        g = (0.0, 0.0, 0.0) if guides is None or guides is False else guides
        if noise_refine is not None:
            nr = _noise_refine_params(noise_refine)
            n = int(rf.size) - max(nr.batch_frames, 0) * max(nr.max_rounds, 0)
            if n < 1:
                raise ValueError("rand_factors holds the pose's frames and then batch_frames * max_rounds more")
            rounds, tiles, spent, stats = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), _lib.RtMovedNoiseStats()
            self._check(self._L.rt_render_moved_to_noise(self._h, cam.ctypes.data_as(c_float_p), n, rf.ctypes.data_as(c_float_p),
                                                         ctypes.byref(nr), _reproject_params(cos_min, kz, max_history),
                                                         _denoise_params(levels, k), _guide_params(g), pp,
                                                         ctypes.byref(rounds), ctypes.byref(tiles), ctypes.byref(spent),
                                                         ctypes.byref(stats)))
            info = dict(rounds_done=rounds.value, tiles_refined=tiles.value, tile_frames_spent=spent.value)
            info.update(stats.as_dict())
            return self.read_presented(), info
        if refine is not None:
            rp = _refine_params(refine)
            n = int(rf.size) - max(rp.extra_frames, 0)
            if n < 1:
                raise ValueError("rand_factors holds the pose's frames and then extra_frames more")
            tiles = ctypes.c_int()
            self._check(self._L.rt_render_moved_refined(self._h, cam.ctypes.data_as(c_float_p), n, rf.ctypes.data_as(c_float_p),
                                                        ctypes.byref(rp), _reproject_params(cos_min, kz, max_history),
                                                        _denoise_params(levels, k), _guide_params(g), pp,
                                                        ctypes.byref(tiles)))
            return self.read_presented(), tiles.value
        self._check(self._L.rt_render_moved(self._h, cam.ctypes.data_as(c_float_p), int(rf.size), rf.ctypes.data_as(c_float_p),
                                            _reproject_params(cos_min, kz, max_history), _denoise_params(levels, k),
                                            _guide_params(g), pp))
        return self.read_presented()

    def read_samples(self):
        """rt_debug_read_samples: the last launch's staged colours, [n_frames, local_rows, W, 4]."""
        n = ctypes.c_int()
        self._check(self._L.rt_debug_read_samples(self._h, None, 0, ctypes.byref(n)))
        out = np.empty((n.value, self.local_rows, self.width, 4), dtype=np.float32)
        self._check(self._L.rt_debug_read_samples(self._h, out.ctypes.data_as(c_float_p), out.size, ctypes.byref(n)))
        return out

    # -- RCCL behind the ABI (rt.h rt_comm_*): one process per GPU
    def comm_init(self, uid, rank, world):
        """rt_comm_init with the 128-byte id rank 0 made (comm_unique_id)."""
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        self._check(self._L.rt_comm_init(self._h, buf, int(rank), int(world)))

    def comm_set_timeout(self, timeout_ms):
        """rt_comm_set_timeout: deadline of comm_init / gather_image in ms (0 = none); past it the
        call raises RTError(RT_ERR_TIMEOUT) with the communicator aborted."""
        self._check(self._L.rt_comm_set_timeout(self._h, int(timeout_ms)))

    def comm_abort(self):
        """rt_comm_abort: abort the communicator and free its queued work."""
        self._check(self._L.rt_comm_abort(self._h))

    def gather_image(self):
        """rt_gather_image: the full [H, W, 4] image on rank 0 (None on the other ranks)."""
        if self.rank == 0:
            out = np.empty((self.height, self.width, 4), dtype=np.float32)
            self._check(self._L.rt_gather_image(self._h, out.ctypes.data_as(c_float_p)))
            return out
        self._check(self._L.rt_gather_image(self._h, None))
        return None

    def gather_path(self):
        """How the last gather ran: 'host', 'peer' (device copies) or 'rccl' (None before any)."""
        return {0: "host", 1: "peer", 2: "rccl"}.get(self._L.rt_gather_path(self._h))

    def bind_device_image(self, ptr, nbytes):
        self._check(self._L.rt_bind_device_image(self._h, ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes)))

    def set_stream(self, stream_ptr):
        self._check(self._L.rt_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RaytraceExecutor:
    """J/system/RaytraceExecutor.java over an rt_ctx.

    One reference ``raytrace()`` = one dispatch = one frame (1 spp) per vsync;
    here ``raytrace(n)`` queues n frames in one rt_render call, with the same
    per-frame uniforms (frame_count = ++numSamples, u_rand_factor).
    """

    def __init__(self, ctx: RenderContext, seed=1):
        self.ctx = ctx
        self.seed = seed
        self._listeners = []
        self.samplePerPixel = 0
        self.resetCompleteState()
        self.lastDispatchTime = 0

    def setSamplePerPixel(self, spp):            # :50-56
        self.samplePerPixel = int(spp)
        self.ctx.set_params(spp=spp)

    def resetCompleteState(self):                # :58-62
        self.isSampleComplete = False
        self.numSamples = 0
        self.finishTime = -1

    def getNumSamples(self):
        return self.numSamples

    def getSamplePerPixel(self):
        return self.samplePerPixel

    def getFinishTime(self):
        return self.finishTime

    def getFinishTimeString(self):               # :76-89
        ms = self.finishTime
        hours, minutes, seconds = ms // 3600000, (ms // 60000) % 60, (ms // 1000) % 60
        s = (f"{hours}hour " if hours > 0 else "") + (f"{minutes}minutes " if minutes > 0 else "")
        return s + f"{seconds}.{ms % 1000}seconds"

    def getLastDispatchTime(self):
        return self.lastDispatchTime

    def addCompleteListener(self, fn):           # :96-98
        self._listeners.append(fn)

    def raytrace(self, n_frames=1):              # :100-142
        if self.numSamples == 0:
            self._start = time.time()
        # the previous call's device time once it is available, without waiting (:106-115)
        done = self.ctx.render_done() if self.numSamples else None
        if done is not None:
            self.lastDispatchTime = done // 1_000_000
        n = max(0, min(int(n_frames), self.samplePerPixel - self.numSamples)) if self.samplePerPixel else int(n_frames)
        if n == 0:
            return
        rf = frame_rand_factors(self.seed, self.numSamples, n)
        self.ctx.render(self.numSamples + 1, rf)
        self.numSamples += n

    def raytraceUntil(self, noise, batch=16):
        """Frames in batches of `batch` until the context's noise figure (rt_noise) is at most
        `noise`, or samplePerPixel frames are done (no reference counterpart; the context needs
        set_moments()).  Continues after numSamples; returns the last batch's noise dict, whose
        'converged' says which of the two ended it."""
        if self.numSamples == 0:
            self._start = time.time()
        left = self.samplePerPixel - self.numSamples
        if left <= 0:
            raise ValueError("raytraceUntil: setSamplePerPixel is the cap and it is reached")
        done, stats = self.ctx.render_until(noise, left, batch, seed=self.seed, first_frame=self.numSamples + 1)
        self.numSamples += done
        if stats["converged"]:
            self.samplePerPixel = self.numSamples   # sampleComplete() then runs the listeners
        return stats

    def raytraceAdaptive(self, noise, batch=16, min_frames=16):
        """raytraceUntil with the per-tile stopping rule (rt_render_adaptive): a tile stops once it holds
        at least `min_frames` frames and its own noise estimate is within `noise`; the others go on,
        up to samplePerPixel frames.  numSamples counts the longest-sampled tiles' frames."""
        if self.numSamples == 0:
            self._start = time.time()
        left = self.samplePerPixel - self.numSamples
        if left <= 0:
            raise ValueError("raytraceAdaptive: setSamplePerPixel is the cap and it is reached")
        done, stats = self.ctx.render_adaptive(noise, left, batch, min_frames=min_frames, seed=self.seed,
                                               first_frame=self.numSamples + 1)
        self.numSamples += done
        if stats["converged"]:
            self.samplePerPixel = self.numSamples
        return stats

    def sampleComplete(self):                    # :144-156
        if not self.isSampleComplete:
            self.isSampleComplete = self.numSamples >= self.samplePerPixel
            if self.isSampleComplete:
                self.ctx.sync()
                self.lastDispatchTime = self.ctx.last_render_ns() // 1_000_000
                self.finishTime = int((time.time() - self._start) * 1000)
                for fn in self._listeners:
                    fn()
        return self.isSampleComplete
