"""TEST INFRASTRUCTURE ONLY — ctypes binding of the CPU oracle (liboracle.so).

May be imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  Never used by the product path (raytracing-book_amd/).
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "build", "liboracle.so")

_L = None


class OracleSceneDesc(ctypes.Structure):
    _fields_ = [
        ("buf", ctypes.c_void_p * 6),
        ("nbytes", ctypes.c_size_t * 6),
        ("tex_format", ctypes.c_int * 8),
        ("tex_w", ctypes.c_int * 8),
        ("tex_h", ctypes.c_int * 8),
        ("tex", ctypes.c_void_p * 8),
        ("camera", ctypes.c_float * 28),
        ("max_depth", ctypes.c_int),
        ("background", ctypes.c_float * 3),
        ("sqrt_spp", ctypes.c_float),
        ("recip_sqrt_spp", ctypes.c_float),
    ]


COUNTER_FIELDS = ["samples", "bounces", "node_visits", "sphere_tests", "quad_tests", "box_tests", "medium_tests",
                  "rand_calls", "framebuffer_bytes", "node_bytes", "prim_bytes", "material_bytes", "texel_bytes",
                  "light_bytes"]


class OracleCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in COUNTER_FIELDS]


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])


def lib():
    global _L
    if _L is None:
        if not os.path.exists(LIB):
            build()
        L = ctypes.CDLL(LIB)
        fp = ctypes.POINTER(ctypes.c_float)
        L.oracle_render.restype = ctypes.c_int
        L.oracle_render.argtypes = [ctypes.POINTER(OracleSceneDesc), ctypes.c_int, ctypes.c_int, fp, ctypes.c_int,
                                    ctypes.c_int, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(OracleCounters)]
        L.oracle_set_thread_cpus.restype = None
        L.oracle_set_thread_cpus.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        L.oracle_get_sphere_uv.argtypes = [ctypes.c_float] * 3 + [fp, fp]
        L.oracle_rand_sequence.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int, fp]
        L.oracle_eval_builtin.argtypes = [ctypes.c_int, fp, fp, fp, ctypes.c_int]
        L.oracle_perlin_turb.restype = ctypes.c_float
        L.oracle_perlin_turb.argtypes = [fp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int]
        L.oracle_hit_sphere.argtypes = [ctypes.c_void_p, ctypes.c_float, fp, fp, ctypes.c_float, ctypes.c_float,
                                        fp, fp, fp, ctypes.POINTER(ctypes.c_int)]
        L.oracle_hit_quad.argtypes = [ctypes.c_void_p, fp, fp, ctypes.c_float, ctypes.c_float, fp, fp, fp,
                                      ctypes.POINTER(ctypes.c_int)]
        L.oracle_hit_aabb.argtypes = [fp, fp, fp, ctypes.c_float, ctypes.c_float]
        ip = ctypes.POINTER(ctypes.c_int)
        L.oracle_hit_box.argtypes = [ctypes.c_void_p, fp, fp, ctypes.c_float, ctypes.c_float, fp, ip, fp]
        L.oracle_medium_boundary_hits.argtypes = [ctypes.c_void_p, ctypes.c_float, fp, fp, fp, fp]
        L.oracle_texture_bilinear.restype = None
        L.oracle_texture_bilinear.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_float, ctypes.c_float, fp]
        L.oracle_checker_parity.argtypes = [ctypes.c_float] * 4
        L.oracle_eval_op.argtypes = [ctypes.c_int, ctypes.c_void_p, fp, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.oracle_eval_shade_op.argtypes = [ctypes.POINTER(OracleSceneDesc), ctypes.c_int, fp, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_uint32)]
        _L = L
    return _L


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class OracleScene:
    """Keeps the scene bytes alive and describes them to the oracle."""

    def __init__(self, scene, max_depth=5, spp=1, background=None, uniforms=None):
        from rtamd.scene import spp_uniforms   # host-side uniform helper
        self.keep = []
        d = OracleSceneDesc()
        for b in range(6):
            data = scene.buffers[b]
            if data:
                cb = ctypes.create_string_buffer(data, len(data))
                self.keep.append(cb)
                d.buf[b] = ctypes.cast(cb, ctypes.c_void_p)
            d.nbytes[b] = len(data)
        for t in scene.textures:
            cb = ctypes.create_string_buffer(t.data, len(t.data))
            self.keep.append(cb)
            d.tex[t.slot] = ctypes.cast(cb, ctypes.c_void_p)
            d.tex_format[t.slot], d.tex_w[t.slot], d.tex_h[t.slot] = t.format, t.width, t.height
        for i in range(28):
            d.camera[i] = float(scene.camera[i])
        d.max_depth = max_depth
        bg = scene.background if background is None else background
        for i in range(3):
            d.background[i] = float(bg[i])
        d.sqrt_spp, d.recip_sqrt_spp = spp_uniforms(spp) if uniforms is None else (float(uniforms[0]),
                                                                                   float(uniforms[1]))
        self.desc = d
        self.width, self.height = scene.width, scene.height


def render(oscene, rand_factors, first_frame=1, image=None, rank=0, world=1, stripe_rows=16, nthreads=0,
           counters=False):
    """Render frames first_frame.. into `image` ([H, W, 4] float32, zero-init)."""
    L = lib()
    W, H = oscene.width, oscene.height
    if image is None:
        image = np.zeros((H, W, 4), dtype=np.float32)
    if image.shape != (H, W, 4) or image.dtype != np.float32 or not image.flags.c_contiguous:
        raise ValueError(f"oracle image must be a contiguous float32 [{H}, {W}, 4] array (full size, any rank)")
    rf = np.ascontiguousarray(rand_factors, dtype=np.float32)
    cnt = OracleCounters() if counters else None
    rc = L.oracle_render(ctypes.byref(oscene.desc), W, H, _fp(image), int(first_frame), int(rf.size), _fp(rf),
                         rank, world, stripe_rows, nthreads, ctypes.byref(cnt) if cnt is not None else None)
    if rc != 0:
        raise RuntimeError(f"oracle_render failed ({rc})")
    if counters:
        return image, {n: getattr(cnt, n) for n in COUNTER_FIELDS}
    return image


def set_thread_cpus(cpus):
    """Pin render()'s worker i to CPU cpus[i % len(cpus)]; None or [] unpins."""
    cpus = list(cpus or [])
    arr = (ctypes.c_int * max(1, len(cpus)))(*cpus)
    lib().oracle_set_thread_cpus(arr, len(cpus))


def sphere_uv(x, y, z):
    u, v = ctypes.c_float(), ctypes.c_float()
    lib().oracle_get_sphere_uv(x, y, z, ctypes.byref(u), ctypes.byref(v))
    return u.value, v.value


def rand_sequence(px, py, f, n):
    out = np.empty(n, dtype=np.float32)
    lib().oracle_rand_sequence(px, py, f, n, _fp(out))
    return out


# ---- per-operation hooks, array in / array out (rt_debug.h's rt_debug_eval_op layout, so the device's
# words compare with these directly)
OPS = {"sphere": 0, "medium_sphere": 1, "quad": 2, "box": 3, "node": 4, "perlin": 5, "sphere_uv": 6, "texture": 7}
OP_REC_BYTES = {"sphere": 48, "medium_sphere": 48, "quad": 80, "box": 480, "node": 24, "perlin": 0, "sphere_uv": 0,
                "texture": 0}
OP_ROW_F, OP_OUT_W = 12, 8
TEXTYPE_IMAGE, TEXTYPE_CHECKER = 1, 2   # texture.glsl:1-4; a texture id is type << 28 | slot << 12 | detail


def op_rows(o, d=None, tmin=0.001, tmax=3.402823e38, time=0.0, word=0):
    """[n, 12] float32 rows: o, d, tmin, tmax, time, an int word (a texture id), 2 unused."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    n = o.shape[0]
    rows = np.zeros((n, OP_ROW_F), np.float32)
    rows[:, 0:3] = o
    if d is not None:
        rows[:, 3:6] = np.asarray(d, np.float32).reshape(-1, 3)
    rows[:, 6], rows[:, 7], rows[:, 8] = tmin, tmax, time
    rows.view(np.int32)[:, 9] = np.asarray(word, np.int32)
    return rows


def eval_op(op, rows, recs=None, tex=None):
    """The oracle's result words [n, 8] uint32 of `op` (a name of OPS) over rows ([n, 12] float32); recs:
    the rows' records as bytes ([n, OP_REC_BYTES[op]] uint8 or any array of that many bytes); tex:
    (format, w, h, texel array) of slot 0 for the Perlin and texture ops."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    assert rows.shape == (n, OP_ROW_F)
    rb = None
    if OP_REC_BYTES[op]:
        rb = np.ascontiguousarray(recs).view(np.uint8).reshape(n, OP_REC_BYTES[op])
    fmt, w, h, texels = tex if tex is not None else (0, 0, 0, None)
    tb = None if texels is None else np.ascontiguousarray(texels)
    out = np.zeros((n, OP_OUT_W), np.uint32)
    rc = lib().oracle_eval_op(OPS[op], None if rb is None else rb.ctypes.data, _fp(rows), n, fmt, w, h,
                              None if tb is None else tb.ctypes.data,
                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    if rc != 0:
        raise ValueError(f"oracle_eval_op({op}) failed ({rc})")
    return out


def _f(words):
    return np.ascontiguousarray(words).view(np.float32)


def hit_spheres(spheres, rows):
    """hit_sphere per row: (hit bool [n], t float32 [n])."""
    w = eval_op("sphere", rows, spheres)
    return w[:, 0] != 0, _f(w[:, 1])


def medium_boundary_hits(spheres, rows):
    """hit_constant_medium's two boundary hits on a sphere boundary: (ok, t1, t2)."""
    w = eval_op("medium_sphere", rows, spheres)
    return w[:, 0] != 0, _f(w[:, 1]), _f(w[:, 2])


def hit_quads(quads, rows):
    """hit_quad per row: (hit, t, alpha, beta); alpha / beta are hit_record.uv."""
    w = eval_op("quad", rows, quads)
    return w[:, 0] != 0, _f(w[:, 1]), _f(w[:, 2]), _f(w[:, 3])


def hit_boxes(boxes, rows):
    """hit_box per row: (hit, t, face, alpha, beta) of the side the record ends with."""
    w = eval_op("box", rows, boxes)
    return w[:, 0] != 0, _f(w[:, 1]), w[:, 2].astype(np.int32), _f(w[:, 3]), _f(w[:, 4])


def hit_aabbs(box6, rows):
    return eval_op("node", rows, np.ascontiguousarray(box6, np.float32))[:, 0] != 0


def perlin_turbs(table, p):
    """noise_turb(p, 7) on a [256, 6] float32 table."""
    t = np.ascontiguousarray(table, np.float32)
    return _f(eval_op("perlin", op_rows(p), tex=(3, 6, 256, t))[:, 0])


def sphere_uvs(p):
    w = eval_op("sphere_uv", op_rows(p))
    return _f(w[:, 0]), _f(w[:, 1])


def texture_bilinears(fmt, w, h, texels, uv):
    """texture2D (GL_LINEAR, CLAMP_TO_EDGE) of uv [n, 2]: rgb [n, 3] float32."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    d = np.zeros((uv.shape[0], 3), np.float32)
    d[:, :2] = uv
    rows = op_rows(np.zeros((uv.shape[0], 3), np.float32), d, word=TEXTYPE_IMAGE << 28)
    return _f(eval_op("texture", rows, tex=(fmt, w, h, texels))[:, 0:3])


def checker_table(scales):
    """An R32F row of checker textures (even colour 0, odd colour 1, scale), one per entry of scales
    (at most 4096): detail k of a checker id selects entry k."""
    s = np.asarray(scales, np.float32).reshape(-1)
    t = np.zeros((s.size, 3), np.float32)
    t[:, 1] = 1.0
    t[:, 2] = s
    return (3, 3 * s.size, 1, t.reshape(-1))


def checker_rows(p, which=0):
    return op_rows(p, word=(TEXTYPE_CHECKER << 28) | np.asarray(which, np.int32))


def checker_parities(scales, p, which=0):
    """checkerboard()'s parity (0 even, 1 odd) of p [n, 3] under scale scales[which]."""
    return _f(eval_op("texture", checker_rows(p, which), tex=checker_table(scales))[:, 0]) != 0.0


# ---- the sampling, light, camera and shading operations on a scene (rt_debug.h's rt_debug_eval_shade_op
# layout: RT_SOP_* numbers, rows of 20 floats, 12 output words)
SHADE_OPS = {"rand": 0, "onb": 1, "unit_vec": 2, "medium_tail": 3, "light_pdf": 4, "light_dir": 5, "camera_ray": 6,
             "shade": 7, "trace": 8}
SOP_ROW_F, SOP_OUT_W = 20, 12
# float index of each row field (ints as their bits)
SOP_O, SOP_D, SOP_T, SOP_TIF, SOP_TIME, SOP_PX, SOP_PY, SOP_RF, SOP_ACC, SOP_UVK, SOP_UV, SOP_FRAME = \
    0, 3, 6, 7, 8, 9, 10, 11, 12, 15, 16, 19


def shade_rows(n, o=None, d=None, t=0.0, tif=0, time=0.0, px=0.0, py=0.0, rf=0.0, acc=1.0, uvk=0, uv=None, frame=1):
    """[n, 20] float32 rows of rt_debug_eval_shade_op (each argument a scalar or an array over the rows)."""
    rows = np.zeros((n, SOP_ROW_F), np.float32)
    iv = rows.view(np.int32)
    if o is not None:
        rows[:, 0:3] = np.asarray(o, np.float32).reshape(-1, 3)
    if d is not None:
        rows[:, 3:6] = np.asarray(d, np.float32).reshape(-1, 3)
    rows[:, SOP_T], rows[:, SOP_TIME], rows[:, SOP_PX], rows[:, SOP_PY], rows[:, SOP_RF] = t, time, px, py, rf
    rows[:, 12:15] = np.asarray(acc, np.float32).reshape(-1, 3) if np.ndim(acc) else acc
    iv[:, SOP_TIF], iv[:, SOP_UVK], iv[:, SOP_FRAME] = tif, uvk, frame
    if uv is not None:
        rows[:, 16:19] = np.asarray(uv, np.float32).reshape(-1, 3)
    return rows


def eval_shade_op(oscene, op, rows):
    """The oracle's result words [n, 12] uint32 of `op` (a name of SHADE_OPS) over rows on an OracleScene."""
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    assert rows.shape == (n, SOP_ROW_F)
    out = np.zeros((n, SOP_OUT_W), np.uint32)
    rc = lib().oracle_eval_shade_op(ctypes.byref(oscene.desc), SHADE_OPS[op], _fp(rows), n,
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    if rc != 0:
        raise ValueError(f"oracle_eval_shade_op({op}) failed ({rc})")
    return out


BUILTINS = {"sin": 0, "cos": 1, "log": 2, "acos": 3, "atan2": 4, "fract": 5, "sqrt": 6, "inversesqrt": 7}


def eval_builtin(name, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    yy = None if y is None else np.ascontiguousarray(y, dtype=np.float32)
    lib().oracle_eval_builtin(BUILTINS[name], _fp(x), None if yy is None else _fp(yy), _fp(out), x.size)
    return out
