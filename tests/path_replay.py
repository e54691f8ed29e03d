"""main()'s and ray_color()'s loop (compute.glsl:298-358) in Python, over every pixel of a frame at once,
driven by an `ops` object that evaluates rt_debug_eval_shade_op rows (pyoracle.shade_rows) to result words:

    time = rand(); ray = get_ray()                                   CAMERA_RAY
    for max_depth rounds:                                            the loop, :304
        TRACE; on a miss  final = acc * background, stop             :305-308
        SHADE (scatter .. the mixture pdf); ended: final = its colour, stop; else go on with its o, d, acc
    a loop that runs out leaves final = vec3(0)                      :299
    image = (image * (frame_count - 1) + final) / frame_count        :355, in float32, alpha 1

The hit record lives across the loop's rounds (:302), so the uv a walk wrote stays until a later sphere, quad
or box side hit writes it again: the uv source is threaded from one TRACE into the SHADE after it and into the
next TRACE.  rf (the running rand_factor) and time are threaded the same way.

ops(name, rows) -> [n, 12] uint32 words of op `name` ("camera_ray", "trace", "shade").  OracleOps evaluates
them with the CPU oracle, DeviceOps with the device's own functions on a RenderContext; `record` collects the
TRACE rows a replay issued (the replay's own bounce rays, for tests/ref64_trace.py).
"""
import numpy as np

import pyoracle
from pyoracle import shade_rows

F32 = np.float32


class OracleOps:
    def __init__(self, oscene):
        self.oscene = oscene

    def __call__(self, name, rows):
        return pyoracle.eval_shade_op(self.oscene, name, rows)


class DeviceOps:
    """The device's ops on the scene a RenderContext uploaded (form 0 of each)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __call__(self, name, rows):
        from rtamd._lib import debug_eval_shade_op
        return debug_eval_shade_op(self.ctx, pyoracle.SHADE_OPS[name], 0, rows)


def _f(w):
    return np.ascontiguousarray(w).view(F32)


def sample(ops, width, height, max_depth, background, frame_count, rand_factor, record=None):
    """One frame's colour per pixel, [height, width, 3] float32: main() up to ray_color's return."""
    n = width * height
    px = np.tile(np.arange(width, dtype=F32), height)
    py = np.repeat(np.arange(height, dtype=F32), width)
    w = ops("camera_ray", shade_rows(n, px=px, py=py, rf=rand_factor, frame=frame_count))
    time, o, d, rf = _f(w[:, 0]).copy(), _f(w[:, 1:4]).copy(), _f(w[:, 4:7]).copy(), _f(w[:, 7]).copy()
    acc = np.ones((n, 3), F32)
    uvk = np.zeros(n, np.int32)
    uv = np.zeros((n, 3), F32)
    final = np.zeros((n, 3), F32)                       # a loop that runs out: vec3(0)
    bg = np.asarray(background, F32).reshape(1, 3)
    live = np.arange(n)                                 # the pixels still in the loop
    for _ in range(max_depth):
        if live.size == 0:
            break
        rows = shade_rows(live.size, o=o[live], d=d[live], time=time[live], px=px[live], py=py[live], rf=rf[live],
                          uvk=uvk[live], uv=uv[live])
        if record is not None:
            record.append(rows)
        w = ops("trace", rows)
        hit = w[:, 0] != 0
        uvk[live], uv[live], rf[live] = w[:, 3].view(np.int32), _f(w[:, 4:7]), _f(w[:, 7])
        with np.errstate(all="ignore"):
            final[live[~hit]] = acc[live[~hit]] * bg
        live, w = live[hit], w[hit]
        if live.size == 0:
            break
        rows = shade_rows(live.size, o=o[live], d=d[live], t=_f(w[:, 1]), tif=w[:, 2].view(np.int32), time=time[live],
                          px=px[live], py=py[live], rf=rf[live], acc=acc[live], uvk=uvk[live], uv=uv[live])
        w = ops("shade", rows)
        ended = w[:, 0] != 0
        rf[live] = _f(w[:, 10])
        final[live[ended]] = _f(w[ended, 1:4])
        go = live[~ended]
        o[go], d[go], acc[go] = _f(w[~ended, 1:4]), _f(w[~ended, 4:7]), _f(w[~ended, 7:10])
        live = go
    return final.reshape(height, width, 3)


def fold(image, cur, frame_count):
    """compute.glsl:355-357 in float32: (previous * (frame_count - 1) + current) / frame_count, alpha 1."""
    out = np.ones_like(image)
    with np.errstate(all="ignore"):
        prev = image[..., :3] * F32(frame_count - 1)
        out[..., :3] = (prev + cur) / F32(frame_count)
    return out


def render(ops, width, height, max_depth, background, rand_factors, first_frame=1, record=None):
    """(the image after the frames [height, width, 4], the frames' colours [frames, height, width, 3])."""
    image = np.zeros((height, width, 4), F32)
    curs = []
    for k, rf in enumerate(np.asarray(rand_factors, F32)):
        cur = sample(ops, width, height, max_depth, background, first_frame + k, rf, record)
        image = fold(image, cur, first_frame + k)
        curs.append(cur)
    return image, np.stack(curs)


def same_bits(a, b):
    """Equal bit for bit, a NaN matching any NaN (payloads are free)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
