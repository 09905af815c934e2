"""Float64 restatement of the reference's per-vertex Phong light (Sim3DR/lighting.py:9-62, `RenderPipeline.__call__` up
to the raster), taking every `RenderPipeline` keyword. The yardstick of tests/test_gpu_normals_light_paths.py.

It consumes float32 inputs -- the vertices and the ORACLE's float32 normals -- and the configuration as the float32
values the reference's arithmetic sees (a Python float against a float32 array is a float32 operand in numpy), and does
every operation from there on in float64. So its distance from a float32 run of the same formula is that run's own
rounding, nothing else. Where the formula has no value (0/0 on a collapsed mesh or a vertex on the light, a negative base
under a fractional exponent) the result is NaN, as numpy's is: the callers compare only where it is finite.
"""
import numpy as np


def _f32(x):
    return np.asarray(np.asarray(x, dtype=np.float32), dtype=np.float64)


def norm_vertices_f64(vertices):
    """lighting.py:9-14 on a float64 copy."""
    v = np.array(vertices, dtype=np.float64)
    v -= v.min(0)[None, :]
    v /= v.max()
    v *= 2
    v -= v.max(0)[None, :] / 2
    return v


def phong_light_f64(normal, vertices, ambient=0.3, directional=0.6, specular=0.1, specular_exp=5, color_ambient=(1, 1, 1),
                    color_directional=(1, 1, 1), light_pos=(0, 0, 5), view_pos=(0, 0, 5), return_cos=False):
    """vertices, normal [nver,3] float32 -> light [nver,3] float64 (and the float64 `cos` [nver] behind the
    `cos != 0` gate of lighting.py:60; NaN where the directional term is skipped)."""
    assert normal.dtype == np.float32 and vertices.dtype == np.float32
    n = normal.astype(np.float64)
    ia, idr, isp = (float(_f32(x)) for x in (ambient, directional, specular))
    ca, cd, lp, vp = (_f32(x)[None, :] for x in (color_ambient, color_directional, light_pos, view_pos))
    unit = lambda a: a / np.sqrt(np.sum(a**2, axis=1))[:, None]  # noqa: E731  lighting.py:6
    light = np.zeros(vertices.shape, dtype=np.float64)
    cos = np.full((vertices.shape[0], 1), np.nan)
    with np.errstate(all="ignore"):
        if ia > 0:
            light += ia * ca
        vn = norm_vertices_f64(vertices)
        if idr > 0:
            direction = unit(lp - vn)
            cos = np.sum(n * direction, axis=1)[:, None]
            light += idr * (cd * np.clip(cos, 0, 1))
            if isp > 0:
                v2v = unit(vp - vn)
                reflection = 2 * cos * n - direction
                spe = np.sum((v2v * reflection) ** float(specular_exp), axis=1)[:, None]
                spe = np.where(cos != 0, np.clip(spe, 0, 1), np.zeros_like(spe))
                light += isp * cd * np.clip(spe, 0, 1)
        light = np.clip(light, 0, 1)
    return (light, cos[:, 0]) if return_cos else light


LIGHT_TOL = 2e-5       # the project's allowance for the float32 light against the reference formula
NP32_QUIET = 5e-6      # numpy-float32's own distance from float64 stays below this on ordinary meshes (about 1e-6) ...
NP32_FACTOR = 4.0      # ... where it does not, the kernel gets this many times numpy's distance: its powf and its product
                       # chain are within an ulp per term like numpy's, so it may be as far off as numpy, not much further
COS_UNDECIDED = 1e-6   # float64 |cos| below this and nonzero: the `cos != 0` gate of lighting.py:60 is a coin toss in float32


def light_error_report(gpu, normal, vertices, mask=None, **cfg):
    """One image's light [nver,3] from the GPU against the float64 restatement, per vertex, wherever the restatement and
    the float32 numpy statement are both finite (where either is not, the reference's own output is garbage) and the
    `cos != 0` gate is decided; `mask` [nver] restricts the rows further. Returns the figures and the tolerance they are
    held to; the caller asserts `gpu_err <= tol`."""
    from oracle.sim3dr_ref import phong_light_ref

    with np.errstate(all="ignore"):
        ref64, cos = phong_light_f64(normal, vertices, return_cos=True, **cfg)
        ref32 = phong_light_ref(normal, vertices, **cfg)
    finite = np.isfinite(ref64).all(1) & np.isfinite(ref32).all(1)
    if mask is not None:
        finite &= mask
    undecided = finite & (cos != 0) & (np.abs(cos) < COS_UNDECIDED)
    keep = finite & ~undecided
    np32_err = float(np.abs(ref32[keep] - ref64[keep]).max()) if keep.any() else 0.0
    gpu_err = float(np.abs(gpu[keep].astype(np.float64) - ref64[keep]).max()) if keep.any() else 0.0
    tol = LIGHT_TOL if np32_err <= NP32_QUIET else NP32_FACTOR * np32_err
    return dict(gpu_err=gpu_err, np32_err=np32_err, tol=tol, kept=int(keep.sum()), left_out=int(undecided.sum()),
                not_finite=int((~finite).sum()))
