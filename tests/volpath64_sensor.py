"""The float64 volpath of tests/volpath64_multi.py -- a homogeneous grey medium with a Henyey-Greenstein phase function in the cube, a
constant environment, point emitters and one-sided rectangles -- started from the primary rays of tests/sensors64.py instead of the
pinhole's.  The estimator is volpath64_multi.render itself: for the duration of a call its ray generator (the module's
`ref64.pinhole_rays`) is replaced by the sensor's, which draws one aperture sample per path from a generator of its own."""
import types
import numpy as np
from tests import ref64, sensors64 as S, volpath64_multi as vm


def render(kind, points, rects, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, aperture_radius=0.0, focus_distance=1.0,
           near=1e-2, far=1e4, spp=2048, seed=0, **kw):
    """kind: sensors64.PERSPECTIVE | ORTHOGRAPHIC | THINLENS | TELECENTRIC; per-pixel mean and variance (height, width)"""
    lens = np.random.default_rng([seed, 977])

    def rays(c2w, w, h, fov, pos):
        u = lens.random((len(pos), 2)) if kind in (S.THINLENS, S.TELECENTRIC) else None
        o, d, _, _ = S.sensor_rays(kind, c2w, w, h, fov, near, far, pos, u, aperture_radius, focus_distance)
        return o, d

    shim = types.SimpleNamespace(**{k: getattr(ref64, k) for k in dir(ref64) if not k.startswith("__")})
    shim.pinhole_rays = rays
    keep = vm.ref64
    vm.ref64 = shim
    try:
        return vm.render(points, rects, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, spp=spp, seed=seed, **kw)
    finally:
        vm.ref64 = keep
