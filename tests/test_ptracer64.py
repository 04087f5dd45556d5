"""tests/ptracer64.py, the float64 light tracer that judges the HIP light tracer (tests/test_gpu_ptracer.py), pinned before it judges:
(a) the once-scattered light of a collimated beam against a float64 quadrature over the beam, per pixel and in total;
(b) the same on a transient film, per frame;
(c) a point emitter against the independent float64 PATH tracer tests/volpath64_multi.py, per pixel: light tracing and path tracing are
    two estimators of one image.
The scene of (a) and (b) is shared with the GPU tests (SCENE, BEAM)."""
import numpy as np
from mitsubaer_amd import params as P
from tests import ptracer64 as pt
from tests import volpath64_multi as vm

W, H, FOV = 24, 20, 40.0
CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
SIGMA_S, SIGMA_A, G = 1.0, 0.2, 0.5
BEAM_O, BEAM_D, POWER = [0.2, 0.1, -3.0], [0.0, 0.0, 1.0], 5.0
TRANSIENT = (4.0, 9.0, 0.5)              # the once-scattered paths are 2 + s + r long: 2 (to the cube) + [0, 2] + [3.2, 3.4]
_CACHE = {}


def quadrature(transient=None):
    """the single-scattering film of the shared scene (computed once, never modified)"""
    key = transient
    if key not in _CACHE:
        q = pt.single_scatter_quadrature(pt.collimated(BEAM_O, BEAM_D, POWER), SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, transient=transient)
        q.setflags(write=False)
        _CACHE[key] = q
    return _CACHE[key]


def _batches(**kw):
    return pt.render(pt.collimated(BEAM_O, BEAM_D, POWER), SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, spp=256, batches=64, full=True, **kw)


def test_single_scattering_of_a_beam_matches_the_quadrature():
    """max_depth 3 is black (the vertex is found at depth 2 and its connection's boundary crossing is the third and last depth); 4 is the
    once-scattered light.  Measured: largest per-pixel |z| 2.38, total z 2.25; the lit pixels lie in one film row."""
    assert not pt.render(pt.collimated(BEAM_O, BEAM_D, POWER), SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, spp=16, max_depth=3)[0].any()
    q = quadrature()[..., 0]
    assert q.sum() > 0 and (q > 0).sum() >= 15
    b = _batches(seed=1, max_depth=4)[..., 0]
    m, sd = b.mean(0), b.std(0, ddof=1) / np.sqrt(len(b))
    z = np.abs(m - q) / np.where(sd > 0, sd, 1.0)
    print("per-pixel |z| max %.2f" % z.max())
    assert ((m == 0) == (q == 0)).all()
    assert (np.abs(m - q) <= 4 * sd).all(), z.max()
    tot = b.sum((1, 2))
    zt = abs(tot.mean() - q.sum()) / (tot.std(ddof=1) / np.sqrt(len(tot)))
    print("total z %.2f" % zt)
    assert zt <= 4


def test_transient_frames_match_the_quadrature():
    """per-frame totals of the once-scattered light against the quadrature restricted by s + r.  Measured: largest frame |z| 0.97 (five lit frames)"""
    q = quadrature(TRANSIENT).sum((0, 1))
    assert (q > 0).sum() >= 3 and abs(q.sum() - quadrature().sum()) < 1e-9 * q.sum()          # every path length lies inside the bounds
    b = _batches(seed=2, max_depth=4, transient=TRANSIENT).sum((1, 2))
    m, sd = b.mean(0), b.std(0, ddof=1) / np.sqrt(len(b))
    print("per-frame |z|", np.abs(m - q) / np.where(sd > 0, sd, 1.0))
    assert ((m == 0) == (q == 0)).all()
    assert (np.abs(m - q) <= 4 * sd).all()


def test_point_emitter_matches_the_float64_path_tracer():
    """a point emitter inside the cube, all scattering orders: the light tracer's film against volpath64_multi's, per pixel (at most
    1 + 1 % of the pixels beyond 4 sigma of the two estimates, and the film total within 4 sigma).  Measured: 4 of 480 pixels beyond (largest 4.9: the path tracer's 1 / r^2 emitter samples
    are heavy-tailed near the emitter's pixel), total z 0.01"""
    pos, inten = [0.3, -0.2, 0.1], 2.0
    a, va = pt.render(pt.point(pos, inten), SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, spp=512, batches=32, seed=3)
    b, vb = vm.render([(pos, inten)], [], 0.0, SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, spp=256, seed=4)
    a, va, vb = a[..., 0], va[..., 0], vb / 256
    assert b.min() > 0 and a.min() > 0
    z = np.abs(a - b) / np.sqrt(va + vb)
    print("pixels beyond 4 sigma: %d, max %.2f" % ((z > 4).sum(), z.max()))
    assert (z > 4).sum() <= 1 + 0.01 * z.size
    # the total: the light tracer's batches are independent renders; the path tracer's pixels are
    full = pt.render(pt.point(pos, inten), SIGMA_S, SIGMA_A, G, W, H, FOV, CAM, spp=512, batches=32, seed=3, full=True).sum((1, 2, 3))
    zt = abs(full.mean() - b.sum()) / np.sqrt(full.var(ddof=1) / len(full) + vb.sum())
    print("total z %.2f" % zt)
    assert zt <= 4
