"""The device memory of a context is reused from render to render and freed with the context (DeviceBuffer, mer_internal.hpp): the pools of a
pipeline grow and are never shrunk, so a render may find them larger than it needs, holding another render's records.  None of that may show:

 1. one long-lived context renders a sequence that grows the pool, runs small inside the larger pool over stale records, parks K_connect states,
    sorts the march lists (first use and reuse of the sort buffers and keys), walks inline, and ends with the per-path golden of
    test_gpu_kevent_handover.py -- and each step gives what a context created for that step alone gives;
 2. eight contexts, one after another, each closed with every handle still alive (volume with records and spline coefficients, envmap, one recorder
    of each family), behave alike;
 3. a refused upload and a refused spline build leave the context as it was.

Only the public Python API is used: the file pins behaviour that the parent of the commit that added it already had.  Shapes, spp and seeds are those
of test_gpu_kevent_handover.py (24^3 grids, 32 x 32 film, 8 spp, box filter: the weight channel counts samples).

Comparisons of step k on the long-lived context against the fresh one: every work counter exactly -- under `small_pool` (nslots=1024, ksteps=4) the
split between spawned side walks and walks in the path's lane depends on the order in which waves pop the hit ring (that file's docstring), so there
the SUM of the two is compared --; the film's alpha and weight exactly; its RGB at the suite's summation-order bar (rtol 1e-5, atol 1e-6) -- under
`small_pool` as well: the parent commit's library met it there in twelve of twelve measured pairs (largest difference 1.9e-6 on values near 2.7).
"""
import os
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes
from tests import test_gpu_exitance as TE
from tests import test_gpu_kevent_handover as TK

pytestmark = pytest.mark.gpu
BOX = ((-1, -1, -1), (1, 1, 1))
SMALL_POOL = TK.CONFIGS["small_pool"]
SPLIT = ("side_walks_spawned", "side_walks_in_the_paths_lane")
POINT = dict(env_radiance=[0, 0, 0], point_position=[0.2, 0.3, -0.1], point_intensity=[1.0, 0.8, 0.5])
# (what the step exercises, scene, options)
STEPS = [
    ("small pool, first allocation", TK.SCENES["rk4"], SMALL_POOL),
    ("default options: the pool grows", TK.SCENES["rk4"], {}),
    ("small render inside the larger pool, over stale records", TK.SCENES["rk4"], SMALL_POOL),
    ("point emitter inside the medium: K_connect's parked states", lambda: scenes.curved_scene(**POINT, **TK._BOX), {}),
    ("march lists sorted by cell: sort buffers and keys, first use", TK.SCENES["rk4"], dict(march_sort=2)),
    ("... and reuse, class-major", TK.SCENES["rk4"], dict(march_sort=3, march_sort_major=1)),
    ("straight rays, gridded sigma_t: inline walks", lambda: scenes.straight_scene(**TK._BOX), {}),
]


def _render(c, make_scene, opts):
    sc, vols = c.upload_scene(make_scene())
    try:
        return TK.render_with_counters(c, sc, opts)
    finally:
        for v in vols:
            v.destroy()


def _same_render(what, got, want, opts):
    (film, cnt), (ref, cref) = got, want
    print("%s: counters %s, largest |film - fresh context's| %.3e" % (what, cnt, float(np.abs(film - ref).max())))
    for k in cnt:
        if opts is SMALL_POOL and k in SPLIT:
            continue
        assert cnt[k] == cref[k], (what, k)
    assert cnt[SPLIT[0]] + cnt[SPLIT[1]] == cref[SPLIT[0]] + cref[SPLIT[1]], what
    assert np.isfinite(film).all() and np.isfinite(ref).all(), what
    assert np.array_equal(film[..., 3:], ref[..., 3:]), what
    assert np.allclose(film[..., :3], ref[..., :3], rtol=1e-5, atol=1e-6), what


def _fresh(make_scene, opts):
    c = capi.Context(0)
    try:
        return _render(c, make_scene, opts)
    finally:
        c.close()


def test_long_lived_context_renders_what_fresh_contexts_render():
    c = capi.Context(0)
    try:
        for what, make_scene, opts in STEPS:
            _same_render(what, _render(c, make_scene, opts), _fresh(make_scene, opts), opts)
        sc, vols = c.upload_scene(TK.SCENES["rk4"]())
        paths = c.render_paths(sc, 0, seed=TK.PATH_SEED)
        for v in vols:
            v.destroy()
        assert np.array_equal(paths, np.load(os.path.join(TK.GOLDEN, "kevent_handover_paths_rk4.npy")))
    finally:
        c.close()


def _lifetime(c):
    """everything a context can own, one chunk of light paths (32 x 32 x 1 spp) into each recorder; nothing is destroyed"""
    from mitsubaer_amd import synth
    vol = c.upload_volume(synth.radial_rif(24), *BOX, layout=capi.LAYOUT_BRICK27)
    coeff = vol.build_spline().download_spline()
    c.upload_envmap(np.linspace(0.5, 2.0, 4 * 8 * 3, dtype=np.float32).reshape(4, 8, 3))
    sc, _ = c.upload_scene(TE._base(w=32, h=32), layout=capi.LAYOUT_DENSE)
    det = capi.detector_desc(P.BOUNDARY_AABB, (1, 1), 5, (0, 1, 0, 1))
    out = [coeff]
    for h, render, read in ((c.fluence_create((4, 4, 4), *BOX), c.render_fluence, c.fluence_read),
                            (c.exitance_create(P.BOUNDARY_AABB, (4, 4), 1), c.render_exitance, c.exitance_read),
                            (c.sensitivity_create((4, 4, 4), *BOX, det), c.render_sensitivity, c.sensitivity_read)):
        render(sc, h, 0, 1, seed=7)
        out += list(read(h))
    return out


def test_contexts_closed_with_live_handles_one_after_another():
    """read-backs against the first context's: the spline coefficients and the path counts (totals[0]) exactly; sums and the other totals are float64
    atomics of one set of deposits in another order: the suite's RTOL_SUM (test_gpu_exitance.py has the derivation)"""
    first = None
    for k in range(8):
        c = capi.Context(0)
        try:
            got = _lifetime(c)
        finally:
            c.close()
        if first is None:
            first = got
            assert np.isfinite(got[0]).all() and all(t[0] == 32 * 32 for t in got[2::2])
            continue
        assert np.array_equal(got[0], first[0])
        for a, b in zip(got[1:], first[1:]):
            np.testing.assert_allclose(a, b, rtol=TE.RTOL_SUM, atol=0)
        assert all(t[0] == 32 * 32 for t in got[2::2])


def test_refusals_leave_the_context_usable():
    what, make_scene, opts = STEPS[0]
    c = capi.Context(0)
    try:
        rgb = scenes.rgb_albedo(24)
        with pytest.raises(capi.MerError, match="the BRICK layouts need a 1-channel float32 grid"):
            c.upload_volume(rgb, *BOX, layout=capi.LAYOUT_BRICK27)
        vol = c.upload_volume(rgb, *BOX)
        with pytest.raises(capi.MerError, match="splinevolume needs a 1-channel float32 grid"):
            vol.build_spline()
        _same_render(what, _render(c, make_scene, opts), _fresh(make_scene, opts), opts)
    finally:
        c.close()
