"""mer_sdf_from_mesh on the GPU against the float64 reference tests/mesh_sdf64.py: signs, distances and winding numbers on a cube, an
icosphere, an open and a reversed mesh; bit-identity over chunk sizes and dropped triangles; download; refusals; the
bounds-checking build; a render from the built grid; and `mer_render --mesh-sdf` against `python -m mitsubaer_amd.meshsdf`."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
from mitsubaer_amd import capi, params as P
from tests import mesh_sdf64 as M, scenes
from tests.mesh_scenes import write_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = (17, 13, 9)                                   # node tails on all three axes of a 256-thread block, a box that is no cube
BOX = ((-1.5, -1.4, -1.3), (1.5, 1.6, 1.7))
DIAG = float(np.linalg.norm(np.subtract(BOX[1], BOX[0])))            # 5.196
# Tolerances: 4 x the largest error observed on the MI355X over the cube, the icosphere, the open cube and the reversed meshes on this
# grid (the factor covers atan2f / sqrtf rounding differences between compiler versions, nothing more).
# Measured: |sdf - ref| / diagonal: cube 2.67e-8, icosphere 2.72e-8, open cube 2.87e-8, reversed 2.58e-8 / 2.25e-8 -> 2.87e-8;
#           |w - ref|: cube 3.6e-7, icosphere 1.01e-6, open cube 2.9e-7, reversed 1.01e-6 / 4.2e-7 -> 1.013e-6.
TOL_DIST = 4 * 2.87e-8 * DIAG         # |sdf - ref|, as a float32 quantity relative to the box diagonal
TOL_W = 4 * 1.013e-6                      # |w - ref|


@pytest.fixture(scope="module")
def meshes():
    """name -> (vertices, triangles, reference sdf, reference w); computed once, never modified"""
    cv, ct = M.cube(); iv, it = M.icosphere(0.9, 2)
    out = {}
    for name, (v, t) in {"cube": (cv, ct), "ico": (iv, it), "open": (cv, ct[:-2])}.items():
        s, w = M.mesh_sdf64(v, t, RES, *BOX)
        s.setflags(write=False); w.setflags(write=False)
        out[name] = (v, t, s, w)
    return out


def build(c, v, t, res=RES, box=BOX, **kw):
    vol, w = c.sdf_from_mesh(v, t, res, *box, return_winding=True, **kw)
    g = c.volume_download(vol)
    vol.destroy()
    return g, w


def check(g, w, rs, rw, where=None):
    where = np.ones(rs.shape, bool) if where is None else where
    ed = np.abs(np.abs(g) - np.abs(rs)).max(); ew = np.abs(w - rw).max()
    print("max |sdf - ref| / diag = %.3e   max |w - ref| = %.3e" % (ed / DIAG, ew))
    assert np.array_equal(np.sign(g)[where], np.sign(rs)[where])
    assert ed <= TOL_DIST and ew <= TOL_W


def test_cube(ctx, meshes):
    v, t, rs, rw = meshes["cube"]
    assert t.shape[0] == 12 and (rs < 0).sum() > 100
    check(*build(ctx, v, t), rs, rw)


def test_icosphere_and_chunking(ctx, meshes):
    v, t, rs, rw = meshes["ico"]
    assert t.shape[0] == 320
    g, w = build(ctx, v, t)
    check(g, w, rs, rw)
    g2, w2 = build(ctx, v, t, max_triangles_per_launch=100)            # four launches, a ragged last chunk
    check(g2, w2, rs, rw)
    assert np.array_equal(g, g2) and np.array_equal(w, w2)
    g3, w3 = build(ctx, v, t, max_triangles_per_launch=1)
    assert np.array_equal(g, g3) and np.array_equal(w, w3)


def test_open_mesh(ctx, meshes):
    v, t, rs, rw = meshes["open"]
    assert t.shape[0] == 10
    band = np.abs(np.abs(rw) - 0.5) < 1e-3
    assert band.mean() <= 0.01                      # the condition of this case: on this grid the reference excludes no node
    g, w = build(ctx, v, t)
    check(g, w, rs, rw, ~band)
    assert (g < 0).sum() == (rs < 0).sum() == 528


@pytest.mark.parametrize("name", ["cube", "ico"])
def test_reversed_orientation(ctx, meshes, name):
    v, t, rs, rw = meshes[name]
    g, w = build(ctx, v, t)
    gr, wr = build(ctx, v, t[:, ::-1].copy())
    assert np.array_equal(np.sign(g), np.sign(gr))
    check(gr, -wr, rs, rw)


def test_a_degenerate_triangle_changes_nothing(ctx, meshes):
    v, t, _, _ = meshes["ico"]
    g, w = build(ctx, v, t)
    v2 = np.vstack([v, [[3, 3, 3], [4, 4, 4], [5, 5, 5]]]).astype(np.float32)
    t2 = np.vstack([t[:7], [[5, 5, 9]], t[7:], [[162, 163, 164]]])         # a repeated index in the middle, a collinear triangle at the end
    g2, w2 = build(ctx, v2, t2)
    assert np.array_equal(g, g2) and np.array_equal(w, w2)


def test_download(ctx, meshes):
    v, t, _, _ = meshes["cube"]
    vol = ctx.sdf_from_mesh(v, t, RES, *BOX)
    g = ctx.volume_download(vol)
    assert g.shape == (9, 13, 17) and g.dtype == np.float32
    for layout in (capi.LAYOUT_DENSE, capi.LAYOUT_CELL8):
        up = ctx.upload_volume(g, *BOX, layout=layout)
        assert np.array_equal(ctx.volume_download(up), g)
        up.destroy()
    vol.destroy()
    # refusals: by the binding, and by the library itself through the raw call (a buffer large enough for whatever it might write)
    buf = np.zeros(4 * 4 * 4 * 3, np.float32)
    rgb = ctx.upload_volume(np.zeros((4, 4, 4, 3), np.float32), *BOX)
    u8 = ctx.upload_volume(np.zeros((4, 4, 4), np.uint8), *BOX)
    env = ctx.upload_envmap(np.ones((4, 8, 3), np.float32))
    for x, msg in ((rgb, "only a 1-channel float32 volume"), (u8, "only a 1-channel float32 volume"), (env, "envmap handle")):
        with pytest.raises(capi.MerError, match=msg):
            ctx.volume_download(x)
        assert ctx.lib.mer_volume_download(ctx.h, C.c_int32(x.handle), buf.ctypes.data_as(C.c_void_p)) != 0
        assert msg in ctx.lib.mer_last_error(ctx.h).decode() and not buf.any()
        x.destroy()


def test_refusals(ctx, meshes):
    v, t, _, _ = meshes["cube"]
    with pytest.raises(capi.MerError, match="triangle index out of range"):
        ctx.sdf_from_mesh(v, np.vstack([t, [[0, 1, 8]]]), RES, *BOX)
    bad = v.copy(); bad[2, 0] = np.nan
    with pytest.raises(capi.MerError, match="a vertex is not finite"):
        ctx.sdf_from_mesh(bad, t, RES, *BOX)
    with pytest.raises(capi.MerError, match="at least 2 nodes along every axis"):
        ctx.sdf_from_mesh(v, t, (17, 1, 9), *BOX)
    with pytest.raises(capi.MerError, match="must not be negative"):
        ctx.sdf_from_mesh(v, t, RES, *BOX, max_triangles_per_launch=-1)
    with pytest.raises(capi.MerError, match="no triangle left"):
        ctx.sdf_from_mesh(v, [[0, 0, 1], [2, 3, 3]], RES, *BOX)
    with pytest.raises(capi.MerError, match=r"n_triangles must be in \[1, 2\^22\]"):
        ctx.sdf_from_mesh(v, np.zeros((0, 3), np.int32), RES, *BOX)
    with pytest.raises(capi.MerError, match="box is empty or not finite"):
        ctx.sdf_from_mesh(v, t, RES, BOX[0], (1.5, -1.4, 1.7))
    d = ctx._desc((9, 13, 17), 1, P.VOL_F32, *BOX, to_world=np.eye(4))      # an identity matrix written out: non-zero
    h = C.c_int32()
    rc = ctx.lib.mer_sdf_from_mesh(ctx.h, C.byref(d), v.ctypes.data_as(C.c_void_p), C.c_int64(8), t.ctypes.data_as(C.c_void_p), C.c_int64(12),
                                   C.c_int32(0), C.c_int32(capi.LAYOUT_DENSE), None, C.byref(h))
    assert rc != 0 and "non-zero world_to_volume" in ctx.lib.mer_last_error(ctx.h).decode()


def test_bounds_checking_build(meshes):
    c = capi.Context(0, check=True)
    try:
        for name in ("cube", "ico"):
            v, t, rs, rw = meshes[name]
            check(*build(c, v, t), rs, rw)
            build(c, v, t, max_triangles_per_launch=100)
        enabled, violations = c.debug_bounds()[:2]
        assert enabled and violations == 0
    finally:
        c.close()


RBOX = ([-1.2] * 3, [1.2] * 3)


@pytest.fixture(scope="module")
def ico48():
    v, t = M.icosphere(0.9, 2)
    s, _ = M.mesh_sdf64(v, t, (48, 48, 48), *RBOX)
    s = s.astype(np.float32); s.setflags(write=False)
    return v, t, s


@pytest.mark.parametrize("bsdf", [P.BSDF_NULL, P.BSDF_HDIELECTRIC])
def test_render_from_the_built_grid(ctx, ico48, bsdf):
    """mer_render_paths with the GPU-built grid against the same scene with the float64 reference grid, cast to float32, uploaded from the host"""
    v, t, ref = ico48
    p = scenes.curved_scene(N=24, rif="radial", boundary=P.BOUNDARY_SDF, sdf=ref, sdf_aabb=RBOX, boundary_bsdf=bsdf)
    sc, vols = ctx.upload_scene(p)
    b = ctx.render_paths(sc, 0, seed=3)
    built = ctx.sdf_from_mesh(v, t, (48, 48, 48), *RBOX)
    sc.sdf = built.handle
    a = ctx.render_paths(sc, 0, seed=3)
    assert np.isfinite(a).all() and np.abs(b).max() > 0
    close = np.abs(a - b).max(2) <= 1e-4 * np.maximum(1.0, np.abs(b).max(2))
    print("paths within 1e-4: %.4f" % close.mean())
    assert close.mean() >= 0.99, close.mean()
    for x in vols + [built]:
        x.destroy()


def _child(args, cwd):
    """a fresh child process under its own time limit"""
    env = dict(os.environ); env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run(["timeout", "-k", "10", "120"] + args, cwd=cwd, env=env, capture_output=True, text=True)
    assert r.returncode == 0, (args, r.returncode, r.stdout, r.stderr)


def _cli_films(d, spp, flags=()):
    """film A: `mer_render --mesh-sdf`; film B: `mer_render` on the same scene with an `sdf` child written by `python -m mitsubaer_amd.meshsdf`
    from the same mesh on the same grid; 32 x 24, the same seed, every run a fresh child process"""
    mer_render = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
    os.rename(write_scene(d), os.path.join(d, "a.xml"))
    _child([mer_render, "--mesh-sdf", "-s", spp, "--seed", "7", "--raw", "-o", "a.npy", "a.xml"] + list(flags), d)
    box = [repr(float(x)) for x in (-1.5, -1.4, -1.3, 1.5, 1.6, 1.7)]
    _child([sys.executable, "-m", "mitsubaer_amd.meshsdf", "mesh.obj", "--res", "16", "16", "16", "--box"] + box + ["-o", "sdf.vol"], d)
    write_scene(d, sdf="sdf.vol")
    _child([mer_render, "-s", spp, "--seed", "7", "--raw", "-o", "b.npy", "scene.xml"] + list(flags), d)
    a = np.load(os.path.join(d, "a.npy")); b = np.load(os.path.join(d, "b.npy"))
    assert a.shape == (24, 32, 5) and a[..., :3].max() > 0
    df = np.abs(a - b)
    print("spp %s: values differing: %d of %d, max abs %.3e" % (spp, (df > 0).sum(), df.size, df.max()))
    return a, b


def test_cli_mesh_sdf_equals_the_file_route(tmp_path):
    """4 spp, same seed: bit-identical films.  The film is summed with float atomics, so two plain 4 spp runs of ONE command agree only up to
    the summation order (measured on an MI355X: `mer_render --mesh-sdf` twice: 6 of 3840 values differ, by one ulp, 2.4e-7; the sample
    counts are equal).  Both routes therefore run with `--ordered`: one render per sample index, the films added in index order, so that
    with this box filter every pixel receives one splat per pass and nothing depends on the order of the atomics.  The ordered film is the
    plain film up to that order."""
    d = str(tmp_path)
    a, b = _cli_films(d, "4", ["--ordered"])
    assert np.array_equal(a, b)
    _child([os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "-s", "4", "--seed", "7", "--raw", "-o", "c.npy", "scene.xml"], d)
    c = np.load(os.path.join(d, "c.npy"))
    assert np.array_equal(c[..., 3:], b[..., 3:]) and np.allclose(c, b, rtol=1e-5, atol=1e-6)          # the bar of tests/test_gpu_render.py for two films of one scene


def test_cli_mesh_sdf_equals_the_file_route_one_sample_per_pixel(tmp_path):
    """1 spp without `--ordered` (box filter: one sample per pixel, so no summation order): bit-identical films -- the two routes hold the same grid"""
    a, b = _cli_films(str(tmp_path), "1")
    assert np.array_equal(a, b)
