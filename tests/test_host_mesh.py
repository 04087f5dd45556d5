"""Host side of --mesh-sdf without a GPU: the `obj` shape exposes its faces, the flattened scene is unchanged without the flag, the grid
the flag would build, and the refusals of `mer_render --mesh-sdf[=N]` up to the point where a device is needed."""
import os
import subprocess
import numpy as np
from mitsubaer_amd import host, meshio, params as P, volio
from tests import mesh_sdf64 as M
from tests.mesh_scenes import write_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")

def test_obj_shape_exposes_its_faces(tmp_path):
    d = str(tmp_path)
    path = write_scene(d, to_world='<transform name="toWorld"><scale x="2" y="0.5" z="1"/><translate x="0.25" y="0" z="-1"/></transform>')
    with open(os.path.join(d, "mesh.obj"), "a") as f:          # a quad in the i/j/k form with relative indices, and records to ignore
        f.write("vn 0 0 1\nvt 0 0\ns off\nf -8/1/1 -7/1/1 -5/1/1 -6/1/1\n")
    v, t = host.obj_mesh(path)
    cv, ct = M.cube()
    assert np.allclose(v, cv * [2, 0.5, 1] + [0.25, 0, -1], atol=1e-6)
    assert np.array_equal(t[:12], ct) and t[12:].tolist() == [[0, 1, 3], [0, 3, 2]]
    rv, rt = meshio.read_obj(os.path.join(d, "mesh.obj"))            # the same reader rules
    assert np.array_equal(rt, t) and np.array_equal(rv, cv)


def test_flattened_scene_without_the_flag_is_unchanged(tmp_path):
    path = write_scene(str(tmp_path), mesh=M.icosphere(0.9, 1))
    d, spp = host.flatten_xml(path)
    assert d.boundary == P.BOUNDARY_AABB and spp == 4
    v, _ = M.icosphere(0.9, 1)
    assert np.allclose(list(d.bmin), v.min(0)) and np.allclose(list(d.bmax), v.max(0))


def test_flag_takes_the_rif_grid_or_the_mesh_box(tmp_path):
    path = write_scene(str(tmp_path), extra='<boolean name="aggressivetracing" value="true"/>')
    d, g = host.flatten_xml_mesh_sdf(path, 0)
    assert d.boundary == P.BOUNDARY_SDF
    assert list(g.res) == [16, 16, 16] and g.channels == 1 and g.dtype == P.VOL_F32 and not any(g.world_to_volume)
    assert np.allclose(list(g.aabb_min), [-1.5, -1.4, -1.3]) and np.allclose(list(g.aabb_max), [1.5, 1.6, 1.7])
    step = (np.array(list(g.aabb_max)) - np.array(list(g.aabb_min))) / 15.0
    assert d.aggressive_tracing == 1 and abs(d.sdf_max_error - np.linalg.norm(step)) < 1e-6        # one voxel diagonal of the built grid
    d, g = host.flatten_xml_mesh_sdf(path, 23)
    assert list(g.res) == [23, 23, 23]                        # the cube [-1,1]^3 grown by 5 % per side: 2.2 wide, 22 cells of 0.1
    assert np.allclose(list(g.aabb_min), [-1.1] * 3, atol=1e-6) and np.allclose(list(g.aabb_max), [1.1] * 3, atol=1e-6)
    assert abs(d.sdf_max_error - 0.1 * 3 ** 0.5) < 1e-6
    path = write_scene(str(tmp_path), to_world='<transform name="toWorld"><scale x="2" y="1" z="0.5"/></transform>')
    d, g = host.flatten_xml_mesh_sdf(path, 45)                # 4.4 x 2.2 x 1.1: 44, 22, 11 cells of 0.1
    assert list(g.res) == [45, 23, 12]
    assert np.allclose(list(g.aabb_min), [-2.2, -1.1, -0.55], atol=1e-5) and np.allclose(list(g.aabb_max), [2.2, 1.1, 0.55], atol=1e-5)


def test_a_malformed_face_record_matters_to_the_flag_only(tmp_path):
    d = str(tmp_path)
    path = write_scene(d)
    with open(os.path.join(d, "mesh.obj"), "a") as f:
        f.write("f 1 x 3\n")
    dsc, _ = host.flatten_xml(path)                           # as before the faces were read: the bounding box
    assert dsc.boundary == P.BOUNDARY_AABB and np.allclose(list(dsc.bmin), [-1] * 3)
    try:
        host.flatten_xml_mesh_sdf(path, 0)
        raise AssertionError("accepted")
    except host.HostError as e:
        assert "malformed face record" in str(e)


def _run(*args):
    r = subprocess.run([MER_RENDER] + list(args), capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


def test_mer_render_refuses_what_the_flag_cannot_serve(tmp_path):
    d = str(tmp_path)
    rc, err = _run("--mesh-sdf=1", write_scene(d))
    assert rc == 2 and "between 2 and 4096" in err
    rc, err = _run("--mesh-sdf=abc", write_scene(d))
    assert rc == 2 and "between 2 and 4096" in err
    volio.write_vol(os.path.join(d, "sdf.vol"), np.ones((4, 4, 4), np.float32), [-1.5, -1.4, -1.3], [1.5, 1.6, 1.7])
    rc, err = _run("--mesh-sdf", write_scene(d, sdf="sdf.vol"))
    assert rc == 1 and "already has an `sdf` child" in err
    rc, err = _run("--mesh-sdf", write_scene(d, shape="cube"))
    assert rc == 1 and "no `obj` shape" in err
    rc, err = _run("--mesh-sdf=16", write_scene(d, medium="homogeneous"))
    assert rc == 1 and "only heterogeneousrefractive" in err
    rc, err = _run("--mesh-sdf", write_scene(d, rif=False))              # an acoustic (analytic) RIF has no grid to take: N is required
    assert rc == 1 and "--mesh-sdf=N" in err
    v, t = M.cube()
    rc, err = _run("--mesh-sdf", write_scene(d, mesh=(v, np.array([[0, 1, 9]]))))
    assert rc == 1 and "index out of range" in err
    rc, err = _run("--mesh-sdf", write_scene(d, mesh=(v, np.zeros((0, 3), int))))
    assert rc == 1 and "between 1 and 2^22 triangles" in err
