"""The float64 reference of the mesh signed-distance builder (tests/mesh_sdf64.py) against closed forms, and mitsubaer_amd.meshio
(the OBJ reader and the library's refusals) -- no GPU."""
import numpy as np
import pytest
from mitsubaer_amd import meshio
from tests import mesh_sdf64 as M

RES = (17, 13, 9)
BOX = ((-1.5, -1.4, -1.3), (1.5, 1.6, 1.7))


@pytest.fixture(scope="module")
def ico():
    v, t = M.icosphere(0.9, 2)
    return v, t, M.mesh_sdf64(v, t, RES, *BOX)


def test_cube_equals_the_closed_form_box_distance():
    v, t = M.cube()
    assert t.shape == (12, 3)
    sdf, w = M.mesh_sdf64(v, t, RES, *BOX)
    ref = M.box_sdf(M.nodes(RES, *BOX))
    assert np.abs(ref).min() > 1e-3                      # no node on the surface
    err = np.abs(sdf - ref).max()
    print("cube: max |sdf - closed form| = %.3e" % err)
    assert err <= 1e-12
    assert np.abs(np.abs(w) - (ref < 0)).max() < 1e-9    # w is 1 inside, 0 outside


def test_icosphere_is_the_sphere_up_to_the_chordal_sag(ico):
    v, t, (sdf, w) = ico
    assert v.shape == (162, 3) and t.shape == (320, 3)
    r = np.linalg.norm(M.nodes(RES, *BOX), axis=-1) - 0.9
    err = np.abs(sdf - r).max()
    print("icosphere: max |sdf - (|p| - 0.9)| = %.4f" % err)
    assert err <= 0.017
    far = np.abs(r) > 0.02
    assert far.sum() > 1900 and np.array_equal(np.sign(sdf[far]), np.sign(r[far]))


def test_reversed_orientation_gives_the_same_grid(ico):
    v, t, (sdf, w) = ico
    rs, rw = M.mesh_sdf64(v, t[:, ::-1], RES, *BOX)
    assert np.array_equal(np.sign(rs), np.sign(sdf))
    assert np.abs(np.abs(rs) - np.abs(sdf)).max() <= 1e-12
    assert np.abs(rw + w).max() <= 1e-12


def test_open_cube_has_no_node_near_the_threshold():
    """the cube without its last face: the counts the GPU test relies on"""
    v, t = M.cube()
    sdf, w = M.mesh_sdf64(v, t[:-2], RES, *BOX)
    band = np.abs(np.abs(w) - 0.5) < 1e-3
    print("open cube: %d of %d nodes in the band, %d inside" % (band.sum(), band.size, (sdf < 0).sum()))
    assert band.mean() <= 0.01


# ---- meshio ----------------------------------------------------------------------------------------------
OBJ = """# a comment
mtllib nothing.mtl
o thing
v 0 0 0
v 1 0 0   # trailing comment
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1
v 0.5 0.5 1
g faces
usemtl none
s off
f 1 2 3
f 1/1 3/1 4/1
f 1/1/1 2/1/1 5/1/1
f 2//1 3//1 5//1
f -1 -2 -3
f 1 2 3 4
f 1 2 3 4 5
l 1 2
"""


def test_read_obj_forms(tmp_path):
    f = tmp_path / "m.obj"
    f.write_text(OBJ)
    v, t = meshio.read_obj(str(f))
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == (5, 3) and np.array_equal(v[4], [0.5, 0.5, 1])
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [4, 3, 2],
                          [0, 1, 2], [0, 2, 3],                  # the quad as a fan
                          [0, 1, 2], [0, 2, 3], [0, 3, 4]]       # the pentagon as a fan


def test_read_obj_relative_indices_count_the_vertices_read_so_far(tmp_path):
    f = tmp_path / "m.obj"
    f.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\nv 0 0 1\nf -1 -2 -3\n")
    _, t = meshio.read_obj(str(f))
    assert t.tolist() == [[0, 1, 2], [3, 2, 1]]


def test_validate_refusals_and_dropping():
    v, t = M.cube()
    with pytest.raises(ValueError, match="index out of range"):
        meshio.validate(v, np.vstack([t, [[0, 1, 8]]]))
    with pytest.raises(ValueError, match="index out of range"):
        meshio.validate(v, np.vstack([t, [[0, -1, 2]]]))
    bad = v.copy(); bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        meshio.validate(bad, t)
    with pytest.raises(ValueError, match="n_triangles"):
        meshio.validate(v, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError, match="no triangle left"):
        meshio.validate(np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32), [[0, 1, 2], [0, 0, 1]])      # collinear; repeated index
    v2, t2 = meshio.validate(v, np.vstack([t[:5], [[3, 3, 6]], t[5:]]))
    assert np.array_equal(t2, t) and np.array_equal(v2, v)
