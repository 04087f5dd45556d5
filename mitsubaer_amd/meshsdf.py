"""python -m mitsubaer_amd.meshsdf mesh.obj --res NX NY NZ --box x0 y0 z0 x1 y1 z1 -o sdf.vol

Writes the signed-distance grid (negative inside) of a triangle mesh as a VOL v3 file: the file the `sdf` child of
heterogeneousrefractive reads.  The grid is built on the GPU by mer_sdf_from_mesh (include/mer.h)."""
import argparse
import sys
from . import capi, meshio, volio


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mitsubaer_amd.meshsdf", description=__doc__.split("\n\n", 1)[1])
    ap.add_argument("mesh", help="Wavefront OBJ file")
    ap.add_argument("--res", type=int, nargs=3, required=True, metavar=("NX", "NY", "NZ"))
    ap.add_argument("--box", type=float, nargs=6, required=True, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("-o", "--output", required=True, help="VOL v3 file to write")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-triangles-per-launch", type=int, default=0)
    a = ap.parse_args(argv)
    try:
        v, t = meshio.validate(*meshio.read_obj(a.mesh))
    except (OSError, ValueError) as e:
        print("meshsdf: %s: %s" % (a.mesh, e), file=sys.stderr)
        return 1
    ctx = capi.Context(a.device)
    try:
        vol = ctx.sdf_from_mesh(v, t, a.res, a.box[:3], a.box[3:], max_triangles_per_launch=a.max_triangles_per_launch)
        grid = ctx.volume_download(vol)
        vol.destroy()
    except capi.MerError as e:
        print("meshsdf: %s" % e, file=sys.stderr)
        return 1
    finally:
        ctx.close()
    volio.write_vol(a.output, grid, a.box[:3], a.box[3:])
    print("meshsdf: %d triangles -> %s (%d x %d x %d, %d nodes inside)" % (t.shape[0], a.output, a.res[0], a.res[1], a.res[2], int((grid < 0).sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
