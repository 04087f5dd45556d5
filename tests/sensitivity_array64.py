"""The sensitivity grids of an array of detectors and gates (mer_sensitivity_array_create, include/mer.h) restated in float64 with numpy: the
walk and the recorder of tests/sensitivity64.py (record) -- the same code, so that one seed walks the same paths in both -- with two
additions read per path:

  the measurement  a path that leaves through raster cell (iu, iv) of the window in gate g = floor((l - t_min) / t_bin), 0 <= g < gates,
                   past the cone, belongs to m = (g ndv + (iv - iv0) // bin_v) ndu + (iu - iu0) // bin_u (gates = 1 and t_bin = 0: no gate);
  the collisions   every collision the path scatters from (it survives the albedo: T.max() > 0 afterwards, as LightPath::collide returns
                   true) adds 1 to the path's row of a dense matrix N[path, cell] at the cell of the collision point, or to the path's
                   count outside the box; the path's count of all of them is kept apart, before any box test.

After the walk, per measurement: J[m] = w^T L and K[m] = w^T N over the paths of m.

Returns J and K (batches, gates, ndv, ndu, nz, ny, nx, 3), meas (batches, gates, ndv, ndu, 8: detected weight x 3, detected paths,
w x collisions x 3, 0) and totals (batches, 16: as sensitivity64.render over all measurements; [13..15] w per collision outside the box)."""
from tests import sensitivity64 as S
from tests.sensitivity64 import shape


def array(res, face, window, bins=None, gates=1, cos_min=0.0, t_min=0.0, t_bin=0.0):
    """the detector dict of sensitivity64.detector plus bins = (bin_u, bin_v) (None: the whole window) and the gates"""
    d = S.detector(res, face, window, cos_min, t_min, t_bin)
    iu0, iu1, iv0, iv1 = d["window"]
    d["bins"] = (iu1 - iu0, iv1 - iv0) if bins is None else tuple(int(v) for v in bins)
    d["gates"] = int(gates)
    assert (iu1 - iu0) % d["bins"][0] == 0 and (iv1 - iv0) % d["bins"][1] == 0 and gates >= 1 and (gates == 1 or t_bin > 0)
    return d


def render(emitter, power, medium, g, res, det, bmin=(-1, -1, -1), bmax=(1, 1, 1), n=1.0, paths=4096, batches=16, seed=0, max_depth=-1,
           rr_depth=5, max_events=4096):
    """`batches` independent batches of `paths` paths: (J, K, meas, totals), raw sums as the library keeps them"""
    rec = S.record(emitter, power, medium, g, res, det, bmin, bmax, True, n=n, paths=paths, batches=batches, seed=seed, max_depth=max_depth,
                   rr_depth=rr_depth, max_events=max_events)
    gates, ndv, ndu = shape(det)
    grid = (batches, gates, ndv, ndu, res[2], res[1], res[0], 3)
    return rec.J.reshape(grid), rec.K.reshape(grid), rec.meas.reshape((batches, gates, ndv, ndu, 8)), rec.totals
