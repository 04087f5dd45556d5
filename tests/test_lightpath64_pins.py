"""The seven float64 light-path references (fluence64, fluence_time64, fluence_track64, exitance64, lightpath64, sensitivity64 and
sensitivity_array64) pinned at tiny sizes to recorded results: the draw order of their walk is a contract (tests/lightpath64.py), and the
seeded references that the CPU and GPU tests were tuned on must not move when the walk is rewritten.  No GPU.

tests/golden/lightpath64_pins.json holds, per case, the `totals` and `meas` arrays in full and, per grid or map, its sum, its sum of
squares and its sum weighted by the flat index.  `python -m tests.test_lightpath64_pins --write` records it anew from the code as it is.

The comparison: entries that count (paths, detected paths, binned exits, hit arrays) exactly; floats within 1e-12 max|recorded| over
the array -- only a re-association of float64 sums and products may differ, 1.1e-16 per operation over at most a few thousand operations
per entry.  A roulette decision flipped by such a rounding shows as a gross mismatch, not a small one."""
import json
import os
import sys
import numpy as np
import pytest
from tests import fluence64 as F
from tests import fluence_time64 as FT
from tests import fluence_track64 as FK
from tests import exitance64 as E
from tests import lightpath64 as LP
from tests import sensitivity64 as S
from tests import sensitivity_array64 as A

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lightpath64_pins.json")
KW = dict(paths=512, batches=2)
RES, MAPRES = (2, 2, 3), (3, 2)
SMALL = dict(bmin=(-0.5, -0.6, -0.7), bmax=(0.6, 0.5, 0.4))                  # a box inside the cube: deposits are dropped
BEAM = ([0.2, 0.1, -3.0], [0, 0, 1])                                          # outside, meets the cube
SLANT = ([0.2, 0.1, -3.0], [0.1, 0.05, 1.0])
INSIDE, OUTSIDE = (0.1, -0.2, 0.3), (0.3, 0.2, -2.0)
P3 = np.array([5.0, 3.0, 8.0])
SS3, SA3 = np.array([1.0, 0.8, 1.3]), np.array([0.2, 0.3, 0.1])
# which entries of a totals row count things, by the first word of the case; of a meas row: the detected paths
COUNTS = {"fluence": (0, 7), "time": (0, 7), "track": (0, 7), "lightpath": (0, 7, 14), "exitance": (0, 7, 14), "sensitivity": (0, 7, 8, 12), "array": (0, 7, 8, 12)}
MEAS_COUNTS = (3,)


def _ramp_sigma(p):
    return 0.4 + 0.8 * (p[:, 2] + 1.0)


def _albedo_grid():
    z, y, x = np.meshgrid(np.linspace(0.2, 0.9, 3), np.linspace(0.5, 1.0, 2), np.linspace(0.3, 0.8, 4), indexing="ij")
    return np.stack([z, z * y, x], -1)                                        # nodes (3, 2, 4, 3)


def _geo(o, d):
    return F.collimated(o, d, 1.0)


def _all_four():
    return dict(grid=dict(res=RES, **SMALL), tgrid=dict(res=RES, frames=3, t_min=2.0, t_bin=1.0), track=dict(res=RES, **SMALL),
                emap=dict(res=MAPRES, frames=2, t_min=2.0, t_bin=2.5, cos_min=0.3))


def _no_track():
    q = _all_four(); del q["track"]
    return q


CASES = {
    # ---- the grey family
    "fluence beam outside rr1": lambda: F.render(F.collimated(*BEAM, 5.0), 2.0, 0.5, 0.6, RES, rr_depth=1, seed=1, **KW),
    "fluence point inside small box depth 2": lambda: F.render(F.point(INSIDE, 1.5), 2.0, 0.5, 0.3, RES, max_depth=2, seed=2, **SMALL, **KW),
    "fluence point outside rr1 isotropic": lambda: F.render(F.point(OUTSIDE, 1.5), 1.5, 0.25, 0.0, RES, rr_depth=1, seed=3, **KW),
    "time beam outside n 1.33": lambda: FT.render(F.collimated(*SLANT, 5.0), 2.0, 0.5, 0.6, RES, 3, 2.0, 1.0, rif_const=1.33, seed=4, **SMALL, **KW),
    "time point inside rr1": lambda: FT.render(F.point(INSIDE, 1.5), 2.0, 0.5, -0.4, RES, 2, 0.5, 1.5, rr_depth=1, seed=5, **KW),
    "track grey beam": lambda: FK.render(F.collimated(*SLANT, 5.0), 2.0, 0.5, 0.6, RES, seed=6, **SMALL, **KW),
    "track chromatic rho": lambda: FK.render(F.collimated(*BEAM, 5.0), (1.0, 2.0, 4.0), (0.25, 0.5, 1.0), 0.6, RES, rho=1.25, rr_depth=1, seed=7, **SMALL, **KW),
    "track chromatic absorber rho 0": lambda: FK.render(F.point(INSIDE, 1.5), 0.0, (0.5, 1.0, 2.0), 0.0, RES, rho=0.0, seed=8, **KW),
    "track delta tracking": lambda: FK.render(F.point(OUTSIDE, 1.5), None, None, 0.5, RES, sigma_fn=_ramp_sigma, sigma_max=2.0, albedo=0.7, rr_depth=1, seed=9, **KW),
    "track depth 2": lambda: FK.render(F.collimated(*BEAM, 5.0), 2.0, 0.5, 0.6, RES, max_depth=2, seed=10, **KW),
    "exitance clear cube point inside counts": lambda: E.render(E.point((0.0, 0.0, 0.0), 1.5), 0.0, 0.0, 0.0, E.CUBE, MAPRES, counts=True, seed=11, **KW),
    "exitance cube beam cone frames n 1.33": lambda: E.render(F.collimated(*SLANT, 5.0), 2.0, 0.5, 0.6, E.CUBE, MAPRES, frames=3, t_min=2.0, t_bin=1.5, cos_min=0.3,
                                                              n=1.33, rr_depth=1, counts=True, seed=12, **KW),
    "exitance sphere point outside rr1": lambda: E.render(E.point(OUTSIDE, 1.5), 1.5, 0.25, 0.3, E.sphere(1.2), MAPRES, rr_depth=1, seed=13, **KW),
    "exitance sphere point inside depth 2 cone": lambda: E.render(E.point(INSIDE, 1.5), 2.0, 0.5, 0.6, E.sphere(0.9), MAPRES, frames=2, t_min=0.0, t_bin=1.0,
                                                                  cos_min=0.5, n=1.33, max_depth=2, seed=14, **KW),
    "exitance clear sphere beam": lambda: E.render(F.collimated(*BEAM, 5.0), 0.0, 0.0, 0.0, E.sphere(1.0), MAPRES, frames=2, t_min=2.0, t_bin=1.0, seed=15, **KW),
    # ---- the RGB throughput
    "lightpath single all four": lambda: LP.render(_geo(*SLANT), P3, LP.homogeneous(SS3, SA3, "single"), 0.6, n=1.33, rr_depth=1, seed=16, **_all_four(), **KW),
    "lightpath balance 0.7": lambda: LP.render(_geo(*BEAM), P3, LP.homogeneous(SS3, SA3, "balance", 0.7), 0.6, seed=17, **_no_track(), **KW),
    "lightpath single 0.7 point inside": lambda: LP.render(F.point(INSIDE, 1.0), P3, LP.homogeneous(SS3, SA3, "single", 0.7), 0.3, max_depth=2, seed=18,
                                                               **_no_track(), **KW),
    "lightpath maximum 0.7 point outside rr1": lambda: LP.render(F.point(OUTSIDE, 1.0), P3, LP.homogeneous(SS3, SA3, "maximum", 0.7), 0.5, rr_depth=1, seed=19,
                                                                     **_no_track(), **KW),
    "lightpath ramp constant albedo all four": lambda: LP.render(_geo(*SLANT), P3, LP.ramp(0.5, 4.0, (0.9, 0.6, 0.3)), 0.6, n=1.33, seed=20, **_all_four(), **KW),
    "lightpath ramp albedo grid": lambda: LP.render(F.point(INSIDE, 1.0), P3, LP.ramp(0.5, 3.0, _albedo_grid()), 0.4, rr_depth=1, seed=21, **_all_four(), **KW),
    # ---- the sensitivity family
    "sensitivity manual cone gate n 1.33": lambda: S.render(_geo(*SLANT), P3, S.manual(SS3, SA3, 1.1, 0.8), 0.5, RES, S.detector((4, 4), 5, (1, 4, 0, 3), cos_min=0.3,
                                                            t_min=2.0, t_bin=4.0), n=1.33, max_depth=20, rr_depth=100000, seed=22, **SMALL, **KW),
    "sensitivity clear": lambda: S.render(_geo(*SLANT), P3, LP.homogeneous(0.0, 0.0, "single"), 0.0, RES, S.detector((4, 4), 5, (0, 4, 0, 4)), seed=23, **SMALL, **KW),
    "sensitivity balance point outside rr1": lambda: S.render(F.point(OUTSIDE, 1.0), P3, LP.homogeneous(SS3, SA3, "balance"), 0.5, RES,
                                                              S.detector((4, 4), 4, (0, 4, 0, 4)), rr_depth=1, seed=24, **KW),
    "sensitivity maximum 0.7 depth 2": lambda: S.render(F.point(INSIDE, 1.0), P3, LP.homogeneous(SS3, SA3, "maximum", 0.7), 0.5, RES,
                                                        S.detector((4, 4), 1, (0, 4, 0, 4)), max_depth=2, seed=25, **KW),
    "sensitivity ramp albedo grid": lambda: S.render(_geo(*BEAM), P3, LP.ramp(0.5, 3.0, _albedo_grid()), 0.4, RES, S.detector((4, 4), 5, (0, 4, 0, 4), cos_min=0.2),
                                                     rr_depth=1, seed=26, **SMALL, **KW),
    "array bins gates cone n 1.33": lambda: A.render(_geo(*SLANT), P3, LP.homogeneous(SS3, SA3, "balance"), 0.5, RES, A.array((4, 4), 5, (0, 4, 0, 4), bins=(2, 2), gates=2,
                                                     cos_min=0.2, t_min=3.0, t_bin=2.0), n=1.33, seed=27, **SMALL, **KW),
    "array manual point inside rr1": lambda: A.render(F.point(INSIDE, 1.0), P3, S.manual(SS3, SA3, 1.1, 0.8), 0.5, RES, A.array((4, 4), 2, (0, 4, 1, 3), bins=(4, 1)),
                                                      rr_depth=1, seed=28, **KW),
    "array ramp": lambda: A.render(_geo(*BEAM), P3, LP.ramp(0.5, 4.0, (0.9, 0.6, 0.3)), 0.6, RES, A.array((4, 4), 5, (0, 4, 0, 4), bins=(2, 4), gates=3, t_min=2.0, t_bin=1.5),
                                   seed=29, **KW),
    "array clear": lambda: A.render(_geo(*SLANT), P3, LP.homogeneous(0.0, 0.0, "single"), 0.0, RES, A.array((4, 4), 5, (0, 4, 0, 4), bins=(1, 1)), seed=30, **KW),
}


def _named(result):
    """the arrays of a render's result by name: a dict as it is, a tuple as a0, a1, ..."""
    return dict(result) if isinstance(result, dict) else {"a%d" % i: a for i, a in enumerate(result)}


def _is_row_table(name, a):
    """the totals and meas arrays, stored in full: 2-D of a totals width, or the (..., 8) meas of the array renderer"""
    return name.endswith("totals") or (a.ndim == 2 and a.shape[1] in (8, 12, 16)) or (a.ndim == 5 and a.shape[-1] == 8)


def summary(result):
    out = {}
    for name, a in _named(result).items():
        a = np.asarray(a, np.float64)
        if _is_row_table(name, a):
            out[name] = {"shape": list(a.shape), "full": a.ravel().tolist()}
        else:
            f = a.ravel()
            out[name] = {"shape": list(a.shape), "sum": float(f.sum()), "sumsq": float((f * f).sum()), "isum": float((f * np.arange(f.size)).sum()),
                         "counts": bool(np.all(f == np.round(f)) and f.any())}
    return out


def compare(case, got, want):
    assert sorted(got) == sorted(want), (case, sorted(got), sorted(want))
    for name, w in want.items():
        g = got[name]
        assert g["shape"] == w["shape"], (case, name)
        if "full" in w:
            a, b = np.array(g["full"]).reshape(w["shape"]), np.array(w["full"]).reshape(w["shape"])
            cols = MEAS_COUNTS if a.ndim == 5 else [c for c in COUNTS[case.split()[0]] if c < a.shape[-1]]
            assert np.array_equal(a[..., cols], b[..., cols]), (case, name, "counts")
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (case, name, float(np.abs(a - b).max()), float(np.abs(b).max()))
        else:
            assert g["counts"] == w["counts"], (case, name)
            for key in ("sum", "sumsq", "isum"):
                if w["counts"]:                                               # a hit array: whole numbers, summed exactly
                    assert g[key] == w[key], (case, name, key, g[key], w[key])
                else:
                    assert abs(g[key] - w[key]) <= 1e-12 * abs(w[key]), (case, name, key, g[key], w[key])


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_cases_reach_every_branch():
    """what the pins are for: dropped deposits, misses, late and rejected exits, several measurements and a read scattering grid occur"""
    g = _golden()
    tot = lambda case, name: np.array(g[case][name]["full"]).reshape(g[case][name]["shape"])
    assert tot("fluence point inside small box depth 2", "a1")[:, 4].min() > 0
    assert tot("track chromatic rho", "a1")[:, 4:7].min() > 0
    assert tot("exitance sphere point outside rr1", "a1")[:, 4].min() > 0
    t = tot("exitance cube beam cone frames n 1.33", "a1")
    assert t[:, 8].min() > 0 and t[:, 11].min() > 0 and t[:, 14].min() > 0
    assert tot("exitance clear cube point inside counts", "a1")[:, 14].min() == KW["paths"]
    assert tot("sensitivity clear", "a1")[:, 8].min() == KW["paths"]
    m = tot("array bins gates cone n 1.33", "a2")
    assert m.shape == (2, 2, 2, 2, 8) and np.all(m[..., 3].sum(0) > 0)
    assert g["array bins gates cone n 1.33"]["a1"]["sum"] > 0 and tot("array bins gates cone n 1.33", "a3")[:, 13].min() > 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_pinned(case):
    compare(case, summary(CASES[case]()), _golden()[case])


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit("usage: python -m tests.test_lightpath64_pins --write")
    with open(GOLDEN, "w") as f:
        json.dump({case: summary(CASES[case]()) for case in sorted(CASES)}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
