"""One map holds the handles of the fluence grids, the exitance maps and the sensitivity grids (mer::Recorder): a handle of one family must stay
unknown to every entry point of the other two, as must a volume handle, 0 and a number never issued; the three kinds of fluence handle share
clear / render / destroy and cross-refuse their two reads; a destroyed handle is unknown to its own family; and a context that has refused all
of this still renders.  Smallest legal shapes throughout; the only launches are the 32 x 32 paths of the last step."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import test_gpu_exitance as TE

pytestmark = pytest.mark.gpu
BOX = ((-1, -1, -1), (1, 1, 1))
# family -> its entry points as (C name, call(ctx, scene, handle)); the reads with sums = False, so that the library does the refusing
ENTRY = {
    "fluence": [("mer_fluence_clear", lambda c, sc, h: c.fluence_clear(h)), ("mer_fluence_destroy", lambda c, sc, h: c.fluence_destroy(h)),
                ("mer_render_fluence", lambda c, sc, h: c.render_fluence(sc, h, 0, 1)), ("mer_fluence_read", lambda c, sc, h: c.fluence_read(h, sums=False)),
                ("mer_fluence_time_read", lambda c, sc, h: c.fluence_time_read(h, sums=False))],
    "exitance": [("mer_exitance_clear", lambda c, sc, h: c.exitance_clear(h)), ("mer_exitance_destroy", lambda c, sc, h: c.exitance_destroy(h)),
                 ("mer_render_exitance", lambda c, sc, h: c.render_exitance(sc, h, 0, 1)), ("mer_exitance_read", lambda c, sc, h: c.exitance_read(h, sums=False))],
    "sensitivity": [("mer_sensitivity_clear", lambda c, sc, h: c.sensitivity_clear(h)), ("mer_sensitivity_destroy", lambda c, sc, h: c.sensitivity_destroy(h)),
                    ("mer_render_sensitivity", lambda c, sc, h: c.render_sensitivity(sc, h, 0, 1)),
                    ("mer_sensitivity_read", lambda c, sc, h: c.sensitivity_read(h, sums=False))],
}
# the reads with sums = True: the Python front end sizes the array by the handle and refuses with the library's words
PY_READ = {"fluence": [("mer_fluence_read", lambda c, h: c.fluence_read(h)), ("mer_fluence_time_read", lambda c, h: c.fluence_time_read(h))],
           "exitance": [("mer_exitance_read", lambda c, h: c.exitance_read(h))], "sensitivity": [("mer_sensitivity_read", lambda c, h: c.sensitivity_read(h))]}


def _create(c):
    """a handle of each of the five kinds at the smallest legal shape: kind -> (family, handle)"""
    det = capi.detector_desc(P.BOUNDARY_AABB, (1, 1), 5, (0, 1, 0, 1))
    return {"collision": ("fluence", c.fluence_create((1, 1, 1), *BOX)), "track": ("fluence", c.fluence_track_create((1, 1, 1), *BOX)),
            "timed": ("fluence", c.fluence_time_create((1, 1, 1), *BOX, 1, 0.0, 1.0)), "exitance": ("exitance", c.exitance_create(P.BOUNDARY_AABB, (1, 1), 1)),
            "sensitivity": ("sensitivity", c.sensitivity_create((1, 1, 1), *BOX, det))}


def _read(c, kind, h):
    return {"collision": c.fluence_read, "track": c.fluence_read, "timed": c.fluence_time_read, "exitance": c.exitance_read,
            "sensitivity": c.sensitivity_read}[kind](h)


def _clear(c, family, h):
    {"fluence": c.fluence_clear, "exitance": c.exitance_clear, "sensitivity": c.sensitivity_clear}[family](h)


def _refused(c, call, msg):
    """the call fails with exactly msg, as the MerError and as mer_last_error"""
    with pytest.raises(capi.MerError) as e:
        call()
    assert str(e.value) == msg
    assert c.lib.mer_last_error(c.h).decode() == msg


def test_handles_do_not_cross_families():
    c = capi.Context(0)
    try:
        sc, _ = c.upload_scene(TE._base(w=32, h=32), layout=capi.LAYOUT_DENSE)      # a valid ptracer scene: a refused render is refused for its handle
        vol = c.upload_volume(np.ones((2, 2, 2), np.float32), *BOX)
        made = _create(c)
        never = max(h for _, h in made.values()) + 1000
        assert len({h for _, h in made.values()} | {vol.handle}) == 6

        def still_works(family):
            for kind, (fam, h) in made.items():
                if fam == family:
                    _clear(c, fam, h)
                    s, t = _read(c, kind, h)
                    assert not s.any() and t[0] == 0 and not t.any()

        # 1. every entry point of every family refuses every handle that is not its family's
        for family, entries in ENTRY.items():
            foreign = [h for fam, h in made.values() if fam != family] + [vol.handle, 0, never]
            for name, call in entries:
                for h in foreign:
                    _refused(c, lambda: call(c, sc, h), "%s: unknown %s handle" % (name, family))
                    still_works(family)
            for name, call in PY_READ[family]:
                for h in foreign:
                    with pytest.raises(capi.MerError) as e:
                        call(c, h)
                    assert str(e.value) == "%s: unknown %s handle" % (name, family)
        assert c.volume_download(vol).shape[:3] == (2, 2, 2)                        # the volume handle is still a volume's

        # 2. the three kinds of fluence handle: one clear / render / destroy, two reads that refuse each other's kind
        for kind in ("collision", "track", "timed"):
            h = made[kind][1]
            c.fluence_clear(h)
            other, msg = (("mer_fluence_read", "mer_fluence_read: time-resolved grid: use mer_fluence_time_read") if kind == "timed" else
                          ("mer_fluence_time_read", "mer_fluence_time_read: steady-state grid: use mer_fluence_read"))
            call = c.fluence_read if other == "mer_fluence_read" else c.fluence_time_read
            _refused(c, lambda: call(h, sums=False), msg)
            with pytest.raises(capi.MerError) as e:
                call(h)
            assert str(e.value) == msg

        # 3. destroyed: unknown to its own family
        for kind, (family, h) in made.items():
            {"fluence": c.fluence_destroy, "exitance": c.exitance_destroy, "sensitivity": c.sensitivity_destroy}[family](h)
        for kind, (family, h) in made.items():
            for name, call in ENTRY[family]:
                _refused(c, lambda: call(c, sc, h), "%s: unknown %s handle" % (name, family))

        # 4. the context is intact: new handles, one 32 x 32, 1-spp launch of each family (of each fluence kind)
        fresh = _create(c)
        assert not {h for _, h in fresh.values()} & {h for _, h in made.values()}
        for kind, (family, h) in fresh.items():
            {"fluence": c.render_fluence, "exitance": c.render_exitance, "sensitivity": c.render_sensitivity}[family](sc, h, 0, 1)
            assert _read(c, kind, h)[1][0] == 32 * 32
        for kind, (family, h) in fresh.items():
            {"fluence": c.fluence_destroy, "exitance": c.exitance_destroy, "sensitivity": c.sensitivity_destroy}[family](h)
        vol.destroy()
    finally:
        c.close()
