"""What tests/fuzz_scenes.py draws over the 48 seeds the GPU tests use, counted without a GPU: every feature tag is present in at least 4
scenes and absent from at least 4, the feature pairs whose interaction the invariance tests are for occur at least twice, and every scene
passes the refusals that can be evaluated on the host (the emitter list, the rough boundary, the sensor, and the rules of the film, of
aggressive tracing and of Simpson restated here)."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import fuzz_scenes as F

SEEDS = range(48)
LENS = {"thinlens", "telecentric"}
BIG = {"33x40", "48x40"}


@pytest.fixture(scope="module")
def drawn():
    return [F.random_extra_scene(s) for s in SEEDS]


def test_every_tag_is_drawn_and_left_out(drawn):
    assert len(F.TAGS) == 25
    for tags in (t for _, _, t in drawn):
        assert tags <= set(F.TAGS), tags - set(F.TAGS)
    counts = {t: sum(t in tags for _, _, tags in drawn) for t in F.TAGS}
    print(counts)
    for t, n in counts.items():
        assert 4 <= n <= len(drawn) - 4, (t, n)


def _unequal_spot_and_point(p):
    w = {k: {e["sampling_weight"] for e in p.emitters if e["type"] == k} for k in (P.EMITTER_SPOT, P.EMITTER_POINT)}
    return bool(w[P.EMITTER_SPOT]) and bool(w[P.EMITTER_POINT]) and len(w[P.EMITTER_SPOT] | w[P.EMITTER_POINT]) > 1


def test_the_interacting_pairs_are_drawn(drawn):
    pairs = {
        "lens x spot": lambda p, t: t & LENS and "spot" in t,
        "lens x envmap": lambda p, t: t & LENS and "envmap" in t,
        "envmap x rectangle": lambda p, t: {"envmap", "rectangle"} <= t,
        "spot x point, unequal weights": lambda p, t: _unequal_spot_and_point(p),
        "rough x point outside": lambda p, t: {"hroughdielectric", "point_outside"} <= t,
        "sdf x curved x point": lambda p, t: "sdf" in t and p.rif_mode != P.RIF_CONST and t & {"point_inside", "point_outside"},
        "lens x more than one tile": lambda p, t: t & LENS and t & BIG,
    }
    counts = {k: sum(bool(f(p, t)) for p, _, t in drawn) for k, f in pairs.items()}
    print(counts)
    for k, n in counts.items():
        assert n >= 2, (k, n)


def test_the_rare_switches_are_drawn(drawn):
    """switches that sit behind another draw and carry no tag of their own: each value of each occurs in at least two scenes, like the pairs"""
    rough = [p for p, _, t in drawn if "hroughdielectric" in t]
    straight_grid = [p for p, _, _ in drawn if p.rif_mode == P.RIF_CONST and p.sigma_mode == P.SIGMA_GRID]
    sdf_curved = [p for p, _, t in drawn if "sdf" in t and p.rif_mode != P.RIF_CONST]
    counts = {
        "beckmann": sum(p.rough_distribution == P.MICROFACET_BECKMANN for p in rough),
        "ggx": sum(p.rough_distribution == P.MICROFACET_GGX for p in rough),
        "phong": sum(p.rough_distribution == P.MICROFACET_PHONG for p in rough),
        "alpha 0.05": sum(p.rough_alpha == 0.05 for p in rough), "alpha 0.2": sum(p.rough_alpha == 0.2 for p in rough),
        "sample_visible": sum(bool(p.rough_sample_visible) for p in rough), "sample all": sum(not p.rough_sample_visible for p in rough),
        "simpson": sum(p.method == P.METHOD_SIMPSON for p in straight_grid), "no simpson": sum(p.method != P.METHOD_SIMPSON for p in straight_grid),
        "aggressive": sum(bool(p.aggressive_tracing) for p in sdf_curved), "not aggressive": sum(not p.aggressive_tracing for p in sdf_curved),
    }
    print(counts)
    for k, n in counts.items():
        assert n >= 2, (k, n)


def test_scenes_are_reproducible_and_respect_the_refusals(drawn):
    for seed, (p, layout, tags) in zip(SEEDS, drawn):
        q, layout2, tags2 = F.random_extra_scene(seed)
        assert layout == layout2 and tags == tags2
        for k, v in p.__dict__.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, q.__dict__[k]), (seed, k)
        capi.validate_sensor(p); capi.validate_emitters(p); capi.validate_rough(p)
        assert 1 <= len(p.emitters) <= 5
        assert len({e["sampling_weight"] for e in p.emitters}) == len(p.emitters)
        assert not any(p.point_intensity) and not any(p.area_radiance)                # always through the list
        if p.modulation != P.MODULATION_NONE:
            assert p.decomposition == P.DECOMPOSITION_TRANSIENT
        if p.decomposition != P.DECOMPOSITION_NONE and p.modulation == P.MODULATION_NONE:
            assert 16 <= int(np.ceil((p.max_bound - p.min_bound) / p.bin_width)) <= 64
        if p.aggressive_tracing:
            assert p.boundary == P.BOUNDARY_SDF and p.rif_mode != P.RIF_CONST
        if p.method == P.METHOD_SIMPSON:
            assert p.rif_mode == P.RIF_CONST and p.sigma_mode == P.SIGMA_GRID
        if p.boundary == P.BOUNDARY_SDF:
            assert p.rif_mode != P.RIF_ACOUSTIC and p.sdf.shape == (32, 32, 32)
        assert layout in (capi.LAYOUT_DENSE, capi.LAYOUT_CELL8, capi.LAYOUT_BRICK27, capi.LAYOUT_AUTO)
        assert (p.width, p.height) in F.SIZES
        for v in (p.density, p.rif):
            assert v is None or max(np.asarray(v).shape[:3]) <= 16
        for e in p.emitters:
            if e["type"] == P.EMITTER_ENVMAP:
                assert e["image"].shape == (8, 16, 3) and not any(p.env_radiance)


def test_the_film_sum_test_has_its_scenes(drawn):
    """test_extra_scene_film_is_the_sum_of_its_paths takes the box-filtered one-frame scenes among seeds 0..23"""
    assert len(F.one_frame_box_seeds(range(24))) >= 6


def test_the_bounds_seeds_carry_every_tag(drawn):
    assert len(F.BOUNDS_SEEDS) == 12
    assert set().union(*(drawn[s][2] for s in F.BOUNDS_SEEDS)) == set(F.TAGS)


def test_the_leak_seeds_change_every_cached_state_from_scene_to_scene(drawn):
    """consecutive scenes of test_context_state_does_not_leak_between_scenes differ in what a context caches or keys by handle: the emitter
    table, the filter table, the envmap, the sensor and the film's channel count"""
    seq = [drawn[s][0] for s in F.LEAK_SEEDS]
    assert len(seq) == 6
    for a, b in zip(seq, seq[1:]):
        assert a.rfilter != b.rfilter and a.sensor != b.sensor and F.film_frames(a) != F.film_frames(b)
        assert [e["type"] for e in a.emitters] != [e["type"] for e in b.emitters] or [e["sampling_weight"] for e in a.emitters] != [e["sampling_weight"] for e in b.emitters]
        ea = [e for e in a.emitters if e["type"] == P.EMITTER_ENVMAP]; eb = [e for e in b.emitters if e["type"] == P.EMITTER_ENVMAP]
        assert ea or eb                                                         # a map appears, goes away, or is another upload
