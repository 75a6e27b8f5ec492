"""Which kernels the scenes of tests/variant_scenes.py reach, decided on the CPU with the planner's own source (tests/plan_probe.py):
every k_shade instantiation, every traversal key the planner can yield (or the relation among prepare_scene's facts that rules it out),
the edges of the three LDS budgets and of the shading classes.  tests/test_gpu_variants.py then renders the same scenes on the GPU.

    python -m pytest tests/test_variant_census.py -q -s      prints the table: kernel -> scene (DESIGN.md holds a copy)
"""
import plan_probe as pp
import variant_scenes as vs

# Traversal keys of the reachable set (tests/kernel_choice_sweep.h) that no accepted scene is given, each with the relation among
# prepare_scene's facts that no scene satisfies.  The census asserts that this is exactly the set VARIANTS leaves uncovered.
#
# Empty: every key has a scene.  Two families looked contradictory and are not.  Long walks next to scene staging want a stack of >= 12 KB
# beside the scene in 20 KB; a BLAS need not be balanced, though: the area-median split peels one triangle off per level where the
# areas fall by more than half, so 15 triangles make 12 levels (variant_scenes.chain_mesh), and a chain of far objects does the same to an
# unscanned TLAS.  Long walks next to scene staging over a SCANNED TLAS (and long walks without wide nodes inside the guarded range): an
# instanced BLAS of 12 levels has 6 wide levels >= PBRS_WIDE_MIN_LEVELS, hence wide_shadow and no staging — but scene_levels counts the
# listed meshes too, so a deep mesh that no instance enters (the `spare_mesh` axis) makes the walks "long" without wide nodes.
UNREACHABLE = {}


def plans():
    return {name: (vs.scene(name),) + vs.plan(name) for name in vs.VARIANTS}


def shade_census():
    table = {}
    for key in pp.shade_keys():
        table[key] = [name for name, (_, _, c) in plans().items() if any(s[:3] == key for s in c[pp.INTEGRATORS[key[0]]]["shade"])]
    return table


def traversal_census():
    table = {k: [] for k in pp.reachable_keys()}
    for name, (_, _, c) in plans().items():
        for k in pp.planned_keys(c):
            table.setdefault(k, []).append(name)
    return table


def test_the_probe_names_the_21_k_shade_instantiations():
    keys = pp.shade_keys()
    assert len(keys) == 21 and len(set(keys)) == 21, keys


def test_every_k_shade_instantiation_is_chosen_by_its_integrator_for_some_scene():
    table = shade_census()
    print()
    for key, names in table.items():
        print(f"k_shade {pp.shade_name(key):72s} {names[0] if names else '-'}")
    missing = [pp.shade_name(k) for k, names in table.items() if not names]
    assert not missing, missing
    print(f"{len(table) - len(missing)} of {len(table)} k_shade keys covered by {len(vs.VARIANTS)} scenes")


def test_every_reachable_traversal_key_is_chosen_for_some_scene_or_ruled_out():
    table = traversal_census()
    reachable = set(pp.reachable_keys())
    print()
    for (which, key), names in sorted(table.items()):
        print(f"k_{which:12s} {key:4d} {pp.feature_names(key):48s} {names[0] if names else 'UNREACHABLE'}")
    # the sweep bounds the planner from above: no scene is given a key outside it
    assert set(table) == reachable, sorted(set(table) - reachable)
    uncovered = {k for k, names in table.items() if not names}
    assert uncovered == set(UNREACHABLE), (sorted(uncovered - set(UNREACHABLE)), sorted(set(UNREACHABLE) - uncovered))
    for k, why in UNREACHABLE.items():
        assert len(why) > 80, (k, why)  # a relation among the facts, spelt out
    print(f"{len(reachable) - len(uncovered)} of {len(reachable)} traversal keys covered, {len(uncovered)} ruled out")


def _pair(what):
    a, b = vs.BOUNDARY_PAIRS[what]
    xa, xb = dict(vs.DEFAULTS, **vs.VARIANTS[a]), dict(vs.DEFAULTS, **vs.VARIANTS[b])
    differ = [k for k in xa if xa[k] != xb[k]]
    assert len(differ) == 1 and xb[differ[0]] == xa[differ[0]] + 1, (what, differ)  # the next-larger sibling: one more instance, material or triangle
    return plans()[a][1:], plans()[b][1:]


def test_scene_staging_budget_has_a_scene_on_either_side():
    (fa, ca), (fb, cb) = _pair("scene")
    for f in (fa, fb):  # nothing else keeps the scene out of LDS
        assert not f["full_steps"] and not ca["wide_shadow"] and not cb["wide_shadow"]
    assert fa["stack_bytes"] + fa["scene_bytes"] <= pp.SCENE_BUDGET < fb["stack_bytes"] + fb["scene_bytes"]
    assert ca["lds_staging"] == pp.LDS_SCENE and ca["extend"][0] & pp.LDS_SCENE and ca["shadow"][0] & pp.LDS_SCENE
    assert ca["extend"][1] == ca["shadow"][1] == fa["stack_bytes"] + fa["scene_bytes"]  # the kernel's dynamic LDS
    assert cb["lds_staging"] != pp.LDS_SCENE and not cb["extend"][0] & pp.LDS_SCENE and not cb["shadow"][0] & pp.LDS_SCENE


def test_tlas_staging_budget_has_a_scene_on_either_side():
    (fa, ca), (fb, cb) = _pair("top")
    for f in (fa, fb):
        assert not f["tlas_scanned"] and not f["full_steps"] and f["stack_bytes"] + f["scene_bytes"] > pp.SCENE_BUDGET
    assert fa["stack_bytes"] + fa["top_bytes"] + 512 <= pp.TOP_BUDGET < fb["stack_bytes"] + fb["top_bytes"] + 512
    assert ca["lds_staging"] == pp.LDS_TOP and ca["extend"][0] & pp.LDS_TOP and ca["shadow"][0] & pp.LDS_TOP
    assert ca["extend"][1] == ca["shadow"][1] == fa["stack_bytes"] + fa["top_bytes"]
    assert cb["lds_staging"] == 0 and not cb["extend"][0] & (pp.LDS_TOP | pp.LDS_SCENE) and cb["extend"][1] == fb["stack_bytes"]  # an unscanned TLAS too large for LDS


def test_k_shade_budget_has_a_scene_on_either_side_of_both_steps():
    (fa, ca), (fb, cb) = _pair("shade_all")  # ALL -> RECORDS: one more triangle
    assert fa["shade_rec_bytes"] + fa["shade_tri_bytes"] <= pp.SHADE_BUDGET < fb["shade_rec_bytes"] + fb["shade_tri_bytes"] and fb["shade_rec_bytes"] <= pp.SHADE_BUDGET
    (sa,), (sb,) = ca["path"]["shade"], cb["path"]["shade"]
    assert sa[2] & pp.SHADE_LDS_ALL == pp.SHADE_LDS_ALL and sa[3] == fa["shade_rec_bytes"] + fa["shade_tri_bytes"]
    assert sb[2] & pp.SHADE_LDS_ALL == pp.SHADE_LDS_RECORDS and sb[3] == fb["shade_rec_bytes"]
    (fa, ca), (fb, cb) = _pair("shade_records")  # RECORDS -> none: one more material
    assert fa["shade_rec_bytes"] <= pp.SHADE_BUDGET < fb["shade_rec_bytes"] and fa["shade_rec_bytes"] + fa["shade_tri_bytes"] > pp.SHADE_BUDGET
    (sa,), (sb,) = ca["path"]["shade"], cb["path"]["shade"]
    assert sa[2] & pp.SHADE_LDS_ALL == pp.SHADE_LDS_RECORDS and sa[3] == fa["shade_rec_bytes"]
    assert sb[2] & pp.SHADE_LDS_ALL == 0 and sb[3] == 0


def _scenes_where(pred):
    return [name for name, (_, f, c) in plans().items() if pred(f, c)]


def test_class_edges_have_scenes():
    every_class_on_an_instance = lambda f: f["max_instance_class"] == min(f["n_signatures"], pp.MAX_CLASSES - 1)  # noqa: E731
    for n in (14, 15):
        assert _scenes_where(lambda f, c: f["n_signatures"] == n and f["n_classes"] == n and every_class_on_an_instance(f)), n
    assert _scenes_where(lambda f, c: f["n_signatures"] >= 16 and f["n_classes"] == 15 and every_class_on_an_instance(f))
    # the overflow class (15) holds two different signatures, both on instances
    assert _scenes_where(lambda f, c: f["overflow_signatures"] >= 2 and f["max_instance_class"] == 15)
    # the Lambert signature at the last position that counts: the path integrator's queue goes class-major with class 14 last ...
    assert _scenes_where(lambda f, c: f["lambert_position"] == 14 and f["lambert_class"] == 14 and c["path"]["order"] == 2 and c["path"]["last_class"] == 14 and
                         c["path"]["shade"][0][2] & pp.SHADE_LAMBERT and c["path"]["shade"][0][4] == 14)
    # ... and at the first that does not: ignored, one general launch over the sorted queue
    assert _scenes_where(lambda f, c: f["lambert_position"] == 15 and f["lambert_class"] == 0 and not f["textured"] and not f["fourier"] and
                         c["path"]["order"] == 1 and len(c["path"]["shade"]) == 1 and not c["path"]["shade"][0][2] & pp.SHADE_LAMBERT)
    # the Fourier signature likewise: class 14 gets the kernel cut down to the lobe, position 15 leaves every class to the general Fourier kernels
    assert _scenes_where(lambda f, c: f["fourier_position"] == 14 and f["fourier_class"] == 14 and all(
        c[i]["order"] == 2 and c[i]["last_class"] == 14 and c[i]["shade"][0][2] == pp.SHADE_FOURIER_ALONE for i in ("path", "direct")))
    assert _scenes_where(lambda f, c: f["fourier_position"] == 15 and f["fourier_class"] == 0 and all(
        [s[1:3] for s in c[i]["shade"]] == [(True, pp.SHADE_FOURIER)] for i in ("path", "direct")))


def test_cameras_are_small():
    for name, (sb, _, _) in plans().items():
        assert sb.camera.width <= 64 and sb.camera.height <= 48, name


def test_the_oracle_renders_every_scene_without_tlas_ties():
    """No comparison of tests/test_gpu_variants.py may be given up for coincident geometry."""
    for name, (sb, _, _) in plans().items():
        for integrator, (_, ost) in vs.reference(name).items():
            assert ost["tlas_ties"] == 0, (name, integrator)


def test_every_way_of_launching_k_shade_has_a_scene():
    """One key can be launched in more than one way: over the whole queue, over a class range of a class-major queue, over the rest."""
    def launches(c, integ):
        return [(s[1], s[2] & ~pp.SHADE_LDS_ALL, s[4]) for s in c[integ]["shade"]]
    NO_ORDER, CLASS_SORT, CLASS_MAJOR = 0, 1, 2
    # every material a Fourier BSDF: the lobe's kernel over the unordered queue, both integrators
    assert _scenes_where(lambda f, c: f["n_classes"] == 1 and f["fourier_class"] == 1 and all(
        c[i]["order"] == NO_ORDER and launches(c, i) == [(False, pp.SHADE_FOURIER_ALONE, 0)] for i in ("path", "direct")))
    # a Fourier class among others, untextured and textured: class-major, the lobe's kernel on its class, the general kernel on the rest
    for tex in (False, True):
        assert _scenes_where(lambda f, c: bool(f["textured"]) == tex and all(
            c[i]["order"] == CLASS_MAJOR and launches(c, i) == [(False, pp.SHADE_FOURIER_ALONE, f["fourier_class"]), (tex, 0, pp.MAX_CLASSES)] for i in ("path", "direct"))), tex
    # several untextured classes without a Lambert one: one general launch over the sorted queue; with one: the Lambert kernel on its class
    assert _scenes_where(lambda f, c: f["n_classes"] > 1 and not f["lambert_class"] and c["path"]["order"] == CLASS_SORT and launches(c, "path") == [(False, 0, 0)])
    for light in (0, pp.SHADE_LIGHT_SPHERE, pp.SHADE_LIGHT_TRIANGLE):
        assert _scenes_where(lambda f, c: c["path"]["order"] == CLASS_MAJOR and launches(c, "path") == [
            (False, pp.SHADE_LAMBERT | light, f["lambert_class"]), (False, 0, pp.MAX_CLASSES)]), light
    # textured scenes sort their classes too; one class sorts nothing and may split the path integrator's queue
    assert _scenes_where(lambda f, c: f["textured"] and not f["fourier"] and f["n_classes"] > 1 and all(
        c[i]["order"] == CLASS_SORT and launches(c, i) == [(True, 0, 0)] for i in ("path", "direct")))
    assert _scenes_where(lambda f, c: f["n_classes"] == 1 and c["split_queue"] and c["path"]["order"] == NO_ORDER and not f["lambert"])
    assert _scenes_where(lambda f, c: f["n_classes"] == 1 and c["split_queue"] and f["lambert"])
    assert _scenes_where(lambda f, c: f["n_classes"] > 1 and not c["split_queue"])
