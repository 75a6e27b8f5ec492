#!/usr/bin/env python3
"""Picks tests/variant_scenes.py's VARIANTS: walks the generator's grid with the plan probe (tests/plan_probe.py, CPU only) and keeps, goal
by goal, the scene that covers the most goals still open — every reachable traversal key, every k_shade instantiation under the integrator
it names, the class edges and the boundary pairs of the three LDS budgets (tests/test_variant_census.py states them).  A scene the oracle
renders with TLAS ties is passed over.  Prints the two tables to paste into tests/variant_scenes.py.

    python tools/search_variants.py > /tmp/variants.txt
"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import plan_probe as pp  # noqa: E402
import variant_scenes as vs  # noqa: E402

import pbrs_amd  # noqa: E402
from oracle.binding import OracleScene  # noqa: E402


def name_of(axes):
    short = {"analytic": "an", "mesh": "mesh", "tangent_check": "tan", "quad": "quad", "instances": "n", "tlas_chain": "chain", "tiny": "tiny", "spare_mesh": "spare",
             "materials": "", "lights": "", "pad_triangles": "tri", "pad_materials": "mat", "seed": "seed"}
    parts = []
    for k, v in axes.items():
        if v == vs.DEFAULTS[k]:
            continue
        if k == "materials":
            parts.append(v if isinstance(v, str) else f"sig{v[1]}" + (f"_{v[2]}{v[3]}" if v[2] else ""))
        elif k == "lights":
            parts.append("+".join(v) if v else "dark")
        elif isinstance(v, bool):
            parts.append(short[k] if v else "no" + short[k])
        else:
            parts.append(f"{short[k]}{v}")
    return "_".join(parts) or "default"


def plan(axes):
    sb = vs.build(**axes)
    return sb, pp.probe(pbrs_amd.HostScene(sb))


def goals_of(facts, choice):
    g = {("key",) + k for k in pp.planned_keys(choice)}
    for integ in ("path", "direct", "materials", "normals"):
        g |= {("shade", s[0], s[1], s[2]) for s in choice[integ]["shade"]}
    # ... and every way the two integrators' shading is launched: the queue order, the kernels without their LDS bits, what each covers
    for integ in ("path", "direct"):
        ch = choice[integ]
        launches = tuple((s[1], s[2] & ~pp.SHADE_LDS_ALL, {0: "queue", pp.MAX_CLASSES: "rest"}.get(s[4], "class")) for s in ch["shade"])
        g.add(("launch", integ, ch["order"], launches, choice["split_queue"] if integ == "path" else None))
    f = facts
    g |= {("signatures", min(f["n_signatures"], 16))} if f["n_signatures"] >= 14 and f["max_instance_class"] >= min(f["n_signatures"], 15) else set()
    for what in ("lambert", "fourier"):
        if f[what + "_position"] in (14, 15):
            g.add((what + "_position", f[what + "_position"]))
    if f["overflow_signatures"] >= 2:
        g.add(("overflow", 2))
    return g


def ties(sb, choice):
    osc = OracleScene(sb)
    for integ, strata, depth in vs.RENDERS:
        _, ost = osc.render(strata[0], strata[1], depth, vs.SEED, integrator=integ)
        if ost["tlas_ties"]:
            return True
    return False


def candidates():
    geometry = []
    for analytic, mesh, tan, tiny, spare, quad in itertools.product((True, False), (None, "box", "quad", 11, 15), (False, True), (False, True), (0, 15), (False, True)):
        if (not analytic and mesh is None) or (tan and mesh is None) or (quad and (mesh is None or tan or tiny or spare)):
            continue
        geometry.append(dict(analytic=analytic, mesh=mesh, tangent_check=tan, tiny=tiny, spare_mesh=spare, quad=quad))
    counts = [dict(instances=6), dict(instances=24), dict(instances=36), dict(instances=48), dict(instances=60), dict(instances=72), dict(instances=100), dict(instances=36, tlas_chain=20), dict(instances=30, tlas_chain=8)]
    dress = [dict(materials=m, lights=l) for m, l in itertools.product(
        ("lambert", "mixed", "glossy", "one_glossy", "textured", "fourier", "fourier_mixed", "fourier_textured"),
        (("sphere",), ("triangle",), ("sphere", "disk", "triangle", "point"), ("point", "env"), ("sphere", "distant", "env")))]
    for g, c, d in itertools.product(geometry, counts, dress):
        yield dict(g, **c, **d)
    # an unscanned TLAS too large for LDS under walks that stay short: many objects of one leaf each
    for n, analytic, tan in itertools.product((200, 230, 260, 300), (False, True), (False, True)):
        yield dict(instances=n, mesh="quad", analytic=analytic, tangent_check=tan)
    # k_shade's LDS variants: records beyond and within its budget, with and without the triangle records
    for n, tri, m, l, mesh in itertools.product((100, 130), (0, 60), ("lambert", "glossy", "mixed"), (("sphere",), ("triangle",), ("sphere", "disk")), (None, "box")):
        yield dict(instances=n, pad_triangles=tri, materials=m, lights=l, mesh=mesh)
    # the class edges
    for sig in ((14, "lambert", 14), (15, "lambert", 15), (16, "lambert", 15), (14, "fourier", 14), (15, "fourier", 15), (17, "fourier", 15), (16, None, 0)):
        for mesh in (None, "box"):
            yield dict(instances=18, materials=("signatures",) + sig, mesh=mesh)


def boundary_pair(base, axis, values, inside):
    """The largest value of `axis` whose scene is inside, with its next-larger sibling outside."""
    best = None
    for v in values:
        _, (f, c) = plan(dict(base, **{axis: v}))
        if inside(f, c):
            best = v
        elif best is not None and v == best + 1:
            return dict(base, **{axis: best}), dict(base, **{axis: v})
    raise SystemExit(f"no boundary along {axis} of {base}")


def main():
    chosen = {}  # name -> axes
    covered = set()

    def take(axes):
        sb, (f, c) = plan(axes)
        if ties(sb, c):
            return False
        chosen[name_of(axes)] = axes
        covered.update(goals_of(f, c))
        return True

    pairs = {
        "scene": boundary_pair(dict(), "instances", range(20, 120), lambda f, c: c["lds_staging"] == pp.LDS_SCENE),
        "top": boundary_pair(dict(tlas_chain=8), "instances", range(40, 200), lambda f, c: c["lds_staging"] == pp.LDS_TOP),
        "shade_all": boundary_pair(dict(mesh="box", instances=12), "pad_triangles", range(1, 200), lambda f, c: f["shade_lds"] == pp.SHADE_LDS_ALL),
        "shade_records": boundary_pair(dict(instances=100, pad_triangles=40), "pad_materials", range(0, 120), lambda f, c: f["shade_lds"] == pp.SHADE_LDS_RECORDS),
    }
    for what, (a, b) in pairs.items():
        for axes in (a, b):
            if not take(axes):
                raise SystemExit(f"boundary pair {what}: the oracle renders {axes} with TLAS ties; change the family")
    print("# boundary pairs taken", file=sys.stderr)

    pool = []
    for axes in candidates():
        try:
            _, (f, c) = plan(axes)
        except Exception as e:  # a refused scene is no candidate
            print("# skipped", axes, e, file=sys.stderr)
            continue
        pool.append((axes, goals_of(f, c), f["n_instances"] + f["n_triangles"]))
    print(f"# {len(pool)} candidates probed", file=sys.stderr)
    wanted = {("key",) + k for k in pp.reachable_keys()} | {("shade",) + k for k in pp.shade_keys()}
    wanted |= {("signatures", 14), ("signatures", 15), ("signatures", 16), ("lambert_position", 14), ("lambert_position", 15), ("fourier_position", 14),
               ("fourier_position", 15), ("overflow", 2)}
    wanted |= {goal for _, goals, _ in pool for goal in goals if goal[0] == "launch"}
    while True:
        open_goals = wanted - covered
        best = max(pool, key=lambda p: (len(p[1] & open_goals), -p[2]), default=None)
        if best is None or not (best[1] & open_goals):
            break
        pool.remove(best)
        take(best[0])
    print("# left open:", sorted(wanted - covered, key=repr), file=sys.stderr)
    print("VARIANTS = {")
    for name, axes in chosen.items():
        print(f"    {name!r}: {({k: v for k, v in axes.items() if v != vs.DEFAULTS[k]})!r},")
    print("}")
    print("BOUNDARY_PAIRS = {")
    for what, (a, b) in pairs.items():
        print(f"    {what!r}: ({name_of(a)!r}, {name_of(b)!r}),")
    print("}")


if __name__ == "__main__":
    main()
