"""The names and signatures the package has promised so far (tests/golden/api_surface.json) still resolve and still match, whichever
module now defines them; and the libraries' symbol tables are whole.  The golden file was written by running this module as a script
(`python tests/test_api_surface.py > tests/golden/api_surface.json`) on the commit before the driver was split into abi.py, libs.py,
devmem.py and api.py; it is regenerated only when a name is added on purpose."""
import inspect
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_surface.json")
# what tests and tools reach for by its private name
PRIVATE_API = ("_display_params", "_upscale_params", "_history_clip", "_temporal_struct", "_matte_select", "_aov_names", "_pass_names", "_motion_args")
PRIVATE_CONTEXT = ("_spatial_params", "_params", "_render_host", "_render_device", "_render_guides_device", "_aov_device", "_check")


def _public(module):
    return sorted(n for n, v in vars(module).items() if not n.startswith("_") and not inspect.ismodule(v))


def surface():
    import pbrs_amd
    from pbrs_amd import api
    functions = {n: str(inspect.signature(getattr(api, n))) for n in _public(api) if inspect.isfunction(getattr(api, n))}
    functions.update({n: str(inspect.signature(getattr(api, n))) for n in PRIVATE_API})
    methods = {n: str(inspect.signature(v)) for n, v in inspect.getmembers(api.Context, callable) if not n.startswith("_")}
    makers = {}
    for cn in _public(api):
        cls = getattr(api, cn)
        if inspect.isclass(cls) and cls is not api.Context:
            makers.update({f"{cn}.{n}": str(inspect.signature(v)) for n, v in inspect.getmembers(cls, inspect.ismethod) if not n.startswith("_")})
    return {"pbrs_amd": _public(pbrs_amd), "pbrs_amd.api": _public(api), "private_api": list(PRIVATE_API),
            "private_context": list(PRIVATE_CONTEXT), "functions": functions, "context_methods": methods, "class_methods": makers,
            "gpu_symbols": sorted(api.GPU_SYMBOLS), "host_symbols": sorted(api.HOST_SYMBOLS)}


def test_every_promised_name_resolves_and_every_signature_matches():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = surface()
    for key in ("pbrs_amd", "pbrs_amd.api"):
        assert not set(want[key]) - set(got[key]), (key, sorted(set(want[key]) - set(got[key])))
    import pbrs_amd
    from pbrs_amd import api
    for n in want["pbrs_amd"]:  # the package's names are the driver's own objects, not copies
        if hasattr(api, n):
            assert getattr(pbrs_amd, n) is getattr(api, n), n
    for n in want["private_api"]:
        assert callable(getattr(api, n)), n
    assert callable(api.hip_runtime)
    for n in want["private_context"]:
        assert callable(getattr(api.Context, n)), n
    for key in ("functions", "context_methods", "class_methods"):
        assert want[key] and {n: got[key].get(n) for n in want[key]} == want[key], key
    assert sorted(api.GPU_SYMBOLS) == want["gpu_symbols"] and sorted(api.HOST_SYMBOLS) == want["host_symbols"]


def test_the_symbol_tables_are_whole():
    """GPU_SYMBOLS and HOST_SYMBOLS are their tables' keys, every entry carries its argument types, and the loader sets them on
    the library (a symbol with a missing entry fails at load, not at first call)."""
    import ctypes as C

    import pbrs_amd
    from pbrs_amd import libs
    for symbols, table, lib in ((libs.GPU_SYMBOLS, libs.GPU_FUNCTIONS, pbrs_amd.gpu_lib()), (libs.HOST_SYMBOLS, libs.HOST_FUNCTIONS, pbrs_amd.host_lib())):
        assert set(symbols) == set(table) and len(symbols) == len(table)
        for name, (argtypes, restype) in table.items():
            assert isinstance(argtypes, (list, tuple)), name
            fn = getattr(lib, name)
            assert list(fn.argtypes) == list(argtypes), name
            assert fn.restype is restype, name
    assert libs.GPU_FUNCTIONS["pbrs_create"][1] is C.c_int  # the default


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
