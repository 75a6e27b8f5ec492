"""The C-ABI libraries load and export every symbol include/*.h declares (no compute calls: runs without a GPU)."""
import ctypes
import os
import re

import pytest

import pbrs_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pbrs_[a-z_0-9]+)\s*\(", text)))


def test_gpu_library_exports_every_declared_symbol():
    names = declared_functions("pbrs_gpu.h")
    assert set(names) == set(pbrs_amd.api.GPU_SYMBOLS), (names, pbrs_amd.api.GPU_SYMBOLS)
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[1])
    for n in names:
        assert getattr(lib, n) is not None, n


def test_host_library_exports_every_declared_symbol():
    names = declared_functions("pbrs_host.h")
    assert set(names) == set(pbrs_amd.api.HOST_SYMBOLS)
    lib = ctypes.CDLL(pbrs_amd.lib_paths()[0])
    for n in names:
        assert getattr(lib, n) is not None, n


def test_struct_sizes_match_the_headers():
    """ctypes mirrors vs the C layout (checked by compiling a tiny C file against the headers)."""
    import subprocess
    import tempfile
    src = r'''
#include <stdio.h>
#include "pbrs_gpu.h"
#include "pbrs_scene_spec.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(pbrs_node), sizeof(pbrs_instance), sizeof(pbrs_shape),
    sizeof(pbrs_mesh), sizeof(pbrs_tri_verts), sizeof(pbrs_tri_shade), sizeof(pbrs_bxdf), sizeof(pbrs_material), sizeof(pbrs_area_light),
    sizeof(pbrs_delta_light), sizeof(pbrs_scene_desc), sizeof(pbrs_camera), sizeof(pbrs_stats), sizeof(pbrs_render_params), sizeof(pbrs_scene_spec));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        sizes = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert sizes[:10] == [32, 128, 48, 32, 48, 64, 64, 32, 64, 32]
    from pbrs_amd import api, spec
    assert sizes[10] == ctypes.sizeof(api.SceneDesc)
    assert sizes[11] == ctypes.sizeof(api.Camera) == 64
    assert sizes[12] == ctypes.sizeof(api.Stats)
    assert sizes[13] == ctypes.sizeof(api.RenderParams)
    assert sizes[14] == ctypes.sizeof(spec.SceneSpec)


def test_product_path_fails_loudly_without_the_hip_library(monkeypatch, tmp_path):
    """No CPU fallback: a missing libpbrs_gpu.so is an error, not a silent detour."""
    from pbrs_amd import api, libs  # (the loaders' state lives in libs.py)
    monkeypatch.setattr(libs, "_gpu", None)
    monkeypatch.setattr(libs, "_LIBDIR", str(tmp_path))
    with pytest.raises(api.PbrsError, match="no CPU fallback"):
        api.gpu_lib()


def test_product_path_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under pbrs_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pbrs_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")) or f == "Makefile":
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not re.search(r"(^|\n)\s*(from|import)\s+oracle\b", text), os.path.join(dirpath, f)
                assert "libpbrs_oracle" not in text and "oracle/" not in text.replace("the CPU oracle in oracle/", ""), os.path.join(dirpath, f)


def test_the_shipped_hip_library_does_not_read_the_environment():
    """Kernel selection must not depend on the box a bench runs on: the developer overrides live behind -DPBRS_DEV_OVERRIDES
    and the shipped libpbrs_gpu.so does not import getenv at all."""
    import subprocess
    from pbrs_amd import api
    syms = subprocess.run(["nm", "-D", "--undefined-only", api.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in syms
    # every translation unit of the library: one call in all, inside dev_env(), which exists only under #ifdef PBRS_DEV_OVERRIDES
    csrc = os.path.join(ROOT, "pbrs_amd", "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(units) > 1, units
    calls = {f: open(os.path.join(csrc, f)).read().count("getenv(") for f in units}
    assert sum(calls.values()) == 1, calls
    src = open(os.path.join(csrc, next(f for f, n in calls.items() if n))).read()
    guarded = re.search(r"#ifdef PBRS_DEV_OVERRIDES\n(.*?)\n#endif", src, flags=re.S).group(1)
    assert "const char* dev_env(const char* name) { return std::getenv(name); }" in guarded


def defined_dynamic_symbols(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in out.splitlines() if line.strip()]


def test_gpu_library_exports_the_header_and_nothing_internal():
    """What the library's translation units share (pbrs_amd/csrc/kernel_tables.h) is hidden: the defined dynamic symbols that begin
    with pbrs_ are exactly the functions of include/pbrs_gpu.h, and of the project's C++ namespace only the host code's interface is
    visible (pbrs_amd/csrc/host/*.h: plain C++ that the CPU tests also compile on its own) — none of the tables' accessors."""
    import subprocess
    syms = defined_dynamic_symbols(pbrs_amd.lib_paths()[1])
    assert sorted(s for s in syms if s.startswith("pbrs_")) == declared_functions("pbrs_gpu.h")
    ours = [s for s in syms if re.match(r"_ZNK?4pbrs", s)]
    assert ours, "the host code's functions are part of the library"
    plain = subprocess.run(["c++filt"], input="\n".join(ours), capture_output=True, text=True, check=True).stdout.splitlines()
    host_dir = os.path.join(ROOT, "pbrs_amd", "csrc", "host")
    host_text = "\n".join(open(os.path.join(host_dir, f)).read() for f in sorted(os.listdir(host_dir)) if f.endswith(".h"))
    tables = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "pbrs_amd", "csrc", "kernel_tables.h")).read())
    internal = set(re.findall(r"^[\w:\* ]+?\b(\w+)\([^()]*\);", tables, flags=re.M))  # the functions it declares
    assert internal == {"extend_fns", "shadow_fns", "intersect_fn", "shade_fn", "bsdf_eval_fn"}, internal
    for name in plain:
        m = re.search(r"\bpbrs::(\w+)", name)
        assert m and m.group(1) not in internal, name
        assert re.search(r"\b%s\b" % m.group(1), host_text), name
