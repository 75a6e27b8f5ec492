"""The entry nodes' two entry points (include/pbrs_gpu.h: pbrse_set_entry_nodes, pbrse_last_entry_info): declared, exported, in a symbol
table of their own and wrapped by the driver (no compute calls: runs without a GPU)."""
import ctypes
import os
import re

import pbrs_amd
from pbrs_amd import api, libs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["pbrse_last_entry_info", "pbrse_set_entry_nodes"]


def test_header_table_library_and_wrapper_agree():
    header = open(os.path.join(ROOT, "include", "pbrs_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(pbrse_[a-z_0-9]+)\s*\(", code))) == SYMBOLS
    assert "int pbrse_set_entry_nodes(pbrs_ctx*, int enabled);" in header and "int pbrse_last_entry_info(pbrs_ctx*, pbrs_entry_info* out);" in header
    assert sorted(libs.GPU_ENTRY_SYMBOLS) == SYMBOLS == sorted(api.GPU_ENTRY_SYMBOLS)
    assert not set(SYMBOLS) & set(libs.GPU_SYMBOLS)
    lib = pbrs_amd.gpu_lib()
    for n, (argtypes, restype) in libs.GPU_ENTRY_FUNCTIONS.items():
        fn = getattr(lib, n)
        assert list(fn.argtypes) == list(argtypes) and fn.restype is restype is ctypes.c_int, n
    assert libs.GPU_ENTRY_FUNCTIONS["pbrse_set_entry_nodes"][0] == [ctypes.c_void_p, ctypes.c_int]
    assert libs.GPU_ENTRY_FUNCTIONS["pbrse_last_entry_info"][0] == [ctypes.c_void_p, ctypes.c_void_p]
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", pbrs_amd.lib_paths()[1]], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("pbrse_")) == SYMBOLS
    assert callable(api.Context.set_entry_nodes) and callable(api.Context.last_entry_info)


def test_the_struct_is_four_words():
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include "pbrs_gpu.h"\nint main(void) { printf("%zu\\n", sizeof(pbrs_entry_info)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        assert int(subprocess.check_output([os.path.join(d, "t")])) == 16
