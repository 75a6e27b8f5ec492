"""tools/isa_same_kernels.py on two small hand-made device assemblies: a kernel whose local labels are merely renumbered counts as the
same, one with another instruction or another register budget does not (the comparison behind `same_isa_as_measured`); the
exit status says whether every kernel is accounted for."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNEL = """
\t.globl\t{name}
{name}:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\t.loc 1 {line} 0
\tv_mov_b32_e32 v1, {imm}
\ts_cbranch_scc1 .LBB{n}_2
.LBB{n}_2:
\ts_endpgm
.Lfunc_end{n}:
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
"""


def asm(path, specs):
    with open(path, "w") as f:
        for n, (name, imm, vgpr) in enumerate(specs):
            f.write(KERNEL.format(name=name, n=n + 7 * (path.endswith("b.s")), imm=imm, vgpr=vgpr, line=10 + n))


def test_kernels_that_differ_are_named(tmp_path):
    a, b = str(tmp_path / "a.s"), str(tmp_path / "b.s")
    asm(a, [("_Z5k_onev", 1, 8), ("_Z5k_twov", 2, 8), ("_Z7k_threev", 3, 8)])
    asm(b, [("_Z5k_onev", 1, 8), ("_Z5k_twov", 5, 8), ("_Z7k_threev", 3, 16)])
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_same_kernels.py"), a, b], capture_output=True, text=True)
    assert run.returncode == 1, run.stderr  # kernels differ
    out = run.stdout
    assert "kernels 3: same 1, different 2" in out
    assert "k_two" in out and "k_three" in out and "k_one" not in out.split("\n", 1)[1]


def test_a_renamed_kernel_with_the_same_body_and_budget_counts_as_the_same(tmp_path):
    a, b = str(tmp_path / "a.s"), str(tmp_path / "b.s")
    asm(a, [("_Z5k_onev", 1, 8), ("_Z5k_oldv", 2, 8), ("_Z6k_gonev", 3, 8), ("_Z6k_lessv", 4, 8)])
    asm(b, [("_Z5k_onev", 1, 8), ("_Z5k_newv", 2, 8), ("_Z6k_camev", 7, 8), ("_Z6k_morev", 4, 16)])
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_same_kernels.py"), a, b], capture_output=True, text=True)
    assert run.returncode == 1, run.stderr  # kernels differ
    out = run.stdout
    # k_old -> k_new: same body, same registers.  k_gone / k_came differ in an instruction, k_less / k_more in the register budget.
    assert "kernels 6: same 2 (1 of them renamed), different 4" in out
    assert re.search(r"renamed: \S*k_old\S* -> \S*k_new", out)  # (mangled where there is no demangler)
    assert out.count("renamed:") == 1 and out.count("differs:") == 4
    for n in ("k_gone", "k_came", "k_less", "k_more"):
        assert any(n in line and "differs:" in line for line in out.splitlines())


def test_masked_register_numbers_make_a_class_of_their_own_and_the_exit_status_follows(tmp_path):
    a, b = str(tmp_path / "a.s"), str(tmp_path / "b.s")
    asm(a, [("_Z5k_onev", 1, 8), ("_Z5k_twov", 2, 8), ("_Z7k_threev", 3, 8)])
    asm(b, [("_Z5k_onev", 1, 8), ("_Z5k_twov", 2, 8), ("_Z7k_threev", 3, 8)])
    text = open(b).read().split("_Z5k_twov:")
    text[1] = text[1].replace("v_mov_b32_e32 v1, 2", "v_mov_b32_e32 v3, 2").replace("s[0:1], s[4:5]", "s[2:3], s[4:5]", 1)  # other registers, same widths
    open(b, "w").write("_Z5k_twov:".join(text))
    tool = [sys.executable, os.path.join(ROOT, "tools", "isa_same_kernels.py")]
    plain = subprocess.run(tool + [a, b], capture_output=True, text=True)
    assert plain.returncode == 1 and "kernels 3: same 2, different 1" in plain.stdout
    masked = subprocess.run(tool + ["--mask-registers", a, b], capture_output=True, text=True)
    assert masked.returncode == 0, masked.stdout + masked.stderr
    assert "kernels 3: same 2, same once register numbers are masked 1, different 0" in masked.stdout
    assert any("same once masked:" in line and "k_two" in line for line in masked.stdout.splitlines())
    # a wider register range or another immediate is no renaming
    open(b, "w").write(open(b).read().replace("s[2:3], s[4:5]", "s[0:3], s[4:5]"))
    assert subprocess.run(tool + ["--mask-registers", a, b], capture_output=True, text=True).returncode == 1
    assert subprocess.run(tool + [a, a], capture_output=True, text=True).returncode == 0
