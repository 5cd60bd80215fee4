"""CPU: the build check of the kernels that issue LDS-DMA (csrc/usage_check.py, run by csrc/Makefile), fed synthetic
compiler remarks: a clean report passes; an SGPR spill or scratch in a matching kernel fails; fewer matching kernels than
counted fails; a spilling kernel of another name is ignored."""
import importlib.util
import os

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "superpoints_registration_amd", "csrc")
_spec = importlib.util.spec_from_file_location("usage_check", os.path.join(CSRC, "usage_check.py"))
usage_check = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(usage_check)


def remarks(name, scratch=0, sgpr_spill=0, vgpr_spill=0):
    """The remarks of one kernel, in the compiler's format (with the source line it quotes under the first)."""
    tag = "[-Rpass-analysis=kernel-resource-usage]"
    fields = [("TotalSGPRs", 96), ("VGPRs", 128), ("AGPRs", 0), ("ScratchSize [bytes/lane]", scratch),
              ("Dynamic Stack", "False"), ("Occupancy [waves/SIMD]", 4), ("SGPRs Spill", sgpr_spill),
              ("VGPRs Spill", vgpr_spill), ("LDS Size [bytes/block]", 16640)]
    lines = [f"k.hip:41:1: remark: Function Name: {name} {tag}",
             "   41 | __global__ void k(",
             "      | ^"]
    lines += [f"k.hip:41:1: remark:     {key}: {val} {tag}" for key, val in fields]
    return "\n".join(lines) + "\n"


def ring(i, **kw):
    return remarks(f"_ZN3spr12_GLOBAL__N_113k_kpconv_ringILi32ELi{32 * (i + 1)}ELi4EEEvPKfi", **kw)


def run(tmp_path, text, name="k_kpconv_ring", count=3):
    path = tmp_path / "k.usage.txt"
    path.write_text(text)
    return usage_check.main(["usage_check.py", str(path), name, str(count)])


def test_clean_report_passes(tmp_path, capsys):
    assert run(tmp_path, ring(0) + ring(1) + ring(2)) == 0
    assert capsys.readouterr().out.count("scratch 0 B/lane, SGPR spills 0") == 3


def test_sgpr_spill_fails(tmp_path, capsys):
    assert run(tmp_path, ring(0) + ring(1, sgpr_spill=3) + ring(2)) == 1
    assert "1 instantiation(s)" in capsys.readouterr().err


def test_scratch_fails(tmp_path):
    assert run(tmp_path, ring(0) + ring(1) + ring(2, scratch=16, vgpr_spill=4)) == 1


def test_fewer_kernels_than_counted_fails(tmp_path, capsys):
    assert run(tmp_path, ring(0) + ring(1)) == 1
    assert "2 kernels named *k_kpconv_ring* reported, expected 3" in capsys.readouterr().err


def test_other_kernels_are_ignored(tmp_path):
    other = remarks("_ZN3spr12_GLOBAL__N_113k_kpconv_mfmaILi32ELi64ELi4EEEvPKfi", scratch=8, sgpr_spill=13, vgpr_spill=2)
    assert run(tmp_path, ring(0) + other + ring(1) + ring(2)) == 0


def test_warnings_stay_visible(tmp_path, capsys):
    warning = "k.hip:7:3: warning: unused variable 'x' [-Wunused-variable]\n    7 |   int x;\n"
    assert run(tmp_path, warning + ring(0) + ring(1) + ring(2)) == 0
    err = capsys.readouterr().err
    assert "unused variable" in err and "remark:" not in err and "__global__" not in err
