"""scripts/phase_census.py on a small hand-written assembly: regions split at the stamp comments, classes and pipe cycles."""
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
spec = importlib.util.spec_from_file_location("phase_census", ROOT / "scripts" / "phase_census.py")
pc = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pc)

ASM = """\
_ZN5ftmpc22ftmpc_solve_f32_kernelILi8EEEvNS_12DeviceConstsENS_11SolveParamsE: ; @x
	v_mov_b32_e32 v0, 0
	s_memtime s[0:1]
	;;#ASMSTART
	; phase_census stamp 0
	;;#ASMEND
	v_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]
	v_fmac_f32_dpp v1, v2, v3 row_newbcast:1 row_mask:0xf bank_mask:0xf
	v_permlane32_swap_b32_e32 v6, v7
	v_rsq_f32_e32 v8, s4
	ds_bpermute_b32 v9, v10, v11
	buffer_load_dwordx4 v[12:15], v16, s[8:11], 0 offen
	scratch_load_dword v17, off, off offset:4
	s_nop 1
	;;#ASMSTART
	; phase_census stamp 5
	;;#ASMEND
	s_endpgm
.Lfunc_end7:
"""


def test_census_regions(tmp_path):
    f = tmp_path / "k.s"
    f.write_text(ASM)
    regions = pc.census(pc.kernel_lines(str(f), 8))
    assert [r[0] for r in regions] == [0, 5, None]
    ph0, ph5 = regions[0][1], regions[1][1]
    assert ph0 == {"valu_other": 1, "salu": 1}
    assert ph5 == {"mfma": 1, "dpp": 1, "permlane": 1, "valu_f32": 1, "lds": 1, "vmem": 1, "scratch": 1, "s_nop": 1}
    assert regions[1][2] == 32 + 4 + 4 + 8          # MFMA, DPP FMA, permlane, rsq
