"""kernel_select = "riccati" (FTMPC_KERNEL_RICCATI): the Python layer's constant and mapping.  No GPU needed."""
import pytest

from ft_mpc_amd import _lib
from ft_mpc_amd.batch import BatchedMPC, MPCConfig


def test_lib_exposes_the_constant():
    assert _lib.KERNEL_RICCATI == 3
    assert len({_lib.KERNEL_AUTO, _lib.KERNEL_DENSE, _lib.KERNEL_WORKGROUP, _lib.KERNEL_RICCATI}) == 4


def test_header_and_python_agree():
    from pathlib import Path
    import re
    text = (Path(__file__).resolve().parents[1] / "include" / "ftmpc.h").read_text()
    assert int(re.search(r"#define\s+FTMPC_KERNEL_RICCATI\s+(\d+)", text).group(1)) == _lib.KERNEL_RICCATI


def test_config_maps_riccati():
    lib = _lib.load_library()
    c = BatchedMPC.make_c_config(lib, MPCConfig(N=17, NT=16, kernel_select="riccati"))
    assert c.kernel_select == _lib.KERNEL_RICCATI
    c = BatchedMPC.make_c_config(lib, MPCConfig(N=17, NT=16))
    assert c.kernel_select == _lib.KERNEL_AUTO


def test_unknown_kernel_select_still_raises():
    lib = _lib.load_library()
    with pytest.raises(ValueError):
        BatchedMPC.make_c_config(lib, MPCConfig(N=17, NT=16, kernel_select="ricatti"))
