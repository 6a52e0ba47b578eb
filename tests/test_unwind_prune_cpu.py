"""The premises of tests/test_gpu_unwind_prune.py, on the CPU oracle alone: the frames
the device is compared on hold both kinds of path -- ones that end with L = +0, whose
unwind the kernel prunes, and lit ones, whose deep levels it must keep -- and the
hostile colours do reach the frame."""
import numpy as np
import pytest

from tests import prune_scenes as PS


@pytest.mark.parametrize("name", ["box", "ball", "c5", "tir_lit"])
def test_base_frames_hold_zero_and_lit_paths(name):
    """A 1-spp pixel is one path: at least 10 % end exactly zero, at least 5 % are lit."""
    depth = 32 if name == "tir_lit" else PS.DEPTH
    rad, _ = PS.oracle_frame(name, PS.base(name), spp=1, depth=depth)
    zero = (PS.bits(rad) == 0).all(-1).mean()
    lit = (rad != 0).any(-1).mean()
    print(f"{name}: zero {zero:.3f} lit {lit:.3f}")
    assert zero >= 0.10 and lit >= 0.05, (zero, lit)


def test_shipped_tir_is_dark():
    """Why the premise above is stated for tir_lit: the shipped tir's 1-spp frame has no lit
    pixel at the test size (every path is pruned; the device test still runs it)."""
    rad, _ = PS.oracle_frame("tir", PS.base("tir"), spp=1, depth=32)
    assert (rad != 0).any(-1).mean() < 0.05


@pytest.mark.parametrize("name", ["inf", "nan"])
def test_nonfinite_colours_reach_the_frame(name):
    """The reference turns zero paths through the floor into NaN (0 * inf, 0 * NaN): a
    kernel that pruned them would return 0."""
    rad, _ = PS.oracle_frame(name, PS.hostile(name))
    nan = np.isnan(rad).any(-1).mean()
    print(f"{name}: NaN pixels {nan:.3f}")
    assert nan >= 0.01, nan
    base, _ = PS.oracle_frame("box", PS.base("box"))
    assert not np.isnan(base).any()


@pytest.mark.parametrize("name", ["negative", "overcap"])
def test_finite_hostile_colours_change_the_frame(name):
    rad, _ = PS.oracle_frame(name, PS.hostile(name))
    base, _ = PS.oracle_frame("box", PS.base("box"))
    assert not np.array_equal(PS.bits(rad), PS.bits(base))


def test_grown_table_keeps_the_hostile_frame():
    """65 materials (the table leaves LDS) around the inf colour: the same frame."""
    rad, _ = PS.oracle_frame("inf", PS.hostile("inf"))
    big, _ = PS.oracle_frame("inf_m65", PS.hostile("inf", 65))
    n = np.isnan(rad)
    assert np.array_equal(n, np.isnan(big)) and np.array_equal(PS.bits(rad)[~n], PS.bits(big)[~n])
