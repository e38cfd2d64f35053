"""Option k1_prio (java-rsync_amd/csrc/options.h) without a device: known, its default, and restored by a reset."""
import pytest

import rsync_hip as R

DEFAULT = 1  # turns of 2 stages (the kbench and bench pairs at 2, 8 and 32 stages)


@pytest.fixture(autouse=True)
def _lib():
    R.build()
    yield
    R.reset_options()


def test_k1_prio_known_with_default():
    R.reset_options()
    assert R.get_option("k1_prio") == DEFAULT
    with pytest.raises(ValueError):
        R.get_option("k1_prio_")


def test_k1_prio_reset_restores():
    R.set_option("k1_prio", 0)
    assert R.get_option("k1_prio") == 0
    R.set_option("k1_prio", 5)
    assert R.get_option("k1_prio") == 5
    R.reset_options()
    assert R.get_option("k1_prio") == DEFAULT
    assert R.get_option("k1_dma") == 1  # the neighbouring entry of the table keeps its own default


def test_k1_prio_option_context():
    with R.option("k1_prio", 4):
        assert R.get_option("k1_prio") == 4
    assert R.get_option("k1_prio") == DEFAULT


def test_md5_asm_files_are_the_generator_output():
    """csrc/md5_asm.inc is the generator's default output (unchanged by its --no-nop flag) and csrc/md5_asm_nonop.inc,
    the kbench-only form, is its --no-nop output: the same steps, no s_nop, under another name."""
    import os
    import subprocess
    import sys

    pkg = os.path.dirname(os.path.abspath(R.__file__))
    gen = os.path.join(pkg, "tools", "gen_md5_asm.py")
    default = subprocess.run([sys.executable, gen], check=True, capture_output=True, text=True).stdout
    nonop = subprocess.run([sys.executable, gen, "--no-nop"], check=True, capture_output=True, text=True).stdout
    assert default == open(os.path.join(pkg, "csrc", "md5_asm.inc")).read()
    assert nonop == open(os.path.join(pkg, "csrc", "md5_asm_nonop.inc")).read()
    assert default.count("s_nop 0") == 64 and "s_nop" not in nonop
    strip = lambda t: [x for x in t.replace("\\n\\ts_nop 0", "").splitlines()[2:]]  # noqa: E731
    assert strip(default) == strip(nonop)
    assert "md5_compress_rot16n(" in default and "md5_compress_rot16(" in nonop


def test_wave_times_export_is_declared():
    assert "rsh_debug_k1_wave_times" in R.DEBUG_EXPORTS
    assert R.lib().rsh_debug_k1_wave_times(None, None, 0, 0, 0, None, 0, None, None) == R.RSH_E_INVAL
