"""train.dist_loss_weight through the C++ host layer on the wavefront emulator: body (b) of tests/test_gpu_distortion.py (the untaped
step against the taped one, the reported term against the fp64 definition) with tests/test_wave_emul_cpu.py's fixtures -- the host
compiled against the emulated kernel library, behind f2_nerf_amd.runtime.  A file of its own that sorts behind test_wave_emul_cpu.py:
that file's `emul_host` loads the emulated library into the global symbol scope, which must not happen before its mutant builds have
been loaded and tried."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_wave_emul_cpu import emul_host, emul_lib, hip, rt  # noqa: E402,F401


def test_untaped_step_equals_taped_step_with_the_term_on_the_emulator(rt, fox_state):
    """the weight is the one the oracle precondition of tests/test_gpu_distortion.py arrives at (1/16)"""
    import test_gpu_distortion as gd
    gd.check_untaped_equals_taped(rt, fox_state, gd._setup(rt, fox_state), 0.0625)
