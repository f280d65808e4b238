"""CPU: the non-staged and the staged instantiation of the owner-binned scatter's producer kernel (f2n_set_scatter_producer) on the
emulated wavefront -- the kernel source's own meaning, whatever the compiler made of it for the GPU.  One case of
tests/test_gpu_scatter_producers.py at the smallest shape the binned path takes: n = 32768, 2^14 entries per level, the
50-samples-per-ray input (about 12 s here)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_scatter_producers as gsp  # noqa: E402
from test_wave_emul_cpu import emul_lib, hip  # noqa: E402,F401  (fixtures: the binding pointed at the emulated library)


def test_producers_agree_on_the_emulator(hip, fox_state):  # noqa: F811
    gsp.test_producers_agree_on_sizes_and_run_structures(hip, fox_state, 32768, "rays50")
