"""What the GPU tests ask about the device they run on.  TEST INFRASTRUCTURE ONLY."""
import functools
import subprocess
import sys

MAX_WAVES_PER_CU = 32       # the most waves a CDNA compute unit keeps resident (8 per SIMD, four SIMDs)


@functools.lru_cache(maxsize=None)
def compute_units():
    """The device's CU count, from torch in a child process (torch brings a HIP runtime of its own, and a process that has loaded
    the library first cannot use it: tests/test_gpu_torch_interop.py).  Asked once per run; the limit allows for torch's cold
    import (some ten seconds at worst), and a failure names its cause in one line."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, "the CU count could not be read through torch: " + (out.stderr.strip().splitlines() or ["?"])[-1]
    cus = int(out.stdout.split()[-1])
    assert 1 <= cus <= 4096
    return cus
