"""Times one batch of 512 image-method RIRs (256 utterances x speech + noise source, rooms / T60s / positions drawn like
the online-RIR simulation) made by pykaldi2_amd.rirgen in one call.  Prints the wall time of the call between two
device synchronisations; the kernel times come from a profiler run:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/rir_time.py
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pykaldi2_amd import rirgen  # noqa: E402

np.random.seed(0)
items = []
for _ in range(256):
    room, t60, mic, src = rirgen.sample_online_room((0.1, 0.5), 2)
    items.append(dict(room=room, source_loc=src, mic_loc=mic, t60=t60))
b = rirgen.rirgen_batch(items)          # warm-up: code objects, allocations
torch.cuda.synchronize()
times = []
for _ in range(10):
    t0 = time.perf_counter()
    b = rirgen.rirgen_batch(items)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
print("512 RIRs (%d samples): wall per call min %.3f ms, median %.3f ms (host descriptors + launches + kernels)"
      % (b.out.numel(), 1e3 * min(times), 1e3 * float(np.median(times))))
assert torch.isfinite(b.out).all()
