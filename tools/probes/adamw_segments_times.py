"""Kernel time of adamw_segments_kernel next to adamw_guarded_kernel on one flat buffer (profiles/round10/r10_adamw_segments_times.txt).
To be run under ``rocprofv3 --kernel-trace --output-format csv``; tools/probes/adamw_segments_parse.py reads the trace.  Serial launches on one
stream, per size: 15 x dyt_adamw_guarded, 15 x dyt_adamw_segments with 1 segment, 15 x with 26 segments (guarded form); the first 3 of each 15
are warm-up.  Sizes: the default model's 1 275 760 trainable elements, and 17 996 127 (the same adapters and gates under a 21 843-class head)."""
import ctypes
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-tuning_amd")]
import torch
import _lib
from _lib import ptr, stream_ptr

SIZES = (1275760, 17996127)
REPS = 15
L = _lib.lib()
g = torch.Generator(device="cuda:0").manual_seed(0)
for n in SIZES:
    p = 0.02 * torch.randn(n, device="cuda:0", generator=g)
    grad = 1e-3 * torch.randn(n, device="cuda:0", generator=g)
    m = 1e-3 * torch.randn(n, device="cuda:0", generator=g)
    v = 1e-6 * torch.rand(n, device="cuda:0", generator=g)
    state = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    one = [(n, 1e-3, 0.05)]
    many = [((k + 1) * n // 26, 1e-3 * 0.75 ** (k // 2), 0.05 * (k % 2)) for k in range(26)]   # the layer-decay recipe's 26 groups
    assert many[-1][0] == n
    torch.cuda.synchronize()
    for _ in range(REPS):
        _lib.check(L.dyt_adamw_guarded(ptr(p), ptr(grad), ptr(m), ptr(v), n, ptr(state), 1e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, stream_ptr()))
    torch.cuda.synchronize()
    for table in (one, many):
        arr = _lib.adamw_segment_array(table)
        for _ in range(REPS):
            _lib.check(L.dyt_adamw_segments(ptr(p), ptr(grad), ptr(m), ptr(v), n, ptr(state), 0, ctypes.cast(arr, ctypes.c_void_p), len(table),
                                            0.9, 0.999, 1e-8, 1.0, stream_ptr()))
        torch.cuda.synchronize()
    assert state.tolist()[:3] == [3 * REPS, 0, 0], state.tolist()
    del p, grad, m, v
print("done")
