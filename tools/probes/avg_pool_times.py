"""A depth-2 fp32 context at B = 128 with DYT_CREATE_AVG_POOL on the serial schedule: twelve fused steps, to be run under
``rocprofv3 --kernel-trace --stats --output-format csv`` (profiles/round9/r9_avg_pool_times.txt)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-tuning_amd")]
import torch
import synth
from runtime import DyTEngine
B, C, r, depth = 128, 100, 64, 2
sd = synth.make_state_dict(C, r, seed=0, kind="bench", depth=depth, gate_bias=0.85, head_norm="fc_norm")
eng = DyTEngine(C, r, 0.1, "cuda:0", precision="fp32", max_batch=B, depth=depth, avg_pool=True)
eng.load_state_dict(sd)
import _lib
eng.set_option(_lib.OPT_STREAM_OVERLAP, 0)   # serial schedule: a kernel's time is its own
x, y = synth.make_batch(B, C, seed=0)
x, y = x.cuda(), y.cuda()
for i in range(12):
    eng.step_fwd_bwd(x, y, 0.5, 2.0, 0.0, 0.0, seed=i)
torch.cuda.synchronize()
print("done", float(eng.losses[0]))
