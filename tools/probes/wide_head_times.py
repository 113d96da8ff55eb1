"""Kernel times of the classification head at B = 128 in a depth-1 fp32 context: the wide form (csrc/head_wide.hip) at C = 21 843 and
C = 1000, the row-kernel form at C = 1000.

  run under the profiler:   rocprofv3 --kernel-trace --stats -d DIR -o wh --output-format csv -- python tools/probes/wide_head_times.py
  summarise its trace:      python tools/probes/wide_head_times.py --summarise DIR/.../wh_kernel_trace.csv

The summary groups the head kernels by (name, workgroups) -- the grid separates the two class counts -- and reports the average of the
timed launches, the achieved GB/s against each kernel's compulsory traffic and TFLOP/s against the 157 TFLOP/s fp32-MFMA peak."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, REPS = 128, 10


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-tuning_amd")]
    import torch
    import synth
    from runtime import DyTEngine
    sd = synth.make_state_dict(1, 8, seed=0, kind="test", depth=1, gate_bias=0.85)
    x, _ = synth.make_batch(B, 10, seed=0)
    x = x.cuda()
    for C, wide in ((21843, True), (1000, True), (1000, False)):
        sdc = dict(sd)
        sdc["head.weight"] = synth._normal("head.weight", (C, 768), 0, 0.02)
        sdc["head.bias"] = synth._normal("head.bias", (C,), 0, 0.02)
        eng = DyTEngine(C, 8, 0.1, "cuda:0", precision="fp32", max_batch=B, depth=1, wide_head=wide)
        eng.load_state_dict(sdc)
        dl = torch.randn(B, C, device="cuda") / B
        grad = torch.zeros(eng.n_train, device="cuda")
        for _ in range(REPS + 2):   # (the first two launches of a kernel are left out of the summary)
            eng.forward(x, slot=0, training=True, save=True, seed=1)
            eng.backward(0, dl, grad)
        torch.cuda.synchronize()
        print("C=%d wide=%d: %d passes" % (C, wide, REPS + 2), flush=True)
        del eng, grad
        torch.cuda.empty_cache()


def summarise(path):
    rows = list(csv.DictReader(open(path)))
    agg = {}
    for r in rows:
        m = re.search(r"(head_[a-z_]+_kernel)", r["Kernel_Name"])
        if not m:
            continue
        wgs = (int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])) // (int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"]))
        agg.setdefault((m.group(1), wgs), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    # compulsory bytes / FLOPs per (kernel, C): head.weight once for logits and dx, read-modify-write for dW; 2 B C 768 FLOPs each
    work = {}
    for C in (21843, 1000):
        w = C * 768 * 4.0
        f = 2.0 * B * C * 768
        work[("head_wide_logits_kernel", -(-C // 128) * 2)] = (C, w, f)
        work[("head_wide_dx_kernel", 6 * 2 * -(-C // 1024))] = (C, w, f)
        work[("head_wide_dw_kernel", 6 * -(-C // 64))] = (C, 2 * w, f)
    print("%-30s %6s %7s %6s %10s %10s %9s %9s" % ("kernel", "wgs", "C", "calls", "avg us", "min us", "GB/s", "TFLOP/s"))
    for (name, wgs), ds in sorted(agg.items()):
        ds = ds[2:] if len(ds) > 4 else ds
        avg, mn = sum(ds) / len(ds), min(ds)
        C, byts, fl = work.get((name, wgs), ("", None, None))
        print("%-30s %6d %7s %6d %10.1f %10.1f %9s %9s" % (name, wgs, C, len(ds), avg, mn, "%.0f" % (byts / avg / 1e3) if byts else "-",
                                                          "%.1f" % (fl / avg / 1e6) if fl else "-"))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        run()
