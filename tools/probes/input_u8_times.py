"""Kernel time of image_load_kernel from both byte layouts next to the fp32 source, in one process.

Run mode (under ``rocprofv3 --kernel-trace --output-format csv``): fp16 eval forwards at B = 128 through one inference-only context,
alternating float images, uint8 [B,3,224,224] and uint8 [B,224,224,3] -- REPS rounds of the three, the first WARM rounds are warm-up.
The weights are left at zero: the embedding prologue's time does not depend on them.  The bytes are uniform random (every table entry
is looked up).
Parse mode: ``python tools/probes/input_u8_times.py --parse TRACE.csv [...]`` prints, per kernel instance, the mean / min / max of the
launches after warm-up, and the bytes each moves over that time."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-tuning_amd")]

B, REPS, WARM = 128, 15, 3
PIX = 3 * 224 * 224


def run():
    import torch
    import synth
    from runtime import DyTEngine
    dev = torch.device("cuda", 0)
    eng = DyTEngine(100, 64, 0.1, dev, precision="fp16", max_batch=B, inference=True)
    x = synth.make_batch(B, 100, seed=0)[0].to(dev)
    u = synth.make_byte_batch(B, seed=0).to(dev)
    nhwc = synth.make_byte_batch(B, seed=0, nhwc=True).to(dev)
    torch.cuda.synchronize()
    for _ in range(REPS):
        for t in (x, u, nhwc):
            eng.forward(t, want_tokens=False)
        torch.cuda.synchronize()
    print("done: %d rounds of float / u8 / u8-nhwc forwards at B=%d" % (REPS, B))


def parse(paths):
    out_bytes = B * 196 * 768 * 2   # the fp16 operand
    moved = {0: B * PIX * 4 + out_bytes, 1: B * PIX + out_bytes, 2: B * PIX + out_bytes}   # by source kind (csrc/image_items.h)
    for path in paths:
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        runs = {}
        for r in rows:
            name = r["Kernel_Name"]
            if "image_load_kernel" in name:
                runs.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for name, d in sorted(runs.items()):
            t = d[WARM:]
            m = re.search(r"image_load_kernel<(\d)", name) or re.search(r"image_load_kernelILi(\d)E", name)   # demangled or not
            kind = int(m.group(1))
            mean = sum(t) / len(t)
            print("%-86s mean %7.2f us  min %7.2f  max %7.2f  (%d launches)  %5.1f MB -> %5.2f TB/s" % (
                name[:86], mean, min(t), max(t), len(t), moved[kind] / 1e6, moved[kind] / mean / 1e6))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--parse":
        parse(sys.argv[2:])
    else:
        run()
