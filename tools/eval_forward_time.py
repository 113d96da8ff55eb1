#!/usr/bin/env python3
"""Time the eval forward (speed.py's harness: synthetic "bench" weights, gate biases calibrated to the target keep ratio) with HIP events.

    python tools/eval_forward_time.py --precision fp16 --batch 128 [--inference-only] [--root OTHER_CHECKOUT]

After warm-up, `--runs` forwards are timed one by one (event pair around each) and their median is taken; that is repeated `--repeats`
times in the same process, so the spread of the medians (max - min) is the run-to-run noise a difference has to exceed.  `--root`
imports the package from another checkout (e.g. the parent commit, built) for a same-box, same-session A/B.  One JSON line."""
import argparse
import json
import math
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--keep", type=float, default=0.7)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--inference-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.root, "dynamic-tuning_amd"))
    import torch
    import synth
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k

    class Cfg(dict):
        __getattr__ = dict.__getitem__

    dev = torch.device("cuda", 0)
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=64, d_model=768)
    kw = dict(inference_only=True) if args.inference_only else {}
    model = vit_base_patch16_224_in21k(num_classes=100, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                       precision=args.precision, max_batch=args.batch, **kw)
    model.load_state_dict(synth.make_state_dict(100, 64, kind="bench", gate_bias=math.log(args.keep / (1 - args.keep))))
    model = model.to(dev).eval()
    x = synth.make_batch(args.batch, 100, seed=0)[0].to(dev)
    with torch.no_grad():
        for _ in range(3):   # speed.py's calibration: the target quantile of every block's token logits at the decision threshold
            _, aux = model(x)
            tl = aux["token_logits"].float()
            tl = tl.reshape(tl.shape[0], tl.shape[1], -1).permute(1, 0, 2).reshape(tl.shape[1], -1)
            q = torch.quantile(tl, 1.0 - args.keep, dim=1)
            for i, blk in enumerate(model.blocks):
                blk.mlp_token_select.mlp_head.bias.sub_(q[i].to(blk.mlp_token_select.mlp_head.bias.device))
        for _ in range(args.warmup):
            _, aux = model(x)
        torch.cuda.synchronize()
        medians = []
        for _ in range(args.repeats):
            ms = []
            for _ in range(args.runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                model(x)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            medians.append(statistics.median(ms))
    print(json.dumps(dict(root=os.path.abspath(args.root), precision=args.precision, batch=args.batch, inference_only=bool(args.inference_only),
                          keep_ratio=round(float(aux["token_select"].mean()), 4), ctx_bytes=model._engine.bytes, runs=args.runs,
                          medians_ms=[round(m, 4) for m in medians], median_ms=round(statistics.median(medians), 4),
                          spread_ms=round(max(medians) - min(medians), 4))))


if __name__ == "__main__":
    main()
