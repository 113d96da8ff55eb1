#!/usr/bin/env python3
"""Cost of the streaming evaluation statistics beside the gather form's torch operations.

  python tools/eval_stream_speed.py [--part kernels,loop] [--shapes 128x100,...] [--rounds 5] [--iters 50] [--batches 10,100] [--precision fp16]

kernels  On one resident fp32 [B, C] tensor, (B, C) = (128, 100), (128, 1000), (1024, 21843): `stream` = dyt_eval_rows (row kernel + fold, two
         launches) against `torch` = what the gather form runs on its concatenated logits -- topk(5) + the hit comparison, topk(1) + two
         bincounts, and F.cross_entropy for the loss the streaming form also returns.  Timed in alternation, `rounds` windows of `iters`
         calls each, a host clock around a window that ends in a device synchronise, after a warm-up of both; GB/s is B * C * 4 bytes over the
         median.  (For per-kernel times run this part under `rocprofv3 --kernel-trace --stats`, on its own.)
loop     engine_finetune.evaluate, streaming against gather, on an inference-only model with a resident synthetic loader of B = 128 batches:
         C = 100, and C = 21843 on the wide head.  ms per batch (alternating windows) and torch.cuda.max_memory_allocated() of each form
         at every batch count of --batches.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-tuning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import synth  # noqa: E402


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def kernels(a):
    from util.metrics import StreamingEval
    out = {}
    for B, C in a.shapes:
        g = torch.Generator().manual_seed(B + C)
        x = (torch.randn(B, C, generator=g) * 3.0).cuda()
        y = torch.randint(0, C, (B,), generator=g).cuda()
        st = StreamingEval(C, device="cuda")

        def stream():
            st.update(x, y)

        def gather():
            ranked = x.topk(5, dim=1).indices
            hits = (ranked == y.reshape(B, 1)).float().cumsum(1)
            top1 = x.topk(1, dim=-1).indices.reshape(-1)
            return hits[:, 0].sum(), hits[:, 4].sum(), torch.bincount(y[top1 == y], minlength=C), torch.bincount(y, minlength=C), F.cross_entropy(x, y)
        forms = {"stream": stream, "torch": gather}
        for f in forms.values():
            window(f, 5)
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, f in forms.items():
                ms[k].append(round(window(f, a.iters), 5))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out["%dx%d" % (B, C)] = dict(ms=ms, median_ms=med, spread_ms={k: round(max(v) - min(v), 5) for k, v in ms.items()},
                                     gbps={k: round(B * C * 4 / (m * 1e-3) / 1e9, 1) for k, m in med.items()})
    return out


class Resident:
    def __init__(self, x, y, n):
        self.x, self.y, self.n = x, y, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for _ in range(self.n):
            yield self.x, self.y


def loop(a):
    from engine_finetune import evaluate
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    dev = torch.device("cuda", 0)
    B, r = 128, 64
    out = {}
    for C in (100, 21843):
        tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                     ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
        model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                           precision=a.precision, train_mode="compact", max_batch=B, inference_only=True)
        model.load_state_dict(synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85))
        model = model.to(dev).eval()
        x, y = synth.make_batch(B, C, seed=1)
        x, y = x.to(dev), y.to(dev)
        res = {}
        for n in a.batches:
            loader = Resident(x, y, n)
            forms = {"stream": types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=True),
                     "gather": types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=False)}
            status = {k: evaluate(loader, model, dev, None, None, None, args) for k, args in forms.items()}   # warm-up of both
            assert status["stream"]["acc1"] == status["gather"]["acc1"], status
            ms, peak = {k: [] for k in forms}, {}
            for _ in range(a.rounds if n <= 10 else 2):
                for k, args in forms.items():
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    t0 = time.perf_counter()
                    evaluate(loader, model, dev, None, None, None, args)   # ends in the .item() / .cpu() of its result
                    torch.cuda.synchronize()
                    ms[k].append(round((time.perf_counter() - t0) * 1e3 / n, 4))
                    peak[k] = torch.cuda.max_memory_allocated() - base
            res[str(n)] = dict(ms_per_batch=ms, median_ms={k: statistics.median(v) for k, v in ms.items()}, peak_bytes_above_model=peak)
        out["B%d_C%d" % (B, C)] = res
        del model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernels,loop")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", default="10,100")
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--shapes", default="128x100,128x1000,1024x21843", help="BxC of the kernels part (one shape per profiler run keeps its per-kernel rows apart)")
    a = ap.parse_args()
    a.batches = [int(v) for v in a.batches.split(",") if v]
    a.shapes = [tuple(int(n) for n in v.split("x")) for v in a.shapes.split(",") if v]
    assert torch.cuda.is_available(), "eval_stream_speed needs the GPU"
    res = dict(tool="eval_stream_speed", precision=a.precision, rounds=a.rounds, iters=a.iters, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))
    if "kernels" in a.part:
        res["kernels"] = kernels(a)
    if "loop" in a.part:
        res["loop"] = loop(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
