"""Host-fed training rate with byte batches and with float batches, relative to the resident rate.

The loop of bench.py's ``host_fed``: 8 distinct PINNED batches cycled through engine_finetune.train_one_epoch (per-iteration lr, the
DevicePrefetcher's copy stream, the fused step, one host sync per 20 steps), B = 128, fp16, compact training mode, at an 80-step and
a 20-step epoch.  Three sources: fp32 images (602 KB each), uint8 [B,3,224,224] and uint8 [B,224,224,3] (150 KB each), the model built
with input_norm.  "resident" = the same loop over two float batches that already live on the device; every rate is reported relative
to it.  The sources are timed in turn, ROUNDS times, and the best epoch of each is kept next to all of them.
Prints one JSON line."""
import json
import math
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dynamic-tuning_amd")]

import torch  # noqa: E402

import synth  # noqa: E402
from engine_finetune import FusedAdamW, train_one_epoch  # noqa: E402
from models.losses import AdaLoss  # noqa: E402
from models.vision_transformer_IN21K import vit_base_patch16_224_in21k  # noqa: E402

B, C, R, KEEP, N, ROUNDS = 128, 100, 64, 0.7, 8, 3


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def main():
    dev = torch.device("cuda", 0)
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=R, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                       precision="fp16", train_mode="compact", max_batch=B, input_norm="imagenet")
    model.load_state_dict(synth.make_state_dict(C, R, kind="bench", gate_bias=math.log(KEEP / (1 - KEEP))))
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.to(dev)
    opt = FusedAdamW(model, lr=1e-4, weight_decay=0.01)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=KEEP, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    args = types.SimpleNamespace(accum_iter=1, lr=1e-4, min_lr=1e-4, warmup_epochs=0, epochs=10 ** 6, hip_graph=False)
    src = {"float": [], "u8": [], "u8_nhwc": []}
    for i in range(N):
        y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(500 + i))
        u = synth.make_byte_batch(B, seed=500 + i)
        # the float source is the normalised image of the same bytes, so that the three loops train on the same data
        m, s = (torch.tensor(v).view(1, 3, 1, 1) for v in model.input_norm)
        src["float"].append((((u.float().div(255) - m) / s).pin_memory(), y.pin_memory()))
        src["u8"].append((u.pin_memory(), y.pin_memory()))
        src["u8_nhwc"].append((u.permute(0, 2, 3, 1).contiguous().pin_memory(), y.pin_memory()))
    src["resident"] = [(x.to(dev), y.to(dev)) for x, y in src["float"][:2]]
    src["resident_u8"] = [(x.to(dev), y.to(dev)) for x, y in src["u8"][:2]]

    def epoch(name, steps, e):
        s = src[name]
        t0 = time.perf_counter()
        train_one_epoch(model, crit, [s[i % len(s)] for i in range(steps)], opt, dev, e, None, args=args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    e = 0
    for name in src:   # warm-up of every source (buffers of both dtypes, the copy-stream pick)
        epoch(name, 4, e)
        e += 1
    out = {"batch": B, "precision": "fp16", "distinct_batches": N, "pinned": True, "rounds": ROUNDS,
           "h2d_mb_per_step": {"float": round(B * 3 * 224 * 224 * 4 / 1e6, 1), "u8": round(B * 3 * 224 * 224 / 1e6, 1)},
           "copy_stream_probe": getattr(model._engine, "_copy_stream_probe", (None, None))[1]}
    for steps in (80, 20):
        ms = {name: [] for name in src}
        for _ in range(ROUNDS):
            for name in src:
                ms[name].append(round(epoch(name, steps, e), 3))
                e += 1
        best = {name: min(v) for name, v in ms.items()}
        out["steps_%d" % steps] = {"ms_per_step_all": ms, "ms_per_step_best": best,
                                    "vs_resident": {name: round(best["resident"] / best[name], 4) for name in src},
                                    "images_per_s": {name: round(B / best[name] * 1e3, 1) for name in src}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
