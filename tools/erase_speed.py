#!/usr/bin/env python3
"""Step time of training with Random Erasing on the device, and of the step without it beside them.

  python tools/erase_speed.py [--batch 128] [--steps 50] [--rounds 3] [--forms off,erase,erase_mix,callable]

One model (default fp16 mode, r = 64, C = 100, compact), a uint8 batch resident on the device, a fresh draw per step from
DeviceRandomErasing(probability=0.25, mode='pixel') (and DeviceMixup(mixup_alpha=0.8, cutmix_alpha=1.0)).  The forms are timed in
alternation, `rounds` windows of `steps` steps each, a host clock around a window that ends in a device synchronise, after a warm-up of
every form; all run eager:
  off        train_step on the bytes, erasing off: the kernels of a library without the feature
  erase      train_step(erase=draw) on the bytes
  erase_mix  train_step(erase=draw, mix=draw) on the bytes and the integer labels
  callable   DeviceRandomErasing.__call__ to fp32 images (dyt_erase_images), then train_step on those
Prints one JSON line: ms per step of every window and the median per form.  DYT_LIB_DIR selects another build of the libraries (`off`
runs on one that has no erase entries)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-tuning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import synth  # noqa: E402


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="off,erase,erase_mix,callable")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "erase_speed needs the GPU"
    from engine_finetune import FusedAdamW, train_step
    from models.losses import AdaLoss
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    from util.erasing import DeviceRandomErasing
    from util.mixup import DeviceMixup
    B, C, r = a.batch, 100, 64
    dev = torch.device("cuda", 0)
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                       precision=a.precision, train_mode="compact", max_batch=B, input_norm="imagenet")
    model.load_state_dict(synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85))
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.to(dev).train()
    opt = FusedAdamW(model, lr=1e-4, weight_decay=0.01)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    g = torch.Generator().manual_seed(1)
    u = torch.randint(0, 256, (B, 3, 224, 224), dtype=torch.uint8, generator=g).to(dev)
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    losses = torch.zeros(8, device=dev)
    mixer = DeviceMixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C, generator=7)
    eraser = DeviceRandomErasing(probability=0.25, mode="pixel", generator=7)
    seed = [0]

    def step(form):
        seed[0] += 1
        kw = dict(losses_out=losses, seed=seed[0])
        if form == "callable":
            train_step(model, eraser(u, norm=model.input_norm), y, opt, crit, graph=False, **kw)
        elif form == "erase":
            train_step(model, u, y, opt, crit, graph=False, erase=eraser.draw_for(B), **kw)
        elif form == "erase_mix":
            train_step(model, u, y, opt, crit, graph=False, erase=eraser.draw_for(B), mix=mixer.draw(), **kw)
        else:
            train_step(model, u, y, opt, crit, graph=False, **kw)

    forms = [f for f in a.forms.split(",") if f]
    for f in forms:
        for _ in range(a.warmup):
            step(f)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            for _ in range(2):   # untimed: the switch between forms
                step(f)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(f)
            torch.cuda.synchronize()
            ms[f].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 3))
    assert bool(torch.isfinite(losses).all())
    print(json.dumps(dict(tool="erase_speed", lib_dir=os.environ.get("DYT_LIB_DIR", ""), batch=B, precision=a.precision, steps=a.steps,
                          ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                          hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
