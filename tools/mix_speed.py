#!/usr/bin/env python3
"""Step time of the three ways to train with Mixup / CutMix, and of the plain step beside them.

  python tools/mix_speed.py [--batch 128] [--steps 50] [--rounds 3] [--forms callable,fused,fused_graph,plain,plain_graph]

One model (default fp16 mode, r = 64, C = 100, compact), a uint8 batch resident on the device, a fresh draw per step from
DeviceMixup(mixup_alpha=0.8, cutmix_alpha=1.0).  The forms are timed in alternation, `rounds` windows of `steps` steps each, a host clock
around a window that ends in a device synchronise, after a warm-up of every form:
  callable     today's callable branch: dyt_normalize_u8, then the mix as torch operations on the fp32 batch, class-probability targets
               handed to the library; eager (it cannot be captured)
  fused        train_step(mix=draw) on the bytes and the integer labels, eager
  fused_graph  the same replayed from the captured graph
  plain        no mix, eager;  plain_graph: no mix, graph
Prints one JSON line: ms per step of every window and the median per form.  DYT_LIB_DIR selects another build of the libraries (the plain
forms run on one that has no mix entries)."""
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


def torch_mix(x, y, d, num_classes):
    """What a host-style mixup_fn does on the device tensors: whole-tensor passes over the fp32 batch."""
    if d.mode == 1:
        x = d.lam * x + (1.0 - d.lam) * x.flip(0)
    elif d.mode == 2:
        yl, yh, xl, xh = d.box
        x = x.clone()
        x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
    off = d.smoothing / num_classes
    t = torch.full((y.shape[0], num_classes), off, dtype=torch.float32, device=y.device).scatter_(1, y.view(-1, 1), 1.0 - d.smoothing + off)
    return x, d.lam * t + (1.0 - d.lam) * t.flip(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="callable,fused,fused_graph,plain,plain_graph")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mix_speed needs the GPU"
    from engine_finetune import FusedAdamW, train_step
    from models.losses import AdaLoss
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
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
    seed = [0]

    def step(form):
        seed[0] += 1
        kw = dict(losses_out=losses, seed=seed[0])
        if form == "callable":
            x, t = torch_mix(model.bytes_to_float(u), y, mixer.draw(), C)
            train_step(model, x, t, opt, crit, graph=False, **kw)
        elif form in ("fused", "fused_graph"):
            train_step(model, u, y, opt, crit, graph=form == "fused_graph", mix=mixer.draw(), **kw)
        else:
            train_step(model, u, y, opt, crit, graph=form == "plain_graph", **kw)

    forms = [f for f in a.forms.split(",") if f]
    for f in forms:
        for _ in range(a.warmup):
            step(f)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            for _ in range(2):   # untimed: the callable form's soft targets drop the captured graphs, a graph form re-captures here
                step(f)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(f)
            torch.cuda.synchronize()
            ms[f].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 3))
    assert bool(torch.isfinite(losses).all())
    print(json.dumps(dict(tool="mix_speed", lib_dir=os.environ.get("DYT_LIB_DIR", ""), batch=B, precision=a.precision, steps=a.steps,
                          ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                          hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
