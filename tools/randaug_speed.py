#!/usr/bin/env python3
"""Step time of video training fed byte clips that the device augments (RandAugment), normalises, crops and resizes, beside the step with
the device crop alone.

  python tools/randaug_speed.py [--clips 16] [--frames 8] [--steps 20] [--rounds 3] [--forms crop256,aug256,crop340,aug340] [--config STR]

One video model (default fp16 mode, r = 64, C = 100, compact), clips resident on the device, a fresh draw per step from
DeviceClipRandomResizedCrop and DeviceRandAugment (seeded generators).  The forms are timed in alternation, `rounds` windows of `steps`
steps each, a host clock around a window that ends in a device synchronise, after a warm-up of every form; all run eager:
  crop256   the loop's _resample_batch on a [B, T, 192, 256, 3] byte batch, then train_step on its output: the step as it was
  aug256    the loop's _randaug_clip_batch in front of it (the SSV2 recipe 'rand-m7-n4-mstd0.5-inc1', bicubic)
  crop340 / aug340   the same from a [B, T, 256, 340, 3] byte batch
Also, per source size: `randaug_ms`, the augmentation launches alone between device events (median of 20 fresh draws), `draw_ms`, the host
time of one batch's draws, and `parts_ms`: the same between device events for batches in which EVERY unit runs one operation in one layer
-- invert (table, no histograms), equalize (histograms + table), contrast (histograms + blend), color (blend), sharpness, affine_bilinear,
affine_bicubic (a 20 degree rotation) -- so equalize - invert is the statistics pass and the families can be told apart.  Prints one JSON
line; run it twice in one command to see the between-process spread."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-tuning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402

SOURCES = {"256": (192, 256), "340": (256, 340)}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def timed(fn, n=20):
    times = []
    for i in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(median=round(statistics.median(times), 4), min=round(min(times), 4), max=round(max(times), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="crop256,aug256,crop340,aug340")
    ap.add_argument("--config", default="rand-m7-n4-mstd0.5-inc1")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "randaug_speed needs the GPU"
    import engine_finetune as E
    from models.losses import AdaLoss
    from util import randaug as RA
    from util.crop import DeviceClipRandomResizedCrop
    from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    B, T, C, r = a.clips, a.frames, 100, 64
    dev = torch.device("cuda", 0)
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                       precision=a.precision, train_mode="compact", max_batch=B * T, input_norm="imagenet")
    model.load_state_dict(synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85, video=True))
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    model = model.to(dev).train()
    opt = E.FusedAdamW(model, lr=1e-4, weight_decay=0.01)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    g = torch.Generator().manual_seed(1)
    forms = [f for f in a.forms.split(",") if f]
    sizes_used = sorted({f[-3:] for f in forms})
    src = {s: torch.randint(0, 256, (B, T) + SOURCES[s] + (3,), dtype=torch.uint8, generator=g).to(dev) for s in sizes_used}
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    losses = torch.zeros(8, device=dev)
    cropper = DeviceClipRandomResizedCrop(py_rng=random.Random(7), np_rng=np.random.RandomState(7))
    augmenter = RA.DeviceRandAugment(a.config, interpolation="bicubic", py_rng=random.Random(11), np_rng=np.random.RandomState(11))
    seed = [0]

    def step(form):
        seed[0] += 1
        x = src[form[-3:]]
        if form.startswith("aug"):
            x = E._randaug_clip_batch(model, augmenter, x, True)
        x = E._resample_batch(model, cropper, x)
        E.train_step(model, x, y, opt, crit, graph=False, losses_out=losses, seed=seed[0])

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
    eng = model._engine
    randaug_ms, draw_ms, parts_ms, applied = {}, {}, {}, {}
    for s in sizes_used:
        h, w = SOURCES[s]
        sizes = [(h, w)] * B
        t0 = time.perf_counter()
        draws = [augmenter.draw_for(sizes) for _ in range(20)]
        draw_ms[s] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
        applied[s] = round(sum(1 for d in draws for r in d.rows if r[0] != RA.IDENTITY) / (20.0 * B), 3)
        randaug_ms[s] = timed(lambda i: eng.randaug(src[s], sizes, draws[i]))
        rot = RA.rotate_coeffs(20.0, h, w)
        one = {"invert": RA.aug_row(RA.INVERT, h, w), "equalize": RA.aug_row(RA.EQUALIZE, h, w), "contrast": RA.aug_row(RA.CONTRAST, h, w, factor=1.6),
               "color": RA.aug_row(RA.COLOR, h, w, factor=1.6), "sharpness": RA.aug_row(RA.SHARPNESS, h, w, factor=1.6),
               "affine_bilinear": RA.aug_row(RA.AFFINE, h, w, coeffs=rot, filter=RA.BILINEAR), "affine_bicubic": RA.aug_row(RA.AFFINE, h, w, coeffs=rot, filter=RA.BICUBIC)}
        parts_ms[s] = {}
        for name, row in one.items():
            d = RA.AugDraw([row] * B, 1)
            eng.randaug(src[s], sizes, d)   # warm
            parts_ms[s][name] = timed(lambda i: eng.randaug(src[s], sizes, d))
    print(json.dumps(dict(tool="randaug_speed", clips=B, frames=T, precision=a.precision, steps=a.steps, config=a.config,
                          ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                          spread_ms={f: round(max(v) - min(v), 3) for f, v in ms.items()}, randaug_ms=randaug_ms, applied_ops_per_clip=applied,
                          draw_ms=draw_ms, parts_ms=parts_ms, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
