#!/usr/bin/env python3
"""Step time of training fed source images that the device crops, resizes and flips, beside the step fed pre-cropped bytes.

  python tools/resample_speed.py [--batch 128] [--steps 40] [--rounds 3] [--forms plain,crop256,crop512] [--host-batches 1]

One model (default fp16 mode, r = 64, C = 100, compact), uint8 batches resident on the device, a fresh draw per step from
DeviceRandomResizedCrop(generator=seeded).  The forms are timed in alternation, `rounds` windows of `steps` steps each, a host clock around
a window that ends in a device synchronise, after a warm-up of every form; all run eager:
  plain     train_step on a 224 x 224 channels-last byte batch: the step as it was (the only form a library without the entries runs)
  crop256   the loop's _resample_batch on a [B, 256, 256, 3] source batch, then train_step on its output
  crop512   the same from a [B, 512, 512, 3] source batch
Also: `resample_ms`, the two resample launches alone between device events (median of 20 calls per source size, the draws of the timed
steps' generator); `draw_ms`, the host time of one batch's draws; and, when PIL imports, `pillow_ms_per_batch`: the host time of Pillow's
crop + bicubic resize + flip of one batch of the same boxes on one core (--host-batches batches per source size) -- what the feature
takes off the host.  Prints one JSON line.  DYT_LIB_DIR selects another build of the libraries (`plain` runs on one without the entries)."""
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


def pillow_batch_ms(pixels, draw, batches):
    """Host milliseconds per batch of img.crop(box).resize((224, 224), BICUBIC) (+ transpose) over the draw's boxes, one core."""
    try:
        from PIL import Image
    except ImportError:
        return None
    imgs = [Image.fromarray(pixels[i].numpy()) for i in range(pixels.shape[0])]
    t0 = time.perf_counter()
    for _ in range(batches):
        for im, (i, j, h, w), flip in zip(imgs, draw.boxes(), draw.flips()):
            out = im.crop((j, i, j + w, i + h)).resize((224, 224), Image.BICUBIC)
            if flip:
                out = out.transpose(Image.FLIP_LEFT_RIGHT)
    return round((time.perf_counter() - t0) * 1e3 / batches, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="plain,crop256,crop512")
    ap.add_argument("--host-batches", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_speed needs the GPU"
    import engine_finetune as E
    from models.losses import AdaLoss
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    from util.crop import DeviceRandomResizedCrop
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
    opt = E.FusedAdamW(model, lr=1e-4, weight_decay=0.01)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    g = torch.Generator().manual_seed(1)
    forms = [f for f in a.forms.split(",") if f]
    host = {"plain": torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g)}
    for side in (256, 512):
        if "crop%d" % side in forms:
            host["crop%d" % side] = torch.randint(0, 256, (B, side, side, 3), dtype=torch.uint8, generator=g)
    src = {k: v.to(dev) for k, v in host.items()}
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    losses = torch.zeros(8, device=dev)
    cropper = DeviceRandomResizedCrop(generator=torch.Generator().manual_seed(7))
    seed = [0]

    def step(form):
        seed[0] += 1
        x = src[form] if form == "plain" else E._resample_batch(model, cropper, src[form])
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
    resample_ms, draw_ms, pillow_ms = {}, {}, {}
    eng = model._engine
    for f in forms:
        if f == "plain":
            continue
        sizes = [(int(src[f].shape[1]), int(src[f].shape[2]))] * B
        t0 = time.perf_counter()
        draws = [cropper.draw_for(sizes) for _ in range(20)]
        draw_ms[f] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
        times = []
        for d in draws:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.resample(src[f], sizes, d)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        resample_ms[f] = dict(median=round(statistics.median(times), 4), min=round(min(times), 4), max=round(max(times), 4))
        if a.host_batches > 0:
            pillow_ms[f] = pillow_batch_ms(host[f], draws[0], a.host_batches)
    print(json.dumps(dict(tool="resample_speed", lib_dir=os.environ.get("DYT_LIB_DIR", ""), batch=B, precision=a.precision, steps=a.steps,
                          ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                          spread_ms={f: round(max(v) - min(v), 3) for f, v in ms.items()}, resample_ms=resample_ms, draw_ms=draw_ms,
                          pillow_ms_per_batch=pillow_ms, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
