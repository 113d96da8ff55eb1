#!/usr/bin/env python3
"""Step time of video training fed byte clips that the device normalises, resizes, crops and mirrors, beside the step fed pre-cropped float
clips.

  python tools/resample_clip_speed.py [--clips 16] [--frames 8] [--steps 20] [--rounds 3] [--forms float,crop256,crop340] [--host-clips 4]

One video model (default fp16 mode, r = 64, C = 100, compact), clips resident on the device, a fresh draw per step from
DeviceClipScaleJitterCrop (seeded generators).  The forms are timed in alternation, `rounds` windows of `steps` steps each, a host clock
around a window that ends in a device synchronise, after a warm-up of every form; all run eager:
  float     train_step on a float clip batch [B, 3, T, 224, 224]: the step as it was
  crop256   the loop's _resample_batch on a [B, T, 192, 256, 3] byte batch, then train_step on its output
  crop340   the same from a [B, T, 256, 340, 3] byte batch
Also: `resample_ms`, the resample launch alone between device events (median of 20 calls per source size, fresh draws); `draw_ms`, the
host time of one batch's draws; and `host_ms_per_batch`: the host time of the reference's pipeline -- float() / 255, normalise,
torch.nn.functional.interpolate(..., 'bilinear'), crop, flip -- for the same clips and rows with torch on ONE thread (measured on
--host-clips clips and scaled to the batch): what the feature takes off the loader.  Prints one JSON line; run it twice in one command to
see the between-process spread."""
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402

SOURCES = {"crop256": (192, 256), "crop340": (256, 340)}


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def host_batch_ms(clips, draw, norm, n):
    """Host milliseconds per batch of the reference's pipeline over the first ``n`` rows of ``draw``, one thread, scaled to the batch."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    mean, std = torch.tensor(norm[0], dtype=torch.float32), torch.tensor(norm[1], dtype=torch.float32)
    try:
        t0 = time.perf_counter()
        for r in draw.rows[:n]:
            sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags, src = r
            frames = clips[src].float() / 255.
            frames = ((frames - mean) / std).permute(3, 0, 1, 2)[:, :, top:top + bh, left:left + bw]
            full = torch.nn.functional.interpolate(frames, size=(fh, fw), mode="bilinear", align_corners=False)
            out = full[:, :, oy:oy + 224, ox:ox + 224]
            if flags & 1:
                out = out.flip(dims=(-1,))
            out = out.contiguous()
        return round((time.perf_counter() - t0) * 1e3 / n * draw.units, 2)
    finally:
        torch.set_num_threads(threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="float,crop256,crop340")
    ap.add_argument("--host-clips", type=int, default=4)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_clip_speed needs the GPU"
    import engine_finetune as E
    from models.losses import AdaLoss
    from util.crop import DeviceClipScaleJitterCrop
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
    host = {f: torch.randint(0, 256, (B, T) + SOURCES[f] + (3,), dtype=torch.uint8, generator=g) for f in forms if f in SOURCES}
    src = {k: v.to(dev) for k, v in host.items()}
    src["float"] = torch.randn(B, T, 3, 224, 224, generator=g).to(dev).permute(0, 2, 1, 3, 4)   # the layout the device pipeline hands over
    y = torch.randint(0, C, (B,), generator=g).to(dev)
    losses = torch.zeros(8, device=dev)
    cropper = DeviceClipScaleJitterCrop(np_rng=np.random.RandomState(7), generator=torch.Generator().manual_seed(7))
    seed = [0]

    def step(form):
        seed[0] += 1
        x = src[form] if form == "float" else E._resample_batch(model, cropper, src[form])
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
    resample_ms, draw_ms, host_ms = {}, {}, {}
    eng = model._engine
    for f in forms:
        if f == "float":
            continue
        sizes = [SOURCES[f]] * B
        t0 = time.perf_counter()
        draws = [cropper.draw_for(sizes) for _ in range(20)]
        draw_ms[f] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
        times = []
        for d in draws:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.resample_clip(src[f], sizes, d)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        resample_ms[f] = dict(median=round(statistics.median(times), 4), min=round(min(times), 4), max=round(max(times), 4))
        if a.host_clips > 0:
            host_ms[f] = host_batch_ms(host[f], draws[0], eng.input_norm, min(a.host_clips, B))
    print(json.dumps(dict(tool="resample_clip_speed", clips=B, frames=T, precision=a.precision, steps=a.steps,
                          ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                          spread_ms={f: round(max(v) - min(v), 3) for f, v in ms.items()}, resample_ms=resample_ms, draw_ms=draw_ms,
                          host_ms_per_batch=host_ms, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
