#!/usr/bin/env python3
"""The wide-tap device crop (any_scale=True; csrc/resample_wide.hip) timed: its launches alone beside the 11-tap route's, the training step
fed large sources beside the step fed pre-cropped bytes, and the host cost that leaves the loader.

  python tools/resample_wide_speed.py [--batch 128] [--steps 30] [--rounds 3] [--calls 20] [--sizes 512x512,1200x1600,2400x3200]
                                      [--step-size 1200x1600] [--host-batches 1]

One model (default fp16 mode, r = 64, C = 100, compact), uint8 source batches resident on the device, a fresh draw per call from
DeviceRandomResizedCrop(any_scale=True, generator=seeded) -- the reference's scale=(0.08, 1.0), ratio=(3/4, 4/3).
  launch_ms    per source size, DyTEngine.resample between device events, `calls` calls per window, `rounds` windows per route in
               alternation: `wide` (three launches) on every size; `narrow` (two launches) on the same draws where every box is at most
               2.5 x 224 a side, i.e. at 512 x 512 only.  Median, min and max over all calls of a route.
  ms_per_step  `plain` = train_step on a 224 x 224 byte batch, `wide` = the loop's _resample_batch on a --step-size source batch and then
               train_step on its output; `rounds` windows of `steps` steps each in alternation, a host clock around a window that ends in a
               device synchronise, after a warm-up of both; all eager.
  pillow_ms_per_batch  when PIL imports: the host time of Pillow's crop + bicubic resize + flip of one batch of the same boxes on one core.
  draw_ms      the host time of one batch's draws.
Prints one JSON line."""
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


def _size(text):
    h, w = text.lower().split("x")
    return int(h), int(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--sizes", default="512x512,1200x1600,2400x3200")
    ap.add_argument("--step-size", default="1200x1600")
    ap.add_argument("--host-batches", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_wide_speed needs the GPU"
    import engine_finetune as E
    from models.losses import AdaLoss
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    from util.crop import CropDraw, DeviceRandomResizedCrop
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
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randint(0, C, (B,), generator=g, device=dev)
    plain = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=g, device=dev)
    losses = torch.zeros(8, device=dev)
    cropper = DeviceRandomResizedCrop(any_scale=True, generator=torch.Generator().manual_seed(7))
    eng = model.engine(B, dev)

    # ---- the launches alone ----------------------------------------------------------------------------------------------------------------
    launch_ms, draw_ms, pillow_ms, scratch_mb = {}, {}, {}, {}
    step_size = _size(a.step_size)
    step_src = None
    for text in [s for s in a.sizes.split(",") if s]:
        hs, ws = _size(text)
        src = torch.randint(0, 256, (B, hs, ws, 3), dtype=torch.uint8, generator=g, device=dev)
        sizes = [(hs, ws)] * B
        t0 = time.perf_counter()
        draws = [cropper.draw_for(sizes) for _ in range(a.calls)]
        draw_ms[text] = round((time.perf_counter() - t0) * 1e3 / a.calls, 3)
        routes = {"wide": draws}
        if all(2 * max(r_[4], r_[5]) <= 5 * 224 for d in draws for r_ in d.rows):
            routes["narrow"] = [CropDraw(d.rows) for d in draws]      # the same rows for the 11-tap entry
        for ds in routes.values():      # warm-up: code objects, the wide scratch of this height
            eng.resample(src, sizes, ds[0])
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, ds in routes.items():
                for d in ds:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.resample(src, sizes, d)
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1))
        launch_ms[text] = {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in times.items()}
        launch_ms[text]["mean_box"] = [round(statistics.mean(r_[4] for d in draws for r_ in d.rows), 1),
                                       round(statistics.mean(r_[5] for d in draws for r_ in d.rows), 1)]
        scratch_mb[text] = round(eng._rsw_scratch.numel() * 4 / 2 ** 20, 1)
        if a.host_batches > 0 and (hs, ws) == step_size:
            pillow_ms[text] = pillow_batch_ms(src.cpu(), draws[0], a.host_batches)
        if (hs, ws) == step_size:
            step_src = src
        del src
    if step_src is None:
        step_src = torch.randint(0, 256, (B,) + step_size + (3,), dtype=torch.uint8, generator=g, device=dev)

    # ---- the step --------------------------------------------------------------------------------------------------------------------------
    seed = [0]

    def step(form):
        seed[0] += 1
        x = plain if form == "plain" else E._resample_batch(model, cropper, step_src)
        E.train_step(model, x, y, opt, crit, graph=False, losses_out=losses, seed=seed[0])

    forms = ["plain", "wide"]
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
    print(json.dumps(dict(tool="resample_wide_speed", batch=B, precision=a.precision, steps=a.steps, calls=a.calls, rounds=a.rounds,
                          launch_ms=launch_ms, wide_scratch_mb=scratch_mb, step_size=a.step_size, ms_per_step=ms,
                          median_ms={f: statistics.median(v) for f, v in ms.items()},
                          spread_ms={f: round(max(v) - min(v), 3) for f, v in ms.items()}, draw_ms=draw_ms,
                          pillow_ms_per_batch=pillow_ms, hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))))


if __name__ == "__main__":
    main()
