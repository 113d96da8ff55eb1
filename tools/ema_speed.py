#!/usr/bin/env python3
"""Cost of the model EMA: the update launch alone, and the training step through train_one_epoch with it off and on.

  python tools/ema_speed.py [--part kernel,step] [--batch 128] [--steps 40] [--rounds 3] [--forms off_eager,ema_eager,off_graph,ema_graph]

kernel  dyt_ema_update at the n_train of the B = `batch` context (r = 64, C = 100): HIP events around `--launches` back-to-back launches after
        a warm-up, `rounds` times; microseconds per launch and the 12 bytes per element (two reads, one write) over that time.  Back-to-back
        launches on one stream: the figure is the launch-to-launch period, which is what the step pays.
step    One model (default fp16 mode, compact), a float batch resident on the device, `train_one_epoch` over a loader of `steps` batches as
        one window -- a host clock around the call, which ends in the loop's own read-back.  The forms are timed in alternation, `rounds`
        windows each, after a warm-up epoch of every form: EMA off / on (args.model_ema = DeviceModelEma(model, 0.9998)), eager / captured
        graph (args.hip_graph).
Prints one JSON line.  DYT_LIB_DIR selects another build of the libraries; one without dyt_ema_update runs the `off` forms only."""
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

import synth  # noqa: E402


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


class Resident:
    def __init__(self, x, y, n):
        self.x, self.y, self.n = x, y, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for _ in range(self.n):
            yield self.x, self.y


def build(a, dev):
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    C, r = 100, 64
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    model = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=Cfg(open=True, keep_layers=0),
                                       precision=a.precision, train_mode="compact", max_batch=a.batch)
    model.load_state_dict(synth.make_state_dict(C, r, seed=0, kind="test", gate_bias=0.85))
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return model.to(dev).train(), C


def kernel(a, model, dev):
    eng = model.engine(a.batch, dev)
    shadow = eng.flat.clone()
    for _ in range(20):
        eng.ema_update(shadow, 0.9998)
    us = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            eng.ema_update(shadow, 0.9998)
        e1.record()
        torch.cuda.synchronize()
        us.append(round(e0.elapsed_time(e1) * 1e3 / a.launches, 3))
    med = statistics.median(us)
    return dict(n_train=eng.n_train, bytes=12 * eng.n_train, launches=a.launches, us_per_launch=us, median_us=med,
                gbps=round(12 * eng.n_train / (med * 1e-6) / 1e9, 1))


def step(a, model, C, dev):
    from engine_finetune import FusedAdamW, train_one_epoch
    from models.losses import AdaLoss
    have = hasattr(model.engine(a.batch, dev).L, "dyt_ema_update")
    forms = [f for f in a.forms.split(",") if f and (have or not f.startswith("ema"))]
    opt = FusedAdamW(model, lr=1e-4, weight_decay=0.01)
    crit = AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.0, token_minimal_weight=0.0)
    x, y = synth.make_batch(a.batch, C, seed=1)
    loader = Resident(x.to(dev), y.to(dev), a.steps)
    ema = None
    if have:
        from util.model_ema import DeviceModelEma
        ema = DeviceModelEma(model, 0.9998)

    def args_of(form):
        ns = types.SimpleNamespace(accum_iter=1, lr=1e-4, min_lr=1e-6, warmup_epochs=0, epochs=1000, hip_graph=form.endswith("graph"))
        if form.startswith("ema"):
            ns.model_ema = ema
        return ns

    def epoch(form, n):
        loader.n = n
        train_one_epoch(model, crit, loader, opt, dev, 0, None, 0, None, None, args=args_of(form))
    for f in forms:
        epoch(f, a.warmup)
    torch.cuda.synchronize()
    ms = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            epoch(f, 2)   # untimed: the switch between forms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            epoch(f, a.steps)
            torch.cuda.synchronize()
            ms[f].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 3))
    return dict(steps=a.steps, ms_per_step=ms, median_ms={f: statistics.median(v) for f, v in ms.items()},
                ema_updates=None if ema is None else ema.updates, applied_and_skipped=opt.applied_and_skipped())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="kernel,step")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--forms", default="off_eager,ema_eager,off_graph,ema_graph")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ema_speed needs the GPU"
    os.environ.setdefault("DYT_PREFETCH", "0")   # the batch is resident: no copy stream to probe for
    dev = torch.device("cuda", 0)
    model, C = build(a, dev)
    res = dict(tool="ema_speed", lib_dir=os.environ.get("DYT_LIB_DIR", ""), batch=a.batch, precision=a.precision, rounds=a.rounds,
               hw_queues=os.environ.get("GPU_MAX_HW_QUEUES", ""))
    if "kernel" in a.part and hasattr(model.engine(a.batch, dev).L, "dyt_ema_update"):
        res["kernel"] = kernel(a, model, dev)
    if "step" in a.part:
        res["step"] = step(a, model, C, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
