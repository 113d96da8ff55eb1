"""GPU tests of the streaming form of engine_finetune.evaluate / evaluate_video (args.stream_eval, DYT_STREAM_EVAL=1; util.metrics.StreamingEval
over dyt_eval_rows / dyt_eval_keep) against the gather form on the same model and loader, the reference's goldens, and tests/eval_refs.py /
block_flops_dict.batch_select_flops on the gather form's own logits and masks."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import eval_refs as R  # noqa: E402
import gpu_diag as D  # noqa: E402
import synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda", 0)


def _args(metric, C, stream):
    return types.SimpleNamespace(metric=metric, nb_classes=C, stream_eval=stream)


def _gather_tensors(model, loader, video=False):
    """What the gather form concatenates: the logits and masks of the same eval forwards."""
    model.eval()
    logits, masks, ys = [], [], []
    with torch.no_grad():
        for x, y in loader:
            x = x.cuda()
            if video:
                B, V = x.shape[:2]
                out, aux = model(x.flatten(0, 1))
                out = out.view(B, V, -1).mean(dim=1)
            else:
                out, aux = model(x)
            logits.append(out.float().cpu())
            masks.append(aux["token_select"].float().cpu())
            ys.append(y)
    return torch.cat(logits), torch.cat(masks), torch.cat(ys)


def _compare(stream, gather, logits, masks, y, C, table=None, base=None):
    """The streaming status against the gather status (same model, same loader) and against the references on the gather form's tensors."""
    from block_flops_dict import batch_select_flops
    from util.metrics import accuracy, mean_per_class_accuracy
    assert stream["metric"] == gather["metric"]
    for k in ("acc1", "acc5"):
        if k in gather:
            assert stream[k] == gather[k], (k, stream[k], gather[k])
    a1, a5 = accuracy(logits.cuda(), y.cuda(), topk=(1, 5))   # on the device, where the gather form evaluates them
    assert stream["acc1"] == a1.item() and stream["acc5"] == a5.item()
    assert stream["mean_per_class_acc"] == mean_per_class_accuracy(logits.cuda(), y.cuda(), C).item()
    assert abs(stream["keep_ratio"] - gather["keep_ratio"]) <= 4 * 2.0 ** -24 * gather["keep_ratio"]   # two fp32 roundings of torch's mean against an exact ratio
    assert stream["n"] == y.shape[0] and stream["ignored"] == 0 and stream["nan_rows"] == 0
    _, loss64 = R.rows(logits.double(), y)
    _, loss32 = R.rows(logits, y)
    want = F.cross_entropy(logits.double(), y, reduction="none")
    assert float((want - loss64).abs().max()) < 1e-12
    floor, bound = R.loss_bound(loss64, loss32)
    err = abs(stream["loss"] - float(want.mean()))
    print("stream eval loss %.6f (fp64 of the gather logits %.6f): error %.2e floor %.2e bound %.2e" % (stream["loss"], float(want.mean()), err, floor, bound))
    assert err <= bound
    per_layer = masks[..., 0].double().mean(dim=(0, 2))
    assert len(stream["keep_ratio_per_layer"]) == 12 and max(abs(a - float(b)) for a, b in zip(stream["keep_ratio_per_layer"], per_layer)) < 1e-12
    assert abs(stream["keep_ratio"] - float(masks.double().mean())) < 1e-12
    if table is not None:
        want_fl = float(batch_select_flops(masks.shape[0], table, masks, block_num=12, base_flops=base).mean())
        assert abs(stream["gflops"] - want_fl) <= 16 * 2.0 ** -24 * want_fl, (stream["gflops"], want_fl)
    else:
        assert "gflops" not in stream


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_streaming_equals_gather_on_eval_acc_golden(prec):
    from block_flops_dict import BASE_FLOPS_IN21K, get_block_flops
    from engine_finetune import evaluate
    g = dict(np.load(os.path.join(GOLDEN, "eval_acc.npz")))
    B, C = int(g["meta_batch"]), int(g["meta_num_classes"])
    x, _ = synth.make_batch(B, C, seed=int(g["meta_seed"]))
    y = torch.from_numpy(g["targets"])
    loader = [(x[:5], y[:5]), (x[5:9], y[5:9]), (x[9:], y[9:])]   # the ragged loader of test_gpu_round2.py
    model, _ = D.build_model(g, prec)
    logits, masks, ys = _gather_tensors(model, loader)
    table = get_block_flops(ffn_num=int(g["meta_ffn_num"]))
    for metric in ("accuracy", "mean_per_class_acc"):
        gather = evaluate(loader, model, DEV, None, None, None, _args(metric, C, False))
        stream = evaluate(loader, model, DEV, None, BASE_FLOPS_IN21K, table, _args(metric, C, True))
        assert set(gather) <= set(stream)
        _compare(stream, gather, logits, masks, ys, C, table, BASE_FLOPS_IN21K)
        assert abs(stream["acc1"] - float(g["metric_accuracy"])) < 1e-5 and abs(stream["acc5"] - float(g["acc5"])) < 1e-5
        assert abs(stream["mean_per_class_acc"] - float(g["metric_mean_per_class_acc"])) < 1e-4
        assert abs(stream["keep_ratio"] - float(g["token_select_mean"])) < (1e-6 if prec == "fp32" else 3e-3)
    assert stream["metric"] == stream["mean_per_class_acc"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_streaming_equals_gather_on_eval_r64_golden(prec):
    from engine_finetune import evaluate
    g = dict(np.load(os.path.join(GOLDEN, "eval_r64.npz")))
    B, C = int(g["meta_batch"]), int(g["meta_num_classes"])
    x, y = synth.make_batch(B, C, seed=int(g["meta_seed"]))
    loader = [(x[:3], y[:3]), (x[3:], y[3:])]
    model, _ = D.build_model(g, prec)
    logits, masks, ys = _gather_tensors(model, loader)
    gather = evaluate(loader, model, DEV, None, None, None, _args("accuracy", C, False))
    stream = evaluate(loader, model, DEV, None, None, None, _args("accuracy", C, True))
    _compare(stream, gather, logits, masks, ys, C)
    assert abs(stream["metric"] - float(g["metric"])) < 1e-9
    assert abs(stream["keep_ratio"] - float(g["token_select"].mean())) < (1e-6 if prec == "fp32" else 2e-3)


def test_env_switch_and_default(monkeypatch):
    """DYT_STREAM_EVAL=1 takes the streaming branch for drivers that pass no stream_eval; without either, the gather form runs."""
    import engine_finetune as E
    g = dict(np.load(os.path.join(GOLDEN, "eval_r64.npz")))
    B, C = int(g["meta_batch"]), int(g["meta_num_classes"])
    x, y = synth.make_batch(B, C, seed=int(g["meta_seed"]))
    loader = [(x[:3], y[:3]), (x[3:], y[3:])]
    model, _ = D.build_model(g, "fp32")
    args = types.SimpleNamespace(metric="accuracy", nb_classes=C)
    monkeypatch.delenv("DYT_STREAM_EVAL", raising=False)
    assert not E.stream_eval_requested(args) and not E.stream_eval_requested(None)
    plain = E.evaluate(loader, model, DEV, None, None, None, args)
    assert set(plain) == {"metric", "acc1", "acc5", "keep_ratio"}
    monkeypatch.setenv("DYT_STREAM_EVAL", "1")
    assert E.stream_eval_requested(args)
    st = E.evaluate(loader, model, DEV, None, None, None, args)
    assert "loss" in st and "keep_ratio_per_layer" in st and st["metric"] == plain["metric"] and st["acc5"] == plain["acc5"]
    monkeypatch.setenv("DYT_STREAM_EVAL", "0")
    assert set(E.evaluate(loader, model, DEV, None, None, None, args)) == set(plain)


def test_video_two_clips_two_views():
    from block_flops_dict import BASE_FLOPS_IN21K, get_block_flops
    from engine_finetune import evaluate_video
    from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    C, r, t = 7, 8, 2
    sd = synth.make_state_dict(C, r, seed=3, kind="test", gate_bias=0.3, video=True)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                   precision="fp32", train_mode="compact", max_batch=2 * 2 * t)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    frames, _ = synth.make_batch(2 * 2 * t, C, seed=9)
    clips = frames.reshape(2, 2, t, 3, 224, 224).permute(0, 1, 3, 2, 4, 5).contiguous()   # [B, V, c, t, h, w]
    y = torch.tensor([1, 4])
    loader = [(clips[:1], y[:1]), (clips[1:], y[1:])]
    logits, masks, ys = _gather_tensors(m, loader, video=True)
    table = get_block_flops(ffn_num=r)
    gather = evaluate_video(loader, m, DEV, None, BASE_FLOPS_IN21K, table, _args("accuracy", C, False))
    stream = evaluate_video(loader, m, DEV, None, BASE_FLOPS_IN21K, table, _args("accuracy", C, True))
    assert set(gather) <= set(stream)
    _compare(stream, gather, logits, masks, ys, C, table, BASE_FLOPS_IN21K)
    assert abs(stream["gflops"] - gather["gflops"]) <= 16 * 2.0 ** -24 * gather["gflops"]
    assert masks.shape[0] == 2 * 2 * t


def test_wide_head_inference_only_model():
    from engine_finetune import evaluate
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    C, r, B = 1025, 8, 3
    sd = synth.make_state_dict(C, r, seed=5, kind="test", gate_bias=0.3)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                   precision="fp16", train_mode="compact", max_batch=B, inference_only=True, wide_head=True)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    x, y = synth.make_batch(B, C, seed=11)
    loader = [(x, y)]
    logits, masks, ys = _gather_tensors(m, loader)
    y = logits.topk(3, dim=1).indices[torch.arange(B), torch.tensor([0, 2, 1])]   # a top-1 hit, and two inside the top 5
    loader = [(x, y)]
    gather = evaluate(loader, m, DEV, None, None, None, _args("accuracy", C, False))
    stream = evaluate(loader, m, DEV, None, None, None, _args("accuracy", C, True))
    _compare(stream, gather, logits, masks, y, C)
    assert stream["acc5"] == 100.0 and 0.0 < stream["acc1"] < 100.0


class _Resident:
    """12 equal batches that live on the device; records torch.cuda.memory_allocated() each time the loop comes back for a batch."""

    def __init__(self, x, y, n=12):
        self.x, self.y, self.n, self.seen = x, y, n, []

    def __iter__(self):
        self.seen = []
        for _ in range(self.n):
            self.seen.append(torch.cuda.memory_allocated())
            yield self.x, self.y
        self.seen.append(torch.cuda.memory_allocated())


def test_memory_does_not_grow_with_the_number_of_batches():
    from engine_finetune import evaluate
    g = dict(np.load(os.path.join(GOLDEN, "eval_r64.npz")))
    C = int(g["meta_num_classes"])
    x, y = synth.make_batch(2, C, seed=1)
    model, _ = D.build_model(g, "fp32")
    loader = _Resident(x.cuda(), y.cuda())
    evaluate(loader, model, DEV, None, None, None, _args("accuracy", C, True))
    assert len(loader.seen) == 13
    assert loader.seen[3] == loader.seen[12], loader.seen   # after batch 3 == after batch 12
    evaluate(loader, model, DEV, None, None, None, _args("accuracy", C, False))
    assert loader.seen[12] > loader.seen[3], loader.seen    # the gather form holds every batch
