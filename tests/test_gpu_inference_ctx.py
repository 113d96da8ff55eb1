"""GPU tests of the inference-only context (dyt_config.inference_only, ABI v3; pytest -m gpu), all through the C ABI.

An inference-only context runs the SAME eval forward as a training-layout context -- one set of per-block buffers shared by the twelve
blocks, two residual streams in turn, no backward transients, the no-save kernel variants -- so every comparison between the two is
``torch.equal``, not a tolerance.  Contexts are built once per module; the two-context comparisons stay at B <= 23."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import parity_rules as PR  # noqa: E402
import synth  # noqa: E402

PRECISIONS = ["fp32", "fp16x3q", "fp16", "bf16"]   # (bf16: the other library)
C, R, SEED, BMAX = 10, 8, 41, 23


def _tuning(r, ln="none"):
    return D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option=ln, ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=r, d_model=768)


def _model(precision, sd, inference, max_batch, classes=C, r=R, ln="none", video=False):
    if video:
        from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    else:
        from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    m = vit_base_patch16_224_in21k(num_classes=classes, drop_path_rate=0.0, tuning_config=_tuning(r, ln),
                                   select_config=D.Cfg(open=True, keep_layers=0), precision=precision, train_mode="compact",
                                   max_batch=max_batch, inference_only=inference)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda().eval()


def _eval(m, x, complete=False):
    with torch.no_grad():
        logits, aux = m(x, complete_model=complete)
    return logits, aux["token_select"], aux["token_logits"]


def _same(a, b, what):
    for name, ta, tb in zip(("logits", "token_select", "token_logits"), a, b):
        assert ta.shape == tb.shape and torch.equal(ta, tb), "%s: %s differs (max |d| = %.3e)" % (what, name, float((ta - tb).abs().max()))


@pytest.fixture(scope="module")
def images():
    return {n: synth.make_batch(n, C, seed=SEED + n)[0].cuda() for n in (5, 16, BMAX)}


@pytest.fixture(scope="module")
def pairs():
    """precision -> (training-layout model, inference-only model) on the same synthetic weights, built on first use."""
    sd = synth.make_state_dict(C, R, seed=SEED, kind="test", gate_bias=0.85)
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = (_model(precision, sd, False, BMAX), _model(precision, sd, True, BMAX))
        return cache[precision]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_eval_forward_is_bit_equal_to_the_training_layout_context(precision, pairs, images):
    """B = 16 and the ragged B = 23; the student and the complete_model pass (which reuses the one slot); forward_features."""
    normal, inf = pairs(precision)
    for B in (16, BMAX):
        x = images[B]
        _same(_eval(inf, x), _eval(normal, x), "%s B=%d" % (precision, B))
        _same(_eval(inf, x, complete=True), _eval(normal, x, complete=True), "%s B=%d complete_model" % (precision, B))
    fa, aa = inf.forward_features(images[16])
    fb, ab = normal.forward_features(images[16])
    assert torch.equal(fa, fb) and torch.equal(aa["token_select"], ab["token_select"]) and torch.equal(aa["token_logits"], ab["token_logits"])
    assert torch.equal(inf.forward_head(fa), normal.forward_head(fb))
    eng = inf._engine
    assert eng.inference and eng.cfg.inference_only == 1 and not normal._engine.inference
    assert eng.bytes < normal._engine.bytes


@pytest.mark.parametrize("precision", PRECISIONS)
def test_aliased_block_buffers_do_not_leak_between_blocks_or_calls(precision, pairs, images):
    """One LayerS serves all twelve blocks and every call: two consecutive forwards on different inputs, then a smaller batch after the
    largest one (stale rows of the larger pass lie behind it in every buffer), each equal the training-layout context's result."""
    normal, inf = pairs(precision)
    want = {B: _eval(normal, images[B]) for B in (16, BMAX, 5)}
    a = _eval(inf, images[16])
    b = _eval(inf, images[BMAX])
    c5 = _eval(inf, images[5])
    _same(a, want[16], "first of two calls")
    _same(b, want[BMAX], "second of two calls")
    _same(c5, want[5], "B=5 after B=23")
    _same(_eval(inf, images[5], complete=True), _eval(normal, images[5], complete=True), "complete_model B=5 after B=23")


def test_adapter_layernorm_in_model_is_bit_equal(images):
    sd = synth.add_adapter_layernorm(synth.make_state_dict(C, R, seed=SEED, kind="test", gate_bias=0.3), seed=SEED)
    normal, inf = (_model("fp16", sd, i, 16, ln="in") for i in (False, True))
    _same(_eval(inf, images[16]), _eval(normal, images[16]), "adapter_ln=in")
    _same(_eval(inf, images[5], complete=True), _eval(normal, images[5], complete=True), "adapter_ln=in complete_model")


def test_video_model_is_bit_equal():
    """frames > 1: the pooling head's forward buffers stay in an inference-only context."""
    clips, frames, Cv = 2, 2, 7
    sd = synth.make_state_dict(Cv, R, seed=SEED, kind="test", gate_bias=0.85, video=True)
    x, _ = synth.make_batch(clips * frames, Cv, seed=SEED)
    xc = x.reshape(clips, frames, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous().cuda()
    for precision in ("fp32", "fp16"):
        normal, inf = (_model(precision, sd, i, clips * frames, classes=Cv, video=True) for i in (False, True))
        got, want = _eval(inf, xc), _eval(normal, xc)
        assert got[0].shape == (clips, Cv)
        _same(got, want, "video %s" % precision)
        _same(_eval(inf, xc, complete=True), _eval(normal, xc, complete=True), "video %s complete_model" % precision)
        assert inf._engine.inference and inf._engine.frames == frames


@pytest.mark.parametrize("gate_bias", [-60.0, 60.0])
def test_all_dropped_and_all_kept_gates_are_bit_equal(gate_bias):
    """The dispatcher's corner cases as tests/test_gpu_round6.py builds them: -60 drops every patch token of every block, +60 keeps all."""
    B, seed = 3, 37
    sd = synth.make_state_dict(C, R, seed=seed, kind="test", gate_bias=gate_bias)
    x = synth.make_batch(B, C, seed=seed)[0].cuda()
    for precision in ("fp16x3q", "fp16"):
        normal, inf = (_model(precision, sd, i, B) for i in (False, True))
        got, want = _eval(inf, x), _eval(normal, x)
        assert bool((got[1] == (1.0 if gate_bias > 0 else 0.0)).all())
        _same(got, want, "gate bias %+.0f %s" % (gate_bias, precision))


def test_context_bytes_at_batch_128_are_below_a_quarter():
    """dyt_ctx_bytes of the two layouts at max_batch = 128, fp16 (no size query without allocation exists: the contexts are created one
    after the other, the first freed before the second).  24 saved layer sets collapse to one and the backward transients go: the
    layout arithmetic gives well under a tenth; the bar is a quarter."""
    from runtime import DyTEngine
    dev = torch.device("cuda", 0)
    sizes = {}
    for inference in (False, True):
        eng = DyTEngine(100, 64, 0.1, dev, precision="fp16", max_batch=128, inference=inference)
        sizes[inference] = eng.bytes
        del eng
        torch.cuda.empty_cache()
    print("dyt_ctx_bytes at max_batch=128, fp16: training layout %.3f GB, inference-only %.3f GB (%.1f %%)" % (
        sizes[False] / 1e9, sizes[True] / 1e9, 100.0 * sizes[True] / sizes[False]))
    assert sizes[True] < sizes[False] / 4


def test_batch_512_in_one_call_equals_four_chunks_of_128():
    """What the training arena cannot hold: an fp32 eval forward at B = 512 in ONE call.  Against the same context run as four B = 128
    chunks: logits within the fp32 eval tolerance of tests/gpu_diag.py, decisions under the tie rule of tests/parity_rules.py (band from
    the fp32 / fp64 oracle pair on the first two images: the round-off of a gate logit does not depend on the image)."""
    from oracle import dyt_oracle as O
    B, seed = 512, 43
    sd = synth.make_state_dict(C, R, seed=seed, kind="test", gate_bias=0.85)
    m = _model("fp32", sd, True, B)
    x, _ = synth.make_batch(B, C, seed=seed)
    xg = x.cuda()
    whole = _eval(m, xg)
    assert m._engine.cfg.max_batch == B and whole[0].shape == (B, C)
    print("inference-only fp32 context at max_batch=512: %.3f GB" % (m._engine.bytes / 1e9))
    parts = [_eval(m, xg[i:i + 128].contiguous()) for i in range(0, B, 128)]
    chunked = tuple(torch.cat([p[k] for p in parts], dim=0) for k in range(3))
    tol = D.TOL["fp32"]
    err = float((whole[0] - chunked[0]).abs().max())
    flip = (whole[1] != chunked[1])[..., 0].cpu()
    # tie band [depth] in z units: zero noise and all-kept dropout masks make the oracle's training-mode margin z = logit / tau the eval decision's
    n = 2
    zeros = torch.zeros(12, n, 196)
    keep = torch.ones(12, n * 197, R, dtype=torch.uint8)
    with torch.no_grad():
        _, o32 = O.forward(sd, x[:n], zeros, zeros, keep, scale=0.1, training=True, mode="compact")
    band = PR.tie_band(sd, x[:n], zeros, zeros, keep, "compact", o32["token_logits"][..., 0])
    z = (chunked[2][..., 0].cpu().abs() / 5.0)
    nflip, outside, zmax, blk = PR.judge_decisions(flip, z, band)
    print("B=512 in one call vs 4 x 128: logits max |d| %.3e (bound %.0e), %d decision(s) differ, %d outside the tie band" % (err, tol["logits"], nflip, outside))
    assert err <= tol["logits"] and outside == 0
    if nflip == 0:
        assert float((whole[2] - chunked[2]).abs().max()) <= tol["tok_logits"]


def test_training_entries_are_refused_and_the_context_stays_usable(pairs, images):
    """Host-side argument checks: every refusal is raised before anything is enqueued, the text names inference_only, and the context
    still produces the bit-equal eval result afterwards."""
    import engine_finetune as E
    from _lib import DyTError
    normal, inf = pairs("fp16")
    x = images[5]
    want = _eval(normal, x)
    _same(_eval(inf, x), want, "before the refusals")
    eng = inf._engine
    y = torch.zeros(5, dtype=torch.long, device="cuda")
    g = torch.zeros_like(eng.flat)
    calls = {
        "forward(save=True)": lambda: eng.forward(x, save=True),
        "forward(save=True, slot=1)": lambda: eng.forward(x, slot=1, complete_model=True, save=True),
        "backward": lambda: eng.backward(0, torch.zeros(5, C, device="cuda"), g),
        "step_fwd_bwd": lambda: eng.step_fwd_bwd(x, y),
        "train_step": lambda: E.train_step(inf, x, y, optimizer=None),
        "adamw": lambda: eng.adamw(torch.zeros_like(g), torch.zeros_like(g), 1, 1e-3),
        "adamw_guarded": lambda: eng.adamw_guarded(torch.zeros_like(g), torch.zeros_like(g), torch.zeros(4, dtype=torch.int32, device="cuda"), 1e-3),
        "clip_grad_norm": lambda: eng.clip_grad_norm(1.0),
        "set_soft_targets": lambda: eng.set_soft_targets(torch.full((5, C), 1.0 / C, device="cuda")),
    }
    for what, call in calls.items():
        with pytest.raises(DyTError, match="inference_only"):
            call()
    # the library's own answer for an entry that takes the context: DYT_ERR_ARG (-1, include/dyt_hip.h)
    rc = eng.L.dyt_clip_grad_norm(eng.h, ctypes.c_void_p(g.data_ptr()), g.numel(), 1.0, 1.0, None, None)
    assert rc == -1 and b"inference_only" in eng.L.dyt_last_error()
    eng.set_soft_targets(None)
    inf.train()
    with torch.enable_grad(), pytest.raises(DyTError, match="inference_only"):
        inf(x)
    inf.eval()
    torch.cuda.synchronize()
    _same(_eval(inf, x), want, "after the refusals")
    assert inf._engine is eng
