"""GPU tests of the on-device Random Erasing (pytest -m gpu): dyt_erase_images, and dyt_set_erase -- the erasing fused into the
patch-embedding load of the training forward and the fused step, before the mix, driven by util.erasing.DeviceRandomErasing through
train_one_epoch.

The fused path is defined as the float path on the erased (then mixed) image (tests/erase_refs.py, tests/mix_refs.py), so every comparison
of `const` mode and every comparison between two device paths is exact and made on the raw bits (``_same_bits``).  The noise of `rand` /
`pixel` mode is compared with the float64 evaluation of the same formula on the same Philox words within ``erase_refs.noise_bound`` =
4 x the largest deviation of the formula in numpy float32 from float64 over the comparison's own words (about 1.6e-6 x 4; the factor
covers the device's 1-2 ulp logf / sinf / cosf).  B = 4, r = 8, C = 10; engines have depth 1, the training loops depth 2."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import erase_refs as R  # noqa: E402
import gpu_diag as D  # noqa: E402
import input_u8_refs as U  # noqa: E402
import mix_refs as MR  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, BMAX, SMOOTH = 10, 8, 83, 4, 0.1
DEV = torch.device("cuda", 0)
NORM = U.STATS["imagenet"]
NOISE_SEED = 0x243F6A8885A308D3

# where an off-by-one shows: the corner, a box ending at row and column 223, a 1 x 1 box; boxes that straddle a 4-pixel and a 16-pixel run
# boundary; two overlapping boxes; an image with no box
BOXES = [[(0, 5, 0, 7), (200, 24, 190, 34), (100, 1, 101, 1)],
         [(10, 3, 3, 2), (20, 3, 15, 2)],
         [(30, 50, 30, 50), (60, 50, 60, 50)],
         []]


def _draw(mode, boxes=BOXES, seed=NOISE_SEED, **kw):
    from util.erasing import EraseDraw
    return EraseDraw(mode, boxes, seed=seed, **kw)


def _same_bits(got, want, what):
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = got.view(torch.int32) != want.view(torch.int32)
        raise AssertionError("%s: %d of %d values differ in their bits (max |d| = %.3e)" % (
            what, int(bad.sum()), bad.numel(), float((got - want)[bad].abs().nan_to_num(float("inf")).max())))


def _table(draw, capacity=None):
    return torch.frombuffer(bytearray(draw.words(capacity)), dtype=torch.int32).to(DEV)


def _mix_params(d):
    return torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(DEV)


def _erase(x, draw, frames=1, mix=None):
    from _lib import erase_images
    norm = NORM if x.dtype == torch.uint8 else None
    return erase_images(x.cuda(), _table(draw, x.shape[0]), frames=frames, norm=norm, mix_params=None if mix is None else _mix_params(mix)).cpu()


@pytest.fixture(scope="module")
def data():
    """Byte batch (B = 4), its channels-last twin, the CPU-normalised floats, an unrelated float batch whose box-less image 3 holds NaN, inf
    and -0.0, and labels: computed once, read only."""
    u = U.byte_images(BMAX, seed=SEED)
    xf = synth.make_batch(BMAX, C, seed=SEED)[0].clone()
    xf[3, 0, 0, 0], xf[3, 1, 100, 101], xf[3, 2, 223, 223] = float("nan"), float("inf"), float("-inf")
    xf[3, :, 10:13, ::3] = -0.0
    return types.SimpleNamespace(u=u, nhwc=U.to_nhwc(u), xn=U.normalize_cpu(u, "imagenet"), xf=xf, y=torch.tensor([3, 7, 7, 0], dtype=torch.int64))


@pytest.fixture(scope="module")
def bound():
    b = R.noise_bound(NOISE_SEED, BMAX)
    print("noise bound over the test's own words: %.3e" % b)
    assert 0 < b < 2e-5
    return b


def _kinds(data):
    return (("fp32", data.xf, data.xf), ("u8 nchw", data.u, data.xn), ("u8 nhwc", data.nhwc, data.xn))


# ---- 1. const ----------------------------------------------------------------------------------------------------------------------------------
def test_const_mode_equals_the_reference_bit_for_bit(data):
    d = _draw("const")
    hit = R.hit_map(d, BMAX) >= 0
    assert hit[0, 0, 0] and hit[0, 223, 223] and hit[0, 100, 101] and hit[0].sum() == 35 + 24 * 34 + 1 and not hit[3].any()
    for what, src, normalised in _kinds(data):
        got = _erase(src, d)
        _same_bits(got, R.erase_ref(normalised, d), "const, " + what)
        assert bool((got[:3][torch.from_numpy(hit[:3])[:, None].expand(3, 3, 224, 224)] == 0).all())
    got = _erase(data.xf, d)
    _same_bits(got[3], data.xf[3], "the image without a box: NaN, inf and -0.0 pass")
    assert bool(torch.isnan(got[3, 0, 0, 0])) and bool((got[3].view(torch.int32)[:, 10:13, ::3] == -2 ** 31).all())
    # two images, and a table with more rows than images
    from _lib import erase_images
    _same_bits(erase_images(data.u[:2].cuda(), _table(d, 7), norm=NORM), R.erase_ref(data.xn[:2], _draw("const", BOXES[:2])), "2 images, 7 rows")


# ---- 2. pixel ----------------------------------------------------------------------------------------------------------------------------------
def test_pixel_mode_noise_is_the_reference_noise(data, bound):
    d = _draw("pixel")
    inside = torch.from_numpy(R.hit_map(d, BMAX) >= 0)[:, None].expand(BMAX, 3, 224, 224)
    want = R.pixel_noise(NOISE_SEED, BMAX)
    outs = {}
    for what, src, normalised in _kinds(data):
        got = outs[what] = _erase(src, d)
        assert torch.equal(got.view(torch.int32)[~inside], normalised.view(torch.int32)[~inside]), what   # outside the boxes: the input's bits
        err = float(np.abs(got.numpy().astype(np.float64) - want)[inside.numpy()].max())
        print("pixel %s: max |device - fp64| = %.3e over %d values (bound %.3e)" % (what, err, int(inside.sum()), bound))
        assert err <= bound, (what, err, bound)
    for what in ("u8 nchw", "u8 nhwc"):   # inside: the three kernel forms write the same bits
        assert torch.equal(outs[what].view(torch.int32)[inside], outs["fp32"].view(torch.int32)[inside]), what
    _same_bits(_erase(data.u, d), outs["u8 nchw"], "the same seed twice")
    other = _erase(data.u, _draw("pixel", seed=NOISE_SEED + 1))
    assert not torch.equal(other[inside], outs["u8 nchw"][inside]) and torch.equal(other[~inside], outs["u8 nchw"][~inside])


def test_pixel_mode_moments(data):
    """One 223 x 223 box x 3 channels, N = 149 187, fixed seed: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N)."""
    d = _draw("pixel", [[(0, 223, 0, 223)], [], [], []])
    z = _erase(data.u, d)[0, :, :223, :223].double().reshape(-1)
    n = z.numel()
    assert n == 149187
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print("pixel moments: mean %.5f (bound %.5f), var - 1 = %.5f (bound %.5f)" % (mean, 5 / n ** 0.5, var - 1, 5 * (2 / n) ** 0.5))
    assert abs(mean) <= 5 / n ** 0.5 and abs(var - 1) <= 5 * (2 / n) ** 0.5


# ---- 3. rand -----------------------------------------------------------------------------------------------------------------------------------
def test_rand_mode_one_colour_per_image_box_and_channel(data, bound):
    d = _draw("rand")
    hit = R.hit_map(d, BMAX)
    col = R.box_colours(NOISE_SEED, BMAX)
    outs = {}
    for what, src, normalised in _kinds(data):
        got = outs[what] = _erase(src, d)
        for i in range(BMAX):
            for k in range(len(BOXES[i])):
                m = torch.from_numpy(hit[i] == k)
                assert int(m.sum()) > 0
                for c in range(3):
                    vals = got[i, c][m]
                    assert bool((vals.view(torch.int32) == vals.view(torch.int32)[0]).all()), (what, i, k, c)   # constant over the box
                    assert abs(float(vals[0]) - col[i, k, c]) <= bound, (what, i, k, c)
        outside = torch.from_numpy(hit < 0)[:, None].expand(BMAX, 3, 224, 224)
        assert torch.equal(got.view(torch.int32)[outside], normalised.view(torch.int32)[outside]), what
    inside = torch.from_numpy(hit >= 0)[:, None].expand(BMAX, 3, 224, 224)
    for what in ("u8 nchw", "u8 nhwc"):
        assert torch.equal(outs[what].view(torch.int32)[inside], outs["fp32"].view(torch.int32)[inside]), what
    # on the overlap of image 2's boxes the later one wins
    g = outs["fp32"]
    assert hit[2, 70, 70] == 1 and hit[2, 40, 40] == 0
    assert torch.equal(g[2, :, 70, 70], g[2, :, 105, 105]) and not torch.equal(g[2, :, 70, 70], g[2, :, 40, 40])
    _same_bits(g, R.erase_ref(data.xf, d).where(~inside, g), "rand: everything outside the boxes")


# ---- 4. cube -----------------------------------------------------------------------------------------------------------------------------------
def test_cube_shares_the_boxes_of_a_clip_not_its_noise(data, bound):
    box = (17, 40, 29, 50)
    cube = _draw("pixel", [[box], []], cube=True, frames=2)
    assert cube.images() == 4
    got = _erase(data.u, cube, frames=2)
    want = R.erase_ref_f64(data.xn, cube)
    assert float(np.abs(got.numpy() - want).max()) <= bound
    inside = torch.zeros(224, 224, dtype=torch.bool)
    inside[17:57, 29:79] = True
    for f in (0, 1):   # both frames of clip 0 carry the box, clip 1 is untouched
        assert torch.equal(got[f][:, ~inside], data.xn[f][:, ~inside]) and not bool((got[f][:, inside] == data.xn[f][:, inside]).any())
    assert not torch.equal(got[0][:, inside], got[1][:, inside])   # noise is per image
    _same_bits(got[2:], data.xn[2:], "cube: the clip without a box")
    # without cube the rows are per image, whatever the frame count
    per = _draw("pixel", [[box], [], [], [box]], frames=2)
    got = _erase(data.nhwc, per, frames=2)
    assert float(np.abs(got.numpy() - R.erase_ref_f64(data.xn, per)).max()) <= bound
    _same_bits(got[1:3], data.xn[1:3], "per-image rows: images 1 and 2")
    assert not bool((got[3][:, inside] == data.xn[3][:, inside]).any())
    # const, exact, through the callable form on clips [b,3,t,224,224] and [b,t,224,224,3]
    from util.erasing import DeviceRandomErasing
    cc = _draw("const", [[box], [(0, 1, 0, 1)]], cube=True, frames=2)
    want = R.erase_ref(data.xn, cc).reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4)
    clips = data.u.reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()
    _same_bits(DeviceRandomErasing(cube=True).inject([cc])(clips.cuda(), norm=NORM).contiguous(), want.contiguous(), "__call__ on byte clips")
    _same_bits(DeviceRandomErasing(cube=True).inject([cc])(data.nhwc.reshape(2, 2, 224, 224, 3).cuda(), norm=NORM).contiguous(),
               want.contiguous(), "__call__ on channels-last byte clips")


# ---- 5. erase, then mix ------------------------------------------------------------------------------------------------------------------------
def _mix_draws():
    from util.mixup import MixDraw
    return {"mixup": MixDraw.mixup(0.31415926).with_targets(SMOOTH, C), "cutmix": MixDraw.cutmix((20, 90, 25, 70)).with_targets(SMOOTH, C)}


def test_erase_then_mix_equals_the_mix_of_the_erased_images(data):
    d = _draw("const")
    for name, mix in _mix_draws().items():
        for what, src, normalised in _kinds(data):
            x = normalised.clone()
            if what == "fp32":
                x[3] = synth.make_batch(1, C, seed=SEED + 1)[0][0]   # (NaN times lam would be NaN in both; keep the comparison meaningful)
                src = x
            e = R.erase_ref(x, d)
            _same_bits(_erase(src, d, mix=mix), MR.mix_images(e, mix), "erase then %s, %s" % (name, what))
            assert not torch.equal(MR.mix_images(e, mix), MR.mix_images(x, mix))   # the partner's erased pixels are what is blended in
    # clips: frame f of clip 0 pairs with frame f of clip 1, each erased with its clip's row
    cube = _draw("const", [[(17, 40, 29, 50)], [(30, 50, 30, 50)]], cube=True, frames=2)
    mix = _mix_draws()["cutmix"]
    _same_bits(_erase(data.u, cube, frames=2, mix=mix), MR.mix_images(R.erase_ref(data.xn, cube), mix, 2), "erase then cutmix, clips")


# ---- 6. fused forward --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    from runtime import DyTEngine
    cache = {}
    sd = synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=1, gate_bias=0.85)

    def get(precision):
        if precision not in cache:
            cache[precision] = DyTEngine(C, RANK, 0.1, DEV, precision=precision, max_batch=BMAX, depth=1)
            cache[precision].load_state_dict(sd)
        return cache[precision]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
def test_training_forward_with_erase_on_equals_the_float_path_on_the_erased_image(precision, engines, data):
    eng = engines(precision)
    xf = data.xf.clone()
    xf[3] = synth.make_batch(1, C, seed=SEED + 1)[0][0]
    d = _draw("pixel")
    fwd = lambda x, training=True: eng.forward(x.cuda(), training=training, seed=11)   # noqa: E731
    plain = fwd(data.u)
    for mix in (None, _mix_draws()["mixup"], _mix_draws()["cutmix"]):
        want = fwd(eng.erase_images(data.u.cuda(), d, mix))
        want_f = fwd(eng.erase_images(xf.cuda(), d, mix))
        assert bool(torch.isfinite(want[0]).all()) and not torch.equal(want[0], plain[0])
        eng.set_erase(d)
        if mix is not None:
            eng.set_mix(mix)
        try:
            assert eng._erase_on
            for what, x, w in (("nchw bytes", data.u, want), ("nhwc bytes", data.nhwc, want), ("float", xf, want_f)):
                got = fwd(x)
                for k, part in enumerate(("logits", "token select", "token logits")):
                    _same_bits(got[k], w[k], "%s mix=%s %s: %s" % (precision, mix and mix.mode, what, part))
            if mix is None:   # an eval-mode forward never erases
                _same_bits(fwd(data.u, training=False)[0], eng.forward(data.xn.cuda(), seed=11)[0], "eval forward while erasing is on")
        finally:
            eng.set_erase(None)
            eng.set_mix(None)
    _same_bits(fwd(data.u)[0], plain[0], "off again")


# ---- 7. / 8. / 9. the training loop ------------------------------------------------------------------------------------------------------------
def _model(sd, mode, **kw):
    from models.vision_transformer_IN21K import VisionTransformer
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0), precision="fp16", train_mode=mode, max_batch=BMAX, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda()


@pytest.fixture(scope="module")
def sd2():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=2, gate_bias=0.85)


def _criterion():
    from models.losses import AdaLoss
    return AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)


def _train(model, loader, mixup_fn=None, eraser=None, graph=False, lr=1e-3):
    from engine_finetune import FusedAdamW, train_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph)
    if eraser is not None:
        args.random_erasing = eraser
    stats = train_one_epoch(model, _criterion(), loader, opt, DEV, 0, None, 0, mixup_fn, None, args=args)
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone(), opt


def _erase_draws():
    return [_draw("pixel"), _draw("pixel", [[], [(0, 223, 0, 223)], [(5, 9, 220, 4), (1, 1, 1, 1)], [(100, 30, 60, 17)]], seed=NOISE_SEED ^ 0x5555)]


@pytest.mark.parametrize("mode,with_mix", [("masked", True), ("masked", False), ("compact", True), ("compact", False)])
def test_two_steps_of_the_loop_equal_the_loop_fed_the_erased_images(mode, with_mix, sd2, data, monkeypatch):
    """train_one_epoch with args.random_erasing holding two injected `pixel` draws (and a DeviceMixup with a mixup and a cutmix draw), byte
    loader, against the same loop fed dyt_erase_images' output as float images (and the mixed class-probability targets)."""
    from _lib import erase_images
    from util.erasing import DeviceRandomErasing
    from util.mixup import DeviceMixup
    monkeypatch.setenv("DYT_PREFETCH", "0")
    ed = _erase_draws()
    md = list(_mix_draws().values()) if with_mix else [None, None]
    extra = [(synth.make_noise(BMAX, depth=2, seed=SEED + 20 + i), synth.make_dropout_masks(BMAX, RANK, depth=2, seed=SEED + 30 + i)) for i in range(2)]
    batches = [data.u, data.nhwc]
    fused_loader = [(batches[i], data.y, extra[i][0], extra[i][1]) for i in range(2)]
    floats = [erase_images(batches[i].cuda(), _table(ed[i]), norm=NORM, mix_params=None if md[i] is None else _mix_params(md[i])).cpu() for i in range(2)]
    plain_loader = [(floats[i], data.y, extra[i][0], extra[i][1]) for i in range(2)]
    ma, mb = _model(sd2, mode, input_norm="imagenet"), _model(sd2, mode, input_norm="imagenet")
    eraser = DeviceRandomErasing(mode="pixel").inject(ed)
    mixer = DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(md) if with_mix else None
    sa, fa, _ = _train(ma, fused_loader, mixer, eraser)
    assert not ma._engine._erase_on and not ma._engine._mix_on and not eraser._injected   # both draws used, erasing switched off after the epoch
    targets = iter(md)
    soft_only = (lambda s, t: (s, MR.mix_targets(t, C, next(targets), SMOOTH))) if with_mix else None
    sb, fb, _ = _train(mb, plain_loader, soft_only)
    assert sa == sb, (sa, sb)
    _same_bits(fa, fb, "%s mix=%s: trainable parameters" % (mode, with_mix))
    moved = max(float((p.detach().cpu() - sd2[n]).abs().max()) for n, p in ma.named_parameters() if p.requires_grad)
    assert moved > 0 and np.isfinite(sa["loss"])
    if not with_mix and mode == "compact":   # and the erasing changed something: the same loop without it ends elsewhere
        mc = _model(sd2, mode, input_norm="imagenet")
        _, fc, _ = _train(mc, fused_loader)
        assert not torch.equal(fc, fa)
        del mc
    del ma, mb


def test_any_other_mixup_fn_gets_the_erased_float_images(sd2, data, monkeypatch):
    """With a callable mixup_fn that is no DeviceMixup the loop erases first (fp32 out), then calls it: the order stays erase, then mix."""
    from util.erasing import DeviceRandomErasing
    monkeypatch.setenv("DYT_PREFETCH", "0")
    d, mix = _draw("const"), _mix_draws()["cutmix"]
    seen = []

    def mixup_fn(samples, targets):
        seen.append(samples.detach().cpu().clone())
        return MR.callable_for([mix], C, SMOOTH)(samples, targets)
    ma, mb = _model(sd2, "compact", input_norm="imagenet"), _model(sd2, "compact", input_norm="imagenet")
    sa, fa, _ = _train(ma, [(data.u, data.y)], mixup_fn, DeviceRandomErasing().inject([d]))
    _same_bits(seen[0], R.erase_ref(data.xn, d), "what the callable was handed")
    sb, fb, _ = _train(mb, [(R.erase_ref(data.xn, d), data.y)], MR.callable_for([mix], C, SMOOTH))
    assert sa == sb
    _same_bits(fa, fb, "callable route: trainable parameters")
    assert not ma._engine._erase_on
    del ma, mb


def test_video_clips_through_the_loop_share_their_boxes(data, monkeypatch):
    """2 byte clips of 2 frames through train_video_one_epoch with a `cube` draw against the same loop fed the erased float clips."""
    import engine_finetune as E
    from util.erasing import DeviceRandomErasing
    from video_models.video_vision_transformer_IN21K import vit_base_patch16_224_in21k
    monkeypatch.setenv("DYT_PREFETCH", "0")
    vsd = synth.make_state_dict(C, RANK, seed=SEED, kind="test", gate_bias=0.85, video=True)
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)

    def video_model():
        m = vit_base_patch16_224_in21k(num_classes=C, drop_path_rate=0.0, tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0),
                                       precision="fp16", train_mode="compact", max_batch=BMAX, input_norm="imagenet")
        m.load_state_dict(vsd)
        for n, p in m.named_parameters():
            p.requires_grad = synth.is_trainable(n)
        return m.cuda()

    def train(m, loader, eraser=None):
        opt = E.FusedAdamW(m, lr=1e-3, weight_decay=0.01)
        args = types.SimpleNamespace(accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=False)
        if eraser is not None:
            args.random_erasing = eraser
        stats = E.train_video_one_epoch(m, _criterion(), loader, opt, DEV, 0, None, 0, None, None, args=args)
        torch.cuda.synchronize()
        return stats, m._engine.flat.clone()
    cube = _draw("pixel", [[(17, 40, 29, 50)], []], cube=True, frames=2)
    clips = data.u.reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()            # [b,3,t,224,224] bytes
    erased = _erase(data.u, cube, frames=2).reshape(2, 2, 3, 224, 224).permute(0, 2, 1, 3, 4).contiguous()
    y = data.y[:2]
    ma, mb = video_model(), video_model()
    sa, fa = train(ma, [(clips, y)], DeviceRandomErasing(mode="pixel", cube=True).inject([cube]))
    sb, fb = train(mb, [(erased, y)])
    assert sa == sb, (sa, sb)
    _same_bits(fa, fb, "video: trainable parameters")
    assert not ma._engine._erase_on and np.isfinite(sa["loss"])
    del ma, mb


def test_three_draws_replay_one_captured_graph_and_equal_the_eager_steps(sd2, data, monkeypatch):
    import engine_finetune as E
    from util.erasing import DeviceRandomErasing
    monkeypatch.setenv("DYT_PREFETCH", "0")
    draws = _erase_draws() + [_draw("rand", [[(50, 60, 70, 80)], [], [], [(0, 224 - 1, 0, 100)]], seed=99)]
    loader = [(data.u, data.y), (data.u.flip(1).contiguous(), data.y.flip(0).contiguous()), (data.u, data.y)]
    out = {}
    real = E.train_step
    for graph in (False, True):
        seq = []

        def spy(*a, **kw):
            r = real(*a, **kw)
            seq.append(kw["losses_out"].clone())
            return r
        monkeypatch.setattr(E, "train_step", spy)
        m = _model(sd2, "compact", input_norm="imagenet")
        stats, flat, _ = _train(m, loader, None, DeviceRandomErasing(mode="pixel").inject(list(draws)), graph=graph)
        monkeypatch.setattr(E, "train_step", real)
        out[graph] = (stats, flat, torch.stack(seq).cpu(), len(m._engine._graphs), [k[-2:] for k in m._engine._graphs])
        del m
    assert out[False][3] == 0 and out[True][3] == 1 and out[True][4] == [(True, False)]   # one graph for the three draws, keyed "erase on", "mix off"
    assert out[False][0] == out[True][0], (out[False][0], out[True][0])
    _same_bits(out[True][2], out[False][2], "per-step losses, graph against eager")
    _same_bits(out[True][1], out[False][1], "trainable parameters, graph against eager")
    assert len({float(v) for v in out[True][2][:, 0]}) == 3   # three draws, three losses


def test_after_the_epoch_nothing_is_erased(sd2, data, monkeypatch):
    """evaluate() sees unerased images, and a step after set_erase(None) equals the step of an engine that never had it on."""
    from engine_finetune import evaluate
    from util.erasing import DeviceRandomErasing
    monkeypatch.setenv("DYT_PREFETCH", "0")
    a = _model(sd2, "compact", input_norm="imagenet")
    _train(a, [(data.u, data.y)], None, DeviceRandomErasing(mode="pixel").inject([_draw("pixel", [[(0, 223, 0, 223)]] * 4)]))
    assert not a._engine._erase_on
    b = _model({k: v.detach().cpu().clone() for k, v in a.state_dict().items()}, "compact", input_norm="imagenet")
    g1, g2 = (t.cuda().contiguous() for t in synth.make_noise(BMAX, depth=2, seed=SEED + 1))
    keep = synth.make_dropout_masks(BMAX, RANK, depth=2, seed=SEED + 2).cuda().contiguous()

    def step(m):
        eng = m.engine(BMAX, DEV)
        losses = torch.zeros(8, device=DEV)
        eng.step_fwd_bwd(data.u.cuda(), data.y.cuda(), 0.5, 2.0, 0.1, 1.0, g1=g1, g2=g2, keep_mask=keep, seed=5, losses=losses)
        torch.cuda.synchronize()
        return losses.clone(), eng.grad.clone()
    (la, ga), (lb, gb) = step(a), step(b)
    _same_bits(la, lb, "losses of the step after the erased epoch")
    _same_bits(ga, gb, "gradient of the step after the erased epoch")
    ea, eb = (evaluate([(data.u, data.y)], m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C)) for m in (a, b))
    assert ea == eb, (ea, eb)
    # even with erasing ON, evaluate's eval-mode forwards are unerased
    a._engine.set_erase(_draw("const", [[(0, 223, 0, 223)]] * 4))
    try:
        assert evaluate([(data.u, data.y)], a, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C)) == eb
    finally:
        a._engine.set_erase(None)
    del a, b


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_text_before_anything_is_enqueued(engines, sd2, data):
    from _lib import DyTError
    from engine_finetune import FusedAdamW, train_step
    from runtime import DyTEngine
    from util.erasing import DeviceRandomErasing
    eng = engines("fp16")
    d = _draw("const")
    tab = _table(d, BMAX)
    L, h = eng.L, eng.h
    # the C entry: a misaligned table, another frame count, no capacity
    for args, text in (((tab.data_ptr() + 4, BMAX, 1), b"16-byte aligned"), ((tab.data_ptr(), BMAX, 2), b"frames"), ((tab.data_ptr(), 0, 1), b"units_capacity")):
        assert L.dyt_set_erase(h, *args) == -1
        assert text in L.dyt_last_error(), L.dyt_last_error()
    # a table with fewer units than the batch: the forward and the step refuse, nothing runs
    assert L.dyt_set_erase(h, tab.data_ptr(), 2, 1) == 0
    try:
        with pytest.raises(DyTError, match="fewer units"):
            eng.forward(data.u.cuda(), training=True)
        eng.grad.fill_(7.0)
        with pytest.raises(DyTError, match="fewer units"):
            eng.step_fwd_bwd(data.u.cuda(), data.y.cuda(), 0.5, 2.0, 0.0, 0.0)
        torch.cuda.synchronize()
        assert bool((eng.grad == 7.0).all()), "something was enqueued"
        eng.forward(data.u[:2].cuda(), training=True)   # two images fit
    finally:
        assert L.dyt_set_erase(h, None, 0, 1) == 0
        eng.grad.zero_()
    # the engine: a draw for more images than max_batch, clips of another length
    with pytest.raises(DyTError, match="max_batch"):
        eng.set_erase(_draw("const", [[]] * (BMAX + 1)))
    with pytest.raises(DyTError, match="frame"):
        eng.set_erase(_draw("const", [[], []], cube=True, frames=2))
    with pytest.raises(DyTError, match="covers"):
        eng.erase_images(data.u.cuda(), _draw("const", [[], []]))
    assert not eng._erase_on
    # train_step: units that do not match the batch
    m = _model(sd2, "compact", input_norm="imagenet").train()
    opt = FusedAdamW(m, lr=1e-3)
    me = m.engine(BMAX, DEV)
    before = me.flat.clone()
    with pytest.raises(DyTError, match="covers 2 images"):
        train_step(m, data.u.cuda(), data.y.cuda(), opt, target_ratio=0.5, token_minimal=0.0, token_minimal_weight=0.0, erase=_draw("const", BOXES[:2]))
    torch.cuda.synchronize()
    assert torch.equal(me.flat, before) and not me._erase_on
    del m
    # an inference-only context
    inf = DyTEngine(C, RANK, 0.1, DEV, precision="fp16", max_batch=2, depth=1, inference=True)
    with pytest.raises(DyTError, match="inference_only"):
        inf.set_erase(_draw("const", BOXES[:2]))
    assert inf.L.dyt_set_erase(inf.h, tab.data_ptr(), BMAX, 1) != 0 and b"inference_only" in inf.L.dyt_last_error()
    # what the kernels do not implement
    for kw in (dict(max_count=5), dict(num_splits=2)):
        with pytest.raises(NotImplementedError):
            DeviceRandomErasing(**kw)
    # the context is as it was
    _same_bits(eng.forward(data.u.cuda(), training=True, seed=3)[0], eng.forward(data.xn.cuda(), training=True, seed=3)[0], "after the refusals")
