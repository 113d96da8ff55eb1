"""GPU tests of the device RandAugment (pytest -m gpu): dyt_randaug_u8 and dyt_randaug_table against tests/randaug_refs.py -- the numpy
restatement of Pillow's 8-bit arithmetic that tests/test_randaug_refs_host.py pins to the reference's recorded output and to live Pillow --
and against the reference's recorded bytes (tests/golden/randaug/randaug.npz); args.device_randaug through the video and the image
train_one_epoch.

Every comparison is exact: byte for byte on the pixels, integer for integer on the tables, bit for bit on the losses and the trainable
parameters.  Batches [2, 2, 64, 64, 3] of the golden's sources with 0xFF and 0x00 padding and one [1, 2, 300, 400, 3]; r = 8, C = 10, models
of depth 2."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import randaug_refs as R  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, T, SMOOTH = 10, 8, 211, 2, 0.1
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug", "randaug.npz")
W = (224, 224, 0, 0)


def _urow(r, h, w):
    from util.randaug import aug_row
    return aug_row(r[0], h, w, r[1], r[2], r[3], r[4], r[5])


def _draw(sizes, unit_rows):
    """AugDraw of ``unit_rows`` = per unit its list of restatement rows"""
    from util.randaug import AugDraw
    layers = len(unit_rows[0])
    return AugDraw([_urow(r, h, w) for (h, w), rows in zip(sizes, unit_rows) for r in rows], layers)


def _flat(unit_rows):
    return [r for rows in unit_rows for r in rows]


def _run(batch, sizes, unit_rows, draw=True, **kw):
    """the augmented batch on the host"""
    from _lib import randaug_u8
    d = _draw(sizes, unit_rows)
    table = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(DEV)
    out = randaug_u8(torch.from_numpy(np.ascontiguousarray(batch)).to(DEV), table, d if draw else None, layers=d.layers, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bytes(got, want, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    bad = got != want
    if bad.any():
        where = np.argwhere(bad)[0].tolist()
        raise AssertionError("%s: %d of %d bytes differ (first at %s: got %d, want %d)" % (
            what, int(bad.sum()), bad.size, where, int(got[tuple(where)]), int(want[tuple(where)])))


def _same_bits(got, want, what):
    got = torch.as_tensor(got).detach().cpu().contiguous()
    want = torch.as_tensor(want).detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        raise AssertionError("%s: %d of %d values differ in their bits" % (what, int(bad.sum()), bad.numel()))


def _rows(g, prefix):
    return [R.row(int(o), int(i), float(f), tuple(c.tolist()), int(fl)) for o, i, f, c, fl in zip(
        g[prefix + "_op"], g[prefix + "_iarg"], g[prefix + "_factor"], g[prefix + "_coeffs"], g[prefix + "_filter"])]


@pytest.fixture(scope="module")
def data():
    """The golden's sources and cases, the zero-padded twins, the big batch and the restatement's outputs: computed once, read only."""
    g = np.load(GOLDEN)
    d = types.SimpleNamespace(g=g, src=g["px_src"], sizes=[tuple(int(v) for v in s) for s in g["px_sizes"]], cases=_rows(g, "case_row"), chain=_rows(g, "chain_row"))
    d.zero = d.src.copy()
    for i, (h, w) in enumerate(d.sizes):
        d.zero[i, :, h:] = 0
        d.zero[i, :, :, w:] = 0
    yy, xx = np.mgrid[0:300, 0:400]
    big = np.stack([(yy * 255 // 299), (xx * 255 // 399), ((yy // 8 + xx // 8) & 1) * 200 + 20], axis=2).astype(np.uint8)
    rng = np.random.default_rng(SEED)
    d.big = np.stack([big, rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)])[None].copy()        # [1, 2, 300, 400, 3]
    d.big[0, 1, :, :, 1] = rng.integers(40, 200, (300, 400))
    d.big_rows = [R.row(R.AFFINE, coeffs=R.rotate_coeffs(17.0, 300, 400), filt=R.BICUBIC), R.row(R.AFFINE, coeffs=(1, -0.25, 0, 0, 1, 0), filt=R.BILINEAR),
                  R.row(R.SHARPNESS, 0, 1.8), R.row(R.EQUALIZE), R.row(R.AUTO_CONTRAST), R.row(R.CONTRAST, 0, 1.55), R.row(R.COLOR, 0, 0.3)]
    d.big_want = [R.apply_batch(d.big, [(300, 400)], [r], 1) for r in d.big_rows]
    d.y = torch.tensor([3, 7], dtype=torch.int64)
    return d


# ---- 0. the negative control comes first: before this module has constructed any augmenter -----------------------------------------------
def _video_model(sd, mode, max_batch=2 * T, **kw):
    from video_models.video_vision_transformer_IN21K import VisionTransformer
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0), precision="fp16", train_mode=mode, max_batch=max_batch, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda()


def _image_model(sd, mode, **kw):
    from models.vision_transformer_IN21K import VisionTransformer
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0), precision="fp16", train_mode=mode, max_batch=2, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda()


@pytest.fixture(scope="module")
def sd_video():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=2, gate_bias=0.85, video=True)


@pytest.fixture(scope="module")
def sd_image():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=2, gate_bias=0.85)


def _criterion():
    from models.losses import AdaLoss
    return AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)


def _train(model, loader, video, graph=False, lr=1e-3, **extra):
    from engine_finetune import FusedAdamW, train_one_epoch, train_video_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph, **extra)
    stats = (train_video_one_epoch if video else train_one_epoch)(model, _criterion(), loader, opt, DEV, 0, None, 0, None, None, args=args)
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone()


def _clip_draws():
    from util.crop import BILINEAR_F32, CropDraw
    first = [(48, 64, 0, 0, 48, 64, 227, 302, 1, 67, 1, 0), (64, 40, 0, 0, 64, 40, 358, 224, 134, 0, 0, 1)]
    second = [(64, 64, 3, 2, 40, 50) + W + (0, 0), (64, 64, 0, 9, 64, 31) + W + (1, 1)]
    return [CropDraw(first, filter=BILINEAR_F32), CropDraw(second, filter=BILINEAR_F32)]


def test_a_loop_without_the_arg_equals_one_run_before_any_augmenter_existed_and_the_refusals(sd_video, sd_image, data, monkeypatch):
    """The plain video loop run first, then -- after an augmenter was constructed and used on the same process -- the loop with
    args.device_randaug = None: the same losses and parameters, and no RandAugment buffer on the engine.  The callable form gives the
    restatement's bytes.  Every refusal of the two loops comes as its text."""
    from _lib import DyTError
    from util.crop import DeviceClipRandomResizedCrop, DeviceRandomResizedCrop
    from util.randaug import DeviceRandAugment
    monkeypatch.setenv("DYT_PREFETCH", "0")
    sizes = torch.tensor(data.sizes[:2], dtype=torch.int32)
    loader = [((torch.from_numpy(data.src[:2]), sizes), data.y), (torch.from_numpy(data.src[:2][::-1].copy()), data.y.flip(0).contiguous())]
    m = _video_model(sd_video, "compact", input_norm="imagenet")
    before = _train(m, loader, True, device_crop=DeviceClipRandomResizedCrop().inject(_clip_draws()))
    assert not hasattr(m._engine, "_ra_dev")
    del m
    # the callable form
    aug = DeviceRandAugment("rand-m7-n4-mstd0.5-inc1")
    unit_rows = [[data.cases[21], data.cases[11]], [data.cases[19], data.cases[2]]]        # ShearX + Equalize | Sharpness + Solarize
    sz = [data.sizes[2], data.sizes[0]]
    batch = np.stack([data.src[2], data.src[0]])
    got = aug.inject(_draw(sz, unit_rows))(torch.from_numpy(batch).to(DEV), sz)
    _same_bytes(got, R.apply_batch(batch, sz, _flat(unit_rows), 2), "DeviceRandAugment.__call__")
    img = np.ascontiguousarray(data.src[0, :, :48, :64])                                    # an image batch that every image fills
    got = aug.inject(_draw([(48, 64)] * 2, [[data.cases[31]], [data.cases[16]]]))(torch.from_numpy(img).to(DEV))
    _same_bytes(got, R.apply_batch(img[:, None], [(48, 64)] * 2, [data.cases[31], data.cases[16]], 1)[:, 0], "DeviceRandAugment.__call__, images")
    m = _video_model(sd_video, "compact", input_norm="imagenet")
    after = _train(m, loader, True, device_crop=DeviceClipRandomResizedCrop().inject(_clip_draws()), device_randaug=None)
    assert after[0] == before[0] and not hasattr(m._engine, "_ra_dev")
    _same_bits(after[1], before[1], "the loop without args.device_randaug")
    # refusals
    floats = torch.zeros(2, 3, T, 224, 224)
    with pytest.raises(DyTError, match="must be a util.randaug.DeviceRandAugment"):
        _train(m, loader, True, device_randaug=object())
    with pytest.raises(DyTError, match=r"already \[B, T, 224, 224, 3\]"):
        _train(m, [(floats, data.y)], True, device_randaug=aug)
    with pytest.raises(DyTError, match="no args.device_crop"):
        _train(m, [(torch.from_numpy(data.src[:2]), data.y)], True, device_randaug=aug)
    del m
    mi = _image_model(sd_image, "compact", input_norm="imagenet")
    for bad in (torch.zeros(2, 3, 224, 224), torch.zeros(2, 3, 224, 224, dtype=torch.uint8), torch.zeros(2, 224, 224, 3)):
        with pytest.raises(DyTError, match=r"channels-last byte batch uint8 \[B, 224, 224, 3\]"):
            _train(mi, [(bad, data.y)], False, device_randaug=aug)
    with pytest.raises(DyTError, match="image model"):
        _train(mi, [(torch.zeros(2, T, 224, 224, 3, dtype=torch.uint8), data.y)], True, device_randaug=aug)
    with pytest.raises(ValueError, match="injected"):
        _train(mi, [(torch.zeros(2, 224, 224, 3, dtype=torch.uint8), data.y)], False, device_randaug=aug.inject(_draw([(48, 64)] * 2, [[data.cases[0]]] * 2)))
    aug._injected.clear()
    assert getattr(mi, "_engine", None) is None or not hasattr(mi._engine, "_ra_dev")   # nothing was uploaded, nothing allocated
    del mi


# ---- 1. kernel bytes ----------------------------------------------------------------------------------------------------------------------
def test_every_operation_alone_equals_the_restatement_and_the_golden(data):
    """Each golden case as unit 0 of a batch of two -- unit 1 is another source with a skipped layer -- with 0xFF and with 0x00 padding."""
    g = data.g
    seen = set()
    for k, r in enumerate(data.cases):
        i = int(g["case_src"][k])
        j = (i + 1) % 3
        sz = [data.sizes[i], data.sizes[j]]
        unit_rows = [[r], [R.row(R.IDENTITY)]]
        for pad, src in (("0xFF", data.src), ("0x00", data.zero)):
            batch = np.stack([src[i], src[j]])
            got = _run(batch, sz, unit_rows)
            want = R.apply_batch(batch, sz, _flat(unit_rows), 1)
            what = "case %d %s (%s), padding %s" % (k, g["case_name"][k], R.OP_NAMES[r[0]], pad)
            _same_bytes(got, want, what)
            _same_bytes(got[1], batch[1], what + ": the skipped unit")
            if pad == "0xFF":
                _same_bytes(got[0], g["case_out"][k], what + ": the reference's recorded bytes")
            else:
                h, w = sz[0]
                _same_bytes(got[0][:, :h, :w], g["case_out"][k][:, :h, :w], what + ": the reference's recorded bytes")
                assert not got[0][:, h:].any() and not got[0][:, :, w:].any()
        seen.add((r[0], r[4] if r[0] == R.AFFINE else 0))
    assert {s[0] for s in seen} == set(range(12)) and {(R.AFFINE, R.BILINEAR), (R.AFFINE, R.BICUBIC)} <= seen


def test_the_big_batch_runs_more_than_one_block_per_frame(data):
    for r, want in zip(data.big_rows, data.big_want):
        _same_bytes(_run(data.big, [(300, 400)], [[r]]), want, "300 x 400 %s" % R.OP_NAMES[r[0]])
    # a smaller valid extent inside the same padded shape: the rest is padding and stays
    sz = [(211, 333)]
    for r in (data.big_rows[0], data.big_rows[2], data.big_rows[3]):
        r = R.row(r[0], r[1], r[2], R.rotate_coeffs(17.0, 211, 333) if r[0] == R.AFFINE else r[3], r[4])
        got = _run(data.big, sz, [[r]])
        _same_bytes(got, R.apply_batch(data.big, sz, [r], 1), "211 x 333 of 300 x 400 %s" % R.OP_NAMES[r[0]])
        assert np.array_equal(got[0, :, 211:], data.big[0, :, 211:]) and np.array_equal(got[0, :, :, 333:], data.big[0, :, :, 333:])


def test_the_debug_tables_equal_the_restatements(data):
    from _lib import randaug_table
    g = data.g
    ks = [k for k, r in enumerate(data.cases) if r[0] in (R.AUTO_CONTRAST, R.EQUALIZE, R.CONTRAST, R.SOLARIZE, R.SOLARIZE_ADD, R.POSTERIZE, R.INVERT, R.COLOR)]
    assert len(ks) >= 14
    for k in ks:
        r = data.cases[k]
        i = int(g["case_src"][k])
        sz = [data.sizes[(i + 1) % 3], data.sizes[i]]                 # the case is unit 1 this time
        batch = np.stack([data.src[(i + 1) % 3], data.src[i]])
        d = _draw(sz, [[R.row(R.INVERT)], [r]])
        table = torch.frombuffer(bytearray(d.words(3)), dtype=torch.int32).to(DEV)
        for f in range(2):
            got = randaug_table(torch.from_numpy(batch).to(DEV), table, 1, 1, f, 0).cpu().numpy()
            h, w = sz[1]
            hist = R.histograms(batch[1, f, :h, :w])
            want = R.table(r[0], r[1], hist) if r[0] <= R.EQUALIZE else R.table(R.IDENTITY, 0, None)
            assert got.shape == (769,) and got.dtype == np.int32
            assert np.array_equal(got[:768].reshape(3, 256), want.astype(np.int32)), (k, f, R.OP_NAMES[r[0]])
            assert got[768] == (R.contrast_mean(hist[3]) if r[0] == R.CONTRAST else 0), (k, f)
    # an invalid unit gives zeros
    words = bytearray(d.words(3))
    words[64 + 80:64 + 84] = struct.pack("<i", 12)
    assert not randaug_table(torch.from_numpy(batch).to(DEV), torch.frombuffer(words, dtype=torch.int32).to(DEV), 1, 1, 0, 0).any()


def test_the_four_layer_chain_and_two_units_with_different_sequences(data):
    g = data.g
    # the chain of the recorded draw on source 2, beside a unit whose sequence is its reverse
    sz = [data.sizes[2], data.sizes[0]]
    batch = np.stack([data.src[2], data.src[0]])
    unit_rows = [data.chain, data.chain[::-1]]
    got = _run(batch, sz, unit_rows)
    _same_bytes(got[0], g["chain_out"], "the four-layer chain: the reference's recorded bytes")
    _same_bytes(got, R.apply_batch(batch, sz, _flat(unit_rows), 4), "the chain and its reverse")
    # Affine then a table operation in one unit, the reverse in the other: every unit ends in dst whichever buffers it went through
    aff0, aff1 = R.row(R.AFFINE, coeffs=R.rotate_coeffs(-11.0, *sz[0]), filt=R.BICUBIC), R.row(R.AFFINE, coeffs=(1, 0.17, 0, 0, 1, 0), filt=R.BILINEAR)
    for unit_rows in ([[aff0, R.row(R.EQUALIZE)], [R.row(R.POSTERIZE, 2), aff1]],
                      [[aff0, R.row(R.SHARPNESS, 0, 1.7), R.row(R.CONTRAST, 0, 0.4), aff0], [R.row(R.AUTO_CONTRAST), R.row(R.IDENTITY), aff1, R.row(R.COLOR, 0, 1.6)]],
                      [[R.row(R.SHARPNESS, 0, 0.2), aff0, aff0], [aff1, R.row(R.BRIGHTNESS, 0, 1.4), R.row(R.SHARPNESS, 0, 1.9)]]):
        d = _draw(sz, unit_rows)
        assert len({b for b in d.buffers()}) >= 3
        want = R.apply_batch(batch, sz, _flat(unit_rows), len(unit_rows[0]))
        _same_bytes(_run(batch, sz, unit_rows), want, "two sequences %r" % (d.names(),))
        _same_bytes(_run(batch, sz, unit_rows, draw=False), want, "two sequences, every kernel of every layer launched")


def test_skipped_layers_are_the_identity_and_one_frame_is_the_image_form(data):
    sz = [data.sizes[0], data.sizes[1]]
    batch = np.stack([data.zero[0], data.src[1]])
    ident, inv = R.row(R.IDENTITY), R.row(R.INVERT)
    _same_bytes(_run(batch, sz, [[ident] * 4, [ident] * 4]), batch, "four skipped layers")
    for at in range(3):
        rows = [ident] * 3
        rows[at] = inv
        got = _run(batch, sz, [rows, [ident] * 3])
        _same_bytes(got, R.apply_batch(batch, sz, rows + [ident] * 3, 3), "one Invert in layer %d" % at)
    # frames = 1: an image batch [B, H, W, 3]
    img = np.ascontiguousarray(batch[:, 0])
    unit_rows = [[data.cases[31], data.cases[11]], [data.cases[20], data.cases[23]]]       # Rotate + Equalize | Sharpness + ShearY
    unit_rows[0][0] = R.row(R.AFFINE, coeffs=R.rotate_coeffs(-13.7, *sz[0]), filt=R.BICUBIC)
    got = _run(img, sz, unit_rows)
    assert got.shape == img.shape
    _same_bytes(got, R.apply_batch(img[:, None], sz, _flat(unit_rows), 2)[:, 0], "the image form")
    _same_bytes(got, _run(batch[:, :1], sz, unit_rows)[:, 0], "the image form against one-frame clips")


def test_padding_and_canaries_around_the_buffers_are_unchanged(data):
    from _lib import randaug_u8
    sz = [data.sizes[2], data.sizes[1]]
    batch = np.stack([data.src[2], data.zero[1]])
    unit_rows = [[data.cases[21], R.row(R.SHARPNESS, 0, 1.9), R.row(R.EQUALIZE)], [R.row(R.CONTRAST, 0, 1.63), R.row(R.AFFINE, coeffs=(1, 0, 0, -0.3, 1, 0), filt=R.BILINEAR), R.row(R.INVERT)]]
    d = _draw(sz, unit_rows)
    n, guard = batch.size, 4096
    bufs = [torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(2)]
    stats = torch.full((2 * T * 1024 + 2048,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    src = torch.from_numpy(batch).to(DEV)
    keep = src.clone()
    table = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(DEV)
    out = randaug_u8(src, table, d, out=bufs[0][guard:guard + n].view(batch.shape), work=bufs[1][guard:guard + n].view(batch.shape), stats=stats[1024:1024 + 2 * T * 1024])
    torch.cuda.synchronize()
    want = R.apply_batch(batch, sz, _flat(unit_rows), 3)
    _same_bytes(out, want, "buffers inside canaries")
    for i, (h, w) in enumerate(sz):
        assert np.array_equal(want[i, :, h:], batch[i, :, h:]) and np.array_equal(want[i, :, :, w:], batch[i, :, :, w:])
    for b in bufs:
        assert bool((b[:guard] == 0xA5).all()) and bool((b[guard + n:] == 0xA5).all())
    assert bool((stats[:1024] == 0x5A5A5A5A).all()) and bool((stats[1024 + 2 * T * 1024:] == 0x5A5A5A5A).all())
    assert torch.equal(src, keep)   # the source batch is never written


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_a_hostile_row_gives_zeros_for_that_unit_only(data):
    from _lib import randaug_u8
    from util.randaug import BUF_DST, BUF_SRC, BUF_WORK, pack_row
    sz = [data.sizes[0], data.sizes[1]]
    batch = np.stack([data.src[0], data.src[1]])
    src = torch.from_numpy(batch).to(DEV)
    unit_rows = [[R.row(R.AFFINE, coeffs=(1, 0.2, 0, 0, 1, 0)), R.row(R.EQUALIZE)], [R.row(R.COLOR, 0, 1.5), R.row(R.SHARPNESS, 0, 0.3)]]
    d = _draw(sz, unit_rows)
    want = R.apply_batch(batch, sz, _flat(unit_rows), 2)
    good = bytes(d.words())
    big, low = 2 ** 31 - 1, -2 ** 31

    def patched(layer, unit, row=None, raw=None, **kw):
        at = 64 + 80 * (layer * 2 + unit)
        words = bytearray(good)
        if raw is not None:
            words[at:at + 80] = raw
        else:
            words[at:at + 80] = pack_row(row, **kw)
        return words
    h0, w0 = sz[0]
    base = _urow(R.row(R.AFFINE, coeffs=(1, 0.2, 0, 0, 1, 0)), h0, w0)

    def change(**kw):
        r = dict(zip(("op", "iarg", "factor", "coeffs", "filter", "fill", "h", "w"), base))
        r.update(kw)
        return (r["op"], r["iarg"], r["factor"], tuple(r["coeffs"]), r["filter"], tuple(r["fill"]), r["h"], r["w"])
    hostile = [dict(row=change(op=12)), dict(row=change(op=-1)), dict(row=change(h=65)), dict(row=change(w=65)), dict(row=change(h=0)), dict(row=change(w=big)),
               dict(row=change(filter=0)), dict(row=change(fill=(-1, 0, 0))), dict(row=change(factor=float("nan"))), dict(row=change(coeffs=(1, float("inf"), 0, 0, 1, 0))),
               dict(row=change(coeffs=(float("nan"),) * 6)), dict(row=change(coeffs=(1, 0, 2.0 ** 41, 0, 1, 0))), dict(row=change(op=R.POSTERIZE, iarg=9)),
               dict(row=base, src=BUF_SRC, dst=BUF_SRC), dict(row=base, src=BUF_DST, dst=BUF_DST), dict(row=base, src=BUF_WORK, dst=BUF_WORK), dict(row=base, src=3, dst=BUF_DST),
               dict(row=base, src=BUF_SRC, dst=3), dict(raw=struct.pack("<20i", *([big] * 20))), dict(raw=struct.pack("<20i", *([low] * 20))), dict(raw=b"\xff" * 80),
               dict(raw=b"\0" * 80)]
    for case in hostile:
        for (layer, unit) in ((0, 0), (1, 1)):
            kw = dict(case)
            if "row" in kw and kw["row"] is not base and unit == 1:
                kw["row"] = kw["row"][:6] + (sz[1][0] if kw["row"][6] == h0 else kw["row"][6], sz[1][1] if kw["row"][7] == w0 else kw["row"][7])
            if "row" in kw and "src" not in kw:   # the buffers the good row of that place has
                kw["src"], kw["dst"] = d.buffers()[unit * 2 + layer]
            tab = torch.frombuffer(patched(layer, unit, **kw), dtype=torch.int32).to(DEV)
            out = torch.full(batch.shape, 7, dtype=torch.uint8, device=DEV)
            randaug_u8(src, tab, None, out=out, layers=2)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not got[unit].any(), (case, layer, unit)
            _same_bytes(got[1 - unit], want[1 - unit], "the valid unit beside %r at layer %d, unit %d" % (case, layer, unit))
    # a row that is valid alone but does not link: layer 1 reads a buffer layer 0 did not write; the last layer not in dst
    for layer, unit, s, t in ((1, 0, BUF_WORK, BUF_WORK), (1, 1, BUF_DST, BUF_WORK), (1, 1, BUF_WORK, BUF_WORK)):
        row = d.rows[unit * 2 + layer]
        if (s, t) == d.buffers()[unit * 2 + layer]:
            continue
        tab = torch.frombuffer(patched(layer, unit, row=row, src=s, dst=t), dtype=torch.int32).to(DEV)
        out = torch.full(batch.shape, 7, dtype=torch.uint8, device=DEV)
        randaug_u8(src, tab, None, out=out, layers=2)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert not got[unit].any(), (layer, unit, s, t)
        _same_bytes(got[1 - unit], want[1 - unit], "the valid unit beside a broken buffer sequence")
    # the header: fewer units than the batch, another magic, another layer count
    for magic, units, layers, zeros in ((None, 1, 2, [1]), (None, 0, 2, [0, 1]), (None, -3, 2, [0, 1]), (0, 2, 2, [0, 1]), (None, 2, 3, [0, 1]), (None, 2, 1, [0, 1]), (None, big, 2, [])):
        words = bytearray(good)
        head = list(struct.unpack("<3i", good[:12]))
        words[0:12] = struct.pack("<3i", head[0] if magic is None else magic, units, layers)
        out = torch.full(batch.shape, 7, dtype=torch.uint8, device=DEV)
        randaug_u8(src, torch.frombuffer(words, dtype=torch.int32).to(DEV), None, out=out, layers=2)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for u in range(2):
            if u in zeros:
                assert not got[u].any(), (magic, units, layers, u)
            else:
                _same_bytes(got[u], want[u], "header %r %r %r unit %d" % (magic, units, layers, u))


def test_refusals_come_as_texts_and_leave_the_destination_untouched(data):
    import _lib
    from _lib import DyTError, randaug_u8
    sz = [data.sizes[0], data.sizes[1]]
    batch = np.stack([data.src[0], data.src[1]])
    src = torch.from_numpy(batch).to(DEV)
    d = _draw(sz, [[data.cases[0]], [data.cases[13]]])
    tab = torch.frombuffer(bytearray(d.words(4)), dtype=torch.int32).to(DEV)
    out, work = torch.full(batch.shape, 7, dtype=torch.uint8, device=DEV), torch.full(batch.shape, 9, dtype=torch.uint8, device=DEV)
    stats = torch.zeros(2 * T * 1024, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        ok = dict(src=p(src), units=2, frames=T, h=64, w=64, dst=p(out), work=p(work), stats=p(stats), tab=p(tab), cap=4, layers=1)
        bad = {"null src": dict(src=None), "null dst": dict(dst=None), "null work": dict(work=None), "null stats": dict(stats=None), "null table": dict(tab=None),
               "misaligned src": dict(src=p(src, 8)), "misaligned dst": dict(dst=p(out, 4)), "misaligned work": dict(work=p(work, 2)), "misaligned stats": dict(stats=p(stats, 4)),
               "misaligned table": dict(tab=p(tab, 4)), "src == dst": dict(src=p(out)), "work == dst": dict(work=p(out)), "work == src": dict(work=p(src)),
               "units 0": dict(units=0), "frames 0": dict(frames=0), "layers 0": dict(layers=0), "layers 9": dict(layers=9), "units above capacity": dict(cap=1),
               "units * frames above 65535": dict(units=256, frames=256, cap=256), "side 0": dict(h=0), "side above 4096": dict(w=4097)}
        for what, change in bad.items():
            a = dict(ok, **change)
            assert L.dyt_randaug_u8(a["src"], a["units"], a["frames"], a["h"], a["w"], a["dst"], a["work"], a["stats"], a["tab"], a["cap"], a["layers"], None, None) == -1, what
            assert b"dyt_randaug_u8: randaug:" in L.dyt_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((work == 9).all())   # nothing ran
    # the Python layer refuses an invalid draw before upload, and what the binding cannot take
    with pytest.raises(DyTError, match="valid extent"):
        randaug_u8(src, tab, _draw([(65, 64), (64, 40)], [[data.cases[0]], [data.cases[13]]]), out=out)
    with pytest.raises(DyTError, match="holds 1 units"):
        randaug_u8(src, tab, _draw([(48, 64)], [[data.cases[0]]]), out=out)
    with pytest.raises(DyTError, match="layers must be given"):
        randaug_u8(src, tab)
    for x in (src[0, 0, 0], src.float(), src.cpu(), src.permute(0, 1, 4, 2, 3).contiguous()):
        with pytest.raises(DyTError):
            randaug_u8(x, tab, layers=1)
    with pytest.raises(DyTError, match="table"):
        randaug_u8(src, tab[:16 + 20].contiguous(), layers=1)
    with pytest.raises(DyTError, match="launch mask"):
        randaug_u8(src, tab, layers=1, launch_mask=[1, 1])
    with pytest.raises(DyTError, match="out is a contiguous uint8"):
        randaug_u8(src, tab, layers=1, out=out[:1])
    assert bool((out == 7).all())


# ---- 3. the loops -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["compact", "masked"])
def test_two_steps_of_the_video_loop_equal_the_loop_fed_the_restatements_bytes(mode, sd_video, data, monkeypatch):
    """train_video_one_epoch with args.device_randaug holding two injected draws, in front of a DeviceClipRandomResizedCrop -- a
    (clips, sizes) batch, then a bare uint8 batch that every clip fills -- eager and from a captured graph, against the same loop (and the
    same crop draws) fed the byte clips tests/randaug_refs.py makes of them."""
    from util.crop import DeviceClipRandomResizedCrop
    from util.randaug import DeviceRandAugment
    monkeypatch.setenv("DYT_PREFETCH", "0")
    srcs = [data.src[:2], data.src[1:3][::-1].copy()]
    szs = [data.sizes[:2], [(64, 64), (64, 64)]]
    aff = R.row(R.AFFINE, coeffs=R.rotate_coeffs(19.0, 48, 64), filt=R.BICUBIC)
    unit_rows = [[[aff, R.row(R.EQUALIZE), R.row(R.IDENTITY), R.row(R.SHARPNESS, 0, 1.6)], [R.row(R.CONTRAST, 0, 0.5), R.row(R.AFFINE, coeffs=(1, 0, 0, 0.2, 1, 0), filt=R.BICUBIC), R.row(R.SOLARIZE, 90), R.row(R.IDENTITY)]],
                 [[R.row(R.IDENTITY)] * 4, [R.row(R.AUTO_CONTRAST), R.row(R.COLOR, 0, 1.8), R.row(R.AFFINE, coeffs=(1, 0, -12.5, 0, 1, 0), filt=R.BICUBIC), R.row(R.POSTERIZE, 3)]]]
    want = [R.apply_batch(srcs[i], szs[i], _flat(unit_rows[i]), 4) for i in range(2)]
    assert (want[0] != srcs[0]).any() and np.array_equal(want[1][0], srcs[1][0]) and (want[1][1] != srcs[1][1]).any()
    sizes = torch.tensor(szs[0], dtype=torch.int32)
    y2 = data.y.flip(0).contiguous()
    out = {}
    for what in ("restated", "eager", "graph"):
        m = _video_model(sd_video, mode, input_norm="imagenet")
        cropper = DeviceClipRandomResizedCrop().inject(_clip_draws())
        if what == "restated":
            loader = [((torch.from_numpy(want[0]), sizes), data.y), (torch.from_numpy(want[1]), y2)]
            out[what] = _train(m, loader, True, device_crop=cropper)
            assert not hasattr(m._engine, "_ra_dev")   # no table, no buffer: no RandAugment launch
        else:
            loader = [((torch.from_numpy(srcs[0]), sizes), data.y), (torch.from_numpy(srcs[1]), y2)]
            aug = DeviceRandAugment("rand-m7-n4-mstd0.5-inc1").inject([_draw(szs[i], unit_rows[i]) for i in range(2)])
            out[what] = _train(m, loader, True, graph=what == "graph", device_crop=cropper, device_randaug=aug)
            assert not aug._injected and not cropper._injected and len(m._engine._graphs) == (1 if what == "graph" else 0)
            assert tuple(m._engine._ra_dev.shape) == (16 + 20 * 2 * 8,) and m._engine._ra_out.numel() == srcs[0].size
        del m
    for what in ("eager", "graph"):
        assert out[what][0] == out["restated"][0], (what, out[what][0], out["restated"][0])
        _same_bits(out[what][1], out["restated"][1], "%s %s: trainable parameters" % (mode, what))
    assert np.isfinite(out["restated"][0]["loss"])


def test_the_video_loop_takes_cropped_byte_clips_and_the_prefetcher(sd_video, data):
    """Byte clips that are already [B, T, 224, 224, 3] need no device_crop; the prefetcher is on (its default) and its probe consumes no draw."""
    from util.randaug import DeviceRandAugment
    rng = np.random.default_rng(SEED + 1)
    clips = [rng.integers(0, 256, (2, T, 224, 224, 3), dtype=np.uint8) for _ in range(2)]
    sz = [(224, 224)] * 2
    unit_rows = [[[R.row(R.AFFINE, coeffs=R.rotate_coeffs(-25.0, 224, 224), filt=R.BICUBIC), R.row(R.INVERT)], [R.row(R.EQUALIZE), R.row(R.SHARPNESS, 0, 0.4)]],
                 [[R.row(R.IDENTITY), R.row(R.AFFINE, coeffs=(1, 0.3, 0, 0, 1, 0), filt=R.BICUBIC)], [R.row(R.BRIGHTNESS, 0, 1.7), R.row(R.IDENTITY)]]]
    want = [R.apply_batch(clips[i], sz, _flat(unit_rows[i]), 2) for i in range(2)]
    ma, mb = _video_model(sd_video, "compact", input_norm="imagenet"), _video_model(sd_video, "compact", input_norm="imagenet")
    aug = DeviceRandAugment("rand-m9-n2").inject([_draw(sz, unit_rows[i]) for i in range(2)])
    sa, fa = _train(ma, [(torch.from_numpy(clips[i]).pin_memory(), data.y) for i in range(2)], True, device_randaug=aug)
    sb, fb = _train(mb, [(torch.from_numpy(want[i]).pin_memory(), data.y) for i in range(2)], True)
    assert sa == sb and not aug._injected and not hasattr(mb._engine, "_ra_dev")
    _same_bits(fa, fb, "cropped byte clips: trainable parameters")
    del ma, mb


@pytest.mark.parametrize("mode", ["masked", "compact"])
def test_two_steps_of_the_image_loop_equal_the_loop_fed_the_restatements_bytes(mode, sd_image, data, monkeypatch):
    """train_one_epoch with args.device_randaug behind a DeviceRandomResizedCrop (crop -> flip -> RandAugment), eager and from a captured
    graph, against the loop fed the bytes tests/resample_refs.py and tests/randaug_refs.py make: cropped first, then augmented."""
    import resample_refs as RS
    from util.crop import CropDraw, DeviceRandomResizedCrop
    from util.randaug import DeviceRandAugment
    monkeypatch.setenv("DYT_PREFETCH", "0")
    srcs = [np.ascontiguousarray(data.src[:2, 0]), np.ascontiguousarray(data.src[1:3, 1])]                # [2, 64, 64, 3]
    crops = [[(48, 64, 5, 7, 30, 41) + W + (1,), (64, 40, 10, 0, 50, 40) + W + (0,)], [(64, 64, 0, 0, 64, 64) + W + (0,), (64, 64, 20, 30, 25, 20) + W + (1,)]]
    sz = [(224, 224)] * 2
    unit_rows = [[[R.row(R.AFFINE, coeffs=R.rotate_coeffs(23.0, 224, 224), filt=R.BICUBIC), R.row(R.EQUALIZE)], [R.row(R.SHARPNESS, 0, 1.9), R.row(R.COLOR, 0, 0.2)]],
                 [[R.row(R.CONTRAST, 0, 1.5), R.row(R.AFFINE, coeffs=(1, 0, 40.0, 0, 1, 0), filt=R.BICUBIC)], [R.row(R.IDENTITY), R.row(R.SOLARIZE_ADD, 70)]]]
    cropped = [RS.resample_batch(srcs[i], crops[i]) for i in range(2)]
    want = [R.apply_batch(cropped[i][:, None], sz, _flat(unit_rows[i]), 2)[:, 0] for i in range(2)]
    assert all((want[i] != cropped[i]).any() for i in range(2))
    sizes = torch.tensor(data.sizes[:2], dtype=torch.int32)
    y2 = data.y.flip(0).contiguous()
    out = {}
    for what in ("restated", "eager", "graph"):
        m = _image_model(sd_image, mode, input_norm="imagenet")
        if what == "restated":
            out[what] = _train(m, [(torch.from_numpy(want[0]), data.y), (torch.from_numpy(want[1]), y2)], False)
            assert not hasattr(m._engine, "_ra_dev") and not hasattr(m._engine, "_rs_dev")
        else:
            cropper = DeviceRandomResizedCrop().inject([CropDraw(c) for c in crops])
            aug = DeviceRandAugment("rand-m9-n2").inject([_draw(sz, unit_rows[i]) for i in range(2)])
            loader = [((torch.from_numpy(srcs[0]), sizes), data.y), (torch.from_numpy(srcs[1]), y2)]
            out[what] = _train(m, loader, False, graph=what == "graph", device_crop=cropper, device_randaug=aug)
            assert not aug._injected and not cropper._injected and len(m._engine._graphs) == (1 if what == "graph" else 0)
        del m
    for what in ("eager", "graph"):
        assert out[what][0] == out["restated"][0], (what, out[what][0], out["restated"][0])
        _same_bits(out[what][1], out["restated"][1], "%s %s: trainable parameters" % (mode, what))
    assert np.isfinite(out["restated"][0]["loss"])
