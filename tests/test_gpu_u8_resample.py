"""GPU tests of the device crop / resize (pytest -m gpu): dyt_resample_coeffs and dyt_resample_u8 against tests/resample_refs.py -- the numpy
restatement of Pillow's 8-bit bicubic resize that tests/test_resample_refs_host.py pins to Pillow -- and against Pillow's recorded bytes
(tests/golden/resample/resample.npz); args.device_crop / args.device_eval_crop through train_one_epoch and evaluate.

Everything is integer arithmetic on both sides, so every comparison is exact: integer for integer on the coefficient tables, byte for byte
on the images, bit for bit on losses and trainable parameters.  B = 4: batches [4, 64, 64, 3] and one [4, 512, 512, 3] for the wide
kernels; r = 8, C = 10, training loops of depth 2."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import resample_refs as R  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, BMAX, SMOOTH = 10, 8, 97, 4, 0.1
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample", "resample.npz")
T = (224, 224, 0, 0)   # a train row's full size and window

# rows (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags) by batch
SMALL_A = [(64, 64, 37, 11, 1, 1) + T + (0,),                       # a box of 1 x 1
           (48, 64, 20, 30, 8, 10) + T + (0,),                      # upsampling, ksize 5
           (64, 64, 0, 0, 20, 30) + T + (0,),                       # flush with the top-left corner
           (33, 57, 33 - 21, 57 - 40, 21, 40) + T + (0,)]           # flush with the bottom-right corner of a smaller valid extent
SMALL_B = [(64, 64, 0, 64 - 25, 17, 25) + T + (0,),                 # top-right
           (64, 40, 64 - 30, 0, 30, 22) + T + (0,),                 # bottom-left
           (64, 64, 0, 0, 64, 64) + T + (0,),                       # the whole image
           (17, 23, 0, 0, 17, 23, 256, 346, 16, 61, 0)]             # Resize(256) + CenterCrop(224) of a 17 x 23 image
BIG = [(512, 512, 100, 200, 224, 224) + T + (0,),                   # identity
       (512, 512, 0, 22, 512, 490) + T + (0,),                      # scales 2.29 / 2.19: 11 coefficient words, 10 taps
       (300, 400, 0, 0, 300, 400, 256, 341, 16, 58, 0),             # the evaluation row
       (512, 512, 512 - 300, 512 - 280, 300, 280) + T + (0,)]       # flush with the far corner of the padded shape


def _mirrored(rows):
    return [r[:10] + (r[10] ^ 1,) for r in rows]


def _draw(rows):
    from util.crop import CropDraw
    return CropDraw(rows)


def _table(rows, capacity=None):
    return torch.frombuffer(bytearray(_draw(rows).words(capacity)), dtype=torch.int32).to(DEV)


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
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        bad = got.view(torch.int32) != want.view(torch.int32)
        raise AssertionError("%s: %d of %d values differ in their bits" % (what, int(bad.sum()), bad.numel()))


def _padded(rng, rows, hs, ws, fill=0xFF):
    """A batch [len(rows), hs, ws, 3]: random bytes inside each row's valid extent, ``fill`` outside."""
    x = np.full((len(rows), hs, ws, 3), fill, dtype=np.uint8)
    for i, r in enumerate(rows):
        x[i, :r[0], :r[1]] = rng.integers(0, 256, (r[0], r[1], 3), dtype=np.uint8)
    return x


@pytest.fixture(scope="module")
def data():
    """The three batches, their rows and the restatement's bytes for the rows as they are and mirrored: computed once, read only."""
    rng = np.random.default_rng(SEED)
    d = types.SimpleNamespace(rows={"small_a": SMALL_A, "small_b": SMALL_B, "big": BIG}, src={}, want={}, want_m={})
    d.src["small_a"], d.src["small_b"], d.src["big"] = _padded(rng, SMALL_A, 64, 64), _padded(rng, SMALL_B, 64, 64), _padded(rng, BIG, 512, 512)
    for k in d.rows:
        d.want[k] = R.resample_batch(d.src[k], d.rows[k])
        d.want_m[k] = R.resample_batch(d.src[k], _mirrored(d.rows[k]))
        assert np.array_equal(d.want_m[k], d.want[k][:, :, ::-1])
    d.y = torch.tensor([3, 7, 7, 0], dtype=torch.int64)
    return d


def _resample(src, rows, **kw):
    from _lib import resample_u8
    out = resample_u8(torch.from_numpy(np.ascontiguousarray(src)).to(DEV), _table(rows), _draw(rows), **kw)
    torch.cuda.synchronize()
    return out.cpu()


# ---- 1. coefficient tables -----------------------------------------------------------------------------------------------------------------
def test_coefficient_tables_equal_the_restatement_integer_for_integer(data):
    from _lib import resample_coeffs
    widest = 0
    for name, rows in data.rows.items():
        hs, ws = data.src[name].shape[1:3]
        tab = _table(rows)
        for i, row in enumerate(rows):
            got = resample_coeffs(tab, i, hs, ws).cpu().numpy()
            want = R.coeff_table(row)
            assert got.shape == want.shape == (2, 13, 224) and got.dtype == np.int32
            bad = got != want
            assert not bad.any(), "%s row %d %r: %d integers differ, first at %s" % (name, i, row, int(bad.sum()), np.argwhere(bad)[0].tolist())
            widest = max(widest, int(got[:, 1].max()))
    assert widest == 10   # the 512 x 490 box: 11 coefficient words per position, 10 of them taps
    small = R.coeff_table(SMALL_A[1])
    assert small[:, 1].max() <= 5 and R.coeff_table(SMALL_A[0])[:, 1].max() == 1
    ident = R.coeff_table(BIG[0])
    assert np.all(ident[:, 2:].sum(axis=1) == 1 << 22) and np.all(np.abs(ident[:, 2:]).max(axis=1) == 1 << 22)


# ---- 2. output bytes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small_a", "small_b", "big"])
def test_output_bytes_equal_the_restatement_with_and_without_the_mirror(data, name):
    rows = data.rows[name]
    _same_bytes(_resample(data.src[name], rows), data.want[name], name)
    _same_bytes(_resample(data.src[name], _mirrored(rows)), data.want_m[name], name + ", mirrored")
    mixed = [r if i % 2 else m for i, (r, m) in enumerate(zip(rows, _mirrored(rows)))]
    want = np.stack([data.want[name][i] if i % 2 else data.want_m[name][i] for i in range(len(rows))])
    _same_bytes(_resample(data.src[name], mixed), want, name + ", every other image mirrored")
    if name == "big":   # the identity box copies its pixels
        r = rows[0]
        assert np.array_equal(data.want[name][0], data.src[name][0, r[2]:r[2] + 224, r[3]:r[3] + 224])


def test_saturated_checkerboards_clamp_like_the_restatement():
    h = np.add.outer(np.arange(64), np.arange(64))
    src = np.stack([(((h // p) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2) for p in (1, 2, 3, 5)])
    rows = [(64, 64, 1, 2, 60, 45) + T + (1,), (64, 64, 0, 0, 64, 64) + T + (0,), (64, 64, 5, 5, 9, 7) + T + (0,), (64, 64, 0, 0, 33, 64) + T + (1,)]
    want = R.resample_batch(src, rows)
    assert want.min() == 0 and want.max() == 255 and 0 < ((want > 0) & (want < 255)).mean() < 1
    _same_bytes(_resample(src, rows), want, "checkerboards")
    big = np.stack([(((np.add.outer(np.arange(512), np.arange(512)) // p) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2) for p in (1, 3)])
    brows = [(512, 512, 0, 0, 512, 512) + T + (0,), (512, 512, 7, 9, 500, 333) + T + (1,)]
    _same_bytes(_resample(big, brows), R.resample_batch(big, brows), "512-pixel checkerboards, downsampled")


def test_the_golden_sources_give_pillows_recorded_bytes():
    g = np.load(GOLDEN)
    src, rows, want = g["small_src"], [tuple(int(v) for v in r) for r in g["small_rows"]], g["small_out"]
    _same_bytes(_resample(src[:4], rows[:4]), want[:4], "golden rows 0-3")
    _same_bytes(_resample(src[2:6], rows[2:6]), want[2:6], "golden rows 2-5")
    erow = tuple(int(v) for v in g["eval_row"])
    _same_bytes(_resample(g["eval_src"][None], [erow]), g["eval_out"][None], "golden evaluation case")


# ---- 3. mixed batch, padding ---------------------------------------------------------------------------------------------------------------
def test_a_mixed_batch_never_reads_its_padding():
    """Rows of different kinds and valid extents in one batch padded to 96 x 80: the output is the restatement's, whatever the padding holds."""
    rows = [(64, 64, 37, 11, 1, 1) + T + (1,), (96, 80, 0, 0, 96, 80, 256, 307, 16, 41, 0), (33, 57, 12, 17, 21, 40) + T + (0,),
            (90, 31, 2, 0, 88, 31) + T + (1,)]
    rng = np.random.default_rng(SEED + 1)
    ff = _padded(rng, rows, 96, 80, fill=0xFF)
    zero = ff.copy()
    for i, r in enumerate(rows):
        zero[i, r[0]:] = 0
        zero[i, :, r[1]:] = 0
    want = R.resample_batch(zero, rows)
    got_ff, got_zero = _resample(ff, rows), _resample(zero, rows)
    _same_bytes(got_ff, want, "padding 0xFF")
    _same_bytes(got_zero, want, "padding 0x00")
    # boxes flush with the valid extent's far edges are where a padding byte would enter first
    edge = [(r[0], r[1], r[0] - min(r[0], 9), r[1] - min(r[1], 7), min(r[0], 9), min(r[1], 7)) + T + (0,) for r in rows]
    _same_bytes(_resample(ff, edge), R.resample_batch(zero, edge), "boxes at the valid extent's far corner")


# ---- 4. hostile table, refusals ------------------------------------------------------------------------------------------------------------
def test_an_invalid_row_gives_zeros_and_the_others_their_bits(data):
    from _lib import resample_u8
    src = torch.from_numpy(data.src["small_a"]).to(DEV)
    big, low = 2 ** 31 - 1, -2 ** 31
    hostile = [(64, 64, 60, 0, 5, 5) + T + (0,),                     # the box leaves the image by one row
               (65, 64, 0, 0, 65, 64) + T + (0,),                    # the valid extent leaves the batch's padded shape
               (64, 64, 0, 0, 64, 64, 223, 224, 0, 0, 0),            # full < 224
               (64, 64, 0, 0, 64, 64, 224, 224, 1, 0, 0),            # the window leaves `full`
               (64, 64, 0, 0, 0, 64) + T + (0,),                     # an empty box
               (big,) * 11, (low,) * 11, (-1,) * 11,
               (64, 64, big, big, big, big, big, big, big, big, 1),
               (64, 64, 0, 0, 64, 64, 224, 224, low, low, 0)]
    for bad in hostile:
        for at in (0, 2, 3):
            rows = list(SMALL_A)
            words = bytearray(_draw(rows).words())
            words[64 + 48 * at:64 + 48 * at + 44] = struct.pack("<11i", *bad)
            tab = torch.frombuffer(words, dtype=torch.int32).to(DEV)
            out = torch.full((4, 224, 224, 3), 0xAA, dtype=torch.uint8, device=DEV)
            resample_u8(src, tab, None, out=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not got[at].any(), (bad, at)
            keep = [i for i in range(4) if i != at]
            _same_bytes(got[keep], data.want["small_a"][keep], "the valid rows beside %r at %d" % (bad, at))
    # fewer units than images: the images without a row are zeros; another filter: all of them
    for units, filt, zeros in ((2, 3, [2, 3]), (0, 3, [0, 1, 2, 3]), (-5, 3, [0, 1, 2, 3]), (4, 2, [0, 1, 2, 3]), (4, 0, [0, 1, 2, 3]), (big, 3, [])):
        words = bytearray(_draw(SMALL_A).words())
        words[0:8] = struct.pack("<2i", filt, units)
        out = torch.full((4, 224, 224, 3), 0xAA, dtype=torch.uint8, device=DEV)
        resample_u8(src, torch.frombuffer(words, dtype=torch.int32).to(DEV), None, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(4):
            if i in zeros:
                assert not got[i].any(), (units, filt, i)
            else:
                _same_bytes(got[i], data.want["small_a"][i], "units %d filter %d image %d" % (units, filt, i))


def test_refusals_come_as_texts_with_nothing_enqueued(data):
    import _lib
    from _lib import DyTError, resample_u8
    src = torch.from_numpy(data.src["small_a"]).to(DEV)
    tab = _table(SMALL_A)
    out = torch.full((4, 224, 224, 3), 0xAA, dtype=torch.uint8, device=DEV)
    need = 4 * 23296
    scr = torch.zeros(need // 4 + 4, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        bad = {"null src": (None, 4, 64, 64, p(out), p(tab), 4, p(scr), need), "misaligned src": (p(src, 8), 4, 64, 64, p(out), p(tab), 4, p(scr), need),
               "misaligned dst": (p(src), 4, 64, 64, p(out, 4), p(tab), 4, p(scr), need), "misaligned table": (p(src), 4, 64, 64, p(out), p(tab, 4), 4, p(scr), need),
               "misaligned scratch": (p(src), 4, 64, 64, p(out), p(tab), 4, p(scr, 4), need), "batch above capacity": (p(src), 4, 64, 64, p(out), p(tab), 3, p(scr), need),
               "small scratch": (p(src), 4, 64, 64, p(out), p(tab), 4, p(scr), need - 4), "batch 0": (p(src), 0, 64, 64, p(out), p(tab), 4, p(scr), need),
               "side above 4096": (p(src), 4, 64, 4097, p(out), p(tab), 4, p(scr), need)}
        for what, a in bad.items():
            assert L.dyt_resample_u8(*a, None) == -1, what
            assert b"dyt_resample_u8: resample:" in L.dyt_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == 0xAA).all()) and not bool(scr.any())   # nothing ran
    # the Python layer refuses an invalid draw before upload, and what the binding cannot take
    from util.crop import CropDraw
    with pytest.raises(DyTError, match="valid extent"):
        resample_u8(src, tab, CropDraw([(65, 64, 0, 0, 10, 10) + T + (0,)] * 4))
    with pytest.raises(DyTError, match="holds 3 images"):
        resample_u8(src, tab, CropDraw(SMALL_A[:3]))
    for x in (src.permute(0, 3, 1, 2).contiguous(), src.float(), src.cpu(), src[None]):
        with pytest.raises(DyTError):
            resample_u8(x, tab)
    with pytest.raises(DyTError, match="table"):
        resample_u8(src, tab[:16 + 12 * 3].contiguous())


# ---- 5. - 7. the loops ---------------------------------------------------------------------------------------------------------------------
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


def _train(model, loader, mixup_fn=None, graph=False, lr=1e-3, **extra):
    from engine_finetune import FusedAdamW, train_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph, **extra)
    stats = train_one_epoch(model, _criterion(), loader, opt, DEV, 0, None, 0, mixup_fn, None, args=args)
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone()


def _augment():
    from util.erasing import DeviceRandomErasing, EraseDraw
    from util.mixup import DeviceMixup, MixDraw
    ed = [EraseDraw("pixel", [[(0, 5, 0, 7)], [(10, 3, 3, 2), (20, 3, 15, 2)], [], [(100, 30, 60, 17)]], seed=0x243F6A8885A308D3),
          EraseDraw("const", [[], [(0, 223, 0, 223)], [(5, 9, 220, 4)], [(30, 50, 30, 50)]])]
    md = [MixDraw.mixup(0.31415926).with_targets(SMOOTH, C), MixDraw.cutmix((20, 90, 25, 70)).with_targets(SMOOTH, C)]
    return DeviceRandomErasing(mode="pixel").inject(ed), DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(md)


@pytest.mark.parametrize("mode,augment", [("masked", True), ("masked", False), ("compact", True), ("compact", False)])
def test_two_steps_of_the_loop_equal_the_loop_fed_the_restatements_bytes(mode, augment, sd2, data, monkeypatch):
    """train_one_epoch with args.device_crop holding two injected draws -- a (pixels, sizes) batch, then a bare uint8 batch that every image
    fills -- eager and from a captured graph, against the same loop fed the 224 x 224 byte batches tests/resample_refs.py makes of them."""
    from util.crop import DeviceRandomResizedCrop
    monkeypatch.setenv("DYT_PREFETCH", "0")
    full = [(64, 64, 3 * i, 2 * i, 40 + i, 50 - i) + T + (i & 1,) for i in range(4)]
    draws = [_mirrored(SMALL_A)[:2] + SMALL_A[2:], full]
    srcs = [data.src["small_a"], data.src["small_b"]]
    sizes = torch.tensor([r[:2] for r in SMALL_A], dtype=torch.int32)
    want = [torch.from_numpy(R.resample_batch(srcs[i], draws[i])) for i in range(2)]
    assert np.array_equal(want[0].numpy()[2:], data.want["small_a"][2:])
    crop_loader = [((torch.from_numpy(srcs[0]), sizes), data.y), (torch.from_numpy(srcs[1]), data.y.flip(0).contiguous())]
    plain_loader = [(want[0], data.y), (want[1], data.y.flip(0).contiguous())]
    out = {}
    for what in ("bytes", "crop eager", "crop graph"):
        m = _model(sd2, mode, input_norm="imagenet")
        eraser, mixer = _augment() if augment else (None, None)
        extra = {} if eraser is None else {"random_erasing": eraser}
        if what == "bytes":
            out[what] = _train(m, plain_loader, mixer, **extra)
            assert not hasattr(m._engine, "_rs_dev")   # no table, no scratch: no resample launch
        else:
            cropper = DeviceRandomResizedCrop().inject([_draw(d) for d in draws])
            out[what] = _train(m, crop_loader, mixer, graph=what.endswith("graph"), device_crop=cropper, **extra)
            assert not cropper._injected and len(m._engine._graphs) == (1 if what.endswith("graph") else 0)   # one capture serves both draws
        del m
    for what in ("crop eager", "crop graph"):
        assert out[what][0] == out["bytes"][0], (what, out[what][0], out["bytes"][0])
        _same_bits(out[what][1], out["bytes"][1], "%s %s augment=%s: trainable parameters" % (mode, what, augment))
    assert np.isfinite(out["bytes"][0]["loss"])


def test_the_prefetcher_carries_source_batches(sd2, data):
    """With the prefetcher on (its default) the loop's result is the same: the pixels travel, the sizes stay on the host."""
    from util.crop import DeviceRandomResizedCrop
    draws = [SMALL_A, SMALL_B, SMALL_A]
    src = [data.src["small_a"], data.src["small_b"], data.src["small_a"]]
    loader = [((torch.from_numpy(src[i]).pin_memory(), torch.tensor([r[:2] for r in draws[i]], dtype=torch.int32)), data.y) for i in range(3)]
    plain = [(torch.from_numpy(R.resample_batch(src[i], draws[i])), data.y) for i in range(3)]
    ma, mb = _model(sd2, "compact", input_norm="imagenet"), _model(sd2, "compact", input_norm="imagenet")
    sa, fa = _train(ma, loader, device_crop=DeviceRandomResizedCrop().inject([_draw(d) for d in draws]))
    sb, fb = _train(mb, plain)
    assert sa == sb, (sa, sb)
    _same_bits(fa, fb, "prefetched source batches: trainable parameters")
    del ma, mb


@pytest.mark.parametrize("stream", [False, True])
def test_evaluate_with_the_device_eval_crop_equals_evaluate_on_the_restatements_bytes(stream, sd2, data):
    from engine_finetune import evaluate
    from util.crop import DeviceResizeCenterCrop
    crop = DeviceResizeCenterCrop()
    sizes = [[r[:2] for r in SMALL_A], [r[:2] for r in SMALL_B]]
    srcs = [data.src["small_a"], data.src["small_b"]]
    rows = [crop.draw_for(s).rows for s in sizes]
    assert rows[1][3] == SMALL_B[3] and rows[0][0][6:10] == (256, 256, 16, 16)
    want = [torch.from_numpy(R.resample_batch(srcs[i], rows[i])) for i in range(2)]
    m = _model(sd2, "compact", input_norm="imagenet")
    loader = [((torch.from_numpy(srcs[i]), torch.tensor(sizes[i], dtype=torch.int32)), data.y) for i in range(2)]
    got = evaluate(loader, m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream, device_eval_crop=crop))
    ref = evaluate([(want[i], data.y) for i in range(2)], m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream))
    assert got == ref, (got, ref)
    assert 0.0 <= got["metric"] <= 100.0 and 0.0 < got["keep_ratio"] <= 1.0
    # the cropped batch is the restatement's
    _same_bytes(crop(torch.from_numpy(srcs[0]).to(DEV), sizes[0]), want[0], "DeviceResizeCenterCrop.__call__")
    del m


def test_without_the_two_args_nothing_changes(sd2, data, monkeypatch):
    """A plain 224 byte batch goes through the loop untouched: the same losses and parameters as the direct fused step on it, and no resample
    buffer is ever allocated; a model without input_norm and a clip are refused with a text."""
    import engine_finetune as E
    from _lib import DyTError
    from util.crop import DeviceRandomResizedCrop
    monkeypatch.setenv("DYT_PREFETCH", "0")
    x = torch.from_numpy(data.want["small_a"])
    ma, mb = _model(sd2, "compact", input_norm="imagenet"), _model(sd2, "compact", input_norm="imagenet")
    sa, fa = _train(ma, [(x, data.y)], device_crop=None, device_eval_crop=None)
    opt = E.FusedAdamW(mb, lr=1e-3, weight_decay=0.01)
    E.lr_sched.adjust_learning_rate(opt, 0.0, types.SimpleNamespace(lr=1e-3, min_lr=0.0, warmup_epochs=0, epochs=10))
    mb.train(True)
    losses = torch.zeros(8, device=DEV)
    E.train_step(mb, x.to(DEV), data.y.to(DEV), opt, _criterion(), losses_out=losses, seed=E.step_seed(0, 0))
    torch.cuda.synchronize()
    assert sa["loss"] == float(losses[0]) and not hasattr(ma._engine, "_rs_dev") and not hasattr(mb._engine, "_rs_dev")
    _same_bits(fa, mb._engine.flat, "the loop without the args against the direct step")
    plain = _model(sd2, "compact")
    with pytest.raises(DyTError, match="input_norm"):
        _train(plain, [(x, data.y)], device_crop=DeviceRandomResizedCrop())
    with pytest.raises(DyTError, match="video clips"):
        _train(ma, [(torch.zeros(2, 2, 64, 64, 3, dtype=torch.uint8), data.y[:2])], device_crop=DeviceRandomResizedCrop())
    del ma, mb, plain
