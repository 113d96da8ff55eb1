"""GPU tests of the device clip pipeline (pytest -m gpu): dyt_resample_clip_coeffs and dyt_resample_clip_f32 against
tests/clip_resample_refs.py -- the numpy restatement of torch's float bilinear interpolate that tests/test_clip_resample_refs_host.py pins
to the reference's recorded output and to live torch -- and against the reference's recorded bits
(tests/golden/resample/clip_resample.npz); args.device_crop / args.device_eval_crop through the video train_one_epoch and evaluate_video.

Both sides evaluate the same correctly rounded fp32 operations in the same order, so every comparison is exact: integer for integer and
bit for bit on the taps and weights, bit for bit on the clips, the losses and the trainable parameters.  B = 2 clips of T = 2 frames:
batches [2, 2, 64, 64, 3] and one [2, 2, 300, 400, 3]; r = 8, C = 10, models of depth 2."""
import ctypes
import os
import struct
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_resample_refs as R  # noqa: E402
import gpu_diag as D  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, T, SMOOTH = 10, 8, 131, 2, 0.1
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample", "clip_resample.npz")
W = (224, 224, 0, 0)   # a random-resized-crop row's full size and window

# rows (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags, src); clip 0 is 48 x 64, clip 1 is 64 x 40
SMALL = [(48, 64, 37, 11, 1, 1) + W + (0, 0),                           # a box of 1 x 1
         (48, 64, 20, 30, 8, 10) + W + (0, 0),                          # 8 x 10 upsampled
         (48, 64, 0, 0, 20, 30) + W + (0, 0),                           # flush with the top-left corner
         (64, 40, 0, 40 - 25, 17, 25) + W + (0, 1),                     # top-right
         (64, 40, 64 - 30, 0, 30, 22) + W + (0, 1),                     # bottom-left
         (48, 64, 48 - 21, 64 - 40, 21, 40) + W + (0, 0),               # bottom-right of the smaller valid extent
         (48, 64, 0, 0, 48, 64, 227, 302, 1, 67, 0, 0),                 # scale jitter + crop
         (64, 40, 0, 0, 64, 40, 358, 224, 134, 0, 0, 1)]                # the third evaluation view of a tall clip
BIG = [(300, 400, 38, 100, 224, 224) + W + (0, 0),                      # identity
       (300, 400, 0, 0, 300, 400, 224, 298, 0, 0, 0, 1),                # the three evaluation views of clip 1: 300 x 400 -> 224 x 298
       (300, 400, 0, 0, 300, 400, 224, 298, 0, 37, 0, 1),
       (300, 400, 0, 0, 300, 400, 224, 298, 0, 74, 0, 1),
       (300, 400, 300 - 290, 400 - 390, 290, 390, 241, 320, 17, 96, 0, 0)]   # flush with the far corner of the padded shape, downscaled


def _mirrored(rows):
    return [r[:10] + (r[10] ^ 1,) + r[11:] for r in rows]


def _draw(rows):
    from util.crop import BILINEAR_F32, CropDraw
    return CropDraw(rows, filter=BILINEAR_F32)


def _table(rows, capacity=None):
    return torch.frombuffer(bytearray(_draw(rows).words(capacity)), dtype=torch.int32).to(DEV)


def _same_bits(got, want, what):
    got = torch.as_tensor(got).detach().cpu().contiguous()
    want = torch.as_tensor(want).detach().cpu().contiguous()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape, got.dtype)
    bad = got.view(torch.int32) != want.view(torch.int32)
    if bool(bad.any()):
        where = torch.nonzero(bad)[0].tolist()
        raise AssertionError("%s: %d of %d values differ in their bits (first at %s: got %r, want %r)" % (
            what, int(bad.sum()), bad.numel(), where, float(got[tuple(where)]), float(want[tuple(where)])))


def _padded(rng, sizes, hs, ws, fill=0xFF):
    """A batch [len(sizes), T, hs, ws, 3]: random bytes inside each clip's valid extent, ``fill`` outside."""
    x = np.full((len(sizes), T, hs, ws, 3), fill, dtype=np.uint8)
    for i, (h, w) in enumerate(sizes):
        x[i, :, :h, :w] = rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
    return x


@pytest.fixture(scope="module")
def data():
    """The two batches, their rows and the restatement's clips [units, T, 3, 224, 224]: computed once, read only."""
    rng = np.random.default_rng(SEED)
    d = types.SimpleNamespace(rows={"small": SMALL, "big": BIG}, sizes={"small": [(48, 64), (64, 40)], "big": [(300, 400), (300, 400)]}, src={}, want={})
    d.src["small"], d.src["big"] = _padded(rng, d.sizes["small"], 64, 64), _padded(rng, d.sizes["big"], 300, 400)
    for k in d.rows:
        d.want[k] = R.resample_batch(d.src[k], d.rows[k])
    d.y = torch.tensor([3, 7], dtype=torch.int64)
    return d


def _resample(src, rows, norm=None, **kw):
    """fp32 [units, T, 3, 224, 224] on the host"""
    from _lib import resample_clip_f32
    out = resample_clip_f32(torch.from_numpy(np.ascontiguousarray(src)).to(DEV), _table(rows), _draw(rows), norm=norm, **kw)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (len(rows), 3, src.shape[1], 224, 224)
    back = out.permute(0, 2, 1, 3, 4)
    assert back.is_contiguous()   # the [units, 3, T, 224, 224] result is a view of the kernel's [units, T, 3, 224, 224]
    return back.cpu()


# ---- 1. taps and weights ---------------------------------------------------------------------------------------------------------------------
def test_taps_and_weights_equal_the_restatement_integer_for_integer_and_bit_for_bit(data):
    from _lib import resample_clip_coeffs
    for name, rows in data.rows.items():
        hs, ws = data.src[name].shape[2:4]
        tab = _table(rows)
        for i, row in enumerate(rows):
            got = resample_clip_coeffs(tab, i, hs, ws).cpu().numpy()
            want = R.coeff_table(row)
            assert got.shape == want.shape == (2, 4, 224) and got.dtype == np.int32
            bad = got != want
            assert not bad.any(), "%s row %d %r: %d words differ, first at %s" % (name, i, row, int(bad.sum()), np.argwhere(bad)[0].tolist())
    ident = R.coeff_table(BIG[0])
    assert np.array_equal(ident[:, 0], np.tile(np.arange(224), (2, 1))) and not ident[:, 3].any() and np.all(ident[:, 2] == np.float32(1).view(np.int32))
    up = R.coeff_table(SMALL[1])
    assert up[0, 1].max() == 7 and up[1, 1].max() == 9 and up[:, 0].min() == 0
    ev = R.coeff_table(BIG[2])
    assert ev[1, 0, 0] == 49 and ev[1, 1].max() <= 399     # window column 0 = position 37 of 298: real = 400 / 298 * 37.5 - 0.5 = 49.8
    one = R.coeff_table(SMALL[0])
    assert not one[:, :2].any()
    # an invalid row gives zeros
    words = bytearray(_draw(SMALL).words())
    words[64:64 + 48] = struct.pack("<12i", 65, 64, 0, 0, 65, 64, 224, 224, 0, 0, 0, 0)
    assert not resample_clip_coeffs(torch.frombuffer(words, dtype=torch.int32).to(DEV), 0, 64, 64).any()


# ---- 2. clip bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "big"])
def test_clip_bits_equal_the_restatement_with_and_without_the_mirror(data, name):
    rows = data.rows[name]
    _same_bits(_resample(data.src[name], rows), data.want[name], name)
    want_m = data.want[name][..., ::-1].copy()
    _same_bits(_resample(data.src[name], _mirrored(rows)), want_m, name + ", mirrored")
    assert np.array_equal(R.resample_batch(data.src[name], _mirrored(rows[:2])), want_m[:2])
    mixed = [r if i % 2 else m for i, (r, m) in enumerate(zip(rows, _mirrored(rows)))]
    want = np.stack([data.want[name][i] if i % 2 else want_m[i] for i in range(len(rows))])
    _same_bits(_resample(data.src[name], mixed), want, name + ", every other unit mirrored")
    if name == "big":   # the identity box is the normalised bytes themselves
        r = rows[0]
        box = data.src[name][0, :, r[2]:r[2] + 224, r[3]:r[3] + 224]
        tab = R.norm_table()
        assert np.array_equal(data.want[name][0], np.stack([tab[c][box[..., c]] for c in range(3)], axis=1))


def test_a_clip_that_ends_off_a_16_byte_chunk_is_staged_byte_by_byte_at_its_end():
    """One frame of 5 x 7 pixels is 105 bytes: the last source row's span ends at the allocation's last byte, so its second 16-byte chunk
    crosses the end and is filled byte by byte (every other source here is a whole number of chunks)."""
    src = np.random.default_rng(SEED + 5).integers(0, 256, (1, 1, 5, 7, 3), dtype=np.uint8)
    rows = [(5, 7, 0, 0, 5, 7) + W + (0, 0)]
    _draw(rows).check(5, 7, 1)      # legal for this route
    assert src.nbytes == 105 and src.nbytes % 16 != 0 and (4 * 7 * 3) // 16 * 16 + 32 > src.nbytes
    want = R.resample_batch(src, rows)
    _same_bits(_resample(src, rows), want, "5 x 7")
    _same_bits(_resample(src, _mirrored(rows)), want[..., ::-1].copy(), "5 x 7, mirrored")


def test_another_norm_and_both_frames_of_a_clip_come_from_one_row(data):
    norm = ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711))
    rows = [SMALL[6], SMALL[7], SMALL[3]]
    got = _resample(data.src["small"], rows, norm)
    _same_bits(got, R.resample_batch(data.src["small"], rows, norm), "the reference's default mean / std")
    assert not np.array_equal(got[:, 0].numpy(), got[:, 1].numpy())
    # frame f of a unit depends on frame f of its source alone: the frames swapped give the frames of the output swapped
    swapped = np.ascontiguousarray(data.src["small"][:, ::-1])
    _same_bits(_resample(swapped, rows, norm), got.flip(1), "frames swapped")
    # and each frame alone is what a one-frame clip gives
    for f in range(T):
        _same_bits(_resample(data.src["small"][:, f:f + 1], rows, norm), got[:, f:f + 1], "frame %d alone" % f)


def test_three_view_rows_share_one_source_clip(data):
    """The three evaluation rows of BIG read clip 1 only; the units are windows of one resized clip."""
    rows = BIG[1:4]
    got = _resample(data.src["big"], rows)
    _same_bits(got, data.want["big"][1:4], "three views")
    assert np.array_equal(got[0][..., 37:].numpy(), got[1][..., :224 - 37].numpy()) and np.array_equal(got[1][..., 37:].numpy(), got[2][..., :224 - 37].numpy())
    other = data.src["big"].copy()
    other[0] = 0
    _same_bits(_resample(other, rows), got, "clip 0 is not read")
    # more units than clips, and fewer
    _same_bits(_resample(data.src["big"][1:], [r[:11] + (0,) for r in rows]), got, "a batch of one clip, three units")
    _same_bits(_resample(data.src["big"], BIG[:1]), data.want["big"][:1], "a batch of two clips, one unit")


# ---- 3. padding ------------------------------------------------------------------------------------------------------------------------------
def test_padding_never_reaches_an_output(data):
    rows = SMALL + [(48, 64, 48 - 9, 64 - 7, 9, 7) + W + (1, 0), (64, 40, 64 - 9, 40 - 7, 9, 7) + W + (0, 1), (64, 40, 0, 0, 64, 40, 258, 224, 34, 0, 1, 1)]
    ff = data.src["small"]
    zero = ff.copy()
    for i, (h, w) in enumerate(data.sizes["small"]):
        zero[i, :, h:] = 0
        zero[i, :, :, w:] = 0
    assert (ff != zero).any()
    want = R.resample_batch(zero, rows)
    _same_bits(_resample(ff, rows), want, "padding 0xFF")
    _same_bits(_resample(zero, rows), want, "padding 0x00")


# ---- 4. golden -------------------------------------------------------------------------------------------------------------------------------
def test_the_golden_sources_give_the_references_recorded_bits():
    g = np.load(GOLDEN)
    norm = (tuple(g["norm"][0].tolist()), tuple(g["norm"][1].tolist()))
    rows, idx, frames = [tuple(int(v) for v in r) for r in g["px_rows"]], g["px_index"], g["px_frames"]
    got = _resample(g["px_src"], rows, norm).numpy()
    _same_bits(got[0, 0], g["px_full"], "golden row 0, frame 0, in full")
    for i in range(len(rows)):
        t = int(frames[i])
        _same_bits(np.ascontiguousarray(got[i, :t][:, :, idx][:, :, :, idx]), g["px_samples"][i, :t], "golden row %d %r" % (i, rows[i]))
    erows = [tuple(int(v) for v in r) for r in g["eval_rows"]]
    got = _resample(g["eval_src"][None], erows, norm).numpy()
    _same_bits(np.ascontiguousarray(got[:, :, :, idx][:, :, :, :, idx]), g["eval_samples"][:, :1], "golden evaluation views")


# ---- 5. hostile table, refusals --------------------------------------------------------------------------------------------------------------
def test_an_invalid_row_gives_a_zero_unit_and_the_others_their_bits(data):
    from _lib import resample_clip_f32
    src = torch.from_numpy(data.src["small"]).to(DEV)
    rows = SMALL[:4]
    want = data.want["small"][:4]
    big, low = 2 ** 31 - 1, -2 ** 31
    hostile = [(48, 64, 44, 0, 5, 5) + W + (0, 0),                       # the box leaves the clip by one row
               (65, 64, 0, 0, 65, 64) + W + (0, 0),                      # the valid extent leaves the batch's padded shape
               (48, 64, 0, 0, 48, 64, 223, 224, 0, 0, 0, 0),             # full < 224
               (48, 64, 0, 0, 48, 64, (1 << 23) + 1, 224, 0, 0, 0, 0),   # full above the bound
               (48, 64, 0, 0, 48, 64, 224, 224, 1, 0, 0, 0),             # the window leaves `full`
               (48, 64, 0, 0, 0, 64) + W + (0, 0),                       # an empty box
               (48, 64, 0, 0, 48, 64) + W + (0, 2),                      # a source clip the batch does not have
               (48, 64, 0, 0, 48, 64) + W + (0, -1),
               (big,) * 12, (low,) * 12, (-1,) * 12,
               (48, 64, big, big, big, big, big, big, big, big, 1, 0),
               (48, 64, 0, 0, 48, 64, 224, 224, low, low, 0, big)]
    for bad in hostile:
        for at in (0, 3):
            words = bytearray(_draw(rows).words())
            words[64 + 48 * at:64 + 48 * at + 48] = struct.pack("<12i", *bad)
            tab = torch.frombuffer(words, dtype=torch.int32).to(DEV)
            out = torch.full((4, T, 3, 224, 224), 7.0, dtype=torch.float32, device=DEV)
            resample_clip_f32(src, tab, None, out=out, units=4)
            torch.cuda.synchronize()
            got = out.cpu()
            assert not got[at].any(), (bad, at)
            keep = [i for i in range(4) if i != at]
            _same_bits(got[keep], want[keep], "the valid units beside %r at %d" % (bad, at))
    # fewer units than rows asked for: the units without a row are zeros; another filter code: all of them
    for units, filt, zeros in ((2, 2, [2, 3]), (0, 2, [0, 1, 2, 3]), (-5, 2, [0, 1, 2, 3]), (4, 3, [0, 1, 2, 3]), (4, 0, [0, 1, 2, 3]), (big, 2, [])):
        words = bytearray(_draw(rows).words())
        words[0:8] = struct.pack("<2i", filt, units)
        out = torch.full((4, T, 3, 224, 224), 7.0, dtype=torch.float32, device=DEV)
        resample_clip_f32(src, torch.frombuffer(words, dtype=torch.int32).to(DEV), None, out=out, units=4)
        torch.cuda.synchronize()
        got = out.cpu()
        for i in range(4):
            if i in zeros:
                assert not got[i].any(), (units, filt, i)
            else:
                _same_bits(got[i], want[i], "units %d filter %d unit %d" % (units, filt, i))


def test_refusals_come_as_texts_and_leave_the_destination_untouched(data):
    import _lib
    from _lib import DyTError, resample_clip_f32
    src = torch.from_numpy(data.src["small"]).to(DEV)
    rows = SMALL[:4]
    tab = _table(rows)
    out = torch.full((4, T, 3, 224, 224), 7.0, dtype=torch.float32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731
    f3 = lambda *v: (ctypes.c_float * 3)(*v)   # noqa: E731
    mean, std = f3(0.485, 0.456, 0.406), f3(0.229, 0.224, 0.225)
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        bad = {"null src": (None, 2, T, 64, 64, p(out), 4, p(tab), 4, mean, std), "misaligned src": (p(src, 8), 2, T, 64, 64, p(out), 4, p(tab), 4, mean, std),
               "misaligned dst": (p(src), 2, T, 64, 64, p(out, 4), 4, p(tab), 4, mean, std), "misaligned table": (p(src), 2, T, 64, 64, p(out), 4, p(tab, 4), 4, mean, std),
               "units above capacity": (p(src), 2, T, 64, 64, p(out), 4, p(tab), 3, mean, std), "batch 0": (p(src), 0, T, 64, 64, p(out), 4, p(tab), 4, mean, std),
               "frames 0": (p(src), 2, 0, 64, 64, p(out), 4, p(tab), 4, mean, std), "units 0": (p(src), 2, T, 64, 64, p(out), 0, p(tab), 4, mean, std),
               "side above 4096": (p(src), 2, T, 64, 4097, p(out), 4, p(tab), 4, mean, std), "std 0": (p(src), 2, T, 64, 64, p(out), 4, p(tab), 4, mean, f3(0.2, 0.0, 0.2)),
               "std nan": (p(src), 2, T, 64, 64, p(out), 4, p(tab), 4, mean, f3(0.2, float("nan"), 0.2))}
        for what, a in bad.items():
            assert L.dyt_resample_clip_f32(*a, None) == -1, what
            assert b"dyt_resample_clip_f32: resample clip:" in L.dyt_last_error(), what
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing ran
    # the Python layer refuses an invalid draw before upload, and what the binding cannot take
    with pytest.raises(DyTError, match="valid extent"):
        resample_clip_f32(src, tab, _draw([(65, 64, 0, 0, 10, 10) + W + (0, 0)]))
    with pytest.raises(DyTError, match="source clip"):
        resample_clip_f32(src, tab, _draw([(48, 64, 0, 0, 10, 10) + W + (0, 2)]))
    from util.crop import CropDraw
    with pytest.raises(DyTError, match="image rows"):
        resample_clip_f32(src, tab, CropDraw([(48, 64, 0, 0, 10, 10) + W + (0,)]))
    for x in (src[0], src.float(), src.cpu(), src.permute(0, 1, 4, 2, 3).contiguous()):
        with pytest.raises(DyTError):
            resample_clip_f32(x, tab)
    with pytest.raises(DyTError, match="table"):
        resample_clip_f32(src, tab[:16 + 12 * 3].contiguous(), units=4)
    assert bool((out == 7.0).all())


# ---- 6. - 8. the loops -----------------------------------------------------------------------------------------------------------------------
def _model(sd, mode, max_batch=2 * T, **kw):
    from video_models.video_vision_transformer_IN21K import VisionTransformer
    tuning = D.Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option="none", ffn_adapter_init_option="lora",
                   ffn_adapter_scalar="0.1", ffn_num=RANK, d_model=768)
    m = VisionTransformer(patch_size=16, embed_dim=768, depth=2, num_heads=12, mlp_ratio=4.0, qkv_bias=True, num_classes=C, drop_path_rate=0.0,
                          tuning_config=tuning, select_config=D.Cfg(open=True, keep_layers=0), precision="fp16", train_mode=mode, max_batch=max_batch, **kw)
    m.load_state_dict(sd)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m.cuda()


@pytest.fixture(scope="module")
def sd2():
    return synth.make_state_dict(C, RANK, seed=SEED, kind="test", depth=2, gate_bias=0.85, video=True)


def _criterion():
    from models.losses import AdaLoss
    return AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)


def _train(model, loader, mixup_fn=None, graph=False, lr=1e-3, **extra):
    from engine_finetune import FusedAdamW, train_video_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph, **extra)
    stats = train_video_one_epoch(model, _criterion(), loader, opt, DEV, 0, None, 0, mixup_fn, None, args=args)
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone()


def _mixer():
    from util.mixup import DeviceMixup, MixDraw
    md = [MixDraw.mixup(0.31415926).with_targets(SMOOTH, C), MixDraw.cutmix((20, 90, 25, 70)).with_targets(SMOOTH, C)]
    return DeviceMixup(label_smoothing=SMOOTH, num_classes=C).inject(md)


def _float_clips(src, rows):
    """[units, 3, T, 224, 224] fp32, contiguous: what a host pipeline would hand the loop"""
    return torch.from_numpy(R.resample_batch(src, rows)).permute(0, 2, 1, 3, 4).contiguous()


@pytest.mark.parametrize("mode,mix", [("masked", True), ("masked", False), ("compact", True), ("compact", False)])
def test_two_steps_of_the_video_loop_equal_the_loop_fed_the_restatements_clips(mode, mix, sd2, data, monkeypatch):
    """train_video_one_epoch with args.device_crop holding two injected draws -- a (clips, sizes) batch, then a bare uint8 batch that every
    clip fills -- eager and from a captured graph, against the same loop fed the float clips tests/clip_resample_refs.py makes of them."""
    from util.crop import DeviceClipRandomResizedCrop, DeviceClipScaleJitterCrop
    monkeypatch.setenv("DYT_PREFETCH", "0")
    first = [SMALL[6][:10] + (1, 0), SMALL[7]]                                            # scale jitter rows, one mirrored
    second = [(64, 64, 3, 2, 40, 50) + W + (0, 0), (64, 64, 0, 9, 64, 31) + W + (1, 1)]   # boxes of clips that fill the padded shape
    draws, srcs = [first, second], [data.src["small"], data.src["small"][::-1].copy()]
    sizes = torch.tensor(data.sizes["small"], dtype=torch.int32)
    want = [_float_clips(srcs[i], draws[i]) for i in range(2)]
    crop_loader = [((torch.from_numpy(srcs[0]), sizes), data.y), (torch.from_numpy(srcs[1]), data.y.flip(0).contiguous())]
    plain_loader = [(want[0], data.y), (want[1], data.y.flip(0).contiguous())]
    out = {}
    for what in ("float", "crop eager", "crop graph"):
        m = _model(sd2, mode, input_norm="imagenet")
        mixer = _mixer() if mix else None
        if what == "float":
            out[what] = _train(m, plain_loader, mixer)
            assert getattr(m._engine, "_rc_dev", None) is None   # no table, no buffer: no resample launch
        else:
            kind = DeviceClipScaleJitterCrop if what.endswith("eager") else DeviceClipRandomResizedCrop
            cropper = kind().inject([_draw(d) for d in draws])
            out[what] = _train(m, crop_loader, mixer, graph=what.endswith("graph"), device_crop=cropper)
            assert not cropper._injected and len(m._engine._graphs) == (1 if what.endswith("graph") else 0)   # one capture serves both draws
            assert getattr(m._engine, "_rs_dev", None) is None and tuple(m._engine._rc_out.shape) == (2, T, 3, 224, 224)
        del m
    for what in ("crop eager", "crop graph"):
        assert out[what][0] == out["float"][0], (what, out[what][0], out["float"][0])
        _same_bits(out[what][1], out["float"][1], "%s %s mix=%s: trainable parameters" % (mode, what, mix))
    assert np.isfinite(out["float"][0]["loss"])


def test_the_prefetcher_carries_source_clips(sd2, data):
    """With the prefetcher on (its default) the loop's result is the same: the clips travel, the sizes stay on the host, and the one-off
    copy-stream probe of the first batch runs on a fixed crop that consumes no draw."""
    from util.crop import DeviceClipScaleJitterCrop
    draws = [[SMALL[6], SMALL[7]], [SMALL[1], SMALL[3]], [SMALL[6][:10] + (1, 0), SMALL[4]]]
    sizes = torch.tensor(data.sizes["small"], dtype=torch.int32)
    loader = [((torch.from_numpy(data.src["small"]).pin_memory(), sizes), data.y) for _ in range(3)]
    plain = [(_float_clips(data.src["small"], d), data.y) for d in draws]
    ma, mb = _model(sd2, "compact", input_norm="imagenet"), _model(sd2, "compact", input_norm="imagenet")
    cropper = DeviceClipScaleJitterCrop().inject([_draw(d) for d in draws])
    sa, fa = _train(ma, loader, device_crop=cropper)
    sb, fb = _train(mb, plain)
    assert sa == sb, (sa, sb)
    assert not cropper._injected
    _same_bits(fa, fb, "prefetched source clips: trainable parameters")
    del ma, mb


@pytest.mark.parametrize("stream", [False, True])
@pytest.mark.parametrize("views", [(3, 1), (1, 3)])
def test_evaluate_video_with_the_device_eval_crop_equals_evaluate_video_on_host_cropped_views(views, stream, sd2, data):
    """(temporal, spatial) views: 3 x 1 from a [B, 3, T, Hs, Ws, 3] source, 1 x 3 from a [B, T, Hs, Ws, 3] source."""
    from engine_finetune import evaluate_video
    from util.crop import DeviceClipUniformCrop
    vt, vs = views
    crop = DeviceClipUniformCrop(spatial_views=vs)
    rng = np.random.default_rng(SEED + vt)
    sizes = data.sizes["small"]
    loader, ref_loader = [], []
    for b in range(2):   # two batches of B = 2
        src = np.stack([_padded(rng, sizes, 64, 64) for _ in range(vt)], axis=1)          # [B, Vt, T, 64, 64, 3]
        flat = src.reshape(2 * vt, T, 64, 64, 3)
        rows = crop.draw_for([s for s in sizes for _ in range(vt)]).rows
        assert len(rows) == 2 * vt * vs and [r[11] for r in rows] == [i for i in range(2 * vt) for _ in range(vs)]
        host = torch.from_numpy(R.resample_batch(flat, rows)).reshape(2, vt * vs, T, 3, 224, 224).permute(0, 1, 3, 2, 4, 5).contiguous()
        pixels = torch.from_numpy(src if vt > 1 else src[:, 0])
        loader.append(((pixels, torch.tensor(sizes, dtype=torch.int32)), data.y))
        ref_loader.append((host, data.y))
    if vs == 3:   # the three views of the 48 x 64 clip are three windows of 224 x 298
        assert [r[6:10] for r in rows[:3]] == [(224, 298, 0, 0), (224, 298, 0, 37), (224, 298, 0, 74)]
    m = _model(sd2, "compact", max_batch=2 * vt * vs * T, input_norm="imagenet")
    got = evaluate_video(loader, m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream, device_eval_crop=crop))
    ref = evaluate_video(ref_loader, m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream))
    assert got == ref, (got, ref)
    assert 0.0 <= got["metric"] <= 100.0 and 0.0 < got["keep_ratio"] <= 1.0
    # the class called on a device batch gives the restatement's clips
    _same_bits(crop(torch.from_numpy(flat).to(DEV), [s for s in sizes for _ in range(vt)]).permute(0, 2, 1, 3, 4), R.resample_batch(flat, rows),
               "DeviceClipUniformCrop.__call__")
    del m


def test_cross_type_refusals_raise_their_texts_and_plain_clips_change_nothing(sd2, data, monkeypatch):
    from _lib import DyTError
    from engine_finetune import evaluate, evaluate_video
    from util.crop import DeviceClipScaleJitterCrop, DeviceClipUniformCrop, DeviceRandomResizedCrop, DeviceResizeCenterCrop
    monkeypatch.setenv("DYT_PREFETCH", "0")
    clips = torch.from_numpy(data.src["small"])
    x = _float_clips(data.src["small"], SMALL[6:8])
    m = _model(sd2, "compact", input_norm="imagenet")
    sa, fa = _train(m, [(x, data.y)], device_crop=None, device_eval_crop=None)
    assert np.isfinite(sa["loss"]) and getattr(m._engine, "_rc_dev", None) is None
    with pytest.raises(DyTError, match="video clips are not implemented"):
        _train(m, [(clips, data.y)], device_crop=DeviceRandomResizedCrop())
    with pytest.raises(DyTError, match="DeviceClipScaleJitterCrop"):
        _train(m, [(clips, data.y)], device_crop=DeviceClipUniformCrop())
    with pytest.raises(DyTError, match="image batches go through"):
        _train(m, [(clips[:, 0], data.y)], device_crop=DeviceClipScaleJitterCrop())
    ev = types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=False)
    with pytest.raises(DyTError, match="video clips are not implemented"):
        evaluate_video([(clips, data.y)], m, DEV, args=types.SimpleNamespace(device_eval_crop=DeviceResizeCenterCrop(), **vars(ev)))
    with pytest.raises(DyTError, match="crops video clips"):
        evaluate([(clips[:, 0], data.y)], m, DEV, args=types.SimpleNamespace(device_eval_crop=DeviceClipUniformCrop(), **vars(ev)))
    plain = _model(sd2, "compact")
    with pytest.raises(DyTError, match="input_norm"):
        _train(plain, [(clips, data.y)], device_crop=DeviceClipScaleJitterCrop())
    del m, plain
