"""GPU tests of the device crop / resize at any downscale (pytest -m gpu): dyt_resample_wide_coeffs and dyt_resample_wide_u8 against
tests/resample_wide_refs.py -- the numpy restatement of Pillow's 8-bit bicubic resize without a tap bound, which
tests/test_resample_wide_host.py pins to Pillow --, against Pillow's recorded bytes (tests/golden/resample/resample_wide.npz) and against
dyt_resample_u8 on the rows that entry takes; ``any_scale=True`` and ``DeviceResize`` through train_one_epoch and evaluate.

Everything is integer arithmetic on both sides, so every comparison is exact: integer for integer on the coefficient tables, byte for byte
on the images, bit for bit on losses and trainable parameters.  The sources are strips of 8 x 4096 and 4096 x 8 (74 taps on one axis),
700 x 700, and one padded shape of 1200 x 1300 (the only large one); B <= 4; r = 8, C = 10, training loops of depth 2."""
import os
import struct
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gpu_diag as D  # noqa: E402
import resample_refs as R  # noqa: E402
import resample_wide_refs as W  # noqa: E402
import synth  # noqa: E402

C, RANK, SEED, BMAX = 10, 8, 131, 4
DEV = torch.device("cuda", 0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample", "resample_wide.npz")
T = (224, 224, 0, 0)   # a train row's full size and window

# name -> (padded shape, the row both images of the batch share, checkerboard period): image 0 is noise, image 1 a saturated 0 / 255
# checkerboard whose squares are a few output pixels wide, so that the filter's overshoot reaches both clamps
CASES = {
    "strip across": ((8, 4096), (8, 4096, 0, 0, 8, 4096) + T + (0,), 64),                    # 74 taps across, an upscale down
    "strip down": ((4096, 8), (4096, 8, 0, 0, 4096, 8) + T + (0,), 64),                      # 74 taps down, an upscale across
    "centre window": ((700, 700), (700, 700, 0, 0, 700, 700, 256, 256, 16, 16, 0), 5),       # the needed rows start below the top
    "odd box": ((1200, 1300), (1200, 1300, 77, 33, 1100, 561) + T + (0,), 8),                # the segment starts off any 16-byte boundary
}


def _mirrored(rows):
    return [r[:10] + (r[10] ^ 1,) for r in rows]


def _draw(rows):
    from util.crop import CropDraw
    return CropDraw(rows, wide=True)


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


def _resample(src, rows, **kw):
    from _lib import resample_wide_u8
    out = resample_wide_u8(torch.from_numpy(np.ascontiguousarray(src)).to(DEV), _table(rows), _draw(rows), **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def data():
    """The four two-image batches and the restatement's bytes for their rows: computed once, read only."""
    rng = np.random.default_rng(SEED)
    d = types.SimpleNamespace(src={}, rows={}, want={})
    for name, ((h, w), row, period) in CASES.items():
        d.src[name] = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), W.checkerboard(h, w, period)])
        d.rows[name] = [row, row]
        d.want[name] = W.resample_batch(d.src[name], d.rows[name])
    d.y = torch.tensor([3, 7, 7, 0], dtype=torch.int64)
    return d


# ---- 4. coefficient tables -----------------------------------------------------------------------------------------------------------------
def test_coefficient_tables_equal_the_restatement_integer_for_integer():
    from _lib import resample_wide_coeffs
    rows = [(4096, 4096, 0, 0, 4096, 561) + T + (0,),                     # 4096 / 224 down, 561 / 224 across
            (4096, 4096, 3, 5, 560, 32) + T + (1,),                       # 560 / 224 (the 11-tap bound) and 32 / 224 (an upscale)
            (700, 700, 0, 0, 700, 700, 256, 256, 16, 16, 0),              # 700 / 256 with a window offset
            (1200, 1300, 77, 33, 1100, 561) + T + (0,)]
    tab = _table(rows)
    widest = 0
    for i, row in enumerate(rows):
        got = resample_wide_coeffs(tab, i, 4096, 4096).cpu().numpy()
        want = W.coeff_table(row)
        assert got.shape == want.shape == (2, 77, 224) and got.dtype == np.int32
        bad = got != want
        assert not bad.any(), "row %d %r: %d integers differ, first at %s" % (i, row, int(bad.sum()), np.argwhere(bad)[0].tolist())
        widest = max(widest, int(got[:, 1].max()))
    assert widest == 74
    narrow = R.coeff_table(rows[1])                                       # where the 11-tap restatement applies, its integers
    assert np.array_equal(W.coeff_table(rows[1])[:, :13], narrow) and int(narrow[0, 1].max()) == 10
    # a row the batch's shape refuses gives zeros
    assert not resample_wide_coeffs(tab, 3, 1199, 1300).cpu().numpy().any()


# ---- 5. output bytes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_output_bytes_equal_the_restatement_with_and_without_the_mirror(data, name):
    rows, want = data.rows[name], data.want[name]
    assert want[1].min() == 0 and want[1].max() == 255                   # the checkerboard clamps at both ends
    _same_bytes(_resample(data.src[name], rows), want, name)
    _same_bytes(_resample(data.src[name], _mirrored(rows)), want[:, :, ::-1], name + ", mirrored")
    mixed = [rows[0], _mirrored(rows)[1]]
    _same_bytes(_resample(data.src[name], mixed), np.stack([want[0], want[1][:, ::-1]]), name + ", the second image mirrored")


def test_a_source_that_ends_off_a_16_byte_run_is_staged_byte_by_byte_at_its_end():
    """One image of 5 x 7 pixels is 105 bytes: the last box row's segment ends at the allocation's last byte, so its second 16-byte run
    crosses the end and is filled byte by byte (every other source here is a whole number of runs)."""
    src = np.random.default_rng(SEED + 5).integers(0, 256, (1, 5, 7, 3), dtype=np.uint8)
    rows = [(5, 7, 0, 0, 5, 7) + T + (0,)]
    assert src.nbytes == 105 and src.nbytes % 16 != 0 and (4 * 7 * 3) // 16 * 16 + 32 > src.nbytes
    want = W.resample_batch(src, rows)
    _same_bytes(_resample(src, rows), want, "5 x 7")
    _same_bytes(_resample(src, _mirrored(rows)), want[:, :, ::-1], "5 x 7, mirrored")


def test_the_strips_take_74_taps_and_the_window_skips_rows():
    lo, cnt, _ = W.coeffs(4096, 224, np.arange(224))
    assert int(cnt.max()) == 74
    lo, cnt, _ = W.coeffs(700, 256, 16 + np.arange(224))
    assert int(lo.min()) > 30 and int((lo + cnt).max()) < 670            # rows at the top and the bottom reach no output
    assert CASES["odd box"][1][2] % 2 == 1 and (CASES["odd box"][1][3] * 3) % 16 != 0


# ---- 6. wide equals narrow -----------------------------------------------------------------------------------------------------------------
def test_the_wide_entry_writes_the_narrow_entrys_bits_on_the_rows_that_one_takes():
    from _lib import resample_u8
    from util.crop import CropDraw
    rows = [(300, 400, 0, 0, 300, 400, 256, 341, 16, 58, 0),             # 300 x 400 to 256: the 11-tap evaluation row
            (560, 576, 301, 417, 21, 40) + T + (1,),                     # a small mirrored box
            (560, 576, 0, 7, 560, 560) + T + (0,)]                       # a 560-side box: the 11-tap bound itself
    rng = np.random.default_rng(SEED + 1)
    src = np.zeros((3, 560, 576, 3), dtype=np.uint8)
    src[0, :300, :400] = rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)
    src[1] = rng.integers(0, 256, (560, 576, 3), dtype=np.uint8)
    src[2] = W.checkerboard(560, 576, 2)
    dev = torch.from_numpy(src).to(DEV)
    narrow = resample_u8(dev, _table(rows), CropDraw(rows))
    torch.cuda.synchronize()
    _same_bytes(_resample(src, rows), narrow, "wide against narrow")
    _same_bytes(narrow[1], R.resample_image(src[1], rows[1]), "the narrow entry's small box")      # and both are the restatement's
    _same_bytes(narrow[0], W.resample_image(src[0], rows[0]), "the evaluation row")


# ---- 7. a mixed batch ----------------------------------------------------------------------------------------------------------------------
def test_a_mixed_batch_with_an_invalid_row_never_reads_its_padding():
    from _lib import resample_wide_u8
    hs, ws = 1200, 1300
    rows = [(1200, 1300, 0, 0, 1200, 1300) + T + (1,),                   # wide: scales 5.4 and 5.8, mirrored
            (300, 400, 10, 20, 250, 333, 256, 341, 16, 58, 0),           # narrow-sized, valid extent far inside the padded shape
            (32, 32, 0, 0, 32, 32) + T + (0,),                           # an upscale
            (700, 900, 0, 0, 700, 900) + T + (0,)]                       # made invalid below
    rng = np.random.default_rng(SEED + 2)
    ff = np.full((4, hs, ws, 3), 0xFF, dtype=np.uint8)
    for i, r in enumerate(rows):
        ff[i, :r[0], :r[1]] = rng.integers(0, 256, (r[0], r[1], 3), dtype=np.uint8)
    zero = ff.copy()
    for i, r in enumerate(rows):
        zero[i, r[0]:] = 0
        zero[i, :, r[1]:] = 0
    want = W.resample_batch(zero, rows)
    outs = []
    for src in (torch.from_numpy(ff).to(DEV), torch.from_numpy(zero).to(DEV)):
        for bad in ((700, 900, 0, 0, 701, 900) + T + (0,), (1201, 1300, 0, 0, 1201, 1300) + T + (0,), (2 ** 31 - 1,) * 11):
            words = bytearray(_draw(rows).words())
            words[64 + 48 * 3:64 + 48 * 3 + 44] = struct.pack("<11i", *bad)
            out = torch.full((4, 224, 224, 3), 0xAA, dtype=torch.uint8, device=DEV)
            resample_wide_u8(src, torch.frombuffer(words, dtype=torch.int32).to(DEV), None, out=out)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert not got[3].any(), bad                                  # the invalid image is zeros
            _same_bytes(got[:3], want[:3], "the valid rows beside %r" % (bad,))
        outs.append(resample_wide_u8(src, _table(rows), _draw(rows)).cpu())
    _same_bytes(outs[0], want, "padding 0xFF")
    _same_bytes(outs[1], want, "padding 0x00")
    # fewer units than images, another filter word: zeros
    for units, filt, zeros in ((2, 3, [2, 3]), (4, 2, [0, 1, 2, 3])):
        words = bytearray(_draw(rows).words())
        words[0:8] = struct.pack("<2i", filt, units)
        out = torch.full((4, 224, 224, 3), 0xAA, dtype=torch.uint8, device=DEV)
        resample_wide_u8(src, torch.frombuffer(words, dtype=torch.int32).to(DEV), None, out=out)      # the batch padded with zeros
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for i in range(4):
            if i in zeros:
                assert not got[i].any(), (units, filt, i)
            else:
                _same_bytes(got[i], want[i], "units %d filter %d image %d" % (units, filt, i))


def test_the_python_layer_refuses_before_upload():
    from _lib import DyTError, resample_wide_u8
    from util.crop import CropDraw
    src = torch.zeros(2, 64, 64, 3, dtype=torch.uint8, device=DEV)
    rows = [(64, 64, 0, 0, 64, 64) + T + (0,)] * 2
    tab = _table(rows)
    with pytest.raises(DyTError, match="valid extent"):
        resample_wide_u8(src, tab, CropDraw([(65, 64, 0, 0, 10, 10) + T + (0,)] * 2, wide=True))
    with pytest.raises(DyTError, match="holds 1 images"):
        resample_wide_u8(src, tab, CropDraw(rows[:1], wide=True))
    with pytest.raises(DyTError, match="too small"):
        resample_wide_u8(src, tab, None, scratch=torch.zeros(2 * 23296 // 4, dtype=torch.int32, device=DEV))      # the 11-tap route's scratch
    for x in (src.permute(0, 3, 1, 2).contiguous(), src.float(), src.cpu(), src[None]):
        with pytest.raises(DyTError):
            resample_wide_u8(x, tab)


# ---- 8. the golden file --------------------------------------------------------------------------------------------------------------------
def test_the_golden_sources_give_pillows_recorded_bytes():
    g = np.load(GOLDEN)
    for case in ("wide", "tall", "eval", "noaug", "box"):
        h, w = (int(v) for v in g[case + "_size"])
        row = tuple(int(v) for v in g[case + "_row"])
        _same_bytes(_resample(W.pattern(h, w)[None], [row]), g[case + "_out"][None], "golden case %s" % case)


# ---- 9. the loops --------------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def big():
    """Two batches of 4 sources of 700 x 900 (the second padded to 704 x 912 around smaller images) and their sizes."""
    rng = np.random.default_rng(SEED + 3)
    a = rng.integers(0, 256, (4, 700, 900, 3), dtype=np.uint8)
    sizes_b = [(700, 900), (650, 912), (704, 600), (300, 400)]
    b = np.zeros((4, 704, 912, 3), dtype=np.uint8)
    for i, (h, w) in enumerate(sizes_b):
        b[i, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return types.SimpleNamespace(src=[a, b], sizes=[[(700, 900)] * 4, sizes_b], y=torch.tensor([3, 7, 7, 0], dtype=torch.int64))


def _criterion():
    from models.losses import AdaLoss
    return AdaLoss(torch.nn.CrossEntropyLoss(), token_target_ratio=0.5, token_loss_ratio=2.0, token_minimal=0.1, token_minimal_weight=1.0)


def _train(model, loader, graph=False, lr=1e-3, **extra):
    from engine_finetune import FusedAdamW, train_one_epoch
    opt = FusedAdamW(model, lr=lr, weight_decay=0.01)
    args = types.SimpleNamespace(accum_iter=1, lr=lr, min_lr=0.0, warmup_epochs=0, epochs=10, metric="accuracy", nb_classes=C, hip_graph=graph, **extra)
    stats = train_one_epoch(model, _criterion(), loader, opt, DEV, 0, None, 0, None, None, args=args)
    torch.cuda.synchronize()
    return stats, model._engine.flat.clone()


def _record_entries(monkeypatch):
    """The resample entries the engine calls, in order."""
    import _lib
    calls = []
    for name in ("resample_u8", "resample_wide_u8"):
        def wrap(*a, _f=getattr(_lib, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(_lib, name, wrap)
    return calls


def test_two_steps_of_the_loop_equal_the_loop_fed_the_restatements_bytes(sd2, big, monkeypatch):
    """train_one_epoch with args.device_crop = DeviceRandomResizedCrop(any_scale=True) drawing from a seeded generator -- a (pixels, sizes)
    batch, then a bare uint8 batch that every image fills --, eager and from a captured graph, against the same loop fed the 224 x 224 byte
    batches tests/resample_wide_refs.py makes of the same draws."""
    from util.crop import DeviceRandomResizedCrop
    monkeypatch.setenv("DYT_PREFETCH", "0")
    host = DeviceRandomResizedCrop(any_scale=True, generator=torch.Generator().manual_seed(SEED))
    draws = [host.draw_for(big.sizes[1]), host.draw_for(big.sizes[0])]
    assert all(d.wide for d in draws) and max(max(r[4], r[5]) for d in draws for r in d.rows) > 560      # beyond the 11-tap route
    assert any(r[10] for d in draws for r in d.rows)
    want = [torch.from_numpy(W.resample_batch(big.src[1], draws[0].rows)), torch.from_numpy(W.resample_batch(big.src[0], draws[1].rows))]
    crop_loader = [((torch.from_numpy(big.src[1]), torch.tensor(big.sizes[1], dtype=torch.int32)), big.y),
                   (torch.from_numpy(big.src[0]), big.y.flip(0).contiguous())]
    plain_loader = [(want[0], big.y), (want[1], big.y.flip(0).contiguous())]
    calls = _record_entries(monkeypatch)
    out = {}
    for what in ("bytes", "crop eager", "crop graph"):
        m = _model(sd2, "compact", input_norm="imagenet")
        del calls[:]
        if what == "bytes":
            out[what] = _train(m, plain_loader)
            assert not calls and not hasattr(m._engine, "_rs_dev") and not hasattr(m._engine, "_rsw_scratch")      # no resample launch
        else:
            cropper = DeviceRandomResizedCrop(any_scale=True, generator=torch.Generator().manual_seed(SEED))
            out[what] = _train(m, crop_loader, graph=what.endswith("graph"), device_crop=cropper)
            assert calls and set(calls) == {"resample_wide_u8"}, calls                                             # the probe included
            assert len(m._engine._graphs) == (1 if what.endswith("graph") else 0)
        del m
    for what in ("crop eager", "crop graph"):
        assert out[what][0] == out["bytes"][0], (what, out[what][0], out["bytes"][0])
        _same_bits(out[what][1], out["bytes"][1], "%s: trainable parameters" % what)
    assert np.isfinite(out["bytes"][0]["loss"])


@pytest.mark.parametrize("stream", [False, True])
def test_evaluate_with_any_scale_and_device_resize_equals_evaluate_on_the_restatements_bytes(stream, sd2, big):
    from engine_finetune import evaluate
    from util.crop import DeviceResize, DeviceResizeCenterCrop
    m = _model(sd2, "compact", input_norm="imagenet")
    small_sizes = [[(300, 400), (32, 32), (400, 300), (64, 48)], [(200, 200)] * 4]
    rng = np.random.default_rng(SEED + 4)
    small = [np.zeros((4, 400, 400, 3), dtype=np.uint8), rng.integers(0, 256, (4, 200, 200, 3), dtype=np.uint8)]
    for i, (h, w) in enumerate(small_sizes[0]):
        small[0][i, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for crop, srcs, sizes in ((DeviceResizeCenterCrop(any_scale=True), big.src, big.sizes), (DeviceResize(any_scale=True), big.src, big.sizes),
                              (DeviceResize(), small, small_sizes)):
        rows = [crop.draw_for(s).rows for s in sizes]
        want = [torch.from_numpy(W.resample_batch(srcs[i], rows[i])) for i in range(2)]
        loader = [((torch.from_numpy(srcs[i]), torch.tensor(sizes[i], dtype=torch.int32)), big.y) for i in range(2)]
        got = evaluate(loader, m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream, device_eval_crop=crop))
        ref = evaluate([(want[i], big.y) for i in range(2)], m, DEV, args=types.SimpleNamespace(metric="accuracy", nb_classes=C, stream_eval=stream))
        assert got == ref, (type(crop).__name__, got, ref)
        assert 0.0 <= got["metric"] <= 100.0 and 0.0 < got["keep_ratio"] <= 1.0
        _same_bytes(crop(torch.from_numpy(srcs[1]).to(DEV), sizes[1]), want[1], "%s.__call__" % type(crop).__name__)
    assert rows[0][1] == (32, 32, 0, 0, 32, 32, 224, 224, 0, 0, 0)
    del m


def test_a_wide_draw_always_takes_the_wide_entry_and_a_narrow_draw_todays_calls(sd2, big, monkeypatch):
    """DyTEngine.resample: the route is the draw's flag, never its rows; the wide scratch is allocated on first use, grows and never shrinks;
    without any_scale the entries called and the bytes written are the 11-tap route's."""
    from util.crop import CropDraw, DeviceResizeCenterCrop
    calls = _record_entries(monkeypatch)
    m = _model(sd2, "compact", input_norm="imagenet")
    eng = m.engine(4, DEV)
    rng = np.random.default_rng(SEED + 5)
    src = torch.from_numpy(rng.integers(0, 256, (4, 300, 400, 3), dtype=np.uint8)).to(DEV)
    sizes = [(300, 400)] * 4
    narrow_draw = DeviceResizeCenterCrop().draw_for(sizes)
    a = eng.resample(src, sizes, narrow_draw).clone()
    assert calls == ["resample_u8"] and not hasattr(eng, "_rsw_scratch")
    wide_draw = DeviceResizeCenterCrop(any_scale=True).draw_for(sizes)
    assert wide_draw.rows == narrow_draw.rows and wide_draw.wide and not narrow_draw.wide
    b = eng.resample(src, sizes, wide_draw).clone()
    assert calls == ["resample_u8", "resample_wide_u8"]                 # every row would fit the 11-tap entry: the wide one all the same
    _same_bytes(a, b, "the two routes on rows both take")
    _same_bytes(a, R.resample_batch(src.cpu().numpy(), narrow_draw.rows), "the 11-tap route's bytes")
    first = eng._rsw_scratch
    assert first.numel() * 4 == eng.L.dyt_resample_wide_scratch_bytes(BMAX, 300)
    low = src[:2, :100].contiguous()
    eng.resample(low, [(100, 400)] * 2, CropDraw([(100, 400, 0, 0, 100, 400) + T + (0,)] * 2, wide=True))
    assert eng._rsw_scratch is first                                    # never shrinks
    tall = torch.from_numpy(big.src[0]).to(DEV)
    c = eng.resample(tall, big.sizes[0], CropDraw([(700, 900, 0, 100, 700, 700) + T + (0,)] * 4, wide=True)).clone()
    assert eng._rsw_scratch.numel() * 4 == eng.L.dyt_resample_wide_scratch_bytes(BMAX, 700) and eng._rsw_scratch is not first
    torch.cuda.synchronize()
    _same_bytes(c, W.resample_batch(big.src[0], [(700, 900, 0, 100, 700, 700) + T + (0,)] * 4), "a 700 x 700 box of a 700 x 900 source")
    from _lib import DyTError
    with pytest.raises(DyTError, match="more than 2.5 times"):          # a narrow draw keeps its refusal: the rows are checked as the draw says
        bad = CropDraw([(300, 400, 0, 0, 300, 400) + T + (0,)] * 4)
        bad.rows = [(700, 900, 0, 0, 700, 900) + T + (0,)] * 4
        eng.resample(tall, big.sizes[0], bad)
    del m
