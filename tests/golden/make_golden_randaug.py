#!/usr/bin/env python3
"""Generate tests/golden/randaug/randaug.npz: the draws and the pixels of the reference's RandAugment (video_datasets/rand_augment.py).

Build container only (reads /root/reference; the arrays it writes are data and are what travels).  The reference's file is loaded BY FILE
PATH; it needs numpy and Pillow only.  Executed from the reference, its OWN code: ``rand_augment_transform``, ``RandAugment.__call__``,
``AugmentOp.__call__``, every level function and every op function of ``NAME_TO_OP``.  Nothing of it is restated here; the rows that
describe a case to the tests (operation number, arguments, coefficients) are built with tests/randaug_refs.py's ``row`` / ``rotate_coeffs``.
``pillow`` = the Pillow version that computed the pixels.

(a) Draws.  ``sizes`` [12, 2] = (h, w) in loader order, ``names`` / ``names_plain`` = the increasing / plain transform lists.  For each of two
    seeds (random.seed(seed), np.random.seed(seed)) one ``rand_augment_transform('rand-m7-n4-mstd0.5-inc1', {translate_const, interpolation:
    BICUBIC})`` per clip, as the reference's dataset builds it, called on a one-frame list; the ops of the transform are wrapped by recorders:
    ``draw<seed>_op`` [12, 4] = the chosen op (index into ``names``), ``draw<seed>_applied`` [12, 4], ``draw<seed>_arg`` [12, 4] = the level
    argument the op function received (NaN: none), ``draw<seed>_filter`` [12, 4] = its resample (0: skipped), ``draw<seed>_next`` = the next
    random.random() and np.random.uniform() -- they pin the number consumed.  ``inc0_*``: the same for one 'rand-m9-n2-inc0' run (seed 3),
    with ``inc0_names`` = the names its ops carry: the parser's ``bool('0')`` selects the increasing set, and there is no gauss draw.
(b) Pixels.  ``px_src`` uint8 [3, 2, 64, 64, 3] (two-frame sources of 48 x 64, 64 x 40 and 33 x 57, padded with 0xFF; a smooth ramp, a
    checkerboard, one constant channel, one narrow channel), ``px_sizes`` [3, 2].  Cases: ``case_name`` = the reference op run, ``case_src``,
    ``case_row_*`` = the device row (op, iarg, factor, coeffs[6], filter) and ``case_out`` uint8 [cases, 2, 64, 64, 3] = the reference's
    output inside the valid extent, 0xFF outside.  ``tab_case`` / ``tab_hist`` int32 [k, 2, 4, 256] / ``tab_lut`` int16 [k, 2, 3, 256]: for the
    AutoContrast and Equalize cases the R, G, B, L histograms of each source frame and the table OBSERVED from the reference's output (-1: the
    value does not occur in the frame); ``con_case`` / ``con_hist`` [k, 2, 256] / ``con_mean`` [k, 2]: the L histogram and Pillow's
    ``int(ImageStat.Stat(L).mean[0] + 0.5)`` for the Contrast cases.  ``chain_*``: the unit of draw (a), seed 0, with the most applied ops,
    replayed through the reference's op functions on source 2.

tests/test_randaug_refs_host.py pins tests/randaug_refs.py to the pixels, tests/test_randaug_draw_host.py pins util.randaug to the draws.
Usage:  python tests/golden/make_golden_randaug.py
"""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference's root)

sys.path.insert(0, os.path.dirname(HERE))
import randaug_refs as R  # noqa: E402

REF_FILE = os.path.join(mg.REF, "video_datasets", "rand_augment.py")
SEEDS = (0, 1234)
SIZES = [(240, 320), (256, 340), (320, 240), (224, 224), (480, 640), (128, 171), (360, 360), (225, 400),
         (32, 512), (512, 32), (96, 64), (300, 400)]   # the SIZES of make_golden_clip_resample.py
CONFIG, CONFIG_INC0 = "rand-m7-n4-mstd0.5-inc1", "rand-m9-n2-inc0"
FILL = (128, 128, 128)


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_rand_augment", REF_FILE)
    ra = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ra)
    assert os.path.realpath(ra.__file__).startswith(mg.REF)
    return ra


class Recorder:
    """Stands for one AugmentOp of a transform: notes that it was chosen, and with what its op function was called (which it does not run)."""

    def __init__(self, ra, op, log):
        self.op, self.log = op, log
        self.name = next(n for n, f in ra.NAME_TO_OP.items() if f is op.aug_fn and ra.LEVEL_TO_ARG[n] is op.level_fn)
        op.aug_fn = self.called

    def called(self, img, *args, **kwargs):
        self.log[-1] = (self.name, True, args[0] if args else float("nan"), kwargs["resample"])
        return img

    def __call__(self, imgs):
        self.log.append((self.name, False, float("nan"), 0))
        return self.op(imgs)


def recorded_draws(ra, config, seed, names):
    from PIL import Image
    random.seed(seed)
    np.random.seed(seed)
    ops, applied, args, filt, seen = [], [], [], [], set()
    for (h, w) in SIZES:
        tfm = ra.rand_augment_transform(config, {"translate_const": int(min(h, w) * 0.45), "interpolation": Image.BICUBIC})
        log = []
        tfm.ops = [Recorder(ra, op, log) for op in tfm.ops]
        seen.update(r.name for r in tfm.ops)
        tfm([Image.new("RGB", (w, h))])
        assert len(log) == tfm.num_layers
        ops.append([names.index(e[0]) for e in log])
        applied.append([int(e[1]) for e in log])
        args.append([float(e[2]) for e in log])
        filt.append([int(e[3]) for e in log])
    nxt = np.array([random.random(), np.random.uniform()], dtype=np.float64)
    return (np.array(ops, dtype=np.int32), np.array(applied, dtype=np.int32), np.array(args, dtype=np.float64), np.array(filt, dtype=np.int32), nxt,
            sorted(seen, key=names.index))


def run_op(ra, name, arg, filt, frames):
    """The reference's op function ``name`` on uint8 frames [T, h, w, 3], through AugmentOp's own kwargs"""
    from PIL import Image
    imgs = [Image.fromarray(np.ascontiguousarray(f)) for f in frames]
    fn = ra.NAME_TO_OP[name]
    args = () if arg is None else (arg,)
    out = [fn(img, *args, **{"fillcolor": FILL, "resample": filt}) for img in imgs]
    return np.stack([np.asarray(o) for o in out])


def device_row(name, arg, filt, h, w):
    """The device row of a case (tests/randaug_refs.py's layout)"""
    if name == "Invert":
        return R.row(R.INVERT)
    if name == "AutoContrast":
        return R.row(R.AUTO_CONTRAST)
    if name == "Equalize":
        return R.row(R.EQUALIZE)
    if name.startswith("Posterize"):
        return R.row(R.POSTERIZE, arg)
    if name == "SolarizeAdd":
        return R.row(R.SOLARIZE_ADD, arg)
    if name.startswith("Solarize"):
        return R.row(R.SOLARIZE, arg)
    for k, op in (("Brightness", R.BRIGHTNESS), ("Color", R.COLOR), ("Contrast", R.CONTRAST), ("Sharpness", R.SHARPNESS)):
        if name.startswith(k):
            return R.row(op, 0, arg)
    if name == "Rotate":
        c = R.rotate_coeffs(arg, h, w)
        return R.row(R.IDENTITY) if c is None else R.row(R.AFFINE, coeffs=c, filt=filt)
    c = {"ShearX": (1, arg, 0, 0, 1, 0), "ShearY": (1, 0, 0, arg, 1, 0), "TranslateXRel": (1, 0, arg * w, 0, 1, 0),
         "TranslateYRel": (1, 0, 0, 0, 1, arg * h), "TranslateX": (1, 0, arg, 0, 1, 0), "TranslateY": (1, 0, 0, 0, 1, arg)}[name]
    return R.row(R.AFFINE, coeffs=c, filt=filt)


def observed_table(src, out):
    """int16 [3, 256]: the value every source value of a channel became (-1: absent); a table operation maps equal values equally"""
    t = np.full((3, 256), -1, dtype=np.int16)
    for c in range(3):
        s, o = src[..., c].ravel(), out[..., c].ravel()
        for v in np.unique(s):
            got = np.unique(o[s == v])
            assert len(got) == 1
            t[c, v] = got[0]
    return t


def main():
    import PIL
    from PIL import ImageStat, Image
    ra = load_reference()
    names, plain = list(ra._RAND_INCREASING_TRANSFORMS), list(ra._RAND_TRANSFORMS)
    out = {"sizes": np.array(SIZES, dtype=np.int32), "names": np.array(names), "names_plain": np.array(plain), "pillow": np.array(PIL.__version__),
           "config": np.array(CONFIG), "config_inc0": np.array(CONFIG_INC0)}
    draws = {}
    for seed in SEEDS:
        ops, applied, args, filt, nxt, seen = recorded_draws(ra, CONFIG, seed, names)
        draws[seed] = (ops, applied, args)
        for k, v in (("op", ops), ("applied", applied), ("arg", args), ("filter", filt), ("next", nxt)):
            out["draw%d_%s" % (seed, k)] = v
        assert seen == names
        print("seed %d: %d of %d ops applied, first clip %s" % (seed, int(applied.sum()), applied.size, [names[i] for i in ops[0]]))
    ops, applied, args, filt, nxt, seen = recorded_draws(ra, CONFIG_INC0, 3, names)
    for k, v in (("op", ops), ("applied", applied), ("arg", args), ("filter", filt), ("next", nxt), ("names", np.array(seen))):
        out["inc0_" + k] = v
    assert seen == names and ops.shape == (12, 2)

    # (b) pixels
    rng = np.random.default_rng(23)
    shapes = [(48, 64), (64, 40), (33, 57)]
    src = np.full((3, 2, 64, 64, 3), 0xFF, dtype=np.uint8)
    for i, (h, w) in enumerate(shapes):
        src[i, :, :h, :w] = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    src[0, 1, :48, :64] = (np.add.outer(np.arange(48) * 3, np.arange(64) * 2)[..., None] + np.array([0, 40, 90])).astype(np.uint8)   # a smooth ramp
    src[1, 0, :64, :40] = ((np.add.outer(np.arange(64), np.arange(40)) & 1) * 255).astype(np.uint8)[..., None]                       # a checkerboard
    src[1, 1, :64, :40, 2] = 77                                                                                                     # a constant channel
    src[2, :, :33, :57, 1] = rng.integers(60, 181, (2, 33, 57), dtype=np.uint8)                                                      # a narrow channel
    BL, BC = Image.BILINEAR, Image.BICUBIC
    cases = [("Invert", None, BC, 0), ("Invert", None, BC, 1),
             ("Solarize", 100, BC, 0), ("Solarize", 256, BC, 2), ("SolarizeAdd", 60, BC, 1), ("SolarizeAdd", 110, BC, 2),
             ("Posterize", 0, BC, 0), ("Posterize", 3, BC, 2), ("Posterize", 8, BC, 1),
             ("AutoContrast", None, BC, 2), ("AutoContrast", None, BC, 1), ("Equalize", None, BC, 0), ("Equalize", None, BC, 1),
             ("Brightness", 0.37, BC, 0), ("Brightness", 1.63, BC, 1), ("Color", 0.1, BC, 2), ("Color", 1.9, BC, 0),
             ("Contrast", 0.37, BC, 1), ("Contrast", 1.63, BC, 2), ("Sharpness", 0.1, BC, 0), ("Sharpness", 1.9, BC, 1),
             ("ShearX", 0.21, BC, 2), ("ShearX", -0.3, BL, 0), ("ShearY", 0.21, BL, 1), ("ShearY", -0.3, BC, 2),
             ("TranslateXRel", 0.3, BC, 0), ("TranslateXRel", -0.2, BL, 1), ("TranslateYRel", -0.45, BC, 2), ("TranslateYRel", 0.2, BL, 0),
             ("TranslateXRel", 0.9, BC, 1),                                         # most of the frame moves out
             ("Rotate", 21.0, BC, 2), ("Rotate", -13.7, BC, 0), ("Rotate", 30.0, BL, 1), ("Rotate", -7.5, BL, 2), ("Rotate", 0.0, BC, 0)]
    rows, outs, tab, con = [], [], [], []
    for k, (name, arg, filt, i) in enumerate(cases):
        h, w = shapes[i]
        got = run_op(ra, name, arg, filt, src[i, :, :h, :w])
        full = np.full((2, 64, 64, 3), 0xFF, dtype=np.uint8)
        full[:, :h, :w] = got
        outs.append(full)
        rows.append(device_row(name, arg, filt, h, w))
        if name in ("AutoContrast", "Equalize"):
            tab.append((k, np.stack([R.histograms(src[i, f, :h, :w]) for f in range(2)]), np.stack([observed_table(src[i, f, :h, :w], got[f]) for f in range(2)])))
        if name == "Contrast":
            ls = [Image.fromarray(np.ascontiguousarray(src[i, f, :h, :w])).convert("L") for f in range(2)]
            con.append((k, np.stack([np.array(im.histogram()) for im in ls]), [int(ImageStat.Stat(im).mean[0] + 0.5) for im in ls]))
    out["px_src"], out["px_sizes"] = src, np.array(shapes, dtype=np.int32)
    out["case_name"], out["case_src"] = np.array([c[0] for c in cases]), np.array([c[3] for c in cases], dtype=np.int32)
    out["case_row_op"] = np.array([r[0] for r in rows], dtype=np.int32)
    out["case_row_iarg"] = np.array([r[1] for r in rows], dtype=np.int32)
    out["case_row_factor"] = np.array([r[2] for r in rows], dtype=np.float64)
    out["case_row_coeffs"] = np.array([r[3] for r in rows], dtype=np.float64)
    out["case_row_filter"] = np.array([r[4] for r in rows], dtype=np.int32)
    out["case_out"] = np.stack(outs)
    out["tab_case"] = np.array([t[0] for t in tab], dtype=np.int32)
    out["tab_hist"] = np.stack([t[1] for t in tab]).astype(np.int32)
    out["tab_lut"] = np.stack([t[2] for t in tab])
    out["con_case"] = np.array([c[0] for c in con], dtype=np.int32)
    out["con_hist"] = np.stack([c[1] for c in con]).astype(np.int32)
    out["con_mean"] = np.array([c[2] for c in con], dtype=np.int32)
    assert sorted(set(out["case_row_op"].tolist())) == list(range(12))

    # the chain: the unit of draw (a), seed 0, with the most applied ops, on source 2
    ops, applied, args = draws[SEEDS[0]]
    u = int(np.argmax(applied.sum(axis=1)))
    h, w = shapes[2]
    frames = src[2, :, :h, :w]
    crow = []
    for layer in range(ops.shape[1]):
        name = names[ops[u, layer]]
        if not applied[u, layer]:
            crow.append(R.row(R.IDENTITY))
            continue
        a = args[u, layer]
        arg = None if np.isnan(a) else (int(a) if name.startswith(("Posterize", "Solarize")) else float(a))   # the integer level arguments
        frames = run_op(ra, name, arg, BC, frames)
        crow.append(device_row(name, arg, BC, h, w))
    full = np.full((2, 64, 64, 3), 0xFF, dtype=np.uint8)
    full[:, :h, :w] = frames
    out["chain_unit"], out["chain_out"] = np.array(u, dtype=np.int32), full
    out["chain_row_op"] = np.array([r[0] for r in crow], dtype=np.int32)
    out["chain_row_iarg"] = np.array([r[1] for r in crow], dtype=np.int32)
    out["chain_row_factor"] = np.array([r[2] for r in crow], dtype=np.float64)
    out["chain_row_coeffs"] = np.array([r[3] for r in crow], dtype=np.float64)
    out["chain_row_filter"] = np.array([r[4] for r in crow], dtype=np.int32)
    print("chain: unit %d of seed %d: %s applied %s" % (u, SEEDS[0], [names[i] for i in ops[u]], applied[u].tolist()))
    os.makedirs(os.path.join(HERE, "randaug"), exist_ok=True)
    path = os.path.join(HERE, "randaug", "randaug.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes), Pillow %s" % (path, os.path.getsize(path), PIL.__version__))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
