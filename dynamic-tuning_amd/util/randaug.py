"""RandAugment on the device for byte clips and images: ``DeviceRandAugment`` stands where ``create_random_augment(...)`` /
``rand_augment_transform(config_str, hparams)`` of the reference's video_datasets/rand_augment.py stand in its SSV2 / K400 train pipeline
(sthv2_dataset.py:128-138), and where timm's RandAugment stands behind the crop and the flip of an image pipeline.  The loader decodes and
pads only (``util.crop.pad_collate_clips`` / ``pad_collate``); the operations are drawn on the host and the pixels are written on the device
(csrc/randaug.h, csrc/randaug.hip): Pillow's 8-bit arithmetic restated byte for byte.

The draws are a RESTATEMENT of ``RandAugment.__call__`` and ``AugmentOp.__call__``, per clip (or image) in this order:

    1. ``np.random.choice(ops, num_layers)`` (with replacement; ``np_rng.choice(len(ops), num_layers)`` makes the same generator call)
    2. for each chosen op in order: ``random.random() > prob`` skips it; ``random.gauss(magnitude, mstd)`` when ``mstd > 0``; the
       magnitude is clipped to [0, 10]; the op's level function, with one more ``random.random()`` where it negates at random

All frames of a clip share one draw.  With ``py_rng=None`` / ``np_rng=None`` they come from the ``random`` module and numpy's global
generator, as the reference's do, so a seeded run draws the reference's operations.  The 24 names of the reference's ``NAME_TO_OP`` map onto
12 device operations; Rotate's matrix is built here exactly as ``PIL.Image.rotate`` builds it, from each clip's own (h, w).

Two ways to use it:
  * ``train_one_epoch(..., args)`` / ``train_video_one_epoch`` with ``args.device_randaug = DeviceRandAugment.from_reference(...)``: the loop
    draws and the engine augments on the compute stream (``DyTEngine.randaug``), in front of the clip crop (video: RandAugment -> normalise
    -> crop, the reference's order) or behind the image crop (crop -> flip -> RandAugment, timm's order).
  * ``augmented = DeviceRandAugment(...)(pixels, sizes)`` on a device batch: new bytes of the same shape (libdyt_hip's dyt_randaug_u8).
"""
import math
import re
import struct

IDENTITY, INVERT, SOLARIZE, SOLARIZE_ADD, POSTERIZE, AUTO_CONTRAST, EQUALIZE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, AFFINE = range(12)
OP_NAMES = ("Identity", "Invert", "Solarize", "SolarizeAdd", "Posterize", "AutoContrast", "Equalize", "Brightness", "Color", "Contrast",
            "Sharpness", "Affine")
BILINEAR, BICUBIC = 2, 3                   # PIL.Image.BILINEAR / BICUBIC
MAGIC, HEADER_WORDS, ROW_WORDS = 0x31475541, 16, 20   # csrc/randaug.h
MAX_LAYERS, MAX_SIDE, MAX_GRID, MAX_COEFF = 8, 4096, 65535, float(1 << 40)
HIST_WORDS, TABLE_WORDS = 4 * 256, 3 * 256 + 1
FAM_TABLE, FAM_BLEND, FAM_SHARP, FAM_AFFINE, LAUNCH_STATS = 0, 1, 2, 3, 1 << 4
BUF_SRC, BUF_DST, BUF_WORK = 0, 1, 2
MAX_LEVEL = 10.0
FILL = (128, 128, 128)
NO_COEFFS = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)

# the reference's NAME_TO_OP / LEVEL_TO_ARG: name -> (device operation, level function)
OPS = {
    "AutoContrast": (AUTO_CONTRAST, None), "Equalize": (EQUALIZE, None), "Invert": (INVERT, None), "Rotate": (AFFINE, "rotate"),
    "Posterize": (POSTERIZE, "posterize"), "PosterizeIncreasing": (POSTERIZE, "posterize_inc"), "PosterizeOriginal": (POSTERIZE, "posterize_orig"),
    "Solarize": (SOLARIZE, "solarize"), "SolarizeIncreasing": (SOLARIZE, "solarize_inc"), "SolarizeAdd": (SOLARIZE_ADD, "solarize_add"),
    "Color": (COLOR, "enhance"), "ColorIncreasing": (COLOR, "enhance_inc"), "Contrast": (CONTRAST, "enhance"),
    "ContrastIncreasing": (CONTRAST, "enhance_inc"), "Brightness": (BRIGHTNESS, "enhance"), "BrightnessIncreasing": (BRIGHTNESS, "enhance_inc"),
    "Sharpness": (SHARPNESS, "enhance"), "SharpnessIncreasing": (SHARPNESS, "enhance_inc"), "ShearX": (AFFINE, "shear"), "ShearY": (AFFINE, "shear"),
    "TranslateX": (AFFINE, "translate_abs"), "TranslateY": (AFFINE, "translate_abs"), "TranslateXRel": (AFFINE, "translate_rel"),
    "TranslateYRel": (AFFINE, "translate_rel"),
}
RAND_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
                   "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RAND_INCREASING_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
                              "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
                              "TranslateXRel", "TranslateYRel")


def family(op):
    return FAM_TABLE if op <= EQUALIZE else (FAM_BLEND if op <= CONTRAST else (FAM_SHARP if op == SHARPNESS else FAM_AFFINE))


def table_words(capacity, layers):
    """32-bit words of a table with ``capacity`` rows per layer (csrc/randaug.h)."""
    return HEADER_WORDS + ROW_WORDS * int(capacity) * int(layers)


def aug_row(op, h, w, iarg=0, factor=0.0, coeffs=NO_COEFFS, filter=BICUBIC, fill=FILL):
    """One row of an AugDraw: ``(op, iarg, factor, coeffs[6], filter, fill[3], h, w)``."""
    return (int(op), int(iarg), float(factor), tuple(float(c) for c in coeffs), int(filter), tuple(int(v) for v in fill), int(h), int(w))


def rotate_coeffs(degrees, h, w):
    """The matrix ``PIL.Image.rotate(degrees)`` hands to ``transform(AFFINE)`` for an image of w x h; None: rotate() copies the image
    (``degrees % 360.0 == 0``).  Within the reference's +-30 degrees no other special case of rotate() is reached."""
    angle = degrees % 360.0
    if angle == 0:
        return None
    cx, cy = w / 2.0, h / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def row_error(row, batch_h=None, batch_w=None):
    """csrc/randaug.h's aug_row_ok as a text (None: the row is valid); the buffer words are made by ``AugDraw.words`` and not part of a row."""
    if len(row) != 8 or len(row[3]) != 6 or len(row[5]) != 3:
        return "a row is (op, iarg, factor, coeffs[6], filter, fill[3], h, w), got %r" % (tuple(row),)
    op, iarg, factor, coeffs, filt, fill, h, w = row
    if h < 1 or w < 1:
        return "the valid extent %d x %d is empty" % (h, w)
    if (batch_h is not None and h > batch_h) or (batch_w is not None and w > batch_w):
        return "the valid extent %d x %d lies outside the batch's %s x %s" % (h, w, batch_h, batch_w)
    if not (0 <= op < len(OP_NAMES)):
        return "operation %d is not one of the %d device operations" % (op, len(OP_NAMES))
    if not (0 <= iarg <= 256) or (op == SOLARIZE_ADD and iarg > 255) or (op == POSTERIZE and iarg > 8):
        return "the integer argument %d of %s is out of range (Solarize 0..256, SolarizeAdd 0..255, Posterize 0..8)" % (iarg, OP_NAMES[op])
    if filt not in (BILINEAR, BICUBIC):
        return "filter %d is not implemented (2 = bilinear, 3 = bicubic)" % filt
    if any(not (0 <= v <= 255) for v in fill):
        return "the fill colour %r is not three bytes" % (tuple(fill),)
    if not math.isfinite(factor) or abs(factor) > 3.4028234663852886e38:
        return "the factor %r is not a finite fp32 value" % (factor,)
    if any(not math.isfinite(c) or abs(c) > MAX_COEFF for c in coeffs):
        return "the coefficients %r are not finite values of at most 2^40" % (tuple(coeffs),)
    return None


def pack_row(row, src=BUF_SRC, dst=BUF_DST):
    """The 20 words of csrc/randaug.h's AugRow, unchecked: op, h, w, iarg, filter, fill, the fp32 factor, source | destination << 8 and
    six fp64 coefficients."""
    op, iarg, factor, coeffs, filt, fill, h, w = row
    return struct.pack("<6ifi6d", op, h, w, iarg, filt, fill[0] | fill[1] << 8 | fill[2] << 16, factor, src | dst << 8, *coeffs)


class AugDraw:
    """The host-side parameters of one batch: ``rows`` holds one row per (unit, layer), unit-major -- ``aug_row(op, h, w, iarg, factor,
    coeffs, filter, fill)`` -- and every unit has ``layers`` rows.  ``words(capacity)`` is the table the kernels read: there each row also
    names the buffer it reads and the one it writes, worked out here from the unit's sequence (layer 0 reads the source; pixel-local
    operations behind layer 0 work in place; Sharpness and Affine write the other buffer; the last layer leaves the unit in dst)."""

    def __init__(self, rows, layers):
        self.layers = int(layers)
        self.rows = []
        for r in rows:
            r = tuple(r)
            if len(r) != 8 or len(tuple(r[3])) != 6 or len(tuple(r[5])) != 3:
                raise ValueError("randaug: a row is (op, iarg, factor, coeffs[6], filter, fill[3], h, w), got %r" % (r,))
            self.rows.append(aug_row(r[0], r[6], r[7], r[1], r[2], r[3], r[4], r[5]))
        if not (1 <= self.layers <= MAX_LAYERS):
            raise ValueError("randaug: a draw has 1 to %d layers (got %d)" % (MAX_LAYERS, self.layers))
        if not self.rows or len(self.rows) % self.layers:
            raise ValueError("randaug: %d rows do not make units of %d layers" % (len(self.rows), self.layers))
        self.check()

    @property
    def units(self):
        return len(self.rows) // self.layers

    def unit_rows(self, u):
        return self.rows[u * self.layers:(u + 1) * self.layers]

    def sizes(self):
        """[(h, w)] of the units"""
        return [(self.rows[u * self.layers][6], self.rows[u * self.layers][7]) for u in range(self.units)]

    def names(self):
        """the operation names, [units][layers]"""
        return [[OP_NAMES[r[0]] for r in self.unit_rows(u)] for u in range(self.units)]

    def check(self, batch_h=None, batch_w=None):
        """The refusal of an invalid row, made where the values are still on the host (the device would write such a unit as zeros)."""
        for i, r in enumerate(self.rows):
            e = row_error(r, batch_h, batch_w)
            if e is None and (r[6], r[7]) != (self.rows[i - i % self.layers][6], self.rows[i - i % self.layers][7]):
                e = "the layers of a unit disagree about its extent"
            if e:
                raise ValueError("randaug: unit %d, layer %d: %s" % (i // self.layers, i % self.layers, e))

    def buffers(self):
        """[(source, destination)] per row, unit-major: the buffer bookkeeping of csrc/randaug.hip."""
        out = []
        for u in range(self.units):
            ops = [r[0] for r in self.unit_rows(u)]
            moves = sum(1 for op in ops[1:] if family(op) >= FAM_SHARP)      # layers behind the first that change buffers
            at = BUF_DST if moves % 2 == 0 else BUF_WORK
            out.append((BUF_SRC, at))
            for op in ops[1:]:
                if family(op) >= FAM_SHARP:
                    nxt = BUF_WORK if at == BUF_DST else BUF_DST
                    out.append((at, nxt))
                    at = nxt
                else:
                    out.append((at, at))
            assert at == BUF_DST
        return out

    def launch_mask(self):
        """One word per layer (csrc/randaug.h): bit f = some unit runs an operation of family f; bit 4 = some unit needs the histograms.
        A layer in which every unit is an Identity behind layer 0 launches nothing."""
        bufs = self.buffers()
        mask = [0] * self.layers
        for i, r in enumerate(self.rows):
            layer = i % self.layers
            if r[0] == IDENTITY and bufs[i][0] == bufs[i][1]:
                continue
            mask[layer] |= 1 << family(r[0])
            if r[0] in (AUTO_CONTRAST, EQUALIZE, CONTRAST):
                mask[layer] |= LAUNCH_STATS
        return mask

    def words(self, capacity=None):
        """The table as bytes: the 16-word header, then rows [layers][capacity] (zero rows behind this draw's units)."""
        capacity = self.units if capacity is None else int(capacity)
        if capacity < self.units:
            raise ValueError("randaug: the draw holds %d units, the table %d" % (self.units, capacity))
        bufs = self.buffers()
        out = [struct.pack("<16i", MAGIC, self.units, self.layers, *([0] * 13))]
        for layer in range(self.layers):
            for u in range(self.units):
                out.append(pack_row(self.rows[u * self.layers + layer], *bufs[u * self.layers + layer]))
            out.append(b"\0" * (4 * ROW_WORDS * (capacity - self.units)))
        return b"".join(out)

    def __repr__(self):
        return "AugDraw(%r, layers=%d)" % (self.rows, self.layers)


def _sizes_list(sizes):
    from util.crop import _sizes_list as f
    return f(sizes)


def parse_config(config_str):
    """(magnitude, num_layers, magnitude_std, transforms) of the reference's ``rand_augment_transform`` config string, quirks included:
    ``bool(val)`` of a non-empty string is true, so ``inc0`` selects the increasing set too; the first ``mstd`` wins."""
    magnitude, num_layers, mstd, transforms = MAX_LEVEL, 2, None, RAND_TRANSFORMS
    config = config_str.split("-")
    if config[0] != "rand":
        raise ValueError("DeviceRandAugment: the config string starts with 'rand' (got %r)" % (config_str,))
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            if mstd is None:
                mstd = float(val)
        elif key == "inc":
            if bool(val):
                transforms = RAND_INCREASING_TRANSFORMS
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "w":
            raise NotImplementedError("DeviceRandAugment: 'w' (weighted choice without replacement) is not implemented")
        else:
            raise NotImplementedError("DeviceRandAugment: config key %r is not implemented (m, n, mstd, inc)" % (key,))
    if not (1 <= num_layers <= MAX_LAYERS):
        raise NotImplementedError("DeviceRandAugment: n = %d is not implemented (1 to %d layers)" % (num_layers, MAX_LAYERS))
    return magnitude, num_layers, (mstd or 0), transforms


class DeviceRandAugment:
    """``rand_augment_transform(config_str, hparams)`` with ``hparams`` = interpolation, img_mean (``fill``) and ``translate_const`` (None:
    the reference's default 250).  ``py_rng`` (a random.Random; None: the ``random`` module) and ``np_rng`` (a numpy RandomState; None:
    numpy's global one).  Only what the kernels implement is accepted: Pillow's bilinear and bicubic filters."""

    def __init__(self, config_str, interpolation="bicubic", fill=FILL, translate_const=None, py_rng=None, np_rng=None):
        if interpolation == "random":
            raise NotImplementedError("DeviceRandAugment: interpolation='random' (a draw per frame) is not implemented")
        interpolation = {"bilinear": BILINEAR, "bicubic": BICUBIC}.get(interpolation, getattr(interpolation, "value", interpolation))
        if interpolation not in (BILINEAR, BICUBIC):
            raise NotImplementedError("DeviceRandAugment: interpolation=%r is not implemented ('bilinear' or 'bicubic')" % (interpolation,))
        fill = tuple(int(v) for v in fill)
        if len(fill) != 3 or any(not (0 <= v <= 255) for v in fill):
            raise ValueError("DeviceRandAugment: fill is three bytes (got %r)" % (fill,))
        self.config_str = config_str
        self.magnitude, self.num_layers, self.magnitude_std, self.transforms = parse_config(config_str)
        self.prob = 0.5
        self.interpolation, self.fill = interpolation, fill
        self.translate_const = 250 if translate_const is None else translate_const
        self.translate_pct = 0.45
        self.py_rng, self.np_rng = py_rng, np_rng
        self._injected = []

    @classmethod
    def from_reference(cls, input_size, auto_augment, interpolation="bilinear", py_rng=None, np_rng=None):
        """``create_random_augment(input_size, auto_augment, interpolation)`` of the reference's video_datasets/transform.py."""
        img_size = input_size[-2:] if isinstance(input_size, tuple) else input_size
        img_size_min = min(img_size) if isinstance(img_size, tuple) else img_size
        if not (isinstance(auto_augment, str) and auto_augment.startswith("rand")):
            raise NotImplementedError("DeviceRandAugment: auto_augment=%r is not implemented ('rand-...')" % (auto_augment,))
        if interpolation in ("lanczos", "hamming"):
            raise NotImplementedError("DeviceRandAugment: interpolation=%r is not implemented ('bilinear' or 'bicubic')" % (interpolation,))
        if interpolation and interpolation != "random":
            interpolation = "bicubic" if interpolation == "bicubic" else "bilinear"   # _pil_interp
        else:
            interpolation = "random"
        return cls(auto_augment, interpolation=interpolation, fill=FILL, translate_const=int(img_size_min * 0.45), py_rng=py_rng, np_rng=np_rng)

    def inject(self, draws):
        """A fixed draw (an AugDraw, or a list of them) that the next calls of ``draw_for()`` hand out in order: for tests and recorded runs."""
        self._injected.extend([draws] if isinstance(draws, AugDraw) else draws)
        return self

    # ---- the reference's level functions -------------------------------------------------------------------------------------------------
    def _negate(self, rnd, v):
        return -v if rnd.random() > 0.5 else v

    def level_args(self, kind, level, rnd):
        if kind == "rotate":
            return self._negate(rnd, (level / MAX_LEVEL) * 30.0)
        if kind == "enhance":
            return (level / MAX_LEVEL) * 1.8 + 0.1
        if kind == "enhance_inc":
            return 1.0 + self._negate(rnd, (level / MAX_LEVEL) * 0.9)
        if kind == "shear":
            return self._negate(rnd, (level / MAX_LEVEL) * 0.3)
        if kind == "translate_abs":
            return self._negate(rnd, (level / MAX_LEVEL) * float(self.translate_const))
        if kind == "translate_rel":
            return self._negate(rnd, (level / MAX_LEVEL) * self.translate_pct)
        if kind == "posterize":
            return int((level / MAX_LEVEL) * 4)
        if kind == "posterize_inc":
            return 4 - int((level / MAX_LEVEL) * 4)
        if kind == "posterize_orig":
            return int((level / MAX_LEVEL) * 4) + 4
        if kind == "solarize":
            return int((level / MAX_LEVEL) * 256)
        if kind == "solarize_inc":
            return 256 - int((level / MAX_LEVEL) * 256)
        if kind == "solarize_add":
            return int((level / MAX_LEVEL) * 110)
        raise ValueError(kind)

    def device_row(self, name, arg, h, w):
        """The device row of the reference's op ``name`` called with level argument ``arg`` on a frame of h x w."""
        op, kind = OPS[name]
        kw = dict(filter=self.interpolation, fill=self.fill)
        if op in (AUTO_CONTRAST, EQUALIZE, INVERT):
            return aug_row(op, h, w, **kw)
        if op in (POSTERIZE, SOLARIZE, SOLARIZE_ADD):
            return aug_row(op, h, w, iarg=arg, **kw)
        if op != AFFINE:
            return aug_row(op, h, w, factor=arg, **kw)
        if name == "Rotate":
            c = rotate_coeffs(arg, h, w)
            return aug_row(IDENTITY, h, w, **kw) if c is None else aug_row(AFFINE, h, w, coeffs=c, **kw)
        if name == "ShearX":
            c = (1, arg, 0, 0, 1, 0)
        elif name == "ShearY":
            c = (1, 0, 0, arg, 1, 0)
        elif name == "TranslateX":
            c = (1, 0, arg, 0, 1, 0)
        elif name == "TranslateY":
            c = (1, 0, 0, 0, 1, arg)
        elif name == "TranslateXRel":
            c = (1, 0, arg * w, 0, 1, 0)
        else:
            c = (1, 0, 0, 0, 1, arg * h)
        return aug_row(AFFINE, h, w, coeffs=c, **kw)

    def draw_unit(self, h, w):
        """[(name, applied, level argument or None)] of one clip: RandAugment.__call__ and AugmentOp.__call__ line by line."""
        import random
        import numpy as np
        rnd = random if self.py_rng is None else self.py_rng
        rng = np.random if self.np_rng is None else self.np_rng
        chosen = rng.choice(len(self.transforms), self.num_layers)
        out = []
        for k in chosen:
            name = self.transforms[int(k)]
            if self.prob < 1.0 and rnd.random() > self.prob:
                out.append((name, False, None))
                continue
            magnitude = self.magnitude
            if self.magnitude_std and self.magnitude_std > 0:
                magnitude = rnd.gauss(magnitude, self.magnitude_std)
            magnitude = min(MAX_LEVEL, max(0, magnitude))
            kind = OPS[name][1]
            out.append((name, True, None if kind is None else self.level_args(kind, magnitude, rnd)))
        return out

    def draw_for(self, sizes):
        """The draw of a batch whose clips (or images) have the (height, width) rows of ``sizes``."""
        sizes = _sizes_list(sizes)
        if self._injected:
            d = self._injected.pop(0)
            if d.units != len(sizes) or d.sizes() != sizes:
                raise ValueError("randaug: the injected draw was made for %r, the batch holds %r" % (d.sizes(), sizes))
            return d
        rows = []
        for (h, w) in sizes:
            for (name, applied, arg) in self.draw_unit(h, w):
                rows.append(self.device_row(name, arg, h, w) if applied else aug_row(IDENTITY, h, w, filter=self.interpolation, fill=self.fill))
        return AugDraw(rows, self.num_layers)

    def __call__(self, pixels, sizes=None):
        """New bytes of the shape of a device batch uint8 [B, T, Hs, Ws, 3] (clips) or [B, Hs, Ws, 3] (images); ``sizes`` [B, 2] (host) =
        the valid (height, width) of each, None: every one fills the batch's shape."""
        from _lib import randaug_u8
        import torch
        if sizes is None:
            sizes = [(int(pixels.shape[-3]), int(pixels.shape[-2]))] * int(pixels.shape[0])
        d = self.draw_for(sizes)
        table = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(pixels.device)
        return randaug_u8(pixels, table, d)
