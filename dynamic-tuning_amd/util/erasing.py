"""Random Erasing on the device: ``DeviceRandomErasing`` stands where ``RandomErasing`` stands in the reference's data pipelines
(util/datasets.py ``re_prob`` / ``re_mode`` / ``re_count``; video_datasets/random_erasing.py for clips).

This is a RESTATEMENT of the "erase a batch after normalisation" RandomErasing of timm / SlowFast (neither is a dependency): the boxes are
drawn on the host, one draw sequence per unit -- an image, or with ``cube`` a clip whose frames share the boxes -- and the pixels are
written on the device (csrc/erase.h, csrc/image_load.hip).  The draws come from a ``random.Random`` (the reference uses the ``random`` module's
global state, so a generator of the same seed draws the same boxes), per unit in this order:

    1. ``random()``; the unit is erased unless the value is > probability
    2. min_count != max_count only: ``count = randint(min_count, max_count)``
    3. per box up to 10 attempts (100 with ``cube``): ``uniform(min_area, max_area)`` for the area (x 224 x 224 / count),
       ``uniform(log min_aspect, log max_aspect)`` for the log aspect ratio, h and w rounded; the attempt counts if w < 224 and h < 224,
       and then draws ``randint(0, 224 - h)`` for the top and ``randint(0, 224 - w)`` for the left edge
    4. after ALL units of the batch: ``getrandbits(64)``, the seed of the batch's noise (so the boxes are those of the reference)

The noise (modes 'rand' and 'pixel') is the library's Philox4x32-10 stream through Box-Muller, keyed by pixel position: N(0,1) values like
the reference's ``normal_()``, not torch's bits.

Two ways to use it:
  * ``train_one_epoch(..., args)`` with ``args.random_erasing = DeviceRandomErasing(...)``: the loop draws, hands the draw to the engine
    (``set_erase``) and passes the batch as it is (bytes stay bytes) to the fused step, which erases -- and then mixes, with a DeviceMixup --
    inside the patch-embedding load; hipGraph replay stays on.
  * ``erased = DeviceRandomErasing(...)(x)`` on a device batch: fp32 images out (libdyt_hip's dyt_erase_images).
"""
import math
import random
import struct

IMG = 224
OFF, CONST, RAND, PIXEL = 0, 1, 2, 3
MODES = {"const": CONST, "rand": RAND, "pixel": PIXEL}
MAX_BOXES = 4
HEADER_WORDS, ROW_WORDS = 16, 20


def table_words(capacity):
    """32-bit words of a table with ``capacity`` rows (csrc/erase.h)."""
    return HEADER_WORDS + ROW_WORDS * int(capacity)


class EraseDraw:
    """The host-side parameters of one batch: ``mode`` (1 const, 2 rand, 3 pixel), per unit the list of its boxes ``(top, h, left, w)`` (at
    most 4, applied in order: a later box overwrites an earlier one), ``cube`` (a unit is a clip of ``frames`` images) and the 64-bit
    ``seed`` of the noise.  ``words(capacity)`` is the table the kernels read (csrc/erase.h)."""

    def __init__(self, mode, boxes, seed=0, cube=False, frames=1):
        self.mode = MODES[mode.lower()] if isinstance(mode, str) else int(mode)
        self.boxes = [[tuple(int(v) for v in b) for b in unit] for unit in boxes]
        self.seed, self.cube, self.frames = int(seed) & (2 ** 64 - 1), bool(cube), int(frames)
        self.check()

    @property
    def units(self):
        return len(self.boxes)

    def images(self):
        """The number of images the draw covers."""
        return self.units * (self.frames if self.cube else 1)

    def check(self):
        """The refusals of csrc/erase.h (erase_mode_error, erase_count_error, erase_box_error), made where the values are still on the host."""
        if self.mode not in (CONST, RAND, PIXEL):
            raise ValueError("erase: mode is 1 (const), 2 (rand) or 3 (pixel), got %r" % (self.mode,))
        if self.frames < 1:
            raise ValueError("erase: frames < 1")
        if not self.boxes:
            raise ValueError("erase: the draw holds no unit")
        for unit in self.boxes:
            if len(unit) > MAX_BOXES:
                raise ValueError("erase: a unit holds 0 to 4 boxes, got %d" % len(unit))
            for b in unit:
                if len(b) != 4:
                    raise ValueError("erase: a box is (top, h, left, w), got %r" % (b,))
                top, h, left, w = b
                if h < 1 or w < 1:
                    raise ValueError("erase: the box %r has h < 1 or w < 1" % (b,))
                if top < 0 or left < 0 or top + h > IMG or left + w > IMG:
                    raise ValueError("erase: the box %r lies outside the 224 x 224 image" % (b,))

    def words(self, capacity=None):
        """The table as bytes: the 16-word header, the rows of this draw, zero rows up to ``capacity``."""
        capacity = self.units if capacity is None else int(capacity)
        if capacity < self.units:
            raise ValueError("erase: the draw holds %d units, the table %d" % (self.units, capacity))
        out = [struct.pack("<4i2I10i", self.mode, self.frames, 1 if self.cube else 0, self.units, self.seed & 0xFFFFFFFF, self.seed >> 32,
                           *([0] * 10))]
        for unit in self.boxes:
            flat = [v for b in unit for v in b] + [0] * (4 * (MAX_BOXES - len(unit)))
            out.append(struct.pack("<20i", len(unit), *flat, 0, 0, 0))
        out.append(b"\0" * (4 * ROW_WORDS * (capacity - self.units)))
        return b"".join(out)

    def __repr__(self):
        return "EraseDraw(mode=%d, boxes=%r, seed=%#x, cube=%r, frames=%d)" % (self.mode, self.boxes, self.seed, self.cube, self.frames)


class DeviceRandomErasing:
    """The reference RandomErasing's arguments (plus ``generator``: a random.Random or a seed; minus ``device``).  Only what the kernels
    implement is accepted: at most 4 boxes per unit, no ``num_splits``."""

    def __init__(self, probability=0.5, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode='const', min_count=1,
                 max_count=None, num_splits=0, cube=False, generator=None):
        if num_splits > 1:
            raise NotImplementedError("DeviceRandomErasing: num_splits=%r is not implemented" % (num_splits,))
        max_count = max_count or min_count
        if max_count > MAX_BOXES:
            raise NotImplementedError("DeviceRandomErasing: max_count=%r (the kernels take at most %d boxes per unit)" % (max_count, MAX_BOXES))
        if min_count < 1 or min_count > max_count:
            raise ValueError("DeviceRandomErasing: 1 <= min_count <= max_count")
        mode = (mode or "const").lower()
        if mode not in MODES:
            raise ValueError("DeviceRandomErasing: mode is 'const', 'rand' or 'pixel', got %r" % (mode,))
        self.probability, self.min_area, self.max_area = probability, min_area, max_area
        max_aspect = max_aspect or 1 / min_aspect
        self.log_aspect_ratio = (math.log(min_aspect), math.log(max_aspect))
        self.min_count, self.max_count, self.num_splits = int(min_count), int(max_count), num_splits
        self.mode, self.cube = mode, bool(cube)
        self.rng = generator if isinstance(generator, random.Random) else random.Random(generator)
        self._injected = []

    def inject(self, draws):
        """Fixed draws (EraseDraw objects) that the next calls of ``draw()`` hand out in order, before the generator is asked again: for
        tests and comparisons against recorded runs."""
        self._injected.extend(draws)
        return self

    def _unit(self):
        rng = self.rng
        if rng.random() > self.probability:
            return []
        count = self.min_count if self.min_count == self.max_count else rng.randint(self.min_count, self.max_count)
        boxes = []
        for _ in range(count):
            for _ in range(100 if self.cube else 10):
                area = rng.uniform(self.min_area, self.max_area) * (IMG * IMG) / count
                aspect = math.exp(rng.uniform(*self.log_aspect_ratio))
                h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
                if w < IMG and h < IMG:
                    top = rng.randint(0, IMG - h)
                    left = rng.randint(0, IMG - w)
                    if h > 0 and w > 0:   # (an empty box erases nothing; its draws are consumed all the same)
                        boxes.append((top, h, left, w))
                    break
        return boxes

    def draw_boxes(self, units):
        """The boxes of ``units`` units, in the reference's draw order (steps 1-3 of the module text)."""
        return [self._unit() for _ in range(int(units))]

    def draw(self, units, frames=1):
        """The host-side parameters of the next batch of ``units`` units (images; clips of ``frames`` images with ``cube``)."""
        if self._injected:
            d = self._injected.pop(0)
            if d.units != int(units):
                raise ValueError("erase: the injected draw holds %d units, the batch %d" % (d.units, int(units)))
            return d
        boxes = self.draw_boxes(units)
        return EraseDraw(self.mode, boxes, self.rng.getrandbits(64), self.cube, frames if self.cube else 1)

    def draw_for(self, images, frames=1):
        """The draw of a batch of ``images`` images folded from clips of ``frames``."""
        images, frames = int(images), int(frames)
        if frames < 1 or images % frames != 0:
            raise ValueError("erase: %d images are not a multiple of %d frames" % (images, frames))
        return self.draw(images // frames if self.cube else images, frames)

    def __call__(self, x, norm=None):
        """The erased fp32 images of a device batch.  ``x``: fp32 or uint8 images [n,3,224,224] / uint8 [n,224,224,3], or clips
        [b,3,t,224,224] / uint8 [b,t,224,224,3] (fp32 clips come back as [b,3,t,224,224]).  ``norm`` = (mean, std) of uint8 input (the
        model's ``input_norm``)."""
        import torch
        from _lib import erase_images
        frames, clips = 1, None
        if x.dim() == 5:
            clips = x.shape[0]
            if x.dtype == torch.uint8 and tuple(x.shape[2:]) == (IMG, IMG, 3):
                frames = x.shape[1]
                x = x.reshape(clips * frames, IMG, IMG, 3)
            else:
                frames = x.shape[2]
                x = x.permute(0, 2, 1, 3, 4).reshape(clips * frames, 3, IMG, IMG)
        d = self.draw_for(x.shape[0], frames)
        table = torch.frombuffer(bytearray(d.words(x.shape[0])), dtype=torch.int32).to(x.device)   # a row for every image: what the entry asks for
        out = erase_images(x.contiguous(), table, frames=frames, norm=norm)
        if clips is not None:
            out = out.reshape(clips, frames, 3, IMG, IMG).permute(0, 2, 1, 3, 4)
        return out
