"""RandomResizedCrop + RandomHorizontalFlip / Resize + CenterCrop on the device, from byte sources: ``DeviceRandomResizedCrop`` stands where
``util/crop.py``'s ``RandomResizedCrop(224, interpolation=3)`` followed by ``RandomHorizontalFlip()`` stands in the reference's train
pipeline (datasets/image_datasets.py), ``DeviceResizeCenterCrop`` where ``Resize(256, interpolation=3)`` + ``CenterCrop(224)`` stand in its
evaluation pipeline.  The loader decodes and pads only (``pad_collate``); the boxes are drawn on the host and the pixels are written on the
device (csrc/resample.h, csrc/resample.hip): Pillow's 8-bit bicubic ``Image.resize`` restated bit for bit.

The draws are a RESTATEMENT of the reference ``RandomResizedCrop.get_params`` (torchvision is not a dependency), per image in this order:

    1. ``torch.empty(1).uniform_(scale[0], scale[1])`` for the area, as a fraction of the image's
    2. ``torch.empty(1).uniform_(log ratio[0], log ratio[1])`` for the log aspect ratio (the logs and the ``exp`` in fp32, as there);
       w and h rounded and clipped to the image
    3. ``torch.randint(0, height - h + 1, (1,))`` for the top and ``torch.randint(0, width - w + 1, (1,))`` for the left edge
    4. ``torch.rand(1) < flip``: RandomHorizontalFlip's own call (``flip=None``: no flip stage, no draw)

With ``generator=None`` they come from torch's global generator, as the reference's do, so a seeded run draws the reference's boxes.

Two ways to use it:
  * ``train_one_epoch(..., args)`` with ``args.device_crop = DeviceRandomResizedCrop()`` (``evaluate`` with
    ``args.device_eval_crop = DeviceResizeCenterCrop()``): the loader yields ``((pixels, sizes), labels)``, the loop draws, the engine
    resamples on the compute stream (``DyTEngine.resample``) and the step sees a 224 x 224 channels-last byte batch.
  * ``cropped = DeviceRandomResizedCrop()(pixels, sizes)`` on a device batch: uint8 [B, 224, 224, 3] out (libdyt_hip's dyt_resample_u8).

Video clips have three classes of their own at the end of this file -- ``DeviceClipScaleJitterCrop`` (the reference's K400 train path),
``DeviceClipRandomResizedCrop`` (its SSV2 train path) and ``DeviceClipUniformCrop`` (its one- / three-view evaluation) -- over
csrc/resample_clip.h / .hip: torch's float bilinear ``interpolate`` of the normalised frames restated bit for bit, fp32 clips out.  Their
rows carry a 12th word, the source clip, so several rows (spatial views) can read one clip; ``pad_collate_clips`` is their collate_fn.
"""
import math
import struct

OUT = 224
BICUBIC = 3
HEADER_WORDS, ROW_WORDS = 16, 12
MAX_SIDE = 4096
FLAG_MIRROR = 1
BILINEAR_F32 = 2          # the header's filter word of a clip table (csrc/resample_clip.h): torch's float bilinear
MAX_FULL = 1 << 23        # largest `full` side of a clip row: (float)d + 0.5f stays exact


def table_words(capacity):
    """32-bit words of a table with ``capacity`` rows (csrc/resample.h)."""
    return HEADER_WORDS + ROW_WORDS * int(capacity)


def row_error(row, batch_h=None, batch_w=None, wide=False):
    """csrc/resample.h's resample_row_ok as a text (None: the row is valid).  ``wide``: csrc/resample_wide.h's resample_wide_row_ok -- the
    same conditions without the bound of 2.5 (a side is at most 4096, which bounds the taps by 75)."""
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags = row
    if wide and (sh > MAX_SIDE or sw > MAX_SIDE):
        return "the valid extent %d x %d has a side above %d" % (sh, sw, MAX_SIDE)
    if sh < 1 or sw < 1:
        return "the valid extent %d x %d is empty" % (sh, sw)
    if (batch_h is not None and sh > batch_h) or (batch_w is not None and sw > batch_w):
        return "the valid extent %d x %d lies outside the batch's %s x %s" % (sh, sw, batch_h, batch_w)
    if bh < 1 or bw < 1:
        return "the box has h < 1 or w < 1 (%d x %d)" % (bh, bw)
    if top < 0 or left < 0 or top + bh > sh or left + bw > sw:
        return "the box (top %d, left %d, %d x %d) lies outside the image's %d x %d" % (top, left, bh, bw, sh, sw)
    if fh < OUT or fw < OUT:
        return "the resized image %d x %d is smaller than the %d x %d window" % (fh, fw, OUT, OUT)
    if oy < 0 or ox < 0 or oy + OUT > fh or ox + OUT > fw:
        return "the window (offset %d, %d) lies outside the resized image %d x %d" % (oy, ox, fh, fw)
    if not wide and (2 * bh > 5 * fh or 2 * bw > 5 * fw):
        return ("the box %d x %d is more than 2.5 times the resized image %d x %d (the kernels take at most 11 taps): decode to a smaller "
                "size" % (bh, bw, fh, fw))
    return None


def clip_row_error(row, batch=None, batch_h=None, batch_w=None):
    """csrc/resample_clip.h's clip_row_ok as a text (None: the row is valid).  ``row`` has 12 words: the 11 of ``row_error`` and ``src``,
    the source clip the row reads.  There is no 2.5x bound; ``full`` is at most 2^23."""
    if len(row) != 12:
        return "a clip row is (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags, src), got %r" % (tuple(row),)
    sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags, src = row
    if sh < 1 or sw < 1:
        return "the valid extent %d x %d is empty" % (sh, sw)
    if (batch_h is not None and sh > batch_h) or (batch_w is not None and sw > batch_w):
        return "the valid extent %d x %d lies outside the batch's %s x %s" % (sh, sw, batch_h, batch_w)
    if bh < 1 or bw < 1:
        return "the box has h < 1 or w < 1 (%d x %d)" % (bh, bw)
    if top < 0 or left < 0 or top + bh > sh or left + bw > sw:
        return "the box (top %d, left %d, %d x %d) lies outside the clip's %d x %d" % (top, left, bh, bw, sh, sw)
    if fh < OUT or fw < OUT:
        return "the resized clip %d x %d is smaller than the %d x %d window" % (fh, fw, OUT, OUT)
    if fh > MAX_FULL or fw > MAX_FULL:
        return "the resized clip %d x %d is larger than %d (positions must stay exact in fp32)" % (fh, fw, MAX_FULL)
    if oy < 0 or ox < 0 or oy + OUT > fh or ox + OUT > fw:
        return "the window (offset %d, %d) lies outside the resized clip %d x %d" % (oy, ox, fh, fw)
    if src < 0 or (batch is not None and src >= batch):
        return "the source clip %d lies outside the batch of %s" % (src, batch)
    return None


class CropDraw:
    """The host-side parameters of one batch: per image the row ``(src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x,
    flags)`` of csrc/resample.h.  ``words(capacity)`` is the table the kernels read.  With ``filter=BILINEAR_F32`` the rows are CLIP rows
    (csrc/resample_clip.h): a 12th word ``src`` names the source clip a row reads, output unit r is written from row r, and the rows are
    checked with ``clip_row_error``.  ``wide``: a draw for the wide-tap kernels (csrc/resample_wide.h) -- the same table, its rows checked
    without the bound of 2.5; the engine resamples a wide draw with dyt_resample_wide_u8, whatever its rows."""

    def __init__(self, rows, filter=BICUBIC, wide=False):
        self.rows = [tuple(int(v) for v in r) for r in rows]
        self.filter = int(filter)
        self.wide = bool(wide)
        if self.wide and self.filter != BICUBIC:
            raise ValueError("resample: wide=True is a draw of image rows (clip rows have no scale bound)")
        if self.filter not in (BICUBIC, BILINEAR_F32):
            raise ValueError("resample: filter %r is not implemented (3 = Pillow's bicubic on bytes, 2 = torch's float bilinear on clips)" % (filter,))
        if not self.rows:
            raise ValueError("resample: the draw holds no image")
        for r in self.rows:
            if len(r) != (12 if self.clip else 11):
                raise ValueError("resample: a row is (src_h, src_w, top, left, box_h, box_w, full_h, full_w, off_y, off_x, flags%s), got %r" % (
                    ", src" if self.clip else "", r))
        self.check()

    @property
    def clip(self):
        return self.filter == BILINEAR_F32

    @property
    def units(self):
        return len(self.rows)

    def images(self):
        return len(self.rows)

    def sources(self):
        """The source image / clip of every row (a bicubic row reads the image of its own number)."""
        return [r[11] for r in self.rows] if self.clip else list(range(len(self.rows)))

    def check(self, batch_h=None, batch_w=None, batch=None, wide=None):
        """The refusal of an invalid row, made where the values are still on the host (the device would write such an image as zeros).
        ``wide`` (None: the draw's own): check the rows for the wide-tap kernels."""
        wide = self.wide if wide is None else bool(wide)
        for i, r in enumerate(self.rows):
            e = clip_row_error(r, batch, batch_h, batch_w) if self.clip else row_error(r, batch_h, batch_w, wide=wide)
            if e:
                raise ValueError("resample: %s %d: %s" % ("unit" if self.clip else "image", i, e))

    def boxes(self):
        """[(i, j, h, w)] as ``get_params`` returns them."""
        return [(r[2], r[3], r[4], r[5]) for r in self.rows]

    def flips(self):
        return [bool(r[10] & FLAG_MIRROR) for r in self.rows]

    def words(self, capacity=None):
        """The table as bytes: the 16-word header, the rows of this draw, zero rows up to ``capacity``."""
        capacity = self.units if capacity is None else int(capacity)
        if capacity < self.units:
            raise ValueError("resample: the draw holds %d images, the table %d" % (self.units, capacity))
        out = [struct.pack("<16i", self.filter, self.units, *([0] * 14))]
        for r in self.rows:
            out.append(struct.pack("<12i", *(r if self.clip else r + (0,))))
        out.append(b"\0" * (4 * ROW_WORDS * (capacity - self.units)))
        return b"".join(out)

    def __repr__(self):
        return "CropDraw(%r%s%s)" % (self.rows, ", filter=%d" % self.filter if self.clip else "", ", wide=True" if self.wide else "")


def _sizes_list(sizes):
    """[(h, w)] from an int tensor / array / list [B, 2] that lives on the host."""
    if hasattr(sizes, "is_cuda") and sizes.is_cuda:
        raise ValueError("resample: sizes must stay on the host (the boxes are drawn there)")
    rows = sizes.tolist() if hasattr(sizes, "tolist") else list(sizes)
    out = []
    for r in rows:
        if len(r) != 2:
            raise ValueError("resample: sizes is [B, 2] = (height, width) per image, got a row %r" % (r,))
        h, w = int(r[0]), int(r[1])
        if h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError("resample: an image of %d x %d (sides are 1 to %d)" % (h, w, MAX_SIDE))
        out.append((h, w))
    if not out:
        raise ValueError("resample: sizes holds no image")
    return out


def full_sizes(pixels):
    """The sizes of a bare batch [B, Hs, Ws, 3] that every image fills."""
    return [(int(pixels.shape[1]), int(pixels.shape[2]))] * int(pixels.shape[0])


class _DeviceCrop:
    def __call__(self, pixels, sizes=None):
        """The cropped byte batch uint8 [B, 224, 224, 3] of a device batch uint8 [B, Hs, Ws, 3]; ``sizes`` [B, 2] (host) = the images' valid
        (height, width), None: every image fills the batch's shape."""
        from _lib import resample_u8, resample_wide_u8
        import torch
        d = self.draw_for(full_sizes(pixels) if sizes is None else sizes)
        if d.units != int(pixels.shape[0]):
            raise ValueError("resample: %d sizes for a batch of %d images" % (d.units, int(pixels.shape[0])))
        table = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(pixels.device)
        return (resample_wide_u8 if d.wide else resample_u8)(pixels, table, d)


class DeviceRandomResizedCrop(_DeviceCrop):
    """The reference RandomResizedCrop's arguments plus ``flip`` (RandomHorizontalFlip's p; None: no flip stage) and ``generator`` (a
    torch.Generator; None: torch's global one, as the reference).  Only what the kernels implement is accepted: size 224, bicubic.
    ``any_scale``: the draws are wide draws (the wide-tap kernels, csrc/resample_wide.h): the same boxes from the same random numbers, and
    a box may be any multiple of 224 instead of at most 2.5 times."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation=3, flip=0.5, generator=None, any_scale=False):
        if isinstance(size, (tuple, list)):
            size = size[0] if len(size) == 1 or (len(size) == 2 and size[0] == size[1]) else size
        if size != OUT:
            raise NotImplementedError("DeviceRandomResizedCrop: size=%r is not implemented (the kernels write 224 x 224)" % (size,))
        if getattr(interpolation, "value", interpolation) not in (BICUBIC, "bicubic"):
            raise NotImplementedError("DeviceRandomResizedCrop: interpolation=%r is not implemented (3 = bicubic only)" % (interpolation,))
        if len(scale) != 2 or len(ratio) != 2 or not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError("DeviceRandomResizedCrop: scale and ratio are (min, max) with 0 < min <= max")
        if flip is not None and not (0.0 <= float(flip) <= 1.0):
            raise ValueError("DeviceRandomResizedCrop: flip is a probability or None")
        self.size, self.scale, self.ratio, self.interpolation, self.flip, self.generator = OUT, tuple(scale), tuple(ratio), BICUBIC, flip, generator
        self.any_scale = bool(any_scale)
        self._injected = []

    def inject(self, draws):
        """Fixed draws (CropDraw objects) that the next calls of ``draw_for()`` hand out in order: for tests and recorded runs."""
        self._injected.extend(draws)
        return self

    def get_params(self, height, width):
        """(i, j, h, w) of one image: the reference's ``get_params`` line by line.  A side that rounds to 0 (images of a few pixels) is
        raised to 1, where the reference would crop an empty box."""
        import torch
        g = self.generator
        area = height * width
        target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
        log_ratio = torch.log(torch.tensor(self.ratio))
        aspect_ratio = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        w = max(1, min(w, width))
        h = max(1, min(h, height))
        i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
        j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
        return i, j, h, w

    def draw_for(self, sizes):
        """The draw of a batch whose images have the (height, width) rows of ``sizes``."""
        import torch
        sizes = _sizes_list(sizes)
        if self._injected:
            d = self._injected.pop(0)
            if d.units != len(sizes):
                raise ValueError("resample: the injected draw holds %d images, the batch %d" % (d.units, len(sizes)))
            return d
        rows = []
        for (sh, sw) in sizes:
            i, j, h, w = self.get_params(sh, sw)
            mirror = bool(torch.rand(1, generator=self.generator) < self.flip) if self.flip is not None else False
            rows.append((sh, sw, i, j, h, w, OUT, OUT, 0, 0, FLAG_MIRROR if mirror else 0))
        return CropDraw(rows, wide=self.any_scale)


class DeviceResizeCenterCrop(_DeviceCrop):
    """``Resize(resize, interpolation=3)`` + ``CenterCrop(size)`` of torchvision: the short side becomes ``resize``, the long side
    ``int(resize * long / short)``; the window starts at ``int(round((full - size) / 2.0))``.  Makes no draw.  ``any_scale``: wide draws
    (csrc/resample_wide.h), so a short side above 2.5 x ``resize`` is taken."""

    def __init__(self, resize=256, size=224, interpolation=3, any_scale=False):
        if size != OUT:
            raise NotImplementedError("DeviceResizeCenterCrop: size=%r is not implemented (the kernels write 224 x 224)" % (size,))
        if getattr(interpolation, "value", interpolation) not in (BICUBIC, "bicubic"):
            raise NotImplementedError("DeviceResizeCenterCrop: interpolation=%r is not implemented (3 = bicubic only)" % (interpolation,))
        if int(resize) != resize or resize < OUT:
            raise ValueError("DeviceResizeCenterCrop: resize is an integer >= %d (the window must fit), got %r" % (OUT, resize))
        self.resize, self.size, self.any_scale = int(resize), OUT, bool(any_scale)

    def geometry(self, height, width):
        """(full_h, full_w, off_y, off_x)"""
        if width <= height:
            fw, fh = self.resize, int(self.resize * height / width)
        else:
            fh, fw = self.resize, int(self.resize * width / height)
        return fh, fw, int(round((fh - OUT) / 2.0)), int(round((fw - OUT) / 2.0))

    def draw_for(self, sizes):
        rows = []
        for (sh, sw) in _sizes_list(sizes):
            fh, fw, oy, ox = self.geometry(sh, sw)
            rows.append((sh, sw, 0, 0, sh, sw, fh, fw, oy, ox, 0))
        return CropDraw(rows, wide=self.any_scale)


class DeviceResize(_DeviceCrop):
    """``Resize((224, 224), interpolation=3)`` of torchvision, the reference's pipeline without augmentation (datasets/image_datasets_noaug.py,
    train and val): the whole image resized to 224 x 224, each axis with its own scale factor.  Makes no draw.  ``any_scale``: wide draws
    (csrc/resample_wide.h), so a side above 560 is taken."""

    def __init__(self, size=(OUT, OUT), interpolation=3, any_scale=False):
        if not isinstance(size, (tuple, list)) or tuple(size) != (OUT, OUT):   # an int is torchvision's short-side rule: DeviceResizeCenterCrop's
            raise NotImplementedError("DeviceResize: size=%r is not implemented ((224, 224) only: the kernels write 224 x 224)" % (size,))
        if getattr(interpolation, "value", interpolation) not in (BICUBIC, "bicubic"):
            raise NotImplementedError("DeviceResize: interpolation=%r is not implemented (3 = bicubic only)" % (interpolation,))
        self.size, self.interpolation, self.any_scale = (OUT, OUT), BICUBIC, bool(any_scale)

    def draw_for(self, sizes):
        return CropDraw([(sh, sw, 0, 0, sh, sw, OUT, OUT, 0, 0, 0) for (sh, sw) in _sizes_list(sizes)], wide=self.any_scale)


def probe_draw(sizes, wide=False):
    """A valid draw that consumes no random number (the top-left 224 x 224 of every image, or the whole of a smaller one): for the loop's
    one-off stream probe, which needs a batch of the step's shape and must leave the generators alone.  ``wide``: a wide draw, so that the
    probe of an ``any_scale`` loop takes the launches its steps take."""
    return CropDraw([(sh, sw, 0, 0, min(sh, OUT), min(sw, OUT), OUT, OUT, 0, 0, 0) for (sh, sw) in _sizes_list(sizes)], wide=wide)


def pad_collate(batch, pad_to=None):
    """collate_fn of a loader that decodes only: a list of ``(image, label)`` with ``image`` an HWC uint8 array / tensor [h, w, 3] ->
    ``((pixels uint8 [B, Hs, Ws, 3], sizes int32 [B, 2]), labels int64 [B])``.  Hs, Ws = the largest height and width of the batch (or
    ``pad_to`` = (Hs, Ws), which keeps the shape the same from batch to batch); the padding is zeros and never reaches an output."""
    import numpy as np
    import torch
    images = [np.asarray(b[0]) for b in batch]
    for im in images:
        if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
            raise ValueError("pad_collate takes HWC uint8 images [h, w, 3] (got %s %s)" % (im.dtype, im.shape))
        if im.shape[0] < 1 or im.shape[1] < 1 or im.shape[0] > MAX_SIDE or im.shape[1] > MAX_SIDE:
            raise ValueError("pad_collate: an image of %d x %d (sides are 1 to %d)" % (im.shape[0], im.shape[1], MAX_SIDE))
    hs, ws = max(im.shape[0] for im in images), max(im.shape[1] for im in images)
    if pad_to is not None:
        if pad_to[0] < hs or pad_to[1] < ws:
            raise ValueError("pad_collate: pad_to=%r is smaller than an image of the batch (%d x %d)" % (tuple(pad_to), hs, ws))
        hs, ws = int(pad_to[0]), int(pad_to[1])
    pixels = torch.zeros(len(images), hs, ws, 3, dtype=torch.uint8)
    for i, im in enumerate(images):
        pixels[i, :im.shape[0], :im.shape[1]] = torch.from_numpy(np.ascontiguousarray(im))
    sizes = torch.tensor([[im.shape[0], im.shape[1]] for im in images], dtype=torch.int32)
    labels = torch.as_tensor([int(b[1]) for b in batch], dtype=torch.int64)
    return (pixels, sizes), labels


# ---- clips: the video loaders' spatial pipeline (csrc/resample_clip.h, csrc/resample_clip.hip) ---------------------------------------------
def full_clip_sizes(clips):
    """The sizes of a bare clip batch [B, T, Hs, Ws, 3] that every clip fills."""
    return [(int(clips.shape[2]), int(clips.shape[3]))] * int(clips.shape[0])


def _refuse_clip_options(name, size, interpolation):
    if isinstance(size, (tuple, list)):
        size = size[0] if len(size) == 1 or (len(size) == 2 and size[0] == size[1]) else size
    if size != OUT:
        raise NotImplementedError("%s: size=%r is not implemented (the kernel writes 224 x 224)" % (name, size))
    if interpolation not in ("bilinear", BILINEAR_F32):
        raise NotImplementedError("%s: interpolation=%r is not implemented (torch's 'bilinear' only)" % (name, interpolation))


class _DeviceClipCrop:
    """What the three clip classes share: ``draw_for(sizes)`` gives a CropDraw of clip rows -- ``views`` rows per source clip, in the
    clips' order -- and ``obj(clips, sizes)`` the resampled float batch of a device batch of byte clips."""
    views = 1

    def inject(self, draws):
        """Fixed draws (CropDraw objects of clip rows) that the next calls of ``draw_for()`` hand out in order: for tests and recorded runs."""
        self._injected.extend(draws)
        return self

    def draw_for(self, sizes):
        sizes = _sizes_list(sizes)
        if getattr(self, "_injected", None):
            d = self._injected.pop(0)
            if not d.clip or d.units != len(sizes) * self.views:
                raise ValueError("resample: the injected draw holds %d %s rows, the batch needs %d clip rows" % (
                    d.units, "clip" if d.clip else "image", len(sizes) * self.views))
            return d
        rows = []
        for i, (sh, sw) in enumerate(sizes):
            for (top, left, bh, bw, fh, fw, oy, ox, flags) in self.rows_for(sh, sw):
                rows.append((sh, sw, top, left, bh, bw, fh, fw, oy, ox, flags, i))
        return CropDraw(rows, filter=BILINEAR_F32)

    def __call__(self, clips, sizes=None, norm=None):
        """fp32 [units, 3, T, 224, 224] (a permuted view of the kernel's [units, T, 3, 224, 224]) of a device batch uint8
        [B, T, Hs, Ws, 3]; ``sizes`` [B, 2] (host) = the clips' valid (height, width), None: every clip fills the batch's shape;
        ``norm`` = (mean, std), None: the ImageNet statistics."""
        from _lib import resample_clip_f32
        import torch
        d = self.draw_for(full_clip_sizes(clips) if sizes is None else sizes)
        if d.units != int(clips.shape[0]) * self.views:
            raise ValueError("resample: %d rows for a batch of %d clips with %d view(s)" % (d.units, int(clips.shape[0]), self.views))
        table = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(clips.device)
        return resample_clip_f32(clips, table, d, norm=norm)


class DeviceClipScaleJitterCrop(_DeviceClipCrop):
    """The K400 train path of the reference (video_datasets/k400.py with resize_type='random_short_side_scale_jitter'):
    ``random_short_side_scale_jitter(frames, round(size * scale_range[0]), round(size * scale_range[1]))``, ``random_crop(frames, size)``
    and the mirror, per clip in the reference's order:

        1. ``np.random.uniform(min_size, max_size)`` -> ``int(round(.))``: the short side of the resized clip (a clip whose short side
           already has that length is left as it is); the long side is ``int(math.floor(float(long) / short * size))``
        2. ``np.random.randint(0, full_h - 224)`` only if ``full_h > 224``, then the same for the width (exclusive upper bound, as there)
        3. ``torch.rand(1).item() < mirror`` (``mirror=None``: no mirror stage, no draw)

    ``np_rng`` (a numpy RandomState; None: numpy's global one) and ``generator`` (a torch.Generator; None: torch's global one)."""

    def __init__(self, size=224, scale_range=(1.0, 1.15), mirror=0.5, interpolation="bilinear", np_rng=None, generator=None):
        _refuse_clip_options("DeviceClipScaleJitterCrop", size, interpolation)
        if len(scale_range) != 2 or not (1.0 <= scale_range[0] <= scale_range[1]):
            raise ValueError("DeviceClipScaleJitterCrop: scale_range is (min, max) with 1 <= min <= max (the window must fit)")
        if mirror is not None and not (0.0 <= float(mirror) <= 1.0):
            raise ValueError("DeviceClipScaleJitterCrop: mirror is a probability or None")
        self.size, self.scale_range, self.mirror, self.np_rng, self.generator = OUT, tuple(scale_range), mirror, np_rng, generator
        self.min_size, self.max_size = round(OUT * scale_range[0]), round(OUT * scale_range[1])
        self._injected = []

    def rows_for(self, height, width):
        import numpy as np
        import torch
        rng = np.random if self.np_rng is None else self.np_rng
        size = int(round(rng.uniform(self.min_size, self.max_size)))
        if (width <= height and width == size) or (height <= width and height == size):
            fh, fw = height, width
        elif width < height:
            fh, fw = int(math.floor((float(height) / width) * size)), size
        else:
            fh, fw = size, int(math.floor((float(width) / height) * size))
        oy, ox = 0, 0
        if not (fh == OUT and fw == OUT):
            if fh > OUT:
                oy = int(rng.randint(0, fh - OUT))
            if fw > OUT:
                ox = int(rng.randint(0, fw - OUT))
        mirror = self.mirror is not None and torch.rand(1, generator=self.generator).item() < self.mirror
        return [(0, 0, height, width, fh, fw, oy, ox, FLAG_MIRROR if mirror else 0)]


class DeviceClipRandomResizedCrop(_DeviceClipCrop):
    """The SSV2 train path of the reference (resize_type='random_resized_crop'): ``random_resized_crop(frames, 224, 224, scale)``, whose box
    is ``_get_param_spatial_crop(scale, ratio, height, width)`` restated line by line -- per attempt ``random.uniform(*scale)``,
    ``random.uniform(*log_ratio)`` and an ``np.random.uniform()`` that is drawn on EVERY attempt (its ``switch_hw`` is off, the draw is
    made all the same), then ``random.randint`` twice; ten attempts, then the central fallback.  The box is resized to 224 x 224.
    ``py_rng`` (a random.Random; None: the ``random`` module) and ``np_rng`` (a numpy RandomState; None: numpy's global one)."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation="bilinear", py_rng=None, np_rng=None):
        _refuse_clip_options("DeviceClipRandomResizedCrop", size, interpolation)
        if len(scale) != 2 or len(ratio) != 2 or not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
            raise ValueError("DeviceClipRandomResizedCrop: scale and ratio are (min, max) with 0 < min <= max")
        self.size, self.scale, self.ratio, self.py_rng, self.np_rng = OUT, tuple(scale), tuple(ratio), py_rng, np_rng
        self._injected = []

    def get_params(self, height, width, num_repeat=10):
        """(i, j, h, w): the reference's ``_get_param_spatial_crop`` with log_scale=True, switch_hw=False."""
        import random
        import numpy as np
        rnd = random if self.py_rng is None else self.py_rng
        rng = np.random if self.np_rng is None else self.np_rng
        scale, ratio = self.scale, self.ratio
        for _ in range(num_repeat):
            area = height * width
            target_area = rnd.uniform(*scale) * area
            log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
            aspect_ratio = math.exp(rnd.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            rng.uniform()   # `np.random.uniform() < 0.5 and switch_hw`: consumed whatever switch_hw says
            if 0 < w <= width and 0 < h <= height:
                i = rnd.randint(0, height - h)
                j = rnd.randint(0, width - w)
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w = width
            h = height
        i = (height - h) // 2
        j = (width - w) // 2
        return i, j, h, w

    def rows_for(self, height, width):
        i, j, h, w = self.get_params(height, width)
        return [(i, j, h, w, OUT, OUT, 0, 0, 0)]


class DeviceClipUniformCrop(_DeviceClipCrop):
    """The reference's evaluation path: the short side becomes 224 and the long side ``long * 224 // short`` (k400.py's val resize), then
    ``_generate_spatial_crops``: one view at ``(full - 224) // 2`` of both axes, or three views at ``0, margin // 2, margin`` along the long
    axis.  The rows of a clip's views share its ``src`` and follow each other, so a batch of B clips gives units [B * views] in the order
    ``sum([spatial_crops(clip) for clip in clips], [])``.  Makes no draw."""

    def __init__(self, size=224, spatial_views=1, interpolation="bilinear"):
        _refuse_clip_options("DeviceClipUniformCrop", size, interpolation)
        if spatial_views not in (1, 3):
            raise NotImplementedError("DeviceClipUniformCrop: spatial_views=%r is not implemented (1 or 3, as the reference)" % (spatial_views,))
        self.size, self.views = OUT, int(spatial_views)
        self._injected = []

    def geometry(self, height, width):
        """(full_h, full_w)"""
        if height < width:
            return OUT, width * OUT // height
        return height * OUT // width, OUT

    def rows_for(self, height, width):
        fh, fw = self.geometry(height, width)
        if self.views == 1:
            return [(0, 0, height, width, fh, fw, (fh - OUT) // 2, (fw - OUT) // 2, 0)]
        margin = max(fh, fw) - OUT
        if fh > fw:
            return [(0, 0, height, width, fh, fw, st, 0, 0) for st in (0, margin // 2, margin)]
        return [(0, 0, height, width, fh, fw, 0, st, 0) for st in (0, margin // 2, margin)]


def probe_clip_draw(sizes):
    """A valid clip draw that consumes no random number (see ``probe_draw``)."""
    return CropDraw([(sh, sw, 0, 0, min(sh, OUT), min(sw, OUT), OUT, OUT, 0, 0, 0, i) for i, (sh, sw) in enumerate(_sizes_list(sizes))],
                    filter=BILINEAR_F32)


def pad_collate_clips(batch, pad_to=None):
    """collate_fn of a video loader that decodes only: a list of ``(clip, label)`` with ``clip`` a THWC uint8 array / tensor [T, h, w, 3],
    as a decoder yields it -> ``((clips uint8 [B, T, Hs, Ws, 3], sizes int32 [B, 2]), labels int64 [B])``.  Every clip has the same T;
    Hs, Ws = the largest height and width of the batch (or ``pad_to`` = (Hs, Ws)); the padding is zeros and never reaches an output."""
    import numpy as np
    import torch
    clips = [np.asarray(b[0]) for b in batch]
    for cl in clips:
        if cl.ndim != 4 or cl.shape[3] != 3 or cl.dtype != np.uint8:
            raise ValueError("pad_collate_clips takes THWC uint8 clips [T, h, w, 3] (got %s %s)" % (cl.dtype, cl.shape))
        if cl.shape[0] < 1 or cl.shape[0] != clips[0].shape[0]:
            raise ValueError("pad_collate_clips: clips of %d and %d frames in one batch" % (clips[0].shape[0], cl.shape[0]))
        if cl.shape[1] < 1 or cl.shape[2] < 1 or cl.shape[1] > MAX_SIDE or cl.shape[2] > MAX_SIDE:
            raise ValueError("pad_collate_clips: a clip of %d x %d (sides are 1 to %d)" % (cl.shape[1], cl.shape[2], MAX_SIDE))
    if not clips:
        raise ValueError("pad_collate_clips: an empty batch")
    hs, ws = max(cl.shape[1] for cl in clips), max(cl.shape[2] for cl in clips)
    if pad_to is not None:
        if pad_to[0] < hs or pad_to[1] < ws:
            raise ValueError("pad_collate_clips: pad_to=%r is smaller than a clip of the batch (%d x %d)" % (tuple(pad_to), hs, ws))
        hs, ws = int(pad_to[0]), int(pad_to[1])
    out = torch.zeros(len(clips), clips[0].shape[0], hs, ws, 3, dtype=torch.uint8)
    for i, cl in enumerate(clips):
        out[i, :, :cl.shape[1], :cl.shape[2]] = torch.from_numpy(np.ascontiguousarray(cl))
    sizes = torch.tensor([[cl.shape[1], cl.shape[2]] for cl in clips], dtype=torch.int32)
    labels = torch.as_tensor([int(b[1]) for b in batch], dtype=torch.int64)
    return (out, sizes), labels
