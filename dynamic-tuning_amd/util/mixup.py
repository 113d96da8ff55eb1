"""Mixup / CutMix on the device: ``DeviceMixup`` stands where ``timm.data.Mixup`` stands in the reference's drivers (main_image.py:
``mixup_fn = Mixup(...)``, engine_finetune.py:44-45).

This is a RESTATEMENT of timm 0.9.12's ``Mixup`` in ``mode='batch'`` with ``correct_lam=True`` (timm is not a dependency): one draw per
batch on the host, image n pairs with ``x.flip(0)[n]``, targets ``lam t(y) + (1 - lam) t(y.flip(0))`` with the smoothed one-hot rows ``t``.
The draws come from a ``numpy.random.Generator`` (timm uses numpy's global legacy state), in this order:

    1. ``u = random()``; the batch is mixed iff ``u < prob`` (else lam = 1: identity)
    2. both alphas > 0 only: ``random() < switch_prob`` chooses cutmix
    3. ``lam = beta(alpha, alpha)`` with the chosen mode's alpha
    4. cutmix only: ``cy = integers(0, 224)``, then ``cx = integers(0, 224)``; box and corrected lam as ``rand_bbox`` / ``correct_lam``

Two ways to use it:
  * ``train_one_epoch(..., mixup_fn=DeviceMixup(...))`` recognises the class: it draws, hands the draw to the engine (``set_mix``) and
    passes the UNMIXED batch (bytes stay bytes) with its INTEGER labels to the fused step, which mixes inside the patch-embedding load
    and writes the class-probability targets itself; hipGraph replay stays on.
  * ``mixed, soft = DeviceMixup(...)(x, target)`` on device tensors is a drop-in ``mixup_fn`` for any other loop (libdyt_hip's
    dyt_mix_images / dyt_mix_targets; fp32 images out).
"""
import math
import struct

import numpy as np

IMG = 224
IDENTITY, MIXUP, CUTMIX = 0, 1, 2


def rand_box(lam, cy, cx):
    """timm's rand_bbox for a 224 x 224 image with the centre already drawn: (yl, yh, xl, xh)."""
    ratio = math.sqrt(1.0 - lam)
    cut_h, cut_w = int(IMG * ratio), int(IMG * ratio)
    clip = lambda v: min(max(v, 0), IMG)   # noqa: E731
    return clip(cy - cut_h // 2), clip(cy + cut_h // 2), clip(cx - cut_w // 2), clip(cx + cut_w // 2)


def corrected_lam(box):
    yl, yh, xl, xh = box
    return 1.0 - (yh - yl) * (xh - xl) / float(IMG * IMG)


class MixDraw:
    """The host-side parameters of one batch: ``mode`` (0 identity, 1 mixup, 2 cutmix), ``lam`` (a Python float; for cutmix the corrected
    one), ``box`` = (yl, yh, xl, xh), and the target row's ``smoothing`` / ``num_classes`` (filled in by the DeviceMixup that hands the draw
    out).  ``words()`` is the 64-byte block the kernels read (csrc/mix.h MixParams)."""

    def __init__(self, mode, lam=1.0, box=(0, 0, 0, 0), smoothing=0.0, num_classes=None):
        self.mode, self.lam, self.box = int(mode), float(lam), tuple(int(v) for v in box)
        self.smoothing, self.num_classes = float(smoothing), num_classes
        self.check()

    @classmethod
    def identity(cls):
        return cls(IDENTITY, 1.0)

    @classmethod
    def mixup(cls, lam):
        return cls(IDENTITY if float(lam) == 1.0 else MIXUP, lam)

    @classmethod
    def cutmix(cls, box):
        """A cutmix draw from its box; lam is the corrected one."""
        return cls(CUTMIX, corrected_lam(box), box)

    @classmethod
    def cutmix_from(cls, lam, cy, cx):
        """A cutmix draw as timm makes it: lam from the Beta draw, the centre from randint."""
        return cls.cutmix(rand_box(float(lam), int(cy), int(cx)))

    def check(self):
        """The refusals of csrc/mix.h (mix_mode_error, mix_lam_error, mix_box_error), made where the values are still on the host."""
        if self.mode not in (IDENTITY, MIXUP, CUTMIX):
            raise ValueError("mix: mode is 0 (identity), 1 (mixup) or 2 (cutmix), got %r" % (self.mode,))
        if not 0.0 <= self.lam <= 1.0:   # (false for NaN)
            raise ValueError("mix: lam outside [0, 1]: %r" % (self.lam,))
        yl, yh, xl, xh = self.box
        if yl < 0 or xl < 0 or yh > IMG or xh > IMG:
            raise ValueError("mix: the cutmix box %r lies outside the 224 x 224 image" % (self.box,))
        if yl > yh or xl > xh:
            raise ValueError("mix: the cutmix box %r is reversed" % (self.box,))
        if self.mode == IDENTITY and self.lam != 1.0:
            raise ValueError("mix: the identity draw has lam = 1")

    def with_targets(self, smoothing, num_classes):
        return MixDraw(self.mode, self.lam, self.box, smoothing, num_classes)

    def words(self, criterion_smoothing=0.0):
        """MixParams as 64 bytes.  Every float is the double expression rounded once to fp32, as torch rounds a Python scalar."""
        if self.num_classes is None or int(self.num_classes) < 1:
            raise ValueError("mix: num_classes < 1")
        C, e = int(self.num_classes), float(criterion_smoothing or 0.0)
        off = self.smoothing / C
        on = 1.0 - self.smoothing + off
        return struct.pack("<iff4iffiff4i", self.mode, self.lam, 1.0 - self.lam, *self.box, on, off,
                           1 if e > 0.0 else 0, 1.0 - e, e / C, 0, 0, 0, 0)

    def __repr__(self):
        return "MixDraw(mode=%d, lam=%r, box=%r, smoothing=%r, num_classes=%r)" % (self.mode, self.lam, self.box, self.smoothing, self.num_classes)


class DeviceMixup:
    """timm.data.Mixup's signature (plus ``generator``: a numpy.random.Generator or a seed).  Only what the fused kernels implement is
    accepted: ``mode='batch'``, ``correct_lam=True``, no ``cutmix_minmax``."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000, generator=None):
        if mode != 'batch':
            raise NotImplementedError("DeviceMixup: mode=%r (only 'batch': one draw per batch)" % (mode,))
        if cutmix_minmax is not None:
            raise NotImplementedError("DeviceMixup: cutmix_minmax is not implemented")
        if not correct_lam:
            raise NotImplementedError("DeviceMixup: correct_lam=False is not implemented")
        if not (mixup_alpha > 0. or cutmix_alpha > 0.):
            raise ValueError("DeviceMixup: one of mixup_alpha > 0., cutmix_alpha > 0. must be true")
        if int(num_classes) < 1:
            raise ValueError("DeviceMixup: num_classes < 1")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.switch_prob = float(prob), float(switch_prob)
        self.label_smoothing, self.num_classes = float(label_smoothing), int(num_classes)
        self.mode, self.correct_lam, self.cutmix_minmax = mode, True, None
        self.mixup_enabled = True   # timm's switch: False makes every batch an identity draw
        self.rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
        self._injected = []

    def inject(self, draws):
        """Fixed draws (MixDraw objects) that the next calls of ``draw()`` hand out in order, before the generator is asked again: for
        tests and comparisons against recorded runs."""
        self._injected.extend(draws)
        return self

    def draw(self):
        """The host-side parameters of the next batch (see the module text for the order of the random draws)."""
        if self._injected:
            return self._injected.pop(0).with_targets(self.label_smoothing, self.num_classes)
        d = MixDraw.identity()
        if self.mixup_enabled and self.rng.random() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                cut = bool(self.rng.random() < self.switch_prob)
            else:
                cut = not self.mixup_alpha > 0.
            alpha = self.cutmix_alpha if cut else self.mixup_alpha
            lam = float(self.rng.beta(alpha, alpha))
            if cut:
                cy = int(self.rng.integers(0, IMG))
                cx = int(self.rng.integers(0, IMG))
                d = MixDraw.cutmix_from(lam, cy, cx)
            else:
                d = MixDraw.mixup(lam)
        return d.with_targets(self.label_smoothing, self.num_classes)

    def __call__(self, x, target, norm=None):
        """(mixed fp32 images, class-probability targets [rows, num_classes]) of device tensors.  ``x``: fp32 or uint8 images
        [n,3,224,224] / uint8 [n,224,224,3], or clips [b,3,t,224,224] / uint8 [b,t,224,224,3] (frame f of clip b pairs with frame f of
        clip nb-1-b; fp32 clips come back as [b,3,t,224,224]).  ``norm`` = (mean, std) of uint8 input (the model's ``input_norm``)."""
        import torch
        from _lib import mix_images, mix_targets
        d = self.draw()
        params = torch.frombuffer(bytearray(d.words()), dtype=torch.int32).to(x.device)
        frames, clips = 1, None
        if x.dim() == 5:
            clips = x.shape[0]
            if x.dtype == torch.uint8 and tuple(x.shape[2:]) == (IMG, IMG, 3):
                frames = x.shape[1]
                x = x.reshape(clips * frames, IMG, IMG, 3)
            else:
                frames = x.shape[2]
                x = x.permute(0, 2, 1, 3, 4).reshape(clips * frames, 3, IMG, IMG)
        mixed = mix_images(x.contiguous(), params, frames=frames, norm=norm)
        if clips is not None:
            mixed = mixed.reshape(clips, frames, 3, IMG, IMG).permute(0, 2, 1, 3, 4)
        return mixed, mix_targets(target, self.num_classes, params)
