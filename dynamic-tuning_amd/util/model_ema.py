"""Model EMA on the device: ``DeviceModelEma`` stands where ``timm.utils.ModelEmaV2`` stands in a DeiT-style recipe
(``model_ema = ModelEmaV2(model, decay)`` after the model is built, ``model_ema.update(model)`` after every optimizer update,
``evaluate(loader, model_ema.module, ...)``).

timm deep-copies the module.  That cannot be done here: the module owns a library context with a multi-GB arena, and its trainable
tensors are views into ONE flat device buffer (``DyTEngine.flat``) that the step reads by pointer.  So the averaged model is one more
flat buffer in the engine's trainable layout -- the *shadow*, ~1.3 M floats -- moved by one elementwise launch (C ABI dyt_ema_update):

    shadow = decay * shadow + (1. - decay) * flat        three fp32 roundings, torch's ``ema_v.copy_(decay * ema_v + (1. - decay) * model_v)``

and ``module`` is an evaluation view that runs the model's own context with the shadow as the ``trainable`` buffer of the pass.  Frozen
tensors are not averaged: they are identical by definition.

The shadow starts as a copy of the trainable tensors as they are at construction (timm's deepcopy semantics; the drivers construct the
object before any engine exists) and is homed into the flat layout at the first ``update()`` / view call; like the moments of
``engine_finetune.FusedAdamW`` it survives a re-created engine (batch growth, device move).  The snapshot, the decay schedule and the
state-dict bookkeeping work on CPU tensors without the library.
"""
import math
import weakref

import torch
import torch.distributed as dist

from _lib import DyTError, is_trainable_param, key_to_param


def decay_at(decay, updates):
    """The decay of update number ``updates`` (0-based): ``decay`` itself, or ``decay(updates)`` for a callable -- a warm-up schedule, or
    ``lambda n: n / (n + 1.)`` for the equal-weight average.  A finite value in [0, 1], else ValueError."""
    d = decay(int(updates)) if callable(decay) else decay
    try:
        d = float(d)
    except (TypeError, ValueError):
        raise ValueError("model EMA: decay %r is not a number (update %d)" % (d, updates))
    if not (math.isfinite(d) and 0.0 <= d <= 1.0):
        raise ValueError("model EMA: decay %r is outside [0, 1] (update %d)" % (d, updates))
    return d


def _trainable_names(model):
    return [(n, p) for n, p in model.named_parameters() if is_trainable_param(key_to_param(n)[0])]


class _EvalView:
    """``DeviceModelEma.module``: the model with the shadow in place of its trainable tensors, for eval forwards.  ``forward`` /
    ``forward_features`` run the model's own context on the shadow; every other attribute (``prepare_input``, ``takes_bytes``,
    ``_engine``, ``input_norm`` ...) is the model's, read and written."""

    def __init__(self, ema):
        object.__setattr__(self, "_ema", ema)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_ema").model, name)

    def __setattr__(self, name, value):
        setattr(self._ema.model, name, value)

    def eval(self):
        self._ema.model.eval()
        return self

    def train(self, mode=True):
        self._ema.model.train(mode)
        return self

    def _check(self, what):
        if self._ema.model.training or torch.is_grad_enabled():
            raise DyTError("model EMA: %s of the averaged model is an eval forward -- call .eval() and run it under torch.no_grad() "
                           "(the shadow is moved by update() alone and carries no gradient)" % what)

    def forward(self, x, complete_model=False, gumbel=None, keep_mask=None):
        self._check("forward")
        return self._ema.model._forward(x, complete_model=complete_model, gumbel=gumbel, keep_mask=keep_mask, trainable=self._ema.buffer)

    __call__ = forward

    def forward_features(self, x, complete_model=False, gumbel=None, keep_mask=None, out_indices=None):
        self._check("forward_features")
        return self._ema.model._forward_features(x, complete_model=complete_model, gumbel=gumbel, keep_mask=keep_mask, out_indices=out_indices,
                                                 trainable=self._ema.buffer)


class DeviceModelEma:
    """``DeviceModelEma(model, decay=0.9998)``.  ``decay``: a float, or a callable ``updates -> float`` evaluated on the host before each
    update (``updates`` is 0-based).  ``update()``: one launch on the current stream against the model's engine, then ``updates += 1``;
    call it after every optimizer update (``train_one_epoch`` does with ``args.model_ema``), whether or not the overflow guard skipped
    that update -- the shadow then moves toward the unchanged parameters, as ``model_ema.update(model)`` after ``loss_scaler(...)`` does."""

    def __init__(self, model, decay=0.9998):
        self.model = getattr(model, "module", model)
        self.decay = decay
        decay_at(decay, 0)   # a bad constant (or a schedule that starts badly) is refused here
        self.updates = 0
        self._names = [(n, tuple(p.shape)) for n, p in _trainable_names(self.model)]
        if not self._names:
            raise DyTError("model EMA: the model has no trainable tensor (adapters, gates, head)")
        # the snapshot (later: a loaded state) tensor by tensor, until an engine exists to home it into
        self._host = {n: p.detach().to(torch.float32).clone() for n, p in _trainable_names(self.model)}
        self.shadow = None      # flat fp32 buffer in the layout of the engine it was homed into
        self._engine = None     # weak: a context the model has dropped (batch growth) must not be kept alive by its average
        self._slices = None     # name -> (offset, numel) in that engine
        self._synced = False    # the once-only broadcast from rank 0 has run
        self.module = _EvalView(self)

    # ---- the flat buffer -------------------------------------------------------------------------
    def _tensors(self):
        """The averaged tensors by name: views of the shadow, or the tensors waiting for an engine."""
        if self.shadow is None:
            return self._host
        return {n: self.shadow[self._slices[n][0]:self._slices[n][0] + self._slices[n][1]].view(shape) for n, shape in self._names}

    def buffer(self, eng=None):
        """The shadow as a flat buffer in ``eng``'s trainable layout (default: the model's current engine), homed / re-homed when the
        engine is new.  Padding words between tensors are zero, as in the engine's own buffer."""
        eng = self.model._engine if eng is None else eng
        if eng is None:
            raise DyTError("model EMA: the model has no engine yet (run a forward / step first)")
        if self.shadow is not None and self._engine is not None and self._engine() is eng:
            return self.shadow
        src = self._tensors()
        new = torch.zeros(eng.n_train, device=eng.device, dtype=torch.float32)
        slices = {}
        for n, shape in self._names:
            off, num = eng.trainable_slice(n)
            if num != src[n].numel():
                raise DyTError("model EMA: %s holds %d elements, the engine's slice %d" % (n, src[n].numel(), num))
            new[off:off + num].copy_(src[n].reshape(-1))
            slices[n] = (off, num)
        self.shadow, self._engine, self._slices, self._host = new, weakref.ref(eng), slices, None
        return new

    def update(self):
        eng = self.model._engine
        if eng is None:
            raise DyTError("model EMA: update() before any forward / step of the model")
        d = decay_at(self.decay, self.updates)
        shadow = self.buffer(eng)
        if not self._synced:
            # ranks seed their head initialisation differently and FusedAdamW.sync_parameters aligns the PARAMETERS at the first step only:
            # every rank starts from rank 0's shadow.  Once: identical parameters give identical shadows from here on.
            if dist.is_available() and dist.is_initialized():
                dist.broadcast(shadow, src=0)
            self._synced = True
        eng.ema_update(shadow, d)
        self.updates += 1

    # ---- checkpoints -----------------------------------------------------------------------------
    def state_dict(self, full=False):
        """The averaged tensors under the reference's parameter names (copies).  Default: the trainable tensors alone (~5 MB).
        ``full=True``: the whole model's state dict with the averaged tensors substituted -- what ``load_state_dict`` of this model, of an
        inference-only model or of the reference's model takes."""
        avg = {n: t.detach().clone() for n, t in self._tensors().items()}
        if not full:
            return avg
        out = {}
        for k, v in self.model.state_dict().items():
            out[k] = avg[k].to(v.device).view(v.shape) if k in avg else v.detach().clone()
        return out

    def load_state_dict(self, sd):
        """Either form of ``state_dict``.  Held tensor by tensor until an engine exists (the next ``update()`` / view call homes it)."""
        host = {}
        for n, shape in self._names:
            if n not in sd:
                raise KeyError("model EMA state has no %s" % n)
            if tuple(sd[n].shape) != shape:
                raise ValueError("model EMA state of %s has shape %s, the parameter has %s" % (n, tuple(sd[n].shape), shape))
            host[n] = sd[n].detach().to(torch.float32).clone()
        self._host, self.shadow, self._engine, self._slices = host, None, None, None
