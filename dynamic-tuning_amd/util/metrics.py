"""Top-k and mean-per-class accuracy (reference util/metrics.py:4-25); host-side bookkeeping on
the gathered [n,C] predictions, not part of the device hot path."""
import torch


def accuracy(output, target, topk=(1,)):
    """Percentage of rows whose label is among the k best-scored classes, one 0-dim tensor per k (the return contract of the
    reference's accuracy(), util/metrics.py:4-11, which engine_finetune.evaluate reads as acc1 / acc5)."""
    n = target.shape[0]
    kmax = min(max(topk), output.shape[1])
    ranked = output.topk(kmax, dim=1).indices                       # [n, kmax], best first (ties: lowest index, as torch.topk)
    hit_rank = (ranked == target.reshape(n, 1)).float().cumsum(1)  # hit_rank[i, j] = 1 iff the label is among the j+1 best
    return [hit_rank[:, min(k, kmax) - 1].sum() * 100.0 / n for k in topk]   # (x 100, then / n: the golden accuracy is compared to the last fp32 bit)


def mean_per_class_accuracy(pred, target, num_classes):
    """Mean over the classes of (correct top-1 predictions of the class / samples of the class), in per cent; a class without samples counts
    as 0 (the VTAB metric of the reference, util/metrics.py:14-25)."""
    top1 = pred.topk(1, dim=-1).indices.reshape(-1)
    per_class_hits = torch.bincount(target[top1 == target], minlength=num_classes)
    per_class_total = torch.bincount(target, minlength=num_classes)
    return (per_class_hits / per_class_total.clamp(min=1).float() * 100).mean(0)


class StreamingEval:
    """The evaluation statistics as a fixed-size device-resident state (csrc/eval_stats.h): ``update`` folds one batch of logits, labels and
    token masks into it with three HIP launches and no host synchronisation, ``result`` reads it once.  Nothing per-sample is kept, so
    memory does not grow with the dataset, and the state is additive: ranks merge with a SUM all-reduce of ``counts`` (a few KB plus 2 C
    words) and of the loss word.

    Where this differs from ``accuracy`` / ``mean_per_class_accuracy`` on gathered tensors: a label outside [0, C) makes its row *ignored*
    (counted in ``ignored``, excluded from everything else) instead of raising or miscounting; a row holding a NaN is counted, is a miss at
    every k and stays out of the loss (``nan_rows``); the tie order is defined -- rank = #{x_j > x_t} + #{j < t : x_j == x_t}, the lowest
    index first, what ``accuracy`` documents -- and not the device-dependent order of torch.topk."""

    def __init__(self, num_classes, layers=12, tokens=196, device="cuda"):
        import _lib
        self.num_classes, self.layers, self.tokens = int(num_classes), int(layers), int(tokens)
        self.device = torch.device(device)
        self.counts = torch.zeros(_lib.eval_counts_words(layers, tokens), dtype=torch.int64, device=self.device)
        self.per_class = torch.zeros(2 * self.num_classes, dtype=torch.int64, device=self.device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._rank = torch.empty(0, dtype=torch.int32, device=self.device)   # per-row scratch, regrown when a larger batch arrives
        self._loss = torch.empty(0, dtype=torch.float32, device=self.device)
        self._rows = 0

    # ---- the device path ----------------------------------------------------------------------------------------------------------------
    def update(self, logits, target, token_select=None):
        """One batch: fp32 logits [n, C] (any row stride), integer labels [n], optionally fp32 masks [n, L, T] or [n, L, T, 1]."""
        import _lib
        if not (torch.is_tensor(logits) and logits.is_cuda and torch.is_tensor(target) and target.is_cuda):
            raise _lib.DyTError("StreamingEval.update takes device tensors (there is no CPU path)")
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise _lib.DyTError("StreamingEval(num_classes=%d).update got logits %s" % (self.num_classes, tuple(logits.shape)))
        n = int(logits.shape[0])
        if self._rank.numel() < n:
            self._rank = torch.empty(n, dtype=torch.int32, device=self.device)
            self._loss = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.eval_rows(logits, target, self.counts, self.per_class, self.loss_sum, self._rank, self._loss)
        self._rows = n
        if token_select is not None:
            _lib.eval_keep(token_select, self.counts, self.layers, self.tokens)

    @property
    def last_rank(self):
        """int32 [n]: the latest update's ranks (-1 ignored, C for a NaN row); valid until the next update."""
        return self._rank[:self._rows]

    @property
    def last_loss(self):
        """fp32 [n]: the latest update's row losses (0 for an ignored or NaN row); valid until the next update."""
        return self._loss[:self._rows]

    def all_reduce(self, group=None):
        """One SUM all-reduce of the counts (head, histograms and per-class words as one buffer) and one of the loss word."""
        import torch.distributed as dist
        flat = torch.cat([self.counts, self.per_class])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        self.counts.copy_(flat[:self.counts.numel()])
        self.per_class.copy_(flat[self.counts.numel():])
        dist.all_reduce(self.loss_sum, op=dist.ReduceOp.SUM, group=group)
        return self

    # ---- plain torch on whatever device the state is on ------------------------------------------------------------------------------------------
    def state_dict(self):
        return dict(num_classes=self.num_classes, layers=self.layers, tokens=self.tokens, counts=self.counts.clone(),
                    per_class=self.per_class.clone(), loss_sum=self.loss_sum.clone())

    def load_state_dict(self, sd):
        if (int(sd["num_classes"]), int(sd["layers"]), int(sd["tokens"])) != (self.num_classes, self.layers, self.tokens):
            raise ValueError("StreamingEval state of (classes, layers, tokens) = (%d, %d, %d), this one has (%d, %d, %d)" % (
                sd["num_classes"], sd["layers"], sd["tokens"], self.num_classes, self.layers, self.tokens))
        self.counts.copy_(sd["counts"])
        self.per_class.copy_(sd["per_class"])
        self.loss_sum.copy_(sd["loss_sum"])
        return self

    def merge(self, other):
        """Add another shard's state (the state is additive)."""
        if (other.num_classes, other.layers, other.tokens) != (self.num_classes, self.layers, self.tokens):
            raise ValueError("StreamingEval.merge: the two states have different shapes")
        self.counts += other.counts.to(self.counts.device)
        self.per_class += other.per_class.to(self.per_class.device)
        self.loss_sum += other.loss_sum.to(self.loss_sum.device)
        return self

    def result(self, flops_dict=None, base_flops=None, topk=(1, 5)):
        """The state read once (one device -> host copy of each buffer): n, ignored, nan_rows, acc<k> for every k of ``topk`` (k <= 15),
        mean_per_class_acc, loss (mean over the rows that entered the sum), keep_ratio, keep_ratio_per_layer, and gflops when the FLOPs
        table is given.  The accuracies are the expressions of accuracy() / mean_per_class_accuracy() on exact counts: below 2^24 rows, their
        bits."""
        import _lib
        if any(int(k) < 1 or int(k) > _lib.EVAL_RANK_BINS - 1 for k in topk):
            raise ValueError("StreamingEval.result: topk within 1 ... %d (the rank histogram has %d bins)" % (_lib.EVAL_RANK_BINS - 1, _lib.EVAL_RANK_BINS))
        counts = self.counts.cpu()
        n, ignored, nan_rows, images = (int(counts[i]) for i in (_lib.EVAL_ROWS, _lib.EVAL_IGNORED, _lib.EVAL_NAN_ROWS, _lib.EVAL_MASK_ROWS))
        # the two accuracy expressions run where the state lives, as accuracy() / mean_per_class_accuracy() run where the gathered logits
        # live: the device's fp32 division need not round like the host's
        rank = self.counts[_lib.EVAL_OFF_RANK:_lib.EVAL_OFF_KEEP]
        out = dict(n=n, ignored=ignored, nan_rows=nan_rows)
        for k in topk:
            hits = rank[:min(int(k), self.num_classes)].sum().to(torch.float32)
            out["acc%d" % k] = (hits * 100.0 / n).item() if n else float("nan")
        total, hit = self.per_class[:self.num_classes], self.per_class[self.num_classes:]
        out["mean_per_class_acc"] = (hit / total.clamp(min=1).float() * 100).mean(0).item()
        scored = n - nan_rows
        out["loss"] = float(self.loss_sum.cpu()[0]) / scored if scored else float("nan")
        hist = counts[_lib.EVAL_OFF_KEEP:].view(self.layers, self.tokens + 1)
        kept = (hist * torch.arange(self.tokens + 1, dtype=torch.int64)).sum(1)          # kept tokens per layer, exact
        out["keep_ratio_per_layer"] = [int(k) / (images * self.tokens) if images else float("nan") for k in kept]
        out["keep_ratio"] = int(kept.sum()) / (images * self.layers * self.tokens) if images else float("nan")
        if flops_dict is not None and base_flops is not None and images:
            table = torch.as_tensor(flops_dict, dtype=torch.float64)[1:self.tokens + 2]        # entry c + 1: c kept tokens + the cls token
            out["gflops"] = float(base_flops) + float((hist.to(torch.float64) * table).sum()) / images
        return out
