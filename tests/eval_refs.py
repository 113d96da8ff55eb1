"""Plain-torch reference of the streaming evaluation statistics (csrc/eval_stats.h, dyt_eval_rows / dyt_eval_keep): what the two HIP entries
compute, restated on whatever dtype the input has (fp64 for the truth, fp32 for the round-off floor of the format).  Pinned to
F.cross_entropy, util.metrics and the reference's goldens by tests/test_eval_refs_host.py."""
import torch

HEAD_WORDS, ROWS, IGNORED, NAN_ROWS, MASK_ROWS = 8, 0, 1, 2, 3
RANK_BINS, OFF_RANK, OFF_KEEP = 16, 8, 24


def counts_words(layers, tokens):
    return OFF_KEEP + layers * (tokens + 1)


def rows(logits, labels):
    """(rank int64 [n], loss [n] in the logits' dtype).  A label outside [0, C): rank -1, loss 0.  A row holding a NaN: rank C, loss 0.
    Otherwise rank = #{j : x_j > x_t} + #{j < t : x_j == x_t} and loss = -((x_t - max) - log(sum exp(x - max)))."""
    n, C = logits.shape
    labels = labels.long()
    ignored = (labels < 0) | (labels >= C)
    t = labels.clamp(0, C - 1)
    xt = logits.gather(1, t.view(n, 1))
    idx = torch.arange(C).view(1, C)
    rank = ((logits > xt) | ((logits == xt) & (idx < t.view(n, 1)))).sum(1)
    nan = torch.isnan(logits).any(1)
    mx = logits.max(1, keepdim=True).values
    loss = -((xt - mx) - torch.log(torch.exp(logits - mx).sum(1, keepdim=True)))[:, 0]
    rank = torch.where(nan, torch.full_like(rank, C), rank)
    rank = torch.where(ignored, torch.full_like(rank, -1), rank)
    loss = torch.where(nan | ignored, torch.zeros_like(loss), loss)
    return rank, loss


def fold(rank, loss, labels, classes, layers=12, tokens=196):
    """The state one dyt_eval_rows call adds: (counts int64 [counts_words], per_class int64 [2 C], loss_sum float64 scalar tensor)."""
    counts = torch.zeros(counts_words(layers, tokens), dtype=torch.int64)
    per_class = torch.zeros(2 * classes, dtype=torch.int64)
    labels = labels.long()
    live = rank >= 0
    nan = rank >= classes
    counts[ROWS] = int(live.sum())
    counts[IGNORED] = int((~live).sum())
    counts[NAN_ROWS] = int(nan.sum())
    counts[OFF_RANK:OFF_KEEP] = torch.bincount(rank[live].clamp(max=RANK_BINS - 1), minlength=RANK_BINS)
    per_class[:classes] = torch.bincount(labels[live], minlength=classes)
    per_class[classes:] = torch.bincount(labels[live & (rank == 0)], minlength=classes)
    return counts, per_class, loss[live & ~nan].double().sum()


def keep_hist(masks):
    """masks [n, L, T] (or [n, L, T, 1]) -> int64 [L, T + 1]: (image, layer) pairs by their number of non-zero entries."""
    if masks.dim() == 4:
        masks = masks[..., 0]
    n, L, T = masks.shape
    kept = (masks != 0).sum(-1)   # [n, L]
    return torch.stack([torch.bincount(kept[:, l], minlength=T + 1) for l in range(L)])


def keep_counts(masks):
    """The state one dyt_eval_keep call adds (counts int64 [counts_words(L, T)])."""
    h = keep_hist(masks)
    counts = torch.zeros(counts_words(h.shape[0], h.shape[1] - 1), dtype=torch.int64)
    counts[MASK_ROWS] = masks.shape[0]
    counts[OFF_KEEP:] = h.reshape(-1)
    return counts


def loss_bound(loss_f64, loss_f32_cpu):
    """The rule of DESIGN 7g with no constant of its own: (floor, bound) with floor = max|fp32_cpu - fp64| of this reference on the same
    input and bound = 4 floor + 4 ulp(max|fp64|)."""
    floor = float((loss_f32_cpu.double() - loss_f64).abs().max())
    top = float(loss_f64.abs().max())
    ulp = float(torch.nextafter(torch.tensor(top, dtype=torch.float32), torch.tensor(float("inf"))) - torch.tensor(top, dtype=torch.float32))
    return floor, 4.0 * floor + 4.0 * ulp
