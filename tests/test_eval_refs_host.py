"""CPU tests that pin tests/eval_refs.py -- the plain-torch statement of what dyt_eval_rows / dyt_eval_keep compute -- to F.cross_entropy,
util.metrics, the reference's eval_acc.npz golden and block_flops_dict.batch_select_flops, and that drive util.metrics.StreamingEval's torch
side (merge, state_dict, result, all_reduce over gloo) on states built by the reference.  Nothing here needs a GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import eval_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _state(logits, labels, masks=None, layers=12, tokens=196):
    """A CPU StreamingEval holding what the two entries would have accumulated for this data (built by the reference)."""
    from util.metrics import StreamingEval
    C = logits.shape[1]
    st = StreamingEval(C, layers=layers, tokens=tokens, device="cpu")
    rank, loss = R.rows(logits.double(), labels)
    counts, pc, ls = R.fold(rank, loss, labels, C, layers, tokens)
    st.counts += counts
    st.per_class += pc
    st.loss_sum += ls
    if masks is not None:
        st.counts += R.keep_counts(masks)
    return st


# ---- the reference against torch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2, 5, 100, 1025, 21843])
def test_loss_is_cross_entropy_in_fp64(C):
    g = torch.Generator().manual_seed(C)
    x = (torch.randn(9, C, generator=g) * 30.0).double()
    x[1] += 1e4
    x[2] -= 1e4
    y = torch.randint(0, C, (9,), generator=g)
    if C > 2:
        off = torch.rand(C, generator=g) < 0.5
        off[int(y[3])] = False
        x[3, off] = float("-inf")
    _, loss = R.rows(x, y)
    want = F.cross_entropy(x, y, reduction="none")
    assert float((loss - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert loss.dtype == torch.float64 and R.rows(x.float(), y)[1].dtype == torch.float32


@pytest.mark.parametrize("C,n", [(2, 64), (10, 257), (1000, 65), (21843, 33)])
def test_rank_is_accuracy_on_tie_free_rows(C, n):
    from util.metrics import accuracy, mean_per_class_accuracy
    g = torch.Generator().manual_seed(C + n)
    x = torch.stack([torch.randperm(C, generator=g) for _ in range(n)]).float() * 0.25 - 100.0   # tie-free by construction
    assert all(len(torch.unique(r)) == C for r in x[:8])
    y = torch.randint(0, C, (n,), generator=g)
    y[: n // 3] = x[: n // 3].argmax(1)   # a good share of hits
    rank, _ = R.rows(x, y)
    st = _state(x, y)
    res = st.result(topk=(1, 5))
    a1, a5 = accuracy(x, y, topk=(1, 5))
    assert res["acc1"] == a1.item() and res["acc5"] == a5.item()
    assert res["mean_per_class_acc"] == mean_per_class_accuracy(x, y, C).item()
    assert int((rank == 0).sum()) == int((x.argmax(1) == y).sum()) and res["n"] == n and res["ignored"] == 0 and res["nan_rows"] == 0
    for k in (1, 2, 3, 7, 15):
        assert st.result(topk=(k,))["acc%d" % k] == accuracy(x, y, topk=(k,))[0].item()
    with pytest.raises(ValueError):
        st.result(topk=(16,))


def test_rank_semantics_on_ties_nan_and_ignored_labels():
    x = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.0, 1.0, 1.0, 0.0], [2.0, 1.0, 3.0, 1.0], [0.0, float("nan"), 0.0, 0.0], [0.0, 1.0, 2.0, 3.0],
                      [0.0, 1.0, 2.0, 3.0], [0.0, float("-inf"), float("-inf"), 0.0]])
    y = torch.tensor([0, 2, 3, 0, -1, 4, 3])
    rank, loss = R.rows(x.double(), y)
    assert rank.tolist() == [0, 2, 3, 4, -1, -1, 1]   # the lowest index wins a tie; a NaN row ranks C; outside [0, C) is ignored
    assert loss[3] == 0 and loss[4] == 0 and loss[5] == 0 and abs(float(loss[6]) - float(np.log(2.0))) < 1e-15
    counts, pc, ls = R.fold(rank, loss, y, 4)
    assert counts[:4].tolist() == [5, 2, 1, 0]
    assert counts[R.OFF_RANK:R.OFF_KEEP].tolist() == [1, 1, 1, 1, 1] + [0] * 11   # C = 4: the NaN row's rank 4 has its own bin below 15
    assert pc.tolist() == [2, 0, 1, 2, 1, 0, 0, 0]
    assert abs(float(ls) - float(loss[[0, 1, 2, 6]].sum())) < 1e-15
    big = torch.zeros(3, 40)
    big[0, :20] = 1.0      # label 30: 20 ahead + 30 - 20 ties in front of it
    big[1, 5] = float("nan")
    rank, loss = R.rows(big.double(), torch.tensor([30, 2, 0]))
    assert rank.tolist() == [30, 40, 0]
    assert R.fold(rank, loss, torch.tensor([30, 2, 0]), 40)[0][R.OFF_RANK:R.OFF_KEEP].tolist() == [1] + [0] * 14 + [2]


def test_the_reference_golden_eval_acc():
    """eval_acc.npz: the reference's own ranks, and its accuracies to the bars of tests/test_gpu_round2.py -- met to the last fp32 bit."""
    g = dict(np.load(os.path.join(GOLDEN, "eval_acc.npz")))
    x, y = torch.from_numpy(g["logits"]).float(), torch.from_numpy(g["targets"]).long()
    rank, _ = R.rows(x, y)
    assert np.array_equal(rank.numpy(), g["ranks"].astype(np.int64))
    res = _state(x, y).result()
    assert abs(res["acc1"] - float(g["metric_accuracy"])) < 1e-5 and abs(res["acc5"] - float(g["acc5"])) < 1e-5
    assert abs(res["mean_per_class_acc"] - float(g["metric_mean_per_class_acc"])) < 1e-4
    assert np.float32(res["acc1"]) == np.float32(g["metric_accuracy"]) and np.float32(res["acc5"]) == np.float32(g["acc5"])
    assert np.float32(res["mean_per_class_acc"]) == np.float32(g["metric_mean_per_class_acc"])


@pytest.mark.parametrize("n", [1, 7, 64])
def test_gflops_and_keep_ratio_against_batch_select_flops(n):
    from block_flops_dict import BASE_FLOPS_IN21K, batch_select_flops, get_block_flops
    g = torch.Generator().manual_seed(n)
    masks = (torch.rand(n, 12, 196, 1, generator=g) < torch.rand(n, 12, 1, 1, generator=g)).float()
    table = get_block_flops(ffn_num=64)
    want = float(batch_select_flops(n, table, masks, block_num=12, base_flops=BASE_FLOPS_IN21K).mean())
    x = torch.randn(n, 10, generator=g)
    res = _state(x, torch.zeros(n, dtype=torch.int64), masks).result(flops_dict=table, base_flops=BASE_FLOPS_IN21K)
    assert abs(res["gflops"] - want) <= 16 * 2.0 ** -24 * want, (res["gflops"], want)   # fp32 storage of each element plus an fp32 mean
    assert abs(res["keep_ratio"] - float(masks.double().mean())) < 1e-15
    per_layer = masks[..., 0].double().mean(dim=(0, 2))
    assert len(res["keep_ratio_per_layer"]) == 12 and max(abs(a - float(b)) for a, b in zip(res["keep_ratio_per_layer"], per_layer)) < 1e-15
    h = R.keep_hist(masks)
    assert h.shape == (12, 197) and int(h.sum()) == 12 * n and torch.equal(h, R.keep_hist(masks[..., 0]))
    assert "gflops" not in _state(x, torch.zeros(n, dtype=torch.int64), masks).result()


# ---- StreamingEval's torch side -----------------------------------------------------------------------------------------------------------
def _data(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * 3.0
    y = torch.randint(0, C, (n,), generator=g)
    y[0], x[1, 2] = -1, float("nan")
    masks = (torch.rand(n, 12, 196, generator=g) < 0.6).float()
    return x, y, masks


def test_two_shards_merged_equal_the_whole():
    x, y, m = _data(23, 7, 3)
    whole = _state(x, y, m)
    a, b = _state(x[:9], y[:9], m[:9]), _state(x[9:], y[9:], m[9:])
    a.merge(b)
    assert torch.equal(a.counts, whole.counts) and torch.equal(a.per_class, whole.per_class)
    assert abs(float(a.loss_sum) - float(whole.loss_sum)) <= 23 * 2.0 ** -52 * abs(float(whole.loss_sum)) * 4
    ra, rw = a.result(), whole.result()
    assert {k: v for k, v in ra.items() if k != "loss"} == {k: v for k, v in rw.items() if k != "loss"}
    assert abs(ra["loss"] - rw["loss"]) < 1e-12 and rw["n"] == 22 and rw["ignored"] == 1 and rw["nan_rows"] == 1
    from util.metrics import StreamingEval
    c = StreamingEval(7, device="cpu").load_state_dict(whole.state_dict())
    assert torch.equal(c.counts, whole.counts) and torch.equal(c.loss_sum, whole.loss_sum) and c.result() == rw
    sd = whole.state_dict()
    sd["counts"] += 1
    assert not torch.equal(sd["counts"], whole.counts)   # state_dict hands out copies
    with pytest.raises(ValueError):
        StreamingEval(8, device="cpu").load_state_dict(whole.state_dict())
    with pytest.raises(ValueError):
        StreamingEval(7, layers=3, device="cpu").merge(whole)
    want = F.cross_entropy(x.double(), y.clamp(min=0), reduction="none")
    live = torch.ones(23, dtype=torch.bool)
    live[0] = live[1] = False
    assert abs(rw["loss"] - float(want[live].mean())) < 1e-12   # the mean over the rows that entered the sum


def test_result_of_an_empty_state_and_the_keys():
    from util.metrics import StreamingEval
    res = StreamingEval(5, device="cpu").result()
    assert res["n"] == 0 and res["ignored"] == 0 and all(np.isnan(res[k]) for k in ("acc1", "acc5", "loss", "keep_ratio"))
    x, y, m = _data(6, 5, 1)
    res = _state(x, y, m).result()
    assert set(res) == {"n", "ignored", "nan_rows", "acc1", "acc5", "mean_per_class_acc", "loss", "keep_ratio", "keep_ratio_per_layer"}


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "dynamic-tuning_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, y, m = _data(23, 7, 3)
    sl = slice(0, 9) if rank == 0 else slice(9, 23)
    st = _state(x[sl], y[sl], m[sl]).all_reduce()
    q.put((rank, st.state_dict(), st.result()))
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_world2_gloo():
    """Ragged shards (9 and 14 rows): after all_reduce every rank holds the state of the whole set."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict((r, (sd, out)) for r, sd, out in (q.get(timeout=120) for _ in procs))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    x, y, m = _data(23, 7, 3)
    whole = _state(x, y, m)
    for r in (0, 1):
        sd, out = res[r]
        assert torch.equal(sd["counts"], whole.counts) and torch.equal(sd["per_class"], whole.per_class)
        assert abs(float(sd["loss_sum"]) - float(whole.loss_sum)) < 1e-12
        assert out["acc1"] == whole.result()["acc1"] and out["keep_ratio"] == whole.result()["keep_ratio"]
    assert torch.equal(res[0][0]["loss_sum"], res[1][0]["loss_sum"])
