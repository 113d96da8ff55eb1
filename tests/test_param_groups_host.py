"""Parameter groups of the fused AdamW, host side (no GPU): the C surface of dyt_adamw_segments, util/lr_decay against what the reference's
function returned (tests/golden/lr_decay_groups.json, recorded by tests/golden/make_golden_lr_decay.py), the segment-table builder, and the
optimizer state of a multi-group torch.optim.AdamW through FusedAdamW before any engine exists."""
import ctypes
import json
import os
import re

import pytest
import torch

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


class Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _model(ln="none", **kw):
    """tests/test_host.py::_model(), optionally with the adapter LayerNorm / further constructor arguments; the freeze rule applied."""
    from models.vision_transformer_IN21K import vit_base_patch16_224_in21k
    tuning = Cfg(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option=ln, ffn_adapter_init_option="lora",
                 ffn_adapter_scalar="0.1", ffn_num=kw.pop("ffn_num", 64), d_model=768)
    m = vit_base_patch16_224_in21k(num_classes=kw.pop("num_classes", 100), drop_path_rate=0.0, tuning_config=tuning,
                                   select_config=Cfg(open=True, keep_layers=0), **kw)
    for n, p in m.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return m


MODELS = {"default": dict(), "avg_pool": dict(global_pool="avg"), "adapter_ln_in": dict(ln="in")}


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = _model(**MODELS[tag])
        return cache[tag]
    return get


# ------------------------------------------------------------------------------------------------------------------------------
# surface
# ------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_declare_dyt_adamw_segments():
    import _lib
    hdr = open(os.path.join(ROOT, "include", "dyt_hip.h")).read()
    assert re.search(r"#define\s+DYT_ADAMW_MAX_SEGMENTS\s+128\b", hdr)
    assert re.search(r"typedef\s+struct\s*\{\s*int64_t\s+end;\s*float\s+lr;\s*float\s+weight_decay;\s*\}\s*dyt_adamw_segment\s*;", hdr)
    m = re.search(r"\bint\s+dyt_adamw_segments\s*\(([^)]*)\)\s*;", hdr)
    assert m, "dyt_adamw_segments is not declared"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert args == ["float* param", "const float* grad", "float* exp_avg", "float* exp_avg_sq", "int64_t numel", "int32_t* state", "int step",
                    "const dyt_adamw_segment* segments", "int num_segments", "float beta1", "float beta2", "float eps", "float grad_scale",
                    "void* stream"], args
    res, argtypes = _lib.SYMBOLS["dyt_adamw_segments"]
    assert res is ctypes.c_int and len(argtypes) == len(args) == 14
    assert argtypes[4] is ctypes.c_int64 and argtypes[6] is ctypes.c_int and argtypes[8] is ctypes.c_int
    assert all(argtypes[i] is ctypes.c_float for i in (9, 10, 11, 12))
    assert ctypes.sizeof(_lib.AdamwSegment) == 16 and _lib.AdamwSegment.lr.offset == 8 and _lib.AdamwSegment.weight_decay.offset == 12
    assert _lib.ADAMW_MAX_SEGMENTS == 128
    for L in (_lib.lib(), _lib.lib(fp16=True)):
        assert hasattr(L, "dyt_adamw_segments")
        assert L.dyt_version() == 5   # added without a version change: discovered by the symbol


def test_refusals_need_no_device():
    """The argument checks run before anything is enqueued, so they can be reached without a GPU (the pointers are never read)."""
    import _lib
    L = _lib.lib()
    if torch.cuda.is_available():   # where a device exists the pointers are real, so that a check that failed to refuse could harm nothing
        buf = torch.zeros(129, device="cuda:0")
        fake = ctypes.c_void_p(buf.data_ptr())
    else:
        fake = ctypes.c_void_p(4096)
    nope = ctypes.c_void_p(0)

    def call(table, numel=100, n=None, state=None, step=1):
        arr = _lib.adamw_segment_array(table) if table else (_lib.AdamwSegment * 1)()
        return L.dyt_adamw_segments(fake, fake, fake, fake, numel, state, step, ctypes.cast(arr, ctypes.c_void_p), len(table) if n is None else n,
                                    0.9, 0.999, 1e-8, 1.0, None)
    for table, n, what in (([], 0, "segments"), ([(i + 1, 1e-3, 0.0) for i in range(129)], None, "segments"),
                           ([(50, 1e-3, 0.0), (50, 1e-3, 0.0), (100, 1e-3, 0.0)], None, "increase"),
                           ([(60, 1e-3, 0.0), (40, 1e-3, 0.0), (100, 1e-3, 0.0)], None, "increase"),
                           ([(0, 1e-3, 0.0), (100, 1e-3, 0.0)], None, "increase"),
                           ([(50, 1e-3, 0.0), (99, 1e-3, 0.0)], None, "last"), ([(50, 1e-3, 0.0), (101, 1e-3, 0.0)], None, "last")):
        assert call(table, numel=129 if len(table) == 129 else 100, n=n) == -1, table[:3]
        assert what in L.dyt_last_error().decode(), (what, L.dyt_last_error())
    assert call([(100, 1e-3, 0.0)], step=0) == -1          # the unguarded form takes a 1-based step
    assert L.dyt_adamw_segments(nope, fake, fake, fake, 100, None, 1, ctypes.cast(_lib.adamw_segment_array([(100, 1e-3, 0.0)]), ctypes.c_void_p), 1,
                                0.9, 0.999, 1e-8, 1.0, None) == -1


# ------------------------------------------------------------------------------------------------------------------------------
# util/lr_decay against the reference's recorded result
# ------------------------------------------------------------------------------------------------------------------------------
def test_param_groups_lrd_returns_what_the_reference_returned(models):
    from util.lr_decay import get_layer_id_for_vit, param_groups_lrd
    gold = json.load(open(os.path.join(GOLDEN, "lr_decay_groups.json")))
    assert sorted({c["model"] for c in gold["cases"]}) == sorted(MODELS) and sorted({c["layer_decay"] for c in gold["cases"]}) == [0.75, 1.0]
    for case in gold["cases"]:
        m = models(case["model"])
        assert sorted(m.no_weight_decay()) == case["no_weight_decay_list"]
        name_of = {id(p): n for n, p in m.named_parameters()}
        groups = param_groups_lrd(m, gold["weight_decay"], no_weight_decay_list=m.no_weight_decay(), layer_decay=case["layer_decay"])
        tag = "%s layer_decay %g" % (case["model"], case["layer_decay"])
        assert len(groups) == len(case["groups"]) == 26, tag
        for g, ref in zip(groups, case["groups"]):
            assert sorted(g) == ["lr_scale", "params", "weight_decay"], tag
            assert [name_of[id(p)] for p in g["params"]] == ref["names"], tag
            assert g["lr_scale"] == ref["lr_scale"] and g["weight_decay"] == ref["weight_decay"], (tag, ref["names"][0])   # the same doubles
        assert sum(len(g["params"]) for g in groups) == case["trainable"] == sum(1 for n, _ in m.named_parameters() if synth.is_trainable(n))
        # what the recipe is for: 1-D tensors are not decayed, matrices are
        for g in groups:
            assert all((p.ndim == 1) == (g["weight_decay"] == 0.0) for p in g["params"]), tag
    assert [get_layer_id_for_vit(n, 13) for n in ("cls_token", "pos_embed", "patch_embed.proj.weight", "blocks.0.norm1.weight",
                                                   "blocks.11.adaptmlp.up_proj.bias", "norm.weight", "fc_norm.bias", "head.weight")] == [0, 0, 0, 1, 12, 13, 13, 13]
    # torch takes the groups as they are, and the schedule writes lr * lr_scale into each (reference util/lr_sched.py:16-20)
    import types
    import util.lr_sched as lr_sched
    m = models("default")
    opt = torch.optim.AdamW(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-3)
    lr = lr_sched.adjust_learning_rate(opt, 7.0, types.SimpleNamespace(lr=1e-3, min_lr=1e-6, warmup_epochs=5, epochs=100))
    assert all(g["lr"] == lr * g["lr_scale"] for g in opt.param_groups) and opt.param_groups[-1]["lr_scale"] == 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# the table builder
# ------------------------------------------------------------------------------------------------------------------------------
def _g(params, lr, wd, **kw):
    return dict(dict(params=list(params), lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8, amsgrad=False, maximize=False), **kw)


def test_segment_table_builder():
    from _lib import DyTError
    from engine_finetune import adamw_segment_table
    # six tensors; the flat buffer holds them in the order 3, 0, 4, 1, 5, 2 (positions are named_parameters order, offsets the library's)
    numel = [10, 1, 7, 300, 64, 5]
    order = [3, 0, 4, 1, 5, 2]
    slices, at = [None] * 6, 0
    for i in order:
        slices[i] = (at, numel[i])
        at += numel[i]
    ends = {i: slices[i][0] + slices[i][1] for i in range(6)}
    assert at == 387
    # one group, tensors given out of flat order: one segment over everything
    assert adamw_segment_table(slices, [_g([5, 2, 0, 1, 4, 3], 1e-3, 0.05)]) == [(387, 1e-3, 0.05)]
    # two groups that interleave in the flat buffer give alternating segments
    t = adamw_segment_table(slices, [_g([0, 1, 2], 1e-3, 0.0), _g([3, 4, 5], 2e-3, 0.05)])
    assert t == [(ends[3], 2e-3, 0.05), (ends[0], 1e-3, 0.0), (ends[4], 2e-3, 0.05), (ends[1], 1e-3, 0.0), (ends[5], 2e-3, 0.05), (ends[2], 1e-3, 0.0)]
    # equal neighbours merge, whatever group they come from: (3, 0) and (4, 1, 5) share their values; 2 stands alone
    t = adamw_segment_table(slices, [_g([0], 1e-3, 0.0), _g([3], 1e-3, 0.0), _g([5, 1], 0.0, 0.05), _g([4], 0.0, 0.05), _g([2], 1e-3, 0.05)])
    assert t == [(ends[0], 1e-3, 0.0), (ends[5], 0.0, 0.05), (387, 1e-3, 0.05)]
    # the table follows the groups' CURRENT values
    groups = [_g([0, 1, 2], 1e-3, 0.0, lr_scale=0.5), _g([3, 4, 5], 1e-3, 0.0)]
    assert adamw_segment_table(slices, groups) == [(387, 1e-3, 0.0)]
    groups[0]["lr"] = 5e-4
    assert len(adamw_segment_table(slices, groups)) == 6
    # a missing or doubled tensor, a foreign position
    for bad in ([_g([0, 1, 2], 1e-3, 0.0), _g([3, 4], 1e-3, 0.0)], [_g([0, 1, 2, 3], 1e-3, 0.0), _g([3, 4, 5], 1e-3, 0.0)],
                [_g([0, 1, 2, 3, 4, 5, 6], 1e-3, 0.0)]):
        with pytest.raises(NotImplementedError):
            adamw_segment_table(slices, bad)
    # shared hyper-parameters: refused by the key's name
    for key, value in (("betas", (0.9, 0.99)), ("eps", 1e-6), ("amsgrad", True), ("maximize", True)):
        with pytest.raises(NotImplementedError, match=key):
            adamw_segment_table(slices, [_g([0, 1, 2], 1e-3, 0.0), _g([3, 4, 5], 1e-3, 0.0, **{key: value})])
    # more distinct segments than the kernel's table holds
    many = [(i, 1) for i in range(130)]
    with pytest.raises(DyTError, match="128"):
        adamw_segment_table(many, [_g([i], 1e-3 * (1 + i % 2), 0.0) for i in range(130)])
    assert len(adamw_segment_table(many[:128], [_g([i], 1e-3 * (1 + i % 2), 0.0) for i in range(128)])) == 128
    # the library aligns its tensors: padding behind a tensor (and behind the last, up to the buffer's length) goes with that tensor
    assert adamw_segment_table([(0, 1), (4, 6)], [_g([0], 1e-3, 0.0), _g([1], 2e-3, 0.0)], total=12) == [(4, 1e-3, 0.0), (12, 2e-3, 0.0)]
    assert adamw_segment_table([(4, 6), (0, 1)], [_g([0], 1e-3, 0.0), _g([1], 2e-3, 0.0)]) == [(4, 2e-3, 0.0), (10, 1e-3, 0.0)]
    # tensors that overlap, or a buffer that does not begin with a tensor, are not a layout of the library's
    for bad in ([(0, 5), (4, 4)], [(1, 3), (4, 4)]):
        with pytest.raises(DyTError):
            adamw_segment_table(bad, [_g([0, 1], 1e-3, 0.0)])
    with pytest.raises(DyTError):
        adamw_segment_table([(0, 4), (4, 4)], [_g([0, 1], 1e-3, 0.0)], total=7)


def test_as_fused_adopts_any_split_of_the_trainable_tensors(models):
    from engine_finetune import FusedAdamW, as_fused
    from util.lr_decay import param_groups_lrd
    m = models("default")
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    ps = [p for _, p in named]
    opt = torch.optim.AdamW(param_groups_lrd(m, 0.05, m.no_weight_decay(), 0.75), lr=1e-3)
    fused = as_fused(opt, m)
    assert fused.param_groups is opt.param_groups and len(fused.param_groups) == 26 and as_fused(opt, m) is fused
    pos = fused.positions()
    assert sorted(i for idx in pos for i in idx) == list(range(74))
    assert [named[i][0] for i in pos[0]] == ["blocks.0.adaptmlp.down_proj.weight", "blocks.0.adaptmlp.up_proj.weight", "blocks.0.mlp_token_select.mlp_head.weight"]
    # one group in another order than named_parameters() is a split like any other
    assert as_fused(torch.optim.AdamW(ps[::-1], lr=1e-3), m).positions() == [list(range(73, -1, -1))]
    # a tensor missing, one held by two optimizers' worth of groups, a foreign tensor
    with pytest.raises(NotImplementedError):
        as_fused(torch.optim.AdamW([dict(params=ps[:40]), dict(params=ps[41:])], lr=1e-3), m)
    with pytest.raises(NotImplementedError):
        as_fused(torch.optim.AdamW([dict(params=ps[:40]), dict(params=ps[40:] + [torch.nn.Parameter(torch.zeros(3))])], lr=1e-3), m)
    with pytest.raises(NotImplementedError):
        FusedAdamW(m, params=[dict(params=ps[:40]), dict(params=ps[39:])])
    for key, kw in (("betas", dict(betas=(0.9, 0.99))), ("eps", dict(eps=1e-6)), ("amsgrad", dict(amsgrad=True)), ("maximize", dict(maximize=True))):
        with pytest.raises(NotImplementedError, match=key):
            as_fused(torch.optim.AdamW([dict(params=ps[:40]), dict(params=ps[40:], **kw)], lr=1e-3), m)
    # FusedAdamW built directly from group dicts fills torch's defaults in and keeps the groups' own keys
    f2 = FusedAdamW(m, params=[dict(params=ps[:40], weight_decay=0.0, lr_scale=0.5), dict(params=ps[40:])], lr=2e-3, weight_decay=0.05)
    assert [g["weight_decay"] for g in f2.param_groups] == [0.0, 0.05] and f2.param_groups[0]["lr_scale"] == 0.5
    assert all(g["lr"] == 2e-3 and g["betas"] == (0.9, 0.999) for g in f2.param_groups)
    assert FusedAdamW(m, lr=1e-3).param_groups[0]["params"] == list(range(74))


# ------------------------------------------------------------------------------------------------------------------------------
# state dict in torch's layout, before an engine exists
# ------------------------------------------------------------------------------------------------------------------------------
def test_three_group_state_dict_is_torch_adamw_layout(models):
    from engine_finetune import FusedAdamW
    m = models("default")
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    is_head = [n.startswith("head.") for n, _ in named]
    split = [[i for i in range(74) if not is_head[i] and named[i][1].ndim > 1], [i for i in range(74) if is_head[i]][::-1],
             [i for i in range(74) if not is_head[i] and named[i][1].ndim == 1]]
    assert [len(s) for s in split] == [36, 2, 36]
    twins = [torch.nn.Parameter(torch.zeros_like(p)) for _, p in named]

    def groups(ps):
        return [dict(params=[ps[i] for i in split[0]], weight_decay=0.05, lr_scale=0.75), dict(params=[ps[i] for i in split[1]], weight_decay=0.05, lr_scale=10.0),
                dict(params=[ps[i] for i in split[2]], weight_decay=0.0, lr_scale=0.75)]
    topt = torch.optim.AdamW(groups(twins), lr=3e-4)
    for g in topt.param_groups:
        g["lr"] = 3e-4 * g["lr_scale"]
    gen = torch.Generator().manual_seed(0)
    for _ in range(2):
        for p in twins:
            p.grad = torch.randn(p.shape, generator=gen)
        topt.step()
    sd = topt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [list(range(36)), [36, 37], list(range(38, 74))]
    opt = FusedAdamW(m, params=groups([p for _, p in named]), lr=1.0, weight_decay=0.5)
    opt.load_state_dict(sd)
    assert opt.step_count == 2
    assert [(g["lr"], g["weight_decay"], g["lr_scale"]) for g in opt.param_groups] == [(3e-4 * 0.75, 0.05, 0.75), (3e-4 * 10.0, 0.05, 10.0), (3e-4 * 0.75, 0.0, 0.75)]
    # the moments landed on the right tensors: running index r of the state is tensor split[...][...] of the model
    flat = [i for s in split for i in s]
    for r, i in enumerate(flat):
        assert torch.equal(opt._pending[named[i][0]]["exp_avg"], topt.state[twins[i]]["exp_avg"]), named[i][0]
    back = opt.state_dict()
    assert [g["params"] for g in back["param_groups"]] == [g["params"] for g in sd["param_groups"]] and len(back["state"]) == 74
    for a, b in zip(back["param_groups"], sd["param_groups"]):
        assert set(a) == set(b) and all(a[k] == b[k] for k in b if k != "betas") and tuple(a["betas"]) == tuple(b["betas"])
    for r in range(74):
        assert torch.equal(back["state"][r]["exp_avg"], sd["state"][r]["exp_avg"]) and torch.equal(back["state"][r]["exp_avg_sq"], sd["state"][r]["exp_avg_sq"])
        assert float(back["state"][r]["step"]) == 2.0
    topt2 = torch.optim.AdamW(groups(twins), lr=1.0)
    topt2.load_state_dict(back)   # torch accepts what we write
    assert [g["lr_scale"] for g in topt2.param_groups] == [0.75, 10.0, 0.75] and topt2.param_groups[1]["lr"] == 3e-4 * 10.0
    assert torch.equal(topt2.state[twins[split[1][0]]]["exp_avg"], topt.state[twins[split[1][0]]]["exp_avg"])
    # a group-count or group-size mismatch stays a ValueError
    one = torch.optim.AdamW(twins, lr=1e-3).state_dict()
    with pytest.raises(ValueError):
        opt.load_state_dict(one)
    with pytest.raises(ValueError):
        opt.load_state_dict({"state": {}, "param_groups": [{"params": list(range(35))}, {"params": [35, 36, 37]}, {"params": list(range(38, 74))}]})
    with pytest.raises(ValueError):
        FusedAdamW(m).load_state_dict(sd)
