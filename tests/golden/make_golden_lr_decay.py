#!/usr/bin/env python3
"""Generate tests/golden/lr_decay_groups.json: the parameter groups the REFERENCE's ``util/lr_decay.param_groups_lrd`` (:15-61, with
``get_layer_id_for_vit`` :64-76) returns on the REAL reference model after the freeze rule of main_image.py:250-256, for three models --
the depth-12 default, one with ``global_pool='avg'`` (trainable ``fc_norm``) and one with the adapter LayerNorm ("in") -- and
``layer_decay`` 0.75 and 1.0, with ``weight_decay`` 0.05 and the model's own ``no_weight_decay()`` list.  Recorded per group, in the
returned order: the parameter NAMES (the function returns the tensors; they are named through ``named_parameters()``), ``lr_scale`` and
``weight_decay``.  Same rules as make_golden.py: build container only, the model and the function are the reference's own code; what is
committed is the recorded result.  tests/test_param_groups_host.py compares our restatement (dynamic-tuning_amd/util/lr_decay.py) with it.
Usage:  python tests/golden/make_golden_lr_decay.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

synth = mg.synth
NUM_CLASSES, FFN_NUM, WEIGHT_DECAY = 100, 64, 0.05
LAYER_DECAYS = (0.75, 1.0)
MODELS = {"default": dict(), "avg_pool": dict(global_pool="avg"), "adapter_ln_in": dict(ln="in")}


def build(kw):
    kw = dict(kw)
    tuning = mg.EasyDict(ffn_adapt=True, ffn_option="parallel", ffn_adapter_layernorm_option=kw.pop("ln", "none"),
                         ffn_adapter_init_option="lora", ffn_adapter_scalar="0.1", ffn_num=FFN_NUM, d_model=768)
    model = mg.vit_base_patch16_224_in21k(num_classes=NUM_CLASSES, drop_path_rate=0.0, tuning_config=tuning,
                                          select_config=mg.EasyDict(open=True, keep_layers=0), **kw)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
    return model


def main():
    import util.lr_decay as ref_lrd
    assert os.path.realpath(ref_lrd.__file__).startswith(mg.REF), ref_lrd.__file__
    out = {"weight_decay": WEIGHT_DECAY, "num_classes": NUM_CLASSES, "ffn_num": FFN_NUM, "cases": []}
    for tag, kw in MODELS.items():
        model = build(kw)
        name_of = {id(p): n for n, p in model.named_parameters()}
        skip = sorted(model.no_weight_decay())
        for ld in LAYER_DECAYS:
            groups = ref_lrd.param_groups_lrd(model, WEIGHT_DECAY, no_weight_decay_list=model.no_weight_decay(), layer_decay=ld)
            rec = [dict(names=[name_of[id(p)] for p in g["params"]], lr_scale=g["lr_scale"], weight_decay=g["weight_decay"]) for g in groups]
            assert sum(len(g["names"]) for g in rec) == sum(1 for p in model.parameters() if p.requires_grad)
            out["cases"].append(dict(model=tag, layer_decay=ld, no_weight_decay_list=skip, trainable=sum(len(g["names"]) for g in rec),
                                     groups=rec))
            print("%s layer_decay %g: %d groups over %d tensors" % (tag, ld, len(rec), out["cases"][-1]["trainable"]))
    with open(os.path.join(HERE, "lr_decay_groups.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
