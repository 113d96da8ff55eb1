"""Parameter groups for fine-tuning with layer-wise learning-rate decay and no weight decay on 1-D tensors: what the reference's
util/lr_decay.py computes (``param_groups_lrd`` :15-61, ``get_layer_id_for_vit`` :64-76; the BEiT / ELECTRA recipe), restated.  For the
same model it returns the same groups in the same order with the same ``lr_scale`` / ``weight_decay`` / membership
(tests/golden/lr_decay_groups.json holds what the reference returned).  The groups go straight into ``torch.optim.AdamW(groups, lr=...)``;
``util.lr_sched.adjust_learning_rate`` multiplies every group's ``lr_scale`` in (reference util/lr_sched.py:16-20) and the fused step
updates all of them in one launch (engine_finetune.FusedAdamW, dyt_adamw_segments)."""


def get_layer_id_for_vit(name, num_layers):
    """Depth of a ViT parameter for the decay ladder (reference :64-76): the embedding (``cls_token``, ``pos_embed``, ``patch_embed.*``)
    is layer 0, ``blocks.<i>.*`` is layer i + 1, everything else (final norm, ``fc_norm``, head) is layer ``num_layers``."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=[], layer_decay=.75):
    """One group per (layer id, decayed or not) that has a trainable tensor, in the order ``model.named_parameters()`` first meets it
    (reference :15-61).  A tensor is NOT decayed when it is 1-D or named in ``no_weight_decay_list`` (:31-37); a group of layer id l has
    ``lr_scale = layer_decay ** (num_layers - l)`` with ``num_layers = len(model.blocks) + 1`` (:23-25), so the head trains at the full
    rate and block 0 at ``layer_decay ** depth`` of it."""
    num_layers = len(model.blocks) + 1
    scales = [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        plain = p.ndim == 1 or name in no_weight_decay_list
        layer = get_layer_id_for_vit(name, num_layers)
        key = "layer_%d_%s" % (layer, "no_decay" if plain else "decay")
        if key not in groups:
            groups[key] = {"lr_scale": scales[layer], "weight_decay": 0. if plain else weight_decay, "params": []}
        groups[key]["params"].append(p)
    return list(groups.values())
