#!/usr/bin/env python3
"""Generate tests/golden/misc_reference.json: what the reference's ``misc.py`` helpers produce on fixed inputs.

``observe(misc_module)`` drives ``SmoothedValue`` (statistics and rendered strings for the format strings the loops use),
``MetricLogger`` (update / add_meter / attribute access / str, and the lines ``log_every`` emits with the timings masked),
``get_grad_norm_`` and the single-process branches of the process-group helpers (reference misc.py:24-168,188-214,281-293,
355-363), all on inputs drawn from fixed seeds, and returns a JSON-able record.  Run as a script, it loads the REFERENCE's
misc.py (behind the third-party stand-ins of tests/driver_stubs.py) and writes that record; the JSON is data and is what
travels.  tests/test_driver_surface.py runs ``observe`` on this package's misc.py and compares it with the stored record.
The observation runs with no GPU visible to the module (``torch.cuda.is_available()`` False): ``log_every`` adds a
``max mem`` field when a GPU is present, and the record is the CPU one.
Usage:  python tests/golden/make_misc_reference.py <reference root>
"""
import builtins
import importlib.util
import io
import json
import logging
import os
import re
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "misc_reference.json")
FORMATS = ((20, None), (1, "{value:.6f}"), (10, "{avg:.4f}"), (5, "{median:.3f} / {max:.3f} / {global_avg:.5f}"))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def observe(mod):
    import torch
    torch.cuda.is_available = lambda: False
    rec = {}
    g = torch.Generator().manual_seed(0)
    vals = torch.rand(57, generator=g).tolist()
    rec["smoothed"] = []
    for win, fmt in FORMATS:
        a = mod.SmoothedValue(window_size=win, fmt=fmt)
        seq = []
        for i, v in enumerate(vals):
            a.update(v, n=1 + i % 3)
            seq.append([str(a), [a.median, a.avg, a.global_avg, a.max, a.value, a.count, a.total]])
        rec["smoothed"].append(seq)

    buf = io.StringIO()
    lg = logging.getLogger("observe_" + mod.__name__)
    lg.handlers[:] = [logging.StreamHandler(buf)]
    lg.setLevel(logging.INFO)
    lg.propagate = False
    ml = mod.MetricLogger(delimiter="  ", logger=lg)
    ml.add_meter("lr", mod.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    seen = []
    for i, x in enumerate(ml.log_every(list(range(7)), 3, "Epoch: [0]")):
        ml.update(loss=0.5 * x, lr=1e-3 * (x + 1), skip=None, t=torch.tensor(2.0 * x))
        seen.append(x)
    try:
        ml.nothing
        missing_raises = False
    except AttributeError:
        missing_raises = True
    rec["logger"] = {"seen": seen, "loss_count": ml.loss.count, "t_global_avg": ml.t.global_avg, "missing_meter_raises": missing_raises,
                     "lines": [re.sub(r"(eta|time|data|Total time): \S+( \(\S+ s / it\))?", r"\1: _", l) for l in buf.getvalue().splitlines()],
                     "str": str(ml)}

    ps = [torch.nn.Parameter(torch.randn(3, 4, generator=g)) for _ in range(4)]
    for p in ps[:3]:
        p.grad = torch.randn(3, 4, generator=g)
    rec["grad_norm"] = {str(nt): float(mod.get_grad_norm_(ps, nt)) for nt in (2.0, 1.0, float("inf"))}
    rec["grad_norm_no_grad"] = float(mod.get_grad_norm_([ps[3]]))
    rec["grad_norm_bare_tensor"] = float(mod.get_grad_norm_(ps[0]))

    keep = builtins.print
    a = types.SimpleNamespace(dist_on_itp=False, dist_url="env://")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SLURM_PROCID"):
        os.environ.pop(k, None)
    mod.init_distributed_mode(a)
    builtins.print = keep
    rec["process_group"] = {"world_size": mod.get_world_size(), "rank": mod.get_rank(), "is_main": mod.is_main_process(),
                            "dist_initialized": mod.is_dist_avail_and_initialized(), "all_reduce_mean": mod.all_reduce_mean(3.5),
                            "distributed": a.distributed}
    rec["scaler_state_dict_key"] = mod.NativeScalerWithGradNormCount.state_dict_key
    return rec


def main(ref):
    sys.path.insert(0, os.path.dirname(HERE))
    import driver_stubs
    driver_stubs.install()
    rec = observe(load(os.path.join(ref, "misc.py"), "ref_misc"))
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
